"""Derived columns at 100 M rows (DESIGN §4b "eval"): pandrs_hip_eval on device-resident f64 columns, random normal, all in one
process.  What each case is compared against:
  (a) one column, one op (x + 1.5)        a device copy (torch.clone) and pandrs_hip_lag SHIFT: one read and one write of 8 bytes per row each
  (b) a * b                               the copy scaled by bytes: 24 against 16 per row
  (c) a * b + c in one call               the same result from two calls, a * b then + c: 32 bytes per row against 48
  (d) a > b && c < 0 (a boolean program)  pandrs_hip_predicate GT on one column
First (c) is checked bit for bit against the two-call result and against torch (a * b, then + c: two roundings), and (d) against
torch.  Then, after warm-up, --reps rounds (at least 20) time every call once per round with device events, so the repeats of the
calls alternate.  Beside the time of the whole call (what the gates compare) the library's own device events are recorded
(`*_device_ms`): the difference is what the host spends around the kernels.
Gate 1: the median of (c) in one call is below the median of (c) in two calls (fusing saves a third of the bytes; anything else
means the interpreter, not memory, is the limit).  Gate 2: the median of (a) is no more than the lag stream's median plus the
spread (max - min) of the lag stream's own repeats.  The script exits 1 when a gate or a check fails.
  python experiments/eval_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

ADD_SCALAR = [(L.EVAL_COL, 0), (L.EVAL_CONST, 1.5), (L.EVAL_ADD, 0)]
MUL = [(L.EVAL_COL, 0), (L.EVAL_COL, 1), (L.EVAL_MUL, 0)]
ADD = [(L.EVAL_COL, 0), (L.EVAL_COL, 1), (L.EVAL_ADD, 0)]
FUSED = [(L.EVAL_COL, 0), (L.EVAL_COL, 1), (L.EVAL_MUL, 0), (L.EVAL_COL, 2), (L.EVAL_ADD, 0)]
COND = [(L.EVAL_COL, 0), (L.EVAL_COL, 1), (L.EVAL_GT, 0), (L.EVAL_COL, 2), (L.EVAL_CONST, 0.0), (L.EVAL_LT, 0), (L.EVAL_AND, 0)]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x, y, z = (torch.randn(n, dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    cx, cy, cz = (x, None, L.F64), (y, None, L.F64), (z, None, L.F64)
    out, tmp = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    out_mask = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    bits = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)

    def two_calls():
        ctx.eval([cx, cy], n, MUL, out=tmp, out_mask=out_mask)
        ctx.eval([(tmp, None, L.F64), cz], n, ADD, out=out, out_mask=out_mask)

    # ---- the checks: one call, two calls and torch agree bit for bit ----
    ctx.eval([cx, cy, cz], n, FUSED, out=out, out_mask=out_mask)
    fused = out.clone()
    two_calls()
    ref = x * y
    ref += z
    same_two = bool(torch.equal(fused.view(torch.int64), out.view(torch.int64)))
    same_torch = bool(torch.equal(fused.view(torch.int64), ref.view(torch.int64)))
    del fused, ref
    _, count = ctx.eval([cx, cy, cz], n, COND, out=bits)
    want = int(((x > y) & (z < 0)).sum())
    checks = {"fused_equals_two_calls": same_two, "fused_equals_torch": same_torch, "cond_count": count, "cond_count_torch": want}
    print(json.dumps(checks), flush=True)
    ok = same_two and same_torch and count == want

    calls = {"copy": lambda: torch.clone(x),
             "lag_shift_1": lambda: ctx.lag(cx, n, L.LAG_SHIFT, 1, out=out, out_mask=out_mask),
             "predicate_gt": lambda: ctx.predicate(cx, n, L.PRED_GT, 0.0, out=bits),
             "a_add_scalar": lambda: ctx.eval([cx], n, ADD_SCALAR, out=out, out_mask=out_mask),
             "b_mul": lambda: ctx.eval([cx, cy], n, MUL, out=out, out_mask=out_mask),
             "c_fused": lambda: ctx.eval([cx, cy, cz], n, FUSED, out=out, out_mask=out_mask),
             "c_two_calls": two_calls,
             "d_cond": lambda: ctx.eval([cx, cy, cz], n, COND, out=bits)}
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    dev_ms = {k: [] for k in calls if k not in ("copy", "c_two_calls")}
    for _ in range(max(a.reps, 20)):                            # one repeat of every call per round: the repeats alternate
        for k, fn in calls.items():
            ms[k].append(once(fn))
            if k in dev_ms:                                     # the library's own device events around the call's kernels
                dev_ms[k].append(ctx.timings()["total_ms"])
    r = {"rows": n}
    for k, v in ms.items():
        r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    for k, v in dev_ms.items():
        r[k + "_device_ms"] = float(np.median(v))
    med = lambda k: r[k + "_ms"]["median"]                      # noqa: E731
    r["a_over_copy"] = med("a_add_scalar") / med("copy")
    r["a_over_lag"] = med("a_add_scalar") / med("lag_shift_1")
    r["b_over_copy"] = med("b_mul") / med("copy")               # by bytes: 24 / 16 = 1.5
    r["c_fused_over_two_calls"] = med("c_fused") / med("c_two_calls")       # by bytes: 32 / 48 = 0.67
    r["d_over_predicate"] = med("d_cond") / med("predicate_gt")             # by bytes: 24.125 / 8.125 = 2.97
    r["lag_spread_ms"] = r["lag_shift_1_ms"]["max"] - r["lag_shift_1_ms"]["min"]
    r["a_spread_ms"] = r["a_add_scalar_ms"]["max"] - r["a_add_scalar_ms"]["min"]
    r["gate_1_fused_faster_than_two_calls"] = med("c_fused") < med("c_two_calls")
    r["gate_2_add_scalar_no_slower_than_lag"] = med("a_add_scalar") <= med("lag_shift_1") + r["lag_spread_ms"]
    ok = ok and r["gate_1_fused_faster_than_two_calls"] and r["gate_2_add_scalar_no_slower_than_lag"]
    print(json.dumps(r), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": max(a.reps, 20), "checks": checks, "gate": ok, "result": r}, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
