"""Cumulative folds and lags at 100 M rows (DESIGN §4b "cumulative"): pandrs_hip_cumulative (SUM, PROD, MAX, MIN, COUNT) and
pandrs_hip_lag (SHIFT, DIFF, PCT_CHANGE at periods 1, 2, 1001 and 10^6) on one device-resident f64 column, random normal, as it
is and with 10 % null bits, against pandrs_hip_window's expanding sum and expanding max on the same column (the kernels the
scan replaces for running totals), torch.cumsum, torch.cummax and a device copy (torch.clone), all in one process.  By bytes a
scan reads the column twice and writes it once, 24 bytes per row against the copy's 16 (1.5 x); a lag reads and writes once.

First the 100 M-row SUM is checked against torch.cumsum within 2 gamma_n sum|x| and MAX bit for bit against torch.cummax.
Then, after warm-up, --reps rounds (at least 20) time every call once per round with device events, so the repeats of the
calls alternate.  The gate: the slowest repeat of cumsum is faster than the fastest repeat of expanding sum, and the same for
cummax against expanding max; the script exits 1 otherwise.
  python experiments/cumulative_bench.py [--rows N] [--reps R] [--out FILE]
The per-kernel split comes from a separate run under rocprofv3 --kernel-trace --stats (--reps 3)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

CUM = (("cumsum", L.CUM_SUM), ("cumprod", L.CUM_PROD), ("cummax", L.CUM_MAX), ("cummin", L.CUM_MIN), ("cumcount", L.CUM_COUNT))
LAG = (("shift", L.LAG_SHIFT), ("diff", L.LAG_DIFF), ("pct_change", L.LAG_PCT_CHANGE))
PERIODS = (1, 2, 1001, 1_000_000)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def check(ctx, x, n, out):
    """SUM within the derived bound of torch.cumsum (another association of the same sum), MAX bit for bit."""
    got = ctx.cumulative((x, None, L.F64), n, L.CUM_SUM, out=out)[0]
    ref = torch.cumsum(x, 0)
    k = torch.arange(1, n + 1, dtype=torch.float64, device=x.device)
    u = 2.0 ** -53
    bound = 2.0 * (k * u / (1.0 - k * u)) * torch.cumsum(x.abs(), 0)
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    del ref, k, bound
    got = ctx.cumulative((x, None, L.F64), n, L.CUM_MAX, out=out)[0]
    same = bool(torch.equal(got.view(torch.int64), torch.cummax(x, 0)[0].view(torch.int64)))
    return worst, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "cumulative_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    bits = torch.rand(n, device=dev, generator=g) < 0.1
    pad = (-n) % 8
    mask = (torch.cat([bits, bits.new_zeros(pad)]).view(-1, 8).to(torch.uint8) << torch.arange(8, device=dev, dtype=torch.uint8)).sum(1).to(torch.uint8)
    del bits
    out = torch.empty(n, dtype=torch.float64, device=dev)
    out_i = torch.empty(n, dtype=torch.int64, device=dev)
    out_mask = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    worst, same = check(ctx, x, n, out)
    print(json.dumps({"sum_error_over_bound": worst, "max_bit_for_bit": same}), flush=True)
    ok = worst <= 1.0 and same
    results = []
    for shape, m in (("as is", None), ("10 % null bits", mask)):
        col = (x, m, L.F64)
        calls = {"copy": lambda: torch.clone(x), "torch_cumsum": lambda: torch.cumsum(x, 0), "torch_cummax": lambda: torch.cummax(x, 0),
                 "expanding_sum": lambda: ctx.window(col, n, L.WINDOW_KIND_EXPANDING, L.WINDOW_SUM, min_periods=1),
                 "expanding_max": lambda: ctx.window(col, n, L.WINDOW_KIND_EXPANDING, L.WINDOW_MAX, min_periods=1)}
        for label, op in CUM:
            calls[label] = lambda op=op: ctx.cumulative(col, n, op, out=out_i if op == L.CUM_COUNT else out, out_mask=out_mask)
        for label, op in LAG:
            for p in PERIODS:
                calls["%s_%d" % (label, p)] = lambda op=op, p=p: ctx.lag(col, n, op, p, out=out, out_mask=out_mask)
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(max(a.reps, 20)):                        # one repeat of every call per round: the repeats alternate
            for k, fn in calls.items():
                ms[k].append(once(fn))
        r = {"shape": shape, "rows": n}
        for k, v in ms.items():
            r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
        for k in ms:
            if k not in ("copy", "torch_cumsum", "torch_cummax", "expanding_sum", "expanding_max"):
                r[k + "_over_copy"] = r[k + "_ms"]["median"] / r["copy_ms"]["median"]
        r["cumsum_over_torch"] = r["cumsum_ms"]["median"] / r["torch_cumsum_ms"]["median"]
        r["cummax_over_torch"] = r["cummax_ms"]["median"] / r["torch_cummax_ms"]["median"]
        r["gate_cumsum"] = r["cumsum_ms"]["max"] < r["expanding_sum_ms"]["min"]
        r["gate_cummax"] = r["cummax_ms"]["max"] < r["expanding_max_ms"]["min"]
        ok = ok and r["gate_cumsum"] and r["gate_cummax"]
        print(json.dumps(r), flush=True)
        results.append(r)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": max(a.reps, 20), "sum_error_over_bound": worst,
                   "max_bit_for_bit": same, "gate": ok, "results": results}, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
