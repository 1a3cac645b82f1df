"""Grouped folds and lags at 100 M rows (DESIGN §4b "grouped"): pandrs_hip_grouped (CUM_SUM, CUM_MAX, CUM_MIN, CUM_COUNT,
ROW_NUMBER, SHIFT, DIFF, PCT_CHANGE at periods 1) on one device-resident f64 column, random normal, over the groups of one i64 key
column: uniform over 1 M, 1 K and 100 M (all distinct) values in random row order, and 1 M values in sorted row order.  All in one
process, per key shape:
  (a) pandrs_hip_groupby_indices alone (the grouping every grouped call reuses)
  (b) each grouped op after it: the op's own cost
  (c) torch's gather x[rows] and scatter out[rows] = x of the same 100 M f64 through the same rows[] permutation
  (d) pandrs_hip_cumulative (SUM) of the column     (e) a device copy (torch.clone)
Reported per op: (b) / ((c) gather + (c) scatter).  A grouped op has to gather the column through rows[] and scatter its result
back, so that sum is its floor by random accesses; an implementation that gathered the column a second time would sit near
(2 gather + scatter) / (gather + scatter) of it.  The gate: every fold's and every lag's ratio (median) stays below that figure.
The script exits 1 otherwise, and the JSON says which.

First every shape's CUM_SUM is checked at the groups' last rows against torch's index_add_ of the same cells.  Then, after
warm-up, --reps rounds (at least 10) time every call once per round with device events, so the repeats of the calls alternate.
  python experiments/grouped_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

OPS = (("cumsum", L.GROUPED_CUM_SUM), ("cummax", L.GROUPED_CUM_MAX), ("cummin", L.GROUPED_CUM_MIN), ("cumcount", L.GROUPED_CUM_COUNT),
       ("row_number", L.GROUPED_ROW_NUMBER), ("shift", L.GROUPED_SHIFT), ("diff", L.GROUPED_DIFF), ("pct_change", L.GROUPED_PCT_CHANGE))
INT_OPS = (L.GROUPED_CUM_COUNT, L.GROUPED_ROW_NUMBER)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {"min": min(v), "median": float(np.median(v)), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "grouped_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n, reps = a.rows, max(a.reps, 10)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    out_i = torch.empty(n, dtype=torch.int64, device=dev)
    out_mask = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    shapes = (("1 M groups", lambda: torch.randint(0, min(n, 1_000_000), (n,), dtype=torch.int64, device=dev, generator=g)),
              ("1 K groups", lambda: torch.randint(0, 1_000, (n,), dtype=torch.int64, device=dev, generator=g)),
              ("every row its own group", lambda: torch.randperm(n, dtype=torch.int64, device=dev, generator=g)),
              ("1 M groups, sorted keys", lambda: torch.sort(torch.randint(0, min(n, 1_000_000), (n,), dtype=torch.int64, device=dev, generator=g))[0]))
    ok, results = True, []
    for shape, make in shapes:
        key = make()
        kcol = [(key, None, L.I64)]
        _, _, off, rows = ctx.groupby_indices(kcol, n)                      # the CSR on the device; the grouping stays retained
        n_groups = int(off.numel()) - 1
        # ---- check: the running sum at every group's last row is the group's sum ----
        got = ctx.grouped((x, None, L.F64), n, L.GROUPED_CUM_SUM, out=out)[0]
        last = rows[off[1:] - 1]
        gkey = key[last]
        ref = torch.zeros(int(key.max()) + 1, dtype=torch.float64, device=dev).index_add_(0, key, x)[gkey]
        mag = torch.zeros(int(key.max()) + 1, dtype=torch.float64, device=dev).index_add_(0, key, x.abs())[gkey]
        size = (off[1:] - off[:-1]).to(torch.float64)
        worst = float(((got[last] - ref).abs() / (2.0 * size * 2.0 ** -53 * mag).clamp_min(1e-300)).max())
        del last, gkey, ref, mag, size, got
        col = (x, None, L.F64)
        calls = {"copy": lambda: torch.clone(x), "cumulative_sum": lambda: ctx.cumulative(col, n, L.CUM_SUM, out=out),
                 "torch_gather": lambda: torch.index_select(x, 0, rows, out=out), "torch_scatter": lambda: out.index_copy_(0, rows, x)}
        for label, op in OPS:
            calls[label] = lambda op=op: ctx.grouped(None if op == L.GROUPED_ROW_NUMBER else col, n, op, 1, out=out_i if op in INT_OPS else out,
                                                     out_mask=out_mask)
        for _ in range(2):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        ms["groupby_indices"] = []
        for r in range(reps):                                               # one repeat of every call per round: the repeats alternate
            for k, fn in calls.items():
                ms[k].append(once(fn))
            if r % 2 == 0:                                                  # regrouping alternates with them too
                ms["groupby_indices"].append(once(lambda: ctx.groupby_indices_compute(kcol, n)))
        r = {"shape": shape, "rows": n, "groups": n_groups, "sum_error_over_bound": worst}
        for k, v in ms.items():
            r[k + "_ms"] = stats(v)
        floor = r["torch_gather_ms"]["median"] + r["torch_scatter_ms"]["median"]
        r["gather_plus_scatter_ms"] = floor
        r["two_gathers_would_be"] = (2 * r["torch_gather_ms"]["median"] + r["torch_scatter_ms"]["median"]) / floor
        for label, op in OPS:
            r[label + "_over_gather_plus_scatter"] = r[label + "_ms"]["median"] / floor
        r["gate"] = {label: r[label + "_over_gather_plus_scatter"] < r["two_gathers_would_be"] for label, op in OPS if op != L.GROUPED_ROW_NUMBER}
        ok = ok and worst <= 1.0 and all(r["gate"].values())
        print(json.dumps(r), flush=True)
        results.append(r)
        del key, off, rows
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": reps, "gate": ok, "results": results}, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
