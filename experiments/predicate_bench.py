"""Row masks at 100 M rows (DESIGN §4b "predicate"): pandrs_hip_predicate (GT, BETWEEN, ISNA on f64 and i64, with and without a
null mask) and pandrs_hip_isin (3, 100, the LDS limit, 10^5 and 10^7 values; random 64-bit patterns and integral f64; hit rates
near 0 and near 1), against the yardsticks measured in the same process on the same columns: pandrs_hip_arg_extreme (the
library's one-pass read-only stream over the same bytes, with more work per row), a device copy of the column,
pandrs_hip_join_indices (INNER) of the column against the same list (the route to a semi-join before isin existed), and torch's
`t > v` and torch.isin.

Device-resident columns; after warm-up, the median of --reps calls with the smallest and largest beside it.  Timing is a pair
of torch.cuda.Events on torch's current stream around each call.  The library runs on its own stream and synchronises it before a
call returns, so for a library call the interval is the call's wall time as the host sees it (launches, the kernels, the 8-byte
count read-back and the sync), not device time alone; for torch's own ops (`t > v`, `copy_`, `torch.isin`) it is device time on
that stream.  The ratios to torch therefore carry the library's host overhead on the library's side only.
The I64 compare is also timed with "predicate_path" 1 (every cell converted with (double)v in the loop) beside the default (the
integer interval bisected on the host): the A/B that decides which of the two the library keeps.
Gates, reported as held or not:
  1. every compare predicate's median <= arg_extreme's median x (1 + (max - min) / median of arg_extreme's own repetitions);
     (max - min) of a handful of repetitions is a noisy width: the default is 15 repetitions, and min / max are in the JSON;
  2. isin's median < the inner join's against the same list, at every list size.
  python experiments/predicate_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

LDS_MAX = int(re.search(r"isin_lds_max_values = (\d+)", open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()).group(1))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def compare_part(ctx, n, reps, dev, g):
    results = []
    nulls = (torch.rand((n + 7) // 8, device=dev, generator=g) < 0.05).to(torch.uint8) * 16        # a sparse null mask
    out = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    for name, data, dtype in (("f64 normal", torch.randn(n, dtype=torch.float64, device=dev, generator=g), L.F64),
                              ("i64 over 1 M values", torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=dev, generator=g), L.I64)):
        a, b = (0.5, 1.5) if dtype == L.F64 else (250_000.0, 750_000.0)
        scratch = torch.empty_like(data)
        r = {"column": name, "rows": n, "copy": timed(lambda: scratch.copy_(data), reps),
             "torch_gt": timed(lambda: data > a, reps), "arg_extreme": {}, "predicates": []}
        del scratch
        for masked in (False, True):
            col = (data, nulls if masked else None, dtype)
            y = timed(lambda: ctx.arg_extreme(col, n), reps)                  # the yardstick: the same column, mask and all
            y["gate_bound_ms"] = y["median_ms"] * (1.0 + (y["max_ms"] - y["min_ms"]) / y["median_ms"])
            r["arg_extreme"]["null mask" if masked else "no mask"] = y
            for op, label in ((L.PRED_GT, "gt"), (L.PRED_BETWEEN, "between"), (L.PRED_ISNA, "isna")):
                t = timed(lambda: ctx.predicate(col, n, op, a, b, out=out), reps)
                c = timed(lambda: ctx.predicate(col, n, op, a, b, count_only=True), reps)
                row = {"op": label, "null_mask": masked, **t, "count_only_median_ms": c["median_ms"],
                       "over_arg_extreme": t["median_ms"] / y["median_ms"], "over_copy": t["median_ms"] / r["copy"]["median_ms"],
                       "over_torch_gt": t["median_ms"] / r["torch_gt"]["median_ms"], "gate_bound_ms": y["gate_bound_ms"],
                       "gate_held": t["median_ms"] <= y["gate_bound_ms"]}
                if dtype == L.I64:                                           # the A/B: convert every cell in the loop
                    ctx.set_option("predicate_path", 1)
                    row["convert_per_row"] = timed(lambda: ctx.predicate(col, n, op, a, b, out=out), reps)
                    ctx.set_option("predicate_path", 0)
                    row["interval_over_convert"] = t["median_ms"] / row["convert_per_row"]["median_ms"]
                print(json.dumps({"column": name, **row}), flush=True)
                r["predicates"].append(row)
        r["gate_compare_within_arg_extreme_noise"] = all(p["gate_held"] for p in r["predicates"])
        results.append(r)
    return results


def isin_part(ctx, n, reps, dev, g):
    results = []
    out = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    for m in (3, 100, LDS_MAX, 100_000, 10_000_000):
        if m > n:
            continue
        for kind in ("random 64-bit patterns", "integral f64"):
            if kind == "integral f64":
                vals, dtype = torch.arange(m, dtype=torch.float64, device=dev), L.F64
            else:
                vals, dtype = torch.randint(-2**63, 2**63 - 1, (m,), dtype=torch.int64, device=dev, generator=g), L.I64
            for hits in ("near 1", "near 0"):
                if hits == "near 1":
                    data = vals[torch.randint(0, m, (n,), device=dev, generator=g)]
                elif dtype == L.F64:
                    data = torch.randint(m, 2 * m + 1000, (n,), device=dev, generator=g).to(torch.float64)
                else:
                    data = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
                col, vcol = (data, None, dtype), (vals, None, dtype)
                t = timed(lambda: ctx.isin(col, n, vcol, out=out), reps)
                path = {1: "lds", 2: "global"}[ctx.timings()["n_partitions"]]
                row = {"values": m, "kind": kind, "hit_rate": hits, "path": path, "isin": t,
                       "join_inner": timed(lambda: ctx.join_indices_compute(col, n, vcol, m, L.INNER), max(2, reps // 2), warmup=1),
                       "torch_isin": timed(lambda: torch.isin(data, vals), max(2, reps // 2), warmup=1)}
                if m <= LDS_MAX:                                             # the other set, for the crossover
                    ctx.set_option("isin_path", 2)
                    row["isin_global_set"] = timed(lambda: ctx.isin(col, n, vcol, out=out), reps)
                    ctx.set_option("isin_path", 0)
                row["isin_over_join"] = t["median_ms"] / row["join_inner"]["median_ms"]
                row["isin_over_torch_isin"] = t["median_ms"] / row["torch_isin"]["median_ms"]
                row["gate_held"] = t["median_ms"] < row["join_inner"]["median_ms"]
                print(json.dumps(row), flush=True)
                results.append(row)
                del data
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "predicate_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    compare = compare_part(ctx, a.rows, a.reps, dev, g)
    isin = isin_part(ctx, a.rows, a.reps, dev, g)
    ctx.close()
    gates = {"compare_within_arg_extreme_noise": all(r["gate_compare_within_arg_extreme_noise"] for r in compare),
             "isin_faster_than_inner_join": all(r["gate_held"] for r in isin)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": a.rows, "reps": a.reps, "isin_lds_max_values": LDS_MAX,
                   "gates": gates, "compare": compare, "isin": isin}, f, indent=1)
        f.write("\n")
    print(json.dumps({"gates": gates}), flush=True)


if __name__ == "__main__":
    main()
