"""Top-k at 100 M rows (DESIGN §4b "top-k"): pandrs_hip_topk for k in {1, 100, 10^4, 10^6, 10^7} in both directions, and
pandrs_hip_arg_extreme, against the yardsticks measured in the same process on the same columns: pandrs_hip_sort_indices of
that key (the route to nlargest before top-k existed: sort, then slice) and a device copy of the column (the bandwidth floor).

Device-resident columns; torch.cuda.Event timing around each call (the library's calls synchronise before they return)
after warm-up; the median of --reps calls.  "topk_path" -1 keeps every k on the select, so the table shows where the select
and the sort cross (--cross adds larger k for that); the default path is timed too.
The gate: for every k <= 10^6 on every column top-k takes less time than sort_indices of the same column.
  python experiments/topk_bench.py [--rows N] [--reps R] [--cross] [--out FILE]
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

KS = [1, 100, 10_000, 1_000_000, 10_000_000]


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
    return float(np.median(ms))


def columns(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    yield "f64 random", torch.rand(n, dtype=torch.float64, device=dev, generator=g), L.F64
    yield "i64 full range", torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g), L.I64
    yield "i64 over 1 M values", torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=dev, generator=g), L.I64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cross", action="store_true", help="also time the select at k = n / 4, n / 2 and 3 n / 4")
    ap.add_argument("--out", default=os.path.join("profiles", "topk_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    ks = [k for k in KS if k <= n] + ([n // 4, n // 2, 3 * (n // 4)] if a.cross else [])
    out = torch.empty(max(ks), dtype=torch.int64, device=dev)
    results = []
    for name, data, dtype in columns(n, dev):
        col = (data, None, dtype)
        scratch = torch.empty_like(data)
        r = {"column": name, "rows": n,
             "sort_indices_ms": {"descending": timed(lambda: ctx.sort_indices([col], n, [False]), a.reps),
                                 "ascending": timed(lambda: ctx.sort_indices([col], n, [True]), a.reps)},
             "copy_ms": timed(lambda: scratch.copy_(data), a.reps),
             "arg_extreme_ms": timed(lambda: ctx.arg_extreme(col, n), a.reps), "topk": []}
        del scratch
        r["arg_extreme_over_copy"] = r["arg_extreme_ms"] / r["copy_ms"]
        for k in ks:
            for largest in (True, False):
                sort_ms = r["sort_indices_ms"]["descending" if largest else "ascending"]
                ctx.set_option("topk_path", -1)
                select_ms = timed(lambda: ctx.topk(col, n, k, largest, out=out), a.reps)
                passes = ctx.timings()["n_partitions"]
                ctx.set_option("topk_path", 0)
                default_ms = timed(lambda: ctx.topk(col, n, k, largest, out=out), a.reps)
                row = {"k": k, "direction": "largest" if largest else "smallest", "select_ms": select_ms, "digit_streams": passes,
                       "default_path_ms": default_ms, "sort_ms": sort_ms, "select_over_sort": select_ms / sort_ms,
                       "default_over_sort": default_ms / sort_ms}
                print(json.dumps({"column": name, **row}), flush=True)
                r["topk"].append(row)
        r["gate_topk_faster_than_sort_up_to_1e6"] = all(t["default_path_ms"] < t["sort_ms"] for t in r["topk"] if t["k"] <= 1_000_000)
        print(json.dumps({k: v for k, v in r.items() if k != "topk"}), flush=True)
        results.append(r)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "results": results}, f, indent=1)
        f.write("\n")
    if not all(r["gate_topk_faster_than_sort_up_to_1e6"] for r in results):
        raise SystemExit("gate failed: top-k is not faster than sort_indices for every k <= 10^6 on every column")


if __name__ == "__main__":
    main()
