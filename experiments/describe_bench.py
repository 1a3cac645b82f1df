"""Describe at 100 M rows (DESIGN §4b "describe"): pandrs_hip_describe (radix select) against pandrs_hip_sort_indices of
the same column (the route to quartiles before describe existed: sort, then gather) and against a device copy of the
column (the bandwidth floor), all in one process.

Device-resident columns; torch.cuda.Event timing around each call (the library's calls synchronise before they return)
after warm-up; the median of --reps calls.  The gate: on every column describe takes less time than sort_indices.
  python experiments/describe_bench.py [--rows N] [--reps R] [--out FILE]
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
    normal = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    yield "f64 normal", normal, None, L.F64
    raw = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g).view(torch.float64)
    yield "f64 full-range random bits", torch.where(torch.isnan(raw), torch.zeros_like(raw), raw), None, L.F64
    del raw
    yield "f64 ten distinct values", torch.randint(0, 10, (n,), device=dev, generator=g).to(torch.float64), None, L.F64
    yield "f64 all equal", torch.full((n,), 3.25, dtype=torch.float64, device=dev), None, L.F64
    yield "i64 over 1 M values", torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=dev, generator=g), None, L.I64
    nulls = np.packbits(np.random.default_rng(2).random(n) < 0.1, bitorder="little")
    yield "f64 normal, 10 % nulls", normal, torch.from_numpy(nulls).to(dev), L.F64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "describe_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    results = []
    for name, data, mask, dtype in columns(n, dev):
        col = (data, mask, dtype)
        scratch = torch.empty_like(data)
        r = {"column": name, "rows": n,
             "describe_ms": timed(lambda: ctx.describe(col, n), a.reps),
             "sort_indices_ms": timed(lambda: ctx.sort_indices([col], n), a.reps),
             "copy_ms": timed(lambda: scratch.copy_(data), a.reps)}
        r["describe_over_sort"] = r["describe_ms"] / r["sort_indices_ms"]
        r["gate_describe_faster_than_sort"] = r["describe_ms"] < r["sort_indices_ms"]
        r["stats"] = {k: float(v) for k, v in ctx.describe(col, n).items()}
        print(json.dumps(r), flush=True)
        results.append(r)
        del scratch
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "results": results}, f, indent=1)
        f.write("\n")
    if not all(r["gate_describe_faster_than_sort"] for r in results):
        raise SystemExit("gate failed: describe is not faster than sort_indices on every column")


if __name__ == "__main__":
    main()
