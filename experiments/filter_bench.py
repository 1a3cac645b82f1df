"""Stream compaction at 100 M rows (DESIGN §4b "filter"): pandrs_hip_filter_indices and pandrs_hip_filter_gather against the
index route (filter_indices + pandrs_hip_gather_f64) and torch's boolean indexing t[mask].

Selectivities 1 %, 50 %, 99 %; masks random (every row on its own) or clustered (runs of 64 K rows, kept or dropped
together).  Device-resident columns, one f64 value column; torch.cuda.Event timing around each call (the library's calls
synchronise before they return) after warm-up; the median of --reps calls.  Byte accounting (not measured): one f64
column at 50 % moves 800 MB read + 12.5 MB of selection bits + 400 MB written.
  python experiments/filter_bench.py [--rows N] [--reps R] [--out FILE]
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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def pack(mask):
    n = mask.numel()
    pad = (-n) % 8
    m = torch.cat([mask, mask.new_zeros(pad)]) if pad else mask
    w = torch.arange(8, device=mask.device, dtype=torch.uint8)
    return (m.view(-1, 8).to(torch.uint8) << w).sum(1, dtype=torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, dev = args.rows, "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    ctx = pa.Context(0)
    res = {"rows": n, "reps": args.reps, "cases": {}}
    for layout in ("random", "clustered"):
        for p in (0.01, 0.5, 0.99):
            if layout == "random":
                mask = torch.rand(n, device=dev, generator=g) < p
            else:
                run = 1 << 16
                keep = torch.rand((n + run - 1) // run, device=dev, generator=g) < p
                mask = keep.repeat_interleave(run)[:n].contiguous()
            bits = pack(mask)
            cond = (bits, None, L.BOOLBITS)
            _, cnt = ctx.filter_indices(cond, n, indices=False)
            case = {"selected": cnt}
            case["filter_indices_ms"] = timed(lambda: ctx.filter_indices(cond, n), args.reps)[0]
            case["filter_count_only_ms"] = timed(lambda: ctx.filter_indices(cond, n, indices=False), args.reps)[0]
            ctx.filter_indices(cond, n, indices=False)
            case["filter_gather_f64_ms"] = timed(lambda: ctx.filter_gather((x, None, L.F64), n, cnt, out_device=True), args.reps)[0]
            t = ctx.timings()
            case["filter_gather_algorithmic_bytes"] = t["algorithmic_bytes"]
            case["filter_gather_GB_per_s"] = t["algorithmic_bytes"] / case["filter_gather_f64_ms"] / 1e6

            def index_route():
                idx, c = ctx.filter_indices(cond, n)
                return ctx.gather(x, None, idx, 0.0, L.F64)
            case["indices_plus_gather_ms"] = timed(index_route, args.reps)[0]
            case["torch_bool_index_ms"] = timed(lambda: x[mask], args.reps)[0]
            # the answer is torch's, bit for bit
            ctx.filter_indices(cond, n, indices=False)
            got = ctx.filter_gather((x, None, L.F64), n, cnt, out_device=True)
            case["equals_torch"] = bool(torch.equal(got.view(torch.int64), x[mask].view(torch.int64)))
            name = "%s_%g" % (layout, p)
            res["cases"][name] = case
            print(name, json.dumps(case), flush=True)
            del mask, bits, got
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
