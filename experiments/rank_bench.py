"""Rank at 100 M rows (DESIGN §4b "rank"): pandrs_hip_rank (Average, First, Dense) against pandrs_hip_sort_indices of the
same column, and the rank phase's unavoidable traffic measured in the same process: a random gather of n f64 through the
sort's permutation (pandrs_hip_gather_column; the boundary pass gathers the cells), a random scatter of n f64 through the
same permutation (torch index_copy_; the ranks go back to row order) and a device copy (the bandwidth floor).

The quantity to read is rank - sort on the same column against scatter (First) or scatter + gather (Average, Dense).
Device-resident columns; torch.cuda.Event timing around each call (the library's calls synchronise before they return)
after warm-up; the median of --reps calls.
  python experiments/rank_bench.py [--rows N] [--reps R] [--out FILE]
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

METHODS = (("average", L.RANK_AVERAGE), ("first", L.RANK_FIRST), ("dense", L.RANK_DENSE))


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
    raw = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g).view(torch.float64)
    yield "f64 full range", torch.where(torch.isnan(raw), torch.zeros_like(raw), raw), L.F64
    del raw
    yield "f64 over 1 M values", torch.randint(0, 1_000_000, (n,), device=dev, generator=g).to(torch.float64) * 0.5, L.F64
    yield "i64 over 1 M values", torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=dev, generator=g), L.I64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "rank_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    results = []
    for name, data, dtype in columns(n, dev):
        col = (data, None, dtype)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        r = {"column": name, "rows": n}
        for label, method in METHODS:
            r["rank_%s_ms" % label] = timed(lambda: ctx.rank(col, n, method, out=out), a.reps)
        r["sort_indices_ms"] = timed(lambda: ctx.sort_indices([col], n), a.reps)
        perm = ctx.sort_indices([col], n)
        payload = torch.arange(n, dtype=torch.float64, device=dev)
        src = (L.Column * 1)()
        src[0].data, src[0].null_mask, src[0].dtype = payload.data_ptr(), None, L.F64

        def gather():
            st = ctx.lib.pandrs_hip_gather_column(ctx.h, L.MEM_DEVICE, src, n, perm.data_ptr(), n, 0, out.data_ptr())
            assert st == 0, L.last_error()
        r["random_gather_ms"] = timed(gather, a.reps)
        r["random_scatter_ms"] = timed(lambda: out.index_copy_(0, perm, payload), a.reps)
        r["copy_ms"] = timed(lambda: out.copy_(payload), a.reps)
        del perm, payload
        for label, _ in METHODS:
            phase = r["rank_%s_ms" % label] - r["sort_indices_ms"]
            floor = r["random_scatter_ms"] + (0.0 if label == "first" else r["random_gather_ms"])
            r["rank_phase_%s_ms" % label] = phase
            r["rank_phase_%s_over_unavoidable" % label] = phase / floor
        print(json.dumps(r), flush=True)
        results.append(r)
        del out
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
