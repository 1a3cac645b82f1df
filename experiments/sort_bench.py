"""pandrs_hip_sort_indices at 100 M rows (DESIGN §4b "sort"), against torch's stable sort of the same column.

Cases: one i64 key uniform over 1 M values (a 20-bit range: the width trimming leaves two 10-bit passes), one full-range
random i64 key (six 11-bit passes), one f64 key, two keys (i64 asc, f64 desc: 84 bits, two words), one string-code key
(u32 codes ranked through a 1 M-entry table).  Device-resident columns; hipEvent timing (torch.cuda.Event on the
library's call, which synchronises before it returns) after warm-up; the median of --reps calls.
  python experiments/sort_bench.py [--rows N] [--reps R] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--digit-bits", type=int, default=0, help="widest radix digit (context option sort_digit_bits; 0 = default)")
    ap.add_argument("--only", default=None, help="comma-separated case names")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    n, dev = args.rows, "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    narrow = torch.randint(0, 1_000_000, (n,), dtype=torch.int64, device=dev, generator=g)
    full = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
    f64 = torch.randn(n, dtype=torch.float64, device=dev, generator=g) * 1e3
    codes = torch.randint(0, 1_000_000, (n,), dtype=torch.int32, device=dev, generator=g)
    rank = torch.randperm(1_000_000, device=dev, generator=g).to(torch.int32)
    ctx = pa.Context(0)
    if args.digit_bits:
        ctx.set_option("sort_digit_bits", args.digit_bits)
    cases = {
        "i64_narrow_1M_values": ([(narrow, None, L.I64)], [True], None),
        "i64_full_range": ([(full, None, L.I64)], [True], None),
        "f64": ([(f64, None, L.F64)], [True], None),
        "i64_asc_f64_desc": ([(narrow, None, L.I64), (f64, None, L.F64)], [True, False], None),
        "string_codes_1M": ([(codes, None, L.U32CODE)], [True], rank),
    }
    res = {"rows": n, "reps": args.reps, "digit_bits": args.digit_bits or 8, "cases": {}}
    for name, (keys, asc, rk) in cases.items():
        if args.only and name not in args.only.split(","):
            continue
        med, lo, hi = timed(lambda: ctx.sort_indices(keys, n, asc, rk), args.reps)
        t = ctx.timings()
        res["cases"][name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "passes": t["n_partitions"],
                              "phase_ms": t["phase_ms"], "algorithmic_bytes": t["algorithmic_bytes"],
                              "GB_per_s": t["algorithmic_bytes"] / med / 1e6}
        print(name, json.dumps(res["cases"][name]), flush=True)
    for name, x in (("i64_narrow_1M_values", narrow), ("i64_full_range", full)):
        if args.no_torch or name not in res["cases"]:
            continue
        med, lo, hi = timed(lambda: torch.sort(x, stable=True), args.reps)
        res["cases"][name]["torch_sort_stable_ms"] = med
        med2, _, _ = timed(lambda: torch.argsort(x, stable=True), args.reps)
        res["cases"][name]["torch_argsort_stable_ms"] = med2
        print(name, "torch.sort(stable) %.3f ms, torch.argsort(stable) %.3f ms" % (med, med2), flush=True)
    # the answer is torch's, row for row (both stable)
    res["full_range_equals_torch"] = bool(torch.equal(ctx.sort_indices([(full, None, L.I64)], n, [True]),
                                                      torch.sort(full, stable=True).indices))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
