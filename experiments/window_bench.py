"""Window statistics at 100 M rows (DESIGN §4b "window"): pandrs_hip_window (rolling / expanding / EWM) against torch's
unfold(0, w, 1).sum / amax, cumsum and cummax, and against a device copy of the column (the bandwidth floor).

One device-resident f64 column (torch.randn), no nulls unless the case says so; torch.cuda.Event timing around each
call (the library's calls synchronise before they return) after warm-up; the median of --reps calls.  Algorithmic
bytes: the column read once (8 B / row) and the result written once (8 B / row), + n/8 bytes of null mask.  The O(n·w)
rolling fold also reports its rate in f64 adds per second (w adds per row for sum / mean; std adds 2w, plus w
multiplies and w subtractions).
  python experiments/window_bench.py [--rows N] [--reps R] [--out FILE] [--quick]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the torch comparisons (profiling runs)")
    args = ap.parse_args()
    n, dev = args.rows, "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    nulls = (torch.rand(n, device=dev, generator=g) < 0.1)
    w8 = torch.arange(8, device=dev, dtype=torch.uint8)
    mask = (nulls.view(-1, 8).to(torch.uint8) << w8).sum(1, dtype=torch.uint8) if n % 8 == 0 else None
    col, col_nulls = (x, None, L.F64), (x, mask, L.F64)
    ctx = pa.Context(0)
    res = {"rows": n, "reps": args.reps, "cases": {}}
    copy_ms = timed(lambda: x.clone(), args.reps)
    res["device_copy_ms"] = copy_ms
    res["device_copy_TB_per_s"] = 16.0 * n / copy_ms / 1e9
    print("copy", copy_ms, flush=True)

    def case(name, fn, adds_per_row=0, bytes_per_row=16.0, torch_fn=None, torch_name=None):
        ms = timed(fn, args.reps)
        c = {"ms": ms, "algorithmic_TB_per_s": bytes_per_row * n / ms / 1e9, "x_copy": ms / copy_ms}
        if adds_per_row:
            c["adds_per_s"] = adds_per_row * n / ms * 1e3
        if torch_fn is not None and not args.quick:
            c[torch_name + "_ms"] = timed(torch_fn, args.reps)
        res["cases"][name] = c
        print(name, json.dumps(c), flush=True)

    def rolling(op, w, c=col):
        return lambda: ctx.window(c, n, L.WINDOW_KIND_ROLLING, op, window=w)

    for w in (3, 30, 300, 3000):
        tsum = (lambda w=w: x.unfold(0, w, 1).sum(-1)) if w <= 300 else None
        case("rolling_sum_w%d" % w, rolling(L.WINDOW_SUM, w), adds_per_row=w, torch_fn=tsum, torch_name="torch_unfold_sum")
        case("rolling_mean_w%d" % w, rolling(L.WINDOW_MEAN, w), adds_per_row=w)
        case("rolling_std_w%d" % w, rolling(L.WINDOW_STD, w), adds_per_row=2 * w)
    for w in (30, 3000):
        tmax = (lambda w=w: x.unfold(0, w, 1).amax(-1)) if w <= 300 else None
        case("rolling_min_w%d" % w, rolling(L.WINDOW_MIN, w))
        case("rolling_max_w%d" % w, rolling(L.WINDOW_MAX, w), torch_fn=tmax, torch_name="torch_unfold_amax")
        case("rolling_count_w%d" % w, rolling(L.WINDOW_COUNT, w))
        if mask is not None:
            case("rolling_count_nulls_w%d" % w, rolling(L.WINDOW_COUNT, w, col_nulls), bytes_per_row=16.125)
            case("rolling_sum_nulls_w%d" % w, rolling(L.WINDOW_SUM, w, col_nulls), adds_per_row=w, bytes_per_row=16.125)
    exp = lambda op: (lambda: ctx.window(col, n, L.WINDOW_KIND_EXPANDING, op, min_periods=0))
    case("expanding_sum", exp(L.WINDOW_SUM), torch_fn=lambda: torch.cumsum(x, 0), torch_name="torch_cumsum")
    case("expanding_var", exp(L.WINDOW_VAR))
    case("expanding_max", exp(L.WINDOW_MAX), torch_fn=lambda: torch.cummax(x, 0), torch_name="torch_cummax")
    ewm = lambda op: (lambda: ctx.window(col, n, L.WINDOW_KIND_EWM, op, alpha=0.1))
    case("ewm_mean", ewm(L.WINDOW_MEAN))
    case("ewm_std", ewm(L.WINDOW_STD))
    # the answers are torch's where torch computes the same thing
    if not args.quick:
        got = ctx.window(col, n, L.WINDOW_KIND_ROLLING, L.WINDOW_MAX, window=30)
        res["rolling_max_w30_equals_torch"] = bool(torch.equal(got[29:], x.unfold(0, 30, 1).amax(-1)))
        got = ctx.window(col, n, L.WINDOW_KIND_EXPANDING, L.WINDOW_MAX, min_periods=0)
        res["expanding_max_equals_torch_cummax"] = bool(torch.equal(got, torch.cummax(x, 0).values))
        del got
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
