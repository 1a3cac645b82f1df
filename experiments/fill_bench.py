"""Fill at 100 M rows (DESIGN §4b "fill"): pandrs_hip_fill (FFILL, BFILL, LINEAR, VALUE) on one device-resident f64 column
whose missing rows are NaN cells: 10 % and 50 % missing at random positions, missing rows in runs of 10^4 (every other run),
and no missing rows.  Each time is set against a device copy of the same column (torch.clone) in the same process: by bytes
FFILL reads the column twice, writes it once and touches 1 / 8 byte per row of bits, 24 bytes per row against the copy's 16.

Device-resident column and outputs; torch.cuda.Event timing around each call (the library's calls synchronise before they
return) after warm-up; the median of --reps calls.
  python experiments/fill_bench.py [--rows N] [--reps R] [--out FILE]
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

METHODS = (("ffill", L.FILL_FFILL), ("bfill", L.FILL_BFILL), ("linear", L.FILL_LINEAR), ("value", L.FILL_VALUE))


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


def shapes(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    base = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    for share in (0.1, 0.5):
        yield "%d %% missing at random" % int(share * 100), torch.where(torch.rand(n, device=dev, generator=g) < share, nan, base)
    yield "missing in runs of 10^4", torch.where((torch.arange(n, device=dev) // 10_000) % 2 == 1, nan, base)
    yield "none missing", base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "fill_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    out = torch.empty(n, dtype=torch.float64, device=dev)
    out_mask = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    results = []
    for name, data in shapes(n, dev):
        col = (data, None, L.F64)
        r = {"shape": name, "rows": n, "copy_ms": timed(lambda: torch.clone(data), a.reps)}
        for label, method in METHODS:
            value = 0.0 if method == L.FILL_VALUE else None
            r["fill_%s_ms" % label] = timed(lambda: ctx.fill(col, n, method, value, out=out, out_mask=out_mask), a.reps)
            r["fill_%s_over_copy" % label] = r["fill_%s_ms" % label] / r["copy_ms"]
            r["fill_%s_still_missing" % label] = ctx.fill(col, n, method, value, out=out, out_mask=out_mask)[2]
        print(json.dumps(r), flush=True)
        results.append(r)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
