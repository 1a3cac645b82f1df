"""Rolling / expanding median and quantile at 100 M rows (DESIGN §4b "window median / quantile"): pandrs_hip_window_quantile
on its two paths, the direct one (LDS selection, rolling windows up to WQ_DIRECT_MAX) and the general one (stable sort,
wavelet matrix over the ranks), against yardsticks measured in the same process on the same column: pandrs_hip_sort_indices
(the general path's first step), the rolling max at the same window (pandrs_hip_window: the cheapest statistic of the same
windows) and a device copy.

Columns: random f64, and f64 with long tie runs (5 distinct values).  Rolling median at w = 3 / 10 / 30 / WQ_DIRECT_MAX (and
any --direct-windows below it) on both paths, at 300 / 3 000 / 10^6 on the general path, the expanding median, and q = 0.9.

Device-resident columns and output; after warm-up, the median of the repetitions with the smallest and largest beside it.
Timing is a pair of torch.cuda.Events on torch's current stream around each call; the library synchronises its own stream
before a call returns, so the interval is the call's wall time as the host sees it.
Gate, reported as held or not: at every measured w <= WQ_DIRECT_MAX the direct path's median <= the general path's median at
the same w x (1 + (max - min) / median of the general path's own repetitions).  WQ_DIRECT_MAX is the largest measured w that
holds it (docs/EXPERIMENT_LOG.md, "Window median / quantile").
  python experiments/window_quantile_bench.py [--rows N] [--reps R] [--direct-windows 48,64] [--out FILE]"""
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

DIRECT_MAX = int(re.search(r"constexpr int WQ_DIRECT_MAX = (\d+);",
                           open(os.path.join(ROOT, "pandrs_amd", "csrc", "window_quantile.hip")).read()).group(1))
AUTO, DIRECT, GENERAL = 0, 1, 2


def timed(fn, reps, warmup=1):
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


def quantile(ctx, col, n, path, reps, **kw):
    ctx.set_option("window_quantile_path", path)
    try:
        return timed(lambda: ctx.window_quantile(col, n, **kw), reps)
    finally:
        ctx.set_option("window_quantile_path", AUTO)


def column_part(ctx, name, data, n, reps, direct_windows):
    col = (data, None, L.F64)
    scratch = torch.empty_like(data)
    r = {"column": name, "rows": n, "copy": timed(lambda: scratch.copy_(data), reps),
         "sort_indices": timed(lambda: ctx.sort_indices([col], n), max(3, reps // 3)), "rolling": []}
    del scratch
    R = L.WINDOW_KIND_ROLLING
    slow = max(3, reps // 3)
    for w in sorted(set(direct_windows) | {300, 3000, 1_000_000}):
        if w > n:
            continue
        row = {"window": w, "rolling_max": timed(lambda: ctx.window(col, n, R, L.WINDOW_MAX, window=w), reps),
               "general": quantile(ctx, col, n, GENERAL, slow, kind=R, window=w)}
        g = row["general"]
        if w <= DIRECT_MAX:
            row["direct"] = quantile(ctx, col, n, DIRECT, reps, kind=R, window=w)
            row["gate_bound_ms"] = g["median_ms"] * (1.0 + (g["max_ms"] - g["min_ms"]) / g["median_ms"])
            row["gate_held"] = row["direct"]["median_ms"] <= row["gate_bound_ms"]
            row["general_over_direct"] = g["median_ms"] / row["direct"]["median_ms"]
        row["general_over_sort"] = g["median_ms"] / r["sort_indices"]["median_ms"]
        print(json.dumps({"column": name, **row}), flush=True)
        r["rolling"].append(row)
    r["expanding_median"] = quantile(ctx, col, n, AUTO, slow, kind=L.WINDOW_KIND_EXPANDING, min_periods=1)
    r["q90"] = {"w30 (default path)": quantile(ctx, col, n, AUTO, reps, kind=R, window=30, median=False, q=0.9),
                "w3000": quantile(ctx, col, n, AUTO, slow, kind=R, window=3000, median=False, q=0.9)}
    r["general_phases_ms_w3000_q90"] = ctx.timings()["phase_ms"]          # the last call's: sort, build (ranks, levels), probe (queries)
    print(json.dumps({"column": name, "expanding_median": r["expanding_median"], "q90": r["q90"]}), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--direct-windows", default="", help="more windows <= WQ_DIRECT_MAX to time on both paths, comma separated")
    ap.add_argument("--out", default=os.path.join("profiles", "window_quantile_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    n = a.rows
    extra = [int(v) for v in a.direct_windows.split(",") if v]
    direct_windows = sorted({w for w in [3, 10, 30, DIRECT_MAX] + extra if w <= DIRECT_MAX})
    columns = []
    for name, make in (("f64 normal", lambda: torch.randn(n, dtype=torch.float64, device=dev, generator=g)),
                       ("f64 over 5 values", lambda: torch.randint(0, 5, (n,), device=dev, generator=g).to(torch.float64))):
        data = make()
        columns.append(column_part(ctx, name, data, n, a.reps, direct_windows))
        del data
    ctx.close()
    held = {}
    for c in columns:
        for row in c["rolling"]:
            if "gate_held" in row:
                held[row["window"]] = held.get(row["window"], True) and row["gate_held"]
    largest = max([w for w, ok in held.items() if ok and all(held[v] for v in held if v <= w)], default=0)
    gates = {"direct_no_slower_than_general_at_every_measured_w": all(held.values()), "largest_w_holding_the_gate": largest}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "WQ_DIRECT_MAX": DIRECT_MAX, "gates": gates,
                   "columns": columns}, f, indent=1)
        f.write("\n")
    print(json.dumps({"WQ_DIRECT_MAX": DIRECT_MAX, "gates": gates}), flush=True)


if __name__ == "__main__":
    main()
