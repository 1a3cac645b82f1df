"""Binning at 100 M rows (DESIGN §4b "bin"): pandrs_hip_bin and pandrs_hip_bin_edges on a device-resident f64 column, all in
one process.  What is measured:
  bin, evenly spaced edges   10, 100 and 4096 bins over a uniform column, codes and counts, through "bin_path" 1 (search), 2
                             (guess) and 0 (auto)
  the same at 2 ... 1024     search against guess alone ("sweep"): where the auto rule's threshold, bin_guess_min_bins, comes from
  bin, quantile edges        100 bins at the column's own quantiles (not evenly spaced: the search)
  codes / counts / both      100 evenly spaced bins, on the uniform column and on a column with every row in one bin (the worst
                             case for the histogram: one LDS cell)
  bin_edges QCUT             q = 4, 10, 31, 100 (q + 1 distinct ranks; 100: four selections)
  alongside                  a device copy (torch.clone), pandrs_hip_predicate BETWEEN on the same column, pandrs_hip_quantiles
                             with as many percentiles as give q + 1 distinct ranks (q <= 31), pandrs_hip_sort_indices
First the checks: both paths give the same codes, the counts are the codes' histogram and sum to the rows, the codes equal
torch.bucketize on the same edges.  Then, after warm-up, --reps rounds (at least 20) time every call once per round with device
events, so the repeats of the calls alternate.
Gate 1: at every bin count the auto path's median is no more than the faster forced path's median plus that path's own spread
(max - min).  Gate 2: codes and counts in one call take no longer than the codes-only call plus the counts-only call, on both
columns.  Gate 3: QCUT at q <= 31 is no slower than pandrs_hip_quantiles at the same number of distinct ranks, beyond that
call's own spread.  The ratios to the copy (bytes predict 0.75) and to BETWEEN are reported without a threshold.  The script
exits 1 when a gate or a check fails.
  python experiments/bin_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

BINS = (10, 100, 4096)
QS = (4, 10, 31, 100)
SWEEP = (2, 4, 8, 16, 32, 64, 128, 256, 1024)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def percentiles_for(ranks):
    """Percentiles whose lower and upper ranks are `ranks` distinct ones: p = 0 gives one rank, any other p two."""
    k = ranks // 2
    ps = [100.0 * (j + 0.37) / (k + 1) for j in range(k)]
    return ([0.0] if ranks % 2 else []) + ps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "bin_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    one = torch.full((n,), 0.505, dtype=torch.float64, device=dev)
    cx, cone = (x, None, L.F64), (one, None, L.F64)
    codes = torch.empty(n, dtype=torch.int32, device=dev)
    bits = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
    even = {nb: np.arange(nb + 1, dtype=np.float64) * (1.0 / nb) for nb in BINS}
    qedges, _ = ctx.bin_edges(cx, n, L.BIN_QCUT, 100)
    qedges[-1] += 0.001

    def bin_call(col, edges, path, want_codes=True, want_counts=True):
        def fn():
            ctx.set_option("bin_path", path)
            return ctx.bin(col, n, edges, out=codes if want_codes else None, want_codes=want_codes, want_counts=want_counts)
        return fn

    # ---- the checks ----
    checks = {}
    ok = True
    for nb in BINS:
        _, c1 = bin_call(cx, even[nb], 1)()
        ran1 = ctx.timings()["n_partitions"]
        first = codes.clone()
        _, c2 = bin_call(cx, even[nb], 2)()
        ran2 = ctx.timings()["n_partitions"]
        hist = torch.bincount((codes + 2).to(torch.int64), minlength=nb + 2).cpu().numpy()       # NAN, NONE, then the bins
        want = torch.bucketize(x, torch.from_numpy(even[nb]).to(dev), right=True).to(torch.int32) - 1
        want[want >= nb] = -1
        checks["bins_%d" % nb] = {"paths_agree": bool(torch.equal(first, codes)), "paths_ran": [ran1, ran2],
                                  "counts_agree": bool(np.array_equal(c1, c2)), "counts_sum": int(c1.sum()),
                                  "counts_are_the_histogram": bool(np.array_equal(c1[:nb], hist[2:]) and c1[nb] == hist[1] and c1[nb + 1] == hist[0]),
                                  "equals_bucketize": bool(torch.equal(codes, want))}
        ck = checks["bins_%d" % nb]
        ok = ok and ck["paths_agree"] and ck["paths_ran"] == [1, 2] and ck["counts_agree"] and ck["counts_sum"] == n and \
            ck["counts_are_the_histogram"] and ck["equals_bucketize"]
        del first, want
    _, c = bin_call(cone, even[100], 0)()
    checks["one_bin"] = {"count": int(c[50]), "sum": int(c.sum())}
    ok = ok and int(c[50]) == n
    print(json.dumps(checks), flush=True)

    calls = {"copy": lambda: torch.clone(x),
             "between": lambda: ctx.predicate(cx, n, L.PRED_BETWEEN, 0.25, 0.75, out=bits),
             "sort_indices": lambda: ctx.sort_indices([cx], n),
             "bin_quantile_edges_100": bin_call(cx, qedges, 0)}
    for nb in BINS:
        for path, name in ((1, "search"), (2, "guess"), (0, "auto")):
            calls["bin_%d_%s" % (nb, name)] = bin_call(cx, even[nb], path)
    for nb in SWEEP:                                            # where the auto rule's threshold comes from
        e = np.arange(nb + 1, dtype=np.float64) * (1.0 / nb)
        calls["sweep_%d_search" % nb] = bin_call(cx, e, 1)
        calls["sweep_%d_guess" % nb] = bin_call(cx, e, 2)
    for cname, col in (("uniform", cx), ("one_bin", cone)):
        calls["codes_only_" + cname] = bin_call(col, even[100], 0, want_counts=False)
        calls["counts_only_" + cname] = bin_call(col, even[100], 0, want_codes=False)
        calls["both_" + cname] = bin_call(col, even[100], 0)
    for q in QS:
        calls["qcut_edges_%d" % q] = (lambda q: lambda: ctx.bin_edges(cx, n, L.BIN_QCUT, q))(q)
        if q + 1 <= 32:
            ps = percentiles_for(q + 1)
            calls["quantiles_%d_ranks" % (q + 1)] = (lambda ps: lambda: ctx.quantiles(cx, n, ps))(ps)
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(max(a.reps, 20)):                            # one repeat of every call per round: the repeats alternate
        for k, fn in calls.items():
            ms[k].append(once(fn))
    ctx.set_option("bin_path", 0)
    r = {"rows": n}
    for k, v in ms.items():
        r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    med = lambda k: r[k + "_ms"]["median"]                      # noqa: E731
    spread = lambda k: r[k + "_ms"]["max"] - r[k + "_ms"]["min"]        # noqa: E731
    gates = {}
    for nb in BINS:
        fast = min(("bin_%d_search" % nb, "bin_%d_guess" % nb), key=med)
        r["bin_%d_faster_path" % nb] = fast.rsplit("_", 1)[1]
        r["bin_%d_auto_over_faster" % nb] = med("bin_%d_auto" % nb) / med(fast)
        r["bin_%d_over_copy" % nb] = med("bin_%d_auto" % nb) / med("copy")          # by bytes: 12 / 16 = 0.75
        r["bin_%d_over_between" % nb] = med("bin_%d_auto" % nb) / med("between")
        gates["gate_1_auto_is_the_faster_path_%d" % nb] = med("bin_%d_auto" % nb) <= med(fast) + spread(fast)
    r["sweep_guess_over_search"] = {str(nb): med("sweep_%d_guess" % nb) / med("sweep_%d_search" % nb) for nb in SWEEP}
    r["bin_quantile_edges_100_over_copy"] = med("bin_quantile_edges_100") / med("copy")
    for cname in ("uniform", "one_bin"):
        two = med("codes_only_" + cname) + med("counts_only_" + cname)
        r["both_over_two_calls_" + cname] = med("both_" + cname) / two
        r["counts_only_over_copy_" + cname] = med("counts_only_" + cname) / med("copy")
        gates["gate_2_fused_counts_" + cname] = med("both_" + cname) <= two
    for q in QS:
        r["qcut_%d_over_sort" % q] = med("qcut_edges_%d" % q) / med("sort_indices")
        if q + 1 <= 32:
            k = "quantiles_%d_ranks" % (q + 1)
            r["qcut_%d_over_quantiles" % q] = med("qcut_edges_%d" % q) / med(k)
            gates["gate_3_qcut_%d_no_slower_than_quantiles" % q] = med("qcut_edges_%d" % q) <= med(k) + spread(k)
    r.update(gates)
    ok = ok and all(gates.values())
    print(json.dumps(r), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": max(a.reps, 20), "checks": checks, "gate": ok, "result": r}, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
