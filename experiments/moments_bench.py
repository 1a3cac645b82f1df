"""Shape statistics at 100 M rows (DESIGN §4b "moments"): pandrs_hip_moments and pandrs_hip_order_stats on device-resident f64
columns, all in one process.  What is measured:
  sums only                 want = 0, one column: the lean first stream
  + LOG / RECIP / PROD      one bit at a time: what the transcendental streams cost
  + CENTRAL                 the second stream (two reads of the column predict 2 x sums only)
  eight columns             one call with eight columns against eight one-column calls (sums only, and CENTRAL)
  order statistics          TRIMMED_MEAN(0.1), AT_FRAC_N x 2 (iqr) and MEDIAN
  alongside                 a device copy (torch.clone), pandrs_hip_reduce_stats and pandrs_hip_quantiles at two percentiles
First the checks, against torch in float64 on the same column: counts, min, max exactly; sum, m2, m3, m4, abs_dev, log_sum,
recip_sum relative to their sums of magnitudes; the order statistics equal to the element of torch.sort at the reference's
index; the trimmed mean against the sorted slice.  Then, after warm-up, --reps rounds (at least 20) time every call once per
round with device events, so the repeats of the calls alternate.  Every gate is judged against its baseline's median plus that
baseline's own spread (max - min) in this process:
  gate 1   sums only is no slower than pandrs_hip_reduce_stats
  gate 2   (recorded, no threshold) LOG, RECIP, PROD over sums only
  gate 3   CENTRAL is no slower than two sums-only streams
  gate 4   eight columns in one call are no slower than eight one-column calls
  gate 5   iqr is no slower than pandrs_hip_quantiles at two percentiles; the trimmed mean no slower than that plus one
           sums-only stream (its band stream)
The script exits 1 when a check or a gate fails.
  python experiments/moments_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

CENTRAL, LOG, RECIP, PROD = L.MOMENTS_WANT_CENTRAL, L.MOMENTS_WANT_LOG, L.MOMENTS_WANT_RECIP, L.MOMENTS_WANT_PROD


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "moments_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cols = []
    for _ in range(8):                                          # lognormal: every cell > 0, so LOG and RECIP take every row
        cols.append((torch.randn(n, dtype=torch.float64, device=dev, generator=g).exp_(), None, L.F64))
    x = cols[0][0]
    cx = cols[0]

    # ---- the checks ----
    st = ctx.moments([cx], n, CENTRAL | LOG | RECIP | PROD)[0]
    variant_all = ctx.timings()["n_partitions"]
    ctx.moments([cx], n, 0)
    variant_lean = ctx.timings()["n_partitions"]
    mean = float(x.sum()) / n
    d = x - mean
    rel = lambda got, want, mag: abs(got - want) / mag          # noqa: E731
    checks = {"count": st["count"] == n == st["count_pos"] == st["count_nonzero"],
              "min_max": st["min"] == float(x.min()) and st["max"] == float(x.max()),
              "mean_is_sum_over_count": st["mean"] == st["sum"] / n,
              "variants": [variant_lean, variant_all],
              "sum_rel": rel(st["sum"], float(x.sum()), float(x.abs().sum())),
              "m2_rel": rel(st["m2"], float((d * d).sum()), float((d * d).sum())),
              "m3_rel": rel(st["m3"], float((d * d * d).sum()), float((d * d * d).abs().sum())),
              "m4_rel": rel(st["m4"], float((d * d * d * d).sum()), float((d * d * d * d).sum())),
              "abs_dev_rel": rel(st["abs_dev"], float(d.abs().sum()), float(d.abs().sum())),
              "log_sum_rel": rel(st["log_sum"], float(x.log().sum()), float(x.log().abs().sum())),
              "recip_sum_rel": rel(st["recip_sum"], float((1.0 / x).sum()), float((1.0 / x).sum()))}
    del d
    s = torch.sort(x).values
    t = int(n * 0.1)
    ops = [(L.OS_AT_FRAC_N, 0.25), (L.OS_AT_FRAC_N, 0.75), (L.OS_AT_FRAC_N1, 0.9), (L.OS_MEDIAN, 0.0), (L.OS_TRIMMED_MEAN, 0.1)]
    got, m = ctx.order_stats(cx, n, ops)
    med_want = (float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0 if n % 2 == 0 else float(s[n // 2])
    checks["order_stats"] = bool(m == n and got[0] == float(s[int(n * 0.25)]) and got[1] == float(s[int(n * 0.75)]) and
                                 got[2] == float(s[int((n - 1) * 0.9)]) and got[3] == med_want)
    checks["trimmed_mean_rel"] = abs(got[4] - float(s[t:n - t].sum()) / (n - 2 * t)) / float(s[t:n - t].mean())
    del s
    tol = 64 * n * 2.0 ** -53                                   # both sides are parallel folds: far inside gamma_n, far above what they differ by
    ok = checks["count"] and checks["min_max"] and checks["mean_is_sum_over_count"] and checks["variants"] == [1, 8] and \
        checks["order_stats"] and all(v <= tol for k, v in checks.items() if k.endswith("_rel"))
    print(json.dumps(checks), flush=True)

    calls = {"copy": lambda: torch.clone(x),
             "reduce_stats": lambda: ctx.column_stats(cx, n),
             "quantiles_2": lambda: ctx.quantiles(cx, n, [25.0, 75.0]),
             "sums_only": lambda: ctx.moments([cx], n, 0),
             "log": lambda: ctx.moments([cx], n, LOG),
             "recip": lambda: ctx.moments([cx], n, RECIP),
             "prod": lambda: ctx.moments([cx], n, PROD),
             "central": lambda: ctx.moments([cx], n, CENTRAL),
             "eight_in_one_call": lambda: ctx.moments(cols, n, 0),
             "eight_calls": lambda: [ctx.moments([c], n, 0) for c in cols],
             "eight_in_one_call_central": lambda: ctx.moments(cols, n, CENTRAL),
             "eight_calls_central": lambda: [ctx.moments([c], n, CENTRAL) for c in cols],
             "iqr": lambda: ctx.order_stats(cx, n, [(L.OS_AT_FRAC_N, 0.25), (L.OS_AT_FRAC_N, 0.75)]),
             "median": lambda: ctx.order_stats(cx, n, [(L.OS_MEDIAN, 0.0)]),
             "trimmed_mean": lambda: ctx.order_stats(cx, n, [(L.OS_TRIMMED_MEAN, 0.1)])}
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(max(a.reps, 20)):                            # one repeat of every call per round: the repeats alternate
        for k, fn in calls.items():
            ms[k].append(once(fn))
    r = {"rows": n}
    for k, v in ms.items():
        r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    med = lambda k: r[k + "_ms"]["median"]                      # noqa: E731
    spread = lambda k: r[k + "_ms"]["max"] - r[k + "_ms"]["min"]        # noqa: E731
    r["sums_only_GBps"] = n * 8 / med("sums_only") / 1e6
    r["sums_only_over_copy"] = med("sums_only") / med("copy")   # by bytes: 8 / 16 = 0.5
    r["sums_only_over_reduce_stats"] = med("sums_only") / med("reduce_stats")
    for k in ("log", "recip", "prod"):
        r[k + "_over_sums_only"] = med(k) / med("sums_only")
    r["central_over_two_sums_only"] = med("central") / (2.0 * med("sums_only"))
    r["eight_in_one_call_over_eight_calls"] = med("eight_in_one_call") / med("eight_calls")
    r["eight_in_one_call_over_eight_calls_central"] = med("eight_in_one_call_central") / med("eight_calls_central")
    r["iqr_over_quantiles_2"] = med("iqr") / med("quantiles_2")
    r["trimmed_mean_over_quantiles_2"] = med("trimmed_mean") / med("quantiles_2")
    gates = {"gate_1_sums_only_no_slower_than_reduce_stats": med("sums_only") <= med("reduce_stats") + spread("reduce_stats"),
             "gate_3_central_is_two_streams": med("central") <= 2.0 * (med("sums_only") + spread("sums_only")),
             "gate_4_eight_columns_in_one_call": med("eight_in_one_call") <= med("eight_calls") + spread("eight_calls"),
             "gate_4_eight_columns_in_one_call_central": med("eight_in_one_call_central") <= med("eight_calls_central") + spread("eight_calls_central"),
             "gate_5_iqr_no_slower_than_quantiles": med("iqr") <= med("quantiles_2") + spread("quantiles_2"),
             "gate_5_trimmed_mean_is_the_select_plus_one_stream":
                 med("trimmed_mean") <= med("quantiles_2") + spread("quantiles_2") + med("sums_only") + spread("sums_only")}
    r.update(gates)
    gate = all(gates.values())
    print(json.dumps(r), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "reps": max(a.reps, 20), "checks": checks, "checks_ok": ok,
                   "gate": gate, "result": r}, f, indent=1)
        f.write("\n")
    sys.exit(0 if ok and gate else 1)


if __name__ == "__main__":
    main()
