"""Distinct values at 100 M rows (DESIGN §4b "distinct"): pandrs_hip_distinct on device-resident columns, all in one process.
What is measured:
  tables                     an i64 column over 2 / 100 / 1024 / 8192 values, uniform and with 90 % of the rows on one value,
                             through "distinct_path" 1 (direct: an LDS table) and 2 (the groupby engine), BY_COUNT
  engine only                i64 over 10^5 and 10^6 values, beside a bare pandrs_hip_groupby_agg COUNT on the same column
  f64                        integral values (direct and engine) and non-integral values (engine)
  alongside                  a device copy (torch.clone) and pandrs_hip_bin counts-only on the same column at the same number of
                             cells (at most bin_max_bins = 4096 bins: the 8192-value column is binned in pairs of values)
First the checks: both paths give the same list, the counts are torch.bincount's and sum to the rows.  Then, after warm-up,
--reps rounds (at least 20) time every call once per round with device events, so the repeats of the calls alternate; the
stream kernels alone are read from pandrs_hip_get_timings (the census: "estimate", the counting stream: "aggregate").
Gate 1: at every table size the direct path's median is no more than the engine path's plus the larger of the two spreads
(max - min).  Gate 2: the direct path's counting stream is no slower than pandrs_hip_bin's counts-only stream beyond the larger
of the two spreads; its ratio to the copy (bytes predict 0.5) is recorded.  Gate 3, no threshold: the engine path's total over
the bare groupby COUNT at 10^5 and 10^6 values (what the census and the finish add).  The script exits 1 when a gate or a
check fails.
  python experiments/distinct_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

TABLES = (2, 100, 1024, 8192)
WIDE = (100_000, 1_000_000)


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
    ap.add_argument("--out", default=os.path.join("profiles", "distinct_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    cols = {}
    for k in TABLES:
        u = torch.randint(0, k, (n,), dtype=torch.int64, device=dev, generator=g) - 7
        hot = torch.where(torch.rand(n, device=dev, generator=g) < 0.9, torch.full_like(u, k // 2 - 7), u)
        cols["uniform_%d" % k], cols["hot_%d" % k] = u, hot
    for k in WIDE:
        cols["wide_%d" % k] = torch.randint(0, k, (n,), dtype=torch.int64, device=dev, generator=g) * 1_000_003
    cols["f64_integral"] = torch.randint(-500, 500, (n,), dtype=torch.int64, device=dev, generator=g).to(torch.float64)
    cols["f64_fractions"] = torch.randint(-500, 500, (n,), dtype=torch.int64, device=dev, generator=g).to(torch.float64) + 0.5
    view = {name: (t, None, L.F64 if t.dtype == torch.float64 else L.I64) for name, t in cols.items()}
    phases = {}

    def distinct_call(name, path):
        def fn():
            ctx.set_option("distinct_path", path)
            out = ctx.distinct(view[name], n, L.DISTINCT_BY_COUNT, out_device=True)
            phases[name, path] = ctx.timings()["phase_ms"]
            return out
        return fn

    def bin_call(name, k):
        bins = min(k, L.BIN_MAX_BINS)
        edges = -7.5 + np.arange(bins + 1, dtype=np.float64) * (k / bins)

        def fn():
            out = ctx.bin(view[name], n, edges, want_codes=False)
            phases[name, "bin"] = ctx.timings()["phase_ms"]
            return out
        return fn

    # ---- the checks ----
    checks = {}
    ok = True
    for k in TABLES:
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            v1, f1, k1, i1 = distinct_call(name, 1)()
            v2, f2, k2, i2 = distinct_call(name, 2)()
            want = torch.bincount(cols[name] + 7, minlength=k)
            order = torch.argsort(v1)
            ck = {"paths": [i1["path"], i2["path"]], "paths_agree": bool(torch.equal(v1, v2) and torch.equal(k1, k2) and torch.equal(f1, f2)),
                  "counts_sum": int(k1.sum()), "counts_are_bincount": bool(torch.equal(k1[order], want[want > 0])),
                  "descending": bool((k1[1:] <= k1[:-1]).all()), "entries": i1["n_entries"]}
            _, c = bin_call(name, k)()
            ck["bin_counts_sum"] = int(c[:min(k, L.BIN_MAX_BINS)].sum())
            checks[name] = ck
            ok = ok and ck["paths"] == [1, 2] and ck["paths_agree"] and ck["counts_sum"] == n and ck["counts_are_bincount"] and \
                ck["descending"] and ck["bin_counts_sum"] == n
    for k in WIDE:
        name = "wide_%d" % k
        v, f, c, info = distinct_call(name, 0)()
        groups = ctx.groupby_compute([view[name]], n, [view[name]], [(0, L.COUNT)])
        checks[name] = {"path": info["path"], "entries": info["n_entries"], "groupby_groups": groups, "counts_sum": int(c.sum())}
        ok = ok and info["path"] == 2 and info["n_entries"] == groups and int(c.sum()) == n
    for name, want_path in (("f64_integral", 1), ("f64_fractions", 2)):
        v, f, c, info = distinct_call(name, 0)()
        checks[name] = {"path": info["path"], "entries": info["n_entries"], "counts_sum": int(c.sum())}
        ok = ok and info["path"] == want_path and int(c.sum()) == n and info["n_entries"] == 1000
    print(json.dumps(checks), flush=True)

    calls = {"copy": lambda: torch.clone(cols["uniform_100"])}
    for k in TABLES:
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            calls[name + "_direct"] = distinct_call(name, 1)
            calls[name + "_engine"] = distinct_call(name, 2)
            calls[name + "_bin_counts"] = bin_call(name, k)
    for k in WIDE:
        name = "wide_%d" % k
        calls[name + "_engine"] = distinct_call(name, 2)
        calls[name + "_groupby_count"] = (lambda name: lambda: ctx.groupby_compute([view[name]], n, [view[name]], [(0, L.COUNT)]))(name)
    calls["f64_integral_direct"] = distinct_call("f64_integral", 1)
    calls["f64_integral_engine"] = distinct_call("f64_integral", 2)
    calls["f64_fractions_engine"] = distinct_call("f64_fractions", 2)
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    stream = {}
    for _ in range(max(a.reps, 20)):                            # one repeat of every call per round: the repeats alternate
        for k, fn in calls.items():
            ms[k].append(once(fn))
        for key, ph in phases.items():
            stream.setdefault(key, {"estimate": [], "aggregate": []})
            for p in ("estimate", "aggregate"):
                stream[key][p].append(ph.get(p, 0.0))
    ctx.set_option("distinct_path", 0)
    r = {"rows": n}
    for k, v in ms.items():
        r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    med = lambda k: r[k + "_ms"]["median"]                      # noqa: E731
    spread = lambda k: r[k + "_ms"]["max"] - r[k + "_ms"]["min"]        # noqa: E731
    smed = lambda key, p: float(np.median(stream[key][p]))      # noqa: E731
    sspread = lambda key, p: max(stream[key][p]) - min(stream[key][p])  # noqa: E731
    gates = {}
    for k in TABLES:
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            d, e = name + "_direct", name + "_engine"
            r[name + "_direct_over_engine"] = med(d) / med(e)
            gates["gate_1_direct_no_slower_than_engine_" + name] = med(d) <= med(e) + max(spread(d), spread(e))
            r[name + "_census_ms"] = smed((name, 1), "estimate")
            r[name + "_stream_ms"] = smed((name, 1), "aggregate")
            r[name + "_bin_stream_ms"] = smed((name, "bin"), "aggregate")
            r[name + "_stream_over_bin_stream"] = r[name + "_stream_ms"] / r[name + "_bin_stream_ms"]
            r[name + "_stream_over_copy"] = r[name + "_stream_ms"] / med("copy")                     # by bytes: 8 / 16 = 0.5
            r[name + "_direct_over_bin_counts"] = med(d) / med(name + "_bin_counts")
            gates["gate_2_stream_no_slower_than_bin_counts_" + name] = \
                r[name + "_stream_ms"] <= r[name + "_bin_stream_ms"] + max(sspread((name, 1), "aggregate"), sspread((name, "bin"), "aggregate"))
    for k in WIDE:
        name = "wide_%d" % k
        r["gate_3_" + name + "_engine_over_groupby_count"] = med(name + "_engine") / med(name + "_groupby_count")
    r["f64_integral_direct_over_engine"] = med("f64_integral_direct") / med("f64_integral_engine")
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
