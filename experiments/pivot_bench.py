"""Pivot at 100 M rows (DESIGN §4b "pivot"): pandrs_hip_pivot on device-resident columns, all in one process.
What is measured:
  grids                      two i64 key columns over 2 x 2, 10 x 10, 64 x 64 and 63 x 63 labels (63 x 63 is the largest grid the
                             direct path takes: 64 x 64 table cells with the missing slots = pivot_direct_max_cells), uniform rows
                             and 90 % of the rows in one cell, crosstab (PANDRS_HIP_PIVOT_ROWS) and pivot_table SUM of an f64
                             column, through "pivot_path" 1 (direct: one fused stream into an LDS table) and 2 (general: the
                             groupby engine)
  alongside                  a device copy (torch.clone) of one key column, pandrs_hip_distinct's direct path on the index column
                             (its counting stream is the yardstick of gate 2) and a bare two-key pandrs_hip_groupby_agg with the
                             same op (the yardstick of gate 3)
First the checks: both paths give the same labels and rows per cell, the rows are torch.bincount's over the flat cell id and sum
to the row count, SUM agrees with the cell sums read off a prefix sum of the values in cell order within 1e-9 relative (no
atomic in the reference: an index_add_ of 10^8 f64 rows onto a handful of addresses takes minutes).  Then, after warm-up,
--reps rounds (at least 20) time every call once per round with device events, so the repeats of the calls alternate; the
stream kernels alone are read from pandrs_hip_get_timings (the census: "estimate", the fused stream: "aggregate").  A line of
progress is printed after the columns, after every checked shape and after the warm-up.
Gate 1: at every grid the direct path takes, its median is no more than the general path's plus the larger of the two spreads
(max - min), for both ops and both row layouts.  Gate 2, recorded: the direct ROWS stream over pandrs_hip_distinct's direct
counting stream of the index column (the byte count predicts 2 for two i64 keys).  Gate 3, recorded: the general path over the
bare two-key groupby_agg of the same op (the excess is the two label lists and the scatter).  The script exits 1 when gate 1 or
a check fails.
  python experiments/pivot_bench.py [--rows N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandrs_amd as pa  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402

GRIDS = (2, 10, 64, 63)


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
    ap.add_argument("--out", default=os.path.join("profiles", "pivot_bench.json"))
    a = ap.parse_args()
    dev = "cuda:0"
    t0 = time.time()
    ctx = pa.Context(0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    keys = {}
    for k in GRIDS:
        u1 = torch.randint(0, k, (n,), dtype=torch.int64, device=dev, generator=g) - 7
        u2 = torch.randint(0, k, (n,), dtype=torch.int64, device=dev, generator=g) + 100
        hot = torch.rand(n, device=dev, generator=g) < 0.9
        keys["uniform_%d" % k] = (u1, u2)
        keys["hot_%d" % k] = (torch.where(hot, torch.full_like(u1, k // 2 - 7), u1), torch.where(hot, torch.full_like(u2, k // 2 + 100), u2))
    values = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    vcol = (values, None, L.F64)
    view = {name: ((a1, None, L.I64), (a2, None, L.I64)) for name, (a1, a2) in keys.items()}
    torch.cuda.synchronize()
    print("columns ready, %.1f s" % (time.time() - t0), flush=True)
    phases = {}
    ops = {"rows": (L.PIVOT_ROWS, None, L.COUNT), "sum": (L.PIVOT_SUM, vcol, L.SUM)}

    def pivot_call(name, op, path):
        code, v, _ = ops[op]

        def fn():
            ctx.set_option("pivot_path", path)
            out = ctx.pivot(view[name][0], view[name][1], n, code, v, out_device=True)
            phases[name, op, path] = ctx.timings()["phase_ms"]
            return out
        return fn

    def distinct_call(name):
        def fn():
            ctx.set_option("distinct_path", 1)
            out = ctx.distinct(view[name][0], n, L.DISTINCT_BY_VALUE, out_device=True)
            phases[name, "distinct"] = ctx.timings()["phase_ms"]
            return out
        return fn

    def groupby_call(name, op):
        _, v, agg = ops[op]
        return lambda: ctx.groupby_compute(list(view[name]), n, [vcol], [(0, agg)])

    # ---- the checks ----
    checks = {}
    ok = True
    for k in GRIDS:
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            a1, a2 = keys[name]
            flat = (a2 - 100) * k + (a1 + 7)
            want_rows = torch.bincount(flat, minlength=k * k)
            # every cell's sum without an atomic: the values in cell order, a prefix sum, the difference at the cell's ends
            prefix = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), values[torch.argsort(flat)].cumsum(0)])
            ends = want_rows.cumsum(0)
            want_sum = (prefix[ends] - prefix[ends - want_rows]).reshape(k, k)
            want_rows = want_rows.reshape(k, k)
            del prefix
            ck = {}
            for op in ops:
                d, e = pivot_call(name, op, 1)(), pivot_call(name, op, 2)()
                same = all(torch.equal(x, y) for x, y in zip(d[:4], e[:4])) and torch.equal(d[5], e[5])
                ck[op] = {"paths": [d[6]["path"], e[6]["path"]], "labels_and_rows_agree": bool(same),
                          "rows_are_bincount": bool(torch.equal(d[5], want_rows)), "rows_sum": int(d[5].sum()),
                          "labels": [d[6]["n_index_labels"], d[6]["n_column_labels"]]}
                good = same and ck[op]["rows_are_bincount"] and ck[op]["rows_sum"] == n and ck[op]["labels"] == [k, k] and \
                    ck[op]["paths"] == [1 if (k + 1) * (k + 1) <= 4096 else 2, 2]
                if op == "sum":
                    for which, got in (("direct", d[4]), ("general", e[4])):
                        err = float(((got - want_sum).abs() / want_sum.abs().clamp_min(1.0)).max())
                        ck[op]["sum_rel_err_" + which] = err
                        good = good and err < 1e-9
                else:
                    good = good and bool(torch.equal(d[4], want_rows.to(torch.float64)))
                ok = ok and good
            groups = ctx.groupby_compute(list(view[name]), n, [vcol], [(0, L.COUNT)])
            ck["groupby_groups"] = groups
            ok = ok and groups == k * k
            checks[name] = ck
            print("checked %s: %s, %.1f s" % (name, "ok" if ok else "FAILED", time.time() - t0), flush=True)
    print(json.dumps(checks), flush=True)

    calls = {"copy": lambda: torch.clone(keys["uniform_10"][0])}
    for k in GRIDS:
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            for op in ops:
                calls["%s_%s_direct" % (name, op)] = pivot_call(name, op, 1)
                calls["%s_%s_general" % (name, op)] = pivot_call(name, op, 2)
                calls["%s_%s_groupby" % (name, op)] = groupby_call(name, op)
            calls[name + "_distinct"] = distinct_call(name)
    for _ in range(2):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    print("warmed up, %.1f s" % (time.time() - t0), flush=True)
    ms = {k: [] for k in calls}
    stream = {}
    for _ in range(max(a.reps, 20)):                            # one repeat of every call per round: the repeats alternate
        for k, fn in calls.items():
            ms[k].append(once(fn))
        for key, ph in phases.items():
            stream.setdefault(key, {"estimate": [], "aggregate": []})
            for p in ("estimate", "aggregate"):
                stream[key][p].append(ph.get(p, 0.0))
    ctx.set_option("pivot_path", 0)
    ctx.set_option("distinct_path", 0)
    r = {"rows": n}
    for k, v in ms.items():
        r[k + "_ms"] = {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    med = lambda k: r[k + "_ms"]["median"]                      # noqa: E731
    spread = lambda k: r[k + "_ms"]["max"] - r[k + "_ms"]["min"]        # noqa: E731
    smed = lambda key, p: float(np.median(stream[key][p]))      # noqa: E731
    gates = {}
    for k in GRIDS:
        direct_taken = (k + 1) * (k + 1) <= 4096
        for kind in ("uniform", "hot"):
            name = "%s_%d" % (kind, k)
            for op in ops:
                d, e, b = "%s_%s_direct" % (name, op), "%s_%s_general" % (name, op), "%s_%s_groupby" % (name, op)
                r["gate_3_%s_%s_general_over_groupby" % (name, op)] = med(e) / med(b)
                if not direct_taken:
                    continue
                r["%s_%s_direct_over_general" % (name, op)] = med(d) / med(e)
                gates["gate_1_direct_no_slower_than_general_%s_%s" % (name, op)] = med(d) <= med(e) + max(spread(d), spread(e))
                r["%s_%s_census_ms" % (name, op)] = smed((name, op, 1), "estimate")
                r["%s_%s_stream_ms" % (name, op)] = smed((name, op, 1), "aggregate")
                r["%s_%s_stream_over_copy" % (name, op)] = r["%s_%s_stream_ms" % (name, op)] / med("copy")
            if direct_taken:
                r[name + "_distinct_stream_ms"] = smed((name, "distinct"), "aggregate")
                r["gate_2_%s_rows_stream_over_distinct_stream" % name] = r[name + "_rows_stream_ms"] / r[name + "_distinct_stream_ms"]
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
