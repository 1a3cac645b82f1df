"""The chain2 kind of experiments/fuzz_ops.py: chains across the column ops and the older ones, every intermediate left on the
device.  Seven shapes; expect_chain2 walks the references alone (each stage applied to the reference's own previous stage,
never to the device's), run_chain2 compares the device's intermediate with it stage by stage, so a wrong stage is reported
where it happens and cannot cancel out later.  The hand-overs the headers promise are the point: an eval or predicate bitmap
taken by filter_indices in place as a BOOLBITS column, the null mask fill / cumulative / eval write bytewise into a caller's
buffer at byte offset 1 read by the next call, topk rows as gather indices.

Every stage compares bit for bit but the two that carry a documented bound: cumulative SUM where the sums are not exact
integers (tests/cumulative_ref.compare_cells) and the groupby sums (1e-9 relative, as every groupby test).  Chains that go
on after a SUM hold small integers, so that the SUM itself is exact and the later stages can be compared by their bits.
The window_quantile shape stays at or below 65 537 rows: its twin is O(n log n) with a large constant."""
import ctypes as C

import numpy as np

from fuzz_common import DRY_MODE, L, Guarded, Mismatch, bits, check, check_guards, describe_case, first_diff_any, mask_of, place, release, to_np
from tests import cumulative_ref as CR
from tests import describe_ref as DR
from tests import eval_ref as ER
from tests import fill_ref as FR
from tests import predicate_ref as PR
from tests import rank_ref as RR
from tests import topk_ref as TR
from tests import window_quantile_ref as QR
from tests import window_ref as WR
from tests.sort_ref import Col, ref_lexsort

SHAPES = ("eval_mask_filter_cum", "predicate_filter_rank", "fill_cum_lag_window", "topk_gather_describe", "sort_gather_wquant_predicate",
          "eval_rank_isin", "join_gather_eval_groupby")
FIRST_SPACES = ("host", "device", "resident")
SIZES = (4097, 65_537, 300_007, 1_000_003)
CHAIN2_FEATURES = ["chain2.%s" % s for s in SHAPES] + ["chain2.first_stage_space=%s" % s for s in FIRST_SPACES]
OP = ER.OP


def small_ints(rng, n, null_p):
    x = rng.integers(-9, 10, n).astype(np.float64)
    return x, (rng.random(n) < null_p if null_p else None)


def draw_chain2(rng, case):
    shape = SHAPES[case % len(SHAPES)]
    n = int(rng.choice(SIZES[:2] if shape == "sort_gather_wquant_predicate" or DRY_MODE == 2 else SIZES))
    space = FIRST_SPACES[(case // len(SHAPES)) % 3] if rng.random() < 0.8 else str(rng.choice(FIRST_SPACES))
    d = dict(shape=shape, n=n, space=space)
    null_p = float(rng.choice([0.0, 0.1, 0.5]))
    if shape == "eval_mask_filter_cum":
        a = np.round(rng.normal(0, 50, n), 2)
        a[rng.random(n) < 0.05] = np.nan
        d.update(a=a, anull=rng.random(n) < 0.1 if rng.random() < 0.5 else None, b=rng.integers(-1000, 1000, n).astype(np.int64),
                 c=float(rng.choice([0.0, 500.0, -2000.0, 40_000.0])), cum_op=int(rng.choice([CR.SUM, CR.MAX])), fill=-1.5)
        d["v"], d["vnull"] = rng.normal(50, 20, n), (rng.random(n) < null_p if null_p else None)
    elif shape == "predicate_filter_rank":
        i64 = bool(rng.random() < 0.4)
        x = rng.integers(-500, 500, n).astype(np.int64) if i64 else np.round(rng.normal(0, 100, n))
        if not i64:
            x[rng.random(n) < 0.03] = np.nan
        d.update(x=x, xnull=rng.random(n) < null_p if null_p else None, op=int(rng.choice([PR.BETWEEN, PR.GT, PR.ISNA])), a=float(rng.choice([-50.0, 0.0, 120.0])),
                 b=float(rng.choice([60.0, 400.0])), method=int(rng.integers(0, 5)), i64=i64, fill=7)
    elif shape == "fill_cum_lag_window":
        x, _ = small_ints(rng, n, 0)
        miss = rng.random(n) < float(rng.choice([0.05, 0.4]))
        miss[:int(rng.integers(0, 4))] = True
        lo = int(rng.integers(0, n - 3000))
        miss[lo:lo + int(rng.integers(1, 2500))] = True
        as_bits = bool(rng.random() < 0.5)
        method = int(rng.choice([FR.FFILL, FR.LINEAR]))
        d.update(x=x if as_bits else np.where(miss, np.nan, x), xnull=miss if as_bits else None, method=method,
                 cum_op=CR.MAX if method == FR.LINEAR else int(rng.choice([CR.SUM, CR.MAX, CR.MIN])), periods=int(rng.choice([1, 2, 64, 2049])),
                 w=int(rng.choice([2, 3, 64])))
    elif shape == "topk_gather_describe":
        a = rng.integers(0, max(2, n // int(rng.choice([3, 50, 5000]))), n).astype(np.float64)
        a[rng.random(n) < 0.02] = np.nan
        d.update(a=a, anull=rng.random(n) < null_p if null_p else None, b=rng.integers(-2**62, 2**62, n, dtype=np.int64), bnull=rng.random(n) < 0.1,
                 k=int(rng.choice([1, 1000, n // 7, n // 4, n])), largest=bool(rng.random() < 0.5), ps=[0.0, 10.0, 50.0, 99.0, 100.0][:int(rng.integers(1, 6))])
    elif shape == "sort_gather_wquant_predicate":
        d.update(key=rng.integers(0, int(rng.choice([3, 500, 20_000])), n).astype(np.int64), fkey=rng.choice([0.5, -0.0, 0.0, 2.0, np.nan, -7.25], n),
                 asc=[bool(rng.random() < 0.5) for _ in range(2)], v=np.round(rng.normal(0, 30, n)), vnull=rng.random(n) < null_p if null_p else None,
                 w=int(rng.choice([3, 44, 45, 300])), gt=float(rng.choice([-10.0, 0.0, 25.0])), fill=float(rng.choice([0.0, -2.5])))
    elif shape == "eval_rank_isin":
        a, anull = small_ints(rng, n, null_p)
        a[rng.random(n) < 0.02] = np.nan
        d.update(a=a, anull=anull, b=rng.integers(1, 50, n).astype(np.int64), bnull=rng.random(n) < 0.1 if rng.random() < 0.5 else None,
                 method=int(rng.integers(0, 5)), m=int(rng.choice([1, 100, 4096, 4097, 50_000])))
    else:
        ng = int(rng.choice([3, 500, 20_000]))
        nr = int(rng.integers(max(ng // 2, 1), ng + 1))
        d.update(lkey=rng.integers(0, ng, n).astype(np.int64), lnull=rng.random(n) < 0.05 if rng.random() < 0.5 else None, rkey=rng.permutation(ng)[:nr].astype(np.int64),
                 nr=nr, how=int(rng.choice([L.INNER, L.LEFT])), a=rng.integers(-99, 100, n).astype(np.float64), rb=rng.integers(1, 9, nr).astype(np.int64))
    return d


def classify_chain2(d):
    return ["chain2.%s" % d["shape"], "chain2.first_stage_space=%s" % d["space"]]


def gathered(v, nulls, rows, fill):
    return v[rows] if nulls is None else np.where(nulls[rows], np.array(fill, v.dtype), v[rows])


def expect_chain2(d):
    """-> the references of every stage, each computed from the reference of the stage before."""
    if "want" in d:
        return d["want"]
    n, shape, w = d["n"], d["shape"], {}
    if shape == "eval_mask_filter_cum":
        w["program"] = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["MUL"], 0.0), (OP["CONST"], d["c"]), (OP["GT"], 0.0)]
        w["eval"] = ER.evaluate([(d["a"], d["anull"], L.F64), (d["b"], None, L.I64)], n, w["program"])
        rows = w["rows"] = np.flatnonzero(w["eval"].mask)
        w["val"] = gathered(d["v"], d["vnull"], rows, d["fill"])
        w["vnull"] = None if d["vnull"] is None else d["vnull"][rows]
        w["cum"] = CR.cum_twin(w["val"], w["vnull"], d["cum_op"])
    elif shape == "predicate_filter_rank":
        w["bits"], w["count"] = PR.predicate(d["x"], mask_of(d["xnull"]), d["op"], d["a"], d["b"])
        rows = w["rows"] = np.flatnonzero(np.unpackbits(w["bits"], count=n, bitorder="little"))
        w["val"] = gathered(d["x"], d["xnull"], rows, d["fill"])
        w["vnull"] = None if d["xnull"] is None else d["xnull"][rows]
        w["rank"] = RR.rank_ref(w["val"], w["vnull"], d["method"])
    elif shape == "fill_cum_lag_window":
        w["fill"] = FR.fill_twin(d["x"], d["xnull"], d["method"])
        w["cum"] = CR.cum_twin(w["fill"][0], w["fill"][1], d["cum_op"])
        w["lag"] = CR.lag_twin(w["cum"][0], w["cum"][1], CR.DIFF, d["periods"])
        w["window"] = WR.rolling_ref(w["lag"][0], ~w["lag"][1], d["w"], False, "mean", mp=1, ddof=1)
    elif shape == "topk_gather_describe":
        rows, w["numbers"] = TR.topk_ref(d["a"], d["anull"], d["k"], d["largest"])
        w["rows"] = rows
        w["ga"] = gathered(d["a"], d["anull"], rows, -1.5)
        w["gb"] = gathered(d["b"], d["bnull"], rows, -42)
    elif shape == "sort_gather_wquant_predicate":
        order = w["order"] = ref_lexsort([Col(L.I64, d["key"]), Col(L.F64, d["fkey"])], d["asc"])
        w["val"] = gathered(d["v"], d["vnull"], order, d["fill"])
        w["wq"] = QR.window_quantile_fast(w["val"], None, "rolling", d["w"], False, 1, True, 0.5, False)
        w["count"] = PR.predicate(w["wq"], None, PR.GT, d["gt"])[1]
    elif shape == "eval_rank_isin":
        w["program"] = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["MUL"], 0.0), (OP["COL"], 0.0), (OP["ADD"], 0.0)]
        w["eval"] = ER.evaluate([(d["a"], d["anull"], L.F64), (d["b"], d["bnull"], L.I64)], n, w["program"])
        w["rank"] = RR.rank_ref(w["eval"].values, w["eval"].nulls, d["method"])
        w["vals"] = np.arange(1, d["m"] + 1, dtype=np.float64) * 2.0 - 1.5 * (d["method"] == RR.AVERAGE)
        w["bits"], w["count"] = PR.isin(w["rank"], None, L.F64, w["vals"], L.F64)
    else:
        from oracle import oracle as O
        li, ri = O.join_indices((d["lkey"], mask_of(d["lnull"]), O.I64), n, (d["rkey"], None, O.I64), d["nr"], d["how"])
        w["li"], w["ri"] = li, ri
        miss = ri < 0
        w["key"] = d["lkey"][li]
        w["a"] = d["a"][li]
        w["b"] = np.where(miss, 1, d["rb"][np.where(miss, 0, ri)]).astype(np.int64)
        w["program"] = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["MUL"], 0.0)]
        w["eval"] = ER.evaluate([(w["a"], None, L.F64), (w["b"], None, L.I64)], len(li), w["program"])
        w["groups"] = O.groupby_agg([(w["key"], None, O.I64)], len(li), [(w["eval"].values, None, O.F64)], [(0, O.SUM)]) if len(li) else None
    d["want"] = w
    return w


def same(what, got, want):
    got = to_np(got)
    if want.dtype == np.uint32 and got.dtype == np.int32:
        got = got.view(np.uint32)
    check(got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what, first_diff_any(got, want))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def join_gather_device(ctx, col, n_src, n_out, side, fill, keep):
    """pandrs_hip_join_gather with its output left on the device (Context.join_gather fetches it)."""
    import torch
    cc, sp = ctx._cols([tuple(col)], keep)
    dtype = tuple(col)[2]
    out = torch.empty(max(int(n_out), 1), dtype=torch.float64 if dtype == L.F64 else torch.int64, device="cuda:0")
    fill_bits = int(np.float64(fill).view(np.uint64)) if dtype == L.F64 else int(fill) & 0xFFFFFFFFFFFFFFFF
    st = ctx.lib.pandrs_hip_join_gather(ctx.h, sp, cc, int(n_src), int(side), C.c_uint64(fill_bits), L.MEM_DEVICE, out.data_ptr())
    check(st == 0, "join_gather status", (st, L.last_error()))
    return out[:n_out]


def run_chain2(ctx, d):
    import torch  # noqa: F401
    n, shape, keep, guards = d["n"], d["shape"], [], []
    w = expect_chain2(d)
    up = lambda data, nulls, dtype, rows=n: place(ctx, d["space"], data, mask_of(nulls), dtype, rows, keep)   # noqa: E731
    nbytes = (n + 7) // 8

    def own_mask(k):
        g = Guarded((k + 7) // 8, np.uint8)
        guards.append(g)
        return g.view

    def own_cells(k, dt=np.float64):
        g = Guarded(k, dt)
        guards.append(g)
        return g.view

    def compact(rows, cnt, v, vnull, fill, dtype):
        """filter_gather of a value column and of its null flags, the flags packed into a bitmap: all on the device."""
        d_val = ctx.filter_gather(up(v, vnull, dtype), n, cnt, fill, out_device=True)
        same("filter_gather", d_val, w["val"])
        if vnull is None:
            return d_val, None
        flags = ctx.filter_gather(up(bits(vnull), None, L.BOOLBITS), n, cnt, 0, out_device=True)
        same("filter_gather of the null flags", flags, w["vnull"].astype(np.uint8))
        d_mask = ctx.bytes_to_bitmap(flags)
        same("bytes_to_bitmap", d_mask, bits(w["vnull"]))
        return d_val, d_mask

    try:
        if shape == "eval_mask_filter_cum":
            out = own_mask(n)
            got, cnt = ctx.eval([up(d["a"], d["anull"], L.F64), up(d["b"], None, L.I64)], n, w["program"], out=out)
            same("eval mask", got, ER.pack(w["eval"].mask))
            check(cnt == w["eval"].count, "eval count", (cnt, w["eval"].count))
            idx, sel = ctx.filter_indices((out, None, L.BOOLBITS), n)         # the buffer eval wrote, in place
            check(sel == len(w["rows"]), "filter count", (sel, len(w["rows"])))
            same("filter rows", idx, w["rows"])
            if sel:
                d_val, d_mask = compact(w["rows"], sel, d["v"], d["vnull"], d["fill"], L.F64)
                vals, mask, n_null = ctx.cumulative((d_val, d_mask, L.F64), sel, d["cum_op"])
                want, gone = w["cum"]
                try:
                    CR.compare_cells(d["cum_op"], to_np(vals), want, w["val"], w["vnull"], False)
                except AssertionError as e:
                    raise Mismatch("cumulative after the gather: %s" % (e,))
                check(n_null == int(gone.sum()) and (mask is None) == (n_null == 0), "cumulative null count", (n_null, int(gone.sum())))
                if mask is not None:
                    same("cumulative mask", mask, bits(gone))
        elif shape == "predicate_filter_rank":
            dt = L.I64 if d["i64"] else L.F64
            got, cnt = ctx.predicate(up(d["x"], d["xnull"], dt), n, d["op"], d["a"], d["b"], out_device=True)
            same("predicate bits", got, w["bits"])
            check(cnt == w["count"], "predicate count", (cnt, w["count"]))
            idx, sel = ctx.filter_indices((got, None, L.BOOLBITS), n)
            same("filter rows", idx, w["rows"])
            if sel:
                d_val, d_mask = compact(w["rows"], sel, d["x"], d["xnull"], d["fill"], dt)
                same("rank of the gathered column", ctx.rank((d_val, d_mask, dt), sel, d["method"]), w["rank"])
        elif shape == "fill_cum_lag_window":
            f_out, f_mask = own_cells(n), own_mask(n)
            ctx.fill(up(d["x"], d["xnull"], L.F64), n, d["method"], out=f_out, out_mask=f_mask)
            same("fill values", f_out, w["fill"][0])
            same("fill mask", f_mask, bits(w["fill"][1]))
            c_out, c_mask = own_cells(n), own_mask(n)
            ctx.cumulative((f_out, f_mask, L.F64), n, d["cum_op"], out=c_out, out_mask=c_mask)     # the mask at byte offset 1, the cells at 8 mod 16
            try:
                CR.compare_cells(d["cum_op"], to_np(c_out), w["cum"][0], w["fill"][0], w["fill"][1], d["method"] == FR.FFILL)
            except AssertionError as e:
                raise Mismatch("cumulative after fill: %s" % (e,))
            same("cumulative mask", c_mask, bits(w["cum"][1]))
            l_out, l_mask = own_cells(n), own_mask(n)
            ctx.lag((c_out, c_mask, L.F64), n, CR.DIFF, d["periods"], out=l_out, out_mask=l_mask)
            same("lag diff values", l_out, w["lag"][0])
            same("lag diff mask", l_mask, bits(w["lag"][1]))
            got = ctx.window((l_out, l_mask, L.F64), n, L.WINDOW_KIND_ROLLING, L.WINDOW_MEAN, window=d["w"], min_periods=1)
            check(WR.same(to_np(got), w["window"]), "rolling mean after the lag", WR.first_diff(to_np(got), w["window"]))
        elif shape == "topk_gather_describe":
            rows, numbers = ctx.topk(up(d["a"], d["anull"], L.F64), n, d["k"], d["largest"], out_device=True)
            same("topk rows", rows, w["rows"])
            check(numbers == w["numbers"], "topk numbers", (numbers, w["numbers"]))
            ga = ctx.gather(dev(d["a"]), None if d["anull"] is None else dev(bits(d["anull"])), rows, -1.5, L.F64)
            gb = ctx.gather(dev(d["b"]), dev(bits(d["bnull"])), rows, -42, L.I64)
            same("gather a by the topk rows", ga, w["ga"])
            same("gather b by the topk rows", gb, w["gb"])
            k = len(w["rows"])
            try:
                DR.compare_describe(ctx.describe((ga, None, L.F64), k), w["ga"], None, np.float64, False)
                q, cnt = ctx.quantiles((gb, None, L.I64), k, d["ps"])
                DR.compare_quantiles(q, cnt, w["gb"], None, np.int64, d["ps"])
            except AssertionError as e:
                raise Mismatch("describe / quantiles of the gathered columns: %s" % (e,))
        elif shape == "sort_gather_wquant_predicate":
            order = ctx.sort_indices([up(d["key"], None, L.I64), up(d["fkey"], None, L.F64)], n, d["asc"])
            same("sort order", order, w["order"])
            g = ctx.gather(dev(d["v"]), None if d["vnull"] is None else dev(bits(d["vnull"])), order, d["fill"], L.F64)
            same("gather by the sort order", g, w["val"])
            wq = ctx.window_quantile((g, None, L.F64), n, L.WINDOW_KIND_ROLLING, median=True, window=d["w"], min_periods=1)
            check(WR.same(to_np(wq), w["wq"]), "rolling median of the sorted column", WR.first_diff(to_np(wq), w["wq"]))
            none, cnt = ctx.predicate((wq, None, L.F64), n, L.PRED_GT, d["gt"], count_only=True)
            check(none is None and cnt == w["count"], "predicate count over the medians", (cnt, w["count"]))
        elif shape == "eval_rank_isin":
            e_out, e_mask = own_cells(n), own_mask(n)
            ctx.eval([up(d["a"], d["anull"], L.F64), up(d["b"], d["bnull"], L.I64)], n, w["program"], out=e_out, out_mask=e_mask)
            same("eval values", e_out, w["eval"].values)
            same("eval mask", e_mask, ER.pack(w["eval"].nulls))
            r = ctx.rank((e_out, e_mask, L.F64), n, d["method"])
            same("rank of the eval output", r, w["rank"])
            got, cnt = ctx.isin((r, None, L.F64), n, (w["vals"], None, L.F64), out_device=True)
            same("isin of the ranks", got, w["bits"])
            _, sel = ctx.filter_indices((got, None, L.BOOLBITS), n, indices=False)
            check(cnt == w["count"] and sel == w["count"], "isin / filter count", (cnt, sel, w["count"]))
        else:
            from oracle import oracle as O
            from tests.helpers import assert_groupby_equal
            lk, rk = up(d["lkey"], d["lnull"], L.I64), up(d["rkey"], None, L.I64, d["nr"])
            li, ri = ctx.join_indices(lk, n, rk, d["nr"], d["how"])      # the pairs land where the keys live
            n_pairs = int(li.shape[0])
            same("join left rows", li, w["li"])
            same("join right rows", ri, w["ri"])
            check(n_pairs == len(w["li"]), "join pairs", (n_pairs, len(w["li"])))
            if n_pairs:
                gk = join_gather_device(ctx, lk, n, n_pairs, 0, 0, keep)
                ga = join_gather_device(ctx, up(d["a"], None, L.F64), n, n_pairs, 0, 0.0, keep)
                gb = join_gather_device(ctx, up(d["rb"], None, L.I64, d["nr"]), d["nr"], n_pairs, 1, 1, keep)
                same("join_gather key", gk, w["key"])
                same("join_gather a", ga, w["a"])
                same("join_gather b", gb, w["b"])
                vals, mask, n_null = ctx.eval([(ga, None, L.F64), (gb, None, L.I64)], n_pairs, w["program"])
                same("eval a * b", vals, w["eval"].values)
                got = tuple(t.cpu().numpy() for t in ctx.groupby_agg([(gk, None, L.I64)], n_pairs, [(vals, None, L.F64)], [(0, L.SUM)]))
                try:
                    assert_groupby_equal((got[0].view(np.uint64), got[1], got[2]), w["groups"], [O.I64], rtol=1e-9)
                except AssertionError as e:
                    raise Mismatch("groupby sum by the gathered key: %s" % (e,))
        check_guards(guards)
    finally:
        release(keep)


KINDS = {"chain2": (draw_chain2, classify_chain2, run_chain2, lambda d: describe_case("chain2", d), CHAIN2_FEATURES, expect_chain2)}
