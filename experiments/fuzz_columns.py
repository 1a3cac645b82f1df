"""The column ops' kinds of experiments/fuzz_ops.py: describe / quantiles, rank, fill, topk / arg_extreme, predicate / isin,
window_quantile (wquant), cumulative / lag (cum) and eval, each against its twin under tests/*_ref.py by the rule its
directed GPU test uses (bit for bit everywhere but cumulative SUM / PROD and describe's moments, which carry the bounds
tests/cumulative_ref.py and tests/describe_ref.py state).

Every kind draws, on top of its own features, the input space, the output placement (host, device, a caller's device buffer
at 8 mod 16 / byte offset 1 between guard cells), the dtype, the null layout, special cells and a row-count class
(fuzz_common.shared_draw).  The structured part of a case is the case number modulo small strides, so a run of a few
hundred cases reaches every ledger line; one draw in five strays from the structure so that the dimensions mix.

A documented refusal is a case of its own that expects the status (never a skipped draw).  Documented limits the generators
stay inside: cumulative PROD is drawn from the inputs of tests/test_gpu_cumulative.py (factors near one, range excursions,
zeros and infinities, small integers) - the contract of a product that leaves f64's range elsewhere than there is the
sticky rewrite, not the sequential fold; an eval program whose MAX / MIN meets +0.0 and -0.0 in one row (the library, like
Rust, does not fix which comes back) has its MAX / MIN replaced by ADD / SUB; arg_extreme's twin is a Python loop, so its
cases stay at or below 70 000 rows; a resident or offset column has at least one row."""
import os
import re

import numpy as np

from fuzz_common import (DRY_MODE, HEADER, I64_MAX, I64_MIN, OUTS, ROOT, L, Mismatch, bits, check, check_guards, describe_case,
                         expect_status, first_diff_any, geometry, grid_checked, mask_of, nulls_of, out_kwargs, pick, place, plain_column,
                         release, shared_classify, shared_draw, shared_features, sprinkle, to_np)
from tests import cumulative_ref as CR
from tests import describe_ref as DR
from tests import eval_ref as ER
from tests import fill_ref as FR
from tests import predicate_ref as PR
from tests import rank_ref as RR
from tests import topk_ref as TR
from tests import window_quantile_ref as QR
from tests.window_ref import first_diff as w_first_diff
from tests.window_ref import same as w_same

NUM = (L.I64, L.F64)
DRY2_MAX_N = 300_000 if DRY_MODE == 2 else None                 # FUZZ_DRY=2 is a CPU-only test: no grid-sized twin runs


def same_u64(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def asserting(fn, *args):
    """A comparison rule shared with a directed test raises AssertionError; here that is a mismatch of the case."""
    try:
        fn(*args)
    except Mismatch:
        raise
    except AssertionError as e:
        raise Mismatch("%s: %s" % (fn.__name__, e))


def check_cells(got, want, gone, guards, n):
    """(values, mask, count) of fill / cumulative / lag / eval against the twin's (values, flags): the cells bit for bit, the
    count, `mask is None` exactly without a bit, the bitmap bytewise; a caller's mask buffer holds the bitmap either way."""
    vals, mask, cnt = got
    vals = to_np(vals)
    check(same_u64(vals, want), "cells", first_diff_any(vals, want))
    check(cnt == int(gone.sum()), "count", (cnt, int(gone.sum())))
    check((mask is None) == (cnt == 0), "mask is None exactly when no bit is set", (mask is None, cnt))
    if mask is not None:
        check(np.array_equal(to_np(mask), bits(gone)), "null bitmap", first_diff_any(to_np(mask), bits(gone)))
    if len(guards) == 2 and n:
        check(np.array_equal(to_np(guards[1].view), bits(gone)), "the caller's mask buffer: ceil(n / 8) bytes, tail bits 0",
              first_diff_any(to_np(guards[1].view), bits(gone)))
    check_guards(guards)


# ==== cum: cumulative and lag ===================================================================================================
CUM_T, CUM_P = geometry("cum")
CUM_WHICH = [("cum", op) for op in CR.CUM_OPS] + [("lag", op) for op in CR.LAG_OPS]
CUM_NAME = dict(zip(CUM_WHICH, ("cumulative sum", "cumulative prod", "cumulative max", "cumulative min", "cumulative count", "lag shift",
                                "lag diff", "lag pct_change")))
PERIOD_BODIES = ("1", "63", "64", "65", "(tile-1)", "(tile+1)", "(n-1)", "n", "(n+1)")
PERIODS = ("0",) + tuple(s + b for b in PERIOD_BODIES for s in "+-")
CUM_LAYOUTS = ("normal", "small integers", "prod factors near one", "prod range excursion", "prod zeros and infinities")
CUM_FEATURES = (shared_features("cum", NUM) + ["cum.%s" % v for v in CUM_NAME.values()] + ["cum.periods=%s" % p for p in PERIODS] +
                ["cum.layout=%s" % s for s in CUM_LAYOUTS] + ["cum.refusal: diff with negative periods"])


def periods_of(name, n, tile):
    if name == "0":
        return 0
    v = {"1": 1, "63": 63, "64": 64, "65": 65, "(tile-1)": tile - 1, "(tile+1)": tile + 1, "(n-1)": n - 1, "n": n, "(n+1)": n + 1}[name[1:]]
    return max(v, 0) * (-1 if name[0] == "-" else 1)


def prod_column(rng, n, layout):
    """The PROD inputs of tests/test_gpu_cumulative.py at n rows."""
    T = CUM_T
    x = np.exp(rng.normal(0.0, 0.1 if layout == "prod factors near one" else 0.05, n)) * rng.choice([-1.0, 1.0], n)
    if layout == "prod range excursion":
        if rng.random() < 0.5:                                  # the sticky rewrite: an overflow or an underflow, then the way back
            at = int(rng.choice([5, T - 2, 2 * T - 2, 3 * T + 1, int(rng.integers(1, n - 8))]))
            at = at if at + 6 < n else 1
            big, back = ((1e200, 1e-200), (1e-200, 1e200))[int(rng.integers(0, 2))]
            x[at], x[at + 1] = big, big
            x[at + 3:at + 6] = back
            later = [None, 0.0, np.inf][int(rng.integers(0, 3))]
            if later is not None and at + 2 * T + 1 < n:
                x[at + 2 * T + 1] = later
        else:                                                   # rows 1 .. 2 alone overflow, no running product does
            x = np.ones(n)
            first = int(rng.choice([2, 3, 511, T - 1, T + 127, int(rng.integers(1, n - 3))]))
            first = first if first + 2 < n else 1
            x[first - 1], x[first], x[first + 1], x[first + 2] = 1e-200, 1e200, 1e200, 1e-200
    elif layout == "prod zeros and infinities":
        rows = rng.choice(n, size=min(n, int(rng.integers(1, 3))), replace=False)
        x[rows] = rng.choice([0.0, -0.0, np.inf, -np.inf], len(rows))
        for edge in (T - 1, T, 2 * T - 1, 2 * T, 0, n - 1):
            if edge < n and rng.random() < 0.15:
                x[edge] = rng.choice([0.0, -0.0, np.inf, -np.inf])
    return x


def draw_cum(rng, case):
    d = shared_draw(rng, case, CUM_T, CUM_P, NUM, max_n=DRY2_MAX_N)
    n = d["n"]
    d["refusal"] = case % 27 == 8
    fam, op = CUM_WHICH[case % 9 if case % 9 < 8 else int(rng.integers(0, 8))]
    pname = "0"
    if fam == "lag":
        pname = pick(rng, case, PERIODS, 9)
        if pname[0] == "-":
            op = CR.SHIFT
    if d["refusal"]:
        fam, op, pname, d["n"], d["size"], n = "lag", CR.DIFF, "-1", max(n, 1), d["size"] if n else "1", max(n, 1)
    layout = str(rng.choice(CUM_LAYOUTS[:2]))
    if (fam, op) == ("cum", CR.PROD):
        layout = pick(rng, case, CUM_LAYOUTS[1:], 9)
        if layout != "small integers" and n < 16:
            layout = "small integers"
    if layout.startswith("prod"):
        d["dtype"], d["specials"] = L.F64, False
        x = prod_column(rng, n, layout)
    elif layout == "small integers":
        x = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 2.0, 4.0]), n)
        x = x.astype(np.int64) if d["dtype"] == L.I64 else x
        if op == CR.PROD and (fam, op) == ("cum", CR.PROD):
            d["specials"] = False
        x = sprinkle(rng, x) if d["specials"] else x
    else:
        x = plain_column(rng, n, d["dtype"], d["specials"])
    d.update(fam=fam, op=op, pname=pname, periods=periods_of(pname, n, CUM_T), layout=layout, x=x, nl=nulls_of(rng, n, d["nulls"]),
             exact=layout == "small integers" and not d["specials"])
    return d


def classify_cum(d):
    if d["refusal"]:
        return ["cum.refusal: diff with negative periods"]
    f = shared_classify("cum", d) + ["cum.%s" % CUM_NAME[(d["fam"], d["op"])], "cum.layout=%s" % d["layout"]]
    if d["fam"] == "lag":
        f.append("cum.periods=%s" % d["pname"])
    return f


def expect_cum(d):
    if "want" not in d and not d["refusal"]:
        d["want"] = CR.cum_twin(d["x"], d["nl"], d["op"]) if d["fam"] == "cum" else CR.lag_twin(d["x"], d["nl"], d["op"], d["periods"])
    return d.get("want")


def run_cum(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.lag(col, n, CR.DIFF, -1), L.ERR_INVALID_ARGUMENT, "lag diff, periods -1")
        want, gone = expect_cum(d)
        kw, guards = out_kwargs(d["outp"], n, np.int64 if (d["fam"], d["op"]) == ("cum", CR.COUNT) else np.float64, True)
        got = ctx.cumulative(col, n, d["op"], **kw) if d["fam"] == "cum" else ctx.lag(col, n, d["op"], d["periods"], **kw)
        if d["fam"] == "cum":                                    # the cells by the op's contract, the rest as everywhere
            vals = to_np(got[0])
            check(vals.dtype == want.dtype and vals.shape == want.shape, "dtype and shape", (vals.dtype, vals.shape))
            asserting(CR.compare_cells, d["op"], vals, want, d["x"], d["nl"], d["exact"])
            got = (want, got[1], got[2])
        check_cells(got, want, gone, guards, n)
        grid_checked(d, "cum", "cum")
    finally:
        release(keep)


# ==== fill ====================================================================================================================
FILL_T, FILL_P = geometry("fill")
FILL_NAME = {FR.FFILL: "ffill", FR.BFILL: "bfill", FR.LINEAR: "linear", FR.VALUE: "value"}
GAPS = ("1", "63", "64", "65", "tile-1", "tile", "tile+1", "longer than a tile", "leading", "trailing", "whole column", "random",
        "fill_ref.sweep_cases")
FILL_VALUES = {L.F64: ("NaN", "-0.0", "1.5"), L.I64: ("an i64 beyond 2^53", "-42")}
FILL_VALUE_OF = {"NaN": float("nan"), "-0.0": -0.0, "1.5": 1.5, "an i64 beyond 2^53": 2**53 + 1, "-42": -42}
FILL_FEATURES = (shared_features("fill", NUM) + ["fill.method=%s" % v for v in FILL_NAME.values()] + ["fill.gap=%s" % g for g in GAPS] +
                 ["fill.value=%s" % v for vs in FILL_VALUES.values() for v in vs] + ["fill.gaps as NaN cells", "fill.gaps as null bits",
                                                                                    "fill.refusal: the output over the column"])


def gap_rows(rng, n, gap):
    """-> (missing rows, the row count the layout needs)"""
    T = FILL_T
    g = {"1": 1, "63": 63, "64": 64, "65": 65, "tile-1": T - 1, "tile": T, "tile+1": T + 1, "longer than a tile": T + int(rng.integers(2, 2 * T))}.get(gap)
    if g is not None:
        n = max(n, g + 3 + int(rng.integers(0, 2 * T)))
        miss, pos = np.zeros(n, bool), int(rng.integers(1, 5))
        while True:
            miss[pos:pos + g] = True
            pos += g + int(rng.integers(1, 2 * g + 6))
            if pos + g >= n - 1:
                break
        return miss, n
    n = max(n, 2)
    miss = np.zeros(n, bool)
    if gap == "leading":
        miss[:int(rng.integers(1, min(n - 1, T + 5) + 1))] = True
    elif gap == "trailing":
        miss[n - int(rng.integers(1, min(n - 1, T + 5) + 1)):] = True
    elif gap == "whole column":
        miss[:] = True
    else:
        miss = rng.random(n) < rng.choice([0.1, 0.5, 0.9])
    return miss, n


def draw_fill(rng, case):
    d = shared_draw(rng, case, FILL_T, FILL_P, NUM, max_n=DRY2_MAX_N)
    d["refusal"] = case % 29 == 28
    method, gap = pick(rng, case, FR.METHODS), pick(rng, case, GAPS, 4)
    value = None
    if d["refusal"]:
        d.update(space="device", dtype=L.F64, n=max(d["n"], 8), size="other")
        gap = "random"
    n = d["n"]
    if gap == "fill_ref.sweep_cases":
        for x, nl, method, value in FR.sweep_cases(rng, cases=1 + int(rng.integers(0, 4)), tile=FILL_T):
            pass
        d.update(n=x.shape[0], size="other", dtype=L.I64 if x.dtype == np.int64 else L.F64, nulls=None, specials=False)
        as_nan = as_bits = False
        x = x.astype(np.int64) if x.dtype == np.int64 else x
    else:
        if d["size"] == "grid+1" or n < 2 or d["nulls"] in ("p=0.5", "all null"):
            gap = "random"                                      # the row count, or the null layout, is the point of the case
            miss = rng.random(n) < 0.3
        else:
            miss, n2 = gap_rows(rng, n, gap)
            if n2 != n:
                d.update(n=n2, size="other")
                n = n2
        x = plain_column(rng, n, d["dtype"], d["specials"])
        as_bits = d["nulls"] in ("p=0.01", "p=0.5", "all null") or (d["dtype"] == L.I64 and d["nulls"] != "no mask" and gap != "random")
        as_nan = not as_bits and d["dtype"] == L.F64
        nl = nulls_of(rng, n, d["nulls"])
        if as_bits:
            nl = (np.zeros(n, bool) if nl is None else nl) | miss
        elif as_nan:
            x[miss] = np.nan
        else:
            gap = "random"                                      # an I64 column without a mask: nothing is missing
    if method == FR.VALUE and value is None:
        vk = pick(rng, case, FILL_VALUES[d["dtype"]], 4)
        value = FILL_VALUE_OF[vk]
    d.update(method=method, gap=gap, value=value, x=x, nl=nl, as_nan=as_nan, as_bits=as_bits)
    return d


def classify_fill(d):
    if d["refusal"]:
        return ["fill.refusal: the output over the column"]
    f = shared_classify("fill", d) + ["fill.method=%s" % FILL_NAME[d["method"]], "fill.gap=%s" % d["gap"]]
    if d["method"] == FR.VALUE:
        v = d["value"]
        name = "NaN" if v != v else "-0.0" if (v == 0 and np.signbit(v)) else "an i64 beyond 2^53" if (d["dtype"] == L.I64 and abs(v) > 2**53) else "1.5" if v == 1.5 else "-42" if v == -42 else None
        if name:
            f.append("fill.value=%s" % name)
    if d["gap"] not in ("random", "fill_ref.sweep_cases"):
        f.append("fill.gaps as NaN cells" if d["as_nan"] else "fill.gaps as null bits")
    return f


def expect_fill(d):
    if "want" not in d and not d["refusal"]:
        d["want"] = FR.fill_twin(d["x"], d["nl"], d["method"], d["value"])
    return d.get("want")


def run_fill(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.fill(col, n, FR.FFILL, out=col[0]), L.ERR_INVALID_ARGUMENT, "fill in place")
        want, gone = expect_fill(d)
        kw, guards = out_kwargs(d["outp"], n, want.dtype, True)
        check_cells(ctx.fill(col, n, d["method"], d["value"], **kw), want, gone, guards, n)
        grid_checked(d, "fill", "fill")
    finally:
        release(keep)


# ==== rank ====================================================================================================================
RANK_T, RANK_P = geometry("rank")
RANK_NAME = ("average", "min", "max", "first", "dense")
RANK_LAYOUTS = ("a tie run ends on a tile edge", "a tie run ends before a tile edge", "a tie run ends after a tile edge",
                "one run over the whole column", "all distinct", "random", "rank_ref.sweep_cases")
DIGIT_BITS = (0, 4, 5, 6, 7, 8)
RANK_FEATURES = (shared_features("rank", NUM) + ["rank.method=%s" % m for m in RANK_NAME] + ["rank.layout=%s" % s for s in RANK_LAYOUTS] +
                 ["rank.sort_digit_bits=%d" % b for b in DIGIT_BITS] + ["rank.reaches: %s" % f for f in RR.FEATURES] +
                 ["rank.refusal: a method outside the enum"])


def draw_rank(rng, case):
    d = shared_draw(rng, case, RANK_T, RANK_P, NUM, max_n=DRY2_MAX_N)
    d["refusal"] = case % 23 == 22
    method, layout, digit_bits = pick(rng, case, RR.METHODS), pick(rng, case, RANK_LAYOUTS, 5), pick(rng, case, DIGIT_BITS, 3)
    t, n = RANK_T, d["n"]
    if d["size"] in ("0", "1", "2", "grid+1") and layout not in ("one run over the whole column", "all distinct", "random"):
        layout = "random"
    if layout == "rank_ref.sweep_cases":
        x, nl, method, digit_bits = next(iter(RR.sweep_cases(seed=int(rng.integers(0, 2**31)), count=1)))
        d.update(n=x.shape[0], size="other", dtype=L.I64 if x.dtype == np.int64 else L.F64, nulls=None, specials=False)
    elif layout.startswith("a tie run"):
        shift = {"on": 0, "before": -1, "after": 1}[layout.split()[4]]
        k = int(rng.integers(1, 3))                              # the edge of tile k, in sorted positions
        runs = [k * t - 3 + shift, 3, 5, int(rng.integers(1, t)), 7]
        x = np.repeat(np.arange(len(runs), dtype=np.float64) * 0.5 - 3.0, runs)
        x = rng.permutation(x) if rng.random() < 0.7 else x
        x = (x * 2).astype(np.int64) if d["dtype"] == L.I64 else x
        d.update(n=x.shape[0], size="other", nulls=str(rng.choice(["no mask", "mask without a bit"])), specials=False)
        nl = nulls_of(rng, d["n"], d["nulls"])
    else:
        if layout == "one run over the whole column":
            x = np.full(n, 7 if d["dtype"] == L.I64 else 2.5, np.int64 if d["dtype"] == L.I64 else np.float64)
        elif layout == "all distinct":
            x = rng.permutation(n).astype(np.int64 if d["dtype"] == L.I64 else np.float64) - n // 2
        else:
            x = plain_column(rng, n, d["dtype"], False)
        x = sprinkle(rng, x) if d["specials"] else x
        nl = nulls_of(rng, n, d["nulls"])
    d.update(method=int(method), layout=layout, digit_bits=int(digit_bits), x=x, nl=nl)
    return d


def classify_rank(d):
    if d["refusal"]:
        return ["rank.refusal: a method outside the enum"]
    return (shared_classify("rank", d) + ["rank.method=%s" % RANK_NAME[d["method"]], "rank.layout=%s" % d["layout"],
                                          "rank.sort_digit_bits=%d" % d["digit_bits"]] +
            ["rank.reaches: %s" % f for f in RR.rank_features(d["x"], d["nl"], RANK_T)])


def expect_rank(d):
    if "want" not in d and not d["refusal"]:
        d["want"] = RR.rank_ref(d["x"], d["nl"], d["method"])
    return d.get("want")


def run_rank(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.rank(col, n, 5), L.ERR_INVALID_ARGUMENT, "rank method 5")
        want = expect_rank(d)
        kw, guards = out_kwargs(d["outp"], n, np.float64, False)
        ctx.set_option("sort_digit_bits", d["digit_bits"])
        try:
            got = to_np(ctx.rank(col, n, d["method"], **kw))
        finally:
            ctx.set_option("sort_digit_bits", 0)
        check(same_u64(got, want), "ranks", first_diff_any(got, want))
        check_guards(guards)
        grid_checked(d, "rank", "rank")
    finally:
        release(keep)


# ==== topk and arg_extreme ======================================================================================================
TOPK_T, TOPK_P = geometry("topk")
CUT_NUM, CUT_DEN = map(int, re.search(r"topk_cutover = (\d+) / (\d+)", HEADER).groups())
TOPK_WHICH = ("topk largest", "topk smallest", "arg_extreme")
K_CLASSES = ("0", "1", "n-1", "n", "n+1", "cut-over-1", "cut-over", "cut-over+1")
TOPK_LAYOUTS = ("ties", "1 byte varies", "3 bytes vary", "8 bytes vary", "plain")
TOPK_FEATURES = (shared_features("topk", NUM) + ["topk.%s" % w for w in TOPK_WHICH] + ["topk.k=%s" % k for k in K_CLASSES] +
                 ["topk.topk_path=%d" % p for p in (-1, 0, 1)] + ["topk.layout=%s" % s for s in TOPK_LAYOUTS] +
                 ["topk.ties straddle the threshold", "topk.the cut-over's side read from the pass count", "topk.refusal: k below 0"])


def byte_column(rng, n, dtype, nbytes):
    """A column whose order-preserving code varies in its lowest `nbytes` bytes only (8: everywhere, both i64 extremes in)."""
    if nbytes == 8:
        v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        if dtype == L.I64 and n >= 2:
            v[rng.choice(n, 2, replace=False)] = [I64_MIN, I64_MAX]
        return v if dtype == L.I64 else v.view(np.float64).copy()
    r = rng.integers(0, 1 << (8 * nbytes), n, dtype=np.int64)
    return r + (1 << 40) if dtype == L.I64 else (r | np.int64(0x4010000000000000)).view(np.float64).copy()


def draw_topk(rng, case):
    which = pick(rng, case, TOPK_WHICH, 2)
    cap = 70_000 if which == "arg_extreme" else DRY2_MAX_N
    d = shared_draw(rng, case, TOPK_T, TOPK_P, NUM, max_n=cap)
    n = d["n"]
    d["refusal"] = case % 31 == 30
    layout = pick(rng, case, TOPK_LAYOUTS, 3)
    if layout == "ties":
        x = rng.integers(0, max(2, n // 50 + 2), n).astype(np.int64 if d["dtype"] == L.I64 else np.float64)
        x = sprinkle(rng, x) if d["specials"] else x
    elif layout == "plain":
        x = plain_column(rng, n, d["dtype"], d["specials"])
    else:
        x = byte_column(rng, n, d["dtype"], int(layout[0]))
        d["specials"] = False
    nl = nulls_of(rng, n, d["nulls"])
    kc = pick(rng, case, K_CLASSES, 3)
    # Both sides of the cut-over give the same rows, so which side ran is read from the pass count the header documents: the
    # select needs no digit stream when every number is wanted (kn == m), the sort of numbers and nulls takes at least one pass.
    # Fewer numbers than the cut-over, and, where the row count is free, a multiple of topk_cutover's denominator, so that k * den == n.
    d["few_numbers"] = kc.startswith("cut-over") and which != "arg_extreme" and n >= 20 and bool(rng.random() < 0.6)
    if d["few_numbers"]:
        if d["size"] == "other":
            n = d["n"] = n - n % CUT_DEN
            x = x[:n]
        nl = np.ones(n, bool)
        nl[rng.choice(n, int(rng.integers(1, max(2, n * CUT_NUM // CUT_DEN - 1))), replace=False)] = False
        d["nulls"] = None
    cut = -(-n * CUT_NUM // CUT_DEN)
    k = max(0, {"0": 0, "1": 1, "n-1": n - 1, "n": n, "n+1": n + 1, "cut-over-1": cut - 1, "cut-over": cut, "cut-over+1": cut + 1}[kc])
    d.update(which=which, layout=layout, x=x, nl=nl, kc=kc, k=k, path=pick(rng, case, (-1, 0, 1)), straddle=False)
    if which != "arg_extreme" and not d["refusal"]:
        order, m = TR.topk_ref(x, nl, k + 1, which == "topk largest")
        if 0 < k < len(order) and k < m:                         # the k-th and the (k + 1)-th row hold one value
            a, b = x[order[k - 1]], x[order[k]]
            d["straddle"] = bool(a == b)
        d["want"] = (order[:k], min(k, m))
    return d


def classify_topk(d):
    if d["refusal"]:
        return ["topk.refusal: k below 0"]
    f = shared_classify("topk", d) + ["topk.%s" % d["which"], "topk.layout=%s" % d["layout"]]
    if d["which"] != "arg_extreme":
        f += ["topk.k=%s" % d["kc"], "topk.topk_path=%d" % d["path"]] + (["topk.ties straddle the threshold"] if d["straddle"] else [])
        if d["few_numbers"] and d["path"] == 0 and d["k"] > 0:
            f.append("topk.the cut-over's side read from the pass count")
    else:
        f = [s for s in f if not s.startswith("topk.out=")]
    return f


def expect_topk(d):
    if "want" not in d and not d["refusal"]:
        d["want"] = TR.idx_extreme_ref(d["x"], d["nl"])
    return d.get("want")


def run_topk(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.topk(col, n, -1), L.ERR_INVALID_ARGUMENT, "topk k = -1")
        want = expect_topk(d)
        if d["which"] == "arg_extreme":
            got = ctx.arg_extreme(col, n)
            check(got == want, "arg_extreme", (got, want))
            return
        kw, guards = out_kwargs(d["outp"], min(d["k"], n), np.int64, False)
        ctx.set_option("topk_path", d["path"])
        try:
            rows, numbers = ctx.topk(col, n, d["k"], d["which"] == "topk largest", **kw)
            if d["few_numbers"] and d["path"] == 0 and d["k"] > 0:
                passes, by_sort = ctx.timings()["n_partitions"], min(d["k"], n) * CUT_DEN >= n * CUT_NUM
                check((passes >= 1) == by_sort, "the cut-over's side (topk_cutover = %d / %d)" % (CUT_NUM, CUT_DEN), (d["k"], n, passes, by_sort))
        finally:
            ctx.set_option("topk_path", 0)
        rows = to_np(rows)
        check(numbers == want[1] and rows.shape == want[0].shape, "counts", (numbers, want[1], rows.shape, want[0].shape))
        check(np.array_equal(rows, want[0]), "rows", first_diff_any(rows, want[0]))
        check_guards(guards)
        grid_checked(d, "topk", "topk")
    finally:
        release(keep)


# ==== predicate and isin ========================================================================================================
PRED_T, PRED_P = geometry("predicate")
LDS_MAX = int(re.search(r"isin_lds_max_values = (\d+)", HEADER).group(1))
PRED_DTYPES = (L.I64, L.F64, L.U32CODE)
CONSTS = ("equal to a cell", "between two cells", "NaN", "+inf", "-inf")
LIST_SIZES = ("0", "1", "3", "lds max-1", "lds max", "lds max+1", "100000")
HIT_RATES = ("near 0", "near 1", "half")
PAIRINGS = ("f64 / f64", "i64 / f64", "i64 / i64", "str / str")
PRED_FEATURES = (shared_features("predicate", PRED_DTYPES) + ["predicate.op=%s" % s for s in PR.OP_NAMES] + ["predicate.const=%s" % c for c in CONSTS] +
                 ["predicate.predicate_path=%d" % p for p in (0, 1)] + ["predicate.predicate_path=%d on i64 beyond 2^53" % p for p in (0, 1)] +
                 ["predicate.count_only", "predicate.isin", "predicate.isin count_only", "predicate.isin negate", "predicate.isin duplicates in the list"] +
                 ["predicate.isin list of %s" % s for s in LIST_SIZES] + ["predicate.isin_path=%d" % p for p in (0, 1, 2)] +
                 ["predicate.isin list space=%s" % s for s in ("host", "device")] + ["predicate.isin hit rate %s" % h for h in HIT_RATES] +
                 ["predicate.isin %s" % p for p in PAIRINGS] + ["predicate.refusal: a string column"])


def draw_predicate(rng, case):
    d = shared_draw(rng, case, PRED_T, PRED_P, PRED_DTYPES, max_n=DRY2_MAX_N)
    n = d["n"]
    d["refusal"] = case % 37 == 36
    d["isin"] = case % 16 >= 12 or d["dtype"] == L.U32CODE
    d["count_only"] = bool(rng.random() < 0.2)
    nl = nulls_of(rng, n, d["nulls"])
    if d["refusal"]:
        d.update(isin=False, dtype=L.U32CODE, x=rng.integers(0, 9, n).astype(np.uint32), nl=nl, op=PR.GT)
        return d
    if not d["isin"]:
        x = plain_column(rng, n, d["dtype"], d["specials"])
        op, ck = int(pick(rng, case, PR.OPS)), pick(rng, case, CONSTS, 16)
        fin = x[np.isfinite(x.astype(np.float64))].astype(np.float64)
        if ck in ("equal to a cell", "between two cells") and not len(fin):
            ck = "NaN"
        if ck == "equal to a cell":
            a = float(fin[rng.integers(0, len(fin))])
            b = a + float(rng.choice([0.0, 1.0, 50.0, -1.0]))
        elif ck == "between two cells":
            u = np.unique(fin)
            i = int(rng.integers(0, max(len(u) - 1, 1)))
            a = float(u[i] + (u[min(i + 1, len(u) - 1)] - u[i]) / 2) if np.isfinite(u[min(i + 1, len(u) - 1)] - u[i]) else float(u[i]) + 0.5
            b = a + float(rng.choice([10.0, 200.0, -5.0]))
        else:
            a = {"NaN": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[ck]
            b = float(rng.choice([0.0, np.inf, np.nan]))
        d.update(x=x, nl=nl, op=op, const=ck, a=a, b=b, path=pick(rng, case, (0, 1), 3))
        return d
    # ---- isin: the list first, then a column that hits it at the drawn rate
    ls = pick(rng, case, LIST_SIZES, 16)
    m = {"lds max-1": LDS_MAX - 1, "lds max": LDS_MAX, "lds max+1": LDS_MAX + 1}.get(ls) or int(ls)
    dup = bool(rng.random() < 0.3) and m >= 2
    distinct = m - m // 2 if dup else m
    if d["dtype"] == L.U32CODE:
        pairing, vdt = "str / str", L.U32CODE
        vals = rng.choice(4 * max(distinct, 4), size=distinct, replace=False).astype(np.uint32)
        other = lambda k: (rng.integers(0, 4 * max(distinct, 4), k) + 4 * max(distinct, 4)).astype(np.uint32)   # noqa: E731
    elif d["dtype"] == L.F64:
        pairing, vdt = "f64 / f64", L.F64
        vals = (rng.integers(0, 1 << 62, distinct).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.float64).copy()
        other = lambda k: rng.normal(0, 100, k)                                                                  # noqa: E731
    elif rng.random() < 0.5:
        pairing, vdt = "i64 / f64", L.F64
        vals = rng.choice(4 * max(distinct, 4), size=distinct, replace=False).astype(np.float64) - 7.0
        other = lambda k: rng.integers(10**7, 10**8, k).astype(np.int64)                                         # noqa: E731
    else:
        pairing, vdt = "i64 / i64", L.I64
        vals = rng.integers(I64_MIN, I64_MAX, distinct, dtype=np.int64)
        other = lambda k: rng.integers(-1000, 1000, k).astype(np.int64)                                          # noqa: E731
    hit = pick(rng, case, HIT_RATES, 5) if m else "near 0"
    p = {"near 0": 0.001, "near 1": 0.999, "half": 0.5}[hit]
    if m:
        cells = vals[rng.integers(0, distinct, n)]
        cells = cells.astype(np.int64) if pairing == "i64 / f64" else cells
        x = np.where(rng.random(n) < p, cells, other(n))
    else:
        x = other(n)
    x = np.ascontiguousarray(x, {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32}[d["dtype"]])
    if d["specials"] and d["dtype"] != L.U32CODE:
        x = sprinkle(rng, x)
    if dup:
        vals = np.concatenate([vals, vals[:m - distinct]])
        vals = vals[rng.permutation(m)]
    d.update(x=x, nl=nl, vals=vals, vdt=vdt, pairing=pairing, ls=ls, dup=dup, hit=hit, negate=bool(rng.random() < 0.5),
             path=pick(rng, case, (0, 1, 2), 2), list_space="device" if m and rng.random() < 0.5 else "host")
    return d


def classify_predicate(d):
    if d["refusal"]:
        return ["predicate.refusal: a string column"]
    f = shared_classify("predicate", d)
    if d["count_only"]:
        f = [s for s in f if not s.startswith("predicate.out=")]
    if not d["isin"]:
        f += ["predicate.op=%s" % PR.OP_NAMES[d["op"]], "predicate.const=%s" % d["const"], "predicate.predicate_path=%d" % d["path"]]
        if d["dtype"] == L.I64 and d["specials"] and d["n"] >= 8:
            f.append("predicate.predicate_path=%d on i64 beyond 2^53" % d["path"])
        return f + (["predicate.count_only"] if d["count_only"] else [])
    f += ["predicate.isin", "predicate.isin list of %s" % d["ls"], "predicate.isin_path=%d" % d["path"], "predicate.isin list space=%s" % d["list_space"],
          "predicate.isin hit rate %s" % d["hit"], "predicate.isin %s" % d["pairing"]]
    for cond, name in ((d["count_only"], "count_only"), (d["negate"], "negate"), (d["dup"], "duplicates in the list")):
        if cond:
            f.append("predicate.isin %s" % name)
    return f


def expect_predicate(d):
    if "want" not in d and not d["refusal"]:
        mask = mask_of(d["nl"])
        d["want"] = (PR.isin(d["x"], mask, d["dtype"], d["vals"], d["vdt"], d["negate"]) if d["isin"] else
                     PR.predicate(d["x"], mask, d["op"], d["a"], d["b"]))
    return d.get("want")


def run_predicate(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.predicate(col, n, L.PRED_GT, 1.0), L.ERR_TYPE_MISMATCH, "predicate on U32CODE")
        want, count = expect_predicate(d)
        kw, guards = (dict(count_only=True), []) if d["count_only"] else out_kwargs(d["outp"], n, None, False)
        opt = "isin_path" if d["isin"] else "predicate_path"
        ctx.set_option(opt, d["path"])
        try:
            if d["isin"]:
                vcol = place(ctx, d["list_space"], d["vals"], None, d["vdt"], len(d["vals"]), keep)
                got, cnt = ctx.isin(col, n, vcol, d["negate"], **kw)
                if n:
                    which, slots = ctx.timings()["n_partitions"], ctx.timings()["table_slots"]
                    lds = d["path"] != 2 and len(d["vals"]) <= LDS_MAX
                    check(which == (1 if lds else 2), "the set isin built", (d["path"], len(d["vals"]), which))
                    check(slots >= 2 * len(d["vals"]) and slots & (slots - 1) == 0, "table slots", slots)
            else:
                got, cnt = ctx.predicate(col, n, d["op"], d["a"], d["b"], **kw)
        finally:
            ctx.set_option(opt, 0)
        check(cnt == count, "count", (cnt, count))
        if d["count_only"]:
            check(got is None, "count_only returns no bits")
        else:
            got = to_np(got)
            check(got.shape == want.shape and np.array_equal(got, want), "bits", first_diff_any(got, want))
        check_guards(guards)
        grid_checked(d, "predicate", "predicate")
    finally:
        release(keep)


# ==== describe and quantiles ======================================================================================================
DESC_T, DESC_P = geometry("describe")
DS_MAX_P = 16
DESC_LAYOUTS = ("constant", "the lowest byte varies", "the top byte varies", "full range", "two values in long runs", "normal")
DESC_FEATURES = (shared_features("describe", NUM, outs=()) + ["describe.describe", "describe.quantiles"] +
                 ["describe.percentiles=%d" % k for k in range(1, DS_MAX_P + 1)] +
                 ["describe.percentiles hold %s" % s for s in ("0", "100", "duplicates", "an unsorted list")] +
                 ["describe.layout=%s" % s for s in DESC_LAYOUTS] + ["describe.non-null count=%d" % k for k in (0, 1, 2)] +
                 ["describe.moments compared", "describe.refusal: 17 percentiles"])


def draw_describe(rng, case):
    d = shared_draw(rng, case, DESC_T, DESC_P, NUM, outs=(), max_n=DRY2_MAX_N)
    n = d["n"]
    d["refusal"] = case % 31 == 30
    layout = pick(rng, case, DESC_LAYOUTS, 3)
    i64 = d["dtype"] == L.I64
    if layout == "constant":
        x = np.full(n, -12345 if i64 else 0.1, np.int64 if i64 else np.float64)
    elif layout == "the lowest byte varies":
        x = byte_column(rng, n, d["dtype"], 1)
    elif layout == "the top byte varies":
        x = rng.integers(-128, 128, n).astype(np.int64) << 56
        x = x if i64 else (rng.integers(0, 128, n).astype(np.int64) << 56 | (rng.integers(0, 2, n).astype(np.int64) << 63)).view(np.float64).copy()
    elif layout == "full range":
        x = byte_column(rng, n, d["dtype"], 8)
    elif layout == "two values in long runs":
        run = int(rng.choice([64, DESC_T, 3 * DESC_T + 1]))
        x = np.repeat(rng.random(n // run + 1) < 0.5, run)[:n]
        x = np.where(x, 7, -3).astype(np.int64) if i64 else np.where(x, 1.5, -2.25)
    else:
        x = rng.integers(-10**6, 10**6, n).astype(np.int64) if i64 else rng.normal(500.0, 10.0, n)
    moments = layout == "normal" and not i64 and not d["specials"]
    if d["specials"] and layout in ("normal", "two values in long runs", "constant"):
        x = sprinkle(rng, x)
    elif layout not in ("normal",):
        d["specials"] = False
    nl = nulls_of(rng, n, d["nulls"])
    d["nonnull"] = None
    if case % 11 >= 8 and n >= 2:
        k = case % 11 - 8
        nl = np.ones(n, bool)
        nl[rng.choice(n, k, replace=False)] = False
        d.update(nonnull=k, nulls=None)
    which = ("describe", "quantiles")[case % 2]
    kp = 1 + (case // 2) % DS_MAX_P
    ps = list(rng.choice([0.0, 100.0, 25.0, 50.0, 75.0, 33.3, 99.9, 0.1] + list(rng.random(8) * 100.0), size=kp, replace=kp > 16))
    if kp >= 2 and rng.random() < 0.4:
        ps[int(rng.integers(0, kp))] = ps[0]
    if rng.random() < 0.5:
        ps = sorted(ps)
    d.update(which=which, layout=layout, x=x, nl=nl, ps=[float(p) for p in ps], moments=moments)
    return d


def classify_describe(d):
    if d["refusal"]:
        return ["describe.refusal: 17 percentiles"]
    f = shared_classify("describe", d) + ["describe.%s" % d["which"], "describe.layout=%s" % d["layout"]]
    if d["nonnull"] is not None:
        f.append("describe.non-null count=%d" % d["nonnull"])
    if d["which"] == "quantiles":
        ps = d["ps"]
        f.append("describe.percentiles=%d" % len(ps))
        for cond, name in ((0.0 in ps, "0"), (100.0 in ps, "100"), (len(set(ps)) < len(ps), "duplicates"), (ps != sorted(ps), "an unsorted list")):
            if cond:
                f.append("describe.percentiles hold %s" % name)
    elif d["moments"]:
        f.append("describe.moments compared")
    return f


def expect_describe(d):
    """The twins run inside the shared comparison rule; here they run once so that a draw they cannot take fails dry."""
    if "want" not in d and not d["refusal"]:
        s, _ = DR.sorted_cells(d["x"], d["nl"], np.int64 if d["dtype"] == L.I64 else np.float64)
        d["want"] = [DR.percentile_ref(s, p) for p in d["ps"]] if len(s) else None
        if len(s) and d["which"] == "describe":
            DR.describe_ref(d["x"], d["nl"], np.int64 if d["dtype"] == L.I64 else np.float64)
    return d.get("want")


def run_describe(ctx, d):
    n, keep = d["n"], []
    npdt = np.int64 if d["dtype"] == L.I64 else np.float64
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        if d["refusal"]:
            return expect_status(lambda: ctx.quantiles(col, n, [50.0] * 17), L.ERR_INVALID_ARGUMENT, "17 percentiles")
        if d["which"] == "describe":
            asserting(DR.compare_describe, ctx.describe(col, n), d["x"], d["nl"], npdt, d["moments"])
        else:
            q, cnt = ctx.quantiles(col, n, d["ps"])
            asserting(DR.compare_quantiles, q, cnt, d["x"], d["nl"], npdt, d["ps"])
        grid_checked(d, "describe", "describe")
    finally:
        release(keep)


# ==== wquant: window_quantile =====================================================================================================
WQ_SRC = open(os.path.join(ROOT, "pandrs_amd", "csrc", "window_quantile.hip")).read()
WQ_DIRECT_MAX = int(re.search(r"constexpr int WQ_DIRECT_MAX = (\d+);", WQ_SRC).group(1))
WQ_SIZES = ("0", "1", "2", "63", "64", "65", "255", "256", "257", "4095", "4096", "4097", "8191", "8193", "other")   # the direct tile, the general one
WQ_W = ("1", "2", "3", "direct max-1", "direct max", "direct max+1", "300", "n", "n+1")
WQ_MP = ("unset", "0", "1", "w", "w+1")
WQ_STAT = ("median", "q=0", "q=1/3", "q=0.5", "q=1")
WQ_FEATURES = (shared_features("wquant", NUM, outs=OUTS[:2], sizes=WQ_SIZES) + ["wquant.rolling", "wquant.expanding"] + ["wquant.w=%s" % w for w in WQ_W] +
               ["wquant.center=%d" % c for c in (0, 1)] + ["wquant.min_periods=%s" % m for m in WQ_MP] + ["wquant.%s" % s for s in WQ_STAT] +
               ["wquant.nan_missing=%d" % c for c in (0, 1)] + ["wquant.window_quantile_path=%d" % p for p in (0, 1, 2)] +
               ["wquant.long tie runs", "wquant.refusal: the direct path beyond its window"])


def draw_wquant(rng, case):
    d = shared_draw(rng, case, 4096, 1, NUM, outs=OUTS[:2], sizes=WQ_SIZES)
    n = d["n"]
    kind = "expanding" if case % 4 == 3 else "rolling"
    wc = pick(rng, case, WQ_W, 4)
    named = {"direct max-1": WQ_DIRECT_MAX - 1, "direct max": WQ_DIRECT_MAX, "direct max+1": WQ_DIRECT_MAX + 1, "n": n, "n+1": n + 1}
    w = max(1, named[wc] if wc in named else int(wc))
    mpc = pick(rng, case, WQ_MP, 3)
    mp = {"unset": None, "0": 0, "1": 1, "w": w, "w+1": w + 1}[mpc]
    if kind == "expanding":
        w, wc = 0, None
        mpc = mpc if mpc in ("0", "1") else "1"
        mp = int(mpc)
    stat = pick(rng, case, WQ_STAT, 5)
    direct_ok = kind == "rolling" and w <= WQ_DIRECT_MAX
    path = pick(rng, case, (0, 1, 2), 2)
    d["refusal"] = path == 1 and not direct_ok and case % 7 == 0 and n > 0
    if path == 1 and not direct_ok and not d["refusal"]:
        path = 0
    ties = bool(rng.random() < 0.3)
    if ties:
        run = int(rng.choice([50, 300, 5000]))
        x = np.repeat(rng.integers(-3, 4, n // run + 1), run)[:n].astype(np.int64 if d["dtype"] == L.I64 else np.float64)
        x = sprinkle(rng, x) if d["specials"] else x
    else:
        x = plain_column(rng, n, d["dtype"], d["specials"])
    d.update(kind=kind, wc=wc, w=w, mpc=mpc, mp=mp, stat=stat, median=stat == "median", q={"median": 0.5, "q=0": 0.0, "q=1/3": 1.0 / 3.0, "q=0.5": 0.5, "q=1": 1.0}[stat],
             center=bool((case // 2) % 2) and kind == "rolling", nan_missing=bool(rng.random() < 0.5), path=path, ties=ties, x=x, nl=nulls_of(rng, n, d["nulls"]))
    return d


def classify_wquant(d):
    if d["refusal"]:
        return ["wquant.refusal: the direct path beyond its window"]
    f = shared_classify("wquant", d) + ["wquant.%s" % d["kind"], "wquant.min_periods=%s" % d["mpc"], "wquant.%s" % d["stat"],
                                        "wquant.nan_missing=%d" % d["nan_missing"], "wquant.window_quantile_path=%d" % d["path"]]
    if d["kind"] == "rolling":
        f += ["wquant.w=%s" % d["wc"], "wquant.center=%d" % d["center"]]
    return f + (["wquant.long tie runs"] if d["ties"] else [])


def expect_wquant(d):
    if "want" not in d and not d["refusal"]:
        valid = None if d["nl"] is None else ~d["nl"]
        d["want"] = QR.window_quantile_fast(d["x"], valid, d["kind"], d["w"], d["center"], d["mp"], d["median"], d["q"], d["nan_missing"])
    return d.get("want")


def run_wquant(ctx, d):
    n, keep = d["n"], []
    try:
        col = place(ctx, d["space"], d["x"], mask_of(d["nl"]), d["dtype"], n, keep)
        kw = dict(median=d["median"], q=d["q"], window=d["w"], min_periods=-1 if d["mp"] is None else d["mp"], center=d["center"],
                  nan_missing=d["nan_missing"], out_device=d["outp"] == "device")
        wk = L.WINDOW_KIND_ROLLING if d["kind"] == "rolling" else L.WINDOW_KIND_EXPANDING
        ctx.set_option("window_quantile_path", d["path"])
        try:
            if d["refusal"]:
                return expect_status(lambda: ctx.window_quantile(col, n, wk, **kw), L.ERR_INVALID_ARGUMENT, "the direct path forced beyond its window")
            want = expect_wquant(d)
            got = to_np(ctx.window_quantile(col, n, wk, **kw))
        finally:
            ctx.set_option("window_quantile_path", 0)
        check(got.shape == want.shape and w_same(got, want), "window quantile", w_first_diff(got, want) if got.shape == want.shape else got.shape)
    finally:
        release(keep)


# ==== eval ======================================================================================================================
EVAL_T, EVAL_P = geometry("eval")
EVAL_DTYPES = (L.I64, L.F64, L.BOOLBITS)
EVAL_PROGS = ("random_program", "one op", "MAX_OPS ops", "depth MAX_DEPTH", "the same column named twice")
OP = ER.OP
EVAL_FEATURES = (shared_features("eval", EVAL_DTYPES) + ["eval.program=%s" % p for p in EVAL_PROGS] + ["eval.want_mask=%d" % m for m in (0, 1)] +
                 ["eval.columns=%d" % k for k in range(1, ER.MAX_COLS + 1)] +
                 ["eval.a column with a mask", "eval.value output with out_mask", "eval.value output without out_mask",
                  "eval.mask output consumed by a count-only filter_indices", "eval.refusal: the output over a named column"])


def draw_program(rng, prog_kind, dtypes, want_mask):
    values = [j for j, t in enumerate(dtypes) if t != L.BOOLBITS]
    col = lambda: (OP["COL"], float(rng.choice(values)))                                           # noqa: E731
    to_mask = [(OP["CONST"], 0.0), (OP["GT"], 0.0)]
    if prog_kind == "one op":
        j = [k for k, t in enumerate(dtypes) if (t == L.BOOLBITS) == want_mask][0]
        return [(OP["COL"], float(j))]
    if prog_kind == "depth MAX_DEPTH":
        prog = [col() if rng.random() < 0.7 else (OP["CONST"], float(rng.choice([0.5, -1.0, 3.0]))) for _ in range(ER.MAX_DEPTH)]
        prog += [(int(rng.choice(ER.BINARY_VALUE)), 0.0) for _ in range(ER.MAX_DEPTH - 1)]
        return prog + (to_mask if want_mask else [])
    if prog_kind == "the same column named twice":
        prog = [(OP["COL"], 0.0), (OP["COL"], 1.0), (int(rng.choice([OP["MUL"], OP["SUB"], OP["ADD"]])), 0.0), (OP["COL"], 0.0), (OP["ADD"], 0.0)]
        return prog + (to_mask if want_mask else [])
    if prog_kind == "MAX_OPS ops":
        prog = ER.random_program(rng, list(dtypes), max_ops=40, want_mask=want_mask)
        while len(prog) < ER.MAX_OPS:
            prog.append((OP["NOT"] if want_mask else int(rng.choice([OP["NEG"], OP["ABS"], OP["FLOOR"], OP["CEIL"], OP["TRUNC"], OP["ROUND"]])), 0.0))
        return prog
    return ER.random_program(rng, list(dtypes), want_mask=want_mask)


def draw_eval(rng, case):
    d = shared_draw(rng, case, EVAL_T, EVAL_P, EVAL_DTYPES, max_n=DRY2_MAX_N)
    n = d["n"]
    d["refusal"] = case % 41 == 40
    prog_kind, want_mask = pick(rng, case, EVAL_PROGS), bool((case // 5) % 2)
    ncols = 1 + (case // 3) % ER.MAX_COLS
    if d["size"] == "grid+1":
        ncols = min(ncols, 3)
    if prog_kind == "the same column named twice":
        ncols = max(ncols, 2)
    dtypes = [d["dtype"]] + [int(rng.choice(EVAL_DTYPES)) for _ in range(ncols - 1)]
    if prog_kind == "the same column named twice" or d["refusal"]:
        if dtypes[0] == L.BOOLBITS:
            dtypes[0] = d["dtype"] = L.F64
        dtypes[1:2] = dtypes[:1] if prog_kind == "the same column named twice" else dtypes[1:2]
    if prog_kind == "one op" and not any((t == L.BOOLBITS) == want_mask for t in dtypes):
        want_mask = not want_mask
    if all(t == L.BOOLBITS for t in dtypes):
        if ncols == 1 and prog_kind != "one op":
            dtypes[0] = d["dtype"] = L.F64
        elif ncols > 1:
            dtypes[-1] = L.I64
    if d["refusal"]:
        d.update(space="device", n=max(n, 8), size="other", dtype=L.F64)
        dtypes[0], n, prog_kind, want_mask = L.F64, d["n"], "the same column named twice" if ncols >= 2 and dtypes[1] == L.F64 else "depth MAX_DEPTH", False
    cols = []
    for j, t in enumerate(dtypes):
        layout = d["nulls"] if j == 0 else str(rng.choice(["no mask", "no mask", "mask without a bit", "p=0.01", "p=0.5"]))
        data = (rng.random(n) < 0.5) if t == L.BOOLBITS else plain_column(rng, n, t, d["specials"] and j < 2)
        cols.append((data, nulls_of(rng, n, layout), t))
    if prog_kind == "the same column named twice":
        cols[1] = cols[0]
    if prog_kind in ("depth MAX_DEPTH",) and all(t == L.BOOLBITS for t in dtypes):
        prog_kind = "one op"
        want_mask = True
    if d["size"] == "grid+1" and prog_kind == "MAX_OPS ops":
        prog_kind = "random_program"
    program = draw_program(rng, prog_kind, dtypes, want_mask) if prog_kind != "random_program" else ER.random_program(
        rng, list(dtypes), max_ops=16 if d["size"] == "grid+1" else ER.MAX_OPS, want_mask=want_mask)
    if d["refusal"]:                                            # the output will lie over column 0: the program names it
        program = [(OP["COL"], 0.0), (OP["CONST"], 2.0), (OP["MUL"], 0.0)]
    want = ER.evaluate(cols, n, program)
    if want.zero_tie:                                           # a documented limit (the module's docstring)
        program = [({OP["MAX"]: OP["ADD"], OP["MIN"]: OP["SUB"]}.get(op, op), arg) for op, arg in program]
        want = ER.evaluate(cols, n, program)
    is_mask, depth = ER.check(dtypes, program)
    d.update(prog_kind=prog_kind, want_mask=bool(is_mask), ncols=ncols, dtypes=tuple(dtypes), cols=cols, program=program, n_ops=len(program), depth=depth,
             with_out_mask=bool(rng.random() < 0.5), want=want)
    return d


def classify_eval(d):
    if d["refusal"]:
        return ["eval.refusal: the output over a named column"]
    f = shared_classify("eval", d) + ["eval.want_mask=%d" % d["want_mask"], "eval.columns=%d" % d["ncols"]]
    k = d["prog_kind"]
    if ((k == "one op" and d["n_ops"] == 1) or (k == "MAX_OPS ops" and d["n_ops"] == ER.MAX_OPS) or (k == "depth MAX_DEPTH" and d["depth"] == ER.MAX_DEPTH) or
            k in ("random_program", "the same column named twice")):
        f.append("eval.program=%s" % k)
    if any(c[1] is not None for c in d["cols"]):
        f.append("eval.a column with a mask")
    if d["want_mask"] and d["outp"] != "host":
        f.append("eval.mask output consumed by a count-only filter_indices")
    if not d["want_mask"] and d["outp"] == "guarded":
        f.append("eval.value output with%s out_mask" % ("" if d["with_out_mask"] else "out"))
    return f


def expect_eval(d):
    return d["want"]


def run_eval(ctx, d):
    n, keep, want = d["n"], [], d["want"]
    try:
        placed = {}
        for data, nl, t in d["cols"]:                            # the column named twice is one buffer passed twice
            if id(data) not in placed:
                placed[id(data)] = place(ctx, d["space"], ER.pack(data) if t == L.BOOLBITS else data, mask_of(nl), t, n, keep)
        passed = [placed[id(c[0])] for c in d["cols"]]
        if d["refusal"]:
            return expect_status(lambda: ctx.eval(passed, n, d["program"], out=passed[0][0]), L.ERR_INVALID_ARGUMENT, "eval in place")
        if want.is_mask:
            kw, guards = out_kwargs(d["outp"], n, None, False)
            got, cnt = ctx.eval(passed, n, d["program"], **kw)
            host = to_np(got)
            check(host.shape[0] == (n + 7) // 8 and np.array_equal(host, ER.pack(want.mask)), "bits", first_diff_any(host, ER.pack(want.mask)))
            check(cnt == want.count, "count", (cnt, want.count))
            if d["outp"] != "host":                              # the bitmap as it lies on the device is a BOOLBITS column
                _, sel = ctx.filter_indices((got, None, L.BOOLBITS), n, indices=False)
                check(sel == want.count, "filter_indices count over the mask output", (sel, want.count))
        else:
            kw, guards = out_kwargs(d["outp"], n, np.float64, d["with_out_mask"])
            check_cells(ctx.eval(passed, n, d["program"], **kw), want.values, want.nulls, guards, n)
        check_guards(guards)
        grid_checked(d, "eval", "eval")
    finally:
        release(keep)


def _desc(kind):
    return lambda d: describe_case(kind, d)


KINDS = {"describe": (draw_describe, classify_describe, run_describe, _desc("describe"), DESC_FEATURES, expect_describe),
         "rank": (draw_rank, classify_rank, run_rank, _desc("rank"), RANK_FEATURES, expect_rank),
         "fill": (draw_fill, classify_fill, run_fill, _desc("fill"), FILL_FEATURES, expect_fill),
         "topk": (draw_topk, classify_topk, run_topk, _desc("topk"), TOPK_FEATURES, expect_topk),
         "predicate": (draw_predicate, classify_predicate, run_predicate, _desc("predicate"), PRED_FEATURES, expect_predicate),
         "wquant": (draw_wquant, classify_wquant, run_wquant, _desc("wquant"), WQ_FEATURES, expect_wquant),
         "cum": (draw_cum, classify_cum, run_cum, _desc("cum"), CUM_FEATURES, expect_cum),
         "eval": (draw_eval, classify_eval, run_eval, _desc("eval"), EVAL_FEATURES, expect_eval)}
