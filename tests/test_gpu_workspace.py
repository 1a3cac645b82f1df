"""The library's own workspace: nothing may read scratch it did not write in the same call.

Every entry point takes its scratch from bump arenas that grow, never shrink and are never cleared (common.hpp Arena::ensure),
so a tile state, a counter or a hash table starts a call as whatever the previous call left there, or as the zeros of a fresh
allocation.  Four angles, every result against the op's own reference (tests/*_ref.py, the CPU oracle) through the op's own
checker, at 3 tiles + 1 row and at the op's "more tiles than workgroups" count, with ~10 % nulls and a few NaN cells:

 a. set_option("poison_workspace"): every workspace block is filled with 0x00, 0xFF and 0xA5 before the call uses it; the
    counter of filled bytes must move with every call, and the deterministic ops must give the same bits under all three
    fills and without any;
 b. no poison, one context: a larger call on other data first, the same call twice, another op of the same arena first:
    the hook cannot plant plausible stale state (a finished look-back flag), a previous call can;
 c. a tiny call, then ONE call whose nested sort / groupby has to grow an arena the outer call still reads;
 d. with the option at 0 the counter stands still and a repeated call allocates nothing.

Every test has a fresh Context, so the arenas are as small as the case allows and a fill costs microseconds.  References are
computed once per input (the inputs are built once and never written) and shared by the runs of a case."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "experiments"))

from oracle import oracle as O  # noqa: E402
from pandrs_amd import _lib as L  # noqa: E402
from tests import join_ref as J  # noqa: E402
from tests import test_gpu_cumulative as TC  # noqa: E402
from tests import describe_ref as DREF  # noqa: E402
from tests import test_gpu_describe as TD  # noqa: E402
from tests import test_gpu_fill as TF  # noqa: E402
from tests import test_gpu_filter as TFI  # noqa: E402
from tests import test_gpu_groupby as TG  # noqa: E402
from tests import test_gpu_join_edges as TJ  # noqa: E402
from tests import test_gpu_predicate as TP  # noqa: E402
from tests import test_gpu_rank as TR  # noqa: E402
from tests import test_gpu_sort as TS  # noqa: E402
from tests import test_gpu_topk as TK  # noqa: E402
from tests import test_gpu_window_quantile as TQ  # noqa: E402
from tests import window_quantile_ref as WQR  # noqa: E402
from tests.helpers import assert_groupby_equal  # noqa: E402
from tests.sort_ref import Col, ref_lexsort  # noqa: E402

import fuzz_ops as FO  # noqa: E402  (experiments/: the window / chain case makers and their comparisons)

POISONS = (0x00, 0xFF, 0xA5)


# ---- the watched context ------------------------------------------------------------------------------------------------
# the calls that size at least one arena whenever a column comes from the host (the staging arena, if nothing else)
ENTRY_POINTS = {"groupby_agg", "groupby_indices", "join_indices", "sort_indices", "filter_indices", "window", "window_quantile",
                "describe", "quantiles", "rank", "fill", "topk", "arg_extreme", "predicate", "isin", "cumulative", "lag", "reduce_column"}
# ... and those of them whose every output bit is defined (the folds of f64 sums are not: their order is the scheduler's)
DETERMINISTIC = {"sort_indices", "filter_indices", "filter_gather", "rank", "fill", "topk", "arg_extreme", "predicate", "isin", "lag",
                 "quantiles", "window_quantile"}
ORDER_STATS = ("count", "min", "q1", "median", "q3", "max")


def digest(o):
    if o is None or isinstance(o, (bool, int, float, str)):
        return repr(o)
    if isinstance(o, dict):
        return tuple((k, digest(o[k])) for k in sorted(o))
    if isinstance(o, (tuple, list)):
        return tuple(digest(v) for v in o)
    a = np.ascontiguousarray(o.cpu().numpy() if hasattr(o, "cpu") else o)
    return (str(a.dtype), a.shape, hashlib.sha1(a.tobytes()).hexdigest())


class Watched:
    """A Context whose entry points assert what the poison counter did during the call (moved with the hook on, stood still
    with it off) and log the bits of every deterministic result, in call order."""

    def __init__(self, ctx):
        self._ctx, self.poison, self.log = ctx, None, []

    def set_poison(self, byte):
        self.poison = byte
        self._ctx.poison_workspace(byte)

    def __getattr__(self, name):
        f = getattr(self._ctx, name)
        if name not in ENTRY_POINTS and name != "filter_gather":
            return f

        def call(*a, **k):
            import pandrs_amd as pa
            before = pa.Context.workspace_poisoned_bytes()
            out = f(*a, **k)
            grew = pa.Context.workspace_poisoned_bytes() - before
            if self.poison is None:
                assert grew == 0, (name, grew)
            elif name in ENTRY_POINTS:
                assert grew > 0, "%s filled no workspace under poison %#x" % (name, self.poison)
            if name in DETERMINISTIC:
                self.log.append((name, digest(out)))
            elif name == "describe":
                self.log.append((name, digest({f: out[f] for f in ORDER_STATS})))
            elif name == "cumulative" and a[2] in (TC.MAX, TC.MIN, TC.COUNT):
                self.log.append((name, a[2], digest(out)))
            return out
        return call


@pytest.fixture
def fresh():
    """-> a function that opens a Watched context on its own library Context; the knob is process-wide: always switched off
    again, and every context closed."""
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    opened = []

    def make():
        opened.append(pa.Context(0))
        return Watched(opened[-1])
    try:
        yield make
    finally:
        pa.Context.poison_workspace(None)
        for c in opened:
            c.close()


# ---- references: once per input -------------------------------------------------------------------------------------------
_memo = {}


def memo(fn):
    """`fn` keyed by the identity of its array arguments (kept alive in the entry, so an id is never reused) and the value of
    the others.  The case inputs below are built once, so every run of a case asks with the same objects."""
    def key_of(v):
        return ("id", id(v)) if isinstance(v, np.ndarray) else ("v", repr(v))

    @functools.wraps(fn)
    def cached(*a, **k):
        key = (fn.__module__, fn.__qualname__, tuple(key_of(v) for v in a), tuple((n, key_of(k[n])) for n in sorted(k)))
        if key not in _memo:
            _memo[key] = ((a, k), fn(*a, **k))
        return _memo[key][1]
    return cached


@pytest.fixture(autouse=True)
def shared_references(monkeypatch):
    """The checkers of the op modules restate their reference on every call; here one input is checked up to a dozen times."""
    for mod, names in ((TK, ("topk_ref", "idx_extreme_ref")), (TR, ("rank_ref_all",)), (TF, ("fill_twin",)), (TC, ("cum_twin", "lag_twin")),
                       (DREF, ("sorted_cells", "describe_ref"))):         # (test_gpu_describe.check compares through tests/describe_ref.py)
        for name in names:
            monkeypatch.setattr(mod, name, memo(getattr(mod, name)))


class SharedWindows:
    """window_quantile_ref.SortedWindows with every (kind, w, center, ...) statistic computed once."""

    def __init__(self, x, valid, nan_missing):
        self._sw = WQR.SortedWindows(x, valid, nan_missing)
        self.lengths = functools.lru_cache(None)(self._sw.lengths)
        self.stat = functools.lru_cache(None)(self._sw.stat)


def once(fn):
    return functools.lru_cache(None)(fn)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@once
def grid_of(per_cu):
    import torch
    return per_cu * torch.cuda.get_device_properties(0).multi_processor_count


@once
def column(n, seed, kind="f64"):
    """The shared column shape: ties, ~10 % null bits, ~0.5 % NaN cells (F64), both signs of zero."""
    rng = np.random.default_rng(seed)
    nulls = rng.random(n) < 0.1
    if kind == "i64":
        x = rng.integers(-n // 7 - 2, n // 7 + 2, n)
    else:
        x = np.round(rng.normal(0, max(n // 50, 3), n))
        x[rng.random(n) < 0.005] = np.nan
        x[rng.random(n) < 0.01] = -0.0
    return frozen(x, nulls)


# ---- the column ops: SIZE = "small" (3 tiles + 1 row) or "large" (more tiles than workgroups), other data ---------------------
def n_rank(size):
    tile, grid = TR.geometry()
    return 3 * tile + 1 if size == "small" else grid * tile + tile + 3


def op_rank(ctx, size):
    for kind in ("f64", "i64"):
        x, nulls = column(n_rank(size), 11 + (size == "large"), kind)
        TR.check(ctx, x, nulls)


def n_fill(size):
    return 3 * TF.T + 1 if size == "small" else grid_of(TF.PER_CU) * TF.T + TF.T + 3


def op_fill(ctx, size):
    x, nulls = column(n_fill(size), 21 + (size == "large"))
    TF.check(ctx, x, nulls)                                             # NaN cells and null bits: ffill, bfill, interpolate, fillna
    xi, _ = column(n_fill(size), 23 + (size == "large"), "i64")
    TF.check(ctx, xi, nulls, methods=(TF.FFILL, TF.BFILL, TF.LINEAR))


def n_topk(size):
    return 3 * TK.TILE + 1 if size == "small" else TK.full_grid() * TK.TILE + TK.TILE + 3


def op_topk(ctx, size):
    n = n_topk(size)
    x, nulls = column(n, 31 + (size == "large"))
    cut = -(-n * TK.CUT_NUM // TK.CUT_DEN)
    if size == "small":
        TK.check(ctx, x, nulls, ks=[1, 100, cut - 1, cut, n], paths=(-1, 1, 0))          # both sides of the cut-over, both paths; idxmax
    else:
        TK.check(ctx, x, nulls, ks=[1, 5000, cut - 1, cut], paths=(0,))
        first, last = ctx.arg_extreme((x, TK.bits(nulls), L.F64), n)
        ok = ~nulls & ~np.isnan(x)
        lo, hi = np.nanmin(x[ok]), np.nanmax(x[ok])
        assert first == int(np.flatnonzero(ok & (x == lo))[0]) and last == int(np.flatnonzero(ok & (x == hi))[-1])


def n_pred(size):
    return 3 * TP.TILE + 1 if size == "small" else TP.full_grid() * TP.TILE + 77


@once
def isin_values(n_values):
    return frozen(np.random.default_rng(n_values).integers(-50, 50, n_values).astype(np.float64))[0]


def op_predicate(ctx, size):
    n = n_pred(size)
    x, nulls = column(n, 41 + (size == "large"))
    TP.check_pred(ctx, x, nulls, ops=(TP.R.GT, TP.R.BETWEEN, TP.R.ISNA, TP.R.NE, TP.R.EQ), args=[(-0.5, 7.0)])
    xi, _ = column(n, 43 + (size == "large"), "i64")
    TP.check_pred(ctx, xi, nulls, ops=(TP.R.LE, TP.R.BETWEEN), args=[(7.0, 90.0)])
    TP.check_isin(ctx, xi, nulls, L.I64, isin_values(300), L.F64, paths=(1, 2))                       # the LDS set and the global table
    if size == "small":
        TP.check_isin(ctx, x, nulls, L.F64, isin_values(TP.LDS_MAX + 1), L.F64, paths=(0,), negates=(True,))


def n_cum(size):
    return TC.SHAPES["2T+1"](0) + TC.T if size == "small" else TC.SHAPES["(G+1)T+3"](grid_of(TC.PER_CU))


@once
def cum_columns(n, seed):
    return [frozen(x, nulls) for x, nulls in TC.columns_of(n, seed)]


def op_cumulative(ctx, size):
    n = n_cum(size)
    for x, nulls in cum_columns(n, n):                                 # small integers: SUM is bit for bit; PROD leaves f64's range
        TC.check_cum(ctx, x, nulls, exact=True)
    x, nulls = column(n, 51 + (size == "large"))
    for periods in (1, TC.T + 1):
        TC.check_lag(ctx, x, nulls, periods)


def n_describe(size):
    tile, grid = TD.geometry()
    return 3 * tile + 1 if size == "small" else grid * tile + tile + 3


def op_describe(ctx, size):
    n = n_describe(size)
    x, nulls = column(n, 61 + (size == "large"))
    TD.check(ctx, x, nulls)
    xi, _ = column(n, 63 + (size == "large"), "i64")
    TD.check(ctx, xi, nulls, dtype=L.I64, moments=False)


N_SORT = {"small": FO.SORT_N[13], "large": FO.SORT_N[-2]}             # 3 tiles of 2048 + 1; one row past 1024 workgroups x 2048 rows
assert N_SORT == {"small": 6145, "large": 2_097_153}


@once
def sort_case(n, seed):
    rng = np.random.default_rng(seed)
    c0 = TS.make_col(rng, L.F64, n, distinct=max(n // 40, 9), null_p=0.1)
    c1 = Col(L.I64, rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True), rng.random(n) < 0.1)
    return c0, c1, ref_lexsort([c1], [True]), ref_lexsort([c0, c1], [False, True])


def op_sort(ctx, size):
    c0, c1, want1, want2 = sort_case(N_SORT[size], 71 + (size == "large"))
    assert np.array_equal(TS.got(ctx, [c1], [True]), want1)                                   # one key: 8 digits of a full-range word
    assert np.array_equal(TS.got(ctx, [c0, c1], [False, True]), want2)                        # two keys, the first with long tie runs


N_FILTER = {"small": FO.FILTER_N[14], "large": FO.FILTER_N[-2]}       # 3 tiles of 4096 + 1; more tiles than a grid holds
assert N_FILTER == {"small": 12_289, "large": 1_000_003}


@once
def filter_case(n, seed):
    rng = np.random.default_rng(seed)
    values, nulls, cond = TFI.cond_of(rng, n, 0.6, 0.1)
    rows = TFI.want_rows(values, nulls)
    srcs = []
    for dtype, fill in ((L.F64, -1.5), (L.I64, 7), (L.BOOLBITS, 0)):
        v, sn, src = TFI.src_of(rng, dtype, n, 0.1)
        srcs.append((src, fill, TFI.want_values(v, sn, rows, dtype, fill)))
    return cond, rows, srcs


def op_filter(ctx, size):
    n = N_FILTER[size]
    cond, rows, srcs = filter_case(n, 81 + (size == "large"))
    idx, cnt = ctx.filter_indices(cond, n)
    assert cnt == len(rows) and np.array_equal(idx.cpu().numpy(), rows)
    for src, fill, want in srcs:
        assert TFI.same_bits(ctx.filter_gather(src, n, cnt, fill), want)


N_WINDOW = {"small": FO.WINDOW_N[14], "large": FO.WINDOW_N[-1]}       # 3 LDS chunks of 4096 values + 1; 2 M rows: more tiles than a grid holds
assert N_WINDOW == {"small": 12_289, "large": 2_000_003}


@once
def window_case(n, seed, exact):
    x, valid = FO.data_of(np.random.default_rng(seed), n, 0.1, special=exact)
    return frozen(x, valid)


def op_window(ctx, size):
    """rolling, expanding and EWM folds, with fuzz_ops' comparison for each kind (window_check: the fold bit for bit, the
    expanding sums and the EWM recurrences inside their bounds).  The references that cost n * w or a Python loop per row keep to
    the row counts fuzz_ops allows them."""
    big = size == "large"
    plans = [("rolling", "sum", 12_289 if big else 6145, dict(w=100)), ("rolling", "min", N_WINDOW[size], dict(w=4097)),
             ("rolling", "count", N_WINDOW[size], dict(w=64, center=True)), ("expanding", "sum", N_WINDOW[size], {}),
             ("expanding", "max", 400_001 if big else 12_289, {}), ("expanding", "var", 8193 if big else 6145, {}),
             ("ewm", "mean", 100_003 if big else 12_289, dict(alpha=0.05)), ("ewm", "var", 100_003 if big else 12_289, dict(alpha=0.5))]
    for kind, op, n, kw in plans:
        exact = kind == "rolling" or op in ("min", "max", "count")
        x, valid = window_case(n, 91 + big, exact)
        d = dict(kind=kind, op=op, n=n, w=0, center=False, mp=1, ddof=1, alpha=0.0, x=x, valid=valid)
        d.update(kw)
        got = FO.to_np(FO.window_call(ctx, (x, FO.bits(~valid), L.F64), d))
        key = ("window", kind, op, n, 91 + big)
        if exact:                                                      # the exact references are pure: once per input
            if key not in _memo:
                FO.window_check(d, got)
                _memo[key] = got.copy()
            assert FO.WR.same(got, _memo[key]), (kind, op, n, FO.WR.first_diff(got, _memo[key]))
        else:
            FO.window_check(d, got)


N_WQ = {"small": TQ.SIZES[-1], "large": TQ.SIZES[-2]}                 # 3 direct tiles + 17 rows; one row past 2^17 (another level)
assert N_WQ == {"small": 3 * TQ.DIRECT_TILE + 17, "large": 2 ** 17 + 1}


@once
def wq_case(n, seed):
    x, valid = TQ.mixed(np.random.default_rng(seed), n)
    x[::97] = np.nan                                                     # NaN cells count as missing (nan_missing) like null bits
    frozen(x, valid)
    return x, valid, SharedWindows(x, valid, True)


def op_window_quantile(ctx, size):
    n = N_WQ[size]
    x, valid, sw = wq_case(n, 101 + (size == "large"))
    col = TQ.col_of(x, valid)
    stats = ((True, 0.5), (False, 0.25))
    TQ.check(ctx, col, n, sw, "rolling", 7, False, mps=(1,), stats=stats, nan_missing=True)                       # both paths (paths_of)
    TQ.check(ctx, col, n, sw, "rolling", TQ.DIRECT_MAX + 1, True, mps=(None, 1), stats=stats, nan_missing=True)   # the general path alone
    TQ.check(ctx, col, n, sw, "expanding", mps=(1,), stats=stats, nan_missing=True)


@once
def reduce_case(n, seed):
    rng = np.random.default_rng(seed)
    cols = [(rng.normal(5, 2, n), O.pack_mask(rng.random(n) < 0.1), O.F64), (rng.integers(-10**9, 10**9, n).astype(np.int64), None, O.I64)]
    return [(col, O.reduce_column(col, n)) for col in cols]


def op_reduce(ctx, size):
    n = 3 * 2048 + 1 if size == "small" else 1_000_003
    for col, (want, wc) in reduce_case(n, 111):
        got, gc = ctx.reduce_column(col, n)
        assert gc == wc and got[2] == want[2] and got[3] == want[3]
        np.testing.assert_allclose(got[:2], want[:2], rtol=1e-9)


# ---- join: one case of the edge suite per join type ---------------------------------------------------------------------------
@once
def join_cases():
    T = TJ.TILE
    out = []
    for c in J.edge_cases("a"):
        if c["nl"] == c["nr"] == 3 * T + 1:
            out.append(dict(c, hows=[O.INNER, O.LEFT]))
    assert {c["options"]["join_one_pass"] for c in out} == {0, 1}
    return out


def op_join(ctx, size):
    for c in join_cases():
        TJ.run_case(ctx, c)
    if size == "large":
        c = next(c for c in J.edge_cases("e"))
        TJ.run_case(ctx, dict(c, hows=[h for h in c["hows"] if h in (O.INNER, O.LEFT)]))


# ---- groupby: one shape per path, the smallest that reaches it ------------------------------------------------------------------
@once
def groupby_case(name):
    """-> keys, n, vals, aggs, key dtypes, exact rows, options, the property of timings() that proves the path, the oracle's answer"""
    rng = np.random.default_rng(sum(map(ord, name)))
    mask = lambda n, p: O.pack_mask(rng.random(n) < p)
    opts, proof, kd, rtol = {"no_small": 1}, lambda t: t["n_partitions"] > 0, [O.I64], 1e-9
    if name == "small_call":
        n, g = 65_537, 1000
        keys, vals, aggs, exact = [(TG.sparse_keys(rng, n, g), None, O.I64)], [(rng.normal(100, 10, n), None, O.F64)], TG.FIVE, TG.EXACT5
        opts, proof = {}, lambda t: t["n_partitions"] == 0
    elif name == "direct":
        n = (1 << 22) + 5                                              # the path is taken from 2^22 rows
        k = rng.integers(-3, 40, n).astype(np.int64)
        k[rng.random(n) < 0.5] = 7
        keys = [(k, mask(n, 0.01), O.I64)]
        vals = [(rng.normal(100, 10, n), mask(n, 0.1), O.F64), (rng.integers(-99, 99, n).astype(np.int64), None, O.I64)]
        aggs = [(0, O.SUM), (0, O.MEAN), (0, O.MIN), (0, O.MAX), (0, O.COUNT), (1, O.SUM), (1, O.MIN), (1, O.MAX), (1, O.MEAN)]
        exact, opts, proof = [2, 3, 4, 5, 6, 7], {"no_small": 1}, lambda t: t["n_partitions"] == 0
    elif name == "direct_large":
        n = 5_000_000
        k = rng.integers(-3, 90, n).astype(np.int64)
        keys = [(k, mask(n, 0.01), O.I64)]
        vals = [(rng.normal(-5, 3, n), mask(n, 0.1), O.F64)]
        aggs, exact, proof = TG.FIVE, TG.EXACT5, lambda t: t["n_partitions"] == 0
    elif name == "partitioned":
        n, g = 300_000, 50_000
        keys, vals, aggs, exact = [(TG.sparse_keys(rng, n, g), mask(n, 0.01), O.I64)], [(rng.normal(100, 10, n), mask(n, 0.1), O.F64)], TG.FIVE, TG.EXACT5
    elif name == "lean_rounds":
        n, g, ncol = 300_000, 50_000, 6
        k = TG.sparse_keys(rng, n, g)
        k[rng.random(n) < 0.001] = -1
        keys = [(k, mask(n, 0.01), O.I64)]
        vals = [(rng.normal(50 + 5 * c, 2, n), mask(n, 0.1), O.F64) for c in range(ncol)]
        aggs = [(c, op) for c in range(ncol) for op in (O.SUM, O.MEAN, O.MIN, O.MAX)] + [(ncol - 1, O.COUNT)]
        exact = [i for i, (_, op) in enumerate(aggs) if op in (O.MIN, O.MAX, O.COUNT)]
    elif name == "clustered":
        n, g = (1 << 20) + 5, 40_000                                   # the path is taken from 2^20 rows
        keys = [(TG.sparse_keys_from(np.sort(rng.integers(0, g, n))), mask(n, 0.001), O.I64)]
        pool = np.concatenate([rng.normal(size=1000), [np.nan, np.inf, -np.inf, -0.0]])
        vals = [(pool[rng.integers(0, len(pool), n)], None, O.F64), (rng.normal(5, 1, n), None, O.F64)]
        aggs, exact = [(c, op) for c in range(2) for op in (O.SUM, O.MEAN, O.MIN, O.MAX)] + [(0, O.COUNT)], [2, 3, 6, 7, 8]
        proof = lambda t: t["n_partitions"] == -2
    elif name == "absorb_forced":
        n, g = 300_000, 10_000
        ids = TG._skewed_ids(rng, n, g, 0.9, 300)
        k = TG.sparse_keys_from(ids)
        k[::10_003] = -1
        keys = [(k, mask(n, 0.001), O.I64)]
        v = rng.standard_normal(n)
        v[::5021] = np.nan
        vals = [(v, mask(n, 0.1), O.F64), (rng.standard_normal(n), mask(n, 0.5), O.F64)]
        aggs = [(0, O.SUM), (0, O.MIN), (0, O.MAX), (0, O.MEAN), (1, O.SUM), (1, O.MIN), (1, O.MAX), (1, O.COUNT)]
        exact, opts, proof = (1, 2, 5, 6, 7), {"no_small": 1, "no_absorb": -1}, lambda t: t["absorbed_rows"] > 0
    elif name in ("sort_based", "sort_based_generic"):
        n, g = 200_000, 1_000                                          # median, nunique, std / var, first / last in one call
        ids = rng.integers(0, g, n)
        ids[rng.random(n) < 0.3] = 7
        keys = [(TG.sparse_keys_from(ids), mask(n, 0.001), O.I64)]
        vf = (np.round(rng.normal(50, 100, n), 1) + 0.0, None, O.F64)
        vi = (rng.integers(-10**6, 10**6, n).astype(np.int64), mask(n, 0.1), O.I64)
        vu = rng.integers(-6, 6, n).astype(np.float64) / 2.0
        vu[rng.random(n) < 0.01] = np.nan
        vals = [vf, vi, (vu, mask(n, 0.1), O.F64)]
        aggs = [(0, O.MEDIAN), (1, O.MEDIAN), (2, O.NUNIQUE), (1, O.NUNIQUE), (0, O.STD), (0, O.VAR), (1, O.FIRST), (0, O.LAST), (1, O.COUNT)]
        exact = [0, 1, 2, 3, 6, 7, 8]
        opts = {"no_small": 1, "median_generic": int(name.endswith("generic"))}
        proof = lambda t: True
    elif name == "two_keys_packed":
        n = 300_000
        keys = [(rng.integers(0, 300, n).astype(np.uint32), mask(n, 0.01), O.U32CODE), (rng.integers(-50, 50, n).astype(np.int64) * 1000 - 7, None, O.I64)]
        vals, aggs, exact, kd = [(rng.normal(100, 10, n), mask(n, 0.1), O.F64)], TG.FIVE, TG.EXACT5, [O.U32CODE, O.I64]
        proof = lambda t: True
    else:
        raise KeyError(name)
    for col in keys + vals:
        frozen(col[0], col[1])
    return keys, n, vals, aggs, kd, exact, opts, proof, rtol, O.groupby_agg(keys, n, vals, aggs)


def run_groupby(ctx, name):
    keys, n, vals, aggs, kd, exact, opts, proof, rtol, want = groupby_case(name)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        got = ctx.groupby_agg(keys, n, vals, aggs)
        t = ctx.timings()
    finally:
        for k in opts:
            ctx.set_option(k, 0)
    assert_groupby_equal(got, want, kd, int_exact_rows=exact, rtol=rtol)
    assert proof(t), (name, t)


@once
def indices_case():
    rng = np.random.default_rng(2300)
    n, g = 300_000, 2_000
    return [frozen(TG.sparse_keys_from(rng.integers(0, g, n)), O.pack_mask(rng.random(n) < 0.01)) + (O.I64,)], n


GROUPBY = ["small_call", "direct", "partitioned", "lean_rounds", "clustered", "absorb_forced", "sort_based", "sort_based_generic", "two_keys_packed"]
OPS = {"sort": op_sort, "filter": op_filter, "window": op_window, "window_quantile": op_window_quantile, "describe": op_describe,
       "rank": op_rank, "fill": op_fill, "topk": op_topk, "predicate": op_predicate, "cumulative": op_cumulative, "reduce": op_reduce,
       "join": op_join}
SIZES = ("small", "large")
# the ops whose results are defined to the bit (the count / extreme / lag modes of cumulative, describe's order statistics)
BIT_IDENTICAL = ("sort", "filter", "rank", "fill", "topk", "predicate", "cumulative", "describe", "window_quantile")


def run_case(ctx, case):
    """-> the bits of the case's deterministic results, in call order"""
    ctx.log = []
    if case == "group_indices":
        TG.check_group_indices(ctx, *indices_case())
    elif case.startswith("groupby:"):
        run_groupby(ctx, case[8:])
    else:
        name, size = case.split(":")
        OPS[name](ctx, size)
    return ctx.log


CASES = ["groupby:" + g for g in GROUPBY] + ["group_indices"] + ["%s:%s" % (o, s) for o in OPS for s in SIZES]


# ---- a. poisoned workspace ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_a_poisoned_workspace(fresh, case):
    """The case without the hook, then with every block the library hands itself filled with 0x00, 0xFF and 0xA5: each run
    against the reference (inside run_case), the counter moving with every call (inside Watched), and the deterministic results
    the same bits in all four runs."""
    ctx = fresh()
    logs = {"off": run_case(ctx, case)}
    for byte in POISONS:
        ctx.set_poison(byte)
        logs[byte] = run_case(ctx, case)
    ctx.set_poison(None)
    for byte in POISONS:
        assert len(logs[byte]) == len(logs["off"])
        for i, (a, b) in enumerate(zip(logs["off"], logs[byte])):
            assert a == b, "call %d (%s) differs under poison %#x" % (i, a[0], byte)
    if case.split(":")[0] in BIT_IDENTICAL:
        assert logs["off"], "the case logged no deterministic result"


def test_a_poison_covers_a_context_of_its_own_from_the_first_call(fresh):
    """The hook on BEFORE the context's first call: the one-off tables (the estimate's, the census's, the small path's) and the
    first allocation of every arena are filled too, where the tests above meet them warm."""
    import pandrs_amd as pa
    pa.Context.poison_workspace(0xA5)
    for case in ("groupby:small_call", "groupby:partitioned", "groupby:absorb_forced", "group_indices", "sort:small", "fill:small", "predicate:small",
                 "topk:small", "describe:small", "filter:small", "window_quantile:small"):
        ctx = fresh()
        ctx.poison = 0xA5
        run_case(ctx, case)


# ---- b. what the previous call left ------------------------------------------------------------------------------------------------
_fresh_logs = {}


def fresh_log(fresh, case):
    if case not in _fresh_logs:
        _fresh_logs[case] = run_case(fresh(), case)
    return _fresh_logs[case]


@pytest.mark.parametrize("op", list(OPS))
def test_b_a_larger_call_first_and_the_same_call_twice(fresh, op):
    want = fresh_log(fresh, op + ":small")
    ctx = fresh()
    run_case(ctx, op + ":large")
    assert run_case(ctx, op + ":small") == want
    assert run_case(ctx, op + ":small") == want
    run_case(ctx, op + ":large")                                        # and the other way round: the large one over the small one's leftovers


def test_b_groupby_paths_after_each_other(fresh):
    """Every groupby path after a larger call of another path, then twice in a row, on one context (the results against the
    oracle inside run_groupby; group counts and keys are exact there)."""
    ctx = fresh()
    for name in GROUPBY + ["small_call"]:
        run_case(ctx, "groupby:clustered" if name != "clustered" else "groupby:direct_large")
        run_case(ctx, "groupby:" + name)
        run_case(ctx, "groupby:" + name)
        run_case(ctx, "group_indices")


SHARED = {"work": ["sort", "rank", "fill", "predicate", "cumulative", "window_quantile"], "temp": ["sort", "describe", "groupby:direct"],
          "topk": ["topk", "sort"]}


@pytest.mark.parametrize("arena,x", [(a, x) for a, ops in SHARED.items() for x in (ops if a != "topk" else ops[:1])])
def test_b_ops_that_share_an_arena(fresh, arena, x):
    """Large X, then small Y, for every ordered pair of ops that take scratch from the same arena (topk: the sort after it): Y
    against its reference and, bit for bit, against Y on a context that never ran anything else."""
    def large(op):
        return "groupby:direct_large" if op.startswith("groupby") else op + ":large"

    def small(op):
        return op if op.startswith("groupby") else op + ":small"
    ctx = fresh()
    for y in SHARED[arena]:
        if y != x:
            run_case(ctx, large(x))
            assert run_case(ctx, small(y)) == fresh_log(fresh, small(y)), (x, y)


# ---- c. an arena that has to grow under a nested run ------------------------------------------------------------------------------
@once
def chain_case(n):
    """fuzz_ops' filter -> gather -> groupby chain at n rows (its generator draws n: the first seed that draws this one)."""
    for seed in range(200):
        d = FO.draw_chain(np.random.default_rng(seed), 1)
        if d["n"] == n:
            assert d["shape"] == "filter_groupby"
            return d
    raise AssertionError("no seed below 200 draws a chain of %d rows" % n)


def grow_topk(ctx):
    n = 2_000_000                                                       # the candidates' nested sort needs far more than the tiny call left
    x, nulls = column(n, 131)
    TK.check(ctx, x, nulls, ks=[n // 3], paths=(-1,))
    TK.check(ctx, x, nulls, ks=[n // 2], paths=(1,))


def grow_window_quantile(ctx):
    n = N_WQ["large"]
    x, valid, sw = wq_case(n, 102)
    TQ.check(ctx, TQ.col_of(x, valid), n, sw, "rolling", 1000, False, mps=(1,), stats=((False, 0.75),), nan_missing=True)


def grow_chain(ctx):
    FO.run_chain(ctx, chain_case(1_000_003))


@pytest.mark.parametrize("poison", [None, 0xA5])
@pytest.mark.parametrize("what", ["topk", "window_quantile", "chain"])
def test_c_growth_under_a_nested_run(fresh, what, poison):
    ctx = fresh()
    if poison is not None:
        ctx.set_poison(poison)
    if what == "topk":
        run_case(ctx, "topk:small")
        grow_topk(ctx)
    elif what == "window_quantile":
        run_case(ctx, "window_quantile:small")
        grow_window_quantile(ctx)
    else:
        FO.run_chain(ctx, chain_case(4097))
        grow_chain(ctx)


# ---- d. hook off -----------------------------------------------------------------------------------------------------------------------
def test_d_hook_off_fills_nothing_and_a_repeated_call_allocates_nothing(fresh):
    import pandrs_amd as pa
    steady = ["groupby:partitioned", "groupby:small_call", "group_indices", "join:small"] + [op + ":small" for op in OPS if op != "join"]
    ctx = fresh()
    before = pa.Context.workspace_poisoned_bytes()
    for case in steady:
        run_case(ctx, case)                                             # (Watched: the counter stands still during every call)
    events = pa.Context.alloc_events()
    assert events > 0
    for case in steady:
        run_case(ctx, case)
    assert pa.Context.alloc_events() == events, "a repeated call allocated device memory"
    assert pa.Context.workspace_poisoned_bytes() == before
    for bad in (-1, 0x101):
        with pytest.raises(pa.PandrsHipError):
            ctx.set_option("poison_workspace", bad)
    ctx.set_option("poison_workspace", 0x100)                            # the zero byte
    n0 = pa.Context.workspace_poisoned_bytes()
    ctx.poison = 0x00
    run_case(ctx, "sort:small")
    assert pa.Context.workspace_poisoned_bytes() > n0
    assert pa.Context.alloc_events() == events, "the fill allocated device memory"
    ctx.set_poison(None)
