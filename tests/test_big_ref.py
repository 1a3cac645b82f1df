"""The closed forms of tests/big_ref.py are right: at about 20 000 rows, with the pivot at a few thousand and n just below, at and
above a multiple of every kernel's tile, each generator's answer over ALL rows equals the op's numpy twin on the materialised
column.  No GPU: the generators run on the CPU here, so a failure of tests/test_gpu_column_ops_beyond_2g.py is the kernel's."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import big_ref as B                       # noqa: E402
from tests import cumulative_ref as CR               # noqa: E402
from tests import eval_ref as ER                     # noqa: E402
from tests import predicate_ref as PR                # noqa: E402
from tests import window_ref as WR                   # noqa: E402
from tests.describe_ref import describe_ref, percentile_ref     # noqa: E402
from tests.fill_ref import fill_twin                 # noqa: E402
from tests.rank_ref import rank_ref                  # noqa: E402
from tests.topk_ref import idx_extreme_ref, topk_ref             # noqa: E402
from tests.window_quantile_ref import window_quantile_fast       # noqa: E402

CPU = "cpu"
TILE = 20_480                                        # a multiple of 2048 and 4096, the tiles of the kernels under test
SIZES = [TILE - 1, TILE, TILE + 1]
PIVOT = 5000


def rows_of(n):
    return B.arange(0, n, CPU)


def np_same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind != "f":
        return got.dtype == want.dtype and np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.uint64), want[~wn].view(np.uint64))


def test_the_bitmap_helpers_round_trip():
    for n in (1, 7, 8, 9, 1000, 1003):
        flags = lambda i: (i * 7) % 5 < 2            # noqa: E731
        bits = B.pack_bits(n, flags, CPU, ch=64)
        want = np.packbits(flags(rows_of(n)).numpy(), bitorder="little")
        assert np.array_equal(bits.numpy(), want)
        assert torch.equal(B.bits_at(bits, rows_of(n)), flags(rows_of(n)))
    out = B.fill(torch.empty(1000, dtype=torch.int64), lambda i: 3 * i, ch=64)
    assert torch.equal(out, 3 * rows_of(1000))
    rows = B.sample_rows(10_000, 5000, CPU, extra=[7000], m=100, stride=999, halo=4)
    assert torch.equal(rows, torch.unique(rows)) and int(rows[0]) == 0 and int(rows[-1]) == 9999
    assert {4900, 5099, 6996, 7003, 999 * 3} <= set(rows.tolist()) and 6000 not in set(rows.tolist())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("M,f64", [(3, False), (3, True), (1021, True), (1021, False), (4096, False), (1 << 19, False)])
def test_rank(n, M, f64):
    g = B.Rank(n, PIVOT, CPU, M=M, f64=f64)
    data, bits, _ = g.column()
    rows = rows_of(n)
    nulls = g.nulls_at(rows).numpy()
    assert np.array_equal(bits.numpy(), np.packbits(nulls, bitorder="little")) and torch.equal(B.bits_at(bits, rows), g.nulls_at(rows))
    assert g.pivot < g.m < n
    for method in g.calls:
        assert np_same(g.expected(method, rows).numpy(), rank_ref(data.numpy(), nulls, method)), method
    if M == 3:                                       # a tie run straddles sorted position `pivot`
        starts = np.cumsum([0] + [(g.m - v + 2) // 3 for v in range(3)])
        assert any(s < PIVOT < e for s, e in zip(starts[:-1], starts[1:])) and starts[-1] == g.m


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("pivot,period", [(5000, 97), (12_000, 4099)])
def test_fill(n, f64, pivot, period):
    g = B.Fill(n, pivot, CPU, f64=f64, period=period, hole=(3000, 1000), tail=500)
    data, bits, _ = g.column()
    rows = rows_of(n)
    nulls = None if bits is None else g.nulls_at(rows).numpy()
    if bits is not None:
        assert np.array_equal(bits.numpy(), np.packbits(nulls, bitorder="little"))
    valid = g.valid_at(rows).numpy()
    assert not valid[0] and not valid[g.h0:g.h1].any() and not valid[g.end:].any() and valid[g.first_valid] and valid[g.last_valid]
    assert all(0 <= r <= n for r in g.structural_rows())
    for method in g.calls:
        want, gone = fill_twin(data.numpy(), nulls, method, g.value if method == B.VALUE else None)
        cells, still = g.expected(method, rows)
        assert cells.numpy().dtype == want.dtype and np_same(cells.numpy(), want), method
        assert np.array_equal(still.numpy(), gone) and g.missing(method) == int(gone.sum()), method


@pytest.mark.parametrize("n", SIZES)                 # TILE + 1 is a multiple of 3: the three-valued column's mean is exactly 0
@pytest.mark.parametrize("kind", ["tri", "ramp"])
def test_describe_quantiles_topk_arg_extreme(n, kind):
    g = B.Ordered(n, PIVOT, CPU, kind)
    data, _, dtype = g.column()
    x = data.numpy()
    want = describe_ref(x, None, x.dtype)
    got, scale = g.describe()
    for k, f in (("count", "count"), ("min", "min"), ("25%", "q1"), ("50%", "median"), ("75%", "q3"), ("max", "max")):
        assert got[f] == want[k], (k, got[f], want[k])
    if kind == "tri" and n % 3 == 0:
        assert got["mean"] == 0.0
    # the twin folds n cells in row order: n rounding errors of at most eps / 2 each, relative to the running magnitude
    assert abs(got["mean"] - want["mean"]) <= n * 2.0 ** -52 * scale and abs(got["std"] - want["std"]) <= n * 2.0 ** -52 * want["std"]
    assert abs(scale - np.abs(x).mean()) <= 1e-12 * scale
    for p in g.percentiles:
        assert g.percentile(p) == percentile_ref(want["sorted"], p), p
    assert all(g.sorted_at(k) == want["sorted"][k] for k in (0, 1, n // 3 - 1, n // 3, n // 3 + 1, PIVOT - 1, PIVOT, n - 2, n - 1))
    for k in g.ks:
        for largest in (True, False):
            rows, n_num = topk_ref(x, None, k, largest)
            assert n_num == k and np.array_equal(g.topk_rows(largest, B.arange(0, k, CPU)).numpy(), rows), (k, largest)
    assert g.arg_extreme() == idx_extreme_ref(x)
    assert PIVOT + 5 in g.ks and 1 in g.ks


@pytest.mark.parametrize("n", SIZES)
def test_window_quantile(n):
    g = B.RollingMedian(n, PIVOT, CPU)
    x = g.column()[0].numpy()
    assert len(np.unique(x)) == n                    # all distinct: no window holds a tie
    rows = rows_of(n)
    for _, w in g.calls:
        assert np_same(g.expected(w, rows).numpy(), window_quantile_fast(x, None, "rolling", w=w)), w
    e = B.ExpandingMedian(n, PIVOT, CPU)
    assert np_same(e.expected(rows).numpy(), window_quantile_fast(e.column()[0].numpy(), None, "expanding", min_periods=1))


def program_of(named):
    return [(ER.OP[name], arg) for name, arg in named]


@pytest.mark.parametrize("n", SIZES)
def test_eval(n):
    g = B.Eval(n, PIVOT, CPU)
    rows = rows_of(n)
    cols = [(d.numpy(), None if b is None else g.c_null_at(rows).numpy(), dt) for d, b, dt in g.value_columns()]
    assert np.array_equal(g.value_columns()[2][1].numpy(), np.packbits(g.c_null_at(rows).numpy(), bitorder="little"))
    res = ER.evaluate(cols, n, program_of(g.VALUE_PROGRAM))
    cells, nulls = g.expected_values(rows)
    assert not res.is_mask and not res.zero_tie
    assert np.array_equal(np.isnan(cells.numpy()), np.isnan(res.values)) and np_same(cells.numpy(), res.values)
    assert np.array_equal(nulls.numpy(), res.nulls) and res.count > 0 and (~np.isnan(res.values)).sum() > n // 2
    res = ER.evaluate([(d.numpy(), None, dt) for d, _, dt in g.mask_columns()], n, program_of(g.mask_program))
    assert res.is_mask and np.array_equal(g.expected_mask(rows).numpy(), res.mask)
    assert B.count_true(n, g.expected_mask, CPU, ch=4096) == res.count
    assert res.mask[g.lo + 1] and res.mask[g.hi - 1] and res.mask[PIVOT] and not res.mask[g.lo] and not res.mask[g.hi]


@pytest.mark.parametrize("n", SIZES)
def test_isin(n):
    g = B.Isin(n, PIVOT, CPU)
    x = g.column()[0].numpy()
    rows = rows_of(n)
    for which, negate in g.calls + (("few", True),):
        vals = g.values(which).numpy()
        bits, count = PR.isin(x, None, PR.I64, vals, PR.I64, negate)
        flags = g.expected(which, negate, rows)
        assert np.array_equal(np.packbits(flags.numpy(), bitorder="little"), bits) and g.count(which, negate) == count, (which, negate)
        assert all(0 <= r < n for r in g.structural_rows(which))
    many = g.values("many").numpy()
    assert (many < PIVOT).any() and (many > PIVOT).any() and (many >= n).any() and len(np.unique(many)) == g.n_many


@pytest.mark.parametrize("n", SIZES)
def test_masked_predicate(n):
    g = B.MaskedPredicate(n, PIVOT, CPU)
    data, bits, _ = g.column()
    rows = rows_of(n)
    assert (g.GT, g.ISNA) == (PR.GT, PR.ISNA)
    for op, a in g.calls:
        want, count = PR.predicate(data.numpy(), bits.numpy(), op, a)
        assert np.array_equal(np.packbits(g.expected(op, rows).numpy(), bitorder="little"), want) and g.count(op) == count, op


@pytest.mark.parametrize("n", SIZES)
def test_window(n):
    g = B.Window(n, PIVOT, CPU)
    rows = rows_of(n)
    ones = np.ones(n, bool)
    for name, what in g.calls:
        x = g.column(name)[0].numpy()
        if what == "rolling_max":
            assert np_same(g.rolling_max(name, 0, n).numpy(), WR.rolling_ref(x, ones, g.W, False, "max")), name
            assert np_same(g.rolling_max(name, 4000, 4100).numpy(), WR.rolling_ref(x, ones, g.W, False, "max")[4000:4100]), name
        elif what == "expanding_max":
            assert np_same(g.expected(name, what, rows).numpy(), WR.rolling_ref(x, ones, n + 1, False, "max", mp=0))
        elif what == "expanding_sum":
            want = g.expected(name, what, rows).numpy()
            assert np.array_equal(want, np.cumsum(x)) and WR.expanding_sum_mean_close(want, x, ones, 0, False)
        else:
            want = g.expected(name, what, rows).numpy()
            assert WR.ewm_close(want, WR.ewm_ref(x, ones, 0.5, "mean"), x, ones) and want[0] == 0.0
    t = g.column("trend")[0].numpy()                 # the running maximum still changes after the pivot, and at the very end
    assert np.maximum.accumulate(t)[PIVOT] < np.maximum.accumulate(t)[-1] and len(np.unique(t)) == n


@pytest.mark.parametrize("n", SIZES)
def test_cumulative_and_lag(n):
    g = B.Cumulative(n, PIVOT, CPU)
    rows = rows_of(n)
    assert {c[1] for calls in g.calls.values() for c in calls if c[0] == "cum"} == set(CR.CUM_OPS)
    for name, calls in g.calls.items():
        data, bits, _ = g.column(name)
        x = data.numpy()
        nulls = None if bits is None else g.nulls_at(name, rows).numpy()
        if bits is not None:
            assert np.array_equal(bits.numpy(), np.packbits(nulls, bitorder="little"))
        for call in calls:
            want, gone = CR.cum_twin(x, nulls, call[1]) if call[0] == "cum" else CR.lag_twin(x, nulls, call[1], call[2])
            cells, flags, count = g.expected(name, call, rows)
            assert cells.numpy().dtype == want.dtype and np_same(cells.numpy(), want), (name, call)
            assert np.array_equal(flags.numpy(), gone) and count == int(gone.sum()), (name, call)
