"""pandrs_hip_window and the mirrors' rolling / expanding / ewm (reference src/dataframe/window.rs:13-160 over
src/series/window.rs: Rolling :163-345, Expanding :379-500, EWM :608-724) against numpy restatements of the reference's
loops written here.  A row-order fold is restated exactly: an accumulator starts at -0.0 and the window's values are
added one shifted slice at a time, in ascending rows.  Rolling sum / mean / var / std and min / max / count are compared
bit for bit (NaN positions equal, every other value identical); expanding sum / mean / var / std and EWM within the
bounds of DESIGN.md §2."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402

OPS = {"sum": L.WINDOW_SUM, "mean": L.WINDOW_MEAN, "var": L.WINDOW_VAR, "std": L.WINDOW_STD, "min": L.WINDOW_MIN,
       "max": L.WINDOW_MAX, "count": L.WINDOW_COUNT}


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


from tests.window_ref import (bounds, counts, ewm_close, ewm_ref, expanding_ref_exact, extreme, first_diff, fold,  # noqa: E402,F401
                              pick, rolling_ref, same, two_pass_prefix)


def data_of(rng, n, null_p, special=True):
    x = rng.normal(0, 100, n)
    r = rng.random(n) < 0.3
    x[r] = np.round(x[r])                                                # ties
    if special and n >= 20:
        k = rng.choice(n, size=max(5, n // 200), replace=False)
        x[k] = rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e300, -1e-300], size=len(k))
    valid = rng.random(n) >= null_p
    return x, valid


def col_of(x, valid, dtype=L.F64):
    return (x, None if valid.all() else bits(~valid), dtype)


def win(ctx, col, n, kind, op, **kw):
    return ctx.window(col, n, kind, OPS[op], **kw)


def roll(ctx, col, n, w, op, center=False, mp=None, ddof=1):
    return win(ctx, col, n, L.WINDOW_KIND_ROLLING, op, window=w, min_periods=-1 if mp is None else mp, center=center, ddof=ddof)


# ---- rolling sum / mean / var / std: bit for bit ---------------------------------------------------------------------------
N_FOLD = 6007                 # > 3 tiles of 1792 outputs; w = 5000 streams its halo through LDS in chunks


@pytest.mark.parametrize("w", [1, 2, 3, 63, 64, 65, 1000, 5000, N_FOLD - 1, N_FOLD, N_FOLD + 5])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("null_p", [0.0, 0.1, 1.0])
def test_rolling_fold_is_the_reference_fold(ctx, w, center, null_p):
    rng = np.random.default_rng(w * 7 + int(center) + int(null_p * 10))
    n = N_FOLD
    x, valid = data_of(rng, n, null_p)
    col = col_of(x, valid)
    s, e = bounds(n, w, center)
    cnt = counts(valid, s, e)
    acc = fold(x, valid, s, e)
    with np.errstate(all="ignore"):
        mean = acc / cnt.astype(np.float64)
        sq = fold(x, valid, s, e, mean)
    for mp in (None, 0, 1, max(w // 2, 1)):
        ok = cnt >= (w if mp is None else mp)
        got = roll(ctx, col, n, w, "sum", center, mp)
        assert same(got, np.where(ok, acc, np.nan)), ("sum", mp, first_diff(got, np.where(ok, acc, np.nan)))
        got = roll(ctx, col, n, w, "mean", center, mp)
        assert same(got, np.where(ok, mean, np.nan)), ("mean", mp, first_diff(got, np.where(ok, mean, np.nan)))
        for ddof in (0, 1, 2):
            with np.errstate(all="ignore"):
                var = np.where(ok & (cnt > ddof), sq / (cnt - ddof).astype(np.float64), np.nan)
                std = np.sqrt(var)
            got = roll(ctx, col, n, w, "var", center, mp, ddof)
            assert same(got, var), ("var", mp, ddof, first_diff(got, var))
            got = roll(ctx, col, n, w, "std", center, mp, ddof)
            assert same(got, std), ("std", mp, ddof, first_diff(got, std))


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 1791, 1792, 1793, 4095, 4096, 4097, 8191, 8193, 12_289])
def test_row_counts_around_tiles_words_and_chunks(ctx, n):
    rng = np.random.default_rng(n)
    x, valid = data_of(rng, n, 0.2)
    col = col_of(x, valid)
    for w in (1, 3, 100, 4097):
        for center in (False, True):
            for op in OPS:
                got = roll(ctx, col, n, w, op, center, mp=1)
                want = rolling_ref(x, valid, w, center, op, mp=1)
                assert same(got, want), (w, center, op, first_diff(got, want))


def test_i64_columns_are_read_as_f64(ctx):
    rng = np.random.default_rng(11)
    n = 20_011
    v = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    v[::7] = rng.integers(-1000, 1000, len(v[::7]))
    valid = rng.random(n) > 0.1
    col = (v, bits(~valid), L.I64)
    x = v.astype(np.float64)                                             # `as f64`: round to nearest
    for w in (3, 64, 700):
        for op in OPS:
            got = roll(ctx, col, n, w, op, False, mp=2)
            want = rolling_ref(x, valid, w, False, op, mp=2)
            assert same(got, want), (w, op, first_diff(got, want))


def test_sum_starts_at_negative_zero(ctx):
    """current Rust std folds `Sum for f64` from -0.0: an empty window under min_periods 0, and a window of
    only -0.0, sum to -0.0; one +0.0 makes it +0.0."""
    x = np.array([-0.0, -0.0, 0.0, -0.0, -0.0, -0.0, 5.0, -5.0])
    valid = np.array([False, False, True, True, True, True, True, True])
    col = col_of(x, valid)
    got = roll(ctx, col, 8, 2, "sum", mp=0)
    assert [np.signbit(g) for g in got[:6]] == [True, True, False, False, True, True]
    assert list(got[:6]) == [0.0] * 6 and got[7] == 0.0 and not np.signbit(got[7])
    got = win(ctx, col, 8, L.WINDOW_KIND_EXPANDING, "sum", min_periods=0)
    assert np.signbit(got[0]) and np.signbit(got[1]) and not np.signbit(got[2])
    allneg = col_of(np.full(10, -0.0), np.ones(10, bool))
    assert np.signbit(win(ctx, allneg, 10, L.WINDOW_KIND_EXPANDING, "sum", min_periods=0)).all()
    assert np.signbit(roll(ctx, allneg, 10, 4, "sum", mp=1)).all()
    assert np.isnan(roll(ctx, col, 8, 2, "mean", mp=0)[:2]).all()      # -0.0 / 0


def test_sqrt_and_division_are_correctly_rounded(ctx):
    """About 10^7 random inputs: rolling std at w = 3 takes sqrt of 10^7 quotients, rolling mean at w = 5000 with half
    the cells null divides by thousands of different counts; numpy's sqrt and division are correctly rounded."""
    rng = np.random.default_rng(12)
    n = 10_000_000
    x = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))
    valid = np.ones(n, bool)
    got = roll(ctx, (x, None, L.F64), n, 3, "std")
    want = rolling_ref(x, valid, 3, False, "std")
    assert same(got, want), first_diff(got, want)
    m = 200_003
    xv, vv = x[:m], rng.random(m) > 0.5
    got = roll(ctx, col_of(xv, vv), m, 5000, "mean", mp=1)
    want = rolling_ref(xv, vv, 5000, False, "mean", mp=1)
    assert same(got, want), first_diff(got, want)


def test_host_device_resident_and_unaligned_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(13)
    n = 30_001
    x, valid = data_of(rng, n, 0.1)
    mask = bits(~valid)
    want = {op: rolling_ref(x, valid, 77, True, op, mp=3) for op in OPS}
    res = ctx.upload_column_n(x, mask, L.F64, n)
    dev = (torch.from_numpy(x).to("cuda:0"), torch.from_numpy(mask).to("cuda:0"), L.F64)
    xb = torch.zeros(n + 3, dtype=torch.float64, device="cuda:0")        # one element in: 8-byte aligned, not 256
    xb[1:n + 1] = dev[0]
    mb = torch.zeros(len(mask) + 8, dtype=torch.uint8, device="cuda:0")   # the mask at byte offset 3
    mb[3:3 + len(mask)] = dev[1]
    off = (xb[1:n + 1], mb[3:3 + len(mask)], L.F64)
    for c in ((x, mask, L.F64), res, dev, off):
        for op in OPS:
            got = roll(ctx, c, n, 77, op, True, mp=3)
            got = got.cpu().numpy() if hasattr(got, "cpu") else got
            assert same(got, want[op]), (op, first_diff(got, want[op]))
    got = roll(ctx, dev, n, 77, "sum", True, mp=3)
    assert got.device.type == "cuda" and got.dtype == torch.float64
    res.release()


# ---- rolling min / max / count: O(1) per row, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 64, 1000, 4097, 100_000])
@pytest.mark.parametrize("center", [False, True])
def test_rolling_min_max_count(ctx, w, center):
    rng = np.random.default_rng(w + 3 * int(center))
    n = 250_007
    x, valid = data_of(rng, n, 0.15)
    z = rng.random(n) < 0.02
    x[z] = rng.choice([0.0, -0.0], size=int(z.sum()))
    x[1000:1000 + min(3 * w, 5000)] = np.nan                             # runs of only NaN: +-inf, as the fold's start
    for op in ("min", "max", "count"):
        for mp in (None, 0, 1, max(w // 2, 1)):
            got = roll(ctx, col_of(x, valid), n, w, op, center, mp)
            want = rolling_ref(x, valid, w, center, op, mp=mp)
            assert same(got, want), (op, mp, first_diff(got, want))
    got = roll(ctx, (x, None, L.F64), n, w, "max", center, 1)            # no null mask
    assert same(got, rolling_ref(x, np.ones(n, bool), w, center, "max", mp=1))


def test_min_max_of_signed_zeros_follow_total_order(ctx):
    x = np.array([0.0, -0.0, 0.0, 0.0, -0.0, -0.0])
    col = col_of(x, np.ones(6, bool))
    mn = roll(ctx, col, 6, 2, "min", mp=1)
    mx = roll(ctx, col, 6, 2, "max", mp=1)
    assert list(np.signbit(mn)) == [False, True, True, False, True, True]
    assert list(np.signbit(mx)) == [False, False, False, False, False, True]


# ---- expanding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 4095, 4096, 4097, 100_003, 1_000_003])
def test_expanding_min_max_count_exact(ctx, n):
    rng = np.random.default_rng(n)
    x, valid = data_of(rng, n, 0.3)
    col = col_of(x, valid)
    v = np.where(valid & ~np.isnan(x), x, np.inf)
    for mp in (0, 1, 50):
        c = np.cumsum(valid)
        want_count = np.where(c >= mp, c, 0).astype(np.float64)
        assert same(win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "count", min_periods=mp), want_count)
        mn = np.minimum.accumulate(v)
        got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "min", min_periods=mp)
        mn_ok = np.where(c >= mp, mn, np.nan)
        # np.minimum's +-0 tie is not the total order: restate it where both zero signs have been seen
        assert np.array_equal(np.isnan(got), np.isnan(mn_ok))
        assert np.array_equal(got[~np.isnan(got)], mn_ok[~np.isnan(mn_ok)])
        if n <= 100_003:
            assert same(got, expanding_ref_exact(x, valid, "min", mp))
            assert same(win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "max", min_periods=mp), expanding_ref_exact(x, valid, "max", mp))


@pytest.mark.parametrize("n", [1, 5, 4097, 100_003, 2_000_003])
def test_expanding_sum_mean_within_bound(ctx, n):
    rng = np.random.default_rng(n + 1)
    x = rng.normal(3, 1000, n) * np.exp(rng.uniform(-5, 5, n))
    valid = rng.random(n) > 0.1
    col = col_of(x, valid)
    xz = np.where(valid, x, 0.0)
    want = np.cumsum(xz)                                                 # row-order prefix (numpy's cumsum is sequential)
    bound = 1e-9 * np.cumsum(np.abs(xz))
    c = np.cumsum(valid)
    for mp in (0, 3):
        got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "sum", min_periods=mp)
        ok = c >= mp
        assert np.array_equal(np.isnan(got), ~ok)
        assert (np.abs(got[ok] - want[ok]) <= bound[ok]).all()
        got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "mean", min_periods=mp)
        ok2 = ok & (c > 0)
        assert np.array_equal(np.isnan(got), ~ok2)
        assert (np.abs(got[ok2] - want[ok2] / c[ok2]) <= bound[ok2] / c[ok2]).all()


def test_expanding_sum_nan_and_inf_positions(ctx):
    x = np.array([1.0, np.inf, 2.0, -np.inf, 3.0, 1.0, np.nan, 4.0])
    valid = np.array([True, True, True, False, True, True, True, True])
    got = win(ctx, col_of(x, valid), 8, L.WINDOW_KIND_EXPANDING, "sum", min_periods=1)
    assert list(got[:6]) == [1.0, np.inf, np.inf, np.inf, np.inf, np.inf] and np.isnan(got[6:]).all()
    x2 = x.copy()
    x2[3] = -np.inf
    got = win(ctx, col_of(x2, np.ones(8, bool)), 8, L.WINDOW_KIND_EXPANDING, "sum", min_periods=1)
    assert list(got[:3]) == [1.0, np.inf, np.inf] and np.isnan(got[3:]).all()
    for op in ("var", "std"):                                              # (x - mean) is NaN once an inf is in
        got = win(ctx, col_of(x, valid), 8, L.WINDOW_KIND_EXPANDING, op, min_periods=1, ddof=0)
        assert got[0] == 0.0 and np.isnan(got[1:]).all()


@pytest.mark.parametrize("n", [3, 4097, 9001])
def test_expanding_var_std_within_bound(ctx, n):
    rng = np.random.default_rng(n + 2)
    x = rng.normal(50, 10, n)
    valid = rng.random(n) > 0.2
    col = col_of(x, valid)
    c, m2 = two_pass_prefix(x, valid)
    amax = np.maximum.accumulate(np.abs(np.where(valid, x, 0.0)))
    for ddof in (0, 1, 2):
        for mp in (0, 4):
            ok = (c >= mp) & (c > ddof)
            with np.errstate(all="ignore"):
                var = m2 / (c - ddof)
            got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "var", min_periods=mp, ddof=ddof)
            assert np.array_equal(np.isnan(got), ~ok)
            assert (np.abs(got[ok] - var[ok]) <= 1e-9 * np.abs(var[ok]) + 1e-12 * amax[ok] ** 2).all()
            got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "std", min_periods=mp, ddof=ddof)
            std = np.sqrt(var)
            assert np.array_equal(np.isnan(got), ~ok)
            assert (np.abs(got[ok] - std[ok]) <= 1e-9 * std[ok] + 1e-6 * amax[ok]).all()


# ---- EWM -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 100, 4097, 10_000])
@pytest.mark.parametrize("alpha", [0.05, 0.5, 1.0, 2.0 / 31.0])
def test_ewm_against_the_reference_loop(ctx, n, alpha):
    rng = np.random.default_rng(n + int(alpha * 100))
    x = rng.normal(10, 5, n)
    valid = rng.random(n) > 0.25
    valid[: min(n, 7)] = False                                           # leading nulls: NaN rows
    if n > 20:
        valid[7] = True
    col = col_of(x, valid)
    for op in ("mean", "std", "var"):
        got = win(ctx, col, n, L.WINDOW_KIND_EWM, op, alpha=alpha)
        want = ewm_ref(x, valid, alpha, op)
        assert ewm_close(got, want, x, valid, op == "var"), op
        first = np.flatnonzero(valid)
        lead = first[0] if len(first) else n
        assert np.isnan(got[:lead]).all()                                # rows before the first value
        if op == "mean" and len(first):
            assert got[lead] == x[lead]                                  # the first value as itself
        if op != "mean" and len(first):
            assert np.isnan(got[lead])                                   # std / var: NaN at the first value too


def test_ewm_var_is_the_std_output_squared(ctx):
    rng = np.random.default_rng(21)
    n = 50_000
    x = rng.normal(0, 3, n)
    valid = rng.random(n) > 0.1
    col = col_of(x, valid)
    std = win(ctx, col, n, L.WINDOW_KIND_EWM, "std", alpha=0.1)
    var = win(ctx, col, n, L.WINDOW_KIND_EWM, "var", alpha=0.1)
    assert same(var, std * std)
    # the null rows right after the first value repeat sqrt(0) = 0 (series/window.rs:703-704)
    x2 = np.array([np.nan, 4.0, 1.0, 1.0, 9.0])
    v2 = np.array([False, True, False, False, True])
    got = win(ctx, col_of(x2, v2), 5, L.WINDOW_KIND_EWM, "std", alpha=0.5)
    assert np.isnan(got[:2]).all() and list(got[2:4]) == [0.0, 0.0] and got[4] == math.sqrt(0.5 * (0.5 * 25.0))


def test_ewm_at_scale_against_lfilter(ctx):
    from scipy.signal import lfilter
    rng = np.random.default_rng(22)
    n = 3_000_000
    x = rng.normal(100, 20, n)
    valid = np.ones(n, bool)
    for alpha in (0.01, 0.3):
        got = win(ctx, (x, None, L.F64), n, L.WINDOW_KIND_EWM, "mean", alpha=alpha)
        want = lfilter([alpha], [1.0, -(1.0 - alpha)], x, zi=[(1.0 - alpha) * x[0]])[0]
        assert ewm_close(got, want, x, valid)
        # std: the variance recurrence is affine in var once the mean series is known
        mprev = np.concatenate([[x[0]], want[:-1]])
        d = x - mprev
        u = (1.0 - alpha) * (alpha * d * d)
        u[0] = 0.0
        var = lfilter([1.0], [1.0, -(1.0 - alpha)], u)
        std = np.sqrt(var)
        std[0] = np.nan
        got = win(ctx, (x, None, L.F64), n, L.WINDOW_KIND_EWM, "std", alpha=alpha)
        assert ewm_close(got, std, x, valid)


# ---- known answers from the reference's tests -------------------------------------------------------------------------------
def test_known_answers_from_the_reference_tests(ctx):
    """tests/window_test.rs and tests/comprehensive_window_test.rs (median / quantile / apply excluded), as data."""
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "window_known_answers.json")))["cases"]
    assert len(cases) >= 20
    for case in cases:
        x = np.array([np.nan if v is None else v for v in case["values"]], np.float64)
        valid = np.array([v is not None for v in case["values"]])
        kind = {"rolling": L.WINDOW_KIND_ROLLING, "expanding": L.WINDOW_KIND_EXPANDING, "ewm": L.WINDOW_KIND_EWM}[case["kind"]]
        kw = {k: case[k] for k in ("window", "min_periods", "ddof", "alpha") if k in case}
        got = win(ctx, col_of(x, valid), len(x), kind, case["op"], **kw)
        for row, want in case["checks"]:
            if want is None:
                assert np.isnan(got[row]), (case["source"], row, got[row])
            else:
                assert abs(got[row] - want) <= case.get("tol", 0.0), (case["source"], row, got[row], want)


# ---- torch at 50 M rows, one call above 2^31 rows -----------------------------------------------------------------------------
def test_50m_rows_match_torch(ctx):
    import torch
    n = 50_000_000
    g = torch.Generator(device="cuda:0").manual_seed(7)
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=g)
    col = (x, None, L.F64)
    for w in (30, 1000):
        got = win(ctx, col, n, L.WINDOW_KIND_ROLLING, "max", window=w, min_periods=-1)
        want = x.unfold(0, w, 1).amax(-1)
        assert torch.equal(got[w - 1:], want) and bool(torch.isnan(got[:w - 1]).all())
        del want
    got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "max", min_periods=0)
    assert torch.equal(got, torch.cummax(x, 0).values)
    got = win(ctx, col, n, L.WINDOW_KIND_EXPANDING, "sum", min_periods=0)
    want = torch.cumsum(x, 0)
    bound = 1e-9 * torch.cumsum(x.abs(), 0)
    assert bool(((got - want).abs() <= bound).all())
    del got, want, bound, x


def test_one_call_above_2_pow_31_rows(ctx):
    """n = 2^31 + 12 345: rolling mean, w = 5, exact on the first and last 10^6 rows and on a strided sample."""
    import torch
    n = (1 << 31) + 12_345
    g = torch.Generator(device="cuda:0").manual_seed(9)
    x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    step = 1 << 28
    for s in range(0, n, step):
        x[s:s + step].normal_(generator=g)
    got = win(ctx, (x, None, L.F64), n, L.WINDOW_KIND_ROLLING, "mean", window=5, min_periods=-1)
    assert got.numel() == n
    m = 1_000_000
    head, tail = x[:m].cpu().numpy(), x[n - m - 4:].cpu().numpy()
    ones = np.ones(m + 4, bool)
    want_head = rolling_ref(head, ones[:m], 5, False, "mean")
    assert same(got[:m].cpu().numpy(), want_head)
    want_tail = rolling_ref(tail, ones, 5, False, "mean")[4:]
    assert same(got[n - m:].cpu().numpy(), want_tail)
    rows = torch.arange(4, n, 7_919_333, device="cuda:0")
    xs = torch.stack([x[rows - 4 + k] for k in range(5)], 1).cpu().numpy()
    acc = np.full(len(rows), -0.0)
    for k in range(5):
        acc = acc + xs[:, k]
    assert same(got[rows].cpu().numpy(), acc / 5.0)
    del x, got


# ---- statuses --------------------------------------------------------------------------------------------------------------
def test_bad_specs_and_types(ctx):
    import pandrs_amd as pa
    x = np.arange(10, dtype=np.float64)
    with pytest.raises(pa.ColumnTypeMismatch) as e:
        ctx.window((np.zeros(10, np.uint32), None, L.U32CODE), 10, L.WINDOW_KIND_ROLLING, L.WINDOW_SUM, window=3)
    assert e.value.status == L.ERR_TYPE_MISMATCH
    for kw in (dict(kind=L.WINDOW_KIND_ROLLING, op=L.WINDOW_SUM, window=0),
               dict(kind=L.WINDOW_KIND_ROLLING, op=L.WINDOW_SUM, window=3, ddof=-1),
               dict(kind=L.WINDOW_KIND_ROLLING, op=9, window=3),
               dict(kind=L.WINDOW_KIND_EXPANDING, op=L.WINDOW_SUM, min_periods=-1),
               dict(kind=L.WINDOW_KIND_EWM, op=L.WINDOW_SUM, alpha=0.5),
               dict(kind=L.WINDOW_KIND_EWM, op=L.WINDOW_MEAN, alpha=float("nan")),
               dict(kind=7, op=L.WINDOW_SUM)):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.window((x, None, L.F64), 10, **kw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, kw
    assert len(ctx.window((x[:0], None, L.F64), 0, L.WINDOW_KIND_ROLLING, L.WINDOW_SUM, window=3)) == 0


def test_memory_limit_and_threshold():
    import pandrs_amd as pa
    lib = L.load()
    try:
        cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        n = 20_000_000                                                  # 160 MB staged + 320 MB of prefix / suffix rows
        big = (np.zeros(n), None, L.F64)
        with pytest.raises(pa.PandrsHipError) as e:
            c.window(big, n, L.WINDOW_KIND_ROLLING, L.WINDOW_MIN, window=10)
        assert e.value.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e.value)
        x = np.arange(1000, dtype=np.float64)
        got = c.window((x, None, L.F64), 1000, L.WINDOW_KIND_ROLLING, L.WINDOW_MAX, window=10, min_periods=1)   # still works
        assert same(got, rolling_ref(x, np.ones(1000, bool), 10, False, "max", mp=1))
        c.close()
        cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        with pytest.raises(pa.BelowThreshold) as e:
            c.window((x, None, L.F64), 1000, L.WINDOW_KIND_ROLLING, L.WINDOW_SUM, window=3)
        assert e.value.status == L.ERR_BELOW_THRESHOLD
        y = np.arange(20_000, dtype=np.float64)
        got = c.window((y, None, L.F64), 20_000, L.WINDOW_KIND_EXPANDING, L.WINDOW_COUNT, min_periods=0)
        assert same(got, np.arange(1, 20_001, dtype=np.float64))
        c.close()
    finally:
        lib.pandrs_hip_init(None)
        pa.Context(0).close()        # resets the limit


# ---- frame level -----------------------------------------------------------------------------------------------------------
def _frame(rng, n):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("id", F.Int64Column(np.arange(n)))
    df.add_column("f", F.Float64Column.with_nulls(rng.normal(0, 1, n), rng.random(n) < 0.2))
    df.add_column("i", F.Int64Column(rng.integers(-50, 50, n)))
    df.add_column("s", F.StringColumn(list(rng.choice(["a", "b"], n))))
    return df


def _floats(df, name):
    return np.asarray(df.column(name).data, np.float64)


def test_frame_rolling_expanding_ewm(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(41)
    n = 3000
    df = _frame(rng, n)
    f = df.column("f")
    x = np.asarray(f.data, np.float64)
    valid = np.array([not f.is_null(k) for k in range(n)])
    r = df.rolling(10, "f", "Mean")
    assert r.column_names == ["id", "f", "i", "s", "f_Mean"] and r.row_count() == n
    assert isinstance(r.column("f_Mean"), F.Float64Column) and r.column("f_Mean").null_mask is None
    assert same(_floats(r, "f_Mean"), rolling_ref(x, valid, 10, False, "mean"))
    r = df.rolling(7, "f", "std", "sd", min_periods=2, center=True, ddof=0)
    assert r.column_names[-1] == "sd" and same(_floats(r, "sd"), rolling_ref(x, valid, 7, True, "std", mp=2, ddof=0))
    r = df.rolling(5, "i", "count")
    assert same(_floats(r, "i_count"), rolling_ref(df.column("i").data.astype(np.float64), np.ones(n, bool), 5, False, "count"))
    r = df.expanding(3, "i", "MAX")
    iv = np.asarray(df.column("i").data, np.float64)
    assert same(_floats(r, "i_MAX"), expanding_ref_exact(iv, np.ones(n, bool), "max", 3))
    r = df.expanding(1, "f", "var", "v")
    c, m2 = two_pass_prefix(x, valid)
    with np.errstate(all="ignore"):
        want = np.where(c > 1, m2 / (c - 1), np.nan)
    got = _floats(r, "v")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    r = df.ewm("f", "mean", span=9)
    assert ewm_close(_floats(r, "f_mean"), ewm_ref(x, valid, 2.0 / 10.0, "mean"), x, valid)
    r = df.ewm("f", "std", alpha=0.3, new_column_name="e")
    assert ewm_close(_floats(r, "e"), ewm_ref(x, valid, 0.3, "std"), x, valid)
    r = df.ewm("f", "var", halflife=4.0)
    a = 1.0 - math.exp(-math.log(2.0) / 4.0)
    assert ewm_close(_floats(r, "f_var"), ewm_ref(x, valid, a, "var"), x, valid, sq=True)
    r = df.ewm("f", "mean", span=3, alpha=0.9)                           # span wins (window.rs:136-141)
    assert ewm_close(_floats(r, "f_mean"), ewm_ref(x, valid, 0.5, "mean"), x, valid)


def test_frame_rolling_sum_without_nulls(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(42)
    n = 10_000
    x = rng.normal(0, 1, n)
    df = F.OptimizedDataFrame()
    df.add_column("x", F.Float64Column(x))
    got = df.rolling(64, "x", "sum").column("x_sum").data
    assert same(np.asarray(got), rolling_ref(x, np.ones(n, bool), 64, False, "sum"))


def test_cpp_mirror_computes_windows():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "window_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
