"""pandrs_hip_cumulative / pandrs_hip_lag and the mirrors' cumsum / cumprod / cummax / cummin / cumcount / shift / diff /
pct_change (reference src/dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094) against tests/cumulative_ref.py.
MAX, MIN, COUNT and the three lags are compared bit for bit (the uint64 view).  SUM is bit for bit on integer-valued data and
within 2 gamma_k sum|x| elsewhere; PROD is within 2 gamma_k relative wherever the reference's running product is normal, and
equal in class and sign elsewhere (pandrs_hip.h derives both bounds)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests.cumulative_ref import (COUNT, CUM_OPS, DIFF, LAG_OPS, MAX, MIN, NAN, PCT_CHANGE, PROD, SHIFT, SUM, TINY, bits, compare_cells,  # noqa: E402
                                  cum_loop, cum_twin, lag_loop, lag_twin, same_bits)

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
T = int(re.search(r"cum_tile_rows = (\d+)", HEADER).group(1))
PER_CU = int(re.search(r"cum_blocks_per_cu = (\d+)", HEADER).group(1))


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid():
    import torch
    return PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


def dtype_of(x):
    return L.I64 if x.dtype == np.int64 else L.F64


def host(vals, mask, n):
    if not isinstance(vals, np.ndarray):
        vals, mask = vals.cpu().numpy(), None if mask is None else mask.cpu().numpy()
    flags = np.zeros(n, bool) if mask is None else np.unpackbits(mask, bitorder="little")[:n].astype(bool)
    return vals, mask, flags


def check_cum(ctx, x, nulls=None, ops=CUM_OPS, col=None, exact=False, wants=None, **kw):
    """One column under `ops` against the vectorised restatement: the cells, the mask, the count, and `mask is None` exactly
    when no bit is set; `col` overrides how the column is passed, `wants` carries twins computed before."""
    x = np.asarray(x)
    n = x.shape[0]
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype_of(x))
    wants = {} if wants is None else wants
    for op in ops:
        if op not in wants:
            wants[op] = cum_twin(x, nulls, op)
        want, gone = wants[op]
        vals, mask, n_null = ctx.cumulative(col, n, op, **kw)
        vals, mask, flags = host(vals, mask, n)
        assert vals.dtype == want.dtype
        compare_cells(op, vals, want, x, nulls, exact)
        assert n_null == int(gone.sum()) and (mask is None) == (n_null == 0), (op, n_null, int(gone.sum()))
        assert np.array_equal(flags, gone), op
    return wants


def check_lag(ctx, x, nulls, periods, ops=LAG_OPS, col=None, **kw):
    x = np.asarray(x)
    n = x.shape[0]
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype_of(x))
    for op in ops:
        if op != SHIFT and periods < 0:
            continue
        want, gone = lag_twin(x, nulls, op, periods)
        vals, mask, n_null = ctx.lag(col, n, op, periods, **kw)
        vals, mask, flags = host(vals, mask, n)
        assert same_bits(vals, want), (op, periods, n, np.flatnonzero(vals.view(np.uint64) != want.view(np.uint64))[:5])
        assert n_null == int(gone.sum()) and (mask is None) == (n_null == 0), (op, periods, n_null, int(gone.sum()))
        assert np.array_equal(flags, gone), (op, periods)


def columns_of(n, seed):
    """F64 with NaN cells, F64 with null bits, I64 with null bits: small integers, so SUM is bit for bit; the products are
    powers of two that leave f64's range after a few thousand rows, so the sticky rewrite runs wherever n allows."""
    rng = np.random.default_rng(seed)
    v = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 2.0, 4.0]), n)
    miss = rng.random(n) < 0.2
    return [(np.where(miss, np.nan, v), None), (v, miss), (v.astype(np.int64), miss)]


def passed_as(ctx, x, nulls):
    """The column on the host, on the device, resident, and on the device 8 bytes off a 16-byte boundary with its mask at an
    odd byte offset -> [(col, release or None)]"""
    import torch
    n, dt = x.shape[0], dtype_of(x)
    mask = None if nulls is None else bits(nulls)
    dx = torch.from_numpy(x).cuda()
    dm = None if mask is None else torch.from_numpy(mask).cuda()
    pad = torch.empty(n + 1, dtype=dx.dtype, device="cuda:0")
    pad[1:] = dx
    assert pad.data_ptr() % 16 == 0
    padm = None
    if mask is not None:
        padm = torch.empty(mask.shape[0] + 3, dtype=torch.uint8, device="cuda:0")
        padm[3:] = dm
        padm = padm[3:]
    res = ctx.upload_column(x, mask, dt)
    return [((x, mask, dt), None), ((dx, dm, dt), None), (res, res.release), ((pad[1:], padm, dt), None)]


# ---- shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = {"1": lambda g: 1, "2": lambda g: 2, "63": lambda g: 63, "64": lambda g: 64, "65": lambda g: 65, "127": lambda g: 127,
          "128": lambda g: 128, "129": lambda g: 129, "T-1": lambda g: T - 1, "T": lambda g: T, "T+1": lambda g: T + 1,
          "2T+1": lambda g: 2 * T + 1, "fewer tiles than workgroups": lambda g: 5 * T + 77,
          "(G+1)T+3": lambda g: (g + 1) * T + 3, "3GT+T/2+1": lambda g: 3 * g * T + T // 2 + 1}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_columns_and_memory_spaces(ctx, grid, shape):
    n = SHAPES[shape](grid)
    for x, nulls in columns_of(n, n):
        wants = {}
        for k, (col, release) in enumerate(passed_as(ctx, x, nulls)):
            try:
                check_cum(ctx, x, nulls, col=col, exact=True, wants=wants, out_device=bool(k % 2))
            finally:
                if release:
                    release()


@pytest.mark.parametrize("shape", ["1", "65", "T+1", "(G+1)T+3"])
def test_lag_periods(ctx, grid, shape):
    n = SHAPES[shape](grid)
    rng = np.random.default_rng(n + 1)
    x = rng.normal(0.0, 10.0, n)
    x[rng.random(n) < 0.05] = 0.0
    nulls = rng.random(n) < 0.1
    i = rng.integers(-1000, 1000, n)
    for periods in (0, 1, -1, 2, 63, 64, 65, T, T + 1, n - 1, n, n + 5, -(n + 5)):
        check_lag(ctx, x, None, periods)
        check_lag(ctx, x, nulls, periods)
        check_lag(ctx, i, nulls, periods)


def test_lag_memory_spaces_and_odd_periods(ctx):
    rng = np.random.default_rng(17)
    n = 2 * T + 1003                                                      # n % 8 and n % 64 both non-zero
    x, nulls = rng.normal(0.0, 5.0, n), rng.random(n) < 0.2
    for col, release in passed_as(ctx, x, nulls):
        try:
            for periods in (1, 2, 3, -1, -2, 1001):                       # the lagged 16-byte access is misaligned at odd periods
                check_lag(ctx, x, nulls, periods, col=col, out_device=False)
                check_lag(ctx, x, nulls, periods, col=col, out_device=True)
        finally:
            if release:
                release()


def test_lag_null_operands_at_tile_edges_and_special_predecessors(ctx):
    n = 3 * T + 5
    x = np.arange(1, n + 1, dtype=np.float64)
    nulls = np.zeros(n, bool)
    nulls[[T - 1, T, 2 * T - 1, 2 * T + 1, 0, n - 1]] = True
    for periods in (1, 2, -1, T):
        check_lag(ctx, x, nulls, periods)
    y = np.array([1.0, 0.0, 2.0, -0.0, 3.0, np.inf, 4.0, np.nan, 5.0, -np.inf, np.inf, np.inf, 0.0, 0.0] * 300)
    for periods in (1, 2, 7):
        check_lag(ctx, y, None, periods)
    vals, mask, n_null = ctx.lag((np.array([-0.0, 5.0, 0.0, 1.0]), None, L.F64), 4, PCT_CHANGE, 1, out_device=False)
    assert same_bits(vals, np.array([NAN, NAN, -1.0, NAN])) and mask is None and n_null == 0
    vals, mask, n_null = ctx.lag((np.array([1.0, 2.0, 4.0]), None, L.F64), 3, SHIFT, 1, out_device=False)
    assert same_bits(vals, np.array([NAN, 1.0, 2.0])) and list(mask) == [0x01] and n_null == 1
    for x0, nl in ((y[:50], None), (np.arange(40), np.arange(40) % 7 == 3)):
        for op in LAG_OPS:
            for periods in (0, 1, 3, 50):
                want, gone = lag_loop(x0, nl, op, periods)                 # the line-for-line loop too
                vals, mask, n_null = ctx.lag((x0, None if nl is None else bits(nl), dtype_of(x0)), len(x0), op, periods, out_device=False)
                assert same_bits(vals, want) and n_null == int(gone.sum())


# ---- SUM -------------------------------------------------------------------------------------------------------------------
def test_sum_of_real_data_stays_inside_the_derived_bound(ctx, grid):
    rng = np.random.default_rng(23)
    for n in (10_007, (grid + 1) * T + 3):
        x = rng.normal(0.0, 1.0, n) * rng.lognormal(0.0, 2.0, n)
        nulls = rng.random(n) < 0.1
        check_cum(ctx, x, None, ops=[SUM])
        check_cum(ctx, x, nulls, ops=[SUM])
        dropped = cum_twin(x, None, SUM)[0]                                # the bound would catch a dropped tile carry
        dropped[T:] -= dropped[T - 1]
        with pytest.raises(AssertionError):
            compare_cells(SUM, dropped, cum_twin(x, None, SUM)[0], x, None, False)


def test_sum_nan_inf_and_negative_zero(ctx, grid):
    n = (grid + 1) * T + 3
    span = 2 * T                                                          # with grid + 1 tiles span 0 holds two: span 1 starts here
    base = np.random.default_rng(29).integers(-5, 6, n).astype(np.float64)
    for row in (T - 1, span, 0, span - 1, n - 1):                          # a tile's last row, a span's first row, row 0
        x = base.copy()
        x[row] = np.nan
        want = check_cum(ctx, x, ops=[SUM], exact=True)[SUM][0]
        assert np.isnan(want[row:]).all() and not np.isnan(want[:row]).any()
    x = base.copy()
    x[span - 1], x[span] = np.inf, -np.inf                                 # inf then -inf across a span edge
    want = check_cum(ctx, x, ops=[SUM], exact=True)[SUM][0]
    assert want[span - 1] == np.inf and np.isnan(want[span:]).all()
    x[span] = np.inf
    check_cum(ctx, x, ops=[SUM], exact=True)
    z = np.full(2 * T + 9, -0.0)
    vals, _, _ = ctx.cumulative((z, None, L.F64), len(z), SUM, out_device=False)
    assert same_bits(vals, np.zeros(len(z)))                               # the fold starts from +0.0
    nl = np.zeros(len(z), bool)
    nl[:T + 3] = True
    check_cum(ctx, z, nl, ops=[SUM], exact=True)


# ---- PROD ------------------------------------------------------------------------------------------------------------------
def test_prod_of_factors_near_one(ctx, grid):
    rng = np.random.default_rng(31)
    for n in (10_007, (grid + 1) * T + 3):
        x = np.exp(rng.normal(0.0, 0.1, n)) * rng.choice([-1.0, 1.0], n)
        ref = cum_twin(x, None, PROD)[0]
        assert np.all(np.isfinite(ref) & (np.abs(ref) >= TINY))            # every reference running product is normal
        check_cum(ctx, x, None, ops=[PROD])
        check_cum(ctx, x, rng.random(n) < 0.1, ops=[PROD])


def test_prod_range_case_in_a_lane_a_wave_and_a_tile(ctx):
    """[1e-200, 1e200, 1e200, 1e-200]: rows 1 .. 2 alone overflow, no running product does.  The pair shares a lane (rows 2l,
    2l + 1), a wave (rows 2l + 1, 2l + 2), a tile (across a wave's 512-row edge), and sits across a tile edge."""
    n = 3 * T
    for first in (2, 3, 511, T - 1, T + 127):
        x = np.ones(n)
        x[first - 1], x[first], x[first + 1], x[first + 2] = 1e-200, 1e200, 1e200, 1e-200
        want = check_cum(ctx, x, ops=[PROD])[PROD][0]
        assert np.all(np.isfinite(want)) and abs(want[first + 1] / 1e200 - 1.0) < 1e-15 and abs(want[-1] - 1.0) < 1e-15


def test_prod_zeros_and_infinities_at_tile_and_span_edges(ctx, grid):
    n = (grid + 1) * T + 3
    span = 2 * T
    rng = np.random.default_rng(37)
    base = np.exp(rng.normal(0.0, 0.05, n)) * rng.choice([-1.0, 1.0], n)
    for rows, cells in (((T - 1,), (0.0,)), ((T,), (-0.0,)), ((span,), (0.0,)), ((span - 1,), (np.inf,)), ((span,), (-np.inf,)),
                        ((T - 1, span), (0.0, np.inf)), ((T, span - 1), (np.inf, 0.0)), ((0,), (0.0,)), ((n - 1,), (np.inf,))):
        x = base.copy()
        x[list(rows)] = cells
        check_cum(ctx, x, ops=[PROD])


def test_prod_is_sticky_after_a_range_excursion(ctx, grid):
    n = (grid + 1) * T + 3
    span = 2 * T
    rng = np.random.default_rng(41)
    base = np.exp(rng.normal(0.0, 0.05, n)) * rng.choice([-1.0, 1.0], n)
    for at in (5, T - 2, span - 2, span + T + 1):
        for big, back in ((1e200, 1e-200), (1e-200, 1e200)):              # an overflow, an underflow to zero
            for later in (None, 0.0, np.inf):
                x = base.copy()
                x[at], x[at + 1] = big, big                               # the excursion is at row at + 1
                x[at + 3:at + 6] = back                                   # the sticky value survives the way back
                if later is not None:
                    x[at + 2 * T + 1] = later
                want = check_cum(ctx, x, ops=[PROD])[PROD][0]
                tail = want[at + 1:at + 2 * T + 1]
                assert np.all(np.isinf(tail)) if big > 1 else np.all(tail == 0.0)
                if later is not None:
                    assert np.isnan(want[-1]) == ((big > 1) == (later == 0.0))
    vals, _, _ = ctx.cumulative((np.array([1e200, 1e200, 1e-200, -1e-200, 0.0, 2.0]), None, L.F64), 6, PROD, out_device=False)
    assert same_bits(vals, np.array([1e200, np.inf, np.inf, -np.inf, NAN, NAN]))      # the values after the restart


# ---- MAX / MIN / COUNT -----------------------------------------------------------------------------------------------------
def test_extremes_and_counts(ctx, grid):
    n = (grid + 1) * T + 3
    span = 2 * T
    rng = np.random.default_rng(43)
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.1] = np.nan
    nulls = rng.random(n) < 0.1
    ops = [MAX, MIN, COUNT]
    check_cum(ctx, x, None, ops=ops)
    check_cum(ctx, x, nulls, ops=ops)
    check_cum(ctx, rng.integers(-2**62, 2**62, n), nulls, ops=ops)
    r = np.zeros(n)                                                        # a new extreme exactly at a tile's first and last row
    for k, row in enumerate((T - 1, T, 2 * T - 1, span, 3 * T, n - 1)):
        r[row] = k + 1.0
    check_cum(ctx, r, None, ops=[MAX])
    check_cum(ctx, -r, None, ops=[MIN])
    s = x.copy()                                                           # a span of only NaN, and NaN from row 0
    s[span:span + 3 * T] = np.nan
    s[:T + 1] = np.nan
    want = check_cum(ctx, s, None, ops=ops)
    assert np.all(want[MAX][0][:T + 1] == -np.inf) and np.all(want[MIN][0][:T + 1] == np.inf) and np.all(want[COUNT][0][:T + 1] == 0)
    z = np.where(rng.random(n) < 0.5, 0.0, -0.0)                           # signed zeros: -0.0 is below +0.0
    z[:T + 5] = -0.0
    want = check_cum(ctx, z, None, ops=[MAX, MIN])
    assert np.signbit(want[MAX][0][:T + 5]).all() and not np.signbit(want[MAX][0][-1])
    check_cum(ctx, -z, None, ops=[MAX, MIN])
    for x0, nl in ((s[:300], None), (np.arange(100) % 7 - 3, np.arange(100) % 5 == 0)):
        for op in CUM_OPS:                                                 # the line-for-line loop too
            want0, gone = cum_loop(x0, nl, op)
            vals, mask, n_null = ctx.cumulative((x0, None if nl is None else bits(nl), dtype_of(x0)), len(x0), op, out_device=False)
            assert same_bits(vals, want0) and n_null == int(gone.sum())


# ---- buffers, errors, limits ---------------------------------------------------------------------------------------------------
def test_outputs_with_guard_cells_and_stray_mask_bits(ctx):
    import torch
    rng = np.random.default_rng(47)
    n = 2 * T + 1003                                                      # n % 8 and n % 64 both non-zero
    nbytes = (n + 7) // 8
    x = rng.integers(-9, 10, n).astype(np.float64)
    nulls = rng.random(n) < 0.3
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8                                                      # stray bits past the last row are ignored
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    calls = [(lambda op=op, **kw: ctx.cumulative((dx, dm, L.F64), n, op, **kw), cum_twin(x, nulls, op)) for op in CUM_OPS]
    calls += [(lambda op=op, **kw: ctx.lag((dx, dm, L.F64), n, op, 3, **kw), lag_twin(x, nulls, op, 3)) for op in LAG_OPS]
    for call, (want, gone) in calls:
        out = np.full(n + 2, -7, want.dtype)                              # host outputs with guard cells and 64 guard bytes
        om = np.full(nbytes + 64, 0xAA, np.uint8)
        _, _, n_null = call(out=out[:n], out_mask=om)
        assert same_bits(out[:n], want) and (out[n:] == -7).all() and n_null == int(gone.sum())
        assert np.array_equal(om[:nbytes], bits(gone)) and (om[nbytes:] == 0xAA).all()
        dout = torch.full((n + 3,), -7, dtype=torch.int64 if want.dtype == np.int64 else torch.float64, device="cuda:0")
        dom = torch.full((nbytes + 1 + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        vals, m, n_null = call(out=dout[1:], out_mask=dom[1:])            # 8 / 1 bytes off
        assert same_bits(vals.cpu().numpy(), want) and (dout[0] == -7) and (dout[n + 1:] == -7).all()
        assert np.array_equal(dom[1:1 + nbytes].cpu().numpy(), bits(gone)) and (dom[0] == 0xAA) and (dom[1 + nbytes:] == 0xAA).all()
    lib, c = L.load(), L.Column()                                         # no output mask and no count asked of the ABI
    c.data, c.null_mask, c.dtype = x.ctypes.data, mask.ctypes.data, L.F64
    out = np.full(n, -7.0)
    assert lib.pandrs_hip_cumulative(ctx.h, L.MEM_HOST, C.byref(c), n, SUM, L.MEM_HOST, out.ctypes.data, None, None) == 0
    assert same_bits(out, cum_twin(x, nulls, SUM)[0])
    assert lib.pandrs_hip_lag(ctx.h, L.MEM_HOST, C.byref(c), n, DIFF, 1, L.MEM_HOST, out.ctypes.data, None, None) == 0
    assert same_bits(out, lag_twin(x, nulls, DIFF, 1)[0])


def test_timings(ctx):
    n = 3 * T
    x = np.ones(n)
    ctx.cumulative((x, None, L.F64), n, SUM)
    t = ctx.timings()
    assert t["n_partitions"] == 0 and t["algorithmic_bytes"] == n * 24 + n // 8
    ctx.lag((x, None, L.F64), n, DIFF, 1)
    assert ctx.timings()["algorithmic_bytes"] == n * 16 + n // 8


def test_bad_arguments(ctx):
    import pandrs_amd as pa
    import torch
    x = np.arange(16, dtype=np.float64)
    col = (x, None, L.F64)
    for bad in (-1, 5, 99):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.cumulative(col, 16, bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, bad
    for bad in (-1, 3, 99):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.lag(col, 16, bad, 1)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, bad
    for op in (DIFF, PCT_CHANGE):                                         # only SHIFT looks ahead
        for periods in (-1, -16, -(1 << 62)):
            with pytest.raises(pa.PandrsHipError) as e:
                ctx.lag(col, 16, op, periods)
            assert e.value.status == L.ERR_INVALID_ARGUMENT and "periods" in str(e.value)
    vals, mask, n_null = ctx.lag(col, 16, SHIFT, -(1 << 63))
    assert np.isnan(vals).all() and n_null == 16
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.cumulative((other, None, dt), 16, SUM)
        assert e.value.status == L.ERR_TYPE_MISMATCH
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.lag((other, None, dt), 16, SHIFT, 1)
        assert e.value.status == L.ERR_TYPE_MISMATCH
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out, om, cnt = np.full(16, -7.0), np.full(2, 0xAA, np.uint8), C.c_int64(-1)

    def cum(space=L.MEM_HOST, colp=C.byref(c), n=16, op=SUM, out_space=L.MEM_HOST, o=out.ctypes.data, m=om.ctypes.data):
        return lib.pandrs_hip_cumulative(ctx.h, space, colp, n, op, out_space, o, m, C.byref(cnt))

    def lag(space=L.MEM_HOST, colp=C.byref(c), n=16, op=DIFF, out_space=L.MEM_HOST, o=out.ctypes.data, m=om.ctypes.data):
        return lib.pandrs_hip_lag(ctx.h, space, colp, n, op, 1, out_space, o, m, C.byref(cnt))
    nodata = L.Column()
    nodata.dtype = L.F64
    for call in (cum, lag):
        assert call(colp=None) == L.ERR_INVALID_ARGUMENT
        assert call(o=None) == L.ERR_INVALID_ARGUMENT
        assert call(space=7) == L.ERR_INVALID_ARGUMENT and call(out_space=7) == L.ERR_INVALID_ARGUMENT
        assert call(n=1 << 32) == L.ERR_INVALID_ARGUMENT and call(n=-1) == L.ERR_INVALID_ARGUMENT
        assert call(colp=C.byref(nodata)) == L.ERR_INVALID_ARGUMENT
        assert call(n=0) == 0 and cnt.value == 0
        assert (out == -7.0).all() and (om == 0xAA).all()                 # no error above, and n_rows == 0, wrote anything
        assert call(o=x.ctypes.data) == L.ERR_INVALID_ARGUMENT and call(o=x.ctypes.data + 8 * 15) == L.ERR_INVALID_ARGUMENT
        assert "in place" in L.last_error()
        cnt.value = -1
    vals, mask, n_null = ctx.cumulative(col, 0, PROD)
    assert vals.shape == (0,) and mask is None and n_null == 0
    d = torch.arange(16, dtype=torch.float64, device="cuda:0")
    for call in (lambda o: ctx.cumulative((d, None, L.F64), 16, MAX, out=o), lambda o: ctx.lag((d, None, L.F64), 16, SHIFT, 0, out=o)):
        with pytest.raises(pa.PandrsHipError) as e:
            call(d)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        vals, _, _ = call(torch.empty_like(d))                            # a buffer of its own is fine
        assert torch.equal(vals, d)


CHILD = r"""
import ctypes as C, numpy as np, sys, torch
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
import pandrs_amd.frame as F
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=16 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
for call in (lambda x, n: c.cumulative((x, None, L.F64), n, L.CUM_SUM), lambda x, n: c.lag((x, None, L.F64), n, L.LAG_DIFF, 1)):
    try:
        call(np.zeros(4_000_000), 4_000_000)                    # 32 MB to stage
        raise SystemExit("no error under memory_limit (staging)")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
k = 3_000_000                                                   # a device column: the workspace is a few KB whatever n
x = torch.ones(k, dtype=torch.float64, device="cuda:0")
v, m, nulls = c.cumulative((x, None, L.F64), k, L.CUM_SUM)
assert nulls == 0 and torch.equal(v, torch.arange(1, k + 1, dtype=torch.float64, device="cuda:0"))
v, m, nulls = c.cumulative((x, None, L.F64), k, L.CUM_PROD)
assert bool((v == 1.0).all())
v, m, nulls = c.lag((x, None, L.F64), k, L.LAG_SHIFT, 1)
assert nulls == 1 and bool((v[1:] == 1.0).all())
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
for call in (lambda: c.cumulative((x, None, L.F64), 1000, L.CUM_MAX), lambda: c.lag((x, None, L.F64), 1000, L.LAG_SHIFT, 1)):
    try:
        call()
        raise SystemExit("no error below min_size_threshold")
    except pa.BelowThreshold as e:
        assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
for call in (lambda: df.cumsum("x"), lambda: df.diff("x", 1)):
    try:
        call()
        raise SystemExit("the frame did not raise below min_size_threshold")
    except pa.BelowThreshold:
        pass
y = np.ones(20_000)
v, m, nulls = c.cumulative((y, None, L.F64), 20_000, L.CUM_COUNT, out_device=False)
assert v[-1] == 20_000 and m is None and nulls == 0
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- mirrors ---------------------------------------------------------------------------------------------------------------
def test_frame_methods_against_the_twins(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(53)
    n = T + 301
    f, fn = rng.integers(-9, 10, n).astype(np.float64), rng.random(n) < 0.2
    f[rng.random(n) < 0.05] = np.nan
    i, inn = rng.integers(-3, 4, n), rng.random(n) < 0.3
    df = F.OptimizedDataFrame()
    df.add_column("i", F.Int64Column.with_nulls(i, inn))
    df.add_column("f", F.Float64Column.with_nulls(f, fn))
    df.add_column("g", F.Float64Column(np.arange(1.0, n + 1)))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    for name, data, nulls in (("i", i, inn), ("f", f, fn), ("g", np.arange(1.0, n + 1), None)):
        for op, call in ((SUM, df.cumsum), (PROD, df.cumprod), (MAX, df.cummax), (MIN, df.cummin), (COUNT, df.cumcount)):
            got = call(name)
            want, _ = cum_twin(data, nulls, op)
            assert isinstance(got, list) and all(type(v) is (int if op == COUNT else float) for v in got)
            compare_cells(op, np.array(got, want.dtype), want, data, nulls, op == SUM)
        for periods in (1, -2, n + 3):
            got = df.shift(name, periods)
            want, gone = lag_twin(data, nulls, SHIFT, periods)
            assert [v is None for v in got] == list(gone)
            assert same_bits(np.array([NAN if v is None else v for v in got]), want)
        for op, call in ((DIFF, df.diff), (PCT_CHANGE, df.pct_change)):
            for periods in (0, 1, 5):
                got = call(name, periods)
                assert all(type(v) is float for v in got) and same_bits(np.array(got), lag_twin(data, nulls, op, periods)[0])
    with pytest.raises(F.ColumnTypeMismatch):
        df.cumsum("b")
    with pytest.raises(F.ColumnNotFound):
        df.shift("nope", 1)
    with pytest.raises(F.InvalidValue):
        df.diff("f", -1)


def test_cpp_mirror_cumulative():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cumulative_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "cumulative_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "3 tests, 0 failed checks" in r.stdout


def test_one_call_above_2_pow_31_rows(ctx):
    """n = 2^31 + 12 345, x_i = i mod 3 built on the device: the prefix has a closed form and stays exact.  SUM, COUNT and DIFF
    with periods = 1, exact on the first and last 10^6 rows and on a strided sample."""
    import torch
    n = (1 << 31) + 12_345
    x = torch.empty(n, dtype=torch.float64, device="cuda:0")
    step = 1 << 28
    for s in range(0, n, step):
        e = min(n, s + step)
        x[s:e] = (torch.arange(s, e, dtype=torch.int64, device="cuda:0") % 3).to(torch.float64)
    m = 1_000_000
    rows = torch.cat([torch.arange(0, m, device="cuda:0"), torch.arange(m, n - m, 7_919_333, device="cuda:0"), torch.arange(n - m, n, device="cuda:0")])
    q, r = (rows + 1) // 3, (rows + 1) % 3
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")
    got, mask, n_null = ctx.cumulative((x, None, L.F64), n, SUM, out=out)
    assert got.numel() == n and mask is None and n_null == 0
    assert torch.equal(got[rows], (3 * q + (r == 2)).to(torch.float64))            # 0 + 1 + 2 per whole triple, then 0, then 1
    got, mask, n_null = ctx.lag((x, None, L.F64), n, DIFF, 1, out=out)
    assert mask is None and n_null == 0 and bool(torch.isnan(got[0]))
    assert torch.equal(got[rows[1:]], torch.where(rows[1:] % 3 == 0, -2.0, 1.0).to(torch.float64))
    del out, got
    cnt = torch.empty(n, dtype=torch.int64, device="cuda:0")
    got, mask, n_null = ctx.cumulative((x, None, L.F64), n, COUNT, out=cnt)
    assert mask is None and n_null == 0 and torch.equal(got[rows], rows + 1)
    del x, cnt, got
