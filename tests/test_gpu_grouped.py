"""pandrs_hip_grouped and GroupBy's cumsum / cummax / cummin / cumcount / row_number / shift / diff / pct_change against
tests/grouped_ref.py: for every group the ungrouped op over the group's rows in ascending row order.  MAX, MIN, COUNT,
ROW_NUMBER and the three lags are compared bit for bit (the uint64 view); SUM is bit for bit on integer-valued data and within
2 gamma_k sum|x| over the group's own prefix elsewhere (cumulative_ref.compare_cells per group).
The order of the groups in the sorted layout is the builder's business, so a test that claims an edge (a head at a tile's first
position, a carry across spans without a head, ...) reads the CSR back and asserts that the edge was reached."""
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
from tests.cumulative_ref import NAN, bits, same_bits  # noqa: E402
from tests.grouped_ref import (CUM_COUNT, CUM_MAX, CUM_MIN, CUM_SUM, G_DIFF, G_PCT_CHANGE, G_SHIFT, GROUPED_OPS, LAGS, ROW_NUMBER,  # noqa: E402
                               compare_grouped, group_ids, grouped_twin, grouped_twin_fast, layout_of)

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
T = int(re.search(r"grouped_tile_rows = (\d+)", HEADER).group(1))
PER_CU = int(re.search(r"grouped_blocks_per_cu = (\d+)", HEADER).group(1))


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


def group(ctx, keys, n):
    """pandrs_hip_groupby_indices over host keys -> (offsets, rows); the grouping stays in the context"""
    _, _, off, rows = ctx.groupby_indices(keys, n)
    off, rows = np.asarray(off), np.asarray(rows)
    assert off[0] == 0 and off[-1] == n and np.all(np.diff(off) > 0)
    return off, rows


def by_ids(ctx, ids):
    ids = np.asarray(ids, np.int64)
    return group(ctx, [(ids, None, L.I64)], len(ids))


def check(ctx, ids, x, nulls=None, ops=GROUPED_OPS, periods=(1,), exact=True, col=None, layout=None, **kw):
    """One column under `ops` against the twin, over the grouping the context retains (that of `ids`): the cells, the mask, the
    count, and `mask is None` exactly when no bit is set.  -> {(op, periods): (values, bits)} as the device gave them"""
    x = np.asarray(x)
    n = x.shape[0]
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype_of(x))
    layout = layout_of(ids) if layout is None else layout
    got = {}
    for op in ops:
        for p in (periods if op in LAGS else (0,)):
            if op in (G_DIFF, G_PCT_CHANGE) and p < 0:
                continue
            want, gone = grouped_twin_fast(ids, x, nulls, op, p, layout=layout)
            vals, mask, n_null = ctx.grouped(col, n, op, p, **kw)
            vals, mask, flags = host(vals, mask, n)
            compare_grouped(op, ids, vals, want, x, nulls, exact)
            assert n_null == int(gone.sum()) and (mask is None) == (n_null == 0), (op, p, n_null, int(gone.sum()))
            assert np.array_equal(flags, gone), (op, p)
            got[op, p] = (vals, flags)
    return got


def columns_of(n, seed):
    """F64 with NaN cells, I64, and each under a ~10 % null mask: small integers, so SUM is bit for bit"""
    rng = np.random.default_rng(seed)
    v = rng.choice(np.array([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 2.0, 4.0]), n)
    f = np.where(rng.random(n) < 0.1, np.nan, v)
    miss = rng.random(n) < 0.1
    return [(f, None), (f, miss), (v.astype(np.int64), None), (v.astype(np.int64), miss)]


# ---- sizes -------------------------------------------------------------------------------------------------------------------
SHAPES = {"1": lambda g: 1, "2": lambda g: 2, "63": lambda g: 63, "64": lambda g: 64, "65": lambda g: 65, "T-1": lambda g: T - 1,
          "T": lambda g: T, "T+1": lambda g: T + 1, "3T+1": lambda g: 3 * T + 1, "(G+1)T+3": lambda g: (g + 1) * T + 3}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sizes_ops_and_columns(ctx, grid, shape):
    n = SHAPES[shape](grid)
    ids = np.random.default_rng(n).integers(0, max(1, n // 7), n)
    by_ids(ctx, ids)
    layout = layout_of(ids)
    for x, nulls in columns_of(n, n):
        check(ctx, ids, x, nulls, periods=(1, -2), layout=layout)


# ---- group shapes ------------------------------------------------------------------------------------------------------------
def test_one_group_is_the_ungrouped_call(ctx):
    n = 3 * T + 1
    ids = np.zeros(n, np.int64)
    off, rows = by_ids(ctx, ids)
    assert list(off) == [0, n] and np.array_equal(rows, np.arange(n))
    cum = {CUM_SUM: L.CUM_SUM, CUM_MAX: L.CUM_MAX, CUM_MIN: L.CUM_MIN, CUM_COUNT: L.CUM_COUNT}
    lag = {G_SHIFT: L.LAG_SHIFT, G_DIFF: L.LAG_DIFF, G_PCT_CHANGE: L.LAG_PCT_CHANGE}
    for x, nulls in columns_of(n, 3):
        col = (x, None if nulls is None else bits(nulls), dtype_of(x))
        got = check(ctx, ids, x, nulls, periods=(0, 1, 5, -3))
        for (op, p), (vals, flags) in got.items():
            if op == ROW_NUMBER:
                assert np.array_equal(vals, np.arange(n))
                continue
            plain, mask, _ = ctx.cumulative(col, n, cum[op], out_device=False) if op in cum else ctx.lag(col, n, lag[op], p, out_device=False)
            assert same_bits(vals, plain) and np.array_equal(flags, host(plain, mask, n)[2]), (op, p)


def test_all_singletons(ctx):
    n = 3 * T + 1
    ids = np.random.default_rng(7).permutation(n)
    off, _ = by_ids(ctx, ids)
    assert np.array_equal(off, np.arange(n + 1))                           # a head at every position
    for x, nulls in columns_of(n, 5):
        check(ctx, ids, x, nulls, periods=(0, 1, -1))


@pytest.mark.parametrize("length", ["2", "63", "64", "65", "T", "T+1"])
def test_groups_of_one_fixed_length(ctx, length):
    """key = i mod m: every group has exactly L rows, strided across the whole row range; in the sorted layout the heads sit
    at the multiples of L and walk through every lane (L = 63, 65), every wave and, for L = T + 1, successive tile offsets."""
    ln = {"2": 2, "63": 63, "64": 64, "65": 65, "T": T, "T+1": T + 1}[length]
    m = {2: T + 37, 63: 130, 64: 70, 65: 130}.get(ln, 5)
    n = m * ln
    ids = np.arange(n) % m
    off, rows = by_ids(ctx, ids)
    assert np.all(np.diff(off) == ln) and np.all(np.diff(rows.reshape(m, ln), axis=1) == m)
    heads = off[:-1]
    if ln in (63, 65):
        assert set(heads % 64) == set(range(64))                           # a head in every lane
        assert len(set(heads % T // 512)) == 4                             # ... and in every wave of a tile
    if ln == 2:
        assert np.any(heads % T == T - 2) and np.any(heads % T == 0)
    if ln == 64:
        assert np.all(heads % 64 == 0)                                     # every load starts a group
    if ln == T:
        assert np.all(heads % T == 0)                                      # every head sits at a tile's first position
    if ln == T + 1:
        assert set(heads % T) == set(range(m))                             # the tile's first position, then one further per group
    for x, nulls in columns_of(n, ln):
        check(ctx, ids, x, nulls, periods=(0, 1, ln - 1, ln, ln + 1, n + 5, -1, -ln))


def test_one_long_group_among_singletons_carries_across_spans_without_a_head(ctx, grid):
    n = 12 * T + 5                                                         # 13 tiles, fewer than the grid: every span is one tile
    assert 13 < grid
    ids = np.arange(n)
    ids[3::2][:5 * T + 7] = -1                                             # one group of 5 T + 7 rows, every second row from row 3
    off, rows = by_ids(ctx, ids)
    g = int(np.argmax(np.diff(off)))
    a, b = int(off[g]), int(off[g + 1])
    assert b - a == 5 * T + 7 and np.all(np.diff(off)[np.arange(len(off) - 1) != g] == 1)
    whole = [t for t in range(13) if a < t * T and (t + 1) * T <= b]       # spans inside the group after its head: no head of their own
    assert len(whole) >= 2 and whole[-1] - whole[0] == len(whole) - 1
    rng = np.random.default_rng(11)
    v = rng.integers(-4, 5, n).astype(np.float64)
    nulls = rng.random(n) < 0.1
    check(ctx, ids, v, None, periods=(1, T, -2 * T))
    check(ctx, ids, np.where(rng.random(n) < 0.1, np.nan, v), nulls, periods=(1, 3 * T))
    real = rng.normal(0.0, 1.0, n) * rng.lognormal(0.0, 2.0, n)            # SUM inside the bound of the group's own prefix
    check(ctx, ids, real, nulls, ops=[CUM_SUM], exact=False)


def test_zipf_keys_with_null_keys(ctx):
    rng = np.random.default_rng(13)
    n = 3 * T + 1
    key = np.minimum(rng.zipf(1.3, n), 500).astype(np.int64)
    knull = rng.random(n) < 0.05
    ids = group_ids([key], [knull])
    off, rows = group(ctx, [(key, bits(knull), L.I64)], n)
    assert len(off) - 1 == len(np.unique(ids)) and np.diff(off).max() > T // 2
    null_rows = np.flatnonzero(knull)
    g = np.searchsorted(off, np.flatnonzero(rows == null_rows[0])[0], side="right") - 1
    assert np.array_equal(rows[off[g]:off[g + 1]], null_rows)              # the NULL keys are one group of their own
    for x, nulls in columns_of(n, 17):
        check(ctx, ids, x, nulls, periods=(1, 2, -1))
    real = rng.normal(0.0, 1.0, n) * rng.lognormal(0.0, 2.0, n)
    check(ctx, ids, real, rng.random(n) < 0.1, ops=[CUM_SUM, CUM_MAX, CUM_MIN], exact=False)
    assert same_bits(grouped_twin(ids, real, None, CUM_SUM)[0],            # the per-group twin itself, once
                     grouped_twin_fast(ids, real, None, CUM_SUM)[0])


def test_two_keys_i64_and_string_codes(ctx):
    rng = np.random.default_rng(19)
    n = 2 * T + 77
    k0, k1 = rng.integers(-3, 4, n), rng.integers(0, 6, n).astype(np.uint32)
    n0, n1 = rng.random(n) < 0.05, rng.random(n) < 0.05
    ids = group_ids([k0, k1], [n0, n1])
    off, _ = group(ctx, [(k0, bits(n0), L.I64), (k1, bits(n1), L.U32CODE)], n)
    assert len(off) - 1 == len(np.unique(ids))
    for x, nulls in columns_of(n, 23):
        check(ctx, ids, x, nulls, periods=(1, -1, 4))


# ---- accuracy: a group's prefix is its own ---------------------------------------------------------------------------------------
def test_no_cancellation_across_groups(ctx):
    """A group of cells near 1e300 sits directly in front of a group of cells near 1e-300 in the sorted layout.  A prefix taken
    as "global prefix minus the prefix at the group's start" gives the small group 0, inf or NaN; its own fold meets the bound."""
    rng = np.random.default_rng(29)
    big, small = T + 5, T + 9
    n = big + small
    for keys in ((1, 2), (2, 1), (1, 3), (3, 1), (5, 4), (4, 5)):
        ids = np.where(rng.permutation(n) < big, keys[0], keys[1])
        off, rows = by_ids(ctx, ids)
        if ids[rows[0]] == keys[0]:
            break
    assert ids[rows[0]] == keys[0] and ids[rows[off[1]]] == keys[1] and off[1] == big      # the big group, then the small one
    x = np.where(ids == keys[0], 1e300, 1e-300) * (1.0 + rng.random(n))
    got = check(ctx, ids, x, None, ops=[CUM_SUM], exact=False)[CUM_SUM, 0][0]
    tail = got[ids == keys[1]]
    assert np.all(np.isfinite(tail)) and np.all(tail > 0) and np.all(np.diff(tail) > 0) and tail[-1] < 2e-300 * small
    nulls = rng.random(n) < 0.1
    check(ctx, ids, x, nulls, ops=[CUM_SUM], exact=False)


# ---- group starts, NaN ------------------------------------------------------------------------------------------------------------
def test_group_starts_and_nan_poisoning(ctx):
    rng = np.random.default_rng(31)
    m, ln = 9, T // 2 + 3
    n = m * ln
    ids = np.arange(n) % m
    off, rows = by_ids(ctx, ids)
    x = rng.integers(-5, 6, n).astype(np.float64)
    x[ids == 4] = -0.0                                                     # a group of only -0.0 gives +0.0
    got = check(ctx, ids, x, None, ops=[CUM_SUM])[CUM_SUM, 0][0]
    assert same_bits(got[ids == 4], np.zeros(ln))
    first = rows[off[:-1]]                                                 # every group's first row holds NaN
    y = x.copy()
    y[first] = np.nan
    got = check(ctx, ids, y, None, ops=[CUM_MAX, CUM_MIN, CUM_COUNT])
    assert np.all(got[CUM_MAX, 0][0][first] == -np.inf) and np.all(got[CUM_MIN, 0][0][first] == np.inf) and np.all(got[CUM_COUNT, 0][0][first] == 0)
    z = x.copy()                                                           # a NaN poisons only its own group's later sums
    mid = rows[off[2] + ln // 2]
    z[mid] = np.nan
    got = check(ctx, ids, z, None, ops=[CUM_SUM])[CUM_SUM, 0][0]
    own = rows[off[2]:off[3]]
    assert np.isnan(got[own[ln // 2:]]).all() and not np.isnan(got[own[:ln // 2]]).any() and not np.isnan(np.delete(got, own)).any()
    w = x.copy()
    w[mid], w[rows[off[5] + 3]] = np.inf, -np.inf                          # infinities stay in their groups too
    got = check(ctx, ids, w, None, ops=[CUM_SUM])[CUM_SUM, 0][0]
    assert np.isfinite(np.delete(got, np.concatenate([own, rows[off[5]:off[6]]]))).all()


# ---- lag --------------------------------------------------------------------------------------------------------------------------
def test_lag_periods_null_operands_at_group_edges_and_zero_predecessors(ctx):
    m, ln = 67, 65
    n = m * ln
    ids = np.arange(n) % m
    off, rows = by_ids(ctx, ids)
    rng = np.random.default_rng(37)
    x = rng.normal(0.0, 10.0, n)
    x[rng.random(n) < 0.1] = 0.0
    x[rng.random(n) < 0.05] = -0.0                                         # prev == 0.0 holds for -0.0 too
    x[rng.random(n) < 0.02] = np.nan                                       # a NaN that SHIFT copies arrives canonical
    x[np.isnan(x)] = np.uint64(0x7FF8000000000123).view(np.float64)
    nulls = np.zeros(n, bool)
    nulls[rows[off[:-1]][::2]] = True                                      # null operands at the groups' first and last rows
    nulls[rows[off[1:] - 1][::3]] = True
    nulls |= rng.random(n) < 0.05
    i = rng.integers(-1000, 1000, n)
    layout = layout_of(ids)
    periods = (0, 1, ln - 1, ln, ln + 1, n + 5, -1, -(ln - 1), -ln, -(n + 5))
    lags = [G_SHIFT, G_DIFF, G_PCT_CHANGE]
    check(ctx, ids, x, None, ops=lags, periods=periods, layout=layout)
    got = check(ctx, ids, x, nulls, ops=lags, periods=periods, layout=layout)
    check(ctx, ids, i, nulls, ops=lags, periods=periods, layout=layout)
    prev, missing = grouped_twin_fast(ids, x, nulls, G_SHIFT, 1, layout=layout)
    zero_prev = np.flatnonzero((prev == 0.0) & ~missing & ~nulls)          # prev = +-0.0 is a NaN value, not a missing row
    assert zero_prev.size > 100 and np.isnan(got[G_PCT_CHANGE, 1][0][zero_prev]).all() and not got[G_PCT_CHANGE, 1][1][zero_prev].any()
    vals, mask, n_null = ctx.grouped((x, None, L.F64), n, G_SHIFT, -(1 << 63), out_device=False)
    assert same_bits(vals, np.full(n, NAN)) and n_null == n


# ---- buffers, memory spaces ---------------------------------------------------------------------------------------------------------
def test_outputs_with_guard_cells_mask_offsets_and_stray_mask_bits(ctx):
    import torch
    rng = np.random.default_rng(47)
    n = 2 * T + 1003                                                      # n % 8 and n % 64 both non-zero
    nbytes = (n + 7) // 8
    ids = rng.integers(0, 40, n)
    by_ids(ctx, ids)
    x = rng.integers(-9, 10, n).astype(np.float64)
    nulls = rng.random(n) < 0.3
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8                                                      # stray bits past the last row are ignored
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    layout = layout_of(ids)
    for k, op in enumerate(GROUPED_OPS):
        want, gone = grouped_twin_fast(ids, x, nulls, op, 3, layout=layout)
        col = None if op == ROW_NUMBER else (dx, dm, L.F64)
        out = np.full(n + 2, -7, want.dtype)                              # host outputs with guard cells and 64 guard bytes
        om = np.full(nbytes + 64, 0xAA, np.uint8)
        _, _, n_null = ctx.grouped(col, n, op, 3, out=out[:n], out_mask=om)
        assert same_bits(out[:n], want) and (out[n:] == -7).all() and n_null == int(gone.sum())
        assert np.array_equal(om[:nbytes], bits(gone)) and (om[nbytes:] == 0xAA).all()
        shift = 1 + k % 7                                                 # the mask at byte offsets 1 .. 7, the cells 8 bytes off
        dout = torch.full((n + 3,), -7, dtype=torch.int64 if want.dtype == np.int64 else torch.float64, device="cuda:0")
        dom = torch.full((nbytes + shift + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        assert dom.data_ptr() % 8 == 0
        vals, m, n_null = ctx.grouped(col, n, op, 3, out=dout[1:], out_mask=dom[shift:])
        assert same_bits(vals.cpu().numpy(), want) and (dout[0] == -7) and (dout[n + 1:] == -7).all()
        assert np.array_equal(dom[shift:shift + nbytes].cpu().numpy(), bits(gone))
        assert (dom[:shift] == 0xAA).all() and (dom[shift + nbytes:] == 0xAA).all()
    lib, c = L.load(), L.Column()                                         # no output mask and no count asked of the ABI
    c.data, c.null_mask, c.dtype = x.ctypes.data, mask.ctypes.data, L.F64
    out = np.full(n, -7.0)
    for op, p in ((CUM_SUM, 0), (G_DIFF, 1)):
        assert lib.pandrs_hip_grouped(ctx.h, L.MEM_HOST, C.byref(c), n, op, p, L.MEM_HOST, out.ctypes.data, None, None) == 0
        assert same_bits(out, grouped_twin_fast(ids, x, nulls, op, p, layout=layout)[0])
    t = ctx.timings()
    assert t["n_partitions"] == 0 and t["algorithmic_bytes"] > n * 16 and "aggregate" in t["phase_ms"]
    numbered, _, _ = ctx.grouped((x, mask, L.F64), n, ROW_NUMBER, out_device=False)      # a column, when given, is not read
    assert np.array_equal(numbered, grouped_twin_fast(ids, x, None, ROW_NUMBER, layout=layout)[0])


def test_memory_spaces(ctx):
    """The column on the host, on the device, resident, and on the device 8 bytes off a 16-byte boundary with its mask at an odd
    byte offset; outputs in both spaces"""
    import torch
    rng = np.random.default_rng(53)
    n = 2 * T + 1003
    ids = rng.integers(0, 300, n)
    by_ids(ctx, ids)
    layout = layout_of(ids)
    for x, nulls in columns_of(n, 59)[1::2]:
        dt, mask = dtype_of(x), bits(nulls)
        dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
        pad = torch.empty(n + 1, dtype=dx.dtype, device="cuda:0")
        pad[1:] = dx
        padm = torch.empty(mask.shape[0] + 3, dtype=torch.uint8, device="cuda:0")
        padm[3:] = dm
        res = ctx.upload_column(x, mask, dt)
        try:
            for k, col in enumerate(((x, mask, dt), (dx, dm, dt), res, (pad[1:], padm[3:], dt))):
                check(ctx, ids, x, nulls, periods=(2,), col=col, layout=layout, out_device=bool(k % 2))
                check(ctx, ids, x, nulls, ops=[CUM_MAX, G_SHIFT], periods=(-1,), col=col, layout=layout, out_device=not k % 2)
        finally:
            res.release()


# ---- the retained grouping ------------------------------------------------------------------------------------------------------------
def test_one_grouping_serves_many_calls_and_stays_intact(ctx):
    import pandrs_amd as pa
    rng = np.random.default_rng(61)
    n = 3 * T + 11
    ids = rng.integers(0, 50, n)
    x, y = rng.integers(-9, 10, n).astype(np.float64), rng.integers(-9, 10, n)
    off, rows = by_ids(ctx, ids)
    token = ctx.grouping_token
    a = [ctx.grouped((x, None, L.F64), n, CUM_SUM, out_device=False)[0], ctx.grouped((y, None, L.I64), n, G_DIFF, 2, out_device=False)[0]]
    assert ctx.grouping_token == token                                     # a grouped call is not a regrouping
    cells = np.empty((1, len(off) - 1), np.uint64)
    knull = np.empty((1, len(off) - 1), np.uint8)
    off2, rows2 = np.empty_like(off), np.empty_like(rows)
    pk, pn = (C.c_void_p * 1)(cells.ctypes.data), (C.c_void_p * 1)(knull.ctypes.data)
    assert L.load().pandrs_hip_groupby_indices_fetch(ctx.h, L.MEM_HOST, pk, pn, off2.ctypes.data, rows2.ctypes.data) == 0
    assert np.array_equal(off2, off) and np.array_equal(rows2, rows)       # the calls left the retained CSR as it was
    by_ids(ctx, ids)
    b0 = ctx.grouped((x, None, L.F64), n, CUM_SUM, out_device=False)[0]
    by_ids(ctx, ids)
    b1 = ctx.grouped((y, None, L.I64), n, G_DIFF, 2, out_device=False)[0]
    assert ctx.grouping_token == token + 2 and same_bits(a[0], b0) and same_bits(a[1], b1)
    try:                                                                   # ... also with every workspace block poisoned
        pa.Context.poison_workspace(0xA5)
        off, rows = by_ids(ctx, ids)
        for op in GROUPED_OPS:
            ctx.grouped((x, None, L.F64), n, op, 1, out_device=False)
        assert L.load().pandrs_hip_groupby_indices_fetch(ctx.h, L.MEM_HOST, pk, pn, off2.ctypes.data, rows2.ctypes.data) == 0
        assert np.array_equal(off2, off) and np.array_equal(rows2, rows)
    finally:
        pa.Context.poison_workspace(None)


def test_results_do_not_depend_on_stale_workspace(ctx, grid):
    """Every op under Context.poison_workspace(0xA5) gives what it gives without: no kernel reads scratch it did not write."""
    import pandrs_amd as pa
    rng = np.random.default_rng(67)
    for n in (T + 1, 5 * T + 77):
        ids = rng.integers(0, max(2, n // 9), n)
        x = np.where(rng.random(n) < 0.1, np.nan, rng.normal(0.0, 3.0, n))
        col = (x, bits(rng.random(n) < 0.1), L.F64)
        by_ids(ctx, ids)
        plain = [ctx.grouped(col, n, op, 2, out_device=False) for op in GROUPED_OPS]
        try:
            pa.Context.poison_workspace(0xA5)                              # (the same grouping: a SUM's rounding follows the layout)
            for op, (vals, mask, n_null) in zip(GROUPED_OPS, plain):
                v, m, k = ctx.grouped(col, n, op, 2, out_device=False)
                assert same_bits(v, vals) and k == n_null and ((m is None and mask is None) or np.array_equal(m, mask)), op
        finally:
            pa.Context.poison_workspace(None)


# ---- errors, limits ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import pandrs_amd as pa
    import torch
    x = np.arange(16, dtype=np.float64)
    col = (x, None, L.F64)
    fresh = pa.Context(0)
    try:
        with pytest.raises(pa.PandrsHipError) as e:
            fresh.grouped(col, 16, CUM_SUM)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "no grouping retained" in str(e.value)
    finally:
        fresh.close()
    by_ids(ctx, np.arange(32) % 3)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.grouped(col, 16, CUM_SUM)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "the retained grouping has 32 rows" in str(e.value)
    by_ids(ctx, np.arange(16) % 3)
    for bad in (-1, 8, 99):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.grouped(col, 16, bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "pandrs_hip_grouped_op" in str(e.value), bad
    for op in (G_DIFF, G_PCT_CHANGE):                                      # only SHIFT looks ahead
        for periods in (-1, -16, -(1 << 62)):
            with pytest.raises(pa.PandrsHipError) as e:
                ctx.grouped(col, 16, op, periods)
            assert e.value.status == L.ERR_INVALID_ARGUMENT and "periods" in str(e.value)
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        for op in (CUM_SUM, G_SHIFT):
            with pytest.raises(pa.ColumnTypeMismatch) as e:
                ctx.grouped((other, None, dt), 16, op, 1)
            assert e.value.status == L.ERR_TYPE_MISMATCH
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out, om, cnt = np.full(16, -7.0), np.full(2, 0xAA, np.uint8), C.c_int64(-1)

    def call(space=L.MEM_HOST, colp=C.byref(c), n=16, op=CUM_SUM, out_space=L.MEM_HOST, o=out.ctypes.data, m=om.ctypes.data):
        return lib.pandrs_hip_grouped(ctx.h, space, colp, n, op, 1, out_space, o, m, C.byref(cnt))
    nodata = L.Column()
    nodata.dtype = L.F64
    assert call(colp=None) == L.ERR_INVALID_ARGUMENT
    assert call(o=None) == L.ERR_INVALID_ARGUMENT
    assert call(space=7) == L.ERR_INVALID_ARGUMENT and call(out_space=7) == L.ERR_INVALID_ARGUMENT
    assert call(n=-1) == L.ERR_INVALID_ARGUMENT and call(colp=C.byref(nodata)) == L.ERR_INVALID_ARGUMENT
    assert call(o=x.ctypes.data) == L.ERR_INVALID_ARGUMENT and "in place" in L.last_error()
    assert call(o=x.ctypes.data + 8 * 15, op=G_SHIFT) == L.ERR_INVALID_ARGUMENT and "in place" in L.last_error()
    assert (out == -7.0).all() and (om == 0xAA).all()                      # no error above wrote a cell or a mask byte
    assert call(colp=None, op=ROW_NUMBER) == 0 and cnt.value == 0 and (om == 0).all()      # ROW_NUMBER reads no column
    assert np.array_equal(out.view(np.int64), np.arange(16) // 3)
    d = torch.arange(16, dtype=torch.float64, device="cuda:0")
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.grouped((d, None, L.F64), 16, CUM_MAX, out=d)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    ctx.groupby_indices_compute([(np.zeros(0, np.int64), None, L.I64)], 0)  # an empty grouping: an empty call is fine
    cnt.value = -1
    assert call(n=0) == 0 and cnt.value == 0
    vals, mask, n_null = ctx.grouped((np.zeros(0), None, L.F64), 0, CUM_SUM)
    assert vals.shape == (0,) and mask is None and n_null == 0


CHILD = r"""
import ctypes as C, numpy as np, sys, torch
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
import pandrs_amd.frame as F
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=0, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
n = 4_000_000
keys = (torch.arange(n, dtype=torch.int64, device="cuda:0") %% 1000)
c.groupby_indices_compute([(keys, None, L.I64)], n)
x = torch.ones(n, dtype=torch.float64, device="cuda:0")
v, m, nulls = c.grouped((x, None, L.F64), n, L.GROUPED_CUM_SUM)
assert nulls == 0 and torch.equal(v, (torch.arange(n, device="cuda:0") // 1000 + 1).to(torch.float64))
cfg.memory_limit = 16 << 20                                     # from here on no arena may grow past 16 MB
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
other = pa.Context(0)
for op in (L.GROUPED_CUM_SUM, L.GROUPED_DIFF):
    try:
        c.grouped((np.zeros(n), None, L.F64), n, op, 1)         # 32 MB to stage
        raise SystemExit("no error under memory_limit (staging)")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
v, m, nulls = c.grouped((x, None, L.F64), n, L.GROUPED_ROW_NUMBER)     # the grouping survived the refused calls
assert torch.equal(v, torch.arange(n, device="cuda:0") // 1000)
other.close()
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
try:
    c.grouped((x, None, L.F64), 1000, L.GROUPED_CUM_MAX)
    raise SystemExit("no error below min_size_threshold")
except pa.BelowThreshold as e:
    assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("k", F.Int64Column(np.arange(1000) %% 7))
df.add_column("x", F.Float64Column(x))
for call in (lambda: df.group_by(["k"]).cumsum("x"), lambda: df.group_by(["k"]).row_number()):
    try:
        call()
        raise SystemExit("the frame did not raise below min_size_threshold")
    except pa.BelowThreshold:
        pass
k = np.arange(20_000) %% 100
c.groupby_indices_compute([(k, None, L.I64)], 20_000)
v, m, nulls = c.grouped((np.ones(20_000), None, L.F64), 20_000, L.GROUPED_CUM_COUNT, out_device=False)
assert np.array_equal(v, np.arange(20_000) // 100 + 1) and m is None and nulls == 0
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- mirrors -----------------------------------------------------------------------------------------------------------------------
def test_frame_methods_against_the_twins(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(71)
    n = T + 301
    f, fn = rng.integers(-9, 10, n).astype(np.float64), rng.random(n) < 0.2
    f[rng.random(n) < 0.05] = np.nan
    i, inn = rng.integers(-3, 4, n), rng.random(n) < 0.3
    k, kn = rng.integers(0, 9, n), rng.random(n) < 0.05
    names = [["a", "b", "c"][v] for v in rng.integers(0, 3, n)]
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column.with_nulls(k, kn))
    df.add_column("s", F.StringColumn(names))
    df.add_column("i", F.Int64Column.with_nulls(i, inn))
    df.add_column("f", F.Float64Column.with_nulls(f, fn))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    for by, ids in ((["k"], group_ids([k], [kn])), (["s", "k"], group_ids([np.unique(names, return_inverse=True)[1], k], [None, kn]))):
        g = df.group_by(by)
        layout = layout_of(ids)
        token = None
        for name, data, nulls in (("i", i, inn), ("f", f, fn)):
            for op, call in ((CUM_SUM, g.cumsum), (CUM_MAX, g.cummax), (CUM_MIN, g.cummin), (CUM_COUNT, g.cumcount)):
                got = call(name)
                want, _ = grouped_twin_fast(ids, data, nulls, op, layout=layout)
                assert isinstance(got, list) and all(type(v) is (int if op == CUM_COUNT else float) for v in got)
                assert same_bits(np.array(got, want.dtype), want)
                token = F.get_context().grouping_token if token is None else token
            for periods in (1, -2, n + 3):
                got = g.shift(name, periods)
                want, gone = grouped_twin_fast(ids, data, nulls, G_SHIFT, periods, layout=layout)
                assert [v is None for v in got] == list(gone)
                assert same_bits(np.array([NAN if v is None else v for v in got]), want)
            for op, call in ((G_DIFF, g.diff), (G_PCT_CHANGE, g.pct_change)):
                for periods in (0, 1, 5):
                    got = call(name, periods)
                    assert all(type(v) is float for v in got) and same_bits(np.array(got), grouped_twin_fast(ids, data, nulls, op, periods, layout=layout)[0])
        got = g.row_number()
        assert all(type(v) is int for v in got) and np.array_equal(got, grouped_twin_fast(ids, f, None, ROW_NUMBER, layout=layout)[0])
        assert F.get_context().grouping_token == token                     # one grouping served every method
        assert len(g.groups) == len(np.unique(ids))                        # ... the closures' row map regroups
        assert g.cumcount("f") == [int(v) for v in grouped_twin_fast(ids, f, fn, CUM_COUNT, layout=layout)[0]]
        assert F.get_context().grouping_token == token + 2                 # ... and so does the next method, once
        with pytest.raises(F.ColumnTypeMismatch):
            g.cumsum("b")
        with pytest.raises(F.ColumnNotFound):
            g.shift("nope", 1)
        with pytest.raises(F.InvalidValue):
            g.diff("f", -1)


def test_cpp_mirror_grouped():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grouped_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "grouped_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "3 tests, 0 failed checks" in r.stdout
