"""pandrs_hip_distinct / pandrs_hip_distinct_fetch and the mirrors' value_counts / unique / nunique / mode / is_unique (reference
src/dataframe/pandas_compat/functions.rs:343-384, :775-788, :1709-1753, :4120-4139, :4226-4259) against tests/distinct_ref.py's
twin of the contract.  Values are bit patterns and counts are integers: every comparison in this file is exact, no tolerance
anywhere.  Wherever the direct (LDS table) path is possible a case runs under "distinct_path" 1 and 2 and both must give the
twin's list, hence the same list."""
import math
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests import distinct_ref as R  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"distinct_tile_rows = (\d+)", HEADER).group(1))
M = int(re.search(r"distinct_direct_max_cells = (\d+)", HEADER).group(1))
BLOCKS_PER_CU = int(re.search(r"distinct_blocks_per_cu = (\d+)", HEADER).group(1))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
assert (L.I64, L.F64, L.U32CODE, L.BOOLBITS) == (R.I64, R.F64, R.U32CODE, R.BOOLBITS)
assert (L.DISTINCT_BY_VALUE, L.DISTINCT_BY_COUNT) == (R.BY_VALUE, R.BY_COUNT)
assert (L.DISTINCT_NUMBER, L.DISTINCT_NAN, L.DISTINCT_NULL) == (R.NUMBER, R.NAN, R.NULL)


def f64(bits_):
    return struct.unpack("<d", struct.pack("<Q", bits_))[0]


NAN_A, NAN_B, NAN_ONES = f64(0x7FF8000000000000), f64(0xFFF8000000000123), f64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.set_option("distinct_path", 0)
    c.close()


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def host(b):
    return b if isinstance(b, np.ndarray) else b.cpu().numpy()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def dtype_of(x):
    return {np.dtype(np.int64): L.I64, np.dtype(np.float64): L.F64, np.dtype(np.uint32): L.U32CODE}[np.asarray(x).dtype]


def check(ctx, x, nulls=None, dtype=None, rank=None, n_rows=None, col=None, out_device=False, orders=(0, 1), direct=None):
    """The list through both options against the twin, the info, the invariants, the path taken.  `col` overrides how the
    column is passed; `direct`: whether the direct path must (True) / cannot (False) be possible (None: the twin's rule)."""
    x = np.asarray(x)
    dtype = dtype_of(x) if dtype is None else dtype
    n = n_rows if n_rows is not None else x.shape[0]
    mask = None if nulls is None else bits(nulls)
    col = col if col is not None else (x, mask, dtype)
    possible = R.direct_possible(x, dtype, nulls, n, M)
    if direct is not None:
        assert possible == direct
    out = None
    try:
        for order in orders:
            wv, wf, wk, winfo = R.distinct(x, dtype, nulls, order, rank, n)
            for option in (1, 2):
                ctx.set_option("distinct_path", option)
                v, f, k, info = ctx.distinct(col, n, order, code_rank=rank, out_device=out_device)
                v, f, k = host(v).view(np.uint64), host(f), host(k)
                where = (n, order, option, info)
                assert v.dtype == np.uint64 and f.dtype == np.uint8 and k.dtype == np.int64, where
                assert np.array_equal(f, wf) and np.array_equal(v, wv) and np.array_equal(k, wk), (where, v[:6], wv[:6], k[:6], wk[:6], f[:6], wf[:6])
                for name, want in winfo.items():
                    assert info[name] == want, (name, where, winfo)
                # the invariants of every case
                assert int(k.sum()) == n and info["n_valid"] + info["nan_count"] + info["null_count"] == n, where
                assert len(set(zip(v.tolist(), f.tolist()))) == v.shape[0] == info["n_entries"], where
                if n:
                    assert info["path"] == (1 if possible and option == 1 else 2), where
                    assert ctx.timings()["n_partitions"] == info["path"], where
                else:
                    assert info["path"] == 0 and info["n_entries"] == 0
                out = (v, f, k, info)
    finally:
        ctx.set_option("distinct_path", 0)
    return out


# ---- row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, rng.integers(-20, 21, n), direct=True)
    x = rng.integers(-20, 21, n).astype(np.float64)
    x[rng.random(n) < 0.1] = np.nan
    check(ctx, x, rng.random(n) < 0.1, direct=True)
    check(ctx, rng.normal(0.0, 1.0, n), rng.random(n) < 0.1, direct=n == 0 or None)


def test_more_workgroups_than_tiles_and_more_tiles_than_workgroups(ctx):
    import torch
    grid = BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2)
    assert 3 * TILE + 1 < grid * TILE                                         # fewer tiles than the full grid: the grid shrinks to them
    n = (grid + 3) * TILE + 5                                                 # some workgroups take two tiles, one a partial tile
    check(ctx, rng.integers(0, 300, n), direct=True)
    check(ctx, rng.integers(0, 300, n).astype(np.float64), rng.random(n) < 0.05, direct=True)


@pytest.mark.parametrize("values", [100, None])
def test_four_million_rows_past_the_small_call_path(ctx, values):
    n = 4_000_000
    rng = np.random.default_rng(3)
    x = rng.integers(0, values, n) if values else rng.permutation(n).astype(np.int64) * 3 - n
    got = check(ctx, x, orders=(1,), direct=values is not None)
    assert got[3]["n_entries"] == (values or n)


def test_four_million_f64_rows_with_nan_payloads_through_the_engine(ctx):
    """The large engine paths with an F64 key: several NaN payloads must come back as the one canonical NaN entry."""
    n = 4_000_000
    rng = np.random.default_rng(31)
    x = rng.integers(0, 300_000, n).astype(np.float64) * 0.25
    x[rng.random(n) < 0.01] = NAN_B
    x[rng.random(n) < 0.01] = NAN_ONES
    x[rng.random(n) < 0.01] = NAN_A
    x[5], x[6] = -0.0, 0.0
    got = check(ctx, x, orders=(0,), direct=False)
    assert (got[1] == L.DISTINCT_NAN).sum() == 1 and got[1][-1] == L.DISTINCT_NAN and got[0][-1] == R.CANON_NAN
    assert got[3]["path"] == 2 and got[3]["nan_count"] > 100_000


def test_zero_rows_after_a_small_groupby_is_an_empty_retained_list(ctx):
    """A small groupby leaves its timings unresolved; a 0-row distinct behind it is still OK, and its empty list fetches."""
    import pandrs_amd as pa
    rng = np.random.default_rng(32)
    n = 10_000
    keys, vals = rng.integers(0, 50, n), rng.normal(0, 1, n)
    empty = (np.empty(0, np.float64), None, L.F64)
    for read_timings in (False, True):
        assert ctx.groupby_compute([(keys, None, L.I64)], n, [(vals, None, L.F64)], [(0, L.SUM)]) == 50
        v, f, k, info = ctx.distinct(empty, 0, L.DISTINCT_BY_VALUE)
        assert v.size == f.size == k.size == 0 and all(info[q] == 0 for q in info)
        if read_timings:
            ctx.timings()
        assert [a.size for a in ctx.distinct_fetch(0)] == [0, 0, 0]
        assert [a.numel() for a in ctx.distinct_fetch(0, out_device=True)] == [0, 0, 0]
    # ... and the other way round: the list of a real call is gone after a small groupby, read or not
    v, f, k, info = ctx.distinct((keys, None, L.I64), n, L.DISTINCT_BY_COUNT)
    assert info["n_entries"] == 50 and [a.size for a in ctx.distinct_fetch(50)] == [50, 50, 50]
    ctx.groupby_compute([(keys, None, L.I64)], n, [(vals, None, L.F64)], [(0, L.SUM)])
    for read_timings in (False, True):
        if read_timings:
            ctx.timings()
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.distinct_fetch(50)
        assert e.value.status == L.ERR_INVALID_ARGUMENT


# ---- table sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [1, 2, 64, M - 1, M, M + 1])
def test_table_sizes(ctx, cells):
    rng = np.random.default_rng(cells)
    n = 3 * TILE + 17
    base = -12345
    x = base + rng.integers(0, cells, n)
    x[:2] = [base, base + cells - 1]                                          # the table's first and last cell are in use
    got = check(ctx, x, direct=cells <= M)
    if cells == M + 1:
        assert got[3]["path"] == 2
    check(ctx, x.astype(np.float64), direct=cells <= M)
    if cells <= M:
        codes = (x - base).astype(np.uint32)
        check(ctx, codes, direct=True)
    # every cell of the table hit exactly once
    once = base + rng.permutation(cells)
    got = check(ctx, once, direct=cells <= M)
    assert got[3]["n_entries"] == cells and got[3]["max_count"] == 1 and got[3]["n_modes"] == cells


# ---- hot values ------------------------------------------------------------------------------------------------------------------
def test_hot_values(ctx):
    rng = np.random.default_rng(4)
    n = 6 * TILE + 99
    got = check(ctx, np.full(n, 42), direct=True)
    assert got[3]["n_entries"] == 1 and got[3]["max_count"] == n
    x = rng.integers(0, 1000, n)
    x[rng.random(n) < 0.9] = 777
    got = check(ctx, x, direct=True)
    assert got[3]["max_count"] == int((x == 777).sum()) and got[3]["n_modes"] == 1
    check(ctx, x.astype(np.float64), rng.random(n) < 0.02, direct=True)


# ---- I64 -------------------------------------------------------------------------------------------------------------------------
def test_i64_extremes(ctx):
    rng = np.random.default_rng(5)
    n = TILE + 9
    wrap = rng.integers(-5, 5, n)
    wrap[3], wrap[n - 2] = I64_MIN, I64_MAX                                   # max - min wraps if computed signed
    check(ctx, wrap, direct=False)
    check(ctx, np.array([I64_MIN, I64_MAX], np.int64), direct=False)
    low = I64_MIN + rng.integers(0, 3, n)
    low[:3] = [I64_MIN, I64_MIN + 1, I64_MIN + 2]
    got = check(ctx, low, orders=(0,), direct=True)
    assert got[0].view(np.int64).tolist() == [I64_MIN, I64_MIN + 1, I64_MIN + 2]
    high = I64_MAX - rng.integers(0, 3, n)
    high[:3] = [I64_MAX, I64_MAX - 1, I64_MAX - 2]
    got = check(ctx, high, orders=(0,), direct=True)
    assert got[0].view(np.int64).tolist() == [I64_MAX - 2, I64_MAX - 1, I64_MAX]
    # beyond 2^53 neighbours collide as f64: counted as i64 they stay apart
    big = (1 << 53) + rng.integers(0, 8, n)
    assert np.unique(big.astype(np.float64)).size < np.unique(big).size
    got = check(ctx, big, direct=True)
    assert got[3]["n_entries"] == 8
    far = np.array([(1 << 62) + 1, (1 << 62), (1 << 62) + 1, -(1 << 62) - 1], np.int64)
    assert check(ctx, far, direct=False)[3]["n_entries"] == 3


# ---- F64 -------------------------------------------------------------------------------------------------------------------------
def test_f64_cases(ctx):
    rng = np.random.default_rng(6)
    n = 2 * TILE + 31
    x = rng.integers(-300, 300, n).astype(np.float64)
    check(ctx, x, direct=True)
    top = 2.0 ** 53 - rng.integers(0, 50, n).astype(np.float64)
    top[0] = 2.0 ** 53
    check(ctx, top, direct=True)
    check(ctx, -top, direct=True)
    check(ctx, np.array([2.0 ** 53, -(2.0 ** 53)] * 40), direct=False)        # integral, but the span is far beyond the table
    beyond = top.copy()
    beyond[7] = 2.0 ** 53 + 2
    check(ctx, beyond, direct=False)
    half = x.copy()
    half[n // 2] = 0.5
    check(ctx, half, direct=False)
    zeros = x.copy()
    zeros[5], zeros[6] = -0.0, 0.0
    got = check(ctx, zeros, orders=(0,), direct=False)
    at = np.flatnonzero(got[0] == R.SIGN)
    assert at.size == 1 and got[0][at[0] + 1] == 0                            # two entries, -0.0 first
    inf = x.copy()
    inf[1], inf[2], inf[3] = math.inf, -math.inf, math.inf
    got = check(ctx, inf, orders=(0,), direct=False)
    assert got[0][0] == np.float64(-math.inf).view(np.uint64) and got[0][-1] == np.float64(math.inf).view(np.uint64)
    nans = x.copy()
    nans[10], nans[11], nans[12], nans[13] = NAN_A, NAN_B, NAN_ONES, NAN_B
    got = check(ctx, nans, direct=True)
    assert got[3]["nan_count"] == 4 and (got[1] == L.DISTINCT_NAN).sum() == 1 and got[0][got[1] == L.DISTINCT_NAN][0] == R.CANON_NAN
    got = check(ctx, np.array([NAN_A, NAN_B, NAN_ONES] * 50), direct=True)
    assert got[3]["n_entries"] == 1 and got[3]["n_valid"] == 0 and got[3]["max_count"] == 0 and got[3]["n_modes"] == 0
    got = check(ctx, x, np.ones(n, bool), direct=True)
    assert got[3]["n_entries"] == 1 and got[3]["null_count"] == n and got[1].tolist() == [L.DISTINCT_NULL] and got[3]["max_count"] == 0


# ---- nulls -----------------------------------------------------------------------------------------------------------------------
def test_nulls_hide_their_cells(ctx):
    rng = np.random.default_rng(7)
    n = 2 * TILE + 13
    nulls = rng.random(n) < 0.3
    x = rng.integers(0, 50, n).astype(np.float64)
    x[nulls] = rng.choice([NAN_B, 1e300, 0.5, -0.0, 2.0 ** 60], int(nulls.sum()))      # garbage that would change the path if read
    got = check(ctx, x, nulls, direct=True)
    assert got[3]["nan_count"] == 0 and got[3]["n_entries"] <= 51
    i = rng.integers(0, 50, n)
    i[nulls] = rng.choice([I64_MIN, I64_MAX, 1 << 40], int(nulls.sum()))
    check(ctx, i, nulls, direct=True)
    c = rng.integers(0, 50, n).astype(np.uint32)
    c[nulls] = 0xFFFFFFFF                                                     # beyond n_codes, under a null bit: never looked at
    check(ctx, c, nulls, rank=rng.permutation(50).astype(np.uint32), direct=True)
    # a mask at a byte offset, bits past n_rows set; nulls only in the last partial word
    dx = dev(x)
    m = bits(nulls)
    m[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    for off in (1, 3):
        buf = np.full(off + m.shape[0] + 8, 0xFF, np.uint8)
        buf[off:off + m.shape[0]] = m
        check(ctx, x, nulls, col=(x, buf[off:off + m.shape[0]], L.F64), direct=True)
        check(ctx, x, nulls, col=(dx, dev(buf)[off:off + m.shape[0]], L.F64), out_device=True, direct=True)
    last = np.zeros(n, bool)
    last[n - (n % 64):] = True
    assert 0 < last.sum() < 64
    got = check(ctx, i, last)
    assert got[3]["null_count"] == int(last.sum())


# ---- U32CODE ---------------------------------------------------------------------------------------------------------------------
def test_codes(ctx):
    import pandrs_amd as pa
    rng = np.random.default_rng(8)
    n = 2 * TILE + 7
    n_codes = 300
    codes = rng.integers(0, n_codes, n).astype(np.uint32)
    rank = rng.permutation(n_codes).astype(np.uint32)
    by_rank = check(ctx, codes, rank=rank, orders=(0,), direct=True)
    assert np.array_equal(rank[by_rank[0].astype(np.int64)], np.sort(rank[np.unique(codes)]))      # BY_VALUE follows the strings
    by_code = check(ctx, codes, orders=(0,), direct=True)
    assert np.array_equal(by_code[0], np.unique(codes).astype(np.uint64))                           # ... and the codes without a table
    check(ctx, codes, rng.random(n) < 0.2, rank=rank)
    wide = rng.integers(0, 1 << 20, n).astype(np.uint32)                                           # too many cells: the engine
    check(ctx, wide, rank=rng.permutation(1 << 20).astype(np.uint32), direct=False)
    # a code >= n_codes: refused from the device, on both paths and both memory spaces; the context serves the next call
    bad = codes.copy()
    bad[n - 3] = n_codes
    for option in (1, 2):
        ctx.set_option("distinct_path", option)
        for col in ((bad, None, L.U32CODE), (dev(bad), None, L.U32CODE)):
            with pytest.raises(pa.PandrsHipError) as e:
                ctx.distinct(col, n, 0, code_rank=rank)
            assert e.value.status == L.ERR_INVALID_ARGUMENT and "n_codes" in str(e.value)
            with pytest.raises(pa.PandrsHipError):
                ctx.distinct_fetch(1)                                         # the failed call left no list
    ctx.set_option("distinct_path", 0)
    check(ctx, codes, rank=rank)


# ---- BOOLBITS --------------------------------------------------------------------------------------------------------------------
def test_bools(ctx):
    rng = np.random.default_rng(9)
    for n in (5, TILE + 3, 3 * TILE + 61):
        b = rng.random(n) < 0.3
        got = check(ctx, bits(b), dtype=L.BOOLBITS, n_rows=n, direct=True)
        assert got[2].tolist() == sorted([int(b.sum()), int((~b).sum())], reverse=True) or got[3]["n_entries"] < 2
        nulls = rng.random(n) < 0.4
        check(ctx, bits(b), nulls, dtype=L.BOOLBITS, n_rows=n, direct=True)
    check(ctx, bits(np.ones(100, bool)), dtype=L.BOOLBITS, n_rows=100, direct=True)


# ---- both orders -----------------------------------------------------------------------------------------------------------------
def test_count_ties_and_modes(ctx):
    # many count ties: the tie order is by value, then NaN, then NULL
    x = np.repeat(np.arange(40, dtype=np.float64)[::-1] - 20.0, 3)
    x = np.concatenate([x, [math.nan] * 3, [5.0] * 2])
    nulls = np.zeros(x.shape[0], bool)
    x = np.concatenate([x, [0.0] * 3])
    nulls = np.concatenate([nulls, [True] * 3])
    v, f, k, info = check(ctx, x, nulls, direct=True)                         # (the last order run: BY_COUNT)
    assert k[0] == 5 and v[0] == np.float64(5.0).view(np.uint64) and (k[1:] == 3).all()
    assert f[-2:].tolist() == [L.DISTINCT_NAN, L.DISTINCT_NULL] and (np.diff(v[1:-2].view(np.float64)) > 0).all()
    assert info["max_count"] == 5 and info["n_modes"] == 1
    # the top count is shared; a NaN / NULL entry with a larger count does not count as a mode
    y = np.array([1.0, 1.0, 2.0, 2.0, 3.0] + [math.nan] * 4)
    v, f, k, info = check(ctx, y, direct=True)
    assert info["max_count"] == 2 and info["n_modes"] == 2 and f[0] == L.DISTINCT_NAN and k[0] == 4
    i = np.array([7, 8, 9, 7, 8, 9], np.int64)
    assert check(ctx, i)[3]["n_modes"] == 3
    only = check(ctx, np.array([math.nan, 1.0, math.nan]), np.array([False, True, False]))
    assert only[3]["max_count"] == 0 and only[3]["n_modes"] == 0 and only[3]["n_entries"] == 2
    # the same on the engine path alone (a fraction keeps the direct path away)
    z = np.concatenate([np.repeat(np.arange(500) + 0.5, 2), [-0.0, 0.0, -0.0, 0.0], [math.nan] * 2])
    v, f, k, info = check(ctx, z, direct=False)
    assert info["max_count"] == 2 and info["n_modes"] == 502 and f[-1] == L.DISTINCT_NAN
    assert v[0] == R.SIGN and v[1] == 0                                       # count ties in value order: -0.0, 0.0, 0.5, ...


# ---- memory ----------------------------------------------------------------------------------------------------------------------
def test_memory_spaces_fetch_and_alignment(ctx):
    import pandrs_amd as pa
    import torch
    rng = np.random.default_rng(10)
    n = 2 * TILE + 19
    for x in (rng.integers(-9, 10, n), rng.normal(0.0, 2.0, n).round(1)):
        nulls = rng.random(n) < 0.1
        dt = dtype_of(x)
        shifted = dev(np.concatenate([x[:1], x]))[1:]                         # the data pointer 8 bytes off a 16-byte boundary
        assert shifted.data_ptr() % 16 == 8
        device_col = (dev(x), dev(bits(nulls)), dt)
        resident = ctx.upload_column(x, bits(nulls), dt)
        try:
            for col in ((x, bits(nulls), dt), device_col, (shifted, device_col[1], dt), resident):
                for out_device in (False, True):
                    check(ctx, x, nulls, col=col, out_device=out_device)
        finally:
            resident.release()
        # fetch twice, fetch with some pointers NULL, fetch after another compute call
        v, f, k, info = ctx.distinct((x, bits(nulls), dt), n, L.DISTINCT_BY_COUNT)
        g = info["n_entries"]
        for out_device in (False, True):
            v2, f2, k2 = ctx.distinct_fetch(g, out_device)
            assert np.array_equal(host(v2).view(np.uint64), v) and np.array_equal(host(f2), f) and np.array_equal(host(k2), k)
        only_k = ctx.distinct_fetch(g, values=False, flags=False)
        assert only_k[0] is None and only_k[1] is None and np.array_equal(only_k[2], k)
        only_v = ctx.distinct_fetch(g, flags=False, counts=False)
        assert np.array_equal(only_v[0], v) and only_v[1] is None and only_v[2] is None
        assert ctx.lib.pandrs_hip_distinct_fetch(ctx.h, L.MEM_HOST, None, None, None) == 0
        ctx.column_stats((x, None, dt), n)                                    # another compute call
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.distinct_fetch(g)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "retained" in str(e.value)
    fresh = pa.Context(0)
    try:
        with pytest.raises(pa.PandrsHipError) as e:
            fresh.distinct_fetch(1)                                           # no compute call at all
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        v, f, k, info = fresh.distinct((np.empty(0, np.int64), None, L.I64), 0, 0)
        assert v.size == 0 and all(info[q] == 0 for q in info)
        assert [a.size for a in fresh.distinct_fetch(0)] == [0, 0, 0]        # an empty list is a list
    finally:
        fresh.close()
    del device_col, shifted
    torch.cuda.empty_cache()


CHILD = r"""
import ctypes as C, numpy as np, sys, torch
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=1 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
small = (torch.arange(1000, dtype=torch.int64, device="cuda:0") %% 7, None, L.I64)
try:
    c.distinct(small, 1000, 0)                   # the census block and the table's counters: an arena asks for 1 MB more than it needs
    raise SystemExit("no error under a 1 MiB memory_limit")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
c.close()
cfg.memory_limit = 16 << 20
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
v, f, k, info = c.distinct(small, 1000, 0)       # fits
assert v.tolist() == list(range(7)) and int(k.sum()) == 1000 and info["path"] == 1
n = 1_000_000                                    # every row distinct: 57 bytes per entry, twice over
assert 57 * n > cfg.memory_limit
wide = (torch.arange(n, dtype=torch.int64, device="cuda:0") * 3, None, L.I64)
try:
    c.distinct(wide, n, 1)
    raise SystemExit("no error under memory_limit (engine path)")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
v, f, k, info = c.distinct(small, 1000, 1)       # the context serves the next call
assert int(k.sum()) == 1000 and info["n_entries"] == 7
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
try:
    c.distinct(small, 1000, 0)
    raise SystemExit("no error below min_size_threshold")
except pa.BelowThreshold as e:
    assert e.status == L.ERR_BELOW_THRESHOLD
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- the randomised sweep --------------------------------------------------------------------------------------------------------
def test_random_sweep(ctx):
    """About 200 small columns drawn over the axes above (dtype, rows, distinct values, offset, nulls, NaNs, fractions, signed
    zeros, order, rank table), each through both options against the twin.  No case is skipped."""
    rng = np.random.default_rng(20261020)
    ran = 0
    for case in range(200):
        dt = int(rng.integers(0, 4))
        n = int(rng.choice([1, 2, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, int(rng.integers(1, 3 * TILE))]))
        distinct_values = int(rng.choice([1, 2, 3, 17, 64, 1000, M - 1, M, M + 1, 3 * M]))
        nulls = (rng.random(n) < rng.choice([0.0, 0.05, 0.5, 1.0])) if rng.random() < 0.5 else None
        order = (int(rng.integers(0, 2)),)
        rank = None
        if dt == L.I64:
            base = int(rng.choice([0, -5, I64_MIN, I64_MAX - distinct_values + 1, 1 << 53, -(1 << 40)]))
            x = (np.int64(base) + rng.integers(0, distinct_values, n)).astype(np.int64)
            if rng.random() < 0.1:
                x[rng.integers(0, n)] = I64_MIN if base > 0 else I64_MAX
        elif dt == L.F64:
            base = float(rng.choice([0.0, -7.0, 2.0 ** 53 - distinct_values + 1, -(2.0 ** 53), 1e6]))
            x = base + rng.integers(0, distinct_values, n).astype(np.float64)
            for value, p in ((math.nan, 0.3), (NAN_B, 0.2), (NAN_ONES, 0.2), (0.5, 0.2), (-0.0, 0.2), (0.0, 0.2), (math.inf, 0.1),
                             (-math.inf, 0.1), (2.0 ** 53 + 2, 0.1)):
                if rng.random() < p:
                    x[rng.random(n) < rng.choice([0.01, 0.3])] = value
        elif dt == L.U32CODE:
            x = rng.integers(0, distinct_values, n).astype(np.uint32)
            if rng.random() < 0.6:
                rank = rng.permutation(distinct_values).astype(np.uint32)
        else:
            x = bits(rng.random(n) < rng.choice([0.0, 0.3, 1.0]))
        check(ctx, x, nulls, dtype=dt, rank=rank, n_rows=n, orders=order)
        ran += 1
    assert ran == 200


# ---- repeatability ---------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_stale_workspace(ctx):
    import pandrs_amd as pa
    rng = np.random.default_rng(11)
    n = 3 * TILE + 77
    table = np.where(rng.random(n) < 0.1, np.nan, rng.integers(-100, 100, n).astype(np.float64))
    spread = np.where(rng.random(n) < 0.1, np.nan, rng.normal(0.0, 3.0, n).round(2))
    nulls = bits(rng.random(n) < 0.1)
    codes = rng.integers(0, 500, n).astype(np.uint32)
    rank = rng.permutation(500).astype(np.uint32)

    def run():
        out = []
        for option in (1, 2):
            ctx.set_option("distinct_path", option)
            for order in (0, 1):
                for col, r in (((table, nulls, L.F64), None), ((spread, nulls, L.F64), None), ((codes, nulls, L.U32CODE), rank)):
                    v, f, k, info = ctx.distinct(col, n, order, code_rank=r)
                    out.extend([v, f, k, np.array([info[q] for q in sorted(info) if q != "path"])])
        ctx.set_option("distinct_path", 0)
        return out

    plain = run()
    half = len(plain) // 2
    assert all(np.array_equal(a, b) for a, b in zip(plain[:half], plain[half:]))       # the direct path's lists are the engine's
    try:
        for fill in (0x00, 0xFF, 0xA5):
            before = pa.Context.workspace_poisoned_bytes()
            pa.Context.poison_workspace(fill)
            got = run()
            assert all(np.array_equal(a, b) for a, b in zip(plain, got)), fill
            assert pa.Context.workspace_poisoned_bytes() > before, fill
    finally:
        pa.Context.poison_workspace(None)
        ctx.set_option("distinct_path", 0)


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------
def test_frame_methods_end_to_end(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(12)
    n = 50_000
    a = rng.integers(-30, 30, n).astype(np.float64)
    a[rng.random(n) < 0.05] = np.nan
    nulls = rng.random(n) < 0.05
    i = rng.integers(0, 1000, n)
    words = ["w%03d" % j for j in rng.permutation(200)]
    s = [words[j] for j in rng.integers(0, 200, n)]
    df = F.OptimizedDataFrame()
    df.add_column("a", F.Float64Column.with_nulls(a, nulls))
    df.add_column("i", F.Int64Column(i))
    df.add_column("s", F.StringColumn(s))
    df.add_column("flag", F.BooleanColumn(i % 3 == 0))
    va = np.where(nulls, np.nan, a).tolist()
    vi = i.astype(np.float64).tolist()

    def same(got, want):
        return len(got) == len(want) and all((g == w) or (g != g and w != w) if not isinstance(g, tuple) else
                                             ((g[0] == w[0]) or (g[0] != g[0] and w[0] != w[0])) and g[1] == w[1] for g, w in zip(got, want))

    # one NaN payload, no signed zero pair: the reference is deterministic except for where its sort leaves the NaN
    assert R.deterministic(va) and R.deterministic(vi)
    want = R.value_counts_numeric_loop(va)
    got = df.value_counts_numeric("a")
    assert sorted(got, key=lambda e: (-e[1], e[0] != e[0], e[0])) == got
    assert same(sorted(want, key=lambda e: (-e[1], e[0] != e[0], e[0])), got)
    assert same(df.value_counts_numeric("i"), R.value_counts_numeric_loop(vi))
    assert same(df.unique_numeric("i"), R.unique_numeric_loop(vi))
    want_u = sorted(v for v in R.unique_numeric_loop(va) if v == v)      # (its sort with a NaN present leaves the numbers anywhere)
    assert same(df.unique_numeric("a"), want_u + [math.nan])
    assert df.mode_numeric("a") == R.mode_numeric_loop(va) and df.mode_numeric("i") == R.mode_numeric_loop(vi)
    for name, v in (("a", va), ("i", vi)):
        m, c = df.mode_with_count(name)
        assert c == R.mode_with_count_loop(v)[1] and m == min(R.mode_numeric_loop(v))
        assert df.is_unique(name) == R.is_unique_loop(v) is False
    assert df.value_counts("s") == R.value_counts_loop(s)
    assert df.unique("s") == R.unique_loop(s) and df.mode_string("s") == R.mode_string_loop(s)
    strings = {"a": [F.rust_f64_to_string(v) for v in va], "i": [str(v) for v in i.tolist()], "s": s,
               "flag": ["true" if v else "false" for v in (i % 3 == 0).tolist()]}
    assert df.nunique() == R.nunique_loop([(name, strings[name]) for name in df.column_names])
    assert df.nunique_all() == R.nunique_all_loop({"a": va, "i": vi}, {"s": s, "flag": strings["flag"]})
    assert df.value_counts("flag") == R.value_counts_loop(strings["flag"])
    assert df.value_counts("i") == R.value_counts_loop(strings["i"])
    u = F.OptimizedDataFrame()
    u.add_column("x", F.Int64Column(rng.permutation(5000)))
    assert u.is_unique("x") and u.nunique_all() == {"x": 5000}


def test_groupby_regroups_after_a_distinct_call(ctx):
    """A GroupBy's retained grouping, a distinct call on the same context (both paths), then a grouped cumsum: still right."""
    import pandrs_amd.frame as F
    rng = np.random.default_rng(13)
    n = 20_000
    key = rng.integers(0, 37, n)
    val = rng.integers(-5, 6, n).astype(np.float64)
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column(key))
    df.add_column("v", F.Float64Column(val))
    want = np.empty(n)
    for g in np.unique(key):
        rows = np.flatnonzero(key == g)
        want[rows] = np.cumsum(val[rows])
    gb = df.group_by(["k"])
    assert gb.cumsum("v") == want.tolist()
    shared = F.get_context()
    try:
        for option, column in ((1, key), (2, key), (2, rng.normal(0, 1, n))):
            shared.set_option("distinct_path", option)
            v, f, k, info = shared.distinct((column, None, dtype_of(column)), n, L.DISTINCT_BY_COUNT)
            assert int(k.sum()) == n and info["path"] == option
            assert gb.cumsum("v") == want.tolist(), option
            assert gb.cummax("v") == [float(x) for x in _grouped_cummax(key, val)], option
    finally:
        shared.set_option("distinct_path", 0)
    assert df.mode_with_count("k")[1] == int(np.bincount(key).max()) and gb.cumsum("v") == want.tolist()


def _grouped_cummax(key, val):
    out = np.empty(val.shape[0])
    for g in np.unique(key):
        rows = np.flatnonzero(key == g)
        out[rows] = np.maximum.accumulate(val[rows])
    return out


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(ctx):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "distinct_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "distinct_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "12 tests, 0 failed checks" in r.stdout
