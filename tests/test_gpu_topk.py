"""pandrs_hip_topk / pandrs_hip_arg_extreme and the mirrors' nlargest / nsmallest / idxmax / idxmin (reference
src/dataframe/pandas_compat/functions.rs:159-192) against tests/topk_ref.py.  Every result is a list of row indices: every
comparison is index for index, no tolerance anywhere in this file.  Every column is asked through the default path, through
the select ("topk_path" -1) and through the whole-column sort (1): the three must agree with the restatement."""
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
from tests.topk_ref import idx_extreme_ref, topk_ref  # noqa: E402

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"topk_tile_rows = (\d+)", HEADER).group(1))
CUT_NUM, CUT_DEN = map(int, re.search(r"topk_cutover = (\d+) / (\d+)", HEADER).groups())


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.set_option("topk_path", 0)
    c.close()


def full_grid():
    import torch
    return int(re.search(r"topk_blocks_per_cu = (\d+)", HEADER).group(1)) * torch.cuda.get_device_properties(0).multi_processor_count


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def interesting_ks(x, nulls):
    """0, 1, 2, the ends of the number / NaN / null blocks, n and beyond, both sides of the cut-over, and the edges of the
    tie run in the middle of the numbers (where `better` ends and where the quota ends)."""
    n = x.shape[0]
    nul = np.zeros(n, bool) if nulls is None else np.asarray(nulls, bool)
    nan = (np.isnan(x) if x.dtype == np.float64 else np.zeros(n, bool)) & ~nul
    m, n_nan = int((~nul & ~nan).sum()), int(nan.sum())
    cut = -(-n * CUT_NUM // CUT_DEN)                                     # the smallest k the sort answers
    ks = {0, 1, 2, m - 1, m, m + 1, m + n_nan, n - 1, n, n + 5, cut - 1, cut}
    if m:
        v = np.sort(x[~nul & ~nan])
        mid = v[m // 2]
        lo, hi = int((v < mid).sum()), int((v <= mid).sum())
        ks |= {lo, lo + 1, hi - 1, hi, hi + 1, m - hi, m - hi + 1, m - lo - 1, m - lo}
    return sorted(k for k in ks if k >= 0)


def check(ctx, x, nulls=None, ks=None, col=None, paths=(0, -1, 1)):
    """Every k in both directions through every path against the restatement; `col` overrides how the column is passed."""
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    n = x.shape[0]
    dtype = L.I64 if x.dtype == np.int64 else L.F64
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype)
    ks = interesting_ks(x, nulls) if ks is None else ks
    try:
        for largest in (True, False):
            order, m = topk_ref(x, nulls, n, largest)                     # once per direction: every k is a head of it
            for path in paths:
                ctx.set_option("topk_path", path)
                for k in ks:
                    got, numbers = ctx.topk(col, n, k, largest, out_device=False)
                    assert got.shape[0] == min(k, n) and numbers == min(k, m), (largest, path, k, got.shape, numbers, m)
                    bad = np.flatnonzero(got != order[:k])
                    assert bad.size == 0, (largest, path, n, k, bad[:5], got[bad[:5]], order[:k][bad[:5]])
    finally:
        ctx.set_option("topk_path", 0)
    want = idx_extreme_ref(x, nulls) if n <= 70_000 else None
    if n <= 70_000:
        assert ctx.arg_extreme(col, n) == want, (n, want)


# ---- row counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, rng.integers(0, max(2, n // 3), n).astype(np.float64))
    check(ctx, rng.integers(-n, n + 1, n))
    check(ctx, rng.normal(0, 1, n))


def test_more_tiles_than_workgroups(ctx):
    n = full_grid() * TILE + TILE + 3                                     # every workgroup loops, one of them twice more
    rng = np.random.default_rng(3)
    x = rng.integers(0, 50_000, n).astype(np.float64)
    x[rng.random(n) < 0.01] = np.nan
    check(ctx, x, rng.random(n) < 0.01, ks=[1, 100, 5000, n // 3], paths=(0,))
    check(ctx, rng.integers(-40, 40, n), ks=[1, 100, n // 80 + 1, n // 3], paths=(-1,))   # tie runs far longer than a tile


def test_both_sides_of_the_cut_over_agree(ctx):
    rng = np.random.default_rng(17)
    n = 4 * TILE + 5
    x = rng.integers(0, 300, n).astype(np.float64)
    nulls = rng.random(n) < 0.05
    cut = -(-n * CUT_NUM // CUT_DEN)
    col = (x, bits(nulls), L.F64)
    for largest in (True, False):
        below, _ = ctx.topk(col, n, cut - 1, largest, out_device=False)
        above, _ = ctx.topk(col, n, cut, largest, out_device=False)
        assert np.array_equal(above[:cut - 1], below)
        for k in (cut - 1, cut):
            outs = []
            for path in (-1, 1):
                ctx.set_option("topk_path", path)
                outs.append(ctx.topk(col, n, k, largest, out_device=False)[0])
            ctx.set_option("topk_path", 0)
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], topk_ref(x, nulls, k, largest)[0])


# ---- ties ------------------------------------------------------------------------------------------------------------------
def test_all_cells_equal_is_the_quota_alone(ctx):
    n = 2 * TILE + 9
    check(ctx, np.full(n, 2.5), ks=[1, 63, 64, 65, TILE, TILE + 1, n - 1, n])
    ctx.set_option("topk_path", -1)
    try:
        got, _ = ctx.topk((np.full(n, 7, np.int64), None, L.I64), n, 100, True, out_device=False)
        assert np.array_equal(got, np.arange(100)) and ctx.timings()["n_partitions"] == 0          # no digit stream at all
    finally:
        ctx.set_option("topk_path", 0)


def test_quota_ends_inside_a_wave_at_a_tile_edge_and_one_row_past_it(ctx):
    n = 3 * TILE + 40
    x = np.zeros(n)                                                       # two values: the 1.0 rows beat the 0.0 rows (largest)
    x[[5, TILE + 7, 2 * TILE + 1]] = 1.0
    # k - 3 zeros are taken: the quota ends inside a wave, at the last row of tile 0, at the first row of tile 1
    zeros_before = lambda row: row - int((np.flatnonzero(x == 1.0) < row).sum())   # noqa: E731
    ks = [3 + 30, 3 + zeros_before(TILE), 3 + zeros_before(TILE) + 1, 3 + zeros_before(2 * TILE), 3 + zeros_before(2 * TILE) + 1]
    check(ctx, x, ks=ks)
    check(ctx, x.astype(np.int64), ks=ks)
    check(ctx, -x, ks=ks)                                                 # the same rows beat the rest the other way round


def test_signed_zeros_tie(ctx):
    x = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0] * 700)
    check(ctx, x)
    got, _ = ctx.topk((x, None, L.F64), x.shape[0], 700 + 5, True, out_device=False)
    assert list(got[700:]) == [0, 1, 3, 4, 6]                             # the zeros of either sign, in row order


def test_int64_neighbours_beyond_2_pow_53_and_the_extremes(ctx):
    rng = np.random.default_rng(51)
    big = np.array([2**53 + 1, 2**53, 2**53 + 1, 2**53], np.int64)       # equal as f64, apart as integers
    check(ctx, big)
    got, _ = ctx.topk((big, None, L.I64), 4, 2, True, out_device=False)
    assert list(got) == [0, 2]
    check(ctx, 2**53 + rng.integers(0, 64, 5001))
    lim = np.array([I64_MIN, I64_MAX, 0, -1, 1], np.int64)[rng.integers(0, 5, 4099)]
    check(ctx, lim, rng.random(4099) < 0.1)
    assert ctx.arg_extreme((np.array([I64_MAX, 7, I64_MIN, I64_MAX, I64_MIN], np.int64), None, L.I64), 5) == (2, 3)


# ---- code width ------------------------------------------------------------------------------------------------------------
def test_code_widths(ctx):
    rng = np.random.default_rng(61)
    n = TILE + 77
    ks = [1, 2, 10, 257, n // 3]
    low = (rng.integers(0, 256, n) + (1 << 40)).astype(np.int64)         # only the lowest byte varies: one digit stream
    check(ctx, low, ks=ks)
    ctx.set_option("topk_path", -1)
    try:
        ctx.topk((low, None, L.I64), n, 10, True)
        assert ctx.timings()["n_partitions"] == 1
        high = (rng.integers(-128, 128, n) << 56).astype(np.int64)       # only the highest byte varies: the lower digits are skipped
        ctx.topk((high, None, L.I64), n, 10, False)
        assert ctx.timings()["n_partitions"] == 1
        wide = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
        wide[:2] = [I64_MIN, I64_MAX]
        ctx.topk((wide, None, L.I64), n, 10, True)
        assert ctx.timings()["n_partitions"] == 8                         # all eight passes
    finally:
        ctx.set_option("topk_path", 0)
    check(ctx, high, ks=ks)
    check(ctx, wide, ks=ks)
    patterns = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64).view(np.float64)     # random 64-bit patterns, NaN among them
    check(ctx, patterns, ks=ks + [n])
    inf = rng.normal(0, 1, n)
    inf[rng.integers(0, n, 9)] = np.inf
    inf[rng.integers(0, n, 9)] = -np.inf
    check(ctx, inf, ks=[1, 5, 9, 10, 18, n])
    sub = rng.integers(-50, 50, n).astype(np.float64) * 5e-324            # subnormals around both zeros
    check(ctx, sub, ks=ks)


# ---- NaN and null cells ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.0, 0.1, 1.0])
def test_nan_and_null_shares(ctx, share):
    rng = np.random.default_rng(int(share * 100) + 20)
    n = 2 * TILE + 311
    x = rng.integers(0, 300, n).astype(np.float64)
    nan = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    nulls = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    xn = np.where(nan, np.nan, x)
    check(ctx, xn)                                                        # NaN cells only
    check(ctx, x, nulls)                                                  # null cells only
    check(ctx, x.astype(np.int64), nulls)
    check(ctx, xn, nulls[::-1].copy())                                    # both
    if share == 1.0:
        check(ctx, x, np.arange(n) != 77)                                 # one number
        assert ctx.arg_extreme((xn, bits(nulls), L.F64), n) is None and ctx.arg_extreme((xn, None, L.F64), n) is None


def test_garbage_under_null_bits_and_stray_mask_bits(ctx):
    rng = np.random.default_rng(31)
    n = 1003                                                              # the last mask byte holds 3 rows
    x = rng.integers(0, 40, n).astype(np.float64)
    nulls = rng.random(n) < 0.3
    junk = x.copy()
    junk[nulls] = rng.choice([np.nan, np.inf, -np.inf, 1e308, -1e308], int(nulls.sum()))   # never looked at
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8
    check(ctx, x, nulls, col=(junk, mask, L.F64))
    ji = x.astype(np.int64)
    ji[nulls] = rng.choice([I64_MIN, I64_MAX], int(nulls.sum()))
    check(ctx, x.astype(np.int64), nulls, col=(ji, mask, L.I64))


# ---- memory spaces ---------------------------------------------------------------------------------------------------------
def test_host_device_resident_and_misaligned_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(71)
    n = 3 * TILE + 7
    x = rng.integers(0, 500, n).astype(np.float64)
    x[rng.random(n) < 0.05] = np.nan
    nulls = rng.random(n) < 0.15
    mask = bits(nulls)
    ks = [1, 40, 700, n]
    check(ctx, x, nulls, ks=ks)
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    pad = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")       # rows start 8 bytes off a 16-byte boundary
    pad[1:] = dx
    assert pad.data_ptr() % 16 == 0
    padm = torch.empty(mask.shape[0] + 3, dtype=torch.uint8, device="cuda:0")   # the mask at byte offsets 0 and 3
    padm[3:] = dm
    res = ctx.upload_column(x, mask, L.F64)
    try:
        for col in ((dx, dm, L.F64), (pad[1:], padm[3:], L.F64), res):
            check(ctx, x, nulls, ks=ks, col=col)                          # host out_rows
            for largest in (True, False):
                want = topk_ref(x, nulls, 700, largest)[0]
                dev, _ = ctx.topk(col, n, 700, largest)                   # device out_rows
                assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
                into = torch.full((700 + 3,), -7, dtype=torch.int64, device="cuda:0")
                ctx.topk(col, n, 700, largest, out=into[1:701])           # 8 bytes off a 16-byte boundary, guard words around it
                got = into.cpu().numpy()
                assert np.array_equal(got[1:701], want) and got[0] == -7 and (got[701:] == -7).all()
                for path in (-1, 1):                                      # n + 5 rows asked for: exactly n written
                    ctx.set_option("topk_path", path)
                    wide = torch.full((n + 9,), -7, dtype=torch.int64, device="cuda:0")
                    rows, _ = ctx.topk(col, n, n + 5, largest, out=wide[2:])
                    ctx.set_option("topk_path", 0)
                    got = wide.cpu().numpy()
                    assert rows.numel() == n and np.array_equal(got[2:2 + n], topk_ref(x, nulls, n, largest)[0])
                    assert (got[:2] == -7).all() and (got[2 + n:] == -7).all()
        dev, _ = ctx.topk((x, mask, L.F64), n, 40, True, out_device=True)     # host column, device out_rows
        assert np.array_equal(dev.cpu().numpy(), topk_ref(x, nulls, 40, True)[0])
        buf = np.full(42, -7, np.int64)
        ctx.topk(res, n, 40, False, out=buf[1:41])                        # resident column, a caller's host out_rows
        assert np.array_equal(buf[1:41], topk_ref(x, nulls, 40, False)[0]) and buf[0] == -7 and buf[41] == -7
    finally:
        res.release()
    for m in (1, 2, 3, 17):                                               # a mask whose byte offset makes rows straddle bytes
        check(ctx, x[:m], nulls[:m], col=(pad[1:1 + m], padm[3:], L.F64))


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import pandrs_amd as pa
    x = np.arange(16, dtype=np.float64)
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.topk((other, None, dt), 16, 3)
        assert e.value.status == L.ERR_TYPE_MISMATCH
        with pytest.raises(pa.ColumnTypeMismatch):
            ctx.arg_extreme((other, None, dt), 16)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.topk((x, None, L.F64), 16, -1)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out = np.full(16, -7, np.int64)
    cnt, num = C.c_int64(0), C.c_int64(0)
    args = (C.byref(cnt), C.byref(num))
    assert lib.pandrs_hip_topk(ctx.h, L.MEM_HOST, C.byref(c), 16, 3, 2, L.MEM_HOST, out.ctypes.data, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_topk(ctx.h, L.MEM_HOST, C.byref(c), 16, 3, 0, L.MEM_HOST, None, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_topk(ctx.h, L.MEM_HOST, C.byref(c), 16, 3, 0, 7, out.ctypes.data, *args) == L.ERR_INVALID_ARGUMENT
    nodata = L.Column()
    nodata.dtype = L.F64
    assert lib.pandrs_hip_topk(ctx.h, L.MEM_HOST, C.byref(nodata), 16, 3, 0, L.MEM_HOST, out.ctypes.data, *args) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_topk(ctx.h, L.MEM_HOST, C.byref(c), 16, 0, 0, L.MEM_HOST, out.ctypes.data, *args) == 0
    assert (out == -7).all() and (cnt.value, num.value) == (0, 0)
    rows, n = ctx.topk((x, None, L.F64), 0, 5)
    assert rows.shape[0] == 0 and n == 0 and ctx.arg_extreme((x, None, L.F64), 0) is None


# ---- limits, in a child process ----------------------------------------------------------------------------------------------
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
n = 8_000_000                                                   # device column, device out_rows: nothing to stage
big = (torch.arange(n, dtype=torch.float64, device="cuda:0"), None, L.F64)
def refused(k, col=big, rows=n, **kw):
    try:
        c.topk(col, rows, k, **kw)
        raise SystemExit("no error under memory_limit (k = %%d)" %% k)
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
assert 16 * 1_500_000 > cfg.memory_limit and %d * 1_500_000 < %d * n   # the candidates alone, below the cut-over (documented: 48 bytes per requested row)
refused(1_500_000)
assert 24 * n > cfg.memory_limit                                 # above the cut-over: the sort's 24 bytes per row
refused(n)
refused(10, col=(np.zeros(n), None, L.F64), out_device=True)     # 64 MB to stage
rows, numbers = c.topk(big, n, 1000)                             # 48 KB of candidates and sort: fits
assert torch.equal(rows, torch.arange(n - 1, n - 1001, -1, device="cuda:0")) and numbers == 1000
assert c.arg_extreme(big, n) == (0, n - 1)
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
for call in (lambda: c.topk((x, None, L.F64), 1000, 3), lambda: c.arg_extreme((x, None, L.F64), 1000)):
    try:
        call()
        raise SystemExit("no error below min_size_threshold")
    except pa.BelowThreshold as e:
        assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
for call in (lambda: df.nlargest(3, "x"), lambda: df.idxmax("x")):
    try:
        call()
        raise SystemExit("the frame did not raise below min_size_threshold")
    except pa.BelowThreshold:
        pass
y = np.arange(20_000, dtype=np.float64)[::-1].copy()
assert list(c.topk((y, None, L.F64), 20_000, 3, out_device=False)[0]) == [0, 1, 2]
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, CUT_DEN, CUT_NUM)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- one case at size: the property the header states ------------------------------------------------------------------------
def test_two_million_rows_equal_the_head_of_sort_indices(ctx):
    import torch
    rng = np.random.default_rng(101)
    n = 2_000_000
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.05] = np.nan
    mask = bits(rng.random(n) < 0.05)
    col = (torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda(), L.F64)
    for largest in (True, False):
        order = ctx.sort_indices([col], n, [not largest])
        for k in (10, 10_000):
            rows, numbers = ctx.topk(col, n, k, largest)
            assert numbers == k and torch.equal(rows, order[:k]), (largest, k)
    both = idx_extreme_ref(x[:50_000], np.unpackbits(mask, bitorder="little")[:50_000])
    assert ctx.arg_extreme((x[:50_000], mask[:6250], L.F64), 50_000) == both


def test_more_than_one_tile_per_scanning_thread(ctx):
    """More than 1024 tiles: a thread of the one-workgroup scan owns two tiles, and the chosen rows lie in both of them."""
    import torch
    rng = np.random.default_rng(103)
    n = 1024 * TILE + TILE + 1
    x = rng.integers(0, 1000, n).astype(np.float64)                       # ties everywhere: every tile holds better and equal rows
    x[rng.random(n) < 0.02] = np.nan
    mask = bits(rng.random(n) < 0.02)
    col = (torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda(), L.F64)
    ctx.set_option("topk_path", -1)
    try:
        for largest in (True, False):
            order = ctx.sort_indices([col], n, [not largest])
            for k in (5000, n - 7):                                       # inside the numbers; into the NaN and null blocks
                rows, _ = ctx.topk(col, n, k, largest)
                assert torch.equal(rows, order[:k]), (largest, k)
    finally:
        ctx.set_option("topk_path", 0)


# ---- arg_extreme -------------------------------------------------------------------------------------------------------------
def test_arg_extreme_keeps_the_first_minimum_and_the_last_maximum_across_tiles(ctx):
    n = full_grid() * TILE + 3 * TILE + 5                                 # workgroups stride: a workgroup meets several tiles
    x = np.full(n, 5.0)
    hi = [7, TILE + 1, 5 * TILE - 1, n - TILE - 3]
    lo = [TILE - 1, 2 * TILE, n - 9]
    x[hi] = 9.0
    x[lo] = -9.0
    assert ctx.arg_extreme((x, None, L.F64), n) == (lo[0], hi[-1])
    assert ctx.arg_extreme(((x * 2).astype(np.int64), None, L.I64), n) == (lo[0], hi[-1])
    nulls = np.zeros(n, bool)
    nulls[[lo[0], hi[-1]]] = True                                         # the winners go missing: the next ones answer
    x[hi[-2]] = np.nan
    assert ctx.arg_extreme((x, bits(nulls), L.F64), n) == (lo[1], hi[-3])
    assert ctx.arg_extreme((np.full(n, 1.5), None, L.F64), n) == (0, n - 1)      # all equal: first and last row
    assert ctx.arg_extreme((np.array([0.0, -0.0, 0.0, -0.0]), None, L.F64), 4) == (0, 3)
    assert ctx.arg_extreme((np.array([3.0]), None, L.F64), 1) == (0, 0)
    assert ctx.arg_extreme((np.array([3.0]), bits([True]), L.F64), 1) is None


# ---- mirrors -----------------------------------------------------------------------------------------------------------------
def test_frame_mirror_on_a_mixed_frame(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(81)
    n = 3001
    f, fn = rng.integers(0, 60, n).astype(np.float64), rng.random(n) < 0.2
    f[rng.random(n) < 0.05] = np.nan
    i = rng.integers(-50, 50, n)
    df = F.OptimizedDataFrame()
    df.add_column("i", F.Int64Column(i))
    df.add_column("f", F.Float64Column.with_nulls(f, fn))
    df.add_column("s", F.StringColumn.with_nulls(list(rng.choice(["a", "b", "c"], n)), rng.random(n) < 0.1))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    for name in ("f", "i"):
        for largest, fn_ in ((True, df.nlargest), (False, df.nsmallest)):
            whole = df.sort_by_columns([name], [not largest])
            for k in (1, 37, n, n + 4):
                got = fn_(k, name)
                assert got.row_count() == min(k, n) and got.column_names == whole.column_names
                for cname in df.column_names:
                    a, b = got.column(cname), whole.column(cname)
                    assert a.null_mask is None
                    if cname == "s":
                        assert a.to_list() == b.to_list()[:k]
                    elif cname == "b":
                        assert [a.get(r) for r in range(min(k, n))] == [b.get(r) for r in range(min(k, n))]
                    else:
                        assert np.array_equal(np.asarray(a.data).view(np.uint64), np.asarray(b.data)[:k].view(np.uint64)), (name, cname, k)
    assert (df.idxmin("f"), df.idxmax("f")) == idx_extreme_ref(f, fn) and (df.idxmin("i"), df.idxmax("i")) == idx_extreme_ref(i)
    known = F.OptimizedDataFrame()                                        # create_test_df, functions.rs:4327-4391
    known.add_column("a", F.Float64Column([1.0, 2.0, 3.0, 4.0, 5.0]))
    known.add_column("name", F.StringColumn(["Alice", "Bob", "Charlie", "David", "Eve"]))
    assert known.nlargest(3, "a").row_count() == 3 and known.nsmallest(2, "a").row_count() == 2
    assert known.nlargest(3, "a").column("name").to_list() == ["Eve", "David", "Charlie"]
    assert known.idxmax("a") == 4 and known.idxmin("a") == 0


def test_cpp_mirror_topk():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "topk_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "topk_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
