"""pandrs_hip_pivot / pandrs_hip_pivot_fetch and the mirrors' crosstab / pivot_table / pivot / unstack (reference
src/dataframe/pandas_compat/functions.rs:2138-2183, :2471-2527, src/pivot/mod.rs:12-250) against tests/pivot_ref.py's twin of the
contract.  Labels, flags, rows per cell and the cells of Min / Max / Count / Last / Rows are compared bit for bit; Sum and Mean of
an F64 column within 2 gamma_k sum|x| over the cell's own rows (pivot_ref.bound), which is 0 for I64 values.  Wherever the direct
(LDS table) path is possible a case runs under "pivot_path" 1 and 2 and both must give the twin's result."""
import math
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
from tests import pivot_ref as R  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"pivot_tile_rows = (\d+)", HEADER).group(1))
M = int(re.search(r"pivot_direct_max_cells = (\d+)", HEADER).group(1))
MAX_CELLS = int(re.search(r"pivot_max_cells = (\d+)", HEADER).group(1))
BLOCKS_PER_CU = int(re.search(r"pivot_blocks_per_cu = (\d+)", HEADER).group(1))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
assert (L.I64, L.F64, L.U32CODE, L.BOOLBITS) == (R.I64, R.F64, R.U32CODE, R.BOOLBITS)
assert (L.PIVOT_ROWS, L.PIVOT_SUM, L.PIVOT_MEAN, L.PIVOT_MIN, L.PIVOT_MAX, L.PIVOT_COUNT, L.PIVOT_LAST) == R.OPS
assert (L.PIVOT_NUMBER, L.PIVOT_MISSING) == (R.NUMBER, R.MISSING)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.set_option("pivot_path", 0)
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


def icol(x, nulls=None):
    return (np.asarray(x, np.int64), None if nulls is None else bits(nulls), L.I64)


def fcol(x, nulls=None):
    return (np.asarray(x, np.float64), None if nulls is None else bits(nulls), L.F64)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def compare(got, want, tol, op, where):
    il, fi, cl, fc, cells, rows = [host(x) for x in got[:6]]
    il, cl = il.view(np.uint64), cl.view(np.uint64)
    assert il.dtype == np.uint64 and fi.dtype == np.uint8 and cells.dtype == np.float64 and rows.dtype == np.int64, where
    assert np.array_equal(il, want[0]) and np.array_equal(fi, want[1]), (where, il[:8], want[0][:8], fi[:8], want[1][:8])
    assert np.array_equal(cl, want[2]) and np.array_equal(fc, want[3]), (where, cl[:8], want[2][:8], fc[:8], want[3][:8])
    assert rows.shape == want[5].shape and np.array_equal(rows, want[5]), (where, rows, want[5])
    w = want[4]
    assert cells.shape == w.shape and np.array_equal(np.isnan(cells), np.isnan(w)), (where, cells, w)
    assert np.array_equal(u64(cells[rows == 0]), np.full(int((rows == 0).sum()), 0x7FF8000000000000, np.uint64)), where     # absent: the canonical NaN
    ok = ~np.isnan(w)
    if op in (R.SUM, R.MEAN):
        exact = ok & (~np.isfinite(w) | ~np.isfinite(tol))
        assert np.array_equal(cells[exact], w[exact]), (where, cells[exact], w[exact])
        close = ok & ~exact
        diff = np.abs(cells[close] - w[close])
        assert (diff <= tol[close]).all(), (where, diff.max(), tol[close][diff.argmax()])
    else:
        assert np.array_equal(u64(cells[ok]), u64(w[ok])), (where, cells[ok][:8], w[ok][:8])


def check(ctx, k1, k2, n, op, v=None, r1=None, r2=None, cols=None, out_device=False, direct=None, options=(1, 2)):
    """The result through both options against the twin, the info, the invariants, the path taken.  `cols` overrides how the
    columns are passed; `direct`: whether the direct path must (True) / cannot (False) be possible (None: the twin's rule)."""
    want = R.pivot(k1, k2, n, op, v, r1, r2)
    tol = R.bound(k1, k2, n, op, v, r1, r2)
    table = R.spans(k1, k2, n)
    possible = table is not None and table <= M
    if direct is not None:
        assert possible == direct, table
    p1, p2, pv = cols if cols is not None else (k1, k2, v)
    out = None
    try:
        for option in options:
            ctx.set_option("pivot_path", option)
            got = ctx.pivot(p1, p2, n, op, pv, index_rank=r1, columns_rank=r2, out_device=out_device)
            info = got[6]
            where = (n, R.OP_NAME[op], option, info)
            compare(got, want, tol, op, where)
            rows = host(got[5])
            assert info["n_index_labels"] == want[0].shape[0] and info["n_column_labels"] == want[2].shape[0], where
            assert info["n_cells_present"] == int((want[5] > 0).sum()) and int(rows.sum()) == n, where
            assert info["index_missing_rows"] == int(want[5][:, want[1] == R.MISSING].sum()), where
            assert info["column_missing_rows"] == int(want[5][want[3] == R.MISSING].sum()), where
            if n:
                assert (rows.sum(axis=0) > 0).all() and (rows.sum(axis=1) > 0).all(), where        # no label without a row
                assert info["path"] == (1 if possible and option != 2 else 2), (where, table)
                assert ctx.timings()["n_partitions"] == info["path"], where
            else:
                assert info["path"] == 0 and rows.size == 0
            out = got
    finally:
        ctx.set_option("pivot_path", 0)
    return out


# ---- row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    k1, k2 = icol(rng.integers(-4, 5, n)), icol(rng.integers(100, 111, n))
    v = fcol(rng.normal(0, 10, n), rng.random(n) < 0.1)
    for op in R.OPS:
        check(ctx, k1, k2, n, op, None if op == R.ROWS else v, direct=True)
    f1 = rng.integers(-4, 5, n).astype(np.float64)
    f1[rng.random(n) < 0.1] = np.nan
    check(ctx, fcol(f1, rng.random(n) < 0.1), k2, n, R.SUM, v, direct=True)
    check(ctx, fcol(rng.normal(0, 1, n).round(1)), k2, n, R.MAX, v, direct=n == 0 or None)


def test_more_workgroups_than_tiles_and_one_tile_past_the_grid(ctx):
    import torch
    grid = BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2)
    assert 3 * TILE + 1 < grid * TILE                                         # fewer tiles than the full grid: the grid shrinks to them
    n = grid * TILE + 1                                                       # one row past the grid: workgroup 0 takes a second, one-row tile
    k1, k2 = rng.integers(0, 9, n), rng.integers(0, 13, n)
    k1[-1], k2[-1] = 9, 13                                                    # the last row is the only one of its cell
    val = rng.integers(-50, 50, n)
    for op, v in ((R.ROWS, None), (R.SUM, icol(val)), (R.LAST, icol(val)), (R.MIN, fcol(val / 4.0))):
        got = check(ctx, icol(k1), icol(k2), n, op, v, direct=True)
        assert host(got[5])[-1, -1] == 1


# ---- ops and dtypes ---------------------------------------------------------------------------------------------------------------
GRID = list(R.grid_cases())


@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_every_op_key_dtype_and_mask(ctx, case):
    name, k1, k2, v, n, op, r1, r2 = case
    check(ctx, k1, k2, n, op, v, r1, r2, direct=True)


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_masks_at_byte_offsets(ctx, offset):
    """Device columns whose null masks start `offset` bytes into their allocation."""
    rng = np.random.default_rng(30 + offset)
    n = TILE + 37
    k1, r1 = R.make_key(rng, n, "f64", 6, 0.2, 0.1)
    k2, r2 = R.make_key(rng, n, "code_rank", 9, 0.2)
    v = R.make_values(rng, n, R.F64, 0.2, special=True)

    def shifted(mask):
        return dev(np.concatenate([np.full(offset, 0xFF, np.uint8), mask]))[offset:]

    cols = ((dev(k1[0]), shifted(k1[1]), k1[2]), (dev(k2[0]), shifted(k2[1]), k2[2]), (dev(v[0]), shifted(v[1]), v[2]))
    assert cols[0][1].data_ptr() % 4 == offset % 4
    for op in R.OPS:
        check(ctx, k1, k2, n, op, None if op == R.ROWS else v, r1, r2, cols=cols[:2] + ((None,) if op == R.ROWS else (cols[2],)), direct=True)


# ---- path switching ---------------------------------------------------------------------------------------------------------------
def test_path_flips_one_cell_past_the_table(ctx):
    rng = np.random.default_rng(4)
    n = 3000
    assert M == 64 * 64 and M + 1 == 17 * 241
    val = fcol(rng.normal(0, 5, n))
    for (s1, s2), direct in (((63, 63), True), ((16, 240), False), ((1, M // 2 - 1), True), ((1, M // 2), False)):
        a, b = rng.integers(0, s1, n), rng.integers(0, s2, n)
        a[:2], b[:2] = (0, s1 - 1), (0, s2 - 1)                              # the whole span is there
        assert R.spans(icol(a), icol(b), n) == (s1 + 1) * (s2 + 1)
        for op in (R.ROWS, R.MEAN, R.LAST):
            got = check(ctx, icol(a), icol(b), n, op, None if op == R.ROWS else val, direct=direct, options=(0, 1, 2))
            assert got[6]["path"] == 2                                        # (the last option run was 2)
        ctx.set_option("pivot_path", 0)
        assert ctx.pivot(icol(a), icol(b), n, R.ROWS)[6]["path"] == (1 if direct else 2)


# ---- cells and labels -------------------------------------------------------------------------------------------------------------
def test_hot_cells_and_every_row_its_own_cell(ctx):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 5
    val = rng.normal(0, 3, n)
    one = np.zeros(n, np.int64)
    for op in R.OPS:
        v = None if op == R.ROWS else fcol(val)
        check(ctx, icol(one + 7), icol(one - 3), n, op, v, direct=True)      # every row in one cell
        hot = rng.random(n) < 0.9                                             # 90 % of the rows in one cell
        check(ctx, icol(np.where(hot, 3, rng.integers(0, 9, n))), icol(np.where(hot, 5, rng.integers(0, 11, n))), n, op, v, direct=True)
        check(ctx, icol(np.where(hot, 3, rng.integers(0, 9, n))), icol(np.where(hot, 5, rng.integers(0, 11, n))), n, op,
              None if op == R.ROWS else icol(rng.integers(-9, 9, n)), direct=True)
    m = 63 * 63                                                               # every row its own cell, the direct table full
    order = rng.permutation(m)
    for op in (R.ROWS, R.SUM, R.MIN, R.LAST):
        got = check(ctx, icol(order % 63), icol(order // 63), m, op, None if op == R.ROWS else fcol(val[:m]), direct=True)
        assert (host(got[5]) == 1).all()
    m = 5000                                                                  # ... and past it
    got = check(ctx, icol(np.arange(m) % 71), icol(np.arange(m) // 71), m, R.LAST, fcol(rng.normal(0, 3, m)), direct=False)
    assert host(got[5]).sum() == m and got[6]["n_cells_present"] == m


def test_span_rows_and_columns_without_a_row_are_dropped(ctx):
    rng = np.random.default_rng(6)
    n = 900
    a = rng.choice([-5, -4, 0, 9, 30], n)                                     # a span of 36 with 5 labels
    b = rng.choice([2.0, 3.0, 50.0], n)                                       # a span of 49 with 3 labels
    keep = ~((a == 0) & (b == 3.0))                                           # and a cell no row reaches
    a, b = a[keep], b[keep]
    n = a.shape[0]
    val = fcol(rng.normal(0, 1, n))
    for op in R.OPS:
        got = check(ctx, icol(a), fcol(b), n, op, None if op == R.ROWS else val, direct=True)
        assert got[6]["n_index_labels"] == 5 and got[6]["n_column_labels"] == 3 and got[6]["n_cells_present"] == 14
        assert host(got[5])[1, 2] == 0 and math.isnan(host(got[4])[1, 2])
    # a label only the missing cells of the OTHER column reach, and a missing label only one row reaches
    a2 = np.array([1, 1, 2, 3, 3], np.int64)
    b2 = np.array([5.0, math.nan, math.nan, 6.0, 5.0])
    got = check(ctx, icol(a2), fcol(b2, [0, 0, 0, 1, 0]), 5, R.ROWS, direct=True)
    assert host(got[5]).tolist() == [[1, 0, 1], [1, 1, 1]] and host(got[3]).tolist() == [0, 1]


def test_nan_and_null_key_cells_are_one_missing_label(ctx):
    rng = np.random.default_rng(7)
    n = TILE + 9
    a = rng.integers(0, 5, n).astype(np.float64)
    a[rng.random(n) < 0.2] = np.nan
    a[rng.random(n) < 0.05] = -np.nan
    b = rng.integers(0, 4, n).astype(np.float64)
    b[rng.random(n) < 0.2] = np.nan
    na, nb = rng.random(n) < 0.2, rng.random(n) < 0.2
    val = R.make_values(rng, n, R.F64, 0.1, special=True)
    for op in R.OPS:
        got = check(ctx, fcol(a, na), fcol(b, nb), n, op, None if op == R.ROWS else val, direct=True)
        assert host(got[1]).tolist() == [0] * 5 + [1] and host(got[3]).tolist() == [0] * 4 + [1]
        assert got[6]["index_missing_rows"] == int((na | np.isnan(a)).sum())
    # every key cell missing
    got = check(ctx, fcol(np.full(70, np.nan)), icol(np.zeros(70), np.ones(70, bool)), 70, R.COUNT, icol(np.arange(70)), direct=True)
    assert host(got[5]).tolist() == [[70]] and host(got[1]).tolist() == [1] and host(got[3]).tolist() == [1]


def test_f64_keys_off_the_direct_path(ctx):
    rng = np.random.default_rng(8)
    n = 700
    b = icol(rng.integers(0, 3, n))
    val = fcol(rng.normal(0, 1, n))
    zeros = np.where(rng.random(n) < 0.5, -0.0, 0.0)
    got = check(ctx, fcol(zeros), b, n, R.MAX, val, direct=False)             # -0.0 and 0.0 are two labels, -0.0 first
    assert host(got[0]).view(np.uint64).tolist() == [1 << 63, 0]
    check(ctx, fcol(rng.integers(0, 4, n) + 0.5), b, n, R.SUM, val, direct=False)
    check(ctx, b, fcol(np.where(rng.random(n) < 0.5, 2.0 ** 53 + 2, 1.0)), n, R.ROWS, direct=False)
    check(ctx, fcol(np.where(rng.random(n) < 0.3, np.inf, np.where(rng.random(n) < 0.5, -np.inf, 1.0))), b, n, R.MIN, val, direct=False)
    nan_too = rng.normal(0, 1, n).round(1)
    nan_too[rng.random(n) < 0.2] = np.nan
    for op in R.OPS:                                                          # NaN and null key cells through the general path
        check(ctx, fcol(nan_too, rng.random(n) < 0.2), fcol(nan_too[::-1].copy(), rng.random(n) < 0.1), n, op, None if op == R.ROWS else val, direct=False)


def test_i64_keys_at_both_ends_of_the_range(ctx):
    rng = np.random.default_rng(9)
    n = 500
    val = icol(rng.integers(-9, 9, n))
    lo, hi = I64_MIN + rng.integers(0, 5, n), I64_MAX - rng.integers(0, 7, n)
    for op in (R.ROWS, R.SUM, R.LAST):
        check(ctx, icol(lo), icol(hi), n, op, None if op == R.ROWS else val, direct=True)
    both = np.where(rng.random(n) < 0.5, I64_MIN, I64_MAX)                   # the span is 2^64 - 1: no table, and nothing wraps
    got = check(ctx, icol(both), icol(hi), n, R.MAX, val, direct=False)
    assert host(got[0]).view(np.int64).tolist() == [I64_MIN, I64_MAX]
    big = icol(np.where(rng.random(n) < 0.5, I64_MAX, I64_MIN))               # I64 values at the sentinels: Min / Max answer 0.0
    check(ctx, icol(lo), icol(hi), n, R.MIN, big, direct=True)
    check(ctx, icol(lo), icol(hi), n, R.MAX, big, direct=True)
    check(ctx, icol(lo), icol(hi), n, R.SUM, big, direct=True)                # the int64 sum wraps on both paths alike


# ---- LAST -------------------------------------------------------------------------------------------------------------------------
def test_last_row_wins_across_workgroups(ctx):
    rng = np.random.default_rng(10)
    n = 3 * TILE
    a, b = rng.integers(0, 4, n), rng.integers(0, 4, n)
    a[:TILE], b[:TILE] = np.where(a[:TILE] == 3, 0, a[:TILE]), b[:TILE]       # pair (3, *) first appears in a later tile
    a[5], b[5] = 2, 2
    a[n - 1], b[n - 1] = 2, 2                                                 # the winner's row lies two tiles after the pair's first row
    val = np.arange(n, dtype=np.float64)
    got = check(ctx, icol(a), icol(b), n, R.LAST, fcol(val), direct=True)
    assert host(got[4])[2, 2] == float(n - 1)
    nulls = np.zeros(n, bool)
    nulls[n - 1] = True                                                       # the last row's value cell is null: 0.0, not the row before
    got = check(ctx, icol(a), icol(b), n, R.LAST, fcol(val, nulls), direct=True)
    assert host(got[4])[2, 2] == 0.0
    check(ctx, icol(a), icol(b), n, R.LAST, icol(np.arange(n)[::-1].copy(), nulls), direct=True)


# ---- limits and errors ------------------------------------------------------------------------------------------------------------
def test_too_many_cells_is_operation_failed_and_the_context_goes_on(ctx):
    import pandrs_amd as pa
    side = int(math.isqrt(MAX_CELLS)) + 2
    assert side == 4098 and side * side > MAX_CELLS >= (side - 2) * (side - 2)
    n = 2 * side
    a = np.concatenate([np.arange(side), np.zeros(side, np.int64)])
    b = np.concatenate([np.zeros(side, np.int64), np.arange(side)])
    info = L.PivotInfo()
    import ctypes as C
    cols = (L.Column * 2)()
    keep = [np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)]
    for i in range(2):
        cols[i].data, cols[i].dtype = keep[i].ctypes.data, L.I64
    at = lambda i: C.cast(C.byref(cols, i * C.sizeof(L.Column)), C.POINTER(L.Column))        # noqa: E731
    st = ctx.lib.pandrs_hip_pivot(ctx.h, L.MEM_HOST, at(0), None, 0, at(1), None, 0, None, n, L.PIVOT_ROWS, C.byref(info))
    assert st == L.ERR_OPERATION_FAILED and "pivot_max_cells" in L.last_error()
    assert (info.n_index_labels, info.n_column_labels, info.path, info.n_cells_present) == (side, side, 2, 0)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.pivot_fetch(side, side)                                           # nothing is retained
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "retained" in str(e.value)
    with pytest.raises(pa.OperationFailed):
        ctx.pivot(icol(a), icol(b), n, R.SUM, fcol(np.ones(n)))
    got = check(ctx, icol(a[side - 40:side + 40]), icol(b[side - 40:side + 40]), 80, R.ROWS, direct=False)     # a normal call afterwards
    assert got[6]["n_index_labels"] == 41 and got[6]["n_column_labels"] == 40 and got[6]["n_cells_present"] == 80
    # a code the rank table does not cover: found on the device, no fault
    codes = (np.array([0, 1, 5, 2], np.uint32), None, L.U32CODE)
    for option in (1, 2):
        ctx.set_option("pivot_path", option)
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.pivot(codes, icol([1, 2, 3, 4]), 4, R.ROWS, index_rank=np.arange(5, dtype=np.uint32))
        assert e.value.status == L.ERR_INVALID_ARGUMENT and ">= n_codes" in str(e.value)
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.pivot(icol([1, 2, 3, 4]), codes, 4, R.ROWS, columns_rank=np.arange(5, dtype=np.uint32))
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "columns" in str(e.value)
    ctx.set_option("pivot_path", 0)
    check(ctx, codes, icol([1, 2, 3, 4]), 4, R.ROWS, r1=np.arange(6, dtype=np.uint32)[::-1].copy(), direct=True)


CHILD = r"""
import ctypes as C, numpy as np, sys, torch
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=1 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
a = (torch.arange(1000, dtype=torch.int64, device="cuda:0") %% 7, None, L.I64)
b = (torch.arange(1000, dtype=torch.int64, device="cuda:0") %% 5, None, L.I64)
try:
    c.pivot(a, b, 1000, L.PIVOT_ROWS)            # the census blocks and the table: an arena asks for 1 MB more than it needs
    raise SystemExit("no error under a 1 MiB memory_limit")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
c.close()
cfg.memory_limit = 24 << 20
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
out = c.pivot(a, b, 1000, L.PIVOT_ROWS)          # fits
assert out[0].tolist() == list(range(7)) and int(out[5].sum()) == 1000 and out[6]["path"] == 1
n = 3000                                         # 3000 x 3000 cells of 16 bytes: the dense result does not fit
wide = (torch.arange(n, dtype=torch.int64, device="cuda:0") * 3, None, L.I64)
assert 16 * n * n > cfg.memory_limit
try:
    c.pivot(wide, wide, n, L.PIVOT_ROWS)
    raise SystemExit("no error under memory_limit (general path)")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
out = c.pivot(a, b, 1000, L.PIVOT_SUM, a)        # the context serves the next call
assert int(out[5].sum()) == 1000 and out[6]["n_cells_present"] == 35
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
try:
    c.pivot(a, b, 1000, L.PIVOT_ROWS)
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


# ---- buffers and retained state ---------------------------------------------------------------------------------------------------
def test_buffers_fetches_and_retained_state(ctx):
    import ctypes as C
    import torch
    import pandrs_amd as pa
    rng = np.random.default_rng(12)
    n = 2 * TILE + 19
    k1, r1 = R.make_key(rng, n, "i64", 6, 0.1)
    k2, r2 = R.make_key(rng, n, "code_rank", 8, 0.1)
    v = R.make_values(rng, n, R.F64, 0.1)
    shifted = dev(np.concatenate([k1[0][:1], k1[0]]))[1:]                     # the data pointer 8 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 == 8
    device = tuple((dev(c[0]), dev(c[1]), c[2]) for c in (k1, k2, v))
    resident = [ctx.upload_column(c[0], c[1], c[2]) for c in (k1, k2, v)]
    try:
        for cols in (None, device, ((shifted, device[0][1], L.I64), device[1], device[2]), tuple(resident)):
            for out_device in (False, True):
                for op in (R.ROWS, R.MEAN, R.LAST):
                    check(ctx, k1, k2, n, op, None if op == R.ROWS else v, r1, r2, out_device=out_device, direct=True,
                          cols=None if cols is None else cols[:2] + ((None,) if op == R.ROWS else (cols[2],)))
    finally:
        for r in resident:
            r.release()
    # fetch twice, into buffers with guard cells, with some pointers NULL, after another compute call
    want = ctx.pivot(k1, k2, n, R.SUM, v, index_rank=r1, columns_rank=r2)
    Rn, Cn = want[6]["n_index_labels"], want[6]["n_column_labels"]
    for out_device in (False, True):
        again = ctx.pivot_fetch(Rn, Cn, out_device)
        for a, b in zip(again, want[:6]):
            assert np.array_equal(host(a).view(np.uint8), host(b).view(np.uint8))
        guard = 5
        if out_device:
            bufs = [torch.full((k + guard,), 7, dtype=t, device="cuda:0") for k, t in
                    ((Rn, torch.int64), (Rn, torch.uint8), (Cn, torch.int64), (Cn, torch.uint8), (Rn * Cn, torch.float64), (Rn * Cn, torch.int64))]
            ptrs = [b.data_ptr() for b in bufs]
            torch.cuda.synchronize()                                          # the fills are torch's, the copies the library's
        else:
            bufs = [np.full(k + guard, 7, t) for k, t in ((Rn, np.uint64), (Rn, np.uint8), (Cn, np.uint64), (Cn, np.uint8), (Rn * Cn, np.float64), (Rn * Cn, np.int64))]
            ptrs = [b.ctypes.data for b in bufs]
        assert ctx.lib.pandrs_hip_pivot_fetch(ctx.h, L.MEM_DEVICE if out_device else L.MEM_HOST, *ptrs) == 0
        for b, w in zip(bufs, want[:6]):
            b, w = host(b), host(w).reshape(-1)
            assert (b[w.size:] == 7).all() and np.array_equal(b[:w.size].view(np.uint8), w.view(np.uint8))
    only_rows = ctx.pivot_fetch(Rn, Cn, labels=False, cells=False)
    assert only_rows[:5] == (None,) * 5 and np.array_equal(only_rows[5], want[5])
    assert ctx.lib.pandrs_hip_pivot_fetch(ctx.h, L.MEM_HOST, None, None, None, None, None, None) == 0
    ctx.column_stats((v[0], None, L.F64), n)                                  # another compute call
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.pivot_fetch(Rn, Cn)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "retained" in str(e.value)
    fresh = pa.Context(0)
    try:
        with pytest.raises(pa.PandrsHipError) as e:
            fresh.pivot_fetch(1, 1)                                           # no compute call at all
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        out = fresh.pivot(icol([]), icol([]), 0, R.ROWS)
        assert out[0].size == 0 and out[4].shape == (0, 0) and all(out[6][q] == 0 for q in out[6])
        assert [a.size for a in fresh.pivot_fetch(0, 0)] == [0] * 6          # an empty result is a result
    finally:
        fresh.close()
    del device, shifted
    torch.cuda.empty_cache()


def test_groupby_before_and_after_a_pivot_call(ctx):
    """A GroupBy's retained grouping and a groupby_agg's answers around pivot calls on the same context (both paths)."""
    import pandrs_amd.frame as F
    rng = np.random.default_rng(13)
    n = 20_000
    key = rng.integers(0, 37, n)
    other = rng.integers(0, 11, n)
    val = rng.integers(-5, 6, n).astype(np.float64)
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column(key))
    df.add_column("o", F.Int64Column(other))
    df.add_column("v", F.Float64Column(val))
    want = np.empty(n)
    for g in np.unique(key):
        rows = np.flatnonzero(key == g)
        want[rows] = np.cumsum(val[rows])
    sums = {str(g): float(val[key == g].sum()) for g in np.unique(key)}

    def group_sums():
        out = df.group_by(["k"]).aggregate([("v", F.AggregateOp.Sum, "s")])
        k = out.column("k")
        names = k.to_list() if hasattr(k, "to_list") else [str(int(x)) for x in k.data]
        return dict(zip(names, out.column("s").data.tolist()))

    gb = df.group_by(["k"])
    assert gb.cumsum("v") == want.tolist() and group_sums() == sums
    shared = F.get_context()
    try:
        for option in (1, 2):
            shared.set_option("pivot_path", option)
            out = shared.pivot(icol(key), icol(other), n, R.SUM, fcol(val))
            assert out[6]["path"] == option and int(out[5].sum()) == n
            assert gb.cumsum("v") == want.tolist(), option                    # the grouping of groupby_indices stays
            assert group_sums() == sums, option
            table = df.pivot_table("k", "o", "v", "sum")
            assert table.row_count() == 37 and group_sums() == sums
    finally:
        shared.set_option("pivot_path", 0)


# ---- the randomised sweep ---------------------------------------------------------------------------------------------------------
def test_random_sweep(ctx):
    """About 200 small cases drawn over the axes above (key kinds, rows, distinct values, offsets, nulls, NaNs, fractions, op,
    values dtype and masks, rank tables), each through both options against the twin.  No case is skipped."""
    rng = np.random.default_rng(20261021)
    ran = 0
    for case in range(200):
        n = int(rng.choice([1, 2, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, int(rng.integers(1, 3 * TILE))]))
        op = int(rng.integers(0, 7))
        keys = []
        for _ in range(2):
            kind = R.KEY_KINDS[int(rng.integers(0, 5))]
            card = int(rng.choice([1, 2, 3, 17, 63, 64, 300, 5000]))
            base = int(rng.choice([0, -5, 1 << 40])) if kind == "f64" else int(rng.choice([0, -5, I64_MIN, I64_MAX - card + 1, 1 << 53]))
            (data, mask, dt), rank = R.make_key(rng, n, kind, card, float(rng.choice([0.0, 0.05, 0.5, 1.0])) if rng.random() < 0.5 else 0.0,
                                                float(rng.choice([0.0, 0.3])), base=base if kind in ("i64", "f64") else 0)
            if kind == "f64" and rng.random() < 0.3:
                data[rng.random(n) < 0.3] = rng.choice([0.5, -0.0, math.inf, 2.0 ** 53 + 2])
            keys.append(((data, mask, dt), rank))
        v = None if op == R.ROWS else R.make_values(rng, n, int(rng.integers(0, 2)), float(rng.choice([0.0, 0.2, 1.0])), special=rng.random() < 0.5)
        check(ctx, keys[0][0], keys[1][0], n, op, v, keys[0][1], keys[1][1])
        ran += 1
    assert ran == 200


# ---- repeatability ----------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_stale_workspace(ctx):
    import pandrs_amd as pa
    rng = np.random.default_rng(11)
    n = 3 * TILE + 77
    k1, r1 = R.make_key(rng, n, "f64", 30, 0.1, 0.1, base=-7)
    k2, r2 = R.make_key(rng, n, "code_rank", 40, 0.1)
    k3 = fcol(rng.normal(0, 3, n).round(1), rng.random(n) < 0.1)
    vi = R.make_values(rng, n, R.I64, 0.1)
    vf = fcol(rng.integers(-1000, 1000, n) / 8.0, rng.random(n) < 0.1)       # sums of these are exact in any order

    def run():
        out = []
        for option in (1, 2):
            ctx.set_option("pivot_path", option)
            for op in R.OPS:
                for a, b, ra, rb in ((k1, k2, r1, r2), (k3, k2, None, r2)):
                    for v in ((None,) if op == R.ROWS else (vi, vf)):
                        got = ctx.pivot(a, b, n, op, v, index_rank=ra, columns_rank=rb)
                        out.extend([x.view(np.uint8) for x in got[:6]] + [np.array([got[6][q] for q in sorted(got[6]) if q != "path"])])
        ctx.set_option("pivot_path", 0)
        return out

    plain = run()
    half = len(plain) // 2
    assert all(np.array_equal(a, b) for a, b in zip(plain[:half], plain[half:]))       # the direct path's results are the general path's
    try:
        for fill in (0x00, 0xFF, 0xA5):
            before = pa.Context.workspace_poisoned_bytes()
            pa.Context.poison_workspace(fill)
            got = run()
            assert all(np.array_equal(a, b) for a, b in zip(plain, got)), fill
            assert pa.Context.workspace_poisoned_bytes() > before, fill
    finally:
        pa.Context.poison_workspace(None)
        ctx.set_option("pivot_path", 0)


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------
def test_frame_methods_end_to_end(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(14)
    n = 30_000
    words = ["w%02d" % j for j in rng.permutation(40)] + ["", "Z", "é"]
    s = [words[j] for j in rng.integers(0, len(words), n)]
    i = rng.integers(-3, 9, n)
    x = rng.integers(1, 4000, n) / 8.0                                        # no NaN, inf or zero: the reference's folds are the engine's
    df = F.OptimizedDataFrame()
    df.add_column("s", F.StringColumn(s))
    df.add_column("i", F.Int64Column(i))
    df.add_column("x", F.Float64Column(x))
    df.add_column("flag", F.BooleanColumn(i % 3 == 0))
    si = [str(v) for v in i.tolist()]
    sf = ["true" if v else "false" for v in (i % 3 == 0).tolist()]

    def columns_of(frame, index):
        assert frame.column_names[0] == index
        return frame.column(index).to_list(), {name: frame.column(name) for name in frame.column_names[1:]}

    for a, sa, b, sb in (("s", s, "i", si), ("i", si, "s", s), ("flag", sf, "i", si)):
        u1, u2, table = R.crosstab_loop(sa, sb)
        labels, cols = columns_of(df.crosstab(a, b), a)
        assert labels == u1 and list(cols) == u2
        for name in u2:
            assert cols[name].null_mask is None and cols[name].data.tolist() == table[name]
        ui, uc, want = R.unstack_loop(sa, sb, x.tolist())
        for frame in (df.unstack(a, b, "x"), df.pivot(a, b, "x")):
            labels, cols = columns_of(frame, a)
            assert labels == ui and list(cols) == uc
            for name in uc:
                np.testing.assert_array_equal(cols[name].data, np.array(want[name]))
                assert cols[name].null_mask is None
        for fn in ("sum", "mean", "min", "max", "count"):
            il, cl, want = R.pivot_table_loop(sa, sb, x.tolist(), fn)
            labels, cols = columns_of(df.pivot_table(a, b, "x", F.AggFunction.from_str(fn)), a)
            assert labels == il and list(cols) == cl
            for name in cl:
                col = cols[name]
                got = [None if col.is_null(r) else float(col.data[r]) for r in range(col.len())]
                if fn in ("sum", "mean"):                                     # eighths below 2^53: exact in any order
                    assert got == want[name], (fn, name)
                else:
                    assert got == want[name], (fn, name)


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(ctx):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pivot_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "pivot_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.search(r"\b[1-9]\d* tests, 0 failed checks", r.stdout), r.stdout


# ---- the code object --------------------------------------------------------------------------------------------------------------
def test_no_kernel_of_pivot_hip_uses_scratch():
    """pivot.hip compiled with the Makefile's flags: every kernel's code object metadata reports a private segment of 0 bytes
    and no spilled register."""
    csrc = os.path.join(ROOT, "pandrs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "pivot.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, "pivot.hip"), "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    kernels = re.findall(r"\.name:\s+(\S*pv_\w*kernel\S*)", text)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    assert len(kernels) >= 16 and len(sizes) == len(kernels) == len(spills), (len(kernels), len(sizes))
    assert all(s == 0 for s in sizes) and all(s == 0 for s in spills), list(zip(kernels, sizes, spills))
