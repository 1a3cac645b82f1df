"""pandrs_hip_predicate / pandrs_hip_isin and the mirrors' gt / ge / lt / le / eq_value / ne_value / between / is_between / isna /
notna / is_finite / is_infinite / isin / isin_numeric / query_* / dropna / count_na (reference
src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46, functions.rs:141-158, :253-257, :4141-4161) against
tests/predicate_ref.py.  Every result is a bitmap and a count: every comparison is bit for bit and count for count, no tolerance
anywhere in this file.  isin runs through the LDS set ("isin_path" 1) and the global set (2) wherever both apply: they must agree
with the restatement, hence with each other."""
import ctypes as C
import gc
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
from tests import predicate_ref as R  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"predicate_tile_rows = (\d+)", HEADER).group(1))
LDS_MAX = int(re.search(r"isin_lds_max_values = (\d+)", HEADER).group(1))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000123))[0]
ALL_ONES = struct.unpack("<d", struct.pack("<Q", 0xFFFFFFFFFFFFFFFF))[0]
EPS = 2.0 ** -52
ARGS = [(1.0, 3.0), (3.0, 1.0), (0.0, 0.0), (math.inf, math.inf), (-math.inf, 2.0 ** 53), (math.nan, 1.0), (2.0 ** 53, math.nan)]
assert [L.PRED_GT, L.PRED_IS_INFINITE, L.I64, L.F64, L.U32CODE] == [R.GT, R.IS_INFINITE, R.I64, R.F64, R.U32CODE]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.set_option("isin_path", 0)
    c.set_option("predicate_path", 0)
    c.close()


def full_grid():
    import torch
    return int(re.search(r"predicate_blocks_per_cu = (\d+)", HEADER).group(1)) * torch.cuda.get_device_properties(0).multi_processor_count


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def host(b):
    return b if isinstance(b, np.ndarray) else b.cpu().numpy()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint32, np.uint64):                                   # (the bytes are what travels)
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(a).to("cuda:0")


def f64_specials(n, seed=0):
    """n cells cycling through the special values, then shuffled: NaN with two payloads (and the all-ones pattern), +-inf, +-0.0,
    denormals, neighbours of 1.0 one EPSILON apart, 2^53 and its neighbour."""
    base = np.array([math.nan, NAN_B, ALL_ONES, math.inf, -math.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, 1.0 + EPS,
                     1.0 - EPS / 2, 2.0, 3.0, -1.0, 1e308, -1e308, 2.0 ** 53, 2.0 ** 53 + 2])
    x = np.resize(base, n)
    np.random.default_rng(seed).shuffle(x)
    return x


def i64_specials(n, seed=0):
    base = np.array([0, 1, -1, 2, 3, 2 ** 53, 2 ** 53 + 1, -2 ** 53, -(2 ** 53 + 1), 2 ** 53 + 2, I64_MIN, I64_MAX, I64_MAX - 1, 7], np.int64)
    x = np.resize(base, n)
    np.random.default_rng(seed).shuffle(x)
    return x


def check_pred(ctx, x, nulls=None, ops=R.OPS, args=ARGS[:2], col=None, out_device=False):
    """Every op with every argument pair against the restatement; `col` overrides how the column is passed."""
    x = np.asarray(x)
    n = x.shape[0]
    mask = None if nulls is None else bits(nulls)
    col = col if col is not None else (x, mask, L.I64 if x.dtype == np.int64 else L.F64)
    for op in ops:
        for a, b in (args if op < R.ISNA else args[:1]):
            want, count = R.predicate(x, mask, op, a, b)
            got, cnt = ctx.predicate(col, n, op, a, b, out_device=out_device)
            got = host(got)
            assert cnt == count and got.shape == want.shape, (R.OP_NAMES[op], n, a, b, cnt, count)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (R.OP_NAMES[op], n, a, b, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- row counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check_pred(ctx, rng.normal(2.0, 2.0, n))
    check_pred(ctx, rng.integers(-3, 6, n), rng.random(n) < 0.1)
    vals = np.array([1.0, 3.0, -2.0])
    for path in (1, 2):
        ctx.set_option("isin_path", path)
        try:
            x = rng.integers(-3, 6, n).astype(np.float64)
            for negate in (False, True):
                got, cnt = ctx.isin((x, None, L.F64), n, (vals, None, L.F64), negate, out_device=False)
                want, count = R.isin(x, None, R.F64, vals, R.F64, negate)
                assert cnt == count and np.array_equal(got, want), (n, path, negate)
        finally:
            ctx.set_option("isin_path", 0)


def test_more_tiles_than_workgroups(ctx):
    n = full_grid() * TILE + 77                                            # every workgroup loops, one of them once more
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.01] = np.nan
    nulls = rng.random(n) < 0.01
    check_pred(ctx, x, nulls, ops=(R.GT, R.BETWEEN, R.ISNA, R.NE), args=[(-0.5, 0.5)])
    check_pred(ctx, rng.integers(-100, 100, n), None, ops=(R.LE, R.EQ), args=[(7.0, 0.0)], out_device=True)
    vals = rng.integers(-50, 50, 300).astype(np.float64)
    xi = rng.integers(-100, 100, n)
    got, cnt = ctx.isin((xi, bits(nulls), L.I64), n, (vals, None, L.F64), out_device=False)
    want, count = R.isin(xi, bits(nulls), R.I64, vals, R.F64)
    assert cnt == count and np.array_equal(got, want)


# ---- ops, dtypes, memory spaces -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls_pct", [0, 10, 100])
def test_every_op_on_special_values(ctx, nulls_pct):
    n = TILE + 333
    rng = np.random.default_rng(nulls_pct)
    nulls = None if nulls_pct == 0 else rng.random(n) < nulls_pct / 100.0
    check_pred(ctx, f64_specials(n, 1), nulls, args=ARGS)
    check_pred(ctx, i64_specials(n, 2), nulls, args=ARGS + [(9.223372036854775807e18, 0.0), (-9.223372036854775808e18, 2.0 ** 53)])


def test_i64_interval_and_per_row_conversion_agree(ctx):
    """The I64 compare as integers against the bisected interval (the default) and with (double)v per row ("predicate_path" 1):
    both against the restatement, on the values where the conversion rounds."""
    n = TILE + 77
    edges = np.array([I64_MAX, I64_MAX - 511, I64_MAX - 512, I64_MAX - 513, I64_MIN, I64_MIN + 512, I64_MIN + 513, 2 ** 53 - 1], np.int64)
    x = np.concatenate([i64_specials(n - 3 * edges.shape[0], 9), edges, edges, edges])
    nulls = np.random.default_rng(9).random(n) < 0.1
    args = ARGS + [(9.223372036854775807e18, 0.0), (-9.223372036854775808e18, 2.0 ** 53), (9.223372036854774784e18, 9.3e18),
                   (2.0 ** 53 + 2, 9.3e18), (-9.3e18, -9.2e18), (0.5, 2.5), (1e300, -1e300)]
    try:
        for path in (0, 1):
            ctx.set_option("predicate_path", path)
            check_pred(ctx, x, nulls, args=args)
            check_pred(ctx, x, None, args=args, out_device=True)
    finally:
        ctx.set_option("predicate_path", 0)


def test_memory_spaces_and_count_only(ctx):
    import torch
    n = 2 * TILE + 19
    rng = np.random.default_rng(5)
    for x in (f64_specials(n, 3), i64_specials(n, 4)):
        nulls = rng.random(n) < 0.1
        dt = L.I64 if x.dtype == np.int64 else L.F64
        device_col = (dev(x.view(np.int64)).view(torch.float64) if dt == L.F64 else dev(x), dev(bits(nulls)), dt)
        resident = ctx.upload_column(x, bits(nulls), dt)
        try:
            for col in ((x, bits(nulls), dt), device_col, resident):
                for out_device in (False, True):
                    check_pred(ctx, x, nulls, col=col, out_device=out_device, args=ARGS[:1])
            got, cnt = ctx.predicate(device_col, n, L.PRED_GT, 1.0)         # device in, device out by default
            assert got.is_cuda and got.dtype == torch.uint8 and got.numel() == (n + 7) // 8
            for col in ((x, bits(nulls), dt), device_col, resident):
                for op in R.OPS:
                    none, cnt = ctx.predicate(col, n, op, 1.0, 3.0, count_only=True)
                    assert none is None and cnt == R.predicate(x, bits(nulls), op, 1.0, 3.0)[1]
                vals = x[:50].copy()
                for vcol in ((vals, None, dt), (device_col[0][:50].clone(), None, dt)):
                    none, cnt = ctx.isin(col, n, vcol, count_only=True)
                    assert none is None and cnt == R.isin(x, bits(nulls), dt, vals, dt)[1]
                    for out_device in (False, True):
                        got, cnt = ctx.isin(col, n, vcol, True, out_device=out_device)
                        want, count = R.isin(x, bits(nulls), dt, vals, dt, True)
                        assert cnt == count and np.array_equal(host(got), want)
        finally:
            resident.release()


@pytest.mark.parametrize("n", [TILE + 13, 8 * 700, 61])
def test_output_at_any_byte_offset_with_guards(ctx, n):
    import torch
    rng = np.random.default_rng(n)
    x = rng.normal(0.0, 1.0, n)
    vals = x[::7].copy()
    nbytes = (n + 7) // 8
    want_p, count_p = R.predicate(x, None, R.GE, 0.0)
    want_i, count_i = R.isin(x, None, R.F64, vals, R.F64, True)
    assert n % 8 == 0 or want_i[-1] >> (n % 8) == 0                         # the tail bits of the restatement are zero
    for off in range(1, 8):
        for make in (lambda: np.full(nbytes + 16, 0xA5, np.uint8), lambda: torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")):
            for call, want, count in ((lambda o: ctx.predicate((x, None, L.F64), n, L.PRED_GE, 0.0, out=o), want_p, count_p),
                                      (lambda o: ctx.isin((x, None, L.F64), n, (vals, None, L.F64), True, out=o), want_i, count_i)):
                buf = make()
                got, cnt = call(buf[off:off + nbytes])
                whole = host(buf)
                assert cnt == count and np.array_equal(whole[off:off + nbytes], want) and np.array_equal(host(got), want), (n, off)
                assert (whole[:off] == 0xA5).all() and (whole[off + nbytes:] == 0xA5).all(), (n, off)


def test_values_at_the_edges(ctx):
    inf = np.array([math.inf, -math.inf, 1.0, math.nan] * 40)
    for a in (math.inf, -math.inf):                                          # inf - inf is NaN: neither equal nor unequal
        eq, n_eq = ctx.predicate((inf, None, L.F64), 160, L.PRED_EQ, a, out_device=False)
        ne, n_ne = ctx.predicate((inf, None, L.F64), 160, L.PRED_NE, a, out_device=False)
        assert n_eq == 0 and n_ne == 120
        sel = np.unpackbits(ne, count=160, bitorder="little").astype(bool)
        assert not sel[inf == a].any() and sel[inf != a].all()
        assert np.array_equal(eq, R.predicate(inf, None, R.EQ, a)[0]) and np.array_equal(ne, R.predicate(inf, None, R.NE, a)[0])
    big = np.array([2 ** 53 + 1, 2 ** 53, 2 ** 53 + 2, 2 ** 53 - 1] * 30, np.int64)
    got, cnt = ctx.predicate((big, None, L.I64), 120, L.PRED_EQ, 2.0 ** 53, out_device=False)
    assert cnt == 60 and np.array_equal(np.unpackbits(got, count=4, bitorder="little"), [1, 1, 0, 0])   # 2^53 + 1 is 2^53 as f64
    got, cnt = ctx.predicate((np.arange(500.0), None, L.F64), 500, L.PRED_BETWEEN, 300.0, 100.0, out_device=False)
    assert cnt == 0 and not got.any()                                        # a > b selects nothing
    for dt, data in ((L.U32CODE, np.arange(8, dtype=np.uint32)), (L.BOOLBITS, np.zeros(8, np.uint8)), (L.CELL64, np.arange(8, dtype=np.uint64))):
        import pandrs_amd as pa
        with pytest.raises(pa.ColumnTypeMismatch):
            ctx.predicate((data, None, dt), 8, L.PRED_GT, 1.0)


# ---- isin ---------------------------------------------------------------------------------------------------------------------------
def check_isin(ctx, x, nulls, dtype, vals, vdtype, paths=(1, 2), negates=(False, True), device=False):
    n = x.shape[0]
    mask = None if nulls is None else bits(nulls)
    col = (dev(x), None if mask is None else dev(mask), dtype) if device else (x, mask, dtype)
    vcol = (dev(vals), None, vdtype) if device and len(vals) else (vals, None, vdtype)
    try:
        for negate in negates:
            want, count = R.isin(x, mask, dtype, vals, vdtype, negate)
            for path in paths:
                ctx.set_option("isin_path", path)
                got, cnt = ctx.isin(col, n, vcol, negate, out_device=device)
                slots, which = ctx.timings()["table_slots"], ctx.timings()["n_partitions"]
                assert which == (2 if path == 2 or len(vals) > LDS_MAX else 1), (path, len(vals), which)
                assert slots >= 2 * len(vals) and slots & (slots - 1) == 0
                got = host(got)
                bad = np.flatnonzero(got != want)
                assert cnt == count and bad.size == 0, (len(vals), path, negate, cnt, count, bad[:5])
    finally:
        ctx.set_option("isin_path", 0)


@pytest.mark.parametrize("n_values", [0, 1, 2, LDS_MAX, LDS_MAX + 1])
def test_isin_set_sizes(ctx, n_values):
    n = 3 * TILE + 1
    rng = np.random.default_rng(n_values)
    pool = rng.integers(0, 1 << 62, 3 * LDS_MAX).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)      # random 64-bit patterns
    x = pool[rng.integers(0, pool.shape[0], n)].view(np.float64)
    vals = pool[:n_values].view(np.float64).copy()
    check_isin(ctx, x, rng.random(n) < 0.1, L.F64, vals, L.F64)
    xi = rng.integers(0, 3 * max(n_values, 2), n)
    check_isin(ctx, xi, None, L.I64, np.arange(n_values, dtype=np.float64), L.F64, negates=(False,))   # consecutive integral f64


def test_isin_a_million_values_against_two_million_rows(ctx):
    rng = np.random.default_rng(11)
    n, m = 2_000_000, 1_000_000
    vals = rng.integers(I64_MIN, I64_MAX, m)
    x = np.where(rng.random(n) < 0.5, vals[rng.integers(0, m, n)], rng.integers(I64_MIN, I64_MAX, n))
    check_isin(ctx, x, rng.random(n) < 0.05, L.I64, vals, L.I64, paths=(0, 2), device=True)
    check_isin(ctx, x.view(np.float64), None, L.F64, vals.view(np.float64), L.F64, paths=(1,), negates=(True,), device=True)


def test_isin_value_lists(ctx):
    n = TILE + 99
    rng = np.random.default_rng(13)
    x = f64_specials(n, 6)
    nulls = rng.random(n) < 0.1
    lists = [
        np.array([3.0, 3.0, 1.0, 3.0, 1.0] * 20),                             # duplicates
        np.array([ALL_ONES, 2.0]),                                            # the empty marker, listed (and a cell: f64_specials)
        np.array([ALL_ONES] * 3),
        np.array([2.0, 1e308]),                                               # ... not listed, but a cell
        np.array([-0.0]),                                                     # 0.0 cells do not match
        np.array([0.0]),
        np.array([math.nan]),                                                 # one payload of two
        np.array([NAN_B, math.nan]),
        np.unique(x.view(np.uint64)).view(np.float64),                        # every row matches (but the nulls)
        np.array([12345.678, -9.75]),                                         # none does
    ]
    for vals in lists:
        check_isin(ctx, x, nulls, L.F64, vals, L.F64)
        check_isin(ctx, x, None, L.F64, vals, L.F64)
    # keys that differ only above bit 40, and consecutive integral f64 values (equal low words)
    hi = (np.arange(1, 3001, dtype=np.uint64) << np.uint64(41)) | np.uint64(0x155)
    cells = hi[rng.integers(0, 3000, n)]
    check_isin(ctx, cells.view(np.int64), nulls, L.I64, hi[::3].view(np.int64).copy(), L.I64)
    ints = rng.integers(0, 6000, n).astype(np.float64)
    check_isin(ctx, ints, nulls, L.F64, np.arange(0.0, 3000.0), L.F64)
    check_isin(ctx, np.full(n, 7.0), nulls, L.F64, np.array([7.0]), L.F64)      # every row on one slot
    check_isin(ctx, np.full(n, 7.0), np.ones(n, bool), L.F64, np.array([7.0]), L.F64)   # all null: nothing, everything with negate


def test_isin_dtype_pairings(ctx):
    import pandrs_amd as pa
    n = TILE + 5
    rng = np.random.default_rng(17)
    nulls = rng.random(n) < 0.1
    xi = i64_specials(n, 8)
    check_isin(ctx, xi, nulls, L.I64, np.array([2.0 ** 53, -1.0, 9.223372036854775807e18, 0.5, -9.223372036854775808e18]), L.F64)
    check_isin(ctx, xi, nulls, L.I64, np.array([2 ** 53 + 1, I64_MIN, -1, 7, 7, I64_MAX - 1], np.int64), L.I64)   # ids beyond 2^53, exactly
    got, cnt = ctx.isin((np.array([2 ** 53, 2 ** 53 + 1] * 8, np.int64), None, L.I64), 16, (np.array([2 ** 53 + 1], np.int64), None, L.I64),
                        out_device=False)
    assert cnt == 8 and list(got) == [0xAA, 0xAA]
    codes = rng.integers(0, 500, n).astype(np.uint32)
    codes[::50] = 0xFFFFFFFF
    check_isin(ctx, codes, nulls, L.U32CODE, np.array([1, 499, 0xFFFFFFFF, 77, 77, 1000], np.uint32), L.U32CODE)
    check_isin(ctx, codes, nulls, L.U32CODE, np.arange(0, 500, 2, dtype=np.uint32), L.U32CODE, device=True)
    data = {L.I64: xi, L.F64: xi.astype(np.float64), L.U32CODE: codes, L.BOOLBITS: np.zeros(n, np.uint8), L.CELL64: xi.view(np.uint64)}
    ok = {(L.F64, L.F64), (L.I64, L.F64), (L.I64, L.I64), (L.U32CODE, L.U32CODE)}
    for cd in data:
        for vd in data:
            if (cd, vd) not in ok:
                with pytest.raises(pa.ColumnTypeMismatch):
                    ctx.isin((data[cd], None, cd), n, (data[vd][:8].copy(), None, vd))
    with pytest.raises(ValueError):
        ctx.isin((xi, None, L.I64), n, (xi[:8].copy(), bits(np.zeros(8, bool)), L.I64))
    lib = L.load()
    c, v = L.Column(), L.Column()
    c.data, c.dtype, v.data, v.null_mask, v.dtype = xi.ctypes.data, L.I64, xi.ctypes.data, xi.ctypes.data, L.I64
    out, cnt = np.zeros((n + 7) // 8, np.uint8), C.c_int64(0)
    assert lib.pandrs_hip_isin(ctx.h, L.MEM_HOST, C.byref(c), n, L.MEM_HOST, C.byref(v), 8, 0, L.MEM_HOST, out.ctypes.data,
                               C.byref(cnt)) == L.ERR_INVALID_ARGUMENT
    for fn in (lambda rows: lib.pandrs_hip_predicate(ctx.h, L.MEM_HOST, C.byref(c), rows, 0, 1.0, 0.0, L.MEM_HOST, out.ctypes.data, C.byref(cnt)),
               lambda rows: lib.pandrs_hip_isin(ctx.h, L.MEM_HOST, C.byref(c), rows, L.MEM_HOST, C.byref(c), 8, 0, L.MEM_HOST, out.ctypes.data,
                                                C.byref(cnt))):
        assert fn(1 << 32) == L.ERR_INVALID_ARGUMENT and "2^32" in L.last_error()
        assert fn(-1) == L.ERR_INVALID_ARGUMENT


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
n = 4_000_000                                                   # device column, device out_bits: nothing to stage
big = (torch.arange(n, dtype=torch.int64, device="cuda:0"), None, L.I64)
def refused(call):
    try:
        call()
        raise SystemExit("no error under memory_limit")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
m = 1_500_000                                                   # 2^22 slots of 8 bytes: 32 MB of table
assert 16 * m > cfg.memory_limit
vals = torch.arange(0, 2 * m, 2, dtype=torch.int64, device="cuda:0")
refused(lambda: c.isin(big, n, (vals, None, L.I64)))
refused(lambda: c.isin(big, n, (vals.cpu().numpy(), None, L.I64)))             # 12 MB to stage, and the table
refused(lambda: c.predicate((np.zeros(n), None, L.F64), n, L.PRED_GT, 0.0, out_device=True))   # 32 MB to stage
got, cnt = c.isin(big, n, (vals[:100_000], None, L.I64))        # 2^18 slots: 2 MB of table fits
assert cnt == 100_000 and int(got[0]) == 0x55
got, cnt = c.predicate(big, n, L.PRED_LT, 1000.0)               # the counter only
assert cnt == 1000
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
for call in (lambda: c.predicate((x, None, L.F64), 1000, L.PRED_GT, 3.0), lambda: c.isin((x, None, L.F64), 1000, (x[:3].copy(), None, L.F64))):
    try:
        call()
        raise SystemExit("no error below min_size_threshold")
    except pa.BelowThreshold as e:
        assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
for call in (lambda: df.gt("x", 3.0), lambda: df.count_na("x"), lambda: df.isin_numeric("x", [1.0]), lambda: df.query_gt("x", 3.0)):
    try:
        call()
        raise SystemExit("the frame did not raise below min_size_threshold")
    except pa.BelowThreshold:
        pass
y = np.arange(20_000, dtype=np.float64)
assert c.predicate((y, None, L.F64), 20_000, L.PRED_GE, 19_990.0, count_only=True)[1] == 10
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT,)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- the chain the masks were built for ----------------------------------------------------------------------------------------
def test_chain_predicate_filter_gather(ctx):
    import torch
    n = 5 * TILE + 321
    rng = np.random.default_rng(19)
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.05] = np.nan
    y = rng.integers(-1000, 1000, n)
    dx, dy = dev(x), dev(y)
    mask, count = ctx.predicate((dx, None, L.F64), n, L.PRED_GT, 0.25)
    assert mask.is_cuda
    idx, cnt = ctx.filter_indices((mask, None, L.BOOLBITS), n)
    sel = x > 0.25
    assert cnt == count == int(sel.sum()) and np.array_equal(idx.cpu().numpy(), np.flatnonzero(sel))
    assert np.array_equal(ctx.filter_gather((dx, None, L.F64), n, cnt), x[sel])
    assert np.array_equal(ctx.filter_gather((dy, None, L.I64), n, cnt), y[sel])
    vals = np.arange(-1000, 1000, 7)
    mask, count = ctx.isin((dy, None, L.I64), n, (dev(vals), None, L.I64))
    idx, cnt = ctx.filter_indices((mask, None, L.BOOLBITS), n)
    sel = np.isin(y, vals)
    assert cnt == count == int(sel.sum()) and np.array_equal(idx.cpu().numpy(), np.flatnonzero(sel))
    assert np.array_equal(ctx.filter_gather((dy, None, L.I64), n, cnt, out_device=True).cpu().numpy(), y[sel])
    del dx, dy, mask, idx
    torch.cuda.empty_cache()


def test_frame_methods(ctx):
    import pandrs_amd.frame as F
    n = 3 * TILE + 17
    rng = np.random.default_rng(23)
    a = rng.normal(3.0, 2.0, n)
    a[rng.random(n) < 0.1] = np.nan
    nulls = rng.random(n) < 0.05
    i = rng.integers(-5, 6, n)
    words = ["w%d" % k for k in rng.integers(0, 40, n)]
    df = F.OptimizedDataFrame()
    df.add_column("a", F.Float64Column.with_nulls(a, nulls))
    df.add_column("i", F.Int64Column(i))
    df.add_column("s", F.StringColumn(words))
    v = np.where(nulls, np.nan, a)
    with np.errstate(invalid="ignore"):
        assert df.gt("a", 3.0) == (v > 3.0).tolist() and df.le("a", 3.0) == (v <= 3.0).tolist()
        assert df.between("a", 2.0, 4.0) == ((v >= 2.0) & (v <= 4.0)).tolist()
        assert df.is_between("a", 2.0, 4.0, False) == ((v > 2.0) & (v < 4.0)).tolist()
    assert df.isna("a") == np.isnan(v).tolist() and df.notna("a") == (~np.isnan(v)).tolist()
    assert df.is_finite("a") == np.isfinite(v).tolist() and df.is_infinite("i") == [False] * n
    assert df.eq_value("i", 2.0) == (i == 2).tolist() and df.ne_value("i", 2.0) == (i != 2).tolist()
    assert df.count_na("a") == int(np.isnan(v).sum()) and df.has_nulls("a") and not df.has_nulls("i")
    assert df.count_value("i", -5.0) == int((i == -5).sum())
    assert df.isin_numeric("i", [1.0, -4.0, 2.5]) == np.isin(i, [1, -4]).tolist()
    listed = ["w3", "w17", "never seen in any column", "w39"]
    assert df.isin("s", listed) == [w in listed for w in words]
    assert df.isin("s", []) == [False] * n
    # query_gt / dropna: filter's frame (nulls become defaults, no masks), against numpy boolean indexing
    with np.errstate(invalid="ignore"):
        keep = v > 3.0
    q = df.query_gt("a", 3.0)
    assert q.row_count() == int(keep.sum()) and q.column_names == ["a", "i", "s"]
    assert np.array_equal(q.column("a").data, a[keep]) and np.array_equal(q.column("i").data, i[keep])
    assert q.column("s").to_list() == [w for w, k in zip(words, keep) if k]
    d = df.dropna("a")
    keep = ~np.isnan(v)
    assert d.row_count() == int(keep.sum()) and np.array_equal(d.column("a").data, a[keep]) and d.column("a").null_mask is None
    assert df.query_eq("i", 4.0).row_count() == int((i == 4).sum()) and df.query_lt("i", -100.0).row_count() == 0
    assert df.query_lt("i", -100.0).column_names == ["a", "i", "s"]


# ---- beyond 2^31 rows -------------------------------------------------------------------------------------------------------------
def test_rows_beyond_2_31(ctx):
    import torch
    n = (1 << 31) + 12345
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = n * 8 + 3 * (n // 8)                                               # the ramp, the bitmap and torch's temporaries over it
    if free < need * 1.2:
        pytest.skip("needs %.0f GB (+20 %%) of device memory, %.0f GB free" % (need / 1e9, free / 1e9))
    x = torch.arange(n, dtype=torch.int64, device="cuda:0")
    t = (1 << 31) - 5                                                         # rows t + 1 .. n - 1 are selected: a run across row 2^31
    got, cnt = ctx.predicate((x, None, L.I64), n, L.PRED_GT, float(t))
    del x
    nbytes = (n + 7) // 8
    assert cnt == n - 1 - t and got.numel() == nbytes
    b0 = (t + 1) // 8                                                         # the byte in which the run starts
    assert int(got[:b0].max()) == 0 and int(got[b0 + 1:nbytes - 1].min()) == 0xFF
    want = np.zeros(64, np.uint8)
    want[np.arange(64) + (b0 - 4) * 8 > t] = 1
    assert np.array_equal(got[b0 - 4:b0 + 4].cpu().numpy(), np.packbits(want, bitorder="little"))      # both sides of row 2^31
    assert int(got[nbytes - 1]) == (1 << (n % 8)) - 1                         # the tail: bits past n_rows are 0
    del got
    torch.cuda.empty_cache()


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(ctx):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "predicate_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "predicate_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
