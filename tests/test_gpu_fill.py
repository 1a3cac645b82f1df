"""pandrs_hip_fill and the mirrors' ffill / bfill / fillna_method / interpolate / fillna (reference
src/dataframe/pandas_compat/functions.rs:789-918, :3626-3683) against tests/fill_ref.py.  Every result is a copied cell or
one f64 expression of two cells and two integers, so every comparison is bit for bit (the uint64 view, NaN included): no
tolerance anywhere in this file."""
import ctypes as C
import json
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
from tests.fill_ref import BFILL, FFILL, I64_MAX, I64_MIN, LINEAR, METHODS, VALUE, bits, fill_loop, fill_twin, same_bits, sweep_cases  # noqa: E402

NAN = np.uint64(0x7FF8000000000000).view(np.float64)
HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
T = int(re.search(r"fill_tile_rows = (\d+)", HEADER).group(1))
PER_CU = int(re.search(r"fill_blocks_per_cu = (\d+)", HEADER).group(1))


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def default_value(x):
    return -42 if x.dtype == np.int64 else -1.5


def check(ctx, x, nulls=None, methods=METHODS, col=None, value=None, **kw):
    """One column under `methods` against the vectorised restatement: the cells, the mask, the count, and `mask is None`
    exactly when nothing is missing; `col` overrides how the column is passed."""
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    n = x.shape[0]
    col = col if col is not None else (x, None if nulls is None else bits(nulls), L.I64 if x.dtype == np.int64 else L.F64)
    for method in methods:
        v = (default_value(x) if value is None else value) if method == VALUE else None
        want, gone = fill_twin(x, nulls, method, v)
        vals, mask, missing = ctx.fill(col, n, method, v, **kw)
        if not isinstance(vals, np.ndarray):
            vals, mask = vals.cpu().numpy(), None if mask is None else mask.cpu().numpy()
        assert same_bits(vals, want), (method, n, np.flatnonzero(vals.view(np.uint64) != want.view(np.uint64))[:5])
        assert missing == int(gone.sum()), (method, missing, int(gone.sum()))
        assert (mask is None) == (missing == 0)
        if mask is not None:
            assert np.array_equal(mask, bits(gone)), method


def gaps(n, spans):
    miss = np.zeros(n, bool)
    for a, b in spans:
        miss[a:b] = True
    return miss


def both_dtypes(ctx, miss, **kw):
    """The layout `miss` as NaN cells, as null bits over finite cells, and as null bits of an I64 column."""
    n = miss.shape[0]
    rng = np.random.default_rng(n)
    x = rng.normal(0.0, 10.0, n)
    check(ctx, np.where(miss, np.nan, x), **kw)
    check(ctx, x, miss, **kw)
    check(ctx, rng.integers(-10**6, 10**6, n), miss, **kw)


# ---- row counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    both_dtypes(ctx, rng.random(n) < 0.4)
    check(ctx, rng.integers(-5, 5, n))                                    # I64 without a mask: nothing missing


def test_more_tiles_than_workgroups(ctx):
    import torch
    grid = PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    n = grid * T + T + 3                                                  # every workgroup loops, one of them twice more
    rng = np.random.default_rng(3)
    miss = rng.random(n) < 0.3
    miss[5 * T - 7:9 * T + 11] = True
    both_dtypes(ctx, miss)


# ---- gaps against tile and word edges ----------------------------------------------------------------------------------------
LAYOUTS = {
    "a gap ends on a tile's last row, the next starts on a tile's first": (3 * T, [(T - 5, T), (2 * T, 2 * T + 4)]),
    "a gap of 2 straddles a tile edge and a word edge": (2 * T + 9, [(T - 1, T + 1), (63, 65)]),
    "a gap covers 3 whole tiles and one row on each side": (6 * T, [(T - 1, 4 * T + 1)]),
    "a gap of exactly 64 aligned to a word": (T + 200, [(128, 192), (T, T + 64)]),
    "gaps of 1 alternate with valid rows": (2 * T + 3, [(i, i + 1) for i in range(0, 2 * T + 3, 2)]),
    "valid rows alternate with gaps of 1": (2 * T + 3, [(i, i + 1) for i in range(1, 2 * T + 3, 2)]),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_gaps_against_tile_and_word_edges(ctx, name):
    n, spans = LAYOUTS[name]
    both_dtypes(ctx, gaps(n, spans))


# ---- degenerate columns --------------------------------------------------------------------------------------------------------
def _only(n, *valid):
    miss = np.ones(n, bool)
    miss[list(valid)] = False
    return miss


DEGENERATE = {
    "all missing": _only(2 * T + 5),
    "none missing": np.zeros(2 * T + 5, bool),
    "only row 0 valid": _only(2 * T + 5, 0),
    "only the last row valid": _only(2 * T + 5, 2 * T + 4),
    "only row t valid": _only(3 * T, T),
    "row 0 missing, the first valid row in tile 2": gaps(4 * T, [(0, 2 * T + 17)]),
    "only rows 0 and the last valid": _only(3 * T + 1, 0, 3 * T),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_columns(ctx, name):
    both_dtypes(ctx, DEGENERATE[name])


def test_row_zero_is_not_mistaken_for_a_source(ctx):
    x = np.full(3 * T, np.nan)
    x[0], x[T] = 123.0, 7.0
    nulls = np.zeros(3 * T, bool)
    nulls[0] = True                                                       # row 0 holds a finite number under a null bit
    vals, mask, missing = ctx.fill((x, bits(nulls), L.F64), 3 * T, FFILL, out_device=False)
    assert np.isnan(vals[:T]).all() and (vals[T:] == 7.0).all() and missing == T
    check(ctx, x, nulls)


# ---- what is missing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.0, 0.1, 0.5, 1.0])
def test_null_bits_nan_cells_and_both(ctx, density):
    rng = np.random.default_rng(int(density * 100) + 20)
    n = 10_007
    x = rng.normal(0.0, 1.0, n)
    nan, nulls = rng.random(n) < density, rng.random(n) < density
    if density == 1.0:
        nan[:], nulls[:] = True, True
    xn = np.where(nan, np.nan, x)
    check(ctx, xn)                                                        # NaN only
    check(ctx, x, nulls)                                                  # null bit only, over finite numbers
    check(ctx, xn, nulls)                                                 # both, some on the same cell
    check(ctx, rng.integers(-99, 99, n), nulls)


def test_stray_mask_bits_past_the_last_row_are_ignored(ctx):
    rng = np.random.default_rng(31)
    n = 1003                                                              # n % 8 and n % 64 both non-zero
    x = rng.normal(0.0, 1.0, n)
    nulls = rng.random(n) < 0.2
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8
    check(ctx, x, nulls, col=(x, mask, L.F64))
    i = rng.integers(0, 9, n)
    check(ctx, i, nulls, col=(i, mask, L.I64))


# ---- values ----------------------------------------------------------------------------------------------------------------------
def test_special_f64_values_and_masked_nan_payloads(ctx):
    rng = np.random.default_rng(41)
    special = np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1.7976931348623157e308, -1.7976931348623157e308])
    n = 4 * T + 77
    x = special[rng.integers(0, len(special), n)]
    miss = rng.random(n) < 0.6
    xn = np.where(miss, np.nan, x)
    check(ctx, xn)                                                        # +-inf and -0.0 are valid; inf - inf inside gaps
    for v in (-0.0, np.inf, 5e-324, float("nan")):
        check(ctx, xn, methods=[VALUE], value=v)                          # a NaN fill leaves the rows missing
    pay = x.copy().view(np.uint64)
    pay[miss] = np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 52, int(miss.sum())).astype(np.uint64)
    pay[miss & (rng.random(n) < 0.5)] |= np.uint64(1 << 63)
    check(ctx, pay.view(np.float64), miss)                                # NaN payloads under null bits, and unmasked
    check(ctx, pay.view(np.float64))
    vals, mask, missing = ctx.fill((np.array([np.inf, np.nan, np.nan, -np.inf, np.nan]), None, L.F64), 5, LINEAR, out_device=False)
    assert np.isnan(vals[1:3]).all() and np.isnan(vals[4]) and missing == 1 and list(mask) == [0x10]      # inf - inf: bit 0


def test_int64_extremes_and_values_beyond_2_pow_53(ctx):
    rng = np.random.default_rng(51)
    special = np.array([I64_MIN, I64_MAX, 0, -1, 2**53 + 1, -(2**53) - 1, 2**62 + 12345, 2**63 - 1025], np.int64)
    n = 3 * T + 5
    x = special[rng.integers(0, len(special), n)]
    nulls = rng.random(n) < 0.5
    check(ctx, x, nulls)                                                  # FFILL / BFILL exact, LINEAR's cast and arithmetic
    check(ctx, x)                                                         # no mask: a copy, and LINEAR's conversion
    for v in (I64_MIN, I64_MAX, 0, 2**53 + 1):
        check(ctx, x, nulls, methods=[VALUE], value=v)
    vals, mask, missing = ctx.fill((np.array([2**53 + 1, 0, 0], np.int64), bits([0, 1, 1]), L.I64), 3, FFILL, out_device=False)
    assert vals.dtype == np.int64 and list(vals) == [2**53 + 1] * 3 and mask is None and missing == 0
    import pandrs_amd as pa
    for bad in (1.5, 2**63, None, True):
        with pytest.raises((ValueError, pa.PandrsHipError)):
            ctx.fill((x, None, L.I64), n, VALUE, bad)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def test_memory_spaces_offsets_and_guards(ctx):
    import torch
    rng = np.random.default_rng(71)
    n = 2 * T + 1003                                                      # n % 8 and n % 64 both non-zero
    nbytes = (n + 7) // 8
    x = rng.normal(0.0, 50.0, n)
    x[rng.random(n) < 0.2] = np.nan
    nulls = rng.random(n) < 0.3
    nulls[:70] = True
    nulls[-70:] = True                                                    # rows stay missing at both ends
    mask = bits(nulls)
    i = rng.integers(-1000, 1000, n)
    for data, dt in ((x, L.F64), (i, L.I64)):
        dx, dm = torch.from_numpy(data).cuda(), torch.from_numpy(mask).cuda()
        pad = torch.empty(n + 1, dtype=dx.dtype, device="cuda:0")        # rows start 8 bytes off a 16-byte boundary
        pad[1:] = dx
        assert pad.data_ptr() % 16 == 0
        res = ctx.upload_column(data, mask, dt)
        try:
            cols = [(data, mask, dt), (dx, dm, dt), res]
            for off in (1, 3, 7):                                         # the input mask at odd byte offsets
                padm = torch.empty(nbytes + off, dtype=torch.uint8, device="cuda:0")
                padm[off:] = dm
                cols.append((pad[1:], padm[off:], dt))
            for col in cols:
                check(ctx, data, nulls, col=col, out_device=False)        # host out
                check(ctx, data, nulls, col=col, out_device=True)         # device out
            for method in METHODS:
                v = default_value(data) if method == VALUE else None
                want, gone = fill_twin(data, nulls, method, v)
                out = np.full(n + 2, -7, want.dtype)                      # host outputs with guard cells and 64 guard bytes
                om = np.full(nbytes + 64, 0xAA, np.uint8)
                ctx.fill(res, n, method, v, out=out[:n], out_mask=om)
                assert same_bits(out[:n], want) and (out[n:] == -7).all()
                assert np.array_equal(om[:nbytes], bits(gone)) and (om[nbytes:] == 0xAA).all()
                dout = torch.full((n + 3,), -7, dtype=torch.int64 if want.dtype == np.int64 else torch.float64, device="cuda:0")
                dom = torch.full((nbytes + 1 + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
                vals, m, missing = ctx.fill((dx, dm, dt), n, method, v, out=dout[1:], out_mask=dom[1:])    # 8 / 1 bytes off
                assert same_bits(vals.cpu().numpy(), want) and (dout[0] == -7) and (dout[n + 1:] == -7).all()
                assert np.array_equal(dom[1:1 + nbytes].cpu().numpy(), bits(gone)) and (dom[0] == 0xAA) and (dom[1 + nbytes:] == 0xAA).all()
                assert missing == int(gone.sum()) > 0 or method == VALUE
        finally:
            res.release()
    vals, m, missing = ctx.fill((x, None, L.F64), n, VALUE, float("nan"), out_device=False)      # no output mask asked of the ABI
    lib, c = L.load(), L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out, cnt = np.full(n, -7.0), C.c_int64(-1)
    assert lib.pandrs_hip_fill(ctx.h, L.MEM_HOST, C.byref(c), n, FFILL, 0, L.MEM_HOST, out.ctypes.data, None, C.byref(cnt)) == 0
    want, gone = fill_twin(x, None, FFILL)
    assert same_bits(out, want) and cnt.value == int(gone.sum())
    assert lib.pandrs_hip_fill(ctx.h, L.MEM_HOST, C.byref(c), n, BFILL, 0, L.MEM_HOST, out.ctypes.data, None, None) == 0
    assert same_bits(out, fill_twin(x, None, BFILL)[0])


def test_timings(ctx):
    n = 3 * T
    x = np.where(np.arange(n) % 3 == 0, np.nan, 1.0)
    ctx.fill((x, None, L.F64), n, FFILL)
    t = ctx.timings()
    assert t["n_partitions"] == 0 and t["algorithmic_bytes"] == n * 8 + 2 * (n // 8) + 3 * 32 + n * 16 + n // 8
    ctx.fill((x, None, L.F64), n, VALUE, 0.0)
    assert ctx.timings()["algorithmic_bytes"] == n * 16 + n // 8


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import pandrs_amd as pa
    import torch
    x = np.arange(16, dtype=np.float64)
    col = (x, None, L.F64)
    for bad in (-1, 4, 99):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.fill(col, 16, bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, bad
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.fill((other, None, dt), 16, FFILL)
        assert e.value.status == L.ERR_TYPE_MISMATCH
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out, om, cnt = np.full(16, -7.0), np.full(2, 0xAA, np.uint8), C.c_int64(-1)

    def call(space=L.MEM_HOST, colp=C.byref(c), n=16, method=FFILL, out_space=L.MEM_HOST, o=out.ctypes.data, m=om.ctypes.data):
        return lib.pandrs_hip_fill(ctx.h, space, colp, n, method, 0, out_space, o, m, C.byref(cnt))
    assert call(colp=None) == L.ERR_INVALID_ARGUMENT
    assert call(o=None) == L.ERR_INVALID_ARGUMENT
    assert call(space=7) == L.ERR_INVALID_ARGUMENT and call(out_space=7) == L.ERR_INVALID_ARGUMENT
    assert call(n=1 << 32) == L.ERR_INVALID_ARGUMENT and call(n=-1) == L.ERR_INVALID_ARGUMENT
    nodata = L.Column()
    nodata.dtype = L.F64
    assert call(colp=C.byref(nodata)) == L.ERR_INVALID_ARGUMENT
    assert call(n=0) == 0 and cnt.value == 0
    assert (out == -7.0).all() and (om == 0xAA).all()                     # no error above, and n_rows == 0, wrote anything
    vals, mask, missing = ctx.fill(col, 0, LINEAR)
    assert vals.shape == (0,) and mask is None and missing == 0
    # an I64 result of a masked column cannot do without the output mask, except under VALUE
    i, im = np.arange(16), bits([1, 0] * 8)
    ci = L.Column()
    ci.data, ci.null_mask, ci.dtype = i.ctypes.data, im.ctypes.data, L.I64
    oi = np.zeros(16, np.int64)
    for method, want in ((FFILL, L.ERR_INVALID_ARGUMENT), (BFILL, L.ERR_INVALID_ARGUMENT), (LINEAR, 0), (VALUE, 0)):
        assert call(colp=C.byref(ci), method=method, o=oi.ctypes.data, m=None) == want, method
    ci.null_mask = None
    assert call(colp=C.byref(ci), method=FFILL, o=oi.ctypes.data, m=None) == 0 and list(oi) == list(range(16))
    # in place
    assert call(o=x.ctypes.data) == L.ERR_INVALID_ARGUMENT and call(o=x.ctypes.data + 8 * 15) == L.ERR_INVALID_ARGUMENT
    ci.null_mask = im.ctypes.data
    assert call(colp=C.byref(ci), o=oi.ctypes.data, m=im.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert "in place" in L.last_error()
    d = torch.arange(16, dtype=torch.float64, device="cuda:0")
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.fill((d, None, L.F64), 16, BFILL, out=d)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    vals, _, _ = ctx.fill((d, None, L.F64), 16, BFILL, out=torch.empty_like(d))          # a buffer of its own is fine
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
PER_ROW = 0.13                                                  # the documented workspace (pandrs_hip.h), bytes per row
n = 130_000_000                                                 # 16.9 MB of workspace, nothing to stage: device column, device outputs
assert PER_ROW * n > cfg.memory_limit
big = (torch.empty(n, dtype=torch.float64, device="cuda:0"), None, L.F64)
out, om = torch.empty(n, dtype=torch.float64, device="cuda:0"), torch.empty((n + 7) // 8, dtype=torch.uint8, device="cuda:0")
for method in (L.FILL_FFILL, L.FILL_LINEAR):
    try:
        c.fill(big, n, method, out=out, out_mask=om)
        raise SystemExit("no error under memory_limit")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
del big, out, om
try:
    c.fill((np.zeros(4_000_000), None, L.F64), 4_000_000, L.FILL_VALUE, 0.0)       # 32 MB to stage
    raise SystemExit("no error under memory_limit (staging)")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
k = 1_000_000                                                   # 0.13 MB: fits (an arena asks for 1 / 8 more and 1 MB)
x = torch.arange(k, dtype=torch.float64, device="cuda:0")
x[1::2] = float("nan")
v, m, missing = c.fill((x, None, L.F64), k, L.FILL_LINEAR)
assert missing == 1 and torch.equal(v[:-1], torch.arange(k - 1, dtype=torch.float64, device="cuda:0"))  # still works
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
try:
    c.fill((x, None, L.F64), 1000, L.FILL_FFILL)
    raise SystemExit("no error below min_size_threshold")
except pa.BelowThreshold as e:
    assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
try:
    df.ffill("x")
    raise SystemExit("the frame did not raise below min_size_threshold")
except pa.BelowThreshold:
    pass
y = np.arange(20_000, dtype=np.float64)
y[5] = np.nan
v, m, missing = c.fill((y, None, L.F64), 20_000, L.FILL_BFILL, out_device=False)
assert v[5] == 6.0 and m is None and missing == 0
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- mirrors and random cases ----------------------------------------------------------------------------------------------------
def test_frame_mirror_gives_the_known_answers(ctx):
    import pandrs_amd.frame as F
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "fill_known_answers.json")))
    for case in golden["cases"]:
        x = np.array([np.nan if v is None else v for v in case["input"]], np.float64)
        want = np.array([NAN if v is None else v for v in case["expected"]], np.float64)
        df = F.OptimizedDataFrame()
        df.add_column("id", F.Int64Column(np.arange(len(x))))
        df.add_column("a", F.Float64Column(x))
        df.add_column("s", F.StringColumn(["x"] * len(x)))
        calls = {"ffill": [lambda: df.ffill("a"), lambda: df.fillna_method("a", "ffill"), lambda: df.fillna_method("a", "forward")],
                 "bfill": [lambda: df.bfill("a"), lambda: df.fillna_method("a", "bfill"), lambda: df.fillna_method("a", "backward")],
                 "interpolate": [lambda: df.interpolate("a")], "fillna": [lambda: df.fillna("a", case["value"])]}[case["op"]]
        for call in calls:
            got = call()
            col = got.column("a")
            assert got is not df and got.column_names == ["id", "a", "s"] and isinstance(col, F.Float64Column), case["name"]
            assert same_bits(col.data, want), case["name"]
            gone = np.isnan(want)
            assert (col.null_mask is None) == (not gone.any()) and [col.is_null(k) for k in range(len(x))] == list(gone)
            assert got.column("id") is df.column("id") and got.column("s") is df.column("s")
            assert same_bits(df.column("a").data, x)                      # the source frame as it was
    with pytest.raises(F.InvalidValue) as e:
        df.fillna_method("a", golden["invalid_method"]["method"])
    assert str(e.value) == golden["invalid_method"]["message"]


def test_frame_mirror_on_int64_and_masked_columns(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(81)
    n = T + 301
    f, fn = rng.normal(0.0, 5.0, n), rng.random(n) < 0.3
    f[rng.random(n) < 0.1] = np.nan
    i, inn = rng.integers(-50, 50, n), rng.random(n) < 0.4
    inn[:3] = True
    df = F.OptimizedDataFrame()
    df.add_column("i", F.Int64Column.with_nulls(i, inn))
    df.add_column("f", F.Float64Column.with_nulls(f, fn))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    for name, data, nulls in (("i", i, inn), ("f", f, fn)):
        for method, call in ((FFILL, lambda: df.ffill(name)), (BFILL, lambda: df.bfill(name)), (LINEAR, lambda: df.interpolate(name)),
                             (VALUE, lambda: df.fillna(name, default_value(data)))):
            want, gone = fill_twin(data, nulls, method, default_value(data) if method == VALUE else None)
            col = call().column(name)
            assert isinstance(col, F.Int64Column if want.dtype == np.int64 else F.Float64Column)
            assert same_bits(col.data, want) and (col.null_mask is None) == (not gone.any())
            if gone.any():
                assert np.array_equal(col.null_mask, bits(gone))
    assert not df.fillna("f", 0.0).column("f").null_mask and df.ffill("i").column("i").is_null(0)
    with pytest.raises(F.ColumnTypeMismatch):
        df.interpolate("b")
    with pytest.raises(F.ColumnNotFound):
        df.bfill("nope")


def test_cpp_mirror_fills():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "fill_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "fill_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "3 tests, 0 failed checks" in r.stdout


def test_randomised_sweep(ctx):
    cases, seen = 0, set()
    for x, nulls, method, value in sweep_cases(np.random.default_rng(7), cases=300, tile=T):
        check(ctx, x, nulls, methods=[method], value=value)
        seen.add((method, x.dtype.name, nulls is not None))
        cases += 1
    assert cases == 300 and len(seen) >= 14, sorted(seen)
    for x, nulls, method, value in sweep_cases(np.random.default_rng(8), cases=12, tile=T):      # the line-for-line loop too
        want, gone = fill_loop(x, nulls, method, value)
        vals, mask, missing = ctx.fill((x, None if nulls is None else bits(nulls), L.I64 if x.dtype == np.int64 else L.F64), x.shape[0],
                                       method, value, out_device=False)
        assert same_bits(vals, want) and missing == int(gone.sum())
