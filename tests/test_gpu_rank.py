"""pandrs_hip_rank and the mirrors' rank (reference src/dataframe/pandas_compat/functions.rs:193-236) against
tests/rank_ref.py.  Every result is an integer or half-integer below 2^33, so every comparison is bit for bit (the uint64
view, NaN included): no tolerance anywhere in this file."""
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
from tests.rank_ref import AVERAGE, DENSE, FEATURES, FIRST, MAX, METHODS, MIN, rank_features, rank_ref_all, sweep_cases  # noqa: E402

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def geometry():
    """(sorted positions per workgroup iteration, workgroups of a full grid), from the entry point's documented geometry."""
    import torch
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    tile = int(re.search(r"rank_tile_rows = (\d+)", header).group(1))
    per_cu = int(re.search(r"rank_blocks_per_cu = (\d+)", header).group(1))
    return tile, per_cu * torch.cuda.get_device_properties(0).multi_processor_count


def tile_rows():
    return int(re.search(r"rank_tile_rows = (\d+)", open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()).group(1))


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(ctx, x, nulls=None, methods=METHODS, col=None, want=None):
    """The ranks of one column under `methods` against the restatement; `col` overrides how the column is passed.
    -> the restatement's five results (so that callers sharing an input compute it once)."""
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    n = x.shape[0]
    dtype = L.I64 if x.dtype == np.int64 else L.F64
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype)
    want = want if want is not None else rank_ref_all(x, nulls)
    for method in methods:
        got = ctx.rank(col, n, method, out_device=False)
        assert same_bits(got, want[method]), (method, n, np.flatnonzero(got.view(np.uint64) != want[method].view(np.uint64))[:5])
    return want


# ---- row counts ------------------------------------------------------------------------------------------------------------
def _counts():
    t = tile_rows()
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("n", _counts())
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, rng.integers(0, max(2, n // 3), n).astype(np.float64))
    check(ctx, rng.integers(-n, n + 1, n))


def test_more_tiles_than_workgroups(ctx):
    tile, grid = geometry()
    n = grid * tile + tile + 3                                            # every workgroup loops, one of them twice more
    rng = np.random.default_rng(3)
    check(ctx, rng.integers(0, 50_000, n).astype(np.float64))
    check(ctx, rng.integers(-40, 40, n))                                  # runs far longer than a tile


# ---- tie runs against tile edges -------------------------------------------------------------------------------------------
def _from_runs(lengths):
    return np.repeat(np.arange(len(lengths), dtype=np.float64) * 0.5 - 3.0, lengths)


def _layouts():
    t = tile_rows()
    return {
        "a run ends at a tile's last position, the next starts at a tile's first": [t - 3, 3, 5, t - 5, 7],
        "a run of 2 straddles an edge": [1] * (t - 1) + [2] + [1] * 9,
        "a run covers 3 whole tiles and one row on each side": [t - 1, 3 * t + 2, 4, 1],
        "the whole column is one run": [2 * t + 5],
        "all distinct": [1] * (2 * t + 3),
        "runs of 1 and 2 alternate": [1, 2] * (t + 1),
    }


@pytest.mark.parametrize("name", list(_layouts()))
def test_tie_runs_against_tile_edges(ctx, name):
    x = _from_runs(_layouts()[name])
    check(ctx, x)                                                         # sorted on purpose
    check(ctx, x.astype(np.int64) if name == "the whole column is one run" else (x * 2).astype(np.int64))
    check(ctx, np.random.default_rng(5).permutation(x))                  # the same cells, shuffled
    if name == "the whole column is one run":
        assert ctx.timings()["n_partitions"] == 0                         # the sort's zero-pass path


def test_first_ranks_ties_in_row_order(ctx):
    t = tile_rows()
    rng = np.random.default_rng(8)
    x = rng.integers(0, 8, 10 * t).astype(np.float64)
    check(ctx, x, methods=[FIRST, AVERAGE])
    got = ctx.rank((x, None, L.F64), x.shape[0], FIRST, out_device=False)
    for v in range(8):
        r = got[x == v]
        assert (np.diff(r) == 1.0).all() and r[0] == (x < v).sum() + 1    # consecutive ranks in row order
    assert sorted(got) == list(range(1, 10 * t + 1))


def test_signed_zeros_tie(ctx):
    x = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0] * 700)
    want = check(ctx, x)
    assert want[MIN][0] == want[MIN][1] == 701.0 and want[DENSE][1] == 2.0


# ---- NaN and null cells ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.0, 0.01, 0.5, 1.0])
def test_nan_and_null_shares(ctx, share):
    rng = np.random.default_rng(int(share * 100) + 20)
    n = 10_007
    x = rng.integers(0, 300, n).astype(np.float64)
    nan = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    nulls = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    xn = np.where(nan, np.nan, x)
    check(ctx, xn)                                                        # NaN cells only
    check(ctx, x, nulls)                                                  # null cells only
    check(ctx, x.astype(np.int64), nulls)
    want = check(ctx, xn, nulls[::-1].copy())                             # both
    out = ~(np.isnan(xn) | nulls[::-1])
    m = int(out.sum())
    assert np.isnan(want[FIRST][~out]).all() and sorted(want[FIRST][out]) == list(range(1, m + 1))
    if share == 1.0:
        check(ctx, x, np.arange(n) != 77)                                 # one rankable cell


def test_largest_run_in_front_of_the_nan_block_ends_at_m(ctx):
    t = tile_rows()
    x = np.concatenate([np.arange(t - 10, dtype=np.float64), np.full(40, 1e300), np.full(25, np.nan)])
    nulls = np.zeros(x.shape[0], bool)
    nulls[5] = True
    for data in (x, np.random.default_rng(9).permutation(x)):
        want = check(ctx, data, nulls)
        m = int((~np.isnan(data) & ~nulls).sum())
        top = (data == 1e300) & ~nulls
        assert (want[MAX][top] == float(m)).all() and top.any() and m < x.shape[0]


def test_stray_mask_bits_past_the_last_row_are_ignored(ctx):
    rng = np.random.default_rng(31)
    n = 1003                                                              # the last mask byte holds 3 rows
    x = rng.integers(0, 40, n).astype(np.float64)
    nulls = rng.random(n) < 0.2
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8
    check(ctx, x, nulls, col=(x, mask, L.F64))


# ---- I64 -----------------------------------------------------------------------------------------------------------------------
def test_int64_extremes_with_a_null_and_neighbours_beyond_2_pow_53(ctx):
    rng = np.random.default_rng(51)
    lim = np.array([I64_MIN, I64_MAX, 0, -1, 1], np.int64)[rng.integers(0, 5, 4099)]
    nulls = rng.random(4099) < 0.1
    assert "two-word code" in rank_features(lim, nulls, tile_rows())
    check(ctx, lim, nulls)
    check(ctx, np.array([I64_MAX, 7, I64_MIN], np.int64), np.array([False, True, False]))
    big = np.array([2**53 + 1, 2**53, 2**53 + 1, 2**53], np.int64)
    want = check(ctx, big)
    assert list(want[MIN]) == [3.0, 1.0, 3.0, 1.0] and list(want[DENSE]) == [2.0, 1.0, 2.0, 1.0]      # apart, though equal as f64
    check(ctx, 2**53 + rng.integers(0, 64, 5001))


# ---- memory spaces ---------------------------------------------------------------------------------------------------------
def test_host_device_resident_and_misaligned_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(71)
    n = 6151
    x = rng.integers(0, 500, n).astype(np.float64)
    x[rng.random(n) < 0.05] = np.nan
    nulls = rng.random(n) < 0.15
    mask = bits(nulls)
    want = check(ctx, x, nulls)
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    pad = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")       # rows start 8 bytes off a 16-byte boundary
    pad[1:] = dx
    assert pad.data_ptr() % 16 == 0
    padm = torch.empty(mask.shape[0] + 1, dtype=torch.uint8, device="cuda:0")
    padm[1:] = dm
    res = ctx.upload_column(x, mask, L.F64)
    try:
        for col in ((dx, dm, L.F64), (pad[1:], padm[1:], L.F64), res):
            check(ctx, x, nulls, col=col, want=want)                      # host out
            for method in METHODS:
                dev = ctx.rank(col, n, method)                            # device out
                assert dev.is_cuda and same_bits(dev.cpu().numpy(), want[method])
                into = torch.full((n + 1,), -7.0, dtype=torch.float64, device="cuda:0")
                ctx.rank(col, n, method, out=into[1:])                    # a device out 8 bytes off a 16-byte boundary
                assert same_bits(into[1:].cpu().numpy(), want[method]) and float(into[0]) == -7.0
        dev = ctx.rank((x, mask, L.F64), n, AVERAGE, out_device=True)     # host column, device out
        assert same_bits(dev.cpu().numpy(), want[AVERAGE])
        buf = np.full(n + 2, -7.0)
        ctx.rank(res, n, MAX, out=buf[:n])                                # resident column, a caller's host out
        assert same_bits(buf[:n], want[MAX]) and (buf[n:] == -7.0).all()
    finally:
        res.release()
    for m in (1, 2, 3, 17):                                               # a mask whose byte offset makes rows straddle bytes
        check(ctx, x[:m], nulls[:m], col=(pad[1:1 + m], padm[1:], L.F64))


# ---- bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import pandrs_amd as pa
    x = np.arange(16, dtype=np.float64)
    col = (x, None, L.F64)
    for bad in (-1, 5, 99):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.rank(col, 16, bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, bad
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.rank((other, None, dt), 16, AVERAGE)
        assert e.value.status == L.ERR_TYPE_MISMATCH
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    out = np.full(16, -7.0)
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, None, 16, AVERAGE, L.MEM_HOST, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, C.byref(c), 16, AVERAGE, L.MEM_HOST, None) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_rank(ctx.h, 7, C.byref(c), 16, AVERAGE, L.MEM_HOST, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, C.byref(c), 16, AVERAGE, 7, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, C.byref(c), 1 << 32, AVERAGE, L.MEM_HOST, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    nodata = L.Column()
    nodata.dtype = L.F64
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, C.byref(nodata), 16, AVERAGE, L.MEM_HOST, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_rank(ctx.h, L.MEM_HOST, C.byref(c), 0, AVERAGE, L.MEM_HOST, out.ctypes.data) == 0
    assert (out == -7.0).all()                                            # no error above, and n_rows == 0, wrote anything
    assert ctx.rank(col, 0, DENSE).shape == (0,)


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
PER_ROW = 32.2                                                  # the documented workspace (pandrs_hip.h), bytes per row
n = 1_000_000                                                   # 32 MB of workspace, nothing to stage: device column, device out
assert PER_ROW * n > cfg.memory_limit
big = (torch.arange(n, dtype=torch.float64, device="cuda:0"), None, L.F64)
for method in (L.RANK_AVERAGE, L.RANK_FIRST):
    try:
        c.rank(big, n, method)
        raise SystemExit("no error under memory_limit")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
try:
    c.rank((np.zeros(4_000_000), None, L.F64), 4_000_000, L.RANK_MIN)       # 32 MB to stage
    raise SystemExit("no error under memory_limit (staging)")
except pa.PandrsHipError as e:
    assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
k = 300_000                                                     # 9.7 MB: fits (an arena asks for 1 / 8 more and 1 MB)
assert PER_ROW * k * 1.125 + (1 << 20) < cfg.memory_limit
r = c.rank((torch.arange(k, dtype=torch.float64, device="cuda:0").flip(0), None, L.F64), k, L.RANK_DENSE)
assert torch.equal(r, torch.arange(k, 0, -1, dtype=torch.float64, device="cuda:0"))                    # still works
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
x = np.arange(1000, dtype=np.float64)
try:
    c.rank((x, None, L.F64), 1000, L.RANK_AVERAGE)
    raise SystemExit("no error below min_size_threshold")
except pa.BelowThreshold as e:
    assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
try:
    df.rank("x")
    raise SystemExit("the frame did not raise below min_size_threshold")
except pa.BelowThreshold:
    pass
y = np.arange(20_000, dtype=np.float64)[::-1].copy()
assert (c.rank((y, None, L.F64), 20_000, L.RANK_MIN, out_device=False) == np.arange(20_000, 0, -1)).all()
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- the refactored sort -------------------------------------------------------------------------------------------------------
def test_sort_indices_after_a_rank_keeps_its_permutation_and_pass_count(ctx):
    from tests.sort_ref import Col, ref_lexsort
    rng = np.random.default_rng(91)
    n = 20_011
    v = rng.integers(0, 1 << 16, n)
    v[:2] = [0, (1 << 16) - 1]                                            # a 16-bit code, every bit varies: two 8-bit digits
    check(ctx, v, methods=[AVERAGE])
    assert ctx.timings()["n_partitions"] == 2                             # the rank reports the sort's passes
    col = Col(L.I64, v, None)
    got = ctx.sort_indices([col.triple()], n, [True]).cpu().numpy()
    assert np.array_equal(got, ref_lexsort([col], [True])) and ctx.timings()["n_partitions"] == 2
    nulls = rng.random(n) < 0.1
    col = Col(L.I64, v, nulls)                                            # + a null code: 17 bits, three digits of 6
    got = ctx.sort_indices([col.triple()], n, [False]).cpu().numpy()
    assert np.array_equal(got, ref_lexsort([col], [False])) and ctx.timings()["n_partitions"] == 3


# ---- randomised sweep ----------------------------------------------------------------------------------------------------------
def test_randomised_sweep_reaches_every_special_path(ctx):
    tile = tile_rows()
    reached = {f: 0 for f in FEATURES}
    cases = 0
    try:
        for values, nulls, method, digit_bits in sweep_cases():
            ctx.set_option("sort_digit_bits", digit_bits)
            check(ctx, values, nulls, methods=[method])
            feats = rank_features(values, nulls, tile)
            if "zero-pass sort" in feats:
                assert ctx.timings()["n_partitions"] == 0
            for f in feats:
                reached[f] += 1
            cases += 1
    finally:
        ctx.set_option("sort_digit_bits", 0)
    print("sweep: %d cases, reached %s" % (cases, reached))
    assert cases == 300 and all(reached[f] > 0 for f in FEATURES), reached


# ---- one case at size ------------------------------------------------------------------------------------------------------------
def test_two_million_rows_from_50_000_values(ctx):
    rng = np.random.default_rng(101)
    n = 2_000_000
    x = rng.normal(0.0, 1.0, 50_000)[rng.integers(0, 50_000, n)]
    check(ctx, x)


# ---- mirrors ---------------------------------------------------------------------------------------------------------------------
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
    df.add_column("s", F.StringColumn(list(rng.choice(["a", "b"], n))))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    wf, wi = rank_ref_all(f, fn), rank_ref_all(i, None)
    assert same_bits(df.rank("f"), wf[AVERAGE]) and same_bits(df.rank("i"), wi[AVERAGE])     # Average is the default
    for method in F.RankMethod:
        got = df.rank("f", method)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n,)
        assert same_bits(got, wf[int(method)]) and same_bits(df.rank("i", method), wi[int(method)])
    for name in ("s", "b"):
        with pytest.raises(F.ColumnTypeMismatch):
            df.rank(name)
    with pytest.raises(F.ColumnNotFound):
        df.rank("nope")
    known = F.OptimizedDataFrame()
    known.add_column("x", F.Float64Column([3.0, 1.0, 4.0, 1.0, 5.0]))    # functions.rs:4393-4404
    ranks = known.rank("x", F.RankMethod.Average)
    assert ranks[1] == 1.5 and ranks[3] == 1.5 and ranks[0] == 3.0


def test_cpp_mirror_ranks():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rank_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "rank_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
