"""pandrs_hip_describe / pandrs_hip_quantiles and the mirrors' describe / describe_all (reference
src/optimized/split_dataframe/stats.rs:50-171 over src/stats/descriptive.rs:91-200) against tests/describe_ref.py.
count, min, max and every percentile are compared bit for bit (zeros by ==: the sign of a zero may differ, pandrs_hip.h);
mean within 1e-9 * sum|x| / n and std within 1e-9 relative of the reference's row-order folds.  On adversarial bit patterns,
where the moments overflow, only the order statistics are compared."""
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
from tests.describe_ref import FIELD, compare_describe, compare_quantiles, describe_ref, percentile_ref, same  # noqa: E402

PS = [0.0, 5.0, 10.0, 25.0, 50.0, 75.0, 90.0, 95.0, 100.0]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def geometry():
    """(rows per workgroup iteration, workgroups of a full grid), from the entry point's documented geometry."""
    import torch
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    tile = int(re.search(r"describe_tile_rows = (\d+)", header).group(1))
    per_cu = int(re.search(r"describe_blocks_per_cu = (\d+)", header).group(1))
    return tile, per_cu * torch.cuda.get_device_properties(0).multi_processor_count


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def check(ctx, x, nulls=None, dtype=L.F64, moments=True, col=None, ps=PS):
    """describe and quantiles of one column against the reference restatement; `col` overrides how the column is passed."""
    npdt = np.int64 if dtype == L.I64 else np.float64
    x = np.asarray(x, npdt)
    n = x.shape[0]
    col = col if col is not None else (x, None if nulls is None else bits(nulls), dtype)
    got = ctx.describe(col, n)
    q, cnt = ctx.quantiles(col, n, ps)
    assert got["count"] == cnt
    compare_describe(got, x, nulls, npdt, moments)
    compare_quantiles(q, cnt, x, nulls, npdt, ps)
    return got


# ---- row counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257])
def test_small_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    check(ctx, rng.normal(500.0, 1.0, n))
    check(ctx, rng.integers(-1000, 1000, n), dtype=L.I64, moments=False)
    if n > 1:
        check(ctx, rng.normal(-3.0, 1.0, n), rng.random(n) < 0.4)


def test_tile_and_grid_boundaries(ctx):
    tile, grid = geometry()
    rng = np.random.default_rng(7)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1, grid * tile + 1):   # the last: one workgroup loops
        x = rng.normal(1000.0, 1.0, n)
        check(ctx, x)
    n = grid * tile + tile + 3
    check(ctx, rng.normal(0.0, 1.0, n), rng.random(n) < 0.1)


# ---- bit patterns ----------------------------------------------------------------------------------------------------------
def test_random_bit_patterns_run_every_digit(ctx):
    rng = np.random.default_rng(11)
    x = rng.integers(0, 2**64, 40_000, dtype=np.uint64).view(np.float64)
    x = x[~np.isnan(x)]
    assert (x < 0).any() and (x > 0).any()
    check(ctx, x, moments=False)
    check(ctx, x, rng.random(x.shape[0]) < 0.5, moments=False)
    check(ctx, rng.integers(-2**63, 2**63 - 1, 30_001, dtype=np.int64), dtype=L.I64, moments=False)


def test_all_equal_last_digit_and_top_digit(ctx):
    rng = np.random.default_rng(12)
    got = check(ctx, np.full(5000, 3.25))                                 # width 0: no digit pass
    assert got["std"] == 0.0 and got["min"] == got["max"] == got["median"] == 3.25
    a = 1.2345
    check(ctx, np.where(rng.random(5001) < 0.5, a, np.nextafter(a, 2.0)), moments=False)    # the last digit decides
    tops = np.array([1.0, -1.0, 2.0**600, -2.0**600, 2.0**-600, -2.0**-600, 3.0])          # differ in the top digit only
    check(ctx, tops[rng.integers(0, len(tops), 4099)], moments=False)
    sub = np.array([5e-324, -5e-324, 2.2e-308, 1e-310, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0])
    check(ctx, sub[rng.integers(0, len(sub), 3001)], moments=False)
    z = np.where(rng.random(1000) < 0.5, 0.0, -0.0)
    check(ctx, z)


# ---- ties and rank placement ---------------------------------------------------------------------------------------------
def test_ties_and_rank_placement(ctx):
    rng = np.random.default_rng(13)
    check(ctx, rng.integers(0, 10, 100_000).astype(np.float64))           # ten distinct values
    check(ctx, rng.integers(0, 10, 100_000), dtype=L.I64)
    check(ctx, [1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 3.0, 4.0])                  # lo and hi inside one run
    check(ctx, [5.0, 5.0, 5.0, 5.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0])        # the median's lo / hi on a run boundary
    check(ctx, [-2.0**500, -1.0, 1.0, 2.0**500], moments=False)           # lo / hi in different top-digit bins
    check(ctx, [-8.0, -3.0, 1e-300, 2.0, 2.0**900, 2.0**901], moments=False)
    for n in (10, 11, 1000, 1001):                                        # even / odd n for the median
        check(ctx, rng.permutation(n).astype(np.float64))


# ---- nulls -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.0, 0.1, 0.5, 1.0])
def test_null_shares(ctx, share):
    rng = np.random.default_rng(int(share * 10) + 20)
    n = 10_007
    x = rng.normal(10.0, 1.0, n)
    nulls = rng.random(n) < share if share < 1.0 else np.ones(n, bool)
    got = check(ctx, x, nulls)
    if share == 1.0:
        assert got["count"] == 0 and np.isnan(got["mean"]) and np.isnan(got["max"])
    check(ctx, rng.integers(0, 50, n), nulls, dtype=L.I64)


def test_stray_mask_bits_past_the_last_row(ctx):
    rng = np.random.default_rng(31)
    n = 1003                                                              # the last mask byte holds 3 rows
    x = rng.normal(0.0, 1.0, n)
    nulls = rng.random(n) < 0.2
    mask = bits(nulls).copy()
    mask[-1] |= 0xF8
    check(ctx, x, nulls, col=(x, mask, L.F64))


# ---- NaN ---------------------------------------------------------------------------------------------------------------------
def test_nan_cells_count_and_order_last(ctx):
    rng = np.random.default_rng(41)
    x = rng.normal(0.0, 1.0, 1000)
    x[rng.choice(1000, 100, replace=False)] = np.nan                      # ranks 900.. are NaN: 90 % interpolates into the block
    got = check(ctx, x, moments=False)
    assert got["count"] == 1000 and np.isnan(got["max"]) and np.isnan(got["mean"]) and np.isnan(got["std"])
    assert got["min"] == np.nanmin(x) and not np.isnan(got["q3"])
    q, _ = ctx.quantiles((x, None, L.F64), 1000, [89.9, 90.0, 90.1, 95.0])
    assert not np.isnan(q[0]) and np.isnan(q[1:]).all()                   # index 899.1 interpolates with rank 900
    x[:] = np.nan
    got = check(ctx, x, moments=False)
    assert got["count"] == 1000 and np.isnan(got["min"]) and np.isnan(got["median"])
    y = rng.normal(0.0, 1.0, 64)
    y[5] = np.nan
    check(ctx, y, rng.random(64) < 0.3, moments=False)


# ---- I64 ---------------------------------------------------------------------------------------------------------------------
def test_int64_extremes_and_collapsing_neighbours(ctx):
    rng = np.random.default_rng(51)
    check(ctx, rng.integers(-5, 6, 999), dtype=L.I64)
    lim = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1], np.int64)
    check(ctx, lim[rng.integers(0, 5, 777)], dtype=L.I64, moments=False)
    big = 2**53 + rng.integers(0, 64, 2001)                               # neighbours collapse to one double
    check(ctx, big, dtype=L.I64, moments=False)
    check(ctx, -(2**60) - rng.integers(0, 1000, 1500), rng.random(1500) < 0.2, dtype=L.I64, moments=False)


# ---- quantiles -----------------------------------------------------------------------------------------------------------
def test_quantile_lists_and_bad_arguments(ctx):
    import pandrs_amd as pa
    rng = np.random.default_rng(61)
    x = rng.normal(0.0, 1.0, 5003)
    check(ctx, x, ps=[75.0, 1.0, 50.0, 50.0, 99.99, 0.0, 75.0])            # unsorted, with repeats
    check(ctx, x, ps=list(np.linspace(0.0, 100.0, 16)))
    check(ctx, x, ps=[100.0 * k / 17.0 for k in range(1, 17)])
    col = (x, None, L.F64)
    for bad in ([50.0] * 17, [-1.0], [101.0], [float("nan")], [50.0, 100.0000001], []):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.quantiles(col, 5003, bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, bad
    for other, dt in ((np.zeros(16, np.uint8), L.BOOLBITS), (np.zeros(16, np.uint32), L.U32CODE)):
        with pytest.raises(pa.ColumnTypeMismatch) as e:
            ctx.quantiles((other, None, dt), 16, [50.0])
        assert e.value.status == L.ERR_TYPE_MISMATCH
        with pytest.raises(pa.ColumnTypeMismatch):
            ctx.describe((other, None, dt), 16)
    lib = L.load()
    c = L.Column()
    c.data, c.dtype = x.ctypes.data, L.F64
    assert lib.pandrs_hip_describe(ctx.h, L.MEM_HOST, C.byref(c), 10, None) == L.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_describe(ctx.h, 7, C.byref(c), 10, C.byref(L.DescribeStats())) == L.ERR_INVALID_ARGUMENT
    out = L.DescribeStats()
    assert lib.pandrs_hip_describe(ctx.h, L.MEM_HOST, C.byref(c), 0, C.byref(out)) == 0 and out.count == 0 and np.isnan(out.median)


# ---- memory spaces ---------------------------------------------------------------------------------------------------------
def test_host_device_resident_and_misaligned_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(71)
    n = 6151
    x = rng.normal(0.0, 1.0, n)
    nulls = rng.random(n) < 0.15
    mask = bits(nulls)
    host = check(ctx, x, nulls)
    hq, _ = ctx.quantiles((x, mask, L.F64), n, PS)
    dx, dm = torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()
    pad = torch.empty(n + 1, dtype=torch.float64, device="cuda:0")       # rows start 8 bytes off a 16-byte boundary
    pad[1:] = dx
    assert pad.data_ptr() % 16 == 0
    padm = torch.empty(mask.shape[0] + 1, dtype=torch.uint8, device="cuda:0")
    padm[1:] = dm
    res = ctx.upload_column(x, mask, L.F64)
    try:
        for col in ((dx, dm, L.F64), (pad[1:], padm[1:], L.F64), res):
            got = check(ctx, x, nulls, col=col)
            gq, _ = ctx.quantiles(col, n, PS)
            assert all(np.float64(got[f]).tobytes() == np.float64(host[f]).tobytes() for f in host), (got, host)
            assert gq.tobytes() == hq.tobytes()
    finally:
        res.release()
    # one row past the head row, and a mask whose byte offset makes row pairs straddle bytes
    for m in (1, 2, 3, 17):
        check(ctx, x[:m], nulls[:m], col=(pad[1:1 + m], padm[1:], L.F64))


CHILD = r"""
import ctypes as C, numpy as np, sys
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
import pandrs_amd.frame as F
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
n = 4_000_000                                                   # 32 MB to stage
big = (np.zeros(n), None, L.F64)
for call in (lambda: c.describe(big, n), lambda: c.quantiles(big, n, [50.0])):
    try:
        call()
        raise SystemExit("no error under memory_limit")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
x = np.arange(1000, dtype=np.float64)
assert c.describe((x, None, L.F64), 1000)["median"] == 499.5     # still works
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
for call in (lambda: c.describe((x, None, L.F64), 1000), lambda: c.quantiles((x, None, L.F64), 1000, [50.0])):
    try:
        call()
        raise SystemExit("no error below min_size_threshold")
    except pa.BelowThreshold as e:
        assert e.status == L.ERR_BELOW_THRESHOLD
df = F.OptimizedDataFrame()
df.add_column("x", F.Float64Column(x))
try:
    df.describe("x")
    raise SystemExit("the frame did not raise below min_size_threshold")
except pa.BelowThreshold:
    pass
y = np.arange(20_000, dtype=np.float64)
assert c.describe((y, None, L.F64), 20_000)["max"] == 19_999.0
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- frames ----------------------------------------------------------------------------------------------------------------
def test_frames_describe_and_describe_all(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(81)
    n = 3001
    f, fn = rng.normal(100.0, 1.0, n), rng.random(n) < 0.2
    i = rng.integers(-50, 50, n)
    df = F.OptimizedDataFrame()
    df.add_column("i", F.Int64Column(i))
    df.add_column("f", F.Float64Column.with_nulls(f, fn))
    df.add_column("s", F.StringColumn(list(rng.choice(["a", "b"], n))))
    df.add_column("b", F.BooleanColumn(list(rng.random(n) < 0.5)))
    df.add_column("void", F.Float64Column.with_nulls(np.zeros(n), np.ones(n, bool)))
    df.add_column("one", F.Int64Column.with_nulls(np.arange(n), np.arange(n) != 5))
    d = df.describe("f")
    assert [k for k, _ in d.stats_list] == ["count", "mean", "std", "min", "25%", "50%", "75%", "max"] and d.stats == dict(d.stats_list)
    want = describe_ref(f, fn, np.float64)
    assert d.stats["count"] == want["count"] and all(same(d.stats[k], want[k]) for k in FIELD)
    assert abs(d.stats["mean"] - want["mean"]) <= 1e-9 * abs(want["mean"]) and abs(d.stats["std"] - want["std"]) <= 1e-9 * want["std"]
    wi = describe_ref(i, None, np.int64)
    di = df.describe("i")
    assert all(same(di.stats[k], wi[k]) for k in FIELD) and di.stats["count"] == n
    for name in ("void", "one"):                                          # no non-null cell; one (0 degrees of freedom)
        with pytest.raises(F.InvalidValue):
            df.describe(name)
    for name in ("s", "b"):
        with pytest.raises(F.ColumnTypeMismatch):
            df.describe(name)
    everything = df.describe_all()
    assert sorted(everything) == ["f", "i"] and everything["f"].stats_list == d.stats_list


def test_the_references_known_answers(ctx):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("values", F.Float64Column([1.0, 2.0, 3.0, 4.0, 5.0]))     # descriptive.rs:612-623, stats.rs:567-583
    df.add_column("constant", F.Float64Column([5.0] * 5))                    # stats_comprehensive_test.rs:478-482
    d = df.describe("values").stats
    assert (d["count"], d["mean"], d["50%"], d["min"], d["max"], d["25%"], d["75%"]) == (5.0, 3.0, 3.0, 1.0, 5.0, 2.0, 4.0)
    assert abs(d["std"] - np.sqrt(2.5)) <= 1e-9 * np.sqrt(2.5)
    assert df.describe("constant").stats["std"] == 0.0
    q, cnt = ctx.quantiles((np.array([1.0, 2.0, 3.0, 4.0, 5.0]), None, L.F64), 5, [0.0, 50.0, 100.0])   # descriptive.rs:625-632
    assert list(q) == [1.0, 3.0, 5.0] and cnt == 5


def test_cpp_mirror_describes():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "describe_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "describe_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout


# ---- one cross-check at size ---------------------------------------------------------------------------------------------
def test_two_million_rows_against_torch_sort(ctx):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(5)
    n = 2_000_000
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=g) * 3.0 + 7.0
    s = torch.sort(x).values.cpu().numpy()
    got = ctx.describe((x, None, L.F64), n)
    q, cnt = ctx.quantiles((x, None, L.F64), n, PS)
    assert cnt == got["count"] == n and got["min"] == s[0] and got["max"] == s[-1]
    assert (got["q1"], got["median"], got["q3"]) == (percentile_ref(s, 25.0), percentile_ref(s, 50.0), percentile_ref(s, 75.0))
    assert list(q) == [percentile_ref(s, p) for p in PS]
    xs = x.cpu().numpy()
    want = describe_ref(xs, None, np.float64)
    assert abs(got["mean"] - want["mean"]) <= 1e-9 * np.abs(xs).sum() / n and abs(got["std"] - want["std"]) <= 1e-9 * want["std"]
