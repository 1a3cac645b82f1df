"""pandrs_hip_window_quantile and the mirrors' rolling_median / apply_rolling / apply_expanding (reference
src/series/window.rs:298-336, :494-530, helpers/window_ops.rs:206-240, dataframe/enhanced_window.rs) against the numpy twins
of tests/window_quantile_ref.py, bit for bit (NaN positions equal, every other value identical), on both paths."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests import window_quantile_ref as R  # noqa: E402
from tests.window_ref import first_diff, same  # noqa: E402

SRC = open(os.path.join(ROOT, "pandrs_amd", "csrc", "window_quantile.hip")).read()
DIRECT_MAX = int(re.search(r"constexpr int WQ_DIRECT_MAX = (\d+);", SRC).group(1))
DIRECT_TILE = 256                                                       # WQ_DT = WN_THREADS
QS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.0 / 3.0)                             # 0.5 over an even len reads the upper middle (half away)
AUTO, DIRECT, GENERAL = 0, 1, 2


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


def col_of(x, valid, dtype=None):
    dtype = (L.I64 if np.asarray(x).dtype == np.int64 else L.F64) if dtype is None else dtype
    return (x, None if valid is None or valid.all() else bits(~valid), dtype)


def run(ctx, col, n, kind, path=AUTO, **kw):
    ctx.set_option("window_quantile_path", path)
    try:
        got = ctx.window_quantile(col, n, L.WINDOW_KIND_ROLLING if kind == "rolling" else L.WINDOW_KIND_EXPANDING, **kw)
    finally:
        ctx.set_option("window_quantile_path", AUTO)
    return got.cpu().numpy() if hasattr(got, "cpu") else got


def paths_of(kind, w):
    return (DIRECT, GENERAL) if kind == "rolling" and w <= DIRECT_MAX else (AUTO,)


def check(ctx, col, n, sw, kind, w=0, center=False, mps=(None,), stats=((True, 0.5),), nan_missing=False, tag=()):
    """Every (min_periods, statistic, path) of one window shape against the twin; one twin run per statistic."""
    length = sw.lengths(kind, w, center)
    for median, q in stats:
        full = sw.stat(kind, w, center, 0, median, q)
        for mp in mps:
            want = np.where(length >= (w if mp is None else mp), full, np.nan)
            for path in paths_of(kind, w):
                got = run(ctx, col, n, kind, path, median=median, q=q, window=w, min_periods=-1 if mp is None else mp, center=center,
                          nan_missing=nan_missing)
                assert same(got, want), (tag, kind, w, center, mp, median, q, path, first_diff(got, want))


def windows_of(n):
    return sorted({1, 2, 3, 4, 7, DIRECT_MAX, DIRECT_MAX + 1, 1000, n, n + 5, 2 * n + 3})


def mixed(rng, n, null_p=0.1):
    x = rng.normal(0, 100, n)
    r = rng.random(n) < 0.3
    x[r] = np.round(x[r] / 50)                                           # ties, zeros among them
    x[rng.random(n) < 0.02] = -0.0
    return x, rng.random(n) >= null_p


# ---- sizes x windows: word, tile and level-count edges, both paths ----------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17, 2 ** 17, 2 ** 17 + 1, 3 * DIRECT_TILE + 17]


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_windows(ctx, n, center):
    rng = np.random.default_rng(n * 2 + int(center))
    x, valid = mixed(rng, n)
    col, sw = col_of(x, valid), R.SortedWindows(x, valid)
    qs = QS if n < 2 ** 17 else (0.25, 1.0 / 3.0)                        # (the twin's time, not the device's)
    for w in windows_of(n):
        check(ctx, col, n, sw, "rolling", w, center, mps=(None, 0, 1, w))
        check(ctx, col, n, sw, "rolling", w, center, mps=(1,), stats=[(False, q) for q in qs])
    if not center:
        check(ctx, col, n, sw, "expanding", mps=(0, 1, 5), stats=[(True, 0.5)] + [(False, q) for q in qs])


def test_twins_agree_where_the_definition_is_affordable(ctx):
    """The fast twin the other tests lean on, against the per-window sort, together with the device."""
    rng = np.random.default_rng(3)
    n = 700
    x, valid = mixed(rng, n, 0.2)
    col = col_of(x, valid)
    for w, center in ((5, False), (DIRECT_MAX, True), (DIRECT_MAX + 1, False), (300, True)):
        for median, q in ((True, 0.5), (False, 0.5), (False, 1.0 / 3.0)):
            want = R.window_quantile_ref(x, valid, "rolling", w, center, 2, median, q)
            assert same(R.window_quantile_fast(x, valid, "rolling", w, center, 2, median, q), want)
            for path in paths_of("rolling", w):
                got = run(ctx, col, n, "rolling", path, median=median, q=q, window=w, min_periods=2, center=center)
                assert same(got, want), (w, center, median, q, path, first_diff(got, want))


# ---- data ------------------------------------------------------------------------------------------------------------------
N_DATA = 3 * 4096 + 17
DATA_WINDOWS = (3, 4, DIRECT_MAX, DIRECT_MAX + 1, 1000)


def masks_of(rng, n):
    runs = np.ones(n, bool)
    for a in range(50, n, 700):
        runs[a:a + 100] = False
    return {"none": np.ones(n, bool), "10%": rng.random(n) >= 0.1, "50%": rng.random(n) >= 0.5, "runs": runs, "all": np.zeros(n, bool)}


def columns_of(rng, n):
    big = rng.choice(np.array([1.7e308, -1.7e308, 1.6e308, 9e307, -9e307]), n)
    i53 = (2 ** 53 + rng.integers(0, 4, n)).astype(np.int64) * rng.choice(np.array([1, -1]), n)
    return {"random": rng.normal(0, 1, n), "five values": rng.integers(0, 5, n).astype(np.float64),
            "signed zeros": rng.choice(np.array([0.0, -0.0, -0.0, 1.0, -1.0]), n),
            "infinities": rng.choice(np.array([np.inf, -np.inf, 0.5, -0.5, 3.0]), n), "near DBL_MAX": big, "i64 beyond 2^53": i53,
            "i64": rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)}


@pytest.mark.parametrize("name", ["random", "five values", "signed zeros", "infinities", "near DBL_MAX", "i64 beyond 2^53", "i64"])
def test_data_kinds_and_null_masks(ctx, name):
    rng = np.random.default_rng(len(name))
    n = N_DATA
    x = columns_of(rng, n)[name]
    for mname, valid in masks_of(rng, n).items():
        col, sw = col_of(x, valid), R.SortedWindows(x, valid)
        for w in DATA_WINDOWS:
            check(ctx, col, n, sw, "rolling", w, w == 4, mps=(1,), stats=((True, 0.5), (False, 0.75)), tag=(name, mname))
        check(ctx, col, n, sw, "expanding", mps=(1,), tag=(name, mname))
    if name == "near DBL_MAX":
        got = run(ctx, col_of(x, None), n, "rolling", window=2, median=True)
        assert np.isinf(got[1:]).any()                                    # (a + b) overflows before the divide, as the reference's


@pytest.mark.parametrize("nan_missing", [False, True])
def test_nan_cells(ctx, nan_missing):
    rng = np.random.default_rng(17 + int(nan_missing))
    n = N_DATA
    x, valid = mixed(rng, n)
    x[rng.random(n) < 0.03] = np.nan
    x[5000:5200] = np.nan
    col, sw = col_of(x, valid), R.SortedWindows(x, valid, nan_missing)
    for w in DATA_WINDOWS:
        check(ctx, col, n, sw, "rolling", w, w == 3, mps=(None, 0, 2), stats=((True, 0.5), (False, 1.0 / 3.0)), nan_missing=nan_missing)
    check(ctx, col, n, sw, "expanding", mps=(0, 3), nan_missing=nan_missing)
    if not nan_missing:                                                   # a window holding a NaN value answers NaN
        got = run(ctx, col, n, "expanding", min_periods=0)
        first = int(np.flatnonzero(np.isnan(x) & valid)[0])
        assert np.isnan(got[first:]).all()


# ---- column forms ------------------------------------------------------------------------------------------------------------
def test_host_device_resident_and_unaligned_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(13)
    n = 30_001
    x, valid = mixed(rng, n)
    mask = bits(~valid)
    sw = R.SortedWindows(x, valid)
    res = ctx.upload_column_n(x, mask, L.F64, n)
    dev = (torch.from_numpy(x).to("cuda:0"), torch.from_numpy(mask).to("cuda:0"), L.F64)
    xb = torch.zeros(n + 3, dtype=torch.float64, device="cuda:0")        # one element in: 8-byte aligned, not 256
    xb[1:n + 1] = dev[0]
    mb = torch.zeros(len(mask) + 8, dtype=torch.uint8, device="cuda:0")   # the mask at byte offset 3
    mb[3:3 + len(mask)] = dev[1]
    off = (xb[1:n + 1], mb[3:3 + len(mask)], L.F64)
    for c in ((x, mask, L.F64), res, dev, off):
        for w in (7, 77):
            check(ctx, c, n, sw, "rolling", w, True, mps=(3,), stats=((True, 0.5), (False, 0.25)))
        check(ctx, c, n, sw, "expanding", mps=(1,))
    got = ctx.window_quantile(dev, n, L.WINDOW_KIND_ROLLING, window=77, min_periods=3)
    assert got.device.type == "cuda" and got.dtype == torch.float64
    got = ctx.window_quantile((x, mask, L.F64), n, L.WINDOW_KIND_ROLLING, window=77, min_periods=3, out_device=True)
    assert got.device.type == "cuda" and same(got.cpu().numpy(), sw.stat("rolling", 77, False, 3))
    res.release()


# ---- statuses --------------------------------------------------------------------------------------------------------------
def test_bad_specs_and_types(ctx):
    import pandrs_amd as pa
    x = np.arange(10, dtype=np.float64)
    R_, E_ = L.WINDOW_KIND_ROLLING, L.WINDOW_KIND_EXPANDING
    with pytest.raises(pa.ColumnTypeMismatch) as e:
        ctx.window_quantile((np.zeros(10, np.uint32), None, L.U32CODE), 10, R_, window=3)
    assert e.value.status == L.ERR_TYPE_MISMATCH
    for kw in (dict(kind=R_, window=0), dict(kind=E_, min_periods=-1), dict(kind=L.WINDOW_KIND_EWM), dict(kind=7),
               dict(kind=R_, window=3, median=False, q=1.5), dict(kind=R_, window=3, median=False, q=-0.1),
               dict(kind=E_, min_periods=0, median=False, q=float("nan")), dict(kind=R_, window=3, median=False, q=float("inf"))):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.window_quantile((x, None, L.F64), 10, **kw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, kw
    assert same(ctx.window_quantile((x, None, L.F64), 10, R_, window=3, q=7.0), R.window_quantile_fast(x, None, "rolling", 3))   # median: q ignored
    assert len(ctx.window_quantile((x[:0], None, L.F64), 0, R_, window=3)) == 0
    ctx.set_option("window_quantile_path", DIRECT)
    try:
        for kw in (dict(kind=R_, window=DIRECT_MAX + 1), dict(kind=E_, min_periods=0)):
            with pytest.raises(pa.PandrsHipError) as e:
                ctx.window_quantile((x, None, L.F64), 10, **kw)
            assert e.value.status == L.ERR_INVALID_ARGUMENT, kw
    finally:
        ctx.set_option("window_quantile_path", AUTO)


def test_memory_limit_and_threshold():
    import pandrs_amd as pa
    lib = L.load()
    try:
        cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        import torch
        n = 4_000_000                                                   # the sort, the ranks and 22 levels: far above 8 MB
        big = (torch.zeros(n, dtype=torch.float64, device="cuda:0"), None, L.F64)
        with pytest.raises(pa.PandrsHipError) as e:
            c.window_quantile(big, n, L.WINDOW_KIND_ROLLING, window=100)
        assert e.value.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e.value)
        with pytest.raises(pa.PandrsHipError) as e:                      # a host column: its staging alone
            c.window_quantile((np.zeros(n), None, L.F64), n, L.WINDOW_KIND_ROLLING, window=3)
        assert e.value.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e.value)
        x = np.arange(1000, dtype=np.float64)
        got = c.window_quantile((x, None, L.F64), 1000, L.WINDOW_KIND_ROLLING, window=100, min_periods=1)   # still works
        assert same(got, R.window_quantile_fast(x, None, "rolling", 100, False, 1))
        c.close()
        cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        with pytest.raises(pa.BelowThreshold) as e:
            c.window_quantile((x, None, L.F64), 1000, L.WINDOW_KIND_ROLLING, window=3)
        assert e.value.status == L.ERR_BELOW_THRESHOLD
        y = np.arange(20_000, dtype=np.float64)
        got = c.window_quantile((y, None, L.F64), 20_000, L.WINDOW_KIND_EXPANDING, min_periods=0)
        assert same(got, np.arange(20_000) / 2.0)
        c.close()
    finally:
        lib.pandrs_hip_init(None)
        pa.Context(0).close()        # resets the limit


# ---- a randomised sweep --------------------------------------------------------------------------------------------------------
def test_randomised_sweep(ctx):
    rng = np.random.default_rng(20261019)
    runs = {AUTO: 0, DIRECT: 0, GENERAL: 0}
    numbers = cells = 0
    for case in range(300):
        n = int(rng.choice([rng.integers(1, 200), rng.integers(200, 5000), rng.integers(5000, 20_001)], p=[0.4, 0.4, 0.2]))
        ties = rng.choice([0, 3, 50])
        x = rng.normal(0, 1, n) if not ties else rng.integers(-ties, ties + 1, n).astype(np.float64)
        if rng.random() < 0.3:
            x[rng.random(n) < 0.1] = -0.0
        nan_missing = bool(rng.integers(0, 2))
        if rng.random() < 0.3:
            x[rng.random(n) < 0.02] = np.nan
        valid = rng.random(n) >= rng.choice([0.0, 0.05, 0.5, 0.95])
        dtype = L.F64
        if rng.random() < 0.25:
            x, dtype = rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64) if not ties else rng.integers(-ties, ties + 1, n, dtype=np.int64), L.I64
        kind = "rolling" if rng.random() < 0.8 else "expanding"
        w = int(rng.choice([rng.integers(1, DIRECT_MAX + 1), rng.integers(DIRECT_MAX + 1, 200), rng.integers(1, 2 * n + 4)]))
        center = bool(rng.integers(0, 2))
        mp = [None, 0, 1, int(rng.integers(0, w + 1))][int(rng.integers(0, 4))]
        if kind == "expanding":
            mp = int(rng.integers(0, 6))
        median = bool(rng.integers(0, 2))
        q = float(rng.choice([0.0, 0.25, 0.5, 0.75, 1.0, 1.0 / 3.0, rng.random()]))
        want = R.window_quantile_fast(x, valid, kind, w, center, mp, median, q, nan_missing)
        for path in paths_of(kind, w):
            got = run(ctx, col_of(x, valid, dtype), n, kind, path, median=median, q=q, window=w, min_periods=-1 if mp is None else mp,
                      center=center, nan_missing=nan_missing)
            assert same(got, want), (case, n, kind, w, center, mp, median, q, nan_missing, path, first_diff(got, want))
            runs[path] += 1
        numbers += int((~np.isnan(want)).sum())
        cells += n
    assert runs[DIRECT] >= 50 and runs[DIRECT] == runs[GENERAL] and runs[AUTO] >= 100, runs       # both paths, and the auto choice
    assert numbers * 4 >= cells, (numbers, cells)                          # the sweep compares numbers, not only NaN


# ---- frame level -----------------------------------------------------------------------------------------------------------
def _floats(df, name):
    return np.asarray(df.column(name).data, np.float64)


def test_frame_rolling_median_and_the_builder(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(41)
    n = 3000
    fx = rng.normal(0, 1, n)
    fx[rng.random(n) < 0.05] = np.nan
    fnull = rng.random(n) < 0.2
    iv = rng.integers(-50, 50, n)
    df = F.OptimizedDataFrame()
    df.add_column("id", F.Int64Column(np.arange(n)))
    df.add_column("f", F.Float64Column.with_nulls(fx, fnull))
    df.add_column("i", F.Int64Column(iv))
    df.add_column("s", F.StringColumn(list(rng.choice(["a", "b"], n))))
    fx = np.asarray(df.column("f").data, np.float64)
    got = df.rolling_median("f", 9)
    assert isinstance(got, np.ndarray) and same(got, R.window_quantile_fast(fx, ~fnull, "rolling", 9, False, 9, True, nan_missing=True))
    assert same(df.rolling_median("i", 40, 2), R.window_quantile_fast(iv, None, "rolling", 40, False, 2, True, nan_missing=True))
    assert same(df.rolling_median("i", 0), R.window_quantile_fast(iv, None, "rolling", 1, False, 0, True, nan_missing=True))
    r = df.apply_rolling(F.DataFrameRolling(5).min_periods(2).center(True)).median()
    assert r.column_names == ["id", "f", "i", "s", "id_median", "f_median", "i_median"] and r.row_count() == n
    assert isinstance(r.column("f_median"), F.Float64Column) and r.column("f_median").null_mask is None
    assert same(_floats(r, "f_median"), R.window_quantile_fast(fx, ~fnull, "rolling", 5, True, 2))
    assert same(_floats(r, "i_median"), R.window_quantile_fast(iv, None, "rolling", 5, True, 2))
    r = df.apply_rolling(F.DataFrameRolling(100).columns(["i"])).quantile(0.9)
    assert r.column_names == ["id", "f", "i", "s", "i_quantile"]
    assert same(_floats(r, "i_quantile"), R.window_quantile_fast(iv, None, "rolling", 100, False, None, False, 0.9))
    r = df.apply_expanding(F.DataFrameExpanding(3).columns(["i", "id"])).median()
    assert r.column_names == ["id", "f", "i", "s", "i_median", "id_median"]
    assert same(_floats(r, "i_median"), R.window_quantile_fast(iv, None, "expanding", min_periods=3))
    r = df.apply_expanding(F.DataFrameExpanding(1).columns(["i"])).quantile(0.25)
    assert same(_floats(r, "i_quantile"), R.window_quantile_fast(iv, None, "expanding", min_periods=1, median=False, q=0.25))
    r = df.apply_rolling(F.DataFrameRolling(4).columns(["i"])).max()       # the builder's other operations: Context.window
    assert same(_floats(r, "i_max")[3:], np.array([iv[k - 3:k + 1].max() for k in range(3, n)], np.float64))
    assert np.isnan(_floats(r, "i_max")[:3]).all()


def test_known_answers_from_the_reference_tests(ctx):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "window_quantile_known_answers.json")))
    for case in doc["cases"]:
        x = np.array(case["values"], np.float64)
        mp = case["min_periods"]
        for path in paths_of(case["kind"], case["window"]):
            got = run(ctx, (x, None, L.F64), len(x), case["kind"], path, median=case["stat"] == "median", q=case["q"] or 0.5,
                      window=case["window"], min_periods=-1 if mp is None else mp, center=case["center"], nan_missing=case["nan_missing"])
            for row, want in case["checks"]:
                if want is None:
                    assert np.isnan(got[row]), (case["source"], row)
                elif case["tol"] == 0:
                    assert got[row] == want, (case["source"], row)
                else:
                    assert abs(got[row] - want) < case["tol"], (case["source"], row)


def test_cpp_mirror_replays_the_known_answers():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_quantile_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "window_quantile_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "0 failed checks" in r.stdout
