"""OptimizedDataFrame::describe / describe_all (reference src/optimized/split_dataframe/stats.rs:50-171 over
src/stats/descriptive.rs:91-200): the parts that need no GPU — the mirror's methods and errors (raised before any device
call), the two C ABI entry points without a device, the header / ctypes / Rust declarations and struct layout, and the C++
mirror's describe compiled against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from pandrs_amd import _lib
    return _lib


def _frame():
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("id", F.Int64Column([1, 2, 3, 4]))
    df.add_column("x", F.Float64Column.with_nulls([0.5, 0.25, 1.0, 2.0], [False, True, False, False]))
    df.add_column("s", F.StringColumn(["a", "b", "c", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    return df


def _no_device(monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)


def test_mirror_has_the_methods(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("describe", "describe_all"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.describe) and callable(E.Context.quantiles)
    d = F.StatDescribe([("count", 2.0), ("mean", 1.5)])
    assert d.stats == {"count": 2.0, "mean": 1.5} and d.stats_list == [("count", 2.0), ("mean", 1.5)]


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    with pytest.raises(F.ColumnNotFound):
        df.describe("nope")
    for col in ("s", "flag"):                                              # Error::Type (stats.rs:146-149), as sum()
        with pytest.raises(F.ColumnTypeMismatch) as e:
            df.describe(col)
        assert "Column '%s' is not a numeric type" % col in str(e.value)
        with pytest.raises(type(e.value)):
            df.sum(col)
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("s", F.StringColumn([]))
    with pytest.raises(F.InvalidValue) as e:                               # descriptive.rs:92-96
        empty.describe("a")
    assert "empty data" in str(e.value)
    assert empty.describe_all() == {}


def test_frame_results_come_from_one_describe_call(built, monkeypatch):
    """A stand-in context: the frame hands the column's view to Context.describe once, orders the eight keys as the
    reference's stats_list, and raises InvalidValue for counts 0 and 1."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        def __init__(self, count):
            self.count = count

        def describe(self, col, n_rows):
            calls.append((col[2], n_rows))
            return {"count": self.count, "mean": 1.0, "std": 2.0, "min": 3.0, "q1": 4.0, "median": 5.0, "q3": 6.0, "max": 7.0}

    df = _frame()
    monkeypatch.setattr(F, "get_context", lambda: Fake(3))
    d = df.describe("x")
    assert calls == [(built.F64, 4)]
    assert d.stats_list == [("count", 3.0), ("mean", 1.0), ("std", 2.0), ("min", 3.0), ("25%", 4.0), ("50%", 5.0), ("75%", 6.0), ("max", 7.0)]
    assert d.stats == dict(d.stats_list)
    assert sorted(df.describe_all()) == ["id", "x"]
    for count in (0, 1):
        monkeypatch.setattr(F, "get_context", lambda count=count: Fake(count))
        with pytest.raises(F.InvalidValue):
            df.describe("x")
        assert df.describe_all() == {}


def test_entry_points_without_a_context_are_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out = built.DescribeStats()
    assert lib.pandrs_hip_describe(None, built.MEM_HOST, C.byref(col), 8, C.byref(out)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    ps = (C.c_double * 1)(50.0)
    q = (C.c_double * 1)()
    cnt = C.c_int64(0)
    assert lib.pandrs_hip_quantiles(None, built.MEM_HOST, C.byref(col), 8, ps, 1, q, C.byref(cnt)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()


def test_stats_layout_matches_the_header(built):
    assert C.sizeof(built.DescribeStats) == 64
    offs = [(name, getattr(built.DescribeStats, name).offset) for name, _ in built.DescribeStats._fields_]
    assert offs == [("count", 0), ("mean", 8), ("std", 16), ("min", 24), ("q1", 32), ("median", 40), ("q3", 48), ("max", 56)]
    assert built.DescribeStats._fields_[0][1] is C.c_int64 and all(t is C.c_double for _, t in built.DescribeStats._fields_[1:])
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef struct pandrs_hip_describe_stats {"):header.index("} pandrs_hip_describe_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.search(r"int64_t\s+count;", body)
    assert re.search(r"double\s+mean,\s*std,\s*min,\s*q1,\s*median,\s*q3,\s*max;", body)


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    for name, arity in (("pandrs_hip_describe", 5), ("pandrs_hip_quantiles", 8)):
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == arity
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    fields = ["count", "mean", "std", "min", "q1", "median", "q3", "max"]
    assert [n for n, _ in hdr[1]["pandrs_hip_describe_stats"]] == fields
    assert [n for n, _ in rst[1]["PandrsHipDescribeStats"]] == fields
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- describe and exact percentiles"):header.index("typedef struct pandrs_hip_describe_stats")]
    for word in ("stats.rs:50-171", "descriptive.rs:91-166", ":169-200", "gpu.rs:240-316", "NaN", "-0.0", "sign bit", "TYPE_MISMATCH",
                 "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT", "2^32", "1e-9", "describe_tile_rows = ",
                 "describe_blocks_per_cu = "):
        assert word in block, word


def test_cpp_mirror_describe_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "describe_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "describe_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
