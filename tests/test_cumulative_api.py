"""PandasCompatExt::cumsum / cumprod / cummax / cummin / cumcount / shift / diff / pct_change (reference
src/dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094): the parts that need no GPU — the mirror's methods
and errors (raised before any device call), the constants, the C ABI entry points without a device, the header / ctypes /
Rust declarations, and the C++ mirror compiled against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUM_PARAMS = ["ctx", "mem_space", "col", "n_rows", "op", "out_mem_space", "out_data", "out_null_mask", "out_n_null"]
LAG_PARAMS = ["ctx", "mem_space", "col", "n_rows", "op", "periods", "out_mem_space", "out_data", "out_null_mask", "out_n_null"]
CUM_ENUM = {"SUM": 0, "PROD": 1, "MAX": 2, "MIN": 3, "COUNT": 4}
LAG_ENUM = {"SHIFT": 0, "DIFF": 1, "PCT_CHANGE": 2}


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
    df.add_column("x", F.Float64Column.with_nulls([0.5, np.nan, 1.0, 2.0], [False, False, True, False]))
    df.add_column("s", F.StringColumn(["a", "b", "c", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    return df


def _calls(df):
    return [df.cumsum, df.cumprod, df.cummax, df.cummin, df.cumcount, lambda c: df.shift(c, 1), lambda c: df.shift(c, -2),
            lambda c: df.diff(c, 1), lambda c: df.pct_change(c, 2)]


def test_mirror_has_the_methods_and_the_constants(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("cumsum", "cumprod", "cummax", "cummin", "cumcount", "shift", "diff", "pct_change"):
        assert callable(getattr(F.OptimizedDataFrame, name))
    assert callable(E.Context.cumulative) and callable(E.Context.lag)
    assert (built.CUM_SUM, built.CUM_PROD, built.CUM_MAX, built.CUM_MIN, built.CUM_COUNT) == (0, 1, 2, 3, 4)
    assert (built.LAG_SHIFT, built.LAG_DIFF, built.LAG_PCT_CHANGE) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_cum_op {"):header.index("} pandrs_hip_cum_op;")]
    assert dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_CUM_(\w+) = (\d+)", body)) == CUM_ENUM
    body = header[header.index("typedef enum pandrs_hip_lag_op {"):header.index("} pandrs_hip_lag_op;")]
    assert dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_LAG_(\w+) = (\d+)", body)) == LAG_ENUM


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    for call in _calls(df):
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value)
            with pytest.raises(type(e.value)) as d:                        # the message describe and rank use
                df.rank(col)
            assert str(d.value) == str(e.value)
    for call in (df.diff, df.pct_change):                                  # the reference takes a usize
        with pytest.raises(F.InvalidValue):
            call("x", -1)
        with pytest.raises(F.ColumnNotFound):
            call("nope", -1)                                               # the column is looked up first
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("b", F.Float64Column([]))
    for call in _calls(empty):
        assert call("a") == [] and call("b") == []


def test_frame_results_come_from_one_call_each(built, monkeypatch):
    """A stand-in context: the frame hands the column's view, the row count, the op's number and the periods to
    Context.cumulative / Context.lag once and turns what comes back into the reference's lists."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        def cumulative(self, col, n_rows, op, out=None, out_mask=None, out_device=None):
            calls.append(("cum", col[2], n_rows, op, out_device))
            return np.arange(n_rows, dtype=np.int64 if op == built.CUM_COUNT else np.float64), None, 0

        def lag(self, col, n_rows, op, periods, out=None, out_mask=None, out_device=None):
            calls.append(("lag", col[2], n_rows, op, periods, out_device))
            return np.array([np.nan, 1.5, np.nan, 3.5]), np.array([0x01], np.uint8), 1

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    assert df.cumsum("x") == [0.0, 1.0, 2.0, 3.0] and all(type(v) is float for v in df.cumprod("id"))
    got = df.cumcount("x")
    assert got == [0, 1, 2, 3] and all(type(v) is int for v in got)
    df.cummax("id"), df.cummin("x")
    assert calls == [("cum", built.F64, 4, built.CUM_SUM, False), ("cum", built.I64, 4, built.CUM_PROD, False),
                     ("cum", built.F64, 4, built.CUM_COUNT, False), ("cum", built.I64, 4, built.CUM_MAX, False),
                     ("cum", built.F64, 4, built.CUM_MIN, False)]
    del calls[:]
    got = df.shift("x", -3)
    assert got[0] is None and got[1] == 1.5 and np.isnan(got[2]) and got[3] == 3.5       # None by the bit, not by the NaN
    got = df.diff("id", 2)
    assert np.isnan(got[0]) and got[1] == 1.5 and all(type(v) is float for v in got)
    df.pct_change("x", 0)
    assert calls == [("lag", built.F64, 4, built.LAG_SHIFT, -3, False), ("lag", built.I64, 4, built.LAG_DIFF, 2, False),
                     ("lag", built.F64, 4, built.LAG_PCT_CHANGE, 0, False)]


def test_entry_points_without_a_context_are_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out, mask, nulls = np.full(8, -1.0), np.full(1, 0xAA, np.uint8), C.c_int64(-5)
    st = lib.pandrs_hip_cumulative(None, built.MEM_HOST, C.byref(col), 8, built.CUM_SUM, built.MEM_HOST, out.ctypes.data, mask.ctypes.data,
                                   C.byref(nulls))
    assert st == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error() and (out == -1.0).all() and mask[0] == 0xAA and nulls.value == -5
    st = lib.pandrs_hip_lag(None, built.MEM_HOST, C.byref(col), 8, built.LAG_DIFF, 1, built.MEM_HOST, out.ctypes.data, mask.ctypes.data,
                            C.byref(nulls))
    assert st == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error() and (out == -1.0).all() and mask[0] == 0xAA and nulls.value == -5


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    for name, params in (("pandrs_hip_cumulative", CUM_PARAMS), ("pandrs_hip_lag", LAG_PARAMS)):
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert built.SYMBOLS["pandrs_hip_lag"][1][5] is C.c_int64
    for k, v in CUM_ENUM.items():
        assert hdr[3]["PANDRS_HIP_CUM_" + k] == v == rst[2]["PANDRS_HIP_CUM_" + k] == getattr(built, "CUM_" + k)
    for k, v in LAG_ENUM.items():
        assert hdr[3]["PANDRS_HIP_LAG_" + k] == v == rst[2]["PANDRS_HIP_LAG_" + k] == getattr(built, "LAG_" + k)
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- running folds and lagged differences of one numeric column"):header.index("typedef enum pandrs_hip_cum_op")]
    for word in ("functions.rs:280-327", ":328-342", ":514-530", ":531-541", ":2081-2094", ":4411-4447", "0x7FF8000000000000", "+0.0", "-0.0",
                 "gamma_k", "2^53", "frexp", "sticky", "subnormal", "f64::max", "cum_tile_rows = ", "cum_blocks_per_cu = ", "Deviations",
                 "no null mask", "kernel boundary", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT",
                 "2^32", "PANDRS_HIP_PHASE_AGGREGATE", "in place", "vec![NAN; n]", "periods < 0", "Group-wise".lower(), "clip", "skipna=",
                 "reverse scans", "String and Boolean", "legacy", "TimeSeries"):
        assert word in block, word
    assert "cumulative.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "cumulative.hip")).read()
    assert int(re.search(r"cum_tile_rows = (\d+)", block).group(1)) == 2048 and "CUM_TILE = CUM_WAVES * CUM_WAVE_ROWS" in src
    assert "CUM_BLOCKS_PER_CU = %s;" % re.search(r"cum_blocks_per_cu = (\d+)", block).group(1) in src


def test_cpp_mirror_cumulative_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cumulative_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "cumulative_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
