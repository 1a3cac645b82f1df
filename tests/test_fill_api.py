"""PandasCompatExt::fillna / fillna_method / interpolate / ffill / bfill (reference src/dataframe/pandas_compat/functions.rs
:789-918, :3626-3683): the parts that need no GPU — the mirror's methods and errors (raised before any device call), the
constants, the C ABI entry point without a device, the header / ctypes / Rust declarations, and the C++ mirror compiled
against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ["ctx", "mem_space", "col", "n_rows", "method", "fill_bits", "out_mem_space", "out_data", "out_null_mask", "out_n_missing"]


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
    return [lambda c: df.ffill(c), lambda c: df.bfill(c), lambda c: df.interpolate(c), lambda c: df.fillna(c, 0.0),
            lambda c: df.fillna_method(c, "ffill"), lambda c: df.fillna_method(c, "backward")]


def test_mirror_has_the_methods_and_the_constants(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("ffill", "bfill", "fillna_method", "interpolate", "fillna"):
        assert callable(getattr(F.OptimizedDataFrame, name))
    assert callable(E.Context.fill)
    assert (built.FILL_FFILL, built.FILL_BFILL, built.FILL_LINEAR, built.FILL_VALUE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_fill_method {"):header.index("} pandrs_hip_fill_method;")]
    assert dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_FILL_(\w+) = (\d+)", body)) == {"FFILL": 0, "BFILL": 1, "LINEAR": 2, "VALUE": 3}


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
    for bad in ("invalid", "", "FFILL", "linear"):
        with pytest.raises(F.InvalidValue) as e:                           # functions.rs:846-851, :4877-4887
            df.fillna_method("x", bad)
        assert str(e.value) == "Invalid fill method: '%s'. Use 'ffill' or 'bfill'." % bad
    with pytest.raises(F.ColumnNotFound):
        df.fillna_method("nope", "invalid")                                # the column is looked up first (:812)
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("b", F.Float64Column([]))
    for call in _calls(empty):
        got = call("b")
        assert got is not empty and got.column_names == ["a", "b"] and got.row_count() == 0


def test_frame_result_comes_from_one_fill_call(built, monkeypatch):
    """A stand-in context: the frame hands the column's view, the row count, the method's number and the value to
    Context.fill once and builds the new frame from what it returns."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        def fill(self, col, n_rows, method, value=None, out=None, out_mask=None, out_device=None):
            calls.append((col[2], n_rows, method, value, out_device))
            i64 = col[2] == built.I64 and method != built.FILL_LINEAR
            vals = np.arange(n_rows, dtype=np.int64 if i64 else np.float64)
            return (vals, np.array([0x08], np.uint8), 1) if method == built.FILL_BFILL else (vals, None, 0)

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    got = df.ffill("x")
    assert calls == [(built.F64, 4, built.FILL_FFILL, None, False)]
    assert got is not df and got.column_names == ["id", "x", "s", "flag"]
    assert isinstance(got.column("x"), F.Float64Column) and got.column("x").null_mask is None and list(got.column("x").data) == [0.0, 1.0, 2.0, 3.0]
    assert all(got.column(n) is df.column(n) for n in ("id", "s", "flag"))                 # shared unchanged
    assert df.column("x").null_mask is not None                                             # and the source as it was
    got = df.bfill("id")
    assert isinstance(got.column("id"), F.Int64Column) and got.column("id").is_null(3) and not got.column("id").is_null(0)
    got = df.interpolate("id")
    assert isinstance(got.column("id"), F.Float64Column) and got.column_names[0] == "id"
    df.fillna("id", -7)
    df.fillna_method("x", "forward")
    df.fillna_method("x", "bfill")
    assert calls[1:] == [(built.I64, 4, built.FILL_BFILL, None, False), (built.I64, 4, built.FILL_LINEAR, None, False),
                         (built.I64, 4, built.FILL_VALUE, -7, False), (built.F64, 4, built.FILL_FFILL, None, False),
                         (built.F64, 4, built.FILL_BFILL, None, False)]


def test_entry_point_without_a_context_is_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out, mask, missing = np.full(8, -1.0), np.full(1, 0xAA, np.uint8), C.c_int64(-5)
    st = lib.pandrs_hip_fill(None, built.MEM_HOST, C.byref(col), 8, built.FILL_FFILL, 0, built.MEM_HOST, out.ctypes.data, mask.ctypes.data,
                             C.byref(missing))
    assert st == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error() and (out == -1.0).all() and mask[0] == 0xAA and missing.value == -5


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    name = "pandrs_hip_fill"
    assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
    assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
    hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
    assert len(hp) == len(rp) == len(cp) == len(PARAMS)
    assert [n for n, _ in hp] == PARAMS
    for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
        assert hn == rn and ht == rt, (hn, ht, rt)
        assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert cp[5] is C.c_uint64
    for k, v in (("FFILL", 0), ("BFILL", 1), ("LINEAR", 2), ("VALUE", 3)):
        assert hdr[3]["PANDRS_HIP_FILL_" + k] == v == rst[2]["PANDRS_HIP_FILL_" + k] == getattr(built, "FILL_" + k)
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- missing cells of one numeric column"):header.index("typedef enum pandrs_hip_fill_method")]
    for word in ("functions.rs:789", ":811-868", ":870-918", ":3626-3683", "0x7FF8000000000000", "inf - inf", "-0.0", "fill_tile_rows = ",
                 "fill_blocks_per_cu = ", "Deviations", "casts every numeric column to f64", "I64 stays I64", "null bit counts as missing",
                 "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT", "2^32", "0.13 bytes per row",
                 "PANDRS_HIP_PHASE_AGGREGATE", "in place", "limit=", "dropna", "non-linear", "group-wise", "String and Boolean", "legacy",
                 "fillna_forward"):
        assert word in block, word
    assert "fill.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()


def test_cpp_mirror_fill_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "fill_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "fill_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
