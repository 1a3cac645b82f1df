"""OptimizedDataFrame::filter / filter_rows / par_filter / select_by_mask / select (reference
src/optimized/split_dataframe/data_ops.rs:15-121, row_ops.rs:26-130, parallel.rs:21-230, select.rs:150-167): the parts that need
no GPU — the mirror's methods and errors (raised before any device call), the C ABI entry points without a device, the
header / ctypes / Rust declarations, and the C++ mirror's filter compiled against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pandrs_hip_filter_indices", "pandrs_hip_filter_gather")


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


def test_mirror_has_the_methods(built):
    import pandrs_amd.frame as F
    for name in ("filter", "filter_rows", "par_filter", "select_by_mask", "select"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(F.LazyFrame.select) and callable(F.LazyFrame.filter)
    assert issubclass(F.FormatError, Exception)


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    for method in (df.filter, df.filter_rows, df.par_filter):
        with pytest.raises(F.ColumnNotFound):
            method("nope")
        with pytest.raises(F.ColumnTypeMismatch) as e:                 # data_ops.rs:115-119
            method("id")
        assert "Boolean" in str(e.value) and "'id'" in str(e.value)
        with pytest.raises(F.ColumnTypeMismatch):
            method("s")
    with pytest.raises(F.FormatError) as e:                            # select.rs:151-157
        df.select_by_mask([True, False, True])
    assert "Mask length (3) does not match DataFrame row count (4)" in str(e.value)
    with pytest.raises(F.ColumnNotFound):
        df.select(["id", "nonexistent"])                               # tests/optimized_dataframe_test.rs:155-156
    with pytest.raises(F.DuplicateColumnName):
        df.select(["id", "id"])
    # the lazy arms raise the same errors at execute(), before any device call
    with pytest.raises(F.ColumnNotFound):
        F.LazyFrame.new(df).select(["id", "flag"]).filter("x").execute()
    with pytest.raises(F.ColumnTypeMismatch):
        F.LazyFrame.new(df).filter("id").execute()
    # no rows: the empty shapes, still without a device call
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("f", F.BooleanColumn([]))
    for method in (empty.filter, empty.filter_rows, empty.par_filter):
        r = method("f")
        assert r.column_names == ["a", "f"] and r.row_count() == 0
    assert empty.select_by_mask([]).column_count() == 0


def test_select_keeps_masks_and_order_on_the_host(built, monkeypatch):
    import pandrs_amd.frame as F
    monkeypatch.setattr(F, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    df = _frame()
    r = df.select(["s", "x"])
    assert r.column_names == ["s", "x"] and r.row_count() == 4
    assert r.column("x").get(1) is None and r.column("x").null_mask is not None      # the null mask is kept
    assert r.column("s").to_list() == ["a", "b", "c", "d"]
    lz = F.LazyFrame.new(df).select(["flag", "id"]).execute()
    assert lz.column_names == ["flag", "id"]


def test_filter_entry_points_without_a_gpu_are_not_initialized(built):
    lib = built.load()
    n = C.c_int32(-1)
    assert lib.pandrs_hip_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("a GPU is present")
    bits = np.packbits(np.array([1, 0, 1, 1], bool), bitorder="little")
    cond = built.Column()
    cond.data, cond.dtype = bits.ctypes.data, built.BOOLBITS
    out = np.empty(4, np.int64)
    cnt = C.c_int64(-1)
    st = lib.pandrs_hip_filter_indices(None, built.MEM_HOST, C.byref(cond), 4, built.MEM_HOST, out.ctypes.data, C.byref(cnt))
    assert st == built.ERR_NOT_INITIALIZED and "context" in built.last_error()
    src = built.Column()
    data = np.arange(4, dtype=np.int64)
    src.data, src.dtype = data.ctypes.data, built.I64
    st = lib.pandrs_hip_filter_gather(None, built.MEM_HOST, C.byref(src), 4, 0, built.MEM_HOST, out.ctypes.data)
    assert st == built.ERR_NOT_INITIALIZED and "context" in built.last_error()


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    h_funcs = {name: params for name, params, _ in g.parse_header()[0]}
    r_funcs = {name: params for name, params, _ in g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))[0]}
    for name in ENTRIES:
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M), name
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs, name
        hp, rp = h_funcs[name], r_funcs[name]
        ctypes_args = built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(ctypes_args), name
        for (hn, ht), (rn, rt), ct in zip(hp, rp, ctypes_args):
            assert hn == rn and ht == rt, (name, hn, ht, rt)
            is_ptr = "*" in ht
            assert is_ptr == (ct is built._P or ct.__name__.startswith("LP_")), (name, hn, ct)
    # the header block documents the rules the tests below rely on
    block = header[header.index("/* ---- filter (stream compaction)"):header.index("int32_t pandrs_hip_filter_gather(")]
    for word in ("Some(true)", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "2^32", "data_ops.rs", "select.rs:150"):
        assert word in block, word


def test_cpp_mirror_filter_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "filter_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "filter_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
