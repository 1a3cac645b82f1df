"""PandasCompatExt::nlargest / nsmallest / idxmax / idxmin (reference src/dataframe/pandas_compat/functions.rs:159-192): the
parts that need no GPU - the mirror's methods and errors (raised before any device call), the enum order, the C ABI entry
points without a device, the header / ctypes / Rust declarations, and the C++ mirror's methods compiled against the header."""
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
    for name in ("nlargest", "nsmallest", "idxmax", "idxmin"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.topk) and callable(E.Context.arg_extreme)
    assert (built.TOPK_LARGEST, built.TOPK_SMALLEST) == (0, 1)


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    for call in (lambda c: df.nlargest(2, c), lambda c: df.nsmallest(2, c), df.idxmax, df.idxmin):
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value)
            with pytest.raises(type(e.value)) as d:                        # the message rank uses
                df.rank(col)
            assert str(d.value) == str(e.value)
    # no rows asked for, and no rows to ask: what sort_by_columns gives for no rows, without a device
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    want = empty.sort_by_columns(["a"])
    for got in (df.nlargest(0, "x"), df.nsmallest(0, "id"), empty.nlargest(3, "a"), empty.nsmallest(3, "a")):
        assert got.row_count() == want.row_count() == 0 and got.column_names == want.column_names
    assert empty.idxmax("a") is None and empty.idxmin("a") is None
    with pytest.raises(F.ColumnNotFound):
        empty.nlargest(1, "b")


def test_frame_results_come_from_one_call_each(built, monkeypatch):
    """A stand-in context: nlargest / nsmallest hand the column's view, the row count, n and the direction to Context.topk
    once; idxmax / idxmin take their half of one Context.arg_extreme."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        device = 0

        def topk(self, col, n_rows, k, largest=True, out=None, out_device=None):
            calls.append(("topk", col[2], n_rows, k, largest))
            raise KeyboardInterrupt                                          # the gathers behind it need a device

        def arg_extreme(self, col, n_rows):
            calls.append(("arg", col[2], n_rows))
            return (1, 3)

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    for fn, largest in ((df.nlargest, True), (df.nsmallest, False)):
        with pytest.raises(KeyboardInterrupt):
            fn(3, "x")
        assert calls.pop() == ("topk", built.F64, 4, 3, largest) and not calls
    assert df.idxmin("id") == 1 and calls.pop() == ("arg", built.I64, 4)
    assert df.idxmax("id") == 3 and calls.pop() == ("arg", built.I64, 4)
    Fake.arg_extreme = lambda self, col, n_rows: None
    assert df.idxmax("x") is None and df.idxmin("x") is None


def test_enum_order_equals_the_headers(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_topk_direction {"):header.index("} pandrs_hip_topk_direction;")]
    values = dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_TOPK_(\w+) = (\d+)", body))
    assert values == {"LARGEST": 0, "SMALLEST": 1}
    for name, v in values.items():
        assert getattr(built, "TOPK_" + name) == v
    hpp = open(os.path.join(ROOT, "include", "pandrs_hip.hpp")).read()
    assert "PANDRS_HIP_TOPK_LARGEST" in hpp and "PANDRS_HIP_TOPK_SMALLEST" in hpp


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out = np.full(8, -1, np.int64)
    cnt, num, found = C.c_int64(-5), C.c_int64(-5), C.c_int32(-5)
    rows = (C.c_int64 * 2)(-5, -5)
    assert lib.pandrs_hip_topk(None, built.MEM_HOST, C.byref(col), 8, 3, built.TOPK_LARGEST, built.MEM_HOST, out.ctypes.data,
                               C.byref(cnt), C.byref(num)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    assert lib.pandrs_hip_arg_extreme(None, built.MEM_HOST, C.byref(col), 8, rows, C.byref(found)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    topk = lambda c, n, k, d, o, pc, pn: lib.pandrs_hip_topk(h, built.MEM_HOST, c, n, k, d, built.MEM_HOST, o, pc, pn)   # noqa: E731
    good = (C.byref(col), 8, 3, built.TOPK_LARGEST, out.ctypes.data, C.byref(cnt), C.byref(num))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, -1), (3, 2), (3, -1), (4, None), (5, None), (6, None)):
        args = list(good)
        args[i] = bad
        assert topk(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_topk(h, 7, *good[:4], built.MEM_HOST, *good[4:]) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_topk(h, built.MEM_HOST, *good[:4], 7, *good[4:]) == built.ERR_INVALID_ARGUMENT
    other = built.Column()
    other.data, other.dtype = x.ctypes.data, built.U32CODE
    assert topk(C.byref(other), *good[1:]) == built.ERR_TYPE_MISMATCH
    assert lib.pandrs_hip_arg_extreme(h, built.MEM_HOST, C.byref(other), 8, rows, C.byref(found)) == built.ERR_TYPE_MISMATCH
    for args in ((None, 8, rows, C.byref(found)), (C.byref(col), 8, None, C.byref(found)), (C.byref(col), 8, rows, None),
                 (C.byref(col), -1, rows, C.byref(found)), (C.byref(col), 1 << 32, rows, C.byref(found))):
        assert lib.pandrs_hip_arg_extreme(h, built.MEM_HOST, *args) == built.ERR_INVALID_ARGUMENT
    # nothing to do is OK, writes nothing and reports 0
    assert topk(C.byref(col), 8, 0, built.TOPK_SMALLEST, None, C.byref(cnt), C.byref(num)) == 0 and (cnt.value, num.value) == (0, 0)
    cnt.value = num.value = -5
    assert topk(C.byref(col), 0, 4, built.TOPK_SMALLEST, None, C.byref(cnt), C.byref(num)) == 0 and (cnt.value, num.value) == (0, 0)
    assert lib.pandrs_hip_arg_extreme(h, built.MEM_HOST, C.byref(col), 0, rows, C.byref(found)) == 0 and found.value == 0
    assert (out == -1).all() and list(rows) == [-5, -5]


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_topk": ["ctx", "mem_space", "col", "n_rows", "k", "direction", "out_mem_space", "out_rows", "out_count",
                                 "out_n_numbers"],
             "pandrs_hip_arg_extreme": ["ctx", "mem_space", "col", "n_rows", "out_rows", "out_found"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    for k, v in (("LARGEST", 0), ("SMALLEST", 1)):
        assert hdr[3]["PANDRS_HIP_TOPK_" + k] == v == rst[2]["PANDRS_HIP_TOPK_" + k]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- the first k rows of one numeric column in order"):header.index("typedef enum pandrs_hip_topk_direction")]
    for word in ("functions.rs:159-174", ":175-192", "functions.rs:4369-4391", "NaN", "-0.0", "2^53", "stable", "min_by", "max_by",
                 "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT", "2^32", "read-back",
                 "topk_tile_rows = ", "topk_blocks_per_cu = ", "topk_cutover = ", "out_n_numbers", "keep=", "multi-column", "grouped",
                 "String and Boolean", "legacy", "argmax"):
        assert word in block, word
    rank = header[header.index("/* ---- rank of one numeric column"):header.index("typedef enum pandrs_hip_rank_method")]
    assert not re.search(r"Out of scope:[^.]*grouped rank, nlargest", rank)   # no longer out of scope there


def test_cut_over_in_the_header_is_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "topk.hip")).read()
    num, den = map(int, re.search(r"TK_CUT_NUM = (\d+), TK_CUT_DEN = (\d+);", src).groups())
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    m = re.search(r"topk_cutover = (\d+) / (\d+)", header)
    assert m and (int(m.group(1)), int(m.group(2))) == (num, den) and 0 < num <= den
    assert int(re.search(r"topk_tile_rows = (\d+)", header).group(1)) == 2048
    assert "TK_TILE = TK_THREADS * TK_LOADS * 2" in src and "TK_THREADS = 256" in src and "TK_LOADS = 4" in src
    assert int(re.search(r"topk_blocks_per_cu = (\d+)", header).group(1)) == int(re.search(r"TK_BLOCKS_PER_CU = (\d+);", src).group(1))


def test_cpp_mirror_topk_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "topk_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "topk_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
