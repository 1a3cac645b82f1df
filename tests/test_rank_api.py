"""PandasCompatExt::rank (reference src/dataframe/pandas_compat/functions.rs:193-236): the parts that need no GPU — the
mirror's methods and errors (raised before any device call), the enum order, the C ABI entry point without a device, the
header / ctypes / Rust declarations, and the C++ mirror's rank compiled against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["Average", "Min", "Max", "First", "Dense"]             # pandas_compat/types.rs:48-59


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
    assert callable(F.OptimizedDataFrame.rank) and callable(E.Context.rank)
    assert [m.name for m in F.RankMethod] == NAMES and [int(m) for m in F.RankMethod] == [0, 1, 2, 3, 4]


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    with pytest.raises(F.ColumnNotFound):
        df.rank("nope")
    for col in ("s", "flag"):
        with pytest.raises(F.ColumnTypeMismatch) as e:
            df.rank(col, F.RankMethod.Dense)
        assert "Column '%s' is not a numeric type" % col in str(e.value)
        with pytest.raises(type(e.value)) as d:                            # the message describe uses
            df.describe(col)
        assert str(d.value) == str(e.value)
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    for method in F.RankMethod:
        got = empty.rank("a", method)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (0,)
    with pytest.raises(F.ColumnNotFound):
        empty.rank("b")


def test_frame_result_comes_from_one_rank_call(built, monkeypatch):
    """A stand-in context: the frame hands the column's view, the row count and the method's number to Context.rank once
    and returns its float64 array."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        def rank(self, col, n_rows, method, out=None, out_device=None):
            calls.append((col[2], n_rows, method, out_device))
            return np.arange(n_rows, dtype=np.float64)

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    got = df.rank("x")
    assert calls == [(built.F64, 4, 0, False)] and got.dtype == np.float64 and list(got) == [0.0, 1.0, 2.0, 3.0]
    df.rank("id", F.RankMethod.First)
    df.rank("id", 4)
    assert calls[1:] == [(built.I64, 4, 3, False), (built.I64, 4, 4, False)]
    with pytest.raises(ValueError):
        df.rank("id", 5)


def test_enum_order_equals_the_headers(built):
    import pandrs_amd.frame as F
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_rank_method {"):header.index("} pandrs_hip_rank_method;")]
    values = dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_RANK_(\w+) = (\d+)", body))
    assert values == {"AVERAGE": 0, "MIN": 1, "MAX": 2, "FIRST": 3, "DENSE": 4}
    for m in F.RankMethod:
        assert values[m.name.upper()] == int(m) == getattr(built, "RANK_" + m.name.upper())
    hpp = open(os.path.join(ROOT, "include", "pandrs_hip.hpp")).read()
    assert re.search(r"enum class RankMethod : int32_t \{ Average = 0, Min = 1, Max = 2, First = 3, Dense = 4 \};", hpp)


def test_entry_point_without_a_context_is_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out = np.full(8, -1.0)
    assert lib.pandrs_hip_rank(None, built.MEM_HOST, C.byref(col), 8, built.RANK_AVERAGE, built.MEM_HOST, out.ctypes.data) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error() and (out == -1.0).all()


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    name = "pandrs_hip_rank"
    assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
    assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
    hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
    assert len(hp) == len(rp) == len(cp) == 7
    assert [n for n, _ in hp] == ["ctx", "mem_space", "col", "n_rows", "method", "out_mem_space", "out"]
    for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
        assert hn == rn and ht == rt, (hn, ht, rt)
        assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    for k, v in (("AVERAGE", 0), ("MIN", 1), ("MAX", 2), ("FIRST", 3), ("DENSE", 4)):
        assert hdr[3]["PANDRS_HIP_RANK_" + k] == v == rst[2]["PANDRS_HIP_RANK_" + k]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- rank of one numeric column"):header.index("typedef enum pandrs_hip_rank_method")]
    for word in ("functions.rs:193-236", "types.rs:48-59", "base.rs:555-561", "base.rs:569", "NaN", "-0.0", "2^53", "TYPE_MISMATCH",
                 "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT", "2^32", "bytes per row", "rank_tile_rows = ",
                 "rank_blocks_per_cu = ", "descending", "pct", "grouped", "nlargest", "legacy", "mann_whitney_u"):
        assert word in block, word


def test_cpp_mirror_rank_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "rank_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "rank_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
