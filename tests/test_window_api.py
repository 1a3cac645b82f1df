"""DataFrameWindowExt::{rolling, expanding, ewm} (reference src/dataframe/window.rs:13-160 over src/series/window.rs): the
parts that need no GPU — the mirror's methods, result shape and errors (raised before any device call), the C ABI entry
point without a device, the header / ctypes / Rust declarations and struct layout, and the C++ mirror's window methods
compiled against the header."""
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
    import pandrs_amd.frame as F
    for name in ("rolling", "expanding", "ewm"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert issubclass(F.InvalidValue, Exception)
    import pandrs_amd.engine as E
    assert callable(E.Context.window)


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    calls = (lambda c, op: df.rolling(3, c, op), lambda c, op: df.expanding(1, c, op), lambda c, op: df.ewm(c, op, span=3))
    for call in calls:
        with pytest.raises(F.ColumnNotFound):
            call("nope", "mean")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col, "mean")
            assert "'%s'" % col in str(e.value)
    with pytest.raises(F.InvalidValue) as e:                           # series/window.rs:112-117
        df.rolling(0, "x", "mean")
    assert "Window size must be greater than 0" in str(e.value)
    for op in ("median", "quantile", "apply", "mode", ""):
        with pytest.raises(F.InvalidValue) as e:
            df.rolling(2, "x", op)
        assert "Unsupported rolling operation" in str(e.value)
        with pytest.raises(F.InvalidValue):
            df.expanding(1, "x", op)
    for op in ("sum", "min", "max", "count", "median"):                # EWM: mean / std / var only
        with pytest.raises(F.InvalidValue) as e:
            df.ewm("x", op, span=3)
        assert "Unsupported EWM operation" in str(e.value)
    with pytest.raises(F.InvalidValue) as e:
        df.ewm("x", "mean")                                            # neither span nor alpha
    assert "span or alpha" in str(e.value)
    for bad in (0.0, -0.1, 1.5, float("nan")):                          # series/window.rs:567-573
        with pytest.raises(F.InvalidValue):
            df.ewm("x", "mean", alpha=bad)
    with pytest.raises(F.DuplicateColumnName):
        df.rolling(2, "x", "sum", "id")
    with pytest.raises(F.DuplicateColumnName):
        df.expanding(1, "id", "max", "x")
    with pytest.raises(F.DuplicateColumnName):
        df.ewm("x", "mean", span=2, new_column_name="s")
    with pytest.raises(F.InvalidValue):
        df.expanding(-1, "x", "sum")


def test_empty_frames_keep_the_shape_without_a_device(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("f", F.Float64Column([]))
    r = empty.rolling(3, "f", "Mean")
    assert r.column_names == ["a", "f", "f_Mean"] and r.row_count() == 0      # the name keeps the caller's spelling
    assert isinstance(r.column("f_Mean"), F.Float64Column)
    assert empty.expanding(0, "a", "count", "c").column_names == ["a", "f", "c"]
    assert empty.ewm("f", "VAR", alpha=0.5).column_names == ["a", "f", "f_VAR"]


def test_window_entry_point_without_a_gpu_is_not_initialized(built):
    lib = built.load()
    n = C.c_int32(-1)
    assert lib.pandrs_hip_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("a GPU is present")
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    spec = built.WindowSpec(kind=built.WINDOW_KIND_ROLLING, op=built.WINDOW_SUM, window=3, min_periods=-1, center=0, ddof=1)
    out = np.empty(8)
    st = lib.pandrs_hip_window(None, built.MEM_HOST, C.byref(col), 8, C.byref(spec), built.MEM_HOST, out.ctypes.data)
    assert st == built.ERR_NOT_INITIALIZED and "context" in built.last_error()


def test_spec_layout_matches_the_header(built):
    assert C.sizeof(built.WindowSpec) == 48
    offs = {name: getattr(built.WindowSpec, name).offset for name, _ in built.WindowSpec._fields_}
    assert offs == {"kind": 0, "op": 4, "window": 8, "min_periods": 16, "center": 24, "reserved": 28, "ddof": 32, "alpha": 40}
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef struct pandrs_hip_window_spec {"):header.index("} pandrs_hip_window_spec;")]
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(built.WindowSpec._fields_)
    for name, value in (("PANDRS_HIP_WINDOW_KIND_ROLLING", built.WINDOW_KIND_ROLLING), ("PANDRS_HIP_WINDOW_KIND_EWM", built.WINDOW_KIND_EWM),
                        ("PANDRS_HIP_WINDOW_SUM", built.WINDOW_SUM), ("PANDRS_HIP_WINDOW_COUNT", built.WINDOW_COUNT)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    name = "pandrs_hip_window"
    assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
    assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
    hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
    assert len(hp) == len(rp) == len(cp) == 7
    for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
        assert hn == rn and ht == rt, (hn, ht, rt)
        assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert [n for n, _ in hdr[1]["pandrs_hip_window_spec"]] == ["kind", "op", "window", "min_periods", "center", "reserved", "ddof", "alpha"]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- window statistics"):header.index("typedef enum pandrs_hip_window_kind")]
    for word in ("series/window.rs", "window.rs:13-160", "-0.0", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "2^32",
                 "INVALID_ARGUMENT", "total order", "1e-9", "1e-12", "squared"):
        assert word in block, word


def test_cpp_mirror_window_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "window_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
