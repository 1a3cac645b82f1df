"""The window median / quantile without a GPU: the mirror's methods (rolling_median, apply_rolling / apply_expanding and
their operations; reference helpers/window_ops.rs:206-240, dataframe/enhanced_window.rs), errors raised before any device
call, empty frames, the builder's column naming and target-column choice, the C ABI entry point without a device, the
header / ctypes / Rust declarations and struct layout, and the C++ mirror compiled against the header."""
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


class _Recorder:
    """Stands in for the context: records every call and answers with its index."""

    def __init__(self):
        self.calls = []

    def window(self, view, n, kind, op, **kw):
        self.calls.append(("window", kind, op, kw))
        return np.full(n, float(len(self.calls)))

    def window_quantile(self, view, n, kind, **kw):
        self.calls.append(("window_quantile", kind, kw))
        return np.full(n, float(len(self.calls)))


def test_mirror_has_the_methods(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("rolling_median", "apply_rolling", "apply_expanding"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    for cls in (F.DataFrameRollingOps, F.DataFrameExpandingOps):
        for name in ("mean", "sum", "std", "var", "min", "max", "count", "median", "quantile"):
            assert callable(getattr(cls, name)), (cls, name)
    cfg = F.DataFrameRolling(5).min_periods(2).center(True).columns(["x"])
    assert isinstance(cfg, F.DataFrameRolling) and cfg.window_size == 5
    assert isinstance(F.DataFrameExpanding(1).columns(["x"]), F.DataFrameExpanding)
    assert callable(E.Context.window_quantile)
    for doc in (F.OptimizedDataFrame.rolling.__doc__, F.OptimizedDataFrame.expanding.__doc__):     # where median lives
        assert "median" in doc and "apply_" in doc


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    R, E = F.DataFrameRolling, F.DataFrameExpanding
    with pytest.raises(F.ColumnNotFound):
        df.rolling_median("nope", 3)
    for col in ("s", "flag"):
        with pytest.raises(F.ColumnTypeMismatch) as e:
            df.rolling_median(col, 3)
        assert "'%s'" % col in str(e.value)
        for ops in (df.apply_rolling(R(3).columns([col])), df.apply_expanding(E(1).columns(["id", col]))):
            for call in (ops.median, lambda ops=ops: ops.quantile(0.5), ops.mean):
                with pytest.raises(F.ColumnTypeMismatch):
                    call()
    for ops in (df.apply_rolling(R(3).columns(["x", "nope"])), df.apply_expanding(E(1).columns(["nope"]))):
        for call in (ops.median, lambda ops=ops: ops.quantile(0.5), ops.sum):
            with pytest.raises(F.ColumnNotFound):
                call()
    for call in (lambda: df.apply_rolling(R(0)).median(), lambda: df.apply_rolling(R(0)).quantile(0.5), lambda: df.apply_rolling(R(0)).max()):
        with pytest.raises(F.InvalidValue) as e:                       # series/window.rs:112-117
            call()
        assert str(e.value) == "Window size must be greater than 0"
    for q in (1.5, -0.1, float("nan"), float("inf")):                   # series/window.rs:318-322, :514-518 (NaN: rejected here)
        for ops in (df.apply_rolling(R(3)), df.apply_expanding(E(1))):
            with pytest.raises(F.InvalidValue) as e:
                ops.quantile(q)
            assert str(e.value) == "Quantile must be between 0 and 1"
    df.add_column("x_median", F.Float64Column([0.0] * 4))
    df.add_column("id_quantile", F.Float64Column([0.0] * 4))
    with pytest.raises(F.DuplicateColumnName):
        df.apply_rolling(R(2).columns(["x"])).median()
    with pytest.raises(F.DuplicateColumnName):
        df.apply_expanding(E(1)).quantile(0.5)
    with pytest.raises(F.DuplicateColumnName):
        df.apply_rolling(R(2).columns(["id", "id"])).median()
    # the string dispatch is unchanged
    with pytest.raises(F.InvalidValue) as e:
        df.rolling(2, "x", "median")
    assert "Unsupported rolling operation" in str(e.value)


def test_empty_frames_keep_the_shape_without_a_device(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("f", F.Float64Column([]))
    empty.add_column("s", F.StringColumn([]))
    got = empty.rolling_median("f", 3)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (0,)
    r = empty.apply_rolling(F.DataFrameRolling(3)).median()
    assert r.column_names == ["a", "f", "s", "a_median", "f_median"] and r.row_count() == 0
    assert isinstance(r.column("f_median"), F.Float64Column)
    r = empty.apply_expanding(F.DataFrameExpanding(0).columns(["f"])).quantile(0.25)
    assert r.column_names == ["a", "f", "s", "f_quantile"] and r.row_count() == 0
    assert empty.apply_rolling(F.DataFrameRolling(2)).count().column_names == ["a", "f", "s", "a_count", "f_count"]


def test_builder_names_targets_and_specs(built, monkeypatch):
    import pandrs_amd.frame as F
    L = built
    rec = _Recorder()
    monkeypatch.setattr(F, "get_context", lambda: rec)
    df = _frame()
    r = df.apply_rolling(F.DataFrameRolling(3)).median()                 # every Int64 / Float64 column, in frame order
    assert r.column_names == ["id", "x", "s", "flag", "id_median", "x_median"] and r.row_count() == 4
    assert [c[0] for c in rec.calls] == ["window_quantile"] * 2
    assert rec.calls[0][1] == L.WINDOW_KIND_ROLLING
    assert rec.calls[0][2] == dict(median=True, out_device=False, window=3, min_periods=3, center=False)    # enhanced_window.rs:325
    assert list(r.column("x_median").data) == [2.0] * 4 and r.column("x_median").null_mask is None
    assert r.column("id") is df.column("id")
    rec.calls.clear()
    r = df.apply_rolling(F.DataFrameRolling(5).min_periods(2).center(True).columns(["x", "id"])).quantile(0.9)
    assert r.column_names == ["id", "x", "s", "flag", "x_quantile", "id_quantile"]                            # the configured order
    assert rec.calls[0][2] == dict(median=False, q=0.9, out_device=False, window=5, min_periods=2, center=True)
    rec.calls.clear()
    r = df.apply_expanding(F.DataFrameExpanding(2).columns(["x"])).median()
    assert r.column_names[-1] == "x_median" and rec.calls == [("window_quantile", L.WINDOW_KIND_EXPANDING,
                                                                dict(median=True, out_device=False, min_periods=2))]
    rec.calls.clear()
    r = df.apply_expanding(F.DataFrameExpanding(0)).quantile(0.0)
    assert r.column_names[-2:] == ["id_quantile", "x_quantile"] and rec.calls[1][2]["q"] == 0.0
    rec.calls.clear()
    for name, op, args in (("mean", L.WINDOW_MEAN, ()), ("sum", L.WINDOW_SUM, ()), ("std", L.WINDOW_STD, (0,)), ("var", L.WINDOW_VAR, (2,)),
                           ("min", L.WINDOW_MIN, ()), ("max", L.WINDOW_MAX, ()), ("count", L.WINDOW_COUNT, ())):
        r = getattr(df.apply_rolling(F.DataFrameRolling(2).columns(["x"])), name)(*args)
        assert r.column_names[-1] == "x_" + name
        kind, got_op, kw = rec.calls[-1][1:]
        assert (kind, got_op) == (L.WINDOW_KIND_ROLLING, op) and kw["window"] == 2 and kw["ddof"] == (args[0] if args else 1)
        r = getattr(df.apply_expanding(F.DataFrameExpanding(1).columns(["id"])), name)(*args)
        assert r.column_names[-1] == "id_" + name and rec.calls[-1][1:3] == (L.WINDOW_KIND_EXPANDING, op)
    rec.calls.clear()
    got = df.rolling_median("x", 0, None)                                # window 0 acts as 1; min_periods stays the caller's window
    assert rec.calls == [("window_quantile", L.WINDOW_KIND_ROLLING, dict(median=True, window=1, min_periods=0, nan_missing=True, out_device=False))]
    assert isinstance(got, np.ndarray)
    df.rolling_median("id", 7, 2)
    assert rec.calls[-1][2] == dict(median=True, window=7, min_periods=2, nan_missing=True, out_device=False)


def test_entry_point_without_a_gpu_is_not_initialized(built):
    lib = built.load()
    n = C.c_int32(-1)
    assert lib.pandrs_hip_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("a GPU is present")
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    spec = built.WindowQuantileSpec(kind=built.WINDOW_KIND_ROLLING, median=1, window=3, min_periods=-1, center=0, nan_missing=0, q=0.5)
    out = np.empty(8)
    st = lib.pandrs_hip_window_quantile(None, built.MEM_HOST, C.byref(col), 8, C.byref(spec), built.MEM_HOST, out.ctypes.data)
    assert st == built.ERR_NOT_INITIALIZED and "context" in built.last_error()


def test_spec_layout_matches_the_header(built):
    assert C.sizeof(built.WindowQuantileSpec) == 40
    offs = {name: getattr(built.WindowQuantileSpec, name).offset for name, _ in built.WindowQuantileSpec._fields_}
    assert offs == {"kind": 0, "median": 4, "window": 8, "min_periods": 16, "center": 24, "nan_missing": 28, "q": 32}
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef struct pandrs_hip_window_quantile_spec {"):header.index("} pandrs_hip_window_quantile_spec;")]
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, re.M)
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(built.WindowQuantileSpec._fields_)


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    name = "pandrs_hip_window_quantile"
    assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
    assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
    hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
    assert [n for n, _ in hp] == ["ctx", "mem_space", "col", "n_rows", "spec", "out_mem_space", "out"]
    assert len(hp) == len(rp) == len(cp) == 7
    for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
        assert hn == rn and ht == rt, (hn, ht, rt)
        assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert [n for n, _ in hdr[1]["pandrs_hip_window_quantile_spec"]] == ["kind", "median", "window", "min_periods", "center", "nan_missing", "q"]
    assert "PandrsHipWindowQuantileSpec" in rst[1]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- window order statistics"):header.index("typedef struct pandrs_hip_window_quantile_spec")]
    for word in ("series/window.rs:298-336", ":494-530", "window_ops.rs:206-240", "enhanced_window.rs", "half away from zero", "-0.0",
                 "row order", "panics", "NaN q", "total order", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "2^32",
                 "INVALID_ARGUMENT", "window_quantile_path"):
        assert word in block, word
    window_block = header[header.index("/* ---- window statistics"):header.index("typedef enum pandrs_hip_window_kind")]
    assert "pandrs_hip_window_quantile" in window_block and "Out of scope: median" not in window_block
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "window_quantile.hip")).read()
    direct_max = int(re.search(r"constexpr int WQ_DIRECT_MAX = (\d+);", src).group(1))
    assert "at most %d rows" % direct_max in header                       # the header's figure is the kernel's


def test_cpp_mirror_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "window_quantile_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "window_quantile_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
