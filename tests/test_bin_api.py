"""PandasCompatExt's value_range / cut / qcut (reference src/dataframe/pandas_compat/functions.rs:2270-2282, :2339-2420): the
parts that need no GPU - the mirror's methods, label strings, row dropping and errors (raised before any device call), the C ABI
entry points without a device, the header / ctypes / Rust declarations, the option name and the geometry the header states,
and the C++ mirror's methods compiled against the header."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bin_ref as R

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


class NumpyContext:
    """The CPU stand-in: Context.bin_edges / Context.bin / Context.column_stats answered by tests/bin_ref.py's fast twin, and
    a record of the calls."""
    device = 0

    def __init__(self):
        self.calls = []

    @staticmethod
    def _values(col, n):
        data, mask, _ = col
        null = None if mask is None else np.unpackbits(np.asarray(mask, np.uint8), bitorder="little")[:n].astype(bool)
        return R.values_of(np.asarray(data)[:n], null)

    def column_stats(self, col, n):
        self.calls.append(("stats", col[2], n))
        v = self._values(col, n)
        v = v[~np.isnan(v)]
        return {"min": v.min() if v.size else math.inf, "max": v.max() if v.size else -math.inf}

    def bin_edges(self, col, n_rows, kind, k):
        self.calls.append(("edges", col[2], n_rows, kind, k))
        v = self._values(col, n_rows)
        valid = int((~np.isnan(v)).sum())
        if not valid:
            return np.full(k + 1, np.nan), 0
        return (R.cut_edges(v, k) if kind == 0 else R.qcut_edges(v, k)), valid

    def bin(self, col, n_rows, edges, out_device=None, want_counts=True, out=None, want_codes=True):
        self.calls.append(("bin", col[2], n_rows, np.array(edges), out_device, want_counts))
        codes, counts = R.codes(self._values(col, n_rows), edges)
        return codes, (counts if want_counts else None)


def test_mirror_has_the_methods(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("value_range", "cut", "qcut", "bin_codes"):
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.bin) and callable(E.Context.bin_edges)
    assert (built.BIN_CUT, built.BIN_QCUT, built.BIN_NONE, built.BIN_NAN) == (0, 1, -1, -2) == (0, 1, R.NONE, R.NAN)


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    calls = {"value_range": lambda c: df.value_range(c), "cut": lambda c: df.cut(c, 3), "qcut": lambda c: df.qcut(c, 3),
             "bin_codes": lambda c: df.bin_codes(c, [0.0, 1.0])}
    for name, call in calls.items():
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value), name
    with pytest.raises(F.InvalidValue, match="Number of bins must be > 0"):
        df.cut("x", 0)                                                             # test_cut_zero_bins, functions.rs:6973-6977
    with pytest.raises(F.InvalidValue, match="Number of quantiles must be > 0"):
        df.qcut("x", 0)                                                            # test_qcut_zero_quantiles, :7013-7018
    for fn in (df.cut, df.qcut):
        with pytest.raises(F.InvalidValue):
            fn("x", built.BIN_MAX_BINS + 1)
    for bad in ([1.0], [2.0, 1.0], [0.0, math.nan], list(range(built.BIN_MAX_BINS + 2))):
        with pytest.raises(F.InvalidValue):
            df.bin_codes("x", bad)
    # no rows: no valid value, as the reference's value_range / qcut on an empty column; bin_codes has nothing to answer
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Float64Column([]))
    for fn in (lambda: empty.value_range("a"), lambda: empty.cut("a", 2), lambda: empty.qcut("a", 2)):
        with pytest.raises(F.InvalidValue, match="No valid values"):
            fn()
    codes, counts = empty.bin_codes("a", [0.0, 1.0, 2.0])
    assert codes.dtype == np.int32 and codes.size == 0 and counts.tolist() == [0, 0, 0, 0]


def test_labels_and_row_dropping_on_the_stand_in(built, monkeypatch):
    """The mirrors against tests/bin_ref.py's line-by-line loops, the device calls answered by the numpy twin: the label
    strings, the rows cut leaves out, qcut's "", the null cell as NaN, the non-finite case without a binning call, one
    edge call and one binning call each."""
    import pandrs_amd.frame as F
    ctx = NumpyContext()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    rng = np.random.default_rng(5)
    columns = [np.array([1.0, 2.5, 4.0, 5.0]), np.array([1.0, np.nan, 3.0]), np.arange(1.0, 9.0), np.array([1.0, np.nan, 3.0, 4.0]),
               np.array([0.0, 1e15, 5e14]), 2.0 ** 52 + rng.integers(0, 64, 50).astype(np.float64), np.full(7, 3.25),
               rng.normal(0, 10, 200), rng.integers(-3, 4, 100).astype(np.float64), np.array([-0.4, 0.0, 0.3])]
    for v in columns:
        df = F.OptimizedDataFrame()
        df.add_column("v", F.Float64Column(v.tolist()))
        for k in (1, 2, 3, 7, 40):
            ctx.calls.clear()
            assert df.cut("v", k) == R.cut_loop(v, k), (v, k)
            assert [c[0] for c in ctx.calls] == ["edges", "bin"] and ctx.calls[1][4] is False and ctx.calls[1][5] is False
            ctx.calls.clear()
            assert df.qcut("v", k) == R.qcut_loop(v, k), (v, k)
            assert [c[0] for c in ctx.calls] == ["edges", "bin"]
            last = ctx.calls[1][3]
            assert last[-1] == R.qcut_edges(v, k)[-1] + 0.001                      # the caller's + 0.001
        assert df.value_range("v") == R.value_range_loop(v)
    # cut drops the maximum at 1e15; the reference's list is shorter than the column
    df = F.OptimizedDataFrame()
    df.add_column("v", F.Float64Column([0.0, 1e15, 5e14]))
    assert df.cut("v", 2) == ["(0.00, 500000000000000.00]", "(500000000000000.00, 1000000000000000.00]"]
    # Int64 cells `as f64`, a null cell as NaN
    df = _frame()
    assert df.qcut("id", 2) == R.qcut_loop(np.array([1.0, 2.0, 3.0, 4.0]), 2) == ["Q1", "Q1", "Q2", "Q2"]
    x = np.array([0.5, np.nan, 1.0, 2.0])
    assert df.cut("x", 2) == R.cut_loop(x, 2) and df.cut("x", 2)[1] == "NaN"
    assert df.qcut("x", 3) == R.qcut_loop(x, 3)
    assert df.value_range("x") == (0.5, 2.0)
    # a width that is not finite: answered from the NaN count, no binning call
    for cells in ([1.0, math.inf], [-math.inf, 2.0], [-1e308, 1e308], [math.inf], [-math.inf, math.inf]):
        for extra in ([], [math.nan, math.nan]):
            df = F.OptimizedDataFrame()
            df.add_column("v", F.Float64Column(cells + extra))
            ctx.calls.clear()
            assert df.cut("v", 3) == ["NaN"] * len(extra) == R.cut_loop(np.array(cells + extra), 3)
            assert [c[0] for c in ctx.calls] == ["edges"]
    # no valid cell
    df = F.OptimizedDataFrame()
    df.add_column("v", F.Float64Column([math.nan, math.nan]))
    for fn in (lambda: df.cut("v", 2), lambda: df.qcut("v", 2), lambda: df.value_range("v")):
        with pytest.raises(F.InvalidValue, match="No valid values"):
            fn()
    # bin_codes: the codes and the counts of one call
    df = F.OptimizedDataFrame()
    df.add_column("v", F.Float64Column([-1.0, 0.0, 0.5, 1.0, 5.0, math.nan]))
    codes, counts = df.bin_codes("v", [0.0, 1.0, 2.0])
    assert codes.tolist() == [-1, 0, 0, 1, -1, -2] and counts.tolist() == [2, 1, 2, 1]


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    edges = np.array([0.0, 2.0, 4.0, 8.0])
    ep = edges.ctypes.data_as(C.POINTER(C.c_double))
    codes = np.full(8, 0x5A5A5A5A, np.int32)
    counts = np.full(5, -7, np.int64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    out_e = np.full(4, 9.0)
    oe = out_e.ctypes.data_as(C.POINTER(C.c_double))
    valid = C.c_int64(-5)
    H = built.MEM_HOST
    assert lib.pandrs_hip_bin(None, H, C.byref(col), 8, ep, 3, H, codes.ctypes.data, cp) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    assert lib.pandrs_hip_bin_edges(None, H, C.byref(col), 8, built.BIN_CUT, 3, oe, C.byref(valid)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    call = lambda c, n, e, nb, o, pc: lib.pandrs_hip_bin(h, H, c, n, e, nb, H, o, pc)                       # noqa: E731
    good = (C.byref(col), 8, ep, 3, codes.ctypes.data, cp)
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, None), (3, 0), (3, -1), (3, built.BIN_MAX_BINS + 1)):
        args = list(good)
        args[i] = bad
        assert call(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert call(C.byref(col), 8, ep, 3, None, None) == built.ERR_INVALID_ARGUMENT                            # nothing asked for
    assert call(C.byref(col), 8, ep, 3, codes.ctypes.data + 2, cp) == built.ERR_INVALID_ARGUMENT and "4-byte" in built.last_error()
    assert lib.pandrs_hip_bin(h, 7, C.byref(col), 8, ep, 3, H, codes.ctypes.data, cp) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_bin(h, H, C.byref(col), 8, ep, 3, 7, codes.ctypes.data, cp) == built.ERR_INVALID_ARGUMENT
    for bad_edges in ([0.0, 2.0, 1.0, 8.0], [0.0, math.nan, 4.0, 8.0], [math.nan, 2.0, 4.0, 8.0], [0.0, 2.0, 4.0, math.nan]):
        be = np.array(bad_edges)
        assert call(C.byref(col), 8, be.ctypes.data_as(C.POINTER(C.c_double)), 3, codes.ctypes.data, cp) == built.ERR_INVALID_ARGUMENT, bad_edges
        assert "edge" in built.last_error()
    other = built.Column()
    other.data = x.ctypes.data
    for dt in (built.U32CODE, built.BOOLBITS, built.CELL64):
        other.dtype = dt
        assert call(C.byref(other), *good[1:]) == built.ERR_TYPE_MISMATCH, dt
        assert lib.pandrs_hip_bin_edges(h, H, C.byref(other), 8, built.BIN_QCUT, 3, oe, C.byref(valid)) == built.ERR_TYPE_MISMATCH, dt
    ecall = lambda c, n, kind, k, o, pv: lib.pandrs_hip_bin_edges(h, H, c, n, kind, k, o, pv)                # noqa: E731
    good_e = (C.byref(col), 8, built.BIN_CUT, 3, oe, C.byref(valid))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, -1), (2, 2), (3, 0), (3, built.BIN_MAX_BINS + 1), (4, None), (5, None)):
        args = list(good_e)
        args[i] = bad
        assert ecall(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_bin_edges(h, 7, C.byref(col), 8, built.BIN_CUT, 3, oe, C.byref(valid)) == built.ERR_INVALID_ARGUMENT
    assert (codes == 0x5A5A5A5A).all() and (out_e == 9.0).all()
    # nothing to do is OK: no code written, the counts all zero; no valid cell: the edges NaN
    assert call(C.byref(col), 0, ep, 3, codes.ctypes.data, cp) == 0
    assert (codes == 0x5A5A5A5A).all() and counts.tolist() == [0, 0, 0, 0, 0]
    for kind in (built.BIN_CUT, built.BIN_QCUT):
        out_e[:] = 9.0
        valid.value = -5
        assert ecall(C.byref(col), 0, kind, 3, oe, C.byref(valid)) == 0 and valid.value == 0 and np.isnan(out_e).all()


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_bin": ["ctx", "mem_space", "col", "n_rows", "edges", "n_bins", "out_mem_space", "out_codes", "out_counts"],
             "pandrs_hip_bin_edges": ["ctx", "mem_space", "col", "n_rows", "kind", "k", "out_edges", "out_valid"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert hdr[3]["PANDRS_HIP_BIN_CUT"] == 0 == rst[2]["PANDRS_HIP_BIN_CUT"] and hdr[3]["PANDRS_HIP_BIN_QCUT"] == 1 == rst[2]["PANDRS_HIP_BIN_QCUT"]
    assert hdr[2]["PANDRS_HIP_BIN_MAX_BINS"] == built.BIN_MAX_BINS == rst[2]["PANDRS_HIP_BIN_MAX_BINS"]
    assert re.search(r"#define PANDRS_HIP_BIN_NONE \(-1\)", header) and re.search(r"#define PANDRS_HIP_BIN_NAN \(-2\)", header)
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    assert g.parse_header()[0] and "pandrs_hip_abi_version" in h_funcs and "#define PANDRS_HIP_ABI_VERSION 1" in header
    block = header[header.index("/* ---- bins of one numeric column: cut, qcut, per-bin counts"):header.index("#define PANDRS_HIP_BIN_MAX_BINS")]
    for word in ("functions.rs:2270-2282", ":2339-2368", ":2370-2420", ":6840-6846", ":6943-7018", "max + 0.001", "FIRST", "2^43", "2^53",
                 "behaves as NaN", "bit for bit", "Signed zero", "-0.00", "no fused multiply-add", "Exactness", "Deviations", "Geometry",
                 "Buffers", "Workspace", "Errors", "Out of scope", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED",
                 "INVALID_ARGUMENT", "2^32", "bin_max_bins = ", "bin_tile_rows = ", "bin_blocks_per_cu = ", "bin_guess_min_bins = ", "bin_path",
                 "more than 4096 bins", "pandas-style", "second column's edges", "String columns", "2^31 and 2^32", "multi-GPU", "group_by"):
        assert word in block, word


def test_option_and_geometry_in_the_header_are_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "bin.hip")).read()
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    capi = open(os.path.join(ROOT, "pandrs_amd", "csrc", "capi.hip")).read()
    threads = int(re.search(r"BIN_THREADS = (\d+);", src).group(1))
    loads = int(re.search(r"BIN_LOADS = (\d+);", src).group(1))
    assert "BIN_TILE = BIN_THREADS * BIN_LOADS * 2;" in src
    assert int(re.search(r"bin_tile_rows = (\d+)", header).group(1)) == threads * loads * 2
    assert int(re.search(r"bin_blocks_per_cu = (\d+)", header).group(1)) == int(re.search(r"BIN_BLOCKS_PER_CU = (\d+);", src).group(1))
    assert int(re.search(r"bin_guess_min_bins = (\d+)", header).group(1)) == int(re.search(r"BIN_GUESS_MIN_BINS = (\d+);", src).group(1))
    max_bins = int(re.search(r"bin_max_bins = (\d+)", header).group(1))
    assert max_bins == built.BIN_MAX_BINS == int(re.search(r"#define PANDRS_HIP_BIN_MAX_BINS (\d+)", header).group(1))
    assert "BIN_MAX_BINS = PANDRS_HIP_BIN_MAX_BINS;" in src
    assert (max_bins + 1) * 8 == 32 * 1024 + 8 and (max_bins + 1) * 8 + (max_bins + 2) * 4 <= 64 * 1024       # edges, then the counters, in LDS
    assert int(re.search(r"at most (\d+) steps", header[header.index("/* ---- bins of one numeric column"):]).group(1)) == \
        int(re.search(r"BIN_FIX = (\d+);", src).group(1))
    assert '"bin_path"' in header and 'std::strcmp(name, "bin_path")) c->opt.bin_path = value;' in capi and "c->opt.bin_path" in src
    assert "fp contract(off)" in src and "fp contract(off)" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "describe.hip")).read()
    # the ranks by number share the selection's slot limit with the percentiles
    ds = open(os.path.join(ROOT, "pandrs_amd", "csrc", "describe.hip")).read()
    assert int(re.search(r"DS_MAX_P = (\d+);", ds).group(1)) * 2 == 32 and "DS_MAX_SLOTS = 2 * DS_MAX_P;" in ds
    assert "up to 32 distinct" in header and "ceil((k + 1) / 32)" in header


def test_cpp_mirror_bins_compile_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bin_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "bin_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
