"""PandasCompatExt's value_counts / unique / nunique / mode / is_unique (reference src/dataframe/pandas_compat/functions.rs:343-384,
:775-788, :1709-1753, :4120-4139, :4226-4259): the parts that need no GPU - the mirror's methods over a numpy stand-in context,
the errors raised before any device call, the C ABI entry points without a device, the header / ctypes / Rust declarations, the
option name and the geometry the header states, and the C++ mirror's methods compiled against the header."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import distinct_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("value_counts", "value_counts_numeric", "unique", "unique_numeric", "nunique", "nunique_all", "mode_numeric", "mode_string",
           "mode_with_count", "is_unique")


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
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in METHODS:
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.distinct) and callable(E.Context.distinct_fetch)
    assert (built.DISTINCT_BY_VALUE, built.DISTINCT_BY_COUNT) == (0, 1) == (R.BY_VALUE, R.BY_COUNT)
    assert (built.DISTINCT_NUMBER, built.DISTINCT_NAN, built.DISTINCT_NULL) == (0, 1, 2) == (R.NUMBER, R.NAN, R.NULL)
    assert C.sizeof(built.DistinctInfo) == 56


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    one_column = [m for m in METHODS if m not in ("nunique", "nunique_all")]
    for name in one_column:
        with pytest.raises(F.ColumnNotFound):
            getattr(df, name)("nope")
    for name in ("value_counts_numeric", "unique_numeric", "mode_numeric", "mode_with_count"):
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                getattr(df, name)(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value), name
    for col in ("id", "x", "flag"):
        with pytest.raises(F.ColumnTypeMismatch) as e:
            df.mode_string(col)
        assert "Column '%s' is not a string type" % col in str(e.value)
    # no rows: nothing to count, no device call
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Float64Column([]))
    empty.add_column("s", F.StringColumn([]))
    assert empty.value_counts_numeric("a") == [] and empty.unique_numeric("a") == [] and empty.mode_numeric("a") == []
    assert empty.value_counts("s") == [] and empty.unique("s") == [] and empty.mode_string("s") == []
    m, c = empty.mode_with_count("a")
    assert m != m and c == 0
    assert empty.is_unique("a") and empty.nunique() == [("a", 0), ("s", 0)] and empty.nunique_all() == {"a": 0, "s": 0}


def test_mirrors_on_the_stand_in(built, monkeypatch):
    """The mirrors against tests/distinct_ref.py's line-by-line loops, the device calls answered by the numpy twin: return
    shapes, the null cell as NaN (numeric) or "" (string), the documented tie rule, one device call per method and column."""
    import pandrs_amd.frame as F
    ctx = R.Stand()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    rng = np.random.default_rng(5)
    columns = [np.array([1.0, 2.5, 4.0, 2.5]), np.array([1.0, np.nan, 3.0, 1.0, np.nan]), np.arange(1.0, 9.0),
               rng.integers(-3, 4, 100).astype(np.float64), rng.normal(0, 10, 50).round(0) + 0.0, np.full(7, 3.25), np.array([math.inf, -math.inf, 1.0, math.inf])]
    for v in columns:
        df = F.OptimizedDataFrame()
        df.add_column("v", F.Float64Column(v.tolist()))
        vals = v.tolist()
        assert R.deterministic(vals)
        n_nan = int(np.isnan(v).sum())
        ctx.calls.clear()
        got = df.value_counts_numeric("v")
        assert [c[0] for c in ctx.calls] == ["distinct"] and ctx.calls[0][3] == R.BY_COUNT
        want = R.value_counts_numeric_loop(vals)
        assert [e for e in got if e[0] == e[0]] == sorted((e for e in want if e[0] == e[0]), key=lambda e: (-e[1], e[0]))
        assert [e[1] for e in got if e[0] != e[0]] == ([n_nan] if n_nan else []) and [c for _, c in got] == sorted((c for _, c in got), reverse=True)
        uniq = df.unique_numeric("v")
        assert [x for x in uniq if x == x] == sorted(x for x in R.unique_numeric_loop(vals) if x == x) and (uniq[-1] != uniq[-1]) == bool(n_nan)
        assert df.mode_numeric("v") == R.mode_numeric_loop(vals)
        m, c = df.mode_with_count("v")
        assert c == R.mode_with_count_loop(vals)[1] and m == min(R.mode_numeric_loop(vals))       # ties: the smallest
        assert df.is_unique("v") == R.is_unique_loop(vals)
        assert df.nunique_all() == R.nunique_all_loop({"v": vals}, {})
        assert df.nunique() == R.nunique_loop([("v", [F.rust_f64_to_string(x) for x in vals])])
        assert df.value_counts("v") == R.value_counts_loop([F.rust_f64_to_string(x) for x in vals])
        assert df.unique("v") == R.unique_loop([F.rust_f64_to_string(x) for x in vals])
    # strings through the pool and its rank table
    words = ["pear", "apple", "fig", "apple", "", "pear", "apple", "Zed", "zed", ""]
    df = F.OptimizedDataFrame()
    df.add_column("s", F.StringColumn(words))
    ctx.calls.clear()
    assert df.value_counts("s") == R.value_counts_loop(words) == [("apple", 3), ("", 2), ("pear", 2), ("Zed", 1), ("fig", 1), ("zed", 1)]
    assert ctx.calls == [("distinct", R.U32CODE, 10, R.BY_COUNT, True)]
    assert df.unique("s") == R.unique_loop(words) and df.mode_string("s") == R.mode_string_loop(words) == ["apple"]
    assert df.nunique() == [("s", 6)] and df.nunique_all() == {"s": 6} and not df.is_unique("s")
    # a null cell: NaN for a numeric column, "" for a string column; nunique_all and is_unique leave it out
    df = _frame()
    got = df.value_counts_numeric("x")
    assert got[:3] == [(0.5, 1), (1.0, 1), (2.0, 1)] and got[3][0] != got[3][0] and got[3][1] == 1
    assert df.unique_numeric("x")[:3] == [0.5, 1.0, 2.0] and len(df.unique_numeric("x")) == 4
    assert df.value_counts_numeric("id") == [(1.0, 1), (2.0, 1), (3.0, 1), (4.0, 1)]
    assert df.nunique_all() == {"id": 4, "x": 3, "s": 4, "flag": 2} and df.is_unique("x") and not df.is_unique("flag")
    assert df.nunique() == [("id", 4), ("x", 4), ("s", 4), ("flag", 2)]
    assert df.value_counts("flag") == [("false", 2), ("true", 2)] and df.value_counts("x") == [("0.5", 1), ("1", 1), ("2", 1), ("NaN", 1)]
    sn = F.OptimizedDataFrame()
    sn.add_column("s", F.StringColumn.with_nulls(["x", "y", "x", "", "y"], [False, True, False, False, False]))
    assert sn.value_counts("s") == [("", 2), ("x", 2), ("y", 1)] and sn.mode_string("s") == ["x"] and sn.unique("s") == ["", "x", "y"]
    # the merged NaN entry takes its place by count
    df = F.OptimizedDataFrame()
    df.add_column("v", F.Float64Column.with_nulls([1.0, 1.0, 1.0, math.nan, 9.0, 2.0, 2.0, 7.0], [False] * 4 + [True] + [False] * 3))
    got = df.value_counts_numeric("v")
    assert got[0] == (1.0, 3) and got[1] == (2.0, 2) and got[2][0] != got[2][0] and got[2][1] == 2 and got[3] == (7.0, 1)
    # -0.0 and 0.0 stay apart, -0.0 first; Int64 beyond 2^53 stays apart
    df = F.OptimizedDataFrame()
    df.add_column("z", F.Float64Column([0.0, -0.0, 0.0, -0.0]))
    df.add_column("big", F.Int64Column([1 << 53, (1 << 53) + 1, 1 << 53, 5]))
    u = df.unique_numeric("z")
    assert len(u) == 2 and math.copysign(1.0, u[0]) == -1.0 and math.copysign(1.0, u[1]) == 1.0
    assert math.copysign(1.0, df.mode_with_count("z")[0]) == -1.0 and df.mode_with_count("z")[1] == 2
    assert [c for _, c in df.value_counts_numeric("big")] == [2, 1, 1] and df.nunique_all()["big"] == 3


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    info = built.DistinctInfo()
    info.n_entries = -5
    rank = np.arange(4, dtype=np.uint32)
    H = built.MEM_HOST
    out_v, out_f, out_k = np.full(8, 7, np.uint64), np.full(8, 7, np.uint8), np.full(8, 7, np.int64)
    assert lib.pandrs_hip_distinct(None, H, C.byref(col), 8, 0, None, 0, C.byref(info)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    assert lib.pandrs_hip_distinct_fetch(None, H, out_v.ctypes.data, out_f.ctypes.data, out_k.ctypes.data) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    call = lambda c, n, order, r, nc, o: lib.pandrs_hip_distinct(h, H, c, n, order, r, nc, o)                # noqa: E731
    good = (C.byref(col), 8, 0, None, 0, C.byref(info))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, -1), (2, 2), (4, -1), (5, None)):
        args = list(good)
        args[i] = bad
        assert call(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_distinct(h, 7, *good) == built.ERR_INVALID_ARGUMENT
    assert call(C.byref(col), 8, 0, rank.ctypes.data, 4, C.byref(info)) == built.ERR_INVALID_ARGUMENT and "rank table" in built.last_error()
    other = built.Column()
    other.data = x.ctypes.data
    other.dtype = built.CELL64
    assert call(C.byref(other), *good[1:]) == built.ERR_INVALID_ARGUMENT and "dtype" in built.last_error()
    other.dtype = 9
    assert call(C.byref(other), *good[1:]) == built.ERR_INVALID_ARGUMENT
    other.dtype = built.U32CODE
    assert call(C.byref(other), 8, 0, rank.ctypes.data, 0, C.byref(info)) == built.ERR_INVALID_ARGUMENT      # a rank table of no codes
    none = built.Column()
    none.dtype = built.F64
    assert call(C.byref(none), *good[1:]) == built.ERR_INVALID_ARGUMENT                                       # rows but no data
    assert lib.pandrs_hip_distinct_fetch(h, 7, None, None, None) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_distinct_fetch(h, H, out_v.ctypes.data, out_f.ctypes.data, out_k.ctypes.data) == built.ERR_INVALID_ARGUMENT
    assert "retained" in built.last_error()
    # (a 0-row call is a call like any other, with a timings record of its own: it needs the device, tests/test_gpu_distinct.py)
    assert info.n_entries == -5 and (out_v == 7).all() and (out_f == 7).all() and (out_k == 7).all()


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_distinct": ["ctx", "mem_space", "col", "n_rows", "order", "code_rank", "n_codes", "out_info"],
             "pandrs_hip_distinct_fetch": ["ctx", "out_mem_space", "out_values", "out_flags", "out_counts"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    # the info struct: the same fields, in order, on all three sides
    fields = ["n_entries", "n_valid", "nan_count", "null_count", "max_count", "n_modes", "path", "reserved"]
    assert [n for n, _ in hdr[1]["pandrs_hip_distinct_info"]] == fields == [n for n, _ in built.DistinctInfo._fields_]
    assert [n for n, _ in rst[1]["PandrsHipDistinctInfo"]] == fields
    assert [t for _, t in hdr[1]["pandrs_hip_distinct_info"]] == ["i64"] * 6 + ["i32"] * 2 == [t for _, t in rst[1]["PandrsHipDistinctInfo"]]
    assert hdr[3]["PANDRS_HIP_DISTINCT_BY_VALUE"] == 0 == rst[2]["PANDRS_HIP_DISTINCT_BY_VALUE"]
    assert hdr[3]["PANDRS_HIP_DISTINCT_BY_COUNT"] == 1 == rst[2]["PANDRS_HIP_DISTINCT_BY_COUNT"]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- distinct values of one column and their counts"):header.index("typedef enum pandrs_hip_distinct_order")]
    for word in ("functions.rs:343-384", ":775-788", ":1709-1753", ":4120-4139", ":4226-4259", "canonical NaN", "-0.0 and 0.0 are two", "to_bits",
                 "never looked at", "sum to n_rows", "-0.0 before 0.0", "code_rank[code]", "byte-wise", "no fault", "count descending",
                 "bit for bit", "Deviations", "NaN payloads apart", "HashMap order", "2^53", "unsigned 64-bit", "does not wrap", "by ballot",
                 "does not\n * serialise", "cannot overflow below 2^32", "No workgroup waits", "Geometry", "distinct_direct_max_cells = ",
                 "distinct_tile_rows = ", "distinct_blocks_per_cu = ", "160 KiB", "distinct_path", "n_partitions", "Retained state",
                 "invalidates the retained groupby result", "join result", "groupby_indices", "Buffers", "Workspace", "written before it is read",
                 "Errors", "NOT_INITIALIZED", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "INVALID_ARGUMENT", "CELL64", "2^32", "n_rows ==\n * 0",
                 "Out of scope", "2^31 and 2^32", "untested", "drop_duplicates", "crosstab", "multi-GPU"):
        assert word in block, word


def test_option_and_geometry_in_the_header_are_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "distinct.hip")).read()
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    capi = open(os.path.join(ROOT, "pandrs_amd", "csrc", "capi.hip")).read()
    threads = int(re.search(r"DN_THREADS = (\d+);", src).group(1))
    loads = int(re.search(r"DN_LOADS = (\d+);", src).group(1))
    assert "DN_TILE = DN_THREADS * DN_LOADS * 2;" in src
    assert int(re.search(r"distinct_tile_rows = (\d+)", header).group(1)) == threads * loads * 2
    blocks = int(re.search(r"DN_BLOCKS_PER_CU = (\d+);", src).group(1))
    assert int(re.search(r"distinct_blocks_per_cu = (\d+)", header).group(1)) == blocks
    cells = int(re.search(r"DN_MAX_CELLS = (\d+);", src).group(1))
    assert int(re.search(r"distinct_direct_max_cells = (\d+)", header).group(1)) == cells
    assert cells * 4 == 32 * 1024 and blocks * cells * 4 <= 160 * 1024 and threads == 256        # four tables per compute unit fit its LDS
    assert '"distinct_path"' in header and 'std::strcmp(name, "distinct_path")) c->opt.distinct_path = value;' in capi
    assert "c->opt.distinct_path" in src
    common = open(os.path.join(ROOT, "pandrs_amd", "csrc", "common.hpp")).read()
    begin = common[common.index("inline void timings_begin("):]
    assert "c->dn.valid = false;" in begin[:begin.index("}")]                                     # every compute call drops the retained list
    # both entry points sit behind the exception firewall, and the Makefile builds the file
    for name in ("pandrs_hip_distinct", "pandrs_hip_distinct_fetch"):
        assert re.search(r"int32_t %s\([^{;]*\) try \{" % name, capi) and 'on_exception("%s")' % name in capi
    assert "distinct.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()


def test_cpp_mirror_distinct_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "distinct_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "distinct_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
