"""crosstab / pivot_table / pivot / unstack (reference src/dataframe/pandas_compat/functions.rs:2138-2183, :2471-2527,
src/pivot/mod.rs:12-250): the parts that need no GPU - the mirror's methods over a numpy stand-in context, the errors raised
before any device call, the C ABI entry points without a device, the header / ctypes / Rust declarations, the option name and
the geometry the header states, and the C++ mirror's methods compiled against the header."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import pivot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("crosstab", "pivot_table", "pivot", "unstack")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from pandrs_amd import _lib
    return _lib


def _frame():
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("id", F.Int64Column([1, 2, 1, 2]))
    df.add_column("x", F.Float64Column.with_nulls([0.5, 0.25, 1.0, 2.0], [False, True, False, False]))
    df.add_column("s", F.StringColumn(["a", "b", "a", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    return df


def test_mirror_has_the_methods(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in METHODS:
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.pivot) and callable(E.Context.pivot_fetch)
    assert (built.PIVOT_ROWS, built.PIVOT_SUM, built.PIVOT_MEAN, built.PIVOT_MIN, built.PIVOT_MAX, built.PIVOT_COUNT, built.PIVOT_LAST) == R.OPS
    assert (built.PIVOT_NUMBER, built.PIVOT_MISSING) == (0, 1) == (R.NUMBER, R.MISSING)
    assert C.sizeof(built.PivotInfo) == 48
    # AggFunction: the order, names and from_str of pivot/mod.rs:12-48
    A = F.AggFunction
    assert [a.name() for a in A] == ["sum", "mean", "min", "max", "count"] and [int(a) for a in A] == [0, 1, 2, 3, 4]
    for text, want in (("sum", A.Sum), ("MEAN", A.Mean), ("avg", A.Mean), ("Average", A.Mean), ("min", A.Min), ("minimum", A.Min),
                       ("max", A.Max), ("MAXIMUM", A.Max), ("count", A.Count), ("median", None), ("", None)):
        assert A.from_str(text) is want, text


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    for args in (("nope", "s"), ("s", "nope")):
        with pytest.raises(F.ColumnNotFound):
            df.crosstab(*args)
        for name in ("pivot", "unstack"):
            with pytest.raises(F.ColumnNotFound):
                getattr(df, name)(*args, "x")
        with pytest.raises(F.ColumnNotFound):
            df.pivot_table(*args, "x", F.AggFunction.Sum)
    for name in ("pivot", "unstack"):
        with pytest.raises(F.ColumnNotFound):
            getattr(df, name)("s", "id", "nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                getattr(df, name)("id", "s", col)
            assert "Column '%s' is not a numeric type" % col in str(e.value)
    with pytest.raises(F.ColumnNotFound):
        df.pivot_table("s", "id", "nope", "sum")
    with pytest.raises(F.ColumnTypeMismatch):
        df.pivot_table("s", "id", "flag", "sum")
    with pytest.raises(F.InvalidValue):
        df.pivot_table("s", "id", "x", "median")
    # no rows: the (empty) index column alone, no device call
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.StringColumn([]))
    empty.add_column("b", F.Int64Column([]))
    empty.add_column("v", F.Float64Column([]))
    for out in (empty.crosstab("a", "b"), empty.pivot_table("a", "b", "v", "mean"), empty.pivot("a", "b", "v"), empty.unstack("b", "a", "v")):
        assert len(out.column_names) == 1 and out.row_count() == 0


def _strings(F, col):
    out = []
    for r in range(col.len()):
        v = col.get(r)
        if v is None:
            out.append("NaN" if col.dtype in (R.I64, R.F64) else "")
        elif col.dtype == R.F64:
            out.append(F.rust_f64_to_string(v))
        elif col.dtype == R.BOOLBITS:
            out.append("true" if v else "false")
        else:
            out.append(str(v))
    return out


def test_mirrors_on_the_stand_in(built, monkeypatch):
    """The mirrors against tests/pivot_ref.py's line-by-line loops, the device calls answered by the numpy twin: the frame's
    shape, the labels' strings and their byte-wise order, the missing cell as "NaN" / "", one device call per method."""
    import pandrs_amd.frame as F
    ctx = R.Stand()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    rng = np.random.default_rng(5)
    n = 300
    words = ["pear", "apple", "fig", "Zed", "zed", "é", "10", "9"]
    df = F.OptimizedDataFrame()
    df.add_column("s", F.StringColumn([words[i] for i in rng.integers(0, len(words), n)]))
    df.add_column("i", F.Int64Column(rng.integers(-3, 12, n)))
    df.add_column("f", F.Float64Column(rng.integers(0, 4, n) / 2.0))
    df.add_column("flag", F.BooleanColumn(rng.random(n) < 0.5))
    df.add_column("v", F.Float64Column(rng.integers(1, 999, n) / 8.0))
    vals = df.column("v").data.tolist()
    for a, b in (("s", "i"), ("i", "s"), ("f", "flag"), ("flag", "f"), ("s", "s")):
        sa, sb = _strings(F, df.column(a)), _strings(F, df.column(b))
        ctx.calls.clear()
        got = df.crosstab(a, b)
        assert [c[0] for c in ctx.calls] == ["pivot"] and ctx.calls[0][4] == R.ROWS and not ctx.calls[0][5]
        assert ctx.calls[0][6] == (a == "s") and ctx.calls[0][7] == (b == "s")                  # the rank table goes with a String column
        u1, u2, table = R.crosstab_loop(sa, sb)
        assert got.column_names == [a] + u2 and got.column(a).to_list() == u1
        for name in u2:
            assert got.column(name).data.tolist() == table[name] and got.column(name).null_mask is None
        if a == b:
            continue
        ui, uc, want = R.unstack_loop(sa, sb, vals)
        for method in ("unstack", "pivot"):
            ctx.calls.clear()
            got = getattr(df, method)(a, b, "v")
            assert [c[4] for c in ctx.calls] == [R.LAST]
            assert got.column_names == [a] + uc and got.column(a).to_list() == ui
            for name in uc:
                np.testing.assert_array_equal(got.column(name).data, np.array(want[name]))
                assert got.column(name).null_mask is None
        for fn, op in (("sum", R.SUM), ("mean", R.MEAN), ("min", R.MIN), ("max", R.MAX), ("count", R.COUNT)):
            il, cl, want = R.pivot_table_loop(sa, sb, vals, fn)
            for aggfunc in (fn, F.AggFunction.from_str(fn)):
                ctx.calls.clear()
                got = df.pivot_table(a, b, "v", aggfunc)
                assert [c[4] for c in ctx.calls] == [op]
                assert got.column_names == [a] + cl and got.column(a).to_list() == il
                for name in cl:
                    col = got.column(name)
                    cells = [None if col.is_null(r) else float(col.data[r]) for r in range(col.len())]
                    assert cells == want[name], (fn, name)
                    assert all(math.isnan(col.data[r]) for r in range(col.len()) if col.is_null(r))
    # a missing cell: "NaN" for a numeric key, "" for a String / Boolean key; merged with a literal "" in crosstab only
    df = F.OptimizedDataFrame()
    df.add_column("x", F.Float64Column.with_nulls([1.0, math.nan, 1.0, 2.0, 2.0], [False, False, False, True, False]))
    df.add_column("s", F.StringColumn.with_nulls(["b", "", "b", "a", "a"], [False, False, False, False, True]))
    df.add_column("k", F.StringColumn(["s", "t", "s", "t", "t"]))
    df.add_column("v", F.Float64Column([1.0, 2.0, 3.0, 4.0, 5.0]))
    got = df.crosstab("x", "s")
    assert got.column("x").to_list() == ["1", "2", "NaN"] and got.column_names == ["x", "", "a", "b"]
    assert got.column("").data.tolist() == [0.0, 1.0, 1.0] and got.column("a").data.tolist() == [0.0, 0.0, 1.0] and got.column("b").data.tolist() == [2.0, 0.0, 0.0]
    for call in (lambda: df.unstack("x", "s", "v"), lambda: df.pivot_table("s", "x", "v", "sum")):
        with pytest.raises(F.OperationFailed) as e:
            call()
        assert "missing cell" in str(e.value)
    got = df.pivot_table("x", "k", "v", "sum")                                # (NaN and null index cells are ONE label)
    assert got.column("x").to_list() == ["1", "2", "NaN"] and got.column("s").data.tolist()[0] == 4.0 and got.column("t").data.tolist()[1:] == [5.0, 6.0]
    assert got.column("s").is_null(1) and got.column("s").is_null(2) and got.column("t").is_null(0)
    with pytest.raises(F.DuplicateColumnName):
        df.crosstab("s", "k")                                                 # a columns label equal to the index column's name


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    info = built.PivotInfo()
    info.n_index_labels = -5
    rank = np.arange(4, dtype=np.uint32)
    H = built.MEM_HOST
    outs = [np.full(8, 7, t) for t in (np.uint64, np.uint8, np.uint64, np.uint8, np.float64, np.int64)]
    ptrs = [o.ctypes.data for o in outs]
    assert lib.pandrs_hip_pivot(None, H, C.byref(col), None, 0, C.byref(col), None, 0, None, 8, 0, C.byref(info)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    assert lib.pandrs_hip_pivot_fetch(None, H, *ptrs) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    call = lambda *a: lib.pandrs_hip_pivot(h, H, *a)                          # noqa: E731
    good = (C.byref(col), None, 0, C.byref(col), None, 0, None, 8, built.PIVOT_ROWS, C.byref(info))
    for i, bad in ((0, None), (3, None), (9, None), (2, -1), (5, -1), (7, -1), (7, 1 << 32), (8, -1), (8, 7)):
        args = list(good)
        args[i] = bad
        assert call(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_pivot(h, 7, *good) == built.ERR_INVALID_ARGUMENT
    with_values = list(good)
    with_values[6] = C.byref(col)
    assert call(*with_values) == built.ERR_INVALID_ARGUMENT and "takes no values column" in built.last_error()
    for op in range(1, 7):
        args = list(good)
        args[8] = op
        assert call(*args) == built.ERR_INVALID_ARGUMENT and "needs a values column" in built.last_error(), op
        args[6] = C.byref(col)
        # (with a values column the checks pass and the call would reach the device: not made here)
    for slot in (1, 4):                                                       # a rank table beside an F64 column, or of no codes
        args = list(good)
        args[slot], args[slot + 1] = rank.ctypes.data, 4
        assert call(*args) == built.ERR_INVALID_ARGUMENT and "rank table" in built.last_error()
    other = built.Column()
    other.data = x.ctypes.data
    for dtype in (built.CELL64, 9, -1):
        other.dtype = dtype
        for slot in (0, 3):
            args = list(good)
            args[slot] = C.byref(other)
            assert call(*args) == built.ERR_INVALID_ARGUMENT and "dtype" in built.last_error(), (dtype, slot)
    other.dtype = built.U32CODE
    args = list(good)
    args[0], args[1], args[2] = C.byref(other), rank.ctypes.data, 0
    assert call(*args) == built.ERR_INVALID_ARGUMENT                          # a rank table of no codes
    for dtype in (built.U32CODE, built.BOOLBITS, built.CELL64):               # values: I64 or F64 only
        other.dtype = dtype
        args = list(good)
        args[6], args[8] = C.byref(other), built.PIVOT_SUM
        assert call(*args) == built.ERR_INVALID_ARGUMENT and "values column" in built.last_error(), dtype
    none = built.Column()
    none.dtype = built.F64
    for slot, op in ((0, 0), (3, 0), (6, built.PIVOT_MAX)):                   # rows but no data
        args = list(good)
        args[slot], args[8] = C.byref(none), op
        if slot != 6 and op:
            args[6] = C.byref(col)
        assert call(*args) == built.ERR_INVALID_ARGUMENT, slot
    assert lib.pandrs_hip_pivot_fetch(h, 7, *([None] * 6)) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_pivot_fetch(h, H, *ptrs) == built.ERR_INVALID_ARGUMENT
    assert "retained" in built.last_error()
    assert info.n_index_labels == -5 and all((o == 7).all() for o in outs)


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_pivot": ["ctx", "mem_space", "index_col", "index_rank", "n_index_codes", "columns_col", "columns_rank", "n_columns_codes",
                                  "values_col", "n_rows", "op", "out_info"],
             "pandrs_hip_pivot_fetch": ["ctx", "out_mem_space", "out_index_labels", "out_index_flags", "out_column_labels", "out_column_flags",
                                        "out_cells", "out_rows"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    fields = ["n_index_labels", "n_column_labels", "n_cells_present", "index_missing_rows", "column_missing_rows", "path", "reserved"]
    assert [n for n, _ in hdr[1]["pandrs_hip_pivot_info"]] == fields == [n for n, _ in built.PivotInfo._fields_]
    assert [n for n, _ in rst[1]["PandrsHipPivotInfo"]] == fields
    assert [t for _, t in hdr[1]["pandrs_hip_pivot_info"]] == ["i64"] * 5 + ["i32"] * 2 == [t for _, t in rst[1]["PandrsHipPivotInfo"]]
    for value, name in enumerate(("ROWS", "SUM", "MEAN", "MIN", "MAX", "COUNT", "LAST")):
        assert hdr[3]["PANDRS_HIP_PIVOT_" + name] == value == rst[2]["PANDRS_HIP_PIVOT_" + name] == getattr(built, "PIVOT_" + name)
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- a group-by over two key columns laid out as a dense matrix"):header.index("typedef enum pandrs_hip_pivot_op")]
    for word in ("functions.rs:2138-2183", "src/pivot/mod.rs:12-250", "functions.rs:2471-2527", "BY_VALUE order", "-0.0 before 0.0", "rank[code]",
                 "byte-wise", "ONE missing label", "never looked at", "no fault", "column-major", "[j * R + i]", "exact, as int64", "sum to n_rows",
                 "0x7FF8000000000000", "DESIGN section 2", "Min / Max skip NaN", "-0.0 < 0.0", "sentinel", "null and NaN value cells included",
                 "last row", "bit for bit", "2 gamma_k sum|x|", "2^53", "Deviations", "pivot/mod.rs:195-228", "functions.rs:2492-2499", "leading NaN",
                 "HashSet order", "the string \"\"", "distinct.hpp", "does not wrap", "pivot_direct_max_cells", "ONE fused stream", "16-byte loads",
                 "64-bit row arithmetic", "no label lookup in the stream", "by ballot", "does not\n * serialise", "cannot overflow below 2^32",
                 "largest row index", "finish kernel", "n_cells_present", "read twice", "nothing per row is written", "pivot_max_cells",
                 "OPERATION_FAILED", "binary search", "stay absent", "No per-row code column", "no workgroup waits", "Geometry", "pivot_direct_max_cells = ",
                 "pivot_max_cells = ", "pivot_tile_rows = ", "pivot_blocks_per_cu = ", "64 KiB", "160 KiB", "256 MiB", "pivot_path", "n_partitions",
                 "Retained state", "invalidates the retained groupby result", "distinct list", "join result", "groupby_indices", "Buffers", "Workspace",
                 "written before it is read", "Errors", "NOT_INITIALIZED", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "INVALID_ARGUMENT", "CELL64", "2^32",
                 "n_rows == 0", "Out of scope", "to_categorical", "drop_duplicates", "margins", "legacy string frame", "multi-GPU", "2^31 and 2^32", "untested"):
        assert word in block, word
    # crosstab has left distinct's out-of-scope list for this section
    distinct = header[header.index("/* ---- distinct values of one column and their counts"):header.index("typedef enum pandrs_hip_distinct_order")]
    scope = distinct[distinct.index("Out of scope"):]
    assert "crosstab is pandrs_hip_pivot" in scope and "drop_duplicates, crosstab" not in scope


def test_option_and_geometry_in_the_header_are_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "pivot.hip")).read()
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    capi = open(os.path.join(ROOT, "pandrs_amd", "csrc", "capi.hip")).read()
    threads = int(re.search(r"PV_THREADS = (\d+);", src).group(1))
    loads = int(re.search(r"PV_LOADS = (\d+);", src).group(1))
    assert "PV_TILE = PV_THREADS * PV_LOADS * 2;" in src
    assert int(re.search(r"pivot_tile_rows = (\d+)", header).group(1)) == threads * loads * 2
    blocks = int(re.search(r"PV_BLOCKS_PER_CU = (\d+);", src).group(1))
    assert int(re.search(r"pivot_blocks_per_cu = (\d+)", header).group(1)) == blocks
    cells = int(re.search(r"PV_DIRECT_MAX_CELLS = (\d+);", src).group(1))
    assert int(re.search(r"pivot_direct_max_cells = (\d+)", header).group(1)) == cells
    most = int(re.search(r"PV_MAX_CELLS = (\d+);", src).group(1))
    assert int(re.search(r"pivot_max_cells = (\d+)", header).group(1)) == most
    assert cells * 16 == 64 * 1024 and 2 * cells * 16 <= 160 * 1024 and blocks * cells * 4 <= 160 * 1024 and threads == 256
    assert 100 << 20 <= most * 16 <= 400 << 20                               # the retained dense result: low hundreds of MB
    assert (math.isqrt(most) + 2) ** 2 > most                                 # 4098 x 4098 labels are refused
    assert re.search(r"cell_bytes = 16;", src) and not re.search(r"cell_bytes = (1[7-9]|[2-9]\d);", src)
    assert '"pivot_path"' in header and 'std::strcmp(name, "pivot_path")) c->opt.pivot_path = value;' in capi
    assert "c->opt.pivot_path" in src
    common = open(os.path.join(ROOT, "pandrs_amd", "csrc", "common.hpp")).read()
    begin = common[common.index("inline void timings_begin("):]
    assert "c->pv.valid = false;" in begin[:begin.index("}")]                                     # every compute call drops the retained result
    for name in ("pandrs_hip_pivot", "pandrs_hip_pivot_fetch"):
        assert re.search(r"int32_t %s\([^{;]*\) try \{" % name, capi) and 'on_exception("%s")' % name in capi
    assert "pivot.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()
    # the census is shared with distinct.hip, not copied
    shared = open(os.path.join(ROOT, "pandrs_amd", "csrc", "distinct.hpp")).read()
    assert "void dn_census(" in shared and "dn_census<DT, PV_THREADS, PV_LOADS>" in src
    assert "dn_census<DT, DN_THREADS, DN_LOADS>" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "distinct.hip")).read()


def test_cpp_mirror_pivot_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pivot_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "pivot_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
