"""PandasCompatExt's row masks - gt / ge / lt / le / eq_value / ne_value, between / is_between, isna / notna, is_finite /
is_infinite, isin / isin_numeric and their consumers (reference src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46,
functions.rs:141-158, :253-257, :4141-4161): the parts that need no GPU - the mirror's methods and errors (raised before any
device call), the enum order, the C ABI entry points without a device, the header / ctypes / Rust declarations, and the C++
mirror's methods compiled against the header."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["GT", "GE", "LT", "LE", "EQ", "NE", "BETWEEN", "BETWEEN_EXCLUSIVE", "ISNA", "NOTNA", "IS_FINITE", "IS_INFINITE"]
MASKS = ("gt", "ge", "lt", "le", "eq_value", "ne_value", "between", "is_between", "isna", "notna", "is_finite", "is_infinite",
         "isin_numeric", "isin")
CONSUMERS = ("count_na", "has_nulls", "count_value", "query_gt", "query_lt", "query_eq", "dropna")


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


def _calls(df):
    one = lambda name: (lambda c: getattr(df, name)(c, 1.0))                      # noqa: E731
    none = lambda name: (lambda c: getattr(df, name)(c))                          # noqa: E731
    calls = {name: one(name) for name in ("gt", "ge", "lt", "le", "eq_value", "ne_value", "count_value", "query_gt", "query_lt", "query_eq")}
    calls.update({name: none(name) for name in ("isna", "notna", "is_finite", "is_infinite", "count_na", "has_nulls", "dropna")})
    calls["between"] = lambda c: df.between(c, 0.0, 1.0)
    calls["is_between"] = lambda c: df.is_between(c, 0.0, 1.0, False)
    calls["isin_numeric"] = lambda c: df.isin_numeric(c, [1.0, 2.0])
    return calls


def test_mirror_has_the_methods(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in MASKS + CONSUMERS:
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.predicate) and callable(E.Context.isin)
    assert [getattr(built, "PRED_" + name) for name in OPS] == list(range(12))


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F
    _no_device(monkeypatch)
    df = _frame()
    calls = _calls(df)
    assert set(calls) | {"isin"} == set(MASKS + CONSUMERS)
    for name, call in calls.items():
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value), name
    with pytest.raises(F.ColumnNotFound):
        df.isin("nope", ["a"])
    for col in ("id", "x", "flag"):                                               # numeric and Boolean columns under isin
        with pytest.raises(F.ColumnTypeMismatch):
            df.isin(col, ["a"])
    # no rows: the reference's empty Vec<bool> / 0 / false / filter's empty shape, without a device
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Float64Column([]))
    empty.add_column("t", F.StringColumn([]))
    for name, call in _calls(empty).items():
        got = call("a")
        if name.startswith("query_") or name == "dropna":
            assert got.row_count() == 0 and got.column_names == ["a", "t"], name
        elif name in ("count_na", "count_value"):
            assert got == 0, name
        elif name == "has_nulls":
            assert got is False, name
        else:
            assert got == [], name
    assert empty.isin("t", ["a"]) == []


def test_frame_results_come_from_one_call_each(built, monkeypatch):
    """A stand-in context: every mask method hands the column's view, the row count, the op and its arguments to
    Context.predicate once; the counts use the count-only form; the query methods keep the mask on the device and hand it
    to filter_indices as a BOOLBITS column; isin on strings sends pool codes, without the strings the pool has never seen."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        device = 0

        def predicate(self, col, n_rows, op, a=0.0, b=0.0, out=None, out_device=None, count_only=False):
            calls.append(("pred", col[2], n_rows, op, a, b, out_device, count_only))
            if count_only:
                return None, 3
            if out_device:
                return "device-mask", 2
            return np.array([0b0101], np.uint8), 2

        def isin(self, col, n_rows, values, negate=False, out=None, out_device=None, count_only=False):
            calls.append(("isin", col[2], n_rows, values[2], list(values[0]), negate))
            return np.array([0b1001], np.uint8), 2

        def filter_indices(self, cond, n_rows, indices=True):
            calls.append(("filter", cond, n_rows))
            raise KeyboardInterrupt                                              # the gathers behind it need a device

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    P = built
    for fn, op, a, b in ((lambda: df.gt("x", 2.5), P.PRED_GT, 2.5, 0.0), (lambda: df.ge("x", 2.5), P.PRED_GE, 2.5, 0.0),
                         (lambda: df.lt("x", 2.5), P.PRED_LT, 2.5, 0.0), (lambda: df.le("x", 2.5), P.PRED_LE, 2.5, 0.0),
                         (lambda: df.eq_value("x", 2.5), P.PRED_EQ, 2.5, 0.0), (lambda: df.ne_value("x", 2.5), P.PRED_NE, 2.5, 0.0),
                         (lambda: df.between("x", 1.0, 2.0), P.PRED_BETWEEN, 1.0, 2.0),
                         (lambda: df.is_between("x", 1.0, 2.0), P.PRED_BETWEEN, 1.0, 2.0),
                         (lambda: df.is_between("x", 1.0, 2.0, False), P.PRED_BETWEEN_EXCLUSIVE, 1.0, 2.0),
                         (lambda: df.isna("x"), P.PRED_ISNA, 0.0, 0.0), (lambda: df.notna("x"), P.PRED_NOTNA, 0.0, 0.0),
                         (lambda: df.is_finite("x"), P.PRED_IS_FINITE, 0.0, 0.0), (lambda: df.is_infinite("x"), P.PRED_IS_INFINITE, 0.0, 0.0)):
        assert fn() == [True, False, True, False]
        assert calls.pop() == ("pred", P.F64, 4, op, a, b, False, False) and not calls
    assert df.count_na("id") == 3 and calls.pop() == ("pred", P.I64, 4, P.PRED_ISNA, 0.0, 0.0, None, True)
    assert df.has_nulls("id") is True and calls.pop() == ("pred", P.I64, 4, P.PRED_ISNA, 0.0, 0.0, None, True)
    assert df.count_value("id", 2.0) == 3 and calls.pop() == ("pred", P.I64, 4, P.PRED_EQ, 2.0, 0.0, None, True)
    for fn, op, a in ((lambda: df.query_gt("x", 1.5), P.PRED_GT, 1.5), (lambda: df.query_lt("x", 1.5), P.PRED_LT, 1.5),
                      (lambda: df.query_eq("x", 1.5), P.PRED_EQ, 1.5), (lambda: df.dropna("x"), P.PRED_NOTNA, 0.0)):
        with pytest.raises(KeyboardInterrupt):
            fn()
        assert calls.pop() == ("filter", ("device-mask", None, P.BOOLBITS), 4)
        assert calls.pop() == ("pred", P.F64, 4, op, a, 0.0, True, False) and not calls
    assert df.isin_numeric("id", [2.0, 3.0]) == [True, False, False, True]
    assert calls.pop() == ("isin", P.I64, 4, P.F64, [2.0, 3.0], False)
    pool = F.GLOBAL_STRING_POOL
    size = len(pool)
    assert df.isin("s", ["d", "a strange string no column has held", "a"]) == [True, False, False, True]
    assert calls.pop() == ("isin", P.U32CODE, 4, P.U32CODE, [pool.get_or_insert("d"), pool.get_or_insert("a")], False)
    assert len(pool) == size                                                     # the unknown string was not inserted
    assert pool.find("a strange string no column has held") is None and pool.find("d") == pool.get_or_insert("d") and len(pool) == size


def test_enum_order_equals_the_headers(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_pred_op {"):header.index("} pandrs_hip_pred_op;")]
    values = dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_PRED_(\w+) = (\d+)", body))
    assert values == {name: i for i, name in enumerate(OPS)}
    for name, v in values.items():
        assert getattr(built, "PRED_" + name) == v
    from tests import predicate_ref as R
    assert [getattr(R, name) for name in OPS] == list(range(12))
    hpp = open(os.path.join(ROOT, "include", "pandrs_hip.hpp")).read()
    for name in OPS:
        assert "PANDRS_HIP_PRED_" + name in hpp, name


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    vals = built.Column()
    vals.data, vals.dtype = x.ctypes.data, built.F64
    out = np.full(4, 0xAA, np.uint8)
    cnt = C.c_int64(-5)
    H = built.MEM_HOST
    assert lib.pandrs_hip_predicate(None, H, C.byref(col), 8, built.PRED_GT, 1.0, 0.0, H, out.ctypes.data, C.byref(cnt)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    assert lib.pandrs_hip_isin(None, H, C.byref(col), 8, H, C.byref(vals), 8, 0, H, out.ctypes.data, C.byref(cnt)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    pred = lambda c, n, op, o, pc: lib.pandrs_hip_predicate(h, H, c, n, op, 1.0, 2.0, H, o, pc)            # noqa: E731
    good = (C.byref(col), 8, built.PRED_GT, out.ctypes.data, C.byref(cnt))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, -1), (2, 12)):
        args = list(good)
        args[i] = bad
        assert pred(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert pred(C.byref(col), 8, built.PRED_GT, None, None) == built.ERR_INVALID_ARGUMENT                  # nothing asked for
    assert lib.pandrs_hip_predicate(h, 7, C.byref(col), 8, 0, 1.0, 2.0, H, out.ctypes.data, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_predicate(h, H, C.byref(col), 8, 0, 1.0, 2.0, 7, out.ctypes.data, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    other = built.Column()
    other.data = x.ctypes.data
    for dt in (built.U32CODE, built.BOOLBITS, built.CELL64):
        other.dtype = dt
        assert pred(C.byref(other), *good[1:]) == built.ERR_TYPE_MISMATCH, dt
    isin = lambda c, n, v, nv, o, pc: lib.pandrs_hip_isin(h, H, c, n, H, v, nv, 0, H, o, pc)               # noqa: E731
    good = (C.byref(col), 8, C.byref(vals), 8, out.ctypes.data, C.byref(cnt))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, None), (3, -1), (3, (1 << 30) + 1)):
        args = list(good)
        args[i] = bad
        assert isin(*args) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert isin(C.byref(col), 8, C.byref(vals), 8, None, None) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_isin(h, H, C.byref(col), 8, 7, C.byref(vals), 8, 0, H, out.ctypes.data, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    masked = built.Column()
    masked.data, masked.null_mask, masked.dtype = x.ctypes.data, out.ctypes.data, built.F64
    assert isin(C.byref(col), 8, C.byref(masked), 8, out.ctypes.data, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    assert "null mask" in built.last_error()
    ok = {(built.F64, built.F64), (built.I64, built.F64), (built.I64, built.I64), (built.U32CODE, built.U32CODE)}
    for cd in range(5):
        for vd in range(5):
            if (cd, vd) in ok:
                continue
            other.dtype, vals.dtype = cd, vd
            assert isin(C.byref(other), 8, C.byref(vals), 8, out.ctypes.data, C.byref(cnt)) == built.ERR_TYPE_MISMATCH, (cd, vd)
    vals.dtype = built.F64
    # nothing to do is OK, writes nothing and reports 0
    cnt.value = -5
    assert pred(C.byref(col), 0, built.PRED_GT, out.ctypes.data, C.byref(cnt)) == 0 and cnt.value == 0
    cnt.value = -5
    assert isin(C.byref(col), 0, C.byref(vals), 8, out.ctypes.data, C.byref(cnt)) == 0 and cnt.value == 0
    assert (out == 0xAA).all()


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_predicate": ["ctx", "mem_space", "col", "n_rows", "op", "a", "b", "out_mem_space", "out_bits", "out_count"],
             "pandrs_hip_isin": ["ctx", "mem_space", "col", "n_rows", "values_mem_space", "values", "n_values", "negate", "out_mem_space",
                                 "out_bits", "out_count"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    for v, k in enumerate(OPS):
        assert hdr[3]["PANDRS_HIP_PRED_" + k] == v == rst[2]["PANDRS_HIP_PRED_" + k]
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- row masks of one column: compare, between, isna, isin"):header.index("typedef enum pandrs_hip_pred_op")]
    for word in ("comparison_ops.rs:7-46", "functions.rs:253-257", "functions.rs:4141-4161", "functions.rs:141-158", "DBL_EPSILON", "2^53",
                 "to_bits", "-0.0", "payload", "behaves as NaN", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED",
                 "INVALID_ARGUMENT", "2^32", "predicate_tile_rows = ", "predicate_blocks_per_cu = ", "isin_lds_max_values = ", "isin_path",
                 "any byte alignment", "and / or / not", "between two columns", "str_contains", "where_cond", "legacy", "multi-GPU"):
        assert word in block, word
    fill = header[header.index("/* ---- missing cells of one numeric column"):header.index("typedef enum pandrs_hip_fill_method")]
    assert not re.search(r"Out of scope: limit=, dropna", fill)                   # no longer out of scope there


def test_geometry_in_the_header_is_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "predicate.hip")).read()
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    threads = int(re.search(r"PRED_THREADS = (\d+);", src).group(1))
    rpt = int(re.search(r"PRED_RPT = (\d+);", src).group(1))
    assert "PRED_TILE = PRED_THREADS * PRED_RPT;" in src
    assert int(re.search(r"predicate_tile_rows = (\d+)", header).group(1)) == threads * rpt
    assert int(re.search(r"predicate_blocks_per_cu = (\d+)", header).group(1)) == int(re.search(r"PRED_BLOCKS_PER_CU = (\d+);", src).group(1))
    lds = int(re.search(r"isin_lds_max_values = (\d+)", header).group(1))
    assert lds == int(re.search(r"PRED_LDS_VALUES = (\d+);", src).group(1))
    assert 2 * lds * 8 <= 64 * 1024 and lds & (lds - 1) == 0                       # the table: a power of two slots, at most 64 KiB
    assert "fp contract(off)" in src and "fast-math" not in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()


def test_cpp_mirror_predicates_compile_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "predicate_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "predicate_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
