"""PandasCompatExt's whole-column shape statistics (reference src/dataframe/pandas_compat/functions.rs:1617-1665, :2284-2314,
:3571-3588, :4207-4224, :934-1022, :1583-1615; helpers/aggregations.rs:8-225): the parts that need no GPU - the mirror's methods
against the restatement with the device calls answered by a numpy stand-in, the early returns, which `want` bits and how many
device calls each method makes, the errors raised before any device call, the C ABI entry points without a device, the header /
ctypes / Rust declarations and the geometry the header states, and the C++ mirror's methods compiled against the header."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import eval_ref
from tests import moments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMN_METHODS = ("skew", "kurtosis", "sem", "mad", "prod", "var_column", "std_column", "range", "abs_sum", "cv", "geometric_mean",
                  "harmonic_mean", "iqr", "percentile_value", "trimmed_mean", "describe_column", "zscore")
FRAME_METHODS = ("sum_all", "mean_all", "std_all", "var_all", "min_all", "max_all", "product_all", "median_all")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from pandrs_amd import _lib
    return _lib


def _values(col, n):
    data, mask, _ = col
    null = None if mask is None else np.unpackbits(np.asarray(mask, np.uint8), bitorder="little")[:n].astype(bool)
    return R.values_of(np.asarray(data)[:n], null)


class NumpyContext:
    """The CPU stand-in: Context.moments / Context.order_stats answered by tests/moments_ref.py, Context.eval by tests/eval_ref.py,
    and a record of the calls."""
    device = 0

    def __init__(self):
        self.calls = []

    def moments(self, cols, n_rows, want=0):
        self.calls.append(("moments", len(cols), n_rows, want))
        return [R.fields(_values(c, n_rows), want) for c in cols]

    def order_stats(self, col, n_rows, ops):
        ops = list(ops)
        self.calls.append(("order_stats", n_rows, ops))
        out, m = R.order_stats(_values(col, n_rows), ops)
        return np.array(out, np.float64), m

    def eval(self, cols, n_rows, program, out=None, out_mask=None, out_device=None):
        self.calls.append(("eval", n_rows))
        cols = [(c[0], None if c[1] is None else eval_ref.unpack(c[1], n_rows), c[2]) for c in cols]
        r = eval_ref.evaluate(cols, n_rows, program)
        return r.values, (eval_ref.pack(r.nulls) if r.nulls.any() else None), int(r.nulls.sum())


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, str):
        return a == b
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def _df(v, name="v", nulls=None):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column(name, F.Float64Column(list(v)) if nulls is None else F.Float64Column.with_nulls(list(v), list(nulls)))
    return df


def test_mirror_has_the_methods_and_the_constants(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in COLUMN_METHODS + FRAME_METHODS:
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.moments) and callable(E.Context.order_stats)
    assert (built.MOMENTS_WANT_CENTRAL, built.MOMENTS_WANT_LOG, built.MOMENTS_WANT_RECIP, built.MOMENTS_WANT_PROD) == (1, 2, 4, 8) == \
        (R.WANT_CENTRAL, R.WANT_LOG, R.WANT_RECIP, R.WANT_PROD)
    assert (built.OS_AT_FRAC_N, built.OS_AT_FRAC_N1, built.OS_MEDIAN, built.OS_TRIMMED_MEAN) == (0, 1, 2, 3) == \
        (R.AT_FRAC_N, R.AT_FRAC_N1, R.MEDIAN, R.TRIMMED_MEAN)
    assert built.MOMENTS_MAX_COLUMNS == 16 and built.ORDER_STATS_MAX_OPS == 8


def _calls(df):
    return {"skew": lambda c: df.skew(c), "kurtosis": lambda c: df.kurtosis(c), "sem": lambda c: df.sem(c, 1), "mad": lambda c: df.mad(c),
            "prod": lambda c: df.prod(c), "var_column": lambda c: df.var_column(c, 1), "std_column": lambda c: df.std_column(c, 0),
            "range": lambda c: df.range(c), "abs_sum": lambda c: df.abs_sum(c), "cv": lambda c: df.cv(c),
            "geometric_mean": lambda c: df.geometric_mean(c), "harmonic_mean": lambda c: df.harmonic_mean(c), "iqr": lambda c: df.iqr(c),
            "percentile_value": lambda c: df.percentile_value(c, 0.3), "trimmed_mean": lambda c: df.trimmed_mean(c, 0.1),
            "describe_column": lambda c: df.describe_column(c), "zscore": lambda c: df.zscore(c)}


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = F.OptimizedDataFrame()
    df.add_column("x", F.Float64Column([0.5, 0.25, 1.0, 2.0]))
    df.add_column("s", F.StringColumn(["a", "b", "c", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    calls = _calls(df)
    assert set(calls) == set(COLUMN_METHODS)
    for name, call in calls.items():
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value), name
    # the reference's early returns for the argument (aggregations.rs:185, :204) are decided before any device call
    for q in (-0.1, 1.5, math.inf):
        assert math.isnan(df.percentile_value("x", q))
    for a in (-0.01, 0.5, 0.75):
        assert math.isnan(df.trimmed_mean("x", a))
    for fn in (lambda: df.percentile_value("x", math.nan), lambda: df.trimmed_mean("x", math.nan), lambda: df.var_column("x", -1),
               lambda: df.sem("x", -1)):
        with pytest.raises(F.InvalidValue):
            fn()
    # a frame without a numeric column asks the device nothing
    only = F.OptimizedDataFrame()
    only.add_column("s", F.StringColumn(["a"]))
    for name in FRAME_METHODS:
        assert getattr(only, name)() == []


COLUMNS = {"empty": [], "one": [3.5], "two": [1.0, 4.0], "three": [1.0, 4.0, 2.0], "four": [1.0, 4.0, 2.0, 8.0], "constant": [2.5] * 6,
           "all_nan": [math.nan] * 3, "nan_inside": [1.0, math.nan, -3.0, 0.0, 7.25, math.nan, 7.25, -0.5],
           "zero_mean": [-1.0, 1.0], "with_zero_and_negative": [0.0, -2.0, 4.0, 0.5], "ties": [1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0],
           "random": np.random.default_rng(8).normal(3.0, 2.0, 97).tolist(),
           # (cells, null flags): built with Float64Column.with_nulls; the cells under a null bit must never count
           "all_null": ([1.0, 2.0, 3.0, 4.0, 5.0], [True] * 5), "all_null_or_nan": ([math.nan, 2.0, math.nan], [False, True, False]),
           "one_valid_among_nulls": ([9.0, 3.5, -9.0], [True, False, True]),
           "nulls_inside": ([1.0, 50.0, 4.0, 2.0, -50.0, 8.0, 8.0], [False, True, False, False, True, False, False])}


@pytest.mark.parametrize("key", list(COLUMNS))
def test_every_method_is_the_restatement_on_the_stand_in(built, monkeypatch, key):
    """n = 0, 1, 2, 3, 4 valid cells, a constant column, all-null, all-NaN, ddof >= count: every early return of the reference,
    and the want bits and the number of device calls of each method."""
    import pandrs_amd.frame as F
    ctx = NumpyContext()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    cells, nulls = COLUMNS[key] if isinstance(COLUMNS[key], tuple) else (COLUMNS[key], None)
    v = R.values_of(np.array(cells, np.float64), nulls)     # what the reference sees: a null cell is its missing value, NaN
    df = _df(cells, nulls=nulls)
    assert (df.column("v").null_mask is not None) == (nulls is not None)
    n_valid = int((~np.isnan(v)).sum())
    CENTRAL, LOG, RECIP, PROD = built.MOMENTS_WANT_CENTRAL, built.MOMENTS_WANT_LOG, built.MOMENTS_WANT_RECIP, built.MOMENTS_WANT_PROD
    plan = [("skew", (), R.skew, (), CENTRAL), ("kurtosis", (), R.kurtosis, (), CENTRAL), ("mad", (), R.mad, (), CENTRAL),
            ("prod", (), R.prod, (), PROD), ("range", (), R.value_span, (), 0), ("abs_sum", (), R.abs_sum, (), 0), ("cv", (), R.cv, (), CENTRAL),
            ("geometric_mean", (), R.geometric_mean, (), LOG), ("harmonic_mean", (), R.harmonic_mean, (), RECIP)]
    for ddof in (0, 1, 2, n_valid, n_valid + 1):
        plan += [("var_column", (ddof,), R.var_column, (ddof,), CENTRAL), ("std_column", (ddof,), R.std_column, (ddof,), CENTRAL),
                 ("sem", (ddof,), R.sem, (ddof,), CENTRAL)]
    for name, args, ref, ref_args, want in plan:
        ctx.calls.clear()
        got = getattr(df, name)("v", *args)
        assert _same(got, ref(v, *ref_args)), (name, args, got, ref(v, *ref_args))
        assert ctx.calls == [("moments", 1, len(v), want)], (name, ctx.calls)
    # order statistics: one call each, only the op it needs
    ctx.calls.clear()
    assert _same(df.iqr("v"), R.iqr(v))
    assert ctx.calls == [("order_stats", len(v), [(built.OS_AT_FRAC_N, 0.25), (built.OS_AT_FRAC_N, 0.75)])]
    for q in (0.0, 0.25, 0.5, 0.75, 1.0, 0.3183098861837907):
        ctx.calls.clear()
        assert _same(df.percentile_value("v", q), R.percentile_value(v, q))
        assert ctx.calls == [("order_stats", len(v), [(built.OS_AT_FRAC_N1, q)])]
    for a in (0.0, 0.1, 0.25, 0.49, 0.3183098861837907):
        ctx.calls.clear()
        assert _same(df.trimmed_mean("v", a), R.trimmed_mean(v, a)), a
        assert ctx.calls == [("order_stats", len(v), [(built.OS_TRIMMED_MEAN, a)])]
    ctx.calls.clear()
    assert _same(df.describe_column("v"), R.describe_column(v))
    assert [c[0] for c in ctx.calls] == (["moments", "order_stats"] if n_valid else ["moments"]) and ctx.calls[0][3] == CENTRAL
    # zscore: one moments call, then one eval call; InvalidValue where the reference returns Err
    ctx.calls.clear()
    try:
        want_z = R.zscore(v)
    except ValueError as e:
        with pytest.raises(F.InvalidValue, match=str(e)):
            df.zscore("v")
        assert [c[0] for c in ctx.calls] == ["moments"]
    else:
        assert _same(df.zscore("v"), want_z)
        assert [c[0] for c in ctx.calls] == ["moments", "eval"] and ctx.calls[0][3] == CENTRAL


def test_null_cells_and_int64_cells(built, monkeypatch):
    import pandrs_amd.frame as F
    ctx = NumpyContext()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    df = _df([1.0, 99.0, 4.0, 2.0, 8.0], nulls=[False, True, False, False, False])
    v = np.array([1.0, math.nan, 4.0, 2.0, 8.0])
    for name, ref in (("skew", R.skew), ("kurtosis", R.kurtosis), ("mad", R.mad), ("prod", R.prod), ("iqr", R.iqr), ("cv", R.cv)):
        assert _same(getattr(df, name)("v"), ref(v)), name
    assert _same(df.zscore("v"), R.zscore(v)) and math.isnan(df.zscore("v")[1])
    ints = F.OptimizedDataFrame()
    ints.add_column("i", F.Int64Column([5, -3, 2 ** 53 + 1, 7]))
    w = np.array([5.0, -3.0, float(2 ** 53 + 1), 7.0])
    assert _same(ints.range("i"), R.value_span(w)) and _same(ints.var_column("i", 1), R.var_column(w, 1))
    assert _same(ints.median_all(), R.median_all({"i": w}))


def test_frame_lists_leave_out_what_the_reference_leaves_out_and_chunk_by_max_columns(built, monkeypatch):
    import pandrs_amd.frame as F
    ctx = NumpyContext()
    monkeypatch.setattr(F, "get_context", lambda: ctx)
    rng = np.random.default_rng(2)
    df = F.OptimizedDataFrame()
    cols = {}
    n_numeric = 2 * built.MOMENTS_MAX_COLUMNS + 3
    for i in range(n_numeric):
        name = "c%d" % i
        if i == 1:
            v = np.full(6, math.nan)
        elif i in (2, 10, 33):                                # all-null columns: Float64, Int64, and one in the last chunk
            cells = rng.integers(-4, 5, 6)
            kind = F.Int64Column if i == 10 else F.Float64Column
            df.add_column(name, kind.with_nulls(cells.astype(np.int64 if i == 10 else np.float64).tolist(), [True] * 6))
            assert df.column(name).null_mask is not None
            cols[name] = np.full(6, math.nan)
            continue
        elif i == 4:
            v = np.array([math.nan, 2.5, math.nan, math.nan, math.nan, math.nan])
        elif i % 5 == 0:
            v = rng.integers(-4, 5, 6).astype(np.float64)
            df.add_column(name, F.Int64Column(v.astype(np.int64).tolist()))
            cols[name] = v
            continue
        else:
            v = rng.normal(0, 3, 6)
        df.add_column(name, F.Float64Column(v.tolist()))
        cols[name] = v
        if i == 7:
            df.add_column("label", F.StringColumn(list("abcdef")))
            df.add_column("flag", F.BooleanColumn([True] * 6))
    wants = {"sum_all": 0, "mean_all": 0, "min_all": 0, "max_all": 0, "var_all": built.MOMENTS_WANT_CENTRAL,
             "std_all": built.MOMENTS_WANT_CENTRAL, "product_all": built.MOMENTS_WANT_PROD}
    M = built.MOMENTS_MAX_COLUMNS
    for name, want in wants.items():
        ctx.calls.clear()
        got = getattr(df, name)()
        assert _same(got, getattr(R, name)(cols)), name
        assert ctx.calls == [("moments", M, 6, want), ("moments", M, 6, want), ("moments", 3, 6, want)], (name, ctx.calls)
    assert [k for k, _ in df.sum_all()] == list(cols) and "c1" not in dict(df.mean_all()) and "c4" not in dict(df.var_all())
    assert "c4" in dict(df.mean_all())
    for name in ("mean_all", "min_all", "max_all", "var_all", "std_all", "product_all", "median_all"):
        assert not {"c1", "c2", "c10", "c33"} & set(dict(getattr(df, name)())), name          # no valid cell: left out
    assert [dict(df.sum_all())[k] for k in ("c2", "c10", "c33")] == [0.0, 0.0, 0.0]
    ctx.calls.clear()
    assert _same(df.median_all(), R.median_all(cols))
    assert len(ctx.calls) == n_numeric and all(c[0] == "order_stats" and c[2] == [(built.OS_MEDIAN, 0.0)] for c in ctx.calls)


def test_entry_points_without_a_context_and_with_bad_arguments(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out = (built.MomentsStats * 2)()
    H = built.MEM_HOST
    assert lib.pandrs_hip_moments(None, H, C.byref(col), 1, 8, 0, out) == built.ERR_NOT_INITIALIZED and "context" in built.last_error()
    ops = (C.c_int32 * 8)(*([built.OS_MEDIAN] * 8))
    args = (C.c_double * 8)(*([0.25] * 8))
    res = (C.c_double * 8)(*([9.0] * 8))
    cnt = C.c_int64(-5)
    assert lib.pandrs_hip_order_stats(None, H, C.byref(col), 8, ops, args, 1, res, C.byref(cnt)) == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error()
    # the argument checks come before the context is used for anything: a stand-in handle is never dereferenced
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    good = (C.byref(col), 1, 8, 0, out)
    for i, bad in ((0, None), (1, 0), (1, -1), (1, built.MOMENTS_MAX_COLUMNS + 1), (2, -1), (2, 1 << 32), (3, 16), (3, 1 << 31), (4, None)):
        a = list(good)
        a[i] = bad
        assert lib.pandrs_hip_moments(h, H, *a) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_moments(h, 7, *good) == built.ERR_INVALID_ARGUMENT
    other = built.Column()
    other.data = x.ctypes.data
    for dt in (built.U32CODE, built.BOOLBITS, built.CELL64):
        other.dtype = dt
        assert lib.pandrs_hip_moments(h, H, C.byref(other), 1, 8, 0, out) == built.ERR_TYPE_MISMATCH, dt
        assert lib.pandrs_hip_order_stats(h, H, C.byref(other), 8, ops, args, 1, res, C.byref(cnt)) == built.ERR_TYPE_MISMATCH, dt
    good_o = (C.byref(col), 8, ops, args, 1, res, C.byref(cnt))
    for i, bad in ((0, None), (1, -1), (1, 1 << 32), (2, None), (3, None), (4, 0), (4, built.ORDER_STATS_MAX_OPS + 1), (5, None), (6, None)):
        a = list(good_o)
        a[i] = bad
        assert lib.pandrs_hip_order_stats(h, H, *a) == built.ERR_INVALID_ARGUMENT, (i, bad)
    assert lib.pandrs_hip_order_stats(h, 7, *good_o) == built.ERR_INVALID_ARGUMENT
    bad_ops = (C.c_int32 * 1)(4)
    assert lib.pandrs_hip_order_stats(h, H, C.byref(col), 8, bad_ops, args, 1, res, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    nan_arg = (C.c_double * 1)(math.nan)
    frac = (C.c_int32 * 1)(built.OS_AT_FRAC_N)
    assert lib.pandrs_hip_order_stats(h, H, C.byref(col), 8, frac, nan_arg, 1, res, C.byref(cnt)) == built.ERR_INVALID_ARGUMENT
    assert "NaN" in built.last_error() and list(res) == [9.0] * 8 and cnt.value == -5
    # no row is OK without a device: the fold identities, NaN results
    for want in (0, 15):
        assert lib.pandrs_hip_moments(h, H, C.byref(col), 1, 0, want, out) == 0
        st = out[0]
        assert (st.count, st.count_pos, st.count_nonzero) == (0, 0, 0) and st.sum == 0.0 and math.copysign(1.0, st.sum) == -1.0
        assert st.min == math.inf and st.max == -math.inf and math.isnan(st.mean)
        assert _same({k: getattr(st, k) for k, _ in built.MomentsStats._fields_}, R.fields(np.array([]), want))
    assert lib.pandrs_hip_order_stats(h, H, C.byref(col), 0, ops, args, 3, res, C.byref(cnt)) == 0
    assert cnt.value == 0 and all(math.isnan(r) for r in list(res)[:3]) and res[3] == 9.0


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    names = {"pandrs_hip_moments": ["ctx", "mem_space", "cols", "n_cols", "n_rows", "want", "out"],
             "pandrs_hip_order_stats": ["ctx", "mem_space", "col", "n_rows", "ops", "args", "n_ops", "out", "out_count"]}
    for name, params in names.items():
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    # the struct: field for field, and its size
    fields = hdr[1]["pandrs_hip_moments_stats"]
    assert [n for n, _ in fields] == [n for n, _ in built.MomentsStats._fields_] == list(R.fields(np.array([1.0])))
    assert [t for _, t in fields] == ["i64"] * 3 + ["f64"] * 12
    assert C.sizeof(built.MomentsStats) == 8 * len(fields) == 120
    assert hdr[1]["pandrs_hip_moments_stats"] == rst[1]["PandrsHipMomentsStats"] if "PandrsHipMomentsStats" in rst[1] else \
        hdr[1]["pandrs_hip_moments_stats"] == rst[1]["pandrs_hip_moments_stats"]
    for k, v in (("PANDRS_HIP_MOMENTS_WANT_CENTRAL", 1), ("PANDRS_HIP_MOMENTS_WANT_LOG", 2), ("PANDRS_HIP_MOMENTS_WANT_RECIP", 4),
                 ("PANDRS_HIP_MOMENTS_WANT_PROD", 8), ("PANDRS_HIP_MOMENTS_MAX_COLUMNS", built.MOMENTS_MAX_COLUMNS),
                 ("PANDRS_HIP_ORDER_STATS_MAX_OPS", built.ORDER_STATS_MAX_OPS)):
        assert hdr[2][k] == v == rst[2][k], k
    for k, v in (("PANDRS_HIP_OS_AT_FRAC_N", 0), ("PANDRS_HIP_OS_AT_FRAC_N1", 1), ("PANDRS_HIP_OS_MEDIAN", 2), ("PANDRS_HIP_OS_TRIMMED_MEAN", 3)):
        assert hdr[3][k] == v == rst[2][k], k
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    assert "#define PANDRS_HIP_ABI_VERSION 1" in header
    block = header[header.index("/* ---- shape statistics of whole columns"):header.index("/* ---- rank of one numeric column")]
    for word in ("functions.rs:1617-1665", "aggregations.rs:8-51", ":3571-3588", ":4207-4224", ":2284-2314", ":934-1022", ":1583-1595",
                 ":1597-1615", ":184-225", "moments_tile_rows = ", "moments_blocks_per_cu = ", "moments_max_columns = ", "lean variant",
                 "No float atomics", "launch-boundary reduce", "read twice", "gamma_m", "4 u", "2^53", "bit for bit", "sticky", "frexp",
                 "Signed zero", "Exactness", "Deviations", "Geometry", "Workspace", "Errors", "Out of scope", "TYPE_MISMATCH",
                 "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT", "2^32", "n_partitions", "table_slots",
                 "Counting rule", "strictly between", "(n_below + n_eq_lo - t)", "m - 2t", "before any launch", "32 slots", "band stream"):
        assert word in block, word
    describe = header[header.index("/* ---- describe and exact percentiles"):header.index("typedef struct pandrs_hip_describe_stats")]
    assert "Out of scope: mode, confidence intervals" in describe and "skewness, kurtosis, mode" not in describe


def test_geometry_in_the_header_is_the_kernels(built):
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "moments.hip")).read()
    shared = open(os.path.join(ROOT, "pandrs_amd", "csrc", "describe.hpp")).read()
    ds = open(os.path.join(ROOT, "pandrs_amd", "csrc", "describe.hip")).read()
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    capi = open(os.path.join(ROOT, "pandrs_amd", "csrc", "capi.hip")).read()
    tile = int(re.search(r"DS_THREADS = (\d+);", shared).group(1)) * int(re.search(r"DS_LOADS = (\d+);", shared).group(1)) * 2
    assert "MO_TILE = DS_TILE;" in src and "DS_TILE = DS_THREADS * DS_LOADS * 2;" in shared
    assert int(re.search(r"moments_tile_rows = (\d+)", header).group(1)) == tile == int(re.search(r"describe_tile_rows = (\d+)", header).group(1))
    assert int(re.search(r"moments_blocks_per_cu = (\d+)", header).group(1)) == int(re.search(r"MO_BLOCKS_PER_CU = (\d+);", src).group(1))
    assert int(re.search(r"moments_max_columns = (\d+)", header).group(1)) == built.MOMENTS_MAX_COLUMNS == \
        int(re.search(r"#define PANDRS_HIP_MOMENTS_MAX_COLUMNS (\d+)", header).group(1))
    assert "MO_MAX_COLUMNS = PANDRS_HIP_MOMENTS_MAX_COLUMNS;" in src
    assert "fp contract(off)" in src and "atomicAdd" not in src and "unsafeAtomicAdd" not in src
    assert int(re.search(r"DS_MAX_OS = (\d+);", ds).group(1)) == built.ORDER_STATS_MAX_OPS and "2 * DS_MAX_OS <= DS_MAX_SLOTS" in ds
    assert "moments.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()
    for entry in ("pandrs_hip_moments", "pandrs_hip_order_stats"):
        assert re.search(r"%s\([^)]*\) try \{" % entry, capi) and 'on_exception("%s")' % entry in capi


def test_cpp_mirror_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "moments_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "moments_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr
