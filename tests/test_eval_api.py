"""Derived columns (pandrs_hip_eval; PandasCompatExt::add_scalar .. sqrt, col_add .. col_div, clip, where_cond / mask, round,
coalesce, sign, normalize and helpers/math_ops.rs of the reference): the parts that need no GPU - the methods, the expression
builder and the constants, the errors raised before any device call, the program every named method hands over, the entry
point without a context, pandrs_hip_eval_check against the twin's validator, the header / ctypes / Rust declarations, the C++
mirror compiled against the header, and that no kernel of eval.hip uses scratch."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_PARAMS = ["ctx", "mem_space", "cols", "n_cols", "n_rows", "ops", "args", "n_ops", "out_mem_space", "out_data", "out_null_mask", "out_count"]
CHECK_PARAMS = ["col_dtypes", "n_cols", "ops", "args", "n_ops", "out_is_mask", "out_depth"]
NAMED = ["add_scalar", "sub_scalar", "mul_scalar", "div_scalar", "sqrt", "col_add", "col_sub", "col_mul", "col_div", "add_columns", "sub_columns",
         "mul_columns", "div_columns", "coalesce", "abs", "abs_column", "round", "round_column", "neg", "floor", "ceil", "trunc", "fract",
         "reciprocal", "mod_column", "floordiv", "clip", "clip_lower", "clip_upper", "where_cond", "mask", "fillna_zero", "replace_inf", "sign",
         "normalize", "with_column", "mask_of", "filter_expr"]
OP = R.OP


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
    df.add_column("x", F.Float64Column.with_nulls([0.5, np.nan, 1.0, 2.0], [False, False, True, False]))
    df.add_column("s", F.StringColumn(["a", "b", "c", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    return df


def _unary_calls(df):
    return [lambda c: df.add_scalar(c, 1.0), lambda c: df.sub_scalar(c, 1.0), lambda c: df.mul_scalar(c, 2.0), lambda c: df.div_scalar(c, 2.0),
            df.sqrt, df.abs, df.abs_column, lambda c: df.round(c, 2), lambda c: df.round_column(c, 2), df.neg, df.floor, df.ceil, df.trunc, df.fract,
            df.reciprocal, lambda c: df.mod_column(c, 2.0), lambda c: df.floordiv(c, 2.0), lambda c: df.clip(c, 0.0, 1.0),
            lambda c: df.clip_lower(c, 0.0), lambda c: df.clip_upper(c, 1.0), lambda c: df.where_cond(c, [True] * df.row_count(), 0.0),
            lambda c: df.mask(c, [True] * df.row_count(), 0.0), df.fillna_zero, lambda c: df.replace_inf(c, 0.0), df.sign]


def _binary_calls(df):
    return [df.col_add, df.col_sub, df.col_mul, df.col_div, df.add_columns, df.sub_columns, df.mul_columns, df.div_columns, df.coalesce]


def test_mirror_has_the_methods_the_builder_and_the_constants(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in NAMED:
        assert callable(getattr(F.OptimizedDataFrame, name)), name
    assert callable(E.Context.eval) and callable(E.Context.eval_check)
    assert callable(F.col) and callable(F.lit) and callable(F.where) and isinstance(F.col("a") * 2 > 1, F.Expr)
    for name, number in OP.items():
        assert getattr(built, "EVAL_" + name) == number
    assert (built.EVAL_MAX_OPS, built.EVAL_MAX_COLS, built.EVAL_MAX_DEPTH) == (64, 8, 8)
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_eval_op {"):header.index("} pandrs_hip_eval_op;")]
    assert dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_EVAL_(\w+) = (\d+)", body)) == OP
    for name in NAMED[:-3]:                                                # the docstrings cite the reference's lines
        assert re.search(r"(functions\.rs|math_ops\.rs):\d+", getattr(F.OptimizedDataFrame, name).__doc__ or ""), name


def test_the_builder_lowers_to_postfix():
    import pandrs_amd.frame as F
    names, prog = (F.col("a") * F.col("b") + 1.0 > 0).lower()
    assert names == ["a", "b"]
    assert prog == [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["MUL"], 0.0), (OP["CONST"], 1.0), (OP["ADD"], 0.0), (OP["CONST"], 0.0), (OP["GT"], 0.0)]
    names, prog = F.where((F.col("x") >= F.col("y")) & ~F.col("x").isnan(), F.col("x").abs().clip(0.0, 9.0), 2.0 - F.col("y")).lower()
    assert names == ["x", "y"]
    assert [op for op, _ in prog] == [OP[k] for k in ("COL", "COL", "GE", "COL", "ISNAN", "NOT", "AND", "COL", "ABS", "CONST", "MAX", "CONST", "MIN",
                                                      "CONST", "COL", "SUB", "SELECT")]
    assert R.check([R.F64, R.F64], prog) == (False, 4)
    assert [op for op, _ in (-(1.0 / F.col("a")) % 3.0).lower()[1]] == [OP[k] for k in ("CONST", "COL", "DIV", "NEG", "CONST", "REM")]
    for e in (F.col("a").floor(), F.col("a").ceil(), F.col("a").trunc(), F.col("a").round(), F.col("a").fract(), F.col("a").sqrt(), F.col("a").sign(),
              F.col("a").isinf(), F.col("a").isfinite(), F.col("a").max(1.0), F.col("a").min(F.col("b")), abs(F.col("a")), F.col("a") != 1,
              (F.col("a") < 1) | (F.col("a") == 2), F.col("a") <= F.lit(3)):
        R.check([R.F64, R.F64], e.lower()[1])
    with pytest.raises(F.InvalidValue):
        bool(F.col("a") > 1)                                               # `and` / `or` / chained compares cannot be overloaded
    with pytest.raises(F.InvalidValue):
        F.col("a") + "b"


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    for call in _unary_calls(df) + [df.normalize]:
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for c in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(c)
            assert "Column '%s' is not a numeric type" % c in str(e.value)
            with pytest.raises(type(e.value)) as d:                        # the message describe and rank use
                df.rank(c)
            assert str(d.value) == str(e.value)
    for call in _binary_calls(df):
        with pytest.raises(F.ColumnNotFound):
            call("x", "nope", "r")
        with pytest.raises(F.ColumnNotFound):
            call("nope", "x", "r")
        with pytest.raises(F.ColumnTypeMismatch):
            call("x", "s", "r")
        with pytest.raises(F.DuplicateColumnName):                         # the reference's DataFrame::add_column (base.rs:143-145)
            call("x", "id", "id")
    for call in (df.where_cond, df.mask):
        with pytest.raises(F.InvalidValue) as e:
            call("x", [True, False], 0.0)
        assert "Condition length must match column length" in str(e.value)
        with pytest.raises(F.InvalidValue):
            call("x", F.BooleanColumn([True] * 5), 0.0)
        with pytest.raises(F.ColumnNotFound):
            call("nope", [True, False], 0.0)                               # the column is looked up first
    # expressions: names, types and limits
    with pytest.raises(F.ColumnNotFound):
        df.with_column("r", F.col("x") + F.col("nope"))
    with pytest.raises(F.ColumnTypeMismatch) as e:
        df.with_column("r", F.col("s") + 1.0)
    assert "Column 's' is not a numeric type" in str(e.value)
    for bad in (F.col("x") + F.col("flag"), F.col("x") & F.col("flag"), ~F.col("x"), F.where(F.col("x"), 1.0, 2.0), F.where(F.col("flag"), 1.0, F.col("flag")),
                F.col("flag").isnan()):
        with pytest.raises(F.InvalidValue) as e:
            df.with_column("r", bad)
        assert re.search(r"op \d+", str(e.value))
    with pytest.raises(F.InvalidValue):
        df.with_column("r", F.col("x") > 1.0)                              # a condition is no column
    with pytest.raises(F.InvalidValue):
        df.mask_of(F.col("x") + 1.0)
    with pytest.raises(F.InvalidValue):
        df.filter_expr(F.col("x") + 1.0)
    with pytest.raises(F.InvalidValue):
        df.with_column("r", F.lit(1.0) + 2.0)                              # names no column
    e9 = F.col("x")
    for _ in range(8):                                                     # nine entries on the stack
        e9 = F.Expr(built.EVAL_ADD, children=(F.col("x"), e9))
    with pytest.raises(F.InvalidValue):
        df.with_column("r", e9)
    long = F.col("x")
    for _ in range(32):                                                    # 65 ops
        long = long + 1.0
    with pytest.raises(F.InvalidValue):
        df.with_column("r", long)
    nine = F.Float64Column([0.0] * 4)
    wide = _frame()
    expr = F.col("x")
    for k in range(8):
        wide.add_column("c%d" % k, nine)
        expr = expr + F.col("c%d" % k)
    with pytest.raises(F.InvalidValue):
        wide.with_column("r", expr)                                        # nine columns
    empty = F.OptimizedDataFrame()
    empty.add_column("a", F.Int64Column([]))
    empty.add_column("b", F.Float64Column([]))
    for call in _unary_calls(empty)[:-1]:
        for c in ("a", "b"):
            got = call(c)
            assert got.column_names == ["a", "b"] and got.row_count() == 0
    for call in _binary_calls(empty):
        got = call("a", "b", "r")
        assert got.column_names == ["a", "b", "r"] and got.row_count() == 0
    assert empty.sign("a") == [] and empty.mask_of(F.col("a") > 1) == [] and empty.filter_expr(F.col("a") > 1).column_names == ["a", "b"]
    assert empty.with_column("r", F.col("a") + 1).column_names == ["a", "b", "r"]
    with pytest.raises(F.InvalidValue):
        empty.normalize("a")                                               # value_range: no valid values (functions.rs:2274-2276)


def test_named_methods_hand_over_one_program_each(built, monkeypatch):
    """A stand-in context: every named method hands the column views, the row count and exactly the expected postfix program
    to Context.eval once and builds the reference's shape from what comes back."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        def eval(self, cols, n_rows, program, out=None, out_mask=None, out_device=None):
            calls.append(([c[2] for c in cols], n_rows, [(int(op), float(arg)) for op, arg in program], out_device))
            if R.check([c[2] for c in cols], program)[0]:
                return np.array([0x05], np.uint8), 2
            return np.array([1.0, 0.0, -3.0, 0.0]), np.array([0x02], np.uint8), 1

        def column_stats(self, col, n):
            return {"min": 1.0, "max": 5.0, "count": 4}

    monkeypatch.setattr(F, "get_context", lambda: Fake())
    df = _frame()
    P = lambda *names_args: [(OP[k], float(a)) for k, a in names_args]     # noqa: E731
    X = ("COL", 0)
    f2 = 100.0
    unary = [(lambda: df.add_scalar("x", 3), P(X, ("CONST", 3), ("ADD", 0))), (lambda: df.sub_scalar("x", 3), P(X, ("CONST", 3), ("SUB", 0))),
             (lambda: df.mul_scalar("x", 3), P(X, ("CONST", 3), ("MUL", 0))), (lambda: df.div_scalar("x", 3), P(X, ("CONST", 3), ("DIV", 0))),
             (lambda: df.sqrt("x"), P(X, ("SQRT", 0))), (lambda: df.abs("x"), P(X, ("ABS", 0))), (lambda: df.abs_column("x"), P(X, ("ABS", 0))),
             (lambda: df.round("x", 2), P(X, ("CONST", f2), ("MUL", 0), ("ROUND", 0), ("CONST", f2), ("DIV", 0))),
             (lambda: df.round_column("x", -2), P(X, ("CONST", 1.0 / f2), ("MUL", 0), ("ROUND", 0), ("CONST", 1.0 / f2), ("DIV", 0))),
             (lambda: df.neg("x"), P(X, ("NEG", 0))), (lambda: df.floor("x"), P(X, ("FLOOR", 0))), (lambda: df.ceil("x"), P(X, ("CEIL", 0))),
             (lambda: df.trunc("x"), P(X, ("TRUNC", 0))), (lambda: df.fract("x"), P(X, ("FRACT", 0))),
             (lambda: df.reciprocal("x"), P(("CONST", 1), X, ("DIV", 0))), (lambda: df.mod_column("x", 7), P(X, ("CONST", 7), ("REM", 0))),
             (lambda: df.floordiv("x", 7), P(X, ("CONST", 7), ("DIV", 0), ("FLOOR", 0))),
             (lambda: df.clip("x", -1, 1), P(X, ("CONST", -1), ("MAX", 0), ("CONST", 1), ("MIN", 0))),
             (lambda: df.clip("x", None, 1), P(X, ("CONST", 1), ("MIN", 0))), (lambda: df.clip_lower("x", -1), P(X, ("CONST", -1), ("MAX", 0))),
             (lambda: df.clip_upper("x", 1), P(X, ("CONST", 1), ("MIN", 0))),
             (lambda: df.fillna_zero("x"), P(X, ("ISNAN", 0), ("CONST", 0), X, ("SELECT", 0))),
             (lambda: df.replace_inf("x", 9), P(X, ("ISINF", 0), ("CONST", 9), X, ("SELECT", 0)))]
    for call, program in unary:
        del calls[:]
        got = call()
        assert calls == [([built.F64], 4, program, False)], program
        assert got.column_names == df.column_names and got.column("id") is df.column("id")          # replaced in position, the rest shared
        new = got.column("x")
        assert new.dtype == built.F64 and new.data.tolist()[::2] == [1.0, -3.0] and new.null_mask.tolist() == [0x02] and new.is_null(1)
    binary = [("col_add", "ADD"), ("col_sub", "SUB"), ("col_mul", "MUL"), ("col_div", "DIV"), ("add_columns", "ADD"), ("sub_columns", "SUB"),
              ("mul_columns", "MUL"), ("div_columns", "DIV")]
    for name, op in binary:
        del calls[:]
        got = getattr(df, name)("id", "x", "r")
        assert calls == [([built.I64, built.F64], 4, P(X, ("COL", 1), (op, 0)), False)]
        assert got.column_names == df.column_names + ["r"] and got.column("r").data[2] == -3.0
    del calls[:]
    df.coalesce("x", "id", "r")
    assert calls == [([built.F64, built.I64], 4, P(X, ("ISNAN", 0), ("COL", 1), X, ("SELECT", 0)), False)]
    del calls[:]
    got = df.where_cond("x", [True, False, True, True], 7.5)
    assert calls == [([built.BOOLBITS, built.F64], 4, P(X, ("COL", 1), ("CONST", 7.5), ("SELECT", 0)), False)] and got.column_names == df.column_names
    del calls[:]
    df.mask("id", df.column("flag"), 7.5)
    assert calls == [([built.BOOLBITS, built.I64], 4, P(X, ("CONST", 7.5), ("COL", 1), ("SELECT", 0)), False)]
    del calls[:]
    got = df.sign("x")
    assert calls == [([built.F64], 4, P(X, ("SIGN", 0)), False)] and got == [1, 0, -3, 0] and all(type(v) is int for v in got)
    del calls[:]
    got = df.normalize("id")                                               # (x - min) / range with two constants
    assert calls == [([built.I64], 4, P(X, ("CONST", 1.0), ("SUB", 0), ("CONST", 4.0), ("DIV", 0)), False)] and all(type(v) is float for v in got)
    del calls[:]
    assert df.mask_of((F.col("x") > F.col("id")) & F.col("flag")) == [True, False, True, False]
    assert calls == [([built.F64, built.I64, built.BOOLBITS], 4, P(X, ("COL", 1), ("GT", 0), ("COL", 2), ("AND", 0)), False)]
    del calls[:]
    got = df.with_column("x", F.col("x") * F.col("id") + 1.0)
    assert calls == [([built.F64, built.I64], 4, P(X, ("COL", 1), ("MUL", 0), ("CONST", 1), ("ADD", 0)), False)] and got.column_names == df.column_names
    assert df.with_column("new", F.col("x") + 0.0).column_names == df.column_names + ["new"]


def test_entry_point_without_a_context_is_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    ops = (C.c_int32 * 3)(built.EVAL_COL, built.EVAL_CONST, built.EVAL_ADD)
    args = (C.c_double * 3)(0.0, 1.0, 0.0)
    out, mask, cnt = np.full(8, -1.0), np.full(1, 0xAA, np.uint8), C.c_int64(-5)
    st = lib.pandrs_hip_eval(None, built.MEM_HOST, C.byref(col), 1, 8, ops, args, 3, built.MEM_HOST, out.ctypes.data, mask.ctypes.data, C.byref(cnt))
    assert st == built.ERR_NOT_INITIALIZED
    assert "context" in built.last_error() and (out == -1.0).all() and mask[0] == 0xAA and cnt.value == -5
    ops[2] = 99                                                            # the context is checked first, as everywhere else
    assert lib.pandrs_hip_eval(None, built.MEM_HOST, C.byref(col), 1, 8, ops, args, 3, built.MEM_HOST, out.ctypes.data, None, None) == built.ERR_NOT_INITIALIZED


def _c_check(built, dtypes, program):
    lib = built.load()
    dts = (C.c_int32 * max(len(dtypes), 1))(*dtypes)
    ops = (C.c_int32 * max(len(program), 1))(*[op for op, _ in program])
    args = (C.c_double * max(len(program), 1))(*[a for _, a in program])
    is_mask, depth = C.c_int32(-1), C.c_int32(-1)
    st = lib.pandrs_hip_eval_check(dts, len(dtypes), ops, args, len(program), C.byref(is_mask), C.byref(depth))
    return st, bool(is_mask.value), depth.value, built.last_error()


def test_eval_check_agrees_with_the_twin_on_random_programs(built):
    rng = np.random.default_rng(7)
    n_bad = n_good = 0
    ways = set()
    for k in range(500):
        dtypes = [int(d) for d in rng.choice([R.I64, R.F64, R.BOOLBITS], size=int(rng.integers(2, 9)))]
        if R.I64 not in dtypes and R.F64 not in dtypes:
            dtypes[0] = R.F64
        prog = R.random_program(rng, dtypes)
        if k % 2:                                                          # about half are made invalid, in each documented way
            way = ["underflow", "type", "leftover", "opcode", "column", "ninth", "ops65", "cols9", "u32"][(k // 2) % 9]
            at = int(rng.integers(0, len(prog)))
            if way == "underflow":
                prog = prog[at + 1:] if len(prog) > at + 1 and prog[at + 1][0] > OP["CONST"] else [(OP["ADD"], 0.0)] + prog
            elif way == "type":
                prog = prog + [(OP["NOT"], 0.0)] if not R.check(dtypes, prog)[0] else prog + [(OP["NEG"], 0.0)]
            elif way == "leftover":
                prog = (prog + [(OP["CONST"], 1.0)])[-R.MAX_OPS:] if len(prog) < R.MAX_OPS else [(OP["CONST"], 1.0)] + prog[1:]
            elif way == "opcode":
                prog[at] = (int(rng.choice([-1, 31, 1000])), 0.0)
            elif way == "column":
                prog = [(OP["COL"], float(rng.choice([-1.0, 0.5, len(dtypes), np.nan, np.inf])))] + prog[1:]
            elif way == "ninth":
                prog = [(OP["CONST"], 1.0)] * 9 + [(OP["ADD"], 0.0)] * 8
            elif way == "ops65":
                prog = [(OP["CONST"], 1.0)] + [(OP["NEG"], 0.0)] * 64
            elif way == "cols9":
                dtypes = [R.F64] * 9
            else:
                dtypes[0] = R.U32CODE
                prog = [(OP["COL"], 0.0)] + prog[1:]
            ways.add(way)
        st, is_mask, depth, msg = _c_check(built, dtypes, prog)
        try:
            want = R.check(dtypes, prog)
        except R.EvalError as e:
            n_bad += 1
            assert st == e.status, (k, prog, msg, str(e))
            if e.op_index is not None:
                assert "op %d:" % e.op_index in msg, (msg, str(e))          # pandrs_hip_last_error names the op index
            continue
        n_good += 1
        assert st == 0 and (is_mask, depth) == want, (k, prog, msg)
    assert len(ways) == 9 and n_bad >= 200 and n_good >= 250
    lib = built.load()                                                     # NULL arguments, NULL outputs
    ops, args, dts = (C.c_int32 * 1)(OP["CONST"]), (C.c_double * 1)(1.0), (C.c_int32 * 1)(R.F64)
    assert lib.pandrs_hip_eval_check(dts, 1, ops, args, 1, None, None) == 0
    assert lib.pandrs_hip_eval_check(None, 1, ops, args, 1, None, None) == built.ERR_INVALID_ARGUMENT
    assert lib.pandrs_hip_eval_check(dts, 1, None, args, 1, None, None) == built.ERR_INVALID_ARGUMENT


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    for name, params in (("pandrs_hip_eval", EVAL_PARAMS), ("pandrs_hip_eval_check", CHECK_PARAMS)):
        assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
        assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
        hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
        assert len(hp) == len(rp) == len(cp) == len(params)
        assert [n for n, _ in hp] == params
        for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
            assert hn == rn and ht == rt, (hn, ht, rt)
            assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    for k, v in OP.items():
        assert hdr[3]["PANDRS_HIP_EVAL_" + k] == v == rst[2]["PANDRS_HIP_EVAL_" + k] == getattr(built, "EVAL_" + k)
    assert open(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs")).read() == g.generate()
    block = header[header.index("/* ---- derived columns: one postfix program"):header.index("typedef enum pandrs_hip_eval_op")]
    for word in ("functions.rs:2819-2840", ":2851-2960", ":3890-3984", ":3846", ":237", ":1079-1139", ":3998-4014", ":2316-2337", "math_ops.rs",
                 "postfix", "2^53 + 1", "fmod", "f64::max", "half away from zero", "x - trunc(x)", "correctly rounded", "EPSILON", "cond ? a : b",
                 "0x7FF8000000000000", "n_ops <= 64", "n_cols <= 8", "at most 8 entries", "2^32", "LSB-first", "pandrs_hip_filter_indices",
                 "in place", "eval_tile_rows = ", "eval_blocks_per_cu = ", "three-address", "scratch", "kernel arguments", "ballots",
                 "one atomic add per workgroup", "PANDRS_HIP_PHASE_AGGREGATE", "Workspace", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY",
                 "NOT_INITIALIZED", "INVALID_ARGUMENT", "op index", "pow / log / exp", "replace_numeric", "zscore", "legacy", "multi-GPU"):
        assert word in block, word
    assert "eval.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "eval.hip")).read()
    assert int(re.search(r"eval_tile_rows = (\d+)", block).group(1)) == 2048 and "EVAL_TILE = EVAL_WAVES * EVAL_STEPS * 128" in src
    assert "EVAL_BLOCKS_PER_CU = %s;" % re.search(r"eval_blocks_per_cu = (\d+)", block).group(1) in src
    assert "#pragma clang fp contract(off)" in src and "__fma" not in src and "fma(" not in src


def test_cpp_mirror_eval_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "eval_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "eval_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr


def test_no_kernel_of_eval_hip_uses_scratch(built):
    """A private array indexed by a run-time stack pointer goes to scratch; the lowered program picks named registers instead.
    eval.hip compiled with the Makefile's flags: every kernel's code object metadata reports a private segment of 0 bytes."""
    csrc = os.path.join(ROOT, "pandrs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "eval.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, "eval.hip"), "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    kernels = re.findall(r"\.name:\s+(\S*eval_kernel\S*)", text)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(kernels) >= 2 and len(kernels) == len(sizes) == len(re.findall(r"^\s+\.name:\s+\S+\s*$", text, re.M)), (kernels, sizes)    # every kernel of the file
    assert sizes and all(v == 0 for v in sizes), sizes
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
