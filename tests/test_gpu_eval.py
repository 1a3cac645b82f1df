"""pandrs_hip_eval and the mirrors' derived columns (reference src/dataframe/pandas_compat/functions.rs:237, :1079-1139, :2316-2337,
:2819-2960, :3846-4118 and helpers/math_ops.rs) against tests/eval_ref.py.  Every comparison is bit for bit: the cells (the uint64
view), the null mask, the count and the bitmap.  The one exception the header names is MAX / MIN of +0.0 and -0.0: the twin reports
such rows, the inputs are free of them and the tests assert that nothing was skipped."""
import math
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests import eval_ref as R  # noqa: E402
from tests.test_eval_ref import I64_SPECIAL, special_pairs  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
T = int(re.search(r"eval_tile_rows = (\d+)", HEADER).group(1))
PER_CU = int(re.search(r"eval_blocks_per_cu = (\d+)", HEADER).group(1))
OP = R.OP
FUSED = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["MUL"], 0.0), (OP["COL"], 2.0), (OP["ADD"], 0.0)]                      # a * b + c
COND = FUSED + [(OP["CONST"], 0.0), (OP["GT"], 0.0), (OP["COL"], 0.0), (OP["ISNAN"], 0.0), (OP["NOT"], 0.0), (OP["AND"], 0.0)]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def view(col):
    """A twin column (data, nulls, dtype) as the engine takes it on the host."""
    data, nulls, dt = col
    mask = None if nulls is None else R.pack(nulls)
    return (R.pack(data) if dt == R.BOOLBITS else np.ascontiguousarray(data), mask, dt)


def device(col, shift=False):
    """The same column in device memory; with `shift` the data sits at 8 mod 16 and the masks / bits at byte offset 1."""
    import torch
    data, mask, dt = view(col)

    def up(a, lead):
        t = torch.empty(len(a) + lead, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
        t[lead:] = torch.from_numpy(a)
        return t[lead:]
    d = up(data, 1 if shift else 0)
    if dt != R.BOOLBITS:
        assert d.data_ptr() % 16 == (8 if shift else 0)
    return (d, None if mask is None else up(mask, 1 if shift else 0), dt)


def to_host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def check(ctx, cols, n, program, passed=None, want=None, **kw):
    """One program against the twin: the cells and the null mask, or the bitmap, and the count.  -> the twin's result."""
    want = R.evaluate(cols, n, program) if want is None else want
    assert not want.zero_tie, "the inputs hold a MAX / MIN of opposite zeros"
    got = ctx.eval([view(c) for c in cols] if passed is None else passed, n, program, **kw)
    if want.is_mask:
        bits, count = got
        bits = to_host(bits)
        assert bits.shape[0] == (n + 7) // 8 and np.array_equal(bits, R.pack(want.mask)), np.flatnonzero(R.unpack(bits, n) != want.mask)[:5]
        assert count == want.count
        return want
    values, mask, n_null = got
    values, mask = to_host(values), to_host(mask)
    assert values.dtype == np.float64 and values.shape[0] == n
    diff = np.flatnonzero(values.view(np.uint64) != want.values.view(np.uint64))
    assert diff.size == 0, (diff[:5], values[diff[:5]], want.values[diff[:5]])
    assert n_null == want.count and (mask is None) == (n_null == 0)
    if mask is not None:
        assert np.array_equal(mask, R.pack(want.nulls))
    return want


three = R.three_columns


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- row counts: the pair loads' tail, the ballot word, the tile edge, the stride ------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1])
def test_row_counts_around_the_word_and_the_tile(ctx, n):
    cols = three(n, seed=n + 1)
    abc = [cols[0], cols[1], cols[0]]
    for place in (None, False, True) if n else (None,):                    # host, device, device at 8 mod 16 / byte offset 1
        passed = None if place is None else [device(c, shift=place) for c in abc]
        check(ctx, abc, n, FUSED, passed)
        check(ctx, abc, n, COND, passed)
    check(ctx, cols, n, [(OP["COL"], 2.0), (OP["COL"], 0.0), (OP["COL"], 1.0), (OP["SELECT"], 0.0)])


def test_the_grid_strides_into_a_second_iteration(ctx):
    n = PER_CU * n_cu() * T + 1
    rng = np.random.default_rng(5)
    a = rng.integers(-999, 999, n).astype(np.float64) / 8.0
    b = rng.integers(1, 99, n).astype(np.int64)
    nulls = np.zeros(n, bool)
    nulls[[0, T - 1, T, n - 2, n - 1]] = True
    cols = [(a, nulls, R.F64), (b, None, R.I64), (a, nulls, R.F64)]
    passed = [device(c, shift=True) for c in cols[:2]]
    want = check(ctx, cols, n, FUSED, passed + [passed[0]])
    assert want.count == 5
    check(ctx, cols, n, COND, passed + [passed[0]])


# ---- every opcode over the special values ----------------------------------------------------------------------------------------
def test_every_opcode_on_the_special_values(ctx):
    a, b = special_pairs()
    n = len(a)
    rng = np.random.default_rng(3)
    an, bn = rng.random(n) < 0.2, rng.random(n) < 0.2
    ia = np.array([I64_SPECIAL[i % len(I64_SPECIAL)] for i in range(n)], dtype=np.int64)
    ib = np.array([I64_SPECIAL[(i // len(I64_SPECIAL)) % len(I64_SPECIAL)] for i in range(n)], dtype=np.int64)
    ib[(ia == 0) & (ib == 0)] = 1
    skipped = 0
    for x, y in (((a, None, R.F64), (b, None, R.F64)), ((a, an, R.F64), (b, bn, R.F64)), ((ia, None, R.I64), (ib, None, R.I64)),
                 ((ia, an, R.I64), (b, bn, R.F64))):
        for name in R.NAMES[2:]:
            op = OP[name]
            if op in R.BINARY_VALUE or op in R.COMPARE:
                prog = [(OP["COL"], 0.0), (OP["COL"], 1.0), (op, 0.0)]
            elif op in R.UNARY_VALUE or op in R.CLASSIFY:
                prog = [(OP["COL"], 0.0), (op, 0.0)]
            elif name == "NOT":
                prog = [(OP["COL"], 0.0), (OP["ISNAN"], 0.0), (op, 0.0)]
            elif name == "SELECT":
                prog = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["LT"], 0.0), (OP["COL"], 0.0), (OP["COL"], 1.0), (op, 0.0)]
            else:
                prog = [(OP["COL"], 0.0), (OP["CONST"], 0.0), (OP["GT"], 0.0), (OP["COL"], 1.0), (OP["ISFINITE"], 0.0), (op, 0.0)]
            want = R.evaluate([x, y], n, prog)
            if want.zero_tie:                                               # (a null cell is NaN: no tie comes from a mask)
                skipped += 1
                continue
            check(ctx, [x, y], n, prog, want=want)
    assert skipped == 0
    # the one dedicated case: either zero is accepted
    z = [(np.array([0.0, -0.0]), None, R.F64), (np.array([-0.0, 0.0]), None, R.F64)]
    for name in ("MAX", "MIN"):
        values, mask, n_null = ctx.eval([view(c) for c in z], 2, [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP[name], 0.0)])
        assert values[0] == 0.0 and values[1] == 0.0 and mask is None and n_null == 0


def test_a_product_and_a_sum_are_rounded_separately(ctx):
    e = 2.0 ** -30
    cols = [(np.full(300, 1.0 + e), None, R.F64), (np.full(300, 1.0 - e), None, R.F64), (np.full(300, -1.0), None, R.F64)]
    values, _, _ = ctx.eval([view(c) for c in cols], 300, FUSED)
    assert (values == 0.0).all()                                            # a fused multiply-add gives -2^-60
    check(ctx, cols, 300, FUSED)


# ---- random programs -------------------------------------------------------------------------------------------------------------
def test_random_programs(ctx):
    n = R.RANDOM_ROWS
    cols = three(n, seed=11)
    passed = [device(c, shift=True) for c in cols]
    dtypes = [c[2] for c in cols]
    rng = np.random.default_rng(R.RANDOM_SEED)            # test_eval_ref.py: the twin alone skips none of these
    skipped, masks, longest, deepest = 0, 0, 0, 0
    for k in range(R.RANDOM_PROGRAMS):
        prog = R.random_program(rng, dtypes)
        want = R.evaluate(cols, n, prog)
        if want.zero_tie:
            skipped += 1
            continue
        masks += want.is_mask
        longest, deepest = max(longest, len(prog)), max(deepest, R.check(dtypes, prog)[1])
        check(ctx, cols, n, prog, passed if k % 2 else None, want=want)
    assert skipped == 0 and 20 < masks < 180 and longest >= 56 and deepest == 8


# ---- the limits ------------------------------------------------------------------------------------------------------------------
def test_the_limits_and_one_past_each(ctx):
    import pandrs_amd as pa
    n = 130
    rng = np.random.default_rng(2)
    cols = [(rng.integers(-50, 50, n).astype(np.float64) + 0.5, None, R.F64) for _ in range(8)]
    eight = [(OP["COL"], float(j)) for j in range(8)] + [(OP["ADD"], 0.0)] * 7                          # 8 columns, depth 8
    check(ctx, cols, n, eight)
    longest = eight + [(OP["NEG"], 0.0), (OP["ABS"], 0.0)] * 24 + [(OP["SQRT"], 0.0)]                   # 64 ops
    assert len(longest) == 64
    check(ctx, cols, n, longest)

    def refused(c, program, status=L.ERR_INVALID_ARGUMENT, word=None):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.eval([view(x) for x in c], n, program)
        assert e.value.status == status and (word is None or word in str(e.value)), str(e.value)
    refused(cols, longest + [(OP["NEG"], 0.0)])                                                          # 65 ops
    refused(cols + cols[:1], eight)                                                                      # 9 columns
    refused(cols, [(OP["COL"], 0.0)] * 9 + [(OP["ADD"], 0.0)] * 8, word="op 8")                          # depth 9
    refused(cols, [(OP["COL"], 0.0), (OP["ADD"], 0.0)], word="op 1")
    refused(cols, [(OP["COL"], 0.0), (OP["COL"], 1.0)], word="op 1")
    refused(cols, [(OP["COL"], 8.0)], word="op 0")
    refused(cols, [(OP["COL"], 0.0), (31, 0.0)], word="op 1")
    refused(cols, [(OP["COL"], 0.0), (OP["NOT"], 0.0)], word="op 1")
    codes = (np.arange(n, dtype=np.uint32), None, R.U32CODE)
    refused([cols[0], codes], [(OP["COL"], 1.0)], status=L.ERR_TYPE_MISMATCH)
    check(ctx, [cols[0], codes], n, [(OP["COL"], 0.0)], passed=[view(cols[0]), codes])                  # a column nobody names is not looked at


# ---- memory spaces, outputs, in place --------------------------------------------------------------------------------------------
def test_host_device_and_resident_inputs_and_both_outputs(ctx):
    import torch
    n = T + 77
    cols = three(n, seed=4)
    value_prog = FUSED[:3] + [(OP["COL"], 2.0), (OP["COL"], 0.0), (OP["CONST"], -1.0), (OP["SELECT"], 0.0), (OP["ADD"], 0.0)]
    mask_prog = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["GT"], 0.0), (OP["COL"], 2.0), (OP["OR"], 0.0)]
    for prog in (value_prog, mask_prog):
        want = R.evaluate(cols, n, prog)
        resident = [ctx.upload_column_n(*view(c), n) for c in cols]
        try:
            for passed in (None, [device(c) for c in cols], resident):
                for out_device in (None, False, True):
                    check(ctx, cols, n, prog, passed, want=want, out_device=out_device)
            res = ctx.eval(resident, n, prog)
            assert type(res[0]).__module__.startswith("torch")                                           # device in, device out by default
        finally:
            for r in resident:
                r.release()
        # outputs the caller owns: host arrays, device tensors at 8 mod 16 / byte offset 1, nothing past the end is touched
        if want.is_mask:
            nbytes = (n + 7) // 8
            out = np.full(nbytes + 3, 0xEE, np.uint8)
            bits, count = ctx.eval([view(c) for c in cols], n, prog, out=out[:nbytes])
            assert np.array_equal(out[:nbytes], R.pack(want.mask)) and (out[nbytes:] == 0xEE).all() and count == want.count
            dev = torch.full((nbytes + 4,), 0xEE, dtype=torch.uint8, device="cuda")
            ctx.eval([device(c) for c in cols], n, prog, out=dev[1:1 + nbytes])
            got = dev.cpu().numpy()
            assert got[0] == 0xEE and np.array_equal(got[1:1 + nbytes], R.pack(want.mask)) and (got[1 + nbytes:] == 0xEE).all()
        else:
            nbytes = (n + 7) // 8
            dev = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
            dmask = torch.full((nbytes + 4,), 0xEE, dtype=torch.uint8, device="cuda")
            assert dev[1:].data_ptr() % 16 == 8
            values, mask, n_null = ctx.eval([device(c) for c in cols], n, prog, out=dev[1:1 + n], out_mask=dmask[1:1 + nbytes])
            assert np.array_equal(dev[1:1 + n].cpu().numpy().view(np.uint64), want.values.view(np.uint64)) and float(dev[0]) == 0.0 and float(dev[n + 1]) == 0.0
            got = dmask.cpu().numpy()
            assert got[0] == 0xEE and np.array_equal(got[1:1 + nbytes], R.pack(want.nulls)) and (got[1 + nbytes:] == 0xEE).all() and n_null == want.count


def test_in_place_is_refused_as_documented(ctx):
    import pandrs_amd as pa
    import torch
    n = 1000
    x = torch.arange(n, dtype=torch.float64, device="cuda")
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    for kw in (dict(out=x), dict(out_mask=x.view(torch.uint8)[: (n + 7) // 8])):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.eval([(x, None, L.F64)], n, [(OP["COL"], 0.0), (OP["NEG"], 0.0)], **kw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "in place" in str(e.value)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.eval([(bits, None, L.BOOLBITS)], n, [(OP["COL"], 0.0), (OP["NOT"], 0.0)], out=bits)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "in place" in str(e.value)
    assert torch.equal(x, torch.arange(n, dtype=torch.float64, device="cuda")) and int(bits.sum()) == 0
    # the bitmap itself goes into the compaction where it is: filter_indices takes it in place
    got, count = ctx.eval([(x, None, L.F64)], n, [(OP["COL"], 0.0), (OP["CONST"], 3.0), (OP["REM"], 0.0), (OP["CONST"], 0.0), (OP["EQ"], 0.0)])
    rows, k = ctx.filter_indices((got, None, L.BOOLBITS), n)
    assert k == count == 334 and rows.cpu().numpy().tolist() == list(range(0, n, 3))


# ---- chains that never visit the host --------------------------------------------------------------------------------------------
def test_predicate_where_cond_groupby_stays_on_the_device(ctx):
    import torch
    n = 3 * T + 5
    rng = np.random.default_rng(8)
    key = rng.integers(0, 37, n).astype(np.int64)
    v = rng.integers(-100, 100, n).astype(np.float64)
    dkey, dv = torch.from_numpy(key).cuda(), torch.from_numpy(v).cuda()
    where = [(OP["COL"], 0.0), (OP["COL"], 1.0), (OP["CONST"], 0.0), (OP["SELECT"], 0.0)]
    mask, _ = ctx.predicate((dv, None, L.F64), n, L.PRED_GT, 10.0, out_device=True)
    vals, _, _ = ctx.eval([(mask, None, L.BOOLBITS), (dv, None, L.F64)], n, where, out_device=True)
    assert type(mask).__module__.startswith("torch") and type(vals).__module__.startswith("torch")
    kc, _, sums = ctx.groupby_agg([(dkey, None, L.I64)], n, [(vals, None, L.F64)], [(0, L.SUM)])
    on_device = dict(zip(kc[0].cpu().numpy().astype(np.int64).tolist(), sums[0].cpu().numpy().tolist()))
    # the same chain through host lists
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column(key))
    df.add_column("v", F.Float64Column(v))
    cond = df.gt("v", 10.0)
    host_vals = df.where_cond("v", cond, 0.0).column("v").data
    hk, _, hs = ctx.groupby_agg([(key, None, L.I64)], n, [(host_vals, None, L.F64)], [(0, L.SUM)])
    through_host = dict(zip(np.asarray(hk[0]).astype(np.int64).tolist(), np.asarray(hs[0]).tolist()))
    assert on_device == through_host and len(on_device) == 37
    assert on_device == {int(k): float(np.where(v > 10.0, v, 0.0)[key == k].sum()) for k in range(37)}       # integers: exact in any order
    # the frame takes the device mask as it is
    got = df.where_cond("v", mask, 0.0).column("v").data
    assert np.array_equal(got.view(np.uint64), host_vals.view(np.uint64))


def _wide_frame(n, seed=6):
    import pandrs_amd.frame as F
    cols = three(n, seed)
    df = F.OptimizedDataFrame()
    df.add_column("a", F.Float64Column(cols[0][0]))
    df.add_column("b", F.Int64Column.with_nulls(cols[1][0], cols[1][1]))
    df.add_column("flag", F.BooleanColumn.with_nulls(cols[2][0], cols[2][1]))
    df.add_column("s", F.StringColumn(["r%d" % (i % 7) for i in range(n)]))
    return df, cols


def test_filter_expr_equals_mask_of_then_select_by_mask(ctx):
    import pandrs_amd.frame as F
    n = T + 300
    df, cols = _wide_frame(n)
    expr = (F.col("a") * F.col("b") + 1.0 > 0) & ~F.col("flag")
    want = R.evaluate(cols, n, expr.lower()[1])
    mask = df.mask_of(expr)
    assert mask == want.mask.tolist() and 0 < want.count < n
    a, b = df.filter_expr(expr), df.select_by_mask(mask)
    assert a.column_names == b.column_names == df.column_names and a.row_count() == b.row_count() == want.count
    for name in df.column_names:
        assert np.array_equal(a.column(name).data, b.column(name).data), name
    none = df.filter_expr(F.col("a") > math.inf)
    assert none.row_count() == 0 and none.column_names == df.column_names


def test_every_named_method_against_the_twin(ctx):
    import pandrs_amd.frame as F
    n = 700
    df, cols = _wide_frame(n)
    A, B = cols[0], cols[1]
    P = lambda *xs: [(OP[k], float(v)) for k, v in xs]                      # noqa: E731
    X, Y = ("COL", 0), ("COL", 1)

    def column(frame, name, want_cols, prog, position=None):
        want = R.evaluate(want_cols, n, prog)
        assert not want.zero_tie
        c = frame.column(name)
        assert c.dtype == L.F64 and np.array_equal(np.asarray(c.data).view(np.uint64), want.values.view(np.uint64)), name
        assert (c.null_mask is None) == (want.count == 0) and (c.null_mask is None or np.array_equal(c.null_mask, R.pack(want.nulls)))
        assert frame.column_names == (df.column_names if position is None else df.column_names + [name])
    for col_, src in (("a", A), ("b", B)):
        column(df.add_scalar(col_, 2.5), col_, [src], P(X, ("CONST", 2.5), ("ADD", 0)))
        column(df.sub_scalar(col_, 2.5), col_, [src], P(X, ("CONST", 2.5), ("SUB", 0)))
        column(df.mul_scalar(col_, 1.1), col_, [src], P(X, ("CONST", 1.1), ("MUL", 0)))
        column(df.div_scalar(col_, 3.0), col_, [src], P(X, ("CONST", 3.0), ("DIV", 0)))
        for name in ("sqrt", "abs", "abs_column", "neg", "floor", "ceil", "trunc", "fract"):
            column(getattr(df, name)(col_), col_, [src], P(X, (name.split("_")[0].upper(), 0)))
        column(df.reciprocal(col_), col_, [src], P(("CONST", 1.0), X, ("DIV", 0)))
        column(df.mod_column(col_, 7.0), col_, [src], P(X, ("CONST", 7.0), ("REM", 0)))
        column(df.floordiv(col_, 7.0), col_, [src], P(X, ("CONST", 7.0), ("DIV", 0), ("FLOOR", 0)))
        for d in (2, 0, -1):
            f = 10.0 ** abs(d) if d >= 0 else 1.0 / 10.0 ** abs(d)
            column(df.round(col_, d), col_, [src], P(X, ("CONST", f), ("MUL", 0), ("ROUND", 0), ("CONST", f), ("DIV", 0)))
        column(df.round_column(col_, 1), col_, [src], P(X, ("CONST", 10.0), ("MUL", 0), ("ROUND", 0), ("CONST", 10.0), ("DIV", 0)))
        column(df.clip(col_, -20.0, 30.0), col_, [src], P(X, ("CONST", -20.0), ("MAX", 0), ("CONST", 30.0), ("MIN", 0)))
        column(df.clip_lower(col_, -20.0), col_, [src], P(X, ("CONST", -20.0), ("MAX", 0)))
        column(df.clip_upper(col_, 30.0), col_, [src], P(X, ("CONST", 30.0), ("MIN", 0)))
        column(df.fillna_zero(col_), col_, [src], P(X, ("ISNAN", 0), ("CONST", 0.0), X, ("SELECT", 0)))
        column(df.replace_inf(col_, -9.0), col_, [src], P(X, ("ISINF", 0), ("CONST", -9.0), X, ("SELECT", 0)))
        want = R.evaluate([src], n, P(X, ("SIGN", 0)))
        assert df.sign(col_) == [int(v) for v in want.values]
        cond = (np.arange(n) % 3 == 0)
        column(df.where_cond(col_, cond.tolist(), 1.5), col_, [(cond, None, R.BOOLBITS), src], P(X, Y, ("CONST", 1.5), ("SELECT", 0)))
        column(df.mask(col_, cond.tolist(), 1.5), col_, [(cond, None, R.BOOLBITS), src], P(X, ("CONST", 1.5), Y, ("SELECT", 0)))
        column(df.where_cond(col_, df.column("flag"), 1.5), col_, [cols[2], src], P(X, Y, ("CONST", 1.5), ("SELECT", 0)))
    for name, op in (("col_add", "ADD"), ("col_sub", "SUB"), ("col_mul", "MUL"), ("col_div", "DIV"), ("add_columns", "ADD"), ("sub_columns", "SUB"),
                     ("mul_columns", "MUL"), ("div_columns", "DIV")):
        column(getattr(df, name)("a", "b", "r"), "r", [A, B], P(X, Y, (op, 0)), position=-1)
    column(df.coalesce("a", "b", "r"), "r", [A, B], P(X, ("ISNAN", 0), Y, X, ("SELECT", 0)), position=-1)
    column(df.with_column("r", F.where(F.col("flag"), F.col("a"), -F.col("b"))), "r", [cols[2], A, B], P(X, Y, ("COL", 2), ("NEG", 0), ("SELECT", 0)), position=-1)
    # clip of NaN: to the bound
    nan_df = F.OptimizedDataFrame()
    nan_df.add_column("x", F.Float64Column([math.nan, -5.0, 5.0, math.nan]))
    assert nan_df.clip("x", -1.0, 1.0).column("x").data.tolist() == [-1.0, -1.0, 1.0, -1.0]
    assert nan_df.clip("x", None, 1.0).column("x").data.tolist() == [1.0, -5.0, 1.0, 1.0]
    # normalize: min / max from the whole-column reduction, NaN stays NaN
    finite = np.where(np.isfinite(A[0]), A[0], np.nan)
    norm_df = F.OptimizedDataFrame()
    norm_df.add_column("x", F.Float64Column(finite))
    lo, hi = float(np.nanmin(finite)), float(np.nanmax(finite))
    want = R.evaluate([(finite, None, R.F64)], n, P(X, ("CONST", lo), ("SUB", 0), ("CONST", hi - lo), ("DIV", 0)))
    got = np.array(norm_df.normalize("x"))
    assert np.array_equal(got.view(np.uint64), want.values.view(np.uint64)) and np.nanmin(got) == 0.0 and np.nanmax(got) == 1.0
    flat = F.OptimizedDataFrame()
    flat.add_column("x", F.Float64Column([2.0, 2.0, math.nan]))
    with pytest.raises(F.InvalidValue):
        flat.normalize("x")
    allnan = F.OptimizedDataFrame()
    allnan.add_column("x", F.Float64Column([math.nan, math.nan]))
    with pytest.raises(F.InvalidValue):
        allnan.normalize("x")


# ---- stale workspace ------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_workspace_held(ctx):
    """Angle (a) of test_gpu_workspace.py for this entry point: every workspace block filled with 0x00, 0xFF and 0xA5 before the
    call uses it; the results keep their bits and the filled-bytes counter moves."""
    import pandrs_amd as pa
    n = 2 * T + 9
    cols = three(n, seed=9)
    progs = [FUSED[:3], COND[:3] + [(OP["CONST"], 0.0), (OP["GT"], 0.0), (OP["COL"], 2.0), (OP["AND"], 0.0)]]
    wants = [R.evaluate(cols, n, p) for p in progs]
    try:
        for byte in (0x00, 0xFF, 0xA5):
            pa.Context.poison_workspace(byte)
            before = pa.Context.workspace_poisoned_bytes()
            for p, w in zip(progs, wants):
                check(ctx, cols, n, p, want=w)                              # host columns: the staging arena and the counter
                check(ctx, cols, n, p, [device(c) for c in cols], want=w)
            assert pa.Context.workspace_poisoned_bytes() > before
    finally:
        pa.Context.poison_workspace(None)
