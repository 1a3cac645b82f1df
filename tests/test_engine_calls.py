"""What pandrs_amd.engine.Context hands to the C ABI and what it gives back, without a library or a device: `lib` is a
recorder, so every case states the symbol a method calls and its arguments literally - the memory-space arguments, the
null-pointer rule of each call, the buffer a caller gets back, and every ValueError the wrapper raises before it calls.
One GPU function at the end runs the same buffer conventions through the real library."""
import ctypes as C

import numpy as np
import pytest

import pandrs_amd.engine as E
from pandrs_amd import _lib as L

H, N, P = "null", "null", "ptr"             # the context's handle (None here), a null pointer, any other pointer
HOST = L.MEM_HOST
ROWS = (0, 1, 9)                            # the empty call, one row, a bitmap that ends inside a byte


def nb(n):
    return (n + 7) // 8


def _norm(arg, ctype):
    """One argument of a recorded call in a form two calls can be compared by."""
    if arg is None:
        return "null"
    if isinstance(arg, C.Array):
        if arg._type_ is L.Column:
            return [(not c.data, not c.null_mask, c.dtype) for c in arg]
        return list(arg)
    if type(arg).__name__ == "CArgObject":                      # C.byref(x): the value the call was given
        x = arg._obj
        return tuple(getattr(x, f) for f, _ in x._fields_) if isinstance(x, C.Structure) else x.value
    if isinstance(arg, C._SimpleCData):
        return arg.value
    if isinstance(arg, C._Pointer):
        return "ptr" if arg else "null"
    if ctype is C.c_void_p:
        return "ptr" if arg else "null"
    return arg


class Recorder:
    """Any attribute is a C function that records (symbol, arguments), writes `results[symbol][i]` through the byref that
    is argument i, and returns status 0."""

    def __init__(self):
        self.calls = []
        self.results = {}

    def __getattr__(self, name):
        ctypes_of = L.SYMBOLS[name][1]

        def fn(*args):
            assert len(args) == len(ctypes_of), (name, len(args))
            self.calls.append((name, tuple(_norm(a, t) for a, t in zip(args, ctypes_of))))
            for i, value in self.results.get(name, {}).items():
                args[i]._obj.value = value
            return 0
        return fn


@pytest.fixture
def ctx(monkeypatch):
    c = E.Context.__new__(E.Context)
    c.device, c.h, c.grouping_token = 0, None, 0
    c.lib = Recorder()
    c.waits = 0

    def wait():
        c.waits += 1
    c._wait_for_producer = wait                                 # a host call never waits for torch's stream
    monkeypatch.setattr(L, "load", lambda: c.lib)               # eval's validator and _raise's message go to the recorder too
    return c


def f64(n):
    return (np.arange(n, dtype=np.float64), None, L.F64)


def i64(n):
    return (np.arange(n, dtype=np.int64), None, L.I64)


def one_call(ctx, symbol=None):
    assert ctx.waits == 0
    calls = [c for c in ctx.lib.calls if symbol is None or c[0] == symbol]
    assert len(calls) == 1, ctx.lib.calls
    ctx.lib.calls.clear()
    return calls[0]


def is_host(a, dtype, count):
    return isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (count,)


def is_view(a, out, dtype, count):
    return is_host(a, dtype, count) and (count == 0 or (np.shares_memory(a, out) and a.ctypes.data == out.ctypes.data))


COL = [(False, True, L.F64)]                # one F64 column: data given, no mask
COL_I = [(False, True, L.I64)]


# ---- one 8-byte cell per row: rank, topk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_rank(ctx, n):
    got = ctx.rank(f64(n), n, L.RANK_MIN)
    assert one_call(ctx) == ("pandrs_hip_rank", (H, HOST, COL, n, L.RANK_MIN, HOST, P if n else N))
    assert is_host(got, np.float64, n)
    out = np.zeros(n + 2)
    got = ctx.rank(f64(n), n, L.RANK_DENSE, out=out, out_device=True)         # a given out decides, not out_device
    assert one_call(ctx) == ("pandrs_hip_rank", (H, HOST, COL, n, L.RANK_DENSE, HOST, P if n else N))
    assert is_view(got, out, np.float64, n)
    got = ctx.rank(f64(n), n, L.RANK_MIN, out_device=False)
    assert one_call(ctx)[1][5] == HOST and is_host(got, np.float64, n)


@pytest.mark.parametrize("n", ROWS)
def test_topk(ctx, n):
    k = 4
    kk = min(k, n)
    ctx.lib.results["pandrs_hip_topk"] = {8: kk, 9: max(kk - 1, 0)}
    rows, numbers = ctx.topk(f64(n), n, k)
    assert one_call(ctx) == ("pandrs_hip_topk", (H, HOST, COL, n, k, L.TOPK_LARGEST, HOST, P if kk else N, 0, 0))
    assert is_host(rows, np.int64, kk) and numbers == max(kk - 1, 0)
    out = np.zeros(kk + 2, np.int64)
    rows, _ = ctx.topk(f64(n), n, k, largest=False, out=out)
    assert one_call(ctx) == ("pandrs_hip_topk", (H, HOST, COL, n, k, L.TOPK_SMALLEST, HOST, P if kk else N, 0, 0))
    assert is_view(rows, out, np.int64, kk)
    ctx.lib.results["pandrs_hip_topk"] = {8: 0, 9: 0}
    rows, numbers = ctx.topk(f64(n), n, -3)                                   # k < 0: nothing asked for, no pointer
    assert one_call(ctx) == ("pandrs_hip_topk", (H, HOST, COL, n, -3, L.TOPK_LARGEST, HOST, N, 0, 0))
    assert is_host(rows, np.int64, 0) and numbers == 0


# ---- a cell per row and a null bitmap: fill, cumulative, lag, grouped, a value program --------------------------------------
def cell_cases(n):
    """(name, symbol, the call, its arguments between the row count and the output space, cell dtype, index of the byref)"""
    return [
        ("fill ffill", "pandrs_hip_fill", lambda c, **kw: c.fill(f64(n), n, L.FILL_FFILL, **kw), COL, (L.FILL_FFILL, 0), np.float64, 9),
        ("fill i64 value", "pandrs_hip_fill", lambda c, **kw: c.fill(i64(n), n, L.FILL_VALUE, -1, **kw), COL_I,
         (L.FILL_VALUE, 0xFFFFFFFFFFFFFFFF), np.int64, 9),
        ("fill i64 linear", "pandrs_hip_fill", lambda c, **kw: c.fill(i64(n), n, L.FILL_LINEAR, **kw), COL_I, (L.FILL_LINEAR, 0), np.float64, 9),
        ("fill f64 value", "pandrs_hip_fill", lambda c, **kw: c.fill(f64(n), n, L.FILL_VALUE, 1.5, **kw), COL,
         (L.FILL_VALUE, 0x3FF8000000000000), np.float64, 9),
        ("cumulative sum", "pandrs_hip_cumulative", lambda c, **kw: c.cumulative(f64(n), n, L.CUM_SUM, **kw), COL, (L.CUM_SUM,), np.float64, 8),
        ("cumulative count", "pandrs_hip_cumulative", lambda c, **kw: c.cumulative(f64(n), n, L.CUM_COUNT, **kw), COL, (L.CUM_COUNT,),
         np.int64, 8),
        ("lag", "pandrs_hip_lag", lambda c, **kw: c.lag(i64(n), n, L.LAG_DIFF, 2, **kw), COL_I, (L.LAG_DIFF, 2), np.float64, 9),
        ("grouped shift", "pandrs_hip_grouped", lambda c, **kw: c.grouped(f64(n), n, L.GROUPED_SHIFT, -1, **kw), COL,
         (L.GROUPED_SHIFT, -1), np.float64, 9),
        ("grouped row number", "pandrs_hip_grouped", lambda c, **kw: c.grouped(None, n, L.GROUPED_ROW_NUMBER, **kw), N,
         (L.GROUPED_ROW_NUMBER, 0), np.int64, 9),
    ]


@pytest.mark.parametrize("n", ROWS)
def test_cell_ops(ctx, n):
    for name, symbol, call, col, middle, dtype, ref in cell_cases(n):
        want = (symbol, (H, HOST, col, n) + middle + (HOST, P if n else N, P if n else N, 0))
        values, mask, count = call(ctx)
        assert one_call(ctx) == want, name
        assert is_host(values, dtype, n) and mask is None and count == 0, name
        ctx.lib.results[symbol] = {ref: 2}
        values, mask, count = call(ctx)
        assert one_call(ctx) == want, name
        assert is_host(values, dtype, n) and is_host(mask, np.uint8, nb(n)) and count == 2, name
        out, out_mask = np.zeros(n + 2, dtype), np.zeros(nb(n) + 2, np.uint8)
        values, mask, count = call(ctx, out=out, out_mask=out_mask, out_device=True)
        # (given buffers decide where the result goes; without a column, out_device still names the space of the call)
        assert one_call(ctx) == ((symbol, (H, L.MEM_DEVICE) + want[1][2:]) if col == N else want), name
        assert is_view(values, out, dtype, n) and is_view(mask, out_mask, np.uint8, nb(n)), name
        values, mask, _ = call(ctx, out=out)                                  # one of the two given: the other is made beside it
        assert one_call(ctx) == want and is_view(values, out, dtype, n) and is_host(mask, np.uint8, nb(n)), name
        values, mask, _ = call(ctx, out_mask=out_mask)
        assert one_call(ctx) == want and is_host(values, dtype, n) and is_view(mask, out_mask, np.uint8, nb(n)), name
        ctx.lib.results[symbol] = {ref: 0}
        assert call(ctx, out_mask=out_mask)[1] is None, name                  # no null: no mask, given or not
        one_call(ctx)


VALUE_PROGRAM = [(L.EVAL_COL, 0), (L.EVAL_CONST, 2.5), (L.EVAL_ADD, 0)]
BOOL_PROGRAM = [(L.EVAL_COL, 0), (L.EVAL_CONST, 2.5), (L.EVAL_GT, 0)]
CHECK_CALL = lambda program: ("pandrs_hip_eval_check", ([L.F64], 1, [op for op, _ in program], [float(a) for _, a in program], 3, 0, 0))  # noqa: E731


@pytest.mark.parametrize("n", ROWS)
def test_eval_value_program(ctx, n):
    ops, args = [op for op, _ in VALUE_PROGRAM], [0.0, 2.5, 0.0]
    want = ("pandrs_hip_eval", (H, HOST, COL, 1, n, ops, args, 3, HOST, P if n else N, P if n else N, 0))
    values, mask, count = ctx.eval([f64(n)], n, VALUE_PROGRAM)
    assert ctx.lib.calls[0] == CHECK_CALL(VALUE_PROGRAM)
    assert one_call(ctx, "pandrs_hip_eval") == want
    assert is_host(values, np.float64, n) and mask is None and count == 0
    ctx.lib.results["pandrs_hip_eval"] = {11: 1}
    out, out_mask = np.zeros(n + 2), np.zeros(nb(n) + 2, np.uint8)
    values, mask, count = ctx.eval([f64(n)], n, VALUE_PROGRAM, out=out, out_mask=out_mask)
    assert one_call(ctx, "pandrs_hip_eval") == want
    assert is_view(values, out, np.float64, n) and is_view(mask, out_mask, np.uint8, nb(n)) and count == 1


@pytest.mark.parametrize("n", ROWS)
def test_eval_boolean_program(ctx, n):
    ctx.lib.results["pandrs_hip_eval_check"] = {5: 1}                         # the validator says: a mask
    ctx.lib.results["pandrs_hip_eval"] = {11: n}
    ops, args = [op for op, _ in BOOL_PROGRAM], [0.0, 2.5, 0.0]
    want = ("pandrs_hip_eval", (H, HOST, COL, 1, n, ops, args, 3, HOST, P if n else N, N, 0))
    bits, count = ctx.eval([f64(n)], n, BOOL_PROGRAM)
    assert ctx.lib.calls[0] == CHECK_CALL(BOOL_PROGRAM)
    assert one_call(ctx, "pandrs_hip_eval") == want
    assert is_host(bits, np.uint8, nb(n)) and count == n
    out = np.zeros(nb(n) + 2, np.uint8)
    bits, _ = ctx.eval([f64(n)], n, BOOL_PROGRAM, out=out)
    assert one_call(ctx, "pandrs_hip_eval") == want and is_view(bits, out, np.uint8, nb(n))
    with pytest.raises(ValueError) as e:
        ctx.eval([f64(n)], n, BOOL_PROGRAM, out_mask=np.zeros(nb(n), np.uint8))
    assert str(e.value) == "a boolean program takes no out_mask"
    assert [c[0] for c in ctx.lib.calls] == ["pandrs_hip_eval_check"]         # the validator ran, the program did not


# ---- row masks: predicate, isin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_predicate(ctx, n):
    ctx.lib.results["pandrs_hip_predicate"] = {9: n}
    want = ("pandrs_hip_predicate", (H, HOST, COL, n, L.PRED_BETWEEN, 1.0, 4.5, HOST, P if n else N, 0))
    bits, count = ctx.predicate(f64(n), n, L.PRED_BETWEEN, 1, 4.5)
    assert one_call(ctx) == want and is_host(bits, np.uint8, nb(n)) and count == n
    out = np.zeros(nb(n) + 2, np.uint8)
    bits, _ = ctx.predicate(f64(n), n, L.PRED_BETWEEN, 1, 4.5, out=out, out_device=True)
    assert one_call(ctx) == want and is_view(bits, out, np.uint8, nb(n))
    bits, count = ctx.predicate(f64(n), n, L.PRED_ISNA, count_only=True, out_device=True)
    assert one_call(ctx) == ("pandrs_hip_predicate", (H, HOST, COL, n, L.PRED_ISNA, 0.0, 0.0, HOST, N, 0))
    assert bits is None and count == n
    with pytest.raises(ValueError) as e:
        ctx.predicate(f64(n), n, L.PRED_ISNA, out=out, count_only=True)
    assert str(e.value) == "count_only takes no out" and ctx.lib.calls == []


@pytest.mark.parametrize("n", ROWS)
def test_isin(ctx, n):
    values = (np.array([1, 5, 7], np.int64), None, L.I64)
    ctx.lib.results["pandrs_hip_isin"] = {10: 1}
    want = (H, HOST, COL_I, n, HOST, COL_I, 3, 0, HOST, P if n else N, 0)
    bits, count = ctx.isin(i64(n), n, values)
    assert one_call(ctx) == ("pandrs_hip_isin", want) and is_host(bits, np.uint8, nb(n)) and count == 1
    out = np.zeros(nb(n) + 2, np.uint8)
    bits, _ = ctx.isin(i64(n), n, values, negate=True, out=out)
    assert one_call(ctx) == ("pandrs_hip_isin", want[:7] + (1,) + want[8:]) and is_view(bits, out, np.uint8, nb(n))
    bits, count = ctx.isin(i64(n), n, values, count_only=True)
    assert one_call(ctx) == ("pandrs_hip_isin", want[:9] + (N, 0)) and bits is None and count == 1
    with pytest.raises(ValueError) as e:
        ctx.isin(i64(n), n, values, out=out, count_only=True)
    assert str(e.value) == "count_only takes no out" and ctx.lib.calls == []


# ---- bin: codes and counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_bin(ctx, n):
    edges = [0.0, 2.0, 4.0, 100.0]
    head = (H, HOST, COL, n, P, 3, HOST)
    codes, counts = ctx.bin(f64(n), n, edges)
    assert one_call(ctx) == ("pandrs_hip_bin", head + (P if n else N, P))
    assert is_host(codes, np.int32, n) and is_host(counts, np.int64, 5)
    out = np.zeros(n + 2, np.int32)
    codes, counts = ctx.bin(f64(n), n, edges, out=out, want_counts=False, out_device=True)
    assert one_call(ctx) == ("pandrs_hip_bin", head + (P, N) if n else head + (N, P))     # no rows: the counts stand in
    assert is_view(codes, out, np.int32, n) and counts is None
    codes, counts = ctx.bin(f64(n), n, edges, want_codes=False, out_device=True)
    assert one_call(ctx) == ("pandrs_hip_bin", head + (N, P))
    assert codes is None and is_host(counts, np.int64, 5)
    with pytest.raises(ValueError) as e:
        ctx.bin(f64(n), n, edges, out=out, want_codes=False)
    assert str(e.value) == "want_codes=False takes no out" and ctx.lib.calls == []
    with pytest.raises(ValueError) as e:
        ctx.bin(f64(n), n, edges, want_codes=False, want_counts=False)
    assert str(e.value) == "bin: neither codes nor counts asked for" and ctx.lib.calls == []


# ---- windows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_window(ctx, n):
    got = ctx.window(f64(n), n, L.WINDOW_KIND_ROLLING, L.WINDOW_MEAN, window=3, min_periods=2, center=True, ddof=0, alpha=0.25)
    spec = (L.WINDOW_KIND_ROLLING, L.WINDOW_MEAN, 3, 2, 1, 0, 0, 0.25)
    assert one_call(ctx) == ("pandrs_hip_window", (H, HOST, COL, n, spec, HOST, P if n else N))
    assert is_host(got, np.float64, n)
    got = ctx.window(i64(n), n, L.WINDOW_KIND_EXPANDING, L.WINDOW_SUM, out_device=False)
    assert one_call(ctx) == ("pandrs_hip_window", (H, HOST, COL_I, n, (L.WINDOW_KIND_EXPANDING, L.WINDOW_SUM, 0, -1, 0, 0, 1, 0.0), HOST,
                                                   P if n else N))
    assert is_host(got, np.float64, n)


@pytest.mark.parametrize("n", ROWS)
def test_window_quantile(ctx, n):
    got = ctx.window_quantile(f64(n), n, L.WINDOW_KIND_ROLLING, median=False, q=0.25, window=4, min_periods=1, nan_missing=True)
    spec = (L.WINDOW_KIND_ROLLING, 0, 4, 1, 0, 1, 0.25)
    assert one_call(ctx) == ("pandrs_hip_window_quantile", (H, HOST, COL, n, spec, HOST, P if n else N))
    assert is_host(got, np.float64, n)
    got = ctx.window_quantile(f64(n), n, L.WINDOW_KIND_EXPANDING, center=True, out_device=False)
    assert one_call(ctx) == ("pandrs_hip_window_quantile", (H, HOST, COL, n, (L.WINDOW_KIND_EXPANDING, 1, 0, -1, 1, 0, 0.5), HOST,
                                                            P if n else N))
    assert is_host(got, np.float64, n)


# ---- gathers through a retained selection / retained pairs ------------------------------------------------------------------
FILL_CASES = [0, -1, 2**63 - 1, 1.5, -0.0, float("nan")]


def old_fill_bits(fill, dtype):
    """The expression join_gather and filter_gather each spelled out."""
    return int(np.float64(fill).view(np.uint64)) if dtype == L.F64 else int(fill) & 0xFFFFFFFFFFFFFFFF


DTYPES = [(L.I64, np.int64), (L.F64, np.float64), (L.U32CODE, np.uint32), (L.BOOLBITS, np.uint8)]


@pytest.mark.parametrize("n", ROWS)
def test_filter_gather(ctx, n):
    for dt, npdt in DTYPES:
        col = (np.zeros(12, npdt), np.zeros(2, np.uint8), dt)
        got = ctx.filter_gather(col, 12, n, fill=3)
        bits = 0x4008000000000000 if dt == L.F64 else 3
        assert one_call(ctx) == ("pandrs_hip_filter_gather", (H, HOST, [(False, False, dt)], 12, bits, HOST, P if n else N))
        assert is_host(got, npdt, n)
    got = ctx.filter_gather((np.zeros(12, np.uint64), None, L.CELL64), 12, n)   # any other dtype comes back as int64
    assert one_call(ctx)[1][2] == [(False, True, L.CELL64)] and is_host(got, np.int64, n)
    for fill in FILL_CASES:
        for dt in (L.F64, L.I64):
            if dt == L.I64 and not isinstance(fill, int):
                continue
            ctx.filter_gather((np.zeros(12, np.float64 if dt == L.F64 else np.int64), None, dt), 12, n, fill=fill)
            assert one_call(ctx)[1][4] == old_fill_bits(fill, dt), (fill, dt)


@pytest.mark.parametrize("n", ROWS)
def test_join_gather(ctx, n):
    for dt, npdt in DTYPES:
        col = (np.zeros(12, npdt), None, dt)
        got = ctx.join_gather(col, 12, n, 1, fill=3)
        bits = 0x4008000000000000 if dt == L.F64 else 3
        assert one_call(ctx) == ("pandrs_hip_join_gather", (H, HOST, [(False, True, dt)], 12, 1, bits, HOST, P))   # a pointer at 0 rows too
        assert is_host(got, npdt, n)
    got = ctx.join_gather(i64(12), 12, n, 0, fill=-1, key_right=i64(5), n_right=5)
    assert one_call(ctx) == ("pandrs_hip_join_gather_key", (H, HOST, COL_I, 12, COL_I, 5, 0xFFFFFFFFFFFFFFFF, HOST, P))
    assert is_host(got, np.int64, n)
    with pytest.raises(KeyError):
        ctx.join_gather((np.zeros(12, np.uint64), None, L.CELL64), 12, n, 0)
    assert ctx.lib.calls == []
    for fill in FILL_CASES:
        for dt in (L.F64, L.I64):
            if dt == L.I64 and not isinstance(fill, int):
                continue
            ctx.join_gather((np.zeros(12, np.float64 if dt == L.F64 else np.int64), None, dt), 12, n, 0, fill=fill)
            assert one_call(ctx)[1][5] == old_fill_bits(fill, dt), (fill, dt)


# ---- fetches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_key_hash_cells(ctx, n):
    got = ctx.key_hash_cells([i64(n), f64(n)], n)
    assert one_call(ctx) == ("pandrs_hip_key_hash_cells", (H, HOST, COL_I + COL, 2, n, P))     # a pointer at 0 rows too
    assert is_host(got, np.uint64, n)


@pytest.mark.parametrize("n", ROWS)
def test_distinct_fetch(ctx, n):
    p = P if n else N
    v, f, k = ctx.distinct_fetch(n)
    assert one_call(ctx) == ("pandrs_hip_distinct_fetch", (H, HOST, p, p, p))
    assert is_host(v, np.uint64, n) and is_host(f, np.uint8, n) and is_host(k, np.int64, n)
    v, f, k = ctx.distinct_fetch(n, values=False, counts=False)
    assert one_call(ctx) == ("pandrs_hip_distinct_fetch", (H, HOST, N, p, N))
    assert v is None and is_host(f, np.uint8, n) and k is None


@pytest.mark.parametrize("n", ROWS)
def test_join_indices(ctx, n):
    ctx.lib.results["pandrs_hip_join_indices"] = {7: n}
    li, ri = ctx.join_indices(i64(9), 9, i64(4), 4, L.LEFT)
    assert ctx.waits == 0
    assert ctx.lib.calls == [("pandrs_hip_join_indices", (H, HOST, COL_I, 9, COL_I, 4, L.LEFT, 0)),
                             ("pandrs_hip_join_fetch", (H, HOST, P, P))]                   # a pointer for 0 pairs too
    assert is_host(li, np.int64, n) and is_host(ri, np.int64, n)


@pytest.mark.parametrize("n", ROWS)
def test_distinct_stages_a_host_rank_table(ctx, n):
    ctx.lib.results["pandrs_hip_distinct"] = {}
    codes = (np.zeros(n, np.uint32), None, L.U32CODE)
    ctx.distinct(codes, n, L.DISTINCT_BY_VALUE, code_rank=np.array([2, 0, 1], np.uint32))
    assert ctx.lib.calls[0] == ("pandrs_hip_distinct", (H, HOST, [(False, True, L.U32CODE)], n, L.DISTINCT_BY_VALUE, P, 3, (0,) * 8))
    ctx.lib.calls.clear()
    ctx.distinct(codes, n, L.DISTINCT_BY_COUNT)
    assert ctx.lib.calls[0] == ("pandrs_hip_distinct", (H, HOST, [(False, True, L.U32CODE)], n, L.DISTINCT_BY_COUNT, N, 0, (0,) * 8))
    assert ctx.lib.calls[1] == ("pandrs_hip_distinct_fetch", (H, HOST, N, N, N))           # no entry recorded: host, no pointers


# ---- every ValueError of a caller's buffer, and that nothing was called -------------------------------------------------------
def raises(ctx, text, call):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text
    assert [c[0] for c in ctx.lib.calls if c[0] != "pandrs_hip_eval_check"] == [] and ctx.waits == 0
    ctx.lib.calls.clear()


def bad_buffers(dtype, count):
    """Buffers a call for `count` cells of `dtype` must refuse (count >= 1)."""
    import torch
    other = np.float32 if dtype != np.float32 else np.float64
    cpu_tensor = torch.zeros(count + 2, dtype={np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32,
                                               np.uint8: torch.uint8}[dtype])
    return {"wrong dtype": np.zeros(count + 2, other), "not contiguous": np.zeros(2 * count + 4, dtype)[::2],
            "one short": np.zeros(count - 1, dtype), "a list": [0] * (count + 2), "a CPU tensor": cpu_tensor}


OUT_TEXT = "out must be a contiguous %s numpy array or CUDA tensor of at least %s elements"
MASK_TEXT = "out_mask must be a contiguous uint8 numpy array or CUDA tensor of at least ceil(n_rows / 8) elements"
BOTH_TEXT = "out and out_mask must both be numpy arrays or both CUDA tensors"


def test_refused_out_buffers(ctx):
    n = 9
    ctx.lib.results["pandrs_hip_eval_check"] = {5: 1}
    single = [
        (np.float64, n, OUT_TEXT % ("float64", "n_rows"), lambda out: ctx.rank(f64(n), n, L.RANK_MIN, out=out)),
        (np.int64, 4, OUT_TEXT % ("int64", "min(k, n_rows)"), lambda out: ctx.topk(f64(n), n, 4, out=out)),
        (np.int64, n, OUT_TEXT % ("int64", "min(k, n_rows)"), lambda out: ctx.topk(f64(n), n, 50, out=out)),
        (np.uint8, 2, OUT_TEXT % ("uint8", "ceil(n_rows / 8)"), lambda out: ctx.predicate(f64(n), n, L.PRED_GT, 1.0, out=out)),
        (np.uint8, 2, OUT_TEXT % ("uint8", "ceil(n_rows / 8)"), lambda out: ctx.isin(f64(n), n, (np.zeros(2), None, L.F64), out=out)),
        (np.uint8, 2, OUT_TEXT % ("uint8", "ceil(n_rows / 8)"), lambda out: ctx.eval([f64(n)], n, BOOL_PROGRAM, out=out)),
        (np.int32, n, OUT_TEXT % ("int32", "n_rows"), lambda out: ctx.bin(f64(n), n, [0.0, 1.0], out=out)),
    ]
    for dtype, count, text, call in single:
        for name, bad in bad_buffers(dtype, count).items():
            raises(ctx, text, lambda: call(bad))


def test_refused_cell_buffers(ctx):
    import torch
    n = 9
    for name, symbol, call, _, _, dtype, _ in cell_cases(n) + [
            ("eval", "pandrs_hip_eval", lambda c, **kw: c.eval([f64(n)], n, VALUE_PROGRAM, **kw), None, None, np.float64, None)]:
        text = OUT_TEXT % (np.dtype(dtype).name, "n_rows")
        for kind, bad in bad_buffers(dtype, n).items():
            raises(ctx, text, lambda: call(ctx, out=bad))
            if kind != "a CPU tensor":
                raises(ctx, text, lambda: call(ctx, out=bad, out_mask=np.zeros(2, np.uint8)))
        for kind, bad in bad_buffers(np.uint8, 2).items():
            raises(ctx, MASK_TEXT, lambda: call(ctx, out_mask=bad))
            if kind != "a CPU tensor":
                raises(ctx, MASK_TEXT, lambda: call(ctx, out=np.zeros(n, dtype), out_mask=bad))
        # one of each kind: refused before any dtype is looked at
        raises(ctx, BOTH_TEXT, lambda: call(ctx, out=np.zeros(n, np.float32), out_mask=torch.zeros(2, dtype=torch.uint8)))
        raises(ctx, BOTH_TEXT, lambda: call(ctx, out=torch.zeros(n, dtype=torch.float32), out_mask=np.zeros(2, np.uint8)))


def test_fill_checks_its_value_before_any_buffer(ctx):
    n = 9
    bad_out = np.zeros(n, np.float32)
    for method in (L.FILL_FFILL, L.FILL_BFILL, L.FILL_LINEAR):
        raises(ctx, "value goes with FILL_VALUE only", lambda: ctx.fill(f64(n), n, method, 1.0))
        raises(ctx, "value goes with FILL_VALUE only", lambda: ctx.fill(f64(n), n, method, 0, out=bad_out))
    raises(ctx, "an I64 column is filled with an int that fits int64, got 1.5", lambda: ctx.fill(i64(n), n, L.FILL_VALUE, 1.5, out=bad_out))
    raises(ctx, "an I64 column is filled with an int that fits int64, got %d" % 2**63, lambda: ctx.fill(i64(n), n, L.FILL_VALUE, 2**63))
    raises(ctx, "an I64 column is filled with an int that fits int64, got True", lambda: ctx.fill(i64(n), n, L.FILL_VALUE, True))
    raises(ctx, "an F64 column is filled with a float, got None", lambda: ctx.fill(f64(n), n, L.FILL_VALUE, out=bad_out))
    raises(ctx, "an F64 column is filled with a float, got 'x'", lambda: ctx.fill(f64(n), n, L.FILL_VALUE, "x"))


# ---- the small helpers ----------------------------------------------------------------------------------------------------------
def test_fill_bits_helper():
    for fill in FILL_CASES:
        assert E._fill_bits(fill, L.F64) == old_fill_bits(fill, L.F64)
        for dt in (L.I64, L.U32CODE, L.BOOLBITS):
            if isinstance(fill, int):
                assert E._fill_bits(fill, dt) == old_fill_bits(fill, dt)
    assert E._fill_bits(-1, L.I64) == 0xFFFFFFFFFFFFFFFF and E._fill_bits(-0.0, L.F64) == 1 << 63
    assert E._fill_bits(float("nan"), L.F64) == 0x7FF8000000000000 and E._fill_bits(1.5, L.F64) == 0x3FF8000000000000
    assert E._space(True) == E._space(1) == L.MEM_DEVICE and E._space(False) == E._space(None) == L.MEM_HOST


def test_code_rank_helper_on_the_host(ctx):
    keep = []
    assert ctx._code_rank(None, L.MEM_HOST, keep) == (None, 0) and keep == []
    table = np.array([3, 0, 2, 1], np.int32)
    rank, n_codes = ctx._code_rank(table, L.MEM_HOST, keep)
    assert rank.dtype == np.uint32 and n_codes == 4 and np.shares_memory(rank, table) and list(rank) == [3, 0, 2, 1]
    assert len(keep) == 1 and keep[0] is rank and ctx.waits == 0
    rank, n_codes = ctx._code_rank(np.array([5, 6], np.uint32)[::-1], L.MEM_HOST, keep)      # not contiguous: a copy, kept alive
    assert rank.flags.c_contiguous and list(rank) == [6, 5] and n_codes == 2 and keep[1] is rank


def test_empty_on_the_host_is_exact_and_needs_no_torch(ctx):
    for shape, dtype in (((0,), np.uint64), ((3, 4), np.float64), (5, np.int32)):
        a = ctx._empty(shape, dtype, False)
        assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (shape if isinstance(shape, tuple) else (shape,))
    assert set(E._TORCH_OF) >= {np.int64, np.uint64, np.float64, np.int32, np.uint32, np.uint8}
    assert E._TORCH_OF[np.uint64] == E._TORCH_OF[np.int64] and E._TORCH_OF[np.uint32] == E._TORCH_OF[np.int32]


# ---- the same conventions through the library ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_buffers_through_the_library():
    """Per op and row count: a device column without out, a given CUDA out (and out_mask) two elements longer than needed, a
    host column with out_device=True - each a CUDA tensor of the right dtype and shape on the context's device, the given
    buffer itself where one was given, and bit for bit the host call's result, which in turn is the numpy reference's."""
    import torch

    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    from tests import bin_ref, cumulative_ref, fill_ref, predicate_ref, rank_ref, topk_ref

    TORCH = {np.float64: torch.float64, np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}
    dev = torch.device("cuda", 0)
    real = pa.Context(0)

    def device_ok(t, dtype, count, into=None):
        assert torch.is_tensor(t) and t.device == dev and t.dtype == TORCH[dtype] and tuple(t.shape) == (count,), (t, dtype, count)
        if into is not None:                                                  # (torch reports data_ptr() 0 for an empty view)
            assert t.data_ptr() == (into.data_ptr() if count else 0)
            assert t.untyped_storage().data_ptr() == into.untyped_storage().data_ptr() and t.storage_offset() == 0

    def same(t, want):
        want = np.ascontiguousarray(want)
        got = t.cpu().numpy() if torch.is_tensor(t) else t
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)

    def to_device(col):
        data, mask, dt = col
        return (torch.from_numpy(data).to(dev), torch.from_numpy(mask).to(dev), dt)

    def buf(dtype, count):
        return torch.full((count + 2,), 7, dtype=TORCH[dtype], device=dev)

    try:
        for n in ROWS:
            x = np.array([np.nan, 3.0, 1.0, 3.0, -2.0, 8.0, np.nan, 0.5, 3.0])[:n]
            nulls = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0], bool)[:n]
            col = (x, np.packbits(nulls, bitorder="little"), L.F64)
            dcol = to_device(col)

            # rank
            want = rank_ref.rank_ref(x, nulls, rank_ref.AVERAGE)
            host = real.rank(col, n, L.RANK_AVERAGE)
            same(host, want)
            out = buf(np.float64, n)
            for got, into in ((real.rank(dcol, n, L.RANK_AVERAGE), None), (real.rank(dcol, n, L.RANK_AVERAGE, out=out), out),
                              (real.rank(col, n, L.RANK_AVERAGE, out_device=True), None)):
                device_ok(got, np.float64, n, into)
                same(got, host)
            assert out[n:].tolist() == [7.0, 7.0]

            # topk
            k = 4
            want_rows, want_numbers = topk_ref.topk_ref(x, nulls, k, True)
            host, numbers = real.topk(col, n, k)
            same(host, want_rows)
            assert numbers == want_numbers
            out = buf(np.int64, min(k, n))
            for (got, m), into in ((real.topk(dcol, n, k), None), (real.topk(dcol, n, k, out=out), out),
                                   (real.topk(col, n, k, out_device=True), None)):
                device_ok(got, np.int64, min(k, n), into)
                same(got, host)
                assert m == numbers
            assert out[min(k, n):].tolist() == [7, 7]

            # fill and cumulative: a cell per row and the bitmap of the rows still null
            want_fill, gone = fill_ref.fill_twin(x, nulls, fill_ref.FFILL)
            want_cum, cum_null = cumulative_ref.cum_twin(x, nulls, cumulative_ref.MAX)
            for call, want, want_null in ((lambda c, **kw: real.fill(c, n, L.FILL_FFILL, **kw), want_fill, gone),
                                          (lambda c, **kw: real.cumulative(c, n, L.CUM_MAX, **kw), want_cum, cum_null)):
                hv, hm, hc = call(col)
                same(hv, want)
                assert hc == int(want_null.sum())
                if hc:
                    same(hm, np.packbits(want_null, bitorder="little"))
                else:
                    assert hm is None
                out, out_mask = buf(np.float64, n), buf(np.uint8, nb(n))
                for (gv, gm, gc), into, into_mask in ((call(dcol), None, None), (call(dcol, out=out, out_mask=out_mask), out, out_mask),
                                                      (call(col, out_device=True), None, None)):
                    device_ok(gv, np.float64, n, into)
                    same(gv, hv)
                    assert gc == hc
                    if hc:
                        device_ok(gm, np.uint8, nb(n), into_mask)
                        same(gm, hm)
                    else:
                        assert gm is None
                assert out[n:].tolist() == [7.0, 7.0] and out_mask[nb(n):].tolist() == [7, 7]

            # predicate
            want_bits, want_count = predicate_ref.predicate(x, col[1], predicate_ref.GE, 1.0)
            host, count = real.predicate(col, n, L.PRED_GE, 1.0)
            same(host, want_bits)
            assert count == want_count
            out = buf(np.uint8, nb(n))
            for (got, m), into in ((real.predicate(dcol, n, L.PRED_GE, 1.0), None), (real.predicate(dcol, n, L.PRED_GE, 1.0, out=out), out),
                                   (real.predicate(col, n, L.PRED_GE, 1.0, out_device=True), None)):
                device_ok(got, np.uint8, nb(n), into)
                same(got, host)
                assert m == count
            assert out[nb(n):].tolist() == [7, 7]

            # bin
            edges = [-5.0, 0.75, 3.0, 3.0, 9.0]
            want_codes, want_counts = bin_ref.codes(np.where(nulls, np.nan, x), edges)
            host, counts = real.bin(col, n, edges)
            same(host, want_codes)
            same(counts, want_counts)
            out = buf(np.int32, n)
            for (got, c), into in ((real.bin(dcol, n, edges), None), (real.bin(dcol, n, edges, out=out), out),
                                   (real.bin(col, n, edges, out_device=True), None)):
                device_ok(got, np.int32, n, into)
                same(got, host)
                same(c, counts)
            assert out[n:].tolist() == [7, 7]
    finally:
        real.close()
