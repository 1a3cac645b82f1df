"""tests/predicate_ref.py against a naive per-row twin - the reference's expressions written out one row at a time, with
struct.pack for to_bits() - and against the known answers of the reference's own tests
(src/dataframe/pandas_compat/functions.rs:4362-4367, :4405-4410, :5007-5008, :8121-8131, :8143-8147, :8206, :8348-8352,
:8483-8485, :8520-8524, :8632-8633), carried over as literals.  No GPU."""
import math
import struct

import numpy as np
import pytest

from tests import predicate_ref as R

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000123))[0]         # another payload, sign set
ALL_ONES = struct.unpack("<d", struct.pack("<Q", 0xFFFFFFFFFFFFFFFF))[0]      # the set's empty marker is a NaN too
EPS = 2.0 ** -52


def to_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def f64_specials():
    return np.array([NAN_A, NAN_B, ALL_ONES, math.inf, -math.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, 1.0 + EPS,
                     1.0 - EPS / 2, 2.0, 3.0, -1.0, 1e308, -1e308, 2.0 ** 53, 2.0 ** 53 + 2], np.float64)


def i64_specials():
    return np.array([0, 1, -1, 2, 3, 2 ** 53, 2 ** 53 + 1, -2 ** 53, -(2 ** 53 + 1), 2 ** 53 + 2, I64_MIN, I64_MAX, I64_MAX - 1, 7], np.int64)


def null_patterns(n):
    rng = np.random.default_rng(n)
    yield None
    yield rng.random(n) < 0.1
    yield np.ones(n, bool)


def cell_f64(x, i, nulls):
    """Row i as get_column_numeric_values gives it; a null cell is NaN."""
    if nulls is not None and nulls[i]:
        return math.nan
    return float(int(x[i])) if x.dtype == np.int64 else float(x[i])          # Python's int -> float rounds to nearest even


def twin_predicate(x, nulls, op, a, b):
    out = []
    for i in range(x.shape[0]):
        v = cell_f64(x, i, nulls)
        nan = v != v
        if op == R.GT:
            r = (not nan) and v > a
        elif op == R.GE:
            r = (not nan) and v >= a
        elif op == R.LT:
            r = (not nan) and v < a
        elif op == R.LE:
            r = (not nan) and v <= a
        elif op == R.EQ:
            r = (not nan) and abs(v - a) < EPS
        elif op == R.NE:
            r = nan or abs(v - a) >= EPS
        elif op == R.BETWEEN:
            r = v >= a and v <= b
        elif op == R.BETWEEN_EXCLUSIVE:
            r = False if nan else (v > a and v < b)
        elif op == R.ISNA:
            r = nan
        elif op == R.NOTNA:
            r = not nan
        elif op == R.IS_FINITE:
            r = math.isfinite(v)
        else:
            r = math.isinf(v)
        out.append(bool(r))
    return out


def twin_isin(x, nulls, dtype, values, values_dtype, negate):
    def key_of(v, as_f64):
        if dtype == R.U32CODE or (values_dtype == R.I64):
            return int(v) & 0xFFFFFFFFFFFFFFFF
        return to_bits(float(int(v)) if as_f64 else float(v))
    if values_dtype == R.F64:
        listed = {to_bits(float(v)) for v in values}
    else:
        listed = {int(v) & 0xFFFFFFFFFFFFFFFF for v in values}
    out = []
    for i in range(x.shape[0]):
        null = nulls is not None and nulls[i]
        hit = (not null) and key_of(x[i], dtype == R.I64) in listed
        out.append(hit != negate)
    return out


def as_bits(sel):
    return np.packbits(np.asarray(sel, bool), bitorder="little")


ARGS = [(0.0, 0.0), (1.0, 3.0), (3.0, 1.0), (math.inf, math.inf), (-math.inf, math.inf), (math.nan, 1.0), (1.0, math.nan),
        (2.0 ** 53, 2.0 ** 53 + 2), (9.223372036854775807e18, -9.223372036854775808e18), (5e-324, 1.0)]


@pytest.mark.parametrize("op", R.OPS, ids=R.OP_NAMES)
def test_predicates_equal_the_twin(op):
    for x in (f64_specials(), i64_specials(), np.tile(f64_specials(), 4)[:67], np.array([], np.float64), np.array([5], np.int64)):
        n = x.shape[0]
        for nulls in null_patterns(n):
            mask = None if nulls is None else as_bits(nulls)
            for a, b in ARGS:
                bits, count = R.predicate(x, mask, op, a, b)
                want = twin_predicate(x, nulls, op, a, b)
                assert bits.shape[0] == (n + 7) // 8 and count == sum(want)
                assert np.array_equal(bits, as_bits(want)), (R.OP_NAMES[op], x.dtype, a, b)


def test_eq_and_ne_at_the_edges():
    inf = np.array([math.inf, -math.inf, 1.0])
    for a in (math.inf, -math.inf):                                            # inf - inf is NaN: neither equal nor unequal
        row = 0 if a > 0 else 1
        eq = np.unpackbits(R.predicate(inf, None, R.EQ, a)[0], count=3, bitorder="little")
        ne = np.unpackbits(R.predicate(inf, None, R.NE, a)[0], count=3, bitorder="little")
        assert eq[row] == 0 and ne[row] == 0 and ne[1 - row] == 1 and ne[2] == 1 and eq.sum() == 0
    big = np.array([2 ** 53 + 1, 2 ** 53, 2 ** 53 + 2], np.int64)               # 2^53 + 1 rounds to 2^53 as f64
    assert R.predicate(big, None, R.EQ, 2.0 ** 53)[1] == 2
    assert R.predicate(np.arange(10.0), None, R.BETWEEN, 7.0, 2.0)[1] == 0     # a > b selects nothing


def test_isin_equals_the_twin():
    f, i = f64_specials(), i64_specials()
    codes = np.array([0, 1, 2, 3, 0xFFFFFFFF, 7, 1], np.uint32)
    cases = [
        (f, R.F64, np.array([0.0, NAN_B, ALL_ONES, 3.0, 3.0, 5e-324]), R.F64),
        (f, R.F64, np.array([-0.0, NAN_A]), R.F64),
        (f, R.F64, np.array([], np.float64), R.F64),
        (f, R.F64, f.copy(), R.F64),
        (i, R.I64, np.array([2.0 ** 53, -1.0, 9.223372036854775807e18, 0.5]), R.F64),
        (i, R.I64, np.array([2 ** 53 + 1, I64_MIN, -1, 7, 7], np.int64), R.I64),
        (i, R.I64, np.array([], np.int64), R.I64),
        (codes, R.U32CODE, np.array([1, 0xFFFFFFFF, 9], np.uint32), R.U32CODE),
    ]
    for x, dt, vals, vdt in cases:
        n = x.shape[0]
        for nulls in null_patterns(n):
            mask = None if nulls is None else as_bits(nulls)
            for negate in (False, True):
                bits, count = R.isin(x, mask, dt, vals, vdt, negate)
                want = twin_isin(x, nulls, dt, vals, vdt, negate)
                assert count == sum(want) and np.array_equal(bits, as_bits(want)), (dt, vdt, negate)
    # -0.0 is not 0.0; a NaN matches its own payload only; all ones is a key like any other
    sel = np.unpackbits(R.isin(f, None, R.F64, np.array([-0.0, NAN_A]), R.F64)[0], count=f.shape[0], bitorder="little").astype(bool)
    assert list(np.flatnonzero(sel)) == [0, 6]
    for dt, vdt in ((R.F64, R.I64), (R.U32CODE, R.F64), (R.I64, R.U32CODE), (R.F64, R.U32CODE), (R.U32CODE, R.I64)):
        with pytest.raises(TypeError):
            R.isin(f, None, dt, f, vdt)


def test_known_answers_of_the_reference():
    def sel(bits_count, n=5):
        return np.unpackbits(bits_count[0], count=n, bitorder="little").astype(bool).tolist()
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert sel(R.predicate(a, None, R.BETWEEN, 2.0, 4.0)) == [False, True, True, True, False]            # functions.rs:4405-4410
    assert sel(R.predicate(a, None, R.GT, 3.0)) == [False, False, False, True, True]                     # :8121-8122
    assert sel(R.predicate(a, None, R.GE, 3.0)) == [False, False, True, True, True]                      # :8124-8125
    assert sel(R.predicate(a, None, R.LT, 3.0)) == [True, True, False, False, False]                     # :8127-8128
    assert sel(R.predicate(a, None, R.LE, 3.0)) == [True, True, True, False, False]                      # :8130-8131
    assert sel(R.predicate(a, None, R.BETWEEN_EXCLUSIVE, 2.0, 4.0)) == [False, False, True, False, False]   # :8523-8524
    assert R.predicate(a, None, R.GT, 3.0)[1] == 2                                                       # query_gt, :7264-7265
    e = np.array([1.0, 2.0, 3.0, 2.0, 1.0])
    assert sel(R.predicate(e, None, R.EQ, 2.0)) == [False, True, False, True, False]                     # :8143-8144
    assert sel(R.predicate(e, None, R.NE, 2.0)) == [True, False, True, False, True]                      # :8146-8147
    na = np.array([1.0, math.nan, 3.0, math.nan, 5.0])
    assert sel(R.predicate(na, None, R.ISNA)) == [False, True, False, True, False]                       # :5007-5008
    assert R.predicate(na, None, R.NOTNA)[1] == 3                                                        # dropna, :4988-4989
    assert R.predicate(np.array([1.0, math.nan, 3.0, math.nan, math.nan]), None, R.ISNA)[1] == 3         # count_na, :8206
    fin = np.array([1.0, math.inf, -math.inf, math.nan])
    assert sel(R.predicate(fin, None, R.IS_FINITE), 4) == [True, False, False, False]                    # :8348-8349
    assert sel(R.predicate(fin, None, R.IS_INFINITE), 4) == [False, True, True, False]                   # :8351-8352
    cv = np.array([1.0, 2.0, 1.0, 3.0, 1.0])
    assert [R.predicate(cv, None, R.EQ, v)[1] for v in (1.0, 2.0, 5.0)] == [3, 1, 0]                     # count_value, :8483-8485
    assert R.predicate(np.array([1.0, math.nan, 3.0]), None, R.ISNA)[1] > 0                              # has_nulls, :8632
    assert R.predicate(np.array([1.0, 2.0, 3.0]), None, R.ISNA)[1] == 0                                  # :8633
    # isin("name", ["Alice", "Bob", "Unknown"]) over Alice .. Eve, as pool codes; "Unknown" has no code (:4362-4367)
    names = np.array([0, 1, 2, 3, 4], np.uint32)
    assert sel(R.isin(names, None, R.U32CODE, np.array([0, 1], np.uint32), R.U32CODE)) == [True, True, False, False, False]
