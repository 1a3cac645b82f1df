"""Vectorised numpy restatements of pandrs_hip_predicate and pandrs_hip_isin (include/pandrs_hip.h; the reference's
PandasCompatExt::gt / ge / lt / le / eq_value / ne_value, src/dataframe/pandas_compat/helpers/comparison_ops.rs:7-46, between /
is_between, functions.rs:253-257, :4141-4161, isna / notna / is_finite / is_infinite, :930-933, :1312-1315, :4016-4024, isin_numeric,
:150-158).  Every function returns (bits, count): the LSB-first uint8 bitmap of ceil(n / 8) bytes, bit = 1 the row is selected, and
the number of set bits.  tests/test_predicate_ref.py checks them against a per-row Python twin of the reference's expressions."""
import numpy as np

GT, GE, LT, LE, EQ, NE, BETWEEN, BETWEEN_EXCLUSIVE, ISNA, NOTNA, IS_FINITE, IS_INFINITE = range(12)
OPS = list(range(12))
OP_NAMES = ["gt", "ge", "lt", "le", "eq", "ne", "between", "between_exclusive", "isna", "notna", "is_finite", "is_infinite"]
EPSILON = float(np.finfo(np.float64).eps)          # f64::EPSILON = DBL_EPSILON = 2^-52
I64, F64, U32CODE = 0, 1, 2
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def unpack_nulls(null_mask, n):
    """LSB-first null bitmap (or None) -> bool array of n rows."""
    if null_mask is None:
        return np.zeros(n, bool)
    return np.unpackbits(np.asarray(null_mask, np.uint8), count=n, bitorder="little").astype(bool)


def pack(sel):
    sel = np.asarray(sel, bool)
    return np.packbits(sel, bitorder="little"), int(sel.sum())


def as_f64(data, null_mask=None):
    """The column as the reference's get_column_numeric_values sees it: `v as f64` for int64 (numpy's astype rounds to nearest
    even as Rust does), the cells themselves for float64; a null cell is NaN (the header's deviation)."""
    data = np.asarray(data)
    v = data.astype(np.float64) if data.dtype == np.int64 else data.view(np.float64).copy()
    v[unpack_nulls(null_mask, v.shape[0])] = np.nan
    return v


def predicate(data, null_mask, op, a=0.0, b=0.0):
    v = as_f64(data, null_mask)
    a, b = np.float64(a), np.float64(b)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore"):
        if op == GT:
            sel = ~nan & (v > a)
        elif op == GE:
            sel = ~nan & (v >= a)
        elif op == LT:
            sel = ~nan & (v < a)
        elif op == LE:
            sel = ~nan & (v <= a)
        elif op == EQ:
            sel = ~nan & (np.abs(v - a) < EPSILON)
        elif op == NE:
            sel = nan | (np.abs(v - a) >= EPSILON)
        elif op == BETWEEN:
            sel = (v >= a) & (v <= b)
        elif op == BETWEEN_EXCLUSIVE:
            sel = ~nan & (v > a) & (v < b)
        elif op == ISNA:
            sel = nan
        elif op == NOTNA:
            sel = ~nan
        elif op == IS_FINITE:
            sel = np.isfinite(v)
        elif op == IS_INFINITE:
            sel = np.isinf(v)
        else:
            raise ValueError("op %r" % (op,))
    return pack(sel)


def keys(data, dtype, values_dtype):
    """The 64-bit key of every cell for a column of `dtype` tested against a list of `values_dtype`."""
    data = np.asarray(data)
    if dtype == U32CODE:
        return data.astype(np.uint32).astype(np.uint64)
    if dtype == I64 and values_dtype == F64:
        return data.astype(np.int64).astype(np.float64).view(np.uint64)
    return data.view(np.uint64)


def isin(data, null_mask, dtype, values, values_dtype, negate=False):
    ok = (dtype, values_dtype) in ((F64, F64), (I64, F64), (I64, I64), (U32CODE, U32CODE))
    if not ok:
        raise TypeError("pairing %r / %r" % (dtype, values_dtype))
    k = keys(data, dtype, values_dtype)
    vals = np.asarray(values)
    vk = vals.astype(np.uint32).astype(np.uint64) if values_dtype == U32CODE else vals.view(np.uint64)
    hit = np.isin(k, np.unique(vk)) & ~unpack_nulls(null_mask, k.shape[0])
    return pack(hit != bool(negate))
