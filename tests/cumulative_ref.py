"""The reference for pandrs_hip_cumulative / pandrs_hip_lag and the mirrors' cumsum / cumprod / cummax / cummin / cumcount /
shift / diff / pct_change: two restatements of PandasCompatExt's row loops (reference
src/dataframe/pandas_compat/functions.rs:280-342, :514-541, :2081-2094), extended by the mask rule of include/pandrs_hip.h: a
row under a null bit is skipped by a fold (NaN with its bit set, the running value passes through; cumcount writes the running
count and sets no bit), and a lag with a null operand is NaN with its bit set.

  cum_loop / lag_loop   line for line after the reference, in plain Python floats (IEEE doubles, sequential)
  cum_twin / lag_twin   vectorised numpy: ufunc.accumulate is the same sequential fold

All -> (values, null_bits): values is float64 (int64 for COUNT), every NaN the canonical quiet NaN; null_bits is a bool array.
SUM and PROD of the device are compared through sum_bound / gamma; everything else on the uint64 view."""
import math

import numpy as np

SUM, PROD, MAX, MIN, COUNT = range(5)                           # pandrs_hip_cum_op
SHIFT, DIFF, PCT_CHANGE = range(3)                              # pandrs_hip_lag_op
CUM_OPS = [SUM, PROD, MAX, MIN, COUNT]
LAG_OPS = [SHIFT, DIFF, PCT_CHANGE]
CANON_NAN = np.uint64(0x7FF8000000000000)
NAN = CANON_NAN.view(np.float64)
U = 2.0 ** -53
TINY = 2.2250738585072014e-308                                  # the smallest normal f64


def bits(flags):
    """bool per row -> the little-endian null bitmap of ceil(n / 8) bytes"""
    return np.packbits(np.asarray(flags, bool), bitorder="little")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def canon(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = NAN
    return v


def _nulls(x, nulls):
    return np.zeros(np.asarray(x).shape[0], bool) if nulls is None else np.asarray(nulls, bool)


def as_f64(x):
    """get_column_numeric_values: an I64 cell `as f64`"""
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    return x.astype(np.float64)


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def sum_bound(x, nulls=None):
    """2 gamma_k sum_{j<=i} |x_j| per row, k the non-null rows in 0 .. i (pandrs_hip.h)"""
    v, nl = as_f64(x), _nulls(x, nulls)
    return 2.0 * gamma(np.cumsum(~nl)) * np.cumsum(np.where(nl, 0.0, np.abs(v)))


def compare_cells(op, got, want, x, nulls, exact):
    """One fold's cells against the twin's, by the contract of its op (pandrs_hip.h): MAX, MIN and COUNT bit for bit, as is a SUM
    the caller knows to be exact; SUM within sum_bound; PROD within 2 gamma_k where the twin's product is normal, the same
    sign, infinity and zero elsewhere.  The rule of tests/test_gpu_cumulative.py and of the randomised sweep."""
    if op in (MAX, MIN, COUNT) or (op == SUM and exact):
        assert same_bits(got, want), (op, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:5])
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (op, np.flatnonzero(np.isnan(got) != nan)[:5])
    k = np.cumsum(np.ones(len(want), bool) if nulls is None else ~np.asarray(nulls, bool))
    with np.errstate(all="ignore"):
        if op == SUM:
            fin = np.isfinite(want)
            err, bound = np.abs(got[fin] - want[fin]), sum_bound(x, nulls)[fin]
            assert np.all(err <= bound), (np.flatnonzero(err > bound)[:5], float(np.max(err / np.maximum(bound, TINY))))
            assert same_bits(got[~fin & ~nan], want[~fin & ~nan])
        else:
            normal = np.isfinite(want) & (np.abs(want) >= TINY)
            rel = np.abs(got[normal] / want[normal] - 1.0)
            assert np.all(rel <= 2 * gamma(k[normal])), (np.flatnonzero(rel > 2 * gamma(k[normal]))[:5], float(rel.max()))
            rest = ~normal & ~nan
            assert np.array_equal(np.signbit(got[rest]), np.signbit(want[rest])) and np.array_equal(np.isinf(got[rest]), np.isinf(want[rest]))
            zero = rest & (want == 0.0)
            assert np.all(got[zero] == 0.0)


# ---- f64::max / f64::min with the signed-zero convention of pandrs_hip_window: -0.0 below +0.0 --------------------------------
def rust_max(a, b):
    if a != a:
        return b
    if b != b:
        return a
    if a == b:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a > b else b


def rust_min(a, b):
    if a != a:
        return b
    if b != b:
        return a
    if a == b:
        return a if math.copysign(1.0, a) < 0 else b
    return a if a < b else b


def _order_key(v):
    """float64 -> int64 that orders as the IEEE total order on non-NaN values; its own inverse"""
    b = np.ascontiguousarray(v, np.float64).view(np.int64)
    return b ^ ((b >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


def cum_loop(x, nulls, op):
    v, nl = [float(t) for t in as_f64(x)], _nulls(x, nulls)
    n = len(v)
    out = np.empty(n, np.int64 if op == COUNT else np.float64)
    gone = np.zeros(n, bool)
    acc = {SUM: 0.0, PROD: 1.0, MAX: -math.inf, MIN: math.inf, COUNT: 0}[op]      # functions.rs:282, :294, :306, :318, :2083
    for i in range(n):
        if nl[i]:
            if op == COUNT:
                out[i] = acc
            else:
                out[i], gone[i] = NAN, True
            continue
        if op == SUM:
            acc += v[i]                                         # :286
        elif op == PROD:
            acc *= v[i]                                         # :298
        elif op == MAX:
            acc = rust_max(acc, v[i])                           # :310
        elif op == MIN:
            acc = rust_min(acc, v[i])                           # :322
        elif not math.isnan(v[i]):
            acc += 1                                            # :2087-2089
        out[i] = acc
    return (out if op == COUNT else canon(out)), gone


def cum_twin(x, nulls, op):
    v, nl = as_f64(x), _nulls(x, nulls)
    with np.errstate(all="ignore"):
        if op == COUNT:
            return np.cumsum(~(nl | np.isnan(v))).astype(np.int64), np.zeros(v.shape[0], bool)
        if op == SUM:
            out = np.add.accumulate(np.concatenate([[0.0], np.where(nl, -0.0, v)]))[1:]
        elif op == PROD:
            out = np.multiply.accumulate(np.concatenate([[1.0], np.where(nl, 1.0, v)]))[1:]
        else:
            start = -np.inf if op == MAX else np.inf
            keys = _order_key(np.where(nl | np.isnan(v), start, v))
            keys = (np.maximum if op == MAX else np.minimum).accumulate(keys)
            out = _order_key(keys.view(np.float64)).view(np.float64)
    out = canon(out)
    out[nl] = NAN
    return out, nl.copy()


def lag_loop(x, nulls, op, periods):
    v, nl = [float(t) for t in as_f64(x)], _nulls(x, nulls)
    n = len(v)
    out, gone = np.full(n, NAN), np.zeros(n, bool)
    if op == SHIFT:
        for i in range(n):
            s = i - periods                                     # :333
            if 0 <= s < n and not nl[s]:
                out[i] = v[s]
            else:
                gone[i] = True                                  # None
        return canon(out), gone
    assert periods >= 0
    for i in range(periods, n):                                 # :520, :537; the rows before stay vec![NAN; n]
        if nl[i] or nl[i - periods]:
            gone[i] = True
            continue
        prev, curr = v[i - periods], v[i]
        with np.errstate(all="ignore"):
            if op == DIFF:
                out[i] = np.float64(curr) - np.float64(prev)    # :538
            else:
                out[i] = NAN if prev == 0.0 else (np.float64(curr) - np.float64(prev)) / np.float64(prev)     # :523-527
    return canon(out), gone


def lag_twin(x, nulls, op, periods):
    v, nl = as_f64(x), _nulls(x, nulls)
    n = v.shape[0]
    i = np.arange(n, dtype=np.int64)
    s = i - max(-n, min(n, int(periods)))
    has = (s >= 0) & (s < n)
    sc = np.clip(s, 0, max(n - 1, 0))
    out, gone = np.full(n, NAN), np.zeros(n, bool)
    if n == 0:
        return out, gone
    if op == SHIFT:
        gone = ~has | nl[sc]
        return canon(np.where(gone, NAN, v[sc])), gone
    assert periods >= 0
    gone = has & (nl | nl[sc])
    ok = has & ~gone
    with np.errstate(all="ignore"):
        d = v - v[sc]
        r = d if op == DIFF else np.where(v[sc] == 0.0, NAN, d / v[sc])
    return canon(np.where(ok, r, NAN)), gone
