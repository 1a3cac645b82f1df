"""The reference for pandrs_hip_fill and the mirrors' ffill / bfill / fillna_method / interpolate / fillna: two restatements of
PandasCompatExt's row loops (reference src/dataframe/pandas_compat/functions.rs:789-918, :3626-3683), extended by the two
rules of include/pandrs_hip.h: a null bit counts as missing (and the cell under it is never a source), and I64 stays I64
under FFILL / BFILL / VALUE.

  fill_loop   line for line after the reference: one pass with a carried `last_valid` / `next_valid` (fillna_method), the
              first / last valid position and a walk between valid neighbours (interpolate), a map (fillna)
  fill_twin   vectorised numpy: np.maximum.accumulate of the valid row indices, its mirror, and the same f64 expression

Both -> (values, still_missing): values is int64 for an I64 column under FFILL / BFILL / VALUE and float64 otherwise; a row
that stays missing holds the canonical quiet NaN (float64) or 0 (int64).  Compare on the uint64 view: no tolerance."""
import numpy as np

FFILL, BFILL, LINEAR, VALUE = range(4)                          # pandrs_hip_fill_method
METHODS = [FFILL, BFILL, LINEAR, VALUE]
CANON_NAN = np.uint64(0x7FF8000000000000)
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def missing_of(x, nulls):
    x = np.asarray(x)
    miss = np.zeros(x.shape[0], bool) if nulls is None else np.asarray(nulls, bool).copy()
    if x.dtype == np.float64:
        miss |= np.isnan(x)
    return miss


def _result(x, method):
    return np.int64 if x.dtype == np.int64 and method != LINEAR else np.float64


def _gone(dt):
    return np.int64(0) if dt == np.int64 else CANON_NAN.view(np.float64)


def _value_cell(x, value):
    """(the cell a filled row gets, whether it is still missing)"""
    if x.dtype == np.int64:
        return np.int64(value), False
    v = np.float64(value)
    return (CANON_NAN.view(np.float64), True) if np.isnan(v) else (v, False)


def fill_loop(x, nulls, method, value=None):
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    n, miss, dt = x.shape[0], missing_of(x, nulls), _result(x, method)
    out, gone = np.empty(n, dt), np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if method == FFILL:                                     # functions.rs:815-831, :3634-3648
            last = None
            for i in range(n):
                if not miss[i]:
                    last = x[i]
                    out[i] = x[i]
                elif last is not None:
                    out[i] = last
                else:
                    out[i], gone[i] = _gone(dt), True
        elif method == BFILL:                                   # functions.rs:832-845, :3663-3677
            nxt = None
            for i in range(n - 1, -1, -1):
                if not miss[i]:
                    nxt = x[i]
                    out[i] = x[i]
                elif nxt is not None:
                    out[i] = nxt
                else:
                    out[i], gone[i] = _gone(dt), True
        elif method == LINEAR:                                  # functions.rs:870-902
            out[:], gone[:] = _gone(dt), True
            valid = [i for i in range(n) if not miss[i]]
            if valid:
                first, last = valid[0], valid[-1]
                prev_idx, prev_val = first, np.float64(x[first])
                out[first], gone[first] = prev_val, False
                for i in range(first + 1, last + 1):
                    if not miss[i]:
                        cur = np.float64(x[i])
                        if i > prev_idx + 1:
                            gap_size = np.float64(i - prev_idx)
                            value_diff = cur - prev_val
                            for j in range(prev_idx + 1, i):
                                position = np.float64(j - prev_idx)
                                out[j], gone[j] = prev_val + (value_diff * position / gap_size), False
                        prev_idx, prev_val = i, cur
                        out[i], gone[i] = cur, False
        else:                                                   # functions.rs:789-794
            cell, stays = _value_cell(x, value)
            for i in range(n):
                if miss[i]:
                    out[i], gone[i] = cell, stays
                else:
                    out[i] = x[i]
    return out, gone


def fill_twin(x, nulls, method, value=None):
    x = np.asarray(x)
    assert x.dtype in (np.int64, np.float64)
    n, miss, dt = x.shape[0], missing_of(x, nulls), _result(x, method)
    rows = np.arange(n, dtype=np.int64)
    if method == VALUE:
        cell, stays = _value_cell(x, value)
        return np.where(miss, cell, x).astype(dt), miss & stays
    prev = np.maximum.accumulate(np.where(miss, -1, rows)) if n else rows                      # -1: no valid row at or before
    nxt = np.minimum.accumulate(np.where(miss, n, rows)[::-1])[::-1] if n else rows             # n: none at or after
    has_p, has_n = prev >= 0, nxt < n
    p, q = np.where(has_p, prev, 0), np.where(has_n, nxt, 0)
    if method == FFILL:
        gone, out = ~has_p, x[p] if n else x
    elif method == BFILL:
        gone, out = ~has_n, x[q] if n else x
    else:
        gone = ~(has_p & has_n)
        xf = x.astype(np.float64)
        with np.errstate(all="ignore"):
            a, b = (xf[p], xf[q]) if n else (xf, xf)
            den = np.where(q > p, q - p, 1).astype(np.float64)
            out = np.where(miss, a + ((b - a) * (rows - p).astype(np.float64)) / den, xf)
    out = np.where(gone, _gone(dt), out).astype(dt)
    return out, gone


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.dtype.itemsize == 8 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


SPECIAL_F64 = np.array([np.inf, -np.inf, -0.0, 0.0, 5e-324, -2.2250738585072009e-308, 1.7976931348623157e308, 1.0, -3.5, 1e16 + 2])
SPECIAL_I64 = np.array([I64_MIN, I64_MAX, 0, -1, 2**53 + 1, -(2**53) - 1, 2**62 + 12345, 7], np.int64)


def sweep_cases(rng, cases=300, tile=2048):
    """`cases` random (values, nulls or None, method, value) over both dtypes, <= 3 * tile rows: densities from 0 to 100 %
    missing as NaN cells, null bits or both (nulls also over finite cells and over NaN payloads), gaps as single rows and as
    runs up to 3 tiles long, special values, lengths on and around word and tile edges."""
    edges = [1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile]
    for k in range(cases):
        n = int(edges[rng.integers(len(edges))]) if rng.random() < 0.3 else int(rng.integers(1, 3 * tile + 1))
        is_i64 = bool(k % 2)
        if is_i64:
            x = rng.integers(-1000, 1000, n)
            sp = rng.random(n) < 0.05
            x[sp] = SPECIAL_I64[rng.integers(0, len(SPECIAL_I64), int(sp.sum()))]
        else:
            x = rng.normal(0.0, 100.0, n)
            sp = rng.random(n) < 0.05
            x[sp] = SPECIAL_F64[rng.integers(0, len(SPECIAL_F64), int(sp.sum()))]
        density = [0.0, 0.1, 0.5, 0.9, 1.0][int(rng.integers(5))]
        if rng.random() < 0.5:                                  # runs: a gap or a valid stretch of random length
            miss, i = np.zeros(n, bool), 0
            while i < n:
                run = int(rng.integers(1, [4, 70, tile, 3 * tile + 2][int(rng.integers(4))] + 1))
                miss[i:i + run] = rng.random() < density
                i += run
        else:
            miss = rng.random(n) < density
        kind = int(rng.integers(3)) if not is_i64 else 1       # 0: NaN cells, 1: null bits, 2: both
        nulls = None
        if kind in (1, 2):
            nulls = miss & (rng.random(n) < 0.7) if kind == 2 else miss.copy()
        if not is_i64:
            nan = miss & ~nulls if kind == 2 else (miss if kind == 0 else np.zeros(n, bool))
            x[nan] = np.nan
            if nulls is not None:                               # NaN payloads under some null bits
                pay = nulls & (rng.random(n) < 0.2)
                xb = x.view(np.uint64)
                xb[pay] = np.uint64(0x7FF0000000000000) | rng.integers(1, 1 << 51, int(pay.sum())).astype(np.uint64)
        if nulls is not None and not nulls.any() and rng.random() < 0.5:
            nulls = None
        method = METHODS[k % 4] if rng.random() < 0.5 else METHODS[int(rng.integers(4))]
        value = None
        if method == VALUE:
            value = int(SPECIAL_I64[rng.integers(len(SPECIAL_I64))]) if is_i64 else float(np.append(SPECIAL_F64, np.nan)[rng.integers(len(SPECIAL_F64) + 1)])
        yield x, nulls, method, value
