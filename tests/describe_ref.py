"""The reference's describe and percentile (src/stats/descriptive.rs:91-200, as OptimizedDataFrame::describe calls them,
src/optimized/split_dataframe/stats.rs:50-151) restated in numpy, for the tests only.  Two deviations, those of
include/pandrs_hip.h: a NaN cell counts and orders after every number (the reference panics on it), and the order is by the
order-preserving code, so -0.0 comes before +0.0.  Everything else is the reference's arithmetic, operation by operation:
the sum and the squared deviations are folded in row order (numpy's cumsum is that fold)."""
import numpy as np

KEYS = ("count", "mean", "std", "min", "25%", "50%", "75%", "max")


def order_code(x):
    """f64 -> the unsigned code whose order is the column order (-0.0 before +0.0; NaN is handled by the caller)."""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def sorted_cells(values, nulls, dtype):
    """The non-null cells in column order as f64 (`v as f64` for int64), and in row order."""
    v = np.asarray(values)
    keep = np.ones(v.shape[0], bool) if nulls is None else ~np.asarray(nulls, bool)
    v = v[keep]
    if np.dtype(dtype) == np.int64:
        v = v.astype(np.int64)
        return np.sort(v, kind="stable").astype(np.float64), v.astype(np.float64)
    v = v.astype(np.float64)
    nan = np.isnan(v)
    order = np.lexsort((order_code(np.where(nan, 0.0, v)), nan))          # numbers by code, then the NaN block
    return v[order], v


def percentile_ref(sorted_data, p):
    """descriptive.rs:169-200 on an ascending float64 array."""
    s = np.asarray(sorted_data, np.float64)
    if s.shape[0] == 0:
        raise ValueError("Cannot compute percentile for empty data")
    p = np.float64(p)
    if p < 0.0 or p > 100.0 or np.isnan(p):
        raise ValueError("Percentile must be between 0 and 100")
    if p == 0.0:
        return s[0]
    if p == 100.0:
        return s[-1]
    n = s.shape[0]
    index = (p / np.float64(100.0)) * np.float64(n - 1)
    lower, upper = int(np.floor(index)), int(np.ceil(index))
    if lower == upper:
        return s[lower]
    weight = index - np.float64(lower)
    with np.errstate(all="ignore"):
        return s[lower] * (np.float64(1.0) - weight) + s[upper] * weight


def describe_ref(values, nulls, dtype):
    """descriptive.rs:91-166, the eight values OptimizedDataFrame::describe returns, as a dict keyed like its stats map
    (plus "sorted": the ordered cells).  ValueError for a column without a non-null cell (:92-96)."""
    s, rows = sorted_cells(values, nulls, dtype)
    n = s.shape[0]
    if n == 0:
        raise ValueError("Cannot compute statistics for empty data")
    with np.errstate(all="ignore"):
        mean = np.cumsum(rows)[-1] / np.float64(n)
        d = rows - mean
        variance = np.cumsum(d * d)[-1] / np.float64(n - 1)
        std = np.sqrt(variance)
    return {"count": n, "mean": mean, "std": std, "min": s[0], "25%": percentile_ref(s, 25.0), "50%": percentile_ref(s, 50.0),
            "75%": percentile_ref(s, 75.0), "max": s[-1], "sorted": s}
