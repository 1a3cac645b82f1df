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


# ---- the comparison rule of tests/test_gpu_describe.py and of the randomised sweep ---------------------------------------------
FIELD = {"min": "min", "25%": "q1", "50%": "median", "75%": "q3", "max": "max"}     # describe_ref's key -> pandrs_hip_describe_stats'


def same(a, b):
    a, b = np.float64(a), np.float64(b)
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def compare_describe(got, values, nulls, dtype, moments=True):
    """Context.describe's dict against describe_ref: the count, and min, max and the quartiles as equal values (a zero may differ
    in its sign, pandrs_hip.h); with `moments` the mean within 1e-9 of the mean magnitude and std within 1e-9 relative."""
    s, rows = sorted_cells(values, nulls, dtype)
    n = np.asarray(values).shape[0]
    assert got["count"] == s.shape[0], (got["count"], s.shape[0])
    if s.shape[0] == 0:
        assert all(np.isnan(got[f]) for f in ("mean", "std", "min", "q1", "median", "q3", "max")), got
        return
    want = describe_ref(values, nulls, dtype)
    for k, f in FIELD.items():
        assert same(got[f], want[k]), (k, got[f], want[k], n)
    if moments:
        if np.isnan(want["mean"]):
            assert np.isnan(got["mean"])
        else:
            assert abs(got["mean"] - want["mean"]) <= 1e-9 * np.abs(rows).sum() / len(rows), (got["mean"], want["mean"])
        if np.isnan(want["std"]):
            assert np.isnan(got["std"])
        else:
            assert abs(got["std"] - want["std"]) <= 1e-9 * want["std"], (got["std"], want["std"])


def compare_quantiles(q, count, values, nulls, dtype, ps):
    """Context.quantiles' (values, count) against percentile_ref over the sorted cells: equal values, NaN without a cell."""
    s, _ = sorted_cells(values, nulls, dtype)
    n = np.asarray(values).shape[0]
    assert count == s.shape[0] and len(q) == len(ps), (count, s.shape[0], len(q), len(ps))
    if s.shape[0] == 0:
        assert np.isnan(q).all(), q
        return
    for p, v in zip(ps, q):
        assert same(v, percentile_ref(s, p)), (p, v, percentile_ref(s, p), n)
