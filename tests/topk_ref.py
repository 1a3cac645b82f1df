"""PandasCompatExt::nlargest / nsmallest / idxmax / idxmin (reference src/dataframe/pandas_compat/functions.rs:159-192) restated
for the tests of pandrs_hip_topk and pandrs_hip_arg_extreme.

topk_ref_lines   line for line of the reference: enumerate, the stable sort_by with the direction's comparator, truncate.  Valid
                 for columns without NaN and without nulls (the reference's comparator is no total order with a NaN present).
topk_ref         the full contract of include/pandrs_hip.h, vectorised: class (number, NaN, null), then value in the direction,
                 then row (np.lexsort).  I64 as integers, -0.0 tied with 0.0.  -> (rows, n_numbers).
idx_extreme_ref  Iterator::min_by (the first of equals) and max_by (the last of equals) as loops; NaN and null cells skipped.
"""
import functools

import numpy as np


def topk_ref_lines(values, k, largest):
    """functions.rs:159-174.  I64 columns arrive as the integers they are (the header's deviation: no cast to f64)."""
    values = np.asarray(values)
    indexed_values = [(i, (int(v) if values.dtype == np.int64 else float(v))) for i, v in enumerate(values)]   # :161 / :169

    def partial_cmp(a, b):
        return (a > b) - (a < b)                          # -0.0 == 0.0: Equal

    if largest:
        cmp = lambda a, b: partial_cmp(b[1], a[1])        # noqa: E731  :162  b.1.partial_cmp(&a.1)
    else:
        cmp = lambda a, b: partial_cmp(a[1], b[1])        # noqa: E731  :170
    indexed_values.sort(key=functools.cmp_to_key(cmp))    # sort_by is stable, and so is list.sort
    del indexed_values[max(int(k), 0):]                   # :163 truncate
    return np.array([i for i, _ in indexed_values], np.int64)


def _classes(values, nulls):
    values = np.asarray(values)
    n = values.shape[0]
    cls = np.zeros(n, np.int64)
    if values.dtype == np.float64:
        cls[np.isnan(values)] = 1
    if nulls is not None:
        cls[np.asarray(nulls, bool)] = 2
    return values, cls


def topk_ref(values, nulls, k, largest):
    values, cls = _classes(values, nulls)
    n = values.shape[0]
    if values.dtype == np.float64:
        v = np.where(cls > 0, 0.0, values) + 0.0          # -0.0 + 0.0 == 0.0: one value
    else:
        v = np.where(cls > 0, 0, values)
    _, inv = np.unique(v, return_inverse=True)            # dense order-preserving integers: exact for I64 beyond 2^53 too
    inv = inv.astype(np.int64).reshape(-1)
    inv = np.where(cls > 0, 0, -inv if largest else inv)
    order = np.lexsort([np.arange(n), inv, cls]).astype(np.int64)         # the LAST key is the primary one
    kk = max(0, min(int(k), n))
    m = int((cls == 0).sum())
    return order[:kk], min(kk, m)


def idx_extreme_ref(values, nulls=None):
    """-> (idxmin, idxmax), or None when no number exists."""
    values, cls = _classes(values, nulls)
    conv = int if values.dtype == np.int64 else float
    best_min = best_max = None
    for i in range(values.shape[0]):
        if cls[i]:
            continue
        x = conv(values[i])
        if best_min is None or x < best_min[1]:           # min_by: a later equal does not replace
            best_min = (i, x)
        if best_max is None or x >= best_max[1]:          # max_by: a later equal replaces
            best_max = (i, x)
    return None if best_min is None else (best_min[0], best_max[0])
