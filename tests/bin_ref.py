"""PandasCompatExt::value_range / cut / qcut (reference src/dataframe/pandas_compat/functions.rs:2270-2282, :2339-2368,
:2370-2420) restated twice: the reference's loops line by line in plain Python floats (IEEE double, every operation rounded
on its own, as Rust's f64), and a fast numpy twin that tests/test_bin_ref.py holds equal to them.  A column is a float64
array (an Int64 column arrives `as f64`, get_column_numeric_values) with an optional boolean null array; a null cell behaves
as NaN (pandrs_hip.h).  Test infrastructure, like oracle/: never imported by pandrs_amd/."""
import math

import numpy as np

NONE, NAN = -1, -2          # PANDRS_HIP_BIN_NONE, PANDRS_HIP_BIN_NAN


class InvalidValue(ValueError):
    pass


def values_of(x, null=None):
    """get_column_numeric_values: float64 cells, a null cell as NaN."""
    v = np.array(x, dtype=np.float64)
    if null is not None:
        v[np.asarray(null, bool)] = np.nan
    return v


# ---- the reference's loops ----------------------------------------------------------------------------------------------
def value_range_loop(values):                                   # :2270-2282
    valid = [float(v) for v in values if not math.isnan(v)]
    if not valid:
        raise InvalidValue("No valid values in column")
    lo, hi = math.inf, -math.inf
    for v in valid:                                             # fold(f64::INFINITY, f64::min) / (NEG_INFINITY, f64::max)
        lo = v if v < lo else lo
        hi = v if v > hi else hi
    return lo, hi


def cut_edges_loop(values, bins):                               # :2340-2351
    if bins == 0:
        raise InvalidValue("Number of bins must be > 0")
    lo, hi = value_range_loop(values)
    w = (hi - lo) / float(bins)                                 # (Python floats: IEEE doubles, inf and NaN without an exception)
    edges = [lo + float(i) * w for i in range(bins + 1)]
    edges[bins] = hi + 0.001
    return edges


def codes_loop(values, edges, last_plus=0.0):
    """The first-match loop both functions share (:2358-2363, :2404-2415): i, NONE or NAN per row.  last_plus: what qcut adds
    to the last upper edge."""
    n_bins = len(edges) - 1
    out = []
    for v in values:
        v = float(v)
        if math.isnan(v):
            out.append(NAN)
            continue
        code = NONE
        for i in range(n_bins):
            upper = edges[i + 1] + last_plus if (i == n_bins - 1 and last_plus) else edges[i + 1]
            if v >= edges[i] and v < upper:
                code = i
                break
        out.append(code)
    return out


def fmt2(x):
    """Rust's {:.2} for a finite f64 (and inf / NaN as Rust spells them)."""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return "%.2f" % x


def cut_loop(values, bins):                                     # :2339-2368
    edges = cut_edges_loop(values, bins)
    result = []
    for code in codes_loop(values, edges):
        if code == NAN:
            result.append("NaN")
        elif code != NONE:                                      # a row that matches no bin pushes nothing
            result.append("(%s, %s]" % (fmt2(edges[code]), fmt2(edges[code + 1])))
    return result


def qcut_edges_loop(values, q):                                 # :2371-2397
    if q == 0:
        raise InvalidValue("Number of quantiles must be > 0")
    valid = [float(v) for v in values if not math.isnan(v)]
    if not valid:
        raise InvalidValue("No valid values")
    valid.sort()                                                # stable, partial_cmp: -0.0 ties 0.0 and keeps row order
    m = len(valid)
    edges = []
    for i in range(q + 1):
        idx = int(float(m) * float(i) / float(q))
        edges.append(valid[min(idx, m - 1)])
    return edges


def qcut_loop(values, q):                                       # :2370-2420
    edges = qcut_edges_loop(values, q)
    out = []
    for code in codes_loop(values, edges, 0.001):
        out.append("NaN" if code == NAN else "" if code == NONE else "Q%d" % (code + 1))
    return out


# ---- the fast twin -------------------------------------------------------------------------------------------------------
def codes(values, edges):
    """pandrs_hip_bin's contract: edges never decrease and hold no NaN; code = (edges <= v) - 1 where that lies in
    [0, n_bins), else NONE; NAN for a NaN cell.  -> (int32 codes, int64 counts of n_bins + 2: the bins, NONE, NAN)."""
    v = np.asarray(values, np.float64)
    e = np.asarray(edges, np.float64)
    assert not np.isnan(e).any() and not (e[1:] < e[:-1]).any()
    n_bins = e.shape[0] - 1
    i = np.searchsorted(e, v, side="right").astype(np.int64) - 1
    out = np.where((i >= 0) & (i < n_bins), i, NONE)
    out = np.where(np.isnan(v), NAN, out).astype(np.int32)
    slot = np.where(out >= 0, out, n_bins - 1 - out.astype(np.int64))
    return out, np.bincount(slot, minlength=n_bins + 2).astype(np.int64)


def value_range(values):
    v = np.asarray(values, np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        raise InvalidValue("No valid values in column")
    return float(v.min()), float(v.max())


def cut_edges(values, bins):
    """The reference's edge list: min + i * w, each operation rounded on its own (numpy does not fuse), then max + 0.001."""
    if bins == 0:
        raise InvalidValue("Number of bins must be > 0")
    lo, hi = value_range(values)
    with np.errstate(all="ignore"):
        w = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
        e = np.float64(lo) + np.arange(bins + 1, dtype=np.float64) * w
        e[bins] = np.float64(hi) + np.float64(0.001)
    return e


def qcut_edges(values, q):
    if q == 0:
        raise InvalidValue("Number of quantiles must be > 0")
    v = np.asarray(values, np.float64)
    v = np.sort(v[~np.isnan(v)], kind="stable")
    m = v.size
    if m == 0:
        raise InvalidValue("No valid values")
    idx = (np.float64(m) * np.arange(q + 1, dtype=np.float64) / np.float64(q)).astype(np.uint64)
    return v[np.minimum(idx, np.uint64(m - 1)).astype(np.int64)]


def search_edges(edges, kind_qcut):
    """What the mirrors hand to pandrs_hip_bin: qcut's last edge + 0.001; cut's last edge clamped to the one before it (no
    row lies between them either way)."""
    e = np.array(edges, np.float64)
    if kind_qcut:
        e[-1] = e[-1] + np.float64(0.001)
    elif e.shape[0] > 1 and e[-1] < e[-2]:
        e[-1] = e[-2]
    return e


def cut(values, bins):
    """-> the reference's list of strings (rows in no bin left out)."""
    v = np.asarray(values, np.float64)
    e = cut_edges(v, bins)
    if np.isnan(e[0]):                                          # w is not finite: every bin is empty
        return ["NaN"] * int(np.isnan(v).sum())
    c, _ = codes(v, search_edges(e, False))
    return ["NaN" if k == NAN else "(%s, %s]" % (fmt2(e[k]), fmt2(e[k + 1])) for k in c.tolist() if k != NONE]


def qcut(values, q):
    v = np.asarray(values, np.float64)
    c, _ = codes(v, search_edges(qcut_edges(v, q), True))
    return ["NaN" if k == NAN else "" if k == NONE else "Q%d" % (k + 1) for k in c.tolist()]
