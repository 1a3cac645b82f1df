"""numpy twins of pandrs_hip_window_quantile (include/pandrs_hip.h): the rolling / expanding median and quantile of the
reference's src/series/window.rs:298-336, :494-530 and helpers/window_ops.rs:206-240, with the entry's documented
deviations (an empty window and a window holding a NaN value answer NaN).  Shared by tests/test_gpu_window_quantile.py and
experiments/window_quantile_bench.py and checked on their own, without a GPU, by tests/test_window_quantile_ref.py.

window_quantile_ref sorts every window by itself (np.argsort(kind="stable") over keys with -0.0 -> 0.0): the definition,
O(n w log w).  window_quantile_fast answers any window of a long column in O(n log n): the k-th smallest global stable
sort rank among the window's rows, by a binary descent over the rank's bits with prefix counts.  The two are compared on
small inputs; tests of long columns use the fast one."""
import numpy as np

from tests.window_ref import bounds, counts


def rust_round(x):
    """f64::round: half away from zero (x >= 0 here)."""
    t = np.trunc(x)
    return t + (x - t >= 0.5)


def as_f64(x):
    """An I64 column's cells `as f64` (round to nearest even, as numpy converts)."""
    return np.asarray(x).astype(np.float64)


def window_bounds(n, kind, w, center):
    if kind == "expanding":
        return np.zeros(n, np.int64), np.arange(1, n + 1, dtype=np.int64)
    return bounds(n, w, center)


def select_ks(length, median, q):
    """The sorted positions a window of `length` (>= 1) values reads: (k1, k2), k1 != k2 only for an even median."""
    length = np.asarray(length, np.int64)
    if median:
        mid = length // 2
        return np.where(length % 2 == 1, mid, mid - 1), mid
    idx = rust_round(q * (length - 1).astype(np.float64)).astype(np.int64)
    idx = np.minimum(idx, length - 1)
    return idx, idx


def _prepare(x, valid, kind, w, center, min_periods, nan_missing):
    x = as_f64(x)
    n = len(x)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    isnan = np.isnan(x)
    incl = valid & ~isnan if nan_missing else valid
    s, e = window_bounds(n, kind, w, center)
    length = counts(incl, s, e)
    poisoned = np.zeros(n, bool) if nan_missing else counts(valid & isnan, s, e) > 0
    if kind == "rolling":
        mp = w if min_periods is None or min_periods < 0 else min_periods
    else:
        mp = min_periods
    ok = (length >= mp) & (length > 0) & ~poisoned
    return x, incl, s, e, length, ok


def _finish(a, b, two):
    with np.errstate(all="ignore"):
        return np.where(two, (a + b) / 2.0, a)


def window_quantile_ref(x, valid, kind, w=0, center=False, min_periods=None, median=True, q=0.5, nan_missing=False):
    x, incl, s, e, length, ok = _prepare(x, valid, kind, w, center, min_periods, nan_missing)
    out = np.full(len(x), np.nan)
    k1, k2 = select_ks(np.maximum(length, 1), median, q)
    for i in np.flatnonzero(ok):
        v = x[s[i]:e[i]][incl[s[i]:e[i]]]
        srt = v[np.argsort(np.where(v == 0.0, 0.0, v), kind="stable")]
        out[i] = _finish(srt[k1[i]], srt[k2[i]], k1[i] != k2[i])
    return out


class RankIndex:
    """The prefix counts of every bit of a permutation `rank`, from the top bit down, each level stably split by its bit:
    kth(s, e, k) is the k-th smallest (0-based) of rank[s:e) for arrays of queries."""

    def __init__(self, rank):
        a = np.asarray(rank, np.int64)
        self.n = n = len(a)
        self.levels = []
        for bit in reversed(range(max(1, int(n - 1).bit_length()))):
            b = (a >> bit) & 1
            ones = np.concatenate([[0], np.cumsum(b)])
            self.levels.append((bit, ones, n - ones[n]))
            a = np.concatenate([a[b == 0], a[b == 1]])

    def kth(self, s, e, k):
        s, e, k = (np.array(v, np.int64) for v in (s, e, k))
        res = np.zeros(len(s), np.int64)
        for bit, ones, zeros in self.levels:
            os_, oe = ones[s], ones[e]
            c0 = (e - s) - (oe - os_)
            low = k < c0
            res |= np.where(low, 0, 1 << bit)
            k = np.where(low, k, k - c0)
            s = np.where(low, s - os_, zeros + os_)
            e = np.where(low, e - oe, zeros + oe)
        return res


class SortedWindows:
    """One column prepared for any number of windows and statistics (the order and the index are built once)."""

    def __init__(self, x, valid=None, nan_missing=False):
        self.x = x = as_f64(x)
        n = len(x)
        self.valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        self.nan_missing = nan_missing
        isnan = np.isnan(x)
        incl = self.valid & ~isnan if nan_missing else self.valid
        # numbers ascending with -0.0 == 0.0 tied in row order; NaN and excluded cells (key NaN) after every number
        key = np.where(incl & ~isnan, np.where(x == 0.0, 0.0, x), np.nan)
        self.order = np.argsort(key, kind="stable")
        rank = np.empty(n, np.int64)
        rank[self.order] = np.arange(n)
        self.index = RankIndex(rank) if n else None

    def lengths(self, kind, w=0, center=False):
        """Every window's number of values (what min_periods is compared with)."""
        return _prepare(self.x, self.valid, kind, w, center, 0, self.nan_missing)[4]

    def stat(self, kind, w=0, center=False, min_periods=None, median=True, q=0.5):
        x, incl, s, e, length, ok = _prepare(self.x, self.valid, kind, w, center, min_periods, self.nan_missing)
        out = np.full(len(x), np.nan)
        rows = np.flatnonzero(ok)
        if not len(rows):
            return out
        k1, k2 = select_ks(length[rows], median, q)
        r1 = self.index.kth(s[rows], e[rows], k1)
        r2 = self.index.kth(s[rows], e[rows], k2) if median else r1
        out[rows] = _finish(x[self.order[r1]], x[self.order[r2]], k1 != k2)
        return out


def window_quantile_fast(x, valid, kind, w=0, center=False, min_periods=None, median=True, q=0.5, nan_missing=False):
    return SortedWindows(x, valid, nan_missing).stat(kind, w, center, min_periods, median, q)
