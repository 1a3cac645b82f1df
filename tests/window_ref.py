"""numpy restatements of the reference's window loops (src/series/window.rs: Rolling :163-345, Expanding :379-500,
EWM :608-724), shared by tests/test_gpu_window.py and experiments/fuzz_ops.py and checked on their own, without a GPU,
by tests/test_references.py.  A row-order fold is restated exactly: an accumulator starts at -0.0 and the window's
values are added one shifted slice at a time, in ascending rows."""
import math

import numpy as np


def same(got, want):
    """NaN positions equal and every other value bit-identical."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and got[~gn].tobytes() == want[~wn].tobytes()


def first_diff(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~gn & ~wn & (got.view(np.int64) != want.view(np.int64))))
    return None if not len(bad) else (int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


# ---- restatements of series/window.rs ------------------------------------------------------------------------------------
def bounds(n, w, center):
    i = np.arange(n, dtype=np.int64)
    if center:
        half = w // 2
        s = np.where(i >= half, i - half, 0)
        e = np.minimum(s + w, n)
    else:
        s = np.where(i + 1 >= w, i + 1 - w, 0)
        e = i + 1
    return s, e


def fold(x, valid, s, e, mean=None):
    """Each row's window values (non-null, ascending rows) folded from -0.0: x, or (x-mean)*(x-mean)."""
    n = len(x)
    acc = np.full(n, -0.0)
    if n == 0:
        return acc
    with np.errstate(all="ignore"):
        for k in range(int((e - s).max())):
            idx = s + k
            j = np.minimum(idx, n - 1)
            m = (idx < e) & valid[j]
            if mean is None:
                t = x[j]
            else:
                d = x[j] - mean
                t = d * d
            acc = acc + np.where(m, t, -0.0)
    return acc


def counts(valid, s, e):
    c = np.concatenate([[0], np.cumsum(valid, dtype=np.int64)])
    return c[e] - c[s]


def rolling_ref(x, valid, w, center, op, mp=None, ddof=1):
    n = len(x)
    s, e = bounds(n, w, center)
    cnt = counts(valid, s, e)
    mp = w if mp is None else mp
    ok = cnt >= mp
    with np.errstate(all="ignore"):
        if op == "count":
            return np.where(ok, cnt, 0).astype(np.float64)
        if op in ("min", "max"):
            return np.where(ok, extreme(x, valid, s, e, op == "max"), np.nan)
        acc = fold(x, valid, s, e)
        if op == "sum":
            return np.where(ok, acc, np.nan)
        mean = acc / cnt.astype(np.float64)
        if op == "mean":
            return np.where(ok, mean, np.nan)
        sq = fold(x, valid, s, e, mean)
        var = sq / (cnt - ddof).astype(np.float64)
        r = var if op == "var" else np.sqrt(var)
        return np.where(ok & (cnt > ddof), r, np.nan)


def pick(a, b, mx):
    """fold(+-INFINITY, f64::min / max) on non-NaN values, with -0.0 < +0.0."""
    if mx:
        take_b = (b > a) | ((a == b) & ~np.signbit(b))
    else:
        take_b = (b < a) | ((a == b) & np.signbit(b))
    return np.where(take_b, b, a)


def extreme(x, valid, s, e, mx):
    """Sparse table: any window is two (overlapping) power-of-two runs; the pick is a total order, so overlap is harmless."""
    n = len(x)
    ident = -np.inf if mx else np.inf
    v = np.where(valid & ~np.isnan(x), x, ident)
    L = e - s
    levels = [v]
    p = 1
    while 2 * p <= L.max():
        prev = levels[-1]
        sh = np.concatenate([prev[p:], np.full(p, ident)])
        levels.append(pick(prev, sh, mx))
        p *= 2
    tab = np.stack(levels)
    k = np.floor(np.log2(np.maximum(L, 1))).astype(np.int64)
    k = np.where((1 << (k + 1)) <= L, k + 1, k)
    k = np.where((1 << k) > L, k - 1, k)
    return pick(tab[k, s], tab[k, e - (1 << k)], mx)


def expanding_ref_exact(x, valid, op, mp):
    n = len(x)
    return rolling_ref(x, valid, n + 1, False, op, mp=mp) if n else np.zeros(0)


def ewm_ref(x, valid, alpha, op):
    """series/window.rs:640-724, line by line."""
    out = []
    if op == "mean":
        y = None
        for v, ok in zip(x, valid):
            if ok:
                y = v if y is None else alpha * v + (1.0 - alpha) * y
            out.append(np.nan if y is None else y)
        return np.array(out)
    m = var = None
    for v, ok in zip(x, valid):
        if ok:
            if m is None:
                m, var = v, 0.0
                out.append(np.nan)
            else:
                prev = m
                m = alpha * v + (1.0 - alpha) * prev
                diff = v - prev
                var = (1.0 - alpha) * (var + alpha * diff * diff)
                out.append(math.sqrt(var))
        else:
            out.append(np.nan if var is None else math.sqrt(var))
    r = np.array(out)
    return r * r if op == "var" else r


def two_pass_prefix(x, valid):
    n = len(x)
    xz = np.where(valid, x, 0.0)
    c = np.cumsum(valid)
    mean = np.cumsum(xz) / np.maximum(c, 1)
    m2 = np.empty(n)
    for i in range(n):
        v = x[:i + 1][valid[:i + 1]]
        m2[i] = ((v - mean[i]) * (v - mean[i])).sum()
    return c, m2


# ---- the bounds of DESIGN.md §2 for the statistics that are not bit for bit --------------------------------------------
def ewm_close(got, want, x, valid, sq=False):
    amax = np.maximum.accumulate(np.abs(np.where(valid, x, 0.0)))
    b = 2e-12 * amax ** 2 if sq else 1e-12 * amax
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and (np.abs(got[~gn] - want[~wn]) <= b[~gn]).all()


def expanding_sum_mean_close(got, x, valid, mp, mean):
    """Expanding sum / mean of finite values: within 1e-9 of the prefix of |x| (over the count for the mean) of numpy's
    sequential row-order prefix, NaN exactly where fewer than mp values have been seen (and, for the mean, none)."""
    xz = np.where(valid, x, 0.0)
    want = np.cumsum(xz)
    bound = 1e-9 * np.cumsum(np.abs(xz))
    c = np.cumsum(valid)
    ok = (c >= mp) & (c > 0) if mean else c >= mp
    if not np.array_equal(np.isnan(got), ~ok):
        return False
    if mean:
        return bool((np.abs(got[ok] - want[ok] / c[ok]) <= bound[ok] / c[ok]).all())
    return bool((np.abs(got[ok] - want[ok]) <= bound[ok]).all())


def expanding_var_std_close(got, x, valid, ddof, mp, std):
    """Expanding var / std of finite values against the two-pass prefix: 1e-9 relative plus 1e-12 amax^2 (var),
    1e-9 relative plus 1e-6 amax (std); NaN exactly where count < mp or count <= ddof."""
    c, m2 = two_pass_prefix(x, valid)
    amax = np.maximum.accumulate(np.abs(np.where(valid, x, 0.0)))
    ok = (c >= mp) & (c > ddof)
    with np.errstate(all="ignore"):
        var = m2 / (c - ddof)
        sd = np.sqrt(var)
    if not np.array_equal(np.isnan(got), ~ok):
        return False
    if std:
        return bool((np.abs(got[ok] - sd[ok]) <= 1e-9 * sd[ok] + 1e-6 * amax[ok]).all())
    return bool((np.abs(got[ok] - var[ok]) <= 1e-9 * np.abs(var[ok]) + 1e-12 * amax[ok] ** 2).all())
