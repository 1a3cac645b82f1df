"""The reference for pandrs_hip_grouped and GroupBy's cumsum / cummax / cummin / cumcount / row_number / shift / diff /
pct_change: a grouped op gives, for every group, the result of the ungrouped op on that group's rows in ascending row order,
written back at those rows' positions (include/pandrs_hip.h).  So the twin splits the rows by a stable argsort of the group id
and runs tests/cumulative_ref.py's cum_twin / lag_twin per group; ROW_NUMBER is a range per group.

  group_ids     key columns (with optional null flags: a NULL key is a key value of its own) -> one int64 id per row
  grouped_twin  -> (values, null_bits) as cumulative_ref: float64 (int64 for CUM_COUNT and ROW_NUMBER), canonical NaNs
  grouped_twin_fast  the same cells for inputs with very many groups: groups of `long_from` rows or more go through cum_twin
                as above, the shorter ones are folded together, the t-th row of every group in one numpy step (each group still
                sees exactly cum_twin's sequence of operations); the lags are one vectorised pass over the sorted layout.
                tests/test_grouped_ref.py holds it to grouped_twin bit for bit.
  compare_grouped  a device result against the twin, per group, through cumulative_ref.compare_cells"""
import numpy as np

from tests.cumulative_ref import (COUNT, DIFF, MAX, MIN, NAN, PCT_CHANGE, SHIFT, SUM, _order_key, as_f64, canon, compare_cells, cum_twin,
                                  lag_twin, same_bits)

CUM_SUM, CUM_MAX, CUM_MIN, CUM_COUNT, ROW_NUMBER, G_SHIFT, G_DIFF, G_PCT_CHANGE = range(8)      # pandrs_hip_grouped_op
GROUPED_OPS = list(range(8))
FOLDS = {CUM_SUM: SUM, CUM_MAX: MAX, CUM_MIN: MIN, CUM_COUNT: COUNT}
LAGS = {G_SHIFT: SHIFT, G_DIFF: DIFF, G_PCT_CHANGE: PCT_CHANGE}
INT_OPS = (CUM_COUNT, ROW_NUMBER)


def group_ids(keys, key_nulls=None):
    """One id per row from one or more key columns; rows are equal when every key is equal or NULL in both."""
    keys = [np.asarray(k) for k in keys]
    n = keys[0].shape[0]
    cols = []
    for i, k in enumerate(keys):
        nl = np.zeros(n, bool) if key_nulls is None or key_nulls[i] is None else np.asarray(key_nulls[i], bool)
        cols += [np.where(nl, 0, k), nl]
    if n == 0:
        return np.zeros(0, np.int64)
    _, ids = np.unique(np.stack(cols, axis=1), axis=0, return_inverse=True)
    return np.asarray(ids, np.int64).reshape(n)


def split(ids):
    """-> the list of ascending row-index arrays, one per group (a stable argsort keeps row order inside a group)"""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    cuts = np.flatnonzero(np.diff(ids[order])) + 1
    return [g for g in np.split(order, cuts) if g.size]


def grouped_twin(ids, x, nulls, op, periods=0):
    n = np.asarray(ids).shape[0]
    out = np.zeros(n, np.int64) if op in INT_OPS else np.full(n, NAN)
    gone = np.zeros(n, bool)
    nl = None if nulls is None else np.asarray(nulls, bool)
    for rows in split(ids):
        if op == ROW_NUMBER:
            out[rows] = np.arange(rows.size)
            continue
        xs, ns = np.asarray(x)[rows], None if nl is None else nl[rows]
        v, g = cum_twin(xs, ns, FOLDS[op]) if op in FOLDS else lag_twin(xs, ns, LAGS[op], periods)
        out[rows], gone[rows] = v, g
    return out, gone


def layout_of(ids):
    """The sorted layout of a grouping, computed once for several grouped_twin_fast calls: (order: sorted position -> row, the
    first position of every group, every group's length, the first position of its group per position)."""
    ids = np.asarray(ids)
    n = ids.shape[0]
    order = np.argsort(ids, kind="stable")
    head = np.concatenate([[True], ids[order][1:] != ids[order][:-1]]) if n else np.zeros(0, bool)
    begin = np.flatnonzero(head)
    length = np.diff(np.concatenate([begin, [n]]))
    return order, begin, length, np.repeat(begin, length)


def grouped_twin_fast(ids, x, nulls, op, periods=0, long_from=1024, layout=None):
    n = np.asarray(ids).shape[0]
    out = np.zeros(n, np.int64) if op in INT_OPS else np.full(n, NAN)
    gone = np.zeros(n, bool)
    if n == 0:
        return out, gone
    order, begin, length, start = layout_of(ids) if layout is None else layout
    j = np.arange(n, dtype=np.int64)
    if op == ROW_NUMBER:
        out[order] = j - start
        return out, gone
    v = as_f64(x)[order]
    nl = np.zeros(n, bool) if nulls is None else np.asarray(nulls, bool)[order]
    if op in LAGS:
        s = j - max(-n, min(n, int(periods)))
        has = (s >= 0) & (s < n)
        sc = np.clip(s, 0, n - 1)
        has &= start[sc] == start
        if op == G_SHIFT:
            g = ~has | nl[sc]
            res = canon(np.where(g, NAN, v[sc]))
        else:
            assert periods >= 0
            g = has & (nl | nl[sc])
            with np.errstate(all="ignore"):
                d = v - v[sc]
                r = d if op == G_DIFF else np.where(v[sc] == 0.0, NAN, d / v[sc])
            res = canon(np.where(has & ~g, r, NAN))
        out[order], gone[order] = res, g
        return out, gone
    res = np.zeros(n, np.int64) if op == CUM_COUNT else np.full(n, NAN)
    for b, ln in zip(begin[length >= long_from], length[length >= long_from]):
        res[b:b + ln] = cum_twin(v[b:b + ln], nl[b:b + ln], FOLDS[op])[0]
    live, ln = begin[length < long_from], length[length < long_from]
    if op == CUM_SUM:
        acc = np.zeros(live.shape[0])
    elif op == CUM_COUNT:
        acc = np.zeros(live.shape[0], np.int64)
    else:
        first = -np.inf if op == CUM_MAX else np.inf
        acc = _order_key(np.full(live.shape[0], first))
    t = 0
    with np.errstate(all="ignore"):
        while live.size:
            keep = ln > t
            live, ln, acc = live[keep], ln[keep], acc[keep]
            p = live + t
            if op == CUM_SUM:
                acc = acc + np.where(nl[p], -0.0, v[p])
                res[p] = acc
            elif op == CUM_COUNT:
                acc = acc + ~(nl[p] | np.isnan(v[p]))
                res[p] = acc
            else:
                key = _order_key(np.where(nl[p] | np.isnan(v[p]), first, v[p]))
                acc = np.maximum(acc, key) if op == CUM_MAX else np.minimum(acc, key)
                res[p] = _order_key(acc.view(np.float64)).view(np.float64)
            t += 1
    if op != CUM_COUNT:
        res = canon(res)
        res[nl] = NAN
        gone[order] = nl
    out[order] = res
    return out, gone


def compare_grouped(op, ids, got, want, x, nulls, exact):
    """The cells of one grouped call against the twin's: the lags, ROW_NUMBER, MAX, MIN and COUNT (and a SUM the caller knows to
    be exact) bit for bit; any other SUM through cumulative_ref.compare_cells on every group's own rows, so that k and the
    running sum of |x| in its bound 2 gamma_k sum|x| cover the group's prefix and nothing else."""
    assert got.dtype == want.dtype and got.shape == want.shape
    if op != CUM_SUM or exact:
        assert same_bits(got, want), (op, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:5])
        return
    nl = None if nulls is None else np.asarray(nulls, bool)
    for rows in split(ids):
        compare_cells(SUM, got[rows], want[rows], np.asarray(x)[rows], None if nl is None else nl[rows], False)
