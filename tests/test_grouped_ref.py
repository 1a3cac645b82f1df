"""tests/grouped_ref.py against a plain per-row loop: one pass over the rows in row order that keeps, per key, the running state
of every fold and the list of the key's earlier cells for the lags.  No sorting, no splitting: nothing the twins do."""
import math

import numpy as np
import pytest

from tests.cumulative_ref import NAN, cum_twin, lag_twin, rust_max, rust_min, same_bits
from tests.grouped_ref import (CUM_COUNT, CUM_MAX, CUM_MIN, CUM_SUM, FOLDS, G_DIFF, G_PCT_CHANGE, G_SHIFT, GROUPED_OPS, LAGS, ROW_NUMBER, group_ids,
                               grouped_twin, grouped_twin_fast)


def loop(keys, x, nulls, op, periods=0):
    """keys: one hashable per row (None-bearing tuples for NULL keys)"""
    n = len(keys)
    v = [float(t) for t in np.asarray(x).astype(np.float64)]
    nl = [False] * n if nulls is None else [bool(t) for t in nulls]
    out = np.zeros(n, np.int64) if op in (CUM_COUNT, ROW_NUMBER) else np.full(n, NAN)
    gone = np.zeros(n, bool)
    state, seen = {}, {}
    for i in range(n):
        k = keys[i]
        cells = seen.setdefault(k, [])                          # the key's earlier rows: (value, null)
        t = len(cells)
        cells.append((v[i], nl[i]))
        if op == ROW_NUMBER:
            out[i] = t
        elif op in FOLDS:
            acc = state.get(k, {CUM_SUM: 0.0, CUM_MAX: -math.inf, CUM_MIN: math.inf, CUM_COUNT: 0}[op])
            if nl[i]:
                if op == CUM_COUNT:
                    out[i] = acc
                else:
                    gone[i] = True
                continue
            if op == CUM_SUM:
                acc = acc + v[i]                                # Python floats: IEEE doubles, inf + -inf is NaN without a warning
            elif op == CUM_MAX:
                acc = rust_max(acc, v[i])
            elif op == CUM_MIN:
                acc = rust_min(acc, v[i])
            elif not math.isnan(v[i]):
                acc += 1
            state[k] = acc
            out[i] = acc
    if op in LAGS:                                              # SHIFT looks ahead: a second pass over the finished lists
        at = {}
        for i in range(n):
            k = keys[i]
            t = at.get(k, 0)
            at[k] = t + 1
            cells, s = seen[k], t - periods
            has = 0 <= s < len(cells)
            if op == G_SHIFT:
                if has and not cells[s][1]:
                    out[i] = cells[s][0]
                else:
                    gone[i] = True
            elif has:
                if nl[i] or cells[s][1]:
                    gone[i] = True
                else:
                    prev, curr = np.float64(cells[s][0]), np.float64(v[i])
                    with np.errstate(all="ignore"):
                        out[i] = curr - prev if op == G_DIFF else (NAN if prev == 0.0 else (curr - prev) / prev)
    if out.dtype == np.float64:
        out[np.isnan(out)] = NAN
    return out, gone


def cases():
    rng = np.random.default_rng(5)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, 1e300, -1e300, 3.0])
    for n in (0, 1, 2, 3, 7, 64, 65, 300):
        for n_keys in (1, 2, 5, max(n, 1)):
            key = rng.integers(0, n_keys, n)
            knull = rng.random(n) < 0.1
            second = rng.integers(0, 2, n)
            x = rng.choice(special, n)
            xi = rng.integers(-5, 6, n)
            nulls = rng.random(n) < 0.2
            for data, nl in ((x, None), (x, nulls), (xi, nulls)):
                yield n, [key], [None], data, nl
                yield n, [key, second], [knull, None], data, nl


def test_twins_against_the_row_loop():
    for n, keys, key_nulls, x, nulls in cases():
        ids = group_ids(keys, key_nulls)
        plain = [tuple(None if kn is not None and kn[i] else int(k[i]) for k, kn in zip(keys, key_nulls)) for i in range(n)]
        for op in GROUPED_OPS:
            for periods in ([0] if op not in LAGS else [-5, -1, 0, 1, 2, 5, n - 1, n, n + 5]):
                if op in (G_DIFF, G_PCT_CHANGE) and periods < 0:
                    continue
                want, gone = loop(plain, x, nulls, op, periods)
                got, g = grouped_twin(ids, x, nulls, op, periods)
                assert same_bits(got, want) and np.array_equal(g, gone), (n, op, periods)
                for long_from in (1, 4, 1 << 20):
                    fast, gf = grouped_twin_fast(ids, x, nulls, op, periods, long_from=long_from)
                    assert same_bits(fast, want) and np.array_equal(gf, gone), (n, op, periods, long_from)


def test_null_keys_form_groups_of_their_own():
    ids = group_ids([np.array([1, 1, 7, 7, 1])], [np.array([False, True, True, False, False])])
    assert ids[0] == ids[4] and ids[1] == ids[2] and len({ids[0], ids[1], ids[3]}) == 3      # the cell under a NULL key is ignored
    two = group_ids([np.array([1, 1, 1]), np.array([5, 5, 6])], [np.array([True, True, True]), None])
    assert two[0] == two[1] != two[2]
    out, _ = grouped_twin(ids, np.arange(5.0), None, ROW_NUMBER)
    assert list(out) == [0, 0, 1, 0, 1]


@pytest.mark.parametrize("n", [0, 1, 5, 300])
def test_a_single_group_is_the_ungrouped_twin(n):
    rng = np.random.default_rng(n)
    x = rng.choice(np.array([np.nan, np.inf, 0.0, -0.0, 1.5, -2.25, 7.0]), n)
    nulls = rng.random(n) < 0.2
    ids = np.zeros(n, np.int64)
    for nl in (None, nulls):
        for op, base in FOLDS.items():
            want, gone = cum_twin(x, nl, base)
            for twin in (grouped_twin, grouped_twin_fast):
                got, g = twin(ids, x, nl, op)
                assert same_bits(got, want) and np.array_equal(g, gone)
        for op, base in LAGS.items():
            for periods in range(-5 if op == G_SHIFT else 0, n + 6):
                want, gone = lag_twin(x, nl, base, periods)
                for twin in (grouped_twin, grouped_twin_fast):
                    got, g = twin(ids, x, nl, op, periods)
                    assert same_bits(got, want) and np.array_equal(g, gone)
    assert list(grouped_twin(ids, x, None, ROW_NUMBER)[0]) == list(range(n))
