"""References for pandrs_hip_pivot and the crosstab / pivot_table / pivot / unstack mirrors.

1. `*_loop`: the reference's three functions restated line by line over Python dicts and sets (crosstab,
   src/dataframe/pandas_compat/functions.rs:2138-2183; PivotTable::execute and aggregate_values_from_vec, src/pivot/mod.rs:107-228;
   unstack, functions.rs:2471-2522).  pivot_table's label order is HashSet order in the reference; the restatement sorts.
2. `pivot_loop`: the device contract (include/pandrs_hip.h) as a per-row dict loop keyed by the two cells, every cell folded by
   the oracle's rules (oracle/oracle_np.py, `fold`).
3. `pivot`: a numpy twin of the same contract: np.unique(..., return_inverse) per key column, ufunc.at per cell.
4. `bound`: what a device Sum / Mean may differ by, 2 gamma_k sum|x| over the cell's own k rows.
Shared by the CPU tests and the GPU tests: no device, no library."""
import math

import numpy as np

from oracle import oracle_np as O
from tests import distinct_ref as D

I64, F64, U32CODE, BOOLBITS = 0, 1, 2, 3
ROWS, SUM, MEAN, MIN, MAX, COUNT, LAST = range(7)
OPS = (ROWS, SUM, MEAN, MIN, MAX, COUNT, LAST)
OP_NAME = {ROWS: "rows", SUM: "sum", MEAN: "mean", MIN: "min", MAX: "max", COUNT: "count", LAST: "last"}
NUMBER, MISSING = 0, 1
_ORACLE_OP = {SUM: O.SUM, MEAN: O.MEAN, MIN: O.MIN, MAX: O.MAX, COUNT: O.COUNT, LAST: O.LAST}
U = 2.0 ** -53


# ---- 1. the reference, line by line -------------------------------------------------------------------------------------
def crosstab_loop(values1, values2):
    """functions.rs:2138-2183 over the two columns' strings -> (unique1, unique2, {u2: [f64 per u1]})."""
    unique1 = sorted(set(values1), key=str.encode)
    unique2 = sorted(set(values2), key=str.encode)
    counts = {}
    for v1, v2 in zip(values1, values2):
        counts[(v1, v2)] = counts.get((v1, v2), 0) + 1
    return unique1, unique2, {u2: [float(counts.get((u1, u2), 0)) for u1 in unique1] for u2 in unique2}


def aggregate_values_from_vec(values, aggfunc):
    """pivot/mod.rs:195-228; aggfunc one of "sum", "mean", "min", "max", "count"."""
    if not values:
        return 0.0
    if aggfunc == "sum":
        s = -0.0                                         # (Iterator::sum for f64 folds from -0.0)
        for x in values:
            s += x
        return s
    if aggfunc == "mean":
        s = -0.0
        for x in values:
            s += x
        return s / float(len(values))
    if aggfunc == "min":
        m = None
        for x in values:
            m = x if m is None else (x if x < m else m)
        return m
    if aggfunc == "max":
        m = None
        for x in values:
            m = x if m is None else (x if x > m else m)
        return m
    return float(len(values))


def pivot_table_loop(index_values, column_values, values, aggfunc):
    """pivot/mod.rs:107-192 -> (index labels, column labels, {column label: [f64 or None per index label]}); None stands for
    the reference's "" (no row holds the pair).  The labels are sorted here; the reference iterates its HashSets."""
    index_set, column_set = set(index_values), set(column_values)
    aggregation_map = {}
    for i in range(min(len(index_values), len(column_values), len(values))):
        aggregation_map.setdefault((index_values[i], column_values[i]), []).append(values[i])
    ilab, clab = sorted(index_set, key=str.encode), sorted(column_set, key=str.encode)
    out = {}
    for c in clab:
        out[c] = [aggregate_values_from_vec(aggregation_map[(i, c)], aggfunc) if (i, c) in aggregation_map else None for i in ilab]
    return ilab, clab, out


def unstack_loop(index_values, column_values, data_values):
    """functions.rs:2471-2522 -> (unique indices, unique cols, {col: [f64 per index]}), NaN where no row holds the pair."""
    unique_indices = sorted(set(index_values), key=str.encode)
    unique_cols = sorted(set(column_values), key=str.encode)
    data_map = {}
    for i in range(len(index_values)):
        data_map[(index_values[i], column_values[i])] = data_values[i]
    return unique_indices, unique_cols, {c: [data_map.get((i, c), math.nan) for i in unique_indices] for c in unique_cols}


# ---- 2. / 3. the device contract ----------------------------------------------------------------------------------------
def _labels(col, n_rows, rank):
    """-> (label cells uint64, flags uint8, per row the label's index): numbers in BY_VALUE order, then one missing label."""
    data, mask, dtype = col
    cells = D.cells_of(data, dtype, n_rows)[:n_rows]
    missing = D.null_of(mask, n_rows)
    if dtype == F64:
        missing = missing | ((cells & ~D.SIGN) > np.uint64(0x7FF0000000000000))
    if dtype == U32CODE and rank is not None:
        key = np.asarray(rank, np.uint32)[np.where(missing, 0, cells).astype(np.int64)].astype(np.uint64)
    else:
        key = D.image_of(cells, dtype)
    uniq, first, inverse = np.unique(key[~missing], return_index=True, return_inverse=True)
    labels = cells[~missing][first]
    flags = np.zeros(labels.shape[0], np.uint8)
    at = np.full(n_rows, labels.shape[0], np.int64)
    at[~missing] = inverse
    if missing.any():
        labels, flags = np.append(labels, np.uint64(0)), np.append(flags, np.uint8(MISSING))
    return labels.astype(np.uint64), flags, at


def pivot_loop(index_col, columns_col, n_rows, op, values_col=None, index_rank=None, columns_rank=None):
    """The contract as a per-row loop: rows are collected per (index label, columns label) in a dict, every cell is the oracle's
    fold of its row list.  -> (index labels, index flags, column labels, column flags, cells (C, R), rows (C, R))."""
    il, fi, ia = _labels(index_col, n_rows, index_rank)
    cl, fc, ca = _labels(columns_col, n_rows, columns_rank)
    groups = {}
    for r in range(n_rows):
        groups.setdefault((int(ia[r]), int(ca[r])), []).append(r)
    cells = np.full((cl.shape[0], il.shape[0]), math.nan)
    rows = np.zeros((cl.shape[0], il.shape[0]), np.int64)
    for (i, j), members in groups.items():
        rows[j, i] = len(members)
        cells[j, i] = float(len(members)) if op == ROWS else O.fold(values_col, _ORACLE_OP[op], members)
    return il, fi, cl, fc, cells, rows


def _values(values_col, n_rows):
    data, mask, dtype = values_col
    return np.asarray(data)[:n_rows], ~D.null_of(mask, n_rows), dtype


def pivot(index_col, columns_col, n_rows, op, values_col=None, index_rank=None, columns_rank=None):
    """The same result from numpy: one flat cell id per row, np.add.at / np.minimum.at / np.maximum.at per cell."""
    il, fi, ia = _labels(index_col, n_rows, index_rank)
    cl, fc, ca = _labels(columns_col, n_rows, columns_rank)
    R, C = il.shape[0], cl.shape[0]
    flat = ca * R + ia
    rows = np.bincount(flat, minlength=R * C).astype(np.int64) if n_rows else np.zeros(R * C, np.int64)
    present = rows > 0
    cells = np.full(R * C, math.nan)
    if op in (ROWS, COUNT):
        cells[present] = rows[present].astype(np.float64)
    else:
        v, ok, dtype = _values(values_col, n_rows)
        if op in (SUM, MEAN):
            nn = np.bincount(flat[ok], minlength=R * C)
            if dtype == I64:
                s = np.zeros(R * C, np.uint64)
                np.add.at(s, flat[ok], v[ok].astype(np.int64).view(np.uint64))       # wraps, as the engine's int64 sum
                total = s.view(np.int64).astype(np.float64)
            else:
                total = np.zeros(R * C, np.float64)
                with np.errstate(invalid="ignore"):
                    np.add.at(total, flat[ok], v[ok].astype(np.float64))              # in row order, from +0.0
            with np.errstate(invalid="ignore", divide="ignore"):
                out = total if op == SUM else np.where(nn > 0, total / np.maximum(nn, 1), 0.0)
            cells[present] = out[present]
        elif op in (MIN, MAX):
            if dtype == I64:
                sentinel = np.int64(2 ** 63 - 1) if op == MIN else np.int64(-2 ** 63)
                acc = np.full(R * C, sentinel, np.int64)
                (np.minimum if op == MIN else np.maximum).at(acc, flat[ok], v[ok].astype(np.int64))
                out = np.where(acc == sentinel, 0.0, acc.astype(np.float64))
            else:                                                                    # on the order image: -0.0 < 0.0, NaN cells skipped
                bits = v.astype(np.float64).view(np.uint64)
                ok = ok & ~((bits & ~D.SIGN) > np.uint64(0x7FF0000000000000))
                image = D.image_of(bits, F64)
                sentinel = D.image_of(np.array([math.inf if op == MIN else -math.inf]).view(np.uint64), F64)[0]
                acc = np.full(R * C, sentinel, np.uint64)
                (np.minimum if op == MIN else np.maximum).at(acc, flat[ok], image[ok])
                out = np.where(acc == sentinel, 0.0, D.cells_of_image(acc, F64).view(np.float64))
            cells[present] = out[present]
        else:                                                                        # LAST
            last = np.full(R * C, -1, np.int64)
            np.maximum.at(last, flat, np.arange(n_rows, dtype=np.int64))
            at = last[present]
            cells[present] = np.where(ok[at], v[at].astype(np.float64), 0.0)
    return il, fi, cl, fc, cells.reshape(C, R), rows.reshape(C, R)


def bound(index_col, columns_col, n_rows, op, values_col, index_rank=None, columns_rank=None):
    """(C, R) float64: how far a device Sum / Mean of an F64 column may lie from the row-order fold, 2 gamma_k sum|x| over the
    cell's own k counted rows (divided by k for Mean); 0 for every other op and for I64 values (exact)."""
    il, _, ia = _labels(index_col, n_rows, index_rank)
    cl, _, ca = _labels(columns_col, n_rows, columns_rank)
    R, C = il.shape[0], cl.shape[0]
    out = np.zeros(R * C)
    if op in (SUM, MEAN) and values_col is not None and values_col[2] == F64:
        v, ok, _ = _values(values_col, n_rows)
        flat = (ca * R + ia)[ok]
        k = np.bincount(flat, minlength=R * C).astype(np.float64)
        mag = np.zeros(R * C)
        with np.errstate(invalid="ignore"):
            np.add.at(mag, flat, np.abs(v[ok].astype(np.float64)))
        gamma = k * U / (1.0 - k * U)
        out = 2.0 * gamma * mag
        if op == MEAN:
            out = out / np.maximum(k, 1.0)
    return out.reshape(C, R)


def spans(index_col, columns_col, n_rows):
    """The number of table cells of the contract's direct path, (span1 + 1) * (span2 + 1) with span = max - min + 1 and the + 1
    the missing slot, or None when either column is not addressable by value."""
    total = 1
    for data, mask, dtype in (index_col, columns_col):
        null = D.null_of(mask, n_rows) if mask is not None else None
        if not D.direct_possible(np.asarray(data) if dtype == BOOLBITS else np.asarray(data)[:n_rows], dtype, null, n_rows, max_cells=1 << 62):
            return None
        cells = D.cells_of(data, dtype, n_rows)[:n_rows]
        number = ~D.null_of(mask, n_rows)
        if dtype == F64:
            number &= ~((cells & ~D.SIGN) > np.uint64(0x7FF0000000000000))
        c = cells[number]
        if c.size == 0:
            span = 1
        elif dtype == F64:
            span = int(c.view(np.float64).max()) - int(c.view(np.float64).min()) + 1
        elif dtype == I64:
            span = int(c.view(np.int64).max()) - int(c.view(np.int64).min()) + 1
        else:
            span = int(c.max()) - int(c.min()) + 1
        total *= span + 1
    return total


class Stand:
    """Context.pivot answered by the twin, and a record of the calls: the mirrors' CPU stand-in."""
    device = 0

    def __init__(self):
        self.calls = []

    def pivot(self, index_col, columns_col, n_rows, op, values_col=None, index_rank=None, columns_rank=None, out_device=False):
        self.calls.append(("pivot", index_col[2], columns_col[2], n_rows, op, values_col is not None, index_rank is not None, columns_rank is not None))
        il, fi, cl, fc, cells, rows = pivot(tuple(index_col), tuple(columns_col), n_rows, op, None if values_col is None else tuple(values_col),
                                            index_rank, columns_rank)
        info = {"n_index_labels": int(il.shape[0]), "n_column_labels": int(cl.shape[0]), "n_cells_present": int((rows > 0).sum()),
                "index_missing_rows": int(rows[:, fi == MISSING].sum()), "column_missing_rows": int(rows[fc == MISSING].sum()), "path": 0}
        return il, fi, cl, fc, cells, rows, info


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------
KEY_KINDS = ("i64", "f64", "code", "code_rank", "bool")


def make_key(rng, n, kind, card, null_frac=0.0, nan_frac=0.0, base=0):
    """-> ((data, mask, dtype), rank or None): a key column of `card` distinct numbers from `base` on; F64 keys are integral."""
    rank = None
    if kind == "i64":
        col = (np.int64(base) + rng.integers(0, card, n).astype(np.int64), I64)
    elif kind == "f64":
        data = (base + rng.integers(0, card, n)).astype(np.float64)
        if nan_frac:
            data[rng.random(n) < nan_frac] = np.nan
        col = (data, F64)
    elif kind in ("code", "code_rank"):
        col = (rng.integers(0, card, n).astype(np.uint32), U32CODE)
        if kind == "code_rank":
            rank = rng.permutation(card + 3).astype(np.uint32)
    else:
        col = (np.packbits(rng.integers(0, 2, n).astype(bool), bitorder="little"), BOOLBITS)
    mask = np.packbits(rng.random(n) < null_frac, bitorder="little") if null_frac else None
    return (col[0], mask, col[1]), rank


def make_values(rng, n, dtype, null_frac=0.0, special=False):
    """A values column; `special` mixes NaN, +-inf and signed zeros into an F64 column."""
    if dtype == I64:
        data = rng.integers(-1000, 1000, n).astype(np.int64)
    else:
        data = rng.normal(0.0, 100.0, n)
        if special and n:
            pick = rng.random(n)
            data[pick < 0.05] = np.nan
            data[(pick >= 0.05) & (pick < 0.08)] = np.inf
            data[(pick >= 0.08) & (pick < 0.11)] = -np.inf
            data[(pick >= 0.11) & (pick < 0.16)] = 0.0
            data[(pick >= 0.16) & (pick < 0.21)] = -0.0
    mask = np.packbits(rng.random(n) < null_frac, bitorder="little") if null_frac else None
    return (data, mask, dtype)


def grid_cases(n=300, seed=11):
    """Every op x key kind x masked / unmasked x values dtype, small: (name, index_col, columns_col, values_col or None, n, op,
    index_rank, columns_rank).  The columns key is always of another kind than the index key."""
    rng = np.random.default_rng(seed)
    for op in OPS:
        for ki, kind in enumerate(KEY_KINDS):
            other = KEY_KINDS[(ki + 2) % len(KEY_KINDS)]
            for masked in (False, True):
                for vdt in ((None,) if op == ROWS else (F64, I64)):
                    k1, r1 = make_key(rng, n, kind, 5, 0.1 if masked else 0.0, 0.1 if masked else 0.0, base=-2)
                    k2, r2 = make_key(rng, n, other, 7, 0.1 if masked else 0.0, 0.1 if masked else 0.0, base=40)
                    v = None if vdt is None else make_values(rng, n, vdt, 0.15 if masked else 0.0, special=masked)
                    yield ("%s-%s-%s-%s-%s" % (OP_NAME[op], kind, other, "masked" if masked else "plain", {None: "none", F64: "f64", I64: "i64"}[vdt]),
                           k1, k2, v, n, op, r1, r2)
