"""References for pandrs_hip_distinct and the value_counts / unique / nunique / mode / is_unique mirrors.

1. `*_loop`: the reference's functions restated line by line over Python dicts (src/dataframe/pandas_compat/functions.rs:343-384,
   :775-788, :1709-1753, :4120-4139, :4226-4259).  A dict stands in for the HashMap: where the reference's answer depends on
   HashMap order (values that compare Equal under partial_cmp: NaN payloads, -0.0 / 0.0; max_by_key among equal counts) the
   restatement's answer is ONE of the reference's possible answers, and `deterministic()` says whether an input has only one.
2. `distinct`: a fast numpy twin of the device contract (include/pandrs_hip.h): one entry per distinct number in the total
   order of the bits' order-preserving image, then one NaN entry, then one NULL entry; counts exact.
Shared by the CPU tests and the GPU tests: no device, no library."""
import functools
import math
import struct

import numpy as np

I64, F64, U32CODE, BOOLBITS = 0, 1, 2, 3
BY_VALUE, BY_COUNT = 0, 1
NUMBER, NAN, NULL = 0, 1, 2
SIGN = np.uint64(1 << 63)
CANON_NAN = np.uint64(0x7FF8000000000000)


# ---- 1. the reference, line by line -------------------------------------------------------------------------------------
def to_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _cmp(a, b):
    return (a > b) - (a < b)


def _partial_cmp_or_equal(a, b):
    """a.partial_cmp(&b).unwrap_or(Ordering::Equal)"""
    if a != a or b != b:
        return 0
    return _cmp(a, b)


def value_counts_loop(values):
    """functions.rs:359-368 over the column's strings."""
    counts = {}
    for value in values:
        counts[value] = counts.get(value, 0) + 1
    result = list(counts.items())
    result.sort(key=functools.cmp_to_key(lambda a, b: _cmp(b[1], a[1]) or _cmp(a[0].encode(), b[0].encode())))
    return result


def value_counts_numeric_loop(values):
    """functions.rs:369-384 over the column's f64 values."""
    counts = {}
    for value in values:
        counts[to_bits(value)] = counts.get(to_bits(value), 0) + 1
    result = [(from_bits(bits), count) for bits, count in counts.items()]
    result.sort(key=functools.cmp_to_key(lambda a, b: _cmp(b[1], a[1]) or _partial_cmp_or_equal(a[0], b[0])))
    return result


def nunique_loop(columns):
    """functions.rs:343-352: `columns` = [(name, the column's strings)]."""
    return [(name, len(set(values))) for name, values in columns]


def unique_loop(values):
    """functions.rs:775-781."""
    return sorted(set(values), key=lambda s: s.encode())


def unique_numeric_loop(values):
    """functions.rs:782-788."""
    unique_set = {}
    for v in values:
        unique_set[to_bits(v)] = None
    result = [from_bits(b) for b in unique_set]
    result.sort(key=functools.cmp_to_key(_partial_cmp_or_equal))
    return result


def mode_numeric_loop(values):
    """functions.rs:1709-1730."""
    counts = {}
    for v in values:
        if v == v:
            counts[to_bits(v)] = counts.get(to_bits(v), 0) + 1
    if not counts:
        return []
    max_count = max(counts.values())
    modes = [from_bits(bits) for bits, c in counts.items() if c == max_count]
    modes.sort(key=functools.cmp_to_key(_partial_cmp_or_equal))
    return modes


def mode_string_loop(values):
    """functions.rs:1732-1753."""
    counts = {}
    for v in values:
        if v != "":
            counts[v] = counts.get(v, 0) + 1
    if not counts:
        return []
    max_count = max(counts.values())
    return sorted((k for k, c in counts.items() if c == max_count), key=lambda s: s.encode())


def nunique_all_loop(numeric, strings):
    """functions.rs:4120-4139: `numeric` = {name: f64 values}, `strings` = {name: strings} for the other columns."""
    result = {}
    for name, vals in numeric.items():
        result[name] = len({to_bits(v) for v in vals if v == v})
    for name, vals in strings.items():
        result[name] = len(set(vals))
    return result


def is_unique_loop(values):
    """functions.rs:4226-4241, the numeric branch."""
    unique = {to_bits(v) for v in values if v == v}
    return len(unique) == sum(1 for v in values if v == v)


def mode_with_count_loop(values):
    """functions.rs:4243-4259.  Iterator::max_by_key returns the LAST maximum in iteration (here: insertion) order; the
    reference iterates in HashMap order, so among equal counts its answer is arbitrary."""
    counts = {}
    for v in values:
        if v == v:
            counts[to_bits(v)] = counts.get(to_bits(v), 0) + 1
    if not counts:
        return (math.nan, 0)
    best = None
    for bits, c in counts.items():
        if best is None or c >= best[1]:
            best = (bits, c)
    return (from_bits(best[0]), best[1])


def deterministic(values):
    """True where the reference's answers do not depend on HashMap order: at most one NaN payload, no -0.0 / 0.0 pair."""
    bits = {to_bits(v) for v in values}
    nans = {b for b in bits if from_bits(b) != from_bits(b)}
    return len(nans) <= 1 and not (to_bits(0.0) in bits and to_bits(-0.0) in bits)


def count_ties(values):
    """True when two numbers share the largest count (mode_with_count is then arbitrary in the reference)."""
    counts = {}
    for v in values:
        if v == v:
            counts[to_bits(v)] = counts.get(to_bits(v), 0) + 1
    return bool(counts) and list(counts.values()).count(max(counts.values())) > 1


# ---- 2. the device contract ---------------------------------------------------------------------------------------------
def cells_of(data, dtype, n_rows=None):
    """A column's data as the uint64 cells of the contract: the i64, the f64 bits, the code, 0 / 1."""
    data = np.asarray(data)
    if dtype == I64:
        return data.astype(np.int64, copy=False).view(np.uint64)
    if dtype == F64:
        return data.astype(np.float64, copy=False).view(np.uint64)
    if dtype == U32CODE:
        return data.astype(np.uint64)
    return np.unpackbits(data.astype(np.uint8, copy=False), bitorder="little")[:n_rows].astype(np.uint64)


def null_of(mask, n_rows):
    if mask is None:
        return np.zeros(n_rows, bool)
    return np.unpackbits(np.asarray(mask, np.uint8), bitorder="little")[:n_rows].astype(bool)


def image_of(cells, dtype):
    """Unsigned, ascending in the contract's value order."""
    if dtype == I64:
        return cells ^ SIGN
    if dtype == F64:
        return np.where(cells >> np.uint64(63), ~cells, cells | SIGN)
    return cells


def cells_of_image(image, dtype):
    if dtype == I64:
        return image ^ SIGN
    if dtype == F64:
        return np.where(image >> np.uint64(63), image & ~SIGN, ~image)
    return image


def distinct(data, dtype, null=None, order=BY_VALUE, code_rank=None, n_rows=None):
    """-> (values uint64, flags uint8, counts int64, info dict): include/pandrs_hip.h's list for the column.  `null`: a bool
    array (True = null) or None; the cells under it are never looked at."""
    cells = cells_of(data, dtype, n_rows)
    n = cells.shape[0]
    null = np.zeros(n, bool) if null is None else np.asarray(null, bool)[:n]
    number = ~null
    n_nan = 0
    if dtype == F64:
        nan = number & ((cells & ~SIGN) > np.uint64(0x7FF0000000000000))
        n_nan = int(nan.sum())
        number &= ~nan
    n_null = int(null.sum())
    image, counts = np.unique(image_of(cells[number], dtype), return_counts=True)
    values = cells_of_image(image, dtype)
    if dtype == U32CODE and code_rank is not None:
        by = np.argsort(np.asarray(code_rank, np.uint32)[values.astype(np.int64)], kind="stable")
        values, counts = values[by], counts[by]
    flags = np.zeros(values.shape[0], np.uint8)
    counts = counts.astype(np.int64)
    max_count = int(counts.max()) if counts.size else 0
    n_modes = int((counts == max_count).sum()) if counts.size else 0
    if n_nan:
        values, flags, counts = np.append(values, CANON_NAN), np.append(flags, np.uint8(NAN)), np.append(counts, np.int64(n_nan))
    if n_null:
        values, flags, counts = np.append(values, np.uint64(0)), np.append(flags, np.uint8(NULL)), np.append(counts, np.int64(n_null))
    if order == BY_COUNT:
        by = np.argsort(-counts, kind="stable")
        values, flags, counts = values[by], flags[by], counts[by]
    info = {"n_entries": int(values.shape[0]), "n_valid": int(number.sum()), "nan_count": n_nan, "null_count": n_null,
            "max_count": max_count, "n_modes": n_modes}
    return values.astype(np.uint64), flags.astype(np.uint8), counts.astype(np.int64), info


def direct_possible(data, dtype, null=None, n_rows=None, max_cells=8192):
    """Whether the contract's direct path applies (info.path == 1 under "distinct_path" 0 / 1): the numbers span at most
    max_cells cells; F64 only when every number is integral with |v| <= 2^53 and no -0.0 is present."""
    cells = cells_of(data, dtype, n_rows)
    n = cells.shape[0]
    number = np.ones(n, bool) if null is None else ~np.asarray(null, bool)[:n]
    if dtype == F64:
        number &= ~((cells & ~SIGN) > np.uint64(0x7FF0000000000000))
    c = cells[number]
    if c.size == 0:
        return True
    if dtype == F64:
        v = c.view(np.float64)
        if (c == SIGN).any() or not (np.abs(v) <= 2.0 ** 53).all() or (v != np.trunc(v)).any():
            return False
        lo, hi = int(v.min()), int(v.max())
    elif dtype == I64:
        lo, hi = int(c.view(np.int64).min()), int(c.view(np.int64).max())
    else:
        lo, hi = int(c.min()), int(c.max())
    return hi - lo + 1 <= max_cells


class Stand:
    """Context.distinct answered by the twin, and a record of the calls: the mirrors' CPU stand-in."""
    device = 0

    def __init__(self):
        self.calls = []

    def distinct(self, col, n_rows, order, code_rank=None, out_device=False):
        data, mask, dtype = col
        self.calls.append(("distinct", dtype, n_rows, order, code_rank is not None))
        v, f, k, info = distinct(np.asarray(data) if dtype == BOOLBITS else np.asarray(data)[:n_rows], dtype, null_of(mask, n_rows) if mask is not None else None,
                                 order, code_rank, n_rows)
        info["path"] = 0
        return v, f, k, info
