"""The reference's sort comparator (src/optimized/split_dataframe/sort.rs:18-272) restated twice: Python's stable
`sorted` with functools.cmp_to_key (ref_cmp, for small inputs) and np.lexsort over encoded keys (ref_lexsort, stable too,
for larger ones).  Shared by tests/test_gpu_sort.py and experiments/fuzz_ops.py and checked against each other, without
a GPU, by tests/test_references.py.  NaN follows the header's documented rule (after every number, before nulls)."""
import functools
import math

import numpy as np

from pandrs_amd import _lib as L


# ---- columns: (engine triple, python values with None for null) ---------------------------------------------------
class Col:
    def __init__(self, dtype, values, nulls=None, strings=None):
        self.dtype, self.n = dtype, len(values)
        self.nulls = None if nulls is None else np.asarray(nulls, bool)
        self.strings = strings                      # U32CODE: the code -> string table
        if dtype == L.BOOLBITS:
            self.values = np.asarray(values, bool)
            self.data = np.packbits(self.values, bitorder="little")
        else:
            self.values = np.asarray(values, {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32}[dtype])
            self.data = self.values
        self.mask = None if self.nulls is None else np.packbits(self.nulls, bitorder="little")

    def triple(self):
        return (self.data, self.mask, self.dtype)

    def py(self, i):
        if self.nulls is not None and self.nulls[i]:
            return None
        v = self.values[i]
        if self.dtype == L.U32CODE:
            return self.strings[int(v)]
        if self.dtype == L.BOOLBITS:
            return bool(v)
        return int(v) if self.dtype == L.I64 else float(v)


def rank_of(strings):
    order = sorted(range(len(strings)), key=lambda c: strings[c].encode("utf-8"))
    r = np.empty(len(strings), np.uint32)
    r[order] = np.arange(len(strings), dtype=np.uint32)
    return r


def _cmp_one(a, b, asc):
    """sort.rs's per-type comparator: (None, _) => Greater before the direction; NaN: the header's rule."""
    if a is None and b is None:
        return 0
    if a is None:
        return 1
    if b is None:
        return -1
    an = isinstance(a, float) and math.isnan(a)
    bn = isinstance(b, float) and math.isnan(b)
    if an or bn:
        return 0 if an and bn else (1 if an else -1)
    if isinstance(a, str):
        a, b = a.encode("utf-8"), b.encode("utf-8")
    c = (a > b) - (a < b)
    return c if asc else -c


def ref_cmp(cols, asc):
    def cmp(i, j):
        for col, a in zip(cols, asc):
            c = _cmp_one(col.py(i), col.py(j), a)
            if c:
                return c
        return 0
    return np.array(sorted(range(cols[0].n), key=functools.cmp_to_key(cmp)), np.int64)


def ref_lexsort(cols, asc):
    keys = []
    for col, a in zip(cols, asc):
        v = col.values
        if col.dtype == L.U32CODE:
            v = rank_of(col.strings)[v].astype(np.int64)
        elif col.dtype == L.BOOLBITS:
            v = v.astype(np.int64)
        cls = np.zeros(col.n, np.int64)
        if col.dtype == L.F64:
            nan = np.isnan(v)
            cls[nan] = 1
            v = np.where(nan, 0.0, v) + 0.0             # (-0.0 + 0.0 == 0.0: one value)
        if col.nulls is not None:
            cls[col.nulls] = 2
        _, inv = np.unique(v, return_inverse=True)
        inv = np.where(cls > 0, 0, inv.astype(np.int64).reshape(-1))    # nulls tie, NaNs tie: the value plays no part
        keys.append((inv if a else -inv, cls))
    seq = []
    for inv, cls in reversed(keys):                     # np.lexsort: the LAST key is the primary one
        seq += [inv, cls]
    return np.lexsort(seq).astype(np.int64)


# codes in an order that differs from the strings' byte order: non-ASCII, empty, prefixes, case
STRINGS = ["zeta", "", "Émile", "alpha", "al", "ä", "Zulu", "alphabet", "日本", "a", "é", "e", "\U0001F600", "b b"]
