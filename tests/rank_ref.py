"""Two restatements of PandasCompatExt::rank (reference src/dataframe/pandas_compat/functions.rs:193-236) under the C ABI's
documented deviations (include/pandrs_hip.h): NaN and null cells are taken out first and get rank NaN, the m others rank
1 .. m; Int64 cells are compared as integers.

rank_naive follows the reference line for line (stable sort, the two `while` walks, the separate dense walk) over Python
values; rank_ref is the vectorised numpy version for larger inputs.  tests/test_rank_ref.py holds them bit-equal.
rank_features is the bookkeeping of the randomised sweep: which special paths an input reaches."""
import numpy as np

AVERAGE, MIN, MAX, FIRST, DENSE = range(5)
METHODS = (AVERAGE, MIN, MAX, FIRST, DENSE)


def _rankable(values, nulls):
    values = np.asarray(values)
    keep = np.ones(values.shape[0], bool) if nulls is None else ~np.asarray(nulls, bool)
    if values.dtype.kind == "f":
        keep &= ~np.isnan(values)
    return keep


def rank_naive(values, nulls, method):
    """functions.rs:193-236 in Python.  `values`: int64 or float64 array, `nulls`: bool array or None."""
    values = np.asarray(values)
    keep = _rankable(values, nulls)
    is_int = values.dtype.kind == "i"
    # :194-196  (row, value) pairs of the rankable cells; Int64 as Python ints, Float64 as Python floats (-0.0 == 0.0)
    indexed_values = [(int(i), int(values[i]) if is_int else float(values[i])) for i in np.flatnonzero(keep)]
    indexed_values.sort(key=lambda iv: iv[1])                   # :197  slice::sort_by is stable, as is list.sort
    ranks = [float("nan")] * values.shape[0]                    # :198
    i = 0
    while i < len(indexed_values):                              # :200
        j = i
        while j < len(indexed_values) and indexed_values[j][1] == indexed_values[i][1]:   # :202
            j += 1
        if method == AVERAGE:                                   # :205-211
            rank = float(i + j + 1) / 2.0
        elif method == MIN:
            rank = float(i + 1)
        elif method == MAX:
            rank = float(j)
        else:
            rank = 0.0
        for k in range(i, j):                                   # :212-219
            idx = indexed_values[k][0]
            ranks[idx] = float(k + 1) if method == FIRST else rank
        i = j
    if method == DENSE:                                         # :222-234
        dense_rank = 0.0
        i = 0
        while i < len(indexed_values):
            dense_rank += 1.0
            j = i
            while j < len(indexed_values) and indexed_values[j][1] == indexed_values[i][1]:
                ranks[indexed_values[j][0]] = dense_rank
                j += 1
            i = j
    return np.array(ranks, np.float64)


def _sorted_runs(values, nulls):
    """-> (rows in ascending stable order of the rankable cells, start flag per sorted position)."""
    values = np.asarray(values)
    rows = np.flatnonzero(_rankable(values, nulls))
    v = values[rows]
    if v.dtype.kind == "f":
        v = v + 0.0                                             # canonical key: -0.0 -> 0.0
    order = np.argsort(v, kind="stable")
    sv = v[order]
    start = np.ones(sv.shape[0], bool)
    start[1:] = sv[1:] != sv[:-1]
    return rows[order], start


def rank_ref_all(values, nulls):
    """-> [ranks under AVERAGE, MIN, MAX, FIRST, DENSE] from one sort."""
    values = np.asarray(values)
    rows, start = _sorted_runs(values, nulls)
    m = rows.shape[0]
    pos = np.arange(m, dtype=np.int64)
    s = np.maximum.accumulate(np.where(start, pos, 0))                                  # the run's start
    nxt = np.append(np.where(start, pos, m)[1:], m)[:m]                                 # a start after this position, else m
    e = np.minimum.accumulate(nxt[::-1])[::-1]                                          # the run's end
    outs = []
    for r in ((s + e + 1).astype(np.float64) / 2.0, (s + 1).astype(np.float64), e.astype(np.float64),
              (pos + 1).astype(np.float64), np.cumsum(start).astype(np.float64)):
        out = np.full(values.shape[0], np.nan, np.float64)
        out[rows] = r
        outs.append(out)
    return outs


def rank_ref(values, nulls, method):
    return rank_ref_all(values, nulls)[method]


def _sortable(values):
    """The order-preserving unsigned image of every cell, as the sort encodes it (uint64)."""
    values = np.asarray(values)
    if values.dtype.kind == "i":
        return values.view(np.uint64) ^ np.uint64(1 << 63)
    b = (values + 0.0).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def rank_features(values, nulls, tile):
    """Which special paths the input reaches: a tie run over more than one tile of `tile` sorted positions, the sort's
    zero-pass case (every code equal), a code wider than 64 bits, a NaN block, a null block."""
    values = np.asarray(values)
    n = values.shape[0]
    null = np.zeros(n, bool) if nulls is None else np.asarray(nulls, bool)
    nan = ~null & np.isnan(values) if values.dtype.kind == "f" else np.zeros(n, bool)
    rows, start = _sorted_runs(values, nulls)
    m = rows.shape[0]
    feats = set()
    if m:
        s = np.flatnonzero(start)
        e = np.append(s[1:], m)
        if ((e - 1) // tile != s // tile).any():
            feats.add("multi-tile run")
        img = _sortable(values[rows])
        span = int(img.max()) - int(img.min())
    else:
        s, span = np.empty(0, np.int64), 0
    if n and len(s) + int(nan.any()) + int(null.any()) == 1:
        feats.add("zero-pass sort")
    if span + int(nan.any()) + int(null.any()) >= 1 << 64:
        feats.add("two-word code")
    if nan.any():
        feats.add("NaN block")
    if null.any():
        feats.add("null block")
    return feats


FEATURES = ("multi-tile run", "zero-pass sort", "two-word code", "NaN block", "null block")
SWEEP_SEED, SWEEP_CASES = 20240, 300


def sweep_cases(seed=SWEEP_SEED, count=SWEEP_CASES):
    """The randomised sweep's inputs, from one seeded stream: (values, nulls or None, method, sort_digit_bits) with the dtype,
    the row count (under 20 000; half the cases log-uniform, so that small counts are as likely as large ones), the value
    range's width (1 bit to the full 64; a full-range Int64 column holds both extremes), the NaN and null shares (0, 1 %,
    50 %, 100 %) and the method drawn."""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(np.exp(rng.uniform(0.0, np.log(20_000.0)))) if rng.integers(0, 2) else int(rng.integers(1, 20_000))
        is_int = bool(rng.integers(0, 2))
        width = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 53, 54, 63, 64, 64)[int(rng.integers(0, 16))]
        raw = rng.integers(0, 2**64, n, dtype=np.uint64) >> np.uint64(64 - width)
        if is_int:
            values = (raw - np.uint64((1 << (width - 1)) if rng.integers(0, 2) else 0)).view(np.int64)   # centred on 0, or from 0 up
            if width == 64 and n >= 2:
                values[rng.choice(n, 2, replace=False)] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max]
        else:
            values = raw.view(np.float64).copy() if width == 64 else raw.astype(np.float64) - float(rng.integers(0, 2)) * 2.0 ** (width - 1)
            values[np.isnan(values)] = 1.0
            share = (0.0, 0.0, 0.01, 0.5, 1.0)[int(rng.integers(0, 5))]
            values[rng.random(n) < share] = np.nan
        share = (0.0, 0.0, 0.01, 0.5, 1.0)[int(rng.integers(0, 5))]
        nulls = rng.random(n) < share if share else None
        yield values, nulls, int(rng.integers(0, 5)), (0, 4, 5, 6, 7, 8)[int(rng.integers(0, 6))]
