"""Closed-form inputs and answers for the column ops at any row count, on any device: plain torch, never a call into the library.

Every generator takes the column length `n`, a `pivot` row around which its structure is placed (2^31 on the device, a few
thousand on the CPU) and the torch device.  It builds its columns in chunks of CH rows into preallocated tensors (`column` ->
a (data, null bitmap or None, dtype) triple, and `nulls_at(rows)` -> the null flags the bitmap packs), names the calls to make
(`calls`) and answers each of them for ANY subset of rows from arithmetic on the row number (`expected(call, rows)`): nothing is
sorted, nothing is read back from the column.  tests/test_big_ref.py holds every closed form against the op's numpy twin on
the materialised column at small sizes; tests/test_gpu_column_ops_beyond_2g.py holds the library against the closed forms."""
import math

import torch

CH = 1 << 28                                        # rows per generation chunk (a multiple of 8: bitmaps split on bytes)
I64, F64 = 0, 1                                     # pandrs_hip_dtype
AVERAGE, MIN_RANK, MAX_RANK, FIRST, DENSE = range(5)          # pandrs_hip_rank_method
FFILL, BFILL, LINEAR, VALUE = range(4)              # pandrs_hip_fill_method
SUM, PROD, MAX, MIN, COUNT = range(5)               # pandrs_hip_cum_op
SHIFT, DIFF, PCT_CHANGE = range(3)                  # pandrs_hip_lag_op
NAN = float("nan")
MUL, MOD = 7919, 1021                               # the scramble of the existing big-row tests: ((i * 7919) % 1021) - 510


# ---- chunked building blocks -----------------------------------------------------------------------------------------------
def arange(lo, hi, device):
    return torch.arange(lo, hi, dtype=torch.int64, device=device)


def fill(out, fn, ch=CH):
    """out[lo:hi] = fn(arange(lo, hi)), chunk by chunk"""
    for lo in range(0, out.numel(), ch):
        hi = min(lo + ch, out.numel())
        out[lo:hi] = fn(arange(lo, hi, out.device))
    return out


def pack_bits(n, fn, device, ch=CH):
    """The LSB-first bitmap of ceil(n / 8) bytes whose bit i is fn(i) (rows past n: 0)."""
    bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=device)
    for lo in range(0, n, ch):
        hi = min(lo + ch, n)
        f = fn(arange(lo, hi, device)).to(torch.uint8)
        if f.numel() % 8:
            f = torch.cat([f, torch.zeros(8 - f.numel() % 8, dtype=torch.uint8, device=device)])
        f = f.view(-1, 8)
        b = f[:, 0].clone()
        for j in range(1, 8):
            b += f[:, j] * (1 << j)
        bits[lo // 8:(hi + 7) // 8] = b
    return bits


def bits_at(bits, rows):
    """bit `rows` of an LSB-first bitmap -> bool"""
    return ((bits[rows >> 3].to(torch.int64) >> (rows & 7)) & 1).bool()


def sample_rows(n, pivot, device, extra=(), m=1_000_000, stride=7_919_333, halo=64):
    """The rows a sampled comparison reads: the first and last m, 2 m centred on the pivot, `halo` rows around every structural
    row in `extra`, and a stride over everything.  Ascending, unique."""
    spans = [(0, m), (pivot - m, pivot + m), (n - m, n)] + [(int(r) - halo, int(r) + halo) for r in extra]
    parts = [arange(max(a, 0), min(b, n), device) for a, b in spans if min(b, n) > max(a, 0)]
    parts.append(torch.arange(0, n, stride, dtype=torch.int64, device=device))
    return torch.unique(torch.cat(parts))


def scramble(i):
    """(i * 7919) mod 1021, as int64"""
    return (i * MUL) % MOD


def small(i):
    return scramble(i) - 510


def trend(i):
    """A bijection of the row numbers that stays exact in f64: the scramble inside every block of 1021 rows, blocks ascending."""
    return scramble(i) + MOD * (i // MOD)


def same(got, want):
    """NaN in the same places and equal values elsewhere (tensors of one dtype)."""
    if got.dtype.is_floating_point:
        gn, wn = torch.isnan(got), torch.isnan(want)
        return bool((gn == wn).all()) and bool((got[~gn] == want[~wn]).all())
    return bool((got == want).all())


def first_bad(got, want, rows):
    if got.dtype.is_floating_point:
        bad = (torch.isnan(got) != torch.isnan(want)) | (~torch.isnan(want) & (got != want))
    else:
        bad = got != want
    j = int(bad.nonzero()[0])
    return "%d of %d rows differ, first at row %d: got %r, expected %r" % (int(bad.sum()), bad.numel(), int(rows[j]), got[j].item(), want[j].item())


# ---- rank ------------------------------------------------------------------------------------------------------------------
class Rank:
    """x_i = i mod M (I64 or F64) over rows [0, m); then, for F64, NAN_TAIL rows of NaN; then NULL_TAIL null rows: m < n and, with
    the pivot below m, m > pivot.  The m numbers sort into M tie runs, value v in sorted positions [S_v, S_v + c_v), its rows in row
    order; with M = 3 a run straddles sorted position `pivot`."""
    NAN_TAIL, NULL_TAIL = 3000, 4000
    calls = (AVERAGE, MIN_RANK, MAX_RANK, FIRST, DENSE)

    def __init__(self, n, pivot, device, M=3, f64=False):
        self.n, self.pivot, self.device, self.M, self.f64 = n, pivot, device, M, f64
        self.first_null = n - self.NULL_TAIL
        self.m = self.first_null - (self.NAN_TAIL if f64 else 0)
        assert pivot < self.m < n, "the rankable rows must reach past the pivot"
        self.dtype = F64 if f64 else I64

    def nulls_at(self, rows):
        return rows >= self.first_null

    def values_at(self, rows):
        v = rows % self.M
        if not self.f64:
            return v
        return torch.where((rows >= self.m) & (rows < self.first_null), NAN, v.to(torch.float64))

    def column(self):
        data = fill(torch.empty(self.n, dtype=torch.float64 if self.f64 else torch.int64, device=self.device), self.values_at)
        return data, pack_bits(self.n, self.nulls_at, self.device), self.dtype

    def structural_rows(self):
        """the rows at both ends of every tie run (M = 3), and the first unrankable ones"""
        ends = [v for v in range(min(self.M, 3))] + [self.m - 1 - v for v in range(min(self.M, 3))]
        return ends + [self.m, self.first_null]

    def expected(self, method, rows):
        M, m = self.M, self.m
        v = rows % M
        c = (m - v + M - 1) // M                                     # rows i < m with i mod M == v
        S = v * (m // M) + torch.clamp(v, max=m % M)                 # ... with i mod M < v: the run's first sorted position
        if method == AVERAGE:
            r = (2 * S + c + 1).to(torch.float64) * 0.5              # S_v + (c_v + 1) / 2
        elif method == MIN_RANK:
            r = (S + 1).to(torch.float64)
        elif method == MAX_RANK:
            r = (S + c).to(torch.float64)
        elif method == FIRST:
            r = (S + rows // M + 1).to(torch.float64)
        else:
            r = (v + 1).to(torch.float64)
        return torch.where(rows >= m, NAN, r)


# ---- fill ------------------------------------------------------------------------------------------------------------------
class Fill:
    """Values ((i * 7919) % 1021) - 510.  A row is valid iff i % period == 0 (period 4099: every gap is longer than a tile of the
    fill kernels), except row 0 (a leading gap), the rows of one long hole [pivot - before, pivot + after) and the last `tail`
    rows (a trailing gap).  F64: the invalid cells are NaN, no mask.  I64: every cell holds its value, the mask marks the invalid."""
    calls = (FFILL, BFILL, LINEAR, VALUE)

    def __init__(self, n, pivot, device, f64=True, period=4099, hole=(3_000_000, 1_000_000), tail=5000):
        self.n, self.pivot, self.device, self.f64, self.P = n, pivot, device, f64, period
        self.h0, self.h1 = max(pivot - hole[0], 0), min(pivot + hole[1], n)
        self.end = n - tail                                          # the first row of the trailing gap
        self.dtype = F64 if f64 else I64
        self.value = -7.5 if f64 else -77
        one = torch.zeros(1, dtype=torch.int64, device=device)
        q, has = self._next(one)
        self.first_valid = int(q) if bool(has) else None
        p, has = self._prev(one + (n - 1))
        self.last_valid = int(p) if bool(has) else None
        assert self.first_valid is not None and self.first_valid < self.h0 and self.last_valid >= self.h1, "valid rows on both sides of the hole"

    def valid_at(self, rows):
        return (rows % self.P == 0) & (rows != 0) & ~((rows >= self.h0) & (rows < self.h1)) & (rows < self.end)

    def nulls_at(self, rows):
        return ~self.valid_at(rows)

    def column(self):
        if self.f64:
            data = fill(torch.empty(self.n, dtype=torch.float64, device=self.device),
                        lambda i: torch.where(self.valid_at(i), small(i).to(torch.float64), NAN))
            return data, None, F64
        data = fill(torch.empty(self.n, dtype=torch.int64, device=self.device), small)
        return data, pack_bits(self.n, self.nulls_at, self.device), I64

    def structural_rows(self):
        P = self.P
        return [self.first_valid, self.h0 - 1, self.h0, ((self.h0 - 1) // P) * P, self.h1 - 1, self.h1, ((self.h1 + P - 1) // P) * P,
                self.last_valid, self.end]

    def _prev(self, rows):
        """the last valid row at or before each row, and whether there is one"""
        P = self.P
        p = (torch.clamp(rows, max=self.end - 1) // P) * P
        p = torch.where((p >= self.h0) & (p < self.h1), ((self.h0 - 1) // P) * P if self.h0 > 0 else 0, p)
        return p, p > 0

    def _next(self, rows):
        P = self.P
        q = ((torch.clamp(rows, min=1) + P - 1) // P) * P
        q = torch.where((q >= self.h0) & (q < self.h1), ((self.h1 + P - 1) // P) * P, q)
        return q, q < self.end

    def expected(self, method, rows):
        """-> (cells, still missing)"""
        miss = ~self.valid_at(rows)
        x = small(rows)
        as_f = self.f64 or method == LINEAR
        gone_cell = NAN if as_f else 0
        if as_f:
            x = x.to(torch.float64)
        if method == VALUE:
            return torch.where(miss, self.value, x), torch.zeros_like(miss)
        p, has_p = self._prev(rows)
        q, has_n = self._next(rows)
        if method == FFILL:
            gone, out = miss & ~has_p, small(p)
        elif method == BFILL:
            gone, out = miss & ~has_n, small(q)
        else:                                                        # the reference's expression in the reference's order
            gone = miss & ~(has_p & has_n)
            a, b = small(p).to(torch.float64), small(q).to(torch.float64)
            den = torch.where(q > p, q - p, 1).to(torch.float64)
            out = a + ((b - a) * (rows - p).to(torch.float64)) / den
        out = torch.where(miss, out.to(x.dtype), x)
        return torch.where(gone, gone_cell, out), gone

    def missing(self, method):
        lead, trail = self.first_valid, self.n - 1 - self.last_valid
        return {FFILL: lead, BFILL: trail, LINEAR: lead + trail, VALUE: 0}[method]


# ---- describe / quantiles / topk / arg_extreme: a three-valued column and a ramp ------------------------------------------------
class Ordered:
    """kind "tri": x_i = i mod 3 - 1 as F64 (with n = 0 mod 3 the mean is exactly 0); kind "ramp": x_i = i as I64.  The sorted
    column and the stable order are closed forms: value class v = i mod 3 holds the rows v, v + 3, ... in row order."""

    def __init__(self, n, pivot, device, kind):
        assert kind in ("tri", "ramp")
        self.n, self.pivot, self.device, self.kind = n, pivot, device, kind
        self.dtype = F64 if kind == "tri" else I64
        self.c = [(n - v + 2) // 3 for v in range(3)]                # rows with i mod 3 == v
        idx = pivot - 0.5
        self.p_straddle = 100.0 * idx / (n - 1)                      # a percentile whose lower / upper ranks are pivot - 1 / pivot
        index = (self.p_straddle / 100.0) * float(n - 1)
        assert math.floor(index) == pivot - 1 and math.ceil(index) == pivot
        self.percentiles = [0.0, 25.0, 50.0, 75.0, 100.0, self.p_straddle]
        self.ks = sorted({1, min(1_000_000, n), min(pivot + 5, n)})

    def nulls_at(self, rows):
        return torch.zeros_like(rows, dtype=torch.bool)

    def values_at(self, rows):
        return (rows % 3 - 1).to(torch.float64) if self.kind == "tri" else rows

    def column(self):
        return fill(torch.empty(self.n, dtype=torch.float64 if self.kind == "tri" else torch.int64, device=self.device), self.values_at), None, self.dtype

    def sorted_at(self, k):
        """the k-th smallest cell as f64 (a Python float)"""
        if self.kind == "ramp":
            return float(k)
        return -1.0 if k < self.c[0] else (0.0 if k < self.c[0] + self.c[1] else 1.0)

    def percentile(self, p):
        """stats/descriptive.rs:169-200 over sorted_at, operation by operation (Python floats are IEEE doubles)"""
        n = self.n
        if p == 0.0:
            return self.sorted_at(0)
        if p == 100.0:
            return self.sorted_at(n - 1)
        index = (p / 100.0) * float(n - 1)
        lower, upper = int(math.floor(index)), int(math.ceil(index))
        if lower == upper:
            return self.sorted_at(lower)
        weight = index - float(lower)
        return self.sorted_at(lower) * (1.0 - weight) + self.sorted_at(upper) * weight

    def describe(self):
        """-> the eight values, and the mean of |x| (the scale of the mean's tolerance)"""
        n = self.n
        if self.kind == "tri":
            mean = (self.c[2] - self.c[0]) / n
            ssq = self.c[0] * (-1.0 - mean) ** 2 + self.c[1] * mean ** 2 + self.c[2] * (1.0 - mean) ** 2
            std, scale = math.sqrt(ssq / (n - 1)), (self.c[0] + self.c[2]) / n
        else:
            mean, std, scale = (n - 1) / 2.0, math.sqrt(n * (n + 1) / 12.0), (n - 1) / 2.0
        return {"count": n, "mean": mean, "std": std, "min": self.sorted_at(0), "q1": self.percentile(25.0), "median": self.percentile(50.0),
                "q3": self.percentile(75.0), "max": self.sorted_at(n - 1)}, scale

    def topk_rows(self, largest, pos):
        """the row at position `pos` (a tensor) of the column's descending / ascending stable order"""
        if self.kind == "ramp":
            return self.n - 1 - pos if largest else pos
        order = (2, 1, 0) if largest else (0, 1, 2)
        start, out = 0, torch.zeros_like(pos)
        for v in order:
            inside = (pos >= start) & (pos < start + self.c[v])
            out = torch.where(inside, v + 3 * (pos - start), out)
            start += self.c[v]
        return out

    def arg_extreme(self):
        """(the first row of the minimum, the last row of the maximum)"""
        n = self.n
        if self.kind == "ramp":
            return 0, n - 1
        return 0, n - 1 - ((n - 1 - 2) % 3)                         # the last row with i mod 3 == 2


# ---- window_quantile -------------------------------------------------------------------------------------------------------------
class RollingMedian:
    """x = trend(i) as F64: all distinct, exact.  A rolling median is recomputed from the w neighbours of the asked rows (the
    closed form of the column, torch.sort over [rows, w]); rows without a full window answer NaN (min_periods = w)."""

    def __init__(self, n, pivot, device, direct_max=44):
        self.n, self.pivot, self.device, self.dtype = n, pivot, device, F64
        self.calls = (("direct", 3), ("direct", direct_max), ("general", 3))

    def nulls_at(self, rows):
        return torch.zeros_like(rows, dtype=torch.bool)

    def column(self):
        return fill(torch.empty(self.n, dtype=torch.float64, device=self.device), lambda i: trend(i).to(torch.float64)), None, F64

    def expected(self, w, rows):
        nb = rows.unsqueeze(1) - torch.arange(w - 1, -1, -1, dtype=torch.int64, device=rows.device).unsqueeze(0)
        s = torch.sort(trend(torch.clamp(nb, min=0)).to(torch.float64), dim=1).values
        med = s[:, w // 2] if w % 2 else (s[:, w // 2 - 1] + s[:, w // 2]) / 2.0
        return torch.where(rows >= w - 1, med, NAN)


class ExpandingMedian:
    """x_i = i as F64: the median of 0 .. i is i / 2 exactly."""

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device, self.dtype = n, pivot, device, F64

    def nulls_at(self, rows):
        return torch.zeros_like(rows, dtype=torch.bool)

    def column(self):
        return fill(torch.empty(self.n, dtype=torch.float64, device=self.device), lambda i: i.to(torch.float64)), None, F64

    def expected(self, rows):
        return rows.to(torch.float64) / 2.0


# ---- eval ------------------------------------------------------------------------------------------------------------------------
class Eval:
    """Value program over a (I64), b (I64) and c (F64, null where i mod 10 == 3): where(a > b, a * b + c, clip(c, LO, HI)), small
    integers, so every operation is exact.  A null c gives NaN under a * b + c (null bit set) and LO under the clip.
    Mask program over r_i = i (I64): (r > lo and r < hi) or r mod 1021 == 7, a run across the pivot plus a periodic pattern."""
    LO, HI = -50.0, 50.0
    RUN = (1000, 2001)                                               # the run holds the rows pivot - 1000 < r < pivot + 2001
    VALUE_PROGRAM = [("COL", 0), ("COL", 1), ("GT", 0), ("COL", 0), ("COL", 1), ("MUL", 0), ("COL", 2), ("ADD", 0),
                     ("COL", 2), ("CONST", LO), ("MAX", 0), ("CONST", HI), ("MIN", 0), ("SELECT", 0)]

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device = n, pivot, device
        self.lo, self.hi = pivot - self.RUN[0], pivot + self.RUN[1]
        self.mask_program = [("COL", 0), ("CONST", float(self.lo)), ("GT", 0), ("COL", 0), ("CONST", float(self.hi)), ("LT", 0), ("AND", 0),
                             ("COL", 0), ("CONST", float(MOD)), ("REM", 0), ("CONST", 7.0), ("EQ", 0), ("OR", 0)]

    @staticmethod
    def a_at(i):
        return small(i)

    @staticmethod
    def b_at(i):
        return (i * 104_729) % 997 - 498

    @staticmethod
    def c_at(i):
        return ((i * 31) % 201 - 100).to(torch.float64)

    @staticmethod
    def c_null_at(i):
        return i % 10 == 3

    def value_columns(self):
        d, n = self.device, self.n
        return [(fill(torch.empty(n, dtype=torch.int64, device=d), self.a_at), None, I64),
                (fill(torch.empty(n, dtype=torch.int64, device=d), self.b_at), None, I64),
                (fill(torch.empty(n, dtype=torch.float64, device=d), self.c_at), pack_bits(n, self.c_null_at, d), F64)]

    def mask_columns(self):
        return [(fill(torch.empty(self.n, dtype=torch.int64, device=self.device), lambda i: i), None, I64)]

    def expected_values(self, rows):
        """-> (cells, null flags)"""
        a, b = self.a_at(rows).to(torch.float64), self.b_at(rows).to(torch.float64)
        cn = self.c_null_at(rows)
        c = torch.where(cn, NAN, self.c_at(rows))
        res = torch.where(a > b, a * b + c, torch.fmin(torch.fmax(c, torch.full_like(c, self.LO)), torch.full_like(c, self.HI)))
        return res, torch.isnan(res) & cn

    def expected_mask(self, rows):
        return ((rows > self.lo) & (rows < self.hi)) | (rows % MOD == 7)

    def structural_rows(self):
        return [self.lo, self.lo + 1, self.hi - 1, self.hi]


def count_true(n, fn, device, ch=CH):
    """the number of rows i < n with fn(i), by a chunked torch reduction"""
    return sum(int(fn(arange(lo, min(lo + ch, n), device)).sum()) for lo in range(0, n, ch))


# ---- isin ------------------------------------------------------------------------------------------------------------------------
class Isin:
    """x_i = i as I64.  "few": three listed values (the LDS set), one below the pivot, one above it, one the column never holds.
    "many": up to 10^5 values OFF + j * stride (the global set), spread over the whole column, and some beyond its last row."""
    OFF = 5

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device = n, pivot, device
        self.few = [7, pivot + 3, n + 11]
        self.n_many = min(100_000, n // 3)
        self.stride = n // (self.n_many - 50)                        # the last 50 or so values lie past row n - 1
        self.calls = (("few", False), ("many", False), ("many", True))

    def nulls_at(self, rows):
        return torch.zeros_like(rows, dtype=torch.bool)

    def column(self):
        return fill(torch.empty(self.n, dtype=torch.int64, device=self.device), lambda i: i), None, I64

    def values(self, which):
        if which == "few":
            return torch.tensor(self.few, dtype=torch.int64, device=self.device)
        return self.OFF + self.stride * arange(0, self.n_many, self.device)

    def expected(self, which, negate, rows):
        if which == "few":
            hit = (rows == self.few[0]) | (rows == self.few[1]) | (rows == self.few[2])
        else:
            d = rows - self.OFF
            hit = (d >= 0) & (d % self.stride == 0) & (d // self.stride < self.n_many)
        return hit != negate

    def count(self, which, negate):
        if which == "few":
            hits = sum(1 for v in self.few if 0 <= v < self.n)
        else:
            hits = min(self.n_many, (self.n - 1 - self.OFF) // self.stride + 1)
        return self.n - hits if negate else hits

    def structural_rows(self, which):
        if which == "few":
            return [v for v in self.few if v < self.n]
        j = (self.pivot - self.OFF) // self.stride
        return [self.OFF, self.OFF + j * self.stride, self.OFF + (j + 1) * self.stride, self.OFF + ((self.n - 1 - self.OFF) // self.stride) * self.stride]


class MaskedPredicate:
    """x_i = i as I64, null where i mod 10 == 3 (a null cell compares as NaN).  GT: the rows above pivot - 5 that are not null, a
    run across the pivot with a periodic pattern of holes; ISNA: the null rows."""
    GT, ISNA = 0, 8                                                  # pandrs_hip_predicate_op

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device = n, pivot, device
        self.t = pivot - 5
        self.calls = ((self.GT, float(self.t)), (self.ISNA, 0.0))

    def nulls_at(self, rows):
        return rows % 10 == 3

    def column(self):
        return fill(torch.empty(self.n, dtype=torch.int64, device=self.device), lambda i: i), pack_bits(self.n, self.nulls_at, self.device), I64

    def expected(self, op, rows):
        nl = self.nulls_at(rows)
        return nl if op == self.ISNA else (rows > self.t) & ~nl

    def count(self, op):
        below = lambda k: (k + 6) // 10                              # noqa: E731  null rows among 0 .. k - 1
        n, t = self.n, self.t
        return below(n) if op == self.ISNA else (n - 1 - t) - (below(n) - below(t + 1))


# ---- window: van Herk max, the expanding scans, EWM ----------------------------------------------------------------------------------
def _prefix_max_table(device):
    """pm[j] = max of (t * 7919) mod 1021 over t <= j, j < 1021"""
    return torch.cummax(scramble(arange(0, MOD, device)), 0).values


class Window:
    """Four columns, one call each (all F64):
      "scramble"  (i * 7919) mod 1021       rolling max, w = 3000: recomputed from the w neighbours of the asked rows
      "trend"     trend(i)                  rolling max, w = 3000, the same way; expanding max: 1021 (i div 1021) + the prefix
                                            maximum of the scramble inside the block, a record after every pivot
      "mod3"      i mod 3                   expanding sum: 3 q + (r == 2) with q, r = divmod(i + 1, 3); integers, so exact
      "bit"       i mod 2                   EWM mean, alpha = 0.5: (1 - 4^-k) / 3 at i = 2 k, (4 - 4^-k) / 6 at i = 2 k + 1"""
    W = 3000
    calls = (("scramble", "rolling_max"), ("trend", "rolling_max"), ("trend", "expanding_max"), ("mod3", "expanding_sum"), ("bit", "ewm_mean"))

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device, self.dtype = n, pivot, device, F64
        self.pm = _prefix_max_table(device)

    def nulls_at(self, rows):
        return torch.zeros_like(rows, dtype=torch.bool)

    def values_at(self, name, rows):
        v = {"scramble": scramble, "trend": trend, "mod3": lambda i: i % 3, "bit": lambda i: i % 2}[name](rows)
        return v.to(torch.float64)

    def column(self, name):
        return fill(torch.empty(self.n, dtype=torch.float64, device=self.device), lambda i: self.values_at(name, i)), None, F64

    def rolling_max(self, name, lo, hi):
        """rows [lo, hi): unfold over the column's closed form on [lo - w + 1, hi); NaN without a full window (min_periods = w)"""
        w = self.W
        rows = arange(lo, hi, self.device)
        x = self.values_at(name, torch.clamp(arange(lo - w + 1, hi, self.device), min=0))
        return torch.where(rows >= w - 1, x.unfold(0, w, 1).amax(1), NAN)

    def expected(self, name, what, rows):
        if what == "expanding_max":
            return (MOD * (rows // MOD) + self.pm[rows % MOD]).to(torch.float64)
        if what == "expanding_sum":
            q, r = (rows + 1) // 3, (rows + 1) % 3
            return (3 * q + (r == 2)).to(torch.float64)
        assert what == "ewm_mean"
        k = (rows // 2).to(torch.float64)
        t = torch.pow(torch.full_like(k, 4.0), -k)
        return torch.where(rows % 2 == 0, (1.0 - t) / 3.0, (4.0 - t) / 6.0)


# ---- cumulative / lag --------------------------------------------------------------------------------------------------------------
class Cumulative:
    """Columns (F64), each with the calls made on it:
      "trend"   trend(i): MAX (a record after every pivot)           "neg"     -trend(i): MIN, the mirror image
      "flip"    2, 0.5, 2, 0.5, ...: PROD = 2, 1, 2, 1, ... (exact, the exponent carries across every tile); PCT_CHANGE(1) = 3 at
                even rows, -0.75 at odd ones, NaN without a bit at row 0
      "masked"  i mod 3, null where i mod 10 == 3: SUM = 27 (i div 30) + the prefix inside the period of 30, NaN under a null bit;
                COUNT = (i + 1) - (i + 7) div 10
      "ramp"    i: SHIFT by pivot + 5, -(pivot + 5) and 1"""

    def __init__(self, n, pivot, device):
        self.n, self.pivot, self.device, self.dtype = n, pivot, device, F64
        self.pm = _prefix_max_table(device)
        i = arange(0, 30, device)
        self.t30 = torch.cumsum(torch.where(i % 10 == 3, 0, i % 3), 0)
        self.calls = {"trend": [("cum", MAX)], "neg": [("cum", MIN)], "flip": [("cum", PROD), ("lag", PCT_CHANGE, 1)],
                      "masked": [("cum", SUM), ("cum", COUNT)], "ramp": [("lag", SHIFT, pivot + 5), ("lag", SHIFT, -(pivot + 5)), ("lag", SHIFT, 1)]}

    def nulls_at(self, name, rows):
        return rows % 10 == 3 if name == "masked" else torch.zeros_like(rows, dtype=torch.bool)

    def values_at(self, name, rows):
        if name == "flip":
            return torch.where(rows % 2 == 0, 2.0, 0.5).to(torch.float64)
        v = {"trend": trend, "neg": lambda i: -trend(i), "masked": lambda i: i % 3, "ramp": lambda i: i}[name](rows)
        return v.to(torch.float64)

    def column(self, name, data=None):
        data = torch.empty(self.n, dtype=torch.float64, device=self.device) if data is None else data
        fill(data, lambda i: self.values_at(name, i))
        return data, (pack_bits(self.n, lambda i: self.nulls_at(name, i), self.device) if name == "masked" else None), F64

    def expected(self, name, call, rows):
        """-> (cells, null flags, total null count)"""
        none = torch.zeros_like(rows, dtype=torch.bool)
        n = self.n
        if call[0] == "cum":
            op = call[1]
            if op in (MAX, MIN):
                r = MOD * (rows // MOD) + self.pm[rows % MOD]
                return (r if op == MAX else -r).to(torch.float64), none, 0
            if op == PROD:
                return torch.where(rows % 2 == 0, 2.0, 1.0).to(torch.float64), none, 0
            nl = self.nulls_at(name, rows)
            if op == COUNT:
                return (rows + 1) - (rows + 7) // 10, none, 0
            s = (27 * (rows // 30) + self.t30[rows % 30]).to(torch.float64)
            return torch.where(nl, NAN, s), nl, (n - 3 + 9) // 10
        op, periods = call[1], call[2]
        if op == PCT_CHANGE:
            r = torch.where(rows % 2 == 0, 3.0, -0.75).to(torch.float64)
            return torch.where(rows == 0, NAN, r), none, 0
        src = rows - periods
        gone = (src < 0) | (src >= n)
        return torch.where(gone, NAN, src.to(torch.float64)), gone, min(abs(periods), n)
