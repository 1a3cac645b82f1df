"""The column ops between 2^31 and 2^32 rows against the closed forms of tests/big_ref.py.

Every entry point written since the sort admits fewer than 2^32 rows per call and keeps row positions, tile carries, run starts,
histogram bins and wavelet ranks in 32-bit words.  One test per op; each runs, in order:
  1. its generator at 300 000 rows (pivot 150 000) through the engine, ALL rows compared: "wrong at any size";
  2. ONE size above 2^31, n = 2^31 + 12 345 (2^31 + 12 346 where the generator wants n = 0 mod 3), pivot = 2^31, the data built
     on the device in chunks of 2^28 rows and every call made once.  Where the closed form is a cheap elementwise expression
     (rank, cumulative / lag, eval, isin, predicate, top-k, the expanding scans, every bitmap) ALL rows are compared in chunks;
     elsewhere (fill, the rolling windows) the first and last 10^6 rows, 2 10^6 rows centred on the pivot, the generator's
     structural rows and a stride of 7 919 333 rows (the rolling maxima: 10^5 rows at either end, 10^5 before and 4096 after the
     pivot and 4096 rows every 79 193 330 - their reference reads w = 3000 cells per compared row);
  3. for the ops whose footprint is the column plus an output or less (describe, quantiles, arg_extreme, the mask outputs of eval
     and isin, fill VALUE, cumulative COUNT) one more call at n = 2^32 - 1, the largest admitted: the last 10^6 rows (eval, isin:
     every byte of the bitmap) and the scalars;
  4. test_2_pow_32_rows_are_refused: the entry points without such a test elsewhere refuse n = 2^32 with INVALID_ARGUMENT and a
     message naming 2^32, before they touch the data (the pointers they get are not dereferenceable for that many rows).
tests/test_big_ref.py proves the closed forms against the numpy twins on the CPU, so a failure here is the kernel's.

Peak device memory stays near or below 120 GB per test (the machines are shared).  rank and the top-k of more than a fifth of
the rows sit on the sort: the column, the output and the sort's workspace and permutation, 56.5 GB measured for rank at 2^30
rows and 117 / 118 GB for the two tests here.
Left out for the cap: the GENERAL path of window_quantile above 2^31 rows (rolling w = 3 through "window_quantile_path" 2, and
the expanding median): on top of the sort it reserves two rank buffers, the sorted cells and 34 bit vectors of 16 bytes per 64
rows - 85.4 GB of device memory measured for one call at 2^30 rows (column and output included), so about 171 GB at
2^31 + 12 345.  It runs at 300 000 rows here (step 1); its 32nd wavelet level (bit 31 of a rank) stays unexecuted until a test
may take that much.  The direct path runs at 2^31 + 12 345 rows with w = 3 and w = WQ_DIRECT_MAX.
fill runs at 2^31 + 2 012 345 rows: its hole ends 10^6 rows after 2^31 and valid rows must follow it, so that the carried
"last valid row + 1" itself passes 2^31.

Every test frees what it allocated and skips, with the numbers, when the device has less free memory than it needs plus 20 %;
each prints its wall time and peak device memory (the `mem` fixture of tests/test_gpu_rows_beyond_2g.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import big_ref as B
from tests.test_gpu_rows_beyond_2g import mem  # noqa: F401  (the fixture: a fresh context, the bookkeeping, the report)

pytestmark = pytest.mark.gpu

D = "cuda:0"
PIVOT = 1 << 31
N_BIG = (1 << 31) + 12_345
N_FILL = (1 << 31) + 2_012_345                       # valid rows on both sides of fill's hole [2^31 - 3 10^6, 2^31 + 10^6)
N_MAX = (1 << 32) - 1
N_SMALL, P_SMALL = 300_000, 150_000
CMP = 1 << 26                                        # rows per comparison chunk: torch's temporaries stay below a few GB
WQ_DIRECT_MAX = 44


def _L():
    from pandrs_amd import _lib as L
    return L


def _all_rows(got, want_of, n, what):
    """got[i] == want_of(rows)[i] for every row, chunk by chunk"""
    assert got.numel() == n, (what, got.numel(), n)
    for lo in range(0, n, CMP):
        rows = B.arange(lo, min(lo + CMP, n), D)
        g, w = got[lo:lo + rows.numel()], want_of(rows)
        assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
        assert B.same(g, w), "%s: %s" % (what, B.first_bad(g, w, rows))


def _at_rows(got, want_of, rows, what):
    g, w = got[rows], want_of(rows)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    assert B.same(g, w), "%s: %s" % (what, B.first_bad(g, w, rows))


def _bitmap(bits, n, flags_of, count, what):
    """every byte of an LSB-first bitmap (None: no bit is set), the bits past row n - 1 zero, and the count"""
    import torch
    if bits is None:
        assert count == 0, (what, count)
        bits = torch.zeros((n + 7) // 8, dtype=torch.uint8, device=D)
    assert bits.numel() == (n + 7) // 8, (what, bits.numel())
    step, seen = CMP // 8, 0
    for b0 in range(0, bits.numel(), step):
        b1 = min(b0 + step, bits.numel())
        rows = min(8 * b1, n) - 8 * b0
        want = B.pack_bits(rows, lambda i: flags_of(i + 8 * b0), D)
        got = bits[b0:b1]
        if not torch.equal(got, want):
            j = int((got != want).nonzero()[0])
            raise AssertionError("%s: byte %d (rows %d ..) is 0x%02X, expected 0x%02X" % (what, b0 + j, 8 * (b0 + j), int(got[j]), int(want[j])))
        seen += int(flags_of(B.arange(8 * b0, 8 * b0 + rows, D)).sum())
    assert seen == count, (what, seen, count)


def _program(named):
    L = _L()
    return [(getattr(L, "EVAL_" + name), arg) for name, arg in named]


def _release(mem):
    """everything this test holds, the context's arenas and torch's cached blocks"""
    mem.mark()
    mem.t.clear()
    mem.fresh()


# ---- rank --------------------------------------------------------------------------------------------------------------------
def _rank(mem, n, pivot, M, f64, methods):
    import torch
    g = B.Rank(n, pivot, D, M=M, f64=f64)
    mem["x"], mem["m"], dt = g.column()
    mem["out"] = torch.empty(n, dtype=torch.float64, device=D)
    for method in methods:
        got = mem.ctx.rank((mem["x"], mem["m"], dt), n, method, out=mem["out"])
        mem.mark()
        _all_rows(got, lambda rows: g.expected(method, rows), n, "rank %s M=%d method %d at %d rows" % ("F64" if f64 else "I64", M, method, n))
    del mem["x"], mem["m"], mem["out"]


def test_rank(mem):
    """x_i = i mod 3 (a tie run straddles sorted position 2^31) and i mod 1021, I64 and F64, a NaN block and a null block at the
    end (m < n, m > 2^31): every method against S_v, c_v and i div M, all rows.  With M = 2^19 the last two tie runs also START
    past sorted position 2^31 (the carried run starts themselves exceed 31 bits)."""
    for M, f64 in ((3, False), (3, True), (1021, True), (1021, False)):
        _rank(mem, N_SMALL, P_SMALL, M, f64, B.Rank.calls)
    mem.need(110)
    _rank(mem, N_BIG, PIVOT, 3, False, B.Rank.calls)
    _rank(mem, N_BIG, PIVOT, 3, True, B.Rank.calls)
    _rank(mem, N_BIG, PIVOT, 1021, True, (B.AVERAGE, B.DENSE))
    _rank(mem, N_BIG, PIVOT, 1 << 19, False, (B.AVERAGE, B.MIN_RANK, B.DENSE))      # runs of 4096 rows: the last two START past 2^31


# ---- fill --------------------------------------------------------------------------------------------------------------------
def _fill(mem, g, methods, rows):
    """rows None: all rows"""
    import torch
    n = g.n
    mem["x"], mem["m"], dt = g.column()
    mem["out"] = torch.empty(n, dtype=torch.int64, device=D)
    mem["om"] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=D)
    for method in methods:
        as_f = g.f64 or method == B.LINEAR
        got, mask, missing = mem.ctx.fill((mem["x"], mem["m"], dt), n, method, value=g.value if method == B.VALUE else None,
                                          out=mem["out"].view(torch.float64) if as_f else mem["out"], out_mask=mem["om"])
        mem.mark()
        what = "fill %s method %d at %d rows" % ("F64" if g.f64 else "I64", method, n)
        assert missing == g.missing(method), (what, missing, g.missing(method))
        if rows is None:
            _all_rows(got, lambda r: g.expected(method, r)[0], n, what)
        else:
            _at_rows(got, lambda r: g.expected(method, r)[0], rows, what)
        _bitmap(mask, n, lambda r: g.expected(method, r)[1], missing, what + " (mask)")
    del mem["x"], mem["m"], mem["out"], mem["om"]


def test_fill(mem):
    """Valid rows every 4099 (each gap spans tiles), a hole of 4 10^6 rows across 2^31, a leading and a trailing gap; F64 with NaN
    gaps and I64 with a mask, 2^31 + 2 012 345 rows: the rows of the hole past 2^31 are filled from 3 10^6 rows back, and after
    the hole the carried "last valid row + 1" is itself past 2^31.  VALUE again at 2^32 - 1 rows."""
    for f64 in (True, False):
        _fill(mem, B.Fill(N_SMALL, P_SMALL, D, f64=f64, hole=(30_000, 10_000)), B.Fill.calls, None)
    mem.need(45)
    for f64 in (True, False):
        g = B.Fill(N_FILL, PIVOT, D, f64=f64)
        assert g.h1 == PIVOT + 1_000_000 and g.last_valid > g.h1
        _fill(mem, g, B.Fill.calls, B.sample_rows(N_FILL, PIVOT, D, extra=g.structural_rows()))
    _release(mem)
    mem.need(75)
    g = B.Fill(N_MAX, PIVOT, D, f64=True)
    _fill(mem, g, (B.VALUE,), B.arange(N_MAX - 1_000_000, N_MAX, D))


# ---- describe / quantiles (and arg_extreme at the largest admitted size: the same columns) --------------------------------------
def _scalars(mem, g, col):
    n = g.n
    want, scale = g.describe()
    got = mem.ctx.describe(col, n)
    mem.mark()
    what = "describe %s at %d rows" % (g.kind, n)
    for f in ("count", "min", "q1", "median", "q3", "max"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert abs(got["mean"] - want["mean"]) <= 1e-9 * scale, (what, got["mean"], want["mean"])        # the rule of tests/describe_ref.py
    assert abs(got["std"] - want["std"]) <= 1e-9 * want["std"], (what, got["std"], want["std"])
    q, count = mem.ctx.quantiles(col, n, g.percentiles)
    assert count == n, (what, count)
    for p, v in zip(g.percentiles, q):
        assert v == g.percentile(p), ("quantiles %s at %d rows" % (g.kind, n), p, v, g.percentile(p))
    assert mem.ctx.arg_extreme(col, n) == g.arg_extreme(), ("arg_extreme %s at %d rows" % (g.kind, n), mem.ctx.arg_extreme(col, n), g.arg_extreme())


def test_describe_and_quantiles(mem):
    """i mod 3 - 1 (F64: every bin and prefix of the select holds hundreds of millions of rows, past 2^31 in all) and the ramp i
    (I64: eight varying digits); percentiles 0, 25, 50, 75, 100 and one whose two ranks are 2^31 - 1 and 2^31.  Again at 2^32 - 1
    rows, where a bin alone passes 2^30 and a prefix 2^31; arg_extreme answers on the same columns there."""
    for kind in ("tri", "ramp"):
        g = B.Ordered(N_SMALL, P_SMALL, D, kind)
        mem["x"] = g.column()[0]
        _scalars(mem, g, (mem["x"], None, g.dtype))
    mem.need(40)
    for kind, n in (("tri", N_BIG + 1), ("ramp", N_BIG), ("tri", N_MAX), ("ramp", N_MAX)):
        del mem["x"]
        g = B.Ordered(n, PIVOT, D, kind)
        assert kind != "tri" or n % 3 == 0
        mem["x"] = g.column()[0]
        _scalars(mem, g, (mem["x"], None, g.dtype))


# ---- topk / arg_extreme ------------------------------------------------------------------------------------------------------------
def _topk(mem, g, col):
    n = g.n
    for k in g.ks:
        for largest in (True, False):
            got, n_num = mem.ctx.topk(col, n, k, largest=largest)
            mem.mark()
            what = "topk %s k=%d %s at %d rows" % (g.kind, k, "largest" if largest else "smallest", n)
            assert n_num == k, (what, n_num)
            _all_rows(got, lambda pos: g.topk_rows(largest, pos), k, what)
            del got
    assert mem.ctx.arg_extreme(col, n) == g.arg_extreme(), ("arg_extreme %s at %d rows" % (g.kind, n),)


def test_topk_and_arg_extreme(mem):
    """The same two columns; k = 1, 10^6 and 2^31 + 5 (the threshold class is the tie run that straddles sorted position 2^31, cut
    by row order; the whole column is sorted), both directions.  The ramp's nlargest is n - 1, n - 2, ...: the rows past 2^31
    first."""
    for kind in ("tri", "ramp"):
        g = B.Ordered(N_SMALL, P_SMALL, D, kind)
        mem["x"] = g.column()[0]
        _topk(mem, g, (mem["x"], None, g.dtype))
    mem.need(110)
    for kind, n in (("tri", N_BIG + 1), ("ramp", N_BIG)):
        del mem["x"]
        g = B.Ordered(n, PIVOT, D, kind)
        if kind == "ramp":
            g.ks = [k for k in g.ks if k <= 1_000_000]           # all distinct: no tie run to cut; the large k ran on the other column
        mem["x"] = g.column()[0]
        _topk(mem, g, (mem["x"], None, g.dtype))
    assert int(g.topk_rows(True, B.arange(0, N_BIG - PIVOT, D)).min()) == PIVOT          # the ramp's first 12 345 answers lie past 2^31


# ---- window_quantile -----------------------------------------------------------------------------------------------------------------
def _rolling_median(mem, g, paths, rows):
    L = _L()
    n = g.n
    mem["x"] = g.column()[0]
    try:
        for path, w in g.calls:
            if path not in paths:
                continue
            mem.ctx.set_option("window_quantile_path", 1 if path == "direct" else 2)
            mem["got"] = mem.ctx.window_quantile((mem["x"], None, L.F64), n, L.WINDOW_KIND_ROLLING, median=True, window=w)
            what = "rolling median w=%d (%s path) at %d rows" % (w, path, n)
            if rows is None:
                _all_rows(mem["got"], lambda r: g.expected(w, r), n, what)
            else:
                for lo in range(0, rows.numel(), 1 << 20):       # [rows, w] neighbourhoods: a few hundred MB at a time
                    _at_rows(mem["got"], lambda r: g.expected(w, r), rows[lo:lo + (1 << 20)], what)
            del mem["got"]
    finally:
        mem.ctx.set_option("window_quantile_path", 0)
    del mem["x"]


def test_window_quantile(mem):
    """The rolling median of a bijective scramble of the row number, recomputed from the w neighbours of the compared rows: the
    direct path with w = 3 and w = WQ_DIRECT_MAX above 2^31 rows; the general path (w = 3, and the expanding median of the ramp,
    i / 2) at 300 000 rows only - see the module docstring for its footprint."""
    L = _L()
    g = B.RollingMedian(N_SMALL, P_SMALL, D, direct_max=WQ_DIRECT_MAX)
    _rolling_median(mem, g, ("direct", "general"), None)
    e = B.ExpandingMedian(N_SMALL, P_SMALL, D)
    mem["x"] = e.column()[0]
    got = mem.ctx.window_quantile((mem["x"], None, L.F64), N_SMALL, L.WINDOW_KIND_EXPANDING, median=True, min_periods=1)
    _all_rows(got, e.expected, N_SMALL, "expanding median at %d rows" % N_SMALL)
    del got, mem["x"]
    mem.need(45)
    g = B.RollingMedian(N_BIG, PIVOT, D, direct_max=WQ_DIRECT_MAX)
    _rolling_median(mem, g, ("direct",), B.sample_rows(N_BIG, PIVOT, D))


# ---- eval ------------------------------------------------------------------------------------------------------------------------------
def _eval_mask(mem, g):
    import torch
    n = g.n
    cols = g.mask_columns()
    mem["r"] = cols[0][0]
    mem["bits"] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=D)
    bits, count = mem.ctx.eval(cols, n, _program(g.mask_program), out=mem["bits"])
    mem.mark()
    what = "eval mask program at %d rows" % n
    periodic, both = (n - 8 + B.MOD) // B.MOD, sum(1 for r in range(g.lo + 1, g.hi) if r % B.MOD == 7)
    assert count == (g.hi - g.lo - 1) + periodic - both, (what, count)
    _bitmap(bits, n, g.expected_mask, count, what)
    del cols, bits, mem["r"], mem["bits"]


def test_eval(mem):
    """where(a > b, a * b + c, clip(c, -50, 50)) over two I64 columns and a masked F64 one, small integers (exact): cells, null
    bitmap and null count over all rows.  A boolean program whose true rows are a run across 2^31 plus every 1021st row: the count
    and every byte of the bitmap, again at 2^32 - 1 rows."""
    import torch

    def values(n, pivot):
        g = B.Eval(n, pivot, D)
        cols = g.value_columns()
        for j, c in enumerate(cols):
            mem["c%d" % j] = c[0]
        mem["cm"] = cols[2][1]
        mem["out"] = torch.empty(n, dtype=torch.float64, device=D)
        mem["om"] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=D)
        got, mask, n_null = mem.ctx.eval(cols, n, _program(g.VALUE_PROGRAM), out=mem["out"], out_mask=mem["om"])
        mem.mark()
        what = "eval value program at %d rows" % n
        _all_rows(got, lambda r: g.expected_values(r)[0], n, what)
        assert n_null == B.count_true(n, lambda r: g.expected_values(r)[1], D, ch=CMP) and n_null > n // 100, (what, n_null)
        _bitmap(mask, n, lambda r: g.expected_values(r)[1], n_null, what + " (mask)")
        del cols, got, mask
        mem.t.clear()
        return g

    _eval_mask(mem, values(N_SMALL, P_SMALL))
    mem.need(80)
    _eval_mask(mem, values(N_BIG, PIVOT))
    _release(mem)
    mem.need(45)
    _eval_mask(mem, B.Eval(N_MAX, PIVOT, D))


# ---- isin, and predicate on a masked column ---------------------------------------------------------------------------------------------
def _isin(mem, n, pivot, masked):
    import torch
    g = B.Isin(n, pivot, D)
    mem["x"] = g.column()[0]
    mem["bits"] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=D)
    L = _L()
    try:
        for which, negate in g.calls:
            mem.ctx.set_option("isin_path", 1 if which == "few" else 2)
            vals = g.values(which)
            bits, count = mem.ctx.isin((mem["x"], None, L.I64), n, (vals, None, L.I64), negate=negate, out=mem["bits"])
            mem.mark()
            what = "isin %s negate=%d at %d rows" % (which, negate, n)
            assert mem.ctx.timings()["n_partitions"] == (1 if which == "few" else 2), (what, mem.ctx.timings())     # 1: the LDS set, 2: the global one
            assert count == g.count(which, negate), (what, count, g.count(which, negate))
            _bitmap(bits, n, lambda r: g.expected(which, negate, r), count, what)
    finally:
        mem.ctx.set_option("isin_path", 0)
    if masked:
        p = B.MaskedPredicate(n, pivot, D)
        mem["m"] = B.pack_bits(n, p.nulls_at, D)                   # the ramp is the column already here
        for op, a in p.calls:
            bits, count = mem.ctx.predicate((mem["x"], mem["m"], L.I64), n, op, a, out=mem["bits"])
            what = "predicate op %d on a masked column at %d rows" % (op, n)
            assert count == p.count(op), (what, count, p.count(op))
            _bitmap(bits, n, lambda r: p.expected(op, r), count, what)
    mem.t.clear()


def test_isin_and_masked_predicate(mem):
    """x_i = i as I64.  isin through the LDS set (3 values) and the global set (10^5 values, below and above 2^31, some the column
    never holds), negated once; GT and ISNA on the same column under a 10 % periodic null mask.  isin again at 2^32 - 1 rows."""
    _isin(mem, N_SMALL, P_SMALL, True)
    mem.need(25)
    _isin(mem, N_BIG, PIVOT, True)
    _release(mem)
    mem.need(45)
    _isin(mem, N_MAX, PIVOT, False)


# ---- window: the rest ----------------------------------------------------------------------------------------------------------------------
def _window(mem, n, pivot, spans):
    """spans: the (lo, hi) row ranges on which the rolling maxima are recomputed"""
    L = _L()
    from tests.window_ref import ewm_close
    g = B.Window(n, pivot, D)
    last = None
    for name, what in g.calls:
        if name != last:
            mem.t.clear()
            mem["x"] = g.column(name)[0]
            last = name
        col = (mem["x"], None, L.F64)
        label = "%s of %s at %d rows" % (what, name, n)
        if what == "rolling_max":
            mem["got"] = mem.ctx.window(col, n, L.WINDOW_KIND_ROLLING, L.WINDOW_MAX, window=g.W)
            mem.mark()
            for lo, hi in spans:
                rows = B.arange(lo, hi, D)
                want = g.rolling_max(name, lo, hi)
                assert B.same(mem["got"][lo:hi], want), "%s: %s" % (label, B.first_bad(mem["got"][lo:hi], want, rows))
        elif what == "ewm_mean":
            mem["got"] = mem.ctx.window(col, n, L.WINDOW_KIND_EWM, L.WINDOW_MEAN, alpha=0.5)
            mem.mark()
            head = min(n, 100_000)                                # tests/window_ref.py's ewm_close itself on the first rows ...
            got, want, x = (t.cpu().numpy() for t in (mem["got"][:head], g.expected(name, what, B.arange(0, head, D)), mem["x"][:head]))
            assert ewm_close(got, want, x, np.ones(head, bool)), label
            for lo in range(0, n, CMP):                           # ... and its bound on all rows: 1e-12 max |x|, which is 1 from row 1 on
                rows = B.arange(lo, min(lo + CMP, n), D)
                err = (mem["got"][lo:lo + rows.numel()] - g.expected(name, what, rows)).abs()
                assert bool((err <= 1e-12 * (rows > 0)).all()), "%s: row %d" % (label, int(rows[(~(err <= 1e-12 * (rows > 0))).nonzero()[0]]))
        else:
            op = L.WINDOW_MAX if what == "expanding_max" else L.WINDOW_SUM
            mem["got"] = mem.ctx.window(col, n, L.WINDOW_KIND_EXPANDING, op, min_periods=0)
            mem.mark()
            _all_rows(mem["got"], lambda r: g.expected(name, what, r), n, label)    # integers: exact in any fold order
        del mem["got"]
    mem.t.clear()


def test_window_van_herk_expanding_scans_and_ewm(mem):
    """Rolling max, w = 3000 (van Herk blocks), of (i * 7919) mod 1021 and of the ascending scramble, recomputed with unfold on
    sampled spans; the expanding max of the ascending scramble (a record after every row 2^31) and the expanding sum of i mod 3,
    all rows; the EWM mean (alpha 0.5) of 0, 1, 0, 1, ... against its closed form."""
    _window(mem, N_SMALL, P_SMALL, [(0, N_SMALL)])
    mem.need(85)
    k = 100_000
    spans = [(0, k), (PIVOT - k, PIVOT + 4096), (N_BIG - k, N_BIG)] + [(s, s + 4096) for s in range(k, N_BIG - k, 79_193_330)]
    _window(mem, N_BIG, PIVOT, spans)


# ---- cumulative / lag: the rest ----------------------------------------------------------------------------------------------------------------
def _cumulative(mem, n, pivot, only=None):
    import torch
    L = _L()
    g = B.Cumulative(n, pivot, D)
    mem["x"] = torch.empty(n, dtype=torch.float64, device=D)
    mem["out"] = torch.empty(n, dtype=torch.int64, device=D)
    mem["om"] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=D)
    for name, calls in g.calls.items():
        calls = [c for c in calls if only is None or (name, c) in only]
        if not calls:
            continue
        _, mem["m"], _ = g.column(name, mem["x"])
        col = (mem["x"], mem["m"], L.F64)
        for call in calls:
            count_op = call == ("cum", B.COUNT)
            out = mem["out"] if count_op else mem["out"].view(torch.float64)
            if call[0] == "cum":
                got, mask, n_null = mem.ctx.cumulative(col, n, call[1], out=out, out_mask=mem["om"])
            else:
                got, mask, n_null = mem.ctx.lag(col, n, call[1], call[2], out=out, out_mask=mem["om"])
            mem.mark()
            what = "%s %r of %s at %d rows" % (call[0], call[1:], name, n)
            want_null = g.expected(name, call, B.arange(0, 1, D))[2]
            assert n_null == want_null, (what, n_null, want_null)
            if n == N_MAX:
                rows = B.arange(n - 1_000_000, n, D)
                _at_rows(got, lambda r: g.expected(name, call, r)[0], rows, what)
            else:
                _all_rows(got, lambda r: g.expected(name, call, r)[0], n, what)
                _bitmap(mask, n, lambda r: g.expected(name, call, r)[1], n_null, what + " (mask)")
    mem.t.clear()


def test_cumulative_and_lag(mem):
    """MAX and MIN with the last record after 2^31; PROD over 2, 0.5, 2, 0.5, ... (exact; the exponent carries); SUM and COUNT under
    a 10 % periodic null mask; SHIFT by 2^31 + 5, -(2^31 + 5) and 1 on the ramp, mask and count included; PCT_CHANGE(1).  COUNT
    again at 2^32 - 1 rows."""
    _cumulative(mem, N_SMALL, P_SMALL)
    mem.need(45)
    _cumulative(mem, N_BIG, PIVOT)
    _release(mem)
    mem.need(80)
    _cumulative(mem, N_MAX, PIVOT, only={("masked", ("cum", B.COUNT))})


# ---- 2^32 rows are refused ------------------------------------------------------------------------------------------------------------------------
def test_2_pow_32_rows_are_refused(mem):
    """window, window_quantile, describe, quantiles, eval, sort_indices and filter_indices: INVALID_ARGUMENT, a message naming 2^32,
    and no touch of the 16 cells behind the pointers.  (rank, fill, cumulative / lag, predicate / isin, topk and arg_extreme have
    this test in their own files.)"""
    L = _L()
    lib, h = L.load(), mem.ctx.h
    x = np.arange(16, dtype=np.float64)
    bits = np.full(2, 0xFF, np.uint8)
    out = np.full(16, -7.0)
    c, b = L.Column(), L.Column()
    c.data, c.dtype, b.data, b.dtype = x.ctypes.data, L.F64, bits.ctypes.data, L.BOOLBITS
    n = 1 << 32
    host = L.MEM_HOST
    wspec = L.WindowSpec(kind=L.WINDOW_KIND_ROLLING, op=L.WINDOW_SUM, window=3, min_periods=-1, center=0, reserved=0, ddof=1, alpha=0.0)
    qspec = L.WindowQuantileSpec(kind=L.WINDOW_KIND_ROLLING, median=1, window=3, min_periods=-1, center=0, nan_missing=0, q=0.5)
    stats, cnt = L.DescribeStats(), C.c_int64(-1)
    ps, qs = (C.c_double * 1)(50.0), (C.c_double * 1)(-7.0)
    ops, args = (C.c_int32 * 1)(L.EVAL_COL), (C.c_double * 1)(0.0)
    calls = {
        "window": lambda: lib.pandrs_hip_window(h, host, C.byref(c), n, C.byref(wspec), host, out.ctypes.data),
        "window_quantile": lambda: lib.pandrs_hip_window_quantile(h, host, C.byref(c), n, C.byref(qspec), host, out.ctypes.data),
        "describe": lambda: lib.pandrs_hip_describe(h, host, C.byref(c), n, C.byref(stats)),
        "quantiles": lambda: lib.pandrs_hip_quantiles(h, host, C.byref(c), n, ps, 1, qs, C.byref(cnt)),
        "eval": lambda: lib.pandrs_hip_eval(h, host, C.byref(c), 1, n, ops, args, 1, host, out.ctypes.data, bits.ctypes.data, C.byref(cnt)),
        "sort_indices": lambda: lib.pandrs_hip_sort_indices(h, host, C.byref(c), 1, None, None, 0, n, host, out.ctypes.data),
        "filter_indices": lambda: lib.pandrs_hip_filter_indices(h, host, C.byref(b), n, host, out.ctypes.data, C.byref(cnt)),
    }
    for name, call in calls.items():
        assert call() == L.ERR_INVALID_ARGUMENT, name
        assert "2^32" in L.last_error() and name.split("_")[0] in L.last_error(), (name, L.last_error())
        assert (out == -7.0).all() and (bits == 0xFF).all() and qs[0] == -7.0, name
