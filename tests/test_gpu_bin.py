"""pandrs_hip_bin / pandrs_hip_bin_edges and the mirrors' value_range / cut / qcut / bin_codes (reference
src/dataframe/pandas_compat/functions.rs:2270-2282, :2339-2420) against tests/bin_ref.py.  Codes and counts are integers and every
edge is one of the column's own cells or the reference's expression of two of them: every comparison in this file is bit for bit
and count for count, no tolerance anywhere.  Every case runs through the search ("bin_path" 1) and through the guess (2; the
timings say whether it applied): they must agree with the restatement, hence with each other."""
import math
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests import bin_ref as R  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"bin_tile_rows = (\d+)", HEADER).group(1))
MAX_BINS = int(re.search(r"bin_max_bins = (\d+)", HEADER).group(1))
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
NAN_B = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000123))[0]
ALL_ONES = struct.unpack("<d", struct.pack("<Q", 0xFFFFFFFFFFFFFFFF))[0]
assert (L.BIN_NONE, L.BIN_NAN, L.BIN_MAX_BINS) == (R.NONE, R.NAN, MAX_BINS)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.set_option("bin_path", 0)
    c.close()


def full_grid():
    import torch
    return int(re.search(r"bin_blocks_per_cu = (\d+)", HEADER).group(1)) * torch.cuda.get_device_properties(0).multi_processor_count


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def host(b):
    return b if isinstance(b, np.ndarray) else b.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def uniform_edges(lo, w, n_bins, last=None):
    """e[0] + i * w, each product and sum rounded on its own, and a free last edge: what the guess is for."""
    e = np.float64(lo) + np.arange(n_bins + 1, dtype=np.float64) * np.float64(w)
    if last is not None:
        e[n_bins] = last
    return e


def around(edges):
    """every finite edge and its neighbours one ulp down and up, and a few cells far outside"""
    e = np.asarray(edges, np.float64)
    f = e[np.isfinite(e)]
    return np.concatenate([e, np.nextafter(f, -np.inf), np.nextafter(f, np.inf), [-1e300, 1e300, -math.inf, math.inf, math.nan]])


def check_bin(ctx, x, nulls, edges, col=None, out_device=False, guess=None):
    """Codes and counts through both paths against the restatement; `col` overrides how the column is passed; guess: whether
    the guess must (True) / cannot (False) apply under "bin_path" 2."""
    x = np.asarray(x)
    n = x.shape[0]
    mask = None if nulls is None else bits(nulls)
    col = col if col is not None else (x, mask, L.I64 if x.dtype == np.int64 else L.F64)
    want, want_counts = R.codes(R.values_of(x, nulls), edges)
    assert want_counts.sum() == n
    try:
        for path in (1, 2):
            ctx.set_option("bin_path", path)
            got, counts = ctx.bin(col, n, edges, out_device=out_device)
            ran = ctx.timings()["n_partitions"] if n else None
            got = host(got)
            assert got.dtype == np.int32 and got.shape == want.shape, (n, path)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (n, path, bad[:5], got[bad[:5]], want[bad[:5]], x[bad[:5]])
            assert np.array_equal(counts, want_counts), (n, path, counts, want_counts)
            if n and path == 1:
                assert ran == 1
            if n and path == 2 and guess is not None:
                assert ran == (2 if guess else 1), (n, ran)
    finally:
        ctx.set_option("bin_path", 0)
    return want, want_counts


# ---- row counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n)
    x = rng.normal(0.0, 3.0, n)
    x[rng.random(n) < 0.05] = np.nan
    check_bin(ctx, x, None, uniform_edges(-6.0, 1.5, 8), guess=True)
    check_bin(ctx, x, rng.random(n) < 0.1, [-math.inf, -2.0, -0.5, -0.5, 0.0, 0.25, 4.0], guess=False)
    check_bin(ctx, rng.integers(-10, 11, n), rng.random(n) < 0.1, uniform_edges(-8.0, 2.0, 40, last=100.0), guess=True)


def test_more_tiles_than_workgroups(ctx):
    n = (full_grid() + 1) * TILE + 5                                        # every workgroup loops, one of them once more
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, n)
    x[rng.random(n) < 0.01] = np.nan
    check_bin(ctx, x, rng.random(n) < 0.01, uniform_edges(-3.0, 0.06, 100), guess=True)
    check_bin(ctx, rng.integers(-100, 100, n), None, np.sort(rng.normal(0, 40, 33)), out_device=True, guess=False)


# ---- bin counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 2, 3, 63, 64, 65, 255, 256, 257, MAX_BINS - 1, MAX_BINS])
def test_bin_counts_with_every_edge_and_its_neighbours(ctx, n_bins):
    rng = np.random.default_rng(n_bins)
    for edges, guess in ((uniform_edges(-1.0, 2.0 / n_bins, n_bins, last=1.0 + 0.001), n_bins >= 2),
                         (uniform_edges(1e15, 37.0, n_bins), n_bins >= 2),
                         (np.sort(rng.normal(0.0, 1.0, n_bins + 1)), None)):
        x = np.concatenate([around(edges), rng.uniform(edges[0], edges[-1], TILE + 1)])
        rng.shuffle(x)
        _, counts = check_bin(ctx, x, None, edges, guess=guess)
        if guess:
            assert counts[:n_bins].min() >= 1                               # every bin of the even lists holds its own lower edge


def test_too_many_bins_and_bad_edge_lists_are_refused(ctx):
    import pandrs_amd as pa
    x = np.arange(100.0)
    for edges in (np.arange(MAX_BINS + 2, dtype=np.float64), [1.0], [0.0, 2.0, 1.0], [0.0, math.nan], [math.nan, 1.0], [3.0, 2.0]):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.bin((x, None, L.F64), 100, edges)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, edges
    for k in (0, MAX_BINS + 1):
        for kind in (L.BIN_CUT, L.BIN_QCUT):
            with pytest.raises(pa.PandrsHipError) as e:
                ctx.bin_edges((x, None, L.F64), 100, kind, k)
            assert e.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.bin_edges((x, None, L.F64), 100, 2, 3)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(pa.ColumnTypeMismatch):
        ctx.bin((np.arange(100, dtype=np.uint32), None, L.U32CODE), 100, [0.0, 1.0])
    with pytest.raises(pa.ColumnTypeMismatch):
        ctx.bin_edges((np.arange(100, dtype=np.uint32), None, L.U32CODE), 100, L.BIN_CUT, 2)


# ---- edge values -------------------------------------------------------------------------------------------------------------------
def test_special_edges_and_cells(ctx):
    cells = np.array([math.nan, NAN_B, ALL_ONES, math.inf, -math.inf, 0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1.0,
                      np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 2.0, 3.0, -1.0, 1e308, -1e308, 2.0 ** 53, 2.0 ** 53 + 2])
    x = np.resize(cells, TILE + 77)
    np.random.default_rng(1).shuffle(x)
    nulls = np.random.default_rng(2).random(x.shape[0]) < 0.1
    lists = [[-math.inf, 0.0, math.inf],                                     # +-inf edges: +inf itself matches no bin
             [-math.inf, -math.inf, -1.0, math.inf, math.inf],
             [-0.0, 1.0], [0.0, 1.0], [-1.0, -0.0], [-1.0, 0.0],             # a zero edge against both zeros
             [-0.0, 0.0, 0.0, 1.0],
             [1.0, 1.0, 1.0, 1.0],                                           # all edges equal: every bin empty
             [-1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0],                           # repeated edges: empty bins are skipped
             [-5e-324, 0.0, 5e-324, 1e-310, 2.2250738585072014e-308],        # denormals
             [-1e308, 0.0, 1e308], [2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 53 + 4],
             uniform_edges(-5e-324, 5e-324, 4)]
    for edges in lists:
        check_bin(ctx, x, None, edges)
        check_bin(ctx, x, nulls, edges)
    want, _ = check_bin(ctx, np.array([0.0, -0.0, 0.0, -0.0]), None, [-0.0, 1.0])
    assert want.tolist() == [0, 0, 0, 0]                                      # comparisons are by value
    want, counts = check_bin(ctx, np.array([math.nan, NAN_B, ALL_ONES, 1.0]), None, [0.0, 2.0])
    assert want.tolist() == [R.NAN, R.NAN, R.NAN, 0] and counts.tolist() == [1, 0, 3]


def test_the_guess_at_an_edge_and_one_ulp_off_it(ctx):
    """Evenly spaced lists whose products round: the guess lands beside the bin, the correction finds it; also a list that is
    even only within the quarter-width tolerance, and one that is not (the search answers under "bin_path" 2)."""
    rng = np.random.default_rng(11)
    for lo, w, nb in ((0.1, 0.1, 1000), (-7.3, 1e-9, 333), (1e15, 0.125, 500), (2.0 ** 52, 1.0, 64), (-1e-3, 3e-7, 4096), (0.0, 1e300, 100)):
        edges = uniform_edges(lo, w, nb)
        x = np.concatenate([around(edges), rng.uniform(edges[0], edges[-1], 2 * TILE)])
        check_bin(ctx, x, None, edges, guess=True)
    jitter = uniform_edges(0.0, 1.0, 200) + np.concatenate([[0.0], rng.uniform(-0.2, 0.2, 198), [0.0, 0.0]])
    check_bin(ctx, np.concatenate([around(jitter), rng.uniform(-1, 201, TILE)]), None, jitter, guess=True)
    uneven = np.cumsum(rng.uniform(0.0, 2.0, 201))
    check_bin(ctx, np.concatenate([around(uneven), rng.uniform(0, 200, TILE)]), None, uneven, guess=False)
    far = uniform_edges(0.0, 1.0, 50)
    far[10:40] += 0.24                                                        # rows between up to a quarter width off the guess
    check_bin(ctx, np.concatenate([around(far), rng.uniform(-1, 51, TILE)]), None, far, guess=True)


# ---- I64 ---------------------------------------------------------------------------------------------------------------------------
def test_i64_cells_as_f64(ctx):
    base = np.array([0, 1, -1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, -2 ** 53, -(2 ** 53 + 1), -(2 ** 53 + 2), I64_MIN,
                     I64_MIN + 1, I64_MAX, I64_MAX - 1, I64_MAX - 512, I64_MAX - 513, 7], np.int64)
    x = np.resize(base, TILE + 9)
    np.random.default_rng(4).shuffle(x)
    nulls = np.random.default_rng(5).random(x.shape[0]) < 0.1
    two63 = 2.0 ** 63
    for edges in ([-two63, -2.0 ** 53, 0.0, 2.0 ** 53, 2.0 ** 53 + 2, two63],     # INT64_MAX as f64 is 2^63: it matches no bin
                  [-two63, np.nextafter(two63, math.inf)], [2.0 ** 53, 2.0 ** 53 + 2], [np.nextafter(2.0 ** 53, 0.0), 2.0 ** 53],
                  [-math.inf, -two63, -2.0 ** 53 - 2, 2.0 ** 53 + 4, two63, math.inf], uniform_edges(-2.0 ** 53 - 4, 2.0, 8),
                  uniform_edges(-two63, 2.0 ** 60, 16)):
        check_bin(ctx, x, None, edges)
        check_bin(ctx, x, nulls, edges, out_device=True)
    want, _ = check_bin(ctx, np.array([2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2], np.int64), None, [2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 53 + 4])
    assert want.tolist() == [0, 0, 1]                                         # 2^53 + 1 falls where 2^53 falls


# ---- null masks --------------------------------------------------------------------------------------------------------------------
def test_null_masks_at_byte_offsets(ctx):
    import torch
    n = 2 * TILE + 13
    rng = np.random.default_rng(6)
    x = rng.normal(0.0, 2.0, n)
    edges = uniform_edges(-4.0, 0.5, 16)
    dx = dev(x)
    for nulls in (rng.random(n) < 0.3, np.ones(n, bool), np.zeros(n, bool)):
        m = bits(nulls)
        tail = m.copy()
        if n % 8:
            tail[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)                    # bits past n_rows set: ignored
        for off in (0, 1, 3):
            buf = np.full(off + m.shape[0] + 8, 0xFF, np.uint8)
            buf[off:off + m.shape[0]] = tail
            hm = buf[off:off + m.shape[0]]
            dm = dev(buf)[off:off + m.shape[0]]
            check_bin(ctx, x, nulls, edges, col=(x, hm, L.F64))
            check_bin(ctx, x, nulls, edges, col=(dx, dm, L.F64), out_device=True)
    want, counts = check_bin(ctx, x, np.ones(n, bool), edges)
    assert (want == R.NAN).all() and counts[-1] == n
    del dx
    torch.cuda.empty_cache()


# ---- buffers -----------------------------------------------------------------------------------------------------------------------
def test_memory_spaces_outputs_and_guards(ctx):
    import torch
    n = 2 * TILE + 19
    rng = np.random.default_rng(7)
    for x in (rng.normal(0.0, 2.0, n), rng.integers(-9, 10, n)):
        nulls = rng.random(n) < 0.1
        dt = L.I64 if x.dtype == np.int64 else L.F64
        edges = uniform_edges(-4.0, 0.25, 32)
        want, want_counts = R.codes(R.values_of(x, nulls), edges)
        shifted = dev(np.concatenate([x[:1], x]))[1:]                         # the data pointer 8 bytes off a 16-byte boundary
        assert shifted.data_ptr() % 16 == 8
        device_col = (dev(x), dev(bits(nulls)), dt)
        resident = ctx.upload_column(x, bits(nulls), dt)
        try:
            for col in ((x, bits(nulls), dt), device_col, (shifted, device_col[1], dt), resident):
                for out_device in (False, True):
                    check_bin(ctx, x, nulls, edges, col=col, out_device=out_device)
                for path in (1, 2):
                    ctx.set_option("bin_path", path)
                    none, counts = ctx.bin(col, n, edges, want_codes=False)                       # the histogram alone
                    assert none is None and np.array_equal(counts, want_counts)
                    got, none = ctx.bin(col, n, edges, out_device=False, want_counts=False)       # the codes alone
                    assert none is None and np.array_equal(got, want)
                    # a caller's buffer at a 4-byte and at an 8-byte boundary, guard cells on both sides
                    for lead in (1, 2):
                        for make in (lambda: np.full(n + 8, 0x5A5A5A5A, np.int32),
                                     lambda: torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")):
                            buf = make()
                            got, _ = ctx.bin(col, n, edges, out=buf[lead:lead + n])
                            whole = host(buf)
                            assert np.array_equal(whole[lead:lead + n], want) and np.array_equal(host(got), want), (path, lead)
                            assert (whole[:lead] == 0x5A5A5A5A).all() and (whole[lead + n:] == 0x5A5A5A5A).all(), (path, lead)
            got, _ = ctx.bin(device_col, n, edges)                                                # device in, device out by default
            assert got.is_cuda and got.dtype == torch.int32 and got.numel() == n
        finally:
            ctx.set_option("bin_path", 0)
            resident.release()
    del device_col, shifted
    torch.cuda.empty_cache()


# ---- counts ------------------------------------------------------------------------------------------------------------------------
def test_counts(ctx):
    n = 5 * TILE + 321
    rng = np.random.default_rng(8)
    edges = uniform_edges(0.0, 1.0, 64)
    cases = {"uniform": rng.uniform(0.0, 64.0, n), "one bin": np.full(n, 17.5), "two alternating": np.where(np.arange(n) % 2 == 0, 3.5, 40.5),
             "all none": np.full(n, -1.0), "all nan": np.full(n, math.nan), "few": rng.integers(0, 6, n) + 0.5}
    for name, x in cases.items():
        for e in (edges, [0.0, 64.0], np.sort(rng.uniform(0.0, 64.0, 300))):
            _, counts = check_bin(ctx, x, None, e)
            assert counts.sum() == n, name
    _, counts = check_bin(ctx, cases["one bin"], None, edges)
    assert counts[17] == n
    _, counts = check_bin(ctx, cases["two alternating"], None, edges)
    assert counts[3] == (n + 1) // 2 and counts[40] == n // 2
    _, counts = check_bin(ctx, cases["all none"], None, edges)
    assert counts[64] == n
    _, counts = check_bin(ctx, cases["all nan"], None, edges)
    assert counts[65] == n


# ---- the edge lists ----------------------------------------------------------------------------------------------------------------
def qcut_check(ctx, x, nulls, q, col=None):
    x = np.asarray(x)
    n = x.shape[0]
    v = R.values_of(x, nulls)
    col = col if col is not None else (x, None if nulls is None else bits(nulls), L.I64 if x.dtype == np.int64 else L.F64)
    got, valid = ctx.bin_edges(col, n, L.BIN_QCUT, q)
    m = int((~np.isnan(v)).sum())
    assert valid == m, (n, q)
    if m == 0:
        assert np.isnan(got).all() and got.shape == (q + 1,)
        return
    want = R.qcut_edges(v, q)
    assert same_bits(got, want), (n, q, got, want)
    assert ctx.timings()["n_partitions"] == -(-(q + 1) // 32)


@pytest.mark.parametrize("q", [1, 2, 4, 10, 31, 32, 33, 100])
def test_qcut_edges(ctx, q):
    rng = np.random.default_rng(q)
    n = 3 * TILE + 17
    x = rng.normal(1.0, 5.0, n)                                               # (no zero cell: the sign of a zero edge is the header's deviation)
    x[rng.random(n) < 0.1] = np.nan
    nulls = rng.random(n) < 0.1
    qcut_check(ctx, x, None, q)
    qcut_check(ctx, x, nulls, q)                                              # NaN and null cells are not among the m
    qcut_check(ctx, rng.integers(1, 6, n).astype(np.float64), nulls, q)       # heavy ties
    qcut_check(ctx, np.full(n, 2.5), None, q)                                 # all equal
    qcut_check(ctx, np.array([3.0, 1.0, 2.0]), None, q)                       # m < q for most q
    qcut_check(ctx, np.array([math.nan, 7.0, math.nan]), None, q)             # one valid cell
    qcut_check(ctx, np.array([math.nan, 7.0, math.nan]), np.array([False, True, False]), q)     # none
    big = rng.integers(2 ** 53, 2 ** 53 + 4096, n).astype(np.int64) * rng.choice([-1, 1], n)
    qcut_check(ctx, big, nulls, q)                                            # I64 beyond 2^53: the selected integer as f64
    qcut_check(ctx, np.array([I64_MIN, I64_MAX, 0, I64_MAX - 1, I64_MIN + 1], np.int64), None, q)
    dx = dev(x)
    qcut_check(ctx, x, None, q, col=(dx, None, L.F64))
    resident = ctx.upload_column(x, bits(nulls), L.F64)
    try:
        qcut_check(ctx, x, nulls, q, col=resident)
    finally:
        resident.release()


def test_qcut_edges_with_both_zeros_equal_by_value(ctx):
    x = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 2.0, 0.0])
    for q in (1, 2, 3, 8):
        got, valid = ctx.bin_edges((x, None, L.F64), 8, L.BIN_QCUT, q)
        want = R.qcut_edges(x, q)
        assert valid == 8 and np.array_equal(got, want)                       # ... and differs at most in a zero's sign bit
        assert same_bits(np.where(got == 0.0, 0.0, got), np.where(want == 0.0, 0.0, want))


def _family(name, rng, n):
    if name == "normal":
        return rng.normal(0.5, 10.0, n)
    if name == "small_ints":
        return rng.integers(-3, 4, n).astype(np.float64)
    if name == "constant":
        return np.full(n, 1.5)
    if name == "1e15":
        return 1e15 + rng.integers(0, 1000, n).astype(np.float64) * 0.125
    if name == "2^52":
        return 2.0 ** 52 + rng.integers(0, 64, n).astype(np.float64)
    if name == "1e-3":
        return rng.uniform(-1.0, 1.0, n) * 1e-3
    v = rng.normal(5.0, 2.0, n)
    v[rng.random(n) < 0.1] = np.nan
    return v


@pytest.mark.parametrize("name", ["normal", "small_ints", "constant", "1e15", "2^52", "1e-3", "nan10"])
def test_cut_edges(ctx, name):
    rng = np.random.default_rng(len(name))
    n = 2 * TILE + 5
    x = _family(name, rng, n)
    nulls = rng.random(n) < 0.05
    for bins in (1, 2, 7, 100, MAX_BINS):
        for nl in (None, nulls):
            got, valid = ctx.bin_edges((x, None if nl is None else bits(nl), L.F64), n, L.BIN_CUT, bins)
            v = R.values_of(x, nl)
            assert valid == int((~np.isnan(v)).sum())
            assert same_bits(got, R.cut_edges(v, bins)), (name, bins)
    xi = rng.integers(-2 ** 53 - 100, 2 ** 53 + 100, n)
    got, valid = ctx.bin_edges((dev(xi), None, L.I64), n, L.BIN_CUT, 9)
    assert valid == n and same_bits(got, R.cut_edges(xi.astype(np.float64), 9))


@pytest.mark.parametrize("cells", [[1.0, math.inf], [-math.inf, 2.0], [-1e308, 1e308], [math.inf], [-math.inf, math.inf]])
def test_cut_edges_when_the_width_is_not_finite(ctx, cells):
    x = np.array(cells + [math.nan])
    for bins in (1, 3):
        got, valid = ctx.bin_edges((x, None, L.F64), x.shape[0], L.BIN_CUT, bins)
        want = R.cut_edges(x, bins)
        assert valid == len(cells) and math.isnan(got[0]) and same_bits(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want))
        assert np.array_equal(np.isnan(got), np.isnan(want))                  # NaN or inf exactly where the host expression gives them


def test_no_valid_cell(ctx):
    for x, nulls in ((np.full(TILE + 3, math.nan), None), (np.arange(10.0), np.ones(10, bool))):
        for kind in (L.BIN_CUT, L.BIN_QCUT):
            got, valid = ctx.bin_edges((x, None if nulls is None else bits(nulls), L.F64), x.shape[0], kind, 4)
            assert valid == 0 and got.shape == (5,) and np.isnan(got).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_frame_methods_end_to_end(ctx):
    import pandrs_amd.frame as F
    n = 100_000
    rng = np.random.default_rng(9)
    a = rng.normal(3.0, 2.0, n)
    a[rng.random(n) < 0.05] = np.nan
    nulls = rng.random(n) < 0.05
    big = 1e15 + rng.integers(0, 4000, n).astype(np.float64) * 0.125
    big[:3] = big.max()                                                       # the maximum, three times: cut leaves those rows out
    i = rng.integers(-50, 51, n)
    df = F.OptimizedDataFrame()
    df.add_column("a", F.Float64Column.with_nulls(a, nulls))
    df.add_column("big", F.Float64Column(big))
    df.add_column("i", F.Int64Column(i))
    va = np.where(nulls, np.nan, a)
    dropped = {}
    for name, v in (("a", va), ("big", big), ("i", i.astype(np.float64))):
        assert df.value_range(name) == R.value_range(v)
        for k in (1, 10, 100):
            want = R.cut(v, k)
            got = df.cut(name, k)
            dropped[name, k] = n - len(got)
            assert len(got) == len(want) and got == want, (name, k)
            assert df.qcut(name, k) == R.qcut(v, k), (name, k)
        e = R.search_edges(R.qcut_edges(v, 10), True)
        codes, counts = df.bin_codes(name, e)
        want_codes, want_counts = R.codes(v, e)
        assert np.array_equal(codes, want_codes) and np.array_equal(counts, want_counts)
    at_max = int((big == big.max()).sum())
    assert at_max >= 3 and all(dropped["a", k] == 0 and dropped["i", k] == 0 for k in (1, 10, 100))
    assert all(dropped["big", k] == at_max for k in (1, 10, 100))             # max + 0.001 == max at 1e15: the reference drops those rows
    # the reference's own cases
    small = F.OptimizedDataFrame()
    small.add_column("a", F.Float64Column([1.0, 2.5, 4.0, 5.0]))
    assert small.cut("a", 2) == ["(1.00, 3.00]", "(1.00, 3.00]", "(3.00, 5.00]", "(3.00, 5.00]"]
    small = F.OptimizedDataFrame()
    small.add_column("a", F.Float64Column([1.0, math.nan, 3.0, 4.0]))
    assert small.qcut("a", 2) == ["Q1", "NaN", "Q2", "Q2"] and small.cut("a", 2)[1] == "NaN"
    inf = F.OptimizedDataFrame()
    inf.add_column("a", F.Float64Column([1.0, math.nan, math.inf]))
    assert inf.cut("a", 3) == ["NaN"]
    nothing = F.OptimizedDataFrame()
    nothing.add_column("a", F.Float64Column([math.nan, math.nan]))
    for fn in (lambda: nothing.cut("a", 2), lambda: nothing.qcut("a", 2), lambda: nothing.value_range("a")):
        with pytest.raises(F.InvalidValue):
            fn()


# ---- repeatability -----------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_stale_workspace(ctx):
    import pandrs_amd as pa
    n = 3 * TILE + 77
    rng = np.random.default_rng(10)
    x = np.where(rng.random(n) < 0.1, np.nan, rng.normal(0.0, 3.0, n))
    col = (x, bits(rng.random(n) < 0.1), L.F64)
    edges = uniform_edges(-6.0, 0.1, 120)

    def run():
        out = []
        for path in (1, 2):
            ctx.set_option("bin_path", path)
            out.extend(ctx.bin(col, n, edges, out_device=False))
        ctx.set_option("bin_path", 0)
        for kind, k in ((L.BIN_CUT, 17), (L.BIN_QCUT, 10), (L.BIN_QCUT, 40)):
            e, valid = ctx.bin_edges(col, n, kind, k)
            out.extend([e.view(np.int64), np.array([valid])])
        return out

    plain = run()
    again = run()
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    try:
        for fill in (0x00, 0xFF, 0xA5):
            before = pa.Context.workspace_poisoned_bytes()
            pa.Context.poison_workspace(fill)
            got = run()
            assert all(np.array_equal(a, b) for a, b in zip(plain, got)), fill
            assert pa.Context.workspace_poisoned_bytes() > before, fill
    finally:
        pa.Context.poison_workspace(None)
        ctx.set_option("bin_path", 0)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(ctx):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bin_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "bin_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "6 tests, 0 failed checks" in r.stdout
