"""One call per path with a row index past 2^31, checked against EXACT references.

The C ABI takes up to 2^32 rows per call and row positions inside the kernels are 32-bit; kernels go wrong at 2^31
(signed wrap) and at 2^32 (unsigned wrap of begin + length).  Every test here makes ONE call with N between 2^31 and the
path's own admitted limit and asserts, through ctx.timings(), that the call took the path it is meant to cover (a silent
fallback to another path fails the test).

Exact references:
  * f64 value columns hold small integers, ((i * 7919) % 1021) - 510: every group's sum stays far below 2^53 and is exact in
    any fold order, so Sum, Mean (one division), Min, Max and Count are compared bit for bit;
  * an i64 column near 2^62 makes Sum wrap; its reference is a torch int64 sum, which wraps the same way;
  * First / Last read a column holding the row index as f64 (exact below 2^53): the group's smallest / largest row;
  * Std / Var: closed form, rtol 1e-9 (the library runs two passes over the rows).
Data and references are built on the device in chunks of 2^28 rows, written into preallocated tensors.  Where a closed form
exists (keys i mod G, sorted keys i >> s) the reference is that closed form or a reduction over a [rows / G, G] view;
otherwise a chunked torch reduction that does not use the library.  The CPU oracle is too slow at this size.

Every test keeps its peak device memory near or below 120 GB (the machines are shared).  A groupby call reserves its radix
workspace, about 1.4 x N x (8 (1 + value sources) + value sources) bytes, before it picks a path; so most cases use u32 codes
and N just over 2^31, and the clustered-rows cases run at 2^31 + 2^29 rows instead of just under their admitted limit of
2^32 - 2^22 (over 150 GB there): their default chunk keeps no bound near 2^32, the forced 2^31 chunk does.  The largest
admitted groupby (Count only: no value source) runs at the engine's limit itself.
Left out for the cap: groupby_indices (its entry point reserves about 80 B per row, 177 GB measured at 2^31 + 2^26 rows), the
fused join -> groupby sum (184 GB at a 2^31 + 2^26-row probe side) and the absorb pass (157 GB at 2^31 + 2^21 rows: past
about 2^31 rows only its compact spill is taken, whose spill buffer holds every row once more).
Paths: the groupby and join cases assert theirs through ctx.timings(); the K1 statistics and gather entry points have one
path each and report none.

Left out on purpose: Median and Nunique (they reserve about 115 and 165 B per row, DESIGN.md, over 250 GB at 2^31 rows),
and the distributed exchange.

Every test frees what it allocated (the `mem` fixture) and skips, with the numbers, when the device has less free memory
than it needs plus 20 %.  Each prints its wall time and peak device memory.
"""
import gc
import time

import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

D = "cuda:0"
CH = 1 << 28                      # rows per generation / reference chunk
GB = 1e9
N_RADIX = (1 << 31) + (1 << 25)   # 2080 rows for each of 2^20 groups
N_JUST = (1 << 31) + (1 << 21)    # just over 2^31: 2050 rows for each of 2^20 groups
G_RADIX = 1 << 20
HASH_MUL, HASH_XOR = -7046029254386353131, 0x5555AAAA5555AAAA


class _Mem:
    """Big tensors live here (not in test locals, which a failure's traceback keeps alive); peak = largest device use seen."""

    def __init__(self, torch):
        self.torch, self.t = torch, {}
        free, total = torch.cuda.mem_get_info()
        self.total, self.base, self.peak = total, total - free, total - free

    def need(self, gbytes):
        free, _ = self.torch.cuda.mem_get_info()
        if free < gbytes * GB * 1.2:
            pytest.skip("needs %.0f GB (+20 %%) of device memory, %.0f GB free" % (gbytes, free / GB))

    def mark(self):
        self.torch.cuda.synchronize()
        free, _ = self.torch.cuda.mem_get_info()
        self.peak = max(self.peak, self.total - free)

    def __getitem__(self, k):
        return self.t[k]

    def __setitem__(self, k, v):
        self.t[k] = v
        self.mark()

    def __delitem__(self, k):
        del self.t[k]

    def fresh(self):
        """A new context (the last call's arenas released) and torch's cached blocks returned, before the next call."""
        import pandrs_amd as pa
        self.ctx.close()
        self.torch.cuda.empty_cache()
        self.ctx = pa.Context(0)


@pytest.fixture
def mem(request):
    torch = pytest.importorskip("torch")
    import pandrs_amd as pa
    gc.collect()
    torch.cuda.empty_cache()
    m = _Mem(torch)
    m.ctx = pa.Context(0)
    t0 = time.perf_counter()
    yield m
    m.mark()
    wall = time.perf_counter() - t0
    m.t.clear()
    m.ctx.close()
    gc.collect()
    torch.cuda.empty_cache()
    print("\n[rows>2^31] %s: %.1f s, peak device memory %.1f GB" % (request.node.name, wall, (m.peak - m.base) / GB))


def _fill(out, fn):
    """out[lo:hi] = fn(i) for i = arange(lo, hi) on the device, in chunks."""
    import torch
    for lo in range(0, out.numel(), CH):
        hi = min(lo + CH, out.numel())
        out[lo:hi] = fn(torch.arange(lo, hi, device=D, dtype=torch.int64))


def _small(i):
    import torch
    return ((i * 7919) % 1021 - 510).to(torch.float64)


def _hkey(g):
    return (g * HASH_MUL) ^ HASH_XOR


def _bits(x):
    import torch
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x


def _assert_bits(got, want, what):
    import torch
    g, w = _bits(got), _bits(want.to(got.dtype) if want.dtype != got.dtype else want)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, "%s: %d of %d differ, first at %d: %r vs %r" % (
        what, bad.numel(), g.numel(), int(bad[0]), float(got.flatten()[int(bad[0])]), float(want.flatten()[int(bad[0])]))


def _by_key(kc, ref_keys):
    """-> (order of the result's groups, order of the reference's groups) so that both list the same keys."""
    import torch
    assert kc.shape[1] == ref_keys.numel(), "%d groups, expected %d" % (kc.shape[1], ref_keys.numel())
    go, ro = torch.argsort(kc[0]), torch.argsort(ref_keys)
    _assert_bits(kc[0][go], ref_keys[ro], "group keys")
    return go, ro


# ---- radix partition + lean aggregate ----------------------------------------------------------------------------------

def test_radix_lean_sum_mean_min_max_count_and_wrapping_i64(mem):
    """2^31 + 2^25 rows, hashed i64 key of 2^20 groups (key of row i: hash(i mod 2^20)).  One call over the f64 column
    (Sum / Mean / Min / Max / Count), one over an i64 column near 2^62 whose sums wrap."""
    import torch
    n, g = N_RADIX, G_RADIX
    m = n // g
    mem.need(110)
    mem["k"] = torch.empty(n, device=D, dtype=torch.int64)
    _fill(mem["k"], lambda i: _hkey(i % g))
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], _small)
    aggs = [(0, O.SUM), (0, O.MEAN), (0, O.MIN), (0, O.MAX), (0, O.COUNT)]
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.I64)], n, [(mem["v"], None, O.F64)], aggs)
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] > 0, t
    assert int(kn.sum()) == 0
    go, ro = _by_key(kc, _hkey(torch.arange(g, device=D, dtype=torch.int64)))
    vv = mem["v"].view(m, g)
    s = vv.sum(0)
    cnt = torch.full((g,), float(m), device=D, dtype=torch.float64)
    want = [s, s / cnt, vv.amin(0), vv.amax(0), cnt]      # (tensor / tensor: torch divides by a scalar through its reciprocal)
    for j, name in enumerate(("sum", "mean", "min", "max", "count")):
        _assert_bits(oa[j][go], want[j][ro], name)
    del mem["v"], vv

    mem["w"] = torch.empty(n, device=D, dtype=torch.int64)
    _fill(mem["w"], lambda i: (1 << 62) - 977 * ((i * 7919) % 1021) + (i % 3) * 0x1000_0000_0000)
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.I64)], n, [(mem["w"], None, O.I64)], [(0, O.SUM)])
    t = mem.ctx.timings()
    mem.mark()
    assert t["n_partitions"] > 0, t
    go, ro = _by_key(kc, _hkey(torch.arange(g, device=D, dtype=torch.int64)))
    ws = mem["w"].view(m, g).sum(0)                 # int64: 2080 values near 2^62 wrap, like the library's sum
    _assert_bits(oa[0][go], ws[ro].to(torch.float64), "i64 sum")


def test_older_kernel_std_var_first_last(mem):
    """2^31 + 2^21 rows, u32 codes i mod 2^20 (narrower than an i64 key: the case stays under the memory cap).
    The value is the row index: group g holds rows g + j 2^20, j < m, so First = g,
    Last = g + (m - 1) 2^20 (past 2^31 for every group) and the sample variance is 2^40 m (m + 1) / 12.
    Std / Var and First / Last take the older kernel by themselves (two calls: a row-index source doubles the workspace)."""
    import torch
    n, g = N_JUST, G_RADIX
    m = n // g
    mem.need(120)
    mem["k"] = torch.empty(n, device=D, dtype=torch.int32)
    _fill(mem["k"], lambda i: (i % g).to(torch.int32))
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], lambda i: i.to(torch.float64))
    keys = torch.arange(g, device=D, dtype=torch.int64)
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["v"], None, O.F64)], [(0, O.STD), (0, O.VAR)])
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] > 0, t
    go, ro = _by_key(kc, keys)
    var = float(g) * float(g) * m * (m + 1) / 12.0
    torch.testing.assert_close(oa[1], torch.full_like(oa[1], var), rtol=1e-9, atol=0)
    torch.testing.assert_close(oa[0], torch.full_like(oa[0], var ** 0.5), rtol=1e-9, atol=0)

    mem.fresh()
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["v"], None, O.F64)], [(0, O.FIRST), (0, O.LAST)])
    t = mem.ctx.timings()
    mem.mark()
    assert t["n_partitions"] > 0, t
    go, ro = _by_key(kc, keys)
    first = torch.arange(g, device=D, dtype=torch.float64)
    _assert_bits(oa[0][go], first[ro], "first")
    _assert_bits(oa[1][go], (first + float((m - 1) * g))[ro], "last")


def test_dominant_key_slices_sum_first_last(mem):
    """2^31 + 2^21 rows: half of them (every odd row) on ONE u32 code, 2^20, the even rows on 2^20 others (row 2r: r mod 2^20).
    The hot key's partition is cut into slices whose states merge; its Last is row N - 1 > 2^31."""
    import torch
    n, g = N_JUST, G_RADIX
    m2 = n // 2 // g
    hot = g
    mem.need(120)
    keys_all = torch.arange(g + 1, device=D, dtype=torch.int64)
    mem["k"] = torch.empty(n, device=D, dtype=torch.int32)
    _fill(mem["k"], lambda i: torch.where(i % 2 == 1, torch.full_like(i, hot), (i >> 1) % g).to(torch.int32))
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], _small)
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["v"], None, O.F64)], [(0, O.SUM)])
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] > 0, t
    go, ro = _by_key(kc, keys_all)
    pairs = mem["v"].view(n // 2, 2)
    want = torch.cat([pairs[:, 0].view(m2, g).sum(0), pairs[:, 1].sum().reshape(1)])
    _assert_bits(oa[0][go], want[ro], "sum")
    del pairs, mem["v"]

    mem.fresh()
    mem["r"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["r"], lambda i: i.to(torch.float64))
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["r"], None, O.F64)], [(0, O.FIRST), (0, O.LAST)])
    t = mem.ctx.timings()
    mem.mark()
    assert t["n_partitions"] > 0, t
    go, ro = _by_key(kc, keys_all)
    r = torch.arange(g, device=D, dtype=torch.float64)
    first = torch.cat([2 * r, torch.tensor([1.0], device=D, dtype=torch.float64)])
    last = torch.cat([2 * (r + float((m2 - 1) * g)), torch.tensor([float(n - 1)], device=D, dtype=torch.float64)])
    assert float(last[-1]) >= 2 ** 31
    _assert_bits(oa[0][go], first[ro], "first")
    _assert_bits(oa[1][go], last[ro], "last")


# ---- the few-groups direct path ----------------------------------------------------------------

def test_few_groups_direct_path(mem):
    """1 K u32 codes, code of row i = i mod 1000: every group fits one table, nothing spills (n_partitions 0)."""
    import torch
    n, g = N_RADIX, 1000
    mem.need(90)
    mem["k"] = torch.empty(n, device=D, dtype=torch.int32)
    _fill(mem["k"], lambda i: (i % g).to(torch.int32))
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], _small)
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["v"], None, O.F64)], [(0, O.SUM), (0, O.COUNT)])
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] == 0, t
    s = torch.zeros(g, device=D, dtype=torch.float64)
    for lo in range(0, n, CH):
        hi = min(lo + CH, n)
        s.index_add_(0, mem["k"][lo:hi].to(torch.int64), mem["v"][lo:hi])
    q, r = divmod(n, g)
    cnt = q + (torch.arange(g, device=D) < r).to(torch.float64)
    go, ro = _by_key(kc, torch.arange(g, device=D, dtype=torch.int64))
    _assert_bits(oa[0][go], s[ro], "sum")
    _assert_bits(oa[1][go], cnt[ro], "count")


# ---- rows clustered by key ------------------------------------------------------------------------------------------------

N_CLUSTERED = (1 << 31) + (1 << 29)
RUN, G_CLUSTERED = 4096, 61


@pytest.mark.parametrize("chunk", [0, 1 << 31], ids=["default_chunk", "chunk_2e31"])
def test_clustered_rows_sum_count(mem, chunk):
    """Rows grouped by key: runs of 4096 rows whose u32 keys cycle over 61 codes (run r: r mod 61) — the sample sees equal
    neighbours and unequal far pairs, so the call takes the one pass over the original columns (n_partitions -2), and a
    chunk never holds more than 61 keys.  With a forced chunk of 2^31 rows, chunk 1 ends at 2^32: the chunk bounds and the
    chunk count must be computed in 64 bits, else the last chunk's rows are dropped without a failure flag."""
    import torch
    n, g = N_CLUSTERED, G_CLUSTERED
    runs = n // RUN
    mem.need(110)
    mem["k"] = torch.empty(n, device=D, dtype=torch.int32)
    _fill(mem["k"], lambda i: ((i // RUN) % g).to(torch.int32))
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], _small)
    if chunk:
        mem.ctx.set_option("clustered_chunk", chunk)
    kc, kn, oa = mem.ctx.groupby_agg([(mem["k"], None, O.U32CODE)], n, [(mem["v"], None, O.F64)], [(0, O.SUM), (0, O.COUNT)])
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] == -2, t
    go, ro = _by_key(kc, torch.arange(g, device=D, dtype=torch.int64))
    s = torch.zeros(g, device=D, dtype=torch.float64)
    s.index_add_(0, torch.arange(runs, device=D) % g, mem["v"].view(runs, RUN).sum(1))      # exact: integers
    q, r = divmod(runs, g)
    _assert_bits(oa[0][go], s[ro], "sum")
    _assert_bits(oa[1][go], (RUN * (q + (torch.arange(g, device=D) < r)).to(torch.float64))[ro], "count")


# ---- the per-call limit ------------------------------------------------------------------------------------------------------

def test_largest_admitted_groupby_and_refusal_above(mem):
    """u32 codes i mod 1000, Count only (the key column is the counted column: no value source).  One real allocation of
    2^32 - 16384 rows: N = 2^32 - SC_TILE_MAX - 1 is answered exactly, N = 2^32 - SC_TILE_MAX is refused."""
    import torch
    import pandrs_amd as pa
    lim = (1 << 32) - 16384
    g = 1000
    mem.need(75)
    mem["k"] = torch.empty(lim, device=D, dtype=torch.int32)
    _fill(mem["k"], lambda i: (i % g).to(torch.int32))
    col = (mem["k"], None, O.U32CODE)
    n = lim - 1
    kc, kn, oa = mem.ctx.groupby_agg([col], n, [col], [(0, O.COUNT)])
    t = mem.ctx.timings()
    mem.mark()
    print(t)
    assert t["n_partitions"] == 0, t
    q, r = divmod(n, g)
    go, ro = _by_key(kc, torch.arange(g, device=D, dtype=torch.int64))
    _assert_bits(oa[0][go], (q + (torch.arange(g, device=D) < r).to(torch.float64))[ro], "count")
    with pytest.raises(pa.PandrsHipError):
        mem.ctx.groupby_agg([col], lim, [col], [(0, O.COUNT)])


# ---- join -------------------------------------------------------------------------------------------------------------------

N_JOIN = (1 << 31) + (1 << 26)
K_JOIN = 1 << 20


@pytest.mark.parametrize("how", ["inner", "left"])
def test_join_probe_side_beyond_2g(mem, how):
    """Left: 2^31 + 2^26 rows with keys i mod 2^20.  Right: 2^20 unique keys in a permuted order; for the left join every
    seventh key is replaced by one the left side never has, so those left rows come back with right index -1.
    The pairs come in left-row order: left index i, right index perm^-1(i mod 2^20)."""
    import torch
    import pandrs_amd as pa
    n, kk = N_JOIN, K_JOIN
    mem.need(110)
    gen = torch.Generator(device=D)
    gen.manual_seed(2031)
    perm = torch.randperm(kk, device=D, generator=gen)
    rkey = perm.clone()
    if how == "left":
        rkey = torch.where(perm % 7 == 0, perm + (1 << 40), perm)
    inv = torch.empty(kk, device=D, dtype=torch.int64)
    inv[perm] = torch.arange(kk, device=D, dtype=torch.int64)
    if how == "left":
        inv[torch.arange(0, kk, 7, device=D)] = -1
    mem["lk"] = torch.empty(n, device=D, dtype=torch.int64)
    _fill(mem["lk"], lambda i: i % kk)
    li, ri = mem.ctx.join_indices((mem["lk"], None, O.I64), n, (rkey, None, O.I64), kk, pa.INNER if how == "inner" else pa.LEFT)
    mem["li"], mem["ri"] = li, ri
    del li, ri
    t = mem.ctx.timings()
    print(t)
    assert t["n_partitions"] > 0, t
    assert mem["li"].numel() == n and mem["ri"].numel() == n
    for lo in range(0, n, CH):
        hi = min(lo + CH, n)
        i = torch.arange(lo, hi, device=D, dtype=torch.int64)
        assert torch.equal(mem["li"][lo:hi], i), "left index, rows %d.." % lo
        assert torch.equal(mem["ri"][lo:hi], inv[i % kk]), "right index, rows %d.." % lo


# ---- K1 column statistics and gather ----------------------------------------------------------------------------------------------

def test_column_stats_reduce_and_gather_beyond_2g(mem):
    """Whole-column statistics of 2^31 + 2^25 integer-valued f64 (sum, count, min, max exact; the minimum sits past 2^31),
    and a gather whose indices lie past 2^31."""
    import torch
    n = N_RADIX
    mem.need(50)
    mem["v"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["v"], lambda i: torch.where(i == n - 5, torch.full_like(i, -1000), (i * 7919) % 1021 - 510).to(torch.float64))
    want_sum = float(mem["v"].sum())                # exact: integers, every partial sum far below 2^53
    st = mem.ctx.column_stats((mem["v"], None, O.F64), n)
    assert st["count"] == n and st["count_finite"] == n
    assert st["sum_f64"] == want_sum and st["min"] == -1000.0 and st["max"] == 510.0, st
    out, cnt = mem.ctx.reduce_column((mem["v"], None, O.F64), n)
    assert cnt == n and out[0] == want_sum and out[2] == -1000.0 and out[3] == 510.0, out
    assert out[1] == want_sum / n
    del mem["v"]

    mem["r"] = torch.empty(n, device=D, dtype=torch.float64)
    _fill(mem["r"], lambda i: i.to(torch.float64))
    gen = torch.Generator(device=D)
    gen.manual_seed(2033)
    idx = torch.cat([torch.randint(1 << 31, n, (1 << 22,), device=D, generator=gen),
                     torch.arange(n - (1 << 20), n, device=D, dtype=torch.int64),
                     torch.randint(0, n, (1 << 20,), device=D, generator=gen),
                     torch.tensor([-1, (1 << 31) - 1, 1 << 31, n - 1], device=D, dtype=torch.int64)])
    got = mem.ctx.gather(mem["r"], None, idx, -7.0, O.F64)
    mem.mark()
    want = torch.where(idx >= 0, idx.to(torch.float64), torch.full_like(idx, -7, dtype=torch.float64))
    _assert_bits(got, want, "gather")
