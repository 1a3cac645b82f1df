"""pandrs_hip_moments / pandrs_hip_order_stats and the mirrors' shape statistics (reference
src/dataframe/pandas_compat/functions.rs:1617-1665, :2284-2314, :3571-3588, :4207-4224, :934-1022, :1583-1615;
helpers/aggregations.rs:8-225) against tests/moments_ref.py.

Two families.  EXACT: integer-valued cells in [-8, 8], adjusted so that the valid cells' sum is a multiple of their count: mean,
every deviation and every power are integers far below 2^53, so the reference's sequential fold and any parallel fold give the
same bits, and everything is compared bit for bit (cells that are +- powers of two in [2^-4, 2^4] do the same for recip_sum and
prod).  RANDOM: every sum S = sum t_i against the restatement's sequential fold of the same terms, the central ones around the
RETURNED mean, with the one bound of pandrs_hip.h: |got - ref| <= (2 gamma_m + 4 u) sum |t_i|, u = 2^-53, gamma_m = m u / (1 - m u)
(both folds lie within gamma_m sum |t| of the true sum; a term may round differently by a few ulps: powi against multiplication,
the device's ln at 1 ulp against libm).  prod carries its own contract, 2 gamma_m relative.  Counts, min, max, mean = sum / count
of the returned fields and every selected order statistic are bit for bit.  No other tolerance appears."""
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from pandrs_amd import _lib as L  # noqa: E402
from tests import bin_ref  # noqa: E402
from tests import describe_ref  # noqa: E402
from tests import moments_ref as R  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
TILE = int(re.search(r"moments_tile_rows = (\d+)", HEADER).group(1))
BLOCKS_PER_CU = int(re.search(r"moments_blocks_per_cu = (\d+)", HEADER).group(1))
MAX_COLUMNS = int(re.search(r"moments_max_columns = (\d+)", HEADER).group(1))
ALL = L.MOMENTS_WANT_CENTRAL | L.MOMENTS_WANT_LOG | L.MOMENTS_WANT_RECIP | L.MOMENTS_WANT_PROD
U = 2.0 ** -53
SUMS = ("sum", "abs_sum", "m2", "m3", "m4", "abs_dev", "log_sum", "recip_sum")
FIELDS = [name for name, _ in L.MomentsStats._fields_]
ARGS = (0.0, 0.25, 0.5, 0.75, 1.0, 0.3183098861837907)
assert MAX_COLUMNS == L.MOMENTS_MAX_COLUMNS


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def gamma(m):
    return m * U / (1.0 - m * U)


def exact_cells(rng, n, as_int=False, nan_share=0.0, null_share=0.1):
    """Integer-valued cells in [-8, 8] (and optional NaN cells) and a null flag per row, the valid cells' sum a multiple of
    their count."""
    v = rng.integers(-7, 9, n).astype(np.float64)
    nulls = rng.random(n) < null_share
    if nan_share and not as_int:
        v[rng.random(n) < nan_share] = np.nan
    valid = np.flatnonzero(~nulls & ~np.isnan(v))
    if valid.size:
        r = int(v[valid].sum()) % valid.size
        v[valid[:r]] -= 1.0                                # every cell was >= -7
        assert int(v[valid].sum()) % valid.size == 0 and v[valid].min() >= -8
    return (v.astype(np.int64) if as_int else v), nulls


def power_cells(rng, n):
    """+- powers of two in [2^-4, 2^4]: 1 / x and every running product are exact."""
    e = rng.integers(-4, 5, n)
    e[1::2] = -e[0:2 * (n // 2):2]                         # neighbours cancel: no prefix product leaves f64's range
    return np.ldexp(rng.choice([-1.0, 1.0], n), e)


def ref_fields(x, nulls, want=ALL, mean=None):
    return R.fields(R.values_of(x, nulls), want, mean)


def check_exact(got, x, nulls, want, names):
    ref = ref_fields(x, nulls, want)
    for name in names:
        assert same(got[name], ref[name]), (name, got[name], ref[name], len(x))


EXACT_FIELDS = ("count", "count_pos", "count_nonzero", "sum", "abs_sum", "min", "max", "mean", "m2", "m3", "m4", "abs_dev")


# ---- the exact family: row counts, memory spaces, repeatability ------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_exact_family_row_counts_host_device_resident(ctx, n):
    rng = np.random.default_rng(100 + n)
    f, fn = exact_cells(rng, n, nan_share=0.05)
    i, inulls = exact_cells(rng, n, as_int=True, null_share=0.0)              # the I64 column has no mask
    p = power_cells(rng, n)
    host_cols = [(f, bits(fn), L.F64), (i, None, L.I64), (p, None, L.F64)]
    got = ctx.moments(host_cols, n, ALL)
    check_exact(got[0], f, fn, ALL, EXACT_FIELDS)
    check_exact(got[1], i, inulls, ALL, EXACT_FIELDS)
    check_exact(got[2], p, None, ALL, ("count", "count_pos", "count_nonzero", "sum", "abs_sum", "min", "max", "recip_sum", "prod"))
    if n == 0:
        assert got[0]["count"] == 0 and math.isnan(got[0]["mean"]) and same(got[0]["sum"], -0.0) and got[0]["prod"] == 1.0
        assert got[0]["min"] == math.inf and got[0]["max"] == -math.inf
        return
    # the same bits for device and resident columns, for a second run, and one column at a time
    device_cols = [(dev(f), dev(bits(fn)), L.F64), (dev(i), None, L.I64), (dev(p), None, L.F64)]
    res = [ctx.upload_column(f, bits(fn), L.F64), ctx.upload_column(i, None, L.I64), ctx.upload_column(p, None, L.F64)]
    try:
        for cols in (device_cols, res, host_cols):
            again = ctx.moments(cols, n, ALL)
            for a, b in zip(got, again):
                assert all(same(a[k], b[k]) for k in FIELDS), (a, b)
        for k, col in enumerate(host_cols):
            one = ctx.moments([col], n, ALL)[0]
            assert all(same(one[name], got[k][name]) for name in FIELDS), (k, one, got[k])
    finally:
        for r_ in res:
            r_.release()


def test_more_tiles_than_workgroups(ctx):
    import torch
    n = BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count * TILE + 1
    rng = np.random.default_rng(7)
    f, fn = exact_cells(rng, n, nan_share=0.05)
    i, _ = exact_cells(rng, n, as_int=True, null_share=0.0)
    got = ctx.moments([(dev(f), dev(bits(fn)), L.F64), (dev(i), None, L.I64)], n, L.MOMENTS_WANT_CENTRAL)
    assert "stage_in" not in ctx.timings()["phase_ms"] and "aggregate" in ctx.timings()["phase_ms"]      # device columns: nothing is staged
    for g, v in ((got[0], f[~fn & ~np.isnan(f)].astype(np.int64)), (got[1], i)):      # integers: numpy's sums are exact in any order
        m, s = v.size, int(v.sum())
        assert s % m == 0
        d = v - s // m
        want = {"count": m, "count_pos": int((v > 0).sum()), "count_nonzero": int((v != 0).sum()), "sum": float(s),
                "abs_sum": float(np.abs(v).sum()), "min": float(v.min()), "max": float(v.max()), "mean": float(s // m),
                "m2": float((d ** 2).sum()), "m3": float((d ** 3).sum()), "m4": float((d ** 4).sum()), "abs_dev": float(np.abs(d).sum())}
        for name, w in want.items():
            assert g[name] == w, (name, g[name], w)
        assert math.isnan(g["log_sum"]) and math.isnan(g["recip_sum"]) and math.isnan(g["prod"])


def test_max_columns_mixed_dtypes_masks_at_byte_offsets_and_an_unaligned_pointer(ctx):
    n = 2 * TILE + 77
    rng = np.random.default_rng(9)
    cols, host_cols, cells = [], [], []
    for c in range(MAX_COLUMNS):
        as_int = c % 2 == 1
        masked = c % 4 < 2
        x, nulls = exact_cells(rng, n, as_int=as_int, nan_share=0.03, null_share=0.1 if masked else 0.0)
        mask = None
        if masked:
            padm = np.concatenate([np.array([0xFF], np.uint8), bits(nulls)])
            mask = dev(padm)[1:] if c % 8 < 4 else dev(bits(nulls))          # byte offset 1, then 0
        data = dev(np.concatenate([x[:1], x]))[1:] if c % 3 == 0 else dev(x)    # 8 bytes off a 16-byte boundary
        if data.data_ptr() % 16 == 8:
            cells.append(c)
        cols.append((data, mask, L.I64 if as_int else L.F64))
        host_cols.append((x, None if mask is None else bits(nulls), L.I64 if as_int else L.F64, nulls))
    assert cells, "no column 8 bytes off a 16-byte boundary"
    for k in (1, 2, MAX_COLUMNS):
        got = ctx.moments(cols[:k], n, L.MOMENTS_WANT_CENTRAL)
        assert len(got) == k
        for g, (x, _, _, nulls) in zip(got, host_cols):
            check_exact(g, x, nulls, L.MOMENTS_WANT_CENTRAL, EXACT_FIELDS)
    # ... and as host columns (staged, 16-byte aligned): the same bits
    staged = ctx.moments([h[:3] for h in host_cols], n, L.MOMENTS_WANT_CENTRAL)
    for a, b in zip(got, staged):
        assert all(same(a[k], b[k]) for k in FIELDS)


# ---- the random family ---------------------------------------------------------------------------------------------------------
def random_columns(n):
    rng = np.random.default_rng(31 + n)
    out = {}
    for name, x in (("normal", rng.normal(3.0, 2.0, n)), ("lognormal", rng.lognormal(0.0, 1.0, n)), ("inf", rng.normal(0.0, 1.0, n))):
        x[rng.random(n) < 0.05] = np.nan
        nulls = rng.random(n) < 0.10
        if name == "inf" and n > 8:
            x[[1, 5]] = math.inf
            x[3] = -math.inf
            nulls[[1, 3, 5]] = False
        out[name] = (x, nulls)
    return out


@pytest.mark.parametrize("n", [65, 3 * TILE + 1])
def test_random_family_within_the_fold_bound(ctx, n):
    columns = random_columns(n)
    names = list(columns)
    got = ctx.moments([(columns[k][0], bits(columns[k][1]), L.F64) for k in names], n, ALL)
    again = ctx.moments([(dev(columns[k][0]), dev(bits(columns[k][1])), L.F64) for k in names], n, ALL)
    for name, g, g2 in zip(names, got, again):
        assert all(same(g[k], g2[k]) for k in FIELDS), name                     # host and device, two runs: the same bits
        x, nulls = columns[name]
        values = R.values_of(x, nulls)
        ref = R.fields(values, ALL, mean=g["mean"])
        for k in ("count", "count_pos", "count_nonzero", "min", "max"):
            assert same(g[k], ref[k]), (name, k, g[k], ref[k])
        assert same(g["mean"], R._div(g["sum"], float(g["count"]))), name          # exactly sum / count of the returned fields
        m = g["count"]
        terms = R.terms(values, g["mean"])
        for k in SUMS:
            mag = R.rsum(abs(t) for t in terms[k])
            if not math.isfinite(mag) or not math.isfinite(ref[k]):
                assert same(g[k], ref[k]) or (math.isnan(g[k]) and math.isnan(ref[k])), (name, k, g[k], ref[k])
                continue
            err, bound = abs(g[k] - ref[k]), (2.0 * gamma(len(terms[k])) + 4.0 * U) * mag
            print("%s n=%d %s: err %.3e bound %.3e" % (name, n, k, err, bound))
            assert err <= bound, (name, k, g[k], ref[k], err, bound)
        if math.isfinite(ref["prod"]) and ref["prod"] != 0.0 and abs(ref["prod"]) > 2.3e-308:
            assert abs(g["prod"] - ref["prod"]) <= 2.0 * gamma(m) * abs(ref["prod"]), (name, g["prod"], ref["prod"])
        else:
            assert same(g["prod"], ref["prod"]), (name, g["prod"], ref["prod"])


def test_want_bits_select_the_fields_and_the_kernel_variant(ctx):
    x = np.random.default_rng(5).lognormal(0.0, 1.0, 3 * TILE + 1)
    col = (x, None, L.F64)
    full = ctx.moments([col], x.size, ALL)[0]
    owners = {"m2": 1, "m3": 1, "m4": 1, "abs_dev": 1, "log_sum": 2, "recip_sum": 4, "prod": 8}
    for want in range(16):
        g = ctx.moments([col], x.size, want)[0]
        t = ctx.timings()
        assert t["n_partitions"] == 1 + (want >> 1), (want, t)                 # 1 = the lean variant: no ln, no divide, no product
        assert t["table_slots"] == (2 if want & 1 else 1)
        assert t["algorithmic_bytes"] == (2 if want & 1 else 1) * 8 * x.size
        for name in FIELDS:
            if name in owners and not want & owners[name]:
                assert math.isnan(g[name]), (want, name)
            else:
                assert same(g[name], full[name]), (want, name)
    assert ctx.moments([col], x.size, 0) and ctx.timings()["n_partitions"] == 1
    assert ctx.moments([col], x.size, L.MOMENTS_WANT_CENTRAL) and ctx.timings()["n_partitions"] == 1


# ---- order statistics -----------------------------------------------------------------------------------------------------------
def order_columns():
    rng = np.random.default_rng(17)
    n = 2 * TILE + 5
    five = rng.choice([-2.0, 0.0, 1.0, 3.0, 8.0], n)
    ties_at_cuts = np.concatenate([np.full(n // 4 + 3, 1.0), rng.integers(2, 7, n - 2 * (n // 4 + 3)).astype(np.float64), np.full(n // 4 + 3, 7.0)])
    rng.shuffle(ties_at_cuts)
    with_nan = rng.integers(-8, 9, n).astype(np.float64)
    with_nan[rng.random(n) < 0.2] = np.nan
    big = (2 ** 53 + rng.integers(0, 1000, 777)).astype(np.int64)
    big[::5] = -big[::5]
    return {"five_values": (five, None), "ties_at_both_cuts": (ties_at_cuts, None), "all_equal": (np.full(TILE + 1, 2.5), None),
            "m1": (np.array([math.nan, 4.0, math.nan]), None), "m2": (np.array([9.0, math.nan, -1.0]), np.array([False, False, False])),
            "nan_and_null": (with_nan, rng.random(n) < 0.1), "i64_beyond_2_53": (big, None),
            "random": (rng.normal(0.0, 5.0, 3 * TILE + 1), rng.random(3 * TILE + 1) < 0.1)}


@pytest.mark.parametrize("name", list(order_columns()))
def test_order_statistics_by_the_four_index_rules(ctx, name):
    x, nulls = order_columns()[name]
    n = x.shape[0]
    dt = L.I64 if x.dtype == np.int64 else L.F64
    col = (x, None if nulls is None else bits(nulls), dt)
    values = R.values_of(x, nulls)
    s = R._sorted(values)
    ops = [(op, a) for a in ARGS for op in (L.OS_AT_FRAC_N, L.OS_AT_FRAC_N1, L.OS_MEDIAN, L.OS_TRIMMED_MEAN)]
    integer_valued = all(float(v).is_integer() and abs(v) < 2 ** 40 for v in s)
    for i in range(0, len(ops), L.ORDER_STATS_MAX_OPS):
        chunk = ops[i:i + L.ORDER_STATS_MAX_OPS]
        got, m = ctx.order_stats(col, n, chunk)
        want, want_m = R.order_stats(values, chunk)
        assert m == want_m == len(s)
        assert ctx.timings()["n_partitions"] == sum(1 for op, a in chunk if op == L.OS_TRIMMED_MEAN and 0.0 <= a < 0.5)
        for (op, a), g, w in zip(chunk, got, want):
            if op != L.OS_TRIMMED_MEAN or math.isnan(w):
                assert same(g, w), (name, op, a, g, w)                             # the element the reference's sort puts there
                continue
            kept = R.trimmed_slice(s, a)
            bound = (2.0 * gamma(len(kept)) + 4.0 * U) * R.rsum(abs(v) for v in kept) / len(kept)
            assert abs(g - w) <= bound, (name, a, g, w, bound)
            if integer_valued:
                assert same(g, w), (name, a, g, w)                                 # an exact numerator: bit for bit
    # device and resident columns, and a second run: the same bits
    dcol = (dev(x), None if nulls is None else dev(bits(nulls)), dt)
    res = ctx.upload_column(x, None if nulls is None else bits(nulls), dt)
    try:
        base = ctx.order_stats(col, n, ops[:8])[0]
        for c in (dcol, res, col):
            assert all(same(a, b) for a, b in zip(base, ctx.order_stats(c, n, ops[:8])[0]))
    finally:
        res.release()
    # describe, quantiles and qcut's edges on the same column are what they were
    ps = [0.0, 25.0, 50.0, 75.0, 100.0, 31.83]
    q, count = ctx.quantiles(col, n, ps)
    describe_ref.compare_quantiles(q, count, x, nulls, x.dtype, ps)
    describe_ref.compare_describe(ctx.describe(col, n), x, nulls, x.dtype)
    for k in (4, 10):
        edges, valid = ctx.bin_edges(col, n, L.BIN_QCUT, k)
        assert valid == len(s) and all(same(a, b) for a, b in zip(edges, bin_ref.qcut_edges(values, k)))


# ---- repeatability ------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_stale_workspace(ctx):
    import pandrs_amd as pa
    n = 3 * TILE + 77
    rng = np.random.default_rng(10)
    x = np.where(rng.random(n) < 0.1, np.nan, rng.lognormal(0.0, 1.0, n))
    col = (x, bits(rng.random(n) < 0.1), L.F64)
    other = (rng.integers(-50, 50, n).astype(np.int64), None, L.I64)
    ops = [(L.OS_TRIMMED_MEAN, 0.1), (L.OS_AT_FRAC_N, 0.25), (L.OS_MEDIAN, 0.0), (L.OS_TRIMMED_MEAN, 0.6), (L.OS_AT_FRAC_N, 1.0),
           (L.OS_TRIMMED_MEAN, 0.3183098861837907)]

    def run():
        out = []
        for want in (0, L.MOMENTS_WANT_CENTRAL, ALL):
            for st in ctx.moments([col, other], n, want):
                out.append(np.array([st[k] for k in FIELDS], np.float64).view(np.int64))
        for c in (col, other):
            got, m = ctx.order_stats(c, n, ops)
            out.extend([np.array(got, np.float64).view(np.int64), np.array([m])])
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


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import pandrs_amd as pa
    x = np.arange(100, dtype=np.float64)
    col = (x, None, L.F64)
    for cols, want in (([], 0), ([col] * (MAX_COLUMNS + 1), 0), ([col], 16), ([col], 1 << 20)):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.moments(cols, 100, want)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, (len(cols), want)
    for bad in ((np.zeros(100, np.uint32), None, L.U32CODE), (np.zeros(13, np.uint8), None, L.BOOLBITS)):
        with pytest.raises(pa.ColumnTypeMismatch):
            ctx.moments([col, bad], 100, 0)
        with pytest.raises(pa.ColumnTypeMismatch):
            ctx.order_stats(bad, 100, [(L.OS_MEDIAN, 0.0)])
    for ops in ([], [(L.OS_MEDIAN, 0.0)] * (L.ORDER_STATS_MAX_OPS + 1), [(4, 0.5)], [(-1, 0.5)], [(L.OS_AT_FRAC_N, math.nan)],
                [(L.OS_TRIMMED_MEAN, math.nan)]):
        with pytest.raises(pa.PandrsHipError) as e:
            ctx.order_stats(col, 100, ops)
        assert e.value.status == L.ERR_INVALID_ARGUMENT, ops
    # the reference's early returns: NaN, and the other ops of the call still answer
    got, m = ctx.order_stats(col, 100, [(L.OS_AT_FRAC_N1, 1.5), (L.OS_TRIMMED_MEAN, 0.5), (L.OS_AT_FRAC_N1, -0.1), (L.OS_AT_FRAC_N, 1.0),
                                        (L.OS_AT_FRAC_N1, 1.0), (L.OS_MEDIAN, math.nan)])
    assert m == 100 and [math.isnan(g) for g in got] == [True, True, True, True, False, False] and got[4] == 99.0 and got[5] == 49.5
    # no valid cell
    nan = np.full(70, math.nan)
    got, m = ctx.order_stats((nan, None, L.F64), 70, [(op, 0.25) for op in range(4)])
    assert m == 0 and np.isnan(got).all()
    got, m = ctx.order_stats((x[:70], bits(np.ones(70, bool)), L.F64), 70, [(op, 0.25) for op in range(4)])      # all null
    assert m == 0 and np.isnan(got).all()
    g = ctx.moments([(nan, None, L.F64), (x[:70], bits(np.ones(70, bool)), L.F64)], 70, ALL)
    for st in g:
        assert all(same(st[k], v) for k, v in R.fields(np.array([]), ALL).items()), st


CHILD = r"""
import ctypes as C, numpy as np, sys
sys.path.insert(0, %r)
import pandrs_amd as pa
from pandrs_amd import _lib as L
lib = L.load()
cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
n = 4_000_000                                                   # 32 MB to stage
big = (np.zeros(n), None, L.F64)
for call in (lambda: c.moments([big], n, 0), lambda: c.order_stats(big, n, [(L.OS_MEDIAN, 0.0)])):
    try:
        call()
        raise SystemExit("no error under memory_limit")
    except pa.PandrsHipError as e:
        assert e.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e), e
x = np.arange(1000, dtype=np.float64)
assert c.moments([(x, None, L.F64)], 1000, 1)[0]["mean"] == 499.5     # still works
c.close()
cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
assert lib.pandrs_hip_init(C.byref(cfg)) == 0
c = pa.Context(0)
for call in (lambda: c.moments([(x, None, L.F64)], 1000, 0), lambda: c.order_stats((x, None, L.F64), 1000, [(L.OS_MEDIAN, 0.0)])):
    try:
        call()
        raise SystemExit("no error below min_size_threshold")
    except pa.BelowThreshold as e:
        assert e.status == L.ERR_BELOW_THRESHOLD
y = np.arange(20_000, dtype=np.float64)
assert c.moments([(y, None, L.F64)], 20_000, 0)[0]["max"] == 19_999.0
assert c.order_stats((y, None, L.F64), 20_000, [(L.OS_MEDIAN, 0.0)])[0][0] == 9999.5
c.close()
print("limits ok")
"""


def test_memory_limit_and_threshold_in_a_child_process():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0 and "limits ok" in r.stdout, r.stdout + r.stderr


# ---- the mirrors, end to end ------------------------------------------------------------------------------------------------------
def test_frame_methods_end_to_end_on_the_exact_family(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(23)
    n = TILE + 300
    f, fn = exact_cells(rng, n, nan_share=0.05)
    i = rng.integers(1, 9, n).astype(np.int64)
    i[:int(i.sum()) % n] -= 1                              # still >= 0: a zero or two for harmonic_mean's filter
    p = power_cells(rng, n)
    df = F.OptimizedDataFrame()
    df.add_column("f", F.Float64Column.with_nulls(f.tolist(), fn.tolist()))
    df.add_column("label", F.StringColumn(["s"] * n))
    df.add_column("i", F.Int64Column(i.tolist()))
    df.add_column("p", F.Float64Column(p.tolist()))
    df.add_column("none", F.Float64Column([math.nan] * n))
    df.add_column("void", F.Int64Column.with_nulls(i.tolist(), [True] * n))                # every cell under a null bit
    cols = {"f": R.values_of(f, fn), "i": i.astype(np.float64), "p": p, "none": np.full(n, math.nan), "void": np.full(n, math.nan)}
    for c in ("f", "i"):
        v = cols[c]
        for name, ref, args in (("skew", R.skew, ()), ("kurtosis", R.kurtosis, ()), ("sem", R.sem, (1,)), ("mad", R.mad, ()),
                                ("var_column", R.var_column, (0,)), ("std_column", R.std_column, (1,)), ("range", R.value_span, ()),
                                ("abs_sum", R.abs_sum, ()), ("cv", R.cv, ()), ("iqr", R.iqr, ()), ("percentile_value", R.percentile_value, (0.3,)),
                                ("trimmed_mean", R.trimmed_mean, (0.1,)), ("trimmed_mean", R.trimmed_mean, (0.25,))):
            got, want = getattr(df, name)(c, *args), ref(v, *args)
            assert same(got, want), (c, name, got, want)
        d, want = df.describe_column(c), R.describe_column(v)
        assert d.keys() == want.keys() and all(same(d[k], want[k]) for k in d), (d, want)
        z, want = df.zscore(c), R.zscore(v)
        assert len(z) == n and all(same(a, b) for a, b in zip(z, want))
    assert same(df.prod("p"), R.prod(p)) and same(df.harmonic_mean("p"), R.harmonic_mean(p))
    gm, want = df.geometric_mean("i"), R.geometric_mean(i.astype(np.float64))
    # ln is not exact: the sums' one bound on log_sum, carried through the division by m (two roundings of u |x| between the two
    # sides) and through exp (the same libm exp on both sides, each result within one ulp = 2 u of the true exponential)
    logs = [math.log(t) for t in i.astype(np.float64) if t > 0.0]
    delta = (2.0 * gamma(len(logs)) + 4.0 * U) * R.rsum(abs(t) for t in logs) / len(logs) + 2.0 * U * abs(R.rsum(logs) / len(logs))
    print("geometric_mean: err %.3e bound %.3e" % (abs(gm - want), want * (math.expm1(delta) + 4.0 * U)))
    assert abs(gm - want) <= want * (math.expm1(delta) + 4.0 * U), (gm, want, delta)
    for c in ("none", "void"):                              # no valid cell: all NaN, or all null
        for name, args in (("skew", ()), ("kurtosis", ()), ("sem", (1,)), ("mad", ()), ("prod", ()), ("var_column", (0,)), ("range", ()),
                           ("cv", ()), ("geometric_mean", ()), ("harmonic_mean", ()), ("iqr", ()), ("percentile_value", (0.5,)),
                           ("trimmed_mean", (0.1,))):
            assert math.isnan(getattr(df, name)(c, *args)), (c, name)
        assert same(df.abs_sum(c), R.abs_sum(cols[c]))
        d = df.describe_column(c)
        assert sorted(d) == ["count", "max", "mean", "min", "std"] and d["count"] == 0.0 and all(math.isnan(d[k]) for k in d if k != "count")
        with pytest.raises(F.InvalidValue):
            df.zscore(c)
    for name in ("sum_all", "mean_all", "var_all", "std_all", "min_all", "max_all", "product_all", "median_all"):
        got, want = getattr(df, name)(), getattr(R, name)(cols)
        assert [k for k, _ in got] == [k for k, _ in want], (name, got, want)
        # what is exact where: the integer cells' product leaves 2^53; the powers of two have no integer mean for the central sums
        skip = {"product_all": ("i", "f"), "var_all": ("p",), "std_all": ("p",)}.get(name, ())
        got, want = [g for g in got if g[0] not in skip], [w for w in want if w[0] not in skip]
        assert [k for k, _ in got] == [k for k, _ in want] and all(same(a[1], b[1]) for a, b in zip(got, want)), (name, got, want)


def test_cpp_mirror(ctx):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "moments_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "moments_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "3 tests, 0 failed checks" in r.stdout, r.stdout + r.stderr
