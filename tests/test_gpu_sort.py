"""pandrs_hip_sort_indices and the mirrors' sort_by / sort_by_columns (reference src/optimized/split_dataframe/sort.rs:18-272,
frame assembly select.rs:172-226) against the reference's comparator restated here: Python's stable `sorted` with
functools.cmp_to_key for small inputs, np.lexsort over encoded keys (stable too) for larger ones, torch.sort(stable=True)
as an independent reference at 50 M rows.  NaN follows the header's documented rule (after every number, before nulls)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as g
    g.build()
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


from pandrs_amd import _lib as L  # noqa: E402
from tests.sort_ref import STRINGS, Col, rank_of, ref_cmp, ref_lexsort  # noqa: E402


def got(ctx, cols, asc, n=None):
    strings = next((c.strings for c in cols if c.dtype == L.U32CODE), None)
    rank = rank_of(strings) if strings is not None else None
    out = ctx.sort_indices([c.triple() for c in cols], cols[0].n if n is None else n, asc, rank)
    return out.cpu().numpy()


def make_col(rng, dtype, n, distinct=5, null_p=0.0, strings=None):
    nulls = rng.random(n) < null_p if null_p else None
    if dtype == L.I64:
        pool = rng.integers(-2**63, 2**63 - 1, distinct, dtype=np.int64, endpoint=True)
        return Col(dtype, pool[rng.integers(0, distinct, n)], nulls)
    if dtype == L.F64:
        pool = np.concatenate([rng.normal(0, 1e6, max(distinct - 4, 1)), [np.nan, -0.0, 0.0, -np.inf]])
        return Col(dtype, pool[rng.integers(0, len(pool), n)], nulls)
    if dtype == L.U32CODE:
        strings = strings or STRINGS
        return Col(dtype, rng.integers(0, len(strings), n).astype(np.uint32), nulls, strings)
    return Col(dtype, rng.random(n) < 0.5, nulls)


DTYPES = [L.I64, L.F64, L.U32CODE, L.BOOLBITS]


# ---- exact permutations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("null_p", [0.0, 0.2])
@pytest.mark.parametrize("asc", [True, False])
def test_every_dtype_with_and_without_nulls(ctx, dtype, null_p, asc):
    rng = np.random.default_rng(dtype * 10 + int(asc) + int(null_p * 10))
    col = make_col(rng, dtype, 5000, distinct=7, null_p=null_p)
    want = ref_cmp([col], [asc])
    assert np.array_equal(got(ctx, [col], [asc]), want)
    assert np.array_equal(ref_lexsort([col], [asc]), want)          # the two restatements agree


@pytest.mark.parametrize("n_keys", [2, 3, 5, 8])
def test_mixed_directions_over_several_keys(ctx, n_keys):
    rng = np.random.default_rng(100 + n_keys)
    n = 20_000 if n_keys < 8 else 300_000
    cols = [make_col(rng, DTYPES[(k + n_keys) % 4], n, distinct=3 + k, null_p=0.1 * (k % 2)) for k in range(n_keys)]
    asc = [bool((k * 7 + n_keys) % 3) for k in range(n_keys)]
    want = ref_cmp(cols, asc) if n <= 20_000 else ref_lexsort(cols, asc)
    assert np.array_equal(got(ctx, cols, asc), want)
    assert np.array_equal(got(ctx, cols, None), ref_lexsort(cols, [True] * n_keys))   # ascending=None: all ascending


def test_signed_zeros_tie_and_nan_sorts_after_numbers_before_nulls(ctx):
    v = [0.0, -0.0, np.nan, 1.0, -0.0, 0.0, -np.inf, np.nan, np.inf, 0.0, -1.0, np.nan]
    nulls = [False] * 12
    nulls[3] = nulls[9] = True
    col = Col(L.F64, v, nulls)
    for asc in (True, False):
        g = got(ctx, [col], [asc])
        assert np.array_equal(g, ref_cmp([col], [asc]))
        assert list(g[-2:]) == [3, 9] and list(g[-5:-2]) == [2, 7, 11]   # nulls last, NaNs just before, in row order
    assert list(got(ctx, [col], [True])[:6]) == [6, 10, 0, 1, 4, 5]      # -inf, -1, then the four zeros in row order


def test_strings_order_by_bytes_not_by_code(ctx):
    rng = np.random.default_rng(7)
    col = make_col(rng, L.U32CODE, 3000, null_p=0.1)
    for asc in (True, False):
        g = got(ctx, [col], [asc])
        assert np.array_equal(g, ref_cmp([col], [asc]))
        assert not np.array_equal(g, np.argsort(col.values, kind="stable"))   # code order would be wrong


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 65537, 1_000_003])
def test_sizes_around_the_tile(ctx, n):
    rng = np.random.default_rng(n)
    if n == 0:
        out = ctx.sort_indices([(np.zeros(0, np.int64), None, L.I64)], 0)
        assert out.numel() == 0
        return
    col = Col(L.I64, rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True) if n > 10 else rng.integers(0, 3, n))
    col2 = make_col(rng, L.F64, n, distinct=9, null_p=0.05)
    for cols, asc in (([col], [True]), ([col2, col], [False, True])):
        assert np.array_equal(got(ctx, cols, asc), ref_lexsort(cols, asc))


def test_sorted_reversed_and_one_key(ctx):
    n = 100_000
    a = np.arange(n, dtype=np.int64) * 3 - 7
    ident = np.arange(n)
    assert np.array_equal(got(ctx, [Col(L.I64, a)], [True]), ident)
    assert np.array_equal(got(ctx, [Col(L.I64, a)], [False]), ident[::-1])
    assert np.array_equal(got(ctx, [Col(L.I64, a[::-1].copy())], [True]), ident[::-1])
    for dtype, v in ((L.I64, np.full(n, -5)), (L.F64, np.full(n, 2.5)), (L.BOOLBITS, np.ones(n, bool)),
                     (L.F64, np.where(np.arange(n) % 2, 0.0, -0.0))):
        for asc in (True, False):                       # all rows on one key: the identity, both directions
            assert np.array_equal(got(ctx, [Col(dtype, v)], [asc]), ident)


def test_keys_wider_than_64_bits(ctx):
    rng = np.random.default_rng(3)
    n = 300_000
    full = lambda: rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    # three full-range i64 columns (192 bits), ties on the first two so that every word decides somewhere
    c0 = Col(L.I64, full()[rng.integers(0, 50, n)])
    c1 = Col(L.I64, full()[rng.integers(0, 40, n)], rng.random(n) < 0.1)
    c2 = Col(L.I64, full())
    for asc in ([True, True, True], [False, True, False]):
        assert np.array_equal(got(ctx, [c0, c1, c2], asc), ref_lexsort([c0, c1, c2], asc))


def test_full_range_64_bit_key_at_50m_rows_matches_torch(ctx):
    import torch
    n = 50_000_000
    g = torch.Generator(device="cuda:0").manual_seed(11)
    x = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    x[::1000] = x[5]                                    # repeated values: stability is visible
    want = torch.sort(x, stable=True).indices
    out = ctx.sort_indices([(x, None, L.I64)], n, [True])
    assert torch.equal(out, want)
    want_d = torch.sort(x, stable=True, descending=True).indices
    assert torch.equal(ctx.sort_indices([(x, None, L.I64)], n, [False]), want_d)


def test_narrow_key_above_2_pow_31_rows(ctx):
    """One call between 2^31 and 2^32 rows, a one-bit key: the expected permutation is every 0-row ascending, then
    every 1-row ascending.  Checked without a host sort: the first z entries are strictly increasing rows holding 0,
    the rest strictly increasing rows holding 1, z = the number of 0-rows."""
    import torch
    n = (1 << 31) + 12_345
    g = torch.Generator(device="cuda:0").manual_seed(5)
    bits = torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device="cuda:0", generator=g)
    out = ctx.sort_indices([(bits, None, L.BOOLBITS)], n, [True])
    assert out.numel() == n
    step = 1 << 28
    ones = 0
    for s in range(0, n, step):
        e = min(n, s + step)
        r = torch.arange(s, e, device="cuda:0", dtype=torch.int64)
        ones += int(((bits[r >> 3] >> (r & 7).to(torch.uint8)) & 1).sum())
        del r
    z = n - ones
    prev_last = {0: -1, 1: -1}
    for s in range(0, n, step):
        e = min(n, s + step)
        seg = out[s:e]
        b = (bits[seg >> 3] >> (seg & 7).to(torch.uint8)) & 1
        want_bit = (torch.arange(s, e, device="cuda:0") >= z).to(torch.uint8)
        assert torch.equal(b, want_bit)
        assert bool((seg[1:] > seg[:-1])[(want_bit[1:] == want_bit[:-1])].all())
        for v in (0, 1):
            part = seg[want_bit == v]
            if part.numel():
                assert int(part[0]) > prev_last[v]
                prev_last[v] = int(part[-1])
        del seg, b, want_bit


# ---- frame level ----------------------------------------------------------------------------------------------------------
def _frame(rng, n):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    nul = lambda p: rng.random(n) < p
    df.add_column("f", F.Float64Column.with_nulls(list(rng.choice([1.5, -0.0, 0.0, np.nan, 2.0], n)), nul(0.2)))
    df.add_column("i", F.Int64Column.with_nulls(list(rng.integers(-3, 3, n)), nul(0.1)))
    df.add_column("s", F.StringColumn.with_nulls(list(rng.choice(STRINGS, n)), nul(0.15)))
    df.add_column("b", F.BooleanColumn.with_nulls(list(rng.random(n) < 0.5), nul(0.1)))
    df.add_column("row", F.Int64Column(list(range(n))))
    return df


def _frame_cols(df, names):
    import pandrs_amd.frame as F
    out = []
    for name in names:
        c = df.column(name)
        nulls = None if c.null_mask is None else np.unpackbits(c.null_mask, bitorder="little")[:c.len()].astype(bool)
        if c.dtype == L.U32CODE:
            out.append(Col(L.U32CODE, c.data, nulls, F.GLOBAL_STRING_POOL._strings))
        elif c.dtype == L.BOOLBITS:
            out.append(Col(L.BOOLBITS, np.unpackbits(c.data, bitorder="little")[:c.len()].astype(bool), nulls))
        else:
            out.append(Col(c.dtype, c.data, nulls))
    return out


def test_sort_by_columns_frame_equals_the_restatement(ctx):
    rng = np.random.default_rng(21)
    n = 3000
    df = _frame(rng, n)
    by, asc = ["s", "f", "b", "i"], [False, True, False, True]
    want = ref_cmp(_frame_cols(df, by), asc)
    r = df.sort_by_columns(by, asc)
    assert r.column_names == df.column_names                       # the input's column order is kept
    assert r.row_count() == n
    for name in df.column_names:
        src, dst = df.column(name), r.column(name)
        assert dst.null_mask is None                                # no null masks in the result
        for k in range(n):
            v = src.get(int(want[k]))
            w = dst.get(k)
            if v is None:                                           # nulls become the type's default
                assert w == {L.I64: 0, L.F64: 0.0, L.U32CODE: "", L.BOOLBITS: False}[src.dtype]
            elif isinstance(v, float) and math.isnan(v):
                assert math.isnan(w)
            else:
                assert w == v and type(w) is type(v)
    r1 = df.sort_by("i", False)
    assert list(r1.column("row").data) == list(ref_cmp(_frame_cols(df, ["i"]), [False]))


def test_empty_frame_has_no_columns(ctx):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("a", F.Int64Column([]))
    df.add_column("b", F.StringColumn([]))
    r = df.sort_by_columns(["a", "b"], [True, False])
    assert r.column_count() == 0 and r.row_count() == 0


# ---- other paths ------------------------------------------------------------------------------------------------------------
def test_resident_and_host_keys_agree(ctx):
    rng = np.random.default_rng(8)
    n = 200_000
    cols = [make_col(rng, L.U32CODE, n, null_p=0.1), make_col(rng, L.F64, n, distinct=20, null_p=0.1), make_col(rng, L.BOOLBITS, n)]
    res = [ctx.upload_column(c.data, c.mask, c.dtype) if c.dtype != L.BOOLBITS else ctx.upload_column_n(c.data, c.mask, c.dtype, n)
           for c in cols]
    asc = [True, False, True]
    rank = rank_of(STRINGS)
    host = ctx.sort_indices([c.triple() for c in cols], n, asc, rank).cpu().numpy()
    dev = ctx.sort_indices(res, n, asc, rank).cpu().numpy()
    assert np.array_equal(host, dev) and np.array_equal(host, ref_lexsort(cols, asc))
    for r in res:
        r.release()


def test_string_key_without_or_with_a_short_rank_table_is_invalid(ctx):
    import pandrs_amd as pa
    col = Col(L.U32CODE, np.array([0, 5, 2], np.uint32), None, STRINGS)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.sort_indices([col.triple()], 3, None, None)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "code_rank" in str(e.value)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.sort_indices([col.triple()], 3, None, rank_of(STRINGS)[:5])   # code 5 >= 5 codes
    assert e.value.status == L.ERR_INVALID_ARGUMENT and "n_codes" in str(e.value)
    with pytest.raises(pa.PandrsHipError) as e:
        ctx.sort_indices([(np.zeros(3, np.uint64), None, L.CELL64)], 3)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    assert np.array_equal(got(ctx, [col], [True]), [0, 2, 1])            # the context still works


def test_memory_limit_and_threshold():
    import pandrs_amd as pa
    lib = L.load()
    rng = np.random.default_rng(4)
    try:
        cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        big = Col(L.I64, rng.integers(-2**63, 2**63 - 1, 2_000_000, dtype=np.int64, endpoint=True))
        with pytest.raises(pa.PandrsHipError) as e:
            got(c, [big], [True])
        assert e.value.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e.value)
        small = Col(L.I64, rng.integers(-9, 9, 1000))
        assert np.array_equal(got(c, [small], [False]), ref_lexsort([small], [False]))   # the same context still works
        c.close()
        cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        with pytest.raises(pa.BelowThreshold) as e:
            got(c, [small], [True])
        assert e.value.status == L.ERR_BELOW_THRESHOLD
        mid = Col(L.I64, rng.integers(-9, 9, 20_000))
        assert np.array_equal(got(c, [mid], [True]), ref_lexsort([mid], [True]))
        c.close()
    finally:
        lib.pandrs_hip_init(None)
        pa.Context(0).close()        # resets the limit


def test_cpp_mirror_sorts_a_frame():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sort_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "sort_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
