"""pandrs_hip_filter_indices / pandrs_hip_filter_gather and the mirrors' filter / filter_rows / par_filter / select_by_mask and the
lazy Select and Filter arms (reference src/optimized/split_dataframe/data_ops.rs:15-121, row_ops.rs:26-130, parallel.rs:21-230,
select.rs:150-226, lazy.rs:172-182) against numpy restatements of the reference's loop: row i is selected iff the condition
is Some(true) (np.flatnonzero(values & ~nulls)), and a selected null cell becomes 0 / 0.0 / "" / false."""
import ctypes as C
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

NP_OF = {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32}


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


def cond_of(rng, n, p, null_p=0.0):
    values = rng.random(n) < p
    nulls = rng.random(n) < null_p if null_p else np.zeros(n, bool)
    return values, nulls, (bits(values), bits(nulls) if null_p else None, L.BOOLBITS)


def want_rows(values, nulls):
    return np.flatnonzero(values & ~nulls).astype(np.int64)


def src_of(rng, dtype, n, null_p):
    nulls = rng.random(n) < null_p
    if dtype == L.I64:
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    elif dtype == L.F64:
        v = rng.normal(0, 1e6, n)
        v[rng.random(n) < 0.05] = np.nan
    elif dtype == L.U32CODE:
        v = rng.integers(0, 2**32 - 1, n, dtype=np.uint32, endpoint=True)
    else:
        v = rng.random(n) < 0.5
    data = bits(v) if dtype == L.BOOLBITS else v
    return v, nulls, (data, bits(nulls) if null_p else None, dtype)


def want_values(v, nulls, rows, dtype, fill):
    if dtype == L.BOOLBITS:
        return np.where(nulls[rows], 0, v[rows]).astype(np.uint8)
    return np.where(nulls[rows], np.asarray(fill, NP_OF[dtype]), v[rows]).astype(NP_OF[dtype])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the selection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.001, 0.01, 0.5, 0.99, 1.0])
@pytest.mark.parametrize("null_p", [0.0, 0.3])
def test_indices_at_every_selectivity(ctx, p, null_p):
    rng = np.random.default_rng(int(p * 1000) + int(null_p * 10))
    n = 300_007
    values, nulls, cond = cond_of(rng, n, p, null_p)
    idx, cnt = ctx.filter_indices(cond, n)
    want = want_rows(values, nulls)
    assert cnt == len(want) and np.array_equal(idx.cpu().numpy(), want)
    _, cnt2 = ctx.filter_indices(cond, n, indices=False)                  # the count alone
    assert cnt2 == len(want)


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 4095, 4096, 4097, 8191, 8193, 12_289, 65_537, 1_000_003])
def test_row_counts_around_bytes_words_and_tiles(ctx, n):
    rng = np.random.default_rng(n + 1)
    values, nulls, cond = cond_of(rng, n, 0.6, 0.2)
    data = np.packbits(values, bitorder="little")
    if n % 8:
        data[-1] |= np.uint8(0xFF << (n % 8) & 0xFF)                     # bits past the last row are not rows
    cond = (data, cond[1], L.BOOLBITS)
    idx, cnt = ctx.filter_indices(cond, n)
    want = want_rows(values, nulls)
    assert cnt == len(want) and np.array_equal(idx.cpu().numpy(), want)
    v, sn, src = src_of(rng, L.F64, n, 0.1)
    assert same_bits(ctx.filter_gather(src, n, cnt, 0.0), want_values(v, sn, want, L.F64, 0.0))


def test_clustered_and_unaligned_device_conditions(ctx):
    import torch
    n = 1_000_000
    values = np.zeros(n, bool)
    for s in (0, 4096 * 3 + 5, 200_000, 999_000):                      # runs across tile edges, one up to the last row
        values[s:s + 50_000] = True
    want = want_rows(values, np.zeros(n, bool))
    b = bits(values)
    for off in (0, 1, 3):                                               # device bit arrays at any byte offset
        buf = torch.zeros(len(b) + 8, dtype=torch.uint8, device="cuda:0")
        buf[off:off + len(b)] = torch.from_numpy(b).to("cuda:0")
        idx, cnt = ctx.filter_indices((buf[off:off + len(b)], None, L.BOOLBITS), n)
        assert cnt == len(want) and torch.equal(idx.cpu(), torch.from_numpy(want))


def test_condition_must_be_boolean(ctx):
    import pandrs_amd as pa
    with pytest.raises(pa.ColumnTypeMismatch) as e:
        ctx.filter_indices((np.zeros(10, np.int64), None, L.I64), 10)
    assert e.value.status == L.ERR_TYPE_MISMATCH


# ---- compaction ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [L.I64, L.F64, L.U32CODE, L.BOOLBITS])
@pytest.mark.parametrize("p", [0.01, 0.5, 0.99])
def test_every_dtype_bit_for_bit_with_nulls_as_the_fill(ctx, dtype, p):
    rng = np.random.default_rng(dtype * 7 + int(p * 100))
    n = 250_003
    values, nulls, cond = cond_of(rng, n, p, 0.1)
    _, cnt = ctx.filter_indices(cond, n, indices=False)
    rows = want_rows(values, nulls)
    fill = {L.I64: 0, L.F64: 0.0, L.U32CODE: 17, L.BOOLBITS: 0}[dtype]
    for null_p in (0.0, 0.2):
        v, sn, src = src_of(rng, dtype, n, null_p)
        assert same_bits(ctx.filter_gather(src, n, cnt, fill), want_values(v, sn, rows, dtype, fill))


def test_host_device_and_resident_columns_agree(ctx):
    import torch
    rng = np.random.default_rng(9)
    n = 400_001
    values, nulls, cond = cond_of(rng, n, 0.4, 0.1)
    rows = want_rows(values, nulls)
    res_cond = ctx.upload_column_n(cond[0], cond[1], L.BOOLBITS, n)
    dev_cond = (torch.from_numpy(cond[0]).to("cuda:0"), torch.from_numpy(cond[1]).to("cuda:0"), L.BOOLBITS)
    for c in (cond, dev_cond, res_cond):
        idx, cnt = ctx.filter_indices(c, n)
        assert np.array_equal(idx.cpu().numpy(), rows)
        for dtype in (L.I64, L.F64, L.U32CODE, L.BOOLBITS):
            v, sn, src = src_of(rng, dtype, n, 0.2)
            want = want_values(v, sn, rows, dtype, 0)
            res = ctx.upload_column_n(src[0], src[1], dtype, n)
            dev = (torch.from_numpy(src[0].view(np.int32) if dtype == L.U32CODE else src[0]).to("cuda:0"),
                   torch.from_numpy(src[1]).to("cuda:0"), dtype)
            for s in (src, res, dev):
                assert same_bits(ctx.filter_gather(s, n, cnt, 0), want)
            res.release()
    res_cond.release()


def test_gather_needs_a_matching_selection():
    import pandrs_amd as pa
    c = pa.Context(0)
    try:
        col = (np.arange(10, dtype=np.int64), None, L.I64)
        with pytest.raises(pa.PandrsHipError) as e:                     # a fresh context retains no selection
            c.filter_gather(col, 10, 0)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "selection" in str(e.value)
        _, cnt = c.filter_indices((bits([1, 0] * 5), None, L.BOOLBITS), 10)
        assert cnt == 5
        with pytest.raises(pa.PandrsHipError) as e:
            c.filter_gather((np.arange(11, dtype=np.int64), None, L.I64), 11, cnt)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "11 rows" in str(e.value)
        with pytest.raises(pa.PandrsHipError) as e:
            c.filter_gather((np.zeros(10, np.uint64), None, L.CELL64), 10, cnt)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        assert np.array_equal(c.filter_gather(col, 10, cnt), [0, 2, 4, 6, 8])     # the selection survives refused calls
        with pytest.raises(pa.ColumnTypeMismatch):
            c.filter_indices((np.zeros(10, np.int64), None, L.I64), 10)
        assert np.array_equal(c.filter_gather(col, 10, cnt), [0, 2, 4, 6, 8])     # ... refused before it is touched
    finally:
        c.close()


def test_50m_rows_match_torch_boolean_indexing(ctx):
    import torch
    n = 50_000_000
    g = torch.Generator(device="cuda:0").manual_seed(3)
    mask = torch.rand(n, device="cuda:0", generator=g) < 0.5
    x = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=g)
    packed = (mask.view(-1, 8).to(torch.uint8) << torch.arange(8, device="cuda:0", dtype=torch.uint8)).sum(1, dtype=torch.uint8)
    idx, cnt = ctx.filter_indices((packed, None, L.BOOLBITS), n)
    want_idx = torch.nonzero(mask).flatten()
    assert cnt == want_idx.numel() and torch.equal(idx, want_idx)
    got = ctx.filter_gather((x, None, L.F64), n, cnt, out_device=True)
    assert torch.equal(got.view(torch.int64), x[mask].view(torch.int64))


def test_one_call_above_2_pow_31_rows(ctx):
    """n = 2^31 + 12 345 rows: the selected rows are exact iff they are strictly increasing, each has its bit set and
    there are as many as set bits; a u32 column holding the row number must compact to those same rows."""
    import torch
    n = (1 << 31) + 12_345
    g = torch.Generator(device="cuda:0").manual_seed(5)
    b = torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device="cuda:0", generator=g)
    b[-1] = 0xFF                                                        # bits past the last row set: must not count
    idx, cnt = ctx.filter_indices((b, None, L.BOOLBITS), n)
    step = 1 << 28
    ones = 0
    for s in range(0, n, step):
        e = min(n, s + step)
        r = torch.arange(s, e, device="cuda:0", dtype=torch.int64)
        ones += int(((b[r >> 3] >> (r & 7).to(torch.uint8)) & 1).sum())
        del r
    assert cnt == ones and idx.numel() == cnt
    assert int(idx[-1]) < n and int(idx[-1]) >= (1 << 31)
    for s in range(0, cnt, step):
        seg = idx[s:min(cnt, s + step + 1)]
        assert bool((seg[1:] > seg[:-1]).all())
        assert bool((((b[seg >> 3] >> (seg & 7).to(torch.uint8)) & 1) == 1).all())
        del seg
    rows = torch.arange(n, dtype=torch.int64, device="cuda:0").to(torch.int32)     # row numbers as u32 codes
    got = ctx.filter_gather((rows, None, L.U32CODE), n, cnt, out_device=True)
    del rows
    for s in range(0, cnt, step):
        assert torch.equal(got[s:s + step], idx[s:s + step].to(torch.int32))


# ---- frame level ----------------------------------------------------------------------------------------------------------
def _frame(rng, n, cond_p=0.5, cond_null_p=0.2):
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    nul = lambda p: rng.random(n) < p
    df.add_column("id", F.Int64Column(np.arange(n)))
    df.add_column("i", F.Int64Column.with_nulls(rng.integers(-9, 9, n), nul(0.1)))
    df.add_column("f", F.Float64Column.with_nulls(rng.normal(0, 1, n), nul(0.2)))
    df.add_column("s", F.StringColumn.with_nulls(list(rng.choice(["a", "bb", "", "é"], n)), nul(0.15)))
    df.add_column("b", F.BooleanColumn.with_nulls(rng.random(n) < 0.5, nul(0.1)))
    df.add_column("flag", F.BooleanColumn.with_nulls(rng.random(n) < cond_p, nul(cond_null_p)))
    return df


def _expect(df, rows):
    """The reference loop: column by column, Some(v) -> v, None -> the type's default."""
    defaults = {L.I64: 0, L.F64: 0.0, L.U32CODE: "", L.BOOLBITS: False}
    out = {}
    for name in df.column_names:
        c = df.column(name)
        out[name] = [defaults[c.dtype] if c.get(int(r)) is None else c.get(int(r)) for r in rows]
    return out


def _values(df):
    return {name: [df.column(name).get(k) for k in range(df.row_count())] for name in df.column_names}


def test_filter_filter_rows_and_par_filter_equal_the_reference_loop(ctx):
    rng = np.random.default_rng(31)
    n = 5000
    df = _frame(rng, n)
    flag = df.column("flag")
    rows = [i for i in range(n) if flag.get(i) is True]
    want = _expect(df, rows)
    for method in (df.filter, df.filter_rows, df.par_filter):
        r = method("flag")
        assert r.column_names == df.column_names and r.row_count() == len(rows)
        assert all(r.column(name).null_mask is None for name in r.column_names)
        assert _values(r) == want
        assert [type(r.column(name)) for name in r.column_names] == [type(df.column(name)) for name in df.column_names]


def test_select_by_mask_equals_select_rows_by_indices(ctx):
    rng = np.random.default_rng(32)
    n = 3001
    df = _frame(rng, n)
    mask = rng.random(n) < 0.3
    r = df.select_by_mask(list(mask))
    assert r.column_names == df.column_names and r.row_count() == int(mask.sum())
    assert _values(r) == _expect(df, np.flatnonzero(mask))


def test_empty_result_shapes(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(33)
    df = _frame(rng, 1000, cond_p=0.0)                                  # nothing Some(true): false or null everywhere
    for method in (df.filter, df.filter_rows, df.par_filter):           # every column kept, typed, 0 rows
        r = method("flag")
        assert r.column_names == df.column_names and r.row_count() == 0
        assert [type(r.column(name)) for name in r.column_names] == [type(df.column(name)) for name in df.column_names]
    r = df.select_by_mask(np.zeros(1000, bool))                          # select_rows_by_indices_impl: no columns
    assert r.column_count() == 0 and r.row_count() == 0
    assert isinstance(df.select_by_mask(np.zeros(1000, bool)), F.OptimizedDataFrame)


def test_reference_test_optimized_dataframe_filter(ctx):
    """tests/optimized_dataframe_test.rs:159-186."""
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("id", F.Int64Column([1, 2, 3, 4]))
    df.add_column("filter", F.BooleanColumn([True, False, True, False]))
    filtered = df.filter("filter")
    assert filtered.row_count() == 2
    assert list(filtered.column("id").data) == [1, 3]
    with pytest.raises(F.ColumnNotFound):
        df.filter("nonexistent")
    df2 = F.OptimizedDataFrame()
    df2.add_column("id", F.Int64Column([1, 2, 3, 4]))
    with pytest.raises(F.ColumnTypeMismatch):
        df2.filter("id")


def test_resident_style_device_frames_and_many_filters_in_a_row(ctx):
    rng = np.random.default_rng(34)
    df = _frame(rng, 20_000)
    a = df.filter("flag")
    b = a.filter("b")                                                   # b has no nulls after the first filter
    rows = [i for i in range(df.row_count()) if df.column("flag").get(i) is True and df.column("b").get(i) is True]
    assert list(b.column("id").data) == rows


def test_lazy_filter_then_aggregate(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(35)
    n = 50_000
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column(rng.integers(0, 50, n)))
    df.add_column("v", F.Float64Column(rng.normal(0, 1, n)))
    df.add_column("flag", F.BooleanColumn.with_nulls(rng.random(n) < 0.4, rng.random(n) < 0.1))
    aggs = [("v", F.AggregateOp.Min, "lo"), ("v", F.AggregateOp.Max, "hi"), ("v", F.AggregateOp.Count, "n"),
            ("v", F.AggregateOp.Sum, "total")]
    got = _by_key(F.LazyFrame.new(df).filter("flag").aggregate(["k"], aggs).execute(), "k")
    want = _by_key(df.par_filter("flag").group_by_with_options(["k"], False).aggregate(aggs), "k")
    assert got.keys() == want.keys() and len(want) == 50
    for k, w in want.items():
        assert got[k][:3] == w[:3]                                      # min / max / count exact
        assert abs(got[k][3] - w[3]) <= 1e-9 * max(1.0, abs(w[3]))


def _by_key(df, key):
    vals = _values(df)
    others = [name for name in df.column_names if name != key]
    return {vals[key][r]: tuple(vals[name][r] for name in others) for r in range(df.row_count())}


def test_lazy_select_filter_join_aggregate(ctx):
    import pandrs_amd.frame as F
    rng = np.random.default_rng(36)
    n, m = 40_000, 500
    left = F.OptimizedDataFrame()
    left.add_column("key", F.Int64Column(rng.integers(0, m, n)))
    left.add_column("v", F.Float64Column(rng.normal(0, 1, n)))
    left.add_column("junk", F.StringColumn(list(rng.choice(["x", "y"], n))))
    left.add_column("flag", F.BooleanColumn(rng.random(n) < 0.5))
    right = F.OptimizedDataFrame()
    right.add_column("key", F.Int64Column(np.arange(m)))
    right.add_column("g", F.StringColumn(["g%d" % (i % 7) for i in range(m)]))
    aggs = [("v", F.AggregateOp.Sum, "total")]
    lz = (F.LazyFrame.new(left).select(["key", "v", "flag"]).filter("flag")
          .join(right, "key", "key", F.JoinType.Inner).aggregate(["g"], aggs))
    got = lz.execute()                                                  # the Join -> Aggregate(Sum) peephole after a Filter
    step = left.select(["key", "v", "flag"]).par_filter("flag").inner_join(right, "key", "key")
    want = step.group_by_with_options(["g"], False).aggregate(aggs)
    gd, wd = _values(got), _values(want)
    assert sorted(gd["g"]) == sorted(wd["g"])
    gm, wm = dict(zip(gd["g"], gd["total"])), dict(zip(wd["g"], wd["total"]))
    for k in wm:
        assert abs(gm[k] - wm[k]) <= 1e-9 * max(1.0, abs(wm[k]))


def test_memory_limit_and_threshold():
    import pandrs_amd as pa
    lib = L.load()
    rng = np.random.default_rng(4)
    try:
        cfg = L.Config(enabled=1, device_id=0, memory_limit=8 << 20, fallback_to_cpu=1, use_pinned_memory=0, min_size_threshold=0)
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        n = 100_000_000                                                 # 12.5 MB of selection words > 8 MB
        big = (np.zeros((n + 7) // 8, np.uint8), None, L.BOOLBITS)
        with pytest.raises(pa.PandrsHipError) as e:
            c.filter_indices(big, n, indices=False)
        assert e.value.status == L.ERR_OUT_OF_MEMORY and "memory_limit" in str(e.value)
        values, nulls, small = cond_of(rng, 1000, 0.5, 0.1)
        idx, cnt = c.filter_indices(small, 1000)                        # the same context still works
        assert np.array_equal(idx.cpu().numpy(), want_rows(values, nulls))
        c.close()
        cfg.memory_limit, cfg.min_size_threshold = 0, 10_000
        assert lib.pandrs_hip_init(C.byref(cfg)) == 0
        c = pa.Context(0)
        with pytest.raises(pa.BelowThreshold) as e:
            c.filter_indices(small, 1000)
        assert e.value.status == L.ERR_BELOW_THRESHOLD
        with pytest.raises(pa.BelowThreshold):
            c.filter_gather((np.zeros(1000, np.int64), None, L.I64), 1000, 0)
        values, nulls, mid = cond_of(rng, 20_000, 0.5)
        idx, cnt = c.filter_indices(mid, 20_000)
        assert np.array_equal(idx.cpu().numpy(), want_rows(values, nulls))
        c.close()
    finally:
        lib.pandrs_hip_init(None)
        pa.Context(0).close()        # resets the limit


def test_cpp_mirror_filters_a_frame():
    import __graft_entry__ as g
    g.build()
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "filter_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "filter_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "2 tests, 0 failed checks" in r.stdout
