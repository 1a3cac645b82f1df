"""The hash join at the edges of its build, probe and emit kernels (pandrs_amd/csrc/join.hip).

tests/test_gpu_join.py draws mid-sized random keys; here every input sits ON a structural boundary — row counts around a wave,
a workgroup and a 2048-row tile, the one matching row at a tile / row-slice / wave edge, build-side runs around BH_MAXRUN, a
partition at, one below and one above what a region takes, the general path's threshold, the scan's batch and segment lengths —
and every boundary is derived from the constants that tests/join_ref.py reads out of the kernels' source.  The cases come from
join_ref.edge_cases (sections a. to i.; tests/test_join_ref.py checks them against a plain dictionary loop on the CPU); expected
pairs always come from oracle.join_indices and are compared IN ORDER, exactly.

What timings() can and cannot show: `retries` proves that a partition overflowed its region and the call was repeated (d., e.),
and `retries == 0` with more rows than a region takes proves the general path was taken from the start.  The bitonic fallback
inside join_build_kernel and the walk past an overflowing bucket leave no trace in timings(): those cases are built from the
constants so that the path MUST be taken (a run of BH_MAXRUN + 1 rows; a region at 7/8 load), and are checked by their pairs only.
"""
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import join_ref as J
from tests.helpers import assert_groupby_equal

pytestmark = pytest.mark.gpu
K = J.join_constants()
TILE, MAXRUN, LDS_MAX = K["TILE"], K["BH_MAXRUN"], K["BH_MAXROWS"]
HOW_NAME = {O.INNER: "inner", O.LEFT: "left", O.RIGHT: "right", O.OUTER: "outer"}


@pytest.fixture(scope="module")
def ctx():
    import pandrs_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


_want = {}


def expected(case, how):
    """oracle.join_indices of a case, computed once (the probe option does not change the inputs) and never modified."""
    key = (case["name"].replace("_onepass", "").replace("_threekernel", ""), how)
    if key not in _want:
        wl, wr = O.join_indices(case["lkey"], case["nl"], case["rkey"], case["nr"], how)
        wl.setflags(write=False)
        wr.setflags(write=False)
        _want[key] = (wl, wr)
    return _want[key]


def run_case(ctx, case, options=None, lkey=None, rkey=None):
    """Every join type of the case against the oracle, in order; -> the `retries` of every call."""
    options = case["options"] if options is None else options
    lkey, rkey = lkey or case["lkey"], rkey or case["rkey"]
    retries = []
    for name, v in options.items():
        ctx.set_option(name, v)
    try:
        for how in case["hows"]:
            gl, gr = ctx.join_indices(lkey, case["nl"], rkey, case["nr"], how)
            retries.append(ctx.timings()["retries"])
            if hasattr(gl, "cpu"):
                gl, gr = gl.cpu().numpy(), gr.cpu().numpy()
            wl, wr = expected(case, how)
            msg = "%s %s %s" % (case["name"], HOW_NAME[how], options)
            assert len(gl) == len(wl), (msg, len(gl), len(wl))
            np.testing.assert_array_equal(gl, wl, err_msg=msg)
            np.testing.assert_array_equal(gr, wr, err_msg=msg)
    finally:
        for name in options:
            ctx.set_option(name, 0)
    return retries


# ---- a. row counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", ["threekernel", "onepass"])
def test_a_row_counts(ctx, probe):
    """nl, nr from {0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 TILE + 1}: the diagonal plus (small, large)
    and (large, small); keys uniform over max(nr, 3) values, 2 % nulls on both sides."""
    cases = [c for c in J.edge_cases("a") if c["name"].endswith(probe)]
    sizes = set(J.row_count_sizes())
    assert {c["nl"] for c in cases} == sizes and {c["nr"] for c in cases} == sizes
    for c in cases:
        assert c["options"]["join_one_pass"] == (probe == "onepass")
        run_case(ctx, c)


# ---- b. which left rows match -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("layout", ["b_only_row%d_matches" % r for r in J.match_rows()] + ["b_only_row", "b_all_miss", "b_all_left_null"])
def test_b_matching_rows_against_tile_slice_and_wave_edges(ctx, layout, onepass):
    """nl = 2 TILE + 1.  One left row alone matches (1, 2 or BH_MAXRUN right rows), at rows {0, 63, 64, 255, 256, TILE - 1, TILE,
    TILE + 1, nl - 1}; every row matches but one of those; all miss; all left keys null.  Left / outer place the (l, -1) rows."""
    cases = [c for c in J.edge_cases("b") if c["name"].startswith(layout) and (layout != "b_only_row" or c["name"].endswith("misses"))]
    assert cases and all(c["nl"] == 2 * TILE + 1 for c in cases)
    for c in cases:
        run_case(ctx, c, {"join_one_pass": onepass})


# ---- c. run lengths on the build side ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", J.run_lengths())
def test_c_build_side_run_lengths(ctx, m):
    """One key on m right rows scattered among 500 unique keys, one forced partition: m = 1 is stored as JN_DIRECT, up to
    BH_MAXRUN rows are insertion-sorted, one more sends the partition to the bitonic sort (not visible in timings(): the run
    length makes it certain).  The key is an ordinary one, the sentinel-valued one on both sides, or -1 sits on one side only."""
    cases = [c for c in J.edge_cases("c") if c["name"].startswith("c_run%d_" % m)]
    assert len(cases) == 4
    for c in cases:
        assert c["options"] == {"partitions": 1}
        assert run_case(ctx, c) == [0] * 4
        run_case(ctx, c, {"partitions": 1, "join_one_pass": 1})


# ---- d. rows per partition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in J.edge_cases("d")])
def test_d_rows_per_partition(ctx, name):
    """One forced partition, so rows per partition are exact.  BH_SLOTS / 8 * 7 rows (and one fewer) are the region at its highest
    load — overflowing buckets, long walks, wraps past the region's end, none of it visible in timings() — and must answer with
    retries == 0; one row more, and JN_RCAP * 0.95 rounded down, overflow and retry; one row above JN_RCAP * 0.95 starts on the
    general path (retries == 0 although no region takes that many rows).  Then a run of BH_MAXRUN + 1 rows — the bitonic
    fallback — in partitions of 49 (one key alone), 64, 65, 4096, 4097 and BH_SLOTS / 8 * 7 rows, and on the general path."""
    case = next(c for c in J.edge_cases("d") if c["name"] == name)
    feats = J.join_features(case)
    assert case["options"] == {"partitions": 1} and case["features"] <= feats
    retries = run_case(ctx, case)
    if feats & {"part_lds_max+1", "part_below_general"}:
        assert min(retries) >= 1, retries
    else:
        assert retries == [0] * len(case["hows"]), retries
    if "part_general" in feats:
        assert case["nr"] > LDS_MAX and tuple(case["hows"]) == J.INNER_OUTER


# ---- e. overflow, then retry ----------------------------------------------------------------------------------------------
def test_e_overflow_then_retry(ctx):
    """Two forced partitions, 13 000 build rows, one key on 3 000 of them: its partition exceeds a region, the call retries at
    four times the fan-out and then sorts that partition (run > BH_MAXRUN)."""
    case = next(J.edge_cases("e"))
    assert {"part_overflow_fits_at_4x", "bitonic_after_retry"} <= J.join_features(case)
    retries = run_case(ctx, case)
    assert min(retries) >= 1, retries


def test_e_overflow_then_retry_fused(ctx):
    """The same shape through join_groupby_sum (i64 sums: bit-exact)."""
    lk, rk = J.overflow_retry_sides()
    rng = np.random.default_rng(51)
    rg = rng.integers(0, 40, len(rk)).astype(np.int64)
    lv = rng.integers(-1000, 1000, len(lk)).astype(np.int64)
    args = ((lk, None, O.I64), (lv, None, O.I64), len(lk), (rk, None, O.I64), (rg, None, O.I64), len(rk))
    ctx.set_option("partitions", 2)
    try:
        got = ctx.join_groupby_sum(*args)
        parts = ctx.timings()["n_partitions"]
    finally:
        ctx.set_option("partitions", 0)
    assert_groupby_equal(got, O.join_groupby_sum(*args), [O.I64], int_exact_rows=[0])
    assert parts == 8                       # the fused entry reports its build fan-out: 2 overflowed, 4 x 2 answered


# ---- f. scan batches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3))
def test_f_scan_batches(ctx, i):
    """nl = 1024 TILE, 1024 TILE + 1 and 2 x 1024 TILE + 1 against 1000 unique build keys: tile_scan_kernel's carry across batches
    of 1024 tiles.  The last tile of the first batch and the first tile of the second both emit.  Inner + outer.
    Measured on an MI355X, engine and oracle together (the line this test prints): 0.12 s, 0.13 s and 0.29 s; with the
    generation of the inputs 0.3 s, 0.2 s and 0.5 s per test — the slowest tests of this file."""
    case = list(J.edge_cases("f"))[i]
    assert case["nl"] == J.scan_batch_sizes()[i] and "scan_batch_edge_tiles_emit" in J.join_features(case)
    t0 = time.perf_counter()
    run_case(ctx, case)
    print("scan-batch case nl=%d: %.2f s" % (case["nl"], time.perf_counter() - t0))


# ---- g. single-pass re-size -----------------------------------------------------------------------------------------------
def test_g_single_pass_resize_keeps_unmatched_right_rows(ctx):
    """join_one_pass with every build key three times: the output exceeds the buffer sized for unique keys and the probe runs
    twice, with the `hit` flags cleared in between.  The unmatched right rows must still be exactly the unmatched ones."""
    case = next(J.edge_cases("g"))
    assert {"one_pass_resize", "one_pass_resize_unmatched_right"} <= J.join_features(case) and case["options"] == {"join_one_pass": 1}
    run_case(ctx, case)
    from oracle import oracle_np as ONP
    lnul, lcell = ONP.key_cells(case["lkey"], case["nl"])
    rnul, rcell = ONP.key_cells(case["rkey"], case["nr"])
    unmatched = np.flatnonzero((rnul == 1) | ~np.isin(rcell, lcell[lnul == 0]))
    assert 0 < len(unmatched) < case["nr"]
    ctx.set_option("join_one_pass", 1)
    try:
        for how in (O.RIGHT, O.OUTER):
            gl, gr = ctx.join_indices(case["lkey"], case["nl"], case["rkey"], case["nr"], how)
            np.testing.assert_array_equal(gr[gl < 0], unmatched)
    finally:
        ctx.set_option("join_one_pass", 0)


# ---- h. unmatched right rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("nr", J.scan_seg_sizes())
def test_h_unmatched_right_rows_around_the_scan_segment(ctx, nr, onepass):
    """nr = the segment length of exclusive_scan_u32, +-1, and twice the length + 1; none / all / only the first / only the last
    right row matched, and all right keys null.  Right + outer."""
    cases = [c for c in J.edge_cases("h") if c["nr"] == nr]
    assert len(cases) == 5 and all(tuple(c["hows"]) == (O.RIGHT, O.OUTER) for c in cases)
    for c in cases:
        run_case(ctx, c, {"join_one_pass": onepass})


# ---- i. key types and memory spaces -----------------------------------------------------------------------------------
def place(ctx, space, col, n, keep):
    """A host (data, mask, dtype) column as the engine takes it in `space`.  device_offset: the data 8 bytes into its allocation
    (4 for u32 codes), masks and bit-packed data 3 bytes into theirs."""
    import torch
    data, mask, dt = col
    if space == "host":
        return col
    if space == "resident":
        r = ctx.upload_column_n(np.ascontiguousarray(data), None if mask is None else np.ascontiguousarray(mask), dt, n)
        keep.append(r)
        return r
    tdt = {O.I64: torch.int64, O.F64: torch.float64, O.U32CODE: torch.int32, O.BOOLBITS: torch.uint8}[dt]

    def dev(a, lead, as_dtype):
        raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy())
        buf = torch.full((len(raw) + lead + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        buf[lead:lead + len(raw)] = raw.to("cuda:0")
        return buf[lead:lead + len(raw)].view(as_dtype)
    off = space == "device_offset"
    lead = 0 if not off else 3 if dt == O.BOOLBITS else 4 if dt == O.U32CODE else 8
    return (dev(data, lead, tdt), None if mask is None else dev(mask, 3 if off else 0, torch.uint8), dt)


@pytest.mark.parametrize("space", ["host", "device", "device_offset", "resident"])
@pytest.mark.parametrize("kind", ["i_f64", "i_u32", "i_bool"])
def test_i_key_types_and_memory_spaces(ctx, kind, space):
    """F64 keys from {0.0, -0.0, NaN, NaN with another payload, inf, -inf, 1.5}; u32 codes; bit-packed bools with nl, nr no
    multiples of 8 and stray bits past the last row in data and null mask — from host arrays, device tensors, device tensors at
    an offset and resident columns."""
    case = next(c for c in J.edge_cases("i") if c["name"] == kind)
    assert case["features"] <= J.join_features(case)
    keep = []
    try:
        lkey, rkey = place(ctx, space, case["lkey"], case["nl"], keep), place(ctx, space, case["rkey"], case["nr"], keep)
        run_case(ctx, case, lkey=lkey, rkey=rkey)
        run_case(ctx, case, {"join_one_pass": 1}, lkey=lkey, rkey=rkey)
    finally:
        for r in keep:
            r.release()


# ---- j. gathers through the retained pairs ------------------------------------------------------------------------------
def _tiny(name, lk, rk, hows):
    return {"name": name, "lkey": (np.asarray(lk, np.int64), None, O.I64), "nl": len(lk), "rkey": (np.asarray(rk, np.int64), None, O.I64),
            "nr": len(rk), "options": {}, "hows": hows}


def _gather_cases():
    c = {x["name"]: x for x in J.edge_cases("ch")}
    yield dict(c["c_run%d_plain" % (MAXRUN + 1)], hows=(O.OUTER,))
    yield dict(c["h_nr%d_only_last_matched" % (K["SCAN_SEG"] + 1)], hows=(O.OUTER,))
    yield _tiny("j_no_output", [1, 2, 3], [4, 5], (O.INNER,))
    yield _tiny("j_only_misses", [1, 2, 3], [4, 5], (O.LEFT,))


@pytest.mark.parametrize("which", range(4))
def test_j_gathers_through_the_retained_pairs(ctx, which):
    """join_gather of either side after an outer join from c. and one from h., after a join without output and after one whose
    output is only misses: F64, I64, U32 and BOOLBITS payloads with and without a null mask, then the key column (key_right).
    Bit for bit against oracle.gather."""
    case = list(_gather_cases())[which]
    how = case["hows"][0]
    rng = np.random.default_rng(70 + which)
    for name, v in case["options"].items():
        ctx.set_option(name, v)
    try:
        gl, gr = ctx.join_indices(case["lkey"], case["nl"], case["rkey"], case["nr"], how)
    finally:
        for name in case["options"]:
            ctx.set_option(name, 0)
    wl, wr = O.join_indices(case["lkey"], case["nl"], case["rkey"], case["nr"], how)
    np.testing.assert_array_equal(gl, wl)
    np.testing.assert_array_equal(gr, wr)
    n_out = len(wl)
    assert (n_out == 0) == (case["name"] == "j_no_output")
    if case["name"] == "j_only_misses":
        assert n_out == case["nl"] and (wr == -1).all()
    for side, n_src, idx in ((0, case["nl"], wl), (1, case["nr"], wr)):
        payloads = [(rng.normal(size=n_src), O.F64, -2.5), (rng.integers(-10 ** 12, 10 ** 12, n_src).astype(np.int64), O.I64, -7),
                    (rng.integers(0, 2 ** 32, n_src).astype(np.uint32), O.U32CODE, 0xFFFFFFFF),
                    (np.packbits(rng.random(n_src) < 0.5, bitorder="little"), O.BOOLBITS, 0)]
        for data, dt, fill in payloads:
            for mask in (None, O.pack_mask(rng.random(n_src) < 0.3)):
                got = ctx.join_gather((data, mask, dt), n_src, n_out, side, fill)
                want = O.gather(data, mask, idx, fill, dt)
                np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg="%s side %d dtype %d" % (case["name"], side, dt))
    got_k = ctx.join_gather(case["lkey"], case["nl"], n_out, 0, 0, key_right=case["rkey"], n_right=case["nr"])
    a, b = O.gather(*case["lkey"][:2], wl, 0, O.I64), O.gather(*case["rkey"][:2], wr, 0, O.I64)
    np.testing.assert_array_equal(got_k, np.where(wl >= 0, a, b))


# ---- k. fused join -> groupby ---------------------------------------------------------------------------------------------
FJ_FULL = int(K["FJ_GENERAL_ROWS"])                 # FJ_MAXROWS * 0.95 rounded down: the LDS multimap at its fullest


def _fused_sides(rng, nr, nl, dup, groups, masked, sentinel="none"):
    ids = np.repeat(np.arange(1, nr // 3 + 2), 3)[:nr] if dup else rng.permutation(nr * 3)[:nr] + 1
    rk = (ids.astype(np.int64) * J.MULT)[rng.permutation(nr)]
    lk = rk[rng.integers(0, nr, nl)].copy()
    lk[rng.random(nl) < 0.1] = J.MISS0
    if sentinel in ("right", "both"):
        rk[rng.integers(0, nr, 3 if dup else 1)] = -1
    if sentinel in ("left", "both") and nl:
        lk[rng.integers(0, nl, max(nl // 50, 1))] = -1
    if masked:      # a masked u32 group column and a masked f64 value column in [1, 2): both go through clean_payload_kernel
        rg = (rng.integers(0, groups, nr).astype(np.uint32), O.pack_mask(rng.random(nr) < 0.1), O.U32CODE)
        lv = (1.0 + rng.random(nl), J._mask(rng, nl, 0.1), O.F64)
    else:
        rg = (rng.integers(-3, groups - 3, nr).astype(np.int64), None, O.I64)
        lv = (rng.integers(-1000, 1000, nl).astype(np.int64), None, O.I64)
    return ((lk, J._mask(rng, nl, 0.02), O.I64), lv, nl, (rk, J._mask(rng, nr, 0.02), O.I64), rg, nr)


def _check_fused(ctx, args, general):
    ctx.set_option("partitions", 1)
    try:
        got = ctx.join_groupby_sum(*args)
        parts = ctx.timings()["n_partitions"]
    finally:
        ctx.set_option("partitions", 0)
    exact = args[1][2] == O.I64
    assert_groupby_equal(got, O.join_groupby_sum(*args), [args[4][2]], int_exact_rows=[0] if exact else [], rtol=1e-9)
    assert parts == (0 if general else 1), parts        # the fused entry reports fan-out 0 for the general fallback


@pytest.mark.parametrize("dup", [0, 1], ids=["unique", "dup3"])
@pytest.mark.parametrize("general", [0, 1], ids=["multimap_fullest", "general_fallback"])
def test_k_fused_join_groupby_at_the_multimap_limit(ctx, general, dup):
    """One forced partition with FJ_MAXROWS * 0.95 (rounded down) build rows — the LDS multimap at its fullest — and one row more,
    the general fallback (pairs_from_indices_kernel).  Unique build keys, and keys three times each (the pair buffer re-sizes);
    nl in {0, 1, TILE, TILE + 1}; 1, 3 and ~2000 distinct group values; plain i64 columns (sums bit-exact) and a masked u32
    group column with masked f64 values in [1, 2) (rtol 1e-9)."""
    nr = FJ_FULL + general
    assert (nr / 1 > K["FJ_GENERAL_ROWS"]) == bool(general)
    rng = np.random.default_rng(1100 + 2 * general + dup)
    for nl in (0, 1, TILE, TILE + 1):
        for groups, masked in ((1, 0), (3, 1), (2000, 0), (2000, 1)):
            _check_fused(ctx, _fused_sides(rng, nr, nl, dup, groups, masked), general)


@pytest.mark.parametrize("sentinel", ["left", "right", "both"])
@pytest.mark.parametrize("general", [0, 1], ids=["multimap_fullest", "general_fallback"])
def test_k_fused_join_sentinel_key_on_either_side(ctx, general, sentinel):
    rng = np.random.default_rng(1200 + general)
    for dup in (0, 1):
        for masked in (0, 1):
            _check_fused(ctx, _fused_sides(rng, FJ_FULL + general, TILE + 1, dup, 3, masked, sentinel), general)
