"""Shared, CPU-only pieces of the hash join's edge tests (tests/test_join_ref.py, tests/test_gpu_join_edges.py).

join_loop       a plain dictionary loop restating join.rs:106-224 on the oracle's key cells: the second opinion on
                oracle.join_indices (slow; a few thousand rows at the most).
join_constants  the tile / table / run-length constants, read out of pandrs_amd/csrc/join.hip (and partition.hip), so that
                every boundary in the tests moves with the kernels.
edge_cases      a deterministic generator of named inputs built ON those boundaries; join_features says, from the inputs
                alone, which structural edges a case reaches, and FEATURES lists every edge the cases must reach together.
"""
import os
import re

import numpy as np

from oracle import oracle as O
from oracle import oracle_np as ONP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pandrs_amd", "csrc")
WAVE = 64                                   # gfx950 wavefront
SENTINEL = -1                               # the i64 whose bits equal the tables' EMPTY_KEY
INNER_OUTER = (O.INNER, O.OUTER)
ALL_HOWS = (O.INNER, O.LEFT, O.RIGHT, O.OUTER)


# ---- the reference loop -----------------------------------------------------------------------------------------------
def join_loop(lkey, nl, rkey, nr, how):
    """join_impl up to join_indices (join.rs:106-224): right map key -> ascending rows (null keys never built), left rows
    ascending (null keys never probed), misses as (l, -1) for left/outer, then the unmatched right rows ascending as (-1, r)
    for right/outer.  Keys compare by oracle_np.key_cells.  -> (left int64[], right int64[])"""
    lnul, lcell = ONP.key_cells(lkey, nl)
    rnul, rcell = ONP.key_cells(rkey, nr)
    right = {}
    for r in range(nr):
        if not rnul[r]:
            right.setdefault(int(rcell[r]), []).append(r)
    li, ri = [], []
    matched = np.zeros(nr, bool)
    for l in range(nl):
        if lnul[l]:
            continue
        rows = right.get(int(lcell[l]))
        if rows is not None:
            for r in rows:
                li.append(l)
                ri.append(r)
                matched[r] = True
        elif how in (O.LEFT, O.OUTER):
            li.append(l)
            ri.append(-1)
    if how in (O.RIGHT, O.OUTER):
        for r in range(nr):
            if not matched[r]:
                li.append(-1)
                ri.append(r)
    return np.array(li, np.int64), np.array(ri, np.int64)


# ---- constants out of the kernels' source -----------------------------------------------------------------------------
_CONST_NAMES = ("JN_RCAP", "BH_SLOTS", "BH_MAXRUN", "LK_THREADS", "LK_RPT", "OP_TILE", "FJ_SLOTS", "FJ_MAXROWS")
_INT = re.compile(r"\b(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?[lL]{0,2})\b")


def _constexprs(text):
    """name -> expression text of every `constexpr <type> A = ..., B = ...;` statement."""
    out = {}
    for stmt in re.findall(r"constexpr\s+(?:unsigned\s+)?(?:long\s+long|\w+)\s+([^;{}]*?=[^;{}]*);", text):
        for part in stmt.split(","):
            m = re.match(r"\s*(\w+)\s*=\s*(.+?)\s*$", part, re.S)
            if m:
                out.setdefault(m.group(1), m.group(2))
    return out


def _evaluate(name, exprs, seen=()):
    if name not in exprs:
        raise KeyError("constant %s is no longer defined in the kernel source" % name)
    if name in seen:
        raise ValueError("constant %s is defined through itself" % name)
    expr = _INT.sub(lambda m: str(int(m.group(1), 0)), exprs[name])
    expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(_evaluate(m.group(0), exprs, seen + (name,))), expr)
    if not re.fullmatch(r"[\d\s*/+\-()<]+", expr):
        raise ValueError("constant %s = %r is not a simple product" % (name, exprs[name]))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))       # digits and operators only (checked above)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


_constants_cache = None


def join_constants():
    """The named constants of join.hip as positive ints, plus what the tests derive from them: TILE (left rows per probe
    tile), BH_MAXROWS (build rows a region takes), GENERAL_ROWS (rows per partition from which the general path starts, a
    float), SCAN_TILES (tiles per batch of tile_scan_kernel), SCAN_SEG (segment of exclusive_scan_u32), JN_SEED, P_MAX."""
    global _constants_cache
    if _constants_cache is not None:
        return dict(_constants_cache)
    src = _read("join.hip")
    exprs = _constexprs(src)
    K = {n: _evaluate(n, exprs) for n in _CONST_NAMES + ("JN_SEED",)}
    K["SCAN_SEG"] = _evaluate("SCAN_SEG", _constexprs(_read("partition.hip")))
    K["P_MAX"] = _evaluate("P_MAX", _constexprs(_read("engine.hpp")))
    m = re.search(r"void\s+tile_scan_kernel.*?base\s*<\s*n_tiles\s*;\s*base\s*\+=\s*(\d+)", src, re.S)
    if not m:
        raise KeyError("tile_scan_kernel's batch length is no longer found in join.hip")
    K["SCAN_TILES"] = int(m.group(1))
    m = re.search(r"nR\s*>\s*BH_SLOTS\s*/\s*(\d+)\s*\*\s*(\d+)", src)
    if not m:
        raise KeyError("join_build_kernel's row limit (BH_SLOTS / 8 * 7) is no longer found in join.hip")
    K["BH_MAXROWS"] = K["BH_SLOTS"] // int(m.group(1)) * int(m.group(2))
    m = re.search(r"\(double\)\s*P\s*>\s*JN_RCAP\s*\*\s*([0-9.]+)", src)
    if not m:
        raise KeyError("join_core's general-path threshold (JN_RCAP * 0.95) is no longer found in join.hip")
    K["GENERAL_ROWS"] = K["JN_RCAP"] * float(m.group(1))
    m = re.search(r"\(double\)\s*P\s*>\s*FJ_MAXROWS\s*\*\s*([0-9.]+)", src)
    if not m:
        raise KeyError("the fused join's general-path threshold (FJ_MAXROWS * 0.95) is no longer found in join.hip")
    K["FJ_GENERAL_ROWS"] = K["FJ_MAXROWS"] * float(m.group(1))
    K["TILE"] = K["LK_THREADS"] * K["LK_RPT"]
    for n, v in K.items():
        if not v > 0:
            raise ValueError("constant %s = %r is not positive" % (n, v))
    _constants_cache = K
    return dict(K)


def hash32(cells, seed):
    """device_utils.hpp hash32 over uint64 cells (vectorised)."""
    c = np.asarray(cells, np.uint64)
    lo, hi = (c & np.uint64(0xFFFFFFFF)).astype(np.uint64), (c >> np.uint64(32)).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    x = (((lo ^ np.uint64(seed)) * np.uint64(0x9E3779B1)) + hi * np.uint64(0x85EBCA77)) & m32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & m32
    x ^= x >> np.uint64(13)
    return x


def partition_rows(rkey, nr, P):
    """Non-null build rows of each of P radix partitions (part_of(hash32(cell, JN_SEED), P)) and every row's partition."""
    nul, cell = ONP.key_cells(rkey, nr)
    live = nul == 0
    part = ((hash32(cell[live], join_constants()["JN_SEED"]) * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
    return np.bincount(part, minlength=P), part, cell[live]


# ---- features -----------------------------------------------------------------------------------------------------------
_SIZE_LABELS = ("0", "1", "2", "wave-1", "wave", "wave+1", "threads-1", "threads", "threads+1", "tile-1", "tile", "tile+1", "tiles+1")
_ROW_LABELS = ("0", "wave-1", "wave", "threads-1", "threads", "tile-1", "tile", "tile+1", "last")
FEATURES = tuple(
    ["nl_" + s for s in _SIZE_LABELS] + ["nr_" + s for s in _SIZE_LABELS]
    + ["nl_scan_batch", "nl_scan_batch+1", "nl_two_scan_batches+1", "scan_batch_edge_tiles_emit"]
    + ["only_match_at_" + s for s in _ROW_LABELS] + ["only_miss_at_" + s for s in _ROW_LABELS]
    + ["only_match_has_1", "only_match_has_2", "only_match_has_maxrun", "all_left_miss", "all_left_null"]
    + ["run_1", "run_2", "run_mid", "run_maxrun-1", "run_maxrun", "run_maxrun+1", "run_long", "build_empty"]
    + ["part_lds_max-1", "part_lds_max", "part_lds_max+1", "part_below_general", "part_general", "part_overflow_fits_at_4x"]
    + ["bitonic_single_key", "bitonic_pad_min", "bitonic_pad_min+1", "bitonic_pow2", "bitonic_pow2+1", "bitonic_lds_max",
       "bitonic_general", "bitonic_after_retry"]
    + ["sentinel_left_only", "sentinel_right_only", "sentinel_both", "sentinel_run_1", "sentinel_run_short", "sentinel_run_long"]
    + ["nulls_left", "nulls_right", "no_nulls", "all_right_null"]
    + ["dtype_i64", "dtype_f64", "dtype_u32", "dtype_bool", "bool_stray_bits", "f64_signed_zeros", "f64_two_nan_payloads"]
    + ["one_pass", "one_pass_resize", "one_pass_resize_unmatched_right"]
    + ["nr_scan_seg-1", "nr_scan_seg", "nr_scan_seg+1", "nr_two_scan_segs+1"]
    + ["right_none_matched", "right_all_matched", "right_only_first_matched", "right_only_last_matched"])


def _size_label(n, K):
    T, TH = K["TILE"], K["LK_THREADS"]
    table = {0: "0", 1: "1", 2: "2", WAVE - 1: "wave-1", WAVE: "wave", WAVE + 1: "wave+1", TH - 1: "threads-1", TH: "threads",
             TH + 1: "threads+1", T - 1: "tile-1", T: "tile", T + 1: "tile+1"}
    if n in table:
        return table[n]
    if n > T + 1 and n % T == 1 and n < K["SCAN_TILES"] * T:
        return "tiles+1"
    return None


def _row_label(r, nl, K):
    T, TH = K["TILE"], K["LK_THREADS"]
    table = {0: "0", WAVE - 1: "wave-1", WAVE: "wave", TH - 1: "threads-1", TH: "threads", T - 1: "tile-1", T: "tile", T + 1: "tile+1"}
    return table.get(r, "last" if r == nl - 1 else None)


def _run_label(m, K):
    M = K["BH_MAXRUN"]
    return "run_1" if m == 1 else "run_2" if m == 2 else "run_maxrun-1" if m == M - 1 else "run_maxrun" if m == M \
        else "run_maxrun+1" if m == M + 1 else "run_long" if m > M + 1 else "run_mid"


def _stray_bits(buf, n):
    return buf is not None and n % 8 != 0 and len(buf) * 8 > n and (int(np.asarray(buf, np.uint8)[n // 8]) >> (n % 8)) != 0


def join_features(case):
    """The structural edges a case reaches, from its inputs and options alone (no engine, no oracle)."""
    K = join_constants()
    lkey, nl, rkey, nr, opt = case["lkey"], case["nl"], case["rkey"], case["nr"], case["options"]
    T, MAXRUN, LDS_MAX = K["TILE"], K["BH_MAXRUN"], K["BH_MAXROWS"]
    f = set()
    lnul, lcell = ONP.key_cells(lkey, nl)
    rnul, rcell = ONP.key_cells(rkey, nr)
    llive, rlive = lnul == 0, rnul == 0
    for side, n in (("nl_", nl), ("nr_", nr)):
        lab = _size_label(n, K)
        if lab:
            f.add(side + lab)
    batch = K["SCAN_TILES"] * T
    f |= {"nl_scan_batch"} if nl == batch else {"nl_scan_batch+1"} if nl == batch + 1 else {"nl_two_scan_batches+1"} if nl == 2 * batch + 1 else set()
    f.add({O.I64: "dtype_i64", O.F64: "dtype_f64", O.U32CODE: "dtype_u32", O.BOOLBITS: "dtype_bool"}[lkey[2]])
    # nulls
    if nl and not llive.any():
        f.add("all_left_null")
    if nr and not rlive.any():
        f.add("all_right_null")
    if nl and (~llive).any():
        f.add("nulls_left")
    if nr and (~rlive).any():
        f.add("nulls_right")
    if nl and nr and llive.all() and rlive.all():
        f.add("no_nulls")
    # build-side runs
    keys, runs = np.unique(rcell[rlive], return_counts=True)
    if len(keys) == 0:
        f.add("build_empty")
    for m in np.unique(runs):
        f.add(_run_label(int(m), K))
    # which left rows match
    hit = llive & np.isin(lcell, keys)
    miss = llive & ~hit
    if nl > T and llive.any():
        if hit.sum() == 1:
            r = int(np.flatnonzero(hit)[0])
            lab = _row_label(r, nl, K)
            if lab:
                f.add("only_match_at_" + lab)
            m = int(runs[np.searchsorted(keys, lcell[r])])
            f |= {"only_match_has_1"} if m == 1 else {"only_match_has_2"} if m == 2 else {"only_match_has_maxrun"} if m == MAXRUN else set()
        if miss.sum() == 1 and hit.sum() == nl - 1:
            lab = _row_label(int(np.flatnonzero(miss)[0]), nl, K)
            if lab:
                f.add("only_miss_at_" + lab)
        if not hit.any():
            f.add("all_left_miss")
    if nl > batch - T and hit[batch - T:batch].any() and (nl <= batch or hit[batch:batch + T].any()):
        f.add("scan_batch_edge_tiles_emit")
    # the sentinel-valued key (cells of null rows are 0, never the sentinel)
    if lkey[2] == O.I64:
        sent = np.uint64(0xFFFFFFFFFFFFFFFF)
        l_has, r_run = bool((lcell[llive] == sent).any()), int((rcell[rlive] == sent).sum())
        if l_has or r_run:
            f.add("sentinel_both" if l_has and r_run else "sentinel_left_only" if l_has else "sentinel_right_only")
        if r_run:
            f.add("sentinel_run_1" if r_run == 1 else "sentinel_run_short" if r_run <= MAXRUN else "sentinel_run_long")
    if lkey[2] == O.F64:
        bits = np.concatenate([np.asarray(lkey[0], np.float64)[:nl].view(np.uint64), np.asarray(rkey[0], np.float64)[:nr].view(np.uint64)])
        if (bits == 0).any() and (bits == np.uint64(1 << 63)).any():
            f.add("f64_signed_zeros")
        vals = bits.view(np.float64)
        if len(np.unique(bits[np.isnan(vals)])) >= 2:
            f.add("f64_two_nan_payloads")
    if lkey[2] == O.BOOLBITS:
        if all(_stray_bits(b, n) for b, n in ((lkey[0], nl), (lkey[1], nl), (rkey[0], nr), (rkey[1], nr))):
            f.add("bool_stray_bits")
    # unmatched right rows behind the probe output
    seg = K["SCAN_SEG"]
    f |= {"nr_scan_seg-1"} if nr == seg - 1 else {"nr_scan_seg"} if nr == seg else {"nr_scan_seg+1"} if nr == seg + 1 else \
        {"nr_two_scan_segs+1"} if nr == 2 * seg + 1 else set()
    if nr >= seg - 1:
        rmatched = rlive & np.isin(rcell, lcell[llive])
        if not rmatched.any():
            f.add("right_none_matched")
        elif rmatched.all():
            f.add("right_all_matched")
        elif rmatched.sum() == 1 and rmatched[0]:
            f.add("right_only_first_matched")
        elif rmatched.sum() == 1 and rmatched[-1]:
            f.add("right_only_last_matched")
    # the single-pass probe and its one re-size
    if opt.get("join_one_pass") and nl > 0:
        f.add("one_pass")
        inner = int(runs[np.searchsorted(keys, lcell[hit])].sum()) if hit.any() else 0
        if inner > nl + 16:                                   # the first buffer holds nl + 16 rows from the probe
            f.add("one_pass_resize")
            if (rlive & ~np.isin(rcell, lcell[llive])).any():
                f.add("one_pass_resize_unmatched_right")
    # rows per FORCED partition (option `partitions`; below 2 x 8192 build rows the engine keeps the forced fan-out as it is)
    P = int(opt.get("partitions", 0))
    if P > 0 and nr < 2 * K["JN_RCAP"] and not opt.get("join_generic"):
        def long_run_partitions(P_):
            counts, part, cells = partition_rows(rkey, nr, P_)
            longest = np.zeros(P_, np.int64)
            kk, inv, cnt = np.unique(cells, return_inverse=True, return_counts=True)
            np.maximum.at(longest, part, cnt[inv])
            distinct = np.bincount(part[np.unique(inv, return_index=True)[1]], minlength=P_)
            return counts, longest, distinct
        counts, longest, distinct = long_run_partitions(P)
        general = nr / P > K["GENERAL_ROWS"]
        if general:
            f.add("part_general")
            if (longest > MAXRUN).any():
                f.add("bitonic_general")
        else:
            if P == 1 and int(counts[0]) == int(K["GENERAL_ROWS"]):
                f.add("part_below_general")
            for n in counts:
                f |= {"part_lds_max-1"} if n == LDS_MAX - 1 else {"part_lds_max"} if n == LDS_MAX else {"part_lds_max+1"} if n == LDS_MAX + 1 else set()
            if (counts > LDS_MAX).any():
                P4 = min(P * 4, K["P_MAX"])
                c4, l4, d4 = long_run_partitions(P4)
                if (c4 <= LDS_MAX).all():
                    f.add("part_overflow_fits_at_4x")
                    if (l4 > MAXRUN).any():
                        f.add("bitonic_after_retry")
            else:
                for n, m, d in zip(counts, longest, distinct):
                    if m <= MAXRUN:
                        continue
                    if d == 1:
                        f.add("bitonic_single_key")
                    f |= {"bitonic_pad_min"} if n == WAVE else {"bitonic_pad_min+1"} if n == WAVE + 1 else \
                        {"bitonic_pow2"} if n == K["JN_RCAP"] // 2 else {"bitonic_pow2+1"} if n == K["JN_RCAP"] // 2 + 1 else \
                        {"bitonic_lds_max"} if n == LDS_MAX else set()
    return f


# ---- the cases ----------------------------------------------------------------------------------------------------------
MULT = 1_000_003                # spreads small ids over i64 (never -1: ids are >= 0)
HOT, MISS0 = -777 * MULT, 10 ** 12     # the hot key is negative, every miss is beyond the largest id: neither collides with an id


def _mask(rng, n, p):
    return O.pack_mask(rng.random(n) < p) if n and p > 0 else None


def _case(name, group, lk, rk, options=None, features=(), hows=ALL_HOWS, dtype=O.I64, lmask=None, rmask=None, nl=None, nr=None):
    nl = len(lk) if nl is None else nl
    nr = len(rk) if nr is None else nr
    return {"name": name, "group": group, "lkey": (lk, lmask, dtype), "nl": nl, "rkey": (rk, rmask, dtype), "nr": nr,
            "options": dict(options or {}), "features": set(features), "hows": tuple(hows)}


def _ids(a):
    return np.asarray(a, np.int64) * MULT


def row_count_sizes():
    T = join_constants()["TILE"]
    OT = join_constants()["OP_TILE"]           # the single-pass probe's tile: today the same 2048 rows
    extra = [OT - 1, OT, OT + 1] if OT != T else []
    TH = join_constants()["LK_THREADS"]
    return sorted(set([0, 1, 2, WAVE - 1, WAVE, WAVE + 1, TH - 1, TH, TH + 1, T - 1, T, T + 1, 3 * T + 1] + extra))


def _cases_a():
    """Row counts: a diagonal plus (small, large) and (large, small); 2 % nulls on both sides; both probes."""
    S = row_count_sizes()
    pairs = sorted(set([(s, s) for s in S] + [(S[i], S[-1 - i]) for i in range(len(S))]))
    for nl, nr in pairs:
        rng = np.random.default_rng(1000 + 7 * nl + nr)
        space = max(nr, 3)
        lk, rk = _ids(rng.integers(0, space, nl)), _ids(rng.integers(0, space, nr))
        lm, rm = _mask(rng, nl, 0.02), _mask(rng, nr, 0.02)
        K = join_constants()
        for onepass in (0, 1):
            yield _case("a_nl%d_nr%d_%s" % (nl, nr, "onepass" if onepass else "threekernel"), "a", lk, rk,
                        {"join_one_pass": onepass}, lmask=lm, rmask=rm,
                        features={side + _size_label(n, K) for side, n in (("nl_", nl), ("nr_", nr)) if _size_label(n, K)}
                        | ({"one_pass"} if onepass and nl else set()))


def match_rows():
    T, TH = join_constants()["TILE"], join_constants()["LK_THREADS"]
    return [0, WAVE - 1, WAVE, TH - 1, TH, T - 1, T, T + 1, 2 * T]


def _cases_b():
    """Which left rows match, against tile, row-slice and wave edges: nl = 2 tiles + 1, a small build side."""
    K = join_constants()
    nl = 2 * K["TILE"] + 1
    others = _ids(np.arange(1, 21))
    for row in match_rows():
        for m in (1, 2, K["BH_MAXRUN"]):
            rng = np.random.default_rng(2000 + row + m)
            rk = np.concatenate([others, np.full(m, HOT, np.int64)])[rng.permutation(20 + m)]
            lk = MISS0 + np.arange(nl, dtype=np.int64)
            lk[row] = HOT
            yield _case("b_only_row%d_matches_%d" % (row, m), "b", lk, rk,
                        features={"only_match_at_" + _row_label(row, nl, K), "only_match_has_" + ("maxrun" if m > 2 else str(m)), _run_label(m, K)})
    rk = _ids(np.arange(1, 51))
    for row in match_rows():
        lk = rk[np.arange(nl) % 50].copy()
        lk[row] = MISS0
        yield _case("b_only_row%d_misses" % row, "b", lk, rk, features={"only_miss_at_" + _row_label(row, nl, K)})
    yield _case("b_all_miss", "b", MISS0 + np.arange(nl, dtype=np.int64), rk, features={"all_left_miss"})
    yield _case("b_all_left_null", "b", rk[np.arange(nl) % 50].copy(), rk, lmask=O.pack_mask(np.ones(nl, bool)), features={"all_left_null"})


def run_lengths():
    M = join_constants()["BH_MAXRUN"]
    return [1, 2, 3, M - 1, M, M + 1, 64, 65, 1000]


def _long_run_sides(rng, m, n_other, long_key, left_key, nl=300, left_extra=()):
    """Build side: `m` rows of long_key scattered among n_other unique keys; probe side: picks of the build keys, 10 % misses and
    left_key (the long key, unless it sits on one side only) at several rows."""
    nr = m + n_other
    rk = _ids(np.arange(1, nr + 1))
    rk[rng.choice(nr, m, replace=False)] = long_key
    lk = rk[rng.integers(0, nr, nl)].copy()
    lk[lk == long_key] = rk[rk != long_key][0] if n_other else MISS0 + 5
    lk[rng.random(nl) < 0.1] = MISS0 + 1
    for r in (0, nl // 3, nl - 1):
        lk[r] = left_key
    for r, v in left_extra:
        lk[r] = v
    return lk, rk


def _cases_c():
    """Run lengths on the build side, one partition: the hot key plain, as the sentinel-valued key, and the sentinel on one side."""
    K = join_constants()
    for m in run_lengths():
        rng = np.random.default_rng(3000 + m)
        run = _run_label(m, K)
        srun = "sentinel_run_1" if m == 1 else "sentinel_run_short" if m <= K["BH_MAXRUN"] else "sentinel_run_long"
        yield _case("c_run%d_plain" % m, "c", *_long_run_sides(rng, m, 500, HOT, HOT), {"partitions": 1}, features={run})
        yield _case("c_run%d_sentinel_both" % m, "c", *_long_run_sides(rng, m, 500, SENTINEL, SENTINEL), {"partitions": 1},
                    features={run, srun, "sentinel_both"})
        yield _case("c_run%d_sentinel_left_only" % m, "c", *_long_run_sides(rng, m, 500, HOT, HOT, left_extra=((7, SENTINEL), (150, SENTINEL))),
                    {"partitions": 1}, features={run, "sentinel_left_only"})
        yield _case("c_run%d_sentinel_right_only" % m, "c", *_long_run_sides(rng, m, 500, SENTINEL, HOT), {"partitions": 1},
                    features={run, srun, "sentinel_right_only"})


def _unique_sides(rng, nr):
    """Unique build keys, no nulls; the probe side holds every build key once plus 10 % misses, shuffled."""
    rk = _ids(rng.permutation(nr * 3)[:nr] + 1)
    lk = np.concatenate([rk, MISS0 + np.arange(nr // 10 + 1, dtype=np.int64)])
    return lk[rng.permutation(len(lk))], rk


def _cases_d():
    """Rows per partition (one forced partition): the region at its highest load, one row more (retry), both sides of the
    general path's threshold, and the bitonic fallback at its padded sizes."""
    K = join_constants()
    LDS_MAX, G, M = K["BH_MAXROWS"], int(K["GENERAL_ROWS"]), K["BH_MAXRUN"]
    for nr, hows, feat in ((LDS_MAX - 1, ALL_HOWS, {"part_lds_max-1"}), (LDS_MAX, ALL_HOWS, {"part_lds_max"}),
                           (LDS_MAX + 1, ALL_HOWS, {"part_lds_max+1", "part_overflow_fits_at_4x"}),
                           (G, ALL_HOWS, {"part_below_general", "part_overflow_fits_at_4x"}), (G + 1, INNER_OUTER, {"part_general"})):
        yield _case("d_unique_nr%d" % nr, "d", *_unique_sides(np.random.default_rng(4000 + nr), nr), {"partitions": 1}, hows=hows,
                    features=feat | {"no_nulls", "run_1"})
    for n, feat in ((LDS_MAX, "bitonic_lds_max"), (M + 1, "bitonic_single_key"), (WAVE, "bitonic_pad_min"), (WAVE + 1, "bitonic_pad_min+1"),
                    (K["JN_RCAP"] // 2, "bitonic_pow2"), (K["JN_RCAP"] // 2 + 1, "bitonic_pow2+1")):
        yield _case("d_run%d_in_%d_rows" % (M + 1, n), "d", *_long_run_sides(np.random.default_rng(4100 + n), M + 1, n - M - 1, HOT, HOT),
                    {"partitions": 1}, features={feat, "run_maxrun+1"})
    yield _case("d_run%d_general" % (M + 1), "d", *_long_run_sides(np.random.default_rng(4200), M + 1, G - M, HOT, HOT), {"partitions": 1},
                hows=INNER_OUTER, features={"bitonic_general", "part_general", "run_maxrun+1"})


def overflow_retry_sides():
    """e.: two forced partitions, ~13 000 build rows with one key on 3 000 of them; -> (lk, rk)."""
    rng = np.random.default_rng(5000)
    return _long_run_sides(rng, 3000, 10_000, HOT, HOT, nl=3000)


def _cases_e():
    yield _case("e_overflow_then_retry", "e", *overflow_retry_sides(), {"partitions": 2},
                features={"part_overflow_fits_at_4x", "bitonic_after_retry", "run_long"})


def scan_batch_sizes():
    K = join_constants()
    batch = K["SCAN_TILES"] * K["TILE"]
    return [batch, batch + 1, 2 * batch + 1]


def _cases_f():
    """Scan batches of tile_scan_kernel: left keys hit with probability 1/2; the last tile of the first batch and the first tile
    of the second both emit."""
    K = join_constants()
    batch = K["SCAN_TILES"] * K["TILE"]
    for nl in scan_batch_sizes():
        rng = np.random.default_rng(6000 + nl % 97)
        rk = _ids(rng.permutation(3000)[:1000] + 1)
        lk = np.where(rng.random(nl) < 0.5, rk[rng.integers(0, 1000, nl)], MISS0 + 3)
        lk[batch - 1] = rk[0]
        if nl > batch:
            lk[batch] = rk[1]
        yield _case("f_nl%d" % nl, "f", lk, rk, hows=INNER_OUTER,
                    features={"scan_batch_edge_tiles_emit", "nl_scan_batch" if nl == batch else "nl_scan_batch+1" if nl == batch + 1 else "nl_two_scan_batches+1"})


def _cases_g():
    """Single-pass probe, every build key three times: the output outgrows the buffer sized for unique keys; the probe side
    never holds the last fifth of the build keys, so right/outer keep unmatched rows across the re-size."""
    rng = np.random.default_rng(7000)
    rk = _ids(np.repeat(np.arange(1, 1001), 3))[rng.permutation(3000)]
    lk = _ids(rng.integers(1, 801, 2000))
    lk[rng.random(2000) < 0.1] = MISS0
    yield _case("g_onepass_resize", "g", lk, rk, {"join_one_pass": 1}, lmask=_mask(rng, 2000, 0.02), rmask=_mask(rng, 3000, 0.02),
                features={"one_pass", "one_pass_resize", "one_pass_resize_unmatched_right"})


def scan_seg_sizes():
    seg = join_constants()["SCAN_SEG"]
    return [seg - 1, seg, seg + 1, 2 * seg + 1]


def _cases_h():
    """Unmatched right rows around the segment length of exclusive_scan_u32; right + outer."""
    seg = join_constants()["SCAN_SEG"]
    for nr in scan_seg_sizes():
        size = "nr_scan_seg-1" if nr == seg - 1 else "nr_scan_seg" if nr == seg else "nr_scan_seg+1" if nr == seg + 1 else "nr_two_scan_segs+1"
        rng = np.random.default_rng(8000 + nr)
        rk = _ids(rng.permutation(nr * 2)[:nr] + 1)
        miss = MISS0 + np.arange(100, dtype=np.int64)
        for layout, lk, rmask in (("none_matched", miss, None), ("all_matched", rk[rng.permutation(nr)], None),
                                  ("only_first_matched", np.concatenate([miss, rk[:1]]), None),
                                  ("only_last_matched", np.concatenate([rk[-1:], miss]), None),
                                  ("all_right_null", rk[:100].copy(), O.pack_mask(np.ones(nr, bool)))):
            yield _case("h_nr%d_%s" % (nr, layout), "h", lk, rk, rmask=rmask, hows=(O.RIGHT, O.OUTER),
                        features={size, layout if layout == "all_right_null" else "right_" + layout})


def _stray(bits_or_mask, n):
    """Sets every bit past row n - 1 of the last byte (n is no multiple of 8)."""
    b = np.asarray(bits_or_mask, np.uint8).copy()
    b[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    return b


def _cases_i():
    """Key types: f64 specials, u32 codes, bit-packed bools with stray bits past the last row in data and mask."""
    rng = np.random.default_rng(9000)
    nan2 = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    pool = np.array([0.0, -0.0, np.nan, nan2, np.inf, -np.inf, 1.5])
    nl, nr = 300, 40
    yield _case("i_f64", "i", pool[rng.integers(0, 7, nl)], pool[rng.integers(0, 7, nr)], dtype=O.F64,
                lmask=_mask(rng, nl, 0.05), rmask=_mask(rng, nr, 0.05), features={"dtype_f64", "f64_signed_zeros", "f64_two_nan_payloads"})
    nl, nr = 1000, 200
    yield _case("i_u32", "i", rng.integers(0, 150, nl).astype(np.uint32), rng.integers(0, 150, nr).astype(np.uint32), dtype=O.U32CODE,
                lmask=_mask(rng, nl, 0.05), rmask=_mask(rng, nr, 0.05), features={"dtype_u32"})
    nl, nr = 77, 13
    bits = lambda n: _stray(np.packbits(rng.random(n) < 0.5, bitorder="little"), n)
    nulls = lambda n: _stray(O.pack_mask(rng.random(n) < 0.2), n)
    yield _case("i_bool", "i", bits(nl), bits(nr), dtype=O.BOOLBITS, lmask=nulls(nl), rmask=nulls(nr), nl=nl, nr=nr,
                features={"dtype_bool", "bool_stray_bits"})


_GROUPS = {"a": _cases_a, "b": _cases_b, "c": _cases_c, "d": _cases_d, "e": _cases_e, "f": _cases_f, "g": _cases_g, "h": _cases_h,
           "i": _cases_i}


def edge_cases(groups=None):
    """The named cases, group by group (a. row counts ... i. key types; the letters are the sections of
    tests/test_gpu_join_edges.py).  Deterministic; `groups` limits the generator to some letters."""
    for g in (sorted(_GROUPS) if groups is None else groups):
        yield from _GROUPS[g]()
