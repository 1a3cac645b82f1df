"""A slice of the randomised parity sweep inside the GPU test suite (the builder-run fuzz —
profiles/r0N_fuzz_summary.txt, thousands of cases — was not part of GPUTEST).  experiments/fuzz_parity.py draws shapes, dtypes,
null rates, skews, row layouts, aggregate sets, join types and engine knobs at random and compares the HIP engine (through the C
ABI) with the CPU oracle, bit for bit where the reference is; experiments/fuzz_absorb.py forces the hot-key absorb pass.  Fixed
seeds: the same cases every run."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, *args, env=None):
    e = dict(os.environ, **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", script), *map(str, args)], capture_output=True, text=True,
                       timeout=280, env=e, cwd=ROOT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0, tail
    return r.stdout


def test_fuzz_slice_default_mix():
    out = _run("fuzz_parity.py", 70, 4001)
    assert "fuzz done: 70 cases, 0 failures" in out


def test_fuzz_slice_joins_and_fused():
    out = _run("fuzz_parity.py", 40, 4002, env={"FUZZ_GROUPBY_FRAC": "0.0"})
    assert "fuzz done: 40 cases, 0 failures" in out


def test_fuzz_slice_absorb_forced():
    out = _run("fuzz_absorb.py", 25, 43)
    assert "0 failures" in out


def test_fuzz_slice_distributed_real_ranks():
    """experiments/fuzz_dist.py: the in-library exchange (dist.hip) with three REAL ranks on the one GPU over a host transport —
    random uneven / empty row ranges, null masks passed by random subsets of the ranks (the layout agreement that rides on the
    count exchange), host and device shards, mergeable and shuffled aggregate sets, one or two key columns; the owners' results,
    concatenated, equal the oracle on the whole frame."""
    out = _run("fuzz_dist.py", 3, 14, 5)
    assert "fuzz_dist done: world 3, 14 cases, 0 failing rank-cases" in out


# experiments/fuzz_ops.py: sort, filter, window, their chains, the eight column-op kinds and chain2.  kind -> (cases, seed); tests/test_references.py runs the same
# slices dry (no engine call) on a CPU-only box and asserts that every coverage line is above zero.
FUZZ_OPS_SLICES = {"sort": (1120, 6001), "filter": (1200, 6002), "window": (920, 6003), "chain": (160, 6004),
                   # The column ops' kinds and the cross-op chains (experiments/fuzz_columns.py, fuzz_chain2.py).  Measured on one MI355X
                   # with FUZZ_KIND=<kind>, start-up (1.7 s) taken off: describe 0.86 ms a case, rank 2.1, fill 0.85, topk 0.96, predicate
                   # 0.77, wquant 0.9, cum 0.65, eval 1.1, chain2 37.  Sized to about ten seconds of wall time; topk and eval stop where the
                   # same slice, run dry by tests/test_references.py on a CPU (their twins run in the draw), costs ten seconds there.
                   "describe": (9500, 6005), "rank": (3900, 6006), "fill": (9500, 6007), "topk": (4500, 6008), "predicate": (10000, 6009),
                   "wquant": (9000, 6010), "cum": (12000, 6011), "eval": (5000, 6012), "chain2": (225, 6013)}


def _run_ops(kind):
    count, seed = FUZZ_OPS_SLICES[kind]
    out = _run("fuzz_ops.py", count, seed, env={"FUZZ_KIND": kind, "FUZZ_DRY": "0", "FUZZ_FIRST": "0"})
    assert "fuzz_ops done: %d cases, 0 failures" % count in out
    assert "features not reached" not in out and "coverage (cases run):" in out


def test_fuzz_ops_slice_sort():
    """Layout-directed keys: every digit width from 1 to 8, one to four and more key words, codes of 65 bits and codes that
    straddle a word, constant digits, all-null / all-NaN / constant keys, sort_digit_bits 0 and 4 ... 8; the permutation
    equals ref_lexsort's (and ref_cmp's up to 20 000 rows) and the pass count equals the one derived from the header's rule."""
    _run_ops("sort")


def test_fuzz_ops_slice_filter():
    _run_ops("filter")


def test_fuzz_ops_slice_window():
    _run_ops("window")


def test_fuzz_ops_slice_chains():
    """filter -> gather -> sort -> gather -> window, filter -> gather -> groupby, sort -> gather -> groupby of the now clustered
    rows, sort -> gather -> window: every intermediate stays on the device, every stage is compared."""
    _run_ops("chain")


# The eight column-op kinds share their draws of the input space (host, device, device 8 bytes off with the mask 3 bytes off,
# resident), the output placement (host, device, a caller's device buffer at 8 mod 16 / byte offset 1 between guard cells that
# must stay intact), the dtype, the null layout (no mask, a mask without a bit, 1 %, 50 %, all null), special cells (NaN, +-inf,
# -0.0, a subnormal; i64 beyond 2^53 and both extremes) and the row count (0, 1, 2, 63, 64, 65, one and two tiles -1 / 0 / +1, one
# row more than a full persistent grid covers).  Each compares by the rule of its directed test, imported from tests/*_ref.py.
def test_fuzz_ops_slice_describe():
    """describe and quantiles with 1 ... 16 percentiles (0, 100, duplicates, unsorted lists) over constant columns, columns whose
    lowest or top byte alone varies, full-range patterns and two values in long runs, non-null counts 0 / 1 / 2; order statistics
    as equal values, the moments within describe_ref's bound where the directed test compares them; 17 percentiles refused."""
    _run_ops("describe")


def test_fuzz_ops_slice_rank():
    """The five methods over tie runs that end on, before and after a tile edge of the sorted positions, one run over the whole
    column, all-distinct cells and rank_ref.sweep_cases, sort_digit_bits 0 and 4 ... 8, every special path rank_features names;
    bit for bit against rank_ref; a method outside the enum refused."""
    _run_ops("rank")


def test_fuzz_ops_slice_fill():
    """ffill, bfill, linear and value over gaps of 1, 63 / 64 / 65, a tile -1 / 0 / +1 and longer, leading, trailing and whole-column
    gaps, as NaN cells and as null bits, fill_ref.sweep_cases, values NaN / -0.0 / an i64 beyond 2^53; cells, mask and count bit for
    bit against fill_twin; an output over the column refused."""
    _run_ops("fill")


def test_fuzz_ops_slice_topk():
    """nlargest, nsmallest and arg_extreme at k = 0, 1, n - 1, n, n + 1 and the cut-over -1 / 0 / +1, topk_path -1 / 0 / 1, ties that
    straddle the threshold, codes that vary in 1, 3 and 8 bytes; rows and the number count equal topk_ref's, and the side of the
    cut-over the default took is read from the pass count; k < 0 refused."""
    _run_ops("topk")


def test_fuzz_ops_slice_predicate():
    """Every predicate op with constants equal to a cell, between two cells, NaN and +-inf, predicate_path 0 / 1 on i64 beyond 2^53,
    count_only; isin with lists of 0, 1, 3, isin_lds_max_values -1 / 0 / +1 and 100 000 values, isin_path 0 / 1 / 2, negate,
    duplicates, the list on the host and on the device, hit rates near 0 and 1, all four dtype pairings: the bitmap bytewise (tail
    bits zero) and the count against predicate_ref, and which set isin built; a string column refused by predicate."""
    _run_ops("predicate")


def test_fuzz_ops_slice_wquant():
    """Rolling and expanding median and quantile (q = 0, 1/3, 0.5, 1) at w = 1, 2, 3, WQ_DIRECT_MAX -1 / 0 / +1, 300, n and n + 1, with
    center, min_periods unset / 0 / 1 / w / w + 1, nan_missing, window_quantile_path 0 / 1 / 2 and long tie runs, bit for bit against
    window_quantile_fast; the direct path forced beyond its window refused."""
    _run_ops("wquant")


def test_fuzz_ops_slice_cum():
    """The five cumulative ops and the three lags, periods 0, +-1, +-63 / 64 / 65, +-(tile +- 1), +-(n - 1), +-n, +-(n + 1), products
    of factors near one and the range-excursion inputs of test_gpu_cumulative.py: MAX / MIN / COUNT, exact sums and every lag bit for
    bit, SUM and PROD inside cumulative_ref.compare_cells' bounds; the mask, its count and the caller's mask buffer bytewise; a diff
    with negative periods refused."""
    _run_ops("cum")


def test_fuzz_ops_slice_eval():
    """Programs from eval_ref.random_program with want_mask both ways, of one op, of MAX_OPS ops and of depth MAX_DEPTH, over 1 ... 8
    columns of mixed dtypes (some masked, one passed twice): value outputs with and without out_mask, mask outputs handed to a
    count-only filter_indices as they lie on the device, bit for bit against eval_ref.evaluate; an output over a named column refused."""
    _run_ops("eval")


def test_fuzz_ops_slice_chain2():
    """Seven chains across the column ops and the older ones, every intermediate on the device and compared with the references'
    own chain stage by stage: eval mask -> filter -> gather -> bitmap -> cumulative; predicate -> filter -> gather -> rank; fill ->
    cumulative -> lag -> rolling mean through caller-owned masks at byte offset 1; topk -> gather -> describe / quantiles; sort ->
    gather -> rolling median -> predicate count; eval -> rank -> isin -> filter count; join -> join_gather -> eval -> groupby."""
    _run_ops("chain2")


# ---- the same sweeps with the library's workspace poisoned --------------------------------------------------------------------
# set_option("poison_workspace") through FUZZ_POISON: every arena and one-off table starts every call as the byte instead of
# as what the previous case left there (tests/test_gpu_workspace.py holds the directed cases, path by path; these slices add
# the generators' variety).  Case counts: the per-case time of the slice above, measured on an MI355X, sized to about ten
# seconds each.  The fuzz_ops slices replay the tail of the slices above (FUZZ_FIRST), so their coverage lines are not the
# condition here.
POISON_ENV = {"FUZZ_POISON": "0xA5"}
FUZZ_OPS_POISONED_FIRST = {"sort": 1120 - 100, "filter": 0, "window": 920 - 590, "chain": 160 - 72,
                           # about five seconds each, from the per-case times above: the tail of the slice
                           "describe": 9500 - 3800, "rank": 3900 - 1570, "fill": 9500 - 3900, "topk": 4500 - 3400, "predicate": 10000 - 4300,
                           "wquant": 9000 - 3650, "cum": 12000 - 5000, "eval": 5000 - 3000, "chain2": 225 - 89}


def test_fuzz_slice_default_mix_poisoned():
    out = _run("fuzz_parity.py", 90, 4001, env=POISON_ENV)
    assert "fuzz done: 90 cases, 0 failures" in out


def test_fuzz_slice_joins_and_fused_poisoned():
    out = _run("fuzz_parity.py", 100, 4002, env=dict(POISON_ENV, FUZZ_GROUPBY_FRAC="0.0", FUZZ_POISON="0xFF"))
    assert "fuzz done: 100 cases, 0 failures" in out


def test_fuzz_slice_absorb_forced_poisoned():
    out = _run("fuzz_absorb.py", 33, 43, env=POISON_ENV)
    assert "fuzz_absorb done: 33 cases" in out and ", 0 failures" in out


def test_fuzz_slice_distributed_real_ranks_poisoned():
    out = _run("fuzz_dist.py", 3, 27, 5, env=POISON_ENV)
    assert "fuzz_dist done: world 3, 27 cases, 0 failing rank-cases" in out


@pytest.mark.parametrize("kind", list(FUZZ_OPS_SLICES))
def test_fuzz_ops_slice_poisoned(kind):
    count, seed = FUZZ_OPS_SLICES[kind]
    first = FUZZ_OPS_POISONED_FIRST[kind]
    out = _run("fuzz_ops.py", count, seed, env=dict(POISON_ENV, FUZZ_KIND=kind, FUZZ_DRY="0", FUZZ_FIRST=str(first)))
    assert "fuzz_ops done: %d cases, 0 failures" % (count - first) in out
