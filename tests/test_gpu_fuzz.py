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


# experiments/fuzz_ops.py: sort, filter, window and their chains.  kind -> (cases, seed); tests/test_references.py runs the same
# slices dry (no engine call) on a CPU-only box and asserts that every coverage line is above zero.
FUZZ_OPS_SLICES = {"sort": (1120, 6001), "filter": (1200, 6002), "window": (920, 6003), "chain": (160, 6004)}


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


# ---- the same sweeps with the library's workspace poisoned --------------------------------------------------------------------
# set_option("poison_workspace") through FUZZ_POISON: every arena and one-off table starts every call as the byte instead of
# as what the previous case left there (tests/test_gpu_workspace.py holds the directed cases, path by path; these slices add
# the generators' variety).  Case counts: the per-case time of the slice above, measured on an MI355X, sized to about ten
# seconds each.  The fuzz_ops slices replay the tail of the slices above (FUZZ_FIRST), so their coverage lines are not the
# condition here.
POISON_ENV = {"FUZZ_POISON": "0xA5"}
FUZZ_OPS_POISONED_FIRST = {"sort": 1120 - 100, "filter": 0, "window": 920 - 590, "chain": 160 - 72}


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
