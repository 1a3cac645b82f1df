"""tests/rank_ref.py against itself and against the reference's own answers (src/dataframe/pandas_compat/functions.rs:193-236,
known answer :4393-4404): the vectorised restatement the GPU tests compare with equals the line-for-line one bit for bit."""
import numpy as np
import pytest

from tests.rank_ref import AVERAGE, DENSE, FIRST, FEATURES, MAX, METHODS, MIN, rank_features, rank_naive, rank_ref, sweep_cases


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cases():
    rng = np.random.default_rng(1)
    n = 300
    yield "heavy ties f64", rng.integers(0, 7, n).astype(np.float64), None
    yield "heavy ties i64", rng.integers(-3, 4, n), None
    yield "all equal", np.full(n, 2.5), None
    yield "all distinct", rng.permutation(n).astype(np.float64), None
    yield "all distinct i64", rng.permutation(n).astype(np.int64) - 150, None
    x = rng.integers(0, 5, n).astype(np.float64)
    x[rng.random(n) < 0.2] = np.nan
    yield "NaN", x, None
    yield "nulls", rng.integers(0, 5, n).astype(np.float64), rng.random(n) < 0.3
    yield "NaN and nulls", x, rng.random(n) < 0.3
    yield "i64 nulls", rng.integers(0, 9, n), rng.random(n) < 0.5
    yield "only NaN", np.full(17, np.nan), None
    yield "only nulls", np.arange(17), np.ones(17, bool)
    yield "signed zeros", np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0] * 30), None
    yield "beyond 2^53", 2**53 + rng.integers(0, 4, n), None
    yield "extremes", np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, np.iinfo(np.int64).min], np.int64), np.array([0, 0, 1, 0], bool)
    yield "infinities", np.array([np.inf, -np.inf, 5e-324, -5e-324, 0.0, np.inf, np.nan]), None
    yield "one row", np.array([4.0]), None
    yield "no row", np.empty(0), None


@pytest.mark.parametrize("name,values,nulls", list(_cases()), ids=[c[0] for c in _cases()])
def test_vectorised_equals_line_for_line(name, values, nulls):
    for method in METHODS:
        assert same_bits(rank_ref(values, nulls, method), rank_naive(values, nulls, method)), (name, method)


def test_the_references_known_answer():
    ranks = rank_naive(np.array([3.0, 1.0, 4.0, 1.0, 5.0]), None, AVERAGE)       # functions.rs:4393-4404
    assert ranks[1] == 1.5 and ranks[3] == 1.5 and ranks[0] == 3.0
    assert same_bits(rank_ref(np.array([3.0, 1.0, 4.0, 1.0, 5.0]), None, AVERAGE), ranks)


TABLE = {   # [3, 1, 4, 1, 5, 4, 4]: sorted 1 1 3 4 4 4 5 -> runs [0, 2) [2, 3) [3, 6) [6, 7)
    AVERAGE: [3.0, 1.5, 5.0, 1.5, 7.0, 5.0, 5.0],
    MIN: [3.0, 1.0, 4.0, 1.0, 7.0, 4.0, 4.0],
    MAX: [3.0, 2.0, 6.0, 2.0, 7.0, 6.0, 6.0],
    FIRST: [3.0, 1.0, 4.0, 2.0, 7.0, 5.0, 6.0],
    DENSE: [2.0, 1.0, 3.0, 1.0, 4.0, 3.0, 3.0],
}


@pytest.mark.parametrize("dtype", [np.float64, np.int64])
def test_hand_written_table(dtype):
    x = np.array([3, 1, 4, 1, 5, 4, 4], dtype)
    for method, want in TABLE.items():
        assert same_bits(rank_naive(x, None, method), want), method
        assert same_bits(rank_ref(x, None, method), want), method


def test_nan_and_null_cells_take_no_rank():
    x = np.array([2.0, np.nan, 1.0, 7.0, 1.0])
    nulls = np.array([False, False, False, True, False])
    got = rank_ref(x, nulls, MIN)
    assert np.isnan(got[1]) and np.isnan(got[3]) and list(got[[0, 2, 4]]) == [3.0, 1.0, 1.0]
    assert rank_ref(x, nulls, MAX)[0] == 3.0                  # the end of the last run is m, not n


def test_features_bookkeeping():
    t = 8
    assert rank_features(np.zeros(20), None, t) == {"multi-tile run", "zero-pass sort"}
    assert rank_features(np.arange(20.0), None, t) == set()
    assert rank_features(np.array([1.0, 1.0, 2.0]), None, t) == set()
    assert rank_features(np.full(5, np.nan), None, t) == {"zero-pass sort", "NaN block"}
    assert rank_features(np.arange(5), np.ones(5, bool), t) == {"zero-pass sort", "null block"}
    lim = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0], np.int64)
    assert rank_features(lim, None, t) == set()
    assert rank_features(lim, np.array([False, False, True]), t) == {"two-word code", "null block"}
    assert rank_features(np.array([1.0, np.nan, 1.0]), np.array([True, False, False]), t) == {"NaN block", "null block"}


def test_the_sweeps_seed_reaches_every_special_path():
    """The GPU sweep (tests/test_gpu_rank.py) fails when a path is not reached; its seed is checked here, without a device,
    at the tile size the header documents."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tile = int(re.search(r"rank_tile_rows = (\d+)", open(os.path.join(root, "include", "pandrs_hip.h")).read()).group(1))
    reached, count, methods, digits, dtypes = {}, 0, set(), set(), set()
    for values, nulls, method, digit_bits in sweep_cases():
        assert 1 <= values.shape[0] < 20_000
        for f in rank_features(values, nulls, tile):
            reached[f] = reached.get(f, 0) + 1
        count += 1
        methods.add(method)
        digits.add(digit_bits)
        dtypes.add(values.dtype.kind)
    assert count == 300 and methods == set(METHODS) and digits == {0, 4, 5, 6, 7, 8} and dtypes == {"i", "f"}
    assert all(reached.get(f, 0) >= 3 for f in FEATURES), reached
