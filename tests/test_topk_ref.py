"""tests/topk_ref.py against itself, against tests/sort_ref.py and against the reference's known answers
(src/dataframe/pandas_compat/functions.rs:4369-4391).  No GPU."""
import numpy as np
import pytest

from pandrs_amd import _lib as L
from tests.sort_ref import Col, ref_lexsort
from tests.topk_ref import idx_extreme_ref, topk_ref, topk_ref_lines


def _columns():
    rng = np.random.default_rng(7)
    yield rng.normal(0, 1, 257)
    yield rng.integers(0, 4, 300).astype(np.float64)                     # heavy ties
    yield rng.integers(-3, 3, 300)                                        # ... as integers
    yield np.zeros(40)                                                    # one value
    yield np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0] * 9)
    yield np.array([2**53 + 1, 2**53, 2**53 + 1, 2**53, -2**63, 2**63 - 1], np.int64)
    yield np.array([np.inf, -np.inf, 5e-324, -5e-324, 0.0, 1.0, np.inf])
    yield np.array([3.5])
    yield np.array([], np.float64)


@pytest.mark.parametrize("largest", [True, False])
def test_line_for_line_equals_vectorised_without_missing_cells(largest):
    for x in _columns():
        n = x.shape[0]
        for k in {0, 1, 2, n // 2, max(n - 1, 0), n, n + 5}:
            rows, numbers = topk_ref(x, None, k, largest)
            assert np.array_equal(rows, topk_ref_lines(x, k, largest)), (x[:6], k)
            assert numbers == min(k, n) == rows.shape[0]


@pytest.mark.parametrize("largest", [True, False])
def test_vectorised_is_the_head_of_the_sort_reference(largest):
    rng = np.random.default_rng(11)
    for trial in range(12):
        n = int(rng.integers(1, 400))
        if trial % 2:
            x = rng.integers(-5, 5, n)
            dtype = L.I64
        else:
            x = rng.integers(-5, 5, n).astype(np.float64) / 2
            x[rng.random(n) < 0.2] = np.nan
            x[rng.random(n) < 0.1] = -0.0
            dtype = L.F64
        nulls = rng.random(n) < (0.0, 0.15, 1.0)[trial % 3]
        order = ref_lexsort([Col(dtype, x, nulls)], [not largest])
        m = int((~nulls & ~(np.isnan(x) if dtype == L.F64 else np.zeros(n, bool))).sum())
        for k in (0, 1, m - 1, m, m + 1, n - 1, n, n + 3):
            if k < 0:
                continue
            rows, numbers = topk_ref(x, nulls, k, largest)
            assert np.array_equal(rows, order[:k]) and numbers == min(k, m, n)


def test_known_answers_of_the_reference():
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0])                              # create_test_df, functions.rs:4327-4355
    rows, numbers = topk_ref(a, None, 3, True)                            # test_nlargest: row_count 3
    assert list(rows) == [4, 3, 2] and numbers == 3
    rows, numbers = topk_ref(a, None, 2, False)                           # test_nsmallest: row_count 2
    assert list(rows) == [0, 1] and numbers == 2
    assert idx_extreme_ref(a) == (0, 4)                                   # test_idxmin: Some(0), test_idxmax: Some(4)
    assert idx_extreme_ref(np.array([], np.float64)) is None
    assert idx_extreme_ref(np.array([2.0, 7.0, 2.0, 7.0])) == (0, 3)      # first minimum, last maximum
    assert idx_extreme_ref(np.array([np.nan, 0.0, -0.0, np.nan])) == (1, 2)
    assert idx_extreme_ref(np.array([1, 9, 9], np.int64), [False, False, True]) == (0, 1)
    assert idx_extreme_ref(np.array([np.nan, 1.0]), [False, True]) is None
