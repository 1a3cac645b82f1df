"""tests/bin_ref.py against itself: the fast twin (searchsorted, the clamp of cut's last edge, the non-finite case answered
from the NaN count) equals the reference's loops restated line by line (functions.rs:2270-2282, :2339-2420), edge for edge
bit by bit and string for string, on the families the device tests draw from; and the reference's own test vectors
(functions.rs:6840-6846, :6943-7018).  No GPU."""
import math
import struct

import numpy as np
import pytest

from tests import bin_ref as R

CASES = 2000


def bits(xs):
    return [struct.pack("<d", float(x)) for x in xs]


def family(name, rng, n):
    if name == "normal":
        return rng.normal(0.0, 10.0, n)
    if name == "small_ints":
        return rng.integers(-3, 4, n).astype(np.float64)
    if name == "constant":
        return np.full(n, float(rng.choice([0.0, 1.5, -7.0, 1e15, 2.0 ** 52])))
    if name == "1e15":
        return 1e15 + rng.integers(0, 1000, n).astype(np.float64) * rng.choice([0.125, 1.0, 37.0])
    if name == "2^52":
        return 2.0 ** 52 + rng.integers(0, 64, n).astype(np.float64)
    if name == "1e-3":
        return rng.uniform(-1.0, 1.0, n) * 1e-3
    assert name == "nan10"
    v = rng.normal(5.0, 2.0, n)
    v[rng.random(n) < 0.1] = np.nan
    return v


FAMILIES = ["normal", "small_ints", "constant", "1e15", "2^52", "1e-3", "nan10"]


@pytest.mark.parametrize("name", FAMILIES)
def test_cut_twin_equals_the_loops(name):
    rng = np.random.default_rng(FAMILIES.index(name))
    dropped = 0
    for _ in range(CASES):
        n, bins = int(rng.integers(1, 25)), int(rng.integers(1, 10))
        v = family(name, rng, n)
        if np.isnan(v).all():
            with pytest.raises(R.InvalidValue):
                R.cut_loop(v, bins)
            with pytest.raises(R.InvalidValue):
                R.cut(v, bins)
            continue
        e_loop, e_fast = R.cut_edges_loop(v, bins), R.cut_edges(v, bins)
        assert bits(e_loop) == bits(e_fast), (v, bins)
        assert all(a <= b for a, b in zip(e_loop[:-2], e_loop[1:-1])), "interior edges never decrease"
        want = R.cut_loop(v, bins)
        assert R.cut(v, bins) == want, (v, bins)
        # the codes themselves: the binary search with the clamp against the first-match loop on the unclamped list
        c, counts = R.codes(v, R.search_edges(e_fast, False))
        assert c.tolist() == R.codes_loop(v, e_loop), (v, bins)
        assert counts.sum() == n and counts[bins] == n - len(want)
        dropped += n - len(want)
    if name in ("1e15", "2^52"):
        assert dropped > 0, "the maximum falls out of the last bin here: the family must show it"


@pytest.mark.parametrize("name", FAMILIES)
def test_qcut_twin_equals_the_loops(name):
    rng = np.random.default_rng(100 + FAMILIES.index(name))
    for _ in range(CASES):
        n, q = int(rng.integers(1, 25)), int(rng.integers(1, 10))
        v = family(name, rng, n)
        if np.isnan(v).all():
            with pytest.raises(R.InvalidValue):
                R.qcut_loop(v, q)
            with pytest.raises(R.InvalidValue):
                R.qcut(v, q)
            continue
        e_loop, e_fast = R.qcut_edges_loop(v, q), R.qcut_edges(v, q)
        assert bits(e_loop) == bits(e_fast), (v, q)
        assert R.qcut(v, q) == R.qcut_loop(v, q), (v, q)
        c, counts = R.codes(v, R.search_edges(e_fast, True))
        assert c.tolist() == R.codes_loop(v, e_loop, 0.001), (v, q)
        assert counts.sum() == n


@pytest.mark.parametrize("cells", [[1.0, math.inf], [-math.inf, 2.0], [-1e308, 1e308], [math.inf], [-math.inf, math.inf]])
def test_a_width_that_is_not_finite_leaves_every_bin_empty(cells):
    for bins in (1, 2, 5):
        for extra in ([], [math.nan], [math.nan, 3.0, math.nan]):
            v = np.array(cells + extra)
            e = R.cut_edges_loop(v, bins)
            assert math.isnan(e[0]) and bits(e) == bits(R.cut_edges(v, bins))
            assert all(math.isnan(x) or x == math.inf for x in e[:bins])
            want = R.cut_loop(v, bins)
            assert want == ["NaN"] * int(np.isnan(v).sum()) == R.cut(v, bins)
            assert set(R.codes_loop(v, e)) <= {R.NONE, R.NAN}


def test_errors_as_the_reference():
    for fn in (R.cut, R.cut_loop, R.qcut, R.qcut_loop):
        with pytest.raises(R.InvalidValue):
            fn(np.array([1.0, 2.0]), 0)                         # test_cut_zero_bins, test_qcut_zero_quantiles
        with pytest.raises(R.InvalidValue):
            fn(np.array([]), 3)
        with pytest.raises(R.InvalidValue):
            fn(np.array([math.nan]), 3)
    for fn in (R.value_range, R.value_range_loop):
        with pytest.raises(R.InvalidValue):
            fn(np.array([math.nan, math.nan]))


def test_the_references_own_vectors():
    a = np.array([1.0, 2.0, 3.0, 4.0, 5.0])                     # create_test_df, column "a"
    for fn in (R.value_range, R.value_range_loop):
        assert fn(a) == (1.0, 5.0)                              # test_value_range, functions.rs:6840-6846
        assert fn(np.array([1.0, math.nan, 3.0])) == (1.0, 3.0)
    for fn in (R.cut, R.cut_loop):
        got = fn(np.array([1.0, 2.5, 4.0, 5.0]), 2)             # test_cut, :6943-6956
        assert len(got) == 4 and ("1.00" in got[0] or "(" in got[0])
        assert got == ["(1.00, 3.00]", "(1.00, 3.00]", "(3.00, 5.00]", "(3.00, 5.00]"]
        got = fn(np.array([1.0, math.nan, 3.0]), 2)             # test_cut_with_nan, :6958-6970
        assert got[1] == "NaN" and got == ["(1.00, 2.00]", "NaN", "(2.00, 3.00]"]
        assert fn(np.array([0.0, 1e15, 5e14]), 2) == ["(0.00, 500000000000000.00]", "(500000000000000.00, 1000000000000000.00]"]
    for fn in (R.qcut, R.qcut_loop):
        got = fn(np.arange(1.0, 9.0), 4)                        # test_qcut, :6979-6997
        assert len(got) == 8 and any(s.startswith("Q") for s in got)
        assert got == ["Q1", "Q1", "Q2", "Q2", "Q3", "Q3", "Q4", "Q4"]
        got = fn(np.array([1.0, math.nan, 3.0, 4.0]), 2)        # test_qcut_with_nan, :6999-7011
        assert got[1] == "NaN" and got == ["Q1", "NaN", "Q2", "Q2"]
        assert fn(np.array([5.0, 1.0, 3.0, 3.0, 9.0]), 2) == ["Q2", "Q1", "Q2", "Q2", "Q2"]
        assert fn(np.array([1.0, 2.0]), 5) == ["Q3", "Q5"]      # m < q: repeated edges are empty bins


def test_codes_contract():
    e = [0.0, 1.0, 1.0, 2.0, math.inf]
    v = np.array([-1.0, 0.0, -0.0, 0.5, 1.0, 1.5, 2.0, 1e300, math.inf, math.nan, np.nextafter(1.0, 0.0)])
    c, counts = R.codes(v, e)
    assert c.tolist() == R.codes_loop(v, e) == [R.NONE, 0, 0, 0, 2, 2, 3, 3, R.NONE, R.NAN, 0]
    assert counts.tolist() == [4, 0, 2, 2, 2, 1]
    assert R.values_of([1, 2, 3], [False, True, False]).tolist()[0::2] == [1.0, 3.0] and math.isnan(R.values_of([1, 2, 3], [False, True, False])[1])
