"""tests/cumulative_ref.py against itself and against the reference's known answers (src/dataframe/pandas_compat/functions.rs
:4411-4447, :4547-4573, :6580-6595): the line-for-line loops equal the vectorised twins bit for bit on seeded random cases,
both reproduce the fixtures, the quirks of the reference's folds and the sticky cases of cumprod.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from tests.cumulative_ref import (COUNT, CUM_OPS, DIFF, LAG_OPS, MAX, MIN, NAN, PCT_CHANGE, PROD, SHIFT, SUM, cum_loop, cum_twin, gamma, lag_loop,
                                  lag_twin, same_bits, sum_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "cumulative_known_answers.json")))
CUM = {"cumsum": SUM, "cumprod": PROD, "cummax": MAX, "cummin": MIN, "cumcount": COUNT}
LAG = {"shift": SHIFT, "diff": DIFF, "pct_change": PCT_CHANGE}
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, 1.7976931348623157e308, 1e200, 1e-200, 2.5])


def columns(rng, cases):
    for k in range(cases):
        n = int(rng.integers(0, 70))
        kind = k % 4
        if kind == 0:
            x = rng.normal(0.0, 3.0, n)
        elif kind == 1:
            x = SPECIAL[rng.integers(0, len(SPECIAL), n)]
        elif kind == 2:
            x = rng.integers(-9, 9, n).astype(np.float64)
        else:
            x = rng.integers(-2**40, 2**40, n)
        yield x, (rng.random(n) < 0.3 if k % 3 else None)


def test_loops_equal_twins():
    rng = np.random.default_rng(2024)
    cases = 0
    for x, nulls in columns(rng, 240):
        for op in CUM_OPS:
            a, ga = cum_loop(x, nulls, op)
            b, gb = cum_twin(x, nulls, op)
            assert same_bits(a, b) and np.array_equal(ga, gb), (cases, op, x, nulls)
            assert a.dtype == (np.int64 if op == COUNT else np.float64)
        n = x.shape[0]
        for op in LAG_OPS:
            for periods in (0, 1, 2, 7, n - 1, n, n + 5) + ((-1, -3, -n - 5) if op == SHIFT else ()):
                if periods < 0 and op != SHIFT:
                    continue
                a, ga = lag_loop(x, nulls, op, periods)
                b, gb = lag_twin(x, nulls, op, periods)
                assert same_bits(a, b) and np.array_equal(ga, gb), (cases, op, periods, x, nulls)
        cases += 1
    assert cases == 240


@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_known_answers(loop, case):
    x = np.array([np.nan if v is None else v for v in case["input"]], np.float64)
    if case["op"] in CUM:
        got, gone = (cum_loop if loop else cum_twin)(x, None, CUM[case["op"]])
        assert not gone.any() and list(got) == case["expected"]
        assert got.dtype == (np.int64 if case["op"] == "cumcount" else np.float64)
        return
    got, gone = (lag_loop if loop else lag_twin)(x, None, LAG[case["op"]], case["periods"])
    for g, bit, want in zip(got, gone, case["expected"]):
        if want is None:
            assert np.isnan(g) and bit == (case["op"] == "shift")          # shift: None; diff / pct_change: a NaN value
        else:
            assert not bit and abs(g - want) <= case.get("tolerance", 0.0)


@pytest.mark.parametrize("cum,lag", [(cum_loop, lag_loop), (cum_twin, lag_twin)])
def test_quirks_of_the_reference_folds(cum, lag):
    got, _ = cum(np.array([np.nan, 2.0, np.nan, 1.0, 3.0]), None, MAX)             # a leading NaN: the fold's start shows
    assert same_bits(got, np.array([-np.inf, 2.0, 2.0, 2.0, 3.0]))
    got, _ = cum(np.array([np.nan, 2.0, np.nan, 1.0, 3.0]), None, MIN)
    assert same_bits(got, np.array([np.inf, 2.0, 2.0, 1.0, 1.0]))
    got, _ = cum(np.array([-0.0, -0.0, -0.0]), None, SUM)                          # +0.0 + -0.0 = +0.0
    assert same_bits(got, np.zeros(3))
    got, _ = cum(np.array([1.0, np.nan, 3.0]), None, SUM)                          # NaN is sticky
    assert same_bits(got, np.array([1.0, NAN, NAN]))
    got, _ = cum(np.array([1.0, np.inf, -np.inf, 2.0]), None, SUM)
    assert same_bits(got, np.array([1.0, np.inf, NAN, NAN]))
    got, _ = cum(np.array([0.0, -0.0, 0.0, -0.0]), None, MAX)                      # -0.0 is below +0.0
    assert same_bits(got, np.array([0.0, 0.0, 0.0, 0.0]))
    got, _ = cum(np.array([0.0, -0.0, 0.0, -0.0]), None, MIN)
    assert same_bits(got, np.array([0.0, -0.0, -0.0, -0.0]))
    got, _ = cum(np.array([-0.0, 0.0]), None, MAX)
    assert same_bits(got, np.array([-0.0, 0.0]))
    got, gone = lag(np.array([-0.0, 5.0, 0.0, 1.0, np.inf, 3.0, np.nan, 2.0]), None, PCT_CHANGE, 1)      # prev == 0.0: -0.0 too
    assert same_bits(got, np.array([NAN, NAN, -1.0, NAN, np.inf, NAN, NAN, NAN])) and not gone.any()
    got, gone = lag(np.array([1.0, 2.0, 4.0]), None, DIFF, 0)
    assert same_bits(got, np.zeros(3)) and not gone.any()
    got, gone = lag(np.array([1.0, 2.0, 4.0]), None, SHIFT, -1)
    assert same_bits(got, np.array([2.0, 4.0, NAN])) and list(gone) == [False, False, True]
    for periods in (3, 4, 99, -3, -99):
        got, gone = lag(np.array([1.0, 2.0, 4.0]), None, SHIFT, periods)
        assert gone.all() and np.isnan(got).all()


@pytest.mark.parametrize("cum", [cum_loop, cum_twin])
def test_cumprod_is_sticky_after_a_range_excursion(cum):
    over = [1e200, 1e200]                                                          # inf at row 1
    under = [1e-200, 1e-200]                                                       # 0 at row 1
    got, _ = cum(np.array(over + [1e-200, 1e-200, 1e-200, -1.0]), None, PROD)     # an overflow then small factors
    assert same_bits(got, np.array([1e200, np.inf, np.inf, np.inf, np.inf, -np.inf]))
    got, _ = cum(np.array(under + [1e200, 1e200, 1e200, -1.0]), None, PROD)       # an underflow to zero then large factors
    assert same_bits(got, np.array([1e-200, 0.0, 0.0, 0.0, 0.0, -0.0]))
    got, _ = cum(np.array(over + [2.0, 0.0, 3.0]), None, PROD)                    # each followed by a 0 ...
    assert same_bits(got, np.array([1e200, np.inf, np.inf, NAN, NAN]))
    got, _ = cum(np.array(under + [2.0, 0.0, 3.0]), None, PROD)
    assert same_bits(got, np.array([1e-200, 0.0, 0.0, 0.0, 0.0]))
    got, _ = cum(np.array(over + [2.0, np.inf, 3.0]), None, PROD)                 # ... or an inf
    assert same_bits(got, np.array([1e200, np.inf, np.inf, np.inf, np.inf]))
    got, _ = cum(np.array(under + [2.0, np.inf, 3.0]), None, PROD)
    assert same_bits(got, np.array([1e-200, 0.0, 0.0, NAN, NAN]))
    got, _ = cum(np.array([1e-200, 1e200, 1e200, 1e-200]), None, PROD)            # no running product leaves the range
    assert np.all(np.abs(got / np.array([1e-200, 1.0, 1e200, 1.0]) - 1.0) <= 2 * gamma(np.arange(1, 5)))


@pytest.mark.parametrize("cum,lag", [(cum_loop, lag_loop), (cum_twin, lag_twin)])
def test_the_mask_rule(cum, lag):
    i = np.array([7, 100, 2, -3, 1], np.int64)
    nulls = np.array([False, True, False, False, False])
    got, gone = cum(i, nulls, SUM)
    assert same_bits(got, np.array([7.0, NAN, 9.0, 6.0, 7.0])) and list(gone) == list(nulls)
    got, gone = cum(i, nulls, PROD)
    assert same_bits(got, np.array([7.0, NAN, 14.0, -42.0, -42.0])) and list(gone) == list(nulls)
    got, gone = cum(i, nulls, MAX)
    assert same_bits(got, np.array([7.0, NAN, 7.0, 7.0, 7.0])) and list(gone) == list(nulls)
    got, gone = cum(i, nulls, COUNT)
    assert got.dtype == np.int64 and list(got) == [1, 1, 2, 3, 4] and not gone.any()
    got, gone = lag(i, nulls, SHIFT, 1)
    assert same_bits(got, np.array([NAN, 7.0, NAN, 2.0, -3.0])) and list(gone) == [True, False, True, False, False]
    got, gone = lag(i, nulls, DIFF, 1)
    assert same_bits(got, np.array([NAN, NAN, NAN, -5.0, 4.0])) and list(gone) == [False, True, True, False, False]
    got, gone = lag(i, nulls, PCT_CHANGE, 2)
    assert same_bits(got, np.array([NAN, NAN, (2.0 - 7.0) / 7.0, NAN, (1.0 - 2.0) / 2.0])) and list(gone) == [False, False, False, True, False]
    for op in CUM_OPS:
        got, gone = cum(np.array([], np.float64), None, op)
        assert got.shape == (0,) and gone.shape == (0,)


def test_a_blocked_scan_stays_far_inside_the_sum_bound():
    """What makes the device's SUM contract checkable: a 4096-row blocked scan against the sequential fold over 300 000
    normal x lognormal rows differs by at most 0.001 of 2 gamma_k sum|x| (so a correct kernel cannot fail the bound), while a
    dropped block carry misses it by orders of magnitude (so the bound hides no such bug)."""
    rng = np.random.default_rng(5)
    n, blk = 300_000, 4096
    x = rng.normal(0.0, 1.0, n) * rng.lognormal(0.0, 2.0, n)
    ref, _ = cum_twin(x, None, SUM)
    got, carry = np.empty(n), 0.0
    for s in range(0, n, blk):
        got[s:s + blk] = carry + np.cumsum(x[s:s + blk])
        carry = got[min(s + blk, n) - 1]
    bound = sum_bound(x)
    assert np.all(np.abs(got - ref)[1:] <= 0.001 * bound[1:]) and got[0] == ref[0]
    dropped = got.copy()
    dropped[blk:2 * blk] = np.cumsum(x[blk:2 * blk])
    assert np.any(np.abs(dropped - ref) > 1000 * bound)
    assert math.isclose(float(gamma(4)), 4 * 2.0 ** -53, rel_tol=1e-12)
