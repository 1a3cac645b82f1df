"""tests/fill_ref.py against itself and against the reference's known answers (src/dataframe/pandas_compat/functions.rs
:4751-4970, :8007-8050, :8489): the line-for-line loop equals the vectorised twin bit for bit on the shared random cases, and
both reproduce the fixtures.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests.fill_ref import BFILL, FFILL, LINEAR, METHODS, VALUE, fill_loop, fill_twin, same_bits, sweep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fill_known_answers.json")))
OPS = {"ffill": FFILL, "bfill": BFILL, "interpolate": LINEAR, "fillna": VALUE}
NAN = np.uint64(0x7FF8000000000000).view(np.float64)


def test_loop_equals_twin_on_the_sweep():
    cases, seen = 0, set()
    for x, nulls, method, value in sweep_cases(np.random.default_rng(2024), cases=300, tile=256):
        a, ga = fill_loop(x, nulls, method, value)
        b, gb = fill_twin(x, nulls, method, value)
        assert same_bits(a, b) and np.array_equal(ga, gb), (cases, method, x.dtype)
        assert a.dtype == (np.int64 if x.dtype == np.int64 and method != LINEAR else np.float64)
        seen.add((method, x.dtype.name, nulls is not None, bool(ga.any())))
        cases += 1
    assert cases == 300
    for method in METHODS:
        for dt in ("int64", "float64"):
            assert any(s[0] == method and s[1] == dt for s in seen)


@pytest.mark.parametrize("fn", [fill_loop, fill_twin])
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_known_answers(fn, case):
    x = np.array([np.nan if v is None else v for v in case["input"]], np.float64)
    want = np.array([NAN if v is None else v for v in case["expected"]], np.float64)
    got, gone = fn(x, None, OPS[case["op"]], case["value"])
    assert same_bits(got, want) and np.array_equal(gone, np.isnan(want))


@pytest.mark.parametrize("fn", [fill_loop, fill_twin])
def test_the_extensions(fn):
    i = np.array([7, 0, 0, -3, 0], np.int64)
    nulls = np.array([False, True, True, False, True])
    for method, want, gone in ((FFILL, [7, 7, 7, -3, -3], [0] * 5), (BFILL, [7, -3, -3, -3, 0], [0, 0, 0, 0, 1])):
        got, g = fn(i, nulls, method)
        assert got.dtype == np.int64 and list(got) == want and list(g) == [bool(v) for v in gone]
    got, g = fn(i, nulls, LINEAR)
    assert got.dtype == np.float64 and same_bits(got, np.array([7.0, 7 + (-10.0 * 1.0) / 3.0, 7 + (-10.0 * 2.0) / 3.0, -3.0, NAN]))
    assert list(g) == [False, False, False, False, True]
    x = np.array([1.0, 99.0, np.nan, 3.0])                      # a null over a finite number is never a source
    got, g = fn(x, np.array([False, True, False, False]), FFILL)
    assert list(got) == [1.0, 1.0, 1.0, 3.0] and not g.any()
    got, g = fn(np.array([np.inf, np.nan, -np.inf]), None, LINEAR)     # inf - inf: NaN in the data, not missing
    assert np.isnan(got[1]) and not g.any()
    got, g = fn(np.array([np.nan, 1.0]), None, VALUE, float("nan"))    # a NaN fill leaves the row missing
    assert same_bits(got, np.array([NAN, 1.0])) and list(g) == [True, False]
    got, g = fn(np.array([], np.float64), None, LINEAR)
    assert got.shape == (0,) and g.shape == (0,)
