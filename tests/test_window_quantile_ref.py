"""tests/window_quantile_ref.py (the numpy twins of pandrs_hip_window_quantile) against a line-by-line pure-Python
restatement of the reference's loops (src/series/window.rs:163-203, :298-336, :379-400, :494-530 and
helpers/window_ops.rs:206-240) on random small inputs, and against the reference's own known answers
(tests/golden/window_quantile_known_answers.json).  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from tests import window_quantile_ref as R
from tests.window_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference, line by line (Option<f64> = None or a float) -----------------------------------------------------------
def rust_round(x):
    return math.floor(x + 0.5) if x - math.floor(x) != 0.5 else math.floor(x) + 1      # x >= 0: half goes up = away from zero


def ref_median(values):                                  # window.rs:299-307
    srt = sorted(values)                                 # stable; no NaN reaches it here
    mid = len(srt) // 2
    if len(srt) % 2 == 0:
        return (srt[mid - 1] + srt[mid]) / 2.0
    return srt[mid]


def ref_quantile(values, q):                             # window.rs:324-328
    srt = sorted(values)
    idx = int(rust_round(q * float(len(srt) - 1)))
    return srt[min(idx, len(srt) - 1)]


def ref_rolling(cells, window_size, min_periods, center, func):       # window.rs:163-203
    out = []
    min_periods = window_size if min_periods is None else min_periods  # :146
    for i in range(len(cells)):
        if center:
            half_window = window_size // 2
            start = i - half_window if i >= half_window else 0
            end = min(start + window_size, len(cells))
        else:
            start = i + 1 - window_size if i + 1 >= window_size else 0
            end = i + 1
        window_values = [v for v in cells[start:end] if v is not None]
        out.append(func(window_values) if len(window_values) >= min_periods else None)
    return [float("nan") if v is None else v for v in out]             # :309-313


def ref_expanding(cells, min_periods, func):                           # window.rs:379-400
    out = []
    for i in range(len(cells)):
        window_values = [v for v in cells[0:i + 1] if v is not None]
        out.append(func(window_values) if len(window_values) >= min_periods else None)
    return [float("nan") if v is None else v for v in out]


def guard(func):
    """The entry's deviation for the windows the reference cannot answer: an empty one (it panics) gives NaN."""
    return lambda values: func(values) if values else float("nan")


def ref_rolling_median_compat(values, window, min_periods):            # window_ops.rs:206-240
    min_periods = window if min_periods is None else min_periods
    out = []
    for i in range(len(values)):
        start = max(0, i - max(0, window - 1))
        window_values = [v for v in values[start:i + 1] if not math.isnan(v)]
        out.append(guard(ref_median)(window_values) if len(window_values) >= min_periods else float("nan"))
    return out


def sorted_is_rusts(cells):
    """Python's sorted() ties -0.0 with 0.0 and is stable, as Rust's sort_by(partial_cmp); NaN values are kept out of the inputs."""
    return all(v is None or not math.isnan(v) for v in cells)


def random_column(rng, n, kind):
    if kind == "ties":
        x = rng.integers(-2, 3, n).astype(np.float64)
    elif kind == "zeros":
        x = rng.choice(np.array([0.0, -0.0, 1.0, -1.0]), n)
    elif kind == "wide":
        x = rng.choice(np.array([np.inf, -np.inf, 1.7e308, -1.7e308, 1.0, 2.5]), n)
    else:
        x = rng.normal(size=n)
    return x


QS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.0 / 3.0)


@pytest.mark.parametrize("data", ["normal", "ties", "zeros", "wide"])
def test_twins_match_the_reference_loops(data):
    rng = np.random.default_rng(["normal", "ties", "zeros", "wide"].index(data))
    for trial in range(60):
        n = int(rng.integers(1, 40))
        x = random_column(rng, n, data)
        valid = rng.random(n) >= rng.choice([0.0, 0.1, 0.5, 1.0])
        cells = [float(v) if ok else None for v, ok in zip(x, valid)]
        assert sorted_is_rusts(cells)
        w = int(rng.choice([1, 2, 3, 4, 7, n, n + 5, 2 * n + 3]))
        center = bool(rng.integers(0, 2))
        mp = rng.choice([None, 0, 1, w])
        mp = None if mp is None else int(mp)
        emp = int(rng.choice([0, 1, 5]))
        for median, q in [(True, 0.5)] + [(False, q) for q in QS]:
            func = guard(ref_median if median else (lambda v, q=q: ref_quantile(v, q)))
            want = np.array(ref_rolling(cells, w, mp, center, func))
            for twin in (R.window_quantile_ref, R.window_quantile_fast):
                got = twin(x, valid, "rolling", w, center, mp, median, q)
                assert same(got, want), (data, trial, twin.__name__, w, center, mp, median, q)
            want = np.array(ref_expanding(cells, emp, func))
            for twin in (R.window_quantile_ref, R.window_quantile_fast):
                assert same(twin(x, valid, "expanding", min_periods=emp, median=median, q=q), want), (data, trial, twin.__name__, emp, median, q)


def test_twins_match_the_compat_rolling_median():
    rng = np.random.default_rng(5)
    for trial in range(80):
        n = int(rng.integers(1, 40))
        x = random_column(rng, n, ["normal", "ties", "zeros"][trial % 3])
        x[rng.random(n) < rng.choice([0.0, 0.2, 0.6])] = np.nan
        window = int(rng.choice([0, 1, 2, 3, 5, n + 2]))
        mp = rng.choice([None, 1, 2])
        mp = None if mp is None else int(mp)
        want = np.array(ref_rolling_median_compat([float(v) for v in x], window, mp))
        w = max(window, 1)                                                 # saturating_sub: window 0 acts as 1 ...
        emp = window if mp is None else mp                                 # ... but min_periods stays the caller's window
        for twin in (R.window_quantile_ref, R.window_quantile_fast):
            got = twin(x, None, "rolling", w, False, emp, True, nan_missing=True)
            assert same(got, want), (trial, twin.__name__, window, mp)


def test_documented_deviations():
    x = np.array([1.0, np.nan, 3.0, 2.0, 5.0])
    for twin in (R.window_quantile_ref, R.window_quantile_fast):
        # a NaN value that is not missing poisons its windows; with nan_missing it is skipped
        assert same(twin(x, None, "rolling", 2, False, 1, True), [1.0, np.nan, np.nan, 2.5, 3.5])
        assert same(twin(x, None, "rolling", 2, False, 1, True, nan_missing=True), [1.0, 1.0, 3.0, 2.5, 3.5])
        # an empty window under min_periods 0: NaN where the reference panics
        valid = np.array([False, False, True, True, True])
        assert same(twin(x, valid, "expanding", min_periods=0), [np.nan, np.nan, 3.0, 2.5, 3.0])


def test_half_away_rounding_and_signed_zeros():
    assert [int(R.rust_round(np.float64(v))) for v in (0.5, 1.5, 2.5, 0.49999999999999994, 2.0)] == [1, 2, 3, 0, 2]
    # q = 0.5 with even len: idx = round(0.5 * (len - 1)) = the upper middle
    x = np.array([4.0, 1.0, 3.0, 2.0])
    for twin in (R.window_quantile_ref, R.window_quantile_fast):
        assert same(twin(x, None, "expanding", min_periods=1, median=False, q=0.5), [4.0, 4.0, 3.0, 3.0])
        z = np.array([0.0, -0.0, -0.0, 0.0])
        got = twin(z, None, "rolling", 2, False, 1, True)                  # ties keep row order: the mean keeps the sum's sign
        assert same(got, [0.0, 0.0, -0.0, 0.0])
        got = twin(z, None, "rolling", 3, False, 3, True)                  # sorted = row order: the middle cell
        assert same(got, [np.nan, np.nan, -0.0, -0.0])
        big = np.array([1.7e308, 1.7e308])
        assert same(twin(big, None, "expanding", min_periods=2), [np.nan, np.inf])      # one add, one divide: the overflow is kept
        i = np.array([2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2], np.int64)       # distinct integers that tie as f64
        assert same(twin(i, None, "rolling", 3, False, 1, True), [2.0 ** 53, 2.0 ** 53, 2.0 ** 53])


def test_known_answers_of_the_reference():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "window_quantile_known_answers.json")))
    assert len(doc["cases"]) >= 5
    for case in doc["cases"]:
        x = np.array(case["values"], np.float64)
        for twin in (R.window_quantile_ref, R.window_quantile_fast):
            got = twin(x, None, case["kind"], case["window"], case["center"], case["min_periods"], case["stat"] == "median",
                       0.5 if case["q"] is None else case["q"], nan_missing=case["nan_missing"])
            for row, want in case["checks"]:
                if want is None:
                    assert np.isnan(got[row]), (case["source"], row)
                elif case["tol"] == 0:
                    assert got[row] == want, (case["source"], row)
                else:
                    assert abs(got[row] - want) < case["tol"], (case["source"], row)
    assert all(not (0.0 <= q <= 1.0) for q in doc["rejected_q"])
