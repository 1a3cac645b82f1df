"""tests/describe_ref.py (the numpy restatement of src/stats/descriptive.rs:91-200 the GPU tests compare against) against a
naive twin written with Python floats, `sorted` and for loops, bit for bit on the order statistics, and against the
reference's own known answers (descriptive.rs:612-632, split_dataframe/stats.rs:567-583,
tests/stats_comprehensive_test.rs:478-487)."""
import math
import struct

import numpy as np
import pytest

from tests.describe_ref import describe_ref, percentile_ref


def _bits(v):
    return struct.pack("<d", float(v))


def naive_percentile(s, p):
    if not s:
        raise ValueError("empty")
    if p < 0.0 or p > 100.0:
        raise ValueError("range")
    if p == 0.0:
        return s[0]
    if p == 100.0:
        return s[len(s) - 1]
    index = (p / 100.0) * float(len(s) - 1)
    lower, upper = int(math.floor(index)), int(math.ceil(index))
    if lower == upper:
        return s[lower]
    weight = index - float(lower)
    return s[lower] * (1.0 - weight) + s[upper] * weight


def naive_describe(cells):
    """cells: Python floats in row order (None = null)."""
    data = [float(v) for v in cells if v is not None]
    if not data:
        raise ValueError("empty")
    s = sorted(data, key=lambda v: (math.isnan(v), 0.0 if math.isnan(v) else v, 0 if math.copysign(1.0, v) < 0 else 1))
    total = -0.0
    for v in data:
        total += v
    mean = total / float(len(data))
    sq = -0.0
    for v in data:
        sq += (v - mean) * (v - mean)
    var = sq / float(len(data) - 1) if len(data) > 1 else float("nan")
    return {"count": len(data), "mean": mean, "std": math.sqrt(var) if var == var else float("nan"), "min": s[0],
            "25%": naive_percentile(s, 25.0), "50%": naive_percentile(s, 50.0), "75%": naive_percentile(s, 75.0), "max": s[-1]}


def _same(a, b):
    return (a != a and b != b) or _bits(a) == _bits(b)


def _agree(x, nulls=None, dtype=np.float64):
    cells = [None if (nulls is not None and nulls[i]) else (int(v) if dtype == np.int64 else float(v)) for i, v in enumerate(x)]
    want = naive_describe(cells)
    got = describe_ref(np.asarray(x, dtype), nulls, dtype)
    assert got["count"] == want["count"]
    for k in ("min", "25%", "50%", "75%", "max", "mean", "std"):
        assert _same(float(got[k]), want[k]), (k, got[k], want[k], list(x))


@pytest.mark.parametrize("n", range(1, 13))
def test_every_small_count_matches_the_naive_twin(n):
    rng = np.random.default_rng(n)
    _agree(rng.normal(0, 10, n))
    _agree(rng.integers(-5, 5, n), dtype=np.int64)
    nulls = rng.random(n) < 0.3
    if not nulls.all():
        _agree(rng.normal(0, 1, n), nulls)
    s = np.sort(rng.normal(0, 1, n))
    for p in (0.0, 5.0, 10.0, 25.0, 33.3, 50.0, 75.0, 90.0, 99.9, 100.0):
        assert _same(float(percentile_ref(s, p)), naive_percentile([float(v) for v in s], p))


def test_ties_at_the_quartile_ranks_nan_and_signed_zero():
    _agree([1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 3.0, 4.0])           # index 1.75 / 3.5 / 5.25 fall inside runs
    _agree([5.0, 5.0, 5.0, 5.0, 7.0, 7.0, 7.0, 7.0, 7.0])       # the median on a run boundary
    _agree([0.0, -0.0, 0.0, -0.0, 1.0])                         # -0.0 before +0.0
    _agree([1.0, float("nan"), 3.0, 2.0, float("nan")])        # NaN after every number: 75% and max are NaN
    _agree([float("nan")] * 3)
    _agree([float("inf"), -float("inf"), 0.0, 1.0])
    got = describe_ref(np.array([1.0, np.nan, 3.0, 2.0, np.nan]), None, np.float64)
    assert got["count"] == 5 and got["min"] == 1.0 and got["50%"] == 3.0 and np.isnan(got["75%"]) and np.isnan(got["max"])
    big = np.array([2**53 + 1, 2**53 + 2, 2**53, -2**62, 2**63 - 1, -2**63], np.int64)
    _agree(big, dtype=np.int64)


def test_the_references_known_answers():
    d = describe_ref(np.array([1.0, 2.0, 3.0, 4.0, 5.0]), None, np.float64)          # descriptive.rs:612-623, stats.rs:567-583
    assert (d["count"], d["mean"], d["50%"], d["min"], d["max"]) == (5, 3.0, 3.0, 1.0, 5.0) and d["max"] - d["min"] == 4.0
    assert d["25%"] == 2.0 and d["75%"] == 4.0 and _same(float(d["std"]), math.sqrt(2.5))
    s = np.array([1.0, 2.0, 3.0, 4.0, 5.0])                                        # descriptive.rs:625-632
    assert (percentile_ref(s, 0.0), percentile_ref(s, 50.0), percentile_ref(s, 100.0)) == (1.0, 3.0, 5.0)
    c = describe_ref(np.array([5.0] * 5), None, np.float64)                        # stats_comprehensive_test.rs:478-482
    assert c["std"] == 0.0
    for bad in (-1.0, 101.0):                                                      # :484-487
        with pytest.raises(ValueError):
            percentile_ref(s, bad)
    with pytest.raises(ValueError):
        describe_ref(np.array([]), None, np.float64)
    with pytest.raises(ValueError):
        describe_ref(np.array([1.0, 2.0]), np.array([True, True]), np.float64)
    assert np.isnan(describe_ref(np.array([4.0]), None, np.float64)["std"])        # 0.0 / 0.0
