"""tests/moments_ref.py (the reference's shape statistics restated line by line) against a naive numpy twin and against the
known answers of the reference's own tests of these methods (tests/golden/moments_known_answers.json).  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from tests import moments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "moments_known_answers.json")))


def _arr(cells):
    return np.array([math.nan if c is None else c for c in cells], dtype=np.float64)


def _call(op, values, args=()):
    fn = {"range": R.value_span}.get(op) or getattr(R, op)
    return fn(values, *args)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_known_answers_of_the_reference(case):
    if "columns" in case:
        got = getattr(R, case["op"])({k: _arr(v) for k, v in case["columns"].items()})
        if "equals" in case:
            assert got == [tuple(e) for e in case["equals"]]
        else:
            assert len(got) == len(case["near"])
            for (name, value), (want_name, want, tol) in zip(got, case["near"]):
                assert name == want_name and abs(value - want) < tol
        return
    v = _arr(case["input"])
    if case.get("error"):
        with pytest.raises(ValueError):
            _call(case["op"], v, case.get("args", ()))
        return
    got = _call(case["op"], v, case.get("args", ()))
    if "equals" in case:
        assert got == case["equals"]
    elif "near" in case:
        assert abs(got - case["near"][0]) < case["near"][1]
    elif case.get("nan"):
        assert math.isnan(got)
    else:
        assert case["not_nan"] and not math.isnan(got)


def test_zscore_and_describe_column_known_answers():
    z = R.zscore(_arr([1.0, 2.0, 3.0, 4.0, 5.0]))                      # functions.rs:6868-6883
    assert z[0] < 0.0 and abs(z[2]) < 0.001 and z[4] > 0.0
    d = R.describe_column(_arr([1.0, 2.0, 3.0, 4.0, 5.0]))             # :8637-8652
    assert d["count"] == 5.0 and d["mean"] == 3.0 and d["min"] == 1.0 and d["max"] == 5.0
    assert (d["25%"], d["50%"], d["75%"]) == (2.0, 3.0, 4.0)
    assert 1.0 < R.iqr(_arr([1.0, 2.0, 3.0, 4.0, 5.0])) < 3.0          # test_iqr, :8727-8737
    assert 0.0 < R.cv(_arr([10.0, 20.0, 30.0])) < 1.0                  # test_cv


# ---- the naive twin: numpy's pairwise sums and closed forms, no shared code with moments_ref ---------------------------------------
def _twin(v):
    x = v[~np.isnan(v)]
    n = x.size
    mean = x.sum() / n if n else math.nan
    d = x - mean
    return x, n, mean, d


COLUMNS = [np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([2.0, math.nan, -3.5, 0.0, 7.25, 7.25, -0.0]),
           np.random.default_rng(3).normal(5.0, 2.0, 301), np.random.default_rng(4).lognormal(0.0, 1.0, 64),
           np.array([4.0, 4.0, 4.0, 4.0]), np.array([math.nan, math.nan]), np.array([]), np.array([3.0]), np.array([3.0, 5.0]),
           np.array([1.0, 2.0, 4.0]), np.array([1.0, 2.0, 4.0, 8.0])]


@pytest.mark.parametrize("v", COLUMNS, ids=[str(i) for i in range(len(COLUMNS))])
def test_restatement_against_the_naive_twin(v):
    x, n, mean, d = _twin(v)
    close = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))   # noqa: E731
    f = R.fields(v)
    assert f["count"] == n and f["count_pos"] == int((x > 0).sum()) and f["count_nonzero"] == int((x != 0).sum())
    assert close(f["sum"], float(x.sum())) and close(f["abs_sum"], float(np.abs(x).sum()))
    assert f["min"] == (x.min() if n else math.inf) and f["max"] == (x.max() if n else -math.inf)
    for name, p in (("m2", 2), ("m3", 3), ("m4", 4)):
        if n:
            assert abs(f[name] - float((d ** p).sum())) <= 1e-9 * float((np.abs(d) ** p).sum()) + 1e-300, name
    assert close(f["abs_dev"], float(np.abs(d).sum()))
    assert close(f["log_sum"], float(np.log(x[x > 0]).sum())) and close(f["recip_sum"], float((1.0 / x[x != 0]).sum()))
    assert close(f["prod"], float(np.prod(x)))
    # the methods
    assert close(R.var_column(v, 1), float(x.var(ddof=1)) if n > 1 else math.nan) or n > 1 and abs(R.var_column(v, 1) - x.var(ddof=1)) < 1e-9
    assert close(R.var_column(v, 0), float(x.var()) if n > 0 else math.nan) or abs(R.var_column(v, 0) - x.var()) < 1e-9
    assert math.isnan(R.var_column(v, n)) and math.isnan(R.sem(v, n)) and math.isnan(R.std_column(v, n + 3))
    if n > 1:
        assert abs(R.sem(v, 1) - x.std(ddof=1) / math.sqrt(n)) < 1e-9
    assert close(R.mad(v), float(np.abs(d).mean()) if n else math.nan)
    assert close(R.value_span(v), float(x.max() - x.min()) if n else math.nan)
    assert close(R.abs_sum(v), float(np.abs(x).sum()))
    assert close(R.prod(v), float(np.prod(x)) if n else math.nan)
    s = np.sort(x)
    if n >= 3 and x.std() > 0:
        g1 = float((d ** 3).mean() / x.std() ** 3)
        assert abs(R.skew(v) - g1 * math.sqrt(n * (n - 1)) / (n - 2)) < 1e-9
    else:
        assert math.isnan(R.skew(v))
    if n >= 4 and x.std() > 0:
        g2 = float((d ** 4).mean() / x.std() ** 4) - 3.0
        assert abs(R.kurtosis(v) - (n - 1) / ((n - 2) * (n - 3)) * ((n + 1) * g2 + 6)) < 1e-9
    else:
        assert math.isnan(R.kurtosis(v))
    pos, nz = x[x > 0], x[x != 0]
    assert close(R.geometric_mean(v), float(np.exp(np.log(pos).mean())) if pos.size else math.nan) or \
        abs(R.geometric_mean(v) - np.exp(np.log(pos).mean())) < 1e-9
    assert close(R.harmonic_mean(v), float(nz.size / (1.0 / nz).sum()) if nz.size else math.nan)
    assert close(R.cv(v), float(x.std(ddof=1) / abs(mean)) if n > 1 and abs(mean) >= 2.0 ** -52 else R.cv(v)) or \
        abs(R.cv(v) - x.std(ddof=1) / abs(mean)) < 1e-9
    # the index rules
    for a in (0.0, 0.25, 0.5, 0.75, 1.0, 0.3183098861837907):
        i = int(n * a)
        assert close(R.order_stats(v, [(R.AT_FRAC_N, a)])[0][0], float(s[i]) if i < n else math.nan)
        assert close(R.percentile_value(v, a), float(s[int((n - 1) * a)]) if n else math.nan)
        if a < 0.5 and n:
            t = int(n * a)
            assert close(R.trimmed_mean(v, a), float(s[t:n - t].mean()) if n - 2 * t > 0 else math.nan) or \
                abs(R.trimmed_mean(v, a) - s[t:n - t].mean()) < 1e-9
    assert math.isnan(R.percentile_value(v, -0.1)) and math.isnan(R.percentile_value(v, 1.5))
    assert math.isnan(R.trimmed_mean(v, 0.5)) and math.isnan(R.trimmed_mean(v, -0.01))
    assert close(R.median_all({"c": v})[0][1] if n else math.nan, float(np.median(x)) if n else math.nan)
    assert close(R.iqr(v), float(s[int(n * 0.75)] - s[int(n * 0.25)]) if n >= 2 else math.nan)
    assert R.order_stats(v, [(R.MEDIAN, 0.0)])[1] == n


def test_early_returns_and_left_out_columns():
    nan = math.nan
    for n in range(0, 5):
        v = np.arange(1.0, n + 1.0)
        assert math.isnan(R.skew(v)) == (n < 3) and math.isnan(R.kurtosis(v)) == (n < 4)
        assert math.isnan(R.var_column(v, 1)) == (n <= 1) and math.isnan(R.sem(v, 2)) == (n <= 2)
        assert math.isnan(R.mad(v)) == (n == 0) and math.isnan(R.prod(v)) == (n == 0) and math.isnan(R.iqr(v)) == (n < 2)
    const = np.full(6, 2.5)
    assert math.isnan(R.skew(const)) and math.isnan(R.kurtosis(const)) and R.cv(const) == 0.0
    assert math.isnan(R.cv(np.array([-1.0, 1.0]))) and math.isnan(R.cv(np.array([1e-17, 1e-17])))       # mean.abs() < EPSILON
    for bad in (np.array([1.0]), np.array([nan, 2.0]), np.full(4, 7.0)):
        with pytest.raises(ValueError):
            R.zscore(bad)
    assert R.describe_column(np.array([nan])) == {"count": 0.0, "mean": nan, "std": nan, "min": nan, "max": nan} or \
        R.describe_column(np.array([nan]))["count"] == 0.0
    assert R.describe_column(np.array([5.0]))["std"] == 0.0                                             # (n - 1).max(1.0)
    cols = {"a": np.array([1.0, 2.0]), "e": np.array([nan]), "one": np.array([4.0])}
    assert [k for k, _ in R.sum_all(cols)] == ["a", "e", "one"] and R.sum_all(cols)[1][1] == 0.0
    for fn in (R.mean_all, R.min_all, R.max_all, R.product_all, R.median_all):
        assert [k for k, _ in fn(cols)] == ["a", "one"], fn.__name__
    for fn in (R.var_all, R.std_all):
        assert [k for k, _ in fn(cols)] == ["a"], fn.__name__
    # ties at both trim cuts count as often as the slice holds them
    v = np.array([1.0, 1.0, 1.0, 2.0, 3.0, 3.0, 3.0, 3.0])
    assert R.trimmed_mean(v, 0.25) == (1.0 + 2.0 + 3.0 + 3.0) / 4.0
    assert R.fields(np.array([]))["sum"] == 0.0 and math.copysign(1.0, R.fields(np.array([]))["sum"]) == -1.0
