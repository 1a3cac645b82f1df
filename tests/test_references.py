"""The references the GPU tests trust bit for bit (tests/window_ref.py, tests/sort_ref.py, helpers.filter_ref), checked
here without a GPU against independent, deliberately naive restatements: a per-row Python loop over each window, a closed
form in exact rational arithmetic, a comparator sort.  Every comparison but the EWM one is bit for bit.  Also: the
generator of experiments/fuzz_ops.py, run dry (no engine call), reaches every feature it means to reach at the seeds and
case counts tests/test_gpu_fuzz.py uses, and the twins of the newer kinds take every case their generators draw."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from pandrs_amd import _lib as L
from tests import window_ref as WR
from tests.helpers import filter_ref
from tests.sort_ref import STRINGS, Col, ref_cmp, ref_lexsort
from tests.test_gpu_fuzz import FUZZ_OPS_SLICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("sum", "mean", "var", "std", "min", "max", "count")
SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e300, -1e-300]


def data(rng, n, null_p):
    x = np.round(rng.normal(0, 100, n), int(rng.integers(0, 4)))
    k = rng.random(n) < 0.25
    x[k] = rng.choice(SPECIALS, size=int(k.sum()))
    return x, rng.random(n) >= null_p


# ---- the naive twins -----------------------------------------------------------------------------------------------------
def total_order(v):
    return (v, 0 if np.signbit(v) else 1)                       # -0.0 < +0.0


def naive_extreme(vals, mx):
    cands = [v for v in vals if v == v] + [np.float64(-np.inf if mx else np.inf)]   # the fold's start
    return max(cands, key=total_order) if mx else min(cands, key=total_order)


def naive_window(i, n, w, center):
    if center:
        s = i - w // 2 if i >= w // 2 else 0
        return s, min(s + w, n)
    return (i + 1 - w if i + 1 >= w else 0), i + 1


def naive_rolling(x, valid, w, center, op, mp, ddof):
    n = len(x)
    out = np.empty(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e = naive_window(i, n, w, center)
            vals = [x[j] for j in range(s, e) if valid[j]]
            cnt = len(vals)
            enough = cnt >= (w if mp is None else mp)
            if op == "count":
                out[i] = cnt if enough else 0
                continue
            out[i] = np.nan
            if not enough:
                continue
            if op in ("min", "max"):
                out[i] = naive_extreme(vals, op == "max")
                continue
            acc = np.float64(-0.0)
            for v in vals:
                acc = acc + v
            if op == "sum":
                out[i] = acc
                continue
            mean = acc / np.float64(cnt)
            if op == "mean":
                out[i] = mean
                continue
            sq = np.float64(-0.0)
            for v in vals:                                      # the second pass of the two-pass fold
                d = v - mean
                sq = sq + d * d
            if cnt > ddof:
                var = sq / np.float64(cnt - ddof)
                out[i] = var if op == "var" else np.sqrt(var)
    return out


ROLLING_CASES = [  # (n, w, center, min_periods, ddof, null rate)
    (400, 7, False, None, 1, 0.1), (400, 7, True, 1, 0, 0.1), (257, 64, False, 0, 1, 0.3), (257, 65, True, 3, 2, 0.0),
    (130, 1, False, None, 1, 0.2), (130, 1, True, 0, 0, 0.2), (90, 200, False, 1, 1, 0.1), (90, 95, True, 0, 1, 0.5),
    (64, 64, False, None, 1, 0.0), (100, 13, True, 5, 1, 1.0), (100, 13, False, 0, 0, 1.0), (33, 2, True, 2, 1, 0.9),
    (1, 3, False, 0, 1, 0.0), (2, 2, True, 1, 1, 0.0)]


@pytest.mark.parametrize("case", ROLLING_CASES, ids=lambda c: "n%d-w%d-c%d-mp%s-ddof%d-null%g" % c)
def test_rolling_ref_is_the_per_row_loop(case):
    n, w, center, mp, ddof, null_p = case
    rng = np.random.default_rng(n * 1000 + w)
    x, valid = data(rng, n, null_p)
    for op in OPS:
        got = WR.rolling_ref(x, valid, w, center, op, mp=mp, ddof=ddof)
        want = naive_rolling(x, valid, w, center, op, mp, ddof)
        assert WR.same(got, want), (op, WR.first_diff(got, want))
    if n > 1:                                                   # expanding_ref_exact: the window is every row so far
        for op in ("min", "max", "count"):
            got = WR.expanding_ref_exact(x, valid, op, 2)
            want = naive_rolling(x, valid, n + 1, False, op, 2, 1)
            assert WR.same(got, want), (op, WR.first_diff(got, want))


def test_same_and_first_diff_tell_zero_signs_and_nan_positions():
    a = np.array([0.0, np.nan, 1.0])
    assert WR.same(a, a.copy()) and WR.first_diff(a, a.copy()) is None
    assert not WR.same(a, np.array([-0.0, np.nan, 1.0])) and WR.first_diff(np.array([-0.0, np.nan, 1.0]), a)[0] == 0
    assert not WR.same(a, np.array([0.0, 2.0, 1.0])) and WR.first_diff(np.array([0.0, 2.0, 1.0]), a)[0] == 1
    assert not WR.same(a, a[:2])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_sparse_table_extreme_is_the_loop(n):
    rng = np.random.default_rng(n)
    x, valid = data(rng, n, 0.2)
    x[rng.random(n) < 0.3] = rng.choice([0.0, -0.0, 5.0])       # ties between the zero signs
    for w in sorted({1, 2, 3, 4, 5, 8, 9, 16, 17, max(n - 1, 1), n, n + 1}):
        for center in (False, True):
            s, e = WR.bounds(n, w, center)
            for mx in (False, True):
                got = WR.extreme(x, valid, s, e, mx)
                want = np.array([naive_extreme([x[j] for j in range(*naive_window(i, n, w, center)) if valid[j]], mx) for i in range(n)])
                assert got.tobytes() == want.tobytes(), (w, center, mx, WR.first_diff(got, want))


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.05, 2.0 / 31.0, 0.999])
def test_ewm_mean_against_the_closed_form_in_exact_arithmetic(alpha):
    """y_k = b^k v_0 + sum_{j=1..k} a b^(k-j) v_j over the non-null values, a = alpha and b = fl(1 - alpha) as the loop has
    them, in fractions.Fraction.  The loop rounds three times per step (a * v, b * y, the sum), each by at most 2^-53
    relative, and a * |v| + b * |y| <= max |v|: after k steps the error is at most 3 k 2^-53 max |v|."""
    rng = np.random.default_rng(int(alpha * 1000))
    for n in (1, 2, 9, 40):
        x = rng.normal(10, 5, n)
        valid = rng.random(n) > 0.25
        valid[:min(n, 2)] = False
        if n > 2:
            valid[2] = True
        got = WR.ewm_ref(x, valid, alpha, "mean")
        a, b = Fraction(alpha), Fraction(1.0 - alpha)
        seen = []
        for i in range(n):
            if valid[i]:
                seen.append(Fraction(float(x[i])))
            if not seen:
                assert np.isnan(got[i])
                continue
            k = len(seen) - 1
            exact = b ** k * seen[0] + sum(a * b ** (k - j) * seen[j] for j in range(1, k + 1))
            tol = 3 * k * Fraction(1, 2 ** 53) * max(abs(v) for v in seen)
            assert abs(Fraction(float(got[i])) - exact) <= tol, (n, i, k)
        if seen:
            first = int(np.flatnonzero(valid)[0])
            assert got[first] == x[first]                       # k = 0: the first value itself, exactly


# ---- sort ---------------------------------------------------------------------------------------------------------------
def sort_col(rng, kind, n):
    nulls = rng.random(n) < 0.2
    if kind == "i64":
        return Col(L.I64, rng.choice(np.array([-2**63, 2**63 - 1, 0, -1, 1, 7], np.int64), n), nulls)
    if kind == "f64":
        return Col(L.F64, rng.choice([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 1e300], n), nulls)
    if kind == "str":
        return Col(L.U32CODE, rng.integers(0, len(STRINGS), n).astype(np.uint32), nulls, STRINGS)
    if kind == "bool":
        return Col(L.BOOLBITS, rng.random(n) < 0.5, nulls)
    if kind == "all_null":
        return Col(L.I64, rng.integers(-3, 3, n), np.ones(n, bool))
    if kind == "all_nan":
        return Col(L.F64, np.full(n, np.nan), rng.random(n) < 0.3)
    return Col(L.F64, rng.normal(0, 1, n))                       # no null mask at all, every value distinct


@pytest.mark.parametrize("kind", ["i64", "f64", "str", "bool", "all_null", "all_nan", "plain"])
@pytest.mark.parametrize("asc", [True, False])
def test_ref_lexsort_is_the_comparator_sort_one_key(kind, asc):
    rng = np.random.default_rng(len(kind) * 2 + int(asc))
    for n in (1, 2, 50, 300):
        col = sort_col(rng, kind, n)
        assert np.array_equal(ref_lexsort([col], [asc]), ref_cmp([col], [asc])), n


@pytest.mark.parametrize("n_keys", [2, 3, 4])
def test_ref_lexsort_is_the_comparator_sort_several_keys(n_keys):
    kinds = ["bool", "f64", "all_null", "str", "i64", "all_nan", "bool", "plain"]
    for seed in range(12):
        rng = np.random.default_rng(n_keys * 100 + seed)
        cols = [sort_col(rng, kinds[(seed + k) % len(kinds)], 250) for k in range(n_keys)]
        asc = [bool(rng.random() < 0.5) for _ in cols]
        assert np.array_equal(ref_lexsort(cols, asc), ref_cmp(cols, asc)), (seed, asc)


# ---- filter -------------------------------------------------------------------------------------------------------------
def test_filter_ref_is_the_row_loop():
    rng = np.random.default_rng(5)
    n = 500
    v, nulls = rng.random(n) < 0.5, rng.random(n) < 0.2
    rows = [i for i in range(n) if v[i] and not nulls[i]]
    assert filter_ref(v, nulls).tolist() == rows and filter_ref(v).tolist() == [i for i in range(n) if v[i]]
    src, sn = rng.normal(0, 1, n), rng.random(n) < 0.3
    src[::9] = np.nan
    got_rows, got = filter_ref(v, nulls, src, sn, np.float64(-0.0))
    want = np.array([np.float64(-0.0) if sn[i] else src[i] for i in rows])
    assert got_rows.tolist() == rows and got.tobytes() == want.tobytes()
    _, got = filter_ref(v, nulls, rng.random(n) < 0.5, None)
    assert got.dtype == np.uint8 and len(got) == len(rows)
    _, got = filter_ref(v, None, np.arange(n, dtype=np.uint32), sn, np.uint32(17))
    assert got.dtype == np.uint32 and got.tolist() == [17 if sn[i] else i for i in range(n) if v[i]]


# ---- the sweep's generator reaches what it means to reach ------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FUZZ_OPS_SLICES))
def test_fuzz_ops_dry_run_reaches_every_feature(kind):
    count, seed = FUZZ_OPS_SLICES[kind]
    env = dict(os.environ, FUZZ_DRY="1", FUZZ_KIND=kind)
    env.pop("FUZZ_FIRST", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", "fuzz_ops.py"), str(count), str(seed)], capture_output=True,
                       text=True, timeout=280, env=env, cwd=ROOT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-60:])
    assert r.returncode == 0, tail
    assert "fuzz_ops done: %d cases, 0 failures" % count in r.stdout
    lines = r.stdout[r.stdout.index("coverage ("):].splitlines()[1:-1]
    assert len(lines) >= 5 and all(line.startswith("  %s." % kind) for line in lines), tail
    assert all(int(line.split()[-1]) > 0 for line in lines), tail


# FUZZ_DRY=2: the generators and the twins alone - every reference result of a drawn case is computed, no engine call - so a
# generator that draws what its twin cannot take, or a chain stage whose reference breaks on the stage before, fails here.
NEW_KINDS = ("describe", "rank", "fill", "topk", "predicate", "wquant", "cum", "eval", "chain2")


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_fuzz_ops_references_take_every_draw(kind):
    assert kind in FUZZ_OPS_SLICES
    count, seed = FUZZ_OPS_SLICES[kind]
    count = count if kind == "chain2" else min(count, 40)
    env = dict(os.environ, FUZZ_DRY="2", FUZZ_KIND=kind)
    env.pop("FUZZ_FIRST", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "experiments", "fuzz_ops.py"), str(count), str(seed)], capture_output=True,
                       text=True, timeout=280, env=env, cwd=ROOT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-60:])
    assert r.returncode == 0, tail
    assert "fuzz_ops done: %d cases, 0 failures" % count in r.stdout and r.stdout.count("\nok ") + r.stdout.startswith("ok ") == count, tail
