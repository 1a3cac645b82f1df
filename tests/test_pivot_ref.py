"""tests/pivot_ref.py against itself and against the reference (no GPU): the per-row dict loop over the oracle's fold rules and
the numpy twin agree on every op x key dtype x mask case the GPU test uses; both agree with a line-by-line restatement of
crosstab (src/dataframe/pandas_compat/functions.rs:2138-2183), PivotTable (src/pivot/mod.rs:107-228) and unstack
(functions.rs:2471-2522) on inputs where the documented deviations do not apply; the reference's own tests' assertions hold."""
import json
import math
import os

import numpy as np
import pytest

from tests import pivot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = list(R.grid_cases())


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a, np.float64).view(np.uint64) == np.ascontiguousarray(b, np.float64).view(np.uint64)).all()


def check_equal(got, want, op, what):
    for k in range(4):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got[5], want[5]), what
    assert np.array_equal(np.isnan(got[4]), np.isnan(want[4])), what
    if op in (R.SUM, R.MEAN):
        np.testing.assert_array_equal(got[4], want[4], err_msg=what)           # both fold in row order
    else:
        ok = ~np.isnan(want[4])
        assert same_bits(got[4][ok], want[4][ok]), what


@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_loop_and_twin_agree_on_the_grid(case):
    name, k1, k2, v, n, op, r1, r2 = case
    check_equal(R.pivot(k1, k2, n, op, v, r1, r2), R.pivot_loop(k1, k2, n, op, v, r1, r2), op, name)


def test_grid_reaches_what_it_names():
    names = [c[0] for c in GRID]
    assert len(names) == len(set(names)) == 7 * 5 * 2 * 2 - 5 * 2
    for op in R.OPS:
        for kind in R.KEY_KINDS:
            assert any(nm.startswith(R.OP_NAME[op] + "-" + kind + "-") for nm in names)
    masked = [c for c in GRID if "-masked-" in c[0]]
    # the masked half has null and NaN key cells, null value cells, NaN / inf / signed zero values
    assert any(c[1][1] is not None and c[1][2] == R.F64 and np.isnan(c[1][0]).any() for c in masked)
    assert any(c[3] is not None and c[3][2] == R.F64 and np.isnan(c[3][0]).any() and np.signbit(c[3][0][c[3][0] == 0]).any() for c in masked)


def test_contract_details():
    n = 8
    k1 = (np.array([3, 3, 1, 1, 3, 1, 2, 2], np.int64), None, R.I64)
    k2 = (np.array([1.0, math.nan, 1.0, 5.0, 1.0, 5.0, math.nan, 1.0]), np.packbits([0, 0, 0, 0, 0, 1, 0, 0], bitorder="little"), R.F64)
    v = (np.array([1.5, 2.0, -0.0, 0.0, math.nan, 7.0, math.inf, 9.0]), np.packbits([0, 0, 0, 0, 0, 0, 0, 1], bitorder="little"), R.F64)
    il, fi, cl, fc, cells, rows = R.pivot(k1, k2, n, R.ROWS)
    assert il.tolist() == [1, 2, 3] and fi.tolist() == [0, 0, 0]
    assert cl.view(np.float64)[:2].tolist() == [1.0, 5.0] and cl[2] == 0 and fc.tolist() == [0, 0, 1]       # NaN and null: ONE missing label
    assert rows.tolist() == [[1, 1, 2], [1, 0, 0], [1, 1, 1]] and rows.sum() == n
    assert math.isnan(cells[1, 1]) and cells[0, 2] == 2.0
    for op in R.OPS[1:]:
        check_equal(R.pivot(k1, k2, n, op, v), R.pivot_loop(k1, k2, n, op, v), op, op)
    count = R.pivot(k1, k2, n, R.COUNT, v)[4]
    assert count[0, 1] == 1.0 and count[0, 2] == 2.0                          # Count: the rows, null and NaN value cells included
    mean = R.pivot(k1, k2, n, R.MEAN, v)[4]
    assert mean[0, 1] == 0.0 and math.isnan(mean[0, 2])                       # no counted cell: 0.0; a NaN cell: NaN
    mn, mx = R.pivot(k1, k2, n, R.MIN, v)[4], R.pivot(k1, k2, n, R.MAX, v)[4]
    assert mn[0, 2] == 1.5 and mx[0, 2] == 1.5                                # the NaN cell is skipped
    assert mx[2, 1] == math.inf and mn[2, 1] == 0.0                           # +inf alone: the sentinel rule answers 0.0 for Min
    last = R.pivot(k1, k2, n, R.LAST, v)[4]
    assert last[0, 1] == 0.0 and math.isnan(last[0, 2]) and last[1, 0] == 0.0 and math.copysign(1.0, last[1, 0]) == 1.0
    # -0.0 < 0.0 in Min / Max
    z = (np.array([0.0, -0.0, 0.0, -0.0]), None, R.F64)
    one = (np.zeros(4, np.int64), None, R.I64)
    assert math.copysign(1.0, R.pivot(one, one, 4, R.MIN, z)[4][0, 0]) == -1.0 and math.copysign(1.0, R.pivot(one, one, 4, R.MAX, z)[4][0, 0]) == 1.0
    # the bound: zero for everything exact
    assert (R.bound(k1, k2, n, R.MIN, v) == 0).all() and (R.bound(one, one, 4, R.SUM, (np.arange(4), None, R.I64)) == 0).all()
    b = R.bound(one, one, 4, R.SUM, (np.array([1.0, -2.0, 3.0, 4.0]), None, R.F64))
    assert b.shape == (1, 1) and 0 < b[0, 0] < 1e-13 and b[0, 0] == 2 * (4 * R.U / (1 - 4 * R.U)) * 10.0
    # spans: the direct path's table
    assert R.spans(k1, k2, n) == (3 + 1) * (5 + 1) and R.spans(k1, (np.array([0.5] * 8), None, R.F64), n) is None
    assert R.spans((np.array([-2 ** 63, 2 ** 63 - 1] * 4, np.int64), None, R.I64), k1, n) is None        # (no table of 2^64 cells)
    assert R.spans((np.array([-2 ** 63, -2 ** 63 + 3] * 4, np.int64), None, R.I64), k1, n) == (4 + 1) * (3 + 1)
    assert R.spans((np.array([2 ** 63 - 4, 2 ** 63 - 1] * 4, np.int64), None, R.I64), k1, n) == (4 + 1) * (3 + 1)
    # n_rows == 0
    e = R.pivot((np.empty(0, np.int64), None, R.I64), (np.empty(0, np.int64), None, R.I64), 0, R.ROWS)
    assert e[0].shape == (0,) and e[4].shape == (0, 0)


def _coded(strings):
    pool = sorted(set(strings), key=lambda s: (len(s), s))                 # (codes in an order that is NOT the byte-wise one)
    code = {s: i for i, s in enumerate(pool)}
    order = sorted(range(len(pool)), key=lambda i: pool[i].encode())
    rank = np.empty(len(pool), np.uint32)
    rank[order] = np.arange(len(pool), dtype=np.uint32)
    return (np.array([code[s] for s in strings], np.uint32), None, R.U32CODE), rank, pool


def test_twin_against_the_reference_restated():
    rng = np.random.default_rng(3)
    words1 = ["b", "a", "zz", "Z", "", "ab", "é"]
    words2 = ["x", "Y", "yy", "10", "9"]
    for n in (1, 5, 64, 400):
        s1 = [words1[i] for i in rng.integers(0, len(words1), n)]
        s2 = [words2[i] for i in rng.integers(0, len(words2), n)]
        vals = (rng.integers(1, 2000, n) / 8.0).tolist()                      # no NaN, no inf, no zero: the deviations do not apply
        k1, r1, p1 = _coded(s1)
        k2, r2, p2 = _coded(s2)
        v = (np.array(vals), None, R.F64)
        u1, u2, table = R.crosstab_loop(s1, s2)
        il, fi, cl, fc, cells, rows = R.pivot(k1, k2, n, R.ROWS, None, r1, r2)
        assert [p1[c] for c in il.tolist()] == u1 and [p2[c] for c in cl.tolist()] == u2 and not fi.any() and not fc.any()
        for j, u in enumerate(u2):
            assert rows[j].tolist() == [int(x) for x in table[u]] and np.nan_to_num(cells[j]).tolist() == table[u]
        for name, op in (("sum", R.SUM), ("mean", R.MEAN), ("min", R.MIN), ("max", R.MAX), ("count", R.COUNT)):
            ilab, clab, want = R.pivot_table_loop(s1, s2, vals, name)
            got = R.pivot(k1, k2, n, op, v, r1, r2)
            assert ilab == u1 and clab == u2
            for j, u in enumerate(clab):
                assert [None if math.isnan(x) else x for x in got[4][j].tolist()] == want[u], (name, n)
        ui, uc, want = R.unstack_loop(s1, s2, vals)
        got = R.pivot(k1, k2, n, R.LAST, v, r1, r2)[4]
        for j, u in enumerate(uc):
            np.testing.assert_array_equal(got[j], np.array(want[u]))


def test_reference_known_answers():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pivot_known_answers.json")))
    assert {c["fn"] for c in golden["cases"]} == {"crosstab", "unstack", "pivot"}
    for case in golden["cases"]:
        assert case["at"].startswith("functions.rs:")
        if case["fn"] == "crosstab":
            u1, u2, table = R.crosstab_loop(case["index"], case["columns"])
            columns = [case["index_name"]] + u2
            if case["test"] == "test_crosstab":
                assert table == {"A": [1.0, 2.0], "B": [1.0, 1.0]} and u1 == ["F", "M"]
        else:
            u1, u2, table = R.unstack_loop(case["index"], case["columns"], case["values"])
            columns = [case["index_name"]] + u2
        for name in case["expect"]["contains_columns"]:
            assert name in columns
        if "row_count" in case["expect"]:
            assert len(u1) == case["expect"]["row_count"]
