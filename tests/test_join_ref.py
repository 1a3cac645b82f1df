"""CPU checks of the join's edge-case generator (tests/join_ref.py): the plain dictionary loop agrees with the oracle on every
small case, every structural edge listed in FEATURES is reached by some case, and the constants are still found in the kernels."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import join_ref as J

SMALL = 5000


@pytest.fixture(scope="module")
def cases():
    return list(J.edge_cases())


def test_constants_are_positive_integers():
    K = J.join_constants()
    for name in ("JN_RCAP", "BH_SLOTS", "BH_MAXRUN", "LK_THREADS", "LK_RPT", "OP_TILE", "FJ_SLOTS", "FJ_MAXROWS", "SCAN_SEG", "TILE",
                 "BH_MAXROWS", "SCAN_TILES"):
        assert isinstance(K[name], int) and K[name] > 0, name
    assert K["BH_MAXROWS"] < K["BH_SLOTS"] and K["BH_MAXRUN"] < K["BH_MAXROWS"] and K["BH_MAXROWS"] < K["GENERAL_ROWS"] <= K["JN_RCAP"]


def test_a_missing_constant_is_named():
    with pytest.raises(KeyError, match="NO_SUCH_CONSTANT"):
        J._evaluate("NO_SUCH_CONSTANT", J._constexprs("constexpr int A = 2, B = A * 3;"))
    assert J._evaluate("B", J._constexprs("constexpr int A = 2, B = A * 3;\nconstexpr uint32_t C = B * 7 / 8;")) == 6
    assert J._evaluate("C", J._constexprs("constexpr int A = 2, B = A * 3;\nconstexpr uint32_t C = B * 7 / 8u;")) == 5


def test_case_names_are_unique_and_inputs_consistent(cases):
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names))
    for c in cases:
        assert set(c) >= {"name", "lkey", "nl", "rkey", "nr", "options", "features"}
        for (data, mask, dt), n in ((c["lkey"], c["nl"]), (c["rkey"], c["nr"])):
            rows = len(data) * 8 if dt == O.BOOLBITS else len(data)
            assert rows >= n and (mask is None or len(mask) * 8 >= n), c["name"]


def test_every_feature_is_reached_and_every_case_reaches_its_own(cases):
    reached = set()
    for c in cases:
        f = J.join_features(c)
        assert c["features"] <= f, (c["name"], sorted(c["features"] - f))
        reached |= f
    assert reached == set(J.FEATURES), (sorted(set(J.FEATURES) - reached), sorted(reached - set(J.FEATURES)))


def test_loop_equals_oracle_on_every_small_case(cases):
    small = [c for c in cases if c["nl"] <= SMALL and c["nr"] <= SMALL]
    assert len(small) > len(cases) // 2
    seen = set()
    for c in small:
        key = (c["name"].replace("_onepass", "").replace("_threekernel", ""))      # the probe option does not change the inputs
        if key in seen:
            continue
        seen.add(key)
        for how in (O.INNER, O.LEFT, O.RIGHT, O.OUTER):
            wl, wr = O.join_indices(c["lkey"], c["nl"], c["rkey"], c["nr"], how)
            gl, gr = J.join_loop(c["lkey"], c["nl"], c["rkey"], c["nr"], how)
            np.testing.assert_array_equal(gl, wl, err_msg="%s how=%d" % (c["name"], how))
            np.testing.assert_array_equal(gr, wr, err_msg="%s how=%d" % (c["name"], how))


def test_fuzz_skip_rule_decides_from_the_drawn_inputs():
    """experiments/fuzz_limits.py: the sweep may skip a refusal only where the drawn inputs reach the documented limit that the
    message names; the same message on ordinary inputs is a failure."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_limits", os.path.join(J.ROOT, "experiments", "fuzz_limits.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    rng = np.random.default_rng(3)
    wide = (rng.integers(-2 ** 62, 2 ** 62, 100_000).astype(np.int64), None, O.I64)
    narrow = (rng.integers(0, 5, 100_000).astype(np.uint32), O.pack_mask(rng.random(100_000) < 0.05), O.U32CODE)
    two = {"kind": "groupby", "keys": [wide, narrow], "n": 100_000, "opts": {}}
    assert F.packed_key_bits([wide, narrow], 100_000) == 17 + 3                 # 100 000 distinct ids -> 17-bit codes; 0..4 + null -> 3 bits
    assert not F.documented_limit("the key columns need more than 64 bits even with ...", two)
    four = dict(two, keys=[wide, wide, wide, wide])
    assert F.packed_key_bits(four["keys"], 100_000) == 68 and F.documented_limit("... more than 64 bits ...", four)
    lk, rk = (np.zeros(300, np.int64), None, O.I64), (np.zeros(20, np.int64), None, O.I64)
    join = {"kind": "join", "lkey": lk, "nl": 300, "rkey": rk, "nr": 20, "opts": {}}
    assert F.join_output_rows(lk, 300, rk, 20) == 6000
    assert F.join_output_rows((np.arange(5, dtype=np.int64), None, O.I64), 5, (np.array([1, 1, 9], np.int64), None, O.I64), 3) == 2 + 4
    assert not F.documented_limit("join: the output exceeds the 2^32-row per-call limit", join)
    assert F.documented_limit("join: a side exceeds the 2^32-row per-call limit", dict(join, nl=F.ROW_LIMIT))
    assert not F.documented_limit("radix fan-out 3072 does not fit the scatter's LDS", dict(two, opts={"p_target": 3072}))
    assert F.documented_limit("radix fan-out 9000 does not fit the scatter's LDS", dict(two, opts={"p_target": F.P_MAX + 1}))
    assert not F.documented_limit("some other refusal", two) and not F.documented_limit("does not fit", {})
    assert F.P_MAX == J.join_constants()["P_MAX"]
