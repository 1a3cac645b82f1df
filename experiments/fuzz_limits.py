"""Which refusals the randomised parity sweep (fuzz_parity.py) may skip: the engine's documented limits, decided from the DRAWN
inputs alone.  A refusal whose message names a limit that the inputs do not reach is a failure, not a skip — otherwise a
regression that refuses ordinary inputs with such a message would pass as "0 failures".  numpy only (tests/test_join_ref.py
checks the rules on a CPU-only box)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O
from oracle import oracle_np as ONP

ROW_LIMIT = (1 << 32) - 16384       # rows of a join side / of a join's output per call (join.hip)
P_MAX = 8192                        # widest radix fan-out whose cursors fit the scatter's LDS (engine.hpp)
SIGN = np.uint64(1 << 63)


def _bits(x):
    return max(int(x).bit_length(), 1)


def packed_key_bits(keys, n):
    """Bits of the packed multi-key cell at its narrowest: per column the smaller of its min..max span and its dictionary code
    (one code per distinct value), plus one code for null where the column has a mask (entries.hip, pack_multi_key)."""
    total = 0
    for col in keys:
        nul, cell = ONP.key_cells(col, n)
        live = cell[nul == 0]
        nullable = 1 if col[1] is not None else 0
        if len(live) == 0:
            total += 1
            continue
        if col[2] == O.I64:
            s = live ^ SIGN
        elif col[2] == O.F64:
            s = np.where((live >> np.uint64(63)).astype(bool), ~live, live | SIGN)
        else:
            s = live
        span = int(s.max()) - int(s.min())
        total += min(_bits(span + nullable), _bits(len(np.unique(live)) - 1 + nullable))
    return total


def join_output_rows(lkey, nl, rkey, nr, keep_left=True):
    """Rows the probe emits (matches, and misses when the join keeps them): the larger of the join types' probe outputs."""
    lnul, lcell = ONP.key_cells(lkey, nl)
    rnul, rcell = ONP.key_cells(rkey, nr)
    keys, runs = np.unique(rcell[rnul == 0], return_counts=True)
    live = lcell[lnul == 0]
    if len(keys) == 0:
        return len(live) if keep_left else 0
    pos = np.minimum(np.searchsorted(keys, live), len(keys) - 1)
    hit = keys[pos] == live
    return int(runs[pos][hit].astype(np.int64).sum()) + (int((~hit).sum()) if keep_left else 0)


def documented_limit(message, drawn):
    """True when `message` names a documented limit AND the drawn inputs reach it.  drawn: {"kind": "groupby", "keys", "n",
    "opts"} or {"kind": "join" | "fused", "lkey", "nl", "rkey", "nr", "opts"}."""
    kind, opts = drawn.get("kind"), drawn.get("opts", {})
    if "more than 64 bits" in message:
        return kind == "groupby" and len(drawn["keys"]) > 1 and packed_key_bits(drawn["keys"], drawn["n"]) > 64
    if "2^32-row" in message:
        if kind not in ("join", "fused"):
            return False
        nl, nr = drawn["nl"], drawn["nr"]
        if nl >= ROW_LIMIT or nr >= ROW_LIMIT:
            return True
        return join_output_rows(drawn["lkey"], nl, drawn["rkey"], nr, keep_left=kind == "join") + nr >= ROW_LIMIT
    if "does not fit" in message:
        return max(int(opts.get("partitions", 0)), int(opts.get("p_target", 0))) > P_MAX
    return False
