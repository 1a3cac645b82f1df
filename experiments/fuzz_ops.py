#!/usr/bin/env python3
"""Randomised parity sweep for pandrs_hip_sort_indices, pandrs_hip_filter_indices / pandrs_hip_filter_gather,
pandrs_hip_window and chains of them with every intermediate left on the device, against the restatements the GPU tests
trust (tests/sort_ref.py, tests/window_ref.py, tests/helpers.filter_ref) and the CPU oracle; and, in fuzz_columns.py and
fuzz_chain2.py, for the column ops (describe / quantiles, rank, fill, topk / arg_extreme, predicate / isin, window_quantile,
cumulative / lag, eval) and the chains across them, against the twins under tests/*_ref.py.  GPU box only, except FUZZ_DRY:
1 draws and classifies every case with no engine call (the coverage condition, checked by tests/test_references.py), 2 also
computes every reference result of the newer kinds (a generator its twin cannot follow fails without a GPU; row counts capped).

usage: fuzz_ops.py [n_cases] [seed]      case i seeds default_rng(seed * 100003 + i)
  FUZZ_KIND=sort|filter|window|chain     restrict the draw to one kind; also describe|rank|fill|topk|predicate|wquant|cum|eval|chain2
  FUZZ_FIRST=i                           replay: FUZZ_FIRST=17 fuzz_ops.py 18 6001 runs case 17 alone
  FUZZ_DRY=1                             no engine: the generator and the coverage summary alone (2: and the references)
  FUZZ_POISON=0xA5                       set_option("poison_workspace"): the library's scratch starts every call as that byte

Sort cases are layout-directed: the structured part of a case (which key layout) is case mod the number of recipes, so a
run of a few dozen cases reaches every digit width, word count and packing edge; everything else is drawn.  The pass count
of every sort (timings n_partitions) must equal the count derived here from the codes this file encodes itself, by the rule
the header documents.  A whole 64-bit word of the packed key cannot be constant (every code's top bit varies and no code
has 64 constant bits below it), so the nearest reachable layouts are drawn instead: 62 constant bits in a word's middle,
and a middle word that takes one 1-bit pass.  The last lines are the coverage summary: one line per feature the sweep
means to reach, with the number of cases that reached it; a zero there, like a mismatch, is exit status 1."""
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_common import DRY, DRY_MODE, DT_NAME, SPACES, L, Mismatch, bits, check, cov, first_diff_any, np, place, to_np  # noqa: E402,F401
from tests import window_ref as WR  # noqa: E402
from tests.helpers import filter_ref  # noqa: E402
from tests.sort_ref import STRINGS, Col, rank_of, ref_cmp, ref_lexsort  # noqa: E402
import fuzz_chain2  # noqa: E402
import fuzz_columns  # noqa: E402

OLD_KINDS = ("sort", "filter", "window", "chain")
OPS = {"sum": L.WINDOW_SUM, "mean": L.WINDOW_MEAN, "var": L.WINDOW_VAR, "std": L.WINDOW_STD, "min": L.WINDOW_MIN,
       "max": L.WINDOW_MAX, "count": L.WINDOW_COUNT}
WKINDS = {"rolling": L.WINDOW_KIND_ROLLING, "expanding": L.WINDOW_KIND_EXPANDING, "ewm": L.WINDOW_KIND_EWM}
CHAINS = ("filter_sort_window", "filter_groupby", "sort_clustered_groupby", "sort_window")
SIGN = np.uint64(1 << 63)


# ---- sort: key makers ---------------------------------------------------------------------------------------------------
B_CHOICES = [1, 2, 7, 8, 9, 13, 16, 17, 31, 32, 33, 47, 63, 64]


def from_sortable(u):
    """int64 values whose order-preserving unsigned image is u."""
    return (u ^ SIGN).view(np.int64)


def k_bits(rng, n, b, s=0, fields=None):
    """i64: base + (random b-bit value << s); both ends of the b-bit range are present, so the code is b + s bits wide with
    its low s bits constant.  fields = (b1, gap, b2): two varying fields with `gap` constant bits between them."""
    if b >= 64:
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
        if n >= 2 and rng.random() < 0.5:                       # width 64 whatever the draw
            v[rng.integers(0, n)] = -2**63 + 1
            v[rng.integers(0, n)] = 2**63 - 2
        return Col(L.I64, v)
    if fields:
        b1, gap, b2 = fields
        r = rng.integers(0, 1 << b1, n, dtype=np.uint64) | (rng.integers(0, 1 << b2, n, dtype=np.uint64) << np.uint64(b1 + gap))
        b, full = b1 + gap + b2, ((1 << b1) - 1) | (((1 << b2) - 1) << (b1 + gap))
    else:
        r = rng.integers(0, 1 << b, n, dtype=np.uint64)
        full = (1 << b) - 1
    if n >= 2:
        i0 = int(rng.integers(0, n))
        r[i0], r[(i0 + 1 + int(rng.integers(0, n - 1))) % n] = 0, full
    s = min(s, 63 - b)
    base = rng.integers(0, 2**64 - (1 << (b + s)), dtype=np.uint64)
    return Col(L.I64, from_sortable(base + (r << np.uint64(s))))


def k_top_bit(rng, n, low_bits=0):
    """i64 of width 64 whose code varies in bit 63 (and in its low `low_bits` bits) only."""
    r = rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    if low_bits:
        r |= rng.integers(0, 1 << low_bits, n, dtype=np.uint64)
    if n >= 2:
        r[0], r[n - 1] = 0, (1 << 63) | ((1 << low_bits) - 1)
    return Col(L.I64, from_sortable(r))


def k_f64(rng, n, b, s):
    """f64: one sign and exponent, b mantissa bits from bit s varying; sometimes the specials on top."""
    b = min(b, 52)
    s = min(s, 52 - b)
    r = rng.integers(0, 1 << b, n, dtype=np.uint64) << np.uint64(s)
    v = ((np.uint64(int(rng.integers(1, 2046))) << np.uint64(52)) | r | (SIGN if rng.random() < 0.5 else np.uint64(0))).view(np.float64)
    if rng.random() < 0.4 and n >= 8:
        k = rng.choice(n, size=max(3, n // 50), replace=False)
        v[k] = rng.choice([np.nan, -0.0, 0.0, np.inf, -np.inf], size=len(k))
    return Col(L.F64, v)


def k_str(rng, n, strings):
    return Col(L.U32CODE, rng.integers(0, len(strings), n).astype(np.uint32), None, strings)


def k_bool(rng, n):
    return Col(L.BOOLBITS, rng.random(n) < rng.choice([0.5, 0.01]))


def k_minmax65(rng, n):
    """INT64_MIN and INT64_MAX together plus a null: a 65-bit code."""
    pool = np.array([-2**63, 2**63 - 1, 0, -1, int(rng.integers(-2**62, 2**62))], np.int64)
    v = pool[rng.integers(0, len(pool), n)]
    nulls = rng.random(n) < 0.1
    if n >= 3:
        p = rng.permutation(n)[:3]
        v[p[0]], v[p[1]], nulls[p[2]] = -2**63, 2**63 - 1, True
        nulls[p[0]] = nulls[p[1]] = False
    return Col(L.I64, v, nulls)


def with_nulls(rng, col, p):
    if p <= 0 or col.nulls is not None:
        return col
    return Col(col.dtype, col.values, rng.random(col.n) < p, col.strings)


def k_special(rng, n, which, strings):
    dtype = int(rng.choice([L.I64, L.F64, L.U32CODE, L.BOOLBITS]))
    base = {L.I64: lambda: k_bits(rng, n, 13), L.F64: lambda: k_f64(rng, n, 9, 3), L.U32CODE: lambda: k_str(rng, n, strings),
            L.BOOLBITS: lambda: k_bool(rng, n)}[dtype]()
    if which == "all_null":
        return Col(dtype, base.values, np.ones(n, bool), base.strings)
    if which == "all_nan":
        return Col(L.F64, np.full(n, np.nan), (rng.random(n) < 0.2) if rng.random() < 0.5 else None)
    if which == "all_equal":
        return Col(dtype, np.repeat(base.values[:1], n), None, base.strings)
    nulls = np.ones(n, bool)                                    # one non-null row
    nulls[rng.integers(0, n)] = False
    return Col(dtype, base.values, nulls, base.strings)


def make_strings(rng, size):
    if size == len(STRINGS):
        return STRINGS
    words = ["%s%x" % ("é" if i % 7 == 0 else "k", (i * 2654435761) % (1 << 32)) for i in range(size)]
    return [words[i] for i in rng.permutation(size)]


N_RECIPES = 14


def sort_keys(rng, n, recipe, strings, turn):
    """-> key columns.  Recipes 1-4 and 8-10 take no nulls: their widths are the point.  `turn` (how often the recipe has
    come round) cycles through a recipe's variants."""
    rb = lambda: int(rng.choice(B_CHOICES))
    rs = lambda: int(rng.choice([0, 0, 1, 5, 12, 30]))
    def any_key():
        r = rng.random()
        if r < 0.45: return k_bits(rng, n, rb(), rs())
        if r < 0.65: return k_f64(rng, n, int(rng.choice([1, 7, 9, 13, 31, 47, 52])), rs())
        if r < 0.85: return k_str(rng, n, strings)
        return k_bool(rng, n)
    nul = lambda c: with_nulls(rng, c, float(rng.choice([0, 0, 0.01, 0.3])))
    if recipe == 0:
        return [nul(k_bits(rng, n, rb(), rs()))]
    if recipe == 1:                                             # 64 bits in all
        split = [[31, 33], [64], [16, 47, 1], [32, 32], [63, 1], [7, 8, 9, 13, 17, 2, 8]][turn % 6]
        return [k_bits(rng, n, b) for b in split]
    if recipe == 2:                                             # 65 bits
        if turn % 2 == 0:
            return [k_minmax65(rng, n)]
        return [k_bits(rng, n, b) for b in [[32, 33], [64, 1], [1, 64], [2, 63]][turn // 2 % 4]]
    if recipe == 3:                                             # 127 to 129 bits
        pick = turn % 5
        if pick == 4:
            return [k_bits(rng, n, 64), k_minmax65(rng, n)]
        return [k_bits(rng, n, b) for b in [[63, 64], [64, 64], [1, 63, 64], [33, 31, 64]][pick]]
    if recipe == 4:                                             # more than 192 bits
        cols = [k_bits(rng, n, b) for b in [[64, 47, 64, 33], [64, 64, 64, 13], [63, 64, 9, 64, 2], [64, 64, 64, 64]][turn % 4]]
        if rng.random() < 0.5:
            cols.insert(int(rng.integers(0, len(cols))), k_minmax65(rng, n))
        return cols
    if recipe == 5:                                             # several narrow keys of every dtype
        return [nul(any_key() if rng.random() < 0.5 else k_bits(rng, n, int(rng.choice([1, 2, 7])), 0)) for _ in range(int(rng.integers(2, 9)))]
    if recipe == 6:                                             # the degenerate columns
        which = ["all_null", "all_nan", "all_equal", "one_row"][turn % 4]
        cols = [k_special(rng, n, which, strings)]
        if rng.random() < 0.5:
            cols.insert(int(rng.integers(0, 2)), nul(any_key()))
        if rng.random() < 0.3:
            cols.append(k_special(rng, n, str(rng.choice(["all_null", "all_nan", "all_equal"])), strings))
        return cols
    if recipe == 7:                                             # two fields, a run of constant bits between them
        b1, b2 = int(rng.choice([3, 8, 9])), int(rng.choice([1, 7, 9]))
        cols = [k_bits(rng, n, 0, rs(), fields=(b1, int(rng.choice([16, 24, 40])), b2))]
        if rng.random() < 0.5:
            cols.insert(int(rng.integers(0, 2)), nul(any_key()))
        return cols
    if recipe == 8:                                             # low word one pass, the next word three or more
        return [k_bits(rng, n, int(rng.choice([17, 20, 24, 31]))), k_top_bit(rng, n)]
    if recipe == 9:                                             # low word three or more passes, the next word one
        return [k_bool(rng, n) if rng.random() < 0.5 else k_bits(rng, n, int(rng.choice([1, 2, 7]))), k_top_bit(rng, n, int(rng.choice([17, 20])))]
    if recipe == 10:                                            # a middle word with a single one-bit pass
        return [k_bits(rng, n, rb()), k_top_bit(rng, n), k_bits(rng, n, 64)]
    if recipe == 11:                                            # string codes
        cols = [nul(k_str(rng, n, strings))]
        if rng.random() < 0.6:
            cols.append(nul(any_key()))
        return cols
    if recipe == 12:                                            # f64 mantissa fields
        cols = [nul(k_f64(rng, n, int(rng.choice([1, 2, 7, 8, 9, 13, 17, 33, 52])), rs()))]
        if rng.random() < 0.4:
            cols.append(nul(any_key()))
        return cols
    return [nul(any_key()) for _ in range(int(rng.integers(1, 9)))]


# ---- sort: the packed key and the pass count, derived here ---------------------------------------------------------------
def sortable(col):
    v = col.values
    if col.dtype == L.I64:
        return v.view(np.uint64) ^ SIGN
    if col.dtype == L.F64:
        b = v.view(np.uint64).copy()
        b[b == SIGN] = 0
        return np.where(b >> np.uint64(63) == 1, ~b, b | SIGN)
    if col.dtype == L.U32CODE:
        return rank_of(col.strings)[v].astype(np.uint64)
    return v.astype(np.uint64)


def sort_plan(cols, asc, max_digit):
    """The header's rule (pandrs_hip_sort_indices): per key a code of bitlength(span + has_nan + has_null) bits, value code
    = sortable - min ascending / max - sortable descending, NaN = span + 1, null = span + 1 + has_nan; the codes packed
    MSB-first with the last key at bit 0; per 64-bit word the bits from the lowest to the highest varying one are cut
    into ceil(bits / max_digit) digits of ceil(bits / digits) bits, and a digit takes a pass iff one of its bits varies."""
    n = cols[0].n
    info = {"widths": [], "straddle": False, "code65": False}
    parts = []
    for col, a in zip(cols, asc):
        s = sortable(col)
        null = col.nulls if col.nulls is not None else np.zeros(n, bool)
        nan = (np.isnan(col.values) if col.dtype == L.F64 else np.zeros(n, bool)) & ~null
        num = ~null & ~nan
        mn, mx = (int(s[num].min()), int(s[num].max())) if num.any() else (0, 0)
        span, has_nan, has_null = mx - mn, int(nan.any()), int(null.any())
        width = (span + has_nan + has_null).bit_length()
        lo = (s - np.uint64(mn)) if a else (np.uint64(mx) - s)
        hi = np.zeros(n, bool)
        for sel, code in ((nan, span + 1), (null, span + 1 + has_nan)):
            lo = np.where(sel, np.uint64(code & (2**64 - 1)), lo)
            hi |= sel & bool(code >> 64)
        parts.append((width, lo, hi))
        info["widths"].append(width)
        info["code65"] |= width == 65
    total = sum(info["widths"])
    W = (total + 63) // 64
    words = np.zeros((W, n), np.uint64)
    off = 0
    for width, lo, hi in reversed(parts):
        if width == 0:
            continue
        j0, sh = off >> 6, off & 63
        words[j0] |= lo << np.uint64(sh)
        if sh and j0 + 1 < W:
            words[j0 + 1] |= lo >> np.uint64(64 - sh)
        if width == 65:
            words[(off + 64) >> 6] |= hi.astype(np.uint64) << np.uint64((off + 64) & 63)
        info["straddle"] |= j0 != (off + width - 1) >> 6
        off += width
    digits, skipped, per_word, lo_above_0 = [], 0, [], False
    for j in range(W):
        vary = int(np.bitwise_and.reduce(words[j]) ^ np.bitwise_or.reduce(words[j]))
        if not vary:
            per_word.append(0)
            continue
        lo, hi = (vary & -vary).bit_length() - 1, vary.bit_length() - 1
        nbits = hi - lo + 1
        nd = -(-nbits // max_digit)
        db = -(-nbits // nd)
        took = 0
        for q in range(nd):
            sh = lo + q * db
            w = min(db, hi + 1 - sh)
            if vary & (((1 << w) - 1) << sh):
                digits.append((j, sh, w))
                took += 1
            else:
                skipped += 1
        per_word.append(took)
        lo_above_0 |= lo > 0
    info.update(total=total, W=W, digits=digits, skipped=skipped, per_word=per_word, lo_above_0=lo_above_0)
    return info


SORT_N = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6145, 10_000, 20_000, 65_537, 300_007, 1_000_003,
          2_097_151, 2_097_152, 2_097_153, 4_194_305]        # 1024 workgroups x 2048-row tiles: rows_per_block steps at 2 097 152
SORT_N_P = np.array([1, 1, 1, 2, 2, 2, 4, 4, 4, 4, 4, 4, 3, 3, 3, 3, 4, 3, 2, 1, 1, 1, 1], float)


def draw_sort(rng, case):
    recipe = case % N_RECIPES
    n = int(rng.choice(SORT_N, p=SORT_N_P / SORT_N_P.sum()))
    if recipe in (6,) and rng.random() < 0.25:
        n = 1
    if recipe in (1, 2, 3, 4, 7, 8, 9, 10):                   # layouts need rows to show
        n = max(n, 2047)
    strings = make_strings(rng, int(rng.choice([2, len(STRINGS), 300, 70_000])))
    cols = sort_keys(rng, n, recipe, strings, case // N_RECIPES)
    if n > 1_100_000:
        cols = cols[:3]
    asc = [bool(rng.random() < 0.5) for _ in cols]
    digit_bits = int(rng.choice([0, 4, 5, 6, 7, 8]))
    space = str(rng.choice(SPACES))
    info = sort_plan(cols, asc, digit_bits or 8)
    return dict(n=n, recipe=recipe, cols=cols, asc=asc, digit_bits=digit_bits, space=space, strings=strings, info=info)


def classify_sort(d):
    info = d["info"]
    f = ["sort.dtype=%s" % DT_NAME[c.dtype] for c in d["cols"]]
    f += ["sort.digit_width=%d" % w for _, _, w in info["digits"]]
    f.append("sort.words=%s" % (">=4" if info["W"] >= 4 else info["W"]) if info["W"] else "sort.all_keys_constant")
    t = info["total"]
    f.append("sort.total_bits " + ("<64" if t < 64 else "=64" if t == 64 else "=65" if t == 65 else "127..129" if 127 <= t <= 129
                                   else ">192" if t > 192 else "other"))
    f.append("sort.digit_bits_option=%d" % d["digit_bits"])
    f.append("sort.keys=%s" % (len(d["cols"]) if len(d["cols"]) < 5 else ">=5"))
    f.append("sort.space=%s" % d["space"])
    pw = info["per_word"]
    for cond, name in ((info["skipped"], "sort.skipped_constant_digit"), (info["code65"], "sort.code_of_65_bits"),
                       (info["straddle"], "sort.code_straddles_a_word"), (info["lo_above_0"], "sort.varying_bits_start_above_bit_0"),
                       (any(c.nulls is not None and c.nulls.all() for c in d["cols"]), "sort.all_null_key"),
                       (any(c.dtype == L.F64 and np.isnan(c.values).all() for c in d["cols"]), "sort.all_nan_key"),
                       (d["n"] == 1, "sort.one_row"),
                       (any(pw[j] == 1 and pw[j + 1] >= 3 for j in range(len(pw) - 1)), "sort.passes_per_word 1 then >=3"),
                       (any(pw[j] >= 3 and pw[j + 1] == 1 for j in range(len(pw) - 1)), "sort.passes_per_word >=3 then 1"),
                       (any(pw[j] == 1 for j in range(1, len(pw) - 1)), "sort.middle_word_one_pass"),
                       (any(p % 2 == 0 and p for p in pw[1:]), "sort.upper_word_even_passes"),
                       (any(p % 2 == 1 and p >= 3 for p in pw[1:]), "sort.upper_word_odd_passes")):
        if cond:
            f.append(name)
    return f


SORT_FEATURES = (["sort.dtype=%s" % v for v in DT_NAME.values()] + ["sort.digit_width=%d" % w for w in range(1, 9)] +
                 ["sort.words=%s" % w for w in (1, 2, 3, ">=4")] + ["sort.all_keys_constant"] +
                 ["sort.total_bits " + t for t in ("<64", "=64", "=65", "127..129", ">192")] +
                 ["sort.digit_bits_option=%d" % b for b in (0, 4, 5, 6, 7, 8)] + ["sort.keys=%s" % k for k in (1, 2, 3, 4, ">=5")] +
                 ["sort.space=%s" % s for s in SPACES] +
                 ["sort.skipped_constant_digit", "sort.code_of_65_bits", "sort.code_straddles_a_word", "sort.varying_bits_start_above_bit_0",
                  "sort.all_null_key", "sort.all_nan_key", "sort.one_row", "sort.passes_per_word 1 then >=3",
                  "sort.passes_per_word >=3 then 1", "sort.middle_word_one_pass", "sort.upper_word_even_passes", "sort.upper_word_odd_passes"])


def run_sort(ctx, d):
    cols, asc, n = d["cols"], d["asc"], d["n"]
    want = ref_lexsort(cols, asc)
    if n <= 20_000:
        alt = ref_cmp(cols, asc)
        check(np.array_equal(want, alt), "ref_lexsort != ref_cmp", first_diff_any(want, alt))
    keep = []
    placed = [place(ctx, d["space"], c.data, c.mask, c.dtype, n, keep) for c in cols]
    rank = rank_of(d["strings"]) if any(c.dtype == L.U32CODE for c in cols) else None
    ctx.set_option("sort_digit_bits", d["digit_bits"])
    try:
        got = ctx.sort_indices(placed, n, None if all(asc) and d["recipe"] % 2 == 0 else asc, rank).cpu().numpy()
        passes = ctx.timings()["n_partitions"]
    finally:
        ctx.set_option("sort_digit_bits", 0)
        for r in keep:
            if hasattr(r, "release"):
                r.release()
    check(np.array_equal(got, want), "permutation", first_diff_any(got, want))
    check(passes == len(d["info"]["digits"]), "pass count", (passes, len(d["info"]["digits"]), d["info"]["digits"]))


def desc_sort(d):
    i = d["info"]
    return "sort n=%d recipe=%d keys=%s asc=%s widths=%s total=%d W=%d digit_bits=%d passes=%d per_word=%s skipped=%d space=%s" % (
        d["n"], d["recipe"], [DT_NAME[c.dtype] + ("?" if c.nulls is not None else "") for c in d["cols"]], [int(a) for a in d["asc"]],
        i["widths"], i["total"], i["W"], d["digit_bits"], len(i["digits"]), i["per_word"], i["skipped"], d["space"])


# ---- filter ------------------------------------------------------------------------------------------------------------------
FILTER_N = [1, 2, 7, 8, 9, 63, 64, 65, 127, 4095, 4096, 4097, 8191, 8193, 12_289, 65_537, 262_145, 1_000_003, 3_000_001]
SELECT = ("none", "one_row", "1e-4", "half", "all_but_1e-4", "all")


def draw_cond(rng, n, select, runs):
    if select == "none":
        v = np.zeros(n, bool)
    elif select == "all":
        v = np.ones(n, bool)
    elif select == "one_row":
        v = np.zeros(n, bool)
        v[rng.integers(0, n)] = True
    else:
        p = {"1e-4": 1e-4, "half": 0.5, "all_but_1e-4": 1 - 1e-4}[select]
        if runs:                                               # long runs: whole 4096-row tiles empty or full
            run = int(rng.choice([64, 4096, 10_000]))
            v = np.repeat(rng.random((n + run - 1) // run) < 0.5, run)[:n]
            v ^= rng.random(n) < min(p, 1 - p) * 0.01
        else:
            v = rng.random(n) < p
    return v


def src_col(rng, dtype, n, null_p):
    nulls = rng.random(n) < null_p if null_p else None
    if dtype == L.I64:
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    elif dtype == L.F64:
        v = rng.normal(0, 1e6, n)
        v[rng.random(n) < 0.05] = rng.choice([np.nan, -0.0, np.inf])
    elif dtype == L.U32CODE:
        v = rng.integers(0, 2**32 - 1, n, dtype=np.uint32, endpoint=True)
    else:
        v = rng.random(n) < 0.5
    return v, nulls


def draw_filter(rng, case):
    n = int(rng.choice(FILTER_N))
    select = SELECT[(case // 2) % len(SELECT)] if rng.random() < 0.7 else str(rng.choice(SELECT))
    runs = bool(rng.random() < 0.4)
    v = draw_cond(rng, n, select, runs)
    cnull = rng.random(n) < rng.choice([0.01, 0.3]) if rng.random() < 0.5 else None
    gathers = []
    for _ in range(int(rng.integers(1, 5))):
        dtype = int(rng.choice([L.I64, L.F64, L.U32CODE, L.BOOLBITS]))
        sv, sn = src_col(rng, dtype, n, float(rng.choice([0, 0.2, 1.0])) if rng.random() < 0.6 else 0)
        fill = {L.I64: int(rng.integers(-2**63, 2**63 - 1)), L.F64: float(rng.choice([0.0, -0.0, 1.5, np.nan])),
                L.U32CODE: int(rng.integers(0, 2**32)), L.BOOLBITS: int(rng.integers(0, 2))}[dtype]
        gathers.append(dict(dtype=dtype, v=sv, nulls=sn, fill=fill, space=str(rng.choice(SPACES)), out_device=bool(rng.random() < 0.5)))
    return dict(n=n, select=select, runs=runs, v=v, cnull=cnull, gathers=gathers, indices=bool(rng.random() < 0.7),
                space=str(rng.choice(SPACES)))


def classify_filter(d):
    f = ["filter.select=%s" % d["select"], "filter.cond_space=%s" % d["space"], "filter.indices=%d" % d["indices"]]
    f += ["filter.gather=%s" % DT_NAME[g["dtype"]] for g in d["gathers"]] + ["filter.src_space=%s" % g["space"] for g in d["gathers"]]
    for cond, name in ((d["runs"], "filter.long_runs"), (d["cnull"] is not None, "filter.cond_null_mask"),
                       (any(g["nulls"] is not None for g in d["gathers"]), "filter.src_null_mask"),
                       (len(d["gathers"]) > 1, "filter.several_gathers"), (d["n"] % 64 != 0, "filter.partial_last_word")):
        if cond:
            f.append(name)
    return f


FILTER_FEATURES = (["filter.select=%s" % s for s in SELECT] + ["filter.cond_space=%s" % s for s in SPACES] +
                   ["filter.src_space=%s" % s for s in SPACES] + ["filter.indices=0", "filter.indices=1"] +
                   ["filter.gather=%s" % v for v in DT_NAME.values()] +
                   ["filter.long_runs", "filter.cond_null_mask", "filter.src_null_mask", "filter.several_gathers", "filter.partial_last_word"])


def cond_bits(v, n):
    data = bits(v)
    if n % 8:
        data[-1] |= np.uint8(0xFF << (n % 8) & 0xFF)          # bits past the last row are not rows
    return data


def run_filter(ctx, d):
    n, keep = d["n"], []
    rows = filter_ref(d["v"], d["cnull"])
    try:
        cond = place(ctx, d["space"], cond_bits(d["v"], n), None if d["cnull"] is None else bits(d["cnull"]), L.BOOLBITS, n, keep)
        idx, cnt = ctx.filter_indices(cond, n, indices=d["indices"])
        check(cnt == len(rows), "count", (cnt, len(rows)))
        if d["indices"]:
            check(np.array_equal(idx.cpu().numpy(), rows), "indices", first_diff_any(idx.cpu().numpy(), rows))
        for k, g in enumerate(d["gathers"]):
            data = bits(g["v"]) if g["dtype"] == L.BOOLBITS else g["v"]
            src = place(ctx, g["space"], data, None if g["nulls"] is None else bits(g["nulls"]), g["dtype"], n, keep)
            got = to_np(ctx.filter_gather(src, n, cnt, g["fill"], out_device=g["out_device"]))
            fill = np.array(g["fill"], np.float64 if g["dtype"] == L.F64 else np.int64 if g["dtype"] == L.I64 else np.uint32 if g["dtype"] == L.U32CODE else np.bool_)
            _, want = filter_ref(d["v"], d["cnull"], g["v"], g["nulls"], fill)
            if g["dtype"] == L.U32CODE:
                got = got.view(np.uint32)
            check(got.dtype == want.dtype and got.tobytes() == want.tobytes(), "gather %d (%s)" % (k, DT_NAME[g["dtype"]]), first_diff_any(got, want))
    finally:
        for r in keep:
            if hasattr(r, "release"):
                r.release()


def desc_filter(d):
    return "filter n=%d select=%s runs=%d cond_null=%d indices=%d space=%s gathers=%s" % (
        d["n"], d["select"], d["runs"], d["cnull"] is not None, d["indices"], d["space"],
        [(DT_NAME[g["dtype"]], g["nulls"] is not None, g["fill"], g["space"], int(g["out_device"])) for g in d["gathers"]])


# ---- window ------------------------------------------------------------------------------------------------------------------
WINDOW_N = [1, 2, 3, 63, 64, 65, 1791, 1792, 1793, 4095, 4096, 4097, 8191, 8193, 12_289, 100_003, 400_001, 2_000_003]
W_SMALL = [1, 2, 3, 63, 64, 65]
W_CHUNK = [2304, 2305, 2306, 4095, 4096, 4097]                  # 1792 outputs + w - 1 values against the 4096-value LDS chunk
KIND_OPS = [(k, op) for k in ("rolling", "expanding") for op in OPS] + [("ewm", op) for op in ("mean", "std", "var")]


def data_of(rng, n, null_p, special=True):
    """tests/test_gpu_window.py's data_of."""
    x = rng.normal(0, 100, n)
    r = rng.random(n) < 0.3
    x[r] = np.round(x[r])                                                # ties
    if special and n >= 20:
        k = rng.choice(n, size=max(5, n // 200), replace=False)
        x[k] = rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e300, -1e-300], size=len(k))
    valid = rng.random(n) >= null_p
    return x, valid


def draw_window(rng, case):
    kind, op = KIND_OPS[case % len(KIND_OPS)] if rng.random() < 0.8 else KIND_OPS[int(rng.integers(0, len(KIND_OPS)))]
    n = int(rng.choice(WINDOW_N))
    exact = kind == "rolling" or op in ("min", "max", "count")
    w = 0
    if kind == "rolling":
        cls = str(rng.choice(["small", "small", "chunk", "thousands", "around_n", "any"]))
        fold_op = op in ("sum", "mean", "var", "std")            # the fold reference costs n * w
        if cls in ("around_n", "any"):
            n = min(n, 6143 if fold_op else 12_289)
        w = int({"small": lambda: rng.choice(W_SMALL), "chunk": lambda: rng.choice(W_CHUNK), "thousands": lambda: rng.integers(1000, 6000),
                 "around_n": lambda: max(1, n + rng.choice([-1, 0, 5])), "any": lambda: rng.integers(1, n + 6)}[cls]())
        if fold_op:
            n = min(n, max(50_000_000 // w, 1))
    elif kind == "ewm":
        n = min(n, 100_003)
    elif op in ("var", "std"):
        n = min(n, 8193)
    elif op in ("min", "max"):
        n = min(n, 400_001)
    null_p = float(rng.choice([0, 0.1, 0.9, 1]))
    i64 = bool(rng.random() < 0.3)
    if i64:
        v = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        small = rng.random(n) < 0.5
        v[small] = rng.integers(-1000, 1000, int(small.sum()))
        if not exact:
            v = rng.integers(-10**6, 10**6, n, dtype=np.int64)
        x, valid = v.astype(np.float64), rng.random(n) >= null_p
        data = v
    else:
        x, valid = data_of(rng, n, null_p, special=exact)      # the bounded statistics are stated for finite values
        data = x
    mp = ([None, 0, 1, max(w // 2, 1), int(rng.integers(0, w + 1))] if kind == "rolling" else [0, 1, 3, 50])[int(rng.integers(0, 4 + (kind == "rolling")))]
    return dict(kind=kind, op=op, n=n, w=w, center=bool(rng.random() < 0.5), mp=mp, ddof=int(rng.choice([0, 1, 1, 2])),
                alpha=float(rng.choice([1.0, 0.5, 0.05, 2.0 / 31.0, 1.0 - rng.random()])), null_p=null_p, i64=i64, data=data, x=x,
                valid=valid, space=str(rng.choice(SPACES)))


def classify_window(d):
    f = ["window.%s.%s" % (d["kind"], d["op"]), "window.dtype=%s" % ("i64" if d["i64"] else "f64"), "window.space=%s" % d["space"],
         "window.null_rate=%g" % d["null_p"]]
    if d["kind"] == "rolling":
        w = d["w"]
        f.append("window.w " + ("1..3" if w <= 3 else "63..65" if 63 <= w <= 65 else "at the LDS chunk" if w in W_CHUNK else
                                ">n" if w > d["n"] else "thousands" if w >= 1000 else "other"))
        f.append("window.center=%d" % d["center"])
    return f


WINDOW_FEATURES = (["window.%s.%s" % ko for ko in KIND_OPS] + ["window.dtype=i64", "window.dtype=f64"] + ["window.space=%s" % s for s in SPACES] +
                   ["window.null_rate=%g" % p for p in (0, 0.1, 0.9, 1)] +
                   ["window.w " + c for c in ("1..3", "63..65", "at the LDS chunk", ">n", "thousands")] + ["window.center=0", "window.center=1"])


def window_check(d, got):
    """The comparison tests/test_gpu_window.py makes for this kind and op."""
    kind, op, x, valid = d["kind"], d["op"], d["x"], d["valid"]
    got = np.asarray(got, np.float64)
    check(got.shape == x.shape, "shape", (got.shape, x.shape))
    if kind == "rolling":
        want = WR.rolling_ref(x, valid, d["w"], d["center"], op, mp=d["mp"], ddof=d["ddof"])
        check(WR.same(got, want), "rolling %s" % op, WR.first_diff(got, want))
    elif kind == "expanding" and op in ("min", "max", "count"):
        want = WR.expanding_ref_exact(x, valid, op, d["mp"])
        check(WR.same(got, want), "expanding %s" % op, WR.first_diff(got, want))
    elif kind == "expanding" and op in ("sum", "mean"):
        check(WR.expanding_sum_mean_close(got, x, valid, d["mp"], op == "mean"), "expanding %s outside its bound" % op)
    elif kind == "expanding":
        check(WR.expanding_var_std_close(got, x, valid, d["ddof"], d["mp"], op == "std"), "expanding %s outside its bound" % op)
    else:
        want = WR.ewm_ref(x, valid, d["alpha"], op)
        check(WR.ewm_close(got, want, x, valid, op == "var"), "ewm %s outside its bound" % op)


def window_call(ctx, col, d):
    kw = dict(min_periods=d["mp"] if d["mp"] is not None else -1)
    if d["kind"] == "rolling":
        kw.update(window=d["w"], center=d["center"], ddof=d["ddof"])
    elif d["kind"] == "expanding":
        kw.update(ddof=d["ddof"])
    else:
        kw = dict(alpha=d["alpha"])
    return ctx.window(col, d["n"], WKINDS[d["kind"]], OPS[d["op"]], **kw)


def run_window(ctx, d):
    keep = []
    try:
        col = place(ctx, d["space"], d["data"], None if d["valid"].all() else bits(~d["valid"]), L.I64 if d["i64"] else L.F64, d["n"], keep)
        got = to_np(window_call(ctx, col, d))
    finally:
        for r in keep:
            if hasattr(r, "release"):
                r.release()
    window_check(d, got)


def desc_window(d):
    return "window %s %s n=%d w=%d center=%d mp=%s ddof=%d alpha=%.6g null_p=%g %s space=%s" % (
        d["kind"], d["op"], d["n"], d["w"], d["center"], d["mp"], d["ddof"], d["alpha"], d["null_p"], "i64" if d["i64"] else "f64", d["space"])


# ---- chains: every intermediate stays on the device ---------------------------------------------------------------------------
def draw_chain(rng, case):
    shape = CHAINS[case % len(CHAINS)]
    n = int(rng.integers(1_100_000, 2_500_000)) if shape == "sort_clustered_groupby" else int(rng.choice([4097, 65_537, 300_007, 1_000_003]))
    g = int(rng.choice([3, 500, 20_000]))
    key = rng.integers(-g // 2, g - g // 2, n).astype(np.int64) * int(rng.choice([1, 7919, 1 << 33]))
    fkey = rng.choice([0.5, -0.0, 0.0, 2.0, np.nan, -7.25, 1e9], n)
    val = rng.normal(50, 20, n)
    ties = rng.random(n) < 0.3
    val[ties] = np.round(val[ties])
    vnull = rng.random(n) < 0.1 if rng.random() < 0.6 else None
    cond = rng.random(n) < rng.choice([0.1, 0.5, 0.95])
    cnull = rng.random(n) < 0.1 if rng.random() < 0.5 else None
    wop = str(rng.choice(["sum", "mean", "min", "max", "count", "std"]))
    w = int(rng.choice([2, 3, 64, 700]))
    if wop in ("sum", "mean", "std") and n > 65_537:             # the fold reference costs n * w
        w = min(w, 64)
    return dict(shape=shape, n=n, g=g, key=key, fkey=fkey, val=val, vnull=vnull, cond=cond, cnull=cnull, asc=[bool(rng.random() < 0.5) for _ in range(2)],
                w=w, wop=wop, wkind=str(rng.choice(["rolling", "rolling", "expanding"])) if wop in ("min", "max", "count") and n <= 300_007 else "rolling",
                space=str(rng.choice(["host", "device", "resident"])),
                aggs=[(0, int(op)) for op in rng.choice([0, 1, 2, 3, 4], size=int(rng.integers(1, 5)), replace=False)])


def classify_chain(d):
    return ["chain.%s" % d["shape"], "chain.first_stage_space=%s" % d["space"]]


CHAIN_FEATURES = ["chain.%s" % s for s in CHAINS] + ["chain.first_stage_space=%s" % s for s in ("host", "device", "resident")]


def run_chain(ctx, d):
    import torch
    from oracle import oracle as O
    from tests.helpers import assert_groupby_equal
    n, keep, shape = d["n"], [], d["shape"]
    key, fkey, val, vnull = d["key"], d["fkey"], d["val"], d["vnull"]
    up = lambda data, mask, dtype: place(ctx, d["space"], data, mask, dtype, n, keep)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    try:
        if shape.startswith("filter"):                           # ---- stage 1: filter, k columns compacted onto the device
            rows = filter_ref(d["cond"], d["cnull"])
            _, cnt = ctx.filter_indices(up(cond_bits(d["cond"], n), None if d["cnull"] is None else bits(d["cnull"]), L.BOOLBITS), n, indices=False)
            check(cnt == len(rows), "filter count", (cnt, len(rows)))
            vm = None if vnull is None else bits(vnull)
            d_key = ctx.filter_gather(up(key, None, L.I64), n, cnt, 0, out_device=True)
            d_fkey = ctx.filter_gather(up(fkey, None, L.F64), n, cnt, 0.0, out_device=True)
            d_val = ctx.filter_gather(up(val, vm, L.F64), n, cnt, -1.5, out_device=True)
            key, fkey = key[rows], fkey[rows]
            val = filter_ref(d["cond"], d["cnull"], val, vnull, np.float64(-1.5))[1]
            for name, got, want in (("key", d_key, key), ("fkey", d_fkey, fkey), ("val", d_val, val)):
                check(got.cpu().numpy().tobytes() == want.tobytes(), "filter_gather %s" % name, first_diff_any(got.cpu().numpy(), want))
            m = cnt
            if vnull is not None:                                # the null flags travel as a bool column and become a bitmap again
                flags = ctx.filter_gather(up(bits(vnull), None, L.BOOLBITS), n, cnt, 0, out_device=True)
                vnull = vnull[rows]
                check(np.array_equal(flags.cpu().numpy(), vnull.astype(np.uint8)), "filter_gather null flags")
                d_vmask = ctx.bytes_to_bitmap(flags) if m else None
            else:
                d_vmask = None
        else:
            m, d_key, d_fkey, d_val = n, dev(key), dev(fkey), dev(val)
            d_vmask = None if vnull is None else dev(bits(vnull))
        if m == 0:
            return
        if shape == "filter_groupby":                            # ---- groupby of the compacted device columns
            got = ctx.groupby_agg([(d_key, None, L.I64)], m, [(d_val, d_vmask, L.F64)], d["aggs"])
            got = tuple(t.cpu().numpy() for t in got)
            got = (got[0].view(np.uint64), got[1], got[2])
            want = O.groupby_agg([(key, None, O.I64)], m, [(val, None if vnull is None else bits(vnull), O.F64)], d["aggs"])
            assert_groupby_equal(got, want, [O.I64], int_exact_rows=[i for i, (_, op) in enumerate(d["aggs"]) if op in (O.MIN, O.MAX, O.COUNT)], rtol=1e-9)
            return
        # ---- sort by (key, fkey), gather through the row order ----
        cols = [Col(L.I64, key), Col(L.F64, fkey)]
        order = ctx.sort_indices([(d_key, None, L.I64), (d_fkey, None, L.F64)], m, d["asc"])
        want_order = ref_lexsort(cols, d["asc"])
        check(np.array_equal(order.cpu().numpy(), want_order), "sort after %s" % shape.split("_")[0], first_diff_any(order.cpu().numpy(), want_order))
        s_val = ctx.gather(d_val, d_vmask, order, -2.5, L.F64)
        s_key = ctx.gather(d_key, None, order, 0, L.I64)
        val = np.where(vnull[want_order], -2.5, val[want_order]) if vnull is not None else val[want_order]
        key = key[want_order]
        check(s_val.cpu().numpy().tobytes() == val.tobytes(), "gather val by the row order", first_diff_any(s_val.cpu().numpy(), val))
        check(np.array_equal(s_key.cpu().numpy(), key), "gather key by the row order")
        if shape == "sort_clustered_groupby":                    # ---- the rows are now sorted by key: the clustered-rows pass
            ctx.set_option("no_small", 1)
            try:
                got = ctx.groupby_agg([(s_key, None, L.I64)], m, [(s_val, None, L.F64)], d["aggs"])
                d["clustered"] = ctx.timings()["n_partitions"] == -2
            finally:
                ctx.set_option("no_small", 0)
            got = tuple(t.cpu().numpy() for t in got)
            got = (got[0].view(np.uint64), got[1], got[2])
            want = O.groupby_agg([(key, None, O.I64)], m, [(val, None, O.F64)], d["aggs"])
            assert_groupby_equal(got, want, [O.I64], int_exact_rows=[i for i, (_, op) in enumerate(d["aggs"]) if op in (O.MIN, O.MAX, O.COUNT)], rtol=1e-9)
            return
        # ---- a window over the gathered value column ----
        wd = dict(kind=d["wkind"], op=d["wop"], n=m, w=d["w"], center=False, mp=1, ddof=1, alpha=0.0, x=val, valid=np.ones(m, bool))
        window_check(wd, window_call(ctx, (s_val, None, L.F64), wd).cpu().numpy())
    finally:
        for r in keep:
            if hasattr(r, "release"):
                r.release()


def desc_chain(d):
    return "chain %s n=%d g=%d asc=%s vnull=%d cnull=%d window=%s/%s/%d aggs=%s space=%s%s" % (
        d["shape"], d["n"], d["g"], [int(a) for a in d["asc"]], d["vnull"] is not None, d["cnull"] is not None, d["wkind"], d["wop"], d["w"],
        d["aggs"], d["space"], " clustered=%d" % d["clustered"] if "clustered" in d else "")


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
# kind -> (draw, classify, run, desc, features, expect).  expect (the column ops' kinds and chain2) computes every reference
# result of a drawn case without the engine: what FUZZ_DRY=2 runs, and what run() compares the device with.
DRAW = {"sort": (draw_sort, classify_sort, run_sort, desc_sort, SORT_FEATURES, None),
        "filter": (draw_filter, classify_filter, run_filter, desc_filter, FILTER_FEATURES, None),
        "window": (draw_window, classify_window, run_window, desc_window, WINDOW_FEATURES, None),
        "chain": (draw_chain, classify_chain, run_chain, desc_chain, CHAIN_FEATURES, None)}
DRAW.update(fuzz_columns.KINDS)
DRAW.update(fuzz_chain2.KINDS)
KINDS = tuple(DRAW)
# With FUZZ_KIND unset: the four older kinds keep their shares of one half, the nine newer ones share the other.
KIND_P = [0.2, 0.1, 0.15, 0.05] + [0.5 / (len(KINDS) - 4)] * (len(KINDS) - 4)
KIND = os.environ.get("FUZZ_KIND", "")
assert KIND in ("",) + KINDS, KIND


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    first_case = int(os.environ.get("FUZZ_FIRST", "0"))
    ctx = None
    if not DRY:
        import torch  # noqa: F401  (before the library's first HIP call, as bench.py does)
        import pandrs_amd as pa
        ctx = pa.Context(0)
        if os.environ.get("FUZZ_POISON"):       # every workspace block is filled with this byte before a call uses it
            pa.Context.poison_workspace(int(os.environ["FUZZ_POISON"], 0))
    fails = 0
    for case in range(first_case, n_cases):
        rng = np.random.default_rng(seed0 * 100003 + case)
        kind = KIND or KINDS[int(rng.choice(len(KINDS), p=KIND_P))]
        draw, classify, run, desc, _, expect = DRAW[kind]
        d = text = None
        try:
            d = draw(rng, case)
            text = desc(d)
            feats = set(classify(d))
            if DRY_MODE == 2 and expect is not None:
                expect(d)
            if not DRY:
                run(ctx, d)
                text = desc(d)
                feats -= set(d.get("uncount", ())) if isinstance(d, dict) else set()
            for f in feats:
                cov[f] += 1
            print("ok   %3d %s" % (case, text), flush=True)
        except Exception:
            fails += 1
            print("FAIL %3d %s" % (case, text or kind), flush=True)
            traceback.print_exc()
            sys.stderr.flush()
    if ctx is not None:
        ctx.close()
    wanted = [f for k in ((KIND,) if KIND else KINDS) for f in DRAW[k][4]]
    print("coverage (%s):" % ("cases run" if not DRY else "dry run: drawn and classified, no engine call" if DRY_MODE == 1 else
                              "dry run: drawn, classified and every reference result computed, no engine call"))
    for f in wanted:
        print("  %-46s %d" % (f, cov[f]))
    missed = [f for f in wanted if cov[f] == 0]
    if missed:
        print("coverage: %d features not reached: %s" % (len(missed), missed))
    print("fuzz_ops done: %d cases, %d failures" % (n_cases - first_case, fails), flush=True)
    sys.exit(1 if fails or (missed and not first_case and DRY_MODE != 2) else 0)      # FUZZ_DRY=2 caps the row counts


if __name__ == "__main__":
    main()
