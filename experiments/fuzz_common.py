"""What the kinds of experiments/fuzz_ops.py share: the switches, the coverage ledger, the mismatch type, placing a column
in a memory space, caller-owned outputs with guard cells, and the draws every column op's kind makes (input space, output
placement, dtype, null layout, special cells, row count).  No kind lives here."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pandrs_amd import _lib as L  # noqa: E402

DRY_MODE = int(os.environ.get("FUZZ_DRY", "0") or "0")          # 1: draw and classify; 2: also every reference expectation
assert DRY_MODE in (0, 1, 2), DRY_MODE
DRY = DRY_MODE != 0

SPACES = ("host", "device", "device_offset", "resident")
DT_NAME = {L.I64: "i64", L.F64: "f64", L.U32CODE: "str", L.BOOLBITS: "bool"}
NP_OF = {L.I64: np.int64, L.F64: np.float64, L.U32CODE: np.uint32}
cov = collections.Counter()
HEADER = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
MI355X_CUS = 256                                                # the dry run cannot ask the device


def bits(a):
    return np.packbits(np.asarray(a, bool), bitorder="little")


class Mismatch(AssertionError):
    pass


def check(ok, what, detail=None):
    if not ok:
        raise Mismatch("%s%s" % (what, "" if detail is None else ": %s" % (detail,)))


def first_diff_any(got, want):
    """First differing position of two arrays compared by their bytes (floats through their int64 view)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    if got.dtype == np.float64 and want.dtype == np.float64:
        gi, wi = got.view(np.int64), want.view(np.int64)
    else:
        gi, wi = got, want
    bad = np.flatnonzero(gi != wi)
    return None if not len(bad) else (int(bad[0]), got[bad[0]].item(), want[bad[0]].item())


# ---- placing a column in a memory space -----------------------------------------------------------------------------
def place(ctx, space, data, mask, dtype, n, keep):
    """(data, mask, dtype) host arrays -> what the engine takes, in `space`.  device_offset: the data 8 bytes into its
    allocation (8-byte aligned, not 256), the mask 3 bytes into its own (odd)."""
    if space == "host":
        return (data, mask, dtype)
    if space == "resident":
        r = ctx.upload_column_n(data, mask, dtype, n)
        keep.append(r)
        return r
    import torch
    def dev(a, lead):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
        if not lead:
            return t.to("cuda:0")
        buf = torch.zeros(len(t) + lead + 3, dtype=t.dtype, device="cuda:0")
        buf[lead:lead + len(t)] = t.to("cuda:0")
        return buf[lead:lead + len(t)]
    off = space == "device_offset"
    d = dev(data, (8 // data.dtype.itemsize) if off else 0)
    m = None if mask is None else dev(mask, 3 if off else 0)
    return (d, m, dtype)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def release(keep):
    for r in keep:
        if hasattr(r, "release"):
            r.release()


# ---- caller-owned device outputs between guard cells ----------------------------------------------------------------------
class Guarded:
    """A device buffer of n cells one cell into its allocation - 8 mod 16 for the 8-byte cells, byte offset 1 for a bitmap -
    with guard cells on both sides that intact() reads back."""

    def __init__(self, n, np_dtype):
        import torch
        self.n, self.pat = int(n), (0xA5 if np.dtype(np_dtype) == np.uint8 else -7)
        tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}[np.dtype(np_dtype)]
        self.buf = torch.full((self.n + 4,), self.pat, dtype=tdt, device="cuda:0")
        self.view = self.buf[1:1 + self.n]
        assert self.buf.data_ptr() % 16 == 0

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:1] == self.pat).all() and (b[1 + self.n:] == self.pat).all())


OUTS = ("host", "device", "guarded")


def out_kwargs(outp, n, cell_dtype, with_mask, mask_kw="out_mask"):
    """-> (keyword arguments of the call, the Guarded buffers to check afterwards).  cell_dtype None: the output is a bitmap."""
    if outp != "guarded":
        return dict(out_device=outp == "device"), []
    nbytes = (n + 7) // 8
    g = Guarded(nbytes if cell_dtype is None else n, np.uint8 if cell_dtype is None else cell_dtype)
    kw, guards = dict(out=g.view), [g]
    if with_mask:
        gm = Guarded(nbytes, np.uint8)
        kw[mask_kw] = gm.view
        guards.append(gm)
    return kw, guards


def check_guards(guards):
    for g in guards:
        check(g.intact(), "a guard cell around the caller's output was written")


# ---- the geometry the header documents --------------------------------------------------------------------------------------
def geometry(op):
    """(rows per workgroup iteration, workgroups per compute unit) of one entry point, as its directed test reads them."""
    return (int(re.search(r"%s_tile_rows = (\d+)" % op, HEADER).group(1)), int(re.search(r"%s_blocks_per_cu = (\d+)" % op, HEADER).group(1)))


def grid_is_exceeded(n, op):
    """At run time: does a full persistent grid of this device leave tiles over, so that a workgroup takes a second one?"""
    import torch
    tile, per_cu = geometry(op)
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu * tile < n


SIZE_NAMES = ("0", "1", "2", "63", "64", "65", "tile-1", "tile", "tile+1", "2 tiles-1", "2 tiles+1", "grid+1", "other")
NULL_LAYOUTS = ("no mask", "mask without a bit", "p=0.01", "p=0.5", "all null")


def size_of(name, tile, per_cu, rng):
    if name == "grid+1":
        return per_cu * MI355X_CUS * tile + 1
    if name == "other":
        return int(rng.integers(3, 3 * tile + 1))
    return {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2 tiles-1": 2 * tile - 1, "2 tiles+1": 2 * tile + 1}.get(name) or int(name)


def pick(rng, case, options, stride=1, stray=0.2):
    """The structured draw: options[(case // stride) mod len], and now and then any of them, so that the dimensions mix."""
    k = (case // stride) % len(options)
    r = int(rng.integers(0, len(options)))
    return options[r if rng.random() < stray else k]


def shared_draw(rng, case, tile, per_cu, dtypes, outs=OUTS, sizes=SIZE_NAMES, max_n=None):
    """The draws every column op's kind makes.  One grid-sized case in 195 (its twins are what a dry run costs), the other size
    classes once in 13."""
    size = SIZE_NAMES[case % 13] if sizes is SIZE_NAMES else sizes[case % len(sizes)]
    if size == "grid+1" and case % 195 != 11:
        size = "other"
    n = size_of(size, tile, per_cu, rng)
    if max_n is not None and n > max_n:
        size, n = "other", int(rng.integers(3, min(max_n, 3 * tile) + 1))
    space = pick(rng, case, SPACES)
    if n == 0 and space in ("device_offset", "resident"):         # no row to upload, no cell to offset
        space = ("host", "device")[case // 4 % 2]
    return dict(n=n, size=size, space=space, outp=pick(rng, case, outs, 7) if outs else None, dtype=pick(rng, case, dtypes, 4),
                nulls=pick(rng, case, NULL_LAYOUTS, 2), specials=bool(rng.random() < 0.5), uncount=[])


def shared_classify(kind, d):
    f = ["%s.space=%s" % (kind, d["space"]), "%s.dtype=%s" % (kind, DT_NAME[d["dtype"]]), "%s.n=%s" % (kind, d["size"])]
    if d["nulls"] is not None:                                  # None: the column came from a reference module's own sweep
        f.append("%s.nulls=%s" % (kind, d["nulls"]))
    if d["outp"] is not None:
        f.append("%s.out=%s" % (kind, d["outp"]))
    if d["specials"] and d["n"] >= 8 and d["dtype"] in (L.I64, L.F64):
        f.append("%s.%s" % (kind, "f64 NaN, inf, -0.0, subnormal cells" if d["dtype"] == L.F64 else "i64 beyond 2^53 and both extremes"))
    return f


def shared_features(kind, dtypes, outs=OUTS, sizes=SIZE_NAMES):
    f = (["%s.space=%s" % (kind, s) for s in SPACES] + ["%s.out=%s" % (kind, o) for o in outs] + ["%s.dtype=%s" % (kind, DT_NAME[t]) for t in dtypes] +
         ["%s.nulls=%s" % (kind, s) for s in NULL_LAYOUTS] + ["%s.n=%s" % (kind, s) for s in sizes])
    if L.F64 in dtypes:
        f.append("%s.f64 NaN, inf, -0.0, subnormal cells" % kind)
    if L.I64 in dtypes:
        f.append("%s.i64 beyond 2^53 and both extremes" % kind)
    return f


def grid_checked(d, kind, op):
    """Run time: a grid-sized case counts toward its feature only where the device's grid really leaves a tile over."""
    if d["size"] == "grid+1" and not grid_is_exceeded(d["n"], op):
        d["uncount"].append("%s.n=grid+1" % kind)


def describe_case(kind, d):
    """One line per case: every scalar the draw holds."""
    return "%s %s" % (kind, " ".join("%s=%s" % (k, v) for k, v in d.items() if k not in ("uncount", "want") and (v is None or isinstance(v, (int, float, str, bool, tuple)))))


F64_SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 5e-324])
I64_SPECIALS = np.array([I64_MIN, I64_MAX, 2**53 + 1, -(2**53) - 1, 2**62 + 12345], np.int64)


def nulls_of(rng, n, layout):
    if layout == "no mask":
        return None
    if layout == "mask without a bit":
        return np.zeros(n, bool)
    if layout == "all null":
        return np.ones(n, bool)
    return rng.random(n) < (0.01 if layout == "p=0.01" else 0.5)


def sprinkle(rng, x):
    """Every special value of x's dtype at a few random rows (columns of at least 8 rows)."""
    n = x.shape[0]
    if n < 8:
        return x
    sp = F64_SPECIALS if x.dtype == np.float64 else I64_SPECIALS
    rows = rng.choice(n, size=min(n, max(len(sp), n // 100)), replace=False)
    x[rows] = np.resize(sp, len(rows))
    return x


def plain_column(rng, n, dtype, specials):
    """Normal cells with ties (a third of them rounded), or integers in +-1000; the special cells on top."""
    if dtype == L.I64:
        x = rng.integers(-1000, 1000, n).astype(np.int64)
    else:
        x = rng.normal(0, 100, n)
        r = rng.random(n) < 0.3
        x[r] = np.round(x[r])
    return sprinkle(rng, x) if specials else x


def mask_of(nulls):
    return None if nulls is None else bits(nulls)


def unpack(mask, n):
    return np.unpackbits(np.asarray(mask, np.uint8), count=n, bitorder="little").astype(bool) if n else np.zeros(0, bool)


def expect_status(call, status, what):
    """A documented refusal, drawn as a case of its own: the call must raise the library's error with this status."""
    import pandrs_amd as pa
    try:
        call()
    except pa.PandrsHipError as e:
        check(e.status == status, "%s: status" % what, (e.status, status))
        return
    raise Mismatch("%s: the call was not refused" % what)
