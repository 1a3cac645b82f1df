"""pandrs_hip_grouped and GroupBy's cumsum / cummax / cummin / cumcount / row_number / shift / diff / pct_change: the parts that
need no GPU — the mirror's methods and errors (raised before any device call), the constants, the C ABI entry point without a
device, the header / ctypes / Rust / C++ declarations, the C++ mirror compiled against the header, and that no kernel of
grouped.hip uses scratch."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ["ctx", "mem_space", "col", "n_rows", "op", "periods", "out_mem_space", "out_data", "out_null_mask", "out_n_null"]
ENUM = {"CUM_SUM": 0, "CUM_MAX": 1, "CUM_MIN": 2, "CUM_COUNT": 3, "ROW_NUMBER": 4, "SHIFT": 5, "DIFF": 6, "PCT_CHANGE": 7}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from pandrs_amd import _lib
    return _lib


def _frame():
    import pandrs_amd.frame as F
    df = F.OptimizedDataFrame()
    df.add_column("k", F.Int64Column([1, 2, 1, 2]))
    df.add_column("x", F.Float64Column.with_nulls([0.5, np.nan, 1.0, 2.0], [False, False, True, False]))
    df.add_column("s", F.StringColumn(["a", "b", "c", "d"]))
    df.add_column("flag", F.BooleanColumn([True, False, True, False]))
    return df


def _calls(g):
    return [g.cumsum, g.cummax, g.cummin, g.cumcount, lambda c: g.shift(c, 1), lambda c: g.shift(c, -2), lambda c: g.diff(c, 1),
            lambda c: g.pct_change(c, 2)]


def test_mirror_has_the_methods_and_the_constants(built):
    import pandrs_amd.engine as E
    import pandrs_amd.frame as F
    for name in ("cumsum", "cummax", "cummin", "cumcount", "row_number", "shift", "diff", "pct_change", "transform"):
        assert callable(getattr(F.GroupBy, name))
    assert callable(E.Context.grouped) and callable(E.Context.groupby_indices_compute)
    for k, v in ENUM.items():
        assert getattr(built, "GROUPED_" + k) == v
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    body = header[header.index("typedef enum pandrs_hip_grouped_op {"):header.index("} pandrs_hip_grouped_op;")]
    assert dict((k, int(v)) for k, v in re.findall(r"PANDRS_HIP_GROUPED_(\w+) = (\d+)", body)) == ENUM
    hpp = open(os.path.join(ROOT, "include", "pandrs_hip.hpp")).read()
    cls = hpp[hpp.index("class GroupBy {"):]
    for k in ENUM:
        assert "PANDRS_HIP_GROUPED_" + k in cls, k
    assert "pandrs_hip_grouped(detail::context()" in cls


def test_errors_are_raised_before_any_device_call(built, monkeypatch):
    import pandrs_amd.frame as F

    def no_device():
        raise AssertionError("the device was touched")
    monkeypatch.setattr(F, "get_context", no_device)
    df = _frame()
    with pytest.raises(F.ColumnNotFound):
        df.group_by(["nope"])
    g = df.group_by(["k"])
    for call in _calls(g):
        with pytest.raises(F.ColumnNotFound):
            call("nope")
        for col in ("s", "flag"):
            with pytest.raises(F.ColumnTypeMismatch) as e:
                call(col)
            assert "Column '%s' is not a numeric type" % col in str(e.value)
    for call in (g.diff, g.pct_change):
        with pytest.raises(F.InvalidValue):
            call("x", -1)
        with pytest.raises(F.ColumnNotFound):
            call("nope", -1)                                               # the column is looked up first
    empty = F.OptimizedDataFrame()
    empty.add_column("k", F.Int64Column([]))
    empty.add_column("b", F.Float64Column([]))
    ge = empty.group_by(["k"])
    for call in _calls(ge):
        assert call("k") == [] and call("b") == []
    assert ge.row_number() == []


def test_frame_results_come_from_one_grouping_and_one_call_each(built, monkeypatch):
    """A stand-in context: the GroupBy builds the grouping once, hands the column's view, the row count, the op's number and the
    periods to Context.grouped once per method, regroups only after somebody else's groupby_indices has bumped the token, and
    turns what comes back into lists aligned with the rows."""
    import pandrs_amd.frame as F
    calls = []

    class Fake:
        grouping_token = 0

        def groupby_indices_compute(self, keys, n_rows):
            self.grouping_token += 1
            calls.append(("group", [k[2] for k in keys], n_rows))
            return 2, built.MEM_HOST

        def grouped(self, col, n_rows, op, periods=0, out=None, out_mask=None, out_device=None):
            calls.append(("grouped", None if col is None else col[2], n_rows, op, periods, out_device))
            if op in (built.GROUPED_CUM_COUNT, built.GROUPED_ROW_NUMBER):
                return np.arange(n_rows, dtype=np.int64), None, 0
            return np.array([np.nan, 1.5, np.nan, 3.5]), np.array([0x01], np.uint8), 1

    fake = Fake()
    monkeypatch.setattr(F, "get_context", lambda: fake)
    g = _frame().group_by(["k", "s"])
    got = g.cumsum("x")
    assert np.isnan(got[0]) and got[1] == 1.5 and all(type(v) is float for v in got)
    got = g.cumcount("x")
    assert got == [0, 1, 2, 3] and all(type(v) is int for v in got)
    assert g.row_number() == [0, 1, 2, 3]
    got = g.shift("x", -3)
    assert got[0] is None and got[1] == 1.5 and np.isnan(got[2]) and got[3] == 3.5       # None by the bit, not by the NaN
    g.diff("k", 2), g.pct_change("x", 0), g.cummax("k"), g.cummin("x")
    assert calls == [("group", [built.I64, built.U32CODE], 4), ("grouped", built.F64, 4, built.GROUPED_CUM_SUM, 0, False),
                     ("grouped", built.F64, 4, built.GROUPED_CUM_COUNT, 0, False), ("grouped", None, 4, built.GROUPED_ROW_NUMBER, 0, False),
                     ("grouped", built.F64, 4, built.GROUPED_SHIFT, -3, False), ("grouped", built.I64, 4, built.GROUPED_DIFF, 2, False),
                     ("grouped", built.F64, 4, built.GROUPED_PCT_CHANGE, 0, False), ("grouped", built.I64, 4, built.GROUPED_CUM_MAX, 0, False),
                     ("grouped", built.F64, 4, built.GROUPED_CUM_MIN, 0, False)]
    del calls[:]
    fake.grouping_token += 1                                               # somebody else grouped through this context
    g.row_number(), g.row_number()
    assert [c[0] for c in calls] == ["group", "grouped", "grouped"]


def test_entry_point_without_a_context_is_not_initialized(built):
    lib = built.load()
    x = np.arange(8, dtype=np.float64)
    col = built.Column()
    col.data, col.dtype = x.ctypes.data, built.F64
    out, mask, nulls = np.full(8, -1.0), np.full(1, 0xAA, np.uint8), C.c_int64(-5)
    for op in ENUM.values():
        st = lib.pandrs_hip_grouped(None, built.MEM_HOST, C.byref(col), 8, op, 1, built.MEM_HOST, out.ctypes.data, mask.ctypes.data, C.byref(nulls))
        assert st == built.ERR_NOT_INITIALIZED
        assert "context" in built.last_error() and (out == -1.0).all() and mask[0] == 0xAA and nulls.value == -5


def test_header_ctypes_and_rust_declarations_agree(built):
    header = open(os.path.join(ROOT, "include", "pandrs_hip.h")).read()
    spec = importlib.util.spec_from_file_location("gen_ffi", os.path.join(ROOT, "integration", "rust", "gen_ffi.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    hdr = g.parse_header()
    rst = g.parse_rust(os.path.join(ROOT, "integration", "rust", "hip_ffi.rs"))
    h_funcs = {name: params for name, params, _ in hdr[0]}
    r_funcs = {name: params for name, params, _ in rst[0]}
    name = "pandrs_hip_grouped"
    assert re.search(r"^int32_t\s*%s\s*\(" % name, header, re.M)
    assert name in built.SYMBOLS and name in h_funcs and name in r_funcs
    hp, rp, cp = h_funcs[name], r_funcs[name], built.SYMBOLS[name][1]
    assert len(hp) == len(rp) == len(cp) == len(PARAMS)
    assert [n for n, _ in hp] == PARAMS
    for (hn, ht), (rn, rt), ct in zip(hp, rp, cp):
        assert hn == rn and ht == rt, (hn, ht, rt)
        assert ("*" in ht) == (ct is built._P or ct.__name__.startswith("LP_")), (hn, ct)
    assert built.SYMBOLS[name][1][5] is C.c_int64
    for k, v in ENUM.items():
        assert hdr[3]["PANDRS_HIP_GROUPED_" + k] == v == rst[2]["PANDRS_HIP_GROUPED_" + k] == getattr(built, "GROUPED_" + k)
    capi = open(os.path.join(ROOT, "pandrs_amd", "csrc", "capi.hip")).read()
    assert 'catch (...) { return pandrs::on_exception("pandrs_hip_grouped"); }' in capi
    assert built.load().pandrs_hip_abi_version() == 1
    block = header[header.index("/* ---- the same folds and lags within groups"):header.index("typedef enum pandrs_hip_grouped_op")]
    for word in ("groupby_window.rs", "pandrs_hip_groupby_indices", "says which", "ascending row order", "+0.0", "-0.0", "gamma_k", "2^53",
                 "its own cells only", "ROW_NUMBER", "may be NULL", "r_{t - periods}", "periods < 0", "0x7FF8000000000000", "bit words",
                 "reduce-then-apply", "(head seen, value)", "gathers the column through rows[] once", "ballot words", "max-scan",
                 "start[j'] == start[j]", "kernel boundary", "scratch", "atomic ORs on 32-bit words", "bytewise", "grouped_tile_rows = ",
                 "grouped_blocks_per_cu = ", "TYPE_MISMATCH", "BELOW_THRESHOLD", "OUT_OF_MEMORY", "NOT_INITIALIZED", "INVALID_ARGUMENT",
                 "2^32 - 16384", "bytes per row", "PANDRS_HIP_PHASE_AGGREGATE", "grouped PROD", "group-wise fills", "grouped rank",
                 "grouped top-k", "group-wise windows"):
        assert word in block, word
    cum = header[header.index("/* ---- running folds and lagged differences of one numeric column"):header.index("typedef enum pandrs_hip_cum_op")]
    assert "pandrs_hip_grouped" in cum                                     # the cumulative block's out-of-scope list points here
    assert "grouped.hip" in open(os.path.join(ROOT, "pandrs_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "pandrs_amd", "csrc", "grouped.hip")).read()
    assert int(re.search(r"grouped_tile_rows = (\d+)", block).group(1)) == 2048 and "GRP_TILE = GRP_WAVES * GRP_WAVE_ROWS" in src
    assert "GRP_BLOCKS_PER_CU = %s;" % re.search(r"grouped_blocks_per_cu = (\d+)", block).group(1) in src
    assert "#pragma clang fp contract(off)" in src and "__fma" not in src and "fma(" not in src


def test_cpp_mirror_grouped_compiles_against_the_header(built):
    libdir = os.path.join(ROOT, "pandrs_amd")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grouped_tests")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "grouped_tests.cpp"), "-L" + libdir, "-lpandrs_hip",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert "test_errors_before_any_device_call" in r.stdout and "0 failed checks" in r.stdout, r.stdout + r.stderr
        if r.returncode != 0:
            assert r.returncode == 1 and "no HIP device available" in r.stderr, r.stdout + r.stderr


def test_no_kernel_of_grouped_hip_uses_scratch(built):
    """grouped.hip compiled with the Makefile's flags: every kernel's code object metadata reports a private segment of 0 bytes
    and no spilled register (the per-load arrays of a tile are indexed by unrolled constants only)."""
    csrc = os.path.join(ROOT, "pandrs_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hipcc = re.search(r"^HIPCC \?= (\S+)", mk, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "grouped.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, "grouped.hip"), "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    kernels = re.findall(r"\.name:\s+(\S*grp_\w*kernel\S*)", text)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(kernels) >= 10 and len(kernels) == len(sizes) == len(re.findall(r"^\s+\.name:\s+\S+\s*$", text, re.M)), (kernels, sizes)    # every kernel of the file
    assert sizes and all(v == 0 for v in sizes), sizes
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text))
