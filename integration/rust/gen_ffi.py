#!/usr/bin/env python3
"""Generates hip_ffi.rs (the `extern "C"` block + #[repr(C)] types a PandRS maintainer adds as src/gpu/hip_ffi.rs)
from include/pandrs_hip.h, and parses both for tests/test_rust_shim.py.  No Rust toolchain exists in the build
image, so the generated file is never compiled here; the test checks it against the header mechanically
(every function: name, arity, parameter types, return type; every struct: field names, types, order)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "pandrs_hip.h")

SCALARS = {"int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "uint32_t": "u32", "uint8_t": "u8", "double": "f64",
           "void": "core::ffi::c_void", "char": "core::ffi::c_char"}
STRUCTS = {"pandrs_hip_ctx": "PandrsHipCtx", "pandrs_hip_comm": "PandrsHipComm", "pandrs_hip_column": "PandrsHipColumn",
           "pandrs_hip_transport": "PandrsHipTransport",
           "pandrs_hip_agg_spec": "PandrsHipAggSpec", "pandrs_hip_config": "PandrsHipConfig",
           "pandrs_hip_timings": "PandrsHipTimings", "pandrs_hip_column_stats": "PandrsHipColumnStats",
           "pandrs_hip_window_spec": "PandrsHipWindowSpec", "pandrs_hip_window_quantile_spec": "PandrsHipWindowQuantileSpec",
           "pandrs_hip_describe_stats": "PandrsHipDescribeStats", "pandrs_hip_distinct_info": "PandrsHipDistinctInfo",
           "pandrs_hip_pivot_info": "PandrsHipPivotInfo", "pandrs_hip_moments_stats": "PandrsHipMomentsStats"}
OPAQUE = ("pandrs_hip_ctx", "pandrs_hip_comm")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def rust_type(ctype):
    """C parameter / field type (without the name) -> Rust type."""
    t = " ".join(ctype.replace("*", " * ").split())
    m = re.fullmatch(r"(const )?(\w+)((?: \*(?: const)?)*)", t)
    if not m:
        raise ValueError("cannot map C type %r" % ctype)
    const0, base, stars = m.group(1), m.group(2), m.group(3).split("*")[1:]
    r = SCALARS.get(base) or STRUCTS.get(base)
    if r is None:
        raise ValueError("unknown base type %r" % base)
    # innermost pointer first: `const T *` -> *const T; a `* const` level is a const POINTER, its pointee mutability
    # comes from the level before it
    quals = [bool(const0)] + ["const" in s for s in stars]      # quals[i] = constness of level i's pointee
    for i in range(len(stars)):
        r = ("*const " if quals[i] else "*mut ") + r
    return r


def parse_header(path=HEADER):
    text = strip_comments(open(path).read())
    funcs = []
    for m in re.finditer(r"^(int32_t|const char \*)\s*(pandrs_hip_\w+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        ret = "i32" if m.group(1) == "int32_t" else "*const core::ffi::c_char"
        params = []
        body = " ".join(m.group(3).split())
        if body != "void":
            for p in body.split(","):
                p = p.strip()
                arr = re.fullmatch(r"(.*?)(\w+)\[(\d+)\]", p)              # `double out[4]` decays to a pointer
                if arr:
                    ctype, name = arr.group(1).strip() + " *", arr.group(2)
                else:
                    mm = re.fullmatch(r"(.*?)(\w+)", p)
                    ctype, name = mm.group(1).strip(), mm.group(2)
                params.append((name, rust_type(ctype)))
        funcs.append((m.group(2), params, ret))
    structs = {}
    for m in re.finditer(r"typedef struct (pandrs_hip_\w+) \{(.*?)\} \1;", text, re.S):
        fields = []
        for line in m.group(2).split(";"):
            line = " ".join(line.split())
            if not line:
                continue
            fp = re.fullmatch(r"(\w+) \( ?\* ?(\w+) ?\) ?\((.*)\)", line)      # `int32_t (*all_gather)(void *user, ...)`: a callback
            if fp:
                args = []
                for a in fp.group(3).split(","):
                    am = re.fullmatch(r"(.*?)(\w+)", a.strip())
                    args.append(rust_type(am.group(1).strip()))
                fields.append((fp.group(2), 'Option<unsafe extern "C" fn(%s) -> %s>' % (", ".join(args), rust_type(fp.group(1)))))
                continue
            names = [x.strip() for x in line.split(",")]             # `int64_t min_i64, max_i64`
            first = re.fullmatch(r"(.*?)(\w+)(\[[\w ]+\])?", names[0])
            ctype = first.group(1).strip()
            for j, nm in enumerate(names):
                mm = first if j == 0 else re.fullmatch(r"()(\w+)(\[[\w ]+\])?", nm)
                rt = rust_type(ctype)
                if mm.group(3):
                    rt = "[%s; %s]" % (rt, mm.group(3).strip("[]"))
                fields.append((mm.group(2), rt))
        structs[m.group(1)] = fields
    consts = dict((k, int(v)) for k, v in re.findall(r"#define (PANDRS_HIP_\w+) (\d+)\b", text))
    enums = dict((k, int(v)) for k, v in re.findall(r"\b(PANDRS_HIP_[A-Z0-9_]+) = (\d+)", text))
    return funcs, structs, consts, enums


def generate():
    funcs, structs, consts, enums = parse_header()
    out = ["// hip_ffi.rs — GENERATED by integration/rust/gen_ffi.py from include/pandrs_hip.h; do not edit by hand.",
           "// The `extern \"C\"` surface of libpandrs_hip.so for PandRS: add as src/gpu/hip_ffi.rs behind cfg(hip_available)",
           "// (build.rs fragment beside this file).  Every entry point's reference seam is cited in the header.",
           "#![allow(non_camel_case_types, dead_code)]", ""]
    for k in sorted(consts):
        out.append("pub const %s: usize = %d;" % (k, consts[k]))
    for k in sorted(enums, key=lambda k: (k.rsplit("_", 1)[0], enums[k])):
        out.append("pub const %s: i32 = %d;" % (k, enums[k]))
    out.append("")
    for cname in OPAQUE:
        out += ["#[repr(C)]", "pub struct %s { _private: [u8; 0] }" % STRUCTS[cname], ""]
    for cname, fields in structs.items():
        out += ["#[repr(C)]", "#[derive(Clone, Copy)]", "pub struct %s {" % STRUCTS[cname]]
        for name, rt in fields:
            rt = re.sub(r"PANDRS_HIP_\w+", lambda m: m.group(0), rt)
            out.append("    pub %s: %s," % (name, rt))
        out += ["}", ""]
    out.append('#[link(name = "pandrs_hip")]')
    out.append('extern "C" {')
    for name, params, ret in funcs:
        args = ", ".join("%s: %s" % (("r#%s" % n) if n in ("in", "type", "ref", "box") else n, t) for n, t in params)
        out.append("    pub fn %s(%s) -> %s;" % (name, args, ret))
    out.append("}")
    return "\n".join(out) + "\n"


def parse_rust(path):
    text = open(path).read()
    funcs = []
    for m in re.finditer(r"pub fn (pandrs_hip_\w+)\((.*?)\) -> ([^;]+);", text):
        params = []
        if m.group(2).strip():
            for p in m.group(2).split(", "):
                n, t = p.split(": ", 1)
                params.append((n.replace("r#", ""), t))
        funcs.append((m.group(1), params, m.group(3).strip()))
    structs = {}
    for m in re.finditer(r"pub struct (\w+) \{\n(.*?)\n\}", text, re.S):
        fields = re.findall(r"^\s*pub (\w+): (.*),$", m.group(2), re.M)
        structs[m.group(1)] = fields
    consts = dict((k, int(v)) for k, v in re.findall(r"pub const (PANDRS_HIP_\w+): \w+ = (\d+);", text))
    return funcs, structs, consts


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip_ffi.rs")
    open(path, "w").write(generate())
    print("wrote", path)
