#!/usr/bin/env python3
"""Writes tests/golden/reference_shim_facts.json from a checkout of the reference (cool-japan/pandrs):

    python tests/golden/make_reference_facts.py <path to the reference checkout>

tests/test_rust_shim.py checks the Rust shim and its seam patches (integration/rust/) against the reference without
the reference being present.  What it needs is stored here as facts, never as source text:
  - declared: the fn names and pub / pub(crate) field names of the files hip_shim.rs reaches into;
  - pub_use / pub_items / enum_variants / error_string_variants: what the modules the shim imports from re-export or
    declare, by name;
  - patch_targets: for every file a seam patch touches, its line count, the SHA-256 of the reference lines under each
    hunk's old side, its bracket counts (outside comments and literals) and the crate types its names resolve to.
Before writing, the patches are applied to a copy of the reference files with patch(1), and the facts are proven to
give what the tests' checks give on the patched files themselves.
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_rust_shim as T  # noqa: E402

MEMBER_FILES = ["src/column/int64_column.rs", "src/column/float64_column.rs", "src/column/string_column.rs", "src/column/boolean_column.rs",
                "src/column/string_pool.rs", "src/core/column.rs", "src/core/error.rs", "src/gpu/mod.rs",
                "src/optimized/split_dataframe/core.rs", "src/optimized/split_dataframe/column_ops.rs",
                "src/optimized/split_dataframe/data_ops.rs", "src/optimized/split_dataframe/group/types.rs",
                "src/optimized/split_dataframe/join.rs", "src/optimized/split_dataframe/index.rs", "src/index/multi_index.rs",
                "src/optimized/dataframe/core.rs", "src/optimized/dataframe/operations.rs"]
EXPORTING = ["src/column/mod.rs", "src/index/mod.rs", "src/optimized/mod.rs"]
DECLARING = ["src/column/string_pool.rs", "src/core/error.rs", "src/gpu/mod.rs", "src/optimized/operations.rs"]


def read(ref, rel):
    with open(os.path.join(ref, rel)) as f:
        return f.read()


def pub_use(text):
    """name -> sorted origins (module path before the name, `self::` dropped) of every `pub use`."""
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"\bpub use ([\w:]+?)::(?:\{([^}]*)\}|(\w+))\s*;", text, re.S):
        origin = re.sub(r"^self::", "", m.group(1))
        for item in (m.group(2).split(",") if m.group(2) is not None else [m.group(3)]):
            name, _, alias = item.strip().partition(" as ")
            if name:
                path = (origin + "::" + name.strip()).split("::")
                out.setdefault((alias or path[-1]).strip(), set()).add("::".join(path[:-1]))
    return {k: sorted(v) for k, v in sorted(out.items())}


def main(ref):
    facts = {"about": "facts about the reference (cool-japan/pandrs) for tests/test_rust_shim.py: names and SHA-256 digests only; "
                      "written by tests/golden/make_reference_facts.py"}
    members = "\n".join(read(ref, f) for f in MEMBER_FILES)
    facts["declared"] = sorted(set(re.findall(r"\bfn (\w+)", members)) | set(re.findall(r"pub(?:\(crate\))? (\w+):", members)))
    facts["pub_use"] = {f: pub_use(read(ref, f)) for f in EXPORTING}
    facts["pub_items"] = {f: sorted(set(re.findall(r"\bpub (?:static ref|static|const|enum|struct|fn|type|trait) (\w+)", read(ref, f))))
                          for f in DECLARING}
    body = re.search(r"pub enum StringColumnOptimizationMode\s*\{([^}]*)\}", read(ref, "src/column/string_column.rs")).group(1)
    facts["enum_variants"] = {"StringColumnOptimizationMode": re.findall(r"^\s*(\w+),", re.sub(r"//[^\n]*", "", body), re.M)}
    facts["error_string_variants"] = sorted(set(re.findall(r"\b(\w+)\(String\)", read(ref, "src/core/error.rs"))))

    targets = {}
    for p in sorted(f for f in os.listdir(os.path.join(T.RUST, "patches")) if f.endswith(".patch")):
        rel, hunks = T._parse_patch(os.path.join(T.RUST, "patches", p))
        text = read(ref, rel)
        assert "hip_shim" not in text, rel       # every call into the shim comes from a patch
        lines = text.split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        targets[rel] = {"lines": len(lines),
                        "hunks": [{"old_start": h["old_start"], "old_len": h["old_len"],
                                   "sha256": T._lines_digest(lines[h["old_start"] - 1:h["old_start"] - 1 + h["old_len"]])} for h in hunks],
                        "brackets": T._bracket_counts(text),
                        "scope": {k: v for k, v in T._names_in_scope(text, T._module_of(rel)).items() if k in T._CRATE_TYPES}}
    facts["patch_targets"] = targets

    # the facts stand in for the reference: prove it on the patched files themselves
    reconstructed = T._patched(facts)
    with tempfile.TemporaryDirectory() as d:
        for rel in T.PATCHED:
            os.makedirs(os.path.join(d, os.path.dirname(rel)), exist_ok=True)
            shutil.copy(os.path.join(ref, rel), os.path.join(d, rel))
        for p in sorted(f for f in os.listdir(os.path.join(T.RUST, "patches")) if f.endswith(".patch")):
            r = subprocess.run(["patch", "-p1", "-i", os.path.join(T.RUST, "patches", p)], cwd=d, capture_output=True, text=True)
            assert r.returncode == 0 and "offset" not in r.stdout and "fuzz" not in r.stdout, p + "\n" + r.stdout + r.stderr
        call = r"hip_shim::(\w+)\s*\(([^;{]*?)\)\s*[{)]"
        for rel in T.PATCHED:
            text = read(d, rel)
            new_sides, brackets, scope = reconstructed[rel]
            assert [m.groups() for m in re.finditer(call, text, re.S)] == [m.groups() for m in re.finditer(call, new_sides, re.S)], rel
            assert re.findall(r"hip_shim::(\w+)\s*\(", text) == re.findall(r"hip_shim::(\w+)\s*\(", new_sides), rel
            assert brackets == T._bracket_counts(text), rel
            assert scope == {k: v for k, v in T._names_in_scope(text, T._module_of(rel)).items() if k in T._CRATE_TYPES}, rel

    with open(os.path.join(ROOT, "tests", "golden", "reference_shim_facts.json"), "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
