#!/usr/bin/env python3
"""Device code of two trees, function by function (no GPU needed: hipcc cross-compiles).

    python tools/device_code_cmp.py PARENT/proof_systems_amd/csrc proof_systems_amd/csrc poly.hip ipa.hip ...

Per file and tree: hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S.  Every function's instruction stream (comments, the __hip_cuid_
lines and the function ordinal of local labels stripped) and every kernel descriptor are compared; functions are matched by their demangled name
WITHOUT the parameter list, so a kernel whose signature changed is still compared with its predecessor.  One line per file, then one per function that
differs: registers, LDS, scratch and instruction counts of both.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
FILT = "/opt/rocm/llvm/bin/llvm-cxxfilt" if os.path.exists("/opt/rocm/llvm/bin/llvm-cxxfilt") else "c++filt"
KEYS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def assemble(csrc, name, out):
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(csrc, name), "-o", out])
    return open(out).read().splitlines()


def functions(lines):
    """mangled name -> (instruction lines, descriptor lines)"""
    body, desc, cur, kern, is_fn = {}, {}, None, None, set()
    for raw in lines:
        line = re.sub(r"\s*;.*$", "", raw).strip()
        if not line or "__hip_cuid_" in line:
            continue
        line = re.sub(r"(\.?L?BB|\.Lfunc_end|\.LJTI|\.Ltmp|\.Lpost_getpc)\d+", r"\1N", line)
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            is_fn.add(m.group(1))
        m = re.match(r"(\S+):$", line)
        if m and m.group(1) in is_fn and m.group(1) not in body:
            cur = m.group(1); body[cur] = []
            continue
        if line.startswith(".Lfunc_endN"):
            cur = None
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern = m.group(1); desc[kern] = []
            continue
        if line == ".end_amdhsa_kernel":
            kern = None
        if kern:
            desc[kern].append(line)
        elif cur and not line.startswith("."):
            body[cur].append(line)
    return body, desc


def short_names(mangled):
    out = subprocess.run([FILT], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.splitlines()
    return {m: re.sub(r"^void ", "", d.replace("(anonymous namespace)", "{anonymous}")).split("(")[0] for m, d in zip(mangled, out)}


def table(csrc, name, tmp, tag):
    body, desc = functions(assemble(csrc, name, os.path.join(tmp, tag + "_" + name + ".s")))
    names = short_names(list(body))
    return {names[m]: (body[m], desc.get(m)) for m in body}


def figures(desc):
    d = dict(l.split(None, 1) for l in desc or [])
    return " ".join("%s=%s" % (k.replace("_fixed_size", "").replace("next_free_", ""), d.get(".amdhsa_" + k, "-")) for k in KEYS)


def main():
    parent, change, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        jobs = {f: (pool.submit(table, parent, f, tmp, "a"), pool.submit(table, change, f, tmp, "b")) for f in files}
        for f in files:
            a, b = jobs[f][0].result(), jobs[f][1].result()
            same_body = sum(1 for k in a if k in b and a[k][0] == b[k][0])
            same_desc = sum(1 for k in a if k in b and a[k][1] == b[k][1])
            print("%-20s functions %3d / %3d   same instructions %3d   same descriptor %3d   only in one tree: %s"
                  % (f, len(a), len(b), same_body, same_desc, sorted(set(a) ^ set(b)) or "-"))
            for k in sorted(a):
                if k in b and (a[k][0] != b[k][0] or a[k][1] != b[k][1]):
                    print("    %s\n        parent %5d instructions  %s\n        change %5d instructions  %s"
                          % (k, len(a[k][0]), figures(a[k][1]), len(b[k][0]), figures(b[k][1])))


if __name__ == "__main__":
    main()
