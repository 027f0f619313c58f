#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the HIP objects, object by object.

    scripts/device_code_diff.py BUILD_DIR_A BUILD_DIR_B [NAME ...]

For every object of the Makefile's HIP_NAMES (or the NAMEs given) the gfx950 code object is taken out of
DIR/NAME.o (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle) and three things are
compared: the sorted list of FUNC symbols, the disassembly (llvm-objdump -d --no-show-raw-insn
--no-leading-addr, after its file-name header) and llvm-readelf --notes.  Where the whole listing or the notes
differ, the kernels are compared one by one by symbol -- instructions, operands and encodings, without the
addresses and the padding between symbols, and each kernel's metadata entry -- which tells a change of order
from a change of code.
A host-side refactor of the launch files must come out "identical" (or "identical up to symbol order") for
every object.  Exit status 0: no object's device code differs.
"""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
HERE = os.path.dirname(os.path.abspath(__file__))


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def code_object(obj, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
        "--input=" + fat, "--output=" + co)
    return co


def facts(co):
    syms = sorted(l.split()[-1] for l in run(os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co).splitlines()
                  if len(l.split()) >= 8 and l.split()[3] == "FUNC")
    lines = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines()
    while lines and ("file format" in lines[0] or not lines[0].strip()):  # the header names the file
        lines.pop(0)
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    return syms, lines, notes.replace(co, "")


def per_symbol(lines):
    """each symbol's instructions, operands and encodings, without the addresses a move changes (branch
    targets are printed relative to their symbol)"""
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^<(.+)>:$", l)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and l.strip() not in ("", "..."):  # ("...": zero padding up to the next symbol)
            cur.append(re.sub(r"// [0-9A-F]{12}:", "//", l))
    return out


def note_parts(notes):
    """the metadata note with its per-kernel entries (each names its kernel) sorted"""
    head, kernels, tail = [], [], []
    for l in notes.splitlines():
        if re.match(r"^  - \.", l) and not tail:
            kernels.append([l])
        elif kernels and not tail and l.startswith("    "):
            kernels[-1].append(l)
        else:
            (tail if kernels else head).append(l)
    return head, sorted(kernels), tail


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a_dir, b_dir, names = sys.argv[1], sys.argv[2], sys.argv[3:]
    if not names:
        mk = open(os.path.join(HERE, "..", "generalsparse_amd", "csrc", "Makefile")).read()
        names = re.search(r"^HIP_NAMES := (.*)$", mk, re.M).group(1).split()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            sa, la, na = facts(code_object(os.path.join(a_dir, n + ".o"), tmp, "a_" + n))
            sb, lb, nb = facts(code_object(os.path.join(b_dir, n + ".o"), tmp, "b_" + n))
            what = []
            if sa != sb:
                what.append("FUNC symbols differ: only in A %s, only in B %s" % (sorted(set(sa) - set(sb))[:4], sorted(set(sb) - set(sa))[:4]))
            if la != lb:
                pa, pb = per_symbol(la), per_symbol(lb)
                diff = sorted(k for k in set(pa) | set(pb) if pa.get(k) != pb.get(k))
                what.append("code of %d symbols differs, e.g. %s" % (len(diff), diff[:2]) if diff else "symbol order")
            if na != nb:
                what.append("notes differ" if note_parts(na) != note_parts(nb) else "note order")
            same = all(w in ("symbol order", "note order") for w in what)
            bad += not same
            print("%-20s %4d FUNC  %s" % (n, len(sa), ("identical" + (" up to " + " and ".join(what) if what else "")) if same
                                          else "DIFFERENT: " + "; ".join(what)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
