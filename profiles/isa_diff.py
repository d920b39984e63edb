#!/usr/bin/env python3
"""Which kernels of two source trees compile to the same gfx950 instructions.

    profiles/isa_diff.py A B [--arch gfx950] [--jobs 8]

A and B are two checkouts of this repository (or any two trees with .hip files at the same relative paths).  Every
.hip file is compiled for the device only, to assembly, with the flags of csrc/Makefile; the assembly is split per
kernel, local labels are renumbered in order of first appearance (branch targets stay part of the text), the kernel's
own symbol is replaced, and per kernel one line says

    same | differs (n -> m instructions) | only in A (n instructions) | only in B (m instructions)

Kernels are paired by their demangled name without the parameter list.  A kernel whose name exists in one tree only is
paired with one left over in the other tree whose text is equal ("same ... (as <name in A>)": a rename, a template
parameter dropped) or, failing that, with the one of the same base name whose template arguments are a prefix of its own
or the other way round ("DIFFERS ... (was <name in A>)").  The comparison is of text: nothing here knows an instruction.
CPU only: it needs hipcc and c++filt, no device.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip", "--cuda-device-only", "-S"]


def hip_files(root):
    out = []
    for d, dirs, files in os.walk(root):
        dirs[:] = [x for x in dirs if not x.startswith(".") and x not in ("build", "_build", "_ref")]
        out += [os.path.relpath(os.path.join(d, f), root) for f in files if f.endswith(".hip")]
    return sorted(out)


def assemble(root, rel, arch, tmp):
    out = os.path.join(tmp, re.sub(r"\W", "_", os.path.abspath(root) + "/" + rel) + ".s")
    src = os.path.join(root, rel)
    r = subprocess.run([HIPCC, *FLAGS, "--offload-arch=" + arch, "-I", os.path.dirname(src), src, "-o", out],
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s: hipcc failed\n%s" % (src, r.stderr[-4000:]))
    return out


def kernels(path):
    """mangled name -> list of normalised lines (labels and instructions, comments and directives dropped)"""
    kernel_syms = set()
    text = open(path).read().split("\n")
    for line in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernel_syms.add(m.group(1))
    out, name, body = {}, None, []
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if name is None:
            if m and m.group(1) in kernel_syms:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = renumber([x.replace(name, "SELF") for x in body])
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.startswith(".L")):
            continue
        body.append(t)
    return out


def renumber(body):
    """local labels (.LBB3_17, .LJTI3_0, .Ltmp12 ...) -> .L<kind>#<k>, k = order of first appearance in the kernel"""
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), ".L%s#%d" % (m.group(1), len(seen)))

    return [re.sub(r"\.L([A-Za-z_]+)\d+(?:_\d+)?", sub, x) for x in body]


def strip_params(d):
    """'void ns::(anonymous namespace)::k<4, 8>(char const*, ...)' -> 'ns::(anonymous namespace)::k<4, 8>': the TRAILING
    parameter list only, found by matching parentheses from the end"""
    d = d.strip()
    if d.endswith(")"):
        depth = 0
        for i in range(len(d) - 1, -1, -1):
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                d = d[:i]
                break
    return d[5:] if d.startswith("void ") else d


def demangle(names):
    """mangled -> demangled name without the parameter list; two symbols that end up with one name keep their mangled names"""
    names = list(names)
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {n: strip_params(d) for n, d in zip(names, r)}
    for n, d in list(out.items()):
        if list(out.values()).count(d) > 1:
            out[n] = n
    return out


def base_and_args(name):
    """'afq::k_decode_par<4, 8, true>' -> ('afq::k_decode_par', ['4', '8', 'true'])"""
    m = re.match(r"^(.*?)<(.*)>$", name)
    return (m.group(1), [x.strip() for x in m.group(2).split(",")]) if m else (name, [])


def sibling(name, left):
    """the one kernel of `left` with name's base name whose template arguments are a prefix of name's, or name's of its"""
    b, a = base_and_args(name)
    hits = [m for m in left if base_and_args(m)[0] == b and
            (lambda x: x[:len(a)] == a or a[:len(x)] == x)(base_and_args(m)[1])]
    return hits[0] if len(hits) == 1 else None


def n_instr(body):
    return sum(1 for x in body if not x.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("A")
    ap.add_argument("B")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    fa, fb = hip_files(a.A), hip_files(a.B)
    tally = {"same": 0, "differs": 0, "only in A": 0, "only in B": 0}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        asm = {(root, rel): ex.submit(assemble, root, rel, a.arch, tmp) for root, fs in ((a.A, fa), (a.B, fb)) for rel in fs}
        for rel in sorted(set(fa) | set(fb)):
            print("== " + rel)
            ka = kernels(asm[(a.A, rel)].result()) if rel in fa else {}
            kb = kernels(asm[(a.B, rel)].result()) if rel in fb else {}
            da, db = demangle(ka), demangle(kb)
            A = {da[k]: v for k, v in ka.items()}
            B = {db[k]: v for k, v in kb.items()}
            left_a = {n: v for n, v in A.items() if n not in B}
            for n in sorted(set(A) & set(B)):
                if A[n] == B[n]:
                    tally["same"] += 1
                    print("  same     %s" % n)
                else:
                    tally["differs"] += 1
                    print("  DIFFERS  %s (%d -> %d instructions)" % (n, n_instr(A[n]), n_instr(B[n])))
            left_b = sorted(set(B) - set(A))
            for n in list(left_b):   # equal text under another name
                twin = next((m for m in sorted(left_a) if left_a[m] == B[n]), None)
                if twin is not None:
                    del left_a[twin]
                    left_b.remove(n)
                    tally["same"] += 1
                    print("  same     %s  (as %s in A)" % (n, twin))
            for n in left_b:   # then the same kernel with template arguments added or dropped
                sib = sibling(n, sorted(left_a))
                if sib is not None:
                    tally["differs"] += 1
                    print("  DIFFERS  %s  (was %s) (%d -> %d instructions)" % (n, sib, n_instr(left_a[sib]), n_instr(B[n])))
                    del left_a[sib]
                else:
                    tally["only in B"] += 1
                    print("  only in B  %s (%d instructions)" % (n, n_instr(B[n])))
            for n in sorted(left_a):
                tally["only in A"] += 1
                print("  only in A  %s (%d instructions)" % (n, n_instr(left_a[n])))
    print("== " + ", ".join("%s: %d" % kv for kv in tally.items()))


if __name__ == "__main__":
    main()
