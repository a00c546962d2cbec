#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds kernel by kernel (no GPU needed).

Each side is a list of device assembly files (`.s`, from
`hipcc --offload-arch=gfx950 --cuda-device-only -S`) or `.hip` sources, which
are compiled that way first (in parallel, with the Makefile's flags).  For every
kernel the instruction stream (comments dropped, local labels renumbered in
order of appearance) and the kernel descriptor (the `.amdhsa_*` lines: VGPR,
SGPR, LDS and scratch sizes among them) must be equal, the two sides must define
the same set of kernels, and no side may define a kernel twice.  Kernels are
matched by their demangled names without `(anonymous namespace)::`, so moving a
kernel or the type of one of its arguments in or out of an anonymous namespace
is no difference (names are demangled with binutils' `c++filt`).  Exit status 0
when all of that holds.

    python scripts/isadiff.py --a /path/to/old/csrc/hip/stft_kernels.hip \\
        --b vv-dsp_amd/csrc/hip/stft_*.hip vv-dsp_amd/csrc/hip/istft_kernels.hip
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCAL = re.compile(r"\.L(?:BB|func_end|func_begin|tmp)[0-9_]*[0-9]")


def assemble(src, tmp, hipcc, arch):
    """device assembly of one .hip source (the Makefile's HIPFLAGS)"""
    out = os.path.join(tmp, "%s_%s.s" % (os.path.basename(src), abs(hash(os.path.abspath(src)))))
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vv-dsp_amd", "csrc", "host")]
    subprocess.run([hipcc, "--offload-arch=" + arch, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", *inc,
                    "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
    return out


def kernels(path, rename=()):
    """{kernel: (instruction lines, descriptor lines)} of one assembly file"""
    text = subprocess.run(["c++filt"], input=open(path).read(), capture_output=True, text=True, check=True).stdout
    for old, new in rename:
        text = re.sub(r"\b%s\b" % re.escape(old), new, text)
    lines = text.replace("(anonymous namespace)::", "").split("\n")
    desc, cur = {}, None
    for ln in lines:   # descriptors first: they name the kernels
        t = ln.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t[len(".amdhsa_kernel "):].split(";")[0].strip()
            desc[cur] = []
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and t:
            desc[cur].append(" ".join(t.split(";")[0].split()))
    body, cur, names = {}, None, {}
    for ln in lines:
        t = ln.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":") and t[:-1] in desc:
            cur, names = t[:-1], {}
            body[cur] = []
            continue
        if cur is None:
            continue
        if t.startswith(".section"):   # not an instruction (and it carries the mangled name)
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
            continue
        # local labels numbered by first appearance inside the kernel
        t = LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), " ".join(t.split()))
        body[cur].append(t)
    return {k: (body.get(k, []), desc[k]) for k in desc}


def side(paths, tmp, hipcc, arch, rename=()):
    with ThreadPoolExecutor(max_workers=8) as ex:
        asm = list(ex.map(lambda p: assemble(p, tmp, hipcc, arch) if p.endswith(".hip") else p, paths))
    allk, dup = {}, []
    for p, a in zip(paths, asm):
        for k, v in kernels(a, rename).items():
            if k in allk:
                dup.append((k, allk[k][2], p))
            allk[k] = (*v, p)
    return allk, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, help="first build: .s or .hip files")
    ap.add_argument("--b", nargs="+", required=True, help="second build: .s or .hip files")
    ap.add_argument("--hipcc", default=os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("-v", action="store_true", help="print the first differing line of each kernel")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="a type renamed between the builds: OLD becomes NEW in side a's demangled names")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        A, dupa = side(args.a, tmp, args.hipcc, args.arch, [r.split("=", 1) for r in args.rename])
        B, dupb = side(args.b, tmp, args.hipcc, args.arch)
    bad = 0
    for name, dup in (("a", dupa), ("b", dupb)):
        for k, p, q in dup:
            print("TWICE in %s: %s (%s, %s)" % (name, k, p, q))
            bad += 1
    for k in sorted(set(A) - set(B)):
        print("ONLY in a: %s (%s)" % (k, A[k][2]))
        bad += 1
    for k in sorted(set(B) - set(A)):
        print("ONLY in b: %s (%s)" % (k, B[k][2]))
        bad += 1
    for k in sorted(set(A) & set(B)):
        (ia, da, pa), (ib, db, pb) = A[k], B[k]
        if da != db:
            print("DESCRIPTOR differs: %s (%s)" % (k, pb))
            for x, y in zip(da, db):
                if x != y:
                    print("    a: %s\n    b: %s" % (x, y))
            bad += 1
        if ia != ib:
            print("CODE differs: %s (%s): %d vs %d lines" % (k, pb, len(ia), len(ib)))
            if args.v:
                i = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
                print("    line %d\n    a: %s\n    b: %s" % (i, ia[i] if i < len(ia) else "-", ib[i] if i < len(ib) else "-"))
            bad += 1
    print("%d kernels in a, %d in b, %d instruction lines compared, %d differences"
          % (len(A), len(B), sum(len(A[k][0]) for k in set(A) & set(B)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
