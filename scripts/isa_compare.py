#!/usr/bin/env python3
"""Device ISA of every kernel in two trees of this repository, compared kernel by kernel.  No GPU needed.

    python3 scripts/isa_compare.py <parent-tree> <this-tree> [-o profiles/isa_compare_X.txt] [--title "..."]

Every .hip under cdv_slam_amd/csrc of both trees is built with the flags the tree's own Makefile gives its objects plus
--cuda-device-only -S.  Per kernel (keyed by its mangled name; the file it lives in is a column, so a kernel that moved to
another file is still compared) four things must match: the body, the .set resource lines, the .amdhsa_kernel block and the
code-object metadata entry.  Exit status 1 when a kernel differs, was added or was removed.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("cdv_slam_amd", "csrc")


def device_asm_command(csrc, src, out):
    """The Makefile's own compile line for build/<src>.o (a dry run prints it), turned into a device-only -S build."""
    lines = subprocess.check_output(["make", "-C", csrc, "-n", "-B", "--no-print-directory", "ARCH=gfx950", "build/%s.o" % src],
                                    text=True).splitlines()
    line = [ln for ln in lines if " -c " in ln][-1]
    argv = shlex.split(line)
    i = argv.index("-c")
    return argv[:i] + ["--cuda-device-only", "-S", src, "-o", out]


def build_tree(tree, tmp, jobs):
    csrc = os.path.join(tree, CSRC)
    srcs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))

    def one(src):
        out = os.path.join(tmp, src + ".s")
        subprocess.run(device_asm_command(csrc, src, out), cwd=csrc, check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            return src, f.read()

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return dict(ex.map(one, srcs))


def renumber(text):
    """Basic-block and temporary labels numbered by first appearance (also where comments name them); blanks collapsed."""
    seen = {}

    def label(m):   # (comments name a block without the .L: "in Loop: Header=BB5_7")
        return m.group(1) + m.group(2) + str(seen.setdefault(m.group(2) + m.group(3), len(seen)))

    text = re.sub(r"(\.L|\b)(BB|tmp|func_begin|func_end|JTI|CPI)(\d+(?:_\d+)*)", label, text)
    text = re.sub(r"%bb\.\d+", lambda m: "%%bb.%d" % seen.setdefault(m.group(0), len(seen)), text)
    return "\n".join(re.sub(r"[ \t]+", " ", ln).strip() for ln in text.splitlines())


def kernels_of(asm):
    """{mangled name: (body, set lines, kernel descriptor, metadata entry)} of one device assembly file."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    meta = {}
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", asm, re.M | re.S)
    if m:
        for entry in re.split(r"^  - ", m.group(1), flags=re.M)[1:]:
            nm = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
            if nm:
                meta[nm.group(1)] = entry
    out = {}
    for n in names:
        q = re.escape(n)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % q, asm, re.M | re.S)
        sets = re.findall(r"^\s*\.set\s+%s\.[^\n]*" % q, asm, re.M)
        kd = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)^\s*\.end_amdhsa_kernel" % q, asm, re.M | re.S)
        assert body and sets and kd and n in meta, "could not find every part of kernel %s" % n
        out[n] = (renumber(body.group(1)), renumber("\n".join(sets)), renumber(kd.group(1)), renumber(meta[n]))
    return out


def demangle(texts):
    """Every _Z... symbol in the texts replaced by its demangled form (left as it is where c++filt does not know it)."""
    filt = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/bin/llvm-cxxfilt") if os.path.exists(p)), "c++filt")
    syms = sorted({m for t in texts for m in re.findall(r"\b_Z\w+", t)})
    res = subprocess.run([filt], input="\n".join(syms), text=True, capture_output=True, check=True).stdout.splitlines()
    table = dict(zip(syms, res))
    return [re.sub(r"\b_Z\w+", lambda m: table.get(m.group(0), m.group(0)), t) for t in texts]


def collect(tree_asm):
    """{mangled name: (file, parts)} over all files of a tree."""
    out = {}
    for src, asm in tree_asm.items():
        for n, parts in kernels_of(asm).items():
            assert n not in out, "kernel %s in %s and %s" % (n, out[n][0], src)
            out[n] = (src, parts)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("change")
    ap.add_argument("-o", "--out", default=None, help="write the table here (default: standard output)")
    ap.add_argument("--title", default="before and after the change", help="ends the first line of the table's header")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        before = collect(build_tree(a.parent, t0, a.jobs))
        after = collect(build_tree(a.change, t1, a.jobs))
    PARTS = ("body", ".set", ".amdhsa_kernel", "metadata")
    rows, bad = [], 0
    names = sorted(set(before) | set(after))
    # demangled, so that a renamed type in a signature shows as such and not as a difference of every reference to it
    flat_b = [p for n in names for p in (before[n][1] if n in before else ("",) * 4)]
    flat_a = [p for n in names for p in (after[n][1] if n in after else ("",) * 4)]
    texts = demangle(names + flat_b + flat_a)
    shown, flat_b, flat_a = texts[:len(names)], texts[len(names):len(names) + len(flat_b)], texts[len(names) + len(flat_b):]
    for i, n in enumerate(names):
        fb = before[n][0] if n in before else None
        fa = after[n][0] if n in after else None
        if fb is None or fa is None:
            status = "added" if fb is None else "removed"
        else:
            diff = [PARTS[k] for k in range(4) if flat_b[4 * i + k] != flat_a[4 * i + k]]
            status = "identical" if not diff else "DIFFERS(" + ",".join(diff) + ")"
        bad += status != "identical"
        file_col = (fb or fa) if fb == fa or fb is None or fa is None else "%s -> %s" % (fb, fa)
        rows.append(((fb or fa), n, file_col, status, shown[i].strip()))
    rows.sort(key=lambda r: (r[0], r[1]))
    ver = "unknown"
    try:
        ver = open("/opt/rocm/.info/version").read().strip().split("-")[0]
    except OSError:
        pass
    moved = {}
    for r in rows:
        if " -> " in r[2]:
            moved[r[2]] = moved.get(r[2], 0) + 1
    w0 = max(len(r[2]) for r in rows) + 2
    w1 = max(len(r[3]) for r in rows) + 2
    head = [
        "# Device ISA of every kernel, " + a.title,
        "# Each .hip built with the Makefile's CXXFLAGS plus -x hip --cuda-device-only -S (gfx950, ROCm %s), at the parent commit" % ver,
        "# and after the change (scripts/isa_compare.py).  Compared per kernel: the body (label to .Lfunc_end; basic-block and",
        "# temporary labels renumbered, also where comments name them; runs of blanks collapsed; symbols demangled), the .set",
        "# resource lines (VGPR / AGPR / SGPR counts, scratch), the .amdhsa_kernel block (LDS, scratch, kernarg size) and the",
        "# kernel's code-object metadata entry (argument offsets, .vgpr_count, .sgpr_count, segment sizes).",
        "# %d kernels before, %d after, %s." % (len(before), len(after), "all identical" if not bad else "%d NOT identical" % bad),
    ]
    if moved:
        head.append("# Moved: " + ", ".join("%d %s" % (c, k) for k, c in sorted(moved.items())) + ".")
    head.append("# %s%s%s" % ("file".ljust(w0 - 2), "status".ljust(w1), "kernel"))
    text = "\n".join(head + ["%s%s%s" % (r[2].ljust(w0), r[3].ljust(w1), r[4]) for r in rows]) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        print("%d kernels before, %d after, %d not identical -> %s" % (len(before), len(after), bad, a.out))
    else:
        sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
