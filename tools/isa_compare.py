"""Device code of two source trees, kernel by kernel: python tools/isa_compare.py [--rename OLD=NEW ...] [--lines] PARENT_CSRC BRANCH_CSRC file.hip ...

Each file is compiled with the Makefile's flags plus --cuda-device-only -S for gfx950.  Per kernel: "identical" (same
instructions, registers and kernel descriptor; basic-block labels compared without their per-file function number, the
kernel's own symbol without its name), "reordered" (same descriptor and the same count of every mnemonic) or "changed" (with
the descriptor's VGPR / SGPR / scratch / LDS numbers of both builds); "added" / "removed" for a kernel that only one tree has.
--rename OLD=NEW: the parent's kernel OLD (as this tool prints it) is compared with the branch's NEW.
--lines: the descriptor's numbers and the instruction count of every kernel, and for a changed kernel where its mnemonic
sequence differs and, when at most 40 lines differ at all (the rest of a longer list is register renumbering), those lines."""
import argparse
import collections
import difflib
import re
import subprocess
import sys
import tempfile

FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -munsafe-fp-atomics -fPIC "
         "-mllvm -amdgpu-kernarg-preload-count=16 --cuda-device-only -S").split()
DESC = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(csrc, name):
    """-> {demangled kernel: (body lines, descriptor dict)}"""
    with tempfile.NamedTemporaryFile(suffix=".s") as out:
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, name, "-o", out.name], cwd=csrc)
        text = open(out.name).read()
    found = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)\n\s*\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        own = re.compile(r"\b%s\b" % re.escape(m.group(1)))
        body = [own.sub("KERNEL", re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip())) for l in m.group(2).splitlines()]
        body = [l for l in body if l and "__hip_cuid_" not in l]
        desc = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(3)))
        found[m.group(1)] = (body, desc)
    nice = subprocess.run(["c++filt"], input="\n".join(found), capture_output=True, text=True).stdout.split("\n")
    short = [re.sub(r"\(.*\)$", "", n) for n in nice]  # without the parameter list: a kernel whose parameter types change keeps its row
    return {(s if short.count(s) == 1 else n): v for s, n, v in zip(short, nice, found.values())}


def main(parent, branch, files, rename, lines):
    for name in files:
        a, b = kernels(parent, name), kernels(branch, name)
        back = {rename[k]: k for k in a if k in rename}
        a = {rename.get(k, k): v for k, v in a.items()}
        print(name)
        for k in list(a) + [k for k in b if k not in a]:
            title = "%s (parent: %s)" % (k, back[k]) if k in back else k
            if k not in b or k not in a:
                print("  %-10s %s" % ("removed" if k in a else "added", title))
                continue
            (ba, da), (bb, db) = a[k], b[k]
            mn = lambda body: collections.Counter(l.split()[0] for l in body if not l.endswith(":") and not l.startswith("."))
            state = "identical" if ba == bb and da == db else "reordered" if da == db and mn(ba) == mn(bb) else "changed"
            print("  %-10s %s" % (state, title))
            if state == "changed" or lines:
                print("             parent: vgpr/sgpr/scratch/lds %s  instructions %d" % ("/".join(da.get(f, "?") for f in DESC), sum(mn(ba).values())))
                print("             branch: vgpr/sgpr/scratch/lds %s  instructions %d" % ("/".join(db.get(f, "?") for f in DESC), sum(mn(bb).values())))
            if state != "identical" and lines:
                for f in sorted(set(da) | set(db)):
                    if da.get(f) != db.get(f):
                        print("             descriptor %s: %s -> %s" % (f, da.get(f), db.get(f)))
                ops = lambda body: [l.split()[0] for l in body]
                sm = difflib.SequenceMatcher(None, ops(ba), ops(bb), autojunk=False)
                print("             mnemonic sequences: ratio %.4f" % sm.ratio())
                for tag, i1, i2, j1, j2 in sm.get_opcodes():
                    if tag != "equal":
                        print("             %s parent %d: %s | branch %d: %s" % (tag, i1 + 1, "; ".join(ba[i1:i2]), j1 + 1, "; ".join(bb[j1:j2])))
                diff = list(difflib.unified_diff(ba, bb, "parent", "branch", n=0, lineterm=""))
                changed = sum(1 for l in diff[2:] if l[0] in "+-")
                print("             lines that differ in any way, registers included: %d removed or added" % changed)
                for l in diff if changed <= 40 else []:
                    print("             " + l)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    main(a.parent, a.branch, a.files, dict(r.split("=") for r in a.rename), a.lines)
