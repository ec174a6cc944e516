"""Device code of two source trees, kernel by kernel: python tools/isa_compare.py PARENT_CSRC BRANCH_CSRC file.hip ...

Each file is compiled with the Makefile's flags plus --cuda-device-only -S for gfx950.  Per kernel: "identical" (same
instructions, registers and kernel descriptor; basic-block labels compared without their per-file function number),
"reordered" (same descriptor and the same count of every mnemonic) or "changed" (with the descriptor's VGPR / SGPR /
scratch / LDS numbers of both builds); "added" / "removed" for a kernel that only one tree has."""
import collections
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
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in m.group(2).splitlines()]
        body = [l for l in body if l and "__hip_cuid_" not in l]
        desc = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(3)))
        found[m.group(1)] = (body, desc)
    nice = subprocess.run(["c++filt"], input="\n".join(found), capture_output=True, text=True).stdout.split("\n")
    short = [re.sub(r"\(.*\)$", "", n) for n in nice]  # without the parameter list: a kernel whose parameter types change keeps its row
    return {(s if short.count(s) == 1 else n): v for s, n, v in zip(short, nice, found.values())}


def main(parent, branch, files):
    for name in files:
        a, b = kernels(parent, name), kernels(branch, name)
        print(name)
        for k in list(a) + [k for k in b if k not in a]:
            if k not in b or k not in a:
                print("  %-10s %s" % ("removed" if k in a else "added", k))
                continue
            (ba, da), (bb, db) = a[k], b[k]
            mn = lambda body: collections.Counter(l.split()[0] for l in body if not l.endswith(":") and not l.startswith("."))
            state = "identical" if ba == bb and da == db else "reordered" if da == db and mn(ba) == mn(bb) else "changed"
            print("  %-10s %s" % (state, k))
            if state == "changed":
                print("             parent: vgpr/sgpr/scratch/lds %s  instructions %d" % ("/".join(da.get(f, "?") for f in DESC), sum(mn(ba).values())))
                print("             branch: vgpr/sgpr/scratch/lds %s  instructions %d" % ("/".join(db.get(f, "?") for f in DESC), sum(mn(bb).values())))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
