"""Same machine code?  Compares the device assembly of two source trees kernel by kernel (no GPU needed).

    python tools/kernel_asm_diff.py OLD_CSRC NEW_CSRC [--jobs 8] [--rename OLD=NEW ...]

Every *.hip of both directories is compiled with
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S
and the output split by kernel symbol (.amdhsa_kernel): a kernel is everything from its label to its .size line,
i.e. its instruction stream and its .amdhsa_* block.  Kernels may move between files; the set of symbols over the whole library and
every kernel's text must be the same.  Lines that name a file or the per-file __hip_cuid_ and the assembler's comments are dropped, and
the function ordinal inside local labels (.LBB3_7 -> .LBB_7: it counts the functions of the file) is removed.
--rename OLD=NEW substitutes NEW for OLD in the old tree's symbols and kernel texts before comparing, for a kernel that changed its
name and nothing else; OLD and NEW are fragments of the mangled symbol (15k_moddown_split=13k_moddown_ntt)."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S"]


def compile_tree(csrc, out, jobs):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))

    def one(s):
        o = os.path.join(out, os.path.basename(s)[:-4] + ".s")
        subprocess.check_call([hipcc, *FLAGS, s, "-o", o], stderr=subprocess.DEVNULL)
        return o
    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, srcs))


def kernels(paths):
    """symbol -> (file, text)"""
    res = {}
    for path in paths:
        lines = open(path).read().split("\n")
        lines = [l for l in lines if "__hip_cuid_" not in l and not re.match(r"\s*\.(file|ident)\b", l)]
        names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m]
        for n in names:
            a = next(i for i, l in enumerate(lines) if l.startswith(n + ":"))
            e = next(i for i in range(a, len(lines)) if lines[i].startswith("\t.size\t" + n + ","))
            text = "\n".join(lines[a:e + 1])
            assert ".amdhsa_kernel " + n in text and ".end_amdhsa_kernel" in text, n
            assert n not in res, f"kernel {n} defined twice"
            # local labels carry the ordinal of the function inside its file (.LBB3_7, .Lfunc_end3): a kernel that moved
            # to another file is renumbered, nothing else
            res[n] = (os.path.basename(path), re.sub(r"(\.L(?:BB|func_end|func_begin|tmp)|\bBB)\d+", r"\1", re.sub(r"[ \t]*;[^\n]*", "", text)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        os.mkdir(t + "/old"), os.mkdir(t + "/new")
        old = kernels(compile_tree(a.old, t + "/old", a.jobs))
        new = kernels(compile_tree(a.new, t + "/new", a.jobs))
    for r in a.rename:
        o, n = r.split("=")
        hit = [k for k in old if o in k]
        assert hit, f"--rename {r}: no kernel of the old tree has {o} in its symbol"
        for k in hit:
            f, text = old.pop(k)
            assert k.replace(o, n) not in old, f"--rename {r}: {k.replace(o, n)} exists in the old tree"
            old[k.replace(o, n)] = (f, text.replace(o, n))
            print(f"renamed: {k} -> {k.replace(o, n)}")
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print(f"ONLY IN {'old' if n in old else 'new'}: {n}")
            bad += 1
        elif old[n][1] != new[n][1]:
            print(f"DIFFERS: {n} ({old[n][0]} -> {new[n][0]})")
            bad += 1
        elif old[n][0] != new[n][0]:
            print(f"moved, identical: {n} ({old[n][0]} -> {new[n][0]})")
    print(f"{len(old)} kernels old, {len(new)} new, {bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
