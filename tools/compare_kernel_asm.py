#!/usr/bin/env python3
"""Are the gfx950 kernels of two source trees the same machine code?   (needs hipcc, no GPU)

usage: python3 tools/compare_kernel_asm.py <root of tree A> <root of tree B>

Compiles every fasttrack_amd/csrc/kernels_*.hip of both trees with the flags of the tree's own Makefile (`-S --cuda-device-only`) and
compares PER KERNEL, whatever file a kernel lives in: the instruction stream with its kernel descriptor (.amdhsa_* block) and
resource symbols, and the kernel's entry in the code-object metadata (registers, scratch, LDS, kernarg layout).  A kernel's
ordinal in its file is normalised away (.LBB<n>_k -> .LBB_k, .Lfunc_end<n>, the loop comments); .file / .ident / __hip_cuid_* lines belong to no
kernel.  The data objects the files define (constant tables) are compared by name: the order in which a file's
anonymous-namespace globals are emitted varies from one run of the same compile to the next (kernels_orient_desc.hip), so whole
files are not compared; a table that a header hands to several files (c_divMagic of extract_dev.h) has to be the same in every one.  Both trees are compiled at the same path by the same command line, one after the other.
Exit status 0: same kernels and objects, all identical.
"""
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).split()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    extra = {m.group(1): m.group(2).split() for m in re.finditer(r"^(\w+)\.o: CXXFLAGS \+= (.*)$", text, re.M)}
    return arch, flags, extra


def compile_tree(root, copy, out):
    """copies the tree's sources to `copy` (the same path for both trees), leaves one .s per kernels_*.hip in `out`"""
    shutil.rmtree(copy, ignore_errors=True)
    work = os.path.join(copy, "fasttrack_amd", "csrc")
    shutil.copytree(os.path.join(root, "fasttrack_amd", "csrc"), work, ignore=shutil.ignore_patterns("*.o", "*.so", "*.s"))
    shutil.copytree(os.path.join(root, "include"), os.path.join(copy, "include"))
    os.makedirs(out)
    arch, flags, extra = makefile_flags(work)

    def one(path):
        stem = os.path.basename(path)[:-4]
        # (the whole command line is the same for both trees, the output's name included: the unit id is derived from it)
        subprocess.check_call([HIPCC, f"--offload-arch={arch}", *flags, *extra.get(stem, []), "-S", "--cuda-device-only", "-o", stem + ".s",
                               stem + ".hip"], cwd=work, stderr=subprocess.DEVNULL)
        shutil.move(os.path.join(work, stem + ".s"), os.path.join(out, stem + ".s"))

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(one, sorted(glob.glob(os.path.join(work, "kernels_*.hip")))))


def normalise(line):
    line = re.sub(r"\s+;", " ;", line)  # (the comment column moves with the width of the ordinal)
    line = re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", line)  # (.LBB<n>_k, and BB<n>_k in the loop comments)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def ignored(line):
    return line.startswith(("\t.file", "\t.ident")) or "__hip_cuid_" in line


def functions(lines):
    """{name: lines} from the function's `-- Begin function` line to the resource symbols and `Kernel info` behind its end"""
    out, name, ended = {}, None, False
    for line in lines:
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, ended = m.group(1), False
            assert name not in out, name
            out[name] = []
        elif name and ended and not line.startswith(("\t.set ", ";", "\t.section\t.AMDGPU.csdata")):
            name = None
        if name:
            out[name].append(normalise(line))
            ended = ended or "; -- End function" in line
    return out


def objects(lines):
    """{name: [section, lines from .type NAME,@object to .size NAME]}"""
    out, name, section = {}, None, None
    for line in lines:
        if line.startswith(("\t.section", "\t.text", "\t.data", "\t.bss")):
            section = line
            if name:
                out[name][0] = line
            continue
        m = re.match(r"\t\.type\t(\S+),@object", line)
        if m:
            name = m.group(1)
            out[name] = [section, []]
        if name:
            out[name][1].append(line)
            if line.startswith("\t.size\t" + name + ","):
                name = None
    return out


def metadata(lines):
    """{kernel name: lines of its entry under amdhsa.kernels}"""
    out, entry = {}, None
    inside = False
    for line in lines:
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and not line.startswith(" "):
            inside = False
        if not inside:
            continue
        if line.startswith("  - "):
            entry = []
        entry.append(line)
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m and len(line) - len(line.lstrip()) == 4:
            out[m.group(1)] = entry
    return out


def load(directory):
    kernels, where, objs, dup = {}, {}, {}, []
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        stem = os.path.basename(path)[:-2]
        lines = [l for l in open(path).read().split("\n") if not ignored(l)]
        for name, obj in objects(lines).items():
            objs.setdefault(name, []).append(obj)
        fn, md = functions(lines), metadata(lines)
        for name in md:  # the kernels: functions with a metadata entry
            if name in kernels:
                dup.append(name)
            kernels[name] = (fn[name], md[name])
            where[name] = stem
    return kernels, where, objs, dup


def main():
    a_root, b_root = sys.argv[1:3]
    tmp = tempfile.mkdtemp(prefix="kernel_asm_")
    try:
        compile_tree(a_root, os.path.join(tmp, "tree"), os.path.join(tmp, "a"))
        compile_tree(b_root, os.path.join(tmp, "tree"), os.path.join(tmp, "b"))
        ka, wa, fa, dupa = load(os.path.join(tmp, "a"))
        kb, wb, fb, dupb = load(os.path.join(tmp, "b"))
    finally:
        if not os.environ.get("KEEP_ASM"):
            shutil.rmtree(tmp, ignore_errors=True)
    bad = 0
    for name in sorted(set(ka) - set(kb)):
        print("lost     ", name, "(" + wa[name] + ")"); bad += 1
    for name in sorted(set(kb) - set(ka)):
        print("added    ", name, "(" + wb[name] + ")"); bad += 1
    for name in dupa + dupb:
        print("duplicate", name); bad += 1
    same = 0
    for name in sorted(set(ka) & set(kb)):
        text, meta = ka[name][0] == kb[name][0], ka[name][1] == kb[name][1]
        same += text and meta
        if not (text and meta):
            print("differs  ", name, "(code)" if not text else "", "(metadata)" if not meta else ""); bad += 1
    moved = sorted(n for n in set(ka) & set(kb) if wa[n] != wb[n])
    for name in sorted(set(fa) | set(fb)):
        # (a table may be emitted by more files of one tree than of the other: every copy the same)
        if len({repr(o) for o in fa.get(name, []) + fb.get(name, [])}) != 1 or not (name in fa and name in fb):
            print("object differs", name); bad += 1
    for stem in sorted(set(wa.values()) | set(wb.values())):
        print(f"file {stem}: {sum(w == stem for w in wa.values())} kernels in A, {sum(w == stem for w in wb.values())} in B")
    print(f"{len(moved)} kernels changed file")
    print(f"{len(set(fa) | set(fb))} data objects")
    print(f"{len(set(ka) | set(kb))} kernels, {same} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
