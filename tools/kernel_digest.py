#!/usr/bin/env python3
"""One line per kernel of libhpgmg_hip.so's device code, to compare two source trees kernel by kernel.

Every hpgmg_amd/csrc/kernels/*.hip is compiled to device assembly with the flags its Makefile rule uses (per-file FLAGS_<stem> included;
-c replaced by -S --cuda-device-only).  For every function of the assembly a line is printed:

    <file stem> <mangled name> <sha1 of the instruction stream> <instructions> vgpr= agpr= sgpr= vspill= sspill= scratch= lds=

The instruction stream is the function's text with assembler comments stripped and the per-function numbers of local labels (.LBB<n>_<m>,
.Lfunc_end<n>, ...) normalised, so a change that only reorders the functions of a file leaves every line as it was.  The figures come from the
kernel's entry in the code object's metadata (a device function that is no kernel has none: '-').

    python tools/kernel_digest.py | sort > after.txt          # and the same in a checkout of the other commit
    diff before.txt after.txt

No GPU is needed.  --root names another source tree, --jobs the number of compilers run at a time, --keep a folder that receives the .s files.
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

LABEL_BLOCK = re.compile(r"\.(LBB|LJTI|LCPI)\d+_")
LABEL_OTHER = re.compile(r"\.L([A-Za-z_]+?)(\d+)\b")
FIGURES = (("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"), ("vspill", "vgpr_spill_count"), ("sspill", "sgpr_spill_count"),
           ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def compile_command(csrc, stem, out):
    """The Makefile's own command for build/<stem>.o, turned into a device-assembly compile."""
    target = os.path.join(os.path.abspath(csrc), "build", stem + ".o")          # the rule's targets are absolute paths
    text = subprocess.run(["make", "-C", csrc, "-n", "-B", target], check=True, capture_output=True, text=True).stdout
    lines = [l for l in text.splitlines() if "kernels/%s.hip" % stem in l and " -c " in l]
    if len(lines) != 1:
        raise RuntimeError("no single compile line for %s in make -n" % stem)
    words = shlex.split(lines[0])
    o = words.index("-o")
    del words[o:o + 2]
    words[words.index("-c")] = "-S"
    return words + ["--cuda-device-only", "-o", out]


def functions(asm):
    """(name, lines of the body) for every function of an assembly text."""
    types = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", asm, re.M))
    name, body = None, []
    for line in asm.splitlines():
        s = line.split(";", 1)[0].strip()
        if name is None:
            if s.endswith(":") and s[:-1] in types:
                name, body = s[:-1], []
            continue
        if s.startswith(".Lfunc_end"):
            yield name, body
            name = None
        elif s:
            body.append(s)


def digest(body):
    seen = {}

    def other(m):
        return ".L%s#%d" % (m.group(1), seen.setdefault(m.group(0), len(seen)))
    text = [LABEL_OTHER.sub(other, LABEL_BLOCK.sub(r".\1_", s)) for s in body]
    count = sum(1 for s in text if not s.startswith(".") and not s.endswith(":"))
    return hashlib.sha1("\n".join(text).encode()).hexdigest()[:16], count


def kernel_figures(asm):
    """name -> {key: value} from the amdhsa.kernels list of the metadata."""
    out, cur = {}, None
    meta = asm.split(".amdgpu_metadata", 1)
    if len(meta) < 2:
        return out
    for line in meta[1].splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'\"")
            if m.group(2) == "name":
                out[cur["name"]] = cur
    return out


def one_file(csrc, stem, folder):
    out = os.path.join(folder, stem + ".s")
    subprocess.run(compile_command(csrc, stem, out), check=True, cwd=csrc, capture_output=True)
    asm = open(out).read()
    figures = kernel_figures(asm)
    rows = []
    for name, body in functions(asm):
        sha, count = digest(body)
        f = figures.get(name)
        rows.append("%s %s %s %d %s" % (stem, name, sha, count, " ".join("%s=%s" % (k, f.get(key, "?") if f else "-") for k, key in FIGURES)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="source tree (default: the one this tool is in)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="folder that receives the .s files")
    ap.add_argument("files", nargs="*", help="stems of kernels/*.hip (default: all)")
    a = ap.parse_args()
    csrc = os.path.join(a.root, "hpgmg_amd", "csrc")
    stems = a.files or sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(csrc, "kernels", "*.hip")))
    with tempfile.TemporaryDirectory() as tmp:
        folder = a.keep or tmp
        os.makedirs(folder, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            for rows in pool.map(lambda s: one_file(csrc, s, folder), stems):
                for r in rows:
                    print(r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
