#!/usr/bin/env python3
"""Registers, scratch and LDS of the kernels inside a built object or library (no GPU needed).

    python tools/kernel_resources.py [--only REGEX] [--digest] file.o|file.so [...]

Takes the .hip_fatbin section out of the file (objcopy), unbundles the gfx950 code object (clang-offload-bundler) and
reads the kernel descriptors' metadata (llvm-readelf --notes): VGPRs, SGPRs, spills, scratch bytes per lane
(private_segment_fixed_size) and static LDS bytes (group_segment_fixed_size) per kernel, names demangled.

--digest adds two columns, for every kernel and every device function that stayed out of line (those have no descriptor:
their resource columns are empty): the number of instructions and a short hash of the function's `llvm-objdump -d` text
without addresses, raw bytes and trailing comments.  "This change keeps the code of kernel K" is then a diff of two such
tables.  Nothing is interpreted: a function whose hash differs at an equal count may differ only in the pc-relative offset
to a callee that moved — look at the disassembly before calling it changed.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(path, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    co = os.path.join(tmp, "k.co")
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                           "--input=" + fat, "--output=" + co])
    return co


def digests(co):
    """{symbol: (instructions, hash)} of every function in the code object's text"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    out, sym, body = {}, None, []
    for line in text.splitlines() + ["0 <>:"]:
        m = re.match(r"[0-9a-f]+ <(.*)>:$", line)
        if m:
            if sym:
                out[sym] = (len(body), hashlib.sha1("\n".join(body).encode()).hexdigest()[:12])
            sym, body = m.group(1), []
        elif sym and line.startswith(("\t", " ")) and line.strip():
            body.append(" ".join(line.split("//")[0].split()))
    return out


def demangle(names):
    names = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"^void ", "", re.sub(r"\(.*$", "", re.sub(r"\(anonymous namespace\)::", "", n))) for n in names]


def kernels(path, digest=False):
    """[{name, vgpr, sgpr, vgpr_spill, sgpr_spill, scratch, lds}] of the gfx950 kernels in an object or shared library;
    digest: with {instructions, hash} each, and behind them the device functions with name, instructions and hash only"""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(path, tmp)
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        code = digests(co) if digest else {}
    out, cur = [], {}
    keys = {".name": "name", ".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".vgpr_spill_count": "vgpr_spill",
            ".sgpr_spill_count": "sgpr_spill", ".private_segment_fixed_size": "scratch", ".group_segment_fixed_size": "lds"}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s+(\S+)", line)
        if not m or m.group(1) not in keys:
            continue
        k = keys[m.group(1)]
        if k in cur:  # the next kernel's block begins
            out.append(cur)
            cur = {}
        cur[k] = m.group(2) if k == "name" else int(m.group(2))
    if cur:
        out.append(cur)
    out = [k for k in out if "name" in k and "vgpr" in k]
    out += [{"name": s} for s in sorted(set(code) - {k["name"] for k in out})]
    for k, n in zip(out, demangle([k["name"] for k in out])):
        if digest:
            k["instructions"], k["hash"] = code[k["name"]]
        k["name"] = n
    return out


def table(path, only=None, digest=False):
    rows = [k for k in kernels(path, digest) if not only or re.search(only, k["name"])]
    lines = ["%-44s %5s %5s %7s %8s %7s" % ("kernel", "VGPR", "SGPR", "spills", "scratch", "LDS") + (" %7s %s" % ("instr", "hash") if digest else "")]
    for k in rows:
        res = "%5d %5d %7d %8d %7d" % (k["vgpr"], k["sgpr"], k.get("vgpr_spill", 0) + k.get("sgpr_spill", 0), k.get("scratch", 0),
                                       k.get("lds", 0)) if "vgpr" in k else " " * 36
        # (a digest table is there to be diffed: names in full)
        lines.append("%-44s %s" % (k["name"] if digest else k["name"][:44], res) + (" %7d %s" % (k["instructions"], k["hash"]) if digest else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        i = args.index("--only")
        only = args[i + 1]
        del args[i:i + 2]
    digest = "--digest" in args
    if digest:
        args.remove("--digest")
    if not args:
        print(__doc__)
        sys.exit(2)
    for p in args:
        print("== %s" % p)
        print(table(p, only, digest))
