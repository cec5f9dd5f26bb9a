#!/usr/bin/env python3
"""One line per gfx950 kernel of the given object files or code objects:

    <mangled name> <code bytes> <sha256 of the code bytes> vgpr=.. sgpr=.. lds=.. scratch=..

sorted by name, so two builds can be compared with diff.  The four numbers are .vgpr_count,
.sgpr_count, .group_segment_fixed_size and .private_segment_fixed_size of the kernel's entry in
the code object's metadata note.

A host object (hipcc -c) carries its code object in the .hip_fatbin section; it is taken out
with llvm-objcopy and clang-offload-bundler.  An offload bundle (hipcc --offload-device-only) is
unbundled, a file that is an AMDGPU ELF already is read as it is.  Symbols, section headers and
the note come from llvm-readelf; the code bytes are read from the file at the symbol's offset in
.text.  A device function that was not inlined gets a line marked not-a-kernel.  Nothing is
disassembled.  Runs on the CPU.

    python tools/kernel_table.py meep_nl_amd/csrc/_obj/mnl_kernels*.o > kernels.txt
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True,
                          text=True).stdout


def code_object(path, arch, tmp):
    """path itself if it is an AMDGPU ELF; else the code object of arch in the offload bundle
    that path is (hipcc --offload-device-only) or holds in .hip_fatbin (a host object)."""
    base = os.path.join(tmp, os.path.basename(path))
    with open(path, "rb") as fh:
        head = fh.read(24)
    if head.startswith(b"__CLANG_OFFLOAD_BUNDLE__"):
        bundle = path
    elif head[:4] == b"\x7fELF" and int.from_bytes(head[18:20], "little") == 224:  # EM_AMDGPU
        return path
    else:
        bundle = base + ".fatbin"
        run("llvm-objcopy", f"--dump-section=.hip_fatbin={bundle}", path)
    run("clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}",
        f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--output={base}.co")
    return base + ".co"


def kernel_meta(co):
    """{symbol of the kernel descriptor: {key: value}} from the amdhsa.kernels list of the note."""
    out, cur = {}, None
    for line in run("llvm-readelf", "--notes", co).splitlines():
        if re.match(r"^  - \.", line):  # a new entry of amdhsa.kernels (arguments nest deeper)
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.\w+):\s*(.*)$", line)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
            if m.group(1) == ".symbol":
                out[cur[".symbol"]] = cur
        elif not line.startswith("    "):
            cur = None
    return out


def kernels(co):
    text = None  # (index, address, file offset) of .text
    for line in run("llvm-readelf", "-S", "-W", co).splitlines():
        m = re.match(r"^\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s", line)
        if m:
            text = (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16))
    if text is None:
        raise SystemExit(f"{co}: no .text section")
    meta = kernel_meta(co)
    data = open(co, "rb").read()
    rows, seen = [], set()
    for line in run("llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        # Num: Value Size Type Bind Vis Ndx Name
        if len(f) != 8 or f[3] != "FUNC" or f[6] != str(text[0]):
            continue
        value, size, name = int(f[1], 16), int(f[2]), f[7]
        if name in seen:  # .dynsym and .symtab list the same kernels
            continue
        seen.add(name)
        off = value - text[1] + text[2]
        sha = hashlib.sha256(data[off:off + size]).hexdigest()
        md = meta.pop(name + ".kd", None)
        if md is None:  # a device function that was not inlined: no kernel, but it shows
            rows.append(f"{name} {size} {sha} not-a-kernel")
            continue
        vg, sg, lds, scr = (md[k] for k in META)
        rows.append(f"{name} {size} {sha} vgpr={vg} sgpr={sg} lds={lds} scratch={scr}")
    if meta:
        raise SystemExit(f"{co}: kernels in the note without a FUNC symbol: " + " ".join(meta))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="+", help="host objects (.o) or gfx950 code objects")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for p in a.files:
            rows += kernels(code_object(p, a.arch, tmp))
    names = [r.split()[0] for r in rows]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise SystemExit("kernel in more than one input: " + " ".join(dup))
    sys.stdout.write("".join(r + "\n" for r in sorted(rows)))
    print(f"{len(rows)} kernels", file=sys.stderr)


if __name__ == "__main__":
    main()
