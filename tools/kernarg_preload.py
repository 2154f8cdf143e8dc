#!/usr/bin/env python3
"""tools/kernarg_preload.py [LIB]: kernarg preload length (dwords) of every kernel in the gfx950 code objects of libkge_hip.so.

The command processor of gfx950 can hand a wavefront the leading kernel-argument dwords in SGPRs when it starts; how many is a
field of the 64-byte kernel descriptor (symbol `<kernel>.kd`, bytes 58-59: bits 0-6 length, bits 7-15 offset, both in dwords).
The compiler only fills it for leading plain (pointer / integer) parameters and only under
`-mllvm -amdgpu-kernarg-preload-count=<n>`, so this is how a build is checked for it (tests/test_kernarg_preload.py).
Needs llvm-readelf (ROCm's LLVM); prints `length  demangled name` per kernel, or returns {name: length} from preload_lengths()."""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dgl-ke_amd", "dglke_amd", "libkge_hip.so")
LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
READELF = os.path.join(LLVM_BIN, "llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob, arch="gfx950"):
    """the device ELFs for `arch` inside an (uncompressed) clang offload bundle; a linked library holds one bundle per source file"""
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if arch in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


def _descriptors(elf_path):
    """{demangled kernel name: preload length} of one device ELF"""
    run = lambda *a: subprocess.run([READELF] + list(a) + [elf_path], check=True, stdout=subprocess.PIPE, text=True).stdout
    secs = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run("-S", "--wide"), re.M):
        secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))        # address, file offset
    with open(elf_path, "rb") as fh:
        data = fh.read()
    out = {}
    for line in run("-s", "--wide", "--demangle").splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or not f[6].isdigit():
            continue
        name = f[7]
        if name.endswith(" (.kd)"):          # demangled: `void kernel<...>(...) (.kd)`
            name = name[:-6]
        elif name.endswith(".kd"):           # extern "C" kernels
            name = name[:-3]
        else:
            continue
        addr, off = secs[int(f[6])]
        kd = int(f[1], 16) - addr + off
        out[name] = struct.unpack_from("<H", data, kd + 58)[0] & 0x7F
    return out


def preload_lengths(lib=LIB):
    with open(lib, "rb") as fh:
        blob = fh.read()
    out = {}
    for elf in code_objects(blob):
        with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
            tmp.write(elf)
            tmp.flush()
            out.update(_descriptors(tmp.name))
    return out


if __name__ == "__main__":
    for name, n in sorted(preload_lengths(sys.argv[1] if len(sys.argv) > 1 else LIB).items()):
        print("%3d  %s" % (n, name))
