#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same, kernel by kernel?

    python tools/compare_code_objects.py before/ba_dense_ldl.o after/ba_dense_ldl.o     (object files or shared libraries)

The guard of a host-only refactor.  Per kernel symbol: the same set of symbols, the same disassembly with the instruction
encodings (only the load address in the trailing comment is dropped) and the same metadata notes (registers, LDS, kernel
arguments) as sorted lines.  Not a hash of the section: moving launch sites changes the order in which templates are first
instantiated, and with it the order of the kernels and their addresses, and nothing else.  Exit status 1 on a difference.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, tmp):
    """every gfx950 ELF of every offload bundle in the .hip_fatbin section"""
    sec = os.path.join(tmp, "fatbin.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, sec], check=True)
    blob = open(sec, "rb").read()
    out, pos = [], 0
    while (pos := blob.find(MAGIC, pos)) >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" in triple and size > 0:
                out.append(blob[pos + off:pos + off + size])
        pos += len(MAGIC)
    return out


def describe(elf_bytes, tmp):
    """({symbol: disassembly without load addresses}, sorted lines of the metadata notes)"""
    elf = os.path.join(tmp, "co.elf")
    open(elf, "wb").write(elf_bytes)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", "--no-leading-addr", elf],
                         capture_output=True, text=True, check=True).stdout
    funcs, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name:
            funcs[name].append(re.sub(r"// [0-9A-F]+:", "//", line.strip()))
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], capture_output=True, text=True, check=True).stdout
    return funcs, sorted(notes.splitlines())


def main(a_path, b_path):
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        a, b = code_objects(a_path, tmp), code_objects(b_path, tmp)
        if len(a) != len(b) or not a:
            print("gfx950 code objects: %d against %d" % (len(a), len(b)))
            return 1
        for n, (x, y) in enumerate(zip(a, b)):
            fa, na = describe(x, tmp)
            fb, nb = describe(y, tmp)
            only = sorted(set(fa) ^ set(fb))
            differ = sorted(k for k in fa if k in fb and fa[k] != fb[k])
            print("code object %d: %d / %d symbols, same order: %s, only in one: %d, disassembly differs: %d, notes equal: %s"
                  % (n, len(fa), len(fb), list(fa) == list(fb), len(only), len(differ), na == nb))
            for k in only + differ:
                print("   ", k)
            bad += len(only) + len(differ) + (na != nb)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
