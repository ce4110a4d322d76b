#!/usr/bin/env python3
"""Name, size and sha256 of every kernel in the gfx950 code objects of built units -- is the device code the same code?

    python tools/kernel_digest.py BUILD_DIR              one line per kernel: name, body bytes, sha256(body + descriptor)
    python tools/kernel_digest.py BUILD_DIR OTHER_DIR    compare two builds: kernels only in one, kernels whose bytes differ

BUILD_DIR holds the objects of csrc/Makefile (csrc/build/*.o).  For each object the device code object is taken out of
the .hip_fatbin section with clang-offload-bundler; a kernel is a function symbol with a `<name>.kd` descriptor
symbol beside it, and its digest covers the bytes of both, located through the symbol table.  Comparing per symbol
and not per file is deliberate: two builds of the same source give identical kernels in files that still differ
(notes, ordering of instantiations).  The script digests bytes only.
"""
import glob
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def sections(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    raw = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = raw[shstrndx]
    name = lambda off: elf[strtab[4] + off:elf.index(b"\0", strtab[4] + off)].decode()
    return [dict(name=name(s[0]), type=s[1], addr=s[3], offset=s[4], size=s[5], link=s[6], entsize=s[9]) for s in raw]


def symbols(elf, secs):
    out = {}
    for sec in secs:
        if sec["type"] != 2:          # SHT_SYMTAB
            continue
        strs = secs[sec["link"]]
        for i in range(sec["size"] // 24):
            st_name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sec["offset"] + i * 24)
            if 0 < shndx < len(secs) and size:
                start = strs["offset"] + st_name
                out[elf[start:elf.index(b"\0", start)].decode()] = (shndx, value, size)
    return out


def kernels_of(code_object):
    secs = sections(code_object)
    syms = symbols(code_object, secs)

    def data(sym):
        shndx, value, size = syms[sym]
        at = secs[shndx]["offset"] + value - secs[shndx]["addr"]
        return code_object[at:at + size]

    return {kd[:-3]: (len(data(kd[:-3])), hashlib.sha256(data(kd[:-3]) + data(kd)).hexdigest())
            for kd in syms if kd.endswith(".kd") and kd[:-3] in syms}


def digest(build_dir):
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
            bundle, out = os.path.join(tmp, "bundle"), os.path.join(tmp, "code_object")
            subprocess.run([ROCM + "/llvm/bin/llvm-objcopy", "--dump-section", ".hip_fatbin=" + bundle, obj, os.devnull], check=True)
            subprocess.run([ROCM + "/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET,
                            "--input=" + bundle, "--output=" + out], check=True)
            with open(out, "rb") as f:
                for name, entry in kernels_of(f.read()).items():
                    assert result.setdefault(name, entry) == entry, "two units disagree on " + name
    return result


if __name__ == "__main__":
    if len(sys.argv) == 2:
        for name, (size, sha) in sorted(digest(sys.argv[1]).items()):
            print(name, size, sha)
    elif len(sys.argv) == 3:
        a, b = digest(sys.argv[1]), digest(sys.argv[2])
        for name in sorted(set(a) ^ set(b)):
            print("only in", sys.argv[1] if name in a else sys.argv[2], name)
        differing = sorted(n for n in set(a) & set(b) if a[n] != b[n])
        for name in differing:
            print("differs", name, a[name][0], b[name][0])
        print("kernels compared: %d, only in one build: %d, differing: %d" % (len(set(a) & set(b)), len(set(a) ^ set(b)), len(differing)))
        sys.exit(1 if differing or set(a) ^ set(b) else 0)
    else:
        sys.exit(__doc__)
