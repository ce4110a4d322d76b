#!/usr/bin/env python3
"""Name, size and sha256 of every function in the gfx950 code objects of built units -- is the device code the same code?

    python tools/kernel_digest.py BUILD_DIR              one line per function: kernel | func, name, body bytes, sha256
    python tools/kernel_digest.py BUILD_DIR OTHER_DIR    compare two builds: functions only in one, functions whose bytes differ

BUILD_DIR holds the objects of csrc/Makefile (csrc/build/*.o).  For each object the device code object is taken out of
the .hip_fatbin section with clang-offload-bundler; a kernel is a function symbol with a `<name>.kd` descriptor
symbol beside it, and its digest covers the bytes of both, located through the symbol table -- without bytes 16..23 of the
descriptor (kernel_code_entry_byte_offset: the distance from the descriptor to the body, which says where the kernel sits
in its code object and nothing about the kernel).  Every other function symbol of .text is an out-of-line device function
(`func`): its body is digested alone.  Bodies are taken as linked into the code object: a call to an out-of-line
function is a PC-relative displacement, so a caller (and nothing else) still differs when the distance to its callee
does.  Comparing per symbol and not per file is deliberate: two builds of the same source give identical kernels in files
that still differ (notes, ordering of instantiations).  The script digests bytes only.
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
            st_name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sec["offset"] + i * 24)
            if 0 < shndx < len(secs) and size:
                start = strs["offset"] + st_name
                out[elf[start:elf.index(b"\0", start)].decode()] = (shndx, value, size, info & 15)
    return out


def kernels_of(code_object):
    secs = sections(code_object)
    syms = symbols(code_object, secs)

    def data(sym):
        shndx, value, size, _ = syms[sym]
        at = secs[shndx]["offset"] + value - secs[shndx]["addr"]
        return code_object[at:at + size]

    out = {}
    for name, (shndx, _value, _size, kind) in syms.items():
        if kind != 2 or secs[shndx]["name"] != ".text":          # STT_FUNC
            continue
        body, kd = data(name), name + ".kd"
        if kd in syms:
            desc = data(kd)
            out[name] = ("kernel", len(body), hashlib.sha256(body + desc[:16] + desc[24:]).hexdigest())
        else:
            out[name] = ("func", len(body), hashlib.sha256(body).hexdigest())
    return out


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
        for name, (kind, size, sha) in sorted(digest(sys.argv[1]).items()):
            print(kind, name, size, sha)
    elif len(sys.argv) == 3:
        a, b = digest(sys.argv[1]), digest(sys.argv[2])
        for name in sorted(set(a) ^ set(b)):
            print("only in", sys.argv[1] if name in a else sys.argv[2], (a.get(name) or b[name])[0], name)
        differing = sorted(n for n in set(a) & set(b) if a[n] != b[n])
        for name in differing:
            print("differs", a[name][0], name, a[name][1], b[name][1])
        both = set(a) & set(b)
        print("kernels compared: %d, only in one build: %d, differing: %d" % (
            sum(a[n][0] == "kernel" for n in both), sum((a.get(n) or b[n])[0] == "kernel" for n in set(a) ^ set(b)),
            sum(a[n][0] == "kernel" for n in differing)))
        print("funcs compared: %d, only in one build: %d, differing: %d" % (
            sum(a[n][0] == "func" for n in both), sum((a.get(n) or b[n])[0] == "func" for n in set(a) ^ set(b)),
            sum(a[n][0] == "func" for n in differing)))
        sys.exit(1 if differing or set(a) ^ set(b) else 0)
    else:
        sys.exit(__doc__)
