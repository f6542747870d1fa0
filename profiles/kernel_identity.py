#!/usr/bin/env python3
"""Byte identity of the env kernels across a refactor of their sources.  No GPU needed.

    python profiles/kernel_identity.py PARENT_CSRC NEW_CSRC

Every .hip file of each directory that names EnvParams (the env step family and the cold kernels around it, in
however many files they live) is compiled for the device alone with the Makefile's CXXFLAGS, and its gfx950 code
object unbundled.  Per kernel symbol, over the union of each side's units: presence, a hash of the code bytes, and
a hash of the 64-byte kernel descriptor (<name>.kd) with bytes 16-23 zeroed -- the descriptor-to-code offset, which
depends on the layout of the unit only.  Bytes are hashed, nothing is disassembled.  Prints every difference and one
summary line; exits non-zero on a difference or a kernel missing on either side."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "marl-sat_amd", "Makefile")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BUNDLER = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "llvm", "bin", "clang-offload-bundler")
ARCH = os.environ.get("ARCH", "gfx950")


def cxxflags(csrc):
    """The Makefile's CXXFLAGS (one continued line), its variables resolved for the source directory csrc."""
    text = open(MAKEFILE).read().replace("\\\n", " ")
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    for var, val in (("ARCH", ARCH), ("ROOT", ROOT), ("CSRC", csrc)):
        flags = flags.replace("$(%s)" % var, val)
    return flags.split()


def kernels(elf):
    """{kernel name: (sha of its code, sha of its masked descriptor)} of one ELF64 little-endian code object."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    # (type, addr, offset, size, link) per section
    secs = [struct.unpack_from("<4xI8xQQQI", elf, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in secs if s[0] == 2)  # SHT_SYMTAB
    strtab = secs[symtab[4]]
    syms = {}
    for off in range(symtab[2], symtab[2] + symtab[3], 24):
        name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, off)
        end = elf.index(b"\0", strtab[2] + name)
        if 0 < shndx < shnum:
            at = secs[shndx][2] + value - secs[shndx][1]
            syms[elf[strtab[2] + name:end].decode()] = elf[at:at + size]
    out = {}
    for name, kd in syms.items():
        if name.endswith(".kd") and name[:-3] in syms:
            assert len(kd) == 64, (name, len(kd))
            masked = kd[:16] + bytes(8) + kd[24:]
            out[name[:-3]] = (hashlib.sha256(syms[name[:-3]]).hexdigest(), hashlib.sha256(masked).hexdigest())
    return out


def side(csrc, tmp, tag):
    csrc = os.path.abspath(csrc)
    out = {}
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(".hip") or "EnvParams" not in open(os.path.join(csrc, f)).read():
            continue
        obj, co = os.path.join(tmp, f"{tag}_{f}.o"), os.path.join(tmp, f"{tag}_{f}.co")
        subprocess.run([HIPCC] + cxxflags(csrc) +
                       ["--cuda-device-only", "-c", os.path.join(csrc, f), "-o", obj], check=True)
        subprocess.run([BUNDLER, "--unbundle", "--type=o",
                        f"--targets=hip-amdgcn-amd-amdhsa--{ARCH}", f"--input={obj}", f"--output={co}"], check=True)
        unit = kernels(open(co, "rb").read())
        assert not set(unit) & set(out), f"{f}: a kernel defined in two units"
        out.update(unit)
        print(f"{tag}: {f}: {len(unit)} kernels")
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old, new = side(sys.argv[1], tmp, "parent"), side(sys.argv[2], tmp, "new")
    missing = ncode = nkd = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            missing += 1
            print(f"MISSING in {'parent' if k not in old else 'new'}: {k}")
            continue
        if old[k][0] != new[k][0]:
            ncode += 1
            print(f"CODE differs: {k}")
        if old[k][1] != new[k][1]:
            nkd += 1
            print(f"DESCRIPTOR differs: {k}")
    print(f"kernel_identity: parent {len(old)} kernels, new {len(new)}, common {len(set(old) & set(new))}; "
          f"missing {missing}, code differences {ncode}, descriptor differences {nkd}")
    sys.exit(1 if missing or ncode or nkd else 0)


if __name__ == "__main__":
    main()
