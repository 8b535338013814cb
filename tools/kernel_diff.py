#!/usr/bin/env python3
"""Is the device code of two source trees the same code?  Compares every kernel of two directories of gfx950 device objects: the
function's size and bytes (sha256) and its 64-byte kernel descriptor (registers, LDS, scratch; all of it but the code's offset from the
descriptor, which is layout).  No device needed.  A refactor that moves kernels between translation units uses it to show that no kernel
changed (the files may be cut differently on the two sides: kernels are matched by symbol name over the whole directory).

  for f in multipathnet_amd/csrc/*.hip; do
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -c $f -o OUT/$(basename $f .hip).o   # [-DMPN_DEBUG_HOOKS=1]
  done
  python tools/kernel_diff.py OLD_DIR NEW_DIR

Prints one line per directory pair (kernels, matches) and every exception: a kernel on one side only, one whose code or descriptor
differs, or one that two objects of a directory define with different code.  Exit status 1 if there is any."""
import glob
import hashlib
import os
import struct
import sys

SHT_SYMTAB, STT_OBJECT, STT_FUNC = 2, 1, 2


def kernels_of(path):
    """{kernel symbol: (code size, sha256 of the code, descriptor bytes)} of one ELF64 little-endian code object"""
    d = open(path, "rb").read()
    if d[:24] == b"__CLANG_OFFLOAD_BUNDLE__":  # what `hipcc --cuda-device-only -c` writes: take the amdgcn entry
        n, = struct.unpack_from("<Q", d, 24)
        pos = 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", d, pos)
            triple = d[pos + 24:pos + 24 + tlen]
            pos += 24 + tlen
            if b"amdgcn" in triple:
                d = d[off:off + size]
                break
    if d[:6] != b"\x7fELF\x02\x01":
        raise SystemExit("%s: neither a 64-bit little-endian ELF code object nor an uncompressed offload bundle holding one" % path)
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]  # name type flags addr offset size link info align entsize
    syms = {}
    for _, typ, _, _, off, size, link, _, _, entsize in sec:
        if typ != SHT_SYMTAB:
            continue
        str_off = sec[link][4]
        for k in range(size // entsize):
            name_i, info, _, shndx, value, sz = struct.unpack_from("<IBBHQQ", d, off + k * entsize)
            if shndx == 0 or shndx >= shnum or (info & 15) not in (STT_OBJECT, STT_FUNC):
                continue
            name = d[str_off + name_i:d.index(b"\0", str_off + name_i)].decode()
            start = sec[shndx][4] + value - sec[shndx][3]
            syms[name] = (info & 15, d[start:start + sz])
    out = {}
    for name, (typ, kd) in syms.items():
        if typ == STT_OBJECT and name.endswith(".kd") and len(kd) == 64 and name[:-3] in syms:
            code = syms[name[:-3]][1]
            # bytes 16-23 of a descriptor are kernel_code_entry_byte_offset, the distance from the descriptor to its code: where the
            # linker put the two, not a property of the kernel
            out[name[:-3]] = (len(code), hashlib.sha256(code).hexdigest(), kd[:16] + kd[24:])
    return out


def kernels_of_dir(path):
    """({kernel: (file,) + kernels_of's tuple} over every object of the directory, kernels defined twice with different code)"""
    out, twice = {}, 0
    for f in sorted(glob.glob(os.path.join(path, "*.o"))):
        for name, v in kernels_of(f).items():
            if name in out and out[name][1:] != v:  # a kernel template instantiated in two files must be the same code
                print("  defined twice with different code in %s: %s (%s, %s)" % (path, name, out[name][0], os.path.basename(f)))
                twice += 1
            out[name] = (os.path.basename(f),) + v
    return out, twice


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    (old, twice_old), (new, twice_new) = kernels_of_dir(sys.argv[1]), kernels_of_dir(sys.argv[2])
    one_side = differing = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("  only in %s: %s" % (sys.argv[2] if name in new else sys.argv[1], name))
            one_side += 1
            continue
        (fo, so, ho, ko), (fn, sn, hn, kn) = old[name], new[name]
        what = [w for w, differs in (("size %d -> %d" % (so, sn), so != sn), ("code bytes", so == sn and ho != hn), ("descriptor", ko != kn)) if differs]
        if what:
            print("  differs: %s (%s -> %s): %s" % (name, fo, fn, ", ".join(what)))
            differing += 1
    both = len(set(old) & set(new))
    bad = one_side + differing + twice_old + twice_new
    print("kernels: %d old, %d new, %d in both, %d identical (code bytes and descriptor), %d exceptions" % (len(old), len(new), both, both - differing, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
