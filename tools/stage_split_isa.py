#!/usr/bin/env python3
"""Compare the kernels of device ELFs byte for byte: one ELF before a change against the ELFs after it.

usage: tools/stage_split_isa.py BEFORE AFTER [AFTER2 ...] [--gone SUBSTRING ...]

The inputs are the device code objects that `hipcc --save-temps=obj` leaves beside an object: the relocatable
`*-hip-amdgcn-amd-amdhsa-gfx950.o` or the linked `*-gfx950.out`.  Both have one FUNC symbol with a size per kernel and
one 64-byte descriptor object `NAME.kd` per kernel.  Per mangled kernel name the code bytes and the descriptor are
compared; the descriptor's code-entry offset (bytes 16-23) moves with the layout and is left out.  Every kernel of
BEFORE has to turn up exactly once among the AFTER files, equal, except the ones whose name contains a --gone
substring; those have to be absent.  Device functions that are called, not inlined, have no descriptor; they may turn
up in several AFTER files and every copy has to equal BEFORE's.

Use the relocatable objects when a kernel calls such a function: the linked file holds the pc-relative distance to
the callee, which moves with the layout, whereas the relocatable one holds zeros there and a relocation record, and
the records (offset in the function, type, symbol, addend) are compared with the bytes.

Prints a summary and exits 1 on any difference.  Symbols, bytes and relocation records only: no instruction is looked at.
"""
import struct
import sys

SHT_SYMTAB, SHT_RELA, STT_OBJECT, STT_FUNC, STT_SECTION = 2, 4, 1, 2, 3


def kernels(path):
    """({kernel: (code, descriptor without the entry offset)}, {called function: (code, None)}) of one ELF64 file; `code`
    is the bytes with the relocation records that fall into them"""
    d = open(path, "rb").read()
    assert d[:6] == b"\x7fELF\x02\x01", path + ": not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i*shentsize) for i in range(shnum)]

    def content(shndx, addr, size):
        s = secs[shndx]
        off = s[4] + (addr - s[3])
        return d[off:off + size]

    funcs, descs, where, names = {}, {}, {}, []
    for s in secs:
        if s[1] != SHT_SYMTAB:
            continue
        stroff = secs[s[6]][4]
        for o in range(s[4], s[4] + s[5], s[9]):
            name_i, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, o)
            name = d[stroff + name_i:d.index(b"\0", stroff + name_i)].decode()
            names.append((name, info & 0xF, shndx))
            if shndx == 0 or shndx >= 0xFF00 or size == 0:
                continue
            if info & 0xF == STT_FUNC:
                funcs[name] = content(shndx, value, size)
                where[name] = (shndx, value, size)
            elif info & 0xF == STT_OBJECT and name.endswith(".kd") and size == 64:
                kd = content(shndx, value, size)
                descs[name[:-3]] = kd[:16] + kd[24:]
    assert set(descs) <= set(funcs), path + ": a descriptor without its function"
    # relocation records of a relocatable file, by the section they apply to; a record against a section symbol names
    # a place in that section, which is given as (function that holds it, offset in the function) instead
    relocs = {}
    for s in secs:
        if s[1] == SHT_RELA:
            for o in range(s[4], s[4] + s[5], s[9]):
                off, info, addend = struct.unpack_from("<QQq", d, o)
                sym, styp, sshndx = names[info >> 32]
                if styp == STT_SECTION:
                    sym, addend = next(((n, addend - v) for n, (x, v, z) in where.items()
                                        if x == sshndx and v <= addend < v + z), ("section %d" % sshndx, addend))
                relocs.setdefault(s[7], []).append((off, info & 0xFFFFFFFF, sym, addend))
    code = {}
    for n, (shndx, value, size) in where.items():
        recs = sorted((off - value, typ, sym, add) for off, typ, sym, add in relocs.get(shndx, ())
                      if value <= off < value + size)
        code[n] = (funcs[n], tuple(recs))
    return ({n: (code[n], descs[n]) for n in descs}, {n: (code[n], None) for n in code if n not in descs})


def main(argv):
    gone = []
    while "--gone" in argv:
        i = argv.index("--gone")
        gone.append(argv[i + 1])
        del argv[i:i + 2]
    (before, called), after = kernels(argv[0]), {}
    twice, called_bad, called_seen = [], [], set()
    for p in argv[1:]:
        ks, fs = kernels(p)
        twice += sorted(set(ks) & set(after))
        after.update(ks)
        called_bad += sorted(n for n in fs if fs[n] != called.get(n))
        called_seen |= set(fs)
        print("%5d kernels  %s" % (len(ks), p))
    print("%5d kernels  %s (before)" % (len(before), argv[0]))
    print("called device functions (before): %s" % (", ".join(sorted(called)) or "none"))
    called_bad += sorted(n for n in called if n not in called_seen)
    is_gone = lambda n: any(g in n for g in gone)
    missing = sorted(n for n in before if n not in after and not is_gone(n))
    still = sorted(n for n in after if is_gone(n))
    new = sorted(n for n in after if n not in before)
    code = sorted(n for n in before if n in after and before[n][0] != after[n][0])
    desc = sorted(n for n in before if n in after and before[n][1] != after[n][1])
    dropped = sorted(n for n in before if is_gone(n) and n not in after)
    equal = sum(1 for n in before if n in after and before[n] == after[n])
    print("equal (code and descriptor): %d" % equal)
    print("removed on purpose: %d" % len(dropped))
    for n in dropped:
        print("  " + n)
    bad = 0
    for what, names in (("missing", missing), ("should be gone", still), ("not in BEFORE", new),
                        ("in more than one AFTER file", twice), ("code differs", code), ("descriptor differs", desc),
                        ("called function differs or is missing", called_bad)):
        print("%s: %d" % (what, len(names)))
        for n in names:
            print("  " + n)
        bad += len(names)
    print("RESULT: " + ("identical" if bad == 0 else "DIFFERENT"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
