#!/usr/bin/env python3
"""One line per gfx950 kernel of the given host objects: has a change moved any kernel's code?

    scripts/kernel_digest.py OBJ...          (without arguments: lmat_amd/csrc/kernels.o)

For every kernel of the gfx950 code objects inside the objects, sorted by name:

    mangled name, VGPRs, SGPRs, VGPR spills, SGPR spills, scratch bytes, LDS bytes, instruction count, SHA-256 of the instruction text

The resources are the code object's metadata notes (as scripts/kernel_resources.sh reads them).  The instruction text is that of
`llvm-objdump -d --no-show-raw-insn` without its comments (which hold the addresses), one instruction a line, as far as the symbol's
size reaches (the listing runs on through the padding up to the next symbol, which is nobody's code).
NORMALISED: the literal operand of the s_add_u32 / s_addc_u32 that complete a pc-relative address begun by s_getpc_b64 (the address of
a table in the code object, e.g. the two of glibc_logf: it moves whenever anything in front of it changes size).  Nothing else.

Two builds whose outputs are equal run the same instructions with the same registers, kernel by kernel, whichever object a kernel
sits in.  Exit status 1 when a kernel name occurs twice across the objects.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lmat_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
KOBJS = ("kernels.o",)
PCREL = "<pcrel>"
NOTE = "# normalised: literal of the s_add_u32 / s_addc_u32 completing an s_getpc_b64 address -> " + PCREL + "; nothing else"


def kernels_of(disasm, sizes=None):
    """disassembly text -> {symbol: [instruction lines]}, comments (and with them the addresses) dropped.  sizes ({symbol: bytes}, from
    the symbol table): what the listing shows behind a symbol's last byte -- the padding up to the next symbol -- is not its code"""
    out, cur, end = {}, None, None
    for ln in disasm.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(.+)>:\s*$", ln)
        if m:
            cur = out.setdefault(m.group(2), [])
            end = int(m.group(1), 16) + sizes[m.group(2)] if sizes else None
            continue
        if cur is None or not ln[:1].isspace():
            continue
        ins, _, comment = ln.partition("//")
        ins = " ".join(ins.split())
        if end is not None:
            a = re.match(r"\s*([0-9A-Fa-f]+):", comment)
            if not a or int(a.group(1), 16) >= end:
                continue
        if ins:
            cur.append(ins)
    return out


def sizes_of(symtab):
    """`llvm-readelf -s` text -> {function symbol: size in bytes}"""
    out = {}
    for ln in symtab.split("\n"):
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC":
            out[f[7]] = int(f[2], 0)
    return out


def normalise(lines):
    """-> the lines with the literal of the adds that complete an s_getpc_b64 address replaced by PCREL"""
    lo, hi, out = set(), set(), []
    for ins in lines:
        m = re.match(r"^s_getpc_b64 s\[(\d+):(\d+)\]$", ins)
        if m:
            lo.add(m.group(1))
            hi.add(m.group(2))
        else:
            m = re.match(r"^(s_add_u32|s_addc_u32) s(\d+), s(\d+), (\S+)$", ins)
            if m and m.group(2) == m.group(3) and not re.match(r"^[sv]\d|^vcc|^exec|^m0", m.group(4)):
                pending = lo if m.group(1) == "s_add_u32" else hi
                if m.group(2) in pending:
                    pending.discard(m.group(2))
                    ins = "%s s%s, s%s, %s" % (m.group(1), m.group(2), m.group(3), PCREL)
        out.append(ins)
    return out


def digest(lines):
    return hashlib.sha256(("\n".join(normalise(lines)) + "\n").encode()).hexdigest()


def resources_of(notes):
    """`llvm-readelf --notes` text -> {kernel name: (vgpr, sgpr, vgpr spills, sgpr spills, scratch bytes, LDS bytes)}"""
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        out[g("name")] = (g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"),
                          g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    return out


def rows_of(disasm, notes, symtab=None):
    """-> {kernel name: its output line}: the kernels the metadata names, with the digest of their instruction text"""
    code, rows = kernels_of(disasm, sizes_of(symtab) if symtab is not None else None), {}
    for name, res in resources_of(notes).items():
        ins = code[name]
        rows[name] = "%s vgpr %s sgpr %s spill_v %s spill_s %s scratch %s lds %s insns %d sha256 %s" % ((name,) + res + (len(ins), digest(ins)))
    return rows


def merge(per_object):
    """[(object, {name: line})] -> (lines sorted by name, [(name, first object, second object)] for every name that occurs twice)"""
    seen, dups = {}, []
    for obj, rows in per_object:
        for name, line in rows.items():
            if name in seen:
                dups.append((name, seen[name][0], obj))
            else:
                seen[name] = (obj, line)
    return [seen[n][1] for n in sorted(seen)], dups


def code_object_texts(obj):
    """host object -> (disassembly, metadata notes, symbol table) of its gfx950 code object; empty texts for an object without device code"""
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "dev.co")
        if ".hip_fatbin" not in subprocess.run(["objdump", "-h", obj], check=True, capture_output=True, text=True).stdout:
            return "", "", ""
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(t, "copy.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
        run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
        readelf = os.path.join(LLVM, "llvm-readelf")
        return run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co), run(readelf, "--notes", co), run(readelf, "-s", "--wide", co)


def main(argv):
    objs = argv[1:] or [os.path.join(CSRC, o) for o in KOBJS]
    lines, dups = merge([(o, rows_of(*code_object_texts(o))) for o in objs])
    print(NOTE, file=sys.stderr)
    for ln in lines:
        print(ln)
    for name, a, b in dups:
        print("kernel twice: %s (%s, %s)" % (name, a, b), file=sys.stderr)
    return 1 if dups else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
