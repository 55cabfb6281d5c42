"""The per-kernel digest (scripts/kernel_digest.py), which stands where `cmp kernels.o` stood: its text functions on hand-made listings.
Builds nothing, needs no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("kernel_digest", os.path.join(ROOT, "scripts", "kernel_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _listing(name, table_lo, table_hi, reg="v8", wait="vmcnt(0)", base=0x1000):
    """a disassembly in llvm-objdump's layout: one kernel that takes a table's address off the pc, and the padding behind it"""
    ins = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, " + table_lo, "s_addc_u32 s5, s5, " + table_hi,
           "s_add_u32 s6, s6, 0x40", "global_load_dwordx2 v[6:7], v4, s[4:5]", "s_waitcnt " + wait, "v_sub_u32_e32 v8, %s, v6" % reg,
           "s_cbranch_vccnz 65521", "s_endpgm", "s_nop 0", "s_nop 0"]
    text = "\nDisassembly of section .text:\n\n%016x <%s>:\n" % (base, name)
    for i, s in enumerate(ins):
        text += "\t%-58s // %012X: BE841C00\n" % (s, base + 4 * i)
    return text, "   1: %016x %d FUNC GLOBAL PROTECTED 7 %s\n" % (base, 4 * (len(ins) - 2), name)


def _notes(name):
    return ("amdhsa.kernels:\n  - .agpr_count:     0\n    .group_segment_fixed_size: 512\n    .name:           %s\n"
            "    .private_segment_fixed_size: 0\n    .sgpr_count:     16\n    .sgpr_spill_count: 0\n    .symbol:         %s.kd\n"
            "    .vgpr_count:     9\n    .vgpr_spill_count: 0\n" % (name, name))


def test_the_digest_follows_the_code_and_not_the_tables_address():
    mod = _script()
    a, syms = _listing("_ZN4lmat1kEv", "0xfffde238", "-1")
    code = mod.kernels_of(a, mod.sizes_of(syms))["_ZN4lmat1kEv"]
    assert code[-1] == "s_endpgm" and len(code) == 10          # the padding behind the symbol's size is not its code
    assert all("//" not in s and "1000" not in s for s in code)  # no address, no comment
    norm = mod.normalise(code)
    assert norm[2] == "s_add_u32 s4, s4, " + mod.PCREL and norm[3] == "s_addc_u32 s5, s5, " + mod.PCREL
    assert norm[4] == "s_add_u32 s6, s6, 0x40"                  # an add that completes no pc-relative address keeps its literal
    assert [s for i, s in enumerate(norm) if i not in (2, 3)] == [s for i, s in enumerate(code) if i not in (2, 3)]
    # the table elsewhere (another literal, behind the code instead of in front of it), the kernel at another address: equal
    b, syms_b = _listing("_ZN4lmat1kEv", "0x4c0", "0", base=0x2300)
    code_b = mod.kernels_of(b, mod.sizes_of(syms_b))["_ZN4lmat1kEv"]
    assert code_b != code and mod.digest(code_b) == mod.digest(code)
    # one register, or one wait count: not equal
    for kw in ({"reg": "v9"}, {"wait": "vmcnt(1)"}):
        c, syms_c = _listing("_ZN4lmat1kEv", "0xfffde238", "-1", **kw)
        assert mod.digest(mod.kernels_of(c, mod.sizes_of(syms_c))["_ZN4lmat1kEv"]) != mod.digest(code)
    # the line: name, resources from the notes, instruction count, digest
    row = mod.rows_of(a, _notes("_ZN4lmat1kEv"), syms)["_ZN4lmat1kEv"]
    assert row == "_ZN4lmat1kEv vgpr 9 sgpr 16 spill_v 0 spill_s 0 scratch 0 lds 512 insns 10 sha256 " + mod.digest(code)
    # lines sorted by name across objects; a name that occurs twice is reported with both objects
    other = mod.rows_of(*[t.replace("_ZN4lmat1kEv", "_ZN4lmat1aEv") for t in (a, _notes("_ZN4lmat1kEv"), syms)])
    lines, dups = mod.merge([("x.o", mod.rows_of(a, _notes("_ZN4lmat1kEv"), syms)), ("y.o", other)])
    assert [ln.split()[0] for ln in lines] == ["_ZN4lmat1aEv", "_ZN4lmat1kEv"] and dups == []
    lines, dups = mod.merge([("x.o", mod.rows_of(a, _notes("_ZN4lmat1kEv"), syms)), ("y.o", other),
                             ("z.o", mod.rows_of(b, _notes("_ZN4lmat1kEv"), syms_b))])
    assert len(lines) == 2 and dups == [("_ZN4lmat1kEv", "x.o", "z.o")]
