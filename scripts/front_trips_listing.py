#!/usr/bin/env python3
"""The listing check of the read loop's front end ("Round trips at the ends of a read").

    scripts/front_trips_listing.py [kernels.s | kernels.o]

Without an argument: lmat_amd/csrc/kernels.o when the library has been built and the object is newer than its sources (its gfx950
code object is disassembled, seconds), else the assembly of kernels.hip is built with hipcc (minutes).  For the three instantiations of the headline class -- UNI, PLAIN
and the generic <160,64,256> compact one -- it looks at the vector-memory loads and at the waits on their counter, nothing else:

  * the first record's load is waited for before any other vector-memory load is issued (before the read loop);
  * from the next record's load (the last one-word load in front of the tail entries' 16-byte load) to the tail entries' loads no
    wait names the vector-memory counter;
  * the tail entries are asked for with the record, so the first such wait behind their loads -- their consumer -- lies at least
    MIN_GAP instructions behind the record's load (pass 1 of two chunks is about 120 vector instructions), in all three.

Prints one line per instantiation; exit status 1 when a condition fails.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lmat_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
MIN_GAP = 100
HEAD = "_ZN4lmat15classify_kernelILi160ELi64ELi256ELb0ELb0ELb1ELb0E"
KERNELS = {"UNI": HEAD + "Lb1ELb1EEEvNS_12ClassifyArgsE", "PLAIN": HEAD + "Lb1ELb0EEEvNS_12ClassifyArgsE",
           "generic": HEAD + "Lb0ELb0EEEvNS_12ClassifyArgsE"}


def hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def built_object():
    """-> lmat_amd/csrc/kernels.o when it can stand for kernels.hip: the tools that take it apart are here, and it is newer than
    kernels.hip and every header the Makefile builds it from; else None (the assembly is then built from the source)"""
    obj = os.path.join(CSRC, "kernels.o")
    tools = [shutil.which("objcopy"), os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-objdump")]
    if not os.path.exists(obj) or not all(t and os.path.exists(t) for t in tools):
        return None
    srcs = [os.path.join(CSRC, f) for f in ("kernels.hip", "kernels.hpp", "lmat_internal.hpp", "devbuf.hpp", "lmat_common.hpp",
                                            "dbbuild.hpp", "outfmt.hpp")] + [os.path.join(ROOT, "include", "lmat_hip.h")]
    return obj if all(os.path.getmtime(obj) >= os.path.getmtime(s) for s in srcs) else None


def listing(path=None):
    """-> the text of an assembly listing or a disassembly that holds the three kernels"""
    if path is None:
        path = built_object() or os.path.join(CSRC, "kernels.hip")
    if path.endswith(".s"):
        with open(path) as f:
            return f.read()
    with tempfile.TemporaryDirectory() as t:
        if path.endswith(".o"):
            fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "dev.co")
            subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(t, "copy.o")], check=True)
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
            return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                  capture_output=True, text=True).stdout
        out = os.path.join(t, "kernels.s")
        subprocess.run([hipcc(), "-std=c++17", "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "--offload-device-only", "-S",
                        "-I" + CSRC, "-w", path, "-o", out], check=True)
        with open(out) as f:
            return f.read()


def body(text, symbol):
    """-> the instruction lines of one kernel, in text order (assembly: `symbol:`; disassembly: `<symbol>:`)"""
    m = re.search(r"^(?:[0-9a-f]+ <" + symbol + r">|" + symbol + r"):.*$", text, flags=re.M)
    if not m:
        raise KeyError(symbol)
    rest = text[m.end():]
    end = re.search(r"^\s*s_endpgm\b.*$|^\s+[0-9a-f]+:\s+s_endpgm\b.*$", rest, flags=re.M)   # (the kernels end in one s_endpgm, behind every block)
    lines = rest[:end.start()].split("\n") if end else rest.split("\n")
    out = []
    for ln in lines:
        ln = re.sub(r"^\s*[0-9a-f]+:\s+", "", ln.split("//")[0].split(";")[0]).strip()   # (disassembly: the address column)
        if ln and not ln.startswith(".") and not ln.endswith(":") and not ln.startswith("<"):
            out.append(ln)
    return out


def check(ins):
    """-> (ok, text) for one kernel's instruction lines"""
    load = [i for i, s in enumerate(ins) if s.startswith("global_load_")]
    wait = [i for i, s in enumerate(ins) if s.startswith("s_waitcnt") and "vmcnt" in s]
    word = [i for i in load if ins[i].startswith("global_load_dword ")]
    x4 = [i for i in load if ins[i].startswith("global_load_dwordx4 ")]
    if not word or not x4:
        return False, "loads not found"
    first = load[0]
    nxt = [i for i in load if i > first]
    settled = any(first < w < nxt[0] for w in wait)
    te = x4[0]
    rec = max(i for i in word if i < te)
    tu = min(i for i in load if i > te)
    between = [w for w in wait if rec < w < tu]
    after = [w for w in wait if w > tu]
    gap = after[0] - rec if after else -1
    ok = settled and not between and rec > first and gap >= MIN_GAP
    return ok, (f"first record settled before the loop: {settled}; waits between the next record's load and the tail loads: "
                f"{len(between)}; instructions from that load to the first wait on vector memory: {gap}")


def main(argv):
    text = listing(argv[1] if len(argv) > 1 else None)
    bad = 0
    for name, sym in KERNELS.items():
        ok, msg = check(body(text, sym))
        print(f"{name:8s} {'ok  ' if ok else 'FAIL'} {msg}")
        bad += not ok
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
