#!/usr/bin/env python3
"""What the closure of the T <= 64 classes (kernels.hip classify_one) meets: how many reads have several eligible ids, how many chains
they walk and how long the longest is, and how many would meet the entry conditions of a walk at a fixed stride -- counted by an
ablation build:

    scripts/build_variant.sh ablate lmat_amd/csrc/kernels.hip -DLMAT_ABLATE=1
    LMAT_LIB=$PWD/lmat_amd/variants/ablate.so python scripts/closure_stride_share.py [bench.py arguments]

Runs bench.py in this process for one launch (--steps 1 --warmup 0 unless given) and prints, beside bench.py's own JSON line, the
counts of lmat_ablate_stride_share (an entry point only the ablation build has).  profiles/closure_stride_share.txt is this output,
laid out."""
import ctypes
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lmat_amd import capi  # noqa: E402

NAMES = {0: "reads that reach the closure (T <= 64 classes, no -s)", 1: "with one eligible slot (`one`: the short closure)",
         2: "with several eligible slots and a walk (!one && W > 0)",
         4: "  walked chains: 2", 5: "  walked chains: 3", 6: "  walked chains: 4", 7: "  walked chains: 5", 8: "  walked chains: 6",
         9: "  walked chains: 7", 10: "  walked chains: 8", 11: "  walked chains: more than 8",
         12: "  longest walked chain <= 8", 13: "  longest walked chain 9 .. 16", 14: "  longest walked chain 17 .. 32",
         15: "  longest walked chain above 32", 16: "  nel <= 64", 17: "  nel > 64",
         18: "  meeting every entry condition (nel <= 64, chains * stride <= 64)", 19: "  the same with the stride fixed to 8"}


def main():
    plain = capi.Engine.last_counters

    def last_counters(self):
        c = np.zeros(32, dtype=np.uint32)
        fn = getattr(self.lib, "lmat_ablate_stride_share", None)
        if fn is None:
            print("[closure_stride_share] not an ablation build: no lmat_ablate_stride_share", flush=True)
        elif fn(c.ctypes.data_as(ctypes.c_void_p), 0) == 0:
            c = [int(v) for v in c]
            for i in sorted(NAMES):
                print(f"[closure_stride_share] all launches: {NAMES[i]:70s} {c[i]:10d}  {100.0 * c[i] / max(c[0], 1):5.1f} % of the reads, "
                      f"{100.0 * c[i] / max(c[2], 1):5.1f} % of those with several", flush=True)
        return plain(self)

    capi.Engine.last_counters = last_counters
    argv = sys.argv[1:]
    if "--steps" not in argv:
        argv += ["--steps", "1"]
    if "--warmup" not in argv:
        argv += ["--warmup", "0"]
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1"] + argv
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
