#!/usr/bin/env python3
"""How long the taxid lists are that K3b stage 1 meets (kernels.hip classify_one), and how many reads would keep a list for stage 2
were lists of up to 3 / 4 / 6 kept ids completed in stage 1 -- counted by an ablation build:

    scripts/build_variant.sh ablate lmat_amd/csrc/kernels.hip -DLMAT_ABLATE=1
    LMAT_LIB=$PWD/lmat_amd/variants/ablate.so python scripts/list_share.py [bench.py arguments]

Runs bench.py in this process for one launch (--steps 1 --warmup 0 unless given) and prints, beside bench.py's own JSON line, the
counts of lmat_ablate_list_share (an entry point only the ablation build has).  profiles/list_inline_share.txt is this output, laid out."""
import ctypes
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lmat_amd import capi  # noqa: E402

READS = ("reads that reach K3b stage 1 (staging classes, not handed on)", "with a list left to stage 2 at a bound of 2 (parent)",
         "with one left at an inline bound of 3", "with one left at an inline bound of 4", "with one left at an inline bound of 6")
LISTS = ("1 kept id", "2", "3", "4", "5..6", "7..14", "above 14", "empty")


def main():
    plain = capi.Engine.last_counters

    def last_counters(self):
        c = np.zeros(16, dtype=np.uint32)
        fn = getattr(self.lib, "lmat_ablate_list_share", None)
        if fn is None:
            print("[list_share] not an ablation build: no lmat_ablate_list_share", flush=True)
        elif fn(c.ctypes.data_as(ctypes.c_void_p), 0) == 0:
            c = [int(v) for v in c]
            for i, name in enumerate(READS):
                print(f"[list_share] all launches: {name:70s} {c[i]:10d}  {100.0 * c[i] / max(c[0], 1):5.1f} % of the reads, "
                      f"{100.0 * c[i] / max(c[1], 1):5.1f} % of those at a bound of 2", flush=True)
            tot = max(sum(c[8:16]), 1)
            for i, name in enumerate(LISTS):
                print(f"[list_share] all launches: distinct lists, {name:58s} {c[8 + i]:10d}  {100.0 * c[8 + i] / tot:5.1f} %", flush=True)
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
