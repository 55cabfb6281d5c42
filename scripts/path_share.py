#!/usr/bin/env python3
"""Share of the default bench workload's reads that the closed forms of the decision step decide (kernels.hip k4_wave_chain,
k4_wave_path), and what turns the others away -- counted by an ablation build:

    scripts/build_variant.sh ablate lmat_amd/csrc/kernels.hip -DLMAT_ABLATE=1
    LMAT_LIB=$PWD/lmat_amd/variants/ablate.so python scripts/path_share.py [bench.py arguments]

Runs bench.py in this process for one launch (--steps 1 --warmup 0 unless given) and prints, beside bench.py's own JSON line, the
counter block of that launch (kernels.hpp kCurChain* / kCurPath*) and k4_wave_path's reasons (lmat_ablate_path_why, an entry
point only the ablation build has).  profiles/decide_path_share.txt is this output, laid out."""
import ctypes
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lmat_amd import capi  # noqa: E402

WHY = ("offered", "decided", "kept count outside 1..nT", "no ancestor of v registered", "another id with a count >= c0",
       "an ancestor of v with a count < c0", "another id below v", "no ancestor of v at depth 0", "a plasmid / screened PhiX id",
       "a close id's walk would end the scan part-way")


def main():
    plain = capi.Engine.last_counters

    def last_counters(self):
        out = np.zeros(16, dtype=np.uint32)
        self._chk(self.lib.lmat_debug_last_counters(self.ctx, out.ctypes.data_as(ctypes.c_void_p)))
        seen, lone, chain, offered, path = (int(out[i]) for i in (11, 12, 13, 14, 1))
        print(f"[path_share] last launch: met k4_wave's entry conditions {seen}, lone {lone}, decided by k4_wave_chain {chain}, "
              f"offered to k4_wave_path {offered}, decided by it {path}", flush=True)
        why = np.zeros(16, dtype=np.uint32)
        fn = getattr(self.lib, "lmat_ablate_path_why", None)
        if fn is None:
            print("[path_share] not an ablation build: no lmat_ablate_path_why", flush=True)
        elif fn(why.ctypes.data_as(ctypes.c_void_p), 1) == 0:
            for name, n in zip(WHY, why.tolist()):
                print(f"[path_share] all launches: {name:48s} {n:10d}  {100.0 * n / max(int(why[0]), 1):5.1f} % of the offered", flush=True)
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
