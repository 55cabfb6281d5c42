#!/usr/bin/env python3
"""What becomes of the reads k4_wave_path turns away for "another id with a count >= c0" (kernels.hip k4_wave_tie): how many have
tied kept ids of one depth, with and without an ancestor counting above c0, how many the closed form decides and what turns the others
away -- counted by an ablation build:

    scripts/build_variant.sh ablate lmat_amd/csrc/kernels.hip -DLMAT_ABLATE=1
    LMAT_LIB=$PWD/lmat_amd/variants/ablate.so python scripts/tie_share.py [bench.py arguments]

Runs bench.py in this process for one launch (--steps 1 --warmup 0 unless given) and prints, beside bench.py's own JSON line and
scripts/path_share.py's counts, k4_wave_tie's reasons (lmat_ablate_tie_why, an entry point only the ablation build has).
profiles/decide_tie_share.txt is this output, laid out."""
import ctypes
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lmat_amd import capi  # noqa: E402

WHY = ("offered", "decided", "kept count outside 2..nT-1", "one kept id at the largest kept count (no tie)", "tied ids of unequal depth",
       "an ancestor of a tied id without a slot", "no common ancestor registered", "a slot above c0 outside COMMON",
       "a PRIVATE count other than c0", "a REST count of c0 or more", "a COMMON count below c0, or falling towards the root",
       "the deepest common ancestor among the kept slots", "no common ancestor at depth 0", "a plasmid / screened PhiX id", "a REST id below a tied id",
       "a negative threshold, or a close id's walk would end the scan part-way",
       "tied ids of one depth WITH an ancestor counting above c0", "tied ids of one depth WITHOUT one")


def main():
    plain = capi.Engine.last_counters

    def last_counters(self):
        out = np.zeros(16, dtype=np.uint32)
        self._chk(self.lib.lmat_debug_last_counters(self.ctx, out.ctypes.data_as(ctypes.c_void_p)))
        seen, lone, chain, offered, path = (int(out[i]) for i in (11, 12, 13, 14, 1))
        print(f"[tie_share] last launch: met k4_wave's entry conditions {seen}, lone {lone}, decided by k4_wave_chain {chain}, "
              f"offered to k4_wave_path {offered}, decided by it {path}", flush=True)
        for entry, names, n in (("lmat_ablate_path_why", None, 16), ("lmat_ablate_tie_why", WHY, 32)):
            why = np.zeros(n, dtype=np.uint32)
            fn = getattr(self.lib, entry, None)
            if fn is None:
                print(f"[tie_share] not an ablation build: no {entry}", flush=True)
            elif fn(why.ctypes.data_as(ctypes.c_void_p), 1) == 0:
                for i, v in enumerate(why.tolist()):
                    name = names[i] if names and i < len(names) else f"[{i}]"
                    if names is None or i < len(names):
                        print(f"[tie_share] all launches: {entry[12:]:9s} {name:70s} {v:10d}  {100.0 * v / max(int(why[0]), 1):5.1f} % of the offered", flush=True)
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
