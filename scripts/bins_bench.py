#!/usr/bin/env python3
"""Reads pulled by called taxon beside the classify step it follows: 2 M synthetic 150-base reads of a synthetic
table, classified calls-only with the records left on the device, then lmat_bins_run on them under groups that select about 1 %,
10 % and 100 % of the reads, with and without bases.

Per arm, host clock around calls that end in a device synchronise, --reps repetitions behind one warm-up, medians reported:
  classify_ms     lmat_classify_async + lmat_sync alone
  run_ms          lmat_bins_run without bases: select, stable partition, group offsets, length scan (blocking)
  run_bases_ms    lmat_bins_run with bases: the same + the unpack kernel        (unpack_ms = the difference)
  fetch_ms        lmat_bins_counts + lmat_bins_fetch of every group: the only copies back
  bytes_back      what those copies carried: 4 per index, 8 per offset, 1 per base
The 1 % and 10 % groups are taxids taken from the records of the run itself (the most called ones, until their share is reached);
the 100 % arm is one REST group.  Ratios to classify_ms are in the output.

  python scripts/bins_bench.py [--out profiles/bins_bench.json] [--reads 2000000] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def spread(v):
    """(max - min) over the median of the repetitions"""
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bins_bench.json"))
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from lmat_amd import Bins, Engine, Params
    from lmat_amd.capi import BIN_REST
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy()
    eng.synth_db(20000, k=20)
    reads = eng.synth_reads(a.reads, (150,), seed=3003)
    n = len(reads)

    def classify():
        eng.classify_async(reads)
        eng.sync()

    classify_ms, classify_all = timed(classify, a.reps)
    res = eng.fetch_results(0, n)
    called = res["call_tid"][(res["status"] == 0) & (res["match_type"] <= 2) & (res["call_score"] >= 0.5) & (res["cand_kmer_cnt"] >= 30)]
    tids, cnt = np.unique(called, return_counts=True)
    order = np.argsort(-cnt, kind="stable")

    def ids_for(share):
        take, have = [], 0
        for j in order:
            if have >= share * n:
                break
            if have + cnt[j] > 1.5 * share * n and take:
                continue
            take.append(int(tids[j]))
            have += int(cnt[j])
        return take

    arms = {"1%": [(ids_for(0.01), 0)], "10%": [(ids_for(0.10), 0)], "100%": [([], BIN_REST)]}
    out = {"reads": n, "read_len": 150, "reps": a.reps, "classify_ms": classify_ms, "classify_ms_spread": spread(classify_all), "arms": {}}
    b = Bins(eng)
    for name, groups in arms.items():
        b.set(groups, 0.5, 30)
        lib, h = b.lib, b.h
        run_ms, run_all = timed(lambda: b._chk(lib.lmat_bins_run(h, reads.h, 0, n, 0)), a.reps)
        runb_ms, runb_all = timed(lambda: b._chk(lib.lmat_bins_run(h, reads.h, 0, n, 1)), a.reps)
        got = {}

        def fetch():
            nr, nb = b.counts()
            tot = 0
            for g in range(len(groups)):
                idx = np.zeros(max(int(nr[g]), 1), dtype=np.uint32)
                off = np.zeros(int(nr[g]) + 1, dtype=np.uint64)
                bases = np.zeros(max(int(nb[g]), 1), dtype=np.uint8)
                b._chk(lib.lmat_bins_fetch(h, g, idx.ctypes.data, off.ctypes.data, bases.ctypes.data))
                tot += 4 * int(nr[g]) + 8 * (int(nr[g]) + 1) + int(nb[g])
            got["bytes"], got["reads"], got["bases"] = tot, int(nr.sum()), int(nb.sum())

        fetch_ms, fetch_all = timed(fetch, a.reps)
        out["arms"][name] = {"ids": len(groups[0][0]), "selected_reads": got["reads"], "selected_share": got["reads"] / n, "selected_bases": got["bases"],
                             "run_ms": run_ms, "run_bases_ms": runb_ms, "unpack_ms": runb_ms - run_ms, "fetch_ms": fetch_ms,
                             "bytes_back": got["bytes"], "bytes_back_without_bases": got["bytes"] - got["bases"],
                             "run_over_classify": run_ms / classify_ms, "run_bases_over_classify": runb_ms / classify_ms,
                             "run_ms_spread": spread(run_all), "run_bases_ms_spread": spread(runb_all), "fetch_ms_spread": spread(fetch_all)}
    b.close()
    reads.free()
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
