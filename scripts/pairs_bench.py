#!/usr/bin/env python3
"""Paired-end reads through the streamed boundary: the boundary-inclusive rate of a 3-slot calls-only Stream
fed from pinned buffers, in two arms on the same 2 x 150-base pairs of a synthetic table:

  A  submit_pairs_pinned: the two blocks of mates as two files give them, joined on the device (pack_pairs_kernel)
  B  submit_pinned on the same pairs joined on the host (mate1 N mate2, 301 bases) BEFORE the clock starts: a host that joins for free

A repetition queues --batches batches of --pairs pairs through the ring and ends when the last batch has come back (lmat_stream_next
waits on the batch's events: the window closes on a device synchronise).  The arms alternate, --reps repetitions each behind one
warm-up each, in one process.  Reported: pairs/s per arm (median, and every repetition), A over B, and B's own run-to-run spread
(max - min over median).  A first batch of each arm is compared record for record.  --laps: a short child run under
LMAT_DEBUG_STREAM=1 whose per-submit host laps (offsets done / copies queued / kernels queued: ms since the submit began) are reported as medians per arm.

  python scripts/pairs_bench.py [--out profiles/pairs_bench.json] [--pairs 131072] [--batches 400] [--reps 5]"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MATE = 150
N_SETS = 3   # distinct batches, one per slot of the ring


class Pinned:
    def __init__(self, capi, arr):
        self.capi, self.addr = capi, capi.host_alloc(arr.size + 64)
        ctypes.memmove(self.addr, arr.ctypes.data, arr.size)

    def free(self):
        self.capi.host_free(self.addr)


def setup(pairs):
    """-> engine, per batch set: (pinned mates 1, pinned mates 2, pinned joined reads)"""
    from lmat_amd import Engine, Params, capi
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy()
    eng.synth_db(20000, k=20)
    sr = eng.synth_reads(2 * pairs * N_SETS, (MATE,), seed=3003)
    blob, off = sr.ascii()
    sr.free()
    assert blob.size == 2 * pairs * N_SETS * MATE
    sets = []
    for s in range(N_SETS):
        m = blob[s * 2 * pairs * MATE:(s + 1) * 2 * pairs * MATE].reshape(pairs, 2, MATE)
        m1, m2 = np.ascontiguousarray(m[:, 0, :]), np.ascontiguousarray(m[:, 1, :])
        joined = np.empty((pairs, 2 * MATE + 1), dtype=np.uint8)
        joined[:, :MATE], joined[:, MATE], joined[:, MATE + 1:] = m1, ord("N"), m2
        sets.append((Pinned(capi, m1.reshape(-1)), Pinned(capi, m2.reshape(-1)), Pinned(capi, joined.reshape(-1))))
    return eng, sets


def run(st, sets, arm, pairs, batches, off_mate, off_joined, keep_first=False):
    """one repetition -> seconds (and the first batch's records)"""
    first = None
    t0 = time.perf_counter()
    for b in range(batches):
        p1, p2, pj = sets[b % N_SETS]
        if st.in_flight == st.n_slots:
            if keep_first and first is None:
                first = st.next()[0]
            else:
                st.next_nocopy()
        if arm == "A":
            st.submit_pairs_pinned(p1.addr, off_mate, p2.addr, off_mate, pairs, tag=b)
        else:
            st.submit_pinned(pj.addr, off_joined, pairs, tag=b)
    while st.in_flight:
        if keep_first and first is None:
            first = st.next()[0]
        else:
            st.next_nocopy()
    return time.perf_counter() - t0, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=1 << 17)
    ap.add_argument("--batches", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--laps", action="store_true", help="internal: six batches per arm and round, markers on stderr (run under LMAT_DEBUG_STREAM=1)")
    a = ap.parse_args()
    from lmat_amd import Stream
    eng, sets = setup(a.pairs)
    off_mate = np.arange(a.pairs + 1, dtype=np.uint64) * MATE
    off_joined = np.arange(a.pairs + 1, dtype=np.uint64) * (2 * MATE + 1)
    st = Stream(eng, 2 * a.pairs, a.pairs * (2 * MATE + 1), 0, n_slots=3)
    try:
        if a.laps:
            for arm in "ab" + "AB" * 3:   # (lower case: warm-up, its laps are not read -- first launches load code objects)
                sys.stderr.write("[arm %s]\n" % arm)
                sys.stderr.flush()
                run(st, sets, arm.upper(), a.pairs, 6, off_mate, off_joined)
            return
        # warm-up of both arms; their first batches must be the same records
        _, ra = run(st, sets, "A", a.pairs, a.batches, off_mate, off_joined, keep_first=True)
        _, rb = run(st, sets, "B", a.pairs, a.batches, off_mate, off_joined, keep_first=True)
        if ra.tobytes() != rb.tobytes():
            sys.stderr.write("the two arms gave different records\n")
            sys.exit(1)
        stats0 = st.stats()
        secs = {"A": [], "B": []}
        for _ in range(a.reps):
            for arm in "AB":
                secs[arm].append(run(st, sets, arm, a.pairs, a.batches, off_mate, off_joined)[0])
        stats1 = st.stats()
    finally:
        st.close()
        for s in sets:
            for p in s:
                p.free()
        eng.close()
    n = a.pairs * a.batches
    rate = {arm: [n / s for s in secs[arm]] for arm in secs}
    med = {arm: statistics.median(rate[arm]) for arm in rate}
    rec = {"seconds_per_repetition": {arm: round(statistics.median(secs[arm]), 4) for arm in secs}, "pairs_per_batch": a.pairs, "batches_per_repetition": a.batches, "repetitions": a.reps, "mate_bases": MATE, "slots": 3,
           "classified_status0_share_first_batch": round(float((ra["status"] == 0).mean()), 4),
           "arm_A_submit_pairs_pinned_pairs_per_s": round(med["A"]), "arm_B_host_joined_submit_pinned_pairs_per_s": round(med["B"]),
           "A_over_B": round(med["A"] / med["B"], 4),
           "arm_B_spread": round((max(rate["B"]) - min(rate["B"])) / med["B"], 4),
           "arm_A_spread": round((max(rate["A"]) - min(rate["A"])) / med["A"], 4),
           "arm_A_repetitions_pairs_per_s": [round(x) for x in rate["A"]], "arm_B_repetitions_pairs_per_s": [round(x) for x in rate["B"]],
           "uniform_submits": stats1["uniform"] - stats0["uniform"], "general_submits": stats1["general"] - stats0["general"],
           "bytes_copied_in_per_pair": {"A": 2 * MATE, "B": 2 * MATE + 1}}
    # host laps of a submit, from a child of its own (the debug prints cost time: not in the timed process)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--laps", "--pairs", str(a.pairs)],
                       env=dict(os.environ, LMAT_DEBUG_STREAM="1"), capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write("the laps run failed (%d)\n%s\n" % (r.returncode, r.stderr[-2000:]))
        sys.exit(1)
    laps, arm = {"A": {}, "B": {}}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[arm (.)\]", line)
        if m:
            arm = m.group(1) if m.group(1) in laps else None
        m = re.match(r"\[stream\] (.+) at ([0-9.]+) ms", line)
        if m and arm:
            laps[arm].setdefault(m.group(1), []).append(float(m.group(2)))
    rec["submit_laps_ms_median"] = {arm: {k: round(statistics.median(v), 3) for k, v in laps[arm].items()} for arm in laps}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
