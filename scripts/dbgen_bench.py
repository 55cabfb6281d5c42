#!/usr/bin/env python3
"""Throughput of the database build from genome FASTA (lmat_build_*): bases/s and k-mers/s end to end and
the HIP-event ms of every stage, at two sizes; the larger one is also run with a device budget that forces several prefix
passes, and (LMAT_DBGEN_SORT=pairs, in a child process) with the pair sort instead of the packed key.  One JSON line per run.

  python scripts/dbgen_bench.py [--out profiles/dbgen_bench.json] [--small 4] [--large 64]     (sizes in Mbp)
  python scripts/dbgen_bench.py --reference-cpu /path/to/bin    times <bin>/kmerPrefixCounter + <bin>/tax_histo on the small input
                                                                (no GPU involved; the reference is not part of this repository)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lmat_amd import synth  # noqa: E402


def make_input(td, mbp, one_line=False):
    """Strain genomes of synth.make_taxonomy((2,2,2,2,4,4)) (256 owners): species ancestors with 1 % strain substitutions and a
    genus block, so that lists of 1, 4 + 1 and 16 + 4 + 1 taxids all occur; three N per genome."""
    tax = synth.make_taxonomy((2, 2, 2, 2, 4, 4), specials=False)
    paths = synth.write_aux_files(td, tax)
    G = int(mbp * 1e6 / len(tax.leaves))
    genomes = synth.make_genomes(tax, G, 2002)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    rng = np.random.default_rng(5)
    fa = os.path.join(td, "genomes_%g.fa" % mbp)
    with open(fa, "wb") as f:
        for leaf in tax.leaves:
            s = bytearray(letters[genomes[leaf]].tobytes())
            for p in rng.integers(0, len(s), 3):
                s[int(p)] = ord("N")
            f.write(b">%d\n" % leaf)
            if one_line:
                f.write(bytes(s) + b"\n")
            else:
                for j in range(0, len(s), 80):
                    f.write(s[j:j + 80] + b"\n")
    return fa, paths["tree"], G * len(tax.leaves)


def run_gpu(fa, tree, k, label, **opts):
    from lmat_amd import Engine
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "th.bin")
            eng.build_taxhisto(fa, tree, k, out, **opts)   # warm-up: code objects, rocPRIM's first launches
            t0 = time.perf_counter()
            st = eng.build_taxhisto(fa, tree, k, out, **opts)
            dt = time.perf_counter() - t0
            size = os.path.getsize(out)
    finally:
        eng.close()
    ms = {n: round(st[n], 3) for n in ("extract_ms", "sort_ms", "segment_ms", "closure_ms")}
    kernel_ms = sum(ms.values())
    # bytes the two own kernels must move at least: extraction reads every base once per pass and writes 8 B per emitted pair; the
    # closure reads owners (4 B per distinct pair, twice: count and write) and run bounds and writes 8 B counts + 4 B per list entry
    ext_bytes = st["bases"] * st["passes"] + 8 * st["emitted_pairs"]
    rec = {"label": label, "k": k, "sort": os.environ.get("LMAT_DBGEN_SORT", "packed"), "end_to_end_s": round(dt, 4),
           "bases_per_s": round(st["bases"] / dt), "kmers_per_s": round(st["distinct_kmers"] / dt), "kernel_ms_total": round(kernel_ms, 3),
           "dominant_stage": max(ms, key=ms.get), "extract_GBps": round(ext_bytes / max(st["extract_ms"], 1e-6) / 1e6, 1),
           "file_bytes": size, **ms, **{n: st[n] for n in st if not n.endswith("_ms")}}
    print(json.dumps(rec), flush=True)
    return rec


def run_reference(bindir, fa, tree, k):
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        subprocess.run([os.path.join(bindir, "kmerPrefixCounter"), "-i", fa, "-k", str(k), "-o", os.path.join(td, "km"), "-l", "0", "-f", "0"],
                       check=True, capture_output=True)
        t1 = time.perf_counter()
        r = subprocess.run([os.path.join(bindir, "tax_histo"), "-o", os.path.join(td, "th.bin"), "-d", os.path.join(td, "km.0"), "-t", tree, "-f", "32"],
                           check=True, capture_output=True, text=True)
        t2 = time.perf_counter()
    n = int([l for l in r.stdout.splitlines() if l.startswith("num mapping kmers processed")][0].split()[-1])
    return {"label": "reference_cpu", "k": k, "kmerPrefixCounter_s": round(t1 - t0, 3), "tax_histo_s": round(t2 - t1, 3), "records": n,
            "kmers_per_s": round(n / (t2 - t0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", type=float, default=4)
    ap.add_argument("--large", type=float, default=64)
    ap.add_argument("-k", type=int, default=20)
    ap.add_argument("--reference-cpu", default=None)
    ap.add_argument("--only", default=None, help="internal: one run in this process (label:mbp)")
    a = ap.parse_args()
    recs = []
    with tempfile.TemporaryDirectory() as td:
        if a.reference_cpu:
            fa, tree, bases = make_input(td, a.small, one_line=True)
            rec = run_reference(a.reference_cpu, fa, tree, a.k)
            rec["bases"] = bases
            rec["bases_per_s"] = round(bases / (rec["kmerPrefixCounter_s"] + rec["tax_histo_s"]))
            print(json.dumps(rec))
            recs.append(rec)
        elif a.only:
            label, mbp = a.only.split(":")
            fa, tree, _ = make_input(td, float(mbp))
            run_gpu(fa, tree, a.k, label)
            return
        else:
            fa_s, tree, _ = make_input(td, a.small)
            fa_l, _, bases_l = make_input(td, a.large)
            recs.append(run_gpu(fa_s, tree, a.k, "small_%gMbp" % a.small))
            recs.append(run_gpu(fa_l, tree, a.k, "large_%gMbp" % a.large))
            # a budget that holds about a quarter of the large input's pairs: several passes
            budget = (64 << 20) + 2 * (16 << 20) + int(bases_l / 4) * 64
            recs.append(run_gpu(fa_l, tree, a.k, "large_%gMbp_small_budget" % a.large, budget_bytes=budget))
            env = dict(os.environ, LMAT_DBGEN_SORT="pairs")   # the other sort: a fresh process, the variable is read per build
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "large_%gMbp_pair_sort:%g" % (a.large, a.large), "-k", str(a.k)],
                               env=env, capture_output=True, text=True, timeout=600)
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    print(line)
                    recs.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
