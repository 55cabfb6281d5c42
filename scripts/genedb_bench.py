#!/usr/bin/env python3
"""Throughput of the gene database build (the builder's id-set mode, lmat_genebuild_create): genes/s, bases/s,
records and the HIP-event ms of every stage (median of three builds after a warm-up), at two sizes; every input is also built
in TREE mode under a star tree (every id a child of the root), the path that does the closure walk over the same text; the two
arms alternate, twice.  One JSON line per run.

  python scripts/genedb_bench.py [--out profiles/genedb_bench.json] [--small 4096] [--large 65536]     (sizes in genes)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_input(td, n_genes, length=1000, family=8):
    """Synthetic genes of `length` bases in families of `family` that share two 200-base blocks (one with the whole family, one with
    half of it); ids are spread over the 32-bit range.  -> (FASTA, star tree file, bases)"""
    rng = np.random.default_rng(21)
    fa = os.path.join(td, "genes_%d.fa" % n_genes)
    ids = np.sort(rng.choice(np.arange(2, 1 << 32, 977, dtype=np.uint64), n_genes, replace=False))
    with open(fa, "wb") as f:
        for g in range(0, n_genes, family):
            whole, half = LETTERS[rng.integers(0, 4, 200)], [LETTERS[rng.integers(0, 4, 200)] for _ in range(2)]
            for j in range(min(family, n_genes - g)):
                s = LETTERS[rng.integers(0, 4, length)].copy()
                s[100:300] = whole
                s[500:700] = half[j & 1]
                f.write(b">%d\n" % ids[g + j])
                for at in range(0, length, 80):
                    f.write(s[at:at + 80].tobytes() + b"\n")
    tree = os.path.join(td, "star_%d.dat" % n_genes)
    with open(tree, "w") as f:   # three header lines, then "id nchild children.. parent" / name pairs; the root is its own parent
        f.write("# star\n# id nchild children... parent / name\n%d\n" % (n_genes + 1))
        f.write("1 %d %s 1\nroot\n" % (n_genes, " ".join(str(i) for i in ids.tolist())))
        f.write("".join("%d 0 1\ng\n" % i for i in ids.tolist()))
    return fa, tree, n_genes * length


def run(fa, tree, k, label, n_genes):
    from lmat_amd import Engine
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "g.bin")
            build = (lambda: eng.build_taxhisto(fa, tree, k, out)) if tree else (lambda: eng.build_gene_taxhisto(fa, k, out))
            build()   # warm-up: code objects, rocPRIM's first launches
            runs = []
            for _ in range(3):
                t0 = time.perf_counter()
                st = build()
                runs.append((time.perf_counter() - t0, st))
            runs.sort(key=lambda r: r[0])
            dt, st = runs[1]   # the median run and its stage times
            size = os.path.getsize(out)
    finally:
        eng.close()
    ms = {n: round(st[n], 3) for n in ("extract_ms", "sort_ms", "segment_ms", "closure_ms")}
    rec = {"label": label, "mode": "tree(star)" if tree else "id-set", "k": k, "genes": n_genes, "end_to_end_s": round(dt, 4),
           "end_to_end_s_min_max": [round(runs[0][0], 4), round(runs[2][0], 4)], "genes_per_s": round(n_genes / dt), "bases_per_s": round(st["bases"] / dt), "records": st["records_written"],
           "kernel_ms_total": round(sum(ms.values()), 3), "file_bytes": size, **ms,
           **{n: st[n] for n in ("bases", "emitted_pairs", "total_list_entries", "longest_list", "singletons", "passes")}}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--large", type=int, default=65536)
    ap.add_argument("-k", type=int, default=20)
    a = ap.parse_args()
    recs = []
    with tempfile.TemporaryDirectory() as td:
        for n in (a.small, a.large):
            fa, tree, _ = make_input(td, n)
            for rep in range(2):
                recs.append(run(fa, None, a.k, "genes_%d_rep%d" % (n, rep), n))
                recs.append(run(fa, tree, a.k, "genes_%d_star_tree_rep%d" % (n, rep), n))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
