#!/usr/bin/env python3
"""Throughput of the export of a loaded database (lmat_export_*): records/s end to end, the ms of every stage and
the scan's GB/s (table bytes read per pass), for a database built from genomes at two sizes, exported in one pass and in 8.  One JSON
line per run.

  python scripts/dbexport_bench.py [--out profiles/dbexport_bench.json] [--small 4] [--large 64]     (sizes in Mbp)"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from dbgen_bench import make_input  # noqa: E402
from lmat_amd import synth  # noqa: E402


def run(td, mbp, k, recs):
    from lmat_amd import Engine, Params
    fa, tree, _ = make_input(td, mbp)
    aux = synth.write_aux_files(os.path.join(td, "aux_%g" % mbp), synth.make_taxonomy((2, 2, 2, 2, 4, 4), specials=False))
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        eng.build_db_from_genomes(fa, tree, k=k)
        out = os.path.join(td, "export.bin")
        for label, pb in (("one_pass", 0), ("8_passes", 3)):
            eng.export_taxhisto(out, prefix_bits=pb)   # warm-up: code objects, rocPRIM's first launches
            t0 = time.perf_counter()
            st = eng.export_taxhisto(out, prefix_bits=pb)
            dt = time.perf_counter() - t0
            ms = {n: round(st[n], 3) for n in ("ms_scan", "ms_sort", "ms_lists", "ms_fetch", "ms_write")}
            rec = {"label": "%gMbp_%s" % (mbp, label), "k": k, "end_to_end_s": round(dt, 4), "records_per_s": round(st["records"] / dt),
                   "table_bytes": eng.table_bytes, "scan_GBps": round(eng.table_bytes * st["passes"] / max(st["ms_scan"], 1e-6) / 1e6, 1),
                   "dominant_stage": max(ms, key=ms.get), "file_bytes": os.path.getsize(out), **ms,
                   **{n: st[n] for n in st if not n.startswith("ms_")}}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", type=float, default=4)
    ap.add_argument("--large", type=float, default=64)
    ap.add_argument("-k", type=int, default=20)
    a = ap.parse_args()
    recs = []
    with tempfile.TemporaryDirectory() as td:
        run(td, a.small, a.k, recs)
        run(td, a.large, a.k, recs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
