#!/usr/bin/env python3
"""A taxonomic slice of a loaded database against the full export (lmat_export_set_filter), on the inputs of
dbexport_bench.py: a database built from genomes at two sizes in the minimum table, exported to a file in one pass.
  arm A   what there was before: the full export
  arm B   the slice export -- any(one superkingdom), about 1/2; any(one genus), about 1/16; none(one strain), nearly everything
The arms alternate inside one process and session: every round runs A, then the three slices; round 0 warms up (code objects,
rocPRIM's first launches, the file's pages), the figures are those of round 1 (the second run) with round 2 beside them as the spread.
One JSON line per arm and size.

  python scripts/dbslice_bench.py [--out profiles/dbslice_bench.json] [--small 4] [--large 64]     (sizes in Mbp)"""
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

STAGES = ("ms_scan", "ms_sort", "ms_select", "ms_lists", "ms_fetch", "ms_write")


def one(eng, out, flt):
    t0 = time.perf_counter()
    st = eng.export_taxhisto(out, prefix_bits=0, **flt)
    dt = time.perf_counter() - t0
    ms = {n: round(st[n], 3) for n in STAGES if n in st}
    ms["ms_select"] = round(st["filter"]["ms_select"], 3) if "filter" in st else 0.0
    return {"end_to_end_s": round(dt, 4), "records": st["records"], "entries": st["entries"], "file_bytes": os.path.getsize(out), **ms}


def run(td, mbp, k, recs):
    from lmat_amd import Engine, Params
    fa, tree, _ = make_input(td, mbp)
    tax = synth.make_taxonomy((2, 2, 2, 2, 4, 4), specials=False)
    aux = synth.write_aux_files(os.path.join(td, "aux_%g" % mbp), tax)
    genus = next(t for t in tax.ids if tax.depth[t] == 4)
    arms = [("A_full", {}), ("B_any_superkingdom", dict(taxa=[tax.children[1][0]], mode="any")), ("B_any_genus", dict(taxa=[genus], mode="any")),
            ("B_none_strain", dict(taxa=[tax.leaves[0]], mode="none"))]
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        eng.build_db_from_genomes(fa, tree, k=k)
        out = os.path.join(td, "export.bin")
        rounds = [[one(eng, out, flt) for _, flt in arms] for _ in range(3)]
        full = rounds[1][0]
        for i, (label, _) in enumerate(arms):
            r = rounds[1][i]
            ms = {n: r[n] for n in STAGES}
            rec = {"label": "%gMbp_%s" % (mbp, label), "k": k, "scanned": eng.db_size, "kept_share": round(r["records"] / max(eng.db_size, 1), 4), **r,
                   "scanned_per_s": round(eng.db_size / r["end_to_end_s"]), "kept_per_s": round(r["records"] / r["end_to_end_s"]),
                   "dominant_stage": max(ms, key=ms.get), "vs_full": round(r["end_to_end_s"] / full["end_to_end_s"], 3),
                   "end_to_end_s_round2": rounds[2][i]["end_to_end_s"]}
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
