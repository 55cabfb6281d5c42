#!/usr/bin/env python3
"""Adding genomes to an existing database (lmat_build_add_taxhisto) against the full rebuild, on the inputs
of scripts/dbgen_bench.py: a database A is built from 15/16 of the genomes; then
  (a) update   add_fasta(last 1/16) + add_taxhisto(A) -> the whole database
  (b) rebuild  all FASTA -> the whole database (what the build alone offers)
Both must end in identical bytes (checked).  Each leg is run once to warm up (code objects, rocPRIM's first launches) and then
timed end to end (parse + GPU + file write); one JSON line per size with the ms of every stage, records/s and entries/s of the
update, the stage that dominates it, and the ratio (b)/(a).

  python scripts/dbmerge_bench.py [--out profiles/dbmerge_bench.json] [--small 4] [--large 64] [--repeat 3]    (sizes in Mbp)"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import dbgen_bench  # noqa: E402


def split_fasta(fa, td, tag):
    """The records of fa dealt 15 : 1 -> (FASTA of records 0..14 of every 16, FASTA of record 15 of every 16)."""
    old, new = os.path.join(td, "old_%s.fa" % tag), os.path.join(td, "new_%s.fa" % tag)
    with open(fa, "rb") as f, open(old, "wb") as fo, open(new, "wb") as fn:
        n, dst = -1, fo
        for line in f:
            if line.startswith(b">"):
                n += 1
                dst = fn if n % 16 == 15 else fo
            dst.write(line)
    return old, new


def timed(fn, repeat):
    fn()   # warm-up
    best, st = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        st = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, st


def run(eng, fa, tree, k, label, td, repeat):
    old, new = split_fasta(fa, td, label)
    a_bin, upd, reb = (os.path.join(td, "%s_%s.bin" % (n, label)) for n in ("A", "update", "rebuild"))
    eng.build_taxhisto(old, tree, k, a_bin)
    t_upd, st = timed(lambda: eng.merge_taxhisto(a_bin, tree, k, upd, fasta=new), repeat)
    t_reb, st_r = timed(lambda: eng.build_taxhisto(fa, tree, k, reb), repeat)
    with open(upd, "rb") as f, open(reb, "rb") as g:
        same = f.read() == g.read()
    if not same:
        raise SystemExit("update and rebuild differ at " + label)
    m = st["merge"]
    ms = {"genome_" + n: round(st[n], 3) for n in ("extract_ms", "sort_ms", "segment_ms", "closure_ms")}
    ms.update({"merge_" + n: round(m[n], 3) for n in ("upload_ms", "sort_ms", "segment_ms", "union_ms", "histogram_ms")})
    rec = {"label": label, "k": k, "identical_bytes": same, "repeat": repeat, "update_s": round(t_upd, 4), "rebuild_s": round(t_reb, 4),
           "rebuild_over_update": round(t_reb / t_upd, 3), "records": st["records_written"], "entries": st["total_list_entries"],
           "update_records_per_s": round(st["records_written"] / t_upd), "update_entries_per_s": round(st["total_list_entries"] / t_upd),
           "update_stage_ms_total": round(sum(ms.values()), 3), "dominant_stage": max(ms, key=ms.get), **ms,
           "rebuild_stage_ms": {n: round(st_r[n], 3) for n in ("extract_ms", "sort_ms", "segment_ms", "closure_ms")},
           "merge": {n: m[n] for n in m if not n.endswith("_ms")}, "new_bases": st["bases"], "all_bases": st_r["bases"],
           "file_bytes": os.path.getsize(upd)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", type=float, default=4)
    ap.add_argument("--large", type=float, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("-k", type=int, default=20)
    a = ap.parse_args()
    from lmat_amd import Engine
    recs = []
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as td:
            for mbp in (a.small, a.large):
                if mbp <= 0:
                    continue
                fa, tree, _ = dbgen_bench.make_input(td, mbp)
                recs.append(run(eng, fa, tree, a.k, "%gMbp" % mbp, td, a.repeat))
    finally:
        eng.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
