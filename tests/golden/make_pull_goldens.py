#!/usr/bin/env python3
"""Builds tests/golden/pull/ by running the reference's own bin/pull_reads.pl (under perl) over the 16 .out files of its example
run (example/example.tgz: two runs of read_label over the same 1000 reads, 8 shards each) with the id files below.

DATA only: the id files, the reads of the example (simple_list.1000.fna.gz), and per run, shard and id file what the script pulled --
(record number in the shard, group = suffix of the pulled file, uid) per pulled read in uid order, and the size and SHA-256 of
every file it wrote.  The .out lines themselves are not stored: tests rebuild them from example_records.json (records in shard
order; `shard_sizes` cuts them) and the reads.  Records the script cannot parse (four columns: no call column) are listed.
Run in the build container:  python3 tests/golden/make_pull_goldens.py [reference root]"""
import glob
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tarfile
import tempfile

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
here = os.path.dirname(os.path.abspath(__file__))
out_dir = os.path.join(here, "pull")
os.makedirs(out_dir, exist_ok=True)

# key -> (lines, thresh, min_kmer)
IDFILES = {
    # the run the issue of this feature tried: shard 0 of the first run gives 79 / 0 / 19 / 1 / 0 reads
    "a": (["5476 237561 294748", "9606", "LowScore 0.2", "NoDbHits", "ReadTooShort"], 0.5, 30),
    # 5476 on two lines (the later line owns it); a group listing the LENGTHS 202 and 100, which pulls the NoDbHits reads (their
    # record prints the read length where a call prints the taxid); LowScore above k, so every other read falls into LowScore
    "b": (["5476 237561", "9606 5476", "777 202 100", "LowScore 25", "NoDbHits"], 1, 15),
    # no NoDbHits line, thresholds no record meets
    "c": (["5476 237561 294748", "9606", "LowScore -5"], 1000, 100000),
    # NoDbHits reads reach LowScore (score k = 20 < 25) before their own group
    "d": (["LowScore 25", "NoDbHits"], 1, 15),
}
RUNS = ("kML+Human.v4-14.20.g10", "kML.v4-14.20.g10")

gold = {"idfiles": {}, "runs": {}, "pulls": {}}
for key, (lines, thresh, min_kmer) in IDFILES.items():
    fn = "ids_%s.txt" % key
    open(os.path.join(out_dir, fn), "w").write("".join(l + "\n" for l in lines))
    gold["idfiles"][key] = {"file": fn, "thresh": thresh, "min_kmer": min_kmer}

with tempfile.TemporaryDirectory() as td:
    tarfile.open(os.path.join(ref, "example", "example.tgz")).extractall(td)
    with open(os.path.join(out_dir, "simple_list.1000.fna.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
        z.write(open(os.path.join(td, "simple_list.1000.fna"), "rb").read())
    for run in RUNS:
        pre = "simple_list.1000.fna.%s.db.lo.rl_output" % run
        shards = sorted(glob.glob(os.path.join(td, pre + "[0-9].out")))
        gold["runs"][run] = {"prefix": pre, "shard_sizes": [], "unparsed": []}
        gold["pulls"][run] = []
        for si, f in enumerate(shards):
            assert os.path.basename(f) == "%s%d.out" % (pre, si)
            hdrs = []
            for ri, line in enumerate(open(f)):
                c = line.rstrip("\n").split("\t")
                hdrs.append(c[0])
                if len(c) != 5:
                    gold["runs"][run]["unparsed"].append([si, ri])
            assert len(set(hdrs)) == len(hdrs)
            where = {h: i for i, h in enumerate(hdrs)}
            gold["runs"][run]["shard_sizes"].append(len(hdrs))
            per_id = {}
            for key, (lines, thresh, min_kmer) in IDFILES.items():
                odir = os.path.join(td, "pulled_%s_%d_%s" % (run, si, key))
                os.makedirs(odir)
                idfile = os.path.join(out_dir, gold["idfiles"][key]["file"])
                subprocess.run(["perl", os.path.join(ref, "bin", "pull_reads.pl"), "%s %s %s %s %s" % (f, idfile, thresh, min_kmer, odir)],
                               check=True, stderr=subprocess.DEVNULL)
                files, triples = {}, []
                stem = "%s.%s.pulled." % (os.path.basename(f), os.path.basename(idfile))
                for pf in sorted(os.listdir(odir)):
                    assert pf.startswith(stem), pf
                    data = open(os.path.join(odir, pf), "rb").read()
                    files[pf] = [len(data), hashlib.sha256(data).hexdigest()]
                    for l in data.decode().split("\n"):
                        if l.startswith(">"):
                            head = l[1:].split(";tid=")[0]
                            uid = int(l.split(";uid=")[1].split(";")[0])
                            triples.append([where[head], pf[len(stem):], uid])
                triples.sort(key=lambda t: t[2])
                assert [t[2] for t in triples] == list(range(len(triples)))
                per_id[key] = {"triples": triples, "files": files}
            gold["pulls"][run].append(per_id)

with open(os.path.join(out_dir, "pull_goldens.json.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as z:
    z.write(json.dumps(gold, separators=(",", ":")).encode())
p0 = gold["pulls"][RUNS[0]][0]["a"]
print({k: v[0] for k, v in p0["files"].items()}, len(p0["triples"]), "reads pulled from shard 0 under ids_a")
for run in RUNS:
    print(run, gold["runs"][run]["shard_sizes"], "unparsed", len(gold["runs"][run]["unparsed"]))
