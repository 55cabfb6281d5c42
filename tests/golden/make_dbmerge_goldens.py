#!/usr/bin/env python3
"""Generates the merge fixtures under tests/golden/dbmerge/ (run in the build container, where the reference lies), on the
recipe of make_dbgen_goldens.py and from its fixtures:

  a_p0_k20.bin.gz   the tax_histo file the REFERENCE's kmerPrefixCounter (-l 0 -f 0) + tax_histo (-f 32) make, at k = 20, of the
                    records of dbgen/a.fa at even positions (0, 2, ...); lists in the reference's own (unordered_map) order
  a_p1_k20.bin.gz   ... of the records at odd positions
  a_k20.par.kcnt    what the REFERENCE's countTaxidFrequency (-f 32) writes for dbgen/a_k20.bin: "<taxid> <count>" lines

The programs are compiled from the reference into a temporary directory (with a stand-in for the header CMake would generate);
only the reference's output files are stored, no reference source travels."""
import gzip
import os
import subprocess
import sys
import tempfile

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import dbgen_model as dm  # noqa: E402

REF = os.environ.get("LMAT_REF", "/root/reference")
REFDEFS = "-DIDX_CONFIG=2027 -DTID_SIZE=16 -DDBTID_T=uint16_t -DUSE_SORTED_DB=1 -DWITH_PJMALLOC=0".split()
out = os.path.join(here, "dbmerge")
os.makedirs(out, exist_ok=True)

with tempfile.TemporaryDirectory() as td:
    with open(os.path.join(td, "all_headers.hpp"), "w") as f:
        f.write("#include <iostream>\n#include <fstream>\n#include <cstdio>\n#include <cstdlib>\n#include <unordered_map>\nusing namespace std;\n"
                '#include "StopWatch.hpp"\n#include "Utils.hpp"\n#include "KmerFileMetaData.hpp"\n#include "KmerNode.hpp"\n')
    inc = ["-I", td, "-I", REF + "/include", "-I", REF + "/src/kmerdb", "-I", REF + "/src"]
    common = [REF + "/src/kmerdb/KmerFileMetaData.cpp", REF + "/src/kmerdb/Utils.cpp"]
    for prog in ("kmerPrefixCounter", "tax_histo", "countTaxidFrequency"):
        subprocess.check_call(["g++", "-std=gnu++17", "-w", "-O2", *REFDEFS, *inc, REF + "/src/%s.cpp" % prog, *common, "-o", os.path.join(td, prog)])
    tree = dm.gunzip_to("tree.dat.gz", os.path.join(td, "tree.dat"))
    recs = dm.parse_fasta(dm.gunzip_to("a.fa.gz", os.path.join(td, "a.fa")))
    for part in (0, 1):
        fa = os.path.join(td, "p%d.fa" % part)
        with open(fa, "w") as f:
            for tid, s in recs[part::2]:
                f.write(">%d\n%s\n" % (tid, s.decode()))
        mid = os.path.join(td, "p%d.kmers" % part)
        subprocess.run([os.path.join(td, "kmerPrefixCounter"), "-i", fa, "-k", "20", "-o", mid, "-l", "0", "-f", "0"], check=True, capture_output=True)
        th = os.path.join(td, "p%d.bin" % part)
        subprocess.run([os.path.join(td, "tax_histo"), "-o", th, "-d", mid + ".0", "-t", tree, "-f", "32"], check=True, capture_output=True)
        with open(th, "rb") as f, gzip.GzipFile(os.path.join(out, "a_p%d_k20.bin.gz" % part), "wb", mtime=0) as g:
            g.write(f.read())
    whole = dm.gunzip_to("a_k20.bin.gz", os.path.join(td, "a_k20.bin"))
    subprocess.run([os.path.join(td, "countTaxidFrequency"), "-i", whole, "-o", os.path.join(td, "a_k20"), "-f", "32"], check=True, capture_output=True)
    with open(os.path.join(td, "a_k20.par.kcnt"), "rb") as f, open(os.path.join(out, "a_k20.par.kcnt"), "wb") as g:
        g.write(f.read())
for fn in sorted(os.listdir(out)):
    print(fn, os.path.getsize(os.path.join(out, fn)))
