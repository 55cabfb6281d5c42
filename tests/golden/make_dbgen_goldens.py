#!/usr/bin/env python3
"""Generates the database-build fixtures under tests/golden/dbgen/ (run in the build container, where the reference lies):

  tree.dat.gz            the taxonomy of synth.make_taxonomy((2,2,2,2,2,2), specials=False): 64 strains under 32 species ...
  a.fa.gz, c.fa.gz       genome FASTA, '>' + taxid headers, one sequence line per record (the reference reads one token)
  a_k20.bin.gz           the tax_histo file the REFERENCE's kmerPrefixCounter (-l 0 -f 0) + tax_histo (-f 32) make of a.fa, k = 20
  b_k18.bin.gz           ... of a.fa, k = 18
  c_k20.bin.gz           ... of c.fa, k = 20
  (a) strains with three N each, lower-case stretches, N runs, one record shorter than k, two records of one taxid
  (c) = (a) + two owners the tree does not know: 999001 shares a stretch with a known strain, 999002 owns its k-mers alone
Both programs are compiled from /root/reference into a temporary directory (with a stand-in for the header CMake would
generate); only inputs and the reference's output files are stored, no reference source travels.  No owner is the root or a
child of the root: the reference asserts on those (TaxTree.hpp:204)."""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
sys.path.insert(0, root)
from lmat_amd import synth  # noqa: E402

REF = os.environ.get("LMAT_REF", "/root/reference")
REFDEFS = "-DIDX_CONFIG=2027 -DTID_SIZE=16 -DDBTID_T=uint16_t -DUSE_SORTED_DB=1 -DWITH_PJMALLOC=0".split()
G = 360
out = os.path.join(here, "dbgen")
os.makedirs(out, exist_ok=True)

tax = synth.make_taxonomy((2, 2, 2, 2, 2, 2), specials=False)
genomes = synth.make_genomes(tax, G, 2002)
rng = np.random.default_rng(616)
letters = np.frombuffer(b"ACGT", dtype=np.uint8)


def text_of(codes):
    s = bytearray(letters[codes].tobytes())
    for p in rng.integers(0, len(s), 3):
        s[int(p)] = ord("N")
    return s


records = []
for n, leaf in enumerate(tax.leaves):
    s = text_of(genomes[leaf])
    if n % 5 == 1:   # a lower-case stretch
        lo = int(rng.integers(0, G - 80))
        s[lo:lo + 80] = bytes(s[lo:lo + 80]).lower()
    if n % 7 == 2:   # a run of N
        lo = int(rng.integers(0, G - 30))
        s[lo:lo + 12] = b"N" * 12
    records.append((leaf, bytes(s)))
records.insert(5, (tax.leaves[9], b"ACGTTGCAAC"))                                   # shorter than k
records.append((tax.leaves[3], bytes(text_of(synth.make_genomes(tax, 200, 77)[tax.leaves[40]]))))   # a second record of one taxid, sharing with another strain
rec_c = list(records)
shared = records[12][1][40:220]
rec_c.append((999001, shared + bytes(letters[rng.integers(0, 4, 150)].tobytes())))
rec_c.append((999002, bytes(letters[rng.integers(0, 4, 200)].tobytes())))


def write_fasta(path, recs):
    with open(path, "w") as f:
        for tid, s in recs:
            f.write(">%d\n%s\n" % (tid, s.decode()))


with tempfile.TemporaryDirectory() as td:
    paths = synth.write_aux_files(td, tax)
    with open(os.path.join(td, "all_headers.hpp"), "w") as f:
        f.write("#include <iostream>\n#include <unordered_map>\nusing namespace std;\n"
                '#include "StopWatch.hpp"\n#include "Utils.hpp"\n#include "KmerFileMetaData.hpp"\n#include "KmerNode.hpp"\n')
    inc = ["-I", td, "-I", REF + "/include", "-I", REF + "/src/kmerdb"]
    common = [REF + "/src/kmerdb/KmerFileMetaData.cpp", REF + "/src/kmerdb/Utils.cpp"]
    for prog in ("kmerPrefixCounter", "tax_histo"):
        subprocess.check_call(["g++", "-std=gnu++17", "-w", "-O2", *REFDEFS, *inc, REF + "/src/%s.cpp" % prog, *common, "-o", os.path.join(td, prog)])
    fa_a, fa_c = os.path.join(td, "a.fa"), os.path.join(td, "c.fa")
    write_fasta(fa_a, records)
    write_fasta(fa_c, rec_c)
    for name, fa, k in (("a_k20", fa_a, 20), ("b_k18", fa_a, 18), ("c_k20", fa_c, 20)):
        mid = os.path.join(td, name + ".kmers")
        subprocess.run([os.path.join(td, "kmerPrefixCounter"), "-i", fa, "-k", str(k), "-o", mid, "-l", "0", "-f", "0"], check=True, capture_output=True)
        th = os.path.join(td, name + ".bin")
        r = subprocess.run([os.path.join(td, "tax_histo"), "-o", th, "-d", mid + ".0", "-t", paths["tree"], "-f", "32"], check=True, capture_output=True, text=True)
        tail = [l for l in r.stdout.splitlines() if l.startswith(("total taxids", "singletons", "num mapping"))]
        print(name, os.path.getsize(th), "bytes;", "; ".join(tail))
        with open(th, "rb") as f, gzip.GzipFile(os.path.join(out, name + ".bin.gz"), "wb", mtime=0) as g:
            g.write(f.read())
    for src, dst in ((fa_a, "a.fa.gz"), (fa_c, "c.fa.gz"), (paths["tree"], "tree.dat.gz")):
        with open(src, "rb") as f, gzip.GzipFile(os.path.join(out, dst), "wb", mtime=0) as g:
            g.write(f.read())
for fn in sorted(os.listdir(out)):
    print(fn, os.path.getsize(os.path.join(out, fn)))
