"""Python model of the database build (kmerPrefixCounter + tax_histo), shared by test_dbgen_model.py and test_gpu_dbgen.py:
synth.kmers_of over the runs of valid bases of every record, then synth.lca_closure over the owners the tree knows.
test_dbgen_model.py holds it against the reference's own output files; that licenses it for shapes the fixtures do not hold."""
import gzip
import os
import struct

import numpy as np

from lmat_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbgen")
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def gunzip_to(name, dst):
    with gzip.open(os.path.join(GOLD, name), "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    return dst


def parse_fasta(path):
    """-> [(taxid, bytes)]; a sequence may span lines."""
    recs = []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if not line:
                continue
            if line.startswith(b">"):
                recs.append([int(line[1:].split()[0]), b""])
            else:
                recs[-1][1] += line
    return [(t, s) for t, s in recs]


def load_tree(path):
    """-> synth.Taxonomy-like object with parent / depth / path (what lca_closure needs) from a tree file."""
    t = synth.Taxonomy()
    lines = open(path).read().split("\n")[3:]
    par = {}
    for i in range(0, len(lines) - 1, 2):
        tok = lines[i].split()
        if len(tok) >= 3:
            par[int(tok[0])] = int(tok[-1])
    t.parent = par
    for tid in par:
        d, x = 0, tid
        while par[x] != x:
            x = par[x]
            d += 1
        t.depth[tid] = d
    return t


def kmer_owners(records, k):
    """{canonical k-mer: set of owner taxids}: any byte outside ACGTacgt breaks the run."""
    own = {}
    for tid, seq in records:
        codes = _CODE[np.frombuffer(seq, dtype=np.uint8)]
        cuts = np.flatnonzero(codes == 255)
        lo = 0
        for hi in list(cuts) + [codes.size]:
            if hi - lo >= k:
                for km in np.unique(synth.kmers_of(codes[lo:hi], k)).tolist():
                    own.setdefault(km, set()).add(tid)
            lo = hi + 1
    return own


def model(records, tax, k):
    """-> ({k-mer: sorted taxid list} for k-mers with a known owner, number of k-mers dropped because no owner is known)."""
    out, dropped, cache = {}, 0, {}
    for km, owners in kmer_owners(records, k).items():
        key = tuple(sorted(o for o in owners if o in tax.parent))
        if not key:
            dropped += 1
            continue
        if key not in cache:
            cache[key] = sorted(synth.lca_closure(tax, key))
        out[km] = cache[key]
    return out, dropped


def read_taxhisto(path):
    """-> (k, header count, [(k-mer, [taxids in file order])]); checks the sanity words and that the file ends with the last record."""
    data = open(path, "rb").read()
    start, count, sanity, version, loc, k = struct.unpack_from("<IQQIcI", data, 0)
    assert (start, sanity, version, loc) == (29, synth.SANITY, 999, b"N")
    pos, recs = 29, []
    for i in range(count):
        km, n = struct.unpack_from("<QH", data, pos)
        pos += 10
        recs.append((km, list(struct.unpack_from("<%dI" % n, data, pos))))
        pos += 4 * n
        if (i + 1) % 1500 == 0:
            assert struct.unpack_from("<Q", data, pos)[0] == synth.SANITY
            pos += 8
    assert pos == len(data), (pos, len(data))
    return k, count, recs
