"""Python model of the id-set build (gene databases): per canonical k-mer the set of ids of the records that
hold it (kmerPrefixCounter's hash[kmer].insert(gid)), the union with parsed tax_histo files, and the file's bytes.  Shared by
test_genedb_model.py, which holds it against a brute-force loop and the gene fixture, and test_gpu_genedb.py."""
import struct

import numpy as np

SANITY = (1 << 64) - 1
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def canonical_kmers(seq, k):
    """Distinct canonical k-mers (min of forward and reverse complement, A=0 C=1 G=2 T=3, first base in the high bits) of a
    byte string; any byte outside ACGTacgt breaks the run."""
    codes = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]
    out, lo = [], 0
    for hi in list(np.flatnonzero(codes == 255)) + [codes.size]:
        n = hi - lo - k + 1
        if n > 0:
            run = codes[lo:hi].astype(np.uint64)
            fwd = np.zeros(n, dtype=np.uint64)
            rev = np.zeros(n, dtype=np.uint64)
            for j in range(k):
                fwd = (fwd << np.uint64(2)) | run[j:j + n]
                rev |= (np.uint64(3) - run[j:j + n]) << np.uint64(2 * j)
            out.append(np.minimum(fwd, rev))
        lo = hi + 1
    return np.unique(np.concatenate(out)).tolist() if out else []


def kmer_ids(records, k, into=None):
    """{canonical k-mer: set of ids} of [(id, bytes)], added to `into`."""
    db = {} if into is None else into
    for gid, seq in records:
        for km in canonical_kmers(seq, k):
            db.setdefault(km, set()).add(gid)
    return db


def parse_taxhisto(data):
    """-> (k, [(k-mer, [ids in file order])]); checks the header, the sanity words and the file's end."""
    start, count, sanity, version, loc, k = struct.unpack_from("<IQQIcI", data, 0)
    assert (start, sanity, version, loc) == (29, SANITY, 999, b"N")
    pos, recs = 29, []
    for i in range(count):
        km, n = struct.unpack_from("<QH", data, pos)
        recs.append((km, list(struct.unpack_from("<%dI" % n, data, pos + 10))))
        pos += 10 + 4 * n
        if (i + 1) % 1500 == 0:
            assert struct.unpack_from("<Q", data, pos)[0] == SANITY
            pos += 8
    assert pos == len(data)
    return k, recs


def union(db, *files):
    """The ids of every parsed file's records added to db ({k-mer: set})."""
    for recs in files:
        for km, ids in recs:
            db.setdefault(km, set()).update(ids)
    return db


def to_bytes(db, k, order=sorted):
    """The tax_histo file of {k-mer: ids}: records ascending, every list through `order`, the sanity word behind every 1500th."""
    out = [struct.pack("<IQQIcI", 29, len(db), SANITY, 999, b"N", k)]
    for i, km in enumerate(sorted(db)):
        ids = order(db[km])
        out.append(struct.pack("<QH%dI" % len(ids), km, len(ids), *ids))
        if (i + 1) % 1500 == 0:
            out.append(struct.pack("<Q", SANITY))
    return b"".join(out)
