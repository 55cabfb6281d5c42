"""The k-mer model the tests own: what a read holds at a k of 1 .. 20, in numpy and from the definitions alone -- no engine, no oracle.

  valid windows   position p is valid when all k bases from p on are one of ACGTacgt
  k-mers          forward-encoded, A C G T = 0 1 2 3, first base in the high bits (as synth.kmers_of has them); the canonical k-mer
                  is the smaller of the window and its reverse complement
  valid_kmers     the number of valid windows
  distinct        the canonical k-mers of the valid windows, each once, in the order of their first positions
  GC bin          tot = the bases covered by at least one valid window, gc = the C/G among them,
                  bin = int(float32(float32(float64(float32(gc) / float32(tot)) * 100.0) / float32(10.0)))   (0 when tot == 0)

The oracle is held to this model at every k (test_kmer_model.py); the model's encoding is held to the reference's own encoder at
k = 9, 11, 17 and 19 (tests/golden/ref_kencode_k*.txt)."""
from collections import namedtuple

import numpy as np

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i     # lower case

Read = namedtuple("Read", "valid fwd rev canon valid_kmers distinct first_pos tot gc bin")


def encode(kmer: bytes) -> int:
    """Forward encoding of a string of valid bases."""
    v = 0
    for c in _CODE[np.frombuffer(kmer, dtype=np.uint8)].tolist():
        assert c < 4
        v = (v << 2) | c
    return v


def revcomp(x: int, k: int) -> int:
    r = 0
    for i in range(k):
        r = (r << 2) | (3 - ((x >> (2 * i)) & 3))
    return r


def gc_bin(gc: int, tot: int) -> int:
    if tot <= 0:
        return 0
    q = np.float32(gc) / np.float32(tot)
    pcnt = np.float32(np.float64(q) * 100.0)
    return int(pcnt / np.float32(10.0))


def model(read: bytes, k: int) -> Read:
    """Everything above for one read.  valid, fwd, rev, canon: one entry per window position (len - k + 1 of them; the k-mer
    entries of invalid windows are 0)."""
    assert 1 <= k <= 20
    codes = _CODE[np.frombuffer(read, dtype=np.uint8)]
    P = codes.size - k + 1
    if P <= 0:
        z = np.zeros(0, dtype=np.uint64)
        return Read(np.zeros(0, dtype=bool), z, z, z, 0, z, np.zeros(0, dtype=np.int64), 0, 0, 0)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    valid = bad[k:] == bad[:-k]                        # no invalid base among the k from p on
    c = np.where(codes > 3, 0, codes).astype(np.uint64)
    fwd = np.zeros(P, dtype=np.uint64)
    rev = np.zeros(P, dtype=np.uint64)
    for i in range(k):
        col = c[i:i + P]
        fwd = (fwd << np.uint64(2)) | col
        rev = rev | ((np.uint64(3) - col) << np.uint64(2 * i))
    fwd, rev = np.where(valid, fwd, np.uint64(0)), np.where(valid, rev, np.uint64(0))
    canon = np.minimum(fwd, rev)
    vp = np.nonzero(valid)[0]
    u, first = np.unique(canon[vp], return_index=True)
    order = np.argsort(first, kind="stable")
    distinct, first_pos = u[order], vp[first[order]]
    cover = np.zeros(codes.size + 1, dtype=np.int64)   # bases under a valid window: +1 at p, -1 at p + k
    np.add.at(cover, vp, 1)
    np.add.at(cover, vp + k, -1)
    covered = np.cumsum(cover[:-1]) > 0
    tot = int(covered.sum())
    gc = int((covered & ((codes == 1) | (codes == 2))).sum())
    return Read(valid, fwd, rev, canon, int(vp.size), distinct, first_pos.astype(np.int64), tot, gc, gc_bin(gc, tot))


def distinct_of(reads, k: int) -> np.ndarray:
    """The distinct canonical k-mers of a list of reads, sorted."""
    parts = [model(r, k).distinct for r in reads]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.uint64)
