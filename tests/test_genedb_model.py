"""CPU: the model of the id-set build (genedb_model.py) against a brute-force double loop, and its union over the gene fixture."""
import os

import numpy as np

import genedb_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENE_BIN = os.path.join(ROOT, "tests", "golden", "gene", "gene.bin")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _brute(records, k):
    db = {}
    for gid, seq in records:
        s = seq.decode("latin-1")
        for i in range(len(s) - k + 1):
            w = s[i:i + k].upper()
            if any(c not in _COMP for c in w):
                continue
            rc = "".join(_COMP[c] for c in reversed(w))
            km = min(int("".join(str("ACGT".index(c)) for c in x), 4) for x in (w, rc))
            db.setdefault(km, set()).add(gid)
    return db


def test_model_equals_brute_force():
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    a = letters[rng.integers(0, 4, 100)].tobytes()
    b = bytearray(letters[rng.integers(0, 4, 100)].tobytes())
    b[10:40] = a[50:80]                      # shared with the first record
    b[60] = ord("N")
    b[70] = ord("-")
    c = bytes(b[5:45]).lower() + b"ACGTACGTACGTACGTACGT" + a[20:60][::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    recs = [(7, a), (3000051781, bytes(b)), (7, c), (1, b"ACG"), (2, b"")]
    assert sum(len(s) for _, s in recs) == 303
    for k in (20, 8, 3):
        want = _brute(recs, k)
        assert gm.kmer_ids(recs, k) == want and len(want) == (32 if k == 3 else len(want)) > 30   # 32: every canonical 3-mer
    assert any(len(v) == 2 for v in _brute(recs, 20).values())


def test_union_over_the_fixture_sorts_its_lists():
    data = open(GENE_BIN, "rb").read()
    k, recs = gm.parse_taxhisto(data)
    assert k == 20 and len(recs) == 25924 and sum(len(l) for _, l in recs) == 38136
    assert any(l != sorted(l) for _, l in recs)            # the fixture's lists are not ascending
    assert gm.to_bytes(dict(recs), k, order=list) == data     # the writer reproduces the file as it is
    db = gm.union({}, recs)
    out = gm.to_bytes(db, k)
    k2, recs2 = gm.parse_taxhisto(out)
    assert k2 == 20 and [km for km, _ in recs2] == [km for km, _ in recs]
    assert all(l2 == sorted(l) for (_, l2), (_, l) in zip(recs2, recs))
    assert sum(len(l) for _, l in recs2) == 38136 and max(max(l) for _, l in recs2) == 3000051781
