"""CPU: the Python model of the database build (tests/dbgen_model.py) against the files the reference's kmerPrefixCounter +
tax_histo wrote for the fixtures of tests/golden/make_dbgen_goldens.py: every k-mer, every list as a set."""
import pytest

import dbgen_model as dm

CASES = [("a.fa.gz", "a_k20.bin.gz", 20), ("a.fa.gz", "b_k18.bin.gz", 18), ("c.fa.gz", "c_k20.bin.gz", 20)]


@pytest.mark.parametrize("fa,gold,k", CASES)
def test_model_reproduces_the_reference(tmp_path, fa, gold, k):
    tax = dm.load_tree(dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    recs = dm.parse_fasta(dm.gunzip_to(fa, str(tmp_path / "g.fa")))
    kk, count, ref = dm.read_taxhisto(dm.gunzip_to(gold, str(tmp_path / "ref.bin")))
    want, dropped = dm.model(recs, tax, k)
    assert kk == k and count == len(ref)
    kmers = [km for km, _ in ref]
    assert kmers == sorted(kmers) and len(set(kmers)) == len(kmers)
    assert kmers == sorted(want)
    for km, lst in ref:
        assert len(set(lst)) == len(lst)
        assert sorted(lst) == want[km], km
    if fa.startswith("c"):
        assert dropped > 0   # the k-mers 999001 / 999002 own alone: the reference writes no record for them
    else:
        assert dropped == 0


def test_fixtures_hold_what_they_are_for(tmp_path):
    recs = dm.parse_fasta(dm.gunzip_to("c.fa.gz", str(tmp_path / "c.fa")))
    tax = dm.load_tree(dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    tids = [t for t, _ in recs]
    assert len(tids) > len(set(tids))                                  # two records of one taxid
    assert any(len(s) < 18 for _, s in recs)                           # a record shorter than k
    assert any(any(c in s for c in b"acgt") for _, s in recs)          # lower case
    assert any(b"NNNNNNNNNNNN" in s for _, s in recs)                  # a run of N
    unknown = {t for t in tids if t not in tax.parent}
    assert unknown == {999001, 999002}
    own = dm.kmer_owners(recs, 20)
    assert any(999001 in o and len(o) > 1 for o in own.values())       # shares k-mers with known owners
    assert all(o == {999002} for o in own.values() if 999002 in o)     # owns its k-mers alone
    assert all(tax.depth[t] >= 2 for t in tids if t in tax.parent)     # no owner is the root or its child
    want, _ = dm.model(recs, tax, 20)
    assert max(len(l) for l in want.values()) >= 7
