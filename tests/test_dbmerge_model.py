"""CPU: the Python statement of the merge rule and of the per-taxid counts (tests/dbmerge_model.py) against the reference's own
files -- the two part files of tests/golden/make_dbmerge_goldens.py merge into the reference's a_k20.bin, the counts are the
reference's a_k20.par.kcnt -- and the C ABI's new symbols."""
import os

import dbgen_model as dm
import dbmerge_model as mm


def _load(tmp_path):
    tax = dm.load_tree(dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    parts = [dict(dm.read_taxhisto(mm.gunzip_to("a_p%d_k20.bin.gz" % p, str(tmp_path / ("p%d.bin" % p))))[2]) for p in (0, 1)]
    _, _, whole = dm.read_taxhisto(dm.gunzip_to("a_k20.bin.gz", str(tmp_path / "a.bin")))
    return tax, parts, whole


def test_merge_model_reproduces_the_reference(tmp_path):
    tax, parts, whole = _load(tmp_path)
    got, st = mm.merge(tax, parts)
    assert sorted(got) == [km for km, _ in whole]
    for km, lst in whole:
        assert got[km] == sorted(lst), km
    # what the fixture is for: k-mers both parts hold, and merged lists with nodes neither part's list holds
    assert st["records_merged"] >= 4000 and st["records_grown"] >= 4000
    assert st["records_merged"] == len(set(parts[0]) & set(parts[1]))
    assert st["records_one_source"] + st["records_merged"] == len(whole)
    assert any(lst != sorted(lst) for p in parts for lst in p.values())   # the reference's own list order, not ascending


def test_merge_model_is_symmetric_and_splits_three_ways(tmp_path):
    tax = dm.load_tree(dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    recs = dm.parse_fasta(dm.gunzip_to("a.fa.gz", str(tmp_path / "a.fa")))
    want, _ = dm.model(recs, tax, 20)
    parts = [dm.model(recs[i::3], tax, 20)[0] for i in range(3)]
    assert mm.merge(tax, parts)[0] == want == mm.merge(tax, parts[::-1])[0]


def test_counts_model_equals_countTaxidFrequency(tmp_path):
    _, _, whole = _load(tmp_path)
    want = open(os.path.join(mm.GOLD, "a_k20.par.kcnt")).read()
    assert mm.kcnt_text(mm.taxid_counts(dict(whole))) == want
    assert len(want.splitlines()) > 100


def test_library_exports_the_merge_symbols():
    import lmat_amd
    from lmat_amd import capi
    lib = lmat_amd.load_library()
    for name in ("lmat_build_add_taxhisto", "lmat_build_merge_stats", "lmat_build_taxid_counts"):
        assert hasattr(lib, name) and name in capi.EXPORTED, name
    assert hasattr(capi.Builder, "add_taxhisto") and hasattr(capi.Builder, "taxid_counts") and hasattr(capi.Engine, "merge_taxhisto")
