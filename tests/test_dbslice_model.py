"""CPU: the Python statement of the export filter (tests/dbslice_model.py) against what its three modes must mean -- any / none
partition the records, all lies inside any, the root's subtree is everything -- and, on the closed lists of the reference's own
tax_histo output (tests/golden/dbgen/a_k20.bin), against the LCA: every entry lies under X exactly when the list's LCA does."""
import os

import pytest

import dbgen_model as dm
import dbslice_model as sm
from lmat_amd import synth

DS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ds")


@pytest.fixture(scope="module")
def ds():
    tax = dm.load_tree(os.path.join(DS, "tax.dat"))
    k, count, recs = dm.read_taxhisto(os.path.join(DS, "th.bin"))
    assert k == 20 and count == len(recs) == 21641
    return tax, recs


def _root(tax):
    return next(t for t, p in tax.parent.items() if p == t)


@pytest.mark.parametrize("taxa", [(1007,), (1021,), (1021, 1049), (1007, 1021)])
def test_modes_partition(ds, taxa):
    tax, recs = ds
    any_, _, ca = sm.slice_records(recs, tax, taxa, "any")
    all_, _, cl = sm.slice_records(recs, tax, taxa, "all")
    none_, _, cn = sm.slice_records(recs, tax, taxa, "none")
    ka, kl, kn = (set(km for km, _ in r) for r in (any_, all_, none_))
    assert ka | kn == set(km for km, _ in recs) and not ka & kn
    assert kl <= ka and 0 < len(kl) < len(ka) < len(recs)
    for c, kept in ((ca, any_), (cl, all_), (cn, none_)):
        assert c[0] == len(recs) and c[1] == len(kept) and c[2] == len(recs) - len(kept) and c[3] == c[4] == 0
        assert c[5] == sum(1 for _, l in recs if len(l) > sm.SHORT_LIST)
    assert [km for km, _ in any_] == sorted(ka)


def test_fixture_counts(ds):
    """the figures test_gpu_dbslice.py leans on"""
    tax, recs = ds
    keep = lambda taxa, mode: sm.slice_records(recs, tax, taxa, mode)[2][1]
    assert (keep((1007,), "any"), keep((1007,), "all")) == (11019, 10975)
    assert (keep((1021,), "any"), keep((1021,), "all")) == (5918, 5894)
    assert tax.depth[1021] == 2 and tax.parent[1021] == 1007
    # nested taxa add nothing to the outer one
    for mode in sm.MODES:
        assert sm.slice_records(recs, tax, (1007, 1021), mode)[0] == sm.slice_records(recs, tax, (1007,), mode)[0]


def test_root_is_everything(ds):
    tax, recs = ds
    kept, counts, c = sm.slice_records(recs, tax, (_root(tax),), "any")
    assert kept == recs and c[:5] == [len(recs), len(recs), 0, 0, 0]
    assert sum(counts.values()) == sum(len(l) for _, l in recs)
    assert sm.slice_records(recs, tax, (_root(tax),), "none")[0] == []
    assert sm.slice_records(recs, tax)[0] == recs
    assert sm.file_bytes(20, recs) == open(os.path.join(DS, "th.bin"), "rb").read()


def test_depth_and_length_and_attribution(ds):
    tax, recs = ds
    mind = lambda l: min(tax.depth.get(t, 0) for t in l)
    for d in (1, 2, 4, 5, 6, 7):
        kept, _, c = sm.slice_records(recs, tax, min_lca_depth=d)
        assert [km for km, _ in kept] == [km for km, l in recs if mind(l) >= d] and c[3] == len(recs) - len(kept) and c[2] == c[4] == 0
    for n in (1, 8, 9, 13):
        kept, _, c = sm.slice_records(recs, tax, max_entries=n)
        assert [km for km, _ in kept] == [km for km, l in recs if len(l) <= n] and c[4] == len(recs) - len(kept)
    kept, _, c = sm.slice_records(recs, tax, (1007,), "none", 5, 8)
    inside = sm.in_set(tax, (1007,))
    t = [l for _, l in recs if any(inside(x) for x in l)]
    d = [l for _, l in recs if not any(inside(x) for x in l) and mind(l) < 5]
    n = [l for _, l in recs if not any(inside(x) for x in l) and mind(l) >= 5 and len(l) > 8]
    assert c == [len(recs), len(recs) - len(t) - len(d) - len(n), len(t), len(d), len(n), c[5]] and min(len(t), len(d)) > 0


def test_refusals_and_unknown_ids(ds):
    tax, recs = ds
    with pytest.raises(KeyError):
        sm.slice_records(recs, tax, (999001,), "any")
    with pytest.raises(ValueError):
        sm.slice_records(recs, tax, (1007,), None)
    with pytest.raises(ValueError):
        sm.slice_records(recs, tax, (), "any")
    with pytest.raises(ValueError):
        sm.slice_records(recs, tax, (1007,), "some")
    alien = [(5, [1007, 999001]), (6, [999001])]
    root = _root(tax)
    assert [len(sm.slice_records(alien, tax, (root,), m)[0]) for m in sm.MODES] == [1, 0, 1]
    assert sm.slice_records(alien, tax, min_lca_depth=1)[0] == []


def test_all_is_the_lca_on_closed_lists(tmp_path):
    tax = dm.load_tree(dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    _, _, recs = dm.read_taxhisto(dm.gunzip_to("a_k20.bin.gz", str(tmp_path / "a.bin")))
    lca = {}
    for _, lst in recs:
        key = tuple(sorted(lst))
        if key not in lca:
            closed = synth.lca_closure(tax, key)
            assert sorted(closed) == list(key)          # the reference writes closed lists
            lca[key] = min(closed, key=lambda t: tax.depth[t])
    inner = sorted(t for t in tax.parent if tax.depth[t] in (1, 3, 5))
    checked = 0
    for x in inner[::3]:
        inside = sm.in_set(tax, (x,))
        kept = set(km for km, _ in sm.slice_records(recs, tax, (x,), "all")[0])
        for km, lst in recs:
            assert (km in kept) == inside(lca[tuple(sorted(lst))]), (x, km)
        checked += len(kept)
    assert checked > 0
