"""GPU: a taxonomic slice of a loaded database, filtered on the device ahead of the fetch (lmat_export_set_filter, lmat_db_from_export;
DESIGN section 15).  The yardstick is tests/dbslice_model.py over the records of the file the database was built from: the slice's
file must be the model's records in the file format, byte for byte, and the six counters the model's.  Every test first asserts what
the MODEL gives for its fixture, so that none passes on an empty or a whole slice."""
import os
import struct
import subprocess

import numpy as np
import pytest

import capacity_probes as cp
import dbgen_model as dm
import dbslice_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "lmat_amd", "csrc")
E_ARG, E_CAPACITY, E_TAXONOMY, E_STATE = -1, -4, -5, -7
STAT_KEYS = ("scanned", "kept", "dropped_taxon", "dropped_depth", "dropped_length", "wave_lists")
LEAF = 1805          # a strain of ds that is neither under 1021 nor alone in its lists (asserted below)


def _ds(name):
    d = os.path.join(G, name)
    return dict(tree=os.path.join(d, "tax.dat"), depth=os.path.join(d, "depth.dat"), rank=os.path.join(d, "rank.txt"),
                idmap=os.path.join(d, "map32to16.txt"), db=os.path.join(d, "th.bin"), k=18 if name == "ds3" else 20)


def _engine(ds):
    from lmat_amd import Engine, Params
    e = Engine(0, Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    return e


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _write_th(path, k, recs):
    with open(path, "wb") as f:
        f.write(sm.file_bytes(k, recs))
    return path


class Fixture:
    """an engine holding a tax_histo file, the file's records, its tree, and the model's slices (computed once per filter)"""

    def __init__(self, eng, tax, k, recs):
        self.eng, self.tax, self.k, self.recs, self.memo = eng, tax, k, recs, {}

    def model(self, **flt):
        key = (tuple(flt.get("taxa", ())), flt.get("mode"), flt.get("min_lca_depth", 0), flt.get("max_entries", 0))
        if key not in self.memo:
            self.memo[key] = sm.slice_records(self.recs, self.tax, *key)
        return self.memo[key]

    def check(self, tmp_path, prefix_bits=-1, fetch=True, **flt):
        """the slice to a file and into host memory, against the model: bytes, records, per-taxid counts, the six counters"""
        from lmat_amd import Export
        kept, counts, six = self.model(**flt)
        x = Export(self.eng)
        try:
            x.set_options(0, prefix_bits)
            x.set_filter(**flt)
            out = str(tmp_path / "slice.bin")
            st = x.run(out)
            assert _bytes(out) == sm.file_bytes(self.k, kept)
            assert st["passes"] == (1 << max(prefix_bits, 0)) and st["records"] == len(kept)
            assert st["entries"] == sum(len(l) for _, l in kept) and st["singletons"] == sum(1 for _, l in kept if len(l) == 1)
            fs = x.filter_stats()
            assert [fs[n] for n in STAT_KEYS] == six and fs["scanned"] == self.eng.db_size
            t, c = x.taxid_counts()
            assert dict(zip(t.tolist(), c.tolist())) == counts and np.all(t[1:] > t[:-1])
            if fetch:
                x.run(None)
                km, off, td = x.fetch()
                assert km.tolist() == [r[0] for r in kept]
                assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(l) for _, l in kept])]).astype(np.uint64))
                assert td.tolist() == [t for _, l in kept for t in l]
                assert [x.filter_stats()[n] for n in STAT_KEYS] == six
            return st, fs
        finally:
            x.close()


@pytest.fixture(scope="module")
def ds():
    d = _ds("ds")
    e = _engine(d)
    e.build_db(d["db"], k=20)
    k, count, recs = dm.read_taxhisto(d["db"])
    assert count == e.db_size == 21641
    yield Fixture(e, dm.load_tree(d["tree"]), k, recs)
    e.close()


# ---- 1. model equality ----------------------------------------------------------------------------------------------------------------
TAXA = [(1007,), (1021,), (1021, 1049), (1007, 1021), (LEAF,), (1,)]


@pytest.mark.parametrize("prefix_bits", [-1, 3])
@pytest.mark.parametrize("mode", sm.MODES)
@pytest.mark.parametrize("taxa", TAXA, ids=lambda t: "_".join(map(str, t)))
def test_slice_equals_the_model(ds, tmp_path, taxa, mode, prefix_bits):
    kept, _, six = ds.model(taxa=taxa, mode=mode)
    lens = [len(l) for _, l in ds.recs]
    assert (len(ds.recs), min(lens), max(lens), lens.count(1), lens.count(8), lens.count(9)) == (21641, 1, 13, 9464, 4, 18)
    want = {((1007,), "any"): 11019, ((1007,), "all"): 10975, ((1021,), "any"): 5918, ((1021,), "all"): 5894, ((1007, 1021), "any"): 11019,
            ((1,), "any"): 21641, ((1,), "all"): 21641, ((1,), "none"): 0}
    if (taxa, mode) in want:
        assert len(kept) == want[(taxa, mode)]
    if taxa == (1007,):    # more than two sanity words, and records dropped before the first of them
        assert len(kept) > 3000 and kept[1499][0] != ds.recs[1499][0]
    if taxa == (LEAF,):
        assert not ds.tax.parent[LEAF] == LEAF and LEAF not in ds.tax.parent.values() and 0 < len(ds.model(taxa=taxa, mode="all")[0]) < len(ds.model(taxa=taxa, mode="any")[0])
    assert six[5] == sum(1 for n in lens if n > 8) > 0
    ds.check(tmp_path, prefix_bits, fetch=prefix_bits < 0, taxa=taxa, mode=mode)


def test_k18_and_a_device_image(tmp_path):
    d = _ds("ds3")
    k, _, recs = dm.read_taxhisto(d["db"])
    tax = dm.load_tree(d["tree"])
    taxon = next(t for t in sorted(tax.parent) if tax.depth[t] == 1)
    eng = _engine(d)
    try:
        eng.build_db(d["db"], k=18)
        fx = Fixture(eng, tax, k, recs)
        kept = fx.model(taxa=(taxon,), mode="all")[0]
        assert k == 18 and 0 < len(kept) < len(recs)
        fx.check(tmp_path, taxa=(taxon,), mode="all")
        img = str(tmp_path / "dev.img")
        eng.save_device_image(img)
    finally:
        eng.close()
    eng = _engine(d)
    try:
        eng.load_image(img)
        fx.eng = eng
        fx.check(tmp_path, 2, taxa=(taxon,), mode="all")
    finally:
        eng.close()


# ---- 2. depth and length boundaries ---------------------------------------------------------------------------------------------------
def test_depth_and_length_boundaries(ds, tmp_path):
    mind = [min(ds.tax.depth[t] for t in l) for _, l in ds.recs]
    assert sorted(set(mind)) == [1, 3, 4, 5, 6] and mind.count(1) == 40
    for d in (1, 2, 4, 5, 6, 7):
        kept, _, six = ds.model(min_lca_depth=d)
        assert len(kept) == sum(1 for m in mind if m >= d) and six[3] == len(ds.recs) - len(kept)
        ds.check(tmp_path, fetch=False, min_lca_depth=d)
    assert len(ds.model(min_lca_depth=1)[0]) == 21641 and len(ds.model(min_lca_depth=2)[0]) == 21601 and ds.model(min_lca_depth=7)[0] == []
    for n in (1, 8, 9, 13):
        kept, _, six = ds.model(max_entries=n)
        assert len(kept) == sum(1 for _, l in ds.recs if len(l) <= n) and six[4] == len(ds.recs) - len(kept)
        ds.check(tmp_path, fetch=False, max_entries=n)
    assert len(ds.model(max_entries=9)[0]) - len(ds.model(max_entries=8)[0]) == 18 and len(ds.model(max_entries=13)[0]) == 21641
    # all three tests at once: a record failing several is charged to the first of taxon, depth, length
    flt = dict(taxa=(1007,), mode="none", min_lca_depth=5, max_entries=8)
    six = ds.model(**flt)[2]
    alone = [ds.model(taxa=(1007,), mode="none")[2][2], ds.model(min_lca_depth=5)[2][3], ds.model(max_entries=8)[2][4]]
    assert six[2] == alone[0] and 0 < six[3] < alone[1] and 0 <= six[4] < alone[2] and six[1] > 0
    ds.check(tmp_path, **flt)
    ds.check(tmp_path, 3, fetch=False, **flt)
    flt = dict(taxa=(1021,), mode="none", min_lca_depth=4, max_entries=3)      # ... and every counter in use
    assert ds.model(**flt)[2] == [21641, 9748, 5918, 336, 5639, 184]
    ds.check(tmp_path, **flt)


# ---- 3. identity and empty -------------------------------------------------------------------------------------------------------------
def test_identity_and_empty(ds, tmp_path):
    from lmat_amd import Export
    whole = _bytes(_ds("ds")["db"])
    assert ds.model(taxa=(1,), mode="any")[0] == ds.recs and ds.model(taxa=(1,), mode="none")[0] == []
    x = Export(ds.eng)
    try:
        out = str(tmp_path / "o.bin")
        x.set_filter(taxa=(1,), mode="any")
        assert x.run(out)["records"] == 21641 and _bytes(out) == whole
        x.set_filter(taxa=(1,), mode="none")
        st = x.run(out)
        assert st["records"] == st["entries"] == 0 and _bytes(out) == struct.pack("<IQQIcI", 29, 0, 0xFFFFFFFFFFFFFFFF, 999, b"N", 20)
        assert x.filter_stats()["scanned"] == 21641 and x.filter_stats()["dropped_taxon"] == 21641
        x.run(None)
        km, off, td = x.fetch()
        assert km.size == 0 and td.size == 0 and off.tolist() == [0] and x.taxid_counts()[0].size == 0
        x.clear_filter()
        st = x.run(out)
        assert _bytes(out) == whole and st["passes"] == 1 and st["records"] == 21641
        fs = x.filter_stats()
        assert [fs[n] for n in STAT_KEYS] == [21641, 21641, 0, 0, 0, 0] and fs["ms_select"] == 0
        x.set_filter(taxa=(1007,), mode="all")
        x.set_filter()                          # every test off: no filter
        assert x.run(out)["records"] == 21641 and _bytes(out) == whole
    finally:
        x.close()
    # the keywords of the engine's own calls
    st = ds.eng.export_taxhisto(str(tmp_path / "e.bin"), taxa=[1021], mode="all")
    assert st["records"] == st["filter"]["kept"] == 5894 and _bytes(str(tmp_path / "e.bin")) == sm.file_bytes(20, ds.model(taxa=(1021,), mode="all")[0])
    assert "filter" not in ds.eng.export_taxhisto(str(tmp_path / "f.bin"))
    got = ds.eng.db_taxid_counts(taxa=[1021], mode="all")
    kept, counts, _ = ds.model(taxa=(1021,), mode="all")
    assert got["counts"] == counts and got["total_tid"] == sum(len(l) for _, l in kept)


# ---- 4. the wave path, exact words, ids the tree lacks ---------------------------------------------------------------------------------
ALIEN = 999001


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    from lmat_amd import Engine, Params, synth
    d = tmp_path_factory.mktemp("dbslice_hand")
    tax = synth.make_taxonomy((3, 4, 4, 4, 4, 3), specials=False)
    aux = synth.write_aux_files(str(d / "aux"), tax)
    with open(aux["idmap"], "a") as f:              # a mapped id the tree does not hold
        f.write("%d %d\n" % (ALIEN, max(tax.id16.values()) + 1))      # the ingest takes codes up to the map's size + 1
    k = 20
    enc = lambda s: int("".join(str("ACGT".index(c)) for c in s), 4)
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    palin = "ACGTACGTAC" + rc("ACGTACGTAC")
    noncanon = "TTGACCATGGTACCATTGCA"
    assert rc(palin) == palin and enc(rc(noncanon)) < enc(noncanon)
    rng = np.random.default_rng(1588)
    ids = list(tax.ids)
    pick = lambda n: [ids[i] for i in rng.permutation(len(ids))[:n].tolist()]
    lists = [pick(300), pick(8), pick(9), pick(64), pick(65), [tax.leaves[5], tax.leaves[3]], [tax.leaves[9]], [tax.leaves[11], ALIEN], [ALIEN],
             pick(3), pick(5), pick(12)]
    kms = [enc("ACGGTCATTGCAAGTCCGTA")] + [int(x) for x in rng.integers(0, 1 << 40, 4)] + [enc(palin), enc(noncanon)] + [int(x) for x in rng.integers(0, 1 << 40, 5)]
    assert len(set(kms)) == len(lists) == 12
    recs = sorted(zip(kms, lists))
    src = _write_th(str(d / "hand.bin"), k, recs)
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
    eng.build_db(src, k=k)
    fx = Fixture(eng, tax, k, recs)
    fx.long_list, fx.src = lists[0], src
    yield fx
    eng.close()


def test_wave_path_and_exact_words(hand, tmp_path):
    tax, long_list = hand.tax, hand.long_list
    inside = sm.in_set(tax, (tax.children[1][0],))
    n_in = sum(1 for t in long_list if inside(t))
    assert 0 < n_in < 300
    st, fs = hand.check(tmp_path)                       # no filter: the file itself, the non-canonical word from the overflow table
    assert _bytes(str(tmp_path / "slice.bin")) == _bytes(hand.src) and st["from_overflow"] >= 1 and fs["wave_lists"] == 0
    has_long = lambda **flt: any(l == long_list for _, l in hand.model(**flt)[0])
    sk = (tax.children[1][0],)
    free_leaf = next(t for t in tax.leaves if t not in long_list)
    assert has_long(taxa=sk, mode="any") and not has_long(taxa=sk, mode="all") and has_long(taxa=(free_leaf,), mode="none")
    for flt in (dict(taxa=sk, mode="any"), dict(taxa=sk, mode="all"), dict(taxa=sk, mode="none"), dict(taxa=(free_leaf,), mode="none"),
                dict(taxa=(free_leaf,), mode="any")):
        st, fs = hand.check(tmp_path, **flt)
        assert fs["wave_lists"] == 5                    # 300, 9, 64, 65 and 12 entries; the list of 8 is its lane's
    for n, kept in ((64, 10), (65, 11), (299, 11), (300, 12)):
        assert len(hand.model(max_entries=n)[0]) == kept
        hand.check(tmp_path, max_entries=n)
    hand.check(tmp_path, 4, taxa=sk, mode="any", max_entries=299)


def test_ids_the_tree_lacks(hand, tmp_path):
    """[leaf, ALIEN] and [ALIEN]: the id counts as outside S and as depth 0, in a list and as a singleton payload"""
    kept = lambda **flt: [l for _, l in hand.model(**flt)[0] if ALIEN in l]
    leaf = hand.tax.leaves[11]
    assert kept(taxa=(1,), mode="any") == [[leaf, ALIEN]] and kept(taxa=(1,), mode="all") == [] and kept(taxa=(1,), mode="none") == [[ALIEN]]
    assert kept(min_lca_depth=1) == [] and len(hand.model(min_lca_depth=1)[0]) < 10
    for flt in (dict(taxa=(1,), mode="any"), dict(taxa=(1,), mode="all"), dict(taxa=(1,), mode="none"), dict(min_lca_depth=1), dict(taxa=(leaf,), mode="all")):
        hand.check(tmp_path, **flt)


# ---- 5. wide taxonomy: pair lists ---------------------------------------------------------------------------------------------------------
def test_wide_taxonomy(tmp_path):
    from lmat_amd import Engine, Params
    ps = cp.build_set(str(tmp_path / "wide"), wide=True)
    k, _, recs = dm.read_taxhisto(ps["db"])
    tax = ps["tax"]
    assert len(tax.ids) > 65534 and max(len(l) for _, l in recs) > 1000
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
        eng.build_db(ps["db"], k=cp.K)
        fx = Fixture(eng, tax, k, recs)
        taxon = 2057        # a species with its 66 strains: half of the lists that touch it lie wholly inside
        assert tax.depth[taxon] == 5 and len(recs) == 182
        assert [len(fx.model(taxa=(taxon,), mode=m)[0]) for m in sm.MODES] == [150, 75, 32]
        for mode in sm.MODES:
            st, fs = fx.check(tmp_path, fetch=mode == "all", taxa=(taxon,), mode=mode)
            assert fs["wave_lists"] > 0
    finally:
        eng.close()


# ---- 6. a derived database -----------------------------------------------------------------------------------------------------------------
def _classify_text(eng, reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    blob = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
    dr = eng.upload_reads((blob, off))
    res, cands = eng.classify(dr)
    txt = eng.format_out(res, cands, (blob, off))
    dr.free()
    return txt


def test_derived_database(ds, tmp_path):
    d = _ds("ds")
    kept, _, six = ds.model(taxa=(1007,), mode="none")
    want = sm.file_bytes(20, kept)
    keys = set(km for km, _ in kept)
    dropped = [km for km, _ in ds.recs if km not in keys]
    assert len(kept) == 21641 - 11019 and len(dropped) == 11019
    reads = [l.rstrip("\n") for l in open(os.path.join(G, "ds", "reads.fa")) if not l.startswith(">")]
    eng, ref = _engine(d), _engine(d)
    try:
        st = eng.derive_db(ds.eng, taxa=[1007], mode="none")
        assert [st["filter"][n] for n in STAT_KEYS] == six and eng.db_size == len(kept)
        out = str(tmp_path / "derived.bin")
        assert eng.export_taxhisto(out)["records"] == len(kept) and _bytes(out) == want
        counts, tids = eng.lookup(np.array(dropped[::len(dropped) // 64][:64], dtype=np.uint64), stride=13)
        assert counts.size == 64 and not counts.any()
        some = kept[::len(kept) // 64][:64]
        counts, tids = eng.lookup(np.array([km for km, _ in some], dtype=np.uint64), stride=13)
        for i, (_, lst) in enumerate(some):
            assert counts[i] == len(lst) and tids[i, :len(lst)].tolist() == lst
        assert max(len(l) for _, l in some) > 1
        ref.build_db(_write_th(str(tmp_path / "slice.bin"), 20, kept), k=20)
        txt = _classify_text(eng, reads)
        assert txt == _classify_text(ref, reads) and txt != _classify_text(ds.eng, reads)
    finally:
        eng.close()
        ref.close()


# ---- 7. the tool ---------------------------------------------------------------------------------------------------------------------------
def test_tool(ds, tmp_path):
    d = _ds("ds")
    kept, counts, six = ds.model(taxa=(1021,), mode="all")
    assert len(kept) == 5894
    img = str(tmp_path / "ds.img")
    ds.eng.save_device_image(img)
    out, prefix = str(tmp_path / "dump.bin"), str(tmp_path / "cnt")
    r = subprocess.run([os.path.join(CSRC, "dump_tax_histo"), "-d", img, "-c", d["tree"], "-e", d["depth"], "-w", d["rank"], "-f", d["idmap"],
                        "-o", out, "-C", prefix, "-T", "1021", "-M", "all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _bytes(out) == sm.file_bytes(20, kept)
    assert open(prefix + ".par.kcnt").read() == "".join("%d %d\n" % (t, counts[t]) for t in sorted(counts))
    assert "kmer count: 5894\n" in r.stdout and "Total-tid: %d\n" % sum(len(l) for _, l in kept) in r.stdout
    assert "slice: scanned %d kept %d dropped: taxon %d depth %d length %d; long lists %d;" % tuple(six) in r.stdout
    # -T alone means any; taxa separated by commas or given twice
    r = subprocess.run([os.path.join(CSRC, "dump_tax_histo"), "-d", img, "-c", d["tree"], "-e", d["depth"], "-w", d["rank"], "-f", d["idmap"],
                        "-o", out, "-T", "1021,1049", "-T", "1007", "-N", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _bytes(out) == sm.file_bytes(20, ds.model(taxa=(1021, 1049, 1007), mode="any", max_entries=8)[0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(code, call, *words):
    from lmat_amd import LmatError
    with pytest.raises(LmatError) as ei:
        call()
    assert ei.value.code == code, str(ei.value)
    assert len(str(ei.value)) > 10 and all(w in str(ei.value) for w in words), str(ei.value)


def test_refusals(ds, tmp_path):
    import ctypes as C
    from lmat_amd import Engine, Export, Params
    from lmat_amd.capi import ExportFilter
    x = Export(ds.eng)
    try:
        _refused(E_TAXONOMY, lambda: x.set_filter(taxa=(1007, 999001), mode="any"), "999001")
        _refused(E_ARG, lambda: x.set_filter(taxa=(1007,)), "mode")
        _refused(E_ARG, lambda: x.set_filter(mode="all"), "taxid")
        _refused(E_ARG, lambda: x.set_filter(taxa=(1007,), mode="some"))
        t = (C.c_uint32 * 1)(1007)
        for mode in (4, -1):
            f = ExportFilter(t, 1, mode, 0, 0)
            _refused(E_ARG, lambda: x._chk(x.lib.lmat_export_set_filter(x.h, C.byref(f))), "mode")
        _refused(E_STATE, lambda: x.filter_stats())
        # a refused filter leaves the export as it was: no filter
        out = str(tmp_path / "o.bin")
        assert x.run(out)["records"] == 21641 and _bytes(out) == _bytes(_ds("ds")["db"])
        # 21 641 pairs take 48 bytes each with a filter
        x.set_options(400_000, 0)
        x.set_filter(taxa=(1007,), mode="any")
        refused = str(tmp_path / "refused.bin")
        _refused(E_CAPACITY, lambda: x.run(refused), "budget")
        assert not os.path.exists(refused)
        x.set_options(400_000, -1)
        assert x.run(refused)["passes"] > 1 and _bytes(refused) == sm.file_bytes(20, ds.model(taxa=(1007,), mode="any")[0])
        x.set_options(0, -1)
        _refused(E_ARG, lambda: x.into(ds.eng), "context")
        bare = Engine(0, Params.run_rl())
        try:
            _refused(E_STATE, lambda: x.into(bare), "taxonomy")
        finally:
            bare.close()
        dst = _engine(_ds("ds"))
        try:
            x.set_filter(taxa=(1,), mode="none")
            _refused(E_ARG, lambda: x.into(dst), "empty")
            x.set_filter(taxa=(1049,), mode="all")
            x.into(dst)                                  # ... and the same objects then work
            assert dst.db_size == len(ds.model(taxa=(1049,), mode="all")[0]) > 0
        finally:
            dst.close()
    finally:
        x.close()
    gene = Engine(0, Params.run_rl())
    try:
        gene.build_gene_db(os.path.join(G, "gene", "gene.bin"), k=20)
        x = Export(gene)
        try:
            _refused(E_ARG, lambda: x.set_filter(max_entries=4), "gene")
            _refused(E_ARG, lambda: x.set_filter(), "gene")
        finally:
            x.close()
    finally:
        gene.close()
