"""GPU: a loaded database back out as tax_histo records (lmat_export_*).  The yardstick is the file the database
was built from: the export of a table must be that file, byte for byte -- every k-mer, every list in stored order, nothing extra --
whatever route the records took into the table (files, either image, genomes), whatever the layout and the label modes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import capacity_probes as cp
import dbgen_model as dm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "lmat_amd", "csrc")
E_ARG, E_CAPACITY, E_STATE = -1, -4, -7
SANITY = 0xFFFFFFFFFFFFFFFF
OPTS = dict(tid_cutoff=2, rank_map=os.path.join(G, "ds", "numeric_ranks.txt"), human_kmers=os.path.join(G, "ds", "human_kmers.txt"),
            adaptor_kmers=os.path.join(G, "ds", "adaptor_kmers.txt"))


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
        f.write(struct.pack("<IQQIcI", 29, len(recs), SANITY, 999, b"N", k))
        for i, (km, lst) in enumerate(recs):
            f.write(struct.pack("<QH%dI" % len(lst), km, len(lst), *lst))
            if (i + 1) % 1500 == 0:
                f.write(struct.pack("<Q", SANITY))
    return path


def _export(eng, path, **kw):
    st = eng.export_taxhisto(path, **kw)
    return st, _bytes(path)


@pytest.fixture(scope="module")
def ds_eng():
    """ds/th.bin in a table, shared by the tests that only read it"""
    ds = _ds("ds")
    e = _engine(ds)
    e.build_db(ds["db"], k=20)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ds_records():
    return dm.read_taxhisto(_ds("ds")["db"])[2]


# ---- 1. byte identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ds", "ds2", "ds3"])
def test_export_is_the_input_file(name, tmp_path):
    ds = _ds(name)
    want = _bytes(ds["db"])
    eng = _engine(ds)
    try:
        eng.build_db(ds["db"], k=ds["k"])
        st, got = _export(eng, str(tmp_path / "a.bin"))
        assert got == want
        assert st["records"] == eng.db_size and st["from_buckets"] + st["from_overflow"] == st["records"] and st["passes"] == 1
        img = str(tmp_path / "dev.img")
        eng.save_device_image(img)
    finally:
        eng.close()
    eng = _engine(ds)
    try:
        eng.load_image(img)
        assert _export(eng, str(tmp_path / "b.bin"))[1] == want
    finally:
        eng.close()
    img1 = str(tmp_path / "ingest.img")
    subprocess.check_call([os.path.join(CSRC, "make_db_image"), "-i", ds["db"], "-o", img1, "-k", str(ds["k"]), "-f", ds["idmap"]],
                          stdout=subprocess.DEVNULL)
    eng = _engine(ds)
    try:
        eng.load_image(img1)
        assert _export(eng, str(tmp_path / "c.bin"))[1] == want
    finally:
        eng.close()


# ---- 2. a database shaped by make_db_table's options --------------------------------------------------------------------------------
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


def test_export_of_a_database_built_with_options(tmp_path):
    ds = _ds("ds")
    reads = [l.rstrip("\n") for l in open(os.path.join(G, "ds", "reads.fa")) if not l.startswith(">")]
    eng = _engine(ds)
    eng2 = _engine(ds)
    try:
        eng.build_db(ds["db"], k=20, **OPTS)
        st, (km, off, td) = eng.export_taxhisto()
        n = km.size
        assert n == eng.db_size == st["records"] and off.size == n + 1 and int(off[-1]) == td.size == st["entries"]
        assert np.all(km[1:] > km[:-1])
        lens = np.diff(off).astype(np.int64)
        assert lens.min() >= 1 and st["singletons"] == int((lens == 1).sum())
        stride = int(lens.max())
        counts, tids = eng.lookup(km, stride=stride)
        assert np.array_equal(counts.astype(np.int64), lens)
        lists = [td[int(off[i]):int(off[i + 1])].tolist() for i in range(n)]
        for i in range(n):
            assert tids[i, :lens[i]].tolist() == lists[i], int(km[i])
        have = dict(zip(km.tolist(), lists))
        n_gold = 0
        for line in open(os.path.join(G, "ref_lookup_opts.txt")):
            f = line.split()
            w = [int(x) for x in f[2:]]
            assert have.get(int(f[0]), []) == w, f[0]
            n_gold += 1
        assert n_gold > 100
        # the export as a plain input: the options changed the content once, the file now holds the result
        out = str(tmp_path / "opts.bin")
        eng.export_taxhisto(out)
        eng2.build_db(out, k=20)
        assert eng2.db_size == n
        counts2, tids2 = eng2.lookup(km, stride=stride)
        assert np.array_equal(counts2, counts) and np.array_equal(tids2, tids)
        assert _classify_text(eng2, reads) == _classify_text(eng, reads)
    finally:
        eng.close()
        eng2.close()


# ---- 3. idempotence ---------------------------------------------------------------------------------------------------------------
def test_export_build_export(tmp_path):
    ds = _ds("ds2")
    eng = _engine(ds)
    try:
        eng.build_db(ds["db"], k=20)
        first = _export(eng, str(tmp_path / "1.bin"))[1]
    finally:
        eng.close()
    eng = _engine(ds)
    try:
        eng.build_db(str(tmp_path / "1.bin"), k=20)
        assert _export(eng, str(tmp_path / "2.bin"))[1] == first
    finally:
        eng.close()


# ---- 4. label modes shape the list records, not the stored lists ------------------------------------------------------------------
@pytest.mark.parametrize("modes", [dict(permissive=True), dict(tid_cutoff=2, rank_map=os.path.join(G, "ds", "numeric_ranks.txt"))],
                         ids=["permissive", "runtime_pruning"])
def test_label_modes_leave_the_export_unchanged(modes, tmp_path):
    ds = _ds("ds")
    eng = _engine(ds)
    try:
        eng.set_label_modes(**modes)
        eng.build_db(ds["db"], k=20)
        assert _export(eng, str(tmp_path / "m.bin"))[1] == _bytes(ds["db"])
    finally:
        eng.close()


# ---- 5. passes ----------------------------------------------------------------------------------------------------------------------
def test_passes_do_not_change_the_bytes(ds_eng, tmp_path):
    from lmat_amd import LmatError
    want = _bytes(_ds("ds")["db"])
    st, got = _export(ds_eng, str(tmp_path / "p3.bin"), prefix_bits=3)
    assert got == want and st["passes"] == 8 and st["prefix_bits"] == 3
    # 21 641 pairs take 40 bytes each: 400 000 bytes hold less than half of them, so the split is derived
    st, got = _export(ds_eng, str(tmp_path / "small.bin"), budget_bytes=400_000)
    assert got == want and st["passes"] > 1
    out = str(tmp_path / "refused.bin")
    with pytest.raises(LmatError) as ei:
        ds_eng.export_taxhisto(out, budget_bytes=400_000, prefix_bits=0)
    assert ei.value.code == E_CAPACITY and not os.path.exists(out)


# ---- 6. both sources of a compact table -----------------------------------------------------------------------------------------------
def test_buckets_and_overflow_table(tmp_path):
    """k = 16 at the minimum table size (2^26 / 127 buckets, 32 MiB): 3.4 M 16-mers of random genomes are 6.5 per 12-slot bucket, and
    neighbouring k-mers share their minimizer and so their bucket.  alloc_table's model (cpt_displaced_share) puts 7 % of them into the
    overflow table; a Poisson load alone would still spill 0.4 %.  Every record is compared, none sampled."""
    from lmat_amd import Engine, Params, synth
    tax = synth.make_taxonomy((2, 2, 2, 2, 2, 2), specials=False)
    aux = synth.write_aux_files(str(tmp_path / "aux"), tax)
    rng = np.random.default_rng(1612)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    fa = str(tmp_path / "g.fa")
    with open(fa, "wb") as f:
        for leaf in tax.leaves[:8]:
            f.write(b">%d\n" % leaf)
            f.write(letters[rng.integers(0, 4, 430_000)].tobytes())
            f.write(b"\n")
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        b = eng._builder(fa, aux["tree"], 16)
        try:
            eng._chk(eng.lib.lmat_db_build_from_genomes(eng.ctx, b.h, 32 << 20))
            bk, boff, btd = b.fetch()
        finally:
            b.close()
        assert eng.table_bytes < 64 << 20
        st, (km, off, td) = eng.export_taxhisto()
        assert st["from_overflow"] > 0 and st["from_buckets"] > 0
        assert st["from_overflow"] + st["from_buckets"] == st["records"] == eng.db_size == bk.size > 3_000_000
        assert np.array_equal(km, bk) and np.array_equal(off, boff) and np.array_equal(td, btd)
    finally:
        eng.close()


# ---- 7. wide layout -------------------------------------------------------------------------------------------------------------------
def test_wide_layout(monkeypatch, tmp_path):
    monkeypatch.setenv("LMAT_TABLE_FORMAT", "wide")
    ds = _ds("ds")
    eng = _engine(ds)
    try:
        eng.build_db(ds["db"], k=20)
        st, got = _export(eng, str(tmp_path / "w.bin"))
        assert got == _bytes(ds["db"])
        assert st["from_buckets"] == 0 and st["from_overflow"] == st["records"]
    finally:
        eng.close()


def test_k9_database_is_wide(ds_records, tmp_path):
    """k < 10 has no compact layout: the table is wide whatever the environment says"""
    ds = _ds("ds")
    rng = np.random.default_rng(9)
    kms = np.unique(rng.integers(0, 4 ** 9, 3000, dtype=np.uint64)).tolist()
    lists = [l for _, l in ds_records]
    src = _write_th(str(tmp_path / "k9.bin"), 9, [(km, lists[(7 * i) % len(lists)]) for i, km in enumerate(kms)])
    eng = _engine(ds)
    try:
        eng.build_db(src, k=9)
        st, got = _export(eng, str(tmp_path / "k9_out.bin"), prefix_bits=2)
        assert got == _bytes(src) and st["from_buckets"] == 0 and st["records"] == len(kms)
    finally:
        eng.close()


# ---- 8. exact words -------------------------------------------------------------------------------------------------------------------
def test_exact_words_and_a_long_list(tmp_path):
    from lmat_amd import Engine, Params, synth
    tax = synth.make_taxonomy((3, 4, 4, 4, 4, 3), specials=False)
    aux = synth.write_aux_files(str(tmp_path / "aux"), tax)
    k = 20
    enc = lambda s: int("".join(str("ACGT".index(c)) for c in s), 4)
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    palin = "ACGTACGTAC" + rc("ACGTACGTAC")
    assert rc(palin) == palin
    noncanon = "TTGACCATGGTACCATTGCA"
    assert enc(rc(noncanon)) < enc(noncanon)
    rng = np.random.default_rng(88)
    ids = list(tax.ids)
    long_list = [ids[i] for i in rng.permutation(len(ids))[:300].tolist()]
    recs = {enc(palin): [tax.leaves[5], tax.leaves[3]], enc(noncanon): [tax.leaves[9]], enc("ACGGTCATTGCAAGTCCGTA"): long_list}
    while len(recs) < 12:
        km = int(rng.integers(0, 1 << 40))
        recs.setdefault(km, [ids[int(j)] for j in rng.permutation(len(ids))[:int(rng.integers(1, 12))]])
    src = _write_th(str(tmp_path / "hand.bin"), k, sorted(recs.items()))
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        eng.build_db(src, k=k)
        st, got = _export(eng, str(tmp_path / "hand_out.bin"))
        assert got == _bytes(src)
        assert st["from_overflow"] >= 1 and st["records"] == 12     # the non-canonical word lives in the overflow table
    finally:
        eng.close()


# ---- 9. wide taxonomy, gene ids -----------------------------------------------------------------------------------------------------
def test_wide_taxonomy_set(tmp_path):
    from lmat_amd import Engine, Params
    ps = cp.build_set(str(tmp_path / "wide"), wide=True)
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
        eng.build_db(ps["db"], k=cp.K)
        st, got = _export(eng, str(tmp_path / "wide_out.bin"))
        assert got == _bytes(ps["db"])
        assert st["entries"] > 20 * st["records"]       # lists of hundreds and thousands of 32-bit taxids
    finally:
        eng.close()


def test_gene_database(ds_eng, tmp_path):
    from lmat_amd import Builder, Engine, LmatError, Params
    src = os.path.join(G, "gene", "gene.bin")
    eng = Engine(0, Params.run_rl())
    try:
        eng.build_gene_db(src, k=20)
        assert _export(eng, str(tmp_path / "gene_out.bin"))[1] == _bytes(src)
        b = Builder(ds_eng, 20, _ds("ds")["tree"])
        try:
            with pytest.raises(LmatError) as ei:
                b.add_db(eng)
            assert ei.value.code == E_ARG
        finally:
            b.close()
    finally:
        eng.close()


# ---- 10. a loaded database as an input of a merge -------------------------------------------------------------------------------------
def test_merge_from_a_loaded_database(ds_eng, tmp_path):
    from lmat_amd import Builder
    ds = _ds("ds")
    fa = dm.gunzip_to("a.fa.gz", str(tmp_path / "a.fa"))       # the genomes test_gpu_dbmerge.py adds; the ds tree knows their taxids
    want_fn = str(tmp_path / "from_file.bin")
    st = ds_eng.merge_taxhisto([ds["db"]], ds["tree"], 20, want_fn, fasta=fa)
    assert st["merge"]["records_merged"] + st["distinct_kmers"] > 0 and st["dropped_unknown"] == 0
    want = _bytes(want_fn)
    b = Builder(ds_eng, 20, ds["tree"])
    try:
        b.add_db(ds_eng)
        b.add_fasta(fa)
        b.run()
        b.write_taxhisto(str(tmp_path / "from_db.bin"))
        assert b.merge_stats["inputs"] == 1 and b.merge_stats["records_in"] == ds_eng.db_size
    finally:
        b.close()
    assert _bytes(str(tmp_path / "from_db.bin")) == want
    img = str(tmp_path / "ds.img")
    ds_eng.save_device_image(img)
    out = str(tmp_path / "from_tool.bin")
    r = subprocess.run([os.path.join(CSRC, "build_tax_histo"), "-D", img, "-t", ds["tree"], "-e", ds["depth"], "-w", ds["rank"], "-f", ds["idmap"],
                        "-i", fa, "-k", "20", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _bytes(out) == want


# ---- 11. per-taxid counts -------------------------------------------------------------------------------------------------------------
def test_taxid_counts(ds_eng, ds_records, tmp_path):
    ds = _ds("ds")
    want = {}
    for _, lst in ds_records:
        for t in lst:
            want[t] = want.get(t, 0) + 1
    total = sum(len(l) for _, l in ds_records)
    single = sum(1 for _, l in ds_records if len(l) == 1)
    got = ds_eng.db_taxid_counts()
    assert got["counts"] == want and got["total_tid"] == total and got["singletons"] == single
    img = str(tmp_path / "ds.img")
    ds_eng.save_device_image(img)
    out, prefix = str(tmp_path / "dump.bin"), str(tmp_path / "cnt")
    r = subprocess.run([os.path.join(CSRC, "dump_tax_histo"), "-d", img, "-c", ds["tree"], "-e", ds["depth"], "-w", ds["rank"], "-f", ds["idmap"],
                        "-o", out, "-C", prefix, "-p", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert _bytes(out) == _bytes(ds["db"])
    assert open(prefix + ".par.kcnt").read() == "".join("%d %d\n" % (t, want[t]) for t in sorted(want))
    assert "Total-tid: %d\n" % total in r.stdout and "Singletons: %d\n" % single in r.stdout


# ---- 12. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    from lmat_amd import Engine, LmatError, Params
    ds = _ds("ds")
    eng = _engine(ds)
    try:
        eng._chk(eng.lib.lmat_db_begin(eng.ctx, 20, 0, 0))
        eng._chk(eng.lib.lmat_db_add_taxhisto(eng.ctx, ds["db"].encode()))
        with pytest.raises(LmatError) as ei:
            eng.export_taxhisto(str(tmp_path / "early.bin"))
        assert ei.value.code == E_STATE and not os.path.exists(str(tmp_path / "early.bin"))
        eng._chk(eng.lib.lmat_db_finalize(eng.ctx))
        assert eng.export_taxhisto(str(tmp_path / "late.bin"))["records"] == eng.db_size
    finally:
        eng.close()
    eng = Engine(0, Params.run_rl())
    try:
        eng.synth_taxonomy((2, 2, 2, 2, 2, 2))
        eng.synth_db(2000, k=20)
        with pytest.raises(LmatError) as ei:
            eng.export_taxhisto(str(tmp_path / "synth.bin"))
        assert ei.value.code == E_STATE and not os.path.exists(str(tmp_path / "synth.bin"))
    finally:
        eng.close()
