"""GPU: gene databases built from gene FASTA -- the id-set mode of the builder (lmat_genebuild_create, dbgen.hip; DESIGN section
13) -- against the Python model genedb_model.py, which test_genedb_model.py pins to a brute-force loop and to the gene fixture."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import genedb_model as gm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "build_tax_histo")
GENE_BIN = os.path.join(ROOT, "tests", "golden", "gene", "gene.bin")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
E_ARG, E_IO, E_CAPACITY = -1, -2, -4
RC = bytes.maketrans(b"ACGT", b"TGCA")
BIG_ID = 3000051781                      # the largest id of the gene fixture


def _rand(rng, n):
    return LETTERS[rng.integers(0, 4, n)].tobytes()


@pytest.fixture(scope="module")
def eng():
    from lmat_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _write_fasta(path, recs, width=0):
    with open(path, "wb") as f:
        for gid, s in recs:
            f.write(b">%d\n" % gid)
            for j in range(0, len(s), width or max(len(s), 1)):
                f.write(s[j:j + (width or len(s))] + b"\n")
    return path


def _case1():
    """Gene-shaped text: 300 records of 21..40 bases back to back, and every special record of the issue's case 1."""
    rng = np.random.default_rng(13)
    recs = [(1000 + 7 * i, _rand(rng, int(rng.integers(21, 41)))) for i in range(300)]
    x, s = _rand(rng, 30), _rand(rng, 24)
    recs[40:40] = [(11, _rand(rng, 20)), (12, _rand(rng, 19)), (13, b"A"), (14, b""), (15, _rand(rng, 8)), (16, _rand(rng, 7))]
    recs[90:90] = [(21, _rand(rng, 35).lower()), (22, _rand(rng, 25) + b"N" + _rand(rng, 25) + b"-x" + _rand(rng, 9) + b"n" + _rand(rng, 22)),
                   (23, b"NNNN-*"), (24, s), (24, s), (25, s + s), (26, b"ACGTACGTACGTACGTACGTACGT"),
                   (27, x + b"N" + recs[3][1]), (28, x[::-1].translate(RC) + recs[5][1].lower())]
    recs.append((BIG_ID, recs[7][1] + _rand(rng, 30)))
    return recs


CASE1 = _case1()


def _fetch_dict(b):
    km, off, td = b.fetch()
    return {int(x): td[int(off[i]):int(off[i + 1])].tolist() for i, x in enumerate(km)}


def _stats_of(db):
    return {"records_written": len(db), "singletons": sum(1 for v in db.values() if len(v) == 1),
            "total_list_entries": sum(len(v) for v in db.values()), "longest_list": max((len(v) for v in db.values()), default=0)}


def _check_stats(st, db):
    for n, v in _stats_of(db).items():
        assert st[n] == v, n
    assert st["dropped_unknown"] == 0


def _check_counts(b, db):
    want = {}
    for ids in db.values():
        for g in ids:
            want[g] = want.get(g, 0) + 1
    t, c = b.taxid_counts()
    assert t.tolist() == sorted(want) and c.tolist() == [want[g] for g in sorted(want)]


# ---- 1 / 9: gene-shaped text, counts and statistics -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 8])
def test_gene_shaped_text(eng, tmp_path, k):
    want = gm.kmer_ids(CASE1, k)
    assert any(len(v) > 1 for v in want.values())
    out = str(tmp_path / "g.bin")
    st = eng.build_gene_taxhisto(_write_fasta(str(tmp_path / "g.fa"), CASE1, width=17), k, out)
    assert open(out, "rb").read() == gm.to_bytes(want, k)
    _check_stats(st, want)
    assert st["bases"] == sum(len(s) for _, s in CASE1) and st["distinct_kmers"] == len(want)
    if k == 20:   # the palindrome is one k-mer; the k-mers of x are forward in gene 27 and reverse-complemented in gene 28
        assert want[gm.canonical_kmers(b"ACGTACGTACGTACGTACGT", 20)[0]] == {26}
        assert sum(1 for v in want.values() if v == {27, 28}) == 11 and sum(1 for v in want.values() if v == {24, 25}) == 5
    from lmat_amd import Builder
    b = Builder(eng, k, genes=True)
    try:
        for gid, s in CASE1:
            b.add_sequence(gid, s)
        st2 = b.run()
        assert _fetch_dict(b) == {km: sorted(v) for km, v in want.items()}
        _check_stats(st2, want)
        _check_counts(b, want)
    finally:
        b.close()


# ---- 2: ids -----------------------------------------------------------------------------------------------------------------------
def test_ids(eng, tmp_path):
    from lmat_amd import Builder, LmatError
    rng = np.random.default_rng(2)
    shared = _rand(rng, 25)
    ids = [BIG_ID, 65536, 1, 2 ** 32 - 1, 65535, 2 ** 31]
    recs = [(g, _rand(rng, 22) + b"N" + shared) for g in ids]
    want = gm.kmer_ids(recs, 20)
    b = Builder(eng, 20, genes=True)
    try:
        for n, bad in enumerate((b">0\n", b">4294967296\n", b">99999999999999999999999\n")):
            fn = str(tmp_path / ("bad%d.fa" % n))
            open(fn, "wb").write(b">5\n" + shared + b"\n" + bad + shared + b"\n")
            with pytest.raises(LmatError) as ei:
                b.add_fasta(fn)
            assert ei.value.code == E_IO and "line 3" in str(ei.value)
        with pytest.raises(LmatError) as ei:
            b.add_sequence(0, shared)
        assert ei.value.code == E_ARG
        b.add_fasta(_write_fasta(str(tmp_path / "ids.fa"), recs))   # the builder stays usable, and the failed files added nothing
        b.run()
        got = _fetch_dict(b)
        assert got == {km: sorted(v) for km, v in want.items()}
        assert sorted(ids) in got.values()          # numeric order: 65535 < 65536 < 2^31 < 3000051781 < 2^32-1
        b.write_taxhisto(str(tmp_path / "ids.bin"))
        assert open(str(tmp_path / "ids.bin"), "rb").read() == gm.to_bytes(want, 20)
    finally:
        b.close()


# ---- 3: list lengths ------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 8, 9, 64, 65, 66, 130)


def _case3():
    rng = np.random.default_rng(3)
    recs, nid = [], 5
    for n in LENGTHS:
        block = _rand(rng, 20)
        for _ in range(n):
            nid += int(rng.integers(1, 50000))
            recs.append((nid, _rand(rng, 23) + b"N" + block))
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def test_list_lengths(eng, tmp_path):
    recs = _case3()
    want = gm.kmer_ids(recs, 20)
    assert sorted(len(v) for v in want.values())[-7:] == list(LENGTHS[1:])   # and singletons below them
    out = str(tmp_path / "l.bin")
    st = eng.build_gene_taxhisto(_write_fasta(str(tmp_path / "l.fa"), recs), 20, out)
    assert open(out, "rb").read() == gm.to_bytes(want, 20)
    _check_stats(st, want)
    assert st["longest_list"] == 130


@pytest.mark.parametrize("n", [65535, 65536])
def test_list_of_the_record_limit(eng, tmp_path, n):
    from lmat_amd import Builder, LmatError
    block = _rand(np.random.default_rng(4), 20)
    ids = np.arange(n, dtype=np.uint64) * 3 + 2
    fa = str(tmp_path / "many.fa")
    open(fa, "wb").write(b"".join(b">%d\n%s\n" % (g, block) for g in ids.tolist()))
    b = Builder(eng, 20, genes=True)
    try:
        b.add_fasta(fa)
        if n > 65535:
            with pytest.raises(LmatError) as ei:
                b.run()
            assert ei.value.code == E_CAPACITY and "65536" in str(ei.value)
        else:
            st = b.run()
            km, off, td = b.fetch()
            assert km.tolist() == gm.canonical_kmers(block, 20) and off.tolist() == [0, n]
            assert np.array_equal(td, ids.astype(np.uint32))        # complete and ascending
            assert st["longest_list"] == n and st["records_written"] == 1
    finally:
        b.close()


# ---- 4: invariance --------------------------------------------------------------------------------------------------------------
def test_invariance(eng, tmp_path, monkeypatch):
    from lmat_amd import LmatError
    k = 20
    fa = _write_fasta(str(tmp_path / "g.fa"), CASE1, width=33)
    want = gm.to_bytes(gm.kmer_ids(CASE1, k), k)
    monkeypatch.delenv("LMAT_DBGEN_SORT", raising=False)
    runs = [dict(prefix_bits=0), dict(prefix_bits=3), dict(prefix_bits=-1), dict(chunk_bases=1024), dict(chunk_bases=1024, prefix_bits=3)]
    for sort in ("", "pairs"):
        if sort:
            monkeypatch.setenv("LMAT_DBGEN_SORT", sort)
        for n, opts in enumerate(runs):
            out = str(tmp_path / ("o%s%d.bin" % (sort, n)))
            st = eng.build_gene_taxhisto(fa, k, out, **opts)
            assert open(out, "rb").read() == want, (sort, opts)
            assert st["passes"] == 1 << max(opts.get("prefix_bits", 0), 0)
    monkeypatch.delenv("LMAT_DBGEN_SORT", raising=False)
    # 64 MiB are the builder's fixed slack; 100 KiB behind them hold about 1 200 of the text's 3 600 pairs: the split is derived, a forced
    # single pass is refused
    small = (64 << 20) + (100 << 10)
    out = str(tmp_path / "small.bin")
    st = eng.build_gene_taxhisto(fa, k, out, budget_bytes=small, chunk_bases=1024)
    assert st["passes"] > 1 and open(out, "rb").read() == want
    with pytest.raises(LmatError) as ei:
        eng.build_gene_taxhisto(fa, k, out, budget_bytes=small, chunk_bases=1024, prefix_bits=0)
    assert ei.value.code == E_CAPACITY


# ---- 5: merge -------------------------------------------------------------------------------------------------------------------
def _merge_sources():
    """Three record sets over shared blocks: k-mers in one, two and three sources; ids 900001.. occur in the files only."""
    rng = np.random.default_rng(5)
    blocks = [_rand(rng, 40) for _ in range(6)]
    fa = [(100 + i, _rand(rng, 30) + b"N" + blocks[i % 3] + b"N" + blocks[3]) for i in range(12)]
    f1 = [(900001 + i, _rand(rng, 30) + b"N" + blocks[i % 2] + b"N" + blocks[4]) for i in range(70)] + [(103, blocks[3] + blocks[5])]
    f2 = [(BIG_ID - i, blocks[0] + b"N" + blocks[4] + _rand(rng, 25)) for i in range(9)] + [(900003, blocks[5])]
    return fa, f1, f2


def test_merge(eng, tmp_path):
    from lmat_amd import Builder
    k = 20
    fa, f1, f2 = _merge_sources()
    dbs = [gm.kmer_ids(r, k) for r in (fa, f1, f2)]
    p_fa = _write_fasta(str(tmp_path / "a.fa"), fa)
    p1, p2 = str(tmp_path / "f1.bin"), str(tmp_path / "f2.bin")
    open(p1, "wb").write(gm.to_bytes(dbs[1], k, order=lambda v: sorted(v, reverse=True)))   # lists of an input need not ascend
    open(p2, "wb").write(gm.to_bytes(dbs[2], k))
    want = gm.union(gm.kmer_ids(fa, k), gm.parse_taxhisto(open(p1, "rb").read())[1], gm.parse_taxhisto(open(p2, "rb").read())[1])
    n_src = {km: sum(km in d for d in dbs) for km in want}
    assert {1, 2, 3} == set(n_src.values()) and any(max(v) > 900000 and min(v) > 900000 for v in want.values())
    assert any(len(v) > 64 for v in want.values())
    outs = []
    for order in itertools.permutations((("fa", p_fa), ("th", p1), ("th", p2))):
        b = Builder(eng, k, genes=True)
        try:
            for kind, p in order:
                (b.add_fasta if kind == "fa" else b.add_taxhisto)(p)
            st = b.run()
            out = str(tmp_path / ("m%d.bin" % len(outs)))
            b.write_taxhisto(out)
            outs.append(open(out, "rb").read())
            ms = b.merge_stats
            assert ms["inputs"] == 2 and ms["records_in"] == len(dbs[1]) + len(dbs[2])
            assert ms["entries_in"] == sum(len(v) for d in dbs[1:] for v in d.values())
            assert ms["records_one_source"] == sum(1 for v in n_src.values() if v == 1)
            assert ms["records_merged"] == sum(1 for v in n_src.values() if v > 1) and ms["records_grown"] == 0
            _check_stats(st, want)
            _check_counts(b, want)
        finally:
            b.close()
    assert all(o == gm.to_bytes(want, k) for o in outs)
    # the same under a split, the pair sort and a budget that forces passes
    for opts in (dict(prefix_bits=3), dict(budget_bytes=(64 << 20) + (100 << 10), chunk_bases=1024)):
        out = str(tmp_path / "split.bin")
        st = eng.build_gene_taxhisto(p_fa, k, out, taxhistos=[p2, p1], **opts)
        assert open(out, "rb").read() == outs[0] and st["passes"] > 1


def test_merge_fixture_and_refusals(eng, tmp_path, monkeypatch):
    from lmat_amd import LmatError
    data = open(GENE_BIN, "rb").read()
    k, recs = gm.parse_taxhisto(data)
    want = gm.to_bytes(gm.union({}, recs), k)
    for sort in ("", "pairs"):
        monkeypatch.setenv("LMAT_DBGEN_SORT", sort)
        out = str(tmp_path / ("sorted%s.bin" % sort))
        st = eng.build_gene_taxhisto(None, 20, out, taxhistos=[GENE_BIN])
        assert open(out, "rb").read() == want and want != data
        assert st["records_written"] == st["merge"]["records_one_source"] == 25924 and st["total_list_entries"] == 38136
        assert st["merge"]["records_merged"] == 0 and st["merge"]["records_grown"] == 0
    monkeypatch.delenv("LMAT_DBGEN_SORT")
    for name, db, kk, code in (("rep.bin", {5: [7, 9, 7]}, 20, E_IO), ("zero.bin", {5: [0, 3]}, 20, E_IO), ("k18.bin", {5: [7]}, 18, E_ARG)):
        fn = str(tmp_path / name)
        open(fn, "wb").write(gm.to_bytes(db, kk, order=list))
        with pytest.raises(LmatError) as ei:
            eng.build_gene_taxhisto(None, 20, str(tmp_path / "x.bin"), taxhistos=[fn])
        assert ei.value.code == code and name in str(ei.value)


# ---- 6: loaded databases as inputs ----------------------------------------------------------------------------------------------
def test_add_db(eng, tmp_path, small_dataset):
    import dbgen_model as dm
    from lmat_amd import Builder, Engine, LmatError
    fa = _write_fasta(str(tmp_path / "g.fa"), CASE1)
    gene = Engine(0)
    plain = Engine(0)
    try:
        gene.build_gene_db(GENE_BIN, k=20)
        plain.load_taxonomy(small_dataset["tree"], small_dataset["depth"], small_dataset["rank"], small_dataset["idmap"])
        plain.build_db(small_dataset["db"], k=20)
        exported = str(tmp_path / "exported.bin")
        gene.export_taxhisto(exported)
        outs = []
        for add in (lambda b: b.add_db(gene), lambda b: b.add_taxhisto(exported)):
            b = Builder(eng, 20, genes=True)
            try:
                b.add_fasta(fa)
                add(b)
                b.run()
                out = str(tmp_path / ("d%d.bin" % len(outs)))
                b.write_taxhisto(out)
                outs.append(open(out, "rb").read())
            finally:
                b.close()
        want = gm.union(gm.kmer_ids(CASE1, 20), gm.parse_taxhisto(open(GENE_BIN, "rb").read())[1])
        assert outs[0] == outs[1] == gm.to_bytes(want, 20)
        b = Builder(eng, 20, genes=True)
        try:
            with pytest.raises(LmatError) as ei:
                b.add_db(plain)                    # a loaded taxonomy database
            assert ei.value.code == E_ARG and "taxonomy database" in str(ei.value)
        finally:
            b.close()
        b = Builder(eng, 20, dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
        try:
            with pytest.raises(LmatError) as ei:
                b.add_db(gene)
            assert ei.value.code == E_ARG and "gene database" in str(ei.value)
        finally:
            b.close()
    finally:
        gene.close()
        plain.close()


# ---- 7: straight to the table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["text", "lengths"])
def test_table(eng, tmp_path, case):
    from lmat_amd import Engine
    recs = CASE1 if case == "text" else _case3()
    want = gm.kmer_ids(recs, 20)
    fa = _write_fasta(str(tmp_path / "g.fa"), recs)
    written = str(tmp_path / "w.bin")
    eng.build_gene_taxhisto(fa, 20, written)
    e = Engine(0)
    try:
        st = e.build_gene_db_from_genes(fa, k=20)
        assert e.db_size == st["records_written"] == len(want)
        kms = np.array(sorted(want), dtype=np.uint64)
        counts, tids = e.lookup(kms, stride=132)
        for i, km in enumerate(kms.tolist()):
            assert counts[i] == len(want[km]) and tids[i, :counts[i]].tolist() == sorted(want[km]), km
        absent = np.array([x for x in np.random.default_rng(8).integers(0, 1 << 40, 1100).tolist() if x not in want][:1000], dtype=np.uint64)
        assert absent.size == 1000 and not e.lookup(absent, stride=4)[0].any()
        e.export_taxhisto(str(tmp_path / "x.bin"))
        assert open(str(tmp_path / "x.bin"), "rb").read() == open(written, "rb").read()
    finally:
        e.close()


def test_table_refuses_the_wrong_builder(eng, tmp_path):
    import dbgen_model as dm
    from lmat_amd import Builder, Engine, LmatError
    e = Engine(0)
    gb = Builder(eng, 20, genes=True)
    tb = Builder(eng, 20, dm.gunzip_to("tree.dat.gz", str(tmp_path / "tree.dat")))
    try:
        gb.add_sequence(5, b"ACGTTGCAAGGCTTAACCGGTTAACG")
        gb.run()
        tb.run()
        assert e.lib.lmat_genedb_build_from_genes(e.ctx, tb.h, 0) == E_ARG
        assert e.lib.lmat_db_build_from_genomes(e.ctx, gb.h, 0) == E_ARG
        with pytest.raises(LmatError) as ei:
            Builder(eng, 20, None)                 # the tree-mode builder still needs its tree
        assert ei.value.code == E_ARG and "taxonomy tree file is required" in str(ei.value)
    finally:
        gb.close()
        tb.close()
        e.close()


# ---- 8: votes -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_set(tmp_path_factory):
    """200 genes of 300 bases in 40 families of five that share a 120-base block; reads of 100 bases cut from the genes (a third of
    them inside the shared block's reach), reads joined from two genes, random reads and a short one; the oracle's votes."""
    import oracle_py
    d = tmp_path_factory.mktemp("genevotes")
    rng = np.random.default_rng(88)
    genes = []
    for fam in range(40):
        block = _rand(rng, 120)
        for j in range(5):
            genes.append((7000 + 13 * (fam * 5 + j) + (BIG_ID if j == 4 else 0), _rand(rng, 90) + block + _rand(rng, 90)))
    fa = _write_fasta(str(d / "genes.fa"), genes, width=60)
    reads = []
    for i in range(600):
        s = genes[int(rng.integers(0, 200))][1]
        at = int(rng.integers(0, 201))
        reads.append(s[at:at + 100])
    for i in range(40):
        a, b = genes[int(rng.integers(0, 200))][1], genes[int(rng.integers(0, 200))][1]
        reads.append(a[230:] + b[:60])
    reads += [_rand(rng, 100) for _ in range(40)] + [b"ACGTACGTAC", genes[3][1][:50] + b"N" + genes[3][1][51:99].lower()]
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    blob = np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8)
    return {"fa": fa, "dir": str(d), "reads": reads, "blob": blob, "off": off, "oracle_py": oracle_py}


@pytest.mark.parametrize("streamed", [False, True])
def test_votes(eng, vote_set, streamed):
    from lmat_amd import Engine, Params, Stream
    v = vote_set
    written = os.path.join(v["dir"], "genes.bin")
    eng.build_gene_taxhisto(v["fa"], 20, written)
    o = v["oracle_py"].GeneOracle(written)
    any_, gid, top, cnt, score = o.label(v["blob"], v["off"], 20)
    multi = [len({g for km in gm.canonical_kmers(r, 20) for g in o.lookup(km)}) > 1 for r in v["reads"]]
    o.close()
    called = np.flatnonzero(any_ == 1)
    assert called.size >= 0.9 * len(v["reads"]) and sum(multi[i] for i in called) >= 0.1 * called.size
    assert (any_ == 0).sum() >= 40
    e = Engine(0, Params.run_rl(prn_all=0))
    try:
        e.build_gene_db_from_genes(v["fa"], k=20)
        if streamed:
            st = Stream(e, max_reads=len(v["reads"]), max_bases=int(v["off"][-1]) + 16, cands_per_read=0, n_slots=2)
            st.submit(v["blob"], v["off"], tag=1)
            res = st.next()[0]
            st.close()
        else:
            res, _ = e.classify(e.upload_reads((v["blob"], v["off"])), want_cands=False)
    finally:
        e.close()
    for i in range(len(v["reads"])):
        if any_[i]:
            assert res["status"][i] == 0 and res["call_tid"][i] == gid[i] and res["n_cand"][i] == top[i] and res["cand_kmer_cnt"][i] == cnt[i], i
            assert res["call_score"][i] == score[i]
        else:
            assert res["status"][i] != 0, i


# ---- 10: the tool ---------------------------------------------------------------------------------------------------------------
def test_tool(eng, tmp_path):
    k = 20
    fa, f1, f2 = _merge_sources()
    p_fa = _write_fasta(str(tmp_path / "b.fa"), fa)
    p1 = str(tmp_path / "a.bin")
    open(p1, "wb").write(gm.to_bytes(gm.kmer_ids(f1, k), k, order=lambda v: sorted(v, reverse=True)))
    api, cli, counts = str(tmp_path / "api.bin"), str(tmp_path / "cli.bin"), str(tmp_path / "counts.txt")
    st = eng.build_gene_taxhisto(p_fa, k, api)
    r = subprocess.run([EXE, "-G", "-i", p_fa, "-k", "20", "-o", cli, "-c", counts], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(cli, "rb").read() == open(api, "rb").read() == gm.to_bytes(gm.kmer_ids(fa, k), k)
    assert "num mapping kmers processed: %d\n" % st["records_written"] in r.stdout
    per_id = {}
    for ids in gm.kmer_ids(fa, k).values():
        for g in ids:
            per_id[g] = per_id.get(g, 0) + 1
    assert open(counts).read() == "".join("%d %d\n" % (g, per_id[g]) for g in sorted(per_id))
    want = gm.union(gm.kmer_ids(fa, k), gm.parse_taxhisto(open(p1, "rb").read())[1])
    r = subprocess.run([EXE, "-G", "-m", p1, "-i", p_fa, "-k", "20", "-o", cli, "-p", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(cli, "rb").read() == gm.to_bytes(want, k) and "merge: inputs 1 " in r.stdout
    r = subprocess.run([EXE, "-G", "-t", str(tmp_path / "tree.dat"), "-i", p_fa, "-k", "20", "-o", cli], capture_output=True, text=True)
    assert r.returncode != 0 and "Usage:" in r.stderr
    r = subprocess.run([EXE, "-G", "-D", str(tmp_path / "img"), "-i", p_fa, "-k", "20", "-o", cli], capture_output=True, text=True)
    assert r.returncode != 0 and "-D is not available with -G" in r.stderr
