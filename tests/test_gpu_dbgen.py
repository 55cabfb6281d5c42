"""GPU: the database built from genome FASTA (lmat_build_*, dbgen.hip) against the reference's own files (fixtures of
tests/golden/make_dbgen_goldens.py) and against the Python model test_dbgen_model.py pins to them."""
import os
import subprocess

import numpy as np
import pytest

import dbgen_model as dm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "build_tax_histo")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    from lmat_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    d = tmp_path_factory.mktemp("dbgen_gold")
    p = {n: dm.gunzip_to(n + ".gz", str(d / n)) for n in ("tree.dat", "a.fa", "c.fa", "a_k20.bin", "b_k18.bin", "c_k20.bin")}
    p["dir"] = str(d)
    return p


def _write_fasta(path, recs, width=0):
    with open(path, "wb") as f:
        for tid, s in recs:
            f.write(b">%d\n" % tid)
            if width:
                for j in range(0, len(s), width):
                    f.write(s[j:j + width] + b"\n")
            else:
                f.write(s + b"\n")
    return path


def _check_against_model(path, recs, tax, k, stats):
    want, dropped = dm.model(recs, tax, k)
    kk, count, got = dm.read_taxhisto(path)
    assert kk == k and count == len(want)
    assert [km for km, _ in got] == sorted(want)
    for km, lst in got:
        assert lst == want[km], km          # ascending taxids, as the header says
    longest = max((len(l) for l in want.values()), default=0)
    assert stats["records_written"] == len(want) and stats["dropped_unknown"] == dropped
    assert stats["distinct_kmers"] == len(want) + dropped
    assert stats["longest_list"] == longest
    assert stats["total_list_entries"] == sum(len(l) for l in want.values())
    assert stats["singletons"] == sum(1 for l in want.values() if len(l) == 1)
    return want


@pytest.mark.parametrize("fa,ref,k", [("a.fa", "a_k20.bin", 20), ("a.fa", "b_k18.bin", 18), ("c.fa", "c_k20.bin", 20)])
def test_goldens(eng, gold, tmp_path, fa, ref, k):
    from lmat_amd import Engine
    out = str(tmp_path / "th.bin")
    stats = eng.build_taxhisto(gold[fa], gold["tree.dat"], k, out)
    _, ref_count, ref_recs = dm.read_taxhisto(gold[ref])
    kk, count, got = dm.read_taxhisto(out)   # header count, sanity words and file length are checked in there
    assert kk == k and count == ref_count == stats["records_written"]
    assert [km for km, _ in got] == [km for km, _ in ref_recs]
    for (km, lst), (_, want) in zip(got, ref_recs):
        assert lst == sorted(want), km
    recs = dm.parse_fasta(gold[fa])
    _, dropped = dm.model(recs, dm.load_tree(gold["tree.dat"]), k)
    assert stats["dropped_unknown"] == dropped and (dropped > 0) == (fa == "c.fa")
    assert stats["bases"] == sum(len(s) for _, s in recs)
    assert stats["windows"] == stats["emitted_pairs"] > stats["distinct_kmers"]
    # the written file through the existing ingest: a database of 32-bit taxids, codes from the tree
    from lmat_amd import synth
    tax = synth.make_taxonomy((2, 2, 2, 2, 2, 2), specials=False)
    aux = synth.write_aux_files(str(tmp_path / "aux"), tax)
    e2 = Engine(0)
    try:
        e2.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        e2.build_db(out, k=k)
        assert e2.db_size == count
        kms = np.array([km for km, _ in got], dtype=np.uint64)
        counts, tids = e2.lookup(kms, stride=16)
        for i, (km, lst) in enumerate(got):
            assert counts[i] == len(lst) and tids[i, :len(lst)].tolist() == lst, km
    finally:
        e2.close()


def _chunk_edge_records(tax):
    """One 10 kb and several 1 kb genomes; an N and a lower-case base within k - 1 of the edges of 4096-base chunks."""
    rng = np.random.default_rng(7)
    leaves = sorted(t for t in tax.parent if tax.depth[t] == 6)
    big = bytearray(LETTERS[rng.integers(0, 4, 10000)].tobytes())
    for edge in (4096, 8192):   # the text starts with this record: its byte i is text position i
        big[edge - 5] = ord("N")
        big[edge + 7] = ord(chr(big[edge + 7]).lower())
        big[edge - 12] = ord(chr(big[edge - 12]).lower())
    recs = [(leaves[0], bytes(big))]
    for j in range(1, 7):
        s = bytearray(LETTERS[rng.integers(0, 4, 1000)].tobytes())
        s[100:400] = big[2000 + 100 * j:2300 + 100 * j]   # shared with the big genome
        s[int(rng.integers(0, 1000))] = ord("N")
        recs.append((leaves[j * 5], bytes(s)))
    return recs


def test_chunk_and_pass_invariance(eng, gold, tmp_path):
    k = 20
    tax = dm.load_tree(gold["tree.dat"])
    recs = _chunk_edge_records(tax)
    fa = _write_fasta(str(tmp_path / "g.fa"), recs, width=70)
    files = {}
    for chunk in (4096, 0):
        for pb in (0, 2, 4):
            out = str(tmp_path / ("o_%d_%d.bin" % (chunk, pb)))
            st = eng.build_taxhisto(fa, gold["tree.dat"], k, out, chunk_bases=chunk, prefix_bits=pb)
            assert st["passes"] == 1 << pb and st["windows"] == st["emitted_pairs"]
            files[(chunk, pb)] = open(out, "rb").read()
    first = files[(4096, 0)]
    for key, data in files.items():
        assert data == first, key
    _check_against_model(str(tmp_path / "o_4096_0.bin"), recs, tax, k, st)


def test_pair_sort_equals_packed_sort(eng, gold, tmp_path, monkeypatch):
    """LMAT_DBGEN_SORT=pairs (read per build): (owner, k-mer) pairs sorted twice write the bytes the one packed key writes."""
    k = 20
    tax = dm.load_tree(gold["tree.dat"])
    recs = _chunk_edge_records(tax)
    fa = _write_fasta(str(tmp_path / "g.fa"), recs, width=70)
    packed = str(tmp_path / "packed.bin")
    counts = lambda s: {n: v for n, v in s.items() if not n.endswith("_ms") and n not in ("passes", "prefix_bits")}
    monkeypatch.delenv("LMAT_DBGEN_SORT", raising=False)
    st = eng.build_taxhisto(fa, gold["tree.dat"], k, packed)
    _check_against_model(packed, recs, tax, k, st)
    monkeypatch.setenv("LMAT_DBGEN_SORT", "pairs")
    for pb in (0, 2):
        out = str(tmp_path / ("pairs_%d.bin" % pb))
        st2 = eng.build_taxhisto(fa, gold["tree.dat"], k, out, prefix_bits=pb)
        assert st2["passes"] == 1 << pb
        assert open(out, "rb").read() == open(packed, "rb").read(), pb
        assert counts(st2) == counts(st), pb


def test_wide_fan_in(eng, tmp_path):
    """72 strains across three genera that all hold one 60 bp block (more than 64 owners and more than 64 list entries for its
    k-mers), species that own a genome besides their strains (owners that are ancestors of owners), blocks shared at every level."""
    from lmat_amd import synth
    k = 20
    rng = np.random.default_rng(11)
    t = synth.Taxonomy()
    t.add(1, 1, "no_rank", "root")
    t.add(10, 1, "superkingdom", "sk")
    t.add(20, 10, "family", "fam")
    block = LETTERS[rng.integers(0, 4, 60)].tobytes()
    recs, nid = [], [1000]

    def new(parent, rank):
        nid[0] += 3
        t.add(nid[0], parent, rank, "%s_%d" % (rank, nid[0]))
        return nid[0]

    for g in range(3):
        genus = new(20, "genus")
        gblock = LETTERS[rng.integers(0, 4, 50)].tobytes()
        for s in range(4):
            sp = new(genus, "species")
            sblock = LETTERS[rng.integers(0, 4, 50)].tobytes()
            if s % 2 == 0:   # the species has a genome of its own
                recs.append((sp, sblock + b"N" + block + LETTERS[rng.integers(0, 4, 40)].tobytes()))
            for _ in range(6):
                strain = new(sp, "strain")
                own = LETTERS[rng.integers(0, 4, 45)].tobytes()
                recs.append((strain, own + block.lower() + b"n" + gblock + b"N" + sblock))
    rng.shuffle(recs)
    t.id16 = {tid: i + 1 for i, tid in enumerate(sorted(t.ids))}   # root -> 1, the rest dense, as make_taxonomy does
    aux = synth.write_aux_files(str(tmp_path / "aux"), t)
    fa = _write_fasta(str(tmp_path / "g.fa"), recs)
    out = str(tmp_path / "th.bin")
    st = eng.build_taxhisto(fa, aux["tree"], k, out)
    tax = dm.load_tree(aux["tree"])
    want = _check_against_model(out, recs, tax, k, st)
    assert st["longest_list"] == 72 + 12 + 3 + 1      # strains, species (six of them owners themselves), genera and the family
    assert sum(1 for l in want.values() if len(l) > 64) >= 41
    assert any(2 < len(l) <= 64 for l in want.values())
    # the same through add_sequence / fetch, no file on either side
    from lmat_amd import Builder
    b = Builder(eng, k, aux["tree"])
    try:
        for tid, s in recs:
            b.add_sequence(tid, s)
        assert b.run() == {**st, **{n: b.stats[n] for n in b.stats if n.endswith("_ms")}}
        km, off, td = b.fetch()
        assert km.tolist() == sorted(want)
        assert all(td[int(off[i]):int(off[i + 1])].tolist() == want[int(x)] for i, x in enumerate(km))
        km2, off2, td2 = b.fetch(5, 3)
        assert km2.tolist() == km[5:8].tolist() and off2[0] == 0 and td2.tolist() == td[int(off[5]):int(off[8])].tolist()
    finally:
        b.close()


def test_direct_path_equals_file_then_ingest(tmp_path):
    from lmat_amd import Engine, Params, synth
    k = 20
    tax = synth.make_taxonomy((2, 2, 2, 2, 3, 3), specials=False)
    aux = synth.write_aux_files(str(tmp_path / "aux"), tax)
    genomes = synth.make_genomes(tax, 600, 2002)
    recs = [(leaf, LETTERS[genomes[leaf]].tobytes()) for leaf in tax.leaves]
    fa = _write_fasta(str(tmp_path / "g.fa"), recs, width=80)
    reads = [s for _, s in synth.make_reads(tax, genomes, 2000, 150, 3003)]
    texts, tallies = [], []
    for direct in (False, True):
        e = Engine(0, Params.run_rl())
        try:
            e.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
            if direct:
                st = e.build_db_from_genomes(fa, aux["tree"], k)
            else:
                th = str(tmp_path / "th.bin")
                st = e.build_taxhisto(fa, aux["tree"], k, th)
                e.build_db(th, k=k)
            assert e.db_size == st["records_written"] > 10000
            dr = e.upload_reads(reads)
            res, cands = e.classify(dr)
            texts.append(e.format_out(res, cands))
            tallies.append(e.counts())
            dr.free()
        finally:
            e.close()
    assert texts[0] == texts[1] and tallies[0] == tallies[1]
    assert len(texts[0]) > 100000


def test_cli(eng, gold, tmp_path):
    out_api, out_cli = str(tmp_path / "api.bin"), str(tmp_path / "cli.bin")
    st = eng.build_taxhisto(gold["a.fa"], gold["tree.dat"], 20, out_api)
    r = subprocess.run([EXE, "-i", gold["a.fa"], "-k", "20", "-t", gold["tree.dat"], "-o", out_cli], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(out_cli, "rb").read() == open(out_api, "rb").read()
    assert "total taxids: %d\n" % st["total_list_entries"] in r.stdout
    assert "singletons: %d\n" % st["singletons"] in r.stdout
    assert "num mapping kmers processed: %d\n" % st["records_written"] in r.stdout
    # a list file, two passes: the same bytes
    lst = str(tmp_path / "list.txt")
    open(lst, "w").write(gold["a.fa"] + "\n")
    r = subprocess.run([EXE, "-i", lst, "-l", "-k", "20", "-t", gold["tree.dat"], "-o", out_cli + "2", "-p", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and open(out_cli + "2", "rb").read() == open(out_api, "rb").read()
    # a missing tree, a bad header
    r = subprocess.run([EXE, "-i", gold["a.fa"], "-k", "20", "-t", str(tmp_path / "none.dat"), "-o", out_cli], capture_output=True, text=True)
    assert r.returncode != 0 and "failed to open" in r.stderr
    bad = str(tmp_path / "bad.fa")
    open(bad, "w").write(">genome_one\nACGTACGTACGTACGTACGTACGT\n")
    r = subprocess.run([EXE, "-i", bad, "-k", "20", "-t", gold["tree.dat"], "-o", out_cli], capture_output=True, text=True)
    assert r.returncode != 0 and "bad FASTA header" in r.stderr
    # a list beyond the 16-bit count of the record: two strains whose paths to their LCA hold 66 000 nodes
    n = 66000
    lines = ["# chain", "# id nchild children... parent / name", str(n + 2), "1 2 2 %d 1" % (n + 2), "root"]
    for i in range(2, n + 1):
        lines += ["%d 1 %d %d" % (i, i + 1, i - 1), "n%d" % i]
    lines += ["%d 0 %d" % (n + 1, n), "deep", "%d 0 1" % (n + 2), "shallow"]
    tree = str(tmp_path / "chain.dat")
    open(tree, "w").write("\n".join(lines))
    seq = LETTERS[np.random.default_rng(3).integers(0, 4, 40)].tobytes().decode()
    fa = str(tmp_path / "two.fa")
    open(fa, "w").write(">%d\n%s\n>%d\n%s\n" % (n + 1, seq, n + 2, seq))
    r = subprocess.run([EXE, "-i", fa, "-k", "20", "-t", tree, "-o", out_cli], capture_output=True, text=True)
    assert r.returncode != 0 and "at most 65535" in r.stderr
