"""GPU: tax_histo files as further inputs of a build (lmat_build_add_taxhisto, the merge of DESIGN section 10) against the
reference's own files (fixtures of tests/golden/make_dbmerge_goldens.py) and against the Python statement of the rule that
test_dbmerge_model.py pins to them; the per-taxid counts against the reference's countTaxidFrequency output."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dbgen_model as dm
import dbmerge_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "build_tax_histo")
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
E_ARG, E_IO, E_CAPACITY, E_TAXONOMY = -1, -2, -4, -5
SANITY = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    from lmat_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gold(tmp_path_factory, eng):
    """The fixtures unpacked, the records of a.fa dealt into FASTA parts, and -- computed once, never changed -- what the plain
    build makes of a.fa: the bytes every merge below must reproduce."""
    d = tmp_path_factory.mktemp("dbmerge_gold")
    p = {n: dm.gunzip_to(n + ".gz", str(d / n)) for n in ("tree.dat", "a.fa", "c.fa", "a_k20.bin", "b_k18.bin")}
    p.update({n: mm.gunzip_to(n + ".gz", str(d / n)) for n in ("a_p0_k20.bin", "a_p1_k20.bin")})
    p["dir"] = str(d)
    p["recs"] = dm.parse_fasta(p["a.fa"])
    p["even.fa"] = _write_fasta(str(d / "even.fa"), p["recs"][0::2])
    p["odd.fa"] = _write_fasta(str(d / "odd.fa"), p["recs"][1::2])
    p["tax"] = dm.load_tree(p["tree.dat"])
    p["whole.bin"] = str(d / "whole.bin")
    p["whole_stats"] = eng.build_taxhisto(p["a.fa"], p["tree.dat"], 20, p["whole.bin"])
    p["whole"] = open(p["whole.bin"], "rb").read()
    p["kcnt"] = open(os.path.join(mm.GOLD, "a_k20.par.kcnt")).read()
    return p


def _write_fasta(path, recs):
    with open(path, "wb") as f:
        for tid, s in recs:
            f.write(b">%d\n%s\n" % (tid, s))
    return path


def _write_th(path, k, recs, count=None):
    """A tax_histo file of [(k-mer, [taxids])] as given (no ordering applied)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQIcI", 29, len(recs) if count is None else count, SANITY, 999, b"N", k))
        for i, (km, lst) in enumerate(recs):
            f.write(struct.pack("<QH%dI" % len(lst), km, len(lst), *lst))
            if (i + 1) % 1500 == 0:
                f.write(struct.pack("<Q", SANITY))
    return path


def _result_stats(st, want):
    assert st["records_written"] == len(want)
    assert st["singletons"] == sum(1 for l in want.values() if len(l) == 1)
    assert st["total_list_entries"] == sum(len(l) for l in want.values())
    assert st["longest_list"] == max(len(l) for l in want.values())


def test_goldens(eng, gold, tmp_path):
    parts = [gold["a_p0_k20.bin"], gold["a_p1_k20.bin"]]
    out = str(tmp_path / "m.bin")
    st = eng.merge_taxhisto(parts, gold["tree.dat"], 20, out)
    assert open(out, "rb").read() == gold["whole"]
    _, ref_count, ref = dm.read_taxhisto(gold["a_k20.bin"])
    kk, count, got = dm.read_taxhisto(out)
    assert kk == 20 and count == ref_count
    for (km, lst), (rkm, want) in zip(got, ref):
        assert km == rkm and lst == sorted(want), km
    st2 = eng.merge_taxhisto(parts[::-1], gold["tree.dat"], 20, out + "2")
    assert open(out + "2", "rb").read() == gold["whole"]
    srcs = [dict(dm.read_taxhisto(p)[2]) for p in parts]
    want, mst = mm.merge(gold["tax"], srcs)
    for s in (st, st2):
        m = s["merge"]
        assert m["inputs"] == 2 and m["passes"] == s["passes"]
        assert m["records_in"] == sum(len(x) for x in srcs) and m["entries_in"] == sum(len(l) for x in srcs for l in x.values())
        assert {n: m[n] for n in mst} == mst
        assert mst["records_merged"] >= 4000 and mst["records_grown"] >= 4000
        _result_stats(s, want)
        assert s["bases"] == s["windows"] == s["emitted_pairs"] == s["distinct_kmers"] == s["dropped_unknown"] == 0


def test_incremental_update(eng, gold, tmp_path):
    from lmat_amd import Builder, Engine, synth
    out = str(tmp_path / "m.bin")
    st = eng.merge_taxhisto(gold["a_p0_k20.bin"], gold["tree.dat"], 20, out, fasta=gold["odd.fa"])
    assert open(out, "rb").read() == gold["whole"]
    odd = gold["recs"][1::2]
    genome_part, _ = dm.model(odd, gold["tax"], 20)
    assert st["bases"] == sum(len(s) for _, s in odd) and st["distinct_kmers"] == len(genome_part) and st["dropped_unknown"] == 0
    assert st["merge"]["inputs"] == 1 and st["merge"]["records_merged"] >= 4000
    _result_stats(st, dict(dm.read_taxhisto(gold["whole.bin"])[2]))
    # the two owners of c.fa the tree does not know, in the FASTA part: their k-mers give no record
    unknown = [r for r in dm.parse_fasta(gold["c.fa"]) if r[0] not in gold["tax"].parent]
    assert len(unknown) == 2
    fa = _write_fasta(str(tmp_path / "odd_c.fa"), odd + unknown)
    st = eng.merge_taxhisto(gold["a_p0_k20.bin"], gold["tree.dat"], 20, out + "2", fasta=fa)
    assert st["dropped_unknown"] > 0 and open(out + "2", "rb").read() == gold["whole"]
    # the result straight into the classify table
    tax = synth.make_taxonomy((2, 2, 2, 2, 2, 2), specials=False)
    aux = synth.write_aux_files(str(tmp_path / "aux"), tax)
    _, count, recs = dm.read_taxhisto(gold["whole.bin"])
    e2 = Engine(0)
    try:
        e2.load_taxonomy(aux["tree"], aux["depth"], aux["rank"], aux["idmap"])
        b = Builder(e2, 20, gold["tree.dat"])
        try:
            b.add_taxhisto(gold["a_p0_k20.bin"])
            b.add_fasta(fa)
            b.run()
            e2._chk(e2.lib.lmat_db_build_from_genomes(e2.ctx, b.h, 0))
        finally:
            b.close()
        assert e2.db_size == count
        counts, tids = e2.lookup(np.array([km for km, _ in recs], dtype=np.uint64), stride=16)
        for i, (km, lst) in enumerate(recs):
            assert counts[i] == len(lst) and tids[i, :len(lst)].tolist() == lst, km
    finally:
        e2.close()


def test_pass_invariance(eng, gold, tmp_path):
    from lmat_amd import LmatError
    parts = []
    for i in range(3):
        fa = _write_fasta(str(tmp_path / ("t%d.fa" % i)), gold["recs"][i::3])
        parts.append(str(tmp_path / ("t%d.bin" % i)))
        eng.build_taxhisto(fa, gold["tree.dat"], 20, parts[-1])
    for pb in (0, 2, 4):
        out = str(tmp_path / ("o%d.bin" % pb))
        st = eng.merge_taxhisto(parts, gold["tree.dat"], 20, out, prefix_bits=pb)
        assert st["passes"] == st["merge"]["passes"] == 1 << pb
        assert open(out, "rb").read() == gold["whole"], pb
    # 64 MiB of the budget are the fixed slack; the rest holds 72 bytes a record and 12 an entry of the largest slice:
    # about 19 000 records and 70 000 entries do not fit 768 KiB in one pass
    small = (64 << 20) + (768 << 10)
    out = str(tmp_path / "small.bin")
    st = eng.merge_taxhisto(parts, gold["tree.dat"], 20, out, budget_bytes=small)
    assert st["passes"] > 1 and open(out, "rb").read() == gold["whole"]
    with pytest.raises(LmatError) as ei:
        eng.merge_taxhisto(parts, gold["tree.dat"], 20, out, budget_bytes=small, prefix_bits=0)
    assert ei.value.code == E_CAPACITY


def test_merge_only_one_pass_and_several(eng, gold, tmp_path):
    """No FASTA: the count -> CSR tail of the merge alone, in one forced pass and in the several a small budget derives
    (64 MiB of it are the fixed slack; 72 bytes a record and 12 an entry of about 18 000 records do not fit 768 KiB at once)."""
    parts = [gold["a_p0_k20.bin"], gold["a_p1_k20.bin"]]
    one = eng.merge_taxhisto(parts, gold["tree.dat"], 20, str(tmp_path / "one.bin"), prefix_bits=0)
    many = eng.merge_taxhisto(parts, gold["tree.dat"], 20, str(tmp_path / "many.bin"), budget_bytes=(64 << 20) + (768 << 10))
    assert one["passes"] == one["merge"]["passes"] == 1 and many["passes"] == many["merge"]["passes"] > 1
    assert open(str(tmp_path / "one.bin"), "rb").read() == gold["whole"]
    assert open(str(tmp_path / "many.bin"), "rb").read() == gold["whole"]
    for n in ("singletons", "total_list_entries", "longest_list", "records_written"):
        assert one[n] == many[n] == gold["whole_stats"][n], n
    for n in ("records_one_source", "records_merged", "records_grown"):
        assert one["merge"][n] == many["merge"][n], n


def test_shapes_the_fixtures_lack(eng, tmp_path):
    """The 72-strain taxonomy of test_gpu_dbgen.test_wide_fan_in, its records dealt into three sources, with further records so
    that every situation listed at the end occurs; all of it against dm.model of all records together."""
    from lmat_amd import synth
    k = 20
    rng = np.random.default_rng(11)
    t = synth.Taxonomy()
    t.add(1, 1, "no_rank", "root")
    t.add(10, 1, "superkingdom", "sk")
    t.add(20, 10, "family", "fam")
    rnd = lambda n: LETTERS[rng.integers(0, 4, n)].tobytes()
    block, block2, block3 = rnd(60), rnd(60), rnd(60)
    nid = [1000]

    def new(parent, rank):
        nid[0] += 3
        t.add(nid[0], parent, rank, "%s_%d" % (rank, nid[0]))
        return nid[0]

    recs, strains, species, genera = [], [], [], []
    for g in range(3):
        genus = new(20, "genus")
        genera.append(genus)
        gblock = rnd(50)
        for s in range(4):
            sp = new(genus, "species")
            species.append(sp)
            sblock = rnd(50)
            if s % 2 == 0:   # the species has a genome of its own: an owner that is an ancestor of owners
                recs.append((sp, sblock + b"N" + block + rnd(40)))
            for _ in range(6):
                strain = new(sp, "strain")
                strains.append(strain)
                recs.append((strain, rnd(45) + block.lower() + b"n" + gblock + b"N" + sblock))
    rng.shuffle(recs)
    src = [list(recs[i::3]) for i in range(3)]
    # block2: all 72 strains in source 0 alone (a list of 88 copied); block3: the same, and one species in source 1 (88 + a short one)
    src[0] += [(s, block2 + b"N" + block3) for s in strains]
    src[1].append((species[1], block3))
    a, a_sib, b_ = strains[0], strains[1], strains[2]          # three strains of one species
    e_block, f_block, g_block, h_block = rnd(30), rnd(30), rnd(30), rnd(30)
    for i in (0, 1):                                           # identical lists of several entries in two sources
        src[i] += [(a, e_block), (b_, e_block)]
    src[0].append((a, f_block))                                # {x} + {x}
    src[2].append((a, f_block))
    src[0].append((a, g_block))                                # two sibling singletons
    src[1].append((a_sib, g_block))
    src[0].append((a, h_block))                                # a singleton and a singleton far up its own path
    src[2].append((genera[0], h_block))
    t.id16 = {tid: i + 1 for i, tid in enumerate(sorted(t.ids))}
    aux = synth.write_aux_files(str(tmp_path / "aux"), t)
    tax = dm.load_tree(aux["tree"])
    files = []
    for i in range(3):
        fa = _write_fasta(str(tmp_path / ("s%d.fa" % i)), src[i])
        files.append(str(tmp_path / ("s%d.bin" % i)))
        eng.build_taxhisto(fa, aux["tree"], k, files[-1])
    out = str(tmp_path / "m.bin")
    st = eng.merge_taxhisto(files, aux["tree"], k, out)
    want, _ = dm.model(src[0] + src[1] + src[2], tax, k)
    kk, count, got = dm.read_taxhisto(out)
    assert kk == k and [km for km, _ in got] == sorted(want)
    for km, lst in got:
        assert lst == want[km], km
    parts = [dm.model(s, tax, k)[0] for s in src]
    merged, mst = mm.merge(tax, parts)
    assert merged == want
    assert {n: st["merge"][n] for n in mst} == mst
    _result_stats(st, want)
    # every situation occurred
    held = {km: [p[km] for p in parts if km in p] for km in want}
    par, dep = tax.parent, tax.depth
    own = dm.kmer_owners(src[0] + src[1] + src[2], k)
    seen = {
        "merged above 64 from parts of at most 64": any(len(h) > 1 and max(map(len, h)) <= 64 and len(want[km]) > 64 for km, h in held.items()),
        "a part above 64 copied alone": any(len(h) == 1 and len(h[0]) > 64 for h in held.values()),
        "a part above 64 merged with a short one": any(len(h) > 1 and max(map(len, h)) > 64 and min(map(len, h)) <= 2 for h in held.values()),
        "owners that are ancestors of owners": any(len(held[km]) > 1 and any(par[y] in o for y in o) for km, o in own.items() if km in held),
        "a k-mer in exactly one source": any(len(h) == 1 for h in held.values()),
        "identical lists in two sources": any(len(h) == 2 and h[0] == h[1] and len(h[0]) > 1 for h in held.values()),
        "{x} + {x}": any(len(h) == 2 and h[0] == h[1] and len(h[0]) == 1 and want[km] == h[0] for km, h in held.items()),
        "two sibling singletons": any(len(h) == 2 and len(h[0]) == len(h[1]) == 1 and h[0] != h[1] and par[h[0][0]] == par[h[1][0]]
                                      and want[km] == sorted([h[0][0], h[1][0], par[h[0][0]]]) for km, h in held.items()),
        "a singleton and one far up its path": any(len(h) == 2 and len(h[0]) == len(h[1]) == 1 and abs(dep[h[0][0]] - dep[h[1][0]]) >= 2
                                                   and len(want[km]) == abs(dep[h[0][0]] - dep[h[1][0]]) + 1 for km, h in held.items()),
    }
    assert all(seen.values()), seen
    # the same in the other order of the inputs and in 8 passes
    eng.merge_taxhisto(files[::-1], aux["tree"], k, out + "2", prefix_bits=3)
    assert open(out + "2", "rb").read() == open(out, "rb").read()


def test_empty_source(eng, gold, tmp_path):
    fa = _write_fasta(str(tmp_path / "u.fa"), [r for r in dm.parse_fasta(gold["c.fa"]) if r[0] not in gold["tax"].parent])
    empty = str(tmp_path / "empty.bin")
    st = eng.build_taxhisto(fa, gold["tree.dat"], 20, empty)
    assert st["records_written"] == 0 and st["dropped_unknown"] > 0 and dm.read_taxhisto(empty)[1] == 0
    out = str(tmp_path / "m.bin")
    st = eng.merge_taxhisto([empty, gold["a_k20.bin"]], gold["tree.dat"], 20, out)
    assert open(out, "rb").read() == gold["whole"]
    assert st["merge"]["records_merged"] == 0 and st["merge"]["records_one_source"] == st["records_written"]


def _good_merge(eng, gold, tmp_path):
    out = str(tmp_path / "good.bin")
    eng.merge_taxhisto([gold["a_p0_k20.bin"], gold["a_p1_k20.bin"]], gold["tree.dat"], 20, out)
    assert open(out, "rb").read() == gold["whole"]


def _fails(eng, gold, tmp_path, inputs, code, *words, tree=None):
    from lmat_amd import LmatError
    with pytest.raises(LmatError) as ei:
        eng.merge_taxhisto(inputs, tree or gold["tree.dat"], 20, str(tmp_path / "never.bin"))
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), str(ei.value)
    assert not os.path.exists(str(tmp_path / "never.bin"))
    _good_merge(eng, gold, tmp_path)


def test_error_other_k(eng, gold, tmp_path):
    _fails(eng, gold, tmp_path, [gold["a_p0_k20.bin"], gold["b_k18.bin"]], E_ARG, "b_k18.bin")


def test_error_not_ascending(eng, gold, tmp_path):
    recs = dm.read_taxhisto(gold["a_p0_k20.bin"])[2][:40]
    recs[10], recs[11] = recs[11], recs[10]
    _fails(eng, gold, tmp_path, _write_th(str(tmp_path / "swapped.bin"), 20, recs), E_IO, "swapped.bin", "ascending")


def test_error_truncated(eng, gold, tmp_path):
    data = open(gold["a_p0_k20.bin"], "rb").read()
    bad = str(tmp_path / "cut.bin")
    open(bad, "wb").write(data[:29 + 10 + 2])   # inside the first record's list (every list of the fixture has at least one 4-byte entry)
    _fails(eng, gold, tmp_path, bad, E_IO, "cut.bin", "truncated")


def test_error_unknown_taxid(eng, gold, tmp_path):
    recs = dm.read_taxhisto(gold["a_p0_k20.bin"])[2][:40]
    recs[7] = (recs[7][0], recs[7][1] + [999001])
    _fails(eng, gold, tmp_path, _write_th(str(tmp_path / "alien.bin"), 20, recs), E_TAXONOMY, "alien.bin", "999001")


def test_error_list_beyond_16_bits(eng, gold, tmp_path):
    """Two single-owner files on the 66 000-node chain of test_gpu_dbgen.test_cli: {deep} + {shallow} is the whole chain."""
    n = 66000
    lines = ["# chain", "# id nchild children... parent / name", str(n + 2), "1 2 2 %d 1" % (n + 2), "root"]
    for i in range(2, n + 1):
        lines += ["%d 1 %d %d" % (i, i + 1, i - 1), "n%d" % i]
    lines += ["%d 0 %d" % (n + 1, n), "deep", "%d 0 1" % (n + 2), "shallow"]
    tree = str(tmp_path / "chain.dat")
    open(tree, "w").write("\n".join(lines))
    deep = _write_th(str(tmp_path / "deep.bin"), 20, [(12345, [n + 1]), (99999, [n + 1])])
    shallow = _write_th(str(tmp_path / "shallow.bin"), 20, [(777, [n + 2]), (12345, [n + 2])])
    _fails(eng, gold, tmp_path, [deep, shallow], E_CAPACITY, "at most 65535", tree=tree)


def test_counts(eng, gold):
    from lmat_amd import Builder
    for fasta, ths in ((gold["a.fa"], ()), (None, (gold["a_p0_k20.bin"], gold["a_p1_k20.bin"])), (gold["odd.fa"], (gold["a_p0_k20.bin"],))):
        b = Builder(eng, 20, gold["tree.dat"])
        try:
            if fasta:
                b.add_fasta(fasta)
            for f in ths:
                b.add_taxhisto(f)
            b.run()
            tids, cnts = b.taxid_counts()
            assert mm.kcnt_text(dict(zip(tids.tolist(), cnts.tolist()))) == gold["kcnt"]
            assert tids.tolist() == sorted(tids.tolist()) and int(cnts.min()) > 0
            n = C.c_uint64(0)
            assert b.lib.lmat_build_taxid_counts(b.h, None, None, 0, C.byref(n)) == E_CAPACITY and n.value == len(tids)
        finally:
            b.close()


def test_cli(eng, gold, tmp_path):
    o1, o2, cf = str(tmp_path / "c1.bin"), str(tmp_path / "c2.bin"), str(tmp_path / "counts.txt")
    r = subprocess.run([EXE, "-m", gold["a_p0_k20.bin"], "-m", gold["a_p1_k20.bin"], "-k", "20", "-t", gold["tree.dat"], "-o", o1, "-c", cf],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(o1, "rb").read() == gold["whole"]
    assert open(cf).read() == gold["kcnt"]
    st = gold["whole_stats"]
    assert "total taxids: %d\n" % st["total_list_entries"] in r.stdout
    assert "singletons: %d\n" % st["singletons"] in r.stdout
    assert "num mapping kmers processed: %d\n" % st["records_written"] in r.stdout
    assert "merge: inputs 2 " in r.stdout
    r = subprocess.run([EXE, "-m", gold["a_p0_k20.bin"], "-i", gold["odd.fa"], "-k", "20", "-t", gold["tree.dat"], "-o", o2], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(o2, "rb").read() == gold["whole"] and "merge: inputs 1 " in r.stdout
    r = subprocess.run([EXE, "-m", str(tmp_path / "none.bin"), "-k", "20", "-t", gold["tree.dat"], "-o", o2 + "x"], capture_output=True, text=True)
    assert r.returncode != 0 and "failed to open" in r.stderr and "none.bin" in r.stderr
