"""The closed form of the decision step for reads of one DOMINANT lineage (kernels.hip k4_wave_path): a table
whose largest kept count sits on one root-to-leaf path, with every other id strictly below it and off that path, is decided without
the sort, the all-pairs pass and the competitor loop -- whatever the closure was.  The references are the general path (k4_part1 /
k4_part2, pinned to the reference's printed records by test_gpu_decide.py) and the same tables with the form switched off
(LMAT_K4_PATH=0: the debug entry reads it per call; the classify kernel's off arm runs in a child process).  Which tables the form
must take is said by the host model of decide_path_tables.py, which test_decide_path_model.py holds against the CPU oracle."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decide_path_tables as dp  # noqa: E402
from test_decide_path_model import forest  # noqa: E402
from test_gpu_decide_chain import BENCH, SMALL, _Pool, _bits, _engine, _params, _pool_bench, _pool_small, _same  # noqa: E402

F = np.float32
FAMILIES = ("sib", "stranger", "two", "genus", "wide", "pair")


class _form_off:
    """LMAT_K4_PATH=0 for the calls inside (the debug entries read the switch per call)."""

    def __enter__(self):
        self.before = os.environ.get("LMAT_K4_PATH")
        os.environ["LMAT_K4_PATH"] = "0"

    def __exit__(self, *a):
        if self.before is None:
            del os.environ["LMAT_K4_PATH"]
        else:
            os.environ["LMAT_K4_PATH"] = self.before


def _three(eng, t, with_cands=False):
    """-> the general path's records, k4_wave's with the form offered (and which path took each table), k4_wave's with the form off"""
    gen = eng.debug_decide_counts(*t.args(), on_the_wave=False)
    got, took = eng.debug_decide_shape(*t.args(), t.shape, with_cands=with_cands)
    with _form_off():
        off, took_off = eng.debug_decide_shape(*t.args(), t.shape, with_cands=with_cands)
    assert (gen["status"] != 255).all()
    assert not took_off.any(), "LMAT_K4_PATH=0 and the form still ran"
    return gen, got, took, off


def _check(eng, t, want_took, what, with_cands=False):
    """Every record of the on arm and of the off arm equals the general path's bit for bit (a table k4_wave's general code declines
    -- status 255: the heapsort turn, two lineage entries of one depth -- is no record); the form took exactly the tables it must."""
    gen, got, took, off = _three(eng, t, with_cands)
    bad = np.nonzero(took != want_took)[0]
    assert bad.size == 0, (what, "took", bad.size, bad[:5], took[bad[:5]], want_took[bad[:5]])
    ok = got["status"] != 255
    assert ok[took == 2].all()
    _same(got[ok], gen[ok], (what, "on"))
    ok_off = off["status"] != 255
    _same(off[ok_off], gen[ok_off], (what, "off"))
    return gen, got, ok, ok_off


def test_path_form_equals_the_general_path_on_250k_tables(tmp_path):
    """Tables of every family of decide_path_tables.build -- v with its path and sibling strains; plus one stranger with its private
    chain, the shared ancestors at c0 + cx; two strangers; genus blocks with one representative per species; nT = 2 and nT = 64 --
    over the small taxonomy and a pool of the benchmark's, cand in {1, 30, 131, 999}, c0 in {1, 2, 3, 4, cand / 2, cand - 1}, path
    counts at c0 or above it, sdiff in {0, 0.5, 1, 3, 1e6}.  The form takes every table the model says it must (took == 2) and
    leaves the ones where a close id's walk would end the scan part-way; all records are the general path's and the off arm's."""
    total = taken = left = 0
    kinds = np.zeros(8, dtype=np.int64)
    seen_nT = np.zeros(65, dtype=np.int64)
    seen_pos = np.zeros(65, dtype=np.int64)
    seen_cand = {}
    off_ok = []
    for branching, mkpool, per in ((SMALL, _pool_small, 2500), (BENCH, _pool_bench, 1800)):
        eng, tax = _engine(tmp_path, branching)
        pool = mkpool(tax)
        for si, sdiff in enumerate((0.0, 0.5, 1.0, 3.0, 1e6)):
            eng.set_params(_params(sdiff))
            for extras in (False, True):
                parts = [dp.build(pool, per, 7000 + 100 * si + 10 * fi + int(extras), fam, extras=extras) for fi, fam in enumerate(FAMILIES)]
                for fam, t in zip(FAMILIES, parts):
                    m = dp.model(t, sdiff)
                    assert m["in_shape"].all()
                    want = np.where(m["partway"], 0, 2).astype(np.uint8)
                    gen, got, ok, ok_off = _check(eng, t, want, (branching, sdiff, extras, fam))
                    assert np.array_equal(_bits(got["stdev"][ok]), _bits(m["stdev"][ok])), "the host's float32 arithmetic is not the device's"
                    total += len(t)
                    taken += int((want == 2).sum())
                    left += int((want == 0).sum())
                    tk = want == 2
                    kinds += np.bincount(gen["match_type"][tk], minlength=8)[:8]
                    seen_nT += np.bincount(t.nT[tk], minlength=65)
                    seen_pos += np.bincount(((t.cn > 0) & (t.ix >= 0)).sum(1)[tk], minlength=65)
                    for c in np.unique(t.cand[tk]):
                        seen_cand[int(c)] = seen_cand.get(int(c), 0) + int((t.cand[tk] == c).sum())
                    off_ok.append(ok_off.mean())
        eng.close()
    assert total >= 250_000 and taken > 220_000 and left > 2000, (total, taken, left)
    assert kinds[0] > 50_000 and kinds[1] > 50_000, kinds                      # direct and multi calls
    assert seen_nT[2] > 1000 and seen_nT[64] > 100, (seen_nT[2], seen_nT[64])
    assert seen_pos[3] > 1000 and seen_pos[4] > 1000, (seen_pos[3], seen_pos[4])
    assert seen_cand.get(1, 0) > 1000 and seen_cand.get(999, 0) > 10_000, seen_cand
    assert min(off_ok) > 0.9, min(off_ok)


def test_one_broken_condition_each_falls_back(tmp_path):
    """An other id at c0 (kept: two kept slots at the maximum; registered behind the kept ones), a path count below c0, an other id
    below v, a path that stops above depth 0, a plasmid id, a PhiX id with the screen on, a candidate buffer (-p): not taken, same
    records.  A PhiX id without the screen is an id like any other."""
    eng, tax = _engine(tmp_path, BENCH)
    pool = _pool_bench(tax)
    eng.set_params(_params(1.0))
    for bi, (brk, fam) in enumerate((("eq_kept", "sib"), ("eq_kept", "wide"), ("eq_anc", "two"), ("ch_below", "stranger"), ("desc", "sib"), ("desc", "wide"))):
        t = dp.build(pool, 4000, 900 + bi, fam, brk=brk)
        m = dp.model(t, 1.0)
        assert t.broken.sum() > 1000 and not m["in_shape"][t.broken].any(), (brk, fam, t.broken.sum())
        want = np.where(m["in_shape"] & ~m["partway"], 2, 0).astype(np.uint8)
        gen, got, ok, ok_off = _check(eng, t, want, (brk, fam))
        assert ok[t.broken].mean() > 0.5, (brk, fam)     # k4_wave's general code decides most of them (the rest: declined, marked)
    # -p: the general code of k4_wave writes the pairs
    t = dp.build(pool, 3000, 950, "stranger")
    gen, got, ok, ok_off = _check(eng, t, np.zeros(len(t), dtype=np.uint8), "candidates", with_cands=True)
    assert ok.mean() > 0.9 and np.array_equal(got["n_cand"][ok], t.nT[ok])
    eng.close()
    # a depth file whose root is at depth 1: the path does not end at depth 0
    eng, tax = _engine(tmp_path, SMALL, root_depth=1)
    t = dp.build(_pool_small(tax), 4000, 960, "stranger")
    gen, got, ok, ok_off = _check(eng, t, np.zeros(len(t), dtype=np.uint8), "root at depth 1")
    assert ok.mean() > 0.5
    eng.close()
    # a plasmid flag / a PhiX flag with screen_phix (and the PhiX id without the screen: an id like any other)
    eng, tax = _engine(tmp_path, BENCH, specials=True)
    nodes = [t_ for t_ in tax.ids if tax.depth[t_] <= 3] + [tax.species_of[tax.leaves[0]], tax.leaves[0], tax.leaves[1], 10000001]
    nodes += tax.path(374840)[:1] + [374840]
    nodes += [x for x in tax.path(tax.leaves[0]) if x not in nodes]
    pool = _Pool(tax, list(dict.fromkeys(nodes)))
    for special, screen in ((10000001, 1), (374840, 1), (374840, 0)):
        eng.set_params(_params(1.0, screen))
        t = dp.build(pool, 6000, 970, "wide", extras=False)
        starts = t.off[:-1].astype(np.int64)
        has = np.add.reduceat((t.tids == special).astype(np.int64), starts) > 0
        phix = (t.tids == 374840) | (t.tids == 32630)      # (the synthetic construct counts as PhiX: tid_checks.hpp)
        flagged = np.add.reduceat(((t.tids == 10000001) | (phix & bool(screen))).astype(np.int64), starts) > 0
        m = dp.model(t, 1.0)
        assert m["in_shape"].all() and not m["partway"].any()
        assert has.sum() > 100 and ((has & flagged).any() if screen else (has & ~flagged).sum() > 100)
        gen, got, ok, ok_off = _check(eng, t, np.where(flagged, 0, 2).astype(np.uint8), (special, screen))
        assert ok.mean() > 0.9
    eng.close()


def _one(ids, cnts, kept, cand):
    """one hand-made table -> Tables-like arguments, and its scores / stdev in the step's own float32 arithmetic"""
    n = len(ids)
    cn = np.zeros((1, 64), dtype=np.int64)
    cn[0, :n] = cnts
    valid = np.arange(64)[None, :] < n
    sc, avg, sd = dp.stats_f32(cn, valid, np.array([cand]))
    args = (np.array(ids, dtype=np.uint32), np.array(cnts, dtype=np.uint32), np.array([0, n], dtype=np.uint64), np.array([cand], dtype=np.uint32))
    return args, np.array([(kept << 8) | (1 << 17)], dtype=np.uint32), sc[0], sd[0]


def _sdiff_for(sd, target):
    """an sdiff with float32(sd * sdiff) == target, or None"""
    s = F(target / sd)
    grid = [s]
    for _ in range(8):
        grid = [np.nextafter(grid[0], F(0))] + grid + [np.nextafter(grid[-1], F(np.inf))]
    ss = [x for x in grid if F(sd * x) == target]
    return float(ss[0]) if ss else None


def test_edges_on_under_and_over_the_thresholds(tmp_path):
    """sdiff is the one free float of `d <= stdev * sdiff`: tuned on the host, in the step's float32 arithmetic (the device's stdev is
    checked against it), until the threshold is exactly d, the float above d (d just under) or the float below (d just over).
      * close / not close: d = s0 - s_j of a sister strain.  On and under: marked, the species is called (Multi).  Over: Direct.
      * the walk that would end part-way: j under another species of v's genus, v's species at c0 + cx; d = s_species - s_j.  On and
        under: taken, Multi at the genus with the genus' score -- above s0 --; over: the general code's (took == 0), same record.
      * no common ancestor of v and a close id (a second tree): LCA error."""
    from lmat_amd import synth
    tax = forest(BENCH)
    d_ = os.path.join(str(tmp_path), "forest")
    p = synth.write_aux_files(d_, tax)
    from lmat_amd import Engine
    eng = Engine(0, _params(1.0))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    a1, a2 = tax.leaves[0], tax.leaves[1]                  # two strains of species A
    sp_a = tax.species_of[a1]
    genus = tax.parent[sp_a]
    sp_b = [s for s in tax.children[genus] if s != sp_a][0]
    b1 = tax.children[sp_b][0]
    above = tax.path(genus)                                 # family .. root
    hit = {k: 0 for k in ("close_on", "close_under", "close_over", "walk_on", "walk_under", "walk_over")}

    def run(args, shape, sdiff):
        eng.set_params(_params(sdiff))
        gen = eng.debug_decide_counts(*args, on_the_wave=False)
        got, took = eng.debug_decide_shape(*args, shape)
        with _form_off():
            off, took_off = eng.debug_decide_shape(*args, shape)
        assert gen["status"][0] != 255 and off["status"][0] != 255 and took_off[0] == 0
        _same(got, gen, ("edge", sdiff))
        _same(off, gen, ("edge off", sdiff))
        return got, int(took[0])

    for cand, c0, cj, cx in ((30, 20, 7, 3), (131, 100, 33, 9), (999, 700, 650, 40), (131, 4, 1, 2), (30, 28, 27, 1), (999, 900, 3, 90)):
        # close / not close: v = a1, its sister a2, the path at c0
        ids = [a1, a2, sp_a, genus] + above
        cn = [c0, cj] + [c0] * (2 + len(above))
        args, shape, sc, sd = _one(ids, cn, 2, cand)
        d = F(sc[0] - sc[1])
        for name, thr in (("on", d), ("under", np.nextafter(d, F(np.inf))), ("over", np.nextafter(d, F(0)))):
            s = _sdiff_for(sd, thr)
            if s is None:
                continue
            got, took = run(args, shape, s)
            assert took == 2 and _bits(got["stdev"])[0] == _bits(np.array([sd]))[0]
            assert int(got["match_type"][0]) == (0 if name == "over" else 1) and int(got["call_tid"][0]) == (a1 if name == "over" else sp_a), (name, got)
            hit["close_" + name] += 1
        # the walk of b1 meets v, then v's species at c0 + cx: the kept ids are v, its sister (cx) and b1 (cj); the closure's are behind
        ids = [a1, a2, b1, sp_a, sp_b, genus] + above
        cjj = min(cj, c0 - 1)
        up = min(c0 + cx + cjj, cand)
        cn = [c0, cx, cjj, min(c0 + cx, cand), cjj, up] + [up] * len(above)
        args, shape, sc, sd = _one(ids, cn, 3, cand)
        d = F(sc[3] - sc[2])
        assert sc[3] > sc[0] and sc[5] > sc[0]
        for name, thr in (("on", d), ("under", np.nextafter(d, F(np.inf))), ("over", np.nextafter(d, F(0)))):
            s = _sdiff_for(sd, thr)
            if s is None or not F(sc[0] - sc[2]) <= thr:
                continue
            got, took = run(args, shape, s)
            assert _bits(got["stdev"])[0] == _bits(np.array([sd]))[0]
            assert took == (0 if name == "over" else 2), (name, took)
            if name != "over":   # v and its species are marked: Multi at the genus, with the largest score from v up to it -- the genus' own
                assert int(got["match_type"][0]) == 1 and int(got["call_tid"][0]) == genus, (name, got)
                assert _bits(got["call_score"])[0] == _bits(np.array([sc[5]]))[0] and got["call_score"][0] > sc[0]
            hit["walk_" + name] += 1
    assert min(hit.values()) >= 3, hit
    # LCA error: a close id of the other tree, with its private chain up to that tree's root
    ids = [a1, 990003, sp_a, genus] + above + [990002, 990001]
    cn = [20, 19] + [20] * (2 + len(above)) + [19, 19]
    args, shape, sc, sd = _one(ids, cn, 2, 30)
    got, took = run(args, shape, 1e6)
    assert took == 2 and int(got["match_type"][0]) == 4 and int(got["call_tid"][0]) == 0, got
    got, took = run(args, shape, 0.0)
    assert took == 2 and int(got["match_type"][0]) == 0 and int(got["call_tid"][0]) == a1, got
    eng.close()


# ---- the kernel test: reads through the classify kernel, default against LMAT_K4_PATH=0 in a child process, and the CPU oracle
KBR = (2, 1, 2, 2, 2, 3)     # 48 strains under 16 species, 8 genera (the fixture of test_gpu_decide_chain.py)
G, BLK = 420, 0.45
N_READS = 4800


def _dataset(tmp):
    from lmat_amd import synth
    tax = synth.make_taxonomy(KBR, specials=False)
    p = synth.write_aux_files(os.path.join(str(tmp), "aux"), tax)
    genomes = synth.make_genomes(tax, G, seed=2002, strain_sub=0.02, genus_block=BLK)
    kmers, lists = synth.build_kmer_table(tax, genomes, k=20, extra_lists=False)
    db = os.path.join(str(tmp), "db.th")
    synth.write_taxhisto(db, kmers, lists, k=20)
    rng = np.random.default_rng(11)
    leaves = list(genomes)
    blk = int(G * BLK)
    reads = []
    for i in range(N_READS):
        li = int(rng.integers(0, len(leaves)))
        g = genomes[leaves[li]]
        kind = i % 5
        # error-free reads behind the genus block / reads with 1 .. 3 substitutions / reads across the end of the genus block /
        # reads inside the genus block (one representative per species) / reads that carry 22 .. 30 bases of a strain of another genus
        if kind < 2 or kind == 4:
            start = int(rng.integers(blk, G - 150 + 1))
        elif kind == 2:
            start = int(rng.integers(max(blk - 140, 0), blk - 10))
        else:
            start = int(rng.integers(0, blk - 150 + 1))
        codes = g[start:start + 150].copy()
        if kind == 1:
            for pos in rng.choice(150, int(rng.integers(1, 4)), replace=False):
                codes[pos] = (codes[pos] + int(rng.integers(1, 4))) & 3
        if kind == 4:
            other = genomes[leaves[(li + len(leaves) // 2) % len(leaves)]]
            ln, at, frm = int(rng.integers(22, 31)), int(rng.integers(0, 120)), int(rng.integers(blk, G - 31))
            codes[at:at + ln] = other[frm:frm + ln]
        if rng.random() < 0.5:
            codes = (3 - codes)[::-1]
        reads.append(np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes())
    return p, db, reads, len(kmers)


def _run(tmp):
    from lmat_amd import Engine, Params
    p, db, seqs, n_kmers = _dataset(tmp)
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    eng.build_db([db], k=20)
    reads = eng.upload_reads(seqs)
    eng.counts_reset()
    before = eng.variant_launches()
    res, _ = eng.classify(reads, 0, len(reads), want_cands=False)
    after = eng.variant_launches()
    counts, nomatch = eng.counts()
    tid = sorted(counts)
    out = {"res": res, "ran": {v: after[v] - before[v] for v in after}, "tally_tid": np.array(tid, dtype=np.uint32),
           "tally_count": np.array([counts[t][0] for t in tid], dtype=np.uint64),
           "tally_score": np.array([counts[t][1] for t in tid], dtype=np.float64), "tally_nomatch": np.array(nomatch, dtype=np.uint64)}
    return eng, reads, out, (p, n_kmers)


def test_classify_kernel_with_and_without_the_path_form(tmp_path):
    """4.8 k reads of 150 bp over the small database of test_gpu_decide_chain.py -- its three kinds of reads, reads inside a
    genus-shared block and reads that carry a stretch of a strain of another genus --: the default run (the plain-run variant, both
    closed forms compiled in), the LMAT_K4_PATH=0 run in a child (the generic kernel without the form) and the CPU oracle give the
    same records and tallies."""
    import oracle_py
    from lmat_amd import Params
    assert os.environ.get("LMAT_K4_PATH") in (None, "1") and os.environ.get("LMAT_K4_CHAIN") in (None, "1") and os.environ.get("LMAT_PLAIN") in (None, "1")
    eng, reads, here, (p, n_kmers) = _run(tmp_path / "here")
    fn = str(tmp_path / "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "child"), fn], env=dict(os.environ, LMAT_K4_PATH="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    assert here["ran"] == {"generic": 0, "plain": 1}
    assert child["ran"] == {"generic": 1, "plain": 0}
    a, b = here["res"], child["res"]
    for f in a.dtype.names:
        bad = np.nonzero(_bits(a[f]) != _bits(b[f]))[0]
        assert bad.size == 0, f"field {f} differs in {bad.size} records, first {int(bad[0])}: {a[f][bad[0]]} != {b[f][bad[0]]}"
    assert a.tobytes() == b.tobytes()
    for t in ("tally_tid", "tally_count", "tally_nomatch"):
        assert np.array_equal(here[t], child[t]), t
    assert np.array_equal(here["tally_score"].view(np.uint64), child["tally_score"].view(np.uint64))
    st = np.bincount(a["status"], minlength=6)
    mt = np.bincount(a["match_type"][a["status"] == 0], minlength=6)
    assert st[0] > 0.9 * N_READS and mt[0] > 500 and mt[1] > 500, (st, mt)
    # the oracle's text against the -p launch of the same reads (candidates: k4_wave's general code), and the records against it
    n = len(reads)
    blob, off = reads.ascii(0, n)
    blob0 = np.append(blob, np.uint8(0))
    eng.set_params(Params.run_rl(prn_all=1))
    eng.counts_reset()
    full, cands = eng.classify(reads, 0, n, want_cands=True, cand_cap=64 * n)
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.set_k(20)
    orc.set_options()
    kms = np.unique(np.concatenate([orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(n)]))
    counts, tids = eng.lookup(kms, stride=32)
    orc.add_lists32(kms, counts, tids)
    want, tally, nomatch = orc.classify(blob0, off, 20)
    orc.close()
    got = eng.format_out(full, cands, (blob0, off))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got.split("\n"), want.split("\n"))) if g != w]
    assert not bad, f"{len(bad)} differing records, first: {bad[0]}"
    assert got == want
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel"):
        assert np.array_equal(_bits(a[f]), _bits(full[f])), f
    assert here["tally_nomatch"].tolist() == list(nomatch)
    assert dict(zip(here["tally_tid"].tolist(), here["tally_count"].tolist())) == {t: c for t, (c, s) in tally.items()}
    reads.free()
    eng.close()


if __name__ == "__main__":   # the child: the same reads with whatever LMAT_K4_PATH says, pickled
    sys.path.insert(0, ROOT)
    _eng, _reads, _out, _ = _run(sys.argv[1])
    _reads.free()
    _eng.close()
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_out, _f)
