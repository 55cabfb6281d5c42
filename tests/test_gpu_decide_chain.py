"""The closed form of the decision step for reads of one lineage (kernels.hip k4_wave_chain): a table whose
closure found ONE eligible id and registered all its ancestors is decided without the sort, the all-pairs pass and the competitor
loop.  The general path (k4_part1 / k4_part2: pinned to the reference's printed records by test_gpu_decide.py) is the reference
here; LMAT_K4_CHAIN=0, read once per process, is the off arm of the kernel test -- that run is a child process."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SMALL = (2, 3, 2, 3)            # 57 nodes, chains of 1 .. 4
BENCH = (3, 4, 4, 4, 4, 3)      # the benchmark's taxonomy: chains of up to 6
SDIFFS = (0.0, 0.5, 1.0, 3.0, 1e6)
CANDS = (1, 30, 131, 999)
FIELDS = ("status", "match_type", "cand_kmer_cnt", "call_tid", "valid_kmers", "read_len", "bin_sel")
FLOATS = ("call_score", "log_avg", "stdev")


class _Pool:
    """A set of taxonomy nodes tables are drawn from, with their relations as matrices."""

    def __init__(self, tax, nodes):
        self.tids = np.array(nodes, dtype=np.int64)
        ix = {t: i for i, t in enumerate(nodes)}
        M = len(nodes)
        self.depth = np.array([tax.depth[t] for t in nodes], dtype=np.int64)
        self.anc = np.zeros((M, M), dtype=bool)          # anc[i, j]: j is a proper ancestor of i
        self.chain = np.full((M, 8), -1, dtype=np.int64)   # chain[i, d]: the ancestor d + 1 steps up (parent first), -1 behind the root
        for i, t in enumerate(nodes):
            for d, a in enumerate(tax.path(t)):
                self.anc[i, ix[a]] = True                # (a pool is closed under "parent of")
                self.chain[i, d] = ix[a]
        self.rel = self.anc | self.anc.T | np.eye(M, dtype=bool)


def _pool_small(tax):
    return _Pool(tax, list(tax.ids))


def _pool_bench(tax):
    """160 nodes of the benchmark's taxonomy: two whole genera (strains included), their ancestors, and every node of the first
    three levels -- so that an unrelated id exists under another species, genus, family, phylum and superkingdom."""
    keep = [t for t in tax.ids if tax.depth[t] <= 3]
    genera = [t for t in tax.ids if tax.rank[t] == "genus"]
    for g in (genera[0], genera[1], genera[-1]):
        keep += [g] + tax.children[g] + [s for sp in tax.children[g] for s in tax.children[sp]]
    keep = list(dict.fromkeys(keep))
    return _Pool(tax, keep)


def _tables(pool, n, seed, c0_of=None, break_with=None):
    """n tables shaped as a closure with one eligible id leaves them -> tids, counts, off, cand, kept, eligible, qualifies.
    break_with: "eq" / "gt" (an other id with count = / > c0), "desc" (an other id below the eligible one)."""
    rng = np.random.default_rng(seed)
    M = pool.tids.size
    deep = np.nonzero(pool.depth >= 1)[0]
    if break_with == "desc":
        deep = np.array([i for i in deep if pool.anc[:, i].any()])     # ids with descendants in the pool
    rep = deep[rng.integers(0, deep.size, n)]
    clen = pool.depth[rep]                                             # the whole chain, down to depth 0
    cand = np.array(CANDS)[rng.integers(0, len(CANDS), n)]
    pick = rng.integers(0, 6, n)
    c0 = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4], [1, 2, 3, 4, cand - 1], cand)
    c0 = np.clip(c0, 1, cand)
    # the others: unrelated to the eligible id; for a third of the tables only from below one of its ancestors (siblings, cousins:
    # several others sharing one LCA), else from anywhere (the LCA lands on every level, the root included)
    ok = ~pool.rel[rep]
    up = pool.chain[rep, np.minimum(rng.integers(0, 4, n), clen - 1)]
    near = rng.random(n) < 0.35
    ok &= np.where(near[:, None], pool.anc[:, up].T, True)
    n_ok = ok.sum(1)
    room = 63 - clen
    want = np.where(rng.random(n) < 0.5, rng.integers(0, 5, n), rng.integers(0, 64, n))
    want = np.where(rng.random(n) < 0.08, room, want)                  # nT = 64 exactly, where the pool has that many
    want = np.where(c0 > 1, np.minimum(np.minimum(want, room), n_ok), 0)   # (a count below c0 = 1 does not exist)
    key = np.where(ok, rng.random((n, M)), 2.0)
    order = np.argsort(key, axis=1)
    n_oth = want
    if break_with == "desc":
        n_oth = np.maximum(n_oth, 1)
    kept_n = 1 + n_oth
    nT = kept_n + clen
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(nT, out=off[1:])
    tids = np.zeros(int(off[-1]), dtype=np.int64)
    cnts = np.zeros(int(off[-1]), dtype=np.int64)
    elig = rng.integers(0, kept_n)
    o = off[:-1].astype(np.int64)
    # kept slots: the others in drawn order, the eligible id swapped into its slot
    col = np.arange(min(63, M))[None, :]
    sel = col < n_oth[:, None]
    rows = np.nonzero(sel)[0]
    slot = col.repeat(n, 0)[sel]
    slot = np.where(slot >= elig[rows], slot + 1, slot)
    tids[o[rows] + slot] = order[:, :col.size][sel]
    lv = rng.integers(1, 5, n)                                           # few distinct counts: equal counts (and depths) among the others
    cj = 1 + (rng.integers(0, lv[rows]) * np.maximum(c0[rows] - 1, 1)) // lv[rows]
    cj = np.where(rng.random(rows.size) < 0.5, rng.integers(1, np.maximum(c0[rows], 2)), cj)
    cj = np.minimum(cj, np.maximum(c0[rows] - 1, 0))
    cj = np.where(rng.random(rows.size) < 0.05, 0, cj)                   # a kept id no position counted for (fewer positive counts than ids)
    cnts[o[rows] + slot] = cj
    tids[o + elig] = rep
    cnts[o + elig] = c0
    for d in range(8):
        m = clen > d
        tids[o[m] + kept_n[m] + d] = pool.chain[rep[m], d]
        cnts[o[m] + kept_n[m] + d] = c0[m]
    rev = rng.random(n) < 0.2                                            # the chain root first: the order of the chain slots is not part of the shape
    for i in np.nonzero(rev)[0]:
        a, b = int(o[i] + kept_n[i]), int(o[i] + nT[i])
        tids[a:b] = tids[a:b][::-1].copy()
    if break_with in ("eq", "gt", "desc"):
        first_other = o + (elig == 0)                                    # a kept slot that is not the eligible one
        if break_with == "desc":
            below = np.array([rng.choice(np.nonzero(pool.anc[:, r])[0]) for r in rep])
            tids[first_other] = below
            cnts[first_other] = np.maximum(c0 - 1, 0)
        else:
            has = n_oth > 0
            cnts[first_other[has]] = c0[has] + (1 if break_with == "gt" else 0)
            cand = np.maximum(cand, c0 + 1)
    return (pool.tids[tids].astype(np.uint32), cnts.astype(np.uint32), off, cand.astype(np.uint32), kept_n.astype(np.uint32),
            elig.astype(np.uint32), n_oth)


def _params(sdiff=1.0, screen_phix=1):
    """bin/run_rl.sh's flags with -b sdiff (and the PhiX screen on or off)."""
    from lmat_amd import Params
    p = Params.run_rl()
    p.sdiff, p.screen_phix = sdiff, screen_phix
    return p


def _bits(x):
    return np.ascontiguousarray(x).view(f"u{x.dtype.itemsize}")


def _same(got, want, what, skip=()):
    for f in FIELDS:
        if f not in skip:
            assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:5])
    for f in FLOATS:
        assert np.array_equal(_bits(got[f]), _bits(want[f])), (what, f, np.nonzero(_bits(got[f]) != _bits(want[f]))[0][:5])


def _engine(tmp, branching, sdiff=1.0, specials=False, root_depth=0, screen_phix=1):
    from lmat_amd import Engine, Params, synth
    tax = synth.make_taxonomy(branching, specials=specials)
    if root_depth:
        for t in tax.ids:
            tax.depth[t] += root_depth
    d = os.path.join(str(tmp), "tax_%s_%d_%d" % ("".join(map(str, branching)), int(specials), root_depth))
    p = synth.write_aux_files(d, tax)
    eng = Engine(0, _params(sdiff, screen_phix))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    if root_depth:
        for t in tax.ids:
            tax.depth[t] -= root_depth
    return eng, tax


def _both(eng, t, with_cands=False):
    tids, cnts, off, cand, kept, elig = t[:6]
    gen = eng.debug_decide_counts(tids, cnts, off, cand, on_the_wave=False)
    got, took = eng.debug_decide_chain(tids, cnts, off, cand, kept, elig, with_cands=with_cands)
    return gen, got, took


def _f32_stats(counts, cand):
    """log_avg and stdev as the decision step computes them (read_label.cpp:803-880), in float32, sums in slot order."""
    f = np.float32
    sc = [f(c) / f(cand) for c in counts]
    s = f(0)
    for x in sc:
        s = f(s + x)
    pos = sum(c > 0 for c in counts)
    use = pos if pos > 3 else len(counts)
    avg = f(s / f(use))
    v = f(0)
    for c, x in zip(counts, sc):
        d = f(avg - x)
        v = f(v + (f(d * d) if (c > 0 or pos <= 3) else f(0)))
    sd = f(np.sqrt(f(v / f(use - 1)))) if use > 1 else f(0)
    return sc, avg, sd


def test_closed_form_equals_the_general_path_on_200k_tables(tmp_path):
    """Tables built as `lone` closures leave them, over the small taxonomy (chains of 1 .. 4) and a pool of the benchmark's (chains
    of up to 6, up to 64 slots): the chain complete, 0 .. 63 - chain others unrelated to the eligible id (siblings, ids below
    another species / genus / family / phylum / superkingdom, several below one LCA), their counts below c0, c0 in
    {1, 2, 3, 4, cand - 1, cand}, cand in {1, 30, 131, 999}, sdiff in {0, 0.5, 1, 3, 1e6}.  Every such table is TAKEN by the closed
    form, and every record equals the general path's bit for bit.  Tables that break one condition each are not taken and still
    equal.  Differences on, one ulp under and one ulp over the threshold: sdiff is the one free float of the comparison
    `s0 - s_j <= stdev * sdiff`, so for a handful of three- to ten-slot tables it is tuned on the host (float32 arithmetic in
    the step's own order; the device's stdev is checked against it) until the product is d, the float below d, the float above."""
    from lmat_amd import Params, synth
    total = 0
    kinds = np.zeros(8, dtype=np.int64)
    full64 = 0
    for branching, mkpool, per in ((SMALL, _pool_small, 28_000), (BENCH, _pool_bench, 12_000)):
        eng, tax = _engine(tmp_path, branching)
        pool = mkpool(tax)
        for si, sdiff in enumerate(SDIFFS):
            eng.set_params(_params(sdiff))
            t = _tables(pool, per, 1000 * len(branching) + si)
            gen, got, took = _both(eng, t)
            assert (gen["status"] != 255).all()
            assert took.all(), ("qualifying tables not taken", branching, sdiff, int((took == 0).sum()), np.nonzero(took == 0)[0][:5])
            _same(got, gen, (branching, sdiff))
            total += per
            kinds += np.bincount(gen["match_type"], minlength=8)[:8]
            full64 += int((np.diff(t[2].astype(np.int64)) == 64).sum())
        # one broken condition each: not taken, same records
        eng.set_params(_params(1.0))
        for how in ("eq", "gt", "desc"):
            t = _tables(pool, 4000, 77, break_with=how)
            gen, got, took = _both(eng, t)
            broken = t[6] > 0
            assert broken.sum() > 1000 and not took[broken].any(), how
            ok = got["status"] != 255
            assert ok[broken].mean() > 0.5, how                      # k4_wave's general code decides most of them (the rest: declined, marked)
            _same(got[ok], gen[ok], how)
            total += 4000
        # cand = 1000: outside k4_wave altogether
        t = list(_tables(pool, 2000, 78))
        t[3] = np.full(2000, 1000, dtype=np.uint32)
        gen, got, took = _both(eng, t)
        assert not took.any() and (got["status"] == 255).all() and (gen["status"] != 255).all()
        # a candidate buffer present (-p): the general code of k4_wave writes the pairs; the record is the same but for them
        t = _tables(pool, 2000, 79)
        gen, got, took = _both(eng, t, with_cands=True)
        assert not took.any()
        ok = got["status"] != 255
        assert ok.mean() > 0.9
        _same(got[ok], gen[ok], "candidates")
        assert np.array_equal(got["n_cand"][ok], np.diff(t[2].astype(np.int64))[ok])
        total += 4000
        eng.close()
    assert total >= 200_000 + 8000
    assert kinds[0] > 5000 and kinds[1] > 5000 and kinds[4] == 0, kinds   # direct and multi matches; one root: no LCA error here
    assert full64 > 100
    # a depth file whose root is at depth 1: the chain does not end at depth 0
    eng, tax = _engine(tmp_path, SMALL, root_depth=1)
    t = _tables(_pool_small(tax), 4000, 80)
    gen, got, took = _both(eng, t)
    assert not took.any()
    ok = got["status"] != 255
    assert ok.mean() > 0.5
    _same(got[ok], gen[ok], "root at depth 1")
    eng.close()
    # a plasmid flag / a PhiX flag with screen_phix (and the PhiX id without the screen: taken)
    eng, tax = _engine(tmp_path, (3, 4, 4, 4, 4, 3), specials=True)
    nodes = [t_ for t_ in tax.ids if tax.depth[t_] <= 3] + [tax.species_of[tax.leaves[0]], tax.leaves[0], tax.leaves[1], 10000001]
    nodes += tax.path(374840)[:1] + [374840]
    nodes += [x for x in tax.path(tax.leaves[0]) if x not in nodes]
    pool = _Pool(tax, list(dict.fromkeys(nodes)))
    for special, screen in ((10000001, 1), (374840, 1), (374840, 0)):
        eng.set_params(_params(1.0, screen))
        t = _tables(pool, 6000, 81)
        starts = t[2][:-1].astype(np.int64)
        has = np.add.reduceat((t[0] == special).astype(np.int64), starts) > 0
        phix = (t[0] == 374840) | (t[0] == 32630)          # (the synthetic construct, at depth 3 in the pool, counts as PhiX: tid_checks.hpp)
        flagged = np.add.reduceat(((t[0] == 10000001) | (phix & bool(screen))).astype(np.int64), starts) > 0
        gen, got, took = _both(eng, t)
        assert has.sum() > 100
        assert not took[flagged].any() and took[~flagged].all(), (special, screen)
        assert (has & flagged).any() if screen else (has & ~flagged).sum() > 100   # (without the screen a PhiX id is an id like any other)
        ok = got["status"] != 255
        assert ok.mean() > 0.9
        _same(got[ok], gen[ok], (special, screen))
    # on / under / over the threshold
    tax_ix = {t_: i for i, t_ in enumerate(pool.tids.tolist())}
    strain = tax.leaves[1]
    chain = tax.path(strain)
    other = tax.leaves[0]                       # its sister strain: LCA = the species
    hit = {"on": 0, "under": 0, "over": 0}
    for cand, c0, cj, clen_extra in ((30, 20, 7, 0), (131, 100, 33, 0), (999, 700, 650, 1), (131, 4, 1, 1), (30, 29, 28, 0), (999, 998, 3, 1)):
        ids = [strain, other] + ([tax.leaves[2]] if clen_extra else []) + chain
        cn = [c0, cj] + ([max(cj - 1, 0)] if clen_extra else []) + [c0] * len(chain)
        sc, avg, sd = _f32_stats(cn, cand)
        d = np.float32(sc[0] - sc[1])
        assert sd > 0
        s = np.float32(d / sd)
        grid = [s]
        for _ in range(8):
            grid = [np.nextafter(grid[0], np.float32(0))] + grid + [np.nextafter(grid[-1], np.float32(np.inf))]
        want = {"on": d, "under": np.nextafter(d, np.float32(0)), "over": np.nextafter(d, np.float32(np.inf))}
        for name, target in want.items():
            ss = [x for x in grid if np.float32(sd * x) == target]
            if not ss:
                continue
            eng.set_params(_params(float(ss[0])))
            off = np.array([0, len(ids)], dtype=np.uint64)
            t = (np.array(ids, dtype=np.uint32), np.array(cn, dtype=np.uint32), off, np.array([cand], dtype=np.uint32),
                 np.array([len(ids) - len(chain)], dtype=np.uint32), np.array([0], dtype=np.uint32))
            gen, got, took = _both(eng, t)
            assert took.all()
            assert _bits(got["stdev"])[0] == _bits(np.array([sd]))[0]        # the host's arithmetic is the device's: the product is what was aimed at
            _same(got, gen, (name, cand, c0, cj))
            # d <= threshold marks the strain (the species is called: Multi); the float under d leaves the call Direct
            assert int(got["match_type"][0]) == (0 if name == "under" else 1), (name, got)
            hit[name] += 1
    assert min(hit.values()) >= 3, hit
    eng.close()


# ---- the kernel test: reads through the classify kernel, default against LMAT_K4_CHAIN=0 in a child process
KBR = (2, 1, 2, 2, 2, 3)     # 48 strains under 16 species, 8 genera
G, BLK = 420, 0.45           # bases per genome; the share of it that is one block per genus
N_READS = 4200


def _dataset(tmp):
    from lmat_amd import synth
    tax = synth.make_taxonomy(KBR, specials=False)
    p = synth.write_aux_files(os.path.join(str(tmp), "aux"), tax)
    genomes = synth.make_genomes(tax, G, seed=2002, strain_sub=0.02, genus_block=BLK)
    kmers, lists = synth.build_kmer_table(tax, genomes, k=20, extra_lists=False)
    db = os.path.join(str(tmp), "db.th")
    synth.write_taxhisto(db, kmers, lists, k=20)
    rng = np.random.default_rng(9)
    leaves = list(genomes)
    blk = int(G * BLK)
    reads = []
    for i in range(N_READS):
        g = genomes[leaves[int(rng.integers(0, len(leaves)))]]
        kind = i % 3
        # error-free reads behind the genus block / reads with 1 .. 3 substitutions / reads across the end of the genus block
        start = int(rng.integers(blk, G - 150 + 1)) if kind < 2 else int(rng.integers(max(blk - 140, 0), blk - 10))
        codes = g[start:start + 150].copy()
        if kind == 1:
            for pos in rng.choice(150, int(rng.integers(1, 4)), replace=False):
                codes[pos] = (codes[pos] + int(rng.integers(1, 4))) & 3
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


def test_classify_kernel_with_and_without_the_closed_form(tmp_path):
    """4.2 k reads of 150 bp over a database of a few thousand k-mers -- error-free reads of one strain, reads with 1 .. 3
    substitutions, reads across the end of a genus-shared block --: the default run (the plain-run variant, closed form compiled in)
    and the LMAT_K4_CHAIN=0 run in a child (the generic kernel without it) give the same records and tallies byte for byte, and
    both are the oracle's text, compared as the parity tests compare it."""
    import oracle_py
    from lmat_amd import Params
    assert os.environ.get("LMAT_K4_CHAIN") in (None, "1") and os.environ.get("LMAT_PLAIN") in (None, "1")
    eng, reads, here, (p, n_kmers) = _run(tmp_path / "here")
    assert 2000 < n_kmers < 20000
    fn = str(tmp_path / "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "child"), fn], env=dict(os.environ, LMAT_K4_CHAIN="0"),
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
    assert st[0] > 0.9 * N_READS and mt[0] > 500 and mt[1] > 500, (st, mt)   # direct and multi calls both occur
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


if __name__ == "__main__":   # the child: the same reads with whatever LMAT_K4_CHAIN says, pickled
    sys.path.insert(0, ROOT)
    _eng, _reads, _out, _ = _run(sys.argv[1])
    _reads.free()
    _eng.close()
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_out, _f)
