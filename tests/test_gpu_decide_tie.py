"""The closed form of the decision step for reads with TIED ids at the top (kernels.hip k4_wave_tie): a table whose
largest kept count is held by two or more ids of one depth -- sibling strains no k-mer tells apart, the strains of a genus-shared
block -- is decided without the sort, the all-pairs pass, the second fetch of the ancestors and the competitor loop.  The references
are the general path (k4_part1 / k4_part2, pinned to the reference's printed records by test_gpu_decide.py) and the same tables with
the form switched off (LMAT_K4_TIE=0: the debug entry reads it per call; the classify kernel's off arm runs in a child process) or
not offered (no bit 18 in the closure's word).  Which tables the form must take is said by the host model of decide_tie_tables.py,
which test_decide_tie_model.py holds against the CPU oracle."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decide_tie_tables as dt  # noqa: E402
from test_decide_path_model import forest  # noqa: E402
from test_gpu_decide_chain import BENCH, SMALL, _Pool, _bits, _engine, _params, _pool_bench, _same  # noqa: E402

SDIFFS = (0.0, 0.5, 1.0, 3.0, 1e6)


class _form_off:
    """LMAT_K4_TIE=0 for the calls inside (the debug entries read the switch per call)."""

    def __enter__(self):
        self.before = os.environ.get("LMAT_K4_TIE")
        os.environ["LMAT_K4_TIE"] = "0"

    def __exit__(self, *a):
        if self.before is None:
            del os.environ["LMAT_K4_TIE"]
        else:
            os.environ["LMAT_K4_TIE"] = self.before


def _check(eng, t, want_took, what, with_cands=False):
    """Every record of the on arm, of the off arm and of the arm without bit 18 equals the general path's bit for bit (a table
    k4_wave's general code declines -- status 255 -- is no record); the form took exactly the tables it must, and none when off."""
    gen = eng.debug_decide_counts(*t.args(), on_the_wave=False)
    got, took = eng.debug_decide_shape(*t.args(), t.shape, with_cands=with_cands)
    with _form_off():
        off, took_off = eng.debug_decide_shape(*t.args(), t.shape, with_cands=with_cands)
    nob, took_nob = eng.debug_decide_shape(*t.args(), t.without_bit18(), with_cands=with_cands)
    assert (gen["status"] != 255).all()
    assert not (took_off == 3).any(), "LMAT_K4_TIE=0 and the form still ran"
    assert not (took_nob == 3).any(), "no bit 18 and the form still ran"
    bad = np.nonzero(took != want_took)[0]
    assert bad.size == 0, (what, "took", bad.size, bad[:5], took[bad[:5]], want_took[bad[:5]], [t.rows[i] for i in bad[:2]])
    ok = got["status"] != 255
    assert ok[took == 3].all()
    _same(got[ok], gen[ok], (what, "on"))
    for arm, name in ((off, "off"), (nob, "no bit 18")):
        ok_arm = arm["status"] != 255
        _same(arm[ok_arm], gen[ok_arm], (what, name))
    return gen, got, ok


def _forest_engine(tmp, branching):
    from lmat_amd import Engine, synth
    tax = forest(branching)
    p = synth.write_aux_files(os.path.join(str(tmp), "forest"), tax)
    eng = Engine(0, _params(1.0))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    return eng, tax


def test_tie_form_equals_the_general_path(tmp_path):
    """Tables of every family of decide_tie_tables.build that must be taken -- two tied children of a root (nT = 3), 2 and 3 tied
    siblings with and without a lower one, a genus block of 12 strains under 4 species, the same with a stranger that lifts the
    shared ancestors above c0, nT = 64 exactly -- and tables with two strangers, over a small forest and a pool of the benchmark's
    taxonomy, cand in {1, 30, 131, 999}, sdiff in {0, 0.5, 1, 3, 1e6}.  The form takes every table the model says it must (took == 3)
    and leaves those where a close id's walk would end the scan part-way; all records are the general path's; with a candidate
    buffer (-p) no table is taken."""
    total = taken = left = 0
    kinds = np.zeros(8, dtype=np.int64)
    seen_nT = np.zeros(65, dtype=np.int64)
    seen_cand = set()
    for bi in range(2):
        if bi == 0:
            eng, tax = _forest_engine(tmp_path, SMALL)
            pool = _Pool(tax, list(tax.ids))
        else:
            eng, tax = _engine(tmp_path, BENCH)
            pool = _pool_bench(tax)
        for si, sdiff in enumerate(SDIFFS):
            eng.set_params(_params(sdiff))
            for fi, fam in enumerate(dt.TAKEN + ("two",)):
                if fam in ("wide", "sib3low") and bi == 0:
                    continue
                t = dt.build(pool, 150, 3000 + 1000 * bi + 100 * si + fi, fam)
                m = dt.model(t, sdiff)
                assert m["in_shape"].all() and (fam == "two" or not m["partway"].any())
                want = np.where(m["partway"], 0, 3).astype(np.uint8)
                gen, got, ok = _check(eng, t, want, (bi, sdiff, fam))
                assert np.array_equal(_bits(got["stdev"][ok]), _bits(m["stdev"][ok])), "the host's float32 arithmetic is not the device's"
                tk = want == 3
                assert np.array_equal(gen["match_type"][tk], m["match"][tk])
                total += len(t)
                taken += int(tk.sum())
                left += int((~tk).sum())
                kinds += np.bincount(gen["match_type"][tk], minlength=8)[:8]
                seen_nT += np.bincount(t.nT[tk], minlength=65)
                seen_cand |= set(t.cand[tk].tolist())
                if si == 2 and fam in ("genus", "genus_stranger", "sib2"):
                    _check(eng, t, np.zeros(len(t), dtype=np.uint8), (bi, fam, "candidates"), with_cands=True)
        eng.close()
    assert total > 10_000 and taken > 9_500 and left > 20, (total, taken, left)
    assert kinds[0] == 0 and kinds[2] == 0 and kinds[1] > 8000 and kinds[4] > 20, kinds   # Multi and the LCA error; never Direct, never Partial
    assert seen_nT[3] > 500 and seen_nT[64] > 500 and seen_nT[17:].sum() > 2000, (seen_nT[3], seen_nT[64])
    assert seen_cand == {1, 30, 131, 999}


def test_one_broken_condition_each_falls_back(tmp_path):
    """Tied ids of unequal depth, a PRIVATE count of c0 + 1 / c0 - 1, a slot above c0 outside COMMON, a COMMON count that falls
    towards the root or lies below c0, an id below a tied id, a registered id at c0 that is no ancestor, the deepest common ancestor
    among the kept slots, an ancestor without a slot, a plasmid id, a PhiX id with the screen on: not taken, same records.  A PhiX id
    without the screen is an id like any other."""
    eng, tax = _engine(tmp_path, BENCH)
    pool = _pool_bench(tax)
    eng.set_params(_params(1.0))
    for fi, fam in enumerate(dt.BROKEN):
        t = dt.build(pool, 300, 600 + fi, fam)
        m = dt.model(t, 1.0)
        assert not m["in_shape"].any(), fam
        gen, got, ok = _check(eng, t, np.zeros(len(t), dtype=np.uint8), fam)
        assert ok.mean() > 0.5, (fam, ok.mean())     # k4_wave's general code decides most of them (the rest: declined, marked)
    eng.close()
    eng, tax = _engine(tmp_path, BENCH, specials=True)
    nodes = [t_ for t_ in tax.ids if tax.depth[t_] <= 3] + [tax.species_of[tax.leaves[0]]] + list(tax.children[tax.species_of[tax.leaves[0]]]) + [10000001]
    nodes += tax.path(374840)[:1] + [374840]
    nodes += [x for leaf in (tax.leaves[0], 10000001, 374840) for x in tax.path(leaf) if x not in nodes]
    nodes = list(dict.fromkeys(nodes))
    pool = _Pool(tax, nodes)
    for special, screen in ((10000001, 1), (374840, 1), (374840, 0)):
        eng.set_params(_params(1.0, screen))
        # (the synthetic construct counts as PhiX: tid_checks.hpp; a family may draw a flagged id among its own as well)
        flagged = [nodes.index(x) for x in ((10000001,) + ((374840, 32630) if screen else ())) if x in nodes]
        for fam in ("sib2", "sib3"):
            t = dt.build(pool, 300, 700 + special % 7 + screen, fam, special=nodes.index(special))
            m = dt.model(t, 1.0, flagged=flagged)
            carries = np.array([any(ix_ in flagged for ix_ in r[0]) for r in t.rows])
            assert np.array_equal(m["in_shape"], ~carries) and not m["partway"].any()
            assert carries.all() if nodes.index(special) in flagged else (~carries).sum() > 200, (special, screen, carries.sum())
            want = np.where(m["in_shape"], 3, 0).astype(np.uint8)
            gen, got, ok = _check(eng, t, want, (special, screen, fam))
            assert ok.mean() > 0.9
    eng.close()


# ---- the kernel test: reads through the classify kernel, default against LMAT_K4_TIE=0 in a child process, and the CPU oracle
KBR = (2, 1, 2, 2, 2, 3)     # 48 strains under 16 species, 8 genera (the fixture of test_gpu_decide_chain.py)
G, BLK = 420, 0.45
N_READS = 4800


def _dataset(tmp):
    from lmat_amd import synth
    tax = synth.make_taxonomy(KBR, specials=False)
    p = synth.write_aux_files(os.path.join(str(tmp), "aux"), tax)
    genomes = synth.make_genomes(tax, G, seed=2002, strain_sub=0.004, genus_block=BLK)   # (few substitutions: sibling strains often tie)
    # every k-mer with the strains that own it and nothing else (synth.build_kmer_table adds the nodes up to their LCA, as tax_histo
    # does: kept ids at c0 above the tied strains, i.e. tied ids of unequal depth -- the general code's)
    owners = {}
    for leaf, g in genomes.items():
        for km in np.unique(synth.kmers_of(g, 20)).tolist():
            owners.setdefault(km, []).append(leaf)
    kmers = np.array(sorted(owners), dtype=np.uint64)
    lists = [sorted(owners[km], key=lambda x: (x * 2654435761) & 0xFFFFFFFF) for km in kmers.tolist()]
    db = os.path.join(str(tmp), "db.th")
    synth.write_taxhisto(db, kmers, lists, k=20)
    rng = np.random.default_rng(13)
    leaves = list(genomes)
    blk = int(G * BLK)
    reads = []
    for i in range(N_READS):
        li = int(rng.integers(0, len(leaves)))
        g = genomes[leaves[li]]
        kind = i % 6
        # error-free reads behind the genus block (sibling strains that no k-mer of the read tells apart) / reads with 1 .. 3
        # substitutions / reads across the end of the genus block / reads inside the genus block (every strain of the genus) / reads
        # behind the block, and (5) inside it, that carry 22 .. 30 bases of a strain of another genus
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
        if kind >= 4:
            other = genomes[leaves[(li + len(leaves) // 2) % len(leaves)]]
            ln, at, frm = int(rng.integers(22, 31)), int(rng.integers(0, 120)), int(rng.integers(blk, G - 31))
            codes[at:at + ln] = other[frm:frm + ln]
        if rng.random() < 0.5:
            codes = (3 - codes)[::-1]
        reads.append(np.frombuffer(b"ACGT", dtype=np.uint8)[codes].tobytes())
    return p, db, reads, tax


def _run(tmp):
    from lmat_amd import Engine, Params
    p, db, seqs, tax = _dataset(tmp)
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
    return eng, reads, out, (p, tax)


def test_classify_kernel_with_and_without_the_tie_form(tmp_path):
    """4.8 k reads of 150 bp over the small database of test_gpu_decide_chain.py with its genus-shared block: the default run (the
    plain-run variant, the three closed forms compiled in), the LMAT_K4_TIE=0 run in a child (the generic kernel without the form)
    and the CPU oracle give the same records and tallies.  The tables the reads form (rebuilt from the -p launch and the lists of
    their k-mers) go through the debug entry: sibling ties, genus ties and ties with a stranger are each taken by the form."""
    import oracle_py
    from lmat_amd import Params
    assert all(os.environ.get(v) in (None, "1") for v in ("LMAT_K4_TIE", "LMAT_K4_PATH", "LMAT_K4_CHAIN", "LMAT_PLAIN"))
    eng, reads, here, (p, tax) = _run(tmp_path / "here")
    fn = str(tmp_path / "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "child"), fn], env=dict(os.environ, LMAT_K4_TIE="0"),
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
    per_read = [orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(n)]
    kms = np.unique(np.concatenate(per_read))
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
    # the tables of the reads: ids and counts from the pairs of the -p launch (count = score * cand, exactly), the kept ids from the
    # lists of the read's k-mers, kept slots first.  Through the debug entry with the form offered: which of them it takes.
    counts = np.asarray(counts).reshape(-1)
    tids = np.asarray(tids).reshape(kms.size, -1)
    listed = {int(k): set(int(x) for x in tids[j, :int(counts[j])]) for j, k in enumerate(kms)}
    T_tid, T_cnt, T_off, T_cand, T_shape, T_kind, T_read = [], [], [0], [], [], [], []
    skipped = {"record": 0, "kept": 0, "no tie": 0}
    for i in range(n):
        nc, co, cand = int(full["n_cand"][i]), int(full["cand_off"][i]), int(full["cand_kmer_cnt"][i])
        if full["status"][i] != 0 or nc < 3 or nc > 64 or len(T_cand) >= 1500:
            skipped["record"] += 1
            continue
        ids = [int(x) for x in cands["tid"][co:co + nc]]
        cn = [int(round(float(s) * cand)) for s in cands["score"][co:co + nc]]
        kept_ids = set().union(*[listed.get(int(k), set()) for k in per_read[i]])
        kept = [j for j in range(nc) if ids[j] in kept_ids]
        rest = [j for j in range(nc) if ids[j] not in kept_ids]
        if len(kept) < 2 or not rest:
            skipped["kept"] += 1
            continue
        c0 = max(cn[j] for j in kept)
        top = [ids[j] for j in kept if cn[j] == c0]
        if len(top) < 2:
            skipped["no tie"] += 1
            continue
        # sibling tie: the tied ids have one parent; genus tie: they do not; with a stranger: a kept id outside the subtree of their
        # deepest common ancestor
        paths = [tax.path(t) for t in top]
        shared = [x for x in paths[0] if all(x in q for q in paths[1:])]
        stranger = bool(shared) and any(shared[0] not in tax.path(ids[j]) for j in kept)
        kind = 2 if stranger else (0 if len({q[0] for q in paths}) == 1 else 1)
        order = kept + rest
        T_tid += [ids[j] for j in order]
        T_cnt += [cn[j] for j in order]
        T_off.append(len(T_tid))
        T_cand.append(cand)
        T_shape.append((len(kept) << 8) | (3 << 17))
        T_kind.append(kind)
        T_read.append(i)
    assert len(T_cand) > 100, (skipped, len(listed), int(counts.max()), int(full["n_cand"].max()))
    eng.set_params(Params.run_rl(prn_all=0))
    args = (np.array(T_tid, dtype=np.uint32), np.array(T_cnt, dtype=np.uint32), np.array(T_off, dtype=np.uint64), np.array(T_cand, dtype=np.uint32))
    rec, took = eng.debug_decide_shape(*args, np.array(T_shape, dtype=np.uint32))
    T_kind, T_read = np.array(T_kind), np.array(T_read)
    by_kind = [int(((T_kind == k) & (took == 3)).sum()) for k in range(3)]
    assert min(by_kind) >= 1, ("sibling ties, genus ties, ties with a stranger taken by the form", by_kind, np.bincount(T_kind, minlength=3))
    tk = took == 3
    assert np.array_equal(rec["call_tid"][tk], a["call_tid"][T_read[tk]]) and np.array_equal(rec["match_type"][tk], a["match_type"][T_read[tk]])
    reads.free()
    eng.close()


if __name__ == "__main__":   # the child: the same reads with whatever LMAT_K4_TIE says, pickled
    sys.path.insert(0, ROOT)
    _eng, _reads, _out, _ = _run(sys.argv[1])
    _reads.free()
    _eng.close()
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_out, _f)
