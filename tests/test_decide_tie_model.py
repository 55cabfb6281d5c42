"""The derivation behind the closed form for tied ids at the top (kernels.hip k4_wave_tie), checked on the CPU: the host model of the
form (decide_tie_tables.model) against the oracle's findReadLabelVer2 (oracle/lmat_oracle.hpp find_read_label, the restatement of
read_label.cpp:284-419) on the tables test_gpu_decide_tie.py runs on the GPU.  Wherever the model says "taken" -- the entry
conditions hold and no close id's walk would end the scan part-way -- its call, score and match type are the oracle's, and they stay
the oracle's when the slots are put in another order: the call does not depend on which tied id std::sort leaves first."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import decide_tie_tables as dt  # noqa: E402
from test_decide_path_model import forest  # noqa: E402
from test_gpu_decide_chain import BENCH, SMALL, _Pool, _pool_bench  # noqa: E402

SDIFFS = (0.0, 0.5, 1.0, 3.0, 1e6)


def _oracle(tmp, tax):
    import oracle_py
    from lmat_amd import synth
    p = synth.write_aux_files(str(tmp), tax)
    return oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])


def _against_oracle(orc, t, m, what, kinds):
    """every taken table of t: the oracle's call on the table as it stands is the model's"""
    pool = t.pool
    checked = 0
    for i in np.nonzero(m["in_shape"] & ~m["partway"])[0]:
        ix, cn, kept = t.rows[i]
        nT = len(ix)
        call, score, match = orc.replay_decision(pool.tids[ix], m["sc"][i, :nT], m["stdev"][i])
        want_tid = int(pool.tids[m["call"][i]]) if m["call"][i] >= 0 else 0
        assert (call, match) == (want_tid, int(m["match"][i])), (what, i, pool.tids[ix], cn, kept, call, match, want_tid, m["match"][i])
        if match != 4:   # (the reference leaves -1 behind an LCA error; the kernels write 0)
            assert np.float32(score) == m["score"][i], (what, i, score, m["score"][i])
        kinds[match] += 1
        checked += 1
    return checked


def test_model_of_the_tie_form_is_find_read_label(tmp_path):
    """Every family that must be taken -- two tied children of a root (nT = 3), 2 and 3 tied siblings with and without a lower one, a
    genus block (12 strains, 4 species, more than 16 slots in the benchmark's taxonomy), the same with a stranger that lifts the shared
    ancestors above c0, nT = 64 -- is taken, none declined; cand in {1, 30, 131, 999}, sdiff in {0, 0.5, 1, 3, 1e6}; Multi at several
    depths and the LCA error both occur.  Tables with two strangers: taken unless part-way."""
    from lmat_amd import synth
    kinds = np.zeros(5, dtype=np.int64)
    call_depths = set()
    checked = partway = gt = 0
    seen_cand = set()
    for bi, (tax, mkpool) in enumerate(((forest(SMALL), lambda tx: _Pool(tx, list(tx.ids))),
                                        (synth.make_taxonomy(BENCH, specials=False), _pool_bench))):
        pool = mkpool(tax)
        orc = _oracle(tmp_path / f"aux{bi}", tax)
        for si, sdiff in enumerate(SDIFFS):
            orc.set_options(sdiff=sdiff)
            for fi, fam in enumerate(dt.TAKEN + ("two",)):
                if fam in ("wide", "sib3low") and bi == 0:   # (the small taxonomy has neither 64 free nodes nor four siblings)
                    continue
                t = dt.build(pool, 40, 1000 * bi + 100 * si + fi, fam)
                m = dt.model(t, sdiff)
                assert m["in_shape"].all(), (fam, sdiff, np.nonzero(~m["in_shape"])[0][:5])
                if fam != "two":
                    assert not m["partway"].any(), (fam, sdiff)
                if fam == "genus" and bi == 1:
                    assert (t.nT > 16).all() and (m["ntop"] == 12).all()
                if fam == "wide":
                    assert (t.nT == 64).all()
                if fam == "root2":
                    assert (t.nT == 3).all()
                partway += int(m["partway"].sum())
                gt += int(m["gt"].sum())
                seen_cand |= set(t.cand.tolist())
                checked += _against_oracle(orc, t, m, (fam, sdiff), kinds)
                tk = m["in_shape"] & ~m["partway"] & (m["match"] == 1)
                call_depths |= set(pool.depth[m["call"][tk]].tolist())
                # the same tables with their slots in another order: another tied id comes first, the call stays
                t2 = t.permuted(7 + fi)
                m2 = dt.model(t2, sdiff)
                assert np.array_equal(m2["in_shape"], m["in_shape"]) and np.array_equal(m2["partway"], m["partway"])
                both = m["in_shape"] & ~m["partway"]
                assert np.array_equal(m2["call"][both], m["call"][both]) and np.array_equal(m2["match"][both], m["match"][both])
                _against_oracle(orc, t2, m2, (fam, sdiff, "permuted"), np.zeros(5, dtype=np.int64))
        orc.close()
    assert checked > 2500 and partway > 10 and gt > 300, (checked, partway, gt)
    assert kinds[0] == 0 and kinds[1] > 1500 and kinds[4] > 5 and kinds[2] == 0, kinds   # never Direct, never Partial
    assert len(call_depths) >= 4, call_depths
    assert seen_cand == {1, 30, 131, 999}


def test_one_broken_condition_each_declines():
    """One family per broken condition: the model declines every table of it."""
    from lmat_amd import synth
    tax = synth.make_taxonomy(BENCH, specials=False)
    pool = _pool_bench(tax)
    for fi, fam in enumerate(dt.BROKEN):
        t = dt.build(pool, 60, 500 + fi, fam)
        m = dt.model(t, 1.0)
        assert not m["in_shape"].any(), (fam, np.nonzero(m["in_shape"])[0][:5])
    # a negative threshold: a tied id's difference of 0 would not mark
    t = dt.build(pool, 20, 77, "sib2")
    assert not dt.model(t, -1.0)["in_shape"][dt.model(t, 1.0)["stdev"] > 0].any()
