"""The derivation behind the closed form for one dominant lineage (kernels.hip k4_wave_path), checked on the CPU: the host model of
the form (decide_path_tables.model) against the oracle's findReadLabelVer2 (oracle/lmat_oracle.hpp find_read_label, the restatement
of read_label.cpp:284-419) on a sample of the tables test_gpu_decide_path.py runs on the GPU.  Wherever the model says "taken"
-- the entry conditions hold and no close id's walk would end the scan part-way -- its call, score and match type are the oracle's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import decide_path_tables as dp  # noqa: E402
from test_gpu_decide_chain import SMALL, _Pool  # noqa: E402


def forest(branching=SMALL):
    """The small taxonomy plus a second tree of three nodes (its root at depth 0): ids with no common ancestor."""
    from lmat_amd import synth
    tax = synth.make_taxonomy(branching, specials=False)
    nxt = max(tax.id16.values()) + 1
    for tid, par in ((990001, 990001), (990002, 990001), (990003, 990002), (990004, 990002)):
        tax.add(tid, par, "no_rank", f"other_tree_{tid}")
        tax.id16[tid] = nxt
        nxt += 1
    return tax


def test_model_of_the_closed_form_is_find_read_label(tmp_path):
    import oracle_py
    from lmat_amd import synth
    tax = forest()
    p = synth.write_aux_files(str(tmp_path / "aux"), tax)
    pool = _Pool(tax, list(tax.ids))
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    kinds = np.zeros(5, dtype=np.int64)
    checked = partway = 0
    for si, sdiff in enumerate((0.0, 0.5, 1.0, 3.0, 1e6)):
        orc.set_options(sdiff=sdiff)
        for fi, fam in enumerate(("sib", "stranger", "two", "genus", "wide", "pair")):
            t = dp.build(pool, 120, 100 * si + fi, fam, extras=bool((si + fi) & 1) or fam in ("stranger", "two"))
            m = dp.model(t, sdiff)
            assert m["in_shape"].all(), (fam, sdiff)
            partway += int(m["partway"].sum())
            for i in np.nonzero(~m["partway"])[0]:
                nT = int(t.nT[i])
                tids = pool.tids[t.ix[i, :nT]]
                call, score, match = orc.replay_decision(tids, m["sc"][i, :nT], m["stdev"][i])
                want_tid = int(pool.tids[m["call"][i]]) if m["call"][i] >= 0 else 0
                assert (call, match) == (want_tid, int(m["match"][i])), (fam, sdiff, i, tids, t.cn[i, :nT], call, match, want_tid, m["match"][i])
                if match != 4:   # (the reference leaves -1 behind an LCA error; the kernels write 0)
                    assert np.float32(score) == m["score"][i], (fam, sdiff, i, score, m["score"][i])
                kinds[match] += 1
                checked += 1
    orc.close()
    assert checked > 3000 and partway > 50, (checked, partway)
    assert kinds[0] > 500 and kinds[1] > 500 and kinds[4] > 20, kinds
