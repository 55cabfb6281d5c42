"""The closure walked at a fixed stride (kernels.hip classify_one), checked on the CPU: the host model of
closure_stride_cases -- item lanes by (chain in element order, path position), new slots by the rank among the registering lanes, the
ancestor mask of an eligible id as the OR of its chain's slots -- against the CPU oracle's closure
(registration order and per-id position counts of retrieve_kmer_labels, Oracle.rkmer_trace), on the designed reads the GPU test
classifies and on random small taxonomies whose lists carry inner nodes, kept ids above other kept ids and chains that share
ancestors.  The general steps' model (dense item list, Euler intervals) is held against the same traces."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import capacity_probes as cp  # noqa: E402
import closure_stride_cases as cs  # noqa: E402


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def _traces(ps):
    import oracle_py
    orc = oracle_py.Oracle(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    orc.add_taxhisto(ps["db"])
    orc.set_options()
    try:
        lines = orc.rkmer_trace(*_blob([p.read for p in ps["probes"]]), cp.K).split("\n")[:-1]
    finally:
        orc.close()
    assert len(lines) == len(ps["probes"])
    return lines


def test_designed_reads_against_the_oracle(tmp_path):
    ps = cs.build_set(str(tmp_path))
    lines = _traces(ps)
    seen = {True: 0, False: 0}
    for p, line in zip(ps["probes"], lines):
        taken, ends = cs.EXPECT[p.name]
        m = cs.check_against_trace(ps["tax"], p, line)
        assert m["taken"] == taken, (p.name, m)
        assert m["overflow"] == (ends != "fast"), (p.name, m)
        g = cs.check_against_trace(ps["tax"], p, line, stride=False)
        assert not g["taken"] and g["overflow"] == m["overflow"]
        seen[taken] += 1
    assert seen[True] >= 15 and seen[False] >= 8
    by = {p.name: p for p in ps["probes"]}
    assert (by["nel64"].E, by["nel65"].E, by["T64"].T, by["T65"].T) == (64, 65, 64, 65)
    assert by["lad32x2"].T > 32 and by["lad7_fam"].T > 32


def _random_tax(rng, n_nodes, max_depth):
    """A random tree with ids in no order of depth; leaves are strains (most of them), their parents species (most of them), the
    rest has no rank, so lists can carry inner nodes and strains without a species."""
    from lmat_amd import synth
    tax = synth.Taxonomy()
    tax.add(1, 1, "no_rank", "root")
    ids = [int(x) for x in rng.permutation(np.arange(2, 2 + 3 * n_nodes))[:n_nodes]]
    nodes = [1]
    for tid in ids:
        while True:
            par = nodes[int(rng.integers(0, len(nodes)))]
            if tax.depth[par] < max_depth:
                break
        tax.add(tid, par, "no_rank", "n%d" % tid)
        nodes.append(tid)
    for t in tax.ids:
        if t != 1 and not tax.children[t] and rng.random() < 0.7:
            tax.rank[t] = "strain"
    for t in tax.ids:
        if t != 1 and tax.children[t] and all(not tax.children[c] for c in tax.children[t]) and rng.random() < 0.8:
            tax.rank[t] = "species"
    return cs.renumber16(tax)


def test_random_small_taxonomies_against_the_oracle(tmp_path):
    import oracle_py
    from lmat_amd import synth
    taken = fallback = above = shared = 0
    for ti, (n_nodes, max_depth) in enumerate(((60, 6), (90, 12), (70, 30))):
        rng = np.random.default_rng(100 + ti)
        tax = _random_tax(rng, n_nodes, max_depth)
        d = str(tmp_path / ("t%d" % ti))
        paths = synth.write_aux_files(d, tax)
        orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], paths["idmap"])
        b = cp._Builder(tax, orc, False, 200 + ti)
        try:
            pool = [t for t in tax.ids if t != 1]
            for r in range(60):
                lists = []
                for _ in range(int(rng.integers(1, 5))):
                    l = []
                    for t in rng.permutation(pool)[:int(rng.integers(1, 5))].tolist():
                        if not any(t in tax.path(u) or u in tax.path(t) for u in l):
                            l.append(t)
                    if sorted(l) not in [sorted(x) for x in lists]:
                        lists.append(l)
                reps = [lists[int(i)] for i in rng.integers(0, len(lists), size=int(rng.integers(0, 4)))]
                b.add("r%d" % r, "stride", 0, lists + reps, positions=[int(x) for x in rng.choice(131, size=len(lists) + len(reps), replace=False)])
        finally:
            orc.close()
        kmers = np.array(sorted(b.table), dtype=np.uint64)
        paths["db"] = os.path.join(d, "random.bin")
        synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], cp.K)
        paths["probes"] = b.probes
        for p, line in zip(b.probes, _traces(paths)):
            m = cs.check_against_trace(tax, p, line)
            g = cs.check_against_trace(tax, p, line, stride=False)
            assert m["overflow"] == g["overflow"]
            taken += m["taken"] and m["nch"] >= 2
            fallback += not m["taken"] and m["nch"] >= 2
            kept = {t for l in p.lists for t in l}
            above += m["taken"] and any(a in kept for t in kept for a in tax.path(t))
            paths_ = [set(tax.path(t)) - {1} for t in kept]
            shared += m["taken"] and any(x & y for i, x in enumerate(paths_) for y in paths_[:i])
    assert taken > 60 and fallback > 5 and above > 10 and shared > 20, (taken, fallback, above, shared)
