"""GPU: the closure of a read with several eligible ids, walked at a fixed stride (kernels.hip classify_one).
Designed single reads of 150 bp (closure_stride_cases.build_set: exact lists on chosen positions of random reads) against a small
database, each the smallest shape at which the path can go wrong:

  - 2, 3, 8 and 9 walked chains at stride 8 (the last falls back to the general steps);
  - a longest chain of 1, 7, 8, 9 and 16 (stride 16), 17 and 32 (stride 32) and 33 entries (falls back), each with as many chains
    as make chains * stride exactly 64 and with one more;
  - 64 and 65 elements; a closure that brings the table to exactly 64 slots and one that passes them (handed to the E = 512 class
    and on to the middle tier, as before);
  - a kept id above another kept id; element order against slot order; a negative-first list among the others; strains of two
    species of which only the representatives walk; more than 32 slots at strides 8 and 32 (the high halves of the masks).

Every read is classified alone with candidates (-p: text and candidate count against the CPU oracle), alone and in a shuffled batch
of a few hundred without (the plain variant; records field for field against the -p launch, tallies against the oracle), and the same
again in a child process under LMAT_CLOSURE_STRIDE=0 (the general steps: byte for byte).  Launches under LMAT_CLOSURE_STRIDE=2 run
the generic kernel with the walk on and count the reads that take it: every read designed to take it must, every other must not.
-s and a taxonomy beyond 16-bit ids are controls: the same comparisons, and no read on the path."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import capacity_probes as cp
import closure_stride_cases as cs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel")
COPIES = 8   # the batch: every read this many times, shuffled


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def build_wide(outdir):
    """The control on a taxonomy beyond 16-bit ids: reads of 2, 3 and 9 chains of strains of different families."""
    import oracle_py
    from lmat_amd import synth
    tax = synth.make_taxonomy(cp.BRANCHING_WIDE, specials=False)
    paths = synth.write_aux_files(outdir, tax)
    paths["idmap"] = None
    orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], None)
    b = cp._Builder(tax, orc, True, cs.SEED + 1)
    try:
        reps = [b.strains[i * 66 * 8] for i in range(9)]
        for n in (2, 3, 9):
            b.add("wide%d" % n, "stride", 0, [reps[:n], reps[:1], reps[1:2]])
    finally:
        orc.close()
    kmers = np.array(sorted(b.table), dtype=np.uint64)
    paths["db"] = os.path.join(outdir, "wide.bin")
    synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], cp.K)
    paths.update(tax=tax, probes=b.probes)
    return paths


def _engine(ps, permissive=False):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    if permissive:
        eng.set_label_modes(True, 0, None)
    eng.build_db(ps["db"], k=cp.K)
    return eng


def _order(n):
    return np.random.default_rng(5).permutation(np.tile(np.arange(n), COPIES))


def run_all(eng, ps):
    """-> dict: text, n_cand, full (the -p launch of every read alone: its text, candidates, records), alone / batch (records of the launches without candidates), tally
    (of the batch), kernels (generic, plain launches of the launches without candidates)."""
    from lmat_amd import Params
    probes = ps["probes"]
    reads = [p.read for p in probes]
    order = _order(len(reads))
    dr = eng.upload_reads(_blob(reads))
    db = eng.upload_reads(_blob([reads[i] for i in order.tolist()]))
    out = {}
    try:
        eng.set_params(Params.run_rl(prn_all=1))
        text, n_cand, full = [], [], []
        for i in range(len(reads)):
            res, cands = eng.classify(dr, i, 1, want_cands=True, cand_cap=4200)
            full.append(res)
            text.append(eng.format_out(res, cands, _blob(reads[i:i + 1]), i))
            n_cand.append(int(res["n_cand"][0]))
        eng.set_params(Params.run_rl(prn_all=0))
        v0 = eng.variant_launches()
        out["alone"] = np.concatenate([eng.classify(dr, i, 1, want_cands=False)[0] for i in range(len(reads))])
        eng.counts_reset()
        out["batch"] = eng.classify(db, want_cands=False)[0]
        out["tally"] = eng.counts()
        v1 = eng.variant_launches()
        out.update(text=text, n_cand=n_cand, full=np.concatenate(full), kernels=(v1["generic"] - v0["generic"], v1["plain"] - v0["plain"]))
    finally:
        dr.free()
        db.free()
    return out


def taken_counts(eng, ps):
    """Every read alone under LMAT_CLOSURE_STRIDE=2 -> (reads that walked at a fixed stride per launch, records, generic launches)."""
    reads = [p.read for p in ps["probes"]]
    dr = eng.upload_reads(_blob(reads))
    assert "LMAT_CLOSURE_STRIDE" not in os.environ
    os.environ["LMAT_CLOSURE_STRIDE"] = "2"
    try:
        v0 = eng.variant_launches()
        taken, recs = [], []
        for i in range(len(reads)):
            recs.append(eng.classify(dr, i, 1, want_cands=False)[0])
            taken.append(eng.closure_stride_taken())
        v1 = eng.variant_launches()
    finally:
        del os.environ["LMAT_CLOSURE_STRIDE"]
        dr.free()
    return taken, np.concatenate(recs), (v1["generic"] - v0["generic"], v1["plain"] - v0["plain"])


def _child(builder, d, permissive):
    fn = os.path.join(d, "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), builder, d, fn, "1" if permissive else "0"],
                       env=dict(os.environ, LMAT_CLOSURE_STRIDE="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        return pickle.load(f)


def _runs(tmp_path_factory, builder, permissive=False):
    assert os.environ.get("LMAT_CLOSURE_STRIDE") is None and os.environ.get("LMAT_PLAIN") in (None, "1")
    d = str(tmp_path_factory.mktemp("closure_stride_" + builder + ("_s" if permissive else "")))
    ps = (cs.build_set if builder == "set" else build_wide)(d)
    eng = _engine(ps, permissive)
    try:
        here = run_all(eng, ps)
        taken = taken_counts(eng, ps)
    finally:
        eng.close()
    return ps, here, taken, _child(builder, d, permissive)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return _runs(tmp_path_factory, "set")


def _differing(a, b, names):
    bad = []
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        for i in np.nonzero(x.view(f"u{x.dtype.itemsize}") != y.view(f"u{y.dtype.itemsize}"))[0].tolist():
            bad.append("%s: %s %r != %r" % (names[i], f, x[i], y[i]))
    return bad


def _oracle(ps, reads, permissive=False):
    orc = cp.mode_oracle(ps, None, None, permissive, 0, None)
    try:
        return orc.classify(*_blob(reads), cp.K)
    finally:
        orc.close()


def _against_the_oracle(ps, here, permissive=False):
    probes = ps["probes"]
    reads = [p.read for p in probes]
    want = _oracle(ps, reads, permissive)[0].split("\n")[:-1]
    assert len(want) == len(reads)
    bad = ["%s %r: %s != %s" % (p.name, p.dims, g[160:420], w[160:420]) for p, g, w in zip(probes, here["text"], want) if g != w + "\n"]
    assert not bad, "\n".join(bad)
    names = [p.name for p in probes]
    order = _order(len(reads))
    # the launches without candidates: the records of the -p launch
    bad = _differing(here["alone"], here["full"], names) + _differing(here["batch"], here["full"][order], [names[i] for i in order.tolist()])
    assert not bad, "launches without candidates against the -p launch:\n" + "\n".join(bad)
    _, tally, nomatch = _oracle(ps, [reads[i] for i in order.tolist()], permissive)
    counts, nm = here["tally"]
    assert list(nm) == [int(x) for x in nomatch]
    assert {t: c for t, (c, _) in counts.items()} == {int(t): int(c) for t, (c, _) in tally.items()}
    for t, (c, s) in counts.items():
        assert abs(s - tally[t][1]) <= 1e-4 * max(1.0, abs(s))


def _against_the_child(ps, here, child):
    names = [p.name for p in ps["probes"]]
    order = _order(len(names))
    assert here["text"] == child["text"] and here["n_cand"] == child["n_cand"]
    bad = _differing(here["alone"], child["alone"], names) + _differing(here["batch"], child["batch"], [names[i] for i in order.tolist()])
    assert not bad, "\n".join(bad)
    assert here["alone"].tobytes() == child["alone"].tobytes() and here["batch"].tobytes() == child["batch"].tobytes()
    assert here["tally"] == child["tally"]


def test_every_read_against_the_oracle(runs):
    ps, here, _, _ = runs
    _against_the_oracle(ps, here)
    by = {p.name: i for i, p in enumerate(ps["probes"])}
    for name in cs.EXPECT:   # as many candidates as the read registers, the closure's new slots included (the negative-first read: one strain is walked nowhere)
        p = ps["probes"][by[name]]
        assert here["n_cand"][by[name]] == p.T - (1 if hasattr(p, "neg") else 0), name
    assert set(by) == set(cs.EXPECT)


def test_against_the_general_steps(runs):
    """LMAT_CLOSURE_STRIDE=0 in a child process: every record, candidate text and tally byte for byte; that arm ran the generic kernel."""
    ps, here, _, child = runs
    _against_the_child(ps, here, child)
    n = len(ps["probes"])
    assert here["kernels"][0] == 0 and here["kernels"][1] >= n + 1     # the plain variant here (the walk compiled in) ...
    assert child["kernels"][1] == 0 and child["kernels"][0] >= n + 1   # ... the generic kernel without it in the child


def test_the_walk_is_taken_where_it_must_be_and_nowhere_else(runs):
    ps, here, (taken, recs, kernels), _ = runs
    names = [p.name for p in ps["probes"]]
    assert kernels[1] == 0 and kernels[0] >= len(names)
    bad = []
    for name, n in zip(names, taken):
        want, ends = cs.EXPECT[name]
        if want and not (n >= 1 if ends == "fast" else n == 2):   # (a read that passes 64 slots walks again in the E = 512 class)
            bad.append("%s: designed for the walk, %d reads took it" % (name, n))
        if not want and n != 0:
            bad.append("%s: designed for the general steps, %d reads took the walk" % (name, n))
    assert not bad, "\n".join(bad)
    assert sum(1 for n in names if cs.EXPECT[n][0]) >= 20
    assert not _differing(recs, here["alone"], names)


def test_the_read_past_64_slots_goes_where_it_went(runs):
    """T65: the walk's overflow exit hands the read to the E = 512 class and that one to the middle tier, as the general steps do."""
    from lmat_amd import Params
    ps = runs[0]
    i = [p.name for p in ps["probes"]].index("T65")
    eng = _engine(ps)
    try:
        dr = eng.upload_reads(_blob([p.read for p in ps["probes"]]))
        eng.classify(dr, i, 1, want_cands=False)
        c = eng.last_counters()
        eng.classify(dr, i - 1, 1, want_cands=False)
        c64 = eng.last_counters()
        dr.free()
    finally:
        eng.close()
    assert (c["past_fast"], c["past_e512"], c["past_middle"]) == (1, 1, 0)
    assert ps["probes"][i - 1].name == "T64" and (c64["past_fast"], c64["past_e512"]) == (0, 0)


@pytest.mark.parametrize("control", ["permissive", "wide"])
def test_untouched_controls(tmp_path_factory, control):
    """-s (no closure at all) and the WIDE classes (their own closure): oracle, general-steps child, and nobody on the walk."""
    ps, here, (taken, recs, kernels), child = _runs(tmp_path_factory, "wide" if control == "wide" else "set", control == "permissive")
    _against_the_oracle(ps, here, control == "permissive")
    _against_the_child(ps, here, child)
    assert taken == [0] * len(ps["probes"])
    assert not _differing(recs, here["alone"], [p.name for p in ps["probes"]])


if __name__ == "__main__":   # the child of _runs: run_all with whatever LMAT_CLOSURE_STRIDE says, pickled
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _d = os.path.join(sys.argv[2], "child")
    os.makedirs(_d)
    _ps = (cs.build_set if sys.argv[1] == "set" else build_wide)(_d)
    _e = _engine(_ps, sys.argv[4] == "1")
    _out = run_all(_e, _ps)
    _e.close()
    with open(sys.argv[3], "wb") as _f:
        pickle.dump(_out, _f)
