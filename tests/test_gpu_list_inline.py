"""GPU: K3b stage 1 of the classes that stage their list records (kernels.hip, classify_one): a staged list of up to three kept ids
is completed there -- ids of both orders and the owners of its elements --, longer lists and lists beyond the 40-list window wait for
stage 2 and the running maximum, and one scan carries both sums of the stage.  Single 150 bp reads against a database of designed
lists (capacity_probes' builder: exact T, E and D), each checked against the CPU oracle:

  - one length of list at a time: 1 .. 8, 14 and 15 kept ids (3 is the bound, 14 the last length whose record is staged whole);
  - the edge of the staged window: three-id lists as the 38th .. 40th, the 39th .. 41st and the 41st .. 43rd distinct list of a read;
  - lists inside and beyond the bound mixed, so that owners written directly stand beside those the running maximum spreads;
  - E - 1, E and E + 1 elements for E = 256 (63 or 64 lists of three and four ids; E + 1 takes one list of five: 64 lists of at most
    four ids end at 256) and for E = 512 (20 lists of three, 20 of four and 23 long ones: 64 lists of at most four ids cannot get
    there), the reads of 257 .. 512 elements being handed to the E = 512 class, the one of 513 beyond it.

The negative-first flag needs a raw list of 32768 ids or more; a tree that lists that many and still leaves the read in a fast class
was not to be had in a few seconds, so that arm (the flag's positions summed on their own) stays with the existing parity tests.

Each read goes through the -p launch (the generic kernel: text and candidate count against the oracle), through the launch without
candidates alone and as a batch (the fixed-geometry plain variant), and through the same two in a child process with LMAT_PLAIN=0."""
import itertools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import capacity_probes as cp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7301
FIELDS = ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel")


def _subsets(pool, n, used):
    """Subsets of `pool` with n members, in a fixed order, none handed out twice."""
    for c in itertools.combinations(pool, n):
        if c not in used:
            used.add(c)
            yield list(c)


def _take(pool, sizes, used):
    gens = {}
    out = []
    for n in sizes:
        gens.setdefault(n, _subsets(pool, n, used))
        out.append(next(gens[n]))
    return out


def build_set(outdir):
    import oracle_py
    from lmat_amd import synth
    tax = synth.make_taxonomy(cp.BRANCHING16, specials=False)
    paths = synth.write_aux_files(outdir, tax)
    orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], paths["idmap"])
    b = cp._Builder(tax, orc, False, SEED)
    pool, pool24 = b.strains[:20], b.strains[:24]
    try:
        for n in (1, 2, 3, 4, 5, 6, 7, 8, 14, 15):   # two lists of n ids, the first on five positions
            first, second = _take(pool, (n, n), set())
            b.add("len%d" % n, "E", 0, [first, second, first, first, first, first], positions=[0, 20, 40, 64, 100, 130])
        for at in (37, 38, 40):                       # three-id lists as distinct lists at .. at + 2 (counted from 0), ones and twos around them
            used = set()
            sizes = [1 + i % 2 for i in range(at)] + [3, 3, 3] + [2, 1, 2][:45 - at - 3]
            p = b.add("window%d" % at, "D", 40, _take(pool24, sizes, used))
            assert p.D == len(sizes) and p.E == sum(sizes)
        sizes = (3, 8, 2, 5, 1, 15, 4, 3, 14, 3, 1, 6, 2, 3)
        b.add("mixed", "E", 0, _take(pool, sizes, set()))
        b.add("mixed_rev", "E", 0, _take(pool, sizes[::-1], set()))
        for E in (255, 256, 257):
            sizes = {255: [4, 3] + [4] * 62, 256: [4] * 64, 257: [4] * 31 + [5] + [4] * 32}[E]
            p = b.add("E%d" % E, "E", 256, _take(pool, sizes, set()))
            assert p.E == E and p.D == 64 and p.T <= 40, p.dims
        for E in (511, 512, 513):
            used = set()
            short = _take(pool24, [3, 4] * 20, used)
            longs = [[pool24[(i + j) % 24] for j in range(16)] for i in range(22)] + [pool24[:E - 140 - 352]]
            lists = [x for pair in itertools.zip_longest(short, longs) for x in pair if x is not None]   # short and long lists in turn: long ones inside and beyond the window
            p = b.add("E%d" % E, "E", 512, lists)
            assert p.E == E and p.D == 63 and p.T <= 40, p.dims
    finally:
        orc.close()
    kmers = np.array(sorted(b.table), dtype=np.uint64)
    paths["db"] = os.path.join(outdir, "lists.bin")
    synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], cp.K)
    paths.update(tax=tax, probes=b.probes)
    return paths


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def _engine(ps):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    eng.build_db(ps["db"], k=cp.K)
    return eng


def _no_cands(eng, ps):
    """The launches without a candidate buffer: the batch, then every probe alone -> (batch records, single records, kernels run)."""
    probes = ps["probes"]
    dr = eng.upload_reads(_blob([p.read for p in probes]))
    v0, u0 = eng.variant_launches(), eng.uniform_launches()
    batch, _ = eng.classify(dr, 0, len(probes), want_cands=False)
    alone = np.concatenate([eng.classify(dr, i, 1, want_cands=False)[0] for i in range(len(probes))])
    v1, u1 = eng.variant_launches(), eng.uniform_launches()
    dr.free()
    return batch, alone, (v1["generic"] - v0["generic"], v1["plain"] - v0["plain"], u1 - u0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert os.environ.get("LMAT_PLAIN") in (None, "1"), "this module compares the default with LMAT_PLAIN=0 itself"
    d = str(tmp_path_factory.mktemp("list_inline"))
    ps = build_set(d)
    eng = _engine(ps)
    here = _no_cands(eng, ps)
    fn = os.path.join(d, "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), d, fn], env=dict(os.environ, LMAT_PLAIN="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    yield ps, eng, here, child
    eng.close()


def _differing(a, b, names):
    bad = []
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        for i in np.nonzero(x.view(f"u{x.dtype.itemsize}") != y.view(f"u{y.dtype.itemsize}"))[0].tolist():
            bad.append("%s: %s %r != %r" % (names[i], f, x[i], y[i]))
    return bad


def test_the_probes_are_what_they_were_designed_to_be(runs):
    ps = runs[0]
    by = {p.name: p for p in ps["probes"]}
    assert [by["len%d" % n].E for n in (1, 2, 3, 4, 5, 6, 7, 8, 14, 15)] == [2, 4, 6, 8, 10, 12, 14, 16, 28, 30]
    assert [by[n].expected for n in ("E255", "E256", "E257", "E511", "E512", "E513")] == ["fast", "fast", "e512", "e512", "e512", "middle"]
    assert all(p.expected == "fast" for n, p in by.items() if not n.startswith("E")) and all(len(p.read) == 150 for p in by.values())
    assert by["window38"].lists[37:42] and [len(l) for l in by["window38"].lists[36:43]] == [1, 2, 3, 3, 3, 2, 1]


def test_each_read_against_the_oracle(runs):
    """The -p launch of every read alone: record and candidates as the oracle prints them, as many candidates as the read registers."""
    import ctypes as C
    import oracle_py
    from lmat_amd import Params
    from lmat_amd.capi import CAND_DTYPE, READ_RESULT_DTYPE
    ps, eng, here, _ = runs
    probes = ps["probes"]
    orc = oracle_py.Oracle(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    orc.add_taxhisto(ps["db"])
    orc.set_options()
    eng.set_params(Params.run_rl(prn_all=1))
    dr = eng.upload_reads(_blob([p.read for p in probes]))
    bad, full = [], np.zeros(len(probes), dtype=READ_RESULT_DTYPE)
    try:
        for i, p in enumerate(probes):
            want = orc.classify(*_blob([p.read]), cp.K, i)[0]
            res, cands, n = np.zeros(1, dtype=READ_RESULT_DTYPE), np.zeros(4200, dtype=CAND_DTYPE), C.c_uint64(0)
            eng._chk(eng.lib.lmat_classify(eng.ctx, dr.h, i, 1, res.ctypes.data_as(C.c_void_p), cands.ctypes.data_as(C.c_void_p), 4200, C.byref(n)))
            full[i] = res[0]
            got = eng.format_out(res, cands, _blob([p.read]), i)
            if got != want:
                bad.append("%s %r: %s != %s" % (p.name, p.dims, got[160:400], want[160:400]))
            elif not int(n.value) == int(res["n_cand"][0]) == p.T:
                bad.append("%s %r: %d candidates written, n_cand %d" % (p.name, p.dims, n.value, res["n_cand"][0]))
    finally:
        dr.free()
        orc.close()
        eng.set_params(Params.run_rl(prn_all=0))
    assert not bad, "\n".join(bad)
    names = [p.name for p in probes]
    bad = _differing(here[0], full, names) + _differing(here[1], full, names)
    assert not bad, "launches without candidates against the -p launch:\n" + "\n".join(bad)


def test_plain_variant_against_the_generic_kernel(runs):
    ps, _, here, child = runs
    n = len(ps["probes"])
    assert here[2][0] == 0 and here[2][1] == here[2][2] >= n + 1   # every launch here ran the fixed-geometry plain variant ...
    assert child[2][0] >= n + 1 and child[2][1:] == (0, 0)         # ... and the generic kernel in the child
    names = [p.name for p in ps["probes"]]
    bad = _differing(here[0], child[0], names) + _differing(here[1], child[1], names) + _differing(here[0], here[1], names)
    assert not bad, "\n".join(bad)
    assert here[0].tobytes() == child[0].tobytes()


if __name__ == "__main__":   # the child of the `runs` fixture: the launches without candidates with whatever LMAT_PLAIN says, pickled
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _d = os.path.join(sys.argv[1], "child")
    os.makedirs(_d)
    _ps = build_set(_d)
    _e = _engine(_ps)
    _out = _no_cands(_e, _ps)
    _e.close()
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_out, _f)
