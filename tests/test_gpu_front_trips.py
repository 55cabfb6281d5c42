"""The front end of the read loop of the headline class (classify_kernel's FRONT, classify_one's TAIL_EARLY, kernels.hip): the next
record is asked for on every trip with its index clamped to the launch's last read, the first record is waited for before the loop,
and the plain variants ask for a read's tail entries with its record.  No lookup moves and no data changes, so every record and
tally must be what it was: the CPU oracle's, and byte for byte those of the generic kernel (LMAT_PLAIN=0) and of a run without
tails (LMAT_TAIL=0).

A wave takes every G-th read of a launch, G being the launch's grid (Engine.classify_grid), and the grid of a default run is far
larger than a test's launch: every wave would make one trip.  The launches under test therefore run in child processes whose
LMAT_GRID_MULT (read once per process) brings G down to 8192; this process holds the oracle, which takes every read of a set once.

A batch of 150-bp reads with one read of 149 bp is still a launch of one geometry (148 .. 151 bases): it runs as UNI.  The batch
with one read of 147 bp is the one that leaves UNI for PLAIN.  Both are here."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BR = (3, 4, 4, 4, 4, 3)
SMALL_TABLE = 4 << 20
NB = 16400                      # reads of the base set: at least 2 G + 1
SMALL_GRID = {"LMAT_GRID_MULT": "1"}   # 32 workgroups a CU instead of 32 x 32: G = 8192
ARMS = {"default": {}, "generic": {"LMAT_PLAIN": "0"}, "no-tail": {"LMAT_TAIL": "0"}}
SIZES = ("1", "2", "G-1", "G", "G+1", "2G-1", "2G", "2G+1")
VARIANTS = ("one149", "one147", "le147", "mixed_uni", "mixed_plain", "exits_uni", "exits_plain")
UNI = {"generic": 0, "plain": 1, "uniform": 1}
PLAIN = {"generic": 0, "plain": 1, "uniform": 0}
GENERIC = {"generic": 1, "plain": 0, "uniform": 0}
RAN = {"one149": UNI, "one147": PLAIN, "le147": GENERIC, "mixed_uni": UNI, "mixed_plain": PLAIN, "exits_uni": UNI, "exits_plain": PLAIN}


def _engine():
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy(BR)
    eng.synth_db(3000, k=20, seed=2002, table_bytes=SMALL_TABLE)
    return eng


def _base(eng):
    """NB synthetic reads of 151 bases as byte strings: the same in every process."""
    synth = eng.synth_reads(NB, (151,), seed=4004)
    blob, off = synth.ascii(0, NB)
    synth.free()
    return [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(NB)]


def _with_ns(r, start, step, end=None):
    q = bytearray(r)
    for p in range(start, len(q) if end is None else end, step):
        q[p] = ord("N")
    return bytes(q)


def _none_valid(r, i):   # an N every 15 .. 19 bases: no valid window at all
    return _with_ns(r, i % 15, 15 + i % 5)


def _few_valid(r, i):    # ... up to base 125: a few valid windows, all at the end (fewer than min_kmer)
    return _with_ns(r, 12 + i % 3, 15 + i % 5, 125)


def _reads(base, key, G):
    """The read set of a case.  Every variant set has G + 101 reads: 101 waves make two trips, the others one."""
    if key == "uni150":
        return [r[:150] for r in base]
    b = base[:G + 101]
    n = len(b)
    if key == "one149":
        return [r[:149 if i == n - 7 else 150] for i, r in enumerate(b)]
    if key == "one147":
        return [r[:147 if i == 5 else 150] for i, r in enumerate(b)]
    if key == "le147":        # at most 128 k-mer positions: no tail; one chunk, two chunks, and the bounds of either
        ls = (147, 146, 140, 100, 84, 83, 64, 50, 147)
        return [r[:ls[i % len(ls)]] for i, r in enumerate(b)]
    if key == "mixed_uni":    # 129 .. 132 positions: tails of one to four
        return [r[:148 + (i + i // 7) % 4] for i, r in enumerate(b)]
    if key == "mixed_plain":  # ... and reads without a tail between them: only some reads of a wave ask for tail entries
        ls = (150, 148, 147, 151, 149, 120, 150, 64, 148)
        return [r[:ls[i % len(ls)]] for i, r in enumerate(b)]
    if key == "exits_uni":    # full length with fewer valid k-mers than min_kmer, or none: the exit behind the tail loads
        return [(_none_valid, _few_valid, lambda r, i: r)[i % 3](r[:150], i) for i, r in enumerate(b)]
    if key == "exits_plain":  # ... and reads shorter than k among them (the exit in front of the tail loads), one the launch's last read
        out = [(_none_valid, _few_valid, lambda r, i: r, lambda r, i: r)[i % 4](r[:150], i) for i, r in enumerate(b)]
        for i in (0, 3, G - 1, G, n - 1):
            out[i] = out[i][:11 + i % 8]
        return out
    raise KeyError(key)


def _cases(G):
    """name -> (read set, first, count)"""
    n_of = {"1": 1, "2": 2, "G-1": G - 1, "G": G, "G+1": G + 1, "2G-1": 2 * G - 1, "2G": 2 * G, "2G+1": 2 * G + 1}
    out = {"n=" + s: ("uni150", 0, n_of[s]) for s in SIZES}
    out["buffer_end"] = ("uni150", G + 3, NB - (G + 3))   # the second launch of the set: first != 0, ends at the last record of the words buffer
    for v in VARIANTS:
        out[v] = (v, 0, G + 101)
    return out


def _ascii(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8), off


def _launch(eng, reads, first, n, want_cands=False):
    before, ub = eng.variant_launches(), eng.uniform_launches()
    res, cands = eng.classify(reads, first, n, want_cands=want_cands, cand_cap=64 * n if want_cands else None)
    after = eng.variant_launches()
    ran = {v: after[v] - before[v] for v in after}
    ran["uniform"] = eng.uniform_launches() - ub
    return res, cands, ran


def _tallies(eng):
    counts, nomatch = eng.counts()
    tid = np.array(sorted(counts), dtype=np.uint32)
    return {"tally_tid": tid, "tally_count": np.array([counts[t][0] for t in tid.tolist()], dtype=np.uint64),
            "tally_score": np.array([counts[t][1] for t in tid.tolist()], dtype=np.float64),
            "tally_nomatch": np.array(nomatch, dtype=np.uint64)}


def _child_main(fn):
    """Every case as the default launch (records, tallies, the kernel that ran, its grid) and as the -p launch (the .out text)."""
    from lmat_amd import Params
    eng = _engine()
    base = _base(eng)
    whole = eng.upload_reads(_reads(base, "uni150", 0))
    _launch(eng, whole, 0, NB)
    G = eng.classify_grid()
    out = {"G": G, "cases": {}}
    if 2 * G + 1 <= NB:
        sets = {"uni150": whole}
        for name, (key, first, n) in _cases(G).items():
            if key not in sets:
                sets[key] = eng.upload_reads(_reads(base, key, G))
            eng.set_params(Params.run_rl(prn_all=0))
            eng.counts_reset()
            res, _, ran = _launch(eng, sets[key], first, n)
            grid = eng.classify_grid()
            c = dict(_tallies(eng), res=res, ran=ran, grid=grid)
            eng.set_params(Params.run_rl(prn_all=1))
            eng.counts_reset()
            full, cands, ranp = _launch(eng, sets[key], first, n, want_cands=True)
            c.update(full=full, ranp=ranp, text=eng.format_out(full, cands, _ascii(_reads(base, key, G)[first:first + n])))
            out["cases"][name] = c
        for r in sets.values():
            r.free()
    eng.close()
    with open(fn, "wb") as f:
        pickle.dump(out, f)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """The three child runs, side by side."""
    d = tmp_path_factory.mktemp("front_trips")
    for v in ("LMAT_PLAIN", "LMAT_TAIL", "LMAT_UNIFORM"):
        assert os.environ.get(v) in (None, "1"), v
    procs, out = {}, {}
    try:
        for arm, env in ARMS.items():
            procs[arm] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / (arm + ".pkl"))],
                                          env=dict(os.environ, **SMALL_GRID, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for arm, p in procs.items():
            log = p.communicate(timeout=600)[0]
            assert p.returncode == 0, (arm, log[-4000:])
            with open(str(d / (arm + ".pkl")), "rb") as f:
                out[arm] = pickle.load(f)
    finally:   # a child that hangs or fails leaves none of the three behind
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    G = out["default"]["G"]
    assert all(o["G"] == G for o in out.values()), [o["G"] for o in out.values()]
    assert 2 <= G and 2 * G + 1 <= NB, f"the grid of the child runs is {G}: the base set of {NB} reads does not hold 2 G + 1"
    return out


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """The CPU oracle over the synthetic database's lists, the base reads, and the k-mers it has been given so far."""
    from lmat_amd import synth
    import oracle_py
    eng = _engine()
    base = _base(eng)
    p = synth.write_aux_files(str(tmp_path_factory.mktemp("aux")), synth.make_taxonomy(BR, specials=False))
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.set_k(20)
    orc.set_options()
    state = {"eng": eng, "orc": orc, "base": base, "known": np.zeros(0, dtype=np.uint64), "sets": {}}
    yield state
    orc.close()
    eng.close()


def _oracle_run(o, key, G, first, n):
    """-> (.out text, tallies, no-match counts) of reads [first, first + n) of a read set"""
    if key not in o["sets"]:
        seqs = _reads(o["base"], key, G)
        kms = np.unique(np.concatenate([o["orc"].extract(s, 20)[0] for s in set(seqs)] + [np.zeros(0, dtype=np.uint64)]))
        new = np.setdiff1d(kms, o["known"])
        if new.size:
            counts, tids = o["eng"].lookup(new, stride=32)
            o["orc"].add_lists32(new, counts, tids)
            o["known"] = np.union1d(o["known"], new)
        o["sets"][key] = seqs
    seqs = o["sets"][key]
    if key != "uni150" or first != 0:
        blob0, off = _ascii(seqs[first:first + n])
        return o["orc"].classify(blob0, off, 20)
    # the launches of the set's first n reads: the oracle takes every read once, in the stretches between one size and the next,
    # and a launch's expected text and tallies are those of the stretches it covers (tallies are counts: they add)
    if "prefix" not in o:
        text, tally, nomatch, lo, o["prefix"] = "", {}, [0, 0, 0], 0, {}
        for hi in sorted({c[2] for name, c in _cases(G).items() if name.startswith("n=")}):
            blob0, off = _ascii(seqs[lo:hi])
            t, tl, nm = o["orc"].classify(blob0, off, 20, first_index=lo)
            text += t
            for tid, (c, s) in tl.items():
                tally[tid] = (tally.get(tid, (0, 0.0))[0] + c, 0.0)
            nomatch = [a + b for a, b in zip(nomatch, nm)]
            o["prefix"][hi] = (text, dict(tally), list(nomatch))
            lo = hi
    return o["prefix"][n]


def _bits(x):
    return np.ascontiguousarray(x).view(f"u{x.dtype.itemsize}")


def _same_records(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    for f in a.dtype.names:
        bad = np.nonzero(_bits(a[f]) != _bits(b[f]))[0]
        assert bad.size == 0, f"{what}: field {f} differs in {bad.size} records, first {int(bad[0])}: {a[f][bad[0]]} != {b[f][bad[0]]}"
    assert a.tobytes() == b.tobytes(), what


def _check(arms, oracle, name, want_ran, want_grid=None):
    G = arms["default"]["G"]
    key, first, n = _cases(G)[name]
    here = arms["default"]["cases"][name]
    assert here["ran"] == want_ran, (name, here["ran"])
    assert here["ranp"] == GENERIC, (name, here["ranp"])   # candidates keep both variants off: the -p launch is the generic kernel's
    assert here["res"].shape[0] == n
    if want_grid is not None:
        assert here["grid"] == want_grid, (name, here["grid"])
    # byte for byte the generic kernel's and the run's without tails
    for arm in ("generic", "no-tail"):
        other = arms[arm]["cases"][name]
        assert other["ran"] == GENERIC and other["ranp"] == GENERIC, (arm, other["ran"])
        _same_records(here["res"], other["res"], f"{name}: default vs {arm}")
        for t in ("tally_tid", "tally_count", "tally_nomatch"):
            assert np.array_equal(here[t], other[t]), (name, arm, t)
        assert np.array_equal(here["tally_score"].view(np.uint64), other["tally_score"].view(np.uint64)), (name, arm, "tally_score")
        assert other["text"] == here["text"], (name, arm, "-p text")
    # the oracle: its text against the -p launch's (the generic kernel, whose read loop has the same front end), the plain launch's
    # records field by field against that launch's, its tallies against the plain launch's
    want, tally, nomatch = _oracle_run(oracle, key, G, first, n)
    got = here["text"]
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got.split("\n"), want.split("\n"))) if g != w]
    assert not bad, f"{name}: {len(bad)} differing records, first: {bad[0]}"
    assert got == want
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel"):
        assert np.array_equal(_bits(here["res"][f]), _bits(here["full"][f])), (name, f)
    assert here["tally_nomatch"].tolist() == list(nomatch), name
    assert dict(zip(here["tally_tid"].tolist(), here["tally_count"].tolist())) == {t: c for t, (c, s) in tally.items()}, name
    return here


@pytest.mark.parametrize("size", SIZES)
def test_launch_sizes_round_the_grid(arms, oracle, size):
    """1, 2, G - 1, G, G + 1, 2 G - 1, 2 G and 2 G + 1 reads of 150 bp: `more` false on the first trip, on the second, and for some
    of the waves only; the last trip of a wave asks for the launch's last record again."""
    G = arms["default"]["G"]
    n = _cases(G)["n=" + size][2]
    here = _check(arms, oracle, "n=" + size, UNI, want_grid=min(n, G))
    whole = arms["default"]["cases"]["n=2G+1"]["res"]
    _same_records(here["res"], whole[:n], f"the first {n} reads of the set")


def test_second_launch_ends_at_the_end_of_the_words_buffer(arms, oracle):
    """first = G + 3, up to the set's last read: result_base is not 0, the tail buffers hold this launch's reads only, and the
    clamped reload reads the last record of the words buffer."""
    G = arms["default"]["G"]
    here = _check(arms, oracle, "buffer_end", UNI, want_grid=min(G, NB - (G + 3)))
    # (the set's first 2 G + 1 reads were a launch of their own: where the two overlap the records are the same)
    whole = arms["default"]["cases"]["n=2G+1"]["res"]
    _same_records(here["res"][:2 * G + 1 - (G + 3)], whole[G + 3:], "reads G + 3 .. 2 G of the set")


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_of_the_headline_class(arms, oracle, variant):
    here = _check(arms, oracle, variant, RAN[variant])
    st = np.bincount(here["res"]["status"], minlength=6)
    if variant.startswith("exits"):
        assert (here["res"]["valid_kmers"] == 0).sum() >= 50 and ((here["res"]["valid_kmers"] > 0) & (here["res"]["valid_kmers"] < 30)).sum() >= 50, st
        assert (st > 0).sum() >= 3 and st[0] > 100, st
    else:
        assert st[0] > 0.5 * here["res"].shape[0], st


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child_main(sys.argv[1])
