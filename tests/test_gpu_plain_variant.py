"""The plain-run variant of the 160-k-mer fast class (classify_one's PLAIN, kernels.hip): the same records and tallies as the generic
kernel, bit for bit, on the launches that qualify, and the generic kernel on every launch that does not.  `Engine.variant_launches`
says which of the two a launch ran as; LMAT_PLAIN=0, read once per process, turns the variant off -- that run is a child process."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BR = (3, 4, 4, 4, 4, 3)
LENS = (148, 149, 150, 151)   # 129 .. 132 k-mer positions at k = 20: every length whose tail is four entries
N_READS = 20000
N_ORACLE = 4000               # reads of the synthetic batch the CPU oracle re-derives (all of the adversarial batch)
SMALL_TABLE = 4 << 20         # the compact layout's smallest table at k = 20: 2^32 / 31 buckets, a width that is no power of two
POW2_TABLE = 16 << 30         # 2^28 buckets of width 16: the shift-and-mask arm of the bucket address


def _engine(k=20, table_bytes=SMALL_TABLE, genome_len=3000):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy(BR)
    eng.synth_db(genome_len, k=k, seed=2002, table_bytes=table_bytes)
    return eng


def _launch(eng, reads, want_cands=False, n=None):
    """One blocking launch over the whole batch -> (records, candidates, the launch's count per kernel variant)."""
    n = len(reads) if n is None else n
    before = eng.variant_launches()
    res, cands = eng.classify(reads, 0, n, want_cands=want_cands, cand_cap=64 * n if want_cands else None)
    after = eng.variant_launches()
    return res, cands, {v: after[v] - before[v] for v in after}


def _tallies(eng):
    counts, nomatch = eng.counts()
    tid = np.array(sorted(counts), dtype=np.uint32)
    return {"tally_tid": tid, "tally_count": np.array([counts[t][0] for t in tid.tolist()], dtype=np.uint64),
            "tally_score": np.array([counts[t][1] for t in tid.tolist()], dtype=np.float64),
            "tally_nomatch": np.array(nomatch, dtype=np.uint64)}


def _adversarial(blob, off):
    """Reads the front end, the tail entries and the early exits must get right, around genome reads of 148 .. 151 bp (blob, off:
    the first reads of the synthetic batch, which also make up every fourth read here)."""
    rng = np.random.default_rng(77)
    base = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(off.size - 1)]
    out = []
    for i, r in enumerate(base):
        kind = i % 12
        if kind == 0:
            r = r[:int(rng.integers(1, 20))]                       # shorter than k
        elif kind in (1, 2):
            p = len(r) - 1 - int(rng.integers(0, 22))              # an N inside the last 22 bases: the tail windows are invalid
            r = r[:p] + b"N" + r[p + 1:]
        elif kind == 3:
            r = b"ACGT"[i // 12 % 4:][:1] * len(r)                 # a homopolymer: one k-mer, repeated (poly-A / poly-T: a palindrome pair)
        elif kind == 4:
            r = (b"AT" if i % 24 < 12 else b"ACGT") * 76           # short tandem repeats: every k-mer recurs, AT..AT is its own reverse complement
            r = r[:len(base[i])]
        elif kind == 5:
            q = bytearray(r)                                       # an N every 25 bases: no window of 20 within the first 125, a few at the end
            for p in range(12, 125, int(rng.integers(15, 20))):
                q[p] = ord("N")
            r = bytes(q)                                           # fewer valid k-mers than min_kmer = 30
        elif kind == 6:
            r = r[:int(rng.integers(20, 49))]                      # 1 .. 29 k-mers: below min_kmer by length
        elif kind == 7:
            r = r[:128 + 19] if i % 24 < 12 else r[:127 + 19]      # exactly two chunks / one position short of them: no tail
        out.append(r)
    return out


def _cases(eng):
    """The two batches every run classifies: the synthetic one, and the adversarial one uploaded as text."""
    synth = eng.synth_reads(N_READS, LENS, seed=3003)
    blob, off = synth.ascii(0, 3000)
    adv = _adversarial(blob, off)
    return {"synth": synth, "adversarial": eng.upload_reads(adv)}


def _run_cases(eng):
    out = {}
    for name, reads in _cases(eng).items():
        eng.counts_reset()
        res, _, ran = _launch(eng, reads)
        out[name] = dict(_tallies(eng), res=res, ran=ran)
        reads.free()
    return out


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def runs(eng, tmp_path_factory):
    """The default run in this process and the LMAT_PLAIN=0 run in a fresh child, once for the tests below."""
    assert os.environ.get("LMAT_PLAIN") in (None, "1"), "this module compares the default with LMAT_PLAIN=0 itself"
    here = _run_cases(eng)
    fn = str(tmp_path_factory.mktemp("plain") / "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), fn], env=dict(os.environ, LMAT_PLAIN="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    return here, child


def _bits(x):
    """A record field as unsigned integers of its own width: floats compare by bit pattern."""
    return np.ascontiguousarray(x).view(f"u{x.dtype.itemsize}")


def _assert_bit_equal(a, b, what):
    assert a["res"].dtype == b["res"].dtype and a["res"].shape == b["res"].shape
    for f in a["res"].dtype.names:   # field by field first: the message names what differs
        x, y = a["res"][f], b["res"][f]
        bad = np.nonzero(_bits(x) != _bits(y))[0]
        assert bad.size == 0, f"{what}: field {f} differs in {bad.size} records, first {int(bad[0])}: {x[bad[0]]} != {y[bad[0]]}"
    assert a["res"].tobytes() == b["res"].tobytes(), what
    for t in ("tally_tid", "tally_count", "tally_nomatch"):
        assert np.array_equal(a[t], b[t]), (what, t)
    assert np.array_equal(a["tally_score"].view(np.uint64), b["tally_score"].view(np.uint64)), (what, "tally_score")


def _oracle_check(eng, reads, n, plain, tmp_path):
    """The oracle's text against the -p launch of the same reads (the generic kernel: candidates keep the variant off), the way
    test_gpu_parity.py compares; the plain launch's records against that launch's, field by field; its tallies against the oracle's.
    The oracle's k-mer table holds the lists the device table returns for these reads' k-mers."""
    from lmat_amd import Params, synth
    import oracle_py
    blob, off = reads.ascii(0, n)
    blob0 = np.append(blob, np.uint8(0))
    eng.set_params(Params.run_rl(prn_all=1))
    eng.counts_reset()
    full, cands, ran = _launch(eng, reads, want_cands=True, n=n)
    assert ran == {"generic": 1, "plain": 0}
    p = synth.write_aux_files(str(tmp_path), synth.make_taxonomy(BR, specials=False))
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.set_k(20)
    orc.set_options()
    kms = [orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(n)]
    kms = np.unique(np.concatenate(kms))
    counts, tids = eng.lookup(kms, stride=32)
    orc.add_lists32(kms, counts, tids)
    want, tally, nomatch = orc.classify(blob0, off, 20)
    orc.close()
    got = eng.format_out(full, cands, (blob0, off))
    eng.set_params(Params.run_rl(prn_all=0))
    gl, wl = got.split("\n"), want.split("\n")
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(gl, wl)) if g != w]
    assert not bad, f"{len(bad)} differing records, first: {bad[0]}"
    assert got == want
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel"):
        assert np.array_equal(_bits(plain["res"][f][:n]), _bits(full[f])), f
    return tally, nomatch, (counts > 0).sum()


def test_variant_parity_on_the_synthetic_batch(eng, runs, tmp_path):
    """20 k synthetic reads of 148 .. 151 bp against the smallest compact table (bucket width 31: the exact-division arm of the
    bucket address): PLAIN ran here, the generic kernel in the child, records and tallies are bit-equal, and both are the oracle's."""
    lib = eng.lib
    import ctypes as C
    nb = C.c_uint64(0)
    assert lib.lmat_table_address(20, SMALL_TABLE // 64, 0, C.byref(nb), None, None) == 0
    assert nb.value == -(-(1 << 32) // 31) and nb.value & (nb.value - 1)   # width 31: no shift, no fractional width
    here, child = runs
    assert here["synth"]["ran"] == {"generic": 0, "plain": 1}
    assert child["synth"]["ran"] == {"generic": 1, "plain": 0}
    _assert_bit_equal(here["synth"], child["synth"], "synthetic batch, PLAIN vs LMAT_PLAIN=0")
    res = here["synth"]["res"]
    assert set(np.unique(res["read_len"]).tolist()) == set(LENS)
    st = np.bincount(res["status"], minlength=6)
    assert st[0] > 0.7 * N_READS, st   # the batch is mostly classified reads: the decision step on the wave runs
    reads = eng.synth_reads(N_READS, LENS, seed=3003)
    _, _, hits = _oracle_check(eng, reads, N_ORACLE, here["synth"], tmp_path)
    assert hits > 10000
    reads.free()


def test_variant_parity_on_adversarial_reads(eng, runs, tmp_path):
    """Reads below k, an N inside the last 22 bases, homopolymers and tandem repeats, fewer valid k-mers than min_kmer, reads that end
    at the chunk boundary -- mixed into genome reads of 148 .. 151 bp, so the launch still qualifies for the variant."""
    here, child = runs
    assert here["adversarial"]["ran"] == {"generic": 0, "plain": 1}
    assert child["adversarial"]["ran"] == {"generic": 1, "plain": 0}
    _assert_bit_equal(here["adversarial"], child["adversarial"], "adversarial batch, PLAIN vs LMAT_PLAIN=0")
    res = here["adversarial"]["res"]
    st = np.bincount(res["status"], minlength=6)
    assert (res["read_len"] < 20).sum() >= 200 and st[0] > 500 and (st > 0).sum() >= 3, st   # short, classified and no-hit records all occur
    assert ((res["valid_kmers"] > 0) & (res["valid_kmers"] < 30)).sum() >= 300               # below min_kmer with some valid k-mers
    synth = eng.synth_reads(N_READS, LENS, seed=3003)
    blob, off = synth.ascii(0, 3000)
    synth.free()
    reads = eng.upload_reads(_adversarial(blob, off))
    tally, nomatch, _ = _oracle_check(eng, reads, len(reads), here["adversarial"], tmp_path)
    assert here["adversarial"]["tally_nomatch"].tolist() == list(nomatch)
    assert dict(zip(here["adversarial"]["tally_tid"].tolist(), here["adversarial"]["tally_count"].tolist())) == {t: c for t, (c, s) in tally.items()}
    reads.free()


def _random_reads(n, length, seed):
    rng = np.random.default_rng(seed)
    return [bytes(row) for row in np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, length))]]


@pytest.mark.parametrize("case", ["candidates", "longest-147", "longest-155", "mixed-classes", "k18", "null-model"])
def test_launches_that_do_not_qualify_take_the_generic_kernel(eng, case, tmp_path, monkeypatch):
    """One launch per condition the variant leaves to the generic kernel; only the dispatch is under test (the results of all of
    these are the existing suites' business).  The first launch shows that the same engine does take the variant otherwise."""
    if case in ("candidates", "longest-147", "longest-155", "mixed-classes"):
        ok = eng.synth_reads(512, LENS, seed=11)
        assert _launch(eng, ok)[2] == {"generic": 0, "plain": 1}
        if case == "candidates":       # -p: candidate pairs are written
            ran = _launch(eng, ok, want_cands=True)[2]
        else:
            # 128 positions: no tail / 136: tails of eight / 131 and 231: two class lists, each launch with a read index
            lens = {"longest-147": (140, 147), "longest-155": (150, 155), "mixed-classes": (150, 250)}[case]
            other = eng.synth_reads(512, lens, seed=12)
            ran = _launch(eng, other)[2]
            other.free()
        ok.free()
        assert ran["plain"] == 0 and ran["generic"] >= 1, ran
        return
    if case == "k18":   # 146 .. 149 bp have 129 .. 132 positions at k = 18: k alone keeps the variant off
        e = _engine(k=18, genome_len=1000)
        reads = e.synth_reads(512, (146, 147, 148, 149), seed=13)
        ran = _launch(e, reads)[2]
        reads.free()
        e.close()
        assert ran == {"generic": 1, "plain": 0}
        return
    # a null model loaded: a database from files, whose taxonomy carries the ranks the models name
    from lmat_amd import Engine, Params, synth
    os.makedirs(str(tmp_path / "ds"))
    info = synth.generate_dataset(str(tmp_path / "ds"), (2, 2, 2, 2, 3, 3), 400, 50)
    tax = synth.make_taxonomy((2, 2, 2, 2, 3, 3))
    lst = synth.write_null_models(str(tmp_path / "nm"), tax)
    monkeypatch.setenv("LMAT_DIR", str(tmp_path / "nm"))
    e = Engine(0, Params.run_rl(prn_all=0))
    e.load_taxonomy(info["tree"], info["depth"], info["rank"], info["idmap"])
    e.build_db(info["db"], k=20)
    reads = e.upload_reads(_random_reads(256, 150, 14))   # random 150-mers: 131 positions, no hits to score
    assert _launch(e, reads)[2] == {"generic": 0, "plain": 1}
    e.load_null_models(lst)
    ran = _launch(e, reads)[2]
    reads.free()
    e.close()
    assert ran == {"generic": 1, "plain": 0}


def test_power_of_two_bucket_width(tmp_path):
    """2^28 buckets (16 GiB): the bucket address is a shift and a mask.  PLAIN against the -p launch (generic kernel) of the same
    reads in this process, and that launch against the oracle.  Measured on an MI355X: 1.8 s for the whole case, the table's
    allocation and build included (the file's nine cases: 6.0 s)."""
    import ctypes as C
    e = _engine(table_bytes=POW2_TABLE, genome_len=20000)
    nb = C.c_uint64(0)
    assert e.lib.lmat_table_address(20, POW2_TABLE // 64, 0, C.byref(nb), None, None) == 0 and nb.value == 1 << 28
    reads = e.synth_reads(N_ORACLE, LENS, seed=3003)
    e.counts_reset()
    res, _, ran = _launch(e, reads)
    assert ran == {"generic": 0, "plain": 1}
    assert np.bincount(res["status"], minlength=6)[0] > 0.7 * N_ORACLE
    _oracle_check(e, reads, N_ORACLE, {"res": res}, tmp_path)
    reads.free()
    e.close()


if __name__ == "__main__":   # the child of the `runs` fixture: the same two batches with whatever LMAT_PLAIN says, pickled
    sys.path.insert(0, ROOT)
    _e = _engine()
    _out = _run_cases(_e)
    _e.close()
    with open(sys.argv[1], "wb") as _f:
        pickle.dump(_out, _f)
