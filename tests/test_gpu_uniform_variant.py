"""The fixed-geometry variant of the plain run (classify_one's UNI, kernels.hip): a launch whose reads all have 148 .. 151 bases at
k = 20 runs the headline kernel with the record geometry folded -- two full chunks and a tail, records of 16 words found by
arithmetic.  It must give the records and tallies of the PLAIN kernel bit for bit, and every launch that is not of that shape must
stay with PLAIN or the generic kernel.  `Engine.uniform_launches` is the sub-count of "plain" launches that ran as UNI;
LMAT_UNIFORM=0, read once per process, sends them to PLAIN -- that run is a child process."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BR = (3, 4, 4, 4, 4, 3)
LENS = (148, 149, 150, 151)   # 129 .. 132 k-mer positions at k = 20
N_READS = 8192
N_ORACLE = 2000
SMALL_TABLE = 4 << 20         # the compact layout's smallest table at k = 20 (bucket width 31)


def _engine(k=20, genome_len=3000):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy(BR)
    eng.synth_db(genome_len, k=k, seed=2002, table_bytes=SMALL_TABLE)
    return eng


def _launch(eng, reads, first=0, n=None, want_cands=False):
    """One blocking launch -> (records, candidates, the launch's count per kernel: generic / plain / of plain, uniform)."""
    n = len(reads) - first if n is None else n
    before, ub = eng.variant_launches(), eng.uniform_launches()
    res, cands = eng.classify(reads, first, n, want_cands=want_cands, cand_cap=64 * n if want_cands else None)
    after = eng.variant_launches()
    ran = {v: after[v] - before[v] for v in after}
    ran["uniform"] = eng.uniform_launches() - ub
    return res, cands, ran


UNI = {"generic": 0, "plain": 1, "uniform": 1}
PLAIN = {"generic": 0, "plain": 1, "uniform": 0}
GENERIC = {"generic": 1, "plain": 0, "uniform": 0}


def _tallies(eng):
    counts, nomatch = eng.counts()
    tid = np.array(sorted(counts), dtype=np.uint32)
    return {"tally_tid": tid, "tally_count": np.array([counts[t][0] for t in tid.tolist()], dtype=np.uint64),
            "tally_score": np.array([counts[t][1] for t in tid.tolist()], dtype=np.float64),
            "tally_nomatch": np.array(nomatch, dtype=np.uint64)}


def _random_reads(n, lengths, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [bytes(acgt[rng.integers(0, 4, size=int(lengths[i % len(lengths)]))]) for i in range(n)]


def _genus_block_reads(eng, n_scan, limit=150):
    """Indices of the first reads of the synthetic batch that hold a k-mer with a longer taxid list than one species gives (its
    strains and the species itself): reads over the genus-shared blocks (host-derived from the generator, as the database tests do)."""
    out = []
    for r in range(n_scan):
        ct = eng.synth_read_windows(LENS, 3003, r)[1]
        if ct.size and int(ct.max()) > BR[-1] + 1:
            out.append(r)
            if len(out) == limit:
                break
    return out


def _adversarial(eng, blob, off):
    """Every read keeps its 148 .. 151 bases, so the launch is a UNI one; what the front end, the tail entries, the repeat path and the
    early exits must get right is inside the reads.  blob, off: the first reads of the synthetic batch."""
    rng = np.random.default_rng(78)
    base = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(off.size - 1)]
    shared = set(_genus_block_reads(eng, len(base)))
    assert len(shared) >= 50, len(shared)
    out = []
    for i, r in enumerate(base):
        kind = i % 10
        n = len(r)
        if i in shared:
            pass                                                   # a read over a genus-shared block, as it is
        elif kind in (0, 1):
            p = n - 1 - int(rng.integers(0, 22))                   # an N inside the last 22 bases: tail windows (and the last of chunk 1) invalid
            r = r[:p] + b"N" + r[p + 1:]
        elif kind == 2:
            q = bytearray(r)                                       # an N every 15 .. 19 bases up to base 125: a few valid windows, all at the end
            for p in range(12, 125, int(rng.integers(15, 20))):
                q[p] = ord("N")
            r = bytes(q)
        elif kind == 3:
            q = bytearray(r)                                       # ... over the whole read: no valid window at all
            for p in range(int(rng.integers(0, 15)), n, int(rng.integers(15, 20))):
                q[p] = ord("N")
            r = bytes(q)
        elif kind == 4:
            r = b"ACGT"[i // 10 % 4:][:1] * n                      # a homopolymer: one k-mer, repeated in every chunk and the tail
        elif kind == 5:
            r = ((b"AT" if i % 20 < 10 else b"ACGT") * 76)[:n]     # tandem repeats: every k-mer recurs (the exact-repeat path)
        elif kind == 6:
            r = _random_reads(1, (n,), 1000 + i)[0]                # random bases: no hits
        out.append(r)
    assert {len(r) for r in out} == set(LENS)
    return out


def _cases(eng):
    synth = eng.synth_reads(N_READS, LENS, seed=3003)
    blob, off = synth.ascii(0, 3000)
    return {"synth": synth, "adversarial": eng.upload_reads(_adversarial(eng, blob, off))}


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
    """The default run in this process and the LMAT_UNIFORM=0 run in a fresh child, once for the tests below."""
    assert os.environ.get("LMAT_UNIFORM") in (None, "1") and os.environ.get("LMAT_PLAIN") in (None, "1")
    here = _run_cases(eng)
    fn = str(tmp_path_factory.mktemp("uniform") / "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), fn], env=dict(os.environ, LMAT_UNIFORM="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    return here, child


def _bits(x):
    return np.ascontiguousarray(x).view(f"u{x.dtype.itemsize}")


def _same_records(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    for f in a.dtype.names:   # field by field first: the message names what differs
        bad = np.nonzero(_bits(a[f]) != _bits(b[f]))[0]
        assert bad.size == 0, f"{what}: field {f} differs in {bad.size} records, first {int(bad[0])}: {a[f][bad[0]]} != {b[f][bad[0]]}"
    assert a.tobytes() == b.tobytes(), what


def _assert_bit_equal(a, b, what):
    _same_records(a["res"], b["res"], what)
    for t in ("tally_tid", "tally_count", "tally_nomatch"):
        assert np.array_equal(a[t], b[t]), (what, t)
    assert np.array_equal(a["tally_score"].view(np.uint64), b["tally_score"].view(np.uint64)), (what, "tally_score")


def _oracle_check(eng, reads, n, uni, tmp_path):
    """The oracle's text against the -p launch of the same reads (the generic kernel: candidates keep both variants off); the UNI
    launch's records against that launch's, field by field.  -> the oracle's tallies."""
    from lmat_amd import Params, synth
    import oracle_py
    blob, off = reads.ascii(0, n)
    blob0 = np.append(blob, np.uint8(0))
    eng.set_params(Params.run_rl(prn_all=1))
    eng.counts_reset()
    full, cands, ran = _launch(eng, reads, 0, n, want_cands=True)
    assert ran == GENERIC
    p = synth.write_aux_files(str(tmp_path), synth.make_taxonomy(BR, specials=False))
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.set_k(20)
    orc.set_options()
    kms = np.unique(np.concatenate([orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(n)]))
    counts, tids = eng.lookup(kms, stride=32)
    orc.add_lists32(kms, counts, tids)
    want, tally, nomatch = orc.classify(blob0, off, 20)
    orc.close()
    got = eng.format_out(full, cands, (blob0, off))
    eng.set_params(Params.run_rl(prn_all=0))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got.split("\n"), want.split("\n"))) if g != w]
    assert not bad, f"{len(bad)} differing records, first: {bad[0]}"
    assert got == want
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel"):
        assert np.array_equal(_bits(uni["res"][f][:n]), _bits(full[f])), f
    return tally, nomatch


def test_bit_equality_on_the_synthetic_batch(eng, runs, tmp_path):
    """8192 synthetic reads of 148 .. 151 bp: UNI ran here, PLAIN in the child, records and tallies are bit-equal, and the first 2000
    reads are the oracle's."""
    here, child = runs
    assert here["synth"]["ran"] == UNI
    assert child["synth"]["ran"] == PLAIN
    _assert_bit_equal(here["synth"], child["synth"], "synthetic batch, UNI vs LMAT_UNIFORM=0")
    res = here["synth"]["res"]
    assert set(np.unique(res["read_len"]).tolist()) == set(LENS)
    assert np.bincount(res["status"], minlength=6)[0] > 0.7 * N_READS   # mostly classified reads: the decision step on the wave runs
    reads = eng.synth_reads(N_READS, LENS, seed=3003)
    _oracle_check(eng, reads, N_ORACLE, here["synth"], tmp_path)
    reads.free()


def test_bit_equality_on_adversarial_reads_at_full_length(eng, runs, tmp_path):
    """An N inside the last 22 bases, an N every 15 .. 19 bases (fewer valid k-mers than min_kmer, or none), homopolymers and tandem
    repeats, random reads, reads over the genus-shared blocks -- every read of 148 .. 151 bases, so the launch is a UNI one."""
    here, child = runs
    assert here["adversarial"]["ran"] == UNI
    assert child["adversarial"]["ran"] == PLAIN
    _assert_bit_equal(here["adversarial"], child["adversarial"], "adversarial batch, UNI vs LMAT_UNIFORM=0")
    res = here["adversarial"]["res"]
    st = np.bincount(res["status"], minlength=6)
    assert st[0] > 500 and (st > 0).sum() >= 3, st                                    # classified, no-hit and too-few-k-mers records all occur
    assert ((res["valid_kmers"] > 0) & (res["valid_kmers"] < 30)).sum() >= 150, st   # below min_kmer with some valid k-mers
    assert (res["valid_kmers"] == 0).sum() >= 150
    synth = eng.synth_reads(N_READS, LENS, seed=3003)
    blob, off = synth.ascii(0, 3000)
    synth.free()
    reads = eng.upload_reads(_adversarial(eng, blob, off))
    tally, nomatch = _oracle_check(eng, reads, len(reads), here["adversarial"], tmp_path)
    assert here["adversarial"]["tally_nomatch"].tolist() == list(nomatch)
    assert dict(zip(here["adversarial"]["tally_tid"].tolist(), here["adversarial"]["tally_count"].tolist())) == {t: c for t, (c, s) in tally.items()}
    reads.free()


@pytest.mark.parametrize("case", ["one-147", "one-152", "one-below-k", "lengths-150-155", "candidates", "k18", "null-model"])
def test_launches_of_another_shape_do_not_take_the_variant(eng, case, tmp_path, monkeypatch):
    """One launch per condition that keeps UNI off; only the dispatch is under test."""
    if case in ("one-147", "one-152", "one-below-k"):
        odd = {"one-147": 147, "one-152": 152, "one-below-k": 11}[case]
        seqs = _random_reads(300, LENS, 21)
        assert _launch(eng, (r := eng.upload_reads(seqs)))[2] == UNI
        r.free()
        seqs[137] = _random_reads(1, (odd,), 22)[0]
        ran = _launch(eng, (r := eng.upload_reads(seqs)))[2]
        r.free()
        # 147 and below k: still one class with tails of four, the plain run / 152 bases: 133 positions, tails of eight
        assert ran == (GENERIC if case == "one-152" else PLAIN), ran
        return
    if case in ("lengths-150-155", "candidates"):
        ok = eng.synth_reads(512, LENS, seed=11)
        assert _launch(eng, ok)[2] == UNI
        if case == "candidates":
            ran = _launch(eng, ok, want_cands=True)[2]
        else:
            other = eng.synth_reads(512, (150, 155), seed=12)
            ran = _launch(eng, other)[2]
            other.free()
        ok.free()
        assert ran == GENERIC, ran
        return
    if case == "k18":   # 146 .. 149 bp have 129 .. 132 positions at k = 18, and records of 16 words
        e = _engine(k=18, genome_len=1000)
        reads = e.synth_reads(512, (146, 147, 148, 149), seed=13)
        ran = _launch(e, reads)[2]
        reads.free()
        e.close()
        assert ran == GENERIC
        return
    from lmat_amd import Engine, Params, synth
    os.makedirs(str(tmp_path / "ds"))
    info = synth.generate_dataset(str(tmp_path / "ds"), (2, 2, 2, 2, 3, 3), 400, 50)
    lst = synth.write_null_models(str(tmp_path / "nm"), synth.make_taxonomy((2, 2, 2, 2, 3, 3)))
    monkeypatch.setenv("LMAT_DIR", str(tmp_path / "nm"))
    e = Engine(0, Params.run_rl(prn_all=0))
    e.load_taxonomy(info["tree"], info["depth"], info["rank"], info["idmap"])
    e.build_db(info["db"], k=20)
    reads = e.upload_reads(_random_reads(256, (150,), 14))
    assert _launch(e, reads)[2] == UNI
    e.load_null_models(lst)
    ran = _launch(e, reads)[2]
    reads.free()
    e.close()
    assert ran == GENERIC


@pytest.mark.parametrize("length", [148, 151])
def test_batches_of_one_length_at_either_end_take_the_variant(eng, length):
    reads = eng.synth_reads(1024, (length,), seed=31)
    res, _, ran = _launch(eng, reads)
    reads.free()
    assert ran == UNI
    assert (res["read_len"] == length).all() and np.bincount(res["status"], minlength=6)[0] > 700


def test_record_offsets_are_arithmetic(eng, runs):
    """Sub-ranges that start at odd reads, and two launches in flight over adjacent ranges: row by row the whole-set records."""
    whole = runs[0]["synth"]
    reads = eng.synth_reads(N_READS, LENS, seed=3003)
    for first, count in ((1, 777), (63, 4099), (4097, 4095)):
        res, _, ran = _launch(eng, reads, first, count)
        assert ran == UNI
        _same_records(res, whole["res"][first:first + count], f"classify(first={first}, count={count})")
    before = eng.uniform_launches()
    eng.counts_reset()
    eng.classify_async(reads, 0, 4097)
    eng.classify_async(reads, 4097, N_READS - 4097)
    eng.sync()
    assert eng.uniform_launches() == before + 2
    _same_records(eng.fetch_results(0, N_READS - 4097), whole["res"][4097:], "second of two launches in flight")
    t = _tallies(eng)
    for f in ("tally_tid", "tally_count", "tally_nomatch"):
        assert np.array_equal(t[f], whole[f]), f
    reads.free()


def test_stream_slots_of_either_shape(eng):
    """A uniform batch (151 bp throughout, then 148 .. 151 mixed) and a non-uniform one through a two-slot stream: the records of
    the blocking call, and the uniform ones ran as UNI."""
    from lmat_amd.capi import Stream
    batches = [_random_reads(500, (151,), 41), None, _random_reads(500, (150, 120, 151), 43)]
    synth = eng.synth_reads(1500, LENS, seed=3003)
    blob, off = synth.ascii(0, 1500)
    synth.free()
    batches[1] = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(1500)]
    want = []
    for b in batches:
        r = eng.upload_reads(b)
        want.append(_launch(eng, r)[0])
        r.free()
    st = Stream(eng, 2048, 2048 * 160, 0, n_slots=2)
    got, ran = [], []
    for i, b in enumerate(batches):
        o = np.zeros(len(b) + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in b], out=o[1:])
        before = eng.uniform_launches()
        st.submit(np.frombuffer(b"".join(b) + b"\0", dtype=np.uint8), o, tag=i)
        ran.append(eng.uniform_launches() - before)
        if st.in_flight == 2:
            got.append(st.next())
    while st.in_flight:
        got.append(st.next())
    st.close()
    assert ran == [1, 1, 0]
    assert [g[2] for g in got] == [0, 1, 2]
    for i, g in enumerate(got):
        _same_records(g[0], want[i], f"stream batch {i}")


# Power-of-two and fractional bucket widths: not repeated here.  Their tables are 16 GiB and more (test_gpu_plain_variant.py builds
# one in 1.8 s, the fractional widths need over 64 GiB), and UNI leaves the bucket address -- cpt_finish from `hi` on, and the tail
# kernel's cpt_address -- as PLAIN has it; the existing width tests run it through PLAIN.


if __name__ == "__main__":   # the child of the `runs` fixture: the same two batches with whatever LMAT_UNIFORM says, pickled
    sys.path.insert(0, ROOT)
    _e = _engine()
    _out = _run_cases(_e)
    _e.close()
    with open(sys.argv[1], "wb") as _f:
        pickle.dump(_out, _f)
