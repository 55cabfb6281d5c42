"""GPU: the streamed boundary (lmat_stream_*) at its own edges.  The blocking path has every capacity edge and every run mode under
single-read probes (test_gpu_capacity_edges.py, test_gpu_mode_tiers.py); this file sends the same probes through the ring of slots
-- slot-owned result and candidate buffers, per-batch error flags, offsets made on the device, length-class lists partitioned on
the host -- and takes the one path only the ring has: a slot that grows its candidate buffer and runs its batch again.

What is expected comes from the CPU oracle (text, tallies, candidate counts) and from capacity_probes.route (class-to-class
counters), never from the engine's blocking path.  Every test asserts through Stream.stats() and Engine.last_counters() that the
branch it is about was taken.

A slot is created with room for cands_per_read * max_reads + 1024 * 2048 candidate pairs (the second term is what the sub-cursors of
a large launch may leave unused); it grows, fourfold, only when one batch prints more than that."""
import numpy as np
import pytest

import capacity_probes as cp
from test_gpu_capacity_edges import CAPACITY_MESSAGE, MID_ON, _Bench, _assert_tallies, _blob, _expected_counters, _good, _orders, _same_records
from test_gpu_mode_tiers import MODES, _ModeBench, _Set

pytestmark = pytest.mark.gpu

SLOT_SLACK = 1024 * 2048      # pairs a slot holds beyond cands_per_read * max_reads (lmat_stream_create)
NO_TALLIES = ({}, [0, 0, 0])


def _submit(st, reads, tag=0):
    st.submit(*_blob(reads), tag=tag)


def _take(st):
    """-> (results, candidates or None, n_cands as lmat_stream_next returned it, tag)"""
    res, cands, tag = st.next()
    return res, cands, 0 if cands is None else len(cands), tag


def _text(eng, res, cands, reads, first_index=0):
    return eng.format_out(res, cands, _blob(reads), first_index)


def _sum_tallies(parts):
    """(tally, no-match counters) of several oracle runs added up."""
    tally, nm = {}, [0, 0, 0]
    for t, m in parts:
        for tid, (c, s) in t.items():
            c0, s0 = tally.get(tid, (0, 0.0))
            tally[tid] = (c0 + c, s0 + s)
        nm = [a + int(b) for a, b in zip(nm, m)]
    return tally, nm


def _reads(probes):
    return [p.read for p in probes]


@pytest.fixture(scope="module")
def bench16(tmp_path_factory):
    b = _Bench(str(tmp_path_factory.mktemp("ring16")), wide=False)
    yield b
    b.close()


@pytest.fixture(scope="module")
def bench_wide(tmp_path_factory):
    b = _Bench(str(tmp_path_factory.mktemp("ring_wide")), wide=True)
    yield b
    b.close()


def _probe(b, name):
    return [p for p in b.probes if p.name == name][0]


# ---- 1. the grow path ------------------------------------------------------------------------------------------------------------
def _want(b, probes):
    """_Bench.want, and for a batch of replicas of one probe the oracle's record of that probe under every index (the oracle takes
    a read at a time: checked below on three replicas), its tallies times the number of replicas."""
    if len(probes) < 100 or any(p is not probes[0] for p in probes):
        return b.want(probes)
    key = ("replicas", probes[0].name, len(probes))
    if key not in b._want:
        text, tally, nm = b.want(probes[:1])
        assert text.startswith("r0\t") and text.count("\n") == 1
        tiled = lambda k: "".join("r%d%s" % (i, text[2:]) for i in range(k))
        assert b.orc.classify(*_blob(_reads(probes[:3])), cp.K)[0] == tiled(3)
        n = len(probes)
        b._want[key] = (tiled(n), {t: (c * n, s * n) for t, (c, s) in tally.items()}, [int(x) * n for x in nm])
    return b._want[key]


def _check_batches(b, st, batches, tags):
    for ps, tag in zip(batches, tags):
        res, cands, n, got_tag = _take(st)
        text = _want(b, ps)[0]
        assert got_tag == tag
        assert n == sum(p.T for p in ps) == int(res["n_cand"].sum()), (tag, n)
        assert _text(b.eng, res, cands, _reads(ps)) == text, tag


def _grow(b, name, copies, rounds):
    """An ordinary batch, `copies` replicas of one probe, an ordinary batch: all three in flight on three slots.  With -p a probe
    prints T pairs; the middle batch prints copies * T, more than its slot's cands_per_read * max_reads + 1024 * 2048."""
    from lmat_amd import Stream
    probe = _probe(b, name)
    big, good = [probe] * copies, _good(b)
    cap0 = 1 * copies + SLOT_SLACK
    assert cap0 * 4 ** (rounds - 1) < copies * probe.T <= cap0 * 4 ** rounds      # the slot must grow `rounds` times, no more
    st = Stream(b.eng, max_reads=copies, max_bases=copies * len(probe.read) + 64, cands_per_read=1, n_slots=3)
    try:
        assert st.stats()["cand_cap"] == cap0 and st.stats()["grow_reruns"] == 0
        batches = [good, big, good[::-1]]
        b.eng.counts_reset()
        for i, ps in enumerate(batches):
            _submit(st, _reads(ps), tag=i)
        assert st.in_flight == 3
        _check_batches(b, st, batches, (0, 1, 2))                     # the batches before and behind it are untouched
        stats = st.stats()
        assert stats["grow_reruns"] == rounds and stats["cand_cap"] == cap0 * 4 ** rounds
        tally, nm = _sum_tallies([_want(b, ps)[1:] for ps in batches])
        _assert_tallies(b.eng.counts(), tally, nm, sum(len(ps) for ps in batches))   # the re-run was not tallied a second time
        # three more batches: the second of them goes through the grown slot
        later = [good[::-1], good, good[1:]]
        b.eng.counts_reset()
        for i, ps in enumerate(later):
            _submit(st, _reads(ps), tag=10 + i)
        _check_batches(b, st, later, (10, 11, 12))
        tally, nm = _sum_tallies([b.want(ps)[1:] for ps in later])
        _assert_tallies(b.eng.counts(), tally, nm, sum(len(ps) for ps in later))
        assert b.eng.last_counters() == _expected_counters(later[-1], 150, b.wide)
        assert st.stats()["grow_reruns"] == rounds
        b.eng.sync()
    finally:
        st.close()


def test_a_slot_grows_and_reruns_its_batch_16bit(bench16):
    """520 replicas of the T = 4096 probe print 2 129 920 pairs; the slot holds 520 + 2 097 152.  One grow re-run, the slot at four
    times its capacity, every record and candidate list the oracle's, the tallies of the three batches exact.  Timed once on an
    MI355X with its two alternatives, all of 2.1 M pairs: 0.31 s, against 0.34 s for 2200 replicas of the T = 1024 probe and 0.31 s
    for 8300 of the T = 256 probe; the batch with the fewest reads stays."""
    _grow(bench16, "T4096", 520, 1)


def test_a_slot_grows_twice_16bit(bench16):
    """2080 replicas print 8 519 680 pairs, more than four times the slot's 2080 + 2 097 152: the loop in lmat_stream_next goes
    round twice (two re-runs, the slot at sixteen times its capacity), and still nothing is tallied twice.  (0.9 s on an MI355X.)"""
    _grow(bench16, "T4096", 2080, 2)


def test_a_grown_slot_without_dash_p_16bit(bench16):
    """prn_all = 0: a read reserves pairs for its lineage, not for its candidates, and the oracle prints none of them.  The
    one-hit probe registers one strain and its ancestors; its lineage is the call with every ancestor up to the root, n1 = depth
    of the call + 1 pairs (checked on a one-read batch).  The same slot arithmetic as with -p: the smallest batch of replicas
    that overflows a slot of 1 * n + 1024 * 2048 pairs has 1024 * 2048 / (n1 - 1) + 1 reads -- above 2^18 (the partition runs on
    four host threads) and above 128 K (the pairs are handed out through sub-cursors, in the slot's own buffer: the cursor
    then counts whole chunks, so the pairs returned are n * n1 plus at most the 1024 * 2048 the sub-cursors may leave unused).
    Three batches in flight on three slots, a one-read batch on either side.  Every record is the one whose text is the oracle's;
    the tallies are the oracle's times the number of reads, so the re-run was tallied nowhere."""
    from lmat_amd import Params, Stream
    b = bench16
    probe = _probe(b, "one_hit")
    b.orc.set_options(prn_all=0)
    try:
        text1, tally1, nm1 = b.orc.classify(*_blob([probe.read]), cp.K)
    finally:
        b.orc.set_options()
    (call, (count, _)), = tally1.items()
    assert count == 1
    b.eng.set_params(Params.run_rl(prn_all=0))
    try:
        st = Stream(b.eng, max_reads=4, max_bases=1024, cands_per_read=1, n_slots=1)
        try:
            _submit(st, [probe.read])
            one, c1, n1, _ = _take(st)
            assert _text(b.eng, one, c1, [probe.read]) == text1
            assert n1 == len(b.ps["tax"].path(call)) + 1 >= 2, n1
        finally:
            st.close()
        n = SLOT_SLACK // (n1 - 1) + 1
        assert n * n1 > 1 * n + SLOT_SLACK and n > (1 << 18)
        st = Stream(b.eng, max_reads=n, max_bases=n * len(probe.read) + 64, cands_per_read=1, n_slots=3)
        try:
            b.eng.counts_reset()
            _submit(st, [probe.read], tag=1)
            off = np.arange(n + 1, dtype=np.uint64) * np.uint64(len(probe.read))
            st.submit(np.frombuffer(probe.read.encode() * n, dtype=np.uint8), off, tag=2)
            _submit(st, [probe.read], tag=3)
            assert st.in_flight == 3
            first, _, nf, tag = _take(st)
            assert tag == 1 and nf == n1
            _same_records(first, one)
            res, cands, nc, tag = _take(st)
            stats = st.stats()
            assert tag == 2 and stats["grow_reruns"] == 1 and stats["cand_cap"] == 4 * (n + SLOT_SLACK), stats
            assert stats["threaded"] == 1 and stats["uniform"] == 3
            assert len(res) == n and n * n1 <= nc <= n * n1 + SLOT_SLACK, (nc, n * n1)
            last, _, nl, tag = _take(st)                                 # the batch behind it is untouched
            assert tag == 3 and nl == n1
            _same_records(last, one)
            _same_records(res, one[np.zeros(n, dtype=np.int64)])
            assert (res["n_cand"] == one["n_cand"][0]).all() and (res["read_len"] == len(probe.read)).all()
            tally = {t: (c * (n + 2), s * (n + 2)) for t, (c, s) in tally1.items()}
            _assert_tallies(b.eng.counts(), tally, [int(x) * (n + 2) for x in nm1], n + 2)
        finally:
            st.close()
    finally:
        b.eng.set_params(Params.run_rl())


# ---- 2. every capacity probe through the ring --------------------------------------------------------------------------------------
def _each_probe_a_batch(b):
    """One Stream, two slots, a probe a batch: the slots are reused probe after probe.  A batch of one read is a batch of one
    length: its offsets are made on the device."""
    from lmat_amd import Stream
    st = Stream(b.eng, max_reads=4, max_bases=4096, cands_per_read=4200, n_slots=2)
    bad = []
    try:
        for p in b.probes:
            text, tally, nm = b.want([p])
            b.eng.counts_reset()
            _submit(st, [p.read])
            res, cands, n, _ = _take(st)
            flow = b.eng.last_counters()
            try:
                assert _text(b.eng, res, cands, [p.read]) == text
                _assert_tallies(b.eng.counts(), tally, nm, 1)
                assert n == int(res["n_cand"][0]) == p.T
                if p.P <= 512:
                    where, want = cp.route(p.dims, len(p.read), b.wide, MID_ON)
                    assert flow == want, (flow, want, where)
                    if MID_ON and p.P > 0:
                        assert where == p.expected
            except AssertionError as e:
                bad.append("%s (T %d, E %d, D %d, P %d; %s): %s" % (p.name, p.T, p.E, p.D, p.P, p.expected, str(e)[:300]))
        stats = st.stats()
        assert stats["uniform"] == len(b.probes) and stats["general"] == 0 and stats["grow_reruns"] == 0, stats
    finally:
        st.close()
    assert not bad, "\n".join(bad)


def test_each_probe_a_batch_16bit(bench16):
    _each_probe_a_batch(bench16)


def test_each_probe_a_batch_wide(bench_wide):
    _each_probe_a_batch(bench_wide)


def _ring(b, batches, n_slots):
    """The batches in flight together on n_slots slots (len(batches) <= n_slots), each compared with the oracle; the tallies are
    the sum; the counters are those of the batch submitted last."""
    from lmat_amd import Stream
    assert len(batches) <= n_slots
    most = max(len(ps) for ps in batches)
    st = Stream(b.eng, max_reads=most, max_bases=max(sum(len(p.read) for p in ps) for ps in batches) + 64,
                cands_per_read=max(sum(p.T for p in ps) for ps in batches) // most + 1, n_slots=n_slots)
    try:
        b.eng.counts_reset()
        for i, ps in enumerate(batches):
            _submit(st, _reads(ps), tag=i)
        assert st.in_flight == len(batches)
        _check_batches(b, st, batches, range(len(batches)))
        tally, nm = _sum_tallies([b.want(ps)[1:] for ps in batches])
        _assert_tallies(b.eng.counts(), tally, nm, sum(len(ps) for ps in batches))
        last = batches[-1]
        want = _expected_counters(last, max(len(p.read) for p in last), b.wide)
        assert b.eng.last_counters() == want, (b.eng.last_counters(), want)
        stats = st.stats()
        assert stats["grow_reruns"] == 0
        return stats
    finally:
        st.close()


@pytest.mark.parametrize("order", ["as_built", "reversed", "shuffled"])
def test_all_probes_in_one_streamed_batch_16bit(bench16, order):
    """Reads of 19 to 2068 bp in one batch: offsets copied in, and all four length-class lists sent."""
    stats = _ring(bench16, [_orders(bench16.probes)[order]], 2)
    assert (stats["general"], stats["class_lists"], stats["uniform"]) == (1, 1, 0)


@pytest.mark.parametrize("order", ["as_built", "reversed", "shuffled"])
def test_all_probes_in_one_streamed_batch_wide(bench_wide, order):
    stats = _ring(bench_wide, [_orders(bench_wide.probes)[order]], 2)
    assert (stats["general"], stats["class_lists"], stats["uniform"]) == (1, 1, 0)


@pytest.mark.parametrize("n_slots", [2, 3])
def test_short_and_long_probes_in_flight_together_16bit(bench16, n_slots):
    """The short probes (every tier) and the long ones (the chain ends in the global-memory class) as batches of their own, both --
    with three slots the short ones once more, reversed -- in flight at once: each launch has the tiers of its own longest read."""
    g = bench16.groups()
    short = g["p131"] + g["len"]
    batches = [short, g["long"]] + ([short[::-1]] if n_slots == 3 else [])
    stats = _ring(bench16, batches, n_slots)
    assert stats["general"] == len(batches)


@pytest.mark.parametrize("n_slots", [2, 3])
def test_short_and_long_probes_in_flight_together_wide(bench_wide, n_slots):
    g = bench_wide.groups()
    batches = [g["p131"], g["long"]] + ([g["p131"][::-1]] if n_slots == 3 else [])
    stats = _ring(bench_wide, batches, n_slots)
    assert stats["uniform"] + stats["general"] == len(batches) and stats["general"] >= 1


def _beyond_the_chain_streamed(b, name):
    """A read beyond the chain as the middle of three batches: LMAT_E_CAPACITY for that batch, every time it is asked for; dropped,
    the batch behind it comes next; nothing leaked into the context, and the tallies are those of the two good batches."""
    from lmat_amd import Stream
    from lmat_amd.capi import LmatError
    good = _good(b)
    batches = [good, [b.beyond[name]], good[::-1]]
    st = Stream(b.eng, max_reads=len(good), max_bases=8192, cands_per_read=4200, n_slots=3)
    try:
        b.eng.counts_reset()
        for i, ps in enumerate(batches):
            _submit(st, _reads(ps), tag=i)
        _check_batches(b, st, batches[:1], (0,))
        for _ in range(2):
            with pytest.raises(LmatError) as ei:
                st.next()
            assert ei.value.code == -4 and CAPACITY_MESSAGE in str(ei.value)
        st.drop_failed()
        _check_batches(b, st, batches[2:], (2,))
        assert st.next() is None
        b.eng.sync()
        tally, nm = _sum_tallies([b.want(good)[1:], b.want(good[::-1])[1:]])
        _assert_tallies(b.eng.counts(), tally, nm, 2 * len(good))
        _submit(st, _reads(good), tag=7)
        _submit(st, _reads(good[::-1]), tag=8)                     # through the slot the failed batch had: its flags are gone
        _check_batches(b, st, [good, good[::-1]], (7, 8))
    finally:
        st.close()


@pytest.mark.parametrize("name", ["T4097", "TL4097", "E16385"])
def test_beyond_the_chain_streamed_16bit(bench16, name):
    _beyond_the_chain_streamed(bench16, name)


def test_beyond_the_chain_streamed_wide(bench_wide):
    _beyond_the_chain_streamed(bench_wide, "wT4097")


def test_a_read_too_long_is_refused_at_submit(bench16):
    """One base over the longest read the chain takes (32 768 + k - 1): refused before anything is queued, the slot is free again
    -- the next acquire and submit work -- and nothing was tallied."""
    from lmat_amd import Stream
    from lmat_amd.capi import LmatError
    b = bench16
    good = _good(b)
    rng = np.random.default_rng(5)
    too_long = "".join("ACGT"[i] for i in rng.integers(0, 4, 32768 + cp.K))
    st = Stream(b.eng, max_reads=len(good) + 1, max_bases=40000, cands_per_read=300, n_slots=2)
    try:
        b.eng.counts_reset()
        with pytest.raises(LmatError) as ei:
            _submit(st, _reads(good[:2]) + [too_long])
        assert ei.value.code == -4 and "read longer than 32787 bases" in str(ei.value)
        assert st.next() is None and b.eng.counts() == NO_TALLIES
        _submit(st, _reads(good[:2]) + [too_long[:-1]])                # the longest read there is: taken
        res, cands, n, _ = _take(st)
        assert len(res) == 3 and int(res["read_len"][2]) == 32787
        assert _text(b.eng, res, cands, _reads(good[:2]) + [too_long[:-1]]) == b.orc.classify(*_blob(_reads(good[:2]) + [too_long[:-1]]), cp.K)[0]
        _submit(st, _reads(good), tag=3)
        _check_batches(b, st, [good], (3,))
    finally:
        st.close()


@pytest.fixture(scope="module")
def gset16(tmp_path_factory):
    return _Set(str(tmp_path_factory.mktemp("ring_modes16")), False)


@pytest.fixture(scope="module")
def gset_wide(tmp_path_factory):
    return _Set(str(tmp_path_factory.mktemp("ring_modes_wide")), True)


def _graded_batch_streamed(gset, mode):
    """All graded probes the mode can take as one streamed batch: the cell of modes x boundary that test_gpu_mode_tiers.py leaves
    out.  Text, tallies, pairs returned and counters as that file holds them for a blocking launch."""
    import os
    from lmat_amd import Stream
    b = _ModeBench(gset, mode)
    try:
        probes = [p for p in b.probes if not b.beyond(p)]
        max_len = max(len(p.read) for p in probes)
        text, tally, nm = b.want(probes)
        st = Stream(b.eng, max_reads=len(probes), max_bases=sum(len(p.read) for p in probes) + 64, cands_per_read=4200, n_slots=2)
        try:
            b.eng.counts_reset()
            _submit(st, _reads(probes))
            res, cands, n, _ = _take(st)
            flow = b.eng.last_counters()
            assert _text(b.eng, res, cands, _reads(probes)) == text
            _assert_tallies(b.eng.counts(), tally, nm, len(probes))
            assert n == b.reserved(probes, text)
            b.check_counters(flow, probes, max_len)
            assert gset.wide or sum(flow.values()) > 0                 # reads did walk down the chain (the wide batch, with a 2068 bp read, starts in its last class)
            assert st.stats()["general"] == 1 and st.stats()["class_lists"] == 1 and st.stats()["grow_reruns"] == 0
        finally:
            st.close()
    finally:
        os.environ["LMAT_DIR"] = gset.lmat_dir
        b.close()


@pytest.mark.parametrize("mode", ["hbias3", "strict", "permissive", "nm"])
def test_graded_probes_streamed_in_a_mode_16bit(gset16, mode):
    assert mode in MODES
    _graded_batch_streamed(gset16, mode)


@pytest.mark.parametrize("mode", ["hbias3", "strict", "permissive", "nm"])
def test_graded_probes_streamed_in_a_mode_wide(gset_wide, mode):
    _graded_batch_streamed(gset_wide, mode)


# ---- 3. submit shapes ------------------------------------------------------------------------------------------------------------
class _Fixture1:
    """The config-1 data set (10 k reads of 75 to 300 bp against a database of about a million k-mers), an engine and an oracle
    on it.  cut(L, n): n reads of exactly L bases -- fixture reads cut to L, or, above 300, consecutive fixture reads joined and
    cut (chimeras: the oracle says what they are)."""

    def __init__(self, outdir):
        import oracle_py
        from lmat_amd import Engine, Params, synth
        info = synth.generate_dataset(outdir, (2, 2, 2, 2, 3, 3), 13400, 10000, L=(75, 100, 125, 150, 200, 250, 300), frac_short=0.01, lower_frac=0.02)
        self.reads = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
        self.eng = Engine(0, Params.run_rl())
        self.eng.load_taxonomy(info["tree"], info["depth"], info["rank"], info["idmap"])
        self.eng.build_db(info["db"], k=20)
        self.orc = oracle_py.Oracle(info["tree"], info["depth"], info["rank"], info["idmap"])
        self.orc.add_taxhisto(info["db"])
        self.orc.set_options()
        self._want = {}

    def cut(self, L, n, start=0):
        out, i = [], start
        while len(out) < n:
            s = ""
            while len(s) < L:
                s += self.reads[i % len(self.reads)]
                i += 1
            out.append(s[:L])
        return out

    def want(self, reads):
        key = hash(tuple(reads))
        if key not in self._want:
            self._want[key] = self.orc.classify(*_blob(reads), 20)
        return self._want[key]

    def check(self, st, reads, submit=None):
        """Submits (the plain copy-in submit unless `submit` does it), takes the batch and holds it against the oracle."""
        text, tally, nm = self.want(reads)
        self.eng.counts_reset()
        (submit or (lambda: _submit(st, reads)))()
        res, cands, n, _ = _take(st)
        assert len(res) == len(reads) and n == int(res["n_cand"].sum())
        assert _text(self.eng, res, cands, reads) == text
        _assert_tallies(self.eng.counts(), tally, nm, len(reads))
        return res, cands

    def close(self):
        self.orc.close()
        self.eng.close()


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    f = _Fixture1(str(tmp_path_factory.mktemp("ring_cfg1")))
    yield f
    f.close()


def _delta(st, before):
    now = st.stats()
    return {k: now[k] - before[k] for k in ("uniform", "general", "threaded", "class_lists", "grow_reruns")}


@pytest.mark.parametrize("length", [19, 20, 150, 179, 180, 275, 276, 339, 340, 531, 532])
def test_equal_lengths_and_one_more(fx, length):
    """At k = 20 the length classes end at 179, 275, 339 and 531 bp (160, 256, 320 and 512 k-mer positions); 19 bp has none and 20
    bp one.  24 reads of one length from offset 0: offsets made on the device.  The same with a read of the same class appended
    (offsets copied in, one class: no lists), and with a read of another class appended (the lists are sent; a 532 bp read rides
    in the last class's list, beyond its 512 positions)."""
    from lmat_amd import Stream
    reads = fx.cut(length, 24, start=length)
    same_class = fx.cut(length - 1, 1, start=7)[0] if length not in (20, 180, 276, 340, 532) else fx.cut(length + 1, 1, start=7)[0]
    other_class = fx.cut(532 if length < 340 else 100, 1, start=11)[0]
    st = Stream(fx.eng, max_reads=32, max_bases=32 * 540, cands_per_read=64, n_slots=2)
    try:
        s0 = st.stats()
        fx.check(st, reads)
        assert _delta(st, s0) == dict(uniform=1, general=0, threaded=0, class_lists=0, grow_reruns=0)
        s0 = st.stats()
        fx.check(st, reads + [same_class])
        assert _delta(st, s0) == dict(uniform=0, general=1, threaded=0, class_lists=0, grow_reruns=0)
        s0 = st.stats()
        fx.check(st, reads[:12] + [other_class] + reads[12:])
        assert _delta(st, s0) == dict(uniform=0, general=1, threaded=0, class_lists=1, grow_reruns=0)
    finally:
        st.close()


def test_offsets_that_do_not_start_at_zero(fx):
    """submit_pinned with reads in the middle of the caller's own pinned buffer (the base offset is subtracted), and the slot's own
    buffers filled from an offset above 0 -- equal lengths too, which must then NOT take the device-made offsets."""
    import ctypes as C
    from lmat_amd import Stream
    from lmat_amd.capi import host_alloc, host_free
    reads = fx.cut(150, 20, start=3) + fx.cut(97, 5, start=50) + fx.cut(301, 3, start=80)
    equal = fx.cut(151, 16, start=200)
    st = Stream(fx.eng, max_reads=32, max_bases=16384, cands_per_read=64, n_slots=2)
    buf = host_alloc(32768)
    try:
        for batch, lead in ((reads, 1237), (equal, 4099), (equal, 0)):
            blob, off = _blob(batch)
            junk = np.frombuffer(("TGCA" * 2000).encode(), dtype=np.uint8)
            C.memmove(buf, junk.ctypes.data, junk.size)
            C.memmove(buf + lead, blob.ctypes.data, int(off[-1]))
            shifted = (off + np.uint64(lead)).astype(np.uint64)
            s0 = st.stats()
            fx.check(st, batch, submit=lambda: st.submit_pinned(buf, shifted, len(batch)))
            d = _delta(st, s0)
            assert d["uniform"] == (1 if batch is equal else 0) and d["uniform"] + d["general"] == 1, (lead, d)   # (the base is subtracted first)

        def acquire_and_fill(batch, lead):
            pb, po = C.c_void_p(), C.c_void_p()
            st.eng._chk(st.lib.lmat_stream_acquire(st.h, C.byref(pb), C.byref(po)))
            blob, off = _blob(batch)
            shifted = (off + np.uint64(lead)).astype(np.uint64)
            C.memmove(pb.value + lead, blob.ctypes.data, int(off[-1]))
            C.memmove(po, shifted.ctypes.data, shifted.size * 8)
            st.eng._chk(st.lib.lmat_stream_submit(st.h, len(batch), 0))
            st.in_flight += 1
        for batch, lead in ((reads, 333), (equal, 2), (equal, 16384 - 16 * 151)):   # the last one ends exactly at max_bases
            s0 = st.stats()
            fx.check(st, batch, submit=lambda: acquire_and_fill(batch, lead))
            assert _delta(st, s0)["general"] == 1, lead
    finally:
        st.close()
        host_free(buf)


def test_batch_sizes_at_the_limits_of_a_stream(fx):
    """No read, one read, max_reads reads; total bases exactly max_bases with every length = 1 mod 32 (each record rounds up the
    most: the worst case of the slot's record-word bound) and the last read ending at an address that is no multiple of 4; empty
    reads between others."""
    from lmat_amd import Stream
    lengths = [33, 65, 97, 129, 161, 193, 225, 257, 289] * 7
    full = [fx.cut(L, 1, start=13 * i)[0] for i, L in enumerate(lengths)]
    total = sum(lengths)
    assert len(full) == 63 and all(L % 32 == 1 for L in lengths) and total % 4 != 0
    st = Stream(fx.eng, max_reads=63, max_bases=total, cands_per_read=64, n_slots=2)
    try:
        st.submit(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64), tag=9)
        res, cands, n, tag = _take(st)
        assert (len(res), cands, n, tag) == (0, None, 0, 9) and st.stats()["uniform"] + st.stats()["general"] == 0
        fx.check(st, full)                                              # max_reads reads, max_bases bases
        fx.check(st, full[:1])
        gaps = [full[0], "", full[1], "", "", full[2][:19], "", full[3]]
        fx.check(st, gaps)
        fx.check(st, ["", ""])
        assert st.stats()["grow_reruns"] == 0
    finally:
        st.close()


def test_a_small_batch_after_a_large_one_in_the_same_slot(fx):
    """One slot: the small batch finds the large one's bases, offsets, class lists, results and candidates still in the slot's
    buffers.  Mixed lengths (lists sent), then equal lengths (nothing but the bases sent)."""
    from lmat_amd import Stream
    large = fx.reads[:3000]
    st = Stream(fx.eng, max_reads=3000, max_bases=sum(len(r) for r in large) + 64, cands_per_read=64, n_slots=1)
    try:
        fx.check(st, large)
        fx.check(st, fx.reads[3000:3037])
        fx.check(st, large[::-1])
        fx.check(st, fx.cut(150, 9, start=4000))
        stats = st.stats()
        assert stats["general"] == 3 and stats["class_lists"] == 3 and stats["uniform"] == 1 and stats["grow_reruns"] == 0
    finally:
        st.close()


def test_a_batch_above_2_to_the_18_reads(fx):
    """2^18 + 1000 reads of mixed lengths -- 1031 fixture reads, tiled --: the partition runs on four host threads, the class lists
    are sent, and (above 128 K reads with a candidate buffer) the pairs are handed out through sub-cursors in the slot's own
    buffer.  The distinct reads are held against the oracle in a batch of their own; every tile must repeat their records and
    candidate lists, and the tallies are the oracle's taken once for every copy."""
    from lmat_amd import Stream
    distinct = fx.reads[5000:6031]
    n = (1 << 18) + 1000
    index = np.arange(n) % len(distinct)
    text, tally, nm = fx.want(distinct)
    blob1, off1 = _blob(distinct)
    lens = np.diff(off1).astype(np.int64)
    st = Stream(fx.eng, max_reads=n, max_bases=int(lens[index].sum()) + 64, cands_per_read=64, n_slots=1)
    try:
        one, c1 = fx.check(st, distinct)
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens[index], out=off[1:])
        base = blob1[:int(off1[-1])]
        reps, rest = divmod(n, len(distinct))
        blob = np.concatenate([np.tile(base, reps), base[:int(off1[rest])]])
        assert blob.size == int(off[-1])
        s0 = st.stats()
        fx.eng.counts_reset()
        st.submit(blob, off, tag=5)
        res, cands, nc, tag = _take(st)
        assert _delta(st, s0) == dict(uniform=0, general=1, threaded=1, class_lists=1, grow_reruns=0)
        assert tag == 5 and len(res) == n and nc >= int(res["n_cand"].sum())
        want = one[index]
        for f in ("read_len", "n_cand"):
            assert (res[f] == want[f]).all(), f
        _same_records(res, want)
        # the candidate lists: read i's pairs are those of distinct read i mod 1031, wherever its chunk put them
        ncand = res["n_cand"].astype(np.int64)
        assert int((res["cand_off"].astype(np.int64) + ncand).max()) <= nc
        flat_got = np.repeat(res["cand_off"].astype(np.int64) - np.concatenate([[0], np.cumsum(ncand)[:-1]]), ncand) + np.arange(int(ncand.sum()))
        flat_want = np.repeat(want["cand_off"].astype(np.int64) - np.concatenate([[0], np.cumsum(ncand)[:-1]]), ncand) + np.arange(int(ncand.sum()))
        assert (cands["tid"][flat_got] == c1["tid"][flat_want]).all()
        assert (cands["score"][flat_got].view(np.uint32) == c1["score"][flat_want].view(np.uint32)).all()
        # pairs of different reads do not overlap
        has = ncand > 0
        order = np.argsort(res["cand_off"][has], kind="stable")
        o, c = res["cand_off"][has].astype(np.int64)[order], ncand[has][order]
        assert (o[1:] >= o[:-1] + c[:-1]).all()
        # tallies: the oracle's of the distinct reads, once per copy
        copies = np.bincount(index, minlength=len(distinct))
        per_read = [fx.want([r]) for r in distinct[:rest]] if rest else []
        whole = {t: (c * reps, s * reps) for t, (c, s) in tally.items()}
        t_all, nm_all = _sum_tallies([(whole, [int(x) * reps for x in nm])] + [w[1:] for w in per_read])
        assert copies.max() - copies.min() <= 1
        _assert_tallies(fx.eng.counts(), t_all, nm_all, n)
    finally:
        st.close()
