"""GPU: paired-end reads joined in the pack step (pack_pairs_kernel, pairs.hip).  The record of a pair is word
for word the record the existing kernel writes for  mate1 + b"N" + mate2,  so the reference throughout is the existing single-read
path on the joined bytes: pack_ref of the joined text for records, Engine.upload_reads / Stream.submit of it for result records
and candidates (bit for bit), the CPU oracle's text of its image for formatted output."""
import ctypes

import numpy as np
import pytest

from test_gpu_pack import _blob, _image, _mixed, _oracle_text, pack_ref

pytestmark = pytest.mark.gpu

MAX_LEN = 32768 + 20 - 1          # the longest read the classify chain takes at k = 20
L2_GRID = (0, 1, 2, 3, 14, 15, 16, 17, 31, 32, 33, 70)
# byte values that are no base: at and above 0x80, below 0x20, and those a wrong mask turns into a letter (0xC1 & 0x7F = 'A',
# 0x01 | 0x40 = 'A', 0x21 | 0x40 = 'a', 0xD4 & 0x7F = 'T' ...)
TRAPS = (0xC1, 0xC3, 0xC7, 0xD4, 0xE1, 0xF4, 0x01, 0x03, 0x07, 0x14, 0x21, 0x23, 0x27, 0x34, 0x00, 0xFF, 0x80, 0x0A, 0x1F)


def _letters(rng, n):
    return np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, n)].tobytes()


def _hostile(rng, n):
    """Letters of either case with N and the trap bytes in a quarter of the positions."""
    r = np.frombuffer(_letters(rng, n), dtype=np.uint8).copy()
    hit = rng.random(n) < 0.25
    pool = np.array(TRAPS + (ord("N"), ord("n")), dtype=np.uint8)
    r[hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
    return r.tobytes()


def _mate(rng, n, i):
    return _hostile(rng, n) if i % 3 == 0 else _letters(rng, n)


def _joined(pairs):
    return [a + b"N" + b for a, b in pairs]


def _blocks(pairs):
    """(blob1, off1), (blob2, off2): the mates of each file end to end, each block ending with its last base."""
    return _blob([a for a, _ in pairs]), _blob([b for _, b in pairs])


def _interleaved(pairs):
    return _blob([m for p in pairs for m in p])


def _check_pairs(eng, pairs, index=None):
    """Uploads the pairs and compares records, record offsets and the decoded image with those of the joined text.  index: the
    pairs are distinct[index[i]] (a tiled batch: the reference packs the distinct pairs once)."""
    distinct = pairs
    if index is not None:
        pairs = [distinct[i] for i in index]
    recs = [pack_ref(j) for j in _joined(distinct)]
    want = np.concatenate([recs[i] for i in (index if index is not None else range(len(pairs)))]) if pairs else np.zeros(0, np.uint32)
    m1, m2 = _blocks(pairs)
    dr = eng.upload_read_pairs(m1, m2)
    try:
        assert len(dr) == len(pairs)
        words, rec_off = dr.words()
        lens = np.array([len(a) + 1 + len(b) for a, b in pairs], dtype=np.int64)
        assert (rec_off == np.concatenate([[0], np.cumsum(1 + (lens + 15) // 16 + (lens + 31) // 32)])).all()
        assert words.size == want.size
        bad = np.nonzero(words != want)[0]
        if bad.size:
            r = int(np.searchsorted(rec_off, bad[0], side="right")) - 1
            a2 = (int(m1[1][-1]) + int(m2[1][r])) % 4
            raise AssertionError("pair %d (%d + %d bases, mates start at %d and %d mod 4), word %d of its record: %08x, expected %08x; %d words differ"
                                 % (r, len(pairs[r][0]), len(pairs[r][1]), int(m1[1][r]) % 4, a2, bad[0] - int(rec_off[r]), words[bad[0]], want[bad[0]], bad.size))
        got, goff = dr.ascii()
        assert (np.diff(goff.astype(np.int64)) == lens).all() and got.tobytes() == b"".join(_image(_joined(pairs)))
    finally:
        dr.free()


@pytest.fixture(scope="module")
def eng(small_dataset):
    from lmat_amd import Engine, Params
    ds = small_dataset
    e = Engine(0, Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    e.build_db(ds["db"], k=20)
    yield e
    e.close()


def _aligned(shapes, rng):
    """The pairs of `shapes` (l1, l2), each at every combination of start addresses mod 4 of its two mates: a filler pair of 0..3 +
    0..3 bases in front of each sets both, as _length_grid's filler reads do for one.  The mates of a file lie end to end and the
    second file's block lies behind the first's on the device, so the first block is closed with a filler that makes it a multiple
    of 4: mate 2 then starts at its own offset mod 4.  -> pairs, the set of (a1, a2, l1, l2) placed."""
    pairs, seen, t1, t2, i = [], set(), 0, 0, 0
    for a1 in range(4):
        for a2 in range(4):
            for l1, l2 in shapes:
                f1, f2 = (a1 - t1) % 4, (a2 - t2) % 4
                pairs.append((_mate(rng, f1, i + 1), _mate(rng, f2, i + 2)))
                t1, t2 = t1 + f1, t2 + f2
                seen.add((t1 % 4, t2 % 4, l1, l2))
                pairs.append((_mate(rng, l1, i), _mate(rng, l2, i + 1)))
                t1, t2, i = t1 + l1, t2 + l2, i + 1
    pairs.append((_letters(rng, (-t1) % 4), b""))
    return pairs, seen


def test_the_joint_at_every_position_and_both_alignments(eng):
    """l1 = 0..48 puts the joint at every position of a code word and on both sides of a validity word; l2 ends the pair inside the
    joint's word, at its end and in later words; both mates start at every address mod 4 independently.  A third of the mates
    carry N and byte values that are no base.  Mate 1 is followed in its buffer by the next mate 1 -- letters --, the last one by
    the first mate 2: whatever leaks across a mate's end shows in the comparison."""
    rng = np.random.default_rng(201)
    shapes = [(l1, l2) for l1 in range(49) for l2 in L2_GRID]
    pairs, seen = _aligned(shapes, rng)
    assert seen == {(a1, a2, l1, l2) for a1 in range(4) for a2 in range(4) for l1, l2 in shapes}
    every = b"".join(a + b for a, b in pairs)
    assert every.count(b"N") > 100 and all(bytes([t]) in every for t in TRAPS)
    assert sum(len(a) for a, _ in pairs) % 4 == 0
    _check_pairs(eng, pairs)


EDGE_SHAPES = ([(5, 3), (0, 0), (0, 17), (17, 0), (0, 1), (1, 0)] +
               [(7, 8), (0, 15), (15, 0), (16, 15), (31, 0), (0, 31), (15, 16), (128, 127), (255, 0), (0, 255), (250, 5)] +   # joined 16, 32, 256
               [(l1, 40) for l1 in (254, 255, 256, 257)] + [(40, l2) for l2 in (214, 215, 216, 217)])


def test_pairs_that_end_in_the_joints_word_and_the_outer_loop(eng):
    """The pair ends inside the word that holds the joint (5 + 3); joined lengths of exactly 16, 32 and 256; an empty mate 1, an
    empty mate 2, both (the one-base record of "N"); the joint on either side of the 256-position step of the outer loop, and a
    pair that ends there.  Each at all 16 start alignments."""
    rng = np.random.default_rng(202)
    pairs, seen = _aligned(EDGE_SHAPES, rng)
    assert len(seen) == 16 * len(EDGE_SHAPES)
    assert {len(a) + 1 + len(b) for a, b in pairs} >= {1, 9, 16, 32, 256}
    _check_pairs(eng, pairs)


def test_neighbour_bytes_behind_a_mate_are_letters(eng):
    """Mates of N only between mates of letters: a dword that holds a mate's last bases holds its neighbour's first letters; the
    records of the N mates have no valid bit anywhere, and the letters' records none past their end."""
    rng = np.random.default_rng(203)
    pairs = []
    for l1 in range(1, 20):
        pairs.append((b"N" * l1, _letters(rng, 23)))
        pairs.append((_letters(rng, 21), b"N" * (l1 % 7)))
    _check_pairs(eng, pairs)


@pytest.fixture(scope="module")
def longest(eng):
    rng = np.random.default_rng(204)
    return _mixed(rng, 20000), _mixed(rng, MAX_LEN - 20001 + 1)    # (one base more than fits; cut below)


def test_the_longest_pair_and_one_base_more(eng, longest):
    """20 000 + 1 + 12 786 = 32 787 joined bases, the longest read there is: packed, and classified like the joined read.  One base
    more: the same error from the same call as a single read of 32 788 bases -- lmat_classify for an upload, submit for a stream."""
    from lmat_amd import Stream
    from lmat_amd.capi import LmatError
    m1, m2 = longest
    fits, over = (m1, m2[:-1]), (m1, m2)
    assert len(_joined([fits])[0]) == MAX_LEN and len(_joined([over])[0]) == MAX_LEN + 1
    _check_pairs(eng, [(b"ACG", b"T"), fits, (b"", b"GG")])
    single = eng.upload_reads(_blob(_joined([fits])))
    paired = eng.upload_read_pairs(*_blocks([fits]))
    a, b = eng.classify(single), eng.classify(paired)
    _same_calls(b, a, "the longest pair")
    assert int(b[0]["read_len"][0]) == MAX_LEN
    single.free(), paired.free()
    errs = []
    for dr in (eng.upload_reads(_blob(_joined([over]))), eng.upload_read_pairs(*_blocks([over]))):
        with pytest.raises(LmatError) as ei:
            eng.classify(dr)
        errs.append((ei.value.code, str(ei.value)))
        dr.free()
    assert errs[0] == errs[1] and errs[0][0] == -4 and "read longer than 32787 bases" in errs[0][1]
    st = Stream(eng, max_reads=4, max_bases=40000, cands_per_read=8, n_slots=1)
    try:
        errs = []
        for submit, batch in ((st.submit, _blob(_joined([over]))), (st.submit_pairs, _interleaved([over]))):
            with pytest.raises(LmatError) as ei:
                submit(*batch)
            errs.append((ei.value.code, str(ei.value)))
            assert st.next() is None
        assert errs[0] == errs[1] and errs[0][0] == -4 and "read longer than 32787 bases" in errs[0][1]
        st.submit_pairs(*_interleaved([fits]))                       # the slot went back untouched
        res, cands, _ = st.next()
        _same_calls((res, cands), a, "the longest pair through a stream")
    finally:
        st.close()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 17])
def test_pair_counts_around_a_wave_of_four(eng, n):
    rng = np.random.default_rng(210 + n)
    _check_pairs(eng, [(_mate(rng, int(a), i), _mate(rng, int(b), i + 1)) for i, (a, b) in enumerate(rng.integers(0, 60, (n, 2)))])


def test_a_grid_stride_pass(eng):
    """The grid is capped at 16384 blocks of four waves, four pairs a wave and pass: 4 * 65536 + 1 pairs make the first wave go round
    once more.  257 distinct short pairs, tiled."""
    rng = np.random.default_rng(220)
    distinct = [(_mate(rng, int(a), i), _mate(rng, int(b), i + 2)) for i, (a, b) in enumerate(rng.integers(0, 21, (257, 2)))]
    _check_pairs(eng, distinct, index=np.arange(4 * 65536 + 1) % 257)


def _same_calls(got, want, what=""):
    """Result records and candidates of two runs of the same reads, bit for bit: every field of every record and every read's
    candidate pairs as raw bytes.  (Where a read's pairs lie in the candidate buffer -- cand_off -- is the order in which the
    waves of a launch took their room, which two launches of the same single reads do not share either.)"""
    (res, cands), (res1, cands1) = got, want
    assert res.dtype == res1.dtype and res.shape == res1.shape, what
    for f in res.dtype.names:
        if f != "cand_off":
            assert res[f].tobytes() == res1[f].tobytes(), (what, f)
    if res["n_cand"].any():   # (a stream hands out no candidate array when a batch printed none; the blocking call its whole buffer)
        for i in np.nonzero(res["n_cand"])[0]:
            a, b, n = int(res["cand_off"][i]), int(res1["cand_off"][i]), int(res["n_cand"][i])
            assert cands[a:a + n].tobytes() == cands1[b:b + n].tobytes(), (what, int(i))


def _odd_end(batch):
    """The batch, closed with one-base pairs until its bytes end at an address that is no multiple of 4."""
    batch = list(batch)
    while sum(len(a) + len(b) for a, b in batch) % 4 == 0:
        batch.append((b"A", b""))
    return batch


# ---- classification ---------------------------------------------------------------------------------------------------------------
def _fixture_pairs(ds, rng, n=64):
    """Pairs cut from fixture reads (they hit the database): 75 + 75 bases, mixed lengths, and a few with one mate of random bases."""
    src = [r.encode() for r in ds["reads"] if len(r) >= 150]
    out = []
    for i in range(n):
        r = src[i % len(src)]
        if i % 3 == 0:
            p = (r[:75], r[75:150])
        else:
            p = (r[:40 + (i * 11) % 61], r[150 - 30 - (i * 7) % 71:150])
        if i % 16 == 5:
            p = (_letters(rng, len(p[0])).upper(), p[1])
        if i % 16 == 11:
            p = (p[0], _letters(rng, len(p[1])).upper())
        out.append(p)
    return out


def test_classification_equals_the_joined_reads(eng, small_dataset, oracle_small):
    rng = np.random.default_rng(230)
    pairs = _fixture_pairs(small_dataset, rng)
    assert len(pairs) == 64 and len({(len(a), len(b)) for a, b in pairs}) > 20
    paired = eng.upload_read_pairs(*_blocks(pairs))
    single = eng.upload_reads(_blob(_joined(pairs)))
    try:
        res, cands = eng.classify(paired)
        _same_calls((res, cands), eng.classify(single))
        want, image = _oracle_text(oracle_small, _joined(pairs))
        assert eng.format_out(res, cands, image) == want
        assert (res["status"] == 0).sum() > len(pairs) // 2
    finally:
        paired.free(), single.free()


# ---- the streamed boundary --------------------------------------------------------------------------------------------------------
class _Pinned:
    """Bytes in page-locked memory of the caller's own (lmat_host_alloc)."""

    def __init__(self, data):
        from lmat_amd import capi
        self.capi, self.addr = capi, capi.host_alloc(len(data) + 16)
        ctypes.memmove(self.addr, data, len(data))

    def free(self):
        self.capi.host_free(self.addr)


def _edge_pairs(rng):
    return [(_mate(rng, l1, i), _mate(rng, l2, i + 1)) for i, (l1, l2) in enumerate(EDGE_SHAPES)]


def test_pairs_through_a_stream(eng, small_dataset, oracle_small):
    """A one-slot Stream whose device buffer holds a full batch of letters from before each paired batch: mixed lengths (offsets
    copied in: `general`), fixed l1 and l2 (offsets made on the device: `uniform`), two pinned blocks whose offsets do not start
    at 0, and the edge pairs of the record tests.  Each batch ends at an address that is no multiple of 4.  The oracle's text of
    the joined image, and read_len the joined lengths."""
    from lmat_amd import Stream
    rng = np.random.default_rng(240)
    ds = small_dataset
    full = [r[:150].encode() for r in ds["reads"] if len(r) >= 150][:64]
    cap = sum(len(r) for r in full)
    mixed = _odd_end(_fixture_pairs(ds, rng, 56))
    src = [r.encode() for r in ds["reads"] if len(r) >= 150]
    fixed = [(src[i][:74], src[i][80:149]) for i in range(33)]
    edges = _odd_end(_edge_pairs(rng))
    st = Stream(eng, max_reads=128, max_bases=cap, cands_per_read=64, n_slots=1)
    pins = []
    try:
        for kind, batch, branch in (("slot", mixed, "general"), ("slot", fixed, "uniform"), ("pinned", _odd_end(mixed[3:40]), "general"),
                                    ("pinned0", fixed, "uniform"), ("slot", edges, "general")):
            total = sum(len(a) + len(b) for a, b in batch)
            assert total % 4 and total + len(batch) < cap - 64
            st.submit(*_blob(full))                                  # letters up to the slot's end
            assert st.next_nocopy()[0] == len(full)
            before = st.stats()
            if kind == "slot":
                st.submit_pairs(*_interleaved(batch), tag=7)
            else:
                lead = (b"ACGTA", b"TTGCATG") if kind == "pinned" else (b"", b"")   # bases in front of the batch: offsets from 5 and 7
                (b1, o1), (b2, o2) = _blocks(batch)
                p1, p2 = _Pinned(lead[0] + b1.tobytes() + b"ACGT" * 4), _Pinned(lead[1] + b2.tobytes() + b"ACGT" * 4)
                pins += [p1, p2]
                o1, o2 = o1 + np.uint64(len(lead[0])), o2 + np.uint64(len(lead[1]))
                st.submit_pairs_pinned(p1.addr, o1, p2.addr, o2, len(batch), tag=7)
            res, cands, tag = st.next()
            after = st.stats()
            assert tag == 7 and len(res) == len(batch)
            assert after[branch] == before[branch] + 1 and after["uniform"] + after["general"] == before["uniform"] + before["general"] + 1
            want, image = _oracle_text(oracle_small, _joined(batch))
            assert eng.format_out(res, cands, image) == want
            assert (res["read_len"] == [len(a) + 1 + len(b) for a, b in batch]).all()
            assert batch is edges or (res["status"] == 0).sum() > len(batch) // 2      # the pairs do hit: the records say something
        assert st.stats()["grow_reruns"] == 0
    finally:
        st.close()
        for p in pins:
            p.free()


def test_fixed_geometry_pairs_take_the_uniform_kernel(small_dataset):
    """74 + 75-base pairs are joined reads of 150 bases: under the run conditions of test_gpu_uniform_variant.py (calls only, no
    -p) the launch runs the fixed-geometry kernel, which meets an N at position 74 of every read.  The records of the joined
    single-read run."""
    from lmat_amd import Engine, Params, Stream
    ds = small_dataset
    e = Engine(0, Params.run_rl(prn_all=0))
    try:
        e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
        e.build_db(ds["db"], k=20)
        src = [r.encode() for r in ds["reads"] if len(r) >= 150][:200]
        pairs = [(r[:74], r[75:150]) for r in src]
        st = Stream(e, 512, 512 * 160, 0, n_slots=1)
        try:
            before = e.uniform_launches()
            st.submit(*_blob(_joined(pairs)))
            want = st.next()[0]
            assert e.uniform_launches() == before + 1                # the conditions hold: the single-read run took the variant
            stats = st.stats()
            st.submit_pairs(*_interleaved(pairs))
            got = st.next()[0]
            assert e.uniform_launches() == before + 2 and st.stats()["uniform"] == stats["uniform"] + 1
            assert got.tobytes() == want.tobytes()
            assert (got["read_len"] == 150).all() and (got["status"] == 0).sum() > len(pairs) // 2
        finally:
            st.close()
    finally:
        e.close()


def test_a_paired_batch_counts_two_reads_and_a_base_per_pair(eng, small_dataset):
    """2 n_pairs = max_reads is accepted and max_reads + 2 refused; sum(l1 + l2) + n_pairs = max_bases is accepted and one base
    more refused; LMAT_E_ARG, and after each refusal the next acquire / submit works."""
    from lmat_amd import Stream
    from lmat_amd.capi import LmatError
    src = [r.encode() for r in small_dataset["reads"] if len(r) >= 150]
    pairs = [(src[i][:70 + i], src[i][75:150]) for i in range(5)]
    four = pairs[:4]
    total = sum(len(a) + len(b) for a, b in four)
    single = eng.upload_reads(_blob(_joined(four)))
    want = eng.classify(single)
    single.free()
    pins = []

    def pinned(st, batch):
        (b1, o1), (b2, o2) = _blocks(batch)
        pins.extend([_Pinned(b1.tobytes() + b"\0" * 8), _Pinned(b2.tobytes() + b"\0" * 8)])
        st.submit_pairs_pinned(pins[-2].addr, o1, pins[-1].addr, o2, len(batch))

    try:
        for submit in (lambda st, batch: st.submit_pairs(*_interleaved(batch)), pinned):
            st = Stream(eng, max_reads=8, max_bases=total + 4, cands_per_read=64, n_slots=1)
            try:
                for refused in (pairs, [(four[0][0] + b"A", four[0][1])] + four[1:]):   # a pair too many; a base too many
                    with pytest.raises(LmatError) as ei:
                        submit(st, refused)
                    assert ei.value.code == -1 and "larger than the stream was created for" in str(ei.value)
                    assert st.next() is None
                    submit(st, four)                                 # exactly at both limits
                    _same_calls(st.next()[:2], want)
                with pytest.raises(ValueError):                      # an odd number of reads is no interleaved batch: no slot is taken
                    st.submit_pairs(*_blob([a for a, _ in four[:3]]))
                submit(st, four)
                _same_calls(st.next()[:2], want)
            finally:
                st.close()
    finally:
        for p in pins:
            p.free()


def test_a_paired_batch_that_grows_its_slot(eng, small_dataset):
    """cands_per_read = 1: a tiled batch of pairs prints more candidates than the slot holds, the slot grows and the batch runs
    again from its resident records.  The results are those of the joined single-read batch through a slot that is large enough,
    and the tallies are counted once."""
    from lmat_amd import Stream
    rng = np.random.default_rng(250)
    distinct = _fixture_pairs(small_dataset, rng, 64)
    probe = eng.upload_read_pairs(*_blocks(distinct))
    per_tile = int(eng.classify(probe)[0]["n_cand"].sum())
    probe.free()
    assert per_tile > 4 * 64
    slack = 1024 * 2048                                               # pairs a slot holds beyond cands_per_read * max_reads
    tiles = slack // (per_tile - 128) + 2                             # tiles * per_tile > slack + 1 * (2 * 64 * tiles): beyond the slot
    pairs = distinct * tiles
    n, bases = len(pairs), sum(len(a) + len(b) + 1 for a, b in pairs)
    eng.counts_reset()
    st = Stream(eng, max_reads=n, max_bases=bases, cands_per_read=per_tile // 64 + 1, n_slots=1)
    st.submit(*_blob(_joined(pairs)))
    want, want_cands, _ = st.next()
    assert st.stats()["grow_reruns"] == 0
    st.close()
    eng.sync()
    want_tallies = eng.counts()
    eng.counts_reset()
    st = Stream(eng, max_reads=2 * n, max_bases=bases, cands_per_read=1, n_slots=1)
    try:
        st.submit_pairs(*_interleaved(pairs))
        res, cands, _ = st.next()
        assert st.stats()["grow_reruns"] == 1
        assert int(res["n_cand"].sum()) == tiles * per_tile > 2 * n + slack      # (more than the slot held; the buffer's own count includes what the sub-cursors left unused)
        _same_calls((res, cands), (want, want_cands), "after the grow re-run")
        eng.sync()
        (counts, nomatch), (counts1, nomatch1) = eng.counts(), want_tallies
        assert list(nomatch) == list(nomatch1) and {t: c for t, (c, _) in counts.items()} == {t: c for t, (c, _) in counts1.items()}
        for t, (_, s) in counts1.items():   # the same n scores added in double in another order: each addition within 2^-53 of the running sum
            assert abs(counts[t][1] - s) <= n * 2.0 ** -52 * max(abs(s), 1.0), t
    finally:
        st.close()
