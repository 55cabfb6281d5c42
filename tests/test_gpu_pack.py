"""GPU: the ASCII-to-record pack kernel (K0, pack_reads_kernel) against a numpy packer written from the layout comment in
lmat_common.hpp, word for word -- padding bits included: the record is what every later kernel reads in whole tiles, and the
layout says what a word holds, not only what its first `len` positions hold.  Every byte value at every position of a code word in
reads that start at every address mod 4, every length mod 32 at every start alignment, the lengths around the 256-base loop, one
grid-stride pass, and -- through a one-slot Stream whose device buffers hold the letters of an earlier batch -- the records the
classify kernels make of the same bytes, against the CPU oracle.  The synthetic reads the benchmark classifies are records written
directly by synth_reads_kernel: they must be the records the pack kernel makes of their own ASCII."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CODE = np.zeros(256, dtype=np.uint64)
_VALID = np.zeros(256, dtype=np.uint64)
for _c, _ch in enumerate(b"ACGT"):
    _CODE[[_ch, _ch | 0x20]] = _c
    _VALID[[_ch, _ch | 0x20]] = 1
_IMAGE = np.full(256, ord("N"), dtype=np.uint8)
for _ch in b"ACGT":
    _IMAGE[[_ch, _ch | 0x20]] = _ch


def pack_ref(read):
    """[len], then ceil(len / 16) words of 2-bit codes (base j at bits 2 * (j mod 16), 0 for anything but ACGTacgt), then
    ceil(len / 32) words of validity bits (bit j mod 32); every bit past the read's end is zero."""
    a = np.frombuffer(read, dtype=np.uint8)
    nb, nv = (a.size + 15) // 16, (a.size + 31) // 32
    code, valid = np.zeros(nb * 16, dtype=np.uint64), np.zeros(nv * 32, dtype=np.uint64)
    code[:a.size], valid[:a.size] = _CODE[a], _VALID[a]
    cw = (code.reshape(nb, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1)
    vw = (valid.reshape(nv, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return np.concatenate([np.array([a.size], dtype=np.uint64), cw, vw]).astype(np.uint32)


def _blob(reads, pad=False):
    """The reads end to end; without `pad` the last read ends the buffer (a spare byte only where there is no base at all)."""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    if reads:
        np.cumsum([len(r) for r in reads], out=off[1:])
    raw = b"".join(reads)
    return np.frombuffer(raw + (b"\0" if pad or not raw else b""), dtype=np.uint8), off


def _image(reads):
    return [_IMAGE[np.frombuffer(r, dtype=np.uint8)].tobytes() for r in reads]


def _check_pack(eng, reads, index=None):
    """Uploads the reads and compares records, record offsets and the decoded image.  index: the reads are distinct[index[i]]
    (a tiled batch: the reference packs the distinct reads once)."""
    distinct = reads
    if index is not None:
        reads = [distinct[i] for i in index]
    recs = [pack_ref(r) for r in distinct]
    want = np.concatenate([recs[i] for i in (index if index is not None else range(len(reads)))]) if reads else np.zeros(0, np.uint32)
    blob, off = _blob(reads)
    assert blob.size == max(int(off[-1]), 1)               # the last read ends the buffer
    dr = eng.upload_reads((blob, off))
    try:
        words, rec_off = dr.words()
        lens = np.diff(off).astype(np.int64)
        assert (rec_off == np.concatenate([[0], np.cumsum(1 + (lens + 15) // 16 + (lens + 31) // 32)])).all()
        assert words.size == want.size
        bad = np.nonzero(words != want)[0]
        if bad.size:
            r = int(np.searchsorted(rec_off, bad[0], side="right")) - 1
            raise AssertionError("read %d (len %d, starts at %d mod 4), word %d of its record: %08x, expected %08x; %d words differ"
                                 % (r, lens[r], int(off[r]) % 4, bad[0] - int(rec_off[r]), words[bad[0]], want[bad[0]], bad.size))
        got, goff = dr.ascii()
        assert (goff == off).all() and got.tobytes() == b"".join(_image(reads))
    finally:
        dr.free()
    return off


@pytest.fixture(scope="module")
def eng(small_dataset):
    from lmat_amd import Engine, Params
    ds = small_dataset
    e = Engine(0, Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    e.build_db(ds["db"], k=20)
    yield e
    e.close()


def _byte_grid():
    rng = np.random.default_rng(101)
    letters = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    reads = []
    for a in range(4):
        reads.append(b"G")
        for v in range(256):
            for j in range(16):
                r = letters[rng.integers(0, 8, 36)].copy()
                r[16 + j] = v
                reads.append(r.tobytes())
    return reads


def test_every_byte_value_at_every_position_and_alignment(eng):
    """256 byte values x 16 positions of a code word x 4 start addresses mod 4: a 36-base read of letters with the one byte at
    position 16 + j (so that both neighbours of the byte's dword are letters), the four groups separated by a one-base read that
    moves the alignment on.  Bytes at and above 0x80, control bytes, and the bytes that turn into a letter when the wrong bits are
    masked (0xC1 under & 0x7F, 0x01 and 0x21 under | 0x40 ...) are all among them."""
    reads = _byte_grid()
    off = _check_pack(eng, reads)
    starts = {(int(off[i]) % 4) for i in range(len(reads)) if len(reads[i]) == 36}
    assert starts == {0, 1, 2, 3} and len(reads) == 4 * 4097


def _mixed(rng, n):
    """n bytes: mostly letters of either case, N, and a sprinkling of every other byte value."""
    pool = np.frombuffer(b"ACGTacgtACGTacgtN", dtype=np.uint8)
    r = pool[rng.integers(0, pool.size, n)].copy()
    hostile = rng.random(n) < 0.05
    r[hostile] = rng.integers(0, 256, int(hostile.sum()), dtype=np.uint8)
    return r.tobytes()


SPECIAL_LENGTHS = (255, 256, 257, 271, 272, 273, 511, 512, 513, 4095, 4096, 4097)


def _length_grid():
    rng = np.random.default_rng(102)
    max_len = 32768 + 20 - 1                               # the longest read the classify chain takes at k = 20
    reads, total, seen = [], 0, set()
    for a in range(4):
        for L in list(range(71)) + list(SPECIAL_LENGTHS) + [max_len]:
            fill = (a - total) % 4
            reads.append(_mixed(rng, fill))
            total += fill
            seen.add((total % 4, L % 32))
            reads.append(_mixed(rng, L))
            total += L
    return reads, seen


def test_every_length_at_every_alignment(eng):
    """Lengths 0..70 (every length mod 32, an empty read and reads shorter than a dword among them), the lengths around the
    256-base step of the outer loop and around 4096, and one read of the 32 787-base maximum, each starting at every address mod
    4: a filler read of 0..3 bases in front of each sets the alignment."""
    reads, seen = _length_grid()
    assert seen == {(a, m) for a in range(4) for m in range(32)}
    _check_pack(eng, reads)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 17])
def test_read_counts_around_a_wave_of_four(eng, n):
    """A wave packs four reads a pass: 1 to 5 reads (idle quarters of a wave, and a second wave), and none at all."""
    rng = np.random.default_rng(103 + n)
    _check_pack(eng, [_mixed(rng, int(L)) for L in rng.integers(1, 90, n)])


def test_a_grid_stride_pass(eng):
    """The grid is capped at 16384 blocks of four waves, four reads a wave and pass: 4 * 65536 + 1 reads make the first wave go
    round once more.  257 distinct short reads, tiled (257 is coprime to every power of two: each distinct read meets every lane
    quarter and alignment)."""
    rng = np.random.default_rng(104)
    distinct = [_mixed(rng, int(L)) for L in rng.integers(0, 41, 257)]
    n = 4 * 65536 + 1
    _check_pack(eng, distinct, index=np.arange(n) % 257)


def _oracle_text(orc, reads):
    blob, off = _blob(_image(reads), pad=True)
    return orc.classify(blob, off, 20)[0], (blob, off)


def _hostile_reads(ds, rng, n, length=None):
    """Reads of the dataset (they hit the database) with a few bytes replaced by other byte values -- N-like as far as the layout
    goes -- and, without `length`, cut to lengths of every residue."""
    out = []
    src = [r for r in ds["reads"] if len(r) >= 150]
    for i in range(n):
        r = np.frombuffer(src[i % len(src)][:150].encode(), dtype=np.uint8).copy()
        if i % 3:
            at = rng.integers(0, 150, 3)
            r[at] = rng.integers(0, 256, 3, dtype=np.uint8)
        out.append(r[:length if length is not None else 150 - (i % 97)].tobytes())
    return out


def test_the_same_bytes_through_a_stream(eng, small_dataset, oracle_small):
    """A one-slot Stream: its device buffers are never cleared, so behind the last base of a batch lie the bases of the batch
    before -- here a batch of letters that fills the slot.  The records must be those the oracle has for the ACGT-or-N image of
    the bytes.  Two kinds of batches go through: (1) batches made for the stream -- fixture reads, which hit the database, with a
    few bytes replaced by other byte values: mixed lengths (offsets copied in), equal lengths (offsets made on the device: the
    `uniform` branch) and reads of 0..3 and 255..257 bases among ordinary ones, each batch ending at an address that is no
    multiple of 4; (2) the very batches of the two grid tests above -- random bytes, so they hit nothing: their records say how
    many valid k-mers the classify kernels saw (none in a 36-base read at -j 30; the 32 787-base read runs in the last class),
    which is what the stream's own copy of the bytes has to get right."""
    from lmat_amd import Stream
    rng = np.random.default_rng(105)
    ds = small_dataset
    full = [r[:150].encode() for r in ds["reads"] if len(r) >= 150][:64]
    mixed = _hostile_reads(ds, rng, 62)
    equal = _hostile_reads(ds, rng, 33, length=149)
    long_ = (_hostile_reads(ds, rng, 2)[0] * 2)[:257]
    edges = [mixed[0], b"", long_[:1], long_[:255], long_[:2], mixed[1], long_[:3], long_[:256], long_, mixed[2][:149]]
    cap = sum(len(r) for r in full)
    assert all(sum(len(r) for r in b) % 4 and sum(len(r) for r in b) < cap - 64 for b in (mixed, equal, edges))
    assert any(b >= 0x80 for r in mixed for b in r) and any(b < 0x20 for r in mixed for b in r)
    st = Stream(eng, max_reads=64, max_bases=cap, cands_per_read=64, n_slots=1)
    try:
        for batch, branch in ((full, "uniform"), (mixed, "general"), (full, "uniform"), (equal, "uniform"), (full, "uniform"), (edges, "general")):
            before = st.stats()
            st.submit(*_blob(batch))
            res, cands, _ = st.next()
            after = st.stats()
            assert after[branch] == before[branch] + 1 and after["uniform"] + after["general"] == before["uniform"] + before["general"] + 1
            want, image = _oracle_text(oracle_small, batch)
            assert eng.format_out(res, cands, image) == want
            assert batch is edges or (res["status"] == 0).sum() > len(batch) // 2      # the reads do hit: the records say something
        assert st.stats()["grow_reruns"] == 0
    finally:
        st.close()
    for grid in (_byte_grid(), _length_grid()[0]):
        total = sum(len(r) for r in grid)
        st = Stream(eng, max_reads=len(grid), max_bases=total + 4, cands_per_read=8, n_slots=1)
        try:
            st.submit(*_blob([b"ACGT" * 8000] * (total // 32000) + [b"ACGT" * ((total % 32000) // 4)]))   # letters up to the slot's end
            assert st.next_nocopy()[0] == total // 32000 + 1
            st.submit(*_blob(grid))
            res, cands, _ = st.next()
            want, image = _oracle_text(oracle_small, grid)
            assert eng.format_out(res, cands, image) == want
            assert (res["read_len"] == [len(r) for r in grid]).all()
        finally:
            st.close()


def test_synthetic_records_are_packed_records():
    """synth_reads_kernel writes the benchmark's reads as records directly.  Decoded to ASCII and packed again by K0 they must be
    the same words: same length word, codes, validity, and zero padding -- an N of a synthetic read carries code 0 like any other."""
    from lmat_amd import Engine, Params
    e = Engine(0, Params.run_rl())
    try:
        e.synth_taxonomy((2, 2, 2, 2, 2, 2))
        e.synth_db(2000, k=20)
        sr = e.synth_reads(3000, (75, 150, 151, 300), seed=3003)
        a, off = sr.ascii()
        assert set(np.diff(off).tolist()) == {75, 150, 151, 300} and (a == ord("N")).sum() >= 5
        up = e.upload_reads((np.append(a, np.uint8(0)), off))
        w_synth, ro_synth = sr.words()
        w_pack, ro_pack = up.words()
        assert (ro_synth == ro_pack).all()
        bad = np.nonzero(w_synth != w_pack)[0]
        assert not bad.size, "word %d: synthetic %08x, packed %08x; %d words differ" % (bad[0], w_synth[bad[0]], w_pack[bad[0]], bad.size)
        # and both are the reference's records of that ASCII
        ab = a.tobytes()
        want = np.concatenate([pack_ref(ab[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)])
        assert (w_pack == want).all()
        sr.free()
        up.free()
    finally:
        e.close()
