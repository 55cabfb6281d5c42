"""tests/img2_model.py -- the device image (LMATIMG2) stated in numpy -- held against the engine where the engine needs no device:
its addressing against lmat_table_address / lmat_table_unaddress at every k and every kind of geometry, its header rules against
lmat_image_check on the same good and damaged files; and against itself on fabricated images, whose single-field damage it must name."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import img2_model as im
from lmat_amd import capi

U = np.uint64
E_IO = -2


def _geometries():
    """(k, want_buckets, header) for every k of 10..20: W = 1, the widest W (the minimum table), a power of two, another integer; and
    fractional widths of 2, 3 and 4 at k = 19 and 20."""
    out = []
    for k in range(10, 21):
        m = k - 3
        lowbits = max(0, 2 * m - 32)
        space = 1 << (2 * m - lowbits)
        wmax = 127 >> lowbits
        for W in sorted({1, wmax, 4 if k == 20 else 16, 3 if k == 20 else 7, min(wmax, 100)}):
            want = space // W            # cpt_geometry: W = floor(space / want), clamped to 1..wmax
            assert max(1, min(wmax, space // want)) == W
            out.append(pytest.param(k, want, im.make_header(k, W), id="k%d-W%d" % (k, W)))
        if k >= 19:
            for want in (3 << 30, (1 << 32) // 3 + 1, (1 << 30) + 12345, 5 << 29):
                out.append(pytest.param(k, want, im.make_header(k, frac_nb=want), id="k%d-frac%d" % (k, want)))
    return out


def _edge_kmers(k, rng):
    enc = lambda s: int("".join(str("ACGT".index(c)) for c in s), 4)
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    words = ["A" * k, "T" * k, "C" * k, "G" * k, ("AC" * k)[:k], ("GT" * k)[:k], ("ACG" * k)[:k], ("TTA" * k)[:k], ("AT" * k)[:k], ("CG" * k)[:k],
             ("A" * (k - 1)) + "C", "C" + "A" * (k - 1), "A" * (k // 2) + "T" * (k - k // 2)]     # equal minimizers at two or more places
    if k % 2 == 0:                                                                                   # palindromes: their own reverse complement
        for _ in range(20):
            half = "".join("ACGT"[i] for i in rng.integers(0, 4, k // 2))
            words.append(half + rc(half))
            assert rc(words[-1]) == words[-1]
    return np.array([enc(w) for w in words], dtype=U)


@pytest.mark.parametrize("k,want,hdr", _geometries())
def test_addressing_is_the_engines(k, want, hdr):
    lib = capi.load_library()
    rng = np.random.default_rng(1000 * k + hdr.W)
    kmers = np.concatenate([_edge_kmers(k, rng), rng.integers(0, 1 << (2 * k), 1500, dtype=U)])
    rcs = im.revcomp(kmers, k)
    canon = np.minimum(kmers, rcs)
    b, t = im.address(hdr, kmers)
    b2, t2 = im.address(hdr, rcs)
    assert np.array_equal(b, b2) and np.array_equal(t, t2)                  # both strands of a k-mer: one address
    assert np.array_equal(im.unaddress(hdr, b, t), canon)                   # address, then unaddress: the identity
    assert (b < U(hdr.nb)).all() and (t >= U(1)).all() and (t <= U((hdr.W << hdr.lowbits) * 512)).all()
    nb, eb, et, ek = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    for i, x in enumerate(kmers.tolist()):
        assert lib.lmat_table_address(k, want, x, C.byref(nb), C.byref(eb), C.byref(et)) == 0
        assert nb.value == hdr.nb, "the header of this test is not the geometry the engine picks for the request"
        assert (eb.value, et.value) == (int(b[i]), int(t[i])), (hex(x), i)
        assert lib.lmat_table_unaddress(k, want, eb.value, et.value, C.byref(ek)) == 0 and ek.value == int(canon[i])
    # all-A: four equal minimizers, the tie goes to the smallest j
    assert ((int(t[0]) - 1) >> 7) & 3 == 0


def test_space_and_width_do_not_round_trip():
    """why the geometry is taken from the header's W and not recomputed from nb: k = 10 (hi-space 2^14), W = 100 gives 164 buckets, and
    2^14 // 164 = 99 is another table; the header rules accept the first and refuse the second under the first's bucket count."""
    h = im.make_header(10, 100)
    assert h.nb == 164 and (1 << 14) // h.nb == 99 and im.make_header(10, 99).nb == 166
    im.check_header(h, h.off_arena + h.bytes_arena)
    with pytest.raises(im.ImageError, match="nb"):
        im.check_header(h._replace(W=99), h.off_arena + h.bytes_arena)


# ---- fabricated images -----------------------------------------------------------------------------------------------------------
def _fabricate(fn, k, n_kmers, seed, wide=False, list_shift=0, n_ids=500):
    """An image written by this test with the insert rules of the engine's kernels restated on the host: a canonical k-mer goes into its
    home bucket while that has room, else -- flag set -- into the overflow table; a non-canonical one always does; wide tables probe
    linearly from their start bucket.  -> (header, the k-mers stored)"""
    rng = np.random.default_rng(seed)
    x = np.unique(rng.integers(0, 1 << (2 * k), n_kmers, dtype=U))
    x = np.minimum(x, im.revcomp(x, k))
    x = np.unique(x)
    noncanon = im.revcomp(x[:3], k)
    noncanon = noncanon[noncanon != x[:3]]
    stored = np.concatenate([x[3:], noncanon])
    unit = 8 << list_shift
    arena = np.zeros(unit * 40, dtype="<u2")
    pays = np.where(rng.random(stored.size) < 0.8, rng.integers(1, n_ids, stored.size), im.LIST_BASE + rng.integers(1, 40, stored.size)).astype(U)

    def wide_put(tab, start, km, pay):
        b = int(start)
        while True:
            free = np.nonzero(tab[b] == 0)[0]
            if free.size:
                tab[b, free[0]] = (U(km) << U(24)) | U(pay)
                return
            b = (b + 1) % tab.shape[0]

    if wide:
        h = im.make_header(k, None, nbuckets=max(16, stored.size // 5), arena_words=arena.size, list_shift=list_shift, n_ids=n_ids, n_kmers=stored.size)
        main = np.zeros((h.nbuckets, 8), dtype="<u8")
        for km, pay, s in zip(stored.tolist(), pays.tolist(), im.wide_bucket(stored, h.nbuckets).tolist()):
            wide_put(main, s, km, pay)
        ovf = np.zeros((0, 8), dtype="<u8")
    else:
        h = im.make_header(k, 127, ovf_nbuckets=1024, arena_words=arena.size, list_shift=list_shift, n_ids=n_ids, n_kmers=stored.size)
        main = np.zeros(h.nb, dtype=im.BUCKET)
        ovf = np.zeros((h.ovf_nbuckets, 8), dtype="<u8")
        bs, ts = im.address(h, stored)
        starts = im.ovf_bucket(bs, ts, h.ovf_nbuckets)
        is_canon = stored <= im.revcomp(stored, k)
        for km, pay, b, t, s, cn in zip(stored.tolist(), pays.tolist(), bs.tolist(), ts.tolist(), starts.tolist(), is_canon.tolist()):
            n = int(main["hdr"][b]) & im.COUNT_MASK
            if cn and n < im.SLOTS:
                main["tag"][b, n], main["plo"][b, n], main["phi"][b, n] = t, pay & 0xFFFF, pay >> 16
                main["hdr"][b] += 1
            else:
                main["hdr"][b] |= im.OVF_FLAG
                wide_put(ovf, s, km, pay)
    with open(fn, "wb") as f:
        f.write(im.pack(h))
        for off, part in ((h.off_slots, main), (h.off_ovf, ovf), (h.off_arena, arena)):
            f.seek(off)
            f.write(part.tobytes())
    assert os.path.getsize(fn) == h.off_arena + h.bytes_arena
    return h, stored


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """k = 12 at the minimum table: 2065 buckets, 16 000 k-mers -- some buckets fill up -- and three non-canonical keys"""
    fn = str(tmp_path_factory.mktemp("img2") / "good.img")
    h, stored = _fabricate(fn, 12, 16000, 12)
    return fn, h, stored


def test_pack_and_parse_are_inverse(good, tmp_path):
    fn, h, _ = good
    assert im.parse(fn) == h
    page = im.pack(h)
    assert len(page) == im.PAGE and page[:8] == b"LMATIMG2" and not any(page[im.HDR_BYTES:])
    # field by field, at the byte offsets of ImgHdr2 (lmat_api.cpp)
    assert struct.unpack_from("<II", page, 8) == (im.VERSION, 12) and struct.unpack_from("<Q", page, 16) == (2065,)
    assert struct.unpack_from("<IIIi", page, 24) == (127, 0, 9, -1) and struct.unpack_from("<IIII", page, 40) == (2065, 1024, 0, 500)
    assert struct.unpack_from("<QQQ", page, 56) == (h.n_kmers, h.arena_words, 0) and struct.unpack_from("<QQ", page, 80) == (0x1234, 0x5678)
    assert struct.unpack_from("<QQQQQQ", page, 96) == (4096, 2065 * 64, h.off_ovf, 65536, h.off_arena, h.bytes_arena)
    for name in im.FIELDS[1:]:
        v = getattr(h, name) + 1
        p = im.patched(fn, str(tmp_path / "p.img"), **{name: v})
        assert im.parse(p) == h._replace(**{name: v})
        assert im.pack(im.parse(p)) == open(p, "rb").read(im.PAGE)


def test_check_accepts_consistent_images(good, tmp_path):
    fn, h, stored = good
    assert im.check(fn, stored) == h
    km, pay, from_ovf = im.decode(fn)
    assert np.array_equal(km, np.sort(stored)) and from_ovf.sum() > 100 and (~from_ovf).sum() > 10000
    for name, k, wide, shift in (("w9.img", 9, True, 0), ("w12.img", 12, True, 0), ("c13.img", 13, False, 2)):
        p = str(tmp_path / name)
        hh, st = _fabricate(p, k, 5000, k, wide=wide, list_shift=shift)
        im.check(p, st)
        assert capi.image_check(p) == (0, "")
    im.check(_with_tail(im.patched(fn, str(tmp_path / "tail.img"))), stored)    # bytes behind the arena stay accepted


def _with_tail(fn):
    with open(fn, "ab") as f:
        f.write(b"\x55" * 1000)
    return fn


def _names(msg, name):
    return re.search(r"(?<![A-Za-z_])" + re.escape(name) + ("" if name.endswith("_") else r"(?![A-Za-z_])"), msg) is not None


def test_header_damage_is_refused_by_the_model_and_by_the_engine(good, tmp_path):
    """every case of header_refusals: check() and lmat_image_check refuse it, and both name the field"""
    fn, h, stored = good
    assert capi.image_check(fn) == (0, "")
    assert capi.image_check(_with_tail(im.patched(fn, str(tmp_path / "tail.img")))) == (0, "")
    cases = im.header_refusals(h, os.path.getsize(fn))
    assert len(cases) >= 40
    for cid, fields, cut, name in cases:
        p = im.patched(fn, str(tmp_path / "bad.img"), cut=cut, **fields)
        with pytest.raises(im.ImageError) as ei:
            im.check(p, stored)
        assert _names(str(ei.value), name), (cid, str(ei.value))
        rc, msg = capi.image_check(p)
        assert rc == E_IO, (cid, rc, msg)
        assert _names(msg.split(p + ": ", 1)[-1], name), (cid, msg)
    # a version-1 image cannot prove its map: the message says what to do
    rc, msg = capi.image_check(im.patched(fn, str(tmp_path / "v1.img"), version=1))
    assert rc == E_IO and "build" in msg and "again" in msg
    # what is no image at all
    assert capi.image_check(str(tmp_path / "missing.img"))[0] == E_IO
    assert capi.image_check(im.patched(fn, str(tmp_path / "magic.img"), magic=b"LMATIMG1"))[0] == E_IO
    with pytest.raises(im.ImageError, match="magic"):
        im.check(str(tmp_path / "magic.img"))
    # fields the loader takes on trust and only a decode can check
    p = im.patched(fn, str(tmp_path / "count.img"), n_kmers=h.n_kmers + 1)
    assert capi.image_check(p) == (0, "")
    with pytest.raises(im.ImageError, match="n_kmers"):
        im.check(p)
    with pytest.raises(im.ImageError, match="header page"):
        im.check(_poke(fn, str(tmp_path / "junk.img"), im.HDR_BYTES + 3, b"\x01"))


def test_wide_and_fractional_headers(tmp_path):
    """the header rules at the geometries the k = 12 image has not: the wide layout, lowbits = 2, the fractional width (files of
    header size claims only: lmat_image_check is held to the model on a sparse file)"""
    def both(h, size=None):
        p = str(tmp_path / "h.img")
        with open(p, "wb") as f:
            f.write(im.pack(h))
            f.truncate(h.off_arena + h.bytes_arena if size is None else size)      # sparse: no section is ever read
        rc, msg = capi.image_check(p)
        try:
            im.check_header(im.parse(p), os.path.getsize(p))
        except im.ImageError as e:
            assert rc == E_IO, (h, str(e))
            return str(e), msg
        assert (rc, msg) == (0, ""), (h, msg)
        return None
    wide = im.make_header(9, None, nbuckets=64)
    assert both(wide) is None
    for f in (dict(W=1), dict(m=6), dict(lowbits=1), dict(wshift=-2), dict(nbuckets=15), dict(bytes_slots=63 * 64)):
        assert both(wide._replace(**f)) is not None, f
    assert both(im.make_header(9, 1)) is not None                                    # k = 9 has no compact layout
    k20 = im.make_header(20, 31, ovf_nbuckets=4096)
    assert k20.lowbits == 2 and k20.nb == -(-(1 << 32) // 31) and both(k20) is None
    for f in (dict(lowbits=0), dict(lowbits=3), dict(W=32), dict(W=30), dict(wshift=0), dict(nb=k20.nb + 1), dict(m=16), dict(k=19)):
        assert both(k20._replace(**f)) is not None, f
    w1 = im.make_header(20, 1)                                                        # 2^32 buckets: indices end at 2^32 - 1
    assert w1.nb == 1 << 32 and w1.nbuckets == (1 << 32) - 1 and w1.wshift == 0 and both(w1) is None
    assert both(w1._replace(nbuckets=0)) is not None
    for k in (19, 20):
        fr = im.make_header(k, frac_nb=3 << 30)
        assert fr.wshift == -2 and fr.W == 2 and both(fr) is None
        for f in (dict(W=3), dict(W=1), dict(nb=1 << 30), dict(nb=(1 << 30) + 1), dict(wshift=-1), dict(wshift=1), dict(nbuckets=fr.nbuckets - 1)):
            assert both(fr._replace(**f)) is not None, (k, f)
    assert both(im.make_header(18, 4)._replace(wshift=-2)) is not None              # hi-space of 30 bits: no fractional width


def _poke(src, dst, offset, data):
    with open(src, "rb") as f:
        b = bytearray(f.read())
    b[offset:offset + len(data)] = data
    with open(dst, "wb") as f:
        f.write(b)
    return dst


def test_body_damage_is_named(good, tmp_path):
    """what the kernels write, damaged one slot at a time: the invariant that breaks is the one the message names"""
    fn, h, stored = good
    main = np.memmap(fn, dtype=im.BUCKET, mode="r", offset=h.off_slots, shape=(h.nb,))
    hdr = np.asarray(main["hdr"])
    n = hdr & im.COUNT_MASK
    full = int(np.nonzero((n == 12) & ((hdr & im.OVF_FLAG) != 0))[0][0])
    part = int(np.nonzero((n >= 2) & (n < 12))[0][0])
    at = lambda b, field_off: h.off_slots + 64 * b + field_off
    p = str(tmp_path / "b.img")
    cases = [
        ("overflow flag", at(full, 60), struct.pack("<I", 12)),                                  # table_insert without its atomicOr
        ("bucket slots", at(part, 60), struct.pack("<I", 0)),                                    # cpt_tidy_kernel without its header write: a count that is not the slots
        ("bucket header", at(part, 60), struct.pack("<I", 13)),
        ("bucket slots", at(part, 60), struct.pack("<I", int(n[part]) - 1)),
        ("bucket slots", at(part, 0), struct.pack("<H", 0)),                                     # a hole at slot 0
        ("tag", at(part, 2), bytes(main["tag"][part, 0:1].tobytes())),                           # slot 1 repeats slot 0's tag
        ("tag", at(part, 0), struct.pack("<H", 65535)),                                          # (W << lowbits) * 512 = 65024 at W = 127
        (("tag", "k-mers"), at(part, 0), struct.pack("<H", ((int(main["tag"][part, 0]) - 1) ^ 0x40) + 1)),   # the strand bit flipped: another k-mer, or one filed elsewhere
        ("bucket slots", at(part, 24 + 2 * 11), struct.pack("<H", 7)),                           # a payload behind the slots in use
        ("payload", at(part, 24), struct.pack("<H", 0)),                                         # (only where the high byte is 0 too: see below)
        ("payload", at(part, 48), struct.pack("<B", 200)),                                       # a list record far behind the arena
    ]
    if int(main["phi"][part, 0]) != 0:
        cases[9] = ("payload", at(part, 24), struct.pack("<H", 41))                              # list 41 of an arena of 40 records
    for want, off, data in cases:
        with pytest.raises(im.ImageError) as ei:
            im.check(_poke(fn, p, off, data), stored)
        assert str(ei.value).startswith(want), (want, off, str(ei.value))
    # the overflow table: a slot emptied (its k-mer is gone, and whatever probed past it is cut off), a key filed twice
    ovf = np.memmap(fn, dtype="<u8", mode="r", offset=h.off_ovf, shape=(h.ovf_nbuckets, 8))
    ob, os_ = [int(v[0]) for v in np.nonzero(np.asarray(ovf))]
    with pytest.raises(im.ImageError):
        im.check(_poke(fn, p, h.off_ovf + 64 * ob + 8 * os_, bytes(8)), stored)
    free_b = int(np.nonzero((np.asarray(ovf) == 0).all(axis=1))[0][0])
    with pytest.raises(im.ImageError, match="overflow table|twice"):
        im.check(_poke(fn, p, h.off_ovf + 64 * free_b, ovf[ob, os_].tobytes()), stored)
    with pytest.raises(im.ImageError, match="k-mers"):
        im.check(fn, stored[1:])
