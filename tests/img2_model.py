"""The device image (LMATIMG2, version 2) stated in numpy, independent of the engine: what a header field, a bucket, a tag, a slot
of the overflow table are, and which invariants a saved image keeps.  lmat_db_save_image writes this layout out of HBM and
lmat_db_load_image copies it back in, so the file IS what the classify kernels index: a test that only loads what it saved would not
notice a layout that changed without its version.  A change of the layout bumps `version` (lmat_api.cpp: kImgVersion) and changes this
file in the same commit.

  file    = header page (4 KiB, fields below, the rest zero) | bucket array | overflow table | list arena, each on a 4 KiB boundary
  compact bucket (64 B) = tag u16[12] | payload low u16[12] | payload high u8[12] | header u32 (bits 0..23 slots in use, bit 31: a
            k-mer of this bucket lives in the overflow table)
  wide bucket (64 B)    = 8 x u64 slots, k-mer << 24 | payload, 0 = empty: the overflow table of a compact table (filed by
            ovf_bucket_of(bucket, tag)) and the whole table of the wide layout (nb == 0, filed by the murmur finaliser of the k-mer)
  payload = 1 .. 65535: an internal taxid index;  65536 + o: the list record at arena byte (16 << list_shift) * o

address() / unaddress() restate cpt_address / cpt_unaddress of lmat_common.hpp on uint64 arrays; the geometry comes from the HEADER's
W, lowbits, m, wshift and nb, never from a bucket count (cpt_geometry(k, nb) need not give back the W that produced nb)."""
import os
import struct
from collections import namedtuple

import numpy as np

MAGIC = b"LMATIMG2"
VERSION = 2
PAGE = 4096
SLOTS = 12                  # per compact bucket
OVF_FLAG = 0x80000000
COUNT_MASK = 0x00FFFFFF
LIST_BASE = 65536
LIST_SHIFT_MAX = 4
_FMT = "<8sIIQIIIiIIIIQQQQQQQQQQQ"
FIELDS = ("magic version k nb W lowbits m wshift nbuckets ovf_nbuckets list_shift n_ids n_kmers arena_words n_lists "
          "tax_fingerprint mode_fingerprint off_slots bytes_slots off_ovf bytes_ovf off_arena bytes_arena").split()
Hdr = namedtuple("Hdr", FIELDS)
HDR_BYTES = struct.calcsize(_FMT)
assert HDR_BYTES == 144
OFFSET = {}                 # field -> (byte offset in the page, struct code): tests patch single fields with it
_o = 0
for _name, _code in zip(FIELDS, ["8s", "I", "I", "Q", "I", "I", "I", "i", "I", "I", "I", "I"] + ["Q"] * 11):
    OFFSET[_name] = (_o, "<" + _code)
    _o += struct.calcsize("<" + _code)
assert _o == HDR_BYTES
BUCKET = np.dtype([("tag", "<u2", SLOTS), ("plo", "<u2", SLOTS), ("phi", "u1", SLOTS), ("hdr", "<u4")])
assert BUCKET.itemsize == 64
U = np.uint64


class ImageError(AssertionError):
    pass


def _fail(field, what):
    raise ImageError("%s: %s" % (field, what))


# ---- header ----------------------------------------------------------------------------------------------------------------------
def parse(fn):
    with open(fn, "rb") as f:
        page = f.read(PAGE)
    if len(page) < PAGE:
        _fail("file size", "%d bytes: shorter than the header page" % len(page))
    if any(page[HDR_BYTES:]):
        _fail("header page", "bytes behind the last field are not zero")
    return Hdr(*struct.unpack(_FMT, page[:HDR_BYTES]))


def pack(hdr):
    return struct.pack(_FMT, *hdr) + bytes(PAGE - HDR_BYTES)


def patched(src, dst, cut=None, **fields):
    """A copy of image `src` at `dst` with the given header fields overwritten in place (nothing else follows suit: that is the
    point), then cut to `cut` bytes if given.  -> dst"""
    with open(src, "rb") as f:
        data = bytearray(f.read())
    for name, value in fields.items():
        o, code = OFFSET[name]
        struct.pack_into(code, data, o, value)
    with open(dst, "wb") as f:
        f.write(data if cut is None else data[:cut])
    return dst


def header_refusals(h, file_size):
    """Single-field damage to a good COMPACT image with header h that every loader must refuse: [(id, fields to overwrite, size to cut
    the file to or None, a name the refusal's message must hold)].  The CPU test holds check_header and lmat_image_check to the
    list, the GPU test lmat_db_load_image, the stand-alone host program restates it."""
    assert h.nb and h.k == 12 and file_size == h.off_arena + h.bytes_arena
    other_ws = 0 if h.wshift != 0 else -1
    cases = [
        ("W_plus_1", dict(W=h.W + 1), None, "W"), ("W_minus_1", dict(W=h.W - 1), None, "W"), ("W_zero", dict(W=0), None, "W"),
        ("wshift_disagrees", dict(wshift=other_ws), None, "wshift"), ("wshift_3", dict(wshift=3), None, "wshift"),
        ("wshift_fractional", dict(wshift=-2), None, "wshift"),
        ("lowbits_2", dict(lowbits=2), None, "lowbits"), ("m_minus_1", dict(m=h.m - 1), None, "m"), ("m_plus_1", dict(m=h.m + 1), None, "m"),
        ("nb_plus_1", dict(nb=h.nb + 1), None, "nb"), ("nb_minus_1", dict(nb=h.nb - 1), None, "nb"), ("nb_twice", dict(nb=2 * h.nb), None, "nb"),
        ("nbuckets_plus_1", dict(nbuckets=h.nbuckets + 1), None, "nbuckets"), ("nbuckets_minus_1", dict(nbuckets=h.nbuckets - 1), None, "nbuckets"),
        ("list_shift_5", dict(list_shift=5), None, "list_shift"),
        ("off_slots_unaligned", dict(off_slots=h.off_slots + 512), None, "off_slots"), ("off_slots_in_header", dict(off_slots=0), None, "off_slots"),
        ("off_ovf_unaligned", dict(off_ovf=h.off_ovf + 512), None, "off_ovf"), ("off_ovf_overlaps_buckets", dict(off_ovf=h.off_slots), None, "off_ovf"),
        ("off_arena_unaligned", dict(off_arena=h.off_arena + 512), None, "off_arena"), ("off_arena_overlaps_overflow", dict(off_arena=h.off_ovf), None, "off_arena"),
        ("off_slots_behind_arena", dict(off_slots=_up(file_size)), None, "off_"), ("off_arena_beyond_file", dict(off_arena=_up(file_size) + PAGE), None, "off_arena"),
        ("off_ovf_beyond_file", dict(off_ovf=_up(file_size) + PAGE), None, "off_ovf"),
        ("bytes_slots_plus_64", dict(bytes_slots=h.bytes_slots + 64), None, "bytes_slots"), ("bytes_slots_minus_64", dict(bytes_slots=h.bytes_slots - 64), None, "bytes_slots"),
        ("bytes_ovf_plus_64", dict(bytes_ovf=h.bytes_ovf + 64), None, "bytes_ovf"), ("bytes_ovf_zero", dict(bytes_ovf=0), None, "bytes_ovf"),
        ("bytes_arena_plus_2", dict(bytes_arena=h.bytes_arena + 2), None, "bytes_arena"), ("bytes_arena_huge", dict(bytes_arena=1 << 63), None, "bytes_arena"),
        ("arena_words_odd", dict(arena_words=h.arena_words + 1), None, "arena_words"),
        ("k_0", dict(k=0), None, "k"), ("k_21", dict(k=21), None, "k"), ("k_13", dict(k=13), None, "k"), ("k_11", dict(k=11), None, "k"),
        ("version_older", dict(version=VERSION - 1), None, "version"), ("version_newer", dict(version=VERSION + 1), None, "version"),
        ("cut_one_byte_short", {}, file_size - 1, "file size"), ("cut_inside_header", {}, 100, "header page"), ("magic_alone", {}, 8, "header page"),
    ]
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def _up(x):
    return (x + PAGE - 1) // PAGE * PAGE


def make_header(k, W=None, nbuckets=0, ovf_nbuckets=0, arena_words=8, list_shift=0, n_ids=100, n_kmers=0, n_lists=0, frac_nb=0):
    """A self-consistent header: compact with integer width W, or with frac_nb buckets of fractional width, or (W None) wide."""
    if frac_nb:
        m, lowbits, nb, wshift = k - 3, max(0, 2 * (k - 3) - 32), frac_nb, -2
        W = -(-(1 << 32) // nb)
    elif W is not None:
        m, lowbits = k - 3, max(0, 2 * (k - 3) - 32)
        nb = -(-(1 << (2 * m - lowbits)) // W)
        wshift = W.bit_length() - 1 if W & (W - 1) == 0 else -1
    else:
        m = lowbits = nb = W = 0
        wshift = -1
    if nb:
        nbuckets = min(nb, (1 << 32) - 1)
    bs, bo, ba = (nb or nbuckets) * 64, ovf_nbuckets * 64, arena_words * 2
    off_s = PAGE
    off_o = _up(off_s + bs)
    off_a = _up(off_o + bo)
    return Hdr(MAGIC, VERSION, k, nb, W, lowbits, m, wshift, nbuckets, ovf_nbuckets, list_shift, n_ids, n_kmers, arena_words, n_lists,
               0x1234, 0x5678, off_s, bs, off_o, bo, off_a, ba)


def check_header(h, file_size):
    """File frame and geometry: raises ImageError naming the field unless the header is one the current engine may load."""
    if h.magic != MAGIC:
        _fail("magic", repr(h.magic))
    if h.version != VERSION:
        _fail("version", "%d, the current one is %d" % (h.version, VERSION))
    if not 1 <= h.k <= 20:
        _fail("k", "%d not in 1..20" % h.k)
    if h.list_shift > LIST_SHIFT_MAX:
        _fail("list_shift", "%d above %d" % (h.list_shift, LIST_SHIFT_MAX))
    if h.nb == 0:
        if h.W or h.lowbits or h.m or h.wshift not in (-1, 0):
            _fail("W / lowbits / m / wshift", "compact fields set in a wide image")
        if h.nbuckets < 16:
            _fail("nbuckets", "%d: a wide table has at least 16" % h.nbuckets)
    else:
        if h.k < 10:
            _fail("nb", "k = %d has no compact layout" % h.k)
        m = h.k - 3
        lowbits = max(0, 2 * m - 32)
        if h.m != m:
            _fail("m", "%d, k - 3 is %d" % (h.m, m))
        if h.lowbits != lowbits:
            _fail("lowbits", "%d, max(0, 2m - 32) is %d" % (h.lowbits, lowbits))
        if not 1 <= h.W <= 127 >> lowbits:
            _fail("W", "%d not in 1..%d" % (h.W, 127 >> lowbits))
        space = 1 << (2 * m - lowbits)
        if h.wshift == -2:
            if space != 1 << 32:
                _fail("wshift", "-2 (fractional width) without a 32-bit hi-space")
            if not (1 << 30) < h.nb < (1 << 32):
                _fail("nb", "%d: a fractional width has between 2^30 and 2^32 buckets" % h.nb)
            if h.W != -(-space // h.nb):
                _fail("W", "%d, ceil(2^32 / nb) is %d" % (h.W, -(-space // h.nb)))
        else:
            if h.nb != -(-space // h.W):
                _fail("nb", "%d, W implies %d" % (h.nb, -(-space // h.W)))
            ws = h.W.bit_length() - 1 if h.W & (h.W - 1) == 0 else -1
            if h.wshift != ws:
                _fail("wshift", "%d, W implies %d" % (h.wshift, ws))
        if h.nbuckets != min(h.nb, (1 << 32) - 1):
            _fail("nbuckets", "%d, nb implies %d" % (h.nbuckets, min(h.nb, (1 << 32) - 1)))
    if h.bytes_slots != (h.nb or h.nbuckets) * 64:
        _fail("bytes_slots", "%d, the bucket count implies %d" % (h.bytes_slots, (h.nb or h.nbuckets) * 64))
    if h.bytes_ovf != h.ovf_nbuckets * 64:
        _fail("bytes_ovf", "%d, ovf_nbuckets implies %d" % (h.bytes_ovf, h.ovf_nbuckets * 64))
    if h.bytes_arena != h.arena_words * 2:
        _fail("bytes_arena", "%d against arena_words = %d" % (h.bytes_arena, h.arena_words))
    if h.off_slots % PAGE or h.off_slots < PAGE or h.off_slots > file_size:
        _fail("off_slots", "%d: not a 4 KiB boundary behind the header page and inside the file" % h.off_slots)
    if h.off_ovf % PAGE or h.off_ovf < h.off_slots + h.bytes_slots or h.off_ovf > file_size:
        _fail("off_ovf", "%d: not a 4 KiB boundary behind the bucket array and inside the file" % h.off_ovf)
    if h.off_arena % PAGE or h.off_arena < h.off_ovf + h.bytes_ovf or h.off_arena > file_size:
        _fail("off_arena", "%d: not a 4 KiB boundary behind the overflow table and inside the file" % h.off_arena)
    if h.off_arena + h.bytes_arena > file_size:
        _fail("file size", "%d, the arena ends at %d" % (file_size, h.off_arena + h.bytes_arena))


# ---- addressing --------------------------------------------------------------------------------------------------------------------
def revcomp(x, k):
    x = np.asarray(x, dtype=U)
    r = np.zeros_like(x)
    y = x.copy()
    for _ in range(k):
        r = (r << U(2)) | (U(3) - (y & U(3)))
        y = y >> U(2)
    return r


def _rounds(x, m, keys, backwards):
    mm = U((1 << m) - 1)
    L, R = x >> U(m), x & mm
    f = lambda v, key: ((v * U(key)) & U(0xFFFFFFFF)) >> U(7) & mm      # v < 2^17, key < 2^15: the 32-bit product never wraps
    ka, kb, kc, kd = keys
    if not backwards:
        L = L ^ f(R, ka)
        R = R ^ f(L, kb)
        L = L ^ f(R, kc)
        R = R ^ f(L, kd)
    else:
        R = R ^ f(L, kd)
        L = L ^ f(R, kc)
        R = R ^ f(L, kb)
        L = L ^ f(R, ka)
    return (L << U(m)) | R


_SCRAMBLE = (0x6A09, 0x3B67, 0x5F1D, 0x7C15)    # minimizer order
_MIX = (0x52DB, 0x4F6D, 0x6E2B, 0x35A7)         # bucket hash


def address(h, kmers):
    """(bucket, tag) of each k-mer (forward-encoded, either strand) in the compact table the header describes."""
    assert h.nb
    x = np.asarray(kmers, dtype=U)
    r = revcomp(x, h.k)
    c, cr = np.minimum(x, r), np.maximum(x, r)
    m = h.m
    mmask = U((1 << (2 * m)) - 1)
    best = np.full(c.shape, ~U(0), dtype=U)
    for j in range(4):
        a = (c >> U(2 * (3 - j))) & mmask             # m-mer j of the canonical k-mer
        ar = (cr >> U(2 * j)) & mmask                 # its reverse complement
        y = np.minimum(a, ar)
        v = (_rounds(y, m, _SCRAMBLE, False) << U(3)) | U(j << 1) | (ar < a).astype(U)
        best = np.minimum(best, v)                    # equal minimizers: the smaller j
    j = (best >> U(1)) & U(3)
    strand = best & U(1)
    sp = _rounds(best >> U(3), m, _MIX, False)
    hi, low = sp >> U(h.lowbits), sp & U((1 << h.lowbits) - 1)
    if h.wshift == -2:
        prod = hi * U(h.nb)                           # hi, nb < 2^32
        b, lowp = prod >> U(32), prod & U(0xFFFFFFFF)
        rho = (lowp >= U(h.nb)).astype(U) + (lowp >= U(2 * h.nb)).astype(U) + (lowp >= U(3 * h.nb)).astype(U)
    else:
        b = hi // U(h.W)
        rho = hi - b * U(h.W)
    rs = U(2) * (U(3) - j)                            # bits of the k-mer right of the minimizer
    other = ((c >> (U(2 * m) + rs)) << rs) | (c & ((U(1) << rs) - U(1)))
    tag = U(1) + ((((rho << U(h.lowbits)) | low) * U(4) + j) * U(2) + strand) * U(64) + other
    return b, tag


def unaddress(h, bucket, tag):
    """The canonical k-mer filed under (bucket, tag != 0)."""
    assert h.nb
    b, t = np.asarray(bucket, dtype=U), np.asarray(tag, dtype=U) - U(1)
    other, strand, j, rl = t & U(63), (t >> U(6)) & U(1), (t >> U(7)) & U(3), t >> U(9)
    rho, low = rl >> U(h.lowbits), rl & U((1 << h.lowbits) - 1)
    if h.wshift == -2:
        hi = ((b << U(32)) + U(h.nb - 1)) // U(h.nb) + rho    # the rho-th hi with hi * nb >> 32 == bucket
    else:
        hi = b * U(h.W) + rho
    m = h.m
    y = _rounds(_rounds((hi << U(h.lowbits)) | low, m, _MIX, True), m, _SCRAMBLE, True)
    x = np.where(strand == U(1), revcomp(y, m), y)
    rs = U(2) * (U(3) - j)
    return ((other >> rs) << (U(2 * m) + rs)) | (x << rs) | (other & ((U(1) << rs) - U(1)))


def _mix64(x):
    x = x ^ (x >> U(33))
    x = x * U(0xff51afd7ed558ccd)
    x = x ^ (x >> U(33))
    x = x * U(0xc4ceb9fe1a85ec53)
    return x ^ (x >> U(33))


def wide_bucket(kmers, nbuckets):
    """Where the wide layout starts probing for a k-mer: mix64(kmer) * nbuckets >> 64."""
    with np.errstate(over="ignore"):
        hsh = _mix64(np.asarray(kmers, dtype=U))
    return ((hsh >> U(32)) * U(nbuckets) + (((hsh & U(0xFFFFFFFF)) * U(nbuckets)) >> U(32))) >> U(32)


def ovf_bucket(bucket, tag, nbuckets):
    """Where the overflow table of a compact table starts probing: a function of the compact address (32-bit arithmetic)."""
    b, t = np.asarray(bucket, dtype=U), np.asarray(tag, dtype=U)
    M = U(0xFFFFFFFF)
    hsh = ((b ^ ((t << U(16)) & M) ^ (t >> U(3))) * U(0x9E3779B1)) & M
    hsh = hsh ^ (hsh >> U(15))
    return (hsh * U(nbuckets)) >> U(32)


# ---- decoding ----------------------------------------------------------------------------------------------------------------------
def _sections(fn, h):
    """memmaps of the bucket array (compact: BUCKET records, wide: u64[n][8]) and of the overflow table (u64[n][8] or None)"""
    if h.nb:
        main = np.memmap(fn, dtype=BUCKET, mode="r", offset=h.off_slots, shape=(h.nb,))
    else:
        main = np.memmap(fn, dtype="<u8", mode="r", offset=h.off_slots, shape=(h.nbuckets, 8))
    ovf = np.memmap(fn, dtype="<u8", mode="r", offset=h.off_ovf, shape=(h.ovf_nbuckets, 8)) if h.nb and h.ovf_nbuckets else None
    return main, ovf


def _wide_entries(tab):
    """(k-mers, payloads, bucket of each) of the occupied slots of a wide-layout table"""
    if tab is None:
        z = np.zeros(0, dtype=U)
        return z, z, z
    b, s = np.nonzero(np.asarray(tab))
    v = np.asarray(tab)[b, s].astype(U)
    return v >> U(24), v & U(0xFFFFFF), b.astype(U)


def _bucket_entries(main, h):
    """(k-mers, payloads, bucket, tag) of the occupied slots of a compact bucket array"""
    tags = np.asarray(main["tag"])
    b, s = np.nonzero(tags)
    tag = tags[b, s].astype(U)
    pay = np.asarray(main["plo"])[b, s].astype(U) | (np.asarray(main["phi"])[b, s].astype(U) << U(16))
    return unaddress(h, b.astype(U), tag), pay, b.astype(U), tag


def decode(fn):
    """-> (k-mers ascending, their payloads, from_overflow flags): every k-mer the image holds, buckets and overflow table together."""
    h = parse(fn)
    main, ovf = _sections(fn, h)
    if h.nb:
        km, pay, _, _ = _bucket_entries(main, h)
        ok, op, _ = _wide_entries(ovf)
        km, pay = np.concatenate([km, ok]), np.concatenate([pay, op])
        src = np.concatenate([np.zeros(km.size - ok.size, dtype=bool), np.ones(ok.size, dtype=bool)])
    else:
        km, pay, _ = _wide_entries(main)
        src = np.zeros(km.size, dtype=bool)
    o = np.argsort(km, kind="stable")
    return km[o], pay[o], src[o]


def probe_buckets(fn, kmers):
    """Reads just the home buckets of `kmers` from a compact image -> (found, payload, overflow flag of the bucket); nothing else
    of the file is touched (the k = 20 table is 8 GB)."""
    h = parse(fn)
    main, _ = _sections(fn, h)
    b, tag = address(h, kmers)
    rows = main[b.astype(np.int64)]
    hit = rows["tag"].astype(U) == tag[:, None]
    assert (hit.sum(axis=1) <= 1).all(), "a tag twice in one bucket"
    pay = rows["plo"].astype(U) | (rows["phi"].astype(U) << U(16))
    return hit.any(axis=1), (pay * hit).sum(axis=1), (rows["hdr"] & np.uint32(OVF_FLAG)) != 0


# ---- invariants --------------------------------------------------------------------------------------------------------------------
def _reachable(start, at, tab, what):
    """linear probing stops at the first bucket with an empty slot: every bucket from a key's start up to the one before its own is full"""
    if not start.size:
        return
    n = tab.shape[0]
    gaps = np.concatenate([[0], np.cumsum((np.asarray(tab) == 0).any(axis=1))]).astype(np.int64)     # gaps[i]: buckets < i with an empty slot
    s, a = start.astype(np.int64), at.astype(np.int64)
    between = np.where(a >= s, gaps[a] - gaps[s], gaps[n] - gaps[s] + gaps[a])
    if (between != 0).any():
        i = int(np.nonzero(between)[0][0])
        _fail(what, "the key in bucket %d starts probing at %d and a bucket with an empty slot lies between: no lookup finds it" % (a[i], s[i]))


def check(fn, source_kmers=None, body=True):
    """Raises ImageError with the field or the invariant named unless the image keeps every rule of this module.  body=False: the
    header alone (frame and geometry).  source_kmers: the decoded set must be exactly these (as stored, either strand)."""
    h = parse(fn)
    check_header(h, os.path.getsize(fn))
    if not body:
        return h
    main, ovf = _sections(fn, h)
    k = h.k
    if h.nb:
        hdr = np.asarray(main["hdr"])
        n = (hdr & np.uint32(COUNT_MASK)).astype(np.int64)
        if (n > SLOTS).any():
            _fail("bucket header", "bucket %d counts %d slots" % (int(np.argmax(n > SLOTS)), int(n[np.argmax(n > SLOTS)])))
        if (hdr & np.uint32(~(OVF_FLAG | COUNT_MASK) & 0xFFFFFFFF)).any():
            _fail("bucket header", "bits 24..30 set")
        used = np.arange(SLOTS)[None, :] < n[:, None]
        tags, plo, phi = np.asarray(main["tag"]), np.asarray(main["plo"]), np.asarray(main["phi"])
        if ((tags != 0) != used).any():
            b = int(np.nonzero(((tags != 0) != used).any(axis=1))[0][0])
            _fail("bucket slots", "bucket %d: header count %d, tags %s (slots 0..n-1 hold tags, the rest is zero)" % (b, n[b], tags[b].tolist()))
        if (plo[~used] != 0).any() or (phi[~used] != 0).any():
            _fail("bucket slots", "a payload behind the slots in use")
        if (tags.astype(np.int64) > (h.W << h.lowbits) * 512).any():
            _fail("tag", "above (W << lowbits) * 512 = %d" % ((h.W << h.lowbits) * 512))
        st = np.sort(tags, axis=1)
        if ((st[:, 1:] == st[:, :-1]) & (st[:, 1:] != 0)).any():
            _fail("tag", "twice in bucket %d" % int(np.nonzero(((st[:, 1:] == st[:, :-1]) & (st[:, 1:] != 0)).any(axis=1))[0][0]))
        bk, bp, bb, bt = _bucket_entries(main, h)
        ab, at = address(h, bk)
        if (ab != bb).any() or (at != bt).any() or (bk > revcomp(bk, k)).any():
            _fail("tag", "a slot does not decode to a canonical k-mer with this address: no lookup finds it")
        ok, op, ob = _wide_entries(ovf)
        orc = revcomp(ok, k)
        if ok.size:
            hb, ht = address(h, ok)
            if (ok >> U(2 * k)).any():
                _fail("overflow table", "a key wider than 2k bits")
            home = hb.astype(np.int64)
            if ((hdr[home] & np.uint32(OVF_FLAG)) == 0).any():
                i = int(np.nonzero((hdr[home] & np.uint32(OVF_FLAG)) == 0)[0][0])
                _fail("overflow flag", "k-mer %d sits in the overflow table, its home bucket %d has bit 31 clear: no lookup finds it" % (int(ok[i]), home[i]))
            canon = ok <= orc
            if (n[home[canon]] != SLOTS).any():
                _fail("overflow table", "a canonical k-mer whose home bucket is not full")
            _reachable(ovf_bucket(hb, ht, h.ovf_nbuckets), ob, ovf, "overflow table")
        km, pay = np.concatenate([bk, ok]), np.concatenate([bp, op])
    else:
        km, pay, wb = _wide_entries(main)
        if (km >> U(2 * k)).any():
            _fail("wide table", "a key wider than 2k bits")
        _reachable(wide_bucket(km, h.nbuckets), wb, main, "wide table")
    skm = np.sort(km)
    if (skm[1:] == skm[:-1]).any():
        _fail("k-mers", "%d occurs twice" % int(skm[1:][skm[1:] == skm[:-1]][0]))
    plain = pay < U(LIST_BASE)
    if ((pay[plain] < U(1)) | (pay[plain] > U(min(h.n_ids, 65536) - 1))).any():
        _fail("payload", "a plain taxid index outside 1..%d" % (min(h.n_ids, 65536) - 1))
    if ((pay[~plain] - U(LIST_BASE)) * U(16 << h.list_shift) >= U(h.bytes_arena)).any():
        _fail("payload", "a list record at or behind the arena's end (%d bytes, list_shift %d)" % (h.bytes_arena, h.list_shift))
    if km.size != h.n_kmers:
        _fail("n_kmers", "%d, the image holds %d" % (h.n_kmers, km.size))
    if source_kmers is not None:
        want = np.sort(np.asarray(source_kmers, dtype=U))
        if not np.array_equal(skm, want):
            _fail("k-mers", "the decoded set (%d) is not the source's (%d)" % (skm.size, want.size))
    return h
