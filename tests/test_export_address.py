"""cpt_unaddress (lmat_common.hpp), through lmat_table_unaddress: the way back from (bucket, tag) to the canonical k-mer, which the
export of a loaded database (dbexport.hip) decodes every occupied slot of the compact table with.  It must invert lmat_table_address
at every kind of geometry: a power-of-two bucket width, any other integer width, and the fractional width of the large tables."""
import ctypes as C

import numpy as np
import pytest

from lmat_amd import capi


def _rc(x, k):
    r = 0
    for i in range(k):
        r = (r << 2) | (3 - ((x >> (2 * i)) & 3))
    return r


def _canon_random(k, n, seed):
    """n random canonical k-mers (numpy, vectorised reverse complement)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)
    r = np.zeros(n, dtype=np.uint64)
    y = x.copy()
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (y & np.uint64(3)))
        y >>= np.uint64(2)
    return np.minimum(x, r)


class _Table:
    def __init__(self, k, want):
        self.lib = capi.load_library()
        self.k, self.want = k, want
        self.nb, self.b, self.t, self.km = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.pnb, self.pb, self.pt, self.pkm = C.byref(self.nb), C.byref(self.b), C.byref(self.t), C.byref(self.km)

    def address(self, kmer):
        assert self.lib.lmat_table_address(self.k, self.want, kmer, self.pnb, self.pb, self.pt) == 0
        return self.b.value, self.t.value

    def unaddress(self, bucket, tag):
        assert self.lib.lmat_table_unaddress(self.k, self.want, bucket, tag, self.pkm) == 0
        return self.km.value


@pytest.mark.parametrize("want", [1, 1000, 1 << 14])   # widths 127, 16 and 1 of the 2^14 values a 7-mer minimizer hashes to
def test_unaddress_inverts_address_exhaustive_k10(want):
    k = 10
    tb = _Table(k, want)
    seen = {}
    for x in range(4 ** k):
        if x > _rc(x, k):
            continue
        b, t = tb.address(x)
        assert tb.unaddress(b, t) == x, (x, b, t)
        seen[(b, t)] = x
    assert len(seen) == (4 ** k + 4 ** (k // 2)) // 2
    # the other direction: distinct pairs give distinct k-mers, and every pair address produced decodes (to the k-mer filed there)
    back = {tb.unaddress(b, t) for (b, t) in seen}
    assert len(back) == len(seen) and back == set(seen.values())


# (k, want_buckets, the bucket count the geometry must come to: 0 = not checked) -- W = hi-space / buckets
GEOMETRIES = [
    (11, 1, 0),                      # W = 127: hi-space 2^16 (odd k: minimizers that are their own reverse complement)
    (11, 1 << 12, 1 << 12),          # W = 16
    (11, (1 << 16) // 3, 0),         # W = 3
    (13, 1, 0),                      # W = 127: hi-space 2^20
    (13, 1 << 17, 1 << 17),          # W = 8
    (13, (1 << 20) // 5, 0),         # W = 5
    (15, 1, 0),                      # W = 127: hi-space 2^24
    (15, 1 << 22, 1 << 22),          # W = 4
    (15, (1 << 24) // 7, 0),         # W = 7
    (17, 1, 0),                      # W = 127: hi-space 2^28
    (17, 1 << 23, 1 << 23),          # W = 32
    (17, (1 << 28) // 9, 0),         # W = 9
    (16, 1 << 20, 1 << 20),          # W = 64, a power of two
    (16, 1, 0),                      # W = 127, the minimum table
    (16, (1 << 26) // 3, 0),         # W = 3
    (18, 1 << 27, 1 << 27),          # W = 8
    (18, 1, 0),                      # W = 127
    (18, (1 << 30) // 5, 0),         # W = 5
    (19, 1 << 28, 1 << 28),          # W = 16
    (19, 1, 0),                      # W = 127
    (19, 3 << 30, 3 << 30),          # fractional: exactly the buckets asked for
    (20, 1 << 30, 1 << 30),          # W = 4, two low bits in the tag
    (20, 1, 0),                      # W = 31
    (20, 3 << 30, 3 << 30),          # fractional
]


@pytest.mark.parametrize("k,want,nb", GEOMETRIES)
def test_unaddress_inverts_address_sampled(k, want, nb):
    tb = _Table(k, want)
    kmers = _canon_random(k, 1 << 18, 7 * k + (want & 0xFFFF))
    seen = set()
    for x in kmers.tolist():
        b, t = tb.address(x)
        assert tb.unaddress(b, t) == x, (hex(x), b, t)
        seen.add((b, t))
    if nb:
        assert tb.nb.value == nb
    assert len(seen) == np.unique(kmers).size


def test_unaddress_refuses_what_the_geometry_has_not():
    lib = capi.load_library()
    km = C.c_uint64()
    assert lib.lmat_table_unaddress(8, 1 << 20, 0, 1, C.byref(km)) == -1          # no compact layout below k = 10
    assert lib.lmat_table_unaddress(20, 1 << 30, 1 << 30, 1, C.byref(km)) == -1    # bucket beyond the table
    assert lib.lmat_table_unaddress(20, 1 << 30, 0, 0, C.byref(km)) == -1          # tag 0 is the empty slot
    assert lib.lmat_table_unaddress(20, 1 << 30, 0, 16 * 512 + 1, C.byref(km)) == -1   # rho = 4 at W = 4
    assert lib.lmat_table_unaddress(20, 1 << 30, 0, 1, None) == -1
