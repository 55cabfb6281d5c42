"""The claim the PLAIN/UNI repeat filter rests on (kernels.hip, classify_one, "repeats"): for EVEN k no two positions of a read
with equal canonical k-mers have their minimizer at the same place in the read.  A run of the filter is a stretch of k-mers with one
bucket and one minimizer position, so a k-mer never recurs inside a run and the filter need not compare digests inside one.

The minimizer position of the k-mer at p is p + j when the forward strand is the canonical one and p + 3 - j otherwise, j being the
m-mer (m = k - 3) that cpt_address (lmat_common.hpp) picks, counted in the canonical k-mer's direction, ties to the smaller j.

cpt_geometry takes k >= 10, so the exhaustive cases (k = 6 and 8, every sequence of k + 3 bases) run a numpy model of cpt_address's
choice; the model is first held against the real function (lmat_table_address: j sits in the tag) at every k of 10 .. 20.  At k = 20
the real function runs on 10^5 random and 10^4 structured sequences.  An odd k (7, exhaustive, model) must SHOW such pairs: the
generic kernel keeps its compares for a reason, and this test can see a pair when there is one."""
import ctypes as C

import numpy as np
import pytest

from lmat_amd import capi

W = 4   # m-mers a k-mer covers (kCptW)
SCRAMBLE = (0x6A09, 0x3B67, 0x5F1D, 0x7C15)   # cpt_scramble's round keys


def _feistel(x, m, keys):
    mm = np.uint64((1 << m) - 1)
    L, R = x >> np.uint64(m), x & mm
    L = L ^ (((R * np.uint64(keys[0])) >> np.uint64(7)) & mm)
    R = R ^ (((L * np.uint64(keys[1])) >> np.uint64(7)) & mm)
    L = L ^ (((R * np.uint64(keys[2])) >> np.uint64(7)) & mm)
    R = R ^ (((L * np.uint64(keys[3])) >> np.uint64(7)) & mm)
    return (L << np.uint64(m)) | R


def _kmers(codes, k):
    """codes: (n, len) of 0..3 -> forward and reverse-complement k-mers, (n, len - k + 1) each, first base in the high bits."""
    n, ln = codes.shape
    f = np.zeros((n, ln - k + 1), dtype=np.uint64)
    r = np.zeros_like(f)
    for i in range(k):
        col = codes[:, i:i + ln - k + 1].astype(np.uint64)
        f = (f << np.uint64(2)) | col
        r = r | ((np.uint64(3) - col) << np.uint64(2 * i))
    return f, r


def _model_j(c, cr, k):
    """cpt_address's choice of the minimizer among the four m-mers of the canonical k-mer c (cr: its reverse complement)."""
    m = k - (W - 1)
    mmask = np.uint64((1 << (2 * m)) - 1)
    best = np.full(c.shape, np.iinfo(np.uint64).max, dtype=np.uint64)
    for j in range(W):
        x = (c >> np.uint64(2 * (W - 1 - j))) & mmask
        xr = (cr >> np.uint64(2 * j)) & mmask
        v = (_feistel(np.minimum(x, xr), m, SCRAMBLE) << np.uint64(3)) | np.uint64(j << 1) | (xr < x).astype(np.uint64)
        best = np.minimum(best, v)
    return ((best >> np.uint64(1)) & np.uint64(3)).astype(np.int64)


def _real_j(lib, kms, k):
    nb, b, t = C.c_uint64(), C.c_uint32(), C.c_uint32()
    out = np.zeros(kms.shape, dtype=np.int64)
    flat, o = kms.ravel(), out.ravel()
    for i in range(flat.size):
        assert lib.lmat_table_address(k, 1 << 20, int(flat[i]), C.byref(nb), C.byref(b), C.byref(t)) == 0
        o[i] = ((t.value - 1) >> 7) & 3
    return out


def _same_place_pairs(codes, k, j_of):
    """-> the number of position pairs (p < p') of one sequence with equal canonical k-mers AND equal minimizer positions."""
    f, r = _kmers(codes, k)
    fc = f < r   # the kernel's `fc`: a k-mer equal to its reverse complement counts as reverse
    c, cr = np.minimum(f, r), np.maximum(f, r)
    j = j_of(c, cr)
    q = np.arange(f.shape[1], dtype=np.int64)[None, :] + np.where(fc, j, W - 1 - j)
    bad = 0
    for a in range(f.shape[1]):
        for b in range(a + 1, f.shape[1]):
            bad += int(((c[:, a] == c[:, b]) & (q[:, a] == q[:, b])).sum())
    return bad


def _all_sequences(length, chunk=1 << 20):
    for lo in range(0, 4 ** length, chunk):
        x = np.arange(lo, min(lo + chunk, 4 ** length), dtype=np.uint64)
        yield np.stack([((x >> np.uint64(2 * (length - 1 - i))) & np.uint64(3)).astype(np.uint8) for i in range(length)], axis=1)


@pytest.mark.parametrize("k", range(10, 21))   # every k with a compact layout: even m (odd k) has m-mers equal to their own reverse complement
def test_the_model_picks_what_cpt_address_picks(k):
    lib = capi.load_library()
    rng = np.random.default_rng(100 + k)
    codes = rng.integers(0, 4, size=(1500, k + 3), dtype=np.uint8)
    codes[:300, k // 2:] = 3 - codes[:300, :k + 3 - k // 2][:, ::-1]   # reverse-complement structure: equal m-mers, ties
    codes[300:400] = codes[300:400, :1]                                # homopolymers
    f, r = _kmers(codes, k)
    c, cr = np.minimum(f, r), np.maximum(f, r)
    assert np.array_equal(_model_j(c, cr, k), _real_j(lib, f, k))
    assert np.array_equal(_real_j(lib, f[:200], k), _real_j(lib, r[:200], k))   # (the entry point takes either strand)


@pytest.mark.parametrize("k", [6, 8])
def test_even_k_exhaustive(k):
    """Every sequence of k + 3 bases (4 k-mer positions: all the pairs at most 3 apart, which is all a run can hold)."""
    pairs = 0
    for codes in _all_sequences(k + 3):
        f, r = _kmers(codes, k)
        c = np.minimum(f, r)
        pairs += int(sum(((c[:, a] == c[:, b]).sum() for a in range(4) for b in range(a + 1, 4))))
        assert _same_place_pairs(codes, k, lambda c, cr: _model_j(c, cr, k)) == 0
    assert pairs > 1000   # equal canonical k-mers within 3 positions do occur: the claim is about where their minimizers lie


def test_odd_k_has_such_pairs():
    bad = sum(_same_place_pairs(codes, 7, lambda c, cr: _model_j(c, cr, 7)) for codes in _all_sequences(10))
    assert bad > 0


def _structured(rng, n, length):
    """Tandem repeats of period 1 .. 6, X.rc(X) with the centre at every place, both with and without one substitution."""
    out = np.zeros((n, length), dtype=np.uint8)
    for i in range(n):
        kind = i % 4
        if kind < 2:
            unit = rng.integers(0, 4, size=1 + i // 4 % 6, dtype=np.uint8)
            s = np.tile(unit, length)[:length]
        else:
            x = rng.integers(0, 4, size=length, dtype=np.uint8)
            centre = 1 + i // 4 % (length - 1)   # bases left of the centre
            s = np.concatenate([x, (3 - x)[::-1]])[length - centre:][:length]
        if kind % 2:
            p = int(rng.integers(0, length))
            s = s.copy()
            s[p] = (s[p] + rng.integers(1, 4)) & 3
        out[i] = s
    return out


def test_k20_random_and_structured():
    lib = capi.load_library()
    rng = np.random.default_rng(2020)
    k = 20
    real = lambda c, cr: _real_j(lib, c, k)
    structured = _structured(rng, 10_000, k + 3)
    f, r = _kmers(structured, k)
    c = np.minimum(f, r)
    assert sum(int((c[:, a] == c[:, b]).sum()) for a in range(4) for b in range(a + 1, 4)) > 2000   # the structure does make equal k-mers
    assert _same_place_pairs(structured, k, real) == 0
    assert _same_place_pairs(rng.integers(0, 4, size=(100_000, k + 3), dtype=np.uint8), k, real) == 0
