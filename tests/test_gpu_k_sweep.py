"""Classify at every kind of k the engine accepts, not only the even 16, 18 and 20 of the rest of the suite.

What an even k >= 16 never runs: an m-mer (m = k - 3) that is its own reverse complement (the palindrome bit of pass1_chunk and of
the tail kernel, the non-ODDM strand of cpt_finish), a k-mer twice inside one run of the repeat filter (the digest compares of the
generic kernel: test_k20_same_run_repeats.py shows why only an odd k has such pairs), the GC accounting's spread_left at a k that is
not 20, hi-spaces of 2^14 .. 2^24, and below k = 10 the wide layout as the only one (the CPT == false instantiations).

Per k one set of 500 to 700 reads built around those arms and around every length edge, which all move with k (positions P = len - k
+ 1: the chunk edges, the three steps of the tail plan and one past, the 160-position class edge, 256/257, 320/321, 512/513), and a
database of six of seven of their distinct k-mers with lists from a small menu, both chosen by a hash of the k-mer's value -- so a
missed, doubled or mis-addressed k-mer shows in cand_kmer_cnt and in the per-taxid found counts behind the scores.  The expected values come from the CPU
oracle (text, tallies) and, independently of it, from kmer_model.py (valid_kmers, cand_kmer_cnt, found counts, the GC bin, the lookups).

k = 16 and 20 are the control: the harness has to pass where the suite already trusts the engine.  The preconditions -- the reads do
hold same-run pairs at odd k and none at even k, and k-mers whose minimizer is a palindrome, on both strands -- are CPU tests."""
import ctypes as C
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (the child process below starts from this file)

import kmer_model
from test_k20_same_run_repeats import W, _kmers, _model_j

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BR = (3, 4, 4, 4, 4, 3)
CONTROL_K = (16, 20)
COMPACT_K = (10, 11, 13, 15, 17, 19)
WIDE_K = (1, 5, 9)                      # no compact layout below k = 10
SWEEP_K = CONTROL_K + COMPACT_K + WIDE_K
NULL_K = (11, 15, 16, 17, 19)           # k - 8 = 3, 7, 0, 1, 3 left over after spread_left's doubling; 16: the arm with nothing left
TAIL0_K = (11, 19)
FUZZ_K = (9, 10, 11, 13, 15, 17, 19)
LONGEST_K = (10, 16, 19)
TAIL_STEPS = (128, 131, 132, 135, 136, 143, 144)   # len - k: the last lengths of the tail plan's 4, 8 and 16 entries a read, and one past
GMEM_U = 32768                                      # k-mer positions of the longest read the classify chain takes
FIELDS = ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(s):
    return s[::-1].translate(_COMP)


def _blob(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8), off


# ---------------------------------------------------------------------------------------------------------------- the reads
@functools.lru_cache(maxsize=None)
def sweep_reads(k):
    """-> (reads, {len - k: indices of the reads of that length, for the TAIL_STEPS}, indices of the palindrome reads,
    indices of the reads with palindromic m-mers)"""
    rng = np.random.default_rng(7000 + k)
    rnd = lambda n: bytes(_ACGT[rng.integers(0, 4, size=n)])
    out, steps, pal, pmm = [], {}, [], []

    def add(r):
        out.append(r)
        return len(out) - 1

    for ln in (k - 1, k, k + 1):                               # no window, one, two
        for _ in range(3):
            add(rnd(ln))
    for d in (62, 63, 64, 65, 126, 127):                      # P = 63 .. 66: the first chunk's edge; P = 127, 128: no tail
        for _ in range(4):
            add(rnd(k + d))
    for d in TAIL_STEPS:                                      # P = 129 .. 145
        steps[d] = [add(rnd(k + d)) for _ in range(6)]
    for d in (159, 160):                                      # P = 160, 161: the class edge
        for _ in range(4):
            add(rnd(k + d))
    for P in (256, 257, 320, 321, 512, 513):
        add(rnd(P + k - 1))
    # reverse palindromes of k + 1 and k + 3 bases (one more at even k: a reverse palindrome has an even length): at odd k the
    # windows at their two ends are each other's reverse complement, one canonical k-mer at two neighbouring positions.  Placed
    # with the centre at 20, 64 and 100 and with the first window among the tail positions (128 and on)
    for extra in (1, 3):
        L = k + extra + ((k + extra) & 1)
        for where in (20, 64, 100, "tail0", "tail1"):
            for i in range(40):
                x = rnd(L // 2)
                p = x + _rc(x)
                if isinstance(where, int):
                    start, total = where - L // 2, 150
                else:
                    start, total = (129 if where == "tail0" else 134 + i % 6), k + 143
                r = rnd(start) + p + rnd(total - start - L)
                assert len(r) == total and r[start:start + L] == p
                pal.append(add(r))
    # m-mers that are their own reverse complement (m = k - 3 is even at odd k): x.rc(x), two a read at varied offsets, the read
    # and its reverse complement (the same k-mers with the other strand the canonical one)
    m = k - 3
    if k >= 10 and k % 2:
        for i in range(60):
            x, y = rnd(m // 2), rnd(m // 2)
            o1, gap = int(rng.integers(0, 60)), int(rng.integers(4, 30))
            r = rnd(o1) + x + _rc(x) + rnd(gap) + y + _rc(y)
            r = r + rnd(150 - len(r))
            pmm += [add(r), add(_rc(r))]
    for period in range(1, 7):                                # tandem repeats, homopolymers, one half twice
        for _ in range(2):
            add((rnd(period) * 150)[:150])
    out += [b"A" * 150, b"C" * 150, b"G" * (k + 131), b"T" * (k + 143), (b"AT" * 150)[:150], (b"CG" * 150)[:150]]
    for ln in (150, k + 135):
        x = rnd(ln // 2)
        add(x + x)
    for pos in (30, 90, 135):                                 # one N in the first chunk, the second, the tail
        r = rnd(k + 143)
        add(r[:pos] + b"N" + r[pos + 1:])
    r = rnd(k + 143)
    add(r[:30] + b"N" + r[31:90] + b"N" + r[91:135] + b"N" + r[136:])
    add(rnd(150).lower())
    r = rnd(k + 131)
    add(r[:70] + r[70:90].lower() + r[90:])
    return tuple(out), steps, tuple(pal), tuple(pmm)


def same_run_pairs(read, k):
    """The pairs of positions of a read with one canonical k-mer AND one minimizer position (test_k20_same_run_repeats.py): what the
    repeat filter can only tell apart by comparing the k-mers of a run with each other."""
    m = kmer_model.model(read, k)
    if m.valid.size < 2:
        return 0
    codes = kmer_model._CODE[np.frombuffer(read, dtype=np.uint8)]
    f, r = _kmers(np.where(codes > 3, 0, codes)[None, :], k)
    f, r = f[0], r[0]
    c, cr = np.minimum(f, r), np.maximum(f, r)
    j = _model_j(c, cr, k)
    q = np.arange(f.size) + np.where(f < r, j, W - 1 - j)
    n = 0
    for d in range(1, W):   # equal minimizer positions lie at most W - 1 apart
        n += int((m.valid[:-d] & m.valid[d:] & (c[:-d] == c[d:]) & (q[:-d] == q[d:])).sum())
    return n


@pytest.mark.parametrize("k", [k for k in SWEEP_K if k >= 10])   # (the filter's runs are the compact layout's: k >= 10)
def test_the_reads_hold_same_run_pairs_at_odd_k_only(k):
    reads, _, pal, _ = sweep_reads(k)
    if k % 2:
        assert sum(same_run_pairs(reads[i], k) > 0 for i in pal) >= 100
    else:
        assert sum(same_run_pairs(r, k) for r in reads) == 0


@pytest.mark.parametrize("k", [k for k in SWEEP_K if k >= 10 and k % 2])
def test_the_reads_hold_palindromic_minimizers_on_both_strands(k):
    """Through lmat_table_address (j sits in the tag): at least 50 k-mers whose chosen minimizer is its own reverse complement, met in
    windows whose forward strand is the canonical one and in windows where it is not."""
    from lmat_amd import capi
    lib = capi.load_library()
    reads, _, _, pmm = sweep_reads(k)
    m = k - 3
    nb, b, t = C.c_uint64(), C.c_uint32(), C.c_uint32()
    found, strands = set(), set()
    for i in pmm:
        md = kmer_model.model(reads[i], k)
        for p in np.nonzero(md.valid)[0].tolist():
            c = int(md.canon[p])
            assert lib.lmat_table_address(k, 1 << 20, c, C.byref(nb), C.byref(b), C.byref(t)) == 0
            j = ((t.value - 1) >> 7) & 3
            x = (c >> (2 * (W - 1 - j))) & ((1 << (2 * m)) - 1)
            if x == kmer_model.revcomp(x, m):
                found.add(c)
                strands.add(bool(md.fwd[p] < md.rev[p]))
    assert len(found) >= 50 and strands == {True, False}


# ------------------------------------------------------------------------------------------------------------- the database
def _menu(tax):
    s = [t for t in tax.ids if tax.rank[t] == "strain"]
    return [[s[0]], [s[0], s[1]], [s[0], s[1], s[2]], [s[3], s[4]], [s[9]], [s[0], s[3], s[30], s[31]]]


def kept_lists(kms, menu):
    """six of seven of these k-mers and the list of each, both by a hash of the k-mer's value -> (kept k-mers, their lists)"""
    h = (kms * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    keep = h % np.uint64(7) != 0
    return kms[keep], [menu[int(x) % len(menu)] for x in (h[keep] >> np.uint64(3)).tolist()]


def _database(outdir, k, reads=None):
    from lmat_amd import synth
    tax = synth.make_taxonomy(BR, specials=False)
    p = synth.write_aux_files(outdir, tax)
    kms = kmer_model.distinct_of(reads if reads is not None else sweep_reads(k)[0], k)
    p["kmers"] = kms
    p["kept"], p["lists"] = kept_lists(kms, _menu(tax))
    p["db"] = os.path.join(outdir, "sweep.bin")
    synth.write_taxhisto(p["db"], p["kept"], p["lists"], k)
    p["tax"] = tax
    return p


def _engine(p, k, prn_all=0, **kw):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=prn_all))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    eng.build_db(p["db"], k=k, **kw)
    return eng


def _oracle(p):
    import oracle_py
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.add_taxhisto(p["db"])
    orc.set_options()
    return orc


def _ran(eng, before):
    v, u = eng.variant_launches(), eng.uniform_launches()
    return (v["generic"] - before[0]["generic"], v["plain"] - before[0]["plain"], u - before[1])


def _default_runs(eng, k):
    """The run without candidates over all the reads, and over the reads of every TAIL_STEPS length as a batch of their own
    -> {"all" | len - k: (records, (generic, plain, uniform launches))}"""
    reads, steps, _, _ = sweep_reads(k)
    out = {}
    for name, idx in [("all", range(len(reads)))] + sorted(steps.items()):
        dr = eng.upload_reads([reads[i] for i in idx])
        before = (eng.variant_launches(), eng.uniform_launches())
        res, _ = eng.classify(dr, 0, len(idx), want_cands=False)
        out[name] = (res, _ran(eng, before))
        dr.free()
    return out


def _assert_fields(a, b, what, fields=FIELDS):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        bad = np.nonzero(x.view(f"u{x.dtype.itemsize}") != y.view(f"u{y.dtype.itemsize}"))[0]
        assert bad.size == 0, f"{what}: field {f} differs in {bad.size} records, first {int(bad[0])}: {x[bad[0]]} != {y[bad[0]]}"


def _assert_text(got, want, what):
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got.split("\n"), want.split("\n"))) if g != w]
    assert not bad, f"{what}: {len(bad)} differing records, first: {bad[0]}"
    assert got == want, what


class _Sweep:
    pass


@pytest.fixture(scope="module", params=SWEEP_K, ids=lambda k: f"k{k}")
def sweep(request, tmp_path_factory):
    from lmat_amd import Params
    s = _Sweep()
    s.k = k = request.param
    s.dir = str(tmp_path_factory.mktemp(f"sweep{k}"))
    s.reads = list(sweep_reads(k)[0])
    s.models = [kmer_model.model(r, k) for r in s.reads]
    s.p = _database(s.dir, k)
    s.blob, s.off = _blob(s.reads)
    s.orc = _oracle(s.p)
    s.want, s.tally, s.nomatch = s.orc.classify(s.blob, s.off, k)
    s.eng = _engine(s.p, k, prn_all=1)
    dr = s.eng.upload_reads((s.blob, s.off))
    s.full, s.cands = s.eng.classify(dr, 0, len(s.reads), want_cands=True, cand_cap=64 * len(s.reads))
    s.text = s.eng.format_out(s.full, s.cands, (s.blob, s.off))
    s.counts, s.got_nomatch = s.eng.counts()
    dr.free()
    s.eng.set_params(Params.run_rl(prn_all=0))
    s.runs = _default_runs(s.eng, k)
    yield s
    s.eng.close()
    s.orc.close()


@gpu
def test_p_run_against_the_oracle(sweep):
    s = sweep
    assert s.eng.k == s.k and (s.eng.table_bytes > 0)
    _assert_text(s.text, s.want, f"k = {s.k}, -p")
    assert s.got_nomatch == s.nomatch
    assert {t: c for t, (c, _) in s.counts.items()} == {t: c for t, (c, _) in s.tally.items()}
    assert int((s.full["status"] == 0).sum()) > len(s.reads) // 2 or s.k < 5      # (k = 1: two canonical 1-mers, one of them kept)


@gpu
def test_default_run_against_the_p_run(sweep):
    s = sweep
    _, steps, _, _ = sweep_reads(s.k)
    _assert_fields(s.runs["all"][0], s.full, f"k = {s.k}: default run vs -p run")
    for d, idx in steps.items():
        _assert_fields(s.runs[d][0], s.full[list(idx)], f"k = {s.k}: the reads of k + {d} bases alone vs -p run")


def _assert_found_counts(res, cands, models, lists, strains, what):
    """Without null models a candidate's score is float32(found) / float32(cand_kmer_cnt), found = the read's distinct k-mers whose
    list holds the taxid; the lists here hold strains only, which nothing is folded into.  So the -p pairs of every classified read
    must hold exactly the strains of its k-mers' lists (`lists`: {k-mer: list}, from the model's k-mers, not from a lookup), each
    with that quotient: a k-mer missed, found at another k-mer's address or counted twice changes one of them."""
    n = 0
    for i, m in enumerate(models):
        if res["status"][i] != 0:
            continue
        found = {}
        for x in m.distinct.tolist():
            for t in lists.get(x, ()):
                found[t] = found.get(t, 0) + 1
        got = cands[int(res["cand_off"][i]):int(res["cand_off"][i]) + int(res["n_cand"][i])]
        got = {int(t): sc for t, sc in zip(got["tid"].tolist(), got["score"]) if int(t) in strains}
        assert set(got) == set(found), f"{what}: strains among the candidates of read {i}: {sorted(got)}, the model's {sorted(found)}"
        for t, c in found.items():
            want = np.float32(c) / np.float32(m.distinct.size)
            assert got[t].view(np.uint32) == want.view(np.uint32), f"{what}: read {i}, taxid {t}: {got[t]}, model {c} of {m.distinct.size}"
        n += 1
    return n


@gpu
def test_against_the_model(sweep):
    """(cand_kmer_cnt is the number of the read's distinct valid k-mers, in the database or not -- lmat_hip.h --, so what the kept set
    decides is checked through the found counts behind the -p scores.)"""
    s = sweep
    lists = dict(zip(s.p["kept"].tolist(), s.p["lists"]))
    for name, res in (("-p", s.full), ("default", s.runs["all"][0])):
        want_valid = np.array([m.valid_kmers for m in s.models])
        bad = np.nonzero(res["valid_kmers"] != want_valid)[0]
        assert bad.size == 0, f"k = {s.k}, {name}: valid_kmers of read {int(bad[0])}: {res['valid_kmers'][bad[0]]}, model {want_valid[bad[0]]}"
        assert np.array_equal(res["read_len"], [len(r) for r in s.reads])
        for i, m in enumerate(s.models):
            if res["status"][i] == 0:
                assert int(res["cand_kmer_cnt"][i]) == m.distinct.size, f"k = {s.k}, {name}: cand_kmer_cnt of read {i} ({len(s.reads[i])} bases)"
                assert any(x in lists for x in m.distinct.tolist()), f"k = {s.k}, {name}: read {i} is classified without a k-mer in the database"
    strains = {t for l in _menu(s.p["tax"]) for t in l}
    n = _assert_found_counts(s.full, s.cands, s.models, lists, strains, f"k = {s.k}, -p")
    assert n == int((s.full["status"] == 0).sum()) and (n > len(s.reads) // 2 or s.k < 5)
    # the device's cpt_address (or, below k = 10, the wide table's hash): every distinct k-mer of the reads, kept or not
    kms = s.p["kmers"]
    counts, tids = s.eng.lookup(kms, stride=8)
    lists = dict(zip(s.p["kept"].tolist(), s.p["lists"]))
    for i, x in enumerate(kms.tolist()):
        want = lists.get(x, [])
        assert int(counts[i]) == len(want) and sorted(tids[i, :len(want)].tolist()) == sorted(want), f"k = {s.k}: lookup of {x:#x}"


@gpu
def test_kernel_variant_and_layout(sweep):
    """The generic kernel at every k but 20 (its variants are compiled for m = 17); at k = 20 the plain variant where the launch
    qualifies -- 4 tail entries a read: up to 132 positions --, in its fixed-geometry form for reads of one length of k + 128 .. k + 131."""
    s = sweep
    for name, (_, (generic, plain, uni)) in s.runs.items():
        if s.k != 20:
            assert plain == 0 and uni == 0, (s.k, name)
            if s.k >= 10 and name != "all":
                assert generic >= 1, (s.k, name)
            if s.k < 10:
                assert generic == 0, (s.k, name)      # the wide layout's instantiations are not the headline class
    if s.k == 20:
        assert s.runs[128][1] == (0, 1, 1) and s.runs[131][1] == (0, 1, 1)
        for d in (132, 135, 136, 143, 144):
            assert s.runs[d][1][1:] == (0, 0), d      # more than 4 tail entries a read, or no tail: the generic kernel
    print(f"k = {s.k}: (generic, plain, fixed-geometry) launches by batch {dict((n, r[1]) for n, r in s.runs.items())}, "
          f"{s.eng.table_bytes // 64} buckets, {'compact' if s.k >= 10 else 'wide'} layout")
    # the layout: compact from k = 10 on (the geometry's buckets and an overflow table of at least 1024), wide below
    buckets, n = s.eng.table_bytes // 64, int(s.p["kept"].size)
    if s.k >= 10:
        from lmat_amd import capi
        nb, b, t = C.c_uint64(), C.c_uint32(), C.c_uint32()
        assert capi.load_library().lmat_table_address(s.k, int(n / 6.4) + 1, 0, C.byref(nb), C.byref(b), C.byref(t)) == 0
        assert buckets >= nb.value + 1024
    else:
        assert buckets == max(16, int(n / (0.8 * 8)) + 1)


@gpu
def test_null_models(sweep, tmp_path):
    """The GC bin under null models: spread_left doubles a span up to k and adds what is left (nothing at k = 16)."""
    s = sweep
    if s.k not in NULL_K:
        return
    from lmat_amd import synth
    nm = os.path.join(str(tmp_path), "nm")
    lst = synth.write_null_models(nm, s.p["tax"], kmer_counts=(63, 128, 129, 144, 161, 257), seed=4100 + s.k)
    old = os.environ.get("LMAT_DIR")
    os.environ["LMAT_DIR"] = nm
    try:
        orc = _oracle(s.p)
        orc.load_null_models(lst)
        want, tally, nomatch = orc.classify(s.blob, s.off, s.k)
        orc.close()
        eng = _engine(s.p, s.k, prn_all=1)
        try:
            eng.load_null_models(lst)
            dr = eng.upload_reads((s.blob, s.off))
            res, cands = eng.classify(dr, 0, len(s.reads), want_cands=True, cand_cap=64 * len(s.reads))
            got = eng.format_out(res, cands, (s.blob, s.off))
            counts, got_nomatch = eng.counts()
            dr.free()
        finally:
            eng.close()
    finally:
        if old is None:
            del os.environ["LMAT_DIR"]
        else:
            os.environ["LMAT_DIR"] = old
    _assert_text(got, want, f"k = {s.k}, null models")
    assert got_nomatch == nomatch and {t: c for t, (c, _) in counts.items()} == {t: c for t, (c, _) in tally.items()}
    n = 0
    for i, m in enumerate(s.models):
        if m.tot > 0:
            n += 1
            assert int(res["bin_sel"][i]) == m.bin, f"k = {s.k}: GC bin of read {i} ({m.gc} of {m.tot})"
            assert int(res["valid_kmers"][i]) == m.valid_kmers
    assert n > len(s.reads) - 8 and len({m.bin for m in s.models}) >= 5     # (the homopolymers and repeats spread the bins)


@gpu
def test_without_the_tail_prepass(sweep):
    """LMAT_TAIL=0 (read once a process: a child): the reads' third chunk in the classify kernel itself, the same records."""
    s = sweep
    if s.k not in TAIL0_K:
        return
    with open(os.path.join(s.dir, "p.pkl"), "wb") as f:
        pickle.dump({x: s.p[x] for x in ("tree", "depth", "rank", "idmap", "db")}, f)
    fn = os.path.join(s.dir, "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), s.dir, str(s.k), fn], env=dict(os.environ, LMAT_TAIL="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    assert set(child) == set(s.runs)
    for name in s.runs:
        _assert_fields(child[name][0], s.runs[name][0], f"k = {s.k}, LMAT_TAIL=0, batch {name}", FIELDS + ("bin_sel",))


# ------------------------------------------------------------------------------------------------------------- the mini-fuzz
@gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("k", FUZZ_K)
def test_random_configuration_matches_oracle(k, seed, tmp_path, monkeypatch):
    """The body of test_gpu_fuzz.py at the k it never draws; null models for seed 0 of every k >= 10."""
    from lmat_amd import Engine, Params, synth
    import oracle_py
    rng = np.random.default_rng(50_000 + 100 * k + seed)
    branching = tuple(int(rng.integers(1, 4)) for _ in range(4)) + (int(rng.integers(2, 4)), int(rng.integers(1, 5)))
    G = int(rng.integers(300, 801))
    pool = [40, 75, 100, 150, 151, 179, 180, 250, 300, 531, 600]
    lens = [int(x) for x in rng.choice(pool, size=4)]
    tax = synth.make_taxonomy(branching, specials=bool(rng.integers(0, 2)))
    p = synth.write_aux_files(str(tmp_path), tax)
    genomes = synth.make_genomes(tax, G, 2002 + seed, strain_sub=float(rng.choice([0.002, 0.01, 0.05])),
                                 genus_block=float(rng.choice([0.0, 0.1, 0.4])))
    kmers, lists = synth.build_kmer_table(tax, genomes, k)
    p["db"] = os.path.join(str(tmp_path), "th.bin")
    synth.write_taxhisto(p["db"], kmers, lists, k)
    reads = synth.make_reads(tax, genomes, 150, lens, 3003 + seed, err=float(rng.choice([0.0, 0.01, 0.05])),
                             frac_random=0.1, frac_n=0.05, frac_lowc=0.03, frac_short=0.03, lower_frac=0.1)
    seqs = [r.encode() for _, r in reads]
    opts = dict(sdiff=float(rng.choice([0.5, 1.0, 2.0])), hbias=float(rng.choice([0.0, 3.0])), prn_all=int(rng.integers(0, 2)),
                screen_phix=int(rng.integers(0, 2)), min_score=float(rng.choice([0.0, 0.3])), min_kmer=int(rng.choice([1, 30, 35])),
                min_fnd_kmer=int(rng.choice([1, 3])))
    permissive = int(rng.integers(0, 4) == 0)
    use_map = bool(rng.integers(0, 4))
    null_lst = None
    if k >= 10 and seed == 0:
        null_lst = synth.write_null_models(os.path.join(str(tmp_path), "nm"), tax, seed=4004 + seed)
        monkeypatch.setenv("LMAT_DIR", os.path.join(str(tmp_path), "nm"))
    idmap = p["idmap"] if use_map else None
    eng = Engine(0, Params(opts["sdiff"], opts["hbias"], opts["min_score"], opts["min_kmer"], opts["min_fnd_kmer"], opts["prn_all"],
                           opts["screen_phix"]))
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], idmap)
    try:
        eng.load_taxonomy(p["tree"], p["depth"], p["rank"], idmap)
        if permissive:
            eng.set_label_modes(permissive=1)
            orc.set_label_modes(permissive=1)
        eng.build_db(p["db"], k=k)
        orc.add_taxhisto(p["db"])
        orc.set_options(**opts)
        if null_lst:
            eng.load_null_models(null_lst)
            orc.load_null_models(null_lst)
        blob, off = _blob(seqs)
        dr = eng.upload_reads((blob, off))
        res, cands = eng.classify(dr, cand_cap=512 * len(seqs))
        got = eng.format_out(res, cands, (blob, off), 0)
        want, tally, nm = orc.classify(blob, off, k, 0)
        _assert_text(got, want, f"k = {k}, seed {seed} ({branching}, {opts}, permissive={permissive}, null_models={bool(null_lst)})")
        counts, nomatch = eng.counts()
        assert nomatch == nm
        assert {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}
        assert np.array_equal(res["valid_kmers"], [kmer_model.model(r, k).valid_kmers for r in seqs])
        dr.free()
    finally:
        eng.close()
        orc.close()


# ------------------------------------------------------------------------------------------- the edges of the accepted range
@gpu
@pytest.mark.parametrize("k", LONGEST_K)
def test_the_longest_read_and_one_base_more(k, tmp_path):
    """GMEM_U k-mer positions are the longest read at every k: GMEM_U + k - 1 bases classify as the oracle has them, one base more is
    LMAT_E_CAPACITY from the blocking call and from a stream's submit, before anything is queued (the engine compares the lengths
    on the host: such a read never reaches a kernel), with this k's limit in the message, and the context goes on classifying."""
    from lmat_amd import Stream
    from lmat_amd.capi import LmatError
    rng = np.random.default_rng(900 + k)
    longest = bytes(_ACGT[rng.integers(0, 4, size=GMEM_U + k - 1)])
    over = longest + b"C"
    few = list(sweep_reads(k)[0][20:60])
    p = _database(str(tmp_path), k, reads=few + [longest[:3000]])
    orc = _oracle(p)
    eng = _engine(p, k, prn_all=1)
    message = f"read longer than {GMEM_U + k - 1} bases"
    try:
        def check(batch):
            blob, off = _blob(batch)
            dr = eng.upload_reads((blob, off))
            res, cands = eng.classify(dr, 0, len(batch), want_cands=True, cand_cap=4096 * len(batch))
            dr.free()
            _assert_text(eng.format_out(res, cands, (blob, off)), orc.classify(blob, off, k)[0], f"k = {k}")
            return res
        res = check(few[:3] + [longest])
        assert int(res["read_len"][3]) == GMEM_U + k - 1 and int(res["valid_kmers"][3]) == GMEM_U
        dr = eng.upload_reads(few[:3] + [over])
        with pytest.raises(LmatError) as ei:
            eng.classify(dr, 0, 4)
        dr.free()
        assert ei.value.code == -4 and message in str(ei.value)
        check(few)
        st = Stream(eng, max_reads=64, max_bases=40000, cands_per_read=64, n_slots=2)
        try:
            with pytest.raises(LmatError) as ei:
                st.submit(*_blob(few[:3] + [over]))
            assert ei.value.code == -4 and message in str(ei.value)
            assert st.next() is None
            blob, off = _blob(few)
            st.submit(blob, off)                                  # the slot went back untouched
            sres, scands, _ = st.next()
            _assert_text(eng.format_out(sres, scands, (blob, off)), orc.classify(blob, off, k)[0], f"k = {k}, streamed")
        finally:
            st.close()
    finally:
        eng.close()
        orc.close()


def _write_taxhisto_single(path, kmers, tid, k):
    """synth.write_taxhisto for one-taxid lists, vectorised: records of (u64 k-mer, u16 1, u32 taxid), the sanity word after every 1500"""
    import struct
    from lmat_amd import synth
    rec = np.zeros(kmers.size, dtype=np.dtype([("k", "<u8"), ("n", "<u2"), ("t", "<u4")]))
    assert rec.dtype.itemsize == 14
    rec["k"], rec["n"], rec["t"] = kmers, 1, tid
    raw = rec.view(np.uint8).reshape(-1, 14)
    full = kmers.size // 1500
    blocks = np.zeros((full, 1500 * 14 + 8), dtype=np.uint8)
    blocks[:, :1500 * 14] = raw[:full * 1500].reshape(full, 1500 * 14)
    blocks[:, 1500 * 14:] = 0xFF
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQIcI", 29, kmers.size, synth.SANITY, 999, b"N", k))
        f.write(blocks.tobytes())
        f.write(raw[full * 1500:].tobytes())


def _dense_kmers(k):
    rng = np.random.default_rng(1200 + k)
    if k == 10:   # the canonical 10-mers of a 400 kb random genome: about 280 k of the 524 800 there are
        from lmat_amd import synth
        return np.unique(synth.kmers_of(rng.integers(0, 4, size=400_000, dtype=np.uint8), k))
    x = rng.integers(0, 1 << (2 * k), size=4_400_000, dtype=np.uint64)   # k = 12: 3 M of the 8.4 M
    r, y = np.zeros_like(x), x.copy()
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (y & np.uint64(3)))
        y >>= np.uint64(2)
    u = np.unique(np.minimum(x, r))
    assert u.size > 3_000_000
    return np.sort(u[rng.permutation(u.size)[:3_000_000]])


@gpu
@pytest.mark.parametrize("k", [10, 12])
def test_a_dense_small_k_database_loads(k, tmp_path):
    """More k-mers than ten a bucket of the largest compact geometry (4^(k-3) buckets: 16 384 at k = 10, 262 144 at k = 12): a caller
    who fixed no size gets the wide layout, every k-mer looks up, and reads classify as the oracle has them.  A caller who fixed
    a size that cannot hold them keeps the error."""
    from lmat_amd import Engine, Params, synth
    from lmat_amd.capi import LmatError
    kms = _dense_kmers(k)
    assert kms.size > 10 * 4 ** (k - 3)
    tax = synth.make_taxonomy(BR, specials=False)
    p = synth.write_aux_files(str(tmp_path), tax)
    tid = [t for t in tax.ids if tax.rank[t] == "strain"][5]
    p["db"] = os.path.join(str(tmp_path), "dense.bin")
    _write_taxhisto_single(p["db"], kms, tid, k)
    eng = _engine(p, k, prn_all=1, table_bytes=0)
    orc = _oracle(p)
    try:
        assert eng.db_size == kms.size
        rng = np.random.default_rng(k)
        absent = np.setdiff1d(kmer_model.distinct_of([bytes(_ACGT[rng.integers(0, 4, size=3000)])], k), kms)
        for lo in range(0, kms.size, 1 << 20):
            counts, tids = eng.lookup(kms[lo:lo + (1 << 20)], stride=2)
            assert (counts == 1).all() and (tids[:, 0] == tid).all()
        counts, _ = eng.lookup(absent, stride=2)
        assert absent.size > 100 and (counts == 0).all()
        reads = list(sweep_reads(k)[0][:80])
        blob, off = _blob(reads)
        dr = eng.upload_reads((blob, off))
        res, cands = eng.classify(dr, 0, len(reads), want_cands=True, cand_cap=64 * len(reads))
        dr.free()
        _assert_text(eng.format_out(res, cands, (blob, off)), orc.classify(blob, off, k)[0], f"k = {k}, dense database")
        models = [kmer_model.model(r, k) for r in reads]
        in_db = set(kms.tolist())
        lists = {x: [tid] for m in models for x in m.distinct.tolist() if x in in_db}
        assert _assert_found_counts(res, cands, models, lists, {tid}, f"k = {k}, dense database") > 40
        assert all(int(res["cand_kmer_cnt"][i]) == m.distinct.size for i, m in enumerate(models) if res["status"][i] == 0)
    finally:
        eng.close()
        orc.close()
    eng = Engine(0, Params.run_rl())
    try:
        eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
        with pytest.raises(LmatError) as ei:
            eng.build_db(p["db"], k=k, table_bytes=64 * 1024, n_kmers_hint=int(kms.size))
        assert ei.value.code == -4 and "too small" in str(ei.value)
    finally:
        eng.close()


if __name__ == "__main__":   # the child of test_without_the_tail_prepass: the default runs with whatever LMAT_TAIL says, pickled
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    with open(os.path.join(sys.argv[1], "p.pkl"), "rb") as _f:
        _p = pickle.load(_f)
    _k = int(sys.argv[2])
    _e = _engine(_p, _k)
    _out = _default_runs(_e, _k)
    _e.close()
    with open(sys.argv[3], "wb") as _f:
        pickle.dump(_out, _f)
