"""GPU: the per-group k-mer coverage (lmat_cov_*, kcov.hip) against the Python statement of its contract (tests/kcov_model.py, pinned to
the reference's own reports by tests/test_kcov_model.py), and content_summ -G against the reference's example run byte for byte."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import kcov_model as km
from test_kcov_model import K_SIZES, cs_argv, example_inputs, select_example_reads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 8, 17, 20, 21, 31, 8]
E_ARG, E_CAPACITY = -1, -4
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(s):
    return s.translate(COMP)[::-1]


def _trap_input():
    """(reads, groups): every trap of the issue.  Eight groups (3 bits: k = 31 takes the two-sort form), ids 0 and 2^32 - 1 among them."""
    rnd = random.Random(20240611)
    dna = lambda n: bytes(rnd.choice(b"ACGT") for _ in range(n))
    G = [0, 1, 7, 9606, 70000, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    reads, groups = [], []

    def add(r, g):
        reads.append(bytes(r))
        groups.append(g)

    add(b"", G[0])
    add(b"", G[7])
    for k in sorted(set(KS)):                                   # k - 1, k, k + 1
        for n in (k - 1, k, k + 1):
            add(dna(n), G[1])
    for n in (15, 16, 17, 63, 64, 65, 991, 992, 993):          # load, wave and span boundaries of the extraction
        add(dna(n), G[2])
        add(b"N" + dna(n - 2) + b"N", G[2])
    s = dna(120)
    add(b"N" + s, G[3])                                         # other bytes first, last and mid-read
    add(s + b"N", G[3])
    add(s[:60] + b"N" + s[60:], G[3])
    add(s[:40] + b"-" + s[40:80] + b"\x00" + s[80:] + b"\xff", G[3])
    add(s.lower(), G[3])
    add(s[:50] + s[50:].lower(), G[3])
    j = dna(62)                                                 # two adjacent reads whose junction would spell valid k-mers
    add(j[:31], G[4])
    add(j[31:], G[4])
    pal = dna(10)
    add(pal + _rc(pal), G[4])                                   # a palindromic window: forward == reverse complement for k = 20
    add(b"ACGT" * 2, G[4])                                      # ... and for k = 8
    add(b"A" * 300, G[5])                                       # homopolymer, tandem repeat
    add(b"ACG" * 100, G[5])
    tw = dna(200)
    add(tw, G[6])                                               # the same read twice in one group: multiplicity 2
    add(tw, G[6])
    add(tw, G[7])                                               # ... and once more in another: 1 there
    add(_rc(tw), G[5])
    rcr = dna(150)
    add(rcr, G[0])                                              # a read and its reverse complement in one group
    add(_rc(rcr), G[0])
    add(dna(5000), G[7])
    genomes = [dna(700), dna(900), dna(1100)]
    for i in range(1000):                                       # ~1000 reads of 1..300 bp from three genomes: 2 % errors, 1 % N
        g = genomes[i % 3]
        n = rnd.randint(1, 300)
        p = rnd.randint(0, len(g) - 1)
        r = bytearray(g[p:p + n])
        if rnd.random() < 0.5:
            r = bytearray(_rc(bytes(r)))
        for x in range(len(r)):
            u = rnd.random()
            if u < 0.02:
                r[x] = rnd.choice(b"ACGT")
            elif u < 0.03:
                r[x] = 78
        add(r, G[i % 3])
    for n in (1, 3, 7, 5, 2):                                   # a group whose reads are all shorter than every k but 1
        add(dna(n), 424242)
    return reads, groups


@pytest.fixture(scope="module")
def eng():
    from lmat_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def trap():
    reads, groups = _trap_input()
    want, st = km.coverage(reads, groups, KS)
    return reads, groups, want, st


def _cover(eng, reads, groups, ks=KS, budget=0, prefix_bits=-1, batch=None):
    from lmat_amd import Coverage
    c = Coverage(eng, ks)
    try:
        c.set_options(budget, prefix_bits)
        step = batch or max(len(reads), 1)
        for i in range(0, len(reads), step):
            c.add_reads(reads[i:i + step], groups[i:i + step])
        st = c.run()
        return c.report(), st
    finally:
        c.close()


def test_traps_against_the_model(eng, trap):
    reads, groups, want, wst = trap
    assert len(set(groups)) >= 6 and 0 in groups and 2 ** 32 - 1 in groups
    assert any(m > 1 for k in want.values() for g in k.values() for m, _ in g[2])
    assert 424242 in want[0] and all(424242 not in want[ki] for ki in range(1, len(KS)))
    got, st = _cover(eng, reads, groups, budget=1 << 30)      # room for every k in one pass, whatever is free on the device
    for ki in range(len(KS)):
        assert got[ki] == want[ki], (ki, KS[ki])
    assert (st["reads"], st["bases"], st["windows"], st["runs"]) == (wst["reads"], wst["bases"], wst["windows"], wst["runs"])
    assert st["prefix_bits"] == 0 and st["passes"] == len(KS)


@pytest.mark.parametrize("pb", [0, 1, 3, 5])
def test_invariance_prefix_bits(eng, trap, pb):
    reads, groups, want, wst = trap
    got, st = _cover(eng, reads, groups, prefix_bits=pb)
    assert got == want
    assert st["passes"] == sum(1 << min(pb, 2 * k) for k in KS) and st["windows"] == wst["windows"] and st["runs"] == wst["runs"]


def test_invariance_budget_batches_order(eng, trap):
    from lmat_amd import LmatError
    reads, groups, want, wst = trap
    bases = sum(len(r) for r in reads) + len(reads)
    # The model of DESIGN 11: fixed buffers (text, 12 B per read, 16 B per wave, 64 KiB) + 64 or 80 B per window occurrence.  Room for about
    # 0.7 windows per base: k = 1 (every base a window, two canonical k-mers) fits only split, every k derives a split above 0.
    fixed = bases + 2048 + 12 * len(reads) + 16 * (bases // 992 + 2) + (64 << 10)
    budget = fixed + int(0.7 * bases) * 80
    got, st = _cover(eng, reads, groups, budget=budget)
    assert got == want and st["prefix_bits"] > 0 and st["windows"] == wst["windows"]
    with pytest.raises(LmatError) as ei:
        _cover(eng, reads, groups, budget=budget, prefix_bits=0)
    assert ei.value.code == E_CAPACITY
    for batch in (1, 7):
        assert _cover(eng, reads, groups, batch=batch)[0] == want
    assert _cover(eng, reads[::-1], groups[::-1])[0] == want


def test_chunked_text(eng, trap):
    """a budget a 64th of which is below the text: the text goes up in chunks (here two), for every pass again"""
    reads, groups, want, wst = trap
    bases = sum(len(r) for r in reads) + len(reads)
    budget = 48 * bases                      # leaves about 0.7 window occurrences per base, as above
    assert (1 << 16) < budget // 64 < bases
    got, st = _cover(eng, reads, groups, budget=budget)
    assert got == want and st["windows"] == wst["windows"] and st["prefix_bits"] > 0


def test_errors_and_conventions(eng):
    from lmat_amd import Coverage, LmatError
    lib = eng.lib
    for ks in ([0], [32], [8, -1], []):
        with pytest.raises(LmatError) as ei:
            Coverage(eng, ks)
        assert ei.value.code == E_ARG
    h = C.c_void_p()
    assert lib.lmat_cov_create(eng.ctx, None, 1, C.byref(h)) == E_ARG
    c = Coverage(eng, [4, 4])
    n = C.c_uint64(99)
    assert lib.lmat_cov_summary(c.h, 0, None, None, None, 0, C.byref(n)) == E_ARG       # fetch before the run
    assert lib.lmat_cov_histogram(c.h, 0, 1, None, None, 0, C.byref(n)) == E_ARG
    blob = np.frombuffer(b"ACGTACGTAC\0", dtype=np.uint8)
    off = np.array([0, 6, 10], dtype=np.uint64)
    grp = np.array([5, 6], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.lmat_cov_add_reads(c.h, None, p(off), 2, p(grp)) == E_ARG
    assert lib.lmat_cov_add_reads(c.h, p(blob), None, 2, p(grp)) == E_ARG
    assert lib.lmat_cov_add_reads(c.h, p(blob), p(off), 2, None) == E_ARG
    bad = np.array([0, 6, 5], dtype=np.uint64)
    assert lib.lmat_cov_add_reads(c.h, p(blob), p(bad), 2, p(grp)) == E_ARG             # ... and a failed call adds nothing
    assert lib.lmat_cov_add_reads(c.h, None, None, 0, None) == 0
    # more than 2^32 - 1 reads in total: the count is checked before any array is read, so small arrays will do; nothing is added
    assert lib.lmat_cov_add_reads(c.h, p(blob), p(off), 2 ** 32, p(grp)) == E_CAPACITY
    with pytest.raises(LmatError) as ei:
        c.set_options(0, 25)
    assert ei.value.code == E_ARG
    assert lib.lmat_cov_add_reads(c.h, p(blob), p(off), 2, p(grp)) == 0
    assert lib.lmat_cov_add_reads(c.h, p(blob), p(off), 2 ** 32 - 2, p(grp)) == E_CAPACITY   # 2 + (2^32 - 2): the total counts
    st = c.run()                                                                         # ... and none of the refused calls left a read
    assert st["reads"] == 2 and st["bases"] == 10
    want, _ = km.coverage([b"ACGTAC", b"GTAC"], [5, 6], [4, 4])
    assert c.report() == want
    # a cap of 0 asks for the size; *n is set with LMAT_E_CAPACITY
    assert lib.lmat_cov_summary(c.h, 0, None, None, None, 0, C.byref(n)) == E_CAPACITY and n.value == 2
    g1, d1, t1 = (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64))
    assert lib.lmat_cov_summary(c.h, 0, p(g1), p(d1), p(t1), 1, C.byref(n)) == E_CAPACITY and n.value == 2
    assert lib.lmat_cov_histogram(c.h, 1, 5, None, None, 0, C.byref(n)) == E_CAPACITY and n.value == len(want[1][5][2])
    assert lib.lmat_cov_histogram(c.h, 0, 777, None, None, 0, C.byref(n)) == 0 and n.value == 0   # a group the summary does not list
    assert lib.lmat_cov_summary(c.h, 2, None, None, None, 0, C.byref(n)) == E_ARG
    with pytest.raises(LmatError) as ei:
        c.run()                                                                          # once per object
    assert ei.value.code == E_ARG
    c.close()
    c = Coverage(eng, [8])                                                               # run without reads
    st = c.run()
    assert st["reads"] == 0 and st["windows"] == 0 and c.report() == {0: {}}
    c.close()
    c = Coverage(eng, [8])                                                               # reads without a single k-mer
    c.add_reads([b"", b"ACG", b"NNNNNNNNNNNN"], [1, 2, 3])
    st = c.run()
    assert st["reads"] == 3 and st["windows"] == 0 and c.report() == {0: {}}
    c.close()


def _cs(tmp_path, out, extra=(), env_extra=None):
    env = dict(os.environ)
    env.pop("LMAT_CS_GPU", None)
    env.pop("LMAT_LIB", None)
    env.update(env_extra or {})
    r = subprocess.run(cs_argv(tmp_path, out) + list(extra), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    base = os.path.basename(out)
    files = {f[len(base):]: open(os.path.join(str(tmp_path), f)).read() for f in os.listdir(str(tmp_path)) if f.startswith(base)}
    return r.stdout, files


def test_content_summ_on_the_device_reproduces_the_reference_example(tmp_path):
    T, _ = example_inputs(tmp_path)
    reads, _tids = select_example_reads(tmp_path, T)
    want = {k[len(".summ"):]: v for k, v in T["files"].items() if k == ".summ" or k.endswith("_kmer_cov")}
    _, host = _cs(tmp_path, str(tmp_path / "host.summ"))
    assert host == want
    for i, (extra, env) in enumerate(((["-G"], {}), ([], {"LMAT_CS_GPU": "1"}))):
        stdout, dev = _cs(tmp_path, str(tmp_path / f"dev{i}.summ"), extra, env)
        assert dev == want and dev == host                      # same set of files (empty ones included), same bytes
        line = [l for l in stdout.splitlines() if l.startswith("kmer coverage on device: ")]
        assert len(line) == 1 and stdout.splitlines()[-2] == line[0] and stdout.splitlines()[-1].startswith("query time: ")
        f = dict(x.split("=") for x in line[0].split(": ")[1].split())
        assert int(f["reads"]) == len(reads) and int(f["passes"]) == len(K_SIZES) and int(f["windows"]) > 0


def test_python_kmer_coverage(eng, trap):
    reads, groups = trap[0][-60:-10], trap[1][-60:-10]
    want, wst = km.coverage(reads, groups, [5, 12])
    got, st = eng.kmer_coverage(reads, groups, [5, 12])
    assert len(reads) == 50 and got == want and st["windows"] == wst["windows"] and st["reads"] == 50
