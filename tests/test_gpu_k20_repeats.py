"""GPU: 150 bp reads built against the even-k argument of the PLAIN/UNI repeat filter (kernels.hip, classify_one, "repeats"; the
claim itself: test_k20_same_run_repeats.py).  The plain variants no longer compare k-mer digests inside a run, so a k-mer that
recurs in a read must still be found through the two bucket filters: tandem repeats of period 1 .. 6, reads X.rc(X) with the centre
at every offset from 60 to 90 -- plain, with one N and with one substitution near the centre --, homopolymers and a read that ends
in its own first 40 bases (the recurrences lie in the looked-up tail).  Every k-mer of these reads is in the database with a list
chosen by the k-mer's value (one in seven is left out), so a repeat counted twice shows in the candidate counts and the scores.

The fixed-geometry variant (every read 150 bp), the plain variant (the same reads and one short one) and the generic kernel
(LMAT_PLAIN=0, a child process; and the -p launch here) must give the same records, and the -p launch the CPU oracle's text."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BR = (3, 4, 4, 4, 4, 3)
K = 20
L = 150


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def _reads():
    rng = np.random.default_rng(4242)
    rnd = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])
    out = []
    for period in range(1, 7):                       # tandem repeats, three units a period
        for _ in range(3):
            out.append((rnd(period) * L)[:L])
    out += [b"A" * L, b"T" * L, b"C" * L, (b"AT" * L)[:L], (b"ACGT" * L)[:L], (b"CG" * L)[:L]]   # homopolymers; units that are their own reverse complement
    for centre in range(60, 91):                     # X.rc(X): `centre` bases, their reverse complement, then random bases
        x = rnd(centre)
        pal = (x + _rc(x) + rnd(L))[:L]
        out.append(pal)
        p = centre + int(rng.integers(-3, 4))
        out.append(pal[:p] + b"N" + pal[p + 1:])
        p = centre + int(rng.integers(-4, 4))
        out.append(pal[:p] + bytes([b"ACGT"[(b"ACGT".index(pal[p]) + int(rng.integers(1, 4))) & 3]]) + pal[p + 1:])
    for _ in range(3):                               # the first 40 bases again at the end: recurrences in the tail entries
        x = rnd(L - 40)
        out.append(x + x[:40])
    x = rnd(75)
    out.append(x + x)                                # ... and a read that is one half twice
    out += [rnd(L) for _ in range(8)]                # nothing special
    assert all(len(r) == L for r in out)
    return out


def _database(outdir):
    """Taxonomy files and a tax_histo file with a list for six of seven distinct k-mers of the reads -> paths."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    from lmat_amd import synth
    tax = synth.make_taxonomy(BR, specials=False)
    p = synth.write_aux_files(outdir, tax)
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    kms = np.unique(np.concatenate([orc.extract(r, K)[0] for r in _reads()]))
    orc.close()
    s = [t for t in tax.ids if tax.rank[t] == "strain"]
    menu = [[s[0]], [s[0], s[1]], [s[0], s[1], s[2]], [s[3], s[4]], [s[9]], [s[0], s[3], s[30], s[31]]]
    h = (kms * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    keep = h % np.uint64(7) != 0
    p["db"] = os.path.join(outdir, "repeats.bin")
    synth.write_taxhisto(p["db"], kms[keep], [menu[int(x) % len(menu)] for x in (h[keep] >> np.uint64(3)).tolist()], K)
    return p


def _engine(p):
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.load_taxonomy(p["tree"], p["depth"], p["rank"], p["idmap"])
    eng.build_db(p["db"], k=K)
    return eng


def _run(eng):
    """-> {"uni": records of the reads alone, "plain": records of the reads and a short one, "ran": the kernels that ran}"""
    out = {}
    for name, reads in (("uni", _reads()), ("plain", _reads() + [b"ACGTTGCAAC" * 6])):
        dr = eng.upload_reads(reads)
        v0, u0 = eng.variant_launches(), eng.uniform_launches()
        res, _ = eng.classify(dr, 0, len(reads), want_cands=False)
        v1, u1 = eng.variant_launches(), eng.uniform_launches()
        dr.free()
        out[name] = res
        out[name + "_ran"] = (v1["generic"] - v0["generic"], v1["plain"] - v0["plain"], u1 - u0)
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert os.environ.get("LMAT_PLAIN") in (None, "1"), "this module compares the default with LMAT_PLAIN=0 itself"
    d = str(tmp_path_factory.mktemp("repeats"))
    p = _database(d)
    eng = _engine(p)
    here = _run(eng)
    fn = os.path.join(d, "child.pkl")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), d, fn], env=dict(os.environ, LMAT_PLAIN="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(fn, "rb") as f:
        child = pickle.load(f)
    yield p, eng, here, child
    eng.close()


def _assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    for f in a.dtype.names:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        bad = np.nonzero(x.view(f"u{x.dtype.itemsize}") != y.view(f"u{y.dtype.itemsize}"))[0]
        assert bad.size == 0, f"{what}: field {f} differs in {bad.size} records, first {int(bad[0])}: {x[bad[0]]} != {y[bad[0]]}"


def test_plain_variants_against_the_generic_kernel(runs):
    _, _, here, child = runs
    assert here["uni_ran"] == (0, 1, 1) and here["plain_ran"] == (0, 1, 0)          # fixed geometry; plain
    assert child["uni_ran"] == (1, 0, 0) and child["plain_ran"] == (1, 0, 0)
    n = len(_reads())
    _assert_same(here["uni"], child["uni"], "fixed-geometry variant vs LMAT_PLAIN=0")
    _assert_same(here["plain"], child["plain"], "plain variant vs LMAT_PLAIN=0")
    _assert_same(here["uni"], here["plain"][:n], "fixed-geometry variant vs plain variant")
    res = here["uni"]
    assert (res["status"] == 0).sum() > n // 2                                          # most of these reads are classified
    assert (res["cand_kmer_cnt"][:18] < 8).all()                                         # tandem repeats: at most 6 distinct k-mers, counted once


def test_against_the_oracle(runs):
    p, eng, here, _ = runs
    import oracle_py
    from lmat_amd import Params
    reads = _reads()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    blob = np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8)
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.add_taxhisto(p["db"])
    orc.set_options()
    want, _, _ = orc.classify(blob, off, K)
    orc.close()
    eng.set_params(Params.run_rl(prn_all=1))
    dr = eng.upload_reads((blob, off))
    v0 = eng.variant_launches()
    full, cands = eng.classify(dr, 0, len(reads), want_cands=True, cand_cap=64 * len(reads))
    assert eng.variant_launches()["plain"] == v0["plain"]                                # -p: the generic kernel
    got = eng.format_out(full, cands, (blob, off))
    dr.free()
    eng.set_params(Params.run_rl(prn_all=0))
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got.split("\n"), want.split("\n"))) if g != w]
    assert not bad, f"{len(bad)} differing records, first: {bad[0]}"
    assert got == want
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "log_avg", "stdev", "call_tid", "call_score", "bin_sel"):
        x, y = np.ascontiguousarray(here["uni"][f]), np.ascontiguousarray(full[f])
        assert np.array_equal(x.view(f"u{x.dtype.itemsize}"), y.view(f"u{y.dtype.itemsize}")), f


if __name__ == "__main__":   # the child of the `runs` fixture: the same launches with whatever LMAT_PLAIN says, pickled
    sys.path.insert(0, ROOT)
    _d = os.path.join(sys.argv[1], "child")
    os.makedirs(_d)
    _e = _engine(_database(_d))
    _out = _run(_e)
    _e.close()
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_out, _f)
