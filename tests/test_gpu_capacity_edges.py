"""GPU: every capacity edge of the classify chain, by single reads (capacity_probes.py; the probes are proved on the CPU by
test_capacity_probes.py).  A read on a capacity stays in its class, a read one above it is listed on the device and re-run by the
class behind it -- with the same record, tallied exactly once, leaving no candidates behind -- and a read beyond the last class is
LMAT_E_CAPACITY.  The routing expectations come from the table in capacity_probes.py, not from the engine."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import capacity_probes as cp

pytestmark = pytest.mark.gpu

# LMAT_MID_TIER=0 (a child run below): the chain without the middle tier -- capacity_probes.route(mid_on=False)
MID_ON = os.environ.get("LMAT_MID_TIER") is None or int(os.environ["LMAT_MID_TIER"]) != 0
CAPACITY_MESSAGE = "a read exceeds the largest tables"


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def _classify(eng, dr, first, count, cand_cap):
    """Engine.classify with the number of candidates the launch returned (lmat_classify's n_cands)."""
    from lmat_amd.capi import CAND_DTYPE, READ_RESULT_DTYPE
    res = np.zeros(count, dtype=READ_RESULT_DTYPE)
    cands = np.zeros(cand_cap, dtype=CAND_DTYPE)
    n = C.c_uint64(0)
    eng._chk(eng.lib.lmat_classify(eng.ctx, dr.h, first, count, res.ctypes.data_as(C.c_void_p), cands.ctypes.data_as(C.c_void_p),
                                   cand_cap, C.byref(n)))
    return res, cands, int(n.value)


def _assert_tallies(got, tally, nm, n_reads):
    """eng.counts() against the oracle's: counts and no-match counters exactly; the score sums within the rounding of the oracle's
    float accumulation (n additions, each within 2^-24 of the running sum; the engine adds the same float scores in double)."""
    counts, nomatch = got
    assert list(nomatch) == [int(x) for x in nm]
    assert {t: c for t, (c, _) in counts.items()} == {int(t): int(c) for t, (c, _) in tally.items()}
    for t, (_, s) in tally.items():
        assert abs(counts[int(t)][1] - s) <= max(n_reads, 1) * 2.0 ** -23 * max(abs(s), 1.0), (t, counts[int(t)][1], s)


def _same_records(got, want):
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "call_tid", "bin_sel"):
        assert (got[f] == want[f]).all(), f
    for f in ("call_score", "stdev"):
        assert (got[f].view(np.uint32) == want[f].view(np.uint32)).all(), f


def _expected_counters(probes, max_len, wide):
    out = dict.fromkeys(cp.COUNTERS, 0)
    for p in probes:
        for name, v in cp.route(p.dims, max_len, wide, MID_ON)[1].items():
            out[name] += v
    return out


class _Bench:
    """One engine and one oracle on a probe database; what the oracle says of a read or a batch is computed once and kept."""

    def __init__(self, outdir, wide):
        import oracle_py
        from lmat_amd import Engine, Params
        self.ps = cp.build_set(outdir, wide)
        self.wide = wide
        self.probes = [p for p in self.ps["probes"] if p.axis != "error"]
        self.beyond = {p.name: p for p in self.ps["probes"] if p.axis == "error"}
        self.eng = Engine(0, Params.run_rl())
        self.eng.load_taxonomy(self.ps["tree"], self.ps["depth"], self.ps["rank"], self.ps["idmap"])
        self.eng.build_db(self.ps["db"], k=cp.K)
        self.orc = oracle_py.Oracle(self.ps["tree"], self.ps["depth"], self.ps["rank"], self.ps["idmap"])
        self.orc.add_taxhisto(self.ps["db"])
        self.orc.set_options()
        self._want = {}

    def want(self, probes):
        """-> (.out text, tally, no-match counters) of the oracle for these probes as one batch."""
        key = tuple(p.name for p in probes)
        if key not in self._want:
            self._want[key] = self.orc.classify(*_blob([p.read for p in probes]), cp.K)
        return self._want[key]

    def groups(self):
        """The probes by the upload that takes them alone: a launch's tiers depend on the longest read of its read set, so the
        150 bp probes (one length class: the plain-run variant of the fast class takes them), the length-crossed ones (mixed
        classes, up to 531 bp) and the long ones are three sets."""
        g = {"p131": [p for p in self.probes if p.axis in ("T", "E", "D", "plain")], "len": [p for p in self.probes if p.axis == "P"],
             "long": [p for p in self.probes if p.axis == "long"]}
        assert sum(len(v) for v in g.values()) == len(self.probes)
        return {k: v for k, v in g.items() if v}

    def run(self, probes, cand_cap=None):
        """One blocking launch over these probes as a read set of their own -> (results, text, n_cands, tallies, counters)."""
        blob, off = _blob([p.read for p in probes])
        dr = self.eng.upload_reads((blob, off))
        try:
            self.eng.counts_reset()
            res, cands, n = _classify(self.eng, dr, 0, len(probes), cand_cap or sum(p.T for p in probes) + 64)
            return res, self.eng.format_out(res, cands, (blob, off)), n, self.eng.counts(), self.eng.last_counters()
        finally:
            dr.free()

    def close(self):
        self.orc.close()
        self.eng.close()


@pytest.fixture(scope="module")
def bench16(tmp_path_factory):
    b = _Bench(str(tmp_path_factory.mktemp("edges16")), wide=False)
    yield b
    b.close()


@pytest.fixture(scope="module")
def bench_wide(tmp_path_factory):
    b = _Bench(str(tmp_path_factory.mktemp("edges_wide")), wide=True)
    yield b
    b.close()


# ---- a. each probe alone ---------------------------------------------------------------------------------------------------
def _each_probe_alone(b):
    from lmat_amd.capi import LmatError
    bad = []
    for gname, probes in b.groups().items():
        blob, off = _blob([p.read for p in probes])
        max_len = max(len(p.read) for p in probes)
        dr = b.eng.upload_reads((blob, off))
        for i, p in enumerate(probes):
            text, tally, nm = b.orc.classify(*_blob([p.read]), cp.K, i)
            b.eng.counts_reset()
            try:
                res, cands, n = _classify(b.eng, dr, i, 1, 4200)
            except LmatError as e:
                bad.append("%s (T %d, E %d, D %d, P %d; %s): %s" % (p.name, p.T, p.E, p.D, p.P, p.expected, e))
                continue
            one = _blob([p.read])
            got = b.eng.format_out(res, cands, one, i)
            flow = b.eng.last_counters()
            try:
                assert got == text                                                    # the record and its candidates, byte for byte
                _assert_tallies(b.eng.counts(), tally, nm, 1)                         # tallied exactly once
                assert n == int(res["n_cand"][0]) == p.T                              # nothing left behind by a class that gave it up
                if p.P <= 512:
                    where, want = cp.route(p.dims, max_len, b.wide, MID_ON)
                    assert flow == want, (flow, want, where)
                    if MID_ON and p.P > 0:
                        assert where == p.expected
            except AssertionError as e:
                bad.append("%s (T %d, E %d, D %d, P %d; %s): %s" % (p.name, p.T, p.E, p.D, p.P, p.expected, str(e)[:300]))
        dr.free()
    assert not bad, "\n".join(bad)


def test_each_probe_alone_16bit(bench16):
    _each_probe_alone(bench16)


def test_each_probe_alone_wide(bench_wide):
    _each_probe_alone(bench_wide)


def test_fast_class_edges_in_the_plain_variant_16bit(bench16):
    """Without a candidate buffer the 150 bp probes -- one length class with a four-position tail -- are the launch the plain-run
    variant of the fast class has compiled in; LMAT_PLAIN=0, LMAT_TAIL=0 and LMAT_K4_WAVE=0 (three of the child runs below) send it
    to the generic kernel instead.  The whole group as one queued launch, then the probes on and one above the fast class's
    capacities alone: the records of the blocking launch, the oracle's tallies, the counters of the table."""
    from lmat_amd import Params
    b = bench16
    probes = b.groups()["p131"]
    res0 = b.run(probes)[0]
    generic = any(os.environ.get(v) == "0" for v in ("LMAT_PLAIN", "LMAT_TAIL", "LMAT_K4_WAVE"))
    ran, idle = ("generic", "plain") if generic else ("plain", "generic")
    dr = b.eng.upload_reads(_blob([p.read for p in probes]))
    b.eng.set_params(Params.run_rl(prn_all=0))
    try:
        edge = [i for i, p in enumerate(probes) if p.name in ("T63", "T64", "T64tie", "T65", "TL64", "TL65", "E255", "E256", "E257", "D64", "D65", "one_hit", "no_hit", "short")]
        assert len(edge) == 14
        for first, count in [(0, len(probes))] + [(i, 1) for i in edge]:
            sub = probes[first:first + count]
            _, tally, nm = b.want(sub)
            before = b.eng.variant_launches()
            b.eng.counts_reset()
            b.eng.classify_async(dr, first, count)
            b.eng.sync()
            after = b.eng.variant_launches()
            assert after[ran] == before[ran] + 1 and after[idle] == before[idle], (before, after)
            _same_records(b.eng.fetch_results(0, count), res0[first:first + count])
            _assert_tallies(b.eng.counts(), tally, nm, count)
            assert b.eng.last_counters() == _expected_counters(sub, 150, False), [p.name for p in sub]
    finally:
        b.eng.set_params(Params.run_rl())
        dr.free()


# ---- b. all probes in one batch ----------------------------------------------------------------------------------------------
def _batch(b, probes):
    max_len = max(len(p.read) for p in probes)
    text, tally, nm = b.want(probes)
    res, got, n, counts, flow = b.run(probes)
    assert got == text
    _assert_tallies(counts, tally, nm, len(probes))
    assert n == int(res["n_cand"].sum()) == sum(p.T for p in probes)
    assert flow == _expected_counters(probes, max_len, b.wide), (flow, _expected_counters(probes, max_len, b.wide))
    return res, (tally, nm)


def _orders(probes):
    shuffled = list(probes)
    random.Random(4711).shuffle(shuffled)
    return {"as_built": list(probes), "reversed": list(probes)[::-1], "shuffled": shuffled}


@pytest.mark.parametrize("order", ["as_built", "reversed", "shuffled"])
def test_all_probes_in_one_batch_16bit(bench16, order):
    """The longest probe has 2068 bp: the launch has neither the middle tier (off above 531 bp) nor the large LDS class (off above
    2067 bp), and the counters are the sum of every probe's walk down that shorter chain."""
    probes = _orders(bench16.probes)[order]
    assert max(len(p.read) for p in probes) == 2068 and len(probes) <= 150
    _batch(bench16, probes)


@pytest.mark.parametrize("order", ["as_built", "reversed", "shuffled"])
def test_all_probes_in_one_batch_wide(bench_wide, order):
    _batch(bench_wide, _orders(bench_wide.probes)[order])


@pytest.mark.parametrize("order", ["as_built", "reversed", "shuffled"])
def test_short_probes_in_one_batch_16bit(bench16, order):
    """Without the long probes (no read above 531 bp) the launch has every tier: the counters are the sum of the per-probe
    expectations of the probes launched alone."""
    g = bench16.groups()
    probes = _orders(g["p131"] + g["len"])[order]
    assert max(len(p.read) for p in probes) == 531
    _batch(bench16, probes)


def test_long_probes_in_batches_of_their_own_16bit(bench16):
    """The long probes alone (2068 bp: the chain ends in the global-memory class), and the short ones with the 532 bp probes (no
    middle tier) and with the 2067 bp probes (the longest batch that still has the large LDS class)."""
    g = bench16.groups()
    _batch(bench16, g["long"])
    for L in (532, 2067):
        probes = g["p131"] + [p for p in g["long"] if len(p.read) == L]
        assert max(len(p.read) for p in probes) == L
        _batch(bench16, probes)


def test_short_and_long_probes_in_batches_of_their_own_wide(bench_wide):
    """150 bp probes: first tier -> second -> global memory.  With the 532 bp probe the chain starts in the second tier, with the
    2068 bp probe in global memory."""
    g = bench_wide.groups()
    _batch(bench_wide, g["p131"])
    _batch(bench_wide, g["long"])
    _batch(bench_wide, g["p131"] + [p for p in g["long"] if len(p.read) == 532])


def test_two_queued_halves_16bit(bench16):
    """The as-built batch as two queued launches: both sets of per-batch buffers carry overflow lists at once.  The tallies are those
    of the whole batch, the records of the second half those of the blocking launch."""
    from lmat_amd import Params
    b, probes = bench16, bench16.probes
    res0, (tally, nm) = _batch(b, probes)
    h = len(probes) // 2
    dr = b.eng.upload_reads(_blob([p.read for p in probes]))
    b.eng.set_params(Params.run_rl(prn_all=0))
    try:
        b.eng.counts_reset()
        b.eng.classify_async(dr, 0, h)
        b.eng.classify_async(dr, h, len(probes) - h)
        b.eng.sync()
        _assert_tallies(b.eng.counts(), tally, nm, len(probes))
        _same_records(b.eng.fetch_results(0, len(probes) - h), res0[h:])
    finally:
        b.eng.set_params(Params.run_rl())
        dr.free()


# ---- c. the end of the chain -------------------------------------------------------------------------------------------------
def _good(b):
    """A few probes of every class the set has, short ones: the company of a read beyond the chain."""
    by = {}
    for p in b.groups()["p131"]:
        by.setdefault(p.expected, []).append(p)
    return [p for ps in by.values() for p in ps[:3]]


def _beyond_the_chain_blocking(b, name):
    from lmat_amd.capi import LmatError
    good = _good(b)
    h = len(good) // 2
    mixed = good[:h] + [b.beyond[name]] + good[h:]
    text, tally, nm = b.want(good)
    dr = b.eng.upload_reads(_blob([p.read for p in mixed]))
    try:
        res, got, n, before, _ = b.run(good)               # tallies to lose
        assert got == text and before[0]
        with pytest.raises(LmatError) as ei:
            _classify(b.eng, dr, 0, len(mixed), sum(p.T for p in mixed) + 64)
        assert ei.value.code == -4 and CAPACITY_MESSAGE in str(ei.value)
        assert b.eng.counts() == before                    # the failed launch tallied nothing
    finally:
        dr.free()
    res, got, n, counts, _ = b.run(good)                   # the sticky error word was cleared
    assert got == text
    _assert_tallies(counts, tally, nm, len(good))


@pytest.mark.parametrize("name", ["T4097", "TL4097", "E16385"])
def test_beyond_the_chain_blocking_16bit(bench16, name):
    """More than 4096 registered taxids (found by the closure pass; found by the registration of the listed ids), and -- apart from
    that -- more than 16384 list elements: LMAT_E_CAPACITY."""
    _beyond_the_chain_blocking(bench16, name)


def test_beyond_the_chain_blocking_wide(bench_wide):
    """The last row of the wide chain has no list to pass a read on to either."""
    _beyond_the_chain_blocking(bench_wide, "wT4097")


@pytest.mark.parametrize("name", ["T4097", "E16385"])
def test_beyond_the_chain_queued_16bit(bench16, name):
    """The same through classify_async: the error surfaces at that sync, once, and a following batch is clean."""
    from lmat_amd import Params
    from lmat_amd.capi import LmatError
    b = bench16
    good = _good(b)
    h = len(good) // 2
    mixed = good[:h] + [b.beyond[name]] + good[h:]
    res0 = b.run(good)[0]
    text, tally, nm = b.want(good)
    dr = b.eng.upload_reads(_blob([p.read for p in mixed]))
    dg = b.eng.upload_reads(_blob([p.read for p in good]))
    b.eng.set_params(Params.run_rl(prn_all=0))
    try:
        b.eng.classify_async(dr, 0, len(mixed))
        with pytest.raises(LmatError) as ei:
            b.eng.sync()
        assert ei.value.code == -4 and CAPACITY_MESSAGE in str(ei.value)
        b.eng.sync()                                       # reported once, then clear
        b.eng.counts_reset()
        b.eng.classify_async(dg, 0, len(good))
        b.eng.sync()
        _same_records(b.eng.fetch_results(0, len(good)), res0)
        _assert_tallies(b.eng.counts(), tally, nm, len(good))
    finally:
        b.eng.set_params(Params.run_rl())
        dr.free()
        dg.free()


# ---- d. the same probes under the switches that change who does the work -----------------------------------------------------
def _child_run(env_name, env_value, files, kexpr):
    """Switches read once per process: the named tests run again in a child pytest with the variable set."""
    import subprocess
    import sys
    if os.environ.get(env_name) is not None:
        pytest.skip("already the child run")
    env = dict(os.environ, **{env_name: env_value})
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(here, f) for f in files], "-m", "gpu", "-x", "-q", "-k", kexpr],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("switch", ["LMAT_K4_WAVE", "LMAT_MID_TIER", "LMAT_PLAIN", "LMAT_PIPELINE", "LMAT_TAIL"])
def test_edges_under_a_switch(switch):
    """LMAT_K4_WAVE=0: every decision by the general path.  LMAT_MID_TIER=0: the chain without the middle tier (the E = 512 class
    passes on to the large LDS class).  LMAT_PLAIN=0: the generic first class.  LMAT_PIPELINE=0: queued launches on one stream and
    one set of buffers.  LMAT_TAIL=0: no looked-up tails.  Tests a to c on the 16-bit set, each way."""
    _child_run(switch, "0", ["test_gpu_capacity_edges.py"], "16bit")
