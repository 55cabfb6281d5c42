"""CPU: the capacity probes (capacity_probes.py) hit their marks before they reach a GPU.  The oracle classifies every probe on the
probe database; its candidate count is the designed T, E and D recomputed from the written file are the designed ones, no k-mer
belongs to two probes, and every capacity edge of the table has a probe below it, on it and above it."""
import numpy as np
import pytest

import capacity_probes as cp


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def oracle_candidates(text):
    """Candidates the oracle printed per record of its .out text (the " taxid score" pairs of the -p field)."""
    out = []
    for line in text.split("\n")[:-1]:
        f = line.split("\t")
        pairs = f[3].split() if len(f) >= 5 else []
        out.append(0 if pairs[:2] == ["-1", "-1"] else len(pairs) // 2)
    return out


@pytest.fixture(scope="module", params=["16bit", "wide"])
def probe_set(request, tmp_path_factory):
    import oracle_py
    ps = cp.build_set(str(tmp_path_factory.mktemp("probes_" + request.param)), wide=request.param == "wide")
    orc = oracle_py.Oracle(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    orc.add_taxhisto(ps["db"])
    orc.set_options()
    ps["orc"] = orc
    yield ps
    orc.close()


def test_oracle_counts_the_designed_T(probe_set):
    probes = probe_set["probes"]
    blob, off = _blob([p.read for p in probes])
    text, tally, nm = probe_set["orc"].classify(blob, off, cp.K)
    got = oracle_candidates(text)
    assert len(got) == len(probes)
    bad = [(p.name, p.T, g) for p, g in zip(probes, got) if g != p.T]
    assert not bad, bad
    # one record per probe was tallied: a call, NoDbHits (no_hit) or ReadTooShort (short)
    assert sum(c for c, _ in tally.values()) + sum(nm) == len(probes)


def test_E_and_D_as_designed_from_the_written_file(probe_set):
    table = cp.read_taxhisto(probe_set["db"])
    orc, tax = probe_set["orc"], probe_set["tax"]
    assert orc.k == cp.K and len(table) == sum(len(p.lists) for p in probe_set["probes"])
    seen = {}
    for p in probe_set["probes"]:
        km = orc.extract(p.read.encode(), cp.K)[0]
        assert km.size == p.P
        for x in km.tolist():
            assert seen.setdefault(x, p.name) == p.name, "k-mer %d in %s and %s" % (x, seen[x], p.name)
        assert len(set(km.tolist())) == km.size
        assert cp.measure(tax, table, km) == (p.T, p.E, p.D), p.name
        assert [table[int(km[i])] for i in p.positions] == p.lists


def test_every_boundary_has_a_probe_on_each_side_and_on_it(probe_set):
    wide = probe_set["wide"]
    cov = cp.coverage(probe_set["probes"], wide)
    for (axis, c), (below, at, above) in sorted(cov.items()):
        print("%s %s = %5d: below %s, on it %s, above %s" % ("wide" if wide else "16bit", axis, c, below, at, above))
    missing = [(axis, c) for (axis, c), (below, at, above) in cov.items() if not (below and at and above)]
    assert not missing, missing
    # ... and the other axes of such a probe stay inside the class it aims at, so that this axis alone decides
    classes = {c[0]: c for c in (cp.CLASSES_WIDE if wide else cp.CLASSES16)}
    for p in probe_set["probes"]:
        if p.axis in ("T", "E", "D") and getattr(p, p.axis) <= p.boundary:
            assert p.expected in classes and getattr(p, p.axis) <= classes[p.expected][{"T": 1, "E": 2, "D": 3}[p.axis]], p.name
            assert classes[p.expected][{"T": 1, "E": 2, "D": 3}[p.axis]] == p.boundary, (p.name, p.expected)
        if p.axis in ("T", "E", "D") and getattr(p, p.axis) == p.boundary + 1:
            # one above: the next class of the table takes it (or nothing does)
            names = [c[0] for c in (cp.CLASSES_WIDE if wide else cp.CLASSES16)]
            at = [q for q in probe_set["probes"] if q.axis == p.axis and q.boundary == p.boundary and getattr(q, q.axis) == p.boundary][0]
            assert names.index(p.expected) > names.index(at.expected), p.name
        if p.axis == "E":
            assert 2 * p.T <= classes[cp.expected_class(1, p.boundary, 1, p.P, wide)][1], p.name   # T at most half the class's
    if not wide:
        by = {p.name: p for p in probe_set["probes"]}
        assert by["E16385"].T < 4096 and by["T4097"].E <= 16384 and by["T4097"].expected == by["E16385"].expected == "error"
        assert [by["D%d" % d].expected for d in (63, 64, 65, 66)] == ["fast", "fast", "middle", "middle"]
        assert all(by["P%d_E257" % P].expected == "e512" and by["P%d_E513" % P].expected == "middle" for P in (160, 161, 256, 257, 320, 321, 512))


def test_route_follows_the_table():
    """The chain walk the GPU tests take their counter expectations from, on hand-worked cases."""
    z = dict.fromkeys(cp.COUNTERS, 0)
    assert cp.route((64, 256, 64, 131), 150) == ("fast", z)
    assert cp.route((65, 60, 1, 131), 150) == ("middle", dict(z, past_fast=1, past_e512=1))
    assert cp.route((65, 60, 1, 131), 150, mid_on=False) == ("large", dict(z, past_fast=1, past_e512=1))
    assert cp.route((30, 257, 14, 131), 150) == ("e512", dict(z, past_fast=1))
    assert cp.route((1025, 900, 2, 131), 150) == ("gmem", dict(z, past_fast=1, past_e512=1, past_middle=1, past_large=1))
    assert cp.route((1025, 900, 2, 131), 532) == ("gmem", dict(z, past_fast=1, past_e512=1, past_large=1))
    assert cp.route((1025, 900, 2, 131), 2068) == ("gmem", dict(z, past_fast=1, past_e512=1))
    assert cp.route((4097, 3600, 2, 131), 150) == ("error", dict(z, past_fast=1, past_e512=1, past_middle=1, past_large=1))
    assert cp.route((20, 20, 1, 513), 532) == ("large", dict(z, past_fast=1, past_e512=1))
    assert cp.route((20, 20, 1, 2049), 2068) == ("gmem", dict(z, past_fast=1, past_e512=1))
    assert cp.route((129, 120, 1, 131), 150, wide=True) == ("w2", dict(z, past_fast=1))
    assert cp.route((129, 120, 1, 513), 532, wide=True) == ("w2", z)
    assert cp.route((129, 120, 1, 2049), 2068, wide=True) == ("gmem", z)
    assert cp.route((513, 500, 1, 131), 150, wide=True) == ("gmem", dict(z, past_fast=1, past_e512=1))
    assert cp.route((0, 0, 0, 0), 150) == ("none", z)


# ---- the graded probes (capacity_probes.build_graded_set): the same exact quantities, and a signal every run mode decides on ----
GRADED_TIER = {   # the tier each graded probe is meant for
    "gT40": "fast", "gT64": "fast", "gT65": "middle", "gT256": "middle", "gT257": "large", "gT1024": "large", "gT1025": "gmem",
    "gT4096": "gmem", "gE256": "fast", "gE257": "e512", "gE512": "e512", "gE513": "middle", "gE1024": "middle", "gE1025": "large",
    "gE4096": "large", "gE4097": "gmem", "gE16384": "gmem", "gT65_P513": "large", "gT65_P2049": "gmem", "gT65_P30": "middle",
    "gT65_tied": "middle", "gT257_tied": "large", "gT1025_tied": "gmem", "gE257_tied": "e512", "gE513_tied": "middle",
    "gE4097_tied": "gmem", "gT65_human": "middle", "gT257_human": "large", "gT1025_human": "gmem", "gE257_human": "e512",
    "gE513_human": "middle", "gE4097_human": "gmem", "gT40_phix": "fast", "gT65_phix": "middle", "gT257_phix": "large",
    "gT1025_phix": "gmem", "gE257_phix": "e512", "gT65_plasmid": "middle", "gE257_P160": "e512",
    "gE257_P161": "e512", "gT257_weak": "large", "gT40_gc": "fast", "gT65_gc": "middle",
    "wT128": "w1", "wT129": "w2", "wT512": "w2", "wT513": "gmem", "wE512": "w1", "wE513": "w2", "wE2048": "w2", "wE2049": "gmem",
    "wT129_P513": "w2", "wT129_P2049": "gmem"}


class _Graded:
    """A graded set with what the oracle says of every probe, alone, in every run mode: {mode: [(text, tally, nomatch)]}."""

    def __init__(self, outdir, wide):
        import time
        t0 = time.process_time()
        self.ps = cp.build_graded_set(outdir, wide)
        self.null_lst, self.lmat_dir, self.nm_counts = cp.null_models(outdir, self.ps)
        self.fixture_cpu_s = time.process_time() - t0
        self.wide, self.probes, self.tax = wide, self.ps["probes"], self.ps["tax"]
        self.ranks = cp.rank_map(outdir, self.tax)
        self._got = {}

    def mode(self, name):
        if name not in self._got:
            import os
            os.environ["LMAT_DIR"] = self.lmat_dir
            kw = {"plain": {}, "phix_off": dict(options=dict(screen_phix=0)), "nm": dict(null_lst=self.null_lst),
                  "nm_hbias3": dict(options=dict(hbias=3.0), null_lst=self.null_lst), "hbias3": dict(options=dict(hbias=3.0)),
                  "strict": dict(options=cp.STRICT), "permissive": dict(permissive=True),
                  "g": dict(cutoff=cp.G_CUTOFF, ranks=self.ranks), "permissive_g": dict(permissive=True, cutoff=cp.G_CUTOFF, ranks=self.ranks)}[name]
            orc = cp.mode_oracle(self.ps, **kw)
            self._got[name] = [orc.classify(*_blob([p.read]), cp.K, i) for i, p in enumerate(self.probes)]
            orc.close()
        return self._got[name]

    def calls(self, name):
        return [cp.record_call(text.split("\n")[0]) for text, _, _ in self.mode(name)]

    def called(self, name):
        """Per probe: tallied as a call (not NoDbHits, ReadTooShort or LowScore)."""
        return [sum(c for c, _ in tally.values()) == 1 and sum(nm) == 0 for _, tally, nm in self.mode(name)]

    def by_tier(self):
        out = {}
        for i, p in enumerate(self.probes):
            out.setdefault(p.expected, []).append(i)
        return out


@pytest.fixture(scope="module")
def graded16(tmp_path_factory):
    return _Graded(str(tmp_path_factory.mktemp("graded_16bit")), False)


@pytest.fixture(scope="module")
def graded_wide(tmp_path_factory):
    return _Graded(str(tmp_path_factory.mktemp("graded_wide")), True)


@pytest.fixture(scope="module", params=["16bit", "wide"])
def graded(request):
    return request.getfixturevalue("graded16" if request.param == "16bit" else "graded_wide")


def test_graded_probes_hit_their_marks(graded):
    """T by the oracle's candidate count (PhiX screening off: a PhiX call prints no candidates), (T, E, D) from the written file,
    the intended tier, no shared k-mer -- and the probe set of build_set is not touched by any of it."""
    import oracle_py
    probes, tax = graded.probes, graded.tax
    assert [p.name for p in probes] == [n for n in GRADED_TIER if n.startswith("w" if graded.wide else "g")]
    got = [oracle_candidates(text)[0] for text, _, _ in graded.mode("phix_off")]
    assert got == [p.T for p in probes]
    assert [p.expected for p in probes] == [GRADED_TIER[p.name] for p in probes]
    assert all(3 <= p.D <= 28 for p in probes)
    table = cp.read_taxhisto(graded.ps["db"])
    orc = oracle_py.Oracle(graded.ps["tree"], graded.ps["depth"], graded.ps["rank"], graded.ps["idmap"])
    seen = {}
    for p in probes:
        km = orc.extract(p.read.encode(), cp.K)[0]
        assert km.size == p.P and len(set(km.tolist())) == km.size
        for x in km.tolist():
            assert seen.setdefault(x, p.name) == p.name, "k-mer %d in %s and %s" % (x, seen[x], p.name)
        assert cp.measure(tax, table, km) == (p.T, p.E, p.D), p.name
        assert [table[int(km[i])] for i in p.positions] == p.lists
        assert p.positions != sorted(p.positions)          # the lists are not met in any sorted order
    orc.close()
    assert len(table) == sum(len(p.lists) for p in probes)


def test_graded_plain_run_calls_every_probe_both_ways(graded):
    assert all(graded.called("plain"))
    kinds = [c[2] for c in graded.calls("plain")]
    if graded.wide:
        return
    for tier, idx in graded.by_tier().items():
        if tier != "fast":
            assert {"DirectMatch", "MultiMatch"} <= {kinds[i] for i in idx}, tier
    # the special taxids do what they are there for: the PhiX short-circuit in every tier, the plasmid override
    by = {p.name: c for p, c in zip(graded.probes, graded.calls("plain"))}
    assert all(by[p.name][0] == 32630 for p in graded.probes if p.shape == "phix")
    assert {p.expected for p in graded.probes if p.shape == "phix"} == {"fast", "e512", "middle", "large", "gmem"}
    assert by["gT65_plasmid"][0] == 10000001


def test_the_probe_set_of_build_set_is_what_it_was(probe_set):
    """The graded family has a builder and a seed of its own: the database of build_set is byte for byte the one the capacity-edge
    tests were written against."""
    import hashlib
    want = {False: "ac184fd88c5b5a1ac9a1493885124dcc8b23a0f161d1eddbd8bbb652570a3a37", True: "d67eb4337bd93abfd9f814b2438497ffd1214b3f78235c258bfd154810e715fa"}
    assert hashlib.sha256(open(probe_set["db"], "rb").read()).hexdigest() == want[probe_set["wide"]]


def test_graded_null_models_decide_differently(graded):
    called, calls, plain = graded.called("nm"), graded.calls("nm"), graded.calls("plain")
    for tier, idx in graded.by_tier().items():
        assert 2 * sum(called[i] for i in idx) >= len(idx), (tier, [graded.probes[i].name for i in idx if not called[i]])
        assert any(calls[i] != plain[i] for i in idx), tier
    tables = {min(graded.nm_counts, key=lambda c: (abs(c - p.P), c)) for p in graded.probes}
    assert len(tables) >= 2 and graded.fixture_cpu_s < 15.0, (tables, graded.fixture_cpu_s)
    assert len({cp.gc_bin(p.read) for p in graded.probes}) >= 2 and max(cp.gc_bin(p.read) for p in graded.probes) < 11
    if not graded.wide:
        assert tables == {31, 131, 513, 2049}
        assert all(cp.gc_bin(p.read) >= 8 for p in graded.probes if p.name.endswith("_gc"))
        scores = [c[1] for c in calls + graded.calls("nm_hbias3") if c[1] is not None]
        assert min(scores) < 0 and max(scores) > 1           # log-odds, not fractions
        assert sum(not c for c in called) >= 1               # LowScore exists under null models


def test_graded_human_bias_changes_the_human_probes(graded16):
    graded = graded16
    human = [i for i, p in enumerate(graded.probes) if p.shape == "human"]
    assert len(human) == 6
    for a, b in (("plain", "hbias3"), ("nm", "nm_hbias3")):
        assert all(graded.mode(a)[i][0] != graded.mode(b)[i][0] for i in human)
    assert any(graded.calls("hbias3")[i][0] == 9606 for i in human)


def test_graded_label_modes_still_cross_every_capacity(graded):
    """Permissive match and -g change what a read registers: by the oracle's own candidate count in each mode at least one probe
    still exceeds each T capacity of the chain -- the counts the GPU test holds the routing counters against."""
    caps = (128, 512) if graded.wide else (64, 256, 1024)
    for mode in ("permissive",) if graded.wide else ("permissive", "g", "permissive_g"):
        n = [oracle_candidates(text)[0] for text, _, _ in graded.mode(mode)]
        for cap in caps:
            assert sum(x > cap for x in n) >= 1, (mode, cap)
        if mode != "permissive":
            assert n != [p.T for p in graded.probes]         # the cutoff prunes something


def test_graded_strict_thresholds_cut_reads_of_later_tiers(graded16):
    graded = graded16
    later = [i for i, p in enumerate(graded.probes) if p.expected in ("middle", "large", "gmem")]
    got = graded.mode("strict")
    assert any(got[i][2][2] == 1 for i in later)                                   # LowScore
    short = [i for i, p in enumerate(graded.probes) if p.name == "gT65_P30"][0]
    assert graded.called("plain")[short] and not graded.called("strict")[short]    # cut by -j 35, called at -j 30
    assert graded.probes[short].expected == "middle" and graded.probes[short].P == cp.MIN_KMER_P


# ---- the gene probes ----------------------------------------------------------------------------------------------------------------
def test_gene_probes_hit_their_marks(tmp_path):
    import oracle_py
    from lmat_amd import synth
    gs = cp.build_gene_set(str(tmp_path))
    table = cp.read_taxhisto(gs["db"])
    everything = gs["probes"] + [gs["beyond"]] + gs["ties"]
    seen = set()
    for p in everything:
        km = synth.kmers_of(np.array(["ACGT".index(c) for c in p.read], dtype=np.uint8), cp.K)
        assert km.size == p.P and not (set(km.tolist()) & seen)
        seen |= set(km.tolist())
        met = {tuple(table[int(x)]) for x in km.tolist() if int(x) in table}
        assert (len({g for l in met for g in l}), sum(len(l) for l in met), len(met)) == (p.T, p.E, p.D), p.name
    want = {"G64": "fast", "G65": "middle", "G256": "middle", "G257": "large", "G1024": "large", "G1025": "gmem", "G4096": "gmem",
            "GE256": "fast", "GE257": "e512", "GE512": "e512", "GE513": "middle", "GE1024": "middle", "GE1025": "large",
            "GE4096": "large", "GE4097": "gmem", "GE16384": "gmem"}
    assert {p.name: p.expected for p in gs["probes"]} == want and (gs["beyond"].T, gs["beyond"].expected) == (4097, "error")
    assert max(g for p in everything for l in p.lists for g in l) > 1 << 31
    o = oracle_py.GeneOracle(gs["db"])
    any_, gid, top, cnt, score = o.label(*_blob([p.read for p in everything]), cp.K)
    o.close()
    for i, p in enumerate(everything[:-2]):      # the winner sits alone on 40 positions: a unique top vote
        assert any_[i] and gid[i] == p.lists[0][0] and top[i] == 40 and cnt[i] == p.P, p.name
    # equal top votes: gene_label sorts the genes, in the order the read met them, by votes alone (gene_label.cpp:289-297); among
    # few genes that sort moves nothing past an equal, so the gene met first keeps the front -- whichever id is the smaller
    lo, hi = 0x7FFFFFF0, 0x80000010
    assert [int(g) for g in gid[-2:]] == [lo, hi] and list(top[-2:]) == [30, 30]
