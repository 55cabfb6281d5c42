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
