"""GPU: every run mode in every capacity tier of the classify chain.  The graded probes (capacity_probes.build_graded_set, proved on
the CPU by test_capacity_probes.py) have exact T, E, D and P like the capacity-edge probes and a signal on top, so null models,
the human bias, the thresholds, the special taxids, permissive match, -g, rand mode and gene mode each decide something in the
fast class, the E = 512 class, the middle tier, the large LDS class and the global-memory class -- and in the three wide classes.
Every probe alone and all of them as batches, against the CPU oracle: the .out text byte for byte, the tallies (every read counted
once, whichever class ended up with it), the candidates returned, and the class-to-class counters of the table in
capacity_probes.py."""
import os

import numpy as np
import pytest

import capacity_probes as cp
from test_capacity_probes import oracle_candidates
from test_gpu_capacity_edges import MID_ON, _assert_tallies, _blob, _child_run, _classify, _same_records

pytestmark = pytest.mark.gpu

# mode -> engine parameters (lmat_params fields, the oracle's option names), null models, label modes; `same_dims`: the mode leaves
# T, E, D and P of a read as designed, so the counters are those of the table exactly
MODES = {
    "nm": dict(nm=True, same_dims=True),
    "nm_hbias3": dict(nm=True, opts=dict(hbias=3.0), same_dims=True),
    "hbias3": dict(opts=dict(hbias=3.0), same_dims=True),
    "no_p": dict(opts=dict(prn_all=0), same_dims=True),
    "strict": dict(opts=cp.STRICT, same_dims=True),
    "permissive": dict(permissive=True),
    "g": dict(cutoff=cp.G_CUTOFF),
    "permissive_g": dict(permissive=True, cutoff=cp.G_CUTOFF),
}
MODES_WIDE = ("nm", "nm_hbias3", "permissive")
DEFAULTS = dict(sdiff=1.0, hbias=0.0, min_score=0.0, min_kmer=30, min_fnd_kmer=1, prn_all=1, screen_phix=1)


def _params(opts, **over):
    from lmat_amd import Params
    o = dict(DEFAULTS, **opts)
    o.update(over)
    return Params(o["sdiff"], o["hbias"], o["min_score"], o["min_kmer"], o["min_fnd_kmer"], o["prn_all"], o["screen_phix"])


class _Set:
    """A graded probe set with its null models and rank map; the probes by the upload that takes them alone (a launch's tiers
    depend on the longest read of its read set)."""

    def __init__(self, outdir, wide):
        self.ps = cp.build_graded_set(outdir, wide)
        self.wide, self.probes, self.tax, self.outdir = wide, self.ps["probes"], self.ps["tax"], outdir
        self.null_lst, self.lmat_dir, self.nm_counts = cp.null_models(outdir, self.ps)
        self.ranks = cp.rank_map(outdir, self.tax)
        self.groups = {}
        for p in self.probes:
            self.groups.setdefault("p131" if p.P <= 512 else "P%d" % p.P, []).append(p)
        assert sorted(self.groups) == ["P2049", "P513", "p131"] and max(len(p.read) for p in self.groups["p131"]) == (150 if wide else 180)


class _ModeBench:
    """One engine and one oracle on a graded set in one run mode; what the oracle says is computed once and kept."""

    def __init__(self, gset, mode, null_lst=None, lmat_dir=None, oracle_null=None):
        from lmat_amd import Engine
        self.set, self.mode, self.spec = gset, mode, MODES[mode]
        self.wide, self.probes = gset.wide, gset.probes
        self.opts = dict(DEFAULTS, **self.spec.get("opts", {}))
        ps = gset.ps
        perm, cut = self.spec.get("permissive", False), self.spec.get("cutoff", 0)
        os.environ["LMAT_DIR"] = lmat_dir or gset.lmat_dir
        self.eng = Engine(0, _params(self.opts))
        self.eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
        if perm or cut:
            self.eng.set_label_modes(perm, cut, gset.ranks if cut else None)
        self.eng.build_db(ps["db"], k=cp.K)
        if self.spec.get("nm"):
            self.eng.load_null_models(null_lst or gset.null_lst)
        if oracle_null:      # (list file, directory): the oracle on tables of its own
            os.environ["LMAT_DIR"] = oracle_null[1]
        self.orc = cp.mode_oracle(ps, dict(self.opts), (oracle_null[0] if oracle_null else gset.null_lst) if self.spec.get("nm") else None, perm, cut,
                                  gset.ranks if cut else None)
        self._want = {}

    def want(self, probes, first_index=0):
        key = (tuple(p.name for p in probes), first_index)
        if key not in self._want:
            self._want[key] = self.orc.classify(*_blob([p.read for p in probes]), cp.K, first_index)
        return self._want[key]

    def dims(self, p):
        """T, E, D, P as the chain meets them in this mode.  A read with fewer valid k-mers than -j is ReadTooShort before anything
        is looked up: it enters no class."""
        return (0, 0, 0, 0) if p.P < self.opts["min_kmer"] else p.dims

    def counters(self, probes, max_len):
        out = dict.fromkeys(cp.COUNTERS, 0)
        for p in probes:
            for name, v in cp.route(self.dims(p), max_len, self.wide, MID_ON)[1].items():
                out[name] += v
        return out

    def at_least(self, probes, max_len):
        """Permissive match and -g change what a read registers.  The counters are then held against the oracle's own candidate
        count in that mode: a read with more candidates than a class has slots was passed on by it (a class that the batch has)."""
        n = [oracle_candidates(self.want([p])[0])[0] for p in probes]
        short_batch = max_len <= 512 + cp.K - 1
        if self.wide:
            return {"past_fast": sum(x > 128 for x in n) if short_batch else 0, "past_e512": sum(x > 512 for x in n) if max_len <= 2048 + cp.K - 1 else 0}
        return {"past_fast": sum(x > 64 for x in n), "past_e512": sum(x > 64 for x in n),
                "past_middle": sum(x > 256 for x in n) if MID_ON and short_batch else 0,
                "past_large": sum(x > 1024 for x in n) if max_len <= 2048 + cp.K - 1 else 0}

    def beyond(self, p):
        """Permissive match keeps the lineage of every id in the list records, so E of a read is the sum over its distinct lists of
        the list with all its ancestors: the E = 16384 probe is beyond the chain in that mode (unless -g prunes its lists)."""
        if not self.spec.get("permissive") or self.spec.get("cutoff"):
            return False
        return sum(len(cp.closure(self.set.tax, l)) for l in {tuple(l) for l in p.lists}) > 16384

    def reserved(self, probes, text):
        """Candidate pairs a -p launch hands out: one per registered taxid of every read that reaches the decision, none for a read
        cut before it (ReadTooShort) or called by the PhiX short-circuit -- whose records have no score statistics."""
        n = 0
        for p, line in zip(probes, text.split("\n")):
            if not line.split("\t")[2].startswith("-1 -1"):
                n += p.T if self.spec.get("same_dims") else oracle_candidates(line + "\n")[0]   # (no null models there: every score is printed)
        return n

    def check_counters(self, flow, probes, max_len):
        if self.spec.get("same_dims"):
            assert flow == self.counters(probes, max_len), (flow, self.counters(probes, max_len))
        else:
            low = self.at_least(probes, max_len)
            assert all(flow[k] >= v for k, v in low.items()), (flow, low)

    def run(self, probes, cand_cap=None):
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
def gset16(tmp_path_factory):
    return _Set(str(tmp_path_factory.mktemp("modes16")), False)


@pytest.fixture(scope="module")
def gset_wide(tmp_path_factory):
    return _Set(str(tmp_path_factory.mktemp("modes_wide")), True)


@pytest.fixture(scope="module", params=list(MODES))
def mode16(request, gset16):
    b = _ModeBench(gset16, request.param)
    yield b
    b.close()


@pytest.fixture(scope="module", params=list(MODES_WIDE))
def mode_wide(request, gset_wide):
    b = _ModeBench(gset_wide, request.param)
    yield b
    b.close()


# ---- a. each probe alone -------------------------------------------------------------------------------------------------------
def _each_probe_alone(b):
    from lmat_amd.capi import LmatError
    bad = []
    for gname, probes in b.set.groups.items():
        blob, off = _blob([p.read for p in probes])
        max_len = max(len(p.read) for p in probes)
        dr = b.eng.upload_reads((blob, off))
        for i, p in enumerate(probes):
            b.eng.counts_reset()
            if b.beyond(p):
                with pytest.raises(LmatError) as ei:
                    _classify(b.eng, dr, i, 1, 4200)
                assert ei.value.code == -4 and b.eng.counts()[0] == {}
                continue
            text, tally, nm = b.want([p], i)
            res, cands, n = _classify(b.eng, dr, i, 1, 4200)
            got = b.eng.format_out(res, cands, _blob([p.read]), i)
            flow = b.eng.last_counters()
            try:
                assert got == text                                            # the record and what it prints, byte for byte
                _assert_tallies(b.eng.counts(), tally, nm, 1)                 # tallied exactly once
                if b.opts["prn_all"]:
                    assert n == b.reserved([p], text)                         # nothing left behind by a class that gave the read up
                else:
                    assert n >= int(res["n_cand"][0])
                b.check_counters(flow, [p], max_len)
                if b.spec.get("same_dims") and MID_ON and b.dims(p)[3]:
                    assert cp.route(p.dims, max_len, b.wide, MID_ON)[0] == p.expected or p.P > 512
            except AssertionError as e:
                bad.append("%s (T %d, E %d, D %d, P %d; %s): %s" % (p.name, p.T, p.E, p.D, p.P, p.expected, str(e)[:400]))
        dr.free()
    assert not bad, "\n".join(bad)


def test_each_probe_alone_16bit(mode16):
    _each_probe_alone(mode16)


def test_each_probe_alone_wide(mode_wide):
    _each_probe_alone(mode_wide)


# ---- b. batches ----------------------------------------------------------------------------------------------------------------
def _batch(b, probes):
    probes = [p for p in probes if not b.beyond(p)]
    max_len = max(len(p.read) for p in probes)
    text, tally, nm = b.want(probes)
    res, got, n, counts, flow = b.run(probes)
    assert got == text
    _assert_tallies(counts, tally, nm, len(probes))
    if b.opts["prn_all"]:
        assert n == b.reserved(probes, text)
    else:
        assert n >= int(res["n_cand"].sum())
    b.check_counters(flow, probes, max_len)
    return res, (tally, nm)


def _batches(b):
    """All probes (the longest has 2068 bp: the launch has neither the middle tier nor the large LDS class), the short ones (every
    tier) and those with the 532 bp probe (no middle tier), the last two in another order."""
    g = b.set.groups
    _batch(b, b.probes)
    _batch(b, g["p131"][::-1])
    _batch(b, g["P513"] + g["p131"])


def test_batches_16bit(mode16):
    _batches(mode16)


def test_batches_wide(mode_wide):
    _batches(mode_wide)


def _two_queued_halves(b):
    """The short probes as two queued launches: both sets of per-batch buffers carry overflow lists at once.  The tallies are those
    of the whole batch, the records of the second half those of the blocking launch."""
    probes = [p for p in b.set.groups["p131"] if not b.beyond(p)]
    res0, (tally, nm) = _batch(b, probes)
    h = len(probes) // 2
    dr = b.eng.upload_reads(_blob([p.read for p in probes]))
    b.eng.set_params(_params(b.opts, prn_all=0))
    try:
        b.eng.counts_reset()
        b.eng.classify_async(dr, 0, h)
        b.eng.classify_async(dr, h, len(probes) - h)
        b.eng.sync()
        _assert_tallies(b.eng.counts(), tally, nm, len(probes))
        _same_records(b.eng.fetch_results(0, len(probes) - h), res0[h:])
    finally:
        b.eng.set_params(_params(b.opts))
        dr.free()


@pytest.mark.parametrize("mode16", ["nm", "nm_hbias3", "permissive", "permissive_g"], indirect=True)
def test_two_queued_halves_16bit(mode16):
    _two_queued_halves(mode16)


def test_two_queued_halves_wide(mode_wide):
    _two_queued_halves(mode_wide)


@pytest.mark.parametrize("mode16", ["no_p"], indirect=True)
def test_without_a_candidate_buffer_16bit(mode16):
    """prn_all = 0 and no buffer for the lineage either: the records of the launch that had one, the same tallies and counters."""
    b = mode16
    probes = b.set.groups["p131"]
    res0, (tally, nm) = _batch(b, probes)
    dr = b.eng.upload_reads(_blob([p.read for p in probes]))
    try:
        for first, count in [(0, len(probes))] + [(i, 1) for i in range(len(probes))]:
            sub = probes[first:first + count]
            _, tally, nm = b.want(sub, first)
            b.eng.counts_reset()
            res, _ = b.eng.classify(dr, first, count, want_cands=False)
            _same_records(res, res0[first:first + count])
            _assert_tallies(b.eng.counts(), tally, nm, count)
            assert b.eng.last_counters() == b.counters(sub, 180), [p.name for p in sub]
    finally:
        dr.free()


# ---- c. a taxid without a null model, met in a later tier --------------------------------------------------------------------------
def test_missing_null_model_row_in_a_later_tier_16bit(gset16, tmp_path):
    """One taxid's row is gone from the 131-k-mer table, a taxid that only probes of the middle tier and beyond register.  The probe
    that meets it, launched alone, is LMAT_E_TAXONOMY (upstream asserts there, read_label.cpp:768-775) from the tier kernels' own
    staging; nothing was tallied and the next launch is clean."""
    import gzip
    from lmat_amd.capi import LmatError
    s = gset16
    early = cp.closure(s.tax, cp.registered(x for p in s.probes if p.expected in ("fast", "e512") for l in p.lists for x in l))
    victim = [p for p in s.probes if p.name == "gT256"][0]
    drop = str(max(cp.closure(s.tax, [x for l in victim.lists for x in l]) - early))
    nmdir = str(tmp_path / "nm")
    os.makedirs(nmdir)
    lst = os.path.join(nmdir, "null_lst.txt")
    dropped = 0
    with open(lst, "w") as lf:
        for line in open(s.null_lst):
            kc, name = line.split()
            lf.write("%s %s\n" % (kc, name))
            rows = gzip.open(os.path.join(s.lmat_dir, name), "rt").read().split("\n")
            keep = [r for r in rows if not (kc == "131" and r and r.split()[0] == drop)]
            dropped += len(rows) - len(keep)
            with gzip.open(os.path.join(nmdir, name), "wt") as g:
                g.write("\n".join(keep))
    assert dropped == 1
    b = _ModeBench(s, "nm", null_lst=lst, lmat_dir=nmdir)
    try:
        good = [p for p in s.probes if p.name == "gT40"]
        text, tally, nm = b.want(good)
        res, got, n, before, _ = b.run(good)
        assert got == text and before[0]
        dr = b.eng.upload_reads(_blob([victim.read]))
        try:
            with pytest.raises(LmatError) as ei:
                _classify(b.eng, dr, 0, 1, 4200)
            assert ei.value.code == -5 and "NULL MODELS" in str(ei.value)
            assert b.eng.counts() == before
        finally:
            dr.free()
        res, got, n, counts, _ = b.run(good)
        assert got == text
        _assert_tallies(counts, tally, nm, 1)
    finally:
        os.environ["LMAT_DIR"] = s.lmat_dir
        b.close()


def test_gc_bin_past_the_last_bin_of_a_table_16bit(gset16, tmp_path):
    """Null models with eight GC bins and reads of more than 80 % G + C (bin 8 or 9): the engine takes the table's last bin.  The
    oracle indexes a row by the bin as upstream does, so it gets the same tables with bins 8 to 10 written out as copies of bin 7:
    equal text means the engine read bin 7 -- in the decision of the fast class and in the staging of the middle tier."""
    import copy
    import gzip
    from lmat_amd import synth
    s = gset16
    probes = [p for p in s.probes if p.name.endswith("_gc")]
    assert [p.expected for p in probes] == ["fast", "middle"] and all(cp.gc_bin(p.read) >= 8 for p in probes)
    tax = copy.copy(s.tax)
    ids = cp.closure(s.tax, cp.registered(x for p in probes for l in p.lists for x in l))
    tax.ids = [t for t in s.tax.ids if t in ids]
    d8, d11 = str(tmp_path / "nm8"), str(tmp_path / "nm11")
    lst8 = synth.write_null_models(d8, tax, kmer_counts=(131,), num_bins=8)
    os.makedirs(d11)
    lst11 = os.path.join(d11, "null_lst.txt")
    with open(lst11, "w") as f:
        f.write(open(lst8).read())
    name = open(lst8).read().split()[1]
    rows = gzip.open(os.path.join(d8, name), "rt").read().split("\n")
    assert rows[0] == "8"
    with gzip.open(os.path.join(d11, name), "wt") as g:
        g.write("\n".join(["11"] + [r + (" " + " ".join(r.split()[-3:])) * 3 for r in rows[1:] if r]) + "\n")
    b = _ModeBench(s, "nm", null_lst=lst8, lmat_dir=d8, oracle_null=(lst11, d11))
    try:
        for p in probes:
            text, tally, nm = b.want([p])
            res, got, n, counts, _ = b.run([p])
            assert int(res["bin_sel"][0]) == cp.gc_bin(p.read) >= 8
            assert got == text, p.name
            _assert_tallies(counts, tally, nm, 1)
        called = [cp.record_call(b.want([p])[0].split("\n")[0]) for p in probes]
        assert all(c[0] is not None for c in called)
    finally:
        os.environ["LMAT_DIR"] = s.lmat_dir
        b.close()


# ---- d. rand mode (rand_read_label) --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rand16(gset16):
    import oracle_py
    from lmat_amd import Engine, Params
    ps = gset16.ps
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    eng.rand_mode(True)
    eng.build_db(ps["db"], k=cp.K)
    orc = oracle_py.Oracle(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    orc.add_taxhisto(ps["db"])
    yield eng, orc
    orc.close()
    eng.close()


def _same_rand_tables(got, want):
    got = {t: v for t, v in got.items() if v[1].any()}
    assert set(got) == set(want)
    for t in want:
        assert (got[t][1] == want[t][1]).all(), t
        assert (got[t][0].view(np.uint32) == want[t][0].view(np.uint32)).all(), t


def test_rand_mode_counts_every_probe_once_16bit(gset16, rand16):
    """A probe launched alone adds exactly one hit for each taxid it registers, in its GC bucket, and nothing else: a read that a
    later class re-ran -- the two launches of the E = 512 class, split by read length, among them -- was not counted by the class
    that gave it up.  In this mode the human variants keep rows of their own, so T is the closure of the listed ids as they are."""
    eng, orc = rand16
    s = gset16
    bad = []
    for gname, probes in s.groups.items():
        blob, off = _blob([p.read for p in probes])
        max_len = max(len(p.read) for p in probes)
        dr = eng.upload_reads((blob, off))
        for i, p in enumerate(probes):
            bucket = (7 * i + 3) % 10
            eng.rand_reset(10)
            eng.rand_label(dr, np.array([bucket], dtype=np.uint8), i, 1)
            got = {t: v for t, v in eng.rand_table().items() if v[1].any()}
            flow = eng.last_counters()
            ids = cp.closure(s.tax, {x for l in p.lists for x in l})
            try:
                assert set(got) == ids
                hit = np.zeros(10, dtype=np.uint32)
                hit[bucket] = 1
                assert all((v[1] == hit).all() for v in got.values())
                _same_rand_tables(got, orc.rand_label(*_blob([p.read]), cp.K, np.array([bucket], dtype=np.uint8)))
                assert flow == cp.route((len(ids), p.E, p.D, p.P), max_len, False, MID_ON)[1]
            except AssertionError as e:
                bad.append("%s (T %d, E %d, D %d, P %d; %s): %s" % (p.name, len(ids), p.E, p.D, p.P, p.expected, str(e)[:300]))
        dr.free()
    assert not bad, "\n".join(bad)


def test_rand_mode_tables_of_a_batch_16bit(gset16, rand16):
    """All probes, GC buckets drawn per read, every upload labelled in two calls (the second with first != 0) that accumulate."""
    eng, orc = rand16
    s = gset16
    rng = np.random.default_rng(11)
    eng.rand_reset(10)
    reads, buckets = [], []
    for gname, probes in s.groups.items():
        gc = rng.integers(0, 10, size=len(probes)).astype(np.uint8)
        dr = eng.upload_reads(_blob([p.read for p in probes]))
        h = len(probes) // 2
        if h:
            eng.rand_label(dr, gc[:h], 0, h)
        eng.rand_label(dr, gc[h:], h, len(probes) - h)
        dr.free()
        reads += [p.read for p in probes]
        buckets += gc.tolist()
    want = orc.rand_label(*_blob(reads), cp.K, np.array(buckets, dtype=np.uint8))
    assert len(want) > 4096
    _same_rand_tables(eng.rand_table(), want)


# ---- e. gene mode ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genes(tmp_path_factory):
    import oracle_py
    from lmat_amd import Engine, Params
    gs = cp.build_gene_set(str(tmp_path_factory.mktemp("genes")))
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.build_gene_db(gs["db"], k=cp.K)
    orc = oracle_py.GeneOracle(gs["db"])
    yield gs, eng, orc
    orc.close()
    eng.close()


def _same_votes(res, want, names):
    any_, gid, top, cnt, score = want
    for i, name in enumerate(names):
        assert any_[i] and res["status"][i] == 0, name
        assert (res["call_tid"][i], res["n_cand"][i], res["cand_kmer_cnt"][i]) == (gid[i], top[i], cnt[i]), name
        assert res["call_score"][i:i + 1].view(np.uint32)[0] == score[i:i + 1].view(np.uint32)[0], name


def test_gene_mode_in_every_tier(genes):
    """G distinct genes and E list elements on and one above every capacity of the chain (the same numbers as for taxids: DESIGN
    section 3): each probe alone, with the counters of the table, and all of them as one batch, against gene_label's vote."""
    gs, eng, orc = genes
    probes = gs["probes"]
    blob, off = _blob([p.read for p in probes])
    want = orc.label(blob, off, cp.K)
    dr = eng.upload_reads((blob, off))
    bad = []
    try:
        for i, p in enumerate(probes):
            res, _ = eng.classify(dr, i, 1, want_cands=False)
            try:
                _same_votes(res, [w[i:i + 1] for w in want], [p.name])
                where, flow = cp.route(p.dims, 150, False, MID_ON)
                assert eng.last_counters() == flow and (where == p.expected or not MID_ON)
            except AssertionError as e:
                bad.append("%s (G %d, E %d, D %d; %s): %s" % (p.name, p.T, p.E, p.D, p.expected, str(e)[:300]))
        assert not bad, "\n".join(bad)
        res, _ = eng.classify(dr, 0, len(probes), want_cands=False)
        _same_votes(res, want, [p.name for p in probes])
        total = dict.fromkeys(cp.COUNTERS, 0)
        for p in probes:
            for k, v in cp.route(p.dims, 150, False, MID_ON)[1].items():
                total[k] += v
        assert eng.last_counters() == total
    finally:
        dr.free()


def test_gene_mode_beyond_the_chain(genes):
    """4097 genes in one read: LMAT_E_CAPACITY, and the next launch is clean."""
    from lmat_amd.capi import LmatError
    gs, eng, orc = genes
    good = gs["probes"][:3]
    dr = eng.upload_reads(_blob([good[0].read, gs["beyond"].read, good[1].read, good[2].read]))
    dg = eng.upload_reads(_blob([p.read for p in good]))
    try:
        with pytest.raises(LmatError) as ei:
            eng.classify(dr, want_cands=False)
        assert ei.value.code == -4
        res, _ = eng.classify(dg, want_cands=False)
        _same_votes(res, orc.label(*_blob([p.read for p in good]), cp.K), [p.name for p in good])
    finally:
        dr.free()
        dg.free()


def test_gene_mode_equal_top_votes(genes):
    """Two genes with 30 votes each, ids on either side of 2^31.  gene_label sorts the genes in the order the read met them by
    votes alone (gene_label.cpp:289-297); among the few genes of these reads that sort moves nothing past an equal.  Where the
    smaller id is met first it wins; where the larger one is met first, upstream -- and so the oracle and the engine -- calls that."""
    gs, eng, orc = genes
    blob, off = _blob([p.read for p in gs["ties"]])
    want = orc.label(blob, off, cp.K)
    dr = eng.upload_reads((blob, off))
    try:
        res, _ = eng.classify(dr, want_cands=False)
    finally:
        dr.free()
    _same_votes(res, want, [p.name for p in gs["ties"]])
    assert [int(x) for x in res["call_tid"]] == [0x7FFFFFF0, 0x80000010] and list(res["n_cand"]) == [30, 30]
    assert int(res["call_tid"][0]) == min(0x7FFFFFF0, 0x80000010)      # the smaller id, met first


# ---- f. the chain without the middle tier ----------------------------------------------------------------------------------------
def test_modes_under_the_mid_tier_switch():
    """LMAT_MID_TIER=0 (read once per process: a child pytest): the E = 512 class passes on to the large LDS class.  The null-model
    and permissive tests of the 16-bit set again, with the counters of that shorter chain."""
    _child_run("LMAT_MID_TIER", "0", ["test_gpu_mode_tiers.py"], "16bit and (nm or permissive) and not rand")
