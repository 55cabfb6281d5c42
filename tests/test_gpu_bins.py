"""GPU: reads pulled by called taxon (lmat_bins_*, lmat_stream_set_bins; bins.hip) on the small dataset at k = 20.

1. replay: the records of the reference's own example run, rebuilt as lmat_read_result from the golden fields, through the select
   kernel alone under the golden id files: the group of every record is the one bin/pull_reads.pl chose (tests/golden/pull/).
2. end to end: classify, run the bins; index lists, offsets, counts and bases against tests/pull_model.py applied to the fetched
   records and test_gpu_pack._image of the selected reads.
3. shapes: batch sizes around a wave and a block, group counts up to more than one 8-bit radix digit, all / none selected, read
   lengths 0..70 with hostile bytes at every output alignment, a sub-range of a Reads.
4. errors.  5. the streamed boundary, a slot that grows and runs its batch again included."""
import numpy as np
import pytest

import pull_model as pm
from test_gpu_pack import _blob, _image, _mixed

pytestmark = pytest.mark.gpu

THRESH, LOW, MIN_KMER = 0.4173, 0.2031, 30      # no k-mer fraction of a 150 bp read lies near them (asserted)
E_ARG, E_CAPACITY, E_STATE = -1, -4, -7
FIELDS = ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "read_len", "call_tid", "call_score")   # (cand_off depends on the launch)


@pytest.fixture(scope="module")
def fx(small_dataset):
    """Engine + the 400 fixture reads uploaded and classified once: records, the taxonomy's parent map, and a called strain and its
    species for the groups."""
    from lmat_amd import Engine, Params, synth
    ds = small_dataset
    e = Engine(0, Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    e.build_db(ds["db"], k=20)
    tax = synth.make_taxonomy((2, 2, 2, 2, 3, 3))
    reads = [r.encode() for r in ds["reads"]]
    dr = e.upload_reads(_blob(reads, pad=True))
    res, _ = e.classify(dr)
    called = res["call_tid"][(res["status"] == 0) & (res["match_type"] <= 2) & (res["call_score"] >= THRESH)]
    strains = [int(t) for t in called if tax.rank.get(int(t)) == "strain"]
    assert strains, "the fixture calls no read at strain level"
    strain = max(set(strains), key=strains.count)

    class F:
        pass
    f = F()
    f.eng, f.ds, f.tax, f.reads, f.dr, f.res = e, ds, tax, reads, dr, res
    f.strain, f.species = strain, tax.parent[strain]
    f.parent = dict(tax.parent)
    yield f
    dr.free()
    e.close()


def _fields(eng, res):
    return [pm.fields_of_result(r, 20, eng.params.min_kmer) for r in res]


def _assert_precondition(fields, thresholds):
    scores = {f[1] for f in fields if f is not None}
    assert not pm.near_threshold(scores, thresholds)


def _std_groups(fx, extra=0):
    """`extra` groups of ids no read is called to, then: one strain | its species as a clade | LowScore | NoDbHits | the rest"""
    g = [([5000000 + 3 * i, 5000001 + 3 * i], 0) for i in range(extra)]
    return g + [([fx.strain], 0), ([fx.species], pm.SUBTREE), ([], pm.LOWSCORE, LOW), ([], pm.NODBHITS), ([], pm.REST)]


def _model_groups(groups):
    return [{"name": str(i), "ids": list(g[0]), "flags": g[1], "low_score": g[2] if len(g) > 2 else 0.0} for i, g in enumerate(groups)]


def _expect(fx, res, reads, first, groups, thresh, min_kmer):
    """group -> (indices into the Reads, offsets, bases) by the model, from fetched records and the reads' own text"""
    mg = _model_groups(groups)
    fields = _fields(fx.eng, res)
    _assert_precondition(fields, [thresh] + [g["low_score"] for g in mg if g["flags"] & pm.LOWSCORE])
    group_of = np.array(pm.select(fields, mg, thresh, min_kmer, pm.key_table(mg, fx.parent)), dtype=np.int64)
    out = {}
    for g in range(len(groups)):
        idx = np.nonzero(group_of == g)[0]
        img = _image([reads[first + i] for i in idx])
        off = np.concatenate([[0], np.cumsum([len(x) for x in img])]).astype(np.uint64)
        out[g] = (idx + first, off, b"".join(img))
    return out, group_of


def _check_run(fx, bins, dr, res, reads, first, count, groups, thresh=THRESH, min_kmer=MIN_KMER, want_bases=True):
    want, group_of = _expect(fx, res, reads, first, groups, thresh, min_kmer)
    got = bins.run(dr, first, count, want_bases=want_bases)
    nr, nb = bins.counts()
    assert set(got) == set(range(len(groups)))
    for g in range(len(groups)):
        idx, off, bases = got[g]
        assert idx.tolist() == want[g][0].tolist(), g
        assert off.tolist() == want[g][1].tolist(), g
        assert int(nr[g]) == len(want[g][0]) and int(nb[g]) == len(want[g][2])
        if want_bases:
            assert bases.tobytes() == want[g][2], g
        else:
            assert bases is None
    return group_of


# ---------------------------------------------------------------------------------------------------------------- 1. replay
@pytest.mark.parametrize("key", sorted(pm.load_goldens()["idfiles"]))
def test_replay_of_the_reference_example(fx, key):
    from lmat_amd import Bins, READ_RESULT_DTYPE
    gold = pm.load_goldens()
    idf = gold["idfiles"][key]
    path = pm.PULL_DIR + "/" + idf["file"]
    groups = pm.parse_idfile(path)
    b = Bins(fx.eng)
    try:
        names = b.set_file(path, idf["thresh"], idf["min_kmer"])
        assert names == [g["name"] for g in groups]
        n_checked = 0
        for run in sorted(gold["runs"]):
            unparsed = {tuple(u) for u in gold["runs"][run]["unparsed"]}
            for si, recs in enumerate(pm.example_shards(gold, run)):
                keep = [ri for ri in range(len(recs)) if (si, ri) not in unparsed]
                res = np.array([pm.result_of_fields(pm.example_fields(recs[ri])[0], 20, fx.eng.params.min_kmer, READ_RESULT_DTYPE) for ri in keep], dtype=READ_RESULT_DTYPE)
                got = b.select_debug(res)
                script = {t[0]: t[1] for t in gold["pulls"][run][si][key]["triples"]}
                for j, ri in enumerate(keep):
                    assert (names[got[j]] if got[j] != pm.NONE else None) == script.get(ri), (run, si, ri)
                n_checked += len(keep)
        assert n_checked == 1008
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------ 2. end to end
def test_end_to_end_on_the_fixture_reads(fx):
    from lmat_amd import Bins
    groups = _std_groups(fx)
    b = Bins(fx.eng)
    try:
        b.set(groups, THRESH, MIN_KMER)
        res, _ = fx.eng.classify(fx.dr)
        assert all((res[f] == fx.res[f]).all() for f in FIELDS)
        group_of = _check_run(fx, b, fx.dr, res, fx.reads, 0, len(fx.reads), groups)
        sizes = [(group_of == g).sum() for g in range(5)]
        assert sizes[0] > 0 and sizes[1] > 0 and sizes[4] > 0 and sum(sizes) == len(fx.reads), sizes   # the clade pulls more than the strain's own group left it
        # calls only, records left on the device: the same lists without bases
        fx.eng.classify_async(fx.dr)
        fx.eng.sync()
        _check_run(fx, b, fx.dr, res, fx.reads, 0, len(fx.reads), groups, want_bases=False)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------------ 3. shapes
def _tiled(fx, n):
    reads = [fx.reads[i % len(fx.reads)] for i in range(n)]
    return reads, fx.eng.upload_reads(_blob(reads, pad=True))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_batch_sizes(fx, n):
    from lmat_amd import Bins, READ_RESULT_DTYPE
    groups = _std_groups(fx)
    reads, dr = _tiled(fx, n)
    b = Bins(fx.eng)
    try:
        b.set(groups, THRESH, MIN_KMER)
        res = fx.eng.classify(dr)[0] if n else np.zeros(0, READ_RESULT_DTYPE)
        _check_run(fx, b, dr, res, reads, 0, n, groups)
    finally:
        b.close()
        dr.free()


@pytest.mark.parametrize("ng", [1, 2, 64, 65, 300])
def test_group_counts(fx, ng):
    """The groups the reads go to come last: with 300 groups their numbers need a second 8-bit digit of the sort."""
    from lmat_amd import Bins
    groups = _std_groups(fx, max(ng - 5, 0))[-ng:] if ng >= 5 else ([([fx.strain], 0), ([], pm.REST)][:ng])
    assert len(groups) == ng
    b = Bins(fx.eng)
    try:
        b.set(groups, THRESH, MIN_KMER)
        res, _ = fx.eng.classify(fx.dr)
        group_of = _check_run(fx, b, fx.dr, res, fx.reads, 0, len(fx.reads), groups)
        assert (group_of == ng - 1).any() and (ng < 5 or (group_of == ng - 5).any())
    finally:
        b.close()


def test_all_reads_in_one_group_and_none_selected(fx):
    from lmat_amd import Bins
    b = Bins(fx.eng)
    try:
        res, _ = fx.eng.classify(fx.dr)
        b.set([([], pm.REST)], THRESH, MIN_KMER)
        assert (_check_run(fx, b, fx.dr, res, fx.reads, 0, len(fx.reads), [([], pm.REST)]) == 0).all()
        none = [([5000000], 0), ([5000001, 5000002], pm.SUBTREE)]
        b.set(none, THRESH, MIN_KMER)
        assert (_check_run(fx, b, fx.dr, res, fx.reads, 0, len(fx.reads), none) == pm.NONE).all()
    finally:
        b.close()


def test_read_lengths_around_the_word_edges(fx):
    """Reads of 0..70 bases (hostile bytes among them: they come back as N) behind fillers of 0..3 bases.  They hit nothing, so
    their records are ReadTooShort rows (fewer than k bases, or fewer than -j 30 valid k-mers), which print the read length or the
    number of valid k-mers where a call prints the taxid, k or 30 as the score and -1 as the third field: with min_kmer = -1 group 0,
    which lists the even numbers, pulls the rows that print one; the rest goes to the REST group.  Selected reads start at every
    output offset mod 16 in both groups together."""
    from lmat_amd import Bins
    rng = np.random.default_rng(161)
    reads = []
    for a in range(4):
        for L in range(71):
            reads.append(_mixed(rng, (a + L) % 4))
            reads.append(_mixed(rng, L))
    groups = [(list(range(0, 71, 2)), 0), ([], pm.REST)]
    dr = fx.eng.upload_reads(_blob(reads, pad=True))
    b = Bins(fx.eng)
    try:
        b.set(groups, 1.0, -1)
        res, _ = fx.eng.classify(dr)
        assert any(c >= 0x80 for r in reads for c in r)
        group_of = _check_run(fx, b, dr, res, reads, 0, len(reads), groups, thresh=1.0, min_kmer=-1)
        assert (group_of == 0).sum() >= 8 and (group_of == 1).sum() >= 8
        want, _ = _expect(fx, res, reads, 0, groups, 1.0, -1)
        blob_at = (0, len(want[0][2]))                                   # the blob is group-major: where a group's text starts in it
        starts = {(blob_at[g] + int(o)) % 16 for g in (0, 1) for o, i in zip(want[g][1][:-1], want[g][0]) if len(reads[i])}
        assert starts == set(range(16))
    finally:
        b.close()
        dr.free()


def test_a_sub_range_of_the_reads(fx):
    from lmat_amd import Bins
    groups = _std_groups(fx)
    b = Bins(fx.eng)
    try:
        b.set(groups, THRESH, MIN_KMER)
        res, _ = fx.eng.classify(fx.dr, first=101, count=203)
        assert all((res[f] == fx.res[f][101:304]).all() for f in FIELDS)
        _check_run(fx, b, fx.dr, res, fx.reads, 101, 203, groups)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------------ 4. errors
def test_errors(fx, tmp_path):
    from lmat_amd import Bins, Engine, LmatError, Params
    b = Bins(fx.eng)
    try:
        b.set(_std_groups(fx), THRESH, MIN_KMER)
        fx.eng.classify(fx.dr, first=0, count=100)
        with pytest.raises(LmatError) as ei:
            b.run(fx.dr, 0, 50)                      # the launch was for 100 reads
        assert ei.value.code == E_STATE
        with pytest.raises(LmatError) as ei:
            b.run(fx.dr, 1, 100)
        assert ei.value.code == E_STATE
        other = fx.eng.upload_reads(_blob(fx.reads[:100], pad=True))
        try:
            with pytest.raises(LmatError) as ei:
                b.run(other, 0, 100)                 # never classified
            assert ei.value.code == E_STATE
        finally:
            other.free()
        b.run(fx.dr, 0, 100)                         # and the launch that was made is still good
        many = tmp_path / "many_ids"
        many.write_text("".join("%d\n" % (7000000 + i) for i in range(65535)))
        with pytest.raises(LmatError) as ei:
            b.set_file(str(many), THRESH, MIN_KMER)
        assert ei.value.code == E_CAPACITY
        with pytest.raises(LmatError) as ei:
            b.set([([1], 0)] * 65535, THRESH, MIN_KMER)
        assert ei.value.code == E_CAPACITY
    finally:
        b.close()
    g = Engine(0, Params.run_rl())
    try:
        g._chk(g.lib.lmat_genedb_begin(g.ctx, 20, 0, 0))
        with pytest.raises(LmatError) as ei:
            Bins(g)
        assert ei.value.code == E_ARG
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------------ 5. stream


def test_stream_lists_and_a_slot_that_grows(fx):
    """Five batches of different sizes through two slots, bins set before the first and cleared before the last.  The third prints
    more candidate pairs than its slot holds (cands_per_read = 1: max_reads + 1024 * 2048): the slot grows, the batch runs again,
    and the lists handed out are those of the records handed out."""
    from lmat_amd import Bins, Stream
    groups = _std_groups(fx)
    mg = _model_groups(groups)
    table = pm.key_table(mg, fx.parent)
    n0 = len(fx.reads)
    per_read = float(fx.res["n_cand"].sum()) / n0
    assert per_read > 4
    big_n = (int((1024 * 2048) / (per_read - 1)) // n0 + 2) * n0          # pairs printed > big_n + 1024 * 2048
    sizes = [n0, 257, big_n, 64, 129]
    assert big_n * per_read > big_n + 1024 * 2048 and big_n < 1_000_000
    bases_cap = sum(len(fx.reads[i % n0]) for i in range(big_n)) + 64
    fields0 = _fields(fx.eng, fx.res)
    _assert_precondition(fields0, [THRESH, LOW])
    group0 = np.array(pm.select(fields0, mg, THRESH, MIN_KMER, table), dtype=np.int64)
    b = Bins(fx.eng)
    st = Stream(fx.eng, max_reads=big_n, max_bases=bases_cap, cands_per_read=1, n_slots=2)
    try:
        b.set(groups, THRESH, MIN_KMER)
        st.set_bins(b)
        grow0 = st.stats()["grow_reruns"]
        pending = []

        def take():
            n, with_bins = pending.pop(0)
            res, cands, tag, lists = st.next()
            assert tag == n and len(res) == n
            tile = np.arange(n) % n0
            for f in FIELDS:
                assert (res[f] == fx.res[f][tile]).all(), f
            if not with_bins:
                assert lists is None
                return
            want = group0[tile]
            assert len(lists) == len(groups)
            for g in range(len(groups)):
                assert lists[g].tolist() == np.nonzero(want == g)[0].tolist(), (n, g)

        for i, n in enumerate(sizes):
            if i == len(sizes) - 1:
                st.set_bins(None)
            if len(pending) == 2:
                take()
            st.submit(*_blob([fx.reads[j % n0] for j in range(n)]), tag=n)
            pending.append((n, i < len(sizes) - 1))
        while pending:
            take()
        assert st.stats()["grow_reruns"] == grow0 + 1
        fx.eng.sync()
    finally:
        st.close()
        b.close()
