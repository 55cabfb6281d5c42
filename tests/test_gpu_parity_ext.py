"""GPU parity, wider cases: reference-pinned lookups, config-1 size, mixed read lengths (U=512 kernel),
parameter variants, taxid-table overflow re-run, async path, and a full-size sample check (config[1])."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DS = os.path.join(G, "ds")


def _blob(reads):
    bs = [r.encode() for r in reads]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


def _engine(ds, params=None):
    from lmat_amd import Engine, Params
    e = Engine(0, params or Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    e.build_db(ds["db"], k=20)
    return e


def _oracle(ds, **opts):
    import oracle_py
    o = oracle_py.Oracle(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    o.add_taxhisto(ds["db"])
    o.set_options(**opts)
    return o


def _compare(eng, orc, reads, first_index=0, cand_per_read=256):
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res, cands = eng.classify(dr, cand_cap=max(cand_per_read * len(reads), 4096))
    got = eng.format_out(res, cands, (blob, off), first_index)
    want, tally, nm = orc.classify(blob, off, 20, first_index)
    dr.free()
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b]
        raise AssertionError(f"{len(bad)} records differ; first: {bad[0]}")
    return res, tally, nm


def _assert_tallies(eng, tally, nm):
    """eng.counts() since the last counts_reset() against the oracle's tally and no-match counters of the same reads: every read
    counted exactly once, whichever class ended up with it."""
    counts, nomatch = eng.counts()
    assert nomatch == nm
    assert {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}


def test_gpu_lookup_matches_reference_sorteddb():
    """The GPU hash returns, for every golden k-mer, what the REFERENCE's SortedDb + TaxNodeStat returned."""
    ds = {k: os.path.join(DS, v) for k, v in dict(tree="tax.dat", depth="depth.dat", rank="rank.txt",
                                                  idmap="map32to16.txt", db="th.bin").items()}
    eng = _engine(ds)
    kms, want = [], []
    for line in open(os.path.join(G, "ref_lookup.txt")):
        f = line.split()
        kms.append(int(f[0]))
        want.append([int(x) for x in f[2:]])
    counts, tids = eng.lookup(np.array(kms, dtype=np.uint64), stride=32)
    for i, w in enumerate(want):
        assert counts[i] == len(w)
        assert tids[i, :len(w)].tolist() == w
    eng.close()


@pytest.fixture(scope="module")
def config1(tmp_path_factory):
    """BASELINE config 1: 10 k reads vs a ~1 M k-mer (10 MB) DB; read lengths mixed 75-300 so the
    512-k-mer kernel class runs too."""
    from lmat_amd import synth
    d = tmp_path_factory.mktemp("cfg1")
    info = synth.generate_dataset(str(d), (2, 2, 2, 2, 3, 3), 13400, 10000, L=(75, 100, 125, 150, 200, 250, 300),
                                  frac_short=0.01, lower_frac=0.02)
    info["reads"] = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
    return info


def test_config1_text_parity(config1):
    assert 0.8e6 < config1["n_kmers"] < 1.3e6
    eng = _engine(config1)
    orc = _oracle(config1)
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, config1["reads"])
    counts, nomatch = eng.counts()
    assert nomatch == nm
    assert {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}
    st = np.bincount(res["status"], minlength=6)
    assert st[0] > 5000 and st[4] > 300  # calls and NoDbHits both well represented
    kinds = np.bincount(res["match_type"][res["status"] == 0], minlength=5)
    assert kinds[0] > 100 and kinds[1] > 100  # DirectMatch and MultiMatch
    orc.close()
    eng.close()


@pytest.mark.parametrize("variant", ["no_p", "hbias3", "phix_off", "strict"])
def test_parameter_variants(config1, variant):
    from lmat_amd import Params
    p = Params.run_rl()
    o = dict(sdiff=1.0, hbias=0.0, prn_all=1, screen_phix=1, min_score=0.0, min_kmer=30, min_fnd_kmer=1)
    if variant == "no_p":
        p.prn_all, o["prn_all"] = 0, 0
    elif variant == "hbias3":
        p.hbias, o["hbias"] = 3.0, 3.0
    elif variant == "phix_off":
        p.screen_phix, o["screen_phix"] = 0, 0
    else:
        p.sdiff, p.min_kmer, p.min_score, p.min_fnd_kmer = 0.25, 35, 0.3, 3
        o.update(sdiff=0.25, min_kmer=35, min_score=0.3, min_fnd_kmer=3)
    eng = _engine(config1, p)
    orc = _oracle(config1, **o)
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, config1["reads"][:3000])
    counts, nomatch = eng.counts()
    assert nomatch == nm and {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}
    orc.close()
    eng.close()


def test_special_taxids_are_exercised(config1):
    """The dataset must actually reach the human / PhiX / plasmid branches the parity tests claim to cover."""
    orc = _oracle(config1)
    blob, off = _blob(config1["reads"])
    text, tally, nm = orc.classify(blob, off, 20)
    assert 9606 in tally and tally[9606][0] > 10          # human call (with 63221 folded in)
    assert 32630 in tally                                  # PhiX short-circuit
    assert any(10000000 <= t < 11000000 for t in tally)    # plasmid override
    orc.close()


def test_taxid_table_overflow_rerun(tmp_path):
    """A k-mer whose list keeps > 128 taxids overflows the fast kernel's table; the engine re-runs the read
    with the 1024-entry kernel on the GPU and still matches the oracle; above 1024 the global-memory class does."""
    from lmat_amd import synth, LmatError
    tax = synth.make_taxonomy((3, 4, 4, 4, 4, 3), specials=False)
    p = synth.write_aux_files(str(tmp_path), tax)
    leaves = tax.leaves[:6]
    tax.leaves = leaves
    genomes = synth.make_genomes(tax, 400, 2002)
    kmers, lists = synth.build_kmer_table(tax, genomes, 20, extra_lists=False)
    all_strains = [t for t in tax.ids if tax.rank[t] == "strain"]
    reads = synth.make_reads(tax, genomes, 40, 150, 3003, err=0.0, frac_random=0.0, frac_n=0.0, frac_lowc=0.0)
    orc_tmp = __import__("oracle_py").Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    km0 = orc_tmp.extract(reads[0][1].encode(), 20)[0]
    km1 = orc_tmp.extract(reads[1][1].encode(), 20)[0]
    orc_tmp.close()
    idx = {int(k): i for i, k in enumerate(kmers.tolist())}
    for j, km in enumerate(km0[:3].tolist()):
        lists[idx[km]] = all_strains[100 * j:100 * j + 300]
    p["db"] = os.path.join(str(tmp_path), "th.bin")
    synth.write_taxhisto(p["db"], kmers, lists, 20)
    eng = _engine(p)
    orc = _oracle(p)
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, [r for _, r in reads], cand_per_read=2048)
    flow = eng.last_counters()
    _assert_tallies(eng, tally, nm)
    assert res["n_cand"].max() > 128
    assert flow["past_fast"] >= 1 and flow["past_e512"] >= 1 and flow["past_large"] == 0, flow   # re-run, and by an LDS class
    eng.close()
    orc.close()
    # > 1024 kept taxids: beyond the large LDS class; the global-memory class (4096 taxids) takes the read
    lists[idx[int(km1[0])]] = all_strains[:1500]
    synth.write_taxhisto(p["db"], kmers, lists, 20)
    eng = _engine(p)
    orc = _oracle(p)
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, [r for _, r in reads], cand_per_read=4096)
    flow = eng.last_counters()
    _assert_tallies(eng, tally, nm)
    assert res["n_cand"].max() > 1024
    assert flow["past_fast"] >= 2 and flow["past_large"] >= 1, flow   # the second read went all the way to the global-memory class
    eng.close()
    orc.close()


def test_many_distinct_lists_in_one_read(tmp_path):
    """More than 64 distinct taxid lists in one read (but few taxids): the fast kernel leaves its
    ballot-peeling of distinct payloads for the LDS-hash path; the result still matches the oracle."""
    import itertools
    from lmat_amd import synth
    tax = synth.make_taxonomy((3, 4, 4, 4, 4, 3), specials=False)
    p = synth.write_aux_files(str(tmp_path), tax)
    tax.leaves = tax.leaves[:6]
    genomes = synth.make_genomes(tax, 400, 2002)
    kmers, lists = synth.build_kmer_table(tax, genomes, 20, extra_lists=False)
    strains = [t for t in tax.ids if tax.rank[t] == "strain"][:12]
    reads = synth.make_reads(tax, genomes, 40, 150, 3003, err=0.0, frac_random=0.0, frac_n=0.0, frac_lowc=0.0)
    orc_tmp = __import__("oracle_py").Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    km = [orc_tmp.extract(reads[i][1].encode(), 20)[0] for i in (0, 1)]
    orc_tmp.close()
    idx = {int(k): i for i, k in enumerate(kmers.tolist())}
    combos = [[s] for s in strains] + [list(c) for c in itertools.combinations(strains, 2)]
    for j, k in enumerate(km[0][:67].tolist()):       # 12 singletons + 55 pairs: 67 payloads, 122 kept ids
        lists[idx[k]] = combos[j]
    for j, k in enumerate(km[1][:100].tolist()):      # 100 payloads, 188 kept ids: also overflows E=128 -> large kernel
        lists[idx[k]] = combos[j % len(combos)] if j < len(combos) else list(strains[:3]) + [strains[3 + j % 8]]
    p["db"] = os.path.join(str(tmp_path), "th.bin")
    synth.write_taxhisto(p["db"], kmers, lists, 20)
    eng = _engine(p)
    orc = _oracle(p)
    eng.counts_reset()
    _, tally, nm = _compare(eng, orc, [r for _, r in reads], cand_per_read=2048)
    flow = eng.last_counters()
    _assert_tallies(eng, tally, nm)
    assert flow["past_fast"] >= 2 and flow["past_e512"] >= 2, flow   # both reads left the fast kernel (its E = 512 form has 64 lists too)
    eng.close()
    orc.close()


def test_async_and_calls_only_agree_with_full_output(config1):
    from lmat_amd import Params
    eng = _engine(config1)
    reads = config1["reads"][:4000]
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res, _ = eng.classify(dr)
    eng.set_params(Params.run_rl(prn_all=0))
    eng.classify_async(dr, 0, len(reads))
    ms, launches = eng.sync()
    res2 = eng.fetch_results(0, len(reads))
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "call_tid", "bin_sel"):
        assert (res[f] == res2[f]).all(), f
    assert (res["call_score"].view(np.uint32) == res2["call_score"].view(np.uint32)).all()
    assert (res["stdev"].view(np.uint32) == res2["stdev"].view(np.uint32)).all()
    assert launches == 1 and ms > 0
    dr.free()
    eng.close()


def _same_records(got, want):
    for f in ("status", "match_type", "cand_kmer_cnt", "valid_kmers", "call_tid", "bin_sel"):
        assert (got[f] == want[f]).all(), f
    for f in ("call_score", "stdev"):
        assert (got[f].view(np.uint32) == want[f].view(np.uint32)).all(), f


def test_async_slices_regrow_both_batch_sets(small_dataset):
    """Queued launches over slices of growing size: the two sets of per-batch buffers are taken in turn, so every launch regrows
    the set it takes (16 -> 112 and 48 -> 224 reads) while the launch before it is still in flight on the other one; a last
    small launch reuses a set as it is.  Tallies and records equal those of one blocking launch over the 400 reads (mixed
    lengths, some below k).  The name matches the child run of test_batches_on_one_stream_give_the_same_answers, which repeats
    this with LMAT_PIPELINE=0: one set, regrown by every launch."""
    from lmat_amd import Params
    ds = small_dataset
    reads = ds["reads"]
    assert len(reads) == 400
    ref = _engine(ds)
    dr = ref.upload_reads(reads)
    ref.counts_reset()
    res0, _ = ref.classify(dr)
    tallies0 = ref.counts()
    dr.free()
    ref.close()
    eng = _engine(ds, Params.run_rl(prn_all=0))   # a fresh engine: both sets start empty
    dr = eng.upload_reads(reads)
    eng.counts_reset()
    lo = 0
    for n in (16, 48, 112, 224):
        eng.classify_async(dr, lo, n)
        lo += n
    assert lo == len(reads)
    eng.sync()
    assert eng.counts() == tallies0
    _same_records(eng.fetch_results(0, 224), res0[176:400])
    eng.classify_async(dr, 0, 16)
    eng.sync()
    _same_records(eng.fetch_results(0, 16), res0[0:16])
    dr.free()
    eng.close()


@pytest.mark.parametrize("gb,n_reads,lens", [(8, 1_000_000, (150,)), (64, 2_000_000, (150,)),
                                             (186, 2_000_000, (75, 100, 125, 150, 200, 250, 300))],
                         ids=["config2-8GiB", "config3-64GiB", "config5-shard-186GiB-mixed"])
def test_full_size_sample_parity(tmp_path, gb, n_reads, lens):
    """BASELINE configs at full table size on one GPU: [1] 1 M reads vs an 8 GB DB, [2] the 64 GB roofline DB, and the
    single-GPU shard of [4]: a 200 GB-class DB (20 G 20-mers, near HBM capacity) with reads of 75-300 bp.  The whole
    batch runs on the GPU; a 20 k-read sample is re-derived by the CPU oracle from lists the HOST derives from the two
    generators (the table's own answers only for collisions and chance hits, both held to their predicted rates) and
    must match byte for byte; size-independent properties are checked on all reads.  (LMAT_TEST_DB_GB /
    LMAT_TEST_READS override the first case, LMAT_TEST_SAMPLE the sample size.)"""
    from lmat_amd import Engine, Params, synth
    import oracle_py
    if gb == 8:
        gb = float(os.environ.get("LMAT_TEST_DB_GB", "8"))
        n_reads = int(os.environ.get("LMAT_TEST_READS", str(n_reads)))
    br = (3, 4, 4, 4, 4, 3)
    eng = Engine(0, Params.run_rl())
    eng.synth_taxonomy(br)
    table_bytes = int(gb * (1 << 30))
    Glen = int(0.8 * (table_bytes / 8) / (768 * (1.0 + 3 * (1 - 0.99 ** 20))))
    eng.synth_db(Glen, k=20, seed=2002, table_bytes=table_bytes)
    assert eng.db_size > 0.7 * table_bytes / 8
    reads = eng.synth_reads(n_reads, lens, seed=3003)
    eng.counts_reset()
    res, cands = eng.classify(reads, cand_cap=40 * n_reads)
    counts, nomatch = eng.counts()
    st = np.bincount(res["status"], minlength=6)
    assert st.sum() == n_reads and st[0] > 0.8 * n_reads
    assert sum(c for c, _ in counts.values()) + sum(nomatch) == n_reads
    assert (res["valid_kmers"][res["status"] == 0] >= 30).all()
    assert set(np.unique(res["read_len"]).tolist()) == set(lens)
    # genome-sampled reads without N: every k-mer is valid
    assert (res["valid_kmers"] == res["read_len"] - 19).mean() > 0.97
    # a call is one of its own candidates or an ancestor reached by the LCA walk: its score is a k-mer fraction
    called = res[res["status"] == 0]
    assert (called["call_score"] > 0).all() and (called["call_score"] <= 1.0).all()
    # sample parity through the oracle
    ns = min(n_reads, int(os.environ.get("LMAT_TEST_SAMPLE", "20000")))  # soak: LMAT_TEST_SAMPLE=200000
    tax = synth.make_taxonomy(br, specials=False)
    p = synth.write_aux_files(str(tmp_path), tax)
    orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
    orc.set_k(20)
    orc.set_options()
    blob, off = reads.ascii(0, ns)
    kms = np.unique(np.concatenate([orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(ns)]))
    space = 4.0 ** 20 / 2                       # canonical 20-mers
    density = eng.db_size / space               # chance that an arbitrary 20-mer is in the table
    # Table CONTENT at full size, against lists derived on the host from the generator's own functions (lmat_synth_window), not
    # from the table: 3000 random ancestor windows, a third of them inside the genus-shared blocks.  The table must return the
    # window's list -- except where ANOTHER window yields the same 20-mer and its payload is the smaller one (a singleton always
    # beats a list, a list another list half the time: ~0.7 of the collisions of a list): predicted share 0.7 x density.
    rng = np.random.default_rng(17)
    blk = Glen * 100 // 1000
    wk, wl = [], []
    for i in range(3000):
        sp = int(rng.integers(0, 768))
        pos = int(rng.integers(0, blk - 20)) if i % 3 == 0 else int(rng.integers(blk, Glen - 20))
        km, lst = eng.synth_window(sp, pos)
        if lst:
            wk.append(km)
            wl.append(sorted(lst))
    wc, wt = eng.lookup(np.array(wk, dtype=np.uint64), stride=32)
    differ = sum(sorted(wt[i, :wc[i]].tolist()) != wl[i] for i in range(len(wk))) / len(wk)
    assert (wc > 0).all() and len(wk) > 2500 and abs(differ - 0.7 * density) <= 0.0075, (differ, 0.7 * density, len(wk))
    assert max(len(l) for l in wl) >= 9 and sum(len(l) == 1 for l in wl) > 100   # genus-spanning lists and lone strains both occur
    # The SAMPLE's lists, host-derived: for every read of the sample the windows that lie in its strain's genome without a
    # substituted base, with the list the database must hold for each (lmat_synth_read_windows: the read generator and the genome
    # generator re-run on the host; nothing read from the device).  The table has to return exactly these, up to the predicted
    # share of k-mers another window took over (0.6 x density for this mix of lists and singletons: 0.1 % at 8 GiB, 0.7 % at
    # 64 GiB, 2 % at 186 GiB) +- 0.5 %.  The oracle's map is filled from the HOST-derived lists; the table's own answer is used
    # only where it differs (a collision, within that share) and for the k-mers nothing can be derived for -- windows with a
    # sequencing error, random and low-complexity reads -- where a hit is a chance hit, whose rate must be the table's density.
    hk, hc, ht = [], [], []
    for i in range(ns):
        a, b, c_ = eng.synth_read_windows(lens, 3003, i)
        hk.append(a); hc.append(b); ht.append(c_)
    hk, hc, ht = np.concatenate(hk), np.concatenate(hc), np.concatenate(ht)
    hk, first_ix = np.unique(hk, return_index=True)
    hc, ht = hc[first_ix], ht[first_ix]
    assert hk.size > 0.5 * kms.size and np.isin(hk, kms).all()   # every derived k-mer is one the oracle extracts from the reads
    gc_, gt_ = eng.lookup(hk, stride=32)
    same_rows = (gc_ == hc) & (np.sort(gt_, axis=1) == np.sort(ht, axis=1)).all(axis=1)
    taken = 1.0 - same_rows.mean()
    assert (gc_ > 0).all() and abs(taken - 0.6 * density) <= 0.005, (taken, 0.6 * density, hk.size)
    rest = np.setdiff1d(kms, hk)
    rc_, rt_ = eng.lookup(rest, stride=32)
    chance = (rc_ > 0).mean()
    assert 0.7 * density <= chance <= 1.3 * density + 0.015, (chance, density, rest.size)   # (+: an error that lands on a sibling strain's variant)
    assert 4 < max(gc_.max(), rc_.max()) <= 17  # strains + species + genus of a genus-block k-mer
    cnts = np.concatenate([np.where(same_rows, hc, gc_), rc_])
    tids = np.concatenate([np.where(same_rows[:, None], ht, gt_), rt_])
    orc.add_lists32(np.concatenate([hk, rest]), cnts, tids)
    want, _, _ = orc.classify(np.append(blob, np.uint8(0)), off, 20)
    got = eng.format_out(res[:ns], cands, (np.append(blob, np.uint8(0)), off))
    assert got == want
    orc.close()
    reads.free()
    eng.close()


# ---- DB ingest tooling ------------------------------------------------------------------
_OPTS = dict(tid_cutoff=2, rank_map=os.path.join(DS, "numeric_ranks.txt"), human_kmers=os.path.join(DS, "human_kmers.txt"),
             adaptor_kmers=os.path.join(DS, "adaptor_kmers.txt"))
_GDS = {k: os.path.join(DS, v) for k, v in dict(tree="tax.dat", depth="depth.dat", rank="rank.txt", idmap="map32to16.txt",
                                                db="th.bin", fasta="reads.fa", names="rank_names.txt").items()}


def test_gpu_lookup_with_build_options_matches_reference(tmp_path):
    """Pruned / human-fed / adaptor-fed database: the GPU hash holds what the REFERENCE's add_data stores; the
    same holds after a save-image / load-image round trip."""
    from lmat_amd import Engine, Params
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(_GDS["tree"], _GDS["depth"], _GDS["rank"], _GDS["idmap"])
    img = str(tmp_path / "db.img")
    eng.build_db(_GDS["db"], k=20, save_image=img, **_OPTS)
    kms, want = [], []
    for line in open(os.path.join(G, "ref_lookup_opts.txt")):
        f = line.split()
        kms.append(int(f[0]))
        want.append([int(x) for x in f[2:]])
    kms = np.array(kms, dtype=np.uint64)
    for phase in ("built", "image"):
        counts, tids = eng.lookup(kms, stride=32)
        for i, w in enumerate(want):
            assert counts[i] == len(w), (phase, int(kms[i]))
            assert tids[i, :len(w)].tolist() == w
        if phase == "built":
            eng.load_image(img)
    eng.close()


def test_classify_parity_on_pruned_database():
    import oracle_py
    from lmat_amd import Engine, Params
    reads = [l.rstrip("\n") for l in open(_GDS["fasta"]) if not l.startswith(">")]
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(_GDS["tree"], _GDS["depth"], _GDS["rank"], _GDS["idmap"])
    eng.build_db(_GDS["db"], k=20, **_OPTS)
    orc = oracle_py.Oracle(_GDS["tree"], _GDS["depth"], _GDS["rank"], _GDS["idmap"])
    orc.set_build_options(_OPTS["tid_cutoff"], _OPTS["rank_map"], _OPTS["human_kmers"], _OPTS["adaptor_kmers"])
    orc.add_taxhisto(_GDS["db"])
    orc.set_options()
    _compare(eng, orc, reads)
    orc.close()
    eng.close()


def test_cli_reads_make_db_image_output(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    img = str(tmp_path / "t.img")
    subprocess.check_call([os.path.join(root, "lmat_amd", "csrc", "make_db_image"), "-i", _GDS["db"], "-o", img, "-k", "20",
                           "-f", _GDS["idmap"]], stdout=subprocess.DEVNULL)
    outs = []
    for tag, db in (("a", _GDS["db"]), ("b", img)):
        out = str(tmp_path / tag)
        r = subprocess.run([os.path.join(root, "lmat_amd", "csrc", "read_label"), "-f", _GDS["idmap"], "-u", _GDS["names"], "-w",
                            _GDS["rank"], "-x", "0", "-j", "30", "-l", "0", "-b", "1.0", "-e", _GDS["depth"], "-p", "-t", "1", "-i",
                            _GDS["fasta"], "-d", db, "-c", _GDS["tree"], "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(open(out + "0.out").read() + open(out + ".0.30.fastsummary").read())
    assert outs[0] == outs[1] and len(outs[0]) > 10000


# ---- null-model scoring (-n) ----------------------------------------
@pytest.fixture(scope="module")
def nullmodel_ds(tmp_path_factory):
    from lmat_amd import synth
    d = tmp_path_factory.mktemp("nm")
    info = synth.generate_dataset(str(d), (2, 2, 2, 2, 3, 3), 2000, 3000, L=(50, 75, 100, 150, 200, 300), frac_short=0.01)
    tax = synth.make_taxonomy((2, 2, 2, 2, 3, 3), True)
    info["null_lst"] = synth.write_null_models(os.path.join(str(d), "nm"), tax)
    info["lmat_dir"] = os.path.join(str(d), "nm")
    info["reads"] = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
    return info


@pytest.mark.parametrize("hbias", [0.0, 3.0])
def test_null_model_text_parity(nullmodel_ds, hbias):
    """log-odds scores against GC-binned null models: GPU (device logf) vs oracle (host libm logf), byte for byte."""
    import oracle_py
    from lmat_amd import Engine, Params
    ds = nullmodel_ds
    os.environ["LMAT_DIR"] = ds["lmat_dir"]
    p = Params.run_rl()
    p.hbias = hbias
    eng = Engine(0, p)
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.build_db(ds["db"], k=20)
    eng.load_null_models(ds["null_lst"])
    orc = oracle_py.Oracle(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    orc.add_taxhisto(ds["db"])
    orc.set_options(hbias=hbias)
    orc.load_null_models(ds["null_lst"])
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, ds["reads"])
    counts, nomatch = eng.counts()
    assert nomatch == nm and {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}
    called = res[res["status"] == 0]
    assert (called["call_score"] < 0).sum() > 20 and (called["call_score"] > 1).sum() > 20  # genuinely log-odds
    assert nm[2] > 0  # LowScore exists now
    # without the tables the same engine goes back to plain fractions
    eng.clear_null_models()
    res2, _ = eng.classify(eng.upload_reads(ds["reads"][:200]))
    assert (res2["call_score"][res2["status"] == 0] <= 1.0).all()
    orc.close()
    eng.close()


def test_cli_with_null_models(nullmodel_ds, tmp_path):
    import subprocess
    import oracle_py
    ds = nullmodel_ds
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "o")
    env = dict(os.environ, LMAT_DIR=ds["lmat_dir"])
    r = subprocess.run([os.path.join(root, "lmat_amd", "csrc", "read_label"), "-f", ds["idmap"], "-u", ds["names"], "-w", ds["rank"],
                        "-x", "0", "-j", "30", "-l", "0", "-b", "1.0", "-n", ds["null_lst"], "-e", ds["depth"], "-p", "-t", "1", "-i",
                        ds["fasta"], "-d", ds["db"], "-c", ds["tree"], "-o", out], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    os.environ["LMAT_DIR"] = ds["lmat_dir"]
    orc = oracle_py.Oracle(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    orc.add_taxhisto(ds["db"])
    orc.set_options()
    orc.load_null_models(ds["null_lst"])
    want, fs, nm = orc.run_file(ds["fasta"], 20, ds["names"])
    orc.close()
    assert open(out + "0.out").read() == want
    assert open(out + ".0.30.nomatchsum").read() == nm
    assert open(out + ".0.30.fastsummary").read() == fs


# ---- run-time pruning (-g/-m), permissive match (-s), 18-mers ------------------------------
@pytest.mark.parametrize("mode", ["prune_ranks", "prune_noranks", "permissive", "permissive_prune"])
def test_label_modes_text_parity(config1, mode):
    import oracle_py
    from lmat_amd import Engine, Params, synth
    ds = config1
    ranks = os.path.join(os.path.dirname(ds["tree"]), "numeric_ranks.txt")
    tax = synth.make_taxonomy((2, 2, 2, 2, 3, 3), True)
    with open(ranks, "w") as f:
        for t in tax.ids:
            f.write(f"{t} {tax.depth[t]}\n")
    perm = mode.startswith("permissive")
    cut = 0 if mode == "permissive" else 2
    rk = ranks if mode in ("prune_ranks", "permissive_prune") else None
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.set_label_modes(perm, cut, rk)
    eng.build_db(ds["db"], k=20)
    orc = oracle_py.Oracle(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    orc.add_taxhisto(ds["db"])
    orc.set_options()
    orc.set_label_modes(perm, cut, rk)
    eng.counts_reset()
    res, tally, nm = _compare(eng, orc, ds["reads"][:3000])
    counts, nomatch = eng.counts()
    assert nomatch == nm and {t: c for t, (c, s) in counts.items()} == {t: c for t, (c, s) in tally.items()}
    # the mode really changes the output
    base = _oracle(ds)
    blob, off = _blob(ds["reads"][:3000])
    t0, _, _ = base.classify(blob, off, 20)
    t1, _, _ = orc.classify(blob, off, 20)
    assert t0 != t1
    base.close()
    orc.close()
    eng.close()


def test_18mer_database(tmp_path):
    from lmat_amd import synth
    info = synth.generate_dataset(str(tmp_path), (2, 2, 2, 2, 3, 3), 1500, 1200, L=(60, 100, 150), k=18)
    reads = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
    eng = _engine_k(info, 18)
    orc = _oracle(info)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res, cands = eng.classify(dr, cand_cap=256 * len(reads))
    got = eng.format_out(res, cands, (blob, off))
    want, _, _ = orc.classify(blob, off, 18)
    assert got == want and eng.k == 18
    assert (res["status"] == 0).sum() > 500
    orc.close()
    eng.close()


def _engine_k(ds, k):
    from lmat_amd import Engine, Params
    e = Engine(0, Params.run_rl())
    e.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    e.build_db(ds["db"], k=k)
    return e


def test_database_of_32bit_taxids_without_id_map():
    """No -f map (upstream's TID_SIZE=32 build): engine and oracle derive storage codes from the tree; the
    text output equals the oracle's and equals the run that uses the 16-bit map."""
    from lmat_amd import Engine, Params
    import oracle_py
    ds = dict(tree=os.path.join(DS, "tax.dat"), depth=os.path.join(DS, "depth.dat"), rank=os.path.join(DS, "rank.txt"),
              idmap=None, db=os.path.join(DS, "th.bin"))
    reads = [l.strip() for l in open(os.path.join(DS, "reads.fa")) if not l.startswith(">")]
    eng = _engine(ds)
    orc = _oracle(ds)
    _compare(eng, orc, reads)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res, cands = eng.classify(dr, cand_cap=256 * len(reads))
    text_nomap = eng.format_out(res, cands, (blob, off), 0)
    eng.close()
    orc.close()
    ds["idmap"] = os.path.join(DS, "map32to16.txt")
    eng = _engine(ds)
    dr = eng.upload_reads((blob, off))
    res, cands = eng.classify(dr, cand_cap=256 * len(reads))
    assert eng.format_out(res, cands, (blob, off), 0) == text_nomap
    eng.close()


def test_long_reads_use_the_global_memory_class(tmp_path):
    """Reads beyond the LDS classes (> 2067 bp, up to 32787 bp) are re-run by the class that keeps its per-read
    tables in global memory; a batch of mostly short reads keeps its fast class.  Longer still: a loud error."""
    from lmat_amd import synth, LmatError
    info = synth.generate_dataset(str(tmp_path), (2, 2, 2, 1, 2, 2), 35000, 60, L=(150, 150, 150, 3000, 12000, 30000))
    reads = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
    assert max(len(r) for r in reads) > 20000 and sum(len(r) < 200 for r in reads) > 10
    eng = _engine(info)
    orc = _oracle(info)
    res, _, _ = _compare(eng, orc, reads, cand_per_read=4096)
    assert (res["status"] == 0).sum() > 40
    # many short reads and one long one: the long one rides the overflow list
    mixed = [r for r in reads if len(r) < 200] * 20 + [max(reads, key=len)]
    _compare(eng, orc, mixed, cand_per_read=512)
    blob, off = _blob(["ACGT" * 10000])
    dr = eng.upload_reads((blob, off))
    with pytest.raises(LmatError) as ei:
        eng.classify(dr)
    assert ei.value.code == -4
    eng.close()
    orc.close()


def test_rand_read_label_tables_match_oracle(tmp_path):
    """rand_read_label (null-model generation): per (taxid, GC bucket) max label_prob and hit count over a read set,
    engine vs the oracle's restatement of src/rand_read_label.cpp + src/rkmer.hpp (no human folding), bit for bit."""
    from lmat_amd import Engine, Params, synth
    import oracle_py
    info = synth.generate_dataset(str(tmp_path), (2, 2, 2, 2, 3, 3), 3000, 3000, L=(100, 150, 150, 250))
    reads = [l.rstrip("\n") for l in open(info["fasta"]) if not l.startswith(">")]
    rng = np.random.default_rng(5)
    reads += ["".join(rng.choice(list("ACGT"), size=150)) for _ in range(500)]   # unrelated reads: mostly no hits
    gc = rng.integers(0, 10, size=len(reads)).astype(np.uint8)
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(info["tree"], info["depth"], info["rank"], info["idmap"])
    eng.rand_mode(True)
    eng.build_db(info["db"], k=20)
    eng.rand_reset(10)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    half = len(reads) // 2
    eng.rand_label(dr, gc[:half], 0, half)              # two calls accumulate
    eng.rand_label(dr, gc[half:], half, len(reads) - half)
    got = eng.rand_table()
    orc = oracle_py.Oracle(info["tree"], info["depth"], info["rank"], info["idmap"])
    orc.add_taxhisto(info["db"])
    want = orc.rand_label(blob, off, 20, gc)
    assert len(want) > 50 and set(got) == set(want)
    for t in want:
        assert (got[t][1] == want[t][1]).all(), t
        assert (got[t][0].view(np.uint32) == want[t][0].view(np.uint32)).all(), t
    # the human variants keep their own rows in this mode when they occur
    eng.close()
    orc.close()


def test_streamed_database_build_equals_buffered(tmp_path, monkeypatch):
    """With the table sized up front the tax_histo files (and images) stream through the insert kernel in chunks;
    chunk boundaries (here every 777 k-mers) must not change a single lookup or call."""
    from lmat_amd import Engine, Params
    ds = dict(tree=os.path.join(DS, "tax.dat"), depth=os.path.join(DS, "depth.dat"), rank=os.path.join(DS, "rank.txt"),
              idmap=os.path.join(DS, "map32to16.txt"), db=os.path.join(DS, "th.bin"))
    reads = [l.strip() for l in open(os.path.join(DS, "reads.fa")) if not l.startswith(">")]
    blob, off = _blob(reads)
    gold = [(int(l.split()[0]), [int(x) for x in l.split()[2:]]) for l in open(os.path.join(G, "ref_lookup.txt"))]
    km = np.array([g[0] for g in gold[::17]], dtype=np.uint64)

    def run(eng):
        counts, tids = eng.lookup(km)
        dr = eng.upload_reads((blob, off))
        res, cands = eng.classify(dr, cand_cap=256 * len(reads))
        return counts.copy(), tids.copy(), eng.format_out(res, cands, (blob, off), 0), eng.db_size

    eng = _engine(ds)
    img = str(tmp_path / "db.img")
    base = run(eng)
    eng.close()
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.build_db(ds["db"], k=20, save_image=img)   # buffered build can still write an image
    eng.close()
    monkeypatch.setenv("LMAT_INGEST_CHUNK", "777")
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.build_db(ds["db"], k=20, n_kmers_hint=base[3])
    streamed = run(eng)
    eng.close()
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.load_image(img)
    from_image = run(eng)
    eng.close()
    for name, other in (("streamed", streamed), ("image", from_image)):
        assert (other[0] == base[0]).all(), name
        bad = np.nonzero((other[1] != base[1]).any(axis=1))[0]
        assert bad.size == 0, (name, int(bad.size), int(km[bad[0]]), base[0][bad[0]], base[1][bad[0]][:8], other[1][bad[0]][:8])
        assert other[2] == base[2] and other[3] == base[3], name


def test_degenerate_reads():
    """Empty, shorter-than-k, all-N, poly-A (one distinct k-mer), single-N-every-19-bases (no valid k-mer), mixed case,
    IUPAC codes, exactly k and k+1 bases, a read repeated verbatim: record by record against the oracle; an empty batch
    and a zero-count classify are no-ops."""
    ds = dict(tree=os.path.join(DS, "tax.dat"), depth=os.path.join(DS, "depth.dat"), rank=os.path.join(DS, "rank.txt"),
              idmap=os.path.join(DS, "map32to16.txt"), db=os.path.join(DS, "th.bin"))
    real = [l.strip() for l in open(os.path.join(DS, "reads.fa")) if not l.startswith(">")]
    r0 = real[0]
    reads = ["", "A", "ACGT" * 4 + "ACG", "N" * 150, "A" * 150, "acgt" * 40, ("ACGTACGTACGTACGTACG" + "N") * 8, r0[:20], r0[:21],
             r0.lower(), r0[:70] + "RYKM" + r0[74:], r0, r0, "T" * 19, "G" * 20, r0[::-1], "ACGTN" * 30, r0[:75] + "N" + r0[76:]]
    eng = _engine(ds)
    orc = _oracle(ds)
    res, _, _ = _compare(eng, orc, reads)
    assert res["status"][0] != 0 and res["status"][11] == res["status"][12]
    # min_kmer 1 lets the short ones through to the lookup
    from lmat_amd import Params
    eng.set_params(Params(1.0, 0.0, 0.0, 1, 1, 1, 1))
    orc.set_options(min_kmer=1)
    _compare(eng, orc, reads)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res0, cands0 = eng.classify(dr, first=3, count=0)
    assert res0.size == 0
    dr.free()
    empty = eng.upload_reads((np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64)))
    assert len(empty) == 0
    empty.free()
    eng.close()
    orc.close()


@pytest.mark.parametrize("dsname", ["ds", "ds2", "ds3", "ds:pruned", "ds:pruned_noranks"])
def test_gpu_label_retrieval_against_reference_rkmer(dsname):
    """The HIP path against the REFERENCE's own retrieve_kmer_labels (src/rkmer.hpp compiled in place,
    tests/golden/ref_rkmer*.txt), without the oracle in between: per taxid, the largest count / valid_kmers over the
    fixture reads and the number of reads that registered it, as the rand_read_label tables hold them."""
    from lmat_amd import Engine, Params
    dsname, _, mode = dsname.partition(":")   # mode: run-time pruning (max_count 2) with / without the numeric rank map
    ds = os.path.join(G, dsname)
    want_max, want_cnt = {}, {}
    tag = ("" if dsname == "ds" else "_" + dsname) + ("_" + mode if mode else "")
    k = 18 if dsname == "ds3" else 20
    for line in open(os.path.join(G, f"ref_rkmer{tag}.txt")):
        f = dict(x.split("=", 1) for x in line.split()[2:] if "=" in x)
        if "valid" not in f or int(f["valid"]) <= 0 or not f.get("reg"):
            continue
        v = np.float32(int(f["valid"]))
        for item in f["reg"].split(","):
            t, c = item.split(":")
            p = np.float32(int(c)) / v
            want_max[int(t)] = max(want_max.get(int(t), np.float32(0)), p)
            want_cnt[int(t)] = want_cnt.get(int(t), 0) + 1
    reads = [l.rstrip("\n") for l in open(os.path.join(ds, "reads.fa")) if not l.startswith(">")]
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(os.path.join(ds, "tax.dat"), os.path.join(ds, "depth.dat"), os.path.join(ds, "rank.txt"), os.path.join(ds, "map32to16.txt"))
    eng.rand_mode(True)
    if mode:
        eng.set_label_modes(False, 2, os.path.join(ds, "numeric_ranks.txt") if mode == "pruned" else None)
    eng.build_db(os.path.join(ds, "th.bin"), k=k)
    eng.rand_reset(10)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    eng.rand_label(dr, np.zeros(len(reads), dtype=np.uint8))
    got = eng.rand_table()
    assert set(got) == set(want_cnt) and len(got) > 100
    for t in want_cnt:
        assert int(got[t][1][0]) == want_cnt[t], t
        assert got[t][0][0].view(np.uint32) == np.float32(want_max[t]).view(np.uint32), t
    eng.close()


def test_gpu_extraction_against_the_example_run(monkeypatch):
    """K1 on the GPU (2-bit packing, canonical 20-mers, N handling, per-read dedupe) against what the REFERENCE
    printed for its own example run (example/example.tgz, 1000 reads of 202 bp): distinct valid k-mers for
    classified reads, valid k-mers for NoDbHits / ReadTooShort rows.  LMAT_STOP_AFTER=2 makes the kernel stop
    after the compaction of first occurrences and report that count."""
    from lmat_amd import Engine, Params
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(G, "example_kmer_counts.tsv"))]
    reads = [r[1] for r in rows]
    monkeypatch.setenv("LMAT_STOP_AFTER", "2")
    eng = Engine(0, Params(1.0, 0.0, 0.0, 1, 1, 1, 1))  # min_kmer 1: every read with a valid k-mer reaches the compaction
    eng.load_taxonomy(os.path.join(DS, "tax.dat"), os.path.join(DS, "depth.dat"), os.path.join(DS, "rank.txt"), os.path.join(DS, "map32to16.txt"))
    eng.build_db(os.path.join(DS, "th.bin"), k=20)
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    res, _ = eng.classify(dr)
    n_dup = 0
    for (hdr, read, kind, what, exp), r in zip(rows, res):
        exp = int(exp)
        if len(read) < 20:
            assert r["status"] == 2 and r["read_len"] == exp, hdr       # ReadTooShort (length)
        elif what == "valid":
            assert r["valid_kmers"] == exp, (hdr, kind)
        else:
            assert r["status"] == 250 and r["cand_kmer_cnt"] == exp, (hdr, kind, int(r["cand_kmer_cnt"]), exp)
            n_dup += exp != len(read) - 19
    assert n_dup >= 40
    eng.close()


# ---- error reporting of the asynchronous path ---------------------------------------------------------------
def test_error_in_a_middle_launch_surfaces_at_sync(nullmodel_ds, tmp_path):
    """Device-side error flags are sticky: of three queued launches only the middle one meets a taxid without a null
    model (upstream asserts there, read_label.cpp:768-775); lmat_sync must still report it, once."""
    import gzip
    from lmat_amd import Engine, Params
    from lmat_amd.capi import LmatError
    ds = nullmodel_ds
    # null models with the root's first child (and nothing else) removed: every read below it fails the lookup
    tree_lines = open(ds["tree"]).read().split("\n")
    drop = None
    nmdir = os.path.join(str(tmp_path), "nm")
    os.makedirs(nmdir)
    lst = os.path.join(nmdir, "null_lst.txt")
    with open(lst, "w") as lf:
        for line in open(ds["null_lst"]):
            kc, name = line.split()
            lf.write(f"{kc} {name}\n")
            rows = gzip.open(os.path.join(ds["lmat_dir"], name), "rt").read().split("\n")
            if drop is None:
                drop = [r.split()[0] for r in rows[1:] if r and r.split()[0] != "1"][0]
            with gzip.open(os.path.join(nmdir, name), "wt") as g:
                g.write("\n".join(r for r in rows if not r or r.split()[0] != drop))
    os.environ["LMAT_DIR"] = nmdir
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.build_db(ds["db"], k=20)
    eng.load_null_models(lst)
    short = ["ACGTACGTAC"] * 64                       # below k: no lookups at all
    normal = [r for r in ds["reads"] if len(r) >= 100][:512]
    dr = eng.upload_reads(short + normal + short)
    eng.classify_async(dr, 0, 64)
    eng.classify_async(dr, 64, len(normal))
    eng.classify_async(dr, 64 + len(normal), 64)
    with pytest.raises(LmatError) as ei:
        eng.sync()
    assert ei.value.code == -5 and "NULL MODELS" in str(ei.value)
    eng.sync()                                        # reported once, then clear
    eng.classify_async(dr, 0, 64)
    eng.sync()
    os.environ["LMAT_DIR"] = ds["lmat_dir"]
    dr.free()
    eng.close()


def test_error_in_a_streamed_batch_belongs_to_that_batch(nullmodel_ds, tmp_path):
    """The streamed boundary keeps a batch's device-side error flags with the batch: of three queued batches only the middle one
    meets a taxid without a null model.  The first comes back fine, the second reports the error -- again when asked again, never
    as a success --, and after it no flag is left behind in the context (lmat_sync) or in the first batch's slot when it is reused."""
    import gzip
    from lmat_amd import Engine, Params, Stream
    from lmat_amd.capi import LmatError
    ds = nullmodel_ds
    drop = None
    nmdir = os.path.join(str(tmp_path), "nm")
    os.makedirs(nmdir)
    lst = os.path.join(nmdir, "null_lst.txt")
    with open(lst, "w") as lf:
        for line in open(ds["null_lst"]):
            kc, name = line.split()
            lf.write(f"{kc} {name}\n")
            rows = gzip.open(os.path.join(ds["lmat_dir"], name), "rt").read().split("\n")
            if drop is None:
                drop = [r.split()[0] for r in rows[1:] if r and r.split()[0] != "1"][0]
            with gzip.open(os.path.join(nmdir, name), "wt") as g:
                g.write("\n".join(r for r in rows if not r or r.split()[0] != drop))
    os.environ["LMAT_DIR"] = nmdir
    try:
        eng = Engine(0, Params.run_rl(prn_all=0))
        eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
        eng.build_db(ds["db"], k=20)
        eng.load_null_models(lst)

        def blob_of(reads):
            bs = [r.encode() for r in reads]
            off = np.zeros(len(bs) + 1, dtype=np.uint64)
            np.cumsum([len(b) for b in bs], out=off[1:])
            return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off

        short = ["ACGTACGTAC"] * 64                       # below k: no lookups at all
        normal = [r for r in ds["reads"] if len(r) >= 100][:512]
        st = Stream(eng, 1024, 1 << 20, cands_per_read=0, n_slots=3)
        st.submit(*blob_of(short), tag=1)
        st.submit(*blob_of(normal), tag=2)
        st.submit(*blob_of(short), tag=3)
        res, _, tag = st.next()
        assert tag == 1 and len(res) == 64
        for _ in range(2):                                # the failed batch never turns into a success
            with pytest.raises(LmatError) as ei:
                st.next()
            assert ei.value.code == -5 and "NULL MODELS" in str(ei.value)
        eng.sync()                                        # nothing leaked into the context's sticky word
        st.close()
        st = Stream(eng, 1024, 1 << 20, cands_per_read=0, n_slots=2)
        for t in (4, 5, 6):                               # slots are reused: old flags do not come back
            st.submit(*blob_of(short), tag=t)
            assert st.next()[2] == t
        st.close()
        eng.close()
    finally:
        os.environ["LMAT_DIR"] = ds["lmat_dir"]


def test_failed_blocking_launch_leaves_the_tallies_alone(small_dataset):
    """lmat_classify with a candidate buffer that is too small fails with LMAT_E_CAPACITY; the documented retry with a
    larger buffer must not count the batch twice."""
    from lmat_amd import Engine, Params
    from lmat_amd.capi import LmatError
    ds = small_dataset
    eng = Engine(0, Params.run_rl())
    eng.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    eng.build_db(ds["db"], k=20)
    dr = eng.upload_reads(ds["reads"])
    eng.counts_reset()
    with pytest.raises(LmatError) as ei:
        eng.classify(dr, cand_cap=8)
    assert ei.value.code == -4
    assert eng.counts() == ({}, [0, 0, 0])
    eng.classify(dr)
    once = eng.counts()
    eng.counts_reset()
    eng.classify(dr)
    assert eng.counts() == once and sum(c for c, _ in once[0].values()) > 100
    dr.free()
    eng.close()


# ---- streamed boundary (lmat_stream_*) and the cross-context merge ------------------------------------------
@pytest.mark.parametrize("prn_all", [1, 0])
def test_stream_equals_blocking_path(config1, prn_all):
    """Batches pushed through the ring of pinned slots (mixed lengths, several batches in flight) give the text and tallies of
    the blocking path.  A slot holds cands_per_read * max_reads + 1024 * 2048 pairs, far more than a thousand of these reads
    print: no slot grows here (asserted) -- the grow path has tests of its own in test_gpu_stream_edges.py."""
    from lmat_amd import Engine, Params, Stream
    eng = _engine(config1, Params.run_rl(prn_all=prn_all))
    reads = config1["reads"][:6000]
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    eng.counts_reset()
    res0, cands0 = eng.classify(dr, cand_cap=256 * len(reads))
    want = eng.format_out(res0, cands0, (blob, off))
    tallies0 = eng.counts()
    dr.free()
    eng.counts_reset()
    st = Stream(eng, max_reads=1000, max_bases=1000 * 300, cands_per_read=2, n_slots=3)
    bounds = list(range(0, len(reads), 1000)) + [len(reads)]
    got, pending = {}, 0
    for bi, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        if st.in_flight == st.n_slots:
            r, cd, tag = st.next()
            got[tag] = (r, cd)
        o = (off[lo:hi + 1] - off[lo]).astype(np.uint64)
        st.submit(np.ascontiguousarray(blob[int(off[lo]):int(off[hi])]), np.ascontiguousarray(o), tag=bi)
    while True:
        x = st.next()
        if x is None:
            break
        got[x[2]] = (x[0], x[1])
    text = ""
    for bi, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        r, cd = got[bi]
        o = (off[lo:hi + 1] - off[lo]).astype(np.uint64)
        text += eng.format_out(r, cd, (np.append(blob[int(off[lo]):int(off[hi])], np.uint8(0)), o), first_index=lo)
    assert text == want
    assert eng.counts() == tallies0
    assert st.stats()["grow_reruns"] == 0 and st.stats()["cand_cap"] == 2 * 1000 + 1024 * 2048
    st.close()
    eng.close()


def test_counts_allreduce_across_contexts(small_dataset):
    """Two contexts (here on one GPU) label disjoint halves; after lmat_counts_allreduce both hold the tallies of the
    whole set -- the merge of read_label.cpp:1760-1800."""
    import ctypes as C
    from lmat_amd import Params
    ds = small_dataset
    a, b, whole = _engine(ds, Params.run_rl()), _engine(ds, Params.run_rl()), _engine(ds, Params.run_rl())
    reads = ds["reads"]
    h = len(reads) // 2
    for e in (a, b, whole):
        e.counts_reset()
    a.classify(a.upload_reads(reads[:h]))
    b.classify(b.upload_reads(reads[h:]))
    whole.classify(whole.upload_reads(reads))
    arr = (C.c_void_p * 2)(a.ctx, b.ctx)
    assert a.lib.lmat_counts_allreduce(arr, 2) == 0
    ca, cb, cw = a.counts(), b.counts(), whole.counts()
    assert ca[1] == cb[1] == cw[1]
    assert {t: c for t, (c, s) in ca[0].items()} == {t: c for t, (c, s) in cb[0].items()} == {t: c for t, (c, s) in cw[0].items()}
    for t, (c, s) in cw[0].items():
        assert abs(ca[0][t][1] - s) < 1e-6 and abs(cb[0][t][1] - s) < 1e-6
    for e in (a, b, whole):
        e.close()


def _child_run(env_name, env_value, files, kexpr):
    """Switches read once per process: the named tests run again in a child pytest with the variable set."""
    import subprocess
    import sys
    if os.environ.get(env_name) is not None:
        pytest.skip("already the child run")
    env = dict(os.environ, **{env_name: env_value})
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(here, f) for f in files], "-m", "gpu", "-x", "-q", "-k", kexpr],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_batches_on_one_stream_give_the_same_answers():
    """Queued launches and the streamed boundary take the two sets of per-batch buffers in turn and the tail of a batch (re-run
    classes, general decision path) runs beside the classify kernel of the next one; LMAT_PIPELINE=0 keeps every launch on the
    context's stream.  The tests that queue batches (async launches, sticky errors, the streamed boundary, the CLI) run both ways."""
    _child_run("LMAT_PIPELINE", "0", ["test_gpu_parity_ext.py", "test_gpu_cli.py"],
               "async or sync or stream or tallies or cli_matches or several_contexts")


def test_general_decision_path_gives_the_same_answers():
    """The decision step (score statistics, std::sort(TCmp), findReadLabelVer2) is made on the classify wave when a read
    qualifies (k4_wave: no null models, no effective human bias, at most 999 candidate k-mers) and by the general path -- a
    statement-by-statement restatement, one lane per read -- otherwise.  LMAT_K4_WAVE=0 sends every read down the general path:
    the text-parity, capacity and fuzz tests must not notice."""
    _child_run("LMAT_K4_WAVE", "0", ["test_gpu_parity_ext.py", "test_gpu_parity.py", "test_gpu_fuzz.py"],
               "text_parity or out_text or parameter_variants or overflow_rerun or many_distinct or degenerate or long_reads or random_configuration or label_modes or example")


def test_decision_by_rows_gives_the_same_answers():
    """LMAT_K4_ROW=1: reads with at most 16 registered taxids are decided by k4_row_kernel (four reads to a wave, a read per row of
    16 lanes) instead of on the classify wave; the measured-slower alternative stays bit-exact."""
    _child_run("LMAT_K4_ROW", "1", ["test_gpu_parity_ext.py", "test_gpu_parity.py", "test_gpu_fuzz.py"],
               "config1_text_parity or out_text or parameter_variants or degenerate or random_configuration or example")


def test_list_records_on_wider_boundaries_give_the_same_answers():
    """LMAT_LIST_SHIFT=2: list records on 64-byte instead of 16-byte boundaries, which is how the 24-bit payloads address an
    arena of 1 GB instead of 256 MB (up to 4 GB at shift 4).  Taxid lists, gene lists and the lookup API read records through the
    same offset rule: the parity tests must not notice."""
    _child_run("LMAT_LIST_SHIFT", "2", ["test_gpu_parity_ext.py", "test_gpu_parity.py", "test_gene_label.py"],
               "config1_text_parity or out_text or lookup or many_distinct or parameter_variants or gene or sorteddb or build_options")


def test_wide_table_format_gives_the_same_answers():
    """LMAT_TABLE_FORMAT=wide keeps round 1's 8-byte-slot table (the non-compact kernel variants share every step after the
    probe with the default ones)."""
    _child_run("LMAT_TABLE_FORMAT", "wide", ["test_gpu_parity_ext.py"],
               "config1_text_parity or parameter_variants or overflow_rerun or many_distinct or degenerate or long_reads or sorteddb")


def _tail_reads(config1, lo, hi, seed):
    """Reads whose k-mer positions end a few past the second 64-lane chunk (lengths lo..hi at k = 20), cut from longer reads of
    config 1, with the cases the looked-up tail has to get right: N's in and before the tail, a tail that repeats an earlier stretch
    of the same read (its k-mers are then not first occurrences), low-complexity reads, and the plain case."""
    import random
    rng = random.Random(seed)
    src = [r for r in config1["reads"] if len(r) >= 200]
    out = []
    for i in range(700):
        L = rng.randint(lo, hi)
        r = src[rng.randrange(len(src))]
        s = rng.randrange(0, len(r) - L + 1)
        r = list(r[s:s + L])
        kind = i % 7
        if kind == 1:    # N inside the tail's windows
            for _ in range(rng.randint(1, 3)):
                r[rng.randrange(L - 30, L)] = "N"
        elif kind == 2:  # N's anywhere
            for _ in range(rng.randint(1, 4)):
                r[rng.randrange(L)] = "N"
        elif kind == 3:  # the tail repeats an earlier stretch: positions 120.. copy positions 20..
            n = L - 120
            r[120:] = r[20:20 + n]
        elif kind == 4:  # low complexity
            unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 9)))
            r = list((unit * (L // len(unit) + 1))[:L])
        elif kind == 5:  # a repeat that straddles the chunk border
            r[100:] = r[40:40 + L - 100]
        out.append("".join(r))
    return out


@pytest.mark.parametrize("lo,hi", [(148, 151), (148, 155), (150, 163), (147, 200)])
def test_reads_ending_just_past_a_chunk(config1, lo, hi):
    """Tail mode (tail_kernel): k-mer positions 128.. of a read of the 160-k-mer class are looked up beforehand, 4 / 8 / 16
    lanes per read by the batch's longest read; the last range mixes in reads of the next class, so the batch is split."""
    eng = _engine(config1)
    orc = _oracle(config1)
    res, _, _ = _compare(eng, orc, _tail_reads(config1, lo, hi, lo * 1000 + hi))
    assert (res["status"] == 0).sum() > 300
    orc.close()
    eng.close()


def test_without_tail_mode_gives_the_same_answers():
    """LMAT_TAIL=0: every read runs all of its chunks on the classify wave, as before tail mode -- now the less travelled path
    for 150 bp reads."""
    _child_run("LMAT_TAIL", "0", ["test_gpu_parity_ext.py", "test_gpu_parity.py", "test_gpu_fuzz.py"],
               "config1_text_parity or out_text or full_size_sample or degenerate or random_configuration or past_a_chunk or example")


# ---- LMATIMG2: the database as it lies in HBM (lmat_db_save_image on a finalized database) ------------------------------
def test_device_image_round_trip(tmp_path, small_dataset):
    """A finalized database is streamed out of HBM (LMATIMG2) and back into a fresh context: same lookups, byte-identical
    .out text, from the API and through `read_label -d <image>`; a context with another taxonomy or other label modes is
    refused (the list records hold internal ids built under both)."""
    import subprocess
    from lmat_amd import Engine, Params
    from lmat_amd.capi import LmatError
    ds = small_dataset
    reads = ds["reads"][:300]

    def text(e):
        dr = e.upload_reads(reads)
        res, cands = e.classify(dr)
        bs = [r.encode() for r in reads]
        off = np.zeros(len(bs) + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        t = e.format_out(res, cands, (np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off))
        dr.free()
        return t

    a = Engine(0, Params.run_rl())
    a.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    a.build_db(ds["db"], k=20)
    want = text(a)
    img = str(tmp_path / "db.img2")
    a.save_device_image(img)
    assert open(img, "rb").read(8) == b"LMATIMG2" and os.path.getsize(img) >= a.table_bytes + a.arena_bytes
    # the header against the format stated in img2_model.py (frame and geometry: the minimum table of k = 20, two low bits in the
    # tag), and the dataset's own buckets read straight from the file -- the other 8 GB are not decoded
    import dbgen_model
    import img2_model
    h = img2_model.check(img, body=False)
    assert (h.k, h.lowbits, h.m, h.W, h.wshift, h.nb) == (20, 2, 17, 31, -1, -(-(1 << 32) // 31))
    assert h.n_kmers == a.db_size and h.bytes_slots + h.bytes_ovf == a.table_bytes and h.bytes_arena == a.arena_bytes
    recs = dbgen_model.read_taxhisto(ds["db"])[2]
    canon = np.array([km for km, _ in recs], dtype=np.uint64)
    canon = canon[canon <= img2_model.revcomp(canon, 20)]                   # (the buckets hold canonical words only)
    found, pay, spilled = img2_model.probe_buckets(img, canon)
    assert found.sum() > 0.9 * canon.size and (found | spilled).all()       # in its home bucket under its tag, or the bucket says where else
    n_list = {km: len(l) for km, l in recs}
    many = np.array([n_list[int(x)] > 1 for x in canon[found].tolist()])
    lp = pay[found]
    assert (lp[many] >= 65536).all() and ((lp[many] - np.uint64(65536)) * np.uint64(16 << h.list_shift) < np.uint64(h.bytes_arena)).all()
    assert ((lp[~many] >= 1) & ((lp[~many] < min(h.n_ids, 65536)) | ((lp[~many] >= 65536) & ((lp[~many] - np.uint64(65536)) * np.uint64(16 << h.list_shift) < np.uint64(h.bytes_arena))))).all()
    rng = np.random.default_rng(5)
    kms = rng.integers(0, 1 << 40, 4000, dtype=np.uint64)
    b = Engine(0, Params.run_rl())
    b.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    b.load_image(img)
    assert b.db_size == a.db_size and b.k == 20
    assert text(b) == want
    ca, ta = a.lookup(kms, stride=32)
    cb, tb_ = b.lookup(kms, stride=32)
    assert (ca == cb).all() and (ta == tb_).all()
    b.close()
    # other label modes / another taxonomy: refused, loudly
    c = Engine(0, Params.run_rl())
    c.load_taxonomy(ds["tree"], ds["depth"], ds["rank"], ds["idmap"])
    c.set_label_modes(permissive=True)
    with pytest.raises(LmatError) as ei:
        c.load_image(img)
    assert "label modes" in str(ei.value)
    c.close()
    from lmat_amd import synth
    other = synth.write_aux_files(str(tmp_path / "other_tax"), synth.make_taxonomy((2, 2, 2, 3, 2, 2), specials=True))
    d = Engine(0, Params.run_rl())
    d.load_taxonomy(other["tree"], other["depth"], other["rank"], other["idmap"])
    with pytest.raises(LmatError) as ei:
        d.load_image(img)
    assert "taxonomy" in str(ei.value)
    d.close()
    a.close()
    # the CLI writes such an image (LMAT_SAVE_DEVICE_IMAGE) and starts from it: the same files as from the tax_histo input
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmat_amd", "csrc", "read_label")
    base = [exe, "-f", ds["idmap"], "-u", ds["names"], "-w", ds["rank"], "-x", "0", "-j", "30", "-l", "0", "-b", "1.0",
            "-e", ds["depth"], "-p", "-t", "1", "-i", ds["fasta"], "-c", ds["tree"]]
    img_b = str(tmp_path / "cli.img2")
    r1 = subprocess.run(base + ["-d", ds["db"], "-o", str(tmp_path / "o1")], env=dict(os.environ, LMAT_SAVE_DEVICE_IMAGE=img_b), capture_output=True, text=True)
    assert r1.returncode == 0, r1.stderr
    assert open(img_b, "rb").read(8) == b"LMATIMG2"
    r2 = subprocess.run(base + ["-d", img_b, "-o", str(tmp_path / "o2")], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    for suffix in ("0.out", ".0.30.fastsummary", ".0.30.nomatchsum"):
        assert open(str(tmp_path / "o1") + suffix).read() == open(str(tmp_path / "o2") + suffix).read(), suffix
    assert len(open(str(tmp_path / "o2") + "0.out").read()) > 1000


# ---- heavy tail of taxid lists (lmat_synth_db_build3): every capacity tier of the classify kernels, against the oracle ------
def test_heavy_tail_lists_parity(tmp_path):
    """Real LMAT lists run to thousands of taxids (doc/lmat-doc.txt:914-931).  The synthetic database gets blocks conserved across a
    whole family / phylum / superkingdom -- k-mers with lists of 69 / 277 / 1109 taxids -- and 3.5 % of the reads come from them:
    more than 64 registered taxids (middle tier, T = 256), more than 256 (large LDS class, T = 1024), more than 1024 (global-memory
    class, T = 4096).  Byte-identical .out text against the CPU oracle, whose lists are derived on the host; then the same reads
    under run-time pruning (-g 64 -m ranks, TaxNodeStat.hpp:76-203), which keeps every read in the fast tiers."""
    from lmat_amd import Engine, Params, synth
    import oracle_py
    br = (3, 4, 4, 4, 4, 3)
    lens, n, seed = (150,), 6000, 3003
    tax = synth.make_taxonomy(br, specials=False)
    p = synth.write_aux_files(str(tmp_path), tax)
    rank_fn = str(tmp_path / "numeric_ranks.txt")
    with open(rank_fn, "w") as f:
        for t in tax.ids:
            f.write(f"{t} {tax.depth[t]}\n")
    table_bytes = int(8.3 * (1 << 30))
    Glen = int(0.8 * (table_bytes / 8) / (768 * (1.0 + 3 * (1 - 0.99 ** 20))))
    for prune in (0, 64):
        eng = Engine(0, Params.run_rl())
        eng.synth_taxonomy(br)
        if prune:
            eng.set_label_modes(False, prune, rank_fn)
        eng.synth_db(Glen, k=20, seed=2002, table_bytes=table_bytes, conserved_permille=(20, 10, 5))
        reads = eng.synth_reads(n, lens, seed=seed)
        eng.counts_reset()
        res, cands = eng.classify(reads, cand_cap=1300 * n)
        flow = eng.last_counters()
        tallies = eng.counts()
        blob, off = reads.ascii(0, n)
        orc = oracle_py.Oracle(p["tree"], p["depth"], p["rank"], p["idmap"])
        orc.set_k(20)
        orc.set_options()
        if prune:
            orc.set_label_modes(False, prune, rank_fn)
        kms = np.unique(np.concatenate([orc.extract(bytes(blob[int(off[i]):int(off[i + 1])]), 20)[0] for i in range(n)]))
        # host-derived lists (the two generators re-run on the host); long ones in a second pass with room for 1109 ids
        hk, hc, ht, long_reads = [], [], [], []
        for i in range(n):
            a, b, c_ = eng.synth_read_windows(lens, seed, i)
            if (b > 32).any():
                long_reads.append(i)
                keep = b <= 32
                a, b, c_ = a[keep], b[keep], c_[keep]
            hk.append(a); hc.append(b); ht.append(c_)
        hk, hc, ht = np.concatenate(hk), np.concatenate(hc), np.concatenate(ht)
        hk, ix = np.unique(hk, return_index=True)
        hc, ht = hc[ix], ht[ix]
        lk, lc, lt = [], [], []
        for i in long_reads:
            a, b, c_ = eng.synth_read_windows(lens, seed, i, stride=1152)
            keep = b > 32
            lk.append(a[keep]); lc.append(b[keep]); lt.append(c_[keep])
        assert len(long_reads) > 0.02 * n
        lk, lc, lt = np.concatenate(lk), np.concatenate(lc), np.concatenate(lt)
        lk, ix = np.unique(lk, return_index=True)
        lc, lt = lc[ix], lt[ix]
        assert set(np.unique(lc).tolist()) == {69, 277, 1109}   # family, phylum and superkingdom lists all occur
        # The oracle prunes raw lists itself, at lookup time (TaxNodeStat::begin), and the engine's records keep the raw list beside
        # the pruned one (lookups return the raw one): with and without -g the oracle is fed the RAW lists -- host-derived where
        # they can be, the table's own answers only for collisions and chance hits.
        gc_, gt_ = eng.lookup(hk, stride=32)
        same = (gc_ == hc) & (np.sort(gt_, axis=1) == np.sort(ht, axis=1)).all(axis=1)
        assert same.mean() > 0.995
        glc, glt = eng.lookup(lk, stride=1152)
        same_l = (glc == lc) & (np.sort(glt, axis=1) == np.sort(lt, axis=1)).all(axis=1)
        assert same_l.mean() > 0.99, same_l.mean()   # (a conserved k-mer another window's singleton took over: the collision share again)
        rest = np.setdiff1d(kms, np.concatenate([hk, lk]))
        rc_, rt_ = eng.lookup(rest, stride=32)
        long_rest = rc_ > 32                          # a chance hit on a conserved k-mer: its list needs the wide lookup
        orc.add_lists32(np.concatenate([hk, rest[~long_rest]]), np.concatenate([np.where(same, hc, gc_), rc_[~long_rest]]),
                        np.concatenate([np.where(same[:, None], ht, gt_), rt_[~long_rest]]))
        orc.add_lists32(lk, np.where(same_l, lc, glc), np.where(same_l[:, None], lt, glt))
        if long_rest.any():
            lrc, lrt = eng.lookup(rest[long_rest], stride=1152)
            orc.add_lists32(rest[long_rest], lrc, lrt)
        if not prune:
            assert flow["past_fast"] > 0.02 * n and flow["past_e512"] > 0.02 * n and flow["past_middle"] > 0.008 * n and flow["past_large"] > 0.002 * n, flow
        else:
            assert flow["past_e512"] <= 2, flow   # pruned lists: nobody needs more than the fast tiers
        want, tally, nm = orc.classify(np.append(blob, np.uint8(0)), off, 20)
        got = eng.format_out(res, cands, (np.append(blob, np.uint8(0)), off))
        assert got == want
        assert tallies[1] == nm and {t: c for t, (c, s) in tallies[0].items()} == {t: c for t, (c, s) in tally.items()}   # every read once, in whichever tier
        orc.close()
        reads.free()
        eng.close()
