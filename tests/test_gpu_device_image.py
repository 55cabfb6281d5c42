"""GPU: device images (LMATIMG2) -- the database as it lies in HBM, lmat_db_save_image on a finalized database and lmat_db_load_image.

Every case is small, so nothing is sampled.  One path serves them all (_round_trip): a database built from records the test wrote is
saved; the file is held to tests/img2_model.py -- the format stated in numpy, independent of the engine: header, geometry, every
bucket, every overflow slot, every payload, the decoded k-mer set -- and to the engine's own counters; then it is loaded into a fresh
context, which must answer every lookup as the source records say, export the source file byte for byte, classify as the building
context did, and save the very same bytes again.

Lookups are word-exact, as SortedDb's are: the stored word answers with its list, the other strand of a k-mer only where the source
holds that word as well (a palindrome is its own other strand).

The refusals patch one good k = 12 image: each damaged file must be refused with a definite code by a context that already holds a
database, and that database must answer as before.  A test never looks up or classifies through an image whose load was expected to
fail: a wrongly accepted load fails the test there and the engine is closed."""
import os
import struct

import numpy as np
import pytest

import dbgen_model as dm
import img2_model as im
from lmat_amd import capi

pytestmark = pytest.mark.gpu
U = np.uint64
BR = (3, 4, 4, 4, 4, 3)
SANITY = 0xFFFFFFFFFFFFFFFF
E_ARG, E_IO, E_TAXONOMY = -1, -2, -5
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- the taxonomy, the records, the reads -----------------------------------------------------------------------------------------
class Aux:
    pass


@pytest.fixture(scope="module")
def aux(tmp_path_factory):
    from lmat_amd import synth
    d = tmp_path_factory.mktemp("img_aux")
    a = Aux()
    a.tax = synth.make_taxonomy(BR, specials=False)
    a.p = synth.write_aux_files(str(d / "aux"), a.tax)
    a.ranks = str(d / "numeric_ranks.txt")
    with open(a.ranks, "w") as f:
        for t in a.tax.ids:
            f.write("%d %d\n" % (t, a.tax.depth[t]))
    a.ids = list(a.tax.ids)
    rng = np.random.default_rng(2)
    a.menu = [[a.ids[int(j)] for j in rng.permutation(len(a.ids))[:n]] for n in [2, 3, 3, 4, 5, 6, 8, 12, 2, 3, 7, 9, 11, 2, 4, 40]]
    return a


def _engine(aux, modes=None, rand=False, idmap=None, depth=None):
    from lmat_amd import Engine, Params
    e = Engine(0, Params.run_rl())
    try:
        e.load_taxonomy(aux.p["tree"], depth or aux.p["depth"], aux.p["rank"], idmap or aux.p["idmap"])
        if modes:
            e.set_label_modes(**modes)
        if rand:
            e.rand_mode(True)
    except Exception:
        e.close()
        raise
    return e


def _write_th(path, k, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQIcI", 29, len(recs), SANITY, 999, b"N", k))
        for i, (km, lst) in enumerate(recs):
            f.write(struct.pack("<QH%dI" % len(lst), km, len(lst), *lst))
            if (i + 1) % 1500 == 0:
                f.write(struct.pack("<Q", SANITY))
    return path


def _genome(n, seed):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def _canon_kmers(codes, k):
    km = np.zeros(codes.size - k + 1, dtype=U)
    for i in range(k):
        km = (km << U(2)) | codes[i:codes.size - k + 1 + i].astype(U)
    return np.unique(np.minimum(km, im.revcomp(km, k)))


def _records(aux, kmers, seed):
    """lists by a draw per k-mer: six of ten a lone leaf (a plain payload), the rest a list from the menu (2 .. 40 ids, stored order)"""
    rng = np.random.default_rng(seed)
    lone = rng.random(kmers.size) < 0.6
    leaf = rng.integers(0, len(aux.tax.leaves), kmers.size)
    pick = rng.integers(0, len(aux.menu), kmers.size)
    return [(int(km), [aux.tax.leaves[int(leaf[i])]] if lone[i] else aux.menu[int(pick[i])]) for i, km in enumerate(kmers.tolist())]


def _reads(codes, n, length, seed):
    """n reads: four of five a stretch of the genome (every tenth reverse-complemented), the rest random"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 5 == 4 or codes is None or codes.size < length:
            r = rng.integers(0, 4, length).astype(np.uint8)
        else:
            s = int(rng.integers(0, codes.size - length + 1))
            r = codes[s:s + length]
            if i % 10 == 3:
                r = (3 - r)[::-1]
        out.append(_ACGT[r].tobytes())
    return out


def _blob(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    return np.frombuffer(b"".join(reads) + b"\0", dtype=np.uint8), off


def _classify(eng, reads):
    """-> (.out text, tallies) of the reads"""
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    eng.counts_reset()
    res, cands = eng.classify(dr, cand_cap=eng.counts_layout()[0] * len(reads))   # (lists drawn from the whole tree: a read may register every id)
    txt = eng.format_out(res, cands, (blob, off))
    per_tid, nomatch = eng.counts()
    dr.free()
    # (the per-taxid score sums are added up by atomics in launch order: the counts are compared, as everywhere in the suite)
    return txt, ({t: c for t, (c, _) in per_tid.items()}, nomatch), int((res["cand_kmer_cnt"] > 0).sum())


def _rand_tables(eng, reads):
    blob, off = _blob(reads)
    dr = eng.upload_reads((blob, off))
    eng.rand_reset(10)
    eng.rand_label(dr, (np.arange(len(reads)) % 10).astype(np.uint8))
    t = eng.rand_table()
    dr.free()
    return {tid: (mx.view(np.uint32).tolist(), ct.tolist()) for tid, (mx, ct) in t.items() if ct.any()}


def _lookups(eng, recs, k, seed=0):
    """every source word, its other strand, and a few thousand absent words; the stride is the longest list"""
    have = dict(recs)
    km = np.array([r[0] for r in recs], dtype=U)
    stride = max(len(l) for _, l in recs)
    counts, tids = eng.lookup(km, stride=stride)
    assert np.array_equal(counts, np.array([len(l) for _, l in recs], dtype=np.uint32))
    want = np.zeros((km.size, stride), dtype=np.uint32)
    for i, (_, l) in enumerate(recs):
        want[i, :len(l)] = l
    assert np.array_equal(tids, want)                                       # ids in stored order, nothing behind a list
    other = im.revcomp(km, k)
    co, to = eng.lookup(other, stride=stride)
    lo = [have.get(int(x), []) for x in other.tolist()]
    assert np.array_equal(co, np.array([len(l) for l in lo], dtype=np.uint32))
    for i in np.nonzero(co)[0].tolist():
        assert to[i, :len(lo[i])].tolist() == lo[i]
    rng = np.random.default_rng(77 + seed)
    absent = rng.integers(0, 1 << (2 * k), 4000, dtype=U)
    absent = absent[~np.isin(absent, km)]
    assert absent.size > (0 if k < 8 else 1000)
    ca, _ = eng.lookup(absent, stride=stride)
    assert not ca.any()


def _round_trip(tmp_path, aux, k, build, reads, modes=None, rand=False, min_hits=10):
    """build(engine) -> the tax_histo file that holds what the engine's database was built from.  -> (header, image, records)"""
    a = _engine(aux, modes, rand)
    b = None
    try:
        src = build(a)
        recs = dm.read_taxhisto(src)[2]
        km = np.array([r[0] for r in recs], dtype=U)
        img = str(tmp_path / "a.img2")
        a.save_device_image(img)
        h = im.check(img, km)                                               # the format, stated independently of the engine
        assert capi.image_check(img) == (0, "")
        assert (h.k, h.n_kmers) == (k, len(recs)) and a.db_size == len(recs) and a.k == k
        assert h.bytes_slots + h.bytes_ovf == a.table_bytes and h.bytes_arena == a.arena_bytes and h.n_lists == a.n_lists
        assert os.path.getsize(img) == h.off_arena + h.bytes_arena
        want = _rand_tables(a, reads) if rand else _classify(a, reads)
        b = _engine(aux, modes, rand)
        b.load_image(img)
        assert (b.k, b.db_size, b.table_bytes, b.arena_bytes, b.n_lists) == (k, len(recs), a.table_bytes, a.arena_bytes, a.n_lists)
        _lookups(b, recs, k)
        out = str(tmp_path / "export.bin")
        b.export_taxhisto(out)
        assert open(out, "rb").read() == open(src, "rb").read()             # the loaded table holds the source file, byte for byte
        got = _rand_tables(b, reads) if rand else _classify(b, reads)
        assert got == want
        assert len(want) > 3 if rand else want[2] >= min_hits               # (the reads do hit the database)
        img2 = str(tmp_path / "b.img2")
        b.save_device_image(img2)
        assert open(img2, "rb").read() == open(img, "rb").read()            # nothing of the image is lost or reordered on the way through HBM
        os.remove(img2)
        return h, img, recs
    finally:
        if b is not None:
            b.close()
        a.close()


def _from_file(aux, tmp_path, k, recs, table_bytes=0):
    src = _write_th(str(tmp_path / "src.bin"), k, recs)

    def build(eng):
        eng.build_db(src, k=k, table_bytes=table_bytes)
        return src
    return build


def _genome_case(aux, tmp_path, k, n_bases, seed, table_bytes=0, read_len=100):
    codes = _genome(n_bases, seed)
    recs = _records(aux, _canon_kmers(codes, k), seed + 1)
    return _from_file(aux, tmp_path, k, recs, table_bytes), _reads(codes, 100, read_len, seed + 2)


# ---- the geometries ------------------------------------------------------------------------------------------------------------------
def test_k10_width_one(aux, tmp_path):
    """k = 10 with 2^14 buckets: W = 1, every minimizer value a bucket of its own, rho always 0"""
    build, reads = _genome_case(aux, tmp_path, 10, 20000, 10, table_bytes=(1 << 14) * 64)
    h, img, _ = _round_trip(tmp_path, aux, 10, build, reads)
    assert (h.nb, h.W, h.wshift, h.lowbits, h.m) == (1 << 14, 1, 0, 0, 7)
    main = np.memmap(img, dtype=im.BUCKET, mode="r", offset=h.off_slots, shape=(h.nb,))
    assert ((np.asarray(main["tag"]).astype(np.int64) - 1) >> 9).max() == 0


def test_k12_power_of_two_width(aux, tmp_path):
    """k = 12 with 4096 buckets: W = 64 = 2^18 / 4096, the shift form of the bucket division"""
    build, reads = _genome_case(aux, tmp_path, 12, 15000, 12, table_bytes=4096 * 64)
    h, _, _ = _round_trip(tmp_path, aux, 12, build, reads)
    assert (h.nb, h.W, h.wshift) == (4096, 64, 6)


def test_k12_minimum_table_with_a_busy_overflow_table(aux, tmp_path):
    """k = 12 at the minimum table: W = 127, 2065 buckets (a request of 2064: 2^18 // 2064 = 127).  The k-mers of ONE random genome,
    so neighbours share minimizers and buckets.  img2_model.address on such genomes puts 8 % of 15 000 k-mers (load 7.3) behind full
    buckets and 12 % of 18 000 (load 8.7): the genome has 18 000 bases, for a tenth in the overflow table with room to spare."""
    build, reads = _genome_case(aux, tmp_path, 12, 18000, 1212, table_bytes=2064 * 64)
    h, img, recs = _round_trip(tmp_path, aux, 12, build, reads)
    assert (h.nb, h.W, h.wshift) == (2065, 127, -1)
    _, _, from_ovf = im.decode(img)
    assert from_ovf.sum() * 10 >= len(recs), (int(from_ovf.sum()), len(recs))
    main = np.memmap(img, dtype=im.BUCKET, mode="r", offset=h.off_slots, shape=(h.nb,))
    assert ((np.asarray(main["hdr"]) & im.COUNT_MASK) == 12).any()


@pytest.mark.parametrize("k,n_bases", [(13, 40000), (16, 150000)])
def test_minimum_tables_by_default_sizing(aux, tmp_path, k, n_bases):
    """no size given: the table is the smallest the 16-bit tag allows, 2^(2k - 6) / 127 buckets (k = 16: 32 MiB, the largest case here)"""
    build, reads = _genome_case(aux, tmp_path, k, n_bases, 100 + k)
    h, _, _ = _round_trip(tmp_path, aux, k, build, reads)
    assert (h.W, h.wshift, h.nb) == (127, -1, -(-(1 << (2 * k - 6)) // 127))


def test_k9_is_wide(aux, tmp_path):
    build, reads = _genome_case(aux, tmp_path, 9, 6000, 9)
    h, _, _ = _round_trip(tmp_path, aux, 9, build, reads)
    assert h.nb == 0 and h.ovf_nbuckets == 0


def test_k20_wide_layout(aux, tmp_path, monkeypatch):
    monkeypatch.setenv("LMAT_TABLE_FORMAT", "wide")
    build, reads = _genome_case(aux, tmp_path, 20, 8000, 20, read_len=150)
    h, _, _ = _round_trip(tmp_path, aux, 20, build, reads)
    assert h.nb == 0 and h.nbuckets >= 16


def _hand_records(aux, k=16):
    enc = lambda s: int("".join(str("ACGT".index(c)) for c in s), 4)
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
    palin = "ACGTACGT" + rc("ACGTACGT")
    noncanon = "TTGACCATGGTACCAT"
    assert len(palin) == len(noncanon) == k and rc(palin) == palin and enc(rc(noncanon)) < enc(noncanon)
    rng = np.random.default_rng(88)
    long_list = [aux.ids[i] for i in rng.permutation(len(aux.ids))[:300].tolist()]
    recs = {enc(palin): [aux.tax.leaves[5], aux.tax.leaves[3]], enc(noncanon): [aux.tax.leaves[9]], enc("ACGGTCATTGCAAGTC"): long_list}
    while len(recs) < 40:
        km = int(rng.integers(0, 1 << (2 * k)))
        recs.setdefault(km, [aux.ids[int(j)] for j in rng.permutation(len(aux.ids))[:int(rng.integers(1, 12))]])
    reads = [("ACGGTCATTGCAAGTC" * 7).encode(), (palin * 7).encode(), (noncanon * 7).encode(), (rc(noncanon) * 7).encode()]
    return sorted(recs.items()), reads + _reads(None, 96, 100, 5), enc(noncanon)


def test_hand_made_records(aux, tmp_path):
    """a palindrome, a word that is not the canonical one of its pair (only the overflow table stores full keys), a list of 300 ids"""
    recs, reads, noncanon = _hand_records(aux)
    h, img, _ = _round_trip(tmp_path, aux, 16, _from_file(aux, tmp_path, 16, recs), reads, min_hits=2)
    km, _, from_ovf = im.decode(img)
    assert from_ovf[km == U(noncanon)].all() and from_ovf.sum() >= 1
    assert h.arena_words * 2 >= 2 * 300 * 3                                           # the long list: kept, sorted and raw ids


def test_list_shift_2(aux, tmp_path, monkeypatch):
    """LMAT_LIST_SHIFT=2: list records on 64-byte boundaries; the header says so and the payload bound of the model uses it"""
    monkeypatch.setenv("LMAT_LIST_SHIFT", "2")
    build, reads = _genome_case(aux, tmp_path, 12, 9000, 122, table_bytes=4096 * 64)
    h, img, _ = _round_trip(tmp_path, aux, 12, build, reads)
    assert h.list_shift == 2
    _, pay, _ = im.decode(img)
    lists = pay[pay >= U(im.LIST_BASE)] - U(im.LIST_BASE)
    assert lists.size and int(lists.max()) * 64 < h.bytes_arena and int(lists.max()) * 16 * 3 < h.bytes_arena


# ---- label modes, build sources -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["permissive", "runtime_pruning", "rand"])
def test_label_modes(aux, tmp_path, mode):
    """saved and loaded under the same modes: -s, -g 4 -m ranks (lists beyond four ids are pruned by rank at run time), rand mode"""
    modes = {"permissive": dict(permissive=True), "runtime_pruning": dict(tid_cutoff=4, rank_map=aux.ranks), "rand": None}[mode]
    build, reads = _genome_case(aux, tmp_path, 12, 9000, 300 + len(mode), table_bytes=4096 * 64)
    _round_trip(tmp_path, aux, 12, build, reads, modes=modes, rand=mode == "rand")


def test_database_built_from_genomes(aux, tmp_path):
    fa = str(tmp_path / "g.fa")
    codes = {leaf: _genome(5000, 500 + i) for i, leaf in enumerate(aux.tax.leaves[:4])}
    codes[aux.tax.leaves[1]][:1500] = codes[aux.tax.leaves[0]][:1500]                 # a shared stretch: lists of more than one id
    with open(fa, "wb") as f:
        for leaf, c in codes.items():
            f.write(b">%d\n%s\n" % (leaf, _ACGT[c].tobytes()))
    src = str(tmp_path / "built.bin")

    def build(eng):
        b = eng._builder(fa, aux.p["tree"], 14)
        try:
            eng._chk(eng.lib.lmat_db_build_from_genomes(eng.ctx, b.h, 0))
            b.write_taxhisto(src)
        finally:
            b.close()
        return src
    h, _, recs = _round_trip(tmp_path, aux, 14, build, _reads(codes[aux.tax.leaves[0]], 100, 100, 6))
    assert h.nb and max(len(l) for _, l in recs) > 1


def test_database_derived_from_an_export(aux, tmp_path):
    codes = _genome(9000, 600)
    recs = _records(aux, _canon_kmers(codes, 12), 601)
    src = _write_th(str(tmp_path / "src.bin"), 12, recs)

    def build(eng):
        s = _engine(aux)
        try:
            s.build_db(src, k=12)
            eng.derive_db(s)
        finally:
            s.close()
        return src
    _round_trip(tmp_path, aux, 12, build, _reads(codes, 100, 100, 602))


def test_load_over_a_database(aux, tmp_path):
    """a context that holds a k = 12 database loads the k = 16 image: the answers are the image's, nothing of the first is left"""
    recs16, reads16, _ = _hand_records(aux)
    codes = _genome(9000, 700)
    recs12 = _records(aux, _canon_kmers(codes, 12), 701)
    a = _engine(aux)
    b = _engine(aux)
    try:
        a.build_db(_write_th(str(tmp_path / "k16.bin"), 16, recs16), k=16)
        img = str(tmp_path / "k16.img2")
        a.save_device_image(img)
        want = _classify(a, reads16)
        b.build_db(_write_th(str(tmp_path / "k12.bin"), 12, recs12), k=12)
        _lookups(b, recs12, 12)
        b.load_image(img)
        assert (b.k, b.db_size, b.table_bytes, b.arena_bytes) == (16, len(recs16), a.table_bytes, a.arena_bytes)
        _lookups(b, recs16, 16)
        assert _classify(b, reads16) == want
        out = str(tmp_path / "out.bin")
        b.export_taxhisto(out)
        assert open(out, "rb").read() == open(str(tmp_path / "k16.bin"), "rb").read()
    finally:
        a.close()
        b.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
class Holder:
    """one good k = 12 image at the minimum table, and a context that holds the database it was saved from"""

    def __init__(self, aux, d):
        self.aux, self.d = aux, d
        codes = _genome(12000, 800)
        self.recs = _records(aux, _canon_kmers(codes, 12), 801)
        self.src = _write_th(str(d / "good.bin"), 12, self.recs)
        self.img = str(d / "good.img2")
        self.eng = None
        e = self.engine()
        e.save_device_image(self.img)
        self.h = im.parse(self.img)
        self.size = os.path.getsize(self.img)

    def engine(self):
        if self.eng is None:
            self.eng = _engine(self.aux)
            self.eng.build_db(self.src, k=12, table_bytes=64)
        return self.eng

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


@pytest.fixture(scope="module")
def holder(aux, tmp_path_factory):
    hd = Holder(aux, tmp_path_factory.mktemp("img_refusals"))
    yield hd
    hd.close()


def _refused(eng, img, code, recs, k=12):
    """load_image(img) must fail with `code` and leave the database of `eng` as it was.  A load that is accepted, or refused with
    another code, fails the test before anything runs on the loaded tables; the caller closes the engine."""
    rc = eng.lib.lmat_db_load_image(eng.ctx, img.encode(), 0)
    msg = eng.lib.lmat_last_error(eng.ctx).decode(errors="replace")
    assert rc == code, "load_image returned %d, expected %d (%s)" % (rc, code, msg if rc else "accepted")
    assert (eng.k, eng.db_size) == (k, len(recs))
    _lookups(eng, recs, k)
    return msg


_NOMINAL = im.make_header(12, 127, ovf_nbuckets=1024)
REFUSAL_IDS = [c[0] for c in im.header_refusals(_NOMINAL, _NOMINAL.off_arena + _NOMINAL.bytes_arena)]


@pytest.mark.parametrize("case", REFUSAL_IDS)
def test_damaged_header_is_refused(holder, tmp_path, case):
    assert (holder.h.nb, holder.h.W, holder.h.wshift, holder.h.lowbits, holder.h.m) == (2065, 127, -1, 0, 9)
    cid, fields, cut, name = [c for c in im.header_refusals(holder.h, holder.size) if c[0] == case][0]
    bad = im.patched(holder.img, str(tmp_path / "bad.img2"), cut=cut, **fields)
    eng = holder.engine()
    try:
        _refused(eng, bad, E_IO, holder.recs)
    except BaseException:
        holder.close()
        raise


def test_trailing_bytes_stay_accepted(holder, tmp_path):
    p = im.patched(holder.img, str(tmp_path / "tail.img2"))
    with open(p, "ab") as f:
        f.write(b"\xAA" * 5000)
    e = _engine(holder.aux)
    try:
        e.load_image(p)
        _lookups(e, holder.recs, 12)
    finally:
        e.close()


def _swapped_idmap(aux, path, recs):
    """the 16-bit map with the codes of two taxids the database stores exchanged: the same tree, the same ids, other codes in the arena"""
    used = sorted({t for _, l in recs if len(l) > 1 for t in l})
    x, y = used[0], used[-1]
    id16 = dict(aux.tax.id16)
    id16[x], id16[y] = id16[y], id16[x]
    with open(path, "w") as f:
        for tid in sorted(aux.tax.ids):
            f.write("%d %d\n" % (tid, id16[tid]))
    return path


def test_another_map_or_depth_is_another_taxonomy(holder, tmp_path):
    """the arena holds the stored 16-bit codes and lookups translate them through the context's map: an image saved under one -f map
    must not load under another map of the same tree (it would answer with exchanged taxids).  Nor under other depths."""
    aux = holder.aux
    other_depth = str(tmp_path / "depth.dat")
    lines = open(aux.p["depth"]).read().split("\n")
    t, d = lines[7].split()
    lines[7] = "%s %d" % (t, int(d) + 1)
    open(other_depth, "w").write("\n".join(lines))
    for kw in (dict(idmap=_swapped_idmap(aux, str(tmp_path / "map.txt"), holder.recs)), dict(depth=other_depth)):
        e = _engine(aux, **kw)
        try:
            e.build_db(holder.src, k=12, table_bytes=64)                 # the file holds 32-bit ids: the same database under either map
            msg = _refused(e, holder.img, E_TAXONOMY, holder.recs)
            assert "taxonomy" in msg
        finally:
            e.close()


def test_other_modes_are_refused(holder, tmp_path):
    aux = holder.aux
    ranks2 = str(tmp_path / "ranks2.txt")
    lines = open(aux.ranks).read().split("\n")
    t, d = lines[5].split()
    lines[5] = "%s %d" % (t, int(d) + 1)
    open(ranks2, "w").write("\n".join(lines))
    pruned = dict(tid_cutoff=4, rank_map=aux.ranks)
    images = {}
    for name, kw in (("rand", dict(rand=True)), ("pruned", dict(modes=pruned))):
        e = _engine(aux, **kw)
        try:
            e.build_db(holder.src, k=12, table_bytes=64)
            images[name] = str(tmp_path / (name + ".img2"))
            e.save_device_image(images[name])
        finally:
            e.close()
    for img, kw in ((holder.img, dict(rand=True)), (images["rand"], dict()),                       # rand mode on one side only
                    (images["pruned"], dict(modes=dict(tid_cutoff=5, rank_map=aux.ranks))),          # another cutoff
                    (images["pruned"], dict(modes=dict(tid_cutoff=4, rank_map=ranks2))),             # another rank map
                    (images["pruned"], dict()), (holder.img, dict(modes=pruned)), (holder.img, dict(modes=dict(permissive=True)))):
        e = _engine(aux, **kw)
        try:
            e.build_db(holder.src, k=12, table_bytes=64)
            msg = _refused(e, img, E_ARG, holder.recs)
            assert "label modes" in msg
        finally:
            e.close()


def test_gene_contexts_and_saving(holder, tmp_path):
    from lmat_amd import Engine, LmatError, Params
    aux = holder.aux
    rng = np.random.default_rng(900)
    gene_recs = [(int(km), sorted({int(g) for g in rng.integers(1, 1 << 20, int(rng.integers(1, 5)))})) for km in np.unique(rng.integers(0, 1 << 24, 500, dtype=U)).tolist()]
    gene_src = _write_th(str(tmp_path / "gene.bin"), 12, gene_recs)
    g = Engine(0, Params.run_rl())
    try:
        g.build_gene_db(gene_src, k=12)
        n = g.db_size
        with pytest.raises(LmatError) as ei:                                  # a gene context saves no device image
            g.save_device_image(str(tmp_path / "gene.img2"))
        assert ei.value.code == E_ARG and not os.path.exists(str(tmp_path / "gene.img2"))
        assert g.lib.lmat_db_load_image(g.ctx, holder.img.encode(), 0) == E_ARG   # ... and loads none
        assert g.db_size == n and n > 400
        c, _ = g.lookup(np.array([r[0] for r in gene_recs], dtype=U), stride=8)
        assert np.array_equal(c, np.array([len(l) for _, l in gene_recs], dtype=np.uint32))
    finally:
        g.close()
    e = _engine(aux)
    try:
        with pytest.raises(LmatError) as ei:                                  # nothing finalized: nothing to save
            e.save_device_image(str(tmp_path / "none.img2"))
        assert ei.value.code == E_ARG and not os.path.exists(str(tmp_path / "none.img2"))
    finally:
        e.close()
    e = holder.engine()
    missing = str(tmp_path / "no_such_dir" / "x.img2")
    with pytest.raises(LmatError) as ei:
        e.save_device_image(missing)
    assert ei.value.code == E_IO and not os.path.exists(os.path.dirname(missing))
    assert _refused(e, str(tmp_path / "no_such_file.img2"), E_IO, holder.recs)
