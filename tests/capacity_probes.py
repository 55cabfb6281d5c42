"""Probe reads whose per-read quantities sit on, just below and just above every capacity of the classify kernels.

Pure Python, no GPU.  A probe is a random ACGT read (seeded generator, never cut from a genome) of which a few k-mer positions
are given designed taxid lists in a tax_histo file that holds nothing else: every other k-mer of the read is absent from the
database, and no k-mer occurs in two probes.  So the four quantities the kernels compare with their capacities are exact:

  P  k-mer positions of the read: len - k + 1.
  D  distinct taxid lists the read meets.  Equal lists are one list (the database stores a list once and a read's positions
     carry a reference to it), so the designed lists of a probe all differ in content.
  E  kept-list elements: the sum of the lengths of those D lists.  A list counts once however many positions carry it.  The
     database keeps the leaf-most ids of a list (an id that stands beside one of its descendants is dropped), so no designed list
     holds an id together with an ancestor of it: kept is what is listed.
  T  registered taxids: the ids of those lists together with all their ancestors up to and including the root.  This is the
     number of candidates the CPU oracle prints for the read (`n_cand` of the engine's record) -- checked for every probe by
     test_capacity_probes.py with T_OFFSET = 0: the root is a candidate like any other ancestor.  (Only the representative
     strain of a species has its lineage walked, but the strains of a species share it, so the union is the same.)

The capacities ("Capacity classes") and the comparison at each edge -- a read stays in a class while
T <= T_cap, E <= E_cap, D <= D_cap and P <= P_cap, and leaves it at cap + 1:

  class    T      E      D    P
  fast     64     256    64   512   (U = 160 / 256 / 320 / 512 by read length)
  e512     64     512    64   512   (the fast kernel with a longer element area; two launches, P <= 160 and P >= 161)
  middle   256    1024   -    512
  large    1024   4096   -    2048
  gmem     4096   16384  -    32768
  beyond: LMAT_E_CAPACITY
  wide taxonomy: w1 128 / 512 (P <= 512), w2 512 / 2048 (P <= 2048), gmem 4096 / 16384

`route()` walks a read down these chains for a batch whose longest read is `max_len`, which is what decides which tiers a
launch has at all; it is written from the table, not from the engine's code.

Two more families are built the same way, each with a builder and a seed of its own (further down): the graded probes
(`build_graded_set`), which add a signal so that every run mode has something to decide in every tier, and the gene probes
(`build_gene_set`), with distinct genes in the place of T."""
import os
import struct
from collections import defaultdict
from dataclasses import dataclass, field

import numpy as np

K = 20
T_OFFSET = 0    # oracle candidates minus |ids + ancestors|; see the docstring
BRANCHING16 = (3, 4, 4, 4, 4, 8)     # 6144 strains, 7168 nodes
BRANCHING_WIDE = (2, 2, 4, 8, 8, 66)  # 67584 strains: beyond any 16-bit numbering
READ_LEN = 150                        # the probes that do not vary the length: 131 k-mer positions, the headline class

NOCAP = 1 << 30
# name, T, E, D, P
CLASSES16 = (("fast", 64, 256, 64, 512), ("e512", 64, 512, 64, 512), ("middle", 256, 1024, NOCAP, 512),
             ("large", 1024, 4096, NOCAP, 2048), ("gmem", 4096, 16384, NOCAP, 32768))
CLASSES_WIDE = (("w1", 128, 512, NOCAP, 512), ("w2", 512, 2048, NOCAP, 2048), ("gmem", 4096, 16384, NOCAP, 32768))
# the cursor word that counts the reads a class passes on, by the name Engine.last_counters() gives it
PASSED_ON = {"fast": "past_fast", "e512": "past_e512", "middle": "past_middle", "large": "past_large", "w1": "past_fast", "w2": "past_e512"}
COUNTERS = ("past_fast", "past_e512", "past_middle", "past_large")


@dataclass
class Probe:
    name: str
    read: str
    T: int
    E: int
    D: int
    P: int
    axis: str           # "T", "E", "D", "P", "long", "plain", "error"
    boundary: int       # the capacity the probe sits at, below or above (0: none)
    expected: str       # the first class of the table that holds it: a CLASSES name, or "error"
    lists: list = field(default_factory=list)       # designed list per chosen position (repeats allowed)
    positions: list = field(default_factory=list)   # the chosen k-mer positions
    shape: str = ""     # graded probes: the signal ("graded", "tied", "human", "phix", "plasmid", "weak")

    @property
    def dims(self):
        return self.T, self.E, self.D, self.P


def holds(cls, T, E, D, P):
    return T <= cls[1] and E <= cls[2] and D <= cls[3] and P <= cls[4]


def expected_class(T, E, D, P, wide=False):
    for cls in (CLASSES_WIDE if wide else CLASSES16):
        if holds(cls, T, E, D, P):
            return cls[0]
    return "error"


def route(dims, max_len, wide=False, mid_on=True, k=K):
    """-> (class that ends up with the read, or "error"; the counters the read adds) in a launch whose longest read has
    max_len bases.  16-bit chain: fast -> e512 -> middle (only while no read exceeds 512 k-mer positions: 531 bp at k = 20;
    never with LMAT_MID_TIER=0) -> large (only while no read exceeds 2048 positions: 2067 bp) -> gmem.  Wide chain: w1 (only
    while no read exceeds 512 positions) -> w2 (only while none exceeds 2048) -> gmem.  A read shorter than k never enters."""
    T, E, D, P = dims
    add = dict.fromkeys(COUNTERS, 0)
    if P <= 0:
        return "none", add
    short_batch, medium_batch = max_len <= 512 + k - 1, max_len <= 2048 + k - 1
    if wide:
        on = {"w1": short_batch, "w2": medium_batch, "gmem": True}
        classes = CLASSES_WIDE
    else:
        on = {"fast": True, "e512": True, "middle": mid_on and short_batch, "large": medium_batch, "gmem": True}
        classes = CLASSES16
    for cls in classes:
        if not on[cls[0]]:
            continue
        if holds(cls, T, E, D, P):
            return cls[0], add
        if cls[0] in PASSED_ON:
            add[PASSED_ON[cls[0]]] += 1
    return "error", add


def closure(tax, ids):
    out = set()
    for t in ids:
        out.add(t)
        out.update(tax.path(t))
    return out


def registered(ids):
    """The ids a read registers for these listed ids: the classifier folds the human variants (63221, 741158) into 9606 when it
    reads a list, so they never take a slot of their own (rand mode keeps them apart)."""
    return {9606 if t in (63221, 741158) else t for t in ids}


def _scramble(ids):
    """File order of a list: fixed, not sorted (as synth.build_kmer_table does)."""
    return sorted(ids, key=lambda x: (x * 2654435761) & 0xFFFFFFFF)


def strains_for_T(tax, strains, target, base=()):
    """Strains taken in order from `strains` (consecutive species) so that |closure(base + them)| == target exactly: the
    shortest prefix that reaches the target, less a few strains of species that keep another one (each such removal takes
    exactly one id out of the closure)."""
    cl = closure(tax, base)
    chosen = []
    for s in strains:
        if len(cl) >= target:
            break
        if s in cl:
            continue
        chosen.append(s)
        cl.add(s)
        cl.update(tax.path(s))
    over = len(cl) - target
    assert over >= 0, "the strain pool is too small for this T"
    if over:
        by_sp = defaultdict(list)
        for s in chosen:
            by_sp[tax.parent[s]].append(s)
        drop = set()
        for ss in by_sp.values():
            while over and len(ss) > 1:
                drop.add(ss.pop())
                over -= 1
        chosen = [s for s in chosen if s not in drop]
    assert len(closure(tax, list(base) + chosen)) == target
    return chosen


def lists_for_E(pool, E):
    """Mutually distinct subsets of `pool` whose lengths add up to E: the pool less its i-th member, i = 0, 1, ...,
    and one shorter list (a prefix of the pool) for the remainder."""
    n = len(pool) - 1
    full, rem = divmod(E, n)
    assert 2 <= full <= len(pool)
    out = [pool[:i] + pool[i + 1:] for i in range(full)]
    if rem:
        out.append(pool[:rem])
    assert sum(len(l) for l in out) == E and len({tuple(sorted(l)) for l in out}) == len(out)
    return out


def read_taxhisto(path):
    """-> {kmer: [taxid32, ...]} of a file synth.write_taxhisto wrote."""
    out = {}
    with open(path, "rb") as f:
        buf = f.read()
    _, n, _, _, _, _ = struct.unpack_from("<IQQIcI", buf, 0)
    at = struct.calcsize("<IQQIcI")
    for i in range(n):
        km, cnt = struct.unpack_from("<QH", buf, at)
        at += 10
        out[km] = list(struct.unpack_from("<%dI" % cnt, buf, at))
        at += 4 * cnt
        if (i + 1) % 1500 == 0:
            at += 8
    assert at == len(buf)
    return out


def measure(tax, table, kmers):
    """(T, E, D) of a read from the k-mers it holds and the database's lists: what the module designed, recomputed."""
    met = {tuple(table[int(km)]) for km in kmers.tolist() if int(km) in table}
    ids = registered(x for l in met for x in l)
    return (len(closure(tax, ids)) + T_OFFSET if ids else 0), sum(len(l) for l in met), len(met)


class _Builder:
    def __init__(self, tax, orc, wide, seed):
        self.tax, self.orc, self.wide = tax, orc, wide
        self.rng = np.random.default_rng(seed)
        self.strains = [t for t in tax.ids if tax.rank[t] == "strain"]
        self.probes = []
        self.table = {}          # kmer -> list
        self.all_kmers = set()   # every k-mer of every probe read, listed or not

    def _read(self, length):
        while True:
            read = "".join("ACGT"[c] for c in self.rng.integers(0, 4, size=length))
            if length < K:
                return read, np.zeros(0, dtype=np.uint64)
            km = self.orc.extract(read.encode(), K)[0]
            s = set(km.tolist())
            if km.size == length - K + 1 and len(s) == km.size and not (s & self.all_kmers):
                self.all_kmers |= s
                return read, km

    def add(self, name, axis, boundary, lists, P=READ_LEN - K + 1, positions=None):
        """lists: one designed list per chosen position; positions default to an even spread over the whole read, the first
        and the last position included (the last ones of a 150 bp read are the looked-up tail)."""
        read, km = self._read(P + K - 1 if P > 0 else 10)
        n = len(lists)
        if positions is None:
            positions = [0] if n == 1 else [int(round(i * (P - 1) / (n - 1))) for i in range(n)]
        assert n <= max(P, 0) and len(set(positions)) == n and all(0 <= p < P for p in positions)
        lists = [_scramble(l) for l in lists]
        for l in lists:   # kept == listed: no id beside an ancestor of it
            assert not set(l) & set(a for t in l for a in self.tax.path(t)), name
        for p, l in zip(positions, lists):
            assert int(km[p]) not in self.table   # no k-mer in two probes (nor twice in one)
            self.table[int(km[p])] = l
        distinct = {tuple(l) for l in lists}
        ids = registered(x for l in distinct for x in l)
        T = len(closure(self.tax, ids)) + T_OFFSET if ids else 0
        E, D = sum(len(l) for l in distinct), len(distinct)
        p = Probe(name, read, T, E, D, max(P, 0), axis, boundary, "error" if axis == "error" else expected_class(T, E, D, P, self.wide),
                  lists, list(positions))
        self.probes.append(p)
        return p

    # ---- the axes ----
    def t_probe(self, name, axis, boundary, T, P=READ_LEN - K + 1, start=0, listed=False):
        """One list (two from 600 ids on, so that no list is long for its own sake) of strains from consecutive species: the
        kernels register the listed ids first and their ancestors in a second pass, and it is that pass which reaches the
        capacity.  listed: the ancestors are listed too, a list per rank (strains, their species, ..., the root), so the
        first pass registers all T and the second finds nothing new -- the other comparison of the same capacity."""
        ids = strains_for_T(self.tax, self.strains[start:], T - T_OFFSET)
        if listed:
            by_depth = defaultdict(list)
            for t in sorted(closure(self.tax, ids)):
                by_depth[self.tax.depth[t]].append(t)
            p = self.add(name, axis, boundary, [by_depth[d] for d in sorted(by_depth, reverse=True)], P)
            assert p.T == T == p.E, (name, p.T, p.E, T)
            return p
        lists = [ids] if len(ids) < 600 else [ids[:len(ids) // 2], ids[len(ids) // 2:]]
        p = self.add(name, axis, boundary, lists, P)
        assert p.T == T, (name, p.T, T)
        return p

    def e_probe(self, name, axis, boundary, E, pool_size, P=READ_LEN - K + 1, start=0):
        p = self.add(name, axis, boundary, lists_for_E(self.strains[start:start + pool_size], E), P)
        assert p.E == E, (name, p.E, E)
        return p

    def d_probe(self, name, D):
        import itertools
        s = self.strains[:12]
        combos = [[x] for x in s] + [list(c) for c in itertools.combinations(s, 2)]
        p = self.add(name, "D", 64, combos[:D])
        assert p.D == D
        return p


def _window(c, top=None):
    return [v for v in (c - 2, c - 1, c, c + 1, c + 2) if top is None or v <= top]


def build_set(outdir, wide=False, seed=7001):
    """Writes taxonomy files and the tax_histo file of the probe set under outdir.
    -> dict: tree / depth / rank / idmap (None for the wide set) / db paths, "tax", "probes" (list of Probe), "wide"."""
    import oracle_py
    from lmat_amd import synth
    tax = synth.make_taxonomy(BRANCHING_WIDE if wide else BRANCHING16, specials=wide)   # (the wide tree as test_gpu_wide.py builds it)
    paths = synth.write_aux_files(outdir, tax)
    if wide:
        assert len(tax.ids) > 65534
        paths["idmap"] = None
    orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], paths["idmap"])
    b = _Builder(tax, orc, wide, seed)
    try:
        if not wide:
            # T: E and D small
            for c in (64, 256, 1024, 4096):
                for T in _window(c, 4096):
                    b.t_probe("T%d" % T, "T", c, T)
            for c in (64, 256, 1024, 4096):
                for T in (c - 1, c, c + 1):
                    if T <= 4096:
                        b.t_probe("TL%d" % T, "T", c, T, listed=True)
            # T = 64 exactly with two sibling strains tied for the top score and a shallow member (a genus of another
            # family) whose ancestors the lineage needs: 64 slots in use, no spare lanes behind the candidates
            sib = b.strains[40:42]
            assert tax.parent[sib[0]] == tax.parent[sib[1]]
            genus = tax.parent[tax.parent[b.strains[4000]]]
            rest = strains_for_T(tax, [s for s in b.strains if s not in sib], 64 - T_OFFSET, base=sib + [genus])
            p = b.add("T64tie", "T", 64, [rest] + [sib] * 5 + [[genus]], positions=[0, 10, 40, 70, 100, 129, 130])
            assert p.T == 64 and p.D == 3
            # E: T at most half the class's T
            for c, pool in ((256, 20), (512, 24), (1024, 96), (4096, 400), (16384, 1600)):
                for E in _window(c, 16384):
                    b.e_probe("E%d" % E, "E", c, E, pool)
            for D in (63, 64, 65, 66):
                b.d_probe("D%d" % D, D)
            # length crossed with capacity: what the fast class passes on (E = 257) and what the E = 512 class passes on too (E = 513)
            for P in (160, 161, 256, 257, 320, 321, 512):
                c = P if P in (160, 256, 320, 512) else P - 1
                b.e_probe("P%d_E257" % P, "P", c, 257, 20, P)
                b.e_probe("P%d_E513" % P, "P", c, 513, 24, P)
            for P in (513, 2048, 2049):
                b.e_probe("long%d_E257" % P, "long", {513: 512, 2048: 2048, 2049: 2048}[P], 257, 20, P)
                b.t_probe("long%d_T65" % P, "long", {513: 512, 2048: 2048, 2049: 2048}[P], 65, P)
            b.add("one_hit", "plain", 0, [[b.strains[77]]])
            b.add("no_hit", "plain", 0, [])
            b.add("short", "plain", 0, [], P=0)
            # beyond the chain: the two causes apart
            b.t_probe("T4097", "error", 4096, 4097)
            b.t_probe("TL4097", "error", 4096, 4097, listed=True)
            p = b.e_probe("E16385", "error", 16384, 16385, 1600)
            assert p.T < 4096
        else:
            for c in (128, 512):
                for T in _window(c):
                    b.t_probe("wT%d" % T, "T", c, T)
            for c in (128, 512):
                for T in (c - 1, c, c + 1):
                    b.t_probe("wTL%d" % T, "T", c, T, listed=True)
            for c, pool in ((512, 40), (2048, 200)):
                for E in _window(c):
                    b.e_probe("wE%d" % E, "E", c, E, pool)
            for P in (513, 2049):
                b.t_probe("wlong%d_T129" % P, "long", {513: 512, 2049: 2048}[P], 129, P)
            b.add("w_one_hit", "plain", 0, [[b.strains[777]]])
            b.add("w_no_hit", "plain", 0, [])
            b.t_probe("wT4097", "error", 4096, 4097)
    finally:
        orc.close()
    kmers = np.array(sorted(b.table), dtype=np.uint64)
    paths["db"] = os.path.join(outdir, "probes.bin")
    synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], K)
    paths.update(tax=tax, probes=b.probes, wide=wide, all_kmers=b.all_kmers)
    return paths


def boundaries(wide=False):
    """Every (axis, capacity) edge of the table that the probe set has to straddle."""
    if wide:
        return [("T", 128), ("T", 512), ("E", 512), ("E", 2048)]
    return [("T", 64), ("T", 256), ("T", 1024), ("T", 4096), ("E", 256), ("E", 512), ("E", 1024), ("E", 4096), ("E", 16384),
            ("D", 64), ("P", 160), ("P", 256), ("P", 320), ("P", 512), ("P", 2048)]


def coverage(probes, wide=False):
    """-> {(axis, c): (values below c, values at c, values above c)} over the probes built for that edge (for P: over all
    probes -- the 150 bp ones are the side below 160)."""
    out = {}
    for axis, c in boundaries(wide):
        vals = sorted({getattr(p, axis) for p in probes
                       if axis == "P" or (p.boundary == c and (p.axis == axis or (p.axis == "error" and getattr(p, axis) > c)))})
        out[(axis, c)] = ([v for v in vals if v < c], [v for v in vals if v == c], [v for v in vals if v > c])
    return out


# ---- graded probes: the same exact T, E, D and P, with a signal -----------------------------------------------------------------
# A probe of build_set puts every designed list on one position, so every candidate scores 1 / P and every run mode decides it the
# same way.  A graded probe adds small lists repeated on many positions -- a repeated list is one list, so the signal costs a
# handful of elements while it spreads the counts --: a lone strain s0, the pair [s0, s1] of sibling strains and two strains of
# another species of the same genus, on about 60, 25 and 10 of 131 positions (in proportion for other lengths).  Then come the bulk
# lists that bring T or E to its target, from strains outside the signal's genus: a bulk list that repeated a signal list would
# merge with it and lose elements.  Positions are a seeded random choice: the order in which the lists are met is not sorted.
GRADED_T = (40, 64, 65, 256, 257, 1024, 1025, 4096)
GRADED_E = ((256, 20), (257, 20), (512, 24), (513, 24), (1024, 96), (1025, 96), (4096, 400), (4097, 400), (16384, 1600))   # E, pool
GRADED_T_WIDE = (128, 129, 512, 513)
GRADED_E_WIDE = ((512, 40), (513, 40), (2048, 200), (2049, 200))
VARIANT_T, VARIANT_E = (65, 257, 1025), ((257, 20), (513, 24), (4097, 400))
# positions of 131: lone strain, sibling pair, cousins, extra list (human / PhiX / plasmid), second extra list (63221)
SHAPES = {"graded": (60, 25, 10, 0, 0), "tied": (0, 80, 12, 0, 0), "human": (35, 14, 6, 25, 12), "phix": (15, 6, 3, 70, 0),
          "plasmid": (40, 18, 8, 28, 0), "weak": (20, 8, 4, 0, 0)}
MIN_KMER_P = 30   # a read of 30 + k - 1 bases: called at -j 30, cut by the strict thresholds' -j 35


class _GradedBuilder(_Builder):
    GC = (0.5, 0.37, 0.63)   # reads drawn with these G + C fractions in turn: more than one GC bin of the null models

    gc_next = None           # ... or with this one, for the next probe only

    def _read(self, length):
        gc, self.gc_next = self.gc_next or self.GC[len(self.probes) % len(self.GC)], None
        while True:
            read = "".join("ACGT"[c] for c in self.rng.choice(4, size=length, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]))
            km = self.orc.extract(read.encode(), K)[0]
            s = set(km.tolist())
            if km.size == length - K + 1 and len(s) == km.size and not (s & self.all_kmers):
                self.all_kmers |= s
                return read, km

    def signal(self, shape, P):
        """-> ([(list, positions)] of the signal, ids that every list of the probe holds).  The genus changes from probe to probe; the plasmid's species is the first one."""
        br = BRANCHING_WIDE if self.wide else BRANCHING16
        per_sp, per_genus = br[-1], br[-1] * br[-2]
        n_genus = len(self.strains) // per_genus
        g = 0 if shape == "plasmid" else n_genus * 3 // 4 + len(self.probes) % (n_genus // 5)
        s0, s1, c0, c1 = (self.strains[g * per_genus + i] for i in (0, 1, per_sp, per_sp + 1))
        assert self.tax.parent[s0] == self.tax.parent[s1] != self.tax.parent[c0] == self.tax.parent[c1]
        assert self.tax.parent[self.tax.parent[s0]] == self.tax.parent[self.tax.parent[c0]]
        extra = {"human": [[9606], [63221]], "phix": [[374840]], "plasmid": [[10000001]]}.get(shape, [])
        if shape == "plasmid":
            assert self.tax.parent[10000001] == self.tax.parent[s0]
        # PhiX, or the plasmid, on every listed position: no candidate scores above it, which is what the short-circuit and the
        # override ask for
        everywhere = {"phix": [374840], "plasmid": [10000001]}.get(shape, [])
        out = []
        for lst, n in zip([[s0] + everywhere, [s0, s1] + everywhere, [c0, c1] + everywhere] + extra, SHAPES[shape]):
            if n:
                out.append((lst, max(1, int(round(n * P / 131.0)))))
        return out, everywhere

    def graded(self, name, axis, boundary, shape, T=None, E=None, pool=0, P=READ_LEN - K + 1):
        sig, everywhere = self.signal(shape, P)
        sig_ids = [x for l, _ in sig for x in l]
        genus = self.tax.parent[self.tax.parent[sig_ids[0]]]
        bulk_pool = [s for s in self.strains[64 if not self.wide else 1056:] if self.tax.parent[self.tax.parent[s]] != genus]
        if T is not None:
            ids = strains_for_T(self.tax, bulk_pool, T - T_OFFSET, base=sorted(registered(sig_ids + everywhere)))
            bulk = [ids] if len(ids) < 600 else [ids[:len(ids) // 2], ids[len(ids) // 2:]]
            bulk = [l + everywhere for l in bulk if l]
        else:   # (every bulk list takes the ids of `everywhere` on top: as many elements less for the lists themselves)
            for n_bulk in range(1, 64):
                bulk = lists_for_E(bulk_pool[:pool], E - len(sig_ids) - n_bulk * len(everywhere))
                if len(bulk) == n_bulk or not everywhere:
                    break
            bulk = [l + everywhere for l in bulk]
        lists = [l for l, n in sig for _ in range(n)] + bulk
        positions = [int(x) for x in self.rng.choice(P, size=len(lists), replace=False)]
        p = self.add(name, axis, boundary, lists, P, positions)
        p.shape = shape
        assert (T is None or p.T == T) and (E is None or p.E == E), (name, p.T, p.E, T, E)
        return p


def build_graded_set(outdir, wide=False, seed=7101):
    """The graded probes, their taxonomy files and their tax_histo file under outdir -> the dict of build_set.  A set of its own:
    its own builder and seed, so build_set's files stay byte for byte what they are.  The 16-bit tree has the special taxids."""
    import oracle_py
    from lmat_amd import synth
    tax = synth.make_taxonomy(BRANCHING_WIDE if wide else BRANCHING16, specials=True)
    paths = synth.write_aux_files(outdir, tax)
    if wide:
        assert len(tax.ids) > 65534
        paths["idmap"] = None
    orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], paths["idmap"])
    b = _GradedBuilder(tax, orc, wide, seed)
    pre = "w" if wide else "g"
    try:
        caps_T, caps_E = ((128, 512), (512, 2048)) if wide else ((64, 256, 1024, 4096), (256, 512, 1024, 4096, 16384))
        edge = lambda v, caps: min(caps, key=lambda c: abs(c - v))
        for T in (GRADED_T_WIDE if wide else GRADED_T):
            b.graded("%sT%d" % (pre, T), "T", edge(T, caps_T), "graded", T=T)
        for E, pool in (GRADED_E_WIDE if wide else GRADED_E):
            b.graded("%sE%d" % (pre, E), "E", edge(E, caps_E), "graded", E=E, pool=pool)
        over = caps_T[0] + 1
        for P in (513, 2049):
            b.graded("%sT%d_P%d" % (pre, over, P), "long", {513: 512, 2049: 2048}[P], "graded", T=over, P=P)
        if not wide:
            b.graded("gT65_P%d" % MIN_KMER_P, "T", 64, "graded", T=65, P=MIN_KMER_P)
            for shape in ("tied", "human"):
                for T in VARIANT_T:
                    b.graded("gT%d_%s" % (T, shape), "T", edge(T, caps_T), shape, T=T)
                for E, pool in VARIANT_E:
                    b.graded("gE%d_%s" % (E, shape), "E", edge(E, caps_E), shape, E=E, pool=pool)
            for T in (40, 65, 257, 1025):            # PhiX in the fast class, the middle tier, the large class and global memory ...
                b.graded("gT%d_phix" % T, "T", edge(T, caps_T), "phix", T=T)
            b.graded("gE257_phix", "E", 256, "phix", E=257, pool=20)    # ... and in the E = 512 class
            b.graded("gT65_plasmid", "T", 64, "plasmid", T=65)
            for P in (160, 161):   # either side of the length that splits the E = 512 class's two launches
                b.graded("gE257_P%d" % P, "P", 160, "graded", E=257, pool=20, P=P)
            b.graded("gT257_weak", "T", 256, "weak", T=257)
            for T in (40, 65):     # G + C above 80 %: GC bin 8 or 9, past the last bin of a table that has eight (fast class, middle tier)
                b.gc_next = 0.86
                b.graded("gT%d_gc" % T, "T", 64, "graded", T=T)
    finally:
        orc.close()
    kmers = np.array(sorted(b.table), dtype=np.uint64)
    paths["db"] = os.path.join(outdir, "graded.bin")
    synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], K)
    paths.update(tax=tax, probes=b.probes, wide=wide, all_kmers=b.all_kmers)
    return paths


def gc_bin(read):
    """bin_sel of an ACGT read: G + C per cent of the bases of its k-mers, in float, over ten (read_label's GC bin)."""
    gc = sum(read.count(c) for c in "GC")
    return int(np.float32(np.float32(gc) / np.float32(len(read)) * np.float32(100.0)) / np.float32(10))


def null_models(outdir, ps):
    """Null-model tables (synth.write_null_models) for a graded set, one per k-mer count of its reads -> (list file, directory for
    LMAT_DIR, k-mer counts).  The 16-bit tree gets a row per taxid; the wide tree (more than 67 000 ids: a row each would take
    longer to write than everything else together) a row for every id its probes can register, which is all a run asks for."""
    from lmat_amd import synth
    tax, counts = ps["tax"], (31, 131, 513, 2049)
    if ps["wide"]:
        import copy
        ids = closure(tax, registered(x for p in ps["probes"] for l in p.lists for x in l))
        tax = copy.copy(tax)
        tax.ids = [t for t in ps["tax"].ids if t in ids]
        counts = (131, 513, 2049)
    d = os.path.join(outdir, "nm")
    return synth.write_null_models(d, tax, kmer_counts=counts), d, counts


# ---- gene mode: the same chain, genes in place of taxids ------------------------------------------------------------------------
# In gene mode (a database of 32-bit gene-id lists, gene_label's vote) the classify chain compares the same quantities with the
# same capacities: G, the distinct genes a read's lists hold, takes the place of T (a gene has no ancestors); E, D and P are what
# they are for taxid lists.  The per-read tables key a 32-bit id in the 32-bit hash entries the taxid tables have anyway, so no
# capacity shrinks.  A gene probe has a winner gene alone on about 40 positions -- the top vote is unique -- and bulk lists of
# fresh genes that bring G or E to its target; ids are drawn from the whole 32-bit range, about half of them above 2^31.
GENE_G = (64, 65, 256, 257, 1024, 1025, 4096)
GENE_E = GRADED_E


def build_gene_set(outdir, seed=7201):
    """-> {"db": tax_histo file of gene-id lists, "probes": [Probe with T = G], "beyond": Probe (G = 4097), "ties": [Probe, Probe]}"""
    from lmat_amd import synth
    rng = np.random.default_rng(seed)
    ids = np.unique(rng.integers(1, 2 ** 32 - 1, size=60000, dtype=np.uint64))
    ids = [int(x) for x in rng.permutation(ids)]
    assert sum(x >= 2 ** 31 for x in ids) > len(ids) // 3
    table, seen, probes = {}, set(), []
    os.makedirs(outdir, exist_ok=True)

    def fresh(n):
        out = ids[:n]
        del ids[:n]
        assert len(out) == n
        return out

    def add(name, axis, boundary, lists, positions=None, P=READ_LEN - K + 1):
        while True:
            codes = rng.integers(0, 4, size=P + K - 1, dtype=np.uint8)
            km = synth.kmers_of(codes, K)
            s = set(km.tolist())
            if len(s) == km.size and not (s & seen):
                seen.update(s)
                break
        if positions is None:
            positions = [int(x) for x in rng.choice(P, size=len(lists), replace=False)]
        for p, l in zip(positions, lists):
            table[int(km[p])] = list(l)
        distinct = {tuple(l) for l in lists}
        G, E, D = len({x for l in distinct for x in l}), sum(len(l) for l in distinct), len(distinct)
        pr = Probe(name, "".join("ACGT"[c] for c in codes), G, E, D, P, axis, boundary, expected_class(G, E, D, P), [list(l) for l in lists], list(positions))
        probes.append(pr)
        return pr

    for G in GENE_G + (4097,):
        bulk = fresh(G - 1)
        p = add("G%d" % G, "T", min((64, 256, 1024, 4096), key=lambda c: abs(c - G)), [fresh(1)] * 40 + [bulk[i:i + 500] for i in range(0, len(bulk), 500)])
        assert p.T == G == p.E
    for E, pool in GENE_E:
        p = add("GE%d" % E, "E", min((256, 512, 1024, 4096, 16384), key=lambda c: abs(c - E)), [fresh(1)] * 40 + lists_for_E(fresh(pool), E - 1))
        assert p.E == E and p.T == pool + 1
    # two genes on equal top votes, ids on either side of 2^31; the smaller one met first, and the larger one met first
    lo, hi = 0x7FFFFFF0, 0x80000010
    assert lo not in ids and hi not in ids
    ties = [add("tie_small_first", "plain", 0, [[lo]] * 30 + [[hi]] * 30 + [[g] for g in fresh(5)], list(range(10, 40)) + list(range(50, 80)) + [0, 5, 45, 90, 130]),
            add("tie_large_first", "plain", 0, [[hi]] * 30 + [[lo]] * 30 + [[g] for g in fresh(5)], list(range(10, 40)) + list(range(50, 80)) + [0, 5, 45, 90, 130])]
    kmers = np.array(sorted(table), dtype=np.uint64)
    db = os.path.join(outdir, "genes.bin")
    synth.write_taxhisto(db, kmers, [table[int(km)] for km in kmers.tolist()], K)
    beyond = [p for p in probes if p.name == "G4097"][0]
    assert beyond.expected == "error"
    return {"db": db, "probes": [p for p in probes if p is not beyond and p not in ties], "beyond": beyond, "ties": ties}


# ---- the run modes the graded probes are classified in (oracle options; the GPU tests set the same on the engine) ---------------
STRICT = dict(sdiff=0.25, min_kmer=35, min_score=0.3, min_fnd_kmer=3)
G_CUTOFF = 500    # -g: lists of more than 500 ids are pruned -- the T = 1025, 257 and 65 probes keep theirs (at most 445 ids a list)


def rank_map(outdir, tax):
    """The -m file of -g: a numeric rank (the depth) per taxid."""
    fn = os.path.join(outdir, "numeric_ranks.txt")
    with open(fn, "w") as f:
        for t in tax.ids:
            f.write("%d %d\n" % (t, tax.depth[t]))
    return fn


def mode_oracle(ps, options=None, null_lst=None, permissive=False, cutoff=0, ranks=None):
    import oracle_py
    orc = oracle_py.Oracle(ps["tree"], ps["depth"], ps["rank"], ps["idmap"])
    orc.add_taxhisto(ps["db"])
    orc.set_options(**(options or {}))
    if null_lst:
        orc.load_null_models(null_lst)
    if permissive or cutoff:
        orc.set_label_modes(permissive, cutoff, ranks)
    return orc


def record_call(line):
    """-> (taxid, score, match type) of a .out record, or (None, None, reason) for a record without a call."""
    f = line.split("\t")[-1].split()
    if len(f) == 3 and f[2].endswith("Match"):
        return int(f[0]), float(f[1]), f[2]
    return None, None, f[-1]
