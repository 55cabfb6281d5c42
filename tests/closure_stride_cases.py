"""The closure of a read with several eligible ids, walked at a fixed stride (kernels.hip classify_one):
a host model of it, and the designed reads test_gpu_closure_stride.py classifies.  Pure Python, no GPU.

The model restates what the wave does after phase 1 has registered the kept ids (their slots are taken from the oracle's registration
order, which phase 1 reproduces): which kept ids are eligible, the elements in their order (distinct list in first-occurrence order,
then ascending id), the first eligible element of every slot, and then either

  * the walk at a fixed stride: nch walked chains, S the largest power of two with nch * S <= 64, taken when no walked chain is longer
    than S and there are at most 64 elements; item lane i serves entry i & (S - 1) of chain i >> log2 S (chains in element order),
    the lowest lane of a new id registers it, new slots go by the rank among those lanes; the ancestor mask of a chain's id is the
    OR of 1 << slot over its item lanes; or
  * the general steps: the dense item list, and per eligible id the slots whose Euler interval lies strictly around its own.

Both end in the same counts: count[a] += m_d for every list d that holds an eligible id below a and does not keep a itself."""
import os

import numpy as np

import capacity_probes as cp

T_CAP, E_CAP = 64, 64   # slots of the fast classes; elements of one chunk


# ---- taxonomy helpers ---------------------------------------------------------------------------------------------------------------
def renumber16(tax):
    """The 16-bit map over again (root -> 1, the rest dense from 2 in ascending 32-bit order) after nodes were added."""
    tax.id16 = {1: 1}
    for n, tid in enumerate(sorted(t for t in tax.ids if t != 1)):
        tax.id16[tid] = n + 2
    return tax


def species_of(tax, t):
    for a in tax.path(t):
        if tax.rank[a] == "species":
            return a
    return 0


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def closure(tax, lists, reg1, stride=True):
    """lists: the read's distinct lists in first-occurrence order, [(kept ids, positions that carry the list, negative-first flag)];
    reg1: the kept ids in the order phase 1 registered them.  A list whose raw count reads negative as int16 (32768 entries or more)
    keeps its ids, but its positions take no part in the closure: its elements are eligible nowhere and its set gains no ancestors.  -> dict(taken=the fixed-stride walk ran, nch, lgS, reg=registration order after the closure,
    cnt={id: positions whose set holds it}), or dict(overflow=True, taken=...) when the closure passes 64 slots."""
    slot = {t: i for i, t in enumerate(reg1)}
    reg = list(reg1)
    cnt = {t: 0 for t in reg1}
    for ids, m, _ in lists:
        for t in ids:
            cnt[t] += m
    # representative strain per species: most positions, ties to the smallest id
    best = {}
    for t in sorted(reg1):
        if tax.rank[t] == "strain":
            sp = species_of(tax, t)
            if sp and (sp not in best or cnt[t] > cnt[best[sp]]):
                best[sp] = t
    elig = {t for t in reg1 if tax.rank[t] != "strain" or best.get(species_of(tax, t)) == t}
    elements = [(d, t) for d, (ids, _, _) in enumerate(lists) for t in sorted(ids)]
    first = {}
    for e, (d, t) in enumerate(elements):
        if t in elig and not lists[d][2]:
            first.setdefault(t, e)
    walked = [t for e, (d, t) in enumerate(elements) if first.get(t) == e]   # element order
    nch = len(walked)
    out = dict(taken=False, nch=nch, lgS=0, nel=len(elements))
    mask = {}
    if stride and nch != 1 and len(elements) <= E_CAP:
        lgS = 6 - (nch - 1).bit_length() if nch > 1 else 0
        out["lgS"] = lgS
        out["taken"] = all(len(tax.path(t)) <= (1 << lgS) for t in walked)
    if out["taken"]:
        S = 1 << lgS
        lanes = [None] * 64
        for c, t in enumerate(walked):
            for rel, a in enumerate(tax.path(t)):
                lanes[c * S + rel] = a
        new = []
        for a in lanes:
            if a is not None and a not in slot and a not in new:
                new.append(a)
        if len(reg) + len(new) > T_CAP:
            return dict(out, overflow=True)
        for a in new:
            slot[a] = len(reg)
            reg.append(a)
        for c, t in enumerate(walked):
            mask[t] = 0
            for a in lanes[c * S:(c + 1) * S]:
                if a is not None:
                    mask[t] |= 1 << slot[a]
    else:
        items = [a for t in walked for a in tax.path(t)]
        for i0 in range(0, len(items), 64):
            new = []
            for a in items[i0:i0 + 64]:
                if a not in slot and a not in new:
                    new.append(a)
            if len(reg) + len(new) > T_CAP:
                return dict(out, overflow=True)
            for a in new:
                slot[a] = len(reg)
                reg.append(a)
        tin, tout = euler(tax)
        for t in walked:
            mask[t] = sum(1 << slot[a] for a in reg if tin[a] < tin[t] and tout[t] <= tout[a])
    for a in reg[len(reg1):]:
        cnt[a] = 0
    if walked and any(tax.path(t) for t in walked):
        for d, (ids, m, neg) in enumerate(lists):
            mem = sum(1 << slot[t] for t in ids)
            hit = 0
            for t in ids:
                if t in elig and not neg:
                    hit |= mask[t]
            for a in reg:
                if (hit & ~mem) >> slot[a] & 1:
                    cnt[a] += m
    return dict(out, overflow=False, reg=reg, cnt=cnt)


def euler(tax):
    """Euler-tour intervals over the tree (taxonomy.cpp build_euler_intervals): a above b <=> tin[a] < tin[b] and tout[b] <= tout[a]."""
    tin, tout, clock = {}, {}, [0]
    roots = [t for t in tax.ids if tax.parent[t] == t]
    for r in roots:
        stack = [(r, 0)]
        tin[r] = clock[0]
        clock[0] += 1
        while stack:
            t, k = stack.pop()
            ch = tax.children[t]
            if k < len(ch):
                stack.append((t, k + 1))
                tin[ch[k]] = clock[0]
                clock[0] += 1
                stack.append((ch[k], 0))
            else:
                tout[t] = clock[0] - 1
    return tin, tout


def parse_trace(line):
    """One line of Oracle.rkmer_trace -> ([registered ids in order], {id: count})."""
    reg = line.split(" reg=")[1].strip()
    pairs = [x.split(":") for x in reg.split(",")] if reg else []
    return [int(t) for t, _ in pairs], {int(t): int(c) for t, c in pairs}


def probe_lists(p):
    """The distinct lists of a probe in first-occurrence order along the read, with the number of positions that carry each."""
    order, mult = [], {}
    for pos, l in sorted(zip(p.positions, p.lists)):
        key = tuple(l)
        if key not in mult:
            order.append(key)
            mult[key] = 0
        mult[key] += 1
    neg = getattr(p, "neg", ())
    return [(list(k), mult[k], tuple(sorted(k)) in neg) for k in order]


def check_against_trace(tax, p, line, stride=True):
    """Model against the oracle's trace of the probe's read -> the model's result (asserts equality unless the closure overflows)."""
    reg, cnt = parse_trace(line)
    lists = probe_lists(p)
    kept = {t for ids, _, _ in lists for t in ids}
    reg1 = reg[:len(kept)]
    assert set(reg1) == kept, (p.name, reg1, kept)
    m = closure(tax, lists, reg1, stride)
    if not m["overflow"]:
        assert m["reg"] == reg, (p.name, m["reg"], reg)
        assert m["cnt"] == cnt, (p.name, m["cnt"], cnt)
    return m


# ---- the designed reads -----------------------------------------------------------------------------------------------------------------
LADDERS = (1, 7, 8, 9, 16, 17, 32, 33)   # chain lengths: the leaves of ladder L have L ancestors
FAN = 12                                  # leaves at the foot of every ladder
SEED = 7401


def make_tax():
    """The 16-bit probe tree (capacity_probes.BRANCHING16) and, beside it, a ladder per chain length of LADDERS: a line of L - 1 nodes
    below the root that ends in FAN leaves, so a leaf has exactly L ancestors.  The ladders' nodes have no rank (every kept one is
    eligible) and ids below the tree's (100 ..), so a ladder leaf sorts before any strain while it is shallower or deeper than it."""
    from lmat_amd import synth
    tax = synth.make_taxonomy(cp.BRANCHING16, specials=False)
    nxt = [100]
    leaves = {}
    for L in LADDERS:
        par = 1
        for _ in range(L - 1):
            tax.add(nxt[0], par, "no_rank", "ladder%d_%d" % (L, nxt[0]))
            par = nxt[0]
            nxt[0] += 1
        leaves[L] = []
        for _ in range(FAN):
            tax.add(nxt[0], par, "no_rank", "leaf%d_%d" % (L, nxt[0]))
            leaves[L].append(nxt[0])
            nxt[0] += 1
    assert nxt[0] < 1000
    for L in LADDERS:
        assert all(len(tax.path(t)) == L for t in leaves[L])
    return renumber16(tax), leaves


# name -> (taken by the fixed-stride walk, or None where the read never gets there; class the read ends in)
EXPECT = {}


def build_set(outdir, seed=SEED):
    """-> the dict of capacity_probes.build_set ("tax", "probes", file paths) plus "leaves"; EXPECT says what each read must do."""
    import oracle_py
    from lmat_amd import synth
    tax, leaves = make_tax()
    paths = synth.write_aux_files(outdir, tax)
    orc = oracle_py.Oracle(paths["tree"], paths["depth"], paths["rank"], paths["idmap"])
    b = cp._Builder(tax, orc, False, seed)
    st = b.strains
    per_sp, per_genus, per_fam = 8, 32, 128
    reps = [st[i * per_fam] for i in range(12)]   # strains of different families: chains of 6 that share little

    def add(name, lists, taken, ends="fast", positions=None):
        p = b.add(name, "stride", 0, lists, positions=positions)
        EXPECT[name] = (taken, ends)
        return p

    try:
        # walked chains at stride 8: 2, 3, 8 taken, 9 falls back (chains of 6 from different families, and the ladder of 7)
        for n in (2, 3, 8, 9):
            add("fam%d" % n, [reps[:n], reps[:1], reps[:1]], n * 8 <= 64)
            add("lad7x%d" % n, [leaves[7][:n], leaves[7][:1]], n * 8 <= 64)
        # the longest chain: 1, 7, 8 | 9, 16 (stride 16) | 17, 32 (stride 32) | 33 falls back; beside it chains on either side of nch * S = 64
        add("lad1x2", [leaves[1][:2]], True)
        add("lad1x12", [leaves[1][:12], leaves[1][3:5]], True)
        add("lad8x8", [leaves[8][:8], leaves[8][:2]], True)          # 8 * 8 == 64
        add("lad8x9", [leaves[8][:9], leaves[8][:2]], False)
        add("lad9x4", [leaves[9][:4], leaves[9][1:2]], True)         # 4 * 16 == 64
        add("lad9x5", [leaves[9][:5], leaves[9][1:2]], False)
        add("lad16x4", [leaves[16][:4], leaves[16][2:4]], True)
        add("lad16x5", [leaves[16][:5]], False)
        add("lad17x2", [leaves[17][:2], leaves[17][1:2]], True)      # 2 * 32 == 64
        add("lad17x3", [leaves[17][:3]], False)
        add("lad32x2", [leaves[32][:2], leaves[32][:1]], True)       # slots beyond 31: the high halves of the masks
        add("lad32x3", [leaves[32][:3]], False)
        add("lad33x2", [leaves[33][:2], leaves[33][:1]], False)
        add("lad1_lad17", [leaves[1][:1] + leaves[17][:1], leaves[17][:1]], True)   # chains of 1 and 17 side by side at stride 32
        add("lad7_fam", [leaves[7][:3] + reps[:5], reps[1:3], leaves[7][2:3]], True)  # 8 chains, more than 32 slots at stride 8
        # 64 and 65 elements: 16 lists of four strains of two species (two walked chains)
        pool = st[:per_sp] + st[per_sp:2 * per_sp]
        import itertools
        combos = [list(c) for c in itertools.combinations(pool[:7] + pool[8:10], 4)]
        add("nel64", combos[:16], True)
        add("nel65", combos[:15] + [pool[:5]], False)
        # the closure brings the table to exactly 64 slots, and past them (capacity_probes' T probes: one list of strains)
        ids = cp.strains_for_T(tax, st[2 * per_genus:], 64)
        add("T64", [ids], True)
        ids = cp.strains_for_T(tax, st[3 * per_genus:], 65)
        add("T65", [ids], True, ends="middle")
        # a kept id above another kept id: a genus on its own positions, a strain below it elsewhere, a second strain for a second chain
        genus = tax.parent[tax.parent[st[5 * per_genus]]]
        add("kept_above", [[genus], [st[5 * per_genus], st[7 * per_genus]], [genus], [st[5 * per_genus]]], True)
        fam = tax.parent[genus]
        add("kept_above2", [[st[5 * per_fam], fam], [genus, st[9 * per_genus]], [st[5 * per_genus + 1]]], True)
        # element order against slot order: a shallow ladder leaf (small id: first element) beside a strain (deeper: registered first)
        add("reversed", [[leaves[7][4], st[11 * per_genus]], [st[11 * per_genus]]], True)
        add("reversed2", [[leaves[1][5], leaves[16][6], st[12 * per_genus]]], True)
        # sibling strains of one species tied, and strains of two species: only the representatives walk
        add("species2", [st[13 * per_genus:13 * per_genus + 3] + st[13 * per_genus + per_sp:13 * per_genus + per_sp + 2],
                         st[13 * per_genus + 1:13 * per_genus + 2]], True)
        # a negative-first list among the others: a raw list of 32768 entries (its two strains and, 32766 times, their common family's
        # parent, which the leaf-most filter drops): its positions keep their ids and take no part in the closure.  One of its
        # strains is eligible through another list, the other nowhere.
        s0, s1, s2 = st[15 * per_genus], st[15 * per_genus + 2 * per_sp], st[17 * per_genus]
        above = [a for a in tax.path(s0) if a in tax.path(s1)][0]
        p = add("negfirst", [[s0, s1], [s0, s2], [s2]], True)
        km = [k for k, l in b.table.items() if sorted(l) == sorted([s0, s1])]
        assert len(km) == 1
        b.table[km[0]] = b.table[km[0]] + [above] * 32766
        p.neg = {tuple(sorted([s0, s1]))}
        # nothing eligible to walk twice: one eligible id (the short closure, never the strided walk)
        add("one_chain", [[st[14 * per_genus], st[14 * per_genus + 1]]], False)
    finally:
        orc.close()
    kmers = np.array(sorted(b.table), dtype=np.uint64)
    paths["db"] = os.path.join(outdir, "stride.bin")
    synth.write_taxhisto(paths["db"], kmers, [b.table[int(km)] for km in kmers.tolist()], cp.K)
    paths.update(tax=tax, probes=b.probes, leaves=leaves)
    return paths
