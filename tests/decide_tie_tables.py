"""Tables for the closed form of the decision step for TIED ids at the top (kernels.hip k4_wave_tie), and a host
model of that form: what test_gpu_decide_tie.py runs on the GPU and test_decide_tie_model.py checks against the CPU oracle.

A table is built in the space of a pool of taxonomy nodes (test_gpu_decide_chain._Pool: closed under "parent of"): two or more ids
of one depth with the largest count c0 ("TOP"), every ancestor of each of them with c0 -- the ones above all of them ("COMMON") with
c0 or more --, other ids below c0.  The kept slots (TOP and the other ids the lists would have kept) come first in a drawn order,
the ids a closure would have registered behind them in a drawn order."""
import numpy as np

import decide_path_tables as dp

CANDS = (1, 30, 131, 999)
F = np.float32
TAKEN = ("root2", "sib2", "sib2low", "sib3", "sib3low", "genus", "genus_stranger", "wide")
BROKEN = ("uneq_depth", "priv_plus", "priv_minus", "gt_outside", "falls", "common_low", "rest_below", "rest_eq", "deepest_kept",
          "deepest_kept_low", "unregistered")


class Tables:
    """tids / cnts (flat), off, cand, shape (kept << 8 | 1 << 17 | 1 << 18) as the debug entry takes them; rows[i] = (pool indices by
    slot, counts by slot, kept) for the model."""

    def __init__(self, pool, rows, cand, bit18=True):
        self.pool, self.rows = pool, rows
        self.nT = np.array([len(r[0]) for r in rows], dtype=np.int64)
        self.off = np.zeros(len(rows) + 1, dtype=np.uint64)
        np.cumsum(self.nT, out=self.off[1:])
        self.tids = pool.tids[np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows])].astype(np.uint32)
        self.cnts = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in rows]).astype(np.uint32)
        self.cand = np.asarray(cand, dtype=np.uint32)
        self.kept = np.array([r[2] for r in rows], dtype=np.uint32)
        self.shape = ((self.kept << 8) | np.uint32((1 << 17) | ((1 << 18) if bit18 else 0))).astype(np.uint32)
        n = len(rows)
        self.cn = np.zeros((n, 64), dtype=np.int64)
        self.valid = np.zeros((n, 64), dtype=bool)
        for i, r in enumerate(rows):
            self.cn[i, :len(r[1])] = r[1]
            self.valid[i, :len(r[1])] = True

    def __len__(self):
        return len(self.rows)

    def args(self):
        return self.tids, self.cnts, self.off, self.cand

    def without_bit18(self):
        return (self.shape & ~np.uint32(1 << 18)).astype(np.uint32)

    def permuted(self, seed):
        """the same tables with the kept slots in another drawn order, and the others in another: whichever tied id std::sort leaves
        first, the call is the same"""
        rng = np.random.default_rng(seed)
        rows = []
        for ix, cn, kept in self.rows:
            p = np.concatenate([rng.permutation(kept), kept + rng.permutation(len(ix) - kept)])
            rows.append(([ix[j] for j in p], [cn[j] for j in p], kept))
        return Tables(self.pool, rows, self.cand)


class _Tree:
    def __init__(self, pool):
        M = pool.tids.size
        self.kids = [[] for _ in range(M)]
        for i in range(M):
            p = int(pool.chain[i, 0])
            if p >= 0:
                self.kids[p].append(i)
        self.ancs = [[int(a) for a in pool.chain[i] if a >= 0] for i in range(M)]   # parent first
        self.desc = [np.nonzero(pool.anc[:, i])[0].tolist() for i in range(M)]


def _tree(pool):
    if not hasattr(pool, "_tie_tree"):
        pool._tie_tree = _Tree(pool)
    return pool._tie_tree


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _one(pool, tr, rng, family, cand, special=None):
    """one table -> (pool indices by slot, counts by slot, kept) or None where the draw does not fit the family"""
    depth = pool.depth
    M = pool.tids.size
    pick = int(rng.integers(0, 6))
    c0 = (1, 2, 3, 4, max(cand // 2, 1), max(cand - 1, 1))[pick]
    c0 = min(max(c0, 1), cand)
    room_up = family in ("genus_stranger", "two", "priv_plus", "gt_outside", "falls")
    if room_up and cand > 1:
        c0 = min(c0, cand - 1)
    if family in ("priv_minus", "common_low", "deepest_kept_low", "genus_stranger", "two", "rest_eq", "gt_outside") and cand > 1:
        c0 = max(c0, 2)
    low = family in ("sib2low", "sib3low")
    ntie = 3 if family in ("sib3", "sib3low") else 2
    top, lower = [], []
    if family == "root2":
        roots = [i for i in range(M) if depth[i] == 0 and len(tr.kids[i]) >= 2]
        if not roots:
            return None
        r = _pick(rng, roots)
        top = [int(x) for x in rng.permutation(tr.kids[r])[:2]]
    elif family in ("genus", "genus_stranger", "priv_plus", "priv_minus"):
        gs = [i for i in range(M) if len(tr.kids[i]) >= 2 and all(len(tr.kids[k]) >= 1 for k in tr.kids[i]) and depth[i] >= 1 and depth[i] == depth.max() - 2
              and all(not tr.kids[s] for k in tr.kids[i] for s in tr.kids[k])]
        if not gs:
            return None
        g = _pick(rng, gs)
        top = [s for k in tr.kids[g] for s in tr.kids[k]]
    elif family == "rest_below":
        ps = [i for i in range(M) if sum(1 for k in tr.kids[i] if tr.kids[k]) >= 2]
        if not ps:
            return None
        p = _pick(rng, ps)
        top = [int(x) for x in rng.permutation([k for k in tr.kids[p] if tr.kids[k]])[:2]]
    else:
        need = ntie + (1 if low else 0)
        ps = [i for i in range(M) if len(tr.kids[i]) >= need and (family != "falls" or depth[i] >= 1)]
        if not ps:
            return None
        p = _pick(rng, ps)
        ks = [int(x) for x in rng.permutation(tr.kids[p])]
        top = ks[:ntie]
        if low:
            lower = ks[ntie:ntie + 1]
    cnt = {}
    for t in top:
        cnt[t] = c0
        for a in tr.ancs[t]:
            cnt[a] = c0
    common = set(tr.ancs[top[0]])
    for t in top[1:]:
        common &= set(tr.ancs[t])
    anyanc = set(a for t in top for a in tr.ancs[t])
    private = anyanc - common
    kept = list(top)

    def below_c0():
        return int(rng.integers(0, c0)) if rng.random() < 0.5 else max(c0 - 1 - int(rng.integers(0, 2)), 0)

    for s in lower:
        cnt[s] = below_c0()
        kept.append(s)
    banned = set(top) | anyanc | set(d for t in top for d in tr.desc[t])

    def stranger(cx, where=None):
        """a kept id off the tied ids' lineages, not below a PRIVATE one, with its chain registered and its count added along it"""
        ok = [i for i in range(M) if i not in banned and i not in cnt and depth[i] >= 1 and not (set(tr.ancs[i]) & private)
              and all(a in common or a not in cnt for a in tr.ancs[i]) and (where is None or where(i))]
        if not ok:
            return None
        j = _pick(rng, ok)
        cnt[j] = cx
        kept.append(j)
        for a in tr.ancs[j]:
            cnt[a] = cnt.get(a, 0) + cx
        return j

    if family in ("genus_stranger", "two", "gt_outside", "rest_eq"):
        cx = int(rng.integers(1, min(c0 - 1, cand - c0) + 1)) if min(c0 - 1, cand - c0) >= 1 else 0
        need_chain = family in ("gt_outside", "rest_eq")
        j = stranger(cx, (lambda i: any(a not in common for a in tr.ancs[i])) if need_chain else None)
        if j is None:
            return None
        if family == "two":
            room = min(c0 - 1, cand - max(cnt.values()))
            if stranger(int(rng.integers(0, room + 1)) if room >= 1 else 0) is None:
                return None
        if need_chain:
            a = _pick(rng, [a for a in tr.ancs[j] if a not in common])
            cnt[a] = c0 + 1 if family == "gt_outside" else c0
            if cnt[a] > cand:
                return None
    if family == "wide":
        ok = [i for i in range(M) if i not in banned and i not in cnt]
        want = 64 - len(cnt)
        if len(ok) < want:
            return None
        for i in rng.permutation(ok)[:want]:
            cnt[int(i)] = below_c0()
            kept.append(int(i))
    if special is not None:
        if special in banned or special in cnt:
            return None
        cnt[special] = below_c0()
        kept.append(special)
    # one broken condition
    if family == "uneq_depth":
        ok = [i for i in range(M) if i not in banned and depth[i] != depth[top[0]] and not (set(tr.ancs[i]) & private)]
        if not ok:
            return None
        j = _pick(rng, ok)
        cnt[j] = c0
        kept.append(j)
        for a in tr.ancs[j]:
            cnt[a] = max(cnt.get(a, 0), c0)
    elif family in ("priv_plus", "priv_minus"):
        a = _pick(rng, sorted(private))
        cnt[a] = c0 + 1 if family == "priv_plus" else c0 - 1
        if cnt[a] > cand or cnt[a] < 0:
            return None
    elif family == "falls":
        deepest = max(common, key=lambda a: depth[a])
        cnt[deepest] = c0 + 1
        if c0 + 1 > cand or len(common) < 2:
            return None
    elif family == "common_low":
        cnt[_pick(rng, sorted(common))] = c0 - 1
    elif family == "rest_below":
        j = _pick(rng, [d for t in top for d in tr.desc[t]])
        cnt[j] = below_c0()
        kept.append(j)
    elif family in ("deepest_kept", "deepest_kept_low"):
        deepest = max(common, key=lambda a: depth[a])
        kept.append(deepest)
        if family == "deepest_kept_low":
            cnt[deepest] = c0 - 1
    elif family == "unregistered":
        a = _pick(rng, sorted(anyanc))
        del cnt[a]
    if len(cnt) > 64 or max(cnt.values()) > cand:
        return None
    kept = [int(kept[j]) for j in rng.permutation(len(kept))]
    ks = set(kept)
    rest = [i for i in cnt if i not in ks]
    rest = [int(rest[j]) for j in rng.permutation(len(rest))]
    if not rest:
        return None
    ix = kept + rest
    return ix, [int(cnt[i]) for i in ix], len(kept)


def build(pool, n, seed, family, cands=CANDS, special=None):
    """n tables of one family.  Taken by construction:
      "root2"           two tied children of a root and the root: nT = 3, the smallest table;
      "sib2" / "sib3"   2 / 3 tied children of one node with their ancestors; "...low": a further child below c0;
      "genus"           every grandchild of a node whose grandchildren are leaves (12 strains under 4 species in the benchmark's
                        taxonomy), the children at c0 (PRIVATE), the node and its ancestors (COMMON);
      "genus_stranger"  the same with a kept id elsewhere, its chain registered, its count cx added along it: the shared ancestors
                        count c0 + cx;
      "wide"            2 tied ids and other ids from anywhere (not below them), nT = 64 exactly.
    "two": two strangers -- a close id's walk may end the scan part-way.  One broken condition each (BROKEN): tied ids of unequal
    depth, a PRIVATE count of c0 + 1 / c0 - 1, a slot above c0 outside COMMON, a COMMON count that falls towards the root / lies below
    c0, an id below a tied id, a registered id at c0 that is no ancestor, the deepest common ancestor among the kept slots (at c0 and
    below it), an ancestor of a tied id without a slot.  special: a pool index added as a kept id below c0 (plasmid / PhiX)."""
    rng = np.random.default_rng(seed)
    tr = _tree(pool)
    rows, cand = [], []
    tries = 0
    while len(rows) < n:
        tries += 1
        assert tries < 50 * n + 1000, (family, len(rows))
        c = int(cands[int(rng.integers(0, len(cands)))])
        if c == 1 and family in ("priv_plus", "priv_minus", "gt_outside", "falls", "common_low", "deepest_kept_low", "rest_eq"):
            continue
        r = _one(pool, tr, rng, family, c, special)
        if r is None:
            continue
        rows.append(r)
        cand.append(c)
    return Tables(pool, rows, cand)


def model(t, sdiff, flagged=None):
    """The closed form on the host -> dict of arrays: in_shape (the entry conditions hold), partway (a close id's walk would end the
    scan part-way: the general code's), match (1 Multi, 4 LCA error), call (pool index, -1 for none), score, stdev, sc [n, 64].
    flagged: pool indices that carry a plasmid or a screened PhiX flag."""
    pool = t.pool
    tr = _tree(pool)
    depth = pool.depth
    n = len(t)
    sc, avg, sd = dp.stats_f32(t.cn, t.valid, t.cand.astype(np.int64))
    thr = (sd * F(sdiff)).astype(F)
    out = {"in_shape": np.zeros(n, dtype=bool), "partway": np.zeros(n, dtype=bool), "match": np.zeros(n, dtype=np.int64),
           "call": np.full(n, -1, dtype=np.int64), "score": np.zeros(n, dtype=F), "log_avg": avg, "stdev": sd, "sc": sc, "thr": thr,
           "gt": np.zeros(n, dtype=bool), "ntop": np.zeros(n, dtype=np.int64)}
    flagged = set(flagged or ())
    for i, (ix, cn, kept) in enumerate(t.rows):
        nT = len(ix)
        if kept < 2 or kept >= nT:
            continue
        c0 = max(cn[:kept])
        top = [s for s in range(kept) if cn[s] == c0]
        if len(top) < 2 or c0 == 0 or len({int(depth[ix[s]]) for s in top}) != 1:
            continue
        slot = {node: s for s, node in enumerate(ix)}
        if any(a not in slot for s in top for a in tr.ancs[ix[s]]):
            continue                                                  # an ancestor of a tied id has no slot
        sets = [set(slot[a] for a in tr.ancs[ix[s]]) for s in top]
        common = set.intersection(*sets)
        anyanc = set.union(*sets)
        private = anyanc - common
        rest = set(range(nT)) - anyanc - set(top)
        gt = {s for s in range(nT) if cn[s] > c0}
        if not common or gt - common or any(cn[s] != c0 for s in private) or any(cn[s] >= c0 for s in rest) or any(cn[s] < c0 for s in common):
            continue
        chain = sorted(common, key=lambda s: -depth[ix[s]])           # deepest first
        if any(cn[chain[k + 1]] < cn[chain[k]] for k in range(len(chain) - 1)):
            continue
        if chain[0] < kept or depth[ix[chain[-1]]] != 0:
            continue
        if any(pool.anc[ix[j], ix[s]] for j in rest for s in top):    # an id below a tied id
            continue
        if any(node in flagged for node in ix) or not thr[i] >= 0:
            continue
        out["in_shape"][i] = True
        out["gt"][i] = bool(gt)
        out["ntop"][i] = len(top)
        s0 = sc[i, top[0]]
        lin = [s for s in chain if s in gt] if gt else chain
        good = list(lin)
        for j in rest:
            if not F(s0 - sc[i, j]) <= thr[i]:
                continue
            anc_j = {s for s in lin if pool.anc[ix[j], ix[s]]}
            if any(F(sc[i, e] - sc[i, j]) > thr[i] for e in lin if e not in anc_j):
                out["partway"][i] = True
            good = [s for s in good if s in anc_j]
        if good:
            out["match"][i], out["call"][i], out["score"][i] = 1, ix[good[0]], sc[i, good[0]]
        else:
            out["match"][i] = 4
    return out
