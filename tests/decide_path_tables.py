"""Tables for the closed form of the decision step for one DOMINANT lineage (kernels.hip k4_wave_path), and a
host model of that form: what test_gpu_decide_path.py runs on the GPU and test_decide_path_model.py checks against the CPU oracle.

A table is built in the space of a pool of taxonomy nodes (test_gpu_decide_chain._Pool: closed under "parent of"): v with count
c0, every ancestor of v ("the path") with c0 or more, other ids that are neither above nor below v with less than c0.  The kept
slots (v and the ids the lists would have kept) come first in a drawn order, the ids a closure would have registered behind them."""
import numpy as np

CANDS = (1, 30, 131, 999)
F = np.float32


class Tables:
    """tids / cnts (flat), off, cand, shape (kept << 8 | 1 << 17) as the debug entry takes them, and what the model needs:
    ix [n, 64] pool indices by slot (-1 behind nT), cn [n, 64] counts by slot, v [n] pool index of the dominant id, pc [n, M] counts in pool space."""

    def __init__(self, pool, ix, cn, v, kept, cand, pc):
        self.pool, self.ix, self.cn, self.v, self.kept, self.pc = pool, ix, cn, v, kept, pc
        valid = ix >= 0
        self.nT = valid.sum(1)
        self.off = np.zeros(ix.shape[0] + 1, dtype=np.uint64)
        np.cumsum(self.nT, out=self.off[1:])
        self.tids = pool.tids[ix[valid]].astype(np.uint32)
        self.cnts = cn[valid].astype(np.uint32)
        self.cand = cand.astype(np.uint32)
        self.shape = ((kept.astype(np.uint32) << 8) | np.uint32(1 << 17)).astype(np.uint32)

    def __len__(self):
        return self.ix.shape[0]

    def args(self):
        return self.tids, self.cnts, self.off, self.cand


def build(pool, n, seed, family, extras=True, cands=CANDS, brk=None, v_from=None):
    """n tables of one family:
      "sib"      v, its path, 0 .. 6 other ids from below v's parent or grandparent (sibling strains, cousins);
      "stranger" the same plus ONE id from anywhere off v's lineage with its private chain; the ancestors it shares with v get c0 + cx;
      "two"      ... plus two such ids (their LCAs with v differ as drawn);
      "genus"    v below a genus, one representative below each other child of that genus, every count added to the shared ancestors;
      "wide"     others from anywhere, up to nT = 64 exactly;
      "pair"     nT = 2: v at depth 1 and the root.
    extras=False: every path count is c0 (no count is added to the shared ancestors).
    brk (one broken condition): "eq_kept" a kept other at c0, "eq_anc" an other behind the kept slots at c0, "ch_below" a path count of
    c0 - 1, "desc" an other id below v."""
    rng = np.random.default_rng(seed)
    M = pool.tids.size
    ar = np.arange(n)
    anc = pool.anc
    depth = pool.depth
    has_desc = anc.any(0)
    if family == "pair":
        start = np.nonzero(depth == 1)[0]
    elif family == "genus":
        # nodes whose parent has at least two children in the pool, at depth >= 2
        par = pool.chain[:, 0]
        nkids = np.bincount(par[par >= 0], minlength=M)
        start = np.nonzero((depth >= 2) & (nkids[np.maximum(par, 0)] >= 2))[0]
    else:
        start = np.nonzero(depth >= 1)[0]
    if brk == "desc":
        start = start[has_desc[start]]
    if v_from is not None:
        start = np.intersect1d(start, v_from)
    v = start[rng.integers(0, start.size, n)]
    clen = depth[v]
    cand = np.array(cands)[rng.integers(0, len(cands), n)]
    pick = rng.integers(0, 6, n)
    c0 = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4], [1, 2, 3, 4, np.maximum(cand // 2, 1)], np.maximum(cand - 1, 1))
    c0 = np.clip(c0, 1, cand)
    path = anc[v]                                   # [n, M] the proper ancestors of v
    unrel = ~pool.rel[v]
    oth = np.zeros((n, M), dtype=bool)              # the kept others
    oc = np.zeros((n, M), dtype=np.int64)           # ... and their counts
    closure = np.zeros(n, dtype=bool)               # their ancestors are registered too, with their counts added

    def draw(ok, want):
        """want[i] ids of ok[i] per table -> mask"""
        key = np.where(ok, rng.random((n, M)), 2.0)
        rank = np.argsort(np.argsort(key, axis=1), axis=1)
        return ok & (rank < want[:, None])

    def below_c0(shape_):
        lv = rng.integers(1, 5, shape_)
        c = (rng.integers(0, 1 << 30, shape_) % lv) * np.maximum(c0 - 1, 1)[:, None] // lv + rng.integers(0, 2, shape_)
        c = np.where(rng.random(shape_) < 0.5, rng.integers(0, 1 << 30, shape_) % np.maximum(c0, 1)[:, None], c)
        return np.minimum(c, (c0 - 1)[:, None])

    if family in ("sib", "stranger", "two"):
        up = pool.chain[v, np.minimum(rng.integers(0, 2, n), clen - 1)]
        near = unrel & anc[:, up].T
        oth |= draw(near, rng.integers(0, 7, n))
    if family in ("stranger", "two"):
        oth |= draw(unrel & (depth >= 1)[None, :] & ~oth, np.full(n, 1 if family == "stranger" else 2))
        closure[:] = True
    if family == "genus":
        g = pool.chain[v, 0]                                                      # v's parent: the "genus" of the block
        # one representative below each other child of g: the child itself or a node below it, as drawn
        idx = np.arange(M)[None, :]
        up_to_kid = depth[None, :] - depth[g][:, None] - 2                        # steps from a node up to its ancestor among g's children
        kid = np.where(up_to_kid >= 0, pool.chain[idx, np.clip(up_to_kid, 0, pool.chain.shape[1] - 1)], idx)
        under = anc[:, g].T & unrel                                               # below g, off v's lineage
        order = np.argsort(np.where(under, kid + rng.random((n, M)) / 2.0, 1e9), axis=1)   # by child, a drawn member of each first
        sk = np.take_along_axis(np.where(under, kid, -1), order, axis=1)
        first = sk >= 0
        first[:, 1:] &= sk[:, 1:] != sk[:, :-1]
        rows, cols = np.nonzero(first)
        oth[rows, order[rows, cols]] = True
        closure[:] = True
    if family == "wide":
        room = 63 - clen - (1 if brk == "desc" else 0)
        want = np.where(rng.random(n) < 0.3, room, rng.integers(0, 64, n))
        oth |= draw(unrel, np.minimum(want, room))
    oc = np.where(oth, below_c0((n, M)), 0)
    if brk == "desc":
        below = draw(anc[:, v].T, np.ones(n, dtype=np.int64))
        oth |= below
        oc = np.where(below, np.maximum(c0 - 1, 0)[:, None], oc)
    present = path | oth
    present[ar, v] = True
    pc = np.where(path, c0[:, None], 0) + np.where(oth, oc, 0)
    pc[ar, v] = c0
    if closure.any():
        ocf = np.where(oth & closure[:, None], oc, 0).astype(np.float64)
        add = (ocf @ anc.astype(np.float64)).astype(np.int64)                 # every ancestor of an other id receives that id's count
        reg = (np.where(oth & closure[:, None], 1.0, 0.0) @ anc.astype(np.float64)) > 0
        present |= reg
        pc = pc + (add if extras else np.where(path, 0, add))
    elif extras:
        pc = pc + np.where(path & (rng.random((n, M)) < 0.4), rng.integers(0, 1 << 30, (n, M)) % (cand - c0 + 1)[:, None], 0)
    # the shape: others below c0, the path from c0 to cand
    pc = np.where(path, np.minimum(pc, cand[:, None]), pc)
    offp = present & ~path
    offp[ar, v] = False
    pc = np.where(offp, np.minimum(pc, (c0 - 1)[:, None]), pc)
    kept = oth.copy()
    kept[ar, v] = True
    some = offp.any(1)
    if brk == "eq_kept":
        t = draw(oth, np.ones(n, dtype=np.int64))
        pc = np.where(t, c0[:, None], pc)
        some = t.any(1)
    elif brk == "eq_anc":
        t = draw(offp & ~kept, np.ones(n, dtype=np.int64))
        pc = np.where(t, c0[:, None], pc)
        some = t.any(1)
    elif brk == "ch_below":
        t = draw(path, np.ones(n, dtype=np.int64))
        pc = np.where(t, (c0 - 1)[:, None], pc)
        some = np.ones(n, dtype=bool)
    elif brk == "desc":
        some = np.ones(n, dtype=bool)
    # slots: the kept ids in a drawn order, the registered ones behind them in a drawn order; at most 64
    assert (present.sum(1) <= 64).all()
    key = np.where(present, np.where(kept, 0.0, 2.0) + rng.random((n, M)), 9.0)
    order = np.argsort(key, axis=1)[:, :64]
    ix = np.where(np.take_along_axis(present, order, axis=1), order, -1)
    if ix.shape[1] < 64:
        ix = np.concatenate([ix, np.full((n, 64 - ix.shape[1]), -1, dtype=ix.dtype)], axis=1)
    cn = np.where(ix >= 0, np.take_along_axis(pc, np.maximum(ix, 0), axis=1), 0)
    t = Tables(pool, ix, cn, v, kept.sum(1), cand, pc)
    t.broken = some
    return t


def stats_f32(cn, valid, cand):
    """scores by slot, log_avg and stdev as the decision step computes them (read_label.cpp:803-880): float32, sums in slot order."""
    sc = np.where(valid, cn.astype(F) / cand.astype(F)[:, None], F(0)).astype(F)
    s = np.zeros(cn.shape[0], dtype=F)
    for t in range(cn.shape[1]):
        s = (s + sc[:, t]).astype(F)
    pos = (valid & (cn > 0)).sum(1)
    nT = valid.sum(1)
    use = np.where(pos > 3, pos, nT)
    avg = (s / use.astype(F)).astype(F)
    dv = (avg[:, None] - sc).astype(F)
    sq = np.where(valid & ((cn > 0) | (pos <= 3)[:, None]), (dv * dv).astype(F), F(0)).astype(F)
    q = np.zeros(cn.shape[0], dtype=F)
    for t in range(cn.shape[1]):
        q = (q + sq[:, t]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.where(use > 1, np.sqrt((q / np.maximum(use - 1, 1).astype(F)).astype(F)).astype(F), F(0)).astype(F)
    return sc, avg, sd


def model(t, sdiff):
    """The closed form on the host -> dict: in_shape (the entry conditions hold), partway (a close id's walk would end the scan
    part-way: the general code's), match (0 Direct, 1 Multi, 4 LCA error), call (pool index, -1 for none), score, log_avg, stdev."""
    pool, ix, cn, v = t.pool, t.ix, t.cn, t.v
    n = ix.shape[0]
    ar = np.arange(n)
    valid = ix >= 0
    jx = np.maximum(ix, 0)
    sc, avg, sd = stats_f32(cn, valid, t.cand.astype(np.int64))
    thr = (sd * F(sdiff)).astype(F)
    is_v = valid & (ix == v[:, None])
    onp = valid & pool.anc[v[:, None], jx]                         # slot holds a proper ancestor of v
    other = valid & ~onp & ~is_v
    c0 = t.pc[ar, v]
    s0 = (c0.astype(F) / t.cand.astype(F)).astype(F)
    in_shape = (~(other & (cn >= c0[:, None]))).all(1) & (~(onp & (cn < c0[:, None]))).all(1) & onp.any(1)
    in_shape &= ~(other & pool.anc[jx, v[:, None]]).any(1)         # no other id below v
    in_shape &= (onp & (pool.depth[jx] == 0)).any(1)
    in_shape &= (np.where(valid & (np.arange(64)[None, :] < t.kept[:, None]), cn * 64 + np.arange(64)[None, :], -1).argmax(1) == is_v.argmax(1))
    close = other & ((s0[:, None] - sc).astype(F) <= thr[:, None])
    partway = np.zeros(n, dtype=bool)
    match = np.where(close.any(1), 4, 0)
    call = np.where(close.any(1), -1, v)
    score = np.where(close.any(1), F(0), s0).astype(F)
    run_max = s0.copy()
    done = ~close.any(1)
    for d in range(pool.chain.shape[1]):                           # the path from v's parent up
        e = pool.chain[v, d]
        have = e >= 0
        ee = np.maximum(e, 0)
        s_e = (t.pc[ar, ee].astype(F) / t.cand.astype(F)).astype(F)
        e_anc_j = pool.anc[jx, ee[:, None]]                        # e is a proper ancestor of the id in slot j
        partway |= have & (close & ~e_anc_j & ((s_e[:, None] - sc).astype(F) > thr[:, None])).any(1)
        run_max = np.where(have, np.maximum(run_max, s_e), run_max).astype(F)
        good = have & ~done & (~close | e_anc_j).all(1)
        match = np.where(good, 1, match)
        call = np.where(good, ee, call)
        score = np.where(good, run_max, score).astype(F)
        done |= good
    return {"in_shape": in_shape, "partway": partway & in_shape, "match": match, "call": call, "score": score, "log_avg": avg, "stdev": sd,
            "sc": sc, "thr": thr, "close": close}
