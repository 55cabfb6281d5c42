"""The contract of the per-group k-mer coverage (lmat_cov_*) as plain Python.

Input: reads (bytes, any length) with a 32-bit group id each, and k sizes in 1..31 (duplicates allowed, reported per index).
Per read and k: every window of k consecutive ACGTacgt bytes gives min(forward, reverse complement) over A=0 C=1 G=2 T=3; any
other byte, and the read's end, breaks the run; the SET of the read's canonical k-mers is what counts.
Per group and k: multiplicity of a k-mer = number of reads of the group whose set holds it; reported are distinct (number of
k-mers), total (sum of multiplicities) and the histogram multiplicity -> number of k-mers, ascending.  A group without a k-mer
for a k is absent from that k's report."""
from collections import Counter

CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def read_kmers(read: bytes, k: int):
    """-> (set of canonical k-mers, number of valid windows)"""
    mask = (1 << (2 * k)) - 1
    high = 2 * (k - 1)
    fwd = rev = run = 0
    out = set()
    windows = 0
    for c in read:
        t = CODE.get(c)
        if t is None:
            run = 0
            continue
        fwd = ((fwd << 2) | t) & mask
        rev = ((t ^ 3) << high) | (rev >> 2)
        run += 1
        if run >= k:
            out.add(min(fwd, rev))
            windows += 1
    return out, windows


def coverage(reads, groups, k_sizes):
    """-> ({k_index: {group: (distinct, total, [(multiplicity, n_kmers), ...])}}, {"reads", "bases", "windows", "runs"})"""
    rep = {}
    windows = runs = 0
    for ki, k in enumerate(k_sizes):
        assert 1 <= k <= 31
        per_group = {}
        for r, g in zip(reads, groups):
            s, w = read_kmers(bytes(r), k)
            windows += w
            if s:
                per_group.setdefault(int(g), Counter()).update(s)
        rep[ki] = {}
        for g, cnt in per_group.items():
            hist = Counter(cnt.values())
            rep[ki][g] = (len(cnt), sum(cnt.values()), sorted(hist.items()))
            runs += len(cnt)
    return rep, {"reads": len(reads), "bases": sum(len(r) for r in reads), "windows": windows, "runs": runs}


def cov_text(rep, k_sizes, group):
    """The block content_summ's comp_kmer_cov writes for one taxid: header line and histogram rows per k (src/content_summ.cpp:538-571).
    tot_kmer_cnt goes through an int there."""
    out = []
    for ki, k in enumerate(k_sizes):
        d, t, hist = rep[ki].get(group, (0, 0, []))
        t32 = (t + 2 ** 31) % 2 ** 32 - 2 ** 31
        out.append(f"taxid={group} distinct_kmer_cnt={d} k_size={k} tot_kmer_cnt={t32}\n")
        out += [f"{group} {k} {m} {n}\n" for m, n in hist]
    return "".join(out)
