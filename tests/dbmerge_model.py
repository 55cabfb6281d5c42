"""Python statement of the merge of tax_histo files (lmat_build_add_taxhisto) and of the per-taxid counts
(countTaxidFrequency), shared by test_dbmerge_model.py and test_gpu_dbmerge.py.  test_dbmerge_model.py holds it against the
reference's own files: the two part files of tests/golden/make_dbmerge_goldens.py merge into the reference's a_k20.bin."""
import gzip
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbmerge")


def gunzip_to(name, dst):
    with gzip.open(os.path.join(GOLD, name), "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    return dst


def lca(tax, a, b):
    while tax.depth[a] > tax.depth[b]:
        a = tax.parent[a]
    while tax.depth[b] > tax.depth[a]:
        b = tax.parent[b]
    while a != b:
        a, b = tax.parent[a], tax.parent[b]
    return a


def merge_lists(tax, lists):
    """The rule for one k-mer: lists = the stored list of every source that holds it -> (sorted result, grown?)."""
    if len(lists) == 1:
        return sorted(lists[0]), False
    x = set()
    for l in lists:
        x.update(l)
    if len(x) == 1:
        return sorted(x), False
    tops = [min(l, key=lambda t: tax.depth[t]) for l in lists]   # a closed list has one shallowest entry: its LCA
    top = tops[0]
    for t in tops[1:]:
        top = lca(tax, top, t)
    out = set(x)
    for t in tops:
        while t != top:
            out.add(t)
            t = tax.parent[t]
    out.add(top)
    return sorted(out), len(out) > len(x)


def merge(tax, sources):
    """sources: [{k-mer: taxid list}] -> ({k-mer: sorted list}, {"records_one_source", "records_merged", "records_grown"})."""
    held = {}
    for src in sources:
        for km, lst in src.items():
            if lst:
                held.setdefault(km, []).append(lst)
    out, st = {}, {"records_one_source": 0, "records_merged": 0, "records_grown": 0}
    for km, lists in held.items():
        out[km], grown = merge_lists(tax, lists)
        st["records_one_source" if len(lists) == 1 else "records_merged"] += 1
        st["records_grown"] += int(grown)
    return out, st


def taxid_counts(result):
    """{taxid: number of records whose list holds it} (countTaxidFrequency.cpp:105-139)."""
    cnt = {}
    for lst in result.values():
        for t in lst:
            cnt[t] = cnt.get(t, 0) + 1
    return cnt


def kcnt_text(cnt):
    return "".join("%d %d\n" % (t, cnt[t]) for t in sorted(cnt))
