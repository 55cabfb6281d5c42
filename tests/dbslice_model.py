"""Python model of the taxonomic slice of a database export (lmat_export_set_filter), shared by
test_dbslice_model.py and test_gpu_dbslice.py.  It states the contract of include/lmat_hip.h over dbgen_model.read_taxhisto records
and a dbgen_model.load_tree taxonomy: S is the named nodes with all their descendants, ancestors come from parent walks, an id the
tree does not hold is outside S and has depth 0, and a record failing several tests is charged to the first of taxon, depth, length."""
import struct

from lmat_amd import synth

SHORT_LIST = 8      # dbexport.hip kShortList: longer lists are judged by the whole wave
MODES = ("any", "all", "none")


def in_set(tax, taxa):
    """-> f(taxid): does the taxid lie in S (a named node or one of its descendants)?  Memoised parent walk."""
    S = set(int(t) for t in taxa)
    for t in S:
        if t not in tax.parent:
            raise KeyError("taxid %d is not in the tree" % t)
    memo = {}

    def f(t):
        if t not in tax.parent:
            return False
        walk, x, hit = [], t, False
        while True:
            if x in memo:
                hit = memo[x]
                break
            walk.append(x)
            if x in S:
                hit = True
                break
            if tax.parent[x] == x:
                break
            x = tax.parent[x]
        for w in walk:
            memo[w] = hit
        return hit
    return f


def verdict(lst, inside, depth_of, mode=None, min_lca_depth=0, max_entries=0):
    """-> 0 kept, 1 dropped by the taxon test, 2 by depth, 3 by length"""
    if mode is not None:
        hits = sum(1 for t in lst if inside(t))
        if not {"any": hits > 0, "all": hits == len(lst), "none": hits == 0}[mode]:
            return 1
    if min_lca_depth and min(depth_of(t) for t in lst) < min_lca_depth:
        return 2
    if max_entries and len(lst) > max_entries:
        return 3
    return 0


def slice_records(records, tax, taxa=(), mode=None, min_lca_depth=0, max_entries=0):
    """-> (kept records in order, {taxid: kept lists that hold it}, [scanned, kept, dropped by taxon, by depth, by length, long lists])"""
    if mode is not None and mode not in MODES:
        raise ValueError("mode")
    if (mode is None) != (len(taxa) == 0):
        raise ValueError("a mode needs taxa and taxa need a mode")
    inside = in_set(tax, taxa)
    depth_of = lambda t: tax.depth.get(t, 0)
    on = bool(mode is not None or min_lca_depth or max_entries)
    kept, counts, c = [], {}, [0] * 6
    for km, lst in records:
        c[0] += 1
        c[5] += on and len(lst) > SHORT_LIST      # without a test nothing is judged
        v = verdict(lst, inside, depth_of, mode, min_lca_depth, max_entries)
        if v:
            c[1 + v] += 1
            continue
        c[1] += 1
        kept.append((km, lst))
        for t in lst:
            counts[t] = counts.get(t, 0) + 1
    return kept, counts, c


def file_bytes(k, records):
    """The tax_histo file of the records: header count = len(records), the sanity word behind every 1500th."""
    out = [struct.pack("<IQQIcI", 29, len(records), synth.SANITY, 999, b"N", k)]
    for i, (km, lst) in enumerate(records):
        out.append(struct.pack("<QH%dI" % len(lst), km, len(lst), *lst))
        if (i + 1) % 1500 == 0:
            out.append(struct.pack("<Q", synth.SANITY))
    return b"".join(out)
