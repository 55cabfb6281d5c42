"""GPU: the builders and the way back out at the k the classify sweep runs (test_gpu_k_sweep.py) -- every other builder test is at
k = 8, 18 or 20 and every export test at 9, 16, 18 or 20, all but one even.  Below k = 10 the table the genomes are built into is in
the wide layout, from 10 on in the compact one; k = 5 makes nearly every k-mer one that every genome owns."""
import os

import numpy as np
import pytest

import dbgen_model as dm
import genedb_model as gm
from test_gpu_genedb import CASE1
from test_gpu_genedb import _write_fasta as _write_gene_fasta

pytestmark = pytest.mark.gpu
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
BUILD_K = (5, 9, 11, 17, 19)
GENE_K = (9, 19)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The tree of the builder's goldens, with the depth and rank files an engine's taxonomy wants beside it."""
    d = tmp_path_factory.mktemp("sweep_build")
    p = {"tree": dm.gunzip_to("tree.dat.gz", str(d / "tree.dat")), "depth": str(d / "depth.dat"), "rank": str(d / "rank.txt")}
    tax = dm.load_tree(p["tree"])
    with open(p["depth"], "w") as f:
        f.write("".join(f"{t} {tax.depth[t]}\n" for t in sorted(tax.parent)))
    with open(p["rank"], "w") as f:
        f.write("".join(f"{t} {'strain' if tax.depth[t] == 6 else 'no_rank'}\n" for t in sorted(tax.parent)))
    p["tax"] = tax
    return p


def _records(tax, k):
    """Six 1 kb genomes that share a block; written 70 bases a line the builder's 4096-base chunk ends 96 bases into the fifth: an N
    and two lower-case bases within k - 1 of that edge, and an N somewhere in every genome."""
    rng = np.random.default_rng(70 + k)
    leaves = sorted(t for t in tax.parent if tax.depth[t] == 6)
    shared = LETTERS[rng.integers(0, 4, 300)].tobytes()
    recs = []
    for j in range(6):
        s = bytearray(LETTERS[rng.integers(0, 4, 1000)].tobytes())
        s[100 + 50 * j:400 + 50 * j] = shared
        s[int(rng.integers(0, 1000))] = ord("N")
        if j == 4:
            s[96 - 5] = ord("N")
            for p in (96 + 7, 96 - 12):
                s[p] = ord(chr(s[p]).lower())
        recs.append((leaves[j * 5], bytes(s)))
    return recs


def _write_fasta(path, recs, width=70):
    with open(path, "wb") as f:
        for tid, s in recs:
            f.write(b">%d\n" % tid)
            for j in range(0, len(s), width):
                f.write(s[j:j + width] + b"\n")
    return path


@pytest.mark.parametrize("k", BUILD_K)
def test_build_and_export_at_k(tree, tmp_path, k):
    from lmat_amd import Engine
    tax = tree["tax"]
    recs = _records(tax, k)
    fa = _write_fasta(str(tmp_path / "g.fa"), recs)
    eng = Engine(0)
    try:
        files = {}
        for chunk in (4096, 0):
            for pb in (0, 2):
                out = str(tmp_path / ("o_%d_%d.bin" % (chunk, pb)))
                st = eng.build_taxhisto(fa, tree["tree"], k, out, chunk_bases=chunk, prefix_bits=pb)
                assert st["passes"] == 1 << pb and st["windows"] == st["emitted_pairs"]
                files[(chunk, pb)] = open(out, "rb").read()
        first = files[(4096, 0)]
        for key, data in files.items():
            assert data == first, key
        # the model: records and statistics
        want, dropped = dm.model(recs, tax, k)
        kk, count, got = dm.read_taxhisto(str(tmp_path / "o_4096_0.bin"))
        assert kk == k and count == len(want) and dropped == 0
        assert [km for km, _ in got] == sorted(want)
        for km, lst in got:
            assert lst == want[km], km
        assert st["bases"] == sum(len(s) for _, s in recs)
        assert st["records_written"] == len(want) and st["dropped_unknown"] == 0 and st["distinct_kmers"] == len(want)
        assert st["longest_list"] == max(len(l) for l in want.values())
        assert st["total_list_entries"] == sum(len(l) for l in want.values())
        assert st["singletons"] == sum(1 for l in want.values() if len(l) == 1)
        assert any(len(l) > 6 for l in want.values())              # the shared block: six owners and the nodes up to their LCA
        # straight into the table, and back out: that same file
        eng.load_taxonomy(tree["tree"], tree["depth"], tree["rank"], None)
        st2 = eng.build_db_from_genomes(fa, tree["tree"], k)
        assert eng.k == k and eng.db_size == st2["records_written"] == len(want)
        back = str(tmp_path / "back.bin")
        assert eng.export_taxhisto(back)["records"] == len(want)
        assert open(back, "rb").read() == first
        kms = np.array(sorted(want), dtype=np.uint64)
        counts, tids = eng.lookup(kms, stride=32)
        for i, km in enumerate(kms.tolist()):
            assert counts[i] == len(want[km]) and sorted(tids[i, :counts[i]].tolist()) == want[km], km
    finally:
        eng.close()


@pytest.mark.parametrize("k", GENE_K)
def test_gene_build_at_k(tmp_path, k):
    from lmat_amd import Engine
    want = gm.kmer_ids(CASE1, k)
    assert any(len(v) > 1 for v in want.values())
    out = str(tmp_path / "g.bin")
    eng = Engine(0)
    try:
        st = eng.build_gene_taxhisto(_write_gene_fasta(str(tmp_path / "g.fa"), CASE1, width=17), k, out)
        assert open(out, "rb").read() == gm.to_bytes(want, k)
        assert st["records_written"] == st["distinct_kmers"] == len(want) and st["dropped_unknown"] == 0
        assert st["bases"] == sum(len(s) for _, s in CASE1)
        assert st["total_list_entries"] == sum(len(v) for v in want.values())
        assert st["singletons"] == sum(1 for v in want.values() if len(v) == 1)
        assert st["longest_list"] == max(len(v) for v in want.values())
    finally:
        eng.close()
