"""CPU: the contract of the per-group k-mer coverage (tests/kcov_model.py) against the reference's own content_summ reports of the
example run (tests/golden/example_tree.json), and the -G / LMAT_CS_GPU switch of the content_summ tool where there is no GPU.

The inputs are rebuilt as tests/test_content_summ.py rebuilds them (its helper, copied): the eight .out files of
tests/golden/example_gene.tar.gz, the run's .fastsummary, the taxonomy tree from the .summ report, the rank table from the ranks the
.fastsummary names.  select_example_reads restates which reads content_summ counts and under which taxid (src/content_summ.cpp:342-351,
376-411): calls that are no 'N...'/'R...' marker and score 0 or more, strains folded into the first species on their path, ranks of -a."""
import json
import os
import subprocess
import tarfile

import kcov_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "content_summ")
K_SIZES = [8, 10, 12, 14, 17]
RANKS = ("plasmid", "species", "genus")


def example_inputs(tmp_path):
    T = json.load(open(os.path.join(G, "example_tree.json")))
    nodes = T["nodes"]
    fastsummary = T["files"][""]
    rank = {}
    for line in fastsummary.splitlines():
        c = line.split("\t")
        rank[int(c[2])] = c[3].split(",", 1)[0].replace(" ", "_")
    parent = {n["tid"]: n["parent"] for n in nodes}
    for n in nodes:
        t = n["tid"]
        if rank.get(t, "no_rank") == "no_rank" and rank.get(parent[t]) == "species":
            rank[t] = "strain"
    children = {}
    for n in nodes:
        if n["parent"] != n["tid"]:
            children.setdefault(n["parent"], []).append(n["tid"])
    lines = ["# taxonomy tree of the example run's content_summ report", "#", str(len(nodes))]
    for n in nodes:
        ch = children.get(n["tid"], [])
        lines += [" ".join(str(x) for x in [n["tid"], len(ch)] + ch + [n["parent"]]), n["name"]]
    (tmp_path / "tax.dat").write_text("\n".join(lines))
    (tmp_path / "ranks.txt").write_text("".join(f"{n['tid']} {rank.get(n['tid'], 'no_rank')}\n" for n in nodes))
    (tmp_path / "run.fastsummary").write_text(fastsummary)
    tar = tarfile.open(os.path.join(G, "example_gene.tar.gz"))
    names = []
    for i in range(8):
        p = tmp_path / f"rl{i}.out"
        p.write_bytes(tar.extractfile(f"rl{i}.out").read())
        names.append(str(p))
    (tmp_path / "rl.flst").write_text("\n".join(names) + "\n")
    return T, rank


def cs_argv(tmp_path, out):
    """the argv of test_content_summ.py's first test (bin/run_cs.sh:148 without the plasmid list)"""
    return [EXE, "-c", str(tmp_path / "tax.dat"), "-l", str(tmp_path / "run.fastsummary"), "-k", ",".join(map(str, K_SIZES)),
            "-f", str(tmp_path / "rl.flst"), "-r", str(tmp_path / "ranks.txt"), "-a", ",".join(RANKS), "-o", out]


def _is_plasmid(t):
    return 10000000 <= t < 11000000


def select_example_reads(tmp_path, T):
    """-> (reads, taxids they are counted under), in file order"""
    parent = {n["tid"]: n["parent"] for n in T["nodes"]}
    rank = dict((int(a), b) for a, b in (l.split() for l in open(tmp_path / "ranks.txt")))
    strain2spec = {}
    for line in T["files"][""].splitlines():
        if "\tNULL\t" in line:
            continue
        tid = int(line.split()[2])
        if rank.get(tid) == "species":
            strain2spec.setdefault(tid, tid)
        if not _is_plasmid(tid):
            t = tid
            while t in parent and parent[t] != t:
                t = parent[t]
                if rank.get(t) == "species":
                    strain2spec.setdefault(tid, t)
    reads, tids = [], []
    for i in range(8):
        for line in open(tmp_path / f"rl{i}.out", "rb").read().split(b"\n"):
            f = line.split(b"\t")
            if len(f) < 5:
                continue
            call = f[4]
            if not call or call[:1] in (b"N", b"R"):
                continue
            tok = call.split()
            taxid = int(tok[0])
            if float(tok[1]) < 0.0:                  # -v, the score threshold: 0 by default
                continue
            use = strain2spec.get(taxid, taxid) if not _is_plasmid(taxid) else taxid
            if rank.get(use, "undef") in RANKS or _is_plasmid(taxid):
                reads.append(f[1])
                tids.append(use)
    return reads, tids


def cov_blocks(text):
    """a _kmer_cov file -> {taxid: its block (header lines and rows of every k) as text}"""
    out = {}
    tid = None
    for line in text.splitlines(keepends=True):
        if line.startswith("taxid="):
            tid = int(line.split()[0][6:])
        out[tid] = out.get(tid, "") + line
    return out


def test_model_reproduces_the_reference_example_reports(tmp_path):
    T, _ = example_inputs(tmp_path)
    reads, tids = select_example_reads(tmp_path, T)
    assert len(reads) > 500 and len(set(tids)) >= 5
    rep, st = km.coverage(reads, tids, K_SIZES)
    assert st["reads"] == len(reads)
    n_blocks = n_rows = 0
    for name, text in T["files"].items():
        if not name.endswith("_kmer_cov"):
            continue
        for tid, block in cov_blocks(text).items():
            assert km.cov_text(rep, K_SIZES, tid) == block, (name, tid)
            n_blocks += 1
            n_rows += block.count("\n")
    assert n_blocks >= 5 and n_rows >= 262          # the species file alone holds 262 lines


def test_model_edges():
    rep, st = km.coverage([b"ACGT", b"acgt", b"ACNGT", b"", b"AC"], [7, 7, 7, 7, 9], [2, 4, 5])
    # k = 2: AC/GT -> AC (1), CG -> CG (6); ACNGT: AC and GT, both AC
    assert rep[0] == {7: (2, 5, [(2, 1), (3, 1)]), 9: (1, 1, [(1, 1)])}
    assert rep[1] == {7: (1, 2, [(2, 1)])}          # ACGT is its own reverse complement
    assert rep[2] == {}
    assert st == {"reads": 5, "bases": 15, "windows": 3 + 3 + 2 + 1 + 1 + 1, "runs": 2 + 1 + 1}


def _run(tmp_path, extra, env_extra, out):
    env = dict(os.environ)
    env.pop("LMAT_CS_GPU", None)
    env.pop("LMAT_LIB", None)
    env.update(env_extra)
    return subprocess.run(cs_argv(tmp_path, out) + extra, capture_output=True, text=True, timeout=120, env=env)


def test_gpu_switch_never_falls_back_to_the_host(tmp_path):
    """Where no HIP device is usable -G and LMAT_CS_GPU=1 end the run, naming the cause; the host path loads no library."""
    import lmat_amd
    T, _ = example_inputs(tmp_path)
    out = str(tmp_path / "run.fastsummary.summ")
    if lmat_amd.load_library().lmat_device_count() == 0:   # with a device the switch works: tests/test_gpu_kcov.py covers it there
        for extra, env in ((["-G"], {}), ([], {"LMAT_CS_GPU": "1"})):
            r = _run(tmp_path, extra, env, out)
            assert r.returncode != 0 and "no usable HIP device" in r.stderr, (r.returncode, r.stderr)
            assert "query time:" not in r.stdout
    r = _run(tmp_path, ["-G"], {"LMAT_LIB": "/nonexistent.so"}, out)
    assert r.returncode != 0 and "/nonexistent.so" in r.stderr, (r.returncode, r.stderr)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".summ") or f.endswith("_kmer_cov")]   # the run ended before any report
    r = _run(tmp_path, [], {"LMAT_LIB": "/nonexistent.so"}, out)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == T["files"][".summ"]
    want = {k: v for k, v in T["files"].items() if k.endswith("_kmer_cov")}
    got = {f[len("run.fastsummary"):]: open(os.path.join(str(tmp_path), f)).read()
           for f in os.listdir(str(tmp_path)) if f.endswith("_kmer_cov")}
    assert got == want
    assert "kmer coverage on device" not in r.stdout
