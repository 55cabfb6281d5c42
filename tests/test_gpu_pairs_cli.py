"""GPU: read_label -i <mates 1> -2 <mates 2> against read_label on the file upstream's bin/merge_fastq_reads_with_N_separator.pl
would write of the two: per pair one record under mate 1's header, sequence mate1 + "N" + mate2, quality q1 + "#" + q2.  The merged
file is written here from that rule; the .out shards, the .fastsummary and the .nomatchsum of the two runs are the same bytes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "read_label")
OUTPUTS = ("0.out", "1.out", ".0.30.fastsummary", ".0.30.nomatchsum")


def _args(ds, out, extra, threads=2):
    return [EXE, "-f", ds["idmap"], "-u", ds["names"], "-w", ds["rank"], "-x", "0", "-j", "30", "-l", "0", "-b", "1.0",
            "-e", ds["depth"], "-t", str(threads), "-d", ds["db"], "-c", ds["tree"], "-o", out, *extra]


def _run(ds, out, extra, env=None, threads=2):
    r = subprocess.run(_args(ds, out, extra, threads), capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr + r.stdout
    return {s: open(out + s, "rb").read() for s in OUTPUTS if threads > 1 or s != "1.out"}


@pytest.fixture(scope="module")
def files(small_dataset, tmp_path_factory):
    """About 300 pairs cut from fixture reads (they hit the database; some carry lower case), mates of many lengths, a few pairs
    with an N inside a mate: two 4-line FASTQ files, two FASTA files, and the merged file of each kind."""
    d = tmp_path_factory.mktemp("pairs_cli")
    src = [r for r in small_dataset["reads"] if len(r) >= 150]
    pairs = []
    for i in range(300):
        r = src[i % len(src)]
        m1, m2 = (r[:75], r[75:150]) if i % 4 == 0 else (r[:35 + (i * 13) % 66], r[150 - 30 - (i * 7) % 71:150])
        if i % 29 == 3:
            m1 = m1[:20] + "N" + m1[21:]
        pairs.append(("pair%d/1 of %d" % (i, len(m1)), m1, "pair%d/2" % i, m2))
    q = lambda s, c: c * len(s)
    p = {k: str(d / k) for k in ("a.fq", "b.fq", "merged.fq", "a.fa", "b.fa", "merged.fa", "b299.fq")}
    with open(p["a.fq"], "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (h1, m1, q(m1, "I")) for h1, m1, _, _ in pairs))
    with open(p["b.fq"], "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (h2, m2, q(m2, "5")) for _, _, h2, m2 in pairs))
    with open(p["b299.fq"], "w") as f:
        f.write("".join("@%s\n%s\n+\n%s\n" % (h2, m2, q(m2, "5")) for _, _, h2, m2 in pairs[:299]))
    with open(p["merged.fq"], "w") as f:
        f.write("".join("@%s\n%sN%s\n+\n%s#%s\n" % (h1, m1, m2, q(m1, "I"), q(m2, "5")) for h1, m1, _, m2 in pairs))
    with open(p["a.fa"], "w") as f:
        f.write("".join(">%s\n%s\n" % (h1, m1) for h1, m1, _, _ in pairs))
    with open(p["b.fa"], "w") as f:
        f.write("".join(">%s\n%s\n" % (h2, m2) for _, _, h2, m2 in pairs))
    with open(p["merged.fa"], "w") as f:
        f.write("".join(">%s\n%sN%s\n" % (h1, m1, m2) for h1, m1, _, m2 in pairs))
    p["pairs"] = pairs
    return p


@pytest.mark.parametrize("mode", ["-p", "-p -a", "plain", "pieces"])
def test_two_fastq_files_equal_the_merged_file(small_dataset, files, tmp_path, mode):
    """Two output shards; with pieces of 700 bytes one: a shard holds a contiguous block of every BATCH, and the merged file is then
    cut into many batches where the two files make one, so only the single shard is the same file by construction."""
    threads = 1 if mode == "pieces" else 2
    flags = {"-p": ["-p"], "-p -a": ["-p", "-a"], "plain": [], "pieces": ["-p"]}[mode]
    env = {"LMAT_FASTA_PIECE": "700"} if mode == "pieces" else {}
    two = _run(small_dataset, str(tmp_path / "two"), ["-q", "-i", files["a.fq"], "-2", files["b.fq"]] + flags, env, threads)
    one = _run(small_dataset, str(tmp_path / "one"), ["-q", "-i", files["merged.fq"]] + flags, env, threads)
    assert set(two) == set(one) and len(two) == 2 + threads
    for s in two:
        assert two[s] == one[s], s
    lines = (two["0.out"] + two.get("1.out", b"")).decode().splitlines()
    assert len(lines) == 300 and len(two[".0.30.fastsummary"]) > 0
    h1, m1, _, m2 = files["pairs"][0]
    # (FASTQ records carry the header of the record before them, the first one none: the reader's pairing, as for one file)
    assert lines[0].split("\t")[:2] == ["unknown_hdr:1", "X" if "-a" in flags else m1 + "N" + m2] and lines[1].split("\t")[0] == h1
    assert sum("DirectMatch" in l or "MultiMatch" in l for l in lines) > 150                # the pairs do hit


def test_many_paired_batches_into_two_shards(small_dataset, files, tmp_path):
    """Pieces of 700 bytes and two shards: the paired run closes a batch after about a piece of bases, so it makes dozens of them,
    and a shard holds a contiguous block of every batch.  The merged file is cut elsewhere, so the shard files of the two runs
    need not coincide; the records they hold between them, and both summaries, must.  That the paired run did make many batches
    shows in its shards: one batch would put the first 150 pairs into shard 0 and the rest into shard 1."""
    env = {"LMAT_FASTA_PIECE": "700"}
    two = _run(small_dataset, str(tmp_path / "two"), ["-q", "-p", "-i", files["a.fq"], "-2", files["b.fq"]], env)
    one = _run(small_dataset, str(tmp_path / "one"), ["-q", "-p", "-i", files["merged.fq"]], env)
    whole = _run(small_dataset, str(tmp_path / "whole"), ["-q", "-p", "-i", files["a.fq"], "-2", files["b.fq"]])
    lines = lambda r: sorted((r["0.out"] + r["1.out"]).splitlines())
    assert lines(two) == lines(one) == lines(whole) and len(lines(two)) == 300
    for s in OUTPUTS[2:]:
        assert two[s] == one[s] == whole[s], s
    # (a record carries the header of the pair before it: "pair<i>/1 of <l1>")
    index = lambda shard: [int(l.split(b"/")[0][4:]) for l in shard.splitlines() if l.startswith(b"pair")]
    first, second = index(two["0.out"]), index(two["1.out"])
    assert max(index(whole["0.out"])) < min(index(whole["1.out"]))            # one batch: a block each
    switches = sum(a > b for a, b in zip(first, first[1:])) + sum(a > b for a, b in zip(second, second[1:]))
    assert switches == 0 and len(first) + len(second) == 299                   # input order inside a shard
    runs = 1 + sum(b != a + 1 for a, b in zip(first, first[1:]))
    assert runs > 20, runs                                                      # shard 0 is made of the blocks of more than 20 batches


def test_two_fasta_files_equal_the_merged_file(small_dataset, files, tmp_path):
    two = _run(small_dataset, str(tmp_path / "two"), ["-p", "-i", files["a.fa"], "-2", files["b.fa"]])
    one = _run(small_dataset, str(tmp_path / "one"), ["-p", "-i", files["merged.fa"]])
    for s in OUTPUTS:
        assert two[s] == one[s], s
    assert two["0.out"].count(b"\n") + two["1.out"].count(b"\n") == 300


def test_files_of_different_read_counts_end_the_run(small_dataset, files, tmp_path):
    r = subprocess.run(_args(small_dataset, str(tmp_path / "x"), ["-q", "-p", "-i", files["a.fq"], "-2", files["b299.fq"]]), capture_output=True, text=True)
    assert r.returncode != 0 and "must hold the same number of reads" in r.stderr and "holds more reads than" in r.stderr
    r = subprocess.run(_args(small_dataset, str(tmp_path / "y"), ["-q", "-p", "-i", files["b299.fq"], "-2", files["a.fq"]]), capture_output=True, text=True)
    assert r.returncode != 0 and "must hold the same number of reads" in r.stderr


def test_pairs_from_standard_input_are_a_usage_error(small_dataset, files, tmp_path):
    r = subprocess.run(_args(small_dataset, str(tmp_path / "x"), ["-q", "-i", "-", "-2", files["b.fq"]]), capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and "-2" in r.stderr and "not with -i -" in r.stderr and "Taxonomic classification module usage" in r.stdout
    assert not os.path.exists(str(tmp_path / "x") + "0.out")
