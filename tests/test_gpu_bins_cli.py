"""GPU: read_label -B <id file> -S <min score> -K <min k-mers> -O <dir> on the fixture FASTA with two shards.  The pulled files
are what the script's writer (tests/pull_model.py, held to bin/pull_reads.pl's own files by test_pull_model.py) makes of the same
run's <o>N.out; a run with -a, which echoes no read, pulls the same bytes; a run without -B writes no pulled file and the same
.out files."""
import os
import subprocess

import pytest

import pull_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "read_label")
THRESH, LOW, MIN_KMER = "0.4173", "0.2031", "30"


def _run(ds, out, extra):
    args = [EXE, "-f", ds["idmap"], "-u", ds["names"], "-w", ds["rank"], "-x", "0", "-j", "30", "-l", "0", "-b", "1.0", "-p",
            "-e", ds["depth"], "-t", "2", "-d", ds["db"], "-c", ds["tree"], "-i", ds["fasta"], "-o", out, *extra]
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    return [open(out + "%d.out" % t, "rb").read() for t in range(2)]


def _pulled(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if ".pulled." in f}


def test_pulled_files_of_a_run(small_dataset, tmp_path):
    ds = small_dataset
    dirs = {k: tmp_path / k for k in ("plain", "pull", "quiet", "elsewhere")}
    for d in dirs.values():
        d.mkdir()
    plain = _run(ds, str(dirs["plain"] / "rl"), [])
    assert not _pulled(str(dirs["plain"]))
    # groups from what the run called: the two most frequent taxids in one group, the third in another
    calls = {}
    for t in range(2):
        for f in pm.parse_out(str(dirs["plain"] / ("rl%d.out" % t)))[2]:
            if f[0] > 0 and f[3] in pm.MATCH_NAMES[:3] and float(f[1]) >= float(THRESH):
                calls[f[0]] = calls.get(f[0], 0) + 1
    top = sorted(calls, key=lambda t: (-calls[t], t))[:3]
    assert len(top) == 3
    ids = tmp_path / "ids.txt"
    ids.write_text("%d %d\n%d\nLowScore %s\nNoDbHits\nReadTooShort\n" % (top[0], top[1], top[2], LOW))
    groups = pm.parse_idfile(str(ids))
    flags = ["-B", str(ids), "-S", THRESH, "-K", MIN_KMER]

    with_b = _run(ds, str(dirs["pull"] / "rl"), flags)
    assert with_b == plain                                               # the .out files do not change
    got = _pulled(str(dirs["pull"]))
    want = {}
    n_pulled = 0
    for t in range(2):
        out_fn = str(dirs["pull"] / ("rl%d.out" % t))
        hdrs, reads, fields, texts = pm.parse_out(out_fn)
        assert not pm.near_threshold({f[1] for f in fields}, [THRESH, LOW])
        group_of = pm.select(fields, groups, float(THRESH), int(MIN_KMER))
        n_pulled += sum(g != pm.NONE for g in group_of)
        want.update(pm.pulled_files(out_fn, str(ids), groups, group_of, hdrs, reads, texts))
    assert len(want) == 10 and n_pulled > 0
    assert set(got) == set(want)
    for f in want:
        assert got[f] == want[f], f
    assert sum(len(v) > 0 for v in got.values()) >= 6 and all(len(got[f]) == 0 for f in got if f.endswith("ReadTooShort"))

    # -a: the records echo no read ("X"); the pulled files are the same bytes.  -O: they go elsewhere
    quiet = _run(ds, str(dirs["quiet"] / "rl"), flags + ["-a", "-O", str(dirs["elsewhere"])])
    assert all(l.split(b"\t")[1] == b"X" for s in quiet for l in s.splitlines())
    assert not _pulled(str(dirs["quiet"]))
    assert _pulled(str(dirs["elsewhere"])) == got
