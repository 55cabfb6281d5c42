"""CPU: the Python restatement of the read puller (tests/pull_model.py) against what the reference's own bin/pull_reads.pl wrote
for its example run (tests/golden/pull/, made by tests/golden/make_pull_goldens.py): on every shard of both runs and under every id
file the (record, group, uid) triples and the bytes of every pulled file.  The .out lines are rebuilt from example_records.json
(records in shard order, cut by the golden's shard sizes) and the example's reads."""
import hashlib
import os

import numpy as np
import pytest

import pull_model as pm

GOLD = pm.load_goldens()
RUNS = sorted(GOLD["runs"])
IDKEYS = sorted(GOLD["idfiles"])


@pytest.fixture(scope="module")
def example():
    reads = pm.example_reads()
    return {run: pm.example_shards(GOLD, run) for run in RUNS}, reads


def _thresholds(key):
    idf = GOLD["idfiles"][key]
    groups = pm.parse_idfile(os.path.join(pm.PULL_DIR, idf["file"]))
    return groups, idf["thresh"], idf["min_kmer"]


def test_goldens_cover_the_issue_cases():
    assert len(RUNS) == 2 and all(len(GOLD["runs"][r]["shard_sizes"]) == 8 for r in RUNS) and len(IDKEYS) >= 3
    first = GOLD["pulls"]["kML+Human.v4-14.20.g10"][0]["a"]
    per = [sum(1 for t in first["triples"] if t[1] == g) for g in ("5476", "9606", "LowScore", "NoDbHits", "ReadTooShort")]
    assert per == [79, 0, 19, 1, 0]
    assert len(first["files"]) == 5                                      # every group's file exists, empty or not
    b = [t for sh in GOLD["pulls"]["kML+Human.v4-14.20.g10"] for t in sh["b"]["triples"]]
    assert {t[1] for t in b} >= {"9606", "777", "LowScore"} and not any(t[1] == "NoDbHits" for t in b)
    assert not any(sh["c"]["triples"] for r in RUNS for sh in GOLD["pulls"][r])


def test_unparsed_records_are_few():
    for run in RUNS:
        n = sum(GOLD["runs"][run]["shard_sizes"])
        assert len(GOLD["runs"][run]["unparsed"]) < 0.01 * n


def test_no_score_lies_at_a_threshold(example):
    """Precondition of every compare below and on the GPU: the script compares the printed 6-digit text, the engine the float."""
    shards, _ = example
    scores = {pm.example_fields(r)[0][1] for run in RUNS for sh in shards[run] for r in sh}
    for key in IDKEYS:
        groups, thresh, _ = _thresholds(key)
        ts = [thresh] + [g["low_score"] for g in groups if g["flags"] & pm.LOWSCORE]
        assert not pm.near_threshold(scores, ts), key


@pytest.mark.parametrize("key", IDKEYS)
@pytest.mark.parametrize("run", RUNS)
def test_model_equals_the_script(example, run, key):
    shards, reads = example
    groups, thresh, min_kmer = _thresholds(key)
    unparsed = {tuple(u) for u in GOLD["runs"][run]["unparsed"]}
    for si, recs in enumerate(shards[run]):
        gold = GOLD["pulls"][run][si][key]
        recs = [r for ri, r in enumerate(recs) if (si, ri) not in unparsed]
        ft = [pm.example_fields(r) for r in recs]
        group_of = pm.select([f for f, _ in ft], groups, thresh, min_kmer)
        triples, uid = [], 0
        for ri, g in enumerate(group_of):
            if g != pm.NONE:
                triples.append([ri, groups[g]["name"], uid])
                uid += 1
        assert triples == gold["triples"], (run, si, key)
        out_name = "%s%d.out" % (GOLD["runs"][run]["prefix"], si)
        files = pm.pulled_files(out_name, GOLD["idfiles"][key]["file"], groups, group_of, [r["hdr"] for r in recs],
                                [reads[r["hdr"]] for r in recs], [t for _, t in ft])
        assert {k: [len(v), hashlib.sha256(v).hexdigest()] for k, v in files.items()} == gold["files"], (run, si, key)


def test_idfile_grammar(tmp_path):
    p = tmp_path / "ids"
    p.write_text("12 0034 x7 12\n\nLowScore 0.25\nLowScore\nReadTooShortish 5\nNoDbHits 99\n4294967296 4294967295\n")
    g = pm.parse_idfile(str(p))
    assert [(x["name"], x["ids"], x["flags"]) for x in g] == [
        ("12", [12, 12], 0), ("LowScore", [], pm.LOWSCORE), ("LowScore", [], 0), ("ReadTooShort", [], 0),
        ("NoDbHits", [99], pm.NODBHITS), ("4294967296", [4294967295], 0)]
    assert g[1]["low_score"] == 0.25


def test_subtree_and_rest_rules():
    parent = {1: 1, 10: 1, 11: 10, 12: 10, 13: 11, 20: 1, 21: 20}
    groups = [{"name": "a", "ids": [10], "flags": pm.SUBTREE, "low_score": 0.0}, {"name": "b", "ids": [11], "flags": 0, "low_score": 0.0},
              {"name": "c", "ids": [20], "flags": 0, "low_score": 0.0}, {"name": "rest", "ids": [], "flags": pm.REST, "low_score": 0.0}]
    table = pm.key_table(groups, parent)
    assert table == {10: 0, 11: 1, 12: 0, 13: 0, 20: 2}                  # 13 passes the exact 11 (no SUBTREE) on its way up to 10
    f = lambda tid: (tid, np.float32(1.0), 50, "DirectMatch")
    got = pm.select([f(13), f(11), f(21), f(20), None, (-1, np.float32(-1), 50, "NoMatch")], groups, 0.5, 30, table)
    assert got == [0, 1, 3, 2, 3, 3]
