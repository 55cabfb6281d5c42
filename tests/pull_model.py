"""The read puller restated in Python: the selection rule of include/lmat_hip.h ("reads pulled by called taxon"; upstream's
bin/pull_reads.pl:76-100 on the printed fields of a record) and the script's writer (file names, header line, 80-column lines).
The tests hold it to the files the script itself wrote (tests/golden/pull/) and the GPU to it."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PULL_DIR = os.path.join(HERE, "golden", "pull")

SUBTREE, REST, LOWSCORE, NODBHITS, NONE = 1, 2, 4, 8, 0xFFFF
ST_CALL, ST_PHIX, ST_SHORT_LEN, ST_SHORT_VALID, ST_NODBHITS, ST_SILENT = range(6)
MATCH_NAMES = ("DirectMatch", "MultiMatch", "PartialMultiMatch", "NoMatch", "LCA_ERROR")


def parse_idfile(path):
    """-> [{"name", "ids", "flags", "low_score"}], one group per non-blank line (pull_reads.pl:36-67)"""
    groups = []
    for line in open(path).read().split("\n"):
        tok = line.split()
        if not tok:
            continue
        g = {"name": tok[0], "ids": [], "flags": 0, "low_score": 0.0}
        if tok[0] == "LowScore" and len(line) > line.index("LowScore") + 8:
            g["flags"] = LOWSCORE
            g["low_score"] = float(tok[1]) if len(tok) > 1 else 0.0
        elif tok[0].startswith("ReadTooShort"):
            g["name"] = "ReadTooShort"
        else:
            if tok[0] == "NoDbHits":
                g["flags"] = NODBHITS
            g["ids"] = [int(t) for t in tok if t.isdigit() and t.isascii() and str(int(t)) == t and int(t) < 2 ** 32]
        groups.append(g)
    return groups


def fields_of_result(r, k, prm_min_kmer):
    """A result record (READ_RESULT_DTYPE element) -> (tid, score float32, third, type) as the .out writer prints them; None: no text"""
    st = int(r["status"])
    if st == ST_SHORT_LEN:
        return int(r["read_len"]), np.float32(k), -1, "ReadTooShort"
    if st == ST_SHORT_VALID:
        return int(r["valid_kmers"]), np.float32(prm_min_kmer), -1, "ReadTooShort"
    if st == ST_NODBHITS:
        return int(r["read_len"]), np.float32(k), int(r["valid_kmers"]), "NoDbHits"
    if st == ST_SILENT:
        return None
    if st == ST_PHIX:
        return int(r["call_tid"]), np.float32(r["call_score"]), int(r["cand_kmer_cnt"]), "DirectMatch"
    mt = int(r["match_type"])
    if mt <= 2:
        return int(r["call_tid"]), np.float32(r["call_score"]), int(r["cand_kmer_cnt"]), MATCH_NAMES[mt]
    return -1, np.float32(-1), int(r["cand_kmer_cnt"]), "NoMatch" if mt == 3 else "Unmatched"


def key_table(groups, parent=None):
    """printed taxid -> group.  Exact ids, the later group overwriting; then, with `parent` (taxid -> parent taxid, the root its own
    parent or absent), every node of the tree no group lists goes to the nearest ancestor owned by a SUBTREE group."""
    exact = {}
    for gi, g in enumerate(groups):
        for t in g["ids"]:
            exact[t] = gi
    table = dict(exact)
    if parent is not None and any(g["flags"] & SUBTREE for g in groups):
        for t in parent:
            if t in exact:
                continue
            a, seen = parent.get(t), 0
            while a is not None and seen < 200:
                if a in exact and groups[exact[a]]["flags"] & SUBTREE:
                    table[t] = exact[a]
                    break
                nxt = parent.get(a)
                a, seen = (None if nxt == a else nxt), seen + 1
    return table


def select(fields, groups, thresh, min_kmer, table=None):
    """The group of every record: fields = [(tid, score, third, type) or None]"""
    table = key_table(groups) if table is None else table
    low = nodb = rest = NONE
    low_score = np.float32(0)
    for gi, g in enumerate(groups):
        if g["flags"] & LOWSCORE:
            low, low_score = gi, np.float32(g["low_score"])
        if g["flags"] & NODBHITS:
            nodb = gi
        if g["flags"] & REST:
            rest = gi
    thresh = np.float32(thresh)
    out = []
    for f in fields:
        g = NONE
        if f is not None:
            tid, score, third, typ = f
            score = np.float32(score)
            enough = third >= min_kmer
            if enough and tid >= 0 and score >= thresh and tid in table:
                g = table[tid]
            elif low != NONE and score < low_score and enough:
                g = low
            elif typ == "NoDbHits" and enough:
                g = nodb
        out.append(rest if g == NONE else g)
    return out


def pulled_files(out_name, idfile_name, groups, group_of, hdrs, reads, texts):
    """The files the script writes for one .out file -> {file name: bytes}.  texts[i] = (tid, score, type, third) as TEXT."""
    stem = "%s.%s.pulled." % (os.path.basename(out_name), os.path.basename(idfile_name))
    files = {stem + g["name"]: [] for g in groups}
    uid = 0
    for i, g in enumerate(group_of):
        if g == NONE:
            continue
        tid, score, typ, third = texts[i]
        s = ">%s;tid=%s;score=%s;mtype=%s;valid_kmers=%s;uid=%d;src=%s\n" % (hdrs[i], tid, score, typ, third, uid, os.path.basename(out_name))
        s += "".join(reads[i][j:j + 80] + "\n" for j in range(0, len(reads[i]), 80))
        files[stem + groups[g]["name"]].append(s)
        uid += 1
    return {k: "".join(v).encode() for k, v in files.items()}


def parse_out(path):
    """A .out file of five-column records -> (hdrs, reads, fields, texts)"""
    hdrs, reads, fields, texts = [], [], [], []
    for line in open(path):
        c = line.rstrip("\n").split("\t")
        assert len(c) == 5, line
        tid, score, typ = c[4].split(" ")
        third = c[2].split(" ")[2]
        hdrs.append(c[0])
        reads.append(c[1])
        fields.append((int(tid), np.float32(score), int(third), typ))
        texts.append((tid, score, typ, third))
    return hdrs, reads, fields, texts


# ---- the reference's example run, as tests/golden holds it
def load_goldens():
    return json.load(gzip.open(os.path.join(PULL_DIR, "pull_goldens.json.gz"), "rt"))


def example_reads():
    """header line (without '>') -> sequence"""
    out, hdr = {}, None
    for line in gzip.open(os.path.join(PULL_DIR, "simple_list.1000.fna.gz"), "rt"):
        line = line.rstrip("\n")
        if line.startswith(">"):
            hdr = line[1:]
            out[hdr] = []
        else:
            out[hdr].append(line)
    return {h: "".join(v) for h, v in out.items()}


def example_shards(gold, run):
    """The records of one example run cut into its shards: [[record of example_records.json]]"""
    recs = json.load(open(os.path.join(HERE, "golden", "example_records.json")))["runs"][run]
    out, at = [], 0
    for n in gold["runs"][run]["shard_sizes"]:
        out.append(recs[at:at + n])
        at += n
    assert at == len(recs)
    return out


def example_fields(rec):
    """A record of example_records.json -> ((tid, score, third, type), the same as text)"""
    tid, score, typ = rec["call"]
    third = rec["stats"][2]
    return (int(tid), np.float32(score), int(third), typ), (tid, score, typ, third)


def result_of_fields(f, k, prm_min_kmer, dtype):
    """The lmat_read_result that prints these fields (k and -j min_kmer: the engine's, printed by NoDbHits / ReadTooShort rows)"""
    tid, score, third, typ = f
    r = np.zeros(1, dtype=dtype)[0]
    if typ == "NoDbHits":
        assert float(score) == k
        r["status"], r["read_len"], r["valid_kmers"] = ST_NODBHITS, tid, third
    elif typ == "ReadTooShort":
        assert third == -1 and float(score) in (k, prm_min_kmer)
        if float(score) == k:
            r["status"], r["read_len"] = ST_SHORT_LEN, tid
        else:
            r["status"], r["valid_kmers"] = ST_SHORT_VALID, tid
    elif typ in MATCH_NAMES[:3]:
        r["status"], r["match_type"], r["call_tid"], r["call_score"], r["cand_kmer_cnt"] = ST_CALL, MATCH_NAMES.index(typ), tid, score, third
    else:
        assert tid == -1 and typ == "NoMatch"
        r["status"], r["match_type"], r["cand_kmer_cnt"] = ST_CALL, 3, third
    return r


def near_threshold(scores, thresholds, rel=1e-5):
    """The scores that lie within rel (relative) of a threshold: there the script's compare of the 6-digit text and the compare of
    the float could differ"""
    bad = []
    for s in scores:
        for t in thresholds:
            if abs(float(s) - float(t)) <= rel * max(abs(float(t)), abs(float(s))):
                bad.append((float(s), float(t)))
    return bad
