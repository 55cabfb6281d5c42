#!/usr/bin/env python3
"""content_summ end to end, host counting against -G (the k-mer coverage on the GPU, lmat_cov_*): wall seconds of both
arms of the same binary on the same synthetic run, their ratio, and the device arm's HIP-event ms per stage.

The run: eight .out files of 150 bp reads drawn with 1 % substitutions from 64 species genomes (so k-mers repeat between reads as they do
in a sample), every read called to its species, with the matching .fastsummary, taxonomy tree and rank table; -k 8,10,12,14,17 as
bin/run_cs.sh passes it.  Sizes: --reads N, or --host-seconds S: a short host-only run finds the N at which the host arm takes about S
(the issue asks for one to two minutes); the device arm is also run alone at ten times that size (--big-factor).  Every step is a child
process under its own `timeout -k 10`; the first failure ends the script.  The two arms' reports are compared with cmp.

  python scripts/kcov_bench.py [--out profiles/kcov_bench.json] [--host-seconds 60 | --reads N] [--repeats 3] [--big-factor 10]
  python scripts/kcov_bench.py --stages DIR     internal: lmat_cov_run through the Python API on the reads of DIR, one JSON line"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "lmat_amd", "csrc", "content_summ")
K_SIZES = "8,10,12,14,17"
N_SPECIES, GENOME, READ_LEN, N_FILES = 64, 200000, 150, 8
TID0 = 1000   # species taxids TID0 .. TID0 + 63: four digits, so every .out line has the same width


def make_run(d, n_reads, seed=11):
    """-> argv tail of content_summ for the run written into d"""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    genomes = letters[rng.integers(0, 4, N_SPECIES * GENOME)]
    head = np.frombuffer(b"r\t", dtype=np.uint8)
    mid = np.frombuffer(b"\t-1 -1 150\t-1\t", dtype=np.uint8)
    tail = np.frombuffer(b" 1.5 DirectMatch\n", dtype=np.uint8)
    width = head.size + READ_LEN + mid.size + 4 + tail.size
    counts = np.zeros(N_SPECIES, dtype=np.int64)
    per_file = (n_reads + N_FILES - 1) // N_FILES
    names = []
    for fi in range(N_FILES):
        fn = os.path.join(d, "rl%d.out" % fi)
        names.append(fn)
        with open(fn, "wb") as f:
            left = min(per_file, n_reads - fi * per_file)
            while left > 0:
                n = min(left, 1 << 19)
                left -= n
                sp = rng.integers(0, N_SPECIES, n)
                pos = rng.integers(0, GENOME - READ_LEN, n)
                reads = genomes[(sp * GENOME + pos)[:, None] + np.arange(READ_LEN)[None, :]]
                err = rng.random((n, READ_LEN)) < 0.01
                reads[err] = letters[rng.integers(0, 4, int(err.sum()))]
                counts += np.bincount(sp, minlength=N_SPECIES)
                line = np.empty((n, width), dtype=np.uint8)
                line[:, :head.size] = head
                o = head.size
                line[:, o:o + READ_LEN] = reads
                o += READ_LEN
                line[:, o:o + mid.size] = mid
                o += mid.size
                tid = sp + TID0
                for j, p in enumerate((1000, 100, 10, 1)):
                    line[:, o + j] = 48 + (tid // p) % 10
                o += 4
                line[:, o:] = tail
                f.write(line.tobytes())
    with open(os.path.join(d, "rl.flst"), "w") as f:
        f.write("\n".join(names) + "\n")
    tids = [TID0 + i for i in range(N_SPECIES)]
    with open(os.path.join(d, "tax.dat"), "w") as f:
        f.write("# synthetic taxonomy of scripts/kcov_bench.py\n#\n%d\n" % (N_SPECIES + 1))
        f.write("1 %d %s 1\nroot\n" % (N_SPECIES, " ".join(map(str, tids))))
        for t in tids:
            f.write("%d 0 1\nspecies %d\n" % (t, t))
    with open(os.path.join(d, "ranks.txt"), "w") as f:
        f.write("1 no_rank\n" + "".join("%d species\n" % t for t in tids))
    with open(os.path.join(d, "run.fastsummary"), "w") as f:
        for t, c in zip(tids, counts):
            if c:
                f.write("%g\t%d\t%d\tspecies,species %d\n" % (float(c), c, t, t))
    return ["-c", os.path.join(d, "tax.dat"), "-l", os.path.join(d, "run.fastsummary"), "-k", K_SIZES, "-f", os.path.join(d, "rl.flst"),
            "-r", os.path.join(d, "ranks.txt"), "-a", "plasmid,species,genus"]


def step(cmd, limit, **kw):
    """one child process under its own time limit; a failure ends the script"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, **kw)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write("step failed (%d): %s\n%s\n" % (r.returncode, " ".join(cmd), r.stderr[-2000:]))
        sys.exit(1)
    sys.stderr.write("[%.1f s] %s\n" % (dt, " ".join(cmd[:1] + cmd[-2:])))
    sys.stderr.flush()
    return dt, r.stdout


def arm(args, out, gpu, repeats, limit):
    """best wall seconds of `repeats` runs behind one warm-up, and the last stdout"""
    cmd = [EXE] + args + ["-o", out] + (["-G"] if gpu else [])
    step(cmd, limit)
    best, stdout = None, ""
    for _ in range(repeats):
        dt, stdout = step(cmd, limit)
        best = dt if best is None else min(best, dt)
    return best, stdout


def same_reports(a, b):
    da, db = os.path.dirname(a), os.path.dirname(b)
    fa = sorted(f[len(os.path.basename(a)):] for f in os.listdir(da) if f.startswith(os.path.basename(a)))
    fb = sorted(f[len(os.path.basename(b)):] for f in os.listdir(db) if f.startswith(os.path.basename(b)))
    if fa != fb:
        sys.stderr.write("the two arms wrote different sets of files: %s / %s\n" % (fa, fb))
        sys.exit(1)
    for suffix in fa:
        step(["cmp", a + suffix, b + suffix], 120)
    return len(fa)


def stages(d):
    """the reads of the run in d through lmat_cov_run: the stages' HIP-event ms (the tool prints none)"""
    from lmat_amd import Coverage, Engine
    eng = Engine(0)
    recs = []
    try:
        for rep in range(2):      # the first run warms up code objects and rocPRIM's first launches
            c = Coverage(eng, [int(k) for k in K_SIZES.split(",")])
            t0 = time.perf_counter()
            for fi in range(N_FILES):
                raw = np.fromfile(os.path.join(d, "rl%d.out" % fi), dtype=np.uint8)
                width = int(np.flatnonzero(raw[:4096] == 10)[0]) + 1
                lines = raw.reshape(-1, width)
                n = lines.shape[0]
                blob = np.ascontiguousarray(lines[:, 2:2 + READ_LEN]).reshape(-1)
                off = np.arange(n + 1, dtype=np.uint64) * READ_LEN
                o = 2 + READ_LEN + 14
                tid = sum((lines[:, o + j].astype(np.uint32) - 48) * p for j, p in enumerate((1000, 100, 10, 1))).astype(np.uint32)
                c._chk(c.lib.lmat_cov_add_reads(c.h, blob.ctypes.data, off.ctypes.data, n, tid.ctypes.data))
            t1 = time.perf_counter()
            st = c.run()
            t2 = time.perf_counter()
            c.close()
            recs.append((st, t1 - t0, t2 - t1))
    finally:
        eng.close()
    st, t_add, t_run = recs[-1]
    ms = {n: round(st[n], 3) for n in ("extract_ms", "sort_ms", "segment_ms", "histogram_ms")}
    print(json.dumps({"add_reads_s": round(t_add, 4), "run_s": round(t_run, 4), "device_ms_total": round(sum(ms.values()), 3),
                      "dominant_stage": max(ms, key=ms.get), "windows_per_s": round(st["windows"] / max(t_run, 1e-9)), **ms,
                      **{n: st[n] for n in st if not n.endswith("_ms")}}), flush=True)


def measure(td, label, n_reads, repeats, host):
    d = os.path.join(td, label)
    args = make_run(d, n_reads)
    rec = {"label": label, "reads": n_reads, "bases": n_reads * READ_LEN, "k_sizes": K_SIZES, "out_bytes": sum(os.path.getsize(os.path.join(d, "rl%d.out" % i)) for i in range(N_FILES))}
    dev_s, stdout = arm(args, os.path.join(d, "dev.summ"), True, repeats, 600)
    line = [l for l in stdout.splitlines() if l.startswith("kmer coverage on device: ")]
    if len(line) != 1:
        sys.stderr.write("the -G run did not say that the device counted\n")
        sys.exit(1)
    rec["device_arm_s"] = round(dev_s, 3)
    rec["device_line"] = line[0]
    if host:
        host_s, _ = arm(args, os.path.join(d, "host.summ"), False, repeats, 900)
        rec["host_arm_s"] = round(host_s, 3)
        rec["host_over_device"] = round(host_s / dev_s, 2)
        rec["files_compared_equal"] = same_reports(os.path.join(d, "host.summ"), os.path.join(d, "dev.summ"))
    _, out = step([sys.executable, os.path.abspath(__file__), "--stages", d], 600)
    rec["device_stages"] = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    # what is left of the device arm's wall time outside lmat_cov_run: process start, library load, parsing the .out text, report writing
    rec["device_arm_outside_run_s"] = round(dev_s - rec["device_stages"]["run_s"], 3)
    print(json.dumps(rec), flush=True)
    shutil.rmtree(d)
    return rec


def calibrate(td, seconds):
    """reads at which the host arm takes about `seconds`, from one short host run (the cost per read grows slowly with the maps)"""
    d = os.path.join(td, "calib")
    n = 20000
    args = make_run(d, n)
    dt, _ = step([EXE] + args + ["-o", os.path.join(d, "host.summ")], 600)
    shutil.rmtree(d)
    return max(n, int(n * seconds / dt / 10000) * 10000), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--host-seconds", type=float, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big-factor", type=int, default=10)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--stages", default=None)
    a = ap.parse_args()
    if a.stages:
        stages(a.stages)
        return
    recs = []
    with tempfile.TemporaryDirectory(dir=a.tmp) as td:
        n = a.reads
        if not n:
            n, dt = calibrate(td, a.host_seconds)
            recs.append({"label": "calibration", "reads": 20000, "host_arm_s": round(dt, 3), "reads_for_%gs" % a.host_seconds: n})
            print(json.dumps(recs[-1]), flush=True)
        recs.append(measure(td, "both_arms", n, a.repeats, True))
        if a.big_factor > 1:
            recs.append(measure(td, "device_alone_x%d" % a.big_factor, n * a.big_factor, a.repeats, False))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
