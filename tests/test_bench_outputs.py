"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy files (CPU: the writer; GPU: a plain
and a --full run of the benchmark write the same outputs, and they are the records a blocking classify of those reads returns)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _records(n):
    from lmat_amd import READ_RESULT_DTYPE
    rec = np.zeros(n, dtype=READ_RESULT_DTYPE)
    rec["call_tid"] = np.arange(n) % 3328 + 1000
    rec["valid_kmers"] = np.arange(n) % 131
    rec["call_score"] = (np.arange(n) % 97) / 97.0
    return rec


def test_dump_writes_float_arrays_within_64_mb_from_a_fixed_sample(tmp_path):
    import bench
    n, first = 3_000_000, 5_000_000
    rec = _records(n)
    counts = {1007: (5, 2.5), 1000: (3, 1.25)}
    a = bench.dump_outputs(str(tmp_path / "a"), rec, first, counts, [1, 2, 3])
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(a) and {"read_index", "call_tid", "call_score", "tally_count"} <= set(names)
    loaded = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    assert all(v.dtype == np.float64 for v in loaded.values())
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in names) <= 64 * 10**6
    ix = loaded["read_index"]
    assert ix.size == bench.DUMP_SAMPLE_READS and (np.diff(ix) > 0).all() and first <= ix[0] and ix[-1] < first + n
    local = (ix - first).astype(np.int64)
    for f in bench.DUMP_FIELDS:
        assert (loaded[f] == rec[f][local].astype(np.float64)).all(), f
    assert loaded["tally_taxid"].tolist() == [1000, 1007] and loaded["tally_count"].tolist() == [3, 5]
    assert loaded["tally_score"].tolist() == [1.25, 2.5] and loaded["tally_nomatch"].tolist() == [1, 2, 3]
    b = bench.dump_outputs(str(tmp_path / "b"), rec, first, counts, [1, 2, 3])   # the same sample every time
    assert all((a[k] == b[k]).all() for k in a)
    small = bench.dump_outputs(str(tmp_path / "c"), rec[:1000], 0, {}, [0, 0, 0])   # a small launch: every read
    assert small["read_index"].tolist() == list(range(1000)) and small["tally_count"].size == 0


def _bench(out_dir, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--db-gb", "8.3", "--batch", "30000", "--launch-reads", "10000",
                        "--steps", "40", "--warmup", "1", "--dump-outputs", str(out_dir), *args],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    names = sorted(f[:-4] for f in os.listdir(out_dir))
    return json.loads(lines[0]), {k: np.load(os.path.join(out_dir, k + ".npy")) for k in names}


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_last_steps_records(tmp_path):
    """40 timed steps of 3 launches of 10 k reads over a pool of 32 batches: the last step is batch (1 + 39) % 32 = 8, its last
    launch reads 260000 .. 269999.  A plain run's line has the headline keys only; --full adds the other legs, after the dump."""
    plain, dp = _bench(tmp_path / "plain")
    full, df = _bench(tmp_path / "full", "--full", "--no-cpu", "--windows", "1")
    for line in (plain, full):
        assert line["steps"] == 40 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["unit"] == "reads/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
        assert line["config"]["read_pool_batches"] == 32
    assert not {"roofline", "value_with_candidates", "e2e_stream", "cpu_baseline"} & set(plain) and plain["windows"] == []
    assert {"roofline", "value_with_candidates", "e2e_stream"} <= set(full) and len(full["windows"]) == 1
    assert sorted(dp) == sorted(df)
    assert dp["read_index"].tolist() == list(range(260000, 270000))
    for k in dp:
        if k == "tally_score":
            assert np.allclose(dp[k], df[k], rtol=1e-9, atol=0), k
        else:
            assert (dp[k] == df[k]).all(), k
    # every read of the 40 timed steps tallied once
    assert dp["tally_count"].sum() + dp["tally_nomatch"].sum() == 40 * 30000
    # the records are those a blocking classify of the same reads returns
    from lmat_amd import Engine, Params
    import bench
    eng = Engine(0, Params.run_rl(prn_all=0))
    eng.synth_taxonomy(bench.BRANCHING)
    table_bytes = int(8.3 * (1 << 30)) // 64 * 64
    G = int(0.8 * (table_bytes / 8) / (768 * (1.0 + 3 * (1.0 - 0.99 ** 20))))
    eng.synth_db(G, k=20, seed=2002, table_bytes=table_bytes)
    assert eng.db_size == full["config"]["db_kmers"]
    reads = eng.synth_reads(270000, (150,), seed=3003)
    res, _ = eng.classify(reads, 260000, 10000, want_cands=False)
    for f in bench.DUMP_FIELDS:
        assert (dp[f] == res[f].astype(np.float64)).all(), f
    reads.free()
    eng.close()
