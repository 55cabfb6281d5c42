#!/bin/bash
# per-kernel times of a bench run WITH the streamed leg (pack kernel, copies): scripts/prof_e2e.sh <tag>  -> $OUT/prof_<tag>*
# (OUT defaults to prof_out/ in the repository)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/prof_out}; mkdir -p $OUT
rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d $OUT/prof_$1 -o p -- python3 $R/bench.py --full --steps 4 --warmup 2 --no-cpu --windows 0 > $OUT/prof_$1.json 2> $OUT/prof_$1.err
f=$(find $OUT/prof_$1 -name '*kernel_stats.csv' | head -1)
python3 - "$f" <<'P'
import csv, sys
for r in list(csv.DictReader(open(sys.argv[1])))[:16]:
    if "synth" in r["Name"] or "cpt_" in r["Name"]: continue
    print("%-70s calls %5s avg_us %10.1f total_ms %9.2f" % (r["Name"][:70], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6))
P
