#!/bin/bash
# tools/collect_evidence.sh PREFIX OUTDIR -- the measurements profiles/ holds besides the counter passes (tools/collect_counters.sh), in one
# GPU run from the repository root: a kernel trace of bench.py (rocprofv3 --kernel-trace --stats), the bench lines of C1-C4, the rank-share projection.
# Steps are joined with &&: a step that is killed ends the run.  Output under OUTDIR/PREFIX_*.  The bench lines are --full runs (roofline
# block, CPU baseline on C3).
set -e
P=$1
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "$2" && cd "$2" && pwd)
cd /tmp && export TMPDIR=/tmp
mkdir -p $O/${P}_trace
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${P}_trace -o run -- python3 $R/bench.py --full --steps 5 --warmup 2 > $O/${P}_trace/bench.json 2> $O/${P}_trace/err.txt &&
cd $R &&
timeout -k 10 400 python bench.py --full --steps 10 --warmup 3 > $O/${P}_bench_c3.json 2> $O/${P}_bench_c3.err &&
timeout -k 10 200 python bench.py --full --workload c2_bunny_standin --steps 10 --warmup 3 --no-cpu-baseline > $O/${P}_bench_c2.json 2> $O/${P}_bench_c2.err &&
timeout -k 10 200 python bench.py --full --workload c1_cornell_teapot --steps 20 --warmup 5 --no-cpu-baseline > $O/${P}_bench_c1.json 2> $O/${P}_bench_c1.err &&
timeout -k 10 300 python bench.py --full --workload c4_sanmiguel_standin --steps 2 --warmup 1 --no-cpu-baseline > $O/${P}_bench_c4.json 2> $O/${P}_bench_c4.err &&
timeout -k 10 300 python tools/rank_share_experiment.py > $O/${P}_rank_share.txt 2>&1 &&
cat $O/${P}_rank_share.txt &&
python - <<PY
import json
for w in ("c3", "c2", "c1", "c4"):
    d = json.load(open("$O/${P}_bench_%s.json" % w))
    print(w, round(d["value"], 1), "Mray/s", round(d["ms_per_step"], 2), "ms", "frac", d["roofline"]["frac"], "of", (d["roofline"]["frac_of"] or "-")[:24], "hbm_frac", d["roofline"]["hbm_frac"], "cpu", d.get("cpu_baseline", {}).get("value"))
PY
