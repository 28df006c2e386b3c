#!/bin/bash
# Round-end evidence: rocprofv3 kernel-trace stats of the default bench command (both precisions), plain bench lines, and the PMC passes of the
# dominant kernel and of the mesh query.   usage (on the GPU box, from the repo root): [OUT=dir] bash tools/profile_round.sh <tag>   -> $OUT/<tag>_* (OUT: relative to the repo root, default profile_out)
set -u
TAG=${1:-r02}; ROOT=$(pwd); export TMPDIR=/tmp; OUT=${OUT:-profile_out}; mkdir -p "$OUT"
for prec in bf16x3 fp32; do
  echo "== kernel trace, $prec"
  (cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/$OUT/${TAG}_trace_$prec" -- python3 "$ROOT/bench.py" --steps 5 --warmup 2 --precision $prec --cpu-rays-side 0 --full > "$ROOT/$OUT/${TAG}_bench_${prec}_profiled.json" 2> "$ROOT/$OUT/${TAG}_trace_$prec.err") || echo "trace $prec failed"
  find "$OUT/${TAG}_trace_$prec" -name "*kernel_stats.csv" -exec cp {} "$OUT/${TAG}_kernel_stats_$prec.csv" \;
  head -8 "$OUT/${TAG}_kernel_stats_$prec.csv"
  python3 bench.py --precision $prec --full > "$OUT/${TAG}_bench_$prec.json" 2> "$OUT/${TAG}_bench_$prec.err"; tail -c 400 "$OUT/${TAG}_bench_$prec.json"; echo
done
bash tools/pmc_mode1.sh 1 $OUT/${TAG}_pmc_q1 > $OUT/${TAG}_pmc_q1.log 2>&1
PMC_TOOL=tools/perf_mesh.py bash tools/pmc_mode1.sh - $OUT/${TAG}_pmc_mesh > $OUT/${TAG}_pmc_mesh.log 2>&1
cp $OUT/${TAG}_pmc_q1/summary.txt $OUT/${TAG}_pmc_q1_summary.txt; cp $OUT/${TAG}_pmc_mesh/summary.txt $OUT/${TAG}_pmc_mesh_summary.txt
