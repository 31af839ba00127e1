#!/bin/bash
# Whole evidence set of a round in one GPU session: tools/profile_all.sh <tag>  ->  $PROFILE_OUT/<tag>/ (default profile_out/; default bench
# profile, per-config tables and rocprofv3 statistics, LastFM sparse-path numbers, the data-parallel step's bench line and timeline)
set -x
T=${1:-r03}
R="$(cd "$(dirname "$0")/.." && pwd)"
export PROFILE_OUT="${PROFILE_OUT:-$R/profile_out}"
O="$PROFILE_OUT/$T"
mkdir -p "$PROFILE_OUT"
cd "$R"
bash tools/profile_round.sh $T > "$PROFILE_OUT/${T}_profile_round.log" 2>&1; echo "profile_round rc=$?"
python tools/config_profiles.py > "$O"/config_profiles.md 2> "$O"/config_profiles.err; echo "config_profiles rc=$?"; tail -2 "$O"/config_profiles.err
for c in c1_defaults c1_tuned c3 c4_e32 c5 c5_f16; do
  bash tools/trace_stats.sh $T/trace_$c tools/config_profiles.py $c > /dev/null 2>&1; echo "trace $c rc=$?"
done
python tools/c1_bench.py > "$O"/c1.log 2>&1
GANMF_BENCH_FORCE_COMM=1 python bench.py --full --no-cpu-baseline > "$O"/bench_fc.json 2> "$O"/bench_fc.err
cd /tmp && export TMPDIR=/tmp
GANMF_BENCH_FORCE_COMM=1 rocprofv3 --kernel-trace --output-format csv -d "$O"/trace_fc -- python3 "$R"/bench.py --full --no-cpu-baseline --steps 64 --warmup 32 > "$O"/trace_fc.log 2>&1
cd "$R"
python3 tools/timeline.py "$(ls "$O"/trace_fc/*/*_kernel_trace.csv | head -1)" 40 1 de_dcoef_kernel > "$O"/timeline_fc_D.txt
python3 tools/timeline.py "$(ls "$O"/trace_fc/*/*_kernel_trace.csv | head -1)" 40 1 > "$O"/timeline_fc_G.txt
find "$O" -name "*_kernel_trace.csv" -delete
du -sh "$O"
