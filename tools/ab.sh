#!/bin/bash
# A/B of bench.py under environment variants, interleaved in one box session:  bash tools/ab.sh <tag> <rounds> "VAR=1 VAR2=x" "..." ...
# Two builds of the library compare the same way, alternating on ONE box (boxes differ by ~1.5 %, a build's effect is often smaller):
# copy each build's flocoder_amd/_lib/libflocoder_amd.so to ab_libs/ (git-ignored) and give one variant per library, e.g.
#     bash tools/ab.sh libs 3 "FLOCODER_AMD_LIB=$PWD/ab_libs/lib_main.so" "FLOCODER_AMD_LIB=$PWD/ab_libs/lib_new.so"
# The first variant that fails stops the run: its number, its environment and its exit status are printed.
TAG=$1; ROUNDS=$2; shift 2
OUT=gpurun_out/$TAG; mkdir -p $OUT
for r in $(seq 1 $ROUNDS); do
  i=0
  for v in "$@"; do
    i=$((i+1))
    env $v timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-secondary --no-roofline --steps 10 --warmup 3 > $OUT/ab_${i}_$r.json 2> $OUT/ab_${i}_$r.err
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "variant $i [$v] failed in round $r with exit status $rc"
      tail -5 $OUT/ab_${i}_$r.err
      exit $rc
    fi
    echo "round $r [$v] $(python3 -c "import json;d=json.load(open('$OUT/ab_${i}_$r.json'));print(d['value'], d['ms_per_step'])" 2>/dev/null)"
  done
done
