#!/bin/bash
# Run ON THE GPU BOX (through gpurun): same-box A/B of the headline between the product library and alternative builds.
# Boxes differ by a few per cent, runs on one box by ~0.5 %: a variant is only ever compared with the library built from
# HEAD in alternation on the SAME box.
#   build:  compile the variant's objects into hironaka_amd/csrc/alt_<name>.so (not tracked; it travels with gpurun)
#   usage:  scripts/ab_headline.sh <rounds> <name> [<name> ...]      ("base" is always the first leg of a round)
#   AB_STEPS / AB_WARMUP in the environment: bench.py's --steps / --warmup (default 20 / 5; 2000 / 200 for a decision)
#   AB_TIMEOUT: seconds a single run may take (default 120); a run that fails or overruns ends the alternation there
set -u
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
C=$ROOT/hironaka_amd/csrc
ROUNDS=$1; shift
B="timeout -k 10 ${AB_TIMEOUT:-120} python $ROOT/bench.py --steps ${AB_STEPS:-20} --warmup ${AB_WARMUP:-5} --no-search --no-cpu-baseline --no-single-step"
cp $C/libhironaka_hip.so /tmp/hk_base.so
for i in $(seq 1 $ROUNDS); do
  for v in base "$@"; do
    if [ "$v" = base ]; then cp /tmp/hk_base.so $C/libhironaka_hip.so; else cp $C/alt_$v.so $C/libhironaka_hip.so; fi
    $B > $ROOT/gpurun_out/ab_${v}_$i.json 2> /dev/null
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v round $i: exit status $rc, stopping"; cp /tmp/hk_base.so $C/libhironaka_hip.so; exit $rc; fi
    echo "$v $(python $ROOT/scripts/bench_summary.py $ROOT/gpurun_out/ab_${v}_$i.json | head -1)"
  done
done
cp /tmp/hk_base.so $C/libhironaka_hip.so
