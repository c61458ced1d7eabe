#!/bin/bash
# Kernel A/B on ONE box: tools/ab.sh build NAME   (here: current tree -> build/ab/NAME.so)
#                        tools/ab.sh run NAME...  (GPU box: bench every build, REPS times (2), interleaved; every run under its
#                                                  own time limit, and the first run that fails or is cut off ends the session;
#                                                  AB_LOG=<file> keeps the whole JSON lines)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
if [ "$1" = build ]; then
  mkdir -p $ROOT/build/ab
  make -s -C $ROOT/cyclistsocialforce_amd/csrc
  cp $ROOT/cyclistsocialforce_amd/libcsf_hip.so $ROOT/build/ab/$2.so
  exit 0
fi
shift
for rep in $(seq ${REPS:-2}); do
  for name in "$@"; do
    echo -n "$name: "
    CSF_LIB=$ROOT/build/ab/$name.so timeout -k 10 ${RUN_TIMEOUT:-300} python3 $ROOT/bench.py --full --steps ${STEPS:-600} --warmup ${WARMUP:-30} --cpu-ticks 0 ${BENCH_ARGS} | tee -a ${AB_LOG:-/dev/null} |
      grep -o '"value": [0-9.]*\|"launch_us": [0-9.]*\|"healthy": [a-z]*' | tr '\n' ' '
    echo
  done
done
