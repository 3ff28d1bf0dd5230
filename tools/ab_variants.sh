#!/bin/bash
# A/B of compile-time variants of libopenr_hip on the GPU box (scratch copy):
#   tools/ab_variants.sh "-DFOO" "" "-DBAR"  -> phase ms + value per variant
# A build, bench or parse that fails ends the script: nothing more runs on the GPU.
set -e
set -o pipefail
for V in "$@"; do
  bash tools/diag_build.sh $V
  LINE=$(timeout -k 10 120 python bench.py --full --steps 20 --no-cpu-baseline --no-route-db | tail -1)
  RES=$(python3 -c "import json,sys;d=json.loads(sys.argv[1]);print(d['roofline']['phase_ms'], d['value'])" "$LINE")
  echo "[$V]: $RES"
done
