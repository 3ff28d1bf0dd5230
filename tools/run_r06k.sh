# usage: tools/run_r06k.sh OUT_DIR   (round 6 wrote its outputs to a folder named r06k)
set -e
OUT=${1:?usage: tools/run_r06k.sh OUT_DIR}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread tests/test_gpu_configs.py tests/test_gpu_policy.py > "$OUT/tests.log" 2>&1
bash tools/ksp2_ab_r06.sh "$OUT" "" g8 g2
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
