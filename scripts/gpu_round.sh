#!/bin/bash
# One GPU session: smoke -> GPU parity tests -> bench (small, then config B) -> rocprof.
# Each GPU step has its own time limit; a crash/timeout (exit > 1) ends the session.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}; export OUT  # where the logs and result files go
mkdir -p "$OUT"
export TMPDIR=/tmp
STEPS="${*:-smoke pytest bench_small bench}"
status() { echo "$1 rc=$2 t=$(date +%s)" | tee -a $OUT/status.txt; }
# a progress tick under $OUT/ while long quiet steps run (input generation, D-sized benches)
( while sleep 45; do date +%s >> $OUT/tick.txt; done ) &
TICK=$!
trap 'kill $TICK 2>/dev/null' EXIT
for s in $STEPS; do
  case $s in
    configs) timeout -k 10 1500 python scripts/configs.py ${CONFIGS:-E91 C20k E9100 C20k_m15} > $OUT/configs.log 2>&1 ;;
    e2e) timeout -k 10 300 python scripts/e2e_quick.py a1k b3k30 m2k_id80 fam2k fam2k_id85 > $OUT/e2e.log 2>&1 ;;
    smoke) timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 ;;
    pytest) timeout -k 10 1500 python -u -m pytest tests -m gpu -v -p no:cacheprovider --timeout 900 --timeout-method thread --durations=25 > $OUT/pytest_gpu.log 2>&1 ;;
    pytest_k) timeout -k 10 1200 python -u -m pytest tests -m gpu -v -p no:cacheprovider --timeout 900 --timeout-method thread -k "${PYK}" > $OUT/pytest_k.log 2>&1 ;;
    bench_d_rehearsal) MC_BENCH_ONE_GPU=1 timeout -k 10 1200 python bench.py --gpus 2 --workload D --steps 2 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench_d_rehearsal.json > $OUT/bench_d_rehearsal.log 2>&1 ;;
    bench_d1) timeout -k 10 900 python bench.py --workload D --steps 2 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench_d1.json > $OUT/bench_d1.log 2>&1 ;;
    bench_b_rehearsal) MC_BENCH_ONE_GPU=1 timeout -k 10 900 python bench.py --gpus 2 --steps 3 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench_b_rehearsal.json > $OUT/bench_b_rehearsal.log 2>&1 ;;
    bench_small) timeout -k 10 600 python bench.py --n 20000 --templates 200 --steps 2 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench_small.json > $OUT/bench_small.log 2>&1 ;;
    bench_align) timeout -k 10 600 python bench.py --n 20000 --templates 200 --id 0.55 --steps 1 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench_align.json > $OUT/bench_align.log 2>&1 ;;
    bench_nocpu) timeout -k 10 900 python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-config-d --stats-out $OUT/bench.json > $OUT/bench.log 2>&1 ;;
    bench) timeout -k 10 900 python bench.py --full --steps 3 --warmup 1 --stats-out $OUT/bench.json > $OUT/bench.log 2>&1 ;;
    prof) timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/prof.log 2>&1 ;;
    pmc_fetch) timeout -k 10 900 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -o run -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/pmc_fetch.log 2>&1 ;;
    pmc_write) timeout -k 10 900 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -o run -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/pmc_write.log 2>&1 ;;
    valu) timeout -k 10 120 ./scripts/microbench/valu_peak > $OUT/valu_peak.json 2> $OUT/valu_peak.err ;;
    accum_prof4) MC_ACCUM_PROFILE=4 timeout -k 10 300 python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/accum_prof4.log 2>&1 ;;
    accum_prof2) MC_ACCUM_PROFILE=2 timeout -k 10 300 python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/accum_prof2.log 2>&1 ;;
    accum_prof1) MC_ACCUM_PROFILE=1 timeout -k 10 300 python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-config-d > $OUT/accum_prof1.log 2>&1 ;;
    *) echo "unknown step $s"; continue ;;
  esac
  rc=$?
  status "$s" "$rc"
  if [ "$s" = pytest ] && [ $rc -eq 1 ]; then continue; fi
  # rocprofv3 on this image segfaults (139) at exit after writing its files: that ends the
  # session too, so give prof / pmc_fetch / pmc_write each a gpurun call of their own (last)
  if [ $rc -ne 0 ]; then exit $rc; fi
done
