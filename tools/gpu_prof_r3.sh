# Round-3 profile set: benches (C1 with the CPU baseline, target, C3, C4), kernel traces (C1 side stream
# on / off, target serial, C3, C4), PMC HBM bytes (FETCH_SIZE / WRITE_SIZE, separate passes) at C1, the
# target shape, C3 and C4.      usage: bash tools/gpu_prof_r3.sh <tag>   (outputs under gpurun_out/<tag>_*)
T=${1:-r3p}
PART=${2:-all}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
PMC() {  # <name> <counter> <bench args>
  echo "180|${T}_$1|timeout -s KILL 170 rocprofv3 --pmc $2 --output-format csv -d gpurun_out/${T}_$1 -o run -- python3 bench.py $3 --no-cpu-baseline --exact-steps 0"
}
STEPS1=(
 "300|${T}_bench_c1|python -u bench.py --full"
 "200|${T}_bench_target|python -u bench.py --full --config target --no-cpu-baseline --steps 20"
 "200|${T}_bench_c3|python -u bench.py --full --config c3 --no-cpu-baseline --steps 10"
 "300|${T}_bench_c4|python -u bench.py --full --config c4 --no-cpu-baseline --steps 6 --warmup 2"
 "300|${T}_prof_c1|rocprofv3 --kernel-trace --stats -d gpurun_out/${T}_prof_c1 -o run -- python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline --exact-steps 0"
 "300|${T}_prof_c1s|MMT_SIDE_STREAM=0 rocprofv3 --kernel-trace --stats -d gpurun_out/${T}_prof_c1s -o run -- python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline --exact-steps 0"
 "300|${T}_prof_ts|MMT_SIDE_STREAM=0 rocprofv3 --kernel-trace --stats -d gpurun_out/${T}_prof_ts -o run -- python3 bench.py --config target --steps 10 --warmup 3 --no-cpu-baseline --exact-steps 0"
 "300|${T}_prof_c3|rocprofv3 --kernel-trace --stats -d gpurun_out/${T}_prof_c3 -o run -- python3 bench.py --config c3 --steps 4 --warmup 2 --no-cpu-baseline --exact-steps 0"
 "300|${T}_prof_c4|rocprofv3 --kernel-trace --stats -d gpurun_out/${T}_prof_c4 -o run -- python3 bench.py --config c4 --steps 3 --warmup 1 --no-cpu-baseline --exact-steps 0"
)
STEPS2=(
 "$(PMC pmc_fetch_c1 FETCH_SIZE '--steps 2 --warmup 1')"
 "$(PMC pmc_write_c1 WRITE_SIZE '--steps 2 --warmup 1')"
 "$(PMC pmc_fetch_t FETCH_SIZE '--config target --steps 2 --warmup 1')"
 "$(PMC pmc_write_t WRITE_SIZE '--config target --steps 2 --warmup 1')"
 "$(PMC pmc_fetch_c3 FETCH_SIZE '--config c3 --steps 1 --warmup 1')"
 "$(PMC pmc_write_c3 WRITE_SIZE '--config c3 --steps 1 --warmup 1')"
 "$(PMC pmc_fetch_c4 FETCH_SIZE '--config c4 --steps 1 --warmup 1')"
 "$(PMC pmc_write_c4 WRITE_SIZE '--config c4 --steps 1 --warmup 1')"
)
case $PART in
  1) bash tools/gpu_steps.sh "${STEPS1[@]}" ;;
  2) bash tools/gpu_steps.sh "${STEPS2[@]}" ;;
  *) bash tools/gpu_steps.sh "${STEPS1[@]}" "${STEPS2[@]}" ;;
esac
