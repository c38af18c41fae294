#!/bin/bash
# One GPU-box visit.  Everything lands in $OUT (default: out/ in the repository; copy what should be judged into profiles/).
# usage: tools/gpu_session.sh [tests|bench|prof|pmc|pmcc4|pmcinf|micro]...
cd "${GRAFT_REPO_ROOT:-/root/repo}" || exit 1
ROOT=$(pwd)
OUT=${OUT:-$ROOT/out}
mkdir -p "$OUT"
export PYTHONDONTWRITEBYTECODE=1
rocm-smi --showproductname 2>/dev/null | head -8 > "$OUT/device.txt"
nproc >> "$OUT/device.txt"
# which physical card this visit ran on (a misbehaving box shows up as the same id across visits)
{ hostname; rocm-smi --showuniqueid --showserial --showbus 2>/dev/null | grep -E "Unique|Serial|PCI"; } >> "$OUT/device.txt"
for WHAT in "${@:-bench}"; do
case $WHAT in
tests)
  timeout 3000 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider --durations=10 > "$OUT/pytest_gpu.log" 2>&1
  echo "pytest exit $?" >> "$OUT/pytest_gpu.log"
  tail -30 "$OUT/pytest_gpu.log"
  timeout 900 python __graft_entry__.py --smoke > "$OUT/smoke.log" 2>&1
  echo "smoke exit $?" >> "$OUT/smoke.log"
  tail -3 "$OUT/smoke.log" ;;
micro)
  timeout 600 python tools/microbench.py > "$OUT/microbench.log" 2>&1
  echo "microbench exit $?" >> "$OUT/microbench.log"
  tail -20 "$OUT/microbench.log" ;;
bench)
  timeout 1200 python bench.py --full > "$OUT/bench.log" 2>&1
  echo "bench exit $?" >> "$OUT/bench.log"
  tail -2 "$OUT/bench.log" ;;
prof)
  # kernel stats of the SAME command (minus the CPU / inference legs): 3 + 10 + 1 + 3 = 17 steps of conv launches
  (cd /tmp && export TMPDIR=/tmp && timeout 1200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -o bench -- \
      python "$ROOT/bench.py" --steps 10 --warmup 3 --full --no-cpu-baseline --no-inference --no-fit-path --no-c4 > "$OUT/rocprof_bench.log" 2>&1; echo "rocprof exit $?")
  F=$(find "$OUT/prof_bench" -name "*kernel_stats.csv" | head -1)
  [ -n "$F" ] && head -30 "$F" && python tools/roofline_check.py "$F" "$OUT/rocprof_bench.log" 17 "$OUT/roofline_check.json"
  T=$(find "$OUT/prof_bench" -name "*kernel_trace.csv" | head -1)
  [ -n "$T" ] && python tools/trace_gaps.py "$T" "$OUT/trace_gaps.json" --lo 0.45 --hi 0.75
  find "$OUT/prof_bench" -name "*kernel_trace.csv" -size +30M -delete ;;
pmc)
  # HBM traffic: FETCH_SIZE and WRITE_SIZE need separate passes (TCC has 4 slots: 3 + 2); counters only, no other trace domain
  for C in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && export TMPDIR=/tmp && timeout 1200 rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$OUT/pmc_$C" -o pmc -- \
        python "$ROOT/bench.py" --steps 2 --warmup 1 --full --no-cpu-baseline --no-inference --no-fit-path --no-c4 > "$OUT/rocprof_pmc_$C.log" 2>&1; echo "pmc $C exit $?")
  done
  python tools/pmc_traffic.py "$OUT/pmc_FETCH_SIZE" "$OUT/pmc_WRITE_SIZE" "$OUT/pmc_traffic.json" > /dev/null
  # (rates also over the un-countered durations of the `prof` step's kernel statistics, when that step ran in this visit)
  python tools/pmc_report.py "$OUT/pmc_FETCH_SIZE" "$OUT/pmc_WRITE_SIZE" "$OUT/pmc_kernels.json" "" \
      "$(find "$OUT/prof_bench" -name '*kernel_stats.csv' 2>/dev/null | head -1)" | head -60
  # (copy $OUT/pmc_traffic.json and $OUT/pmc_kernels.json to profiles/: bench.py reads them there, keyed on the source hash)
  find "$OUT/pmc_FETCH_SIZE" "$OUT/pmc_WRITE_SIZE" -name "*.csv" -size +8M -delete ;;
pmcc4)
  # HBM traffic of the position-sensitive R-FCN head's kernels (BASELINE C4, tools/c4_bench.py): durations from an un-countered --stats
  # run, FETCH / WRITE from two counter passes of the same command -> $OUT/pmc_c4_kernels.json (copy to profiles/: bench.py's c4 leg)
  (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_c4" -o c4 -- \
      python "$ROOT/tools/c4_bench.py" 6 2 16 > "$OUT/prof_c4.log" 2>&1; echo "prof c4 exit $?")
  for C in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$OUT/pmcc4_$C" -o pmc -- \
        python "$ROOT/tools/c4_bench.py" 2 1 16 > "$OUT/rocprof_pmcc4_$C.log" 2>&1; echo "pmcc4 $C exit $?")
  done
  python tools/pmc_report.py "$OUT/pmcc4_FETCH_SIZE" "$OUT/pmcc4_WRITE_SIZE" "$OUT/pmc_c4_kernels.json" "" \
      "$(find "$OUT/prof_c4" -name '*kernel_stats.csv' 2>/dev/null | head -1)" | grep -i "psroi_ps\|avgpool\|kernel" | head -12
  find "$OUT/pmcc4_FETCH_SIZE" "$OUT/pmcc4_WRITE_SIZE" "$OUT/prof_c4" -name "*.csv" -size +8M -delete ;;
pmcinf)
  # HBM traffic of the inference pass's kernels: the same two counter passes over a 16-image AutoFocus pass,
  # durations from an un-countered --stats run of the same command
  (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_inf16" -o inf16 -- \
      python "$ROOT/tools/infer_profile.py" 1 3 - 1 16 - distinct > "$OUT/prof_inf16.log" 2>&1; echo "prof inf16 exit $?")
  for C in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --pmc $C --output-format csv -d "$OUT/pmcinf_$C" -o pmc -- \
        python "$ROOT/tools/infer_profile.py" 1 3 - 1 16 - distinct > "$OUT/rocprof_pmcinf_$C.log" 2>&1; echo "pmcinf $C exit $?")
  done
  python tools/pmc_report.py "$OUT/pmcinf_FETCH_SIZE" "$OUT/pmcinf_WRITE_SIZE" "$OUT/pmc_infer_kernels.json" "" \
      "$(find "$OUT/prof_inf16" -name '*kernel_stats.csv' 2>/dev/null | head -1)" | head -40
  find "$OUT/pmcinf_FETCH_SIZE" "$OUT/pmcinf_WRITE_SIZE" "$OUT/prof_inf16" -name "*.csv" -size +8M -delete ;;
esac
done
