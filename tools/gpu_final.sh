#!/bin/bash
# Round evidence on the GPU box (repo root), everything for one TAG, written under $OUT (default out/):
#  1. -m gpu tests and smoke();
#  2. PMC FETCH/WRITE passes over tools/kprof.py -> $OUT/<TAG>_pmc_traffic.json (per launch and per
#     kernel, stamped with the library's build id), copied into profiles/ on the box so the bench below
#     reports roofline.traffic from THIS build (bench.py refuses a summary of another build);
#  3. the bench --full line -> $OUT/<TAG>_bench.json;
#  4. rocprofv3 --kernel-trace --stats of the bench --full step, per call site (roctx ranges, --kernel-rename)
#     -> $OUT/<TAG>_prof/, and per kernel (no rename) -> $OUT/<TAG>_prof_raw/;
#  5. tools/roofline_check.py: the roofline site's rocprof mean next to the bench's in-step mean.
# Usage: TAG=r06_final bash tools/gpu_final.sh ; afterwards copy the $OUT/<TAG>_* summaries into profiles/
set -o pipefail
R=$(pwd); TAG=${TAG:-rNN}
export OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -q -m gpu -x --timeout 300 --timeout-method thread > "$OUT/${TAG}_pytest_gpu.log" 2>&1
rc=$?; echo "pytest rc=$rc" >> "$OUT/${TAG}_pytest_gpu.log"; tail -3 "$OUT/${TAG}_pytest_gpu.log"
[ $rc -eq 0 ] || { grep -E "^E |Error" "$OUT/${TAG}_pytest_gpu.log" | head -20; exit 1; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/${TAG}_smoke.log" 2>&1 || { echo "smoke failed"; tail "$OUT/${TAG}_smoke.log"; exit 1; }
PASSES="3 4" timeout -k 10 900 bash tools/gpu_pmc.sh > "$OUT/${TAG}_pmc.log" 2>&1 || { echo "pmc failed"; tail -20 "$OUT/${TAG}_pmc.log"; exit 1; }
python tools/pmc_traffic.py "$OUT/pmc" > "$OUT/${TAG}_pmc_traffic.json" || exit 1
cp "$OUT/${TAG}_pmc_traffic.json" profiles/ || exit 1
timeout -k 10 600 python bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err" || { echo "bench failed"; grep -v "MIOpen(HIP): Warning" "$OUT/${TAG}_bench.err" | tail -30; exit 1; }
head -c 600 "$OUT/${TAG}_bench.json"; echo
export TMPDIR=/tmp USF_ROCTX=1
timeout -k 10 600 rocprofv3 --kernel-trace --stats --kernel-rename --marker-trace --output-format csv -d "$R/$OUT/${TAG}_prof" -o run -- python3 "$R/bench.py" --full --steps 10 --warmup 5 --no-cpu-baseline --no-replay > "$OUT/${TAG}_bench_prof.json" 2> "$OUT/${TAG}_bench_prof.err" || { echo "rocprof failed"; tail -20 "$OUT/${TAG}_bench_prof.err"; exit 1; }
unset USF_ROCTX
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$OUT/${TAG}_prof_raw" -o run -- python3 "$R/bench.py" --full --steps 10 --warmup 5 --no-cpu-baseline --no-replay > "$OUT/${TAG}_bench_prof_raw.json" 2> "$OUT/${TAG}_bench_prof_raw.err" || { echo "rocprof raw failed"; tail -20 "$OUT/${TAG}_bench_prof_raw.err"; exit 1; }
python tools/roofline_check.py "$OUT/${TAG}_bench_prof.json" "$OUT/${TAG}_prof/run_kernel_stats.csv" "$OUT/${TAG}_bench.json" > "$OUT/${TAG}_roofline_check.json" || exit 1
echo ALLDONE
