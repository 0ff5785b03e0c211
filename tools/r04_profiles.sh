#!/bin/bash
# round-4 evidence: bench lines + rocprofv3 kernel traces for every workload (PMC passes for configs[3] only)
#   bash tools/r04_profiles.sh OUTDIR          (the bench lines are written under OUTDIR)
OUT=${1:?usage: bash tools/r04_profiles.sh OUTDIR}
mkdir -p "$OUT"
for wl in lorenz63 lorenz96; do
  timeout 900 python bench.py --full --workload $wl --steps 200 --warmup 20 > "$OUT/${wl}_g1c1_bench.json" 2> "$OUT/${wl}.err"
  PROFILE_PMC=0 PROFILE_KERNEL=net1d bash tools/profile_bench.sh r04_${wl}_g1c1 --workload $wl --steps 200 --warmup 20 > /dev/null 2>&1
done
for wl in kolmogorov64 qg128; do
  timeout 1200 python bench.py --full --workload $wl --steps 20 --warmup 3 > "$OUT/${wl}_g1c1_bench.json" 2> "$OUT/${wl}.err"
  PROFILE_PMC=0 bash tools/profile_bench.sh r04_${wl}_g1c1 --workload $wl --steps 4 --warmup 1 > /dev/null 2>&1
done
for net in global local; do for fr in lo hi; do
  timeout 900 python bench.py --full --workload lorenz_eval --lorenz-net $net --lorenz-freq $fr --cpu-seconds 8 > "$OUT/lorenz_eval_${net}_${fr}_bench.json" 2> "$OUT/le_${net}_$fr.err"
done; done
timeout 900 python bench.py --full --gpus 2 --backend gloo --workload kolmogorov64 --steps 4 --warmup 1 --no-cpu-baseline > "$OUT/kolmogorov64_2rank_gloo_selflaunch_bench.json" 2> "$OUT/2rank.err"
ls -la "$OUT" | head -30
