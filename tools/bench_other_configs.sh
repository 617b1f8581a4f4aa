# usage: tools/bench_other_configs.sh OUTDIR   (the non-headline workloads and precisions, each with its roofline leg)
out="${1:?usage: tools/bench_other_configs.sh OUTDIR}"
mkdir -p "$out"
for c in "--config celebahq256" "--config edm32" "--dtype f16" "--dtype f32x3 --steps 1"; do
  n=$(echo $c | tr -d "-" | tr " " "_")
  python3 bench.py $c --full --no-cpu-baseline > "$out/bench_$n.json" 2> "$out/bench_$n.err" || exit 1
  echo "$n done" >> "$out/bench_progress.log"
done
