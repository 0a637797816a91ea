# Regenerates the evidence under <out>/<tag>/ (run on the GPU box from the repo root); copy what is to be tracked
# into profiles/ with the round prefix.   tools/refresh_profiles.sh [tag (default r03)] [out (default out)]
set -e
tag=${1:-r03}
R=$PWD
O=$R/${2:-out}/$tag
export TMPDIR=/tmp
mkdir -p $O
# (1) default bench line with the roofline pass and cpu_baseline (--full)
timeout -k 10 900 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
tail -1 $O/bench_default.json | cut -c1-200
# (2) kernel stats of the same command (no cpu leg under the profiler)
(cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o st -- python3 $R/bench.py --full --no-cpu-baseline --no-instep > $O/stats.log 2>&1)
cp $O/stats/st_kernel_stats.csv $O/kernel_stats_bench_default.csv
# (3) per-shape conv report + timeline of one replayed step
timeout -k 10 600 python tools/conv_report.py > $O/conv_per_shape_report.txt 2>&1
(cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $O/tl -o tl -- python3 $R/bench.py --steps 4 --warmup 2 --no-conv-timer --no-cpu-baseline > $O/tl.log 2>&1)
python tools/timeline.py $O/tl/tl_kernel_trace.csv > $O/timeline_one_replayed_step.txt
# (4) the other two configurations, same harness
for m in mask_rcnn retinanet; do
  timeout -k 10 600 python bench.py --full --model $m --no-cpu-baseline > $O/bench_$m.json 2> $O/bench_$m.err
  tail -1 $O/bench_$m.json | cut -c1-160
done
rm -rf $O/stats $O/tl
echo refreshed $tag
