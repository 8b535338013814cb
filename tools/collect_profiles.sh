# Collects the evidence set judged under profiles/ (run on the GPU box: gpurun -- bash tools/collect_profiles.sh r01)
# $1 = round tag.  Output goes to gpurun_out/prof_<tag>/ ; copy the summaries into profiles/ afterwards.
TAG=${1:-r01}
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/prof_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
python $R/bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/bench.err
rm -rf /tmp/kt && timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/kt -o kt --output-format csv -- python $R/bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench_under_rocprof.json 2> /tmp/kt.err
cp $(find /tmp/kt -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_bench_kernel_stats.csv
for set in "sq:GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT" "fetch:FETCH_SIZE" "write:WRITE_SIZE"; do
  name=${set%%:*}; ctrs=${set#*:}
  rm -rf /tmp/pmc_$name
  timeout 600 rocprofv3 --kernel-trace --pmc $ctrs -d /tmp/pmc_$name -o p --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > /tmp/pmc_$name.log 2>&1
  D=$(dirname $(find /tmp/pmc_$name -name "*counter_collection.csv" | head -1))
  python $R/tools/pmc_summary.py $D > $OUT/${TAG}_pmc_$name.summary.txt 2>&1
done
ls -la $OUT
# the other BASELINE configs as bench.py lines (own metric strings, never the headline)
for c in c1 c3 c4 c5; do
  timeout 600 python $R/bench.py --full --config $c --steps $([ $c = c1 ] && echo 50 || echo 6) --warmup 2 > $OUT/${TAG}_bench_$c.json 2> /tmp/bench_$c.err
done
timeout 600 python $R/bench.py --full --config c4 --dtype bf16 --steps 6 --warmup 2 > $OUT/${TAG}_bench_c4_bf16.json 2> /tmp/bench_c4b.err
# round 3: the ROI-sharded latency mode at N = 1 (+ the one-GPU projection of rank 0's share of an 8-rank world)
timeout 600 python $R/bench.py --mode latency --steps 20 --warmup 5 > $OUT/${TAG}_bench_latency.json 2> /tmp/bench_lat.err
timeout 600 python $R/bench.py --mode latency --config c3 --steps 6 --warmup 2 > $OUT/${TAG}_bench_latency_c3.json 2> /tmp/bench_lat3.err
# NMS: per-path latency on the SURVEY 8d micro-inputs + the chunked scan's per-chunk cycle trace
timeout 300 python $R/tools/bench_nms.py > $OUT/${TAG}_nms_paths.txt 2>&1
timeout 300 python $R/tools/nms_trace.py > $OUT/${TAG}_nms_trace.txt 2>&1
timeout 300 python $R/tools/bench_layers.py > $OUT/${TAG}_vgg_layers.txt 2>&1
# the widened configurations: per-kernel stats + the tools' own timing lines
for cfg in "mpn:bench_mpn.py" "resnet50:bench_resnet.py" "resnet50_bf16:bench_resnet.py 50 1000 bf16" "inception_mpn_bf16:bench_inception.py 2000 mpn"; do
  name=${cfg%%:*}; tool=${cfg#*:}
  rm -rf /tmp/kt_$name
  timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/kt_$name -o kt --output-format csv -- python $R/tools/$tool > $OUT/${TAG}_${name}_timing.txt 2> /tmp/kt_$name.err
  cp $(find /tmp/kt_$name -name "*kernel_stats.csv" | head -1) $OUT/${TAG}_${name}_kernel_stats.csv
done
ls -la $OUT
# per-launch timeline of the bf16 ResNet-50 image (kernel, grid threads, us)
bash $R/tools/prof_resnet.sh 50 1000 bf16 > $OUT/${TAG}_resnet50_bf16_layers.txt 2>&1
# SQ counters of the bf16 ResNet-50 run (matrix-pipe busy %, waits, LDS bank conflicts per kernel)
rm -rf /tmp/pmc_rn
timeout 600 rocprofv3 --kernel-trace --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT -d /tmp/pmc_rn -o p --output-format csv -- python $R/tools/bench_resnet.py 50 1000 bf16 > /tmp/pmc_rn.log 2>&1
D=$(dirname $(find /tmp/pmc_rn -name "*counter_collection.csv" | head -1))
python $R/tools/pmc_summary.py $D > $OUT/${TAG}_resnet50_bf16_pmc_sq.summary.txt 2>&1
# round 2: the HBM-bound kernels' timing experiments (stores / loads / MFMAs knocked out), the write-bandwidth ceiling they are
# judged against, keep_top_k's phase trace, and the libnms.so drop-in cost per class call
timeout 200 python $R/tools/probes/write_bw.py > $OUT/${TAG}_write_bw.txt 2>&1
timeout 200 python $R/tools/ablate_first.py > $OUT/${TAG}_ablate_conv1_1.txt 2>&1
timeout 200 python $R/tools/ablate_roipool.py > $OUT/${TAG}_ablate_roipool.txt 2>&1
timeout 200 python $R/tools/topk_trace.py > $OUT/${TAG}_topk_trace.txt 2>&1
(cd $R && timeout 300 python -m pytest tests/test_gpu_nms.py -k dropin_cost -m gpu -q -s -p no:cacheprovider > $OUT/${TAG}_libnms_dropin.txt 2>&1)
ls -la $OUT
