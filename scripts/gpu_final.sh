# end-of-round evidence run (one box): tests, default bench, kernel trace, PMC traffic, dtype / config variants, raster workload, N > 1 on one GPU
set -x
cd $GRAFT_REPO_ROOT
R=$PWD
O=gpurun_out/r3f
mkdir -p $O
export TMPDIR=/tmp
timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -12 > $O/tests.log
tail -4 $O/tests.log
timeout 900 python bench.py --full > $O/bench_bf16.json 2> $O/bench_bf16.err
(cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $R/$O/prof -o bench -- python $R/bench.py --full --no-cpu-baseline --no-secondary > $R/$O/bench_bf16_profiled.json 2> $R/$O/bench_profiled.err)
DB=$(find $O/prof -name "*.db" | head -1)
python scripts/rocpd_stats.py $DB 70 > $O/bench_kernel_stats.txt
rm -rf $O/prof
timeout 900 python scripts/pmc_kernel_traffic.py 'k_attn5' $O/attn_traffic.json -- python $R/scripts/attn5_check.py time 0 > $O/attn_traffic.log 2>&1
timeout 600 python bench.py --full --dtype f16 --no-cpu-baseline --no-secondary > $O/bench_f16.json 2> $O/bench_f16.err
timeout 600 python bench.py --full --dtype fp8 --no-cpu-baseline --no-secondary > $O/bench_fp8.json 2> $O/bench_fp8.err
timeout 600 python bench.py --full --chunk-size 8 --mask --dtype fp8 --no-cpu-baseline --no-secondary > $O/bench_config4_fp8.json 2> $O/bench_config4_fp8.err
timeout 600 python bench.py --full --chunk-size 8 --mask --no-cpu-baseline --no-secondary > $O/bench_config4_bf16.json 2> $O/bench_config4_bf16.err
timeout 600 python bench.py --full --gaussians 2000000 --views 10 --no-cpu-baseline --no-secondary > $O/bench_config3_one_shard.json 2> $O/bench_config3.err
timeout 600 python bench.py --full --inflight 1 --no-cpu-baseline --no-secondary > $O/bench_bf16_inflight1.json 2> $O/bench_inflight1.err
GC_ATTN_V=4 timeout 600 python bench.py --full --no-cpu-baseline --no-secondary > $O/bench_bf16_attn4.json 2> $O/bench_attn4.err
GC_FUSED_HEAD=0 GC_FUSED_TAIL=0 timeout 600 python bench.py --full --no-cpu-baseline --no-secondary > $O/bench_bf16_perop_blocks.json 2> $O/bench_perop_blocks.err
GC_FUSED_HEAD=0 timeout 600 python bench.py --full --no-cpu-baseline --no-secondary > $O/bench_bf16_tail_only.json 2> $O/bench_tail_only.err
PYTHONPATH=. timeout 300 python scripts/ttail_check.py bf16 time > $O/ttail_check_bf16.txt 2>&1
PYTHONPATH=. timeout 300 python scripts/ttail_check.py f16 time > $O/ttail_check_f16.txt 2>&1
PYTHONPATH=. timeout 300 python scripts/thead_check.py > $O/thead_check_bf16.txt 2>&1
PYTHONPATH=. timeout 300 python scripts/thead_check.py f16 > $O/thead_check_f16.txt 2>&1
PYTHONPATH=. timeout 300 python scripts/gn_shapes.py > $O/gn_shapes.txt 2>&1
PYTHONPATH=$R timeout 900 python scripts/pmc.py 'k_ttail|k_thead' -- python $R/scripts/ttail_check.py bf16 time > $O/ttail_pmc.txt 2>&1
PYTHONPATH=$R timeout 900 python scripts/pmc.py 'k_thead' -- python $R/scripts/thead_check.py > $O/thead_pmc.txt 2>&1
PYTHONPATH=. timeout 600 python scripts/cpu_bound_check.py 2>&1 | grep -E 'host enqueue' > $O/host_enqueue.txt
timeout 600 python bench.py --full --workload raster --gaussians 1000000 --steps 20 --warmup 2 > $O/raster_1m.json 2> $O/raster_1m.err
timeout 600 python bench.py --full --workload raster --gaussians 4000000 --steps 20 --warmup 2 --no-cpu-baseline > $O/raster_4m.json 2> $O/raster_4m.err
GC_BENCH_ONE_GPU=1 GC_BENCH_BACKEND=gloo timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 2 --steps 14 --warmup 1 > $O/bench2_gloo.json 2> $O/bench2_gloo.err
GC_BENCH_ONE_GPU=1 GC_BENCH_BACKEND=gloo timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29514 bench.py --full --gpus 2 --steps 14 --warmup 1 --ref-mode replicate > $O/bench2_gloo_replicate.json 2> $O/bench2_gloo_replicate.err
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
# HBM traffic of the rasterizer stages (PMC, calibrated), 1 M and 4 M Gaussians
timeout 1200 python scripts/pmc_traffic.py 1000000 4 $O/raster_traffic_1m.json > $O/raster_traffic_1m.log 2>&1
timeout 1500 python scripts/pmc_traffic.py 4000000 4 $O/raster_traffic_4m.json > $O/raster_traffic_4m.log 2>&1
tail -3 $O/smoke.log
python - <<'P'
import json, glob
for f in sorted(glob.glob("gpurun_out/r3f/*.json")):
    try:
        d=json.loads([l for l in open(f).read().strip().splitlines() if l.startswith("{")][-1])
        r=d.get("roofline") or {}
        print(f.split("/")[-1], d.get("value"), d.get("ms_per_step"), d.get("mfma_util_step"), r.get("frac"), r.get("avg_launch_us"), (d.get("secondary") or {}).get("value"), (d.get("roofline_raster") or r.get("chain") or {}).get("frac"))
    except Exception as e: print(f, "ERR", str(e)[:80])
P
