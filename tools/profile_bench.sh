set -x
# usage: tools/profile_bench.sh [OUTDIR] — OUTDIR absolute or relative to the repository root (default profile_out/, which
# git ignores); the condensed files land there
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-profile_out}
case $OUT in /*) ;; *) OUT=$R/$OUT ;; esac
cd /tmp && export TMPDIR=/tmp
mkdir -p $OUT
cd $R
python bench.py --full --steps 2000 --warmup 200 > $OUT/bench.json 2> $OUT/bench.err
MPPI_BENCH_NO_TSCAN=1 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python bench.py --full --steps 300 --warmup 50 --no-cpu-baseline > $OUT/stats.log 2>&1
MPPI_BENCH_NO_TSCAN=1 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmc_fetch -- python bench.py --full --steps 100 --warmup 20 --no-cpu-baseline > $OUT/pmc_fetch.log 2>&1
MPPI_BENCH_NO_TSCAN=1 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmc_write -- python bench.py --full --steps 100 --warmup 20 --no-cpu-baseline > $OUT/pmc_write.log 2>&1
find $OUT -type f | head -50
for f in $(find $OUT -name "*.csv" | head -12); do echo "== $f"; head -3 $f | cut -c1-400; done
# matrix / vector pipe utilisation of the rollout kernels (tools/pmc_mfma_summary.py)
MPPI_BENCH_NO_TSCAN=1 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_MFMA SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/pmc_mfma -- python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline > $OUT/pmc_mfma.log 2>&1
# the elevation-map RACER models: kernel trace of tools/time_workloads.py racer, then the SQ pipe counters
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/racer_stats -- python tools/time_workloads.py racer > $OUT/racer_stats.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_MFMA SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/racer_pmc -- python tools/time_workloads.py racer > $OUT/racer_pmc.log 2>&1
# condensed files for profiles/ (copy the ones to keep)
python tools/stats_summary.py $OUT/stats $OUT/kernel_stats.csv "python bench.py --full --steps 300 --warmup 50 --no-cpu-baseline" || true
python tools/pmc_summary.py $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_hbm_traffic.json || true
python tools/pmc_mfma_summary.py $OUT/pmc_mfma $OUT/pmc_mfma_valu.json "python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline" || true
python tools/stats_summary.py $OUT/racer_stats $OUT/racer_kernel_stats.csv "python tools/time_workloads.py racer" || true
python tools/pmc_mfma_summary.py $OUT/racer_pmc $OUT/racer_pmc_valu.json "python tools/time_workloads.py racer" || true
rm -rf $OUT/stats $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_mfma $OUT/racer_stats $OUT/racer_pmc
