# Round profile: run from the repo root on the GPU machine (bash tools/profile_round.sh [OUTDIR]).
# Full GPU test suite, the bench line (bench.py --full), rocprofv3 kernel stats, and counter passes (each --pmc set in its own run,
# never combined with a trace: MI355X_MICROARCH.md).  Outputs land in OUTDIR (default profile_out/).
set -e
export TMPDIR=/tmp
O=${1:-profile_out}
mkdir -p $O
python -m pytest tests -x -q -m gpu > $O/t_full.log 2>&1 || { tail -30 $O/t_full.log; exit 1; }
tail -2 $O/t_full.log
python bench.py --steps 20 --warmup 3 --full > $O/bench.json 2> $O/bench.err
tail -1 $O/bench.json | cut -c1-400
# kernel stats twice: with ONE step in flight (per-kernel durations comparable with bench.py's live HIP-event numbers, which are
# taken launch by launch) and with the default three (durations inflated wherever the two streams' kernels share the GPU)
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -o s -- python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-extras --pipeline 1 > $O/prof_stats.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats_p2 -o s -- python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-extras > $O/prof_stats_p2.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o f -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-extras --pipeline 1 > $O/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o w -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline --no-extras --pipeline 1 > $O/pmc_w.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_sq1 -o q -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-extras --pipeline 1 > $O/pmc_q1.log 2>&1
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d $O/pmc_sq2 -o q -- python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-extras --pipeline 1 > $O/pmc_q2.log 2>&1
# (counter passes run ONE step in flight: with several, kernels of different steps share the GPU and per-dispatch cycle counts stretch)
find $O/prof_stats $O/pmc_fetch $O/pmc_write $O/pmc_sq1 $O/pmc_sq2 -name "*.csv" | head -20
