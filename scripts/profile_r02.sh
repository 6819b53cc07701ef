#!/bin/bash
# round-2 measurement set (run on the GPU box from the repo root): default bench line, rocprofv3 kernel stats of the same
# command, self-play bench lines + SQ counters of the walker kernel, GPU tests, smoke.
set -e
export TMPDIR=/tmp
out=$PWD/gpurun_out/r02; mkdir -p $out
python3 bench.py --full --steps 5 --warmup 2 > $out/bench.json 2> $out/bench.err
(cd /tmp && rocprofv3 --kernel-trace --stats -d $out/stats -o s -f csv -- python3 $OLDPWD/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/stats.log 2>&1)
for cfg in "256 100 8" "512 100 8" "512 1000 8" "1024 100 8" "1024 1000 8" "2048 100 8" "4096 100 8" "4096 1000 8" "6144 100 8" "16384 32 4" "65536 32 4" "262144 32 4"; do set -- $cfg
  python3 scripts/bench_az.py --envs $1 --searches $2 --difficulty $3 --steps 2 2>/dev/null | grep metric >> $out/az_batches.jsonl
done
python3 scripts/bench_az.py --envs 4096 --searches 100 --variant 2 --steps 2 2>/dev/null | grep metric > $out/az_4096x100_lane_per_episode.json
(cd /tmp && rocprofv3 --kernel-trace --stats -d $out/az_stats -o s -f csv -- python3 $OLDPWD/scripts/bench_az.py --envs 4096 --searches 100 --steps 3 > $out/az_stats.log 2>&1)
(cd /tmp && rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_MFMA SQ_WAVE_CYCLES SQ_WAIT_ANY --kernel-trace -d $out/az_pmc -o p -f csv -- python3 $OLDPWD/scripts/bench_az.py --envs 4096 --searches 100 --steps 1 > $out/az_pmc.log 2>&1) || true
python3 scripts/bench_generic_engine.py 2>/dev/null | grep policy > $out/generic_engine.jsonl
python3 -m pytest tests -x -q -m gpu > $out/pytest_gpu.log 2>&1
tail -2 $out/pytest_gpu.log
python3 -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
ls $out
