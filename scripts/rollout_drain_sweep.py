"""The persistent 256-episode f32 rollout's hand-over (TW_OPT_ROLLOUT_DRAIN) off and at several thresholds, alternating in one process:
rollout ms (both launches, HIP events), the episodes handed over and the drain's grid.  Default: the bench headline (Puzzle-15,
262,144 envs, D = 128, bench weights and twists); `trained [D]`: the reference's trained Puzzle-8 policy at difficulty D (default 32).
Thresholds: `--thr -1,32,64,...` (-1 = off).  profiles/r14_rollout_drain.txt."""
import json, sys
sys.path.insert(0, ".")
import bench
from tests.util import amd_policy, trained_puzzle8_arrays
from twisterl_amd import _lib, twisterl
E = 262144
args = sys.argv[1:]
thr = [-1, 32, 64, 96, 128, 160]
for a in args:
    if a.startswith("--thr="):
        thr = [int(x) for x in a[6:].split(",")]
rounds = next((int(a[9:]) for a in args if a.startswith("--rounds=")), 3)
if "trained" in args:
    nums = [a for a in args if a.isdigit()]
    side, diff, pol = 3, int(nums[0]) if nums else 32, amd_policy(trained_puzzle8_arrays())
else:
    side, diff = 4, 128
    pol = bench.build_policy(bench.synthetic_weights(side * side, seed=0), *bench.transpose_twist(side))
env = twisterl.env.Puzzle(side, side, diff, 2, 256)
coll = twisterl.collector.PPOCollector(E, 0.995, 0.995, 32)
for v in thr[:2]:                                            # warm both launches
    with _lib.launch_option(_lib.TW_OPT_ROLLOUT_DRAIN, v):
        coll.collect(env, pol, seed=999)
for i in range(rounds):
    for v in thr:
        with _lib.launch_option(_lib.TW_OPT_ROLLOUT_DRAIN, v):
            d = coll.collect(env, pol, seed=1000 + i)
            cnt = _lib.debug_counters(2)
        st = d.stats
        print(json.dumps({"drain_live": v, "seed": 1000 + i, "ms_rollout": round(st["ms_rollout"], 3), "ms_total": round(st["ms_total"], 3),
                          "records": st["records"], "reused_evals": st["reused_evals"], "handed_over": cnt[0], "drain_blocks": cnt[1]}), flush=True)
        del d
