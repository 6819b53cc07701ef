"""The f32 rollout's fast-forward rounds off / on (TW_OPT_ROLLOUT_REUSE) alternating in one process: rollout kernel ms and the share
of the records taken from the trajectory.  Default: the bench headline (Puzzle-15, 262,144 envs, D = 128, bench weights and twists);
`trained`: the reference's trained Puzzle-8 policy at D = 32 (the case with the fewest hits).  profiles/r10_rollout_reuse.txt."""
import json, sys
sys.path.insert(0, ".")
import bench
from tests.util import amd_policy, trained_puzzle8_arrays
from twisterl_amd import _lib, twisterl
E = 262144
if "trained" in sys.argv[1:]:
    side, diff, pol = 3, 32, amd_policy(trained_puzzle8_arrays())
else:
    side, diff = 4, 128
    pol = bench.build_policy(bench.synthetic_weights(side * side, seed=0), *bench.transpose_twist(side))
env = twisterl.env.Puzzle(side, side, diff, 2, 256)
coll = twisterl.collector.PPOCollector(E, 0.995, 0.995, 32)
for off in (1, 0):                                           # warm both paths
    with _lib.launch_option(_lib.TW_OPT_ROLLOUT_REUSE, off):
        coll.collect(env, pol, seed=999)
for i in range(3):
    for off in (1, 0):
        with _lib.launch_option(_lib.TW_OPT_ROLLOUT_REUSE, off):
            d = coll.collect(env, pol, seed=1000 + i)
        st = d.stats
        print(json.dumps({"reuse": "off" if off else "on", "seed": 1000 + i, "ms_rollout": round(st["ms_rollout"], 3), "records": st["records"],
                          "reused_evals": st["reused_evals"], "share": round(st["reused_evals"] / st["records"], 4)}), flush=True)
        del d
