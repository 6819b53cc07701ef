"""Records/s of a user-written environment collected ON THE DEVICE (tw_ppo_collect_device_env) against the host-stepped path over
the same struct (tw_ppo_collect_env over the module's vtable): GridWorld 5 x 5 (examples/device_env/gridworld.hpp, max_steps 64)
with the policy shape of the reference's ppo_grid_world_5x5_v1.json (embedding 512, common [128], linear heads), at 1,024 and
65,536 episodes.  Wall clock of whole collect() calls (finalize and result included), median of --reps after --warmup; every
device collect is checked byte-equal to the host one first.

    python scripts/bench_device_env.py [--reps 5] [--out profiles/r05_device_env.jsonl]

--env lamps40: the same comparison for an environment whose observations vary in length (tests/device_envs/lamps.hpp with 40 lamps:
0 .. 40 ids per state, obs_size 1,600, at most 24 records per episode; policy 1600-64-64-32 + heads): profiles/r07_var_obs.jsonl.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--episodes", default="1024,65536")
    ap.add_argument("--out", default=None)
    ap.add_argument("--env", default="gridworld", choices=["gridworld", "lamps40"])
    args = ap.parse_args()
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.collector import CollectedData, _DeviceResult
    from tests.device_env_util import gridworld
    from tests.util import amd_policy, make_deep_policy_arrays
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.env == "lamps40":
        from tests.var_obs_util import lamps, lamps_policy_arrays
        env, pol = lamps(40), amd_policy(lamps_policy_arrays(40))
        env_name, pol_name = "Lamps40 (0..40 ids per state)", "1600-64-64-32+heads (generic)"
    else:
        env = gridworld(max_steps=64, difficulty=1, max_records=65)
        pol = amd_policy(make_deep_policy_arrays(25, seed=0, emb=512, common=(128,), n_actions=4))
        env_name, pol_name = "GridWorld5x5", "625-512-128+heads (generic)"
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))

    def host(E, seed):
        prm = _lib.PPOParams(E, 0, 0.995, 0.995, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
        out = C.c_void_p()
        _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), pol._handle(), C.byref(prm), env.max_records, C.byref(out)))
        return CollectedData._from_device(_DeviceResult(out.value))

    def device(E, seed):
        return twisterl.collector.PPOCollector(E, 0.995, 0.995, 32).collect(env, pol, seed=seed)

    rows = []
    info = twisterl_amd.device_info()
    for E in [int(x) for x in args.episodes.split(",")]:
        g, h = device(E, 1), host(E, 1)
        a, b = g.to_numpy(), h.to_numpy()
        assert all(a[k].tobytes() == b[k].tobytes() for k in a), "device and host collects differ"
        for path, fn in (("device", device), ("host_stepped", host)):
            for i in range(args.warmup):
                fn(E, 100 + i)
            ts, recs, roll = [], [], []
            for i in range(args.reps):
                t0 = time.perf_counter()
                c = fn(E, 1000 + i)
                n = len(c)
                ts.append(time.perf_counter() - t0)
                recs.append(n)
                roll.append(c.stats.get("ms_rollout", 0.0))
            k = int(np.argsort(ts)[len(ts) // 2])
            row = {"env": env_name, "policy": pol_name, "path": path, "episodes": E,
                   "records": recs[k], "wall_ms": round(ts[k] * 1e3, 3), "records_per_s": round(recs[k] / ts[k], 1),
                   "ms_rollout": round(roll[k], 3) if path == "device" else None, "reps": args.reps, "device": info["name"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
