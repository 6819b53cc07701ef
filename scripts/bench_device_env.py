"""Records/s of a user-written environment collected ON THE DEVICE (tw_ppo_collect_device_env) against the host-stepped path over
the same struct (tw_ppo_collect_env over the module's vtable): GridWorld 5 x 5 (examples/device_env/gridworld.hpp, max_steps 64)
with the policy shape of the reference's ppo_grid_world_5x5_v1.json (embedding 512, common [128], linear heads), at 1,024 and
65,536 episodes.  Wall clock of whole collect() calls (finalize and result included), median of --reps after --warmup; every
device collect is checked byte-equal to the host one first.

    python scripts/bench_device_env.py [--reps 5] [--out profiles/r05_device_env.jsonl]

--env lamps40: the same comparison for an environment whose observations vary in length (tests/device_envs/lamps.hpp with 40 lamps:
0 .. 40 ids per state, obs_size 1,600, at most 24 records per episode; policy 1600-64-64-32 + heads): profiles/r07_var_obs.jsonl.

--env perm8: an environment of MORE than four actions (examples/device_env/permutation.hpp with N = 8: 28 transpositions, 8 ids per
state, obs_size 64, max_steps 32, difficulty 4; a module built with wide=True; policy 64-512-128-64 + heads -- two common layers: with one of 128 units and an obs_size of at most 256 the policy has
the MFMA shape, which the device environments hand to the host-stepped path unless the module was built with basic=True -- see --basic): the same two kernels stream over the 28 actions.  profiles/r11_device_env_wide.jsonl.

--az: self-play instead.  Whole AZCollector.collect calls of GridWorld 5 x 5 with the same policy, --az-shape episodes x searches
(4096x100; if the first call takes more than a minute the run goes on at 1024x32 and says so), median of --reps: ONE row, whose
"path" is what the call ran on -- "device" when the library reports the module's search kernel (a module built with search=True),
else "host_stepped".  The comparison is this command on two trees: --tree names the checkout whose package, tests/ helpers and
built library are measured (default: the tree the script lies in); a tree from before the search kernel builds the plain module
and its collect is host-stepped.  profiles/r08_device_env_search.jsonl holds the two rows.  --az --env perm8: the same for the 28 actions of
Permutation8 with the policy of --env perm8 (a module built with wide_search=True; a tree from before the wide search builds it with
wide=True and its collect is host-stepped): profiles/r12_device_env_wide_search.jsonl.

--solve: collector.solve (best of N sampled attempts from the environment's CURRENT state, the action list back) of GridWorld 5 x 5 and
Permutation8, plain and with --solve-mcts searches per move, at --solve-searches 1,64,1024 attempts: the call as the tree runs it (one
kernel launch since tw_solve_device_env; host-stepped on a --tree from before it) and tw_solve_env32 over the module's host vtable, the
two results compared in the same run; wall clock of whole calls, median / min / max of --reps after --warmup, rows APPENDED to --out.
profiles/r13_device_env_solve.jsonl.

--no-persist: TW_OPT_NO_PERSIST = 1 for the whole run -- one workgroup per 16 episodes whatever their number, instead of the persistent
grid with its episode queue that a collect of more episodes than the chip holds columns gets by itself.  Every device row says which
of the two ran ("persist") and the grid ("blocks").  --skip-host leaves the host-stepped rows (and the byte comparison with them) out:
the A/B of two trees or two launch forms needs only the device rows.  profiles/r09_device_env_persist.jsonl.

--precision fp32,fp16 (--env gridworld or perm8): the device collect in each of the listed precisions FROM THE SAME MODULE, built with
fp16=True (rollout_env_kernel and rollout_env16_kernel side by side; fp16 has no host-stepped counterpart, so these runs are device
rows only).  --policy small: embedding 128, common [64] (perm8: [64, 64] -- with one common layer of 64 units and 64 obs ids the
policy has the MFMA shape, which device environments hand to the host-stepped path); --policy deep: embedding 256, common [512, 256].
Every row carries the rollout's milliseconds (the events around the launch: in fp16 the pack of the weight image and the rollout)
as median / min / max of --reps, and records per second of rollout time.  Rows are APPENDED to --out.
profiles/r16_device_env_fp16.jsonl.  With fp16x2 in the list (--precision fp32,fp16,fp16x2) the module is built with fp16x2=True
instead and holds rollout_env16x2_kernel as well (EngineV16x2: split binary16 operands, f32 answers); a --tree from before that flag
builds the fp16 module and gives the other rows.  profiles/r21_device_env_fp16x2.jsonl.

--evaluate (with --precision, --policy, --env gridworld or perm8 as above): collector.evaluate of --episodes episodes x 1 search,
deterministic and sampled, in each listed precision from ONE module built with fp16_solve=True (solve_env_kernel and solve_env16_kernel
side by side).  evaluate returns two means and no statistics, so a row carries the WHOLE CALL (checks, the image's pack in fp16, the
kernel, the copies back, the reduction on the host) as median / min / max of --reps after --warmup, and the two means.  A --tree from
before the keyword builds the plain module and gives the fp32 rows only: the parent's figures of the same session.
profiles/r17_device_env_fp16_solve.jsonl.  With fp16x2 in the list (--precision fp32,fp16,fp16x2) the module is built with
fp16_solve=True, fp16x2_solve=True and holds solve_env16x2_kernel as well (EngineV16x2: split binary16 operands, f32 answers); a --tree
from before that flag builds the module it can and gives the rows it has.  profiles/r22_device_env_fp16x2_solve.jsonl.

--az and the MCTS shapes of --solve with --precision fp32,fp16 (and --policy default | deep): each listed precision from ONE module
built with fp16_search=True (mcts_env_kernel and mcts_env16_kernel side by side; name + _f16), whole calls, median / min / max of --reps,
rows APPENDED to --out with their "precision".  fp16 has no host-stepped counterpart: the fp16 rows of --solve are device rows only.  A
--tree from before the flag builds the plain search module and gives the fp32 rows only: the parent's figures of the same session.
profiles/r20_device_env_fp16_search.jsonl.

--basic: the reference's DEFAULT policy shape -- embedding 256 -> ONE common layer of 256 units -> linear heads, the "MFMA shape" that a
device environment with at most 256 obs ids used to hand to the host-stepped path -- on GridWorld 3 x 3 (obs_size 81, max_steps 64) and
Permutation8 (obs_size 64, 28 actions, max_steps 32), PPO collect of --episodes episodes from ONE module per environment built with
basic=True: (a) the call as the tree runs it, in rollout_env_kernel behind pack_basic_view_kernel; (b) tw_ppo_collect_env over the
module's host vtable, which is what the call ran on before the flag (byte-compared with (a) first); (c) the same module under
common=(48,), the one-common-layer policy that is NOT the MFMA shape and that the other rows of this script's family use.  Whole calls,
median / min / max of --reps after --warmup; the device rows also carry the rollout's milliseconds (the events around the module's
launcher: in (a) the pack and the rollout).  Rows are APPENDED to --out.  profiles/r23_device_env_basic.jsonl.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)


def az(args):
    """One row: AZCollector.collect of GridWorld 5 x 5 (--env perm8: of the 28-action Permutation8) on the path this tree takes for it."""
    import inspect
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    from tests.device_env_util import GRIDWORLD_HPP
    from tests.util import amd_policy, make_deep_policy_arrays
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    params = inspect.signature(build_device_env).parameters
    # --precision: every listed precision from one module built with fp16_search=True (a tree from before the flag: the plain search
    # module, fp32 only)
    f16 = {"fp16_search": True} if args.precision and "fp16_search" in params else {}
    precs = [p for p in (args.precision or "fp32").split(",") if p == "fp32" or f16]
    suffix = "_f16" if f16 else ""
    if args.env == "perm8":
        # 28 actions: the search kernel takes them in a module built with wide_search=True; a tree from before that builds the wide
        # module without the search kernel and its collect is host-stepped
        from tests.util import make_deep_policy_arrays_obs
        can_search = "wide_search" in params
        name = ("perm8_az" if can_search else "perm8") + suffix
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "permutation.hpp"), "tw_examples::Permutation8", name,
                              **({"wide_search": True} if can_search else {"wide": True}), **f16)
        env = DeviceEnv(so, name, [8, 32, 4], max_records=33)
        emb, common = {"default": (512, (128, 64)), "small": (128, (64, 64)), "deep": (256, (512, 256))}[args.policy]
        pol = amd_policy(make_deep_policy_arrays_obs(64, seed=0, emb=emb, common=common, n_actions=28))
        env_name, pol_name = "Permutation8 (28 actions)", "-".join(str(x) for x in (64, emb) + tuple(common)) + "+heads (generic)"
    elif args.env != "gridworld":
        raise SystemExit("--az: --env gridworld or perm8")
    else:
        can_search = "search" in params
        name = ("gridworld5x5_az" if can_search else "gridworld5x5") + suffix
        so = build_device_env(GRIDWORLD_HPP, "tw_examples::GridWorld5x5", name, **({"search": True} if can_search else {}), **f16)
        env = DeviceEnv(so, name, [5, 5, 64, 1], max_records=65)
        emb, common = {"default": (512, (128,)), "small": (128, (64,)), "deep": (256, (512, 256))}[args.policy]
        pol = amd_policy(make_deep_policy_arrays(25, seed=0, emb=emb, common=common, n_actions=4))
        env_name, pol_name = "GridWorld5x5", "-".join(str(x) for x in (625, emb) + tuple(common)) + "+heads (generic)"
    E, S = (int(x) for x in args.az_shape.lower().split("x"))
    for prec in precs:
        az_rows(args, env, pol, env_name, pol_name, E, S, prec if args.precision else None)


def az_rows(args, env, pol, env_name, pol_name, E, S, prec):
    """The row of one precision (None: the collector's default, for a tree from before the keyword reached the device)."""
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl

    def collect(seed):
        t0 = time.perf_counter()
        c = twisterl.collector.AZCollector(E, S, 1.41, 1, 32, **({"precision": prec} if prec else {})).collect(env, pol, seed=seed)
        n = len(c)
        return time.perf_counter() - t0, n, c.stats

    fell_back = False
    t, _, _ = collect(100)                                                   # warm-up; also decides the shape
    if t > 60.0 and (E, S) != (1024, 32):
        E, S, fell_back = 1024, 32, True
        collect(100)
    for i in range(1, args.warmup):
        collect(100 + i)
    runs = [collect(1000 + i) for i in range(args.reps)]
    k = int(np.argsort([r[0] for r in runs])[len(runs) // 2])
    t, n, stats = runs[k]
    on_device = _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_MCTS_BIG
    if prec:
        assert on_device and _lib.debug_last_launch()["nw"] == (16 if prec == "fp16" else 0), _lib.debug_last_launch()
    evals = int(stats.get("forward_evals", 0)) if on_device else None
    row = {"bench": "az", "env": env_name, "policy": pol_name, "path": "device" if on_device else "host_stepped",
           "episodes": E, "num_mcts_searches": S, "max_expand_depth": 1, "shape_fell_back": fell_back, "records": n,
           "wall_ms": round(t * 1e3, 3), "records_per_s": round(n / t, 1),
           "ms_rollout": round(float(stats.get("ms_rollout", 0.0)), 3) if on_device else None,
           "evaluations": evals, "evaluations_per_s": round(evals / t, 1) if evals else None,
           "persist": _lib.debug_last_launch()["persist"] if on_device else None, "blocks": _lib.debug_last_launch()["blocks"] if on_device else None,
           "wall_ms_all": [round(r[0] * 1e3, 3) for r in runs],
           "reps": args.reps, "device": twisterl_amd.device_info()["name"]}
    if prec:
        row.update(precision=prec, wall_ms_min=round(min(r[0] for r in runs) * 1e3, 3), wall_ms_max=round(max(r[0] for r in runs) * 1e3, 3),
                   tree=os.path.basename(ROOT) if args.tree else "this")
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


def solve(args):
    """collector.solve of GridWorld 5 x 5 and Permutation8 from a state one step behind a reset, plain and with MCTS (--solve-mcts searches
    per move, expansion depth 1), best of 1 / 64 / 1024 sampled attempts: the call as this tree runs it ("device" when the library reports
    a kernel of the module, else "host_stepped") against tw_solve_env32 over the module's host vtable, whose result must be the same."""
    import inspect
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    from tests.device_env_util import GRIDWORLD_HPP
    from tests.util import amd_policy, make_deep_policy_arrays, make_deep_policy_arrays_obs
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    params = inspect.signature(build_device_env).parameters
    perm_hpp = os.path.join(ROOT, "examples", "device_env", "permutation.hpp")
    grid_pol = amd_policy(make_deep_policy_arrays(25, seed=0, emb=512, common=(128,), n_actions=4))
    perm_pol = amd_policy(make_deep_policy_arrays_obs(64, seed=0, emb=512, common=(128, 64), n_actions=28))

    # --precision: the MCTS shapes in every listed precision from one module built with fp16_search=True
    f16 = {"fp16_search": True} if args.precision and "fp16_search" in params else {}
    precs = [p for p in (args.precision or "fp32").split(",") if p == "fp32" or f16]

    def grid(search):
        name = ("gridworld5x5_az" + ("_f16" if f16 else "")) if search else "gridworld5x5"
        so = build_device_env(GRIDWORLD_HPP, "tw_examples::GridWorld5x5", name, **({"search": True, **f16} if search else {}))
        return DeviceEnv(so, name, [5, 5, 64, 8], max_records=65)

    def perm(search):
        name = ("perm8_az" + ("_f16" if f16 else "")) if search else "perm8"
        so = build_device_env(perm_hpp, "tw_examples::Permutation8", name, **({"wide_search": True, **f16} if search else {"wide": True}))
        return DeviceEnv(so, name, [8, 32, 4], max_records=33)

    S = args.solve_mcts
    shapes = [("GridWorld5x5", "625-512-128+heads (generic)", grid, grid_pol, 0), ("GridWorld5x5", "625-512-128+heads (generic)", grid, grid_pol, S),
              ("Permutation8 (28 actions)", "64-512-128-64+heads (generic)", perm, perm_pol, 0),
              ("Permutation8 (28 actions)", "64-512-128-64+heads (generic)", perm, perm_pol, S)]
    info = twisterl_amd.device_info()
    rows = []
    for env_name, pol_name, make, pol, mcts in shapes:
        if mcts and ("wide_search" not in params or "search" not in params):
            continue
        env = make(mcts > 0)
        env.reset(seed=3, episode=5)
        env.step(next(i for i, m in enumerate(env.masks()) if m))       # the current state is no reset state
        vt = _lib.EnvVTable()
        _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))

        def call(N, seed, prec=None):
            return twisterl.collector.solve(env, pol, False, N, mcts, 1.41, 1, seed=seed, **({"precision": prec} if prec else {}))

        def host(N, seed):
            prm = _lib.SolveParams(0, N, mcts, 1.41, 1, seed, _lib.TW_PREC_F32_EXACT)
            cap = env.max_records + 1
            acts = (C.c_uint32 * cap)()
            s, r, n = C.c_float(), C.c_float(), C.c_uint32()
            _lib.check(_lib.lib().tw_solve_env32(C.byref(vt), pol._handle(), C.byref(prm), env.max_records, C.byref(s), C.byref(r), acts, cap, C.byref(n)))
            return (float(s.value), float(r.value)), [int(acts[i]) for i in range(n.value)]

        for N in [int(x) for x in args.solve_searches.split(",")]:
            a, b = call(N, 1), host(N, 1)
            same = a[0][0] == b[0][0] and np.float32(a[0][1]).tobytes() == np.float32(b[0][1]).tobytes() and a[1] == b[1]
            assert same, f"solve() and the host-stepped path differ: {a} {b}"
            last = _lib.debug_last_launch()
            on_device = last["family"] in (_lib.TW_KERNEL_SOLVE_BIG, _lib.TW_KERNEL_MCTS_BIG)
            for path, fn in ((("device" if on_device else "host_stepped"), call),) + ((("host_stepped", host),) if on_device and not args.skip_host else ()):
                for i in range(args.warmup):
                    fn(N, 100 + i)
                ts = []
                for i in range(args.reps):
                    t0 = time.perf_counter()
                    fn(N, 1000 + i)
                    ts.append(time.perf_counter() - t0)
                ts_ms = sorted(t * 1e3 for t in ts)
                row = {"bench": "solve", "env": env_name, "policy": pol_name, "path": path, "entry": "collector.solve" if fn is call else "tw_solve_env32",
                       "num_searches": N, "num_mcts_searches": mcts, "max_expand_depth": 1, "deterministic": False, "same_result_as_host_stepped": same,
                       "wall_ms": round(ts_ms[len(ts_ms) // 2], 3), "wall_ms_min": round(ts_ms[0], 3), "wall_ms_max": round(ts_ms[-1], 3),
                       "wall_ms_all": [round(t * 1e3, 3) for t in ts], "reps": args.reps,
                       "persist": last["persist"] if fn is call and on_device else None, "blocks": last["blocks"] if fn is call and on_device else None,
                       "tree": os.path.basename(ROOT) if args.tree else "this", "device": info["name"]}
                if args.precision:
                    row.update(precision="fp32")
                rows.append(row)
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")
            if mcts and "fp16" in precs:
                # the f16 search kernel of the same module: device rows only (the host-stepped path is f32)
                for i in range(args.warmup):
                    call(N, 100 + i, "fp16")
                ts = []
                for i in range(args.reps):
                    t0 = time.perf_counter()
                    call(N, 1000 + i, "fp16")
                    ts.append(time.perf_counter() - t0)
                last = _lib.debug_last_launch()
                assert (last["family"], last["nw"]) == (_lib.TW_KERNEL_MCTS_BIG, 16), last
                ts_ms = sorted(t * 1e3 for t in ts)
                row = {"bench": "solve", "env": env_name, "policy": pol_name, "path": "device", "entry": "collector.solve", "precision": "fp16",
                       "num_searches": N, "num_mcts_searches": mcts, "max_expand_depth": 1, "deterministic": False, "same_result_as_host_stepped": None,
                       "wall_ms": round(ts_ms[len(ts_ms) // 2], 3), "wall_ms_min": round(ts_ms[0], 3), "wall_ms_max": round(ts_ms[-1], 3),
                       "wall_ms_all": [round(t * 1e3, 3) for t in ts], "reps": args.reps, "persist": last["persist"], "blocks": last["blocks"],
                       "tree": os.path.basename(ROOT) if args.tree else "this", "device": info["name"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")


def precisions(args):
    """PPO collect on the device in fp32 and fp16 from ONE module built with fp16=True: rollout milliseconds, their spread, records/s."""
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    from tests.util import amd_policy, make_deep_policy_arrays_obs
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    # (--tree of a checkout from before the fp16 form: the plain module, fp32 rows only -- the parent's figure of the same run)
    import inspect
    params = inspect.signature(build_device_env).parameters
    fp16 = {"fp16": True} if "fp16" in params else {}
    split = "fp16x2" in args.precision.split(",") and "fp16x2" in params        # the split kernel beside the other two, in one module
    if split:
        fp16 = {"fp16x2": True}
    suffix = "_fp16x2" if split else "_fp16"
    if args.env == "perm8":
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "permutation.hpp"), "tw_examples::Permutation8", "perm8" + suffix, wide=True, **fp16)
        env = DeviceEnv(so, "perm8" + suffix, [8, 32, 4], max_records=33)
        env_name, obs_size, A = "Permutation8 (28 actions)", 64, 28
        emb, common = {"default": (512, (128, 64)), "small": (128, (64, 64)), "deep": (256, (512, 256))}[args.policy]
    elif args.env == "gridworld":
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "gridworld.hpp"), "tw_examples::GridWorld5x5", "gridworld5x5" + suffix, **fp16)
        env = DeviceEnv(so, "gridworld5x5" + suffix, [5, 5, 64, 1], max_records=65)
        env_name, obs_size, A = "GridWorld5x5", 625, 4
        emb, common = {"default": (512, (128,)), "small": (128, (64,)), "deep": (256, (512, 256))}[args.policy]
    else:
        raise SystemExit("--precision: --env gridworld or perm8")
    pol = amd_policy(make_deep_policy_arrays_obs(obs_size, seed=0, emb=emb, common=common, n_actions=A))
    pol_name = "-".join(str(x) for x in (obs_size, emb) + tuple(common)) + "+heads (generic)"
    info = twisterl_amd.device_info()
    for E in [int(x) for x in args.episodes.split(",")]:
        for prec in args.precision.split(","):
            if (prec != "fp32" and not fp16) or (prec == "fp16x2" and not split):
                continue
            fn = lambda seed: twisterl.collector.PPOCollector(E, 0.995, 0.995, 32, precision=prec).collect(env, pol, seed=seed)
            for i in range(args.warmup):
                fn(100 + i)
            ts, recs, roll = [], [], []
            for i in range(args.reps):
                t0 = time.perf_counter()
                c = fn(1000 + i)
                n = len(c)
                ts.append(time.perf_counter() - t0)
                recs.append(n)
                roll.append(float(c.stats.get("ms_rollout", 0.0)))
            last = _lib.debug_last_launch()
            assert (last["family"], last["nw"]) == (_lib.TW_KERNEL_ROLLOUT_BIG, {"fp16": 16, "fp16x2": 32}.get(prec, 0)), last
            k = int(np.argsort(roll)[len(roll) // 2])
            row = {"bench": "precision", "env": env_name, "policy": pol_name, "precision": prec, "path": "device", "episodes": E, "records": recs[k],
                   "ms_rollout": round(roll[k], 3), "ms_rollout_min": round(min(roll), 3), "ms_rollout_max": round(max(roll), 3),
                   "records_per_s_rollout": round(recs[k] / (roll[k] * 1e-3), 1), "wall_ms": round(float(np.median(ts)) * 1e3, 3),
                   "ms_rollout_all": [round(x, 3) for x in roll], "persist": last["persist"], "blocks": last["blocks"],
                   "reps": args.reps, "warmup": args.warmup, "tree": os.path.basename(ROOT) if args.tree else "this", "device": info["name"]}
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")


def evaluate_bench(args):
    """collector.evaluate on the device in fp32, fp16 (and fp16x2) from ONE module built with fp16_solve=True (and fp16x2_solve=True):
    whole-call milliseconds, their spread."""
    import inspect
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    from tests.util import amd_policy, make_deep_policy_arrays_obs
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    # (--tree of a checkout from before the fp16_solve form: the plain module, fp32 rows only)
    has16 = "fp16_solve" in inspect.signature(build_device_env).parameters
    kw, suffix = ({"fp16_solve": True}, "_fp16s") if has16 else ({}, "")
    # fp16x2 in the list: the split evaluate kernel beside the other two, in one module (a tree from before the flag: the rows it has)
    split = "fp16x2" in (args.precision or "").split(",") and "fp16x2_solve" in inspect.signature(build_device_env).parameters
    if split:
        kw, suffix = {"fp16_solve": True, "fp16x2_solve": True}, "_fp16s_x2s"
    if args.env == "perm8":
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "permutation.hpp"), "tw_examples::Permutation8", "perm8" + suffix, wide=True, **kw)
        env = DeviceEnv(so, "perm8" + suffix, [8, 32, 4], max_records=33)
        env_name, obs_size, A = "Permutation8 (28 actions)", 64, 28
        emb, common = {"default": (512, (128, 64)), "small": (128, (64, 64)), "deep": (256, (512, 256))}[args.policy]
    elif args.env == "gridworld":
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "gridworld.hpp"), "tw_examples::GridWorld5x5", "gridworld5x5" + suffix, **kw)
        env = DeviceEnv(so, "gridworld5x5" + suffix, [5, 5, 64, 1], max_records=65)
        env_name, obs_size, A = "GridWorld5x5", 625, 4
        emb, common = {"default": (512, (128,)), "small": (128, (64,)), "deep": (256, (512, 256))}[args.policy]
    else:
        raise SystemExit("--evaluate: --env gridworld or perm8")
    pol = amd_policy(make_deep_policy_arrays_obs(obs_size, seed=0, emb=emb, common=common, n_actions=A))
    pol_name = "-".join(str(x) for x in (obs_size, emb) + tuple(common)) + "+heads (generic)"
    info = twisterl_amd.device_info()
    for E in [int(x) for x in args.episodes.split(",")]:
        for prec in (args.precision or "fp32").split(","):
            if (prec != "fp32" and not has16) or (prec == "fp16x2" and not split):
                continue
            for det in (True, False):
                pkw = {"precision": prec} if has16 else {}
                fn = lambda seed: twisterl.collector.evaluate(env, pol, E, det, 1, 0, seed, 1.41, 1, 1, **pkw)
                for i in range(args.warmup):
                    fn(100 + i)
                ts, res = [], None
                for i in range(args.reps):
                    t0 = time.perf_counter()
                    res = fn(1000 + i)
                    ts.append((time.perf_counter() - t0) * 1e3)
                last = _lib.debug_last_launch()
                assert (last["family"], last["nw"]) == (_lib.TW_KERNEL_SOLVE_BIG, {"fp16": 16, "fp16x2": 32}.get(prec, 0)), last
                row = {"bench": "evaluate", "env": env_name, "policy": pol_name, "precision": prec, "deterministic": det, "path": "device",
                       "episodes": E, "searches": 1, "wall_ms": round(float(np.median(ts)), 3), "wall_ms_min": round(min(ts), 3),
                       "wall_ms_max": round(max(ts), 3), "wall_ms_all": [round(t, 3) for t in ts], "success_rate": res[0], "mean_reward": res[1],
                       "persist": last["persist"], "blocks": last["blocks"], "reps": args.reps, "warmup": args.warmup,
                       "tree": os.path.basename(ROOT) if args.tree else "this", "device": info["name"]}
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")


def basic_bench(args):
    """PPO collect of GridWorld 3 x 3 and Permutation8 under the one-common-layer policy 256 -> 256, from a module built with basic=True:
    device, host-stepped, and the same module under common=(48,)."""
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.build import build_device_env
    from twisterl_amd.collector import CollectedData, _DeviceResult
    from twisterl_amd.env import DeviceEnv
    from tests.util import amd_policy, make_deep_policy_arrays_obs, make_policy_arrays_obs
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    info = twisterl_amd.device_info()
    grid = (os.path.join(ROOT, "examples", "device_env", "gridworld.hpp"), "tw_examples::GridWorld3x3", "gridworld3x3_basic", {}, [3, 3, 64, 1], 65,
            "GridWorld3x3", 81, 4)
    perm = (os.path.join(ROOT, "examples", "device_env", "permutation.hpp"), "tw_examples::Permutation8", "perm8_basic", {"wide": True}, [8, 32, 4], 33,
            "Permutation8 (28 actions)", 64, 28)
    for header, type_, name, kw, params, max_records, env_name, obs_size, A in (grid, perm):
        env = DeviceEnv(build_device_env(header, type_, name, basic=True, **kw), name, params, max_records=max_records)
        assert env.basic
        vt = _lib.EnvVTable()
        _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
        basic = amd_policy(make_policy_arrays_obs(obs_size, seed=0, emb=256, hidden=256, n_actions=A))
        c48 = amd_policy(make_deep_policy_arrays_obs(obs_size, seed=0, emb=256, common=(48,), n_actions=A))

        def device(pol, E, seed):
            return twisterl.collector.PPOCollector(E, 0.995, 0.995, 32).collect(env, pol, seed=seed)

        def host(pol, E, seed):
            prm = _lib.PPOParams(E, 0, 0.995, 0.995, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
            out = C.c_void_p()
            _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), pol._handle(), C.byref(prm), env.max_records, C.byref(out)))
            return CollectedData._from_device(_DeviceResult(out.value))

        for E in [int(x) for x in args.episodes.split(",")]:
            if not args.skip_host:
                a, b = device(basic, E, 1).to_numpy(), host(basic, E, 1).to_numpy()
                assert all(a[k].tobytes() == b[k].tobytes() for k in a), "device and host collects differ"
            runs = [("device", "basic=True", basic, device, f"{obs_size}-256-256+heads (one common layer: the MFMA shape)")]
            if not args.skip_host:
                runs.append(("host_stepped", "tw_ppo_collect_env", basic, host, f"{obs_size}-256-256+heads (one common layer: the MFMA shape)"))
            runs.append(("device", "common=(48,)", c48, device, f"{obs_size}-256-48+heads (generic)"))
            for path, what, pol, fn, pol_name in runs:
                for i in range(args.warmup):
                    fn(pol, E, 100 + i)
                ts, recs, roll = [], [], []
                for i in range(args.reps):
                    t0 = time.perf_counter()
                    c = fn(pol, E, 1000 + i)
                    n = len(c)
                    ts.append((time.perf_counter() - t0) * 1e3)
                    recs.append(n)
                    roll.append(float(c.stats.get("ms_rollout", 0.0)))
                k = int(np.argsort(ts)[len(ts) // 2])
                row = {"bench": "basic", "env": env_name, "policy": pol_name, "path": path, "what": what, "episodes": E, "records": recs[k],
                       "wall_ms": round(ts[k], 3), "wall_ms_min": round(min(ts), 3), "wall_ms_max": round(max(ts), 3),
                       "records_per_s": round(recs[k] / (ts[k] * 1e-3), 1), "wall_ms_all": [round(t, 3) for t in ts],
                       "ms_rollout": round(roll[k], 3) if path == "device" else None, "reps": args.reps, "warmup": args.warmup, "device": info["name"]}
                if path == "device":
                    last = _lib.debug_last_launch()
                    assert last["family"] == _lib.TW_KERNEL_ROLLOUT_BIG, f"the device rows did not run the module's kernel: {last}"
                    row.update(persist=last["persist"], blocks=last["blocks"])
                print(json.dumps(row), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solve", action="store_true", help="collector.solve from the current state against the host-stepped path; appends rows to --out")
    ap.add_argument("--solve-searches", default="1,64,1024", help="num_searches of --solve")
    ap.add_argument("--solve-mcts", type=int, default=8, help="num_mcts_searches of the MCTS shapes of --solve")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--episodes", default="1024,65536")
    ap.add_argument("--out", default=None)
    ap.add_argument("--env", default="gridworld", choices=["gridworld", "lamps40", "perm8"])
    ap.add_argument("--az", action="store_true", help="self-play (AZCollector.collect) instead of the PPO collect; appends one row to --out")
    ap.add_argument("--az-shape", default="4096x100", help="episodes x num_mcts_searches of --az")
    ap.add_argument("--tree", default=None, help="the checkout to measure (default: this one)")
    ap.add_argument("--no-persist", action="store_true", help="TW_OPT_NO_PERSIST = 1: never the persistent grid + episode queue")
    ap.add_argument("--skip-host", action="store_true", help="device rows only (no host-stepped rows, no byte comparison with them)")
    ap.add_argument("--precision", default=None, help="fp32,fp16[,fp16x2]: device rows in these precisions from one module built with fp16=True (fp16x2=True); appends to --out")
    ap.add_argument("--policy", default="default", choices=["default", "small", "deep"], help="with --precision: the policy's widths")
    ap.add_argument("--evaluate", action="store_true", help="collector.evaluate (episodes x 1 search) instead of the PPO collect, in the precisions of --precision; appends to --out")
    ap.add_argument("--basic", action="store_true", help="the one-common-layer policy 256 -> 256 from a module built with basic=True: device, host-stepped, and common=(48,); appends to --out")
    args = ap.parse_args()
    if args.basic:
        return basic_bench(args)
    if args.evaluate:
        return evaluate_bench(args)
    if args.az:
        return az(args)
    if args.solve:
        return solve(args)
    if args.precision:
        return precisions(args)
    import numpy as np
    import twisterl_amd
    from twisterl_amd import _lib, twisterl
    from twisterl_amd.collector import CollectedData, _DeviceResult
    from tests.device_env_util import gridworld
    from tests.util import amd_policy, make_deep_policy_arrays
    if twisterl_amd.device_count() < 1:
        raise SystemExit("no GPU")
    if args.no_persist:
        _lib.check(_lib.lib().tw_set_launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    if args.env == "lamps40":
        from tests.var_obs_util import lamps, lamps_policy_arrays
        env, pol = lamps(40), amd_policy(lamps_policy_arrays(40))
        env_name, pol_name = "Lamps40 (0..40 ids per state)", "1600-64-64-32+heads (generic)"
    elif args.env == "perm8":
        from twisterl_amd.build import build_device_env
        from twisterl_amd.env import DeviceEnv
        from tests.util import make_deep_policy_arrays_obs
        so = build_device_env(os.path.join(ROOT, "examples", "device_env", "permutation.hpp"), "tw_examples::Permutation8", "perm8", wide=True)
        env = DeviceEnv(so, "perm8", [8, 32, 4], max_records=33)
        pol = amd_policy(make_deep_policy_arrays_obs(64, seed=0, emb=512, common=(128, 64), n_actions=28))
        env_name, pol_name = "Permutation8 (28 actions)", "64-512-128-64+heads (generic)"
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
        if not args.skip_host:
            g, h = device(E, 1), host(E, 1)
            a, b = g.to_numpy(), h.to_numpy()
            assert all(a[k].tobytes() == b[k].tobytes() for k in a), "device and host collects differ"
        for path, fn in (("device", device),) + (() if args.skip_host else (("host_stepped", host),)):
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
            if path == "device":
                last = _lib.debug_last_launch()
                assert last["family"] == _lib.TW_KERNEL_ROLLOUT_BIG, f"the device rows did not run the module's kernel: {last}"
                row.update(persist=last.get("persist"), blocks=last.get("blocks"), wall_ms_all=[round(t * 1e3, 3) for t in ts])
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
