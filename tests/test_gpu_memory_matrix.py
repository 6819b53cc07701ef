"""GPU: no result depends on what device memory held before the call -- every case of tests/memory_matrix.py, four times.

The library clears none of its buffers (cached workspace, pooled result arenas, call-local scratch); the other GPU tests run on
whatever those happen to hold, which on a fresh process is mostly zeros.  Here the test hook tw_debug_fill_memory sets every buffer
the library hands to a call to a 32-bit pattern, over its whole capacity, before the call's first use of it.  Per case, with the same
collect seed throughout:

  a  hook on, 0xFFFFFFFF, policy P2: the EXISTING check of the row the case points to, unchanged in what it asserts (launch shape held
     to the row, the result bit for bit against the oracle -- the f16 modes against the replay and the float64 bounds --, every attempt
     of an evaluate / solve), run by the helper of the test file that owns the row;
  b  hook on, 0x00000001, P2;
  c  hook on, 0x00000000, P2;
  d  hook off: the identical call with P1 (the same shapes, other weights) first, its result freed so that its arena goes back to the
     pool, then P2 on P1's leftovers -- workspace, arena and scratch as the previous collect under older weights left them, which is
     what a training loop hands the next collect.

b, c and d must equal a BYTE FOR BYTE: every field the front end exposes (ep_len and ep_start among them), the bytes of the result's
arena inside the fields (tw_debug_collected_arena), the launch shape and the counts that come from device counters (reused_evals,
forward_evals, the hand-over counters of tw_debug_counters; the range fall-back shows in the launch shape) -- the counts only where they
do not depend on which persistent lane took which episode off the queue (tests/memory_matrix.py `counters`).  In a, b and c every byte
of the arena outside the fields (and outside the finalize kernel's four-column scratch behind them) must still hold the pattern:
nothing may write there.  For evaluate / solve the attempts (tw_debug_last_attempts), the two results and the action list are compared.
Byte equality and three fixed patterns: there is no tolerance here.
"""
import contextlib
import signal

import numpy as np
import pytest

from tests import memory_matrix as mm
from tests.util import amd_policy, f32_bits, oracle_policy
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

COUNT_STATS = ("forward_evals", "speculative_evals", "reused_evals")
SHAPE_STATS = ("records", "episodes", "padded_bytes", "rollout_blocks", "rollout_threads")
P1_SEED = 9001            # the other weights of run d: a seed no table uses
HOOK_AT_START = _lib.debug_fill_memory._current()


@pytest.fixture(scope="module", autouse=True)
def device():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    yield
    _lib.release_cached_memory()


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code; a hang inside a HIP call is bounded by the `timeout`
    around the pytest run."""
    def boom(*_):
        raise TimeoutError("memory matrix case exceeded its time limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(240)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


# ------------------------------------------------------------------------------------------ snapshots
def pattern_bytes(pattern, n):
    """The n bytes a buffer filled with the 32-bit pattern holds (little-endian words from offset 0)."""
    return np.tile(np.frombuffer(np.uint32(pattern).tobytes(), dtype=np.uint8), (n + 3) // 4)[:n]


_before_snapshot = []


@contextlib.contextmanager
def before_snapshot(hook):
    """While the block runs, hook(g) sees every collect's result before snap_collected's first read of it.  The family runners build
    their snapshots inside closures, so a driver that has to look at a result first (tests/test_gpu_stream_matrix.py, run d) says so
    here instead of every runner passing an argument through."""
    _before_snapshot.append(hook)
    try:
        yield
    finally:
        _before_snapshot.remove(hook)


def snap_collected(g, pattern, counters=True, extra=None):
    """Everything a collect returned, as bytes: the front end's arrays, the arena's bytes inside the fields, the launch shape and (where
    `counters`) the counts.  With a pattern: the arena outside the fields and the four-column scratch must still hold it."""
    for hook in _before_snapshot:
        hook(g)
    dev = g._dev
    snap = {}
    for name, arr in g.to_numpy().items():
        snap["field:" + name] = (str(arr.dtype), arr.shape, arr.tobytes())
    arena, offs, scratch = _lib.debug_collected_arena(dev.h)
    outside = np.ones(arena.size, dtype=bool)
    for f in range(_lib.TW_F_COUNT):
        _, nbytes = dev.ptr(f)
        if nbytes:
            assert offs[f] + nbytes <= arena.size and outside[offs[f]:offs[f] + nbytes].all(), f
            snap[f"arena:{f}"] = arena[offs[f]:offs[f] + nbytes].tobytes()
            outside[offs[f]:offs[f] + nbytes] = False
    outside[scratch[0]:scratch[0] + scratch[1]] = False
    if pattern is not None:
        touched = np.flatnonzero((arena != pattern_bytes(pattern, arena.size)) & outside)
        assert touched.size == 0, (f"{touched.size} bytes of the arena outside the fields do not hold the fill {pattern:#010x}: the first at offset "
                                   f"{int(touched[0])} of {arena.size} holds {arena[touched[0]]:#04x}")
    snap["meta"] = (dev.n, dev.n_episodes, dev.n_cells, dev.n_actions, dev.is_ppo, dev.obs_width, dev.ragged)
    st = g.stats
    snap["shape"] = tuple(st[k] for k in SHAPE_STATS)
    if counters:
        snap["counts"] = tuple(st[k] for k in COUNT_STATS)
    if extra is not None:
        snap["extra"] = extra
    return snap


def snap_attempts(result, actions=None):
    """An evaluate's / solve's outcome: the two numbers as bits, the action list, every attempt (tw_debug_last_attempts)."""
    s, t, n = _lib.debug_last_attempts()
    return {"result": (f32_bits(np.float32(result[0])).tobytes(), f32_bits(np.float32(result[1])).tobytes()),
            "actions": None if actions is None else tuple(int(a) for a in actions),
            "attempts": (s.tobytes(), t.tobytes(), n.tobytes())}


def snap_tensors(tensors):
    return {f"tensor:{i}": (str(t.dtype), tuple(t.shape), t.detach().cpu().numpy().tobytes()) for i, t in enumerate(tensors)}


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        if a[k] != b[k]:
            x, y = a[k], b[k]
            where = ""
            if isinstance(x, tuple) and len(x) == 3 and isinstance(x[2], bytes) and len(x[2]) == len(y[2]):
                d = np.flatnonzero(np.frombuffer(x[2], np.uint8) != np.frombuffer(y[2], np.uint8))
                where = f": {d.size} of {len(x[2])} bytes differ, the first at byte {int(d[0])}" if d.size else f": {x[:2]} / {y[:2]}"
            elif isinstance(x, bytes) and len(x) == len(y):
                d = np.flatnonzero(np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8))
                where = f": {d.size} of {len(x)} bytes differ, the first at byte {int(d[0])}"
            elif not isinstance(x, (bytes, dict)) and len(repr(x)) < 400:
                where = f": {x!r} / {y!r}"
            raise AssertionError(f"{what}: {k} differs from the run under the fill 0xffffffff{where}")


def four_runs(case, check, call, leftovers=None):
    """check(pattern) -> the snapshot of run a (the row's own check, under the first fill); call(policy, pattern) -> a snapshot of the
    plain call with policy "P2" (the case's) or "P1" (other weights; run d's first call, whose result is dropped before P2 runs).
    This is the driver of this file; every family runner takes another one as its `driver` argument (tests/test_gpu_stream_matrix.py
    runs the same families, with the same assertions, on a caller's stream)."""
    p_a, p_b, p_c = mm.PATTERNS
    with _lib.debug_fill_memory(p_a):
        a = check(p_a)
        again = call("P2", p_a)                  # the plain call the other runs use returns what the checked call returned
    assert_same(a, again, f"{case.id}: the plain call under 0xffffffff")
    for p in (p_b, p_c):
        with _lib.debug_fill_memory(p):
            assert_same(a, call("P2", p), f"{case.id}: fill {p:#010x}")
    assert _lib.debug_fill_memory._current() == HOOK_AT_START             # (off, unless TW_DEBUG_FILL had it on for the whole process)
    first = (leftovers or call)("P1", None)
    if "field:logits" in first and "field:logits" in a:
        assert first["field:logits"] != a["field:logits"], f"{case.id}: the other weights gave the same logits"
    del first
    assert_same(a, call("P2", None), f"{case.id}: hook off, on the leftovers of the same call under other weights")


# ------------------------------------------------------------------------------------------ families
def fam_tail(case, tw, oracle, cus, driver=None):
    """tw_debug_collect_tail: tests/test_gpu_finalize.py's check compares every field with the numpy reference as bits and the gaps with
    the hook's own arena fill (which follows the pool's), so every pass of it is a result equal to one reference; the snapshot the
    driver compares is that reference."""
    from tests import finalize_matrix as fm
    from tests.test_gpu_finalize import _check
    fc = case.ref
    assert fc.values == "normal"                  # (no NaN anywhere: the check's one relaxation is never used)
    other = (fm._ppo(fm.E0 + 3, fc.t_pad + 1, n_cells=fc.n_cells, ids=fc.ids, A=fc.A) if fc.kind == "ppo" else
             fm._az(fm.E0 + 3, fc.t_pad + 1, n_cells=fc.n_cells, ids=fc.ids, A=fc.A))              # other records: what run d leaves behind
    snap = lambda ref: {"ref:" + k: (str(v.dtype), v.shape, v.tobytes()) for k, v in ref.items()}
    (driver or four_runs)(case, lambda p: snap(_check(fc)), lambda who, p: snap(_check(fc if who == "P2" else other)))


def fam_km(case, tw, oracle, cus, driver=None):
    from tests import kernel_matrix as km
    from tests import test_gpu_kernel_matrix as t
    row = case.ref
    seed = 100 + km.TABLE.index(row)
    pol = {"P2": t._policy(tw, *t._row_policy(oracle, row)), "P1": t._policy(tw, *t._row_policy(oracle, row, seed=P1_SEED))}
    counters = lambda: tuple(_lib.debug_counters(2)) if row.prec == "fp32" and row.common is None else None
    check = lambda p: snap_collected(t.check_row(tw, oracle, cus, row), p, case.counters, counters())
    call = lambda who, p: snap_collected(t._collect(tw, row, pol[who], cus, seed, merge_order=False), p, case.counters, counters())
    (driver or four_runs)(case, check, call)


def fam_drain(case, tw, oracle, cus, driver=None):
    import bench
    from tests import test_gpu_rollout_drain as t
    name, thr = case.ref
    _, side, diff, twists, E, weights, merge, seed = next(c for c in t.CASES if c[0] == name)
    arrs, op, ap, _ = t.reference(oracle, name)
    assert weights == "bench"
    pol = {"P2": amd_policy(arrs, op, ap), "P1": amd_policy(bench.synthetic_weights(side * side, seed=1), op, ap)}

    def check(p):
        g, cnt = t.check_hand_over(tw, oracle, cus, name, thr)
        return snap_collected(g, p, case.counters, tuple(cnt))

    def call(who, p):
        g, cnt = t.collect(tw, cus, side, diff, E, pol[who], seed, merge, thr)
        return snap_collected(g, p, case.counters, tuple(cnt))
    (driver or four_runs)(case, check, call)


def fam_reuse(case, tw, oracle, cus, driver=None):
    import bench
    from tests import test_gpu_rollout_reuse as t
    name = case.ref
    _, side, diff, twists, E, geom = next(s for s in t.SHAPES if s[0] == name)
    arrs, op, ap = t.reference(oracle, name)[:3]
    pol = {"P2": amd_policy(arrs, op, ap), "P1": amd_policy(bench.synthetic_weights(side * side, seed=1), op, ap)}

    def check(p):
        g = t.check_shape(tw, oracle, name)
        assert g.stats["reused_evals"] > 0
        return snap_collected(g, p, case.counters)
    (driver or four_runs)(case, check, lambda who, p: snap_collected(t.collect_shape(tw, name, pol[who]), p, case.counters))


def fam_range(case, tw, oracle, cus, driver=None):
    """fp16x2 outside its range: the kernel raises the range flag, the collect runs again in fp32 on the same workspace."""
    from tests import test_gpu_kernel_matrix as t
    w, name = case.ref
    arrs, relu, inside = t._range_case(w * w, name)
    assert not inside
    other = list(t._range_case(w * w, name)[0])
    other[0] = other[0] * np.float32(0.5)                  # other embedding rows; the unit that leaves the range keeps its bias
    pol = {"P2": t._policy(tw, arrs, [], [], emb_relu=relu), "P1": t._policy(tw, tuple(other), [], [], emb_relu=relu)}
    env = tw.env.Puzzle(w, w, 4, 2, 256)
    collect = lambda who: tw.collector.PPOCollector(300, t.G, t.G, 32, merge_order=False, precision="fp16x2").collect(env, pol[who], seed=7)

    def check(p):
        g2, was_inside = t.check_range_case(tw, oracle, cus, w, name)
        assert not was_inside
        return snap_collected(g2, p, case.counters)
    (driver or four_runs)(case, check, lambda who, p: snap_collected(collect(who), p, case.counters))


def _sm_policies(t, oracle, row):
    from tests import search_matrix as sm
    idx = sm.TABLE.index(row) if row in sm.TABLE else 500 + sorted(mm.EXTRA_ROWS).index(next(k for k, v in mm.EXTRA_ROWS.items() if v[0] == row))
    gp, opol = t.policies(oracle, row, seed=idx)
    return gp, opol, t.policies(oracle, row, seed=P1_SEED)[0], 100 + idx


def fam_sm_ppo(case, tw, oracle, cus, driver=None):
    from tests import test_gpu_search_matrix as t
    row = mm.row_of(case)
    gp, opol, p1, seed = _sm_policies(t, oracle, row)
    pol = {"P2": gp, "P1": p1}
    check = lambda p: snap_collected(t.run_ppo(tw, oracle, cus, row, gp, opol, seed), p, case.counters)
    (driver or four_runs)(case, check, lambda who, p: snap_collected(t.collect_ppo(tw, row, pol[who], seed), p, case.counters))


def fam_sm_az(case, tw, oracle, cus, driver=None):
    from tests import search_matrix as sm
    from tests import test_gpu_search_matrix as t
    row = mm.row_of(case)
    kernel = sm.dispatch(row, cus)[0]
    if "split" in case.on:
        assert kernel[0] == "deep" and kernel[7], (case.id, kernel, cus)
    gp, opol, p1, seed = _sm_policies(t, oracle, row)
    pol = {"P2": gp, "P1": p1}

    def after(g, p):
        c = _lib.debug_counters(14)
        assert c[12] == 0 and c[13] == 0, c
        return snap_collected(g, p, case.counters)
    check = lambda p: after(t.run_self_play(tw, oracle, cus, row, gp, opol, seed), p)
    (driver or four_runs)(case, check, lambda who, p: after(t.collect_self_play(tw, cus, row, pol[who], seed), p))


def fam_sm_eval(case, tw, oracle, cus, driver=None):
    from tests import test_gpu_search_matrix as t
    row = mm.row_of(case)
    gp, opol, p1, seed = _sm_policies(t, oracle, row)
    pol = {"P2": gp, "P1": p1}

    def check(p):
        result, actions, _ = t.run_evaluate(tw, oracle, cus, row, gp, opol, seed)
        return snap_attempts(result, actions)            # (the oracle runs on the CPU: the last attempts are still the checked call's)

    def call(who, p):
        _, _, result, actions = t.call_evaluate(tw, oracle, row, pol[who], seed)
        return snap_attempts(result, actions)
    (driver or four_runs)(case, check, call)


def _denv_p1(module_table, module):
    from tests.util import make_deep_policy_arrays_obs
    r = module_table.BY_MODULE[module]
    arrs = make_deep_policy_arrays_obs(r.obs_size, seed=P1_SEED, emb=r.emb, common=r.common, policy_layers=r.policy_layers,
                                       value_layers=r.value_layers, n_actions=r.A, scale=2.0)
    return amd_policy(arrs, *module_table.twists(module))


def fam_denv_ppo(case, tw, oracle, cus, driver=None):
    which, module, E = case.ref
    if which == "matrix":
        from tests import device_env_matrix as table
        from tests import test_gpu_device_env_matrix as t
        r, env, gp, _ = t._setup(module)
        check = lambda p: snap_collected(t.check_ppo_collect(tw, module, E), p)
        collect = lambda pol: t._collect(tw, r, env, pol, E)
    else:
        from tests import device_env_wide as table
        from tests import test_gpu_device_env_wide as t
        r, env, gp, _ = t._setup(module)
        check = lambda p: snap_collected(t.check_ppo_collect(tw, module), p)
        collect = lambda pol: t._collect(tw, r, env, pol)
    pol = {"P2": gp, "P1": _denv_p1(table, module)}
    (driver or four_runs)(case, check, lambda who, p: snap_collected(collect(pol[who]), p))


def fam_denv_ppo_queued(case, tw, oracle, cus, driver=None):
    which, module, groups = case.ref
    if which == "matrix":
        from tests import device_env_matrix as table
        from tests import test_gpu_device_env_matrix as t
        r, env, gp, _ = t._setup(module)
        check = lambda p: snap_collected(t.check_ppo_collect_queued(tw, module, groups), p)
        collect = lambda pol: t._collect(tw, r, env, pol, 100)
    else:
        from tests import device_env_wide as table
        from tests import test_gpu_device_env_wide as t
        r, env, gp, _ = t._setup(module)
        check = lambda p: snap_collected(t.check_ppo_collect_queued(tw, module), p)
        collect = lambda pol: t._collect(tw, r, env, pol)
    pol = {"P2": gp, "P1": _denv_p1(table, module)}

    def call(who, p):
        with t._hook(groups):
            g = collect(pol[who])
        assert g.stats["rollout_blocks"] == groups
        return snap_collected(g, p)
    (driver or four_runs)(case, check, call)


def fam_denv_var(case, tw, oracle, cus, driver=None):
    from tests import test_gpu_var_obs as t
    from tests.var_obs_util import E, GAMMA, LAM, SEED, lamps, lamps_policy_arrays
    n = case.ref
    env = lamps(n)
    pol = {"P2": t._policies(oracle, n)[0], "P1": amd_policy(lamps_policy_arrays(n, seed=P1_SEED))}
    check = lambda p: snap_collected(t.check_device_collect(tw, oracle, n, E), p)
    (driver or four_runs)(case, check, lambda who, p: snap_collected(tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, pol[who], seed=SEED), p))


@contextlib.contextmanager
def _det_exp(oracle):
    oracle.set_det_exp(True)
    try:
        yield oracle
    finally:
        oracle.set_det_exp(False)


def fam_denv_az(case, tw, oracle, cus, driver=None):
    which, module, shape = case.ref
    with _det_exp(oracle):
        if which == "matrix":
            from tests import device_env_matrix as table
            from tests import test_gpu_device_env_matrix as t
            E, S, med = shape
            r, env, gp, _ = t._setup(module)
            check = lambda p: snap_collected(t.check_self_play(tw, oracle, module, E, S, med), p)
            collect = lambda pol: tw.collector.AZCollector(E, S, 1.41, med, 4, episode_offset=r.offset).collect(env, pol, seed=r.seed)
        else:
            from tests import device_env_wide_search as table
            from tests import test_gpu_device_env_wide_search as t
            r, env, gp, _ = t._setup(module, oracle)
            check = lambda p: snap_collected(t.check_self_play(tw, oracle, module), p)
            collect = lambda pol: tw.collector.AZCollector(table.E, r.S, table.C_UCB, r.med, 4).collect(env, pol, seed=r.seed)
        pol = {"P2": gp, "P1": _denv_p1(table, module)}
        (driver or four_runs)(case, check, lambda who, p: snap_collected(collect(pol[who]), p))


def fam_denv_solve(case, tw, oracle, cus, driver=None):
    from tests import device_env_solve as D
    from tests import test_gpu_device_env_solve as t
    from tests.util import make_deep_policy_arrays
    which, N, S = case.ref
    assert which == "gridworld"
    dcase = D.gridworld_case(2, search=bool(S))
    env = dcase[0]
    pol = {"P2": D.lib_policy(dcase), "P1": amd_policy(make_deep_policy_arrays(25, seed=P1_SEED, emb=64, common=(64, 32), n_actions=4, scale=2.0))}
    snap = lambda res, att: {"result": (res[0][0], f32_bits(np.float32(res[0][1])).tobytes()), "actions": tuple(res[1]),
                             "attempts": tuple(x.tobytes() for x in att)}
    with _det_exp(oracle), t._plain():
        def check(p):
            res, att = t._check(tw, oracle, dcase, pol["P2"], False, N, S, 1)
            return snap(res, att)

        def call(who, p):
            res, _, att = t._solve(tw, env, pol[who], False, N, S, 1)
            return snap(res, att)
        (driver or four_runs)(case, check, call)


def _python_env(tw, oracle, w, h, steps, emb, common):
    from tests import test_gpu_parity as t
    arrs = t.python_env_policy_arrays(w, h, emb, common)
    proto, env = t.python_env(tw, w, h, steps)
    pol = {"P2": amd_policy(arrs), "P1": amd_policy(t.python_env_policy_arrays(w, h, emb, common, seed=P1_SEED))}
    return t, proto, env, pol, oracle_policy(oracle, arrs)


def fam_host_ppo(case, tw, oracle, cus, driver=None):
    w, h, steps, emb, common, E = case.ref
    t, proto, env, pol, op = _python_env(tw, oracle, w, h, steps, emb, common)
    check = lambda p: snap_collected(t.check_python_env_ppo(tw, oracle, proto, env, pol["P2"], op, w * h, E, False), p)
    call = lambda who, p: snap_collected(tw.collector.PPOCollector(E, 0.99, 0.95, 4, merge_order=False).collect(env, pol[who], seed=77), p)
    (driver or four_runs)(case, check, call)


def fam_host_az(case, tw, oracle, cus, driver=None):
    w, h, steps, emb, common, E, S, med = case.ref
    t, proto, env, pol, op = _python_env(tw, oracle, w, h, steps, emb, common)
    with _det_exp(oracle):
        check = lambda p: snap_collected(t.check_python_env_self_play(tw, oracle, proto, env, pol["P2"], op, w * h, E, S, med), p)
        call = lambda who, p: snap_collected(tw.collector.AZCollector(min(E, 16), S, 1.41, med, 4).collect(env, pol[who], seed=79), p)
        (driver or four_runs)(case, check, call)


def fam_host_solve(case, tw, oracle, cus, driver=None):
    w, h, steps, emb, common, (det, ns, S) = case.ref
    t, proto, env, pol, op = _python_env(tw, oracle, w, h, steps, emb, common)
    snap = lambda ge, sv: {"evaluate": tuple(f32_bits(np.float32(x)).tobytes() for x in ge), "solve": (sv[0][0], f32_bits(np.float32(sv[0][1])).tobytes()),
                           "actions": tuple(sv[1])}

    def call(who, p):
        ge = tw.collector.evaluate(env, pol[who], num_episodes=12, deterministic=det, num_searches=ns, num_mcts_searches=S, seed=5, C=1.41,
                                   max_expand_depth=1, num_cores=4)
        cur = proto.copy(); cur.seed_episode(3, 1); cur.reset(3)
        return snap(ge, tw.collector.solve(tw.env.PyEnv(cur), pol[who], det, ns, S, 1.41, 1, seed=9))
    with _det_exp(oracle):
        (driver or four_runs)(case, lambda p: snap(*t.check_python_env_evaluate_and_solve(tw, oracle, proto, env, pol["P2"], op, det, ns, S)), call)


def _handoff(case, tw, normalize, driver=None):
    """ppo_data_to_torch on a collect of a layout that follows no rule (tests/free_ids_env.py): the collect itself is host-stepped (its
    staging and its result arena are filled too), the hand-off's sums use call-local scratch."""
    from tests import test_gpu_trainer_handoff as t
    from tests.free_ids_env import ACTIONS, LAYOUTS, FreeIdsWalk, policy_arrays
    from twisterl_amd import trainer
    layout = case.ref
    _, obs_size, n_obs, _ = LAYOUTS[layout]
    A = ACTIONS[layout]
    ident = list(range(obs_size))
    twists = ([ident, ident], [list(range(A)), list(range(A))]) if layout in "ac" else ((), ())
    pol = {"P2": amd_policy(policy_arrays(layout, seed=11), *twists), "P1": amd_policy(policy_arrays(layout, seed=12), *twists)}

    def run(who, p, checked):
        env = tw.env.PyEnv(FreeIdsWalk(layout, A))
        env.difficulty = 6
        data = tw.collector.PPOCollector(200, 0.99, 0.95, 1).collect(env, pol[who], seed=5)
        out = trainer.ppo_data_to_torch(data, obs_size, normalize_advantage=normalize)
        form = t._form()
        stats = trainer.adv_stats(data) if normalize else None
        if checked:
            a = data.to_numpy()
            assert form == (0, 0, -(-len(data) * n_obs // 256), 256), form
            t._check_onehot(out[0].cpu().numpy(), a["obs"], obs_size, layout)
            t._check_log_probs(out[1].cpu().numpy(), a["logits"], a["actions"], A, f"layout {layout} under the fill")
            assert np.array_equal(out[2].cpu().numpy(), a["actions"].astype(np.int64)) and np.array_equal(out[5].cpu().numpy(), a["perms"].astype(np.int64))
            assert np.array_equal(f32_bits(out[4].cpu().numpy()), f32_bits(a["rets"]))
            if normalize:
                t._check_normalized(out[3].cpu().numpy(), a["advs"], f"layout {layout} under the fill")
                t._check_adv_stats(data, a["advs"])
            else:
                assert np.array_equal(f32_bits(out[3].cpu().numpy()), f32_bits(a["advs"]))
        snap = snap_collected(data, p)
        snap.update(snap_tensors(out))
        snap["form"], snap["adv_stats"] = form, None if stats is None else tuple(np.float64(x).tobytes() for x in stats)
        return snap
    (driver or four_runs)(case, lambda p: run("P2", p, True), lambda who, p: run(who, p, False))


def fam_handoff_ppo(case, tw, oracle, cus, driver=None):
    _handoff(case, tw, True, driver)


def fam_handoff_ppo_plain(case, tw, oracle, cus, driver=None):
    _handoff(case, tw, False, driver)


def fam_handoff_az(case, tw, oracle, cus, driver=None):
    from tests import test_gpu_trainer_handoff as t
    from tests.free_ids_env import ACTIONS, FreeIdsWalk, policy_arrays
    from twisterl_amd import trainer
    layout = case.ref
    assert layout == "b"
    pol = {"P2": amd_policy(policy_arrays("b", seed=11)), "P1": amd_policy(policy_arrays("b", seed=12))}

    def run(who, p, checked):
        env = tw.env.PyEnv(FreeIdsWalk("b", ACTIONS["b"]))
        env.difficulty = 4
        az = tw.collector.AZCollector(24, 4, 1.41, 1, 1).collect(env, pol[who], seed=2)
        out = trainer.az_data_to_torch(az, 27)
        form = t._form()
        if checked:
            b = az.to_numpy()
            assert form == (0, 0, -(-len(az) * 3 // 256), 256)
            t._check_onehot(out[0].cpu().numpy(), b["obs"], 27)
            assert np.array_equal(f32_bits(out[1].cpu().numpy()), f32_bits(b["logits"]))
            assert np.array_equal(f32_bits(out[2].cpu().numpy()[:, 0]), f32_bits(b["remaining_values"]))
        snap = snap_collected(az, p)
        snap.update(snap_tensors(out))
        snap["form"] = form
        return snap
    (driver or four_runs)(case, lambda p: run("P2", p, True), lambda who, p: run(who, p, False))


FAMILIES = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("fam_")}


def test_every_family_of_the_table_has_its_runner():
    assert {c.family for c in mm.CASES} == set(FAMILIES)


@pytest.mark.parametrize("case_id", mm.IDS)
def test_results_do_not_depend_on_what_device_memory_held(tw, oracle, cus, case_id):
    case = mm.BY_ID[case_id]
    try:
        FAMILIES[case.family](case, tw, oracle, cus)
    finally:
        assert _lib.debug_fill_memory._current() == HOOK_AT_START         # no case leaves the hook on
