"""GPU: the PERSISTENT grid of the device-environment rollout and evaluate kernels (PPO collect, plain evaluate; the search kernel
has none).  With more episodes (attempts) than the grid holds columns, a column
whose episode is over takes the next one from a device-side counter (EnvRolloutArgs::queue) -- and every byte stays what the plain
launch, the host-stepped path and the oracle give.  The hook TW_OPT_ENV_RESIDENT_GROUPS caps the grid at one or two workgroups (16 or
32 columns), so that a few dozen episodes go through the queue several times over; every case first asserts what the library says
it launched (persist == 1, blocks == the hook), which is what fails without the feature.  All comparisons are bitwise."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests.device_env_search_util import host_evaluate
from tests.device_env_util import HostEnv, gridworld, ring
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays, oracle_policy
from tests.var_obs_util import lamps, lamps_policy_arrays, lamps_twists

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code.  A signal handler runs only when control returns to
    the interpreter, so a hang inside a HIP call is bounded by the `timeout` around the pytest run, not by this."""
    def boom(*_):
        raise TimeoutError("device-environment persistence test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    from twisterl_amd import twisterl
    if twisterl_amd.device_count() < 1:
        pytest.fail("no GPU visible")
    return twisterl


@pytest.fixture()
def det_exp(oracle):
    oracle.set_det_exp(True)
    yield oracle
    oracle.set_det_exp(False)


def _hook(groups):
    from twisterl_amd import _lib
    return _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups)


def _plain():
    from twisterl_amd import _lib
    return _lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1)


def _assert_launch(family, persist, blocks):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["persist"], info["blocks"], info["threads"]) == (family, 1, persist, blocks, 256), info


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k


def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def _host_collect(env, policy, E, gamma, lam, seed, offset=0, merge_order=True):
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.PPOParams(E, offset, gamma, lam, seed, _lib.TW_PREC_F32_EXACT, int(merge_order), 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _ppo_oracle_same(g, o, n_obs, A):
    a = g.to_numpy()
    assert a["obs"].shape[1] == n_obs and a["logits"].shape[1] == A
    assert np.array_equal(a["obs"].astype(np.int64), o.obs) and np.array_equal(a["actions"].astype(np.int64), o.actions)
    assert np.array_equal(a["perms"].astype(np.int32), o.perms) and np.array_equal(a["ep_len"], o.ep_len)
    for k, ok in (("logits", o.logits), ("values", o.values), ("rewards", o.rewards), ("advs", o.additional_data["advs"]),
                  ("rets", o.additional_data["rets"])):
        assert np.array_equal(f32_bits(a[k]), f32_bits(ok)), k


def _ppo_persistent(tw, env, gp, E, groups, seed, offset=0, merge_order=True, runs=1):
    """The collect on a grid of `groups` workgroups (asserted), equal to the plain launch and the host-stepped path; returns it."""
    from twisterl_amd import _lib
    col = lambda: tw.collector.PPOCollector(E, 0.99, 0.95, 4, merge_order=merge_order, episode_offset=offset).collect(env, gp, seed=seed)
    with _hook(groups):
        g = col()
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, groups)
        assert g.stats["rollout_blocks"] == groups and g.stats["rollout_threads"] == 256
        for _ in range(runs - 1):                                         # (two workgroups race for the counter: not for the bytes)
            _same_bytes(g, col())
            _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, groups)
    with _plain():
        p = col()
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 0, (E + 15) // 16)
    _same_bytes(g, p)
    _same_bytes(g, _host_collect(env, gp, E, 0.99, 0.95, seed, offset=offset, merge_order=merge_order))
    return g


def _ring_twists(n):
    mir = lambda p: (n - p) % n
    ident = list(range(2 * n))
    flip = [mir(i) if i < n else n + mir(i - n) for i in range(2 * n)]
    return [ident, flip], [[0, 1, 2], [2, 1, 0]]


# ---- 1. PPO, GridWorld 5 x 5: 100 episodes on 16 columns are six full refills and a tail of 4 with the queue running dry ------------------
@pytest.mark.parametrize("groups,merge_order,offset", [(1, True, 0), (2, False, 1000)])
def test_ppo_gridworld(tw, oracle, groups, merge_order, offset):
    env = gridworld(max_steps=24, difficulty=2, max_records=25)
    arrs = make_deep_policy_arrays(25, seed=3, emb=64, common=(32,), n_actions=4)
    gp, op = amd_policy(arrs), oracle_policy(oracle, arrs)
    g = _ppo_persistent(tw, env, gp, 100, groups, 123, offset=offset, merge_order=merge_order, runs=2)
    o = oracle.ppo_collect_env(HostEnv(env), op, 100, 0.99, 0.95, seed=123, episode_offset=offset, difficulty=2, merge_order=merge_order)
    _ppo_oracle_same(g, o, 25, 4)
    n = g.to_numpy()["ep_len"]
    assert len(n) == 100 and len(set(n.tolist())) > 3                     # ragged: the columns take their next episodes at different steps


# ---- 2. PPO, RingWalk: a step() that draws from (seed, episode, t) -- a refilled column's t and episode key restart ------------------------
def test_ppo_ring(tw, oracle):
    env = ring(n=32, max_steps=40, difficulty=3, noise=0.25, max_records=41)
    tws = _ring_twists(32)
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64, 32), n_actions=3)
    gp, op = amd_policy(arrs, *tws), oracle_policy(oracle, arrs, *tws)
    g = _ppo_persistent(tw, env, gp, 50, 1, 41)
    o = oracle.ppo_collect_env(HostEnv(env), op, 50, 0.99, 0.95, seed=41, difficulty=3)
    _ppo_oracle_same(g, o, 2, 3)
    assert set(np.unique(g.to_numpy()["perms"]).tolist()) == {0, 1}


# ---- 3. PPO, Lamps: observe_n; EngineV<16> and EngineV<64> -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 40])
def test_ppo_lamps(tw, n):
    env = lamps(n)
    gp = amd_policy(lamps_policy_arrays(n), *lamps_twists(n))
    g = _ppo_persistent(tw, env, gp, 40, 1, 29)
    assert g.ragged and (g.to_numpy()["obs"] == 0xFFFF).any()


# ---- 4. reserve_cus, without the hook ---------------------------------------------------------------------------------------------------------
def test_reserve_cus_sizes_the_grid(tw):
    import twisterl_amd
    from twisterl_amd import _lib
    cus = int(twisterl_amd.device_info()["compute_units"])
    env = gridworld(max_steps=24, difficulty=2, max_records=25)
    gp = amd_policy(make_deep_policy_arrays(25, seed=3, emb=64, common=(32,), n_actions=4))
    E = 100
    a = tw.collector.PPOCollector(E, 0.99, 0.95, 4, reserve_cus=cus - 1).collect(env, gp, seed=7)
    info = _lib.debug_last_launch()
    assert info["family"] == _lib.TW_KERNEL_ROLLOUT_BIG and info["persist"] == 1 and 1 <= info["blocks"] and info["blocks"] * 16 < E, info
    assert a.stats["rollout_blocks"] == info["blocks"]
    b = tw.collector.PPOCollector(E, 0.99, 0.95, 4, reserve_cus=0).collect(env, gp, seed=7)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 0, (E + 15) // 16)        # every CU: 100 episodes are resident at once
    _same_bytes(a, b)


# ---- 5. errors: the episodes that decide which id is reported first include ones taken from the queue ---------------------------------------
@pytest.mark.parametrize("bad_at", [0, 2])
def test_bad_ids_fail_alike(tw, bad_at):
    from twisterl_amd import _lib
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64,), policy_layers=(32,), n_actions=3)
    gp = amd_policy(arrs)
    env = ring(n=32, max_steps=40, difficulty=8, noise=0.0, bad_at=bad_at, max_records=41)
    col = lambda: tw.collector.PPOCollector(50, 0.99, 0.95, 4).collect(env, gp, seed=1)
    with _hook(1):
        dev = _message(col)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, 1)
    with _plain():
        plain = _message(col)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 0, 4)
    host = _message(lambda: _host_collect(env, gp, 50, 0.99, 0.95, 1))
    assert dev == plain == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (dev, plain, host)
    # evaluate: 25 episodes x 2 attempts on 16 columns
    ev = lambda: tw.collector.evaluate(env, gp, 25, False, 2, 0, 1, 1.41, 1, 1)
    with _hook(1):
        dev = _message(ev)
        _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, 1, 1)
    with _plain():
        plain = _message(ev)
    host = _message(lambda: host_evaluate(env, gp, 25, False, 2, 0, 1))
    assert dev == plain == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (dev, plain, host)
    # the same handles work afterwards
    ok = ring(n=32, max_steps=40, difficulty=3, noise=0.0, max_records=41)
    with _hook(1):
        g = tw.collector.PPOCollector(50, 0.99, 0.95, 4).collect(ok, gp, seed=1)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, 1)
    assert len(g) >= 50


def test_an_episode_longer_than_max_records_fails_alike(tw):
    from twisterl_amd import _lib
    gp = amd_policy(make_deep_policy_arrays(8, seed=9, emb=64, common=(64,), policy_layers=(32,), n_actions=3))
    short = ring(n=32, max_steps=40, difficulty=8, noise=0.0, max_records=2)
    col = lambda: tw.collector.PPOCollector(50, 0.99, 0.95, 4).collect(short, gp, seed=1)
    with _hook(1):
        dev = _message(col)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, 1)
    with _plain():
        plain = _message(col)
    host = _message(lambda: _host_collect(short, gp, 50, 0.99, 0.95, 1))
    assert dev == plain == host and dev[0] is ValueError and "did not end within 2 records" in dev[1], (dev, plain, host)
    ok = ring(n=32, max_steps=40, difficulty=3, noise=0.0, max_records=41)
    with _hook(1):
        g = tw.collector.PPOCollector(50, 0.99, 0.95, 4).collect(ok, gp, seed=1)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, 1)
    assert len(g) >= 50


# ---- 6. plain evaluate: 40 episodes x 2 attempts = 80 attempts on 16 columns ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["gridworld", "ring"])
def test_evaluate(tw, det_exp, which):
    from twisterl_amd import _lib
    if which == "gridworld":
        env, diff = gridworld(max_steps=24, difficulty=2, max_records=25), 2
        arrs, tws = make_deep_policy_arrays(25, seed=11, emb=64, common=(64, 32), n_actions=4), ((), ())
    else:
        env, diff = ring(n=32, max_steps=30, difficulty=4, noise=0.1, max_records=31), 4
        arrs, tws = make_deep_policy_arrays(8, seed=2, emb=64, common=(64, 32), n_actions=3), _ring_twists(32)
    gp, op = amd_policy(arrs, *tws), oracle_policy(det_exp, arrs, *tws)
    for det in (True, False):
        ev = lambda: tw.collector.evaluate(env, gp, num_episodes=40, deterministic=det, num_searches=2, num_mcts_searches=0, seed=5, C=1.41,
                                           max_expand_depth=1, num_cores=4)
        with _hook(1):
            ge = ev()
            _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, 1, 1)
            ga = _lib.debug_last_attempts()
        with _plain():
            pe = ev()
            _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, 0, 5)
            pa = _lib.debug_last_attempts()
        assert len(ga[0]) == 80 and all(x.tobytes() == y.tobytes() for x, y in zip(ga, pa))
        he = host_evaluate(env, gp, 40, det, 2, 0, 5)
        oe = det_exp.evaluate_env(HostEnv(env), op, 40, det, 2, 0, 1.41, 1, seed=5, difficulty=diff)
        for other in (pe, he, oe):
            assert f32_bits(ge[0]) == f32_bits(other[0]) and f32_bits(ge[1]) == f32_bits(other[1]), (which, det, ge, other)


# ---- 7. the automatic rule: more episodes than the chip holds columns -------------------------------------------------------------------------
def test_the_automatic_rule(tw):
    """resident = groups_per_cu x CUs x 16.  groups_per_cu is the module's own answer for the launch's LDS size, which the test does
    not know to the byte: this policy's widest layer is 32 units, so the engine's three activation buffers (17 floats per unit) hold
    at most 3 x 32 x 17 floats and its other segments 128 + 256 + 16 x 25 + 544 -- about 12 KiB.  The answer is asked for 8 KiB and
    for 20 KiB and must be the same (with this little LDS the registers decide), then it is the launch's too."""
    import twisterl_amd
    from twisterl_amd import _lib
    cus = int(twisterl_amd.device_info()["compute_units"])
    env = gridworld(max_steps=8, difficulty=2, max_records=9)
    gp = amd_policy(make_deep_policy_arrays(25, seed=3, emb=32, common=(32,), n_actions=4))
    lo, hi = C.c_int(0), C.c_int(0)
    assert env._desc.groups_per_cu(0, 8 * 1024, C.byref(lo)) == 0 and env._desc.groups_per_cu(0, 20 * 1024, C.byref(hi)) == 0
    assert 1 <= lo.value == hi.value <= 8, (lo.value, hi.value)
    resident = lo.value * cus * 16
    col = lambda E: tw.collector.PPOCollector(E, 0.99, 0.95, 4).collect(env, gp, seed=3)
    g = col(resident + 16)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 1, resident // 16)
    with _plain():
        p = col(resident + 16)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 0, resident // 16 + 1)
    _same_bytes(g, p)
    col(resident)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, 0, resident // 16)
