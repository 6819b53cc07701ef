"""GPU: user-written environments collected and evaluated ON THE DEVICE (tw_ppo_collect_device_env / tw_evaluate_device_env) are
bit-equal to the host-stepped path over the module's own vtable (tw_ppo_collect_env) and to the oracle's restatement of
ppo.rs / evaluate.rs running the same struct's host code; what the kernel does not take gives the host path's bytes and errors."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests.device_env_util import HostEnv, big_puzzle, gridworld, ring
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays, oracle_policy

pytestmark = pytest.mark.gpu
FIELDS = ("obs", "logits", "perms", "values", "rewards", "actions", "advs", "rets", "ep_len", "ep_start")


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code.  A signal handler runs only when control returns to
    the interpreter, so a hang inside a HIP call is bounded by the `timeout` around the pytest run, not by this."""
    def boom(*_):
        raise TimeoutError("device-environment test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(240)
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


def _host_collect(env, policy, E, gamma, lam, seed, offset=0, merge_order=True):
    """tw_ppo_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.PPOParams(E, offset, gamma, lam, seed, _lib.TW_PREC_F32_EXACT, int(merge_order), 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k


def _same_as_oracle(g, o, n_obs, A):
    a = g.to_numpy()
    assert a["obs"].shape[1] == n_obs and a["logits"].shape[1] == A
    assert np.array_equal(a["obs"].astype(np.int64), o.obs)
    assert np.array_equal(a["actions"].astype(np.int64), o.actions)
    assert np.array_equal(a["perms"].astype(np.int32), o.perms)
    for k, ok in (("logits", o.logits), ("values", o.values), ("rewards", o.rewards), ("advs", o.additional_data["advs"]),
                  ("rets", o.additional_data["rets"])):
        assert np.array_equal(f32_bits(a[k]), f32_bits(ok)), k
    assert np.array_equal(a["ep_len"], o.ep_len)


def _grid_policy(oracle, seed=3, common=(128,)):
    arrs = make_deep_policy_arrays(25, seed=seed, emb=512, common=common, n_actions=4)     # 625 -> 512 -> 128 -> heads
    return amd_policy(arrs), oracle_policy(oracle, arrs)


def test_gridworld_collect_equals_host_path_and_oracle(tw, oracle):
    env = gridworld(max_steps=64, difficulty=2, max_records=65)
    gp, op = _grid_policy(oracle)
    E = 1024
    g = tw.collector.PPOCollector(E, 0.995, 0.995, 32).collect(env, gp, seed=123)
    assert g.stats["rollout_threads"] == 256 and g.stats["rollout_blocks"] == E // 16      # the device kernel ran
    h = _host_collect(env, gp, E, 0.995, 0.995, 123)
    _same_bytes(g, h)
    o = oracle.ppo_collect_env(HostEnv(env), op, E, 0.995, 0.995, seed=123, difficulty=2)
    _same_as_oracle(g, o, 25, 4)
    a = g.to_numpy()
    assert a["obs"].dtype == np.uint16 and a["ep_len"].max() <= 65 and a["ep_len"].min() >= 1


def test_gridworld_65536_episodes_sampled_against_the_oracle(tw, oracle):
    env = gridworld(max_steps=64, difficulty=3, max_records=65)
    gp, op = _grid_policy(oracle, seed=5)
    E = 65536
    g = tw.collector.PPOCollector(E, 0.99, 0.95, 32, merge_order=False).collect(env, gp, seed=77)
    a = g.to_numpy()
    rng = np.random.default_rng(1)
    picks = sorted(set([0, 1, 2, E // 2, E - 2, E - 1] + rng.integers(0, E, 70).tolist()))
    assert len(picks) >= 64
    for e in picks:
        o = oracle.ppo_collect_env(HostEnv(env), op, 1, 0.99, 0.95, seed=77, episode_offset=e, difficulty=3)
        s, n = int(a["ep_start"][e]), int(a["ep_len"][e])
        assert n == len(o.values), e
        sl = slice(s, s + n)
        assert np.array_equal(a["obs"][sl].astype(np.int64), o.obs), e
        assert np.array_equal(a["actions"][sl].astype(np.int64), o.actions), e
        for k, ok in (("logits", o.logits), ("values", o.values), ("rewards", o.rewards), ("advs", o.additional_data["advs"]),
                      ("rets", o.additional_data["rets"])):
            assert np.array_equal(f32_bits(a[k][sl]), f32_bits(ok)), (e, k)


def _ring_twists(n):
    mir = lambda p: (n - p) % n
    ident = list(range(2 * n))
    flip = [mir(i) if i < n else n + mir(i - n) for i in range(2 * n)]
    return [ident, flip], [[0, 1, 2], [2, 1, 0]]


def test_ring_three_actions_twists_and_difficulty(tw, oracle):
    n = 32
    env = ring(n=n, max_steps=40, difficulty=3, noise=0.25, max_records=41)
    op_, ap_ = _ring_twists(n)
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64, 32), n_actions=3)          # obs_size 64, two common layers
    gp, orp = amd_policy(arrs, op_, ap_), oracle_policy(oracle, arrs, op_, ap_)
    for diff, E, seed in ((3, 300, 41), (9, 200, 42)):
        env.difficulty = diff
        assert env.difficulty == diff
        g = tw.collector.PPOCollector(E, 0.99, 0.95, 4).collect(env, gp, seed=seed)
        assert g.stats["rollout_threads"] == 256 and g.stats["rollout_blocks"] == (E + 15) // 16    # the device kernel ran
        o = oracle.ppo_collect_env(HostEnv(env), orp, E, 0.99, 0.95, seed=seed, difficulty=diff)
        _same_as_oracle(g, o, 2, 3)
        _same_bytes(g, _host_collect(env, gp, E, 0.99, 0.95, seed))
        a = g.to_numpy()
        assert a["logits"].shape[1] == 3 and a["actions"].max() <= 2 and a["obs"].dtype == np.uint8
        assert set(np.unique(a["perms"]).tolist()) == {0, 1}


def test_evaluate_equals_the_oracle(tw, oracle):
    env = gridworld(max_steps=24, difficulty=2, max_records=25)
    gp, op = _grid_policy(oracle, seed=11, common=(64, 32))
    n = 32
    r = ring(n=n, max_steps=30, difficulty=4, noise=0.1, max_records=31)
    arrs = make_deep_policy_arrays(8, seed=2, emb=64, common=(64, 32), n_actions=3)
    rp, rop = amd_policy(arrs, *_ring_twists(n)), oracle_policy(oracle, arrs, *_ring_twists(n))
    oracle.set_det_exp(True)                                              # the soft-max's exp: the same spec on both sides
    try:
        for e, p, po, diff in ((env, gp, op, 2), (r, rp, rop, 4)):
            for det, ns in ((True, 1), (False, 2)):
                ge = tw.collector.evaluate(e, p, num_episodes=40, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=5, C=1.41,
                                           max_expand_depth=1, num_cores=4)
                oe = oracle.evaluate_env(HostEnv(e), po, 40, det, ns, 0, 1.41, 1, seed=5, difficulty=diff)
                assert f32_bits(ge[0]) == f32_bits(oe[0]) and f32_bits(ge[1]) == f32_bits(oe[1]), (det, ns, ge, oe)
    finally:
        oracle.set_det_exp(False)


def test_big_puzzle_module_gives_the_bytes_of_the_library_puzzle(tw):
    """One Puzzle, two pairs of kernels: tw.env.Puzzle of a 5 x 5 board runs in rollout_big_kernel / solve_big_kernel, the same
    step / masks / reward / is_final as the struct BigPuzzleEnv<25>, built as a module, in rollout_env_kernel / solve_env_kernel --
    the same bytes from both.  40 episodes are two and a half workgroups."""
    from tests.util import puzzle_transpose_twist
    D = 5
    gp = amd_policy(make_deep_policy_arrays(25, seed=7, emb=64, common=(64, 32), scale=2.0), *puzzle_transpose_twist(5))
    lib_env, mod_env = tw.env.Puzzle(5, 5, D, 2, 256), big_puzzle(5, 5, D, 2, 256, max_records=2 * D + 1)
    for merge_order in (True, False):
        a = tw.collector.PPOCollector(40, 0.995, 0.995, 4, merge_order=merge_order).collect(lib_env, gp, seed=23)
        b = tw.collector.PPOCollector(40, 0.995, 0.995, 4, merge_order=merge_order).collect(mod_env, gp, seed=23)
        assert a.stats["rollout_blocks"] == b.stats["rollout_blocks"] == 3 and a.stats["rollout_threads"] == b.stats["rollout_threads"] == 256
        _same_bytes(a, b)
        x = a.to_numpy()
        assert sorted(x) == sorted(FIELDS) and x["obs"].dtype == np.uint16 and x["obs"].shape[1] == 25 and set(np.unique(x["perms"]).tolist()) == {0, 1}
    for det, ns in ((True, 1), (False, 2)):
        ea = tw.collector.evaluate(lib_env, gp, num_episodes=200, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=5, C=1.41,
                                   max_expand_depth=1, num_cores=4)
        eb = tw.collector.evaluate(mod_env, gp, num_episodes=200, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=5, C=1.41,
                                   max_expand_depth=1, num_cores=4)
        assert f32_bits(ea[0]) == f32_bits(eb[0]) and f32_bits(ea[1]) == f32_bits(eb[1]), (det, ns, ea, eb)


def test_shapes_the_kernel_does_not_take_run_on_the_host(tw, oracle):
    from tests.util import make_policy_arrays
    from twisterl_amd import _lib
    env = gridworld(size=3, max_steps=12, difficulty=2, max_records=13)
    arrs = make_policy_arrays(9, seed=4, emb=64, hidden=64)             # obs_size 81, ONE common layer of 64: the MFMA shape
    gp = amd_policy(arrs)
    g = tw.collector.PPOCollector(200, 0.99, 0.95, 4).collect(env, gp, seed=3)
    _same_bytes(g, _host_collect(env, gp, 200, 0.99, 0.95, 3))
    o = oracle.ppo_collect_env(HostEnv(env), oracle_policy(oracle, arrs), 200, 0.99, 0.95, seed=3, difficulty=2)
    _same_as_oracle(g, o, 9, 4)
    # AZCollector: the host path over the module's vtable
    z = tw.collector.AZCollector(8, 6, 1.41, 1, 4).collect(env, gp, seed=8)
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.AZParams(8, 0, 6, 1.41, 1, 8, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_az_collect_env(C.byref(vt), gp._handle(), C.byref(prm), env.max_records, C.byref(out)))
    from twisterl_amd.collector import CollectedData, _DeviceResult
    _same_bytes(z, CollectedData._from_device(_DeviceResult(out.value)))
    with pytest.raises(RuntimeError, match="f32 only"):
        tw.collector.PPOCollector(16, 0.99, 0.95, 4, precision="fp16").collect(env, gp, seed=1)


def _message(fn):
    """The exception a call raises: type and message."""
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def _host_evaluate(env, policy, n, det, ns, seed):
    """tw_evaluate_env over the module's host vtable, called directly."""
    from twisterl_amd import _lib
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.SolveParams(int(det), ns, 0, 1.41, 1, seed, _lib.TW_PREC_F32_EXACT)
    s, r = C.c_float(), C.c_float()
    _lib.check(_lib.lib().tw_evaluate_env(C.byref(vt), policy._handle(), C.byref(prm), n, 0, env.max_records, C.byref(s), C.byref(r)))


def test_invalid_obs_id_fails_the_collect_without_a_fault(tw, oracle):
    """Bad ids -- above obs_size in every episode, negative ones beside them in odd episodes -- fail the collect and evaluate with
    the host path's exception and message, naming the same (first) id; the kernel guards the loads, nothing faults.  The exception
    is ValueError: the host path's TW_ERR_INVALID, raised by _lib.check for both paths alike."""
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64,), policy_layers=(32,), n_actions=3)
    gp = amd_policy(arrs)
    for bad_at in (0, 2, 5):
        env = ring(n=32, max_steps=40, difficulty=8, noise=0.0, bad_at=bad_at, max_records=41)
        dev = _message(lambda: tw.collector.PPOCollector(64, 0.99, 0.95, 4).collect(env, gp, seed=1))
        host = _message(lambda: _host_collect(env, gp, 64, 0.99, 0.95, 1))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
        dev = _message(lambda: tw.collector.evaluate(env, gp, 16, False, 2, 0, 1, 1.41, 1, 1))
        host = _message(lambda: _host_evaluate(env, gp, 16, False, 2, 1))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
    # an episode longer than max_records: the host path's error
    short = ring(n=32, max_steps=40, difficulty=8, noise=0.0, max_records=2)
    with pytest.raises(ValueError, match="did not end within 2 records"):
        tw.collector.PPOCollector(64, 0.99, 0.95, 4).collect(short, gp, seed=1)
    # the device is fine afterwards
    ok = ring(n=32, max_steps=40, difficulty=3, noise=0.0, max_records=41)
    g = tw.collector.PPOCollector(64, 0.99, 0.95, 4).collect(ok, gp, seed=1)
    assert len(g) > 0 and g.stats["rollout_threads"] == 256


def test_long_horizons_run_on_the_host_path(tw, oracle):
    """The finalize step's LDS tile holds 1,820 records of an episode: a collect that allows longer episodes runs on the
    host-stepped path, byte-equal; at 1,820 it still runs on the device, byte-equal too."""
    env_arrs = make_deep_policy_arrays(8, seed=12, emb=64, common=(64, 32), n_actions=3)
    gp = amd_policy(env_arrs, *_ring_twists(32))
    for max_records, on_device in ((1820, True), (1821, False), (5000, False)):
        env = ring(n=32, max_steps=60, difficulty=6, noise=0.2, max_records=max_records)
        g = tw.collector.PPOCollector(300, 0.99, 0.95, 4).collect(env, gp, seed=31)
        assert (g.stats["rollout_threads"] == 256) == on_device, (max_records, g.stats)
        _same_bytes(g, _host_collect(env, gp, 300, 0.99, 0.95, 31))


def test_trainer_hand_off_equals_the_host_collect(tw, oracle):
    import torch
    from twisterl_amd.trainer import ppo_data_to_torch
    # (the one-hot packing takes one-byte obs ids: the ring's 64, three actions, twists)
    env = ring(n=32, max_steps=40, difficulty=5, noise=0.2, max_records=41)
    arrs = make_deep_policy_arrays(8, seed=6, emb=64, common=(64, 32), n_actions=3)
    gp = amd_policy(arrs, *_ring_twists(32))
    g = tw.collector.PPOCollector(256, 0.99, 0.95, 4).collect(env, gp, seed=19)
    h = _host_collect(env, gp, 256, 0.99, 0.95, 19)
    for norm in (False, True):
        tg, th = ppo_data_to_torch(g, 64, normalize_advantage=norm), ppo_data_to_torch(h, 64, normalize_advantage=norm)
        assert len(tg) == len(th) == 6
        for x, y in zip(tg, th):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
