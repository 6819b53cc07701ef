"""GPU: environments whose observations vary in length.  The lamps modules (tests/device_envs/lamps.hpp: N_OBS 12 on EngineV<16>, 40 on
EngineV<64>) collected ON THE DEVICE are byte-equal to the host-stepped collect over the module's own vtable (observe_n) and bit-equal to
the oracle's loop over the same struct's host code -- the 0xFFFF padding of the two-byte obs field included; evaluate, the host-stepped
self-play, the errors (an id outside obs_size, a count above N_OBS: same message, same first occurrence on both paths), the trainer
hand-off's two-byte scatter (ragged results, and fixed-length environments with more than 256 ids), a Python environment with
max_obs(), and the gather's refusal.  The oracle's collect is computed once (tests/var_obs_util.shared_collect) and shared."""
import ctypes as C
import signal
import struct

import numpy as np
import pytest

from tests.device_env_util import ring
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays, oracle_policy
from tests.var_obs_util import (DIFFICULTY, E, GAMMA, LAM, NO_ID, SEED, SIZES, PyLamps, VarHostEnv, lamps, lamps_policy_arrays, lamps_twists,
                                oracle_az_loop, oracle_ppo_loop, shared_collect)

pytestmark = pytest.mark.gpu
BAD_AT_OFFSET = 3 * 8 + 2 * 4          # struct Lamps: mask, seed, episode (uint64), max_steps, diff, then bad_at (int32)


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for the Python side of a test; a hang inside a HIP call is bounded by the `timeout` around the run."""
    def boom(*_):
        raise TimeoutError("variable-length-observation test exceeded its time limit")
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


def _policies(oracle, n, twists=False):
    arrs = lamps_policy_arrays(n)
    t = lamps_twists(n) if twists else ((), ())
    return amd_policy(arrs, *t), oracle_policy(oracle, arrs, *t)


def _vtable(env):
    from twisterl_amd import _lib
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    return vt


def _host_collect(env, policy, num_episodes, seed):
    """tw_ppo_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _vtable(env)
    prm = _lib.PPOParams(num_episodes, 0, GAMMA, LAM, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _host_evaluate(env, policy, n, det, ns, seed):
    from twisterl_amd import _lib
    vt = _vtable(env)
    prm = _lib.SolveParams(int(det), ns, 0, 1.41, 1, seed, _lib.TW_PREC_F32_EXACT)
    s, r = C.c_float(), C.c_float()
    _lib.check(_lib.lib().tw_evaluate_env(C.byref(vt), policy._handle(), C.byref(prm), n, 0, env.max_records, C.byref(s), C.byref(r)))
    return s.value, r.value


def _device_kernel_ran(family, n, blocks):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["blocks"], info["threads"]) == (family, 1, 16 if n == 12 else 64, blocks, 256), info


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k


def _same_as_loop(g, o, n):
    a = g.to_numpy()
    assert g.ragged and a["obs"].dtype == np.uint16 and a["obs"].shape == o.obs.shape and a["obs"].shape[1] == n
    assert np.array_equal(a["obs"], o.obs)                                    # the ids AND the 0xFFFF padding
    assert np.array_equal((a["obs"] != NO_ID).sum(axis=1), o.counts)
    assert np.array_equal(a["actions"].astype(np.int64), o.actions) and np.array_equal(a["perms"].astype(np.int32), o.perms)
    for k in ("logits", "values", "rewards", "advs", "rets"):
        assert np.array_equal(f32_bits(a[k]), f32_bits(getattr(o, k))), k
    assert np.array_equal(a["ep_len"], o.ep_len)
    assert g.obs == o.obs_lists                                               # the reference's lists: the padding stripped


@pytest.mark.parametrize("num_episodes", [E, 1])
@pytest.mark.parametrize("n", SIZES)
def test_device_collect_equals_the_host_stepped_collect_and_the_oracle(tw, oracle, n, num_episodes):
    check_device_collect(tw, oracle, n, num_episodes)


def check_device_collect(tw, oracle, n, num_episodes):
    """-> the device collect of Lamps<n> that was checked"""
    from twisterl_amd import _lib
    env = lamps(n)
    gp, _ = _policies(oracle, n)
    g = tw.collector.PPOCollector(num_episodes, GAMMA, LAM, 4).collect(env, gp, seed=SEED)
    _device_kernel_ran(_lib.TW_KERNEL_ROLLOUT_BIG, n, (num_episodes + 15) // 16)
    assert g.stats["rollout_threads"] == 256 and g.stats["rollout_blocks"] == (num_episodes + 15) // 16
    h = _host_collect(env, gp, num_episodes, SEED)
    assert h.ragged and h.stats["rollout_threads"] == 0
    _same_bytes(g, h)
    _same_as_loop(g, shared_collect(n, False, num_episodes), n)
    return g


@pytest.mark.parametrize("n", SIZES)
def test_device_collect_with_twists(tw, oracle, n):
    """Two twists (n = 40: obs_size 1,600, the two-byte twist table): the ids are stored as the environment wrote them, the forward sums
    the twisted rows of exactly the ids the record has."""
    from twisterl_amd import _lib
    env = lamps(n)
    gp, _ = _policies(oracle, n, twists=True)
    g = tw.collector.PPOCollector(40, GAMMA, LAM, 4).collect(env, gp, seed=SEED)
    _device_kernel_ran(_lib.TW_KERNEL_ROLLOUT_BIG, n, 3)
    _same_bytes(g, _host_collect(env, gp, 40, SEED))
    o = shared_collect(n, True, 40)
    _same_as_loop(g, o, n)
    assert set(np.unique(o.perms).tolist()) == {0, 1}


@pytest.mark.parametrize("n", SIZES)
def test_evaluate_equals_the_oracle(tw, oracle, n):
    from twisterl_amd import _lib
    env = lamps(n)
    gp, op = _policies(oracle, n)
    oracle.set_det_exp(True)
    try:
        for det in (True, False):
            for ns in (1, 3):
                ge = tw.collector.evaluate(env, gp, num_episodes=40, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=5, C=1.41,
                                           max_expand_depth=1, num_cores=4)
                _device_kernel_ran(_lib.TW_KERNEL_SOLVE_BIG, n, (40 * ns + 15) // 16)
                oe = oracle.evaluate_env(VarHostEnv(env), op, 40, det, ns, 0, 1.41, 1, seed=5, difficulty=DIFFICULTY)
                he = _host_evaluate(env, gp, 40, det, ns, 5)
                assert f32_bits(ge[0]) == f32_bits(oe[0]) == f32_bits(he[0]) and f32_bits(ge[1]) == f32_bits(oe[1]) == f32_bits(he[1]), (det, ns, ge, oe, he)
    finally:
        oracle.set_det_exp(False)


@pytest.mark.parametrize("n", SIZES)
def test_self_play_on_the_host_stepped_path_equals_the_oracle(tw, oracle, n):
    env = lamps(n, max_steps=9)
    gp, op = _policies(oracle, n)
    z = tw.collector.AZCollector(12, 8, 1.41, 1, 4).collect(env, gp, seed=11)
    oracle.set_det_exp(True)
    try:
        o = oracle_az_loop(oracle, VarHostEnv(env), op, 12, 8, 1.41, 1, 11, n, difficulty=DIFFICULTY)
    finally:
        oracle.set_det_exp(False)
    a = z.to_numpy()
    assert z.ragged and a["obs"].dtype == np.uint16 and np.array_equal(a["obs"], o.obs) and z.obs == o.obs_lists
    assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits)) and np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.remaining_values))
    assert np.array_equal(a["ep_len"], o.ep_len) and set(a["perms"].tolist()) == {-1}
    assert int(o.counts.min()) == 0 or int(o.counts.max()) > int(o.counts.min())


def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


@pytest.mark.parametrize("bad_at", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_a_bad_id_and_a_bad_count_fail_alike_on_both_paths(tw, oracle, n, bad_at):
    """From step bad_at on the environment returns an id outside [0, obs_size) (kind 1) or a count of N_OBS + 1 (kind 2): the device
    path and the host-stepped path raise the same exception with the same message, which names the FIRST occurrence -- the smallest
    record index, then the smallest episode (worked out here from the oracle's collect of the valid environment: the episodes are the
    same up to that record).  Nothing faults: the next collect on the same environment object and policy succeeds."""
    from twisterl_amd import _lib
    gp, _ = _policies(oracle, n)
    good = shared_collect(n)
    for kind in (1, 2):
        env = lamps(n, bad_at=bad_at, bad_kind=kind)
        # where each episode first meets the bad observation: from record bad_at on, two records later in every third episode; kind 1
        # needs a record that has an id.  The first occurrence is the smallest record index, then the smallest episode -- not episode 0
        starts = [bad_at + (2 if e % 3 == 0 else 0) for e in range(E)]
        hits = [(next((t for t in range(starts[e], len(ep)) if kind == 2 or len(ep[t]) > 0), None), e) for e, ep in enumerate(good.episodes)]
        first = min((t, e) for t, e in hits if t is not None)[1]
        assert first not in (0, 3) and len(good.episodes[0]) > bad_at + 2
        if kind == 1:
            want = f"index out of bounds: obs id {(-1 - first % 7) if first & 1 else (n * n + first % 5)}, obs_size {n * n}"
        else:
            want = f"observation of {n + 1} ids, at most {n}"
        dev = _message(lambda: tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, gp, seed=SEED))
        _device_kernel_ran(_lib.TW_KERNEL_ROLLOUT_BIG, n, (E + 15) // 16)
        host = _message(lambda: _host_collect(env, gp, E, SEED))
        assert dev == host == (ValueError, want), (kind, dev, host, want)
        dev = _message(lambda: tw.collector.evaluate(env, gp, 24, False, 2, 0, 1, 1.41, 1, 1))
        host = _message(lambda: _host_evaluate(env, gp, 24, False, 2, 1))
        assert dev == host and dev[0] is ValueError and dev[1].startswith(want.split(" id")[0]), (kind, dev, host)
        # the same handles afterwards: the struct with bad_at switched off is the valid environment again
        raw = bytearray(env.state_bytes())
        struct.pack_into("<i", raw, BAD_AT_OFFSET, -1)
        env.set_state_bytes(bytes(raw))
        g = tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, gp, seed=SEED)
        assert g.stats["rollout_threads"] == 256
        _same_as_loop(g, good, n)


def _onehot(obs_lists, obs_size):
    out = np.zeros((len(obs_lists), obs_size), dtype=np.float32)
    for i, ids in enumerate(obs_lists):
        out[i, ids] = 1.0
    return out


@pytest.mark.parametrize("n", SIZES)
def test_trainer_hand_off_of_a_ragged_result(tw, oracle, n):
    from twisterl_amd import _lib
    from twisterl_amd.trainer import ppo_data_to_torch
    gp, _ = _policies(oracle, n)
    g = tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(lamps(n), gp, seed=SEED)
    o = shared_collect(n)
    want = _onehot(o.obs_lists, n * n)
    t = ppo_data_to_torch(g, n * n)
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"]) == (_lib.TW_KERNEL_ONEHOT, 2), info
    assert np.array_equal(t[0].cpu().numpy(), want) and t[0].shape == want.shape
    assert np.array_equal(want.sum(axis=1), o.counts.astype(np.float32))
    total = len(o.obs_lists)
    for lo, hi in ((0, 1), (1, 18), (total - 33, total), (7, 7)):
        part = ppo_data_to_torch(g, n * n, rows=(lo, hi))
        assert np.array_equal(part[0].cpu().numpy(), want[lo:hi]), (lo, hi)
        assert np.array_equal(f32_bits(part[1].cpu().numpy()), f32_bits(t[1].cpu().numpy()[lo:hi]))
    with pytest.raises(ValueError, match=f"obs_size {n * n + 1}"):
        ppo_data_to_torch(g, n * n + 1)


def test_trainer_hand_off_of_a_fixed_length_environment_with_more_than_256_ids(tw):
    """ring(n=200): two ids per state out of 400 -- two-byte ids, which tw_collected_pack_trainer refused before the scatter form."""
    from twisterl_amd import _lib
    from twisterl_amd.trainer import ppo_data_to_torch
    env = ring(n=200, max_steps=30, difficulty=5, noise=0.2, max_records=31)
    gp = amd_policy(make_deep_policy_arrays(20, seed=8, emb=64, common=(64, 32), n_actions=3))
    g = tw.collector.PPOCollector(70, 0.99, 0.95, 4).collect(env, gp, seed=13)
    a = g.to_numpy()
    assert not g.ragged and a["obs"].dtype == np.uint16 and a["obs"].shape[1] == 2 and int(a["obs"].max()) > 255
    want = _onehot(a["obs"].astype(np.int64).tolist(), 400)
    t = ppo_data_to_torch(g, 400)
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"]) == (_lib.TW_KERNEL_ONEHOT, 2), info
    assert np.array_equal(t[0].cpu().numpy(), want)
    assert np.array_equal(ppo_data_to_torch(g, 400, rows=(5, 40))[0].cpu().numpy(), want[5:40])


def test_a_python_environment_with_max_obs(tw, oracle):
    arrs = make_deep_policy_arrays(6, seed=4, emb=32, common=(32, 32), n_actions=4)
    gp, op = amd_policy(arrs), oracle_policy(oracle, arrs)
    env = tw.env.PyEnv(PyLamps())
    env.difficulty = 3
    g = tw.collector.PPOCollector(20, GAMMA, LAM, 1).collect(env, gp, seed=7)
    o = oracle_ppo_loop(oracle, PyLamps(), op, 20, GAMMA, LAM, 7, 6, difficulty=3)
    _same_as_loop(g, o, 6)
    assert len(set(o.counts.tolist())) >= 3
    fixed = PyLamps(declare_max=False)                    # without max_obs(): the prototype's two ids are THE length, as before
    fixed.mask = 0b11
    with pytest.raises(ValueError, match="needs a fixed number of obs ids per state"):
        tw.collector.PPOCollector(20, GAMMA, LAM, 1).collect(tw.env.PyEnv(fixed), gp, seed=7)


def test_the_gather_refuses_a_ragged_result(tw, oracle):
    import os
    import torch.distributed as dist
    from twisterl_amd.dist import Comm, RcclGather, collect_sharded
    gp, _ = _policies(oracle, 12)
    env = lamps(12)
    g = tw.collector.PPOCollector(20, GAMMA, LAM, 4, merge_order=False).collect(env, gp, seed=SEED)
    assert g.ragged
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29541")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        comm = Comm()
        rg = RcclGather(comm, 0, 1, 0, 0, 20, True, 12)
        with pytest.raises(RuntimeError, match="variable-length observations .*cannot be gathered yet"):
            rg.submit(g, 0)
        with pytest.raises(RuntimeError, match="variable-length observations"):
            collect_sharded(tw.collector.PPOCollector(20, GAMMA, LAM, 4), env, gp, seed=SEED)
        comm.close()
    finally:
        dist.destroy_process_group()
