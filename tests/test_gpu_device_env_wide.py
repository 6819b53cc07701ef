"""GPU: device environments of 5 .. 31 actions (tests/device_env_wide.py: the hash walk of tests/device_envs/wide.hpp with 5, 8, 16, 17
and 31 actions, examples/device_env/permutation.hpp with 28, and a struct of three actions built with the opt-in) through the SAME two
device kernels -- PPO collect plain and queued on 16 columns, evaluate deterministic and sampled, plain and queued -- against the
host-stepped path over the module's own vtable (byte for byte, dtype and shape included) and the oracle's restatement running the
struct's host code (field by field).  Every case first asserts through tw_debug_last_launch that the device kernel ran: the big-board
family, nt = 1, the row's EngineV width, persist -- a host-stepped fall-back does not pass as the feature.  EVERYTHING IS BITWISE: no
tolerance appears anywhere but in the trainer hand-off, whose float64 bounds are those of tests/test_gpu_trainer_handoff.py (tests/ref64.py).
The oracle's collects are computed once (device_env_wide.shared_collect: the ones tests/test_device_env_wide_build.py holds the input
conditions against) and shared.

Deliberate breaks, each tried once on the MI355X against this file; "all six" = the rows of more than four actions, and with
test_ppo_collect of a row its queued form, the bad-id case of the 31-action row and the hand-off of the rows it covers failed too:
  act_perms[perm * 4 + i]                          test_ppo_collect and test_evaluate [wideo5a8v, wideo16a16, wideo64a31] (the rows with twists)
  the draw index without (i >> 2) << 24            test_ppo_collect [all six] (another action: other episodes, other record counts)
  word i & 3 taken as i % A                        test_ppo_collect [all six]
  the mask tested on i & 7                         test_ppo_collect [wideo16a16, wideo17a17, wideo64a31, perm8] (5 and 8 actions cannot tell)
  the head read with lds_out's column stride of 8  test_ppo_collect [all six]
  2A passed to the compaction as A                 test_ppo_collect [all six] (logits)
"""
import ctypes as C
import functools
import signal

import numpy as np
import pytest

from tests import ref64
from tests.device_env_search_util import host_az_collect, host_evaluate
from tests.device_env_wide import (AZ_ROW, BY_MODULE, E, ERROR_ROW, EVAL_SEED_OFFSET, GAMMA, HANDOFF_ROWS, IDS, LAM, PERM8, engine_nc, host_env,
                                   make_env, policies, shared_collect)
from tests.util import f32_bits
from tests.var_obs_util import NO_ID

pytestmark = pytest.mark.gpu
BLOCKS = (E + 15) // 16


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code; a hang inside a HIP call is bounded by the `timeout`
    around the pytest run."""
    def boom(*_):
        raise TimeoutError("wide device-environment test exceeded its time limit")
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


@pytest.fixture()
def det_exp(oracle):
    """The oracle's soft-max with the deterministic exp, as the library's."""
    oracle.set_det_exp(True)
    yield oracle
    oracle.set_det_exp(False)


@functools.lru_cache(maxsize=None)
def _setup(module):
    """(row, the environment, the library's policy, the oracle's): once per row."""
    from oracle import oracle as O
    O.build()
    r = BY_MODULE[module]
    gp, op = policies(O, r)
    return r, make_env(r), gp, op


def _hook(groups):
    from twisterl_amd import _lib
    return _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups)


def _assert_launch(family, r, persist, blocks):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["persist"], info["blocks"], info["threads"]) == \
        (family, 1, engine_nc(r.n_obs), persist, blocks, 256), info


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k
    assert a.ragged == b.ragged


def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def _host_collect(env, policy, seed):
    """tw_ppo_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.PPOParams(E, 0, GAMMA, LAM, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _ppo_same_as_oracle(g, o, r):
    a = g.to_numpy()
    assert a["obs"].dtype == (np.uint8 if not r.var and r.obs_size <= 256 else np.uint16), a["obs"].dtype
    assert a["obs"].shape[1] == r.n_obs and a["logits"].shape[1] == r.A and a["logits"].dtype == np.float32 and bool(g.ragged) is r.var
    assert a["obs"].shape == o.obs.shape and np.array_equal(a["obs"].astype(np.uint16), o.obs)       # the ids AND the 0xFFFF padding
    assert np.array_equal(a["actions"].astype(np.int64), o.actions), "actions"
    assert np.array_equal(a["perms"].astype(np.int32), o.perms), "perms"
    for k in ("logits", "values", "rewards", "advs", "rets"):
        assert a[k].shape == getattr(o, k).shape and np.array_equal(f32_bits(a[k]), f32_bits(getattr(o, k))), k
    assert np.array_equal(a["ep_len"], o.ep_len)
    if r.var:
        assert g.obs == o.obs_lists and np.array_equal((a["obs"] != NO_ID).sum(axis=1), o.counts)


def _collect(tw, r, env, gp):
    return tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, gp, seed=r.seed)


# ---- 1. PPO collect, one column per episode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", IDS)
def test_ppo_collect(tw, module):
    check_ppo_collect(tw, module)


def check_ppo_collect(tw, module):
    """-> the device collect that was checked"""
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(module)
    g = _collect(tw, r, env, gp)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, BLOCKS)
    assert g.stats["rollout_blocks"] == BLOCKS and g.stats["rollout_threads"] == 256
    h = _host_collect(env, gp, r.seed)
    assert h.stats["rollout_threads"] == 0
    _ppo_same_as_oracle(g, shared_collect(module), r)
    _same_bytes(g, h)
    return g


# ---- 2. PPO collect on a persistent grid of ONE workgroup: 40 episodes on 16 columns -----------------------------------------------------------
@pytest.mark.parametrize("module", IDS)
def test_ppo_collect_queued(tw, module):
    check_ppo_collect_queued(tw, module)


def check_ppo_collect_queued(tw, module):
    """-> the collect on the persistent grid that was checked"""
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(module)
    with _hook(1):
        g = _collect(tw, r, env, gp)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 1, 1)
        assert g.stats["rollout_blocks"] == 1 and g.stats["rollout_threads"] == 256
    _ppo_same_as_oracle(g, shared_collect(module), r)
    _same_bytes(g, _host_collect(env, gp, r.seed))
    return g


# ---- 3. evaluate: deterministic and sampled, 2 attempts per episode; plain and queued ------------------------------------------------------------
@pytest.mark.parametrize("module", IDS)
def test_evaluate(tw, det_exp, module):
    from twisterl_amd import _lib
    r, env, gp, op = _setup(module)
    seed = r.seed + EVAL_SEED_OFFSET
    n, ns = E, 2
    for det in (True, False):
        ev = lambda: tw.collector.evaluate(env, gp, num_episodes=n, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=seed, C=1.41,
                                           max_expand_depth=1, num_cores=4)
        pe = ev()
        _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 0, (n * ns + 15) // 16)
        pa = _lib.debug_last_attempts()
        assert len(pa[0]) == n * ns and 1 <= int(pa[2].max()) <= r.max_records - 1
        he = host_evaluate(env, gp, n, det, ns, 0, seed)
        oe = det_exp.evaluate_env(host_env(env), op, n, det, ns, 0, 1.41, 1, seed=seed, difficulty=r.diff)
        for other in (he, oe):
            assert f32_bits(pe[0]) == f32_bits(other[0]) and f32_bits(pe[1]) == f32_bits(other[1]), (module, det, pe, other)
        with _hook(1):
            ge = ev()
            _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 1, 1)
            ga = _lib.debug_last_attempts()
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(ga, pa)), (module, det)
        assert f32_bits(ge[0]) == f32_bits(pe[0]) and f32_bits(ge[1]) == f32_bits(pe[1]), (module, det, ge, pe)


# ---- 4. a bad id at step 0 and at step 3 of the 31-action row: the host path's message and first-occurrence rule ---------------------------------
@pytest.mark.parametrize("bad_at", [0, 3])
def test_bad_ids_fail_alike(tw, bad_at):
    from twisterl_amd import _lib
    r, ok, gp, _ = _setup(ERROR_ROW)
    env = make_env(r, bad_at=bad_at)
    want = "index out of bounds: obs id "
    dev = _message(lambda: _collect(tw, r, env, gp))
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, BLOCKS)
    host = _message(lambda: _host_collect(env, gp, r.seed))
    assert dev == host and dev[0] is ValueError and dev[1].startswith(want) and dev[1].endswith(f", obs_size {r.obs_size}"), (dev, host)
    with _hook(1):
        q = _message(lambda: _collect(tw, r, env, gp))
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 1, 1)
    assert q == host, (q, host)
    ev = lambda: tw.collector.evaluate(env, gp, 24, False, 2, 0, r.seed, 1.41, 1, 1)
    dev = _message(ev)
    _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 0, 3)
    host = _message(lambda: host_evaluate(env, gp, 24, False, 2, 0, r.seed))
    assert dev == host and dev[0] is ValueError and dev[1].startswith(want), (dev, host)
    with _hook(1):
        q = _message(ev)
        _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 1, 1)
    assert q == host, (q, host)
    g = _collect(tw, r, ok, gp)                                                # the device and the handles are fine afterwards
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, BLOCKS)
    _ppo_same_as_oracle(g, shared_collect(ERROR_ROW), r)


# ---- 5. trainer hand-off of the 17- and 31-action results: the float64 checks of tests/test_gpu_trainer_handoff.py --------------------------------
@pytest.mark.parametrize("module", HANDOFF_ROWS)
def test_trainer_hand_off_against_float64(tw, module):
    import torch
    from twisterl_amd import _lib, trainer
    r, env, gp, _ = _setup(module)
    g = _collect(tw, r, env, gp)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, BLOCKS)
    a = g.to_numpy()
    assert a["logits"].shape == (len(g), r.A)
    obs, logp, acts, advs, rets, perm = trainer.ppo_data_to_torch(g, r.obs_size, normalize_advantage=True)
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_ONEHOT
    got = obs.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, ref64.onehot_ref(a["obs"], r.obs_size))
    want = ref64.log_prob_f64(a["logits"], a["actions"])
    dev = np.abs(logp.cpu().numpy().astype(np.float64) - want)
    bound = ref64.log_prob_bound(r.A, want)
    print(f"[handoff-tol] {module}: log-prob worst |GPU - f64| {dev.max():.3e}, largest share of its bound {np.max(dev / bound):.3f}")
    assert logp.dtype == torch.float32 and np.all(dev <= bound)
    want = ref64.normalized_adv_f64(a["advs"])
    dev = np.abs(advs.cpu().numpy().astype(np.float64) - want)
    bound = ref64.normalized_adv_bound(a["advs"], want)
    print(f"[handoff-tol] {module}: normalised advantage worst |GPU - f64| {dev.max():.3e}, largest share of its bound {np.max(dev / bound):.3f}")
    assert np.all(dev <= bound)
    assert np.array_equal(acts.cpu().numpy(), a["actions"].astype(np.int64)) and np.array_equal(perm.cpu().numpy(), a["perms"].astype(np.int64))
    assert np.array_equal(f32_bits(rets.cpu().numpy()), f32_bits(a["rets"]))
    th = trainer.ppo_data_to_torch(_host_collect(env, gp, r.seed), r.obs_size, normalize_advantage=True)
    for x, y in zip((obs, logp, acts, advs, rets, perm), th):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


# ---- 6. self-play and MCTS-evaluate of a wide module: host-stepped, and said so ----------------------------------------------------------------------
def test_self_play_of_a_wide_module_is_host_stepped(tw):
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(AZ_ROW)
    assert env.search is False
    g = tw.collector.AZCollector(E, 4, 1.41, 1, 4).collect(env, gp, seed=r.seed)
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    h = host_az_collect(env, gp, E, 4, 1.41, 1, r.seed)
    _same_bytes(g, h)
    assert g.to_numpy()["logits"].shape[1] == r.A
    ge = tw.collector.evaluate(env, gp, num_episodes=8, deterministic=True, num_searches=1, num_mcts_searches=4, seed=r.seed, C=1.41,
                               max_expand_depth=1, num_cores=4)
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    he = host_evaluate(env, gp, 8, True, 1, 4, r.seed)
    assert f32_bits(ge[0]) == f32_bits(he[0]) and f32_bits(ge[1]) == f32_bits(he[1])


# ---- 7. the example through the Python surface ---------------------------------------------------------------------------------------------------------
def test_permutation_example_through_the_python_surface(tw):
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(PERM8)
    assert env.num_actions() == 28 and env.obs_shape() == [8, 8] and env.difficulty == 2
    env.reset(seed=3, episode=5)
    assert env.masks() == [True] * 28
    before = env.observe()
    assert sorted(i % 8 for i in before) == list(range(8)) and [i // 8 for i in before] == list(range(8))
    env.step(9)                                                               # the pair (1, 4)
    after = env.observe()
    assert [after[k] % 8 for k in (1, 4)] == [before[k] % 8 for k in (4, 1)] and all(after[k] == before[k] for k in (0, 2, 3, 5, 6, 7))
    assert env.masks() == [k != 9 for k in range(28)]
    with pytest.raises(ValueError):
        env.step(28)
    g = tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, gp, seed=r.seed)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, BLOCKS)
    a = g.to_numpy()
    assert a["logits"].shape == (len(g), 28) and a["obs"].dtype == np.uint8 and int(a["actions"].max()) >= 4
    _ppo_same_as_oracle(g, shared_collect(PERM8), r)
