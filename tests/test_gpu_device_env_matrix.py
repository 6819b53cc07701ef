"""GPU: every row of the device-environment matrix (tests/device_env_matrix.py: the probe struct of tests/device_envs/probe.hpp at
every EngineV class and class edge, NUM_ACTIONS 1..4, the obs_size edges, structs that live in scratch memory, observe_n, episodes
that are final at reset) through the device kernels -- PPO collect plain and queued, evaluate plain and queued, and for the rows
built with the search kernel self-play and MCTS-guided evaluate -- against the host-stepped path over the module's own vtable
(byte for byte, dtype and shape included) and the oracle's restatement running the same struct's host code (field by field).
Every case first asserts, through tw_debug_last_launch and the result's stats, that the device kernel ran: family, nt = 1, the
module's EngineV width, grid, persist.  EVERYTHING IS BITWISE: no tolerance appears anywhere.  The oracle's PPO collects are computed
once (device_env_matrix.shared_collect: the ones tests/test_device_env_matrix.py holds the input conditions against) and shared."""
import ctypes as C
import functools
import signal

import numpy as np
import pytest

from tests.device_env_matrix import (BY_MODULE, EPISODES, ERROR_ROWS, EVAL_SEED_OFFSET, GAMMA, HANDOFF_ROWS, IDS, LAM, SEARCH_IDS, engine_nc,
                                     host_env, policies, probe, shared_collect)
from tests.device_env_search_util import host_az_collect, host_evaluate
from tests.util import f32_bits
from tests.var_obs_util import NO_ID, oracle_az_loop

pytestmark = pytest.mark.gpu
AZ_FIELDS = ("obs", "logits", "perms", "remaining_values", "ep_len", "ep_start")
# self-play: (episodes, num_mcts_searches, max_expand_depth) -- S in {1, 6} x max_expand_depth in {0, 1, 2}; 100 episodes once
AZ_CASES = [(40, 6, 2), (40, 6, 1), (40, 6, 0), (100, 1, 0), (40, 1, 1), (40, 1, 2)]


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code.  A signal handler runs only when control returns to
    the interpreter, so a hang inside a HIP call is bounded by the `timeout` around the pytest run, not by this."""
    def boom(*_):
        raise TimeoutError("device-environment matrix test exceeded its time limit")
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
    return r, probe(r), gp, op


def _hook(groups):
    from twisterl_amd import _lib
    return _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups)


def _assert_launch(family, r, persist, blocks):
    """The last call ran the module's own kernel: family with nt 1, the EngineV width of the row's class, the grid, persistent or not."""
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


def _host_collect(env, policy, E, seed, offset=0):
    """tw_ppo_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.PPOParams(E, offset, GAMMA, LAM, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _obs_form(g, r):
    """The obs field's form: one-byte ids exactly when the row is fixed-length with at most 256 ids; ragged exactly for observe_n."""
    a = g.to_numpy()
    assert a["obs"].dtype == (np.uint8 if not r.var and r.obs_size <= 256 else np.uint16), a["obs"].dtype
    assert a["obs"].shape[1] == r.n_obs and a["logits"].shape[1] == r.A and a["logits"].dtype == np.float32
    assert bool(g.ragged) is r.var
    return a


def _ppo_same_as_oracle(g, o, r):
    a = _obs_form(g, r)
    assert a["obs"].shape == o.obs.shape and np.array_equal(a["obs"].astype(np.uint16), o.obs)       # the ids AND the 0xFFFF padding
    assert np.array_equal(a["actions"].astype(np.int64), o.actions) and np.array_equal(a["perms"].astype(np.int32), o.perms)
    for k in ("logits", "values", "rewards", "advs", "rets"):
        assert a[k].shape == getattr(o, k).shape and np.array_equal(f32_bits(a[k]), f32_bits(getattr(o, k))), k
    assert np.array_equal(a["ep_len"], o.ep_len)
    if r.var:
        assert g.obs == o.obs_lists and np.array_equal((a["obs"] != NO_ID).sum(axis=1), o.counts)


def _collect(tw, r, env, gp, E):
    return tw.collector.PPOCollector(E, GAMMA, LAM, 4, episode_offset=r.offset).collect(env, gp, seed=r.seed)


# ---- 1. PPO collect, one column per episode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("module", IDS)
def test_ppo_collect(tw, module, E):
    check_ppo_collect(tw, module, E)


def check_ppo_collect(tw, module, E):
    """-> the device collect that was checked"""
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(module)
    g = _collect(tw, r, env, gp, E)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, (E + 15) // 16)
    assert g.stats["rollout_blocks"] == (E + 15) // 16 and g.stats["rollout_threads"] == 256
    h = _host_collect(env, gp, E, r.seed, offset=r.offset)
    assert h.stats["rollout_threads"] == 0
    _same_bytes(g, h)
    _ppo_same_as_oracle(g, shared_collect(module, E), r)
    return g


# ---- 2. PPO collect on a persistent grid of one and two workgroups: 100 episodes on 16 (32) columns, every column takes several -------------------
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("module", IDS)
def test_ppo_collect_queued(tw, module, groups):
    check_ppo_collect_queued(tw, module, groups)


def check_ppo_collect_queued(tw, module, groups):
    """-> the collect on the persistent grid that was checked"""
    from twisterl_amd import _lib
    r, env, gp, _ = _setup(module)
    E = 100
    with _hook(groups):
        g = _collect(tw, r, env, gp, E)
        _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 1, groups)
        assert g.stats["rollout_blocks"] == groups and g.stats["rollout_threads"] == 256
    p = _collect(tw, r, env, gp, E)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, (E + 15) // 16)
    _same_bytes(g, p)
    _ppo_same_as_oracle(g, shared_collect(module, E), r)
    return g


# ---- 3. evaluate without MCTS: deterministic (100 attempts) and sampled with 2 searches (80 attempts); plain and queued ---------------------------
@pytest.mark.parametrize("module", IDS)
def test_evaluate(tw, det_exp, module):
    from twisterl_amd import _lib
    r, env, gp, op = _setup(module)
    seed = r.seed + EVAL_SEED_OFFSET
    for det, n, ns in ((True, 100, 1), (False, 40, 2)):
        ev = lambda: tw.collector.evaluate(env, gp, num_episodes=n, deterministic=det, num_searches=ns, num_mcts_searches=0, seed=seed, C=1.41,
                                           max_expand_depth=1, num_cores=4)
        pe = ev()
        _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 0, (n * ns + 15) // 16)
        pa = _lib.debug_last_attempts()
        assert len(pa[0]) == n * ns and (pa[2] == 0).any() and int(pa[2].max()) <= r.max_steps       # (0 moves: final at reset)
        he = host_evaluate(env, gp, n, det, ns, 0, seed)
        oe = det_exp.evaluate_env(host_env(env), op, n, det, ns, 0, 1.41, 1, seed=seed, difficulty=r.diff)
        for other in (he, oe):
            assert f32_bits(pe[0]) == f32_bits(other[0]) and f32_bits(pe[1]) == f32_bits(other[1]), (module, det, pe, other)
        for groups in (1, 2):
            with _hook(groups):
                ge = ev()
                _assert_launch(_lib.TW_KERNEL_SOLVE_BIG, r, 1, groups)
                ga = _lib.debug_last_attempts()
            assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(ga, pa)), (module, det, groups)
            assert f32_bits(ge[0]) == f32_bits(pe[0]) and f32_bits(ge[1]) == f32_bits(pe[1]), (module, det, groups, ge, pe)


# ---- 4. search rows: self-play ------------------------------------------------------------------------------------------------------------------------
def _assert_search_launch(r, columns, solve):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["persist"], info["blocks"], info["threads"]) == \
        (_lib.TW_KERNEL_MCTS_BIG, 1, engine_nc(r.n_obs), 0, (columns + 15) // 16, 256), info


class _Counted:
    """Counts the oracle policy's full_predict calls: one per evaluated state, a root or a leaf."""

    def __init__(self, pol):
        self.pol, self.n = pol, 0

    def __getattr__(self, name):
        return getattr(self.pol, name)

    def full_predict(self, *a, **kw):
        self.n += 1
        return self.pol.full_predict(*a, **kw)


@pytest.mark.parametrize("E,S,med", AZ_CASES)
@pytest.mark.parametrize("module", SEARCH_IDS)
def test_self_play(tw, det_exp, module, E, S, med):
    check_self_play(tw, det_exp, module, E, S, med)


def check_self_play(tw, det_exp, module, E, S, med):
    """-> the device self-play that was checked"""
    r, env, gp, op = _setup(module)
    g = tw.collector.AZCollector(E, S, 1.41, med, 4, episode_offset=r.offset).collect(env, gp, seed=r.seed)
    _assert_search_launch(r, E, False)
    assert g.stats["rollout_blocks"] == (E + 15) // 16 and g.stats["rollout_threads"] == 256
    h = host_az_collect(env, gp, E, S, 1.41, med, r.seed, offset=r.offset)
    x = g.to_numpy()
    assert sorted(x) == sorted(AZ_FIELDS)
    _same_bytes(g, h)
    a = _obs_form(g, r)
    cop = _Counted(op)
    o = oracle_az_loop(det_exp, host_env(env), cop, E, S, 1.41, med, r.seed, r.n_obs, episode_offset=r.offset, difficulty=r.diff)
    assert a["obs"].shape == o.obs.shape and np.array_equal(a["obs"].astype(np.uint16), o.obs)
    assert np.array_equal(a["ep_len"], o.ep_len) and set(a["perms"].tolist()) == {-1}
    assert a["logits"].shape == o.logits.shape and np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
    assert np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.remaining_values))
    if r.var:
        assert g.obs == o.obs_lists
    assert 1 in o.ep_len.tolist() and len(set(o.ep_len.tolist())) >= 3                 # episodes final at reset are searched and recorded too
    assert g.stats["forward_evals"] == cop.n * max(r.twists, 1), (g.stats["forward_evals"], cop.n, r.twists)
    return g


# ---- 5. search rows: MCTS-guided evaluate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", SEARCH_IDS)
def test_mcts_evaluate(tw, det_exp, module):
    r, env, gp, op = _setup(module)
    seed = r.seed + EVAL_SEED_OFFSET
    for det, ns, S, med in ((True, 1, 6, 1), (False, 2, 4, 2)):
        n = 24
        ge = tw.collector.evaluate(env, gp, num_episodes=n, deterministic=det, num_searches=ns, num_mcts_searches=S, seed=seed, C=1.41,
                                   max_expand_depth=med, num_cores=4)
        _assert_search_launch(r, n * ns, True)
        he = host_evaluate(env, gp, n, det, ns, S, seed, med=med)
        oe = det_exp.evaluate_env(host_env(env), op, n, det, ns, S, 1.41, med, seed=seed, difficulty=r.diff)
        for other in (he, oe):
            assert f32_bits(ge[0]) == f32_bits(other[0]) and f32_bits(ge[1]) == f32_bits(other[1]), (module, det, ge, other)


# ---- 6. errors: a struct in scratch memory and a struct with ONE action; the same exception and text as the host path --------------------------------
@pytest.mark.parametrize("bad_at", [0, 3])
@pytest.mark.parametrize("module", ERROR_ROWS)
def test_bad_ids_fail_alike(tw, module, bad_at):
    from twisterl_amd import _lib
    r, ok, gp, _ = _setup(module)
    env = probe(r, bad_at=bad_at)
    E = 40
    want = "index out of bounds: obs id "
    dev = _message(lambda: _collect(tw, r, env, gp, E))
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, 3)
    host = _message(lambda: _host_collect(env, gp, E, r.seed, offset=r.offset))
    assert dev == host and dev[0] is ValueError and dev[1].startswith(want) and dev[1].endswith(f", obs_size {r.obs_size}"), (dev, host)
    with _hook(1):
        q = _message(lambda: _collect(tw, r, env, gp, E))
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
    dev = _message(lambda: tw.collector.AZCollector(E, 6, 1.41, 2, 4).collect(env, gp, seed=r.seed))
    _assert_search_launch(r, E, False)
    host = _message(lambda: host_az_collect(env, gp, E, 6, 1.41, 2, r.seed))
    assert dev == host and dev[0] is ValueError and dev[1].startswith(want), (dev, host)
    dev = _message(lambda: tw.collector.evaluate(env, gp, 16, False, 2, 6, r.seed, 1.41, 1, 1))
    _assert_search_launch(r, 32, True)
    host = _message(lambda: host_evaluate(env, gp, 16, False, 2, 6, r.seed))
    assert dev == host and dev[0] is ValueError and dev[1].startswith(want), (dev, host)
    # the device and the handles are fine afterwards: one healthy collect
    g = _collect(tw, r, ok, gp, E)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, 3)
    _ppo_same_as_oracle(g, shared_collect(module, E), r)


# ---- 7. trainer hand-off: one-byte ids (obs_size 256) and two-byte ids (257, 65535) -------------------------------------------------------------------
@pytest.mark.parametrize("module", HANDOFF_ROWS)
def test_trainer_hand_off_equals_the_host_collect(tw, module):
    import torch
    from twisterl_amd import _lib
    from twisterl_amd.trainer import ppo_data_to_torch
    r, env, gp, _ = _setup(module)
    E = 40
    g = _collect(tw, r, env, gp, E)
    _assert_launch(_lib.TW_KERNEL_ROLLOUT_BIG, r, 0, 3)
    h = _host_collect(env, gp, E, r.seed, offset=r.offset)
    tg = ppo_data_to_torch(g, r.obs_size)
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"]) == (_lib.TW_KERNEL_ONEHOT, 0 if r.obs_size <= 256 and not r.var else 2), info
    th = ppo_data_to_torch(h, r.obs_size)
    assert len(tg) == len(th) == 6
    for x, y in zip(tg, th):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
    o = shared_collect(module, E)                                              # ... and the one-hot of the oracle's ids
    want = np.zeros((len(o.obs_lists), r.obs_size), dtype=np.float32)
    for i, ids in enumerate(o.obs_lists):
        want[i, ids] = 1.0
    assert tg[0].shape == want.shape and np.array_equal(tg[0].cpu().numpy(), want)
