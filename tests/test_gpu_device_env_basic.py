"""GPU: a device environment under the reference's DEFAULT policy -- embedding -> ONE common Linear of 32 / 64 / 128 / 256 units -> linear
heads, obs_size <= 256: tw_policy_create's "MFMA shape" -- in a module built with basic=True (TW_DEVICE_ENV_BASIC).  Such a policy's
image has no EngineV layer table; the module's pack_basic_view_kernel builds one from the policy's live natural-layout arrays in front
of every launch, and the call runs in the module's f32 kernels instead of the host-stepped path.

Every case first checks WHICH kernel ran (tw_debug_last_launch: the family of the environment kernels, never TW_KERNEL_NONE -- a
fall-back cannot pass as the feature) and then holds the result, bit for bit, to the host-stepped path over the module's own vtable
(tw_ppo_collect_env / tw_evaluate_env / tw_solve_env32 / tw_az_collect_env, called directly), and to the oracle's ARITH_CHAIN loops where
the shared helpers give them.  Shapes: GridWorld 3 x 3 (obs_size 81), the ring (64), probes with 1 and 3 actions and obs_size 256 | 257,
Lamps 12 (observe_n), and 5 and 28 actions on wide modules; 16 and 40 episodes (one full workgroup of columns, and a ragged last one),
the persistent grid at 40; H = 32 (one block of two tiles) and 256 (four blocks, tb = 4), E = 32 and 96, two twists, emb_relu on and
off."""
import ctypes as C
import functools
import signal

import numpy as np
import pytest

from tests import device_env_solve as D
from tests.device_env_matrix import PROBE_HPP, host_env
from tests.device_env_search_util import host_az_collect, host_evaluate
from tests.device_env_util import GRIDWORLD_HPP, RING_HPP, HostEnv, gridworld
from tests.device_env_wide import PERM_HPP, WIDE_HPP
from tests.util import f32_bits, make_policy_arrays_obs, oracle_policy
from tests.var_obs_util import LAMPS_HPP

pytestmark = pytest.mark.gpu
GAMMA, LAM = 0.99, 0.95
C_UCB = 1.41

# name -> (header, type, build flags, constructor parameters, max_records)
MODULES = {
    "gw3_basic":     (GRIDWORLD_HPP, "tw_examples::GridWorld3x3", {}, [3, 3, 12, 4], 13),
    "gw3_basic_az":  (GRIDWORLD_HPP, "tw_examples::GridWorld3x3", {"search": True}, [3, 3, 12, 4], 13),
    "ring_basic":    (RING_HPP, "RingWalk", {}, [32, 12, 4, 0.1, -1], 13),
    "ring_basic_az": (RING_HPP, "RingWalk", {"search": True}, [32, 12, 4, 0.1, -1], 13),
    "o1a1_basic":    (PROBE_HPP, "ProbeO1A1", {}, [64, 9, 6, -1], 10),
    "o5a3v_basic":   (PROBE_HPP, "ProbeO5A3V", {}, [256, 10, 7, -1], 11),
    "lamps12_basic": (LAMPS_HPP, "Lamps12", {}, [10, 3, -1, 0], 11),
    "wide5_basic":   (WIDE_HPP, "WideO2A5", {"wide": True}, [64, 11, 8, -1], 12),
    "perm8_basic":   (PERM_HPP, "tw_examples::Permutation8", {"wide": True}, [8, 11, 2], 12),
    "wide5_basic_ws": (WIDE_HPP, "WideO2A5", {"wide_search": True}, [64, 11, 8, -1], 12),
}


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code; a hang inside a HIP call is bounded by the `timeout`
    around the pytest run."""
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


@functools.lru_cache(maxsize=None)
def _paths():
    """Every module once per session, side by side (at most 16 compilations at a time)."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    names = list(MODULES)
    with ThreadPoolExecutor(max_workers=min(16, len(names))) as pool:
        paths = list(pool.map(lambda n: build_device_env(MODULES[n][0], MODULES[n][1], n, basic=True, **MODULES[n][2]), names))
    return dict(zip(names, paths))


def _env(name, params=None):
    from twisterl_amd.env import DeviceEnv
    env = DeviceEnv(_paths()[name], name, list(params or MODULES[name][3]), max_records=MODULES[name][4])
    assert env.basic is True
    return env


def _policy(arrs, twists=((), ()), emb_relu=True):
    """tests.util.amd_policy with the embedding's ReLU as a switch."""
    from twisterl_amd import twisterl
    emb, eb, common, action, value = arrs
    seq = lambda ls: twisterl.nn.Sequential([twisterl.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    return twisterl.nn.Policy(twisterl.nn.EmbeddingBag(emb.tolist(), eb.tolist(), bool(emb_relu), [emb.shape[0]], 0),
                              seq(common), seq(action), seq(value), [list(p) for p in twists[0]], [list(p) for p in twists[1]])


def _arrs(obs_size, A, emb, hidden, seed):
    return make_policy_arrays_obs(obs_size, seed=seed, emb=emb, hidden=hidden, n_actions=A, scale=2.0)   # (logits that differ)


def _twists(obs_size, A, n, seed):
    """n seeded random permutations of the ids and of the actions (none of them the identity on purpose: full_predict averages over
    the untwisted pass and these)."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(obs_size).tolist() for _ in range(n)], [rng.permutation(A).tolist() for _ in range(n)]


def _launch():
    from twisterl_amd import _lib
    i = _lib.debug_last_launch()
    return i["family"], i["nt"], i["nw"], i["persist"], i["blocks"], i["threads"]


def _hook(groups):
    from twisterl_amd import _lib
    return _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups)


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k


def _host_collect(env, policy, E, seed):
    """tw_ppo_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.PPOParams(E, 0, GAMMA, LAM, seed, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def _collect(tw, env, gp, E, seed, persist=0, blocks=None):
    """PPOCollector.collect, held to the rollout kernel's launch."""
    from twisterl_amd import _lib
    g = tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, gp, seed=seed)
    assert _launch() == (_lib.TW_KERNEL_ROLLOUT_BIG, 1, 0, persist, (E + 15) // 16 if blocks is None else blocks, 256), _launch()
    return g


# ---- 1. PPO collect ------------------------------------------------------------------------------------------------------------------------
#        id               module           params  obs  A   emb  H   twists emb_relu  E  seed
PPO = [("gw3_h32_e32",   "gw3_basic",     None,    81,  4,  32,  32, 0,     True,    16, 11),
       ("gw3_h256_e96",  "gw3_basic",     None,    81,  4,  96, 256, 0,     False,   40, 12),
       ("gw3_h64_tw",    "gw3_basic",     None,    81,  4,  64,  64, 2,     True,    40, 13),
       ("ring_h128",     "ring_basic",    None,    64,  3,  32, 128, 2,     True,    40, 14),
       ("o1a1_h32",      "o1a1_basic",    None,    64,  1,  32,  32, 0,     True,    16, 15),
       ("o5a3v_obs256",  "o5a3v_basic",   None,   256,  3,  96,  64, 2,     False,   40, 16),
       ("lamps12_h64",   "lamps12_basic", None,   144,  4,  64,  64, 0,     True,    40, 17),
       ("wide5_h64",     "wide5_basic",   None,    64,  5,  32,  64, 2,     True,    40, 18),
       ("perm8_h256",    "perm8_basic",   None,    64, 28,  96, 256, 0,     True,    40, 19)]


def _case(row):
    _, module, params, obs, A, emb, H, n_tw, relu, E, seed = row
    env = _env(module, params)
    assert env.obs_size == obs and env.num_actions() == A
    arrs = _arrs(obs, A, emb, H, seed)
    twists = _twists(obs, A, n_tw, seed) if n_tw else ((), ())
    return env, arrs, twists, _policy(arrs, twists, relu), E, seed


@pytest.mark.parametrize("row", PPO, ids=[r[0] for r in PPO])
def test_ppo_collect_runs_in_the_rollout_kernel_with_the_host_paths_bytes(tw, row):
    env, arrs, twists, gp, E, seed = _case(row)
    g = _collect(tw, env, gp, E, seed)
    assert g.stats["rollout_threads"] == 256 and g.stats["rollout_blocks"] == (E + 15) // 16
    _same_bytes(g, _host_collect(env, gp, E, seed))
    a = g.to_numpy()
    assert a["logits"].shape[1] == row[4] and len(a["ep_len"]) == E and a["ep_len"].min() >= 1


def test_ppo_collect_equals_the_oracle(tw, oracle):
    """GridWorld 3 x 3, H = 64, two twists: the oracle's restatement of ppo.rs over the struct's host code (ARITH_CHAIN)."""
    env, arrs, twists, gp, E, seed = _case(PPO[2])
    g = _collect(tw, env, gp, E, seed)
    o = oracle.ppo_collect_env(HostEnv(env), oracle_policy(oracle, arrs, *twists), E, GAMMA, LAM, seed=seed, difficulty=4)
    a = g.to_numpy()
    assert np.array_equal(a["obs"].astype(np.int64), o.obs) and np.array_equal(a["actions"].astype(np.int64), o.actions)
    assert np.array_equal(a["perms"].astype(np.int32), o.perms) and np.array_equal(a["ep_len"], o.ep_len)
    for k, ok in (("logits", o.logits), ("values", o.values), ("rewards", o.rewards), ("advs", o.additional_data["advs"]),
                  ("rets", o.additional_data["rets"])):
        assert np.array_equal(f32_bits(a[k]), f32_bits(ok)), k


def test_obs_size_256_and_257_both_run_on_the_device(tw):
    """256 is the MFMA shape's last obs_size (the view); 257 is a generic stack by tw_policy_create's own rule and needs no flag.  Both
    run in the rollout kernel and agree with their host paths."""
    for obs in (256, 257):
        env = _env("o5a3v_basic", [obs, 10, 7, -1])
        gp = _policy(_arrs(obs, 3, 32, 32, 21), _twists(obs, 3, 2, 21))
        g = _collect(tw, env, gp, 40, 21)
        _same_bytes(g, _host_collect(env, gp, 40, 21))


def test_the_persistent_grid(tw):
    """40 episodes on ONE resident workgroup (the test hook): the view's block is packed once, in front of the persistent launch."""
    from twisterl_amd import _lib
    env, arrs, twists, gp, E, seed = _case(PPO[1])
    with _hook(1):
        g = _collect(tw, env, gp, E, seed, persist=1, blocks=1)
        s = tw.collector.evaluate(env, gp, 40, False, 1, 0, seed, C_UCB, 1, 1)
        assert _launch() == (_lib.TW_KERNEL_SOLVE_BIG, 1, 0, 1, 1, 256), _launch()
    _same_bytes(g, _host_collect(env, gp, E, seed))
    assert s == host_evaluate(env, gp, 40, False, 1, 0, seed)


# ---- 2. evaluate and solve without MCTS ------------------------------------------------------------------------------------------------------
ATTEMPTS = [PPO[0], PPO[1], PPO[3], PPO[4], PPO[5], PPO[6], PPO[7], PPO[8]]


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("row", ATTEMPTS, ids=[r[0] for r in ATTEMPTS])
def test_evaluate_and_solve_run_in_the_evaluate_kernel(tw, row, det):
    from twisterl_amd import _lib
    env, arrs, twists, gp, E, seed = _case(row)
    N = 3
    s = tw.collector.evaluate(env, gp, E, det, N, 0, seed, C_UCB, 1, 1)
    assert _launch() == (_lib.TW_KERNEL_SOLVE_BIG, 1, 0, 0, (E * N + 15) // 16, 256), _launch()
    assert s == host_evaluate(env, gp, E, det, N, 0, seed)
    D.start(env, seed, 3, 1)                                                  # a state no reset gives
    r = tw.collector.solve(env, gp, det, 17, 0, C_UCB, 1, seed=seed)
    assert _launch() == (_lib.TW_KERNEL_SOLVE_BIG, 1, 0, 0, 2, 256), _launch()
    assert D.same(r, D.host_solve(env, gp, det, 17, seed=seed))


@pytest.fixture()
def det_exp(oracle):
    oracle.set_det_exp(True)
    yield oracle
    oracle.set_det_exp(False)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "sampled"])
def test_solve_equals_the_oracle(tw, det_exp, det):
    """tests/device_env_solve.mfma_case()'s policy and start state, in the basic module: the oracle's solve from the same state."""
    from twisterl_amd import _lib
    env = D.start(_env("gw3_basic"), 3, 3, 1)
    arrs = D.mfma_case()[1]
    gp = _policy(arrs)
    r = tw.collector.solve(env, gp, det, 3, 0, C_UCB, 1, seed=D.SEED)
    assert _launch()[0] == _lib.TW_KERNEL_SOLVE_BIG, _launch()
    assert D.same(r, D.host_solve(env, gp, det, 3))
    assert D.same(r, D.oracle_solve(det_exp, env, oracle_policy(det_exp, arrs), det, 3))


# ---- 3. self-play and the MCTS-guided calls ---------------------------------------------------------------------------------------------------
#          id            module            obs  A  emb  H   twists
SEARCH = [("gw3_az",    "gw3_basic_az",    81,  4,  32,  32, 0),
          ("ring_az",   "ring_basic_az",   64,  3,  96, 256, 2),
          ("wide5_ws",  "wide5_basic_ws",  64,  5,  32,  64, 2)]


@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("row", SEARCH, ids=[r[0] for r in SEARCH])
def test_search_runs_in_the_search_kernel(tw, row, S):
    from twisterl_amd import _lib
    _, module, obs, A, emb, H, n_tw = row
    env = _env(module)
    assert env.search and env.obs_size == obs and env.num_actions() == A
    twists = _twists(obs, A, n_tw, 31) if n_tw else ((), ())
    gp = _policy(_arrs(obs, A, emb, H, 31 + S), twists)
    E, med, seed = 16 if S == 8 else 40, 1 if S == 4 else 2, 5
    g = tw.collector.AZCollector(E, S, C_UCB, med, 4).collect(env, gp, seed=seed)
    assert _launch() == (_lib.TW_KERNEL_MCTS_BIG, 1, 0, 0, (E + 15) // 16, 256), _launch()
    _same_bytes(g, host_az_collect(env, gp, E, S, C_UCB, med, seed))
    for det in (True, False):
        s = tw.collector.evaluate(env, gp, 16, det, 2, S, seed, C_UCB, med, 1)
        assert _launch() == (_lib.TW_KERNEL_MCTS_BIG, 1, 0, 0, 2, 256), _launch()
        assert s == host_evaluate(env, gp, 16, det, 2, S, seed, Cc=C_UCB, med=med)
    D.start(env, seed, 3, 1)
    r = tw.collector.solve(env, gp, False, 3, S, C_UCB, med, seed=seed)
    assert _launch() == (_lib.TW_KERNEL_MCTS_BIG, 1, 0, 0, 1, 256), _launch()
    assert D.same(r, D.host_solve(env, gp, False, 3, S=S, med=med, seed=seed))


# ---- 4. the block is packed from the LIVE arrays, in front of every launch ----------------------------------------------------------------------
def test_update_from_torch_is_seen_by_the_next_call(tw):
    import torch
    env = _env("gw3_basic")
    old, new = _arrs(81, 4, 96, 128, 41), _arrs(81, 4, 96, 128, 42)
    gp, fresh = _policy(old), _policy(new)
    E, seed = 40, 9
    before = _collect(tw, env, gp, E, seed)
    we, be, cs, as_, vs = new
    state = {"embeddings.weight": torch.tensor(we.T.copy()).cuda(), "embeddings.bias": torch.tensor(be).cuda()}
    for name, layers in (("common", cs), ("action", as_), ("value", vs)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = torch.tensor(np.asarray(wl).reshape(-1, len(bl)).T.copy()).cuda()
            state[f"{name}.{2 * i}.bias"] = torch.tensor(np.asarray(bl)).cuda()
    gp.update_from_torch(state)
    after = _collect(tw, env, gp, E, seed)
    _same_bytes(after, _host_collect(env, gp, E, seed))
    _same_bytes(after, _host_collect(env, fresh, E, seed))
    assert not np.array_equal(before.to_numpy()["logits"][:8], after.to_numpy()["logits"][:8])


# ---- 5. no result depends on what the workspace held ---------------------------------------------------------------------------------------------
def test_no_result_depends_on_what_the_workspace_held(tw):
    """As tests/test_gpu_device_env_fp16.py holds its image: the same bytes with every workspace and result word pre-set to 0xFFFFFFFF,
    1 and 0 (tw_debug_fill_memory), and -- hook off -- on the leftovers of the same call under a policy of other widths."""
    from twisterl_amd import _lib
    env = _env("gw3_basic")
    gp = _policy(_arrs(81, 4, 96, 256, 51), _twists(81, 4, 2, 51))
    other = _policy(_arrs(81, 4, 32, 64, 52))
    E, seed = 40, 3
    start = env.state_bytes()

    def run():
        env.set_state_bytes(start)
        g = _collect(tw, env, gp, E, seed)
        D.start(env, seed, 3, 1)
        r = tw.collector.solve(env, gp, False, 17, 0, C_UCB, 1, seed=seed)
        assert _launch()[0] == _lib.TW_KERNEL_SOLVE_BIG, _launch()
        return g, r

    want_g, want_r = run()
    _same_bytes(want_g, _host_collect(env, gp, E, seed))
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            g, r = run()
            _same_bytes(want_g, g)
            assert D.same(want_r, r)
    env.set_state_bytes(start)
    _collect(tw, env, other, E, seed)
    tw.collector.solve(env, other, False, 17, 0, C_UCB, 1, seed=seed)
    g, r = run()
    _same_bytes(want_g, g)
    assert D.same(want_r, r)


# ---- 6. what stays as it was ---------------------------------------------------------------------------------------------------------------------
def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def test_refusals_kept(tw):
    from twisterl_amd import _lib
    env = _env("gw3_basic")
    gp = _policy(_arrs(81, 4, 64, 64, 61))
    ppo = lambda e, prec: tw.collector.PPOCollector(16, GAMMA, LAM, 4, precision=prec).collect(e, gp, seed=1)
    for prec in ("fp16", "fp16x2"):                                           # the MFMA shape in another precision: the host path's answer
        assert _message(lambda: ppo(env, prec)) == (RuntimeError, "tw_ppo_collect_env: f32 only")
        assert _launch()[0] == _lib.TW_KERNEL_NONE
        msg = _message(lambda: tw.collector.evaluate(env, gp, 4, True, 1, 0, 1, C_UCB, 1, 1, precision=prec))
        assert msg[0] is RuntimeError and "f32 only" in msg[1], msg
        assert _launch()[0] == _lib.TW_KERNEL_NONE
    # a module built without the define: host-stepped as ever, the same bytes
    plain = gridworld(3, max_steps=12, difficulty=4, max_records=13)
    assert plain.basic is False
    h = ppo(plain, "fp32")
    assert _launch()[0] == _lib.TW_KERNEL_NONE, _launch()
    g = ppo(env, "fp32")
    assert _launch()[0] == _lib.TW_KERNEL_ROLLOUT_BIG, _launch()
    _same_bytes(g, h)
    tw.collector.evaluate(plain, gp, 4, True, 1, 0, 1, C_UCB, 1, 1)
    assert _launch()[0] == _lib.TW_KERNEL_NONE, _launch()
    # a search module without the define: self-play of the MFMA shape stays host-stepped
    from tests.device_env_search_util import ring_az
    az_plain = ring_az(n=32, max_steps=12, difficulty=4, noise=0.1, max_records=13)
    rp = _policy(_arrs(64, 3, 32, 32, 62))
    tw.collector.AZCollector(4, 4, C_UCB, 1, 4).collect(az_plain, rp, seed=1)
    assert _launch()[0] == _lib.TW_KERNEL_NONE, _launch()
