"""GPU: AlphaZero self-play and MCTS-guided evaluate of device environments with 5 .. 31 actions ON THE DEVICE (mcts_env_kernel of a
module built with wide_search=True; the rows of tests/device_env_wide_search.py) are byte-equal to the host-stepped path over the
module's own vtable (tw_az_collect_env / tw_evaluate_env) and bit-equal to the oracle running the same struct's host code; errors are
the host path's; the trainer hand-off is the host collect's; what the kernel does not take runs host-stepped.  Every device case first
asserts the launch the library reports (TW_KERNEL_MCTS_BIG with nt 1, the module's EngineV width, one workgroup per 16 columns), then
compares.  No tolerance anywhere: every comparison is bytes or bits.

Deliberate breaks and what failed then (each tried on the GPU, each reversed): the action read back as `& 3` -- self-play and evaluate
of every row above four actions, the hand-off and the fall-back test; the twist unit with stride 4 -- self-play and evaluate of the three
twist rows above four actions; the average divided after the sum -- test_near_tied_priors_hold_the_twist_average_to_its_order alone
(visit counts are deaf to the last bit of a prior everywhere else); the child loop stopping at 4 -- self-play of six rows, evaluate of
five; the 1/A fallback with A = 4 -- test_a_root_without_children_gives_the_uniform_fallback; A instead of 2A units to the compaction
(the library) -- every self-play test above four actions."""
import signal

import numpy as np
import pytest

from tests.device_env_search_util import host_az_collect, host_evaluate
from tests.device_env_wide_search import (BY_MODULE, C_UCB, E, ERROR_ROW, EVAL_EPISODES, EVAL_S, EVAL_SEED_OFFSET, FALLBACK_ROW, HANDOFF_ROW, IDS, SHUT, TIE,
                                          host_env, make_env, policies, shared_self_play)
from tests.util import f32_bits

pytestmark = pytest.mark.gpu
AZ_FIELDS = ("obs", "logits", "perms", "remaining_values", "ep_len", "ep_start")


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code.  A signal handler runs only when control returns to
    the interpreter, so a hang inside a HIP call is bounded by the `timeout` around the pytest run, not by this."""
    def boom(*_):
        raise TimeoutError("wide device-environment search test exceeded its time limit")
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


def _assert_search_launch(env, columns):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["blocks"], info["threads"]) == \
        (_lib.TW_KERNEL_MCTS_BIG, 1, int(env._desc.engine_nc), (columns + 15) // 16, 256), info


def _assert_no_launch():
    from twisterl_amd import _lib
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE


def _same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y) == sorted(AZ_FIELDS), (sorted(x), sorted(y))
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (k, x[k].dtype, y[k].dtype, x[k].shape, y[k].shape)
        assert x[k].tobytes() == y[k].tobytes(), k
    assert a.ragged == b.ragged


def _setup(module, O):
    r = BY_MODULE[module]
    gp, op = policies(O, r)
    return r, make_env(r), gp, op


def _message(fn):
    """The exception a call raises: type and message."""
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


# ---- 1. self-play: the host-stepped path's bytes, the oracle's fields ------------------------------------------------------------------------------
@pytest.mark.parametrize("module", IDS)
def test_self_play_equals_host_path_and_oracle(tw, det_exp, module):
    check_self_play(tw, det_exp, module)


def check_self_play(tw, det_exp, module):
    """-> the device self-play that was checked"""
    r, env, gp, _ = _setup(module, det_exp)
    assert env.search is True
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, r.S, C_UCB, r.med, r.seed))
    a = g.to_numpy()
    assert a["logits"].shape == (len(a["perms"]), r.A) and a["obs"].shape[1] == r.n_obs and g.stats["rollout_blocks"] == (E + 15) // 16
    o = shared_self_play(module)
    assert (r.o_E, r.o_S) == (E, r.S)                      # (every row's oracle run is the full size)
    assert np.array_equal(a["ep_len"], o.ep_len) and np.all(a["perms"] == -1)
    if r.var:
        assert g.ragged and np.array_equal(a["obs"], o.obs) and g.obs == o.obs_lists
    else:
        assert np.array_equal(a["obs"].astype(np.int64), o.obs.astype(np.int64))
    assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
    assert np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.remaining_values))
    n_tw = max(r.twists, 1)
    assert g.stats["forward_evals"] == o.evals * n_tw and g.stats["forward_evals"] % n_tw == 0      # full_predict averages ALL twists
    return g


# ---- 2. MCTS-guided evaluate: deterministic with 1 attempt, sampled with 2 -------------------------------------------------------------------------
@pytest.mark.parametrize("module", IDS)
def test_mcts_guided_evaluate_equals_host_path_and_oracle(tw, det_exp, module):
    r, env, gp, op = _setup(module, det_exp)
    seed = r.seed + EVAL_SEED_OFFSET
    for det, ns in ((True, 1), (False, 2)):
        ge = tw.collector.evaluate(env, gp, num_episodes=EVAL_EPISODES, deterministic=det, num_searches=ns, num_mcts_searches=EVAL_S, seed=seed,
                                   C=C_UCB, max_expand_depth=r.med, num_cores=4)
        _assert_search_launch(env, EVAL_EPISODES * ns)
        he = host_evaluate(env, gp, EVAL_EPISODES, det, ns, EVAL_S, seed, Cc=C_UCB, med=r.med)
        oe = det_exp.evaluate_env(host_env(env), op, EVAL_EPISODES, det, ns, EVAL_S, C_UCB, r.med, seed=seed, difficulty=r.diff)
        for other in (he, oe):
            assert f32_bits(ge[0]) == f32_bits(other[0]) and f32_bits(ge[1]) == f32_bits(other[1]), (module, det, ns, ge, he, oe)


# ---- 2b. a state without an allowed action: a root without children, the uniform fallback 1 / A ------------------------------------------------
def test_a_root_without_children_gives_the_uniform_fallback(tw, det_exp):
    """WideShutA7: one state in four allows no action.  Host-stepped path only (the oracle, like the reference, cannot run a leaf
    without children).  Some record's probabilities are all 1 / 7."""
    r, env, gp, _ = _setup(SHUT.module, det_exp)
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, r.S, C_UCB, r.med, r.seed))
    lg = g.to_numpy()["logits"]
    uniform = np.float32(1.0) / np.float32(r.A)
    assert lg.shape[1] == r.A == 7 and (f32_bits(lg) == f32_bits(np.full_like(lg, uniform))).all(axis=1).any(), "no record with the uniform fallback"
    assert g.stats["forward_evals"] % r.twists == 0
    for det, ns in ((True, 1), (False, 2)):
        ge = tw.collector.evaluate(env, gp, num_episodes=EVAL_EPISODES, deterministic=det, num_searches=ns, num_mcts_searches=EVAL_S, seed=r.seed,
                                   C=C_UCB, max_expand_depth=r.med, num_cores=4)
        _assert_search_launch(env, EVAL_EPISODES * ns)
        he = host_evaluate(env, gp, EVAL_EPISODES, det, ns, EVAL_S, r.seed, Cc=C_UCB, med=r.med)
        assert f32_bits(ge[0]) == f32_bits(he[0]) and f32_bits(ge[1]) == f32_bits(he[1]), (det, ns, ge, he)


# ---- 2c. near-tied priors: the order of the twist average decides which child a move's searches visit first -----------------------------------
def test_near_tied_priors_hold_the_twist_average_to_its_order(tw, det_exp):
    """WideTieA6 under twists that rotate the actions within (0 1 2) and (3 4 5) over an unchanged observation: the priors of a cycle's
    actions are the same three head outputs averaged in three orders.  Bytes of the host path, bits of the oracle -- which only an
    average that runs x / n pass by pass from 0.0f gives."""
    r, env, gp, _ = _setup(TIE.module, det_exp)
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, r.S, C_UCB, r.med, r.seed))
    a, o = g.to_numpy(), shared_self_play(TIE.module)
    assert np.array_equal(a["ep_len"], o.ep_len) and np.array_equal(a["obs"].astype(np.int64), o.obs.astype(np.int64))
    assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
    assert g.stats["forward_evals"] == 3 * o.evals


# ---- 3. errors are the host path's (31 actions, EngineV<64>) ---------------------------------------------------------------------------------------
def test_errors_are_the_host_path_s(tw, det_exp):
    """A bad id at step 0 (a root) and at step 2 (a leaf reaches it before the episode does) fails self-play and MCTS evaluate with the
    host path's exception and message; the kernel guards every load, nothing faults.  An episode longer than max_records fails like the
    host path's; the device is fine afterwards."""
    r, _, gp, _ = _setup(ERROR_ROW, det_exp)
    for bad_at in (0, 2):
        env = make_env(r, bad_at=bad_at)
        dev = _message(lambda: tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed))
        _assert_search_launch(env, E)
        host = _message(lambda: host_az_collect(env, gp, E, r.S, C_UCB, r.med, r.seed))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
        dev = _message(lambda: tw.collector.evaluate(env, gp, 16, False, 2, EVAL_S, r.seed, C_UCB, r.med, 1))
        _assert_search_launch(env, 32)
        host = _message(lambda: host_evaluate(env, gp, 16, False, 2, EVAL_S, r.seed, Cc=C_UCB, med=r.med))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
    short = make_env(r, max_records=2)
    with pytest.raises(ValueError, match="did not end within 2 records"):
        tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(short, gp, seed=r.seed)
    _assert_search_launch(short, E)
    assert _message(lambda: host_az_collect(short, gp, E, r.S, C_UCB, r.med, r.seed))[1].endswith("an episode did not end within 2 records")
    ok = make_env(r)
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(ok, gp, seed=r.seed)
    _assert_search_launch(ok, E)
    assert len(g) >= E


# ---- 4. the trainer hand-off ---------------------------------------------------------------------------------------------------------------------
def test_trainer_hand_off_equals_the_host_collect(tw, det_exp):
    import torch
    from twisterl_amd.trainer import az_data_to_torch
    r, env, gp, _ = _setup(HANDOFF_ROW, det_exp)
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed + 7)
    _assert_search_launch(env, E)
    h = host_az_collect(env, gp, E, r.S, C_UCB, r.med, r.seed + 7)
    tg, th = az_data_to_torch(g, r.obs_size), az_data_to_torch(h, r.obs_size)
    assert len(tg) == len(th) == 3 and tg[1].shape[1] == r.A
    for x, y in zip(tg, th):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


# ---- 5. what the kernel does not take runs host-stepped ---------------------------------------------------------------------------------------------
def test_what_the_kernel_does_not_take_runs_on_the_host_path(tw, det_exp):
    """The same struct in a module built with wide=True alone (no search kernel): TW_KERNEL_NONE, and the bytes of the wide-search
    module's device run.  A policy of the MFMA shape: host-stepped on the wide-search module too."""
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    from tests.util import amd_policy, make_policy_arrays
    r, env, gp, _ = _setup(FALLBACK_ROW, det_exp)
    plain = DeviceEnv(build_device_env(r.header, r.type, r.module + "_plain", wide=True), r.module + "_plain", list(r.params), max_records=r.max_records)
    assert plain.search is False and env.search is True
    p = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(plain, gp, seed=r.seed)
    _assert_no_launch()
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed)
    _assert_search_launch(env, E)
    _same_bytes(p, g)
    pe = tw.collector.evaluate(plain, gp, EVAL_EPISODES, False, 2, EVAL_S, r.seed, C_UCB, r.med, 1)
    _assert_no_launch()
    ge = tw.collector.evaluate(env, gp, EVAL_EPISODES, False, 2, EVAL_S, r.seed, C_UCB, r.med, 1)
    _assert_search_launch(env, 2 * EVAL_EPISODES)
    assert f32_bits(pe[0]) == f32_bits(ge[0]) and f32_bits(pe[1]) == f32_bits(ge[1])
    # ONE common layer of 64 over obs_size 64 and an embedding of 64: the MFMA shape
    mp = amd_policy(make_policy_arrays(8, seed=4, emb=64, hidden=64, n_actions=r.A))
    z = tw.collector.AZCollector(20, 8, C_UCB, 1, 4).collect(env, mp, seed=8)
    _assert_no_launch()
    _same_bytes(z, host_az_collect(env, mp, 20, 8, C_UCB, 1, 8))
    e = tw.collector.evaluate(env, mp, EVAL_EPISODES, False, 2, EVAL_S, 5, C_UCB, 1, 1)
    _assert_no_launch()
    assert e == host_evaluate(env, mp, EVAL_EPISODES, False, 2, EVAL_S, 5, Cc=C_UCB, med=1)


# ---- 6. a launcher that refuses the arguments: the library says what to do ------------------------------------------------------------------------
def test_a_launcher_that_refuses_the_arguments_says_rebuild_the_module(tw, det_exp):
    """A module compiled against an EnvMctsArgs of another size answers hipErrorInvalidValue from its launcher (struct_bytes).  Stood in
    for by a descriptor whose launcher is a callback that answers just that: the collect fails with "rebuild the module", no result."""
    import ctypes as C
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    r, env, gp, _ = _setup(FALLBACK_ROW, det_exp)
    refuse = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_size_t, C.c_void_p)(lambda *_: 1)      # hipErrorInvalidValue
    bad = DeviceEnvDesc.from_buffer_copy(env._desc)
    bad.launch_search = C.cast(refuse, C.c_void_p).value
    prm = _lib.AZParams(E, 0, r.S, C_UCB, r.med, r.seed, _lib.TW_PREC_F32_EXACT, 1, 0)
    out = C.c_void_p()
    rc = _lib.lib().tw_az_collect_device_env(C.addressof(bad), env._obj, env._desc.state_bytes, gp._handle(), C.byref(prm), env.max_records,
                                             C.byref(out))
    assert rc == _lib.TW_ERR_INVALID and "rebuild the module" in _lib.last_error() and not out.value, (rc, _lib.last_error())
    g = tw.collector.AZCollector(E, r.S, C_UCB, r.med, 4).collect(env, gp, seed=r.seed)              # the module itself is fine
    _assert_search_launch(env, E)
    assert len(g) >= E
