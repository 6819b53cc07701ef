"""GPU: AlphaZero self-play and MCTS-guided evaluate of user-written environments ON THE DEVICE (tw_az_collect_device_env, and
tw_evaluate_device_env with num_mcts_searches > 0: mcts_env_kernel of a module built with search=True) are bit-equal to the
host-stepped path over the module's own vtable (tw_az_collect_env / tw_evaluate_env) and to the oracle's restatement of az.rs /
search.rs / solve.rs running the same struct's host code; BigPuzzleEnv<25> gives the bytes of the library's own mcts_big_kernel;
errors are the host path's; what the kernel does not take runs on the host path.  Every device case first asserts the launch the
library reports (TW_KERNEL_MCTS_BIG with nt 1), then compares bytes.  All comparisons are bitwise."""
import signal

import numpy as np
import pytest

from tests.device_env_search_util import big_puzzle_az, gridworld_az, host_az_collect, host_evaluate, lamps_az, ring_az
from tests.device_env_util import HostEnv, gridworld
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays, make_policy_arrays, oracle_policy, puzzle_transpose_twist
from tests.var_obs_util import VarHostEnv, lamps_policy_arrays, lamps_twists, oracle_az_loop

pytestmark = pytest.mark.gpu
AZ_FIELDS = ("obs", "logits", "perms", "remaining_values", "ep_len", "ep_start")


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code.  A signal handler runs only when control returns to
    the interpreter, so a hang inside a HIP call is bounded by the `timeout` around the pytest run, not by this."""
    def boom(*_):
        raise TimeoutError("device-environment search test exceeded its time limit")
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
    """The oracle's soft-max with the deterministic exp, as the library's (where the existing search tests set it)."""
    oracle.set_det_exp(True)
    yield oracle
    oracle.set_det_exp(False)


def _assert_search_launch(env, columns):
    """The last call ran mcts_env_kernel of the module: family TW_KERNEL_MCTS_BIG with nt 1, the module's EngineV width, one
    workgroup of 256 per 16 columns."""
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


def _same_as_oracle(g, o, n_obs, A):
    a = g.to_numpy()
    assert a["obs"].shape[1] == n_obs and a["logits"].shape[1] == A
    assert np.array_equal(a["ep_len"], o.ep_len)
    assert np.array_equal(a["obs"].astype(np.int64), o.obs)
    assert np.all(a["perms"] == -1)
    assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
    assert np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.additional_data["remaining_values"]))


def _grid():
    env = gridworld_az(max_steps=12, difficulty=2, max_records=13)
    arrs = make_deep_policy_arrays(25, seed=3, emb=64, common=(32,), n_actions=4)          # 625 -> 64 -> 32 -> heads (obs_size > 256: EngineV)
    return env, arrs


def _ring_twists(n):
    mir = lambda p: (n - p) % n
    ident = list(range(2 * n))
    flip = [mir(i) if i < n else n + mir(i - n) for i in range(2 * n)]
    return [ident, flip], [[0, 1, 2], [2, 1, 0]]


def _ring(**kw):
    env = ring_az(n=32, max_steps=40, difficulty=3, noise=0.25, max_records=41, **kw)
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64, 32), n_actions=3)          # obs_size 64, two common layers: EngineV
    return env, arrs, _ring_twists(32)


@pytest.mark.parametrize("E,S,med,merge_order,offset", [(40, 6, 1, True, 0), (17, 16, 2, False, 1000)])
def test_gridworld_self_play_equals_host_path_and_oracle(tw, det_exp, E, S, med, merge_order, offset):
    """40 and 17 episodes: more than one workgroup, a partial last one; both merge orders; one run with an episode offset."""
    env, arrs = _grid()
    gp, op = amd_policy(arrs), oracle_policy(det_exp, arrs)
    g = tw.collector.AZCollector(E, S, 1.41, med, 4, merge_order=merge_order, episode_offset=offset).collect(env, gp, seed=123)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, S, 1.41, med, 123, offset=offset, merge_order=merge_order))
    o = det_exp.az_collect_env(HostEnv(env), op, E, S, 1.41, med, seed=123, episode_offset=offset, difficulty=2, merge_order=merge_order)
    _same_as_oracle(g, o, 25, 4)
    a = g.to_numpy()
    assert a["obs"].dtype == np.uint16 and 1 <= a["ep_len"].min() and a["ep_len"].max() <= 13 and len(set(a["ep_len"].tolist())) > 1
    assert g.stats["rollout_blocks"] == (E + 15) // 16 and g.stats["forward_evals"] > len(a["perms"])


def test_ring_three_actions_twists_and_a_step_that_draws(tw, det_exp):
    """A < 4 (the narrowing), full_predict averaged over two twists, and replay of the tree's actions through a step() that draws."""
    env, arrs, twists = _ring()
    gp, op = amd_policy(arrs, *twists), oracle_policy(det_exp, arrs, *twists)
    E, S, med = 33, 8, 2
    g = tw.collector.AZCollector(E, S, 1.41, med, 4).collect(env, gp, seed=41)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, S, 1.41, med, 41))
    o = det_exp.az_collect_env(HostEnv(env), op, E, S, 1.41, med, seed=41, difficulty=3)
    _same_as_oracle(g, o, 2, 3)
    a = g.to_numpy()
    assert a["obs"].dtype == np.uint8 and a["logits"].shape[1] == 3
    assert g.stats["forward_evals"] % 2 == 0                                # evaluations x twists


def test_lamps_variable_length_observations(tw, det_exp):
    """observe_n: records of 0 .. 12 ids; the result is ragged, 0xFFFF in the free slots."""
    env = lamps_az()
    arrs, twists = lamps_policy_arrays(12), lamps_twists(12)
    gp, op = amd_policy(arrs, *twists), oracle_policy(det_exp, arrs, *twists)
    E, S = 20, 6
    g = tw.collector.AZCollector(E, S, 1.41, 1, 4).collect(env, gp, seed=11)
    _assert_search_launch(env, E)
    _same_bytes(g, host_az_collect(env, gp, E, S, 1.41, 1, 11))
    o = oracle_az_loop(det_exp, VarHostEnv(env), op, E, S, 1.41, 1, 11, 12, difficulty=3)
    a = g.to_numpy()
    assert g.ragged and a["obs"].dtype == np.uint16 and np.array_equal(a["obs"], o.obs) and g.obs == o.obs_lists
    assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits)) and np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.remaining_values))
    assert np.array_equal(a["ep_len"], o.ep_len) and set(a["perms"].tolist()) == {-1}
    assert int(o.counts.min()) == 0 and (a["obs"] == 0xFFFF).any()         # states without an id occur (the final, all-off one)


def test_big_puzzle_module_gives_the_bytes_of_the_library_search_kernel(tw):
    """One Puzzle, two search kernels: tw.env.Puzzle of a 5 x 5 board runs in the library's mcts_big_kernel, the struct
    BigPuzzleEnv<25> over the same step / masks / reward / is_final, built with search=True, in mcts_env_kernel."""
    from twisterl_amd import _lib
    D = 5
    gp = amd_policy(make_deep_policy_arrays(25, seed=7, emb=64, common=(64, 32), scale=2.0), *puzzle_transpose_twist(5))
    lib_env, mod_env = tw.env.Puzzle(5, 5, D, 2, 256), big_puzzle_az(5, 5, D, 2, 256, max_records=2 * D + 1)
    b = tw.collector.AZCollector(40, 8, 1.41, 1, 4).collect(mod_env, gp, seed=23)
    _assert_search_launch(mod_env, 40)
    a = tw.collector.AZCollector(40, 8, 1.41, 1, 4).collect(lib_env, gp, seed=23)
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["blocks"]) == (_lib.TW_KERNEL_MCTS_BIG, 0, 25, 3), info
    _same_bytes(a, b)
    x = a.to_numpy()
    assert x["obs"].dtype == np.uint16 and x["obs"].shape[1] == 25 and len(x["perms"]) > 40
    for det, ns in ((True, 1), (False, 2)):
        eb = tw.collector.evaluate(mod_env, gp, num_episodes=24, deterministic=det, num_searches=ns, num_mcts_searches=6, seed=5, C=1.41,
                                   max_expand_depth=1, num_cores=4)
        _assert_search_launch(mod_env, 24 * ns)
        ea = tw.collector.evaluate(lib_env, gp, num_episodes=24, deterministic=det, num_searches=ns, num_mcts_searches=6, seed=5, C=1.41,
                                   max_expand_depth=1, num_cores=4)
        assert f32_bits(ea[0]) == f32_bits(eb[0]) and f32_bits(ea[1]) == f32_bits(eb[1]), (det, ns, ea, eb)


def test_mcts_guided_evaluate_equals_host_path_and_oracle(tw, det_exp):
    genv, garrs = _grid()
    renv, rarrs, twists = _ring()
    cases = ((genv, amd_policy(garrs), oracle_policy(det_exp, garrs), 2), (renv, amd_policy(rarrs, *twists), oracle_policy(det_exp, rarrs, *twists), 3))
    for env, gp, op, diff in cases:
        for det, ns in ((True, 1), (False, 2)):
            ge = tw.collector.evaluate(env, gp, num_episodes=12, deterministic=det, num_searches=ns, num_mcts_searches=6, seed=5, C=1.41,
                                       max_expand_depth=1, num_cores=4)
            _assert_search_launch(env, 12 * ns)
            he = host_evaluate(env, gp, 12, det, ns, 6, 5)
            oe = det_exp.evaluate_env(HostEnv(env), op, 12, det, ns, 6, 1.41, 1, seed=5, difficulty=diff)
            assert f32_bits(ge[0]) == f32_bits(he[0]) and f32_bits(ge[1]) == f32_bits(he[1]), (env.name, det, ns, ge, he)
            assert f32_bits(ge[0]) == f32_bits(oe[0]) and f32_bits(ge[1]) == f32_bits(oe[1]), (env.name, det, ns, ge, oe)


def _message(fn):
    """The exception a call raises: type and message."""
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def test_errors_are_the_host_path_s(tw):
    """Bad ids at an evaluated state -- a root or a leaf of the search: a leaf reaches step bad_at before the episode does -- fail
    self-play and MCTS evaluate with the host path's exception and message, naming the same (first) id; the kernel guards every
    load, nothing faults.  An episode longer than max_records fails like the host path's; the device is fine afterwards."""
    arrs = make_deep_policy_arrays(8, seed=9, emb=64, common=(64,), policy_layers=(32,), n_actions=3)
    gp = amd_policy(arrs)
    for bad_at in (0, 2):
        env = ring_az(n=32, max_steps=40, difficulty=8, noise=0.0, bad_at=bad_at, max_records=41)
        dev = _message(lambda: tw.collector.AZCollector(40, 6, 1.41, 2, 4).collect(env, gp, seed=1))
        _assert_search_launch(env, 40)
        host = _message(lambda: host_az_collect(env, gp, 40, 6, 1.41, 2, 1))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
        dev = _message(lambda: tw.collector.evaluate(env, gp, 16, False, 2, 6, 1, 1.41, 1, 1))
        _assert_search_launch(env, 32)
        host = _message(lambda: host_evaluate(env, gp, 16, False, 2, 6, 1))
        assert dev == host and dev[0] is ValueError and "index out of bounds: obs id " in dev[1], (bad_at, dev, host)
    short = ring_az(n=32, max_steps=40, difficulty=8, noise=0.0, max_records=2)
    with pytest.raises(ValueError, match="did not end within 2 records"):
        tw.collector.AZCollector(40, 6, 1.41, 1, 4).collect(short, gp, seed=1)
    _assert_search_launch(short, 40)
    assert _message(lambda: host_az_collect(short, gp, 40, 6, 1.41, 1, 1))[1].endswith("an episode did not end within 2 records")
    ok = ring_az(n=32, max_steps=40, difficulty=3, noise=0.0, max_records=41)
    g = tw.collector.AZCollector(40, 6, 1.41, 1, 4).collect(ok, gp, seed=1)
    _assert_search_launch(ok, 40)
    assert len(g) >= 40


def test_what_the_kernel_does_not_take_runs_on_the_host_path(tw):
    """A module built without search, and a policy of the MFMA shape: the host path's bytes, and no kernel of the launch hook's."""
    plain = gridworld(max_steps=12, difficulty=2, max_records=13)
    assert not plain.search
    gp = amd_policy(_grid()[1])
    g = tw.collector.AZCollector(20, 6, 1.41, 1, 4).collect(plain, gp, seed=8)
    _assert_no_launch()
    _same_bytes(g, host_az_collect(plain, gp, 20, 6, 1.41, 1, 8))
    e = tw.collector.evaluate(plain, gp, 12, True, 1, 6, 5, 1.41, 1, 1)
    _assert_no_launch()
    assert e == host_evaluate(plain, gp, 12, True, 1, 6, 5)
    # the same bytes as the search module's device run: one struct, two modules
    _same_bytes(g, tw.collector.AZCollector(20, 6, 1.41, 1, 4).collect(gridworld_az(max_steps=12, difficulty=2, max_records=13), gp, seed=8))
    # ring with ONE common layer of 64 over obs_size 64: the MFMA shape
    env = ring_az(n=32, max_steps=40, difficulty=3, noise=0.25, max_records=41)
    mp = amd_policy(make_policy_arrays(8, seed=4, emb=64, hidden=64, n_actions=3))
    z = tw.collector.AZCollector(20, 6, 1.41, 1, 4).collect(env, mp, seed=8)
    _assert_no_launch()
    _same_bytes(z, host_az_collect(env, mp, 20, 6, 1.41, 1, 8))
    e = tw.collector.evaluate(env, mp, 12, False, 2, 6, 5, 1.41, 1, 1)
    _assert_no_launch()
    assert e == host_evaluate(env, mp, 12, False, 2, 6, 5)


def test_trainer_hand_off_equals_the_host_collect(tw):
    import torch
    from twisterl_amd.trainer import az_data_to_torch
    env, arrs, twists = _ring()
    gp = amd_policy(arrs, *twists)
    g = tw.collector.AZCollector(33, 8, 1.41, 1, 4).collect(env, gp, seed=19)
    _assert_search_launch(env, 33)
    h = host_az_collect(env, gp, 33, 8, 1.41, 1, 19)
    tg, th = az_data_to_torch(g, 64), az_data_to_torch(h, 64)
    assert len(tg) == len(th) == 3
    for x, y in zip(tg, th):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())
