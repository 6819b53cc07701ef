"""GPU: solve() of a device environment in ONE kernel launch (tw_solve_device_env: solve_env_kernel / mcts_env_kernel started from the
prototype as it is, with the played actions kept).  Every case (tests/device_env_solve.py; tests/test_device_env_solve_build.py holds
them to the oracle on the CPU) makes three comparisons: the device result against the host-stepped path (tw_solve_env32 over the
module's own vtable: success equal, reward equal in f32 bits, action list equal), against oracle.solve_env over the struct's host code,
and tw_debug_last_launch against the kernel that had to run -- the family of the big-board kernels, nt = 1, solve = 1, the grid --
which is what fails while solve steps the struct on the host (TW_KERNEL_NONE).  The returned actions are replayed on a host clone,
and the caller's environment keeps its bytes.  EVERYTHING IS BITWISE."""
import signal

import pytest

from tests import device_env_solve as D
from tests.device_env_matrix import engine_nc
from tests.device_env_search_util import host_evaluate
from tests.util import f32_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A per-test time limit (SIGALRM) for tests that run long in Python code; a hang inside a HIP call is bounded by the `timeout`
    around the pytest run."""
    def boom(*_):
        raise TimeoutError("device-environment solve test exceeded its time limit")
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


def _launch():
    from twisterl_amd import _lib
    i = _lib.debug_last_launch()
    return i["family"], i["nt"], i["nc"], i["persist"], i["solve"], i["blocks"], i["threads"]


def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def _solve(tw, env, gp, det, N, S=0, med=1, seed=D.SEED):
    """collector.solve on the caller's env (whose bytes stay) -> (result, what was launched, the attempts)."""
    from twisterl_amd import _lib
    before = env.state_bytes()
    res = tw.collector.solve(env, gp, det, N, S, D.C_UCB, med, seed=seed)
    launch, att = _launch(), _lib.debug_last_attempts()
    assert env.state_bytes() == before
    assert isinstance(res, tuple) and isinstance(res[0], tuple) and isinstance(res[1], list)
    return res, launch, att


def _replays(env, res):
    exact, success, total = D.replay(env, res[1])
    assert exact and float(success) == res[0][0] and f32_bits(total) == f32_bits(res[0][1]), (res, exact, success, total)


def _first_strictly_best(att):
    best, bk = -1, (0.0, float("-inf"))
    for i, k in enumerate(zip(att[0].tolist(), att[1].tolist())):
        if k[0] > bk[0] or (k[0] == bk[0] and k[1] > bk[1]):
            best, bk = i, k
    return best


def _check(tw, O, case, gp, det, N, S=0, med=1, seed=D.SEED, persist=0, blocks=None):
    """The three comparisons of one solve on the device; returns the result and the attempts."""
    from twisterl_amd import _lib
    env, op = case[0], D.oracle_policy(case)
    res, launch, att = _solve(tw, env, gp, det, N, S, med, seed)
    family = _lib.TW_KERNEL_MCTS_BIG if S else _lib.TW_KERNEL_SOLVE_BIG
    assert launch == (family, 1, engine_nc(int(env._desc.n_obs)), persist, 1, blocks if blocks is not None else (N + 15) // 16, 256), launch
    host = D.host_solve(env, gp, det, N, S, med, seed)
    assert D.same(res, host), (res, host)
    orc = D.oracle_solve(O, env, op, det, N, S, med, seed)
    assert D.same(res, orc), (res, orc)
    _replays(env, res)
    # best of N: the first attempt that is strictly better, and its moves
    assert len(att[0]) == N
    best = _first_strictly_best(att)
    assert best >= 0 and (float(att[0][best]), f32_bits(att[1][best])) == (res[0][0], f32_bits(res[0][1])) and len(res[1]) == int(att[2][best])
    return res, att


# ---- 1. GridWorld 5 x 5 from a state no reset gives; 16 | 17 attempts: the edge of one workgroup's columns ----------------------------------------
@pytest.mark.parametrize("steps", [0, 2])
@pytest.mark.parametrize("det", [True, False])
def test_gridworld(tw, det_exp, steps, det):
    case = D.gridworld_case(steps)
    gp = D.lib_policy(case)
    for N in D.GRID_N:
        with _plain():
            _check(tw, det_exp, case, gp, det, N)


# ---- 2. the persistent form: a column that takes the next attempt from the queue writes that attempt's row --------------------------------------
@pytest.mark.parametrize("N", [40, 100])
def test_persistent_grid(tw, det_exp, N):
    case = D.gridworld_case(2)
    gp = D.lib_policy(case)
    with _hook(1):
        g, ga = _check(tw, det_exp, case, gp, False, N, persist=1, blocks=1)
    with _plain():
        p, pa = _check(tw, det_exp, case, gp, False, N)
    assert D.same(g, p) and all(x.tobytes() == y.tobytes() for x, y in zip(ga, pa))


# ---- 3. best of N: attempts that differ, the best not the first ----------------------------------------------------------------------------------
def test_best_of_n_is_the_first_strictly_best_attempt(tw, det_exp):
    case = D.gridworld_case(2)
    gp = D.lib_policy(case)
    res, att = _check(tw, det_exp, case, gp, False, D.BEST_OF_N["N"], seed=D.BEST_OF_N["seed"])
    best = _first_strictly_best(att)
    assert best > 0 and len(set(zip(att[0].tolist(), att[1].tolist()))) > 2, att
    orc = D.oracle_attempts(det_exp, case[0], D.oracle_policy(case), False, **D.BEST_OF_N)
    assert [(a[0][0], f32_bits(a[0][1]), len(a[1])) for a in orc] == [(float(s), f32_bits(t), int(n)) for s, t, n in zip(*att)]


# ---- 4. a start state that is already final: nothing to play --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 17])
def test_a_final_start_state_returns_no_action(tw, det_exp, N):
    case = D.final_case()
    env = case[0]
    assert env.is_final()
    res, _ = _check(tw, det_exp, case, D.lib_policy(case), False, N)
    assert res[1] == [] and res[0][0] == float(env.success()) and f32_bits(res[0][1]) == f32_bits(env.reward())


# ---- 5. the struct contract's corners: observe_n, a struct in scratch memory, n_obs() below N_OBS, a step() that draws -----------------------------
@pytest.mark.parametrize("which", ["lamps", "probe1k", "big_puzzle3x3", "ring"])
def test_struct_corners(tw, det_exp, which):
    case = {"lamps": D.lamps_case, "probe1k": lambda: D.probe_case("probe_o64a4s"), "big_puzzle3x3": D.big_puzzle_case, "ring": D.ring_case}[which]()
    gp = D.lib_policy(case)
    for det, N in ((True, 1), (False, 17)):
        _check(tw, det_exp, case, gp, det, N)


# ---- 6. 5 .. 31 actions: the list holds actions the four-action kernels cannot name ---------------------------------------------------------------
@pytest.mark.parametrize("module", sorted(D.WIDE_SEEDS))
def test_wide(tw, det_exp, module):
    case = D.wide_case(module)
    gp = D.lib_policy(case)
    res, _ = _check(tw, det_exp, case, gp, False, D.WIDE_N, seed=D.WIDE_SEEDS[module][1])
    assert max(res[1]) >= 4 and (module != "wideo64a31" or 30 in res[1]), res
    _check(tw, det_exp, case, gp, True, 1)


# ---- 7. MCTS-guided: the search kernel in solve mode, one column per attempt ---------------------------------------------------------------------
def _mcts_cases():
    from tests.device_env_wide_search import IDS
    return ["gridworld", "ring"] + list(IDS)


@pytest.mark.parametrize("which", _mcts_cases())
def test_mcts(tw, det_exp, which):
    case = D.gridworld_case(2, search=True) if which == "gridworld" else D.ring_case(search=True) if which == "ring" else D.wide_search_case(which)
    gp = D.lib_policy(case)
    assert case[0].search
    for med in (1, 2):
        for N in D.MCTS_N:
            _check(tw, det_exp, case, gp, N == 1, N, D.MCTS_S, med)


def test_mcts_without_a_search_kernel_runs_host_stepped(tw, det_exp):
    """The struct of the first wide row in its module built with wide=True alone: no search launcher, TW_KERNEL_NONE, the same result."""
    from twisterl_amd import _lib
    case = D.wide_case("wideo2a5")
    env, gp = case[0], D.lib_policy(case)
    assert env.search is False
    res, launch, _ = _solve(tw, env, gp, False, 3, D.MCTS_S, 2)
    assert launch[0] == _lib.TW_KERNEL_NONE, launch
    assert D.same(res, D.host_solve(env, gp, False, 3, D.MCTS_S, 2)) and D.same(res, D.oracle_solve(det_exp, env, D.oracle_policy(case), False, 3, D.MCTS_S, 2))
    _replays(env, res)


# ---- 8. errors: the host path's exception and text ------------------------------------------------------------------------------------------------
def _errors_alike(tw, case, det, N, S=0, contains=""):
    from twisterl_amd import _lib
    env, gp = case[0], D.lib_policy(case)
    dev = _message(lambda: tw.collector.solve(env, gp, det, N, S, D.C_UCB, 1, seed=D.SEED))
    assert _launch()[0] == (_lib.TW_KERNEL_MCTS_BIG if S else _lib.TW_KERNEL_SOLVE_BIG) and _launch()[4] == 1, _launch()
    host = _message(lambda: D.host_solve(env, gp, det, N, S, 1))
    assert dev == host and dev[0] is ValueError and contains in dev[1], (dev, host)


@pytest.mark.parametrize("S", [0, D.MCTS_S])
def test_a_bad_id_fails_alike(tw, S):
    _errors_alike(tw, D.ring_case(search=S > 0, bad_at=3, steps=1), False, 17, S, "index out of bounds: obs id ")


def test_a_bad_observe_n_count_fails_alike(tw):
    _errors_alike(tw, D.lamps_case(bad_at=2, bad_kind=2), False, 17, 0, "observation of 13 ids, at most 12")


def test_an_attempt_longer_than_max_records_fails_alike(tw, det_exp):
    case = D.gridworld_case(2, max_records=D.TOO_SHORT_STEPS - 1)
    _errors_alike(tw, case, True, 1, 0, f"solve: an attempt did not end within {D.TOO_SHORT_STEPS - 1} steps")
    ok = D.gridworld_case(2, max_records=D.TOO_SHORT_STEPS)              # the same handles work afterwards, and one step more is enough
    res, _ = _check(tw, det_exp, ok, D.lib_policy(ok), True, 1)
    assert len(res[1]) == D.TOO_SHORT_STEPS


# ---- 9. the hand-off, and evaluate over the shared body -------------------------------------------------------------------------------------------
def test_a_policy_of_the_mfma_shape_runs_host_stepped(tw, det_exp):
    from twisterl_amd import _lib
    case = D.mfma_case()
    env, gp = case[0], D.lib_policy(case)
    res, launch, _ = _solve(tw, env, gp, False, 3)
    assert launch[0] == _lib.TW_KERNEL_NONE, launch
    assert D.same(res, D.host_solve(env, gp, False, 3)) and D.same(res, D.oracle_solve(det_exp, env, D.oracle_policy(case), False, 3))


@pytest.mark.parametrize("S", [0, D.MCTS_S])
def test_evaluate_still_equals_the_host_path(tw, S):
    """The body evaluate shares with solve: reset per episode, no action rows, solve = 0 for the plain launch as before."""
    from twisterl_amd import _lib
    case = D.gridworld_case(0, search=S > 0)
    env, gp = case[0], D.lib_policy(case)
    with _plain():
        ge = tw.collector.evaluate(env, gp, 20, False, 2, S, 5, D.C_UCB, 1, 4)
        assert _launch() == (_lib.TW_KERNEL_MCTS_BIG if S else _lib.TW_KERNEL_SOLVE_BIG, 1, 25, 0, 1 if S else 0, 3, 256), _launch()
    he = host_evaluate(env, gp, 20, False, 2, S, 5)
    assert f32_bits(ge[0]) == f32_bits(he[0]) and f32_bits(ge[1]) == f32_bits(he[1]), (ge, he)
