"""solve() of a device environment ON THE DEVICE (tw_solve_device_env): the cases tests/test_device_env_solve_build.py (no GPU: every
case ends within max_records under the oracle and contains what it is about) and tests/test_gpu_device_env_solve.py (the device
against the host-stepped path and the oracle) share, and their helpers.  A case = (environment in a start state that is NO reset
state, the policy's weights, its twists) -- lib_policy() / oracle_policy() make the two policies of it (the library's needs a device);
the oracle runs the struct's own host code (tests/device_env_util.HostEnv)."""
import ctypes as C
import functools

import numpy as np

from tests.device_env_matrix import host_env

C_UCB = 1.41
SEED = 7                              # the seed of the solves, unless a case says otherwise
GRID_N = (1, 3, 16, 17, 40)          # 16 | 17: the edge of one workgroup's columns
MCTS_N = (1, 3, 17)
MCTS_S = 8                            # searches per move; expansion depth 1 and 2
# found with the oracle (tests/test_device_env_solve_build.py holds them to it): sampled GridWorld attempts from the 2-step start that
# differ in (success, total), the best of them not attempt 0
BEST_OF_N = dict(seed=2, N=17)
# wide rows: (episode of the start state's reset, seed of the solve) whose sampled best of 3 holds an action >= 4 (31 actions: action 30)
WIDE_SEEDS = {"wideo2a5": (0, 1), "wideo17a17": (0, 1), "wideo64a31": (0, 4), "perm8": (0, 1)}
WIDE_N = 3
# the moves of the deterministic single attempt from GridWorld's 2-step start: max_records one below it fails the solve
TOO_SHORT_STEPS = 10
# wide-search rows: an episode whose reset state is not final after one step
WS_EPISODE = {"wideo2a5_ws": 0, "wideo5a8v_ws": 0, "wideo16a16_ws": 2, "wideo17a17_ws": 0, "wideo64a31_ws": 0, "perm8_ws": 0, "wideo4a3_ws": 0,
              "wideopena31_ws": 0}


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


def start(env, seed, episode, steps):
    """reset(seed, episode), then `steps` times the first allowed action: a state no reset gives."""
    env.reset(seed=seed, episode=episode)
    for _ in range(steps):
        assert not env.is_final()
        env.step(next(i for i, m in enumerate(env.masks()) if m))
    return env


def run_out(env, seed, episode):
    """reset, then the first allowed action until the state is final."""
    env.reset(seed=seed, episode=episode)
    while not env.is_final():
        env.step(next(i for i, m in enumerate(env.masks()) if m))
    return env


def host_solve(env, policy, det, N, S=0, med=1, seed=SEED, max_steps=None):
    """tw_solve_env32 over the module's host vtable, called directly: the host-stepped path -> ((success, reward), actions)."""
    from twisterl_amd import _lib
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    prm = _lib.SolveParams(int(det), N, S, C_UCB, med, seed, _lib.TW_PREC_F32_EXACT)
    ms = env.max_records if max_steps is None else max_steps
    acts = (C.c_uint32 * (ms + 1))()
    s, r, n = C.c_float(), C.c_float(), C.c_uint32()
    _lib.check(_lib.lib().tw_solve_env32(C.byref(vt), policy._handle(), C.byref(prm), ms, C.byref(s), C.byref(r), acts, ms + 1, C.byref(n)))
    return (float(s.value), float(r.value)), [int(acts[i]) for i in range(n.value)]


def oracle_solve(O, env, op, det, N, S=0, med=1, seed=SEED):
    """oracle.solve_env from the environment's current state (caller: set_det_exp(True)) -> ((success, reward), actions)."""
    (s, r), acts = O.solve_env(host_env(env), op, det, N, S, C_UCB, med, seed=seed)
    return (float(s), float(r)), [int(a) for a in acts]


def oracle_attempts(O, env, op, det, N, S=0, med=1, seed=SEED):
    """Every attempt on its own: attempt k of N is the one attempt of solve_env keyed `episode * 1 + 0 = k`."""
    return [O.solve_env(host_env(env), op, det, 1, S, C_UCB, med, seed=seed, episode=k) for k in range(N)]


def replay(env, actions):
    """A host clone of `env` stepped through `actions` -> (final exactly after the last one, success(), the rewards summed in f32 in
    solve.rs's order: before every step and once at the end)."""
    h = host_env(env).copy()
    total = np.float32(0)
    exact = True
    for a in actions:
        if h.is_final():
            exact = False
        total = np.float32(total + np.float32(h.value()))
        h.next(a)
    total = np.float32(total + np.float32(h.value()))
    return exact and h.is_final(), h.success(), float(total)


def same(a, b):
    """success equal, reward equal in f32 bits, action list equal"""
    bits = lambda x: np.float32(x).view(np.uint32)
    return a[0][0] == b[0][0] and bits(a[0][1]) == bits(b[0][1]) and list(a[1]) == list(b[1])


# ---- the cases: (env, policy arrays, twists) ---------------------------------------------------------------------------------------------------
def lib_policy(case):
    from tests.util import amd_policy
    return amd_policy(case[1], *case[2])


def oracle_policy(case):
    from tests import util
    return util.oracle_policy(_oracle(), case[1], *case[2])


def _ring_twists(n):
    mir = lambda p: (n - p) % n
    ident = list(range(2 * n))
    flip = [mir(i) if i < n else n + mir(i - n) for i in range(2 * n)]
    return [ident, flip], [[0, 1, 2], [2, 1, 0]]


@functools.lru_cache(maxsize=None)
def grid_policies():
    from tests.util import make_deep_policy_arrays
    return make_deep_policy_arrays(25, seed=11, emb=64, common=(64, 32), n_actions=4, scale=2.0), ((), ())


@functools.lru_cache(maxsize=None)
def ring_policies():
    from tests.util import make_deep_policy_arrays
    return make_deep_policy_arrays(8, seed=2, emb=64, common=(64, 32), n_actions=3), _ring_twists(32)


def gridworld_case(steps, search=False, max_steps=12, max_records=None):
    """GridWorld 5 x 5 after reset(seed=3, episode=5) and `steps` allowed steps."""
    from tests.device_env_search_util import gridworld_az
    from tests.device_env_util import gridworld
    make = gridworld_az if search else (lambda **kw: gridworld(size=5, **kw))
    env = make(max_steps=max_steps, difficulty=6, max_records=max_records or max_steps + 1)
    return (start(env, 3, 5, steps),) + grid_policies()


def mfma_case():
    """GridWorld 3 x 3 (obs_size 81) under a policy of ONE common layer of 64 units: the MFMA shape, which the environment kernels do
    not take (tests/test_gpu_device_env.py's hand-off case)."""
    from tests.device_env_util import gridworld
    from tests.util import make_policy_arrays
    env = gridworld(size=3, max_steps=12, difficulty=4, max_records=13)
    return start(env, 3, 3, 1), make_policy_arrays(9, seed=4, emb=64, hidden=64), ((), ())


def final_case():
    """GridWorld 5 x 5 run until it is final: solve has nothing to play."""
    from tests.device_env_util import gridworld
    return (run_out(gridworld(size=5, max_steps=6, difficulty=6, max_records=7), 3, 5),) + grid_policies()


def ring_case(search=False, bad_at=-1, steps=1):
    from tests.device_env_search_util import ring_az
    from tests.device_env_util import ring
    env = (ring_az if search else ring)(n=32, max_steps=12, difficulty=4, noise=0.1, bad_at=bad_at, max_records=13)
    return (start(env, 3, 5, steps),) + ring_policies()


def lamps_case(bad_at=-1, bad_kind=0):
    """Lamps 12: observe_n, 1 .. 12 ids per state.  (A state without a lit lamp is final -- lamps.hpp's is_final() -- so no solve ever
    evaluates a zero-id observation of it; the count 0 stays with the collect tests.)"""
    from tests.var_obs_util import lamps, lamps_policy_arrays, lamps_twists
    env = lamps(12, max_steps=10, difficulty=3, bad_at=bad_at, bad_kind=bad_kind)
    return start(env, 3, 5, 1), lamps_policy_arrays(12), lamps_twists(12)


def probe_case(module):
    """A row of tests/device_env_matrix.py (probe_o64a4s: the struct of exactly 1 KiB, which the kernels keep in scratch memory)."""
    from tests import device_env_matrix as M
    r = M.BY_MODULE[module]
    return start(M.probe(r), r.seed, 5, 1), M.policy_arrays(module), M.twists(module)


def big_puzzle_case():
    """BigPuzzleEnv<25> holding a 3 x 3 board: n_obs() = 9 below N_OBS = 25."""
    from tests.device_env_util import big_puzzle
    from tests.util import make_deep_policy_arrays
    env = big_puzzle(3, 3, 4, 2, 16, max_records=17)
    return start(env, 3, 5, 1), make_deep_policy_arrays(9, seed=7, emb=64, common=(64, 32), scale=2.0), ((), ())


def wide_case(module):
    """A row of tests/device_env_wide.py (5 .. 31 actions, the two-kernel module) one step after reset(row seed, WIDE_SEEDS[module][0])."""
    from tests import device_env_wide as W
    r = W.BY_MODULE[module]
    return start(W.make_env(r), r.seed, WIDE_SEEDS[module][0], 1), W.policy_arrays(module), W.twists(module)


def wide_search_case(module):
    """A row of tests/device_env_wide_search.py (the module with the search kernel) one step after reset(row seed, WS_EPISODE[module])."""
    from tests import device_env_wide_search as WS
    r = WS.BY_MODULE[module]
    return start(WS.make_env(r), r.seed, WS_EPISODE[module], 1), WS.policy_arrays(module), WS.twists(module)
