"""Self-play and MCTS-guided evaluate of device environments with 5 .. 31 actions ON THE DEVICE (TW_DEVICE_ENV_WIDE_SEARCH of
include/twisterl_device_env.hpp, build_device_env(wide_search=True)): one table row per module and the helpers
tests/test_device_env_wide_search_build.py (no GPU) and tests/test_gpu_device_env_wide_search.py share.

The rows are the structs of tests/device_env_wide.py -- the hash walk of tests/device_envs/wide.hpp with 5, 8 (observe_n, three twists),
16 (policy and value layers, two twists), 17 and 31 (EngineV<64>, mask bit 30, three twists) actions, the 28-action example
examples/device_env/permutation.hpp, a struct of three actions built WITH the opt-in -- under module names of their own (`_ws`: the
modules of the wide tests in the same cache directory stay as they are), and one struct more: tests/device_envs/wide_open.hpp, 31
actions that are all allowed in every state, so that its roots have 31 children.  Every row: 40 episodes (three workgroups, the last one
partial), at most 12 records per episode, S searches of {8, 40} (40 > 31: every child of a full root can be visited) and a
max_expand_depth of {1, 2}.

Row fields: the C++ type, the module name, the header, N_OBS, NUM_ACTIONS, var (observe_n), obs_size, the number of twists, the policy
(embedding width, common / policy / value layers), the constructor parameters, max_records, the difficulty, the seed of the row's
collects, S and max_expand_depth, and what the ORACLE runs of it (o_S searches, o_E episodes): its loop is pure Python, and a row whose
full size took it longer than some 20 s would be compared with it at fewer searches (never fewer than 17 episodes).  No row needs that
today -- the slowest, perm8, takes 12 s -- so o_S and o_E are S and E everywhere, and the GPU test asserts it."""
import functools
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from tests.device_env_matrix import engine_nc, host_env        # noqa: F401  (shared with the two tests)
from tests.device_env_wide import MAX_STEPS, PERM_HPP, WIDE_HPP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN_HPP = os.path.join(ROOT, "tests", "device_envs", "wide_open.hpp")
E = 40
C_UCB = 1.41
EVAL_SEED_OFFSET = 1000
EVAL_EPISODES = 12                    # evaluate: 12 episodes, deterministic with 1 attempt and sampled with 2
EVAL_S = 8                            # ... of 8 searches per move

Row = namedtuple("Row", "type module header n_obs A var obs_size twists emb common policy_layers value_layers params max_records diff seed "
                        "S med o_S o_E")


def W(type_, n_obs, A, var, obs_size, twists, emb, common, diff, seed, S, med, o_S=None, o_E=E, policy_layers=(), value_layers=(), header=WIDE_HPP):
    return Row(type_, type_.lower() + "_ws", header, n_obs, A, var, obs_size, twists, emb, common, policy_layers, value_layers,
               (obs_size, MAX_STEPS, diff, -1), MAX_STEPS + 1, diff, seed, S, med, o_S or S, o_E)


# common=(48,): one common layer that is not the MFMA shape, so the device kernel takes the policy at any obs_size
TABLE = [
    #  type        N_OBS  A  var    obs_size tw emb common    diff seed  S med
    W("WideO2A5",     2,  5, False,    64, 0, 32, (48,),      8, 41, 40, 2),
    W("WideO5A8V",    5,  8, True,    257, 3, 32, (48,),      8, 42,  8, 1),
    W("WideO16A16",  16, 16, False,   500, 2, 32, (48,),      8, 43,  8, 2, policy_layers=(32,), value_layers=(16,)),
    W("WideO17A17",  17, 17, False,   300, 0, 64, (64, 32),   8, 44,  8, 1),
    W("WideO64A31",  64, 31, False,  4096, 3, 32, (48,),      8, 45,  8, 2),
    Row("tw_examples::Permutation8", "perm8_ws", PERM_HPP, 8, 28, False, 64, 0, 32, (48,), (), (), (8, MAX_STEPS, 2), MAX_STEPS + 1, 2, 46,
        40, 1, 40, E),
    W("WideO4A3",     4,  3, False,    64, 2, 32, (48,),      8, 47,  8, 2),
    W("WideOpenA31",  4, 31, False,    64, 0, 32, (48,),      8, 49, 40, 2, header=OPEN_HPP),
]
# not a row of the table: one state in four allows NO action (tests/device_envs/wide_open.hpp), which the oracle cannot run -- held to
# the host-stepped path alone, for the uniform fallback 1 / A of a root without children
SHUT = W("WideShutA7",    4,  7, False,    64, 2, 32, (48,),      8, 50,  8, 2, header=OPEN_HPP)
# not a row of the table either: six actions, all allowed, under three twists that keep the observation and rotate the actions within
# (0 1 2) and (3 4 5).  The actions of a cycle average the same three head outputs in three orders: their priors differ by the rounding
# of the twist average alone, and which of them the searches visit first says whether that average ran in the reference's order
# (x / n added pass by pass from 0.0f).  The visit counts of every other row are deaf to the last bit of a prior.
TIE = W("WideTieA6",     4,  6, False,    64, 3, 32, (48,),      8, 51,  8, 1, header=OPEN_HPP)
EXTRA = [SHUT, TIE]
BY_MODULE = {r.module: r for r in TABLE + EXTRA}
IDS = [r.module for r in TABLE]
PERM8 = "perm8_ws"
ALL_OPEN = "wideopena31_ws"
OPT_IN_WITHOUT_USE = "wideo4a3_ws"
ERROR_ROW = "wideo64a31_ws"
HANDOFF_ROW = "wideo17a17_ws"
FALLBACK_ROW = "wideo2a5_ws"


@functools.lru_cache(maxsize=None)
def build_all():
    """Builds every row's module once per session (side by side, at most 16 at a time) -> {module name: path of the .so}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    rows = TABLE + EXTRA
    with ThreadPoolExecutor(max_workers=min(16, len(rows))) as pool:
        paths = list(pool.map(lambda r: build_device_env(r.header, r.type, r.module, wide_search=True), rows))
    return {r.module: p for r, p in zip(rows, paths)}


def make_env(row, bad_at=-1, max_records=None):
    from twisterl_amd.env import DeviceEnv
    params = list(row.params)
    if bad_at >= 0:
        assert row.header != PERM_HPP
        params[3] = bad_at
    return DeviceEnv(build_all()[row.module], row.module, params, max_records=max_records or row.max_records)


@functools.lru_cache(maxsize=None)
def policy_arrays(module):
    from tests.util import make_deep_policy_arrays_obs
    r = BY_MODULE[module]
    return make_deep_policy_arrays_obs(r.obs_size, seed=100 + r.seed, emb=r.emb, common=r.common, policy_layers=r.policy_layers,
                                       value_layers=r.value_layers, n_actions=r.A, scale=2.0)   # (logits that differ: a wrong sum flips actions)


@functools.lru_cache(maxsize=None)
def twists(module):
    """Seeded random permutations of [0, obs_size) and of the A actions, the identity first."""
    r = BY_MODULE[module]
    if r.twists == 0:
        return (), ()
    if module == TIE.module:
        ident = list(range(r.obs_size))
        return [ident, ident, ident], [[0, 1, 2, 3, 4, 5], [1, 2, 0, 4, 5, 3], [2, 0, 1, 5, 3, 4]]
    rng = np.random.default_rng(500 + r.seed)
    obs = [list(range(r.obs_size))] + [rng.permutation(r.obs_size).tolist() for _ in range(r.twists - 1)]
    act = [list(range(r.A))] + [rng.permutation(r.A).tolist() for _ in range(r.twists - 1)]
    return obs, act


def policies(O, row):
    """(the library's policy, the oracle's) over the row's weights and twists."""
    from tests.util import amd_policy, oracle_policy
    tw = twists(row.module)
    return amd_policy(policy_arrays(row.module), *tw), oracle_policy(O, policy_arrays(row.module), *tw)


class _Counting:
    """The oracle's policy with its full_predict calls counted: one per evaluated state, a root or a leaf."""

    def __init__(self, policy):
        self._p, self.evals = policy, 0

    def __getattr__(self, name):
        return getattr(self._p, name)

    def full_predict(self, *a, **kw):
        self.evals += 1
        return self._p.full_predict(*a, **kw)


def oracle_self_play(O, proto, policy, num_episodes, S, C_, med, seed, n_obs, difficulty):
    """oracle.az_collect_env (AZCollector::collect, az.rs:51-109, over oracle.mcts_probs_env) restated as tests/var_obs_util.py
    restates it for observations of any length, keeping what that function drops: the action each move took (per episode, in index
    order) and the number of states the searches evaluated.  Caller: set_det_exp(True) around the call."""
    from tests.var_obs_util import _pad, _u01
    f32 = np.float32
    pol = _Counting(policy)
    eps = []
    for ep in range(num_episodes):
        env = proto.copy()
        env.seed_episode(seed, ep)
        env.reset(difficulty)
        obs_l, prob_l, val_l, act_l = [], [], [], []
        t = 0
        while True:
            mp = O.mcts_probs_env(env, pol, S, C_, med, seed, ep, t, arith=O.ARITH_CHAIN)
            w = O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t, 3], [seed & 0xFFFFFFFF, seed >> 32])
            action = O.sample_weighted(mp, float(_u01(w[0])))
            obs_l.append([int(x) for x in env.observe()]); prob_l.append(mp); val_l.append(f32(env.value()))
            if env.is_final():
                break
            act_l.append(action)
            env.next(action)
            t += 1
        total, before = f32(0), []
        for v in val_l:
            before.append(total)
            total = f32(total + v)
        eps.append((obs_l, prob_l, [f32(total - b) for b in before], act_l))
    order = [num_episodes - 1] + list(range(num_episodes - 1))                     # (merge order: the last episode first)
    n_of = [len(e[2]) for e in eps]
    lists = [o for i in order for o in eps[i][0]]
    cat = lambda k: np.concatenate([np.asarray(eps[i][k], dtype=np.float32).reshape(n_of[i], -1) for i in order])
    return SimpleNamespace(obs_lists=lists, obs=_pad(lists, n_obs), counts=np.asarray([len(o) for o in lists], dtype=np.int64),
                           logits=cat(1), remaining_values=cat(2).reshape(-1), ep_len=np.asarray(n_of, dtype=np.uint32),
                           actions=[e[3] for e in eps], evals=pol.evals)


@functools.lru_cache(maxsize=None)
def shared_self_play(module):
    """The oracle's self-play over the module's own host code at the row's seed (o_E episodes of o_S searches): what the CPU test holds
    its input conditions against and the GPU test compares with.  Computed once per process, never modified."""
    from oracle import oracle as O
    from tests.util import oracle_policy
    O.build()
    r = BY_MODULE[module]
    O.set_det_exp(True)
    try:
        return oracle_self_play(O, host_env(make_env(r)), oracle_policy(O, policy_arrays(module), *twists(module)), r.o_E, r.o_S, C_UCB, r.med,
                                r.seed, r.n_obs, r.diff)
    finally:
        O.set_det_exp(False)
