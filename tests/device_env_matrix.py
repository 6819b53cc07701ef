"""The struct contract of include/twisterl_device_env.hpp, corner by corner: one table row per instantiation of the probe environment
(tests/device_envs/probe.hpp: a hash walk, `Probe<N_OBS, NUM_ACTIONS, K, VAR>`) and the helpers the two test files share.

The device-environment kernels (rollout_env_kernel, solve_env_kernel, mcts_env_kernel: twisterl_amd/csrc/tw_rollout_env.hpp,
tw_mcts_env.hpp) are templates over the user's struct; env_engine_nc() picks EngineV<4 | 9 | 16 | 25 | 36 | 64> from N_OBS.  The rows
cover every one of those classes and BOTH sides of every class edge (N_OBS 4|5, 9|10, 16|17, 25|26, 36|37, and the ends 1 and 64),
NUM_ACTIONS 1..4 for each of the three kernels, obs_size 1, 256 (one-byte ids, the id 255), 257 (the first two-byte size and the
first use of the two-byte twist table), 65535, three twists (full_predict's division by a number that is no power of two), a struct
of exactly 1,024 bytes and two of exactly 128 bytes (the search form's limit) whose run-time-indexed array compiles to scratch
memory, and observe_n with counts 0 and N_OBS.  tests/test_device_env_matrix.py (no GPU) holds the table to the built modules and
to the oracle's data; tests/test_gpu_device_env_matrix.py runs every row on the GPU, bitwise against the host-stepped path and
the oracle.

Row fields: the type alias in probe.hpp, the module name, N_OBS, NUM_ACTIONS, K (words of history), var (observe_n), obs_size, the
number of twists, the policy (embedding width, common / policy / value layers), search (built with the search kernel), scratch (the
struct is expected to leave the registers), the struct's size, max_steps and difficulty of the environment, the seed of the row's
collects and the episode offset of its PPO collects."""
import functools
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_HPP = os.path.join(ROOT, "tests", "device_envs", "probe.hpp")
CLASSES = (4, 9, 16, 25, 36, 64)
GAMMA, LAM = 0.99, 0.95
EPISODES = (40, 100)                  # 2.5 and 6.25 workgroups of 16 columns
EVAL_SEED_OFFSET = 1000               # evaluate runs with seed + this

Row = namedtuple("Row", "alias module n_obs A K var obs_size twists emb common policy_layers value_layers search scratch state_bytes "
                        "max_steps diff seed offset")


def R(alias, n_obs, A, K, var, obs_size, twists, emb, common, search, max_steps, diff, seed, policy_layers=(), value_layers=(),
      scratch=False, offset=0):
    return Row(alias, "probe_" + alias[5:].lower(), n_obs, A, K, var, obs_size, twists, emb, common, policy_layers, value_layers, search, scratch,
               (32 + 4 * K + 7) // 8 * 8, max_steps, diff, seed, offset)


# common=(48,): ONE common layer that is not the MFMA shape (48 is no multiple of 32), so the device kernel takes it at any obs_size
TABLE = [
    #  alias          N_OBS A   K  var    obs_size tw emb common    search steps diff seed
    R("ProbeO1A1",      1, 1,   1, False,     1, 0, 32, (48,),     True,  9,  6, 11),
    R("ProbeO4A2",      4, 2,   1, False,   256, 2, 64, (64, 32),  True, 12,  8, 12, offset=1000),
    R("ProbeO5A3V",     5, 3,   1, True,    257, 3, 32, (48,),     True, 10,  7, 13),
    R("ProbeO9A3S",     9, 3,  24, False,    81, 0, 64, (32, 32),  True, 12,  8, 14, scratch=True),
    R("ProbeO10A4V",   10, 4,   1, True,    100, 0, 32, (64,),     False, 11, 7, 15, policy_layers=(32,), value_layers=(16,)),
    R("ProbeO16A3",    16, 3,   1, False,   500, 0, 32, (48,),     True,  8,  6, 16),
    R("ProbeO17A2",    17, 2,   4, False,   300, 3, 64, (32,),     True, 12,  9, 17, policy_layers=(16,), value_layers=(32, 16)),
    R("ProbeO25A4V",   25, 4,   1, True,    625, 2, 32, (32, 32),  True,  9,  7, 18),
    R("ProbeO26A1V",   26, 1,   4, True,    700, 0, 64, (48,),     True, 10,  8, 19, offset=(1 << 33) + 5),
    R("ProbeO36A4",    36, 4,   4, False,  1296, 2, 32, (64, 32),  True, 12,  8, 20),
    R("ProbeO37A3",    37, 3,   1, False,    64, 0, 64, (48,),     False, 7,  5, 21),
    R("ProbeO64A4S",   64, 4, 248, False, 65535, 0, 32, (32, 32),  False, 12, 8, 22, scratch=True),
    R("ProbeO64A2SV",  64, 2,  24, True,   4096, 2, 64, (48,),     True, 11,  8, 23, scratch=True, value_layers=(16,)),
]
BY_MODULE = {r.module: r for r in TABLE}
IDS = [r.module for r in TABLE]
SEARCH_IDS = [r.module for r in TABLE if r.search]
ERROR_ROWS = ("probe_o9a3s", "probe_o1a1")          # one scratch row and one NUM_ACTIONS = 1 row run the bad-id variant
HANDOFF_ROWS = ("probe_o4a2", "probe_o5a3v", "probe_o64a4s")      # obs_size 256 (one-byte ids), 257 and 65535 (two-byte ids)


def engine_nc(n_obs):
    """env_engine_nc (tw_rollout_env.hpp)."""
    return next(c for c in CLASSES if n_obs <= c)


@functools.lru_cache(maxsize=None)
def build_all():
    """Builds the module of EVERY row once per session and returns {module name: path of the .so}.  The compilations (one hipcc each,
    11-17 s with the search kernel) run side by side, AT MOST 16 AT A TIME: a GPU machine's os.cpu_count() is the whole machine's,
    not what one job may use, so the pool is not sized by it."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    with ThreadPoolExecutor(max_workers=min(16, len(TABLE))) as pool:
        paths = list(pool.map(lambda r: build_device_env(PROBE_HPP, r.alias, r.module, search=r.search), TABLE))
    return dict(zip(IDS, paths))


def probe(row, bad_at=-1):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[row.module], row.module, [row.obs_size, row.max_steps, row.diff, bad_at], max_records=row.max_steps + 1)


def host_env(env):
    """The oracle's env protocol over the module's host vtable; a struct with observe_n: the ids the state HAS."""
    from tests.device_env_util import HostEnv
    from tests.var_obs_util import VarHostEnv
    return VarHostEnv(env) if env.variable_obs else HostEnv(env)


@functools.lru_cache(maxsize=None)
def policy_arrays(module):
    from tests.util import make_deep_policy_arrays_obs
    r = BY_MODULE[module]
    return make_deep_policy_arrays_obs(r.obs_size, seed=100 + r.seed, emb=r.emb, common=r.common, policy_layers=r.policy_layers,
                                       value_layers=r.value_layers, n_actions=r.A, scale=2.0)   # (logits that differ: a wrong sum flips actions)


@functools.lru_cache(maxsize=None)
def twists(module):
    """Seeded random permutations of [0, obs_size) and of the actions, the identity first.  A twist is data to both paths."""
    r = BY_MODULE[module]
    if r.twists == 0:
        return (), ()
    rng = np.random.default_rng(500 + r.seed)
    obs = [list(range(r.obs_size))] + [rng.permutation(r.obs_size).tolist() for _ in range(r.twists - 1)]
    act = [list(range(r.A))] + [rng.permutation(r.A).tolist() for _ in range(r.twists - 1)]
    return obs, act


def policies(O, row):
    """(the library's policy, the oracle's) over the row's weights and twists."""
    from tests.util import amd_policy, oracle_policy
    tw = twists(row.module)
    return amd_policy(policy_arrays(row.module), *tw), oracle_policy(O, policy_arrays(row.module), *tw)


def oracle_only_policy(O, row):
    from tests.util import oracle_policy
    return oracle_policy(O, policy_arrays(row.module), *twists(row.module))


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def shared_collect(module, E):
    """The oracle's PPO loop over the module's own host code at the row's seed and offset: what the CPU test holds its input conditions
    against and the GPU test compares with.  Computed once per process, never modified.  Fields as tests/var_obs_util.oracle_ppo_loop's
    (obs: uint16 [records, N_OBS], 0xFFFF in the slots a record leaves free; obs_lists; counts; ...)."""
    from tests.var_obs_util import oracle_ppo_loop
    O = _oracle()
    r = BY_MODULE[module]
    return oracle_ppo_loop(O, host_env(probe(r)), oracle_only_policy(O, r), E, GAMMA, LAM, r.seed, r.n_obs, episode_offset=r.offset,
                           difficulty=r.diff)


@functools.lru_cache(maxsize=None)
def reset_is_final(module, n):
    """For episodes 0 .. n - 1 of the row's evaluate (seed + EVAL_SEED_OFFSET, no offset): is the reset state final?"""
    r = BY_MODULE[module]
    h = host_env(probe(r))
    out = []
    for e in range(n):
        c = h.copy()
        c.seed_episode(r.seed + EVAL_SEED_OFFSET, e)
        c.reset()
        out.append(c.is_final())
    return tuple(out)
