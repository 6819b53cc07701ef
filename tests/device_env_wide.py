"""Device environments of 5 .. 31 actions (TW_DEVICE_ENV_WIDE of include/twisterl_device_env.hpp, build_device_env(wide=True)): one
table row per module and the helpers tests/test_device_env_wide_build.py (no GPU) and tests/test_gpu_device_env_wide.py share.

The rows: the hash walk of tests/device_envs/wide.hpp at the corners of the streaming step -- 5 actions (the first value past the edge;
the second Gumbel draw uses one word), 8 (two whole draws, observe_n, three twists with a two-byte twist table), 16 (a full head tile;
policy_layers + value_layers: the stack() head path of EngineV::forward), 17 (the head's second tile holds one row), 31 (the limit: mask
bit 30, draw index 7, EngineV<64>) -- the example examples/device_env/permutation.hpp with N = 8 (28 actions), and a struct of three
actions built WITH the opt-in.  Every row: 40 episodes, at most 12 records per episode.

Row fields: the C++ type, the module name, the header, N_OBS, NUM_ACTIONS, var (observe_n), obs_size, the number of twists, the policy
(embedding width, common / policy / value layers), the constructor parameters, max_records, the difficulty and the seed of the row's
collects."""
import functools
import os
from collections import namedtuple

import numpy as np

from tests.device_env_matrix import EVAL_SEED_OFFSET, GAMMA, LAM, engine_nc, host_env        # noqa: F401  (shared with the two tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_HPP = os.path.join(ROOT, "tests", "device_envs", "wide.hpp")
PERM_HPP = os.path.join(ROOT, "examples", "device_env", "permutation.hpp")
E = 40
MAX_STEPS = 11                        # at most 12 records per episode

Row = namedtuple("Row", "type module header n_obs A var obs_size twists emb common policy_layers value_layers params max_records diff seed")


def W(type_, n_obs, A, var, obs_size, twists, emb, common, diff, seed, policy_layers=(), value_layers=()):
    return Row(type_, type_.lower(), WIDE_HPP, n_obs, A, var, obs_size, twists, emb, common, policy_layers, value_layers,
               (obs_size, MAX_STEPS, diff, -1), MAX_STEPS + 1, diff, seed)


# common=(48,): one common layer that is not the MFMA shape, so the device kernel takes the policy at any obs_size
TABLE = [
    #  type        N_OBS  A  var    obs_size tw emb common    diff seed
    W("WideO2A5",     2,  5, False,    64, 0, 32, (48,),      8, 31),
    W("WideO5A8V",    5,  8, True,    257, 3, 32, (48,),      8, 32),
    W("WideO16A16",  16, 16, False,   500, 2, 32, (48,),      8, 33, policy_layers=(32,), value_layers=(16,)),
    W("WideO17A17",  17, 17, False,   300, 0, 64, (64, 32),   8, 34),
    W("WideO64A31",  64, 31, False,  4096, 3, 32, (48,),      8, 35),
    Row("tw_examples::Permutation8", "perm8", PERM_HPP, 8, 28, False, 64, 0, 32, (48,), (), (), (8, MAX_STEPS, 2), MAX_STEPS + 1, 2, 36),
    W("WideO4A3",     4,  3, False,    64, 2, 32, (48,),      8, 37),
]
BY_MODULE = {r.module: r for r in TABLE}
IDS = [r.module for r in TABLE]
PERM8 = "perm8"
OPT_IN_WITHOUT_USE = "wideo4a3"
ERROR_ROW = "wideo64a31"
HANDOFF_ROWS = ("wideo17a17", "wideo64a31")
AZ_ROW = "wideo2a5"


@functools.lru_cache(maxsize=None)
def build_all():
    """Builds every row's module once per session (side by side, at most 16 at a time) -> {module name: path of the .so}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    with ThreadPoolExecutor(max_workers=min(16, len(TABLE))) as pool:
        paths = list(pool.map(lambda r: build_device_env(r.header, r.type, r.module, wide=True), TABLE))
    return dict(zip(IDS, paths))


def make_env(row, bad_at=-1):
    from twisterl_amd.env import DeviceEnv
    params = list(row.params)
    if bad_at >= 0:
        assert row.header == WIDE_HPP
        params[3] = bad_at
    return DeviceEnv(build_all()[row.module], row.module, params, max_records=row.max_records)


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
    rng = np.random.default_rng(500 + r.seed)
    obs = [list(range(r.obs_size))] + [rng.permutation(r.obs_size).tolist() for _ in range(r.twists - 1)]
    act = [list(range(r.A))] + [rng.permutation(r.A).tolist() for _ in range(r.twists - 1)]
    return obs, act


def policies(O, row):
    """(the library's policy, the oracle's) over the row's weights and twists."""
    from tests.util import amd_policy, oracle_policy
    tw = twists(row.module)
    return amd_policy(policy_arrays(row.module), *tw), oracle_policy(O, policy_arrays(row.module), *tw)


@functools.lru_cache(maxsize=None)
def shared_collect(module):
    """The oracle's PPO loop over the module's own host code at the row's seed: what the CPU test holds its input conditions against
    and the GPU test compares with.  Computed once per process, never modified."""
    from oracle import oracle as O
    from tests.util import oracle_policy
    from tests.var_obs_util import oracle_ppo_loop
    O.build()
    r = BY_MODULE[module]
    return oracle_ppo_loop(O, host_env(make_env(r)), oracle_policy(O, policy_arrays(module), *twists(module)), E, GAMMA, LAM, r.seed, r.n_obs,
                           difficulty=r.diff)
