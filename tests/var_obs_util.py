"""Helpers of the variable-length-observation tests: the lamps modules (tests/device_envs/lamps.hpp, N_OBS 12 and 40), a host wrapper
whose observe() returns the ids a state HAS (tw_env_vtable.observe_n), a Python environment of the same kind for PyEnv, and the oracle's
PPO / self-play loops over such environments -- oracle.ppo_collect_env / az_collect_env end in a fixed-width np.asarray, so the loops are
restated here from the oracle's public pieces (Policy.forward, philox4x32_10, sample_from_logits, gae; mcts_probs_env, sample_weighted).
Both return the obs as the library lays them out: uint16 [records, n_obs], a record's ids first, 0xFFFF in the free slots."""
import ctypes as C
import functools
import os
import random
from types import SimpleNamespace

import numpy as np

from tests.device_env_util import HostEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMPS_HPP = os.path.join(ROOT, "tests", "device_envs", "lamps.hpp")
NO_ID = 0xFFFF
SIZES = (12, 40)                 # N_OBS 12: EngineV<16>, every row of a column in registers; 40: EngineV<64>, rows in blocks of 16
# the collect every test shares: 150 episodes = nine workgroups of 16 and one of six
E, MAX_STEPS, MAX_RECORDS, DIFFICULTY, SEED, GAMMA, LAM = 150, 23, 24, 3, 29, 0.99, 0.95


def build_lamps(n):
    from twisterl_amd.build import build_device_env
    return build_device_env(LAMPS_HPP, f"Lamps{n}", f"lamps{n}")


def lamps(n, max_steps=MAX_STEPS, difficulty=DIFFICULTY, bad_at=-1, bad_kind=0, **kw):
    from twisterl_amd.env import DeviceEnv
    kw.setdefault("max_records", max_steps + 1)
    return DeviceEnv(build_lamps(n), f"lamps{n}", [max_steps, difficulty, bad_at, bad_kind], **kw)


class VarHostEnv(HostEnv):
    """HostEnv whose observe() is the vtable's observe_n: the ids of this state, however many."""

    def copy(self):
        c = VarHostEnv(self._env, self._vt.clone(self._obj))
        c._key = self._key
        return c

    def observe(self):
        cap = int(self._vt.n_obs)
        out = (C.c_int32 * cap)()
        k = int(self._vt.observe_n(self._obj, out, cap))
        assert k <= cap, (k, cap)
        return [int(x) for x in out[:k]]


def lamps_policy_arrays(n, seed=5):
    """A deep generic stack (two common layers: EngineV, not the MFMA shape) over the lamps' obs_size n * n."""
    from tests.util import make_deep_policy_arrays
    return make_deep_policy_arrays(n, seed=seed, emb=64, common=(64, 32), n_actions=4)


def lamps_twists(n):
    """Two twists over the n * n ids: identity, and the lamps mirrored with toggle / toggle-pair swapped.  (Any permutation serves:
    a twist is data to the collectors.)"""
    ident = list(range(n * n))
    mir = [(n - 1 - i // n) * n + i % n for i in range(n * n)]
    return [ident, mir], [[0, 1, 2, 3], [1, 0, 2, 3]]


def _u01(word):
    return np.float32(word >> 8) * np.float32(1.0 / 16777216.0)


def _pad(obs_lists, n_obs):
    out = np.full((len(obs_lists), n_obs), NO_ID, dtype=np.uint16)
    for i, o in enumerate(obs_lists):
        assert len(o) <= n_obs
        out[i, :len(o)] = o
    return out


def oracle_ppo_loop(O, proto, policy, num_episodes, gamma, lam, seed, n_obs, episode_offset=0, difficulty=1, merge_order=True):
    """PPOCollector::collect (ppo.rs:41-126) as oracle.ppo_collect_env restates it, over observations of any length."""
    A = policy.n_actions
    eps = []
    for i in range(num_episodes):
        e = proto.copy()
        ep = episode_offset + i
        if hasattr(e, "seed_episode"):
            e.seed_episode(seed, ep)
        e.reset(difficulty)
        obs_l, lg_l, perm_l, val_l, rew_l, act_l = [], [], [], [], [], []
        t = 0
        while True:
            obs = [int(x) for x in e.observe()]
            masks = [bool(m) for m in e.masks()]
            rew = np.float32(e.value())
            perm = -1
            if policy.n_perms > 0:
                w = O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t, 2], [seed & 0xFFFFFFFF, seed >> 32])
                perm = (w[0] * policy.n_perms) >> 32
            lg, v = policy.forward(obs, masks, perm=perm, arith=O.ARITH_CHAIN)
            u = []
            for a in range(A):
                w = O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t | ((a >> 2) << 24), 1], [seed & 0xFFFFFFFF, seed >> 32])
                u.append(_u01(w[a & 3]))
            act = O.sample_from_logits(lg, u, det_log=True)
            obs_l.append(obs); lg_l.append(lg); perm_l.append(perm); val_l.append(v); rew_l.append(rew); act_l.append(act)
            if e.is_final():
                break
            e.next(act)
            t += 1
        advs, rets = O.gae(rew_l, val_l, gamma, lam)
        eps.append((obs_l, lg_l, perm_l, val_l, rew_l, act_l, advs, rets))
    order = ([num_episodes - 1] + list(range(num_episodes - 1))) if merge_order else list(range(num_episodes))
    cat = lambda k, dt: np.concatenate([np.asarray(eps[i][k], dtype=dt).reshape(len(eps[i][3]), -1) for i in order])
    lists = [o for i in order for o in eps[i][0]]
    return SimpleNamespace(obs_lists=lists, obs=_pad(lists, n_obs), counts=np.asarray([len(o) for o in lists], dtype=np.int64),
                           episodes=[eps[i][0] for i in range(num_episodes)],           # per episode (index order): its records' id lists
                           logits=cat(1, np.float32), perms=cat(2, np.int32).reshape(-1), values=cat(3, np.float32).reshape(-1),
                           rewards=cat(4, np.float32).reshape(-1), actions=cat(5, np.int64).reshape(-1), advs=cat(6, np.float32).reshape(-1),
                           rets=cat(7, np.float32).reshape(-1), ep_len=np.asarray([len(e[3]) for e in eps], dtype=np.uint32))


def oracle_az_loop(O, proto, policy, num_episodes, num_mcts_searches, C_, max_expand_depth, seed, n_obs, episode_offset=0, difficulty=1,
                   merge_order=True):
    """AZCollector::collect (az.rs:51-109) as oracle.az_collect_env restates it, over observations of any length.  Caller:
    set_det_exp(True) around the call."""
    f32 = np.float32
    eps = []
    for i in range(num_episodes):
        env = proto.copy()
        ep = episode_offset + i
        if hasattr(env, "seed_episode"):
            env.seed_episode(seed, ep)
        env.reset(difficulty)
        obs_l, prob_l, val_l = [], [], []
        t = 0
        while True:
            mp = O.mcts_probs_env(env, policy, num_mcts_searches, C_, max_expand_depth, seed, ep, t, arith=O.ARITH_CHAIN)
            w = O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t, 3], [seed & 0xFFFFFFFF, seed >> 32])
            action = O.sample_weighted(mp, float(_u01(w[0])))
            obs_l.append([int(x) for x in env.observe()]); prob_l.append(mp); val_l.append(f32(env.value()))
            if env.is_final():
                break
            env.next(action)
            t += 1
        total, before = f32(0), []
        for v in val_l:
            before.append(total)
            total = f32(total + v)
        eps.append((obs_l, prob_l, [f32(total - b) for b in before]))
    order = ([num_episodes - 1] + list(range(num_episodes - 1))) if merge_order else list(range(num_episodes))
    n_of = [len(e[2]) for e in eps]
    lists = [o for i in order for o in eps[i][0]]
    cat = lambda k: np.concatenate([np.asarray(eps[i][k], dtype=np.float32).reshape(n_of[i], -1) for i in order])
    return SimpleNamespace(obs_lists=lists, obs=_pad(lists, n_obs), counts=np.asarray([len(o) for o in lists], dtype=np.int64),
                           logits=cat(1), remaining_values=cat(2).reshape(-1), ep_len=np.asarray(n_of, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def shared_collect(n, twists=False, num_episodes=E):
    """The oracle's PPO loop over the lamps module's own host code, the collect the CPU test holds its input condition against and the
    GPU tests compare with: computed once per process, never modified."""
    from oracle import oracle as O
    from tests.util import oracle_policy
    O.build()
    env = lamps(n)
    tw = lamps_twists(n) if twists else ((), ())
    pol = oracle_policy(O, lamps_policy_arrays(n), *tw)
    return oracle_ppo_loop(O, VarHostEnv(env), pol, num_episodes, GAMMA, LAM, SEED, n, difficulty=DIFFICULTY)


class PyLamps:
    """A Python environment (the reference's protocol, python_interface/pyenv.rs) whose observation is the indices of the set bits of
    its state: 6 lamps, obs id of lit lamp b = 6 * b + (b + steps_left) % 6 (obs_shape [6, 6]), up to max_obs() = 6 of them."""
    N = 6

    def __init__(self, max_steps=9, declare_max=True):
        self.max_steps, self.steps_left, self.mask = max_steps, max_steps, 0
        self.rng = random.Random(0)
        self.max_records = max_steps + 1
        if declare_max:
            self.max_obs = lambda: self.N

    def copy(self):
        c = PyLamps(self.max_steps, hasattr(self, "max_obs"))
        c.steps_left, c.mask = self.steps_left, self.mask
        return c

    def seed_episode(self, seed, episode):
        self.rng = random.Random(seed * 1000003 + episode)

    def num_actions(self):
        return 4

    def obs_shape(self):
        return [self.N, self.N]

    def reset(self, difficulty):
        self.mask = 0
        for _ in range(1 + self.rng.randrange(max(1, difficulty))):
            self.next(self.rng.randrange(4))
        self.steps_left = 2 + self.rng.randrange(self.max_steps - 1)

    def next(self, action):
        if action == 3:
            self.mask ^= (1 << self.N) - 1
        else:
            self.mask ^= 1 << (2 * action + (self.steps_left & 1))
        self.steps_left = max(0, self.steps_left - 1)

    def masks(self):
        return [True, True, self.steps_left % 3 != 0, True]

    def is_final(self):
        return self.mask == 0 or self.steps_left == 0

    def value(self):
        return 1.0 if self.mask == 0 else (-0.5 if self.steps_left == 0 else -0.125 * bin(self.mask).count("1"))

    def success(self):
        return self.mask == 0

    def observe(self):
        return [self.N * b + (b + self.steps_left) % self.N for b in range(self.N) if (self.mask >> b) & 1]

    def set_state(self, state):
        self.mask = sum(1 << int(b) for b in state)
