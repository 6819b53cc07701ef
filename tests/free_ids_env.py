"""A Python environment whose obs ids follow NO layout: test fixture for the trainer hand-off (tests/test_gpu_trainer_handoff.py).

The reference's Python env protocol (python_interface/pyenv.rs) asks of observe() only ids inside obs_shape -- in any order, with
repeats; the trainer's one-hot is `np_obs[i, obs_i] = 1.0` (src/twisterl/rl/ppo.py:37-39).  Puzzle, GridWorld and RingWalk all happen
to put an id of [k * n2, (k + 1) * n2) at position k; this one does not.

The dynamics: a walk on `n` positions of a ring.  Action k moves by +1, -1, +2, -2, ... (k // 2 + 1 steps, forwards when k is even);
an action is legal by a fixed rule of the position; the episode ends on the goal or after `max_steps` moves (at most max_steps + 1
records).  reset(difficulty) draws the start anywhere and the goal 0 .. difficulty steps ahead of it (0: the episode starts solved and
has one record) from a generator seeded per (seed, episode): nothing else is random.

LAYOUTS: name -> (n positions, obs_size, ids per observation, what observe() returns)
  a   2 ids of 64:  [32 + goal, pos]                     the two halves swapped (a cell-major reader finds nothing in either)
  b   3 ids of 27:  anywhere, two of them equal in some states
  c   3 ids of 50:  50 is no multiple of 3; repeats in some states
  d  64 ids of 256: the largest shape the one-hot hand-off takes, the ids spread over all of [0, 256)
  e   8 ids of 5:   more ids than distinct values (every observation repeats)
"""
import random

import numpy as np

LAYOUTS = {
    "a": (32, 64, 2, lambda p, g: [32 + g, p]),
    "b": (27, 27, 3, lambda p, g: [(5 * p + 3) % 27, g, (p + g) % 27]),
    "c": (50, 50, 3, lambda p, g: [p, g, (3 * p + 7) % 50]),
    "d": (256, 256, 64, lambda p, g: [(p * (k + 1) + g + 4 * k) % 256 for k in range(64)]),
    "e": (5, 5, 8, lambda p, g: [(p + k * g) % 5 for k in range(8)]),
}
ACTIONS = {"a": 4, "b": 3, "c": 5, "d": 17, "e": 31}          # actions per layout in the hand-off tests: 3, 4, 5, 17 and 31


class FreeIdsWalk:
    def __init__(self, layout, n_actions, max_steps=19):
        self.layout, self.n_actions_, self.max_steps = layout, int(n_actions), int(max_steps)
        self.n, self.obs_size, self.n_obs, self._ids = LAYOUTS[layout]
        self.pos = self.goal = 0
        self.steps_left = self.max_steps
        self.rng = random.Random(0)
        self.max_records = self.max_steps + 1

    def copy(self):
        c = FreeIdsWalk(self.layout, self.n_actions_, self.max_steps)
        c.pos, c.goal, c.steps_left = self.pos, self.goal, self.steps_left
        return c

    def seed_episode(self, seed, episode):
        self.rng = random.Random(seed * 1000003 + episode)

    def num_actions(self):
        return self.n_actions_

    def obs_shape(self):
        return [self.obs_size]

    def reset(self, difficulty):
        self.pos = self.rng.randrange(self.n)
        self.goal = (self.pos + self.rng.randrange(min(int(difficulty), self.n - 1) + 1)) % self.n
        self.steps_left = self.max_steps

    def next(self, action):
        k = int(action)
        self.pos = (self.pos + (k // 2 + 1) * (1 if k % 2 == 0 else -1)) % self.n
        self.steps_left = max(0, self.steps_left - 1)

    def masks(self):
        # about two actions of three; action pos % A always, so that one is legal in every state; position 1: that one alone
        A, p = self.n_actions_, self.pos
        return [k == p % A or (p != 1 and (p + 2 * k) % 3 != 0) for k in range(A)]

    def is_final(self):
        return self.steps_left == 0 or self.pos == self.goal

    def success(self):
        return self.pos == self.goal

    def value(self):
        if self.pos == self.goal:
            return 1.0
        if self.steps_left == 0:
            return -0.5
        return -0.5 / float(self.steps_left)

    def observe(self):
        return self._ids(self.pos, self.goal)

    def set_state(self, state):
        self.pos, self.goal = int(state[0]) % self.n, int(state[1]) % self.n
        self.steps_left = self.max_steps


def all_states(layout, stride=1):
    """(obs ids [m, n_obs], masks [m, A]) of every (position, goal) pair of a layout (every stride-th position and goal), with
    ACTIONS[layout] actions."""
    env = FreeIdsWalk(layout, ACTIONS[layout])
    obs, masks = [], []
    for p in range(0, env.n, stride):
        for g in range(0, env.n, stride):
            env.set_state([p, g])
            obs.append(env.observe())
            masks.append(env.masks())
    return np.asarray(obs, np.int64), np.asarray(masks, bool)


def policy_arrays(layout, seed=0, max_logit=None):
    """A policy for a layout from tests.util.make_deep_policy_arrays(..., n_actions=ACTIONS[layout]): its embedding table cut to the
    layout's obs_size rows.  max_logit: the last action layer scaled so that the largest |logit| over the environment's states (float64;
    of the 256-position layout every fourth position and goal) is that number -- log-probs far from zero."""
    from tests.ref64 import forward_f64
    from tests.util import make_deep_policy_arrays
    obs_size = LAYOUTS[layout][1]
    n2 = int(np.ceil(np.sqrt(obs_size)))
    emb, eb, common, action, value = make_deep_policy_arrays(n2, seed=seed, emb=64, common=(64, 32), n_actions=ACTIONS[layout], scale=2.0)
    arrs = (np.ascontiguousarray(emb[:obs_size]), eb, common, action, value)
    if max_logit is not None:
        obs, masks = all_states(layout, stride=max(1, LAYOUTS[layout][0] // 64))
        l64, _ = forward_f64(arrs, [], [], obs, masks, np.full(len(obs), -1))
        f = np.float32(max_logit / np.abs(l64[masks]).max())
        w, b, relu = action[-1]
        arrs = (arrs[0], eb, common, action[:-1] + [(w * f, b * f, relu)], value)
    return arrs
