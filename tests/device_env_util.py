"""Helpers of the device-environment tests: the test modules (examples/device_env/gridworld.hpp, tests/device_envs/ring.hpp,
tests/device_envs/big_puzzle.hpp) and a wrapper that gives a module's host functions the oracle's Python env protocol."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDWORLD_HPP = os.path.join(ROOT, "examples", "device_env", "gridworld.hpp")
RING_HPP = os.path.join(ROOT, "tests", "device_envs", "ring.hpp")
BIG_PUZZLE_HPP = os.path.join(ROOT, "tests", "device_envs", "big_puzzle.hpp")
GRIDWORLD_FIELDS = ("max_steps", "diff", "ax", "ay", "gx", "gy", "tx", "ty", "steps_left")     # struct GridWorld, int32 each


def build_gridworld(size=5):
    from twisterl_amd.build import build_device_env
    return build_device_env(GRIDWORLD_HPP, f"tw_examples::GridWorld{size}x{size}", f"gridworld{size}x{size}")


def build_ring():
    from twisterl_amd.build import build_device_env
    return build_device_env(RING_HPP, "RingWalk", "ring")


def build_big_puzzle():
    from twisterl_amd.build import build_device_env
    return build_device_env(BIG_PUZZLE_HPP, "BigPuzzle25", "big_puzzle25")


def gridworld(size=5, max_steps=64, difficulty=1, **kw):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_gridworld(size), f"gridworld{size}x{size}", [size, size, max_steps, difficulty], **kw)


def ring(n=32, max_steps=40, difficulty=3, noise=0.2, bad_at=-1, **kw):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_ring(), "ring", [n, max_steps, difficulty, noise, bad_at], **kw)


def big_puzzle(width, height, difficulty, depth_slope, max_depth, **kw):
    """tw::BigPuzzleEnv<25> (boards of up to 25 cells) with Puzzle::new's parameters."""
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_big_puzzle(), "big_puzzle25", [width, height, difficulty, depth_slope, max_depth], **kw)


class HostEnv:
    """The oracle's env protocol (copy, seed_episode, reset, next, masks, is_final, value, observe, success) over a device
    environment's host vtable (tw_device_env_host_vtable): the struct's own C++ code, run by the oracle's Python collectors."""

    def __init__(self, env, obj=None):
        from twisterl_amd import _lib
        self._env = env
        self._vt = _lib.EnvVTable()
        _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(self._vt)))
        self._owned = obj is not None
        self._obj = obj if obj is not None else env._obj
        self._key = (0, 0)

    def __del__(self):
        if getattr(self, "_owned", False) and self._obj:
            self._vt.destroy(self._obj)
            self._obj = None

    def copy(self):
        c = HostEnv(self._env, self._vt.clone(self._obj))
        c._key = self._key
        return c

    def seed_episode(self, seed, episode):
        self._key = (int(seed), int(episode))

    def reset(self, difficulty=None):                # the struct carries its own difficulty
        self._vt.reset(self._obj, self._key[0] & (2**64 - 1), self._key[1])

    def next(self, action):
        self._vt.step(self._obj, int(action))

    def num_actions(self):
        return int(self._vt.num_actions)

    def masks(self):
        out = (C.c_uint8 * self._vt.num_actions)()
        self._vt.masks(self._obj, out)
        return [bool(x) for x in out]

    def is_final(self):
        return bool(self._vt.is_final(self._obj))

    def value(self):
        return float(self._vt.reward(self._obj))

    def success(self):
        return bool(self._vt.success(self._obj))

    def observe(self):
        out = (C.c_int32 * self._vt.n_obs)()
        self._vt.observe(self._obj, out)
        return [int(x) for x in out]
