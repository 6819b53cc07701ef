"""Helpers of the device-environment search tests: the test structs built WITH the search kernel (build_device_env(search=True),
TW_DEVICE_ENV_SEARCH) under module names of their own -- the modules tests/device_env_util.py and tests/var_obs_util.py build stay
as they are -- and the host-stepped calls over a module's vtable that the device results are held against."""
import ctypes as C

from tests.device_env_util import BIG_PUZZLE_HPP, GRIDWORLD_HPP, RING_HPP
from tests.var_obs_util import LAMPS_HPP


def build_gridworld_az():
    from twisterl_amd.build import build_device_env
    return build_device_env(GRIDWORLD_HPP, "tw_examples::GridWorld5x5", "gridworld5x5_az", search=True)


def build_ring_az():
    from twisterl_amd.build import build_device_env
    return build_device_env(RING_HPP, "RingWalk", "ring_az", search=True)


def build_lamps_az():
    from twisterl_amd.build import build_device_env
    return build_device_env(LAMPS_HPP, "Lamps12", "lamps12_az", search=True)


def build_big_puzzle_az():
    from twisterl_amd.build import build_device_env
    return build_device_env(BIG_PUZZLE_HPP, "BigPuzzle25", "big_puzzle25_az", search=True)


SEARCH_MODULES = {"gridworld5x5_az": build_gridworld_az, "ring_az": build_ring_az, "lamps12_az": build_lamps_az,
                  "big_puzzle25_az": build_big_puzzle_az}


def gridworld_az(max_steps=64, difficulty=1, **kw):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_gridworld_az(), "gridworld5x5_az", [5, 5, max_steps, difficulty], **kw)


def ring_az(n=32, max_steps=40, difficulty=3, noise=0.2, bad_at=-1, **kw):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_ring_az(), "ring_az", [n, max_steps, difficulty, noise, bad_at], **kw)


def lamps_az(max_steps=23, difficulty=3, bad_at=-1, bad_kind=0, **kw):
    from twisterl_amd.env import DeviceEnv
    kw.setdefault("max_records", max_steps + 1)
    return DeviceEnv(build_lamps_az(), "lamps12_az", [max_steps, difficulty, bad_at, bad_kind], **kw)


def big_puzzle_az(width, height, difficulty, depth_slope, max_depth, **kw):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_big_puzzle_az(), "big_puzzle25_az", [width, height, difficulty, depth_slope, max_depth], **kw)


def _vtable(env):
    from twisterl_amd import _lib
    vt = _lib.EnvVTable()
    _lib.check(_lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)))
    return vt


def host_az_collect(env, policy, E, S, Cc, med, seed, offset=0, merge_order=True):
    """tw_az_collect_env over the module's host vtable: the host-stepped path, called directly."""
    from twisterl_amd import _lib
    from twisterl_amd.collector import CollectedData, _DeviceResult
    vt = _vtable(env)
    prm = _lib.AZParams(E, offset, S, Cc, med, seed, _lib.TW_PREC_F32_EXACT, int(merge_order), 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_az_collect_env(C.byref(vt), policy._handle(), C.byref(prm), env.max_records, C.byref(out)))
    return CollectedData._from_device(_DeviceResult(out.value))


def host_evaluate(env, policy, n, det, ns, S, seed, Cc=1.41, med=1):
    """tw_evaluate_env over the module's host vtable, called directly -> (success_rate, mean_reward)."""
    from twisterl_amd import _lib
    vt = _vtable(env)
    prm = _lib.SolveParams(int(det), ns, S, Cc, med, seed, _lib.TW_PREC_F32_EXACT)
    s, r = C.c_float(), C.c_float()
    _lib.check(_lib.lib().tw_evaluate_env(C.byref(vt), policy._handle(), C.byref(prm), n, 0, env.max_records, C.byref(s), C.byref(r)))
    return float(s.value), float(r.value)
