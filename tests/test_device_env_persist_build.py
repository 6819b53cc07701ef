"""CPU: the persistent grid of the device-environment kernels (EnvRolloutArgs::queue) -- what can be checked without a device.  Every
test module's descriptor carries groups_per_cu, the occupancy query from which the library sizes the grid (it is what an older
module lacks: layout[2], the descriptor's size, then differs and the library says "rebuild it"), and the test hook
TW_OPT_ENV_RESIDENT_GROUPS takes a count, refuses a negative one and goes back to automatic with 0."""
import ctypes as C

import pytest

from tests.device_env_search_util import SEARCH_MODULES, gridworld_az, lamps_az, ring_az
from tests.device_env_util import gridworld, ring
from tests.var_obs_util import lamps


def _envs():
    return {"gridworld": gridworld, "ring": ring, "lamps12": lambda: lamps(12), "lamps40": lambda: lamps(40),
            "gridworld_az": gridworld_az, "ring_az": ring_az, "lamps_az": lamps_az}


@pytest.mark.parametrize("name", sorted(_envs()))
def test_every_descriptor_has_the_occupancy_query(name):
    from twisterl_amd.env import DeviceEnvDesc
    env = _envs()[name]()
    d = env._desc
    assert d.groups_per_cu, name                                           # (a null function pointer is falsy)
    assert d.layout[2] == C.sizeof(DeviceEnvDesc) and len(d.layout) == 8
    assert DeviceEnvDesc.groups_per_cu.offset == DeviceEnvDesc.launch_search.offset + C.sizeof(C.c_void_p)   # appended: the last member
    assert bool(d.launch_search) == name.endswith("_az")


def test_search_modules_all_carry_it():
    from twisterl_amd.env import DeviceEnvDesc
    for name in sorted(SEARCH_MODULES):
        mod = C.CDLL(SEARCH_MODULES[name]())
        fn = getattr(mod, f"tw_device_env_{name}")
        fn.restype = C.c_void_p
        d = DeviceEnvDesc.from_address(fn())
        assert d.groups_per_cu and d.launch_search, name


def test_a_descriptor_without_it_is_refused():
    """A module from before the member is shorter by one pointer: the library refuses it by the layout tag, with the rebuild message;
    and a descriptor of today's size whose pointer is null is refused as lacking a function."""
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    L = _lib.lib()
    env = gridworld()
    vt = _lib.EnvVTable()
    old = DeviceEnvDesc.from_buffer_copy(env._desc)
    old.layout[2] -= C.sizeof(C.c_void_p)
    assert L.tw_device_env_host_vtable(C.addressof(old), env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
    assert "another library layout" in _lib.last_error() and "rebuild it" in _lib.last_error()
    null = DeviceEnvDesc.from_buffer_copy(env._desc)
    C.memset(C.addressof(null) + DeviceEnvDesc.groups_per_cu.offset, 0, C.sizeof(C.c_void_p))
    assert L.tw_device_env_host_vtable(C.addressof(null), env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
    assert "lacks a function" in _lib.last_error()


def test_resident_groups_option():
    from twisterl_amd import _lib
    L = _lib.lib()
    assert _lib.TW_OPT_ENV_RESIDENT_GROUPS == 6
    try:
        assert L.tw_set_launch_option(6, 1) == _lib.TW_OK
        assert L.tw_set_launch_option(6, 2) == _lib.TW_OK
        assert L.tw_set_launch_option(6, -1) == _lib.TW_ERR_INVALID
        assert "TW_OPT_ENV_RESIDENT_GROUPS" in _lib.last_error()
    finally:
        assert L.tw_set_launch_option(6, 0) == _lib.TW_OK                  # the default: automatic
    with _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, 3):
        pass
    assert L.tw_set_launch_option(7, 0) == _lib.TW_ERR_INVALID             # still no option 7
