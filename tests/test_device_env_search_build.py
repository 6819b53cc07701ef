"""CPU: device-environment modules built WITH the search kernel (build_device_env(search=True), TW_DEVICE_ENV_SEARCH): GridWorld, RingWalk,
the 12-lamp Lamps and BigPuzzleEnv<25> compile to three kernels -- mcts_env_kernel among them -- without scratch memory and without an
MFMA hazard; the default form still has two; a struct above the size bound fails to compile with its message; the descriptor says
which form a module is; and without a GPU the new entry point fails loudly."""
import ctypes as C
import os
import re

import pytest

from tests.device_env_search_util import SEARCH_MODULES, gridworld_az, ring_az
from tests.device_env_util import build_gridworld, gridworld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


def _kernels(asm_text):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, flags=re.M)


@pytest.mark.parametrize("name", sorted(SEARCH_MODULES))
def test_search_modules_have_three_clean_kernels(name):
    so = SEARCH_MODULES[name]()
    asm = so[:-3] + ".s"
    assert os.path.exists(so) and os.path.exists(asm)
    text = open(asm).read()
    kernels = _kernels(text)
    assert len(kernels) == 3 and sum("mcts_env_kernel" in k for k in kernels) == 1, kernels
    assert sum("rollout_env_kernel" in k for k in kernels) == 1 and sum("solve_env_kernel" in k for k in kernels) == 1, kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == 3 and all(int(s) == 0 for s in sizes), sizes
    hits, counts = _scan(asm)
    assert hits == [] and sum(counts.values()) > 0
    assert "gfx950" in text and f"TW_DEVICE_ENV_SEARCH(" in open(so[:-3] + ".hip").read()


def test_default_module_still_has_two_kernels():
    text = open(build_gridworld()[:-3] + ".s").read()
    kernels = _kernels(text)
    assert len(kernels) == 2 and not any("mcts_env_kernel" in k for k in kernels), kernels


_BIG = """#pragma once
#include "twisterl_device_env.hpp"
struct Wide {{
    static constexpr int NUM_ACTIONS = 2;
    static constexpr int N_OBS = 2;
    int x = 0;
    int filler[{words}] = {{}};
    __host__ __device__ int obs_size() const {{ return 4; }}
    __host__ __device__ int difficulty() const {{ return 1; }}
    __host__ void set_difficulty(int) {{}}
    __host__ __device__ void reset(uint64_t, uint64_t) {{ x = 0; }}
    __host__ __device__ void step(int) {{ ++x; }}
    __host__ __device__ void observe(int *ids) const {{ ids[0] = 0; ids[1] = 1; }}
    __host__ __device__ uint32_t masks() const {{ return 3u; }}
    __host__ __device__ float reward() const {{ return 0.0f; }}
    __host__ __device__ bool is_final() const {{ return x > 3; }}
    __host__ __device__ bool success() const {{ return false; }}
    __host__ bool init(const double *, int) {{ return true; }}
}};
"""


def test_struct_above_the_size_bound_fails_to_compile(tmp_path):
    """TW_DEVICE_ENV_SEARCH: at most 128 bytes (two copies live in a lane's registers).  132 bytes fail with the message and leave no
    module; the same struct builds in the default form, and 128 bytes build in the search form."""
    from twisterl_amd.build import build_device_env
    hdr = tmp_path / "wide.hpp"
    hdr.write_text(_BIG.format(words=32))                                   # 4 + 128 bytes
    with pytest.raises(RuntimeError) as ei:
        build_device_env(str(hdr), "Wide", "wide", out_dir=str(tmp_path), search=True)
    assert "TW_DEVICE_ENV_SEARCH needs a struct of at most 128 bytes" in str(ei.value)
    assert not os.path.exists(tmp_path / "libtw_env_wide.so")
    assert os.path.exists(build_device_env(str(hdr), "Wide", "wide_plain", out_dir=str(tmp_path)))
    fits = tmp_path / "fits.hpp"
    fits.write_text(_BIG.format(words=31))                                  # 128 bytes
    so = build_device_env(str(fits), "Wide", "fits", out_dir=str(tmp_path), search=True)
    assert len(_kernels(open(so[:-3] + ".s").read())) == 3


def test_descriptor_says_which_form_a_module_is():
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    L = _lib.lib()
    plain, az = gridworld(), gridworld_az()
    assert plain.search is False and az.search is True and ring_az().search is True
    assert not plain._desc.launch_search and az._desc.launch_search
    for env in (plain, az):
        d = env._desc
        assert d.layout[0] == 0x45445754 and d.layout[1] == _lib.ABI_VERSION and d.layout[2] == C.sizeof(DeviceEnvDesc)
        assert d.layout[7] == C.sizeof(_lib.EnvVTable) and len(d.layout) == 8
    # the host side of the two forms is the same struct
    plain.reset(seed=3, episode=5); az.reset(seed=3, episode=5)
    assert plain.state_bytes() == az.state_bytes() and plain.observe() == az.observe()
    # a module that was built against a descriptor of another size is refused
    vt = _lib.EnvVTable()
    bad = DeviceEnvDesc.from_buffer_copy(az._desc)
    bad.layout[2] -= 8
    assert L.tw_device_env_host_vtable(C.addressof(bad), az._obj, az._desc.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
    assert "another library layout" in _lib.last_error()
    out = C.c_void_p()
    prm = _lib.AZParams(4, 0, 4, 1.41, 1, 1, _lib.TW_PREC_F32_EXACT, 1, 0)
    assert L.tw_az_collect_device_env(C.addressof(bad), az._obj, az._desc.state_bytes, None, C.byref(prm), 13, C.byref(out)) == _lib.TW_ERR_INVALID
    assert not out.value


def test_no_gpu_means_loud_failure_for_device_self_play():
    """Without a device self-play and MCTS-guided evaluate of a search module raise, never fall back.  (The first thing that needs the
    device is the policy upload, as for every collector: test_abi.py's convention.)"""
    import twisterl_amd
    from twisterl_amd import twisterl
    from tests.util import amd_policy, make_deep_policy_arrays
    if twisterl_amd.device_count() > 0:
        pytest.skip("GPU present")
    pol = amd_policy(make_deep_policy_arrays(25, emb=32, common=(32, 32)))
    env = gridworld_az()
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        twisterl.collector.AZCollector(4, 4, 1.41, 1, 1).collect(env, pol)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        twisterl.collector.evaluate(env, pol, 4, True, 1, 4, 1, 1.41, 1, 1)
