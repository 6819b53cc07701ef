"""CPU: environments whose observations vary in length (tw_env_vtable.observe_n; a device struct's observe_n()).  The two lamps modules
(tests/device_envs/lamps.hpp, N_OBS 12 and 40) build for gfx950, hazard-free and scratch-free, and their host vtables carry observe_n
while GridWorld's does not; the collect every GPU test of tests/test_gpu_var_obs.py compares against contains what those tests are
about (an empty observation, a full one, counts that change inside an episode, several episode lengths) -- checked on the ORACLE's
data; PyEnv takes max_obs() and keeps refusing a changing length without it; a struct with neither observe nor observe_n fails to
compile with the contract's message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.device_env_util import build_gridworld, gridworld
from tests.var_obs_util import E, MAX_RECORDS, NO_ID, SIZES, PyLamps, build_lamps, lamps, shared_collect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


@pytest.mark.parametrize("n", SIZES)
def test_lamps_modules_build_clean_two_kernels_no_scratch(n):
    so = build_lamps(n)
    asm = so[:-3] + ".s"
    assert os.path.exists(so) and os.path.exists(asm)
    hits, counts = _scan(asm)
    assert hits == [] and sum(counts.values()) > 0
    text = open(asm).read()
    assert "gfx950" in text
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 2 and any("rollout_env_kernel" in k for k in kernels) and any("solve_env_kernel" in k for k in kernels), kernels
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == 2 and all(int(s) == 0 for s in sizes), sizes
    assert all(f"5LampsILi{n}EELi{16 if n == 12 else 64}E" in k for k in kernels), kernels      # EngineV<16> for 12 ids, EngineV<64> for 40


@pytest.mark.parametrize("n", SIZES)
def test_lamps_vtable_has_observe_n_and_gridworld_has_not(n):
    from twisterl_amd import _lib
    env = lamps(n)
    vt = _lib.EnvVTable()
    assert _lib.lib().tw_device_env_host_vtable(*env._args(), C.byref(vt)) == 0
    assert vt.observe_n and vt.observe and (vt.num_actions, vt.n_obs, vt.obs_size) == (4, n, n * n)
    gvt = _lib.EnvVTable()
    assert _lib.lib().tw_device_env_host_vtable(*gridworld()._args(), C.byref(gvt)) == 0
    assert not gvt.observe_n and gvt.observe and gvt.n_obs == 25
    assert C.sizeof(_lib.EnvVTable) == 8 + 16 + 14 * 8 and _lib.ABI_VERSION == 6     # one trailing pointer; the version stays


@pytest.mark.parametrize("n", SIZES)
def test_lamps_python_surface_returns_the_ids_a_state_has(n):
    env = lamps(n)
    assert env.variable_obs and env.n_obs == n and env.obs_shape() == [n * n] and env.num_actions() == 4
    assert not gridworld().variable_obs and gridworld().obs_shape() == [25, 25]
    seen = set()
    for ep in range(200):
        env.reset(seed=3, episode=ep)
        for t in range(6):
            ids = env.observe()
            lit = [i // n for i in ids]
            assert lit == sorted(set(lit)) and all(i % n == t % n for i in ids) and len(ids) <= n, (ep, t, ids)
            assert (len(ids) == 0) == env.success() and (env.is_final() or not env.success())
            seen.add(len(ids))
            # the fixed-length member of the same vtable: the ids, then -1
            out = (C.c_int32 * n)()
            env._vt.observe(env._obj, out)
            assert list(out) == ids + [-1] * (n - len(ids))
            if env.is_final():
                break
            env.step((ep + t) % 4 if not (t & 1 and (ep + t) % 4 == 2) else 0)
    assert 0 in seen and n in seen and len(seen) >= 4, seen
    # the deliberately invalid variants: a count of N_OBS + 1, an id outside [0, obs_size)
    bad = lamps(n, bad_at=0, bad_kind=2)
    bad.reset(seed=3, episode=1)
    with pytest.raises(ValueError, match=f"observation of {n + 1} ids, at most {n}"):
        bad.observe()
    bad.reset(seed=3, episode=3)                                           # every third episode: two steps later
    assert len(bad.observe()) <= n
    bad = lamps(n, bad_at=0, bad_kind=1)
    bad.reset(seed=3, episode=2)
    assert not bad.success() and bad.observe()[0] == n * n + 2
    bad.reset(seed=3, episode=1)
    assert not bad.success() and bad.observe()[0] == -2


@pytest.mark.parametrize("n", SIZES)
def test_the_shared_collect_contains_what_the_gpu_tests_are_about(n):
    """The input condition, on the oracle's data: 150 episodes of at most 24 records hold a record of no ids, one of exactly N_OBS ids,
    an episode whose consecutive records differ in count, and at least three episode lengths."""
    o = shared_collect(n)
    assert len(o.ep_len) == E and int(o.ep_len.max()) <= MAX_RECORDS and int(o.ep_len.sum()) == len(o.obs_lists) == o.obs.shape[0]
    assert o.obs.dtype == np.uint16 and o.obs.shape[1] == n
    assert np.array_equal((o.obs != NO_ID).sum(axis=1), o.counts)
    assert int(o.counts.min()) == 0, "no empty observation in the shared collect"
    assert int(o.counts.max()) == n, "no observation of exactly N_OBS ids in the shared collect"
    assert any(len({len(r) for r in ep}) > 1 for ep in o.episodes), "no episode whose records differ in count"
    assert any(any(len(a) != len(b) for a, b in zip(ep, ep[1:])) for ep in o.episodes)
    assert len(set(o.ep_len.tolist())) >= 3, sorted(set(o.ep_len.tolist()))
    assert all(0 <= i < n * n for r in o.obs_lists for i in r)


def test_pyenv_takes_max_obs_and_refuses_a_changing_length_without_it():
    from twisterl_amd import twisterl
    from twisterl_amd.collector import _PyEnvBridge
    # with max_obs(): n_obs is the maximum, observe_n is filled and returns the ids a state has
    var = PyLamps()
    br = _PyEnvBridge(twisterl.env.PyEnv(var))
    assert br.vt.observe_n and (br.vt.n_obs, br.vt.obs_size, br.vt.num_actions) == (6, 36, 4)
    var.mask = 0b101001
    buf = (C.c_int32 * 6)()
    assert br.vt.observe_n(1, buf, 6) == 3 and list(buf[:3]) == var.observe() and not br.err
    var.mask = 0
    assert br.vt.observe_n(1, buf, 6) == 0 and not br.err                 # an empty observation is legal
    var.mask = 0b111
    assert br.vt.observe_n(1, buf, 2) == 0 and len(br.err) == 1           # a longer one than the C side has room for raises
    with pytest.raises(ValueError, match=r"observe\(\) returned 3 ids, max_obs\(\) is 2"):
        br.finish(0)
    # without it: exactly as before -- the prototype's length is THE length, observe_n stays NULL, another length raises
    fixed = PyLamps(declare_max=False)
    fixed.mask = 0b11
    br = _PyEnvBridge(twisterl.env.PyEnv(fixed))
    assert not br.vt.observe_n and br.vt.n_obs == 2
    br.vt.observe(1, buf)
    assert not br.err and list(buf[:2]) == fixed.observe()
    fixed.mask = 0b111
    br.vt.observe(1, buf)
    with pytest.raises(ValueError, match="needs a fixed number of obs ids per state"):
        br.finish(0)


def test_a_struct_with_neither_observe_nor_observe_n_fails_to_compile(tmp_path):
    from twisterl_amd.build import build_device_env
    hdr = tmp_path / "blind.hpp"
    hdr.write_text("""#pragma once
#include "twisterl_device_env.hpp"
struct Blind {
    static constexpr int NUM_ACTIONS = 2;
    static constexpr int N_OBS = 2;
    int x = 0;
    __host__ __device__ int obs_size() const { return 4; }
    __host__ __device__ int difficulty() const { return 1; }
    __host__ void set_difficulty(int) {}
    __host__ __device__ void reset(uint64_t, uint64_t) { x = 0; }
    __host__ __device__ void step(int) { ++x; }
    __host__ __device__ uint32_t masks() const { return 1u; }
    __host__ __device__ float reward() const { return 0.0f; }
    __host__ __device__ bool is_final() const { return x > 3; }
    __host__ __device__ bool success() const { return false; }
    __host__ bool init(const double *, int) { return true; }
};
""")
    with pytest.raises(RuntimeError) as ei:
        build_device_env(str(hdr), "Blind", "blind", out_dir=str(tmp_path))
    assert "the struct needs `void observe(int *ids) const`, or `int observe_n(int *ids) const`" in str(ei.value)
    assert not os.path.exists(tmp_path / "libtw_env_blind.so")


def test_gridworld_module_still_has_its_two_scratch_free_kernels():
    text = open(build_gridworld()[:-3] + ".s").read()
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s+\S+", text, flags=re.M)) == 2
    assert [int(s) for s in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)] == [0, 0]
