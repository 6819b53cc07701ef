"""CPU: user-written device environments (include/twisterl_device_env.hpp) -- the modules build for gfx950 with the library's flags,
their kernels are hazard-free and scratch-free, the contract's violations fail to compile with its messages, the descriptor and the
host vtable are right, the C++ GridWorld's host side is the reference's GridWorld transition by transition, the big-board
Puzzle as a device-environment struct (BigPuzzleEnv) collects what the oracle's Puzzle collects, and without a GPU the collectors fail loudly."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.device_env_util import GRIDWORLD_FIELDS, HostEnv, big_puzzle, build_gridworld, build_ring, gridworld, ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


@pytest.mark.parametrize("build", [build_gridworld, build_ring])
def test_modules_build_and_scan_clean(build):
    so = build()
    asm = so[:-3] + ".s"
    assert os.path.exists(so) and os.path.exists(asm)
    hits, counts = _scan(asm)
    assert hits == [] and sum(counts.values()) > 0           # the EngineV layers are MFMAs; none with a hazard
    text = open(asm).read()
    assert "rollout_env_kernel" in text and "solve_env_kernel" in text
    assert "gfx950" in text


def test_descriptor_exports_and_layout():
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    L = _lib.lib()
    for so, name, A, NO, size in ((build_gridworld(), "gridworld5x5", 4, 25, 4 * 9), (build_ring(), "ring", 3, 2, 56)):
        out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert re.search(rf"\bT tw_device_env_{name}\b", out), out
        mod = C.CDLL(so)
        fn = getattr(mod, f"tw_device_env_{name}")
        fn.restype = C.c_void_p
        d = DeviceEnvDesc.from_address(fn())
        assert (d.num_actions, d.n_obs, d.state_bytes) == (A, NO, size)
        assert d.layout[0] == 0x45445754 and d.layout[1] == _lib.ABI_VERSION == 6 and d.layout[2] == C.sizeof(DeviceEnvDesc)
        assert d.layout[7] == C.sizeof(_lib.EnvVTable)
        # the library accepts its own layout ...
        env = gridworld() if name == "gridworld5x5" else ring()
        vt = _lib.EnvVTable()
        assert L.tw_device_env_host_vtable(*env._args(), C.byref(vt)) == 0
        assert (vt.num_actions, vt.n_obs, vt.obs_size) == (A, NO, 625 if A == 4 else 64) and vt.clone and not vt.track_solution
        # ... and refuses another one, with a message
        bad = DeviceEnvDesc.from_buffer_copy(d)
        bad.layout[4] += 8
        assert L.tw_device_env_host_vtable(C.addressof(bad), env._obj, d.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
        assert "another library layout" in _lib.last_error()
        assert L.tw_device_env_host_vtable(fn(), env._obj, d.state_bytes + 4, C.byref(vt)) == _lib.TW_ERR_INVALID


def test_gridworld_kernels_use_no_scratch():
    text = open(build_gridworld()[:-3] + ".s").read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == 2 and all(int(s) == 0 for s in sizes), sizes


def test_each_step_loop_exists_once():
    """The f32 and the f16 kernel of a pair include ONE body file inside their function bodies (no once-pragma: it is included twice);
    tw_rollout_env.hpp itself holds no step loop.  A loop forked again fails here."""
    csrc = os.path.join(ROOT, "twisterl_amd", "csrc")
    head = "while (__syncthreads_or("
    header = open(os.path.join(csrc, "tw_rollout_env.hpp")).read()
    assert header.count(head) == 0
    for body in ("tw_env_rollout_loop.hpp", "tw_env_solve_loop.hpp"):
        text = open(os.path.join(csrc, body)).read()
        assert text.count(head) == 1 and "#pragma once" not in text, body
        assert header.count(f'#include "{body}"') == 2, body


_VIOLATIONS = {
    "NUM_ACTIONS must be 1..4": ("NUM_ACTIONS = 5", "N_OBS = 2", ""),
    "N_OBS must be 1..64": ("NUM_ACTIONS = 2", "N_OBS = 65", ""),
    "must be trivially copyable": ("NUM_ACTIONS = 2", "N_OBS = 2", "Bad() {} Bad(const Bad &o) : x(o.x) {}"),
    "must be default-constructible": ("NUM_ACTIONS = 2", "N_OBS = 2", "explicit Bad(int v) : x(v) {}"),
}


@pytest.mark.parametrize("message", sorted(_VIOLATIONS))
def test_contract_violations_fail_to_compile(tmp_path, message):
    from twisterl_amd.build import build_device_env
    na, no, extra = _VIOLATIONS[message]
    hdr = tmp_path / "bad.hpp"
    hdr.write_text(f"""#pragma once
#include "twisterl_device_env.hpp"
struct Bad {{
    static constexpr int {na};
    static constexpr int {no};
    int x = 0;
    {extra}
    __host__ __device__ int obs_size() const {{ return 4; }}
    __host__ __device__ int difficulty() const {{ return 1; }}
    __host__ void set_difficulty(int) {{}}
    __host__ __device__ void reset(uint64_t, uint64_t) {{ x = 0; }}
    __host__ __device__ void step(int) {{ ++x; }}
    __host__ __device__ void observe(int *ids) const {{ for (int i = 0; i < N_OBS; ++i) ids[i] = 0; }}
    __host__ __device__ uint32_t masks() const {{ return 1u; }}
    __host__ __device__ float reward() const {{ return 0.0f; }}
    __host__ __device__ bool is_final() const {{ return x > 3; }}
    __host__ __device__ bool success() const {{ return false; }}
    __host__ bool init(const double *, int) {{ return true; }}
}};
""")
    with pytest.raises(RuntimeError) as ei:
        build_device_env(str(hdr), "Bad", "bad", out_dir=str(tmp_path))
    assert message in str(ei.value)
    assert not os.path.exists(tmp_path / "libtw_env_bad.so")


class _PyGrid:
    """tests/gridworld_env.py's GridWorld with a given state."""

    def __init__(self, w, h, st):
        from tests.gridworld_env import GridWorld
        self.g = GridWorld(w, h, st["max_steps"])
        self.g.agent, self.g.goal, self.g.trap = (st["ax"], st["ay"]), (st["gx"], st["gy"]), (st["tx"], st["ty"])
        self.g.steps_left = st["steps_left"]


def test_gridworld_host_side_matches_the_python_restatement():
    """step / masks / reward / is_final / observe of the C++ GridWorld (through the module's host vtable) against
    tests/gridworld_env.py -- the reference's examples/grid_world dynamics -- from the same set states."""
    w = h = 5
    env = gridworld(max_steps=64)
    rnd = random.Random(7)
    fmt = "<9i"
    for it in range(4000):
        pos = lambda: (rnd.randrange(w), rnd.randrange(h))
        (ax, ay), (gx, gy), (tx, ty) = pos(), pos(), pos()
        st = dict(max_steps=64, diff=1, ax=ax, ay=ay, gx=gx, gy=gy, tx=tx, ty=ty, steps_left=rnd.choice([0, 1, 2, rnd.randrange(65)]))
        env.set_state_bytes(struct.pack(fmt, *[st[k] for k in GRIDWORLD_FIELDS]))
        py = _PyGrid(w, h, st).g
        assert env.observe() == py.observe(), st
        assert env.masks() == py.masks(), st
        assert np.float32(env.reward()).tobytes() == np.float32(py.value()).tobytes(), st
        assert env.is_final() == py.is_final() and env.success() == py.success(), st
        a = rnd.randrange(4)
        env.step(a)
        py.next(a)
        got = dict(zip(GRIDWORLD_FIELDS, struct.unpack(fmt, env.state_bytes())))
        assert ((got["ax"], got["ay"]), got["steps_left"]) == (py.agent, py.steps_left), (st, a)
        assert env.observe() == py.observe() and env.masks() == py.masks() and env.is_final() == py.is_final()


def test_gridworld_reset_places_as_the_reference():
    """reset(): agent, goal and trap on three different cells, the goal within `difficulty` steps of the agent (lib.rs:118-129);
    the same (seed, episode) gives the same state, and every cell is reached."""
    for diff in (1, 2, 4):
        env = gridworld(difficulty=diff)
        assert env.difficulty == diff
        seen = set()
        for ep in range(400):
            env.reset(seed=11, episode=ep)
            s = dict(zip(GRIDWORLD_FIELDS, struct.unpack("<9i", env.state_bytes())))
            a, g, t = (s["ax"], s["ay"]), (s["gx"], s["gy"]), (s["tx"], s["ty"])
            assert len({a, g, t}) == 3 and abs(a[0] - g[0]) + abs(a[1] - g[1]) <= diff and s["steps_left"] == 64
            seen.add(a)
            b = env.state_bytes()
            env.reset(seed=11, episode=ep)
            assert env.state_bytes() == b
        assert len(seen) == 25
    env.difficulty = 99
    assert env.difficulty == 10                                            # min(width + height, d) (lib.rs: set_difficulty)


@pytest.mark.parametrize("w,h", [(5, 5), (6, 4)])
def test_big_puzzle_struct_collects_what_the_oracle_puzzle_collects(oracle, w, h):
    """BigPuzzleEnv<25> -- the functions rollout_big_kernel calls, as a device-environment struct -- built as a module: the oracle's any-environment
    collector over its host vtable against the oracle's own Puzzle collect, every field bit for bit.  6 x 4 runs in the same class
    of 25 with 24 ids per observation (the struct's n_obs())."""
    from tests.util import f32_bits, make_deep_policy_arrays, oracle_policy, puzzle_transpose_twist
    D, E, seed = 5, 40, 17
    env = big_puzzle(w, h, D, 2, 256)
    assert (env.n_obs, env.obs_size, env.num_actions(), env.difficulty) == (w * h, (w * h) ** 2, 4, D)
    twists = puzzle_transpose_twist(w) if w == h else ((), ())
    op = oracle_policy(oracle, make_deep_policy_arrays(w * h, seed=6, emb=32, common=(64, 32), scale=2.0), *twists)
    want = oracle.ppo_collect(oracle.Puzzle(w, h, D, 2, 256), op, E, 0.995, 0.995, seed=seed, arith=oracle.ARITH_CHAIN, det_log=True)
    got = oracle.ppo_collect_env(HostEnv(env), op, E, 0.995, 0.995, seed=seed, difficulty=D)
    assert got.obs.shape == want.obs.shape == (len(want.values), w * h) and len(want.values) > E
    for k in ("obs", "actions", "perms", "ep_len"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    for k in ("logits", "values", "rewards"):
        assert np.array_equal(f32_bits(getattr(got, k)), f32_bits(getattr(want, k))), k
    for k in ("advs", "rets"):
        assert np.array_equal(f32_bits(got.additional_data[k]), f32_bits(want.additional_data[k])), k
    if w == h:
        assert set(np.unique(want.perms).tolist()) == {0, 1}


def test_device_env_python_surface():
    env = ring(n=32, difficulty=3)
    assert env.num_actions() == 3 and env.obs_shape() == [2, 32] and env.difficulty == 3 and env.twists() == ([], [])
    env.reset(seed=5, episode=9)
    o = env.observe()
    assert 0 <= o[0] < 32 and 32 <= o[1] < 64 and env.masks() == [True, True, True]
    env.step(2)
    assert env.masks() == [True, False, True]                              # "stay" on even steps only
    with pytest.raises(ValueError):
        env.step(3)
    with pytest.raises(ValueError, match="refused"):
        ring(n=2)
    assert env.__extract_env__() != 0


def test_no_gpu_means_loud_failure_for_device_environments():
    """Without a device the collect and evaluate of a DeviceEnv raise, never fall back.  (The first thing that needs the device is
    the policy upload, as for every collector: test_abi.py's convention.)"""
    import twisterl_amd
    from twisterl_amd import twisterl
    from tests.util import amd_policy, make_deep_policy_arrays
    if twisterl_amd.device_count() > 0:
        pytest.skip("GPU present")
    pol = amd_policy(make_deep_policy_arrays(25, emb=32, common=(32,)))
    env = gridworld()
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        twisterl.collector.PPOCollector(4, 0.9, 0.9, 1).collect(env, pol)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):
        twisterl.collector.evaluate(env, pol, 4, True, 1, 0, 1, 1.41, 1, 1)
