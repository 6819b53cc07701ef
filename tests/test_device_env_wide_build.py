"""CPU: device environments of 5 .. 31 actions (tests/device_env_wide.py).  Every row's module builds for gfx950 with the opt-in and
passes the MFMA hazard scan of the module build; each holds exactly TWO kernels (the wide step is the same rollout_env_kernel /
solve_env_kernel, no third one); the default build still refuses five actions with the 1..4 message, which now names the opt-in, and
TW_DEVICE_ENV_SEARCH refuses them with its own; a struct of three actions compiles to the same kernel instruction text with and
without the opt-in, and the two builds never share a cache entry; the kernels' scratch use is recorded; and the oracle's collect of
every row contains what tests/test_gpu_device_env_wide.py is about, so that test cannot pass for lack of cases."""
import os
import re

import numpy as np
import pytest

from tests.device_env_wide import (BY_MODULE, E, IDS, OPT_IN_WITHOUT_USE, PERM8, WIDE_HPP, build_all, engine_nc, make_env, shared_collect)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rollout_env_kernel", "solve_env_kernel")
# .private_segment_fixed_size of (rollout_env_kernel, solve_env_kernel).  Every row's struct is small (40 bytes at most) and every
# row up to EngineV<25> must stay in registers.  EngineV<64> with 31 actions: 48 bytes in both kernels, recorded as compiled.  That is
# the 40-byte STATE, not a register spill: with 64 unrolled id hashes and their bounds checks around it the kernel has more basic blocks
# than the compiler's inliner accepts, so masks() and is_final() of the struct stay calls and the struct they read lives in memory.  The
# same struct with FOUR actions (Probe<64, 4, 1, false>) compiles to the same 48 bytes: the streaming step adds nothing to it.
SCRATCH = {"wideo2a5": (0, 0), "wideo5a8v": (0, 0), "wideo16a16": (0, 0), "wideo17a17": (0, 0), "wideo64a31": (48, 48), "perm8": (0, 0),
           "wideo4a3": (0, 0)}

_FIVE = """#pragma once
#include "twisterl_device_env.hpp"
struct Five {
    static constexpr int NUM_ACTIONS = 5;
    static constexpr int N_OBS = 2;
    int x = 0;
    __host__ __device__ int obs_size() const { return 4; }
    __host__ __device__ int difficulty() const { return 1; }
    __host__ void set_difficulty(int) {}
    __host__ __device__ void reset(uint64_t, uint64_t) { x = 0; }
    __host__ __device__ void step(int a) { x += 1 + a; }
    __host__ __device__ void observe(int *ids) const { for (int i = 0; i < N_OBS; ++i) ids[i] = (x + i) & 3; }
    __host__ __device__ uint32_t masks() const { return 31u; }
    __host__ __device__ float reward() const { return 0.0f; }
    __host__ __device__ bool is_final() const { return x > 9; }
    __host__ __device__ bool success() const { return false; }
    __host__ bool init(const double *, int) { return true; }
};
"""


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


def _asm(module):
    so = build_all()[module]
    assert os.path.exists(so) and os.path.exists(so[:-3] + ".s")
    return so[:-3] + ".s", open(so[:-3] + ".s").read()


def _kernel_text(text):
    """{kernel: its instruction text} of a module's assembly: the lines between a kernel's label and its .amdhsa_kernel block, without
    comments, directives and blank lines -- the symbol names (which carry the struct's name) are replaced by the kernel's."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    out = {}
    for n in names:
        body = text.split(f"\n{n}:", 1)[1].split(".amdhsa_kernel", 1)[0]
        lines = []
        for ln in body.splitlines():
            ln = ln.split(";", 1)[0].strip()
            if ln and not ln.startswith("."):
                lines.append(ln)
        out[next(k for k in KERNELS if k in n)] = "\n".join(lines).replace(n, "KERNEL")
    return out


@pytest.mark.parametrize("module", IDS)
def test_module_builds_clean_with_exactly_two_kernels(module):
    r = BY_MODULE[module]
    path, text = _asm(module)
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 2, kernels
    nc = engine_nc(r.n_obs)
    for k in KERNELS:                                     # kernel<Env, NC>: the mangled name ends in the column count
        assert sum(1 for n in kernels if re.search(rf"{k}I.*Li{nc}EEEvNS_", n)) == 1, (k, nc, kernels)
    hits, counts = _scan(path)
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(path[:-2] + ".hip").read()
    assert "#define TW_DEVICE_ENV_WIDE\n#include" in src and f"TW_DEVICE_ENV({r.type}, {r.module})" in src
    env = make_env(r)
    d = env._desc
    assert (int(d.num_actions), int(d.n_obs), int(d.engine_nc)) == (r.A, r.n_obs, nc)
    assert env.num_actions() == r.A and env.search is False and env.variable_obs is r.var and env.obs_size == r.obs_size
    m = env.masks()
    assert len(m) == r.A


@pytest.mark.parametrize("module", IDS)
def test_scratch_use_is_as_recorded(module):
    text = _asm(module)[1]
    sizes = {}
    for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text):
        sizes[next(k for k in KERNELS if k in name)] = int(size)
    assert tuple(sizes[k] for k in KERNELS) == SCRATCH[module], sizes
    if engine_nc(BY_MODULE[module].n_obs) <= 25:
        assert SCRATCH[module] == (0, 0)


def _build_five(tmp_path, **kw):
    from twisterl_amd.build import build_device_env
    hdr = tmp_path / "five.hpp"
    hdr.write_text(_FIVE)
    return build_device_env(str(hdr), "Five", "five", out_dir=str(tmp_path), **kw)


def test_five_actions_need_the_opt_in_and_the_message_names_it(tmp_path):
    with pytest.raises(RuntimeError) as ei:
        _build_five(tmp_path)
    msg = str(ei.value)
    assert "NUM_ACTIONS must be 1..4" in msg and "5..31: define TW_DEVICE_ENV_WIDE / build_device_env(wide=True)" in msg
    assert not os.path.exists(tmp_path / "libtw_env_five.so")
    so = _build_five(tmp_path, wide=True)                 # the same header and name with the opt-in: builds
    assert os.path.exists(so)


def test_the_search_form_refuses_five_actions_with_its_own_message(tmp_path):
    with pytest.raises(RuntimeError) as ei:
        _build_five(tmp_path, wide=True, search=True)
    assert "TW_DEVICE_ENV_SEARCH needs NUM_ACTIONS 1..4 (the search kernel keeps four children per node)" in str(ei.value)
    assert not os.path.exists(tmp_path / "libtw_env_five.so")


def test_three_actions_compile_alike_with_and_without_the_opt_in(tmp_path):
    """The same struct, the same module name, two out_dirs: identical kernel instruction text.  Then the cache: a second build of the
    OTHER form in a directory that holds one form rebuilds (the generated source differs), and the form asked for is what is there."""
    from twisterl_amd.build import build_device_env
    r = BY_MODULE[OPT_IN_WITHOUT_USE]
    a, b = tmp_path / "narrow", tmp_path / "wide"
    so_n = build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a))
    so_w = build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(b), wide=True)
    tn, tw_ = _kernel_text(open(so_n[:-3] + ".s").read()), _kernel_text(open(so_w[:-3] + ".s").read())
    assert sorted(tn) == sorted(tw_) == sorted(KERNELS)
    for k in KERNELS:
        assert len(tn[k].splitlines()) > 500 and tn[k] == tw_[k], k
    assert tn == _kernel_text(_asm(OPT_IN_WITHOUT_USE)[1])
    src = so_n[:-3] + ".hip"
    assert "TW_DEVICE_ENV_WIDE" not in open(src).read()
    before = os.stat(so_n).st_mtime_ns
    assert build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a)) == so_n and os.stat(so_n).st_mtime_ns == before      # cached
    assert build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a), wide=True) == so_n
    assert "#define TW_DEVICE_ENV_WIDE" in open(src).read() and os.stat(so_n).st_mtime_ns != before                           # rebuilt


def _allowed(o):
    return (o.logits > np.float32(-1e9)).sum(axis=1)


@pytest.mark.parametrize("module", IDS)
def test_the_shared_collect_contains_what_the_gpu_test_is_about(module):
    """The input conditions, on the oracle's data (the struct's own host code under the oracle's PPO loop) at the GPU test's seeds."""
    r = BY_MODULE[module]
    o = shared_collect(module)
    lens = o.ep_len.tolist()
    assert len(lens) == E and int(o.ep_len.sum()) == o.obs.shape[0] and o.obs.shape[1] == r.n_obs and o.logits.shape[1] == r.A
    assert max(lens) <= r.max_records and len(set(lens)) >= 3, sorted(set(lens))
    assert set(o.actions.tolist()) == set(range(r.A)), ("an action is never taken", sorted(set(range(r.A)) - set(o.actions.tolist())))
    n_allowed = _allowed(o)
    assert int(n_allowed.min()) >= 1
    if module == PERM8:
        # the example's mask forbids ONE action (undoing the last move) and nothing else: no state of it has a single allowed action.
        # What its collect must hold instead: first records (everything allowed) and later ones (one action forbidden), solved episodes
        assert set(n_allowed.tolist()) == {r.A - 1, r.A} and 1.0 in o.rewards.tolist() and r.max_records in lens
    else:
        assert (n_allowed == 1).any(), "no record with exactly one allowed action"
        assert (o.logits[:, r.A - 1] > np.float32(-1e9)).any(), "the last mask bit is never set"
    if r.A > 4:
        start = np.concatenate([[0], np.cumsum(o.ep_len[[E - 1] + list(range(E - 1))].astype(np.int64))])           # (merge order: the last episode first)
        high = sum(1 for i in range(E) if (o.actions[start[i]:start[i + 1]] >= 4).any())
        assert 2 * high >= E, f"a chosen action >= 4 in {high} of {E} episodes"
    if r.twists:
        assert set(o.perms.tolist()) == set(range(r.twists))
    else:
        assert set(o.perms.tolist()) == {-1}
    if r.var:
        assert int(o.counts.min()) == 0 and int(o.counts.max()) == r.n_obs
