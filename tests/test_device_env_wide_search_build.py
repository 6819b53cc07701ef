"""CPU: device environments of 5 .. 31 actions WITH the search kernel (tests/device_env_wide_search.py; TW_DEVICE_ENV_WIDE_SEARCH,
build_device_env(wide_search=True)).  Every row's module builds for gfx950, passes the MFMA hazard scan and holds exactly THREE kernels
(the wide search is the same mcts_env_kernel, no fourth one) and says `search`; a struct of three actions compiles to the same
instruction text in all three kernels as its TW_DEVICE_ENV_SEARCH build, and the two forms never share a cache entry; 129 bytes are
refused with the 128-byte message; the kernels' scratch use is recorded; and the oracle's self-play of every row contains what
tests/test_gpu_device_env_wide_search.py is about, so that test cannot pass for lack of cases.  (That wide=True with search=True
still refuses five actions is tests/test_device_env_wide_build.py's.)"""
import os
import re

import numpy as np
import pytest

from tests.device_env_wide_search import (ALL_OPEN, BY_MODULE, IDS, OPT_IN_WITHOUT_USE, PERM8, WIDE_HPP, build_all, engine_nc, make_env,
                                          shared_self_play)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rollout_env_kernel", "solve_env_kernel", "mcts_env_kernel")
# .private_segment_fixed_size of (rollout_env_kernel, solve_env_kernel, mcts_env_kernel).  Every row up to EngineV<25> stays in
# registers in all three kernels: the probabilities, the priors and the visit counts of the wide search stream through LDS and the
# nodes, never through an indexed register array.  EngineV<64> with 31 actions, recorded as compiled and explained from the assembly in
# in a module of three kernels the struct's observe(), masks() and is_final() stay CALLS in the rollout and solve kernels
# (one call site more than the inliner accepts at this size), so the 64 ids travel through a 256-byte array in memory next to the
# 40-byte state: 320 bytes where the two-kernel module has 48.  The search kernel inlines everything and sits at the 512-register limit
# of one wave per SIMD: 892 bytes are spilled registers of EngineV<64> under two copies of the state and 64 ids -- not the
# probabilities, the priors or the visit counts, which are in LDS.  The same struct with FOUR actions under TW_DEVICE_ENV_SEARCH compiles
# to 320 / 320 / 920: the wide branches add nothing to it.
SCRATCH = {"wideo2a5_ws": (0, 0, 0), "wideo5a8v_ws": (0, 0, 0), "wideo16a16_ws": (0, 0, 0), "wideo17a17_ws": (0, 0, 0),
           "wideo64a31_ws": (320, 320, 892), "perm8_ws": (0, 0, 0), "wideo4a3_ws": (0, 0, 0), "wideopena31_ws": (0, 0, 0)}

_BYTES = """#pragma once
#include "twisterl_device_env.hpp"
struct Bytes {{
    static constexpr int NUM_ACTIONS = 5;
    static constexpr int N_OBS = 2;
    unsigned char x = 0;
    unsigned char filler[{filler}] = {{}};
    __host__ __device__ int obs_size() const {{ return 4; }}
    __host__ __device__ int difficulty() const {{ return 1; }}
    __host__ void set_difficulty(int) {{}}
    __host__ __device__ void reset(uint64_t, uint64_t) {{ x = 0; }}
    __host__ __device__ void step(int a) {{ x = (unsigned char)(x + 1 + a); }}
    __host__ __device__ void observe(int *ids) const {{ ids[0] = x & 3; ids[1] = (x + 1) & 3; }}
    __host__ __device__ uint32_t masks() const {{ return 31u; }}
    __host__ __device__ float reward() const {{ return 0.0f; }}
    __host__ __device__ bool is_final() const {{ return x > 9; }}
    __host__ __device__ bool success() const {{ return false; }}
    __host__ bool init(const double *, int) {{ return true; }}
}};
static_assert(sizeof(Bytes) == {filler} + 1, "Bytes: one byte of state and the filler");
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
def test_module_builds_clean_with_exactly_three_kernels(module):
    r = BY_MODULE[module]
    path, text = _asm(module)
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert len(kernels) == 3, kernels
    nc = engine_nc(r.n_obs)
    for k in KERNELS:                                     # kernel<Env, NC>: the mangled name ends in the column count
        assert sum(1 for n in kernels if re.search(rf"{k}I.*Li{nc}EEEvNS_", n)) == 1, (k, nc, kernels)
    hits, counts = _scan(path)
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(path[:-2] + ".hip").read()
    assert "#define TW_DEVICE_ENV_WIDE\n#include" in src and f"TW_DEVICE_ENV_WIDE_SEARCH({r.type}, {r.module})" in src
    env = make_env(r)
    d = env._desc
    assert (int(d.num_actions), int(d.n_obs), int(d.engine_nc)) == (r.A, r.n_obs, nc)
    assert env.num_actions() == r.A and env.search is True and bool(d.launch_search) and env.variable_obs is r.var and env.obs_size == r.obs_size
    assert len(env.masks()) == r.A


@pytest.mark.parametrize("module", IDS)
def test_scratch_use_is_as_recorded(module):
    text = _asm(module)[1]
    sizes = {}
    for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text):
        sizes[next(k for k in KERNELS if k in name)] = int(size)
    assert tuple(sizes[k] for k in KERNELS) == SCRATCH[module], sizes
    if engine_nc(BY_MODULE[module].n_obs) <= 25:
        assert SCRATCH[module] == (0, 0, 0)


def test_three_actions_compile_as_the_search_form_does(tmp_path):
    """The same struct, the same module name, two out_dirs: TW_DEVICE_ENV_SEARCH and TW_DEVICE_ENV_WIDE_SEARCH give identical instruction
    text in all three kernels.  Then the cache: a second build of the OTHER form in a directory that holds one form rebuilds (the
    generated source differs), and the form asked for is what is there."""
    from twisterl_amd.build import build_device_env
    r = BY_MODULE[OPT_IN_WITHOUT_USE]
    a, b = tmp_path / "search", tmp_path / "wide_search"
    so_s = build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a), search=True)
    so_w = build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(b), wide_search=True)
    ts, tw_ = _kernel_text(open(so_s[:-3] + ".s").read()), _kernel_text(open(so_w[:-3] + ".s").read())
    assert sorted(ts) == sorted(tw_) == sorted(KERNELS)
    for k in KERNELS:
        assert len(ts[k].splitlines()) > 500 and ts[k] == tw_[k], k
    assert ts == _kernel_text(_asm(OPT_IN_WITHOUT_USE)[1])
    src = so_s[:-3] + ".hip"
    assert "TW_DEVICE_ENV_WIDE" not in open(src).read() and f"TW_DEVICE_ENV_SEARCH({r.type}, {r.module})" in open(src).read()
    before = os.stat(so_s).st_mtime_ns
    assert build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a), search=True) == so_s and os.stat(so_s).st_mtime_ns == before     # cached
    assert build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a), wide_search=True) == so_s
    text = open(src).read()
    assert "#define TW_DEVICE_ENV_WIDE\n" in text and "TW_DEVICE_ENV_WIDE_SEARCH(" in text and os.stat(so_s).st_mtime_ns != before      # rebuilt
    with pytest.raises(ValueError, match="wide_search=True is a form of its own"):
        build_device_env(WIDE_HPP, r.type, r.module, out_dir=str(a), search=True, wide_search=True)


def test_the_wide_search_form_keeps_the_128_byte_bound(tmp_path):
    """129 bytes with five actions: refused with the 128-byte message, no module left; 128 bytes build, with three kernels."""
    from twisterl_amd.build import build_device_env
    hdr = tmp_path / "bytes129.hpp"
    hdr.write_text(_BYTES.format(filler=128))
    with pytest.raises(RuntimeError) as ei:
        build_device_env(str(hdr), "Bytes", "bytes129", out_dir=str(tmp_path), wide_search=True)
    assert "TW_DEVICE_ENV_WIDE_SEARCH needs a struct of at most 128 bytes" in str(ei.value)
    assert not os.path.exists(tmp_path / "libtw_env_bytes129.so")
    fits = tmp_path / "bytes128.hpp"
    fits.write_text(_BYTES.format(filler=127))
    so = build_device_env(str(fits), "Bytes", "bytes128", out_dir=str(tmp_path), wide_search=True)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(so[:-3] + ".s").read(), flags=re.M)) == 3


def test_the_macro_without_the_define_says_what_is_missing(tmp_path):
    hdr = tmp_path / "bytes8.hpp"
    hdr.write_text(_BYTES.format(filler=7).replace("NUM_ACTIONS = 5", "NUM_ACTIONS = 3"))
    src = tmp_path / "no_define.hip"
    src.write_text(f'#include "{hdr}"\nTW_DEVICE_ENV_WIDE_SEARCH(Bytes, bytes8)\n')
    import subprocess
    from twisterl_amd.build import CSRC, FLAGS, hipcc
    r = subprocess.run([hipcc(), *FLAGS, "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path))
    assert r.returncode != 0 and "TW_DEVICE_ENV_WIDE_SEARCH needs `#define TW_DEVICE_ENV_WIDE`" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("module", IDS)
def test_the_shared_self_play_contains_what_the_gpu_test_is_about(module):
    """The input conditions, on the oracle's data (the struct's own host code under the oracle's self-play) at the GPU test's seeds."""
    r = BY_MODULE[module]
    o = shared_self_play(module)
    lens = o.ep_len.tolist()
    assert len(lens) == r.o_E >= 17 and int(o.ep_len.sum()) == o.obs.shape[0] == o.logits.shape[0] and o.obs.shape[1] == r.n_obs
    assert o.logits.shape[1] == r.A
    assert max(lens) <= r.max_records and len(set(lens)) >= 3, sorted(set(lens))
    assert (o.logits[:, r.A - 1] != 0).any(), "no record with a nonzero probability at the last index"
    if r.A > 4:
        high = sum(1 for acts in o.actions if any(a >= 4 for a in acts))
        assert 2 * high >= r.o_E, f"a taken action >= 4 in {high} of {r.o_E} episodes"
    if module in (ALL_OPEN, PERM8):
        assert ((o.logits != 0).sum(axis=1) > 4).any(), "no record with more than four nonzero probabilities"
    if module == ALL_OPEN:
        assert ((o.logits != 0).sum(axis=1) == r.A).any(), "no root whose 31 children were all visited"
    if r.twists:
        assert o.evals > 0                    # (full_predict averages ALL twists: the device's forward_evals is evals x twists)
    assert o.evals >= int(o.ep_len.sum())     # a root per record at least
    if r.var:
        assert int(o.counts.min()) == 0 and int(o.counts.max()) == r.n_obs
