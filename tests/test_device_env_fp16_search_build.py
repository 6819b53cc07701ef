"""CPU: the fp16_search form of a device-environment module (build_device_env(..., fp16_search=True) beside search=True or
wide_search=True: `#define TW_DEVICE_ENV_FP16_SEARCH`, which implies TW_DEVICE_ENV_FP16) -- what can be checked without a device.  Such
a module holds mcts_env16_kernel beside mcts_env_kernel and the image pack, has the new kernel on v_mfma_f32_16x16x32_f16 and passes
the MFMA hazard scan; a search module without the flag -- fp16_solve=True included -- holds no such kernel; the flag without a search
form is a ValueError before anything is compiled; the capability query groups_per_cu(4, 0, null) -- what the library's search_f16() and
DeviceEnv.fp16_search ask, the descriptor having no member for it -- answers without a GPU; the form has a cache entry of its own; and
the search loop exists ONCE, in csrc/tw_env_mcts_loop.hpp, which the two kernels include."""
import ctypes as C
import functools
import glob
import os
import re
import signal

import pytest

from tests.device_env_util import GRIDWORLD_HPP
from tests.device_env_wide_search import BY_MODULE as WIDE_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GW3 = "tw_examples::GridWorld3x3"
HIP_ERROR_INVALID_VALUE = 1
WIDE_ROW = "wideo17a17_ws"
# name -> (header, type, flags, the kernels the module holds)
BASE = ("rollout_env_kernel", "solve_env_kernel")
F16 = ("rollout_env16_kernel", "pack_generic16_kernel")
MODULES = {
    "gridworld3x3_f16az": (GRIDWORLD_HPP, GW3, {"fp16_search": True, "search": True}, BASE + F16 + ("mcts_env_kernel", "mcts_env16_kernel")),
    WIDE_ROW + "_f16": (WIDE_ROWS[WIDE_ROW].header, WIDE_ROWS[WIDE_ROW].type, {"fp16_search": True, "wide_search": True},
                        BASE + F16 + ("mcts_env_kernel", "mcts_env16_kernel")),
    "gridworld3x3_az": (GRIDWORLD_HPP, GW3, {"search": True}, BASE + ("mcts_env_kernel",)),
    "gridworld3x3_fp16s_az": (GRIDWORLD_HPP, GW3, {"fp16_solve": True, "search": True}, BASE + F16 + ("solve_env16_kernel", "mcts_env_kernel")),
}
NEW = [n for n, m in MODULES.items() if m[2].get("fp16_search")]


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16_search build test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(600)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@functools.lru_cache(maxsize=None)
def build_all():
    """The four modules of this file, built once per session side by side -> {name: path}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    with ThreadPoolExecutor(max_workers=min(16, len(MODULES))) as pool:
        paths = list(pool.map(lambda n: build_device_env(MODULES[n][0], MODULES[n][1], n, **MODULES[n][2]), MODULES))
    return dict(zip(MODULES, paths))


def _env(name):
    from twisterl_amd.env import DeviceEnv
    if name.startswith("gridworld"):
        return DeviceEnv(build_all()[name], name, [3, 3, 12, 1], max_records=13)
    r = WIDE_ROWS[WIDE_ROW]
    return DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)


def _kernels(so):
    text = open(so[:-3] + ".s").read()
    return text, re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)


def _body(text, kernel):
    """The instructions of one kernel: from its label to the end of the function."""
    sym = next(n for n in re.findall(r"^(_Z\S+):", text, flags=re.M) if re.search(rf"\d+{kernel}I", n))
    body = text.split(f"\n{sym}:", 1)[1]
    return body.split(".Lfunc_end", 1)[0]


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


@pytest.mark.parametrize("name", sorted(MODULES))
def test_the_kernels_a_module_holds(name):
    so = build_all()[name]
    text, kernels = _kernels(so)
    want = MODULES[name][3]
    assert len(kernels) == len(want), kernels
    for k in want:
        assert sum(1 for n in kernels if re.search(rf"\d+{k}I", n)) == 1, (k, kernels)
    assert ("mcts_env16_kernel" in text) == (name in NEW)
    src = open(so[:-3] + ".hip").read()
    assert ("#define TW_DEVICE_ENV_FP16_SEARCH\n" in src) == (name in NEW)
    env = _env(name)
    assert env.search is True and env.fp16_search is (name in NEW)
    assert env.fp16 is ("rollout_env16_kernel" in want) and env.fp16_solve is ("solve_env16_kernel" in want)


@pytest.mark.parametrize("name", NEW)
def test_the_new_kernel_is_on_the_f16_matrix_core_and_the_scan_is_clean(name):
    so = build_all()[name]
    text, kernels = _kernels(so)
    nc = 9 if name.startswith("gridworld") else 25
    assert sum(1 for n in kernels if re.search(rf"mcts_env16_kernelI.*Li{nc}EEEvNS_11EnvMctsArgsE", n)) == 1, kernels
    body = _body(text, "mcts_env16_kernel")
    assert "v_mfma_f32_16x16x32_f16" in body and "s_endpgm" in body
    assert "v_mfma_f32_16x16x32_f16" not in _body(text, "mcts_env_kernel")                # the f32 kernel of the same module stays f32
    hits, counts = _scan(so[:-3] + ".s")
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(so[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_FP16\n" in src and "#define TW_DEVICE_ENV_FP16_SEARCH\n#include" in src
    assert "TW_DEVICE_ENV_FP16_SOLVE" not in src


def test_the_define_alone_implies_the_fp16_form():
    header = open(os.path.join(ROOT, "include", "twisterl_device_env.hpp")).read()
    m = re.search(r"#if defined\(TW_DEVICE_ENV_FP16_SEARCH\) && !defined\(TW_DEVICE_ENV_FP16\)\n#define TW_DEVICE_ENV_FP16\n#endif\n", header)
    assert m and m.start() < header.index('#include "tw_rollout_env.hpp"')


@pytest.mark.parametrize("extra", [{}, {"wide": True}, {"fp16": True}, {"fp16_solve": True}])
def test_the_flag_without_a_search_form_is_refused_before_anything_is_compiled(tmp_path, monkeypatch, extra):
    import subprocess
    from twisterl_amd import build

    def no_compiler(*_a, **_k):
        raise AssertionError("the compiler was started")
    monkeypatch.setattr(subprocess, "run", no_compiler)
    with pytest.raises(ValueError, match="fp16_search=True needs the search kernel: search=True or wide_search=True"):
        build.build_device_env(GRIDWORLD_HPP, GW3, "gw3_refused", out_dir=str(tmp_path), fp16_search=True, **extra)
    assert os.listdir(str(tmp_path)) == []


def test_the_capability_query_needs_no_gpu():
    """Index 4 with a null result: 0 where the module holds the kernel, hipErrorInvalidValue elsewhere, with or without a device.  A
    null result for the other kernels stays an error, and index 3 stays the f16 evaluate kernel's."""
    for name in sorted(MODULES):
        env = _env(name)
        want = 0 if name in NEW else HIP_ERROR_INVALID_VALUE
        assert int(env._desc.groups_per_cu(4, 0, None)) == want, name
        assert int(env._desc.groups_per_cu(4, 1 << 14, None)) == want, name
        assert int(env._desc.groups_per_cu(3, 0, None)) == (0 if "solve_env16_kernel" in MODULES[name][3] else HIP_ERROR_INVALID_VALUE), name
        for k in (0, 1, 2, 5, -1):
            assert int(env._desc.groups_per_cu(k, 0, None)) == HIP_ERROR_INVALID_VALUE, (name, k)
    out = C.c_int(-7)
    for name in sorted(set(MODULES) - set(NEW)):                                          # no kernel: the result is not touched either
        assert int(_env(name)._desc.groups_per_cu(4, 0, C.byref(out))) == HIP_ERROR_INVALID_VALUE and out.value == -7


def test_the_descriptor_did_not_grow_and_the_abi_stays():
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    env, old = _env("gridworld3x3_f16az"), _env("gridworld3x3_az")
    assert env._desc.layout[2] == C.sizeof(DeviceEnvDesc) == DeviceEnvDesc.groups_per_cu16.offset + C.sizeof(C.c_void_p)
    assert list(env._desc.layout) == list(old._desc.layout)
    assert _lib.lib().tw_abi_version() == 6


def test_the_form_has_a_cache_entry_of_its_own(tmp_path):
    """The same struct and name in one directory: the form asked for is what is there, a repeated build of it is served from the cache,
    and a form without the flag generates the source it generated before."""
    from twisterl_amd.build import build_device_env
    name, d = "gw3_cache", str(tmp_path)
    before = None
    for kw, has in (({"search": True}, False), ({"search": True, "fp16_search": True}, True), ({"search": True, "fp16": True}, False),
                    ({"search": True, "fp16_search": True, "fp16": True}, True)):
        so = build_device_env(GRIDWORLD_HPP, GW3, name, out_dir=d, **kw)
        now = os.stat(so).st_mtime_ns
        assert now != before, (kw, "served from another form's cache entry")
        src = open(so[:-3] + ".hip").read()
        defines = "".join(f"#define {x}\n" for x, on in (("TW_DEVICE_ENV_FP16", has or kw.get("fp16")), ("TW_DEVICE_ENV_FP16_SEARCH", has)) if on)
        assert src == f'// generated by twisterl_amd.build.build_device_env\n{defines}#include "{GRIDWORLD_HPP}"\nTW_DEVICE_ENV_SEARCH({GW3}, {name})\n'
        assert sum("mcts_env16_kernel" in k for k in _kernels(so)[1]) == (1 if has else 0), kw
        assert build_device_env(GRIDWORLD_HPP, GW3, name, out_dir=d, **kw) == so and os.stat(so).st_mtime_ns == now, (kw, "not cached")
        before = now


def test_the_search_loop_exists_once():
    """mcts_env_kernel and mcts_env16_kernel include ONE body file; a marker line of the loop occurs in no other file."""
    csrc = os.path.join(ROOT, "twisterl_amd", "csrc")
    kernels = open(os.path.join(csrc, "tw_mcts_env.hpp")).read()
    assert len(re.findall(r'^#include "tw_env_mcts_loop\.hpp"$', kernels, flags=re.M)) == 2
    marker = "auto expand = [&](uint32_t idx) -> uint32_t {"
    holders = []
    for path in sorted(glob.glob(os.path.join(csrc, "*")) + glob.glob(os.path.join(ROOT, "include", "*"))):
        n = open(path, errors="replace").read().count(marker)
        if n:
            holders.append((os.path.basename(path), n))
    assert holders == [("tw_env_mcts_loop.hpp", 1)], holders
    loop = open(os.path.join(csrc, "tw_env_mcts_loop.hpp")).read()
    assert "#pragma once" not in loop and "#ifndef" not in loop
    for other in sorted(glob.glob(os.path.join(csrc, "*")) + glob.glob(os.path.join(ROOT, "include", "*"))):
        if os.path.basename(other) != "tw_mcts_env.hpp":
            assert '#include "tw_env_mcts_loop.hpp"' not in open(other, errors="replace").read(), other
