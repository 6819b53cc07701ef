"""CPU: the fp16x2_solve form of a device-environment module (build_device_env(..., fp16x2_solve=True): `#define
TW_DEVICE_ENV_FP16X2_SOLVE`) -- what can be checked without a device.  The module of GridWorld 3 x 3 holds solve_env16x2_kernel beside
the six kernels of an fp16x2 module, keeps it out of scratch memory, passes the MFMA hazard scan, answers the capability query
groups_per_cu(6, 0, null) with hipSuccess and says DeviceEnv.fp16x2_solve; the same struct built without the flag, with fp16x2=True
alone and with fp16_solve=True alone answers hipErrorInvalidValue and says False.  Neither the descriptor nor its layout words grew;
the kinds never serve each other from the cache; the flag composes with wide=True and with the search forms; the evaluate loop still
exists once, included twice by tw_rollout_env.hpp and once by tw_solve_env16x2.hpp."""
import ctypes as C
import glob
import os
import re

from tests.device_env_util import GRIDWORLD_HPP
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE

GW3 = "tw_examples::GridWorld3x3"
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVEN = ("rollout_env_kernel", "solve_env_kernel", "rollout_env16_kernel", "pack_generic16_kernel", "rollout_env16x2_kernel",
         "pack_generic16x2_kernel", "solve_env16x2_kernel")


def _build(name, out_dir=None, **kw):
    from twisterl_amd.build import build_device_env
    return build_device_env(GRIDWORLD_HPP, GW3, name, out_dir=out_dir, **kw)


def _desc(so, name):
    from twisterl_amd.env import DeviceEnvDesc
    from twisterl_amd import _lib
    _lib.lib()
    mod = C.CDLL(so)
    fn = getattr(mod, f"tw_device_env_{name}")
    fn.restype = C.c_void_p
    return mod, DeviceEnvDesc.from_address(fn())


def _kernels(so):
    text = open(so[:-3] + ".s").read()
    return text, re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)


def _count(kernels, k):
    return sum(1 for n in kernels if re.search(rf"\d+{k}I", n))


def _env(so, name):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(so, name, [3, 3, 12, 1], max_records=13)


def test_fp16x2_solve_module_of_gridworld3x3():
    import sys
    from twisterl_amd.env import DeviceEnvDesc
    name = "gridworld3x3_fp16x2s"
    so = _build(name, fp16x2_solve=True)
    mod, d = _desc(so, name)
    assert d.launch_rollout16 and d.groups_per_cu16 and d.groups_per_cu and d.launch_solve and not d.launch_search
    text, kernels = _kernels(so)
    assert len(kernels) == 7, kernels
    for k in SEVEN:
        assert _count(kernels, k) == 1, (k, kernels)
    assert sum(1 for n in kernels if re.search(r"solve_env16x2_kernelI.*Li9EEEvNS_12EnvSolveArgsE", n)) == 1, kernels   # the kernarg of the other two
    scratch = {n: int(size) for n, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) == 7
    new = [n for n in scratch if "solve_env16x2_kernel" in n]
    assert len(new) == 1 and scratch[new[0]] == 0, scratch
    body = text.split(new[0] + ":", 1)[1].split(".end_amdhsa_kernel", 1)[0]
    assert "v_mfma_f32_16x16x32_f16" in body and "s_endpgm" in body
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    hits, counts = scan.scan_file(so[:-3] + ".s")
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(so[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_FP16\n#define TW_DEVICE_ENV_FP16X2\n#define TW_DEVICE_ENV_FP16X2_SOLVE\n#include" in src
    assert f"TW_DEVICE_ENV({GW3}, {name})" in src
    assert int(d.groups_per_cu(6, 0, None)) == HIP_SUCCESS and int(d.groups_per_cu(5, 0, None)) == HIP_SUCCESS
    assert int(d.groups_per_cu(3, 0, None)) == HIP_ERROR_INVALID_VALUE and int(d.groups_per_cu(4, 0, None)) == HIP_ERROR_INVALID_VALUE
    assert int(d.groups_per_cu(7, 0, None)) == HIP_ERROR_INVALID_VALUE
    env = _env(so, name)
    assert env.fp16x2_solve is True and env.fp16x2 is True and env.fp16 is True
    assert env.fp16_solve is False and env.fp16_search is False and env.search is False
    assert C.sizeof(DeviceEnvDesc) == d.layout[2]


def test_modules_without_the_flag_and_the_sizes(tmp_path):
    """A default module, an fp16x2=True module and an fp16_solve=True module refuse kernel 6 with the test they always had; the
    descriptor and every layout word of the new form are a default module's."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.env import DeviceEnvDesc
    kinds = {"gw3_plain": {}, "gw3_x2": {"fp16x2": True}, "gw3_s16": {"fp16_solve": True}, "gw3_x2s": {"fp16x2_solve": True}}
    with ThreadPoolExecutor(max_workers=4) as pool:
        paths = dict(zip(kinds, pool.map(lambda n: _build(n, out_dir=str(tmp_path), **kinds[n]), kinds)))
    descs = {n: _desc(paths[n], n) for n in kinds}
    for n in ("gw3_plain", "gw3_x2", "gw3_s16"):
        d = descs[n][1]
        assert int(d.groups_per_cu(6, 0, None)) == HIP_ERROR_INVALID_VALUE, n
        assert "solve_env16x2_kernel" not in open(paths[n][:-3] + ".s").read() and "FP16X2_SOLVE" not in open(paths[n][:-3] + ".hip").read(), n
        env = _env(paths[n], n)
        assert env.fp16x2_solve is False, n
        assert (env.fp16x2, env.fp16, env.fp16_solve, env.fp16_search) == (n == "gw3_x2", n != "gw3_plain", n == "gw3_s16", False), n
    assert len(_kernels(paths["gw3_plain"])[1]) == 2 and len(_kernels(paths["gw3_x2"])[1]) == 6 and len(_kernels(paths["gw3_s16"])[1]) == 5
    new, plain = descs["gw3_x2s"][1], descs["gw3_plain"][1]
    assert int(new.groups_per_cu(6, 0, None)) == HIP_SUCCESS and _env(paths["gw3_x2s"], "gw3_x2s").fp16x2_solve is True
    assert C.sizeof(DeviceEnvDesc) == new.layout[2] == plain.layout[2] == DeviceEnvDesc.groups_per_cu16.offset + C.sizeof(C.c_void_p)
    assert len(new.layout) == len(plain.layout) == 8
    assert [int(x) for x in new.layout] == [int(x) for x in plain.layout]


def test_the_kinds_never_share_a_cache_entry(tmp_path):
    """The same struct and name in one directory: the kind asked for is what is there, a repeated build of it is served from the cache."""
    name, d = "gw3_cache_x2s", str(tmp_path)
    so = _build(name, out_dir=d, fp16x2_solve=True)
    src = so[:-3] + ".hip"
    assert "#define TW_DEVICE_ENV_FP16X2_SOLVE" in open(src).read() and len(_kernels(so)[1]) == 7
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16x2_solve=True) == so and os.stat(so).st_mtime_ns == before                  # cached
    assert _build(name, out_dir=d, fp16x2=True, fp16x2_solve=True) == so and os.stat(so).st_mtime_ns == before     # (implied: the same source)
    assert _build(name, out_dir=d, fp16x2=True) == so and os.stat(so).st_mtime_ns != before                        # fp16x2 alone: rebuilt
    assert "FP16X2_SOLVE" not in open(src).read() and "FP16X2" in open(src).read() and len(_kernels(so)[1]) == 6
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d) == so and os.stat(so).st_mtime_ns != before                                     # the default: rebuilt
    assert "FP16" not in open(src).read() and len(_kernels(so)[1]) == 2
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16x2_solve=True) == so and os.stat(so).st_mtime_ns != before                  # and back
    assert "#define TW_DEVICE_ENV_FP16X2_SOLVE" in open(src).read() and len(_kernels(so)[1]) == 7


def test_the_flag_composes_with_wide_and_with_search(tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE["wideo17a17"]
    d = str(tmp_path)
    jobs = [(r.header, r.type, "wide_x2s", {"wide": True, "fp16x2_solve": True}),
            (GRIDWORLD_HPP, GW3, "all_x2s", {"search": True, "fp16x2_solve": True, "fp16_solve": True, "fp16_search": True})]
    with ThreadPoolExecutor(max_workers=2) as pool:
        wide, everything = pool.map(lambda j: build_device_env(j[0], j[1], j[2], out_dir=d, **j[3]), jobs)
    src = open(wide[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_WIDE\n#define TW_DEVICE_ENV_FP16\n#define TW_DEVICE_ENV_FP16X2\n#define TW_DEVICE_ENV_FP16X2_SOLVE\n" in src
    # wide: the seven kernels of the plain form
    text, kernels = _kernels(wide)
    assert len(kernels) == 7 and all(_count(kernels, k) == 1 for k in SEVEN), kernels
    scratch = {n: int(size) for n, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert [v for n, v in scratch.items() if "solve_env16x2_kernel" in n] == [0]
    env = DeviceEnv(wide, "wide_x2s", list(r.params), max_records=r.max_records)
    assert env.fp16x2_solve is True and env.fp16x2 is True and env.num_actions() == 17 and not env.search and not env.fp16_solve
    # everything: those seven, solve_env16_kernel, mcts_env_kernel and mcts_env16_kernel -- the search module's query delegates kernel 6
    kernels = _kernels(everything)[1]
    assert len(kernels) == 10, kernels
    for k in SEVEN + ("solve_env16_kernel", "mcts_env_kernel", "mcts_env16_kernel"):
        assert _count(kernels, k) == 1, (k, kernels)
    env = DeviceEnv(everything, "all_x2s", [3, 3, 12, 1], max_records=13)
    assert env.fp16x2_solve and env.fp16x2 and env.search and env.fp16_search and env.fp16_solve and env.fp16
    mod, desc = _desc(everything, "all_x2s")
    assert [int(desc.groups_per_cu(k, 0, None)) for k in (3, 4, 5, 6)] == [HIP_SUCCESS] * 4
    assert int(desc.groups_per_cu(2, 0, None)) == HIP_ERROR_INVALID_VALUE      # (the f32 kernels have no capability query)


def test_the_evaluate_loop_still_exists_once():
    """(The loop head is looked for in the headers of csrc/, where every device-environment kernel lives: the Puzzle kernels of
    tw_rollout16.hip, tw_rollout_big.hip and tw_solve.hip have step loops of their own with the same head.)"""
    csrc = os.path.join(ROOT, "twisterl_amd", "csrc")
    head, inc = "while (__syncthreads_or(", '#include "tw_env_solve_loop.hpp"'
    assert open(os.path.join(csrc, "tw_rollout_env.hpp")).read().count(inc) == 2
    new = open(os.path.join(csrc, "tw_solve_env16x2.hpp")).read()
    assert new.count(inc) == 1 and new.count(head) == 0
    loop = open(os.path.join(csrc, "tw_env_solve_loop.hpp")).read()
    assert loop.count(head) == 1 and "#pragma once" not in loop
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        base = os.path.basename(path)
        text = open(path).read()
        if base.endswith(".hpp") and base not in ("tw_env_solve_loop.hpp", "tw_env_rollout_loop.hpp"):
            assert text.count(head) == 0, base
        if base not in ("tw_rollout_env.hpp", "tw_solve_env16x2.hpp"):
            assert inc not in text, base
