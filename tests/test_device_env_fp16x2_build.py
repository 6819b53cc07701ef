"""CPU: the fp16x2 form of a device-environment module (build_device_env(..., fp16x2=True): `#define TW_DEVICE_ENV_FP16X2`) -- what can
be checked without a device.  The fp16x2 module of GridWorld 3 x 3 holds rollout_env16x2_kernel and pack_generic16x2_kernel beside
the f32 and fp16 kernels, keeps both out of scratch memory, passes the MFMA hazard scan, answers the capability query
groups_per_cu(5, 0, null) with hipSuccess and says DeviceEnv.fp16x2; the same struct built without the flag, and with fp16=True
alone, names neither kernel, answers hipErrorInvalidValue and says False.  The descriptor did not grow (it ends with groups_per_cu16,
layout[2] == its size); the kinds never serve each other from the cache; the flag composes with wide=True and with search=True."""
import ctypes as C
import os
import re

import pytest

from tests.device_env_util import GRIDWORLD_HPP
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE

GW3 = "tw_examples::GridWorld3x3"
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1


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


def _env(so, name):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(so, name, [3, 3, 12, 1], max_records=13)


def test_fp16x2_module_of_gridworld3x3():
    import sys
    from twisterl_amd.env import DeviceEnvDesc
    so = _build("gridworld3x3_fp16x2", fp16x2=True)
    mod, d = _desc(so, "gridworld3x3_fp16x2")
    assert d.launch_rollout16 and d.groups_per_cu16 and d.groups_per_cu and not d.launch_search
    # the descriptor still ends with groups_per_cu16
    assert d.layout[2] == C.sizeof(DeviceEnvDesc) == DeviceEnvDesc.groups_per_cu16.offset + C.sizeof(C.c_void_p) and len(d.layout) == 8
    text, kernels = _kernels(so)
    want = ("rollout_env_kernel", "solve_env_kernel", "rollout_env16_kernel", "pack_generic16_kernel", "rollout_env16x2_kernel",
            "pack_generic16x2_kernel")
    assert len(kernels) == 6, kernels
    for k in want:
        assert sum(1 for n in kernels if re.search(rf"\d+{k}I", n)) == 1, (k, kernels)
    assert sum(1 for n in kernels if re.search(r"rollout_env16x2_kernelI.*Li9EEEvNS_16EnvRollout16ArgsE", n)) == 1, kernels   # the kernarg of the fp16 kernel
    scratch = {name: int(size) for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) == 6
    for name, size in scratch.items():
        if "16x2_kernel" in name:
            assert size == 0, (name, size)
    body = text.split("rollout_env16x2_kernel", 1)[1]
    assert "v_mfma_f32_16x16x32_f16" in body
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    hits, counts = scan.scan_file(so[:-3] + ".s")
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(so[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_FP16\n#define TW_DEVICE_ENV_FP16X2\n#include" in src and f"TW_DEVICE_ENV({GW3}, gridworld3x3_fp16x2)" in src
    assert int(d.groups_per_cu(5, 0, None)) == HIP_SUCCESS
    assert int(d.groups_per_cu(3, 0, None)) == HIP_ERROR_INVALID_VALUE and int(d.groups_per_cu(4, 0, None)) == HIP_ERROR_INVALID_VALUE
    env = _env(so, "gridworld3x3_fp16x2")
    assert env.fp16x2 is True and env.fp16 is True and env.fp16_solve is False and env.fp16_search is False and env.search is False


@pytest.mark.parametrize("kw", [{}, {"fp16": True}], ids=["default", "fp16"])
def test_a_module_without_the_flag_holds_neither_kernel(tmp_path, kw):
    name = "gw3_no_split"
    so = _build(name, out_dir=str(tmp_path), **kw)
    text, kernels = _kernels(so)
    assert len(kernels) == (4 if kw else 2), kernels
    assert "16x2" not in text and "TW_DEVICE_ENV_FP16X2" not in open(so[:-3] + ".hip").read()
    mod, d = _desc(so, name)
    assert int(d.groups_per_cu(5, 0, None)) == HIP_ERROR_INVALID_VALUE
    env = _env(so, name)
    assert env.fp16x2 is False and env.fp16 is bool(kw)


def test_the_kinds_never_share_a_cache_entry(tmp_path):
    """The same struct and name in one directory: the kind asked for is what is there, a repeated build of it is served from the cache."""
    name, d = "gw3_cache_x2", str(tmp_path)
    so = _build(name, out_dir=d, fp16x2=True)
    src = so[:-3] + ".hip"
    assert "#define TW_DEVICE_ENV_FP16X2" in open(src).read() and len(_kernels(so)[1]) == 6
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16x2=True) == so and os.stat(so).st_mtime_ns == before                        # cached
    assert _build(name, out_dir=d, fp16=True) == so and os.stat(so).st_mtime_ns != before                          # fp16 alone: rebuilt
    assert "FP16X2" not in open(src).read() and len(_kernels(so)[1]) == 4
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d) == so and os.stat(so).st_mtime_ns != before                                     # the default: rebuilt
    assert "FP16" not in open(src).read() and len(_kernels(so)[1]) == 2
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16x2=True) == so and os.stat(so).st_mtime_ns != before                        # and back
    assert "#define TW_DEVICE_ENV_FP16X2" in open(src).read() and len(_kernels(so)[1]) == 6


def test_the_flag_composes_with_wide_and_with_search(tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE["wideo17a17"]
    d = str(tmp_path)
    jobs = [(r.header, r.type, "wide_x2", {"wide": True, "fp16x2": True}), (GRIDWORLD_HPP, GW3, "search_x2", {"search": True, "fp16x2": True}),
            (GRIDWORLD_HPP, GW3, "all_x2", {"search": True, "fp16x2": True, "fp16_solve": True, "fp16_search": True})]
    with ThreadPoolExecutor(max_workers=3) as pool:
        wide, search, everything = pool.map(lambda j: build_device_env(j[0], j[1], j[2], out_dir=d, **j[3]), jobs)
    src = open(wide[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_WIDE\n#define TW_DEVICE_ENV_FP16\n#define TW_DEVICE_ENV_FP16X2\n" in src
    kernels = _kernels(wide)[1]
    assert len(kernels) == 6 and sum("rollout_env16x2_kernel" in k for k in kernels) == 1 and sum("pack_generic16x2_kernel" in k for k in kernels) == 1
    env = DeviceEnv(wide, "wide_x2", list(r.params), max_records=r.max_records)
    assert env.fp16x2 is True and env.num_actions() == 17 and not env.search
    kernels = _kernels(search)[1]
    assert len(kernels) == 7 and sum("rollout_env16x2_kernel" in k for k in kernels) == 1 and sum("mcts_env_kernel" in k for k in kernels) == 1
    env = _env(search, "search_x2")
    assert env.fp16x2 is True and env.search is True and env.fp16_search is False and env.fp16_solve is False
    kernels = _kernels(everything)[1]
    assert len(kernels) == 9, kernels
    env = _env(everything, "all_x2")
    assert env.fp16x2 and env.search and env.fp16_search and env.fp16_solve and env.fp16
