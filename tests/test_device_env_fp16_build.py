"""CPU: the fp16 form of a device-environment module (build_device_env(..., fp16=True): `#define TW_DEVICE_ENV_FP16`) -- what can be
checked without a device.  The fp16 module of GridWorld 3 x 3 carries both new descriptor members, holds rollout_env_kernel,
solve_env_kernel, rollout_env16_kernel and pack_generic16_kernel and no others, keeps the f16 kernel out of scratch memory and
passes the MFMA hazard scan; a default module has both members null and the two kernels it had before; the two forms (alone and
with wide / search) never serve each other from the cache; a descriptor shortened by the two members is refused with the rebuild
message; and the layout function of the binary16 weight image (gen16_elem, twisterl_amd/csrc/tw_engine_generic16.hpp), compiled
on the host in a stand-alone program, tiles each layer's [in_pad32][out_pad16] exactly once."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.device_env_util import GRIDWORLD_HPP, gridworld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GW3 = "tw_examples::GridWorld3x3"
WIDTHS = [(4, 1), (32, 16), (36, 17), (48, 48), (512, 508)]


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


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


def test_fp16_module_of_gridworld3x3():
    from twisterl_amd.env import DeviceEnv, DeviceEnvDesc
    so = _build("gridworld3x3_fp16", fp16=True)
    mod, d = _desc(so, "gridworld3x3_fp16")
    assert d.launch_rollout16 and d.groups_per_cu16 and d.launch_rollout and d.launch_solve and d.groups_per_cu and not d.launch_search
    assert d.layout[2] == C.sizeof(DeviceEnvDesc) and d.layout[1] == 6 and len(d.layout) == 8
    assert DeviceEnvDesc.launch_rollout16.offset == DeviceEnvDesc.groups_per_cu.offset + C.sizeof(C.c_void_p)      # appended, in this order
    assert DeviceEnvDesc.groups_per_cu16.offset == DeviceEnvDesc.launch_rollout16.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(DeviceEnvDesc) == DeviceEnvDesc.groups_per_cu16.offset + C.sizeof(C.c_void_p)
    text, kernels = _kernels(so)
    want = ("rollout_env_kernel", "solve_env_kernel", "rollout_env16_kernel", "pack_generic16_kernel")
    assert len(kernels) == 4, kernels
    for k in want:
        assert sum(1 for n in kernels if re.search(rf"\d+{k}I", n)) == 1, (k, kernels)
    assert sum(1 for n in kernels if re.search(r"rollout_env16_kernelI.*Li9EEEvNS_16EnvRollout16ArgsE", n)) == 1, kernels
    scratch = {name: int(size) for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) == 4
    for name, size in scratch.items():
        if "rollout_env16_kernel" in name or "pack_generic16_kernel" in name:
            assert size == 0, (name, size)
    assert "v_mfma_f32_16x16x32_f16" in text.split("rollout_env16_kernel", 1)[1]
    hits, counts = _scan(so[:-3] + ".s")
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(so[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_FP16\n#include" in src and f"TW_DEVICE_ENV({GW3}, gridworld3x3_fp16)" in src
    env = DeviceEnv(so, "gridworld3x3_fp16", [3, 3, 12, 1], max_records=13)
    assert env.fp16 is True and env.search is False and env.num_actions() == 4 and env.n_obs == 9


def test_default_module_has_neither_member_nor_kernel():
    env = gridworld(3)
    assert env.fp16 is False and not env._desc.launch_rollout16 and not env._desc.groups_per_cu16
    from tests.device_env_util import build_gridworld
    text, kernels = _kernels(build_gridworld(3))
    assert len(kernels) == 2 and sum("rollout_env_kernel" in k for k in kernels) == 1 and sum("solve_env_kernel" in k for k in kernels) == 1, kernels
    assert "rollout_env16" not in text and "pack_generic16" not in text and "16x16x32_f16" not in text
    assert "TW_DEVICE_ENV_FP16" not in open(build_gridworld(3)[:-3] + ".hip").read()


@pytest.mark.parametrize("extra", [{}, {"wide": True}, {"search": True}])
def test_the_two_forms_never_share_a_cache_entry(tmp_path, extra):
    """The same struct and name in one directory: the form asked for is what is there, a repeated build of it is served from the cache."""
    name = "gw3_cache"
    d = str(tmp_path)
    so = _build(name, out_dir=d, fp16=True, **extra)
    src = so[:-3] + ".hip"
    assert "#define TW_DEVICE_ENV_FP16" in open(src).read()
    assert ("#define TW_DEVICE_ENV_WIDE" in open(src).read()) == bool(extra.get("wide"))
    assert ("TW_DEVICE_ENV_SEARCH(" in open(src).read()) == bool(extra.get("search"))
    mod, desc = _desc(so, name)
    assert desc.launch_rollout16 and desc.groups_per_cu16 and bool(desc.launch_search) == bool(extra.get("search"))
    n16 = len(_kernels(so)[1])
    assert n16 == (5 if extra.get("search") else 4)
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16=True, **extra) == so and os.stat(so).st_mtime_ns == before                 # cached
    assert _build(name, out_dir=d, **extra) == so and os.stat(so).st_mtime_ns != before                            # the other form: rebuilt
    assert "TW_DEVICE_ENV_FP16" not in open(src).read() and len(_kernels(so)[1]) == n16 - 2
    before = os.stat(so).st_mtime_ns
    assert _build(name, out_dir=d, fp16=True, **extra) == so and os.stat(so).st_mtime_ns != before                 # and back
    assert "#define TW_DEVICE_ENV_FP16" in open(src).read() and len(_kernels(so)[1]) == n16


def test_a_descriptor_without_the_two_members_is_refused():
    """A module from before the members is shorter by two pointers: refused by the layout tag, with the rebuild message."""
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    L = _lib.lib()
    env = gridworld(3)
    vt = _lib.EnvVTable()
    assert L.tw_device_env_host_vtable(env._desc_ptr, env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_OK
    old = DeviceEnvDesc.from_buffer_copy(env._desc)
    old.layout[2] -= 2 * C.sizeof(C.c_void_p)
    assert L.tw_device_env_host_vtable(C.addressof(old), env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
    assert "another library layout" in _lib.last_error() and "rebuild it" in _lib.last_error()


_LAYOUT_MAIN = r"""
#include "tw_engine_generic16.hpp"
#include <cstdio>
#include <vector>
int main()
{
    const unsigned cases[][2] = {%s};
    for (auto &c : cases) {
        const unsigned in = c[0], out = c[1], ip = tw::gen16_in_pad(in), op = tw::gen16_out_pad(out);
        const size_t n = tw::gen16_layer_halves(in, out);
        std::vector<unsigned char> seen(n, 0);
        size_t bad = 0;
        for (unsigned k = 0; k < ip; ++k)
            for (unsigned o = 0; o < op; ++o) {
                const size_t e = tw::gen16_elem(in, k, o);
                if (e >= n || seen[e]++) ++bad;
            }
        size_t holes = 0;
        for (size_t i = 0; i < n; ++i) holes += seen[i] != 1;
        // a lane's eight halves of one MFMA are eight consecutive inputs of one output, 16 bytes apart from the next lane's
        const size_t lane_ok = tw::gen16_elem(in, 7, 0) - tw::gen16_elem(in, 0, 0) == 7 && tw::gen16_elem(in, 0, 1) - tw::gen16_elem(in, 0, 0) == 8 &&
                               tw::gen16_elem(in, 8, 0) - tw::gen16_elem(in, 0, 0) == 128;
        std::printf("%%u %%u %%u %%u %%zu %%zu %%zu %%zu\n", in, out, ip, op, n, bad, holes, lane_ok);
    }
    tw::LayerDev ls[2] = {};
    ls[0].in = 36; ls[0].out = 20; ls[1].in = 17; ls[1].out = 4;
    std::printf("base %%zu %%zu %%zu %%zu\n", tw::gen16_table_halves(81, 36), tw::gen16_layer_base(81, 36, ls, 0), tw::gen16_layer_base(81, 36, ls, 1),
                tw::gen16_image_halves(81, 36, ls, 2));
    return 0;
}
"""


def test_the_image_layout_tiles_every_layer_exactly_once(tmp_path):
    from twisterl_amd.build import CSRC, FLAGS, hipcc
    src = tmp_path / "layout_main.hip"
    src.write_text(_LAYOUT_MAIN % ", ".join("{%d, %d}" % w for w in WIDTHS))
    exe = tmp_path / "layout_main"
    r = subprocess.run([hipcc(), *[f for f in FLAGS if f not in ("-fPIC",)], "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(WIDTHS) + 1, out.stdout
    for (i, o), ln in zip(WIDTHS, lines):
        f = [int(x) for x in ln.split()]
        ip, op = (i + 31) // 32 * 32, (o + 15) // 16 * 16
        assert f == [i, o, ip, op, ip * op, 0, 0, 1], (ln, ip, op)
    tab = (81 * 36 + 7) // 8 * 8
    assert lines[-1] == f"base {tab} {tab} {tab + 64 * 32} {tab + 64 * 32 + 32 * 16 + 4 * 512}", lines[-1]
