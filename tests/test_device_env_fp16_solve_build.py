"""CPU: the fp16_solve form of a device-environment module (build_device_env(..., fp16_solve=True): `#define TW_DEVICE_ENV_FP16_SOLVE`,
which implies TW_DEVICE_ENV_FP16) -- what can be checked without a device.  The module of GridWorld 3 x 3 holds rollout_env_kernel,
solve_env_kernel, rollout_env16_kernel, pack_generic16_kernel and solve_env16_kernel (with search=True: mcts_env_kernel too) and no
others, keeps the new kernel out of scratch memory, has it on v_mfma_f32_16x16x32_f16 and passes the MFMA hazard scan; the capability
query groups_per_cu(3, 0, null) -- what the library's attempts_on_device() and DeviceEnv.fp16_solve ask, the descriptor having no member
for it -- answers without a GPU, 0 for this form and hipErrorInvalidValue for a fp16=True and a default module, whose kernel lists do
not name the new kernel; the three forms never serve each other from the cache; a descriptor whose layout[5] is the EnvSolveArgs of
before the image is refused with the rebuild message; and collector.evaluate / collector.solve refuse an unknown precision before
anything else happens."""
import ctypes as C
import functools
import os
import re
import signal

import pytest

from tests.device_env_util import GRIDWORLD_HPP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GW3 = "tw_examples::GridWorld3x3"
HIP_ERROR_INVALID_VALUE = 1
FIVE = ("rollout_env_kernel", "solve_env_kernel", "rollout_env16_kernel", "pack_generic16_kernel", "solve_env16_kernel")
# what EnvSolveArgs gained: Gen16Image = {_Float16 *img; uint64_t halves;}
IMAGE_BYTES = C.sizeof(C.c_void_p) + C.sizeof(C.c_uint64)


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16_solve build test exceeded its time limit")
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
    jobs = [("gridworld3x3_fp16s", {"fp16_solve": True}), ("gridworld3x3_fp16s_az", {"fp16_solve": True, "search": True}),
            ("gridworld3x3_fp16", {"fp16": True}), ("gridworld3x3", {})]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(GRIDWORLD_HPP, GW3, j[0], **j[1]), jobs))
    return {j[0]: p for j, p in zip(jobs, paths)}


def _env(name):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[name], name, [3, 3, 12, 1], max_records=13)


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


@pytest.mark.parametrize("search", [False, True])
def test_fp16_solve_module_of_gridworld3x3(search):
    name = "gridworld3x3_fp16s_az" if search else "gridworld3x3_fp16s"
    so = build_all()[name]
    text, kernels = _kernels(so)
    want = FIVE + (("mcts_env_kernel",) if search else ())
    assert len(kernels) == len(want), kernels
    for k in want:
        assert sum(1 for n in kernels if re.search(rf"\d+{k}I", n)) == 1, (k, kernels)
    assert sum(1 for n in kernels if re.search(r"solve_env16_kernelI.*Li9EEEvNS_12EnvSolveArgsE", n)) == 1, kernels
    scratch = {n: int(size) for n, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(scratch) == len(want)
    new = [n for n in scratch if "solve_env16_kernel" in n]
    assert len(new) == 1 and scratch[new[0]] == 0, scratch
    body = _body(text, "solve_env16_kernel")
    assert "v_mfma_f32_16x16x32_f16" in body and "s_endpgm" in body
    assert "v_mfma_f32_16x16x32_f16" not in _body(text, "solve_env_kernel")               # the f32 kernel of the same module stays f32
    hits, counts = _scan(so[:-3] + ".s")
    assert hits == [] and sum(counts.values()) > 0 and "gfx950" in text
    src = open(so[:-3] + ".hip").read()
    assert "#define TW_DEVICE_ENV_FP16_SOLVE\n#include" in src and "#define TW_DEVICE_ENV_FP16\n" in src
    assert f"{'TW_DEVICE_ENV_SEARCH' if search else 'TW_DEVICE_ENV'}({GW3}, {name})" in src
    env = _env(name)
    assert env.fp16_solve is True and env.fp16 is True and env.search is search and env.num_actions() == 4 and env.n_obs == 9


def test_the_define_alone_implies_the_fp16_form():
    """A hand-written module source that defines only TW_DEVICE_ENV_FP16_SOLVE gets the f16 rollout kernel and its descriptor members too:
    the header defines TW_DEVICE_ENV_FP16 for it before anything reads that."""
    header = open(os.path.join(ROOT, "include", "twisterl_device_env.hpp")).read()
    m = re.search(r"#if defined\(TW_DEVICE_ENV_FP16_SOLVE\) && !defined\(TW_DEVICE_ENV_FP16\)\n#define TW_DEVICE_ENV_FP16\n#endif\n", header)
    assert m and m.start() < header.index('#include "tw_rollout_env.hpp"')


def test_the_other_forms_have_neither_the_kernel_nor_the_capability():
    for name, n_kernels, fp16 in (("gridworld3x3_fp16", 4, True), ("gridworld3x3", 2, False)):
        text, kernels = _kernels(build_all()[name])
        assert len(kernels) == n_kernels and "solve_env16" not in text, (name, kernels)
        assert "TW_DEVICE_ENV_FP16_SOLVE" not in open(build_all()[name][:-3] + ".hip").read()
        env = _env(name)
        assert env.fp16_solve is False and env.fp16 is fp16


def test_the_capability_query_needs_no_gpu():
    """Index 3 with a null result: 0 where the module holds the kernel, hipErrorInvalidValue elsewhere -- with or without a device, and
    through the search form's groups_per_cu as through the plain one.  A null result for the other kernels stays an error."""
    for name, want in (("gridworld3x3_fp16s", 0), ("gridworld3x3_fp16s_az", 0), ("gridworld3x3_fp16", HIP_ERROR_INVALID_VALUE),
                       ("gridworld3x3", HIP_ERROR_INVALID_VALUE)):
        env = _env(name)
        assert int(env._desc.groups_per_cu(3, 0, None)) == want, name
        assert int(env._desc.groups_per_cu(3, 1 << 14, None)) == want, name
        for k in (0, 1, 4, -1):
            assert int(env._desc.groups_per_cu(k, 0, None)) == HIP_ERROR_INVALID_VALUE, (name, k)
    out = C.c_int(-7)
    for name in ("gridworld3x3_fp16", "gridworld3x3"):                                     # no kernel: the result is not touched either
        assert int(_env(name)._desc.groups_per_cu(3, 0, C.byref(out))) == HIP_ERROR_INVALID_VALUE and out.value == -7


def _build(name, out_dir, **kw):
    from twisterl_amd.build import build_device_env
    return build_device_env(GRIDWORLD_HPP, GW3, name, out_dir=out_dir, **kw)


@pytest.mark.parametrize("extra", [{}, {"wide": True}, {"search": True}, {"wide_search": True}])
def test_the_three_forms_never_share_a_cache_entry(tmp_path, extra):
    """The same struct and name in one directory: the form asked for is what is there, a repeated build of it is served from the cache."""
    name, d = "gw3_cache", str(tmp_path)
    n_search = 1 if extra.get("search") or extra.get("wide_search") else 0
    forms = [({}, 2), ({"fp16_solve": True}, 5), ({"fp16": True}, 4), ({"fp16_solve": True, "fp16": True}, 5)] + ([({}, 2)] if not extra else [])
    so, before = None, None
    for kw, n in forms:
        so = _build(name, d, **kw, **extra)
        now = os.stat(so).st_mtime_ns
        assert now != before, (kw, "served from another form's cache entry")
        src = open(so[:-3] + ".hip").read()
        assert ("#define TW_DEVICE_ENV_FP16_SOLVE\n" in src) == bool(kw.get("fp16_solve"))
        assert ("#define TW_DEVICE_ENV_FP16\n" in src) == bool(kw.get("fp16") or kw.get("fp16_solve"))
        assert ("#define TW_DEVICE_ENV_WIDE\n" in src) == bool(extra.get("wide") or extra.get("wide_search"))
        kernels = _kernels(so)[1]
        assert len(kernels) == n + n_search and sum("solve_env16_kernel" in k for k in kernels) == (1 if kw.get("fp16_solve") else 0), (kw, kernels)
        assert _build(name, d, **kw, **extra) == so and os.stat(so).st_mtime_ns == now, (kw, "not cached")
        before = now


def test_a_module_of_the_old_solve_arguments_is_refused_with_the_rebuild_message():
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    L = _lib.lib()
    env = _env("gridworld3x3_fp16s")
    vt = _lib.EnvVTable()
    assert L.tw_device_env_host_vtable(env._desc_ptr, env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_OK
    old = DeviceEnvDesc.from_buffer_copy(env._desc)
    old.layout[5] -= IMAGE_BYTES
    assert L.tw_device_env_host_vtable(C.addressof(old), env._obj, env._desc.state_bytes, C.byref(vt)) == _lib.TW_ERR_INVALID
    assert "another library layout" in _lib.last_error() and "rebuild it" in _lib.last_error()
    prm = _lib.SolveParams(1, 1, 0, 1.41, 1, 7, _lib.TW_PREC_F16)
    s, r = C.c_float(), C.c_float()
    no_policy = C.create_string_buffer(64)            # (never read: the descriptor is checked first, and a policy needs a device)
    rc = L.tw_evaluate_device_env(C.addressof(old), env._obj, env._desc.state_bytes, C.addressof(no_policy), C.byref(prm), 4, 0, 13, C.byref(s), C.byref(r))
    assert rc == _lib.TW_ERR_INVALID
    msg = _lib.last_error()
    assert "tw_evaluate_device_env" in msg and "another library layout" in msg and "rebuild it" in msg, msg
    assert _lib.lib().tw_abi_version() == 6


def test_the_descriptor_did_not_grow():
    from twisterl_amd.env import DeviceEnvDesc
    env = _env("gridworld3x3_fp16s")
    assert env._desc.layout[2] == C.sizeof(DeviceEnvDesc) == DeviceEnvDesc.groups_per_cu16.offset + C.sizeof(C.c_void_p)


@pytest.mark.parametrize("bad", ["fp8", "", "FP16", None, 16])
def test_an_unknown_precision_is_a_value_error_before_any_library_call(monkeypatch, bad):
    from twisterl_amd import _lib, collector
    from twisterl_amd.nn import Policy

    def no_library(*_a, **_k):
        raise AssertionError("the library was called")
    env = _env("gridworld3x3_fp16s")
    policy = object.__new__(Policy)                   # (never uploaded: the precision is checked first)
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match="precision must be one of"):
        collector.evaluate(env, policy, 4, True, 1, 0, 7, 1.41, 1, 1, precision=bad)
    with pytest.raises(ValueError, match="precision must be one of"):
        collector.solve(env, policy, True, 1, 0, 1.41, 1, seed=7, precision=bad)
    with pytest.raises(TypeError):                    # keyword-only, both
        collector.evaluate(env, policy, 4, True, 1, 0, 7, 1.41, 1, 1, "fp16")
    with pytest.raises(TypeError):
        collector.solve(env, policy, True, 1, 0, 1.41, 1, 7)


def test_every_known_precision_reaches_the_solve_parameters():
    from twisterl_amd import _lib, collector
    for name, value in _lib.PRECISIONS.items():
        assert collector._solve_params(True, 1, 0, 1.41, 1, 7, name).precision == value
    assert collector._solve_params(True, 1, 0, 1.41, 1, 7).precision == _lib.TW_PREC_F32_EXACT
    import inspect
    for fn in (collector.evaluate, collector.solve):
        p = inspect.signature(fn).parameters["precision"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "fp32"
