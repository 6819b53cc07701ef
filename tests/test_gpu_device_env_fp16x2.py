"""GPU: PPOCollector(precision="fp16x2").collect of device environments -- rollout_env16x2_kernel over EngineV16x2
(twisterl_amd/csrc/tw_engine_generic16x2.hpp: every Linear operand of a generic policy split into two binary16 terms, three products
per k-group on v_mfma_f32_16x16x32_f16), modules built with build_device_env(..., fp16x2=True).

Every collect (merge_order=False) is held to seven things: (1) tw_debug_last_launch names the split kernel (family ROLLOUT_BIG, nt 1,
the row's engine width, nw 32, persist as expected); (2) two collects give the same bytes; (3) the GPU's own actions replayed through
the module's HOST code give its obs ids (0xFFFF slots included), rewards, masks (-1e10 positions), ep_len and twist draws bit for bit;
(4) every action is oracle.sample_from_logits of the GPU's own logits and the spec's uniforms; (5) advs / rets are oracle.gae of the
GPU's own rewards and values, bit for bit; (6) every logit and value is within tests/ref64.forward_f64_bound(mode="fp16x2") of
float64, and within that bound plus the "f32" bound of the oracle's f32 forward (the triangle inequality; no fixed number, no record
left out) -- bounds that hold while every operand is below 4095, which a weight-norm ceiling shows on the CPU BEFORE the GPU is
touched; (7) the largest |gpu - oracle f32| is recorded, not gated: printed, and appended to the file TW_FP16X2_RECORD names.

The exactness probe needs no bound (tests/split16x2_ref.exact_arrays, shown exact on the CPU by tests/test_split16x2_ref.py): the GPU
must equal the oracle's f32 collect bit for bit and differ from its ARITH_F16 collect, which shows that the lo terms are really used.
Range: a weight of 4094 runs the split kernel; a weight of 4095, -4095, 5000 or NaN, an embedding output of -5000 and a hidden
activation of 5000 give the fp32 collect's bytes from the f32 kernel, with one line on stderr."""
import functools
import json
import os
import signal
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ref64, split16x2_ref as S
from tests.device_env_matrix import BY_MODULE as PROBE_ROWS_BY_MODULE, GAMMA, LAM, PROBE_HPP, engine_nc, host_env
from tests.device_env_matrix import policy_arrays as probe_arrays, twists as probe_twists
from tests.device_env_util import GRIDWORLD_HPP, gridworld
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE, policy_arrays as wide_arrays, twists as wide_twists
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs, oracle_policy

pytestmark = pytest.mark.gpu

PROBE_ROWS, WIDE_ROWS, WIDTHS = S.PROBE_ROWS, S.WIDE_ROWS, S.WIDTHS
EPISODES = (40, 100)                               # 2.5 and 6.25 workgroups of 16 columns
GW = SimpleNamespace(name="gridworld3x3_fp16x2", type="tw_examples::GridWorld3x3", n_obs=9, obs_size=81, A=4, max_steps=12, diff=3, seed=41)
NO_ID = 0xFFFF
NW_SPLIT = 32
FALLBACK_LINE = "[twisterl_hip] precision fp16x2: a weight or an activation is outside the range of the split-f16 terms"


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16x2 device-environment test exceeded its time limit")
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    from twisterl_amd import twisterl
    if twisterl_amd.device_count() < 1:
        pytest.fail("no GPU visible")
    return twisterl


def _oracle():
    from oracle import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def build_all():
    """Every fp16x2 module of this file, built once per session side by side, AT MOST 16 AT A TIME -> {name: path}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    jobs = [(PROBE_HPP, PROBE_ROWS_BY_MODULE[m].alias, m + "_fp16x2", {"fp16x2": True}) for m in PROBE_ROWS]
    jobs += [(WIDE_ROWS_BY_MODULE[m].header, WIDE_ROWS_BY_MODULE[m].type, m + "_fp16x2", {"fp16x2": True, "wide": True}) for m in WIDE_ROWS]
    jobs += [(GRIDWORLD_HPP, GW.type, GW.name, {"fp16x2": True})]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(j[0], j[1], j[2], **j[3]), jobs))
    return {j[2]: p for j, p in zip(jobs, paths)}


# ---- a case: environment, policies, what the replay needs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe_case(module):
    from twisterl_amd.env import DeviceEnv
    r = PROBE_ROWS_BY_MODULE[module]
    name = module + "_fp16x2"
    env = DeviceEnv(build_all()[name], name, [r.obs_size, r.max_steps, r.diff, -1], max_records=r.max_steps + 1)
    arrs, tws = probe_arrays(module), probe_twists(module)
    return SimpleNamespace(name=module, env=env, arrs=arrs, tw=tws, gp=amd_policy(arrs, *tws), op=oracle_policy(_oracle(), arrs, *tws),
                           n_obs=r.n_obs, A=r.A, var=r.var, diff=r.diff, seed=r.seed, offset=r.offset, nc=engine_nc(r.n_obs))


@functools.lru_cache(maxsize=None)
def _wide_case(module):
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE[module]
    name = module + "_fp16x2"
    env = DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)
    arrs, tws = wide_arrays(module), wide_twists(module)
    return SimpleNamespace(name=module, env=env, arrs=arrs, tw=tws, gp=amd_policy(arrs, *tws), op=oracle_policy(_oracle(), arrs, *tws),
                           n_obs=r.n_obs, A=r.A, var=r.var, diff=r.diff, seed=r.seed, offset=0, nc=engine_nc(r.n_obs))


def _gw_env():
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[GW.name], GW.name, [3, 3, GW.max_steps, GW.diff], max_records=GW.max_steps + 1)


def _gw_case(name, arrs, gp=None):
    return SimpleNamespace(name=name, env=_gw_env(), arrs=arrs, tw=((), ()), gp=gp if gp is not None else amd_policy(arrs),
                           op=oracle_policy(_oracle(), arrs), n_obs=GW.n_obs, A=GW.A, var=False, diff=GW.diff, seed=GW.seed, offset=0, nc=9)


@functools.lru_cache(maxsize=None)
def _width_case(key):
    return _gw_case("gw3_" + key, S.width_arrays(key))


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------
def collect(tw, c, E, precision="fp16x2", **kw):
    kw.setdefault("episode_offset", c.offset)
    return tw.collector.PPOCollector(E, GAMMA, LAM, 4, merge_order=False, precision=precision, **kw).collect(c.env, c.gp, seed=c.seed)


def assert_launch(c, persist, blocks=None, nw=NW_SPLIT):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["nw"], info["persist"], info["threads"]) == \
        (_lib.TW_KERNEL_ROLLOUT_BIG, 1, c.nc, nw, persist, 256), info
    if blocks is not None:
        assert info["blocks"] == blocks, info
    return info


def same_bytes(a, b):
    x, y = a.to_numpy(), b.to_numpy()
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k


def _uniforms(O, seed, ep, t, A):
    u = []
    for a in range(A):
        w = O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t | ((a >> 2) << 24), 1], [seed & 0xFFFFFFFF, seed >> 32])
        u.append(np.float32(w[a & 3] >> 8) * np.float32(1.0 / 16777216.0))
    return u


def _record(case, E, worst, n_records):
    print(f"[fp16x2] {case} E={E}: {n_records} records, max |gpu - oracle f32| = {worst:.3e}")
    path = os.environ.get("TW_FP16X2_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"what": "max_abs_deviation_from_oracle_f32", "case": case, "episodes": E, "records": n_records,
                                "value": worst}) + "\n")


def check_collect(c, g, E):
    """Checks 3 - 7 of the module docstring on one collect (merge_order=False); -> the largest deviation from the oracle's f32 forward."""
    O = _oracle()
    a = g.to_numpy()
    L = a["ep_len"].astype(np.int64)
    assert L.size == E and int(L.sum()) == a["logits"].shape[0] and a["logits"].shape[1] == c.A and a["obs"].shape[1] == c.n_obs
    starts = np.concatenate([[0], np.cumsum(L)])
    n_perms = len(c.tw[0])
    hproto = host_env(c.env)
    obs_rows, mask_rows, perm_rows = [], [], []
    for e in range(E):
        s, n = int(starts[e]), int(L[e])
        ep = c.offset + e
        env = hproto.copy()
        env.seed_episode(c.seed, ep)
        env.reset(c.diff)
        for t in range(n):
            ids = [int(x) for x in env.observe()]
            masks = [bool(m) for m in env.masks()]
            row = a["obs"][s + t].astype(np.int64)
            assert row[:len(ids)].tolist() == ids and (row[len(ids):] == NO_ID).all(), (c.name, e, t, row, ids)
            assert len(ids) == c.n_obs or c.var
            assert f32_bits(np.float32(env.value())) == f32_bits(a["rewards"][s + t]), (c.name, e, t)
            lg = a["logits"][s + t]
            assert ((lg == np.float32(-1e10)) == ~np.asarray(masks)).all(), (c.name, e, t, lg, masks)
            perm = -1
            if n_perms:
                perm = (O.philox4x32_10([ep & 0xFFFFFFFF, ep >> 32, t, 2], [c.seed & 0xFFFFFFFF, c.seed >> 32])[0] * n_perms) >> 32
            assert int(a["perms"][s + t]) == perm, (c.name, e, t)
            act = int(a["actions"][s + t])
            assert act == O.sample_from_logits(lg, _uniforms(O, c.seed, ep, t, c.A), det_log=True), (c.name, e, t)
            obs_rows.append(ids + [-1] * (c.n_obs - len(ids))); mask_rows.append(masks); perm_rows.append(perm)
            final = env.is_final()
            assert final == (t == n - 1), (c.name, e, t, n)
            if not final:
                env.next(act)
        advs, rets = O.gae(a["rewards"][s:s + n], a["values"][s:s + n], GAMMA, LAM)
        assert np.array_equal(f32_bits(advs), f32_bits(a["advs"][s:s + n])) and np.array_equal(f32_bits(rets), f32_bits(a["rets"][s:s + n])), (c.name, e)
    obs_arr, mask_arr, perm_arr = np.asarray(obs_rows, np.int64), np.asarray(mask_rows, bool), np.asarray(perm_rows, np.int64)
    m0, m1 = ref64.max_activations(c.arrs, c.tw[0], c.tw[1], obs_arr, perm_arr)
    assert max(m0, m1) < S.LIMIT
    l64, v64, el, ev = ref64.forward_f64_bound(c.arrs, c.tw[0], c.tw[1], obs_arr, mask_arr, perm_arr, "fp16x2")
    gl, gv = a["logits"].astype(np.float64), a["values"].astype(np.float64)
    dl, dv = np.abs(gl - l64), np.abs(gv - v64)
    # the oracle's f32 forward on the same records (a variable-length record: the ids it has)
    lo = np.empty_like(a["logits"]); vo = np.empty_like(a["values"])
    for i, (ids, mk, pm) in enumerate(zip(obs_rows, mask_rows, perm_rows)):
        l1, v1 = c.op.forward([x for x in ids if x >= 0], mk, perm=pm, arith=O.ARITH_CHAIN)
        lo[i], vo[i] = np.asarray(l1, np.float32), np.float32(v1)
    d32l, d32v = np.abs(gl - lo.astype(np.float64)), np.abs(gv - vo.astype(np.float64))
    worst = max(float(d32l[mask_arr].max()) if mask_arr.any() else 0.0, float(d32v.max()))
    _record(c.name, E, worst, int(L.sum()))
    print(f"[fp16x2] {c.name} E={E}: max |gpu - f64| logits {float(dl[mask_arr].max()):.3e} (bound at least {float(el[mask_arr].min()):.3e}), "
          f"values {float(dv.max()):.3e} (bound at least {float(ev.min()):.3e})")
    assert (dl[mask_arr] <= el[mask_arr]).all(), (c.name, float((dl - el)[mask_arr].max()), float(dl[mask_arr].max()), float(el[mask_arr].min()))
    assert (dv <= ev).all(), (c.name, float((dv - ev).max()), float(dv.max()))
    _, _, el32, ev32 = ref64.forward_f64_bound(c.arrs, c.tw[0], c.tw[1], obs_arr, mask_arr, perm_arr, "f32")
    assert (d32l[mask_arr] <= (el + el32)[mask_arr]).all(), (c.name, float((d32l - el - el32)[mask_arr].max()))
    assert (d32v <= ev + ev32).all(), (c.name, float((d32v - ev - ev32).max()))
    return worst


def assert_in_range(c):
    wmax, top = S.weight_ceiling(c.arrs, c.n_obs)                      # (on the CPU, before the GPU is touched)
    assert wmax < S.LIMIT and top < S.LIMIT, (c.name, wmax, top)


def run_case(tw, c, E):
    assert_in_range(c)
    g = collect(tw, c, E)
    assert_launch(c, 0, (E + 15) // 16)
    assert g.stats["rollout_blocks"] == (E + 15) // 16 and g.stats["rollout_threads"] == 256
    same_bytes(g, collect(tw, c, E))
    check_collect(c, g, E)
    return g


# ---- 1. the probe rows of tests/device_env_matrix.TABLE, rebuilt with fp16x2=True -------------------------------------------------------------
@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("module", PROBE_ROWS)
def test_probe_rows(tw, module, E):
    c = _probe_case(module)
    assert c.env.fp16x2
    run_case(tw, c, E)


# ---- 2. widths: everything padding, no width a multiple of 32 or 16, the widest layers, no common layer ---------------------------------------
@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("key", sorted(WIDTHS))
def test_widths(tw, key, E):
    run_case(tw, _width_case(key), E)


# ---- 3. persistent lanes: one and two resident workgroups ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
def test_persistent_lanes(tw, groups):
    from twisterl_amd import _lib
    c = _width_case("no_multiple")
    E = 100
    with _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups):
        g = collect(tw, c, E)
        info = assert_launch(c, 1, groups)
        assert g.stats["rollout_blocks"] == groups, info
    with _lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1):
        p = collect(tw, c, E)
        assert_launch(c, 0, (E + 15) // 16)
    same_bytes(g, p)
    if groups == 1:
        check_collect(c, g, E)


# ---- 4. more than four actions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", WIDE_ROWS)
def test_wide(tw, module):
    c = _wide_case(module)
    assert c.env.fp16x2 and c.A > 4
    run_case(tw, c, 100)


# ---- 5. the exactness probe ------------------------------------------------------------------------------------------------------------------------
def _oracle_loop(O, proto, policy, E, seed, diff, arith):
    """tests/var_obs_util.oracle_ppo_loop with the forward's arithmetic as a parameter, episodes in index order."""
    A = policy.n_actions
    out = SimpleNamespace(obs=[], logits=[], values=[], rewards=[], actions=[], ep_len=[], advs=[], rets=[], masks=[])
    for ep in range(E):
        e = proto.copy()
        e.seed_episode(seed, ep)
        e.reset(diff)
        lg_l, v_l, r_l = [], [], []
        t = 0
        while True:
            obs, masks = [int(x) for x in e.observe()], [bool(m) for m in e.masks()]
            lg, v = policy.forward(obs, masks, perm=-1, arith=arith)
            act = O.sample_from_logits(lg, _uniforms(O, seed, ep, t, A), det_log=True)
            out.obs.append(obs); out.masks.append(masks); out.actions.append(act)
            lg_l.append(lg); v_l.append(v); r_l.append(np.float32(e.value()))
            if e.is_final():
                break
            e.next(act)
            t += 1
        advs, rets = O.gae(r_l, v_l, GAMMA, LAM)
        out.logits += lg_l; out.values += v_l; out.rewards += r_l; out.advs += list(advs); out.rets += list(rets); out.ep_len.append(len(v_l))
    return out


def test_exactness_probe(tw):
    O = _oracle()
    c = _gw_case("gw3_exact", S.exact_arrays())
    assert_in_range(c)
    E = 100
    # on the CPU, before the GPU is touched: along the oracle's f32 collect the numpy restatement of the spec gives the oracle's bits
    o = _oracle_loop(O, host_env(c.env), c.op, E, c.seed, c.diff, O.ARITH_CHAIN)
    obs, masks = np.asarray(o.obs, np.int64), np.asarray(o.masks, bool)
    lg, v = S.forward(c.arrs, (), (), obs, masks, np.full(len(obs), -1))
    assert np.array_equal(f32_bits(lg), f32_bits(np.asarray(o.logits, np.float32))) and np.array_equal(f32_bits(v), f32_bits(np.asarray(o.values, np.float32)))
    l64, v64 = ref64.forward_f64(c.arrs, (), (), obs, masks, np.full(len(obs), -1))
    assert np.array_equal(lg.astype(np.float64), l64) and np.array_equal(v.astype(np.float64), v64)
    o16 = _oracle_loop(O, host_env(c.env), c.op, E, c.seed, c.diff, O.ARITH_F16)
    assert len(set(o.ep_len)) >= 3 and len(set(o.actions)) >= 2
    # the GPU: bit for bit the oracle's f32 collect
    g = collect(tw, c, E)
    assert_launch(c, 0, (E + 15) // 16)
    a = g.to_numpy()
    assert np.array_equal(a["ep_len"], np.asarray(o.ep_len, a["ep_len"].dtype))
    assert np.array_equal(a["obs"].astype(np.int64), obs) and np.array_equal(a["actions"].astype(np.int64), np.asarray(o.actions, np.int64))
    for k in ("logits", "values", "rewards", "advs", "rets"):
        assert np.array_equal(f32_bits(a[k]), f32_bits(np.asarray(getattr(o, k), np.float32).reshape(a[k].shape))), k
    # ... and not the rounded mode's: the lo terms are really used
    n = min(len(o16.values), len(o.values))
    assert len(o16.values) != len(o.values) or not np.array_equal(f32_bits(a["logits"]), f32_bits(np.asarray(o16.logits, np.float32).reshape(a["logits"].shape)))
    assert not np.array_equal(f32_bits(a["values"][:n]), f32_bits(np.asarray(o16.values, np.float32)[:n]))
    assert check_collect(c, g, E) == 0.0
    same_bytes(g, collect(tw, c, E, precision="fp32"))


# ---- 6. the range ----------------------------------------------------------------------------------------------------------------------------------
def _with_head_weight(arrs, w):
    """The GridWorld policy `arrs` with one weight of the action head's last layer set to w (its output is never split: only the
    weight's own range is in question)."""
    emb, eb, common, action, value = arrs
    wl, bl, r = action[-1]
    wl = np.array(wl, np.float32, copy=True)
    wl[5] = np.float32(w)
    return (emb, eb, common, action[:-1] + [(wl, bl, r)], value)


def _state_dict(arrs):
    import torch
    we, be, cs, as_, vs = arrs
    state = {"embeddings.weight": torch.tensor(we.T.copy()).cuda(), "embeddings.bias": torch.tensor(be).cuda()}
    for name, layers in (("common", cs), ("action", as_), ("value", vs)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = torch.tensor(np.asarray(wl).reshape(-1, len(bl)).T.copy()).cuda()
            state[f"{name}.{2 * i}.bias"] = torch.tensor(np.asarray(bl)).cuda()
    return state


def test_a_weight_of_4094_runs_the_split_kernel(tw, capfd):
    c = _gw_case("gw3_w4094", _with_head_weight(S.width_arrays("no_multiple"), 4094.0))
    run_case(tw, c, 40)
    assert "fp16x2" not in capfd.readouterr().err


def _assert_falls_back(tw, c, capfd, E=40):
    capfd.readouterr()
    g = collect(tw, c, E)
    assert_launch(c, 0, (E + 15) // 16, nw=0)                                # the f32 kernel
    err = capfd.readouterr().err
    assert err.count(FALLBACK_LINE) == 1 and err.count("\n") == 1, err
    same_bytes(g, collect(tw, c, E, precision="fp32"))
    assert capfd.readouterr().err == ""
    return g


@pytest.mark.parametrize("w", [4095.0, -4095.0, 5000.0, float("nan")])
def test_a_weight_outside_the_range_gives_the_fp32_collect(tw, capfd, w):
    base = S.width_arrays("no_multiple")
    c = _gw_case("gw3_wbad", _with_head_weight(base, w))
    _assert_falls_back(tw, c, capfd)
    # back into range: the split kernel runs again, on the image of the new weights
    c.gp.update_from_torch(_state_dict(base))
    g = collect(tw, c, 40)
    assert_launch(c, 0, 3)
    assert capfd.readouterr().err == ""
    same_bytes(g, collect(tw, _width_case("no_multiple"), 40))


def test_an_activation_outside_the_range_gives_the_fp32_collect(tw, capfd):
    emb, eb, common, action, value = S.width_arrays("no_multiple")
    # an embedding output of -5000 (no ReLU behind the embedding)
    eb2 = np.array(eb, np.float32, copy=True)
    eb2[3] = np.float32(-5000.0)
    arrs = (emb, eb2, common, action, value)
    seq = lambda ls: tw.nn.Sequential([tw.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    gp = tw.nn.Policy(tw.nn.EmbeddingBag(emb.tolist(), eb2.tolist(), False, [emb.shape[0]], 0), seq(common), seq(action), seq(value), [], [])
    _assert_falls_back(tw, _gw_case("gw3_embbad", arrs, gp=gp), capfd)
    # a hidden activation of about 5000 (a common layer's bias)
    w0, b0, r0 = common[0]
    b1 = np.array(b0, np.float32, copy=True)
    b1[7] = np.float32(5000.0)
    _assert_falls_back(tw, _gw_case("gw3_hidbad", (emb, eb, [(w0, b1, r0)] + common[1:], action, value)), capfd)


# ---- 7. after Policy.update_from_torch the image is packed again ------------------------------------------------------------------------------------
def test_update_from_torch_repacks_the_image(tw):
    emb, common = 36, (40, 20)
    mk = lambda seed: make_deep_policy_arrays_obs(GW.obs_size, seed=seed, emb=emb, common=common, n_actions=4, scale=2.0)
    old, new = mk(71), mk(72)
    c_old, c_new = _gw_case("gw3_update_old", old), _gw_case("gw3_update_new", new)
    E = 100
    before = collect(tw, c_old, E)
    c_old.gp.update_from_torch(_state_dict(new))
    after = collect(tw, c_old, E)
    assert_launch(c_old, 0, (E + 15) // 16)
    same_bytes(after, collect(tw, c_new, E))
    assert not np.array_equal(before.to_numpy()["logits"][:8], after.to_numpy()["logits"][:8])
    check_collect(c_new, after, E)


# ---- 8. the fp16x2 carve (the f32 segments and the split image behind them) on pre-filled workspace memory -------------------------------------------
@pytest.mark.parametrize("which", ["gridworld", "probe_o26a1v", "wideo16a16"])
def test_no_result_depends_on_what_the_workspace_held(tw, which):
    """The same bytes with every workspace and result word pre-set to 0xFFFFFFFF (a NaN in either half of the image), 1 and 0, and --
    hook off -- on the leftovers of the same call under another policy's weights."""
    from twisterl_amd import _lib
    c = {"gridworld": lambda: _width_case("no_multiple"), "probe_o26a1v": lambda: _probe_case("probe_o26a1v"),
         "wideo16a16": lambda: _wide_case("wideo16a16")}[which]()
    E = 100
    want = collect(tw, c, E)
    assert_launch(c, 0, (E + 15) // 16)
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            same_bytes(want, collect(tw, c, E))
            assert_launch(c, 0, (E + 15) // 16)
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(make_deep_policy_arrays_obs(c.arrs[0].shape[0], seed=5, emb=64, common=(96, 48), n_actions=c.A,
                                                                                         scale=3.0), *c.tw)})
    collect(tw, other, E)
    assert_launch(c, 0, (E + 15) // 16)
    same_bytes(want, collect(tw, c, E))


# ---- 9. on a caller's stream, the null stream kept busy ----------------------------------------------------------------------------------------------
def test_on_a_callers_stream(tw):
    import torch
    from tests import stream_util as su
    from twisterl_amd import _lib
    c = _width_case("no_multiple")
    E = 100
    want = collect(tw, c, E)
    stream = su.independent_stream()
    try:
        with _lib.library_stream(stream):
            busy = su.delay(su.null_stream(), 40.0)
            got = collect(tw, c, E)
            ran_beside = not busy.query()
            assert_launch(c, 0, (E + 15) // 16)
            host = {k: v.copy() for k, v in got.to_numpy().items()}
    finally:
        torch.cuda.synchronize()
    assert ran_beside, "the collect on the caller's stream waited for the null stream's work"
    w = want.to_numpy()
    assert sorted(w) == sorted(host)
    for k in w:
        assert w[k].tobytes() == host[k].tobytes(), k


# ---- 10. what the split kernel does not take keeps its message ---------------------------------------------------------------------------------------
def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def test_refusals(tw):
    from twisterl_amd import _lib
    from tests.util import make_policy_arrays_obs
    c = _width_case("no_multiple")
    ppo = lambda env, gp, prec: tw.collector.PPOCollector(40, GAMMA, LAM, 4, precision=prec).collect(env, gp, seed=1)
    default_env = gridworld(3, max_steps=GW.max_steps, difficulty=GW.diff, max_records=GW.max_steps + 1)
    assert not default_env.fp16x2
    want = (RuntimeError, "tw_ppo_collect_env: f32 only")
    assert _message(lambda: ppo(default_env, c.gp, "fp16x2")) == want                     # a module built without fp16x2=True
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    mfma = amd_policy(make_policy_arrays_obs(GW.obs_size, seed=3, emb=64, hidden=64, n_actions=4))
    assert _message(lambda: ppo(c.env, mfma, "fp16x2")) == want                            # an MFMA-shape policy
    az = lambda env: tw.collector.AZCollector(16, 4, 1.41, 1, 4, precision="fp16x2").collect(env, c.gp, seed=1)
    assert _message(lambda: az(c.env)) == _message(lambda: az(default_env)) == (RuntimeError, "tw_az_collect_env: f32 only")
    ev = lambda env: tw.collector.evaluate(env, c.gp, 8, True, 1, 0, 1, 1.41, 1, 1, precision="fp16x2")
    assert _message(lambda: ev(c.env)) == _message(lambda: ev(default_env))
    assert "f32 only" in _message(lambda: ev(c.env))[1]
    so = lambda env: tw.collector.solve(env, c.gp, True, 1, 0, 1.41, 1, seed=1, precision="fp16x2")
    assert _message(lambda: so(c.env)) == _message(lambda: so(default_env))
    assert "f32 only" in _message(lambda: so(c.env))[1]
    ok = ppo(c.env, c.gp, "fp32")                                                          # the f32 kernel of the fp16x2 module is the f32 kernel
    info = _lib.debug_last_launch()
    assert (info["family"], info["nw"], info["nc"]) == (_lib.TW_KERNEL_ROLLOUT_BIG, 0, 9), info
    same_bytes(ok, ppo(default_env, c.gp, "fp32"))
    ok16 = ppo(c.env, c.gp, "fp16")                                                        # ... and its fp16 kernel the fp16 kernel
    assert _lib.debug_last_launch()["nw"] == 16
    assert not np.array_equal(ok16.to_numpy()["logits"], ok.to_numpy()["logits"])


def test_the_deepest_policy_runs_in_the_split_kernel(tw):
    """EngineV16x2 takes at most 24 layers (engine16_takes, the fp16 collect's own rule) and a deeper policy would go the host-stepped
    way -- but the library builds none: tw_policy_create refuses a ninth layer in a stack, so 8 + 8 + 8 is the deepest policy there is.
    That one runs in the split kernel (every entry of the engine's layer-offset table in use), and the ninth layer is refused."""
    with pytest.raises(Exception, match="at most 8 layers per stack"):
        amd_policy(make_deep_policy_arrays_obs(GW.obs_size, seed=9, emb=32, common=(32,) * 9, n_actions=4))._handle()   # (uploaded on first use)
    rng_arrs = make_deep_policy_arrays_obs(GW.obs_size, seed=9, emb=32, common=(32,) * 8, policy_layers=(16,) * 7, value_layers=(16,) * 7, n_actions=4,
                                           scale=0.3)       # (the weight-norm ceiling grows with every layer: 0.85 at this scale)
    c = _gw_case("gw3_24_layers", rng_arrs)
    run_case(tw, c, 40)
