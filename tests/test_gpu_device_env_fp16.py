"""GPU: PPOCollector(precision="fp16").collect of device environments -- rollout_env16_kernel over EngineV16
(twisterl_amd/csrc/tw_engine_generic16.hpp: every Linear of a generic policy on v_mfma_f32_16x16x32_f16), modules built with
build_device_env(..., fp16=True).

Every collect (merge_order=False) is held to seven things: (1) tw_debug_last_launch names the f16 kernel (family ROLLOUT_BIG, nt 1, the
row's engine width, nw 16, persist as expected); (2) two collects give the same bytes; (3) the GPU's own actions replayed through the
module's HOST code give its obs ids (0xFFFF slots included), rewards, masks (-1e10 positions), ep_len and twist draws bit for bit;
(4) every action is oracle.sample_from_logits of the GPU's own logits and the spec's uniforms; (5) advs / rets are oracle.gae of the
GPU's own rewards and values, bit for bit; (6) every logit and value is within tests/ref64.forward_f64_bound(mode="fp16") of float64 --
an a-priori bound that holds for any conforming f16-input forward with f32 accumulation, valid while no activation reaches 65504,
which a weight-norm ceiling shows on the CPU BEFORE the GPU is touched; (7) the largest |gpu - oracle ARITH_F16| is recorded, not gated
(it depends on the weights): printed, and appended to the file TW_FP16_RECORD names.

The exactness probe needs no bound: integer-valued binary16 operands and half-integer activations below 1024 make every sum exact in
f32 in any order, so the GPU must equal the oracle's ARITH_F16 collect bit for bit -- and differ from ARITH_CHAIN, which shows that
the rounding to binary16 really happens."""
import functools
import json
import os
import signal
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ref64
from tests.device_env_matrix import BY_MODULE as PROBE_ROWS_BY_MODULE, GAMMA, LAM, PROBE_HPP, engine_nc, host_env
from tests.device_env_matrix import policy_arrays as probe_arrays, twists as probe_twists
from tests.device_env_util import GRIDWORLD_HPP, gridworld
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE, policy_arrays as wide_arrays, twists as wide_twists
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs, oracle_policy

pytestmark = pytest.mark.gpu

PROBE_ROWS = ("probe_o1a1", "probe_o4a2", "probe_o5a3v", "probe_o10a4v", "probe_o16a3", "probe_o17a2", "probe_o26a1v", "probe_o64a4s")
WIDE_ROWS = ("wideo17a17", "wideo16a16")           # the head's second tile holds one row | deep heads and twists
EPISODES = (40, 100)                               # 2.5 and 6.25 workgroups of 16 columns
GW = SimpleNamespace(name="gridworld3x3_fp16", type="tw_examples::GridWorld3x3", n_obs=9, obs_size=81, A=4, max_steps=12, diff=3, seed=41)
# GridWorld 3 x 3 policies: (embedding, common layers)
WIDTHS = {"all_padding": (4, (4,)), "no_multiple": (36, (40, 20)), "wide": (512, (512, 272)), "no_common": (32, ())}
F16_MAX = 65504.0
NO_ID = 0xFFFF


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16 device-environment test exceeded its time limit")
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
    """Every fp16 module of this file, built once per session side by side, AT MOST 16 AT A TIME -> {name: path}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    jobs = [(PROBE_HPP, PROBE_ROWS_BY_MODULE[m].alias, m + "_fp16", {"fp16": True}) for m in PROBE_ROWS]
    jobs += [(WIDE_ROWS_BY_MODULE[m].header, WIDE_ROWS_BY_MODULE[m].type, m + "_fp16", {"fp16": True, "wide": True}) for m in WIDE_ROWS]
    jobs += [(GRIDWORLD_HPP, GW.type, GW.name, {"fp16": True})]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(j[0], j[1], j[2], **j[3]), jobs))
    return {j[2]: p for j, p in zip(jobs, paths)}


# ---- a case: environment, policies, what the replay needs ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe_case(module):
    from twisterl_amd.env import DeviceEnv
    r = PROBE_ROWS_BY_MODULE[module]
    name = module + "_fp16"
    env = DeviceEnv(build_all()[name], name, [r.obs_size, r.max_steps, r.diff, -1], max_records=r.max_steps + 1)
    arrs, tws = probe_arrays(module), probe_twists(module)
    return SimpleNamespace(name=module, env=env, arrs=arrs, tw=tws, gp=amd_policy(arrs, *tws), op=oracle_policy(_oracle(), arrs, *tws),
                           n_obs=r.n_obs, A=r.A, var=r.var, diff=r.diff, seed=r.seed, offset=r.offset, nc=engine_nc(r.n_obs))


@functools.lru_cache(maxsize=None)
def _wide_case(module):
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE[module]
    name = module + "_fp16"
    env = DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)
    arrs, tws = wide_arrays(module), wide_twists(module)
    return SimpleNamespace(name=module, env=env, arrs=arrs, tw=tws, gp=amd_policy(arrs, *tws), op=oracle_policy(_oracle(), arrs, *tws),
                           n_obs=r.n_obs, A=r.A, var=r.var, diff=r.diff, seed=r.seed, offset=0, nc=engine_nc(r.n_obs))


def _gw_env():
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[GW.name], GW.name, [3, 3, GW.max_steps, GW.diff], max_records=GW.max_steps + 1)


def _gw_case(name, arrs):
    return SimpleNamespace(name=name, env=_gw_env(), arrs=arrs, tw=((), ()), gp=amd_policy(arrs), op=oracle_policy(_oracle(), arrs),
                           n_obs=GW.n_obs, A=GW.A, var=False, diff=GW.diff, seed=GW.seed, offset=0, nc=9)


@functools.lru_cache(maxsize=None)
def _width_case(key):
    emb, common = WIDTHS[key]
    return _gw_case("gw3_" + key, make_deep_policy_arrays_obs(GW.obs_size, seed=60 + len(key), emb=emb, common=common, n_actions=4, scale=2.0))


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------
def activation_ceiling(arrs, n_obs):
    """An upper bound of every activation the forward can produce, from the weights alone (no state, no GPU): the embedding's output
    is at most n_obs x the largest table entry plus the bias; a layer's at most max over outputs of sum |w| x the input's bound + |b|."""
    emb, eb, common, action, value = arrs
    x = n_obs * float(np.abs(emb).max()) + float(np.abs(eb).max())
    top = x

    def through(layers, x, top):
        for w, b, _ in layers:
            W = np.abs(np.asarray(w, np.float64).reshape(-1, len(b)))
            x = float((W.sum(axis=0) * x + np.abs(np.asarray(b, np.float64))).max())
            top = max(top, x)
        return x, top

    x, top = through(common, x, top)
    for head in (action, value):
        _, t2 = through(head[:-1], x, top)
        top = max(top, t2)
    return top


def collect(tw, c, E, **kw):
    kw.setdefault("episode_offset", c.offset)
    return tw.collector.PPOCollector(E, GAMMA, LAM, 4, merge_order=False, precision="fp16", **kw).collect(c.env, c.gp, seed=c.seed)


def assert_f16_launch(c, persist, blocks=None):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["nw"], info["persist"], info["threads"]) == \
        (_lib.TW_KERNEL_ROLLOUT_BIG, 1, c.nc, 16, persist, 256), info
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


_RECORDED = {}


def _record(case, E, worst, n_records):
    _RECORDED[(case, E)] = worst
    print(f"[fp16] {case} E={E}: {n_records} records, max |gpu - oracle ARITH_F16| = {worst:.3e}")
    path = os.environ.get("TW_FP16_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"what": "max_abs_deviation_from_oracle_arith_f16", "case": case, "episodes": E, "records": n_records,
                                "value": worst}) + "\n")


def check_collect(c, g, E):
    """Checks 3 - 7 of the module docstring on one collect (merge_order=False); -> the largest deviation from the oracle's ARITH_F16."""
    O = _oracle()
    a = g.to_numpy()
    L = a["ep_len"].astype(np.int64)
    assert L.size == E and int(L.sum()) == a["logits"].shape[0] and a["logits"].shape[1] == c.A and a["obs"].shape[1] == c.n_obs
    starts = np.concatenate([[0], np.cumsum(L)])
    n_perms = len(c.tw[0])
    hproto = host_env(c.env)
    obs_rows, mask_rows, perm_rows = [], [], []
    worst = 0.0
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
            lo, vo = c.op.forward(ids, masks, perm=perm, arith=O.ARITH_F16)
            worst = max(worst, float(np.max(np.abs(lg.astype(np.float64) - np.asarray(lo, np.float64)))), abs(float(a["values"][s + t]) - float(vo)))
            obs_rows.append(ids + [-1] * (c.n_obs - len(ids))); mask_rows.append(masks); perm_rows.append(perm)
            final = env.is_final()
            assert final == (t == n - 1), (c.name, e, t, n)
            if not final:
                env.next(act)
        advs, rets = O.gae(a["rewards"][s:s + n], a["values"][s:s + n], GAMMA, LAM)
        assert np.array_equal(f32_bits(advs), f32_bits(a["advs"][s:s + n])) and np.array_equal(f32_bits(rets), f32_bits(a["rets"][s:s + n])), (c.name, e)
    obs_arr, mask_arr, perm_arr = np.asarray(obs_rows, np.int64), np.asarray(mask_rows, bool), np.asarray(perm_rows, np.int64)
    m0, m1 = ref64.max_activations(c.arrs, c.tw[0], c.tw[1], obs_arr, perm_arr)
    assert max(m0, m1) < F16_MAX
    l64, v64, el, ev = ref64.forward_f64_bound(c.arrs, c.tw[0], c.tw[1], obs_arr, mask_arr, perm_arr, "fp16")
    dl = np.abs(a["logits"].astype(np.float64) - l64)
    assert (dl[mask_arr] <= el[mask_arr]).all(), (c.name, float((dl - el)[mask_arr].max()), float(dl[mask_arr].max()), float(el[mask_arr].min()))
    dv = np.abs(a["values"].astype(np.float64) - v64)
    assert (dv <= ev).all(), (c.name, float((dv - ev).max()), float(dv.max()))
    _record(c.name, E, worst, int(L.sum()))
    return worst


def run_case(tw, c, E):
    assert activation_ceiling(c.arrs, c.n_obs) < F16_MAX                 # (on the CPU, before the GPU is touched)
    g = collect(tw, c, E)
    assert_f16_launch(c, 0, (E + 15) // 16)
    assert g.stats["rollout_blocks"] == (E + 15) // 16 and g.stats["rollout_threads"] == 256
    same_bytes(g, collect(tw, c, E))
    check_collect(c, g, E)
    return g


# ---- 1. the probe rows of tests/device_env_matrix.TABLE, rebuilt with fp16=True ---------------------------------------------------------------
@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("module", PROBE_ROWS)
def test_probe_rows(tw, module, E):
    c = _probe_case(module)
    assert c.env.fp16
    run_case(tw, c, E)


# ---- 2. widths: everything padding, no width a multiple of 32 or 16, the widest layers, no common layer ---------------------------------------
@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("key", sorted(WIDTHS))
def test_widths(tw, key, E):
    run_case(tw, _width_case(key), E)


# ---- 3. persistent lanes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [100, 1000])
def test_persistent_lanes(tw, E):
    import twisterl_amd
    from twisterl_amd import _lib
    c = _width_case("no_multiple")
    cus = int(twisterl_amd.device_info()["compute_units"])
    g = collect(tw, c, E, reserve_cus=cus - 1)
    info = assert_f16_launch(c, 1)
    assert 1 <= info["blocks"] and info["blocks"] * 16 < E and g.stats["rollout_blocks"] == info["blocks"], info
    with _lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1):
        p = collect(tw, c, E, reserve_cus=cus - 1)
        assert_f16_launch(c, 0, (E + 15) // 16)
    same_bytes(g, p)
    if E == 100:
        check_collect(c, g, E)


# ---- 4. more than four actions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", WIDE_ROWS)
def test_wide(tw, module):
    c = _wide_case(module)
    assert c.env.fp16 and c.A > 4
    run_case(tw, c, 100)


# ---- 5. the exactness probe ------------------------------------------------------------------------------------------------------------------------
def _exact_arrays():
    """Table entries and weights: 0, or a small integer plus 2^-12 away from zero (binary16 rounds it to the integer: its spacing from
    1 up is at least 2^-10); biases: half-integers, which stay f32."""
    rng = np.random.default_rng(2024)
    tiny = np.float32(2.0 ** -12)

    def ints(shape, p, hi):
        v = rng.integers(1, hi + 1, size=shape).astype(np.float32) * rng.choice(np.float32([-1.0, 1.0]), size=shape)
        v = v + np.sign(v) * tiny
        return np.where(rng.random(shape) < p, v, np.float32(0.0)).astype(np.float32)

    def half(n, lo, hi):
        return (rng.integers(lo, hi, size=n).astype(np.float32) + np.float32(0.5)).astype(np.float32)

    def lin(i, o, relu, p, hi):
        return (np.ascontiguousarray(ints((i, o), p, hi)).reshape(-1), half(o, -2, 2), relu)

    emb = ints((GW.obs_size, 32), 1.0, 2)
    return (emb, half(32, -2, 2), [lin(32, 32, True, 0.25, 2), lin(32, 16, True, 0.25, 1)], [lin(16, 4, False, 0.5, 1)], [lin(16, 1, False, 0.5, 1)])


def _r16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def _oracle_loop(O, proto, policy, E, seed, n_obs, diff, arith):
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
    arrs = _exact_arrays()
    c = _gw_case("gw3_exact", arrs)
    E = 100
    # on the CPU, before the GPU is touched: along the oracle's ARITH_F16 collect every activation is an integer or a half-integer below 1024
    o = _oracle_loop(O, host_env(c.env), c.op, E, c.seed, c.n_obs, c.diff, O.ARITH_F16)
    emb, eb, common, action, value = arrs
    obs = np.asarray(o.obs, np.int64)
    x = np.maximum(_r16(emb)[obs].sum(axis=1) + np.asarray(eb, np.float64), 0.0)
    acts = [x]
    for w, b, _ in common:
        x = np.maximum(_r16(x) @ _r16(w).reshape(-1, len(b)) + np.asarray(b, np.float64), 0.0)
        acts.append(x)
    for h in acts:
        assert np.array_equal(2 * h, np.round(2 * h)) and float(np.abs(h).max()) < 1024 and np.array_equal(_r16(h), h)
    assert float(acts[-1].max()) > 0.0 and float(acts[1].max()) > 0.0
    la = _r16(acts[-1]) @ _r16(action[0][0]).reshape(-1, 4) + np.asarray(action[0][1], np.float64)
    lv = (_r16(acts[-1]) @ _r16(value[0][0]).reshape(-1, 1) + np.asarray(value[0][1], np.float64)).sum(axis=1)
    want = np.where(np.asarray(o.masks, bool), la, -1e10).astype(np.float32)
    assert np.array_equal(f32_bits(want), f32_bits(np.asarray(o.logits, np.float32)))          # the oracle's ARITH_F16 is this exact forward
    assert np.array_equal(f32_bits(lv.astype(np.float32)), f32_bits(np.asarray(o.values, np.float32)))
    chain = np.asarray([c.op.forward(ob, mk, perm=-1, arith=O.ARITH_CHAIN)[0] for ob, mk in zip(o.obs, o.masks)], np.float32)
    assert (chain != np.asarray(o.logits, np.float32)).any(), "ARITH_CHAIN and ARITH_F16 agree everywhere: the rounding would not show"
    assert len(set(o.ep_len)) >= 3 and len(set(o.actions)) >= 2
    # the GPU: bit for bit the oracle's collect
    g = collect(tw, c, E)
    assert_f16_launch(c, 0, (E + 15) // 16)
    a = g.to_numpy()
    assert np.array_equal(a["ep_len"], np.asarray(o.ep_len, a["ep_len"].dtype))
    assert np.array_equal(a["obs"].astype(np.int64), obs) and np.array_equal(a["actions"].astype(np.int64), np.asarray(o.actions, np.int64))
    for k in ("logits", "values", "rewards", "advs", "rets"):
        assert np.array_equal(f32_bits(a[k]), f32_bits(np.asarray(getattr(o, k), np.float32).reshape(a[k].shape))), k
    assert check_collect(c, g, E) == 0.0


# ---- 6. after Policy.update_from_torch the image is packed again ------------------------------------------------------------------------------------
def test_update_from_torch_repacks_the_image(tw):
    import torch
    emb, common = 36, (40, 20)
    mk = lambda seed: make_deep_policy_arrays_obs(GW.obs_size, seed=seed, emb=emb, common=common, n_actions=4, scale=2.0)
    old, new = mk(71), mk(72)
    c_old, c_new = _gw_case("gw3_update_old", old), _gw_case("gw3_update_new", new)
    E = 100
    before = collect(tw, c_old, E)
    we, be, cs, as_, vs = new
    state = {"embeddings.weight": torch.tensor(we.T.copy()).cuda(), "embeddings.bias": torch.tensor(be).cuda()}
    for name, layers in (("common", cs), ("action", as_), ("value", vs)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = torch.tensor(np.asarray(wl).reshape(-1, len(bl)).T.copy()).cuda()
            state[f"{name}.{2 * i}.bias"] = torch.tensor(np.asarray(bl)).cuda()
    c_old.gp.update_from_torch(state)
    after = collect(tw, c_old, E)
    assert_f16_launch(c_old, 0, (E + 15) // 16)
    fresh = collect(tw, c_new, E)
    same_bytes(after, fresh)
    assert not np.array_equal(before.to_numpy()["logits"][:8], after.to_numpy()["logits"][:8])
    check_collect(c_new, after, E)


# ---- 6b. the fp16 carve (the f32 segments and the weight image behind them) on pre-filled workspace memory ------------------------------------------
@pytest.mark.parametrize("which", ["gridworld", "probe_o26a1v", "wideo16a16"])
def test_no_result_depends_on_what_the_workspace_held(tw, which):
    """As tests/test_gpu_memory_matrix.py holds the other carves: the same bytes with every workspace word pre-set to 0xFFFFFFFF (a NaN
    in either half of the image), 1 and 0, and -- hook off -- on the leftovers of the same call under another policy's weights."""
    from twisterl_amd import _lib
    c = {"gridworld": lambda: _width_case("no_multiple"), "probe_o26a1v": lambda: _probe_case("probe_o26a1v"),
         "wideo16a16": lambda: _wide_case("wideo16a16")}[which]()
    E = 100
    want = collect(tw, c, E)
    assert_f16_launch(c, 0, (E + 15) // 16)
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            same_bytes(want, collect(tw, c, E))
            assert_f16_launch(c, 0, (E + 15) // 16)
    # another policy of other widths leaves its own image and activations behind; then the first again, hook off
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(make_deep_policy_arrays_obs(c.arrs[0].shape[0], seed=5, emb=64, common=(96, 48), n_actions=c.A,
                                                                                         scale=3.0), *c.tw)})
    collect(tw, other, E)
    assert_f16_launch(c, 0, (E + 15) // 16)
    same_bytes(want, collect(tw, c, E))


# ---- 7. what the f16 kernel does not take keeps its message -----------------------------------------------------------------------------------------
def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def test_refusals(tw):
    from twisterl_amd import _lib
    c = _width_case("no_multiple")
    ppo = lambda env, gp, prec: tw.collector.PPOCollector(40, GAMMA, LAM, 4, precision=prec).collect(env, gp, seed=1)
    default_env = gridworld(3, max_steps=GW.max_steps, difficulty=GW.diff, max_records=GW.max_steps + 1)
    assert not default_env.fp16
    want = (RuntimeError, "tw_ppo_collect_env: f32 only")
    assert _message(lambda: ppo(default_env, c.gp, "fp16")) == want                       # a module built without fp16=True
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    from tests.util import make_policy_arrays_obs
    mfma = amd_policy(make_policy_arrays_obs(GW.obs_size, seed=3, emb=64, hidden=64, n_actions=4))
    assert _message(lambda: ppo(c.env, mfma, "fp16")) == want                              # an MFMA-shape policy
    assert _message(lambda: ppo(default_env, mfma, "fp16")) == want
    assert _message(lambda: ppo(c.env, c.gp, "fp16x2")) == want                            # the split mode
    az = lambda env: tw.collector.AZCollector(16, 4, 1.41, 1, 4, precision="fp16").collect(env, c.gp, seed=1)
    assert _message(lambda: az(c.env)) == _message(lambda: az(default_env)) == (RuntimeError, "tw_az_collect_env: f32 only")
    ok = ppo(c.env, c.gp, "fp32")                                                          # and the f32 kernel of the fp16 module is the f32 kernel
    info = _lib.debug_last_launch()
    assert (info["family"], info["nw"], info["nc"]) == (_lib.TW_KERNEL_ROLLOUT_BIG, 0, 9), info
    same_bytes(ok, ppo(default_env, c.gp, "fp32"))
