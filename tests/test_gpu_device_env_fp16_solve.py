"""GPU: collector.evaluate / collector.solve of device environments with precision="fp16" -- solve_env16_kernel over EngineV16
(twisterl_amd/csrc/tw_rollout_env.hpp, tw_engine_generic16.hpp), modules built with build_device_env(..., fp16_solve=True).

Evaluate returns two means and no logits, so nothing can be replayed, and an a-priori float64 bound of the logits is wider than the
gaps between them for policies of realistic width.  Two tiers:

A  EXACT ARITHMETIC.  Table entries and weights are small integers plus 2^-12 (binary16 rounds it away), biases half-integers, the
   density such that every activation along the oracle's own ARITH_F16 trajectories is an integer or a half-integer below 1024 --
   asserted on the CPU before the GPU is touched.  Every sum is then exact in any order, and every attempt's (success, total, n_steps)
   (tw_debug_last_attempts) must be bit for bit the oracle's: oracle.solve_env(arith=ARITH_F16) over the module's host code, attempt
   by attempt; so must evaluate's two means and solve's ((success, reward), actions).
B  GENERAL WEIGHTS, gated where float64 decides.  Along the oracle's ARITH_F16 attempt every step's probabilities are enclosed by
   ref64.predict_f64 +- ref64.prob_bound(ref64.forward_f64_bound(mode="fp16")); a deterministic step is decided when the chosen
   action's lower end is above every other upper end, a sampled one when every comparison of the weighted sample has the same outcome
   at both ends of the intervals (f32 rounding of the A additions and the product added).  An attempt of decided steps only is what
   ANY conforming implementation plays: there the GPU must equal the oracle bit for bit; the others are not compared, and at most a
   quarter of a case's attempts may be such (asserted on the CPU first).

Then what the kernel does not take: the messages and paths of before, exact."""
import ctypes as C
import functools
import signal
from types import SimpleNamespace

import numpy as np
import pytest

from tests import device_env_solve as D
from tests import ref64
from tests.device_env_matrix import BY_MODULE as PROBE_ROWS_BY_MODULE, PROBE_HPP, engine_nc, host_env
from tests.device_env_matrix import twists as probe_twists
from tests.device_env_util import GRIDWORLD_HPP
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE, twists as wide_twists
from tests.test_gpu_device_env_fp16 import GW, WIDTHS, activation_ceiling
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs, make_policy_arrays_obs, oracle_policy

pytestmark = pytest.mark.gpu

PROBE_ROWS = ("probe_o1a1", "probe_o5a3v", "probe_o17a2", "probe_o64a4s")      # NC 4, 9, 25, 64 (struct in scratch); observe_n; A < 4
WIDE_ROW = "wideo17a17"                                                       # A > 4: forward_head + env_predict_stream
SHAPES = ((40, 1), (34, 3))                       # episodes x searches: 2.5 and 6.4 workgroups of 16 columns, N not dividing 16
F16_MAX = 65504.0
C_UCB = 1.41
F32_ONLY = (RuntimeError, "solve: f32 only for this environment")
GW_S, GW_AZ, GW_16, GW_DEFAULT = "gridworld3x3_fp16s", "gridworld3x3_fp16s_az", "gridworld3x3_fp16", "gridworld3x3"


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16 evaluate / solve device-environment test exceeded its time limit")
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


@pytest.fixture(scope="module", autouse=True)
def O():
    from oracle import oracle as O_
    O_.build()
    O_.set_det_exp(True)                          # the soft-max's exp as the kernels compute it
    yield O_
    O_.set_det_exp(False)


@functools.lru_cache(maxsize=None)
def build_all():
    """Every module of this file, built once per session side by side, AT MOST 16 AT A TIME -> {name: path}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    jobs = [(PROBE_HPP, PROBE_ROWS_BY_MODULE[m].alias, m + "_fp16s", {"fp16_solve": True}) for m in PROBE_ROWS]
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    jobs += [(r.header, r.type, WIDE_ROW + "_fp16s", {"fp16_solve": True, "wide": True})]
    jobs += [(GRIDWORLD_HPP, GW.type, GW_S, {"fp16_solve": True}), (GRIDWORLD_HPP, GW.type, GW_AZ, {"fp16_solve": True, "search": True}),
             (GRIDWORLD_HPP, GW.type, GW_16, {"fp16": True}), (GRIDWORLD_HPP, GW.type, GW_DEFAULT, {})]
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(j[0], j[1], j[2], **j[3]), jobs))
    return {j[2]: p for j, p in zip(jobs, paths)}


# ---- exact policies -------------------------------------------------------------------------------------------------------------------------------
TINY = np.float32(2.0 ** -12)


def _ints(rng, shape, nonzero_per_output, hi, tiny=True):
    """0, or an integer of 1 .. hi of either sign (plus 2^-12 away from zero, which binary16 rounds away: its spacing from 1 up is at
    least 2^-10); on average `nonzero_per_output` entries per output column are not 0."""
    v = rng.integers(1, hi + 1, size=shape).astype(np.float32) * rng.choice(np.float32([-1.0, 1.0]), size=shape)
    if tiny:
        v = v + np.sign(v) * TINY
    p = min(1.0, nonzero_per_output / shape[0])
    return np.where(rng.random(shape) < p, v, np.float32(0.0)).astype(np.float32)


def _half(rng, n, lo, hi):
    return (rng.integers(lo, hi, size=n).astype(np.float32) + np.float32(0.5)).astype(np.float32)


def exact_arrays(obs_size, emb, common, policy_layers, value_layers, A, seed, emb_hi=1, k=6):
    """A policy in make_deep_policy_arrays_obs' format whose f16-input forward is exact: see the module docstring."""
    rng = np.random.default_rng(seed)

    def lin(i, o, relu):
        return (np.ascontiguousarray(_ints(rng, (i, o), k if relu else 3 * k, 1)).reshape(-1), _half(rng, o, -2, 2), relu)

    table = _ints(rng, (obs_size, emb), obs_size, emb_hi)
    be = _half(rng, emb, -2, 2)
    cs, w = [], emb
    for h in common:
        cs.append(lin(w, h, True)); w = h
    acts, wa = [], w
    for h in policy_layers:
        acts.append(lin(wa, h, True)); wa = h
    acts.append(lin(wa, A, False))
    vals, wv = [], w
    for h in value_layers:
        vals.append(lin(wv, h, True)); wv = h
    vals.append(lin(wv, 1, False))
    return (table, be, cs, acts, vals)


def _r16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def assert_exact_along(c, steps):
    """On the CPU: every activation the f16-input forward stores along `steps` (the oracle's ARITH_F16 trajectories) is an integer or a
    half-integer below 1024 that binary16 holds, every weight a binary16 integer; so any order of any f32 sum is exact."""
    emb, eb, common, action, value = c.arrs
    OP = np.asarray(c.tw[0], np.int64) if len(c.tw[0]) else None
    lay = lambda ls: [(_r16(w).reshape(-1, len(b)), np.asarray(b, np.float64)) for w, b, _ in ls]
    table, common16, heads16 = _r16(emb), lay(common), [lay(action[:-1]), lay(value[:-1])]
    acts_seen = 0.0
    for ids, _, perm, _u in steps:
        ids = np.asarray(ids, np.int64)
        if perm >= 0:
            ids = OP[perm][ids]
        x = np.maximum(table[ids].sum(axis=0) + np.asarray(eb, np.float64), 0.0)
        hs = [x]
        for w, b in common16:
            x = np.maximum(_r16(x) @ w + b, 0.0)
            hs.append(x)
        for head in heads16:
            y = x
            for w, b in head:
                y = np.maximum(_r16(y) @ w + b, 0.0)
                hs.append(y)
        for h in hs:
            assert np.array_equal(2 * h, np.round(2 * h)) and float(np.abs(h).max(initial=0.0)) < 1024 and np.array_equal(_r16(h), h), (c.name, float(np.abs(h).max()))
        acts_seen = max(acts_seen, float(hs[-1].max(initial=0.0)))
    for w in [emb] + [l[0] for ls in (common, action, value) for l in ls]:
        w16 = _r16(w)
        assert np.array_equal(w16, np.round(w16)) and float(np.abs(w16).max()) <= 2.0
    assert acts_seen > 0.0, "every last hidden activation is zero: the heads would be their biases"


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
def _case(name, env, arrs, tws, n_obs, A, diff, seed, offset=0):
    from oracle import oracle as O_
    return SimpleNamespace(name=name, env=env, arrs=arrs, tw=tws, gp=amd_policy(arrs, *tws), op=oracle_policy(O_, arrs, *tws), n_obs=n_obs, A=A,
                           diff=diff, seed=seed, offset=offset, nc=engine_nc(n_obs))


def _gw_env(module=GW_S):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[module], module, [3, 3, GW.max_steps, GW.diff], max_records=GW.max_steps + 1)


def _gw_case(name, arrs, module=GW_S):
    return _case(name, _gw_env(module), arrs, ((), ()), GW.n_obs, GW.A, GW.diff, GW.seed)


@functools.lru_cache(maxsize=None)
def _gw_exact(key):
    emb, common = WIDTHS[key]
    return _gw_case("gw3_exact_" + key, exact_arrays(GW.obs_size, emb, common, (), (), 4, seed=300 + len(key)))


@functools.lru_cache(maxsize=None)
def _probe_exact(module):
    from twisterl_amd.env import DeviceEnv
    r = PROBE_ROWS_BY_MODULE[module]
    name = module + "_fp16s"
    env = DeviceEnv(build_all()[name], name, [r.obs_size, r.max_steps, r.diff, -1], max_records=r.max_steps + 1)
    arrs = exact_arrays(r.obs_size, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=400 + r.seed)
    return _case(module + "_exact", env, arrs, probe_twists(module), r.n_obs, r.A, r.diff, r.seed, r.offset)


@functools.lru_cache(maxsize=None)
def _wide_exact():
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    name = WIDE_ROW + "_fp16s"
    env = DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)
    arrs = exact_arrays(r.obs_size, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=400 + r.seed)
    return _case(WIDE_ROW + "_exact", env, arrs, wide_twists(WIDE_ROW), r.n_obs, r.A, r.diff, r.seed)


BUILDERS = {}                                     # every case oracle_evaluate knows by name: CASES, the witness, tier B's
CASES = {**{"gw3_" + k: (lambda k=k: _gw_exact(k)) for k in sorted(WIDTHS)}, **{m: (lambda m=m: _probe_exact(m)) for m in PROBE_ROWS},
         WIDE_ROW: _wide_exact}
BUILDERS.update(CASES)


# ---- the oracle, attempt by attempt -----------------------------------------------------------------------------------------------------------------
def _unit(O, seed, key, t, stream):
    w = O.philox4x32_10([key & 0xFFFFFFFF, key >> 32, t, stream], [seed & 0xFFFFFFFF, seed >> 32])
    return w


def oracle_attempt(O, start, c, det, seed, key, arith):
    """One attempt from `start` (not modified), keyed `key`: oracle.solve_env's loop restated with the steps kept ->
    (success, total as f32, actions, [(ids, masks, perm, u)]); held to oracle.solve_env itself."""
    e = start.copy()
    total, acts, steps, t = np.float32(0), [], [], 0
    n_perms = len(c.tw[0])
    while not e.is_final():
        total = np.float32(total + np.float32(e.value()))
        ids, masks = [int(x) for x in e.observe()], [bool(m) for m in e.masks()]
        perm = (_unit(O, seed, key, t, 2)[0] * n_perms) >> 32 if n_perms else -1
        probs = np.asarray(c.op.predict(ids, masks, perm=perm, arith=arith)[0], np.float32)
        u = float(np.float32(_unit(O, seed, key, t, 5)[0] >> 8) * np.float32(1.0 / 16777216.0))
        if det:
            action, bv = 0, probs[0]
            for i in range(1, len(probs)):
                if probs[i] > bv:
                    action, bv = i, probs[i]
        else:
            action = O.sample_weighted(probs, u)
        steps.append((ids, masks, perm, u))
        e.next(action)
        acts.append(action)
        t += 1
    total = np.float32(total + np.float32(e.value()))
    mine = ((1.0 if e.success() else 0.0, float(total)), acts)
    (s, r), a = O.solve_env(start, c.op, det, 1, 0, C_UCB, 1, seed=seed, episode=key, arith=arith)
    assert (float(s), f32_bits(r), [int(x) for x in a]) == (mine[0][0], f32_bits(mine[0][1]), acts), (c.name, key)
    return mine[0][0], np.float32(total), acts, steps


@functools.lru_cache(maxsize=None)
def oracle_evaluate(case_key, E, N, det, arith, seed=None):
    """Every attempt of evaluate (episode e of E from reset(seed, offset + e), attempt k keyed (offset + e) N + k), computed once and
    shared -> SimpleNamespace(success, total, n_steps [E N], steps, means)."""
    from oracle import oracle as O
    c = BUILDERS[case_key]()
    seed = c.seed if seed is None else seed
    proto = host_env(c.env)
    out = SimpleNamespace(success=[], total=[], n_steps=[], acts=[], steps=[], by_attempt=[])
    for ep in range(E):
        e = proto.copy()
        e.seed_episode(seed, c.offset + ep)
        e.reset(c.diff)
        for k in range(N):
            s, tot, acts, steps = oracle_attempt(O, e, c, det, seed, (c.offset + ep) * N + k, arith)
            out.success.append(s); out.total.append(tot); out.n_steps.append(len(acts)); out.acts.append(acts)
            out.by_attempt.append(steps); out.steps += steps
    out.success, out.total, out.n_steps = np.asarray(out.success, np.float32), np.asarray(out.total, np.float32), np.asarray(out.n_steps, np.uint32)
    out.means = means_of(out.success, out.total, E, N)
    return out


def means_of(success, total, E, N):
    """evaluate.rs:36-52 over solve.rs:84-98: per episode the first attempt whose (success, total) is strictly better, the means in f32."""
    succ, rew = np.float32(0), np.float32(0)
    for ep in range(E):
        best = (0.0, float("-inf"))
        for k in range(N):
            val = (float(success[ep * N + k]), float(total[ep * N + k]))
            if val > best:
                best = val
        succ, rew = np.float32(succ + np.float32(best[0])), np.float32(rew + np.float32(best[1]))
    return float(np.float32(succ / np.float32(E))), float(np.float32(rew / np.float32(E)))


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------
def gpu_evaluate(tw, c, E, N, det, precision="fp16", seed=None, mcts=0):
    """collector.evaluate; a case with an episode offset (which the Python call does not take) through the C ABI the call wraps."""
    from twisterl_amd import _lib
    seed = c.seed if seed is None else seed
    if c.offset == 0:
        return tw.collector.evaluate(c.env, c.gp, E, det, N, mcts, seed, C_UCB, 1, 1, precision=precision)
    prm = _lib.SolveParams(int(det), N, mcts, C_UCB, 1, seed, _lib.PRECISIONS[precision])
    s, r = C.c_float(), C.c_float()
    _lib.check(_lib.lib().tw_evaluate_device_env(*c.env._args(), c.gp._handle(), C.byref(prm), E, c.offset, c.env.max_records, C.byref(s), C.byref(r)))
    return float(s.value), float(r.value)


def assert_f16_launch(c, persist, blocks=None, from_state=0):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["nw"], info["persist"], info["solve"], info["threads"]) == \
        (_lib.TW_KERNEL_SOLVE_BIG, 1, c.nc, 16, persist, from_state, 256), info
    if blocks is not None:
        assert info["blocks"] == blocks, info
    return info


def attempts():
    from twisterl_amd import _lib
    s, t, k = _lib.debug_last_attempts()
    return f32_bits(s).copy(), f32_bits(t).copy(), k.copy()


def same_attempts(o, got, only=None):
    s, t, k = got
    want = (f32_bits(o.success), f32_bits(o.total), o.n_steps)
    sel = slice(None) if only is None else np.asarray(only, bool)
    assert s.size == want[0].size
    assert np.array_equal(s[sel], want[0][sel]) and np.array_equal(k[sel], want[2][sel]) and np.array_equal(t[sel], want[1][sel]), \
        (np.flatnonzero((s != want[0]) | (k != want[2]) | (t != want[1]))[:8], k[:8], want[2][:8])


# ---- tier A ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_evaluate(tw, O, case, shape, det):
    E, N = shape
    c = CASES[case]()
    assert c.env.fp16_solve and c.env.fp16
    o = oracle_evaluate(case, E, N, det, O.ARITH_F16)
    assert_exact_along(c, o.steps)                                        # (on the CPU, before the GPU is touched)
    assert len(o.steps) > 0
    got = gpu_evaluate(tw, c, E, N, det)
    assert_f16_launch(c, 0, (E * N + 15) // 16)
    first = attempts()
    same_attempts(o, first)
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(o.means[0]), f32_bits(o.means[1])), (got, o.means)
    assert gpu_evaluate(tw, c, E, N, det) == got                          # twice the same
    again = attempts()
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_the_exact_cases_play_different_actions_and_lengths(O):
    """No GPU: the cases above cannot pass for lack of variety."""
    for case in sorted(CASES):
        o = oracle_evaluate(case, 34, 3, False, O.ARITH_F16)
        c = CASES[case]()
        assert len(set(int(n) for n in o.n_steps)) >= (3 if c.A > 1 else 2), (case, sorted(set(int(n) for n in o.n_steps)))
        assert len(set(a for acts in o.acts for a in acts)) >= min(2, c.A), case
    assert max(a for acts in oracle_evaluate(WIDE_ROW, 34, 3, False, O.ARITH_F16).acts for a in acts) >= 4


@pytest.mark.parametrize("groups", [1, 2])
def test_persistent_grid(tw, O, groups):
    from twisterl_amd import _lib
    case, E, N = "gw3_no_multiple", 100, 1
    c = CASES[case]()
    o = oracle_evaluate(case, E, N, False, O.ARITH_F16)
    assert_exact_along(c, o.steps)
    with _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups):
        got = gpu_evaluate(tw, c, E, N, False)
        assert_f16_launch(c, 1, groups)
        queued = attempts()
    with _lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1):
        plain = gpu_evaluate(tw, c, E, N, False)
        assert_f16_launch(c, 0, (E + 15) // 16)
        one_each = attempts()
    assert got == plain and all(np.array_equal(a, b) for a, b in zip(queued, one_each))
    same_attempts(o, queued)
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(o.means[0]), f32_bits(o.means[1]))


SOLVE_EPISODE = {"gw3_no_multiple": 5, "probe_o5a3v": 5, WIDE_ROW: 0}   # whose reset state is not final after one step


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("case", ["gw3_no_multiple", "probe_o5a3v", WIDE_ROW])
def test_solve_from_a_stepped_state(tw, O, case, N):
    c = CASES[case]()
    D.start(c.env, c.seed, SOLVE_EPISODE[case], 1)                        # a state no reset gives
    assert not c.env.is_final()
    start = host_env(c.env)
    for det in (True, False):
        per = [oracle_attempt(O, start, c, det, D.SEED, k, O.ARITH_F16) for k in range(N)]
        assert_exact_along(c, [s for p in per for s in p[3]])
        want = O.solve_env(start, c.op, det, N, 0, C_UCB, 1, seed=D.SEED, arith=O.ARITH_F16)
        want = ((float(want[0][0]), float(want[0][1])), [int(a) for a in want[1]])
        before = c.env.state_bytes()
        got = tw.collector.solve(c.env, c.gp, det, N, 0, C_UCB, 1, seed=D.SEED, precision="fp16")
        assert_f16_launch(c, 0, (N + 15) // 16, from_state=1)
        assert c.env.state_bytes() == before
        assert D.same(got, want), (got, want)
        s, t, k = attempts()
        assert np.array_equal(s, f32_bits([p[0] for p in per])) and np.array_equal(t, f32_bits([p[1] for p in per])) and \
            np.array_equal(k, np.asarray([len(p[2]) for p in per], np.uint32))
        exact, success, total = D.replay(c.env, got[1])                   # the returned moves lead to the returned result
        assert exact and float(success) == got[0][0] and f32_bits(total) == f32_bits(got[0][1])
        assert D.same(tw.collector.solve(c.env, c.gp, det, N, 0, C_UCB, 1, seed=D.SEED, precision="fp16"), got)


@functools.lru_cache(maxsize=None)
def _witness():
    """The exact GridWorld policy 32-32-16 with action columns 0 and 1 made of the same integers: column 0 carries the 2^-12 offsets,
    column 1 none.  Both get the largest bias, so the two lead wherever they are legal."""
    emb, eb, common, action, value = exact_arrays(GW.obs_size, 32, (32, 16), (), (), 4, seed=77)
    w, b, relu = action[0]
    w = w.reshape(-1, 4).copy()
    w[:, 1] = np.round(w[:, 0])
    b = b.copy()
    b[0] = b[1] = np.float32(6.5)
    return _gw_case("gw3_witness", (emb, eb, common, [(np.ascontiguousarray(w).reshape(-1), b, relu)], value))


BUILDERS["witness"] = _witness


def test_rounding_witness(tw, O):
    E, N = 40, 1
    c = _witness()
    f16 = oracle_evaluate("witness", E, N, True, O.ARITH_F16)
    chain = oracle_evaluate("witness", E, N, True, O.ARITH_CHAIN)
    assert_exact_along(c, f16.steps)
    # on the CPU: the two logits tie in ARITH_F16 (the first maximum wins) and differ in ARITH_CHAIN, and that changes an attempt
    tie = [c.op.forward(ids, [True] * 4, perm=-1, arith=O.ARITH_F16)[0] for ids, _, _, _ in f16.steps]
    assert all(f32_bits(l[0]) == f32_bits(l[1]) for l in tie)
    untie = [c.op.forward(ids, [True] * 4, perm=-1, arith=O.ARITH_CHAIN)[0] for ids, _, _, _ in f16.steps]
    assert any(l[1] > l[0] for l in untie)
    differ = (f32_bits(f16.success) != f32_bits(chain.success)) | (f32_bits(f16.total) != f32_bits(chain.total)) | (f16.n_steps != chain.n_steps)
    assert differ.any(), "ARITH_CHAIN and ARITH_F16 give the same attempts: the rounding to binary16 would not show"
    got = gpu_evaluate(tw, c, E, N, True)
    assert_f16_launch(c, 0, (E + 15) // 16)
    same_attempts(f16, attempts())
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(f16.means[0]), f32_bits(f16.means[1]))
    f32 = gpu_evaluate(tw, c, E, N, True, precision="fp32")              # and the f32 kernel of the same module is the f32 arithmetic
    same_attempts(chain, attempts())
    assert (f32_bits(f32[0]), f32_bits(f32[1])) == (f32_bits(chain.means[0]), f32_bits(chain.means[1]))


def test_update_from_torch_repacks_the_image(tw, O):
    import torch
    E, N = 40, 1
    old = _gw_case("gw3_update_old", exact_arrays(GW.obs_size, 36, (40, 20), (), (), 4, seed=71))
    new = _gw_case("gw3_update_new", exact_arrays(GW.obs_size, 36, (40, 20), (), (), 4, seed=72))
    before = gpu_evaluate(tw, old, E, N, False)
    s_before = attempts()
    we, be, cs, as_, vs = new.arrs
    state = {"embeddings.weight": torch.tensor(we.T.copy()).cuda(), "embeddings.bias": torch.tensor(be).cuda()}
    for name, layers in (("common", cs), ("action", as_), ("value", vs)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = torch.tensor(np.asarray(wl).reshape(-1, len(bl)).T.copy()).cuda()
            state[f"{name}.{2 * i}.bias"] = torch.tensor(np.asarray(bl)).cuda()
    old.gp.update_from_torch(state)
    after = gpu_evaluate(tw, old, E, N, False)
    assert_f16_launch(old, 0, (E + 15) // 16)
    s_after = attempts()
    fresh = gpu_evaluate(tw, new, E, N, False)
    s_fresh = attempts()
    assert after == fresh and all(np.array_equal(a, b) for a, b in zip(s_after, s_fresh))
    assert not all(np.array_equal(a, b) for a, b in zip(s_before, s_after)), (before, after)
    BUILDERS["update_new"] = lambda: new
    o = oracle_evaluate("update_new", E, N, False, O.ARITH_F16)
    assert_exact_along(new, o.steps)
    same_attempts(o, s_after)


@pytest.mark.parametrize("case", ["gw3_no_multiple", "probe_o64a4s", WIDE_ROW])
def test_no_result_depends_on_what_the_workspace_held(tw, O, case):
    from twisterl_amd import _lib
    E, N = 34, 3
    c = CASES[case]()
    o = oracle_evaluate(case, E, N, False, O.ARITH_F16)
    want = gpu_evaluate(tw, c, E, N, False)
    first = attempts()
    same_attempts(o, first)
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            assert gpu_evaluate(tw, c, E, N, False) == want
            assert_f16_launch(c, 0, (E * N + 15) // 16)
            assert all(np.array_equal(a, b) for a, b in zip(first, attempts())), hex(pattern)
    # another policy of other widths leaves its own image and results behind; then the first again, hook off
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(make_deep_policy_arrays_obs(c.arrs[0].shape[0], seed=5, emb=64, common=(96, 48), n_actions=c.A,
                                                                                         scale=1.0), *c.tw)})
    gpu_evaluate(tw, other, E, N, False)
    assert_f16_launch(c, 0, (E * N + 15) // 16)
    assert gpu_evaluate(tw, c, E, N, False) == want
    assert all(np.array_equal(a, b) for a, b in zip(first, attempts()))


# ---- tier B ----------------------------------------------------------------------------------------------------------------------------------------
# (flat_32's seed: chosen on the CPU, with the oracle alone -- at seed 62 the sampled 40 x 1 case had 11 of 40 attempts undecided on the
# device struct's start states, above the quarter; the cap stays)
GENERAL = {"deep_36_40_20": dict(seed=61, emb=36, common=(40, 20), scale=0.5), "flat_32": dict(seed=65, emb=32, common=(), scale=2.0)}
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _general(key):
    return _gw_case("gw3_" + key, make_deep_policy_arrays_obs(GW.obs_size, n_actions=4, **GENERAL[key]))


BUILDERS.update({k: (lambda k=k: _general(k)) for k in GENERAL})


def decided_attempts(c, o, det):
    """-> bool per attempt of `o`: every step's action is the one any conforming f16-input implementation takes."""
    n = len(o.steps)
    obs = np.asarray([s[0] for s in o.steps], np.int64)
    masks = np.asarray([s[1] for s in o.steps], bool)
    perms = np.asarray([s[2] for s in o.steps], np.int64)
    m0, m1 = ref64.max_activations(c.arrs, c.tw[0], c.tw[1], obs, perms)
    assert max(m0, m1) < F16_MAX
    l64, _, el, _ = ref64.forward_f64_bound(c.arrs, c.tw[0], c.tw[1], obs, masks, perms, "fp16")
    p64 = ref64.masked_softmax_f64(l64, masks)
    ep = ref64.prob_bound(l64, el, masks)
    lo, hi = np.maximum(p64 - ep, 0.0), p64 + ep
    A = c.A
    ok = np.zeros(n, bool)
    for i in range(n):
        if det:
            a = int(np.argmax(p64[i]))
            ok[i] = all(lo[i, a] > hi[i, b] for b in range(A) if b != a)
        else:
            u = np.float64(np.float32(o.steps[i][3]))
            margin = (A + 2) * U32 * float(hi[i].sum())                   # the A additions of the total and the cumulative sums, the product
            t_lo, t_hi = u * float(lo[i].sum()) - margin, u * float(hi[i].sum()) + margin
            good, c_lo, c_hi = True, 0.0, 0.0
            for a in range(A - 1):
                c_lo, c_hi = c_lo + float(lo[i, a]), c_hi + float(hi[i, a])
                if c_lo - margin > t_hi:                                  # cum > u total at both ends: this action, nothing behind it is compared
                    break
                if not c_hi + margin <= t_lo:                             # neither: the ends disagree
                    good = False
                    break
            ok[i] = good
    out, at = [], 0
    for steps in o.by_attempt:
        out.append(bool(ok[at:at + len(steps)].all()))
        at += len(steps)
    return np.asarray(out, bool)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("shape", ((40, 1), (40, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("key", sorted(GENERAL))
def test_general_weights_where_float64_decides(tw, O, key, shape, det):
    E, N = shape
    c = _general(key)
    assert activation_ceiling(c.arrs, c.n_obs) < F16_MAX                  # (on the CPU, before the GPU is touched)
    o = oracle_evaluate(key, E, N, det, O.ARITH_F16)
    decided = decided_attempts(c, o, det)
    undecided = int((~decided).sum())
    print(f"[fp16 solve] {key} {E}x{N} {'deterministic' if det else 'sampled'}: {undecided} of {E * N} attempts undecided")
    assert 4 * undecided <= E * N, (key, undecided, E * N)
    acts = set(a for acts_, d in zip(o.acts, decided) if d for a in acts_)
    lens = set(int(n) for n, d in zip(o.n_steps, decided) if d)
    assert len(acts) >= 2 and len(lens) >= 3, (acts, lens)
    gpu_evaluate(tw, c, E, N, det)
    assert_f16_launch(c, 0, (E * N + 15) // 16)
    same_attempts(o, attempts(), only=decided)


# ---- what the kernel does not take keeps its path and its message -----------------------------------------------------------------------------------
def _message(fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)
    raise AssertionError("no error")


def test_refusals_and_unchanged_paths(tw, O):
    from twisterl_amd import _lib
    arrs = _general("deep_36_40_20").arrs
    gp = amd_policy(arrs)
    mfma = amd_policy(make_policy_arrays_obs(GW.obs_size, seed=3, emb=64, hidden=64, n_actions=4))
    env_s, env_az, env_16, env_d = (_gw_env(m) for m in (GW_S, GW_AZ, GW_16, GW_DEFAULT))
    assert env_s.fp16_solve and env_az.fp16_solve and env_az.search and env_16.fp16 and not env_16.fp16_solve and not env_d.fp16 and not env_d.fp16_solve
    ev = lambda env, pol, prec, mcts=0: tw.collector.evaluate(env, pol, 20, True, 2, mcts, 5, C_UCB, 1, 1, precision=prec)
    so = lambda env, pol, prec, mcts=0: tw.collector.solve(D.start(env, 3, 3, 1), pol, True, 2, mcts, C_UCB, 1, seed=5, precision=prec)
    for call in (ev, so):
        for refused in (lambda: call(env_az, gp, "fp16", 4),              # MCTS-guided, on a module that has both kernels
                        lambda: call(env_16, gp, "fp16"),                 # a module built with fp16=True alone
                        lambda: call(env_d, gp, "fp16"),                  # a default module
                        lambda: call(env_s, mfma, "fp16"),                # an MFMA-shape policy
                        lambda: call(env_s, gp, "fp16x2"),                # the split mode
                        lambda: call(env_az, gp, "fp16x2", 4)):
            assert _message(refused) == F32_ONLY
            assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    # precision="fp32" on the new module: the f32 kernel, and a default module's bytes
    for call, from_state in ((ev, 0), (so, 1)):
        a = call(env_s, gp, "fp32")
        info = _lib.debug_last_launch()
        assert (info["family"], info["nw"], info["nc"], info["solve"]) == (_lib.TW_KERNEL_SOLVE_BIG, 0, 9, from_state), info
        sa = attempts()
        b = call(env_d, gp, "fp32")
        sb = attempts()
        assert a == b and all(np.array_equal(x, y) for x, y in zip(sa, sb))
        assert call(env_s, gp, "fp32") == call(env_s, gp, "exact") == a
    # and fp16 on it: the f16 kernel
    ev(env_s, gp, "fp16")
    assert _lib.debug_last_launch()["nw"] == 16
    ev(env_az, gp, "fp16")                                                # the search form without MCTS: the f16 kernel too
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_SOLVE_BIG, 16)
    ev(env_az, gp, "fp32", 4)                                             # MCTS in f32 on it: the search kernel, as ever
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_MCTS_BIG
