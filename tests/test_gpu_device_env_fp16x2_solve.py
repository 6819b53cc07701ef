"""GPU: collector.evaluate / collector.solve of device environments with precision="fp16x2" -- solve_env16x2_kernel over EngineV16x2
(twisterl_amd/csrc/tw_solve_env16x2.hpp, tw_engine_generic16x2.hpp), modules built with build_device_env(..., fp16x2_solve=True).

The split mode gives f32 answers, so the reference is the oracle's f32 loop (ARITH_CHAIN) over the module's host code, attempt by
attempt, in the two tiers of tests/test_gpu_device_env_fp16_solve.py (whose helpers this file imports):

A  EXACT ARITHMETIC.  tests/split16x2_ref.exact_arrays() on GridWorld 3 x 3, and policies of the same recipe (exact_split_arrays below)
   on the probe rows of NC 4, 9, 25, 64 and the wide row: an integer table, first Linear with weights m + n 2^-12 (lo terms not zero),
   later Linears with integer weights over the fractional activations, half-integer biases.  On the CPU, before the GPU is touched,
   along the oracle's ARITH_CHAIN trajectories: the numpy restatement of the split spec (split16x2_ref.forward) gives the oracle's f32
   bits and float64's values -- the split spec IS the f32 spec on those inputs, in any order of summation.  Every attempt's (success,
   total, n_steps), the two means and solve's action list must then be bit for bit the oracle's, and the same module's fp32 call's.
   (The fp16 file's own exact policies carry 2^-12 in the table AND in every layer; the product of two lo terms, which the split
   drops, is not zero there, so they are exact in the f16-input mode only: the assertion above fails for them on the CPU.)
B  GENERAL WEIGHTS, gated where float64 decides: the fp16 file's tier B with ref64.forward_f64_bound(mode="fp16x2"); at most a quarter
   of a case's attempts may be undecided (asserted on the CPU first, the count printed).

Then: the lo terms are used (the fp16 file's rounding witness), the persistent grid, solve from a stepped state, the range fall-back
to the f32 kernel, the image after update_from_torch, pre-filled workspace memory, a caller's stream, and what the kernel does not
take.  Every fp16x2 call is held to tw_debug_last_launch = (SOLVE_BIG, nt 1, the row's nc, nw 32, ...) and to a second call's bytes."""
import functools
import signal
from types import SimpleNamespace

import numpy as np
import pytest

from tests import device_env_solve as D
from tests import ref64, split16x2_ref as S
from tests import test_gpu_device_env_fp16_solve as F
from tests import test_gpu_device_env_fp16x2 as X
from tests.device_env_matrix import BY_MODULE as PROBE_ROWS_BY_MODULE, PROBE_HPP, host_env
from tests.device_env_matrix import twists as probe_twists
from tests.device_env_util import GRIDWORLD_HPP
from tests.device_env_wide import BY_MODULE as WIDE_ROWS_BY_MODULE, twists as wide_twists
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs, make_policy_arrays_obs

pytestmark = pytest.mark.gpu

GW = F.GW
PROBE_ROWS, WIDE_ROW, SHAPES, C_UCB = F.PROBE_ROWS, F.WIDE_ROW, F.SHAPES, F.C_UCB
SUFFIX = "_fp16x2s"
GW_X2S, GW_ALL, GW_X2 = "gridworld3x3_fp16x2s", "gridworld3x3_all_x2s", "gridworld3x3_fp16x2"
NW_SPLIT = 32
FALLBACK_LINE = X.FALLBACK_LINE
F32_ONLY = F.F32_ONLY
WORST = {"tier_a": 0.0}                            # the largest |gpu - oracle f32| of a total seen in tier A (recorded, not gated)


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16x2 evaluate / solve device-environment test exceeded its time limit")
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
    jobs = [(PROBE_HPP, PROBE_ROWS_BY_MODULE[m].alias, m + SUFFIX, {"fp16x2_solve": True}) for m in PROBE_ROWS]
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    jobs += [(r.header, r.type, WIDE_ROW + SUFFIX, {"fp16x2_solve": True, "wide": True})]
    jobs += [(GRIDWORLD_HPP, GW.type, GW_X2S, {"fp16x2_solve": True}),
             (GRIDWORLD_HPP, GW.type, GW_ALL, {"fp16x2_solve": True, "fp16_solve": True, "fp16_search": True, "search": True}),
             (GRIDWORLD_HPP, GW.type, GW_X2, {"fp16x2": True}), (GRIDWORLD_HPP, GW.type, F.GW_S, {"fp16_solve": True}),
             (GRIDWORLD_HPP, GW.type, F.GW_DEFAULT, {})]
    assert len(jobs) <= 16
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(j[0], j[1], j[2], **j[3]), jobs))
    return {j[2]: p for j, p in zip(jobs, paths)}


# ---- exact policies ---------------------------------------------------------------------------------------------------------------------------------
def exact_split_arrays(obs_size, n_obs, emb, common, policy_layers, value_layers, A, seed):
    """split16x2_ref.exact_arrays()'s recipe for any row: table and embedding bias small integers (the embedding's output an integer,
    its lo term zero); the FIRST Linear -- common[0], every row here has one -- weights m + n 2^-12 (lo terms not zero); every later
    Linear integer weights (lo zero, so lo x lo is identically zero) over the fractional activations; biases half-integers.  The
    densities keep every value a multiple of 2^-12 small enough for f32 to hold every partial sum: assert_split_is_f32 shows it."""
    assert len(common) >= 1
    rng = np.random.default_rng(seed)
    f32 = np.float32

    def ints(shape, per_output, hi):
        v = rng.integers(1, hi + 1, size=shape).astype(f32) * rng.choice(f32([-1.0, 1.0]), size=shape)
        return np.where(rng.random(shape) < min(1.0, per_output / shape[0]), v, f32(0.0)).astype(f32)

    def half(n, lo, hi):
        return (rng.integers(lo, hi, size=n).astype(f32) + f32(0.5)).astype(f32)

    def lin(i, o, relu, per_output, hi, frac):
        w = ints((i, o), per_output, hi)
        if frac:
            w = np.where(w != 0, w + rng.integers(1, 4, size=w.shape).astype(f32) * rng.choice(f32([-1.0, 1.0]), size=w.shape) * f32(2.0 ** -12),
                         f32(0.0)).astype(f32)
        return (np.ascontiguousarray(w).reshape(-1), half(o, -2, 2), relu)

    table = np.where(rng.random((obs_size, emb)) < min(0.5, 3.0 / n_obs), rng.choice(f32([-1.0, 1.0]), size=(obs_size, emb)), f32(0.0)).astype(f32)
    be = rng.integers(-1, 2, size=emb).astype(f32)
    cs, w = [], emb
    for n, h in enumerate(common):
        cs.append(lin(w, h, True, 6, 2 if n == 0 else 1, n == 0)); w = h
    acts, wa = [], w
    for h in policy_layers:
        acts.append(lin(wa, h, True, 5, 1, False)); wa = h
    acts.append(lin(wa, A, False, 8, 1, False))
    vals, wv = [], w
    for h in value_layers:
        vals.append(lin(wv, h, True, 5, 1, False)); wv = h
    vals.append(lin(wv, 1, False, 8, 1, False))
    return (table, be, cs, acts, vals)


def _rows_of(c, steps):
    """The observations, masks and twists of `steps` as split16x2_ref.forward and ref64 take them (-1 = no id)."""
    obs = np.asarray([list(s[0]) + [-1] * (c.n_obs - len(s[0])) for s in steps], np.int64).reshape(len(steps), c.n_obs)
    return obs, np.asarray([s[1] for s in steps], bool), np.asarray([s[2] for s in steps], np.int64)


def assert_split_is_f32(O, c, steps):
    """On the CPU: along `steps` (the oracle's ARITH_CHAIN trajectories) the numpy restatement of the split spec gives the oracle's
    f32 bits, and float64's values: every product and partial sum is exact, so all orders agree and the split spec is the f32 spec."""
    assert len(steps) > 0
    obs, masks, perms = _rows_of(c, steps)
    fed = []
    lg, v = S.forward(c.arrs, c.tw[0], c.tw[1], obs, masks, perms, fed=fed)
    assert max(float(np.abs(x).max(initial=0.0)) for x in fed) < S.LIMIT
    l64, v64 = ref64.forward_f64(c.arrs, c.tw[0], c.tw[1], obs, masks, perms)
    assert np.array_equal(lg.astype(np.float64), l64) and np.array_equal(v.astype(np.float64), v64), c.name
    seen = set()
    for i, (ids, mk, pm, _u) in enumerate(steps):
        key = (tuple(ids), tuple(mk), pm)
        if key in seen:
            continue
        seen.add(key)
        l1, v1 = c.op.forward(list(ids), list(mk), perm=pm, arith=O.ARITH_CHAIN)
        assert np.array_equal(f32_bits(np.asarray(l1, np.float32)), f32_bits(lg[i])) and f32_bits(np.float32(v1)) == f32_bits(v[i]), (c.name, i)
    assert any(bool((2 * x != np.round(2 * x)).any()) for x in fed[1:]), "no fractional activation: the lo terms would be zero"


def assert_in_range(c):
    wmax, top = S.weight_ceiling(c.arrs, c.n_obs)                         # (on the CPU, before the GPU is touched)
    assert wmax < S.LIMIT and top < S.LIMIT, (c.name, wmax, top)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
def _gw_env(module=GW_X2S):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[module], module, [3, 3, GW.max_steps, GW.diff], max_records=GW.max_steps + 1)


def _gw_case(name, arrs, module=GW_X2S):
    return F._case(name, _gw_env(module), arrs, ((), ()), GW.n_obs, GW.A, GW.diff, GW.seed)


@functools.lru_cache(maxsize=None)
def _gw_exact():
    return _gw_case("gw3_exact", S.exact_arrays())


@functools.lru_cache(maxsize=None)
def _probe_exact(module):
    from twisterl_amd.env import DeviceEnv
    r = PROBE_ROWS_BY_MODULE[module]
    name = module + SUFFIX
    env = DeviceEnv(build_all()[name], name, [r.obs_size, r.max_steps, r.diff, -1], max_records=r.max_steps + 1)
    arrs = exact_split_arrays(r.obs_size, r.n_obs, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=500 + r.seed)
    return F._case(module + "_exact", env, arrs, probe_twists(module), r.n_obs, r.A, r.diff, r.seed, r.offset)


@functools.lru_cache(maxsize=None)
def _wide_exact():
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    name = WIDE_ROW + SUFFIX
    env = DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)
    arrs = exact_split_arrays(r.obs_size, r.n_obs, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=500 + r.seed)
    return F._case(WIDE_ROW + "_exact", env, arrs, wide_twists(WIDE_ROW), r.n_obs, r.A, r.diff, r.seed)


# (the keys carry "x2:" -- F.oracle_evaluate looks its cases up in F.BUILDERS, which holds the fp16 file's own under the plain names)
CASES = {"x2:gw3_exact": _gw_exact, **{"x2:" + m: (lambda m=m: _probe_exact(m)) for m in PROBE_ROWS}, "x2:" + WIDE_ROW: _wide_exact}
F.BUILDERS.update(CASES)


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------
def gpu_evaluate(tw, c, E, N, det, precision="fp16x2", seed=None, mcts=0):
    return F.gpu_evaluate(tw, c, E, N, det, precision=precision, seed=seed, mcts=mcts)


def assert_launch(c, persist, blocks=None, from_state=0, nw=NW_SPLIT):
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["nw"], info["persist"], info["solve"], info["threads"]) == \
        (_lib.TW_KERNEL_SOLVE_BIG, 1, c.nc, nw, persist, from_state, 256), info
    if blocks is not None:
        assert info["blocks"] == blocks, info
    return info


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def evaluate_twice(tw, c, E, N, det, persist=0, blocks=None):
    """One fp16x2 evaluate held to the launch record and to a second call's bytes -> (the two means, the attempts)."""
    got = gpu_evaluate(tw, c, E, N, det)
    assert_launch(c, persist, (E * N + 15) // 16 if blocks is None else blocks)
    first = F.attempts()
    again = gpu_evaluate(tw, c, E, N, det)
    assert (f32_bits(again[0]), f32_bits(again[1])) == (f32_bits(got[0]), f32_bits(got[1])) and same_bits(first, F.attempts())
    return got, first


# ---- tier A ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "sampled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_evaluate(tw, O, case, shape, det):
    E, N = shape
    c = CASES[case]()
    assert c.env.fp16x2_solve and c.env.fp16x2 and c.env.fp16
    o = F.oracle_evaluate(case, E, N, det, O.ARITH_CHAIN)
    assert_split_is_f32(O, c, o.steps)                                    # (on the CPU, before the GPU is touched; the range as well)
    got, first = evaluate_twice(tw, c, E, N, det)
    worst = float(np.abs(first[1].view(np.float32).astype(np.float64) - o.total.astype(np.float64)).max())
    WORST["tier_a"] = max(WORST["tier_a"], worst)
    print(f"[fp16x2 solve] {case} {E}x{N}: max |gpu - oracle f32| of a total = {worst:.3e} (tier A so far: {WORST['tier_a']:.3e})")
    F.same_attempts(o, first)
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(o.means[0]), f32_bits(o.means[1])), (got, o.means)
    f32 = gpu_evaluate(tw, c, E, N, det, precision="fp32")                # the same module's f32 kernel
    assert_launch(c, 0, (E * N + 15) // 16, nw=0)
    assert same_bits(first, F.attempts()) and (f32_bits(f32[0]), f32_bits(f32[1])) == (f32_bits(got[0]), f32_bits(got[1]))


def test_the_exact_cases_play_different_actions_and_lengths(O):
    """No GPU: the cases above cannot pass for lack of variety."""
    for case in sorted(CASES):
        o = F.oracle_evaluate(case, 34, 3, False, O.ARITH_CHAIN)
        c = CASES[case]()
        assert len(set(int(n) for n in o.n_steps)) >= (3 if c.A > 1 else 2), (case, sorted(set(int(n) for n in o.n_steps)))
        assert len(set(a for acts in o.acts for a in acts)) >= min(2, c.A), case
    assert max(a for acts in F.oracle_evaluate("x2:" + WIDE_ROW, 34, 3, False, O.ARITH_CHAIN).acts for a in acts) >= 4


# ---- the lo terms are used -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _witness():
    """The fp16 file's rounding witness (F._witness's arrays: the exact GridWorld policy 32-32-16 with action columns 0 and 1 made of
    the same integers, column 0 with the 2^-12 offsets, column 1 without -- they tie in ARITH_F16 and not in ARITH_CHAIN), on the
    module with both flags."""
    emb, eb, common, action, value = F.exact_arrays(GW.obs_size, 32, (32, 16), (), (), 4, seed=77)
    w, b, relu = action[0]
    w = w.reshape(-1, 4).copy()
    w[:, 1] = np.round(w[:, 0])
    b = b.copy()
    b[0] = b[1] = np.float32(6.5)
    return _gw_case("gw3_witness_x2", (emb, eb, common, [(np.ascontiguousarray(w).reshape(-1), b, relu)], value), module=GW_ALL)


F.BUILDERS["x2:witness"] = _witness


def test_rounding_witness(tw, O):
    E, N = 40, 1
    c = _witness()
    assert c.env.fp16x2_solve and c.env.fp16_solve
    f16 = F.oracle_evaluate("x2:witness", E, N, True, O.ARITH_F16)
    chain = F.oracle_evaluate("x2:witness", E, N, True, O.ARITH_CHAIN)
    tie = [c.op.forward(ids, [True] * 4, perm=-1, arith=O.ARITH_F16)[0] for ids, _, _, _ in f16.steps]
    assert all(f32_bits(l[0]) == f32_bits(l[1]) for l in tie)
    differ = (f32_bits(f16.success) != f32_bits(chain.success)) | (f32_bits(f16.total) != f32_bits(chain.total)) | (f16.n_steps != chain.n_steps)
    assert differ.any(), "ARITH_CHAIN and ARITH_F16 give the same attempts: the lo terms would not show"
    # on the CPU: the numpy restatement of the split spec leads with the ARITH_CHAIN action at every step of the f32 trajectories (the
    # policy carries 2^-12 in every layer, so the split forward is not exact on it: the witness's gap of n 2^-12 per unit of activation
    # is what the lo terms must carry, and they do in the spec)
    obs, masks, perms = _rows_of(c, chain.steps)
    fed = []
    lg, _ = S.forward(c.arrs, (), (), obs, masks, perms, fed=fed)
    assert max(float(np.abs(x).max(initial=0.0)) for x in fed) < S.LIMIT
    for i, (ids, mk, pm, _u) in enumerate(chain.steps):
        l32 = np.asarray(c.op.forward(list(ids), list(mk), perm=pm, arith=O.ARITH_CHAIN)[0], np.float32)
        assert int(np.argmax(lg[i])) == int(np.argmax(l32)) and np.sort(lg[i])[-1] > np.sort(lg[i])[-2], (i, lg[i], l32)
    got, first = evaluate_twice(tw, c, E, N, True)
    F.same_attempts(chain, first)                                         # fp16x2: the ARITH_CHAIN action
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(chain.means[0]), f32_bits(chain.means[1]))
    gpu_evaluate(tw, c, E, N, True, precision="fp16")                     # fp16 from the same module: the other
    assert_launch(c, 0, (E + 15) // 16, nw=16)
    F.same_attempts(f16, F.attempts())


# ---- the persistent grid and the attempt queue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2])
def test_persistent_grid(tw, O, groups):
    from twisterl_amd import _lib
    case, E, N = "x2:gw3_exact", 100, 1
    c = CASES[case]()
    o = F.oracle_evaluate(case, E, N, False, O.ARITH_CHAIN)
    assert_split_is_f32(O, c, o.steps)
    with _lib.launch_option(_lib.TW_OPT_ENV_RESIDENT_GROUPS, groups):
        got, queued = evaluate_twice(tw, c, E, N, False, persist=1, blocks=groups)
    with _lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1):
        plain, one_each = evaluate_twice(tw, c, E, N, False)
    assert got == plain and same_bits(queued, one_each)
    F.same_attempts(o, queued)
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(o.means[0]), f32_bits(o.means[1]))


# ---- solve from a stepped state ----------------------------------------------------------------------------------------------------------------------
SOLVE_CASES = {"x2:gw3_exact": F.SOLVE_EPISODE["gw3_no_multiple"], "x2:probe_o5a3v": F.SOLVE_EPISODE["probe_o5a3v"],
               "x2:" + WIDE_ROW: F.SOLVE_EPISODE[WIDE_ROW]}


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("case", sorted(SOLVE_CASES))
def test_solve_from_a_stepped_state(tw, O, case, N):
    c = CASES[case]()
    D.start(c.env, c.seed, SOLVE_CASES[case], 1)                          # a state no reset gives
    assert not c.env.is_final()
    start = host_env(c.env)
    for det in (True, False):
        per = [F.oracle_attempt(O, start, c, det, D.SEED, k, O.ARITH_CHAIN) for k in range(N)]
        assert_split_is_f32(O, c, [s for p in per for s in p[3]])
        want = O.solve_env(start, c.op, det, N, 0, C_UCB, 1, seed=D.SEED, arith=O.ARITH_CHAIN)
        want = ((float(want[0][0]), float(want[0][1])), [int(a) for a in want[1]])
        before = c.env.state_bytes()
        got = tw.collector.solve(c.env, c.gp, det, N, 0, C_UCB, 1, seed=D.SEED, precision="fp16x2")
        assert_launch(c, 0, (N + 15) // 16, from_state=1)
        assert c.env.state_bytes() == before
        assert D.same(got, want), (got, want)
        first = F.attempts()
        s, t, k = first
        assert np.array_equal(s, f32_bits([p[0] for p in per])) and np.array_equal(t, f32_bits([p[1] for p in per])) and \
            np.array_equal(k, np.asarray([len(p[2]) for p in per], np.uint32))
        exact, success, total = D.replay(c.env, got[1])                   # the returned moves lead to the returned result
        assert exact and float(success) == got[0][0] and f32_bits(total) == f32_bits(got[0][1])
        assert D.same(tw.collector.solve(c.env, c.gp, det, N, 0, C_UCB, 1, seed=D.SEED, precision="fp16x2"), got)
        assert same_bits(first, F.attempts())
        f32 = tw.collector.solve(c.env, c.gp, det, N, 0, C_UCB, 1, seed=D.SEED, precision="fp32")
        assert_launch(c, 0, (N + 15) // 16, from_state=1, nw=0)
        assert D.same(f32, got) and same_bits(first, F.attempts())


# ---- tier B ----------------------------------------------------------------------------------------------------------------------------------------
GENERAL = F.GENERAL
U32 = F.U32


@functools.lru_cache(maxsize=None)
def _general(key):
    return _gw_case("gw3_" + key, make_deep_policy_arrays_obs(GW.obs_size, n_actions=4, **GENERAL[key]))


F.BUILDERS.update({"x2:" + k: (lambda k=k: _general(k)) for k in GENERAL})


def decided_attempts(c, o, det, mode="fp16x2"):
    """F.decided_attempts with the bound's mode as a parameter and the split range in place of binary16's: -> bool per attempt of
    `o`: every step's action is the one any conforming implementation of `mode` takes."""
    n = len(o.steps)
    obs, masks, perms = _rows_of(c, o.steps)
    m0, m1 = ref64.max_activations(c.arrs, c.tw[0], c.tw[1], obs, perms)
    assert max(m0, m1) < S.LIMIT
    l64, _, el, _ = ref64.forward_f64_bound(c.arrs, c.tw[0], c.tw[1], obs, masks, perms, mode)
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
    assert_in_range(c)                                                    # (on the CPU, before the GPU is touched)
    o = F.oracle_evaluate("x2:" + key, E, N, det, O.ARITH_CHAIN)
    decided = decided_attempts(c, o, det)
    undecided = int((~decided).sum())
    print(f"[fp16x2 solve] {key} {E}x{N} {'deterministic' if det else 'sampled'}: {undecided} of {E * N} attempts undecided")
    assert 4 * undecided <= E * N, (key, undecided, E * N)
    acts = set(a for acts_, d in zip(o.acts, decided) if d for a in acts_)
    lens = set(int(n) for n, d in zip(o.n_steps, decided) if d)
    assert len(acts) >= 2 and len(lens) >= 3, (acts, lens)
    got, first = evaluate_twice(tw, c, E, N, det)
    F.same_attempts(o, first, only=decided)


# ---- the range ---------------------------------------------------------------------------------------------------------------------------------------
def _bits_of(result):
    (s, r), acts = result if isinstance(result[0], tuple) else (result, [])
    bits = lambda x: int(np.float32(x).view(np.uint32))
    return bits(s), bits(r), list(acts)


def _outcome(fn):
    """A call's result as bits (NaN compares equal to itself), or its error."""
    try:
        return _bits_of(fn())
    except Exception as e:       # noqa: BLE001
        return type(e), str(e)


def _calls(tw, c):
    ev = lambda prec: tw.collector.evaluate(c.env, c.gp, 40, True, 1, 0, c.seed, C_UCB, 1, 1, precision=prec)
    so = lambda prec: tw.collector.solve(D.start(c.env, c.seed, 5, 1), c.gp, False, 8, 0, C_UCB, 1, seed=D.SEED, precision=prec)
    return (("evaluate", ev, 0, 3), ("solve", so, 1, 1))


def _assert_falls_back(tw, c, capfd):
    for what, call, from_state, blocks in _calls(tw, c):
        capfd.readouterr()
        got = _outcome(lambda: call("fp16x2"))
        assert_launch(c, 0, blocks, from_state=from_state, nw=0)          # the f32 kernel
        split_attempts = F.attempts()
        err = capfd.readouterr().err
        assert err.count(FALLBACK_LINE) == 1 and err.count("\n") == 1 and f"this {what} runs in fp32" in err, err
        assert got == _outcome(lambda: call("fp32"))
        assert same_bits(split_attempts, F.attempts())
        assert capfd.readouterr().err == ""


def test_a_weight_of_4094_runs_the_split_kernel(tw, capfd):
    c = _gw_case("gw3_w4094", X._with_head_weight(S.width_arrays("no_multiple"), 4094.0))
    assert_in_range(c)
    for what, call, from_state, blocks in _calls(tw, c):
        capfd.readouterr()
        a = _outcome(lambda: call("fp16x2"))
        assert_launch(c, 0, blocks, from_state=from_state)
        assert a == _outcome(lambda: call("fp16x2"))
        assert capfd.readouterr().err == ""


@pytest.mark.parametrize("w", [4095.0, -4095.0, 5000.0, float("nan")])
def test_a_weight_outside_the_range_gives_the_fp32_call(tw, capfd, w):
    base = S.width_arrays("no_multiple")
    c = _gw_case("gw3_wbad", X._with_head_weight(base, w))
    _assert_falls_back(tw, c, capfd)
    # back into range: the split kernel runs again, on the image of the new weights
    c.gp.update_from_torch(X._state_dict(base))
    good = _gw_case("gw3_wgood", base)
    for (what, call, from_state, blocks), (_, fresh, _, _) in zip(_calls(tw, c), _calls(tw, good)):
        got = _outcome(lambda: call("fp16x2"))
        assert_launch(c, 0, blocks, from_state=from_state)
        mine = F.attempts()
        assert capfd.readouterr().err == ""
        assert got == _outcome(lambda: fresh("fp16x2")) and same_bits(mine, F.attempts())


def test_an_activation_outside_the_range_gives_the_fp32_call(tw, capfd):
    emb, eb, common, action, value = S.width_arrays("no_multiple")
    # an embedding output of -5000 (no ReLU behind the embedding)
    eb2 = np.array(eb, np.float32, copy=True)
    eb2[3] = np.float32(-5000.0)
    seq = lambda ls: tw.nn.Sequential([tw.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    gp = tw.nn.Policy(tw.nn.EmbeddingBag(emb.tolist(), eb2.tolist(), False, [emb.shape[0]], 0), seq(common), seq(action), seq(value), [], [])
    c = _gw_case("gw3_embbad", (emb, eb2, common, action, value))
    c.gp = gp
    _assert_falls_back(tw, c, capfd)
    # a hidden activation of about 5000 (a common layer's bias)
    w0, b0, r0 = common[0]
    b1 = np.array(b0, np.float32, copy=True)
    b1[7] = np.float32(5000.0)
    _assert_falls_back(tw, _gw_case("gw3_hidbad", (emb, eb, [(w0, b1, r0)] + common[1:], action, value)), capfd)


# ---- image, memory, stream -----------------------------------------------------------------------------------------------------------------------------
def test_update_from_torch_repacks_the_image(tw, O):
    E, N = 40, 1
    mk = lambda seed: make_deep_policy_arrays_obs(GW.obs_size, seed=seed, emb=36, common=(40, 20), n_actions=4, scale=2.0)
    old, new = _gw_case("gw3_update_old", mk(71)), _gw_case("gw3_update_new", mk(72))
    gpu_evaluate(tw, old, E, N, False)
    s_before = F.attempts()
    old.gp.update_from_torch(X._state_dict(new.arrs))
    after, s_after = evaluate_twice(tw, old, E, N, False)
    fresh, s_fresh = evaluate_twice(tw, new, E, N, False)
    assert after == fresh and same_bits(s_after, s_fresh)
    assert not same_bits(s_before, s_after)


@pytest.mark.parametrize("case", ["x2:gw3_exact", "x2:probe_o64a4s", "x2:" + WIDE_ROW])
def test_no_result_depends_on_what_the_workspace_held(tw, O, case):
    from twisterl_amd import _lib
    E, N = 34, 3
    c = CASES[case]()
    o = F.oracle_evaluate(case, E, N, False, O.ARITH_CHAIN)
    want, first = evaluate_twice(tw, c, E, N, False)
    F.same_attempts(o, first)
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            assert gpu_evaluate(tw, c, E, N, False) == want
            assert_launch(c, 0, (E * N + 15) // 16)
            assert same_bits(first, F.attempts()), hex(pattern)
    # another policy of other widths leaves its own image and results behind; then the first again, hook off
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(make_deep_policy_arrays_obs(c.arrs[0].shape[0], seed=5, emb=64, common=(96, 48), n_actions=c.A,
                                                                                         scale=1.0), *c.tw)})
    gpu_evaluate(tw, other, E, N, False)
    assert_launch(c, 0, (E * N + 15) // 16)
    assert gpu_evaluate(tw, c, E, N, False) == want
    assert same_bits(first, F.attempts())


def test_on_a_callers_stream(tw, O):
    import torch
    from tests import stream_util as su
    from twisterl_amd import _lib
    c = CASES["x2:gw3_exact"]()
    E, N = 34, 3
    want, first = evaluate_twice(tw, c, E, N, False)
    stream = su.independent_stream()
    try:
        with _lib.library_stream(stream):
            busy = su.delay(su.null_stream(), 40.0)
            got = gpu_evaluate(tw, c, E, N, False)
            ran_beside = not busy.query()
            assert_launch(c, 0, (E * N + 15) // 16)
            mine = F.attempts()
    finally:
        torch.cuda.synchronize()
    assert ran_beside, "the evaluate on the caller's stream waited for the null stream's work"
    assert got == want and same_bits(first, mine)


# ---- what the kernel does not take keeps its path and its message -----------------------------------------------------------------------------------
def test_refusals_and_unchanged_paths(tw, O):
    from twisterl_amd import _lib
    arrs = _general("deep_36_40_20").arrs
    gp = amd_policy(arrs)
    mfma = amd_policy(make_policy_arrays_obs(GW.obs_size, seed=3, emb=64, hidden=64, n_actions=4))
    env_all, env_new, env_x2, env_s, env_d = (_gw_env(m) for m in (GW_ALL, GW_X2S, GW_X2, F.GW_S, F.GW_DEFAULT))
    assert env_all.fp16x2_solve and env_all.search and env_all.fp16_search and env_all.fp16_solve and env_new.fp16x2_solve
    assert env_x2.fp16x2 and not env_x2.fp16x2_solve and env_s.fp16_solve and not env_s.fp16x2_solve and not env_d.fp16x2_solve and not env_d.fp16
    ev = lambda env, pol, prec, mcts=0: tw.collector.evaluate(env, pol, 20, True, 2, mcts, 5, C_UCB, 1, 1, precision=prec)
    so = lambda env, pol, prec, mcts=0: tw.collector.solve(D.start(env, 3, 3, 1), pol, True, 2, mcts, C_UCB, 1, seed=5, precision=prec)
    for call in (ev, so):
        for refused in (lambda: call(env_all, gp, "fp16x2", 4),           # MCTS-guided, on a module that has every flag
                        lambda: call(env_x2, gp, "fp16x2"),               # a module built with fp16x2=True alone
                        lambda: call(env_s, gp, "fp16x2"),                # ... with fp16_solve=True alone
                        lambda: call(env_d, gp, "fp16x2"),                # a default module
                        lambda: call(env_new, mfma, "fp16x2")):           # an MFMA-shape policy
            assert F._message(refused) == F32_ONLY
            assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    az = lambda env: tw.collector.AZCollector(16, 4, C_UCB, 1, 4, precision="fp16x2").collect(env, gp, seed=1)
    assert F._message(lambda: az(env_all)) == (RuntimeError, "tw_az_collect_env: f32 only")
    # precision="fp32" on the new module: the f32 kernel, and a default module's bytes
    for call, from_state in ((ev, 0), (so, 1)):
        a = call(env_new, gp, "fp32")
        info = _lib.debug_last_launch()
        assert (info["family"], info["nw"], info["nc"], info["solve"]) == (_lib.TW_KERNEL_SOLVE_BIG, 0, 9, from_state), info
        sa = F.attempts()
        b = call(env_d, gp, "fp32")
        assert a == b and same_bits(sa, F.attempts())
        assert call(env_new, gp, "fp32") == call(env_new, gp, "exact") == a
    ev(env_all, gp, "fp16")                                               # fp16 on the module with every flag: the fp16 kernel
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_SOLVE_BIG, 16)
    ev(env_all, gp, "fp16x2")                                             # ... and the split one
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_SOLVE_BIG, NW_SPLIT)
    ev(env_all, gp, "fp32", 4)                                            # MCTS in f32 on it: the search kernel, as ever
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_MCTS_BIG
    from tests.test_gpu_device_env_fp16x2 import GAMMA, LAM
    tw.collector.PPOCollector(40, GAMMA, LAM, 4, precision="fp16x2").collect(env_new, gp, seed=1)   # the fp16x2 collect still runs
    info = _lib.debug_last_launch()
    assert (info["family"], info["nw"]) == (_lib.TW_KERNEL_ROLLOUT_BIG, NW_SPLIT), info
