"""GPU: AZCollector(precision="fp16").collect and collector.evaluate / collector.solve with num_mcts_searches > 0 and precision="fp16"
of device environments -- mcts_env16_kernel over EngineV16 (twisterl_amd/csrc/tw_mcts_env.hpp, tw_env_mcts_loop.hpp,
tw_engine_generic16.hpp), modules built with build_device_env(..., fp16_search=True) beside search=True or wide_search=True.

A search turns a last-bit difference of a prior into another visit count, so nothing is compared within a tolerance.  Two tiers, as
tests/test_gpu_device_env_fp16_solve.py (whose helpers this file imports):

A  EXACT ARITHMETIC.  Policies from exact_arrays(): every activation along the oracle's own ARITH_F16 trajectories is an integer or a
   half-integer below 1024 -- asserted on the CPU over EVERY state the oracle's searches evaluate, roots and leaves, before the GPU is
   touched.  Every sum of the forward is then exact in any order, everything behind the heads is the same f32 code in the same order,
   and the collected data (obs, MCTS probabilities, remaining values, episode lengths and order), every attempt's (success, total,
   n_steps) and solve's ((success, reward), actions) must be bit for bit the oracle's: oracle.mcts_probs_env / oracle.solve_env with
   arith=ARITH_F16 over the module's host code.
B  GENERAL WEIGHTS, gated where float64 decides.  oracle.mcts_probs_env restated with intervals along the oracle's ARITH_F16 trajectory:
   every prior is masked_softmax_f64 +- ref64.prob_bound, every network value +- err_values (ref64.full_predict_f64_bound(mode="fp16")),
   value_sum carries its accumulated error and the rounding of each addition, each UCB term the rounding of its operations.  A descent is
   decided when the chosen child's lower end is above every other child's upper end, a weighted sample as decided_attempts decides one.
   An episode of decided steps only is what ANY conforming f16-input implementation produces: there the GPU must equal the oracle bit
   for bit; the others are not compared, and at most a quarter of a case's episodes may be such (asserted on the CPU first).

Then what the kernel does not take: the messages and paths of before, exact."""
import functools
import signal
from types import SimpleNamespace

import numpy as np
import pytest

from tests import device_env_solve as D
from tests import ref64
from tests import test_gpu_device_env_fp16_solve as F
from tests.device_env_matrix import BY_MODULE as PROBE_ROWS_BY_MODULE, PROBE_HPP, engine_nc, host_env
from tests.device_env_matrix import twists as probe_twists
from tests.device_env_util import GRIDWORLD_HPP, RING_HPP
from tests.device_env_wide_search import BY_MODULE as WIDE_ROWS_BY_MODULE, twists as wide_twists
from tests.test_gpu_device_env_fp16 import GW, WIDTHS, activation_ceiling
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs, make_policy_arrays_obs, oracle_policy
from tests.var_obs_util import LAMPS_HPP, _pad, lamps_twists

pytestmark = pytest.mark.gpu

exact_arrays, assert_exact_along, _message, means_of, attempts, same_attempts = \
    F.exact_arrays, F.assert_exact_along, F._message, F.means_of, F.attempts, F.same_attempts

# search: yes in the matrix (probe_o64a4s is built without the search kernel there); NC 4, 9, 25, 64; observe_n, twists, A < 4;
# probe_o64a2sv: a struct of 128 bytes that lives in scratch memory
PROBE_ROWS = ("probe_o1a1", "probe_o5a3v", "probe_o17a2", "probe_o64a2sv")
SCRATCH_ROW = "probe_o64a2sv"
WIDE_ROW = "wideo17a17_ws"                                                    # A > 4: forward_head + the LDS row of probabilities
F16_MAX = 65504.0
C_UCB = 1.41
AZ_F32_ONLY = (RuntimeError, "tw_az_collect_env: f32 only")
GW_Z, GW_ALL, GW_SOLVE_AZ, GW_AZ = "gridworld3x3_f16az", "gridworld3x3_f16sz", "gridworld3x3_fp16s_az", "gridworld3x3_az"
# self-play: episodes, searches, max_expand_depth -- 2.5 and 2.1 workgroups of 16 columns
PLAYS = ((40, 4, 1), (34, 8, 1))
# evaluate: episodes, attempts, deterministic, searches
EVALS = ((40, 1, True, 4), (34, 3, False, 4))


@pytest.fixture(autouse=True)
def _time_limit():
    def boom(*_):
        raise TimeoutError("fp16 search device-environment test exceeded its time limit")
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


def _jobs():
    z = {"fp16_search": True, "search": True}
    jobs = [(PROBE_HPP, PROBE_ROWS_BY_MODULE[m].alias, m + "_f16az", z) for m in PROBE_ROWS]
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    jobs += [(r.header, r.type, WIDE_ROW + "_f16", {"fp16_search": True, "wide_search": True})]
    jobs += [(RING_HPP, "RingWalk", "ring_f16az", z), (LAMPS_HPP, "Lamps12", "lamps12_f16az", z)]
    jobs += [(GRIDWORLD_HPP, GW.type, GW_Z, z), (GRIDWORLD_HPP, GW.type, GW_ALL, {"fp16_search": True, "fp16_solve": True, "search": True}),
             (GRIDWORLD_HPP, GW.type, GW_SOLVE_AZ, {"fp16_solve": True, "search": True}), (GRIDWORLD_HPP, GW.type, GW_AZ, {"search": True})]
    return jobs


@functools.lru_cache(maxsize=None)
def build_all():
    """Every module of this file, built once per session side by side, AT MOST 16 AT A TIME -> {name: path}."""
    from concurrent.futures import ThreadPoolExecutor
    from twisterl_amd.build import build_device_env
    jobs = _jobs()
    assert len(jobs) <= 16
    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as pool:
        paths = list(pool.map(lambda j: build_device_env(j[0], j[1], j[2], **j[3]), jobs))
    return {j[2]: p for j, p in zip(jobs, paths)}


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------
class Case(SimpleNamespace):
    """env, arrs, tw, the oracle's policy `op`; the library's policy `gp` is made on first use (it needs a device)."""

    @property
    def gp(self):
        if self._gp is None:
            self._gp = amd_policy(self.arrs, *self.tw)
        return self._gp


def _case(name, env, arrs, tws, n_obs, A, diff, seed, offset=0):
    from oracle import oracle as O_
    return Case(name=name, env=env, arrs=arrs, tw=tws, _gp=None, op=oracle_policy(O_, arrs, *tws), n_obs=n_obs, A=A, diff=diff, seed=seed,
                offset=offset, nc=engine_nc(n_obs))


def _gw_env(module=GW_Z):
    from twisterl_amd.env import DeviceEnv
    return DeviceEnv(build_all()[module], module, [3, 3, GW.max_steps, GW.diff], max_records=GW.max_steps + 1)


def _gw_case(name, arrs, module=GW_Z, seed=GW.seed):
    return _case(name, _gw_env(module), arrs, ((), ()), GW.n_obs, GW.A, GW.diff, seed)


@functools.lru_cache(maxsize=None)
def _gw_exact(key):
    emb, common = WIDTHS[key]
    return _gw_case("gw3_exact_" + key, exact_arrays(GW.obs_size, emb, common, (), (), 4, seed=300 + len(key)))


@functools.lru_cache(maxsize=None)
def _probe_exact(module):
    from twisterl_amd.env import DeviceEnv
    r = PROBE_ROWS_BY_MODULE[module]
    name = module + "_f16az"
    env = DeviceEnv(build_all()[name], name, [r.obs_size, r.max_steps, r.diff, -1], max_records=r.max_steps + 1)
    arrs = exact_arrays(r.obs_size, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=400 + r.seed)
    return _case(module + "_exact", env, arrs, probe_twists(module), r.n_obs, r.A, r.diff, r.seed, r.offset)


@functools.lru_cache(maxsize=None)
def _wide_exact():
    from twisterl_amd.env import DeviceEnv
    r = WIDE_ROWS_BY_MODULE[WIDE_ROW]
    name = WIDE_ROW + "_f16"
    env = DeviceEnv(build_all()[name], name, list(r.params), max_records=r.max_records)
    # k=4: with the default density some leaf's 17 logits pass 88, its exponentials overflow and it gets no child at all -- which the
    # oracle, like the reference, cannot run (tests/device_env_wide_search.py: SHUT)
    arrs = exact_arrays(r.obs_size, r.emb, r.common, r.policy_layers, r.value_layers, r.A, seed=400 + r.seed, k=4)
    return _case(WIDE_ROW + "_exact", env, arrs, wide_twists(WIDE_ROW), r.n_obs, r.A, r.diff, r.seed)


def _ring_twists(n):
    mir = lambda p: (n - p) % n
    ident = list(range(2 * n))
    flip = [mir(i) if i < n else n + mir(i - n) for i in range(2 * n)]
    return [ident, flip], [[0, 1, 2], [2, 1, 0]]


@functools.lru_cache(maxsize=None)
def _ring_exact():
    """RingWalk: three actions, full_predict averaged over two twists, and a step() that draws (the tree's actions are replayed through it)."""
    from twisterl_amd.env import DeviceEnv
    env = DeviceEnv(build_all()["ring_f16az"], "ring_f16az", [32, 12, 3, 0.25, -1], max_records=13)
    return _case("ring_exact", env, exact_arrays(64, 32, (48,), (), (), 3, seed=431), _ring_twists(32), 2, 3, 3, 43)


@functools.lru_cache(maxsize=None)
def _lamps_exact():
    """Lamps12: observe_n, records of 0 .. 12 ids."""
    from twisterl_amd.env import DeviceEnv
    env = DeviceEnv(build_all()["lamps12_f16az"], "lamps12_f16az", [11, 3, -1, 0], max_records=12)
    return _case("lamps_exact", env, exact_arrays(144, 32, (32, 16), (), (), 4, seed=432), tuple(lamps_twists(12)), 12, 4, 3, 44)


BUILDERS = {}
CASES = {**{"gw3_" + k: (lambda k=k: _gw_exact(k)) for k in sorted(WIDTHS)}, **{m: (lambda m=m: _probe_exact(m)) for m in PROBE_ROWS},
         "ring": _ring_exact, "lamps": _lamps_exact, WIDE_ROW: _wide_exact}
BUILDERS.update(CASES)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------------
class _Recording:
    """The oracle's policy with every state its full_predict is asked for kept: the roots and the leaves of the searches."""

    def __init__(self, policy):
        self._p, self.states = policy, []

    def __getattr__(self, name):
        return getattr(self._p, name)

    def full_predict(self, obs, masks, **kw):
        self.states.append((list(obs), list(masks)))
        return self._p.full_predict(obs, masks, **kw)


def _steps(c, states):
    """assert_exact_along's (ids, masks, twist, u) of the evaluated states: full_predict runs EVERY twist."""
    n = len(c.tw[0])
    return [(ids, masks, p, 0.0) for ids, masks in states for p in (range(n) if n else (-1,))]


def _unit(O, seed, key, t, stream):
    w = O.philox4x32_10([key & 0xFFFFFFFF, key >> 32, t, stream], [seed & 0xFFFFFFFF, seed >> 32])
    return float(np.float32(w[0] >> 8) * np.float32(1.0 / 16777216.0))


def _ids(e):
    return [int(x) for x in e.observe()]


def _masks(e):
    return [bool(m) for m in e.masks()]


def _move_probs(O, e, pol, c, S, med, seed, key, t, arith, gate):
    """-> (the MCTS probabilities of the move, decided).  Without a gate: oracle.mcts_probs_env itself."""
    if gate is None:
        return O.mcts_probs_env(e, pol, S, C_UCB, med, seed, key, t, arith=arith), True
    return gated_probs(O, e, pol, c, S, med, seed, key, t, gate)


@functools.lru_cache(maxsize=None)
def oracle_play(case_key, E, S, med, arith, seed=None, gated=False, merge_order=True):
    """oracle.az_collect_env restated with the played actions, the evaluated states and (gated) the decisions kept; computed once and
    shared, never modified -> SimpleNamespace(eps [(obs lists, probs, remaining values, actions, decided)], the merged arrays, states)."""
    from oracle import oracle as O
    c = BUILDERS[case_key]()
    seed = c.seed if seed is None else seed
    pol = _Recording(c.op)
    gate = Gate(c) if gated else None
    proto = host_env(c.env)
    f32 = np.float32
    eps = []
    for i in range(E):
        ep = c.offset + i
        e = proto.copy()
        e.seed_episode(seed, ep)
        e.reset(c.diff)
        obs_l, prob_l, val_l, act_l, decided, t = [], [], [], [], True, 0
        while True:
            mp, ok = _move_probs(O, e, pol, c, S, med, seed, ep, t, arith, gate)
            u = _unit(O, seed, ep, t, 3)
            action = O.sample_weighted(mp, u)
            obs_l.append(_ids(e)); prob_l.append(mp); val_l.append(f32(e.value()))
            if e.is_final():
                break
            decided = decided and ok and (gate is None or sample_decided(mp.astype(np.float64), mp.astype(np.float64), u))
            act_l.append(action)
            e.next(action)
            t += 1
        total, before = f32(0), []
        for v in val_l:
            before.append(total)
            total = f32(total + v)
        eps.append((obs_l, prob_l, [f32(total - b) for b in before], act_l, decided))
    order = ([E - 1] + list(range(E - 1))) if merge_order else list(range(E))
    n_of = [len(e[2]) for e in eps]
    lists = [o for i in order for o in eps[i][0]]
    cat = lambda k: np.concatenate([np.asarray(eps[i][k], dtype=np.float32).reshape(n_of[i], -1) for i in order])
    return SimpleNamespace(eps=eps, order=order, obs_lists=lists, obs=_pad(lists, c.n_obs), logits=cat(1), remaining_values=cat(2).reshape(-1),
                           ep_len=np.asarray(n_of, dtype=np.uint32), actions=[e[3] for e in eps], states=pol.states,
                           decided=np.asarray([e[4] for e in eps], bool))


def oracle_attempt(O, start, pol, c, det, seed, key, S, med, arith, gate=None):
    """One MCTS-guided attempt from `start` (not modified), keyed `key`: oracle.solve_env's loop with the decisions kept ->
    (success, total as f32, actions, decided)."""
    e = start.copy()
    total, acts, t, decided = np.float32(0), [], 0, True
    while not e.is_final():
        total = np.float32(total + np.float32(e.value()))
        mp, ok = _move_probs(O, e, pol, c, S, med, seed, key, t, arith, gate)
        decided = decided and ok
        if det:
            action, bv = 0, mp[0]
            for i in range(1, len(mp)):
                if mp[i] > bv:
                    action, bv = i, mp[i]
        else:
            u = _unit(O, seed, key, t, 5)
            action = O.sample_weighted(mp, u)
            decided = decided and (gate is None or sample_decided(mp.astype(np.float64), mp.astype(np.float64), u))
        e.next(action)
        acts.append(action)
        t += 1
    total = np.float32(total + np.float32(e.value()))
    return (1.0 if e.success() else 0.0), total, acts, decided


@functools.lru_cache(maxsize=None)
def oracle_evaluate(case_key, E, N, det, S, med, arith, seed=None):
    """Every attempt of an MCTS-guided evaluate (episode e from reset(seed, offset + e), attempt k keyed (offset + e) N + k) -> the fields
    of tests/test_gpu_device_env_fp16_solve.oracle_evaluate, and the evaluated states.  Held to oracle.solve_env, attempt by attempt."""
    from oracle import oracle as O
    c = BUILDERS[case_key]()
    seed = c.seed if seed is None else seed
    pol = _Recording(c.op)
    proto = host_env(c.env)
    out = SimpleNamespace(success=[], total=[], n_steps=[], acts=[])
    for ep in range(E):
        e = proto.copy()
        e.seed_episode(seed, c.offset + ep)
        e.reset(c.diff)
        for k in range(N):
            key = (c.offset + ep) * N + k
            s, tot, acts, _ = oracle_attempt(O, e, pol, c, det, seed, key, S, med, arith)
            if k == 0:
                (s2, r2), a2 = O.solve_env(e, c.op, det, 1, S, C_UCB, med, seed=seed, episode=key, arith=arith)
                assert (float(s2), f32_bits(r2), [int(x) for x in a2]) == (s, f32_bits(tot), acts), (c.name, key)
            out.success.append(s); out.total.append(tot); out.n_steps.append(len(acts)); out.acts.append(acts)
    out.success, out.total, out.n_steps = np.asarray(out.success, np.float32), np.asarray(out.total, np.float32), np.asarray(out.n_steps, np.uint32)
    out.means = means_of(out.success, out.total, E, N)
    out.states = pol.states
    return out


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------
def gpu_play(tw, c, E, S, med, precision="fp16", seed=None, merge_order=True, gp=None):
    seed = c.seed if seed is None else seed
    return tw.collector.AZCollector(E, S, C_UCB, med, 4, precision=precision, episode_offset=c.offset, merge_order=merge_order).collect(
        c.env, gp or c.gp, seed=seed)


def gpu_evaluate(tw, c, E, N, det, S, med=1, precision="fp16", seed=None):
    import ctypes as C
    from twisterl_amd import _lib
    seed = c.seed if seed is None else seed
    if c.offset == 0:
        return tw.collector.evaluate(c.env, c.gp, E, det, N, S, seed, C_UCB, med, 1, precision=precision)
    prm = _lib.SolveParams(int(det), N, S, C_UCB, med, seed, _lib.PRECISIONS[precision])
    s, r = C.c_float(), C.c_float()
    _lib.check(_lib.lib().tw_evaluate_device_env(*c.env._args(), c.gp._handle(), C.byref(prm), E, c.offset, c.env.max_records, C.byref(s), C.byref(r)))
    return float(s.value), float(r.value)


def assert_f16_search(c, columns, solve):
    """Which kernel ran: the search family with nw = 16 (mcts_env16_kernel), the module's engine width, one workgroup per 16 columns."""
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nt"], info["nc"], info["nw"], info["persist"], info["solve"], info["blocks"], info["threads"]) == \
        (_lib.TW_KERNEL_MCTS_BIG, 1, c.nc, 16, 0, solve, (columns + 15) // 16, 256), info
    return info


def play_arrays(g):
    a = g.to_numpy()
    return {k: np.array(v, copy=True) for k, v in a.items()}


def same_play(c, g, o, only=None):
    """Every field of the collected data against the oracle's; `only`: per episode, which to compare (the lengths of the others may
    differ, so the rows are cut by the device's own lengths: merge_order=False)."""
    a = g.to_numpy()
    assert a["obs"].shape[1] == c.n_obs and a["logits"].shape[1] == c.A and np.all(a["perms"] == -1)
    if only is None:
        assert np.array_equal(a["ep_len"], o.ep_len), (a["ep_len"], o.ep_len)
        if c.env.variable_obs:
            assert g.ragged and np.array_equal(a["obs"], o.obs) and g.obs == o.obs_lists
        else:
            assert np.array_equal(a["obs"].astype(np.int64), o.obs.astype(np.int64))
        assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
        assert np.array_equal(f32_bits(a["remaining_values"]), f32_bits(o.remaining_values))
        return
    assert o.order == list(range(len(o.eps)))
    at = np.concatenate([[0], np.cumsum(a["ep_len"].astype(np.int64))])
    for i, (obs_l, prob_l, rem, _acts, _d) in enumerate(o.eps):
        if not only[i]:
            continue
        n = len(rem)
        assert int(a["ep_len"][i]) == n, (i, int(a["ep_len"][i]), n)
        rows = slice(int(at[i]), int(at[i]) + n)
        assert np.array_equal(a["obs"][rows].astype(np.int64), np.asarray(obs_l, np.int64)), i
        assert np.array_equal(f32_bits(a["logits"][rows]), f32_bits(np.asarray(prob_l, np.float32))), i
        assert np.array_equal(f32_bits(a["remaining_values"][rows]), f32_bits(np.asarray(rem, np.float32))), i


def same_bytes(x, y):
    assert sorted(x) == sorted(y)
    for k in x:
        assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k


# ---- tier A ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("play", PLAYS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_self_play(tw, O, case, play):
    E, S, med = play
    c = CASES[case]()
    assert c.env.fp16_search and c.env.search and c.env.fp16
    o = oracle_play(case, E, S, med, O.ARITH_F16)
    assert_exact_along(c, _steps(c, o.states))                            # (on the CPU, before the GPU is touched)
    assert len(o.states) > E
    g = gpu_play(tw, c, E, S, med)
    assert_f16_search(c, E, 0)
    same_play(c, g, o)
    n_tw = max(len(c.tw[0]), 1)
    assert g.stats["forward_evals"] == len(o.states) * n_tw and g.stats["rollout_blocks"] == (E + 15) // 16
    first = play_arrays(g)
    same_bytes(first, play_arrays(gpu_play(tw, c, E, S, med)))            # twice the same
    assert_f16_search(c, E, 0)


@pytest.mark.parametrize("case,E,S,med", [("gw3_no_multiple", 34, 4, 2), ("gw3_no_common", 40, 1, 1), (WIDE_ROW, 34, 4, 2)],
                         ids=["depth2", "one_search", "wide_depth2"])
def test_exact_self_play_other_search_shapes(tw, O, case, E, S, med):
    """max_expand_depth 2 (next_sample's draw index it * 2 + expanded, two evaluations per search) and a single search per move."""
    c = CASES[case]()
    o = oracle_play(case, E, S, med, O.ARITH_F16)
    assert_exact_along(c, _steps(c, o.states))
    if case == "gw3_no_multiple":                                         # the restatement is the oracle's own collect
        ref = O.az_collect_env(host_env(c.env), c.op, E, S, C_UCB, med, seed=c.seed, difficulty=c.diff, arith=O.ARITH_F16)
        assert np.array_equal(ref.obs, o.obs.astype(np.int64)) and np.array_equal(f32_bits(ref.logits), f32_bits(o.logits))
        assert np.array_equal(f32_bits(ref.additional_data["remaining_values"]), f32_bits(o.remaining_values)) and np.array_equal(ref.ep_len, o.ep_len)
    g = gpu_play(tw, c, E, S, med)
    assert_f16_search(c, E, 0)
    same_play(c, g, o)
    same_bytes(play_arrays(g), play_arrays(gpu_play(tw, c, E, S, med)))


@pytest.mark.parametrize("shape", EVALS, ids=lambda s: f"{s[0]}x{s[1]}_{'det' if s[2] else 'sampled'}")
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_mcts_evaluate(tw, O, case, shape):
    E, N, det, S = shape
    c = CASES[case]()
    o = oracle_evaluate(case, E, N, det, S, 1, O.ARITH_F16)
    assert_exact_along(c, _steps(c, o.states))                            # (on the CPU, before the GPU is touched)
    got = gpu_evaluate(tw, c, E, N, det, S)
    assert_f16_search(c, E * N, 1)
    first = attempts()
    same_attempts(o, first)
    assert (f32_bits(got[0]), f32_bits(got[1])) == (f32_bits(o.means[0]), f32_bits(o.means[1])), (got, o.means)
    assert gpu_evaluate(tw, c, E, N, det, S) == got                       # twice the same
    assert all(np.array_equal(a, b) for a, b in zip(first, attempts()))


def test_the_exact_cases_play_different_actions_and_lengths(O):
    """No GPU: the cases above cannot pass for lack of variety."""
    for case in sorted(CASES):
        c = CASES[case]()
        o = oracle_play(case, 40, 4, 1, O.ARITH_F16)
        assert len(set(int(n) for n in o.ep_len)) >= (3 if c.A > 1 else 2), (case, sorted(set(int(n) for n in o.ep_len)))
        assert len(set(a for acts in o.actions for a in acts)) >= min(2, c.A), case
        e = oracle_evaluate(case, 34, 3, False, 4, 1, O.ARITH_F16)
        assert len(set(int(n) for n in e.n_steps)) >= (3 if c.A > 1 else 2), (case, sorted(set(int(n) for n in e.n_steps)))
    assert max(a for acts in oracle_play(WIDE_ROW, 40, 4, 1, O.ARITH_F16).actions for a in acts) >= 4


SOLVE_EPISODE = {"gw3_no_multiple": 5, "probe_o5a3v": 5, WIDE_ROW: 0}       # whose reset state is not final after one step


@pytest.mark.parametrize("N", [1, 8])
@pytest.mark.parametrize("case", ["gw3_no_multiple", "probe_o5a3v", WIDE_ROW])
def test_solve_from_a_stepped_state(tw, O, case, N):
    c = CASES[case]()
    S = 4
    D.start(c.env, c.seed, SOLVE_EPISODE[case], 1)                        # a state no reset gives
    assert not c.env.is_final()
    start = host_env(c.env)
    for det in (True, False):
        pol = _Recording(c.op)
        per = [oracle_attempt(O, start, pol, c, det, D.SEED, k, S, 1, O.ARITH_F16) for k in range(N)]
        assert_exact_along(c, _steps(c, pol.states))
        want = O.solve_env(start, c.op, det, N, S, C_UCB, 1, seed=D.SEED, arith=O.ARITH_F16)
        want = ((float(want[0][0]), float(want[0][1])), [int(a) for a in want[1]])
        before = c.env.state_bytes()
        got = tw.collector.solve(c.env, c.gp, det, N, S, C_UCB, 1, seed=D.SEED, precision="fp16")
        assert_f16_search(c, N, 1)
        assert c.env.state_bytes() == before
        assert D.same(got, want), (got, want)
        s, t, k = attempts()
        assert np.array_equal(s, f32_bits([p[0] for p in per])) and np.array_equal(t, f32_bits([p[1] for p in per])) and \
            np.array_equal(k, np.asarray([len(p[2]) for p in per], np.uint32))
        exact, success, total = D.replay(c.env, got[1])                   # the returned moves lead to the returned result
        assert exact and float(success) == got[0][0] and f32_bits(total) == f32_bits(got[0][1])
        assert D.same(tw.collector.solve(c.env, c.gp, det, N, S, C_UCB, 1, seed=D.SEED, precision="fp16"), got)


@functools.lru_cache(maxsize=None)
def _witness():
    """As the witness of tests/test_gpu_device_env_fp16_solve.py: the exact GridWorld policy 32-32-16 with action columns 0 and 1 made of
    the same integers, column 0 with the 2^-12 offsets and column 1 without; both get the largest bias, so the two lead wherever they
    are legal.  In ARITH_F16 their priors are equal and the first child wins every tie of the descent; in ARITH_CHAIN they differ."""
    emb, eb, common, action, value = exact_arrays(GW.obs_size, 32, (32, 16), (), (), 4, seed=77)
    w, b, relu = action[0]
    w = w.reshape(-1, 4).copy()
    w[:, 1] = np.round(w[:, 0])
    b = b.copy()
    b[0] = b[1] = np.float32(6.5)
    return _gw_case("gw3_witness", (emb, eb, common, [(np.ascontiguousarray(w).reshape(-1), b, relu)], value))


BUILDERS["witness"] = _witness


def test_rounding_witness(tw, O):
    E, S, med = 40, 4, 1
    c = _witness()
    f16 = oracle_play("witness", E, S, med, O.ARITH_F16)
    chain = oracle_play("witness", E, S, med, O.ARITH_CHAIN)
    assert_exact_along(c, _steps(c, f16.states))
    # on the CPU: the two logits tie in ARITH_F16 and differ in ARITH_CHAIN, and that changes the collected data
    tie = [c.op.forward(ids, [True] * 4, perm=-1, arith=O.ARITH_F16)[0] for ids, _ in f16.states]
    assert all(f32_bits(l[0]) == f32_bits(l[1]) for l in tie)
    untie = [c.op.forward(ids, [True] * 4, perm=-1, arith=O.ARITH_CHAIN)[0] for ids, _ in f16.states]
    assert any(l[1] > l[0] for l in untie)
    assert f16.logits.shape != chain.logits.shape or not np.array_equal(f32_bits(f16.logits), f32_bits(chain.logits)), \
        "ARITH_CHAIN and ARITH_F16 give the same self-play: the rounding to binary16 would not show"
    g = gpu_play(tw, c, E, S, med)
    assert_f16_search(c, E, 0)
    same_play(c, g, f16)
    g32 = gpu_play(tw, c, E, S, med, precision="fp32")                    # and the f32 kernel of the same module is the f32 arithmetic
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert (info["family"], info["nw"], info["nc"]) == (_lib.TW_KERNEL_MCTS_BIG, 0, 9), info
    same_play(c, g32, chain)


def test_update_from_torch_repacks_the_image(tw, O):
    import torch
    E, S, med = 40, 4, 1
    old = _gw_case("gw3_update_old", exact_arrays(GW.obs_size, 36, (40, 20), (), (), 4, seed=71))
    new = _gw_case("gw3_update_new", exact_arrays(GW.obs_size, 36, (40, 20), (), (), 4, seed=72))
    before = play_arrays(gpu_play(tw, old, E, S, med))
    we, be, cs, as_, vs = new.arrs
    state = {"embeddings.weight": torch.tensor(we.T.copy()).cuda(), "embeddings.bias": torch.tensor(be).cuda()}
    for name, layers in (("common", cs), ("action", as_), ("value", vs)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = torch.tensor(np.asarray(wl).reshape(-1, len(bl)).T.copy()).cuda()
            state[f"{name}.{2 * i}.bias"] = torch.tensor(np.asarray(bl)).cuda()
    old.gp.update_from_torch(state)
    g_after = gpu_play(tw, old, E, S, med)
    assert_f16_search(old, E, 0)
    after = play_arrays(g_after)
    fresh = play_arrays(gpu_play(tw, new, E, S, med))
    same_bytes(after, fresh)
    assert any(before[k].shape != after[k].shape or before[k].tobytes() != after[k].tobytes() for k in before)
    BUILDERS["update_new"] = lambda: new
    o = oracle_play("update_new", E, S, med, O.ARITH_F16)
    assert_exact_along(new, _steps(new, o.states))
    same_play(new, g_after, o)


@pytest.mark.parametrize("what", ["self_play", "evaluate"])
@pytest.mark.parametrize("case", ["gw3_no_multiple", SCRATCH_ROW, WIDE_ROW])
def test_no_result_depends_on_what_the_memory_held(tw, O, case, what):
    from twisterl_amd import _lib
    c = CASES[case]()
    if what == "self_play":
        E, S = 34, 4
        o = oracle_play(case, E, S, 1, O.ARITH_F16)

        def run(cc=c):
            g = gpu_play(tw, cc, E, S, 1)
            assert_f16_search(c, E, 0)
            return play_arrays(g), g
        want, g = run()
        same_play(c, g, o)
        equal = lambda x: same_bytes(x[0], want)
    else:
        E, N, S = 34, 3, 4
        o = oracle_evaluate(case, E, N, False, S, 1, O.ARITH_F16)

        def run(cc=c):
            r = gpu_evaluate(tw, cc, E, N, False, S)
            assert_f16_search(c, E * N, 1)
            return r, attempts()
        want = run()
        same_attempts(o, want[1])

        def equal(x):
            assert x[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(x[1], want[1]))
    for pattern in (0xFFFFFFFF, 0x00000001, 0x00000000):
        with _lib.debug_fill_memory(pattern):
            equal(run())
    # another policy of other widths leaves its own image, tree and results behind; then the first again, hook off
    other = Case(**{**vars(c), "_gp": amd_policy(make_deep_policy_arrays_obs(c.arrs[0].shape[0], seed=5, emb=64, common=(96, 48), n_actions=c.A,
                                                                             scale=1.0), *c.tw)})
    run(other)
    equal(run())


# ---- tier B ----------------------------------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24
TINY = 2.0 ** -149


def _rnd(lo, hi):
    """One f32 rounding of a result enclosed by [lo, hi]."""
    return lo - abs(lo) * U32 - TINY, hi + abs(hi) * U32 + TINY


def sample_decided(lo, hi, u):
    """sample_weighted over weights enclosed by [lo, hi] at the draw u: every comparison has the same outcome at both ends of the
    intervals -- the rule of tests/test_gpu_device_env_fp16_solve.decided_attempts, over any number of weights."""
    n = len(lo)
    u = float(np.float32(u))
    margin = (n + 2) * U32 * float(np.sum(hi))                            # the n additions of the total and the cumulative sums, the product
    t_lo, t_hi = u * float(np.sum(lo)) - margin, u * float(np.sum(hi)) + margin
    c_lo = c_hi = 0.0
    for a in range(n - 1):
        c_lo, c_hi = c_lo + float(lo[a]), c_hi + float(hi[a])
        if c_lo - margin > t_hi:                                          # cum > u total at both ends: this one, nothing behind it is compared
            return True
        if not c_hi + margin <= t_lo:                                     # neither: the ends disagree
            return False
    return True


class Gate:
    """Per evaluated state the enclosures any conforming f16-input implementation stays in: the priors, masked_softmax_f64 +- prob_bound,
    and the value, +- err_values (ref64.full_predict_f64_bound(mode="fp16")).  The oracle's own ARITH_F16 figures are held to them."""

    def __init__(self, c):
        self.c, self.seen = c, {}
        assert activation_ceiling(c.arrs, c.n_obs) < F16_MAX

    def enclose(self, ids, masks, probs, value):
        key = (tuple(ids), tuple(masks))
        if key not in self.seen:
            c = self.c
            l64, v64, el, ev = ref64.full_predict_f64_bound(c.arrs, c.tw[0], c.tw[1], np.asarray([ids], np.int64), mode="fp16")
            m = np.asarray([masks], bool)
            p64, ep = ref64.masked_softmax_f64(l64, m), ref64.prob_bound(l64, el, m)
            v, e = float(np.asarray(v64).reshape(-1)[0]), float(np.asarray(ev).reshape(-1)[0])
            self.seen[key] = (np.maximum(p64 - ep, 0.0)[0], (p64 + ep)[0], v - e, v + e)
        lo, hi, v_lo, v_hi = self.seen[key]
        p = np.asarray(probs, np.float64)
        assert np.all(lo <= p) and np.all(p <= hi) and v_lo <= float(value) <= v_hi, (ids, "the oracle's ARITH_F16 leaves the float64 enclosure")
        return lo, hi, v_lo, v_hi


def gated_probs(O, env, pol, c, S, med, seed, key, t, gate):
    """oracle.mcts_probs_env along its ARITH_F16 trajectory with every compared quantity enclosed -> (the probabilities, decided)."""
    f32 = np.float32
    A = c.A
    decided = True
    root = env.copy()
    ids, masks = _ids(root), _masks(root)
    probs, rv = pol.full_predict(ids, masks, arith=O.ARITH_F16)
    plo, phi, _, _ = gate.enclose(ids, masks, probs, rv)
    nodes = [dict(state=root, parent=-1, action=-1, prior=f32(0), plo=0.0, phi=0.0, visit=1, vsum=f32(0), vlo=0.0, vhi=0.0, children=[])]

    def expand(idx, pri, lo, hi):
        nonlocal decided
        for a in range(A):
            if not (lo[a] > 0 or hi[a] == 0):                             # a child exists where the prior is > 0
                decided = False
            if not (pri[a] > 0):
                continue
            st = nodes[idx]["state"].copy()
            st.next(a)
            nodes.append(dict(state=st, parent=idx, action=a, prior=f32(pri[a]), plo=float(lo[a]), phi=float(hi[a]), visit=0, vsum=f32(0),
                              vlo=0.0, vhi=0.0, children=[]))
            nodes[idx]["children"].append(len(nodes) - 1)
    expand(0, probs, plo, phi)
    Cf = float(f32(C_UCB))
    for it in range(S):
        idx = 0
        while nodes[idx]["children"]:
            par, best, best_ucb, enc = nodes[idx], None, f32(-np.inf), {}
            for ci in par["children"]:
                ch = nodes[ci]
                q = f32(0) if ch["visit"] == 0 else f32(ch["vsum"] / f32(ch["visit"]))
                d = f32(np.sqrt(f32(par["visit"])) / f32(f32(ch["visit"]) + f32(1)))
                d = f32(f32(C_UCB) * d)
                d = f32(d * ch["prior"])
                ucb = f32(q + d)
                if ucb > best_ucb:
                    best, best_ucb = ci, ucb
                q_lo, q_hi = (0.0, 0.0) if ch["visit"] == 0 else _rnd(ch["vlo"] / ch["visit"], ch["vhi"] / ch["visit"])
                sq = float(np.sqrt(float(par["visit"])))
                d_lo, d_hi = _rnd(sq, sq)
                d_lo, d_hi = _rnd(d_lo / (ch["visit"] + 1.0), d_hi / (ch["visit"] + 1.0))
                d_lo, d_hi = _rnd(Cf * d_lo, Cf * d_hi)
                d_lo, d_hi = _rnd(d_lo * ch["plo"], d_hi * ch["phi"])
                enc[ci] = _rnd(q_lo + d_lo, q_hi + d_hi)
                assert enc[ci][0] <= float(ucb) <= enc[ci][1]
            if any(enc[o][1] >= enc[best][0] for o in enc if o != best):
                decided = False
            idx = best
        value, v_lo, v_hi, expanded = f32(0), 0.0, 0.0, 0
        while expanded < med:
            st = nodes[idx]["state"]
            value = f32(st.value())
            v_lo = v_hi = float(value)
            if st.is_final():
                break
            ids, masks = _ids(st), _masks(st)
            pr, nv = pol.full_predict(ids, masks, arith=O.ARITH_F16)
            lo, hi, n_lo, n_hi = gate.enclose(ids, masks, pr, nv)
            expand(idx, pr, lo, hi)
            ch = nodes[idx]["children"]
            u = _unit(O, seed, key, it * med + expanded, 4 | (t << 8))
            if ch:
                if not sample_decided([nodes[x]["plo"] for x in ch], [nodes[x]["phi"] for x in ch], u):
                    decided = False
                idx = ch[O.sample_weighted([nodes[x]["prior"] for x in ch], u)]
            value, v_lo, v_hi = f32(nv), n_lo, n_hi
            expanded += 1
        j = idx
        while j >= 0:
            nodes[j]["vsum"] = f32(nodes[j]["vsum"] + value)
            nodes[j]["vlo"], nodes[j]["vhi"] = _rnd(nodes[j]["vlo"] + v_lo, nodes[j]["vhi"] + v_hi)
            assert nodes[j]["vlo"] <= float(nodes[j]["vsum"]) <= nodes[j]["vhi"]
            nodes[j]["visit"] += 1
            j = nodes[j]["parent"]
    mp = np.zeros(A, dtype=np.float32)
    for ci in nodes[0]["children"]:
        mp[nodes[ci]["action"]] = f32(nodes[ci]["visit"])
    sm = f32(0)
    for a in range(A):
        sm = f32(sm + mp[a])
    return ((mp / sm).astype(np.float32) if sm > 0 else np.full(A, f32(1.0) / f32(A), dtype=np.float32)), decided


# (the weights' seeds: chosen on the CPU, with the oracle alone, over the device struct's start states and the real Philox draws of the
# collect's seed 41.  Undecided episodes of 40 at the weights' seeds 61 / 62 / 65 -- deep, 4 searches: 4 / 3 / 3; deep, 8 searches:
# 7 / 4 / 8; flat, 4 searches: 8 / 6 / 10.  The cap of a quarter stays whatever the seed.)
GENERAL = {"deep_36_40_20_s4": dict(policy=dict(seed=61, emb=36, common=(40, 20), scale=0.5), S=4, seed=GW.seed),      # 4 of 40
           "deep_36_40_20_s8": dict(policy=dict(seed=61, emb=36, common=(40, 20), scale=0.5), S=8, seed=GW.seed),      # 7 of 40
           "flat_32_s4": dict(policy=dict(seed=62, emb=32, common=(), scale=0.5), S=4, seed=GW.seed)}                 # 6 of 40


@functools.lru_cache(maxsize=None)
def _general(key):
    g = GENERAL[key]
    return _gw_case("gw3_" + key, make_deep_policy_arrays_obs(GW.obs_size, n_actions=4, **g["policy"]), seed=g["seed"])


BUILDERS.update({k: (lambda k=k: _general(k)) for k in GENERAL})


@pytest.mark.parametrize("key", sorted(GENERAL))
def test_general_weights_where_float64_decides(tw, O, key):
    E, S = 40, GENERAL[key]["S"]
    c = _general(key)
    o = oracle_play(key, E, S, 1, O.ARITH_F16, gated=True, merge_order=False)
    ref = O.az_collect_env(host_env(c.env), c.op, E, S, C_UCB, 1, seed=c.seed, difficulty=c.diff, arith=O.ARITH_F16, merge_order=False)
    assert np.array_equal(f32_bits(ref.logits), f32_bits(o.logits)) and np.array_equal(ref.ep_len, o.ep_len)     # the restatement is the oracle
    undecided = int((~o.decided).sum())
    print(f"[fp16 search] {key} {E} episodes x {S} searches: {undecided} of {E} episodes undecided")
    assert 4 * undecided <= E, (key, undecided, E)                        # (on the CPU, before the GPU is touched)
    acts = set(a for acts_, d in zip(o.actions, o.decided) if d for a in acts_)
    lens = set(int(n) for n, d in zip(o.ep_len, o.decided) if d)
    assert len(acts) >= 2 and len(lens) >= 3, (acts, lens)
    g = gpu_play(tw, c, E, S, 1, merge_order=False)
    assert_f16_search(c, E, 0)
    same_play(c, g, o, only=o.decided)


# ---- what the kernel does not take keeps its path and its message -----------------------------------------------------------------------------------
def test_refusals_and_unchanged_paths(tw, O):
    from twisterl_amd import _lib
    arrs = make_deep_policy_arrays_obs(GW.obs_size, n_actions=4, seed=61, emb=36, common=(40, 20), scale=0.5)
    gp = amd_policy(arrs)
    mfma = amd_policy(make_policy_arrays_obs(GW.obs_size, seed=3, emb=64, hidden=64, n_actions=4))
    env_z, env_all, env_saz, env_az = (_gw_env(m) for m in (GW_Z, GW_ALL, GW_SOLVE_AZ, GW_AZ))
    assert env_z.fp16_search and not env_z.fp16_solve and env_all.fp16_search and env_all.fp16_solve
    assert env_saz.fp16_solve and env_saz.search and not env_saz.fp16_search and env_az.search and not env_az.fp16 and not env_az.fp16_search
    az = lambda env, pol, prec: tw.collector.AZCollector(20, 4, C_UCB, 1, 4, precision=prec).collect(env, pol, seed=5)
    ev = lambda env, pol, prec, mcts=4: tw.collector.evaluate(env, pol, 20, True, 2, mcts, 5, C_UCB, 1, 1, precision=prec)
    so = lambda env, pol, prec, mcts=4: tw.collector.solve(D.start(env, 3, 3, 1), pol, True, 2, mcts, C_UCB, 1, seed=5, precision=prec)
    for call, want in ((az, AZ_F32_ONLY), (ev, F.F32_ONLY), (so, F.F32_ONLY)):
        for refused in (lambda: call(env_saz, gp, "fp16"),                # fp16 search on a module with fp16_solve and search, no fp16_search
                        lambda: call(env_az, gp, "fp16"),                 # a default search module
                        lambda: call(env_z, mfma, "fp16"),                # an MFMA-shape policy
                        lambda: call(env_z, gp, "fp16x2"),                # the split mode
                        lambda: call(env_all, gp, "fp16x2")):
            assert _message(refused) == want
            assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
    # the host-stepped collect itself
    from tests.device_env_search_util import _vtable
    import ctypes as C
    prm = _lib.AZParams(20, 0, 4, C_UCB, 1, 5, _lib.TW_PREC_F16, 1, 0)
    out = C.c_void_p()
    assert _lib.lib().tw_az_collect_env(C.byref(_vtable(env_z)), gp._handle(), C.byref(prm), env_z.max_records, C.byref(out)) != _lib.TW_OK
    assert _lib.last_error() == AZ_F32_ONLY[1]
    # precision="fp32" on the new module: the f32 search kernel, and a default search module's bytes
    a = az(env_z, gp, "fp32")
    info = _lib.debug_last_launch()
    assert (info["family"], info["nw"], info["nc"], info["solve"]) == (_lib.TW_KERNEL_MCTS_BIG, 0, 9, 0), info
    same_bytes(play_arrays(a), play_arrays(az(env_az, gp, "fp32")))
    same_bytes(play_arrays(a), play_arrays(az(env_z, gp, "exact")))
    for call in (ev, so):
        x = call(env_z, gp, "fp32")
        info = _lib.debug_last_launch()
        assert (info["family"], info["nw"], info["nc"], info["solve"]) == (_lib.TW_KERNEL_MCTS_BIG, 0, 9, 1), info
        sx = attempts()
        y = call(env_az, gp, "fp32")
        assert x == y and all(np.array_equal(p, q) for p, q in zip(sx, attempts()))
    # fp16 without MCTS on a module that holds both f16 attempt kernels: solve_env16_kernel; with MCTS: the new kernel
    ev(env_all, gp, "fp16", 0)
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_SOLVE_BIG, 16)
    ev(env_all, gp, "fp16", 4)
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_MCTS_BIG, 16)
    az(env_all, gp, "fp16")
    assert (_lib.debug_last_launch()["family"], _lib.debug_last_launch()["nw"]) == (_lib.TW_KERNEL_MCTS_BIG, 16)
    # ... and fp16 without MCTS on the module WITHOUT fp16_solve keeps the message
    assert _message(lambda: ev(env_z, gp, "fp16", 0)) == F.F32_ONLY
    assert _lib.debug_last_launch()["family"] == _lib.TW_KERNEL_NONE
