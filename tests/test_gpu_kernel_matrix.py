"""GPU: every rollout kernel the build ships (tests/kernel_matrix.py, one row each) against the oracle and the float64 bound,
and the operand range of the two f16 modes.

Per row the launch shape in `stats` is first held to the restated dispatch -- that is what proves the row ran the kernel it
names.  Then:
* fp32 rows: the whole collect bit-exact to the oracle's ARITH_CHAIN, and logits / values / advantages / returns inside the
  float64 bound of the f32 mode (tests/ref64.py forward_f64_bound, gae_bound_episodes);
* fp16 rows: per-record replay parity with ARITH_F16 (test_gpu_parity._check_f16_collect) and inside the fp16 bound;
* fp16x2 rows: replay parity within 1e-5 of ARITH_REF and inside the fp16x2 bound.
Persistent rows reserve all CUs but one (reserve_cus), so that 300 episodes already take the queue of the one workgroup left.

Range cases (Puzzle-8 and Puzzle-15): a hidden unit at ~250 (inside the split's range) and ~300 (outside), an embedding unit at
~4000 / ~5000, a head weight of 5000, weights below 2^-18, an embedding without ReLU at -5000.  fp16x2 either runs its own kernel
inside its bound or -- outside its range -- returns the fp32 mode's bytes from the fp32 kernel; fp16 matches its spec in all.
"""
import os

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests.ref64 import MASKED, forward_f64_bound, gae_bound_episodes, gae_f64_episodes, max_activations
from tests.test_gpu_parity import _assert_same_collect, _check_f16_collect
from tests.util import make_deep_policy_arrays, make_policy_arrays, puzzle_transpose_twist
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu
G = 0.995


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _policy(tw, arrs, op, ap, emb_relu=True):
    emb, eb, common, action, value = arrs
    seq = lambda ls: tw.nn.Sequential([tw.nn.Linear(np.asarray(w).tolist(), np.asarray(b).tolist(), r) for (w, b, r) in ls])
    return tw.nn.Policy(tw.nn.EmbeddingBag(emb.tolist(), eb.tolist(), emb_relu, [emb.shape[0]], 0), seq(common), seq(action), seq(value),
                        [list(p) for p in op], [list(p) for p in ap])


def _collect(tw, row, gp, cus, seed, merge_order):
    opts = []
    if row.force_geom:
        opts.append(_lib.launch_option(_lib.TW_OPT_FORCE_GEOM, row.force_geom))
    if row.no_persist:
        opts.append(_lib.launch_option(_lib.TW_OPT_NO_PERSIST, 1))
    coll = tw.collector.PPOCollector(row.E, G, G, 32, merge_order=merge_order, precision=row.prec, reserve_cus=km.reserve_cus(row, cus))
    for o in opts:
        o.__enter__()
    try:
        return coll.collect(tw.env.Puzzle(row.w, row.h, row.diff, 2, 256), gp, seed=seed)
    finally:
        for o in reversed(opts):
            o.__exit__(None, None, None)


def _check_bounds(a, arrs, op, ap, mode, label, emb_relu=True, also_1e5=False):
    """GPU logits / values / advs / rets against forward_f64 + gae_f64 of the GPU's own records, inside the mode's bound."""
    L = a["ep_len"].astype(np.int64)
    masks = a["logits"] != np.float32(MASKED)
    l64, v64, el, ev = forward_f64_bound(arrs, op, ap, a["obs"].astype(np.int64), masks, a["perms"].astype(np.int64), mode, emb_relu=emb_relu)
    dl = np.abs(a["logits"].astype(np.float64) - l64)
    dv = np.abs(a["values"].astype(np.float64) - v64)
    assert np.all(dl[masks] <= el[masks]), (label, float(np.max(dl[masks] - el[masks])))
    assert np.all(dv <= ev), (label, float(np.max(dv - ev)))
    a64, r64 = gae_f64_episodes(a["rewards"], v64, L, G, G)
    ea, er = gae_bound_episodes(a["rewards"], v64, ev, L, G, G)
    da, dr = np.abs(a["advs"] - a64), np.abs(a["rets"] - r64)
    assert np.all(da <= ea) and np.all(dr <= er), (label, float(np.max(da - ea)), float(np.max(dr - er)))
    if also_1e5:
        small = el[masks] < 1e-5
        assert np.all(dl[masks][small] < 1e-5) and np.all(dv[ev < 1e-5] < 1e-5), label
    return float(np.max(dl[masks])), float(np.max(dv))


def _row_policy(oracle, row, seed=None):
    """The row's policy arrays and twists; `seed`: other weights of the same shapes (default: the row's index in the table)."""
    n2 = row.w * row.h
    op, ap = puzzle_transpose_twist(row.w) if row.twists else ([], [])
    seed = km.TABLE.index(row) if seed is None else seed
    if row.common is not None:
        arrs = make_deep_policy_arrays(n2, seed=seed, emb=row.emb, common=row.common, scale=2.0)
    else:
        arrs = make_policy_arrays(n2, seed=seed, emb=row.emb, hidden=row.hidden)
    return arrs, op, ap


def check_row(tw, oracle, cus, row):
    """One row of the table: the launch shape, then the oracle and the float64 bound.  -> the collect that was checked."""
    arrs, op, ap = _row_policy(oracle, row)
    gp, opol = _policy(tw, arrs, op, ap), oracle.Policy(*arrs, op, ap)
    seed = 100 + km.TABLE.index(row)
    kernel, shape = km.dispatch(row, cus)
    label = km.kernel_name(kernel)
    g = _collect(tw, row, gp, cus, seed, merge_order=False)      # records in episode order (the bounds' GAE walks them so)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == shape, (label, g.stats)
    if row.prec == "fp32":
        o = oracle.ppo_collect(oracle.Puzzle(row.w, row.h, row.diff, 2, 256), opol, row.E, G, G, seed=seed, arith=oracle.ARITH_CHAIN,
                               det_log=True, merge_order=False, num_threads=_threads())
        _assert_same_collect(g, o, row.w * row.h)
        _check_bounds(g.to_numpy(), arrs, op, ap, "f32", label)
        return g
    a = g.to_numpy()
    n_perms = len(op)
    if row.prec == "fp16":
        _check_f16_collect(oracle, a, opol, row.w, row.h, row.diff, seed, n_perms, range(row.E))
        _check_bounds(a, arrs, op, ap, "fp16", label)
    else:
        worst = _check_f16_collect(oracle, a, opol, row.w, row.h, row.diff, seed, n_perms, range(row.E), arith=oracle.ARITH_REF, atol=1e-5)
        assert worst < 1e-5, (label, worst)
        _check_bounds(a, arrs, op, ap, "fp16x2", label, also_1e5=True)
    return g


@pytest.mark.parametrize("row", km.TABLE, ids=[km.row_id(r) for r in km.TABLE])
def test_every_rollout_kernel_against_the_oracle_and_the_f64_bound(tw, oracle, cus, row):
    check_row(tw, oracle, cus, row)


# ------------------------------------------------------------------------------ operand range of the f16 modes
def _range_case(n2, case):
    """-> (policy arrays, emb_relu, inside fp16x2's range?) for make_policy_arrays(n2, seed=3, emb=64, hidden=32) with one edit."""
    emb, eb, common, action, value = make_policy_arrays(n2, seed=3, emb=64, hidden=32)
    (w1, b1, r1), = common
    (wa, ba, ra), = action
    w1, b1, wa, eb, emb = w1.copy().reshape(64, 32), b1.copy(), wa.copy(), eb.copy(), emb.copy()
    relu, inside = True, True
    if case == "h1_250":
        b1[5] = 250.0                       # |sum W1 h0| < 5 here: h1[5] in [245, 255] < 255.94
    elif case == "h1_300":
        b1[5], inside = 300.0, False
    elif case in ("h0_4000", "h0_5000"):
        w1[7, :] = 0.0                      # the unit feeds nothing: only the embedding's own range is at stake
        eb[7] = 4000.0 if case == "h0_4000" else 5000.0
        inside = case == "h0_4000"
    elif case == "head_5000":
        wa[0], inside = 5000.0, False
    elif case == "tiny":
        f = np.float32(2.0 ** -20)          # every |weight| below 2^-18: even 16 x weight is an f16 subnormal
        emb, eb, w1, b1, wa, ba = emb * f, eb * f, w1 * f, b1 * f, wa * f, ba * f
        value = [(value[0][0] * f, value[0][1] * f, False)]
    elif case == "no_relu_neg":
        w1[7, :] = 0.0
        eb[7], relu, inside = -5000.0, False, False
    arrs = (emb, eb, [(w1.reshape(-1), b1, r1)], [(wa, ba, ra)], value)
    return arrs, relu, inside


RANGE_CASES = ["h1_250", "h1_300", "h0_4000", "h0_5000", "head_5000", "tiny", "no_relu_neg"]


def check_range_case(tw, oracle, cus, w, case):
    """One operand-range case of the f16 modes.  -> (the fp16x2 collect, inside the split's range?)"""
    n2, E, diff, seed = w * w, 300, 4, 7
    arrs, relu, inside = _range_case(n2, case)
    gp, opol = _policy(tw, arrs, [], [], emb_relu=relu), oracle.Policy(*arrs, emb_relu=relu)
    env = tw.env.Puzzle(w, w, diff, 2, 256)
    run = lambda prec: tw.collector.PPOCollector(E, G, G, 32, merge_order=False, precision=prec).collect(env, gp, seed=seed)
    obs = np.arange(n2)[None, :] * n2 + np.argsort(np.random.default_rng(0).random((64, n2)), axis=1)
    m0, m1 = max_activations(arrs, [], [], obs, np.full(64, -1), emb_relu=relu)
    # fp16 (a reduced-precision mode): its spec, ARITH_F16, at every case (all below 65504); tolerance grows with the activations
    a16 = run("fp16").to_numpy()
    assert max(m0, m1) < 65504 / 2
    _check_f16_collect(oracle, a16, opol, w, w, diff, seed, 0, range(E), atol=1e-4 * max(1.0, m0, m1))
    _check_bounds(a16, arrs, [], [], "fp16", f"fp16/{case}", emb_relu=relu)
    # fp16x2: inside its range its own kernel within its bound, outside the fp32 mode's bytes from the fp32 kernel
    g2 = run("fp16x2")
    g32 = run("fp32")
    a2, a32 = g2.to_numpy(), g32.to_numpy()
    shape = lambda g: (g.stats["rollout_blocks"], g.stats["rollout_threads"])
    assert shape(g32) == km.dispatch(km.R(w, w, 64, 32, E, diff=diff), cus)[1]
    if inside:
        assert shape(g2) == km.dispatch(km.R(w, w, 64, 32, E, "fp16x2", diff=diff), cus)[1]
        assert np.isfinite(a2["logits"]).all() and np.isfinite(a2["values"]).all()
        _check_f16_collect(oracle, a2, opol, w, w, diff, seed, 0, range(E), arith=oracle.ARITH_REF, atol=1e-5 * max(1.0, m1))
        _check_bounds(a2, arrs, [], [], "fp16x2", f"fp16x2/{case}", emb_relu=relu)
    else:
        assert shape(g2) == shape(g32), (case, g2.stats)
        for k in a32:
            assert np.array_equal(a2[k], a32[k]), (case, k)
    return g2, inside


@pytest.mark.parametrize("w", [3, 4])
@pytest.mark.parametrize("case", RANGE_CASES)
def test_f16_modes_at_the_edges_of_their_operand_range(tw, oracle, cus, w, case):
    check_range_case(tw, oracle, cus, w, case)
