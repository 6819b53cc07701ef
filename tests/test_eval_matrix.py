"""The table of tests/eval_matrix.py, pinned on the CPU: every row reaches the branch of tw_eval.hip its comment names, the
oracle's three modes run on every row (action counts other than four, free slots) and lie inside the float64 bounds of
tests/ref64.py, the new float64 functions agree with a case worked by hand and with torch, and results mutated the way a wrong
kernel would mutate them leave the bounds."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import eval_matrix as M
from tests import ref64
from tests.eval_matrix import FORWARD, FULL_PREDICT, PREDICT
from tests.util import f32_bits

IN_RANGE = [r for r in M.TABLE if r.in_range]
ids = lambda rows: [r.name for r in rows]


def inside(got, want, bound):
    """|got - want| <= bound everywhere; a nan or inf in `got` is outside"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return bool(np.all(d <= bound))


def legal_logits(O, row, wp=True):
    l, _ = M.oracle_results(O, row)[(FORWARD, wp)]
    return l[M.records(row)[1] != 0]


# ------------------------------------------------------------------------------------------------ the table itself
def test_the_table_covers_the_list():
    for kind in ("basic", "generic"):
        rows = [r for r in M.TABLE if r.kind == kind]
        assert {1, 2, 3, 5, 30, 31} <= {M.n_actions(r) for r in rows}, kind
        assert {None, 1, 2, 3} <= {r.twists and r.twists[0] for r in rows}, kind
        for what in ("ragged", "free", "nobs1", "nobs64", "tw1", "tw2", "tw3", "notwist", "allmasked", "onelegal", "maskbytes", "eps",
                     "norelu-emb", "norelu-common", "exp"):
            assert f"{kind}-{what}" in M.BY_NAME, (kind, what)
    for name in ("basic-emb288-a5", "basic-emb512-a31", "generic-obs300-tw2", "generic-w512", "generic-w300", "generic-w30", "generic-value3",
                 "generic-nocommon", "generic-noaction", "generic-novalue", "generic-8common", "generic-8heads", "cross-basic", "cross-generic"):
        assert name in M.BY_NAME, name
    for r in M.TABLE:
        assert r.n <= 64 and 1 <= r.n_obs <= 64, r.name
        assert M.is_basic_shape(r) == (r.kind == "basic"), r.name           # the kernel the row is written for is the one that runs it
        obs, masks, perms = M.records(r)
        T = len(M.twists(r)[0])
        assert obs.min() >= -1 and obs.max() < r.obs_size and perms.min() >= -1 and perms.max() < max(T, 0)
        assert set(range(-1, T)) <= set(perms.tolist()), r.name             # every twist, and none, in every row
        for p in M.twists(r)[0]:
            assert sorted(p) == list(range(r.obs_size))
        for p in M.twists(r)[1]:
            assert sorted(p) == list(range(M.n_actions(r)))


def test_rows_reach_what_their_comments_claim(oracle):
    T = M.BY_NAME
    widths = lambda r: [b.size for (_, b, _) in M.policy_arrays(r)[2] + M.policy_arrays(r)[3] + M.policy_arrays(r)[4]]
    for kind in ("basic", "generic"):
        obs, masks, _ = M.records(T[f"{kind}-ragged"])
        assert obs[0, 0] == -1 and obs[0, 1] >= 0 and obs[0, 2] == -1                       # a free slot before and after a real id
        assert (obs >= 0).all(axis=1).any() and ((obs < 0).any(axis=1) & (obs >= 0).any(axis=1)).sum() > 4
        obs, _, _ = M.records(T[f"{kind}-free"])
        assert (obs < 0).all(axis=1).any() and (obs >= 0).any()
        assert M.records(T[f"{kind}-nobs1"])[0].shape[1] == 1 and M.records(T[f"{kind}-nobs64"])[0].shape[1] == 64
        _, masks, _ = M.records(T[f"{kind}-allmasked"])
        assert (masks.sum(axis=1) == 0).any() and (masks.sum(axis=1) > 0).any()               # a zero mask sum, beside ordinary records
        _, masks, _ = M.records(T[f"{kind}-onelegal"])
        assert (masks.sum(axis=1) == 1).all() and len(set(masks.argmax(axis=1).tolist())) > 1
        _, masks, _ = M.records(T[f"{kind}-maskbytes"])
        assert {2, 0x80, 255} <= set(masks.reshape(-1).tolist()) and 0 in masks
        # 1 / 3 is not an f32, and a logit of the row divided by three is not either: the quotient is rounded, pass by pass
        assert Fraction(float(np.float32(1) / np.float32(3))) != Fraction(1, 3)
        r = T[f"{kind}-tw3"]
        assert len(M.twists(r)[0]) == 3
        l = legal_logits(oracle, r)
        assert any(Fraction(float(np.float32(x) / np.float32(3))) * 3 != Fraction(float(x)) for x in l)
        assert len(M.twists(T[f"{kind}-tw1"])[0]) == 1 and len(M.twists(T[f"{kind}-tw2"])[0]) == 2 and not M.twists(T[f"{kind}-notwist"])[0]
        # the 1e-6 of the denominator is a good part of it
        r = T[f"{kind}-eps"]
        s = np.exp(legal_logits(oracle, r).astype(np.float64))
        assert s.max() < 2e-6
        # without the ReLU a negative activation goes on: the flag changes the numbers
        r = T[f"{kind}-norelu-emb"]
        assert not M.emb_relu(r)
        assert ref64.embedding_bag_f64(M.policy_arrays(r)[0], M.policy_arrays(r)[1], False, M.records(r)[0]).min() < -0.05
        r = T[f"{kind}-norelu-common"]
        emb, eb, common, _, _ = M.policy_arrays(r)
        assert not any(rl for (_, _, rl) in common)
        h = ref64.embedding_bag_f64(emb, eb, True, M.records(r)[0])
        assert ref64.linear_f64(common[0][0], common[0][1], False, h).min() < -0.05
        # exp past both ends of an f32, in legal entries, with the activations on the way far from overflow
        r = T[f"{kind}-exp"]
        l = legal_logits(oracle, r)
        assert l.max() > 88.73 and l.min() < -103.98 and ((l < -87.4) & (l > -103.9)).any()
        rows_l, rows_m = M.oracle_results(oracle, r)[(FORWARD, True)][0], M.records(r)[1] != 0
        assert any((rows_l[i][rows_m[i]] < 88.7).all() and (rows_l[i][rows_m[i]] < -87.4).any() for i in range(r.n))      # underflow without an inf in the sum
        p, v = M.oracle_results(oracle, r)[(PREDICT, True)]
        assert np.isnan(p).any() and ((p > 0) & (p < 2.0 ** -126)).any() and np.isfinite(v).all()
        assert max(ref64.max_activations(M.policy_arrays(r), *M.twists(r), M.records(r)[0], M.records(r)[2])) < 1e6
    for r in IN_RANGE:                                                                       # .. and every other row stays inside the range of the bounds
        assert np.abs(legal_logits(oracle, r)).max(initial=0.0) < 20.0, r.name
    assert M.policy_arrays(T["basic-emb288-a5"])[0].shape[1] == 288 > M.EVAL_THREADS and M.n_actions(T["basic-emb288-a5"]) != 4
    assert M.policy_arrays(T["basic-emb512-a31"])[0].shape[1] == 512 and M.n_actions(T["basic-emb512-a31"]) == 31
    assert widths(T["basic-h256-a3"])[0] == M.EVAL_THREADS
    for name in ("generic-obs300-tw2", "generic-obs300-tw3-ragged"):                         # a twisted id above 255: the one-byte table is wrong for it
        r = T[name]
        obs, _, perms = M.records(r)
        op = np.asarray(M.twists(r)[0])
        assert r.obs_size > 256
        img = [op[p, i] for rec, p in zip(obs, perms) if p >= 0 for i in rec if i >= 0]
        assert max(img) > 255 and any((x & 255) != x for x in img)
        full_img = [op[p, i] for rec in obs for p in range(len(op)) for i in rec if i >= 0]
        assert max(full_img) > 255
    assert widths(T["generic-w512"])[0] == M.EVAL_GEN_W
    assert M.policy_arrays(T["generic-emb512"])[0].shape[1] == M.EVAL_GEN_W
    assert M.EVAL_THREADS < widths(T["generic-w300"])[0] < M.EVAL_GEN_W
    assert all(w % 4 for w in widths(T["generic-w30"])[:-2]) and widths(T["generic-a30"])[-2] % 4 == 2
    assert M.policy_arrays(T["generic-value3"])[4][-1][1].size == 3
    assert len(M.policy_arrays(T["generic-nocommon"])[2]) == 0
    assert len(M.policy_arrays(T["generic-noaction"])[3]) == 0 and M.n_actions(T["generic-noaction"]) == 8
    assert len(M.policy_arrays(T["generic-novalue"])[4]) == 0 and M.policy_arrays(T["generic-novalue"])[2][-1][1].size % 4
    assert [len(s) for s in M.policy_arrays(T["generic-8common"])[2:]] == [8, 1, 1]
    assert [len(s) for s in M.policy_arrays(T["generic-8heads"])[2:]] == [1, 8, 8]
    for name in ("generic-8common", "generic-8heads"):                                       # the deep stacks still tell the records apart
        l, v = M.oracle_results(oracle, T[name])[(FORWARD, False)]
        assert v.std() > 0.05 and l[M.records(T[name])[1] != 0].std() > 0.05, name
    # the cross rows: the same numbers from a policy each kernel takes
    a, b = M.oracle_results(oracle, T["cross-basic"]), M.oracle_results(oracle, T["cross-generic"])
    for k in a:
        assert np.array_equal(f32_bits(a[k][0]), f32_bits(b[k][0])) and np.array_equal(f32_bits(a[k][1]), f32_bits(b[k][1]))
    assert M.policy_arrays(T["cross-generic"])[0].shape[0] == 257


# ------------------------------------------------------------------------------------------------ the oracle against float64
@pytest.mark.parametrize("row", IN_RANGE, ids=ids(IN_RANGE))
def test_the_oracle_lies_inside_the_float64_bounds(oracle, row):
    """ARITH_CHAIN with the deterministic exp (the kernels' arithmetic) against tests/ref64.py, all three modes, with and without
    perms; with libm's expf the probabilities stay within the 1e-6 / 1e-5 of test_policy_evaluate_matches_oracle."""
    got, libm, want = M.oracle_results(oracle, row), M.oracle_results(oracle, row, det_exp=False), M.f64_results(row)
    _, masks, _ = M.records(row)
    legal = masks != 0
    for key in M.cases():
        (o, v), (wo, wv, bo, bv) = got[key], want[key]
        assert np.isfinite(o).all() and np.isfinite(v).all()
        assert inside(o, wo, bo), (row.name, key, np.abs(o - wo).max(), bo.max())
        assert inside(v, wv, bv), (row.name, key, np.abs(v - wv).max(), bv.max())
        assert bo.max() < 1e-3 and bv.max() < 1e-3                           # a bound that means something: far below the numbers themselves
        if key[0] == FORWARD:
            assert np.all(f32_bits(o[~legal]) == f32_bits(np.float32(-1e10)))
        else:
            assert np.all(f32_bits(o[~legal]) == 0)
            dead = ~legal.any(axis=1)
            assert np.all(f32_bits(o[dead]) == 0)                            # 0 / (0 + 1e-6)
            np.testing.assert_allclose(o, libm[key][0], atol=1e-6, rtol=1e-5)
        assert np.array_equal(f32_bits(v), f32_bits(libm[key][1]))
    a, b = got[(FULL_PREDICT, True)], got[(FULL_PREDICT, False)]
    assert a is b or np.array_equal(f32_bits(a[0]), f32_bits(b[0]))


def test_the_exp_constant_of_the_probability_bound_is_the_measured_one(oracle):
    """ref64.EXP_REL: four times the largest relative error of two_expf_det and of libm's expf against float64, measured here again
    on 200,001 arguments of [-87, 88] and on every in-range logit of the table."""
    L = oracle.lib()
    libm = C.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = C.c_float, [C.c_float]
    x = np.concatenate([np.linspace(-87, 88, 200001).astype(np.float32)] + [legal_logits(oracle, r).reshape(-1) for r in IN_RANGE])
    want = np.exp(x.astype(np.float64))
    worst = 0.0
    for f in (L.two_expf_det, libm.expf):
        got = np.array([f(C.c_float(float(v))) for v in x], np.float32).astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / want).max()))
    assert 0.9 * 2.0 ** -24 < worst <= ref64.EXP_REL / 4, worst / 2.0 ** -24


# ------------------------------------------------------------------------------------------------ ref64 by hand and against torch
def _hand_policy():
    emb = np.array([[1, 0], [0, 2], [-1, -1]], np.float32)
    eb = np.array([0.5, -0.5], np.float32)
    common = [(np.array([[1, 2], [3, 4]], np.float32).reshape(-1), np.array([0, 1], np.float32), True)]
    action = [(np.array([[1, 0], [0, 1]], np.float32).reshape(-1), np.array([0, 0], np.float32), False)]
    value = [(np.array([[1], [1]], np.float32).reshape(-1), np.array([0.25], np.float32), False)]
    return (emb, eb, common, action, value), [[0, 1, 2], [1, 2, 0]], [[0, 1], [1, 0]]


def test_ref64_agrees_with_a_case_worked_by_hand():
    """ids [0, 1, free]: embedding (0.5, -0.5) + (1, 0) + (0, 2) = (1.5, 1.5); common (1.5 + 4.5, 3 + 6 + 1) = (6, 10); logits (6, 10),
    value 16.25.  Twist 1 maps the ids to [1, 2]: embedding (-0.5, 0.5) -> ReLU (0, 0.5); common (1.5, 3); logits gathered by [1, 0]:
    (3, 1.5); value 4.75.  full_predict: logits (4.5, 5.75), value 10.5."""
    arrs, op, ap = _hand_policy()
    obs = np.array([[0, 1, -1]] * 3)
    masks = np.array([[1, 1], [0, 1], [0, 0]], np.uint8)
    l, v = ref64.forward_f64(arrs, op, ap, obs, masks, [-1, 1, 0])
    assert np.array_equal(l, [[6, 10], [ref64.MASKED, 1.5], [ref64.MASKED, ref64.MASKED]]) and np.array_equal(v, [16.25, 4.75, 16.25])
    assert np.array_equal(ref64.forward_f64(arrs, op, ap, [[-1, 0, 1]], [[1, 1]], [-1])[0], [[6, 10]])       # a free slot anywhere adds nothing
    assert np.array_equal(ref64.forward_f64(arrs, op, ap, [[-1, -1, -1]], [[1, 1]], [1])[1], [0.5 + 2 + 0.25])   # no id: the bias alone, (0.5, 0) -> (0.5, 2)
    p, v = ref64.predict_f64(arrs, op, ap, obs, masks, [-1, 1, 0])
    e6, e10, e15 = np.exp(6.0), np.exp(10.0), np.exp(1.5)
    np.testing.assert_allclose(p, [[e6 / (e6 + e10 + 1e-6), e10 / (e6 + e10 + 1e-6)], [0, e15 / (e15 + 1e-6)], [0, 0]], rtol=1e-15, atol=0)
    assert p[1, 0] == 0 and np.array_equal(p[2], [0, 0]) and np.array_equal(v, [16.25, 4.75, 16.25])
    p, v = ref64.full_predict_f64(arrs, op, ap, obs, masks)
    a, b = np.exp(4.5), np.exp(5.75)
    np.testing.assert_allclose(p, [[a / (a + b + 1e-6), b / (a + b + 1e-6)], [0, b / (b + 1e-6)], [0, 0]], rtol=1e-15, atol=0)
    assert np.array_equal(v, [10.5, 10.5, 10.5])
    p0, v0 = ref64.full_predict_f64(arrs, (), (), obs, masks)                                   # no twists: one plain pass (policy.rs:103)
    p1, v1 = ref64.predict_f64(arrs, (), (), obs, masks, [-1, -1, -1])
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1) and np.array_equal(v0, [16.25] * 3)
    l, v, el, ev = ref64.forward_f64_bound(arrs, op, ap, obs, masks, [-1, 1, 0], "f32")         # the bound's forward is the same forward
    assert np.array_equal(l[0], [6, 10]) and v[1] == 4.75 and el[1, 0] == 0 and 0 < el[0, 0] < 1e-4 and 0 < ev[0] < 1e-4


def test_ref64_softmax_agrees_with_torch():
    """Where no action is masked the reference's soft-max is torch's times S / (S + 1e-6), S = sum exp(l)."""
    import torch
    rng = np.random.default_rng(5)
    l = rng.normal(0, 3, size=(50, 7))
    got = ref64.masked_softmax_f64(l, np.ones_like(l, bool))
    S = np.exp(l).sum(axis=1, keepdims=True)
    want = torch.softmax(torch.from_numpy(l), dim=1).numpy() * (S / (S + 1e-6))
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    for r in (M.BY_NAME["basic-a5"], M.BY_NAME["generic-a31"]):
        arrs, (op, ap) = M.policy_arrays(r), M.twists(r)
        obs, _, perms = M.records(r)
        ones = np.ones((r.n, M.n_actions(r)), bool)
        lg, _ = ref64.forward_f64(arrs, op, ap, obs, ones, perms)
        p, _ = ref64.predict_f64(arrs, op, ap, obs, ones, perms)
        S = np.exp(lg).sum(axis=1, keepdims=True)
        np.testing.assert_allclose(p, torch.softmax(torch.from_numpy(lg), dim=1).numpy() * (S / (S + 1e-6)), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ mutations
def _per_pass(oracle, row):
    """the oracle's f32 logits [T][n][A] (gathered by the pass's act_perms) and values [T][n] of every twist of a row"""
    pol = M.oracle_policy(oracle, row)
    obs, _, _ = M.records(row)
    T = len(M.twists(row)[0])
    out = [[pol.raw_predict([int(x) for x in rec if x >= 0], perm=p, arith=oracle.ARITH_CHAIN) for rec in obs] for p in range(T)]
    return (np.array([[l for l, _ in o] for o in out], np.float32), np.array([[v for _, v in o] for o in out], np.float32))


def _average_f32(xs, order):
    acc = np.zeros_like(xs[0])
    n = np.float32(len(xs))
    for p in order:
        acc = (acc + xs[p] / n).astype(np.float32)
    return acc


@pytest.mark.parametrize("name", ["basic-tw3", "generic-tw3", "basic-a31", "generic-a31"])
def test_a_wrong_pass_order_of_the_twist_average_is_seen(oracle, name):
    """Two mutations of FULL_PREDICT, built from the oracle's own per-pass numbers.  (1) The passes summed last to first: the same
    real number, other roundings -- no float64 bound can see a rounding order (this mutant stays inside, asserted), the bit
    comparison with the oracle does.  (2) Pass p's logits gathered by the action permutation of pass p + 1: outside the bound."""
    row = M.BY_NAME[name]
    l, v = _per_pass(oracle, row)
    T = l.shape[0]
    _, masks, _ = M.records(row)
    (wo, wv, bo, bv), (o, ov) = M.f64_results(row)[(FULL_PREDICT, True)], M.oracle_results(oracle, row)[(FULL_PREDICT, True)]
    wl, _, bl, _ = ref64.full_predict_f64_bound(M.policy_arrays(row), *M.twists(row), M.records(row)[0], "f32", emb_relu=M.emb_relu(row))
    # the oracle's own order, rebuilt here, is the oracle's average
    assert np.array_equal(f32_bits(_average_f32(v, range(T))), f32_bits(ov))
    assert inside(_average_f32(l, range(T)), wl, bl)
    back_l, back_v = _average_f32(l, range(T - 1, -1, -1)), _average_f32(v, range(T - 1, -1, -1))
    assert inside(back_l, wl, bl) and inside(back_v, wv, bv)
    assert not (np.array_equal(f32_bits(back_l), f32_bits(_average_f32(l, range(T)))) and np.array_equal(f32_bits(back_v), f32_bits(ov)))
    ap = np.asarray(M.twists(row)[1])
    raw = np.empty_like(l)
    for p in range(T):
        raw[p][:, ap[p]] = l[p]                                               # l[p][i] = raw[p][ap[p][i]]
    wrong = _average_f32(np.stack([raw[p][:, ap[(p + 1) % T]] for p in range(T)]), range(T))
    assert not inside(wrong, wl, bl)
    with np.errstate(over="ignore"):
        e = np.where(masks != 0, np.exp(wrong.astype(np.float64)), 0.0)
    assert not inside(e / (e.sum(axis=1, keepdims=True) + 1e-6), wo, bo)


@pytest.mark.parametrize("name", ["basic-eps", "generic-eps"])
def test_a_softmax_without_the_1e_6_is_seen(oracle, name):
    row = M.BY_NAME[name]
    _, masks, perms = M.records(row)
    for key in ((PREDICT, True), (FULL_PREDICT, True)):
        wo, _, bo, _ = M.f64_results(row)[key]
        l = M.oracle_results(oracle, row)[(FORWARD, True if key[0] == PREDICT else False)][0]
        if key[0] == FULL_PREDICT and len(M.twists(row)[0]):
            continue
        e = np.where(masks != 0, np.array([[oracle.expf_det(float(x)) if x > -1e9 else 0.0 for x in rec] for rec in l], np.float32), np.float32(0))
        s = np.zeros(len(e), np.float32)
        for i in range(e.shape[1]):
            s = (s + e[:, i]).astype(np.float32)
        with_eps = (e / (s + np.float32(0.000001))[:, None]).astype(np.float32)
        assert np.array_equal(f32_bits(with_eps), f32_bits(M.oracle_results(oracle, row)[key][0]))     # the restatement is the oracle's soft-max
        assert inside(with_eps, wo, bo)
        assert not inside((e / s[:, None]).astype(np.float32), wo, bo)


@pytest.mark.parametrize("name", ["basic-ragged", "generic-ragged", "basic-free", "generic-free", "generic-obs300-tw3-ragged"])
def test_a_free_slot_counted_as_id_0_is_seen(oracle, name):
    row = M.BY_NAME[name]
    obs, masks, perms = M.records(row)
    pol = M.oracle_policy(oracle, row)
    as_zero = np.where(obs < 0, 0, obs)
    oracle.set_det_exp(True)
    try:
        for mode in (FORWARD, PREDICT, FULL_PREDICT):
            wo, wv, bo, bv = M.f64_results(row)[(mode, True)]
            o, v = pol.evaluate_batch(mode, as_zero, masks, perms, arith=oracle.ARITH_CHAIN)
            good = pol.evaluate_batch(mode, obs, masks, perms, arith=oracle.ARITH_CHAIN)
            assert inside(good[0], wo, bo) and inside(good[1], wv, bv)
            assert not inside(v, wv, bv), (name, mode)
            assert not inside(o, wo, bo), (name, mode)
    finally:
        oracle.set_det_exp(False)
