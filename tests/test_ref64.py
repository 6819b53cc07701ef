"""CPU: the oracle's batched forward and the float64 reference (tests/ref64.py) the GPU tolerance tests stand on.

* Policy.forward_batch gives the bits of one Policy.forward per record in every arithmetic mode, with and without twists,
  with partial masks, on one thread and on several.
* The float64 forward stays within 1e-5 of the oracle's reference order and of its fma chain, and the float64 GAE within
  1e-5 of the oracle's f32 GAE at the benchmark's horizon and beyond.
* Both float64 pieces reproduce the reference's own known answers (tests/golden/reference_known_answers.json).
* The trainer hand-off's references (one-hot, log-prob, normalised advantages) agree with torch in float64 and with cases worked by hand,
  and torch's own f32 Categorical stays inside the bound the GPU log-probs are held to.
"""
import json
import os

import numpy as np
import pytest

from tests.ref64 import MASKED, embedding_bag_f64, forward_f64, gae_f64, gae_f64_episodes, linear_f64
from tests.util import make_deep_policy_arrays, make_policy_arrays, puzzle_transpose_twist, trained_puzzle8_arrays

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_known_answers.json")


def _records(n2, n, seed, all_legal=False):
    """n records of random boards of an n2-cell puzzle: obs ids 16c + tile, random masks with at least one legal move,
    twists drawn from {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    boards = np.argsort(rng.random((n, n2)), axis=1)
    obs = np.arange(n2)[None, :] * n2 + boards
    masks = np.ones((n, 4), bool) if all_legal else rng.random((n, 4)) < 0.6
    masks[np.arange(n), rng.integers(0, 4, n)] = True
    perms = rng.integers(-1, 2, n).astype(np.int32)
    return obs, masks, perms


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("arith", [0, 1, 2])
def test_forward_batch_equals_per_record_forward(oracle, arith):
    arrs = make_policy_arrays(16, seed=4, emb=64, hidden=32)
    op, ap = puzzle_transpose_twist(4)
    pol = oracle.Policy(*arrs, op, ap)
    obs, masks, perms = _records(16, 400, seed=arith)
    assert set(perms.tolist()) == {-1, 0, 1} and not masks.all()
    want_l = np.empty((400, 4), np.float32)
    want_v = np.empty(400, np.float32)
    for r in range(400):
        lg, v = pol.forward(obs[r].tolist(), masks[r].tolist(), perm=int(perms[r]), arith=arith)
        want_l[r], want_v[r] = lg, v
    for threads in (1, 3):
        lg, v = pol.forward_batch(obs, masks, perms, arith=arith, num_threads=threads)
        assert np.array_equal(_bits(lg), _bits(want_l)), threads
        assert np.array_equal(_bits(v), _bits(want_v)), threads
    assert np.all((want_l == np.float32(MASKED)) == ~masks)


def test_forward_batch_rejects_out_of_range_records(oracle):
    arrs = make_policy_arrays(9, seed=0, emb=32, hidden=32)
    pol = oracle.Policy(*arrs)
    obs, masks, _ = _records(9, 4, seed=0)
    with pytest.raises(ValueError):
        pol.forward_batch(obs + 81, masks, np.full(4, -1))
    with pytest.raises(ValueError):
        pol.forward_batch(obs, masks, np.zeros(4))              # no twists in this policy


def _policies():
    op16, ap16 = puzzle_transpose_twist(4)
    op9, ap9 = puzzle_transpose_twist(3)
    return {
        "synthetic_scale1": (16, make_policy_arrays(16, seed=0), op16, ap16),
        "synthetic_scale3": (16, make_policy_arrays(16, seed=1, scale=3.0), op16, ap16),
        "trained_puzzle8": (9, trained_puzzle8_arrays(), op9, ap9),
        "deep": (16, make_deep_policy_arrays(16, seed=2, emb=96, common=(128, 64), policy_layers=(32,), value_layers=(48, 16)),
                 op16, ap16),
    }


@pytest.mark.parametrize("name", ["synthetic_scale1", "synthetic_scale3", "trained_puzzle8", "deep"])
def test_forward_f64_within_1e5_of_the_oracle(oracle, name):
    n2, arrs, op, ap = _policies()[name]
    pol = oracle.Policy(*arrs, op, ap)
    obs, masks, perms = _records(n2, 3000, seed=7)
    l64, v64 = forward_f64(arrs, op, ap, obs, masks, perms, chunk=1000)
    assert np.all((l64 == MASKED) == ~masks)
    assert np.all(np.float32(l64[~masks]) == np.float32(MASKED))
    for arith in (oracle.ARITH_REF, oracle.ARITH_CHAIN):
        lg, v = pol.forward_batch(obs, masks, perms, arith=arith, num_threads=4)
        assert np.array_equal(lg == np.float32(MASKED), ~masks)
        dl = float(np.max(np.abs(lg[masks] - l64[masks])))
        dv = float(np.max(np.abs(v - v64)))
        assert dl < 1e-5 and dv < 1e-5, (name, arith, dl, dv)
    # the check is not vacuous: the reference's own scale keeps the logits and values away from zero
    assert float(np.max(np.abs(l64[masks]))) > 1e-2 and float(np.max(np.abs(v64))) > 1e-2


def test_forward_f64_twists_follow_the_reference(oracle):
    """perm p: obs ids through obs_perms[p], logits gathered by act_perms[p] -- a transposed board under the transpose twist
    sees the un-twisted forward of the original board, its logits permuted left<->up, right<->down."""
    arrs = make_policy_arrays(9, seed=5, emb=64, hidden=32)
    op, ap = puzzle_transpose_twist(3)
    obs, masks, _ = _records(9, 200, seed=3, all_legal=True)
    T = np.array([(i % 3) * 3 + (i // 3) for i in range(9)])
    board = obs - np.arange(9) * 9
    tboard = np.empty_like(board)
    tboard[:, T] = T[board]
    tobs = np.arange(9) * 9 + tboard
    l0, v0 = forward_f64(arrs, [], [], obs, masks, np.full(200, -1))
    l1, v1 = forward_f64(arrs, op, ap, tobs, masks, np.ones(200, np.int64))
    np.testing.assert_allclose(v1, v0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(l1, l0[:, [1, 0, 3, 2]], rtol=0, atol=1e-12)


def _episode(n, seed):
    rng = np.random.default_rng(seed)
    rews = np.full(n, np.float32(-0.5 / 256), np.float32)
    rews[-1] = np.float32(1.0) if seed % 2 else np.float32(-0.5)
    vals = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return rews, vals


@pytest.mark.parametrize("n", [1, 2, 257, 1022])
def test_gae_f64_within_1e5_of_the_oracle(oracle, n):
    for seed in range(4):
        rews, vals = _episode(n, seed)
        a32, r32 = oracle.gae(rews, vals, 0.995, 0.995)
        a64, r64 = gae_f64(rews, vals, 0.995, 0.995)
        assert float(np.max(np.abs(a32 - a64))) < 1e-5 and float(np.max(np.abs(r32 - r64))) < 1e-5, (n, seed)


def test_gae_f64_episodes_equals_one_episode_at_a_time():
    lens = [257, 1, 13, 257, 2, 100]
    parts = [_episode(n, s) for s, n in enumerate(lens)]
    rews = np.concatenate([p[0] for p in parts])
    vals = np.concatenate([p[1] for p in parts])
    a, r = gae_f64_episodes(rews, vals, lens, 0.995, 0.99)
    s = 0
    for n, (rw, vl) in zip(lens, parts):
        a1, r1 = gae_f64(rw, vl, 0.995, 0.99)
        assert np.array_equal(a[s:s + n], a1) and np.array_equal(r[s:s + n], r1)
        s += n


def test_known_answers_of_the_reference(oracle):
    ka = json.load(open(GOLDEN))
    for key in ("linear_forward", "linear_forward_relu"):
        c = ka[key]
        out = linear_f64(c["weights"], c["bias"], c["relu"], np.asarray([c["input"]]))
        assert np.array_equal(out[0], np.asarray(c["out"], np.float64)), key
        # the same Linear as a one-layer policy head of the oracle (an identity EmbeddingBag feeding it)
        n_in = len(c["input"])
        pol = oracle.Policy(np.eye(n_in, dtype=np.float32), np.zeros(n_in, np.float32), [],
                            [(np.asarray(c["weights"], np.float32), np.asarray(c["bias"], np.float32), c["relu"])],
                            [(np.zeros(n_in, np.float32), np.zeros(1, np.float32), False)], emb_relu=False)
        for arith in (oracle.ARITH_REF, oracle.ARITH_CHAIN):
            ids = [i for i, x in enumerate(c["input"]) for _ in range(int(x))]
            lg, _ = pol.raw_predict(ids, arith=arith)
            assert lg == c["out"], (key, arith)
    c = ka["embedding_bag"]
    out = embedding_bag_f64(c["vectors"], c["bias"], c["relu"], np.asarray([c["input"]]))
    assert np.array_equal(out[0], np.asarray(c["out"], np.float64))
    arrs = (np.asarray(c["vectors"], np.float32), np.asarray(c["bias"], np.float32), [],
            [(np.eye(2, dtype=np.float32).reshape(-1), np.zeros(2, np.float32), False)],
            [(np.zeros(2, np.float32), np.zeros(1, np.float32), False)])
    l64, _ = forward_f64(arrs, [], [], np.asarray([c["input"]]), np.ones((1, 2), bool), [-1], emb_relu=c["relu"])
    lg, _ = oracle.Policy(*arrs, emb_relu=c["relu"]).forward_batch(np.asarray([c["input"]]), np.ones((1, 2), bool), [-1])
    assert l64[0].tolist() == c["out"] == lg[0].tolist()
    c = ka["dummy_env_ppo"]
    a64, r64 = gae_f64(c["rewards"], c["values"], c["gamma"], c["lambda"])
    np.testing.assert_allclose(r64, c["derived_rets"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a64, c["derived_advs"], rtol=0, atol=1e-12)
    a32, r32 = oracle.gae(c["rewards"], c["values"], c["gamma"], c["lambda"])
    np.testing.assert_allclose(r32, r64, rtol=0, atol=1e-6)
    np.testing.assert_allclose(a32, a64, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------- a-priori error bounds
def _scaled(arrs, k):
    f = np.float32(2.0 ** k)
    emb, eb, common, action, value = arrs
    sc = lambda ls: [(np.asarray(w, np.float32) * f, np.asarray(b, np.float32) * f, r) for (w, b, r) in ls]
    return (np.asarray(emb, np.float32) * f, np.asarray(eb, np.float32) * f, sc(common), sc(action), sc(value))


BOUND_FIXTURES = ["synthetic_scale1", "trained_puzzle8", "deep"]


@pytest.mark.parametrize("name", BOUND_FIXTURES)
def test_oracle_forwards_stay_inside_their_a_priori_bounds(oracle, name):
    """ARITH_REF and ARITH_CHAIN inside the f32 bound, ARITH_F16 inside the fp16 bound (where no activation reaches 65504),
    with every weight scaled by 2^k, k = -12 .. 6."""
    from tests.ref64 import forward_f64_bound, max_activations
    n2, arrs0, op, ap = _policies()[name]
    obs, masks, perms = _records(n2, 300, seed=11)
    checked_f16 = 0
    for k in range(-12, 7):
        arrs = _scaled(arrs0, k)
        pol = oracle.Policy(*arrs, op, ap)
        for arith, mode in ((oracle.ARITH_REF, "f32"), (oracle.ARITH_CHAIN, "f32"), (oracle.ARITH_F16, "fp16")):
            if mode == "fp16" and max(max_activations(arrs, op, ap, obs, perms)) >= 65504 / 2:
                continue                                           # outside fp16's range: it overflows there as its spec says
            l64, v64, el, ev = forward_f64_bound(arrs, op, ap, obs, masks, perms, mode)
            lg, v = pol.forward_batch(obs, masks, perms, arith=arith, num_threads=4)
            dl = np.abs(lg.astype(np.float64) - l64)[masks]
            dv = np.abs(v.astype(np.float64) - v64)
            assert np.all(dl <= el[masks]) and np.all(dv <= ev), (name, k, arith, float(np.max(dl - el[masks])), float(np.max(dv - ev)))
            checked_f16 += mode == "fp16"
            # the bound is a bound, not a blanket: within three orders of magnitude of the largest deviation seen at scale 1
            if k == 0 and mode == "f32":
                assert float(np.max(el[masks])) < 1e-3 * max(1.0, float(np.max(np.abs(l64[masks]))))
    assert checked_f16 >= 10, checked_f16


def _split(x):
    """x16 split of f32 values into binary16 hi / lo terms (tw_engine16x2.hpp), back in f64 and unscaled."""
    sx = np.asarray(x, np.float32) * np.float32(16)
    hi = sx.astype(np.float16)
    lo = (sx - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64) / 16, lo.astype(np.float64) / 16


def _split_forward(arrs, obs, drop_wlo_hhi):
    """numpy emulation of EngineS on one-common-layer policies, no twists: logits and values in f64 from the split terms."""
    emb, eb, common, action, value = arrs
    (w1, b1, _), = common
    (wa, ba, _), = action
    (wv, bv, _), = value
    H = np.asarray(b1).size
    Th, Tl = _split(emb)
    h0 = np.maximum(Th[obs].sum(axis=1) + Tl[obs].sum(axis=1) + np.asarray(eb, np.float64), 0)
    h0 = h0.astype(np.float32)

    def lin(x, w, b):
        Wh, Wl = _split(np.asarray(w).reshape(-1, np.asarray(b).size))
        xh, xl = _split(x)
        y = xh @ Wh + xl @ Wh + (0 if drop_wlo_hhi else xh @ Wl)
        return y + np.asarray(b, np.float64)
    h1 = np.maximum(lin(h0, w1, b1), 0).astype(np.float32)
    Wh = np.concatenate([np.asarray(wa).reshape(H, -1), np.asarray(wv).reshape(H, 1)], axis=1)
    out = lin(h1, Wh.reshape(-1), np.concatenate([np.asarray(ba), np.asarray(bv)]))
    return out[:, :-1], out[:, -1]


def _coherent_policy():
    """make_policy_arrays(16, seed=0, emb=64, hidden=32) with every common and head weight set to (1/3) / sqrt(fan_in): all
    products of a layer are positive (ReLU outputs times positive weights) and every W_lo has the same sign, so an error in
    the split terms adds up instead of averaging out."""
    emb, eb, common, action, value = make_policy_arrays(16, seed=0, emb=64, hidden=32)
    third = lambda ls, fan: [(np.full_like(w, np.float32(1 / 3) / np.float32(np.sqrt(fan))), b, r) for (w, b, r) in ls]
    return emb, eb, third(common, 64), third(action, 32), third(value, 32)


def test_split_emulation_inside_the_fp16x2_bound_and_the_bound_can_fail():
    """The fp16x2 bound holds for a numpy emulation of the split on a random policy and on the coherent one, and the
    emulation with the W_lo * h_hi product dropped exceeds it on the coherent one (500 Puzzle-15 boards, no twists)."""
    from tests.ref64 import forward_f64_bound
    obs, masks, _ = _records(16, 500, seed=5, all_legal=True)
    perms = np.full(500, -1)
    arrs = make_policy_arrays(16, seed=0, emb=128, hidden=64)
    l64, v64, el, ev = forward_f64_bound(arrs, [], [], obs, masks, perms, "fp16x2")
    lg, v = _split_forward(arrs, obs, drop_wlo_hhi=False)
    assert np.all(np.abs(lg - l64) <= el) and np.all(np.abs(v - v64) <= ev)
    arrs = _coherent_policy()
    perms = np.full(500, -1)
    l64, v64, el, ev = forward_f64_bound(arrs, [], [], obs, masks, perms, "fp16x2")
    lg, v = _split_forward(arrs, obs, drop_wlo_hhi=False)
    assert np.all(np.abs(lg - l64) <= el) and np.all(np.abs(v - v64) <= ev)
    lg, v = _split_forward(arrs, obs, drop_wlo_hhi=True)
    assert np.any(np.abs(lg - l64) > el) and np.any(np.abs(v - v64) > ev)


def test_gae_bound_holds_for_perturbed_values(oracle):
    """The GAE bound carries a value error through the recurrence: the oracle's f32 GAE of values moved by up to `err` stays
    inside it, at the benchmark's horizon."""
    from tests.ref64 import gae_bound_episodes, gae_f64_episodes
    rng = np.random.default_rng(3)
    lens = [257, 1, 2, 100]
    rews = np.concatenate([_episode(n, s)[0] for s, n in enumerate(lens)])
    vals = np.concatenate([_episode(n, s)[1] for s, n in enumerate(lens)]).astype(np.float64)
    err = np.full(vals.size, 3e-6)
    moved = (vals + rng.uniform(-1, 1, vals.size) * err).astype(np.float32)
    a64, r64 = gae_f64_episodes(rews, vals, lens, 0.995, 0.995)
    ea, er = gae_bound_episodes(rews, vals, err + 2.0 ** -24, lens, 0.995, 0.995)       # (+ the rounding of the moved values)
    s = 0
    for n in lens:
        a32, r32 = oracle.gae(rews[s:s + n], moved[s:s + n], 0.995, 0.995)
        assert np.all(np.abs(a32 - a64[s:s + n]) <= ea[s:s + n]) and np.all(np.abs(r32 - r64[s:s + n]) <= er[s:s + n])
        s += n


# ---------------------------------------------------------------------------------------------- trainer hand-off references
def test_onehot_ref_is_a_set_per_row():
    from tests.ref64 import onehot_ref
    got = onehot_ref([[4, 0, 4], [2, 1, 0], [3, 3, 3]], 5)
    assert got.dtype == np.float32 and got.tolist() == [[1, 0, 0, 0, 1], [1, 1, 1, 0, 0], [0, 0, 0, 1, 0]]
    assert np.array_equal(onehot_ref([[1, 0]], 2), onehot_ref([[0, 1]], 2))             # order does not matter
    assert onehot_ref(np.zeros((0, 3), np.uint8), 7).shape == (0, 7)
    rng = np.random.default_rng(0)
    obs = rng.integers(0, 50, (300, 3))
    want = np.zeros((300, 50), np.float32)
    for i, o in enumerate(obs):
        want[i, o] = 1.0                                                                # ppo.py:37-39, literally
    assert np.array_equal(onehot_ref(obs.astype(np.uint8), 50), want)
    for bad in ([[5]], [[-1]]):
        with pytest.raises(ValueError):
            onehot_ref(bad, 5)


def _random_logits(A, n, seed, scale):
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((n, A)) * scale).astype(np.float32)
    masks = rng.random((n, A)) < 0.6
    masks[np.arange(n), rng.integers(0, A, n)] = True
    l[~masks] = np.float32(MASKED)
    acts = np.array([rng.choice(np.flatnonzero(m)) for m in masks])
    return l, acts


@pytest.mark.parametrize("A", [3, 4, 5, 17, 31])
def test_log_prob_f64_against_torch_and_by_hand(A):
    import torch
    from tests.ref64 import log_prob_bound, log_prob_f64, logsumexp_f64
    for scale in (1.0, 30.0):
        l, acts = _random_logits(A, 4000, A, scale)
        want = torch.distributions.Categorical(logits=torch.tensor(l, dtype=torch.float64)).log_prob(torch.tensor(acts)).numpy()
        got = log_prob_f64(l, acts)
        assert np.max(np.abs(got - want) / (1.0 + np.abs(want))) < 1e-13
        # torch's own f32 arithmetic: inside the bound the hand-off kernel is held to while the logits are of the size of the log-probs;
        # with large logits only inside the bound of ITS form, logits - logsumexp(logits), which rounds at the size of the logits
        t32 = torch.distributions.Categorical(logits=torch.tensor(l)).log_prob(torch.tensor(acts)).numpy().astype(np.float64)
        dev = np.abs(t32 - got)
        assert np.all(dev <= log_prob_bound(A, got, lse=logsumexp_f64(l))), (A, scale, float(np.max(dev / log_prob_bound(A, got, lse=logsumexp_f64(l)))))
        assert np.all(dev <= log_prob_bound(A, got)) == (scale == 1.0), (A, scale, float(np.max(dev / log_prob_bound(A, got))))
    # one legal action: its probability is one; equal logits: 1 / A each; two logits ln 3 apart: 1/4 and 3/4
    one = np.full((1, A), MASKED)
    one[0, A - 2] = -3.25
    assert log_prob_f64(one, [A - 2])[0] == 0.0
    np.testing.assert_allclose(log_prob_f64(np.full((2, A), 7.5), [0, A - 1]), [-np.log(A)] * 2, rtol=0, atol=1e-14)
    two = np.full((2, A), MASKED)
    two[:, 0], two[:, 2] = 1.0, 1.0 + np.log(3.0)
    np.testing.assert_allclose(log_prob_f64(two, [0, 2]), [np.log(0.25), np.log(0.75)], rtol=0, atol=1e-15)
    assert np.isclose(log_prob_f64(two, [1])[0], MASKED - 1.0 - np.log(4.0), rtol=1e-15)     # a masked action: an ordinary number


def test_normalized_adv_f64_against_torch_and_by_hand():
    import torch
    from tests.ref64 import normalized_adv_bound, normalized_adv_f64
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(5000) * 0.3 - 0.2).astype(np.float32)
    t = torch.tensor(a, dtype=torch.float64)
    want = ((t - t.mean()) / (t.std() + 1e-8)).numpy()
    got = normalized_adv_f64(a)
    assert np.max(np.abs(got - want)) < 1e-12
    assert np.array_equal(normalized_adv_f64([1.0, 2.0, 3.0]), np.array([-1.0, 0.0, 1.0]) / (1.0 + 1e-8))
    assert np.all(normalized_adv_f64([2.0, 2.0, 2.0]) == 0.0)                            # std 0: the 1e-8 keeps it finite
    assert np.isnan(normalized_adv_f64([0.7])).all()                                     # one record: torch.std is nan
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                              # (torch says so too: degrees of freedom <= 0)
        assert np.isnan(((torch.tensor([0.7]) - 0.7) / (torch.tensor([0.7]).std() + 1e-8)).numpy()).all()
    # torch's f32 normalisation inside the bound the hand-off kernel is held to
    t32 = torch.tensor(a)
    n32 = ((t32 - t32.mean()) / (t32.std() + 1e-8)).numpy().astype(np.float64)
    assert np.all(np.abs(n32 - got) <= normalized_adv_bound(a, got) + 2.0 ** -22 * np.abs(got).max())   # (+ torch's own f32 mean and std)
