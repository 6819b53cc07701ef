"""A float64 reference of the PPO policy forward, GAE and the trainer hand-off, in plain numpy.

Written from the reference's definitions, not from the oracle's C code, so that a test can hold both the GPU and the oracle's own
f32 orders against an arithmetic neither of them uses:

* EmbeddingBag (layers.rs:56-86): bias + the sum of the rows of the obs ids in cell order, then ReLU when its flag is set.
* Linear (layers.rs:31-37): out = W x + b (+ ReLU), W in the export layout w[k * out + o] (src/twisterl/nn/utils.py:17-42).
* Policy::_raw_predict (policy.rs:79-100): embedding, common layers, value layers summed, action layers; a twist maps the obs ids
  through obs_perms[perm] (policy.rs:81-83) and gathers the logits by act_perms[perm] (policy.rs:95-97).
* Policy::forward_with_perm (policy.rs:56-65): masked logits are exactly -1e10.
* Policy::predict_with_perm (policy.rs:39-49): exp(l) for a legal action, 0 for a masked one, divided by their sum + 1e-6.
* Policy::full_predict (policy.rs:102-126): logits / n and value / n summed over all n twists in twist order, then that soft-max;
  without twists it is predict.
* GAE (ppo.rs:82-92): ret[t] = r[t] + gamma (v[t+1] + lambda adv[t+1]), adv[t] = ret[t] - v[t]; at the last record adv = r - v,
  ret = r.
"""
import numpy as np

MASKED = -1e10


def linear_f64(w, b, relu, x):
    """One Linear on a batch x [n, in] -> [n, out] in float64."""
    b = np.asarray(b, np.float64).reshape(-1)
    W = np.asarray(w, np.float64).reshape(-1, b.size)                  # [in][out]
    y = np.asarray(x, np.float64) @ W + b
    return np.maximum(y, 0.0) if relu else y


def embedding_bag_f64(vectors, bias, relu, ids):
    """EmbeddingBag on a batch of obs ids [n, cells] -> [n, vec_len] in float64: bias plus the rows in cell order.  An id of -1
    is a free slot of a shorter observation: the reference is handed the shorter list, so the slot adds nothing."""
    V = np.asarray(vectors, np.float64)
    ids = np.asarray(ids, np.int64)
    h = np.broadcast_to(np.asarray(bias, np.float64), (ids.shape[0], V.shape[1])).copy()
    for c in range(ids.shape[1]):
        h += np.where(ids[:, c, None] >= 0, V[ids[:, c]], 0.0)         # a free slot (-1) adds nothing
    return np.maximum(h, 0.0) if relu else h


def twist_ids(OP, perms, ids):
    """obs_perms[perm][id] per record (policy.rs:81-83); a free slot (-1) stays free."""
    return np.where(ids >= 0, np.take_along_axis(OP[perms], np.maximum(ids, 0), axis=1), -1)


def _n_actions(emb, common, action):
    """Width of the action stack's output: an empty Sequential hands its input on (modules.rs:28-34)."""
    for stack in (action, common):
        if len(stack):
            return int(np.asarray(stack[-1][1]).size)
    return int(np.asarray(emb).shape[1])


def forward_f64(arrs, obs_perms, act_perms, obs, masks, perms, emb_relu=True, chunk=8192):
    """Masked logits [n, A] and values [n] (float64) of the policy `arrs` (make_policy_arrays / make_deep_policy_arrays /
    trained_puzzle8_arrays layout) on records obs [n, cells], masks [n, A], perms [n] (-1 = no twist).  Works in chunks of
    `chunk` records: at 8,192 records and a 512-wide embedding a temporary is 32 MB."""
    emb, eb, common, action, value = arrs
    V = np.asarray(emb, np.float64)
    obs = np.asarray(obs, np.int64)
    n = obs.shape[0]
    obs = obs.reshape(n, -1)
    masks = np.asarray(masks, bool).reshape(n, -1)
    perms = np.asarray(perms, np.int64).reshape(n)
    OP = np.asarray(obs_perms, np.int64) if len(obs_perms) else None
    AP = np.asarray(act_perms, np.int64) if len(act_perms) else None
    if (perms >= 0).any() and (OP is None or AP is None or perms.max() >= len(OP)):
        raise ValueError("a record names a twist the policy does not have")
    common = [(np.asarray(w, np.float64).reshape(-1, np.asarray(b).size), np.asarray(b, np.float64), r) for (w, b, r) in common]
    action = [(np.asarray(w, np.float64).reshape(-1, np.asarray(b).size), np.asarray(b, np.float64), r) for (w, b, r) in action]
    value = [(np.asarray(w, np.float64).reshape(-1, np.asarray(b).size), np.asarray(b, np.float64), r) for (w, b, r) in value]

    def seq(layers, x):
        for W, b, r in layers:
            x = x @ W + b
            if r:
                x = np.maximum(x, 0.0)
        return x

    A = _n_actions(emb, common, action)
    logits = np.empty((n, A), np.float64)
    values = np.empty(n, np.float64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ids, p = obs[s:e], perms[s:e]
        tw = p >= 0
        if tw.any():
            ids = ids.copy()
            ids[tw] = twist_ids(OP, p[tw], ids[tw])
        h = embedding_bag_f64(V, eb, emb_relu, ids)
        h = seq(common, h)
        values[s:e] = seq(value, h).sum(axis=1)
        la = seq(action, h)
        if tw.any():
            la[tw] = np.take_along_axis(la[tw], AP[p[tw]], axis=1)
        logits[s:e] = np.where(masks[s:e], la, MASKED)
    return logits, values


def gae_f64(rews, vals, gamma, lam):
    """GAE of one episode in float64 -> (advs, rets)."""
    r = np.asarray(rews, np.float64)
    v = np.asarray(vals, np.float64)
    n = r.size
    advs, rets = np.empty(n), np.empty(n)
    advs[n - 1] = r[n - 1] - v[n - 1]
    rets[n - 1] = r[n - 1]
    for t in range(n - 2, -1, -1):
        rets[t] = r[t] + gamma * (v[t + 1] + lam * advs[t + 1])
        advs[t] = rets[t] - v[t]
    return advs, rets


def gae_f64_episodes(rews, vals, ep_len, gamma, lam):
    """gae_f64 over consecutive episodes of lengths ep_len (records in episode order), vectorised across the episodes."""
    L = np.asarray(ep_len, np.int64)
    starts = np.concatenate([[0], np.cumsum(L)[:-1]])
    r = np.asarray(rews, np.float64)
    v = np.asarray(vals, np.float64)
    advs, rets = np.empty(r.size), np.empty(r.size)
    nxt_v = np.zeros(L.size)
    nxt_a = np.zeros(L.size)
    for k in range(int(L.max()) if L.size else 0):         # k-th record from the end of every episode at least k+1 long
        live = L > k
        idx = starts[live] + L[live] - 1 - k
        if k == 0:
            rets[idx] = r[idx]
        else:
            rets[idx] = r[idx] + gamma * (nxt_v[live] + lam * nxt_a[live])
        advs[idx] = rets[idx] - v[idx]
        nxt_v[live], nxt_a[live] = v[idx], advs[idx]
    return advs, rets


# ---------------------------------------------------------------------------------------------- trainer hand-off
# PPO.data_to_torch / AZ.data_to_torch of the reference trainer (src/twisterl/rl/ppo.py:25-61, rl/az.py:28-46), from their definitions.
def onehot_ref(obs, obs_size):
    """np_obs[i, obs_i] = 1.0 (ppo.py:37-39): row i has a one in every column that appears among the ids of record i -- in any order,
    any number of times -- and zeros elsewhere.  float32 [n, obs_size]."""
    obs = np.asarray(obs, np.int64)
    obs = obs.reshape(obs.shape[0], -1) if obs.size else obs.reshape(obs.shape[0], 0)
    if obs.size and (obs.min() < 0 or obs.max() >= obs_size):
        raise ValueError(f"an obs id outside [0, {obs_size})")
    out = np.zeros((obs.shape[0], int(obs_size)), np.float32)
    for i in range(obs.shape[0]):
        out[i, obs[i]] = 1.0
    return out


def log_prob_f64(logits, actions):
    """Categorical(logits=l).log_prob(a) = l[a] - logsumexp(l) per row, in float64 (ppo.py:57-59).  A masked logit (-1e10) is an
    ordinary number: its term exp(-1e10 - max) is 0.0 in float64 whenever another action is legal."""
    l = np.asarray(logits, np.float64)
    a = np.asarray(actions, np.int64).reshape(-1)
    m = l.max(axis=1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    return l[np.arange(l.shape[0]), a] - lse


def normalized_adv_f64(advs):
    """(a - mean) / (std + 1e-8), std unbiased as torch.std (ppo.py:55-56), in float64.  One record: nan, as torch."""
    a = np.asarray(advs, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = a.std(ddof=1) if a.size > 1 else np.float64("nan")
        return (a - a.mean()) / (sd + 1e-8)


def log_prob_bound(n_actions, want, lse=0.0):
    """|f32 log-prob - log_prob_f64| per record for a kernel that computes (l[a] - max) - log(sum exp(l - max)) in f32:
    (A + 8) 2^-24 + 2^-23 |want|.  A rounded additions of terms <= 1 into a sum in [1, A] (relative to the sum, which the logarithm
    divides by), a few ulp for exp, log and the two subtractions, and the rounding of the result relative to its size.
    `lse`: |logsumexp(l)| per record for an implementation that forms l[a] - (max + log(sum)) instead, as torch's Categorical does
    (logits - logits.logsumexp()): max + log(sum) and the difference are rounded at the size of the logits, not of the result --
    2^-23 |lse| more.  With logits of size 50 that is 6e-6 on a log-prob that may be 1e-5: the form the hand-off kernel does not use."""
    return (int(n_actions) + 8) * 2.0 ** -24 + 2.0 ** -23 * (np.abs(np.asarray(want, np.float64)) + np.abs(np.asarray(lse, np.float64)))


def logsumexp_f64(logits):
    l = np.asarray(logits, np.float64)
    m = l.max(axis=1)
    return m + np.log(np.exp(l - m[:, None]).sum(axis=1))


def normalized_adv_bound(advs, want):
    """|f32 (a - mean) / (std + 1e-8) - normalized_adv_f64| per record, mean and std rounded to f32 from exact values:
    2^-23 (|a| + |mean|) / (std + 1e-8) for the subtraction and the rounded mean, 2^-23 |want| for the rounded denominator and the
    division."""
    a = np.asarray(advs, np.float64)
    sd = a.std(ddof=1)
    return 2.0 ** -23 * (np.abs(a) + abs(a.mean())) / (sd + 1e-8) + 2.0 ** -23 * np.abs(np.asarray(want, np.float64))


# ---------------------------------------------------------------------------------------------- a-priori error bounds
# Forward error of one Linear y = W^T x + b computed in a mode with rounded operands and f32 accumulation, against float64
# on the exact inputs:  |y^ - y| <= |W|^T err_in + gamma(k) (|W|^T |x| + |b|) + eta (|W|^T 1 + sum |x|),   k = fan_in + 1.
# ReLU is non-expansive, so the bound of a layer's output is the bound of its input to the next.  Per mode:
#   "f32"    (ARITH_REF / ARITH_CHAIN, Engine3, EngineV): operands exact, gamma = k u / (1 - k u), u = 2^-24, eta = 0;
#   "fp16x2" (EngineS): x = hi + lo + r with |r| <= 2^-22 |x| (+ a subnormal lo's 2^-25 at the x16 scale, 2^-29 unscaled),
#            lo * lo dropped (<= 2^-22 |W||x|); per product 3 x 2^-22 + 2^-44, three products per term accumulated in f32;
#   "fp16"   (ARITH_F16, Engine16): weights and activations rounded to binary16, 2^-11 each (+ 2^-25 below 2^-14).
# Valid while no operand overflows its format: |x| < 65504 in fp16; the split's range (tw_engine16x2.hpp) in fp16x2.
U32 = 2.0 ** -24
MODES = {
    #          relative error per product of two operands, absolute error per operand, accumulated terms per input
    "f32":    (0.0, 0.0, 1),
    "fp16x2": (3 * 2.0 ** -22 + 2.0 ** -44, 2.0 ** -29, 3),
    "fp16":   (2 * 2.0 ** -11 + 2.0 ** -22, 2.0 ** -25, 1),
}


def _gamma(mode, k):
    rel, _, per = MODES[mode]
    n = per * k
    return rel + n * U32 / (1 - n * U32) + rel * n * U32


def _layer_bound(mode, W, b, x, err):
    """float64 |W|^T err + gamma (|W|^T |x| + |b|) + eta (|W|^T 1 + sum |x|) for a batch x [n, in]."""
    aW, ax = np.abs(W), np.abs(x)
    eta = MODES[mode][1]
    out = err @ aW + _gamma(mode, W.shape[0] + 1) * (ax @ aW + np.abs(b))
    if eta:
        out += eta * (aW.sum(axis=0)[None, :] + ax.sum(axis=1, keepdims=True))
    return out


def forward_f64_bound(arrs, obs_perms, act_perms, obs, masks, perms, mode, emb_relu=True, chunk=8192):
    """forward_f64 plus an a-priori bound of |mode's result - float64| per logit and value (0 where the logit is masked).
    -> logits, values, err_logits, err_values.  Holds only inside the mode's range: see max_activations()."""
    emb, eb, common, action, value = arrs
    V = np.asarray(emb, np.float64)
    obs = np.asarray(obs, np.int64).reshape(len(obs), -1)
    n = obs.shape[0]
    masks = np.asarray(masks, bool).reshape(n, -1)
    perms = np.asarray(perms, np.int64).reshape(n)
    OP = np.asarray(obs_perms, np.int64) if len(obs_perms) else None
    AP = np.asarray(act_perms, np.int64) if len(act_perms) else None
    lay = lambda ls: [(np.asarray(w, np.float64).reshape(-1, np.asarray(b).size), np.asarray(b, np.float64), r) for (w, b, r) in ls]
    common, action, value = lay(common), lay(action), lay(value)
    ebias = np.asarray(eb, np.float64)
    rel, eta, _ = MODES[mode]
    A = _n_actions(emb, common, action)
    logits, values = np.empty((n, A)), np.empty(n)
    el, ev = np.zeros((n, A)), np.empty(n)

    def seq(layers, x, e):
        for W, b, r in layers:
            e = _layer_bound(mode, W, b, x, e)
            x = x @ W + b
            if r:
                x = np.maximum(x, 0.0)
        return x, e

    for s in range(0, n, chunk):
        ids, p = obs[s:s + chunk], perms[s:s + chunk]
        tw = p >= 0
        if tw.any():
            ids = ids.copy()
            ids[tw] = twist_ids(OP, p[tw], ids[tw])
        rows = V[ids] * (ids >= 0)[:, :, None]                           # [m, cells, emb]; a free slot (-1) adds nothing
        h = ebias + rows.sum(axis=1)
        # EmbeddingBag: the table entries are the rounded operands (one-hot x table), the bias an f32 addend
        e = _gamma(mode, ids.shape[1] + 1) * (np.abs(rows).sum(axis=1) + np.abs(ebias)) + eta * ids.shape[1]
        if emb_relu:
            h = np.maximum(h, 0.0)
        h, e = seq(common, h, e)
        v, evv = seq(value, h, e)
        la, ela = seq(action, h, e)
        m = slice(s, s + len(ids))
        values[m], ev[m] = v.sum(axis=1), evv.sum(axis=1)
        if tw.any():
            la[tw] = np.take_along_axis(la[tw], AP[p[tw]], axis=1)
            ela[tw] = np.take_along_axis(ela[tw], AP[p[tw]], axis=1)
        logits[m] = np.where(masks[m], la, MASKED)
        el[m] = np.where(masks[m], ela, 0.0)
    return logits, values, el, ev


def gae_bound_episodes(rews, vals, err_vals, ep_len, gamma, lam):
    """A bound of |f32 GAE of values v^ (|v^ - vals| <= err_vals) - gae_f64_episodes(rews, vals)| per record -> (err_advs,
    err_rets): the value errors carried through the recurrence plus f32 rounding (three roundings per step)."""
    advs, rets = gae_f64_episodes(rews, vals, ep_len, gamma, lam)
    L = np.asarray(ep_len, np.int64)
    starts = np.concatenate([[0], np.cumsum(L)[:-1]])
    r, v, dv = (np.asarray(x, np.float64) for x in (rews, vals, err_vals))
    ea, er = np.empty(r.size), np.empty(r.size)
    nxt_a = np.zeros(L.size)
    for k in range(int(L.max()) if L.size else 0):
        live = L > k
        idx = starts[live] + L[live] - 1 - k
        if k == 0:
            er[idx] = 0.0
        else:
            nxt = idx + 1
            er[idx] = gamma * (dv[nxt] + lam * nxt_a[live]) + 3 * U32 * (np.abs(r[idx]) + gamma * (np.abs(v[nxt]) + lam * np.abs(advs[nxt]))
                                                                           + np.abs(rets[idx])) * 1.01
        ea[idx] = er[idx] + dv[idx] + U32 * np.abs(advs[idx]) * 1.01
        nxt_a[live] = ea[idx]
    return ea, er


def max_activations(arrs, obs_perms, act_perms, obs, perms, emb_relu=True):
    """Largest |embedding output| and |hidden-layer output| (after the activation: common layers and the heads' hidden
    layers) over the records: what the f16 modes' ranges are stated in (fp16: 65504; fp16x2: 4095 and 255.94)."""
    emb, eb, common, action, value = arrs
    obs = np.asarray(obs, np.int64).reshape(len(obs), -1)
    p = np.asarray(perms, np.int64).reshape(-1)
    if (p >= 0).any():
        OP = np.asarray(obs_perms, np.int64)
        obs = obs.copy()
        obs[p >= 0] = twist_ids(OP, p[p >= 0], obs[p >= 0])
    h = embedding_bag_f64(emb, eb, emb_relu, obs)
    m0, m1 = float(np.abs(h).max()), 0.0
    for w, b, r in common:
        h = linear_f64(w, b, r, h)
        m1 = max(m1, float(np.abs(h).max()))
    for head in (action, value):
        x = h
        for w, b, r in head[:-1]:
            x = linear_f64(w, b, r, x)
            m1 = max(m1, float(np.abs(x).max()))
    return m0, m1


# ---------------------------------------------------------------------------------------------- predict / full_predict
SOFTMAX_EPS = 0.000001            # policy.rs:47,124
# Relative error of an f32 exp against the exact exponential of its f32 argument, MEASURED on the CPU against float64 (never on
# a GPU): the oracle's two_expf_det (the operation sequence the kernels' tw_expf repeats) and libm's expf over 2,000,001 evenly
# spaced f32 arguments of [-87, 88].  Measured maxima: 1.392 x 2^-24 (two_expf_det, at x = -59.956) and 0.999 x 2^-24 (glibc's
# expf).  Margin 4 x the larger, one rounding model for both implementations; tests/test_eval_matrix.py repeats the measurement
# on a coarser grid and on every in-range logit of tests/eval_matrix.py and holds it under a quarter of this constant.
EXP_REL = 4 * 1.392 * 2.0 ** -24
EXP_RANGE = 40.0                  # |logit| + its error below this: exp, the sum of 31 of them and every quotient are normal f32 numbers


def masked_softmax_f64(logits, masks):
    """policy.rs:43-47 / 118-124 in float64: exp(l) where the mask is set and 0 where it is not, over their sum + 1e-6.  No
    maximum is subtracted; a row without a legal action is 0 / 1e-6 = 0 everywhere."""
    l = np.asarray(logits, np.float64)
    m = np.asarray(masks, bool).reshape(l.shape)
    with np.errstate(over="ignore"):
        e = np.where(m, np.exp(np.where(m, l, 0.0)), 0.0)
        return e / (e.sum(axis=1, keepdims=True) + SOFTMAX_EPS)


def predict_f64(arrs, obs_perms, act_perms, obs, masks, perms, emb_relu=True):
    """Policy::predict_with_perm (policy.rs:39-49) on a batch -> (probs [n, A], values [n]) in float64; perms [n], -1 = no twist."""
    logits, values = forward_f64(arrs, obs_perms, act_perms, obs, masks, perms, emb_relu=emb_relu)
    return masked_softmax_f64(logits, masks), values


def _twist_average(per_twist):
    """policy.rs:109-115: acc += x_pi / n for pi = 0 .. n - 1, from 0."""
    acc = np.zeros_like(per_twist[0])
    for x in per_twist:
        acc = acc + x / float(len(per_twist))
    return acc


def full_predict_logits_f64(arrs, obs_perms, act_perms, obs, emb_relu=True):
    """The logits [n, A] and values [n] that Policy::full_predict (policy.rs:102-116) hands its soft-max, before any mask:
    the average over all twists, or the one un-twisted pass of a policy without twists (policy.rs:103)."""
    n = len(obs)
    legal = np.ones((n, _n_actions(arrs[0], arrs[2], arrs[3])), bool)
    if len(obs_perms) == 0:
        return forward_f64(arrs, (), (), obs, legal, np.full(n, -1), emb_relu=emb_relu)
    per = [forward_f64(arrs, obs_perms, act_perms, obs, legal, np.full(n, pi), emb_relu=emb_relu) for pi in range(len(obs_perms))]
    return _twist_average([l for l, _ in per]), _twist_average([v for _, v in per])


def full_predict_f64(arrs, obs_perms, act_perms, obs, masks, emb_relu=True):
    """Policy::full_predict (policy.rs:102-126) on a batch -> (probs [n, A], values [n]) in float64."""
    logits, values = full_predict_logits_f64(arrs, obs_perms, act_perms, obs, emb_relu=emb_relu)
    return masked_softmax_f64(logits, masks), values


def full_predict_f64_bound(arrs, obs_perms, act_perms, obs, mode="f32", emb_relu=True):
    """full_predict_logits_f64 plus an a-priori bound of |mode's f32 twist average - float64| -> logits, values, err_logits,
    err_values (all unmasked).  Twist pi contributes t = fl(x^ / n) with |x^ - x| <= e (forward_f64_bound): |t - x / n| <=
    (e + u (|x| + e)) / n; the n terms are added from 0 with n - 1 rounded additions: gamma(n - 1) sum |t| more."""
    n = len(obs)
    T = len(obs_perms)
    legal = np.ones((n, _n_actions(arrs[0], arrs[2], arrs[3])), bool)
    if T == 0:
        return forward_f64_bound(arrs, (), (), obs, legal, np.full(n, -1), mode, emb_relu=emb_relu)
    per = [forward_f64_bound(arrs, obs_perms, act_perms, obs, legal, np.full(n, pi), mode, emb_relu=emb_relu) for pi in range(T)]
    g = _gamma("f32", T - 1)

    def avg(xs, es):
        term_err = sum((e + U32 * (np.abs(x) + e)) / T for x, e in zip(xs, es))
        term_abs = sum((np.abs(x) + e) * (1 + U32) / T for x, e in zip(xs, es))
        return _twist_average(xs), term_err + g * term_abs

    logits, el = avg([p[0] for p in per], [p[2] for p in per])
    values, ev = avg([p[1] for p in per], [p[3] for p in per])
    return logits, values, el, ev


def prob_bound(logits, err_logits, masks, exp_rel=EXP_REL):
    """|f32 masked soft-max of logits l^ - masked_softmax_f64(l)| per entry, for |l^ - l| <= err_logits and a kernel that computes
    e_i = exp(l^_i) (0 where masked), S = e_0 + .. + e_{A-1} in index order, p_i = e_i / (S + 1e-6f), every operation rounded to f32
    (u = 2^-24):

      e^_i = exp(l_i) (1 + a_i),   |a_i| <= rho_i = expm1(err_i) + exp_rel exp(err_i)     (the shifted argument, then the exp itself);
      |S^ - sum e^_i| <= gamma(A - 1) sum e^_i                                              (A - 1 rounded additions of terms >= 0);
      D^ = fl(S^ + fl(1e-6)):  |D^ - D| <= dD = sum rho_i e_i + gamma(A - 1) sum (1 + rho_i) e_i + 1e-6 u + u (D + the three before);
      p^_i = fl(e^_i / D^)  =>  |p^_i - p_i| <= p_i ((1 + rho_i) (1 + u) / (1 - dD / D) - 1).

    A masked entry is exactly 0 on both sides.  Holds while every number is a normal f32: raises outside |l| + err < EXP_RANGE."""
    l = np.asarray(logits, np.float64)
    m = np.asarray(masks, bool).reshape(l.shape)
    el = np.where(m, np.asarray(err_logits, np.float64), 0.0)
    if m.any() and float((np.abs(l) + el)[m].max()) >= EXP_RANGE:
        raise ValueError("prob_bound: a legal logit outside the range the bound is derived for")
    e = np.where(m, np.exp(np.where(m, l, 0.0)), 0.0)
    rho = np.where(m, np.expm1(el) + exp_rel * np.exp(el), 0.0)
    g = _gamma("f32", l.shape[1] - 1)
    D = e.sum(axis=1) + SOFTMAX_EPS
    dD = (rho * e).sum(axis=1) + g * ((1 + rho) * e).sum(axis=1) + SOFTMAX_EPS * U32
    dD = dD + U32 * (D + dD)
    rD = dD / D
    if float(rD.max(initial=0.0)) >= 0.5:
        raise ValueError("prob_bound: the logit errors are too large for a bound of the quotient")
    want = e / D[:, None]
    return want * ((1 + rho) * (1 + U32) / (1 - rD[:, None]) - 1)
