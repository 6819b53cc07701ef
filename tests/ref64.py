"""A float64 reference of the PPO policy forward and GAE, in plain numpy.

Written from the reference's definitions, not from the oracle's C code, so that a test can hold both the GPU and the oracle's own
f32 orders against an arithmetic neither of them uses:

* EmbeddingBag (layers.rs:56-86): bias + the sum of the rows of the obs ids in cell order, then ReLU when its flag is set.
* Linear (layers.rs:31-37): out = W x + b (+ ReLU), W in the export layout w[k * out + o] (src/twisterl/nn/utils.py:17-42).
* Policy::_raw_predict (policy.rs:79-100): embedding, common layers, value layers summed, action layers; a twist maps the obs ids
  through obs_perms[perm] (policy.rs:81-83) and gathers the logits by act_perms[perm] (policy.rs:95-97).
* Policy::forward_with_perm (policy.rs:56-65): masked logits are exactly -1e10.
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
    """EmbeddingBag on a batch of obs ids [n, cells] -> [n, vec_len] in float64: bias plus the rows in cell order."""
    V = np.asarray(vectors, np.float64)
    ids = np.asarray(ids, np.int64)
    h = np.broadcast_to(np.asarray(bias, np.float64), (ids.shape[0], V.shape[1])).copy()
    for c in range(ids.shape[1]):
        h += V[ids[:, c]]
    return np.maximum(h, 0.0) if relu else h


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
    A = np.asarray(action[-1][1]).size
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

    logits = np.empty((n, A), np.float64)
    values = np.empty(n, np.float64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ids, p = obs[s:e], perms[s:e]
        tw = p >= 0
        if tw.any():
            ids = ids.copy()
            ids[tw] = np.take_along_axis(OP[p[tw]], ids[tw], axis=1)
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
