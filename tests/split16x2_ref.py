"""The split-f16 forward of a generic stack (DESIGN.md §2 "Forward, split-f16 mode, generic stacks"; EngineV16x2,
twisterl_amd/csrc/tw_engine_generic16x2.hpp) restated in numpy for any depth, and the policies the GPU tests of that engine use.

* EmbeddingBag: f32 -- the bias plus the rows in id order, then ReLU (EngineV's embedding, bit for bit).
* Every Linear operand x, weight or activation, is carried as u = 16 x: hi = f16(u) (RNE), lo = f16(u - f32(hi)).
* One Linear, per k-group of 32 inputs: acc += W_hi x_hi, acc += W_hi x_lo, acc += W_lo x_hi, accumulated in f32 in that order
  (W_lo x_lo is dropped); then r = acc * 2^-8 + bias in f32, then ReLU.  The products of one k-group are summed exactly here
  (float64 holds 32 products of 22 bits) and rounded to f32 once when they join the accumulator; the order inside the MFMA is the
  hardware's, so a GPU result is held to the a-priori bound (tests/ref64.forward_f64_bound(mode="fp16x2")), not to these bits --
  except where every partial sum is exact in f32 (the exactness probe), where all orders agree.
* value = the f32 sum of the value head's outputs in index order; a twist maps the ids and gathers the logits; a masked logit is -1e10.

`drop` leaves one of the three products out (0: hi x hi, 1: W_hi x_lo, 2: W_lo x_hi): what a wrong engine would compute."""
import functools

import numpy as np

F32 = np.float32
SCALE = F32(16.0)
UNSCALE = F32(2.0 ** -8)
LIMIT = 4095.0                     # |16 x| < 65520: every |weight| and every |activation that feeds a Linear| below this


def split(x):
    """hi, lo (float16) of 16 x for an f32 array; hi + lo is 16 x up to 2^-22 relative."""
    u = np.asarray(x, F32) * SCALE
    with np.errstate(over="ignore", invalid="ignore"):
        hi = u.astype(np.float16)
        lo = (u - hi.astype(F32)).astype(np.float16)
    return hi, lo


def in_range(x):
    with np.errstate(invalid="ignore"):
        return bool((np.abs(np.asarray(x, F32) * SCALE) < 65520.0).all())


def linear(w, b, relu, x, drop=None):
    """One Linear of the spec on a batch x [n, in] (f32) -> [n, out] f32."""
    b = np.asarray(b, F32).reshape(-1)
    W = np.asarray(w, F32).reshape(-1, b.size)
    wh, wl = (a.astype(np.float64) for a in split(W))
    xh, xl = (a.astype(np.float64) for a in split(x))
    acc = np.zeros((x.shape[0], b.size), F32)
    for k0 in range(0, W.shape[0], 32):
        k = slice(k0, k0 + 32)
        for i, (xa, wa) in enumerate(((xh, wh), (xl, wh), (xh, wl))):
            if i != drop:
                acc = (acc.astype(np.float64) + xa[:, k] @ wa[k]).astype(F32)
    r = (acc * UNSCALE).astype(F32) + b
    return np.maximum(r, F32(0.0)) if relu else r


def embedding(vectors, bias, relu, ids):
    V = np.asarray(vectors, F32)
    ids = np.asarray(ids, np.int64)
    h = np.broadcast_to(np.asarray(bias, F32), (ids.shape[0], V.shape[1])).copy()
    for c in range(ids.shape[1]):
        h = (h + np.where(ids[:, c, None] >= 0, V[np.maximum(ids[:, c], 0)], F32(0.0))).astype(F32)
    return np.maximum(h, F32(0.0)) if relu else h


def forward(arrs, obs_perms, act_perms, obs, masks, perms, emb_relu=True, drop=None, fed=None):
    """Masked logits [n, A] f32 and values [n] f32.  `fed` (a list): every activation that feeds a Linear is appended to it."""
    emb, eb, common, action, value = arrs
    obs = np.asarray(obs, np.int64).reshape(len(obs), -1)
    perms = np.asarray(perms, np.int64).reshape(-1)
    tw = perms >= 0
    if tw.any():
        OP = np.asarray(obs_perms, np.int64)
        obs = obs.copy()
        obs[tw] = np.where(obs[tw] >= 0, np.take_along_axis(OP[perms[tw]], np.maximum(obs[tw], 0), axis=1), -1)
    h = embedding(emb, eb, emb_relu, obs)

    def seq(layers, x):
        for w, b, r in layers:
            if fed is not None:
                fed.append(x)
            x = linear(w, b, r, x, drop)
        return x

    h = seq(common, h)
    v = seq(value, h)
    val = np.zeros(v.shape[0], F32)
    for i in range(v.shape[1]):
        val = (val + v[:, i]).astype(F32)
    la = seq(action, h)
    if tw.any():
        la[tw] = np.take_along_axis(la[tw], np.asarray(act_perms, np.int64)[perms[tw]], axis=1)
    return np.where(np.asarray(masks, bool), la, F32(-1e10)).astype(F32), val


def weight_ceiling(arrs, n_obs):
    """(largest |weight|, an upper bound of every |activation that feeds a Linear|) from the weights alone: the embedding's output is
    at most n_obs x the largest table entry plus the bias; a layer's at most max over outputs of sum |w| x the input's bound + |b|."""
    emb, eb, common, action, value = arrs
    x = n_obs * float(np.abs(emb).max()) + float(np.abs(eb).max())
    top, wmax = x, 0.0

    def through(layers, x, top, wmax, last_feeds):
        for i, (w, b, _) in enumerate(layers):
            W = np.abs(np.asarray(w, np.float64).reshape(-1, len(b)))
            wmax = max(wmax, float(W.max()))
            x = float((W.sum(axis=0) * x + np.abs(np.asarray(b, np.float64))).max())
            if last_feeds or i < len(layers) - 1:
                top = max(top, x)
        return x, top, wmax

    x, top, wmax = through(common, x, top, wmax, True)
    for head in (action, value):
        _, top, wmax = through(head, x, top, wmax, False)
    return wmax, top


# ---- the policies of tests/test_gpu_device_env_fp16x2.py ----------------------------------------------------------------------------------
PROBE_ROWS = ("probe_o1a1", "probe_o4a2", "probe_o5a3v", "probe_o16a3", "probe_o17a2", "probe_o26a1v", "probe_o64a4s")
WIDE_ROWS = ("wideo17a17", "wideo16a16")
GW_OBS_SIZE, GW_N_OBS = 81, 9
# GridWorld 3 x 3 policies, the fp16 file's: (embedding, common layers)
WIDTHS = {"all_padding": (4, (4,)), "no_multiple": (36, (40, 20)), "wide": (512, (512, 272)), "no_common": (32, ())}


def width_arrays(key):
    from tests.util import make_deep_policy_arrays_obs
    emb, common = WIDTHS[key]
    return make_deep_policy_arrays_obs(GW_OBS_SIZE, seed=60 + len(key), emb=emb, common=common, n_actions=4, scale=2.0)


@functools.lru_cache(maxsize=None)
def exact_arrays():
    """The exactness probe.  Table and embedding bias: small integers, so the embedding's output is an integer and its lo term zero.
    Layer 1: weights m + n 2^-12 (m, n small non-zero integers, or 0), whose lo terms are not zero.  Later layers: integer weights (lo
    zero, so lo x lo is identically zero) over the fractional activations, whose lo terms are not zero.  Biases: half-integers.
    Every value is a multiple of 2^-12 below 2^11 in size, so every product and partial sum is exact in f32 in any order."""
    rng = np.random.default_rng(2025)

    def ints(shape, p, hi):
        v = rng.integers(1, hi + 1, size=shape).astype(F32) * rng.choice(F32([-1.0, 1.0]), size=shape)
        return np.where(rng.random(shape) < p, v, F32(0.0)).astype(F32)

    def half(n, lo, hi):
        return (rng.integers(lo, hi, size=n).astype(F32) + F32(0.5)).astype(F32)

    def lin(i, o, relu, p, hi, frac):
        w = ints((i, o), p, hi)
        if frac:
            w = np.where(w != 0, w + rng.integers(1, 4, size=w.shape).astype(F32) * rng.choice(F32([-1.0, 1.0]), size=w.shape) * F32(2.0 ** -12),
                         F32(0.0)).astype(F32)
        return (np.ascontiguousarray(w).reshape(-1), half(o, -2, 2), relu)

    emb = ints((GW_OBS_SIZE, 32), 0.5, 1)
    return (emb, rng.integers(-1, 2, size=32).astype(F32), [lin(32, 32, True, 0.25, 2, True), lin(32, 16, True, 0.25, 1, False)],
            [lin(16, 4, False, 0.5, 1, False)], [lin(16, 1, False, 0.5, 1, False)])


def all_policies():
    """(name, arrays, (obs twists, action twists), n_obs, obs_size) of every policy the GPU tests run in fp16x2."""
    from tests import device_env_matrix as M, device_env_wide as Wd
    out = [(m, M.policy_arrays(m), M.twists(m), M.BY_MODULE[m].n_obs, M.BY_MODULE[m].obs_size) for m in PROBE_ROWS]
    out += [(m, Wd.policy_arrays(m), Wd.twists(m), Wd.BY_MODULE[m].n_obs, Wd.BY_MODULE[m].obs_size) for m in WIDE_ROWS]
    out += [("gw3_" + k, width_arrays(k), ((), ()), GW_N_OBS, GW_OBS_SIZE) for k in sorted(WIDTHS)]
    out.append(("gw3_exact", exact_arrays(), ((), ()), GW_N_OBS, GW_OBS_SIZE))
    return out
