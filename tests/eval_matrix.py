"""Every branch of the two policy evaluate kernels, one named table row each (GPU-free).

`tw_policy_evaluate` (tw_api.hip) checks its arguments on the host and launches `policy_eval_kernel` for the one-common-layer
shape of `is_mfma_shape` and `policy_eval_generic_kernel` for every other Sequential stack (tw_eval.hip): one workgroup per
record, FORWARD / PREDICT / FULL_PREDICT after the reference's Policy::forward, predict and full_predict (policy.rs:34-126).
The same kernels evaluate every policy of the host-stepped collectors (tw_env_generic.hip).

A row fixes the policy (tests/util.py make_policy_arrays_obs / make_deep_policy_arrays_obs arguments plus the edits listed at
`policy_arrays`), obs_size and n_obs, the twists as (count, seed) of random permutations of the ids and of the actions, the
record generator ("full", "ragged": free slots (-1) among real ids, "free": records without any id), the mask generator
("random", "all", "none": every other record without a legal action, "one": exactly one legal action, "bytes": mask bytes
other than 0 and 1) and n; the perms are drawn in [-1, n_perms).  `in_range` rows are held against float64 (tests/ref64.py) and
bit for bit against the oracle; the others (exp pushed past what an f32 holds; eight-layer heads, see there) are compared with
the oracle alone.

tests/test_eval_matrix.py pins the table on the CPU (every row reaches the branch its comment names, the oracle lies inside the
float64 bounds, mutated results do not); tests/test_gpu_eval_matrix.py runs every row through Policy.evaluate_batch.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.util import make_deep_policy_arrays_obs, make_policy_arrays_obs

FORWARD, PREDICT, FULL_PREDICT = 0, 1, 2          # TW_EVAL_* (include/twisterl_hip.h)
EVAL_THREADS, EVAL_MAX_ACT, EVAL_GEN_W = 256, 32, 512

Row = namedtuple("Row", "name kind pol obs_size n_obs twists recs masks n in_range")


def _frozen(**pol):
    return tuple(sorted(pol.items()))           # (a row is a key of the caches below)


def B(name, A=4, emb=32, hidden=32, obs_size=40, n_obs=5, n=16, twists=None, recs="full", masks="random", in_range=True, **pol):
    """a row of policy_eval_kernel: embedding -> one common Linear of 32 / 64 / 128 / 256 units -> linear heads"""
    return Row(name, "basic", _frozen(gen="basic", emb=emb, hidden=hidden, n_actions=A, **pol), obs_size, n_obs, twists, recs, masks, n, in_range)


def G(name, A=4, emb=32, common=(24,), policy_layers=(), value_layers=(), obs_size=40, n_obs=5, n=16, twists=None, recs="full",
      masks="random", in_range=True, **pol):
    """a row of policy_eval_generic_kernel: any Sequential stack"""
    return Row(name, "generic", _frozen(gen="deep", emb=emb, common=tuple(common), policy_layers=tuple(policy_layers), value_layers=tuple(value_layers),
                                        n_actions=A, **pol), obs_size, n_obs, twists, recs, masks, n, in_range)


# The weight scale of the exp-range rows, chosen on the CPU (test_eval_matrix.py holds what it was chosen for): with it the oracle's
# logits pass +88.73 (two_expf_det returns inf) and -103.98 (it returns 0) in legal entries, and lie between -87.4 and -103.9
# (results below the smallest normal f32) in others, while every hidden activation stays far below the f32 maximum.
EXP_SCALE_BASIC, EXP_SCALE_GENERIC = 12.0, 12.0

TABLE = [
    # ================================================================================ policy_eval_kernel
    # ---- action counts: `tid < A` computes a logit, `tid == A` the value; act_perms rows of A bytes; the A-term soft-max loops
    B("basic-a1", A=1, masks="all"),                                    # thread 0 the logit, thread 1 the value; soft-max of one term
    B("basic-a2", A=2),
    B("basic-a3", A=3, twists=(1, 11)),
    B("basic-a5", A=5, twists=(2, 12)),                                 # act_perms[perm * 5 + tid]
    B("basic-a30", A=30),
    B("basic-a31", A=31, twists=(3, 13)),                               # tid == 31 == EVAL_MAX_ACT - 1 computes the value
    # ---- `if (id < 0) continue`: free slots of a shorter observation, with a twist table that must not be read at id -1
    B("basic-ragged", recs="ragged", twists=(2, 14)),
    B("basic-free", recs="free", twists=(1, 15)),                       # no id at all: the embedding is its bias
    # ---- n_obs: the inner loop over the slots, 1 and the largest tw_policy_evaluate takes
    B("basic-nobs1", n_obs=1),
    B("basic-nobs64", n_obs=64, obs_size=200, twists=(2, 16)),
    # ---- twist counts: `l / np` summed in pass order; 1 / 3 is not an f32
    B("basic-tw1", twists=(1, 17)),
    B("basic-tw2", twists=(2, 18)),
    B("basic-tw3", twists=(3, 19)),
    B("basic-notwist"),                                                 # FULL_PREDICT without twists: `full` false, one un-twisted pass
    # ---- masks: `m[i] ? .. : ..` on bytes; 0 / (0 + 1e-6)
    B("basic-allmasked", masks="none", twists=(2, 20)),
    B("basic-onelegal", A=5, masks="one"),
    B("basic-maskbytes", masks="bytes"),                                # 2, 0x80, 255 are legal
    B("basic-eps", act_shift=-14.0),                                    # legal sums of ~1e-6: the 1e-6 of the denominator decides
    # ---- pol.emb_relu / pol.common_relu off
    B("basic-norelu-emb", emb_relu=False),
    B("basic-norelu-common", common_relu=False, twists=(2, 21)),
    # ---- widths: `k += EVAL_THREADS` over an embedding above 256, `o += EVAL_THREADS` at exactly 256 hidden units
    B("basic-emb288-a5", emb=288, A=5, twists=(2, 22)),
    B("basic-emb512-a31", emb=512, hidden=64, A=31),
    B("basic-h256-a3", hidden=256, A=3),
    # ---- tw_expf past overflow and underflow (oracle only)
    B("basic-exp", masks="random", n=64, scale=EXP_SCALE_BASIC, in_range=False),
    # ================================================================================ policy_eval_generic_kernel
    # ---- the branches both kernels have, in the order of the rows above: action counts (`tid < A` gathers bufs[ao][src], the
    #      last LayerDev::out padded to four), free slots, n_obs, twist counts, masks, the 1e-6, the ReLU flags (EmbeddingBag; every
    #      LayerDev::relu of the common stack)
    G("generic-a1", A=1, masks="all"),
    G("generic-a2", A=2),
    G("generic-a3", A=3, twists=(1, 31)),
    G("generic-a5", A=5, twists=(2, 32)),
    G("generic-a30", A=30),                                             # LayerDev::out 32 for 30 outputs
    G("generic-a31", A=31, twists=(3, 33)),
    G("generic-ragged", recs="ragged", twists=(2, 34)),
    G("generic-free", recs="free", twists=(1, 35)),
    G("generic-nobs1", n_obs=1),
    G("generic-nobs64", n_obs=64, obs_size=200, twists=(2, 36)),
    G("generic-tw1", twists=(1, 37)),
    G("generic-tw2", twists=(2, 38)),
    G("generic-tw3", twists=(3, 39)),
    G("generic-notwist"),
    G("generic-allmasked", masks="none", twists=(2, 40)),
    G("generic-onelegal", A=5, masks="one"),
    G("generic-maskbytes", masks="bytes"),
    G("generic-eps", act_shift=-14.0),
    G("generic-norelu-emb", emb_relu=False),
    G("generic-norelu-common", common_relu=False, twists=(2, 41)),
    # ---- obs_size > 256: the two-byte twist table obs_perms16 (the one-byte table holds the ids modulo 256)
    G("generic-obs300-tw2", obs_size=300, twists=(2, 42)),
    G("generic-obs300-tw3-ragged", obs_size=300, recs="ragged", twists=(3, 43), A=5),
    # ---- widths: exactly EVAL_GEN_W; 257..511, the second trip of `o += EVAL_THREADS`; not a multiple of four (LayerDev::out padded)
    G("generic-w512", common=(512,), A=5),
    G("generic-emb512", emb=512, common=(40,)),
    G("generic-w300", common=(300,), A=3, twists=(2, 44)),
    G("generic-w30", common=(30,), policy_layers=(10,), value_layers=(6,), A=5),
    # ---- the value: a head of more than one output is summed over value_out (not over the padded LayerDev::out)
    G("generic-value3", common=(30,), value_outs=3, twists=(2, 45)),
    # ---- stacks without layers: an empty Sequential hands its input on
    G("generic-nocommon", common=()),                                   # the heads read the embedding buffer
    # the logits are the common output.  Regression row: nn.Policy took such a policy for one of zero actions and refused every mask
    G("generic-noaction", common=(8,), A=8, drop_action=True, twists=(2, 46)),
    G("generic-novalue", common=(30,), drop_value=True),                # the value is the sum of the 30 common outputs
    # ---- eight layers in a stack.  The a-priori float64 bound grows by the worst-case gain of every layer, ~scale * sqrt(width) / 2,
    # while a random ReLU stack loses its signal at about the same rate: a linear common stack of width 4 keeps both in hand;
    # seven hidden ReLU layers in both heads need scale 2.8 to tell the records apart, where that bound (~1e5) is wider than
    # the numbers themselves -- the row is compared with the oracle alone
    G("generic-8common", common=(4,) * 8, common_relu=False, A=3, twists=(2, 47), scale=1.7),
    G("generic-8heads", common=(16,), policy_layers=(12,) * 7, value_layers=(12,) * 7, A=3, twists=(2, 49), scale=2.8, in_range=False),
    G("generic-exp", masks="random", n=64, scale=EXP_SCALE_GENERIC, in_range=False),
    # ================================================================================ the two kernels on the same weights
    # one is_mfma_shape policy, and the same policy with its table extended to 257 rows that no record names: obs_size > 256
    # sends it to the generic kernel, every number it computes is the same
    B("cross-basic", emb=64, hidden=128, A=5, twists=(2, 48), seed=7),
    G("cross-generic", emb=64, common=(128,), A=5, twists=(2, 48), seed=7, obs_size=257, same_as="cross-basic"),
]

BY_NAME = {r.name: r for r in TABLE}
assert len(BY_NAME) == len(TABLE)


def base_row(row):
    """the row whose weights, twists and records this row repeats (itself, but for cross-generic)"""
    same = dict(row.pol).get("same_as")
    return BY_NAME[same] if same else row


def _rng(row, what):
    return np.random.default_rng(zlib.crc32(f"{base_row(row).name}/{what}".encode()))


@lru_cache(maxsize=None)
def policy_arrays(row):
    """-> (emb [obs_size][emb], emb bias, common, action, value) as tests/util.py makes them, then, by the row's `pol` entries:
    common_relu=False (no ReLU after the common layers), value_outs=k (the last value Linear ends in k outputs),
    drop_action / drop_value (the stack is empty), act_shift (added to the last action bias), same_as (the weights of another
    row, the table extended with rows nobody names).  emb_relu is an argument of the policy constructors, see emb_relu()."""
    base = base_row(row)
    p = dict(base.pol)
    seed, scale = p.get("seed", 1), p.get("scale", 1.0)
    if p["gen"] == "basic":
        arrs = make_policy_arrays_obs(base.obs_size, seed=seed, emb=p["emb"], hidden=p["hidden"], n_actions=p["n_actions"], scale=scale)
    else:
        arrs = make_deep_policy_arrays_obs(base.obs_size, seed=seed, emb=p["emb"], common=p["common"], policy_layers=p["policy_layers"],
                                           value_layers=p["value_layers"], n_actions=p["n_actions"], scale=scale)
    emb, eb, common, action, value = arrs
    common, action, value = list(common), list(action), list(value)
    if not p.get("common_relu", True):
        common = [(w, b, False) for (w, b, _) in common]
    if p.get("value_outs"):
        k, rng = p["value_outs"], _rng(row, "value_outs")
        fan_in = value[-1][0].size // value[-1][1].size
        bound = scale / np.sqrt(fan_in)
        value[-1] = (rng.uniform(-bound, bound, size=(fan_in, k)).astype(np.float32).reshape(-1), rng.uniform(-bound, bound, size=k).astype(np.float32), False)
    if p.get("drop_action"):
        action = []
    if p.get("drop_value"):
        value = []
    if p.get("act_shift"):
        w, b, r = action[-1]
        action[-1] = (w, (b + np.float32(p["act_shift"])).astype(np.float32), r)
    if row is not base:
        extra = _rng(row, "table").uniform(-1, 1, size=(row.obs_size - base.obs_size, emb.shape[1])).astype(np.float32)
        emb = np.ascontiguousarray(np.concatenate([emb, extra]))
    return (emb, eb, common, action, value)


def emb_relu(row):
    return bool(dict(base_row(row).pol).get("emb_relu", True))


def n_actions(row):
    return int(dict(base_row(row).pol)["n_actions"])


def is_basic_shape(row):
    """tw_api.hip is_mfma_shape on the row's policy: the policies policy_eval_kernel serves; every other runs the generic kernel."""
    emb, _, common, action, value = policy_arrays(row)
    if len(common) != 1 or len(action) != 1 or len(value) != 1:
        return False
    E, H, A = emb.shape[1], common[0][1].size, action[0][1].size
    return (E % 32 == 0 and H in (32, 64, 128, 256) and 1 <= A <= 31 and emb.shape[0] <= 256 and value[0][1].size == 1
            and not action[0][2] and not value[0][2])


@lru_cache(maxsize=None)
def twists(row):
    """-> (obs_perms [count][obs_size], act_perms [count][A]) as lists, random permutations; ((), ()) without twists"""
    base = base_row(row)
    if not base.twists:
        return (), ()
    count, seed = base.twists
    rng = np.random.default_rng(seed)
    A = n_actions(row)
    op = [rng.permutation(base.obs_size) for _ in range(count)]
    ap = [rng.permutation(A) for _ in range(count)]
    if row is not base:                                           # the ids nobody names map to themselves
        op = [np.concatenate([p, np.arange(base.obs_size, row.obs_size)]) for p in op]
    return tuple(tuple(int(x) for x in p) for p in op), tuple(tuple(int(x) for x in p) for p in ap)


@lru_cache(maxsize=None)
def records(row):
    """-> obs [n][n_obs] int32 (-1: a free slot), masks [n][A] uint8, perms [n] int32 in [-1, n_perms)"""
    base = base_row(row)
    rng = _rng(row, "records")
    n, n_obs, A = base.n, base.n_obs, n_actions(row)
    obs = rng.integers(0, base.obs_size, size=(n, n_obs)).astype(np.int32)
    if base.recs in ("ragged", "free"):
        free = rng.random((n, n_obs)) < 0.4
        free[0, :3] = (True, False, True)                         # a free slot before and after a real id
        free[1] = False
        if base.recs == "free":
            free[: n // 2] = True
        obs[free] = -1
    elif base.recs != "full":
        raise ValueError(base.recs)
    if base.masks == "all":
        masks = np.ones((n, A), np.uint8)
    elif base.masks in ("random", "none"):
        masks = rng.integers(0, 2, size=(n, A)).astype(np.uint8)
        masks[np.arange(n), rng.integers(0, A, size=n)] = 1
        if base.masks == "none":
            masks[::2] = 0
    elif base.masks == "one":
        masks = np.zeros((n, A), np.uint8)
        masks[np.arange(n), rng.integers(0, A, size=n)] = 1
    elif base.masks == "bytes":
        masks = rng.choice(np.array([0, 0, 0, 1, 2, 0x80, 255], np.uint8), size=(n, A))
        masks[np.arange(n), rng.integers(0, A, size=n)] = 2
    else:
        raise ValueError(base.masks)
    T = len(twists(row)[0])
    perms = rng.integers(-1, T, size=n).astype(np.int32)
    perms[: T + 1] = np.arange(-1, T)[:n]                         # every twist, and none, at least once
    for a in (obs, masks, perms):
        a.setflags(write=False)
    return obs, masks, perms


def cases():
    """the (mode, with a perms array) pairs every row runs"""
    return [(mode, wp) for mode in (FORWARD, PREDICT, FULL_PREDICT) for wp in (True, False)]


def oracle_policy(O, row):
    return O.Policy(*policy_arrays(row), *twists(row), emb_relu=emb_relu(row))


_oracle_cache = {}


def oracle_results(O, row, det_exp=True):
    """{(mode, with_perms): (logits or probs [n][A] f32, values [n] f32)} of the oracle in its ARITH_CHAIN order (the kernels'), the
    exp of the soft-max the deterministic one (the kernels' tw_expf) or libm's.  Computed once per row."""
    key = (row.name, bool(det_exp))
    if key not in _oracle_cache:
        obs, masks, perms = records(row)
        pol = oracle_policy(O, row)
        O.set_det_exp(bool(det_exp))
        try:
            out = {}
            for mode, wp in cases():
                if mode == FULL_PREDICT and not wp:
                    out[(mode, wp)] = out[(mode, True)]            # full_predict takes no perm (policy.rs:102)
                else:
                    out[(mode, wp)] = pol.evaluate_batch(mode, obs, masks, perms if wp else None, arith=O.ARITH_CHAIN)
        finally:
            O.set_det_exp(False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


_f64_cache = {}


def f64_results(row):
    """{(mode, with_perms): (want [n][A], want values [n], bound [n][A], bound values [n])} in float64 with the a-priori bounds of
    tests/ref64.py for the f32 order, for an in-range row.  Computed once per row."""
    from tests import ref64
    if row.name not in _f64_cache:
        assert row.in_range, row.name
        obs, masks, perms = records(row)
        arrs, (op, ap), er = policy_arrays(row), twists(row), emb_relu(row)
        out = {}
        for wp in (True, False):
            p = perms if wp else np.full(len(obs), -1)
            l, v, el, ev = ref64.forward_f64_bound(arrs, op, ap, obs, masks, p, "f32", emb_relu=er)
            out[(FORWARD, wp)] = (l, v, el, ev)
            out[(PREDICT, wp)] = (ref64.masked_softmax_f64(l, masks), v, ref64.prob_bound(l, el, masks), ev)
        l, v, el, ev = ref64.full_predict_f64_bound(arrs, op, ap, obs, "f32", emb_relu=er)
        out[(FULL_PREDICT, True)] = out[(FULL_PREDICT, False)] = (ref64.masked_softmax_f64(l, masks), v, ref64.prob_bound(l, el, masks), ev)
        _f64_cache[row.name] = out
    return _f64_cache[row.name]


def amd_policy(row):
    """twisterl_amd.nn.Policy of the row, through the constructor calls BasicPolicy.to_rust() makes"""
    from twisterl_amd import twisterl
    emb, eb, common, action, value = policy_arrays(row)
    seq = lambda ls: twisterl.nn.Sequential([twisterl.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    op, ap = twists(row)
    return twisterl.nn.Policy(twisterl.nn.EmbeddingBag(emb.tolist(), eb.tolist(), emb_relu(row), [emb.shape[0]], 0),
                              seq(common), seq(action), seq(value), [list(p) for p in op], [list(p) for p in ap])
