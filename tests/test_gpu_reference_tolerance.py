"""GPU: the north star's accuracy bound at the benchmark's full horizon, in every precision of the PPO rollout.

Returns and advantages must be within 1e-5 of the reference arithmetic (BASELINE.json north_star; TWO_ARITH_REF, nalgebra's
un-fused order).  Two workloads at the launch shape the bench times (262,144 envs, persistent lanes and the episode queue):

* headline: Puzzle-15, difficulty 128 (257-record episodes), bench.synthetic_weights(16, seed=0), the transpose twist,
  gamma = lambda = 0.995 -- BASELINE config 3;
* ragged: the reference's trained Puzzle-8 checkpoint at difficulty 32 -- episodes of every length, most of them solved.

On at least 2,048 episodes of each run (the first and last four and a seeded draw) the env is replayed on the oracle (obs,
masks, rewards and the terminal record bit-exact) and two references are built from the GPU's own obs, twists and masks:
REF = the oracle's reference-order forward and its f32 GAE, F64 = tests/ref64.py's float64 forward and GAE.  `fp32` and
`fp16x2` hold logits, values, advantages and returns within 1e-5 of both; `fp16` (a reduced-precision mode) within bounds
of about twice what it measured on the MI355X.
"""
import os

import numpy as np
import pytest
import torch

from tests.ref64 import forward_f64, gae_f64_episodes
from tests.util import f32_bits, trained_puzzle8_arrays

pytestmark = pytest.mark.gpu

E_FULL = 262_144
MASKED = np.float32(-1e10)
FIELDS = ("logits", "values", "advs", "rets")
F32_CLASS = {k: 1e-5 for k in FIELDS}
# fp16: about 2x the worst deviation from the float64 reference measured on the MI355X, per workload --
# headline 5.5e-5 / 5.6e-5 / 5.4e-5 / 6.7e-6, ragged (the trained policy's larger activations) 3.6e-3 / 3.0e-4 / 3.0e-4 / 1.2e-5
F16_BOUNDS = {
    "headline": {"logits": 1.1e-4, "values": 1.1e-4, "advs": 1.1e-4, "rets": 1.4e-5},
    "ragged": {"logits": 7.5e-3, "values": 6e-4, "advs": 6e-4, "rets": 2.5e-5},
}


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _workload(name):
    """-> (w, difficulty, policy arrays, obs_perms, act_perms, seed)"""
    if name == "headline":
        import bench
        op, ap = bench.transpose_twist(4)
        return 4, 128, bench.synthetic_weights(16, seed=0), op, ap, 1000
    return 3, 32, trained_puzzle8_arrays(), [], [], 77


def _episodes(E, seed, n_random=2048):
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, 3, E - 4, E - 3, E - 2, E - 1]
    return np.array(sorted(set(edge) | set(int(x) for x in rng.choice(E, size=n_random, replace=False))), np.int64)


def _gather(t, sel):
    """Records of the episodes `sel` (in that order) copied from the device: the slices only."""
    L = t["ep_len"].cpu().numpy().astype(np.int64)
    S = t["ep_start"].cpu().numpy().astype(np.int64)
    lens = L[sel]
    first = np.repeat(S[sel] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    idx = torch.from_numpy(first + np.arange(int(lens.sum()))).to(t["obs"].device)
    out = {k: t[k].index_select(0, idx).cpu().numpy() for k in ("obs", "logits", "perms", "values", "rewards", "actions", "advs", "rets")}
    return out, lens


def _replay(oracle, a, lens, sel, w, diff, seed):
    """Env replay of the GPU's actions on the oracle: obs, rewards, terminal flags bit-exact -> the masks of every record."""
    p = oracle.Puzzle(w, w, diff, 2, 256)
    masks = np.empty((lens.sum(), 4), bool)
    s = 0
    for e, n in zip(sel, lens):
        p.reset(seed=seed, episode=int(e))
        obs, m, rew, fin, _ = oracle.replay(p, a["actions"][s:s + n - 1].astype(np.int64))
        assert np.array_equal(obs, a["obs"][s:s + n].astype(np.int64)), e
        assert np.array_equal(f32_bits(rew), f32_bits(a["rewards"][s:s + n])), e
        assert fin[-1] and not fin[:-1].any(), e
        masks[s:s + n] = m
        s += n
    return masks


def _references(oracle, arrs, op, ap, a, masks, lens):
    obs = a["obs"].astype(np.int64)
    perms = a["perms"].astype(np.int32)
    lr, vr = oracle.Policy(*arrs, op, ap).forward_batch(obs, masks, perms, arith=oracle.ARITH_REF, num_threads=_threads())
    ar, rr = np.empty_like(vr), np.empty_like(vr)
    s = 0
    for n in lens:
        ar[s:s + n], rr[s:s + n] = oracle.gae(a["rewards"][s:s + n], vr[s:s + n], 0.995, 0.995)
        s += n
    l64, v64 = forward_f64(arrs, op, ap, obs, masks, perms)
    a64, r64 = gae_f64_episodes(a["rewards"], v64, lens, 0.995, 0.995)
    return {"REF": {"logits": lr, "values": vr, "advs": ar, "rets": rr},
            "F64": {"logits": l64, "values": v64, "advs": a64, "rets": r64}}


def _worst(g, ref, masks):
    """Largest |GPU - reference| per field (logits over the legal moves only)."""
    d = {"logits": float(np.max(np.abs(g["logits"][masks].astype(np.float64) - ref["logits"][masks])))}
    for k in ("values", "advs", "rets"):
        d[k] = float(np.max(np.abs(g[k].astype(np.float64) - ref[k])))
    return d


def _check(worst, bounds, label):
    bad = {k: v for k, v in worst.items() if not v < bounds[k]}
    assert not bad, f"{label}: worst deviation {worst} over the bounds {bounds} in {sorted(bad)}"


@pytest.mark.parametrize("precision", ["fp32", "fp16x2", "fp16"])
@pytest.mark.parametrize("workload", ["headline", "ragged"])
def test_within_bounds_of_the_reference_at_full_horizon(tw, oracle, workload, precision):
    import bench
    import twisterl_amd
    w, diff, arrs, op, ap, seed = _workload(workload)
    gp = bench.build_policy(arrs, op, ap)
    coll = tw.collector.PPOCollector(**{"num_episodes": E_FULL, "gamma": 0.995, "lambda": 0.995, "num_cores": 32}, precision=precision)
    g = coll.collect(tw.env.Puzzle(w, w, diff, 2, 256), gp, seed=seed)
    cus = twisterl_amd.device_info()["compute_units"]
    if precision == "fp32":      # the benched kernel: 8 waves x 32 episodes, one persistent workgroup per CU, the episode queue behind it
        assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (cus, 512)
    t = g.to_torch()
    sel = _episodes(E_FULL, seed=10 * ["headline", "ragged"].index(workload) + ["fp32", "fp16x2", "fp16"].index(precision))
    assert sel.size >= 2048 and sel[0] == 0 and sel[-1] == E_FULL - 1
    a, lens = _gather(t, sel)
    del t, g
    if workload == "headline":
        assert int((lens == 2 * diff + 1).sum()) >= 1000, np.bincount(lens)[-4:]
    else:
        assert np.unique(lens).size > 10 and (a["rewards"] == np.float32(1.0)).sum() > 0       # ragged, solved episodes among them
    masks = _replay(oracle, a, lens, sel, w, diff, seed)
    # masked logits are the reference's constant, bit for bit; every legal move has a finite logit
    assert np.array_equal(f32_bits(a["logits"][~masks]), f32_bits(np.full((~masks).sum(), MASKED)))
    assert np.isfinite(a["logits"][masks]).all() and not (a["logits"][masks] == MASKED).any()
    assert a["perms"].min() >= (0 if op else -1) and a["perms"].max() <= (len(op) - 1 if op else -1)
    refs = _references(oracle, arrs, op, ap, a, masks, lens)
    bounds = F32_CLASS if precision != "fp16" else F16_BOUNDS[workload]
    worst = {name: _worst(a, ref, masks) for name, ref in refs.items()}
    print(f"[ref-tol] {workload} {precision} episodes={sel.size} records={int(lens.sum())} worst={worst}")
    for name in refs:
        _check(worst[name], bounds, f"{workload}/{precision} vs {name}")
    # the check is not vacuous: a copy of the GPU's output with one field moved by 2e-5 fails the f32-class bound
    for k in FIELDS:
        moved = dict(a)
        moved[k] = a[k].copy()
        moved[k][masks if k == "logits" else slice(None)] += np.float32(2e-5)
        with pytest.raises(AssertionError):
            _check(_worst(moved, refs["F64"], masks), F32_CLASS, "perturbed")
