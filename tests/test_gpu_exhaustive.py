"""GPU: EVERY episode of the benched launch shapes, bit for bit against the oracle.

The sampled full-size checks (tests/test_gpu_full_size.py) compare a few dozen of 262,144 episodes; a fault confined to one
lane pair, one hand-off of the episode queue or one ring phase would slip past them.  Here each collect is swept whole: the RNG is
keyed by the global episode index, so `oracle.ppo_collect(num_episodes=n, episode_offset=a, merge_order=False)` is the oracle's
version of episodes [a, a + n) of the big batch.  Shards of at most SHARD_RECORDS records keep host memory near 1 GB; only
the shard's slices leave the device (located through ep_start; merge order puts episode E-1 first).

* config 3 exactly as bench.py runs it (Puzzle-15, 262,144 envs, difficulty 128, transpose twist, seed-0 bench weights);
* config 2's shape in f32 as bench.side_configs runs it (65,536 Puzzle-8 envs, difficulty 32, bench weights);
* the episode queue at its edges: R = CUs x 256 resident lanes of the full shape, E in {R-1, R, R+1, 4R+37}, and where the
  small-batch shape takes the queue, E in {CUs x 32 - 1, CUs x 32 + 1}, with the trained Puzzle-8 policy (ragged episodes).
"""
import os

import numpy as np
import pytest

from tests.util import f32_bits, trained_puzzle8_arrays

pytestmark = pytest.mark.gpu

SHARD_RECORDS = 2_000_000
FIELDS = ("obs", "actions", "perms", "rewards", "logits", "values", "advs", "rets")


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def _cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def _tables(t, E):
    """ep_len / ep_start on the host, and the record-count identities of the merge order [E-1, 0, .., E-2]."""
    L = t["ep_len"].cpu().numpy().astype(np.int64)
    S = t["ep_start"].cpu().numpy().astype(np.int64)
    assert L.shape == (E,) and L.min() >= 1 and int(L.sum()) == t["obs"].shape[0]
    order = np.concatenate([[E - 1], np.arange(E - 1)])
    assert np.array_equal(S[order], np.concatenate([[0], np.cumsum(L[order])[:-1]]))
    return L, S


def _device_slices(t, S, L, a, b):
    """Records of episodes [a, b) in episode-index order, copied from the device run by run (episodes whose records are
    adjacent in the merged buffer form one run)."""
    runs, r0 = [], a
    for e in range(a + 1, b + 1):
        if e == b or S[e] != S[e - 1] + L[e - 1]:
            runs.append((int(S[r0]), int(S[e - 1] + L[e - 1])))
            r0 = e
    return {k: np.concatenate([t[k][s0:s1].cpu().numpy() for s0, s1 in runs]) for k in FIELDS}


def _first_bad_episode(ok_per_record, L, a):
    r = int(np.argmin(ok_per_record))
    return a + int(np.searchsorted(np.cumsum(L), r, side="right"))


def _sweep(oracle, t, E, oenv, op, seed, label, shard_ranges=None):
    """Every episode of the collect `t` (device tensors) against the oracle, field by field and bitwise."""
    L, S = _tables(t, E)
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    shard = max(1, SHARD_RECORDS // int(L.max()))
    lo, hi = shard_ranges if shard_ranges is not None else (0, E)
    for a in range(lo, hi, shard):
        b = min(hi, a + shard)
        o = oracle.ppo_collect(oenv, op, b - a, 0.995, 0.995, seed=seed, episode_offset=a, arith=oracle.ARITH_CHAIN, det_log=True,
                               num_threads=threads, merge_order=False)
        assert np.array_equal(o.ep_len.astype(np.int64), L[a:b]), (label, a, _first_bad_episode(o.ep_len == L[a:b], np.ones(b - a), a))
        g = _device_slices(t, S, L, a, b)
        want = {"obs": o.obs, "actions": o.actions, "perms": o.perms, "rewards": f32_bits(o.rewards), "logits": f32_bits(o.logits),
                "values": f32_bits(o.values), "advs": f32_bits(o.additional_data["advs"]), "rets": f32_bits(o.additional_data["rets"])}
        for k in FIELDS:
            got = g[k] if k in ("obs", "actions", "perms") else f32_bits(g[k])
            same = got == want[k]
            if same.ndim == 2:
                same = same.all(axis=1)
            assert same.all(), f"{label}: {k} differs from the oracle, first in episode {_first_bad_episode(same, L[a:b], a)} (shard {a}..{b})"
        del o, g, want


@pytest.fixture(scope="module")
def config3(tw, oracle):
    """BASELINE config 3 exactly as benched: one collect held on the device for the shard tests."""
    import bench
    arrs = bench.synthetic_weights(16, seed=0)
    op, ap = bench.transpose_twist(4)
    E, D = 262_144, 128
    coll = tw.collector.PPOCollector(**{"num_episodes": E, "gamma": 0.995, "lambda": 0.995, "num_cores": 32})
    g = coll.collect(tw.env.Puzzle(4, 4, D, 2, 256), bench.build_policy(arrs, op, ap), seed=1000)
    # the launch shape of the bench: 8 waves x 32 episodes per workgroup, one persistent workgroup per CU, the episode queue
    assert g.stats["rollout_threads"] == 512 and g.stats["rollout_blocks"] == _cus()
    t = g.to_torch()
    t["_keep"] = g
    return t, E, oracle.Puzzle(4, 4, D, 2, 256), oracle.Policy(*arrs, op, ap)


@pytest.mark.parametrize("part", range(4))
def test_config3_as_benched_every_episode(config3, oracle, part):
    t, E, oenv, op = config3
    q = E // 4
    _sweep(oracle, t, E, oenv, op, 1000, f"config3 part {part}", shard_ranges=(part * q, E if part == 3 else (part + 1) * q))


def test_config2_f32_every_episode(tw, oracle):
    """bench.side_configs' "config2_puzzle8_65k_f32": 65,536 Puzzle-8 envs at difficulty 32, bench weights, no twists, fp32."""
    import bench
    arrs = bench.synthetic_weights(9, seed=0)
    E, D = 65_536, 32
    coll = tw.collector.PPOCollector(**{"num_episodes": E, "gamma": 0.995, "lambda": 0.995, "num_cores": 32}, precision="fp32")
    g = coll.collect(tw.env.Puzzle(3, 3, D, 2, 256), bench.build_policy(arrs, [], []), seed=2)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (min(E // 256, _cus()), 512)
    _sweep(oracle, g.to_torch(), E, oracle.Puzzle(3, 3, D, 2, 256), oracle.Policy(*arrs, [], []), 2, "config2 f32")


def _queue_edges():
    """(label, E as a function of the CU count, launch shape (blocks, threads) as a function of the CU count)."""
    full = lambda c: (c, 512)               # 8 waves x 32 episodes; resident or persistent, one workgroup per CU
    small = lambda c: (c, 256)              # four waves share 32 episodes (Engine3S)
    return [
        ("R-1", lambda c: 256 * c - 1, full),          # every episode resident, the last workgroup one short
        ("R", lambda c: 256 * c, full),                # every lane resident exactly once
        ("R+1", lambda c: 256 * c + 1, full),          # one episode for the queue (without it: c + 1 workgroups)
        ("4R+37", lambda c: 1024 * c + 37, full),      # the queue hands out three rounds and a ragged tail
        ("32C-1", lambda c: 32 * c - 1, small),        # the small-batch shape, all resident
        ("32C+1", lambda c: 32 * c + 1, small),        # ... with the queue (without it: c + 1 workgroups)
    ]


@pytest.mark.parametrize("label", [q[0] for q in _queue_edges()])
def test_episode_queue_at_its_edges_every_episode(tw, oracle, label):
    import bench
    _, e_of, shape_of = next(q for q in _queue_edges() if q[0] == label)
    cus = _cus()
    E, D = e_of(cus), 32
    arrs = trained_puzzle8_arrays()
    coll = tw.collector.PPOCollector(**{"num_episodes": E, "gamma": 0.995, "lambda": 0.995, "num_cores": 32})
    g = coll.collect(tw.env.Puzzle(3, 3, D, 2, 256), bench.build_policy(arrs, [], []), seed=31)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == shape_of(cus), (label, E, g.stats["rollout_blocks"], g.stats["rollout_threads"])
    t = g.to_torch()
    L = t["ep_len"].cpu().numpy()
    assert L.min() < L.max()                                    # ragged: lanes refill at different times
    _sweep(oracle, t, E, oracle.Puzzle(3, 3, D, 2, 256), oracle.Policy(*arrs, [], []), 31, f"queue {label} (E={E})")
