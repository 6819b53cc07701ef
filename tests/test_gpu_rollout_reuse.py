"""GPU: the fast-forward rounds of the 256-episode f32 rollout kernel (tw_rollout.hip).

A step whose board and twist the episode recorded 2 or 4 steps earlier takes that record's masked logits and value instead of a
column of a forward.  The policy output is a pure function of (board, twist), so every field of the collect must keep the oracle's
bytes, with the rounds on and with them off (TW_OPT_ROLLOUT_REUSE = 1), and `reused_evals` must lie between two walks of the
oracle's own trajectory:

  lo  look-back t-2 only, at most one hit after each forwarded record (any look-back >= 1 and any number of rounds >= 1 reaches it:
      the kernel takes every eligible record of a run except each (R+1)-th, the walk never two neighbours);
  hi  look-back t-2 / t-4 (the kernel's REUSE_LB = 2), runs of any length.

Shapes: Puzzle-15 with twists on the plain 256-episode launch (episodes whose depth runs out inside a round), Puzzle-8 without
twists (the n_perms == 0 path), and 66,000 short Puzzle-8 episodes on the persistent lanes (a lane whose episode ends on a hit
takes the next one off the queue inside the rounds).  bench.py's weights and twists; collect seed 7.
"""
import numpy as np
import pytest

from tests.util import amd_policy, f32_bits, oracle_policy
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 7
LOOK_BACK = 2          # REUSE_LB of tw_rollout.hip

#        name          side diff twists episodes force_geom
SHAPES = [("p15_plain", 4, 8, True, 512, 8),
          ("p8_no_twist", 3, 4, False, 512, 8),
          ("p8_persist", 3, 2, True, 66000, 0)]


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def walk(o, look_back, max_run):
    """(records taken from the trajectory, of those the ones that end their episode) when a record whose obs ids and twist equal
    those of the episode's record 2k steps earlier, k = 1 .. look_back, is taken -- at most max_run in a row."""
    obs = np.ascontiguousarray(o.obs); perms = np.asarray(o.perms)
    n = obs.shape[0]
    elig = np.zeros(n, dtype=bool)
    start = np.concatenate(([0], np.cumsum(o.ep_len.astype(np.int64))))      # (merge_order=False: episode-index order)
    t_of = np.arange(n) - np.repeat(start[:-1], o.ep_len)
    for k in range(1, look_back + 1):
        d = 2 * k
        same = np.zeros(n, dtype=bool)
        same[d:] = (obs[d:] == obs[:-d]).all(axis=1) & (perms[d:] == perms[:-d])
        elig |= same & (t_of >= d)
    last = np.zeros(n, dtype=bool); last[start[1:] - 1] = True
    taken = ends = run = 0
    for i in range(n):
        if t_of[i] == 0:
            run = 0
        if elig[i] and run < max_run:
            taken += 1; run += 1; ends += int(last[i])
        else:
            run = 0
    return taken, ends


_cache = {}


def reference(oracle, name):
    """The oracle's collect of a shape and the bounds walked from it: computed once, shared, never modified."""
    if name not in _cache:
        import bench
        _, side, diff, twists, E, _ = next(s for s in SHAPES if s[0] == name)
        arrs = bench.synthetic_weights(side * side, seed=0)
        op, ap = bench.transpose_twist(side) if twists else ((), ())
        o = oracle.ppo_collect(oracle.Puzzle(side, side, diff, 2, 256), oracle_policy(oracle, arrs, op, ap), E, 0.995, 0.995, seed=SEED,
                               arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
        lo, lo_ends = walk(o, 1, 1)
        hi, _ = walk(o, LOOK_BACK, 1 << 30)
        _cache[name] = (arrs, op, ap, o, lo, hi, lo_ends)
    return _cache[name]


def same_bytes(a, o, n_cells):
    assert a["obs"].shape == (o.obs.shape[0], n_cells)
    assert np.array_equal(a["ep_len"], o.ep_len)
    assert np.array_equal(a["obs"].astype(np.int64), o.obs)
    assert np.array_equal(a["actions"].astype(np.int64), o.actions)
    assert np.array_equal(a["perms"].astype(np.int32), o.perms)
    for f, ref in (("rewards", o.rewards), ("logits", o.logits), ("values", o.values), ("advs", o.additional_data["advs"]), ("rets", o.additional_data["rets"])):
        assert np.array_equal(f32_bits(a[f]), f32_bits(ref)), f


def collect_shape(tw, name, gp, off=0):
    """One collect of a shape with the fast-forward rounds on (off = 0) or off (1)."""
    _, side, diff, twists, E, geom = next(s for s in SHAPES if s[0] == name)
    with _lib.launch_option(_lib.TW_OPT_FORCE_GEOM, geom), _lib.launch_option(_lib.TW_OPT_ROLLOUT_REUSE, off):
        return tw.collector.PPOCollector(E, 0.995, 0.995, 32, merge_order=False).collect(tw.env.Puzzle(side, side, diff, 2, 256), gp, seed=SEED)


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_reused_records_keep_the_oracles_bytes(tw, oracle, name):
    check_shape(tw, oracle, name)


def check_shape(tw, oracle, name):
    """-> the collect with the rounds on that was checked."""
    _, side, diff, twists, E, geom = next(s for s in SHAPES if s[0] == name)
    arrs, op, ap, o, lo, hi, lo_ends = reference(oracle, name)
    print(f"[{name}] records {len(o.values)} lo {lo} hi {hi} hits at t-2 that end an episode {lo_ends}")
    assert 0 < lo <= hi                                   # the shape exercises the path ...
    if twists:
        assert lo_ends > 0                                # ... and an episode that ends on a hit (depth out / queue refill inside a round)
    gp = amd_policy(arrs, op, ap)
    g_on, g_off = collect_shape(tw, name, gp, 0), collect_shape(tw, name, gp, 1)
    (a_on, st_on), (a_off, st_off) = (g_on.to_numpy(), g_on.stats), (g_off.to_numpy(), g_off.stats)
    if geom == 0:
        assert st_on["rollout_blocks"] * 256 < E          # persistent lanes: fewer lanes than episodes, the queue refills them
    print(f"[{name}] reused_evals on {st_on['reused_evals']} off {st_off['reused_evals']} launch {st_on['rollout_blocks']} x {st_on['rollout_threads']}")
    same_bytes(a_on, o, side * side)
    same_bytes(a_off, o, side * side)
    for f in a_on:
        assert a_on[f].tobytes() == a_off[f].tobytes(), f
    assert st_off["reused_evals"] == 0
    assert st_on["forward_evals"] == st_off["forward_evals"] == len(o.values)
    assert lo <= st_on["reused_evals"] <= hi, (lo, st_on["reused_evals"], hi)
    return g_on
