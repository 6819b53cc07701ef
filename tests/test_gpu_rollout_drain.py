"""GPU: the hand-over of the persistent 256-episode f32 rollout kernel (tw_rollout.hip, DESIGN.md 5.1, TW_OPT_ROLLOUT_DRAIN).

Once the episode queue is dry and at most N episodes of a workgroup still run, the workgroup appends them to a resume list and ends;
a second launch of the 32-episode persistent shape finishes them.  RNG is keyed by (episode, t), so which kernel runs a step cannot
matter: every field of every collect must keep the oracle's bytes and those of the same collect without the hand-over.

All CUs but one are reserved (as tests/kernel_matrix.py does), so one 256-lane workgroup is resident and a few hundred episodes are
a persistent launch; TW_OPT_FORCE_GEOM = 8 pins the 256-episode shape at that size.  tw_debug_counters reports the episodes handed
over and the drain launch's grid.  Every case's seed is the first of 1, 2, .. for which the last episode of the launch ends alone,
so that a threshold of 1 hands it over (where the last two end in one iteration the live count passes from 2 to 0 and a threshold of 1
hands nothing over; which episode starts at which iteration does not depend on the order the lanes reach the queue in, so the count is
the same every run).
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import _assert_same_collect
from tests.util import amd_policy, oracle_policy, puzzle_transpose_twist, trained_puzzle8_arrays
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 0.995
OFF = -1

#        name           side diff twists episodes weights  merge_order seed
CASES = [("p15_twists", 4, 6, True, 800, "bench", False, 1),
         ("p15_plain", 4, 5, False, 700, "bench", True, 1),
         ("p8_twists", 3, 8, True, 700, "bench", True, 1),
         ("p8_plain", 3, 3, False, 600, "bench", False, 4),
         ("p8_trained", 3, 6, False, 800, "trained", False, 1)]
THRESHOLDS = [1, 32, 256]


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def _weights(side, twists, weights):
    import bench
    arrs = trained_puzzle8_arrays() if weights == "trained" else bench.synthetic_weights(side * side, seed=0)
    op, ap = puzzle_transpose_twist(side) if twists else ((), ())
    return arrs, op, ap


_cache = {}


def reference(oracle, name):
    """The oracle's collect of a case: computed once, shared, never modified."""
    if name not in _cache:
        _, side, diff, twists, E, weights, merge, seed = next(c for c in CASES if c[0] == name)
        arrs, op, ap = _weights(side, twists, weights)
        o = oracle.ppo_collect(oracle.Puzzle(side, side, diff, 2, 256), oracle_policy(oracle, arrs, op, ap), E, G, G, seed=seed,
                               arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=merge)
        _cache[name] = (arrs, op, ap, o)
    return _cache[name]


def collect(tw, cus, side, diff, E, gp, seed, merge, drain, reserve=None, geom=8, extra=()):
    """-> (CollectedData, [episodes handed over, drain grid]) with the hand-over at `drain` live episodes (OFF: none)."""
    opts = [_lib.launch_option(_lib.TW_OPT_FORCE_GEOM, geom), _lib.launch_option(_lib.TW_OPT_ROLLOUT_DRAIN, drain)]
    opts += [_lib.launch_option(o, v) for o, v in extra]
    coll = tw.collector.PPOCollector(E, G, G, 32, merge_order=merge, reserve_cus=cus - 1 if reserve is None else reserve)
    for o in opts:
        o.__enter__()
    try:
        g = coll.collect(tw.env.Puzzle(side, side, diff, 2, 256), gp, seed=seed)
        return g, _lib.debug_counters(2)
    finally:
        for o in reversed(opts):
            o.__exit__(None, None, None)


def same_fields(a, b):
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), f


def check_hand_over(tw, oracle, cus, name, thr):
    """One collect of a case with the hand-over at `thr` live episodes: episodes were handed over, a second launch ran, the oracle's
    bytes.  -> (the collect, [episodes handed over, drain grid])"""
    _, side, diff, twists, E, weights, merge, seed = next(c for c in CASES if c[0] == name)
    arrs, op, ap, o = reference(oracle, name)
    g, cnt = collect(tw, cus, side, diff, E, amd_policy(arrs, op, ap), seed, merge, thr)
    assert 0 < cnt[0] <= min(thr, 256), (name, thr, cnt)
    assert 0 < cnt[1] <= cus - (cus - 1), (name, thr, cnt)                                  # at most CUs - reserve_cus workgroups
    _assert_same_collect(g, o, side * side)
    assert g.stats["forward_evals"] == len(o.values)
    return g, cnt


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_handed_over_episodes_keep_the_oracles_bytes(tw, oracle, cus, name):
    _, side, diff, twists, E, weights, merge, seed = next(c for c in CASES if c[0] == name)
    arrs, op, ap, o = reference(oracle, name)
    gp = amd_policy(arrs, op, ap)
    g_off, cnt_off = collect(tw, cus, side, diff, E, gp, seed, merge, OFF)
    assert (g_off.stats["rollout_blocks"], g_off.stats["rollout_threads"]) == (1, 512)      # the persistent 256-episode shape, one workgroup
    assert cnt_off == [0, 0]                                                                # no hand-over, no second launch
    _assert_same_collect(g_off, o, side * side)
    a_off = g_off.to_numpy()
    assert len(set(o.ep_len.tolist())) > 1                                                  # ragged episodes
    for thr in THRESHOLDS:
        g, cnt = check_hand_over(tw, oracle, cus, name, thr)
        print(f"[{name}] drain_live {thr}: handed over {cnt[0]}, drain grid {cnt[1]}, reused {g.stats['reused_evals']} (off: {g_off.stats['reused_evals']})")
        same_fields(g.to_numpy(), a_off)
        assert g.stats["forward_evals"] == g_off.stats["forward_evals"]
        assert g.stats["reused_evals"] <= g_off.stats["reused_evals"]                       # the drain shape runs no fast-forward rounds


def test_episode_at_its_last_step_and_episode_solved_in_the_hand_over_iteration(tw, oracle, cus):
    """Threshold 256, fast-forward rounds off, queue in index order: every iteration is one step of every live lane, so the schedule
    follows from the oracle's episode lengths -- an episode that starts at iteration s has its record t at iteration s + t, and the n
    lanes whose episodes end at iteration i take the next n queue entries, which start at i + 1.  The workgroup hands over at the
    loop top after the first lane found the queue dry.  The walk must find among the handed-over episodes one with a single step
    left (t == depth0 - 1) and among the episodes that ended in the iteration before one that was solved (not handed over), and
    the kernel must hand over exactly the walk's number; ep_len, rewards and the rest: the oracle's bytes."""
    side, diff, E, seed = 3, 3, 700, 3
    import bench
    arrs = bench.synthetic_weights(side * side, seed=0)
    op, ap = puzzle_transpose_twist(side)
    o = oracle.ppo_collect(oracle.Puzzle(side, side, diff, 2, 256), oracle_policy(oracle, arrs, op, ap), E, G, G, seed=seed,
                           arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
    L = o.ep_len.astype(np.int64)
    depth0 = int(L.max()) - 1                                    # (an episode that is never solved makes depth0 + 1 records)
    assert depth0 == 2 * diff
    start = np.zeros(E, dtype=np.int64)
    nxt, it, live = 256, 0, list(range(256))
    while True:                                                  # iteration `it`: who ends, who refills
        ended = [e for e in live if start[e] + L[e] - 1 == it]
        live = [e for e in live if start[e] + L[e] - 1 != it]
        dry = False
        for _ in ended:
            if nxt < E:
                start[nxt] = it + 1; live.append(nxt); nxt += 1
            else:
                dry = True
        it += 1
        if dry:
            break
    t_at = {e: it - start[e] for e in live}                      # the step each handed-over episode is at
    rew = np.split(o.rewards, np.cumsum(L)[:-1])
    solved_just_before = [e for e in ended if rew[e][-1] == np.float32(1.0)]
    print(f"hand-over at iteration {it}: {len(live)} live, {sum(1 for t in t_at.values() if t == depth0 - 1)} at depth 1, "
          f"{sum(1 for t in t_at.values() if t == depth0)} at depth 0, {len(ended)} ended in the iteration before ({len(solved_just_before)} solved)")
    assert 0 < len(live) < 256
    assert any(t == depth0 - 1 for t in t_at.values())           # depth 1 at the hand-over: one step left
    assert any(t == depth0 for t in t_at.values())               # depth 0: only the final record left
    assert solved_just_before
    gp = amd_policy(arrs, op, ap)
    extra = ((_lib.TW_OPT_ROLLOUT_REUSE, 1), (_lib.TW_OPT_AZ_VARIANT, 64))
    g, cnt = collect(tw, cus, side, diff, E, gp, seed, False, 256, extra=extra)
    assert cnt == [len(live), 1], (cnt, len(live))
    _assert_same_collect(g, o, side * side)
    a = g.to_numpy()
    g_off, cnt_off = collect(tw, cus, side, diff, E, gp, seed, False, OFF, extra=extra)
    assert cnt_off == [0, 0]
    a_off = g_off.to_numpy()
    same_fields(a, a_off)
    first = np.concatenate(([0], np.cumsum(L)))
    for e in list(t_at) + solved_just_before:                    # those episodes one by one: length, rewards, remaining
        assert a["ep_len"][e] == L[e]
        assert a["rewards"][first[e]:first[e + 1]].tobytes() == np.asarray(rew[e], dtype=np.float32).tobytes()
        if "remaining" in a:
            assert a["remaining"][first[e]:first[e + 1]].tobytes() == a_off["remaining"][first[e]:first[e + 1]].tobytes()


_FRESH = """
import hashlib, json, sys
sys.path.insert(0, {root!r})
import twisterl_amd
from tests import test_gpu_rollout_drain as T
tw = twisterl_amd.twisterl
cus = twisterl_amd.device_info()["compute_units"]
arrs, op, ap = T._weights(3, True, "bench")
g, cnt = T.collect(tw, cus, 3, 4, 650, T.amd_policy(arrs, op, ap), 12, True, 32)
a = g.to_numpy()
print(json.dumps({{"cnt": cnt, "sha": {{f: hashlib.sha256(a[f].tobytes()).hexdigest() for f in sorted(a)}}}}))
"""


def test_second_collect_of_a_collector_equals_a_fresh_process(tw, oracle, cus):
    """Two collects in a row with different seeds and sizes: the second one's bytes and hand-over count are those of a process
    that ran nothing before (the resume counter, the list and both queue words are reset on the stream, every collect)."""
    arrs, op, ap = _weights(3, True, "bench")
    gp = amd_policy(arrs, op, ap)
    first, cnt1 = collect(tw, cus, 3, 5, 900, gp, 11, True, 32)
    assert cnt1[0] > 0
    g, cnt = collect(tw, cus, 3, 4, 650, gp, 12, True, 32)
    a = g.to_numpy()
    o = oracle.ppo_collect(oracle.Puzzle(3, 3, 4, 2, 256), oracle_policy(oracle, arrs, op, ap), 650, G, G, seed=12,
                           arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=True)
    _assert_same_collect(g, o, 9)
    r = subprocess.run([sys.executable, "-c", _FRESH.format(root=ROOT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = json.loads(r.stdout.strip().splitlines()[-1])
    assert fresh["cnt"] == cnt and cnt[0] > 0
    assert fresh["sha"] == {f: hashlib.sha256(a[f].tobytes()).hexdigest() for f in sorted(a)}


def test_no_second_launch_without_a_queue_or_a_drain_shape(tw, oracle, cus):
    """At most the resident episodes (a plain launch) and hidden 64 (no 32-episode shape to drain into): no hand-over, no second
    launch, the oracle's bytes, whatever the option says."""
    from tests.util import make_policy_arrays
    arrs, op, ap = _weights(3, True, "bench")
    o = oracle.ppo_collect(oracle.Puzzle(3, 3, 4, 2, 256), oracle_policy(oracle, arrs, op, ap), 256, G, G, seed=5,
                           arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
    g, cnt = collect(tw, cus, 3, 4, 256, amd_policy(arrs, op, ap), 5, False, 32)           # E == resident: every lane has its episode
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512) and cnt == [0, 0]
    _assert_same_collect(g, o, 9)
    arrs64 = make_policy_arrays(9, seed=2, emb=64, hidden=64)
    o64 = oracle.ppo_collect(oracle.Puzzle(3, 3, 4, 2, 256), oracle_policy(oracle, arrs64, op, ap), 700, G, G, seed=5,
                             arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
    for drain in (0, 32, 256):
        g, cnt = collect(tw, cus, 3, 4, 700, amd_policy(arrs64, op, ap), 5, False, drain)
        assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512) and cnt == [0, 0], (drain, cnt)
        _assert_same_collect(g, o64, 9)
