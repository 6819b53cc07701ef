"""GPU: the 256-episode f32 rollout kernel reads its launch constants where it uses them (tw_rollout.hip: kernarg_view).

Inside the step loop the kernel no longer uses the copies of its arguments it loaded in front of the loop: the tail of a step, the
fast-forward rounds, the queue refill, the hand-over block and the observation's row look-up (Engine3::rows_of_args) read them from the
kernarg segment on either side of the forward.  A wrong offset, a constant read from the wrong place or a look-up that differs from
Engine3::rows_of shows in the records, so every case compares every field with the oracle's bytes and `reused_evals` with
tests/test_gpu_rollout_reuse.py's walk(o, 2, 2).

Cases (256 + 37 episodes: one workgroup of the 256-episode shape is full and 37 lanes take a second episode off the queue):
  * Puzzle-15, difficulty 6, twists {identity, transpose}, on ONE persistent workgroup (all CUs but one reserved): refills inside a
    round, the twist of a new episode drawn at the loop top, the look-back ring cleared; without the hand-over the count is exact;
  * the same collect with the hand-over at 1 and at 256 live episodes (the drain shape takes no records from the trajectory: the
    count can only fall);
  * the same shape at a non-zero episode offset and another seed (seed and offset enter every Philox key);
  * Puzzle-8, difficulty 4, no twists, the plain launch (the <8, 9, 8, false> instantiation: n_perms == 0, no queue);
  * Puzzle-15 at difficulty 0: every episode ends at its first record (reset() leaves the solved board), every lane goes straight
    back to the queue.
"""
import numpy as np
import pytest

from tests.test_gpu_rollout_drain import OFF, collect, same_fields
from tests.test_gpu_rollout_reuse import same_bytes, walk
from tests.util import amd_policy, oracle_policy, puzzle_transpose_twist
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

G = 0.995
E = 256 + 37
LOOK_BACK, ROUNDS = 2, 2       # REUSE_LB, REUSE_R of tw_rollout.hip


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


_cache = {}


def reference(oracle, side, diff, twists, seed, offset=0):
    """The oracle's collect of a case and walk(o, 2, 2): computed once, shared, never modified."""
    key = (side, diff, twists, seed, offset)
    if key not in _cache:
        import bench
        arrs = bench.synthetic_weights(side * side, seed=0)
        op, ap = puzzle_transpose_twist(side) if twists else ((), ())
        o = oracle.ppo_collect(oracle.Puzzle(side, side, diff, 2, 256), oracle_policy(oracle, arrs, op, ap), E, G, G, seed=seed,
                               episode_offset=offset, arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
        _cache[key] = (arrs, op, ap, o, walk(o, LOOK_BACK, ROUNDS)[0])
    return _cache[key]


def test_one_persistent_group_with_refills(tw, oracle, cus):
    arrs, op, ap, o, taken = reference(oracle, 4, 6, True, 1)
    assert taken > 0 and len(set(o.ep_len.tolist())) > 1          # records to take, ragged episodes
    g, cnt = collect(tw, cus, 4, 6, E, amd_policy(arrs, op, ap), 1, False, OFF)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512) and cnt == [0, 0]
    same_bytes(g.to_numpy(), o, 16)
    print(f"reused_evals {g.stats['reused_evals']} walk(o, 2, 2) {taken}")
    assert g.stats["reused_evals"] == taken
    assert g.stats["forward_evals"] == len(o.values)


@pytest.mark.parametrize("thr", [1, 256])
def test_hand_over_thresholds(tw, oracle, cus, thr):
    arrs, op, ap, o, taken = reference(oracle, 4, 6, True, 1)
    gp = amd_policy(arrs, op, ap)
    g, cnt = collect(tw, cus, 4, 6, E, gp, 1, False, thr)
    g_off, _ = collect(tw, cus, 4, 6, E, gp, 1, False, OFF)
    print(f"drain_live {thr}: handed over {cnt[0]}, drain grid {cnt[1]}, reused {g.stats['reused_evals']} of {taken}")
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512)
    assert cnt[0] <= thr and cnt[1] == 1                          # (the drain launch follows whatever the list holds: it reads the count on the device)
    if thr == 256:
        assert cnt[0] > 0                                          # the queue runs dry with episodes alive: they are handed over
    same_bytes(g.to_numpy(), o, 16)
    same_fields(g.to_numpy(), g_off.to_numpy())
    assert g.stats["reused_evals"] <= taken and g_off.stats["reused_evals"] == taken
    assert g.stats["forward_evals"] == len(o.values)


def test_episode_offset_and_second_seed(tw, oracle, cus):
    offset, seed = 100003, 77
    arrs, op, ap, o, taken = reference(oracle, 4, 6, True, seed, offset)
    base = reference(oracle, 4, 6, True, 1)[3]
    assert o.obs.shape != base.obs.shape or not np.array_equal(o.obs, base.obs)     # another trajectory than the first case's
    coll = tw.collector.PPOCollector(E, G, G, 32, merge_order=False, reserve_cus=cus - 1, episode_offset=offset)
    with _lib.launch_option(_lib.TW_OPT_FORCE_GEOM, 8), _lib.launch_option(_lib.TW_OPT_ROLLOUT_DRAIN, OFF):
        g = coll.collect(tw.env.Puzzle(4, 4, 6, 2, 256), amd_policy(arrs, op, ap), seed=seed)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512)
    same_bytes(g.to_numpy(), o, 16)
    assert g.stats["reused_evals"] == taken


def test_puzzle8_plain_launch_without_twists(tw, oracle, cus):
    arrs, op, ap, o, taken = reference(oracle, 3, 4, False, 1)
    assert taken > 0
    g, cnt = collect(tw, cus, 3, 4, E, amd_policy(arrs, op, ap), 1, False, OFF, reserve=0)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (2, 512) and cnt == [0, 0]     # no queue: two workgroups, the second one 37 episodes
    same_bytes(g.to_numpy(), o, 9)
    assert g.stats["reused_evals"] == taken


def test_every_episode_ends_at_reset(tw, oracle, cus):
    arrs, op, ap, o, taken = reference(oracle, 4, 0, True, 1)
    assert taken == 0 and o.ep_len.tolist() == [1] * E
    g, cnt = collect(tw, cus, 4, 0, E, amd_policy(arrs, op, ap), 1, False, OFF)
    assert (g.stats["rollout_blocks"], g.stats["rollout_threads"]) == (1, 512)
    same_bytes(g.to_numpy(), o, 16)
    assert g.stats["reused_evals"] == 0 and g.stats["forward_evals"] == E
