"""GPU: the 256-episode rollout engine (Engine3, eight waves) with compile-time ring positions and the split Gumbel step.

Chunk c of every forward sits in ring slot c % 3; when the chunk count is not a multiple of three the forward ends with a bubble
whose streams are issued behind its last barrier.  Each residue of the chunk count (embedding 64 / 96 / 128 / 512 -> 4 / 6 / 8 /
32 chunks), boards with fewer cells than the kernel's cell count, and every hidden-size template of the engine are run with the
throughput shape forced and compared bit for bit with the oracle.  The Gumbel transform runs on two lanes per episode (uniforms
0-1 on the lower half, 2-3 on the upper): checked with NaN logits and masked logits against the oracle's single-lane argmax.
"""
import numpy as np
import pytest

from tests.util import amd_policy, f32_bits, make_policy_arrays, oracle_policy, puzzle_transpose_twist
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def _same_bits_or_both_nan(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(f32_bits(a[~nan]), f32_bits(b[~nan]))


def _collect_both(tw, oracle, arrs, w, h, diff, E, twists, seed):
    op, ap = puzzle_transpose_twist(w) if twists else ((), ())
    gp, orp = amd_policy(arrs, op, ap), oracle_policy(oracle, arrs, op, ap)
    with _lib.launch_option(_lib.TW_OPT_FORCE_GEOM, 8):
        g = tw.collector.PPOCollector(E, 0.995, 0.995, 32).collect(tw.env.Puzzle(w, h, diff, 2, 256), gp, seed=seed)
    o = oracle.ppo_collect(oracle.Puzzle(w, h, diff, 2, 256), orp, E, 0.995, 0.995, seed=seed, arith=oracle.ARITH_CHAIN, det_log=True)
    return g.to_numpy(), o


def _assert_same(a, o, n_cells, nan_ok=False):
    assert a["obs"].shape == (o.obs.shape[0], n_cells)
    assert np.array_equal(a["ep_len"], o.ep_len)
    assert np.array_equal(a["obs"].astype(np.int64), o.obs)
    assert np.array_equal(a["actions"].astype(np.int64), o.actions)
    assert np.array_equal(a["perms"].astype(np.int32), o.perms)
    assert np.array_equal(f32_bits(a["rewards"]), f32_bits(o.rewards))
    if nan_ok:
        assert _same_bits_or_both_nan(a["logits"], o.logits)
    else:
        assert np.array_equal(f32_bits(a["logits"]), f32_bits(o.logits))
    assert np.array_equal(f32_bits(a["values"]), f32_bits(o.values))
    assert np.array_equal(f32_bits(a["advs"]), f32_bits(o.additional_data["advs"]))
    assert np.array_equal(f32_bits(a["rets"]), f32_bits(o.additional_data["rets"]))


@pytest.mark.parametrize("w,h,diff,emb,hidden,E,twists", [
    (4, 4, 7, 64, 256, 300, True),      # 4 chunks: two bubbles' places, chunk 0 and chunk 1 of the next forward streamed behind it
    (4, 4, 7, 96, 256, 300, True),      # 6 chunks: no bubble
    (4, 4, 7, 128, 128, 300, False),    # 8 chunks: one bubble, hidden 128
    (4, 4, 6, 512, 256, 600, True),     # the benchmark's network: 32 chunks
    (3, 2, 5, 64, 64, 300, False),      # 6 cells on the 9-cell kernel (zero rows), hidden 64
    (3, 3, 5, 32, 32, 300, False),      # 2 chunks, hidden 32 (the MFMA head path)
    (2, 2, 3, 96, 256, 100, False),     # 4 cells on the 4-cell kernel
])
def test_throughput_engine_bit_exact_at_every_ring_phase(tw, oracle, w, h, diff, emb, hidden, E, twists):
    n2 = w * h
    arrs = make_policy_arrays(n2, seed=3, emb=emb, hidden=hidden)
    a, o = _collect_both(tw, oracle, arrs, w, h, diff, E, twists, seed=17)
    _assert_same(a, o, n2)


@pytest.mark.parametrize("nan_actions", [(0,), (1,), (2,), (3,), (1, 2), (0, 3)])
def test_split_gumbel_with_nan_and_masked_logits(tw, oracle, nan_actions):
    """A NaN action bias makes that logit NaN wherever the move is legal (a masked move's logit is -1e10 either way): the argmax
    over the lanes' halves must keep first-max-wins and NaN-never-wins exactly as the oracle's sequential scan."""
    arrs = make_policy_arrays(16, seed=8, emb=64, hidden=256)
    emb, eb, common, action, value = arrs
    (wa, ba, ra), = action
    ba = ba.copy()
    for i in nan_actions:
        ba[i] = np.float32("nan")
    arrs = (emb, eb, common, [(wa, ba, ra)], value)
    a, o = _collect_both(tw, oracle, arrs, 4, 4, 6, 400, True, seed=23)
    _assert_same(a, o, 16, nan_ok=True)
    assert np.isnan(a["logits"]).any()
