"""The episode sort (init_boards_kernel and the three episode_order_* kernels, tw_rollout.hip) where episode_order_shape doubles
the span of a wave: up to 64 x 16 x 1,024 = 1,048,576 episodes a wave sorts 1,024 indices (the benchmark's own size is the last
of these), from 1,048,577 on 2,048, from 2,097,153 on 4,096 -- 32 and 64 trips of the ballot-rank loop per wave, and a scratch
buffer sized by episode_order_scratch_bytes for the smaller grid.  test_gpu_parity.py holds the sizes up to 20,000.
Through the tw_debug_episode_order hook, with the same numpy check, vectorised: a few n-long arrays per size."""
import numpy as np
import pytest

from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

SEED, OFFSET = 41, 5


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def episode_order_shape(n):
    """tw_rollout.hip episode_order_shape -> (span, workgroups)"""
    sp = 1024
    while -(-n // (sp * 16)) > 64:
        sp *= 2
    return sp, -(-n // (sp * 16))


def check_order(boards, order, w, h):
    """the boards are permutations of the tiles, the order is a permutation of the episodes, sorted by decreasing sum of the tiles'
    Manhattan distances to their places (at most 63), ties in index order -> the keys"""
    n, cells = boards.size, w * h
    px, py = np.arange(16) % w, np.arange(16) // w           # the solved board holds tile v at cell v (the blank, 0, at cell 0)
    key = np.zeros(n, np.int32)
    seen = np.zeros(n, np.uint32)
    for i in range(cells):
        t = ((boards >> np.uint64(4 * i)) & np.uint64(15)).astype(np.int32)
        seen |= np.uint32(1) << t.astype(np.uint32)
        key += (np.abs(i % w - px[t]) + np.abs(i // w - py[t])).astype(np.int32) * (t != 0)
    assert np.all(seen == (1 << cells) - 1)                   # `cells` nibbles, every tile among them: a permutation
    assert cells == 16 or np.all(boards >> np.uint64(4 * cells) == 0)
    key = np.minimum(key, 63)
    assert np.array_equal(np.bincount(order, minlength=n), np.ones(n, np.int64))
    want = np.argsort(-key, kind="stable")
    assert np.array_equal(order.astype(np.int64), want)
    return key


@pytest.mark.parametrize("w,h,diff,n,span", [
    (4, 4, 8, 1_048_576, 1024),        # the last single-span size: 64 workgroups, 1,024 segments for the prefix kernel
    (4, 4, 8, 1_048_577, 2048),        # the first doubled size: 33 workgroups, the last one's first wave holds one episode
    (4, 4, 8, 2_097_153, 4096),        # doubled twice
    (2, 2, 3, 1_048_577, 2048),        # a handful of keys: every cursor of a wave advances by hundreds per trip
])
def test_episode_order_at_and_past_the_span_doubling(tw, w, h, diff, n, span):
    assert episode_order_shape(n)[0] == span and episode_order_shape(n)[1] <= 64
    env = tw.env.Puzzle(w, h, diff, 2, 256)
    boards, order = _lib.debug_episode_order(env._desc(), SEED, OFFSET, n)
    key = check_order(boards, order, w, h)
    populated = np.unique(key).size
    print(f"{w}x{h} n={n}: span {span}, {episode_order_shape(n)[1]} workgroups, {populated} keys populated, largest {key.max()}")
    assert 1 < populated <= (7 if w * h == 4 else 64)        # (three tiles at most two steps from their places: keys 0..6 on the 2 x 2 board)
    if n == 2_097_153:                                        # init_boards_kernel is indexed by the episode alone
        small, _ = _lib.debug_episode_order(env._desc(), SEED, OFFSET, 4096)
        assert np.array_equal(boards[:300], small[:300])
