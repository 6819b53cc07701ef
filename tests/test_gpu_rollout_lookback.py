"""GPU: the look-back ring of the 256-episode f32 rollout kernel (tw_rollout.hip).

The fast-forward rounds compare the pending step's (board, twist) with the episode's steps t-2 and t-4, which the kernel keeps in a
four-slot ring in LDS, and the twist of the pending step comes out of the Philox pass of the step before it (the lower half of a wave
draws the Gumbel words, the upper half the next twist).  Neither may change a byte: every case's collect with the rounds on has the
oracle's bytes in every field and is byte-equal to the collect with the rounds off, which reports no reused record.

`reused_evals` is checked exactly.  Per episode the kernel takes every eligible record of a run except each (R+1)-th (eligible: board
and twist equal to those at t-2 or t-4, t >= that distance); that does not depend on how the episodes share waves, so the count must be
tests/test_gpu_rollout_reuse.py's walk(o, 2, R) for exactly one R in 1..8, the same R in every case.  The hand-over is off
(TW_OPT_ROLLOUT_DRAIN = -1): the drain shape takes no records.

Cases: Puzzle-15 with twists at D = 8 on the plain launch (17 records: the ring wraps four times); Puzzle-8 without twists (the key
byte 0xff of n_perms == 0); and on ONE persistent workgroup (all CUs but one reserved) Puzzle-15 with twists and 800 episodes, and
Puzzle-8 with twists at D = 2 (5 records: a lane takes its next episode inside the rounds and finds the previous episode's entries in
the slots).  Each case's seed is the first of 1, 2, .. whose oracle trajectory holds a hit at t = 2, a hit at t = 4 that is no hit at
t-2, a hit that ends its episode and a run of eligible records longer than 4 -- at D = 2 an episode has the records t = 0..4, so the
longest run there is can have 3 records (t = 2, 3, 4) and that one is asked for instead.  All of it is asserted on the CPU before the
GPU runs, so no case passes for lack of cases.
"""
import numpy as np
import pytest

from tests.test_gpu_rollout_reuse import same_bytes, walk
from tests.util import amd_policy, oracle_policy
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

G = 0.995
LOOK_BACK = 2          # REUSE_LB of tw_rollout.hip

#        name             side diff twists episodes persistent
CASES = [("p15_plain_wrap", 4, 8, True, 512, False),
         ("p8_no_twist", 3, 4, False, 512, False),
         ("p15_one_group", 4, 6, True, 800, True),
         ("p8_refill_in_rounds", 3, 2, True, 800, True)]


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def features(o, diff):
    """What the oracle's trajectory holds of the paths the ring has: hits at t = 2, hits at t = 4 that are none at t-2, hits that end
    their episode, the longest run of eligible records, and the longest run the horizon allows (records t = 2 .. 2 * diff)."""
    obs = np.ascontiguousarray(o.obs); perms = np.asarray(o.perms)
    n = obs.shape[0]
    start = np.concatenate(([0], np.cumsum(o.ep_len.astype(np.int64))))      # (merge_order=False: episode-index order)
    t_of = np.arange(n) - np.repeat(start[:-1], o.ep_len)
    same = {}
    for d in (2, 4):
        m = np.zeros(n, dtype=bool)
        m[d:] = (obs[d:] == obs[:-d]).all(axis=1) & (perms[d:] == perms[:-d])
        same[d] = m & (t_of >= d)
    elig = same[2] | same[4]
    last = np.zeros(n, dtype=bool); last[start[1:] - 1] = True
    longest = run = 0
    for i in range(n):
        run = run + 1 if elig[i] and t_of[i] != 0 else int(elig[i])
        longest = max(longest, run)
    return {"t2": int((same[2] & (t_of == 2)).sum()), "t4_only": int((same[4] & ~same[2] & (t_of == 4)).sum()),
            "ends": int((elig & last).sum()), "longest": longest, "wanted_run": min(5, 2 * diff - 1)}


def has_all(f):
    return f["t2"] > 0 and f["t4_only"] > 0 and f["ends"] > 0 and f["longest"] >= f["wanted_run"]


_cache = {}
_rounds = {}           # case -> the R its count identified


def reference(oracle, name):
    """The oracle's collect of a case at its seed, the features found and walk(o, 2, R) for R = 1..8: computed once, shared, never modified."""
    if name not in _cache:
        import bench
        _, side, diff, twists, E, _ = next(c for c in CASES if c[0] == name)
        arrs = bench.synthetic_weights(side * side, seed=0)
        op, ap = bench.transpose_twist(side) if twists else ((), ())
        pol = oracle_policy(oracle, arrs, op, ap)
        for seed in range(1, 33):
            o = oracle.ppo_collect(oracle.Puzzle(side, side, diff, 2, 256), pol, E, G, G, seed=seed,
                                   arith=oracle.ARITH_CHAIN, det_log=True, num_threads=8, merge_order=False)
            f = features(o, diff)
            if has_all(f):
                break
        walks = [walk(o, LOOK_BACK, r)[0] for r in range(1, 9)]
        _cache[name] = (arrs, op, ap, seed, o, f, walks)
    return _cache[name]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_ring_hits_keep_the_oracles_bytes_and_the_exact_count(tw, oracle, cus, name):
    _, side, diff, twists, E, persistent = next(c for c in CASES if c[0] == name)
    arrs, op, ap, seed, o, f, walks = reference(oracle, name)
    print(f"[{name}] seed {seed} records {len(o.values)} hits at t=2 {f['t2']}, at t=4 only {f['t4_only']}, ending an episode {f['ends']}, "
          f"longest run {f['longest']} (wanted {f['wanted_run']}); walk(o, 2, R=1..8) {walks}")
    assert has_all(f), f                                   # the trajectory exercises every path (CPU only, before any launch)
    assert f["wanted_run"] == 5 or 2 * diff + 1 < 7        # a shorter run only where the horizon has none of 5
    gp = amd_policy(arrs, op, ap)
    env = tw.env.Puzzle(side, side, diff, 2, 256)

    def collect(off):
        coll = tw.collector.PPOCollector(E, G, G, 32, merge_order=False, reserve_cus=cus - 1 if persistent else 0)
        with _lib.launch_option(_lib.TW_OPT_FORCE_GEOM, 8), _lib.launch_option(_lib.TW_OPT_ROLLOUT_DRAIN, -1), \
             _lib.launch_option(_lib.TW_OPT_ROLLOUT_REUSE, off):
            g = coll.collect(env, gp, seed=seed)
        return g.to_numpy(), g.stats

    a_on, st_on = collect(0)
    a_off, st_off = collect(1)
    launch = (st_on["rollout_blocks"], st_on["rollout_threads"])
    print(f"[{name}] reused_evals on {st_on['reused_evals']} off {st_off['reused_evals']} launch {launch[0]} x {launch[1]}")
    assert launch == ((1, 512) if persistent else ((E + 255) // 256, 512))    # the 256-episode shape; persistent: one workgroup, the queue refills it
    same_bytes(a_on, o, side * side)
    same_bytes(a_off, o, side * side)
    for fld in a_on:
        assert a_on[fld].tobytes() == a_off[fld].tobytes(), fld
    assert st_off["reused_evals"] == 0
    assert st_on["forward_evals"] == st_off["forward_evals"] == len(o.values)
    rs = [r for r, w in zip(range(1, 9), walks) if w == st_on["reused_evals"]]
    print(f"[{name}] rounds R identified: {rs}")
    assert len(rs) == 1, (st_on["reused_evals"], walks)
    _rounds[name] = rs[0]
    assert len(set(_rounds.values())) == 1, _rounds         # the same R in every case of the file
