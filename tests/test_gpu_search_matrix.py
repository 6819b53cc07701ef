"""GPU: every self-play, evaluate / solve and big-board kernel the build ships (tests/search_matrix.py, one row each) against the oracle.

Per row, in this order:
1. the launch the library reports (tw_debug_last_launch: family, template arguments and grid, written by the launcher from its own
   template parameters) is the row's kernel and the restated dispatch's launch shape -- for collects also `stats`' --, for the split
   shape the engine kernel's grid too;
2. self-play rows: the whole collect bit-equal to the oracle's ARITH_CHAIN (records in episode order; some rows of every family also in
   the merged order), no stored output offered for the wrong board and no wait that ran into its watchdog (debug counters 12 / 13),
   forward_evals >= records, and for the decoupled and split shapes a second collect with the same bytes;
3. the collect's own arrays in float64 / integers, whatever the oracle says (search_matrix.check_self_play_output: boards follow from
   each other by legal moves, probabilities are visits / searches, remaining_values is the f32 suffix sum of the states' rewards);
4. evaluate / solve rows: (success, total bits, steps) of every attempt (tw_debug_last_attempts) equal to the oracle's, the two means
   bit-equal to the oracle's attempts reduced in the reference's serial order (which, up to 8,192 attempts, is first held to
   oracle.evaluate's bits); solve rows: the oracle's action list, which replays on oracle.replay to the reported (success, reward);
5. big-board rows (25, 36, 64 cells): PPO collect, self-play and evaluate against the oracle, one row per instantiation.
No tolerance anywhere: these are the f32-exact paths.
"""
import contextlib
import os

import numpy as np
import pytest

from tests import search_matrix as sm
from tests.test_gpu_parity import _assert_same_az, _assert_same_collect
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays, make_policy_arrays, oracle_policy, puzzle_transpose_twist
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu
G = 0.995
SOLVE_MAX_DEPTH = 16           # solve() starts from set_state, whose depth is max_depth (puzzle.rs:107-117)


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


FAMILY = {_lib.TW_KERNEL_MCTS_F32: "mcts", _lib.TW_KERNEL_SOLVE_F32: "solve", _lib.TW_KERNEL_MCTS_DEEP: "deep", _lib.TW_KERNEL_MCTS_BIG: "mcts_big",
          _lib.TW_KERNEL_SOLVE_BIG: "solve_big", _lib.TW_KERNEL_ROLLOUT_BIG: "rollout_big"}


def reported_kernel(info):
    """tw_debug_last_launch -> the kernel tuple of search_matrix.kernel_name()."""
    fam = FAMILY.get(info["family"])
    if fam == "mcts":
        return (fam, info["nt"], info["nc"], info["nw"], bool(info["persist"]))
    if fam == "solve":
        return (fam, info["nt"], info["nc"], info["nw"])
    if fam == "deep":
        return (fam, info["nt"], info["nc"], info["nw"], info["nwk"], bool(info["solve"]), bool(info["dec"]), bool(info["split"]))
    return (fam, info["nc"])


def assert_launch(row, cus, stats=None):
    kernel, shape, engine = sm.dispatch(row, cus)
    info = _lib.debug_last_launch()
    label = sm.kernel_name(kernel)
    assert info["family"] != _lib.TW_KERNEL_NONE, (label, "the call launched none of the kernels")
    assert sm.kernel_name(reported_kernel(info)) == label, info
    assert (info["blocks"], info["threads"]) == shape, (label, info, shape)
    assert (info["engine_blocks"], info["engine_threads"]) == (engine or (0, 0)), (label, info, engine)
    if stats is not None:
        assert (stats["rollout_blocks"], stats["rollout_threads"]) == shape, (label, stats)
    return kernel


@contextlib.contextmanager
def options(row):
    with contextlib.ExitStack() as st:
        if row.force_geom:
            st.enter_context(_lib.launch_option(_lib.TW_OPT_FORCE_GEOM, row.force_geom))
        if row.variant:
            st.enter_context(_lib.launch_option(_lib.TW_OPT_AZ_VARIANT, row.variant))
        yield


def policies(oracle, row, seed=None):
    """(the library's policy, the oracle's) of a row; `seed`: other weights of the same shapes (default: the row's index in the table)."""
    n2, idx = row.w * row.h, sm.TABLE.index(row) if seed is None else seed
    op, ap = puzzle_transpose_twist(row.w) if row.twists else ((), ())
    if row.common is not None:
        arrs = make_deep_policy_arrays(n2, seed=idx, emb=row.emb, common=row.common, scale=2.0)
    else:
        arrs = make_policy_arrays(n2, seed=idx, emb=row.emb, hidden=row.hidden, scale=2.0)
    return amd_policy(arrs, op, ap), oracle_policy(oracle, arrs, op, ap)


def merged_too(row):
    """The rows that are also collected in the merged order: every eighth one, and the first row of every family."""
    if row not in sm.TABLE:                                           # (a further case of a kernel that has its row: tests/memory_matrix.py)
        return False
    idx = sm.TABLE.index(row)
    fam = lambda r: sm.dispatch(r, 256)[0][0]
    return idx % 8 == 0 or all(fam(r) != fam(row) for r in sm.TABLE[:idx])


def collect_self_play(tw, cus, row, gp, seed, merge_order=False):
    coll = tw.collector.AZCollector(row.E, row.S, 1.41, row.med, 32, merge_order=merge_order, reserve_cus=sm.reserve_cus(row, cus))
    with options(row):
        return coll.collect(tw.env.Puzzle(row.w, row.h, row.diff, 2, 256), gp, seed=seed)


def run_self_play(tw, oracle, cus, row, gp, opol, seed):
    """-> the collect (records in episode order) that was checked."""
    n2 = row.w * row.h
    oenv = oracle.Puzzle(row.w, row.h, row.diff, 2, 256)
    collect = lambda merge_order: collect_self_play(tw, cus, row, gp, seed, merge_order)

    g = collect(False)
    kernel = assert_launch(row, cus, g.stats)
    o = oracle.az_collect(oenv, opol, row.E, row.S, 1.41, row.med, seed=seed, arith=oracle.ARITH_CHAIN, num_threads=_threads(), merge_order=False, det_math=True)
    _assert_same_az(g, o, n2)
    counters = _lib.debug_counters(14)
    assert counters[12] == 0 and counters[13] == 0, counters
    assert g.stats["forward_evals"] >= len(o.obs)
    a = g.to_numpy()
    if kernel[0] == "deep" and (kernel[6] or kernel[7]):             # decoupled / split: which engine pass serves which walker when must not matter
        b = collect(False)
        assert_launch(row, cus, b.stats)
        b = b.to_numpy()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    sm.check_self_play_output(a, row)
    if merged_too(row):
        m = collect(True)
        assert_launch(row, cus, m.stats)
        _assert_same_az(m, oracle.az_collect(oenv, opol, row.E, row.S, 1.41, row.med, seed=seed, arith=oracle.ARITH_CHAIN, num_threads=_threads(),
                                             merge_order=True, det_math=True), n2)
    return g


def call_evaluate(tw, oracle, row, gp, seed):
    """The row's evaluate or solve (from episode 3's start board) -> (genv, start state or None, (success, reward), actions or None)."""
    solve = row.entry == "solve"
    max_depth = SOLVE_MAX_DEPTH if solve else 256
    genv = tw.env.Puzzle(row.w, row.h, row.diff, 2, max_depth)
    if solve:
        start = oracle.Puzzle(row.w, row.h, row.diff, 2, max_depth)
        start.reset(seed=seed, episode=3)
        state = start.get_state()
        genv.set_state(state)
        with options(row):
            (gs, gr), gact = tw.collector.solve(genv, gp, row.det, row.ns, row.S, 1.41, row.med, seed=seed)
        return genv, state, (gs, gr), gact
    with options(row):
        gs, gr = tw.collector.evaluate(genv, gp, num_episodes=row.E, deterministic=row.det, num_searches=row.ns, num_mcts_searches=row.S, seed=seed,
                                       C=1.41, max_expand_depth=row.med, num_cores=32)
    return genv, None, (gs, gr), None


def run_evaluate(tw, oracle, cus, row, gp, opol, seed):
    """-> ((success, reward), the solve's actions or None, the attempts) of the call that was checked."""
    solve = row.entry == "solve"
    max_depth = SOLVE_MAX_DEPTH if solve else 256
    oenv = oracle.Puzzle(row.w, row.h, row.diff, 2, max_depth)
    kw = dict(num_mcts_searches=row.S, seed=seed, Cc=1.41, max_expand_depth=row.med, arith=oracle.ARITH_CHAIN, det_math=True)
    genv, state, (gs, gr), gact = call_evaluate(tw, oracle, row, gp, seed)
    if solve:
        oenv.set_state(state)
    assert_launch(row, cus)
    # every attempt
    a_s, a_t, a_n = _lib.debug_last_attempts()
    o_s, o_t, o_n = oracle.evaluate_attempts(oenv, opol, row.E, row.det, row.ns, num_threads=_threads(), from_state=solve, **kw)
    assert len(a_s) == sm.attempts(row)
    assert np.array_equal(a_n, o_n), np.flatnonzero(a_n != o_n)[:8]
    assert np.array_equal(f32_bits(a_s), f32_bits(o_s)), np.flatnonzero(a_s != o_s)[:8]
    assert np.array_equal(f32_bits(a_t), f32_bits(o_t)), np.flatnonzero(f32_bits(a_t) != f32_bits(o_t))[:8]
    rate, mean, best = oracle.reduce_attempts(o_s, o_t, row.E, row.ns)
    if solve:
        (os_, or_), oact = oracle.solve(oenv, opol, row.det, row.ns, **kw)
        assert f32_bits(o_s[best[0]]) == f32_bits(os_) and f32_bits(o_t[best[0]]) == f32_bits(or_) and len(oact) == o_n[best[0]]
        assert (gs, f32_bits(gr)) == (os_, f32_bits(or_)) and gact == oact
        rp = oracle.Puzzle(row.w, row.h, row.diff, 2, max_depth)
        rp.set_state(state)
        _, _, rew, fin, boards = oracle.replay(rp, gact)             # the action list leads where the result says
        total = np.float32(0.0)
        for r in rew:
            total = np.float32(total + r)
        assert fin[-1] and not fin[:-1].any()
        assert gs == float(boards[-1].tolist() == list(range(row.w * row.h))) and f32_bits(gr) == f32_bits(total)
        assert genv.get_state() == state
        return (gs, gr), gact, (a_s, a_t, a_n)
    if sm.attempts(row) <= 8192:                                      # the reduction of the attempts is the reference's (serial: only up to here)
        ref = oracle.evaluate(oenv, opol, row.E, row.det, row.ns, **kw)
        assert f32_bits(ref[0]) == f32_bits(rate) and f32_bits(ref[1]) == f32_bits(mean), (ref, rate, mean)
    assert f32_bits(gs) == f32_bits(rate) and f32_bits(gr) == f32_bits(mean), (gs, gr, rate, mean)
    return (gs, gr), None, (a_s, a_t, a_n)


def collect_ppo(tw, row, gp, seed, merge_order=False):
    return tw.collector.PPOCollector(row.E, G, G, 32, merge_order=merge_order).collect(tw.env.Puzzle(row.w, row.h, row.diff, 2, 256), gp, seed=seed)


def run_ppo(tw, oracle, cus, row, gp, opol, seed):
    """-> the collect in episode order that was checked."""
    oenv = oracle.Puzzle(row.w, row.h, row.diff, 2, 256)
    first = None
    for merge_order in (False, True):
        g = collect_ppo(tw, row, gp, seed, merge_order)
        assert_launch(row, cus, g.stats)
        o = oracle.ppo_collect(oenv, opol, row.E, G, G, seed=seed, arith=oracle.ARITH_CHAIN, det_log=True, num_threads=_threads(), merge_order=merge_order)
        _assert_same_collect(g, o, row.w * row.h)
        first = g if first is None else first
    return first


@pytest.mark.parametrize("row", sm.TABLE, ids=[sm.row_id(r) for r in sm.TABLE])
def test_every_search_kernel_against_the_oracle(tw, oracle, cus, row):
    gp, opol = policies(oracle, row)
    seed = 100 + sm.TABLE.index(row)
    {"az": run_self_play, "evaluate": run_evaluate, "solve": run_evaluate, "ppo": run_ppo}[row.entry](tw, oracle, cus, row, gp, opol, seed)
