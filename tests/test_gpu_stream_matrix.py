"""GPU: every case of tests/stream_matrix.py on a caller's stream -- the family runners of tests/test_gpu_memory_matrix.py, their
assertions unchanged, under another driver.

`S` is one non-blocking torch.cuda.Stream per test, chosen so that it shares no hardware queue with the null stream (the runtime maps
streams onto a few hardware queues in turn, and two streams on one queue run in order whatever the library does:
tests/stream_util.py independent_stream).  A delay is torch.cuda._sleep(n) enqueued on a given stream, n from a calibration
made once per process with two events (cycles per millisecond, tests/stream_util.py).  Per case, with the same seed throughout:

  a  null stream, fill 0xFFFFFFFF: the row's own check against the oracle, numpy or float64, unchanged -> snapshot a.  The plain call
     that the other runs use is made once more on the null stream under a proxy that times the listed entry points: t_a, their sum.
     The delay of the case is max(MIN_DELAY_MS, 2 t_a); a case that would need more than MAX_DELAY_MS has to take a smaller shape.
  b  mode 1, the caller's stream is busy: inside _lib.library_stream(S), directly before each listed entry point of the case (collect,
     evaluate, solve, tw_collected_pack_trainer, tw_collected_adv_stats, the policy updates, tw_policy_evaluate) a delay on S and then an
     event m on S.  m.query() is false immediately before the call, and an entry point that waits for its stream returns with m
     complete.  Under the fill 0x00000001 first, then under 0xFFFFFFFF; each snapshot equals a byte for byte.  Work that should be on S
     but went to stream 0 runs before the fill and the memsets that precede it on S: it is overwritten by them, or it reads the
     pattern.  The mild pattern comes first, so that a misordering shows as different bytes from small in-range words and the case
     stops before the harsh one.
  c  hook off, on S, behind a delay, on the leftovers of the same call under P1's weights made on the null stream: equals a.  Here
     the cached workspace and the pooled arena cross streams.
  d  mode 2, the null stream is busy (the collect families): one unmeasured warm-up call on S, so that workspace and arena are cached;
     a delay and then an event z on the null stream; the call on S, under the fill 0x00000001 (the warm-up left the same bytes behind: with
     the fill a late producer shows).  Every field is read through the zero-copy tensors of to_torch(),
     copied to the host on S, so that nothing touches stream 0; then z.query() must still be false -- the call did not wait for
     unrelated null-stream work --; only then the full snapshot is taken.  Early fields and snapshot equal a.  A producer misrouted to
     stream 0 runs too late here.

Known limit: mode 1 is deterministic up to a call's first wait for its stream; what a call enqueues after that wait is no longer behind
the delay.  Mode 2 covers the rest for the collects.  For evaluate, solve and the hand-off everything lies before the first wait,
apart from the second sum of tw_collected_adv_stats.

Byte equality everywhere: there is no tolerance here.  With TW_STREAM_RECORD=<file> every case appends its calibration, t_a and delay.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import memory_matrix as mm
from tests import stream_matrix as st
from tests import stream_util as su
from tests import test_gpu_memory_matrix as G
from tests.test_gpu_memory_matrix import P1_SEED, _time_limit, assert_same, cus, device, snap_collected, tw  # noqa: F401 (fixtures)
from tests.util import amd_policy, f32_bits, make_deep_policy_arrays_obs
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

HARSH, MILD = 0xFFFFFFFF, 0x00000001
MIN_DELAY_MS = 50.0          # no delay is shorter: the preconditions then hold with room for the host's own jitter
SIDE_PROBE_MS = 80.0         # the delay of beside_the_side_stream: long against a split collect (under 10 ms), short against its watchdog (seconds)
MAX_DELAY_MS = 1000.0        # a case whose 2 t_a is above this takes a smaller shape


def _record(**what):
    path = os.environ.get("TW_STREAM_RECORD")
    print("[stream]", json.dumps(what))
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(what) + "\n")


class StreamDriver:
    """The driver a family runner gets instead of four_runs: runs a - d of the module docstring over check(pattern) / call(who, pattern)."""

    def __init__(self, case, stream):
        self.case, self.S = case, stream

    def beside_the_side_stream(self, call):
        """The split self-play shape runs walkers on the caller's stream and the engine on a side stream of the library's own, and the
        two kernels need each other: on a caller's stream that the runtime maps onto the side stream's hardware queue they cannot run
        side by side, the collect runs into its watchdog (seconds) and the process keeps the single-kernel shapes from then on.  Which
        queue the side stream got depends on what the process did before, so the case looks: a short delay is parked on the candidate
        and the call is made on the NULL stream; if the delay is still running when the call returns, the engine did not queue behind
        it and the candidate is taken, otherwise the next one.  (A candidate that shares the queue costs the probe SIDE_PROBE_MS, a
        hundredth of the watchdog's time.)"""
        S, rejected = self.S, []
        for _ in range(8):
            m = su.delay(S, SIDE_PROBE_MS)
            call("P2", None)
            free = not m.query()
            m.synchronize()
            if free:
                return S
            rejected.append(S)
            S = su.independent_stream(others=tuple(rejected))
        raise AssertionError(f"{self.case.id}: no stream runs beside the library's side stream")

    def __call__(self, mcase, check, call, leftovers=None):
        import torch
        sc, S = self.case, self.S
        assert S.cuda_stream != 0 and su.null_stream().cuda_stream == 0
        # ---- a
        with _lib.debug_fill_memory(HARSH):
            a = check(HARSH)
            with su.entry_proxy() as px:
                again = call("P2", HARSH)
        assert_same(a, again, f"{sc.id}: the plain call under 0xffffffff")
        seen = [n for n, _, status in px.calls if status == _lib.TW_OK]
        assert set(sc.entries) <= set(seen), (sc.id, sc.entries, seen)
        t_a = sum(ms for _, ms, _ in px.calls)
        delay_ms = max(MIN_DELAY_MS, 2.0 * t_a)
        _record(case=sc.id, cycles_per_ms=su.cycles_per_ms(), t_a_ms=round(t_a, 3), delay_ms=round(delay_ms, 1), calls=[(n, round(ms, 3)) for n, ms, _ in px.calls])
        assert delay_ms <= MAX_DELAY_MS, f"{sc.id}: t_a = {t_a:.0f} ms needs a delay of {delay_ms:.0f} ms: take a smaller shape"
        if "split" in getattr(mcase, "on", ()):
            S = self.S = self.beside_the_side_stream(call)
        # ---- b
        for p in (MILD, HARSH):
            with _lib.library_stream(S), _lib.debug_fill_memory(p), su.delayed_entries(S, delay_ms) as px:
                got = call("P2", p)
            assert [n for n, _, status in px.calls if status == _lib.TW_OK] == seen, (sc.id, px.calls, seen)
            assert_same(a, got, f"{sc.id}: on a busy caller's stream, fill {p:#010x}")
        assert _lib.debug_fill_memory._current() == G.HOOK_AT_START
        # ---- c
        first = (leftovers or call)("P1", None)
        if "field:logits" in first and "field:logits" in a:
            assert first["field:logits"] != a["field:logits"], f"{sc.id}: the other weights gave the same logits"
        del first
        with _lib.library_stream(S), su.delayed_entries(S, delay_ms):
            got = call("P2", None)
        assert_same(a, got, f"{sc.id}: hook off, on a busy caller's stream, on the leftovers of the same call made on the null stream under other weights")
        # ---- d
        if st.MODE2 not in sc.modes:
            return
        early = []

        def read_early(g):
            with torch.cuda.stream(S):
                host = {name: t.cpu().numpy() for name, t in g.to_torch().items()}
            early.append((not z.query(), host))
        with _lib.library_stream(S):
            warm = call("P2", None)
            del warm
            z = su.delay(su.null_stream(), delay_ms)
            assert not z.query()
            with G.before_snapshot(read_early), _lib.debug_fill_memory(MILD):     # (the fill: a late producer leaves the pattern, not the warm-up's equal bytes)
                got = call("P2", MILD)
        assert len(early) == 1, (sc.id, len(early))
        pending, host = early[0]
        if sc.id not in st.MODE2_EXEMPT:
            assert pending, f"{sc.id}: the call on the caller's stream returned only after the delay on the null stream had ended: it waits for unrelated null-stream work"
        for name, arr in host.items():
            dt, shape, data = a["field:" + name]
            assert (str(arr.dtype), arr.shape) == (dt, shape) and arr.tobytes() == data, f"{sc.id}: {name}, read on the caller's stream while the null stream was busy, differs"
        assert {"field:" + n for n in host} == {k for k in a if k.startswith("field:")}
        assert_same(a, got, f"{sc.id}: on the caller's stream while the null stream is busy")


# ------------------------------------------------------------------------------------------ the families no memory-matrix case has
def fam_denv16_ppo(case, tw, oracle, cus, driver):
    """The fp16 device-environment collect: tests/test_gpu_device_env_fp16.py's checks 3 - 7 on the GridWorld widths no tile divides."""
    from tests import test_gpu_device_env_fp16 as F
    _, key, E = case.ref
    c = F._width_case(key[len("gw3_"):])
    emb, common = F.WIDTHS[key[len("gw3_"):]]
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(make_deep_policy_arrays_obs(F.GW.obs_size, seed=P1_SEED, emb=emb, common=common, n_actions=4, scale=2.0))})
    who = {"P2": c, "P1": other}

    def check(p):
        g = F.collect(tw, c, E)
        F.assert_f16_launch(c, 0, (E + 15) // 16)
        F.check_collect(c, g, E)
        return snap_collected(g, p)

    def call(w, p):
        g = F.collect(tw, who[w], E)
        F.assert_f16_launch(c, 0, (E + 15) // 16)
        return snap_collected(g, p)
    driver(case, check, call)


def fam_denv16_solve(case, tw, oracle, cus, driver):
    """The fp16 device-environment solve with its action list, from a stepped state: the oracle's attempts, result and moves in ARITH_F16
    (tests/test_gpu_device_env_fp16_solve.py, test_solve_from_a_stepped_state, sampled)."""
    from tests import device_env_solve as D
    from tests import test_gpu_device_env_fp16_solve as T
    from tests.device_env_matrix import host_env
    O = oracle
    _, key, N = case.ref
    c = T.CASES[key]()
    emb, common = T.WIDTHS[key[len("gw3_"):]]
    pol = {"P2": c.gp, "P1": amd_policy(T.exact_arrays(T.GW.obs_size, emb, common, (), (), 4, seed=P1_SEED))}
    D.start(c.env, c.seed, T.SOLVE_EPISODE[key], 1)
    assert not c.env.is_final()
    start, before = host_env(c.env), c.env.state_bytes()

    def solve(w):
        got = tw.collector.solve(c.env, pol[w], False, N, 0, T.C_UCB, 1, seed=D.SEED, precision="fp16")
        T.assert_f16_launch(c, 0, (N + 15) // 16, from_state=1)
        assert c.env.state_bytes() == before
        return got, T.attempts()

    snap = lambda got, att: {"result": (got[0][0], f32_bits(np.float32(got[0][1])).tobytes()), "actions": tuple(got[1]), "attempts": tuple(x.tobytes() for x in att)}

    def check(p):
        per = [T.oracle_attempt(O, start, c, False, D.SEED, k, O.ARITH_F16) for k in range(N)]
        T.assert_exact_along(c, [s for q in per for s in q[3]])
        want = O.solve_env(start, c.op, False, N, 0, T.C_UCB, 1, seed=D.SEED, arith=O.ARITH_F16)
        want = ((float(want[0][0]), float(want[0][1])), [int(x) for x in want[1]])
        got, (s, t, k) = solve("P2")
        assert D.same(got, want), (got, want)
        assert np.array_equal(s, f32_bits([q[0] for q in per])) and np.array_equal(t, f32_bits([q[1] for q in per])) and \
            np.array_equal(k, np.asarray([len(q[2]) for q in per], np.uint32))
        exact, success, total = D.replay(c.env, got[1])
        assert exact and float(success) == got[0][0] and f32_bits(total) == f32_bits(got[0][1])
        assert len(got[1]) > 0
        return snap(got, (s, t, k))
    driver(case, check, lambda w, p: snap(*solve(w)))


def fam_denv16_eval(case, tw, oracle, cus, driver):
    """The fp16 device-environment evaluate, sampled: every attempt and the two means are the oracle's in ARITH_F16
    (tests/test_gpu_device_env_fp16_solve.py)."""
    from tests import test_gpu_device_env_fp16_solve as T
    _, key, (E, N) = case.ref
    c = T.CASES[key]()
    emb, common = T.WIDTHS[key[len("gw3_"):]]
    other = SimpleNamespace(**{**vars(c), "gp": amd_policy(T.exact_arrays(T.GW.obs_size, emb, common, (), (), 4, seed=P1_SEED))})
    who = {"P2": c, "P1": other}

    def call(w, p):
        got = T.gpu_evaluate(tw, who[w], E, N, False)
        T.assert_f16_launch(c, 0, (E * N + 15) // 16)
        return {"result": tuple(f32_bits(np.float32(x)).tobytes() for x in got), "attempts": tuple(x.tobytes() for x in T.attempts())}

    def check(p):
        o = T.oracle_evaluate(key, E, N, False, oracle.ARITH_F16)
        T.assert_exact_along(c, o.steps)
        snap = call("P2", p)
        T.same_attempts(o, T.attempts())
        assert snap["result"] == tuple(f32_bits(np.float32(x)).tobytes() for x in o.means)
        return snap
    driver(case, check, call)


def fam_policy_update(case, tw, oracle, cus, driver):
    """Policy.update_from_torch followed by a collect: the synced policy collects what a freshly created policy of the new weights
    collects, and has its image (tests/test_gpu_policy_sync.py)."""
    from tests import policy_sync_matrix as pm
    from tests.test_gpu_policy_sync import _build, _cuda, _image
    _, table, index = case.ref
    row = getattr(pm, table)[index]
    assert pm.is_generic(row) == (table == "GEN_TABLE") and row.obs_size == 16 and row.A == 4
    env = tw.env.Puzzle(2, 2, 4, 2, 256)
    collect = lambda pol: tw.collector.PPOCollector(300, 0.995, 0.995, 32, merge_order=False).collect(env, pol, seed=7)
    new = {"P2": pm.arrays(row, 2), "P1": pm.arrays(row, 3)}
    fresh = _build(row, new["P2"])                                         # (made on the null stream, before the driver sets another)

    def run(w, p, checked):
        pol = _build(row, pm.arrays(row, 1))
        state = _cuda(pm.torch_layout(new[w]))
        pol.update_from_torch(state)
        g = collect(pol)
        snap = snap_collected(g, p)
        snap["image"] = _image(pol)[0].tobytes()
        if checked:
            want = snap_collected(collect(fresh), p)
            want["image"] = _image(fresh)[0].tobytes()
            assert_same(want, snap, f"{case.id}: the synced policy against a fresh policy of the new weights")
        return snap
    driver(case, lambda p: run("P2", p, True), lambda w, p: run(w, p, False))


def fam_policy_eval(case, tw, oracle, cus, driver):
    """tw_policy_evaluate in its three modes, with and without a perms array: bit for bit the oracle's (tests/test_gpu_eval_matrix.py)."""
    from tests import eval_matrix as M
    from tests import test_gpu_eval_matrix as T
    _, name, _ = case.ref
    row = M.BY_NAME[name]
    p1 = M.amd_policy(M.B("stream-matrix-p1", twists=row.twists, seed=P1_SEED))          # the row's shapes and twists, other weights
    obs, masks, perms = M.records(row)
    snap = lambda got: {f"{mode}/{wp}": (f32_bits(o).tobytes(), f32_bits(v).tobytes()) for (mode, wp), (o, v) in got.items()}

    def check(p):
        got = T.evaluate(row)
        T.assert_oracle_bits(got, M.oracle_results(oracle, row), row.name)
        return snap(got)

    def call(w, p):
        pol = T.gpu_policy(row) if w == "P2" else p1
        return snap({(mode, wp): pol.evaluate_batch(mode, obs, masks, perms if wp else None) for mode, wp in M.cases()})
    driver(case, check, call)


FAMILIES = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("fam_")}


def test_every_family_of_the_table_has_its_runner():
    assert {c.family for c in st.CASES} == set(FAMILIES) | set(G.FAMILIES) and not set(FAMILIES) & set(G.FAMILIES)


@pytest.mark.parametrize("case_id", st.IDS)
def test_results_on_a_callers_stream(tw, oracle, cus, case_id):
    import torch
    case = st.BY_ID[case_id]
    S = su.independent_stream()
    driver = StreamDriver(case, S)
    try:
        if case.family in G.FAMILIES:
            G.FAMILIES[case.family](mm.BY_ID[case_id], tw, oracle, cus, driver=driver)
        else:
            FAMILIES[case.family](case, tw, oracle, cus, driver)
    finally:
        proxied = isinstance(_lib.lib(), su.EntryProxy)
        if proxied:
            _lib._lib = _lib.lib()._real
        _lib.lib().tw_set_stream(None)
        hook = _lib.debug_fill_memory._current()
        if hook != G.HOOK_AT_START:
            _lib.debug_fill_memory._set(G.HOOK_AT_START)
        torch.cuda.synchronize()
    assert not proxied and hook == G.HOOK_AT_START, (case_id, proxied, hook)     # no case leaves the proxy, a stream or the hook behind


def test_episode_order_hook_on_a_busy_stream(tw):
    """tw_debug_episode_order asks for the stream too (tests/stream_matrix.py `UNLISTED`): the same boards and order behind a delay."""
    env = tw.env.Puzzle(4, 4, 6, 2, 256)
    with _lib.debug_fill_memory(HARSH):
        want = _lib.debug_episode_order(env._desc(), 41, 5, 3000)
    S = su.independent_stream()
    for p in (MILD, HARSH):
        with _lib.library_stream(S), _lib.debug_fill_memory(p):
            m = su.delay(S, MIN_DELAY_MS)
            assert not m.query()
            got = _lib.debug_episode_order(env._desc(), 41, 5, 3000)
            assert m.query()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), hex(p)
