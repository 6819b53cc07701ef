"""GPU: what INTEGRATION.md ("Threads and streams") promises, from two threads and on two streams of one process.

One process, at most two threads, the handles used directly through twisterl_amd._lib.  The shape is small: the kernel matrix's row
(4, 4, 32, 32, 300), its policy (P2, whose collect tests/test_gpu_kernel_matrix.py's check_row holds to the oracle first) and a second
policy of other weights (P1, whose reference is its own collect on the null stream from one thread).  Streams are chosen so that they
share no hardware queue with the null stream or with each other (tests/stream_util.py independent_stream): only then does a missing
fence show.  Every comparison is of bytes.

* a result is freed by another thread, which never called tw_set_stream, while a pack kernel the producer queued on its own stream is
  still pending behind a delay; the freeing thread's next collects take the same arena out of the pool (under the fills 0x00000000 and
  0x00000001: a broken fence shows as wrong bytes from in-range actions and ids, never as an out-of-range index).  The pack's tensors
  equal the same pack done beforehand without a delay, which is itself held to tests/ref64.py as tests/test_gpu_trainer_handoff.py
  does; the other thread's collects equal their reference;
* the same on one thread with two streams;
* the fence's other half: the pack is pending on the FREEING stream (the consumer's), the result was produced on another; the producing
  stream's next collects into the same arena wait for it;
* the hand-off queued behind a delay and a refill of its destination tensors on the caller's stream still comes last, for one-byte and
  two-byte obs ids;
* two threads on two streams start together: a Puzzle collect and a device-environment collect, three times each, serialised by the
  library; every result equals its single-threaded snapshot;
* the stream is thread-local: while thread A's stream is parked behind a delay, thread B's collect returns with the right bytes and the
  delay still pending; A's collect waits for it; after A has exited with its stream still set, the main thread still launches on the
  null stream;
* tw_release_cached_memory with a live result made on a stream: its bytes stay, and the next collect under a fill is byte-equal.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests import ref64
from tests import stream_util as su
from tests.test_gpu_memory_matrix import P1_SEED, cus, device, tw  # noqa: F401 (fixtures)
from tests.util import f32_bits
from twisterl_amd import _lib
from twisterl_amd.collector import CollectedData, _DeviceResult

pytestmark = pytest.mark.gpu

ROW = km.R(4, 4, 32, 32, 300)
assert ROW in km.TABLE
SEED = 100 + km.TABLE.index(ROW)
OBS_SIZE = 256
PARK_MS = 200.0              # a parked delay: long against the few milliseconds of everything that has to happen under it
JOIN_S = 120


class Result:
    """A tw_collected handle owned by the test: freed where and when the test says."""

    def __init__(self, handle):
        self.dev = _DeviceResult(handle)
        self.data = CollectedData._from_device(self.dev)

    @property
    def h(self):
        return self.dev.h

    def base(self):
        return int(_lib.lib().tw_collected_device_ptr(self.dev.h, _lib.TW_F_OBS, None) or 0)

    def snap(self):
        return {name: (str(a.dtype), a.shape, a.tobytes()) for name, a in self.data.to_numpy().items()}

    def free(self):
        h, self.dev.h = self.dev.h, None
        _lib.lib().tw_collected_free(h)


def raw_collect(tw, policy):
    """tw_ppo_collect of ROW with the policy on the calling thread's library stream -> Result."""
    env = tw.env.Puzzle(ROW.w, ROW.h, ROW.diff, 2, 256)
    desc = env._desc()
    from tests.test_gpu_kernel_matrix import G
    prm = _lib.PPOParams(ROW.E, 0, G, G, SEED, _lib.TW_PREC_F32_EXACT, 0, 0)
    out = C.c_void_p()
    _lib.check(_lib.lib().tw_ppo_collect(C.byref(desc), policy._handle(), C.byref(prm), C.byref(out)))
    return Result(out.value)


def pack_tensors(n):
    import torch
    t = (torch.empty((n, OBS_SIZE), dtype=torch.float32, device="cuda"), torch.empty((n,), dtype=torch.float32, device="cuda"),
         torch.empty((n,), dtype=torch.int64, device="cuda"), torch.empty((n,), dtype=torch.int64, device="cuda"),
         torch.empty((n,), dtype=torch.float32, device="cuda"))
    for x in t:
        x.fill_(7)                                        # (what a pack that never ran would leave)
    torch.cuda.synchronize()
    return t


def refill(tensors, stream):
    """Sets the tensors to 7 again, on `stream`: what the caller had queued there before it asked for the pack."""
    import torch
    with torch.cuda.stream(stream):
        for x in tensors:
            x.fill_(7)


def raw_pack(res, tensors):
    """tw_collected_pack_trainer of every record, without normalisation: enqueued on the calling thread's library stream, not waited for."""
    p = [C.c_void_p(x.data_ptr()) for x in tensors]
    _lib.check(_lib.lib().tw_collected_pack_trainer(res.h, OBS_SIZE, 0, 0, res.dev.n, *p))


def tensor_bytes(tensors):
    return [x.cpu().numpy().tobytes() for x in tensors]


def run_threads(*bodies):
    """Runs each body in a thread of its own and hands the first exception on."""
    errors = []

    def guard(fn):
        def run():
            try:
                fn()
            except BaseException as e:      # noqa: BLE001 (handed to the main thread)
                errors.append(e)
        return run
    threads = [threading.Thread(target=guard(b)) for b in bodies]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
        assert not t.is_alive(), "a thread of the test did not end"
    if errors:
        raise errors[0]


@pytest.fixture(scope="module")
def ref(tw, oracle, cus):
    """P2 (the row's policy; its collect checked against the oracle and float64 by the kernel matrix's helper), P1 (other weights), their
    null-stream snapshots, and P2's pack without a delay, held to tests/ref64.py."""
    import torch
    from tests import test_gpu_kernel_matrix as t
    from types import SimpleNamespace
    g = t.check_row(tw, oracle, cus, ROW)
    p2 = t._policy(tw, *t._row_policy(oracle, ROW))
    p1 = t._policy(tw, *t._row_policy(oracle, ROW, seed=P1_SEED))
    checked = {name: (str(a.dtype), a.shape, a.tobytes()) for name, a in g.to_numpy().items()}
    r2 = raw_collect(tw, p2)
    s2 = r2.snap()
    assert s2 == checked, "the raw call does not return what the checked collect returned"
    tensors = pack_tensors(r2.dev.n)
    raw_pack(r2, tensors)
    torch.cuda.synchronize()
    a = r2.data.to_numpy()
    onehot, logp, acts, perms, advs = [x.cpu().numpy() for x in tensors]
    assert onehot.dtype == np.float32 and np.array_equal(onehot, ref64.onehot_ref(a["obs"], OBS_SIZE))
    want = ref64.log_prob_f64(a["logits"], a["actions"])
    assert np.all(np.abs(logp.astype(np.float64) - want) <= ref64.log_prob_bound(4, want))
    assert np.array_equal(acts, a["actions"].astype(np.int64)) and np.array_equal(perms, a["perms"].astype(np.int64))
    assert np.array_equal(f32_bits(advs), f32_bits(a["advs"]))
    packed = tensor_bytes(tensors)
    r2.free()
    r1 = raw_collect(tw, p1)
    s1 = r1.snap()
    r1.free()
    assert s1["logits"] != s2["logits"]
    return SimpleNamespace(p1=p1, p2=p2, s1=s1, s2=s2, packed=packed, n=len(a["actions"]))


def _free_elsewhere(tw, ref, producer_stream, free_side):
    """The producer collects P2 on its stream, parks a delay there and queues the pack behind it; free_side(body) then runs body -- the
    free, and two collects of P1 under fills -- on another thread or on another stream."""
    import torch
    _lib.release_cached_memory()                          # the pool is empty: the freed arena is the only one the next collect can get
    tensors = pack_tensors(ref.n)
    state = {}

    def produce():
        with _lib.library_stream(producer_stream):
            r = raw_collect(tw, ref.p2)
            assert r.snap() == ref.s2
            state["r"], state["base"] = r, r.base()
            state["m"] = su.delay(producer_stream, PARK_MS)
            refill(tensors, producer_stream)              # (behind the delay, in front of the pack: a pack that left the stream would be overwritten)
            raw_pack(r, tensors)
        assert not state["m"].query(), "the pack was not pending behind the delay when the producer handed the result over"

    def consume():
        r, m = state["r"], state["m"]
        assert not m.query(), "proves nothing: the delay in front of the pack had ended before the result was freed"
        r.free()
        for pattern in (0x00000000, 0x00000001):
            with _lib.debug_fill_memory(pattern):
                b = raw_collect(tw, ref.p1)
            assert b.base() == state["base"], f"proves nothing: the collect after the free did not get the freed arena ({b.base():#x}, {state['base']:#x})"
            assert b.snap() == ref.s1, f"the collect into the freed arena, fill {pattern:#010x}"
            b.free()
    free_side(produce, consume)
    torch.cuda.synchronize()
    got = tensor_bytes(tensors)
    for i, (x, y) in enumerate(zip(got, ref.packed)):
        assert x == y, f"tensor {i} of the pack that was pending when its result was freed differs from the same pack done without a delay"


def test_free_from_another_thread(tw, ref):
    S = su.independent_stream()

    def two_threads(produce, consume):
        run_threads(produce)                              # thread A: sets S, collects, parks the delay, queues the pack, exits
        run_threads(consume)                              # thread B: never called tw_set_stream
    _free_elsewhere(tw, ref, S, two_threads)


def test_free_on_another_stream_of_the_same_thread(tw, ref):
    S1 = su.independent_stream()
    S2 = su.independent_stream(others=(S1,))

    def one_thread(produce, consume):
        produce()
        with _lib.library_stream(S2):
            consume()
    _free_elsewhere(tw, ref, S1, one_thread)


def _free_under_the_freers_own_pack(tw, ref, in_thread):
    """The other half of the fence: the result is produced on S1; the consumer, whose stream is S2, queues the pack on S2 behind a
    delay and frees the result on S2.  The next collects, on S1, take the same arena: they must wait for S2's pack."""
    import torch
    S1 = su.independent_stream()
    S2 = su.independent_stream(others=(S1,))
    _lib.release_cached_memory()
    tensors = pack_tensors(ref.n)
    with _lib.library_stream(S1):
        r = raw_collect(tw, ref.p2)
        assert r.snap() == ref.s2
    base, state = r.base(), {}

    def consumer():
        with _lib.library_stream(S2):
            state["m"] = su.delay(S2, PARK_MS)
            refill(tensors, S2)
            raw_pack(r, tensors)
            r.free()
        assert not state["m"].query(), "proves nothing: the delay in front of the pack had ended before the result was freed"
    if in_thread:
        run_threads(consumer)
    else:
        consumer()
    with _lib.library_stream(S1):
        for pattern in (0x00000000, 0x00000001):
            with _lib.debug_fill_memory(pattern):
                b = raw_collect(tw, ref.p1)
            assert b.base() == base, f"proves nothing: the collect after the free did not get the freed arena ({b.base():#x}, {base:#x})"
            assert b.snap() == ref.s1, f"the collect into the freed arena, fill {pattern:#010x}"
            b.free()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(tensor_bytes(tensors), ref.packed)):
        assert x == y, f"tensor {i} of the pack the freeing stream still had pending differs from the same pack done without a delay"


@pytest.mark.parametrize("in_thread", [True, False], ids=["freed by another thread", "freed by the same thread"])
def test_free_under_a_pack_pending_on_the_freeing_stream(tw, ref, in_thread):
    _free_under_the_freers_own_pack(tw, ref, in_thread)


def test_collects_of_two_threads_are_serialised(tw, ref):
    from tests import test_gpu_device_env_matrix as dm
    r, env, gp, _ = dm._setup("probe_o4a2")
    denv = lambda: {name: (str(a.dtype), a.shape, a.tobytes()) for name, a in dm._collect(tw, r, env, gp, 40).to_numpy().items()}
    want_denv = denv()
    assert want_denv == denv()
    S1 = su.independent_stream()
    S2 = su.independent_stream(others=(S1,))
    barrier = threading.Barrier(2)
    got = {"puzzle": [], "denv": []}

    def puzzle():
        with _lib.library_stream(S1):
            barrier.wait(JOIN_S)
            for _ in range(3):
                res = raw_collect(tw, ref.p2)
                got["puzzle"].append(res.snap())
                res.free()

    def device_env():
        with _lib.library_stream(S2):
            barrier.wait(JOIN_S)
            for _ in range(3):
                got["denv"].append(denv())
    run_threads(puzzle, device_env)
    assert len(got["puzzle"]) == 3 and len(got["denv"]) == 3
    for i in range(3):
        assert got["puzzle"][i] == ref.s2, f"Puzzle collect {i} beside a device-environment collect on another thread"
        assert got["denv"][i] == want_denv, f"device-environment collect {i} beside a Puzzle collect on another thread"


def test_the_stream_is_thread_local(tw, ref):
    S = su.independent_stream()
    parked, b_done = threading.Event(), threading.Event()
    state = {}

    def thread_a():
        _lib.check(_lib.lib().tw_set_stream(C.c_void_p(S.cuda_stream)))      # (and never puts the null stream back: the thread ends with S set)
        state["m"] = su.delay(S, PARK_MS)
        parked.set()
        assert b_done.wait(JOIN_S)
        res = raw_collect(tw, ref.p2)                                          # on S: behind the delay
        assert state["m"].query(), "thread A's collect returned with the delay on its own stream still running: it did not run on that stream"
        assert res.snap() == ref.s2
        res.free()

    def thread_b():
        try:
            assert parked.wait(JOIN_S)
            res = raw_collect(tw, ref.p2)
            assert not state["m"].query(), "thread B's collect waited for the stream thread A had set (or the delay was too short to tell)"
            assert res.snap() == ref.s2
            res.free()
        finally:
            b_done.set()
    run_threads(thread_a, thread_b)
    # A has exited with S set; the main thread never set a stream
    m = su.delay(S, PARK_MS)
    res = raw_collect(tw, ref.p2)
    assert not m.query(), "the main thread's collect waited for the stream a thread that has ended had set"
    assert res.snap() == ref.s2
    res.free()
    m.synchronize()


@pytest.mark.parametrize("ids", ["one-byte ids", "two-byte ids"])
def test_the_pack_runs_behind_what_the_caller_queued_on_its_stream(tw, oracle, ref, ids):
    """The hand-off enqueues on the caller's stream and does not wait: behind a delay and a refill of the destination tensors that the
    caller queued there, every kernel and memset of it (the one-hot of one-byte ids; the memset and the scatter of two-byte ids; the
    pack) must still come last.  The reference is the same pack on the null stream, its one-hot held to tests/ref64.py."""
    import torch
    if ids == "one-byte ids":
        collect, obs_size = (lambda: raw_collect(tw, ref.p2)), 256
    else:
        from tests import test_gpu_var_obs as t
        from tests.var_obs_util import E, GAMMA, LAM, SEED, lamps, lamps_policy_arrays
        env, pol, obs_size = lamps(12), t._policies(oracle, 12)[0], int(lamps_policy_arrays(12)[0].shape[0])

        def collect():
            data = tw.collector.PPOCollector(E, GAMMA, LAM, 4).collect(env, pol, seed=SEED)
            r = Result.__new__(Result)
            r.dev, r.data = data._dev, data
            return r
    S = su.independent_stream()

    def pack(r, tensors):
        p = [C.c_void_p(x.data_ptr()) for x in tensors]
        _lib.check(_lib.lib().tw_collected_pack_trainer(r.h, obs_size, 0, 0, r.dev.n, *p))
    r0 = collect()
    assert r0.dev.obs_width == (1 if ids == "one-byte ids" else 2)
    n = r0.dev.n
    make = lambda: tuple(torch.empty(shape, dtype=dt, device="cuda") for shape, dt in
                         (((n, obs_size), torch.float32), ((n,), torch.float32), ((n,), torch.int64), ((n,), torch.int64), ((n,), torch.float32)))
    want_t = make()
    refill(want_t, su.null_stream())
    pack(r0, want_t)
    torch.cuda.synchronize()
    a = r0.data.to_numpy()
    ids_of = a["obs"].astype(np.int64)
    rows, slots = np.nonzero(ids_of != 0xFFFF if r0.dev.obs_width == 2 else np.ones_like(ids_of, bool))      # (0xFFFF: a free slot of a shorter observation)
    onehot = np.zeros((n, obs_size), np.float32)
    onehot[rows, ids_of[rows, slots]] = 1.0
    if r0.dev.obs_width == 1:
        assert np.array_equal(onehot, ref64.onehot_ref(a["obs"], obs_size))
    else:
        assert (ids_of == 0xFFFF).any() and rows.size                     # (free slots and ids: both branches of the scatter)
    assert np.array_equal(want_t[0].cpu().numpy(), onehot)
    assert np.array_equal(want_t[2].cpu().numpy(), a["actions"].astype(np.int64))
    want = tensor_bytes(want_t)
    with _lib.library_stream(S):
        r = collect()
        got_t = make()
        torch.cuda.synchronize()
        m = su.delay(S, PARK_MS)
        refill(got_t, S)
        pack(r, got_t)
        assert not m.query(), "the hand-off waited for the caller's stream (or the delay was too short to tell)"
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(tensor_bytes(got_t), want)):
        assert x == y, f"{ids}: tensor {i} of a pack queued behind a delay and a refill on the caller's stream differs from the null-stream pack"


def test_release_cached_memory_with_a_live_result_made_on_a_stream(tw, ref):
    S = su.independent_stream()
    with _lib.library_stream(S):
        live = raw_collect(tw, ref.p2)
        assert live.snap() == ref.s2
        _lib.release_cached_memory()
        assert live.snap() == ref.s2, "tw_release_cached_memory changed a live result"
        with _lib.debug_fill_memory(0x00000001):
            nxt = raw_collect(tw, ref.p1)
        assert nxt.snap() == ref.s1 and live.snap() == ref.s2
        assert nxt.base() != live.base()
        nxt.free()
        live.free()
