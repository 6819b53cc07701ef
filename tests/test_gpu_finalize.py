"""GPU: the tail of every device collector, kernel by kernel -- the three-launch episode-length scan, finalize_ppo_group_kernel<16> / <8>,
finalize_ppo_kernel, finalize_az_kernel, compact_obs16_kernel, compact_env_obs8_kernel and narrow_logits_kernel -- on records the
test wrote (`tw_debug_collect_tail`: the production `launch_scan` and `collect_tail`, nothing re-implemented), at every row of
tests/finalize_matrix.py and in both merge orders.

Every test first holds the finalize kernel the tail reports (form, waves, grid, LDS) against the restated launch rules, then
compares EVERY compact field with the plain numpy reference as bits: obs, logits or probabilities, perms, values, rewards, actions,
ep_len, ep_start; advs, rets and remaining as bits wherever the reference is no NaN and as "a NaN" where it is one (sign and payload
of a generated NaN differ between x86 and the GPU -- the only relaxation in this file; the normal-valued rows hold no NaN at all).
Padding records are poison (signalling NaNs, 0xFF), the result's arena is pre-filled with a byte, and every byte of it outside the
fields must still be that byte afterwards: a row read or written one too far shows in a field or in a gap.  Nothing is sampled.
"""
import ctypes as C

import numpy as np
import pytest

from tests import finalize_matrix as fm
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

FIELDS = {"obs": _lib.TW_F_OBS, "logits": _lib.TW_F_LOGITS, "perms": _lib.TW_F_PERMS, "values": _lib.TW_F_VALUES, "rewards": _lib.TW_F_REWARDS,
          "actions": _lib.TW_F_ACTIONS, "advs": _lib.TW_F_ADVS, "rets": _lib.TW_F_RETS, "remaining": _lib.TW_F_REMAINING,
          "ep_len": _lib.TW_F_EP_LEN, "ep_start": _lib.TW_F_EP_START}
MIN_NORMAL = np.float32(1.1754944e-38)


@pytest.fixture(scope="module", autouse=True)
def device():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    yield
    _lib.release_cached_memory()             # (the largest rows leave a 270 MB workspace and arenas of that order in the pool)


def _call(case, L, rec, o16, wide, merge_order):
    """One call of the hook -> (launch, {field: bytes of the result}, the arena's bytes outside every field)."""
    handle, launch = _lib.debug_collect_tail(L, rec, case.t_pad, is_ppo=case.kind == "ppo", n_cells=case.n_cells, n_actions=case.A, obs16=o16,
                                             obs_width=case.ids or 1, wide=wide, gamma=case.gamma, lam=case.lam, merge_order=merge_order,
                                             arena_fill=fm.FILL)
    try:
        lib = _lib.lib()
        assert lib.tw_collected_num_records(handle) == int(L.sum(dtype=np.uint64)) and lib.tw_collected_num_episodes(handle) == case.E
        assert lib.tw_collected_is_ppo(handle) == int(case.kind == "ppo") and lib.tw_collected_obs_width(handle) == (case.ids or 1)
        arena, offs, scratch = _lib.debug_collected_arena(handle)
        outside = np.ones(arena.size, dtype=bool)
        got = {}
        for name, f in FIELDS.items():
            n = C.c_size_t()
            ptr = lib.tw_collected_device_ptr(handle, f, C.byref(n))
            if n.value:
                assert ptr and offs[f] % 256 == 0 and offs[f] + n.value <= arena.size, name
                assert outside[offs[f]:offs[f] + n.value].all(), f"{name} overlaps another field"
                got[name] = arena[offs[f]:offs[f] + n.value]
                outside[offs[f]:offs[f] + n.value] = False
        assert (scratch[1] != 0) == (case.A != 4) and scratch[0] + scratch[1] <= arena.size
        assert outside[scratch[0]:scratch[0] + scratch[1]].all()
        outside[scratch[0]:scratch[0] + scratch[1]] = False
        return launch, got, arena[outside]
    finally:
        _lib.lib().tw_collected_free(handle)


def _check(case, L=None):
    L = fm.episode_lengths(case.E, case.t_pad) if L is None else L
    rec, o16, wide = fm.make_inputs(case, L)
    want_launch = fm.case_dispatch(case)
    for merge_order in (False, True):
        what = f"{fm.case_id(case)}, merge order {int(merge_order)}"
        ref = fm.reference(case, L, rec, o16, wide, merge_order)
        if case.values == "normal":                          # no NaN anywhere: the relaxation below is never used
            for name in ("logits", "values", "rewards"):
                if name in ref:
                    assert not np.isnan(ref[name].view(np.float32)).any(), (what, name)
            for name in fm.COMPUTED:
                if name in ref:
                    assert np.isfinite(ref[name]).all(), (what, name)
        launch, got, outside = _call(case, L, rec, o16, wide, merge_order)
        assert launch == want_launch, f"{what}: launched {launch}, the restated rules say {want_launch}"
        assert sorted(got) == sorted(ref), f"{what}: fields {sorted(got)}"
        for name, want in ref.items():
            g = got[name]
            assert g.size == want.nbytes, f"{what}: {name} holds {g.size} bytes, the reference {want.nbytes}"
            if name in fm.COMPUTED:
                bad = fm.same_or_nan(g.view(np.float32), want)
                assert bad.size == 0, (f"{what}: {name}: {bad.size} of {want.size} records differ, the first at {int(bad[0])}: "
                                       f"{g.view(np.uint32)[bad[0]]:#010x}, the reference has {want.view(np.uint32)[bad[0]]:#010x}")
            else:
                bad = np.flatnonzero(g != want.reshape(-1).view(np.uint8))
                assert bad.size == 0, (f"{what}: {name}: {bad.size} bytes differ, the first at byte {int(bad[0])} "
                                       f"(row {int(bad[0]) // max(want.nbytes // max(len(want), 1), 1)}): {g[bad[0]]:#04x}, the reference has "
                                       f"{want.reshape(-1).view(np.uint8)[bad[0]]:#04x}")
        touched = np.flatnonzero(outside != fm.FILL)
        assert touched.size == 0, f"{what}: {touched.size} bytes outside the fields were written, the first is outside byte {int(touched[0])}"
    return ref


# ------------------------------------------------------------------------------------------ forms, edges, columns, horizons
@pytest.mark.parametrize("case", fm.FORMS, ids=fm.case_id)
def test_every_form_on_both_sides_of_every_switch(case):
    _check(case)


@pytest.mark.parametrize("case", fm.GROUP_EDGES, ids=fm.case_id)
def test_episode_counts_around_a_workgroup_of_the_grouped_forms(case):
    _check(case)


@pytest.mark.parametrize("case", fm.COLUMNS, ids=fm.case_id)
def test_columns_narrowed_kept_and_moved_from_the_wide_array(case):
    ref = _check(case)
    assert ref["logits"].shape[1] == case.A
    if case.kind == "az":
        assert (ref["perms"] == 0xFF).all()                  # -1 everywhere (az.rs:95)


@pytest.mark.parametrize("case", fm.AZ_HORIZONS, ids=fm.case_id)
def test_az_horizons(case):
    ref = _check(case)
    assert (ref["perms"] == 0xFF).all()


@pytest.mark.parametrize("case", fm.SECOND_TRIPS, ids=fm.case_id)
def test_second_trip_of_every_grid_stride_loop(case):
    assert fm.finalize_trips(case) >= 2 or fm.mover_trips(case.E) >= 2
    _check(case)


# ------------------------------------------------------------------------------------------ refusals
def _raw(args):
    launch, handle = _lib.FinalizeLaunch(), C.c_void_p()
    rc = _lib.lib().tw_debug_collect_tail(C.byref(args), C.byref(launch), C.byref(handle))
    return rc, launch, handle


def _args(case, L, rec, o16_arr=None, wide_arr=None, **over):
    keep = [np.ascontiguousarray(L, dtype=np.uint32), np.ascontiguousarray(rec)]
    a = _lib.DebugTailArgs(n_episodes=case.E, t_pad=case.t_pad, is_ppo=int(case.kind == "ppo"), n_cells=case.n_cells, n_actions=case.A,
                           obs_width=case.ids or 1, merge_order=0, scan_only=0, arena_fill=fm.FILL, gamma=case.gamma, lambda_=case.lam,
                           ep_len=keep[0].ctypes.data, records=keep[1].ctypes.data, obs16=None if o16_arr is None else o16_arr.ctypes.data,
                           wide=None if wide_arr is None else wide_arr.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a, keep


@pytest.mark.parametrize("case", fm.REFUSED, ids=fm.case_id)
def test_a_horizon_beyond_the_forms_is_refused_and_leaves_nothing_behind(case):
    assert fm.case_dispatch(case) is None
    L = fm.episode_lengths(case.E, case.t_pad)
    rec, o16, wide = fm.make_inputs(case, L)
    a, keep = _args(case, L, rec, o16, wide)
    rc, launch, handle = _raw(a)
    assert rc == _lib.TW_ERR_UNSUPPORTED and handle.value is None and launch.form == _lib.TW_FIN_NONE and launch.blocks == 0
    assert "too large for the LDS tile" in _lib.last_error()
    _check(case._replace(t_pad=case.t_pad - 1))              # and the library goes on as before


def test_arguments_a_kernel_would_fault_on_are_refused_on_the_host():
    case = fm._ppo(5, 9, n_cells=9)
    L = fm.episode_lengths(5, 9)
    rec, _, _ = fm.make_inputs(case, L)
    o16, wide = np.zeros((45, 64), np.uint16), np.zeros((45, 31), np.float32)
    zero, over = L.copy(), L.copy()
    zero[3], over[4] = 0, 10
    bad = [dict(n_episodes=0), dict(ep_len=zero.ctypes.data), dict(ep_len=over.ctypes.data), dict(n_cells=0), dict(n_cells=17), dict(n_actions=0),
           dict(n_actions=32), dict(n_actions=5), dict(wide=wide.ctypes.data), dict(t_pad=0), dict(arena_fill=256), dict(records=None), dict(ep_len=None),
           dict(obs16=o16.ctypes.data, n_cells=65), dict(obs16=o16.ctypes.data, n_cells=0), dict(obs16=o16.ctypes.data, n_cells=25, obs_width=3),
           dict(obs16=o16.ctypes.data, n_cells=25, obs_width=0)]
    for kw in bad:
        a, keep = _args(case, L, rec, **kw)
        rc, launch, handle = _raw(a)
        assert rc == _lib.TW_ERR_INVALID and handle.value is None and launch.form == _lib.TW_FIN_NONE and _lib.last_error(), kw
    a, keep = _args(case, L, rec, scan_only=1)               # scan-only mode without its outputs
    assert _raw(a)[0] == _lib.TW_ERR_INVALID
    _check(case)


# ------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize("E", fm.SCAN_E)
def test_scan_offsets_and_total_are_exact(E):
    L = (fm.mix32(np.arange(E, dtype=np.uint32), 3) % np.uint32(1000) + 1).astype(np.uint32)
    for merge_order in (False, True):
        got, total = _lib.debug_scan(L, merge_order)
        want, want_total = fm.ep_start_ref(L, merge_order)
        assert total == want_total and got.dtype == np.uint64
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"E {E}, merge order {int(merge_order)}: {bad.size} offsets differ, the first at episode {int(bad[0])}: {int(got[bad[0]])} / {int(want[bad[0]])}"


def test_scan_with_tile_sums_carry_and_total_beyond_32_bits():
    E = 263171                                               # 258 tiles: a second trip of the carry loop
    L = (np.uint32(0xFFFFFFFF) - fm.mix32(np.arange(E, dtype=np.uint32), 4) % np.uint32(1000)).astype(np.uint32)
    L[::97] = 0
    L[5], L[E - 1] = 0xFFFFFFFF, 0xFFFFFFFF
    for merge_order in (False, True):
        got, total = _lib.debug_scan(L, merge_order)
        want, want_total = fm.ep_start_ref(L, merge_order)
        assert int(L[:1024].sum(dtype=np.uint64)) > 1 << 32 and int(want[256 * 1024]) > 1 << 32 and want_total > 1 << 49
        assert total == want_total and np.array_equal(got, want), f"merge order {int(merge_order)}"


@pytest.mark.parametrize("case", fm.SCAN_WITH_RECORDS, ids=fm.case_id)
def test_records_placed_by_a_scan_that_uses_its_carry(case):
    assert fm.scan_carry_trips(case.E) == 2
    _check(case)


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("case", fm.VALUES, ids=fm.case_id)
def test_signed_zeros_denormals_overflow_and_nan_bit_patterns(case):
    L = fm.episode_lengths(case.E, case.t_pad)
    rec, o16, wide = fm.make_inputs(case, L)
    # before the GPU is compared: the reference itself keeps denormals (a host that flushes them would hide a kernel that does), turns
    # the large episodes into infinities and NaNs, and the copied fields hold signalling and payload NaNs
    ref = fm.reference(case, L, rec, o16, wide, False)
    start = np.concatenate([[0], np.cumsum(L.astype(np.int64))])
    comp = ref["advs"] if case.kind == "ppo" else ref["remaining"]
    cls = lambda k: np.concatenate([np.arange(start[e], start[e + 1]) for e in range(case.E) if e % 5 == k])
    den = comp[cls(1)]
    assert ((den != 0) & (np.abs(den) < MIN_NORMAL)).any(), "the reference shows no denormal"
    z = comp[cls(0)].view(np.uint32)
    assert ((z == 0) | (z == 0x80000000)).all()
    if case.kind == "ppo":
        assert (ref["rewards"][cls(0)] == 0x80000000).all() and (ref["values"][cls(0)] == 0x80000000).all()
        bits = np.concatenate([ref["logits"].reshape(-1), ref["values"], ref["rewards"]])
        assert {0x7F800001, 0xFFC12345, 0x7FA00000, 0xFFFFFFFF} <= set(bits[np.isnan(bits.view(np.float32))].tolist())
    else:
        assert {0x7F800001, 0xFFC12345} <= set(ref["logits"].reshape(-1).tolist())
    assert np.isinf(comp[cls(2)]).any() and np.isnan(comp[cls(3)]).any() and not np.isnan(comp[cls(4)]).any()
    _check(case, L)
