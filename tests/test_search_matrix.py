"""CPU: tests/search_matrix.py's table has exactly one row per self-play / evaluate / solve / big-board kernel the build ships, its
restatement of the launch rules agrees with the launch shapes other tests assert on the GPU, and a census of the whole build: every
kernel in the built assembly belongs to one of the two tables (tests/kernel_matrix.py, tests/search_matrix.py) or to the short list
of non-templated kernels below, each with the GPU test that launches it.

The kernels are read from the device assembly the build keeps (lib/asm/*.s: one `.amdhsa_kernel` directive per kernel, the text
test_mfma_hazards.py scans).  A new instantiation without a row, a row whose restated dispatch lands on a kernel that is not built,
or a new kernel that is in no table and not in the list fails here by name.
"""
import collections
import glob
import os
import re

import pytest

from tests import kernel_matrix as km
from tests import search_matrix as sm
from tests.test_kernel_matrix import F16, F32, _num

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MCTS = re.compile(r"^_ZN2tw15mcts_f32_kernelILi(\d+)ELi(\d+)ELi(n?\d+)ELb([01])EEEvNS_8MctsArgsE$")
SOLVE = re.compile(r"^_ZN2tw16solve_f32_kernelILi(\d+)ELi(\d+)ELi(n?\d+)EEEvNS_9SolveArgsE$")
DEEP = re.compile(r"^_ZN2tw16mcts_deep_kernelILi(\d+)ELi(\d+)ELi(n?\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])EEEvNS_8MctsArgsE$")
ENGINE = re.compile(r"^_ZN2tw18mcts_engine_kernelILi(\d+)ELi(\d+)EEEvNS_8MctsArgsE$")
BIG = re.compile(r"^_ZN2tw\d+(mcts_big|solve_big|rollout_big)_kernelILi(\d+)EEEvNS_")

FAMILY_COUNTS = {"mcts_f32_kernel": 54, "solve_f32_kernel": 36, "mcts_deep_kernel": 96, "mcts_engine_kernel": 6, "mcts_big_kernel": 3,
                 "solve_big_kernel": 3, "rollout_big_kernel": 3}
ROLLOUT_COUNTS = {"rollout_f32_kernel": 57, "rollout_f16_kernel": 48}
TOTAL_KERNELS = 331

# The kernels that are no template family: name (with its integer template arguments, if any) -> (source file, GPU test file, test that launches it)
OTHER = {
    "scan_tile_sums": ("tw_finalize", "test_gpu_finalize.py", "test_scan_offsets_and_total_are_exact"),
    "scan_tile_offsets": ("tw_finalize", "test_gpu_finalize.py", "test_scan_offsets_and_total_are_exact"),
    "scan_write": ("tw_finalize", "test_gpu_finalize.py", "test_scan_offsets_and_total_are_exact"),
    "finalize_ppo_kernel": ("tw_finalize", "test_gpu_finalize.py", "test_every_form_on_both_sides_of_every_switch"),
    "finalize_ppo_group_kernel<16>": ("tw_finalize", "test_gpu_finalize.py", "test_every_form_on_both_sides_of_every_switch"),
    "finalize_ppo_group_kernel<8>": ("tw_finalize", "test_gpu_finalize.py", "test_every_form_on_both_sides_of_every_switch"),
    "finalize_az_kernel": ("tw_mcts", "test_gpu_finalize.py", "test_az_horizons"),
    "split_gate_kernel": ("tw_mcts_deep", "test_gpu_parity.py", "test_split_walker_shape_bit_exact_vs_oracle"),
    "init_boards_kernel": ("tw_rollout", "test_gpu_parity.py", "test_persistent_lane_mode_bit_exact"),
    "episode_order_count_kernel": ("tw_rollout", "test_gpu_parity.py", "test_episode_order_is_a_stable_sort_by_manhattan_distance"),
    "episode_order_prefix_kernel": ("tw_rollout", "test_gpu_parity.py", "test_episode_order_is_a_stable_sort_by_manhattan_distance"),
    "episode_order_scatter_kernel": ("tw_rollout", "test_gpu_parity.py", "test_episode_order_is_a_stable_sort_by_manhattan_distance"),
    "compact_obs16_kernel": ("tw_rollout_big", "test_gpu_finalize.py", "test_every_form_on_both_sides_of_every_switch"),
    "policy_eval_kernel": ("tw_eval", "test_gpu_parity.py", "test_policy_evaluate_matches_oracle"),
    "policy_eval_generic_kernel": ("tw_eval", "test_gpu_parity.py", "test_policies_of_any_depth"),
    "policy_sync_kernel": ("tw_sync", "test_gpu_policy_sync.py", "test_synced_image_equals_the_host_built_image"),
    "policy_sync_generic_kernel": ("tw_sync", "test_gpu_policy_sync.py", "test_synced_image_equals_the_host_built_image"),
    "onehot_kernel": ("tw_trainer", "test_gpu_parity.py", "test_trainer_handoff_matches_reference_formulas"),
    "onehot_scatter_kernel": ("tw_trainer", "test_gpu_trainer_handoff.py", "test_one_hot_of_ids_that_follow_no_layout"),
    "onehot4_kernel<8>": ("tw_trainer", "test_gpu_parity.py", "test_trainer_one_hot_of_boards_whose_cells_own_multiples_of_four_ids"),
    "ppo_pack_kernel": ("tw_trainer", "test_gpu_parity.py", "test_trainer_handoff_matches_reference_formulas"),
    "sum_kernel": ("tw_trainer", "test_gpu_parity.py", "test_trainer_handoff_matches_reference_formulas"),
    "sum_partials_kernel": ("tw_trainer", "test_gpu_parity.py", "test_trainer_handoff_matches_reference_formulas"),
    "compact_env_obs8_kernel": ("tw_device_env", "test_gpu_finalize.py", "test_every_form_on_both_sides_of_every_switch"),
    "narrow_logits_kernel": ("tw_device_env", "test_gpu_finalize.py", "test_columns_narrowed_kept_and_moved_from_the_wide_array"),
}


def built_kernel_symbols():
    """{assembly file stem: [kernel symbols]} of the whole build."""
    from twisterl_amd import build as tb
    if not all(os.path.exists(os.path.join(tb.ASM_DIR, s.replace(".hip", ".s"))) for s in tb.SOURCES):
        tb.build_library()
    out = {}
    for p in sorted(glob.glob(os.path.join(tb.ASM_DIR, "*.s"))):
        syms = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in open(p)) if m]
        out[os.path.basename(p)[:-2]] = syms
    return out


def search_kernel(sym):
    """A kernel symbol of the five families -> its search_matrix kernel tuple (None: not one of them)."""
    m = MCTS.match(sym)
    if m:
        return ("mcts", int(m.group(1)), int(m.group(2)), _num(m.group(3)), m.group(4) == "1")
    m = SOLVE.match(sym)
    if m:
        return ("solve", int(m.group(1)), int(m.group(2)), _num(m.group(3)))
    m = DEEP.match(sym)
    if m:
        return ("deep", int(m.group(1)), int(m.group(2)), _num(m.group(3)), int(m.group(4)), m.group(5) == "1", m.group(6) == "1", m.group(7) == "1")
    m = ENGINE.match(sym)
    if m:
        return ("engine", int(m.group(1)), int(m.group(2)))
    m = BIG.match(sym)
    if m:
        return (m.group(1), int(m.group(2)))
    return None


def plain_name(sym):
    """`_ZN2tw25finalize_ppo_group_kernelILi16EEEv...` -> `finalize_ppo_group_kernel<16>` (the last identifier of the nested name and
    its integer template arguments)."""
    assert sym.startswith("_ZN"), sym
    i, name = 3, None
    while sym[i].isdigit():
        j = i
        while sym[j].isdigit():
            j += 1
        n = int(sym[i:j])
        name, i = sym[j:j + n], j + n
    if sym[i] == "I":
        args = re.match(r"I((?:Li?n?\d+E)+)E", sym[i:])
        assert args, sym
        name += "<" + ", ".join(str(_num(a)) for a in re.findall(r"Li(n?\d+)E", args.group(1))) + ">"
    return name


def built_search_kernels():
    names = []
    for syms in built_kernel_symbols().values():
        for s in syms:
            k = search_kernel(s)
            if k is not None:
                names.append(sm.kernel_name(k))
            else:
                assert not re.search(r"mcts_f32|solve_f32|mcts_deep|mcts_engine|_big_kernel", s) or "compact" in s, f"a kernel of a form the table does not know: {s}"
    return names


def _covered(table, cus):
    return collections.Counter(sm.kernel_name(k) for k in (sm.covered_kernel(r, cus) for r in table) if k is not None)


def test_built_kernels_are_the_known_families():
    names = built_search_kernels()
    assert len(names) == len(set(names))
    assert collections.Counter(n.split("<")[0] for n in names) == FAMILY_COUNTS
    deep = [n for n in names if n.startswith("mcts_deep_kernel")]
    # the solve-mode engine (NW = -17) exists in solve mode only, the split shape with twelve or sixteen walkers only
    assert all(("-17" in n) == (", true, false, false>" in n) for n in deep)
    assert sorted(n.split(", ")[3] for n in deep if n.endswith("true, true>")) == ["12"] * 6 + ["16"] * 6


@pytest.mark.parametrize("cus", [256, 304])
def test_table_covers_every_built_search_kernel_once(cus):
    built = set(built_search_kernels())
    got = _covered(sm.TABLE, cus)
    missing = sorted(built - set(got))
    assert not missing, f"kernels without a row in tests/search_matrix.py: {missing}"
    launched = {sm.kernel_name(sm.dispatch(r, cus)[0]) for r in sm.TABLE} | set(got)
    unknown = sorted(launched - built)
    assert not unknown, f"rows whose restated dispatch names a kernel the build does not have: {unknown}"
    twice = sorted(k for k, n in got.items() if n > 1)
    assert not twice, f"instantiations with more than one row: {twice}"
    assert sum(r.covers != "extra" for r in sm.TABLE) == len(built) == sum(FAMILY_COUNTS.values())
    # the rows' comments name the kernel they stand for
    text = open(os.path.join(ROOT, "tests", "search_matrix.py")).read()
    comments = re.findall(r"^    (?:AZ|EV|SV|PPO)\(.*\),\s+# (\S.*)$", text, flags=re.M)
    assert comments == [sm.kernel_name(sm.covered_kernel(r, cus) or sm.dispatch(r, cus)[0]) for r in sm.TABLE]


def test_deleting_any_row_names_the_kernel_it_covered():
    built = set(built_search_kernels())
    for i, row in enumerate(sm.TABLE):
        rest = sm.TABLE[:i] + sm.TABLE[i + 1:]
        missing = built - set(_covered(rest, 256))
        want = set() if row.covers == "extra" else {sm.kernel_name(sm.covered_kernel(row, 256))}
        assert missing == want, (i, row)


def test_rows_are_shapes_the_library_takes_and_cheap_enough_for_the_oracle():
    ids = [sm.row_id(r) for r in sm.TABLE]
    assert len(set(ids)) == len(ids)
    for r in sm.TABLE:
        cells = r.w * r.h
        assert 1 <= cells <= 64 and r.prec == "fp32" and not r.no_persist, r
        assert not r.twists or r.w == r.h, r                     # the transpose twist needs a square board
        assert (r.common is None) == (r.hidden in (32, 64, 128, 256)), r
        assert cells <= 16 or r.common is not None, r            # boards above 16 cells: generic policies
        assert r.emb % 32 == 0 and 32 <= r.emb <= 128, r
        assert r.force_geom in (0, 8, 32) and r.reserve in (None, sm.AB1, sm.AB16) and 0 <= r.diff <= 10 and r.med in (1, 2), r
        assert r.entry in ("az", "evaluate", "solve", "ppo") and r.covers in ("main", "engine", "extra"), r
        # the oracle's cost: policy evaluations ~ episodes (attempts) x moves (at most 2 x difficulty + 1) x (searches + 1)
        moves = 2 * r.diff + 1
        if r.entry == "az":
            assert r.E <= sm.MAX_EPISODES and r.E * moves * (r.S + 1) <= 3_000_000, r
        elif r.entry in ("evaluate", "solve"):
            assert r.ns >= 1 and (r.entry == "evaluate" or r.E == 1), r
            assert sm.attempts(r) <= sm.MAX_ATTEMPTS and sm.attempts(r) * moves * (r.S + 1) <= 3_000_000, r
            assert not r.force_geom and not r.reserve, r         # tw_evaluate / tw_solve take no reserve_cus
        else:
            assert cells > 16 and r.E <= 1000, r
        # a diagnostic option only where the section comments say no plain call reaches the kernel
        k = sm.dispatch(r, 256)[0]
        if r.force_geom == 8:
            assert k[0] == "mcts" and k[3] == 8 and not k[4], r
        if r.force_geom == 32 or r.variant == 32:
            assert k[0] == "deep" and k[3] == -4, r
        if r.variant == 256:
            assert k[0] == "deep" and k[3] == -16 and k[4] in (2, 4, 8) and not k[6], r
        assert r.variant in (0, 32, 256), r
        if k[0] == "mcts" and k[4]:                               # persistent rows: at least three times the resident lanes
            for cus in (256, 304):
                res = sm.reserve_cus(r, cus)
                assert r.E >= 3 * sm.f32_resident_selfplay(r.E, r.hidden, cus, res), r
    # what the rows of a family vary
    az = [r for r in sm.TABLE if r.entry == "az"]
    for fam in ("mcts", "deep"):
        rows = [r for r in az if sm.dispatch(r, 256)[0][0] == fam]
        assert {r.med for r in rows} == {1, 2} and any(r.twists for r in rows) and any(r.diff <= 1 for r in rows), fam
        assert any(r.S == 0 for r in rows) and any(r.S > 100 for r in rows), fam
    eps = {"mcts": lambda k: km.F32_BLOCK[k[3]][0], "deep": lambda k: k[4]}
    ragged = [r for r in az if r.w * r.h <= 16 and r.E % eps[sm.dispatch(r, 256)[0][0]](sm.dispatch(r, 256)[0]) != 0]
    assert len(ragged) >= 40


def test_restated_dispatch_matches_the_launch_shapes_the_suite_asserts():
    for cus in (256, 304):
        # test_walker_self_play_uses_as_few_walkers_per_workgroup_as_keep_the_chip_busy (Puzzle-8, 32 / 128)
        for E, want in ((cus // 2, (cus // 2, 256)), (cus, (cus, 256)), (2 * cus, (cus, 256)), (3 * cus, (cus, 384)), (6 * cus, (cus, 512)),
                        (13 * cus, (min(-(-13 * cus // 12), (cus - cus // 2) * 2), 768))):
            k, shape, eng = sm.dispatch(sm.AZ(3, 3, 32, 128, E, 4 if E <= 8 * cus else 24, diff=2), cus)
            assert k[0] == "deep" and shape == want, (E, k, shape)
            assert (eng is not None) == (E >= 8 * cus)
        # ... and its pinned shapes exist (TW_OPT_AZ_VARIANT 16 / 32 + 3 .. 6, + 128 / 256, 512, 1024)
        for variant in (16 + 4, 16 + 3, 16 + 5, 16 + 6, 32 + 4, 32 + 3, 32 + 5, 32 + 6, 256 + 16 + 3, 256 + 16 + 5, 256 + 16 + 6, 128 + 16 + 3, 128 + 16 + 5,
                        128 + 16 + 6, 256, 512, 1024):
            k, shape, _ = sm.dispatch(sm.AZ(3, 3, 32, 128, 3 * cus, 6, diff=2, variant=variant), cus)
            walkers = {3: 2, 4: 1, 5: 4, 6: 8}.get(variant & 7, 12 if variant == 512 else 2)
            assert k[0] == "deep" and k[4] == walkers and k[3] == (-4 if variant & 32 else -16), (variant, k)
            assert k[6] == (walkers >= 2 and not variant & 32 and not variant & 256), (variant, k)
        # test_split_walker_shape_bit_exact_vs_oracle (TW_OPT_AZ_VARIANT 512)
        for w, h, diff, emb, hidden, E, S, med, twists in ((3, 3, 3, 64, 128, 70, 24, 1, False), (3, 3, 4, 64, 128, 300, 40, 2, True),
                                                           (4, 4, 5, 128, 256, 500, 16, 1, False), (2, 2, 2, 32, 128, 40, 10, 1, False)):
            k, shape, eng = sm.dispatch(sm.AZ(w, h, emb, hidden, E, S, med=med, diff=diff, twists=twists, variant=512), cus)
            assert k[7] and shape[1] in (768, 1024) and shape[0] == -(-E // (shape[1] // 64)) and eng == (min(cus // 2, shape[0]), 256), (k, shape, eng)
        # test_split_shape_falls_back_when_its_kernels_cannot_run_side_by_side: the automatic split shape, and the decoupled shapes inside
        # one workgroup once the split shape is off (TW_OPT_AZ_VARIANT + 1024 restates what the process keeps after the fallback)
        E = 8 * cus + 100
        k, shape, eng = sm.dispatch(sm.AZ(3, 3, 64, 128, E, 16, diff=3), cus)
        assert k == ("deep", 4, 9, -16, 12, False, True, True) and shape == (min(-(-E // 12), (cus - cus // 2) * 2), 768)
        k, shape, eng = sm.dispatch(sm.AZ(3, 3, 64, 128, E, 16, diff=3, variant=1024), cus)
        assert k[6] and not k[7] and shape[1] in (512, 768) and eng is None
        # test_mid_size_batches_use_the_queue_with_the_small_batch_geometry: 9,000 self-play episodes, 128 hidden units, 6 searches
        E = 9_000 if cus == 256 else 10_000
        k, shape, _ = sm.dispatch(sm.AZ(3, 3, 64, 128, E, 6, diff=2), cus)
        assert k == ("mcts", 4, 9, -4, True) and shape == (cus, 256) and shape[0] * 32 < E
        # test_az_persistent_lane_mode_bit_exact: 66,000 episodes on 32 hidden units -> one persistent 256-lane workgroup per CU (below CUs x 256
        # episodes: plain workgroups); TW_OPT_NO_PERSIST: plain 256-episode workgroups
        row = sm.AZ(3, 3, 32, 32, 66_000, 3, diff=1)
        want = (("mcts", 1, 9, 8, True), (cus, 512), None) if cus == 256 else (("mcts", 1, 9, 8, False), (258, 512), None)
        assert sm.dispatch(row, cus) == want
        assert sm.dispatch(row._replace(no_persist=True), cus) == (("mcts", 1, 9, 8, False), (258, 512), None)
        # test_mcts_guided_evaluate_on_the_walker_kernel: one / two / four walkers per workgroup by the attempts (no reserved CUs); its last
        # case (more than 8 attempts per CU at 3 searches) is beyond the walker kernel's range: 16 attempts per workgroup of the lane kernel
        for n_ep, ns, S, nwk in ((40, 1, 5, 1), (cus + 9, 2, 4, 2), (2 * cus + 5, 3, 4, 4)):
            k, shape, _ = sm.dispatch(sm.EV(3, 3, 64, 128, n_ep, ns, S=S, diff=3, twists=True), cus)
            assert k == ("deep", 4, 9, -17, nwk, True, False, False) and shape == (min(-(-n_ep * ns // nwk), cus), 256), (n_ep, k, shape)
        k, shape, _ = sm.dispatch(sm.EV(3, 3, 64, 128, 3 * cus + 1, 5, det=True, S=3, diff=3, twists=True), cus)
        assert k == ("mcts", 4, 9, -16, False) and shape == (-(-(3 * cus + 1) * 5 // 16), 256), (k, shape)
        # test_boards_of_17_to_64_cells_roll_out_on_the_device: 16 episodes per workgroup of 256 threads
        assert sm.dispatch(sm.PPO(5, 5, 64, (128,), 65_536), cus) == (("rollout_big", 25), (4096, 256), None)
        assert sm.dispatch(sm.PPO(7, 5, 32, (64, 32), 150), cus) == (("rollout_big", 36), (10, 256), None)
        assert sm.dispatch(sm.AZ(8, 8, 32, 0, 40, 8, common=(64, 32)), cus) == (("mcts_big", 64), (3, 256), None)


def test_census_of_the_whole_build():
    """Every kernel of every object: in one of the two tables' families, or in OTHER with the test that launches it."""
    by_file = built_kernel_symbols()
    counts, seen_other = collections.Counter(), collections.Counter()
    for stem, syms in by_file.items():
        for s in syms:
            if F32.match(s) or F16.match(s):
                counts["rollout_f32_kernel" if F32.match(s) else "rollout_f16_kernel"] += 1
                continue
            k = search_kernel(s)
            if k is not None:
                counts[sm.kernel_name(k).split("<")[0]] += 1
                continue
            name = plain_name(s)
            assert name in OTHER, f"{stem}.s: kernel {name} ({s}) is in no table and not in the list of non-templated kernels"
            assert OTHER[name][0] == stem, (name, stem)
            seen_other[name] += 1
    assert seen_other == collections.Counter(list(OTHER)), f"listed kernels the build does not have: {sorted(set(OTHER) - set(seen_other))}"
    assert counts == {**FAMILY_COUNTS, **ROLLOUT_COUNTS}, counts
    assert sum(counts.values()) + len(OTHER) == sum(len(v) for v in by_file.values()) == TOTAL_KERNELS
    assert len(km.TABLE) == sum(ROLLOUT_COUNTS.values())
    for name, (_, test_file, test_name) in OTHER.items():          # the tests the list names exist
        text = open(os.path.join(ROOT, "tests", test_file)).read()
        assert f"def {test_name}(" in text and "pytest.mark.gpu" in text, (name, test_file, test_name)


def _oracle_policy(oracle, row):
    from tests.util import make_deep_policy_arrays, make_policy_arrays, oracle_policy, puzzle_transpose_twist
    n2, idx = row.w * row.h, sm.TABLE.index(row)
    op, ap = puzzle_transpose_twist(row.w) if row.twists else ((), ())
    arrs = (make_deep_policy_arrays(n2, seed=idx, emb=row.emb, common=row.common, scale=2.0) if row.common is not None else
            make_policy_arrays(n2, seed=idx, emb=row.emb, hidden=row.hidden, scale=2.0))
    return oracle_policy(oracle, arrs, op, ap)


def test_the_checks_of_a_self_play_result_by_itself_hold_on_the_oracle(oracle):
    """search_matrix.check_self_play_output (what the GPU test asks of a collect's own arrays) on the oracle's collect of every fifth
    self-play row -- and it notices one probability moved by an ulp, one remaining value moved by an ulp, and a swapped pair of tiles."""
    import numpy as np
    rows = [r for r in sm.TABLE if r.entry == "az"][::5]
    assert len(rows) >= 25 and any(r.S == 0 for r in rows) and any(r.w * r.h > 16 for r in sm.TABLE if r.entry == "az")
    for row in rows:
        o = oracle.az_collect(oracle.Puzzle(row.w, row.h, row.diff, 2, 256), _oracle_policy(oracle, row), row.E, row.S, 1.41, row.med,
                              seed=100 + sm.TABLE.index(row), arith=oracle.ARITH_CHAIN, num_threads=4, merge_order=False, det_math=True)
        L = o.ep_len.astype(np.int64)
        a = {"obs": o.obs, "logits": o.logits, "remaining_values": o.additional_data["remaining_values"], "ep_len": o.ep_len,
             "ep_start": np.concatenate([[0], np.cumsum(L)[:-1]])}
        sm.check_self_play_output(a, row)
        if row is rows[1]:
            assert row.S > 0 and L.max() > 1
            for field, edit in (("logits", lambda x: np.nextafter(x, np.float32(2.0))), ("remaining_values", lambda x: np.nextafter(x, np.float32(2.0)))):
                bad = dict(a)
                bad[field] = a[field].copy()
                i = np.unravel_index(np.argmax(bad[field] > 0) if field == "logits" else 0, bad[field].shape)
                bad[field][i] = edit(bad[field][i])
                with pytest.raises(AssertionError):
                    sm.check_self_play_output(bad, row)
            bad = dict(a)
            bad["obs"] = a["obs"].copy()
            cells = row.w * row.h
            t = int(np.flatnonzero(L > 1)[0])                       # second record of an episode: swap the tiles of two cells that are not the blank
            r = int(a["ep_start"][t]) + 1
            c = [k for k in range(cells) if bad["obs"][r, k] % cells != 0][:2]
            v0, v1 = bad["obs"][r, c[0]] % cells, bad["obs"][r, c[1]] % cells
            bad["obs"][r, c[0]], bad["obs"][r, c[1]] = c[0] * cells + v1, c[1] * cells + v0
            with pytest.raises(AssertionError):
                sm.check_self_play_output(bad, row)


def test_the_oracles_attempts_reduce_to_its_evaluate(oracle):
    """oracle.evaluate_attempts + oracle.reduce_attempts (what the GPU test holds tw_debug_last_attempts and tw_evaluate's two means to)
    reproduce oracle.evaluate's bits -- greedy and sampled, with and without MCTS, boards above 16 cells -- and oracle.solve's best attempt."""
    import numpy as np
    from tests.util import f32_bits
    rows = [r for r in sm.TABLE if r.entry == "evaluate" and sm.attempts(r) <= 2000]
    assert len(rows) >= 12 and any(r.S for r in rows) and any(r.det for r in rows) and any(r.w * r.h > 16 for r in rows)
    for row in rows:
        env, pol = oracle.Puzzle(row.w, row.h, row.diff, 2, 256), _oracle_policy(oracle, row)
        kw = dict(num_mcts_searches=row.S, seed=100 + sm.TABLE.index(row), Cc=1.41, max_expand_depth=row.med, arith=oracle.ARITH_CHAIN, det_math=True)
        s, t, n = oracle.evaluate_attempts(env, pol, row.E, row.det, row.ns, num_threads=4, **kw)
        rate, mean, _ = oracle.reduce_attempts(s, t, row.E, row.ns)
        ref = oracle.evaluate(env, pol, row.E, row.det, row.ns, **kw)
        assert f32_bits(ref[0]) == f32_bits(rate) and f32_bits(ref[1]) == f32_bits(mean), (row, ref, rate, mean)
        assert n.max() <= 2 * row.diff and set(np.unique(s)) <= {0.0, 1.0}
    for row in [r for r in sm.TABLE if r.entry == "solve"]:
        env, pol = oracle.Puzzle(row.w, row.h, row.diff, 2, 16), _oracle_policy(oracle, row)
        start = oracle.Puzzle(row.w, row.h, row.diff, 2, 16)
        start.reset(seed=7, episode=3)
        env.set_state(start.get_state())
        kw = dict(num_mcts_searches=row.S, seed=7, Cc=1.41, max_expand_depth=row.med, arith=oracle.ARITH_CHAIN, det_math=True)
        s, t, n = oracle.evaluate_attempts(env, pol, 1, row.det, row.ns, num_threads=2, from_state=True, **kw)
        _, _, best = oracle.reduce_attempts(s, t, 1, row.ns)
        (rs, rr), acts = oracle.solve(env, pol, row.det, row.ns, **kw)
        assert f32_bits(s[best[0]]) == f32_bits(rs) and f32_bits(t[best[0]]) == f32_bits(rr) and n[best[0]] == len(acts), row
