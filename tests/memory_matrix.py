"""Every entry point that lays out device memory, one case per carve and per side of each condition that adds a segment (GPU-free).

The library clears none of its device buffers: the trajectory workspace is cached across calls (`ws_reserve`, tw_api.hip), result
arenas come back from a pool (`arena_acquire`), call-local scratch comes from `scratch_alloc` (one hipMalloc, which hands back recently
freed blocks).  Every entry point initialises the words it needs on the stream and every kernel is trusted to read only what it or a
predecessor in the same call wrote.  tests/test_gpu_memory_matrix.py holds the library to that: with the test hook
`tw_debug_fill_memory` every one of those buffers is set to a 32-bit pattern before use, and a case must return the same bytes under
0xFFFFFFFF, 0x00000001, 0x00000000 and -- hook off -- on the leftovers of the identical call under another policy's weights.

This file is the table.  `SEGMENTS` names every `seg(` of every call carve in source order (the two policy-image builders at the top
of tw_api.hip are no call carves: a policy image is uploaded whole and tests/test_gpu_policy_sync.py compares it byte for byte);
`SEG_COUNTS` / `MALLOC_COUNTS` are what tests/test_memory_matrix.py counts in twisterl_amd/csrc, so that a new workspace segment or a
new raw allocation has to come here first, as a new kernel has to come to tests/search_matrix.py.  `CONDITIONS` says which condition
adds which segments (or, where it adds none, which words the entry point initialises only then); every condition has a case that turns
it on and a case of the same carve that leaves it off.

A case points to the row of the existing table that runs its shape (tests/kernel_matrix.py, tests/search_matrix.py,
tests/finalize_matrix.py, the device-environment tables, the named cases of the drain / reuse / range tests) instead of restating it;
`ref` is resolved by tests/test_gpu_memory_matrix.py, which runs the row's own check under the first fill.  The few shapes no table
has (the self-play shapes the issue names by size, solve from a 25-cell state) are rows built with the tables' own constructors.
"""
from collections import namedtuple

from tests import finalize_matrix as fm
from tests import kernel_matrix as km
from tests import search_matrix as sm

PATTERNS = (0xFFFFFFFF, 0x00000001, 0x00000000)

# ---------------------------------------------------------------------------------------------- census (tests/test_memory_matrix.py)
# `seg(` per carve, in source order.  tw_api.hip is counted behind `struct tw_collected {`: the policy-image builders lie in front of it.
SEGMENTS = {
    "tw_api.hip": {
        "tw_debug_collect_tail": "o_rec o_len o_start o_total o_scan o_obs16 o_lgw",
        "tw_ppo_collect": "o_rec o_len o_start o_total o_resume o_scan o_init o_queue o_obs16 o_boards o_ordscr",
        "tw_az_collect": "o_rec o_len o_start o_total o_scan o_arena o_init o_queue o_order o_ordscr o_obs16 o_tbl o_mb",
        "run_solve": "o_s o_r o_n o_a o_cells o_cnt o_arena o_tbl o_init o_queue o_sv",
    },
    "tw_device_env.hip": {
        "tw_ppo_collect_device_env": "o_rec o_len o_start o_total o_scan o_obs16 o_lgw",
        "tw_az_collect_device_env": "o_rec o_len o_start o_total o_scan o_obs16 o_ce o_arena o_pw",
        "run_attempts_device_env": "o_s o_t o_n o_err o_ce o_arena o_act",
    },
    "tw_comm.hip": {
        "gather_alloc": "off[f] o_len o_start o_tot o_scan",         # (scratch_alloc: filled by the hook; run by tests/test_gpu_multirank.py only)
    },
}
SEGMENTS = {f: {carve: names.split() for carve, names in carves.items()} for f, carves in SEGMENTS.items()}
SEG_COUNTS = {f: sum(len(n) for n in carves.values()) for f, carves in SEGMENTS.items()}        # 42, 23, 5
POLICY_IMAGE_MARK = "struct tw_collected {"       # tw_api.hip: `seg(` in front of this line builds policy images
# `hipMalloc(` per file, message texts included (the scan knows two words).  tw_api.hip: scratch_alloc (1), ws_reserve (2 + its message),
# arena_acquire (2 + its message), the two policy images (2); tw_comm.hip: the transport's count buffer.  Everything else allocates
# through scratch_alloc, which fills.
MALLOC_COUNTS = {"tw_api.hip": 9, "tw_comm.hip": 1}

# ---------------------------------------------------------------------------------------------- conditions
# carve -> {condition: the segments it adds (or, in parentheses, the words that are initialised only then)}
CONDITIONS = {
    "tw_debug_collect_tail": {"obs16": ["o_obs16"], "wide": ["o_lgw"]},
    "tw_ppo_collect": {
        "persist": ["o_init", "o_queue", "o_boards", "o_ordscr"],
        "drain": ["o_resume", "(o_total + 16: resume_cnt, + 20: drain_queue)"],
        "big": ["o_obs16"],
        "reuse_words": ["(o_total + 8 .. + 20 cleared: the launches that can take the 256-episode f32 shape)"],
        "reuse_rounds": ["(RolloutArgs::reused counted by the kernel: the 256-episode f32 shape)"],
        "generic": ["(EngineV: no counters beside the record total)"],
        "fp16": ["(Engine16)"],
        "range_flag": ["(o_total + 8 copied from the policy's split_range: fp16x2)"],
        "range_fallback": ["(a second rollout, fp32, on the same workspace)"],
    },
    "tw_az_collect": {
        "persist": ["o_init", "o_queue"],
        "deep": ["o_order", "o_ordscr", "o_tbl"],
        "decoupled": ["(request / completion hand-shake in LDS)"],
        "split": ["o_mb"],
        "big": ["o_obs16"],
        "deep_tree": ["(statistics beyond the LDS nodes live in o_arena)"],
    },
    "run_solve": {
        "want_actions": ["o_a"],
        "big_state": ["o_cells"],
        "mcts": ["o_cnt", "o_arena"],
        "deep": ["o_tbl", "o_queue", "o_sv"],
        "deep_boards": ["o_init"],
        "deterministic": ["(no draw)"],
    },
    "tw_ppo_collect_device_env": {"wide": ["o_lgw"], "queued": ["(o_total + 16: the episode queue's counter)"], "var_obs": ["(0xFFFF in the free slots of o_obs16)"]},
    "tw_az_collect_device_env": {"wide": ["o_pw"]},
    "run_attempts_device_env": {"mcts": ["o_ce", "o_arena"]},
    "host_stepped": {"az": ["(HostEvalBatch)"], "solve": ["(HostEvalBatch, no result arena)"]},
    "trainer_hand_off": {"normalize": ["(sum scratch of tw_collected_adv_stats)"], "az": ["(no pack kernel: one-hot only)"]},
}

Case = namedtuple("Case", "id carve family ref on counters")
# counters: the result's count statistics are compared too (False where the order in which persistent lanes / walkers reach the episode
# queue -- timing -- decides which lane runs which episode, and with it how many evaluations a board table saves: the bytes do not depend
# on it, the counts may)


def _km(*a, **k):
    row = km.R(*a, **k)
    assert row in km.TABLE, row
    return row


def _sm(row):
    assert row in sm.TABLE, row
    return row


def C(id_, carve, family, ref, on=(), counters=True):
    return Case(id_, carve, family, ref, frozenset(on), counters)


AB1, AB16 = km.AB1, sm.AB16
# the shapes no table has a row of, built with the tables' constructors (tests/test_memory_matrix.py holds their restated dispatch)
WALKER_DEEP_TREE = sm.AZ(4, 4, 64, 256, 9, 300, diff=10, twists=True, covers="extra")      # the test_gpu_parity.py shape "trees larger than the LDS table"
SPLIT_2048 = sm.AZ(4, 4, 32, 128, 2048, 1, diff=4, covers="extra")                           # 8 episodes per CU: the split shape at one search per move
SOLVE_25_CELLS = sm.SV(5, 5, 32, 0, 3, diff=8, common=(64, 32), covers="extra")              # solve from a state of 25 cells (one byte per cell)
EXTRA_ROWS = {"walker_deep_tree": (WALKER_DEEP_TREE, "mcts_deep_kernel<8, 16, -16, 1, false, false, false>"),
              "split_2048": (SPLIT_2048, "mcts_deep_kernel<4, 16, -16, 12, false, true, true>"),
              "solve_25_cells": (SOLVE_25_CELLS, "solve_big_kernel<25>")}

CASES = [
    # ---- tw_debug_collect_tail (tests/finalize_matrix.py; tests/test_gpu_finalize.py's check compares every field with numpy)
    C("tail-plain", "tw_debug_collect_tail", "tail", fm._ppo(fm.E0, 65)),
    C("tail-obs16-wide", "tw_debug_collect_tail", "tail", fm._ppo(fm.E0, 65, n_cells=25, ids=2, A=31), {"obs16", "wide"}),
    C("tail-az-obs8-narrow", "tw_debug_collect_tail", "tail", fm._az(fm.E0, 65, n_cells=25, ids=1, A=3), {"obs16"}),
    # ---- tw_ppo_collect
    C("ppo-resident", "tw_ppo_collect", "km", _km(4, 4, 32, 32, 300), {"reuse_words"}),
    C("ppo-queue", "tw_ppo_collect", "km", _km(4, 3, 64, 128, 300, force_geom=8, reserve=AB1), {"persist", "reuse_words", "reuse_rounds"}),
    C("ppo-drain", "tw_ppo_collect", "drain", ("p8_plain", 32), {"persist", "drain", "reuse_words", "reuse_rounds"}),
    C("ppo-reuse-rounds", "tw_ppo_collect", "reuse", "p15_plain", {"reuse_words", "reuse_rounds"}),
    C("ppo-big-board", "tw_ppo_collect", "sm_ppo", _sm(sm.PPO(5, 5, 64, (128,), 150, diff=5)), {"big", "generic"}),
    C("ppo-generic-queue", "tw_ppo_collect", "km", _km(4, 3, 32, 0, 300, common=(48, 24), reserve=AB1), {"persist", "generic"}),
    C("ppo-fp16-queue", "tw_ppo_collect", "km", _km(4, 4, 32, 32, 300, "fp16", reserve=AB1, twists=True), {"persist", "fp16"}),
    C("ppo-fp16x2-in-range", "tw_ppo_collect", "km", _km(4, 4, 96, 32, 300, "fp16x2"), {"range_flag"}),
    C("ppo-fp16x2-out-of-range", "tw_ppo_collect", "range", (3, "h1_300"), {"range_flag", "range_fallback", "reuse_words"}),
    # ---- tw_az_collect
    C("az-lane", "tw_az_collect", "sm_az", _sm(sm.AZ(4, 4, 32, 32, 150, 36, med=2, diff=7, twists=True))),
    C("az-lane-persistent", "tw_az_collect", "sm_az", _sm(sm.AZ(4, 4, 64, 32, 777, 24, diff=5, twists=True, reserve=AB1)), {"persist"}, counters=False),
    C("az-walker", "tw_az_collect", "sm_az", _sm(sm.AZ(2, 2, 32, 128, 300, 120, diff=7)), {"persist", "deep"}, counters=False),
    C("az-walker-deep-tree", "tw_az_collect", "sm_az", "walker_deep_tree", {"persist", "deep", "deep_tree"}, counters=False),
    C("az-decoupled", "tw_az_collect", "sm_az", _sm(sm.AZ(4, 4, 32, 128, 701, 30, diff=6)), {"persist", "deep", "decoupled"}, counters=False),
    C("az-split-2048", "tw_az_collect", "sm_az", "split_2048", {"persist", "deep", "decoupled", "split"}, counters=False),
    C("az-split-deep-tree", "tw_az_collect", "sm_az", _sm(sm.AZ(2, 2, 32, 256, 128, 450, diff=7, reserve=AB16)),
      {"persist", "deep", "decoupled", "split", "deep_tree"}, counters=False),
    C("az-big-board", "tw_az_collect", "sm_az", _sm(sm.AZ(5, 5, 64, 0, 40, 8, diff=5, twists=True, common=(64, 32))), {"big"}),
    # ---- evaluate / solve (run_solve)
    C("eval-sampled", "run_solve", "sm_eval", _sm(sm.EV(3, 3, 32, 64, 150, 4, diff=5, twists=True))),
    C("eval-deterministic", "run_solve", "sm_eval", _sm(sm.EV(4, 3, 32, 32, 333, 1, det=True, diff=5)), {"deterministic"}),
    C("eval-mcts-lane", "run_solve", "sm_eval", _sm(sm.EV(3, 3, 32, 32, 40, 3, S=6, diff=4, covers="extra")), {"mcts"}),
    C("eval-mcts-deep", "run_solve", "sm_eval", _sm(sm.EV(3, 2, 32, 128, 251, 4, S=6, diff=4)), {"mcts", "deep", "deep_boards"}),
    C("solve-actions", "run_solve", "sm_eval", _sm(sm.SV(4, 4, 32, 64, 5, diff=6)), {"want_actions"}),
    C("solve-mcts-deep-actions", "run_solve", "sm_eval", _sm(sm.SV(3, 3, 64, 128, 6, S=20, diff=6, twists=True)), {"want_actions", "mcts", "deep"}),
    C("solve-25-cells", "run_solve", "sm_eval", "solve_25_cells", {"want_actions", "big_state"}),
    # ---- device environments (tests/device_env_matrix.py, device_env_wide.py, device_env_wide_search.py, device_env_solve.py, var_obs_util.py)
    C("denv-collect", "tw_ppo_collect_device_env", "denv_ppo", ("matrix", "probe_o4a2", 40)),
    C("denv-collect-queued", "tw_ppo_collect_device_env", "denv_ppo_queued", ("matrix", "probe_o16a3", 1), {"queued"}),
    C("denv-collect-wide", "tw_ppo_collect_device_env", "denv_ppo", ("wide", "wideo17a17", None), {"wide"}),
    C("denv-collect-wide-queued", "tw_ppo_collect_device_env", "denv_ppo_queued", ("wide", "wideo64a31", 1), {"wide", "queued"}),
    C("denv-collect-var-obs", "tw_ppo_collect_device_env", "denv_var", 12, {"var_obs"}),
    C("denv-search", "tw_az_collect_device_env", "denv_az", ("matrix", "probe_o9a3s", (40, 6, 2))),
    C("denv-search-wide", "tw_az_collect_device_env", "denv_az", ("wide", "wideo16a16_ws", None), {"wide"}),
    C("denv-solve", "run_attempts_device_env", "denv_solve", ("gridworld", 17, 0)),
    C("denv-solve-mcts", "run_attempts_device_env", "denv_solve", ("gridworld", 17, 8), {"mcts"}),
    # ---- the host-stepped path over a Python environment (tw_env_generic.hip; tests/test_gpu_parity.py's GridWorld)
    C("host-collect", "host_stepped", "host_ppo", (5, 5, 12, 64, (128, 32), 60)),
    C("host-self-play", "host_stepped", "host_az", (3, 3, 8, 64, (64,), 120, 8, 1), {"az"}),
    C("host-solve", "host_stepped", "host_solve", (3, 3, 8, 64, (64,), (False, 2, 4)), {"solve"}),
    # ---- the trainer hand-off (tests/test_gpu_trainer_handoff.py's layouts)
    C("handoff-ppo-normalized", "trainer_hand_off", "handoff_ppo", "c", {"normalize"}),
    C("handoff-ppo", "trainer_hand_off", "handoff_ppo_plain", "a"),
    C("handoff-az", "trainer_hand_off", "handoff_az", "b", {"az"}),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]


def row_of(case):
    """The kernel_matrix / search_matrix row of a case that has one."""
    return EXTRA_ROWS[case.ref][0] if isinstance(case.ref, str) and case.ref in EXTRA_ROWS else case.ref
