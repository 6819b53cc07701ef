"""Every entry point that launches on the library's stream (`tw_set_stream`, thread-local), one case per shape of
tests/memory_matrix.py plus the entry points that table does not reach (GPU-free).

On the legacy null stream, where every other test runs, ordering against blocking streams is free and memory is mostly zero: a launch or
an async copy that went to stream 0 instead of the caller's stream `s`, a missing event between `s` and the self-play side stream, a
wrong fence when a pooled arena changes hands -- all of them still give the right bytes there.  On a non-blocking stream (every
torch.cuda.Stream is one) each is a silent race.  tests/test_gpu_stream_matrix.py runs every case of this table on such a stream, with
the caller's stream or the null stream kept busy by a delay kernel, and tests/test_gpu_threads.py runs the promises of INTEGRATION.md
("Threads and streams") from two threads.

This file is the table.  `STREAM_USERS` names every function of twisterl_amd/csrc that asks for `current_stream()`, with how often and
with the C entry points through which a caller reaches it; tests/test_stream_matrix.py counts the sources against it, so that a new user
of the stream has to come here first.  A case records which modes it runs (`MODE1`: the caller's stream is busy -- runs b and c of
tests/test_gpu_stream_matrix.py; `MODE2`: the null stream is busy, run d, the collect families) and which of the entry points the test
delays (`LISTED`) it reaches.
"""
from collections import namedtuple

from tests import memory_matrix as mm

MODE1, MODE2 = "caller's stream busy", "null stream busy"

# ---------------------------------------------------------------------------------------------- census (tests/test_stream_matrix.py)
NOT_RUN = "multi-rank, not run here"
# file -> {function: (`current_stream()` in it, the C entry points that reach it)}
STREAM_USERS = {
    "tw_api.hip": {
        "current_stream": (1, ()),                                                        # the definition
        "ws_reserve": (1, ("tw_ppo_collect", "tw_az_collect", "tw_debug_collect_tail", "tw_ppo_collect_device_env", "tw_az_collect_device_env",
                           "tw_evaluate_device_env", "tw_solve_device_env")),
        "arena_acquire": (3, ("tw_ppo_collect", "tw_az_collect", "tw_debug_collect_tail", "tw_ppo_collect_device_env", "tw_az_collect_device_env")),
        "arena_release": (1, ("tw_collected_free",)),
        "tw_policy_update_device": (2, ("tw_policy_update_device",)),
        "tw_policy_update_device_layers": (1, ("tw_policy_update_device_layers",)),
        "tw_debug_policy_image": (1, ("tw_debug_policy_image",)),
        "tw_policy_evaluate": (1, ("tw_policy_evaluate",)),
        "tw_collected_adv_stats": (1, ("tw_collected_adv_stats",)),
        "tw_collected_pack_trainer": (1, ("tw_collected_pack_trainer",)),
        "collected_adopt": (1, ("tw_ppo_collect_env", "tw_az_collect_env")),
        "tw_debug_collect_tail": (1, ("tw_debug_collect_tail",)),
        "tw_debug_collected_arena": (1, ("tw_debug_collected_arena",)),
        "tw_debug_episode_order": (1, ("tw_debug_episode_order",)),
        "ppo_collect_once": (1, ("tw_ppo_collect",)),
        "az_collect_once": (1, ("tw_az_collect",)),
        "run_solve": (1, ("tw_evaluate", "tw_solve")),
    },
    "tw_common.hpp": {"current_stream": (1, ())},                                         # the declaration
    "tw_device_env.hip": {
        "tw_ppo_collect_device_env": (3, ("tw_ppo_collect_device_env",)),                 # two of them: the fp16 layer table's copy and its wait
        "tw_az_collect_device_env": (1, ("tw_az_collect_device_env",)),
        "attempts_device_env": (3, ("tw_evaluate_device_env", "tw_solve_device_env")),    # (the same two)
    },
    "tw_env_generic.hip": {
        "upload_collected": (1, ("tw_ppo_collect_env", "tw_az_collect_env")),
        "tw_ppo_collect_env": (1, ("tw_ppo_collect_env",)),
        "tw_az_collect_env": (1, ("tw_az_collect_env",)),
        "run_attempts_env": (1, ("tw_evaluate_env", "tw_solve_env32")),
    },
    "tw_comm.hip": {"tw_comm_broadcast_policy": (1, NOT_RUN)},
}
STREAM_COUNTS = {f: sum(n for n, _ in fns.values()) for f, fns in STREAM_USERS.items()}      # 20, 1, 7, 4, 1

# The entry points tests/test_gpu_stream_matrix.py puts a delay in front of: collect, evaluate, solve, the trainer hand-off, the policy
# updates, tw_policy_evaluate (and the tail hook, which is a collect's second half on records of the caller).
# WAITS: the call returns only after its stream has finished.  The others only enqueue (the hand-off without normalisation, the updates).
WAITS = ("tw_ppo_collect", "tw_az_collect", "tw_evaluate", "tw_solve", "tw_ppo_collect_env", "tw_az_collect_env", "tw_evaluate_env",
         "tw_solve_env32", "tw_ppo_collect_device_env", "tw_az_collect_device_env", "tw_evaluate_device_env", "tw_solve_device_env",
         "tw_collected_adv_stats", "tw_policy_evaluate", "tw_debug_collect_tail")
ENQUEUES = ("tw_collected_pack_trainer", "tw_policy_update_device", "tw_policy_update_device_layers")
LISTED = WAITS + ENQUEUES
# entry points that use the stream and that no case puts a delay in front of: the free (tests/test_gpu_threads.py runs its fence) and three
# test hooks -- every snapshot of a collect reads the arena through the first, the policy-update cases read the image, and the episode
# order has a test of its own in tests/test_gpu_stream_matrix.py
UNLISTED = {"tw_collected_free": "tests/test_gpu_threads.py", "tw_debug_collected_arena": "every snapshot of a collect",
            "tw_debug_episode_order": "test_episode_order_hook_on_a_busy_stream", "tw_debug_policy_image": "the policy-update cases"}

# ---------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "id family ref modes entries")

FAMILY_ENTRIES = {
    "tail": ("tw_debug_collect_tail",),
    "km": ("tw_ppo_collect",), "drain": ("tw_ppo_collect",), "reuse": ("tw_ppo_collect",), "range": ("tw_ppo_collect",), "sm_ppo": ("tw_ppo_collect",),
    "sm_az": ("tw_az_collect",),
    "sm_eval": None,                                        # tw_evaluate or tw_solve, by the row (below)
    "denv_ppo": ("tw_ppo_collect_device_env",), "denv_ppo_queued": ("tw_ppo_collect_device_env",), "denv_var": ("tw_ppo_collect_device_env",),
    "denv_az": ("tw_az_collect_device_env",), "denv_solve": ("tw_solve_device_env",),
    "host_ppo": ("tw_ppo_collect_env",), "host_az": ("tw_az_collect_env",), "host_solve": ("tw_evaluate_env", "tw_solve_env32"),
    "handoff_ppo": ("tw_ppo_collect_env", "tw_collected_pack_trainer", "tw_collected_adv_stats"),
    "handoff_ppo_plain": ("tw_ppo_collect_env", "tw_collected_pack_trainer"),
    "handoff_az": ("tw_az_collect_env", "tw_collected_pack_trainer"),
}
# run d: the families whose call is one collect (the issue's list)
MODE2_FAMILIES = ("km", "drain", "reuse", "range", "sm_ppo", "sm_az", "denv_ppo", "denv_ppo_queued", "denv_var", "denv_az", "denv16_ppo")
# case id -> why run d is not held to "the call did not wait for the null stream" (no Puzzle tw_ppo_collect / tw_az_collect case may be here)
MODE2_EXEMPT = {}


def _from_memory_matrix(c):
    entries = FAMILY_ENTRIES[c.family]
    if entries is None:
        entries = ("tw_solve",) if mm.row_of(c).entry == "solve" else ("tw_evaluate",)
    return Case(c.id, c.family, c.ref, (MODE1, MODE2) if c.family in MODE2_FAMILIES else (MODE1,), entries)


# the rows the memory matrix does not have: (module of the row, its name, the shape)
EXTRA = [
    Case("denv16-collect", "denv16_ppo", ("tests/test_gpu_device_env_fp16.py", "gw3_no_multiple", 100), (MODE1, MODE2), ("tw_ppo_collect_device_env",)),
    Case("denv16-solve-actions", "denv16_solve", ("tests/test_gpu_device_env_fp16_solve.py", "gw3_no_multiple", 8), (MODE1,), ("tw_solve_device_env",)),
    # (the table's own finding: no case of the memory matrix evaluates a device environment on the device)
    Case("denv16-evaluate", "denv16_eval", ("tests/test_gpu_device_env_fp16_solve.py", "gw3_no_multiple", (34, 3)), (MODE1,), ("tw_evaluate_device_env",)),
    Case("policy-update-mfma", "policy_update", ("tests/policy_sync_matrix.py", "ONE_TABLE", 0), (MODE1,), ("tw_policy_update_device", "tw_ppo_collect")),
    Case("policy-update-generic", "policy_update", ("tests/policy_sync_matrix.py", "GEN_TABLE", 3), (MODE1,), ("tw_policy_update_device_layers", "tw_ppo_collect")),
    Case("policy-evaluate", "policy_eval", ("tests/eval_matrix.py", "basic-tw3", None), (MODE1,), ("tw_policy_evaluate",)),
]
CASES = [_from_memory_matrix(c) for c in mm.CASES] + EXTRA
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
