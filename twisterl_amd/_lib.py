"""ctypes binding of the C ABI in include/twisterl_hip.h (libtwisterl_hip.so).

This is the only place the shared library is loaded.  There is no fallback: if the library is
missing it is built with hipcc; if that fails, or no GPU is present when a compute entry point
is called, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

# status codes (include/twisterl_hip.h)
TW_OK, TW_ERR_INVALID, TW_ERR_UNSUPPORTED, TW_ERR_NO_DEVICE, TW_ERR_HIP, TW_ERR_EMPTY = range(6)
TW_PREC_F32_EXACT, TW_PREC_F16, TW_PREC_F16X2 = 0, 1, 2
TW_EVAL_FORWARD, TW_EVAL_PREDICT, TW_EVAL_FULL_PREDICT = 0, 1, 2
TW_OPT_FORCE_GEOM, TW_OPT_NO_PERSIST, TW_OPT_AZ_VARIANT, TW_OPT_AZ_TREE_BUDGET, TW_OPT_AZ_TREE_BUDGET_MIN, TW_OPT_AZ_REUSE = 0, 1, 2, 3, 4, 5
TW_OPT_ENV_RESIDENT_GROUPS = 6
TW_OPT_ROLLOUT_REUSE = 8       # (7 stays unassigned: tw_set_launch_option refuses it)
TW_OPT_ROLLOUT_DRAIN = 9       # hand-over of the persistent 256-episode f32 rollout: 0 automatic, 1 .. 256 live episodes, -1 off
ABI_VERSION = 6
(TW_F_OBS, TW_F_LOGITS, TW_F_PERMS, TW_F_VALUES, TW_F_REWARDS, TW_F_ACTIONS, TW_F_ADVS, TW_F_RETS,
 TW_F_REMAINING, TW_F_EP_LEN, TW_F_EP_START, TW_F_COUNT) = range(12)

PRECISIONS = {"fp32": TW_PREC_F32_EXACT, "f32": TW_PREC_F32_EXACT, "exact": TW_PREC_F32_EXACT,
              "fp16": TW_PREC_F16, "f16": TW_PREC_F16, "fp16x2": TW_PREC_F16X2, "f16x2": TW_PREC_F16X2}


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 64), ("compute_units", C.c_int32),
                ("wavefront_size", C.c_int32), ("total_mem_bytes", C.c_uint64),
                ("lds_bytes_per_block", C.c_uint64)]


class PuzzleDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("difficulty", C.c_uint32),
                ("depth_slope", C.c_uint32), ("max_depth", C.c_uint32)]


class LinearDesc(C.Structure):
    _fields_ = [("in_features", C.c_uint32), ("out_features", C.c_uint32),
                ("weights", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float)),
                ("apply_relu", C.c_uint32)]


class PolicyDesc(C.Structure):
    _fields_ = [("obs_size", C.c_uint32), ("emb_size", C.c_uint32),
                ("emb_vectors", C.POINTER(C.c_float)), ("emb_bias", C.POINTER(C.c_float)),
                ("emb_apply_relu", C.c_uint32),
                ("n_common", C.c_uint32), ("common", C.POINTER(LinearDesc)),
                ("n_action", C.c_uint32), ("action", C.POINTER(LinearDesc)),
                ("n_value", C.c_uint32), ("value", C.POINTER(LinearDesc)),
                ("n_perms", C.c_uint32), ("n_actions", C.c_uint32),
                ("obs_perms", C.POINTER(C.c_int32)), ("act_perms", C.POINTER(C.c_int32))]


class PPOParams(C.Structure):
    _fields_ = [("num_episodes", C.c_uint64), ("episode_offset", C.c_uint64),
                ("gamma", C.c_float), ("lambda_", C.c_float), ("seed", C.c_uint64),
                ("precision", C.c_uint32), ("merge_order", C.c_uint32), ("reserve_cus", C.c_uint32)]


class AZParams(C.Structure):
    _fields_ = [("num_episodes", C.c_uint64), ("episode_offset", C.c_uint64),
                ("num_mcts_searches", C.c_uint32), ("C", C.c_float), ("max_expand_depth", C.c_uint32),
                ("seed", C.c_uint64), ("precision", C.c_uint32), ("merge_order", C.c_uint32),
                ("reserve_cus", C.c_uint32)]


class SolveParams(C.Structure):
    _fields_ = [("deterministic", C.c_uint32), ("num_searches", C.c_uint32), ("num_mcts_searches", C.c_uint32),
                ("C", C.c_float), ("max_expand_depth", C.c_uint32), ("seed", C.c_uint64), ("precision", C.c_uint32)]


class CollectStats(C.Structure):
    _fields_ = [("ms_rollout", C.c_float), ("ms_scan", C.c_float), ("ms_finalize", C.c_float),
                ("ms_total", C.c_float), ("records", C.c_uint64), ("episodes", C.c_uint64),
                ("padded_bytes", C.c_uint64), ("rollout_blocks", C.c_uint32),
                ("rollout_threads", C.c_uint32), ("forward_evals", C.c_uint64), ("speculative_evals", C.c_uint64), ("reused_evals", C.c_uint64)]


class LaunchInfo(C.Structure):
    _fields_ = [("family", C.c_int32), ("nt", C.c_int32), ("nc", C.c_int32), ("nw", C.c_int32), ("nwk", C.c_int32),
                ("persist", C.c_uint32), ("solve", C.c_uint32), ("dec", C.c_uint32), ("split", C.c_uint32),
                ("blocks", C.c_uint32), ("threads", C.c_uint32), ("engine_blocks", C.c_uint32), ("engine_threads", C.c_uint32)]


(TW_KERNEL_NONE, TW_KERNEL_MCTS_F32, TW_KERNEL_SOLVE_F32, TW_KERNEL_MCTS_DEEP, TW_KERNEL_MCTS_BIG, TW_KERNEL_SOLVE_BIG,
 TW_KERNEL_ROLLOUT_BIG, TW_KERNEL_ONEHOT) = range(8)


TW_FIN_NONE, TW_FIN_GROUP16, TW_FIN_GROUP8, TW_FIN_WAVE, TW_FIN_AZ = range(5)


class FinalizeLaunch(C.Structure):
    _fields_ = [("form", C.c_uint32), ("waves", C.c_uint32), ("blocks", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint64)]


class DebugTailArgs(C.Structure):
    _fields_ = [("n_episodes", C.c_uint64), ("t_pad", C.c_uint32), ("is_ppo", C.c_uint32), ("n_cells", C.c_uint32), ("n_actions", C.c_uint32),
                ("obs_width", C.c_uint32), ("merge_order", C.c_uint32), ("scan_only", C.c_uint32), ("arena_fill", C.c_uint32),
                ("gamma", C.c_float), ("lambda_", C.c_float), ("ep_len", C.c_void_p), ("records", C.c_void_p), ("obs16", C.c_void_p),
                ("wide", C.c_void_p), ("ep_start_out", C.c_void_p), ("total_out", C.c_void_p)]


class EnvVTable(C.Structure):
    _fields_ = [("prototype", C.c_void_p), ("num_actions", C.c_uint32), ("n_obs", C.c_uint32), ("obs_size", C.c_uint32),
                ("clone", C.CFUNCTYPE(C.c_void_p, C.c_void_p)), ("destroy", C.CFUNCTYPE(None, C.c_void_p)),
                ("reset", C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64)), ("step", C.CFUNCTYPE(None, C.c_void_p, C.c_uint32)),
                ("observe", C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_int32))), ("masks", C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8))),
                ("reward", C.CFUNCTYPE(C.c_float, C.c_void_p)), ("is_final", C.CFUNCTYPE(C.c_int, C.c_void_p)),
                ("success", C.CFUNCTYPE(C.c_int, C.c_void_p)),
                # the rest of `trait Env` (rust/src/rl/env.rs:30,58-66); NULL = the trait's default body
                ("track_solution", C.CFUNCTYPE(C.c_int, C.c_void_p)),
                ("solution", C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32)),
                ("set_state", C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_int64), C.c_uint32)),
                ("twists", C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32)),
                # observations of variable length (optional, trailing; NULL = observe() and its fixed length): writes at most `cap`
                # ids, returns how many; n_obs is then the maximum
                ("observe_n", C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32))]


class CommId(C.Structure):
    _fields_ = [("bytes", C.c_ubyte * 128)]      # (c_ubyte: a c_char array field would read back truncated at the first NUL)


# every symbol include/twisterl_hip.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "tw_abi_version": (C.c_int, []),
    "tw_last_error": (C.c_char_p, []),
    "tw_device_count": (C.c_int, []),
    "tw_set_device": (C.c_int, [C.c_int]),
    "tw_set_stream": (C.c_int, [_VP]),
    "tw_get_device_info": (C.c_int, [C.POINTER(DeviceInfo)]),
    "tw_release_cached_memory": (C.c_int, []),
    "tw_set_launch_option": (C.c_int, [C.c_int, C.c_int]),
    "tw_debug_counters": (C.c_int, [C.POINTER(C.c_uint64), C.c_int]),
    "tw_debug_last_launch": (C.c_int, [C.POINTER(LaunchInfo)]),
    "tw_debug_last_attempts": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint64)]),
    "tw_debug_episode_order": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "tw_debug_policy_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tw_debug_collect_tail": (C.c_int, [C.POINTER(DebugTailArgs), C.POINTER(FinalizeLaunch), C.POINTER(_VP)]),
    "tw_debug_collected_arena": (C.c_int, [_VP, _VP, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tw_debug_fill_memory": (C.c_int, [C.c_int, C.c_uint32]),
    "tw_puzzle_create": (_VP, [C.c_uint32] * 5),
    "tw_puzzle_clone": (_VP, [_VP]),
    "tw_puzzle_destroy": (None, [_VP]),
    "tw_puzzle_get_desc": (C.c_int, [_VP, C.POINTER(PuzzleDesc)]),
    "tw_puzzle_num_actions": (C.c_uint32, [_VP]),
    "tw_puzzle_obs_shape": (C.c_int, [_VP, C.POINTER(C.c_uint32)]),
    "tw_puzzle_set_difficulty": (C.c_int, [_VP, C.c_uint32]),
    "tw_puzzle_get_difficulty": (C.c_uint32, [_VP]),
    "tw_puzzle_set_state": (C.c_int, [_VP, C.POINTER(C.c_int64), C.c_size_t]),
    "tw_puzzle_reset": (C.c_int, [_VP, C.c_uint64, C.c_uint64]),
    "tw_puzzle_step": (C.c_int, [_VP, C.c_uint32]),
    "tw_puzzle_masks": (C.c_int, [_VP, C.POINTER(C.c_uint8)]),
    "tw_puzzle_is_final": (C.c_int, [_VP]),
    "tw_puzzle_reward": (C.c_float, [_VP]),
    "tw_puzzle_observe": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    "tw_puzzle_solved": (C.c_int, [_VP]),
    "tw_puzzle_get_state": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    "tw_puzzle_set_position": (C.c_int, [_VP, C.c_uint32, C.c_uint32, C.c_int64]),
    "tw_puzzle_get_position": (C.c_int64, [_VP, C.c_uint32, C.c_uint32]),
    "tw_puzzle_depth": (C.c_uint32, [_VP]),
    "tw_policy_create": (_VP, [C.POINTER(PolicyDesc)]),
    "tw_policy_destroy": (None, [_VP]),
    "tw_policy_update_device": (C.c_int, [_VP] * 9),
    "tw_policy_update_device_layers": (C.c_int, [_VP, _VP, _VP, C.POINTER(_VP), C.POINTER(_VP), C.c_uint32]),
    "tw_policy_num_actions": (C.c_uint32, [_VP]),
    "tw_policy_num_perms": (C.c_uint32, [_VP]),
    "tw_policy_evaluate": (C.c_int, [_VP, C.c_int, C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)]),
    "tw_ppo_collect": (C.c_int, [C.POINTER(PuzzleDesc), _VP, C.POINTER(PPOParams), C.POINTER(_VP)]),
    "tw_az_collect": (C.c_int, [C.POINTER(PuzzleDesc), _VP, C.POINTER(AZParams), C.POINTER(_VP)]),
    "tw_ppo_collect_env": (C.c_int, [C.POINTER(EnvVTable), _VP, C.POINTER(PPOParams), C.c_uint32, C.POINTER(_VP)]),
    "tw_az_collect_env": (C.c_int, [C.POINTER(EnvVTable), _VP, C.POINTER(AZParams), C.c_uint32, C.POINTER(_VP)]),
    "tw_evaluate_env": (C.c_int, [C.POINTER(EnvVTable), _VP, C.POINTER(SolveParams), C.c_uint64, C.c_uint64, C.c_uint32,
                                  C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tw_solve_env": (C.c_int, [C.POINTER(EnvVTable), _VP, C.POINTER(SolveParams), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                               C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tw_solve_env32": (C.c_int, [C.POINTER(EnvVTable), _VP, C.POINTER(SolveParams), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tw_device_env_host_vtable": (C.c_int, [_VP, _VP, C.c_size_t, C.POINTER(EnvVTable)]),
    "tw_ppo_collect_device_env": (C.c_int, [_VP, _VP, C.c_size_t, _VP, C.POINTER(PPOParams), C.c_uint32, C.POINTER(_VP)]),
    "tw_az_collect_device_env": (C.c_int, [_VP, _VP, C.c_size_t, _VP, C.POINTER(AZParams), C.c_uint32, C.POINTER(_VP)]),
    "tw_evaluate_device_env": (C.c_int, [_VP, _VP, C.c_size_t, _VP, C.POINTER(SolveParams), C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tw_solve_device_env": (C.c_int, [_VP, _VP, C.c_size_t, _VP, C.POINTER(SolveParams), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tw_evaluate":(C.c_int, [C.POINTER(PuzzleDesc), _VP, C.POINTER(SolveParams), C.c_uint64, C.c_uint64,
                              C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "tw_solve": (C.c_int, [_VP, _VP, C.POINTER(SolveParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                           C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]),
    "tw_collected_num_records": (C.c_uint64, [_VP]),
    "tw_collected_num_episodes": (C.c_uint64, [_VP]),
    "tw_collected_num_cells": (C.c_uint32, [_VP]),
    "tw_collected_num_actions": (C.c_uint32, [_VP]),
    "tw_collected_is_ppo": (C.c_int, [_VP]),
    "tw_collected_obs_width": (C.c_uint32, [_VP]),
    "tw_collected_obs_ragged": (C.c_int, [_VP]),
    "tw_collected_device_ptr": (_VP, [_VP, C.c_int, C.POINTER(C.c_size_t)]),
    "tw_collected_copy_to_host": (C.c_int, [_VP, C.c_int, _VP, C.c_size_t]),
    "tw_collected_stats": (C.c_int, [_VP, C.POINTER(CollectStats)]),
    "tw_collected_free": (None, [_VP]),
    "tw_collected_pack_trainer": (C.c_int, [_VP, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, _VP, _VP, _VP, _VP, _VP]),
    "tw_collected_adv_stats": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "tw_comm_get_unique_id": (C.c_int, [C.POINTER(CommId)]),
    "tw_comm_init": (C.c_int, [C.c_int, C.c_int, C.POINTER(CommId), C.POINTER(_VP)]),
    "tw_comm_destroy": (None, [_VP]),
    "tw_comm_rank": (C.c_int, [_VP]),
    "tw_comm_world": (C.c_int, [_VP]),
    "tw_comm_broadcast_policy": (C.c_int, [_VP, _VP, C.c_int]),
    "tw_comm_set_timeout_ms": (C.c_int, [_VP, C.c_uint32]),
    "tw_gather_plan": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _VP]),
    "tw_gather_begin": (C.c_int, [_VP, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(_VP)]),
    "tw_gather_submit": (C.c_int, [_VP, _VP, C.c_uint64]),
    "tw_gather_finish": (C.c_int, [_VP, C.POINTER(_VP)]),
}

_lib = None


def library_path() -> str:
    return _build.LIB_PATH


def lib():
    """Load (building first if needed) libtwisterl_hip.so and declare every prototype."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm bundles its own HIP runtime under the same soname as /opt/rocm's.  Whichever is loaded first
        # serves the whole process, and torch fails to initialise ("No HIP GPUs are available") when it finds the
        # other one already loaded: load torch's first, this library then binds to it as well.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = _build.LIB_PATH
        if not os.path.exists(path) or os.environ.get("TWISTERL_AMD_REBUILD"):
            path = _build.build_library()
        try:
            L = C.CDLL(path)
        except OSError as e:  # loud: no CPU fallback exists
            raise RuntimeError(f"cannot load the HIP collector library {path}: {e}") from e
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.tw_abi_version() != ABI_VERSION:
            raise RuntimeError("libtwisterl_hip.so ABI version mismatch; rebuild with python -m twisterl_amd.build")
        _lib = L
    return _lib


def last_error() -> str:
    msg = lib().tw_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status: int) -> None:
    """Status-code -> exception, following the reference's convention: anyhow::Error ->
    PyRuntimeError (python_interface/error_mapping.rs:20-33); bad arguments -> ValueError."""
    if status == TW_OK:
        return
    msg = last_error()
    if status == TW_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


class launch_option:
    """`with launch_option(TW_OPT_NO_PERSIST, 1): ...` -- pins a diagnostic launch override (tw_set_launch_option) for
    the block; the parity tests use it to show that every launch shape gives the same bytes."""

    def __init__(self, option: int, value: int):
        self.option, self.value = option, value

    def __enter__(self):
        check(lib().tw_set_launch_option(self.option, self.value))
        return self

    def __exit__(self, *exc):
        check(lib().tw_set_launch_option(self.option, 0))
        return False


class debug_fill_memory:
    """`with debug_fill_memory(0xFFFFFFFF): ...` -- while the block runs, every device buffer the library hands to a call (the cached
    workspace, a result arena, a call-local scratch allocation) is set to the 32-bit pattern before its first use
    (tw_debug_fill_memory; test hook).  Leaving the block turns the hook off, whatever happened inside: no result may depend on what
    device memory held before a call, and tests/test_gpu_memory_matrix.py shows it pattern by pattern."""

    _state = None          # (on, pattern) as the library holds it; None: not asked yet (TW_DEBUG_FILL gives the initial value)

    def __init__(self, pattern: int):
        if not 0 <= pattern <= 0xFFFFFFFF:
            raise ValueError(f"debug_fill_memory: pattern {pattern:#x} is not a 32-bit word")
        self.pattern = pattern

    @classmethod
    def _current(cls):
        if cls._state is None:
            try:
                cls._state = (1, int(os.environ["TW_DEBUG_FILL"], 16))
            except (KeyError, ValueError):
                cls._state = (0, 0)
            if not 0 <= cls._state[1] <= 0xFFFFFFFF:
                cls._state = (0, 0)
        return cls._state

    @classmethod
    def _set(cls, state):
        check(lib().tw_debug_fill_memory(*state))
        cls._state = state

    def __enter__(self):
        self.before = self._current()
        self._set((1, self.pattern))
        return self

    def __exit__(self, *exc):
        self._set(self.before)          # (off, unless TW_DEBUG_FILL or an enclosing block had it on)
        return False


class library_stream:
    """`with library_stream(torch.cuda.Stream()): ...` -- while the block runs, the library calls of THE CALLING THREAD launch on the
    given stream (tw_set_stream with the stream's raw handle, its `.cuda_stream`; None or 0: the null stream).  Leaving the block puts
    the null stream back, whatever happened inside.  The setting is thread-local in the library: another thread's calls stay on the
    stream that thread set (the null stream if it never set one), and a block entered on one thread must be left on the same thread.
    Blocks do not nest (the library has no getter: the exit restores the null stream, not an enclosing block's stream).  A result
    produced inside the block may be read, handed over and freed outside it, by any thread: every collect, evaluate and solve returns
    after its stream has finished, and tw_collected_free fences the producing stream ("Threads and streams").
    torch's own current stream is not changed: use `torch.cuda.stream(s)` for that."""

    def __init__(self, stream):
        handle = 0 if stream is None else getattr(stream, "cuda_stream", stream)
        if not isinstance(handle, int) or handle < 0:
            raise TypeError("library_stream: a torch.cuda.Stream (or a raw hipStream_t as an int) expected")
        self.stream, self.handle = stream, handle       # (the stream object is kept alive for the block)

    def __enter__(self):
        check(lib().tw_set_stream(C.c_void_p(self.handle)))
        return self

    def __exit__(self, *exc):
        check(lib().tw_set_stream(None))
        return False


def debug_counters(n: int = 16) -> list:
    """Diagnostic counters of this process's last self-play launch (tw_debug_counters); after an f32 PPO collect: [0] the episodes
    the persistent 256-episode launch handed over, [1] the workgroups of the drain launch (TW_OPT_ROLLOUT_DRAIN), the rest 0."""
    buf = (C.c_uint64 * n)()
    check(lib().tw_debug_counters(buf, n))
    return [int(x) for x in buf]


def debug_last_launch() -> dict:
    """The kernel the last self-play / evaluate / solve / big-board PPO / one-hot hand-off call of this process launched, as its launcher
    reported it (tw_debug_last_launch; test hook): family (TW_KERNEL_*), template arguments, grid, and the engine kernel's grid of the
    split shape.  TW_KERNEL_ONEHOT: nt = 4 / 1 / 0 / 2 for onehot4_kernel / onehot_kernel / memset + onehot_scatter_kernel / the same on
    two-byte ids, nc = the rows a workgroup writes per trip of its loop."""
    info = LaunchInfo()
    check(lib().tw_debug_last_launch(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in LaunchInfo._fields_}


def debug_last_attempts():
    """(success, total, n_steps) of every attempt of the last evaluate / solve that ran on the device, attempt a of episode e at
    e * num_searches + a (tw_debug_last_attempts; test hook)."""
    import numpy as np
    n = C.c_uint64()
    check(lib().tw_debug_last_attempts(None, None, None, 0, C.byref(n)))
    s, t, k = np.zeros(n.value, np.float32), np.zeros(n.value, np.float32), np.zeros(n.value, np.uint32)
    check(lib().tw_debug_last_attempts(s.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_float)),
                                       k.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
    return s, t, k


def debug_episode_order(desc, seed: int, episode_offset: int, n: int):
    """Start boards (uint64, nibble i = tile at cell i) of n Puzzle episodes and the order in which the self-play walkers take them
    (tw_debug_episode_order; test hook).  `desc`: a PuzzleDesc."""
    import numpy as np
    boards = np.zeros(n, dtype=np.uint64); order = np.zeros(n, dtype=np.uint32)
    check(lib().tw_debug_episode_order(C.byref(desc), seed, episode_offset, n, boards.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       order.ctypes.data_as(C.POINTER(C.c_uint32))))
    return boards, order


def debug_policy_image(policy):
    """(image, ptr_ranges) of a twisterl_amd.nn.Policy (tw_debug_policy_image; test hook): its device image as a uint8 array, read
    once the library's stream has finished, and the (offset, length) byte ranges of it that hold device pointers -- the layer table
    of a stack of any depth; none for the one-common-layer shape."""
    import numpy as np
    h = policy._handle()
    size, n = C.c_uint64(), C.c_uint32()
    check(lib().tw_debug_policy_image(h, None, 0, C.byref(size), None, 0, C.byref(n)))
    img, ranges = np.zeros(size.value, dtype=np.uint8), np.zeros((max(n.value, 1), 2), dtype=np.uint64)
    check(lib().tw_debug_policy_image(h, img.ctypes.data_as(C.c_void_p), size.value, C.byref(size), ranges.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      n.value, C.byref(n)))
    return img, [(int(o), int(b)) for o, b in ranges[:n.value]]


def debug_scan(ep_len, merge_order: bool):
    """(ep_start, total) of the collectors' episode-length scan over any uint32 lengths (tw_debug_collect_tail in scan-only mode; test
    hook): ep_start[e] = the lengths in front of episode e in the output order, as uint64; total as a Python int."""
    import numpy as np
    ep_len = np.ascontiguousarray(ep_len, dtype=np.uint32)
    ep_start, total = np.zeros(ep_len.size, dtype=np.uint64), C.c_uint64()
    a = DebugTailArgs(n_episodes=ep_len.size, merge_order=int(bool(merge_order)), scan_only=1, ep_len=ep_len.ctypes.data,
                      ep_start_out=ep_start.ctypes.data, total_out=C.addressof(total))
    check(lib().tw_debug_collect_tail(C.byref(a), None, None))
    return ep_start, int(total.value)


def debug_collect_tail(ep_len, records, t_pad: int, *, is_ppo: bool, n_cells: int, n_actions: int, obs16=None, obs_width: int = 1, wide=None,
                       gamma: float = 0.0, lam: float = 0.0, merge_order: bool = False, arena_fill: int = 0):
    """The tail of every device collector on records the caller wrote (tw_debug_collect_tail; test hook) -> (handle, launch):
    a tw_collected handle (debug_collected_fields / debug_collected_arena; free it with lib().tw_collected_free) and the finalize
    kernel that was launched as a dict of FinalizeLaunch's fields.  records: [E][t_pad] records of 48 bytes (any array of that many
    bytes); obs16: uint16 [E][t_pad][n_cells] or None; wide: float32 [E][t_pad][n_actions] for more than four actions."""
    import numpy as np
    ep_len = np.ascontiguousarray(ep_len, dtype=np.uint32)
    records = np.ascontiguousarray(records)
    if records.nbytes != ep_len.size * t_pad * 48:
        raise ValueError(f"debug_collect_tail: {records.nbytes} bytes of records, {ep_len.size} x {t_pad} x 48 expected")
    if obs16 is not None:
        obs16 = np.ascontiguousarray(obs16, dtype=np.uint16)
        if obs16.size != ep_len.size * t_pad * n_cells:
            raise ValueError("debug_collect_tail: obs16 is not [E][t_pad][n_cells]")
    if wide is not None:
        wide = np.ascontiguousarray(wide, dtype=np.float32)
        if wide.size != ep_len.size * t_pad * n_actions:
            raise ValueError("debug_collect_tail: wide is not [E][t_pad][n_actions]")
    a = DebugTailArgs(n_episodes=ep_len.size, t_pad=t_pad, is_ppo=int(bool(is_ppo)), n_cells=n_cells, n_actions=n_actions, obs_width=obs_width,
                      merge_order=int(bool(merge_order)), scan_only=0, arena_fill=arena_fill, gamma=gamma, lambda_=lam,
                      ep_len=ep_len.ctypes.data, records=records.ctypes.data, obs16=None if obs16 is None else obs16.ctypes.data,
                      wide=None if wide is None else wide.ctypes.data)
    launch, handle = FinalizeLaunch(), _VP()
    check(lib().tw_debug_collect_tail(C.byref(a), C.byref(launch), C.byref(handle)))
    return handle, {name: int(getattr(launch, name)) for name, _ in FinalizeLaunch._fields_}


def debug_collected_arena(handle):
    """(arena, offsets, scratch) of a tw_collected handle (tw_debug_collected_arena; test hook): every byte of its arena as a uint8
    array, the offset of each field TW_F_* in it, and (offset, bytes) of the four-column logits scratch behind the fields."""
    import numpy as np
    size, offs, scratch = C.c_uint64(), (C.c_uint64 * TW_F_COUNT)(), (C.c_uint64 * 2)()
    check(lib().tw_debug_collected_arena(handle, None, 0, C.byref(size), offs, scratch))
    arena = np.zeros(size.value, dtype=np.uint8)
    check(lib().tw_debug_collected_arena(handle, arena.ctypes.data_as(C.c_void_p), size.value, C.byref(size), offs, scratch))
    return arena, [int(x) for x in offs], (int(scratch[0]), int(scratch[1]))


def release_cached_memory() -> None:
    """Gives the library's cached device memory (trajectory workspace, pooled result arenas) back to the driver -- e.g. before
    the trainer needs the GPU's memory for itself, or after a torch out-of-memory error (torch's allocator cannot see it)."""
    check(lib().tw_release_cached_memory())


def device_count() -> int:
    return int(lib().tw_device_count())


def device_info() -> dict:
    info = DeviceInfo()
    check(lib().tw_get_device_info(C.byref(info)))
    return {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units,
            "wavefront_size": info.wavefront_size, "total_mem_bytes": info.total_mem_bytes,
            "lds_bytes_per_block": info.lds_bytes_per_block}
