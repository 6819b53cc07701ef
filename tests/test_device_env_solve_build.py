"""CPU: solve() of a device environment on the device (tw_solve_device_env).  The entry point is declared, exported and bound; a module
built against the EnvSolveArgs of before (without from_state's action rows) is refused with the rebuild message; without a GPU the
call raises and never falls back; and every case of tests/test_gpu_device_env_solve.py ends within max_records under the oracle and
contains what it is about, so that test cannot pass for lack of cases.  (Kernel counts, the name census, the pinned scratch sizes and
the MFMA scan of the modules are the existing build tests', unchanged.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import device_env_solve as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what EnvSolveArgs gained: uint8_t *actions, uint32_t actions_stride and the tail padding of an 8-byte aligned struct
NEW_MEMBER_BYTES = C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_uint32)


@pytest.fixture()
def det_exp(oracle):
    oracle.set_det_exp(True)
    yield oracle
    oracle.set_det_exp(False)


def test_the_entry_point_is_declared_exported_and_bound():
    from twisterl_amd import _lib
    header = open(os.path.join(ROOT, "include", "twisterl_hip.h")).read()
    assert re.search(r"int tw_solve_device_env\(const tw_device_env \*env, const void \*proto, size_t proto_bytes, const tw_policy \*policy,", header)
    assert "tw_solve_device_env" in _lib.SYMBOLS and len(_lib.SYMBOLS["tw_solve_device_env"][1]) == 11
    assert _lib.SYMBOLS["tw_solve_device_env"][1][4:] == _lib.SYMBOLS["tw_solve_env32"][1][2:]      # the contract of tw_solve_env32
    assert getattr(_lib.lib(), "tw_solve_device_env") is not None
    assert _lib.lib().tw_abi_version() == 6
    assert "fn tw_solve_device_env(" in open(os.path.join(ROOT, "docs", "hip.rs")).read()


def test_a_module_of_the_old_layout_is_refused_with_the_rebuild_message():
    from twisterl_amd import _lib
    from twisterl_amd.env import DeviceEnvDesc
    env = D.gridworld_case(2)[0]
    old = DeviceEnvDesc()
    C.memmove(C.byref(old), env._desc_ptr, C.sizeof(DeviceEnvDesc))
    old.layout[5] -= NEW_MEMBER_BYTES
    prm = _lib.SolveParams(1, 1, 0, D.C_UCB, 1, D.SEED, _lib.TW_PREC_F32_EXACT)
    s, r, n = C.c_float(), C.c_float(), C.c_uint32()
    acts = (C.c_uint32 * 16)()
    _, proto, nbytes = env._args()
    no_policy = C.create_string_buffer(64)        # (never read: the descriptor is checked first, and a policy needs a device)
    rc = _lib.lib().tw_solve_device_env(C.byref(old), proto, nbytes, C.addressof(no_policy), C.byref(prm), env.max_records, C.byref(s), C.byref(r), acts, 16,
                                        C.byref(n))
    assert rc != _lib.TW_OK
    msg = _lib.last_error()
    assert "tw_solve_device_env" in msg and "another library layout" in msg and "rebuild it" in msg, msg


@pytest.mark.parametrize("search", [False, True])
def test_without_a_gpu_solve_raises(search):
    import twisterl_amd
    from twisterl_amd import twisterl
    if twisterl_amd.device_count() > 0:
        pytest.skip("GPU present")                # (tests/test_gpu_device_env_solve.py runs the call)
    case = D.gridworld_case(2, search=search)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback"):         # (the policy upload is the first thing that needs it)
        twisterl.collector.solve(case[0], D.lib_policy(case), True, 3, D.MCTS_S if search else 0, D.C_UCB, 1, seed=D.SEED)


def _ends(env, result):
    assert len(result[1]) <= env.max_records, (len(result[1]), env.max_records)
    exact, success, total = D.replay(env, result[1])
    assert exact and float(success) == result[0][0] and np.float32(total) == np.float32(result[0][1])


def test_the_plain_cases_end_within_max_records(det_exp):
    cases = [D.gridworld_case(0), D.gridworld_case(2), D.ring_case(), D.lamps_case(), D.probe_case("probe_o64a4s"), D.big_puzzle_case(), D.mfma_case()]
    for case in cases:
        env, op = case[0], D.oracle_policy(case)
        assert not env.is_final()
        for det in (True, False):
            for N in (1, 17):
                _ends(env, D.oracle_solve(det_exp, env, op, det, N))
    case = D.gridworld_case(2)
    env, op = case[0], D.oracle_policy(case)
    _ends(env, D.oracle_solve(det_exp, env, op, False, 40))
    case = D.big_puzzle_case()
    env, op = case[0], D.oracle_policy(case)
    assert env.n_obs == 9 and int(env._desc.n_obs) == 25
    case = D.lamps_case()
    env, op = case[0], D.oracle_policy(case)
    assert env.variable_obs
    case = D.probe_case("probe_o64a4s")
    env, op = case[0], D.oracle_policy(case)
    assert int(env._desc.state_bytes) == 1024
    case = D.final_case()
    env, op = case[0], D.oracle_policy(case)
    assert env.is_final() and D.oracle_solve(det_exp, env, op, True, 17) == ((float(env.success()), env.reward()), [])


def test_the_best_of_n_case_has_a_best_that_is_not_the_first(det_exp):
    case = D.gridworld_case(2)
    env, op = case[0], D.oracle_policy(case)
    att = D.oracle_attempts(det_exp, env, op, False, **D.BEST_OF_N)
    keys = [a[0] for a in att]
    best = max(range(len(keys)), key=lambda i: (keys[i], -i))
    assert best > 0 and keys[best] > keys[0] and len(set(keys)) > 2, keys
    assert D.same(D.oracle_solve(det_exp, env, op, False, D.BEST_OF_N["N"], seed=D.BEST_OF_N["seed"]), att[best])


@pytest.mark.parametrize("module", sorted(D.WIDE_SEEDS))
def test_the_wide_cases_play_an_action_beyond_the_fourth(det_exp, module):
    case = D.wide_case(module)
    env, op = case[0], D.oracle_policy(case)
    r = D.oracle_solve(det_exp, env, op, False, D.WIDE_N, seed=D.WIDE_SEEDS[module][1])
    _ends(env, r)
    assert max(r[1]) >= 4 and (module != "wideo64a31" or 30 in r[1]), r


def test_the_mcts_cases_end_within_max_records(det_exp):
    from tests.device_env_wide_search import IDS
    cases = [D.gridworld_case(2, search=True), D.ring_case(search=True)] + [D.wide_search_case(m) for m in IDS]
    for case in cases:
        env, op = case[0], D.oracle_policy(case)
        assert not env.is_final() and env.search
        for med in (1, 2):
            _ends(env, D.oracle_solve(det_exp, env, op, False, 3, D.MCTS_S, med))
        _ends(env, D.oracle_solve(det_exp, env, op, True, 1, D.MCTS_S, 1))


def test_the_too_short_case_needs_one_step_more(det_exp):
    case = D.gridworld_case(2)
    env, op = case[0], D.oracle_policy(case)
    r = D.oracle_solve(det_exp, env, op, True, 1)
    assert len(r[1]) >= 2 and D.TOO_SHORT_STEPS == len(r[1])
