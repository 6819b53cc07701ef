"""CPU: the device-environment matrix (tests/device_env_matrix.py) against the built modules and the oracle's data.  Every row's
module of the probe struct (tests/device_envs/probe.hpp) builds for gfx950 without an MFMA hazard, holds the two or three kernels of
the EngineV class its N_OBS selects and reports the row in its descriptor; the table covers the contract (every class for every
kernel, both sides of every class edge, every NUM_ACTIONS, both struct-size limits, the obs_size edges); the scratch rows really
compile to scratch memory and the K = 1 rows to none; and the oracle's collects at the GPU test's episode counts and seeds contain
what that test is about."""
import os
import re

import numpy as np
import pytest

from tests.device_env_matrix import (BY_MODULE, CLASSES, EPISODES, ERROR_ROWS, HANDOFF_ROWS, IDS, TABLE, build_all, engine_nc, probe,
                                     reset_is_final, shared_collect)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("rollout_env_kernel", "solve_env_kernel", "mcts_env_kernel")


def _scan(path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    return scan.scan_file(path)


def _asm(module):
    so = build_all()[module]
    assert os.path.exists(so) and os.path.exists(so[:-3] + ".s")
    return so[:-3] + ".s", open(so[:-3] + ".s").read()


def _scratch_sizes(text):
    """{kernel: .private_segment_fixed_size} from the module's metadata."""
    out = {}
    for name, size in re.findall(r"\.name:\s+(\S+)\s+\.private_segment_fixed_size:\s+(\d+)", text):
        out[next(k for k in KERNELS if k in name)] = int(size)
    return out


@pytest.mark.parametrize("module", IDS)
def test_module_builds_clean_and_holds_the_kernels_of_its_class(module):
    r = BY_MODULE[module]
    path, text = _asm(module)
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    want = KERNELS if r.search else KERNELS[:2]
    assert len(kernels) == len(want), kernels
    nc = engine_nc(r.n_obs)
    for k in want:                                        # kernel<Env, NC>: the mangled name ends in the column count
        assert sum(1 for n in kernels if re.search(rf"{k}I.*Li{nc}EEEvNS_", n)) == 1, (k, nc, kernels)
    hits, counts = _scan(path)
    assert hits == [] and sum(counts.values()) > 0
    assert "gfx950" in text
    form = "TW_DEVICE_ENV_SEARCH(" if r.search else "TW_DEVICE_ENV("
    assert form + r.alias in open(path[:-2] + ".hip").read()


@pytest.mark.parametrize("module", IDS)
def test_descriptor_reports_the_row(module):
    r = BY_MODULE[module]
    env = probe(r)
    d = env._desc
    assert (int(d.num_actions), int(d.n_obs), int(d.state_bytes), int(d.engine_nc)) == (r.A, r.n_obs, r.state_bytes, engine_nc(r.n_obs))
    assert env.search is r.search and env.variable_obs is r.var and env.obs_size == r.obs_size and env.n_obs == r.n_obs
    assert env.max_records == r.max_steps + 1 and len(env.state_bytes()) == r.state_bytes


def test_the_table_covers_the_contract():
    for k, rows in (("rollout", TABLE), ("solve", TABLE), ("search", [r for r in TABLE if r.search])):
        assert {engine_nc(r.n_obs) for r in rows} == set(CLASSES), k              # every EngineV class, for every kernel
        assert {r.A for r in rows} == {1, 2, 3, 4}, k                              # every NUM_ACTIONS, for every kernel
    n_obs = {r.n_obs for r in TABLE}
    assert {1, 64} <= n_obs
    for lo in CLASSES[:-1]:                                                         # both sides of every class edge
        assert {lo, lo + 1} <= n_obs and engine_nc(lo) == lo and engine_nc(lo + 1) > lo, lo
    assert {1024, 128} <= {r.state_bytes for r in TABLE}
    assert all(r.state_bytes <= (128 if r.search else 1024) for r in TABLE)
    assert {1, 256, 257, 65535} <= {r.obs_size for r in TABLE}
    assert {0, 2, 3} <= {r.twists for r in TABLE}
    assert {True, False} == {r.var for r in TABLE} and any(r.var and r.search for r in TABLE)
    # policies: one and two common layers; a row with policy_layers AND value_layers (the other head path of EngineV::forward)
    assert {1, 2} <= {len(r.common) for r in TABLE} and any(r.policy_layers and r.value_layers for r in TABLE)
    assert all(r.emb in (32, 64) for r in TABLE)
    assert all(r.max_steps <= 12 for r in TABLE) and sum(1 for r in TABLE if r.offset) >= 2
    assert len(set(IDS)) == len(IDS) == len({r.alias for r in TABLE})
    scratch = [r for r in TABLE if r.scratch]
    assert len(scratch) == 3 and {r.state_bytes for r in scratch} == {128, 1024} and any(r.var for r in scratch)
    assert any(BY_MODULE[m].scratch for m in ERROR_ROWS) and any(BY_MODULE[m].A == 1 for m in ERROR_ROWS)
    assert all(not BY_MODULE[m].var for m in ERROR_ROWS)
    assert [BY_MODULE[m].obs_size for m in HANDOFF_ROWS] == [256, 257, 65535]
    alias_text = open(os.path.join(ROOT, "tests", "device_envs", "probe.hpp")).read()
    for r in TABLE:
        assert re.search(rf"using {r.alias}\s+= Probe<{r.n_obs}, {r.A}, {r.K}, {'true' if r.var else 'false'}>;", alias_text), r.alias


@pytest.mark.parametrize("module", IDS)
def test_scratch_rows_leave_the_registers_and_k1_rows_do_not(module):
    """A struct whose array is indexed at run time compiles to scratch memory: the three scratch rows have a non-zero
    .private_segment_fixed_size in EVERY kernel they hold -- if a later compiler keeps hist in registers, this fails instead of the
    GPU test silently losing its point.  The K = 1 rows use none."""
    r = BY_MODULE[module]
    sizes = _scratch_sizes(_asm(module)[1])
    assert sorted(sizes) == sorted(KERNELS if r.search else KERNELS[:2]), sizes
    if r.scratch:
        assert all(v >= r.state_bytes for v in sizes.values()), sizes          # (at least the struct itself)
    elif r.K == 1:
        assert all(v == 0 for v in sizes.values()), sizes


def _allowed(o):
    return (o.logits > np.float32(-1e9)).sum(axis=1)


@pytest.mark.parametrize("E", EPISODES)
@pytest.mark.parametrize("module", IDS)
def test_the_shared_collect_contains_what_the_gpu_test_is_about(module, E):
    """The input conditions, on the oracle's data (the struct's own host code under the oracle's PPO loop), at the episode counts,
    seeds and offsets of the GPU test."""
    r = BY_MODULE[module]
    o = shared_collect(module, E)
    lens = o.ep_len.tolist()
    assert len(lens) == E and int(o.ep_len.sum()) == len(o.obs_lists) == o.obs.shape[0] and o.obs.shape[1] == r.n_obs
    assert len(set(lens)) >= 3, sorted(set(lens))
    assert 1 in lens, "no episode of one record (final at reset)"
    assert r.max_steps + 1 in lens and max(lens) == r.max_steps + 1, "no episode that reaches max_steps"
    assert set(o.actions.tolist()) == set(range(r.A)), "an action is never taken"
    n_allowed = _allowed(o)
    assert int(n_allowed.min()) >= 1
    if r.A >= 2:
        assert (n_allowed == 1).any() and (n_allowed == r.A).any(), "no record with exactly one allowed action"
    ids = [i for rec in o.obs_lists for i in rec]
    assert all(0 <= i < r.obs_size for i in ids)
    if r.var:
        assert int(o.counts.min()) == 0 and int(o.counts.max()) == r.n_obs, (int(o.counts.min()), int(o.counts.max()))
    else:
        assert set(o.counts.tolist()) == {r.n_obs}
    if r.obs_size == 256:
        assert 255 in ids, "the id 255 does not occur"
    if r.obs_size == 65535:
        assert max(ids) >= 32768, "no id with the top bit of its two bytes set"
    if r.twists:
        assert set(o.perms.tolist()) == set(range(r.twists))
    else:
        assert set(o.perms.tolist()) == {-1}


@pytest.mark.parametrize("module", IDS)
def test_evaluate_meets_a_final_reset_state(module):
    """evaluate's attempts (40 episodes) include one whose reset state is final (`alive = !st.is_final()` of solve_env_kernel, the
    EP_DONE line of the search kernel) and one whose is not."""
    fin = reset_is_final(module, 40)
    assert any(fin) and not all(fin), fin
