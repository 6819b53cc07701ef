"""CPU: tests/memory_matrix.py against the sources and against itself.

* Census: `seg(` in the call carves of twisterl_amd/csrc (tw_api.hip behind its two policy-image builders) and `hipMalloc(`, counted per
  file, equal the numbers the table declares -- a pull request that adds a workspace segment or a raw allocation has to touch the
  table, as a new kernel has to come to tests/search_matrix.py.  The scan looks for these two words and nothing else.
* Coverage: every condition of every carve is turned on by at least one case and left off by at least one case of the same carve, and
  every segment a carve names belongs either to no condition (always there) or to exactly one.
* The cases that point to a row of tests/kernel_matrix.py / tests/search_matrix.py: the restated dispatch of that row agrees with the
  conditions the case claims (persistent, walker kernel, decoupled, split, big board, generic stack), at 256 compute units; the three
  rows no table has land on the kernels the table says.
* The hook's Python side: debug_fill_memory refuses a pattern that is no 32-bit word, and the header, _lib.py and docs/hip.rs name it.
"""
import glob
import os

import pytest

from tests import kernel_matrix as km
from tests import memory_matrix as mm
from tests import search_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twisterl_amd", "csrc")
CUS = 256


def count_words(csrc=CSRC):
    """-> ({file: `seg(` in its call carves}, {file: `hipMalloc(`}) over every file of `csrc`, files without either left out."""
    segs, mallocs = {}, {}
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        name, text = os.path.basename(path), open(path, errors="ignore").read()
        carves = text[text.index(mm.POLICY_IMAGE_MARK):] if name == "tw_api.hip" else text
        if carves.count("seg("):
            segs[name] = carves.count("seg(")
        if text.count("hipMalloc("):
            mallocs[name] = text.count("hipMalloc(")
    return segs, mallocs


def test_census_of_workspace_segments_and_raw_allocations():
    segs, mallocs = count_words()
    assert segs == mm.SEG_COUNTS, (segs, mm.SEG_COUNTS)
    assert mallocs == mm.MALLOC_COUNTS, (mallocs, mm.MALLOC_COUNTS)
    assert mm.SEG_COUNTS == {"tw_api.hip": 42, "tw_device_env.hip": 23, "tw_comm.hip": 5}


def test_census_notices_an_added_segment_and_an_added_allocation(tmp_path):
    """A copy of the sources with one more `seg(` in a carve, and one with one more raw hipMalloc: the counts move off the table's."""
    import shutil
    for name, old, new in (("tw_device_env.hip", "o_act = seg((size_t)NA * stride);", "o_act = seg((size_t)NA * stride), o_more = seg(64);"),
                           ("tw_env_generic.hip", "hipStream_t s = current_stream();", "hipStream_t s = current_stream(); void *q = nullptr; (void)hipMalloc(&q, 64);")):
        dst = tmp_path / name.replace(".", "_")
        shutil.copytree(CSRC, dst)
        text = (dst / name).read_text()
        assert old in text, (name, old)
        (dst / name).write_text(text.replace(old, new, 1))
        segs, mallocs = count_words(str(dst))
        assert (segs, mallocs) != (mm.SEG_COUNTS, mm.MALLOC_COUNTS), name
        assert (segs != mm.SEG_COUNTS) == (name == "tw_device_env.hip") and (mallocs != mm.MALLOC_COUNTS) == (name == "tw_env_generic.hip")


def test_every_condition_has_a_case_on_each_side():
    carves = {c for f in mm.SEGMENTS.values() for c in f}
    for carve, conds in mm.CONDITIONS.items():
        cases = [c for c in mm.CASES if c.carve == carve]
        assert cases, carve
        for cond in conds:
            on = [c.id for c in cases if cond in c.on]
            off = [c.id for c in cases if cond not in c.on]
            assert on and off, (carve, cond, on, off)
        for c in cases:
            assert c.on <= set(conds), (c.id, c.on - set(conds))
    assert {c.carve for c in mm.CASES} == set(mm.CONDITIONS)
    # every carve that takes workspace has its cases; the gather arena is filled by the hook and run by tests/test_gpu_multirank.py alone
    assert carves - set(mm.CONDITIONS) == {"gather_alloc"}
    assert len(set(mm.IDS)) == len(mm.IDS)


def test_conditional_segments_belong_to_one_condition_of_their_carve():
    by_carve = {c: names for f in mm.SEGMENTS.values() for c, names in f.items()}
    for carve, conds in mm.CONDITIONS.items():
        if carve not in by_carve:
            continue
        seen = []
        for cond, segs in conds.items():
            for s in segs:
                if not s.startswith("("):
                    assert s in by_carve[carve], (carve, cond, s)
                    seen.append(s)
        assert len(seen) == len(set(seen)), (carve, seen)


def _az_conditions(row):
    kernel, _, engine = sm.dispatch(row, CUS)
    on = set()
    if kernel[0] == "mcts_big":
        return {"big"}
    if kernel[0] == "deep":
        on |= {"persist", "deep"}
        if kernel[6]:
            on.add("decoupled")
        if kernel[7]:
            on.add("split")
            assert engine is not None
    elif kernel[0] == "mcts" and kernel[4]:
        on.add("persist")
    return on


@pytest.mark.parametrize("case", [c for c in mm.CASES if c.family in ("km", "sm_az", "sm_eval", "sm_ppo")], ids=lambda c: c.id)
def test_the_rows_dispatch_agrees_with_the_conditions_the_case_claims(case):
    row = mm.row_of(case)
    if case.family == "km":
        kernel, _ = km.dispatch(row, CUS)
        assert kernel[-1] == ("persist" in case.on), (case.id, kernel)
        assert (row.common is not None) == ("generic" in case.on) and (row.prec == "fp16") == ("fp16" in case.on)
        assert (row.prec == "fp16x2") == ("range_flag" in case.on) and (row.prec == "fp32" and row.common is None) == ("reuse_words" in case.on)
        assert (kernel[:1] == ("f32",) and kernel[3] == 8) == ("reuse_rounds" in case.on), (case.id, kernel)
    elif case.family == "sm_ppo":
        assert sm.dispatch(row, CUS)[0][0] == "rollout_big" and {"big", "generic"} == set(case.on)
    elif case.family == "sm_az":
        assert _az_conditions(row) == set(case.on) - {"deep_tree"}, (case.id, sm.dispatch(row, CUS)[0])
    else:
        kernel = sm.dispatch(row, CUS)[0]
        solve = row.entry == "solve"
        want = set()
        if solve:
            want.add("want_actions")
        if row.S:
            want.add("mcts")
        if kernel[0] == "deep":
            want.add("deep")
            if not solve:
                want.add("deep_boards")
        if solve and row.w * row.h > 16:
            want.add("big_state")
        if row.det:
            want.add("deterministic")
        assert want == set(case.on), (case.id, kernel, want)


def test_the_rows_no_table_has_land_on_the_kernels_the_table_says():
    for name, (row, kernel) in mm.EXTRA_ROWS.items():
        assert row not in sm.TABLE and sm.kernel_name(sm.dispatch(row, CUS)[0]) == kernel, name
    # 2,048 episodes are 8 per compute unit: the fewest that take the split shape with no compute unit reserved, at any number of searches
    # below 16 (mcts_deep_applies: up to 8 episodes per CU); one episode fewer is the decoupled shape inside one workgroup
    fewer = mm.SPLIT_2048._replace(E=2047)
    assert not sm.dispatch(fewer, CUS)[0][7] and sm.dispatch(mm.SPLIT_2048, CUS)[0][7]


def test_the_hook_is_declared_bound_and_mirrored():
    from twisterl_amd import _lib
    header = open(os.path.join(ROOT, "include", "twisterl_hip.h")).read()
    rs = open(os.path.join(ROOT, "docs", "hip.rs")).read()
    assert "int tw_debug_fill_memory(int on, uint32_t pattern);" in header and "fn tw_debug_fill_memory(on: c_int, pattern: u32) -> c_int;" in rs
    assert "tw_debug_fill_memory" in _lib.SYMBOLS and mm.PATTERNS == (0xFFFFFFFF, 0x00000001, 0x00000000)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            _lib.debug_fill_memory(bad)
    # the state is process-wide and off unless TW_DEBUG_FILL says otherwise; the context manager puts back what it found (needs no device)
    before = _lib.debug_fill_memory._current()
    with _lib.debug_fill_memory(0x00000001):
        assert _lib.debug_fill_memory._current() == (1, 1)
        with _lib.debug_fill_memory(0xFFFFFFFF):
            assert _lib.debug_fill_memory._current() == (1, 0xFFFFFFFF)
        assert _lib.debug_fill_memory._current() == (1, 1)
    assert _lib.debug_fill_memory._current() == before
