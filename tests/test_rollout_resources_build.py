"""CPU: compile-time resources of every rollout_f32_kernel instantiation, and the lane moves in the step loop of the 256-episode shape.

The f32-input MFMA runs on the SIMD's f32 FMA lanes, so no vector instruction hides under it: a scalar that lives
across the forward in a lane of a spill VGPR costs vector-ALU time at every v_readlane_b32 / v_writelane_b32 that moves it.  The
256-episode shape therefore reads its launch constants from the kernarg segment where it uses them (tw_rollout.hip: kernarg_view).
Checked on the assembly the library was built from (twisterl_amd/lib/asm/tw_rollout.s: the library's flags; the figures in its
kernel descriptors are those of -Rpass-analysis=kernel-resource-usage), against the figures of the parent commit,
tests/golden/rollout_f32_resources_e5f53c9.json:

  * every instantiation: VGPRs, scratch, SGPR spills and VGPR spills no higher, occupancy no lower than the parent's; the shapes
    with NW != 8 exactly the parent's;
  * <8, 16, 8, true> (the benchmark's kernel): no scratch, no VGPR spill, at most 256 VGPRs, occupancy 2, at most half the parent's
    120 SGPR spills; <8, 16, 8, false>: scratch <= 64, VGPR spills <= 15;
  * <8, 16, 8, true> and <8, 9, 8, true>: v_readlane_b32 + v_writelane_b32 inside the step loop at most half the parent's, and no
    basic block of the loop parks scalars wholesale (fewer than 16 v_writelane_b32 in any one of them).

The step loop is the outermost loop that holds MFMAs: from the target of the longest backward branch around a v_mfma to that branch,
extended over the blocks laid out behind it that branch back into it (the fast-forward rounds).  Counted that way the parent
(e5f53c9) has 208 v_readlane_b32 and no v_writelane_b32 in the loop of <8, 16, 8, true> and 149 / 0 in <8, 9, 8, true>; its 83
v_writelane_b32 sit in the loop's preheader.  (DPP reductions of __syncthreads_count read two lanes as well; they are in both counts.)
"""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout_f32_resources_e5f53c9.json")
PARENT_LANE_MOVES = {"Li8ELi16ELi8ELb1": (208, 0), "Li8ELi9ELi8ELb1": (149, 0)}      # e5f53c9: (v_readlane_b32, v_writelane_b32) in the step loop
FIELDS = ("vgprs", "scratch", "sgpr_spills", "vgpr_spills", "occupancy")


@pytest.fixture(scope="module")
def asm():
    from twisterl_amd import build as tb
    path = os.path.join(tb.ASM_DIR, "tw_rollout.s")
    tb.build_library(force=not os.path.exists(path))           # (incremental; leaves the assembly of every object in lib/asm/)
    return open(path).read()


@pytest.fixture(scope="module")
def parent():
    return json.load(open(GOLDEN))["kernels"]


def resources(text):
    """name -> the figures of every rollout_f32_kernel: VGPRs, scratch and occupancy from the kernel info comments behind the function
    (the remark's figures), the spill counts from the descriptors of the metadata at the file's end."""
    info = {}
    for m in re.finditer(r"^(_ZN2tw18rollout_f32_kernel\w+):.*?^; NumVgprs: (\d+)$.*?^; ScratchSize: (\d+)$.*?^; Occupancy: (\d+)$", text, re.S | re.M):
        info[m.group(1)] = {"vgprs": int(m.group(2)), "scratch": int(m.group(3)), "occupancy": int(m.group(4))}
    out = {}
    for blk in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        if not name.startswith("_ZN2tw18rollout_f32_kernel"):
            continue
        num = lambda key: int(re.search(r"^\s+\.%s:\s+(\d+)" % key, blk, re.M).group(1))
        assert num("private_segment_fixed_size") == info[name]["scratch"], name
        out[name] = dict(info[name], sgpr_spills=num("sgpr_spill_count"), vgpr_spills=num("vgpr_spill_count"))
    return out


def function_lines(text, key):
    m = re.search(r"^(_ZN2tw18rollout_f32_kernelI%sEEEvNS_11RolloutArgsE):\s.*?^\.Lfunc_end\d+:" % key, text, re.S | re.M)
    assert m, key
    return m.group(0).splitlines()


_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def step_loop(lines):
    labels = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    best = None
    for i, ln in enumerate(lines):
        m = _BRANCH.match(ln)
        if m and labels.get(m.group(1), i) < i and any("v_mfma" in x for x in lines[labels[m.group(1)]:i]):
            if best is None or i - labels[m.group(1)] > best[1] - best[0]:
                best = (labels[m.group(1)], i)
    assert best, "no loop around an MFMA"
    lo, hi = best
    grown = True
    while grown:
        grown = False
        for i in range(len(lines) - 1, hi, -1):
            m = _BRANCH.match(lines[i])
            if m and lo <= labels.get(m.group(1), -1) <= hi:
                hi, grown = i, True
                break
    return lo, hi


def lane_moves(lines):
    """(v_readlane_b32, v_writelane_b32, most v_writelane_b32 in one basic block, MFMAs) of the step loop."""
    lo, hi = step_loop(lines)
    rd = wr = in_block = worst = mfma = 0
    for ln in lines[lo:hi + 1]:
        if re.match(r"^\.LBB\d+_\d+:", ln):
            in_block = 0
        op = re.match(r"^\s+([a-z_0-9]+)", ln)
        if not op:
            continue
        rd += op.group(1) == "v_readlane_b32"
        mfma += op.group(1).startswith("v_mfma")
        if op.group(1) == "v_writelane_b32":
            wr += 1; in_block += 1; worst = max(worst, in_block)
    return rd, wr, worst, mfma


def test_every_instantiation_is_no_worse_than_the_parent(asm, parent):
    now = resources(asm)
    assert set(now) == set(parent) and len(now) == 57
    for name, p in sorted(parent.items()):
        n = now[name]
        print(name, {f: (p[f], n[f]) for f in FIELDS if p[f] != n[f]})
        if not re.search(r"ELi8ELb[01]EEEv", name):                                    # NW != 8: the parent's figures
            assert {f: n[f] for f in FIELDS} == {f: p[f] for f in FIELDS}, name
        for f in ("vgprs", "scratch", "sgpr_spills", "vgpr_spills"):
            assert n[f] <= p[f], (name, f, p[f], n[f])
        assert n["occupancy"] >= p["occupancy"], name


def test_the_benchmark_kernel_keeps_its_registers_and_halves_its_scalar_spills(asm, parent):
    now = resources(asm)
    name = "_ZN2tw18rollout_f32_kernelILi8ELi16ELi8ELb1EEEvNS_11RolloutArgsE"
    n, p = now[name], parent[name]
    print(name, n)
    assert p["sgpr_spills"] == 120
    assert n["scratch"] == 0 and n["vgpr_spills"] == 0 and n["vgprs"] <= 256 and n["occupancy"] == 2
    assert n["sgpr_spills"] <= p["sgpr_spills"] // 2
    plain = now["_ZN2tw18rollout_f32_kernelILi8ELi16ELi8ELb0EEEvNS_11RolloutArgsE"]
    assert plain["scratch"] <= 64 and plain["vgpr_spills"] <= 15


@pytest.mark.parametrize("key", sorted(PARENT_LANE_MOVES))
def test_lane_moves_in_the_step_loop_are_at_most_half_the_parents(asm, key):
    rd, wr, worst, mfma = lane_moves(function_lines(asm, key))
    prd, pwr = PARENT_LANE_MOVES[key]
    print(f"{key}: v_readlane_b32 {rd} (parent {prd}) v_writelane_b32 {wr} (parent {pwr}), most in one block {worst}; MFMAs in the loop {mfma}")
    assert mfma == 3 * 64                                       # the loop found is the step loop: three chunk bodies of 64 MFMAs
    assert 2 * (rd + wr) <= prd + pwr
    assert worst < 16
