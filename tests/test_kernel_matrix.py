"""CPU: tests/kernel_matrix.py's table has exactly one row per rollout kernel the build ships, and its restatement of the
launch rule agrees with the launch shapes other tests assert on the GPU.

The kernels are read from the device assembly the build keeps (lib/asm/tw_rollout.s, tw_rollout16.s: one `.amdhsa_kernel`
directive per instantiation, the text test_mfma_hazards.py scans).  A new instantiation without a row, or a row whose
restated dispatch lands on a kernel that is not built, fails here by name.
"""
import collections
import os
import re

import pytest

from tests import kernel_matrix as km

F32 = re.compile(r"^_ZN2tw18rollout_f32_kernelILi(\d+)ELi(\d+)ELi(n?\d+)ELb([01])EEEvNS_11RolloutArgsE$")
F16 = re.compile(r"^_ZN2tw18rollout_f16_kernelINS_\d+(Engine16|EngineS)ILi(\d+)ELi(\d+)EEELi(\d+)ELb([01])EEEvNS_11RolloutArgsE$")


def _num(s):
    return -int(s[1:]) if s.startswith("n") else int(s)


def built_rollout_kernels():
    """Names (kernel_matrix.kernel_name form) of every rollout_f32_kernel / rollout_f16_kernel in the built assembly."""
    from twisterl_amd import build as tb
    paths = [os.path.join(tb.ASM_DIR, f) for f in ("tw_rollout.s", "tw_rollout16.s")]
    if not all(os.path.exists(p) for p in paths):
        tb.build_library()
    names = []
    for p in paths:
        for line in open(p):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if not m or "rollout_f" not in m.group(1):
                continue
            sym = m.group(1)
            a, b = F32.match(sym), F16.match(sym)
            assert a or b, f"a rollout kernel of a form the table does not know: {sym}"
            if a:
                names.append(km.kernel_name(("f32", int(a.group(1)), int(a.group(2)), _num(a.group(3)), a.group(4) == "1")))
            else:
                assert b.group(3) == b.group(4), sym
                names.append(km.kernel_name(("f16", b.group(1), int(b.group(2)), int(b.group(3)), b.group(5) == "1")))
    return names


def _covered(table, cus):
    return collections.Counter(km.kernel_name(km.dispatch(r, cus)[0]) for r in table)


def test_built_kernels_are_the_known_family():
    names = built_rollout_kernels()
    assert len(names) == len(set(names))
    f32 = [n for n in names if n.startswith("rollout_f32")]
    f16 = [n for n in names if n.startswith("rollout_f16")]
    assert len(f16) == 48 and sum("EngineS" in n for n in f16) == 24, len(f16)
    assert len(f32) == 57 and sum(", -65, " in n for n in f32) == 6, len(f32)      # (the census of the whole build: tests/test_search_matrix.py)


@pytest.mark.parametrize("cus", [256, 304])
def test_table_covers_every_built_rollout_kernel_once(cus):
    built = set(built_rollout_kernels())
    got = _covered(km.TABLE, cus)
    missing = sorted(built - set(got))
    assert not missing, f"rollout kernels without a row in tests/kernel_matrix.py: {missing}"
    unknown = sorted(set(got) - built)
    assert not unknown, f"rows whose restated dispatch names a kernel the build does not have: {unknown}"
    twice = sorted(k for k, n in got.items() if n > 1)
    assert not twice, f"instantiations with more than one row: {twice}"
    assert len(km.TABLE) == len(built)


def test_deleting_any_row_names_the_kernel_it_covered():
    built = set(built_rollout_kernels())
    for i, row in enumerate(km.TABLE):
        rest = km.TABLE[:i] + km.TABLE[i + 1:]
        missing = built - set(_covered(rest, 256))
        assert missing == {km.kernel_name(km.dispatch(row, 256)[0])}, (i, row)


def test_rows_are_shapes_the_library_takes():
    for r in km.TABLE:
        cells = r.w * r.h
        assert 1 <= cells <= 16 and r.emb % 32 == 0 and r.emb >= (64 if r.prec == "fp16x2" else 32), r
        assert not r.twists or r.w == r.h, r                     # the transpose twist needs a square board
        assert r.prec == "fp32" or r.common is None, r           # the f16 modes exist for the one-common-layer shape only
        assert (r.common is None) == (r.hidden in (32, 64, 128, 256)), r
        assert r.force_geom in (0, 8, 32) and r.reserve in (None, km.AB1) and 1 <= r.diff <= 6, r
        assert r.E <= 12_800, r                                  # every row stays cheap enough to compare in full on the GPU


def test_restated_dispatch_matches_the_launch_shapes_the_suite_asserts():
    cus = 256
    big = lambda E, h, **kw: km.R(4, 4, 512, h, E, **kw)
    # BASELINE config 3 as benched: 262,144 Puzzle-15 envs -> 8 waves x 32, one persistent workgroup per CU
    # (test_gpu_reference_tolerance, test_gpu_exhaustive)
    assert km.dispatch(big(262_144, 256), cus) == (("f32", 8, 16, 8, True), (cus, 512))
    # config 2 in f32: 65,536 Puzzle-8 envs -> min(E // 256, CUs) x 512 (test_gpu_exhaustive)
    assert km.dispatch(km.R(3, 3, 512, 256, 65_536), cus) == (("f32", 8, 9, 8, False), (256, 512))
    # generic stacks beyond two 16-episode workgroups per CU: the queue, (2 CUs, 256) (test_gpu_parity)
    k, shape = km.dispatch(km.R(3, 3, 32, 0, cus * 32 + 1500, common=(48, 32)), cus)
    assert k == ("f32", 0, 9, -65, True) and shape == (2 * cus, 256)
    # mid-size batches: the 32-episode shape with the queue, fewer lanes than episodes (test_gpu_parity)
    k, shape = km.dispatch(km.R(3, 3, 64, 128, 9_000), cus)
    assert k == ("f32", 4, 9, -4, True) and shape[1] == 256 and shape[0] * 32 < 9_000
    # tiny batches: 16 episodes per workgroup (test_gpu_parity, E // 16 x 256)
    assert km.dispatch(km.R(4, 4, 512, 256, 4096), cus)[1] == (4096 // 16, 256)
    # TW_OPT_FORCE_GEOM moves a 600-episode Puzzle-15 collect off its default shape (test_every_launch_shape_gives_the_same_bytes)
    base = km.dispatch(big(600, 256), cus)
    for g in (8, 32):
        assert km.dispatch(big(600, 256, force_geom=g), cus)[1] != base[1]
    # reserved CUs shrink the persistent grid: (CUs - reserve) x 512 (test_gpu_full_size)
    assert km.dispatch(big(262_144, 256, reserve=km.AB1), cus)[1] == (1, 512)
    # the f16 modes: 256 episodes per workgroup, one persistent workgroup per CU beyond CUs x 256
    assert km.dispatch(km.R(3, 3, 512, 256, 65_536, "fp16"), cus) == (("f16", "Engine16", 8, 9, False), (256, 256))
    assert km.dispatch(km.R(3, 3, 64, 32, 70_000, "fp16x2"), cus) == (("f16", "EngineS", 1, 9, True), (cus, 256))
    assert km.dispatch(km.R(3, 3, 64, 32, 70_000, "fp16x2", no_persist=True), cus) == (("f16", "EngineS", 1, 9, False), (274, 256))
