"""CPU: tests/policy_sync_matrix.py's table reaches every layout class of the two policy-sync kernels (tw_sync.hip) at least once,
and every row is a shape the library takes.

A class is a way the image of a policy is laid out or padded: which images exist, where an index map's guard cuts, where a
count is rounded up.  The list below names them; a row taken out of the table, or a class added without a row, fails here by
the class's name.  tests/test_gpu_policy_sync.py then syncs every row on the GPU.
"""
import numpy as np

from tests import policy_sync_matrix as pm

# class name -> predicate over (row, one_classes(row)) for the one-common-layer kernel
ONE_CLASSES = {
    "n16 == nc16 (4, 9 or 16 cells a side: no guarded table pieces)": lambda r, c: c["f16_ok"] and c["n16"] == c["nc16"],
    "n16 2 < nc16 4": lambda r, c: (c["n16"], c["nc16"]) == (2, 4),
    "n16 5 < nc16 9": lambda r, c: (c["n16"], c["nc16"]) == (5, 9),
    "n16 10 < nc16 16": lambda r, c: (c["n16"], c["nc16"]) == (10, 16),
    "A == 4 with f16 images": lambda r, c: c["f16_ok"] and r.A == 4,
    "A < 4 with f16 images (zero head rows)": lambda r, c: c["f16_ok"] and r.A < 4,
    "A == 1": lambda r, c: r.A == 1,
    "A > 4 (wh8 / bh8 zero, no f16 images)": lambda r, c: r.A > 4 and not c["f16_ok"],
    "obs_size not a square (no f16 images)": lambda r, c: c["n16"] ** 2 != r.obs_size and not c["f16_ok"],
    "more than 4 twists (no f16 images)": lambda r, c: c["n_perms"] > 4 and c["n16"] ** 2 == r.obs_size and r.A <= 4 and not c["f16_ok"],
    "twists with f16 images": lambda r, c: c["f16_ok"] and c["n_perms"] > 0,
    "emb 32 (NKT 1: f16 images without the split ones)": lambda r, c: c["f16_ok"] and c["NKT"] == 1 and not c["split_ok"],
    "odd NKT > 1": lambda r, c: c["split_ok"] and c["NKT"] % 2 == 1,
    "NT 1 (three zero row-tiles in the w1p quad)": lambda r, c: c["NT"] == 1,
    "NT 2 (two zero row-tiles in the w1p quad)": lambda r, c: c["NT"] == 2,
    "NT 4 (a full w1p quad)": lambda r, c: c["NT"] == 4,
    "NQ 2": lambda r, c: c["NQ"] == 2,
    "SP16 rounded up (empty pieces at the end of a stage)": lambda r, c: c["f16_ok"] and c["SP16"] > c["nc16"] + 2 * c["NT"],
    "SP16 exact": lambda r, c: c["f16_ok"] and c["SP16"] == c["nc16"] + 2 * c["NT"],
    "SPS from nc16 + 2 NT": lambda r, c: c["split_ok"] and c["nc16"] + 2 * c["NT"] > 4 * c["NT"],
    "SPS from 4 NT": lambda r, c: c["split_ok"] and 4 * c["NT"] > c["nc16"] + 2 * c["NT"],
    "obs_size 256 (258 rows of 268 in a t_img16 slot)": lambda r, c: r.obs_size == 256,
    "the benchmark's shape": lambda r, c: (r.obs_size, r.emb, r.hidden, r.A, r.twists) == (256, 512, 256, 4, "transpose"),
}

# class name -> predicate over (row, gen_classes(row)) for the kernel of stacks of any depth
GEN_CLASSES = {
    "in % 4 != 0 (rows of -0.0 below the matrix-core image)": lambda r, ls: any(l["inp"] % 4 for l in ls),
    "width not a multiple of 4 (zero columns in the natural image)": lambda r, ls: any(l["out"] % 4 for l in ls),
    "width a multiple of 4, not of 16 (a part-filled tile)": lambda r, ls: any(l["out"] % 4 == 0 and l["out"] % 16 for l in ls),
    "a last block with empty tiles": lambda r, ls: any(l["nb"] * l["tb"] > l["tiles"] for l in ls),
    "several full blocks": lambda r, ls: any(l["nb"] > 1 and l["out"] % 64 == 0 for l in ls),
    "fewer than four tiles (tb < 4)": lambda r, ls: any(1 < l["tb"] < 4 for l in ls),
    "one output": lambda r, ls: any(l["out"] == 1 for l in ls),
    "obs_size > 256": lambda r, ls: r.obs_size > 256,
    "emb not a multiple of 32 under one common layer (the shape the other kernel would take but for its widths)":
        lambda r, ls: r.emb % 32 != 0 and len(ls) == 3 and len(r.common) == 1,
    "no common layer": lambda r, ls: not r.common,
    "31 actions": lambda r, ls: r.A == 31,
    "hidden policy and value layers": lambda r, ls: bool(r.policy_layers) and bool(r.value_layers),
    "GEN_SYNC_MAX_LAYERS layers": lambda r, ls: len(ls) == pm.GEN_SYNC_MAX_LAYERS,
}


def test_table_reaches_every_class_of_the_one_common_layer_kernel():
    for name, pred in ONE_CLASSES.items():
        assert any(pred(r, pm.one_classes(r)) for r in pm.ONE_TABLE), f"no row of ONE_TABLE reaches: {name}"


def test_table_reaches_every_class_of_the_generic_kernel():
    for name, pred in GEN_CLASSES.items():
        assert any(pred(r, pm.gen_classes(r)) for r in pm.GEN_TABLE), f"no row of GEN_TABLE reaches: {name}"


def test_every_row_reaches_a_class_no_other_row_does():
    """No row is spare: taking any one out leaves a class without a row."""
    for table, classes, of in ((pm.ONE_TABLE, ONE_CLASSES, pm.one_classes), (pm.GEN_TABLE, GEN_CLASSES, pm.gen_classes)):
        for i, row in enumerate(table):
            rest = table[:i] + table[i + 1:]
            lost = [n for n, pred in classes.items() if not any(pred(r, of(r)) for r in rest)]
            assert lost, f"row {row} reaches nothing the other rows do not"


def test_rows_are_shapes_the_library_takes():
    for r in pm.ONE_TABLE:
        assert pm.is_mfma_shape(r), r
        op, ap = pm.twists_of(r)
        assert len(op) == len(ap) <= 127 and all(sorted(p) == list(range(r.obs_size)) for p in op) and all(sorted(p) == list(range(r.A)) for p in ap), r
    for r in pm.GEN_TABLE:
        assert pm.generic_accepts(r), r
        assert len(pm.gen_layers(r)) <= pm.GEN_SYNC_MAX_LAYERS, r
        # what keeps a row off the one-common-layer path (is_mfma_shape): another number of layers, or widths it does not take
        assert (len(r.common), len(r.policy_layers), len(r.value_layers)) != (1, 0, 0) or r.emb % 32 or r.common[0] not in (32, 64, 128, 256), r
    assert max(pm.image_bytes(pm.segments(r)) for r in pm.ONE_TABLE + pm.GEN_TABLE) < 8 << 20      # every image stays cheap to read back


def test_the_table_holds_the_smallest_shape_of_every_class():
    """The rows by value: the smallest shapes that reach their class, so that a row is not swapped for an easier one unnoticed."""
    want = [(16, 32, 32, 4, None), (4, 64, 64, 2, None), (25, 96, 128, 3, None), (81, 64, 256, 4, "transpose"), (100, 128, 32, 1, None),
            (256, 512, 256, 4, "transpose"), (30, 160, 64, 4, None), (36, 64, 32, 7, None), (16, 64, 32, 4, "five")]
    assert [tuple(r) for r in pm.ONE_TABLE] == want
    assert [tuple(r)[:2] + (r.A,) for r in pm.GEN_TABLE] == [(9, 36, 4), (625, 64, 4), (16, 32, 31), (16, 32, 4)]
    assert pm.GEN_TABLE[1].common == (80, 512) and pm.GEN_TABLE[1].policy_layers == (17,) and pm.GEN_TABLE[1].value_layers == (5,)
    deep = pm.GEN_TABLE[3]
    assert len(deep.common) == 8 and len(deep.policy_layers) == len(deep.value_layers) == 7
    assert all(8 <= h <= 40 for h in deep.common + deep.policy_layers + deep.value_layers)


def test_class_formulas_at_shapes_known_from_the_engines():
    """The restated formulas at shapes whose geometry the engines' sources state."""
    c = pm.one_classes(pm.One(256, 512, 256, 4, "transpose"))       # Puzzle-15, the benchmark: 16 table pieces + 16 W1 pieces per stage
    assert (c["n16"], c["nc16"], c["NT"], c["NQ"], c["NKT"], c["SP16"], c["SPS"], c["f16_ok"], c["split_ok"]) == (16, 16, 8, 2, 16, 32, 32, True, True)
    c = pm.one_classes(pm.One(81, 64, 32, 4, None))                 # Puzzle-8 at the kernel matrix's smallest split shape
    assert (c["n16"], c["nc16"], c["NT"], c["NQ"], c["NKT"], c["SP16"], c["SPS"]) == (9, 9, 1, 1, 2, 12, 12)
    c = pm.one_classes(pm.One(25, 96, 128, 3, None))
    assert (c["n16"], c["nc16"], c["SP16"], c["SPS"], c["split_ok"]) == (5, 9, 20, 20, True)
    assert pm.one_classes(pm.One(30, 160, 64, 4, None))["nc16"] == 0
    ls = pm.gen_classes(pm.Gen(625, 64, (80, 512), (17,), (5,), 4))
    assert [(l["pad4"], l["tb"], l["nb"], l["kg"]) for l in ls] == [(80, 4, 2, 16), (512, 4, 8, 20), (20, 2, 1, 128), (4, 1, 1, 5), (8, 1, 1, 128), (4, 1, 1, 2)]
    # a twist that splits a cell's ids over two cells has no f16 image
    bad = list(range(16)); bad[0], bad[5] = bad[5], bad[0]
    assert pm.cells_map_to_cells([list(range(16))], 4) and not pm.cells_map_to_cells([bad], 4)


def test_segments_tile_the_image():
    for r in pm.ONE_TABLE + pm.GEN_TABLE:
        segs = pm.segments(r)
        end = 0
        for name, off, b in segs:
            assert off % 256 == 0 and off >= end, (r, name)
            end = off + b
        assert pm.segment_of(segs, segs[1][1] + 5) == f"{segs[1][0]}+5"
    one = dict((n, (o, b)) for n, o, b in pm.one_segments(pm.One(16, 32, 32, 4, None)))
    assert one["stageS"][1] == one["t0S"][1] == one["split_range"][1] == 0 and one["stage16"][1] == 8 * 1024
    flag = pm.one_segments(pm.One(16, 64, 32, 4, None))[-1]
    assert flag[0] == "split_range" and flag[2] == 4


def test_array_helpers_keep_the_draws_and_round_trip():
    from tests.util import make_policy_arrays, make_policy_arrays_obs
    a, b = make_policy_arrays(9, seed=7, emb=32, hidden=32), make_policy_arrays_obs(81, seed=7, emb=32, hidden=32)
    flat = lambda arrs: [arrs[0], arrs[1]] + [x for st in arrs[2:] for (w, bias, _) in st for x in (w, bias)]
    assert all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))
    c = make_policy_arrays_obs(30, seed=1, emb=32, hidden=64, n_actions=7)
    assert c[0].shape == (30, 32) and c[3][0][0].shape == (64 * 7,) and c[3][0][1].shape == (7,)
    for row in (pm.ONE_TABLE[2], pm.GEN_TABLE[1]):
        arrs = pm.arrays(row, 3)
        st = pm.torch_layout(arrs)
        assert st["embeddings.weight"].shape == (row.emb, row.obs_size)
        back = pm.export_layout(st, arrs)
        assert all(np.array_equal(x, y) for x, y in zip(flat(arrs), flat(back)))
        assert [r for s in back[2:] for (_, _, r) in s] == [r for s in arrs[2:] for (_, _, r) in s]
    other = pm.arrays(pm.ONE_TABLE[2], 4)
    assert all(not np.any(x == y) for x, y in zip(flat(pm.arrays(pm.ONE_TABLE[2], 3)), flat(other)))     # another seed: every element differs
