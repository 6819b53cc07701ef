"""Every layout class of the trainer-to-collector weight sync, one table row each, and the layout rules themselves (GPU-free).

`Policy.update_from_torch` rebuilds a policy's device image from the trainer's tensors with `policy_sync_kernel` (the
one-common-layer shape) or `policy_sync_generic_kernel` (a stack of any depth), both in twisterl_amd/csrc/tw_sync.hip.  The
kernels re-state on the device the index maps `tw_policy_create` / `create_generic_policy` (tw_api.hip) apply on the host, and
which images exist, how large they are and which of their elements are padding depends on the shape.  This module restates, in
Python, the class formulas of the two host builders and the order and size of the segments of the image, and lists the
smallest shapes that reach every class.

tests/test_policy_sync_matrix.py holds the table against the list of classes; tests/test_gpu_policy_sync.py syncs every row on
the GPU and compares the image, byte for byte, with the one the host builder makes of the same weights.

One-common-layer rows: (obs_size, emb, hidden, A, twists), twists one of None, "transpose" (the board transpose of a square
board whose obs ids are cell * n + tile), "five" (five twists: more than the f16 engines take).
Generic rows: (obs_size, emb, common, policy_layers, value_layers, A): hidden widths; the heads (A and 1 outputs) come on top.
"""
from collections import namedtuple

import numpy as np

One = namedtuple("One", "obs_size emb hidden A twists")
Gen = namedtuple("Gen", "obs_size emb common policy_layers value_layers A")

GEN_SYNC_MAX_LAYERS = 24       # tw_common.hpp
LAYER_DEV_BYTES = 56           # sizeof(LayerDev), tw_common.hpp: w, b, (in, out, relu, pad), wm, (kg, nb, tb, pad2)
LAYER_DEV_POINTERS = (0, 8, 32)  # offsets of w, b, wm

ONE_TABLE = [
    One(16, 32, 32, 4, None),            # emb 32: NKT 1, no split images; NT 1 (w1p quads zero-padded)
    One(4, 64, 64, 2, None),             # n16 2 < nc16 4; A < 4; NT 2
    One(25, 96, 128, 3, None),           # n16 5 / nc16 9; odd NKT; NT 4 (no padding in the w1p quad)
    One(81, 64, 256, 4, "transpose"),    # NQ 2; SPS from 4 * NT; stage16 padded to a whole round of pieces
    One(100, 128, 32, 1, None),          # n16 10 / nc16 16; one action
    One(256, 512, 256, 4, "transpose"),  # the benchmark's shape: 258 rows in t_img16
    One(30, 160, 64, 4, None),           # not a square: no f16 images
    One(36, 64, 32, 7, None),            # A > 4: wh8 / bh8 zero, no f16 images
    One(16, 64, 32, 4, "five"),          # more than 4 twists: no f16 images
]

GEN_TABLE = [
    Gen(9, 36, (30,), (), (), 4),                                   # the heads read 30 inputs: in % 4 != 0
    Gen(625, 64, (80, 512), (17,), (5,), 4),                        # obs_size > 256; 5 tiles in 2 blocks; widths not a multiple of 4
    Gen(16, 32, (), (24,), (), 31),                                 # no common layer; the widest action head
    Gen(16, 32, (40, 8, 36, 12, 28, 20, 24, 16), (16, 9, 24, 33, 8, 40, 12), (12, 40, 8, 31, 24, 10, 16), 4),   # 24 layers
]


def align_up(x, a=256):
    return (x + a - 1) // a * a


# ------------------------------------------------------------------------------------------ twists
def twists_of(row):
    """(obs_perms, act_perms) of a one-common-layer row."""
    if row.twists is None:
        return [], []
    if row.twists == "transpose":
        from tests.util import puzzle_transpose_twist
        n2 = int(round(row.obs_size ** 0.5))
        return puzzle_transpose_twist(int(round(n2 ** 0.5)))
    assert row.twists == "five"
    rng = np.random.default_rng(5)
    return ([rng.permutation(row.obs_size).tolist() for _ in range(5)], [rng.permutation(row.A).tolist() for _ in range(5)])


def cells_map_to_cells(obs_perms, n16):
    """tw_policy_create's condition on the twists of an f16 image: ids are cell * n16 + tile, and every twist sends all ids of a
    cell to one cell, each cell once."""
    for p in obs_perms:
        seen = set()
        for sc in range(n16):
            cells = {p[sc * n16 + v] // n16 for v in range(n16)}
            if len(cells) != 1 or (cells & seen):
                return False
            seen |= cells
    return True


# ------------------------------------------------------------------------------------------ the one-common-layer shape
def is_mfma_shape(row):
    """tw_api.hip is_mfma_shape for embedding -> one common Linear -> linear heads (the layer counts and the chain of widths are
    what a One row is made of)."""
    E, H, A, OS = row.emb, row.hidden, row.A, row.obs_size
    return (1 <= A <= 31 and E != 0 and E % 32 == 0 and H != 0 and H % 32 == 0 and H <= 256 and (H & (H - 1)) == 0 and 1 <= OS <= 256)


def one_classes(row):
    """The class formulas of tw_policy_create."""
    OS, E, H, A = row.obs_size, row.emb, row.hidden, row.A
    obs_perms, _ = twists_of(row)
    n_perms = len(obs_perms)
    n16 = 1
    while n16 * n16 < OS:
        n16 += 1
    f16_ok = n16 * n16 == OS and n16 <= 16 and n_perms <= 4 and A <= 4 and cells_map_to_cells(obs_perms, n16)
    nc16 = 0 if not f16_ok else (4 if n16 <= 4 else (9 if n16 <= 9 else 16))
    NT, NKT = H // 32, E // 32
    NQ = (NT + 3) // 4
    SP16 = (nc16 + 2 * NT + 3) // 4 * 4
    SPS = (max(nc16 + 2 * NT, 4 * NT) + 3) // 4 * 4 if f16_ok else 0
    split_ok = f16_ok and NKT >= 2
    return dict(n16=n16, nc16=nc16, f16_ok=f16_ok, split_ok=split_ok, NT=NT, NQ=NQ, NKT=NKT, SP16=SP16, SPS=SPS, n_perms=n_perms)


def one_segments(row):
    """[(name, offset, bytes)] of the one-common-layer image in the order tw_policy_create lays it out; every segment starts on
    a multiple of 256 and the gaps stay zero.  `split_range` (the range flag word of the split-f16 images) comes last."""
    c = one_classes(row)
    OS, E, H, A = row.obs_size, row.emb, row.hidden, row.A
    NT, NQ, NKT, nc16, f16, split = c["NT"], c["NQ"], c["NKT"], c["nc16"], c["f16_ok"], c["split_ok"]
    np_ = max(c["n_perms"], 1)
    sizes = [("emb_rows", (OS + 2) * E * 4), ("w1p", E * NQ * 128 * 4), ("b1", H * 4), ("t_img16", (E // 16) * 21 * 256 * 4),
             ("wh8", H * 8 * 4), ("bh8", 32), ("w1", E * H * 4), ("wa", H * A * 4), ("ba", A * 4), ("wv", H * 4), ("bv", 4),
             ("obs_perms", np_ * OS), ("act_perms", np_ * A),
             ("stage16", NKT * c["SP16"] * 1024 if f16 else 0), ("head16", NT * 2048 if f16 else 0),
             ("ebias16", NKT * 32 * 4), ("b1img16", NT * 32 * 4), ("bh16", 32),
             ("srcmap16", (c["n_perms"] + 1) * 16), ("vmap16", (c["n_perms"] + 1) * 256),
             ("stageS", (2 * NKT + 1) * c["SPS"] * 1024 if split else 0), ("t0S", 2 * nc16 * 1024 if split else 0),
             ("split_range", 4 if split else 0)]
    return _lay_out(sizes)


def _lay_out(sizes):
    out, cur = [], 0
    for name, b in sizes:
        out.append((name, cur, b))
        cur = align_up(cur + b)
    return out


def image_bytes(segments):
    name, off, b = segments[-1]
    return align_up(off + b)


def segment_of(segments, offset):
    """'name+byte' of the segment an image offset lies in (or of the gap after it)."""
    for name, off, b in reversed(segments):
        if offset >= off:
            return f"{name}+{offset - off}" + ("" if offset < off + b else " (past its end)")
    return str(offset)


# ------------------------------------------------------------------------------------------ stacks of any depth
def gen_layers(row):
    """[(in, out, relu)] of every Linear in the order common.., action.., value.. (create_generic_policy's `all`)."""
    out, w = [], row.emb
    for h in row.common:
        out.append((w, h, True)); w = h
    wa = w
    for h in row.policy_layers:
        out.append((wa, h, True)); wa = h
    out.append((wa, row.A, False))
    wv = w
    for h in row.value_layers:
        out.append((wv, h, True)); wv = h
    out.append((wv, 1, False))
    return out


def generic_accepts(row):
    """create_generic_policy's conditions."""
    E, OS = row.emb, row.obs_size
    if E == 0 or E % 4 != 0 or E > 512 or OS == 0 or OS > 65535:
        return False
    if len(row.common) > 8 or len(row.policy_layers) + 1 > 8 or len(row.value_layers) + 1 > 8:
        return False
    return all(1 <= o <= 512 for _, o, _ in gen_layers(row)) and 1 <= row.A <= 31


def gen_classes(row):
    """Per layer, the class formulas of create_generic_policy: pad4 (the padded width of the natural image), tb tiles of 16
    outputs per block, nb blocks, kg groups of four inputs."""
    out = []
    for i, o, _ in gen_layers(row):
        tiles = (o + 15) // 16
        tb = 4 if tiles >= 4 else tiles
        out.append(dict(inp=i, out=o, pad4=(o + 3) & ~3, tiles=tiles, tb=tb, nb=(tiles + tb - 1) // tb, kg=(i + 3) // 4))
    return out


def gen_segments(row):
    """[(name, offset, bytes)] of a generic stack's image in create_generic_policy's order."""
    ls = gen_classes(row)
    OS = row.obs_size
    sizes = [("emb_rows", (OS + 2) * row.emb * 4), ("layer_table", max(len(ls), 1) * LAYER_DEV_BYTES), ("obs_perms", OS), ("act_perms", row.A),
             ("obs_perms16", OS * 2 if OS > 256 else 0)]            # (no twists in the table's generic rows: room for one)
    for n, l in enumerate(ls):
        sizes.append((f"w_nat[{n}]", l["inp"] * l["pad4"] * 4))
        sizes.append((f"b_img[{n}]", l["nb"] * l["tb"] * 16 * 4 + 16))
        sizes.append((f"wm[{n}]", (l["kg"] + 8) * 4 * l["nb"] * 16 * l["tb"] * 4 + 64))
    return _lay_out(sizes)


def is_generic(row):
    return isinstance(row, Gen)


def segments(row):
    return gen_segments(row) if is_generic(row) else one_segments(row)


# ------------------------------------------------------------------------------------------ weights
def arrays(row, seed):
    """A row's weights in the reference's export layout (tests/util.py)."""
    from tests.util import make_deep_policy_arrays_obs, make_policy_arrays_obs
    if is_generic(row):
        return make_deep_policy_arrays_obs(row.obs_size, seed=seed, emb=row.emb, common=row.common, policy_layers=row.policy_layers,
                                           value_layers=row.value_layers, n_actions=row.A, scale=2.0)
    return make_policy_arrays_obs(row.obs_size, seed=seed, emb=row.emb, hidden=row.hidden, n_actions=row.A, scale=2.0)


def torch_layout(arrs):
    """{state_dict key: float32 array in torch's layout} of export-layout weights: Linear.weight = [out][in]; the Linear layers of
    a stack are the even entries of its Sequential (Linear, ReLU, Linear, ..)."""
    we, be, cs, acts, vals = arrs
    state = {"embeddings.weight": np.ascontiguousarray(we.T), "embeddings.bias": np.array(be, dtype=np.float32)}
    for name, layers in (("common", cs), ("action", acts), ("value", vals)):
        for i, (wl, bl, _) in enumerate(layers):
            state[f"{name}.{2 * i}.weight"] = np.ascontiguousarray(np.asarray(wl, dtype=np.float32).reshape(-1, len(bl)).T)
            state[f"{name}.{2 * i}.bias"] = np.array(bl, dtype=np.float32)
    return state


def export_layout(state, like):
    """The inverse of torch_layout: export-layout arrays (what the Policy constructors take) of a torch-layout state, with the
    ReLU flags of `like`."""
    _, _, cs, acts, vals = like
    stack = lambda name, ls: [(np.ascontiguousarray(state[f"{name}.{2 * i}.weight"].T).reshape(-1), np.array(state[f"{name}.{2 * i}.bias"]), r)
                              for i, (_, _, r) in enumerate(ls)]
    return (np.ascontiguousarray(state["embeddings.weight"].T), np.array(state["embeddings.bias"]),
            stack("common", cs), stack("action", acts), stack("value", vals))
