"""GPU: the trainer-to-collector weight sync (Policy.update_from_torch -> policy_sync_kernel / policy_sync_generic_kernel,
tw_sync.hip), image by image, at every layout class of tests/policy_sync_matrix.py.

The reference of an image is the one tw_policy_create builds on the host with plain loops of the same weights (the kernel
matrix holds that builder to the oracle and to float64); `_lib.debug_policy_image` reads both.  No comparison here has a
tolerance: images and collects are compared as bytes.

(a) every row of the table: a policy built from weight set 1 and synced to set 2 has the image of a policy built from set 2,
    and a change of the last element of any one tensor shows in it;
(b) dense rollouts (Puzzle-15 at difficulty 128, Puzzle-8 at 40) that read every row of the embedding table, after a sync,
    in the three precisions -- in fp32 against the oracle as well;
(c) the range flag of the split-f16 images through the sync: set by a weight of 4095 or more, cleared again afterwards;
(d) the Python front end: modules, state dicts, Parameters, float64, CPU, non-contiguous and offset tensors, the Conv1dPolicy
    layout, and what it refuses.
"""
import ctypes as C

import numpy as np
import pytest

from tests import kernel_matrix as km
from tests import policy_sync_matrix as pm
from tests.test_gpu_parity import _assert_same_collect
from tests.util import amd_policy, make_policy_arrays, oracle_policy, puzzle_transpose_twist
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


@pytest.fixture(scope="module")
def cus():
    import twisterl_amd
    return twisterl_amd.device_info()["compute_units"]


def _row_id(r):
    if pm.is_generic(r):
        return f"deep-{r.obs_size}-{r.emb}-{len(pm.gen_layers(r))}layers-A{r.A}"
    return f"one-{r.obs_size}-{r.emb}-{r.hidden}-A{r.A}" + (f"-{r.twists}" if r.twists else "")


def _build(row, arrs):
    op, ap = ([], []) if pm.is_generic(row) else pm.twists_of(row)
    return amd_policy(arrs, op, ap)


def _cuda(state):
    import torch
    return {k: torch.tensor(v).cuda() for k, v in state.items()}


def _image(pol):
    """The policy's device image with its pointer ranges zeroed, and the ranges."""
    img, ranges = _lib.debug_policy_image(pol)
    for off, n in ranges:
        img[off:off + n] = 0
    return img, ranges


def _first_difference(row, got, want):
    """'segment+byte: got / want' of the first byte two images differ in, '' if they are the same."""
    if got.shape != want.shape:
        return f"{got.size} bytes, the reference has {want.size}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    at = int(bad[0]) & ~3
    where = pm.segment_of(pm.segments(row), at)
    return (f"{bad.size} bytes differ, the first in {where} (image offset {int(bad[0])}): word {got[at:at + 4].view(np.uint32)[0]:#010x}, "
            f"the host builder has {want[at:at + 4].view(np.uint32)[0]:#010x}")


def _assert_image(row, pol, want, what):
    got, _ = _image(pol)
    diff = _first_difference(row, got, want)
    assert not diff, f"{_row_id(row)}, {what}: {diff}"
    return got


# ------------------------------------------------------------------------------------------ (a) image equality
@pytest.mark.parametrize("row", pm.ONE_TABLE + pm.GEN_TABLE, ids=_row_id)
def test_synced_image_equals_the_host_built_image(tw, row):
    arrs1, arrs2 = pm.arrays(row, 1), pm.arrays(row, 2)
    pol, ref = _build(row, arrs1), _build(row, arrs2)
    want, ranges = _image(ref)
    segs = pm.segments(row)
    assert want.size == pm.image_bytes(segs), (_row_id(row), want.size)                   # the restated layout is the library's
    before, pol_ranges = _image(pol)
    assert pol_ranges == ranges and before.size == want.size
    if pm.is_generic(row):
        tab = dict((n, o) for n, o, _ in segs)["layer_table"]
        assert ranges == [(tab + l * pm.LAYER_DEV_BYTES + f, 8) for l in range(len(pm.gen_layers(row))) for f in pm.LAYER_DEV_POINTERS]
    else:
        assert ranges == []
    assert _first_difference(row, before, want)                                             # another weight set: not the same image
    state = _cuda(pm.torch_layout(arrs2))
    assert pol.update_from_torch(state) is pol
    _assert_image(row, pol, want, "after the sync")
    pol.update_from_torch(state)
    _assert_image(row, pol, want, "after a second sync of the same state")
    # the comparison can fail: the last element of each tensor, one at a time
    for key in state:
        t = state[key].clone()
        t.view(-1)[-1] += 1.0
        pol.update_from_torch({**state, key: t})
        got, _ = _image(pol)
        assert _first_difference(row, got, want), f"{_row_id(row)}: the last element of {key} does not reach the image"
        pol.update_from_torch(state)
        _assert_image(row, pol, want, f"after {key} was put back")


# ------------------------------------------------------------------------------------------ (b) dense behaviour
@pytest.mark.parametrize("w,diff,E", [(4, 128, 256), (3, 40, 200)])
def test_synced_policy_on_rollouts_that_read_the_whole_table(tw, oracle, w, diff, E):
    n2 = w * w
    row = pm.One(n2 * n2, 64, 32, 4, "transpose")
    op, ap = puzzle_transpose_twist(w)
    arrs1, arrs2 = make_policy_arrays(n2, seed=1, emb=64, hidden=32), make_policy_arrays(n2, seed=2, emb=64, hidden=32)
    pol, ref, opol = amd_policy(arrs1, op, ap), amd_policy(arrs2, op, ap), oracle_policy(oracle, arrs2, op, ap)
    want, _ = _image(ref)
    pol.update_from_torch(_cuda(pm.torch_layout(arrs2)))
    _assert_image(row, pol, want, "after the sync")
    env = tw.env.Puzzle(w, w, diff, 2, 256)
    for prec in ("fp32", "fp16", "fp16x2"):
        coll = tw.collector.PPOCollector(E, 0.99, 0.95, 1, precision=prec)
        g = coll.collect(env, pol, seed=3)
        a, b = g.to_numpy(), coll.collect(env, ref, seed=3).to_numpy()
        seen = np.unique(a["obs"]).size
        print(f"[policy sync] {w}x{w} difficulty {diff}, {E} episodes, {prec}: {len(a['values'])} records visit {seen} of {n2 * n2} ids")
        assert seen == n2 * n2, (prec, seen)            # the condition of this test: every row of the table is read
        for k in a:
            assert np.array_equal(a[k], b[k]), (prec, k)
        if prec == "fp32":
            o = oracle.ppo_collect(oracle.Puzzle(w, w, diff, 2, 256), opol, E, 0.99, 0.95, seed=3, arith=oracle.ARITH_CHAIN, det_log=True)
            assert np.unique(o.obs).size == n2 * n2
            _assert_same_collect(g, o, n2)


# ------------------------------------------------------------------------------------------ (c) the range flag
RANGE_ROW = pm.One(16, 64, 32, 4, None)


def _flag(row, img):
    (name, off, n), = [s for s in pm.segments(row) if s[0] == "split_range"]
    assert n == 4
    return int(img[off:off + 4].view(np.uint32)[0])


def test_range_flag_follows_the_synced_weights(tw, cus):
    row = RANGE_ROW
    arrs1 = pm.arrays(row, 1)
    plain = pm.torch_layout(pm.arrays(row, 2))

    def edited(key, index, value):
        st = {k: v.copy() for k, v in plain.items()}
        st[key][index] = value
        return st

    states = [("a table element of 4094", edited("embeddings.weight", (7, 5), 4094.0), True),
              ("a table element of 4095", edited("embeddings.weight", (7, 5), 4095.0), False),
              ("a common.0.weight element of -4095", edited("common.0.weight", (3, 9), -4095.0), False),
              ("action.0.weight[0][0] = 5000", edited("action.0.weight", (0, 0), 5000.0), False),
              ("a value.0.weight element of 4095", edited("value.0.weight", (0, 11), 4095.0), False),
              ("the plain weights again", plain, True)]
    pol = _build(row, arrs1)
    env = tw.env.Puzzle(2, 2, 4, 2, 256)
    E = 300
    run = lambda p, prec: tw.collector.PPOCollector(E, 0.995, 0.995, 32, merge_order=False, precision=prec).collect(env, p, seed=7)
    shape = lambda g: (g.stats["rollout_blocks"], g.stats["rollout_threads"])
    for what, st, inside in states:
        host = _build(row, pm.export_layout(st, arrs1))
        want, _ = _image(host)
        assert _flag(row, want) == (0 if inside else 1), what          # the host builder's own flag, as the kernel matrix tests it
        pol.update_from_torch(_cuda(st))
        got = _assert_image(row, pol, want, what)
        assert _flag(row, got) == (0 if inside else 1), what
        g2, h2 = run(pol, "fp16x2"), run(host, "fp16x2")
        a2, b2 = g2.to_numpy(), h2.to_numpy()
        assert shape(g2) == shape(h2), (what, g2.stats, h2.stats)
        for k in a2:
            assert np.array_equal(a2[k], b2[k]), (what, k)
        if not inside:                                                  # outside the range: the fp32 mode's bytes from the fp32 kernel
            g32 = run(pol, "fp32")
            a32 = g32.to_numpy()
            assert shape(g2) == shape(g32) == km.dispatch(km.R(2, 2, 64, 32, E), cus)[1], (what, g2.stats)
            for k in a32:
                assert np.array_equal(a2[k], a32[k]), (what, k)
    # the flag is down again: fp16x2 is back on its own kernel
    assert shape(g2) == km.dispatch(km.R(2, 2, 64, 32, E, "fp16x2"), cus)[1] != km.dispatch(km.R(2, 2, 64, 32, E), cus)[1]
    # a NaN weight has no finite pair either: the flag goes up (no collect with it; its f16 payload is not compared)
    pol.update_from_torch(_cuda(edited("common.0.weight", (30, 63), np.float32("nan"))))
    got, _ = _image(pol)
    assert _flag(row, got) == 1
    pol.update_from_torch(_cuda(plain))
    assert _flag(row, _assert_image(row, pol, want, "the plain weights after the NaN")) == 0


# ------------------------------------------------------------------------------------------ (d) the Python front end
def _module(row, state):
    """A torch module in the BasicPolicy layout -- embeddings (a Linear over the one-hot observation), and common / action /
    value as Sequential(Linear, ReLU, Linear, ..) -- holding the weights of `state`, on the GPU."""
    import torch
    nn = torch.nn

    def stack(name):
        mods, i = [], 0
        while f"{name}.{2 * i}.weight" in state:
            out_f, in_f = state[f"{name}.{2 * i}.weight"].shape
            if i:
                mods.append(nn.ReLU())
            mods.append(nn.Linear(in_f, out_f))
            i += 1
        return nn.Sequential(*mods)

    class Basic(nn.Module):
        def __init__(self):
            super().__init__()
            self.embeddings = nn.Linear(row.obs_size, row.emb)
            self.common, self.action, self.value = stack("common"), stack("action"), stack("value")

    m = Basic()
    assert sorted(m.state_dict()) == sorted(state)
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()})
    return m.cuda()


def _state_forms(row, state):
    """[(name, a state update_from_torch takes)]: the same weights in every form a trainer may hold them in."""
    import torch
    cuda = _cuda(state)
    module = _module(row, state)
    forms = [("a module", module), ("its state_dict", module.state_dict()), ("Parameters", dict(module.named_parameters())),
             ("float64", {k: v.double() for k, v in cuda.items()}), ("CPU tensors", {k: torch.tensor(v) for k, v in state.items()})]
    assert all(p.requires_grad for p in forms[2][1].values())

    def strided(t):             # the same values behind other strides: a .t() view of a transposed store, every second element of a vector
        if t.dim() == 2:
            v = t.t().contiguous().t()
        else:
            v = torch.stack([t, t + 1.0], dim=1).reshape(-1)[::2]
        assert torch.equal(v, t) and (not v.is_contiguous() or min(v.shape) == 1)
        return v

    def offset(t):              # a slice of a larger buffer: contiguous, storage offset 5
        buf = torch.full((t.numel() + 9,), 7.0, device=t.device, dtype=t.dtype)
        buf[5:5 + t.numel()] = t.reshape(-1)
        v = buf[5:5 + t.numel()].view(t.shape)
        assert v.storage_offset() == 5 and torch.equal(v, t)
        return v

    forms.append(("non-contiguous views", {k: strided(v) for k, v in cuda.items()}))
    forms.append(("slices with a storage offset", {k: offset(v) for k, v in cuda.items()}))
    return forms


FRONT_ROWS = [pm.One(16, 64, 32, 4, None), pm.Gen(9, 36, (30,), (12,), (), 4)]


@pytest.mark.parametrize("row", FRONT_ROWS, ids=_row_id)
def test_every_form_of_state_gives_the_host_built_image(tw, row):
    arrs1, arrs2 = pm.arrays(row, 1), pm.arrays(row, 2)
    pol, ref = _build(row, arrs1), _build(row, arrs2)
    want, _ = _image(ref)
    old, new = _cuda(pm.torch_layout(arrs1)), pm.torch_layout(arrs2)
    for name, form in _state_forms(row, new):
        pol.update_from_torch(old)                       # back to weight set 1: a form that syncs nothing would leave it there
        assert _first_difference(row, _image(pol)[0], want), name
        pol.update_from_torch(form)
        _assert_image(row, pol, want, name)


@pytest.mark.parametrize("row", FRONT_ROWS, ids=_row_id)
def test_refused_states_raise_and_leave_the_image_alone(tw, row):
    import torch
    arrs1, arrs2 = pm.arrays(row, 1), pm.arrays(row, 2)
    pol = _build(row, arrs1)
    held, _ = _image(pol)
    good = _cuda(pm.torch_layout(arrs2))
    last = list(good)[-1]
    assert last == "value.0.bias"
    bad = [(ValueError, "a wrong shape in the last tensor", {**good, last: torch.zeros(3).cuda()}),
           (ValueError, "a transposed weight", {**good, "common.0.weight": good["common.0.weight"].t()}),
           (ValueError, "a table of another obs_size", {**good, "embeddings.weight": torch.zeros(row.emb, row.obs_size + 1).cuda()}),
           (KeyError, "a missing key", {k: v for k, v in good.items() if k != "action.0.bias"}),
           (KeyError, "no common layer", {k: v for k, v in good.items() if not k.startswith("common.")})]
    if pm.is_generic(row):
        shallow = _cuda(pm.torch_layout(pm.arrays(row._replace(policy_layers=()), 2)))          # one action layer fewer
        deep = _cuda(pm.torch_layout(pm.arrays(row._replace(value_layers=(10,)), 2)))           # one value layer more
        bad += [(KeyError, "a stack with a layer fewer", shallow), (ValueError, "a stack with a layer more", deep)]
    else:
        deep = _cuda(pm.torch_layout(pm.arrays(pm.Gen(row.obs_size, row.emb, (row.hidden, 16), (), (), row.A), 2)))
        bad += [(ValueError, "a stack with a common layer more", deep)]
    for exc, what, state in bad:
        with pytest.raises(exc):
            pol.update_from_torch(state)
        assert not _first_difference(row, _image(pol)[0], held), what
    # the C ABI's own refusals: the other shape's entry point, and a layer count the policy does not have
    h = pol._handle()
    p = C.c_void_p(good["embeddings.bias"].data_ptr())
    n = len(pm.gen_layers(row)) if pm.is_generic(row) else 3
    ptrs = (C.c_void_p * (n + 1))(*[p.value] * (n + 1))
    if pm.is_generic(row):
        with pytest.raises(RuntimeError):
            _lib.check(_lib.lib().tw_policy_update_device(h, *[p] * 8))
        for count in (n - 1, n + 1):
            with pytest.raises(ValueError):
                _lib.check(_lib.lib().tw_policy_update_device_layers(h, p, p, ptrs, ptrs, count))
    else:
        with pytest.raises(RuntimeError):
            _lib.check(_lib.lib().tw_policy_update_device_layers(h, p, p, ptrs, ptrs, n))
    assert not _first_difference(row, _image(pol)[0], held)
    pol.update_from_torch(good)                          # and the policy still takes a good state
    _assert_image(row, pol, _image(_build(row, arrs2))[0], "a good state after the refusals")


def _conv_policy(tw, n2, conv_dim, v, hidden, seed):
    """Conv1dPolicy.to_rust() (src/twisterl/nn/policy.py:258-266): EmbeddingBag(conv_w.squeeze(2).T, zeros, True, [n2, n2], conv_dim);
    the dense table is made by EmbeddingBag.dense_table on the host."""
    emb = n2 * v
    arrs = make_policy_arrays(n2, seed=seed, emb=emb, hidden=hidden)
    conv_w = np.random.default_rng(seed).uniform(-0.3, 0.3, size=(v, n2)).astype(np.float32)        # Conv1d.weight.squeeze(2): [out][in]
    _, _, common, action, value = arrs
    seq = lambda ls: tw.nn.Sequential([tw.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    pol = tw.nn.Policy(tw.nn.EmbeddingBag(np.ascontiguousarray(conv_w.T).tolist(), np.zeros(emb, np.float32).tolist(), True, [n2, n2], conv_dim),
                       seq(common), seq(action), seq(value), [], [])
    return pol, conv_w, arrs


@pytest.mark.parametrize("conv_dim", [0, 1])
@pytest.mark.parametrize("three_d", [True, False], ids=["v_nvec_1", "v_nvec"])
def test_conv1d_layout_gives_the_image_of_the_dense_table(tw, conv_dim, three_d):
    import torch
    n2, v, hidden = 4, 16, 32
    row = pm.One(n2 * n2, n2 * v, hidden, 4, None)
    pol, _, _ = _conv_policy(tw, n2, conv_dim, v, hidden, 3)
    ref, conv_w, arrs = _conv_policy(tw, n2, conv_dim, v, hidden, 4)
    want, _ = _image(ref)
    assert want.size == pm.image_bytes(pm.segments(row)) and _first_difference(row, _image(pol)[0], want)
    state = {k: val for k, val in _cuda(pm.torch_layout(arrs)).items() if not k.startswith("embeddings.")}
    w = torch.tensor(conv_w).cuda()
    state["conv_layer.weight"] = w.unsqueeze(2) if three_d else w
    pol.update_from_torch(state)
    _assert_image(row, pol, want, f"conv_dim {conv_dim}")
    other = _conv_policy(tw, n2, 1 - conv_dim, v, hidden, 4)[0]                     # the other conv_dim is another table
    assert _first_difference(row, _image(other)[0], want)
    with pytest.raises(ValueError):
        pol.update_from_torch({**state, "conv_layer.weight": w.t()})
    with pytest.raises(KeyError):
        pol.update_from_torch({k: val for k, val in state.items() if k != "conv_layer.weight"})
    _assert_image(row, pol, want, "after the refusals")
