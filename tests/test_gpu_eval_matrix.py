"""policy_eval_kernel and policy_eval_generic_kernel (tw_eval.hip), row by row of tests/eval_matrix.py, through
Policy.evaluate_batch -> tw_policy_evaluate: all three modes, with and without a perms array, bit for bit against the oracle
(ARITH_CHAIN, the deterministic exp) and, for the in-range rows, inside the float64 bounds of tests/ref64.py."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_matrix as M
from tests.eval_matrix import FORWARD, FULL_PREDICT, PREDICT
from tests.util import f32_bits
from twisterl_amd import _lib

pytestmark = pytest.mark.gpu

ids = lambda rows: [r.name for r in rows]


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


_policies = {}


def gpu_policy(row):
    if row.name not in _policies:
        _policies[row.name] = M.amd_policy(row)
    return _policies[row.name]


def evaluate(row, obs=None, masks=None, perms=None):
    """{(mode, with_perms): (out, values)} of the row's policy on the GPU, on the row's records or the given ones"""
    o, m, p = M.records(row)
    obs, masks, perms = (o if obs is None else obs), (m if masks is None else masks), (p if perms is None else perms)
    pol = gpu_policy(row)
    return {(mode, wp): pol.evaluate_batch(mode, obs, masks, perms if wp else None) for mode, wp in M.cases()}


def same_bits(a, b):
    return np.array_equal(f32_bits(a[0]), f32_bits(b[0])) and np.array_equal(f32_bits(a[1]), f32_bits(b[1]))


def assert_oracle_bits(got, want, what):
    for key in M.cases():
        (o, v), (wo, wv) = got[key], want[key]
        bad_o, bad_v = f32_bits(o) != f32_bits(wo), f32_bits(v) != f32_bits(wv)
        with np.errstate(invalid="ignore"):
            print(f"{what} {key}: {int(bad_o.sum())} of {o.size} outputs and {int(bad_v.sum())} of {v.size} values differ from the oracle's bits; "
                  f"max |diff| {np.nanmax(np.abs(o.astype(np.float64) - wo), initial=0.0):.3g} / {np.nanmax(np.abs(v.astype(np.float64) - wv), initial=0.0):.3g}")
        assert not bad_o.any(), (what, key, np.argwhere(bad_o)[:4].tolist(), o[bad_o][:4], wo[bad_o][:4])
        assert not bad_v.any(), (what, key, np.argwhere(bad_v)[:4].tolist(), v[bad_v][:4], wv[bad_v][:4])


@pytest.mark.parametrize("row", M.TABLE, ids=ids(M.TABLE))
def test_every_row_matches_the_oracle_and_float64(tw, oracle, row):
    got = evaluate(row)
    _, masks, _ = M.records(row)
    legal = masks != 0
    dead = ~legal.any(axis=1)
    assert_oracle_bits(got, M.oracle_results(oracle, row), row.name)
    for key in M.cases():
        o, v = got[key]
        if key[0] == FORWARD:
            assert np.all(f32_bits(o[~legal]) == f32_bits(np.float32(-1e10)))       # masked logits are exactly -1e10
        else:
            assert np.all(f32_bits(o[~legal]) == 0)                                  # masked probabilities exactly +0
            assert np.all(f32_bits(o[dead]) == 0)                                    # no legal action: 0 / (0 + 1e-6) everywhere
        assert np.isfinite(v[dead]).all()
    assert same_bits(got[(FULL_PREDICT, True)], got[(FULL_PREDICT, False)])         # FULL_PREDICT ignores a perms array
    if row.in_range:
        want = M.f64_results(row)
        for key in M.cases():
            (o, v), (wo, wv, bo, bv) = got[key], want[key]
            do, dv = np.abs(o.astype(np.float64) - wo), np.abs(v.astype(np.float64) - wv)
            print(f"{row.name} {key}: max |gpu - float64| {do.max():.3g} (bound there {bo.reshape(-1)[do.argmax()]:.3g}) / {dv.max():.3g} ({bv[dv.argmax()]:.3g})")
            assert np.isfinite(o).all() and np.isfinite(v).all()
            assert np.all(do <= bo), (row.name, key, do.max())
            assert np.all(dv <= bv), (row.name, key, dv.max())


NEIGHBOUR_ROWS = [M.BY_NAME[n] for n in ("basic-a5", "basic-ragged", "basic-emb288-a5", "generic-a31", "generic-obs300-tw3-ragged", "generic-w300")]


@pytest.mark.parametrize("row", NEIGHBOUR_ROWS, ids=ids(NEIGHBOUR_ROWS))
def test_a_block_does_not_depend_on_its_neighbours(tw, oracle, row):
    """One workgroup per record: a batch of one record, and one of 300 with the row's records repeated, give every record the
    bytes it has in the row's own batch."""
    obs, masks, perms = M.records(row)
    base = evaluate(row)
    one = evaluate(row, obs[:1], masks[:1], perms[:1])
    idx = (np.arange(300) * 7) % row.n                                    # (7 and n = 16 are coprime: every record, never beside the same neighbour twice)
    many = evaluate(row, obs[idx], masks[idx], perms[idx])
    for key in M.cases():
        assert same_bits(one[key], (base[key][0][:1], base[key][1][:1])), key
        assert same_bits(many[key], (base[key][0][idx], base[key][1][idx])), key
    assert_oracle_bits(base, M.oracle_results(oracle, row), row.name)


SINGLE_ROWS = [M.BY_NAME[n] for n in ("basic-tw3", "basic-notwist", "generic-a5", "generic-ragged", "generic-notwist")]


@pytest.mark.parametrize("row", SINGLE_ROWS, ids=ids(SINGLE_ROWS))
def test_the_single_observation_methods_return_the_batch_s_row(tw, row):
    obs, masks, _ = M.records(row)
    pol = gpu_policy(row)
    T = len(M.twists(row)[0])
    for i in (0, 1, row.n - 1):
        for perm in ([None] if T == 0 else range(T)):
            perms = None if perm is None else np.full(row.n, perm, np.int32)
            for mode, method in ((FORWARD, pol.forward), (PREDICT, pol.predict)):
                a, v = pol.evaluate_batch(mode, obs, masks, perms)
                sa, sv = method(obs[i].tolist(), [bool(m) for m in masks[i]], perm=perm)
                assert np.array_equal(f32_bits(sa), f32_bits(a[i])) and f32_bits(sv) == f32_bits(v[i]), (i, perm, mode)
        a, v = pol.evaluate_batch(FULL_PREDICT, obs, masks)
        sa, sv = pol.full_predict(obs[i].tolist(), [bool(m) for m in masks[i]])
        assert np.array_equal(f32_bits(sa), f32_bits(a[i])) and f32_bits(sv) == f32_bits(v[i]), i


REFUSAL_ROWS = [M.BY_NAME[n] for n in ("basic-tw2", "generic-tw2")]


@pytest.mark.parametrize("row", REFUSAL_ROWS, ids=ids(REFUSAL_ROWS))
def test_refusals_leave_nothing_behind(tw, oracle, row):
    """Every refusal is a check of tw_policy_evaluate (or of Policy.evaluate_batch) on the host, before anything is allocated or
    launched: the library's error is raised, and the valid call that follows is bit-equal to the oracle."""
    obs, masks, perms = M.records(row)
    pol = gpu_policy(row)
    want = M.oracle_results(oracle, row)
    n, A = row.n, M.n_actions(row)

    def still_good():
        assert_oracle_bits(evaluate(row), want, row.name)

    def with_id(bad):
        o = obs.copy()
        o[n // 2, row.n_obs - 1] = bad
        return o

    bad_perms = perms.copy()
    bad_perms[n - 1] = len(M.twists(row)[0])
    refused = [
        ("n_obs 0", lambda m: pol.evaluate_batch(m, np.zeros((n, 0), np.int32), masks, perms), "n_obs"),
        ("n_obs 65", lambda m: pol.evaluate_batch(m, np.zeros((n, 65), np.int32), masks, perms), "n_obs"),
        ("id -2", lambda m: pol.evaluate_batch(m, with_id(-2), masks, perms), "obs id"),
        ("id obs_size", lambda m: pol.evaluate_batch(m, with_id(row.obs_size), masks, perms), "obs id"),
        ("perm n_perms", lambda m: pol.evaluate_batch(m, obs, masks, bad_perms), "perm index"),
        ("masks too narrow", lambda m: pol.evaluate_batch(m, obs, masks[:, : A - 1], perms), "masks"),
        ("masks too wide", lambda m: pol.evaluate_batch(m, obs, np.concatenate([masks, masks], axis=1), perms), "masks"),
    ]
    for what, call, text in refused:
        for mode in (FORWARD, PREDICT, FULL_PREDICT):
            with pytest.raises(ValueError, match=text):
                call(mode)
        still_good()
    for mode in (-1, 3):
        with pytest.raises(ValueError, match="bad mode"):
            pol.evaluate_batch(mode, obs, masks, perms)
    still_good()
    out_a, out_v = np.empty((n, A), np.float32), np.empty(n, np.float32)
    for prec in (_lib.TW_PREC_F16, _lib.TW_PREC_F16X2, 7):
        rc = _lib.lib().tw_policy_evaluate(pol._handle(), FORWARD, prec, obs.ctypes.data_as(C.POINTER(C.c_int32)), n, row.n_obs,
                                           masks.ctypes.data_as(C.POINTER(C.c_uint8)), None, out_a.ctypes.data_as(C.POINTER(C.c_float)),
                                           out_v.ctypes.data_as(C.POINTER(C.c_float)))
        with pytest.raises(RuntimeError, match="TW_PREC_F32_EXACT"):
            _lib.check(rc)
    still_good()


def test_thirty_two_actions_are_refused_when_the_policy_is_made(tw):
    """EVAL_MAX_ACT is 32 and thread `A` computes the value: 31 actions are the most; tw_policy_create refuses 32 on the host."""
    from tests.util import make_deep_policy_arrays_obs, make_policy_arrays_obs
    from twisterl_amd import twisterl
    seq = lambda ls: twisterl.nn.Sequential([twisterl.nn.Linear(w.tolist(), b.tolist(), r) for (w, b, r) in ls])
    for arrs in (make_policy_arrays_obs(40, seed=1, emb=32, hidden=32, n_actions=32),
                 make_deep_policy_arrays_obs(40, seed=1, emb=32, common=(24,), n_actions=32)):
        emb, eb, common, action, value = arrs
        pol = twisterl.nn.Policy(twisterl.nn.EmbeddingBag(emb.tolist(), eb.tolist(), True, [40], 0), seq(common), seq(action), seq(value), [], [])
        with pytest.raises(RuntimeError, match="n_actions"):
            pol.evaluate_batch(FORWARD, np.zeros((1, 5), np.int32), np.ones((1, 32), np.uint8))


def test_the_two_kernels_give_the_same_bytes_on_the_same_weights(tw, oracle):
    """cross-basic is an is_mfma_shape policy (policy_eval_kernel); cross-generic is the same policy with an embedding table of 257
    rows, the last 217 named by no record (obs_size > 256: policy_eval_generic_kernel, and the two-byte twist table).  Same
    weights, same records: the same bytes in all three modes, and both the oracle's."""
    b, g = M.BY_NAME["cross-basic"], M.BY_NAME["cross-generic"]
    assert M.is_basic_shape(b) and not M.is_basic_shape(g)
    rb, rg = evaluate(b), evaluate(g)
    for key in M.cases():
        assert same_bits(rb[key], rg[key]), key
    assert_oracle_bits(rb, M.oracle_results(oracle, b), b.name)
    assert_oracle_bits(rg, M.oracle_results(oracle, g), g.name)
