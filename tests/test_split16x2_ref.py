"""CPU: the numpy restatement of the split-f16 forward of generic stacks (tests/split16x2_ref.py) against the a-priori float64
bound, before a GPU is touched.  On every policy tests/test_gpu_device_env_fp16x2.py runs, over seeded records with every twist: the
emulation lies inside tests/ref64.forward_f64_bound(mode="fp16x2"), and every operand is inside the split's range (shown from the
weights alone).  The bound can fail: with any one of the three products left out it is violated.  The exactness probe's
construction is exact: emulation == the oracle's f32 arithmetic (both orders) == float64, bit for bit, and differs from the oracle's
ARITH_F16.  And the split itself: 4094 has a finite pair of terms, 4095, -4095, 5000 and NaN have none."""
import numpy as np
import pytest

from tests import ref64, split16x2_ref as S
from tests.util import f32_bits, oracle_policy

N = 48


def _records(name, n_obs, obs_size, A, n_perms, seed=0):
    rng = np.random.default_rng(1000 + seed)
    obs = rng.integers(0, obs_size, size=(N, n_obs))
    if name.endswith("v"):                                   # observations of variable length: free slots behind the ids
        keep = rng.integers(0, n_obs + 1, size=N)
        obs = np.where(np.arange(n_obs)[None, :] < keep[:, None], obs, -1)
    masks = rng.random((N, A)) < 0.7
    masks[np.arange(N), rng.integers(0, A, size=N)] = True
    perms = rng.integers(-1, n_perms, size=N) if n_perms else np.full(N, -1)
    return obs, masks, perms


def _n_actions(arrs):
    return int(np.asarray(arrs[3][-1][1]).size)


CASES = S.all_policies()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_emulation_lies_inside_the_bound(case):
    name, arrs, tw, n_obs, obs_size = case
    wmax, top = S.weight_ceiling(arrs, n_obs)
    assert wmax < S.LIMIT and top < S.LIMIT, (name, wmax, top)          # the bound's range, from the weights alone
    obs, masks, perms = _records(name, n_obs, obs_size, _n_actions(arrs), len(tw[0]))
    fed = []
    lg, v = S.forward(arrs, tw[0], tw[1], obs, masks, perms, fed=fed)
    assert all(S.in_range(x) for x in fed) and float(max(np.abs(x).max() for x in fed)) <= top
    l64, v64, el, ev = ref64.forward_f64_bound(arrs, tw[0], tw[1], obs, masks, perms, "fp16x2")
    dl = np.abs(lg.astype(np.float64) - l64)
    assert (dl[masks] <= el[masks]).all(), (name, float((dl - el)[masks].max()))
    assert (np.abs(v.astype(np.float64) - v64) <= ev).all(), name
    assert np.array_equal(lg[~masks], np.full((~masks).sum(), np.float32(-1e10)))


@pytest.mark.parametrize("drop", [0, 1, 2])
def test_the_bound_fails_without_one_of_the_three_products(drop):
    violated = []
    for name, arrs, tw, n_obs, obs_size in CASES:
        obs, masks, perms = _records(name, n_obs, obs_size, _n_actions(arrs), len(tw[0]))
        lg, v = S.forward(arrs, tw[0], tw[1], obs, masks, perms, drop=drop)
        l64, v64, el, ev = ref64.forward_f64_bound(arrs, tw[0], tw[1], obs, masks, perms, "fp16x2")
        if (np.abs(lg.astype(np.float64) - l64)[masks] > el[masks]).any() or (np.abs(v.astype(np.float64) - v64) > ev).any():
            violated.append(name)
    assert violated, drop
    if drop == 0:
        assert len(violated) == len(CASES)


def test_the_exactness_probe_is_exact():
    from oracle import oracle as O
    O.build()
    arrs = S.exact_arrays()
    emb, eb, common, action, value = arrs
    obs, masks, perms = _records("gw3_exact", S.GW_N_OBS, S.GW_OBS_SIZE, 4, 0, seed=7)
    fed = []
    lg, v = S.forward(arrs, (), (), obs, masks, perms, fed=fed)
    # the construction: an integer embedding (lo zero), layer-1 weights with lo terms, later layers with integer weights (lo zero) over
    # fractional activations (lo not zero); every |w| |x| sum below 2^11 in multiples of 2^-12: exact in f32 in any order
    assert np.array_equal(fed[0], np.round(fed[0])) and not S.split(fed[0])[1].any()
    assert S.split(common[0][0])[1].any()
    for w, _, _ in common[1:] + action + value:
        assert np.array_equal(w, np.round(w)) and not S.split(w)[1].any()
    assert S.split(fed[1])[1].any() and S.split(fed[2])[1].any() and float(fed[2].max()) > 0
    x = fed[0].astype(np.float64)
    for (w, b, _), a in zip(common + action, fed[1:] + [None]):
        W = np.abs(np.asarray(w, np.float64).reshape(-1, len(b)))
        assert float((np.abs(x) @ W + np.abs(b)).max()) < 2.0 ** 11
        if a is not None:
            x = a.astype(np.float64)
            assert np.array_equal(x * 4096, np.round(x * 4096)) and float(np.abs(x).max()) < 1024    # 16 x spans at most 22 bits: hi + lo == 16 x
            hi, lo = S.split(a)
            assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), 16.0 * x)
    l64, v64 = ref64.forward_f64(arrs, (), (), obs, masks, perms)
    assert np.array_equal(lg.astype(np.float64), l64) and np.array_equal(v.astype(np.float64), v64)
    op = oracle_policy(O, arrs)
    for arith in (O.ARITH_CHAIN, O.ARITH_REF):
        lo_, vo = op.forward_batch(obs, masks, perms, arith=arith)
        assert np.array_equal(f32_bits(lo_), f32_bits(lg)) and np.array_equal(f32_bits(vo), f32_bits(v)), arith
    l16, v16 = op.forward_batch(obs, masks, perms, arith=O.ARITH_F16)
    assert (l16 != lg)[masks].any() and (v16 != v).any()


def test_the_split_and_its_range():
    hi, lo = S.split(np.float32([4094.0, 1.0 + 2.0 ** -12, 0.1, -3.3]))
    assert np.isfinite(hi.astype(np.float32)).all() and float(hi[0]) == 65504.0 and float(lo[1]) == 2.0 ** -8
    x = np.float32([0.1, -3.3, 4094.0])
    rel = np.abs(hi[[2, 3, 0]].astype(np.float64) + lo[[2, 3, 0]].astype(np.float64) - 16.0 * x.astype(np.float64)) / (16.0 * np.abs(x))
    assert (rel <= 2.0 ** -22).all()
    assert S.in_range(np.float32([4094.0, -4094.0, 4094.99]))
    for bad in (4095.0, -4095.0, 5000.0, np.nan, np.inf):
        assert not S.in_range(np.float32([bad])), bad
        assert not np.isfinite(S.split(np.float32([bad]))[0].astype(np.float32)).all()
