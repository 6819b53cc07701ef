"""GPU: the trainer hand-off (twisterl_amd/csrc/tw_trainer.hip, tw_collected_pack_trainer / tw_collected_adv_stats, twisterl_amd/trainer.py)
against float64 restatements of PPO.data_to_torch / AZ.data_to_torch (src/twisterl/rl/ppo.py:25-61, rl/az.py:28-46; tests/ref64.py).

* Environments whose obs ids follow no layout (tests/free_ids_env.py, layouts a-e through tw.env.PyEnv; 3, 4, 5, 17 and 31 actions):
  the one-hot must be the set of the ids of every record, whole collects and row windows that start and end inside a group of 8 and of
  32 rows, with the form of the kernel that ran asserted first (tw_debug_last_launch, TW_KERNEL_ONEHOT): the fast forms run on data
  known to be cell-major -- Puzzle's -- and on nothing else.
* Log-probs within (A + 8) 2^-24 + 2^-23 |want| of float64, also with a policy whose logits reach 20 .. 80; normalised advantages
  within 2^-23 (|a| + |mean|) / (std + 1e-8) + 2^-23 |want|; the statistics within 1e-9.  A result moved by less than the old
  tolerances fails these checks.
* The grid-stride loops of onehot_kernel, onehot4_kernel<8> and sum_kernel iterate (collects of more than 524,288 and 262,144 records).
* One record (std = nan, as torch), empty row ranges, an obs_size that is not the one the data was collected with.

MI355X, worst |GPU - float64| over all of it: log-probs 5.5e-7 (0.26 of the bound), normalised advantages 1.2e-6 (0.71 of the bound);
per collect in DESIGN.md §2.  The tests print theirs ([handoff-tol] ...).
"""
import functools

import numpy as np
import pytest
import torch

from tests import ref64
from tests.free_ids_env import ACTIONS, LAYOUTS, FreeIdsWalk, policy_arrays
from tests.util import amd_policy, f32_bits, make_policy_arrays, puzzle_transpose_twist

pytestmark = pytest.mark.gpu

HOT_LOGIT = 50.0          # the scaled action head: largest |logit| over the environment's states


@pytest.fixture(scope="module")
def tw():
    import twisterl_amd
    assert twisterl_amd.device_count() >= 1, "no GPU visible: the -m gpu tests need the MI355X box"
    return twisterl_amd.twisterl


def _form():
    """(nt, rows per workgroup and trip, blocks, threads) of the one-hot kernel the last hand-off launched."""
    from twisterl_amd import _lib
    info = _lib.debug_last_launch()
    assert info["family"] == _lib.TW_KERNEL_ONEHOT, info
    return info["nt"], info["nc"], info["blocks"], info["threads"]


@functools.lru_cache(maxsize=None)
def _collect(layout, hot=False):
    """About 200 episodes of a layout through PyEnv -> (CollectedData, its arrays on the host, obs_size, A).  Shared by the tests; nobody
    writes to it."""
    import twisterl_amd
    tw = twisterl_amd.twisterl
    n, obs_size, n_obs, _ = LAYOUTS[layout]
    A = ACTIONS[layout]
    arrs = policy_arrays(layout, seed=11, max_logit=HOT_LOGIT if hot else None)
    ident = list(range(obs_size))
    twists = ([ident, ident], [list(range(A)), list(range(A))]) if layout in "ac" else ((), ())     # (twist indices 0 / 1 in the records)
    env = tw.env.PyEnv(FreeIdsWalk(layout, A))
    env.difficulty = 6
    data = tw.collector.PPOCollector(200, 0.99, 0.95, 1).collect(env, amd_policy(arrs, *twists), seed=5)
    a = data.to_numpy()
    for v in a.values():
        v.setflags(write=False)
    assert a["obs"].shape == (len(data), n_obs) and a["logits"].shape == (len(data), A) and 200 <= len(data) <= 200 * 20
    return data, a, obs_size, A


def _windows(n):
    return [None, (0, 1), (5, 38), (n - 13, n), (17, n - 3), (41, 41), (0, 0), (n, n)]


# ------------------------------------------------------------------------------ the checks (what a moved result must fail)
def _check_onehot(got, obs, obs_size, label=""):
    assert got.dtype == np.float32 and np.array_equal(got, ref64.onehot_ref(obs, obs_size)), label


def _check_log_probs(got, logits, actions, A, label):
    want = ref64.log_prob_f64(logits, actions)
    dev = np.abs(got.astype(np.float64) - want)
    bound = ref64.log_prob_bound(A, want)
    i = int(np.argmax(dev / bound))
    print(f"[handoff-tol] {label}: log-prob worst |GPU - f64| {dev.max():.3e} (largest share of its bound {dev[i] / bound[i]:.3f} at want {want[i]:.4g}), "
          f"largest legal |logit| {np.abs(logits[logits > -1e9]).max():.4g}, A {A}, {len(want)} records")
    assert got.dtype == np.float32 and np.all(dev <= bound), (label, float(dev[i]), float(bound[i]), float(want[i]))
    return float(dev.max())


def _check_normalized(got, advs, label):
    want = ref64.normalized_adv_f64(advs)
    dev = np.abs(got.astype(np.float64) - want)
    bound = ref64.normalized_adv_bound(advs, want)
    i = int(np.argmax(dev / bound))
    print(f"[handoff-tol] {label}: normalised advantage worst |GPU - f64| {dev.max():.3e} (largest share of its bound {dev[i] / bound[i]:.3f}), {len(want)} records")
    assert got.dtype == np.float32 and np.all(dev <= bound), (label, float(dev[i]), float(bound[i]), float(want[i]))


def _check_adv_stats(data, advs):
    from twisterl_amd import trainer
    m, sd = trainer.adv_stats(data)
    a = np.asarray(advs, np.float64)
    assert abs(m - float(a.mean())) < 1e-9 and abs(sd - float(a.std(ddof=1))) < 1e-9, (m, sd, float(a.mean()), float(a.std(ddof=1)))


# ------------------------------------------------------------------------------ ids that follow no layout
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_one_hot_of_ids_that_follow_no_layout(tw, layout):
    """Layouts a-e, whole collects and row windows: the general form ran (memset + scatter, one thread per id), the one-hot is the set
    of each record's ids, actions / twist indices are the collect's as int64, returns and un-normalised advantages its bits."""
    from twisterl_amd import trainer
    data, a, obs_size, A = _collect(layout)
    n, n_obs = len(data), LAYOUTS[layout][2]
    assert n > 60
    if layout in "ac":
        assert set(np.unique(a["perms"])) == {0, 1}
    for rows in _windows(n):
        lo, hi = rows if rows else (0, n)
        pt_obs, pt_logp, pt_acts, pt_advs, pt_rets, pt_perm = trainer.ppo_data_to_torch(data, obs_size, rows=rows)
        if hi > lo:
            assert _form() == (0, 0, -(-(hi - lo) * n_obs // 256), 256), (rows, _form())
        assert pt_obs.shape == (hi - lo, obs_size) and pt_obs.is_cuda and pt_obs.dtype == torch.float32
        _check_onehot(pt_obs.cpu().numpy(), a["obs"][lo:hi], obs_size, (layout, rows))
        assert pt_acts.dtype == torch.int64 and np.array_equal(pt_acts.cpu().numpy(), a["actions"][lo:hi].astype(np.int64)), rows
        assert pt_perm.dtype == torch.int64 and np.array_equal(pt_perm.cpu().numpy(), a["perms"][lo:hi].astype(np.int64)), rows
        assert np.array_equal(f32_bits(pt_rets.cpu().numpy()), f32_bits(a["rets"][lo:hi])), rows
        assert np.array_equal(f32_bits(pt_advs.cpu().numpy()), f32_bits(a["advs"][lo:hi])), rows
        assert pt_logp.shape == (hi - lo,)


def test_self_play_data_of_a_python_environment(tw):
    """az_data_to_torch on a self-play collect of layout b (three ids of 27 anywhere, repeats): general form, the set of ids."""
    from twisterl_amd import trainer
    env = tw.env.PyEnv(FreeIdsWalk("b", ACTIONS["b"]))
    env.difficulty = 4
    az = tw.collector.AZCollector(24, 4, 1.41, 1, 1).collect(env, amd_policy(policy_arrays("b", seed=11)), seed=2)
    b = az.to_numpy()
    n = len(az)
    assert n >= 24
    for rows in (None, (3, n - 2), (n, n)):
        lo, hi = rows if rows else (0, n)
        o, p, v = trainer.az_data_to_torch(az, 27, rows=rows)
        if hi > lo:
            assert _form() == (0, 0, -(-(hi - lo) * 3 // 256), 256)
        _check_onehot(o.cpu().numpy(), b["obs"][lo:hi], 27)
        assert np.array_equal(f32_bits(p.cpu().numpy()), f32_bits(b["logits"][lo:hi])) and v.shape == (hi - lo, 1)
        assert np.array_equal(f32_bits(v.cpu().numpy()[:, 0]), f32_bits(b["remaining_values"][lo:hi]))


# ------------------------------------------------------------------------------ log-probs and normalised advantages
@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_log_probs_against_float64(tw, layout, hot):
    """|got - log_prob_f64| <= (A + 8) 2^-24 + 2^-23 |want| for 3, 4, 5, 17 and 31 actions, masked actions included, with the plain
    policy and with one whose logits reach 20 .. 80 (`hot`).

    torch's own f32 Categorical(logits).log_prob on the same logits stays inside this bound with the plain policies (MI355X collects:
    at most 0.23 of it); with the hot ones it does not: worst deviation 1.83e-6 = 2.8 times the bound, on a log-prob of -5.6e-5
    (layout b; a 1.4, c 1.3 times; random logits of size 30 on the CPU, tests/test_ref64.py: up to 3.8 times).  The cause is torch's
    form, not the bound: torch computes logits - logsumexp(logits), which rounds at the size of the logits (2^-24 x 48 = 2.9e-6), the
    kernel (l[a] - max) - log(sum), which rounds at the size of the result.  Twice torch's worst as the constant term would be 3.7e-6,
    six times what the kernel needs (its worst: 5.5e-7, 0.26 of the bound).  So the kernel is held to the bound as stated, and torch to
    the bound of its own form (ref64.log_prob_bound(..., lse): 2^-23 |logsumexp| more)."""
    from twisterl_amd import trainer
    data, a, obs_size, A = _collect(layout, hot)
    n = len(data)
    legal = a["logits"] > -1e9
    assert legal.any(axis=1).all() and not legal.all() and legal[np.arange(n), a["actions"]].all()
    if hot:
        assert 20.0 <= np.abs(a["logits"][legal]).max() <= 80.0, np.abs(a["logits"][legal]).max()
    got = trainer.ppo_data_to_torch(data, obs_size)[1].cpu().numpy()
    _check_log_probs(got, a["logits"], a["actions"], A, f"layout {layout} {'hot' if hot else 'plain'}")
    lo, hi = 17, n - 3
    assert np.array_equal(f32_bits(trainer.ppo_data_to_torch(data, obs_size, rows=(lo, hi))[1].cpu().numpy()), f32_bits(got[lo:hi]))
    want = ref64.log_prob_f64(a["logits"], a["actions"])
    t32 = torch.distributions.Categorical(logits=torch.tensor(a["logits"])).log_prob(torch.tensor(a["actions"].astype(np.int64))).numpy()
    dev = np.abs(t32.astype(np.float64) - want)
    print(f"[handoff-tol] layout {layout} {'hot' if hot else 'plain'}: torch f32 Categorical worst |f32 - f64| {dev.max():.3e}, "
          f"largest share of the kernel's bound {np.max(dev / ref64.log_prob_bound(A, want)):.3f}")
    assert np.all(dev <= ref64.log_prob_bound(A, want, lse=0.0 if not hot else ref64.logsumexp_f64(a["logits"])))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_normalised_advantages_against_float64(tw, layout):
    from twisterl_amd import trainer
    data, a, obs_size, A = _collect(layout)
    n = len(data)
    got = trainer.ppo_data_to_torch(data, obs_size, normalize_advantage=True)[3].cpu().numpy()
    _check_normalized(got, a["advs"], f"layout {layout}")
    _check_adv_stats(data, a["advs"])
    for lo, hi in ((5, 38), (n - 13, n)):             # a window: the statistics are still those of the whole collect
        mb = trainer.ppo_data_to_torch(data, obs_size, normalize_advantage=True, rows=(lo, hi))[3].cpu().numpy()
        assert np.array_equal(f32_bits(mb), f32_bits(got[lo:hi]))


def test_a_moved_result_fails_the_checks(tw):
    """One log-prob moved by 1e-5, one normalised advantage moved by 1e-4 (either way; at the smallest, the largest and a middle
    value), a one of the one-hot cleared and a zero set: each copy of the GPU's result fails its check; the result itself passes."""
    from twisterl_amd import trainer
    data, a, obs_size, A = _collect("c")
    out = trainer.ppo_data_to_torch(data, obs_size, normalize_advantage=True)
    oh, logp, norm = out[0].cpu().numpy(), out[1].cpu().numpy(), out[3].cpu().numpy()
    _check_onehot(oh, a["obs"], obs_size)
    _check_log_probs(logp, a["logits"], a["actions"], A, "layout c (moved-result test)")
    _check_normalized(norm, a["advs"], "layout c (moved-result test)")
    want_lp = ref64.log_prob_f64(a["logits"], a["actions"])
    for i in (int(np.argmin(np.abs(want_lp))), int(np.argmax(np.abs(want_lp))), len(logp) // 2):
        for d in (1e-5, -1e-5):
            bad = logp.copy()
            bad[i] = np.float32(np.float64(bad[i]) + d)
            assert bad[i] != logp[i]
            with pytest.raises(AssertionError):
                _check_log_probs(bad, a["logits"], a["actions"], A, "moved")
    for i in (int(np.argmin(np.abs(norm))), int(np.argmax(np.abs(norm))), len(norm) // 2):
        for d in (1e-4, -1e-4):
            bad = norm.copy()
            bad[i] = np.float32(np.float64(bad[i]) + d)
            with pytest.raises(AssertionError):
                _check_normalized(bad, a["advs"], "moved")
    r = len(oh) // 3
    for col in (int(a["obs"][r, 0]), int(np.flatnonzero(oh[r] == 0)[0])):       # a one cleared, a zero set
        bad = oh.copy()
        bad[r, col] = 1.0 - bad[r, col]
        with pytest.raises(AssertionError):
            _check_onehot(bad, a["obs"], obs_size)


# ------------------------------------------------------------------------------ the grid-stride loops
def _device_onehot(t_obs, lo, hi, obs_size):
    ref = torch.zeros((hi - lo, obs_size), dtype=torch.float32, device=t_obs.device)
    return ref.scatter_(1, t_obs[lo:hi].long(), 1.0)


def test_loops_of_the_one_row_form_and_of_the_sums_iterate(tw):
    """Puzzle-8 (81 ids: nine blocks of nine -- onehot_kernel), more than 524,288 records: 8,192 workgroups of four rows cover 32,768
    rows per trip, sum_kernel's 2,048 workgroups 524,288 records per trip.  Whole collect, normalised."""
    from twisterl_amd import trainer
    E = 16_384
    arrs = make_policy_arrays(9, seed=3, emb=64, hidden=32)
    data = tw.collector.PPOCollector(E, 0.995, 0.995, 1).collect(tw.env.Puzzle(3, 3, 32, 2, 256), amd_policy(arrs, *puzzle_transpose_twist(3)), seed=9)
    n = len(data)
    assert n > 524_288, n
    t = data.to_torch()
    pt_obs, pt_logp, pt_acts, pt_advs, pt_rets, pt_perm = trainer.ppo_data_to_torch(data, 81, normalize_advantage=True)
    assert _form() == (1, 4, 8192, 256) and n > 8192 * 4
    assert torch.equal(pt_obs, _device_onehot(t["obs"], 0, n, 81))
    assert torch.equal(pt_acts, t["actions"].long()) and torch.equal(pt_perm, t["perms"].long()) and torch.equal(pt_rets, t["rets"])
    logits, actions, advs = t["logits"].cpu().numpy(), t["actions"].cpu().numpy(), t["advs"].cpu().numpy()
    _check_log_probs(pt_logp.cpu().numpy(), logits, actions, 4, f"Puzzle-8, {n} records")
    _check_normalized(pt_advs.cpu().numpy(), advs, f"Puzzle-8, {n} records")
    _check_adv_stats(data, advs)


def test_loop_of_the_eight_row_form_iterates(tw):
    """Puzzle-15 (16 blocks of 16 ids -- onehot4_kernel<8>): a window of 262,144 + 8 * 4 * 3 + 5 rows from row 7 -- 8,192 workgroups of
    32 rows cover 262,144 per trip; the second trip has three whole groups and one of five rows."""
    from twisterl_amd import trainer
    arrs = make_policy_arrays(16, seed=4, emb=64, hidden=32)
    data = tw.collector.PPOCollector(4096, 0.995, 0.995, 1).collect(tw.env.Puzzle(4, 4, 40, 2, 256), amd_policy(arrs, *puzzle_transpose_twist(4)), seed=10)
    rows = 262_144 + 8 * 4 * 3 + 5
    n = len(data)
    assert n > 262_144 + 100 and n >= 7 + rows, n
    t = data.to_torch()
    out = trainer.ppo_data_to_torch(data, 256, rows=(7, 7 + rows))
    assert _form() == (4, 32, 8192, 256)
    assert out[0].shape == (rows, 256) and torch.equal(out[0], _device_onehot(t["obs"], 7, 7 + rows, 256))
    assert torch.equal(out[2], t["actions"][7:7 + rows].long()) and torch.equal(out[3], t["advs"][7:7 + rows])


# ------------------------------------------------------------------------------ edges
def test_one_record(tw):
    """One episode that starts solved: one record.  Its std is nan and so are its normalised advantages (torch.std of one element);
    everything else is exact."""
    from twisterl_amd import trainer
    arrs = make_policy_arrays(9, seed=3, emb=64, hidden=32)
    data = tw.collector.PPOCollector(1, 0.99, 0.95, 1).collect(tw.env.Puzzle(3, 3, 0, 2, 256), amd_policy(arrs), seed=1)
    assert len(data) == 1
    a = data.to_numpy()
    m, sd = trainer.adv_stats(data)
    assert m == float(np.float64(a["advs"][0])) and np.isnan(sd)
    pt_obs, pt_logp, pt_acts, pt_advs, pt_rets, pt_perm = trainer.ppo_data_to_torch(data, 81, normalize_advantage=True)
    assert _form() == (1, 4, 1, 256)
    assert np.isnan(pt_advs.cpu().numpy()).all() and pt_advs.shape == (1,)
    _check_onehot(pt_obs.cpu().numpy(), a["obs"], 81)
    _check_log_probs(pt_logp.cpu().numpy(), a["logits"], a["actions"], 4, "one record")
    assert pt_acts.cpu().numpy().tolist() == a["actions"].astype(np.int64).tolist() and pt_perm.cpu().numpy().tolist() == a["perms"].astype(np.int64).tolist()
    assert np.array_equal(f32_bits(pt_rets.cpu().numpy()), f32_bits(a["rets"]))
    plain = trainer.ppo_data_to_torch(data, 81)[3].cpu().numpy()
    assert np.array_equal(f32_bits(plain), f32_bits(a["advs"]))


def test_an_obs_size_the_data_was_not_collected_with_is_refused(tw):
    """One below and one above the recorded value, Puzzle data and layout c: refused on the host, before anything is launched, naming
    both numbers (TW_ERR_INVALID: ValueError, the library's convention for a bad argument).  The right value still works afterwards."""
    from twisterl_amd import trainer
    arrs = make_policy_arrays(9, seed=3, emb=64, hidden=32)
    puzzle = tw.collector.PPOCollector(20, 0.99, 0.95, 1).collect(tw.env.Puzzle(3, 3, 4, 2, 256), amd_policy(arrs), seed=1)
    az = tw.collector.AZCollector(6, 3, 1.41, 1, 1).collect(tw.env.Puzzle(3, 3, 3, 2, 256), amd_policy(arrs), seed=1)
    free = _collect("c")[0]
    for data, size, fn in ((puzzle, 81, trainer.ppo_data_to_torch), (free, 50, trainer.ppo_data_to_torch), (az, 81, trainer.az_data_to_torch)):
        for wrong in (size - 1, size + 1):
            with pytest.raises(ValueError, match=rf"obs_size {wrong}\b.*obs_size {size}\b"):
                fn(data, wrong)
            with pytest.raises(ValueError, match=rf"obs_size {wrong}\b.*obs_size {size}\b"):
                fn(data, wrong, rows=(1, 2))
        a = data.to_numpy()
        _check_onehot(fn(data, size)[0].cpu().numpy(), a["obs"], size)
    for wrong in (256, 257, 300):                          # (above 256 there is no one-hot form at all)
        with pytest.raises(ValueError, match=f"obs_size {wrong}"):
            trainer.ppo_data_to_torch(free, wrong)
