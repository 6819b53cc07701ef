"""CPU: tests/free_ids_env.py, the environment the trainer hand-off tests collect from, does what its layouts say: ids, masks,
episode lengths, determinism -- and none of its layouts is the cell-major one the fast one-hot kernels assume."""
import numpy as np
import pytest

from tests.free_ids_env import ACTIONS, LAYOUTS, FreeIdsWalk, all_states, policy_arrays


def _episode(env, seed, episode, difficulty, pick):
    env.seed_episode(seed, episode)
    env.reset(difficulty)
    recs = []
    while True:
        recs.append((env.observe(), env.masks(), env.value()))
        if env.is_final():
            return recs
        legal = [k for k, m in enumerate(env.masks()) if m]
        env.next(legal[pick(len(recs)) % len(legal)])


def test_action_counts_of_the_layouts():
    assert sorted(ACTIONS) == sorted(LAYOUTS) == list("abcde")
    assert sorted(ACTIONS.values()) == [3, 4, 5, 17, 31]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ids_masks_and_lengths(layout):
    n, obs_size, n_obs, _ = LAYOUTS[layout]
    A = ACTIONS[layout]
    env = FreeIdsWalk(layout, A)
    assert env.obs_shape() == [obs_size] and env.num_actions() == A and env.max_records == 20
    obs, masks = all_states(layout, stride=1 if n <= 64 else 5)
    assert obs.shape[1] == n_obs and masks.shape[1] == A
    assert obs.min() == 0 and obs.max() == obs_size - 1                      # the whole range, both ends
    assert masks.any(axis=1).all() and not masks.all()                       # a legal action everywhere, never all of them everywhere
    env.set_state([1, 0])
    assert env.masks() == [k == 1 for k in range(A)]                         # ... and a position with exactly one
    repeats = np.array([len(set(o)) < len(o) for o in obs.tolist()])
    assert repeats.any() == (layout != "a") and (layout != "e" or repeats.all())
    if layout in "bcd":
        assert not repeats.all()
    # not the layout of Puzzle / GridWorld / RingWalk: position k does not hold an id of [k * n2, (k + 1) * n2)
    if obs_size % n_obs == 0:
        n2 = obs_size // n_obs
        assert (obs // n2 != np.arange(n_obs)).any(axis=1).mean() > 0.9
    if layout == "a":
        env.set_state([3, 7])
        assert env.observe() == [32 + 7, 3]
    lens, solved_at_start = [], 0
    for e in range(200):
        recs = _episode(FreeIdsWalk(layout, A), 11, e, 6, lambda t: 7 * t + e)
        again = _episode(FreeIdsWalk(layout, A), 11, e, 6, lambda t: 7 * t + e)
        assert recs == again                                                # nothing random beyond the seeded start
        lens.append(len(recs))
        solved_at_start += len(recs) == 1
        assert recs[-1][2] in (1.0, -0.5) and all(-0.5 <= r[2] < 0 for r in recs[:-1])
    assert 1 <= min(lens) and max(lens) <= 20 and len(set(lens)) >= 4 and solved_at_start >= 1
    c = env.copy()
    c.next(0)
    assert c.observe() != env.observe() or c.steps_left != env.steps_left


def test_policies_fit_the_layouts_and_the_scaled_head_is_the_same_policy_otherwise():
    from tests.ref64 import forward_f64
    for layout in sorted(LAYOUTS):
        n, obs_size, n_obs, _ = LAYOUTS[layout]
        arrs, hot = policy_arrays(layout, seed=3), policy_arrays(layout, seed=3, max_logit=50.0)
        assert arrs[0].shape == (obs_size, 64) and arrs[3][-1][1].size == ACTIONS[layout]
        obs, masks = all_states(layout, stride=max(1, n // 64))
        l0, v0 = forward_f64(arrs, [], [], obs, masks, np.full(len(obs), -1))
        l1, v1 = forward_f64(hot, [], [], obs, masks, np.full(len(obs), -1))
        assert np.array_equal(v0, v1) and abs(np.abs(l1[masks]).max() - 50.0) < 1e-3 and np.abs(l0[masks]).max() < 20.0
