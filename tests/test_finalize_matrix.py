"""CPU: tests/finalize_matrix.py's table reaches every form of the collectors' tail, both sides of every switch of the restated launch
rules, a second grid-stride trip of every capped kernel and a second trip of the scan's carry loop; its float32 GAE reference equals
the oracle bit for bit and lies inside the float64 bound; its restated constants are the ones in the sources."""
import os
import re

import numpy as np
import pytest

from tests import finalize_matrix as fm
from tests import ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twisterl_amd", "csrc")


def _forms(cases):
    return {(fm.case_dispatch(c)["form"], fm.case_dispatch(c)["waves"]) for c in cases}


def test_restated_constants_are_the_sources():
    fin = open(os.path.join(CSRC, "tw_finalize.hip")).read()
    mcts = open(os.path.join(CSRC, "tw_mcts.hip")).read()
    assert re.search(r"constexpr int SCAN_THREADS = (\d+);", fin).group(1) == str(fm.SCAN_THREADS)
    assert re.search(r"constexpr int SCAN_ITEMS\s+= (\d+);", fin).group(1) == str(fm.SCAN_ITEMS)
    assert "base += SCAN_THREADS" in fin                                  # the carry loop's step
    assert re.search(r"constexpr int FIN_WAVES = (\d+);", fin).group(1) == str(fm.FIN_WAVES)
    assert re.search(r"constexpr int AZF_WAVES = (\d+);", mcts).group(1) == str(fm.AZF_WAVES)
    assert "blocks > 256ull * 16" in fin and "blocks > 256ull * 16" in mcts and "256ull * per_cu * 2" in fin
    assert "(n_cells == 16 ? 5 : 9)" in fin and "(t_pad | 1) * 8" in fin
    header = open(os.path.join(ROOT, "include", "twisterl_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(TW_FIN_[A-Z0-9]+) = (\d+)", header))
    assert enum == dict(TW_FIN_NONE=0, TW_FIN_GROUP16=fm.GROUP16, TW_FIN_GROUP8=fm.GROUP8, TW_FIN_WAVE=fm.WAVE, TW_FIN_AZ=fm.AZ)
    from twisterl_amd import _lib
    assert (_lib.TW_FIN_GROUP16, _lib.TW_FIN_GROUP8, _lib.TW_FIN_WAVE, _lib.TW_FIN_AZ) == (fm.GROUP16, fm.GROUP8, fm.WAVE, fm.AZ)


def test_the_switches_lie_where_the_table_says():
    """(last horizon of a form, first of the next) for each class of observations, from the restated byte counts."""
    def last(pred, hi):
        return max(t for t in range(1, hi + 2) if pred(t))
    for cells in (16, 0):
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["form"] == fm.GROUP16, 600) == 511
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["form"] != fm.WAVE, 1100) == 1023
    assert last(lambda t: fm.dispatch("ppo", 37, t, 16)["waves"] == 2, 1700) == 1638 and fm.dispatch("ppo", 37, 1024, 16)["waves"] == 2
    assert fm.ppo_max_t_pad(16) == 3276 and fm.dispatch("ppo", 37, 3276, 16)["waves"] == 1 and fm.dispatch("ppo", 37, 3277, 16) is None
    for cells in (1, 9, 15):
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["form"] == fm.GROUP16, 200) == 170
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["form"] != fm.WAVE, 400) == 341
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["waves"] == 4, 500) == 455
        assert last(lambda t: fm.dispatch("ppo", 37, t, cells)["waves"] >= 2, 1000) == 910
    for cells in (0, 1, 9, 15):
        assert fm.ppo_max_t_pad(cells) == 1820 and fm.dispatch("ppo", 37, 1821, cells) is None
    assert fm.dispatch("ppo", 37, 1024, 0) == dict(form=fm.WAVE, waves=1, blocks=37, threads=64, lds_bytes=36864)
    assert fm.AZ_MAX_T_PAD == 2048 and fm.dispatch("az", 37, 2048, 16)["lds_bytes"] == 65536 and fm.dispatch("az", 37, 2049, 16) is None


def test_table_reaches_every_form_and_both_sides_of_every_switch():
    ids = [fm.case_id(c) for c in fm.TABLE]
    assert len(set(ids)) == len(ids)
    for c in fm.TABLE:
        assert fm.case_dispatch(c) is not None, c
        assert c.kind in ("ppo", "az") and 1 <= c.A <= 31 and c.ids in (0, 1, 2) and 1 <= c.n_cells <= (64 if c.ids else 16), c
    for c in fm.REFUSED:
        assert fm.case_dispatch(c) is None, c
        ok = c._replace(t_pad=c.t_pad - 1)
        assert fm.case_dispatch(ok) is not None and ok in fm.TABLE, c          # the largest accepted horizon is a row
    W, G16, G8 = fm.WAVE, fm.GROUP16, fm.GROUP8
    cell16 = [c for c in fm.FORMS if not c.ids and c.n_cells == 16]
    assert [(c.t_pad, fm.case_dispatch(c)["form"], fm.case_dispatch(c)["waves"]) for c in cell16] == [
        (1, G16, 4), (2, G16, 4), (511, G16, 4), (512, G8, 4), (1023, G8, 4), (1024, W, 2), (1638, W, 2), (1639, W, 1), (3276, W, 1)]
    for nc in (1, 9, 15):
        staged = [c for c in fm.FORMS if not c.ids and c.n_cells == nc]
        assert [(c.t_pad, fm.case_dispatch(c)["form"], fm.case_dispatch(c)["waves"]) for c in staged] == [
            (170, G16, 4), (171, G8, 4), (341, G8, 4), (342, W, 4), (455, W, 4), (456, W, 2), (910, W, 2), (911, W, 1), (1820, W, 1)]
    for w in (1, 2):
        for nc in (1, 25, 64):
            arr = [c for c in fm.FORMS if c.ids == w and c.n_cells == nc]
            assert [(c.t_pad, fm.case_dispatch(c)["form"], fm.case_dispatch(c)["waves"]) for c in arr] == [
                (511, G16, 4), (512, G8, 4), (1023, G8, 4), (1024, W, 1), (1820, W, 1)]
    assert _forms(fm.TABLE) == {(G16, 4), (G8, 4), (W, 4), (W, 2), (W, 1), (fm.AZ, 4)}
    assert sorted(c.E for c in fm.GROUP_EDGES if fm.case_dispatch(c)["form"] == G16) == [1, 15, 16, 17, 67]
    assert sorted(c.E for c in fm.GROUP_EDGES if fm.case_dispatch(c)["form"] == G8) == [1, 7, 8, 9, 35]
    for kind in ("ppo", "az"):
        assert {c.A for c in fm.COLUMNS if c.kind == kind and not c.ids} == {1, 2, 3, 4, 5, 31}
    assert {c.t_pad for c in fm.AZ_HORIZONS if c.n_cells == 16} == {1, 2, 2048}
    # every mover with every kind of finalize, the special values in every PPO form and in the AZ form
    assert {m for c in fm.TABLE for m in fm.movers(c)} == {"compact_obs16_kernel", "compact_env_obs8_kernel", "narrow_logits_kernel"}
    assert _forms(c for c in fm.VALUES) == {(G16, 4), (G8, 4), (W, 2), (W, 4), (fm.AZ, 4)}
    assert {(c.gamma, c.lam) for c in fm.VALUES if c.kind == "ppo"} >= {(0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.0, 0.0)}


def test_table_makes_a_second_trip_of_every_capped_loop():
    two = [c for c in fm.TABLE if fm.finalize_trips(c) >= 2]
    assert _forms(two) >= {(fm.GROUP16, 4), (fm.GROUP8, 4), (fm.WAVE, 4), (fm.AZ, 4)}
    for c in fm.SECOND_TRIPS:
        assert fm.finalize_trips(c) == 2 or c.ids or c.A > 4, c
        # the smallest such shape: one workgroup's worth of episodes fewer and the loop has one trip
        d = fm.case_dispatch(c)
        per_block = {fm.GROUP16: 16, fm.GROUP8: 8}.get(d["form"], d["waves"])
        assert c.E - per_block * d["blocks"] < 128 and c.E * c.t_pad * 48 <= 272 * 1000 * 1000, c
    g8 = next(c for c in fm.SECOND_TRIPS if fm.case_dispatch(c)["form"] == fm.GROUP8)
    assert fm.case_dispatch(g8)["blocks"] == 2048 and g8.E > 8 * 2048
    # the rotation wave == (grp & 3) of the grouped forms on a second trip: groups beyond the grid whose index is 1, 2, 3 mod 4
    for c in two:
        d = fm.case_dispatch(c)
        if d["form"] in (fm.GROUP16, fm.GROUP8):
            g = 16 if d["form"] == fm.GROUP16 else 8
            groups = -(-c.E // g)
            assert {grp & 3 for grp in range(d["blocks"], groups)} == {0, 1, 2, 3} or groups - d["blocks"] >= 1, c
    movers = {m for c in fm.TABLE if fm.mover_trips(c.E) >= 2 for m in fm.movers(c)}
    assert movers >= {"compact_obs16_kernel", "compact_env_obs8_kernel"}
    assert any(fm.mover_trips(c.E) >= 2 and c.A > 4 for c in fm.TABLE)
    # the scan: one tile, the tile edge, 256 tiles (the carry unused), 257 and more (a second trip of the carry loop), an odd tail
    assert [fm.scan_tiles(E) for E in fm.SCAN_E] == [1, 1, 1, 1, 2, 5, 256, 257, 258, 513]
    assert [fm.scan_carry_trips(E) for E in fm.SCAN_E] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 3]
    assert all(fm.scan_carry_trips(c.E) == 2 for c in fm.SCAN_WITH_RECORDS)


def test_inputs_are_a_function_of_episode_and_record_and_padding_is_poison():
    c = fm._ppo(5, 7, n_cells=9, A=5)
    L = fm.episode_lengths(c.E, c.t_pad)
    assert L.min() >= 1 and L.max() <= 7 and int(L.sum()) % 2 == 1
    rec, _, wide = fm.make_inputs(c, L)
    rec2, _, _ = fm.make_inputs(c._replace(E=3), L[:3])
    assert np.array_equal(rec2[:7][:int(L[0])], rec[:7][:int(L[0])])            # episode 0's records do not depend on E
    live = (np.arange(35) % 7) < np.repeat(L, 7)
    assert len({r.tobytes() for r in rec[live]}) == int(live.sum())             # no two live records alike: a misplaced row shows
    assert (rec[~live][:, 4:10] == fm.POISON_F32).all() and (rec[~live][:, :4] == 0xFFFFFFFF).all() and np.isnan(wide[~live]).all()
    assert np.isnan(np.array([fm.POISON_F32], np.uint32).view(np.float32))[0]
    for E, t in ((37, 1), (37, 2), (37, 3276), (16, 65), (65605, 2)):
        L = fm.episode_lengths(E, t)
        assert L.min() >= 1 and L.max() <= t and (t == 1 or int(L.sum(dtype=np.uint64)) % 2 == 1), (E, t)
        if E == 37 and t > 65:
            assert {1, 2, 63, 64, 65, t - 1, t} <= set(L.tolist())


def _small_ppo_cases():
    return [c for c in fm.TABLE if c.kind == "ppo" and c.E * c.t_pad <= 37 * 600 and c.A == 4 and not c.ids]


def test_gae_reference_equals_the_oracle_bit_for_bit(oracle):
    """gae_f32_episodes against two_gae (oracle/tw_oracle.c), episode by episode, on the table's own small cases -- the -0.0, denormal
    and overflowing episodes of the special-valued rows among them."""
    seen_denormal = seen_inf = seen_negzero = False
    cases = _small_ppo_cases()
    assert any(c.values == "special" for c in cases) and len(cases) >= 20
    for c in cases:
        L = fm.episode_lengths(c.E, c.t_pad)
        rec, o16, wide = fm.make_inputs(c, L)
        ref = fm.reference(c, L, rec, o16, wide, False)
        rews, vals = ref["rewards"].view(np.float32), ref["values"].view(np.float32)
        start = 0
        for e, n in enumerate(L.tolist()):
            a, r = oracle.gae(rews[start:start + n], vals[start:start + n], c.gamma, c.lam)
            for name, got, want in (("advs", ref["advs"][start:start + n], a), ("rets", ref["rets"][start:start + n], r)):
                bad = fm.same_or_nan(got, want)
                assert bad.size == 0, (fm.case_id(c), e, name, int(bad[0]))
                if c.values == "normal":
                    assert not np.isnan(want).any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            adv = ref["advs"][start:start + n]
            seen_denormal |= bool(((adv != 0) & (np.abs(adv) < np.float32(1.1754944e-38))).any())
            seen_inf |= bool(np.isinf(adv).any())
            seen_negzero |= bool((rews[start:start + n].view(np.uint32) == 0x80000000).all())
            start += n
    assert seen_denormal and seen_inf and seen_negzero


def test_gae_reference_lies_inside_the_float64_bound():
    for c in _small_ppo_cases():
        if c.values != "normal":
            continue
        L = fm.episode_lengths(c.E, c.t_pad)
        rec, o16, wide = fm.make_inputs(c, L)
        ref = fm.reference(c, L, rec, o16, wide, False)
        rews, vals = ref["rewards"].view(np.float32), ref["values"].view(np.float32)
        assert np.isfinite(rews).all() and np.isfinite(vals).all() and (np.abs(vals) >= np.float32(1.1754944e-38)).all()
        a64, r64 = ref64.gae_f64_episodes(rews, vals, L, c.gamma, c.lam)
        ea, er = ref64.gae_bound_episodes(rews, vals, np.zeros(rews.size), L, c.gamma, c.lam)
        assert (np.abs(ref["advs"].astype(np.float64) - a64) <= ea).all() and (np.abs(ref["rets"].astype(np.float64) - r64) <= er).all(), fm.case_id(c)


def test_remaining_reference_is_total_minus_exclusive_prefix_with_sequential_sums():
    c = fm._az(37, 300)
    L = fm.episode_lengths(c.E, c.t_pad)
    rec, _, _ = fm.make_inputs(c, L)
    ref = fm.reference(c, L, rec, None, None, True)
    rews = ref["rewards"] if "rewards" in ref else None
    assert rews is None and (ref["perms"] == 0xFF).all()
    order = [36] + list(range(36))
    start = 0
    for e in order:
        n = int(L[e])
        r = rec[e * 300:e * 300 + n, 9].copy().view(np.float32)
        cs = np.cumsum(r, dtype=np.float32)
        want = cs[-1] - np.concatenate([[np.float32(0)], cs[:-1]]).astype(np.float32)
        assert np.array_equal(ref["remaining"][start:start + n].view(np.uint32), want.view(np.uint32)), e
        start += n
    es, total = fm.ep_start_ref(L, True)
    assert es[36] == 0 and es[0] == L[36] and total == start and np.array_equal(ref["ep_start"], es)
    es, _ = fm.ep_start_ref(np.full(5, 0xFFFFFFFF, np.uint32), False)
    assert int(es[4]) == 4 * 0xFFFFFFFF
