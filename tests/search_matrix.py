"""Every self-play, evaluate / solve and big-board kernel the library builds, one table row each, and the launch rule that picks
it (GPU-free).  The companion of tests/kernel_matrix.py (the PPO rollout family) for the other templated families:

* `mcts_f32_kernel<NT, NC, NW, PERSIST>` (tw_mcts.hip): lane-per-episode self-play; MCTS-guided evaluate / solve through `solve.on`;
* `solve_f32_kernel<NT, NC, NW>` (tw_solve.hip): evaluate / solve without search;
* `mcts_deep_kernel<NT, NC, NW, NWK, SOLVE, DEC, SPL>` and `mcts_engine_kernel<NT, NC>` (tw_mcts_deep.hip): the walker kernel in its
  plain (NW = -16), wide (-4), decoupled, split and solve-mode (-17) shapes, and the engine side of the split shape;
* `mcts_big_kernel<NC>`, `solve_big_kernel<NC>`, `rollout_big_kernel<NC>` (tw_mcts_big.hip, tw_rollout_big.hip): boards of 17 .. 64 cells.

`dispatch(row, cus)` restates, in Python, how the library gets from a call to one of them and to its launch shape:

* tw_az_collect: the big-board branch; mcts_deep_applies (hidden 128 / 256, episodes <= CUs x {8, 32, 96, 192, 256} by num_searches,
  TW_OPT_FORCE_GEOM, TW_OPT_AZ_VARIANT & 7); deep_shape (walkers 1 / 2 / 4 / 8 from avail = CUs - reserve_cus and num_searches, wide,
  decoupled, split, every TW_OPT_AZ_VARIANT bit) -> mcts_deep_walkers -> launch_deep_nt / geom / nwk / split; else
  f32_resident_episodes(selfplay) -> launch_mcts_one / geom, the generic-policy branch (<0, NC, -65>, never persistent);
* tw_evaluate / tw_solve: attempts = episodes x num_searches; without MCTS geometry_for<NT>(attempts) -> launch_solve_geom; with it
  mcts_deep_applies on the attempts (no reserved CUs) -> deep_shape(solve) (16 columns, 1 / 2 / 4 walkers), else mcts_f32_kernel;
* tw_ppo_collect of a big board: launch_rollout_big.

tests/test_search_matrix.py holds the table against the kernels in the built assembly (and takes a census of the whole build);
tests/test_gpu_search_matrix.py runs every row on the GPU: the launch identity the library reports (tw_debug_last_launch) first, then
the oracle.

Row fields: those of kernel_matrix.Row (`E`: episodes; `reserve`: None, "all_but_one" or "all_but_16" -- reserve_cus = CUs - 1 / CUs - 16,
so that avail is 1 / 16 on every chip), plus `S` (num_mcts_searches), `med` (max_expand_depth), `variant` (TW_OPT_AZ_VARIANT), `entry`
("az", "evaluate", "solve", "ppo"), `det` / `ns` (deterministic / num_searches of evaluate and solve) and `covers`: "main" (the row is
THE row of the kernel it launches), "engine" (a split-shape launch that stands for its mcts_engine_kernel) or "extra" (a further
case of a kernel that has its row: the sampled MCTS-guided evaluates of every lane-per-episode shape class and the greedy ones of
the solve-mode walker kernels).

A row uses a diagnostic option (TW_OPT_FORCE_GEOM, TW_OPT_AZ_VARIANT) only where no plain call of at most MAX_EPISODES episodes /
MAX_ATTEMPTS attempts reaches the kernel; the section comments say which and why.
"""
from collections import namedtuple

from tests import kernel_matrix as km

Row = namedtuple("Row", "w h emb hidden E prec twists force_geom no_persist reserve common diff S med variant entry det ns covers")

AB1, AB16 = "all_but_one", "all_but_16"
MAX_EPISODES = 32_768          # self-play rows (the oracle collects every one of them in full, under 2 s on 16 threads)
MAX_ATTEMPTS = 40_960          # evaluate rows: episodes x num_searches
BIG_NC = 25                    # tw_big_board.hpp: cells of a 5-bit board; 36 and 64: byte boards


def AZ(w, h, emb, hidden, E, S, med=1, diff=4, twists=False, force_geom=0, reserve=None, variant=0, common=None, covers="main"):
    return Row(w, h, emb, hidden, E, "fp32", twists, force_geom, False, reserve, common, diff, S, med, variant, "az", False, 0, covers)


def EV(w, h, emb, hidden, E, ns, det=False, S=0, med=1, diff=4, twists=False, variant=0, common=None, covers="main", entry="evaluate"):
    return Row(w, h, emb, hidden, E, "fp32", twists, 0, False, None, common, diff, S, med, variant, entry, det, ns, covers)


def SV(w, h, emb, hidden, ns, det=False, S=0, med=1, diff=4, twists=False, common=None, covers="main"):
    return EV(w, h, emb, hidden, 1, ns, det, S, med, diff, twists, 0, common, covers, entry="solve")


def PPO(w, h, emb, common, E, diff=4, twists=False):
    return Row(w, h, emb, 0, E, "fp32", twists, 0, False, None, common, diff, 0, 1, 0, "ppo", False, 0, "main")


# @TABLE@
TABLE = [
    # ---- mcts_f32_kernel<NT, NC, NW, PERSIST> (tw_mcts.hip), self-play.  32 / 64 hidden units take it always, 128 / 256 beyond the walker kernel's
    # range (fewer than 16 searches and more than 8 episodes per CU here).  <.., 8, false> would need 39,681 episodes (waves_per_group): TW_OPT_FORCE_GEOM 8.
    AZ(2, 2, 32, 32, 77, 27, diff=4),                                                                   # mcts_f32_kernel<1, 4, 1, false>
    AZ(2, 2, 32, 32, 12801, 4, diff=3),                                                                 # mcts_f32_kernel<1, 4, 2, false>
    AZ(2, 2, 64, 32, 300, 0, diff=3, force_geom=8),                                                     # mcts_f32_kernel<1, 4, 8, false>
    AZ(2, 2, 32, 32, 900, 18, diff=5, reserve=AB1),                                                     # mcts_f32_kernel<1, 4, 8, true>
    AZ(2, 2, 32, 64, 100, 5, diff=0),                                                                   # mcts_f32_kernel<2, 4, -2, false>
    AZ(2, 2, 32, 64, 300, 24, med=2, diff=5, twists=True, force_geom=8),                                # mcts_f32_kernel<2, 4, 8, false>
    AZ(2, 2, 64, 64, 800, 12, diff=4, reserve=AB1),                                                     # mcts_f32_kernel<2, 4, 8, true>
    AZ(2, 2, 32, 128, 2500, 6, diff=3),                                                                 # mcts_f32_kernel<4, 4, -16, false>
    AZ(2, 2, 64, 128, 5000, 4, diff=3),                                                                 # mcts_f32_kernel<4, 4, -4, false>
    AZ(2, 2, 32, 128, 30000, 2, diff=3, twists=True),                                                   # mcts_f32_kernel<4, 4, -4, true>
    AZ(2, 2, 32, 128, 300, 30, diff=5, force_geom=8),                                                   # mcts_f32_kernel<4, 4, 8, false>
    AZ(2, 2, 32, 128, 2500, 12, diff=4, reserve=AB1),                                                   # mcts_f32_kernel<4, 4, 8, true>
    AZ(2, 2, 32, 256, 2533, 6, diff=3, twists=True),                                                    # mcts_f32_kernel<8, 4, -16, false>
    AZ(2, 2, 64, 256, 5001, 4, diff=4),                                                                 # mcts_f32_kernel<8, 4, -4, false>
    AZ(2, 2, 32, 256, 30000, 2, diff=3),                                                                # mcts_f32_kernel<8, 4, -4, true>
    AZ(2, 2, 32, 256, 300, 30, diff=5, force_geom=8),                                                   # mcts_f32_kernel<8, 4, 8, false>
    AZ(2, 2, 32, 256, 2500, 12, diff=5, reserve=AB1),                                                   # mcts_f32_kernel<8, 4, 8, true>
    AZ(2, 2, 32, 0, 100, 24, diff=5, common=(48,)),                                                     # mcts_f32_kernel<0, 4, -65, false>
    AZ(3, 3, 64, 32, 333, 120, diff=9),                                                                 # mcts_f32_kernel<1, 9, 1, false>
    AZ(3, 3, 32, 32, 12801, 8, diff=5, twists=True),                                                    # mcts_f32_kernel<1, 9, 2, false>
    AZ(3, 3, 32, 32, 700, 90, diff=7, twists=True, force_geom=8),                                       # mcts_f32_kernel<1, 9, 8, false>
    AZ(3, 2, 32, 32, 1000, 48, med=2, diff=6, reserve=AB1),                                             # mcts_f32_kernel<1, 9, 8, true>
    AZ(3, 3, 32, 64, 45, 400, diff=10),                                                                 # mcts_f32_kernel<2, 9, -2, false>
    AZ(3, 2, 64, 64, 513, 0, diff=4, force_geom=8),                                                     # mcts_f32_kernel<2, 9, 8, false>
    AZ(3, 3, 32, 64, 1111, 21, diff=6, twists=True, reserve=AB1),                                       # mcts_f32_kernel<2, 9, 8, true>
    AZ(3, 2, 64, 128, 3000, 12, diff=4),                                                                # mcts_f32_kernel<4, 9, -16, false>
    AZ(3, 3, 32, 128, 6001, 5, med=2, diff=4),                                                          # mcts_f32_kernel<4, 9, -4, false>
    AZ(3, 2, 32, 128, 30011, 3, diff=4),                                                                # mcts_f32_kernel<4, 9, -4, true>
    AZ(3, 3, 64, 128, 290, 150, diff=9, twists=True, force_geom=8),                                     # mcts_f32_kernel<4, 9, 8, false>
    AZ(3, 3, 32, 128, 2600, 15, diff=5, twists=True, reserve=AB1),                                      # mcts_f32_kernel<4, 9, 8, true>
    AZ(3, 3, 64, 256, 3001, 12, med=2, diff=4),                                                         # mcts_f32_kernel<8, 9, -16, false>
    AZ(3, 3, 32, 256, 6001, 5, diff=4, twists=True),                                                    # mcts_f32_kernel<8, 9, -4, false>
    AZ(3, 3, 32, 256, 30011, 3, diff=3),                                                                # mcts_f32_kernel<8, 9, -4, true>
    AZ(3, 3, 64, 256, 290, 60, diff=6, twists=True, force_geom=8),                                      # mcts_f32_kernel<8, 9, 8, false>
    AZ(3, 3, 32, 256, 2600, 15, med=2, diff=5, twists=True, reserve=AB1),                               # mcts_f32_kernel<8, 9, 8, true>
    AZ(3, 3, 64, 0, 75, 60, med=2, diff=7, twists=True, common=(48, 40)),                               # mcts_f32_kernel<0, 9, -65, false>
    AZ(4, 4, 32, 32, 150, 36, med=2, diff=7, twists=True),                                              # mcts_f32_kernel<1, 16, 1, false>
    AZ(4, 3, 32, 32, 12321, 3, med=2, diff=4),                                                          # mcts_f32_kernel<1, 16, 2, false>
    AZ(4, 4, 32, 32, 257, 10, diff=1, force_geom=8),                                                    # mcts_f32_kernel<1, 16, 8, false>
    AZ(4, 4, 64, 32, 777, 24, diff=5, twists=True, reserve=AB1),                                        # mcts_f32_kernel<1, 16, 8, true>
    AZ(4, 4, 64, 64, 130, 60, med=2, diff=7, twists=True),                                              # mcts_f32_kernel<2, 16, -2, false>
    AZ(4, 4, 32, 64, 290, 42, diff=8, force_geom=8),                                                    # mcts_f32_kernel<2, 16, 8, false>
    AZ(4, 3, 32, 64, 900, 5, med=2, diff=1, reserve=AB1),                                               # mcts_f32_kernel<2, 16, 8, true>
    AZ(4, 4, 128, 128, 2600, 8, diff=5, twists=True),                                                   # mcts_f32_kernel<4, 16, -16, false>
    AZ(4, 4, 32, 128, 5555, 3, diff=5),                                                                 # mcts_f32_kernel<4, 16, -4, false>
    AZ(4, 4, 64, 128, 29500, 2, diff=3),                                                                # mcts_f32_kernel<4, 16, -4, true>
    AZ(4, 4, 32, 128, 520, 18, med=2, diff=5, force_geom=8),                                            # mcts_f32_kernel<4, 16, 8, false>
    AZ(4, 4, 64, 128, 2470, 9, diff=5, reserve=AB1),                                                    # mcts_f32_kernel<4, 16, 8, true>
    AZ(4, 4, 64, 256, 2601, 8, diff=1),                                                                 # mcts_f32_kernel<8, 16, -16, false>
    AZ(4, 3, 32, 256, 5555, 0, diff=4),                                                                 # mcts_f32_kernel<8, 16, -4, false>
    AZ(4, 4, 64, 256, 29500, 2, med=2, diff=3),                                                         # mcts_f32_kernel<8, 16, -4, true>
    AZ(4, 3, 32, 256, 520, 18, med=2, diff=5, force_geom=8),                                            # mcts_f32_kernel<8, 16, 8, false>
    AZ(4, 4, 64, 256, 2470, 9, diff=5, reserve=AB1),                                                    # mcts_f32_kernel<8, 16, 8, true>
    AZ(4, 3, 32, 0, 130, 36, diff=6, common=(96, 24)),                                                  # mcts_f32_kernel<0, 16, -65, false>
    # ---- solve_f32_kernel<NT, NC, NW> (tw_solve.hip): evaluate / solve without search, geometry_for<NT>(episodes x num_searches)
    EV(2, 2, 32, 32, 100, 3, diff=3),                                                                   # solve_f32_kernel<1, 4, 1>
    EV(2, 2, 32, 32, 2500, 5, diff=2),                                                                  # solve_f32_kernel<1, 4, 2>
    EV(2, 2, 32, 32, 5000, 8, diff=2),                                                                  # solve_f32_kernel<1, 4, 8>
    EV(2, 2, 64, 64, 200, 1, det=True, diff=1),                                                         # solve_f32_kernel<2, 4, -2>
    EV(2, 2, 32, 64, 10000, 4, diff=2),                                                                 # solve_f32_kernel<2, 4, 8>
    EV(2, 2, 32, 128, 300, 2, diff=3),                                                                  # solve_f32_kernel<4, 4, -16>
    EV(2, 2, 64, 128, 1000, 6, diff=3),                                                                 # solve_f32_kernel<4, 4, -4>
    EV(2, 2, 32, 128, 10000, 4, diff=2),                                                                # solve_f32_kernel<4, 4, 8>
    EV(2, 2, 32, 256, 300, 2, diff=3, twists=True),                                                     # solve_f32_kernel<8, 4, -16>
    EV(2, 2, 64, 256, 1000, 5, diff=3),                                                                 # solve_f32_kernel<8, 4, -4>
    EV(2, 2, 32, 256, 10000, 4, diff=2),                                                                # solve_f32_kernel<8, 4, 8>
    EV(2, 2, 32, 0, 150, 2, diff=3, common=(48,)),                                                      # solve_f32_kernel<0, 4, -65>
    SV(3, 3, 64, 32, 8, diff=6, twists=True),                                                           # solve_f32_kernel<1, 9, 1>
    EV(3, 3, 32, 32, 12500, 1, det=True, diff=4),                                                       # solve_f32_kernel<1, 9, 2>
    EV(3, 2, 32, 32, 8000, 5, diff=3),                                                                  # solve_f32_kernel<1, 9, 8>
    EV(3, 3, 32, 64, 150, 4, diff=5, twists=True),                                                      # solve_f32_kernel<2, 9, -2>
    EV(3, 3, 64, 64, 39800, 1, det=True, diff=3),                                                       # solve_f32_kernel<2, 9, 8>
    SV(3, 3, 64, 128, 6, diff=5),                                                                       # solve_f32_kernel<4, 9, -16>
    EV(3, 3, 32, 128, 6000, 2, det=False, diff=4, twists=True),                                         # solve_f32_kernel<4, 9, -4>
    EV(3, 2, 32, 128, 39700, 1, det=True, diff=3),                                                      # solve_f32_kernel<4, 9, 8>
    EV(3, 3, 64, 256, 4000, 1, det=True, diff=0),                                                       # solve_f32_kernel<8, 9, -16>
    EV(3, 3, 32, 256, 6001, 1, det=True, diff=4, twists=True),                                          # solve_f32_kernel<8, 9, -4>
    EV(3, 3, 32, 256, 39700, 1, det=True, diff=3),                                                      # solve_f32_kernel<8, 9, 8>
    SV(3, 3, 64, 0, 7, diff=5, twists=True, common=(48, 40)),                                           # solve_f32_kernel<0, 9, -65>
    EV(4, 3, 32, 32, 333, 1, det=True, diff=5),                                                         # solve_f32_kernel<1, 16, 1>
    EV(4, 4, 64, 32, 4100, 3, diff=3, twists=True),                                                     # solve_f32_kernel<1, 16, 2>
    EV(4, 4, 32, 32, 39700, 1, det=True, diff=3),                                                       # solve_f32_kernel<1, 16, 8>
    SV(4, 4, 32, 64, 5, diff=6),                                                                        # solve_f32_kernel<2, 16, -2>
    EV(4, 3, 32, 64, 8000, 5, diff=2),                                                                  # solve_f32_kernel<2, 16, 8>
    EV(4, 4, 64, 128, 1000, 4, diff=4, twists=True),                                                    # solve_f32_kernel<4, 16, -16>
    EV(4, 4, 32, 128, 2001, 3, diff=3),                                                                 # solve_f32_kernel<4, 16, -4>
    EV(4, 4, 64, 128, 8001, 5, diff=2),                                                                 # solve_f32_kernel<4, 16, 8>
    EV(4, 4, 64, 256, 1001, 4, diff=4),                                                                 # solve_f32_kernel<8, 16, -16>
    EV(4, 3, 32, 256, 2001, 3, diff=3),                                                                 # solve_f32_kernel<8, 16, -4>
    EV(4, 4, 64, 256, 8001, 5, diff=2, twists=True),                                                    # solve_f32_kernel<8, 16, 8>
    EV(4, 3, 32, 0, 333, 1, det=True, diff=4, common=(96, 24)),                                         # solve_f32_kernel<0, 16, -65>
    # ---- mcts_deep_kernel<NT, NC, NW, NWK, SOLVE, DEC, SPL> (tw_mcts_deep.hip): 128 / 256 hidden units.  Plain <.., -16, 1, ..> and the decoupled
    # <.., -16, 2 | 4 | 8, false, true, false> are the automatic shapes (eight decoupled walkers only below 16 available CUs: from 8 episodes per CU on
    # the split shape takes over); undecoupled two / four / eight walkers exist behind TW_OPT_AZ_VARIANT + 256 only, the 32-column engine (NW = -4)
    # behind + 32 or TW_OPT_FORCE_GEOM 32 only.  reserve AB1 / AB16: 1 / 16 available CUs, so that 2 / 4 / 10 / 11+ episodes pick 1 / 2 / 4 / 8 walkers and
    # 128 episodes the split shape (12 walkers below 400 searches, 16 from there on; 8 engine workgroups).
    AZ(2, 2, 32, 128, 300, 120, diff=7),                                                                # mcts_deep_kernel<4, 4, -16, 1, false, false, false>
    AZ(2, 2, 32, 128, 700, 24, diff=6, variant=256),                                                    # mcts_deep_kernel<4, 4, -16, 2, false, false, false>
    AZ(2, 2, 32, 128, 1500, 15, diff=5, twists=True, variant=256),                                      # mcts_deep_kernel<4, 4, -16, 4, false, false, false>
    AZ(2, 2, 64, 128, 3300, 72, med=2, diff=5, variant=256),                                            # mcts_deep_kernel<4, 4, -16, 8, false, false, false>
    AZ(2, 2, 32, 128, 701, 24, diff=6, twists=True),                                                    # mcts_deep_kernel<4, 4, -16, 2, false, true, false>
    AZ(2, 2, 64, 128, 1500, 15, diff=5),                                                                # mcts_deep_kernel<4, 4, -16, 4, false, true, false>
    AZ(2, 2, 32, 128, 40, 60, diff=7, reserve=AB1),                                                     # mcts_deep_kernel<4, 4, -16, 8, false, true, false>
    AZ(2, 2, 32, 128, 2500, 48, diff=5),                                                                # mcts_deep_kernel<4, 4, -16, 12, false, true, true>
    AZ(2, 2, 64, 128, 128, 400, diff=6, reserve=AB16, twists=True),                                     # mcts_deep_kernel<4, 4, -16, 16, false, true, true>
    AZ(2, 2, 32, 128, 300, 60, diff=6, force_geom=32),                                                  # mcts_deep_kernel<4, 4, -4, 1, false, false, false>
    AZ(2, 2, 64, 128, 700, 24, med=2, diff=6, force_geom=32),                                           # mcts_deep_kernel<4, 4, -4, 2, false, false, false>
    AZ(2, 2, 32, 128, 1500, 18, diff=5, force_geom=32),                                                 # mcts_deep_kernel<4, 4, -4, 4, false, false, false>
    AZ(2, 2, 32, 128, 3300, 48, diff=5, force_geom=32),                                                 # mcts_deep_kernel<4, 4, -4, 8, false, false, false>
    EV(2, 2, 32, 128, 100, 3, S=8, diff=3),                                                             # mcts_deep_kernel<4, 4, -17, 1, true, false, false>
    EV(2, 2, 32, 128, 250, 4, S=4, diff=3, twists=True),                                                # mcts_deep_kernel<4, 4, -17, 2, true, false, false>
    EV(2, 2, 32, 128, 500, 3, S=5, med=2, diff=3),                                                      # mcts_deep_kernel<4, 4, -17, 4, true, false, false>
    AZ(3, 3, 64, 128, 2, 300, diff=10, reserve=AB1),                                                    # mcts_deep_kernel<4, 9, -16, 1, false, false, false>
    AZ(3, 3, 64, 128, 4, 150, med=2, diff=10, twists=True, reserve=AB1, variant=256),                   # mcts_deep_kernel<4, 9, -16, 2, false, false, false>
    AZ(3, 3, 32, 128, 9, 120, diff=9, reserve=AB1, variant=256),                                        # mcts_deep_kernel<4, 9, -16, 4, false, false, false>
    AZ(3, 3, 32, 128, 30, 101, diff=10, reserve=AB1, variant=256),                                      # mcts_deep_kernel<4, 9, -16, 8, false, false, false>
    AZ(3, 3, 32, 128, 72, 200, diff=10, reserve=AB16),                                                  # mcts_deep_kernel<4, 9, -16, 2, false, true, false>
    AZ(3, 3, 64, 128, 7, 130, diff=10, reserve=AB1),                                                    # mcts_deep_kernel<4, 9, -16, 4, false, true, false>
    AZ(3, 3, 64, 128, 41, 72, med=2, diff=6, twists=True, reserve=AB1),                                 # mcts_deep_kernel<4, 9, -16, 8, false, true, false>
    AZ(3, 3, 64, 128, 128, 100, diff=9, twists=True, reserve=AB16),                                     # mcts_deep_kernel<4, 9, -16, 12, false, true, true>
    AZ(3, 3, 64, 128, 129, 450, diff=8, reserve=AB16),                                                  # mcts_deep_kernel<4, 9, -16, 16, false, true, true>
    AZ(3, 3, 32, 128, 2, 160, diff=10, reserve=AB1, variant=32),                                        # mcts_deep_kernel<4, 9, -4, 1, false, false, false>
    AZ(3, 3, 64, 128, 4, 110, diff=9, reserve=AB1, variant=32),                                         # mcts_deep_kernel<4, 9, -4, 2, false, false, false>
    AZ(3, 3, 32, 128, 8, 140, diff=10, reserve=AB1, variant=32),                                        # mcts_deep_kernel<4, 9, -4, 4, false, false, false>
    AZ(3, 3, 32, 128, 35, 105, diff=9, twists=True, reserve=AB1, variant=32),                           # mcts_deep_kernel<4, 9, -4, 8, false, false, false>
    SV(3, 3, 64, 128, 6, S=20, diff=6, twists=True),                                                    # mcts_deep_kernel<4, 9, -17, 1, true, false, false>
    EV(3, 2, 32, 128, 251, 4, S=6, diff=4),                                                             # mcts_deep_kernel<4, 9, -17, 2, true, false, false>
    EV(3, 3, 32, 128, 501, 3, S=4, diff=3),                                                             # mcts_deep_kernel<4, 9, -17, 4, true, false, false>
    AZ(4, 4, 64, 128, 16, 0, diff=4),                                                                   # mcts_deep_kernel<4, 16, -16, 1, false, false, false>
    AZ(4, 4, 32, 128, 700, 24, diff=6, variant=256),                                                    # mcts_deep_kernel<4, 16, -16, 2, false, false, false>
    AZ(4, 3, 32, 128, 1500, 15, diff=5, variant=256),                                                   # mcts_deep_kernel<4, 16, -16, 4, false, false, false>
    AZ(4, 4, 64, 128, 3300, 72, med=2, diff=5, twists=True, variant=256),                               # mcts_deep_kernel<4, 16, -16, 8, false, false, false>
    AZ(4, 4, 32, 128, 701, 30, diff=6),                                                                 # mcts_deep_kernel<4, 16, -16, 2, false, true, false>
    AZ(4, 4, 64, 128, 1502, 15, med=2, diff=5, twists=True),                                            # mcts_deep_kernel<4, 16, -16, 4, false, true, false>
    AZ(4, 4, 32, 128, 42, 0, diff=3, reserve=AB1),                                                      # mcts_deep_kernel<4, 16, -16, 8, false, true, false>
    AZ(4, 4, 64, 128, 131, 120, med=2, diff=7, reserve=AB16),                                           # mcts_deep_kernel<4, 16, -16, 12, false, true, true>
    AZ(4, 4, 64, 128, 130, 400, diff=8, reserve=AB16, twists=True),                                     # mcts_deep_kernel<4, 16, -16, 16, false, true, true>
    AZ(4, 4, 32, 128, 300, 60, diff=6, variant=32),                                                     # mcts_deep_kernel<4, 16, -4, 1, false, false, false>
    AZ(4, 4, 64, 128, 700, 24, diff=6, variant=32),                                                     # mcts_deep_kernel<4, 16, -4, 2, false, false, false>
    AZ(4, 4, 32, 128, 1500, 18, diff=5, variant=32),                                                    # mcts_deep_kernel<4, 16, -4, 4, false, false, false>
    AZ(4, 4, 32, 128, 3300, 48, diff=5, variant=32),                                                    # mcts_deep_kernel<4, 16, -4, 8, false, false, false>
    EV(4, 4, 64, 128, 60, 2, S=120, diff=7),                                                            # mcts_deep_kernel<4, 16, -17, 1, true, false, false>
    EV(4, 4, 32, 128, 252, 4, S=16, diff=3),                                                            # mcts_deep_kernel<4, 16, -17, 2, true, false, false>
    EV(4, 4, 64, 128, 502, 3, S=3, diff=4, twists=True),                                                # mcts_deep_kernel<4, 16, -17, 4, true, false, false>
    AZ(2, 2, 32, 256, 333, 75, med=2, diff=7, twists=True),                                             # mcts_deep_kernel<8, 4, -16, 1, false, false, false>
    AZ(2, 2, 64, 256, 4, 150, med=2, diff=10, reserve=AB1, variant=256),                                # mcts_deep_kernel<8, 4, -16, 2, false, false, false>
    AZ(2, 2, 32, 256, 9, 120, diff=9, reserve=AB1, variant=256),                                        # mcts_deep_kernel<8, 4, -16, 4, false, false, false>
    AZ(2, 2, 32, 256, 30, 101, diff=10, reserve=AB1, variant=256),                                      # mcts_deep_kernel<8, 4, -16, 8, false, false, false>
    AZ(2, 2, 32, 256, 72, 200, diff=10, twists=True, reserve=AB16),                                     # mcts_deep_kernel<8, 4, -16, 2, false, true, false>
    AZ(2, 2, 64, 256, 7, 130, diff=10, reserve=AB1),                                                    # mcts_deep_kernel<8, 4, -16, 4, false, true, false>
    AZ(2, 2, 64, 256, 43, 110, diff=10, twists=True, reserve=AB1),                                      # mcts_deep_kernel<8, 4, -16, 8, false, true, false>
    AZ(2, 2, 32, 256, 140, 150, diff=9, reserve=AB16),                                                  # mcts_deep_kernel<8, 4, -16, 12, false, true, true>
    AZ(2, 2, 32, 256, 128, 450, diff=7, reserve=AB16),                                                  # mcts_deep_kernel<8, 4, -16, 16, false, true, true>
    AZ(2, 2, 32, 256, 2, 160, diff=10, force_geom=32, reserve=AB1),                                     # mcts_deep_kernel<8, 4, -4, 1, false, false, false>
    AZ(2, 2, 64, 256, 4, 110, diff=9, force_geom=32, reserve=AB1),                                      # mcts_deep_kernel<8, 4, -4, 2, false, false, false>
    AZ(2, 2, 32, 256, 8, 140, diff=10, twists=True, force_geom=32, reserve=AB1),                        # mcts_deep_kernel<8, 4, -4, 4, false, false, false>
    AZ(2, 2, 32, 256, 35, 105, diff=9, force_geom=32, reserve=AB1),                                     # mcts_deep_kernel<8, 4, -4, 8, false, false, false>
    EV(2, 2, 32, 256, 150, 2, S=5, med=2, diff=1),                                                      # mcts_deep_kernel<8, 4, -17, 1, true, false, false>
    EV(2, 2, 32, 256, 253, 4, S=3, diff=2),                                                             # mcts_deep_kernel<8, 4, -17, 2, true, false, false>
    EV(2, 2, 32, 256, 503, 3, S=17, diff=2, twists=True),                                               # mcts_deep_kernel<8, 4, -17, 4, true, false, false>
    AZ(3, 3, 32, 256, 10, 5, diff=0),                                                                   # mcts_deep_kernel<8, 9, -16, 1, false, false, false>
    AZ(3, 3, 32, 256, 700, 24, diff=6, twists=True, variant=256),                                       # mcts_deep_kernel<8, 9, -16, 2, false, false, false>
    AZ(3, 3, 32, 256, 1500, 15, diff=5, variant=256),                                                   # mcts_deep_kernel<8, 9, -16, 4, false, false, false>
    AZ(3, 3, 64, 256, 3300, 72, med=2, diff=5, variant=256),                                            # mcts_deep_kernel<8, 9, -16, 8, false, false, false>
    AZ(3, 3, 32, 256, 701, 36, diff=6),                                                                 # mcts_deep_kernel<8, 9, -16, 2, false, true, false>
    AZ(3, 2, 64, 256, 1504, 5, diff=1),                                                                 # mcts_deep_kernel<8, 9, -16, 4, false, true, false>
    AZ(3, 3, 32, 256, 44, 16, diff=1, reserve=AB1),                                                     # mcts_deep_kernel<8, 9, -16, 8, false, true, false>
    AZ(3, 2, 32, 256, 2501, 72, med=2, diff=5),                                                         # mcts_deep_kernel<8, 9, -16, 12, false, true, true>
    AZ(3, 3, 64, 256, 129, 400, diff=8, reserve=AB16),                                                  # mcts_deep_kernel<8, 9, -16, 16, false, true, true>
    AZ(3, 3, 32, 256, 300, 60, diff=6, variant=32),                                                     # mcts_deep_kernel<8, 9, -4, 1, false, false, false>
    AZ(3, 3, 64, 256, 700, 24, diff=6, variant=32),                                                     # mcts_deep_kernel<8, 9, -4, 2, false, false, false>
    AZ(3, 3, 32, 256, 1500, 18, diff=5, variant=32),                                                    # mcts_deep_kernel<8, 9, -4, 4, false, false, false>
    AZ(3, 3, 32, 256, 3300, 48, med=2, diff=5, variant=32),                                             # mcts_deep_kernel<8, 9, -4, 8, false, false, false>
    SV(3, 3, 32, 256, 4, S=40, med=2, diff=6),                                                          # mcts_deep_kernel<8, 9, -17, 1, true, false, false>
    EV(3, 3, 32, 256, 254, 4, S=8, diff=3, twists=True),                                                # mcts_deep_kernel<8, 9, -17, 2, true, false, false>
    EV(3, 3, 32, 256, 504, 3, S=6, diff=1),                                                             # mcts_deep_kernel<8, 9, -17, 4, true, false, false>
    AZ(4, 4, 64, 256, 2, 450, diff=10, twists=True, reserve=AB1),                                       # mcts_deep_kernel<8, 16, -16, 1, false, false, false>
    AZ(4, 4, 64, 256, 4, 150, med=2, diff=10, reserve=AB1, variant=256),                                # mcts_deep_kernel<8, 16, -16, 2, false, false, false>
    AZ(4, 4, 32, 256, 9, 120, diff=9, reserve=AB1, variant=256),                                        # mcts_deep_kernel<8, 16, -16, 4, false, false, false>
    AZ(4, 4, 32, 256, 30, 101, diff=10, twists=True, reserve=AB1, variant=256),                         # mcts_deep_kernel<8, 16, -16, 8, false, false, false>
    AZ(4, 4, 32, 256, 72, 200, diff=10, reserve=AB16),                                                  # mcts_deep_kernel<8, 16, -16, 2, false, true, false>
    AZ(4, 4, 64, 256, 7, 130, diff=10, reserve=AB1),                                                    # mcts_deep_kernel<8, 16, -16, 4, false, true, false>
    AZ(4, 4, 64, 256, 45, 90, diff=7, reserve=AB1),                                                     # mcts_deep_kernel<8, 16, -16, 8, false, true, false>
    AZ(4, 4, 64, 256, 300, 100, diff=9, twists=True, reserve=AB16),                                     # mcts_deep_kernel<8, 16, -16, 12, false, true, true>
    AZ(4, 4, 64, 256, 130, 450, diff=8, reserve=AB16),                                                  # mcts_deep_kernel<8, 16, -16, 16, false, true, true>
    AZ(4, 4, 32, 256, 2, 160, diff=10, twists=True, reserve=AB1, variant=32),                           # mcts_deep_kernel<8, 16, -4, 1, false, false, false>
    AZ(4, 4, 64, 256, 4, 110, diff=9, reserve=AB1, variant=32),                                         # mcts_deep_kernel<8, 16, -4, 2, false, false, false>
    AZ(4, 4, 32, 256, 8, 140, diff=10, reserve=AB1, variant=32),                                        # mcts_deep_kernel<8, 16, -4, 4, false, false, false>
    AZ(4, 4, 32, 256, 35, 105, diff=9, reserve=AB1, variant=32),                                        # mcts_deep_kernel<8, 16, -4, 8, false, false, false>
    EV(4, 4, 64, 256, 200, 2, S=12, diff=4, twists=True),                                               # mcts_deep_kernel<8, 16, -17, 1, true, false, false>
    EV(4, 4, 32, 256, 255, 4, S=5, med=2, diff=4),                                                      # mcts_deep_kernel<8, 16, -17, 2, true, false, false>
    EV(4, 4, 32, 256, 505, 3, S=4, diff=3),                                                             # mcts_deep_kernel<8, 16, -17, 4, true, false, false>
    # ---- mcts_engine_kernel<NT, NC>: the engine side of the split shape (rows of their own; the walker side has its row above)
    AZ(2, 2, 32, 128, 200, 30, diff=4, reserve=AB16, covers='engine'),                                  # mcts_engine_kernel<4, 4>
    AZ(3, 2, 64, 128, 2600, 48, diff=5, covers='engine'),                                               # mcts_engine_kernel<4, 9>
    AZ(4, 4, 128, 128, 129, 420, diff=7, twists=True, reserve=AB16, covers='engine'),                   # mcts_engine_kernel<4, 16>
    AZ(2, 2, 32, 256, 128, 400, diff=6, reserve=AB16, covers='engine'),                                 # mcts_engine_kernel<8, 4>
    AZ(3, 3, 64, 256, 300, 120, med=2, diff=6, twists=True, reserve=AB16, covers='engine'),             # mcts_engine_kernel<8, 9>
    AZ(4, 3, 32, 256, 150, 60, diff=7, reserve=AB16, covers='engine'),                                  # mcts_engine_kernel<8, 16>
    # ---- boards of 17 .. 64 cells (tw_mcts_big.hip, tw_rollout_big.hip): generic policies, 16 episodes / attempts per workgroup
    AZ(5, 5, 64, 0, 40, 8, diff=5, twists=True, common=(64, 32)),                                       # mcts_big_kernel<25>
    AZ(6, 6, 32, 0, 33, 5, med=2, diff=4, common=(48,)),                                                # mcts_big_kernel<36>
    AZ(8, 8, 32, 0, 20, 30, diff=4, twists=True, common=(64,)),                                         # mcts_big_kernel<64>
    EV(5, 5, 32, 0, 300, 2, diff=5, common=(64, 32)),                                                   # solve_big_kernel<25>
    EV(6, 5, 64, 0, 200, 1, det=True, diff=6, common=(48,)),                                            # solve_big_kernel<36>
    EV(7, 7, 32, 0, 100, 3, diff=4, twists=True, common=(32, 32)),                                      # solve_big_kernel<64>
    PPO(5, 5, 64, (128,), 150, diff=5),                                                                 # rollout_big_kernel<25>
    PPO(7, 5, 32, (48, 32), 100, diff=6),                                                               # rollout_big_kernel<36>
    PPO(8, 8, 32, (32,), 61, diff=3, twists=True),                                                      # rollout_big_kernel<64>
    # ---- further cases of kernels that have their row (covers = "extra"): a sampled MCTS-guided evaluate with several attempts per episode on every
    # lane-per-episode shape class (mcts_f32_kernel with solve.on), and greedy ones on the solve-mode walker kernels (whose own rows are sampled)
    EV(3, 3, 32, 32, 40, 3, S=6, diff=4, covers='extra'),                                               # mcts_f32_kernel<1, 9, 1, false>
    EV(3, 3, 32, 32, 2500, 5, S=2, diff=2, covers='extra'),                                             # mcts_f32_kernel<1, 9, 2, false>
    EV(2, 2, 32, 32, 5000, 8, S=2, diff=2, covers='extra'),                                             # mcts_f32_kernel<1, 4, 8, false>
    EV(4, 4, 32, 64, 40, 3, S=8, med=2, diff=4, twists=True, covers='extra'),                           # mcts_f32_kernel<2, 16, -2, false>
    EV(3, 3, 32, 128, 1000, 5, S=3, diff=3, covers='extra'),                                            # mcts_f32_kernel<4, 9, -4, false>
    EV(4, 3, 32, 256, 1000, 3, S=3, diff=3, covers='extra'),                                            # mcts_f32_kernel<8, 16, -16, false>
    EV(3, 3, 64, 0, 40, 3, S=5, diff=4, twists=True, common=(48, 40), covers='extra'),                  # mcts_f32_kernel<0, 9, -65, false>
    EV(3, 3, 64, 128, 300, 1, det=True, S=6, diff=4, twists=True, covers='extra'),                      # mcts_deep_kernel<4, 9, -17, 1, true, false, false>
    EV(4, 4, 32, 256, 1000, 1, det=True, S=4, diff=3, covers='extra'),                                  # mcts_deep_kernel<8, 16, -17, 2, true, false, false>
    EV(2, 2, 32, 128, 1500, 1, det=True, S=5, diff=2, covers='extra'),                                  # mcts_deep_kernel<4, 4, -17, 4, true, false, false>
]


def reserve_cus(row, cus):
    return cus - 1 if row.reserve == AB1 else cus - 16 if row.reserve == AB16 else 0


def attempts(row):
    return row.E * row.ns if row.entry in ("evaluate", "solve") else row.E


# ---------------------------------------------------------------------------------------------- tw_mcts_deep.hip
def mcts_deep_applies(n, hidden, S, cus, force_geom=0, variant=0):
    if hidden not in (128, 256) or n == 0:
        return False
    if force_geom in (8, 1) or (variant & 7) == 2:
        return False
    if (variant & 7) >= 3:
        return True
    return n <= cus * (256 if S >= 64 else 192 if S >= 48 else 96 if S >= 32 else 32 if S >= 16 else 8)


def split_walkers_per_group(S):
    return 16 if S >= 400 else 12


def split_groups_per_cu(walkers):
    return 2 if walkers <= 12 else 1


DeepShape = namedtuple("DeepShape", "walkers wide dec split engines")


def deep_shape(n, reserve, S, cus, solve=False, force_geom=0, variant=0):
    avail = cus - min(max(reserve, 0), cus - 1)
    long_search = S >= 400
    if n <= (3 if long_search else 2) * avail:
        walkers = 1
    elif (n < 8 * avail) if long_search else (2 * n <= 9 * avail):
        walkers = 2
    else:
        walkers = 4
    if S < 800 and n > 10 * avail:
        walkers = 8
    wide, v = False, variant
    if (v & 7) == 3:
        walkers = 2
    if (v & 7) == 4:
        walkers = 1
    if (v & 7) == 5:
        walkers = 4
    if (v & 7) == 6:
        walkers, wide = 8, True
    if v & 16:
        wide = False
    if v & 32:
        wide = True
    if not (v & 48) and force_geom == 32:
        wide = True
    if solve:
        wide = False
        if walkers == 8:
            walkers = 4
    dec = not solve and not wide and 2 <= walkers <= 8
    if v & 256:
        dec = False
    if (v & 128) and not solve and not wide and walkers >= 2:
        dec = True
    engines = avail // 2
    split = not solve and not wide and (v & 7) == 0 and avail >= 16 and n >= 8 * avail and not (v & 256)
    if v & 1024:
        split = False
    if (v & 512) and not solve and avail >= 16:
        split, wide = True, False
    if split:
        dec, walkers = True, split_walkers_per_group(S)
    return DeepShape(walkers, wide, dec, split, engines)


def mcts_deep_walkers(n, reserve, S, cus, solve=False, force_geom=0, variant=0):
    avail = cus - min(max(reserve, 0), cus - 1)
    sh = deep_shape(n, reserve, S, cus, solve, force_geom, variant)
    blocks = -(-n // sh.walkers)
    room = (avail - sh.engines) * split_groups_per_cu(sh.walkers) if sh.split else avail
    return min(blocks, room) * sh.walkers


def launch_mcts_deep(n, NT, nc, reserve, S, cus, solve, force_geom=0, variant=0):
    """launch_deep_nt / geom / nwk / split -> (kernel, (blocks, threads), engine (blocks, threads) or None)."""
    sh = deep_shape(n, reserve, S, cus, solve, force_geom, variant)
    nb = mcts_deep_walkers(n, reserve, S, cus, solve, force_geom, variant) // sh.walkers
    if sh.wide:
        nw = -4
    elif solve:
        nw = -17
    else:
        nw = -16
    if nw == -17:
        return ("deep", NT, nc, nw, sh.walkers, True, False, False), (nb, 256), None
    if nw == -16 and sh.split:
        nwk = 12 if sh.walkers == 12 else 16
        return ("deep", NT, nc, nw, nwk, False, True, True), (nb, 64 * nwk), (min(sh.engines, nb), 256)
    if nw == -16 and sh.dec:
        nwk = sh.walkers if sh.walkers in (2, 8) else 4
        return ("deep", NT, nc, nw, nwk, False, True, False), (nb, 64 * (4 + nwk)), None
    nwk = sh.walkers if sh.walkers in (1, 2, 8) else 4
    return ("deep", NT, nc, nw, nwk, False, False, False), (nb, 512 if nwk > 4 else 256), None


# ---------------------------------------------------------------------------------------------- tw_mcts.hip, tw_solve.hip
def f32_resident_selfplay(E, hidden, cus, reserve=0, force_geom=0):
    """f32_resident_episodes(.., selfplay = true, ..): CUs x 32 lanes between that many episodes and 3/4 of CUs x 256."""
    full = km.resident_full(cus, reserve)
    small = full // 8
    if hidden >= 128 and E > small and E * 4 <= full * 3 and not force_geom:
        return small
    return full


def lane_geometry(NT, n, cus, force_geom=0):
    """launch_mcts_one / launch_solve_one below the queue: geometry_for<NT>(n), then the shapes NT has."""
    nw = km.geometry_for(NT, n, cus, force_geom)
    if (NT >= 4 and nw not in (-16, -4)) or (NT == 2 and nw != -2) or (NT == 1 and nw not in (1, 2)):
        nw = 8
    return nw


def launch_mcts_f32(row, n, cus, solve):
    nc = km.n_chunks(row.w * row.h)
    if row.common is not None:                                           # generic stacks: EngineV, never persistent
        return ("mcts", 0, nc, -65, False), (-(-n // 16), 256), None
    NT, res = row.hidden // 32, reserve_cus(row, cus)
    resident = f32_resident_selfplay(n, row.hidden, cus, res, row.force_geom)
    if not solve and n > resident and not row.no_persist:                # tw_az_collect's `persist`, launch_mcts_one with the queue
        full = km.resident_full(cus, res)
        nw = -4 if NT >= 4 and resident < full else 8
        return ("mcts", NT, nc, nw, True), (full // 256, km.F32_BLOCK[nw][1]), None
    nw = lane_geometry(NT, n, cus, row.force_geom)
    ep, threads = km.F32_BLOCK[nw]
    return ("mcts", NT, nc, nw, False), (-(-n // ep), threads), None


def dispatch(row, cus):
    """-> (kernel, (blocks, threads), engine (blocks, threads) or None); kernel as in kernel_name()."""
    cells = row.w * row.h
    if cells > 16:                                                       # boards of 17 .. 64 cells: the generic engine, 16 episodes / attempts a workgroup
        nc = BIG_NC if cells <= BIG_NC else 36 if cells <= 36 else 64
        fam = {"ppo": "rollout_big", "az": "mcts_big"}.get(row.entry, "mcts_big" if row.S else "solve_big")
        return (fam, nc), (-(-attempts(row) // 16), 256), None
    nc = km.n_chunks(cells)
    NT = row.hidden // 32
    if row.entry == "az":
        res = reserve_cus(row, cus)
        if mcts_deep_applies(row.E, row.hidden, row.S, cus, row.force_geom, row.variant):
            return launch_mcts_deep(row.E, NT, nc, res, row.S, cus, False, row.force_geom, row.variant)
        return launch_mcts_f32(row, row.E, cus, False)
    n = attempts(row)
    if row.S == 0:                                                       # launch_solve_f32
        if row.common is not None:
            return ("solve", 0, nc, -65), (-(-n // 16), 256), None
        nw = lane_geometry(NT, n, cus, row.force_geom)
        ep, threads = km.F32_BLOCK[nw]
        return ("solve", NT, nc, nw), (-(-n // ep), threads), None
    if mcts_deep_applies(n, row.hidden, row.S, cus, row.force_geom, row.variant):      # (run_solve: no reserved CUs)
        return launch_mcts_deep(n, NT, nc, 0, row.S, cus, True, row.force_geom, row.variant)
    return launch_mcts_f32(row._replace(reserve=None), n, cus, True)


def covered_kernel(row, cus):
    """The kernel the row stands for in the coverage count (None: an extra row)."""
    k, _, _ = dispatch(row, cus)
    if row.covers == "engine":
        assert k[0] == "deep" and k[7], row
        return ("engine", k[1], k[2])
    return None if row.covers == "extra" else k


def kernel_name(k):
    b = lambda x: str(bool(x)).lower()
    if k[0] == "mcts":
        return f"mcts_f32_kernel<{k[1]}, {k[2]}, {k[3]}, {b(k[4])}>"
    if k[0] == "solve":
        return f"solve_f32_kernel<{k[1]}, {k[2]}, {k[3]}>"
    if k[0] == "deep":
        return f"mcts_deep_kernel<{k[1]}, {k[2]}, {k[3]}, {k[4]}, {b(k[5])}, {b(k[6])}, {b(k[7])}>"
    if k[0] == "engine":
        return f"mcts_engine_kernel<{k[1]}, {k[2]}>"
    return f"{k[0]}_kernel<{k[1]}>"


def row_id(row):
    net = f"c{'.'.join(map(str, row.common))}" if row.common else f"h{row.hidden}"
    call = f"-S{row.S}" + (f"-med{row.med}" if row.med != 1 else "")
    if row.entry in ("evaluate", "solve"):
        call += f"-{'det' if row.det else 'smp'}{row.ns}"
    return (f"{row.entry}-{row.w}x{row.h}-e{row.emb}-{net}-E{row.E}{call}-d{row.diff}" + ("-tw" if row.twists else "") +
            (f"-g{row.force_geom}" if row.force_geom else "") + (f"-v{row.variant}" if row.variant else "") +
            ({AB1: "-r1", AB16: "-r16"}.get(row.reserve, "")) + ("" if row.covers == "main" else f"-{row.covers}"))


# ---------------------------------------------------------------------------------------------- checks of a self-play result by itself
SUM_BOUND = 2.0 ** -24 * (1.0 + 2.0 ** -20)


def check_self_play_output(a, row, max_depth=256):
    """What a self-play result must satisfy whatever the oracle says, from its own arrays (records in episode order: merge_order = False),
    in float64 / integers.  `a`: obs [R, cells], logits [R, 4] (the MCTS probabilities), remaining_values [R], ep_len [E], ep_start [E].

    * Boards: every record's board is a permutation; within an episode it follows from the one before by the move of the blank that an
      action of non-zero probability makes -- or, at zero searches, it may stay: no child of the root is visited then, the reference falls
      back to 0.25 on all four actions, the masked ones too (search.rs:180-186), and an action into the wall changes only the depth
      (puzzle.rs:135-160).  An episode ends at its first final record: solved, or depth 0 after depth_slope x difficulty moves.
    * Probabilities (search.rs:168-186: the root is expanded before the first search, final or not; every search ends in a backpropagation
      through exactly one child of the root; the children's visit counts as f32, divided by their f32 sum): with S searches every
      probability is f32(v) / f32(S), bit for bit, for whole v >= 0 that add up to S, zero on masked actions; hence >= 0 and the float64
      sum of a record within SUM_BOUND of 1: each quotient is rounded once (relative error <= 2^-24), so |sum - 1| <= 2^-24 x sum, and the
      factor 1 + 2^-20 covers that sum being a little above 1 and the float64 additions.  At zero searches: exactly 0.25 four times.
    * remaining_values (az.rs:64-93): with val_t the reward of record t's state (1 solved, -0.5 out of depth, else -0.5 / max_depth,
      puzzle.rs:171-177), prefix_0 = 0, prefix_(t+1) = f32(prefix_t + val_t) and total = prefix_n: remaining_t = f32(total - prefix_t), bit for bit.
    """
    import numpy as np
    w, h, cells = row.w, row.h, row.w * row.h
    obs = a["obs"].astype(np.int64)
    L, S0 = a["ep_len"].astype(np.int64), a["ep_start"].astype(np.int64)
    R = len(obs)
    assert L.sum() == R and L.min() >= 1 and L.max() <= 2 * row.diff + 1
    assert np.array_equal(np.sort(S0), np.concatenate([[0], np.cumsum(L[np.argsort(S0, kind="stable")])[:-1]]))
    assert np.array_equal(obs // cells, np.broadcast_to(np.arange(cells), obs.shape))     # obs id of cell c holding tile v: cells x c + v
    board = obs % cells
    assert np.array_equal(np.sort(board, axis=1), np.broadcast_to(np.arange(cells), board.shape))
    blank = np.argmin(board, axis=1)
    zx, zy = blank % w, blank // w
    solved = np.all(board == np.arange(cells), axis=1)
    t = np.empty(R, np.int64)                      # index of a record in its episode
    for e in range(len(L)):
        t[S0[e]:S0[e] + L[e]] = np.arange(L[e])
    depth0 = 2 * row.diff
    final = solved | (t == depth0)
    last = np.zeros(R, bool); last[S0 + L - 1] = True
    assert np.array_equal(final, last), "an episode ends at its first final record and not before"
    # probabilities
    p = a["logits"].astype(np.float64)
    masks = np.stack([zx > 0, zy > 0, zx < w - 1, zy < h - 1], axis=1)
    fallback = np.full(R, row.S == 0)
    assert np.all(p >= 0.0)
    if row.S == 0:
        assert np.all(a["logits"] == np.float32(0.25)), "zero searches: 0.25 on every action"
    else:
        assert np.all(p[~masks] == 0.0), "probability on a masked action"
        assert np.all(np.abs(p.sum(axis=1) - 1.0) <= SUM_BOUND), float(np.max(np.abs(p.sum(axis=1) - 1.0)))
        visits = np.rint(p * row.S)
        assert np.array_equal(visits.sum(axis=1), np.full(R, float(row.S))), "the root's children were not visited num_searches times in all"
        quot = (visits.astype(np.float32) / np.float32(row.S)).astype(np.float32)
        assert np.array_equal(quot.view(np.uint32), np.ascontiguousarray(a["logits"], dtype=np.float32).view(np.uint32)), "a probability is not visits / searches"
    # moves
    nxt = np.flatnonzero(~last)
    moved = np.full(len(nxt), -1)
    dx, dy = zx[nxt + 1] - zx[nxt], zy[nxt + 1] - zy[nxt]
    for act, (ax, ay) in enumerate(((-1, 0), (0, -1), (1, 0), (0, 1))):
        moved[(dx == ax) & (dy == ay)] = act
    stay = (dx == 0) & (dy == 0)
    assert np.all((moved >= 0) | (stay & fallback[nxt])), "a record's board does not follow from the one before by one move of the blank"
    mv = np.flatnonzero(moved >= 0)
    i, act = nxt[mv], moved[mv]
    assert np.all(masks[i, act]) and np.all(p[i, act] > 0.0), "a move the record's distribution does not allow"
    want = board[i].copy()
    want[np.arange(len(i)), blank[i]] = board[i, blank[i + 1]]
    want[np.arange(len(i)), blank[i + 1]] = 0
    assert np.array_equal(board[i + 1], want), "more than the blank and its neighbour changed"
    st = nxt[stay]
    assert np.array_equal(board[st + 1], board[st])
    assert not masks[st].all(axis=1).any(), "a board stayed though every action was legal"
    # remaining_values
    f = np.float32
    val = np.where(solved, f(1.0), np.where(t == depth0, f(-0.5), f(-0.5) / f(max_depth))).astype(np.float32)
    rem = np.empty(R, np.float32)
    for e in range(len(L)):
        v = val[S0[e]:S0[e] + L[e]]
        prefix = np.zeros(L[e] + 1, np.float32)
        for k in range(L[e]):
            prefix[k + 1] = f(prefix[k] + v[k])
        rem[S0[e]:S0[e] + L[e]] = (prefix[L[e]] - prefix[:L[e]]).astype(np.float32)
    assert np.array_equal(rem.view(np.uint32), np.ascontiguousarray(a["remaining_values"], dtype=np.float32).view(np.uint32)), "remaining_values"
