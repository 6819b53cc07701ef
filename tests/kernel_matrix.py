"""Every PPO rollout kernel the library builds, one table row each, and the launch rule that picks it (GPU-free).

The rollout is a family of template instantiations: `rollout_f32_kernel<NT, NC, NW, PERSIST>` (tw_rollout.hip; Engine3 and
its small-batch shapes, EngineV for policies of any depth: NT = 0, NW = -65) and `rollout_f16_kernel<Engine16 | EngineS<NHT,
NC>, NC, PERSIST>` (tw_rollout16.hip; the fp16 and fp16x2 modes).  `dispatch(row, cus)` restates, in Python, how the library
gets from a collect to one of them and to its launch shape:

* tw_ppo_collect: the persistent rule (more episodes than resident lanes and no TW_OPT_NO_PERSIST -> episode queue);
* f32_resident_episodes / rollout_f32_resident_episodes / rollout_generic_resident_episodes (tw_rollout.hip);
* launch_rollout_f32 -> launch_nt -> launch_one -> geometry_for (tw_engine.hpp) -> launch_geom;
* launch_rollout_16 -> launch16_nc -> launch16 -> launch16p (tw_rollout16.hip).

tests/test_kernel_matrix.py holds the table against the kernels in the built assembly and pins the restatement to launch
shapes other tests assert; tests/test_gpu_kernel_matrix.py runs every row on the GPU and compares it with the oracle.

Row fields: board (w, h), embedding and hidden widths, episodes, precision, transpose twists, TW_OPT_FORCE_GEOM,
TW_OPT_NO_PERSIST, `reserve` ("all_but_one": reserve_cus = CUs - 1, so that a few hundred episodes already overflow the one
persistent workgroup left and take the queue), `common` (a tuple: a generic policy with these common layers) and the
scramble difficulty (short: 3..6 moves).
"""
from collections import namedtuple

EPW = 32                       # episodes per wave of Engine3 (tw_engine.hpp)

Row = namedtuple("Row", "w h emb hidden E prec twists force_geom no_persist reserve common diff")


def R(w, h, emb, hidden, E, prec="fp32", twists=False, force_geom=0, no_persist=False, reserve=None, common=None, diff=4):
    return Row(w, h, emb, hidden, E, prec, twists, force_geom, no_persist, reserve, common, diff)


AB1 = "all_but_one"

# one row per instantiation; the comment names it (f32: <NT, NC, NW, PERSIST>; f16: <Engine<NHT, NC>, NC, PERSIST>)
TABLE = [
    # ---- Engine3, 32 hidden units (NT = 1): 32-, 64- and 256-episode workgroups, persistent 256
    R(2, 2, 32, 32, 300),                                     # f32 <1, 4, 1, false>
    R(2, 2, 32, 32, 12800, diff=3),                           # f32 <1, 4, 2, false>
    R(2, 2, 64, 32, 300, force_geom=8, twists=True),          # f32 <1, 4, 8, false>
    R(2, 2, 32, 32, 300, reserve=AB1),                        # f32 <1, 4, 8, true>
    R(3, 3, 32, 32, 300, twists=True),                        # f32 <1, 9, 1, false>
    R(3, 2, 32, 32, 12800, diff=3),                           # f32 <1, 9, 2, false>
    R(3, 3, 96, 32, 300, force_geom=8),                       # f32 <1, 9, 8, false>
    R(3, 3, 32, 32, 300, reserve=AB1, twists=True),           # f32 <1, 9, 8, true>
    R(4, 4, 32, 32, 300),                                     # f32 <1, 16, 1, false>
    R(4, 3, 32, 32, 12800, diff=3),                           # f32 <1, 16, 2, false>
    R(4, 4, 64, 32, 300, force_geom=8, twists=True),          # f32 <1, 16, 8, false>
    R(4, 3, 32, 32, 300, reserve=AB1),                        # f32 <1, 16, 8, true>
    # ---- 64 hidden units (NT = 2): 32-episode workgroups of two waves, 256-episode ones, persistent 256
    R(2, 2, 32, 64, 300),                                     # f32 <2, 4, -2, false>
    R(2, 2, 64, 64, 300, force_geom=8),                       # f32 <2, 4, 8, false>
    R(2, 2, 32, 64, 300, reserve=AB1, twists=True),           # f32 <2, 4, 8, true>
    R(3, 3, 64, 64, 300, twists=True),                        # f32 <2, 9, -2, false>
    R(3, 2, 32, 64, 300, force_geom=8),                       # f32 <2, 9, 8, false>
    R(3, 3, 64, 64, 300, reserve=AB1),                        # f32 <2, 9, 8, true>
    R(4, 4, 32, 64, 300),                                     # f32 <2, 16, -2, false>
    R(4, 4, 64, 64, 300, force_geom=8, twists=True),          # f32 <2, 16, 8, false>
    R(4, 3, 32, 64, 300, reserve=AB1),                        # f32 <2, 16, 8, true>
    # ---- 128 hidden units (NT = 4): 16-episode workgroups, 32-episode ones (plain and queued), 256 (plain and queued)
    R(2, 2, 32, 128, 300),                                    # f32 <4, 4, -16, false>
    R(2, 2, 64, 128, 300, force_geom=32, twists=True),        # f32 <4, 4, -4, false>
    R(2, 2, 32, 128, 300, reserve=AB1),                       # f32 <4, 4, -4, true>
    R(2, 2, 32, 128, 300, force_geom=8),                      # f32 <4, 4, 8, false>
    R(2, 2, 64, 128, 300, force_geom=8, reserve=AB1),         # f32 <4, 4, 8, true>
    R(3, 3, 64, 128, 300, twists=True),                       # f32 <4, 9, -16, false>
    R(3, 2, 32, 128, 300, force_geom=32),                     # f32 <4, 9, -4, false>
    R(3, 3, 32, 128, 300, reserve=AB1, twists=True),          # f32 <4, 9, -4, true>
    R(3, 3, 96, 128, 300, force_geom=8),                      # f32 <4, 9, 8, false>
    R(3, 2, 32, 128, 300, force_geom=8, reserve=AB1),         # f32 <4, 9, 8, true>
    R(4, 3, 32, 128, 300),                                    # f32 <4, 16, -16, false>
    R(4, 4, 64, 128, 300, force_geom=32),                     # f32 <4, 16, -4, false>
    R(4, 4, 32, 128, 300, reserve=AB1, twists=True),          # f32 <4, 16, -4, true>
    R(4, 4, 32, 128, 300, force_geom=8, twists=True),         # f32 <4, 16, 8, false>
    R(4, 3, 64, 128, 300, force_geom=8, reserve=AB1),         # f32 <4, 16, 8, true>
    # ---- 256 hidden units (NT = 8)
    R(2, 2, 64, 256, 300, twists=True),                       # f32 <8, 4, -16, false>
    R(2, 2, 32, 256, 300, force_geom=32),                     # f32 <8, 4, -4, false>
    R(2, 2, 32, 256, 300, reserve=AB1),                       # f32 <8, 4, -4, true>
    R(2, 2, 32, 256, 300, force_geom=8, twists=True),         # f32 <8, 4, 8, false>
    R(2, 2, 32, 256, 300, force_geom=8, reserve=AB1),         # f32 <8, 4, 8, true>
    R(3, 3, 32, 256, 300),                                    # f32 <8, 9, -16, false>
    R(3, 3, 64, 256, 300, force_geom=32, twists=True),        # f32 <8, 9, -4, false>
    R(3, 2, 32, 256, 300, reserve=AB1),                       # f32 <8, 9, -4, true>
    R(3, 3, 32, 256, 300, force_geom=8),                      # f32 <8, 9, 8, false>
    R(3, 3, 64, 256, 300, force_geom=8, reserve=AB1, twists=True),   # f32 <8, 9, 8, true>
    R(4, 4, 512, 256, 300, twists=True),                      # f32 <8, 16, -16, false>
    R(4, 3, 32, 256, 300, force_geom=32),                     # f32 <8, 16, -4, false>
    R(4, 4, 64, 256, 300, reserve=AB1, twists=True),          # f32 <8, 16, -4, true>
    R(4, 4, 32, 256, 300, force_geom=8),                      # f32 <8, 16, 8, false>
    R(4, 4, 32, 256, 300, force_geom=8, reserve=AB1),         # f32 <8, 16, 8, true>
    # ---- EngineV: policies of any depth (16-episode workgroups; two per CU for these small stacks)
    R(2, 2, 32, 0, 300, common=(48,)),                        # f32 <0, 4, -65, false>
    R(2, 2, 32, 0, 300, common=(64, 32), reserve=AB1),        # f32 <0, 4, -65, true>
    R(3, 3, 64, 0, 300, common=(48, 40), twists=True),        # f32 <0, 9, -65, false>
    R(3, 2, 32, 0, 300, common=(96,), reserve=AB1),           # f32 <0, 9, -65, true>
    R(4, 4, 64, 0, 300, common=(80,)),                        # f32 <0, 16, -65, false>
    R(4, 3, 32, 0, 300, common=(48, 24), reserve=AB1),        # f32 <0, 16, -65, true>
    # ---- Engine16 (fp16): 256 episodes per workgroup, persistent one per CU
    R(2, 2, 32, 32, 300, "fp16"),                             # f16 <Engine16<1, 4>, 4, false>
    R(2, 2, 64, 32, 300, "fp16", reserve=AB1),                # f16 <Engine16<1, 4>, 4, true>
    R(3, 3, 32, 32, 300, "fp16", twists=True),                # f16 <Engine16<1, 9>, 9, false>
    R(3, 2, 64, 32, 300, "fp16", reserve=AB1),                # f16 <Engine16<1, 9>, 9, true>
    R(4, 4, 64, 32, 300, "fp16"),                             # f16 <Engine16<1, 16>, 16, false>
    R(4, 4, 32, 32, 300, "fp16", reserve=AB1, twists=True),   # f16 <Engine16<1, 16>, 16, true>
    R(2, 2, 96, 64, 300, "fp16", twists=True),                # f16 <Engine16<2, 4>, 4, false>
    R(2, 2, 32, 64, 300, "fp16", reserve=AB1),                # f16 <Engine16<2, 4>, 4, true>
    R(3, 2, 64, 64, 300, "fp16"),                             # f16 <Engine16<2, 9>, 9, false>
    R(3, 3, 96, 64, 300, "fp16", reserve=AB1, twists=True),   # f16 <Engine16<2, 9>, 9, true>
    R(4, 3, 32, 64, 300, "fp16"),                             # f16 <Engine16<2, 16>, 16, false>
    R(4, 4, 64, 64, 300, "fp16", reserve=AB1),                # f16 <Engine16<2, 16>, 16, true>
    R(2, 2, 64, 128, 300, "fp16"),                            # f16 <Engine16<4, 4>, 4, false>
    R(2, 2, 32, 128, 300, "fp16", reserve=AB1, twists=True),  # f16 <Engine16<4, 4>, 4, true>
    R(3, 3, 128, 128, 300, "fp16"),                           # f16 <Engine16<4, 9>, 9, false>
    R(3, 3, 64, 128, 300, "fp16", reserve=AB1),               # f16 <Engine16<4, 9>, 9, true>
    R(4, 4, 96, 128, 300, "fp16", twists=True),               # f16 <Engine16<4, 16>, 16, false>
    R(4, 3, 64, 128, 300, "fp16", reserve=AB1),               # f16 <Engine16<4, 16>, 16, true>
    R(2, 2, 64, 256, 300, "fp16", twists=True),               # f16 <Engine16<8, 4>, 4, false>
    R(2, 2, 32, 256, 300, "fp16", reserve=AB1),               # f16 <Engine16<8, 4>, 4, true>
    R(3, 3, 64, 256, 300, "fp16"),                            # f16 <Engine16<8, 9>, 9, false>
    R(3, 3, 32, 256, 300, "fp16", reserve=AB1, twists=True),  # f16 <Engine16<8, 9>, 9, true>
    R(4, 4, 512, 256, 300, "fp16", twists=True),              # f16 <Engine16<8, 16>, 16, false>
    R(4, 4, 64, 256, 300, "fp16", reserve=AB1),               # f16 <Engine16<8, 16>, 16, true>
    # ---- EngineS (fp16x2: split-f16, at least two embedding tiles)
    R(2, 2, 64, 32, 300, "fp16x2"),                           # f16 <EngineS<1, 4>, 4, false>
    R(2, 2, 96, 32, 300, "fp16x2", reserve=AB1, twists=True), # f16 <EngineS<1, 4>, 4, true>
    R(3, 3, 64, 32, 300, "fp16x2", twists=True),              # f16 <EngineS<1, 9>, 9, false>
    R(3, 2, 64, 32, 300, "fp16x2", reserve=AB1),              # f16 <EngineS<1, 9>, 9, true>
    R(4, 4, 96, 32, 300, "fp16x2"),                           # f16 <EngineS<1, 16>, 16, false>
    R(4, 4, 64, 32, 300, "fp16x2", reserve=AB1, twists=True), # f16 <EngineS<1, 16>, 16, true>
    R(2, 2, 128, 64, 300, "fp16x2", twists=True),             # f16 <EngineS<2, 4>, 4, false>
    R(2, 2, 64, 64, 300, "fp16x2", reserve=AB1),              # f16 <EngineS<2, 4>, 4, true>
    R(3, 2, 96, 64, 300, "fp16x2"),                           # f16 <EngineS<2, 9>, 9, false>
    R(3, 3, 64, 64, 300, "fp16x2", reserve=AB1, twists=True), # f16 <EngineS<2, 9>, 9, true>
    R(4, 3, 64, 64, 300, "fp16x2"),                           # f16 <EngineS<2, 16>, 16, false>
    R(4, 4, 128, 64, 300, "fp16x2", reserve=AB1),             # f16 <EngineS<2, 16>, 16, true>
    R(2, 2, 64, 128, 300, "fp16x2"),                          # f16 <EngineS<4, 4>, 4, false>
    R(2, 2, 96, 128, 300, "fp16x2", reserve=AB1, twists=True),# f16 <EngineS<4, 4>, 4, true>
    R(3, 3, 128, 128, 300, "fp16x2", twists=True),            # f16 <EngineS<4, 9>, 9, false>
    R(3, 3, 64, 128, 300, "fp16x2", reserve=AB1),             # f16 <EngineS<4, 9>, 9, true>
    R(4, 4, 64, 128, 300, "fp16x2"),                          # f16 <EngineS<4, 16>, 16, false>
    R(4, 3, 96, 128, 300, "fp16x2", reserve=AB1),             # f16 <EngineS<4, 16>, 16, true>
    R(2, 2, 64, 256, 300, "fp16x2", twists=True),             # f16 <EngineS<8, 4>, 4, false>
    R(2, 2, 64, 256, 300, "fp16x2", reserve=AB1),             # f16 <EngineS<8, 4>, 4, true>
    R(3, 3, 96, 256, 300, "fp16x2"),                          # f16 <EngineS<8, 9>, 9, false>
    R(3, 3, 64, 256, 300, "fp16x2", reserve=AB1, twists=True),# f16 <EngineS<8, 9>, 9, true>
    R(4, 4, 512, 256, 300, "fp16x2", twists=True),            # f16 <EngineS<8, 16>, 16, false>
    R(4, 4, 64, 256, 300, "fp16x2", reserve=AB1),             # f16 <EngineS<8, 16>, 16, true>
]


def reserve_cus(row, cus):
    return cus - 1 if row.reserve == AB1 else 0


def waves_per_group(n):
    """tw_common.hpp waves_per_group."""
    if (n + 255) // 256 >= 156:
        return 8
    if (n + 63) // 64 >= 192:
        return 2
    return 1


def resident_full(cus, reserve=0):
    """rollout_f32_resident_episodes: one 256-episode workgroup per CU not reserved."""
    return (cus - min(max(reserve, 0), cus - 1)) * 8 * EPW


def f32_resident(E, hidden, cus, reserve=0, force_geom=0):
    """f32_resident_episodes (PPO): CUs x 32 between that and the 256-episode crossover for >= 128 hidden units."""
    full = resident_full(cus, reserve)
    small = full // 8
    if hidden >= 128 and E > small and waves_per_group(E) != 8 and not force_geom:
        return small
    return full


def geometry_for(NT, n, cus, force_geom=0):
    """tw_engine.hpp geometry_for (its resident count takes no reserved CUs)."""
    nw = waves_per_group(n)
    if force_geom:
        nw = 8 if force_geom == 8 else 1
    if nw == 8 or NT < 2:
        return nw
    if NT >= 4 and n <= resident_full(cus) // 16 and force_geom != 32:
        return -16
    return -4 if NT >= 4 else -2


def n_chunks(cells):
    return 4 if cells <= 4 else (9 if cells <= 9 else 16)


# workgroup (episodes, threads) of each f32 geometry: Engine3<NW> (NW x 32, 64 NW), Engine3S (32), Engine3T (16), EngineV (16)
F32_BLOCK = {8: (256, 512), 2: (64, 128), 1: (32, 64), -2: (32, 128), -4: (32, 256), -16: (16, 256), -65: (16, 256)}
GENERIC_GROUPS_PER_CU = 2      # generic_groups_per_cu(): two 16-episode workgroups per CU when twice the LDS fits (all table rows)


def dispatch(row, cus):
    """-> (kernel, (rollout_blocks, rollout_threads)); kernel as in kernel_name()."""
    E, cells = row.E, row.w * row.h
    nc = n_chunks(cells)
    res = reserve_cus(row, cus)
    full = resident_full(cus, res)
    if row.prec != "fp32":
        nht = row.hidden // 32
        persist = E > full and not row.no_persist                        # tw_ppo_collect, launch16
        eng = "Engine16" if row.prec == "fp16" else "EngineS"
        blocks = full // 256 if persist else -(-E // 256)
        return ("f16", eng, nht, nc, persist), (blocks, 256)
    if row.common is not None:                                           # generic stacks: EngineV
        resident = (cus - res) * GENERIC_GROUPS_PER_CU * 16
        persist = E > resident and not row.no_persist
        blocks = (cus - res) * GENERIC_GROUPS_PER_CU if persist else -(-E // 16)
        return ("f32", 0, nc, -65, persist), (blocks, 256)
    NT = row.hidden // 32
    resident = f32_resident(E, row.hidden, cus, res, row.force_geom)
    persist = E > resident and not row.no_persist                        # tw_ppo_collect
    if persist:                                                          # launch_one, queue set
        nw = -4 if NT >= 4 and resident < full else 8
        return ("f32", NT, nc, nw, True), (full // 256, F32_BLOCK[nw][1])
    nw = geometry_for(NT, E, cus, row.force_geom)
    if (NT >= 4 and nw not in (-16, -4)) or (NT == 2 and nw != -2) or (NT == 1 and nw not in (1, 2)):
        nw = 8
    ep, threads = F32_BLOCK[nw]
    return ("f32", NT, nc, nw, False), (-(-E // ep), threads)


def kernel_name(k):
    """('f32', NT, NC, NW, P) -> 'rollout_f32_kernel<NT, NC, NW, P>'; ('f16', eng, NHT, NC, P) -> 'rollout_f16_kernel<eng<NHT, NC>, NC, P>'."""
    if k[0] == "f32":
        _, nt, nc, nw, p = k
        return f"rollout_f32_kernel<{nt}, {nc}, {nw}, {str(p).lower()}>"
    _, eng, nht, nc, p = k
    return f"rollout_f16_kernel<{eng}<{nht}, {nc}>, {nc}, {str(p).lower()}>"


def row_id(row):
    return (f"{row.prec}-{row.w}x{row.h}-e{row.emb}-" + (f"c{'.'.join(map(str, row.common))}" if row.common else f"h{row.hidden}") +
            f"-E{row.E}" + ("-tw" if row.twists else "") + (f"-g{row.force_geom}" if row.force_geom else "") +
            ("-np" if row.no_persist else "") + ("-r" if row.reserve else ""))
