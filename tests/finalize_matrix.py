"""Every form of the collectors' tail -- the episode-length scan, GAE / remaining values and compaction, the obs and logits movers --
one table row each, the launch rules themselves, a deterministic record generator and the plain numpy references (GPU-free).

Every device collector ends in `collect_tail` (tw_api.hip): `launch_scan` (scan_tile_sums, scan_tile_offsets, scan_write),
`launch_finalize_ppo` (finalize_ppo_group_kernel<16>, <8> or finalize_ppo_kernel, tw_finalize.hip) or `launch_finalize_az`
(finalize_az_kernel, tw_mcts.hip), then compact_obs16_kernel / compact_env_obs8_kernel for ids that have their own array and
for more than four columns, narrow_logits_kernel for fewer.  Which kernel runs, with how many waves and on what grid, depends
on the horizon `t_pad`, on where the obs ids live and on the episode count.  This module restates those rules in Python and
lists the smallest shapes that reach every form, both sides of every switch, a second grid-stride trip of every capped kernel
and a second trip of the scan's carry loop.

tests/test_finalize_matrix.py holds the table against the restated rules and the references against the oracle and float64;
tests/test_gpu_finalize.py drives every row through `tw_debug_collect_tail` on the GPU and compares every field as bits.

A row: Case(kind, E, t_pad, n_cells, ids, A, values, gamma, lam)
  kind    "ppo" | "az"
  ids     0: the obs ids are the first n_cells bytes of the records; 1 / 2: they have their own two-byte array and are written out
          at one / two bytes each (the finalize kernel then sees 0 cells)
  values  "normal": modest finite values; "special": episode e is of class e % 5 -- all -0.0, denormals, magnitudes near 3e38,
          raw hash bits (signalling and payload NaNs among them), normal
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "kind E t_pad n_cells ids A values gamma lam")

SCAN_THREADS, SCAN_ITEMS = 256, 4
SCAN_TILE = SCAN_THREADS * SCAN_ITEMS        # episodes per tile (tw_finalize.hip)
SCAN_CARRY_STEP = SCAN_THREADS               # tile sums per trip of scan_tile_offsets' loop; the carry crosses trips
LDS_LIMIT = 64 * 1024
FIN_WAVES = AZF_WAVES = 4
WAVE_GRID_CAP = 256 * 16                     # finalize_ppo_kernel, finalize_az_kernel, both obs movers, narrow_logits_kernel
GROUP16, GROUP8, WAVE, AZ = 1, 2, 3, 4       # TW_FIN_* (include/twisterl_hip.h)
FORM_NAMES = {GROUP16: "group16", GROUP8: "group8", WAVE: "wave", AZ: "az"}
AZ_MAX_T_PAD = LDS_LIMIT // (AZF_WAVES * 2 * 4)
GAMMA, LAM = 0.995, 0.95
FILL = 0xA5                                  # the arena fill byte of the GPU tests
POISON_F32 = 0x7FA5DEAD                      # padding records: a signalling NaN in every float, 0xFF in every other byte
REC_WORDS = 12                               # a padded record: 48 bytes


# ------------------------------------------------------------------------------------------ the launch rules
def rec_cells(case):
    """The n_cells the finalize launchers see (collect_tail): 0 where the ids have their own array."""
    return 0 if case.ids else case.n_cells


def fin_wave_bytes(t_pad, cells):
    return ((5 if cells == 16 else 9) * t_pad * 4 + 15) // 16 * 16


def fin_group_bytes(g, t_pad, cells):
    return g * (t_pad | 1) * 8 + (0 if cells in (16, 0) else g * t_pad * 16)


def ppo_max_t_pad(cells):
    t = 1
    while fin_wave_bytes(t + 1, cells) <= LDS_LIMIT:
        t += 1
    return t


def dispatch(kind, E, t_pad, cells):
    """launch_finalize_ppo / launch_finalize_az -> dict(form, waves, blocks, threads, lds_bytes), or None where they refuse."""
    if kind == "az":
        lds = AZF_WAVES * 2 * t_pad * 4
        if lds > LDS_LIMIT:
            return None
        return dict(form=AZ, waves=AZF_WAVES, blocks=min((E + AZF_WAVES - 1) // AZF_WAVES, WAVE_GRID_CAP), threads=AZF_WAVES * 64, lds_bytes=lds)
    for form, g in ((GROUP16, 16), (GROUP8, 8)):
        lds = fin_group_bytes(g, t_pad, cells)
        if lds <= LDS_LIMIT:
            per_cu = min(160 * 1024 // lds, 8)
            return dict(form=form, waves=4, blocks=min((E + g - 1) // g, 256 * per_cu * 2), threads=256, lds_bytes=lds)
    per_wave, waves = fin_wave_bytes(t_pad, cells), FIN_WAVES
    while waves > 1 and waves * per_wave > LDS_LIMIT:
        waves >>= 1
    if waves * per_wave > LDS_LIMIT:
        return None
    return dict(form=WAVE, waves=waves, blocks=min((E + waves - 1) // waves, WAVE_GRID_CAP), threads=waves * 64, lds_bytes=waves * per_wave)


def case_dispatch(case):
    return dispatch(case.kind, case.E, case.t_pad, rec_cells(case))


def finalize_trips(case):
    """Trips of the finalize kernel's grid-stride loop that the busiest workgroup makes."""
    d = case_dispatch(case)
    per_block = {GROUP16: 16, GROUP8: 8}.get(d["form"], d["waves"])
    return -(-case.E // (per_block * d["blocks"]))


def mover_trips(E):
    """Trips of compact_obs16_kernel / compact_env_obs8_kernel: a wave per episode, four per workgroup, at most WAVE_GRID_CAP."""
    blocks = min((E + 3) // 4, WAVE_GRID_CAP)
    return -(-E // (4 * blocks))


def scan_tiles(E):
    return (E + SCAN_TILE - 1) // SCAN_TILE


def scan_carry_trips(E):
    return -(-scan_tiles(E) // SCAN_CARRY_STEP)


def movers(case):
    """The kernels beside finalize that collect_tail launches for a row."""
    out = []
    if case.ids:
        out.append("compact_obs16_kernel" if case.ids == 2 else "compact_env_obs8_kernel")
    if case.A > 4:
        out.append("compact_obs16_kernel")
    if case.A < 4:
        out.append("narrow_logits_kernel")
    return out


# ------------------------------------------------------------------------------------------ the table
def _ppo(E, t_pad, n_cells=16, ids=0, A=4, values="normal", gamma=GAMMA, lam=LAM):
    return Case("ppo", E, t_pad, n_cells, ids, A, values, gamma, lam)


def _az(E, t_pad, n_cells=16, ids=0, A=4, values="normal"):
    return Case("az", E, t_pad, n_cells, ids, A, values, 0.0, 0.0)


E0 = 37
CELL16_T = [1, 2, 511, 512, 1023, 1024, 1638, 1639, 3276]
STAGED_T = [170, 171, 341, 342, 455, 456, 910, 911, 1820]
IDS_T = [511, 512, 1023, 1024, 1820]

FORMS = ([_ppo(E0, t) for t in CELL16_T]
         + [_ppo(E0, t, n_cells=nc) for nc in (1, 9, 15) for t in STAGED_T]
         + [_ppo(E0, t, n_cells=nc, ids=w) for w in (1, 2) for nc in (1, 25, 64) for t in IDS_T])
# E around the episodes of a workgroup: G = 16 (16-cell, t_pad 65) and G = 8 (staged, t_pad 171)
GROUP_EDGES = ([_ppo(E, 65) for E in (1, 15, 16, 17, 67)] + [_ppo(E, 171, n_cells=9) for E in (1, 7, 8, 9, 35)])
COLUMNS = ([_ppo(E0, 65, A=A) for A in (1, 2, 3, 4, 5, 31)] + [_ppo(E0, 65, n_cells=25, ids=2, A=A) for A in (3, 31)]
           + [_az(E0, 65, A=A) for A in (1, 2, 3, 4, 5, 31)] + [_az(E0, 65, n_cells=25, ids=1, A=A) for A in (3, 31)])
AZ_HORIZONS = [_az(E0, t) for t in (1, 2, 2048)] + [_az(E0, 300, n_cells=9), _az(E0, 300, n_cells=64, ids=2)]
# the smallest shapes whose busiest workgroup makes a second trip of its grid-stride loop
SECOND_TRIPS = [_ppo(65536 + 69, 2),                          # group 16: 4,096 workgroups of 16 episodes
                _ppo(16384 + 13, 171, n_cells=9),              # group 8: 2,048 workgroups of 8 (two fit a CU's LDS)
                _ppo(16384 + 5, 342, n_cells=9),               # wave: 4,096 workgroups of 4
                _az(16384 + 5, 2),                             # AZ: 4,096 workgroups of 4
                _ppo(16384 + 5, 2, n_cells=25, ids=1), _ppo(16384 + 5, 2, n_cells=25, ids=2),    # both obs movers
                _az(16384 + 5, 2, n_cells=25, ids=2, A=5)]     # ... and the mover on wide rows
SCAN_E = [1, 2, 1023, 1024, 1025, 4097, 262144, 262145, 263171, 524293]
SCAN_WITH_RECORDS = [_ppo(263171, 2), _az(263171, 2)]
SPECIAL_PARAMS = [(GAMMA, LAM), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.0, 0.0)]
VALUES = ([_ppo(E0, t, n_cells=nc, values="special", gamma=g, lam=l)
           for (t, nc) in ((65, 16), (600, 16), (1100, 16), (400, 9)) for g, l in SPECIAL_PARAMS] + [_az(E0, 300, values="special")])

REFUSED = [_ppo(E0, 3277), _ppo(E0, 1821, n_cells=9), _ppo(E0, 1821, n_cells=1), _ppo(E0, 1821, n_cells=15), _ppo(E0, 1821, n_cells=25, ids=2),
           _az(E0, 2049)]

TABLE = FORMS + GROUP_EDGES + COLUMNS + AZ_HORIZONS + SECOND_TRIPS + SCAN_WITH_RECORDS + VALUES


def case_id(c):
    ids = {0: "", 1: "-ids8", 2: "-ids16"}[c.ids]
    extra = "" if c.values == "normal" else f"-{c.values}-g{c.gamma:g}-l{c.lam:g}"
    return f"{c.kind}-E{c.E}-t{c.t_pad}-c{c.n_cells}{ids}-A{c.A}{extra}"


# ------------------------------------------------------------------------------------------ deterministic inputs
def mix32(x, salt):
    """murmur3's 32-bit finaliser over x * golden ratio + salt: uint32 array -> uint32 array."""
    h = (x.astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(salt * 0x85EBCA6B & 0xFFFFFFFF)).astype(np.uint32)
    h ^= h >> np.uint32(16); h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13); h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def episode_lengths(E, t_pad, seed=7):
    """uint32 [E]: 1, 2, 63, 64, 65, t_pad - 1, t_pad (those that fit) and hashed lengths of 1 .. t_pad, the last of them adjusted so
    that the record total is odd where it can be: no field of the result then ends on a 256-byte boundary."""
    L = (mix32(np.arange(E, dtype=np.uint32), seed) % np.uint32(t_pad) + 1).astype(np.uint32)
    fixed = [x for x in dict.fromkeys([1, 2, 63, 64, 65, t_pad - 1, t_pad]) if 1 <= x <= t_pad]
    n = min(len(fixed), E)
    L[(np.arange(n) * 5) % E if E >= 5 * n else np.arange(n)] = fixed[:n]
    if int(L.sum(dtype=np.uint64)) % 2 == 0 and t_pad > 1:
        L[E - 1] = L[E - 1] - 1 if L[E - 1] > 1 else 2
    return L


def _normal_f32(h):
    """Hash -> a finite float32 of modest size with a full mantissa: (-8, 8)."""
    return ((h.astype(np.int64) - (1 << 31)).astype(np.float64) / float(1 << 28)).astype(np.float32)


def make_inputs(case, ep_len):
    """(records uint32 [E * t_pad][12], obs16 uint16 [E * t_pad][n_cells] or None, wide float32 [E * t_pad][A] or None): every byte a hash
    of (e, t) and the field, records at and beyond ep_len[e] poisoned."""
    E, T = case.E, case.t_pad
    idx = np.arange(E * T, dtype=np.uint32)
    live = (idx % np.uint32(T)) < np.repeat(ep_len.astype(np.uint32), T)
    rec = np.empty((E * T, REC_WORDS), dtype=np.uint32)
    for w in range(4):
        rec[:, w] = mix32(idx, 1 + w)
    for w in range(4, 10):
        rec[:, w] = _normal_f32(mix32(idx, 1 + w)).view(np.uint32)
    rec[:, 10] = mix32(idx, 11)                       # action | perm << 8 | 16 bits no kernel may let through
    rec[:, 11] = mix32(idx, 12)                       # unused
    if case.values == "special":
        cls = np.repeat(np.arange(E, dtype=np.uint32) % 5, T)
        h8, h9 = mix32(idx, 21), mix32(idx, 22)
        f = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)
        sign = lambda h: (h & np.uint32(0x80000000))
        for w, h in ((8, h8), (9, h9)):
            col = rec[:, w]
            col[cls == 0] = 0x80000000                                                           # -0.0
            den = np.where(h & 1, f(np.full(idx.size, 1e-41)), f(np.full(idx.size, -3e-42)))
            col[cls == 1] = den[cls == 1]
            big = (f(np.full(idx.size, 3e38)) - (h >> np.uint32(12))) | sign(h)                   # (2.9e38 .. 3e38, either sign)
            col[cls == 2] = big[cls == 2]
            col[cls == 3] = h[cls == 3]
        raw = cls == 3
        for w in range(4, 8):
            rec[raw, w] = mix32(idx, 30 + w)[raw]
        # a signalling and a payload NaN in every copied float field of the first record of the raw-bits episodes
        first = np.flatnonzero(raw & (idx % np.uint32(T) == 0))
        rec[first, 4], rec[first, 5], rec[first, 8], rec[first, 9] = 0x7F800001, 0xFFC12345, 0x7FA00000, 0xFFFFFFFF
    rec[~live, :4] = 0xFFFFFFFF
    rec[~live, 4:10] = POISON_F32
    rec[~live, 10:] = 0xFFFFFFFF
    obs16 = wide = None
    if case.ids:
        obs16 = np.empty((E * T, case.n_cells), dtype=np.uint16)
        for c in range(case.n_cells):
            obs16[:, c] = mix32(idx, 100 + c) & np.uint32(0xFF if case.ids == 1 else 0xFFFF)
        obs16[~live] = 0xFFFF
    if case.A > 4:
        wide = np.empty((E * T, case.A), dtype=np.uint32)
        for c in range(case.A):
            wide[:, c] = _normal_f32(mix32(idx, 200 + c)).view(np.uint32) if case.values == "normal" else mix32(idx, 200 + c)
        wide[~live] = POISON_F32
        wide = wide.view(np.float32)
    return rec, obs16, wide


# ------------------------------------------------------------------------------------------ references
def ep_start_ref(ep_len, merge_order):
    """(ep_start uint64 [E], total): exclusive prefix sums of the lengths in the OUTPUT order -- merge order: the last episode first,
    then 0 .. E-2 (collector.rs:40-46)."""
    L = np.asarray(ep_len, dtype=np.uint64)
    order = np.concatenate([[L.size - 1], np.arange(L.size - 1)]).astype(np.int64) if merge_order else np.arange(L.size)
    csum = np.cumsum(L[order], dtype=np.uint64)
    start = np.empty(L.size, dtype=np.uint64)
    start[order] = csum - L[order]
    return start, int(csum[-1])


def gae_f32_episodes(rews, vals, ep_len, gamma, lam):
    """The chain of ppo.rs:82-92 in float32, one rounding per operation in the reference's order, over consecutive episodes of
    lengths ep_len, vectorised across the episodes -> (advs, rets) float32."""
    L = np.asarray(ep_len, np.int64)
    starts = np.concatenate([[0], np.cumsum(L)[:-1]])
    r, v = np.asarray(rews, np.float32), np.asarray(vals, np.float32)
    g, l = np.float32(gamma), np.float32(lam)
    advs, rets = np.empty(r.size, np.float32), np.empty(r.size, np.float32)
    nxt_v, nxt_a = np.zeros(L.size, np.float32), np.zeros(L.size, np.float32)
    with np.errstate(all="ignore"):
        for k in range(int(L.max()) if L.size else 0):
            live = L > k
            idx = starts[live] + L[live] - 1 - k
            if k == 0:
                ret = r[idx]
            else:
                inner = l * nxt_a[live]
                inner = nxt_v[live] + inner
                inner = g * inner
                ret = r[idx] + inner
            adv = ret - v[idx]
            rets[idx], advs[idx] = ret, adv
            nxt_v[live], nxt_a[live] = v[idx], adv
    return advs, rets


def remaining_f32_episodes(rews, ep_len):
    """az.rs:64,74-76,93 in float32: remaining[t] = total - (sum of the rewards before t), the sums sequential from t = 0."""
    L = np.asarray(ep_len, np.int64)
    starts = np.concatenate([[0], np.cumsum(L)[:-1]])
    r = np.asarray(rews, np.float32)
    prefix, run = np.empty(r.size, np.float32), np.zeros(L.size, np.float32)
    with np.errstate(all="ignore"):
        for k in range(int(L.max()) if L.size else 0):
            live = L > k
            idx = starts[live] + k
            prefix[idx] = run[live]
            run[live] = run[live] + r[idx]
        return np.repeat(run, L) - prefix


def reference(case, ep_len, rec, obs16, wide, merge_order):
    """Every field of the result as the bytes it must hold: {name: array}.  advs / rets / remaining are float32 (compare by
    same_or_nan), everything else is compared as bytes."""
    E, T, A, NC = case.E, case.t_pad, case.A, case.n_cells
    L = np.asarray(ep_len, np.int64)
    order = np.concatenate([[E - 1], np.arange(E - 1)]).astype(np.int64) if merge_order else np.arange(E)
    Lo = L[order]
    out_start = np.concatenate([[0], np.cumsum(Lo)[:-1]])
    total = int(Lo.sum())
    src = np.repeat(order * T - out_start, Lo) + np.arange(total)        # the padded record behind every compact one
    r = rec[src]
    out = {}
    if case.ids:
        o = obs16[src]
        out["obs"] = o.astype(np.uint8) if case.ids == 1 else o
    else:
        out["obs"] = np.ascontiguousarray(r[:, :4]).view(np.uint8).reshape(total, 16)[:, :NC]
    out["logits"] = wide.view(np.uint32)[src] if A > 4 else r[:, 4:4 + A]
    if case.kind == "ppo":
        out["perms"] = ((r[:, 10] >> np.uint32(8)) & np.uint32(0xFF)).astype(np.uint8)
        out["values"], out["rewards"] = r[:, 8], r[:, 9]
        out["actions"] = (r[:, 10] & np.uint32(0xFF)).astype(np.uint8)
        adv, ret = gae_f32_episodes(r[:, 9].copy().view(np.float32), r[:, 8].copy().view(np.float32), Lo, case.gamma, case.lam)
        out["advs"], out["rets"] = adv, ret
    else:
        out["perms"] = np.full(total, 0xFF, dtype=np.uint8)
        out["remaining"] = remaining_f32_episodes(r[:, 9].copy().view(np.float32), Lo)
    out["ep_len"] = np.asarray(ep_len, dtype=np.uint32)
    out["ep_start"] = ep_start_ref(ep_len, merge_order)[0]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


COMPUTED = ("advs", "rets", "remaining")


def same_or_nan(got, want):
    """Computed float32 fields: the reference's bits wherever it is not a NaN, a NaN (of any sign and payload: those of a generated
    NaN differ between x86 and the GPU) where it is one -> the indices that break the rule."""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(w)
    return np.flatnonzero(np.where(nan, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32)))
