// tw_rollout.hip -- fused PPO rollout kernel for gfx950 (MI355X), f32 "exact" arithmetic.
//
// Replaces the hot loop of PPOCollector::single_collect (reference rust/src/collector/ppo.rs:
// 54-80): per record observe + masks + reward (envs/puzzle.rs:162-185), Policy::forward_with_perm
// (nn/policy.rs:56-100: twist, EmbeddingBag, common Linear+ReLU, value/action heads, act-perm,
// -1e10 mask), sample_from_logits (policy.rs:169-172) and Env::step (puzzle.rs:135-160).
//
// Mapping to CDNA4
//   * one workgroup = 8 waves (2 per SIMD) = 256 episodes, resident for the WHOLE episode: no
//     inter-workgroup communication (episodes are independent, ppo.rs:59).  Board state lives in
//     registers as 16 packed nibbles; both lanes (j, j+32) of an MFMA column hold the same episode.
//   * the network is evaluated TRANSPOSED: h1^T[hidden x 32 episodes] = W1^T . h0^T on
//     v_mfma_f32_32x32x2_f32, episode = MFMA column = lane&31.  The B operand of k-step s is ONE
//     f32 per lane: h0[episode][2s + (lane>>5)], which the lane computes itself as the EmbeddingBag
//     gather-sum (bias + sum over cells of table[id][k], in cell order) from a 16-column chunk of
//     the table held in LDS.  The chunk image is column-permuted ([even k | odd k]) so the four
//     k-steps a lane handles next sit in ONE 16-byte word: one ds_read_b128 per cell feeds four add
//     chains.  Row stride 20 floats: (16i+tile)*20 mod 64 takes 16 distinct 16-byte bank slots for
//     the 16 tiles of a cell (conflict-free; equal tiles broadcast).
//   * an f32 MFMA chain IS a k-ordered fmaf chain, so the result is bit-equal to the oracle's
//     TWO_ARITH_CHAIN forward; rows of W1 are fed in an order (hid()) that makes the accumulator
//     registers come out in natural hidden order for the head product.
//   * both weight streams are pure LDS-DMA (global_load_lds_dwordx4 via inline asm) into a ring of
//     three slots, two chunks ahead, spread between the MFMAs; the inner loop is software-pipelined
//     by hand across chunk boundaries (issue order pinned with sched_barrier, chunk body branch-free),
//     so nothing but the barrier itself sits between the last MFMA of a chunk and the first of the next.
//   * heads: [4 logits + value] x hidden as v_fma_f32 chains in hidden order over v_permlane32_swap'd accumulators
//     (tw_engine.hpp; the dependent-MFMA form cost 6 % of the matrix-pipe time for 1 % of the FLOPs).
//   * the f32-input MFMA executes on the SIMD's f32 FMA lanes, so the gather's VALU adds do NOT overlap
//     it: the practical ceiling is MFMA cycles + add cycles (~0.85 of the MFMA-only peak).
#include "tw_engine.hpp"

#include <cstdlib>
#include <cstring>

namespace tw {

// scrambled start boards of episodes [offset, offset+n) (Env::reset, puzzle.rs:119-133) for the persistent-lane mode
__global__ void __launch_bounds__(256) init_boards_kernel(const PuzzleConsts env, uint64_t seed, uint64_t episode_offset, uint64_t n, uint64_t *out, uint4 *entries)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    PuzzleLane st;
    puzzle_reset(st, env, seed, episode_offset + i);
    if (out) out[i] = st.board;
    if (entries) entries[i] = make_uint4((uint32_t)st.board, (uint32_t)(st.board >> 32), (uint32_t)i, 0u);
}

int launch_init_boards(const PuzzleConsts &env, uint64_t seed, uint64_t episode_offset, uint64_t n, uint64_t *out, hipStream_t s, uint4 *entries)
{
    if (n == 0) return TW_OK;
    hipLaunchKernelGGL(init_boards_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, env, seed, episode_offset, n, out, entries);
    TW_HIP(hipGetLastError());
    return TW_OK;
}

// Longest-first order for the self-play episode queue.  A collect is as long as its longest episode's chain of searches plus
// the time that episode waited for a walker; episodes that are not solved run to the depth limit (17 moves against a mean of 5 at
// difficulty 8), and the boards far from the solved one are the ones that are not solved.  Key = sum over the tiles of the Manhattan
// distance to their place (a lower bound of the moves needed), counting sort by decreasing key (below), ~0.1 ms for 262,144 episodes.
// Which walker runs which episode never changes a bit of the result (every episode is keyed by its own global index).
__device__ __forceinline__ bool rank_is_leader(unsigned long long peers, int lane) { return (peers & ((1ull << lane) - 1ull)) == 0ull; }

// A STABLE counting sort by decreasing key (equal keys stay in index order: the schedule, and with it the collect's time, is the same
// every run), in three small launches so that a quarter of a million episodes cost ~0.1 ms, not 1.8: the indices are cut into segments
// of ORD_SPAN (one wave each, 16 per workgroup); (1) every wave counts its segment's keys, (2) one workgroup turns the counts into every
// segment's first output position per key -- all larger keys first, then the segments in index order --, (3) every wave scatters its
// segment in order from those cursors.
constexpr uint32_t ORD_WAVES = 16;
struct OrdKey {
    uint64_t lutx, luty; int n_cells, width;
    __device__ explicit OrdKey(const PuzzleConsts &env) : lutx(0), luty(0), n_cells(env.n_cells), width(env.width)
    {
        for (int i = 0; i < env.n_cells; ++i) {                 // place of tile v in the solved board, one nibble each
            const uint64_t v = nib(env.ident, i);
            lutx |= (uint64_t)(i % env.width) << (4 * v); luty |= (uint64_t)(i / env.width) << (4 * v);
        }
    }
    __device__ uint32_t operator()(uint64_t b) const
    {
        int d = 0;
        for (int i = 0; i < n_cells; ++i) {
            const uint64_t v = nib(b, i);
            if (v == 0) continue;                               // the blank
            const int dx = i % width - (int)((lutx >> (4 * v)) & 15), dy = i / width - (int)((luty >> (4 * v)) & 15);
            d += (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        }
        return (uint32_t)(d < 63 ? d : 63);
    }
};

__global__ void __launch_bounds__(1024) episode_order_count_kernel(const PuzzleConsts env, const uint64_t *boards, uint32_t n, uint32_t span, uint32_t *cnt)
{
    __shared__ uint32_t c[ORD_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < (int)ORD_WAVES * 64; i += 1024) (&c[0][0])[i] = 0;
    const OrdKey key(env);
    const uint32_t seg = blockIdx.x * ORD_WAVES + (uint32_t)wave;
    const uint64_t lo64 = (uint64_t)seg * span;
    const uint32_t lo = lo64 < n ? (uint32_t)lo64 : n, hi = lo64 + span < n ? (uint32_t)(lo64 + span) : n;
    __syncthreads();
    for (uint32_t i = lo + lane; i < hi; i += 64) atomicAdd(&c[wave][key(boards[i])], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < (int)ORD_WAVES * 64; i += 1024) cnt[(size_t)blockIdx.x * ORD_WAVES * 64 + i] = (&c[0][0])[i];
}

__global__ void __launch_bounds__(64) episode_order_prefix_kernel(uint32_t *cnt, uint32_t n_seg)      // cnt[seg][key] -> first output position
{
    __shared__ uint32_t total[64];
    const int k = threadIdx.x;
    uint32_t t = 0;
    for (uint32_t sgm = 0; sgm < n_seg; ++sgm) t += cnt[(size_t)sgm * 64 + k];
    total[k] = t;
    __syncthreads();
    uint32_t pos = 0;
    for (int kk = 63; kk > k; --kk) pos += total[kk];
    for (uint32_t sgm = 0; sgm < n_seg; ++sgm) { const uint32_t c = cnt[(size_t)sgm * 64 + k]; cnt[(size_t)sgm * 64 + k] = pos; pos += c; }
}

__global__ void __launch_bounds__(1024) episode_order_scatter_kernel(const PuzzleConsts env, const uint64_t *boards, uint32_t n, uint32_t span, const uint32_t *base,
                                                                      uint32_t *order, uint4 *entries)
{
    __shared__ uint32_t cur[ORD_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < (int)ORD_WAVES * 64; i += 1024) (&cur[0][0])[i] = base[(size_t)blockIdx.x * ORD_WAVES * 64 + i];
    const OrdKey key(env);
    const uint32_t seg = blockIdx.x * ORD_WAVES + (uint32_t)wave;
    const uint64_t lo64 = (uint64_t)seg * span;
    const uint32_t lo = lo64 < n ? (uint32_t)lo64 : n, hi = lo64 + span < n ? (uint32_t)(lo64 + span) : n;
    __syncthreads();
    for (uint32_t i0 = lo; i0 < hi; i0 += 64) {                 // (wave-uniform trip count)
        const uint32_t i = i0 + lane;
        const bool on = i < hi;
        const uint64_t bd = on ? boards[i] : 0ull;
        const uint32_t k = on ? key(bd) : 64u;
        unsigned long long peers = __builtin_amdgcn_ballot_w64(on);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(on && ((k >> b) & 1u));
            peers &= ((k >> b) & 1u) ? m : ~m;
        }
        if (on) {
            const uint32_t rank = (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
            const uint32_t pos = cur[wave][k] + rank;
            if (order) order[pos] = i;
            if (entries) entries[pos] = make_uint4((uint32_t)bd, (uint32_t)(bd >> 32), i, 0u);
        }
        __builtin_amdgcn_wave_barrier();
        if (on && rank_is_leader(peers, lane)) cur[wave][k] += (uint32_t)__builtin_popcountll(peers);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// segments of at least 1,024 indices, at most 64 workgroups
static void episode_order_shape(uint64_t n, uint32_t *span, uint32_t *blocks)
{
    uint64_t sp = 1024;
    while ((n + sp * ORD_WAVES - 1) / (sp * ORD_WAVES) > 64) sp *= 2;
    *span = (uint32_t)sp;
    *blocks = (uint32_t)((n + sp * ORD_WAVES - 1) / (sp * ORD_WAVES));
}
size_t episode_order_scratch_bytes(uint64_t n)
{
    uint32_t span, blocks; episode_order_shape(n, &span, &blocks);
    return (size_t)blocks * ORD_WAVES * 64 * sizeof(uint32_t);
}

int launch_episode_order(const PuzzleConsts &env, const uint64_t *boards, uint64_t n, uint32_t *order, void *scratch, hipStream_t s, uint4 *entries)
{
    if (n == 0) return TW_OK;
    if (n > 0xffffffffull || env.n_cells < 1 || env.n_cells > 16 || !scratch) { set_error("episode order: unsupported shape"); return TW_ERR_INVALID; }
    uint32_t span, blocks; episode_order_shape(n, &span, &blocks);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch);
    hipLaunchKernelGGL(episode_order_count_kernel, dim3(blocks), dim3(1024), 0, s, env, boards, (uint32_t)n, span, cnt);
    hipLaunchKernelGGL(episode_order_prefix_kernel, dim3(1), dim3(64), 0, s, cnt, blocks * ORD_WAVES);
    hipLaunchKernelGGL(episode_order_scatter_kernel, dim3(blocks), dim3(1024), 0, s, env, boards, (uint32_t)n, span, (const uint32_t *)cnt, order, entries);
    TW_HIP(hipGetLastError());
    return TW_OK;
}

TW_STAMP_ARRAY(g_gen_stamps, 8);   // cycle stamps of the generic engine and the 32- and 16-episode shapes (tw_common.hpp)

// The tail of one step, shared by the forwarded step (RAW: `lg` comes out of the forward) and the fast-forward rounds of the
// 256-episode shape (`lg` and `value` come out of the episode's look-back ring: act-permuted and masked already): reward,
// Gumbel arg-max, the record, is_final / step, and in persistent mode the next episode off the queue.  `on`: this lane takes the
// step (the forwarded step: every lane; a round: the lanes that hit).
// entries of RolloutArgs::init_boards: the drain launch of a hand-over (the <NT, NC, -4, true> shape) reads the count the first launch left
// The launch arguments as they sit in the kernarg segment, through a pointer the compiler cannot see through.  The 256-episode shape
// reads every launch constant of the step's tail, of the rounds and of the loop top through such a view taken where it is needed:
// a constant read from the by-value argument is loaded once in front of the loop and then lives across the forward, which has no
// scalar register to spare -- it was parked in a lane of a spill VGPR and fetched back with a v_readlane_b32 (vector-ALU time: the
// f32 MFMA hides none of it) at every use.  A scalar load behind the forward costs the vector ALU nothing.
typedef const __attribute__((address_space(4))) RolloutArgs KernArgs;
__device__ __forceinline__ KernArgs &kernarg_view()
{
    KernArgs *p = (KernArgs *)__builtin_amdgcn_kernarg_segment_ptr();   // (the kernel's one by-value argument: offset 0)
    asm volatile("" : "+s"(p));
    return *p;
}
template <class Args>
__device__ __forceinline__ PuzzleConsts env_of(Args &a)
{
    PuzzleConsts e;
    e.width = a.env.width; e.height = a.env.height; e.n_cells = a.env.n_cells; e.difficulty = a.env.difficulty;
    e.depth0 = a.env.depth0; e.r_step = a.env.r_step; e.ident = a.env.ident;
    return e;
}

// Policy::get_perm_id of step t of an episode (policy.rs:67-77); n_perms > 0
template <class Args>
__device__ __forceinline__ int draw_twist(Args &a, int n_perms, uint32_t e_local, int t)
{
    const u32x4 w = rng_draw(a.seed, a.episode_offset + (uint64_t)e_local, (uint32_t)t, STREAM_PERM);
    return (int)u32_below(w.x, (uint32_t)n_perms);
}

// Look-back ring of the 256-episode shape: the last RING_SLOTS steps of every episode of the workgroup, in LDS behind
// the engine's image and the four counter words -- [slot][dword][episode] with the dwords board lo, hi | masked, act-permuted
// logits | value, then one dword per episode with the slots' four twist bytes (perm & 0xff: 0xff without twists).  Step t sits in
// slot t & 3.  Only the episode's writer lane stores; both lanes of the episode (j and j + 32 of one wave, whose LDS operations
// execute in program order) read, so no barrier is involved.
// Why a slot never answers for another step than the one asked for: a lane clears its episode's four twist bytes to RING_EMPTY
// (byte 0xfd, which is no key: a twist index is below 128, "no twist" is 0xff, "twist not drawn yet" is 0xfe) before the kernel's
// first step and whenever it takes a new episode off the queue, and it stores step t of an episode before it looks anything up at
// a later step.  So the slots of t-2 and t-4 hold those very steps once this lane has run them, and RING_EMPTY before (t < 2,
// t < 4, the steps a previous episode left there): the twist byte of such a slot equals no key, whatever its board words are
// (unwritten LDS included).  A step whose twist is not drawn yet (the first one of an episode taken inside the rounds, key byte
// 0xfe) equals no stored byte either.
constexpr int      RING_SLOTS = 4, RING_DW = 7, RING_EPS = 8 * EPW;
constexpr int      RING_AT    = 4;                                           // in dwords behind the engine's image: the counter words first
constexpr size_t   RING_BYTES = (size_t)(RING_SLOTS * RING_DW + 1) * RING_EPS * 4;
constexpr unsigned RING_EMPTY = 0xfdfdfdfdu;
constexpr int      PERM_UNDRAWN = -2;                                        // (key byte 0xfe: no stored byte, so such a step never hits)
static_assert(RING_BYTES == 116 * 256, "look-back ring: 116 bytes per episode");
static_assert((engine3_lds_floats<8>(256) + RING_AT) * 4 + RING_BYTES <= 159 * 1024, "the look-back ring must fit behind the largest engine image (launch_geom checks every launch)");

// (`ring`: the lane's own view, the ring's first dword + the episode's index inside the workgroup)
__device__ __forceinline__ void ring_clear(unsigned *ring) { ring[RING_SLOTS * RING_DW * RING_EPS] = RING_EMPTY; }
__device__ __forceinline__ void ring_put(unsigned *ring, int t, uint64_t board, int perm, const float (&lg)[4], float value)
{
    unsigned *e = ring + (t & (RING_SLOTS - 1)) * (RING_DW * RING_EPS);
    e[0] = (uint32_t)board; e[RING_EPS] = (uint32_t)(board >> 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) e[(2 + i) * RING_EPS] = __float_as_uint(lg[i]);
    e[6 * RING_EPS] = __float_as_uint(value);
    reinterpret_cast<uint8_t *>(ring + RING_SLOTS * RING_DW * RING_EPS)[t & (RING_SLOTS - 1)] = (uint8_t)(perm & 0xff);
}

template <int NW, class Args>
__device__ __forceinline__ uint64_t queue_entries(Args &a)
{
    if constexpr (NW == -4) { if (a.num_episodes_dev) return (uint64_t)*a.num_episodes_dev; }
    return a.num_episodes;
}

// 256-episode shape (NW == 8): `perm` comes in as the twist of this step and goes out as the twist of the lane's pending step
// (PERM_UNDRAWN where that is the first step of a new episode), and
// the step's (board, twist) -> (logits, value) goes into the look-back ring (`ring`: the lane's view of it, below).
template <int NW, bool PERSIST, bool RAW, class Eng, class Args>
__device__ __forceinline__ void step_tail(Args &a, const PuzzleConsts &env, const Eng &eng, bool writer, bool on, int &perm, float (&lg)[4], float value,
                                          uint32_t &e_local, uint64_t &board, int &depth, int &t, bool &alive, bool &more, unsigned *wg_words = nullptr, unsigned *ring = nullptr)
{
    const int j = eng.j, h = eng.h;
    PuzzleLane st; st.board = board; st.depth = depth;
    { const int z = blank_cell(board); st.zx = z % env.width; st.zy = z / env.width; }
    if constexpr (RAW) {
        eng.act_perm(perm, lg);
        const uint32_t mb = puzzle_maskbits(st, env);
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[i] = ((mb >> i) & 1u) ? lg[i] : -1e10f;   // policy.rs:62
    }
    const float rew = puzzle_reward(st, env);
    int action, perm_next = perm;
    if constexpr (NW == 8) {
        // Lanes j and j+32 carry one episode, so ONE Philox pass serves both draws the step needs: the lower half runs it for
        // (episode, t, Gumbel), the upper half the same instructions for (episode, t + 1, twist) -- integer arithmetic, the same
        // bits whichever lane computes a word.  swap(x, z): the first result holds the lower half's x (lower lanes) and z (upper
        // lanes), the uniforms gumbel_argmax4_words transforms there; the second one hands the upper half's x, the twist word,
        // to the lower lanes.
        const u32x4 w = rng_draw(a.seed, a.episode_offset + (uint64_t)e_local, (uint32_t)(t + h), h ? STREAM_PERM : STREAM_GUMBEL);
        const auto s0 = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
        action = gumbel_argmax4_words(lg, s0[0], s1[0], h != 0);
        const int n_perms = a.pol.n_perms;
        if (n_perms > 0) perm_next = (int)u32_below(h ? w.x : s0[1], (uint32_t)n_perms);
    } else {
        const u32x4 gw = rng_draw(a.seed, a.episode_offset + (uint64_t)e_local, (uint32_t)t, STREAM_GUMBEL);
        action = gumbel_argmax4(lg, gw);
    }
    // ---- push the record (ppo.rs:71-76), then is_final / step (ppo.rs:78-79) --------------
    if (alive && on) {
        if (writer) {
            const uint64_t rec = (uint64_t)e_local * (uint64_t)a.out.t_pad + (uint64_t)t;
            uint32_t obs_base[4], pk[4];
            obs_base_words(env.n_cells, obs_base);
            obs_bytes(board, obs_base, pk);
            store_rec(a.out.rec + rec, pk, lg, value, rew, action, perm);
            if constexpr (NW == 8) ring_put(ring, t, board, perm, lg, value);
        }
        if (puzzle_final(st, env)) {
            alive = false;
            if constexpr (PERSIST) { if (writer) a.out.ep_len[e_local] = (uint32_t)t + 1u; }
        } else { puzzle_step(st, env, action); board = st.board; depth = st.depth; ++t; perm = perm_next; }
    }
    if constexpr (PERSIST) {
        const bool want = on && !alive && more;       // take the next episode off the queue (every lane of the episode the same one)
        unsigned got = 0xffffffffu;
        if (want && writer) got = atomicAdd(a.queue, 1u);
        if constexpr (Eng::SPLIT) {                   // all waves of the workgroup carry this episode: hand the index round in LDS
            unsigned *bc = reinterpret_cast<unsigned *>(eng.lds_user);
            if (writer) bc[j] = got;
            __syncthreads();
            got = bc[j];
        } else got = (unsigned)__shfl((int)got, j, 64);
        if (want) {
            if ((uint64_t)got < queue_entries<NW>(a)) {
                const uint4 ib = a.init_boards[got];          // (w: the step the episode is at -- 0, or where a hand-over left it)
                e_local = ib.z; board = ((uint64_t)ib.y << 32) | ib.x; t = (int)ib.w;
                depth = env.depth0 > t ? env.depth0 - t : 0;
                alive = true;
                if constexpr (NW == 8) { if (writer) ring_clear(ring); }
            } else {
                more = false;
                if constexpr (NW == 8) { if (writer) wg_words[1] = 1u; }     // the queue never refills: from here on the workgroup only drains
            }
        }
        // a lane that took a new episode: its pending step is not (episode, t + 1) -- the loop top draws that twist
        if constexpr (NW == 8) perm = want && alive && a.pol.n_perms > 0 ? PERM_UNDRAWN : perm;
    }
}

// Fast-forward rounds of the 256-episode shape: after a forwarded step every wave on its own takes up to REUSE_R
// further steps whose output the episode's look-back ring holds from 2, 4, .. 2 * REUSE_LB steps ago (same board, same twist).
#ifndef TW_REUSE_LB        // (-DTW_REUSE_LB / -DTW_REUSE_R with TW_VARIANT: the pairs measured in profiles/r10_rollout_reuse.txt)
#define TW_REUSE_LB 2
#endif
#ifndef TW_REUSE_R
#define TW_REUSE_R 2
#endif
constexpr int REUSE_LB = TW_REUSE_LB, REUSE_R = TW_REUSE_R;

// -DTW_DRAIN_ANATOMY (a TW_VARIANT build; TW_STAMPS=1 prints): per workgroup of the persistent 256-episode shape, the iteration at
// which the queue was dry, at which 128 / 64 / 32 or fewer episodes lived, and the last one (profiles/r14_rollout_drain.txt).
// Thread 0 alone keeps the iteration count and the events seen in the two spare LDS words behind the reuse counter.
#ifdef TW_DRAIN_ANATOMY
__device__ unsigned g_drain_anat[1024 * 8];
#define TW_DRAIN_ANATOMY_INIT(w) do { (w)[2] = 0u; (w)[3] = 0u; } while (0)
#define TW_DRAIN_ANATOMY_STEP(w, live, wg)                                                                              \
    do {                                                                                                                \
        if (threadIdx.x == 0 && (wg) < 1024u) {                                                                         \
            const unsigned it_ = (w)[2]++; unsigned seen_ = (w)[3]; unsigned *o_ = g_drain_anat + 8u * (wg);            \
            if (!(seen_ & 1u) && (w)[1]) { o_[0] = it_; seen_ |= 1u; }                                                  \
            if (!(seen_ & 2u) && (live) <= 128u) { o_[1] = it_; seen_ |= 2u; }                                          \
            if (!(seen_ & 4u) && (live) <= 64u) { o_[2] = it_; seen_ |= 4u; }                                           \
            if (!(seen_ & 8u) && (live) <= 32u) { o_[3] = it_; seen_ |= 8u; }                                           \
            o_[4] = it_; o_[5] = (live);                                                                                \
            (w)[3] = seen_;                                                                                             \
        }                                                                                                               \
    } while (0)
#else
#define TW_DRAIN_ANATOMY_INIT(w) do {} while (0)
#define TW_DRAIN_ANATOMY_STEP(w, live, wg) do {} while (0)
#endif

// -DTW_STEP_ANATOMY (with -DTW_ABLATE, a TW_VARIANT build; TW_STAMPS=1 prints): where wave 0 of every workgroup of the 256-episode
// shape spends an iteration of the step loop -- observe + forward | forwarded tail | rounds, of which the wait for the look-back
// entries | the rest: the loop-top barrier (profiles/r15_rollout_lookback.txt).  No other build holds any of it.
#if defined(TW_STEP_ANATOMY) && defined(TW_ABLATE)
TW_STAMP_ARRAY(g_step_stamps, 8);
#define TW_STEP_VARS(...)          unsigned long long __VA_ARGS__
#define TW_STEP_STAMP(t)           TW_RESTAMP(t)
#define TW_STEP_ADD(acc, t0, t1)   TW_STAMP_ADD(acc, t0, t1)
#define TW_STEP_USE(x)             TW_STAMP_USE(x)
constexpr bool STEP_ANATOMY = true;
#else
#define TW_STEP_VARS(...)          static_assert(true, "")
#define TW_STEP_STAMP(t)           do {} while (0)
#define TW_STEP_ADD(acc, t0, t1)   do {} while (0)
#define TW_STEP_USE(x)             do {} while (0)
constexpr bool STEP_ANATOMY = false;
#endif

// (the generic engine's workgroups are small -- 256 threads, exact-size activation buffers: two of them share a CU, and while one
//  gathers its embeddings from L2 the other one keeps the matrix cores busy)
template <int NT, int NC, int NW = 8, bool PERSIST = false>
__global__ void __launch_bounds__((Geom<NT, NC, NW>::WAVES * 64), ((NW == 8 || NW == -65) ? 2 : 1)) rollout_f32_kernel(const RolloutArgs a)
{
    using Eng = typename Geom<NT, NC, NW>::Eng;       // NW < 0: -NW waves share 32 episodes (Engine3S); all carry the same state
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
    eng.begin1(a.pol, lds);                               // first weight chunks stream in while the scramble runs

    const PuzzleConsts env = a.env;
    const int h = eng.h;
    // Loop-carried per-episode state is kept to five registers (board, depth, episode, t): everything derivable (blank position,
    // global episode index, record address, obs-id constants) is recomputed after the forward -- held across it, those were the
    // registers the 8-wave x 256-accumulator shape spilled to scratch.
    const uint64_t e_first = (uint64_t)blockIdx.x * Eng::EPB + (uint64_t)eng.ep_lane();
    const bool valid  = e_first < (PERSIST ? queue_entries<NW>(a) : a.num_episodes);
    const bool writer = h == 0 && eng.primary();          // the lane that stores the episode's records
    uint32_t e_local = (uint32_t)e_first;                 // (launch_geom bounds the episode count of a launch to 2^31)
    uint64_t board = env.ident; int depth = 0;
    int      t = 0;                                       // (stays at the last record once the episode is over: records = t + 1)
    if (valid) {
        if constexpr (PERSIST) {              // the episode and its start board from the pre-pass (RolloutArgs::init_boards: in the order the lanes take them)
            const uint4 ib = a.init_boards[e_local];
            e_local = ib.z; board = ((uint64_t)ib.y << 32) | ib.x; t = (int)ib.w;
            depth = env.depth0 > t ? env.depth0 - t : 0;
        }
        else { PuzzleLane s0; puzzle_reset(s0, env, a.seed, a.episode_offset + e_first); board = s0.board; depth = s0.depth; }
    }

    bool     alive = valid;
    bool     more  = PERSIST;                             // the queue may still hold episodes

    eng.begin2();
    // (the barrier inside __syncthreads_or publishes the first two ring slots and the LDS constants)
    TW_STAMP(q_loop);
    TW_STAMP_VARS(n_fwd = 0);
    // records taken from the trajectory: counted in one LDS word behind the engine's image (launch_geom adds it) -- a counter
    // in a register would be live across the forward, which has none to spare
    // ([1]: "the queue is dry", set by whichever lane finds it so in step_tail)
    unsigned *reuse_cnt = nullptr;
    // (behind the four words: the look-back ring, every writer lane its own episode's part)
    int perm = -1;                                        // 256-episode shape: the twist of the lane's pending step, handed on by step_tail
    if constexpr (NW == 8) {
        reuse_cnt = reinterpret_cast<unsigned *>(lds + Eng::lds_floats(a.pol));
        if (threadIdx.x == 0) { reuse_cnt[0] = 0u; reuse_cnt[1] = 0u; TW_DRAIN_ANATOMY_INIT(reuse_cnt); }
        if (writer) ring_clear(reuse_cnt + RING_AT + eng.ep_lane());
        if (eng.pol.n_perms > 0) perm = PERSIST ? PERM_UNDRAWN : draw_twist(a, eng.pol.n_perms, e_local, t);
    }

    // The loop runs while an episode of the workgroup lives.  Persistent 256-episode shape: the same barrier counts them, and once
    // the queue is dry and no more than drain_live are left the workgroup hands them over instead of running 256-column forwards
    // for a handful of columns (RolloutArgs::resume; the flag was stored before this barrier, and the next store to it lies behind
    // the forward's barriers).  Exit plus stream order: nothing waits.
    // (256-episode shape: the launch constants inside the loop come through kernarg_view(), taken anew on either side of the forward)
    auto args = [&]() -> decltype(auto) { if constexpr (NW == 8) return kernarg_view(); else return (a); };
    auto env_at = [&](auto &v) -> decltype(auto) { if constexpr (NW == 8) return env_of(v); else return (env); };
    auto go_on = [&]() -> bool {
        if constexpr (NW == 8 && PERSIST) {
            const unsigned live = (unsigned)__syncthreads_count(alive && writer ? 1 : 0);
            TW_DRAIN_ANATOMY_STEP(reuse_cnt, live, blockIdx.x);
            if (live == 0u) return false;
            // (every lane reads the same word: the first lane's copy makes the test a scalar one and this exit of the loop wave-uniform --
            //  as a vector compare it sent the exit through a divergent region whose lane masks then lived across the forward)
            if (live > args().drain_live || !__builtin_amdgcn_readfirstlane(*(volatile unsigned *)(reuse_cnt + 1))) return true;
            if (alive && writer) {
                auto &ha = args();
                ha.resume[atomicAdd(ha.resume_cnt, 1u)] = make_uint4((uint32_t)board, (uint32_t)(board >> 32), e_local, (uint32_t)t);
            }
            return false;
        } else return __syncthreads_or(alive ? 1 : 0) != 0;
    };
    TW_STEP_VARS(sq0 = 0, sq1 = 0, sq2 = 0, s_fwd = 0, s_tail = 0, s_rounds = 0, s_wait = 0, s_iter = 0);
    while (go_on()) {
        TW_STAMP_COUNT(n_fwd, 1);
        TW_STEP_STAMP(sq0);
        // ---- observe (puzzle.rs:183-185) + twist of the obs ids (policy.rs:67-83) -------------
        auto &la = args();
        if constexpr (NW == 8) {
            // step_tail left the twist of the pending step with the step before it; only a lane whose pending step is an episode's
            // first one has none yet (persistent lanes: the first iteration, a lane that took an episode off the queue; the plain
            // launch drew it in front of the loop): one more pass, wave-uniform
            if constexpr (PERSIST) {
                if (__builtin_amdgcn_ballot_w64(perm == PERM_UNDRAWN) != 0ull) {
                    const int p = draw_twist(la, la.pol.n_perms, e_local, t);
                    perm = perm == PERM_UNDRAWN ? p : perm;
                }
            }
        } else {
            perm = -1;
            if (eng.pol.n_perms > 0) perm = draw_twist(a, eng.pol.n_perms, e_local, t);
        }
        int rowoff[NC];
        if constexpr (NW == 8) eng.rows_of_args(la, board, perm, rowoff);
        else eng.rows_of(board, env.n_cells, perm, rowoff);

        float lg[4]; float value;
        if constexpr (NW == 8) eng.template forward<true>(rowoff, lg, value);
        else eng.forward(rowoff, lg, value);
        TW_STEP_USE(value); TW_STEP_STAMP(sq1); TW_STEP_ADD(s_fwd, sq0, sq1);

        // the lane's view of the look-back ring, computed behind the forward (through an opaque copy of the lane's column: an address
        // hoisted out of the loop would be one more register live across the forward)
        unsigned *ring = nullptr;
        if constexpr (NW == 8) { int jj = eng.j; asm volatile("" : "+v"(jj)); ring = reuse_cnt + RING_AT + eng.wave * EPW + jj; }
        auto &ta = args();
        const PuzzleConsts &tenv = env_at(ta);
        step_tail<NW, PERSIST, true>(ta, tenv, eng, writer, true, perm, lg, value, e_local, board, depth, t, alive, more, reuse_cnt, ring);
        TW_STEP_USE(t); TW_STEP_USE(perm); TW_STEP_STAMP(sq2); TW_STEP_ADD(s_tail, sq1, sq2); TW_STEP_ADD(s_iter, 0, 1);

        // ---- fast-forward rounds: a step whose (board, perm) the episode recorded 2k steps ago takes that record's output -----
        if constexpr (NW == 8) {
            if (!ta.reuse_off) {
                static_assert(2 * REUSE_LB <= RING_SLOTS, "the look-back ring holds the last RING_SLOTS steps");
                bool cand = true;                         // a lane that missed stays where it is: it would miss again
#pragma unroll 1
                for (int r = 0; r < REUSE_R; ++r) {
                    TW_STEP_STAMP(sq0);
                    // the pending step's key against the ring's entries of t-2 and t-4 (both lanes of the episode the same reads)
                    const uint32_t tws = ring[RING_SLOTS * RING_DW * RING_EPS];
                    bool hit = false; int hs = 0;
#pragma unroll
                    for (int k = REUSE_LB; k >= 1; --k) {             // (the nearer step last: it wins, though any match holds the same bits)
                        const int sl = (t - 2 * k) & (RING_SLOTS - 1);
                        const unsigned *e = ring + sl * (RING_DW * RING_EPS);
                        const uint32_t blo = e[0], bhi = e[RING_EPS];
                        if (blo == (uint32_t)board && bhi == (uint32_t)(board >> 32) && ((tws >> (8 * sl)) & 0xffu) == (uint32_t)(perm & 0xff)) { hit = true; hs = sl; }
                    }
                    hit = hit && cand && alive;
                    TW_STEP_USE(hit ? 1 : 0); TW_STEP_STAMP(sq1); TW_STEP_ADD(s_wait, sq0, sq1);
                    const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
                    if (hm == 0ull) break;
                    if (hit && writer) atomicAdd(reuse_cnt, 1u);
                    cand = hit;
                    const unsigned *e = ring + hs * (RING_DW * RING_EPS);
#pragma unroll
                    for (int i = 0; i < 4; ++i) lg[i] = __uint_as_float(e[(2 + i) * RING_EPS]);
                    value = __uint_as_float(e[6 * RING_EPS]);
                    step_tail<NW, PERSIST, false>(ta, tenv, eng, writer, hit, perm, lg, value, e_local, board, depth, t, alive, more, reuse_cnt, ring);
                }
                TW_STEP_USE(t); TW_STEP_STAMP(sq1); TW_STEP_ADD(s_rounds, sq2, sq1);
            }
        }
    }
    if constexpr (NW == 8) {                              // (behind the loop's last barrier) whichever wave comes first takes the count
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u) {
            const unsigned n = atomicExch(reuse_cnt, 0u);
            if (n) atomicAdd(a.reused, n);
        }
    }
    if constexpr (!PERSIST) { if (valid && writer) a.out.ep_len[e_local] = (uint32_t)t + 1u; }
    eng.end();
    if constexpr (NW == 8 && STEP_ANATOMY) {              // wave 0: forward | tail | rounds | of those the look-back wait; iterations; cycles in the step loop
        TW_STEP_STAMP(sq1);
        TW_STAMP_FLUSH(eng.lane == 0 && eng.wave == 0, g_step_stamps, s_fwd, s_tail, s_rounds, s_wait, s_iter, sq1 - q_loop);
    }
    if constexpr (NW == -65)                              // waves 0 and 3: embed | common | value | action
        TW_STAMP_FLUSH(eng.lane == 0 && (eng.wave == 0 || eng.wave == 3), g_gen_stamps + (eng.wave ? 4 : 0), eng.stq[0], eng.stq[1], eng.stq[2], eng.stq[3]);
    if constexpr (NW == -16 || NW == -4) {                // wave 0: prologue | chunk loop | - | - | heads; forwards; cycles in the step loop
        TW_STAMP(q_end);
        TW_STAMP_FLUSH(eng.lane == 0 && eng.wave == 0, g_gen_stamps, eng.stq[0], eng.stq[1], eng.stq[2], eng.stq[3], eng.stq[4], n_fwd, q_end - q_loop);
    }
}

// persistent mode: one 256-episode workgroup per CU of the current device (256 on an MI355X; every rollout kernel needs
// most of a CU's LDS, so one workgroup is resident per CU)
static uint64_t persist_blocks(int reserve_cus)
{
    const int cus = device_cus();
    const int r = reserve_cus < 0 ? 0 : (reserve_cus > cus - 1 ? cus - 1 : reserve_cus);   // reserve_cus CUs stay free (RCCL beside the persistent grid)
    return (uint64_t)(cus - r);
}

uint64_t rollout_f32_resident_episodes(int reserve_cus) { return persist_blocks(reserve_cus) * 8 * EPW; }

// generic policy stacks (EngineV): workgroups of 16 episodes, as many per CU as their LDS allows (at most two: the registers)
static uint64_t generic_groups_per_cu(const PolicyDev &pol, int n_cells)
{
    const size_t lds_bytes = (n_cells <= 4 ? EngineV<4>::lds_floats(pol) : (n_cells <= 9 ? EngineV<9>::lds_floats(pol) : EngineV<16>::lds_floats(pol))) * sizeof(float);
    return lds_bytes * 2 <= 159 * 1024 ? 2 : 1;
}
uint64_t rollout_generic_resident_episodes(const PolicyDev &pol, int n_cells, int reserve_cus) { return persist_blocks(reserve_cus) * generic_groups_per_cu(pol, n_cells) * 16; }

// Episodes are ragged (a solved puzzle ends its episode), and a lane whose episode is over can only be refilled when there
// are more episodes than lanes.  Between CUs x 32 episodes and 3/4 of CUs x 256 the small-batch shape with the episode
// queue (CUs x 32 lanes, every one busy until the queue is empty) beats both running the 32-episode workgroups one after
// the other and leaving most of the lanes of the 256-episode shape idle behind the longest episodes (self-play, 32,768
// episodes: 1.8x); from there on the 256-episode shape wins.
// Upper end of that range: where the 256-episode shape overtakes with episodes of equal length (the rollout crossover of
// waves_per_group()); self-play episodes are always ragged, there the range extends to 3/4 of CUs x 256.
uint64_t f32_resident_episodes(uint64_t num_episodes, int hidden, bool selfplay, int reserve_cus)
{
    const uint64_t full = rollout_f32_resident_episodes(reserve_cus), small = full / 8;
    const bool in_range = selfplay ? num_episodes * 4 <= full * 3 : waves_per_group(num_episodes) != 8;
    if (hidden >= 128 && num_episodes > small && in_range && !launch_options().force_geom) {
        return small;
    }
    return full;
}

template <int NT, int NC, int NW = 8, bool PERSIST = false>
static int launch_geom(const RolloutArgs &a, hipStream_t s, uint32_t *blocks, uint32_t *threads)
{
    using G = Geom<NT, NC, NW>;
    constexpr int EPB = G::Eng::EPB, THREADS = 64 * G::WAVES;
    const uint64_t nb = PERSIST ? persist_blocks(a.reserve_cus) * (NW == -65 ? generic_groups_per_cu(a.pol, a.env.n_cells) : 1) : (a.num_episodes + EPB - 1) / EPB;
    if (nb == 0 || nb > 0x7fffffffull) { set_error("rollout: bad episode count %llu", (unsigned long long)a.num_episodes); return TW_ERR_INVALID; }
    const size_t lds_bytes = G::Eng::lds_floats(a.pol) * sizeof(float) + (NW == 8 ? RING_AT * 4 + RING_BYTES : 0);    // (+ the 256-episode shape's counter words and look-back ring)
    if (lds_bytes > 159 * 1024) { set_error("rollout: %zu bytes of LDS needed, 159 KiB available", lds_bytes); return TW_ERR_UNSUPPORTED; }
    if (NW == 8 && !a.reused && !a.reuse_off) { set_error("rollout: the 256-episode shape needs RolloutArgs::reused (or reuse_off)"); return TW_ERR_INVALID; }
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(&rollout_f32_kernel<NT, NC, NW, PERSIST>), lds_bytes)) return rc;
    constexpr bool STAMPED = NW == -65 || NW == -16 || NW == -4;      // the shapes that take cycle stamps
    if constexpr (STAMPED) TW_STAMPS_CLEAR(g_gen_stamps);
    if constexpr (NW == 8 && STEP_ANATOMY) TW_STAMPS_CLEAR(g_step_stamps);
    hipLaunchKernelGGL((rollout_f32_kernel<NT, NC, NW, PERSIST>), dim3((unsigned)nb), dim3(THREADS), lds_bytes, s, a);
    if constexpr (STAMPED) TW_STAMPS_REPORT(g_gen_stamps, s, g, {
        if (NW == -65)
            fprintf(stderr, "[generic engine stamps, cycles summed over %llu workgroups] wave0: embed %llu common %llu value %llu action %llu | wave3: %llu %llu %llu %llu\n",
                    (unsigned long long)nb, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7]);
        else
            fprintf(stderr, "[geometry %d, wave 0, cycles per forward] prologue %.0f chunk loop %.0f heads %.0f | whole step %.0f (%llu forwards)\n",
                    NW, (double)g[0] / g[5], (double)g[1] / g[5], (double)g[4] / g[5], (double)g[6] / g[5], g[5]);
    });
    if constexpr (NW == 8 && STEP_ANATOMY) TW_STAMPS_REPORT(g_step_stamps, s, g, {
        const double n = (double)g[4];
        fprintf(stderr, "[step anatomy, wave 0 of %llu workgroups, cycles per iteration] observe + forward %.0f | forwarded tail %.0f | rounds %.0f (look-back wait %.0f) | "
                        "barrier %.0f | whole %.0f (%.1f iterations per workgroup)\n", (unsigned long long)nb, g[0] / n, g[1] / n, g[2] / n, g[3] / n,
                ((double)g[5] - g[0] - g[1] - g[2]) / n, g[5] / n, n / (double)nb);
    });
    TW_HIP(hipGetLastError());
#ifdef TW_DRAIN_ANATOMY
    if constexpr (NW == 8 && PERSIST) {
        if (getenv("TW_STAMPS") && nb <= 1024) {
            static unsigned h[1024 * 8];
            TW_HIP(hipStreamSynchronize(s));
            TW_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_drain_anat), sizeof(h)));
            static const char *what[6] = {"queue dry", "live <= 128", "live <= 64", "live <= 32", "last", "live at last"};
            for (int k = 0; k < 6; ++k) {
                double sum = 0; unsigned lo = ~0u, hi = 0;
                for (uint64_t b = 0; b < nb; ++b) { const unsigned v = h[8 * b + k]; sum += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
                fprintf(stderr, "[drain anatomy, %llu workgroups, iteration] %-12s mean %.1f min %u max %u\n", (unsigned long long)nb, what[k], sum / (double)nb, lo, hi);
            }
        }
    }
#endif
    if (blocks) *blocks = (uint32_t)nb;
    if (threads) *threads = THREADS;
    return TW_OK;
}

// The launch of more than `resident` episodes is the persistent 256-episode shape, and the policy has the 32-episode shape the
// hand-over drains into (hidden >= 128).
bool rollout_f32_hands_over(const PolicyDev &pol, uint64_t resident, int reserve_cus)
{
    return !pol.generic && pol.hidden >= 128 && resident == rollout_f32_resident_episodes(reserve_cus);
}

template <int NT, int NC>
static int launch_one(const RolloutArgs &a, hipStream_t s, uint32_t *blocks, uint32_t *threads, uint32_t *drain_blocks)
{
    // small batches: fewer waves per workgroup, so that the episodes spread over more CUs
    const uint64_t resident = f32_resident_episodes(a.num_episodes, a.pol.hidden, false, a.reserve_cus);
    if (a.queue && a.init_boards && a.num_episodes > resident) {
        if constexpr (NT >= 4) {
            const uint64_t full = rollout_f32_resident_episodes(a.reserve_cus);
            if (resident < full) return launch_geom<NT, NC, -4, true>(a, s, blocks, threads);
        }
        if (a.drain_live && (NT < 4 || !a.resume || !a.resume_cnt || !a.drain_queue)) { set_error("rollout: hand-over without a drain shape or its workspace"); return TW_ERR_INVALID; }
        int rc = launch_geom<NT, NC, 8, true>(a, s, blocks, threads);
        if constexpr (NT >= 4) {
            // the drain: the 32-episode persistent shape over the episodes the workgroups above left in `resume`, right behind them on
            // the stream; how many there are it reads on the device (an empty list: every lane leaves at its first barrier)
            if (rc == TW_OK && a.drain_live) {
                RolloutArgs d = a;
                d.init_boards = a.resume; d.queue = a.drain_queue; d.num_episodes_dev = a.resume_cnt;
                d.num_episodes = rollout_f32_resident_episodes(a.reserve_cus);          // (the list's capacity)
                d.drain_live = 0; d.resume = nullptr; d.resume_cnt = nullptr; d.drain_queue = nullptr;
                rc = launch_geom<NT, NC, -4, true>(d, s, drain_blocks, nullptr);
            }
        }
        return rc;
    }
    const int nw = geometry_for<NT>(a.num_episodes);
    if constexpr (NT >= 4) { if (nw == -16) return launch_geom<NT, NC, -16>(a, s, blocks, threads); }
    if constexpr (NT >= 4) { if (nw == -4) return launch_geom<NT, NC, -4>(a, s, blocks, threads); }
    else if constexpr (NT == 2) { if (nw == -2) return launch_geom<NT, NC, -2>(a, s, blocks, threads); }
    else {
        if (nw == 1) return launch_geom<NT, NC, 1>(a, s, blocks, threads);
        if (nw == 2) return launch_geom<NT, NC, 2>(a, s, blocks, threads);
    }
    return launch_geom<NT, NC>(a, s, blocks, threads);
}

template <int NT>
static int launch_nt(const RolloutArgs &a, hipStream_t s, uint32_t *blocks, uint32_t *threads, uint32_t *drain_blocks)
{
    const int nc = a.env.n_cells;
    if (nc <= 4) return launch_one<NT, 4>(a, s, blocks, threads, drain_blocks);
    if (nc <= 9) return launch_one<NT, 9>(a, s, blocks, threads, drain_blocks);
    return launch_one<NT, 16>(a, s, blocks, threads, drain_blocks);
}

int launch_rollout_f32(const RolloutArgs &a, hipStream_t s, uint32_t *blocks, uint32_t *threads, uint32_t *drain_blocks)
{
    if (drain_blocks) *drain_blocks = 0;
    if (a.pol.generic) {          // any Sequential depth: the vector-ALU engine (tw_engine_generic.hpp); shapes validated by tw_policy_create
        if (a.env.n_cells < 1 || a.env.n_cells > 16 || a.pol.obs_size != a.env.n_cells * a.env.n_cells || a.pol.n_actions != 4 ||
            a.out.t_pad < a.env.depth0 + 1 || (a.queue == nullptr) != (a.init_boards == nullptr)) {
            set_error("rollout: unsupported shape for a generic policy (n_cells=%d obs_size=%d actions=%d)", a.env.n_cells, a.pol.obs_size, a.pol.n_actions);
            return TW_ERR_UNSUPPORTED;
        }
        const int nc = a.env.n_cells;
        if (a.queue) {            // more episodes than one 16-episode workgroup per CU: persistent lanes + episode queue
            if (nc <= 4) return launch_geom<0, 4, -65, true>(a, s, blocks, threads);
            if (nc <= 9) return launch_geom<0, 9, -65, true>(a, s, blocks, threads);
            return launch_geom<0, 16, -65, true>(a, s, blocks, threads);
        }
        if (nc <= 4) return launch_geom<0, 4, -65>(a, s, blocks, threads);
        if (nc <= 9) return launch_geom<0, 9, -65>(a, s, blocks, threads);
        return launch_geom<0, 16, -65>(a, s, blocks, threads);
    }
    // host-side shape checks: everything the kernel indexes with is validated here
    if (a.env.n_cells < 1 || a.env.n_cells > 16 || a.pol.obs_size != a.env.n_cells * a.env.n_cells ||
        a.pol.obs_size > 256 || a.pol.n_actions != 4 || a.pol.emb % 32 != 0 || a.pol.emb < 32 ||
        a.out.t_pad < a.env.depth0 + 1) {
        set_error("rollout: unsupported shape (n_cells=%d obs_size=%d actions=%d emb=%d hidden=%d t_pad=%d)",
                  a.env.n_cells, a.pol.obs_size, a.pol.n_actions, a.pol.emb, a.pol.hidden, a.out.t_pad);
        return TW_ERR_UNSUPPORTED;
    }
    switch (a.pol.hidden) {
        case 32:  return launch_nt<1>(a, s, blocks, threads, drain_blocks);
        case 64:  return launch_nt<2>(a, s, blocks, threads, drain_blocks);
        case 128: return launch_nt<4>(a, s, blocks, threads, drain_blocks);
        case 256: return launch_nt<8>(a, s, blocks, threads, drain_blocks);
        default:
            set_error("rollout: hidden size %d not in {32,64,128,256}", a.pol.hidden);
            return TW_ERR_UNSUPPORTED;
    }
}

}  // namespace tw
