// tw_rollout_env.hpp -- the fused PPO rollout and evaluate loop of tw_rollout_big.hip as templates over a user-written device
// environment (include/twisterl_device_env.hpp), and the argument structs a device-environment module shares with the library.
//
// A module (twisterl_amd.build.build_device_env) instantiates rollout_env_kernel<Env, NC> / solve_env_kernel<Env, NC> and their
// launchers through TW_DEVICE_ENV (TW_DEVICE_ENV_SEARCH / TW_DEVICE_ENV_WIDE_SEARCH: mcts_env_kernel<Env, NC> of tw_mcts_env.hpp as well); the library (tw_device_env.hip) owns everything around them: the checks, the workspace, the scan,
// GAE and compaction, the error messages, the hand-off to the host-stepped path for what the kernels do not take.  Per record, in the
// order of PPOCollector::single_collect (collector/ppo.rs:69-80): observe -> twist of the ids -> EngineV::forward -> act_perm -> mask
// -> reward -> Gumbel arg-max over the environment's actions; store the record and the ids, then is_final / step.  Same RNG keys and
// the same arithmetic as tw_ppo_collect_env / tw_evaluate_env over the environment's host vtable: bit-equal to them.  Both kernels have a
// persistent form behind a run-time branch on their argument struct's `queue` (fewer columns than episodes; a column whose episode is
// over takes the next one from a counter), which the library chooses from the kernel's own occupancy (tw_device_env::groups_per_cu).
// A module built with TW_DEVICE_ENV_FP16 also holds rollout_env16_kernel<Env, NC>: the rollout's loop over EngineV16
// (tw_engine_generic16.hpp), PPOCollector(precision="fp16"), within the a-priori bound of the f16-input spec instead of bit-equal.
// A module built with TW_DEVICE_ENV_FP16_SOLVE holds solve_env16_kernel<Env, NC> as well: evaluate's loop over EngineV16,
// collector.evaluate / collector.solve with precision="fp16" and no MCTS.  One built with TW_DEVICE_ENV_FP16_SEARCH beside a search form
// holds mcts_env16_kernel<Env, NC> (tw_mcts_env.hpp): self-play and MCTS-guided evaluate / solve with precision="fp16".
// A module built with TW_DEVICE_ENV_FP16X2 holds rollout_env16x2_kernel<Env, NC>: the rollout's loop over EngineV16x2
// (tw_engine_generic16x2.hpp), PPOCollector(precision="fp16x2"), f32 answers from split binary16 operands on the f16 matrix core.
// One built with TW_DEVICE_ENV_FP16X2_SOLVE holds solve_env16x2_kernel<Env, NC> as well (tw_solve_env16x2.hpp): evaluate's loop over
// EngineV16x2, collector.evaluate / collector.solve with precision="fp16x2" and no MCTS.
// A module built with TW_DEVICE_ENV_BASIC holds pack_basic_view_kernel (tw_env_basic_view.hpp): its f32 launchers then also take the
// reference's default policy -- one common layer, the "MFMA shape" -- as a view whose EngineV layers that kernel packs into the call's
// workspace in front of every launch; the kernels themselves are the ones above, unchanged.
//
// In this file: the argument structs and the descriptor; what the steps call (the Gumbel arg-max, the twist of the actions, the
// streaming steps of 5 .. 31 actions, env_rows / env_rows_n); the four kernels; their launchers and occupancy queries.  The two step
// loops are NOT here: tw_env_rollout_loop.hpp and tw_env_solve_loop.hpp hold the text of each once, and its f32 and f16 kernels
// include it inside their bodies.  A change to a step is made there, and reaches both kernels.
#pragma once
#include "tw_engine_generic.hpp"
#include "tw_engine_generic16.hpp"
#include "tw_engine_generic16x2.hpp"
#include "tw_env_basic_view.hpp"

#include <type_traits>
#include <utility>

namespace tw {

// What one launch of the rollout kernel needs besides the prototype (which travels by value as the kernel's second argument).
struct EnvRolloutArgs {
    PolicyDev  pol;
    PaddedTraj out;                  // records [E][t_pad]: obs bytes zero (the ids have their own array), logits, value, reward, action | twist
    uint16_t  *obs16;                // [E][t_pad][n_obs] obs ids as the environment wrote them (before the twist); a struct with
                                     // observe_n: the ids of the record, then 0xFFFF up to the row stride n_obs
    uint32_t  *err;                  // |= 1: an obs id outside [0, obs_size); |= 2: an episode did not end within t_pad records;
                                     // |= 8: observe_n returned a count outside 0 .. n_obs; |= 16 (rollout_env16x2_kernel and its pack
                                     // kernel alone): an operand outside the split terms' range; zeroed by the library before the launch.
                                     // An episode that met a bad id (count) at record t ends there: its ep_len is (t + 1) | 1 << 31,
                                     // record t's value field holds the id (the count) as bits and its reward field is 0.0f (1.0f)
    uint64_t   num_episodes, episode_offset, seed;
    unsigned int *queue;             // null: one column per episode (the grid covers them all).  Else the grid is PERSISTENT: fewer columns
                                     // than episodes, column i starts with episode i, and a column whose episode is over takes the next
                                     // index from this counter (which starts at the number of columns) until it passes num_episodes
    float     *lgw;                  // an environment of more than four actions: [E][t_pad][A] masked logits of the records, addressed by
                                     // episode like obs16 (the record's four logit slots are then zero and nobody reads them); else null
};

// ... and what rollout_env16_kernel (precision="fp16": the same loop over EngineV16, tw_engine_generic16.hpp) needs on top
struct EnvRollout16Args {
    EnvRolloutArgs r;
    Gen16Image     image;            // carved from the collect's workspace, packed by the launcher before the rollout.  image.halves with
                                     // GEN16X2_REQUEST (bit 63) set: precision="fp16x2" -- the image is EngineV16x2's (gen16x2_image_halves()
                                     // halves in the low bits) and the launcher runs pack_generic16x2_kernel and rollout_env16x2_kernel.
                                     // Only a module that answers groups_per_cu(5, 0, nullptr) is ever handed such a request
};

// evaluate(): one column = one attempt (episode, search), as solve_big_kernel
struct EnvSolveArgs {
    PolicyDev pol;
    uint64_t  num_attempts, episode_offset, seed;
    uint32_t  num_searches, deterministic, max_steps;
    uint32_t  from_state;            // solve(): every attempt starts from the prototype AS IT IS (solve.rs:85) -- no reset; its draw key is
                                     // the attempt's index (episode_offset 0, one episode)
    float    *success, *total;       // [num_attempts]
    uint32_t *n_steps;               // [num_attempts]; an attempt that met a bad id (a bad count of observe_n) at move t: t | 1 << 31,
                                     // its total = the id (the count) as bits; a bad count: its success = 2.0f
    uint32_t *err;                   // as EnvRolloutArgs::err (|= 4: an attempt did not end within max_steps steps)
    unsigned int *queue;             // as EnvRolloutArgs::queue, over attempts
    uint8_t  *actions;               // null, or [num_attempts][actions_stride]: the moves an attempt played, one byte each (A <= 31),
    uint32_t  actions_stride;        // addressed by attempt like the three results; a move at or beyond the stride is not stored
    Gen16Image image;                // img null: solve_env_kernel, f32.  Else precision="fp16": solve_env16_kernel over EngineV16 (a module
                                     // built with TW_DEVICE_ENV_FP16_SOLVE), the image carved from the call's workspace and packed by the
                                     // launcher before the kernel; the f32 kernel never reads this member.  image.halves with
                                     // GEN16X2_REQUEST (bit 63) set: precision="fp16x2" -- the image is EngineV16x2's and the launcher runs
                                     // pack_generic16x2_kernel and solve_env16x2_kernel (a module built with TW_DEVICE_ENV_FP16X2_SOLVE:
                                     // only one that answers groups_per_cu(6, 0, nullptr) is ever handed such a request); err then also
                                     // takes |= 16, GEN16X2_ERR_RANGE: an operand outside the split terms' range
};

// Self-play (solve_on == 0) and MCTS-guided evaluate (solve_on != 0) of mcts_env_kernel (tw_mcts_env.hpp), which a module has when it
// was built with TW_DEVICE_ENV_SEARCH or TW_DEVICE_ENV_WIDE_SEARCH.  One column = one episode, or one attempt (episode, search) as in EnvSolveArgs.
struct EnvMctsArgs {
    uint32_t   struct_bytes, pad0;   // sizeof(EnvMctsArgs) as the caller knows it: the launcher refuses another one (hipErrorInvalidValue)
    PolicyDev  pol;
    PaddedTraj out;                  // self-play: records [E][t_pad] with the MCTS probabilities in the four logit slots, value 0, reward =
                                     // env.reward() of the recorded state; ep_len
    uint16_t  *obs16;                // self-play: [E][t_pad][n_obs] obs ids, as EnvRolloutArgs::obs16
    uint32_t  *err;                  // as EnvRolloutArgs::err / EnvSolveArgs::err; zeroed by the library before the launch
    uint32_t  *col_err;              // [columns][4], zeroed likewise: {0} = the column ended by itself, else {1 + kind, ordinal, what, 0} --
                                     // kind 0: obs id `what` out of range, 1: observe_n count `what` out of range, at the column's
                                     // evaluation number `ordinal` (0 = its first); kind 2: not ended within t_pad records / max_steps
                                     // steps, after `ordinal` evaluations
    uint64_t   num_columns, episode_offset, seed;
    uint32_t   num_searches, max_expand_depth;
    float      C;
    uint32_t   node_cap;             // nodes per column's tree, at least env_mcts_node_cap()
    void      *arena;                // [columns][node_cap] nodes of ENV_MCTS_NODE_BYTES
    unsigned long long *eval_count;  // [1] += the policy evaluations the searches consumed (roots and leaves)
    uint32_t   solve_on, deterministic, attempts /* per episode */, max_steps;
    float     *success, *total;      // solve mode: [columns]
    uint32_t  *n_steps;              // solve mode: [columns]
    float     *pw;                   // self-play of an environment of more than four actions: [E][t_pad][A] MCTS probabilities of the records,
                                     // addressed like obs16 (the record's four logit slots are then zero and nobody reads them); else null
    uint32_t   from_state, actions_stride;   // solve mode, as EnvSolveArgs: no reset of the prototype; the row stride of `actions`
    uint8_t   *actions;              // solve mode: null, or [columns][actions_stride] the moves a column played
    Gen16Image image;                // img null: mcts_env_kernel, f32.  Else precision="fp16": mcts_env16_kernel over EngineV16 (a module
                                     // built with TW_DEVICE_ENV_FP16_SEARCH), the image carved from the call's workspace and packed by the
                                     // launcher before the kernel; the f32 kernel never reads this member
};
constexpr int ENV_MCTS_NODE_BYTES = 32;
// the most nodes one move's tree can hold: the root, its children, and per search at most max(max_expand_depth, 1) expansions
constexpr uint64_t env_mcts_node_cap(uint32_t n_actions, uint32_t num_searches, uint32_t max_expand_depth)
{
    return 1ull + n_actions + (uint64_t)n_actions * num_searches * (max_expand_depth ? max_expand_depth : 1u);
}
// LDS of mcts_env_kernel behind the engine's: the ids of the 16 columns' pending states
constexpr size_t env_mcts_pending_bytes(uint32_t n_obs) { return (size_t)16 * n_obs * sizeof(int); }
// ... and behind those, for an environment of more than four actions, a row of n_actions floats per column: the twist average of the
// action head, which the column's owner lane turns into the probabilities in place
constexpr size_t env_mcts_probs_bytes(uint32_t n_actions) { return n_actions > 4 ? (size_t)16 * n_actions * sizeof(float) : 0; }

// EngineV column count for an environment of n_obs ids: the smallest instantiation the Puzzle kernels already use
constexpr int env_engine_nc(int n_obs) { return n_obs <= 4 ? 4 : n_obs <= 9 ? 9 : n_obs <= 16 ? 16 : n_obs <= 25 ? 25 : n_obs <= 36 ? 36 : 64; }

}  // namespace tw

// The descriptor a module exports (tw_device_env_<name>()).  `layout` = what the module was compiled against; the library refuses a
// descriptor whose layout differs from its own (tw_device_env_layout()).
enum { TW_DEVICE_ENV_MAGIC = 0x45445754u, TW_DEVICE_ENV_LAYOUT_WORDS = 8 };    // "TWDE"
struct tw_device_env {
    uint32_t layout[TW_DEVICE_ENV_LAYOUT_WORDS];
    uint32_t num_actions, n_obs, state_bytes, engine_nc;
    const char *type_name;
    // launchers: hipFuncSetAttribute (dynamic LDS) + the launch; a hipError_t
    int (*launch_rollout)(const tw::EnvRolloutArgs *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s);
    int (*launch_solve)(const tw::EnvSolveArgs *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s);
    // host side of the same struct: a new object from constructor parameters (null if init() refuses them), the accessors the
    // Python surface needs, and the tw_env_vtable methods over the type (prototype, obs_size left to the caller)
    void *(*create)(const double *params, int n);
    int   (*get_difficulty)(const void *env);
    void  (*set_difficulty)(void *env, int d);
    int   (*obs_size)(const void *env);
    int   (*n_obs_of)(const void *env);                    // ids per observation of THIS object: n_obs, or the struct's own n_obs() (<= n_obs)
    void  (*fill_vtable)(tw_env_vtable *out);
    // null unless the module was built with TW_DEVICE_ENV_SEARCH / TW_DEVICE_ENV_WIDE_SEARCH: the launcher of mcts_env_kernel (tw_mcts_env.hpp).
    // lds_bytes is the engine's share; the launcher adds env_mcts_pending_bytes(n_obs) + env_mcts_probs_bytes(num_actions).  (layout[2], this struct's size, tells the two layouts apart;
    // the launcher itself checks EnvMctsArgs::struct_bytes.)
    int (*launch_search)(const tw::EnvMctsArgs *a, const void *proto, unsigned blocks, size_t engine_lds_bytes, hipStream_t s);
    // how many workgroups of one of the module's kernels -- 0: rollout, 1: solve, 2: search -- a CU holds at once with lds_bytes of
    // dynamic LDS (what the launcher of that kernel is given): the kernel's own answer, hipOccupancyMaxActiveBlocksPerMultiprocessor,
    // from which the library sizes a persistent grid.  A hipError_t; kernel 2 of a module without the search kernel: hipErrorInvalidValue.
    // Kernel 3: solve_env16_kernel of a module built with TW_DEVICE_ENV_FP16_SOLVE (lds_bytes = EngineV16<engine_nc>::lds_bytes(pol));
    // any other module: hipErrorInvalidValue.  Kernel 3 with out == nullptr only asks whether the module holds that kernel: hipSuccess
    // without a call into the HIP runtime (no device needed), which is how the library and DeviceEnv.fp16_solve learn it -- the
    // descriptor has no member for it.  launch_solve runs that kernel, the pack of the image in front of it, when EnvSolveArgs::image.img
    // is not null (a module without the kernel, or a policy EngineV16 does not take: hipErrorInvalidValue).
    // Kernel 4: mcts_env16_kernel of a module built with TW_DEVICE_ENV_FP16_SEARCH beside a search form (lds_bytes = the f16 engine's
    // share, EngineV16<engine_nc>::lds_bytes(pol); the pending ids and the rows of probabilities are added as for kernel 2); any other
    // module: hipErrorInvalidValue.  Kernel 4 with out == nullptr is that kernel's capability query, as kernel 3's (the library's
    // search_f16(), DeviceEnv.fp16_search).  launch_search runs that kernel, the pack of the image in front of it, when
    // EnvMctsArgs::image.img is not null.
    // Kernel 5: rollout_env16x2_kernel of a module built with TW_DEVICE_ENV_FP16X2 (lds_bytes = EngineV16x2<engine_nc>::lds_bytes(pol));
    // any other module: hipErrorInvalidValue.  Kernel 5 with out == nullptr is that kernel's capability query, as kernel 3's (the PPO
    // collect's dispatch, DeviceEnv.fp16x2): the library asks it BEFORE it hands launch_rollout16 a split request -- bit 63 of
    // EnvRollout16Args::image.halves, GEN16X2_REQUEST -- so a module from before that kernel never sees one.  launch_rollout16 then
    // runs pack_generic16x2_kernel and that kernel instead of the fp16 pair.
    // Kernel 6: solve_env16x2_kernel of a module built with TW_DEVICE_ENV_FP16X2_SOLVE (lds_bytes = EngineV16x2<engine_nc>::lds_bytes(pol));
    // any other module: hipErrorInvalidValue.  Kernel 6 with out == nullptr is that kernel's capability query (evaluate's and solve's
    // dispatch, DeviceEnv.fp16x2_solve): the library asks it BEFORE it hands launch_solve a split request -- bit 63 of
    // EnvSolveArgs::image.halves -- so a module from before that kernel never sees one.
    // Kernel 7: pack_basic_view_kernel of a module built with TW_DEVICE_ENV_BASIC (tw_env_basic_view.hpp; lds_bytes is not used); any
    // other module: hipErrorInvalidValue.  Kernel 7 with out == nullptr is the capability query (every entry point's dispatch,
    // DeviceEnv.basic): the library asks it BEFORE it hands launch_rollout / launch_solve / launch_search a VIEW of a one-common-layer
    // policy -- PolicyDev::generic with a non-zero PolicyDev::hidden, `layers` pointing at a block of the call's workspace that the
    // launcher packs before its kernel -- so a module without that kernel never sees one.  No argument struct grew for it
    int (*groups_per_cu)(int kernel, size_t lds_bytes, int *out);
    // null unless the module was built with TW_DEVICE_ENV_FP16 (build_device_env(..., fp16=True)): pack_generic16_kernel (the policy's
    // f32 device copies -> the binary16 image a->image, on stream s) and then rollout_env16_kernel, with launch_rollout's return
    // convention (hipErrorInvalidValue: no image, or a policy EngineV16 does not take); and that kernel's occupancy, as
    // groups_per_cu gives the others'.  lds_bytes = EngineV16<engine_nc>::lds_bytes(pol).
    int (*launch_rollout16)(const tw::EnvRollout16Args *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s);
    int (*groups_per_cu16)(size_t lds_bytes, int *out);
};

inline void tw_device_env_layout(uint32_t (&out)[TW_DEVICE_ENV_LAYOUT_WORDS])
{
    out[0] = TW_DEVICE_ENV_MAGIC; out[1] = TW_ABI_VERSION; out[2] = (uint32_t)sizeof(tw_device_env); out[3] = (uint32_t)sizeof(tw::PolicyDev);
    out[4] = (uint32_t)sizeof(tw::EnvRolloutArgs); out[5] = (uint32_t)sizeof(tw::EnvSolveArgs); out[6] = (uint32_t)sizeof(tw::PaddedRec);
    out[7] = (uint32_t)sizeof(tw_env_vtable);
}

namespace tw {

// ids per observation: the struct's own n_obs() where it has one (BigPuzzleEnv<25>, tw_big_board.hpp, holds boards of 1 .. 25 cells),
// else the constant Env::N_OBS -- which is what every use below folds to for a struct without the method
template <class Env, class = void>
struct EnvNObs { __host__ __device__ static constexpr int of(const Env &) { return Env::N_OBS; } };
template <class Env>
struct EnvNObs<Env, decltype((void)std::declval<const Env &>().n_obs())> { __host__ __device__ static int of(const Env &e) { return e.n_obs(); } };
template <class Env>
__host__ __device__ inline int env_n_obs(const Env &e) { return EnvNObs<Env>::of(e); }

// Observations of variable length: a struct that defines `int observe_n(int *ids) const` (the ids of THIS state, at most env_n_obs
// of them, and their count) is asked through it, and need not have observe().  Detected as n_obs() is above; a struct without the
// method compiles to what it compiled to before (every use below is an `if constexpr`).
template <class Env, class = void>
struct EnvHasObserveN : std::false_type {};
template <class Env>
struct EnvHasObserveN<Env, decltype((void)std::declval<const Env &>().observe_n(std::declval<int *>()))> : std::true_type {};
template <class Env, class = void>
struct EnvHasObserve : std::false_type {};
template <class Env>
struct EnvHasObserve<Env, decltype((void)std::declval<const Env &>().observe(std::declval<int *>()))> : std::true_type {};

// sample_from_logits (policy.rs:169-172) over the environment's A <= 4 actions: the words of ONE draw (t, STREAM_GUMBEL) as the
// host path takes them (tw_env_generic.hip), first maximum wins, NaN never; A = 4 is gumbel_argmax4
template <int A>
__device__ __forceinline__ int gumbel_argmax_n(const float (&l)[4], const u32x4 w)
{
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    int best = 0; float bv = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        const float a1 = tw_logf(u32_to_unit(ww[i]));
        const float gi = l[i] - tw_logf(__builtin_fabsf(a1));
        if (i == 0) { bv = gi; best = 0; } else if (gi > bv) { bv = gi; best = i; }
    }
    return best;
}

// act_perm of a twist over A actions (EngineV::act_perm reads a table of four per twist): lg[i] = lg[act_perms[perm][i]]
template <int A>
__device__ __forceinline__ void env_act_perm(const PolicyDev &pol, int perm, float (&lg)[4])
{
    if (perm < 0) return;
    const float l0 = lg[0], l1 = lg[1], l2 = lg[2], l3 = lg[3];
#pragma unroll
    for (int i = 0; i < A; ++i) {
        const int src = pol.act_perms[perm * A + i];
        lg[i] = src == 0 ? l0 : (src == 1 ? l1 : (src == 2 ? l2 : l3));
    }
}

// ---- environments of 5 .. 31 actions (TW_DEVICE_ENV_WIDE) -----------------------------------------------------------------------------
// The action head's outputs stay where EngineV::forward_head leaves them -- LDS, [unit][column] rows of GEN_STRIDE floats -- and the
// step STREAMS over the actions instead of holding A values in registers (EngineV<64> alone takes some 450): action i reads unit
// act_perms[perm][i] (i without a twist) of column j, so a twist is an LDS index, never an index into a register array.

// the head's unit behind action i under twist `perm` (policy.rs:95-97; PolicyDev::act_perms is [n_perms][A])
template <int A>
__device__ __forceinline__ int env_head_unit(const PolicyDev &pol, int perm, int i) { return perm < 0 ? i : (int)pol.act_perms[perm * A + i]; }

// The rollout's step: mask (policy.rs:62), sample_from_logits (policy.rs:169-172) with the words the host path takes
// (tw_env_generic.hip: draw t | ((i >> 2) << 24), word i & 3), first maximum wins.  `row` (null: nothing is stored) is the record's
// row of EnvRolloutArgs::lgw; all sixteen lane groups of the workgroup carry column j, so group g stores the logits g and g + 16.
template <int A>
__device__ __forceinline__ int env_gumbel_stream(const PolicyDev &pol, const float *head, int j, int g, int perm, uint32_t mb, uint64_t seed,
                                                 uint64_t key, uint32_t t, float *row)
{
    // ONE rolled loop (a draw every fourth action): with EngineV<64> around it the kernel is large enough that every basic block counts
    // towards the compiler's limit for inlining the struct's methods
    int best = 0; float bv = 0.0f;
    u32x4 w = {};
#pragma unroll 1
    for (int i = 0; i < A; ++i) {
        if ((i & 3) == 0) w = rng_draw(seed, key, t | ((uint32_t)(i >> 2) << 24), STREAM_GUMBEL);
        const uint32_t word = (i & 3) == 0 ? w.x : ((i & 3) == 1 ? w.y : ((i & 3) == 2 ? w.z : w.w));
        const float l  = head[env_head_unit<A>(pol, perm, i) * GEN_STRIDE + j];
        const float lm = ((mb >> i) & 1u) ? l : -1e10f;
        if (row && g == (i & 15)) row[i] = lm;
        const float a1 = tw_logf(u32_to_unit(word));
        const float gi = lm - tw_logf(__builtin_fabsf(a1));
        if (i == 0) { bv = gi; best = 0; } else if (gi > bv) { bv = gi; best = i; }
    }
    return best;
}

// evaluate's step: Policy::predict (policy.rs:43-47: tw_expf of the allowed logits, summed in index order, / (sum + 1e-6)) and the
// arg-max of policy.rs:130-151 or nn::policy::sample (sample_weighted, tw_common.hpp), in passes over the LDS-resident logits: the
// operations, their order and their bits are those of masked_softmax4 + sample_weighted over A values.
template <int A>
__device__ __forceinline__ float env_prob_at(const PolicyDev &pol, const float *head, int j, int perm, uint32_t mb, int i)
{
    return ((mb >> i) & 1u) ? tw_expf(head[env_head_unit<A>(pol, perm, i) * GEN_STRIDE + j]) : 0.0f;
}
template <int A>
__device__ __forceinline__ int env_predict_stream(const PolicyDev &pol, const float *head, int j, int perm, uint32_t mb, bool deterministic, float u)
{
    // pass 0: the sum of the exponentials (den = 1: x / 1.0f is x); pass 1: the probabilities -- their arg-max, or their validity and
    // total; pass 2 (sampling): the cumulative weights of the first A - 1 against u * total.  One loop body for all three.
    float den = 1.0f, acc = 0.0f, bv = 0.0f, chosen = 0.0f;
    bool bad = false, found = false;
    int action = 0;
    const int n_pass = deterministic ? 2 : 3;
#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
        acc = 0.0f;
#pragma unroll 1
        for (int i = 0; i < A; ++i) {
            const float p = env_prob_at<A>(pol, head, j, perm, mb, i) / den;
            acc = acc + p;
            if (pass == 1) {
                if (!deterministic) { if (!(p >= 0.0f)) bad = true; }
                else if (i == 0) bv = p;
                else if (p > bv) { bv = p; action = i; }
            } else if (pass == 2) {
                if (i < A - 1 && !found && !(acc <= chosen)) { action = i; found = true; }
            }
        }
        if (pass == 0) den = acc + 0.000001f;
        else if (pass == 1 && !deterministic) {
            if (bad || !(acc > 0.0f)) { action = 0; break; }                          // invalid weights: 0, as the reference
            chosen = u * acc;
            action = A - 1;
        }
    }
    return action;
}

// observe + guard + twist: rows of the forward (-1 = no row) and the raw ids.  An id outside [0, obs_size) is never used as an
// index: its row is -1, `bad` is set and `bad_id` is the FIRST such id of the observation (the one the host path reports; the
// caller ends the episode and flags the collect).
template <class Env, int NC>
__device__ __forceinline__ void env_rows(const Env &st, const PolicyDev &pol, int perm, int (&ids)[Env::N_OBS], int (&rowoff)[NC], bool &bad, int &bad_id)
{
    st.observe(ids);
    const int n = env_n_obs(st);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        int row = -1;
        if (i < Env::N_OBS && i < n) {
            const int id = ids[i];
            if ((unsigned)id >= (unsigned)pol.obs_size) { if (!bad) bad_id = id; bad = true; }
            else row = perm < 0 ? id : (pol.obs_size > 256 ? (int)pol.obs_perms16[(size_t)perm * pol.obs_size + id]
                                                            : (int)pol.obs_perms[(size_t)perm * pol.obs_size + id]);
        }
        rowoff[i] = row;
    }
}

// The same for a struct with observe_n: the rows of the ids the state has, -1 beyond them; returns their number.  A count outside
// 0 .. env_n_obs is never used as an index: no id is read (the count becomes 0), `bad` and `bad_count` are set and `bad_id` is the
// count (the host path reports it before it looks at an id).  `obs_row` (the rollout's writer lanes; else null): where the record's
// raw ids go, followed by 0xFFFF = no id up to the row stride env_n_obs -- stored HERE, before the twist: with up to 64 ids and 64 rows
// alive together the 64-column kernel went to scratch memory.  (Of an observation that turns out to hold a bad id the row is written
// all the same; the collect fails and nobody reads it.)
template <class Env, int NC>
__device__ __forceinline__ int env_rows_n(const Env &st, const PolicyDev &pol, int perm, int (&ids)[Env::N_OBS], int (&rowoff)[NC], bool &bad, int &bad_id,
                                          bool &bad_count, uint16_t *obs_row)
{
    const int stride = env_n_obs(st);
    int n = st.observe_n(ids);
    if ((unsigned)n > (unsigned)stride) { bad = true; bad_count = true; bad_id = n; n = 0; }
    else if (obs_row) {
#pragma unroll
        for (int i = 0; i < Env::N_OBS; ++i) if (i < stride) obs_row[i] = i < n ? (uint16_t)ids[i] : (uint16_t)0xFFFFu;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        int row = -1;
        if (i < Env::N_OBS && i < n) {
            const int id = ids[i];
            if ((unsigned)id >= (unsigned)pol.obs_size) { if (!bad) bad_id = id; bad = true; }
            else row = perm < 0 ? id : (pol.obs_size > 256 ? (int)pol.obs_perms16[(size_t)perm * pol.obs_size + id]
                                                            : (int)pol.obs_perms[(size_t)perm * pol.obs_size + id]);
        }
        rowoff[i] = row;
    }
    return n;
}

// The four kernels.  Each step loop exists ONCE, as a body file that its f32 and its f16 kernel include inside their function
// bodies (tw_env_rollout_loop.hpp, tw_env_solve_loop.hpp: the loops' comments are there, and what a kernel declares in front of the
// #include).  A kernel is its engine, its LDS and that #include; the two of a pair differ in `Eng` and in where the arguments and the
// image come from, and in nothing else.  Shared by inclusion and not through a function template, because the f32 kernels are to stay
// what they are, instruction for instruction: with the loop in one __forceinline__ function that both kernels inline, this compiler
// allocated the f32 kernels differently (ProbeO64A4S: 1,032 instead of 1,040 bytes of scratch memory, GridWorld 5 x 5: 160 instead of
// 164 spilled SGPRs, or 280 instead of 276 VGPRs with the arguments by value), while the included text compiles to the assembly the
// written-out loops compiled to (device environments; profiles/r19_env_loop_identity.txt).
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) rollout_env_kernel(const EnvRolloutArgs a, const Env proto)
{
    using Eng = EngineV<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
#include "tw_env_rollout_loop.hpp"
}

// The same loop over EngineV16 (tw_engine_generic16.hpp): precision="fp16" of PPOCollector.collect.  A module holds it when it was
// built with TW_DEVICE_ENV_FP16 (build_device_env(..., fp16=True)); pack_generic16_kernel runs in front of it, on the same stream.
// tests/test_gpu_device_env_fp16.py holds its environment side, record by record, to the host code the f32 kernel is held to.
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) rollout_env16_kernel(const EnvRollout16Args a16, const Env proto)
{
    using Eng = EngineV16<NC>;
    const EnvRolloutArgs &a = a16.r;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
    eng.img = a16.image.img;
#include "tw_env_rollout_loop.hpp"
}

// rollout_env16x2_kernel, the same loop over EngineV16x2 (precision="fp16x2" of PPOCollector.collect), its launcher and its occupancy
// query live in tw_rollout_env16x2.hpp, which the end of this file includes: a third kernel that includes tw_env_rollout_loop.hpp.
// solve_env16x2_kernel, the evaluate loop over EngineV16x2, lives likewise in tw_solve_env16x2.hpp: the third kernel of that loop.

// evaluate() (rust/src/rl/evaluate.rs:22-89 over single_solve, rl/solve.rs:17-71), as solve_big_kernel: one column = one attempt
// (episode e, search a): reset, then while !is_final { total += reward; probs = Policy::predict (masked softmax, random twist);
// action = argmax | weighted sample; step }.  Best-of-N and the means are reduced on the host.  An attempt's three results are
// written when it ends; with a.queue its column then takes the next attempt, as rollout_env_kernel takes episodes.  The key of an
// attempt's draws, ep * num_searches + att % num_searches, is episode_offset * num_searches + att: no division on the step path.
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) solve_env_kernel(const EnvSolveArgs a, const Env proto)
{
    using Eng = EngineV<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
#include "tw_env_solve_loop.hpp"
}

// The same loop over EngineV16: precision="fp16" of collector.evaluate and collector.solve without MCTS.  A module holds it when it
// was built with TW_DEVICE_ENV_FP16_SOLVE (build_device_env(..., fp16_solve=True)); pack_generic16_kernel runs in front of it, on the
// same stream, into EnvSolveArgs::image.  tests/test_gpu_device_env_fp16_solve.py holds it, attempt by attempt, to the oracle's
// ARITH_F16 loop over the module's host code.
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) solve_env16_kernel(const EnvSolveArgs a, const Env proto)
{
    using Eng = EngineV16<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
    eng.img = a.image.img;
#include "tw_env_solve_loop.hpp"
}

// ---- launchers (host) ---------------------------------------------------------------------------------------------------------------------
// hipFuncSetAttribute (the kernel's dynamic LDS) and then the kernel's own answer to how many of its workgroups a CU holds at once:
// tw_device_env::groups_per_cu / groups_per_cu16 of every kernel
inline int kernel_groups_per_cu(const void *k, int threads, size_t lds_bytes, int *out)
{
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(out, k, threads, lds_bytes);
}

// What the launcher of an f16 kernel `k` does before it launches it: refuses a missing image and a policy EngineV16 does not take
// (hipErrorInvalidValue, before any HIP call), sets k's dynamic LDS, and packs the policy's f32 copies into the image on stream s.
// The pack runs in front of EVERY launch: the image is never older than the policy's f32 copies.  Its grid: one thread per eight
// halves, at most 1,024 workgroups (grid-stride beyond).  (A template, so that only a module with an f16 kernel holds the pack kernel.)
template <class Kernel>
int pack_image_for(Kernel *k, size_t lds_bytes, const PolicyDev &pol, const Gen16Image &image, hipStream_t s)
{
    const int n_layers = pol.n_common + pol.n_action + pol.n_value;
    if (!image.img || !pol.generic || n_layers > GEN16_MAX_LAYERS) return (int)hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    uint64_t pb = (image.halves / 8 + 255) / 256;
    if (pb > 1024) pb = 1024;
    hipLaunchKernelGGL((pack_generic16_kernel<256>), dim3((unsigned)(pb ? pb : 1)), dim3(256), 0, s, pol, image);
    return (int)hipGetLastError();
}

template <class Env>
int launch_rollout_env(const EnvRolloutArgs *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    Env p;
    __builtin_memcpy(&p, proto, sizeof(Env));
    const void *k = reinterpret_cast<const void *>(&rollout_env_kernel<Env, NC>);
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
#ifdef TW_DEVICE_ENV_BASIC
    const int eb = pack_basic_view_for(a->pol, s);        // (a view of a one-common-layer policy: its EngineV layers first, on the same stream)
    if (eb != (int)hipSuccess) return eb;
#endif
    hipLaunchKernelGGL((rollout_env_kernel<Env, NC>), dim3(blocks), dim3(EngineV<NC>::THREADS), lds_bytes, s, *a, p);
    return (int)hipGetLastError();
}

// defined in tw_rollout_env16x2.hpp (used below only inside #ifdef TW_DEVICE_ENV_FP16X2)
template <class Env>
int launch_rollout_env16x2(const EnvRollout16Args *a, const Env &p, unsigned blocks, size_t lds_bytes, hipStream_t s);
template <class Env>
int groups_per_cu_env16x2(size_t lds_bytes, int *out);
// defined in tw_solve_env16x2.hpp (used below only inside #ifdef TW_DEVICE_ENV_FP16X2_SOLVE)
template <class Env>
int launch_solve_env16x2(const EnvSolveArgs *a, const Env &p, unsigned blocks, size_t lds_bytes, hipStream_t s);
template <class Env>
int groups_per_cu_solve_env16x2(size_t lds_bytes, int *out);

// tw_device_env::launch_rollout16 / groups_per_cu16
template <class Env>
int launch_rollout_env16(const EnvRollout16Args *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    Env p;
    __builtin_memcpy(&p, proto, sizeof(Env));
#ifdef TW_DEVICE_ENV_FP16X2
    if (a->image.halves & GEN16X2_REQUEST) return launch_rollout_env16x2<Env>(a, p, blocks, lds_bytes, s);
#endif
    auto *k = &rollout_env16_kernel<Env, NC>;         // (taken BEFORE the call: a module's assembly lists its kernels in the order they are first named)
    const int e = pack_image_for(k, lds_bytes, a->r.pol, a->image, s);
    if (e != (int)hipSuccess) return e;
    hipLaunchKernelGGL((rollout_env16_kernel<Env, NC>), dim3(blocks), dim3(EngineV16<NC>::THREADS), lds_bytes, s, *a, p);
    return (int)hipGetLastError();
}

template <class Env>
int groups_per_cu_env16(size_t lds_bytes, int *out)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    if (!out) return (int)hipErrorInvalidValue;
    return kernel_groups_per_cu(reinterpret_cast<const void *>(&rollout_env16_kernel<Env, NC>), EngineV16<NC>::THREADS, lds_bytes, out);
}

// tw_device_env::groups_per_cu of a module without the search kernel (with it: groups_per_cu_search_env, tw_mcts_env.hpp)
template <class Env>
int groups_per_cu_env(int kernel, size_t lds_bytes, int *out)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
#ifdef TW_DEVICE_ENV_FP16_SOLVE
    // kernel 3: solve_env16_kernel, lds_bytes = EngineV16<engine_nc>::lds_bytes(pol).  With out == nullptr the question is only whether
    // the module HOLDS the kernel (the library's attempts_on_device(), DeviceEnv.fp16_solve): answered without the HIP runtime
    if (kernel == 3) {
        if (!out) return (int)hipSuccess;
        return kernel_groups_per_cu(reinterpret_cast<const void *>(&solve_env16_kernel<Env, NC>), EngineV16<NC>::THREADS, lds_bytes, out);
    }
#endif
#ifdef TW_DEVICE_ENV_FP16X2
    // kernel 5: rollout_env16x2_kernel, lds_bytes = EngineV16x2<engine_nc>::lds_bytes(pol); out == nullptr: the capability query
    if (kernel == 5) return groups_per_cu_env16x2<Env>(lds_bytes, out);
#endif
#ifdef TW_DEVICE_ENV_FP16X2_SOLVE
    // kernel 6: solve_env16x2_kernel, lds_bytes = EngineV16x2<engine_nc>::lds_bytes(pol); out == nullptr: the capability query
    if (kernel == 6) return groups_per_cu_solve_env16x2<Env>(lds_bytes, out);
#endif
#ifdef TW_DEVICE_ENV_BASIC
    // kernel 7: pack_basic_view_kernel (tw_env_basic_view.hpp); out == nullptr: the capability query
    if (kernel == ENV_KERNEL_PACK_BASIC) return groups_per_cu_pack_basic(out);
#endif
    if (!out || (kernel != 0 && kernel != 1)) return (int)hipErrorInvalidValue;
    const void *k = kernel == 0 ? reinterpret_cast<const void *>(&rollout_env_kernel<Env, NC>) : reinterpret_cast<const void *>(&solve_env_kernel<Env, NC>);
    return kernel_groups_per_cu(k, EngineV<NC>::THREADS, lds_bytes, out);
}

// tw_device_env::launch_solve.  EnvSolveArgs::image.img null: solve_env_kernel.  Else the pack of the image and solve_env16_kernel,
// as launch_rollout_env16 runs the collect's -- in a module built with TW_DEVICE_ENV_FP16_SOLVE; any other module holds no such kernel
// and refuses (hipErrorInvalidValue), as this one refuses a policy EngineV16 does not take.  An image whose size carries
// GEN16X2_REQUEST: the split pack and solve_env16x2_kernel (launch_solve_env16x2), in a module built with TW_DEVICE_ENV_FP16X2_SOLVE --
// the library asks groups_per_cu(6, 0, nullptr) first, so no other module is handed one.
template <class Env>
int launch_solve_env(const EnvSolveArgs *a, const void *proto, unsigned blocks, size_t lds_bytes, hipStream_t s)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    Env p;
    __builtin_memcpy(&p, proto, sizeof(Env));
#ifdef TW_DEVICE_ENV_FP16X2_SOLVE
    if (a->image.halves & GEN16X2_REQUEST) return launch_solve_env16x2<Env>(a, p, blocks, lds_bytes, s);
#endif
    if (a->image.img) {
#ifdef TW_DEVICE_ENV_FP16_SOLVE
        auto *k16 = &solve_env16_kernel<Env, NC>;         // (taken before the call, as in launch_rollout_env16)
        const int e16 = pack_image_for(k16, lds_bytes, a->pol, a->image, s);
        if (e16 != (int)hipSuccess) return e16;
        hipLaunchKernelGGL((solve_env16_kernel<Env, NC>), dim3(blocks), dim3(EngineV16<NC>::THREADS), lds_bytes, s, *a, p);
        return (int)hipGetLastError();
#else
        return (int)hipErrorInvalidValue;
#endif
    }
    const void *k = reinterpret_cast<const void *>(&solve_env_kernel<Env, NC>);
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
#ifdef TW_DEVICE_ENV_BASIC
    const int eb = pack_basic_view_for(a->pol, s);        // (as launch_rollout_env)
    if (eb != (int)hipSuccess) return eb;
#endif
    hipLaunchKernelGGL((solve_env_kernel<Env, NC>), dim3(blocks), dim3(EngineV<NC>::THREADS), lds_bytes, s, *a, p);
    return (int)hipGetLastError();
}

}  // namespace tw

#include "tw_rollout_env16x2.hpp"
#include "tw_solve_env16x2.hpp"
