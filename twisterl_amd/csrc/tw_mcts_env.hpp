// tw_mcts_env.hpp -- AlphaZero self-play and MCTS-guided evaluate of a user-written device environment ON THE DEVICE: the search
// of tw_mcts_big.hip as a template over the environment struct (include/twisterl_device_env.hpp).
//
// The same algorithm, RNG keys and arithmetic as mcts_big_kernel and as HostMcts (tw_env_generic.hip: AZCollector::single_collect,
// rust/src/collector/az.rs:51-109, over predict_probs_mcts, rust/src/rl/search.rs:104-189; solve mode: single_solve,
// rust/src/rl/solve.rs:17-71): one column of EngineV = one episode (one attempt), one batched Policy::full_predict per search step
// across the 16 columns of a workgroup, the per-episode tree in an HBM arena of 32-byte nodes WITHOUT a state, children contiguous.
// What the Puzzle lines of that kernel were is the struct here:
//   * reset / step / masks / reward / is_final / success are the struct's; only actions < Env::NUM_ACTIONS are expanded, sampled and
//     counted, the uniform fallback of the visit counts is 1 / NUM_ACTIONS;
//   * a node's state is re-derived by replaying the actions from the move's root.  The host path clones the environment per node;
//     the two agree because a device environment's step() depends on the struct and the action alone (the contract);
//   * two states per lane: the episode's and the walking one.  The state whose evaluation is pending is always the walking one
//     (it is set to the episode's wherever a move begins), so no third copy and no choice between two register structs;
//   * only the owner lane of a column holds its tree and states.  It observes the pending state, guards the ids (env_rows /
//     env_rows_n: the id guard, the count guard) and hands the ids -- -1 where the observation has none -- to the forward through
//     LDS; every lane derives its rows per twist pass from them (env_twist_row: both table widths);
//   * a bad id or a bad observe_n count at ANY evaluated state never indexes anything: the column ends, err gets bit 0 or 3, and
//     col_err[column] = {1 + kind, the column's evaluation ordinal, the id or the count, 0}.  An episode that has not ended after
//     t_pad records (solve mode: max_steps steps) sets bit 1 (bit 2) and leaves kind 2 with the evaluations it had consumed.
// The library (tw_device_env.hip) owns the checks, the workspace, the scan / finalize / compaction and the messages.  A module gets
// this kernel with TW_DEVICE_ENV_SEARCH; the MFMAs are EngineV's, the intrinsic form only (tw_engine_generic.hpp).
// The loop itself is NOT here: tw_env_mcts_loop.hpp holds its text once, and mcts_env_kernel (EngineV, f32) and mcts_env16_kernel
// (EngineV16, precision="fp16": a module built with TW_DEVICE_ENV_FP16_SEARCH as well) include it inside their bodies.  A change to the
// search is made there, and reaches both kernels.
// More than four actions (TW_DEVICE_ENV_WIDE_SEARCH): the SAME kernel, every difference an `if constexpr (A > 4)`.  The twist average
// of the action head is kept per (action, column) in LDS behind the pending ids (env_mcts_probs_bytes), the owner lane turns its
// column's row into the probabilities in place, and everything that was four registers -- the priors of the children just created, the
// children of a node in the UCB descent, the visit counts at the end of a move -- is a rolled loop over that row or over the nodes
// themselves: nothing of A values is ever a register array indexed at run time.  A record's A probabilities go to EnvMctsArgs::pw.
#pragma once
#include "tw_rollout_env.hpp"

namespace tw {

struct __attribute__((aligned(16))) EnvNode {     // MCTSNode + Node<T> (search.rs:20-26, tree.rs:18-23) without the state
    float    value_sum;
    uint32_t visit;
    float    prior;
    uint32_t parent;       // 0xffffffff = None
    uint32_t child_base;   // children are contiguous in the arena (expand adds them together)
    uint32_t meta;         // n_children | action_taken << 8 (0xff = None)
    uint32_t pad[2];
};
static_assert(sizeof(EnvNode) == ENV_MCTS_NODE_BYTES, "EnvNode must be 32 bytes");

constexpr uint32_t EN_NONE = 0xffffffffu;
enum { EP_ROOT = 0, EP_LEAF = 1, EP_DONE = 2 };

// the row of the embedding table an id selects under twist `perm` (-1: none); id < 0: no row
__device__ __forceinline__ int env_twist_row(const PolicyDev &pol, int perm, int id)
{
    if (id < 0) return -1;
    return perm < 0 ? id : (pol.obs_size > 256 ? (int)pol.obs_perms16[(size_t)perm * pol.obs_size + id]
                                                 : (int)pol.obs_perms[(size_t)perm * pol.obs_size + id]);
}

// sample_weighted (tw_common.hpp; the host path's sample_weighted_host) over n weights that are streamed -- w(i) reads weight i from
// where it lives, LDS or the nodes just written -- instead of held: a weight that is negative or NaN gives 0, the cumulative sums run
// in index order, the index is the number of leading sums <= u * total among the first n - 1.
template <class W>
__device__ __forceinline__ int env_sample_stream(W w, int n, float u)
{
    if (n <= 0) return 0;
    float total = 0.0f;
    bool bad = false;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const float x = w(i);
        if (!(x >= 0.0f)) bad = true;
        total = total + x;
    }
    if (bad || !(total > 0.0f)) return 0;
    const float chosen = u * total;
    float cum = 0.0f;
    int idx = 0;
#pragma unroll 1
    for (int i = 0; i < n - 1; ++i) {
        cum = cum + w(i);
        if (!(cum <= chosen)) break;
        idx = i + 1;
    }
    return idx;
}

template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) mcts_env_kernel(const EnvMctsArgs a, const Env proto)
{
    using Eng = EngineV<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
#include "tw_env_mcts_loop.hpp"
}

// The same loop over EngineV16 (tw_engine_generic16.hpp): AZCollector(precision="fp16").collect and collector.evaluate / collector.solve
// with num_mcts_searches > 0 and precision="fp16".  Every Linear and the embedding sum are the f16-input forward -- weights and
// activations rounded to binary16, f32 accumulation, f32 biases: what solve_env16_kernel computes -- and everything behind the heads
// is the f32 text of the loop, unchanged.  A module holds it when it was built with TW_DEVICE_ENV_FP16_SEARCH
// (build_device_env(..., fp16_search=True)); pack_generic16_kernel runs in front of it, on the same stream, into EnvMctsArgs::image.
// tests/test_gpu_device_env_fp16_search.py holds it to the oracle's ARITH_F16 searches over the module's host code.
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) mcts_env16_kernel(const EnvMctsArgs a, const Env proto)
{
    using Eng = EngineV16<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
    eng.img = a.image.img;
#include "tw_env_mcts_loop.hpp"
}

// hipFuncSetAttribute (dynamic LDS: the engine's share, which the library passes, plus the pending ids of the 16 columns and, with more
// than four actions, their rows of A floats) + the launch
template <class Env>
int launch_mcts_env(const EnvMctsArgs *a, const void *proto, unsigned blocks, size_t engine_lds_bytes, hipStream_t s)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    using Eng = EngineV<NC>;
    const uint64_t need = env_mcts_node_cap(Env::NUM_ACTIONS, a->num_searches, a->max_expand_depth);
    if (a->struct_bytes != sizeof(EnvMctsArgs) || a->node_cap < need || !a->arena || !a->eval_count || !a->err || !a->col_err ||
        (a->solve_on ? (!a->success || !a->total || !a->n_steps || a->attempts == 0 || a->max_steps == 0)
                     : (!a->out.rec || !a->out.ep_len || !a->obs16 || a->out.t_pad < 1 || (Env::NUM_ACTIONS > 4 && !a->pw))) ||
        blocks == 0 || (uint64_t)blocks * Eng::EPB < a->num_columns ||
        (a->actions && (!a->solve_on || a->num_columns * (uint64_t)a->actions_stride > 0xffffffffull)))       // (the kernel's 32-bit row index)
        return (int)hipErrorInvalidValue;
    const size_t lds_bytes = engine_lds_bytes + env_mcts_pending_bytes(Env::N_OBS) + env_mcts_probs_bytes(Env::NUM_ACTIONS);
    Env p;
    __builtin_memcpy(&p, proto, sizeof(Env));
    if (a->image.img) {
        // precision="fp16": the pack of the image and mcts_env16_kernel, as launch_solve_env runs solve_env16_kernel -- in a module built
        // with TW_DEVICE_ENV_FP16_SEARCH; any other module holds no such kernel and refuses, as this one refuses a policy EngineV16 does
        // not take.  engine_lds_bytes is then EngineV16<NC>::lds_bytes(pol)
#ifdef TW_DEVICE_ENV_FP16_SEARCH
        auto *k16 = &mcts_env16_kernel<Env, NC>;          // (taken before the call, as in launch_rollout_env16)
        const int e16 = pack_image_for(k16, lds_bytes, a->pol, a->image, s);
        if (e16 != (int)hipSuccess) return e16;
        hipLaunchKernelGGL((mcts_env16_kernel<Env, NC>), dim3(blocks), dim3(EngineV16<NC>::THREADS), lds_bytes, s, *a, p);
        return (int)hipGetLastError();
#else
        return (int)hipErrorInvalidValue;
#endif
    }
    const void *k = reinterpret_cast<const void *>(&mcts_env_kernel<Env, NC>);
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
#ifdef TW_DEVICE_ENV_BASIC
    const int eb = pack_basic_view_for(a->pol, s);        // (a view of a one-common-layer policy: as launch_rollout_env)
    if (eb != (int)hipSuccess) return eb;
#endif
    hipLaunchKernelGGL((mcts_env_kernel<Env, NC>), dim3(blocks), dim3(Eng::THREADS), lds_bytes, s, *a, p);
    return (int)hipGetLastError();
}

// tw_device_env::groups_per_cu of a module with the search kernel (kernel 2: lds_bytes is the engine's share, as for the launcher)
template <class Env>
int groups_per_cu_search_env(int kernel, size_t lds_bytes, int *out)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
#ifdef TW_DEVICE_ENV_FP16_SEARCH
    // kernel 4: mcts_env16_kernel, lds_bytes = EngineV16<engine_nc>::lds_bytes(pol).  With out == nullptr the question is only whether
    // the module HOLDS the kernel (the library's fp16 search paths, DeviceEnv.fp16_search): answered without the HIP runtime
    if (kernel == 4) {
        if (!out) return (int)hipSuccess;
        const size_t all16 = lds_bytes + env_mcts_pending_bytes(Env::N_OBS) + env_mcts_probs_bytes(Env::NUM_ACTIONS);
        return kernel_groups_per_cu(reinterpret_cast<const void *>(&mcts_env16_kernel<Env, NC>), EngineV16<NC>::THREADS, all16, out);
    }
#endif
    // (kernels 0, 1, 3, 5, 6 -- solve_env16x2_kernel of TW_DEVICE_ENV_FP16X2_SOLVE -- and 7 -- pack_basic_view_kernel of
    // TW_DEVICE_ENV_BASIC -- are the plain module's, with its answers)
    if (kernel != 2) return groups_per_cu_env<Env>(kernel, lds_bytes, out);
    if (!out) return (int)hipErrorInvalidValue;
    const size_t all = lds_bytes + env_mcts_pending_bytes(Env::N_OBS) + env_mcts_probs_bytes(Env::NUM_ACTIONS);
    return kernel_groups_per_cu(reinterpret_cast<const void *>(&mcts_env_kernel<Env, NC>), EngineV<NC>::THREADS, all, out);
}

}  // namespace tw
