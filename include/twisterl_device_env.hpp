// twisterl_device_env.hpp -- write your own environment and collect it on the device.
//
// The reference's extension story is `trait Env` (rust/src/rl/env.rs:18-68, its README's "Creating your own environment",
// examples/grid_world).  Here an environment is a C++ struct whose methods are all __host__ __device__: the SAME code runs inside
// the fused PPO rollout / evaluate kernels (twisterl_amd/csrc/tw_rollout_env.hpp, one GPU lane group per episode) and behind a host
// tw_env_vtable (the host-stepped collectors, and the reference oracle in the tests).  A module is built with
//
//     twisterl_amd.build.build_device_env("my_env.hpp", "MyEnv", "my_env")      # -> libtw_env_my_env.so
//
// which compiles `#include "my_env.hpp"` + `TW_DEVICE_ENV(MyEnv, my_env)` with the library's own flags (search=True:
// TW_DEVICE_ENV_SEARCH, which adds the self-play / MCTS-evaluate kernel -- at the end of this file), and loaded with
// twisterl_amd.env.DeviceEnv(path, "my_env", params=[...]).  The contract (checked by static_assert below):
//
//   struct MyEnv {                                      // trivially copyable, default-constructible, at most 1 KiB: the prototype AND
//                                                       // the per-episode state
//       static constexpr int NUM_ACTIONS = 4;           // 1..4; 5..31 with TW_DEVICE_ENV_WIDE (below)
//       static constexpr int N_OBS       = 25;          // observe() writes EXACTLY this many ids, 1..64 (observe_n(): at most)
//       __host__ __device__ int      obs_size() const;  // every id < obs_size() <= 65535 (the policy's obs_size)
//       __host__ __device__ int      difficulty() const;
//       __host__            void     set_difficulty(int d);
//       __host__ __device__ void     reset(uint64_t seed, uint64_t episode);   // Env::reset; episode = the GLOBAL episode index
//       __host__ __device__ void     step(int action);
//       __host__ __device__ void     observe(int *ids) const;                  // N_OBS ids            } one of the two
//       __host__ __device__ int      observe_n(int *ids) const;                // 0..N_OBS ids, returns how many } (see below)
//       __host__ __device__ uint32_t masks() const;                            // bit i = action i allowed
//       __host__ __device__ float    reward() const;
//       __host__ __device__ bool     is_final() const;
//       __host__ __device__ bool     success() const;
//       __host__            bool     init(const double *params, int n);        // the prototype from constructor parameters
//   };
//
// Randomness: tw::env_draw(seed, episode, index) -> four 32-bit words (Philox4x32-10 on stream 6).  The environment
// chooses its own `index` values, e.g. the draw number in reset() and (t << 8) | k in step(); tw::u32_below(word, n) gives an
// integer in [0, n), tw::u32_to_unit(word) a float in [0, 1).  Everything a method reads must be in the struct: no pointers to host
// memory, no globals, no virtual functions.  step() in particular depends on the struct and the action ALONE -- a step-time draw is
// keyed by what the struct holds, e.g. its own step counter: the search kernel (TW_DEVICE_ENV_SEARCH below) re-derives a tree
// node's state by replaying the actions from the move's root, where the host path keeps a clone per node, and the two must agree.  An id outside [0, obs_size()) fails the collect ("index out of bounds: obs id ..."), an
// episode that has not ended within the collect's max_records_per_episode records fails it too -- as on the host-stepped path.  A
// collect whose max_records_per_episode is above 1,820 (what the finalize step's LDS tile holds) runs on the host-stepped path.
// More episodes than the GPU holds columns at once (the module's own occupancy x the compute units x 16): the PPO collect and the plain
// evaluate run on a persistent grid whose columns take the next episode from a device-side queue -- reset() is then called again on a
// fresh clone of the prototype, from the same single place in the kernel; the bytes are those of one column per episode.
// solve (collector.solve / tw_solve_device_env: best of N attempts from the object's CURRENT state, the played actions back) is one launch
// of the evaluate kernel -- of the search kernel with num_mcts_searches > 0 -- that skips reset(): every attempt starts from a copy of the
// struct as the caller holds it, which is not modified.  Nothing is asked of the struct for it beyond the methods above.
// A struct that holds instances of several sizes may add `int n_obs() const`, 1..N_OBS and CONSTANT for the object's lifetime (the
// library reads it once, from the prototype): observe() then writes that many ids.
// Observations of VARIABLE length (the reference's Env::observe returns a Vec of any length and its EmbeddingBag adds however many
// vectors it is given): define observe_n() instead of observe().  It writes the ids of the current state -- at most N_OBS (n_obs()) of
// them, WHATEVER it returns, in the order the embedding adds them -- and returns their number; 0 is legal (the embedding is then its
// bias).  Write ids[i] with indices the compiler can resolve after unrolling (slot i = the i-th id, not ids[k++]), or the array goes to
// scratch memory.  So does a struct that holds an array it indexes at run time: that is no build error, the kernels then keep the
// state in scratch memory, and tests/test_gpu_device_env_matrix.py holds such structs (128 bytes and 1 KiB) to the host path's BYTES,
// not to a speed.  A count outside 0..N_OBS fails the collect ("observation of %u ids, at most %u") without anything being indexed
// by it.  The collected obs field is then two-byte ids [records][N_OBS], a record's ids first and 0xFFFF in the slots it leaves free
// (2 x N_OBS bytes per record however short the observation); the module's host vtable carries observe_n, and observe (the ids,
// then -1) for hosts that only know the fixed-length member.
// More than four actions: `#define TW_DEVICE_ENV_WIDE` before this header (build_device_env(..., wide=True) emits it) lifts the bound
// to 1..31, tw_env_vtable's own and what the one mask word holds; masks() stays a uint32_t, bit i < NUM_ACTIONS.  The SAME two kernels
// then stream over the actions: the action head's outputs stay in LDS, a twist of the actions is an LDS index, the Gumbel words are
// those of the host path (draw t | ((i >> 2) << 24), word i & 3), and the masked logits go to a workspace array of their own
// (EnvRolloutArgs::lgw, NUM_ACTIONS floats per record).  Every addition is an `if constexpr (A > 4)`: a struct of at most four actions
// compiles to the same kernels with or without the define.  TW_DEVICE_ENV_SEARCH does not take such a struct (the search kernel keeps
// four children per node there); TW_DEVICE_ENV_WIDE_SEARCH (at the end of this file, build_device_env(..., wide_search=True)) does:
// self-play and MCTS-guided evaluate of 5..31 actions then run in the same mcts_env_kernel, which loops over a node's children and keeps
// a column's probabilities in LDS, byte-equal to the host-stepped path.  A module built with the define alone (wide=True) has no search
// kernel: its AZCollector.collect and evaluate with MCTS run host-stepped over the module's vtable.
// Reduced precision: `#define TW_DEVICE_ENV_FP16` before this header (build_device_env(..., fp16=True) emits it) adds
// rollout_env16_kernel -- the same step loop over EngineV16 (twisterl_amd/csrc/tw_engine_generic16.hpp: every Linear on
// v_mfma_f32_16x16x32_f16, DESIGN.md §2 "Forward, f16-input mode") -- and the kernel that packs its binary16 weight image at the start
// of every collect; the descriptor's launch_rollout16 / groups_per_cu16 are then set and PPOCollector(precision="fp16").collect runs
// on the device for any generic policy.  Everything outside the forward is the f32 kernel's instruction sequence: given the same
// actions, states, ids, masks, rewards and draws are bit-equal to it.  Nothing is asked of the struct for it.  The define composes
// with every form above and below; without it both members are null and the module holds exactly the other kernels.
// `#define TW_DEVICE_ENV_FP16_SOLVE` (build_device_env(..., fp16_solve=True); it implies TW_DEVICE_ENV_FP16) adds solve_env16_kernel,
// the evaluate loop over the same EngineV16 and the same image: collector.evaluate / collector.solve with precision="fp16" and
// num_mcts_searches == 0 then run on the device for any generic policy, launched by the descriptor's launch_solve when its arguments
// carry an image (EnvSolveArgs::image), its occupancy behind groups_per_cu(3, ...) -- the descriptor itself does not grow.  Again
// everything outside the forward is the f32 kernel's sequence, and nothing is asked of the struct.  A module built with
// TW_DEVICE_ENV_FP16 alone holds exactly the kernels it held.
// `#define TW_DEVICE_ENV_FP16_SEARCH` (build_device_env(..., fp16_search=True); it implies TW_DEVICE_ENV_FP16 and belongs with
// TW_DEVICE_ENV_SEARCH or TW_DEVICE_ENV_WIDE_SEARCH) adds mcts_env16_kernel, the search loop over EngineV16 and the same image:
// AZCollector(precision="fp16").collect and collector.evaluate / collector.solve with precision="fp16" and num_mcts_searches > 0 then
// run on the device, launched by the descriptor's launch_search when its arguments carry an image (EnvMctsArgs::image), its occupancy
// and the capability query behind groups_per_cu(4, ...).  Everything behind the heads -- the soft-max, the tree, the draws -- is the
// f32 kernel's text.  Without the define the search kernel is f32 alone: self-play and MCTS-guided evaluate and solve in another
// precision answer "f32 only".
// Split precision: `#define TW_DEVICE_ENV_FP16X2` (build_device_env(..., fp16x2=True); it implies TW_DEVICE_ENV_FP16) adds
// rollout_env16x2_kernel -- the same step loop over EngineV16x2 (twisterl_amd/csrc/tw_engine_generic16x2.hpp: every Linear operand
// split into two binary16 terms, three products per k-group on v_mfma_f32_16x16x32_f16, DESIGN.md §2 "Forward, split-f16 mode, generic
// stacks") -- and the kernel that packs its two-plane weight image at the start of every collect:
// PPOCollector(precision="fp16x2").collect then runs on the device for any generic policy, f32 answers within the split mode's
// a-priori bound.  The descriptor does not grow: the request travels to launch_rollout16 as bit 63 of EnvRollout16Args::image.halves,
// the kernel's occupancy and the capability query are behind groups_per_cu(5, ...).  A weight or an activation of 4095 or more has no
// finite pair of terms; the kernels flag it and the library returns the f32 kernel's collect instead.  Without the define a module
// holds exactly the kernels it held.
// `#define TW_DEVICE_ENV_FP16X2_SOLVE` (build_device_env(..., fp16x2_solve=True); it implies TW_DEVICE_ENV_FP16X2) adds
// solve_env16x2_kernel, the evaluate loop over the same EngineV16x2 and the same two-plane image (twisterl_amd/csrc/tw_solve_env16x2.hpp):
// collector.evaluate / collector.solve with precision="fp16x2" and num_mcts_searches == 0 then run on the device for any generic
// policy, launched by the descriptor's launch_solve when its image carries the request bit (bit 63 of EnvSolveArgs::image.halves), its
// occupancy and the capability query behind groups_per_cu(6, ...) -- again the descriptor does not grow.  Out of range, the library
// returns the f32 kernel's answer, as for the collect.  The search kernel has no split form: self-play and MCTS-guided evaluate /
// solve with precision="fp16x2" answer "f32 only" (tw_mcts_env.hpp includes the search loop exactly twice, and a test pins that).
// A module built with TW_DEVICE_ENV_FP16X2 alone holds exactly the kernels it held.
// The reference's default policy: every kernel above runs EngineV, which takes a "generic stack".  A policy of ONE common Linear of
// 32 / 64 / 128 / 256 units with linear heads, an embedding size that is a multiple of 32 and obs_size <= 256 -- what the reference's
// trainer builds unless it is told otherwise, BasicPolicy(common_layers=(256,)) -- gets the image of the Puzzle engines from
// tw_policy_create instead (the "MFMA shape"), without EngineV's layer table, and a device environment under it runs host-stepped over
// the module's vtable.  `#define TW_DEVICE_ENV_BASIC` before this header (build_device_env(..., basic=True) emits it; it composes
// with every form and flag above) adds pack_basic_view_kernel (twisterl_amd/csrc/tw_env_basic_view.hpp): the module's f32 launchers
// then also take a VIEW of such a policy, whose three layers that kernel packs -- table, padded biases, matrix-core images -- from the
// policy's live natural-layout arrays into the call's workspace in front of every launch, and PPO collect, evaluate and solve, and with
// a search form self-play and the MCTS-guided calls, run in the same kernels, byte-equal to the host-stepped path.  The descriptor and
// the argument structs do not grow: the capability query is groups_per_cu(7, 0, nullptr) (DeviceEnv.basic), asked before a view is
// formed, and a view is told by PolicyDev::generic with a non-zero PolicyDev::hidden.  fp16 / fp16x2 under such a policy still answer
// "f32 only".  Without the define a module holds exactly the kernels it held, and behaves as it did.
#pragma once

#if defined(TW_DEVICE_ENV_FP16_SOLVE) && !defined(TW_DEVICE_ENV_FP16)
#define TW_DEVICE_ENV_FP16
#endif
#if defined(TW_DEVICE_ENV_FP16_SEARCH) && !defined(TW_DEVICE_ENV_FP16)
#define TW_DEVICE_ENV_FP16
#endif
#if defined(TW_DEVICE_ENV_FP16X2_SOLVE) && !defined(TW_DEVICE_ENV_FP16X2)
#define TW_DEVICE_ENV_FP16X2
#endif
#if defined(TW_DEVICE_ENV_FP16X2) && !defined(TW_DEVICE_ENV_FP16)
#define TW_DEVICE_ENV_FP16
#endif

#include "twisterl_hip.h"
#include "tw_rollout_env.hpp"
#include "tw_mcts_env.hpp"

#include <new>
#include <type_traits>

namespace tw {

template <class T>
struct DeviceEnvModule {
    static_assert(std::is_trivially_copyable<T>::value, "twisterl device environment: the struct must be trivially copyable (the kernels clone it by value)");
    static_assert(std::is_default_constructible<T>::value, "twisterl device environment: the struct must be default-constructible (init() fills a default-constructed one)");
    static_assert(sizeof(T) <= 1024, "twisterl device environment: the struct must be at most 1 KiB (it lives in registers on the device)");
#ifdef TW_DEVICE_ENV_WIDE
    static_assert(T::NUM_ACTIONS >= 1 && T::NUM_ACTIONS <= 31, "twisterl device environment: NUM_ACTIONS must be 1..31 (tw_env_vtable's limit; masks() is one 32-bit word)");
#else
    static_assert(T::NUM_ACTIONS >= 1 && T::NUM_ACTIONS <= 4, "twisterl device environment: NUM_ACTIONS must be 1..4 (EngineV's head has four action columns); 5..31: define TW_DEVICE_ENV_WIDE / build_device_env(wide=True)");
#endif
    static_assert(T::N_OBS >= 1 && T::N_OBS <= 64, "twisterl device environment: N_OBS must be 1..64");
    static constexpr bool VAR_OBS = EnvHasObserveN<T>::value;
    static_assert(VAR_OBS || EnvHasObserve<T>::value, "twisterl device environment: the struct needs `void observe(int *ids) const`, or `int observe_n(int *ids) const` for observations of variable length");
    static constexpr int A = T::NUM_ACTIONS, NO = T::N_OBS;

    // tw_env_vtable over T (the host-stepped collectors, and solve for what the kernels do not take, run the same code on the CPU)
    static void *clone(void *e) { return new (std::nothrow) T(*static_cast<const T *>(e)); }
    static void destroy(void *e) { delete static_cast<T *>(e); }
    static void reset(void *e, uint64_t seed, uint64_t episode) { static_cast<T *>(e)->reset(seed, episode); }
    static void step(void *e, uint32_t action) { static_cast<T *>(e)->step((int)action); }
    static void observe(void *e, int32_t *out)
    {
        if constexpr (VAR_OBS) {                                      // for a host that only knows observe(): the ids, then -1 = no id
            const uint32_t k = observe_n(e, out, (uint32_t)n_obs_of(e));
            for (int i = (int)k < 0 ? 0 : (int)k, n = n_obs_of(e); i < n; ++i) out[i] = -1;
        } else if constexpr (EnvHasObserve<T>::value) {
            int ids[NO];
            static_cast<const T *>(e)->observe(ids);
            for (int i = 0, n = n_obs_of(e); i < n; ++i) out[i] = (int32_t)ids[i];
        }
    }
    // tw_env_vtable::observe_n: at most `cap` ids are written; the count is returned as the struct gave it (the caller holds it against cap)
    static uint32_t observe_n(void *e, int32_t *out, uint32_t cap)
    {
        int ids[NO] = {};
        int k = 0;
        if constexpr (VAR_OBS) k = static_cast<const T *>(e)->observe_n(ids);
        for (int i = 0; i < k && i < NO && (uint32_t)i < cap; ++i) out[i] = (int32_t)ids[i];
        return (uint32_t)k;
    }
    static void masks(void *e, uint8_t *out)
    {
        const uint32_t b = static_cast<const T *>(e)->masks();
        for (int i = 0; i < A; ++i) out[i] = (uint8_t)((b >> i) & 1u);
    }
    static float reward(void *e) { return static_cast<const T *>(e)->reward(); }
    static int is_final(void *e) { return static_cast<const T *>(e)->is_final() ? 1 : 0; }
    static int success(void *e) { return static_cast<const T *>(e)->success() ? 1 : 0; }

    static void *create(const double *params, int n)
    {
        T *t = new (std::nothrow) T();
        if (t && !t->init(params, n)) { delete t; t = nullptr; }
        return t;
    }
    static int get_difficulty(const void *e) { return static_cast<const T *>(e)->difficulty(); }
    static void set_difficulty(void *e, int d) { static_cast<T *>(e)->set_difficulty(d); }
    static int obs_size(const void *e) { return static_cast<const T *>(e)->obs_size(); }
    static int n_obs_of(const void *e) { return env_n_obs(*static_cast<const T *>(e)); }
    static void fill_vtable(tw_env_vtable *v)
    {
        *v = tw_env_vtable{};
        v->num_actions = (uint32_t)A; v->n_obs = (uint32_t)NO;
        v->clone = clone; v->destroy = destroy; v->reset = reset; v->step = step; v->observe = observe; v->masks = masks;
        v->reward = reward; v->is_final = is_final; v->success = success;
        if (VAR_OBS) v->observe_n = observe_n;
    }

    static const tw_device_env *descriptor(const char *type_name, decltype(tw_device_env::launch_search) search = nullptr,
                                           decltype(tw_device_env::groups_per_cu) groups = groups_per_cu_env<T>)
    {
        static const tw_device_env d = [type_name, search, groups]() {
            tw_device_env x{};
            tw_device_env_layout(x.layout);
            x.num_actions = (uint32_t)A; x.n_obs = (uint32_t)NO; x.state_bytes = (uint32_t)sizeof(T); x.engine_nc = (uint32_t)env_engine_nc(NO);
            x.type_name = type_name;
            x.launch_rollout = launch_rollout_env<T>; x.launch_solve = launch_solve_env<T>;
            x.create = create; x.get_difficulty = get_difficulty; x.set_difficulty = set_difficulty; x.obs_size = obs_size; x.n_obs_of = n_obs_of;
            x.fill_vtable = fill_vtable;
            x.launch_search = search;                                     // (TW_DEVICE_ENV: null, and no third kernel in the module)
            x.groups_per_cu = groups;                                     // (occupancy of the kernels THIS module holds)
#ifdef TW_DEVICE_ENV_FP16
            x.launch_rollout16 = launch_rollout_env16<T>;                 // (else null, and the module holds neither f16 kernel)
            x.groups_per_cu16 = groups_per_cu_env16<T>;
#endif
            return x;
        }();
        return &d;
    }
};

}  // namespace tw

// Instantiates the rollout and evaluate kernels, their launchers and the host adapter of `Type`, and exports
// `extern "C" const tw_device_env *tw_device_env_<name>(void)`.  Once per module.
#define TW_DEVICE_ENV(Type, name)                                                                           \
    extern "C" __attribute__((visibility("default"))) const tw_device_env *tw_device_env_##name(void)      \
    {                                                                                                       \
        return ::tw::DeviceEnvModule<Type>::descriptor(#Type);                                              \
    }

// The same, and the module also holds mcts_env_kernel (twisterl_amd/csrc/tw_mcts_env.hpp) with its launcher: AZCollector.collect and
// evaluate with num_mcts_searches > 0 then run on the device too.  That kernel keeps TWO copies of the struct in a lane's registers
// (the episode's state and the one that walks the tree), so the struct may have at most TW_DEVICE_ENV_SEARCH_MAX_BYTES = 128 bytes
// here.  build_device_env(..., search=True) emits this form.
#define TW_DEVICE_ENV_SEARCH_MAX_BYTES 128
#define TW_DEVICE_ENV_SEARCH(Type, name)                                                                    \
    static_assert(sizeof(Type) <= TW_DEVICE_ENV_SEARCH_MAX_BYTES,                                           \
                  "twisterl device environment: TW_DEVICE_ENV_SEARCH needs a struct of at most 128 bytes (the search kernel keeps two copies in registers)"); \
    static_assert(Type::NUM_ACTIONS <= 4,                                                                   \
                  "twisterl device environment: TW_DEVICE_ENV_SEARCH needs NUM_ACTIONS 1..4 (the search kernel keeps four children per node); with 5..31 actions use TW_DEVICE_ENV_WIDE_SEARCH / build_device_env(wide_search=True)"); \
    extern "C" __attribute__((visibility("default"))) const tw_device_env *tw_device_env_##name(void)      \
    {                                                                                                       \
        return ::tw::DeviceEnvModule<Type>::descriptor(#Type, ::tw::launch_mcts_env<Type>,                  \
                                                       ::tw::groups_per_cu_search_env<Type>);               \
    }

// The search form for 1..31 actions: needs `#define TW_DEVICE_ENV_WIDE` in front of this header (build_device_env(..., wide_search=True)
// emits both).  The same mcts_env_kernel: with more than four actions it walks a node's children in a loop and keeps its column's
// probabilities in LDS; a struct of at most four actions compiles to the kernels of TW_DEVICE_ENV_SEARCH.  The 128-byte bound stays.
#ifdef TW_DEVICE_ENV_WIDE
#define TW_DEVICE_ENV_WIDE_SEARCH(Type, name)                                                               \
    static_assert(sizeof(Type) <= TW_DEVICE_ENV_SEARCH_MAX_BYTES,                                           \
                  "twisterl device environment: TW_DEVICE_ENV_WIDE_SEARCH needs a struct of at most 128 bytes (the search kernel keeps two copies in registers)"); \
    extern "C" __attribute__((visibility("default"))) const tw_device_env *tw_device_env_##name(void)      \
    {                                                                                                       \
        return ::tw::DeviceEnvModule<Type>::descriptor(#Type, ::tw::launch_mcts_env<Type>,                  \
                                                       ::tw::groups_per_cu_search_env<Type>);               \
    }
#else
#define TW_DEVICE_ENV_WIDE_SEARCH(Type, name)                                                               \
    static_assert(sizeof(Type) == 0, "twisterl device environment: TW_DEVICE_ENV_WIDE_SEARCH needs `#define TW_DEVICE_ENV_WIDE` in front of twisterl_device_env.hpp / build_device_env(wide_search=True)");
#endif
