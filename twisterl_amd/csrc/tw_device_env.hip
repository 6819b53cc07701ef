// tw_device_env.hip -- PPO collect and evaluate of a user-written environment ON THE DEVICE (include/twisterl_device_env.hpp).
//
// A device-environment module (twisterl_amd.build.build_device_env) holds the environment's kernels -- rollout_env_kernel /
// solve_env_kernel of tw_rollout_env.hpp instantiated over the user's struct -- their launchers and a host adapter.  Everything
// else is here: the checks, the workspace, the scan, the error messages.  The result is built by collect_tail (tw_api.hip), the one
// ending of every device collector: the ids always have their own array here (CollectTail::obs16, written out as one or two bytes per
// id), and an environment with other than four actions has its logits narrowed (A < 4) or moved from a wide array (A > 4).  The two
// small kernels that serves, compact_env_obs8_kernel and narrow_logits_kernel, live here behind launch_compact_obs8 / launch_narrow_logits.
// What the kernels do not take runs on the host-stepped path (tw_env_generic.hip) over the module's own vtable, the same code on
// the CPU: a policy of the MFMA shape (its image has no EngineV layers -- unless the module was built with TW_DEVICE_ENV_BASIC: its
// launchers then pack those layers from the policy's live natural-layout arrays into the call's workspace in front of every f32 launch,
// and the call runs in the same kernels under a view of the policy, kernel_policy() below; fp16 / fp16x2 under such a policy stay
// with the host path's "f32 only"), another precision (that path's "f32 only" error; but a PPO
// collect with precision fp16 of a module built with TW_DEVICE_ENV_FP16 runs in rollout_env16_kernel over EngineV16, its binary16
// weight image packed into the collect's workspace by the module's launcher in front of every rollout, and evaluate / solve without
// MCTS of a module built with TW_DEVICE_ENV_FP16_SOLVE run likewise in solve_env16_kernel, self-play and evaluate / solve WITH MCTS of
// one built with TW_DEVICE_ENV_FP16_SEARCH in mcts_env16_kernel; a PPO collect with precision fp16x2 of a module built with
// TW_DEVICE_ENV_FP16X2 runs in rollout_env16x2_kernel over EngineV16x2, its split image packed likewise, and runs again in the f32
// kernel when an operand left the split terms' range, and evaluate / solve without MCTS of one built with
// TW_DEVICE_ENV_FP16X2_SOLVE run likewise in solve_env16x2_kernel, with the same f32 run out of range), and -- for
// a module built without TW_DEVICE_ENV_SEARCH / TW_DEVICE_ENV_WIDE_SEARCH, whose descriptor has no search launcher -- self-play,
// evaluate and solve with MCTS.  With the launcher those two run in mcts_env_kernel (tw_mcts_env.hpp), for
// 1..4 actions and (TW_DEVICE_ENV_WIDE_SEARCH) for 5..31, which lives in the module
// alone: tw_az_collect_device_env, and tw_evaluate_device_env / tw_solve_device_env with num_mcts_searches > 0.  The result is an
// ordinary tw_collected, byte-equal to tw_ppo_collect_env / tw_az_collect_env over the same vtable.  solve (tw_solve_device_env) is
// evaluate's body started from the prototype as it is, with the played moves kept: attempts_device_env below.
#include "tw_rollout_env.hpp"

#include <cstring>
#include <vector>

using namespace tw;

namespace {

// obs ids of the padded trajectories -> the compact one-byte result (environments with at most 256 ids; one wave per episode)
__global__ void __launch_bounds__(256) compact_env_obs8_kernel(const uint16_t *obs16, const uint32_t *ep_len, const uint64_t *ep_start, uint64_t E,
                                                               int t_pad, int n_obs, uint8_t *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t e = (uint64_t)blockIdx.x * 4 + wave; e < E; e += (uint64_t)gridDim.x * 4) {
        const uint64_t n = (uint64_t)ep_len[e] * (uint64_t)n_obs;
        const uint16_t *src = obs16 + e * (uint64_t)t_pad * (uint64_t)n_obs;
        uint8_t *dst = out + ep_start[e] * (uint64_t)n_obs;
        for (uint64_t i = lane; i < n; i += 64) dst[i] = (uint8_t)src[i];
    }
}

// logits of the compact records, four per record -> the environment's A < 4 columns
__global__ void __launch_bounds__(256) narrow_logits_kernel(const float *lg4, uint64_t n, int A, float *out)
{
    const uint64_t total = n * (uint64_t)A;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / (uint64_t)A, c = i - r * (uint64_t)A;
        out[i] = lg4[r * 4 + c];
    }
}

unsigned grid_for(uint64_t items, uint64_t per_block)
{
    uint64_t b = (items + per_block - 1) / per_block;
    if (b > 256ull * 16) b = 256ull * 16;
    return (unsigned)(b ? b : 1);
}

int check_descriptor(const tw_device_env *d, const void *proto, size_t proto_bytes, const char *who)
{
    if (!d || !proto) { set_error("%s: null argument", who); return TW_ERR_INVALID; }
    uint32_t mine[TW_DEVICE_ENV_LAYOUT_WORDS];
    tw_device_env_layout(mine);
    if (memcmp(d->layout, mine, sizeof(mine)) != 0) {
        set_error("%s: the device environment module was built against another library layout (module: tag %08x ABI %u, %u/%u/%u/%u/%u/%u bytes; "
                  "this library: tag %08x ABI %u, %u/%u/%u/%u/%u/%u bytes) -- rebuild it with twisterl_amd.build.build_device_env", who,
                  d->layout[0], d->layout[1], d->layout[2], d->layout[3], d->layout[4], d->layout[5], d->layout[6], d->layout[7],
                  mine[0], mine[1], mine[2], mine[3], mine[4], mine[5], mine[6], mine[7]);
        return TW_ERR_INVALID;
    }
    if (!d->launch_rollout || !d->launch_solve || !d->groups_per_cu || !d->create || !d->get_difficulty || !d->set_difficulty || !d->obs_size || !d->n_obs_of || !d->fill_vtable) {
        set_error("%s: the device environment descriptor lacks a function", who); return TW_ERR_INVALID;
    }
    if (d->num_actions < 1 || d->num_actions > 31 || d->n_obs < 1 || d->n_obs > 64 || d->engine_nc != (uint32_t)env_engine_nc((int)d->n_obs)) {
        set_error("%s: descriptor with %u actions, %u obs ids, %u engine columns", who, d->num_actions, d->n_obs, d->engine_nc); return TW_ERR_INVALID;
    }
    if (proto_bytes != d->state_bytes) {
        set_error("%s: the prototype has %zu bytes, the module's environment %u", who, proto_bytes, d->state_bytes); return TW_ERR_INVALID;
    }
    const int os = d->obs_size(proto), no = d->n_obs_of(proto);
    if (os < 1 || os > 65535) { set_error("%s: obs_size() is %d (1..65535)", who, os); return TW_ERR_INVALID; }
    if (no < 1 || no > (int)d->n_obs) { set_error("%s: n_obs() is %d (1..N_OBS = %u)", who, no, d->n_obs); return TW_ERR_INVALID; }
    return TW_OK;
}

tw_env_vtable host_table(const tw_device_env *d, const void *proto)
{
    tw_env_vtable vt{};
    d->fill_vtable(&vt);
    vt.prototype = const_cast<void *>(proto);          // the collectors clone it and never write to it
    vt.obs_size = (uint32_t)d->obs_size(proto);
    vt.n_obs = (uint32_t)d->n_obs_of(proto);
    return vt;
}

size_t engine_lds_bytes(uint32_t nc, const PolicyDev &p)
{
    switch (nc) {
        case 4:  return EngineV<4>::lds_floats(p) * sizeof(float);
        case 9:  return EngineV<9>::lds_floats(p) * sizeof(float);
        case 16: return EngineV<16>::lds_floats(p) * sizeof(float);
        case 25: return EngineV<25>::lds_floats(p) * sizeof(float);
        case 36: return EngineV<36>::lds_floats(p) * sizeof(float);
        default: return EngineV<64>::lds_floats(p) * sizeof(float);
    }
}

// EngineV16 (tw_engine_generic16.hpp): the f16 rollout kernel of a module built with TW_DEVICE_ENV_FP16
size_t engine16_lds_bytes(uint32_t nc, const PolicyDev &p)
{
    switch (nc) {
        case 4:  return EngineV16<4>::lds_bytes(p);
        case 9:  return EngineV16<9>::lds_bytes(p);
        case 16: return EngineV16<16>::lds_bytes(p);
        case 25: return EngineV16<25>::lds_bytes(p);
        case 36: return EngineV16<36>::lds_bytes(p);
        default: return EngineV16<64>::lds_bytes(p);
    }
}

// EngineV16x2 (tw_engine_generic16x2.hpp): the split-f16 rollout kernel of a module built with TW_DEVICE_ENV_FP16X2
size_t engine16x2_lds_bytes(uint32_t nc, const PolicyDev &p)
{
    switch (nc) {
        case 4:  return EngineV16x2<4>::lds_bytes(p);
        case 9:  return EngineV16x2<9>::lds_bytes(p);
        case 16: return EngineV16x2<16>::lds_bytes(p);
        case 25: return EngineV16x2<25>::lds_bytes(p);
        case 36: return EngineV16x2<36>::lds_bytes(p);
        default: return EngineV16x2<64>::lds_bytes(p);
    }
}

// the checks of the host path (tw_env_generic.hip), with its messages
int check_env_policy(const tw_env_vtable &vt, const PolicyDev *pd)
{
    if ((int)vt.num_actions != pd->n_actions) { set_error("environment has %u actions, policy has %d (at most 31)", vt.num_actions, pd->n_actions); return TW_ERR_INVALID; }
    if ((int)vt.obs_size != pd->obs_size) { set_error("index out of bounds: policy obs_size %d != environment obs ids %u", pd->obs_size, vt.obs_size); return TW_ERR_INVALID; }
    return TW_OK;
}

// The grid of a module's rollout (0), solve (1), f16 solve (3), split-f16 rollout (5), split-f16 solve (6) or f16 rollout (ENV_KERNEL_ROLLOUT16: tw_device_env::groups_per_cu16) kernel over
// `columns` episodes or attempts.  (The search kernel, 2, has no persistent
// form: a first one faulted on the device and was taken out again -- DESIGN.md §8.)  As many workgroups
// as the kernel's own occupancy puts on the CUs that reserve_cus leaves are resident at once (TW_OPT_ENV_RESIDENT_GROUPS > 0 caps
// their total: the test hook); more columns than those hold run on a PERSISTENT grid of that size whose columns take the next
// episode from a 32-bit counter (EnvRolloutArgs::queue), which starts at the number of slots and is taken once more by every slot that
// finds it empty: columns + slots must fit 32 bits.  Otherwise -- and with TW_OPT_NO_PERSIST -- one workgroup per 16 columns, as ever.
struct EnvGrid { uint64_t blocks; bool persist; };
constexpr int ENV_KERNEL_ROLLOUT16 = 16;
int env_grid(const tw_device_env *d, int kernel, size_t lds_bytes, uint64_t columns, uint32_t reserve_cus, EnvGrid *g)
{
    g->blocks = (columns + GEN_COLS - 1) / GEN_COLS; g->persist = false;
    const LaunchOptions o = launch_options();
    if (o.no_persist) return TW_OK;
    int per_cu = 0;
    const int e = kernel == ENV_KERNEL_ROLLOUT16 ? d->groups_per_cu16(lds_bytes, &per_cu) : d->groups_per_cu(kernel, lds_bytes, &per_cu);
    if (e != (int)hipSuccess) return hip_fail((hipError_t)e, "device environment occupancy query", __FILE__, __LINE__);
    if (per_cu < 1) { set_error("device environment: the kernel does not fit a compute unit with %zu bytes of LDS", lds_bytes); return TW_ERR_UNSUPPORTED; }
    const uint64_t cus = (uint64_t)device_cus(), keep = reserve_cus < cus - 1 ? reserve_cus : cus - 1;   // reserve_cus CUs stay free (RCCL beside the grid)
    uint64_t groups = (uint64_t)per_cu * (cus - keep);
    if (o.env_resident_groups > 0 && (uint64_t)o.env_resident_groups < groups) groups = (uint64_t)o.env_resident_groups;
    const uint64_t slots = groups * GEN_COLS;
    if (columns > slots && columns + slots <= 0xffffffffull) { g->blocks = groups; g->persist = true; }
    return TW_OK;
}

// launch_finalize_az keeps two floats per record of an episode for each of its four waves in 64 KiB of LDS
constexpr uint32_t FINALIZE_AZ_MAX_T_PAD = 64 * 1024 / (4 * 2 * sizeof(float));

// what mcts_env_kernel takes of a search: the tree fits 31-bit node indices and a column's evaluation ordinal 32 bits
bool search_fits(uint32_t A, uint32_t S, uint32_t MED, uint64_t moves, uint64_t *node_cap)
{
    const uint64_t per_move = (uint64_t)S * (MED ? MED : 1u);
    *node_cap = env_mcts_node_cap(A, S, MED);
    return per_move <= 0x0fffffffull && *node_cap <= 0x7fffffffull && (per_move + 1) * moves <= 0xffffffffull;
}

// The error the host-stepped path reports for the columns mcts_env_kernel ended (EnvMctsArgs::col_err).  That path evaluates one
// state per live episode per round and checks the ids as it stages them, episode by episode: the first bad id (count) is the one
// with the smallest evaluation ordinal, then the smallest column.  It notices an overlong episode only before the NEXT round, so a
// bad id wins exactly when its ordinal is below the evaluations every overlong column had consumed.  Returns true for a bad id.
bool first_search_error(const std::vector<uint32_t> &ce, uint64_t n, uint32_t NO, int obs_size)
{
    uint64_t bad = n;
    uint32_t over = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t kind = ce[4 * i], ord = ce[4 * i + 1];
        if ((kind == 1u || kind == 2u) && (bad == n || ord < ce[4 * bad + 1])) bad = i;
        else if (kind == 3u && ord < over) over = ord;
    }
    if (bad == n || ce[4 * bad + 1] >= over) return false;
    if (ce[4 * bad] == 2u) set_error("observation of %u ids, at most %u", ce[4 * bad + 2], NO);
    else set_error("index out of bounds: obs id %d, obs_size %d", (int)ce[4 * bad + 2], obs_size);
    return true;
}

// launch_search answered hipErrorInvalidValue: it refuses arguments it was not compiled for, above all an EnvMctsArgs of another size
// (struct_bytes; the descriptor's layout words do not cover that struct)
int search_launch_refused(const char *who)
{
    set_error("%s: the module's search launcher refused the arguments (it was compiled against another EnvMctsArgs): rebuild the module", who);
    return TW_ERR_INVALID;
}

// What EngineV16 takes of a policy: a generic stack with both heads, at most GEN16_MAX_LAYERS layers (the fp16 collect's own rule)
bool engine16_takes(const PolicyDev *pd)
{
    return pd->generic && pd->n_action >= 1 && pd->n_value >= 1 && pd->n_common + pd->n_action + pd->n_value <= GEN16_MAX_LAYERS;
}

// index of rollout_env16x2_kernel for tw_device_env::groups_per_cu (a module built with TW_DEVICE_ENV_FP16X2)
constexpr int ENV_KERNEL_ROLLOUT16X2 = 5;

// index of mcts_env16_kernel for tw_device_env::groups_per_cu (a module built with TW_DEVICE_ENV_FP16_SEARCH)
constexpr int ENV_KERNEL_SEARCH16 = 4;

// precision="fp16" of self-play and of MCTS-guided evaluate / solve: mcts_env16_kernel over EngineV16, when the module holds it (the
// capability query: kernel 4 with a null result, answered without the HIP runtime) and EngineV16 takes the policy
bool search_f16(const tw_device_env *env, const PolicyDev *pd, uint32_t precision)
{
    return precision == TW_PREC_F16 && env->launch_search && engine16_takes(pd) && env->groups_per_cu(ENV_KERNEL_SEARCH16, 0, nullptr) == (int)hipSuccess;
}

// the size of the f16 weight image of a generic policy: the layout function the pack kernel and the engine index with
// (tw_engine_generic16.hpp) over the layer table's widths, which live on the device and are read on the call's stream `s`
int gen16_image_size(const PolicyDev *pd, hipStream_t s, size_t *halves)
{
    const int n_layers = pd->n_common + pd->n_action + pd->n_value;
    std::vector<LayerDev> layers((size_t)n_layers);
    TW_HIP(hipMemcpyAsync(layers.data(), pd->layers, (size_t)n_layers * sizeof(LayerDev), hipMemcpyDeviceToHost, s));
    TW_HIP(hipStreamSynchronize(s));
    *halves = gen16_image_halves((uint32_t)pd->obs_size, (uint32_t)pd->emb, layers.data(), n_layers);
    return TW_OK;
}

// The policy the environment kernels run.  They run EngineV, which wants a layer table: a generic stack has one, a policy of the MFMA
// shape -- the reference's default, one common layer -- does not, and goes to the host-stepped path.  But a module built with
// TW_DEVICE_ENV_BASIC holds pack_basic_view_kernel (tw_env_basic_view.hpp), which builds that table and the three layers' images from
// the policy's live natural-layout arrays, in a block of the call's workspace, in front of every launch: for such a module, in f32, the
// answer is a VIEW of the policy (*view: generic = 1, one layer per stack, the same embedding rows and twist tables; `layers` is set by
// the caller once the workspace is reserved, see launch_policy()), and the call goes down the device path with it unchanged.  The
// capability query -- kernel 7 with a null result, answered without the HIP runtime -- is asked BEFORE a view is formed, so a module
// built without the define never sees one.  Other precisions keep the host path's "f32 only" under such a policy.
const PolicyDev *kernel_policy(const tw_device_env *env, const PolicyDev *pd, uint32_t precision, PolicyDev *view)
{
    if (precision != TW_PREC_F32_EXACT || !basic_view_source(*pd) || env->groups_per_cu(ENV_KERNEL_PACK_BASIC, 0, nullptr) != (int)hipSuccess) return pd;
    *view = basic_view(*pd, nullptr);
    return view;
}

// bytes of a view's block behind a call's carve (any other policy: none)
size_t basic_block_bytes(const PolicyDev *pd)
{
    return is_basic_view(*pd) ? (size_t)basic_view_layout((uint32_t)pd->emb, (uint32_t)pd->hidden, (uint32_t)pd->n_actions).bytes : 0;
}

// the policy a launcher is handed: *pd, a view with its block at `block`
PolicyDev launch_policy(const PolicyDev *pd, const void *block)
{
    PolicyDev p = *pd;
    if (is_basic_view(p)) p.layers = reinterpret_cast<const LayerDev *>(block);
    return p;
}

}  // namespace

int tw::launch_compact_obs8(const uint16_t *obs16, const uint32_t *ep_len, const uint64_t *ep_start, uint64_t E, int t_pad, int n_obs,
                            uint8_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(compact_env_obs8_kernel, dim3(grid_for(E, 4)), dim3(256), 0, s, obs16, ep_len, ep_start, E, t_pad, n_obs, out);
    TW_HIP(hipGetLastError());
    return TW_OK;
}

int tw::launch_narrow_logits(const float *lg4, uint64_t n, int A, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_logits_kernel, dim3(grid_for(n * (uint64_t)A, 256)), dim3(256), 0, s, lg4, n, A, out);
    TW_HIP(hipGetLastError());
    return TW_OK;
}

extern "C" int tw_device_env_host_vtable(const tw_device_env *env, const void *proto, size_t proto_bytes, tw_env_vtable *out)
{
    if (!out) { set_error("tw_device_env_host_vtable: null argument"); return TW_ERR_INVALID; }
    int rc = check_descriptor(env, proto, proto_bytes, "tw_device_env_host_vtable"); if (rc) return rc;
    *out = host_table(env, proto);
    return TW_OK;
}

// precision="fp16x2" computes what the f32 kernel computes only while every operand has a finite pair of binary16 terms
// (tw_engine_generic16x2.hpp, "Range": every |weight| and every |activation that feeds a Linear| below 4095).  The pack kernel and
// the engine flag a collect that left that range; the library then says so on stderr and returns the f32 kernel's collect, on the
// same workspace, instead -- never results the f32 mode would not have given (as tw_ppo_collect does for the Puzzle kernels).
extern "C" int tw_ppo_collect_device_env(const tw_device_env *env, const void *proto, size_t proto_bytes, const tw_policy *policy,
                                         const tw_ppo_params *prm, uint32_t max_records_per_episode, tw_collected **out)
{
    if (!policy || !prm || !out) { set_error("tw_ppo_collect_device_env: null argument"); return TW_ERR_INVALID; }
    *out = nullptr;
    int rc = check_descriptor(env, proto, proto_bytes, "tw_ppo_collect_device_env"); if (rc) return rc;
    note_launch(TW_KERNEL_NONE, 0, 0, 0, 0, false, false, false, false, 0, 0);      // (tw_debug_last_launch: nothing yet; the host-stepped path reports nothing)
    const tw_env_vtable vt = host_table(env, proto);
    PolicyDev view;                                                       // (a one-common-layer policy in a module that packs its layers)
    const PolicyDev *pd = kernel_policy(env, policy_dev(policy), prm->precision, &view);
    // precision="fp16": rollout_env16_kernel over EngineV16, when the module holds it (built with TW_DEVICE_ENV_FP16) and the policy
    // is a generic stack with both heads (at most GEN16_MAX_LAYERS layers: tw_policy_create's own limit)
    const bool f16 = prm->precision == TW_PREC_F16 && env->launch_rollout16 && env->groups_per_cu16 && pd->generic && pd->n_action >= 1 &&
                     pd->n_value >= 1 && pd->n_common + pd->n_action + pd->n_value <= GEN16_MAX_LAYERS;
    // precision="fp16x2": rollout_env16x2_kernel over EngineV16x2, when the module holds it (the capability query: kernel 5 with a null
    // result, answered without the HIP runtime -- asked BEFORE anything else, so that a module built without TW_DEVICE_ENV_FP16X2 is
    // never handed a split request) and EngineV16 takes the policy.  It travels through launch_rollout16
    const bool f16x2 = prm->precision == TW_PREC_F16X2 && env->launch_rollout16 && engine16_takes(pd) &&
                       env->groups_per_cu(ENV_KERNEL_ROLLOUT16X2, 0, nullptr) == (int)hipSuccess;
    // what the kernels do not take: the host-stepped path over the module's own vtable (same bytes; its messages).  Episodes
    // longer than the finalize step's LDS tile holds (finalize_ppo_max_t_pad: 1,820 records) go there too.
    if (!pd->generic || (prm->precision != TW_PREC_F32_EXACT && !f16 && !f16x2) || max_records_per_episode > (uint32_t)finalize_ppo_max_t_pad(0))
        return tw_ppo_collect_env(&vt, policy, prm, max_records_per_episode, out);
    if (prm->num_episodes == 0) { set_error("Something went wrong. No data in collected data chunks to merge. "); return TW_ERR_EMPTY; }   // collector.rs:41
    rc = check_env_policy(vt, pd); if (rc) return rc;
    if (max_records_per_episode == 0) { set_error("tw_ppo_collect_env: max_records_per_episode must be positive"); return TW_ERR_INVALID; }
    if (pd->n_perms > 0 && pd->obs_size > 256 && !pd->obs_perms16) { set_error("tw_ppo_collect_device_env: policy without its two-byte twist table"); return TW_ERR_INVALID; }
    rc = require_device(); if (rc) return rc;

    const uint64_t E = prm->num_episodes;
    const bool ragged = vt.observe_n != nullptr;                          // observations of variable length: two-byte ids, 0xFFFF = no id
    const uint32_t A = env->num_actions, NO = vt.n_obs, OW = (ragged || pd->obs_size > 256) ? 2u : 1u;
    const uint64_t t_pad = max_records_per_episode, R = E * t_pad;
    const size_t lds_bytes = f16x2 ? engine16x2_lds_bytes(env->engine_nc, *pd) : f16 ? engine16_lds_bytes(env->engine_nc, *pd) : engine_lds_bytes(env->engine_nc, *pd);
    if (lds_bytes > 159 * 1024) { set_error("rollout: %zu bytes of LDS needed, 159 KiB available", lds_bytes); return TW_ERR_UNSUPPORTED; }
    EnvGrid grid;
    rc = env_grid(env, f16x2 ? ENV_KERNEL_ROLLOUT16X2 : f16 ? ENV_KERNEL_ROLLOUT16 : 0, lds_bytes, E, prm->reserve_cus, &grid); if (rc) return rc;
    const uint64_t blocks = grid.blocks;
    if (blocks > 0x7fffffffull || t_pad > 0x7fffffffull) { set_error("tw_ppo_collect_device_env: bad episode count %llu", (unsigned long long)E); return TW_ERR_INVALID; }
    // the f16 image's size, from the layout function the pack kernel and the engine index with (tw_engine_generic16.hpp), over the
    // layer table's widths -- which live on the device (they never change after tw_policy_create)
    size_t image_halves = 0;
    if (f16 || f16x2) {
        const int n_layers = pd->n_common + pd->n_action + pd->n_value;
        std::vector<LayerDev> layers((size_t)n_layers);
        // (on the library's stream, not the null stream: a blocking copy there would wait for whatever else the process has queued on it)
        TW_HIP(hipMemcpyAsync(layers.data(), pd->layers, (size_t)n_layers * sizeof(LayerDev), hipMemcpyDeviceToHost, current_stream()));
        TW_HIP(hipStreamSynchronize(current_stream()));
        // (fp16x2: two planes per layer and no table, tw_engine_generic16x2.hpp)
        image_halves = f16x2 ? gen16x2_image_halves(layers.data(), n_layers)
                             : gen16_image_halves((uint32_t)pd->obs_size, (uint32_t)pd->emb, layers.data(), n_layers);
    }

    std::unique_lock<std::mutex> lock(workspace_mutex());      // (released before the f32 run of an out-of-range fp16x2 collect)
    hipStream_t s = current_stream();
    size_t cur = 0;
    auto seg = [&](size_t bytes) { size_t o = cur; cur = (cur + bytes + 255) / 256 * 256; return o; };
    const size_t o_rec = seg(R * sizeof(PaddedRec)), o_len = seg(E * 4), o_start = seg(E * 8), o_total = seg(32), o_scan = seg(scan_scratch_bytes(E)),
                 o_obs16 = seg(R * NO * 2),                                // (o_total: record total | err | the episode queue's counter)
                 o_lgw = seg(A > 4 ? R * A * sizeof(float) : 0);           // more than four actions: the masked logits, [E][t_pad][A]
    // fp16: the binary16 weight image behind the f32 carve, which does not move (f32: no bytes).  Every half of it -- table padding,
    // weight padding and read slack included -- is written by pack_generic16_kernel before the rollout reads it; the table of
    // tests/memory_matrix.py lists the f32 carve's segments, and tests/test_gpu_device_env_fp16.py runs the fp16 collect on pre-filled
    // workspace memory (tw_debug_fill_memory) for this one.  fp16x2: the split image in the same place, every half of it written by
    // pack_generic16x2_kernel (tests/test_gpu_device_env_fp16x2.py).  f32 under a view of a one-common-layer policy: its block of
    // EngineV layers in the same place, every byte of it written by pack_basic_view_kernel (tests/test_gpu_device_env_basic.py)
    const size_t o_img = cur;
    cur = (cur + image_halves * sizeof(_Float16) + basic_block_bytes(pd) + 255) / 256 * 256;
    void *wsp = nullptr;
    rc = workspace_reserve(cur, &wsp); if (rc) return rc;
    uint8_t *ws = reinterpret_cast<uint8_t *>(wsp);
    EnvRolloutArgs ra{};
    ra.pol = launch_policy(pd, ws + o_img);
    ra.out.rec = reinterpret_cast<PaddedRec *>(ws + o_rec); ra.out.ep_len = reinterpret_cast<uint32_t *>(ws + o_len); ra.out.t_pad = (int32_t)t_pad;
    ra.obs16 = reinterpret_cast<uint16_t *>(ws + o_obs16);
    if (A > 4) ra.lgw = reinterpret_cast<float *>(ws + o_lgw);
    ra.err = reinterpret_cast<uint32_t *>(ws + o_total + 8);
    ra.num_episodes = E; ra.episode_offset = prm->episode_offset; ra.seed = prm->seed;
    uint64_t *ep_start_ws = reinterpret_cast<uint64_t *>(ws + o_start), *total_d = reinterpret_cast<uint64_t *>(ws + o_total);

    EventSet ev; rc = ev.init(); if (rc) return rc;
    TW_HIP(hipMemsetAsync(ws + o_total, 0, 32, s));
    if (grid.persist) {                                                   // slot i starts with episode i; the queue starts behind the slots
        ra.queue = reinterpret_cast<unsigned int *>(ws + o_total + 16);
        const unsigned int first = (unsigned int)(blocks * GEN_COLS);
        TW_HIP(hipMemcpyAsync(ra.queue, &first, 4, hipMemcpyHostToDevice, s));
    }
    TW_HIP(hipEventRecord(ev.ev[0], s));
    int lr;
    if (f16 || f16x2) {                                                   // the pack of the image, then the rollout (the module's launcher)
        EnvRollout16Args ra16{};
        ra16.r = ra;
        ra16.image.img = reinterpret_cast<_Float16 *>(ws + o_img);
        ra16.image.halves = f16x2 ? ((uint64_t)image_halves | GEN16X2_REQUEST) : (uint64_t)image_halves;   // (the request: bit 63)
        lr = env->launch_rollout16(&ra16, proto, (unsigned)blocks, lds_bytes, s);
    } else
        lr = env->launch_rollout(&ra, proto, (unsigned)blocks, lds_bytes, s);
    if (lr != (int)hipSuccess) return hip_fail((hipError_t)lr, "device environment rollout launch", __FILE__, __LINE__);
    // (tw_debug_last_launch: nw = 32 marks the split-f16 kernel, 16 the f16 one, 0 the f32 one -- include/twisterl_hip.h)
    note_launch(TW_KERNEL_ROLLOUT_BIG, 1, (int)env->engine_nc, f16x2 ? 32 : f16 ? 16 : 0, 0, grid.persist, false, false, false, (uint32_t)blocks, 256);
    TW_HIP(hipEventRecord(ev.ev[1], s));
    rc = launch_scan(ra.out.ep_len, E, prm->merge_order ? 1 : 0, ep_start_ws, total_d, ws + o_scan, scan_scratch_bytes(E), s);
    if (rc) return rc;
    TW_HIP(hipEventRecord(ev.ev[2], s));
    uint64_t hv[2] = {0, 0};
    TW_HIP(hipMemcpyAsync(hv, ws + o_total, 16, hipMemcpyDeviceToHost, s));
    TW_HIP(hipStreamSynchronize(s));
    const uint64_t total = hv[0];
    const uint32_t err = (uint32_t)hv[1];
    if (f16x2 && (err & GEN16X2_ERR_RANGE)) {                             // before every other error: the f32 kernel's run decides those
        lock.unlock();
        fprintf(stderr, "[twisterl_hip] precision fp16x2: a weight or an activation is outside the range of the split-f16 terms "
                        "(|weight| < 4095, |activation| < 4095): this collect runs in fp32\n");
        tw_ppo_params p32 = *prm;
        p32.precision = TW_PREC_F32_EXACT;
        return tw_ppo_collect_device_env(env, proto, proto_bytes, policy, &p32, max_records_per_episode, out);
    }
    if (err & 9u) {
        // the id (or the count of observe_n) the host path reports: the first it meets -- the smallest record index, then the smallest
        // episode (the kernel flagged each such episode in ep_len and left the id / the count in that record's value field, which of
        // the two in its reward field)
        std::vector<uint32_t> len(E);
        TW_HIP(hipMemcpy(len.data(), ra.out.ep_len, E * 4, hipMemcpyDeviceToHost));
        uint64_t first = E;
        for (uint64_t e = 0; e < E; ++e)
            if ((len[e] & 0x80000000u) && (first == E || (len[e] & 0x7fffffffu) < (len[first] & 0x7fffffffu))) first = e;
        int32_t id = 0; bool count = false;
        if (first < E) {
            PaddedRec r;
            TW_HIP(hipMemcpy(&r, ra.out.rec + first * t_pad + ((len[first] & 0x7fffffffu) - 1u), sizeof(r), hipMemcpyDeviceToHost));
            id = __builtin_bit_cast(int32_t, r.value); count = r.reward != 0.0f;
        }
        if (count) set_error("observation of %u ids, at most %u", (uint32_t)id, NO);
        else set_error("index out of bounds: obs id %d, obs_size %d", (int)id, pd->obs_size);
        return TW_ERR_INVALID;
    }
    if (err & 2u) { set_error("tw_ppo_collect_env: an episode did not end within %u records", max_records_per_episode); return TW_ERR_INVALID; }
    if (total == 0 || total > R) { set_error("collect: inconsistent record count %llu (max %llu)", (unsigned long long)total, (unsigned long long)R); return TW_ERR_HIP; }

    CollectTail tail{};
    tail.is_ppo = true; tail.traj = ra.out; tail.ep_start = ep_start_ws; tail.E = E; tail.total = total;
    tail.n_cells = NO; tail.n_actions = A; tail.obs_size = (uint32_t)pd->obs_size; tail.ragged = ragged;
    tail.cell_major = false;                                              // an environment's ids: any of [0, obs_size), in any order
    tail.obs16 = ra.obs16; tail.obs_width = OW; tail.wide = ra.lgw;
    tail.gamma = prm->gamma; tail.lambda = prm->lambda; tail.ev = &ev; tail.stream = s;
    tail.stats.padded_bytes = cur; tail.stats.forward_evals = total;
    tail.stats.rollout_blocks = (uint32_t)blocks; tail.stats.rollout_threads = 256;
    return collect_tail(tail, out);
}

// AZCollector::collect (az.rs:51-109) of a device environment whose module holds the search kernel: self-play in mcts_env_kernel, the
// scan, then collect_tail as above.  Byte-equal to tw_az_collect_env over the module's vtable, which is also where everything
// the kernel or the finalize step does not take goes.
extern "C" int tw_az_collect_device_env(const tw_device_env *env, const void *proto, size_t proto_bytes, const tw_policy *policy,
                                        const tw_az_params *prm, uint32_t max_records_per_episode, tw_collected **out)
{
    if (!policy || !prm || !out) { set_error("tw_az_collect_device_env: null argument"); return TW_ERR_INVALID; }
    *out = nullptr;
    int rc = check_descriptor(env, proto, proto_bytes, "tw_az_collect_device_env"); if (rc) return rc;
    note_launch(TW_KERNEL_NONE, 0, 0, 0, 0, false, false, false, false, 0, 0);      // (the host-stepped path reports nothing)
    const tw_env_vtable vt = host_table(env, proto);
    PolicyDev view;                                                       // (as the PPO collect)
    const PolicyDev *pd = kernel_policy(env, policy_dev(policy), prm->precision, &view);
    uint64_t node_cap = 0;
    // precision="fp16": mcts_env16_kernel, when the module holds it and EngineV16 takes the policy (search_f16); any other precision but
    // f32, and fp16 without that, are the host-stepped path's to refuse
    const bool f16 = search_f16(env, pd, prm->precision);
    if (!env->launch_search || !pd->generic || (prm->precision != TW_PREC_F32_EXACT && !f16) || max_records_per_episode > FINALIZE_AZ_MAX_T_PAD ||
        !search_fits(env->num_actions, prm->num_mcts_searches, prm->max_expand_depth, max_records_per_episode, &node_cap))
        return tw_az_collect_env(&vt, policy, prm, max_records_per_episode, out);
    if (prm->num_episodes == 0) { set_error("Something went wrong. No data in collected data chunks to merge. "); return TW_ERR_EMPTY; }   // collector.rs:41
    rc = check_env_policy(vt, pd); if (rc) return rc;
    if (max_records_per_episode == 0) { set_error("tw_az_collect_env: max_records_per_episode must be positive"); return TW_ERR_INVALID; }
    if (pd->n_perms > 0 && pd->obs_size > 256 && !pd->obs_perms16) { set_error("tw_az_collect_device_env: policy without its two-byte twist table"); return TW_ERR_INVALID; }
    rc = require_device(); if (rc) return rc;

    const uint64_t E = prm->num_episodes;
    const bool ragged = vt.observe_n != nullptr;
    const uint32_t A = env->num_actions, NO = vt.n_obs, OW = (ragged || pd->obs_size > 256) ? 2u : 1u;
    const uint64_t t_pad = max_records_per_episode, R = E * t_pad;
    const size_t lds_bytes = f16 ? engine16_lds_bytes(env->engine_nc, *pd) : engine_lds_bytes(env->engine_nc, *pd);
    const size_t search_lds = env_mcts_pending_bytes(env->n_obs) + env_mcts_probs_bytes(env->num_actions);      // what the launcher adds
    if (lds_bytes + search_lds > 159 * 1024) {
        set_error("mcts: %zu bytes of LDS needed, 159 KiB available", lds_bytes + search_lds); return TW_ERR_UNSUPPORTED;
    }
    const uint64_t blocks = (E + GEN_COLS - 1) / GEN_COLS;              // (the search kernel has no persistent form: one column per episode)
    if (blocks > 0x7fffffffull) { set_error("tw_az_collect_device_env: bad episode count %llu", (unsigned long long)E); return TW_ERR_INVALID; }

    std::lock_guard<std::mutex> lock(workspace_mutex());
    hipStream_t s = current_stream();
    size_t image_halves = 0;                                              // fp16: the image's size, as the PPO collect reads it
    if (f16) { rc = gen16_image_size(pd, s, &image_halves); if (rc) return rc; }
    size_t cur = 0;
    auto seg = [&](size_t bytes) { size_t o = cur; cur = (cur + bytes + 255) / 256 * 256; return o; };
    const size_t o_rec = seg(R * sizeof(PaddedRec)), o_len = seg(E * 4), o_start = seg(E * 8), o_total = seg(32), o_scan = seg(scan_scratch_bytes(E)),
                 o_obs16 = seg(R * NO * 2), o_ce = seg(E * 16), o_arena = seg((size_t)E * node_cap * ENV_MCTS_NODE_BYTES),
                 o_pw = seg(A > 4 ? R * A * sizeof(float) : 0);           // more than four actions: the MCTS probabilities, [E][t_pad][A]
    // fp16: the binary16 weight image behind everything else, so that no f32 offset moves (f32: no bytes).  Every half of it is written
    // by pack_generic16_kernel before mcts_env16_kernel reads it (tests/test_gpu_device_env_fp16_search.py runs on pre-filled memory).
    // f32 under a view of a one-common-layer policy: its block of EngineV layers in the same place, as in the PPO collect
    const size_t o_img = cur;
    cur = (cur + image_halves * sizeof(_Float16) + basic_block_bytes(pd) + 255) / 256 * 256;
    rc = check_memory_fit(cur, "tw_az_collect_device_env"); if (rc) return rc;
    void *wsp = nullptr;
    rc = workspace_reserve(cur, &wsp); if (rc) return rc;
    uint8_t *ws = reinterpret_cast<uint8_t *>(wsp);
    EnvMctsArgs ma{};
    ma.struct_bytes = (uint32_t)sizeof(EnvMctsArgs);
    ma.pol = launch_policy(pd, ws + o_img);
    ma.out.rec = reinterpret_cast<PaddedRec *>(ws + o_rec); ma.out.ep_len = reinterpret_cast<uint32_t *>(ws + o_len); ma.out.t_pad = (int32_t)t_pad;
    ma.obs16 = reinterpret_cast<uint16_t *>(ws + o_obs16);
    ma.err = reinterpret_cast<uint32_t *>(ws + o_total + 8); ma.eval_count = reinterpret_cast<unsigned long long *>(ws + o_total + 16);
    ma.col_err = reinterpret_cast<uint32_t *>(ws + o_ce);
    ma.num_columns = E; ma.episode_offset = prm->episode_offset; ma.seed = prm->seed;
    ma.num_searches = prm->num_mcts_searches; ma.max_expand_depth = prm->max_expand_depth; ma.C = prm->C; ma.node_cap = (uint32_t)node_cap;
    ma.arena = ws + o_arena;
    if (A > 4) ma.pw = reinterpret_cast<float *>(ws + o_pw);
    if (f16) { ma.image.img = reinterpret_cast<_Float16 *>(ws + o_img); ma.image.halves = image_halves; }   // the launcher packs it, then mcts_env16_kernel
    uint64_t *ep_start_ws = reinterpret_cast<uint64_t *>(ws + o_start), *total_d = reinterpret_cast<uint64_t *>(ws + o_total);

    EventSet ev; rc = ev.init(); if (rc) return rc;
    TW_HIP(hipMemsetAsync(ws + o_total, 0, 32, s));
    TW_HIP(hipMemsetAsync(ws + o_ce, 0, E * 16, s));
    TW_HIP(hipEventRecord(ev.ev[0], s));
    const int lr = env->launch_search(&ma, proto, (unsigned)blocks, lds_bytes, s);
    if (lr == (int)hipErrorInvalidValue) return search_launch_refused("tw_az_collect_device_env");
    if (lr != (int)hipSuccess) return hip_fail((hipError_t)lr, "device environment search launch", __FILE__, __LINE__);
    // (tw_debug_last_launch: nw = 16 marks the f16 kernel, 0 the f32 one -- include/twisterl_hip.h)
    note_launch(TW_KERNEL_MCTS_BIG, 1, (int)env->engine_nc, f16 ? 16 : 0, 0, false, false, false, false, (uint32_t)blocks, 256);
    TW_HIP(hipEventRecord(ev.ev[1], s));
    rc = launch_scan(ma.out.ep_len, E, prm->merge_order ? 1 : 0, ep_start_ws, total_d, ws + o_scan, scan_scratch_bytes(E), s);
    if (rc) return rc;
    TW_HIP(hipEventRecord(ev.ev[2], s));
    uint64_t hv[3] = {0, 0, 0};
    TW_HIP(hipMemcpyAsync(hv, ws + o_total, 24, hipMemcpyDeviceToHost, s));
    TW_HIP(hipStreamSynchronize(s));
    const uint64_t total = hv[0];
    const uint32_t err = (uint32_t)hv[1];
    if (err & 11u) {
        std::vector<uint32_t> ce(E * 4);
        TW_HIP(hipMemcpy(ce.data(), ma.col_err, E * 16, hipMemcpyDeviceToHost));
        if (!first_search_error(ce, E, NO, pd->obs_size)) set_error("tw_az_collect_env: an episode did not end within %u records", max_records_per_episode);
        return TW_ERR_INVALID;
    }
    if (total == 0 || total > R) { set_error("az collect: inconsistent record count %llu (max %llu)", (unsigned long long)total, (unsigned long long)R); return TW_ERR_HIP; }

    CollectTail tail{};
    tail.is_ppo = false; tail.traj = ma.out; tail.ep_start = ep_start_ws; tail.E = E; tail.total = total;
    tail.n_cells = NO; tail.n_actions = A; tail.obs_size = (uint32_t)pd->obs_size; tail.ragged = ragged;
    tail.cell_major = false;                                              // an environment's ids: any of [0, obs_size), in any order
    tail.obs16 = ma.obs16; tail.obs_width = OW; tail.wide = ma.pw;
    tail.ev = &ev; tail.stream = s;
    tail.stats.padded_bytes = cur;
    tail.stats.forward_evals = hv[2] * (uint64_t)(pd->n_perms > 0 ? pd->n_perms : 1);
    tail.stats.rollout_blocks = (uint32_t)blocks; tail.stats.rollout_threads = 256;
    return collect_tail(tail, out);
}

namespace {

// the most bytes of action rows (attempts x max_steps) a solve keeps on the device; a longer bound goes to the host-stepped path
constexpr uint64_t SOLVE_ACTION_BYTES_MAX = 1ull << 30;

// index of solve_env16_kernel for tw_device_env::groups_per_cu (a module built with TW_DEVICE_ENV_FP16_SOLVE)
constexpr int ENV_KERNEL_SOLVE16 = 3;

// index of solve_env16x2_kernel for tw_device_env::groups_per_cu (a module built with TW_DEVICE_ENV_FP16X2_SOLVE)
constexpr int ENV_KERNEL_SOLVE16X2 = 6;

// precision="fp16x2" of evaluate / solve: solve_env16x2_kernel over EngineV16x2, without MCTS alone (the search kernel has no split
// form), when EngineV16 takes the policy and the module holds the kernel (the capability query: kernel 6 with a null result, answered
// without the HIP runtime -- asked BEFORE a split request is formed, so that a module built without TW_DEVICE_ENV_FP16X2_SOLVE is
// never handed one)
bool attempts_f16x2(const tw_device_env *env, const PolicyDev *pd, const tw_solve_params *prm)
{
    return prm->precision == TW_PREC_F16X2 && prm->num_mcts_searches == 0 && engine16_takes(pd) &&
           env->groups_per_cu(ENV_KERNEL_SOLVE16X2, 0, nullptr) == (int)hipSuccess;
}

// precision="fp16" of evaluate / solve: solve_env16_kernel over EngineV16, when the module holds it (the capability query: kernel 3
// with a null result, answered without the HIP runtime), the policy is a generic stack with both heads (at most GEN16_MAX_LAYERS
// layers: the collect's own rule).  With MCTS the kernel is mcts_env16_kernel instead, under the same rule: search_f16
bool attempts_f16(const tw_device_env *env, const PolicyDev *pd, const tw_solve_params *prm)
{
    if (prm->precision == TW_PREC_F16X2) return attempts_f16x2(env, pd, prm);
    if (prm->num_mcts_searches != 0) return search_f16(env, pd, prm->precision);
    return prm->precision == TW_PREC_F16 && engine16_takes(pd) && env->groups_per_cu(ENV_KERNEL_SOLVE16, 0, nullptr) == (int)hipSuccess;
}

// What solve_env_kernel / solve_env16_kernel / solve_env16x2_kernel / mcts_env_kernel take of an evaluate or a solve; everything else is the host-stepped path's (the callers
// hand over to it).  node_cap: the search's tree size, for attempts_device_env.
bool attempts_on_device(const tw_device_env *env, const PolicyDev *pd, const tw_solve_params *prm, uint64_t num_episodes, uint32_t max_steps,
                        uint64_t *node_cap)
{
    const bool mcts = prm->num_mcts_searches != 0;
    *node_cap = 0;
    return !(!pd->generic || (prm->precision != TW_PREC_F32_EXACT && !attempts_f16(env, pd, prm)) || prm->num_searches == 0 || num_episodes == 0 || max_steps > 0x7fffffffu ||
             (mcts && (!env->launch_search || !search_fits(env->num_actions, prm->num_mcts_searches, prm->max_expand_depth, max_steps ? max_steps : 1u, node_cap))));
}

// The attempts of evaluate (from_state == false: episode e of num_episodes starts from reset(seed, episode_offset + e)) and of solve
// (from_state: ONE episode, every attempt starts from the prototype as it is) in one launch of solve_env_kernel or, with
// num_mcts_searches > 0, of mcts_env_kernel in solve mode: checks, grid, workspace, launch, the errors of the host-stepped path, and
// run_attempts_env's reduction -- per episode the first attempt whose (success, total) is strictly better (solve.rs:84-98).
// best_actions (solve; else null): the moves of that attempt, the only row that is copied back.
// precision="fp16x2" (attempts_f16x2) computes what the f32 kernel computes only while every operand has a finite pair of binary16
// terms; the pack kernel and the engine flag a call that left that range (GEN16X2_ERR_RANGE), and this function then says so on stderr
// and runs itself again in f32, on the same workspace -- never results the f32 mode would not have given, as the PPO collect above.
int attempts_device_env(const char *who, const tw_device_env *env, const void *proto, const tw_env_vtable &vt, const PolicyDev *pd,
                        const tw_solve_params *prm, uint64_t num_episodes, uint64_t episode_offset, bool from_state, uint32_t max_steps_in,
                        uint64_t node_cap, std::vector<float> &best_s, std::vector<float> &best_r, std::vector<uint32_t> *best_actions)
{
    const bool mcts = prm->num_mcts_searches != 0;
    const bool f16 = prm->precision == TW_PREC_F16;                       // (attempts_on_device: then attempts_f16 holds; with mcts: search_f16)
    const bool f16x2 = prm->precision == TW_PREC_F16X2;                   // (attempts_on_device: then attempts_f16x2 holds, and mcts does not)
    const uint32_t max_steps = max_steps_in ? max_steps_in : 1u;
    int rc = check_env_policy(vt, pd); if (rc) return rc;
    if (pd->n_perms > 0 && pd->obs_size > 256 && !pd->obs_perms16) { set_error("%s: policy without its two-byte twist table", who); return TW_ERR_INVALID; }
    rc = require_device(); if (rc) return rc;
    const uint64_t N = prm->num_searches, NA = num_episodes * N;
    if (NA / N != num_episodes) { set_error("solve: bad attempt count %llu", (unsigned long long)NA); return TW_ERR_INVALID; }
    const size_t lds_bytes = f16x2 ? engine16x2_lds_bytes(env->engine_nc, *pd) : f16 ? engine16_lds_bytes(env->engine_nc, *pd) : engine_lds_bytes(env->engine_nc, *pd);
    const size_t search_lds = mcts ? env_mcts_pending_bytes(env->n_obs) + env_mcts_probs_bytes(env->num_actions) : 0;
    if (lds_bytes + search_lds > 159 * 1024) {
        set_error("solve: %zu bytes of LDS needed, 159 KiB available", lds_bytes + search_lds); return TW_ERR_UNSUPPORTED;
    }
    EnvGrid grid;                                                         // (MCTS-guided attempts: the search kernel, one column per attempt)
    grid.blocks = (NA + GEN_COLS - 1) / GEN_COLS; grid.persist = false;
    if (!mcts) { rc = env_grid(env, f16x2 ? ENV_KERNEL_SOLVE16X2 : f16 ? ENV_KERNEL_SOLVE16 : 1, lds_bytes, NA, 0, &grid); if (rc) return rc; }
    const uint64_t blocks = grid.blocks;
    if (blocks > 0x7fffffffull) { set_error("solve: bad attempt count %llu", (unsigned long long)NA); return TW_ERR_INVALID; }
    // the played moves: one row of max_steps bytes per attempt (an attempt that ends has played at most max_steps)
    const uint32_t stride = best_actions ? max_steps : 0u;
    // fp16: the image's size, as the collect reads it -- the layout function over the layer table's widths, which live on the device
    size_t image_halves = 0;
    if (f16 || f16x2) {
        const int n_layers = pd->n_common + pd->n_action + pd->n_value;
        std::vector<LayerDev> layers((size_t)n_layers);
        TW_HIP(hipMemcpyAsync(layers.data(), pd->layers, (size_t)n_layers * sizeof(LayerDev), hipMemcpyDeviceToHost, current_stream()));   // (as the collect)
        TW_HIP(hipStreamSynchronize(current_stream()));
        // (fp16x2: two planes per layer and no table, tw_engine_generic16x2.hpp)
        image_halves = f16x2 ? gen16x2_image_halves(layers.data(), n_layers)
                             : gen16_image_halves((uint32_t)pd->obs_size, (uint32_t)pd->emb, layers.data(), n_layers);
    }

    std::vector<float> succ(NA), tot(NA);
    std::vector<uint32_t> steps(NA), ce;
    uint64_t hv[2] = {0, 0};
    std::unique_lock<std::mutex> lock(workspace_mutex());                 // (to the end: the best attempt's row is read from the workspace;
                                                                          // released before the f32 run of an out-of-range fp16x2 call)
    hipStream_t s = current_stream();
    size_t cur = 0;
    auto seg = [&](size_t bytes) { size_t o = cur; cur = (cur + bytes + 255) / 256 * 256; return o; };
    const size_t o_s = seg(NA * 4), o_t = seg(NA * 4), o_n = seg(NA * 4), o_err = seg(32), o_ce = seg(mcts ? NA * 16 : 0),
                 o_arena = seg(mcts ? (size_t)NA * node_cap * ENV_MCTS_NODE_BYTES : 0), o_act = seg((size_t)NA * stride);
    // fp16: the binary16 weight image behind o_act, appended as the fp16 collect appends its own (f32: no bytes, and nothing moves).
    // Every half of it is written by pack_generic16_kernel before solve_env16_kernel reads it; tests/test_gpu_device_env_fp16_solve.py
    // runs the call on pre-filled workspace memory for this region.  fp16x2: the split image in the same place, every half of it
    // written by pack_generic16x2_kernel (tests/test_gpu_device_env_fp16x2_solve.py).  f32 under a view of a one-common-layer policy
    // (the callers' kernel_policy): its block of EngineV layers in the same place, every byte of it written by pack_basic_view_kernel
    const size_t o_img = cur;
    cur = (cur + image_halves * sizeof(_Float16) + basic_block_bytes(pd) + 255) / 256 * 256;
    if (mcts) { rc = check_memory_fit(cur, who); if (rc) return rc; }
    void *wsp = nullptr;
    rc = workspace_reserve(cur, &wsp); if (rc) return rc;
    uint8_t *ws = reinterpret_cast<uint8_t *>(wsp);
    uint8_t *act_d = stride ? ws + o_act : nullptr;
    TW_HIP(hipMemsetAsync(ws + o_err, 0, 32, s));                         // (o_err: err | the queue's counter or the evaluation count)
    if (mcts) {
        // MCTS-guided attempts (solve.rs:41-47): mcts_env_kernel in solve mode, one column = one attempt
        EnvMctsArgs ma{};
        ma.struct_bytes = (uint32_t)sizeof(EnvMctsArgs);
        ma.pol = launch_policy(pd, ws + o_img); ma.num_columns = NA; ma.episode_offset = episode_offset; ma.seed = prm->seed;
        ma.num_searches = prm->num_mcts_searches; ma.max_expand_depth = prm->max_expand_depth; ma.C = prm->C; ma.node_cap = (uint32_t)node_cap;
        ma.arena = ws + o_arena; ma.err = reinterpret_cast<uint32_t *>(ws + o_err); ma.eval_count = reinterpret_cast<unsigned long long *>(ws + o_err + 8);
        ma.col_err = reinterpret_cast<uint32_t *>(ws + o_ce);
        ma.solve_on = 1u; ma.deterministic = prm->deterministic ? 1u : 0u; ma.attempts = (uint32_t)N; ma.max_steps = max_steps;
        ma.success = reinterpret_cast<float *>(ws + o_s); ma.total = reinterpret_cast<float *>(ws + o_t); ma.n_steps = reinterpret_cast<uint32_t *>(ws + o_n);
        ma.from_state = from_state ? 1u : 0u; ma.actions = act_d; ma.actions_stride = stride;
        if (f16) { ma.image.img = reinterpret_cast<_Float16 *>(ws + o_img); ma.image.halves = image_halves; }   // the launcher packs it, then mcts_env16_kernel
        TW_HIP(hipMemsetAsync(ws + o_ce, 0, NA * 16, s));
        const int lr = env->launch_search(&ma, proto, (unsigned)blocks, lds_bytes, s);
        if (lr == (int)hipErrorInvalidValue) return search_launch_refused(who);
        if (lr != (int)hipSuccess) return hip_fail((hipError_t)lr, "device environment search launch", __FILE__, __LINE__);
        note_launch(TW_KERNEL_MCTS_BIG, 1, (int)env->engine_nc, f16 ? 16 : 0, 0, false, true, false, false, (uint32_t)blocks, 256);
    } else {
        EnvSolveArgs sa{};
        sa.pol = launch_policy(pd, ws + o_img); sa.num_attempts = NA; sa.episode_offset = episode_offset; sa.seed = prm->seed;
        sa.num_searches = (uint32_t)N; sa.deterministic = prm->deterministic ? 1u : 0u; sa.max_steps = max_steps;
        sa.success = reinterpret_cast<float *>(ws + o_s); sa.total = reinterpret_cast<float *>(ws + o_t);
        sa.n_steps = reinterpret_cast<uint32_t *>(ws + o_n); sa.err = reinterpret_cast<uint32_t *>(ws + o_err);
        sa.from_state = from_state ? 1u : 0u; sa.actions = act_d; sa.actions_stride = stride;
        if (grid.persist) {
            sa.queue = reinterpret_cast<unsigned int *>(ws + o_err + 8);
            const unsigned int first = (unsigned int)(blocks * GEN_COLS);
            TW_HIP(hipMemcpyAsync(sa.queue, &first, 4, hipMemcpyHostToDevice, s));
        }
        if (f16 || f16x2) {                                               // the module's launcher packs it, then solve_env16_kernel
            sa.image.img = reinterpret_cast<_Float16 *>(ws + o_img);      // (fp16x2, the request: bit 63 -- then solve_env16x2_kernel)
            sa.image.halves = f16x2 ? ((uint64_t)image_halves | GEN16X2_REQUEST) : (uint64_t)image_halves;
        }
        const int lr = env->launch_solve(&sa, proto, (unsigned)blocks, lds_bytes, s);
        if (lr != (int)hipSuccess) return hip_fail((hipError_t)lr, "device environment evaluate launch", __FILE__, __LINE__);
        // (tw_debug_last_launch: nw = 32 marks the split-f16 kernel, 16 the f16 one, 0 the f32 one -- include/twisterl_hip.h)
        note_launch(TW_KERNEL_SOLVE_BIG, 1, (int)env->engine_nc, f16x2 ? 32 : f16 ? 16 : 0, 0, grid.persist, from_state, false, false, (uint32_t)blocks, 256);
    }
    TW_HIP(hipMemcpyAsync(succ.data(), ws + o_s, NA * 4, hipMemcpyDeviceToHost, s));
    TW_HIP(hipMemcpyAsync(tot.data(), ws + o_t, NA * 4, hipMemcpyDeviceToHost, s));
    TW_HIP(hipMemcpyAsync(steps.data(), ws + o_n, NA * 4, hipMemcpyDeviceToHost, s));
    TW_HIP(hipMemcpyAsync(hv, ws + o_err, 8, hipMemcpyDeviceToHost, s));
    TW_HIP(hipStreamSynchronize(s));
    const uint32_t err = (uint32_t)hv[0];
    if (f16x2 && (err & GEN16X2_ERR_RANGE)) {                             // before every other error: the f32 kernel's run decides those
        lock.unlock();
        fprintf(stderr, "[twisterl_hip] precision fp16x2: a weight or an activation is outside the range of the split-f16 terms "
                        "(|weight| < 4095, |activation| < 4095): this %s runs in fp32\n", from_state ? "solve" : "evaluate");
        tw_solve_params p32 = *prm;
        p32.precision = TW_PREC_F32_EXACT;
        return attempts_device_env(who, env, proto, vt, pd, &p32, num_episodes, episode_offset, from_state, max_steps_in, node_cap, best_s, best_r, best_actions);
    }
    if (mcts) {
        if (err & 13u) {
            ce.resize(NA * 4);
            TW_HIP(hipMemcpy(ce.data(), ws + o_ce, NA * 16, hipMemcpyDeviceToHost));
            if (!first_search_error(ce, NA, vt.n_obs, pd->obs_size)) set_error("solve: an attempt did not end within %u steps", max_steps);
            return TW_ERR_INVALID;
        }
    }
    note_attempts(succ.data(), tot.data(), steps.data(), NA);      // (tw_debug_last_attempts)
    if (err & 9u) {       // the first bad id (or count of observe_n) the host path meets: the smallest move, then the smallest attempt
                          // (its total holds the id / the count; a count: its success is 2.0f)
        uint64_t first = NA;
        for (uint64_t i = 0; i < NA; ++i)
            if ((steps[i] & 0x80000000u) && (first == NA || (steps[i] & 0x7fffffffu) < (steps[first] & 0x7fffffffu))) first = i;
        const int32_t id = first < NA ? __builtin_bit_cast(int32_t, tot[first]) : 0;
        if (first < NA && succ[first] == 2.0f) set_error("observation of %u ids, at most %u", (uint32_t)id, vt.n_obs);
        else set_error("index out of bounds: obs id %d, obs_size %d", (int)id, pd->obs_size);
        return TW_ERR_INVALID;
    }
    if (err & 4u) { set_error("solve: an attempt did not end within %u steps", max_steps); return TW_ERR_INVALID; }
    // best of N per episode (solve.rs:84-98: `if next_val.0 > best.0` on (success, total) tuples) -- run_attempts_env's reduction
    best_s.assign(num_episodes, 0.0f); best_r.assign(num_episodes, -__builtin_inff());
    uint64_t best_att = (uint64_t)-1;                                    // (of the last episode: solve has one)
    for (uint64_t ep = 0; ep < num_episodes; ++ep) {
        best_att = (uint64_t)-1;
        for (uint64_t k = 0; k < N; ++k) {
            const float sc = succ[ep * N + k], tr = tot[ep * N + k];
            if (sc > best_s[ep] || (sc == best_s[ep] && tr > best_r[ep])) { best_s[ep] = sc; best_r[ep] = tr; best_att = ep * N + k; }
        }
    }
    if (best_actions) {
        best_actions->clear();
        if (num_episodes == 1 && best_att != (uint64_t)-1) {
            const uint32_t n = steps[best_att] < stride ? steps[best_att] : stride;
            std::vector<uint8_t> row(n);
            if (n) { TW_HIP(hipMemcpy(row.data(), act_d + best_att * (uint64_t)stride, n, hipMemcpyDeviceToHost)); }
            best_actions->assign(row.begin(), row.end());                 // widened to the 32-bit entries of tw_solve_env32
        }
    }
    return TW_OK;
}

}  // namespace

extern "C" int tw_evaluate_device_env(const tw_device_env *env, const void *proto, size_t proto_bytes, const tw_policy *policy,
                                      const tw_solve_params *prm, uint64_t num_episodes, uint64_t episode_offset, uint32_t max_steps,
                                      float *success_rate, float *mean_reward)
{
    if (!policy || !prm || !success_rate || !mean_reward) { set_error("tw_evaluate_device_env: null argument"); return TW_ERR_INVALID; }
    int rc = check_descriptor(env, proto, proto_bytes, "tw_evaluate_device_env"); if (rc) return rc;
    note_launch(TW_KERNEL_NONE, 0, 0, 0, 0, false, false, false, false, 0, 0);
    const tw_env_vtable vt = host_table(env, proto);
    PolicyDev view;                                                       // (as the PPO collect)
    const PolicyDev *pd = kernel_policy(env, policy_dev(policy), prm->precision, &view);
    uint64_t node_cap = 0;
    if (!attempts_on_device(env, pd, prm, num_episodes, max_steps, &node_cap))
        return tw_evaluate_env(&vt, policy, prm, num_episodes, episode_offset, max_steps, success_rate, mean_reward);
    std::vector<float> bs, br;
    rc = attempts_device_env("tw_evaluate_device_env", env, proto, vt, pd, prm, num_episodes, episode_offset, false, max_steps, node_cap, bs, br, nullptr);
    if (rc) return rc;
    // the means in episode order (evaluate.rs:36-52) -- tw_evaluate_env's reduction
    float successes = 0.0f, rewards = 0.0f;
    for (uint64_t ep = 0; ep < num_episodes; ++ep) { successes = successes + bs[ep]; rewards = rewards + br[ep]; }
    *success_rate = successes / (float)num_episodes;
    *mean_reward = rewards / (float)num_episodes;
    return TW_OK;
}

// solve() (solve.rs:73-101) of a device environment: best of num_searches attempts from the prototype AS IT IS, in one launch; the
// contract and the bytes of tw_solve_env32 over the module's host vtable, which is also where everything the kernels do not take goes
extern "C" int tw_solve_device_env(const tw_device_env *env, const void *proto, size_t proto_bytes, const tw_policy *policy,
                                   const tw_solve_params *prm, uint32_t max_steps, float *success, float *reward,
                                   uint32_t *solution_out, uint32_t solution_cap, uint32_t *n_solution)
{
    if (!policy || !prm || !success || !reward) { set_error("tw_solve_device_env: null argument"); return TW_ERR_INVALID; }
    int rc = check_descriptor(env, proto, proto_bytes, "tw_solve_device_env"); if (rc) return rc;
    note_launch(TW_KERNEL_NONE, 0, 0, 0, 0, false, false, false, false, 0, 0);
    const tw_env_vtable vt = host_table(env, proto);
    PolicyDev view;                                                       // (as the PPO collect)
    const PolicyDev *pd = kernel_policy(env, policy_dev(policy), prm->precision, &view);
    uint64_t node_cap = 0;
    if (!attempts_on_device(env, pd, prm, 1, max_steps, &node_cap) ||
        (uint64_t)prm->num_searches * (uint64_t)(max_steps ? max_steps : 1u) > SOLVE_ACTION_BYTES_MAX)
        return tw_solve_env32(&vt, policy, prm, max_steps, success, reward, solution_out, solution_cap, n_solution);
    std::vector<float> bs, br; std::vector<uint32_t> acts;
    rc = attempts_device_env("tw_solve_device_env", env, proto, vt, pd, prm, 1, 0, true, max_steps, node_cap, bs, br, &acts);
    if (rc) return rc;
    *success = bs[0]; *reward = br[0];
    if (n_solution) *n_solution = (uint32_t)acts.size();
    if (solution_out) {
        if (acts.size() > solution_cap) { set_error("tw_solve_env: %zu entries, caller's buffer holds %u", acts.size(), solution_cap); return TW_ERR_INVALID; }
        if (!acts.empty()) memcpy(solution_out, acts.data(), acts.size() * sizeof(uint32_t));
    }
    return TW_OK;
}

