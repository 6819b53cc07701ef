// tw_env_basic_view.hpp -- the reference's DEFAULT policy (embedding -> ONE common Linear of 32 / 64 / 128 / 256 units -> linear heads,
// obs_size <= 256: tw_policy_create's "MFMA shape") inside the device-environment kernels.
//
// Such a policy's device image (PolicyDev) is built for the Puzzle engines: it has no EngineV layer table, so rollout_env_kernel,
// solve_env_kernel and mcts_env_kernel -- which run EngineV -- did not take it, and a device environment under it ran host-stepped.
// The image does carry the policy's natural-layout arrays (w1 [emb][hidden] with b1, wa [hidden][n_actions] with ba, wv with bv), kept
// live by Policy.update_from_torch.  Here is what turns those into the three LayerDev entries EngineV wants:
//   * basic_view_layout(): where the table, the padded biases and the matrix-core images of the three layers sit in ONE block of
//     memory, from gen_layer_shape (tw_common.hpp) -- the rule tw_policy_create lays a generic stack out with;
//   * basic_view(): the PolicyDev the kernels are handed -- the same embedding rows, twist tables and ReLU switches, generic = 1, one
//     layer per stack, the rows of EngineV's three activation buffers, `layers` = that block (in the call's workspace);
//   * pack_basic_view_kernel: writes EVERY byte of the block on the call's stream, in front of every launch, so that the kernels never
//     see weights older than the policy's.  A module holds it only when it was built with TW_DEVICE_ENV_BASIC
//     (build_device_env(..., basic=True)); its launchers (tw_rollout_env.hpp, tw_mcts_env.hpp) run it when the policy they are handed
//     is such a view, and the library (tw_device_env.hip) forms a view only for a module that answers groups_per_cu(7, 0, nullptr).
// The arithmetic does not change: both shapes follow the one numeric spec (k-ordered fma chain, bias last), and the image's padding
// multiplies -0.0 into the chains, an exact identity.
#pragma once
#include "tw_engine_generic.hpp"

namespace tw {

// index of pack_basic_view_kernel for tw_device_env::groups_per_cu (a module built with TW_DEVICE_ENV_BASIC)
constexpr int ENV_KERNEL_PACK_BASIC = 7;

constexpr uint32_t BASIC_VIEW_TABLE_BYTES = 256;     // three LayerDev entries (168 bytes) and zeros
constexpr uint32_t LAYER_DEV_WORDS = 14;
static_assert(sizeof(LayerDev) == LAYER_DEV_WORDS * 4, "pack_basic_view_kernel writes the LayerDev table word by word");

// The block: | table | b common | wm common | b action | wm action | b value | wm value |, every part on a 256-byte boundary.
// Layer 0 = common (emb -> hidden), 1 = action head (hidden -> n_actions), 2 = value head (hidden -> 1).
struct BasicViewLayout {
    uint32_t in[3], out[3];
    GenLayerShape shape[3];
    uint64_t o_b[3], o_wm[3];     // byte offsets
    uint64_t bytes;               // the whole block, a multiple of 256
};
__host__ __device__ inline BasicViewLayout basic_view_layout(uint32_t emb, uint32_t hidden, uint32_t n_actions)
{
    BasicViewLayout L;
    L.in[0] = emb; L.out[0] = hidden; L.in[1] = hidden; L.out[1] = n_actions; L.in[2] = hidden; L.out[2] = 1u;
    uint64_t cur = BASIC_VIEW_TABLE_BYTES;
    for (int l = 0; l < 3; ++l) {
        L.shape[l] = gen_layer_shape(L.in[l], L.out[l]);
        L.o_b[l] = cur;  cur = (cur + L.shape[l].b_bytes + 255u) / 256u * 256u;
        L.o_wm[l] = cur; cur = (cur + L.shape[l].wm_bytes + 255u) / 256u * 256u;
    }
    L.bytes = cur;
    return L;
}

// a policy of the MFMA shape with its natural-layout copies: what a view can be formed of
inline bool basic_view_source(const PolicyDev &p)
{
    return !p.generic && p.hidden > 0 && p.emb > 0 && p.n_actions > 0 && p.emb_rows && p.w1 && p.b1 && p.wa && p.ba && p.wv && p.bv;
}
// ... and a view itself (generic with a hidden width: tw_policy_create gives a generic stack hidden == 0)
__host__ __device__ inline bool is_basic_view(const PolicyDev &p) { return p.generic != 0 && p.hidden > 0; }

// The view of `p` over the block at `block` (device memory of basic_view_layout().bytes, or null while its address is not known: the
// sizes do not depend on it).  gen_rows*: the buffer choices of EngineV::forward for one common layer and two single-Linear heads --
// the embedding and the value head's tile in buffer 0, the common output in 1, the action head's in 2.
inline PolicyDev basic_view(const PolicyDev &p, const void *block)
{
    const BasicViewLayout L = basic_view_layout((uint32_t)p.emb, (uint32_t)p.hidden, (uint32_t)p.n_actions);
    PolicyDev v = p;
    v.generic = 1; v.n_common = 1; v.n_action = 1; v.n_value = 1; v.value_out = 1;
    const int e_rows = (int)(L.shape[0].kg * 4u);
    v.gen_rows0 = e_rows > (int)L.shape[2].row ? e_rows : (int)L.shape[2].row;
    v.gen_rows1 = (int)L.shape[0].row > (int)(L.shape[1].kg * 4u) ? (int)L.shape[0].row : (int)(L.shape[1].kg * 4u);
    v.gen_rows2 = (int)L.shape[1].row;
    v.layers = reinterpret_cast<const LayerDev *>(block);
    return v;
}

// word w of the LayerDev table (entries 0 .. 2, zeros behind them).  LayerDev::w stays null: EngineV reads wm and b alone.
__host__ __device__ inline uint32_t basic_view_table_word(const BasicViewLayout &L, const PolicyDev &pol, uint32_t w)
{
    const uint32_t e = w / LAYER_DEV_WORDS, f = w - e * LAYER_DEV_WORDS;
    if (e >= 3u) return 0u;
    const uint64_t block = reinterpret_cast<uint64_t>(pol.layers);
    uint32_t in = 0, out = 0, relu = 0;
    uint64_t b = 0, wm = 0;
    GenLayerShape s = L.shape[0];
#pragma unroll
    for (uint32_t l = 0; l < 3u; ++l)
        if (l == e) {
            in = L.in[l]; out = (L.out[l] + 3u) & ~3u; relu = l == 0u ? (uint32_t)(pol.common_relu != 0) : 0u;
            b = block + L.o_b[l]; wm = block + L.o_wm[l]; s = L.shape[l];
        }
    switch (f) {
        case 2:  return (uint32_t)b;
        case 3:  return (uint32_t)(b >> 32);
        case 4:  return in;
        case 5:  return out;
        case 6:  return relu;
        case 8:  return (uint32_t)wm;
        case 9:  return (uint32_t)(wm >> 32);
        case 10: return s.kg;
        case 11: return s.nb;
        case 12: return s.tb;
        default: return 0u;              // w (two words), pad, pad2
    }
}

// The 16 bytes at byte offset `off` (a multiple of 16) of the block, as four words: the ONE description of the block's contents,
// which pack_basic_view_kernel stores and a host program can run over host arrays (tests/test_device_env_basic_build.py holds it to
// tw_policy_create's rule that way).  No source is read outside its [in][out] elements.
__host__ __device__ inline void basic_view_quad(const BasicViewLayout &L, const PolicyDev &pol, uint64_t off, uint32_t (&v)[4])
{
    v[0] = v[1] = v[2] = v[3] = 0u;                                           // (the gaps between the parts: zeros)
    if (off < BASIC_VIEW_TABLE_BYTES) {
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) v[e] = basic_view_table_word(L, pol, (uint32_t)(off / 4u) + e);
        return;
    }
#pragma unroll
    for (uint32_t l = 0; l < 3u; ++l) {
        const float *W = l == 0u ? pol.w1 : l == 1u ? pol.wa : pol.wv;
        const float *B = l == 0u ? pol.b1 : l == 1u ? pol.ba : pol.bv;
        const uint32_t in = L.in[l], out = L.out[l];
        const GenLayerShape s = L.shape[l];
        if (off >= L.o_b[l] && off < L.o_b[l] + s.b_bytes) {                  // the bias, 0 beyond the layer's outputs
            const uint32_t o0 = (uint32_t)((off - L.o_b[l]) / 4u);
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) v[e] = o0 + e < out ? __builtin_bit_cast(uint32_t, B[o0 + e]) : 0u;
        } else if (off >= L.o_wm[l] && off < L.o_wm[l] + s.wm_bytes) {        // the image: -0.0 where the input or the output does not
            const uint64_t f0 = (off - L.o_wm[l]) / 4u;                       // exist -- the padding, the k-groups of read slack, the tail
            const uint32_t k = (uint32_t)(f0 / s.row), d0 = (uint32_t)(f0 - (uint64_t)k * s.row);
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) {
                const uint32_t d = d0 + e, t = d % s.tb, i = (d / s.tb) & 15u, b = d / (s.tb * 16u);
                const uint32_t o = (b * s.tb + t) * 16u + i;
                v[e] = (k < in && o < out) ? __builtin_bit_cast(uint32_t, W[(size_t)k * out + o]) : 0x80000000u;
            }
        }
    }
}

#ifdef TW_DEVICE_ENV_BASIC

// One thread per 16 bytes of the block, grid-stride: the four words are gathered (a row of the image is a permutation of a row of the
// natural array: element (b, i, t) of input k is output (b * tb + t) * 16 + i, so the 16 lanes of a tile row read 64 contiguous bytes
// per word) and leave as ONE 16-byte store, consecutive lanes on consecutive addresses.  No LDS: at most a few hundred KiB move, once
// per call.  Nothing outside [block, block + L.bytes) is written.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) pack_basic_view_kernel(const PolicyDev pol)
{
    const BasicViewLayout L = basic_view_layout((uint32_t)pol.emb, (uint32_t)pol.hidden, (uint32_t)pol.n_actions);
    uint8_t *block = reinterpret_cast<uint8_t *>(const_cast<LayerDev *>(pol.layers));
    const uint64_t quads = L.bytes / 16u;
    for (uint64_t q = (uint64_t)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * THREADS) {
        uint32_t v[4];
        basic_view_quad(L, pol, q * 16u, v);
        typedef uint32_t u4v __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u4v *>(block + q * 16u) = u4v{v[0], v[1], v[2], v[3]};
    }
}

// What a launcher of a module built with TW_DEVICE_ENV_BASIC does in front of its f32 kernel when the policy is a view: refuses a view
// without its block or its sources (hipErrorInvalidValue, before any HIP call) and packs the block on stream s -- in front of EVERY
// launch.  Its grid: one thread per 16 bytes, at most 1,024 workgroups.  Any other policy: nothing, hipSuccess.
inline int pack_basic_view_for(const PolicyDev &pol, hipStream_t s)
{
    if (!is_basic_view(pol)) return (int)hipSuccess;
    if (!pol.layers || !pol.w1 || !pol.b1 || !pol.wa || !pol.ba || !pol.wv || !pol.bv || pol.emb < 1 || pol.n_actions < 1 ||
        pol.n_common != 1 || pol.n_action != 1 || pol.n_value != 1 || (reinterpret_cast<uint64_t>(pol.layers) & 15u))
        return (int)hipErrorInvalidValue;
    const BasicViewLayout L = basic_view_layout((uint32_t)pol.emb, (uint32_t)pol.hidden, (uint32_t)pol.n_actions);
    uint64_t pb = (L.bytes / 16u + 255u) / 256u;
    if (pb > 1024u) pb = 1024u;
    hipLaunchKernelGGL((pack_basic_view_kernel<256>), dim3((unsigned)pb), dim3(256), 0, s, pol);
    return (int)hipGetLastError();
}

// tw_device_env::groups_per_cu, kernel 7.  With out == nullptr the question is only whether the module HOLDS the pack kernel (the
// library's dispatch, DeviceEnv.basic): answered without the HIP runtime
inline int groups_per_cu_pack_basic(int *out)
{
    if (!out) return (int)hipSuccess;
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(out, reinterpret_cast<const void *>(&pack_basic_view_kernel<256>), 256, 0);
}

#endif  // TW_DEVICE_ENV_BASIC

}  // namespace tw
