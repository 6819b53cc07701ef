// tw_engine_generic16.hpp -- EngineV16: the f16-input forward of EngineV's policies (tw_engine_generic.hpp: any Sequential stack,
// widths up to 512, any obs_size) on v_mfma_f32_16x16x32_f16, and the kernel that packs its weight image.
//
// Same interface as EngineV<NC> (16 episode columns per 256-thread workgroup, all four waves carry every column's state), so the
// environment kernels of tw_rollout_env.hpp compile over either.  Arithmetic = DESIGN.md §2 "Forward, f16-input mode", which the
// oracle restates as TWO_ARITH_F16 for any depth: the EmbeddingBag output is the f32 sum, in id order, of the table rows ROUNDED TO
// binary16, then the f32 bias, then ReLU; every Linear takes its inputs and weights rounded to binary16 (RNE), multiplies exactly,
// accumulates in f32 inside the MFMA and adds the f32 bias last; the outputs of the last layer of each head stay f32 and are never
// rounded.  The accumulation order inside the MFMA is the hardware's: the forward is within tests/ref64.forward_f64_bound(mode="fp16")
// of float64, not bit-equal to the oracle (it is, where every sum is exact in f32 -- tests/test_gpu_device_env_fp16.py).
//
// The image: binary16 copies of the embedding table and of every layer's weights in A-operand order, packed from the policy's f32
// device copies (PolicyDev::emb_rows, LayerDev::w) by pack_generic16_kernel at the start of EVERY fp16 collect, on the collect's
// stream -- so it can never be stale after Policy.update_from_torch, and tw_policy_create / the device-to-device sync know nothing
// of it.  Sizes and offsets come from the gen16_* layout functions below: the library sizes the workspace segment with them, the
// pack kernel and the engine index with them.
//
// The MFMAs are the intrinsic, for the reason at the top of tw_engine_generic.hpp; a module's assembly is scanned for MFMA hazards
// by build_device_env like every other.
#pragma once
#include "tw_engine_generic.hpp"

namespace tw {

typedef _Float16 hx8 __attribute__((ext_vector_type(8)));
typedef _Float16 hx4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) hx8 ghx8;
typedef const __attribute__((address_space(1))) hx4 ghx4;

constexpr int GEN16_PF = 4;                // k-groups of weights (1 KiB per wave each) in flight per tile
constexpr int GEN16_MAX_LAYERS = 24;       // tw_policy_create: at most 8 layers per stack

// ---- the image's layout ---------------------------------------------------------------------------------------------------------
// | table [obs_size][emb], padded to 8 halves | layer 0 | layer 1 | ... | GEN16_PF KiB of read slack |, offsets in halves.
// A layer of `in` inputs and `out` outputs is [out_pad16 / 16 tiles][in_pad32 / 32 k-groups][64 lanes][8]: the eight halves of a
// lane are ONE MFMA's A operand (lane l holds A[row l & 15][k = 8 (l >> 4) + i]: row = the tile's output, k = the k-group's input),
// a tile's k-groups follow each other (a wave streams a tile's weights with one 16-byte load per lane and MFMA, 512 halves per
// k-group), weights of inputs >= in and of outputs that do not exist are +0.0.
__host__ __device__ constexpr uint32_t gen16_in_pad(uint32_t in) { return (in + 31u) & ~31u; }
__host__ __device__ constexpr uint32_t gen16_out_pad(uint32_t out) { return (out + 15u) & ~15u; }
__host__ __device__ constexpr size_t gen16_table_halves(uint32_t obs_size, uint32_t emb) { return ((size_t)obs_size * emb + 7u) & ~(size_t)7u; }
__host__ __device__ constexpr size_t gen16_layer_halves(uint32_t in, uint32_t out) { return (size_t)gen16_in_pad(in) * gen16_out_pad(out); }
// where weight (input k, output o) of a layer with `in` inputs sits inside the layer's image; k < in_pad32, o < out_pad16
__host__ __device__ constexpr size_t gen16_elem(uint32_t in, uint32_t k, uint32_t o)
{
    return ((size_t)(o >> 4) * (gen16_in_pad(in) >> 5) + (k >> 5)) * 512u + ((((k & 31u) >> 3) * 16u + (o & 15u)) * 8u) + (k & 7u);
}
// where layer idx of the table `ls` starts (idx = the number of layers: where the read slack starts)
__host__ __device__ inline size_t gen16_layer_base(uint32_t obs_size, uint32_t emb, const LayerDev *ls, int idx)
{
    size_t o = gen16_table_halves(obs_size, emb);
    for (int l = 0; l < idx; ++l) o += gen16_layer_halves((uint32_t)ls[l].in, (uint32_t)ls[l].out);
    return o;
}
__host__ __device__ inline size_t gen16_image_halves(uint32_t obs_size, uint32_t emb, const LayerDev *ls, int n_layers)
{
    return gen16_layer_base(obs_size, emb, ls, n_layers) + (size_t)GEN16_PF * 512u;
}

// What the f16 rollout kernel needs besides EnvRolloutArgs (tw_rollout_env.hpp): the image, carved from the collect's workspace
struct Gen16Image {
    _Float16 *img;                   // gen16_image_halves() halves, 256-byte aligned
    uint64_t  halves;                // its size, as the library computed it (the launcher refuses another one)
};

// f32 device copies -> the image.  RNE (v_cvt_f16_f32 under the default rounding mode, as the oracle's two_round_f16); a value beyond
// 65504 becomes +-inf, as in the spec.  One thread per half, grid-stride; reads the layer table on the device.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) pack_generic16_kernel(const PolicyDev pol, const Gen16Image im)
{
    const size_t stride = (size_t)gridDim.x * THREADS, first = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const size_t tab = (size_t)pol.obs_size * (size_t)pol.emb, tab_pad = gen16_table_halves((uint32_t)pol.obs_size, (uint32_t)pol.emb);
    for (size_t i = first; i < tab_pad; i += stride) im.img[i] = i < tab ? (_Float16)pol.emb_rows[i] : (_Float16)0.0f;
    const int n_layers = pol.n_common + pol.n_action + pol.n_value;
    size_t base = tab_pad;
    for (int l = 0; l < n_layers; ++l) {
        const LayerDev L = pol.layers[l];
        const uint32_t in = (uint32_t)L.in, outw = (uint32_t)L.out /* row stride of L.w: the outputs padded to four, zero columns */, op = gen16_out_pad(outw);
        const size_t n = gen16_layer_halves(in, outw);
        for (size_t i = first; i < n; i += stride) {
            const uint32_t k = (uint32_t)(i / op), o = (uint32_t)(i % op);
            const float w = (k < in && o < outw) ? L.w[(size_t)k * outw + o] : 0.0f;
            im.img[base + gen16_elem(in, k, o)] = (_Float16)w;
        }
        base += n;
    }
    for (size_t i = first; i < (size_t)GEN16_PF * 512u; i += stride) im.img[base + i] = (_Float16)0.0f;   // the slack is loaded and never used
}

template <int NC>
struct EngineV16 {
    static constexpr int NW = 4, THREADS = 256, EPB = GEN_COLS, NS = 4;
    static constexpr bool SPLIT = true;

    PolicyDev pol;
    const _Float16 *img = nullptr;         // the image (the kernel sets it before begin1)
    int tid, lane, wave, j, h, g;
    _Float16 *lds0;
    float *lds_hv, *lds_ha, *lds_out, *lds_user;   // the heads' f32 outputs, [unit][column] rows of GEN_STRIDE floats as EngineV hands them over
    uint64_t boffs, bcols;                 // half offsets and column strides of the three activation buffers, 21 bits each (ONE value
                                           // each, as EngineV::boffs: three adjacent members were indexed in memory)
    int *lds_rows;                         // [16 columns][NC] obs ids of the forward
    uint32_t *lds_loff;                    // [GEN16_MAX_LAYERS] where a layer's image starts, in units of 8 halves
    const uint8_t *perm_obs, *perm_act;
    TW_STAMP_VARS(stq[4] = {});    // cycle stamps (tw_common.hpp): embedding | common | value head | action head

    // Activations live in LDS as binary16 [column][unit] -- a lane's eight k of a k-group are one ds_read_b128 -- rounded once where they
    // are stored, after bias and ReLU.  Three buffers with EngineV's buffer rule (stack()), each as many units as the widest layer
    // it ever holds (PolicyDev::gen_rows*), up to a multiple of 32 (a layer reads whole k-groups; what it reads beyond its inputs is
    // zeroed where the buffer is written) plus 8 halves, which spreads the columns over the banks.
    // | 3 buffers | value head f32 | action head f32 | head outputs [16][8] | kernel use | ids | layer offsets | 512 B of read slack
    __host__ __device__ static constexpr uint32_t col_halves(int rows) { return gen16_in_pad((uint32_t)rows) + 8u; }
    __host__ __device__ static constexpr uint32_t head_rows(int units) { return gen16_out_pad((uint32_t)units); }
    __host__ __device__ static size_t lds_bytes(const PolicyDev &p)
    {
        const size_t act = (size_t)GEN_COLS * (col_halves(p.gen_rows0) + col_halves(p.gen_rows1) + col_halves(p.gen_rows2)) * sizeof(_Float16);
        const size_t heads = (size_t)(head_rows(p.value_out) + head_rows(p.n_actions)) * GEN_STRIDE * sizeof(float);
        return act + heads + (GEN_COLS * 8 + 256 + GEN_COLS * NC + GEN16_MAX_LAYERS) * 4 + 512;
    }
    // the same in floats, as EngineV::lds_floats: where a kernel's own LDS starts behind the engine's (every term above is a multiple of 4 bytes)
    __host__ __device__ static size_t lds_floats(const PolicyDev &p) { return lds_bytes(p) / sizeof(float); }
    __device__ __forceinline__ bool primary() const { return wave == 0; }
    __device__ __forceinline__ int  ep_lane() const { return j; }
    __device__ __forceinline__ bool owns_lane() const { return wave == j / (EPB / NS); }

    __device__ __forceinline__ void begin1(const PolicyDev &p, float *lds)
    {
        pol = p;
        tid = threadIdx.x; lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        j = lane & 15; h = lane >> 4; g = tid >> 4;
        lds0 = reinterpret_cast<_Float16 *>(lds);
        const uint32_t c0 = col_halves(pol.gen_rows0), c1 = col_halves(pol.gen_rows1), c2 = col_halves(pol.gen_rows2);
        boffs = ((uint64_t)(GEN_COLS * c0) << 21) | ((uint64_t)(GEN_COLS * (c0 + c1)) << 42);
        bcols = (uint64_t)c0 | ((uint64_t)c1 << 21) | ((uint64_t)c2 << 42);
        lds_hv = reinterpret_cast<float *>(lds0 + (size_t)GEN_COLS * (c0 + c1 + c2));
        lds_ha = lds_hv + head_rows(pol.value_out) * GEN_STRIDE;
        lds_out = lds_ha + head_rows(pol.n_actions) * GEN_STRIDE;
        lds_user = lds_out + GEN_COLS * 8;
        lds_rows = reinterpret_cast<int *>(lds_user + 256);
        lds_loff = reinterpret_cast<uint32_t *>(lds_rows + GEN_COLS * NC);
        perm_obs = pol.obs_perms; perm_act = pol.act_perms;
        // (read after the first forward's first barrier)
        if (tid < pol.n_common + pol.n_action + pol.n_value && tid < GEN16_MAX_LAYERS)
            lds_loff[tid] = (uint32_t)(gen16_layer_base((uint32_t)pol.obs_size, (uint32_t)pol.emb, pol.layers, tid) >> 3);
    }
    __device__ __forceinline__ void begin2() {}
    __device__ __forceinline__ void end() {}

    __device__ __forceinline__ _Float16 *bufp(int i) const { return lds0 + (size_t)((boffs >> (21 * i)) & 0x1fffffu); }
    __device__ __forceinline__ int bufc(int i) const { return (int)((bcols >> (21 * i)) & 0x1fffffu); }

    // TB tiles of 16 outputs from tile0 on, all k-groups: per k-group TB weight loads (16 bytes per lane: one MFMA's A operand), ONE
    // LDS read (the B operand: lane = (kq, jj) holds x[32 g + 8 kq .. + 7] of column jj) and TB MFMAs.  Weights and activations are
    // requested GEN16_PF k-groups ahead; beyond the last k-group that reads the next tile's weights (the image's slack behind the
    // last one) and the next column's units (the LDS allocation's slack behind the last one), never used.
    // D: lane holds column jj, outputs 4 kq .. 4 kq + 3 of each tile -- the layout EngineV::layer_tb stores from.
    template <int TB>
    __device__ __forceinline__ void tiles(const LayerDev &L, const _Float16 *wl, int KG, int tile0, const _Float16 *x, int xc, _Float16 *y, int yc,
                                          float *yf, bool zero_next) const
    {
        typedef float f4v __attribute__((ext_vector_type(4)));
        constexpr int PF = GEN16_PF;
        const int kq = lane >> 4, jj = lane & 15;
        f4v acc[TB];
#pragma unroll
        for (int t = 0; t < TB; ++t) acc[t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
        ghx8 *wq = (ghx8 *)(wl + gen16_elem((uint32_t)L.in, 8u * (uint32_t)kq, 16u * (uint32_t)tile0 + (uint32_t)jj));
        const size_t ts = (size_t)KG * 64;                                          // hx8 per tile
        const hx8 *xq = reinterpret_cast<const hx8 *>(x + jj * xc + 8 * kq);         // (4 hx8 per k-group)
        hx8 w[PF][TB], xv[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
#pragma unroll
            for (int t = 0; t < TB; ++t) w[i][t] = wq[t * ts + i * 64];
            xv[i] = xq[i * 4];
        }
        wq += PF * 64; xq += PF * 4;
        int g0 = 0;
        for (; g0 + PF <= KG; g0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[i][t], xv[i], acc[t], 0, 0, 0);
                xv[i] = xq[i * 4];
#pragma unroll
                for (int t = 0; t < TB; ++t) w[i][t] = wq[t * ts + i * 64];
            }
            wq += PF * 64; xq += PF * 4;
        }
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            if (g0 + i < KG) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[i][t], xv[i], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            const int o0 = (tile0 + t) * 16 + 4 * kq;
            const fx4 bb = *(const gfx4 *)(L.b + o0);                                // (zero beyond the layer's outputs)
            float r[4] = {acc[t][0] + bb.x, acc[t][1] + bb.y, acc[t][2] + bb.z, acc[t][3] + bb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (L.relu) r[e] = r[e] > 0.0f ? r[e] : 0.0f;
            if (yf) {                                                                // a head's last layer: f32, never rounded
#pragma unroll
                for (int e = 0; e < 4; ++e) yf[(o0 + e) * GEN_STRIDE + jj] = r[e];
            } else
                *reinterpret_cast<hx4 *>(y + jj * yc + o0) = hx4{(_Float16)r[0], (_Float16)r[1], (_Float16)r[2], (_Float16)r[3]};
        }
        // an odd number of tiles: the next layer's last k-group reads 16 units more than this layer writes
        if (!yf && zero_next) *reinterpret_cast<hx4 *>(y + jj * yc + (tile0 + TB) * 16 + 4 * kq) = hx4{(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
    }

    // one Linear for the 16 columns on waves w0 .. w0 + nwv - 1: blocks of four tiles wave by wave, then the one to three tiles that
    // are left on the next wave.  (No barrier: the caller publishes the output.)
    __device__ __forceinline__ void layer_on(int idx, int src, int dst, float *yf, int w0, int nwv) const
    {
        const LayerDev &L = pol.layers[idx];
        const int KG = (int)(gen16_in_pad((uint32_t)L.in) >> 5), T = (int)(gen16_out_pad((uint32_t)L.out) >> 4);
        const _Float16 *wl = img + ((size_t)lds_loff[idx] << 3);
        const _Float16 *x = bufp(src); _Float16 *y = bufp(dst);
        const int xc = bufc(src), yc = bufc(dst);
        const int full = T >> 2, rem = T & 3;
        if (wave < w0 || wave >= w0 + nwv) return;                                   // (wave-uniform)
        for (int b = wave - w0; b < full; b += nwv) tiles<4>(L, wl, KG, 4 * b, x, xc, y, yc, yf, false);
        if (rem != 0 && wave - w0 == full % nwv) {
            const bool zn = (T & 1) != 0;
            switch (rem) {
                case 1: tiles<1>(L, wl, KG, 4 * full, x, xc, y, yc, yf, zn); break;
                case 2: tiles<2>(L, wl, KG, 4 * full, x, xc, y, yc, yf, zn); break;
                default: tiles<3>(L, wl, KG, 4 * full, x, xc, y, yc, yf, zn); break;
            }
        }
    }

    // runs layers first .. first + n - 1 from buffer `src` with EngineV's buffer rule (never `keep`); the last one stores f32 to `yf`
    // when that is given.  Returns the buffer its (binary16) output went to.
    __device__ __forceinline__ int stack(int first, int n, int src, int keep, float *yf)
    {
        int cur = src;
        for (int l = 0; l < n; ++l) {
            int dst = 0;
            while (dst == cur || dst == keep) ++dst;
            layer_on(first + l, cur, dst, l == n - 1 ? yf : nullptr, 0, NW);
            __syncthreads();
            cur = dst;
        }
        return cur;
    }

    // as EngineV::forward_head: the action head's f32 outputs where they are, [unit][column] rows of GEN_STRIDE floats, valid until
    // the next forward starts
    __device__ __forceinline__ const float *forward_head(const int (&rowoff)[NC], float &value)
    {
        float none[4];
        return forward<true>(rowoff, none, value);
    }

    template <bool HEAD_IN_PLACE = false>
    __device__ __forceinline__ const float *forward(const int (&rowoff)[NC], float (&lg)[4], float &value)
    {
        // EmbeddingBag: f32 sum of the binary16 table rows in id order, then the f32 bias, then ReLU -- EngineV's gather (thread t
        // gathers for column t >> 4 the output quads t & 15, + 16, ..) over rows of half the bytes
        TW_STAMP(c0);
        const int E = pol.emb;
        const _Float16 *tab = img;
        const float *bias = pol.emb_rows + (size_t)pol.obs_size * E;
        if (g == 0) {
#pragma unroll
            for (int i = 0; i < NC; ++i) lds_rows[j * NC + i] = rowoff[i];
        }
        __syncthreads();
        const int col = tid >> 4, ql = tid & 15;
        const int nq = E / 4;
        _Float16 *y0 = bufp(0) + col * bufc(0);
        auto put = [&](int q, fx4 a) {
            a.x = a.x + (*(const gfx4 *)(bias + 4 * q)).x; a.y = a.y + (*(const gfx4 *)(bias + 4 * q)).y;
            a.z = a.z + (*(const gfx4 *)(bias + 4 * q)).z; a.w = a.w + (*(const gfx4 *)(bias + 4 * q)).w;
            if (pol.emb_relu) { a.x = a.x > 0.0f ? a.x : 0.0f; a.y = a.y > 0.0f ? a.y : 0.0f; a.z = a.z > 0.0f ? a.z : 0.0f; a.w = a.w > 0.0f ? a.w : 0.0f; }
            *reinterpret_cast<hx4 *>(y0 + 4 * q) = hx4{(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w};
        };
        if constexpr (NC <= 25) {
        int ro[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) ro[i] = lds_rows[col * NC + i];
        constexpr int QT = NC > 16 ? 1 : (NC > 9 ? 2 : 4);     // QT x NC row quads (two registers each) are in flight per lane
        for (int q0 = ql; q0 < nq; q0 += 16 * QT) {
            int qs[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) qs[u] = q0 + 16 * u < nq ? q0 + 16 * u : q0;  // (past the end: a repeat of the trip's first quad)
            hx4 r[QT][NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const _Float16 *row = tab + (size_t)(ro[i] >= 0 ? ro[i] : 0) * E;
#pragma unroll
                for (int u = 0; u < QT; ++u) r[u][i] = *(ghx4 *)(row + 4 * qs[u]);
            }
            fx4 a[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) a[u] = fx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                if (ro[i] >= 0) {
#pragma unroll
                    for (int u = 0; u < QT; ++u) { a[u].x = a[u].x + (float)r[u][i].x; a[u].y = a[u].y + (float)r[u][i].y; a[u].z = a[u].z + (float)r[u][i].z; a[u].w = a[u].w + (float)r[u][i].w; }
                }
            }
#pragma unroll
            for (int u = 0; u < QT; ++u) put(qs[u], a[u]);
        }
        } else {
        // 26 .. 64 ids: in blocks of 16 (the row loads of a block are in flight together, the adds stay in id order)
        constexpr int QT = 2, CB = 16;
        for (int q0 = ql; q0 < nq; q0 += 16 * QT) {
            int qs[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) qs[u] = q0 + 16 * u < nq ? q0 + 16 * u : q0;
            fx4 a[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) a[u] = fx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c0 = 0; c0 < NC; c0 += CB) {
                hx4 r[QT][CB]; int ro[CB];
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    ro[i] = c0 + i < NC ? lds_rows[col * NC + c0 + i] : -1;
                    const _Float16 *row = tab + (size_t)(ro[i] >= 0 ? ro[i] : 0) * E;
#pragma unroll
                    for (int u = 0; u < QT; ++u) r[u][i] = *(ghx4 *)(row + 4 * qs[u]);
                }
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    if (ro[i] >= 0) {
#pragma unroll
                        for (int u = 0; u < QT; ++u) { a[u].x = a[u].x + (float)r[u][i].x; a[u].y = a[u].y + (float)r[u][i].y; a[u].z = a[u].z + (float)r[u][i].z; a[u].w = a[u].w + (float)r[u][i].w; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < QT; ++u) put(qs[u], a[u]);
        }
        }
        // the units between the embedding's width and the first layer's whole k-groups: zero (0 x NaN would otherwise enter a chain)
        for (int q = nq + ql; q < (int)(gen16_in_pad((uint32_t)E) >> 2); q += 16)
            *reinterpret_cast<hx4 *>(y0 + 4 * q) = hx4{(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
        __syncthreads();
        TW_STAMP(c1);
        const int co = stack(0, pol.n_common, 0, -1, nullptr);
        TW_STAMP(c2);
        bool heads_done = false;
        if (pol.n_value == 1 && pol.n_action == 1) {
            // single-Linear heads: both at once, the value head on waves 2..3, the action head on waves 0..1 (as EngineV)
            layer_on(pol.n_common + pol.n_action, co, co, lds_hv, 2, 2);
            layer_on(pol.n_common, co, co, lds_ha, 0, 2);
            __syncthreads();
            heads_done = true;
        } else
            (void)stack(pol.n_common + pol.n_action, pol.n_value, co, co, lds_hv);
        if (g == 0) {                                                                          // .sum() of the value head's outputs
            float s = 0.0f;
            for (int i = 0; i < pol.value_out; ++i) s = s + lds_hv[i * GEN_STRIDE + j];
            lds_out[j * 8 + 4] = s;
        }
        __syncthreads();
        TW_STAMP(c3);
        if (!heads_done) (void)stack(pol.n_common, pol.n_action, co, co, lds_ha);
        value = lds_out[j * 8 + 4];
        if constexpr (HEAD_IN_PLACE) {                                                         // (both heads are behind a barrier here)
            TW_STAMP(c4);
            TW_STAMP_ADD(stq[0], c0, c1); TW_STAMP_ADD(stq[1], c1, c2); TW_STAMP_ADD(stq[2], c2, c3); TW_STAMP_ADD(stq[3], c3, c4);
            return lds_ha;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) lg[i] = lds_ha[i * GEN_STRIDE + j];                        // (16 rows at least: zero beyond the actions)
        TW_STAMP(c4);
        TW_STAMP_ADD(stq[0], c0, c1); TW_STAMP_ADD(stq[1], c1, c2); TW_STAMP_ADD(stq[2], c2, c3); TW_STAMP_ADD(stq[3], c3, c4);
        __syncthreads();           // (the buffers and the heads' outputs are rewritten by the next forward)
        return nullptr;
    }
};

}  // namespace tw
