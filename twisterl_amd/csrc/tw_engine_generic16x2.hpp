// tw_engine_generic16x2.hpp -- EngineV16x2: the split-f16 forward of EngineV's policies (tw_engine_generic.hpp: any Sequential stack,
// widths up to 512, any obs_size) on v_mfma_f32_16x16x32_f16, and the kernel that packs its weight image.  precision="fp16x2" of a
// device environment's PPO collect: f32 answers on the f16 matrix core, where EngineV16 (tw_engine_generic16.hpp) rounds.
//
// Same interface as EngineV<NC> / EngineV16<NC> (16 episode columns per 256-thread workgroup, all four waves carry every column's
// state), so tw_env_rollout_loop.hpp compiles over it unchanged.  Arithmetic = DESIGN.md §2 "Forward, split-f16 mode, generic stacks":
//   embedding  EngineV's f32 gather over the policy's f32 table (PolicyDev::emb_rows), bit-equal to EngineV's embedding output; the
//              image holds no table
//   split      every Linear operand x, weight or activation, is carried as u = 16 x (exact): hi = f16(u) RNE, lo = f16(u - f32(hi))
//   Linear     per k-group of 32 inputs and tile of 16 outputs, in this order: acc += W_hi x_hi, acc += W_hi x_lo, acc += W_lo x_hi
//              (f32 accumulation inside the MFMA; W_lo x_lo is dropped), then r = acc * 2^-8 + bias in f32, then ReLU.  The last layer
//              of a head stores r as f32, [unit][column] rows of GEN_STRIDE floats; every other layer stores the split of 16 r into two
//              LDS planes, [column][unit] binary16
// The forward is within tests/ref64.forward_f64_bound(mode="fp16x2") of float64; where every product and partial sum is exact in f32
// and lo x lo is zero it is bit-equal to the f32 engine (tests/test_gpu_device_env_fp16x2.py).
//
// Range: a term is finite only while |16 x| < 65520, so every |weight| and every |activation that feeds a Linear| must be below 4095.
// The pack kernel raises GEN16X2_ERR_RANGE in the collect's err word for a weight whose hi term is not finite (NaN included); the
// engine notes every activation whose hi term is not finite WHERE IT STORES THE SPLIT (the embedding's output and every hidden
// layer's) in a per-lane flag, and end() raises the same bit.  The library then runs the collect again with the f32 kernel
// (tw_device_env.hip): an out-of-range collect never returns what the f32 mode would not have given.
//
// The image: per layer two planes (hi, lo) of 16 w in EngineV16's A-operand order (gen16_elem), packed from the policy's f32 device
// copies by pack_generic16x2_kernel at the start of EVERY fp16x2 collect, on the collect's stream -- never stale after
// Policy.update_from_torch.  Sizes and offsets come from the gen16x2_* functions below: the library sizes the workspace segment with
// them, the pack kernel and the engine index with them.
//
// The MFMAs are the intrinsic, for the reason at the top of tw_engine_generic.hpp; build_device_env scans a module's assembly for
// MFMA hazards like every other.
#pragma once
#include "tw_engine_generic16.hpp"

namespace tw {

constexpr int GEN16X2_PF = 2;                         // k-groups of weights (two planes: 2 KiB per wave each) in flight per tile
constexpr uint32_t GEN16X2_ERR_RANGE = 16u;           // EnvRolloutArgs::err: an operand outside the range of the split terms (1, 2, 4, 8 are taken)
constexpr uint64_t GEN16X2_REQUEST = 1ull << 63;      // Gen16Image::halves of a launch_rollout16 call: run the split pack and kernel

// ---- the image's layout ---------------------------------------------------------------------------------------------------------
// | layer 0 hi | layer 0 lo | layer 1 hi | layer 1 lo | ... | GEN16_PF KiB of read slack |, offsets in halves.  A plane is EngineV16's
// layer image (gen16_layer_halves, gen16_elem): +0.0 for inputs >= in and outputs that do not exist, in both planes.
__host__ __device__ constexpr size_t gen16x2_plane_halves(uint32_t in, uint32_t out) { return gen16_layer_halves(in, out); }
__host__ __device__ constexpr size_t gen16x2_layer_halves(uint32_t in, uint32_t out) { return 2u * gen16_layer_halves(in, out); }
// where layer idx of the table `ls` starts (idx = the number of layers: where the read slack starts)
__host__ __device__ inline size_t gen16x2_layer_base(const LayerDev *ls, int idx)
{
    size_t o = 0;
    for (int l = 0; l < idx; ++l) o += gen16x2_layer_halves((uint32_t)ls[l].in, (uint32_t)ls[l].out);
    return o;
}
__host__ __device__ inline size_t gen16x2_image_halves(const LayerDev *ls, int n_layers)
{
    return gen16x2_layer_base(ls, n_layers) + (size_t)GEN16_PF * 512u;
}

// the split of one f32 operand: hi, lo of 16 x; false when hi is not finite (|x| >= 4095, or a NaN)
__host__ __device__ __forceinline__ bool gen16x2_split(float x, _Float16 &hi, _Float16 &lo)
{
    const float u = 16.0f * x;
    hi = (_Float16)u;
    lo = (_Float16)(u - (float)hi);
    return __builtin_fabsf(u) < 65520.0f;
}

// f32 device copies -> the image.  One thread per weight (both planes), grid-stride; reads the layer table on the device.  A weight
// without a finite hi term raises GEN16X2_ERR_RANGE in *err (the collect's err word, zeroed by the library before the launch).
template <int THREADS>
__global__ void __launch_bounds__(THREADS) pack_generic16x2_kernel(const PolicyDev pol, const Gen16Image im, uint32_t *err)
{
    const size_t stride = (size_t)gridDim.x * THREADS, first = (size_t)blockIdx.x * THREADS + threadIdx.x;
    const int n_layers = pol.n_common + pol.n_action + pol.n_value;
    size_t base = 0;
    bool bad = false;
    for (int l = 0; l < n_layers; ++l) {
        const LayerDev L = pol.layers[l];
        const uint32_t in = (uint32_t)L.in, outw = (uint32_t)L.out /* row stride of L.w: the outputs padded to four, zero columns */, op = gen16_out_pad(outw);
        const size_t n = gen16x2_plane_halves(in, outw);
        for (size_t i = first; i < n; i += stride) {
            const uint32_t k = (uint32_t)(i / op), o = (uint32_t)(i % op);
            const float w = (k < in && o < outw) ? L.w[(size_t)k * outw + o] : 0.0f;
            _Float16 hi, lo;
            if (!gen16x2_split(w, hi, lo)) bad = true;
            const size_t at = base + gen16_elem(in, k, o);
            im.img[at] = hi;
            im.img[at + n] = lo;
        }
        base += 2 * n;
    }
    for (size_t i = first; i < (size_t)GEN16_PF * 512u; i += stride) im.img[base + i] = (_Float16)0.0f;   // the slack is loaded and never used
    if (bad) atomicOr(err, GEN16X2_ERR_RANGE);
}

template <int NC>
struct EngineV16x2 {
    static constexpr int NW = 4, THREADS = 256, EPB = GEN_COLS, NS = 4;
    static constexpr bool SPLIT = true;

    PolicyDev pol;
    const _Float16 *img = nullptr;         // the image (the kernel sets it before begin1)
    uint32_t *err = nullptr;               // the collect's err word (the kernel sets it before begin1)
    bool oor = false;                      // this lane stored the split of an activation without a finite hi term
    int tid, lane, wave, j, h, g;
    _Float16 *lds0;
    float *lds_hv, *lds_ha, *lds_out, *lds_user;   // the heads' f32 outputs, [unit][column] rows of GEN_STRIDE floats as EngineV hands them over
    uint64_t boffs, bcols;                 // half offsets of the three activation buffers (hi plane; lo = hi + 16 columns) and their
                                           // column strides, 21 bits each (ONE value each, as EngineV::boffs)
    int *lds_rows;                         // [16 columns][NC] obs ids of the forward
    uint32_t *lds_loff;                    // [GEN16_MAX_LAYERS] where a layer's image starts, in units of 8 halves
    const uint8_t *perm_obs, *perm_act;
    TW_STAMP_VARS(stq[4] = {});    // cycle stamps (tw_common.hpp): embedding | common | value head | action head

    // Activations live in LDS as two binary16 planes [column][unit] per buffer, hi then lo -- a lane's eight k of a k-group are one
    // ds_read_b128 per plane -- split once where they are stored, after bias and ReLU.  Three buffers with EngineV's buffer rule, each
    // plane as EngineV16 sizes its buffers (whole k-groups, + 8 halves that spread the columns over the banks).
    // | 3 buffers x 2 planes | value head f32 | action head f32 | head outputs [16][8] | kernel use | ids | layer offsets | 512 B of read slack
    __host__ __device__ static constexpr uint32_t col_halves(int rows) { return gen16_in_pad((uint32_t)rows) + 8u; }
    __host__ __device__ static constexpr uint32_t head_rows(int units) { return gen16_out_pad((uint32_t)units); }
    __host__ __device__ static size_t lds_bytes(const PolicyDev &p)
    {
        const size_t act = (size_t)2 * GEN_COLS * (col_halves(p.gen_rows0) + col_halves(p.gen_rows1) + col_halves(p.gen_rows2)) * sizeof(_Float16);
        const size_t heads = (size_t)(head_rows(p.value_out) + head_rows(p.n_actions)) * GEN_STRIDE * sizeof(float);
        return act + heads + (GEN_COLS * 8 + 256 + GEN_COLS * NC + GEN16_MAX_LAYERS) * 4 + 512;
    }
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
        boffs = ((uint64_t)(2 * GEN_COLS * c0) << 21) | ((uint64_t)(2 * GEN_COLS * (c0 + c1)) << 42);
        bcols = (uint64_t)c0 | ((uint64_t)c1 << 21) | ((uint64_t)c2 << 42);
        lds_hv = reinterpret_cast<float *>(lds0 + (size_t)2 * GEN_COLS * (c0 + c1 + c2));
        lds_ha = lds_hv + head_rows(pol.value_out) * GEN_STRIDE;
        lds_out = lds_ha + head_rows(pol.n_actions) * GEN_STRIDE;
        lds_user = lds_out + GEN_COLS * 8;
        lds_rows = reinterpret_cast<int *>(lds_user + 256);
        lds_loff = reinterpret_cast<uint32_t *>(lds_rows + GEN_COLS * NC);
        perm_obs = pol.obs_perms; perm_act = pol.act_perms;
        // (read after the first forward's first barrier)
        if (tid < pol.n_common + pol.n_action + pol.n_value && tid < GEN16_MAX_LAYERS)
            lds_loff[tid] = (uint32_t)(gen16x2_layer_base(pol.layers, tid) >> 3);
    }
    __device__ __forceinline__ void begin2() {}
    // Range: one atomic per lane that met an activation outside the split terms' range, after the last step
    __device__ __forceinline__ void end() { if (oor) atomicOr(err, GEN16X2_ERR_RANGE); }

    __device__ __forceinline__ _Float16 *bufp(int i) const { return lds0 + (size_t)((boffs >> (21 * i)) & 0x1fffffu); }
    __device__ __forceinline__ int bufc(int i) const { return (int)((bcols >> (21 * i)) & 0x1fffffu); }

    // the split of four f32 activations of one column into the two planes at y (hi) and y + lo_off
    __device__ __forceinline__ void put_split(_Float16 *y, int lo_off, const float (&r)[4])
    {
        _Float16 hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!gen16x2_split(r[e], hi[e], lo[e])) oor = true;
        *reinterpret_cast<hx4 *>(y) = hx4{hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<hx4 *>(y + lo_off) = hx4{lo[0], lo[1], lo[2], lo[3]};
    }
    __device__ __forceinline__ static void put_zero(_Float16 *y, int lo_off)
    {
        const hx4 z = hx4{(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
        *reinterpret_cast<hx4 *>(y) = z;
        *reinterpret_cast<hx4 *>(y + lo_off) = z;
    }

    // TB tiles of 16 outputs from tile0 on, all k-groups: per k-group 2 TB weight loads (16 bytes per lane: one MFMA's A operand, hi
    // and lo), TWO LDS reads (the B operands: lane = (kq, jj) holds x[32 g + 8 kq .. + 7] of column jj, hi and lo) and 3 TB MFMAs --
    // product by product over the tiles, so that a tile's three MFMAs are TB - 1 independent ones apart, and per tile in the spec's
    // order.  Weights and activations are requested GEN16X2_PF k-groups ahead; beyond the last k-group that reads the next tile's
    // weights (the image's slack behind the last one) and the next column's units (the LDS allocation's slack), never used.
    // D: lane holds column jj, outputs 4 kq .. 4 kq + 3 of each tile.
    template <int TB>
    __device__ __forceinline__ void tiles(const LayerDev &L, const _Float16 *wl, int KG, int tile0, const _Float16 *x, int xc, _Float16 *y, int yc,
                                          float *yf, bool zero_next)
    {
        typedef float f4v __attribute__((ext_vector_type(4)));
        constexpr int PF = GEN16X2_PF;
        const int kq = lane >> 4, jj = lane & 15;
        f4v acc[TB];
#pragma unroll
        for (int t = 0; t < TB; ++t) acc[t] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
        ghx8 *wq = (ghx8 *)(wl + gen16_elem((uint32_t)L.in, 8u * (uint32_t)kq, 16u * (uint32_t)tile0 + (uint32_t)jj));
        const size_t ts = (size_t)KG * 64;                                          // hx8 per tile
        const size_t wlo = gen16x2_plane_halves((uint32_t)L.in, (uint32_t)L.out) >> 3;   // hx8 from a weight's hi term to its lo term
        const hx8 *xq = reinterpret_cast<const hx8 *>(x + jj * xc + 8 * kq);         // (4 hx8 per k-group)
        const int xlo = (GEN_COLS * xc) >> 3;                                        // hx8 from an activation's hi term to its lo term
        hx8 wh[PF][TB], wo[PF][TB], xh[PF], xo[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
#pragma unroll
            for (int t = 0; t < TB; ++t) { wh[i][t] = wq[t * ts + i * 64]; wo[i][t] = wq[wlo + t * ts + i * 64]; }
            xh[i] = xq[i * 4]; xo[i] = xq[xlo + i * 4];
        }
        wq += PF * 64; xq += PF * 4;
        int g0 = 0;
        for (; g0 + PF <= KG; g0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i][t], xh[i], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i][t], xo[i], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wo[i][t], xh[i], acc[t], 0, 0, 0);
                xh[i] = xq[i * 4]; xo[i] = xq[xlo + i * 4];
#pragma unroll
                for (int t = 0; t < TB; ++t) { wh[i][t] = wq[t * ts + i * 64]; wo[i][t] = wq[wlo + t * ts + i * 64]; }
            }
            wq += PF * 64; xq += PF * 4;
        }
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            if (g0 + i < KG) {
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i][t], xh[i], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i][t], xo[i], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TB; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wo[i][t], xh[i], acc[t], 0, 0, 0);
            }
        }
        const int ylo = GEN_COLS * yc;
#pragma unroll
        for (int t = 0; t < TB; ++t) {
            const int o0 = (tile0 + t) * 16 + 4 * kq;
            const fx4 bb = *(const gfx4 *)(L.b + o0);                                // (zero beyond the layer's outputs)
            // both operands carried 16 x: the products are 256 times the layer's (an exact scale), the f32 bias is added last
            float r[4] = {acc[t][0] * 0.00390625f + bb.x, acc[t][1] * 0.00390625f + bb.y, acc[t][2] * 0.00390625f + bb.z, acc[t][3] * 0.00390625f + bb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (L.relu) r[e] = r[e] > 0.0f ? r[e] : 0.0f;
            if (yf) {                                                                // a head's last layer: f32, never split
#pragma unroll
                for (int e = 0; e < 4; ++e) yf[(o0 + e) * GEN_STRIDE + jj] = r[e];
            } else
                put_split(y + jj * yc + o0, ylo, r);
        }
        // an odd number of tiles: the next layer's last k-group reads 16 units more than this layer writes, in both planes
        if (!yf && zero_next) put_zero(y + jj * yc + (tile0 + TB) * 16 + 4 * kq, ylo);
    }

    // one Linear for the 16 columns on waves w0 .. w0 + nwv - 1: blocks of four tiles wave by wave, then the one to three tiles that
    // are left on the next wave.  (No barrier: the caller publishes the output.)
    __device__ __forceinline__ void layer_on(int idx, int src, int dst, float *yf, int w0, int nwv)
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
    // when that is given.  Returns the buffer its (split) output went to.
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
        // EmbeddingBag: EngineV's gather over the f32 table -- the f32 bias plus the rows in id order, then ReLU (thread t gathers for
        // column t >> 4 the output quads t & 15, + 16, ..) -- bit-equal to EngineV's; the split of 16 x is stored
        TW_STAMP(c0);
        const int E = pol.emb;
        const float *tab = pol.emb_rows;
        const float *bias = tab + (size_t)pol.obs_size * E;
        if (g == 0) {
#pragma unroll
            for (int i = 0; i < NC; ++i) lds_rows[j * NC + i] = rowoff[i];
        }
        __syncthreads();
        const int col = tid >> 4, ql = tid & 15;
        const int nq = E / 4;
        _Float16 *y0 = bufp(0) + col * bufc(0);
        const int y0lo = GEN_COLS * bufc(0);
        auto put = [&](int q, fx4 a) {
            if (pol.emb_relu) { a.x = a.x > 0.0f ? a.x : 0.0f; a.y = a.y > 0.0f ? a.y : 0.0f; a.z = a.z > 0.0f ? a.z : 0.0f; a.w = a.w > 0.0f ? a.w : 0.0f; }
            const float r[4] = {a.x, a.y, a.z, a.w};
            put_split(y0 + 4 * q, y0lo, r);
        };
        if constexpr (NC <= 25) {
        int ro[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) ro[i] = lds_rows[col * NC + i];
        constexpr int QT = NC > 16 ? 1 : (NC > 9 ? 2 : 4);     // QT x NC row quads are in flight per lane, as in EngineV
        for (int q0 = ql; q0 < nq; q0 += 16 * QT) {
            int qs[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) qs[u] = q0 + 16 * u < nq ? q0 + 16 * u : q0;  // (past the end: a repeat of the trip's first quad)
            fx4 r[QT][NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const float *row = tab + (size_t)(ro[i] >= 0 ? ro[i] : 0) * E;
#pragma unroll
                for (int u = 0; u < QT; ++u) r[u][i] = *(const gfx4 *)(row + 4 * qs[u]);
            }
            fx4 a[QT];
#pragma unroll
            for (int u = 0; u < QT; ++u) a[u] = *(const gfx4 *)(bias + 4 * qs[u]);
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                if (ro[i] >= 0) {
#pragma unroll
                    for (int u = 0; u < QT; ++u) { a[u].x = a[u].x + r[u][i].x; a[u].y = a[u].y + r[u][i].y; a[u].z = a[u].z + r[u][i].z; a[u].w = a[u].w + r[u][i].w; }
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
            for (int u = 0; u < QT; ++u) a[u] = *(const gfx4 *)(bias + 4 * qs[u]);
#pragma unroll
            for (int c0 = 0; c0 < NC; c0 += CB) {
                fx4 r[QT][CB]; int ro[CB];
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    ro[i] = c0 + i < NC ? lds_rows[col * NC + c0 + i] : -1;
                    const float *row = tab + (size_t)(ro[i] >= 0 ? ro[i] : 0) * E;
#pragma unroll
                    for (int u = 0; u < QT; ++u) r[u][i] = *(const gfx4 *)(row + 4 * qs[u]);
                }
#pragma unroll
                for (int i = 0; i < CB; ++i) {
                    if (ro[i] >= 0) {
#pragma unroll
                        for (int u = 0; u < QT; ++u) { a[u].x = a[u].x + r[u][i].x; a[u].y = a[u].y + r[u][i].y; a[u].z = a[u].z + r[u][i].z; a[u].w = a[u].w + r[u][i].w; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < QT; ++u) put(qs[u], a[u]);
        }
        }
        // the units between the embedding's width and the first layer's whole k-groups: zero in both planes
        for (int q = nq + ql; q < (int)(gen16_in_pad((uint32_t)E) >> 2); q += 16) put_zero(y0 + 4 * q, y0lo);
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
