// probe.hpp -- a test device environment that is friendly to nothing: a hash walk, templated over every corner of the struct contract
// of include/twisterl_device_env.hpp (N_OBS 1..64, NUM_ACTIONS 1..4, obs_size 1..65535, a struct of up to 1 KiB, observe / observe_n).
//
// State: obs_size, max_steps, diff, bad_at, the step counter t, a 32-bit hash h, the episode index and uint32_t hist[K].
// reset(): ONE draw, tw::env_draw(seed, episode, 0): h and every hist[i] come from it.  step(a): h = mix(LCG(h), a + 1), then
// hist[t % K] ^= h and ++t -- an index computed at run time which, with the indexed read of observe(), keeps hist alive: K = 1 stays in
// registers, a K of a few dozen and more compiles to SCRATCH memory (tests/test_device_env_matrix.py holds both to the compiled
// kernels).  step() depends on the struct and the action alone (the search contract).  observe(): id i = mix(h ^ hist[(i + t) % K], i)
// % obs_size -- unordered, repeating, anywhere in [0, obs_size).  The VAR form adds observe_n(): the same ids, of which the state has
// (h >> 17) % (N_OBS + 1): 0 and N_OBS both occur.  masks(): bits of h under (1 << A) - 1, never 0 (then one bit picked from h), so
// states with exactly one allowed action occur; the bits A .. 7 above them are garbage, which the contract lets them be.  reward(): a
// multiple of 1/8 in [-1, 0.875], exact in f32.  is_final(): t >= max_steps or (h >> 11) % (diff + 1) == 0 -- WITHOUT a `t > 0` term:
// some episodes are final at reset().  success(): a bit of h.
// Parameters: [obs_size, max_steps, difficulty, bad_at]; bad_at >= 0 is the deliberately invalid variant (as in ring.hpp): at step
// bad_at the first id is obs_size + episode % 5, which the collectors must refuse, naming the first they meet.
#pragma once
#include "twisterl_device_env.hpp"

#include <type_traits>

template <int N_OBS_, int NUM_ACTIONS_, int K>
struct ProbeFixed {
    static_assert(K >= 1, "Probe: at least one word of history");
    static constexpr int NUM_ACTIONS = NUM_ACTIONS_;
    static constexpr int N_OBS = N_OBS_;

    int32_t  obs_sz, max_steps, diff, bad_at;
    int32_t  t;
    uint32_t h;
    uint64_t episode;
    uint32_t hist[K];

    __host__ __device__ static uint32_t mix(uint32_t x, uint32_t i)
    {
        x ^= i * 0x9E3779B9u;
        x ^= x >> 16; x *= 0x7FEB352Du;
        x ^= x >> 15; x *= 0x846CA68Bu;
        x ^= x >> 16;
        return x;
    }

    __host__ __device__ int obs_size() const { return obs_sz; }
    __host__ __device__ int difficulty() const { return diff; }
    __host__ void set_difficulty(int d) { diff = d < 1 ? 1 : (d > 64 ? 64 : d); }

    __host__ bool init(const double *p, int k)
    {
        if (k != 4 || p[0] < 1 || p[0] > 65535 || p[1] < 1 || p[1] > 4096) return false;
        obs_sz = (int32_t)p[0]; max_steps = (int32_t)p[1]; bad_at = (int32_t)p[3];
        set_difficulty((int)p[2]);
        t = 0; h = 0; episode = 0;
        for (int i = 0; i < K; ++i) hist[i] = 0;
        return true;
    }

    __host__ __device__ void reset(uint64_t s, uint64_t e)
    {
        const tw::u32x4 w = tw::env_draw(s, e, 0u);
        episode = e;
        h = w.x;
        for (int i = 0; i < K; ++i) hist[i] = mix(w.y, (uint32_t)i) ^ w.z;
        t = 0;
    }

    __host__ __device__ void step(int action)
    {
        h = mix(h * 1664525u + 1013904223u, (uint32_t)action + 1u);
        hist[t % K] ^= h;                                   // (an index computed at run time)
        ++t;
    }

    __host__ __device__ uint32_t masks() const
    {
        constexpr uint32_t AM = (1u << NUM_ACTIONS) - 1u;
        const uint32_t m = (h >> 5) & AM;
        // (bits NUM_ACTIONS .. 7 are garbage: only bit i < NUM_ACTIONS means anything, and a kernel that forgets it fails)
        return (m ? m : 1u << ((h >> 9) % (uint32_t)NUM_ACTIONS)) | ((h >> 13) & 0xffu & ~AM);
    }
    __host__ __device__ float reward() const { return (float)((int)((h >> 20) & 15u) - 8) * 0.125f; }
    __host__ __device__ bool is_final() const { return t >= max_steps || (h >> 11) % (uint32_t)(diff + 1) == 0u; }
    __host__ __device__ bool success() const { return ((h >> 2) & 1u) != 0u; }

    __host__ __device__ void observe(int *ids) const
    {
#pragma unroll
        for (int i = 0; i < N_OBS; ++i) ids[i] = (int)(mix(h ^ hist[(i + t) % K], (uint32_t)i) % (uint32_t)obs_sz);
        if (bad_at >= 0 && t == bad_at) ids[0] = obs_sz + (int)(episode % 5u);
    }
};

// the same, with observations of variable length: the first (h >> 17) % (N_OBS + 1) of observe()'s ids
template <int N_OBS_, int NUM_ACTIONS_, int K>
struct ProbeVar : ProbeFixed<N_OBS_, NUM_ACTIONS_, K> {
    __host__ __device__ int observe_n(int *ids) const
    {
        this->observe(ids);                                 // slot i = the i-th id, all N_OBS slots
        return (int)((this->h >> 17) % (uint32_t)(N_OBS_ + 1));
    }
};

template <int N_OBS, int NUM_ACTIONS, int K, bool VAR>
using Probe = typename std::conditional<VAR, ProbeVar<N_OBS, NUM_ACTIONS, K>, ProbeFixed<N_OBS, NUM_ACTIONS, K>>::type;

// one alias per row of tests/device_env_matrix.py (build_device_env wants an identifier)
using ProbeO1A1   = Probe<1, 1, 1, false>;        // EngineV<4>
using ProbeO4A2   = Probe<4, 2, 1, false>;        // EngineV<4>
using ProbeO5A3V  = Probe<5, 3, 1, true>;         // EngineV<9>
using ProbeO9A3S  = Probe<9, 3, 24, false>;       // EngineV<9>, exactly 128 bytes: scratch
using ProbeO10A4V = Probe<10, 4, 1, true>;        // EngineV<16>
using ProbeO16A3  = Probe<16, 3, 1, false>;       // EngineV<16>
using ProbeO17A2  = Probe<17, 2, 4, false>;       // EngineV<25>
using ProbeO25A4V = Probe<25, 4, 1, true>;        // EngineV<25>
using ProbeO26A1V = Probe<26, 1, 4, true>;        // EngineV<36>
using ProbeO36A4  = Probe<36, 4, 4, false>;       // EngineV<36>
using ProbeO37A3  = Probe<37, 3, 1, false>;       // EngineV<64>
using ProbeO64A4S = Probe<64, 4, 248, false>;     // EngineV<64>, exactly 1 KiB: scratch (and too large for the search form)
using ProbeO64A2SV = Probe<64, 2, 24, true>;      // EngineV<64>, exactly 128 bytes: scratch

static_assert(sizeof(ProbeO9A3S) == 128 && sizeof(ProbeO64A2SV) == 128, "Probe: the 128-byte rows must be exactly 128 bytes");
static_assert(sizeof(ProbeO64A4S) == 1024, "Probe: the 1 KiB row must be exactly 1,024 bytes");
