// lamps.hpp -- a test device environment whose observations VARY IN LENGTH: observe_n() returns the ids of the lit lamps.
//
// N lamps in a row (a bit mask), a cursor and a step budget.  Action 0 toggles the lamp under the cursor, 1 that lamp and the one half
// a row away (both advance the cursor), 2 moves the cursor three lamps on (not allowed on odd steps), 3 inverts every lamp.  All lamps
// off is final and a success -- its observation is EMPTY --, an exhausted budget is final too.  reset() starts from all-off, plays
// 1..difficulty uniform moves (draws 1, 2, ..) and puts the cursor back; the budget is 3..max_steps (draw 0), so episodes end at many
// lengths.  Obs id of lit lamp b at step t: N * b + t % N, ascending in b (obs_size N * N).  Reward 1.0 when all are off, -0.5 out of
// budget, else -0.01 per lit lamp.  Parameters: [max_steps, difficulty, bad_at, bad_kind]; bad_at >= 0 is the deliberately invalid
// variant, from step bad_at on (two steps later in every third episode, so that the first occurrence is NOT in the first episode):
// bad_kind 1 replaces the first id (where there is one) by obs_size + episode % 5, in odd episodes by a negative one; bad_kind 2
// returns a count of N + 1 -- what the collectors must refuse, naming the first they meet.
// observe_n() writes slot i with the i-th lit lamp, all N slots, by indices that are constants after unrolling: no scratch memory.
#pragma once
#include "twisterl_device_env.hpp"

template <int N>
struct Lamps {
    static_assert(N >= 4 && N <= 64, "Lamps: 4..64 lamps");
    static constexpr int NUM_ACTIONS = 4;
    static constexpr int N_OBS = N;

    uint64_t mask, seed, episode;
    int32_t  max_steps, diff, bad_at, bad_kind;
    int32_t  cur, t, steps_left, pad;

    __host__ __device__ static uint64_t full() { return N == 64 ? ~0ull : ((1ull << N) - 1ull); }
    __host__ __device__ int obs_size() const { return N * N; }
    __host__ __device__ int difficulty() const { return diff; }
    __host__ void set_difficulty(int d) { diff = d < 1 ? 1 : (d > 16 ? 16 : d); }

    __host__ bool init(const double *p, int k)
    {
        if (k != 4 || p[0] < 3 || p[0] > 4096 || p[3] < 0 || p[3] > 2) return false;
        max_steps = (int32_t)p[0]; bad_at = (int32_t)p[2]; bad_kind = (int32_t)p[3];
        set_difficulty((int)p[1]);
        mask = seed = episode = 0; cur = t = pad = 0; steps_left = max_steps;
        return true;
    }

    __host__ __device__ void apply(int action)
    {
        if (action == 0) { mask ^= 1ull << cur; cur = (cur + 1) % N; }
        else if (action == 1) { mask ^= (1ull << cur) | (1ull << ((cur + N / 2) % N)); cur = (cur + 1) % N; }
        else if (action == 2) cur = (cur + 3) % N;
        else mask ^= full();
    }

    __host__ __device__ void reset(uint64_t s, uint64_t e)
    {
        seed = s; episode = e;
        const tw::u32x4 w = tw::env_draw(s, e, 0u);
        const int moves = 1 + (int)tw::u32_below(w.x, (uint32_t)diff);
        mask = 0; cur = 0;
        for (int i = 0; i < moves; ++i) apply((int)tw::u32_below(tw::env_draw(s, e, 1u + (uint32_t)i).x, 4u));
        cur = 0; t = 0;
        steps_left = 3 + (int)tw::u32_below(w.y, (uint32_t)(max_steps - 2));
    }

    __host__ __device__ void step(int action)
    {
        apply(action);
        ++t;
        steps_left = steps_left > 0 ? steps_left - 1 : 0;
    }

    __host__ __device__ uint32_t masks() const { return (t & 1) ? 11u : 15u; }
    __host__ __device__ bool is_final() const { return mask == 0 || steps_left == 0; }
    __host__ __device__ bool success() const { return mask == 0; }
    __host__ __device__ float reward() const
    {
        return mask == 0 ? 1.0f : (steps_left == 0 ? -0.5f : -0.01f * (float)__builtin_popcountll(mask));
    }

    __host__ __device__ int observe_n(int *ids) const
    {
        uint64_t m = mask;
        const int k = __builtin_popcountll(m), phase = t % N;
#pragma unroll
        for (int i = 0; i < N; ++i) {                       // slot i: the i-th lit lamp (slots past the count are not read)
            const int b = m ? __builtin_ctzll(m) : 0;
            ids[i] = N * b + phase;
            m &= m - 1ull;
        }
        const bool bad = bad_at >= 0 && t >= bad_at + (episode % 3u == 0 ? 2 : 0);
        if (bad && bad_kind == 1 && k > 0) ids[0] = (episode & 1u) ? -1 - (int)(episode % 7u) : N * N + (int)(episode % 5u);
        return bad && bad_kind == 2 ? N + 1 : k;
    }
};

using Lamps12 = Lamps<12>;       // EngineV<16>: the gather that holds every row of a column in registers
using Lamps40 = Lamps<40>;       // EngineV<64>: the gather in blocks of 16 rows
