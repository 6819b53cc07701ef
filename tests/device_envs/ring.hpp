// ring.hpp -- a test device environment deliberately unlike GridWorld: 3 actions, step-time randomness, two obs ids.
//
// A noisy walk on a ring of n positions towards a goal: action 0 steps left, 1 stays (allowed on even steps only), 2 steps right;
// with probability `noise` the move is replaced by a uniform one, drawn from tw::env_draw(seed, episode, (t << 8) | 1).  The start
// lies 1..difficulty positions from the goal (reset: draw 0).  Obs ids: [position, n + goal] (obs_size 2n).  Reward 1.0 at the
// goal, -1.0 when out of steps, else -1/n.  Parameters: [n, max_steps, difficulty, noise, bad_at]; bad_at >= 0 is the deliberately
// invalid variant: at step bad_at the second id is obs_size + episode % 5 and, in odd episodes, the first one is negative -- ids
// the collectors must refuse, naming the first they meet.
#pragma once
#include "twisterl_device_env.hpp"

struct RingWalk {
    static constexpr int NUM_ACTIONS = 3;
    static constexpr int N_OBS = 2;

    int32_t n, max_steps, diff, bad_at;
    int32_t pos, goal, t, steps_left;
    float noise;
    uint64_t seed, episode;

    __host__ __device__ int obs_size() const { return 2 * n; }
    __host__ __device__ int difficulty() const { return diff; }
    __host__ void set_difficulty(int d) { diff = d < 1 ? 1 : (d > n / 2 ? n / 2 : d); }

    __host__ bool init(const double *p, int k)
    {
        if (k != 5 || p[0] < 4 || p[0] > 1024 || p[1] < 1 || p[3] < 0.0 || p[3] > 1.0) return false;
        n = (int32_t)p[0]; max_steps = (int32_t)p[1]; noise = (float)p[3]; bad_at = (int32_t)p[4];
        set_difficulty((int)p[2]);
        pos = goal = t = 0; steps_left = max_steps; seed = episode = 0;
        return true;
    }

    __host__ __device__ void reset(uint64_t s, uint64_t e)
    {
        seed = s; episode = e;
        const tw::u32x4 w = tw::env_draw(s, e, 0u);
        goal = (int)tw::u32_below(w.x, (uint32_t)n);
        const int d = 1 + (int)tw::u32_below(w.y, (uint32_t)diff);
        pos = (w.z & 1u) ? (goal + d) % n : (goal - d + n) % n;
        t = 0; steps_left = max_steps;
    }

    __host__ __device__ void step(int action)
    {
        const tw::u32x4 w = tw::env_draw(seed, episode, ((uint32_t)t << 8) | 1u);
        if (tw::u32_to_unit(w.x) < noise) action = (int)tw::u32_below(w.y, 3u);
        pos = (pos + (action == 0 ? n - 1 : (action == 2 ? 1 : 0))) % n;
        ++t;
        steps_left = steps_left > 0 ? steps_left - 1 : 0;
    }

    __host__ __device__ uint32_t masks() const { return (t & 1) ? 5u : 7u; }
    __host__ __device__ bool is_final() const { return pos == goal || steps_left == 0; }
    __host__ __device__ bool success() const { return pos == goal; }
    __host__ __device__ float reward() const { return pos == goal ? 1.0f : (steps_left == 0 ? -1.0f : -1.0f / (float)n); }

    __host__ __device__ void observe(int *ids) const
    {
        const bool bad = bad_at >= 0 && t == bad_at;
        ids[0] = (bad && (episode & 1u)) ? -1 - (int)(episode % 7u) : pos;
        ids[1] = bad ? 2 * n + (int)(episode % 5u) : n + goal;
    }
};
