// permutation.hpp -- sort a permutation of N elements by transpositions: a device environment (include/twisterl_device_env.hpp) with
// MORE than four actions, N (N - 1) / 2 of them (28 for N = 8, 10 for N = 5), so its module is built with the opt-in for 5 .. 31 actions:
//
//     build_device_env("examples/device_env/permutation.hpp", "tw_examples::Permutation8", "perm8", wide=True)
//     DeviceEnv(path, "perm8", params=[8, 16, 4])                 # N, max_steps, difficulty
//
// Action k is the k-th pair (a, b), a < b, in lexicographic order -- (0,1), (0,2), .., (N-2,N-1) -- and swaps the elements at the
// positions a and b.  The observation is one id per position, i * N + p[i] (obs_size N * N); the episode ends when the permutation is
// sorted (success, reward 1.0) or after max_steps moves; until then the reward is -1/16 per misplaced element, exact in f32.  The mask
// forbids undoing the last move (the same transposition again).  reset() starts from the identity and applies `difficulty` random
// transpositions, one tw::env_draw(seed, episode, d) each -- so a scramble may come out sorted, and such an episode is over at once.
// step() depends on the struct and the action alone.  The permutation is packed four bits per element in one 64-bit word (N <= 16): an
// array indexed by the action's positions would live in scratch memory on the device.
#pragma once
#include "twisterl_device_env.hpp"

namespace tw_examples {

template <int N>
struct Permutation {
    static_assert(N >= 3 && N <= 8, "Permutation: 3..8 elements (N (N - 1) / 2 actions, at most 31)");
    static constexpr int NUM_ACTIONS = N * (N - 1) / 2;
    static constexpr int N_OBS = N;

    int32_t  max_steps, diff;
    int32_t  steps_left, last;                                   // last: the action of the previous move, -1 at the start
    uint64_t p;                                                  // element at position i: bits 4i .. 4i + 3

    __host__ __device__ int obs_size() const { return N * N; }
    __host__ __device__ int difficulty() const { return diff; }
    __host__ void set_difficulty(int d) { diff = d < 0 ? 0 : (d > 64 ? 64 : d); }

    __host__ bool init(const double *q, int n)                   // N, max_steps, difficulty
    {
        if (n != 3 || (int)q[0] != N || q[1] < 1 || q[1] > 4096 || q[2] < 0) return false;
        max_steps = (int32_t)q[1];
        set_difficulty((int)q[2]);
        steps_left = max_steps; last = -1; p = identity();
        return true;
    }

    __host__ __device__ void reset(uint64_t seed, uint64_t episode)
    {
        p = identity();
        for (int d = 0; d < diff; ++d) swap_pair((int)tw::u32_below(tw::env_draw(seed, episode, (uint32_t)d).x, (uint32_t)NUM_ACTIONS));
        steps_left = max_steps; last = -1;
    }

    __host__ __device__ void step(int action)
    {
        swap_pair(action);
        last = action;
        steps_left = steps_left > 0 ? steps_left - 1 : 0;
    }

    __host__ __device__ uint32_t masks() const
    {
        const uint32_t all = (1u << NUM_ACTIONS) - 1u;
        return last >= 0 ? all & ~(1u << last) : all;
    }
    __host__ __device__ bool sorted() const { return p == identity(); }
    __host__ __device__ bool is_final() const { return steps_left == 0 || sorted(); }
    __host__ __device__ bool success() const { return sorted(); }
    __host__ __device__ float reward() const
    {
        int misplaced = 0;
        for (int i = 0; i < N; ++i) misplaced += at(i) != i ? 1 : 0;
        return misplaced == 0 ? 1.0f : -0.0625f * (float)misplaced;
    }
    __host__ __device__ void observe(int *ids) const
    {
        for (int i = 0; i < N; ++i) ids[i] = i * N + at(i);
    }

private:
    __host__ __device__ static constexpr uint64_t identity()
    {
        uint64_t v = 0;
        for (int i = 0; i < N; ++i) v |= (uint64_t)i << (4 * i);
        return v;
    }
    __host__ __device__ int at(int i) const { return (int)((p >> (4 * i)) & 15u); }
    // the k-th pair (a, b), a < b, in lexicographic order: swap the elements at a and b
    __host__ __device__ void swap_pair(int k)
    {
        int a = 0, b = 1;
        for (int r = 0, left = k; r < N - 1; ++r) {
            const int n = N - 1 - r;                             // pairs (r, r + 1) .. (r, N - 1)
            if (left >= 0 && left < n) { a = r; b = r + 1 + left; }
            left -= n;
        }
        const uint64_t x = ((p >> (4 * a)) ^ (p >> (4 * b))) & 15u;
        p ^= (x << (4 * a)) | (x << (4 * b));
    }
};

using Permutation8 = Permutation<8>;
using Permutation5 = Permutation<5>;

}  // namespace tw_examples
