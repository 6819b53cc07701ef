// gridworld.hpp -- the reference's example environment (examples/grid_world/src/lib.rs:84-164) as a device environment
// (include/twisterl_device_env.hpp): agent, goal and trap on a W x H grid, actions up / down / left / right, reward 1.0 at the goal,
// -0.5 at the trap or out of steps, else -0.5 / steps_left; obs id of cell i = i * (W*H) + {0 empty, 1 agent, 2 goal, 3 trap}.
//
//     build_device_env("examples/device_env/gridworld.hpp", "tw_examples::GridWorld5x5", "gridworld5x5")
//     DeviceEnv(path, "gridworld5x5", params=[5, 5, 64, 1])       # width, height, max_steps, difficulty (lib.rs: GridWorld::new)
//
// The placement draws come from tw::env_draw(seed, episode, 0): word x places the agent, y the goal among the cells within
// `difficulty` steps of it (Manhattan distance, the agent's own cell excluded), z the trap on a free cell -- the reference's
// distributions (uniform choices, lib.rs:118-129), drawn by rank instead of by rejection so that reset() is a bounded loop.
#pragma once
#include "twisterl_device_env.hpp"

namespace tw_examples {

template <int W, int H>
struct GridWorld {
    static constexpr int NUM_ACTIONS = 4;
    static constexpr int N_OBS = W * H;
    static_assert(W * H >= 3, "GridWorld: at least three cells (agent, goal and trap)");

    int32_t max_steps, diff;
    int32_t ax, ay, gx, gy, tx, ty;
    int32_t steps_left;

    __host__ __device__ int obs_size() const { return N_OBS * N_OBS; }
    __host__ __device__ int difficulty() const { return diff; }
    __host__ void set_difficulty(int d) { diff = d < W + H ? (d < 0 ? 0 : d) : W + H; }    // lib.rs: set_difficulty

    __host__ bool init(const double *p, int n)                  // GridWorld::new(width, height, max_steps, difficulty)
    {
        if (n != 4 || (int)p[0] != W || (int)p[1] != H || p[2] < 1 || p[3] < 0) return false;
        max_steps = (int32_t)p[2];
        set_difficulty((int)p[3]);
        ax = ay = gx = gy = tx = ty = 0;
        steps_left = max_steps;
        return true;
    }

    __host__ __device__ void reset(uint64_t seed, uint64_t episode)                            // lib.rs:118-129
    {
        const tw::u32x4 w = tw::env_draw(seed, episode, 0u);
        const int a = (int)tw::u32_below(w.x, (uint32_t)N_OBS);
        ax = a % W; ay = a / W;
        // goal: uniform over the cells within `diff` steps of the agent, the agent's cell excluded (a difficulty of 0 leaves none:
        // the reference loops for ever there; here the goal is then a neighbour, as with difficulty 1)
        const int d = diff > 0 ? diff : 1;
        int cand = 0;
        for (int i = 0; i < N_OBS; ++i) cand += (i != a && manhattan(i, a) <= d) ? 1 : 0;
        int r = (int)tw::u32_below(w.y, (uint32_t)cand), g = 0;
        for (int i = 0; i < N_OBS; ++i) if (i != a && manhattan(i, a) <= d) { if (r == 0) { g = i; break; } --r; }
        gx = g % W; gy = g / W;
        // trap: uniform over the cells that hold neither
        int s = (int)tw::u32_below(w.z, (uint32_t)(N_OBS - 2)), tr = 0;
        for (int i = 0; i < N_OBS; ++i) if (i != a && i != g) { if (s == 0) { tr = i; break; } --s; }
        tx = tr % W; ty = tr / W;
        steps_left = max_steps;
    }

    __host__ __device__ void step(int action)                                                  // lib.rs:131-140
    {
        if (action == 0 && ay > 0) ay -= 1;
        else if (action == 1 && ay + 1 < H) ay += 1;
        else if (action == 2 && ax > 0) ax -= 1;
        else if (action == 3 && ax + 1 < W) ax += 1;
        steps_left = steps_left > 0 ? steps_left - 1 : 0;
    }

    __host__ __device__ uint32_t masks() const                                                 // lib.rs:142-149
    {
        return (ay > 0 ? 1u : 0u) | (ay + 1 < H ? 2u : 0u) | (ax > 0 ? 4u : 0u) | (ax + 1 < W ? 8u : 0u);
    }
    __host__ __device__ bool at_goal() const { return ax == gx && ay == gy; }
    __host__ __device__ bool at_trap() const { return ax == tx && ay == ty; }
    __host__ __device__ bool is_final() const { return steps_left == 0 || at_goal() || at_trap(); }
    __host__ __device__ float reward() const                                                   // lib.rs:155-159
    {
        return at_goal() ? 1.0f : (at_trap() || steps_left == 0 ? -0.5f : -0.5f / (float)steps_left);
    }
    __host__ __device__ bool success() const { return at_goal(); }

    __host__ __device__ void observe(int *ids) const                                           // lib.rs:165-167 over get_state
    {
        const int a = ay * W + ax, g = gy * W + gx, t = ty * W + tx;
        for (int i = 0; i < N_OBS; ++i) ids[i] = i * N_OBS + (i == a ? 1 : (i == t ? 3 : (i == g ? 2 : 0)));
    }

private:
    __host__ __device__ static int manhattan(int i, int j)
    {
        const int dx = i % W - j % W, dy = i / W - j / W;
        return (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    }
};

using GridWorld5x5 = GridWorld<5, 5>;
using GridWorld3x3 = GridWorld<3, 3>;

}  // namespace tw_examples
