// tw_big_board.hpp -- Puzzle boards of 17 .. 64 cells for the device kernels (tw_rollout_big.hip, tw_mcts_big.hip): 25 x 5 bits in a
// 128-bit integer up to 25 cells, one byte per cell in 9 / 16 registers up to 36 / 64; Env::step / reward / is_final / masks on either
// (puzzle.rs:135-181, the big_* functions: the one copy every kernel of the two files calls), and BigPuzzleEnv<NC>: such a Puzzle as a
// device environment (include/twisterl_device_env.hpp) over the same functions.  Everything here is __host__ __device__: the struct's
// host side is pinned to the oracle without a GPU, its device side to the Puzzle kernels through the env kernels of tw_rollout_env.hpp.
#pragma once
#include "tw_common.hpp"

#include <type_traits>

namespace tw {

typedef unsigned __int128 u128;
constexpr int BIG_NC = 25;               // cells of a 5-bit board; 36 and 64: byte boards

// 5 bits per cell in 128 bits: cell i holds tile (b >> 5i) & 31
struct Board5 {
    u128 b;
    __host__ __device__ static Board5 ident(int n_cells)
    {
        Board5 r; r.b = 0;
        for (int i = 0; i < n_cells; ++i) r.b |= (u128)(uint32_t)i << (5 * i);
        return r;
    }
    __host__ __device__ uint32_t cell(int i) const { return (uint32_t)(b >> (5 * i)) & 31u; }
    __host__ __device__ void slide(int zi, int ti)                                   // the tile at cell ti moves to the blank's cell zi
    {
        const u128 tile = (b >> (5 * ti)) & (u128)31;                       // cell zi holds 0
        b = (b & ~((u128)31 << (5 * ti))) | (tile << (5 * zi));
    }
    __host__ __device__ void put(int i, uint32_t tile) { b = (b & ~((u128)31 << (5 * i))) | ((u128)(tile & 31u) << (5 * i)); }
    __host__ __device__ bool operator==(const Board5 &o) const { return b == o.b; }
};

// one byte per cell, NC / 4 registers.  Cells are addressed with compile-time indices wherever the cell loop is unrolled; the two
// run-time accesses of a step select among the words (a register array indexed at run time would live in scratch)
template <int NC>
struct Board8 {
    static constexpr int NW = (NC + 3) / 4;
    uint32_t w[NW];
    __host__ __device__ static Board8 ident(int n_cells)
    {
        Board8 r;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const int i = 4 * k + c; if (i < n_cells) v |= (uint32_t)i << (8 * c); }
            r.w[k] = v;
        }
        return r;
    }
    __host__ __device__ uint32_t cell(int i) const                                   // (i: a constant after unrolling)
    {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) v = (k == (i >> 2)) ? w[k] : v;
        return (v >> (8 * (i & 3))) & 255u;
    }
    __host__ __device__ void slide(int zi, int ti)
    {
        const uint32_t tile = cell(ti);
        const uint32_t clr = ~(255u << (8 * (ti & 3))), put = tile << (8 * (zi & 3));
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            uint32_t v = w[k];
            v = (k == (ti >> 2)) ? (v & clr) : v;
            v = (k == (zi >> 2)) ? (v | put) : v;                           // cell zi holds 0
            w[k] = v;
        }
    }
    __host__ __device__ void put(int i, uint32_t tile)
    {
        const uint32_t clr = ~(255u << (8 * (i & 3))), val = (tile & 255u) << (8 * (i & 3));
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = (k == (i >> 2)) ? ((w[k] & clr) | val) : w[k];
    }
    __host__ __device__ bool operator==(const Board8 &o) const
    {
        uint32_t d = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) d |= w[k] ^ o.w[k];
        return d == 0;
    }
};

// a board from one byte per cell (solve() from a given state)
template <typename Board>
__host__ __device__ inline Board big_board_from_cells(const uint8_t *cells, int n_cells, const Board &solved)
{
    Board b = solved;                                   // (cell i of the solved board holds tile i: slide tile by tile into place would be
    for (int i = 0; i < n_cells; ++i) b.put(i, cells[i]);   //  the long way round -- every cell is simply overwritten)
    return b;
}

template <int NC> struct BoardOf { using T = Board8<NC>; };
template <> struct BoardOf<BIG_NC> { using T = Board5; };

template <typename Board>
struct BigLaneT { Board board; int32_t zx, zy, depth; };

template <typename Board>
__host__ __device__ inline void big_step(BigLaneT<Board> &s, const PuzzleConsts &c, int action)          // Env::step (puzzle.rs:135-160), as puzzle_step
{
    const int dx = (action == 2 ? 1 : 0) - (action == 0 ? 1 : 0), dy = (action == 3 ? 1 : 0) - (action == 1 ? 1 : 0);
    int nx = s.zx + dx, ny = s.zy + dy;
    const bool ok = (unsigned)nx < (unsigned)c.width && (unsigned)ny < (unsigned)c.height;
    nx = ok ? nx : s.zx; ny = ok ? ny : s.zy;
    const int zi = s.zy * c.width + s.zx, ti = ny * c.width + nx;
    s.board.slide(zi, ti);                                                  // (an illegal move: zi == ti, the board stays)
    s.zx = nx; s.zy = ny;
    s.depth = s.depth > 0 ? s.depth - 1 : 0;
}

// Env::reward / is_final / masks of such a state (puzzle.rs:162-181)
template <typename Board>
__host__ __device__ inline float big_reward(const BigLaneT<Board> &s, const Board &ident, const PuzzleConsts &c)
{
    return s.board == ident ? 1.0f : (s.depth == 0 ? -0.5f : c.r_step);
}
template <typename Board>
__host__ __device__ inline bool big_final(const BigLaneT<Board> &s, const Board &ident) { return s.depth == 0 || s.board == ident; }
template <typename Board>
__host__ __device__ inline uint32_t big_maskbits(const BigLaneT<Board> &s, const PuzzleConsts &c)
{
    return (s.zx > 0 ? 1u : 0u) | (s.zy > 0 ? 2u : 0u) | (s.zx < c.width - 1 ? 4u : 0u) | (s.zy < c.height - 1 ? 8u : 0u);
}

// The Puzzle of up to NC cells as a device environment: the per-episode state (board, blank, depth) and the constants its methods
// read.  One class of NC serves every board it can hold (6 x 4 runs as BigPuzzleEnv<25>): n_obs() is the board's own cell count.
template <int NC>
struct BigPuzzleEnv {
    static constexpr int NUM_ACTIONS = 4;
    static constexpr int N_OBS = NC;
    static constexpr int MAX_DEPTH = 0x7ffffff;                             // of every parameter and of depth_slope * difficulty
    using Board = typename BoardOf<NC>::T;

    BigLaneT<Board> st;
    Board           solved;
    PuzzleConsts    c;
    int32_t         depth_slope;

    // solved board, blank at (0, 0), depth 0
    __host__ __device__ void init(const PuzzleConsts &consts)
    {
        c = consts; depth_slope = 0;
        solved = Board::ident(c.n_cells);
        st.board = solved; st.zx = 0; st.zy = 0; st.depth = 0;
    }
    // [width, height, difficulty, depth_slope, max_depth] (Puzzle::new, puzzle.rs:34-42)
    __host__ bool init(const double *p, int n)
    {
        if (n != 5) return false;
        for (int i = 0; i < 5; ++i) if (!(p[i] >= 0 && p[i] <= MAX_DEPTH) || p[i] != (double)(int32_t)p[i]) return false;   // (NaN: no comparison holds)
        if (p[0] < 1 || p[1] < 1 || p[0] * p[1] > NC || p[4] < 1 || p[2] * p[3] > MAX_DEPTH) return false;
        PuzzleConsts k{};
        k.width = (int32_t)p[0]; k.height = (int32_t)p[1]; k.n_cells = k.width * k.height;
        k.r_step = -0.5f / (float)(uint32_t)p[4];                           // puzzle.rs:175
        init(k);
        depth_slope = (int32_t)p[3];
        set_difficulty((int)p[2]);
        return true;
    }

    __host__ __device__ int n_obs() const { return c.n_cells; }             // (a constant of the object: reset / step leave it)
    __host__ __device__ int obs_size() const { return c.n_cells * c.n_cells; }
    __host__ __device__ int difficulty() const { return c.difficulty; }
    __host__ void set_difficulty(int d)                                     // (clamped to what init() accepts)
    {
        const int top = depth_slope > 0 ? MAX_DEPTH / depth_slope : MAX_DEPTH;
        c.difficulty = d < 0 ? 0 : (d > top ? top : d); c.depth0 = depth_slope * c.difficulty;
    }

    __host__ __device__ void reset(uint64_t seed, uint64_t episode)         // Env::reset (puzzle.rs:119-133)
    {
        st.board = solved; st.zx = 0; st.zy = 0; st.depth = 0;
        for (int d = 0; d < c.difficulty; ++d) {
            const u32x4 w = rng_draw(seed, episode, (uint32_t)d, STREAM_SCRAMBLE);
            big_step(st, c, (int)u32_below(w.x, 4u));
        }
        st.depth = c.depth0;
    }
    __host__ __device__ void step(int action) { big_step(st, c, action); }
    __host__ __device__ void observe(int *ids) const                        // puzzle.rs:183-185
    {
#pragma unroll
        for (int i = 0; i < NC; ++i) if (i < c.n_cells) ids[i] = i * c.n_cells + (int)st.board.cell(i);
    }
    __host__ __device__ uint32_t masks() const { return big_maskbits(st, c); }
    __host__ __device__ float reward() const { return big_reward(st, solved, c); }
    __host__ __device__ bool is_final() const { return big_final(st, solved); }
    __host__ __device__ bool success() const { return st.board == solved; }   // puzzle.rs:179-181
};
static_assert(std::is_trivially_copyable<BigPuzzleEnv<BIG_NC>>::value && std::is_trivially_copyable<BigPuzzleEnv<64>>::value &&
              std::is_default_constructible<BigPuzzleEnv<64>>::value && sizeof(BigPuzzleEnv<64>) <= 1024,
              "BigPuzzleEnv: the contract of include/twisterl_device_env.hpp (the kernels clone it by value)");

}  // namespace tw
