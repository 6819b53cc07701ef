// wide_open.hpp -- the hash walk of probe.hpp with 31 actions that are ALL allowed in every state, for the search kernel of
// TW_DEVICE_ENV_WIDE_SEARCH (tests/device_env_wide_search.py).  wide.hpp's masks almost never allow all 31 actions, so a root there
// never has 31 children; here every node that is expanded gets one child per action whose prior is above zero -- with a finite head all
// 31 -- and a search of more than 31 iterations can visit every child of the root.  The bit 31 above the actions is garbage, which the
// contract lets it be.
// WideShutA7 is the opposite corner: seven actions of which one state in four allows NONE (only garbage above bit 6).  A root of such a
// state has no children, its visit counts sum to zero and the move's probabilities are the uniform fallback 1 / NUM_ACTIONS; a leaf of
// such a state is expanded to nothing and the search goes on from it.  The reference panics there and the oracle cannot run it: this
// struct is held to the host-stepped path alone.
// WideTieA6: six actions, all allowed.  Its test gives it three twists that leave the observation alone and rotate the actions within
// (0 1 2) and (3 4 5): the three actions of a cycle then average the SAME three head outputs in three different orders, so their
// priors differ by the rounding of that order alone and the first search of a move goes to whichever the order makes the largest.
#pragma once
#include "probe.hpp"

struct WideOpenA31 : Probe<4, 31, 1, false> {
    __host__ __device__ uint32_t masks() const { return 0x7fffffffu | (mix(this->h, 0x55u) & 0x80000000u); }
};

static_assert(sizeof(WideOpenA31) == sizeof(ProbeFixed<4, 31, 1>), "WideOpenA31: masks() adds no state");

struct WideShutA7 : Probe<4, 7, 1, false> {
    __host__ __device__ uint32_t masks() const
    {
        const uint32_t m = (mix(this->h, 0x56u) & 3u) == 0u ? 0u : ((mix(this->h, 0x53u) | mix(this->h, 0x54u)) & 0x7fu);
        return m | (mix(this->h, 0x55u) & ~0x7fu);
    }
};

struct WideTieA6 : Probe<4, 6, 1, false> {
    __host__ __device__ uint32_t masks() const { return 0x3fu | (mix(this->h, 0x55u) & ~0x3fu); }
};
