// wide.hpp -- the hash walk of probe.hpp with 5 .. 31 actions (TW_DEVICE_ENV_WIDE of include/twisterl_device_env.hpp), one alias per
// row of tests/device_env_wide.py.  probe.hpp's templates are used as they are -- state, reset(), step() (which mixes action + 1 into
// the hash: every index up to 30 changes the walk), observe() / observe_n(), reward(), is_final() -- except for masks(): probe.hpp
// draws its mask from 27 bits of h, which do not reach the bits 27 .. 30.  Here every bit comes from a full 32-bit mix of h:
// half of the states allow EXACTLY ONE action, uniform over 0 .. A - 1 (so every index is the only allowed one somewhere, bit 30
// included); the others allow each action with probability 1/4 (never none), and the bits A .. 31 are garbage, which the contract lets
// them be.
#pragma once
#include "probe.hpp"

template <class Base>
struct WideMasks : Base {
    __host__ __device__ uint32_t masks() const
    {
        constexpr uint32_t A = (uint32_t)Base::NUM_ACTIONS, AM = (1u << A) - 1u;
        const uint32_t sel = Base::mix(this->h, 0x51u);
        const uint32_t one = 1u << (Base::mix(this->h, 0x52u) % A);
        uint32_t m = (sel & 1u) ? one : (Base::mix(this->h, 0x53u) & Base::mix(this->h, 0x54u) & AM);
        if (m == 0u) m = one;
        return m | (Base::mix(this->h, 0x55u) & ~AM);
    }
};

template <int N_OBS, int NUM_ACTIONS, bool VAR>
using Wide = WideMasks<Probe<N_OBS, NUM_ACTIONS, 1, VAR>>;

using WideO2A5    = Wide<2, 5, false>;        // EngineV<4>: the first value past the edge; the second Gumbel draw uses one word
using WideO5A8V   = Wide<5, 8, true>;         // EngineV<9>, observe_n: two whole draws
using WideO16A16  = Wide<16, 16, false>;      // EngineV<16>: a full head tile
using WideO17A17  = Wide<17, 17, false>;      // EngineV<25>: the head's second tile holds one row
using WideO64A31  = Wide<64, 31, false>;      // EngineV<64>: the limit -- mask bit 30, draw index 7
using WideO4A3    = Wide<4, 3, false>;        // EngineV<4>: the opt-in without use (built with and without it)

static_assert(sizeof(WideO64A31) == sizeof(ProbeFixed<64, 31, 1>), "Wide: masks() adds no state");
