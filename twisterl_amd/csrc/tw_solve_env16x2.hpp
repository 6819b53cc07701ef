// tw_solve_env16x2.hpp -- solve_env16x2_kernel: the device-environment evaluate / solve over EngineV16x2 (tw_engine_generic16x2.hpp),
// precision="fp16x2" of collector.evaluate and collector.solve without MCTS, with its launcher and its occupancy query.  Included by
// the END of tw_rollout_env.hpp (which declares the two host templates ahead of their uses) and by nothing else.  A module
// instantiates what is here only when it was built with TW_DEVICE_ENV_FP16X2_SOLVE (build_device_env(..., fp16x2_solve=True)); the
// library instantiates none of it.
#pragma once
#include "tw_rollout_env.hpp"

namespace tw {

// The evaluate loop over EngineV16x2: the third kernel that includes tw_env_solve_loop.hpp.  pack_generic16x2_kernel runs in front of
// it, on the same stream, into EnvSolveArgs::image.  The engine raises GEN16X2_ERR_RANGE in a.err for an activation outside the split
// terms' range (eng.end()), the pack kernel for a weight; the library then runs the call again in f32.
// tests/test_gpu_device_env_fp16x2_solve.py holds it, attempt by attempt, to the oracle's ARITH_CHAIN loop over the module's host code.
template <class Env, int NC>
__global__ void __launch_bounds__(256, 1) solve_env16x2_kernel(const EnvSolveArgs a, const Env proto)
{
    using Eng = EngineV16x2<NC>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Eng eng;
    eng.img = a.image.img;
    eng.err = a.err;
#include "tw_env_solve_loop.hpp"
}

// precision="fp16x2": what launch_solve_env does with arguments whose image carries GEN16X2_REQUEST, in a module built with
// TW_DEVICE_ENV_FP16X2_SOLVE -- refuses a missing image or err word, another image size than the layout functions give for the widths
// the library read, and a policy EngineV16x2 does not take (hipErrorInvalidValue, before any HIP call), packs the two planes of every
// layer on stream s (one thread per weight, at most 1,024 workgroups) and launches solve_env16x2_kernel.
// lds_bytes = EngineV16x2<engine_nc>::lds_bytes(pol).
template <class Env>
int launch_solve_env16x2(const EnvSolveArgs *a, const Env &p, unsigned blocks, size_t lds_bytes, hipStream_t s)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    EnvSolveArgs x = *a;
    x.image.halves = a->image.halves & ~GEN16X2_REQUEST;
    const PolicyDev &pol = x.pol;
    const int n_layers = pol.n_common + pol.n_action + pol.n_value;
    if (!x.image.img || !x.err || !pol.generic || n_layers > GEN16_MAX_LAYERS || x.image.halves < (uint64_t)GEN16_PF * 512u)
        return (int)hipErrorInvalidValue;
    auto *k = &solve_env16x2_kernel<Env, NC>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return (int)e;
    uint64_t pb = (x.image.halves / 2 + 255) / 256;
    if (pb > 1024) pb = 1024;
    hipLaunchKernelGGL((pack_generic16x2_kernel<256>), dim3((unsigned)(pb ? pb : 1)), dim3(256), 0, s, pol, x.image, x.err);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((solve_env16x2_kernel<Env, NC>), dim3(blocks), dim3(EngineV16x2<NC>::THREADS), lds_bytes, s, x, p);
    return (int)hipGetLastError();
}

// tw_device_env::groups_per_cu, kernel 6: solve_env16x2_kernel of a module built with TW_DEVICE_ENV_FP16X2_SOLVE.  With out == nullptr
// the question is only whether the module HOLDS the kernel (the library's dispatch, DeviceEnv.fp16x2_solve): answered without the HIP
// runtime
template <class Env>
int groups_per_cu_solve_env16x2(size_t lds_bytes, int *out)
{
    constexpr int NC = env_engine_nc(Env::N_OBS);
    if (!out) return (int)hipSuccess;
    return kernel_groups_per_cu(reinterpret_cast<const void *>(&solve_env16x2_kernel<Env, NC>), EngineV16x2<NC>::THREADS, lds_bytes, out);
}

}  // namespace tw
