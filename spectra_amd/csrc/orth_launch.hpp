// Host-side helpers of the orthogonalisation launchers (krylov.hip, orth_dma.hip, orth_dma_modes.hip, orth_wide.hip): the map from
// a run-time slot count to a template instantiation, and the launch of a kernel that needs more dynamic LDS than the default
// limit.  Internal.
#pragma once
#include "common.hpp"

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace {

// Calls f(std::integral_constant<int, S>{}) for S = s when LO <= s <= HI and returns true; returns false otherwise.  Every S in
// [LO, HI] is instantiated, whether a caller can reach it or not.
template <int LO, int... I, class F>
bool dispatch_slots_seq(int s, std::integer_sequence<int, I...>, F&& f)
{
    return ((s == LO + I ? (f(std::integral_constant<int, LO + I>{}), true) : false) || ...);
}
template <int LO, int HI, class F>
bool dispatch_slots(int s, F&& f)
{
    return dispatch_slots_seq<LO>(s, std::make_integer_sequence<int, HI - LO + 1>{}, f);
}

// Launches Kernel with `lds` bytes of dynamic LDS.  The attribute that allows more than 64 KiB is per device and function: set once
// per device and kernel (one context per device and process in practice, and setting it again is harmless).
template <auto Kernel, typename... Args>
void launch_with_dynamic_lds(const mispec_ctx& ctx, dim3 grid, dim3 block, size_t lds, const Args&... args)
{
    static thread_local int attr_dev = -1;
    if (attr_dev != ctx.device)
    {
        MISPEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        attr_dev = ctx.device;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, ctx.stream, args...);
}

}  // namespace
