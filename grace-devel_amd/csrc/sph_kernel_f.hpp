// The built-in SPH kernels' f(q) in fp32, shared by the walks that evaluate W(r, H) = H^-3 f(r / H) at
// points (interpolate.hip: scatter sums, range.hip: gather sums).  Each including translation unit
// gets its own copies (internal linkage).
#pragma once

#include "common.hpp"

#include <cmath>
#include <type_traits>

namespace {

__device__ __forceinline__ float pow4(const float t)
{
    const float t2 = t * t;
    return t2 * t2;
}

// K = f(q) in the fp32 operation sequence of include/grace_hip.h ("SPH interpolation at points");
// u = max(1 - q, 0), normalisation constant last.  (-ffp-contract=off: no operation is fused.)
template <int KIND>
__device__ __forceinline__ float kernel_f(const float q)
{
    const float u = fmaxf(1.0f - q, 0.0f);
    if constexpr (KIND == GRACE_SPH_KERNEL_CUBIC) {
        const float inner = ((6.0f * q - 6.0f) * (q * q)) + 1.0f;
        const float outer = 2.0f * ((u * u) * u);
        return (q < 0.5f ? inner : outer) * float(8.0 / M_PI);
    } else if constexpr (KIND == GRACE_SPH_KERNEL_QUARTIC) {
        const float t2 = fmaxf(u - 0.4f, 0.0f), t3 = fmaxf(u - 0.8f, 0.0f);
        return ((pow4(u) - 5.0f * pow4(t2)) + 10.0f * pow4(t3)) * float(25.0 * 39.0625 / (32.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_QUINTIC) {
        const float t2 = fmaxf(u - float(1.0 / 3.0), 0.0f), t3 = fmaxf(u - float(2.0 / 3.0), 0.0f);
        return ((pow4(u) * u - 6.0f * (pow4(t2) * t2)) + 15.0f * (pow4(t3) * t3))
            * float(9.0 * 243.0 / (40.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_WENDLAND_C2) {
        return (pow4(u) * (4.0f * q + 1.0f)) * float(21.0 / (2.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_WENDLAND_C4) {
        const float u6 = pow4(u) * (u * u);
        return (u6 * (q * (q * float(35.0 / 3.0) + 6.0f) + 1.0f)) * float(495.0 / (32.0 * M_PI));
    } else {
        static_assert(KIND == GRACE_SPH_KERNEL_WENDLAND_C6, "built-in SPH kernels only");
        const float u4 = pow4(u);
        return ((u4 * u4) * (q * (q * (32.0f * q + 25.0f) + 8.0f) + 1.0f)) * float(1365.0 / (64.0 * M_PI));
    }
}

__device__ __forceinline__ float pow3(const float t)
{
    return (t * t) * t;
}

// E = f'(q) in the fp32 operation sequence of include/grace_hip.h ("SPH gradients at points"); u, t2,
// t3 and the normalisation constants are kernel_f's.
template <int KIND>
__device__ __forceinline__ float kernel_df(const float q)
{
    const float u = fmaxf(1.0f - q, 0.0f);
    if constexpr (KIND == GRACE_SPH_KERNEL_CUBIC) {
        const float inner = (18.0f * q - 12.0f) * q;
        const float outer = -6.0f * (u * u);
        return (q < 0.5f ? inner : outer) * float(8.0 / M_PI);
    } else if constexpr (KIND == GRACE_SPH_KERNEL_QUARTIC) {
        const float t2 = fmaxf(u - 0.4f, 0.0f), t3 = fmaxf(u - 0.8f, 0.0f);
        return ((20.0f * pow3(t2) - 4.0f * pow3(u)) - 40.0f * pow3(t3)) * float(25.0 * 39.0625 / (32.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_QUINTIC) {
        const float t2 = fmaxf(u - float(1.0 / 3.0), 0.0f), t3 = fmaxf(u - float(2.0 / 3.0), 0.0f);
        return ((30.0f * pow4(t2) - 5.0f * pow4(u)) - 75.0f * pow4(t3)) * float(9.0 * 243.0 / (40.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_WENDLAND_C2) {
        return ((-20.0f * q) * pow3(u)) * float(21.0 / (2.0 * M_PI));
    } else if constexpr (KIND == GRACE_SPH_KERNEL_WENDLAND_C4) {
        return (((float(-56.0 / 3.0) * q) * (5.0f * q + 1.0f)) * (pow4(u) * u)) * float(495.0 / (32.0 * M_PI));
    } else {
        static_assert(KIND == GRACE_SPH_KERNEL_WENDLAND_C6, "built-in SPH kernels only");
        return (((-22.0f * q) * (q * (16.0f * q + 7.0f) + 1.0f)) * ((pow4(u) * (u * u)) * u))
            * float(1365.0 / (64.0 * M_PI));
    }
}

// The run-time choice of a built-in kernel and 1..4 channels as compile-time constants:
// f(kind, nw) gets two std::integral_constant<int, ...> (a generic lambda reads their ::value).
// Steps through the kinds CUBIC .. WENDLAND_C6 (consecutive values), then through the channel
// counts, to the first that matches; a value that matches none gets the last, as a switch's default.
template <int KIND = GRACE_SPH_KERNEL_CUBIC, int NW = 1, typename F>
void with_kernel(const int kind, const int nw, F f)
{
    static_assert(GRACE_SPH_KERNEL_CUBIC == 0 && GRACE_SPH_KERNEL_WENDLAND_C6 == 5, "six consecutive kinds");
    if constexpr (KIND < GRACE_SPH_KERNEL_WENDLAND_C6) {
        if (kind != KIND) return with_kernel<KIND + 1, NW>(kind, nw, f);
    }
    if constexpr (NW < 4) {
        if (nw != NW) return with_kernel<KIND, NW + 1>(kind, nw, f);
    }
    f(std::integral_constant<int, KIND>(), std::integral_constant<int, NW>());
}

} // namespace
