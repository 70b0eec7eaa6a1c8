// pgmg_grad_dev.h — what the passes that difference a grid along its lines share (k_gradient,
// pgmg_gradient.hip; k_divergence and k_grad_update, pgmg_project.hip): the rows of loads they
// keep in flight and the one-sided line formulas of include/pgmg.h "Gradient of the solution".
// Device only.
#pragma once
#include <hip/hip_runtime.h>

namespace pgmg {

constexpr int kGradU = 4;   // rows of loads in flight per wave

// The one-sided differences along a line, their points in ascending order, before the factor w:
// order 2 at the first and the last point of three ...
template <class T> __device__ __forceinline__ T os2_first(T v0, T v1, T v2)
{
    return T(4) * v1 - T(3) * v0 - v2;
}
template <class T> __device__ __forceinline__ T os2_last(T u0, T u1, T u2)
{
    return T(3) * u2 - T(4) * u1 + u0;
}
// ... order 4 at the first, second, last but one and last point of five
template <class T> __device__ __forceinline__ T os4_first(T v0, T v1, T v2, T v3, T v4)
{
    return T(48) * v1 - T(25) * v0 - T(36) * v2 + T(16) * v3 - T(3) * v4;
}
template <class T> __device__ __forceinline__ T os4_second(T v0, T v1, T v2, T v3, T v4)
{
    return T(18) * v2 - T(10) * v1 - T(3) * v0 - T(6) * v3 + v4;
}
template <class T> __device__ __forceinline__ T os4_penult(T u0, T u1, T u2, T u3, T u4)
{
    return T(10) * u3 - T(18) * u2 + T(3) * u4 + T(6) * u1 - u0;
}
template <class T> __device__ __forceinline__ T os4_last(T u0, T u1, T u2, T u3, T u4)
{
    return T(25) * u4 - T(48) * u3 + T(36) * u2 - T(16) * u1 + T(3) * u0;
}

}  // namespace pgmg
