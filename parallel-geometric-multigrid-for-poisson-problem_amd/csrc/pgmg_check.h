// pgmg_check.h — the sums and the decision of an early-exit check, one copy.
//
// A smoother's early exit is sqrt(sum r^2) < eps (Smoother.hpp:75-88).  A pass leaves the sum
// as per-workgroup partials; whoever decides the check -- the in-stream rare paths, the scalar
// fix-ups, the decision kernels, the validation of a speculative call -- re-reduces those
// partials, and all of them must reach the same decision bit for bit.  They do because all of
// them take the sum from here, in ONE fixed order:
//   thread t adds p[t], p[t + nt], p[t + 2 nt], ... from 0.0 (nt = the workgroup's threads:
//   256 at every decision site);
//   wave_sum (pgmg_real.h) over each wave;
//   thread 0 adds the waves' sums in wave order from 0.0.
// Included by every kernel file that sums or decides a check.  (Not the monitor's norms,
// pgmg_monitor.hip: three sums behind one barrier, added by threads 0..2 -- no check's
// decision depends on them.)
//
// WAVES: the workgroup's waves at compile time (the unrolled form of the kernels launched
// with a fixed size); 0: taken from blockDim.x (the fused passes launch 1 to 4 waves).  Both
// forms give the same sum; the parameter only keeps each kernel's instructions.
#pragma once
#include "pgmg_real.h"

namespace pgmg {

// deterministic sum of one double per thread over the workgroup (fixed tree); the result is
// valid in thread 0.  red: WAVES (blockDim.x / 64) doubles of LDS; a second sum through the
// same red needs a barrier first.
template <int WAVES = 0>
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        if constexpr (WAVES > 0) {
            #pragma unroll
            for (int i = 0; i < WAVES; ++i) s += red[i];
        } else {
            for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
        }
    }
    return s;
}

// sum of p[0 .. n) over the workgroup, strided by its thread count; valid in thread 0
template <int WAVES = 0, class I>
__device__ __forceinline__ double partials_sum(const double *p, I n, double *red)
{
    const I nt = WAVES > 0 ? (I)(64 * WAVES) : (I)blockDim.x;
    double s = 0.0;
    for (I k = threadIdx.x; k < n; k += nt) s += p[k];
    return block_sum<WAVES>(s, red);
}

// the comparison itself (thread 0's value of a sum above, or an all-rank sum)
__device__ __forceinline__ bool check_fires(double sum, double eps) { return sqrt(sum) < eps; }

// Decision of an in-stream check from the partial sums of the pass just run: every workgroup
// re-reduces them (a row strip's all-rank sum comes in global_sum instead) and returns the
// same decision to all its threads; workgroup (0,0) books a fired check in stats (one sweep
// less, one exit more).
template <int WAVES = 0>
__device__ __forceinline__ bool check_decide(const double *partials, int np, double eps,
                                             const double *global_sum,
                                             unsigned long long *stats, double *red, int *trig)
{
    const double s = partials_sum<WAVES>(partials, np, red);
    if (threadIdx.x == 0) *trig = check_fires(global_sum != nullptr ? *global_sum : s, eps) ? 1 : 0;
    __syncthreads();
    const bool t = *trig != 0;
    if (t && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && stats != nullptr) {
        atomicAdd(&stats[0], (unsigned long long)-1LL);
        atomicAdd(&stats[1], 1ull);
    }
    return t;
}

}  // namespace pgmg
