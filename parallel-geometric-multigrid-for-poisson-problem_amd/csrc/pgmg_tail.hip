// pgmg_tail.hip — the coarse end of the hierarchy in ONE workgroup, all in LDS.
//
// Below N ~ 129 every level is launch/latency-bound: a level of the multi-kernel
// path costs ~9 dependent launches (~1.5-2 us each) for a few microseconds of
// data.  The tail instead runs the complete gamma-cycle (gamma = 1: V, 3: W) for
// the tail's top level and everything below it inside one 1024-thread workgroup:
// the level pyramid (solution E, right-hand side F) plus one scratch grid T live
// in LDS (N_top = 65: 125 KiB of the CU's 160 KiB), separated by __syncthreads.
//
// Semantics are exactly MultigridSolver::v_cycle / w_cycle (MultiGrid.hpp:57-136)
// with JacobiSmoother::smooth (Smoother.hpp:38-116), including the per-sweep
// residual-norm early exit, evaluated sequentially (no speculation needed here).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "pgmg_internal.h"
#include "pgmg_tail_dev.h"

namespace pgmg {

// analytic right-hand side of tail level t from host sine tables (DynamicGridUtils.hpp:111-124)
template <class Real>
__device__ __forceinline__ void tail_rhs(const TailArgsDev<Real> &d, int t, Real *F)
{
    const int N = d.lv[t].N, n = N * N;
    const double *sx = d.a.fmg_tab + d.a.fmg_tab_off[t];
    const double *sy = sx + N;
    for (int k = threadIdx.x; k < n; k += kTailThreads) {
        const int j = k / N;
        const int i = k - j * N;
        F[k] = (Real)(d.a.fmg_factor * sx[i] * sy[j]);
    }
}

// values restriction (compute_coarsest_grid) fine level t -> t+1, coarse boundary 0
template <class Real>
__device__ __forceinline__ void tail_restrict_values(const Real *x, const TailLevel<Real> &Lf, Real *xc,
                                     const TailLevel<Real> &Lc)
{
    const int N = Lf.N, Nc = Lc.N, nc = Nc * Nc;
    for (int q = threadIdx.x; q < nc; q += kTailThreads) {
        const int jc = q / Nc;
        const int ic = q - jc * Nc;
        if (ic == 0 || jc == 0 || ic == Nc - 1 || jc == Nc - 1) {
            xc[q] = Real(0);
            continue;
        }
        const int k = (2 * jc) * N + 2 * ic;
        xc[q] = Real(0.25) * x[k] + Real(0.125) * (x[k + 1] + x[k - 1] + x[k + N] + x[k - N]) +
                Real(0.0625) * (x[k - N - 1] + x[k - N + 1] + x[k + N - 1] + x[k + N + 1]);
    }
    __syncthreads();
}

template <class Real>
__global__ __launch_bounds__(kTailThreads) void k_tail(TailArgsDev<Real> d)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned long long k0 = d.prof ? tail_clock() : 0;
    const TailArgsT<Real> &a = d.a;
    const int S = d.S;
    double *red = lds;                                   // kTailThreads / 64 + 1 partial sums
    Real *E = reinterpret_cast<Real *>(lds + kTailRed);
    Real *F = E + S;
    Real *T = E + 2 * S;

    for (int k = threadIdx.x; k < 2 * S; k += kTailThreads) E[k] = Real(0);
    __syncthreads();
    {
        // the top level from global memory: every load of a thread issued before the first
        // LDS store (a load-store loop waited one global-memory latency per point)
        const int N = d.lv[0].N, n = N * N;
        const long long P = a.P_top;
        const bool ldf = !a.fmg, lde = a.x0_from_global || a.fmg;
        constexpr int KU = (65 * 65 + kTailThreads - 1) / kTailThreads;   // N_top <= 65
        Real fv[KU], ev[KU];
        #pragma unroll
        for (int q = 0; q < KU; ++q) {
            // (clamped: a point past the grid re-reads the last one, never past the array)
            const int k = min((int)threadIdx.x + q * kTailThreads, n - 1);
            const int j = tail_row(k, d.lv[0].rN), i = k - j * N;
            fv[q] = ldf ? a.f_top[j * P + i] : Real(0);
            ev[q] = lde ? a.e_top[j * P + i] : Real(0);
        }
        #pragma unroll
        for (int q = 0; q < KU; ++q) {
            const int k = threadIdx.x + q * kTailThreads;
            if (k < n) {
                if (ldf) F[k] = fv[q];
                if (lde) E[k] = ev[q];
            }
        }
        for (int k = threadIdx.x + KU * kTailThreads; k < n; k += kTailThreads) {
            const int j = k / N;
            const int i = k - j * N;
            if (ldf) F[k] = a.f_top[j * P + i];
            if (lde) E[k] = a.e_top[j * P + i];
        }
    }
    __syncthreads();

    Cnt cnt;   // sweeps and exits of this launch (< 2^31)
    int par = 0;
    const int last = d.nl - 1;
    if (!a.fmg) {
        for (int v = 0; v < max(1, a.visits); ++v)
            cnt += tail_gcycle<BlockTeam>(d, 0, 1, E, F, T, red, par);
    } else {
        // compute_coarsest_grid: restrict phi down to the coarsest level
        for (int t = 0; t < last; ++t)
            tail_restrict_values(E + d.lv[t].off, d.lv[t], E + d.lv[t + 1].off, d.lv[t + 1]);
        for (int t = last; t >= 0; --t) {
            Real *Et = E + d.lv[t].off;
            Real *Ft = F + d.lv[t].off;
            tail_rhs(d, t, Ft);                      // f_fine = compute_rhs (MultiGrid.hpp:162)
            if (t < last) {
                const int n = d.lv[t].N * d.lv[t].N;
                for (int k = threadIdx.x; k < n; k += kTailThreads) Et[k] = Real(0);
                __syncthreads();
                tail_prolong<BlockTeam>(Et, d.lv[t], E + d.lv[t + 1].off, d.lv[t + 1]);   // :164
                cnt += tail_gcycle<BlockTeam>(d, t, 1, E, F, T, red, par);  // :167 v_cycle
            } else {
                __syncthreads();
            }
            if (t > 0 || a.fmg_smooth_top)                                   // :153 smooth(3)
                cnt += tail_smooth<BlockTeam>(Et, Ft, d.lv[t], 3, d.eps2, T, red, par);
        }
    }

    {
        const int N = d.lv[0].N, n = N * N;
        const long long P = a.P_top;
        for (int k = threadIdx.x; k < n; k += kTailThreads) {
            const int j = k / N;
            const int i = k - j * N;
            a.e_top[j * P + i] = E[k];
        }
    }
    if (threadIdx.x == 0 && a.stats != nullptr) {
        atomicAdd(&a.stats[0], (unsigned long long)cnt.sweeps);
        atomicAdd(&a.stats[1], (unsigned long long)cnt.exits);
    }
    if (d.prof && threadIdx.x == 0) {
        d.prof[4] += tail_clock() - k0;
        d.prof[5] += 1;
    }
}

template <class Real>
size_t tail_lds_bytes(int N_top, int n_coarse)
{
    size_t S = 0;
    int N = N_top;
    for (int l = 0; l < kTailMaxLevels; ++l) {
        S += (size_t)N * N;
        if (N <= n_coarse) break;
        N = (N - 1) / 2 + 1;
    }
    // scratch T: one grid of the top level, and at least tail_smooth_rows' edge-row buffers
    const size_t t = std::max((size_t)N_top * N_top, (size_t)kTailRows * 4 * kTailWaves * 64);
    return kTailRed * sizeof(double) + (2 * S + t) * sizeof(Real);
}

// PGMG_TAIL_PROF=1 (measurement build libpgmg_ab.so only): the per-stage cycle counters
// of k_tail
static unsigned long long *tail_prof_buffer()
{
    static unsigned long long *buf = [] {
        unsigned long long *p = nullptr;
        if (tuning_int("PGMG_TAIL_PROF", 0) == 1 &&
            hipMalloc(&p, 16 * sizeof(unsigned long long)) == hipSuccess)
            (void)hipMemset(p, 0, 16 * sizeof(unsigned long long));
        return p;
    }();
    return buf;
}

template <class Real>
hipError_t launch_tail_gamma(const TailArgsT<Real> &a, int gamma, hipStream_t s)
{
    static bool attr_set = false;
    TailArgsDev<Real> d;
    d.a = a;
    d.gamma = gamma;
    d.eps2 = norm2_threshold(a.eps);
    int N = a.N_top;
    double h = a.h_top;
    int off = 0, nl = 0;
    for (; nl < kTailMaxLevels; ++nl) {
        d.lv[nl].N = N;
        d.lv[nl].off = off;
        d.lv[nl].hh = (Real)(h * h);
        d.lv[nl].ih = (Real)(1.0 / (h * h));
        d.lv[nl].rN = 1.0f / (float)N;
        off += N * N;
        if (N <= a.n_coarse) {
            ++nl;
            break;
        }
        N = (N - 1) / 2 + 1;
        h = 2 * h;  // MultiGrid.hpp:83 v_cycle(e_coarse, res_coarse, Nc, 2 * h)
    }
    d.nl = nl;
    d.S = off;
    {
        static const int wave_n = tuning_int("PGMG_TAIL_WAVE_N", 9);
        d.wave_n = wave_n;
    }
    d.prof = tail_prof_buffer();
    const size_t bytes = tail_lds_bytes<Real>(a.N_top, a.n_coarse);
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)k_tail<Real>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    k_tail<Real><<<dim3(1), dim3(kTailThreads), bytes, s>>>(d);
    return hipGetLastError();
}

template hipError_t launch_tail_gamma<double>(const TailArgsT<double> &, int, hipStream_t);

}  // namespace pgmg

// Read (and optionally reset) the k_tail cycle counters; -1 when PGMG_TAIL_PROF is unset.
extern "C" int pgmg_tail_prof(unsigned long long *out16, int reset)
{
    unsigned long long *b = pgmg::tail_prof_buffer();
    if (!b || !out16) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpy(out16, b, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -2;
    if (reset) (void)hipMemset(b, 0, 16 * sizeof(unsigned long long));
    return 0;
}

namespace pgmg {
template hipError_t launch_tail_gamma<float>(const TailArgsT<float> &, int, hipStream_t);
template size_t tail_lds_bytes<double>(int, int);
template size_t tail_lds_bytes<float>(int, int);

}  // namespace pgmg
