// pgmg_fixup.hip — what follows a fused pass whose early-exit check is decided in a launch of
// its own: the scalar fix-ups of k_pre / k_post, and the decision kernels of k_postpre_lds
// and of its smooth(3) form with the latter's rare path.
//
// The fused passes (pgmg_pre.hip, pgmg_post.hip, pgmg_postpre_impl.h) run both sweeps and leave
// the checks' sums r(x_k)^2 as per-workgroup partials.  The kernels here re-reduce them
// (pgmg_check.h: one order everywhere), decide, book the exit, and when a check fired (rare)
// recompute the reference result point by point from the inputs the pass left untouched.
#include <algorithm>

#include "pgmg.h"
#include "pgmg_check.h"
#include "pgmg_fused.h"

namespace pgmg {

// ---------------------------------------------------------------------------
// Fix-ups (rare path): the early-exit check after the first sweep fired.
// Scalar grid-stride code recomputing the reference result from the inputs
// the fused pass left untouched.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool fix_decide(const FixArgsF &a, double *red, int *trig)
{
    if (a.cond != nullptr && *a.cond == 0u) return false;  // uniform
    if (a.force) return true;  // recompute requested by k_postpre_decide (stats done there)
    return check_decide(a.partials, a.np, a.eps, a.global_sum, a.stats, red, trig);
}

template <class T>
struct FixCtx {
    const T *x0, *f;
    const T *ec;
    int N, Nc;
    long long P, Pc;
    T hh, ih;
    bool x0_zero;
    const unsigned *pre_fired;  // non-null: phi (x0 of fxeff) is recomputed from f
    bool pin;                   // x0 = (+0) + P ec (k_pre PIN, F-cycle)
    long long Px;               // x0's pitch (0: P; the caller's array: N)
};

template <class T>
__device__ T fxpin(const FixCtx<T> &c, int j, int i);

template <class T>
__device__ __forceinline__ T fx0(const FixCtx<T> &c, int j, int i)
{
    if (c.pin) return fxpin(c, j, i);
    return c.x0_zero ? T(0) : c.x0[(long long)j * (c.Px != 0 ? c.Px : c.P) + i];
}

template <bool POST, class T>
__device__ T fx1(const FixCtx<T> &c, int j, int i);

// pre-smoothed iterate of x0 = 0 (k_post RECOMP): x1 = J(0), phi = fired ? x1 : J(x1)
template <class T>
__device__ T fphi0(const FixCtx<T> &c, int j, int i)
{
    FixCtx<T> z = c;
    z.x0_zero = true;
    z.pre_fired = nullptr;
    if (*c.pre_fired != 0u || j <= 0 || i <= 0 || j >= c.N - 1 || i >= c.N - 1)
        return fx1<false>(z, j, i);
    return T(0.25) * ((c.hh * c.f[(long long)j * c.P + i]) + fx1<false>(z, j, i - 1) +
                   fx1<false>(z, j, i + 1) + fx1<false>(z, j - 1, i) + fx1<false>(z, j + 1, i));
}

// x_eff = phi + P ec at one fine point (MultiGrid.hpp:208-226)
template <class T>
__device__ T fxeff(const FixCtx<T> &c, int j, int i)
{
    T v = c.pre_fired != nullptr ? fphi0(c, j, i) : c.x0[(long long)j * c.P + i];
    if (j < 2 || i < 2 || j > c.N - 2 || i > c.N - 2) return v;
    const int jc = j >> 1, ic = i >> 1;
    const T *C0 = c.ec + (long long)jc * c.Pc;
    T w;
    if ((j & 1) == 0) {
        w = ((i & 1) == 0) ? C0[ic] : T(0.5) * (C0[ic] + C0[ic + 1]);
    } else {
        const T *C1 = C0 + c.Pc;
        w = ((i & 1) == 0) ? T(0.5) * (C0[ic] + C1[ic]) : T(0.25) * (C0[ic] + C0[ic + 1] + C1[ic] + C1[ic + 1]);
    }
    return v + w;
}

// x0 of a PIN pre-smooth: the prolongation of ec into a zeroed grid (frame 0)
template <class T>
__device__ T fxpin(const FixCtx<T> &c, int j, int i)
{
    const T v = T(0);
    if (j < 2 || i < 2 || j > c.N - 2 || i > c.N - 2) return v;
    const int jc = j >> 1, ic = i >> 1;
    const T *C0 = c.ec + (long long)jc * c.Pc;
    T w;
    if ((j & 1) == 0) {
        if ((i & 1) == 0) return v + C0[ic];
        w = T(0.5) * (C0[ic] + C0[ic + 1]);
    } else {
        const T *C1 = C0 + c.Pc;
        w = ((i & 1) == 0) ? T(0.5) * (C0[ic] + C1[ic]) : T(0.25) * (C0[ic] + C0[ic + 1] + C1[ic] + C1[ic + 1]);
    }
    return v + w;
}

template <bool POST, class T>
__device__ T fin(const FixCtx<T> &c, int j, int i)
{
    return POST ? fxeff(c, j, i) : fx0(c, j, i);
}

template <bool POST, class T>
__device__ T fx1(const FixCtx<T> &c, int j, int i)
{
    if (j <= 0 || i <= 0 || j >= c.N - 1 || i >= c.N - 1) return fin<POST>(c, j, i);
    return T(0.25) * ((c.hh * c.f[(long long)j * c.P + i]) + fin<POST>(c, j, i - 1) +
                   fin<POST>(c, j, i + 1) + fin<POST>(c, j - 1, i) + fin<POST>(c, j + 1, i));
}

// two post-smooth sweeps from x_eff (row-strip rare path: x2 on rows past the strip)
template <class T>
__device__ T fx2post(const FixCtx<T> &c, int j, int i)
{
    if (j <= 0 || i <= 0 || j >= c.N - 1 || i >= c.N - 1) return fxeff(c, j, i);
    return T(0.25) * ((c.hh * c.f[(long long)j * c.P + i]) + fx1<true>(c, j, i - 1) +
                      fx1<true>(c, j, i + 1) + fx1<true>(c, j - 1, i) + fx1<true>(c, j + 1, i));
}

template <class T>
__device__ T fr1(const FixCtx<T> &c, int j, int i)
{
    return c.f[(long long)j * c.P + i] -
           c.ih * (T(4) * fx1<false>(c, j, i) - fx1<false>(c, j, i - 1) - fx1<false>(c, j, i + 1) -
                   fx1<false>(c, j - 1, i) - fx1<false>(c, j + 1, i));
}

template <class T>
__global__ __launch_bounds__(256) void k_pre_fixup(FixArgsF a, PreArgsT<T> p, int x0_zero)
{
    __shared__ double red[4];
    __shared__ int trig;
    const bool t = fix_decide(a, red, &trig);
    if (p.fired != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *p.fired = t ? 1u : 0u;
    if (!t) return;
    FixCtx<T> c{p.x0, p.f, p.pin_ec, p.N, p.Nc, p.P, p.Pc, p.hh, p.ih, x0_zero != 0, nullptr,
                p.pin_ec != nullptr, p.Px};
    const long long W = p.N - 2;
    const long long nrows = p.x2 != nullptr ? (long long)(p.row_hi - p.row_lo) : 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nrows * W; k += stride) {
        const int j = p.row_lo + (int)(k / W), i = 1 + (int)(k % W);
        p.x2[(long long)j * p.P + i] = fx1<false>(c, j, i);
    }
    const int clo = max(1, p.rc_lo), chi = min(p.Nc - 1, p.rc_hi);
    const long long Wc = p.Nc - 2;
    const long long ncr = chi > clo ? (long long)(chi - clo) : 0;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < ncr * Wc; k += stride) {
        const int jc = clo + (int)(k / Wc), ic = 1 + (int)(k % Wc);
        const int j = 2 * jc, i = 2 * ic;
        p.rc[(long long)jc * p.Pc + ic] =
            T(0.25) * fr1(c, j, i) + T(0.125) * (fr1(c, j, i + 1) + fr1(c, j, i - 1) + fr1(c, j + 1, i) + fr1(c, j - 1, i)) +
            T(0.0625) * (fr1(c, j - 1, i - 1) + fr1(c, j - 1, i + 1) + fr1(c, j + 1, i - 1) + fr1(c, j + 1, i + 1));
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_post_fixup(FixArgsF a, PostArgsT<T> p)
{
    __shared__ double red[4];
    __shared__ int trig;
    if (!fix_decide(a, red, &trig)) return;
    FixCtx<T> c{p.phi, p.f, p.ec, p.N, p.Nc, p.P, p.Pc, p.hh, p.ih, false, p.pre_fired};
    const long long W = p.N - 2;
    const long long nrows = (long long)(p.row_hi - p.row_lo);
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long Po = p.Po != 0 ? p.Po : p.P;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nrows * W; k += stride) {
        const int j = p.row_lo + (int)(k / W), i = 1 + (int)(k % W);
        p.x2[(long long)j * Po + i] = p.fix_sweeps == 2 ? fx2post(c, j, i) : fx1<true>(c, j, i);
    }
}

// Fix-up grid: every block re-reduces the partials (the decision) and the grid-stride
// recompute only runs when a check fired, so small levels get few blocks (a 256-block
// launch costs ~2 us more than a 1-block one on a latency-bound level); 256 blocks from
// 2^20 points up (a fired recompute on the finest levels then still has the whole chip).
static int fixup_blocks(int N, int row_lo, int row_hi)
{
    // the rare-path recompute is scalar pointwise recursion (tens of loads per point): one
    // thread per point, up to 8192 blocks (was one per 16, at most 256 blocks: a fired
    // coarse-level fix-up cost ~40 us; 200 V-cycles at N = 4097, where the levels above
    // the tail converge and fire every cycle: 1083 -> 2435 V-cycles/s; 100 at 16385:
    // 439 -> 523; scripts/long_run.sh)
    const long long pts = (long long)(row_hi > row_lo ? row_hi - row_lo : 0) * N;
    const long long shift = 8, cap = 8192;
    long long b = pts >> shift;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <class T>
void launch_pre_fixup(const FixArgsF &a, const PreArgsT<T> &p, bool x0_zero, hipStream_t s)
{
    k_pre_fixup<T><<<dim3(fixup_blocks(p.N, p.row_lo, p.row_hi)), dim3(256), 0, s>>>(
        a, p, x0_zero ? 1 : 0);
}

template <class T>
void launch_post_fixup(const FixArgsF &a, const PostArgsT<T> &p, hipStream_t s)
{
    k_post_fixup<T><<<dim3(fixup_blocks(p.N, p.row_lo, p.row_hi)), dim3(256), 0, s>>>(a, p);
}

// one block: both decisions, stats, flags for the conditional rare-path kernels
// global != nullptr (row strips): the all-rank sums {post, pre} instead of the partials
__global__ __launch_bounds__(256) void k_postpre_decide(const double *p1, const double *p2, int np,
                                                        const double *global, double eps,
                                                        unsigned *flags,
                                                        unsigned long long *stats)
{
    __shared__ double red[4];
    double s1 = partials_sum(p1, np, red);
    __syncthreads();
    double s2 = partials_sum(p2, np, red);
    if (threadIdx.x == 0 && global != nullptr) {
        s1 = global[0];
        s2 = global[1];
    }
    if (threadIdx.x == 0) {
        const unsigned t1 = sqrt(s1) < eps ? 1u : 0u;
        const unsigned t2 = (!t1 && sqrt(s2) < eps) ? 1u : 0u;
        flags[0] = t1;
        flags[1] = t2;
        if (stats != nullptr) {
            // t1: the post-smooth stopped after 1 sweep and the pre-smooth is redone from
            //     x1 by the conditional k_pre (which counts its own sweeps): -1 - 2
            // t2: the pre-smooth stopped after 1 sweep: -1
            if (t1) {
                atomicAdd(&stats[0], (unsigned long long)-3LL);
                atomicAdd(&stats[1], 1ull);
                atomicAdd(&stats[2], 1ull);
            }
            if (t2) {
                atomicAdd(&stats[0], (unsigned long long)-1LL);
                atomicAdd(&stats[1], 1ull);
                atomicAdd(&stats[3], 1ull);
            }
        }
    }
}

void launch_postpre_decide(const double *partials1, const double *partials2, unsigned long long *stats,
                           int np, const double *global, double eps, unsigned *flags, hipStream_t s)
{
    k_postpre_decide<<<dim3(1), dim3(256), 0, s>>>(partials1, partials2, np, global, eps, flags,
                                                  stats);
}

// ---------------------------------------------------------------------------
// After the fused smooth(3) (launch_smooth4, pgmg_postpre_impl.h: four sweeps x0 -> x4 with the
// checks ||r(x1)||, ||r(x2)||, ||r(x3)|| < eps summed speculatively): the decision kernel
// finds the first check that fires and the rare-path kernel recomputes x_k from the
// untouched x0.
// ---------------------------------------------------------------------------
// flags[0] = first k in 1..3 whose check ||r(x_k)|| < eps fires, 0 if none; stats
// [sweeps, exits].  global3 (row strips): all-rank sums {r(x1), r(x3), r(x2)}.
__global__ __launch_bounds__(256) void k_smooth4_decide(const double *p1, const double *p2,
                                                        const double *p3, int np,
                                                        const double *global3, double eps,
                                                        unsigned *flags,
                                                        unsigned long long *stats)
{
    __shared__ double red[4];
    double s1 = partials_sum(p1, np, red);
    __syncthreads();
    double s3 = partials_sum(p3, np, red);
    __syncthreads();
    double s2 = partials_sum(p2, np, red);
    if (threadIdx.x == 0) {
        if (global3 != nullptr) {
            s1 = global3[0];
            s2 = global3[1];
            s3 = global3[2];
        }
        const int k = sqrt(s1) < eps ? 1 : (sqrt(s3) < eps ? 2 : (sqrt(s2) < eps ? 3 : 0));
        flags[0] = (unsigned)k;
        if (stats != nullptr) {
            atomicAdd(&stats[0], (unsigned long long)(k ? k : 4));
            if (k) atomicAdd(&stats[1], 1ull);
        }
    }
}

// x_K = J^K(x0) at one point (boundary points pass through)
template <int K, class T>
__device__ T fxs(const T *x0, const T *f, long long P, int N, T hh, int j, int i)
{
    if constexpr (K == 0) {
        return x0[(long long)j * P + i];
    } else {
        if (j <= 0 || i <= 0 || j >= N - 1 || i >= N - 1) return x0[(long long)j * P + i];
        return T(0.25) * ((hh * f[(long long)j * P + i]) + fxs<K - 1>(x0, f, P, N, hh, j, i - 1) +
                          fxs<K - 1>(x0, f, P, N, hh, j, i + 1) +
                          fxs<K - 1>(x0, f, P, N, hh, j - 1, i) +
                          fxs<K - 1>(x0, f, P, N, hh, j + 1, i));
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_smooth4_fix(const unsigned *flags, const T *x0, const T *f,
                                                     T *out, long long P, int N, T hh, int row_lo,
                                                     int row_hi)
{
    const unsigned k = flags[0];
    if (k == 0) return;   // uniform: the normal case
    const long long W = N - 2;
    const long long n = (long long)(row_hi - row_lo) * W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const int j = row_lo + (int)(q / W), i = 1 + (int)(q % W);
        T v;
        if (k == 1) v = fxs<1>(x0, f, P, N, hh, j, i);
        else if (k == 2) v = fxs<2>(x0, f, P, N, hh, j, i);
        else v = fxs<3>(x0, f, P, N, hh, j, i);
        out[(long long)j * P + i] = v;
    }
}

template <class T>
void launch_smooth4_finish(const PostPreArgsT<T> &a, int np, const double *global3, double eps,
                           unsigned *flags, unsigned long long *stats, hipStream_t s)
{
    k_smooth4_decide<<<dim3(1), dim3(256), 0, s>>>(a.partials1, a.partials2, a.partials3, np,
                                                    global3, eps, flags, stats);
    const int blocks = std::max(1, std::min(1024, (int)(((long long)(a.row_hi - a.row_lo) * a.N + 255) / 256)));
    k_smooth4_fix<T><<<dim3(blocks), dim3(256), 0, s>>>(flags, a.phi, a.f, a.x4, a.P, a.N, a.hh,
                                                        a.row_lo, a.row_hi);
}

#define PGMG_INSTANTIATE(T)                                                                       \
    template void launch_pre_fixup<T>(const FixArgsF &, const PreArgsT<T> &, bool, hipStream_t);  \
    template void launch_post_fixup<T>(const FixArgsF &, const PostArgsT<T> &, hipStream_t);      \
    template void launch_smooth4_finish<T>(const PostPreArgsT<T> &, int, const double *, double,  \
                                           unsigned *, unsigned long long *, hipStream_t);
PGMG_INSTANTIATE(double)
PGMG_INSTANTIATE(float)
#undef PGMG_INSTANTIATE

}  // namespace pgmg
