// pgmg_pre.hip — k_pre: a level's pre-smooth, residual and restriction as one HBM pass.
//
// With v = 1 the reference smoother runs two sweeps and checks ||r(x1)|| < eps after
// the first (the check after the last sweep cannot change the result).  Instead of three
// passes (2 sweeps, residual+restriction) the way down a level is one:
//
//   k_pre : x0, f  -> x1 = J(x0) -> x2 = J(x1) -> r = f - A x2 -> rc = R r(x2)
//           writes x2 (into the ping-pong buffer) and rc; sum r(x1)^2 per block
//           (MultiGrid.hpp:66-78 + Smoother.hpp:59-88)
//
// 26 B/point instead of 64.  The pass is speculative in the early exit: when
// ||r(x1)|| < eps fires (rare; never on fine levels in practice) the rare path (k_pre_rare
// in-stream, or the scalar k_pre_fixup of pgmg_fixup.hip) recomputes the exact reference
// result (x1 instead of x2, and rc from r(x1)) from the still-intact inputs; k_pre1 is that
// result in one launch for a check predicted to fire.
//
// Rows march down a band with every stage lagging one row behind the previous one (wave
// tiles: pgmg_fused_dev.h); the pipeline needs 4 rows of x0 above and below the band (the
// halo rows are re-read by the neighbouring band, mostly from L2 / Infinity Cache).
#include <algorithm>

#include "pgmg.h"
#include "pgmg_fused_dev.h"

namespace pgmg {

// GENF: f is the analytic RHS, regenerated per row from the gfx/gsy tables (see k_postpre_lds)
// PIN (F-cycle): x0 = (+0) + P ec (a.pin_ec), computed per row from the coarse rows
// (2 B/point read instead of 8, and the prolongation pass into the zeroed grid is gone)
// S1 (rare path of an in-stream check, k_pre_rare): the check after the first sweep fired,
// so the pass is redone with ONE sweep — x1 stored instead of x2, rc = R r(x1) — and
// writes no partial sums and no sweep count (the decision kernel's job)
// S1P (a pre check predicted to fire, k_pre1): the S1 pass that also writes the per-block
// partials of the check's r(x1)^2 (the same terms, rows and order as the full pass), so the
// speculative call's validation can confirm the prediction
template <class T, bool X0_ZERO, bool FINE, int PAIRS, bool GENF, bool PIN, bool S1, bool S1P = false>
__device__ __forceinline__ void pre_body(const PreArgsT<T> &a, double *red)
{
    constexpr int R = 2 * PAIRS;  // rows loaded per iteration (and prefetched ahead)
    if (a.cond != nullptr && *a.cond == 0u) return;  // conditional (rare-path) launch
    int lbx, lby;
    fused_block(lbx, lby, (a.nt & 16) != 0);
    const Cols k = lane_cols(a.N, lbx);
    const int N = a.N;
    const long long P = a.P;
    const int jcb = a.jc0 + lby * a.rows_per_block;
    const int jce = min(jcb + a.rows_per_block, a.jc1);
    const int olo = max(2 * jcb, a.row_lo), ohi = min(2 * jce, a.row_hi);  // x2 rows written
    const int clo = max(jcb, max(1, a.rc_lo)), chi = min(jce, min(N / 2, a.rc_hi));  // rc rows
    if (!S1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (a.stats != nullptr) atomicAdd(&a.stats[0], 2ull);
        // the pre check's outcome for k_post RECOMP: "did not fire" unless a rare path or the
        // predicted-to-fire pass says otherwise (a level's visits share the flag: a W-cycle's
        // visit recorded "does not fire" may follow one predicted to fire)
        if (a.fired != nullptr) *a.fired = 0u;
    }
    const T *__restrict__ X = a.x0 + k.c;
    const long long Px = a.Px != 0 ? a.Px : P;   // x0's pitch (the caller's array: N)
    const T *__restrict__ F = a.f + k.c;
    const double fxa = GENF ? a.gfx[k.c] : 0.0, fxb = GENF ? a.gfx[k.c + 1] : 0.0;
    const bool store = a.x2 != nullptr;
    T *__restrict__ O = a.x2 + k.c;
    const T hh = a.hh, ih = a.ih;
    const V2<T> z = zero2<T>();
    // windows: x0 rows i-2,i-1 ; x1 rows i-3,i-2 ; x2 rows i-4,i-3 ; r rows i-5,i-4 ;
    //          f rows i-3,i-2,i-1
    V2<T> a0 = z, a1 = z, b0 = z, b1 = z, c0 = z, c1 = z, d0 = z, d1 = z, f0 = z, f1 = z, f2 = z;
    V2<T> q0 = z, q1 = z;   // S1: r(x1) rows ii-4, ii-3
    double acc = 0.0;
    // steps [i_begin, i_end): rows 2jcb-4 .. 2jce+3, rounded up to whole iterations
    // (the extra rows are computed but never stored; kHalo covers their loads)
    const int i_begin = 2 * jcb - 4;
    // a wave whose owned columns all lie past the grid (the last block's spare
    // waves) streams nothing; it still joins the block reduction below
    // (c0w: the wave's first column, wave-uniform, so the row loop is scalar-controlled)
    const int c0w = __builtin_amdgcn_readfirstlane(k.c - 2 * (int)(threadIdx.x & 63));
    const bool idle = c0w + 4 > N - 2;
    // wave-uniform: no lane has a boundary column and every prolongation column pair is
    // corrected (c0 >= 3, c0 + 127 <= N - 3)
    const bool inner = c0w >= 3 && c0w + 127 <= N - 3;
    const int i_end = idle ? i_begin
                           : i_begin + ((2 * (jce - jcb) + 8 + R - 1) / R) * R;
    V2<T> nx[R], nf[R];
    // PIN: coarse rows (i >> 1) .. (i >> 1) + PAIRS of an iteration starting at row i
    ProlongCols pc;
    pc.ic = (k.c - 1) >> 1;
    pc.vx = k.c >= 3 && k.c <= N - 2;
    pc.vy = k.c + 1 >= 2 && k.c + 1 <= N - 3;
    const T *__restrict__ E = PIN ? a.pin_ec + pc.ic : nullptr;
    const long long Pc = a.Pc;
    // both coarse columns ic and ic+1 are loaded (no DPP for ic+1): the wave's last lane
    // needs column ic+1 too, since k_pre's four stencil levels after x0 use the whole
    // 4-column margin of the 128-column tile
    T ncr[PAIRS + 1], ncrn[PAIRS + 1];
    #pragma unroll
    for (int q = 0; q < R; ++q) {
        nx[q] = (X0_ZERO || PIN || idle) ? z : ldvu(X + (i_begin + q) * Px);
        if constexpr (!GENF) nf[q] = idle ? z : ldv(F + (i_begin + q) * P);
    }
    if constexpr (PIN) {
        #pragma unroll
        for (int q = 0; q <= PAIRS; ++q) {
            ncr[q] = idle ? T(0) : E[(long long)((i_begin >> 1) + q) * Pc];
            ncrn[q] = idle ? T(0) : E[(long long)((i_begin >> 1) + q) * Pc + 1];
        }
    }
    // FULL: every row of the iteration is interior to the band, the grid and the restriction
    // range, and the wave's columns are all interior (no boundary column, every prolongation
    // column corrected): the per-row range checks and the boundary selects drop out.  The
    // condition holds on one contiguous run of iterations (each clause bounds i from one side)
    auto full_at = [&](int i) {
        return !S1 && inner && i >= 3 && i + R <= N && i - 2 >= olo && i + R - 3 < ohi &&
               ((i - 4) >> 1) >= clo && ((i + R - 6) >> 1) < chi &&
               (!PIN || ((i >> 1) >= 1 && ((i + R - 1) >> 1) <= a.Nc - 2));
    };
    auto iter = [&](int i, auto full_t) {
        V2<T> cx[R], cf[R];
        T cr[PAIRS + 1], crn[PAIRS + 1];
        #pragma unroll
        for (int q = 0; q < R; ++q) {
            cx[q] = nx[q];
            if constexpr (!GENF) cf[q] = nf[q];
        }
        if constexpr (PIN) {
            #pragma unroll
            for (int q = 0; q <= PAIRS; ++q) {
                cr[q] = ncr[q];
                crn[q] = ncrn[q];
            }
        }
        if (i + R < i_end) {  // prefetch the next R rows
            #pragma unroll
            for (int q = 0; q < R; ++q) {
                if (!X0_ZERO && !PIN) nx[q] = ldvu(X + (i + R + q) * Px);
                if constexpr (!GENF) nf[q] = ldv(F + (i + R + q) * P);
            }
            if constexpr (PIN) {
                #pragma unroll
                for (int q = 0; q <= PAIRS; ++q) {
                    ncr[q] = E[(long long)(((i + R) >> 1) + q) * Pc];
                    ncrn[q] = E[(long long)(((i + R) >> 1) + q) * Pc + 1];
                }
            }
        }
        double gy[R];   // GENF row factors of the iteration, loaded together up front
        if constexpr (GENF) {
            #pragma unroll
            for (int q = 0; q < R; ++q) gy[q] = gsy_s(a.gsy, i + q);
        }
        {
            constexpr bool FULL = decltype(full_t)::value;
            #pragma unroll
            for (int s = 0; s < R; ++s) {
                const int ii = i + s;
                V2<T> a2 = cx[s];
                if constexpr (PIN) {
                    const int pq = s >> 1;
                    a2 = add_prolong<T, !FULL>(z, ii, cr[pq], crn[pq], cr[pq + 1], crn[pq + 1], pc, a.Nc);
                }
                V2<T> f3;
                if constexpr (GENF) {
                    f3 = mk2<T>((T)(fxa * gy[s]), (T)(fxb * gy[s]));
                } else {
                    f3 = cf[s];
                }
                // x1 row ii-1
                const V2<T> b2 = (X0_ZERO && !PIN) ? j0stage<T, !FULL>(f2, hh, k, boundary_row(ii - 1, N))
                                                   : jstage<T, !FULL>(a0, a1, a2, f2, hh, k, boundary_row(ii - 1, N));
                // r(x1) and x2 on row ii-2
                const V2<T> r1 = rstage(b0, b1, b2, f1, ih);
                if constexpr (S1) {
                    // x1 row ii-1 is the result; restriction of r(x1): rows ii-4, ii-3, ii-2 =
                    // 2jc-1, 2jc, 2jc+1 when ii is odd
                    if (store && ii - 1 >= olo && ii - 1 < ohi && k.own) stv(O + (ii - 1) * P, b2);
                    if constexpr (S1P) {   // the check's terms: r(x1) on row ii-2
                        const int row = ii - 2;
                        if (row >= olo && row < ohi && k.own) {
                            acc = sqacc(acc, r1.x);
                            if (!k.by) acc = sqacc(acc, r1.y);
                        }
                    }
                    if ((s & 1) == 1) {
                        const int jc = (ii - 3) >> 1;
                        const T m2 = dpp_shl(q1.x);
                        const T u2 = dpp_shl(q0.x);
                        const T e2 = dpp_shl(r1.x);
                        const int ic = (k.c + 1) >> 1;
                        if (jc >= clo && jc < chi && k.own && ic <= a.Nc - 2) {
                            const T v = T(0.25) * q1.y + T(0.125) * (m2 + q1.x + r1.y + q0.y) +
                                        T(0.0625) * (q0.x + u2 + r1.x + e2);
                            a.rc[(long long)jc * a.Pc + ic] = v;
                        }
                    }
                    q0 = q1;
                    q1 = r1;
                    a0 = a1;
                    a1 = a2;
                    b0 = b1;
                    b1 = b2;
                    f0 = f1;
                    f1 = f2;
                    f2 = f3;
                    continue;
                }
                {
                    const int row = ii - 2;
                    if ((FULL || (row >= olo && row < ohi)) && k.own) {
                        acc = sqacc(acc, r1.x);
                        if (FULL || !k.by) acc = sqacc(acc, r1.y);
                    }
                }
                const V2<T> c2 = jstage<T, !FULL>(b0, b1, b2, f1, hh, k, boundary_row(ii - 2, N));
                if (store && (FULL || (ii - 2 >= olo && ii - 2 < ohi)) && k.own) {
                    if (a.nt & 1) stv_nt(O + (ii - 2) * P, c2);
                    else stv(O + (ii - 2) * P, c2);
                }
                // r(x2) on row ii-3 (garbage on boundary rows; never used there)
                const V2<T> d2 = rstage(c0, c1, c2, f0, ih);
                // restriction: rows ii-5, ii-4, ii-3 = 2jc-1, 2jc, 2jc+1 when ii is even
                if ((s & 1) == 0) {
                    const int jc = (ii - 4) >> 1;
                    const T m2 = dpp_shl(d1.x);
                    const T u2 = dpp_shl(d0.x);
                    const T e2 = dpp_shl(d2.x);
                    const int ic = (k.c + 1) >> 1;
                    if ((FULL || (jc >= clo && jc < chi && ic <= a.Nc - 2)) && k.own) {
                        const T v = T(0.25) * d1.y + T(0.125) * (m2 + d1.x + d2.y + d0.y) +
                                         T(0.0625) * (d0.x + u2 + d2.x + e2);
                        if (a.nt & 2) __builtin_nontemporal_store(v, &a.rc[(long long)jc * a.Pc + ic]);
                        else a.rc[(long long)jc * a.Pc + ic] = v;
                    }
                }
                a0 = a1;
                a1 = a2;
                b0 = b1;
                b1 = b2;
                c0 = c1;
                c1 = c2;
                d0 = d1;
                d1 = d2;
                f0 = f1;
                f1 = f2;
                f2 = f3;
            }
        }
    };
    // (PIN: the 12-row form needs 170 VGPRs, past the 168 of 3 waves per SIMD)
    row_loop<R, PIN ? 0 : 3>(i_begin, i_end, full_at, iter);
    if constexpr (!S1 || S1P) {
        const double sum = block_sum(acc, red);
        if (threadIdx.x == 0) a.partials[lby * gridDim.x + lbx] = sum;
    }
}

template <class T, bool X0_ZERO, bool FINE, int PAIRS, bool GENF = false, bool PIN = false>
__global__ __launch_bounds__(256) void k_pre(PreArgsT<T> a)
{
    __shared__ double red[4];
    pre_body<T, X0_ZERO, FINE, PAIRS, GENF, PIN, false>(a, red);
}

// A coarse level's pre-smooth whose check is predicted to fire (speculative calls, levels that
// converged: pgmg_spec.hip "predicted to fire"): x1 = J(x0) (J(0) on a level entered with
// x0 = 0) is the result, rc = R r(x1), one sweep and one exit booked, the "pre fired" flag the
// level's RECOMP k_post reads set -- what k_pre + k_pre_rare compute when the check fires, in
// one launch; the partials confirm it afterwards
template <class T, bool X0_ZERO, int PAIRS>
__global__ __launch_bounds__(256) void k_pre1(PreArgsT<T> a)
{
    __shared__ double red[4];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (a.fired != nullptr) *a.fired = 1u;
        if (a.stats != nullptr) {
            atomicAdd(&a.stats[0], 1ull);
            atomicAdd(&a.stats[1], 1ull);
        }
    }
    pre_body<T, X0_ZERO, false, PAIRS, false, false, true, true>(a, red);
}

// rare path of k_pre's check (replaces the scalar k_pre_fixup on in-stream levels): when it
// fired, the same fused pass with one sweep; a.fired records the decision for k_post RECOMP
template <class T, bool X0_ZERO, int PAIRS, bool PIN>
__global__ __launch_bounds__(256) void k_pre_rare(PreArgsT<T> a, FixArgsF f)
{
    __shared__ double red[4];
    __shared__ int trig;
    const bool t = check_decide(f.partials, f.np, f.eps, f.global_sum, f.stats, red, &trig);
    if (a.fired != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        *a.fired = t ? 1u : 0u;
    if (!t) return;
    __syncthreads();
    pre_body<T, X0_ZERO, false, PAIRS, false, PIN, true>(a, red);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// The finest level gets its own kernel symbols (FINE) so rocprofv3 statistics
// isolate the roofline kernels.
template <class T>
int launch_pre(const PreArgsT<T> &a0, bool x0_zero, bool fine, hipStream_t s)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r);
    if (const int e = pre_spans(a0, t, gx, r, !x0_zero && a0.pin_ec == nullptr, a0.gfx == nullptr))
        return e;
    PreArgsT<T> a = a0;
    a.rows_per_block = r;
    // non-temporal stores on the finest level only (its x2 is read again a level-pass later;
    // coarse outputs are re-read while still in the caches): fine k_pre 0.99 -> 0.97 ms
    a.nt = (fine ? 1 : 0) | (tuning_int("PGMG_FUSED_XCD", 1) ? 16 : 0);
    const dim3 g(gx, gy), b(t);
    // two row pairs per iteration (r01 sweeps: on x0 = 0 levels 2 as fast as 3 at 8193 and
    // faster below, 4 slower; one pair slower everywhere)
    if (a.pin_ec != nullptr) {   // F-cycle: x0 = prolongation of the coarse grid
        if (fine && a.gfx != nullptr) launchk(k_pre<T, false, true, 2, true, true>, g, b, s, a);
        else if (fine) launchk(k_pre<T, false, true, 2, false, true>, g, b, s, a);
        else if (a.gfx != nullptr) launchk(k_pre<T, false, false, 2, true, true>, g, b, s, a);
        else launchk(k_pre<T, false, false, 2, false, true>, g, b, s, a);
    } else if (x0_zero) {
        launchk(k_pre<T, true, false, 2>, g, b, s, a);
    } else if (fine && a.gfx != nullptr) {
        launchk(k_pre<T, false, true, 2, true>, g, b, s, a);
    } else if (fine) {
        launchk(k_pre<T, false, true, 2>, g, b, s, a);
    } else if (a.gfx != nullptr) {
        launchk(k_pre<T, false, false, 2, true>, g, b, s, a);
    } else {
        launchk(k_pre<T, false, false, 2>, g, b, s, a);
    }
    // x0 (unless zero or the F-cycle's prolongation, which reads the coarse grid instead), f
    // (unless regenerated) in; x2 (unless recomputed later), rc out
    const double n = row_pts(std::max(2 * a.jc0, a.row_lo), std::min(2 * a.jc1, a.row_hi), a.N);
    const double nc = row_pts(a.rc_lo, a.rc_hi, a.Nc);
    const bool rx0 = !x0_zero && a.pin_ec == nullptr;
    g_last_launch.bytes = (8.0 * n * ((rx0 ? 1 : 0) + (a.gfx == nullptr ? 1 : 0) + (a.x2 != nullptr ? 1 : 0)) +
                           8.0 * nc * (a.pin_ec != nullptr ? 2 : 1)) * sizeof(T) / 8.0;
    return PGMG_OK;
}

// The one-sweep passes (k_pre_rare, k_pre1) run with the full pass's geometry and spans, f
// streamed (the stored f is valid whenever a pass regenerates it in-kernel) and plain stores:
// the arguments as launched in a, the grid in g and b.
template <class T>
static int pre1_setup(const PreArgsT<T> &a0, bool x0_read, PreArgsT<T> &a, dim3 &g, dim3 &b)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r);
    if (const int e = pre_spans(a0, t, gx, r, x0_read, true)) return e;
    a = a0;
    a.rows_per_block = r;
    a.gfx = a.gsy = nullptr;
    a.nt = 0;
    g = dim3(gx, gy);
    b = dim3(t);
    return PGMG_OK;
}

// rare path of the in-stream check as a fused one-sweep pass (decision inside; a launch
// that finds the check did not fire returns at once)
template <class T>
int launch_pre_rare(const FixArgsF &f, const PreArgsT<T> &a0, bool x0_zero, hipStream_t s)
{
    PreArgsT<T> a;
    dim3 g, b;
    if (const int e = pre1_setup(a0, !x0_zero && a0.pin_ec == nullptr, a, g, b)) return e;
    if (x0_zero) k_pre_rare<T, true, 2, false><<<g, b, 0, s>>>(a, f);
    else if (a.pin_ec != nullptr) k_pre_rare<T, false, 2, true><<<g, b, 0, s>>>(a, f);
    else k_pre_rare<T, false, 2, false><<<g, b, 0, s>>>(a, f);
    return PGMG_OK;
}

// the predicted-to-fire pass of a coarse level (entered with x0 = 0, or from the previous
// gamma visit's iterate)
template <class T>
int launch_pre1(const PreArgsT<T> &a0, bool x0_zero, hipStream_t s)
{
    PreArgsT<T> a;
    dim3 g, b;
    if (const int e = pre1_setup(a0, !x0_zero, a, g, b)) return e;
    if (x0_zero) k_pre1<T, true, 2><<<g, b, 0, s>>>(a);
    else k_pre1<T, false, 2><<<g, b, 0, s>>>(a);
    return PGMG_OK;
}

#define PGMG_INSTANTIATE(T)                                                                      \
    template int launch_pre<T>(const PreArgsT<T> &, bool, bool, hipStream_t);                    \
    template int launch_pre1<T>(const PreArgsT<T> &, bool, hipStream_t);                         \
    template int launch_pre_rare<T>(const FixArgsF &, const PreArgsT<T> &, bool, hipStream_t);
PGMG_INSTANTIATE(double)
PGMG_INSTANTIATE(float)
#undef PGMG_INSTANTIATE

}  // namespace pgmg
