// pgmg_post.hip — k_post: a level's prolongation and post-smooth as one HBM pass.
//
// With v = 1 the reference smoother runs two sweeps and checks ||r(x1)|| < eps after
// the first.  Instead of three passes (prolongation, 2 sweeps) the way up a level is one:
//
//   k_post: phi, ec, f -> x_eff = phi + P ec -> x1 = J(x_eff) -> x2 = J(x1)
//           writes x2 (back into the level's solution buffer); sum r(x1)^2 per block
//           (MultiGrid.hpp:86-89 + Smoother.hpp:59-88)
//
// 24+2 B/point instead of 64 (RECOMP, the levels entered with x0 = 0: phi is recomputed from
// f, 16 B/point less).  Speculative in the early exit like k_pre (pgmg_pre.hip): the rare path
// is k_post_rare in-stream or the scalar k_post_fixup (pgmg_fixup.hip), k_post1 the pass of a
// check predicted to fire.  k_post_r2 is the finest level's last pass of an F-cycle that
// another follows: it also restricts its result twice, into level 2.
//
// Rows march down a band as in k_pre (wave tiles: pgmg_fused_dev.h), 2 rows of x_eff above
// and below the band.
#include <algorithm>

#include "pgmg.h"
#include "pgmg_fused_dev.h"

namespace pgmg {

// full weighting of one point from its 3x3 neighbourhood (rows u / m / d = above / centre /
// below, columns w / c / e): MultiGrid.hpp:187-205's expression and operand order (the same as
// pgmg_kernels.hip's rfw for k_restrict2_values)
template <class T>
__device__ __forceinline__ T rfw_post(T u_w, T u_c, T u_e, T m_w, T m_c, T m_e, T d_w, T d_c, T d_e)
{
    return T(0.25) * m_c + T(0.125) * (m_e + m_w + d_c + u_c) + T(0.0625) * (u_w + u_e + d_w + d_e);
}

// R2 (k_post_r2, the finest level's last pass of an F-cycle that another one follows): the next
// F-cycle starts by restricting this pass's result twice (compute_coarsest_grid, MultiGrid.hpp:
// 28-55; the level-1 values are dead), so the pass forms level 2 itself from the x2 rows it
// holds.  The band starts 4 rows earlier and ends 6 rows later (x2 valid on fine rows 2jcb-4 ..
// 2jce+1 instead of its own 2jcb .. 2jce-1; only its own rows are stored), the last two x2 rows
// and level-1 rows stay in registers, lane t forms the level-1 value at fine column c+1 (its
// east column from lane t+1 by DPP) and the level-2 centre lanes (level-1 column even) the
// level-2 value from lanes t-1 .. t+1.  A band owns the level-2 rows r2 with 4 r2 in its own
// fine rows; a wave the level-2 columns whose centre fine column it owns.  A level-2 point
// reads x2 three columns past its centre each side, so the wave tiles are 116 columns apart
// with a 6-column margin (lanes 3 .. 60 own, instead of 120 / 4 and lanes 2 .. 61) and lane 63
// loads its own east coarse column (x_eff, x1, x2 then valid on tile columns 0 .. 127, 1 .. 126,
// 2 .. 125): every owned centre's window (at most columns 2t-2 .. 2t+4 of lane t <= 60) is in
// the tile.
// RECOMP (levels entered with x0 = 0): phi is not read.  The loaded row is f[ii+1];
// x1 = J(0) is pointwise, so x1 row ii+1 -> phi row ii = J(x1) (or x1 when the pre
// check fired) -> x_eff row ii: one more row of lag than reading phi, 16 B/point less.
template <class T, bool FINE, int PAIRS, bool RECOMP, bool GENF, bool S1, bool S1P = false,
          bool R2 = false>
__device__ __forceinline__ void post_body(const PostArgsT<T> &a, double *red)
{
    constexpr int R = 2 * PAIRS;
    if (a.cond != nullptr && *a.cond == 0u) return;  // conditional (rare-path) launch
    int lbx, lby;
    fused_block(lbx, lby, (a.nt & 16) != 0);
    // R2: 116-column stride, 6-column margin (kR2Stride): see k_post_r2
    const Cols k = R2 ? lane_cols_t<kR2Stride, 6>(a.N, lbx) : lane_cols(a.N, lbx);
    const int N = a.N, Nc = a.Nc;
    const long long P = a.P, Pc = a.Pc;
    const int jcb = a.jc0 + lby * a.rows_per_block;
    const int jce = min(jcb + a.rows_per_block, a.jc1);
    const int olo = max(2 * jcb, a.row_lo), ohi = min(2 * jce, a.row_hi);
    const int slo = a.sum_hi > a.sum_lo ? max(olo, a.sum_lo) : olo;
    const int shi = a.sum_hi > a.sum_lo ? min(ohi, a.sum_hi) : ohi;
    if (!S1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.stats != nullptr)
        atomicAdd(&a.stats[0], (unsigned long long)(2 + a.sw_adj));
    ProlongCols pc;
    pc.ic = (k.c - 1) >> 1;
    pc.vx = k.c >= 3 && k.c <= N - 2;
    pc.vy = k.c + 1 >= 2 && k.c + 1 <= N - 3;
    const T *__restrict__ F = a.f + k.c;
    const double fxa = GENF ? a.gfx[k.c] : 0.0, fxb = GENF ? a.gfx[k.c + 1] : 0.0;
    // the streamed array: phi, or f one row ahead (RECOMP)
    const T *__restrict__ X = RECOMP ? F + P : a.phi + k.c;
    const T *__restrict__ E = a.ec + pc.ic;
    T *__restrict__ O = a.x2 + k.c;
    const long long Po = a.Po != 0 ? a.Po : P;   // x2's pitch (the caller's array: N)
    const T hh = a.hh, ih = a.ih;
    const V2<T> z = zero2<T>();
    // windows: x_eff rows i-2,i-1 ; x1 rows i-3,i-2 ; f rows i-2,i-1
    V2<T> a0 = z, a1 = z, b0 = z, b1 = z, f1 = z, f2 = z;
    // RECOMP: pre-smooth x1 rows ii-1, ii ; f row ii
    V2<T> g0 = z, g1 = z, fc = z;
    double acc = 0.0;
    const int i_begin = 2 * jcb - 2 - (R2 ? 4 : 0);
    const int c0w = __builtin_amdgcn_readfirstlane(k.c - 2 * (int)(threadIdx.x & 63));
    const bool idle = c0w + 4 > N - 2;  // spare wave (wave-uniform)
    const bool inner = c0w >= 3 && c0w + 127 <= N - 3;   // see pre_body
    const int i_end = idle ? i_begin
                           : i_begin + ((2 * (jce - jcb) + (R2 ? 10 : 4) + R - 1) / R) * R;
    const bool pfired = RECOMP && *a.pre_fired != 0u;
    // R2: x2 rows q-2, q-1 and level-1 rows r1-2, r1-1 of this lane's level-1 column i1
    V2<T> q0 = z, q1 = z;
    T w0 = T(0), w1 = T(0);
    const int i1 = (k.c + 1) >> 1, i2 = i1 >> 1;
    const bool lane63 = (threadIdx.x & 63) == 63;
    const bool eall = R2 && (a.nt & 8) != 0;   // every lane loads its east coarse column
    const bool r2col = R2 && (i1 & 1) == 0 && k.own && i2 >= 1 && i2 <= a.Nr2 - 2;
    if (RECOMP && !idle) {
        const V2<T> fm = ldv(F + (i_begin - 1) * P);
        fc = ldv(F + i_begin * P);
        g0 = j0stage(fm, hh, k, boundary_row(i_begin - 1, N));
        g1 = j0stage(fc, hh, k, boundary_row(i_begin, N));
    }
    // coarse row m = ii/2 of fine row ii; an iteration of R rows uses coarse rows
    // i/2 .. i/2 + PAIRS
    V2<T> np_[R], nf[R];
    T ncr[PAIRS + 1], ncre[PAIRS + 1];   // ncre (R2): lane 63's east coarse column
    #pragma unroll
    for (int q = 0; q < R; ++q) {
        np_[q] = idle ? z : ldv(X + (i_begin + q) * P);
        if (!RECOMP && !GENF) nf[q] = idle ? z : ldv(F + (i_begin + q) * P);
    }
    #pragma unroll
    for (int q = 0; q <= PAIRS; ++q) {
        ncr[q] = idle ? T(0) : E[(long long)((i_begin >> 1) + q) * Pc];
        if (R2) ncre[q] = idle || !(lane63 || eall) ? T(0) : E[(long long)((i_begin >> 1) + q) * Pc + 1];
    }
    // FULL: as in pre_body (rows interior to the band, the sum range and the grid; interior
    // wave columns)
    auto full_at = [&](int i) {
        return !S1 && inner && i >= 3 && i + R <= N - 2 && i - 2 >= slo && i + R - 3 < shi &&
               ((i + R - 1) >> 1) <= Nc - 2;
    };
    auto iter = [&](int i, auto full_t) {
        V2<T> cp[R], cf[R];
        T cr[PAIRS + 1], cre[PAIRS + 1];
        #pragma unroll
        for (int q = 0; q < R; ++q) {
            cp[q] = np_[q];
            if (!RECOMP && !GENF) cf[q] = nf[q];
        }
        #pragma unroll
        for (int q = 0; q <= PAIRS; ++q) {
            cr[q] = ncr[q];
            if (R2) cre[q] = ncre[q];
        }
        if (i + R < i_end) {
            #pragma unroll
            for (int q = 0; q < R; ++q) {
                np_[q] = ldv(X + (i + R + q) * P);
                if (!RECOMP && !GENF) nf[q] = ldv(F + (i + R + q) * P);
            }
            #pragma unroll
            for (int q = 0; q <= PAIRS; ++q) {
                ncr[q] = E[(long long)(((i + R) >> 1) + q) * Pc];
                if (R2 && (lane63 || eall)) ncre[q] = E[(long long)(((i + R) >> 1) + q) * Pc + 1];
            }
        }
        T crn[PAIRS + 1];
        #pragma unroll
        for (int q = 0; q <= PAIRS; ++q) {
            crn[q] = dpp_shl(cr[q]);
            // R2: lane 63's own east column, so x_eff is valid on all 128 columns of the tile
            if (R2 && (lane63 || eall)) crn[q] = cre[q];
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
                const int pq = s >> 1;
                V2<T> ph, f3;
                if (RECOMP) {
                    const V2<T> fn = cp[s];  // f row ii+1
                    const V2<T> g2 = j0stage<T, !FULL>(fn, hh, k, boundary_row(ii + 1, N));
                    ph = pfired ? g1 : jstage<T, !FULL>(g0, g1, g2, fc, hh, k, boundary_row(ii, N));
                    f3 = fc;
                    g0 = g1;
                    g1 = g2;
                    fc = fn;
                } else {
                    ph = cp[s];
                    if constexpr (GENF) {
                        f3 = mk2<T>((T)(fxa * gy[s]), (T)(fxb * gy[s]));
                    } else {
                        f3 = cf[s];
                    }
                }
                const V2<T> a2 = add_prolong<T, !FULL>(ph, ii, cr[pq], crn[pq], cr[pq + 1], crn[pq + 1], pc, Nc);
                const V2<T> b2 = jstage<T, !FULL>(a0, a1, a2, f2, hh, k, boundary_row(ii - 1, N));
                if constexpr (S1) {   // the post check fired: x1 row ii-1 is the result
                    if (ii - 1 >= olo && ii - 1 < ohi && k.own) stvu(O + (ii - 1) * Po, b2);
                    if constexpr (S1P) {   // the check's terms: r(x1) on row ii-2 (k_post1)
                        const int row = ii - 2;
                        const V2<T> r1 = rstage(b0, b1, b2, f1, ih);
                        if constexpr (R2 && chk_sel_lv<T>()) {
                            acc = chk_acc<T>(acc, r1, row >= slo && row < shi && k.own, k.by);
                        } else if (row >= slo && row < shi && k.own) {
                            acc = sqacc(acc, r1.x);
                            if (!k.by) acc = sqacc(acc, r1.y);
                        }
                        b0 = b1;
                        b1 = b2;
                    }
                    a0 = a1;
                    a1 = a2;
                    f1 = f2;
                    f2 = f3;
                    continue;
                }
                {
                    const int row = ii - 2;
                    const V2<T> r1 = rstage(b0, b1, b2, f1, ih);
                    if constexpr (R2 && chk_sel_lv<T>()) {
                        acc = chk_acc<T>(acc, r1, (FULL || (row >= slo && row < shi)) && k.own, !FULL && k.by);
                    } else if ((FULL || (row >= slo && row < shi)) && k.own) {
                        acc = sqacc(acc, r1.x);
                        if (FULL || !k.by) acc = sqacc(acc, r1.y);
                    }
                }
                const V2<T> c2 = jstage<T, !FULL>(b0, b1, b2, f1, hh, k, boundary_row(ii - 2, N));
                if ((FULL || (ii - 2 >= olo && ii - 2 < ohi)) && k.own) {
                    if (a.nt & 4) stv_nt(O + (ii - 2) * Po, c2);
                    else stvu(O + (ii - 2) * Po, c2);
                }
                if constexpr (R2) {
                    // x2 row q = ii - 2 (i is even: q is odd exactly for odd s)
                    if (s & 1) {   // q = 2 r1 + 1: level-1 row r1 from x2 rows q-2, q-1, q
                        const T v1 = rfw_post<T>(q0.x, q0.y, dpp_shl(q0.x), q1.x, q1.y, dpp_shl(q1.x),
                                                 c2.x, c2.y, dpp_shl(c2.x));
                        const int r1 = (ii - 3) >> 1;
                        if (r1 & 1) {   // r1 = 2 r2 + 1 (wave-uniform): level-2 row r2
                            const T v2 = rfw_post<T>(dpp_shr(w0), w0, dpp_shl(w0), dpp_shr(w1), w1,
                                                     dpp_shl(w1), dpp_shr(v1), v1, dpp_shl(v1));
                            const int r2 = r1 >> 1;
                            if (r2col && 4 * r2 >= olo && 4 * r2 < ohi && r2 >= 1 && r2 <= a.Nr2 - 2)
                                a.r2out[(long long)r2 * a.Pr2 + i2] = v2;
                        }
                        w0 = w1;
                        w1 = v1;
                    }
                    q0 = q1;
                    q1 = c2;
                }
                a0 = a1;
                a1 = a2;
                b0 = b1;
                b1 = b2;
                f1 = f2;
                f2 = f3;
            }
        }
    };
    // (one loop with the path chosen per iteration: the 12-row form of k_pre costs k_post
    // 150 -> 210 VGPRs, i.e. 3 -> 2 waves per SIMD, and measured slower; hoisting the pre
    // check's outcome out of the loop measured no gain)
    row_loop<R, 0>(i_begin, i_end, full_at, iter);
    if constexpr (!S1 || S1P) {
        const double sum = block_sum(acc, red);
        if (threadIdx.x == 0) a.partials[lby * gridDim.x + lbx] = sum;
    }
}

template <class T, bool FINE, int PAIRS, bool RECOMP, bool GENF = false>
__global__ __launch_bounds__(256) void k_post(PostArgsT<T> a)
{
    __shared__ double red[4];
    post_body<T, FINE, PAIRS, RECOMP, GENF, false>(a, red);
}

// the finest level's last pass of an F-cycle with the next F-cycle's level-2 restriction
template <class T, bool GENF>
__global__ __launch_bounds__(256) void k_post_r2(PostArgsT<T> a)
{
    __shared__ double red[4];
    post_body<T, true, 2, false, GENF, false, false, true>(a, red);
}

// a coarse level's post-smooth whose check is predicted to fire (see k_pre1): x1 is the
// result (RECOMP: the pre-smoothed iterate recomputed as the pre check decided; otherwise read),
// one sweep and one exit booked, the check's partials written
template <class T, int PAIRS, bool RECOMP>
__global__ __launch_bounds__(256) void k_post1(PostArgsT<T> a)
{
    __shared__ double red[4];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && a.stats != nullptr) {
        atomicAdd(&a.stats[0], 1ull);
        atomicAdd(&a.stats[1], 1ull);
    }
    post_body<T, false, PAIRS, RECOMP, false, true, true>(a, red);
}

// rare path of k_post's check (replaces the scalar k_post_fixup on in-stream levels)
template <class T, int PAIRS, bool RECOMP>
__global__ __launch_bounds__(256) void k_post_rare(PostArgsT<T> a, FixArgsF f)
{
    __shared__ double red[4];
    __shared__ int trig;
    if (!check_decide(f.partials, f.np, f.eps, f.global_sum, f.stats, red, &trig)) return;
    __syncthreads();
    post_body<T, false, PAIRS, RECOMP, false, true>(a, red);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// phi (unless recomputed from f), f (unless regenerated), ec in; x2 out
template <class T>
static double post_bytes(const PostArgsT<T> &a)
{
    const double n = row_pts(std::max(2 * a.jc0, a.row_lo), std::min(2 * a.jc1, a.row_hi), a.N);
    const double nc = row_pts(std::max(a.jc0, 1), std::min(a.jc1 + 1, a.Nc - 1), a.Nc);
    return (8.0 * n * ((a.pre_fired == nullptr ? 1 : 0) + (a.gfx == nullptr ? 1 : 0) + 1) + 8.0 * nc) *
           sizeof(T) / 8.0;
}

template <class T>
int launch_post(const PostArgsT<T> &a0, bool fine, hipStream_t s)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r);
    if (const int e = post_spans(a0, t, gx, r, a0.gfx == nullptr)) return e;
    PostArgsT<T> a = a0;
    a.rows_per_block = r;
    // fine k_post: 1.01 -> 0.93 ms with non-temporal stores
    a.nt = (fine ? 4 : 0) | (tuning_int("PGMG_FUSED_XCD", 1) ? 16 : 0);
    const dim3 g(gx, gy), b(t);
    const bool rec = a.pre_fired != nullptr;
    if (fine && a.gfx != nullptr) launchk(k_post<T, true, 2, false, true>, g, b, s, a);
    else if (fine) launchk(k_post<T, true, 2, false>, g, b, s, a);
    else if (rec) launchk(k_post<T, false, 2, true>, g, b, s, a);
    else if (a.gfx != nullptr) launchk(k_post<T, false, 2, false, true>, g, b, s, a);
    else launchk(k_post<T, false, 2, false>, g, b, s, a);
    g_last_launch.bytes = post_bytes(a);
    return PGMG_OK;
}

template <class T>
int launch_post_r2(const PostArgsT<T> &a0, hipStream_t s)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r, kR2Stride, r2_target());
    if (a0.r2out == nullptr || a0.pre_fired != nullptr || a0.Po != 0 || a0.Nr2 < 3 ||
        4 * (a0.Nr2 - 1) != a0.N - 1)
        return PGMG_ERR_ARG;
    if (const int e = post_spans(a0, t, gx, r, a0.gfx == nullptr, true)) return e;
    PGMG_SPAN(a0.r2out, a0.Pr2, 1, a0.Nr2 - 2, 1, a0.Nr2 - 2, "k_post_r2 level-2 restriction");
    PostArgsT<T> a = a0;
    a.rows_per_block = r;
    a.nt = 4 | (tuning_int("PGMG_R2_EALL", 0) ? 8 : 0) | (tuning_int("PGMG_F_XCD", 1) ? 16 : 0);
    const dim3 g(gx, gy), b(t);
    if (a.gfx != nullptr) launchk(k_post_r2<T, true>, g, b, s, a);
    else launchk(k_post_r2<T, false>, g, b, s, a);
    // k_post's, plus the level-2 restriction written
    g_last_launch.bytes = post_bytes(a) + 8.0 * row_pts(1, a.Nr2 - 1, a.Nr2) * sizeof(T) / 8.0;
    return PGMG_OK;
}

// The one-sweep passes (k_post_rare, k_post1) run with the full pass's geometry and spans, f
// streamed (the stored f is valid whenever a pass regenerates it in-kernel) and plain stores:
// the arguments as launched in a, the grid in g and b.
template <class T>
static int post1_setup(const PostArgsT<T> &a0, PostArgsT<T> &a, dim3 &g, dim3 &b)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r);
    if (const int e = post_spans(a0, t, gx, r, true)) return e;
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
int launch_post_rare(const FixArgsF &f, const PostArgsT<T> &a0, hipStream_t s)
{
    PostArgsT<T> a;
    dim3 g, b;
    if (const int e = post1_setup(a0, a, g, b)) return e;
    if (a.pre_fired != nullptr) k_post_rare<T, 2, true><<<g, b, 0, s>>>(a, f);
    else k_post_rare<T, 2, false><<<g, b, 0, s>>>(a, f);
    return PGMG_OK;
}

// the predicted-to-fire pass of a coarse level (RECOMP, or phi read)
template <class T>
int launch_post1(const PostArgsT<T> &a0, hipStream_t s)
{
    PostArgsT<T> a;
    dim3 g, b;
    if (const int e = post1_setup(a0, a, g, b)) return e;
    if (a.pre_fired != nullptr) k_post1<T, 2, true><<<g, b, 0, s>>>(a);
    else k_post1<T, 2, false><<<g, b, 0, s>>>(a);
    return PGMG_OK;
}

#define PGMG_INSTANTIATE(T)                                                                  \
    template int launch_post<T>(const PostArgsT<T> &, bool, hipStream_t);                    \
    template int launch_post_r2<T>(const PostArgsT<T> &, hipStream_t);                       \
    template int launch_post1<T>(const PostArgsT<T> &, hipStream_t);                         \
    template int launch_post_rare<T>(const FixArgsF &, const PostArgsT<T> &, hipStream_t);
PGMG_INSTANTIATE(double)
PGMG_INSTANTIATE(float)
#undef PGMG_INSTANTIATE

}  // namespace pgmg
