// pgmg_monitor.hip — the convergence monitor and solve-to-tolerance (include/pgmg.h
// "Convergence monitor and solve-to-tolerance"; DESIGN.md "Convergence monitor").
//
// The reference's driver measures convergence after every cycle (MultigridTestRunner::
// run_cycle, 2_part_MG/MultiGridTestRunner.hpp:190-244: compute_residual + norm, and with
// flag_err_norm_iteration ||phi - u|| / ||u||, :110-122, :252-254).  Here that is ONE streaming
// pass over the finest-level iterate, read where it lies, that yields up to three fp64 sums:
//   sum r^2   interior points of the rows this rank updates,
//             r = f - ih * (4x - x_l - x_r - x_u - x_d)   (DynamicGridUtils.hpp:59-69's order)
//   sum e^2   all points of the rows this rank owns, boundary included, e = (double)phi - u
//   sum u^2   the same points, u = sx[i] * sy[j]           (compute_function's product)
// shaped like the other level-0 passes (pgmg_kernels.hip): lane t of a wave owns a column pair
// (one 16-byte row load), a workgroup marches down a band keeping a three-row window in
// registers (each phi row crosses HBM once per band, plus one halo row at each end), horizontal
// neighbours come through DPP, and kMonU rows are loaded before any is used.
//
// Decomposition (a function of N and the rank's rows [lo, hi) only -- not of pitch, address,
// which array is bound, or the sums asked for): tiles of kMonTile = 512 columns starting at
// column 1 (column 0 rides with lane 0 of the first tile), bands of kMonBand = 64 rows starting
// at row lo.  Every lane adds its terms in row order, the lanes of a wave in wave_sum's fixed
// tree, the four waves in index order; the workgroups' partials are written with plain stores
// and added in index order by k_mon_reduce.  No floating-point atomics: the same state gives the
// same bits.
//
// The damping pass (pgmg_damp; DESIGN.md "Damping pass") is the same kernel with kMonDamp: after
// forming r it also writes x + w r, in place.  Every r must come from the phi of BEFORE the pass,
// and a workgroup's halo rows and edge columns are another workgroup's outputs, so (the scheme of
// k_op_sweep_ip, pgmg_gops.hip) an output another workgroup reads is not written in place but
// deferred to a side buffer: the first row of a band with a band above it and the last row of a
// band with one below -> SR, one row per slot (2 per band); the two columns either side of the
// boundary between tiles e and e+1 (512 (e+1) and the next) -> SC[(e * N + row) * 2 + k].
// k_mon_scatter_rows / _cols write them into phi afterwards, in stream order.  The four waves of
// a workgroup read each other's edge columns: a barrier between an iteration's loads (waited
// for) and its stores orders them (iteration i stores rows no wave loads in iteration i+1 or
// later).  No wave leaves early in this mode (a wave past the last column loads nothing and
// stores nothing), so every barrier is met.  The partial sums are untouched: the norm is the
// monitor's, bit for bit.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <type_traits>

#include "pgmg_host.h"
#include "pgmg_stop.h"

using namespace pgmg;

namespace pgmg {

// (kMonBand, kMonTile, kMonU: pgmg_internal.h, shared with k_defect of pgmg_mixed.hip)

constexpr unsigned kMonRes = PGMG_MON_RESIDUAL, kMonErr = PGMG_MON_ERROR;
constexpr unsigned kMonGen = 4u;       // f regenerated from the sine tables (not streamed)
constexpr unsigned kMonDamp = 8u;      // also write x + w r (with kMonRes)

// SX / SF: the element types phi and a stored f are read as (T, or double for the caller's
// arrays of a device-bound problem, converted on load as launch_from_double converts them)
template <class T, class SX, class SF>
struct MonArgsT {
    const SX *x;             // element (0, 0) of phi, pitch Px
    const SF *f;             // element (0, 0) of the stored f, pitch Pf (unused with kMonGen)
    long long Px, Pf;
    const double *gfx, *gsy; // kMonGen: f = (T)(gfx[i] * gsy[j])
    const double *sx, *sy;   // kMonErr: u = sx[i] * sy[j]
    double *partials;        // 3 per workgroup: sum r^2, sum e^2, sum u^2
    T ih;
    int N;
    int lo, hi;              // rows this rank owns (the error sums' rows)
    int u0, u1;              // interior rows this rank updates (the residual sum's rows)
    SX *xw;                  // kMonDamp: the same array, written
    T *sr, *sc;              // kMonDamp: deferred band-edge rows (pitch N) / tile-edge columns
    T w;                     // kMonDamp: omega h^2 / 4
};

// a column pair read as S, as the context's element type
template <class T, class S> __device__ __forceinline__ V2<T> mon_cv(V2<S> v)
{
    return mk2<T>((T)v.x, (T)v.y);
}

template <class T, class SX, class SF, unsigned MODE>
__global__ __launch_bounds__(kBlock) void k_monitor(MonArgsT<T, SX, SF> a)
{
    constexpr bool RES = (MODE & kMonRes) != 0, ERR = (MODE & kMonErr) != 0;
    constexpr bool GEN = (MODE & kMonGen) != 0;
    constexpr bool DAMP = (MODE & kMonDamp) != 0;
    static_assert(!DAMP || RES, "the damping pass needs the residual");
    __shared__ double red[3][kBlock / 64];
    const int lane = threadIdx.x & 63;
    // (readfirstlane: the wave index, and so every row descriptor, is wave-uniform for the compiler)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N;
    const int npairs = (N - 1) >> 1;                 // pairs (1+2t, 2+2t) cover columns 1 .. N-1
    const int p0 = blockIdx.x * kBlock + wave * 64;  // the wave's first pair
    const int nw = min(max(npairs - p0, 0), 64);     // its pairs
    const int cw = 1 + 2 * p0;                       // its first column
    const int c = cw + 2 * lane;                     // this lane's columns c, c + 1
    const bool act = lane < nw;
    const bool second = c + 1 <= N - 2;              // else column c + 1 is the right boundary
    const bool has_right = cw + 128 <= N - 1;        // lane 63 has a neighbour column in the row
    const int jb = a.lo + blockIdx.y * kMonBand;
    const int je = min(jb + kMonBand, a.hi);
    const long long Px = a.Px, Pf = a.Pf;
    // (DAMP writes the array X reads: no __restrict__ promise there)
    using XPtr = std::conditional_t<DAMP, const SX *, const SX *__restrict__>;
    const XPtr X = a.x;
    const SF *__restrict__ F = a.f;
    const T ih = a.ih;
    using D2 = V2<T>;
    double accr = 0.0, acce = 0.0, accu = 0.0;
    // kMonDamp: the outputs other workgroups read (deferred), and the side buffer's slots
    const bool def_top = blockIdx.y > 0, def_bot = blockIdx.y + 1 < gridDim.y;
    const bool def_l = threadIdx.x == 0 && blockIdx.x > 0;
    const bool def_r = threadIdx.x == kBlock - 1 && blockIdx.x + 1 < gridDim.x;
    const bool on = DAMP ? nw > 0 : true;   // (DAMP: the waves past the last column march too)

    // (wave-uniform; a wave past the last column only joins the block sum and, DAMP, the barriers)
    if (nw > 0 || DAMP) {
        double fx0 = 0.0, fx1 = 0.0, sx0 = 0.0, sx1 = 0.0, sxl = 0.0;
        if (RES && GEN && act) {
            fx0 = a.gfx[c];
            fx1 = a.gfx[c + 1];
        }
        if (ERR && act) {
            sx0 = a.sx[c];
            sx1 = a.sx[c + 1];
            sxl = a.sx[0];
        }
        // rows are clamped into the grid: a clamped row only feeds residuals of rows outside
        // [u0, u1), which are not summed
        auto rowx = [&](int r) -> D2 {
            r = min(max(r, 0), N - 1);
            return mon_cv<T, SX>(buf_row<SX, 0>(X + r * Px + cw, nw, lane));
        };
        D2 w0 = zero2<T>(), w1;
        if (RES) w0 = rowx(jb - 1);
        w1 = rowx(jb);
        for (int j = jb; j < je; j += kMonU) {
            D2 xn[kMonU], fv[kMonU];
            T el[kMonU], er[kMonU];
            #pragma unroll
            for (int u = 0; u < kMonU; ++u) {
                const int r = min(j + u, je - 1);
                xn[u] = rowx(r + 1);
                if (RES && !GEN) fv[u] = mon_cv<T, SF>(buf_row<SF, 0>(F + r * Pf + cw, nw, lane));
                else fv[u] = zero2<T>();
                el[u] = T(0);
                er[u] = T(0);
                if (lane == 0 && on) el[u] = (T)X[r * Px + cw - 1];
                if (RES && lane == 63 && has_right) er[u] = (T)X[r * Px + cw + 128];
            }
            if (DAMP) {   // every wave's loads of this iteration have returned before any store
                __builtin_amdgcn_s_waitcnt(0);
                __syncthreads();
            }
            #pragma unroll
            for (int u = 0; u < kMonU; ++u) {
                const int r = j + u;
                const D2 up = (u == 0) ? w0 : (u == 1 ? w1 : xn[u - 2]);
                const D2 ce = (u == 0) ? w1 : xn[u - 1];
                const D2 dn = xn[u];
                const bool live = act && r < je;
                if (RES) {
                    T left = dpp_shr(ce.y);
                    T right = dpp_shl(ce.x);
                    if (lane == 0) left = el[u];
                    if (lane == 63) right = er[u];
                    D2 fr = fv[u];
                    if (GEN) {
                        const double sy = a.gsy[min(r, N - 1)];
                        fr = mk2<T>((T)(fx0 * sy), (T)(fx1 * sy));
                    }
                    const T r0 = fr.x - ih * (T(4) * ce.x - left - ce.y - up.x - dn.x);
                    const T r1 = fr.y - ih * (T(4) * ce.y - ce.x - right - up.y - dn.y);
                    if (live && r >= a.u0 && r < a.u1) {
                        accr += sq(r0);
                        if (second) accr += sq(r1);
                        if (DAMP) {
                            const T w = a.w;
                            D2 o;
                            o.x = ce.x + w * r0;
                            o.y = second ? ce.y + w * r1 : ce.y;
                            const bool dt = def_top && r == jb, db = def_bot && r == je - 1;
                            const long long by = blockIdx.y, bx = blockIdx.x;
                            if (dt) stvu<T>(a.sr + (2 * by) * N + c, o);
                            if (db) stvu<T>(a.sr + (2 * by + 1) * N + c, o);
                            if (def_l) a.sc[((bx - 1) * N + r) * 2 + 1] = o.x;
                            if (def_r) a.sc[(bx * N + r) * 2] = o.y;
                            if (!dt && !db) {
                                SX *q = a.xw + r * Px + c;
                                if (def_l) {
                                    if (second) q[1] = (SX)o.y;
                                } else if (def_r || !second) {
                                    q[0] = (SX)o.x;
                                } else {
                                    stvu<SX>(q, mk2<SX>((SX)o.x, (SX)o.y));
                                }
                            }
                        }
                    }
                }
                if (ERR) {
                    const double sy = a.sy[min(r, N - 1)];
                    const double u0v = sx0 * sy, u1v = sx1 * sy;
                    const double e0 = (double)ce.x - u0v, e1 = (double)ce.y - u1v;
                    if (live) {
                        acce += e0 * e0;
                        accu += u0v * u0v;
                        acce += e1 * e1;
                        accu += u1v * u1v;
                        if (lane == 0 && cw == 1) {   // column 0
                            const double ul = sxl * sy, elv = (double)el[u] - ul;
                            acce += elv * elv;
                            accu += ul * ul;
                        }
                    }
                }
            }
            w0 = xn[kMonU - 2];
            w1 = xn[kMonU - 1];
        }
    }
    const double sr = wave_sum(accr), se = wave_sum(acce), su = wave_sum(accu);
    if (lane == 0) {
        red[0][wave] = sr;
        red[1][wave] = se;
        red[2][wave] = su;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        #pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
        a.partials[3 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = s;
    }
}

// out[q] = sum over the np workgroups of partials[3 k + q], in a fixed order
__global__ __launch_bounds__(kBlock) void k_mon_reduce(const double *partials, int np, double *out)
{
    __shared__ double red[3][kBlock / 64];
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < np; k += kBlock) {
        #pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += partials[3 * (size_t)k + q];
    }
    #pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double v = wave_sum(s[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        #pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += red[threadIdx.x][w];
        out[threadIdx.x] = t;
    }
}

// The damping pass's deferred outputs into phi, two launches (their shapes differ: the rows are
// coalesced copies that want many threads, the columns scattered 8-byte writes, one row each,
// that go faster with fewer writers in flight -- defer_scatter, pgmg_gops.hip).
// Rows: blockIdx.y = one band-row slot (even: the band's first row when a band lies above it,
// odd: its last when one lies below), the x blocks striding over its interior columns.
template <class T, class SX>
__global__ __launch_bounds__(kBlock) void k_mon_scatter_rows(SX *X, long long Px, const T *SR, int N,
                                                             int lo, int hi, int u0, int u1,
                                                             int bands)
{
    const int tid = blockIdx.x * kBlock + threadIdx.x, nthr = gridDim.x * kBlock;
    const int slot = blockIdx.y, by = slot >> 1;
    const int jb = lo + by * kMonBand, je = min(jb + kMonBand, hi);
    const bool top = (slot & 1) == 0;
    const int row = top ? jb : je - 1;
    if (!(top ? by > 0 : by + 1 < bands) || row < u0 || row >= u1) return;
    const T *src = SR + (long long)slot * N;
    SX *dst = X + row * Px;
    for (int col = 1 + tid; col <= N - 2; col += nthr) dst[col] = (SX)src[col];
}
// Columns: blockIdx.y = tile boundary e (columns 512 (e + 1) and the next), the x blocks striding
// over the updated rows [u0, u1).  A point deferred both ways gets the same value twice.
template <class T, class SX>
__global__ __launch_bounds__(kBlock) void k_mon_scatter_cols(SX *X, long long Px, const T *SC, int N,
                                                             int u0, int u1)
{
    const int tid = blockIdx.x * kBlock + threadIdx.x, nthr = gridDim.x * kBlock;
    const long long e = blockIdx.y;
    const int c0 = kMonTile * ((int)e + 1);
    for (int row = u0 + tid; row < u1; row += nthr) {
        const T *src = SC + (e * N + row) * 2;
        SX *dst = X + row * Px + c0;
        if (c0 <= N - 2) dst[0] = (SX)src[0];
        if (c0 + 1 <= N - 2) dst[1] = (SX)src[1];
    }
}

struct MonGrid {
    int tiles, bands;
};
static MonGrid mon_grid(int N, int lo, int hi)
{
    return {(N - 1 + kMonTile - 1) / kMonTile, (hi - lo + kMonBand - 1) / kMonBand};
}
// elements of the damping pass's side buffer: 2 row slots per band, 2 columns per tile boundary
static size_t mon_side_elems(int N, const MonGrid &mg)
{
    return ((size_t)2 * mg.bands + (size_t)2 * (mg.tiles - 1)) * N;
}

template <class T, class SX, class SF>
static void mon_launch_mode(const MonArgsT<T, SX, SF> &a, unsigned mode, dim3 g, hipStream_t s)
{
    switch (mode) {
    case kMonDamp | kMonRes:
        k_monitor<T, SX, SF, kMonDamp | kMonRes><<<g, dim3(kBlock), 0, s>>>(a);
        break;
    case kMonDamp | kMonRes | kMonGen:
        k_monitor<T, SX, SF, kMonDamp | kMonRes | kMonGen><<<g, dim3(kBlock), 0, s>>>(a);
        break;
    case kMonDamp | kMonRes | kMonErr:
        k_monitor<T, SX, SF, kMonDamp | kMonRes | kMonErr><<<g, dim3(kBlock), 0, s>>>(a);
        break;
    case kMonDamp | kMonRes | kMonErr | kMonGen:
        k_monitor<T, SX, SF, kMonDamp | kMonRes | kMonErr | kMonGen><<<g, dim3(kBlock), 0, s>>>(a);
        break;
    case kMonRes: k_monitor<T, SX, SF, kMonRes><<<g, dim3(kBlock), 0, s>>>(a); break;
    case kMonRes | kMonGen: k_monitor<T, SX, SF, kMonRes | kMonGen><<<g, dim3(kBlock), 0, s>>>(a); break;
    case kMonErr: k_monitor<T, SX, SF, kMonErr><<<g, dim3(kBlock), 0, s>>>(a); break;
    case kMonRes | kMonErr: k_monitor<T, SX, SF, kMonRes | kMonErr><<<g, dim3(kBlock), 0, s>>>(a); break;
    default: k_monitor<T, SX, SF, kMonRes | kMonErr | kMonGen><<<g, dim3(kBlock), 0, s>>>(a); break;
    }
}

// the deferred outputs of a damping pass into x: ~4 columns per thread of a row, ~16 rows per
// thread of a tile boundary
template <class T, class SX>
static void mon_scatter(SX *x, long long Px, const T *sr, const T *sc, int N, int lo, int hi, int u0,
                        int u1, const MonGrid &mg, hipStream_t s)
{
    const int bxr = std::max(1, (N + 4 * kBlock - 1) / (4 * kBlock));
    const int bxc = std::max(1, (N + 16 * kBlock - 1) / (16 * kBlock));
    k_mon_scatter_rows<T, SX><<<dim3(bxr, 2 * mg.bands), dim3(kBlock), 0, s>>>(x, Px, sr, N, lo, hi,
                                                                               u0, u1, mg.bands);
    if (mg.tiles > 1)
        k_mon_scatter_cols<T, SX><<<dim3(bxc, mg.tiles - 1), dim3(kBlock), 0, s>>>(x, Px, sc, N, u0,
                                                                                   u1);
}

// The damping pass on any level: a whole grid of N = 2^k + 1 points per side, k >= 2 (rows
// [0, N), the interior updated), in T, wherever it lies.  The decomposition is mon_grid's, a
// function of N alone, so the partial sums -- and the norm -- are those of the monitor of a
// context of that N.  At the small end (N = 5, 9: npairs = 2, 4) one workgroup runs: wave 0
// holds every column, waves 1 .. 3 have nw = 0 -- their row loads are buffer loads of zero
// records (nothing is read, whatever the address), their edge-column loads are off (`on`,
// has_right) and they store nothing, but they march the band and meet every barrier.  N = 65 is
// two bands: the second holds row 64 alone, which is a boundary row (r >= u1): it is neither
// updated nor deferred, and k_mon_scatter_rows skips its slots; band 0 defers row 63 (a band
// lies below it) and the scatter writes it.
int damp_grid_blocks(int N)
{
    const MonGrid mg = mon_grid(N, 0, N);
    return mg.tiles * mg.bands;
}
size_t damp_grid_side_elems(int N) { return mon_side_elems(N, mon_grid(N, 0, N)); }

template <class T>
void launch_damp_grid(T *x, long long Px, const T *f, long long Pf, int N, double ih, double h,
                      double omega, const double *gfx, const double *gsy, double *partials, T *side,
                      double *sums, hipStream_t s)
{
    const MonGrid mg = mon_grid(N, 0, N);
    MonArgsT<T, T, T> a{};
    a.x = a.xw = x;
    a.Px = Px;
    a.f = f;
    a.Pf = Pf;
    a.gfx = gfx;
    a.gsy = gsy;
    a.partials = partials;
    a.ih = (T)ih;
    a.N = N;
    a.lo = 0;
    a.hi = N;
    a.u0 = 1;
    a.u1 = N - 1;
    a.sr = side;
    a.sc = side + (size_t)2 * mg.bands * N;
    // omega * 0.25 * (h * h) in double, left to right, then the element type
    a.w = (T)(omega * 0.25 * (h * h));
    const dim3 g(mg.tiles, mg.bands);
    if (gfx != nullptr) k_monitor<T, T, T, kMonDamp | kMonRes | kMonGen><<<g, dim3(kBlock), 0, s>>>(a);
    else k_monitor<T, T, T, kMonDamp | kMonRes><<<g, dim3(kBlock), 0, s>>>(a);
    mon_scatter<T, T>(x, Px, a.sr, a.sc, N, 0, N, 1, N - 1, mg, s);
    if (sums != nullptr)
        k_mon_reduce<<<dim3(1), dim3(kBlock), 0, s>>>(partials, mg.tiles * mg.bands, sums);
}
template void launch_damp_grid<double>(double *, long long, const double *, long long, int, double,
                                       double, double, const double *, const double *, double *,
                                       double *, double *, hipStream_t);
template void launch_damp_grid<float>(float *, long long, const float *, long long, int, double,
                                      double, double, const double *, const double *, double *,
                                      float *, double *, hipStream_t);

// k_mon_reduce on np workgroups' partials, for the passes that write the monitor's partial sums
// on the monitor's decomposition (k_defect, pgmg_mixed.hip)
void launch_mon_reduce(const double *partials, int np, double *out, hipStream_t s)
{
    k_mon_reduce<<<dim3(1), dim3(kBlock), 0, s>>>(partials, np, out);
}

// the context's partials (np workgroups) and, for a damping pass, its side buffer (side bytes)
int mon_reserve(pgmg_ctx *c, int np, size_t side)
{
    if (side > c->mon_side_bytes) {
        if (c->mon_side) HIPC(hipFree(c->mon_side));
        c->mon_side = nullptr;
        c->mon_side_bytes = 0;
        if (hipMalloc(&c->mon_side, side) != hipSuccess)
            return set_err(PGMG_ERR_NOMEM, "damping pass side buffer");
        c->mon_side_bytes = side;
    }
    if (np > c->mon_cap) {
        if (c->mon_buf) HIPC(hipFree(c->mon_buf));
        c->mon_buf = nullptr;
        c->mon_cap = 0;
        if (hipMalloc((void **)&c->mon_buf, sizeof(double) * 3 * ((size_t)np + 1)) != hipSuccess)
            return set_err(PGMG_ERR_NOMEM, "monitor partials");
        c->mon_cap = np;
    }
    return PGMG_OK;
}

// One damping pass on a level of the FMG pyramid (pgmg_fmg_damped): u and f the level's grids
// as they lie now, L its geometry; gen: level 0's analytic f regenerated.  No norm: the
// reduction is skipped, nothing is copied and nothing waits.  The side buffer and the partials
// grow to the largest level asked for (the climb asks for level 0 first, fmg_damp_reserve).
int fmg_damp_reserve(pgmg_ctx *c, int N)
{
    return mon_reserve(c, damp_grid_blocks(N), damp_grid_side_elems(N) * (c->fp32 ? 4 : 8));
}
template <class T>
static int fmg_damp_level_t(pgmg_ctx *c, const Grid &u, const Grid &f, const Level &L, double omega,
                            bool gen)
{
    PGMG_TRY(mon_reserve(c, damp_grid_blocks(L.N), damp_grid_side_elems(L.N) * sizeof(T)));
    // every row and column the pass reads or writes lies inside the level's grids
    PGMG_TRY(check_span(G<T>(u), L.P, (int)sizeof(T), 0, L.N - 1, 0, L.N - 1, "damping pass u"));
    if (!gen) PGMG_TRY(check_span(G<T>(f), L.P, (int)sizeof(T), 0, L.N - 1, 0, L.N - 1, "damping pass f"));
    launch_damp_grid<T>(G<T>(u), L.P, G<T>(f), L.P, L.N, L.ih, L.h, omega, gen ? c->rgfx : nullptr,
                        gen ? c->rgsy : nullptr, c->mon_buf, static_cast<T *>(c->mon_side), nullptr,
                        c->s);
    return PGMG_OK;
}
int fmg_damp_level(pgmg_ctx *c, const Grid &u, const Grid &f, const Level &L, double omega,
                   bool gen)
{
    return c->fp32 ? fmg_damp_level_t<float>(c, u, f, L, omega, gen)
                   : fmg_damp_level_t<double>(c, u, f, L, omega, gen);
}
int damp_omega_check(double omega, const char *who)
{
    if (!std::isfinite(omega) || omega <= 0.0 || omega > 1.0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": omega must be in (0, 1]");
    return PGMG_OK;
}

// Enqueue the pass and the reduction of its partials: the three totals land in c->mon_buf +
// 3 * c->mon_cap.  phi and f are read where they lie: the level-0 grids, or the caller's arrays
// of a device-bound problem (pitch N, double).  omega > 0: the damping pass (what includes the
// residual), which writes phi there too, and the scatter of its deferred outputs.
template <class T>
static int mon_enqueue(pgmg_ctx *c, unsigned what, double omega = 0.0)
{
    const Level &L = c->lv[0];
    const MonGrid mg = mon_grid(L.N, L.lo, L.hi);
    const int np = mg.tiles * mg.bands;
    const bool damp = omega > 0.0;
    PGMG_TRY(mon_reserve(c, np, damp ? mon_side_elems(L.N, mg) * sizeof(T) : 0));
    const bool res = (what & kMonRes) != 0;
    const bool gen = res && c->ext_f == nullptr && c->gen_rhs;
    const unsigned mode = what | (gen ? kMonGen : 0u) | (damp ? kMonDamp : 0u);
    const dim3 g(mg.tiles, mg.bands);
    T *const sr = static_cast<T *>(c->mon_side), *const sc = sr + (size_t)2 * mg.bands * L.N;
    double *out = c->mon_buf + 3 * (size_t)c->mon_cap;
    auto fill = [&](auto &a) {
        a.gfx = c->gfx;
        a.gsy = c->gsy;
        a.sx = c->mon_sx;
        a.sy = c->mon_sy;
        a.partials = c->mon_buf;
        a.ih = (T)L.ih;
        a.N = L.N;
        a.lo = L.lo;
        a.hi = L.hi;
        a.u0 = L.u0;
        a.u1 = L.u1;
        a.sr = sr;
        a.sc = sc;
        // omega * 0.25 * (h0 * h0) in double, left to right, then the element type
        a.w = (T)(omega * 0.25 * (L.h * L.h));
    };
    auto scatter = [&](auto *x, long long Px) {
        using SX = std::remove_pointer_t<decltype(x)>;
        mon_scatter<T, SX>(x, Px, sr, sc, L.N, L.lo, L.hi, L.u0, L.u1, mg, c->s);
    };
    if (c->ext_phi == nullptr) {
        MonArgsT<T, T, T> a{};
        a.x = a.xw = G<T>(L.A);
        a.Px = L.P;
        a.f = G<T>(L.F);
        a.Pf = L.P;
        fill(a);
        mon_launch_mode(a, mode, g, c->s);
        if (damp) scatter(a.xw, a.Px);
    } else if (c->ext_f != nullptr) {
        MonArgsT<T, double, double> a{};
        a.x = a.xw = c->ext_phi;
        a.Px = L.N;
        a.f = c->ext_f;
        a.Pf = L.N;
        fill(a);
        mon_launch_mode(a, mode, g, c->s);
        if (damp) scatter(a.xw, a.Px);
    } else {   // the analytic f: regenerated, or the context's stored copy
        MonArgsT<T, double, T> a{};
        a.x = a.xw = c->ext_phi;
        a.Px = L.N;
        a.f = G<T>(L.F);
        a.Pf = L.P;
        fill(a);
        mon_launch_mode(a, mode, g, c->s);
        if (damp) scatter(a.xw, a.Px);
    }
    k_mon_reduce<<<dim3(1), dim3(kBlock), 0, c->s>>>(c->mon_buf, np, out);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

static int mon_check(pgmg_ctx *c, unsigned what)
{
    if (what == 0 || (what & ~(kMonRes | kMonErr))) return set_err(PGMG_ERR_ARG, "bad monitor bits");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (!c->lv[0].on_this_rank) return set_err(PGMG_ERR_STATE, "level 0 not on this rank");
    if ((what & kMonErr) && !c->analytic)
        return set_err(PGMG_ERR_STATE, "PGMG_MON_ERROR needs the analytic problem (f = NULL): the "
                                       "exact solution of a caller's f is not known");
    return PGMG_OK;
}

// omega of the damping entries, and what they cannot run on
static int damp_check(pgmg_ctx *c, double omega, const char *who)
{
    PGMG_TRY(damp_omega_check(omega, who));
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, std::string(who) + ": one GPU only (world 1); row strips "
                                                          "are not supported");
    return PGMG_OK;
}

// the three sums of the current iterate on the host (synchronous; collective on row strips).
// omega > 0 (one GPU): the damping pass -- the sums are the iterate's of before its update; phi
// changes, so the carry goes (the speculation history and the statistics stay)
static int mon_sums(pgmg_ctx *c, unsigned what, double sums[3], double omega = 0.0)
{
    const Level &L = c->lv[0];
    if (omega > 0.0) c->carry = false;
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    if (c->comm && (what & kMonRes)) PGMG_TRY(c->comm->halo(L.A, L, 1, c->s));
    PGMG_TRY(c->fp32 ? mon_enqueue<float>(c, what, omega) : mon_enqueue<double>(c, what, omega));
    double *out = c->mon_buf + 3 * (size_t)c->mon_cap;
    if (c->comm) PGMG_TRY(c->comm->allreduce_sum(out, 3, c->s));
    HIPC(hipMemcpyAsync(sums, out, 3 * sizeof(double), hipMemcpyDeviceToHost, c->s));
    PGMG_TRY(stream_wait(c));
    return PGMG_OK;
}

static int mon_run(pgmg_ctx *c, unsigned what, pgmg_monitor_out *o, double omega = 0.0)
{
    double s[3] = {0.0, 0.0, 0.0};
    PGMG_TRY(mon_sums(c, what, s, omega));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    o->res_norm = (what & kMonRes) ? std::sqrt(s[0]) : nan;
    o->err_norm = (what & kMonErr) ? std::sqrt(s[1]) : nan;
    o->exact_norm = (what & kMonErr) ? std::sqrt(s[2]) : nan;
    o->rel_error = (what & kMonErr) ? std::sqrt(s[1]) / std::sqrt(s[2]) : nan;   // orc_rel_error's form
    return PGMG_OK;
}

// algorithmic HBM bytes of one monitor pass; the damping pass writes one element per interior
// point more
static double mon_bytes(const pgmg_ctx *c, unsigned what, bool damp)
{
    const Level &L = c->lv[0];
    const bool stored = (what & kMonRes) && !(c->ext_f == nullptr && c->gen_rhs);
    const double xb = c->ext_phi ? 8.0 : L.es, fb = c->ext_f ? 8.0 : L.es;
    const double interior = (double)(L.N - 2) * (L.N - 2);
    return xb * (double)L.N * L.N + (stored ? fb * interior : 0.0) + (damp ? xb * interior : 0.0);
}

// `reps` passes between two events after two warm ones: mean device ms per pass
static int mon_time(pgmg_ctx *c, unsigned what, double omega, int reps, double *ms)
{
    auto run = [&]() {
        return c->fp32 ? mon_enqueue<float>(c, what, omega) : mon_enqueue<double>(c, what, omega);
    };
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    for (int k = 0; k < 2; ++k) PGMG_TRY(run());
    HIPC(hipEventRecord(c->ev0, c->s));
    for (int k = 0; k < reps; ++k) PGMG_TRY(run());
    HIPC(hipEventRecord(c->ev1, c->s));
    HIPC(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = f / reps;
    return PGMG_OK;
}

// pgmg_solve's loop; omega > 0: every check made by the damping pass (pgmg_solve_damped)
static int solve_loop(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, pgmg_solve_info *info)
{
    const unsigned what = o->monitor | PGMG_MON_RESIDUAL;
    const auto t0 = std::chrono::steady_clock::now();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    c->solve_hist.clear();
    *info = pgmg_solve_info{};
    info->rel_error = nan;
    StopState st;
    int cycles = 0;
    for (;;) {
        pgmg_monitor_out m{};
        PGMG_TRY(mon_run(c, what, &m, omega));
        c->solve_hist.push_back({cycles, m.res_norm, m.rel_error});
        int next = 0;
        const int reason = stop_check(*o, st, cycles, m.res_norm, &next);
        info->cycles = cycles;
        info->checks = st.checks;
        info->res0 = st.r0;
        info->res = m.res_norm;
        info->rel_error = m.rel_error;
        if (reason) {
            info->reason = reason;
            break;
        }
        PGMG_TRY(o->cycle == PGMG_CYCLE_V   ? pgmg_vcycle(c, next)
                 : o->cycle == PGMG_CYCLE_W ? pgmg_wcycle(c, next)
                                            : pgmg_fcycle(c, next));
        cycles += next;
    }
    info->elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_monitor(pgmg_ctx *c, unsigned what, pgmg_monitor_out *out)
{
    if (!c || !out) return set_err(PGMG_ERR_ARG, "null argument");
    PGMG_TRY(mon_check(c, what));
    return mon_run(c, what, out);
}

int pgmg_monitor_time(pgmg_ctx *c, unsigned what, int reps, double *ms, double *bytes)
{
    if (!c || !ms || reps <= 0) return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(mon_check(c, what));
    if (c->comm) return set_err(PGMG_ERR_STATE, "pgmg_monitor_time: one GPU only (world 1)");
    PGMG_TRY(mon_time(c, what, 0.0, reps, ms));
    if (bytes) *bytes = mon_bytes(c, what, false);
    return PGMG_OK;
}

int pgmg_solve_opts_default(pgmg_solve_opts *o)
{
    if (!o) return set_err(PGMG_ERR_ARG, "null opts");
    *o = pgmg_solve_opts{};
    o->cycle = PGMG_CYCLE_V;
    o->max_cycles = 30;
    o->check_every = 1;
    o->rtol = 1e-3;
    o->atol = 0.0;
    o->stall_ratio = 0.0;
    o->stall_checks = 2;
    o->monitor = PGMG_MON_RESIDUAL;
    return PGMG_OK;
}

int pgmg_solve(pgmg_ctx *c, const pgmg_solve_opts *o, pgmg_solve_info *info)
{
    if (!c || !o || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, std::string("pgmg_solve: ") + bad);
    PGMG_TRY(mon_check(c, o->monitor | PGMG_MON_RESIDUAL));
    return solve_loop(c, o, 0.0, info);
}

int pgmg_damp(pgmg_ctx *c, double omega, double *res_norm)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    PGMG_TRY(damp_check(c, omega, "pgmg_damp"));
    PGMG_TRY(mon_check(c, PGMG_MON_RESIDUAL));
    pgmg_monitor_out m{};
    PGMG_TRY(mon_run(c, PGMG_MON_RESIDUAL, &m, omega));
    if (res_norm) *res_norm = m.res_norm;
    return PGMG_OK;
}

int pgmg_solve_damped(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, pgmg_solve_info *info)
{
    if (!c || !o || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o))
        return set_err(PGMG_ERR_ARG, std::string("pgmg_solve_damped: ") + bad);
    PGMG_TRY(damp_check(c, omega, "pgmg_solve_damped"));
    PGMG_TRY(mon_check(c, o->monitor | PGMG_MON_RESIDUAL));
    return solve_loop(c, o, omega, info);
}

int pgmg_damp_time(pgmg_ctx *c, double omega, int reps, double *ms, double *bytes)
{
    if (!c || !ms || reps <= 0) return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(damp_check(c, omega, "pgmg_damp_time"));
    PGMG_TRY(mon_check(c, PGMG_MON_RESIDUAL));
    c->carry = false;   // phi is changed
    PGMG_TRY(mon_time(c, PGMG_MON_RESIDUAL, omega, reps, ms));
    if (bytes) *bytes = mon_bytes(c, PGMG_MON_RESIDUAL, true);
    return PGMG_OK;
}

int pgmg_history(pgmg_ctx *c, int cap, int *cycle, double *res, double *rel_error, int *n)
{
    if (!c || !n || cap < 0) return set_err(PGMG_ERR_ARG, "bad argument");
    const int have = (int)c->solve_hist.size();
    *n = have;
    for (int i = 0; i < have && i < cap; ++i) {
        if (cycle) cycle[i] = c->solve_hist[i].cycle;
        if (res) res[i] = c->solve_hist[i].res;
        if (rel_error) rel_error[i] = c->solve_hist[i].rel_error;
    }
    return PGMG_OK;
}

}  // extern "C"
