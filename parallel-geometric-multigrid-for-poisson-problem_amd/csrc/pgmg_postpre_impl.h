// pgmg_postpre_impl.h — k_postpre_lds: the finest level between two consecutive cycles of one
// call as one HBM pass, and its smooth(3) form for the F-cycle.
//
//   xe = phi + P ec -> x1 -> x2 (post-smooth of cycle k, never stored)
//   -> x3 -> x4 (pre-smooth of cycle k+1, stored) -> r(x4) -> rc (cycle k+1)
// Checks: ||r(x1)|| (post) and ||r(x3)|| (pre), both speculative (partials1/2; decided by
// k_postpre_decide, pgmg_fixup.hip).
// Read phi, f, ec; write x4, rc: 24 B per fine point + 16 B per coarse point,
// replacing k_post + k_pre (48 + 16).  Wave tile: 116 owned columns of 128
// (validity shrinks 6 columns per side through 6 stencil levels + restriction;
// pgmg_fused_geom.h).
// Stage lags behind the loaded row i: xe i, x1 i-1, x2 i-2, x3 i-3, x4 i-4,
// r(x4) i-5, rc when i-5 = 2jc+1.
// The rows are staged once per block in LDS ("k_postpre_lds" below); the forms of the pass
// (row strips, carry, recompute, FAST, smooth(3)) are compile-time options of one body.
//
// The whole pass, kernels and launchers, as templates on the element type; compiled once per
// type, by pgmg_postpre_f64.hip (20 kernel instantiations) and pgmg_postpre_f32.hip (12): one
// translation unit for both was by far the longest compile of the build
// (profiles/fused_split/build_times.txt).  The sampled-check forms of the cross-cycle pass are
// compiled by pgmg_postpre_f64s.hip (16) and pgmg_postpre_f32s.hip (8), see launch_pp_sampled.
#pragma once
#include <algorithm>
#include <type_traits>

#include "pgmg.h"
#include "pgmg_fused_dev.h"

namespace pgmg {

// Horizontal neighbours of a row's column pair (left of c, right of c+1), shared by the
// stages that use the same centre row (a Jacobi sweep and a residual of the same iterate).
template <class T> struct Nbr {
    T l, r;
};
template <class T> __device__ __forceinline__ Nbr<T> nbr(V2<T> ce)
{
    return Nbr<T>{dpp_shr(ce.y), dpp_shl(ce.x)};
}
template <class T, bool EDGE>
__device__ __forceinline__ V2<T> jsn(V2<T> up, V2<T> ce, V2<T> dn, Nbr<T> n, V2<T> f, T hh,
                                       const Cols &k, bool brow)
{
    V2<T> o;
    if constexpr (sizeof(T) == 4 && PGMG_F32_PK) {   // packed (as jstage)
        const pf2 L = {n.l, ce.x}, R = {ce.y, n.r};
        o = unpk(0.25f * (((((hh * pk(f)) + L) + R) + pk(up)) + pk(dn)));
    } else {
        o.x = T(0.25) * ((hh * f.x) + n.l + ce.y + up.x + dn.x);
        o.y = T(0.25) * ((hh * f.y) + ce.x + n.r + up.y + dn.y);
    }
    if constexpr (EDGE) {
        if (brow || k.bx) o.x = ce.x;
        if (brow || k.by) o.y = ce.y;
    }
    return o;
}
// jsn with the RHS term hh*f precomputed (hf): the same IEEE product, formed once per row
// instead of once per sweep that reads the row
template <class T, bool EDGE>
__device__ __forceinline__ V2<T> jsh(V2<T> up, V2<T> ce, V2<T> dn, Nbr<T> n, V2<T> hf,
                                       const Cols &k, bool brow)
{
    V2<T> o;
    if constexpr (sizeof(T) == 4 && PGMG_F32_PK) {   // packed: L = (l, c), R = (c+1, r), same order per element
        const pf2 L = {n.l, ce.x}, R = {ce.y, n.r};
        o = unpk(0.25f * ((((pk(hf) + L) + R) + pk(up)) + pk(dn)));
    } else {
        o.x = T(0.25) * (hf.x + n.l + ce.y + up.x + dn.x);
        o.y = T(0.25) * (hf.y + ce.x + n.r + up.y + dn.y);
    }
    if constexpr (EDGE) {
        if (brow || k.bx) o.x = ce.x;
        if (brow || k.by) o.y = ce.y;
    }
    return o;
}
// FAST mode (OPT & 16): the neighbour sum of a centre row, S = (l + r) + (u + d), shared by
// its Jacobi stage, 0.25 * (hh*f + S), and its residual, f - ih * (4x - S) as two FMAs
template <class T>
__device__ __forceinline__ V2<T> nsum(V2<T> up, V2<T> ce, V2<T> dn, Nbr<T> n)
{
    V2<T> sm;
    sm.x = (n.l + ce.y) + (up.x + dn.x);
    sm.y = (ce.x + n.r) + (up.y + dn.y);
    return sm;
}
template <class T, bool EDGE>
__device__ __forceinline__ V2<T> jsum(V2<T> sm, V2<T> ce, V2<T> hf, const Cols &k, bool brow)
{
    V2<T> o;
    o.x = T(0.25) * (hf.x + sm.x);
    o.y = T(0.25) * (hf.y + sm.y);
    if constexpr (EDGE) {
        if (brow || k.bx) o.x = ce.x;
        if (brow || k.by) o.y = ce.y;
    }
    return o;
}
template <class T>
__device__ __forceinline__ V2<T> rsum(V2<T> sm, V2<T> ce, V2<T> f, T ih)
{
    V2<T> o;
    o.x = __builtin_fma(-ih, __builtin_fma(T(4), ce.x, -sm.x), f.x);
    o.y = __builtin_fma(-ih, __builtin_fma(T(4), ce.y, -sm.y), f.y);
    return o;
}
template <class T>
__device__ __forceinline__ V2<T> rsn(V2<T> up, V2<T> ce, V2<T> dn, Nbr<T> n, V2<T> f, T ih)
{
    V2<T> o;
    if constexpr (sizeof(T) == 4 && PGMG_F32_PK) {   // packed (as jsh)
        const pf2 L = {n.l, ce.x}, R = {ce.y, n.r};
        o = unpk(pk(f) - ih * ((((4.0f * pk(ce) - L) - R) - pk(up)) - pk(dn)));
    } else {
        o.x = f.x - ih * (T(4) * ce.x - n.l - ce.y - up.x - dn.x);
        o.y = f.y - ih * (T(4) * ce.y - ce.x - n.r - up.y - dn.y);
    }
    return o;
}

// ---------------------------------------------------------------------------
// k_postpre_lds (default): the same pass, but the rows of phi, f and ec are staged
// once per block in LDS.  A block's 4 wave tiles overlap by 12 columns each; loading
// every tile from HBM re-reads 14 of each 128 columns (12 %).  Here the block's
// 256 lanes load its 468-column window (4 x 114 owned + 2 x 6 margin) exactly once
// per row (one 16-byte load per lane), and each wave reads its 128-column window
// (and the coarse correction, with its right neighbour) from LDS.  Double-buffered
// by row pairs: while the waves compute pair g from one slot, the loads of pair g+2
// are in flight in registers and pair g+1 sits in the other slot; one barrier per
// row pair.  Coarse rows live in a ring of 3 (pair g reads coarse rows g and g+1).
// ---------------------------------------------------------------------------
template <int OPT> constexpr int pp_stride() { return (OPT & 256) ? kPPStrideRC : kPPStride; }
template <int OPT> constexpr int pp_margin() { return (OPT & 256) ? kPPMarginRC : kPPMargin; }
constexpr int kPPLdsRow = kPPWaves * kPPStride + 2 * kPPMargin + 4;          // doubles per row
constexpr int kPPLdsCoarse = kPPWaves * (kPPStride / 2) + kPPMargin + 8;     // per coarse row
static_assert(kPPWaves * kPPStrideRC + 2 * kPPMarginRC + 4 <= kPPLdsRow &&
                  kPPWaves * (kPPStrideRC / 2) + kPPMarginRC + 8 <= kPPLdsCoarse,
              "the recompute form's windows fit the LDS rows");
// fp32 (r05): the rows are staged from 16-byte loads of FOUR columns per lane (8-byte lane
// loads stream at 0.54-0.70x the 16-byte rate, MI355X_MICROARCH.md), starting two columns
// left of the window (column L0 - 2 is 16-byte aligned: column 1 of every row sits on a
// 128-byte boundary), so an fp32 LDS row carries a 2-element shift and 4 more elements; the
// coarse rows likewise from 16-byte loads at cc0 (aligned), rows padded to whole 16 bytes.
// Compile-time A/B knobs of the fp32 form (scripts/build_variant.sh): quad row loads, quad
// coarse loads, quad x4 stores, register sets of loads in flight.  Measured (r05,
// scripts/pp_ab.py --dtype f32, profiles/r05_fp32/pp_f32.jsonl, 3 interleaved rounds at 16385):
// k_postpre_lds<float> 0.636-0.651 ms as built before, 0.644-0.648 with every knob off,
// 0.675-0.687 with quad loads (2 waves of 4 do all the loading, ds_write_b128), 0.647-0.649
// with quad stores only -- the knobs stay off; the pass's cost for fp32 is its per-lane work
// on 2 columns, not the load width.
#ifndef PGMG_F32_QLOAD
#define PGMG_F32_QLOAD 0
#endif
#ifndef PGMG_F32_QCOARSE
#define PGMG_F32_QCOARSE 0
#endif
#ifndef PGMG_F32_QSTORE
#define PGMG_F32_QSTORE 0
#endif
#ifndef PGMG_F32_DEPTH
#define PGMG_F32_DEPTH 3
#endif
template <class T> constexpr bool pp_ql() { return sizeof(T) == 4 && PGMG_F32_QLOAD; }
template <class T> constexpr bool pp_qc() { return sizeof(T) == 4 && PGMG_F32_QCOARSE; }
template <class T> constexpr bool pp_qs() { return sizeof(T) == 4 && PGMG_F32_QSTORE; }
template <class T> constexpr int pp_sh() { return pp_ql<T>() ? 2 : 0; }
template <class T> constexpr int pp_lds_row() { return kPPLdsRow + (pp_ql<T>() ? 4 : 0); }
template <class T> constexpr int pp_lds_coarse()
{
    return pp_qc<T>() ? (kPPLdsCoarse + 3) / 4 * 4 : kPPLdsCoarse;
}
// the register type of one row's staging load: a column pair (fp64), a column quad (fp32)
template <class T> using PPV = typename std::conditional<pp_ql<T>(), float4, V2<T>>::type;
template <class T> using PPC = typename std::conditional<pp_qc<T>(), float4, V2<T>>::type;

// R2 (row strips): also sum r(x2)^2 into partials3.  When the post check fires the
// pre-smooth restarts from x1 and its first check is ||r(J(x1))|| = ||r(x2)||; having it
// here lets one allreduce of three sums decide every rare path.
// GENF (the problem's f is the analytic RHS of compute_rhs): f is not streamed from HBM
// but regenerated per point as (T)(fx[i] * sy[j]) with fx[i] = factor*sin(p pi x_i / a)
// (per lane, in registers) and sy[j] = sin(q pi y_j / a) (per row, a scalar load) — the
// same IEEE operations as k_rhs, so the values are identical to the stored f.  One
// multiply per point replaces 8 bytes per point of the pass (28 -> 20 B/pt).
// OPT (compile-time, result-identical): 2 non-temporal x4 stores, 4 non-temporal rc
// stores, 64 the F-cycle's smooth(3) (no correction, no restriction), 128 the carry pass
// (the last pass of a call that hands the next call its pre-smooth: x2 -- the call's result --
// is stored INSTEAD of x4; the next call recomputes x4 from it), 256 the recompute form
// (the first pass of a call that took the carry: the input is the previous call's x2, whose
// pre-smooth -- two Jacobi stages, the carry pass's own expressions, bitwise its x4 -- runs in
// front of the correction; the pipeline's rows lag two more), 512 sampled checks.
// Sampled checks (OPT & 512; speculative calls on one GPU, pgmg_spec.hip): the two checks'
// residuals r(x1), r(x3) and their sums are compiled only for the first row of one step of the
// loop body each -- 1 row in 6 (depth 3, none in the remainder steps) or in 4 (depth 2): the
// band's first row and every 6th (4th) after it, so a band of any height sums a row -- with the full form's expressions and its in-band and ownership masks, into the same
// partial slots.  A sampled partial adds a subsequence of the full partial's non-negative terms
// in the same order, so it is a lower bound of it (rounding is monotonic): enough to prove that
// a check cannot fire, never to decide that it does (k_postpre_decide only sees full sums).
// Everything the pass stores is the full form's, bit for bit.  Not for R2 or OPT & 64.
template <int K> using BodyStep = std::integral_constant<int, K>;   // (postpre_lds_run's step)
// Logical block of the 2D grid (x: column block, y: band).
struct Blk {
    int x, y;
};

// Row pairs of loads in flight per wave (register sets).  3 also makes the guard-free loop
// body 6 rows, the period of the row windows (no window copies: 141 -> 129 VALU per row);
// the fp64 instantiations with more live state (streamed f, the strips' third sum, the
// F-cycle's four-sweep form, the recompute form) keep 2, which fits 256 VGPRs without spilling.
template <class T, bool R2, bool GENF, int OPT>
constexpr int pp_depth()
{
    return sizeof(T) == 4 ? PGMG_F32_DEPTH : ((GENF && !R2 && !(OPT & (64 | 32 | 256))) ? 3 : 2);
}
// (buf_row, the row-segment load of a lane's column pair: pgmg_internal.h)
template <class T, int NT>
__device__ __forceinline__ void buf_store_row(T *base, int bytes, int off, V2<T> v)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
    if constexpr (sizeof(T) == 8) {
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, off, 0, NT ? 2 : 0);
    } else {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, off, 0, NT ? 2 : 0);
    }
}
template <class T>
__device__ __forceinline__ void buf_store_one(T *base, int bytes, int off, T v)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
    if constexpr (sizeof(T) == 8) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, off, 0, 0);
    } else {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, 0);
    }
}
// fp32: lane t's 16-byte column quad of a row segment of n quads starting at `base`
__device__ __forceinline__ float4 buf_quad(const float *base, int n, int t)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(base), (short)0, n * 16, 0x00020000);
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, t * 16, 0, 0));
}
template <int NT>
__device__ __forceinline__ void buf_store_quad(float *base, int bytes, int off, float4 v)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, off, 0, NT ? 2 : 0);
}
template <class T>
__device__ __forceinline__ T buf_one(const T *base, int n, int t)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T *>(base), (short)0, n * (int)sizeof(T), 0x00020000);
    if constexpr (sizeof(T) == 8)
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, t * 8, 0, 0));
    else
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, t * 4, 0, 0));
}

// The body of k_postpre_lds for one block.  EDGE = false: no row of the block's band and
// no column of this wave is a boundary, so the Jacobi stages carry no passthrough selects.
template <class T, bool R2, bool GENF, bool EDGE, int OPT>
__device__ __forceinline__ void postpre_lds_run(const PostPreArgsT<T> &a, const Cols &k,
                                                double *red, T (&sx)[2][kPPR][pp_lds_row<T>()],
                                                T (&sf)[2][kPPR][GENF ? 1 : pp_lds_row<T>()],
                                                T (&se)[3][pp_lds_coarse<T>()], const Blk bk)
{
    constexpr bool Q = pp_ql<T>();   // fp32: 16-byte column quads (above)
    constexpr bool QC = pp_qc<T>(), QS = pp_qs<T>();
    constexpr int SH = pp_sh<T>();
    constexpr int R = kPPR;
    constexpr bool RC = (OPT & 256) != 0;           // the recompute form
    constexpr bool CARRY = (OPT & 128) != 0;        // the carry pass
    constexpr int ST = pp_stride<OPT>(), MG = pp_margin<OPT>();
    constexpr int LAG = RC ? 2 : 0;                 // rows the correction lags the input
    constexpr bool SAMPLED = (OPT & 512) != 0;      // sampled checks
    static_assert(!SAMPLED || (!R2 && !(OPT & 64)), "sampled checks: the cross-cycle pass, one GPU");
    const int N = a.N, Nc = a.Nc;
    const long long P = a.P, Pc = a.Pc;
    const int jcb = a.jc0 + bk.y * a.rows_per_block;
    const int jce = min(jcb + a.rows_per_block, a.jc1);
    const int olo = max(2 * jcb, a.row_lo), ohi = min(2 * jce, a.row_hi);
    const int clo = max(jcb, max(1, a.rc_lo)), chi = min(jce, min(N / 2, a.rc_hi));
    if (bk.x == 0 && bk.y == 0 && threadIdx.x == 0 && a.stats != nullptr)
        atomicAdd(&a.stats[0], (unsigned long long)(4 + a.sw_adj));
    ProlongCols pc;
    pc.ic = (k.c - 1) >> 1;
    pc.vx = k.c >= 3 && k.c <= N - 2;
    pc.vy = k.c + 1 >= 2 && k.c + 1 <= N - 3;
    const T hh = a.hh, ih = a.ih;
    const V2<T> z = zero2<T>();

    // loader geometry: the block window starts at column L0 (odd: 16-byte aligned pairs)
    const int wpb = blockDim.x >> 6;
    const int t = threadIdx.x;
    const int L0 = ST * wpb * bk.x + 1 - MG;
    const int npairs = (ST * wpb + 2 * MG) / 2;
    const int cc0 = (L0 - 1) >> 1;                               // first coarse column
    const int ncc = (ST / 2) * wpb + MG + 2;
    // OPT & 64 (F-cycle smooth(3)): no coarse correction, no restriction
    // Row loads through buffer descriptors (one per row, built from wave-uniform values):
    // VMEM-only loads whose out-of-range lanes (past the window or the grid's last column)
    // read 0 from the descriptor's range check.  A `ldr ? load : 0` select compiles to a
    // FLAT load, which also counts on lgkmcnt, so the LDS wait before every barrier drained
    // the row pairs prefetched for later steps.
    // lanes that load (columns >= N never matter)
    const int nvx = max(0, min(npairs, (N - 1 - L0) / 2 + 1));
    const int nve = (OPT & 64) ? 0 : max(0, min(ncc, Nc - cc0));
    // stores: x4 row segment of the block window (lanes that own their pair), rc (lanes
    // owning a coarse column <= Nc-2); anything else gets an out-of-range offset
    constexpr int kOOB = 1 << 30;
    const int xbytes = (2 * npairs + 8) * (int)sizeof(T);
    const int xoff = k.own ? (k.c - L0) * (int)sizeof(T) : kOOB;
    const int cbytes = (ncc + 8) * (int)sizeof(T);
    const int coff = (k.own && ((k.c + 1) >> 1) <= Nc - 2) ? (((k.c + 1) >> 1) - cc0) * (int)sizeof(T) : kOOB;
    // GENF: this lane's columns of fx (tables padded: valid for columns/rows -8 ..)
    const double fxa = GENF ? a.gfx[k.c] : 0.0, fxb = GENF ? a.gfx[k.c + 1] : 0.0;
    // land them before the row loop: a load still in flight at the loop entry makes the
    // loop's first use of fxa wait for every outstanding load (vmcnt(0)) in every iteration
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    // this wave's window in the LDS rows
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int xo = ST * w + 2 * lane;
    const int co = (ST / 2) * w + lane;
    // fp32 quads: the window's 2 * npairs columns from L0 - 2 (nq4 quads; nvq of them inside
    // the loaded range, the rest read 0); coarse: ncc columns from cc0 (ncq quads, nveq valid).
    // A quad past the old pair/element range loads columns past the grid's last one or the
    // window: they reach only lanes that own nothing (the margins), as before.
    const int nq4 = (2 * npairs + 2 + 3) / 4, nvq = (2 * nvx + 2 + 3) / 4;
    const int ncq = (ncc + 3) / 4, nveq = (nve + 3) / 4;
    // fp32 x4 stores: odd lane l (16-byte aligned column) stores its pair and lane l+1's as
    // one quad when both own theirs; an owning odd lane without an owning partner (the grid's
    // right edge) stores its pair alone
    const bool own_next = lane + 1 < MG / 2 + ST / 2 && k.c + 2 <= N - 2;
    const int xoff16 = (QS && (lane & 1) && k.own && own_next) ? xoff : kOOB;
    const int xoff8 = QS ? (((lane & 1) && k.own && !own_next) ? xoff : kOOB) : xoff;

    V2<T> e0 = z, e1 = z, b0 = z, b1 = z, c0 = z, c1 = z, g0 = z, g1 = z, h0 = z, h1 = z,
            d0 = z, d1 = z;
    V2<T> f1 = z, f2 = z, f3 = z, f4 = z, f5 = z;  // f[i-1], f[i-2], ..., f[i-5]
    V2<T> q1 = z, q2 = z, q3 = z, q4 = z;          // hh * f[i-1], ..., hh * f[i-4]
    V2<T> f6 = z, f7 = z, q5 = z, q6 = z;          // RC: the windows two rows longer
    V2<T> p0 = z, p1 = z, a0 = z, a1 = z;          // RC: input rows i-2, i-1; stage-1 rows i-3, i-2
    double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    const int i_begin = 2 * jcb - 6 - LAG;
    // row pairs (uniform over the block): the input rows 2jcb-6-LAG .. 2jce+4+LAG
    const int ng = (2 * (jce - jcb) + 11 + 2 * LAG + R - 1) / R;
    // coarse row of the first pair (RC: the correction of pair gi's rows lags one pair)
    const int m0 = (i_begin >> 1) - (RC ? 1 : 0);
    auto ring = [](int m) { return (m + 3 * 4096) % 3; };  // m >= -3

    if (t < 2 * R * 4) {   // the 4 pad doubles past the window (read by spare lanes only)
        const int sl = t >> 3, q = (t >> 2) & 1, j = pp_lds_row<T>() - 4 + (t & 3);
        sx[sl][q][j] = T(0);
        if constexpr (!GENF) sf[sl][q][j] = T(0);
    }
    // D register sets: pair p's loads go to set p % D, issued D pairs ahead (D = 2: sets
    // A, B; D = 3: A, B, C)
    constexpr int D = pp_depth<T, R2, GENF, OPT>();
    static_assert(D == 2 || D == 3, "two or three register sets");
    using PV = PPV<T>;
    PV pxA[R], pfA[R], pxB[R], pfB[R], pxC[R], pfC[R];   // C unused (dead) when D = 2
    using PC = PPC<T>;
    const PC cz{};
    PC peA = cz, peB = cz, peC = cz;   // the pair's second coarse row (pairs: in .x)
    auto load_coarse = [&](int m) {
        if constexpr (QC) return buf_quad(reinterpret_cast<const float *>(a.ec) + (long long)m * Pc + cc0, nveq, t);
        else {
            PC v = cz;
            v.x = buf_one<T>(a.ec + (long long)m * Pc + cc0, nve, t);
            return v;
        }
    };
    auto store_coarse = [&](int m, PC v) {
        if constexpr (QC) {
            if (t < ncq) *reinterpret_cast<float4 *>(&se[ring(m)][4 * t]) = v;
        } else {
            if (t < ncc) se[ring(m)][t] = v.x;
        }
    };
    auto load_pair = [&](int p, PV (&px)[R], PV (&pf)[R], PC &pe) {
        #pragma unroll
        for (int q = 0; q < R; ++q) {
            const long long row = (long long)(i_begin + p * R + q) * P + L0;
            if constexpr (Q) {
                px[q] = buf_quad(reinterpret_cast<const float *>(a.phi) + row - SH, nvq, t);
                if constexpr (!GENF) pf[q] = buf_quad(reinterpret_cast<const float *>(a.f) + row - SH, nvq, t);
            } else {
                px[q] = buf_row<T, 0>(a.phi + row, nvx, t);
                if constexpr (!GENF) pf[q] = buf_row<T, 0>(a.f + row, nvx, t);
            }
        }
        pe = load_coarse(m0 + p + 1);   // 2nd coarse row
    };
    auto store_pair = [&](int p, const PV (&px)[R], const PV (&pf)[R], PC pe) {
        if (t < (Q ? nq4 : npairs)) {
            #pragma unroll
            for (int q = 0; q < R; ++q) {
                *reinterpret_cast<PV *>(&sx[p & 1][q][(Q ? 4 : 2) * t]) = px[q];
                if constexpr (!GENF) *reinterpret_cast<PV *>(&sf[p & 1][q][(Q ? 4 : 2) * t]) = pf[q];
            }
        }
        store_coarse(m0 + p + 1, pe);
    };
    // prologue: pair 0 (+ its first coarse row) into slot 0; pairs 1 .. D in flight
    load_pair(0, pxA, pfA, peA);
    store_coarse(m0, load_coarse(m0));
    store_pair(0, pxA, pfA, peA);
    if (ng > 1) load_pair(1, pxB, pfB, peB);
    if constexpr (D == 3) {
        if (ng > 2) load_pair(2, pxC, pfC, peC);
        if (ng > 3) load_pair(3, pxA, pfA, peA);
    } else {
        if (ng > 2) load_pair(2, pxA, pfA, peA);
    }
    __syncthreads();

    // pair gi: compute from slot gi & 1; pair gi+1 (set (gi+1) & 1) -> the other slot;
    // issue pair gi+3 into the set just freed; one barrier
    T wprev = T(0);   // dpp_shl(d2.x) of the previous restriction row (d0 starts as zero)
    // kb (compile time): the step's place in the loop body, -1 in the remainder steps.  Sampled
    // checks: the first row of body step SPOST carries the post check and that of step SPRE the
    // pre check -- the steps whose first row's check falls on the band's first row 2jcb (then
    // every 2D rows), so that a band of any height sums at least that row
    constexpr int SPOST = (4 + LAG) % D, SPRE = (5 + LAG) % D;
    auto step = [&](auto kb, int gi, PV (&px)[R], PV (&pf)[R], PC &pe) {
        // keep the scheduler inside one pair: interleaving the unrolled pairs only raises
        // the register pressure (the loads of a pair are issued two pairs ahead anyway)
        __builtin_amdgcn_sched_barrier(0);
        const int slot = gi & 1;
        // the other slot's previous readers passed the last barrier: stage pair gi+1 (loaded
        // D steps ago) first and reissue its register set for pair gi+1+D, so the loads in
        // flight are never younger than this step's stores (counted waits stay small)
        if (gi + 1 < ng) store_pair(gi + 1, px, pf, pe);
        if (gi + 1 + D < ng) load_pair(gi + 1 + D, px, pf, pe);
        const int i = i_begin + gi * R;
        const int m = m0 + gi;
        const T *E0 = se[ring(m)], *E1 = se[ring(m + 1)];
        const T cr0 = E0[co], crn0 = E0[co + 1], cr1 = E1[co], crn1 = E1[co + 1];
        #pragma unroll
        for (int s = 0; s < R; ++s) {
            const int ii = i + s;
            // (s is a constant of the unrolled body: the other rows' checks are not compiled)
            constexpr int KB = decltype(kb)::value;
            const bool chk1 = !SAMPLED || (KB == SPOST && s == 0);
            const bool chk3 = !SAMPLED || (KB == SPRE && s == 0);
            const V2<T> xr = ldv(&sx[slot][s][xo + SH]);
            // f[ii]: from LDS, or (GENF) generated once here and carried in the f window
            // (regenerating it at every use instead: fewer VGPRs, 8 more multiplies per
            // row, measured slower in r01)
            V2<T> f0 = z;
            if constexpr (!GENF) f0 = ldv(&sf[slot][s][xo + SH]);
            if constexpr (GENF) {
                const double sy = gsy_s(a.gsy, ii);
                f0 = mk2<T>((T)(fxa * sy), (T)(fxb * sy));
            }
            const V2<T> q0 = mk2<T>(hh * f0.x, hh * f0.y);
            constexpr bool FAST = (OPT & 16) != 0;
            // RC: the carry pass's pre-smooth of the input (its g / h stages, the same
            // expressions on the same values: bitwise its x4), row ii-2; then every stage below
            // runs on row L = ii - 2 with the f windows two rows further back
            V2<T> xin = xr;
            if constexpr (RC) {
                const V2<T> a2 = FAST ? jsum<T, EDGE>(nsum<T>(p0, p1, xr, nbr<T>(p1)), p1, q1, k, boundary_row(ii - 1, N))
                                      : jsh<T, EDGE>(p0, p1, xr, nbr<T>(p1), q1, k, boundary_row(ii - 1, N));
                xin = FAST ? jsum<T, EDGE>(nsum<T>(a0, a1, a2, nbr<T>(a1)), a1, q2, k, boundary_row(ii - 2, N))
                           : jsh<T, EDGE>(a0, a1, a2, nbr<T>(a1), q2, k, boundary_row(ii - 2, N));
                p0 = p1; p1 = xr;
                a0 = a1; a1 = a2;
            }
            const int L = ii - LAG;
            const V2<T> fq2 = RC ? f4 : f2, fq3 = RC ? f5 : f3, fq4 = RC ? f6 : f4, fq5 = RC ? f7 : f5;
            const V2<T> hq1 = RC ? q3 : q1, hq2 = RC ? q4 : q2, hq3 = RC ? q5 : q3, hq4 = RC ? q6 : q4;
            const V2<T> e2 = (OPT & 64) ? xin : add_prolong<T, EDGE>(xin, L, cr0, crn0, cr1, crn1, pc, Nc);
            // post-smooth sweep 1: x1 row ii-1
            const V2<T> b2 = FAST ? jsum<T, EDGE>(nsum<T>(e0, e1, e2, nbr<T>(e1)), e1, hq1, k, boundary_row(L - 1, N))
                                  : jsh<T, EDGE>(e0, e1, e2, nbr<T>(e1), hq1, k, boundary_row(L - 1, N));
            const Nbr<T> nb1 = nbr<T>(b1), nc1 = nbr<T>(c1), ng1 = nbr<T>(g1);
            // FAST: the neighbour sums of x1 row ii-2 and x3 row ii-4, each shared by a sweep
            // and a check
            const V2<T> sb = FAST ? nsum<T>(b0, b1, b2, nb1) : z;
            if (chk1) {   // post check: r(x1) on row ii-2
                const V2<T> r1 = FAST ? rsum<T>(sb, b1, fq2, ih) : rsn<T>(b0, b1, b2, nb1, fq2, ih);
                const int row = L - 2;
                if constexpr (chk_sel<T>()) {
                    acc1 = chk_acc<T>(acc1, r1, row >= olo && row < ohi && k.own, k.by);
                } else if (row >= olo && row < ohi && k.own) {
                    acc1 = sqacc(acc1, r1.x);
                    if (!k.by) acc1 = sqacc(acc1, r1.y);
                }
            }
            // post-smooth sweep 2: x2 row L-2 (= phi of cycle k+1)
            const V2<T> c2 = FAST ? jsum<T, EDGE>(sb, b1, hq2, k, boundary_row(L - 2, N))
                                  : jsh<T, EDGE>(b0, b1, b2, nb1, hq2, k, boundary_row(L - 2, N));
            if constexpr (CARRY) {   // the carry pass: x2 is the call's result (x4 is not stored)
                const int xb2 = (L - 2 >= olo && L - 2 < ohi) ? xbytes : 0;
                buf_store_row<T, (OPT & 2) ? 1 : 0>(a.x2 + (long long)(L - 2) * P + L0, xb2, xoff, c2);
            }
            if (R2) {   // r(x2) on row ii-3
                const V2<T> r2 = rsn<T>(c0, c1, c2, nc1, fq3, ih);
                const int row = L - 3;
                if constexpr (chk_sel<T>()) {
                    acc3 = chk_acc<T>(acc3, r2, row >= olo && row < ohi && k.own, k.by);
                } else if (row >= olo && row < ohi && k.own) {
                    acc3 = sqacc(acc3, r2.x);
                    if (!k.by) acc3 = sqacc(acc3, r2.y);
                }
            }
            // pre-smooth sweep 1: x3 row ii-3
            const V2<T> g2 = FAST ? jsum<T, EDGE>(nsum<T>(c0, c1, c2, nc1), c1, hq3, k, boundary_row(L - 3, N))
                                  : jsh<T, EDGE>(c0, c1, c2, nc1, hq3, k, boundary_row(L - 3, N));
            const V2<T> sgg = FAST ? nsum<T>(g0, g1, g2, ng1) : z;
            if (chk3) {   // pre check: r(x3) on row ii-4
                const V2<T> r3 = FAST ? rsum<T>(sgg, g1, fq4, ih) : rsn<T>(g0, g1, g2, ng1, fq4, ih);
                const int row = L - 4;
                if constexpr (chk_sel<T>()) {
                    acc2 = chk_acc<T>(acc2, r3, row >= olo && row < ohi && k.own, k.by);
                } else if (row >= olo && row < ohi && k.own) {
                    acc2 = sqacc(acc2, r3.x);
                    if (!k.by) acc2 = sqacc(acc2, r3.y);
                }
            }
            // pre-smooth sweep 2: x4 row ii-4 (stored)
            const V2<T> h2 = FAST ? jsum<T, EDGE>(sgg, g1, hq4, k, boundary_row(L - 4, N))
                                  : jsh<T, EDGE>(g0, g1, g2, ng1, hq4, k, boundary_row(L - 4, N));
            // branch-free: rows outside the band get a zero-record descriptor, lanes that do
            // not own their pair an out-of-range offset (every step issues the same memory
            // instructions, so the compiler can count its waits)
            if constexpr (!CARRY) {
                const int xb = (L - 4 >= olo && L - 4 < ohi) ? xbytes : 0;
                T *xrow = a.x4 + (long long)(L - 4) * P + L0;
                if constexpr (QS) {   // lane l+1's pair by DPP; odd lanes store the quad
                    const float4 v4 = make_float4(h2.x, h2.y, dpp_shl(h2.x), dpp_shl(h2.y));
                    buf_store_quad<(OPT & 2) ? 1 : 0>(reinterpret_cast<float *>(xrow), xb, xoff16, v4);
                    if constexpr (EDGE)
                        buf_store_row<T, (OPT & 2) ? 1 : 0>(xrow, xb, xoff8, h2);
                } else {
                    buf_store_row<T, (OPT & 2) ? 1 : 0>(xrow, xb, xoff8, h2);
                }
            }
            // r(x4) on row ii-5
            const V2<T> d2 = FAST ? rsum<T>(nsum<T>(h0, h1, h2, nbr<T>(h1)), h1, fq5, ih)
                                  : rsn<T>(h0, h1, h2, nbr<T>(h1), fq5, ih);
            // restriction: rows L-7, L-6, L-5 = 2jc-1, 2jc, 2jc+1 when L is even
            if (!(OPT & 64) && (s & 1) == 0) {
                const int jc = (L - 6) >> 1;
                const T m2 = dpp_shl(d1.x);
                const T u2 = wprev;               // = dpp_shl(d0.x): row ii-7 was d2 two rows ago
                const T w2 = dpp_shl(d2.x);
                wprev = w2;
                const T v = T(0.25) * d1.y + T(0.125) * (m2 + d1.x + d2.y + d0.y) +
                                 T(0.0625) * (d0.x + u2 + d2.x + w2);
                buf_store_one<T>(a.rc + (long long)jc * Pc + cc0, (jc >= clo && jc < chi) ? cbytes : 0,
                                 coff, v);
            }
            e0 = e1; e1 = e2;
            b0 = b1; b1 = b2;
            c0 = c1; c1 = c2;
            g0 = g1; g1 = g2;
            h0 = h1; h1 = h2;
            d0 = d1; d1 = d2;
            if constexpr (RC) {
                f7 = f6; f6 = f5;
                q6 = q5; q5 = q4;
            }
            f5 = f4; f4 = f3; f3 = f2; f2 = f1; f1 = f0;
            q4 = q3; q3 = q2; q2 = q1; q1 = q0;
        }
        __syncthreads();
    };
    if constexpr (D == 3) {
        // 6 rows per iteration, no guard inside: the row windows rotate with periods 3 (two
        // carried rows and the new one) and 6 (f), so after 6 rows every carried value is
        // back in its register (a guarded step would merge two paths and force copies)
        int gi = 0;
        for (; gi + 3 <= ng; gi += 3) {
            step(BodyStep<0>{}, gi, pxB, pfB, peB);
            step(BodyStep<1>{}, gi + 1, pxC, pfC, peC);
            step(BodyStep<2>{}, gi + 2, pxA, pfA, peA);
        }
        if (gi < ng) step(BodyStep<-1>{}, gi, pxB, pfB, peB);
        if (gi + 1 < ng) step(BodyStep<-1>{}, gi + 1, pxC, pfC, peC);
    } else {
        for (int gi = 0; gi < ng; gi += 2) {
            step(BodyStep<0>{}, gi, pxB, pfB, peB);
            if (gi + 1 < ng) step(BodyStep<1>{}, gi + 1, pxA, pfA, peA);
        }
    }
    const int slot = bk.y * gridDim.x + bk.x;
    const double s1 = block_sum(acc1, red);
    __syncthreads();
    const double s2 = block_sum(acc2, red);
    if (R2) {
        __syncthreads();
        const double s3 = block_sum(acc3, red);
        if (threadIdx.x == 0) a.partials3[slot] = s3;
    }
    if (threadIdx.x == 0) {
        a.partials1[slot] = s1;
        a.partials2[slot] = s2;
    }
}


// two waves per SIMD (3 spills and measured slower, r02)
// fp32: the minimum waves per SIMD the register allocation must allow (PGMG_F32_WAVES, r05);
// 2 lets it take up to 256 VGPRs (it uses 118 with the branch-form checks: 4 waves anyway;
// 4 with the select-form checks spills 140 bytes)
#ifndef PGMG_F32_WAVES
#define PGMG_F32_WAVES 2
#endif
template <class T> constexpr int pp_waves() { return sizeof(T) == 4 ? PGMG_F32_WAVES : 2; }
template <class T, bool R2, bool GENF, int OPT>
__global__ __launch_bounds__(64 * kPPWaves) __attribute__((amdgpu_waves_per_eu(pp_waves<T>())))
void k_postpre_lds(PostPreArgsT<T> a)
{
    __shared__ double red[kPPWaves];
    __shared__ __attribute__((aligned(16))) T sx[2][kPPR][pp_lds_row<T>()];
    __shared__ __attribute__((aligned(16))) T sf[2][kPPR][GENF ? 1 : pp_lds_row<T>()];
    __shared__ __attribute__((aligned(16))) T se[3][pp_lds_coarse<T>()];
    Blk bk{(int)blockIdx.x, (int)blockIdx.y};
    if (a.xcd) xcd_tile(bk.x, bk.y);
    const Cols k = lane_cols_t<pp_stride<OPT>(), pp_margin<OPT>()>(a.N, bk.x);
    // the band's rows 2jcb-6 .. 2jce+5 (RC: from 2jcb-8; see postpre_lds_run): does it reach
    // row 0 or N-1?
    const int jcb = a.jc0 + bk.y * a.rows_per_block;
    const int jce = min(jcb + a.rows_per_block, a.jc1);
    constexpr int lag = (OPT & 256) ? 2 : 0;
    const bool edge_rows = 2 * jcb - 6 - lag <= 0 || 2 * jce + 6 + lag >= a.N - 1;
    if (k.edge || edge_rows)
        postpre_lds_run<T, R2, GENF, true, OPT>(a, k, red, sx, sf, se, bk);
    else
        postpre_lds_run<T, R2, GENF, false, OPT>(a, k, red, sx, sf, se, bk);
}

// The cross-cycle finest-level pass.  OPT 2: non-temporal x4 stores (x4 is read again
// only by the next cycle's pass; r01: 1.18 vs 1.20 ms; non-temporal rc stores no gain).
// Forms (one GPU unless noted): the plain pass; R2 (row strips: the third sum); the carry pass
// (x2 stored instead of x4, OPT 128); the recompute form (OPT 256), alone or as a carry pass
// too (a one-cycle call that took the carry and makes the next); FAST (fp64) of each.
// Every launch path below launches: there is no configuration that returns without the pass.
template <class T, bool GENF, int OPT>
static void launch_pp_form(const PostPreArgsT<T> &a, dim3 g, dim3 b, hipStream_t s)
{
    launchk(k_postpre_lds<T, false, GENF, OPT>, g, b, s, a);
}
template <class T, int OPT>
static void launch_pp_form(const PostPreArgsT<T> &a, bool genf, dim3 g, dim3 b, hipStream_t s)
{
    if (genf) launch_pp_form<T, true, OPT>(a, g, b, s);
    else launch_pp_form<T, false, OPT>(a, g, b, s);
}

// The sampled-check forms (OPT | 512) of every form above: `form` is the full-sum switch's
// value (16 FAST, 128 carry, 256 recompute).  Instantiated by translation units of their own
// (pgmg_postpre_f64s.hip, pgmg_postpre_f32s.hip: these are the build's longest compiles), which
// define PGMG_POSTPRE_SAMPLED_TU; the others only see the declaration.
template <class T>
void launch_pp_sampled(const PostPreArgsT<T> &a, int form, bool genf, dim3 g, dim3 b, hipStream_t s);
#ifdef PGMG_POSTPRE_SAMPLED_TU
template <class T>
void launch_pp_sampled(const PostPreArgsT<T> &a, int form, bool genf, dim3 g, dim3 b, hipStream_t s)
{
    if constexpr (sizeof(T) == 8) {
        switch (form) {
        case 0: launch_pp_form<T, 2 | 512>(a, genf, g, b, s); break;
        case 16: launch_pp_form<T, 2 | 16 | 512>(a, genf, g, b, s); break;
        case 128: launch_pp_form<T, 2 | 128 | 512>(a, genf, g, b, s); break;
        case 144: launch_pp_form<T, 2 | 16 | 128 | 512>(a, genf, g, b, s); break;
        case 256: launch_pp_form<T, 2 | 256 | 512>(a, genf, g, b, s); break;
        case 272: launch_pp_form<T, 2 | 16 | 256 | 512>(a, genf, g, b, s); break;
        case 384: launch_pp_form<T, 2 | 128 | 256 | 512>(a, genf, g, b, s); break;
        default: launch_pp_form<T, 2 | 16 | 128 | 256 | 512>(a, genf, g, b, s); break;
        }
    } else {
        switch (form) {
        case 0: launch_pp_form<T, 2 | 512>(a, genf, g, b, s); break;
        case 128: launch_pp_form<T, 2 | 128 | 512>(a, genf, g, b, s); break;
        case 256: launch_pp_form<T, 2 | 256 | 512>(a, genf, g, b, s); break;
        default: launch_pp_form<T, 2 | 128 | 256 | 512>(a, genf, g, b, s); break;
        }
    }
}
#define PGMG_POSTPRE_SAMPLED_INSTANTIATE(T) \
    template void launch_pp_sampled<T>(const PostPreArgsT<T> &, int, bool, dim3, dim3, hipStream_t);
#endif

template <class T>
int launch_postpre(const PostPreArgsT<T> &a0, hipStream_t s)
{
    const bool rc = a0.recompute != 0, carry = a0.x2 != nullptr;
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r, rc ? kPPStrideRC : kPPStride,
                   pp_target(a0.jc0, a0.jc1), kPPWaves);
    if ((rc || carry) && a0.partials3 != nullptr) return PGMG_ERR_ARG;   // one GPU only
    if (carry == (a0.x4 != nullptr)) return PGMG_ERR_ARG;                // x2 replaces x4
    if (const int e = postpre_spans(a0, t, gx, r, true)) return e;
    PostPreArgsT<T> a = a0;
    a.rows_per_block = r;
    a.xcd = tuning_int("PGMG_PP_XCD", 1);
    const dim3 g(gx, gy), b(t);
    const bool genf = a.gfx != nullptr;
    const bool fast = a.fast && sizeof(T) == 8;   // FAST mode: fp64
    if (a.sampled && a.partials3 != nullptr) return PGMG_ERR_ARG;        // one GPU only
    if (a.partials3 != nullptr) {
        if (genf) launchk(k_postpre_lds<T, true, true, 2>, g, b, s, a);
        else launchk(k_postpre_lds<T, true, false, 2>, g, b, s, a);
    } else if (a.sampled) {
        launch_pp_sampled<T>(a, ((fast ? 16 : 0) | (carry ? 128 : 0) | (rc ? 256 : 0)), genf, g, b, s);
    } else if constexpr (sizeof(T) == 8) {
        switch ((fast ? 16 : 0) | (carry ? 128 : 0) | (rc ? 256 : 0)) {
        case 0: launch_pp_form<T, 2>(a, genf, g, b, s); break;
        case 16: launch_pp_form<T, 2 | 16>(a, genf, g, b, s); break;
        case 128: launch_pp_form<T, 2 | 128>(a, genf, g, b, s); break;
        case 144: launch_pp_form<T, 2 | 16 | 128>(a, genf, g, b, s); break;
        case 256: launch_pp_form<T, 2 | 256>(a, genf, g, b, s); break;
        case 272: launch_pp_form<T, 2 | 16 | 256>(a, genf, g, b, s); break;
        case 384: launch_pp_form<T, 2 | 128 | 256>(a, genf, g, b, s); break;
        default: launch_pp_form<T, 2 | 16 | 128 | 256>(a, genf, g, b, s); break;
        }
    } else {
        switch ((carry ? 128 : 0) | (rc ? 256 : 0)) {
        case 0: launch_pp_form<T, 2>(a, genf, g, b, s); break;
        case 128: launch_pp_form<T, 2 | 128>(a, genf, g, b, s); break;
        case 256: launch_pp_form<T, 2 | 256>(a, genf, g, b, s); break;
        default: launch_pp_form<T, 2 | 128 | 256>(a, genf, g, b, s); break;
        }
    }
    // phi (x2 of the previous call in the recompute form), f (unless regenerated), ec in; x4
    // (x2 in the carry pass), rc out: the same bytes in every form
    const double n = row_pts(std::max(2 * a.jc0, a.row_lo), std::min(2 * a.jc1, a.row_hi), a.N);
    const double nc = row_pts(a.rc_lo, a.rc_hi, a.Nc);
    g_last_launch.bytes = (8.0 * n * (2 + (genf ? 0 : 1)) + 16.0 * nc) * sizeof(T) / 8.0;
    return PGMG_OK;
}

// ---------------------------------------------------------------------------
// Fused smooth(3) (JacobiSmoother::smooth with num_iter = 3, Smoother.hpp:38-116): four
// sweeps x0 -> x4 in ONE pass of k_postpre_lds (OPT 64: no correction, no restriction)
// with the checks ||r(x1)||, ||r(x2)||, ||r(x3)|| < eps summed speculatively; the decision
// kernel finds the first check that fires and the rare-path kernel recomputes x_k from
// the untouched x0.  Used by the F-cycle climb on the levels below the finest.
// ---------------------------------------------------------------------------
template <class T>
int launch_smooth4(const PostPreArgsT<T> &a0, hipStream_t s)
{
    int t, gx, gy, r;
    fused_geometry(a0.N, a0.jc0, a0.jc1, &t, &gx, &gy, &r, kPPStride, pp_target(a0.jc0, a0.jc1),
                   kPPWaves);
    if (const int e = postpre_spans(a0, t, gx, r, false)) return e;
    PostPreArgsT<T> a = a0;
    a.rows_per_block = r;
    a.xcd = tuning_int("PGMG_F_XCD", 1);
    if (a.gfx != nullptr) k_postpre_lds<T, true, true, 64><<<dim3(gx, gy), dim3(t), 0, s>>>(a);
    else k_postpre_lds<T, true, false, 64><<<dim3(gx, gy), dim3(t), 0, s>>>(a);
    return PGMG_OK;
}

// the launchers of one element type (and with them every kernel they launch)
#define PGMG_POSTPRE_INSTANTIATE(T)                                          \
    template int launch_postpre<T>(const PostPreArgsT<T> &, hipStream_t);    \
    template int launch_smooth4<T>(const PostPreArgsT<T> &, hipStream_t);

}  // namespace pgmg
