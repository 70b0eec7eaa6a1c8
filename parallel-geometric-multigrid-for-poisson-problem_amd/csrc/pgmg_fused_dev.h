// pgmg_fused_dev.h — device helpers shared by the fused smoother passes (pgmg_pre.hip,
// pgmg_post.hip, pgmg_postpre_impl.h): a lane's column pair and its wave tile, the Jacobi and
// residual stages on a row, the check sums' terms, the prolongation of a row, the XCD-aware
// tile order and the row loop.
//
// Tiling: a wave owns 120 columns but loads 128 (4-column overlap each side), so
// every stencil level's horizontal neighbours come from the adjacent lane by DPP
// and the validity shrinks one column per level: x0 [c0, c0+127] -> x1 [+1,-1] ->
// x2 [+2,-2] -> r [+3,-3] -> rc centres [+4,-4] = the owned columns.  (k_post_r2 and
// k_postpre_lds run more levels and own 116 or 112 columns: pgmg_fused_geom.h.)
//
// Every expression keeps the reference's left-to-right order; built with
// -ffp-contract=off, so the results are bit-identical to the unfused path.
#pragma once
#include <type_traits>

#include "pgmg_check.h"
#include "pgmg_fused.h"
#include "pgmg_fused_geom.h"

namespace pgmg {

struct Cols {
    int c;          // odd column of this lane's pair (c, c+1)
    bool bx, by;    // column c / c+1 is a boundary (or outside) column: passthrough
    bool own;       // lane owns its pair (lanes 2..61 of the wave tile)
    bool edge;      // wave-uniform: some lane of this wave has a boundary/outside column
};

// fp32 stencil stages as packed 2-vector arithmetic (pgmg_real.h pf2); 0 = the scalar
// expressions (measurement builds: scripts/build_variant.sh NAME -DPGMG_F32_PK=0)
#ifndef PGMG_F32_PK
#define PGMG_F32_PK 1
#endif
// One Jacobi stage on a row: J(ce) with boundary passthrough.  EDGE = false: the caller
// guarantees that neither the row nor any column of the wave is a boundary (no selects).
template <class T, bool EDGE = true>
__device__ __forceinline__ V2<T> jstage(V2<T> up, V2<T> ce, V2<T> dn, V2<T> f, T hh,
                                          const Cols &k, bool brow)
{
    const T l = dpp_shr(ce.y);
    const T r = dpp_shl(ce.x);
    V2<T> o;
    if constexpr (sizeof(T) == 4 && PGMG_F32_PK) {   // packed: L = (l, c), R = (c+1, r)
        const pf2 L = {l, ce.x}, R = {ce.y, r};
        o = unpk(0.25f * (((((hh * pk(f)) + L) + R) + pk(up)) + pk(dn)));
    } else {
        o.x = T(0.25) * ((hh * f.x) + l + ce.y + up.x + dn.x);
        o.y = T(0.25) * ((hh * f.y) + ce.x + r + up.y + dn.y);
    }
    if constexpr (EDGE) {
        if (brow || k.bx) o.x = ce.x;
        if (brow || k.by) o.y = ce.y;
    }
    return o;
}

// J(0): the Jacobi stage of an all-zero iterate, 0.25 * ((hh*f) + 0 + 0 + 0 + 0).  The first
// +0 turns a -0 into +0 and the other three change nothing, so ONE add of +0 gives the same
// IEEE result (the compiler may not drop x + 0 itself: it is not an identity for x = -0)
template <class T, bool EDGE = true>
__device__ __forceinline__ V2<T> j0stage(V2<T> f, T hh, const Cols &k, bool brow)
{
    V2<T> o;
    o.x = T(0.25) * ((hh * f.x) + T(0));
    o.y = T(0.25) * ((hh * f.y) + T(0));
    if constexpr (EDGE) {
        if (brow || k.bx) o.x = T(0);
        if (brow || k.by) o.y = T(0);
    }
    return o;
}

// Residual r = f - (1/h^2)(4x - xl - xr - xu - xd) on a row (DynamicGridUtils.hpp:59-69)
template <class T>
__device__ __forceinline__ V2<T> rstage(V2<T> up, V2<T> ce, V2<T> dn, V2<T> f, T ih)
{
    const T l = dpp_shr(ce.y);
    const T r = dpp_shl(ce.x);
    V2<T> o;
    if constexpr (sizeof(T) == 4 && PGMG_F32_PK) {
        const pf2 L = {l, ce.x}, R = {ce.y, r};
        o = unpk(pk(f) - ih * ((((4.0f * pk(ce) - L) - R) - pk(up)) - pk(dn)));
    } else {
        o.x = f.x - ih * (T(4) * ce.x - l - ce.y - up.x - dn.x);
        o.y = f.y - ih * (T(4) * ce.y - ce.x - r - up.y - dn.y);
    }
    return o;
}

// Check sums of k_postpre_lds: acc + r.x^2 (+ r.y^2 unless column c+1 is a boundary) on an
// owned pair of a band row.  PGMG_CHK_SEL (r05): as selects instead of a branch around the
// residual (0: neither type, 1: fp32 only, 2: both, 3: fp64 only) -- a skipped term adds
// (+0)^2, which leaves the sum (>= +0) bitwise unchanged, and the residual's dependent chain,
// no longer in a branch of its own, can interleave with the sweeps around it.  Measured at
// 16385 (scripts/pp_ab.py, profiles/r05_fp32/chk_sel_*.jsonl, 3-4 interleaved rounds on two
// boxes): fp64 0.4-0.6 % faster (1.0687 -> 1.0646 ms); fp32 6 % slower although its packed
// chains lose their s_nops (92 -> 12 per 6 rows): 118 -> 161 VGPRs, 4 -> 3 waves per SIMD
// (and at 2 register sets of loads, 109 VGPRs, still 4.6 % slower) -- so fp64 only.
#ifndef PGMG_CHK_SEL
#define PGMG_CHK_SEL 3
#endif
template <int M, class T> constexpr bool chk_sel_m() { return M == 2 || (M == 1 && sizeof(T) == 4) || (M == 3 && sizeof(T) == 8); }
template <class T> constexpr bool chk_sel() { return chk_sel_m<PGMG_CHK_SEL, T>(); }
// the same choice for the check sums of k_post_r2 (the F-cycle's finest post pass; same
// values).  Measured (scripts/pp_ab.py, profiles/r05_fp32/chk_sel_post_*.jsonl, 3 interleaved
// rounds): selects in every k_post -- F at 16385 4.449 -> 4.408 ms per cycle (-0.9 %), V at
// 16385 1.7875 -> 1.7917 (+0.2 %, level 1's k_post), V at 4097 equal; in k_post_r2 alone
// (chk_sel_r2only_*.jsonl) F 4.470 -> 4.421 (-1.1 %), V unchanged -- so k_post_r2 only.
// In k_pre the select form raises most instantiations' VGPRs by 14-100, several from 3 to 2
// waves per SIMD: not used there.
#ifndef PGMG_CHK_SEL_LV
#define PGMG_CHK_SEL_LV 3
#endif
template <class T> constexpr bool chk_sel_lv() { return chk_sel_m<PGMG_CHK_SEL_LV, T>(); }
template <class T>
__device__ __forceinline__ double chk_acc(double acc, V2<T> r, bool in, bool by)
{
    const T rx = in ? r.x : T(0);
    const T ry = (in && !by) ? r.y : T(0);
    return sqacc(sqacc(acc, rx), ry);
}

// Row factor of the regenerated RHS through the constant address space: a scalar load
// (the table is read-only), not a per-row vector load the row loop would wait on
__device__ __forceinline__ double gsy_s(const double *gsy, int row)
{
    return ((const __attribute__((address_space(4))) double *)gsy)[row];
}

__device__ __forceinline__ bool boundary_row(int row, int N) { return row <= 0 || row >= N - 1; }

// Wave tile: STRIDE owned columns, loaded window starts MARGIN columns to the left;
// lanes [MARGIN/2, 63 - (64*2 - STRIDE - MARGIN)/2] own their pair.
template <int STRIDE, int MARGIN>
__device__ __forceinline__ Cols lane_cols_t(int N, int bx = -1)
{
    if (bx < 0) bx = blockIdx.x;
    const int wave = (bx * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    Cols k;
    k.c = STRIDE * wave + 1 - MARGIN + 2 * lane;
    k.bx = k.c <= 0 || k.c >= N - 1;
    k.by = k.c + 1 <= 0 || k.c + 1 >= N - 1;
    k.own = lane >= MARGIN / 2 && lane < MARGIN / 2 + STRIDE / 2 && k.c <= N - 2;
    // the wave's columns are [c0, c0 + 127]: uniform, kept in a scalar register
    const int c0 = __builtin_amdgcn_readfirstlane(STRIDE * wave + 1 - MARGIN);
    k.edge = c0 <= 0 || c0 + 127 >= N - 1;
    return k;
}

__device__ __forceinline__ Cols lane_cols(int N, int bx = -1) { return lane_cols_t<120, 4>(N, bx); }

// Logical (column block, band) of this workgroup.  xcd: XCD-aware order -- the hardware
// deals linear workgroup ids round-robin to the 8 XCDs (id mod 8), so XCD x takes the ids
// x, x+8, ...; those get one contiguous run of tiles, and tiles that share halo columns run
// side by side behind the same L2 (k_postpre: 1.1 % per V-cycle)
__device__ __forceinline__ void xcd_tile(int &bx, int &by)
{
    const int nb = (int)(gridDim.x * gridDim.y), id = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const int q = nb >> 3, r = nb & 7, x = id & 7;
    const int t = x * q + min(x, r) + (id >> 3);
    bx = t % (int)gridDim.x;
    by = t / (int)gridDim.x;
}
__device__ __forceinline__ void fused_block(int &bx, int &by, bool xcd = false)
{
    bx = blockIdx.x;
    by = blockIdx.y;
    if (xcd) xcd_tile(bx, by);
}

struct ProlongCols {
    bool vx, vy;   // column c / c+1 receives a correction
    int ic;        // coarse column of the odd fine column c: (c-1)/2
};

// EDGE = false: the caller guarantees row in [2, Nf-2] and both columns in [2, Nf-2]
// (interior bands and wave tiles), so no masks
template <class T, bool EDGE = true>
__device__ __forceinline__ V2<T> add_prolong(V2<T> p, int row, T ca, T cb, T da, T db, const ProlongCols &pc, int Nc)
{
    // MultiGrid.hpp:219-223; row in [2, Nf-2] <=> its coarse row m in [1, Nc-2]
    const int m = row >> 1;
    if (EDGE && (m < 1 || m > Nc - 2)) return p;
    if ((row & 1) == 0) {
        if (!EDGE || pc.vx) p.x = p.x + T(0.5) * (ca + cb);
        if (!EDGE || pc.vy) p.y = p.y + cb;
    } else {
        if (!EDGE || pc.vx) p.x = p.x + T(0.25) * (ca + cb + da + db);
        if (!EDGE || pc.vy) p.y = p.y + T(0.5) * (cb + db);
    }
    return p;
}

// The row loop of k_pre / k_post: iterations of R rows at i = i_begin, i_begin + R, ..,
// < i_end; full_at(i) holds on one contiguous run of them.  The run is executed three
// iterations (3R = 12 rows) at a time with no branch inside: the row windows (two carried
// rows and the new one: period 3; f in k_pre: period 4) come back to their registers after
// 12 rows, and no merge of the FULL and general paths forces copies of every window.
template <int R, int U, class FullAt, class Iter>
__device__ __forceinline__ void row_loop(int i_begin, int i_end, const FullAt &full_at, const Iter &iter)
{
    int i = i_begin;
    if constexpr (U == 0) {   // one loop, the path chosen per iteration
        for (; i < i_end; i += R) {
            if (full_at(i)) iter(i, std::true_type{});
            else iter(i, std::false_type{});
        }
        return;
    }
    for (; i < i_end && !full_at(i); i += R) iter(i, std::false_type{});
    if constexpr (U == 3) {
        for (; i + 3 * R <= i_end && full_at(i + 2 * R); i += 3 * R) {
            iter(i, std::true_type{});
            iter(i + R, std::true_type{});
            iter(i + 2 * R, std::true_type{});
        }
    } else {
        for (; i < i_end && full_at(i); i += R) iter(i, std::true_type{});
    }
    for (; i < i_end; i += R) {
        if (full_at(i)) iter(i, std::true_type{});
        else iter(i, std::false_type{});
    }
}

}  // namespace pgmg
