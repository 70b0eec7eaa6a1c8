// pgmg_fused_geom.h — what the fused passes' kernels, their launchers and the span checks
// must agree on (internal to pgmg_fused.hip and the pass files pgmg_pre.hip, pgmg_post.hip,
// pgmg_postpre_impl.h): the wave-tile constants, the launch geometry and the read/write extents.
// The functions are defined in pgmg_fused.hip.
#pragma once
#include "pgmg_fused.h"

namespace pgmg {

// k_pre / k_post: 128-column wave tiles owning 120, 4-column margin (pgmg_fused_dev.h).
constexpr int kR2Stride = 116;   // k_post_r2's wave-tile stride (6-column margin)
// k_postpre_lds: 128-column wave tiles owning 116: six stencil levels shrink the validity six
// columns from the left; on the right the prolongation reads coarse column ic+1 from LDS (no
// DPP), so six suffice there too (114 + 6/8 before: 1.13-1.14 -> 1.11-1.13 ms; 112 + 8/8 with
// line-aligned stores: slower, 1.133 ms)
constexpr int kPPStride = 116, kPPMargin = 6;
constexpr int kPPWaves = 4;   // waves per k_postpre block (8-wave blocks measured equal, r02)
// The recompute form (OPT 256, the first finest pass of a call that took the carry): two more
// Jacobi stages in front, so two more columns of margin per side (112-column stride) and two
// more lead rows
constexpr int kPPStrideRC = 112, kPPMarginRC = 8;
constexpr int kPPR = 2;   // rows per LDS slot of k_postpre_lds (a row pair)

// Bands of coarse rows [jc0, jc1) and column blocks of `maxw` wave tiles `stride` columns
// apart: threads per workgroup, grid (gx, gy) and coarse rows per band.  target: workgroups
// aimed at (0: the default per level size, see the definition).
void fused_geometry(int N, int jc0, int jc1, int *threads, int *gx, int *gy, int *rpb,
                    int stride = 120, int target = 0, int maxw = 4);
int r2_target();                  // k_post_r2's grid target (launch and log sizing)
int pp_target(int jc0, int jc1);  // k_postpre_lds's grid target (likewise)

// Read/write extents of a pass launched with t threads, gx column blocks and r coarse rows per
// band, each checked against the allocation registry (check_span): PGMG_OK, or the error of the
// first span outside its array (then nothing may be launched).
template <class T>
int pre_spans(const PreArgsT<T> &a, int t, int gx, int r, bool x0_read, bool f_read);
template <class T>
int post_spans(const PostArgsT<T> &a, int t, int gx, int r, bool f_read, bool r2 = false);
template <class T>
int postpre_spans(const PostPreArgsT<T> &a, int t, int gx, int r, bool coarse);

// one span of a T array inside a function that returns the error code
#define PGMG_SPAN(o, P, r0, r1, c0, c1, what)                                                  \
    do {                                                                                       \
        const int e_ = check_span((o), (P), (int)sizeof(T), (r0), (r1), (c0), (c1), (what));   \
        if (e_) return e_;                                                                     \
    } while (0)

}  // namespace pgmg
