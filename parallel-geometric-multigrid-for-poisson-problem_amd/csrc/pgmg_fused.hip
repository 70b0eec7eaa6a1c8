// pgmg_fused.hip — launch geometry and read/write extents of the fused smoother passes.
// Host only.
//
// With v1 = v2 = 1 a level of the default cycle costs two HBM passes instead of six, and the
// finest level between two cycles of a call one.  The passes and their launchers:
//   pgmg_pre.hip         k_pre (two sweeps, residual, restriction), k_pre1, k_pre_rare
//   pgmg_post.hip        k_post (prolongation, two sweeps), k_post_r2, k_post1, k_post_rare
//   pgmg_postpre_impl.h  k_postpre_lds (post-smooth of cycle k + pre-smooth of cycle k+1) and
//                        its smooth(3) form; compiled by pgmg_postpre_f64.hip / _f32.hip
//   pgmg_fixup.hip       the scalar fix-ups and the decision kernels of their checks
// (device helpers: pgmg_fused_dev.h; the checks' sums and decision: pgmg_check.h).
// Here is what their launchers share (pgmg_fused_geom.h): how a level is cut into bands and
// column blocks (fused_geometry), and the rows and columns each pass then reads and writes,
// checked against the allocations before a pass is launched.
#include <algorithm>
#include <cstdlib>

#include "pgmg.h"
#include "pgmg_fused_geom.h"

namespace pgmg {

// ---------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------
// Launch geometry.  Blocks march down long row bands: the grid is sized to about
// the number of workgroups resident at once, so the 8 halo rows per band are a small
// fraction and there is no tail wave of blocks.
thread_local LaunchNote g_last_launch;

#ifdef PGMG_TUNING
int tuning_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
#endif

void fused_geometry(int N, int jc0, int jc1, int *threads, int *gx, int *gy, int *rpb,
                    int stride, int target, int maxw)
{
    const int waves = (N - 2 + stride - 1) / stride;
    const int wpb = waves < maxw ? waves : maxw;
    *threads = 64 * wpb;
    *gx = (waves + wpb - 1) / wpb;
    const int rows = jc1 - jc0;   // coarse rows
    // ~22k fine points per workgroup, 256 .. 3072 workgroups: measured per level at N =
    // 16385 (scripts/level_sweep.sh): 8193 best at 3072, 4097 at 768 (band halos), and
    // the finest level's first/last passes at 3072 (6 rounds of the 512 resident)
    if (target <= 0) {
        const long long pts = 2LL * rows * N;
        if (pts > (1LL << 23)) {
            // ~22k points per workgroup, at least one round of the 512 resident (8193 on 8
            // strips: 37+28 -> 34+24 us), at most 3072
            // (measurement build: PGMG_FUSED_BLOCKS_BIG for the levels of N >= 8193 alone)
            const int dflt = (int)std::min(3072LL, std::max(512LL, pts / 21845));
            target = tuning_int("PGMG_FUSED_BLOCKS", pts >= (1LL << 25) ? tuning_int("PGMG_FUSED_BLOCKS_BIG", dflt) : dflt);
        } else {
            // latency-bound levels (N <= 2049): short bands (~8k points per workgroup);
            // measured at N = 16385: 2049 26+20 -> 23+18 us, 1025 13+11 -> 12+10, 513..129
            // 12+10 -> 7+7
            target = tuning_int("PGMG_FUSED_SMALL_BLOCKS",
                                (int)std::max((long long)tuning_int("PGMG_FUSED_SMALL_MIN", 256),
                                              pts / tuning_int("PGMG_FUSED_SMALL_PTS", 8192)));
        }
    }

    // (no cap on the band height: a cap of 512 coarse rows once turned a one-round target of
    // 504 workgroups at N = 16385 into 576, i.e. 1.125 rounds)
    const int rmin = 2, rmax = 1 << 20;
    // bands so that gx * gy does not exceed the target (a target of whole rounds of the
    // resident workgroups must not spill a few workgroups into one more round: 3096
    // workgroups for a 3072 target cost ~2 % in k_postpre)
    const int gymax = std::max(1, target / *gx);
    int r = (rows + gymax - 1) / gymax;
    r = r < rmin ? rmin : (r > rmax ? rmax : r);
    if (r > rows) r = rows;
    if (r < 1) r = 1;
    *rpb = r;
    *gy = (rows + r - 1) / r;
}

int fused_blocks(int N, int jc0, int jc1)
{
    int t, gx, gy, r;
    fused_geometry(N, jc0, jc1, &t, &gx, &gy, &r);
    return gx * gy;
}

// k_post_r2's workgroups (its 116-column tiles): the partial sums its check writes
// k_post_r2's grid target (0: fused_geometry's default, 3072 at N = 16385 = 4 rounds of the 768
// resident at 3 waves/SIMD); one function for the launch and the log sizing
int r2_target() { return tuning_int("PGMG_R2_BLOCKS", 0); }

int post_r2_blocks(int N, int jc0, int jc1)
{
    int t, gx, gy, r;
    fused_geometry(N, jc0, jc1, &t, &gx, &gy, &r, kR2Stride, r2_target());
    return gx * gy;
}

// k_postpre's grid target: 3072 workgroups = 6 full rounds of the 512 that are resident
// at once (2 per CU at its ~200 VGPRs); measured r01 against 2048 .. 8192
// (PGMG_PP_BLOCKS): 2048 1.30 ms, 3072 1.18 ms, 4096 1.25 ms, 8192 1.28 ms at N = 16385.
// Workgroups of k_postpre: whole rounds of the 512 resident (2 per CU at 184 VGPRs), about
// one round per ~2700 fine rows: 3072 on the full 16385 grid (r01: 2048 1.30 ms, 3072 1.18,
// 4096 1.25), 512 on strips of 2048 / 4096 rows (scripts/strip_probe.py, per-rank time at
// 8 ranks 0.43 -> 0.39 ms; 768 / 1024, i.e. 1.5 / 2 rounds of short bands, lose)
// (r02: bands of ~190 fine rows are the invariant — on the 32769 grid 12 rounds, 6144
// workgroups, beat 6: 6.79 -> 6.70 ms per V-cycle; 9216 / 12288 the same as 6144)
int pp_target(int jc0, int jc1)
{
    const int rounds = std::max(1, std::min(12, 6 * (2 * (jc1 - jc0) + 64) / 16384));
    return tuning_int("PGMG_PP_BLOCKS", (2048 / kPPWaves) * rounds);   // 512 resident at 4 waves
}

int postpre_blocks(int N, int jc0, int jc1, bool rc)
{
    int t, gx, gy, r;
    fused_geometry(N, jc0, jc1, &t, &gx, &gy, &r, rc ? kPPStrideRC : kPPStride, pp_target(jc0, jc1),
                   kPPWaves);
    return gx * gy;
}

// ---------------------------------------------------------------------------
// read/write extents of the fused passes (pgmg_internal.h, check_span)
// ---------------------------------------------------------------------------
// Every span below restates the kernel's own loop bounds: a band of coarse rows
// [jcb, jce) streams fine rows 2jcb - lead .. 2jcb - lead + ceil((2(jce - jcb) + extra) / R)
// * R - 1 (k_pre: lead 4, extra 8, R 4; k_post: 2, 4, 4; k_postpre_lds: 6, 11, 2), and wave w
// of a 120-column tiling reads columns 120w - 3 .. 120w + 124 unless it is idle
// (120w - 3 + 4 > N - 2).
static inline long long fdiv2(long long v) { return v >= 0 ? v / 2 : -((1 - v) / 2); }

struct Span {
    long long r0, r1;   // fine rows (inclusive)
    bool any;
};

static Span band_rows(int jc0, int jc1, int r, int lead, int extra, int R)
{
    Span sp{0, -1, false};
    if (jc1 <= jc0 || r <= 0) return sp;
    const int nb = (jc1 - jc0 + r - 1) / r;
    sp.r0 = 2LL * jc0 - lead;
    for (int b = std::max(0, nb - 2); b < nb; ++b) {   // the last (full or short) bands
        const int jcb = jc0 + b * r, jce = std::min(jcb + r, jc1);
        const long long n = ((2LL * (jce - jcb) + extra + R - 1) / R) * R;
        sp.r1 = std::max(sp.r1, 2LL * jcb - lead + n - 1);
    }
    sp.any = true;
    return sp;
}

// last column read by a non-idle wave of k_pre / k_post (120-column stride, 4-column
// margin: wave w covers 120w - 3 .. 120w + 124); -1 when every wave is idle
static long long tile_col_hi(int N, int waves, int stride = 120, int margin = 4)
{
    // wave w's tile starts at column stride*w + 1 - margin; idle once that + 4 > N - 2
    const int wmax = std::min(waves - 1, (N - 7 + margin) / stride);
    return wmax < 0 ? -1 : (long long)stride * wmax + 1 - margin + 127;
}

// k_pre / k_pre_rare: x0 and f over the band rows, the PIN coarse rows, x2 and rc stores
template <class T>
int pre_spans(const PreArgsT<T> &a, int t, int gx, int r, bool x0_read, bool f_read)
{
    const Span sp = band_rows(a.jc0, a.jc1, r, 4, 8, 4);
    const long long chi = tile_col_hi(a.N, gx * (t / 64));
    if (!sp.any || chi < 0) return PGMG_OK;
    if (x0_read) PGMG_SPAN(a.x0, a.Px != 0 ? a.Px : a.P, sp.r0, sp.r1, -3, chi, "k_pre x0");
    if (f_read) PGMG_SPAN(a.f, a.P, sp.r0, sp.r1, -3, chi, "k_pre f");
    if (a.pin_ec != nullptr)   // coarse rows i/2 .. i/2 + 2 of every 4-row iteration i
        PGMG_SPAN(a.pin_ec, a.Pc, fdiv2(sp.r0), fdiv2(sp.r1 + 1 - 4) + 2, -2,
                  fdiv2(chi - 2) + 1, "k_pre PIN coarse grid");
    const int olo = std::max(2 * a.jc0, a.row_lo), ohi = std::min(2 * a.jc1, a.row_hi);
    if (a.x2 != nullptr) PGMG_SPAN(a.x2, a.P, olo, ohi - 1, 1, a.N - 1, "k_pre x2");
    const int clo = std::max(a.jc0, std::max(1, a.rc_lo));
    const int chi2 = std::min(a.jc1, std::min(a.N / 2, a.rc_hi));
    if (a.rc != nullptr) PGMG_SPAN(a.rc, a.Pc, clo, chi2 - 1, 1, a.Nc - 2, "k_pre rc");
    return PGMG_OK;
}

// k_post / k_post_rare: phi (or f one row ahead, RECOMP), f, the coarse correction, x2
// (r2: k_post_r2's bands start 4 rows earlier and stream 6 rows more)
template <class T>
int post_spans(const PostArgsT<T> &a, int t, int gx, int r, bool f_read, bool r2)
{
    const Span sp = band_rows(a.jc0, a.jc1, r, r2 ? 6 : 2, r2 ? 10 : 4, 4);
    const int margin = r2 ? 6 : 4;   // k_post_r2: 116-column stride, 6-column margin
    const long long chi = tile_col_hi(a.N, gx * (t / 64), r2 ? kR2Stride : 120, margin);
    const long long clo = 1 - margin;
    if (!sp.any || chi < 0) return PGMG_OK;
    if (a.pre_fired != nullptr) {   // RECOMP: f rows i_begin - 1 .. last + 1, phi not read
        PGMG_SPAN(a.f, a.P, sp.r0 - 1, sp.r1 + 1, clo, chi, "k_post f (recompute)");
    } else {
        PGMG_SPAN(a.phi, a.P, sp.r0, sp.r1, clo, chi, "k_post phi");
        if (f_read) PGMG_SPAN(a.f, a.P, sp.r0, sp.r1, clo, chi, "k_post f");
    }
    PGMG_SPAN(a.ec, a.Pc, fdiv2(sp.r0), fdiv2(sp.r1 + 1 - 4) + 2, fdiv2(clo - 1), fdiv2(chi - 2) + 1,
              "k_post coarse correction");
    const int olo = std::max(2 * a.jc0, a.row_lo), ohi = std::min(2 * a.jc1, a.row_hi);
    if (a.x2 != nullptr) PGMG_SPAN(a.x2, a.Po != 0 ? a.Po : a.P, olo, ohi - 1, 1, a.N - 1, "k_post x2");
    return PGMG_OK;
}

// k_postpre_lds (and its smooth(3) form, coarse = false): each block loads its window of
// row pairs through buffer descriptors (columns L0 .. L0 + 2 nvx - 1, coarse columns
// cc0 .. cc0 + nve - 1; the descriptor range stops them at the grid's last column)
template <class T>
int postpre_spans(const PostPreArgsT<T> &a, int t, int gx, int r, bool coarse)
{
    const int lag = a.recompute ? 2 : 0;   // the recompute form: 2 more rows each end
    const int ST = a.recompute ? kPPStrideRC : kPPStride, MG = a.recompute ? kPPMarginRC : kPPMargin;
    const Span sp = band_rows(a.jc0, a.jc1, r, 6 + lag, 11 + 2 * lag, kPPR);
    if (!sp.any) return PGMG_OK;
    const int wpb = t / 64;
    const int npairs = (ST * wpb + 2 * MG) / 2;
    const int ncc = (ST / 2) * wpb + MG + 2;
    long long c1 = -1, e0 = 0, e1 = -1;
    bool first = true;
    for (int bx = 0; bx < gx; ++bx) {
        const int L0 = ST * wpb * bx + 1 - MG;
        const int nvx = std::max(0, std::min(npairs, (a.N - 1 - L0) / 2 + 1));
        if (nvx > 0) c1 = std::max(c1, (long long)L0 + 2 * nvx - 1);
        const int cc0 = (L0 - 1) >> 1;
        const int nve = std::max(0, std::min(ncc, a.Nc - cc0));
        if (nve > 0) {
            e0 = first ? cc0 : std::min(e0, (long long)cc0);
            e1 = std::max(e1, (long long)cc0 + nve - 1);
            first = false;
        }
    }
    const long long c0 = 1 - MG;
    if (c1 < c0) return PGMG_OK;
    PGMG_SPAN(a.phi, a.P, sp.r0, sp.r1, c0, c1, "k_postpre phi");
    if (a.gfx == nullptr) PGMG_SPAN(a.f, a.P, sp.r0, sp.r1, c0, c1, "k_postpre f");
    if (coarse && e1 >= e0)   // coarse rows m0 .. m0 + ng of a band (m0 = jcb - 3; RC jcb - 5)
        PGMG_SPAN(a.ec, a.Pc, a.jc0 - 3 - lag, fdiv2(sp.r1 + 1), e0, e1, "k_postpre coarse correction");
    const int olo = std::max(2 * a.jc0, a.row_lo), ohi = std::min(2 * a.jc1, a.row_hi);
    if (a.x4 != nullptr) PGMG_SPAN(a.x4, a.P, olo, ohi - 1, 1, a.N - 1, "k_postpre x4");
    if (a.x2 != nullptr) PGMG_SPAN(a.x2, a.P, olo, ohi - 1, 1, a.N - 1, "k_postpre x2 (carry pass)");
    if (coarse && a.rc != nullptr) {
        const int clo = std::max(a.jc0, std::max(1, a.rc_lo));
        const int chi = std::min(a.jc1, std::min(a.N / 2, a.rc_hi));
        PGMG_SPAN(a.rc, a.Pc, clo, chi - 1, 1, a.Nc - 2, "k_postpre rc");
    }
    return PGMG_OK;
}

#define PGMG_INSTANTIATE(T)                                                          \
    template int pre_spans<T>(const PreArgsT<T> &, int, int, int, bool, bool);       \
    template int post_spans<T>(const PostArgsT<T> &, int, int, int, bool, bool);     \
    template int postpre_spans<T>(const PostPreArgsT<T> &, int, int, int, bool);
PGMG_INSTANTIATE(double)
PGMG_INSTANTIATE(float)
#undef PGMG_INSTANTIATE

}  // namespace pgmg
