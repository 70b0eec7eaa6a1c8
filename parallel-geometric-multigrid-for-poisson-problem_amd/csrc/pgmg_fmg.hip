// pgmg_fmg.hip — full multigrid for the problem's own right-hand side (include/pgmg.h "Full
// multigrid"): the cubic interpolation pass k_interp_cubic, the restricted f
// chain, the climb, pgmg_fmg and pgmg_fmg_interp_time.
//
// pgmg_fcycle is the reference's F-cycle, which rebuilds the analytic right-hand side on every
// level; pgmg_fmg restricts the f the problem was set with (full weighting, level by level),
// solves the coarsest level from zero and climbs: each finer level starts from the CUBIC
// interpolation of the coarser solution and runs nu V-cycles with its restricted f.  Everything
// but the interpolation is the existing machinery: launch_restrict_values for the f chain, the
// LDS tail (one launch per level at or below the tail's top, that level as its top) and
// enqueue_cycle from a bulk level with the level's restricted f standing in for lv[l].F.
// pgmg_fmg_damped is the same climb with the damping pass (pgmg_monitor.hip, fmg_damp_level)
// after every V-cycle of it, on that level's grids.  pgmg_fmg_bc is either climb with the frame
// of the current phi carried down the pyramid by injection (k_frame_save, k_frame_inject) and
// put back on every level after the interpolation, beside the passes, not inside them.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "pgmg_host.h"

using namespace pgmg;

namespace pgmg {

constexpr int kCubU = 4;   // coarse rows of loads in flight per wave

template <class T>
struct InterpArgsT {
    const T *c;          // element (0, 0) of the coarse grid, pitch Pc
    T *f;                // element (0, 0) of the fine grid (2 Nc - 1 points per side), pitch Pf
    long long Pc, Pf;
    int Nc;
    int band;            // coarse rows per workgroup
};

// Tensor-product cubic interpolation, every fine point assigned (pgmg.h has the formulas).
// Lane t of a workgroup owns coarse column i = 1 + 256 bx + t and writes the fine column pair
// (2i-1, 2i) of every fine row of its band as one aligned 16-byte store (8 bytes in fp32:
// column 1 of a row lies on a 128-byte boundary, so a wave's 64 pairs are whole lines); fine
// column 0 rides with the lane that owns i = 1.  A row of the coarse grid is interpolated
// along x in registers: the lane's own value is one load, c[i-1], c[i-2] and c[i+1] come from
// the neighbouring lanes by DPP (lanes 0 and 63 load their halo columns; the moves are
// unconditional, every lane of a running wave is active: a move inside a branch that disables
// its source lane reads stale data).  The two one-sided columns (fine 1 and Nf-2) are a second
// expression selected per lane in the waves that hold them, a wave-uniform branch.  The
// workgroup marches down its band of coarse rows j (fine rows 2j-1, 2j) with a four-row window
// of x-interpolated rows, kCubU coarse rows loaded before the first is used; the one-sided
// rows (fine 1 and Nf-2) take their fourth row from one extra load in a workgroup-uniform
// branch.  Lanes past the last column load column Nc-1 again and store nothing.
template <class T>
__global__ __launch_bounds__(kBlock) void k_interp_cubic(InterpArgsT<T> a)
{
    using D2 = V2<T>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Nc = a.Nc;
    const int i0 = 1 + blockIdx.x * kBlock + wave * 64;   // the wave's first coarse column
    if (i0 > Nc - 1) return;                              // (wave-uniform; no barrier below)
    const int i = i0 + lane;
    const bool own = i <= Nc - 1;
    const int ic = min(i, Nc - 1);
    const bool first = i == 1, last = i == Nc - 1;
    const bool edge_wave = i0 == 1 || Nc - 1 < i0 + 64;   // holds fine column 1 or Nf-2
    const int xcol = first ? 3 : Nc - 4;                  // the one-sided formulas' fourth point
    const long long Pc = a.Pc, Pf = a.Pf;
    const T *__restrict__ C = a.c;
    T *__restrict__ F = a.f;
    const T k9 = T(9), k5 = T(5), k15 = T(15), s16 = T(0.0625);

    // what one coarse row contributes: the lane's loads ...
    struct RowLd {
        T own, hb, ha, hd, x3;
    };
    auto load_row = [&](int r) -> RowLd {
        const T *p = C + (long long)r * Pc;
        RowLd v;
        v.own = p[ic];
        v.hb = v.ha = v.hd = v.x3 = T(0);
        if (lane == 0) {
            v.hb = p[ic - 1];
            v.ha = p[max(ic - 2, 0)];
        }
        if (lane == 63) v.hd = p[min(ic + 1, Nc - 1)];
        if (edge_wave) v.x3 = p[xcol];
        return v;
    };
    // ... and its x-interpolation: .x fine column 2i-1, .y fine column 2i; z = coarse column
    // i-1 (fine column 0 for the lane that owns i = 1)
    auto xrow = [&](const RowLd &v, T &z) -> D2 {
        T b = dpp_shr(v.own);
        if (lane == 0) b = v.hb;
        T aa = dpp_shr(b);
        if (lane == 0) aa = v.ha;
        T d = dpp_shl(v.own);
        if (lane == 63) d = v.hd;
        T odd = (k9 * (b + v.own) - (aa + d)) * s16;
        if (edge_wave) {
            const T p1 = (k5 * b + k15 * v.own - k5 * d + v.x3) * s16;
            const T pn = (k5 * v.own + k15 * b - k5 * aa + v.x3) * s16;
            odd = first ? p1 : (last ? pn : odd);
        }
        z = b;
        return mk2<T>(odd, v.own);
    };
    auto put = [&](int fr, D2 v, T z) {
        T *p = F + (long long)fr * Pf;
        if (own) stv(p + 2 * i - 1, v);
        if (first) p[0] = z;
    };

    const int jb = 1 + blockIdx.y * a.band;
    const int je = min(jb + a.band, Nc);   // coarse rows jb .. je-1 (at most Nc-1)
    D2 wa, wb, wc;                         // x-interpolated rows j-2, j-1, j
    T za, zb, zc;
    {
        const RowLd ra = load_row(max(jb - 2, 0)), rb = load_row(jb - 1), rc = load_row(jb);
        wa = xrow(ra, za);
        wb = xrow(rb, zb);
        wc = xrow(rc, zc);
    }
    if (jb == 1) put(0, wb, zb);
    for (int j = jb; j < je; j += kCubU) {
        RowLd ld[kCubU];
        #pragma unroll
        for (int u = 0; u < kCubU; ++u) ld[u] = load_row(min(j + u + 1, Nc - 1));
        #pragma unroll
        for (int u = 0; u < kCubU; ++u) {
            const int r = j + u;   // this step's coarse row (uniform over the workgroup)
            T zd;
            const D2 wd = xrow(ld[u], zd);
            if (r < je) {
                D2 o;
                T zo;
                if (r == 1 || r == Nc - 1) {
                    // fine row 1: rows 0, 1, 2 and 3; fine row Nf-2: rows Nc-1 .. Nc-4
                    T zx;
                    const RowLd rx = load_row(r == 1 ? 3 : Nc - 4);
                    const D2 wx = xrow(rx, zx);
                    if (r == 1) {
                        o.x = (k5 * wb.x + k15 * wc.x - k5 * wd.x + wx.x) * s16;
                        o.y = (k5 * wb.y + k15 * wc.y - k5 * wd.y + wx.y) * s16;
                        zo = (k5 * zb + k15 * zc - k5 * zd + zx) * s16;
                    } else {
                        o.x = (k5 * wc.x + k15 * wb.x - k5 * wa.x + wx.x) * s16;
                        o.y = (k5 * wc.y + k15 * wb.y - k5 * wa.y + wx.y) * s16;
                        zo = (k5 * zc + k15 * zb - k5 * za + zx) * s16;
                    }
                } else {
                    o.x = (k9 * (wb.x + wc.x) - (wa.x + wd.x)) * s16;
                    o.y = (k9 * (wb.y + wc.y) - (wa.y + wd.y)) * s16;
                    zo = (k9 * (zb + zc) - (za + zd)) * s16;
                }
                put(2 * r - 1, o, zo);
                put(2 * r, wc, zc);
            }
            wa = wb;
            wb = wc;
            wc = wd;
            za = zb;
            zb = zc;
            zc = zd;
        }
    }
}

struct InterpGrid {
    int gx, gy, band;
};
// bands of 32 coarse rows (64 fine rows, 256 KB of fp64 output per workgroup), shorter while
// a level has fewer than ~1024 workgroups
static InterpGrid interp_grid(int Nc)
{
    InterpGrid g;
    g.gx = (Nc - 1 + kBlock - 1) / kBlock;
    g.band = 32;
    while (g.band > 4 && g.gx * ((Nc - 1 + g.band - 1) / g.band) < 1024) g.band /= 2;
    g.gy = (Nc - 1 + g.band - 1) / g.band;
    return g;
}

// fine = C(coarse), Nc >= 5 points per side; both spans are checked against the registered
// allocations before the launch (every coarse and every fine point, nothing past them)
template <class T>
static int launch_interp_cubic(const T *coarse, int Nc, int Pc, T *fine, int Pf, hipStream_t s)
{
    const int Nf = 2 * Nc - 1;
    if (Nc < 5) return set_err(PGMG_ERR_ARG, "cubic interpolation needs 5 coarse points per side");
    PGMG_TRY(check_span(coarse, Pc, (int)sizeof(T), 0, Nc - 1, 0, Nc - 1, "k_interp_cubic coarse"));
    PGMG_TRY(check_span(fine, Pf, (int)sizeof(T), 0, Nf - 1, 0, Nf - 1, "k_interp_cubic fine"));
    InterpArgsT<T> a{};
    a.c = coarse;
    a.f = fine;
    a.Pc = Pc;
    a.Pf = Pf;
    a.Nc = Nc;
    const InterpGrid g = interp_grid(Nc);
    a.band = g.band;
    k_interp_cubic<T><<<dim3(g.gx, g.gy), dim3(kBlock), 0, s>>>(a);
    return PGMG_OK;
}

// pgmg_fmg_bc: the frame g of level-0 phi (rows 0 and N-1, columns 0 and N-1) is saved into the
// context's frame buffer -- top row, bottom row, left column, right column, N elements each --
// before anything of the call writes level 0, and injected into a level's grids from there:
// g_l(j, i) = g(stride j, stride i), stride = 2^l.  A corner is one element of g, stored in a
// row line and in a column line: both writers of a corner write the same value.
template <class T>
__global__ void k_frame_save(const T *src, long long P, int N, T *frame)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < 4 * N; k += gridDim.x * blockDim.x) {
        const int q = k % N, w = k / N;
        const int j = w == 0 ? 0 : (w == 1 ? N - 1 : q);
        const int i = w < 2 ? q : (w == 2 ? 0 : N - 1);
        frame[k] = src[(long long)j * P + i];
    }
}

// the four frame lines of an Nl x Nl level grid from the buffer of the (Nl - 1) stride + 1
// points per side of level 0 (the column stores are pitch-strided: 4 Nl elements a level)
template <class T>
__global__ void k_frame_inject(T *dst, long long P, int Nl, const T *frame, int stride)
{
    const long long N = (long long)(Nl - 1) * stride + 1;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < 4 * Nl; k += gridDim.x * blockDim.x) {
        const int q = k % Nl, w = k / Nl;
        const int j = w == 0 ? 0 : (w == 1 ? Nl - 1 : q);
        const int i = w < 2 ? q : (w == 2 ? 0 : Nl - 1);
        dst[(long long)j * P + i] = frame[w * N + (long long)q * stride];
    }
}

// the frame buffer, 4 N elements of the context's type (allocated on the first pgmg_fmg_bc)
static int fmg_frame_reserve(pgmg_ctx *c)
{
    if (c->fmg_frame) return PGMG_OK;
    const size_t bytes = (size_t)4 * c->cfg.N * c->lv[0].es;
    if (hipMalloc(&c->fmg_frame, bytes) != hipSuccess) {
        c->fmg_frame = nullptr;
        return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_fmg_bc's frame buffer");
    }
    register_alloc(c->fmg_frame, bytes);
    return PGMG_OK;
}

template <class T>
static int launch_frame_save(pgmg_ctx *c, const T *src, int P, int N)
{
    T *frame = static_cast<T *>(c->fmg_frame);
    PGMG_TRY(check_span(src, P, (int)sizeof(T), 0, N - 1, 0, N - 1, "k_frame_save phi"));
    PGMG_TRY(check_span(frame, 0, (int)sizeof(T), 0, 0, 0, 4LL * N - 1, "k_frame_save frame"));
    k_frame_save<T><<<dim3((4 * N + 255) / 256), dim3(256), 0, c->s>>>(src, P, N, frame);
    return PGMG_OK;
}

// level l's frame g_l into one of its grids (N_0 = (Nl - 1) 2^l + 1: the buffer's line length)
template <class T>
static int launch_frame_inject(pgmg_ctx *c, T *dst, int P, int Nl, int l)
{
    const T *frame = static_cast<const T *>(c->fmg_frame);
    const long long N = (long long)(Nl - 1) * (1LL << l) + 1;
    if (N != c->cfg.N) return set_err(PGMG_ERR_STATE, "k_frame_inject: not a level of this context");
    PGMG_TRY(check_span(dst, P, (int)sizeof(T), 0, Nl - 1, 0, Nl - 1, "k_frame_inject grid"));
    PGMG_TRY(check_span(frame, 0, (int)sizeof(T), 0, 0, 0, 4 * N - 1, "k_frame_inject frame"));
    k_frame_inject<T><<<dim3((4 * Nl + 255) / 256), dim3(256), 0, c->s>>>(dst, P, Nl, frame, 1 << l);
    return PGMG_OK;
}

// FMG level l of the context: levels 0 .. nb are the context's own (bulk levels and the tail's
// top), the ones below continue the halving down to the first N <= n_coarse
static int fmg_setup(pgmg_ctx *c)
{
    if (!c->fmg_lv.empty()) return PGMG_OK;
    std::vector<Level> lv(c->lv.begin(), c->lv.end());
    for (Level &L : lv) L.A = L.B = L.F = Grid{};   // geometry only: the grids are c->lv's
    while (lv.back().N > c->cfg.n_coarse) {
        Level L = lv.back();
        L.N = (L.N - 1) / 2 + 1;
        L.P = c->fp32 ? pitch_elems<float>(L.N) : pitch_elems<double>(L.N);
        L.h = 2 * L.h;
        L.hh = L.h * L.h;
        L.ih = 1.0 / (L.h * L.h);
        L.lo = 0;
        L.hi = L.N;
        L.u0 = 1;
        L.u1 = L.N - 1;
        lv.push_back(L);
    }
    const int n = (int)lv.size();
    c->fmg_F.assign(n, Grid{});
    c->fmg_U.assign(n, Grid{});
    c->fmg_lv = lv;   // (set first: pgmg_destroy frees whatever an allocation failure leaves)
    for (int l = 1; l < n; ++l) {
        PGMG_TRY(alloc_grid(c->fmg_F[l], lv[l]));
        if (l > c->nb) PGMG_TRY(alloc_grid(c->fmg_U[l], lv[l]));
    }
    return PGMG_OK;
}

static int fmg_coarsest_n(const pgmg_ctx *c)
{
    int N = c->cfg.N;
    while (N > c->cfg.n_coarse) N = (N - 1) / 2 + 1;
    return N;
}

static const Grid &fmg_u(const pgmg_ctx *c, int l) { return l <= c->nb ? c->lv[l].A : c->fmg_U[l]; }
static const Grid &fmg_f(const pgmg_ctx *c, int l) { return l == 0 ? c->lv[0].F : c->fmg_F[l]; }

// a bulk level's restricted f stands in for lv[l].F while the level cycles (its V-cycles write
// the coarser levels' own F grids with restricted residuals); undone on every way out
struct FmgLevelF {
    pgmg_ctx *c;
    int l;
    FmgLevelF(pgmg_ctx *c_, int l_) : c(c_), l(l_)
    {
        if (l > 0) std::swap(c->lv[l].F, c->fmg_F[l]);
    }
    ~FmgLevelF()
    {
        if (l > 0) std::swap(c->lv[l].F, c->fmg_F[l]);
    }
};

// omega > 0 (pgmg_fmg_damped): one damping pass after every V-cycle of the climb
// bc (pgmg_fmg_bc): every u_l carries the frame g_l of the current phi instead of a zero one
template <class T>
static int fmg_enqueue(pgmg_ctx *c, int nu, double omega, bool bc)
{
    const bool damped = omega > 0.0;
    const int nb = c->nb, Lc = (int)c->fmg_lv.size() - 1;
    const std::vector<Level> &lv = c->fmg_lv;
    // 0. g, before the last interpolation (or, at Lc = 0, the coarsest start) overwrites it
    if (bc) PGMG_TRY(launch_frame_save(c, G<T>(c->lv[0].A), lv[0].P, lv[0].N));
    auto inject = [&](const Grid &g, int l) -> int {
        return launch_frame_inject(c, G<T>(g), lv[l].P, lv[l].N, l);
    };
    // 1. the f chain, level by level (every level's values are used)
    for (int l = 0; l < Lc; ++l)
        launch_restrict_values(G<T>(fmg_f(c, l)), lv[l].N, lv[l].P, G<T>(c->fmg_F[l + 1]), lv[l + 1].N,
                               lv[l + 1].P, c->s);
    // nu V-cycles of a level at or below the tail's top: one k_tail launch with that level as
    // its top (at N <= n_coarse the coarsest smoother call)
    auto tail_level = [&](int l, bool from_global, int visits) -> int {
        TailArgsT<T> t = tail_args<T>(c);
        t.f_top = G<T>(fmg_f(c, l));
        t.e_top = G<T>(fmg_u(c, l));
        t.P_top = lv[l].P;
        t.N_top = lv[l].N;
        t.h_top = lv[l].h;
        t.visits = visits;
        t.x0_from_global = from_global ? 1 : 0;
        HIPC(launch_tail_gamma(t, 1, c->s));
        return PGMG_OK;
    };
    // 2. the coarsest level from zero (the tail starts from zero in LDS and stores every point);
    // with a frame: from the zeroed grid with g_L injected, read from global memory
    if (bc) {
        const Grid &u = fmg_u(c, Lc);
        PGMG_TRY(check_span(G<T>(u), lv[Lc].P, (int)sizeof(T), 0, lv[Lc].N - 1, 0, lv[Lc].P - 1,
                            "pgmg_fmg_bc coarsest grid"));
        launch_fill_rows(G<T>(u), lv[Lc].P, 0, lv[Lc].N, c->s);
        PGMG_TRY(inject(u, Lc));
    }
    PGMG_TRY(tail_level(Lc, bc, nu));
    // 3. the climb
    for (int l = Lc - 1; l >= 0; --l) {
        PGMG_TRY(launch_interp_cubic(G<T>(fmg_u(c, l + 1)), lv[l + 1].N, lv[l + 1].P,
                                     G<T>(fmg_u(c, l)), lv[l].P, c->s));
        if (bc) {
            // the interpolated frame is g_l + O(h^4): the caller's data goes back bitwise
            PGMG_TRY(inject(fmg_u(c, l), l));
            // level l + 1 is a child from here on, entered from zero: the frames of its error
            // grids are zero again (a tail top is stored whole by its first visit)
            if (l + 1 < nb) {
                launch_zero_frame(G<T>(c->lv[l + 1].A), lv[l + 1].P, lv[l + 1].N, c->s);
                launch_zero_frame(G<T>(c->lv[l + 1].B), lv[l + 1].P, lv[l + 1].N, c->s);
            }
        }
        const bool gen = l == 0 && c->rgfx != nullptr;   // level 0's analytic f: regenerated
        if (l >= nb) {
            if (!damped) {
                PGMG_TRY(tail_level(l, true, nu));
                continue;
            }
            // a damp between the cycles: one launch per cycle, each from the damped grid
            for (int k = 0; k < nu; ++k) {
                PGMG_TRY(tail_level(l, true, 1));
                PGMG_TRY(fmg_damp_level(c, fmg_u(c, l), fmg_f(c, l), lv[l], omega, gen));
            }
            continue;
        }
        // u_l has a zero boundary (u_L = 0 and C keeps it), or g_l: the level's other grids (the
        // ping-pong buffer; at level 0 the cross-fused cycles rotate through S too) mirror it
        Level &L = c->lv[l];
        if (bc) {
            PGMG_TRY(inject(L.B, l));
            if (l == 0 && c->S.base) PGMG_TRY(inject(c->S, 0));
        } else {
            launch_zero_frame(G<T>(L.B), L.P, L.N, c->s);
            if (l == 0 && c->S.base) launch_zero_frame(G<T>(c->S), L.P, L.N, c->s);
        }
        const FmgLevelF stand_in(c, l);
        // the damp of what a cycle left: every cycle ends with its iterate under lv[l].A, but
        // which grid that is may change (the cross-fused cycles swap the roles of A / B / S), so
        // the grids are read here, after the cycle; f is the stand-in
        auto damp = [&]() -> int {
            return fmg_damp_level(c, c->lv[l].A, c->lv[l].F, lv[l], omega, gen);
        };
        // a cross-fused context runs level 0's nu cycles as k_pre, (k_postpre) x (nu - 1), k_post
        // (one finest pass per further cycle instead of two), every check in-stream
        if (l == 0 && c->cross) {
            if (!damped) {
                PGMG_TRY(run_cycles_plain(c, nu, 1, false));
                continue;
            }
            // (a damp between the cycles: nu calls of one cycle, k_pre .. k_post each)
            for (int k = 0; k < nu; ++k) {
                PGMG_TRY(run_cycles_plain(c, 1, 1, false));
                PGMG_TRY(damp());
            }
            continue;
        }
        for (int k = 0; k < nu; ++k) {
            PGMG_TRY(enqueue_cycle(c, l, 1, false));
            if (damped) PGMG_TRY(damp());
        }
    }
    return PGMG_OK;
}

// pgmg_fmg (omega = 0), pgmg_fmg_damped and, with bc, pgmg_fmg_bc
static int fmg_run(pgmg_ctx *c, int nu, double omega, const char *who_, bool bc = false)
{
    const std::string who(who_);
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (nu < 1) return set_err(PGMG_ERR_ARG, who + ": nu must be at least 1");
    if (omega != 0.0) PGMG_TRY(damp_omega_check(omega, who_));
    if (fmg_coarsest_n(c) < 5)
        return set_err(PGMG_ERR_ARG, who + ": the coarsest level needs 5 points per side for the "
                                           "cubic interpolation (n_coarse >= 5)");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    PGMG_TRY(fmg_setup(c));
    // the damping pass's side buffer and partials, sized for level 0 (the largest) before
    // anything is enqueued
    if (omega != 0.0) PGMG_TRY(fmg_damp_reserve(c, c->cfg.N));
    if (bc) PGMG_TRY(fmg_frame_reserve(c));
    // an entry that changes phi: the carry goes, the speculation starts over (the statistics
    // continue)
    c->carry = false;
    c->hist.reset(c->nb);
    const CallScope scope{c};
    // a device-bound problem: the caller's f into the level-0 RHS grid, the climb on the
    // context's grids, the result copied into the caller's phi (synchronous, like pgmg_fcycle)
    const bool ext = c->ext_phi != nullptr;
    if (ext) PGMG_TRY(ext_stage_in(c, false));
    HIPC(hipEventRecord(c->ev0, c->s));
    PGMG_TRY(c->fp32 ? fmg_enqueue<float>(c, nu, omega, bc) : fmg_enqueue<double>(c, nu, omega, bc));
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev1, c->s));
    if (ext) {
        PGMG_TRY(ext_stage_out(c));
        PGMG_TRY(stream_wait(c));
    }
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_fmg(pgmg_ctx *c, int nu) { return fmg_run(c, nu, 0.0, "pgmg_fmg"); }

int pgmg_fmg_damped(pgmg_ctx *c, int nu, double omega)
{
    // (omega = 0 is no damped call: refused here, fmg_run reads it as pgmg_fmg)
    if (omega == 0.0) return damp_omega_check(omega, "pgmg_fmg_damped");
    return fmg_run(c, nu, omega, "pgmg_fmg_damped");
}

int pgmg_fmg_bc(pgmg_ctx *c, int nu, double omega)
{
    // (omega = 0: the undamped climb; fmg_run checks any other value)
    return fmg_run(c, nu, omega, "pgmg_fmg_bc", true);
}

int pgmg_fmg_interp_time(pgmg_ctx *c, int reps, double *ms_per_pass, double *bytes)
{
    if (!c || !ms_per_pass || reps <= 0) return set_err(PGMG_ERR_ARG, "bad argument");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, "pgmg_fmg_interp_time: one GPU only (world 1)");
    if (fmg_coarsest_n(c) < 5 || c->cfg.N < 9)
        return set_err(PGMG_ERR_ARG, "pgmg_fmg_interp_time: needs a level 1 of 5 points per side");
    PGMG_TRY(fmg_setup(c));
    c->carry = false;   // phi is overwritten
    const Level &L0 = c->fmg_lv[0], &L1 = c->fmg_lv[1];
    auto run = [&]() {
        return c->fp32 ? launch_interp_cubic(G<float>(fmg_u(c, 1)), L1.N, L1.P, G<float>(fmg_u(c, 0)), L0.P, c->s)
                       : launch_interp_cubic(G<double>(fmg_u(c, 1)), L1.N, L1.P, G<double>(fmg_u(c, 0)), L0.P, c->s);
    };
    for (int k = 0; k < 2; ++k) PGMG_TRY(run());
    HIPC(hipEventRecord(c->ev0, c->s));
    for (int k = 0; k < reps; ++k) PGMG_TRY(run());
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev1, c->s));
    HIPC(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms_per_pass = f / reps;
    if (bytes) *bytes = (double)L0.es * ((double)L0.N * L0.N + (double)L1.N * L1.N);
    return PGMG_OK;
}

}  // extern "C"
