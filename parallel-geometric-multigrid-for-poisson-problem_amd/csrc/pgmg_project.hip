// pgmg_project.hip — the pressure projection (include/pgmg.h "Projection"):
// k_divergence, k_grad_update, pgmg_project and pgmg_project_time (pgmg_divergence_grid and
// pgmg_gradient_add_grid, on the caller's arrays: pgmg_ops.hip).
//
// Two streaming passes beside k_gradient (pgmg_gradient.hip), in its shape and on its
// decomposition grad_grid(N): lane t of a wave owns the column pair (1 + 2t, 2 + 2t), column 0
// rides with the lane that owns column 1, a workgroup marches down a band of rows, kGradU rows of
// loads in flight; the x neighbours at +-1 and +-2 of the array differenced along x are the
// neighbouring lanes' pairs, moved by DPP (lanes 0 and 63 load their halo pair, the lane that owns
// columns N-2 and N-1 the one value its one-sided formulas reach past its left neighbour for);
// the array differenced along y is a window of rows in registers; the one-sided columns are a
// second expression in the waves that hold them (wave-uniform), the one-sided rows a branch on
// the row (uniform over the workgroup) that loads the rows of its stencil again.
//   k_divergence   out = dx(u) + dy(v): u is read once per row with its halos, v through the
//                  window (its column 0 by the first lane; no halo loads); out may be null, the
//                  pass then only sums.  The norm follows k_gradient's scheme and k_grad_reduce
//                  adds the partials.
//   k_grad_update  u += gx(phi), v += gy(phi): phi as k_gradient reads it, a point's u and v read
//                  and written by the lane that owns it alone, so the update is safe in place
//                  whatever the launch geometry.
// Every value is formed as include/pgmg.h writes it: the line formula, * w, then one add.
#include <chrono>
#include <cmath>
#include <limits>
#include <string>

#include "pgmg_grad_dev.h"
#include "pgmg_host.h"
#include "pgmg_stop.h"

using namespace pgmg;

namespace pgmg {

using PD2 = V2<double>;

// a lane's share of one row: its pair and the two values an edge lane loads beside it
struct PRow {
    PD2 o;
    double hx, hy;
};

// what k_gradient derives from the lane's place in the grid (its names)
template <int ORDER>
struct PLanes {
    int lane, N, c, cl, ix, iy, nw;
    bool act, firstl, lastl, edge_wave, edge;
    __device__ __forceinline__ PLanes(int N_) : N(N_)
    {
        lane = threadIdx.x & 63;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int npairs = (N - 1) >> 1;                 // pairs (1+2t, 2+2t) cover columns 1 .. N-1
        const int p0 = blockIdx.x * kBlock + wave * 64;  // the wave's first pair
        nw = min(max(npairs - p0, 0), 64);               // its pairs
        c = 1 + 2 * (p0 + lane);                         // this lane's columns c, c + 1
        act = lane < nw;
        cl = min(c, N - 2);                              // (a lane past the last pair loads the last)
        firstl = p0 + lane == 0;                         // owns columns 0, 1 and 2
        lastl = p0 + lane == npairs - 1;                 // owns columns N-2 and N-1
        edge_wave = p0 == 0 || npairs <= p0 + 64;        // holds a one-sided column
        edge = act && (lane == 0 || lane == 63 || lastl);
        ix = lastl ? N - 1 - ORDER : (lane == 0 ? max(c - 2, 0) : min(c + 2, N - 1));
        iy = lastl ? N - 1 - ORDER : (lane == 0 ? c - 1 : min(c + 3, N - 1));
    }
    // a row of the array differenced along x: the pair and the edge lanes' two values
    __device__ __forceinline__ PRow load_x(const double *p) const
    {
        PRow v;
        v.o = ldvu<double>(p + cl);
        v.hx = v.hy = 0.0;
        if (edge) {
            v.hx = p[ix];
            v.hy = p[iy];
        }
        return v;
    }
    // a row of the array differenced along y only: the pair, and column 0 in the first lane (hy)
    __device__ __forceinline__ PRow load_y(const double *p) const
    {
        PRow v;
        v.o = ldvu<double>(p + cl);
        v.hx = v.hy = 0.0;
        if (firstl) v.hy = p[0];
        return v;
    }
    // the difference along x on the lane's pair of a row, and (g0, the first lane's) on column 0.
    // The moves are unconditional: every lane of the wave is active here
    __device__ __forceinline__ PD2 xdiff(const PRow &ce, double w, double &g0) const
    {
        PD2 l = mk2<double>(dpp_shr(ce.o.x), dpp_shr(ce.o.y));
        PD2 r = mk2<double>(dpp_shl(ce.o.x), dpp_shl(ce.o.y));
        if (lane == 0) l = mk2<double>(ce.hx, ce.hy);
        if (lane == 63) r = mk2<double>(ce.hx, ce.hy);
        PD2 g;
        g0 = 0.0;
        if constexpr (ORDER == 4) {
            g.x = (8.0 * (ce.o.y - l.y) - (r.x - l.x)) * w;
            g.y = (8.0 * (r.x - ce.o.x) - (r.y - l.y)) * w;
            if (edge_wave) {
                // the first lane: columns 0 .. 4 are l.y, its pair and r; the last: columns
                // N-5 .. N-1 are hx, l and its pair
                const double f0 = os4_first(l.y, ce.o.x, ce.o.y, r.x, r.y) * w;
                const double f1 = os4_second(l.y, ce.o.x, ce.o.y, r.x, r.y) * w;
                const double e1 = os4_penult(ce.hx, l.x, l.y, ce.o.x, ce.o.y) * w;
                const double e0 = os4_last(ce.hx, l.x, l.y, ce.o.x, ce.o.y) * w;
                g0 = f0;
                g.x = firstl ? f1 : (lastl ? e1 : g.x);
                g.y = lastl ? e0 : g.y;
            }
        } else {
            g.x = (ce.o.y - l.y) * w;
            g.y = (r.x - ce.o.x) * w;
            if (edge_wave) {
                const double f0 = os2_first(l.y, ce.o.x, ce.o.y) * w;
                const double e0 = os2_last(l.y, ce.o.x, ce.o.y) * w;
                g0 = f0;
                g.y = lastl ? e0 : g.y;
            }
        }
        return g;
    }
};

// the central difference along y from the window s[0 .. 2H] of rows r-H .. r+H (pair and hy)
template <int ORDER>
__device__ __forceinline__ PD2 ydiff(const PRow *s, double w, double &g0)
{
    PD2 g;
    if constexpr (ORDER == 4) {
        const PRow &m2 = s[0], &m1 = s[1], &q1 = s[3], &q2 = s[4];
        g.x = (8.0 * (q1.o.x - m1.o.x) - (q2.o.x - m2.o.x)) * w;
        g.y = (8.0 * (q1.o.y - m1.o.y) - (q2.o.y - m2.o.y)) * w;
        g0 = (8.0 * (q1.hy - m1.hy) - (q2.hy - m2.hy)) * w;
    } else {
        const PRow &m1 = s[0], &q1 = s[2];
        g.x = (q1.o.x - m1.o.x) * w;
        g.y = (q1.o.y - m1.o.y) * w;
        g0 = (q1.hy - m1.hy) * w;
    }
    return g;
}

// the one-sided difference along y on row r (r < H or r > N-1-H) from the ORDER + 1 rows q of
// its stencil, rows 0 .. ORDER or N-1-ORDER .. N-1
template <int ORDER>
__device__ __forceinline__ PD2 ydiff_onesided(const PRow *q, int r, int N, double w, double &g0)
{
    PD2 g;
    if constexpr (ORDER == 4) {
        if (r == 0) {
            g.x = os4_first(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
            g.y = os4_first(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
            g0 = os4_first(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
        } else if (r == 1) {
            g.x = os4_second(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
            g.y = os4_second(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
            g0 = os4_second(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
        } else if (r == N - 2) {
            g.x = os4_penult(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
            g.y = os4_penult(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
            g0 = os4_penult(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
        } else {
            g.x = os4_last(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
            g.y = os4_last(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
            g0 = os4_last(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
        }
    } else {
        if (r == 0) {
            g.x = os2_first(q[0].o.x, q[1].o.x, q[2].o.x) * w;
            g.y = os2_first(q[0].o.y, q[1].o.y, q[2].o.y) * w;
            g0 = os2_first(q[0].hy, q[1].hy, q[2].hy) * w;
        } else {
            g.x = os2_last(q[0].o.x, q[1].o.x, q[2].o.x) * w;
            g.y = os2_last(q[0].o.y, q[1].o.y, q[2].o.y) * w;
            g0 = os2_last(q[0].hy, q[1].hy, q[2].hy) * w;
        }
    }
    return g;
}

struct DivArgs {
    const double *u, *v;   // element (0, 0), pitch N
    double *out;           // element (0, 0), pitch Po; null: nothing is stored
    long long Po;
    double *partials;      // one per workgroup, or null
    double w;              // scale * 0.5 / h (order 2), scale / (12 h) (order 4)
    int N;
    int band;              // rows per workgroup
};

template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_divergence(DivArgs a)
{
    static_assert(ORDER == 2 || ORDER == 4, "second or fourth order");
    constexpr int H = ORDER / 2;    // rows the central y stencil reaches either way
    constexpr int NR = ORDER + 1;   // points of a one-sided stencil
    static_assert(kGradU >= 2 * H, "the window is the tail of an iteration's rows");
    __shared__ double red[kBlock / 64];
    const int N = a.N;
    const PLanes<ORDER> L(N);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double *__restrict__ U = a.u;
    const double *__restrict__ V = a.v;
    const double w = a.w;
    double acc = 0.0;
    auto vrow = [&](int r) { return L.load_y(V + (long long)r * N); };

    // (wave-uniform; a wave past the last column only joins the block sum)
    if (L.nw > 0) {
        const int jb = blockIdx.y * a.band;
        const int je = min(jb + a.band, N);
        // s[0 .. 2H-1]: the window of v, rows j-H .. j+H-1; s[2H ..]: this iteration's loads.
        // Rows are clamped into the grid: a clamped row only feeds a row outside the grid or a
        // one-sided row, which takes its own
        PRow s[2 * H + kGradU];
        #pragma unroll
        for (int k = 0; k < 2 * H; ++k) s[k] = vrow(min(max(jb - H + k, 0), N - 1));
        for (int j = jb; j < je; j += kGradU) {
            PRow ur[kGradU];
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) s[2 * H + k] = vrow(min(j + k + H, N - 1));
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) ur[k] = L.load_x(U + (long long)min(j + k, N - 1) * N);
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) {
                const int r = j + k;   // this step's row (uniform over the workgroup)
                double dx0;
                const PD2 dx = L.xdiff(ur[k], w, dx0);
                if (r < je) {
                    PD2 dy;
                    double dy0;
                    if (r < H || r > N - 1 - H) {
                        PRow q[NR];
                        const int base = r < H ? 0 : N - 1 - ORDER;
                        #pragma unroll
                        for (int m = 0; m < NR; ++m) q[m] = vrow(base + m);
                        dy = ydiff_onesided<ORDER>(q, r, N, w, dy0);
                    } else {
                        dy = ydiff<ORDER>(&s[k], w, dy0);
                    }
                    if (L.act) {
                        const PD2 o = mk2<double>(dx.x + dy.x, dx.y + dy.y);
                        const double o0 = dx0 + dy0;
                        if (a.out != nullptr) {
                            double *p = a.out + (long long)r * a.Po + L.c;
                            stvu<double>(p, o);
                            if (L.firstl) p[-1] = o0;
                        }
                        acc += sq(o.x);
                        acc += sq(o.y);
                        if (L.firstl) acc += sq(o0);
                    }
                }
            }
            #pragma unroll
            for (int k = 0; k < 2 * H; ++k) s[k] = s[kGradU + k];
        }
    }
    if (a.partials == nullptr) return;   // (uniform over the grid)
    const double sw = wave_sum(acc);
    if (L.lane == 0) red[wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        #pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) t += red[k];
        a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

struct UpdArgs {
    const double *x;    // element (0, 0) of phi, pitch Px
    long long Px;
    double *u, *v;      // element (0, 0), pitch N; either may be null
    double w;
    int N;
    int band;
};

template <int ORDER>
__global__ __launch_bounds__(kBlock) void k_grad_update(UpdArgs a)
{
    static_assert(ORDER == 2 || ORDER == 4, "second or fourth order");
    constexpr int H = ORDER / 2;
    constexpr int NR = ORDER + 1;
    static_assert(kGradU >= 2 * H, "the window is the tail of an iteration's rows");
    const int N = a.N;
    const PLanes<ORDER> L(N);
    if (L.nw <= 0) return;   // (wave-uniform; no barrier below)
    const double *__restrict__ X = a.x;
    const long long Px = a.Px;
    const double w = a.w;
    auto xrow = [&](int r) { return L.load_x(X + r * Px); };
    // a row of the field as it is: the pair of u and of v, and column 0 in the first lane
    struct Cur {
        PD2 u, v;
        double u0, v0;
    };
    auto cur = [&](int r) -> Cur {
        Cur q;
        q.u = q.v = mk2<double>(0.0, 0.0);
        q.u0 = q.v0 = 0.0;
        const long long at = (long long)r * N;
        if (a.u != nullptr) {
            q.u = ldvu<double>(a.u + at + L.cl);
            if (L.firstl) q.u0 = a.u[at];
        }
        if (a.v != nullptr) {
            q.v = ldvu<double>(a.v + at + L.cl);
            if (L.firstl) q.v0 = a.v[at];
        }
        return q;
    };

    const int jb = blockIdx.y * a.band;
    const int je = min(jb + a.band, N);
    PRow s[2 * H + kGradU];   // (k_divergence's window, of phi)
    #pragma unroll
    for (int k = 0; k < 2 * H; ++k) s[k] = xrow(min(max(jb - H + k, 0), N - 1));
    for (int j = jb; j < je; j += kGradU) {
        Cur f[kGradU];
        #pragma unroll
        for (int k = 0; k < kGradU; ++k) s[2 * H + k] = xrow(min(j + k + H, N - 1));
        // (a row past the band is loaded and dropped: only its owner writes it)
        #pragma unroll
        for (int k = 0; k < kGradU; ++k) f[k] = cur(min(j + k, N - 1));
        #pragma unroll
        for (int k = 0; k < kGradU; ++k) {
            const int r = j + k;   // this step's row (uniform over the workgroup)
            double gx0;
            const PD2 gx = L.xdiff(s[k + H], w, gx0);
            if (r < je) {
                PD2 gy;
                double gy0;
                if (r < H || r > N - 1 - H) {
                    PRow q[NR];
                    const int base = r < H ? 0 : N - 1 - ORDER;
                    #pragma unroll
                    for (int m = 0; m < NR; ++m) q[m] = xrow(base + m);
                    gy = ydiff_onesided<ORDER>(q, r, N, w, gy0);
                } else {
                    gy = ydiff<ORDER>(&s[k], w, gy0);
                }
                if (L.act) {
                    const long long at = (long long)r * N + L.c;
                    if (a.u != nullptr) {
                        stvu<double>(a.u + at, mk2<double>(f[k].u.x + gx.x, f[k].u.y + gx.y));
                        if (L.firstl) a.u[at - 1] = f[k].u0 + gx0;
                    }
                    if (a.v != nullptr) {
                        stvu<double>(a.v + at, mk2<double>(f[k].v.x + gy.x, f[k].v.y + gy.y));
                        if (L.firstl) a.v[at - 1] = f[k].v0 + gy0;
                    }
                }
            }
        }
        #pragma unroll
        for (int k = 0; k < 2 * H; ++k) s[k] = s[kGradU + k];
    }
}

void launch_divergence(const double *u, const double *v, double *out, long long Po, int N, double w,
                       int order, double *partials, double *sum, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    DivArgs a{};
    a.u = u;
    a.v = v;
    a.out = out;
    a.Po = Po;
    a.partials = sum != nullptr ? partials : nullptr;
    a.w = w;
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (order == 4) k_divergence<4><<<grid, dim3(kBlock), 0, s>>>(a);
    else k_divergence<2><<<grid, dim3(kBlock), 0, s>>>(a);
    if (sum != nullptr) launch_grad_reduce(partials, g.tiles * g.bands, sum, s);
}

void launch_grad_update(const double *phi, long long Pphi, double *u, double *v, int N, double w,
                        int order, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    UpdArgs a{};
    a.x = phi;
    a.Px = Pphi;
    a.u = u;
    a.v = v;
    a.w = w;
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (order == 4) k_grad_update<4><<<grid, dim3(kBlock), 0, s>>>(a);
    else k_grad_update<2><<<grid, dim3(kBlock), 0, s>>>(a);
}

// the two events of pgmg_project and pgmg_project_time
static int project_events(pgmg_ctx *c)
{
    if (!c->pj_ev0) HIPC(hipEventCreate(&c->pj_ev0));
    if (!c->pj_ev1) HIPC(hipEventCreate(&c->pj_ev1));
    return PGMG_OK;
}

// the divergence of (u, v) at scale -1 on c's stream between the two events, its sum of squares
// read back; out: element (0, 0) at pitch Po, or null.  Synchronous
static int project_divergence(pgmg_ctx *c, const double *u, const double *v, double *out,
                              long long Po, int order, double *norm, double *ms)
{
    const Level &L = c->lv[0];
    const int N = L.N;
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    double *const total = c->grad_buf + c->grad_cap;
    HIPC(hipEventRecord(c->pj_ev0, c->s));
    launch_divergence(u, v, out, Po, N, gradient_weight(order, -1.0, L.h), order, c->grad_buf, total,
                      c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->pj_ev1, c->s));
    double t = 0.0;
    HIPC(hipMemcpyAsync(&t, total, sizeof(double), hipMemcpyDeviceToHost, c->s));
    PGMG_TRY(stream_wait(c));
    *norm = std::sqrt(t);
    if (ms) {
        float f = 0.f;
        HIPC(hipEventElapsedTime(&f, c->pj_ev0, c->pj_ev1));
        *ms = f;
    }
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_project(pgmg_ctx *c, const pgmg_solve_opts *o, int order, int nu, double omega, double *d_u,
                 double *d_v, int measure_after, pgmg_project_info *info)
{
    const std::string who("pgmg_project");
    if (!c || !o || !d_u || !d_v || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (order != 2 && order != 4) return set_err(PGMG_ERR_ARG, who + ": order must be 2 or 4");
    if (nu < 1) return set_err(PGMG_ERR_ARG, who + ": nu must be at least 1");
    // (omega = 0, the undamped route, is refused: it stalls on a general right-hand side)
    PGMG_TRY(damp_omega_check(omega, "pgmg_project"));
    const Level &L = c->lv[0];
    const int N = c->cfg.N;
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_u, N) || !device_range(d_v, N))
        return set_err(PGMG_ERR_ARG, who + ": u and v must be device memory");
    if (ranges_overlap(d_u, bytes, d_v, bytes)) return set_err(PGMG_ERR_ARG, who + ": u and v overlap");
    {
        std::vector<const Grid *> gs{&c->S, &c->bk};
        for (const Level &l : c->lv)
            for (const Grid *g : {&l.A, &l.B, &l.F}) gs.push_back(g);
        for (const Grid *g : gs)
            if (g->base && (ranges_overlap(d_u, bytes, g->base, g->bytes) ||
                            ranges_overlap(d_v, bytes, g->base, g->bytes)))
                return set_err(PGMG_ERR_ARG, who + ": u or v overlaps a grid of the context");
    }
    if (coarsest_n(N, c->cfg.n_coarse) < 5)
        return set_err(PGMG_ERR_ARG, who + ": the coarsest level needs 5 points per side for the "
                                           "cubic interpolation (n_coarse >= 5)");
    if (order == 4) {   // pgmg_solve_extrap's rules
        if (N < 9)
            return set_err(PGMG_ERR_ARG, who + ": order 4 needs N >= 9 (a half-resolution grid of 5 "
                                               "points per side)");
        if (coarsest_n((N + 1) / 2, c->cfg.n_coarse) < 5)
            return set_err(PGMG_ERR_ARG, who + ": the coarsest level of the half-resolution grid "
                                               "needs 5 points per side (n_coarse >= 5)");
    }
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    if (c->fp32) return set_err(PGMG_ERR_STATE, who + ": fp64 contexts only");
    if (c->ext_phi)
        return set_err(PGMG_ERR_STATE, who + ": the problem is bound to the caller's arrays "
                                             "(pgmg_set_problem_device): its f is not the context's "
                                             "to write");
    if (o->monitor & PGMG_MON_ERROR)
        return set_err(PGMG_ERR_STATE, who + ": PGMG_MON_ERROR needs the analytic problem; the "
                                             "right-hand side is the divergence");
    const auto t0 = std::chrono::steady_clock::now();
    *info = pgmg_project_info{};
    info->div_after = std::numeric_limits<double>::quiet_NaN();
    PGMG_TRY(project_events(c));
    PGMG_TRY(stream_wait(c));
    // 1. f = -div(u, v), written into the level-0 f grid at its own pitch; the context's stream
    // starts after the caller's work on u and v
    PGMG_TRY(check_span(G<double>(L.F), L.P, 8, 0, N - 1, 0, N - 1, "k_divergence f"));
    PGMG_TRY(order_after_caller(c));
    PGMG_TRY(project_divergence(c, d_u, d_v, G<double>(L.F), L.P, order, &info->div_before,
                                &info->div_ms));
    PGMG_TRY(set_problem_rhs_on_device(c));
    // 2. the solve
    if (order == 4) {
        PGMG_TRY(pgmg_solve_extrap(c, o, nu, omega, &info->solve));
    } else {
        PGMG_TRY(pgmg_fmg_bc(c, nu, omega));
        PGMG_TRY(pgmg_solve_damped(c, o, omega, &info->solve.fine));
    }
    // 3. (u, v) -= grad(phi), phi where it lies now (the cross-fused cycles rotate the grids)
    PGMG_TRY(check_span(G<double>(L.A), L.P, 8, 0, N - 1, 0, N - 1, "k_grad_update phi"));
    PGMG_TRY(order_after_caller(c));
    HIPC(hipEventRecord(c->pj_ev0, c->s));
    launch_grad_update(G<double>(L.A), L.P, d_u, d_v, N, gradient_weight(order, -1.0, L.h), order, c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->pj_ev1, c->s));
    PGMG_TRY(stream_wait(c));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, c->pj_ev0, c->pj_ev1));
    info->update_ms = ms;
    // 4. what is left of the divergence
    if (measure_after)
        PGMG_TRY(project_divergence(c, d_u, d_v, nullptr, 0, order, &info->div_after, nullptr));
    info->elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

int pgmg_project_time(pgmg_ctx *c, int which, int order, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_project_time");
    if (!c || !ms_per_pass || reps <= 0 || (which != 0 && which != 1))
        return set_err(PGMG_ERR_ARG, "bad argument");
    if (order != 2 && order != 4) return set_err(PGMG_ERR_ARG, who + ": order must be 2 or 4");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    if (c->fp32) return set_err(PGMG_ERR_STATE, who + ": fp64 contexts only");
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    if (!c->pj_out) {
        if (hipMalloc((void **)&c->pj_out, 3 * elems * sizeof(double)) != hipSuccess) {
            c->pj_out = nullptr;
            return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_project_time's arrays");
        }
        register_alloc(c->pj_out, 3 * elems * sizeof(double));
        HIPC(hipMemsetAsync(c->pj_out, 0, 3 * elems * sizeof(double), c->s));
    }
    // u, v and (which 0) the divergence or (which 1) a phi of zeros: the update then leaves the
    // field as it is, pass after pass
    double *const u = c->pj_out, *const v = u + elems, *const x = v + elems;
    for (double *p : {u, v, x}) PGMG_TRY(check_span(p, N, 8, 0, N - 1, 0, N - 1, "pgmg_project_time"));
    PGMG_TRY(project_events(c));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    const double w = gradient_weight(order, 1.0, L.h);
    auto run = [&]() {
        if (which == 0) launch_divergence(u, v, x, N, N, w, order, c->grad_buf, c->grad_buf + c->grad_cap, c->s);
        else launch_grad_update(x, N, u, v, N, w, order, c->s);
    };
    if (which == 1) HIPC(hipMemsetAsync(x, 0, elems * sizeof(double), c->s));
    for (int k = 0; k < 2; ++k) run();
    HIPC(hipEventRecord(c->pj_ev0, c->s));
    for (int k = 0; k < reps; ++k) run();
    HIPC(hipEventRecord(c->pj_ev1, c->s));
    HIPC(hipGetLastError());
    HIPC(hipEventSynchronize(c->pj_ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->pj_ev0, c->pj_ev1));
    *ms_per_pass = f / reps;
    if (bytes) *bytes = (double)elems * (which == 0 ? 24.0 : 40.0);
    return PGMG_OK;
}

}  // extern "C"
