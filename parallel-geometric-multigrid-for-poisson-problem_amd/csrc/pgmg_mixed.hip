// pgmg_mixed.hip — mixed-precision iterative refinement (include/pgmg.h "Mixed-precision
// refinement"): the two streaming passes k_defect and k_correct, the fp32 context
// an fp64 context owns, pgmg_solve_mixed and pgmg_mixed_time (pgmg_defect_grid and
// pgmg_correct_grid, on the caller's arrays: pgmg_ops.hip).
//
// The iterate and its residual stay in fp64; the correction equation A e = r is solved by the
// existing pgmg_fmg_damped on an fp32 context, whose right-hand side is the residual scaled by a
// power of two into fp32's range and whose solution is added back unscaled.
//   k_defect   the monitor's residual pass (pgmg_monitor.hip, k_monitor with kMonRes: its
//              decomposition, loads, expression and sums) in double that also stores
//              g = (float)(r * s).  g is another array, so nothing is deferred and no barrier is
//              needed; a wave past the last column only joins the block sum.
//   k_correct  x += (double)e * t, pointwise on the interior, on pgmg_gradient's decomposition.
#include <chrono>
#include <cmath>
#include <limits>
#include <string>

#include "pgmg_host.h"
#include "pgmg_stop.h"

using namespace pgmg;

namespace pgmg {

constexpr int kCorU = 4;   // rows of loads in flight per wave of k_correct

struct DefectArgs {
    const double *x;     // element (0, 0) of phi, pitch Px
    const double *f;     // element (0, 0) of f, pitch Pf
    float *g;            // element (0, 0) of the scaled residual, pitch Pg
    long long Px, Pf, Pg;
    double *partials;    // 3 per workgroup (the monitor's layout): sum r^2, 0, 0
    double ih, s;
    int N;
};

// Lane t of a wave owns the column pair (cw + 2t, cw + 2t + 1), a workgroup a tile of kMonTile
// columns from column 1 (column 0 rides with the lane that owns column 1) and a band of kMonBand
// rows from row 0, a three-row window of x in registers, kMonU rows loaded before any is used,
// the horizontal neighbours by DPP -- k_monitor's march.  Every row of the band is stored: the
// frame rows and columns as +0, the last pair's second column (N - 1) with them.
__global__ __launch_bounds__(kBlock) void k_defect(DefectArgs a)
{
    __shared__ double red[kBlock / 64];
    using D2 = V2<double>;
    const int lane = threadIdx.x & 63;
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
    const int jb = blockIdx.y * kMonBand;
    const int je = min(jb + kMonBand, N);
    const long long Px = a.Px, Pf = a.Pf, Pg = a.Pg;
    const double *__restrict__ X = a.x;
    const double *__restrict__ F = a.f;
    float *__restrict__ Gp = a.g;
    const double ih = a.ih, s = a.s;
    double accr = 0.0;

    if (nw > 0) {   // (wave-uniform)
        // rows are clamped into the grid: a clamped row only feeds the residual of a frame row,
        // which is neither summed nor stored
        auto rowx = [&](int r) -> D2 {
            r = min(max(r, 0), N - 1);
            return buf_row<double, 0>(X + r * Px + cw, nw, lane);
        };
        D2 w0 = rowx(jb - 1), w1 = rowx(jb);
        for (int j = jb; j < je; j += kMonU) {
            D2 xn[kMonU], fv[kMonU];
            double el[kMonU], er[kMonU];
            #pragma unroll
            for (int u = 0; u < kMonU; ++u) {
                const int r = min(j + u, je - 1);
                xn[u] = rowx(r + 1);
                fv[u] = buf_row<double, 0>(F + r * Pf + cw, nw, lane);
                el[u] = 0.0;
                er[u] = 0.0;
                if (lane == 0) el[u] = X[r * Px + cw - 1];
                if (lane == 63 && has_right) er[u] = X[r * Px + cw + 128];
            }
            #pragma unroll
            for (int u = 0; u < kMonU; ++u) {
                const int r = j + u;
                const D2 up = (u == 0) ? w0 : (u == 1 ? w1 : xn[u - 2]);
                const D2 ce = (u == 0) ? w1 : xn[u - 1];
                const D2 dn = xn[u];
                double left = dpp_shr(ce.y);
                double right = dpp_shl(ce.x);
                if (lane == 0) left = el[u];
                if (lane == 63) right = er[u];
                const D2 fr = fv[u];
                const double r0 = fr.x - ih * (4.0 * ce.x - left - ce.y - up.x - dn.x);
                const double r1 = fr.y - ih * (4.0 * ce.y - ce.x - right - up.y - dn.y);
                if (act && r < je) {
                    float2 o = mk2<float>(0.0f, 0.0f);
                    if (r >= 1 && r < N - 1) {
                        accr += sq(r0);
                        o.x = (float)(r0 * s);
                        if (second) {
                            accr += sq(r1);
                            o.y = (float)(r1 * s);
                        }
                    }
                    float *q = Gp + r * Pg + c;
                    stvu<float>(q, o);
                    if (c == 1) q[-1] = 0.0f;
                }
            }
            w0 = xn[kMonU - 2];
            w1 = xn[kMonU - 1];
        }
    }
    const double sr = wave_sum(accr);
    if (lane == 0) red[wave] = sr;
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        if (threadIdx.x == 0) {
            #pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) t += red[w];
        }
        a.partials[3 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = t;
    }
}

struct CorrectArgs {
    double *x;         // element (0, 0), pitch Px
    const float *e;    // element (0, 0), pitch Pe
    long long Px, Pe;
    double t;
    int N;
    int band;          // rows per workgroup
};

// x(y, x) += (double)e(y, x) * t on 1 <= y, x <= N - 2: a lane owns the column pair (1 + 2p,
// 2 + 2p), read with one 8-byte load of e and one 16-byte load of x (element-aligned) and
// written with one store; the lane that owns column N - 2 stores it alone (column N - 1 is
// loaded, never stored).  A point is read and written by its owner only: safe in place.
__global__ __launch_bounds__(kBlock) void k_correct(CorrectArgs a)
{
    const int N = a.N;
    const int c = 1 + 2 * (blockIdx.x * kBlock + threadIdx.x);
    if (c > N - 2) return;
    const bool second = c + 1 <= N - 2;
    const int jb = 1 + blockIdx.y * a.band;
    const int je = min(jb + a.band, N - 1);   // rows jb .. je-1 (at most N-2)
    const float *__restrict__ E = a.e;
    double *X = a.x;
    const long long Px = a.Px, Pe = a.Pe;
    const double t = a.t;
    for (int j = jb; j < je; j += kCorU) {
        V2<float> ev[kCorU];
        V2<double> cur[kCorU];
        #pragma unroll
        for (int u = 0; u < kCorU; ++u) {
            const int r = min(j + u, je - 1);
            ev[u] = ldvu<float>(E + r * Pe + c);
            cur[u] = ldvu<double>(X + r * Px + c);
        }
        #pragma unroll
        for (int u = 0; u < kCorU; ++u) {
            const int r = j + u;
            if (r < je) {
                double *p = X + r * Px + c;
                const double o0 = cur[u].x + (double)ev[u].x * t;
                const double o1 = cur[u].y + (double)ev[u].y * t;
                if (second) stvu<double>(p, mk2<double>(o0, o1));
                else p[0] = o0;
            }
        }
    }
}

void launch_defect(const double *x, long long Px, const double *f, long long Pf, float *g,
                   long long Pg, int N, double ih, double scale, double *partials, double *sums,
                   hipStream_t s)
{
    DefectArgs a{};
    a.x = x;
    a.f = f;
    a.g = g;
    a.Px = Px;
    a.Pf = Pf;
    a.Pg = Pg;
    a.partials = partials;
    a.ih = ih;
    a.s = scale;
    a.N = N;
    // the monitor's grid of a whole level: tiles of kMonTile columns from column 1, bands of
    // kMonBand rows from row 0 (damp_grid_blocks(N) workgroups)
    const dim3 g2((N - 1 + kMonTile - 1) / kMonTile, (N + kMonBand - 1) / kMonBand);
    k_defect<<<g2, dim3(kBlock), 0, s>>>(a);
    if (sums != nullptr) launch_mon_reduce(partials, (int)(g2.x * g2.y), sums, s);
}

void launch_correct(double *x, long long Px, const float *e, long long Pe, int N, double t,
                    hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    CorrectArgs a{};
    a.x = x;
    a.e = e;
    a.Px = Px;
    a.Pe = Pe;
    a.t = t;
    a.N = N;
    a.band = g.band;
    k_correct<<<dim3(g.tiles, (N - 2 + g.band - 1) / g.band), dim3(kBlock), 0, s>>>(a);
}

bool device_range_f32(const float *p, int N)
{
    return is_device_ptr(p) && is_device_ptr(p + (size_t)N * N - 1);
}

// s of step (a): 2^(-ilogb(rho / (N - 2))), the exponent clamped so that s and 1 / s are normal
static double mixed_scale(double rho, int N)
{
    const double q = rho / (N - 2);
    if (q == 0.0 || !std::isfinite(q)) return 1.0;
    int e = std::ilogb(q);
    e = e < -1022 ? -1022 : (e > 1022 ? 1022 : e);
    return std::ldexp(1.0, -e);
}

// the fp32 context and the six events, made on the first call
static int mixed_setup(pgmg_ctx *c)
{
    if (!c->mx_child) {
        pgmg_config cfg = c->cfg;
        cfg.precision = PGMG_PRECISION_FP32;
        cfg.eps = -1.0;
        cfg.flags &= ~PGMG_FLAG_FAST;
        cfg.rank = 0;
        cfg.world = 1;
        cfg.nccl_unique_id = nullptr;
        PGMG_TRY(pgmg_create(&c->mx_child, &cfg));
        if (c->mx_child->lv[0].h != c->lv[0].h) {
            pgmg_destroy(c->mx_child);
            c->mx_child = nullptr;
            return set_err(PGMG_ERR_STATE, "pgmg_solve_mixed: the fp32 context's mesh width is not "
                                           "the context's");
        }
    }
    for (hipEvent_t &e : c->mx_ev)
        if (!e) HIPC(hipEventCreate(&e));
    return PGMG_OK;
}

// what pgmg_solve_mixed and pgmg_mixed_time refuse in the context
static int mixed_ctx_check(pgmg_ctx *c, const std::string &who)
{
    if (coarsest_n(c->cfg.N, c->cfg.n_coarse) < 5)
        return set_err(PGMG_ERR_ARG, who + ": the coarsest level needs 5 points per side for the "
                                           "cubic interpolation (n_coarse >= 5)");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    if (c->fp32)
        return set_err(PGMG_ERR_STATE, who + ": fp64 contexts only: the iterate and its residual "
                                             "are fp64, the fp32 context is the one it owns");
    return PGMG_OK;
}

// phi and the stored f where they lie now, span-checked where they are the library's
struct MixedGrids {
    double *x;
    const double *f;
    long long Px, Pf;
};
static int mixed_grids(pgmg_ctx *c, MixedGrids *m)
{
    const Level &L = c->lv[0];
    const int N = L.N;
    m->x = c->ext_phi ? c->ext_phi : G<double>(L.A);
    m->Px = c->ext_phi ? N : L.P;
    m->f = c->ext_f ? c->ext_f : G<double>(L.F);
    m->Pf = c->ext_f ? N : L.P;
    if (!c->ext_phi) PGMG_TRY(check_span(m->x, m->Px, 8, 0, N - 1, 0, N - 1, "pgmg_solve_mixed phi"));
    if (!c->ext_f) PGMG_TRY(check_span(m->f, m->Pf, 8, 0, N - 1, 0, N - 1, "pgmg_solve_mixed f"));
    return PGMG_OK;
}

static int mixed_elapsed(hipEvent_t e0, hipEvent_t e1, double *acc)
{
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, e0, e1));
    *acc += ms;
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_solve_mixed(pgmg_ctx *c, const pgmg_solve_opts *o, int nu, double omega,
                     pgmg_mixed_info *info)
{
    const std::string who("pgmg_solve_mixed");
    if (!c || !o || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (o->check_every != 1) return set_err(PGMG_ERR_ARG, who + ": check_every must be 1");
    if (o->cycle != PGMG_CYCLE_V) return set_err(PGMG_ERR_ARG, who + ": the cycle must be PGMG_CYCLE_V");
    if (o->monitor & PGMG_MON_ERROR)
        return set_err(PGMG_ERR_ARG, who + ": PGMG_MON_ERROR is not recorded; call pgmg_monitor "
                                           "afterwards");
    if (nu < 1) return set_err(PGMG_ERR_ARG, who + ": nu must be at least 1");
    PGMG_TRY(damp_omega_check(omega, "pgmg_solve_mixed"));
    PGMG_TRY(mixed_ctx_check(c, who));
    const auto t0 = std::chrono::steady_clock::now();
    *info = pgmg_mixed_info{};
    info->solve.rel_error = std::numeric_limits<double>::quiet_NaN();
    PGMG_TRY(mixed_setup(c));
    pgmg_ctx *ch = c->mx_child;
    PGMG_TRY(stream_wait(ch));
    const Level &L = c->lv[0];
    const int N = L.N;
    const int np = damp_grid_blocks(N);
    hipEvent_t *ev = c->mx_ev;
    // rho_0 (the monitor also sizes the partial sums and, device-bound, orders the stream)
    pgmg_monitor_out m0{};
    PGMG_TRY(pgmg_monitor(c, PGMG_MON_RESIDUAL, &m0));
    PGMG_TRY(mon_reserve(c, np, 0));
    MixedGrids mg{};
    PGMG_TRY(mixed_grids(c, &mg));
    // an entry that changes phi
    c->carry = false;
    c->hist.reset(c->nb);
    c->solve_hist.clear();
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    StopState st;
    double rho = m0.res_norm;
    int steps = 0;
    bool pending = false;   // a step's child solve and correction have not been accounted yet
    for (;;) {
        // a. the defect into the child's f grid, and its norm
        const double s = mixed_scale(rho, N);
        const Level &Lc = ch->lv[0];
        PGMG_TRY(check_span(G<float>(Lc.F), Lc.P, 4, 0, N - 1, 0, N - 1, "k_defect g"));
        double *const sums = c->mon_buf + 3 * (size_t)c->mon_cap;
        HIPC(hipEventRecord(ev[0], c->s));
        launch_defect(mg.x, mg.Px, mg.f, mg.Pf, G<float>(Lc.F), Lc.P, N, L.ih, s, c->mon_buf, sums, c->s);
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(ev[1], c->s));
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, sums, sizeof(double), hipMemcpyDeviceToHost, c->s));
        PGMG_TRY(stream_wait(c));
        const double r = std::sqrt(t);
        PGMG_TRY(mixed_elapsed(ev[0], ev[1], &info->defect_ms));
        if (pending) {   // the last step is complete: this pass ran after its correction
            long long sw = 0;
            PGMG_TRY(pgmg_stats(ch, &sw, nullptr));
            info->inner_sweeps += sw;
            PGMG_TRY(mixed_elapsed(ev[2], ev[3], &info->inner_ms));
            PGMG_TRY(mixed_elapsed(ev[4], ev[5], &info->correct_ms));
            pending = false;
        }
        // b. the rule
        c->solve_hist.push_back({steps, r, std::numeric_limits<double>::quiet_NaN()});
        int next = 0;
        const int reason = stop_check(*o, st, steps, r, &next);
        info->solve.cycles = steps;
        info->solve.checks = st.checks;
        info->solve.res0 = st.r0;
        info->solve.res = r;
        if (reason) {
            info->solve.reason = reason;
            break;
        }
        // c. the child's problem and its solve, on the child's stream (idle: the host has waited
        // for the defect, which ran after the last correction, which waited for the child)
        PGMG_TRY(set_problem_zero_rhs_on_device_f32(ch));
        HIPC(hipEventRecord(ev[2], ch->s));
        PGMG_TRY(pgmg_fmg_damped(ch, nu, omega));
        HIPC(hipEventRecord(ev[3], ch->s));
        // d. the correction, after the child (its phi where it lies after the solve)
        const Level &Ld = ch->lv[0];
        PGMG_TRY(check_span(G<float>(Ld.A), Ld.P, 4, 0, N - 1, 0, N - 1, "k_correct e"));
        HIPC(hipStreamWaitEvent(c->s, ev[3], 0));
        HIPC(hipEventRecord(ev[4], c->s));
        launch_correct(mg.x, mg.Px, G<float>(Ld.A), Ld.P, N, 1.0 / s, c->s);
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(ev[5], c->s));
        pending = true;
        steps += next;
        rho = r;
    }
    info->solve.elapsed_ms = info->elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

int pgmg_mixed_time(pgmg_ctx *c, int which, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_mixed_time");
    if (!c || !ms_per_pass || reps <= 0 || (which != 0 && which != 1))
        return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(mixed_ctx_check(c, who));
    PGMG_TRY(mixed_setup(c));
    pgmg_ctx *ch = c->mx_child;
    PGMG_TRY(stream_wait(ch));
    const Level &L = c->lv[0], &Lc = ch->lv[0];
    const int N = L.N;
    PGMG_TRY(mon_reserve(c, damp_grid_blocks(N), 0));
    MixedGrids mg{};
    PGMG_TRY(mixed_grids(c, &mg));
    PGMG_TRY(check_span(G<float>(Lc.F), Lc.P, 4, 0, N - 1, 0, N - 1, "k_defect g"));
    PGMG_TRY(check_span(G<float>(Lc.A), Lc.P, 4, 0, N - 1, 0, N - 1, "k_correct e"));
    if (which == 1) {   // phi is changed
        c->carry = false;
        c->hist.reset(c->nb);
    }
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    auto run = [&]() {
        if (which == 0)
            launch_defect(mg.x, mg.Px, mg.f, mg.Pf, G<float>(Lc.F), Lc.P, N, L.ih, 1.0, c->mon_buf,
                          c->mon_buf + 3 * (size_t)c->mon_cap, c->s);
        else
            launch_correct(mg.x, mg.Px, G<float>(Lc.A), Lc.P, N, 1.0, c->s);
    };
    for (int k = 0; k < 2; ++k) run();
    HIPC(hipEventRecord(c->mx_ev[0], c->s));
    for (int k = 0; k < reps; ++k) run();
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->mx_ev[1], c->s));
    HIPC(hipEventSynchronize(c->mx_ev[1]));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->mx_ev[0], c->mx_ev[1]));
    *ms_per_pass = f / reps;
    if (bytes) *bytes = (double)N * N * 20.0;
    return PGMG_OK;
}

}  // extern "C"
