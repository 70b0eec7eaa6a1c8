// pgmg_vorticity.hip — streamfunction-vorticity flow (include/pgmg.h "Vorticity transport";
// DESIGN.md §4h): k_vort_step, k_vort_max, k_vort_wall, pgmg_vorticity_step and
// pgmg_vorticity_time (pgmg_vorticity_grid and pgmg_wall_vorticity_grid, on the caller's arrays:
// pgmg_ops.hip), and vort_advance, the time loop pgmg_vorticity_step shares with
// pgmg_vorticity_step_rk (pgmg_vort_rk.hip: the Runge-Kutta stage pass k_vort_stage).
//
// The problem the library solves, -lap(phi) = f with phi's frame as Dirichlet data, is the
// streamfunction equation: phi = psi, f = omega, u = psi_y, v = -psi_x.  One explicit Euler step
// of the vorticity transport equation is a streaming pass beside k_gradient and k_divergence
// (pgmg_gradient.hip, pgmg_project.hip), in their shape and on their decomposition grad_grid(N):
// lane t of a wave owns the column pair (1 + 2t, 2 + 2t), column 0 rides with the lane that owns
// column 1, a workgroup marches down a band of rows with a three-row window of psi and one of
// omega in registers, kGradU rows of loads in flight; the x neighbours at +-1 are the
// neighbouring lanes' values, moved by DPP (lanes 0 and 63 load the one value past their wave).
//   k_vort_step  out = omega + dt (nu lap(omega) - (psi_y omega_x - psi_x omega_y)) on the
//                interior, out's frame = omega's, word for word; 16 B read and 8 B written per
//                point.  VMAX: also the maximum of |psi_x| + |psi_y| over the workgroup's interior
//                points, one partial per workgroup, plain stores, combined by k_vort_max (NaN
//                terms are skipped, as fmax skips them; a maximum does not depend on the order).
//   k_vort_wall  the frame of omega from psi by Thom's formula (no-slip walls that move along
//                themselves), or +0.0 (free slip): O(N) work, one thread per frame index.
// Every value is formed as include/pgmg.h writes it: left to right, one rounding per operation.
#include <chrono>
#include <cmath>
#include <string>

#include "pgmg_host.h"
#include "pgmg_stop.h"
#include "pgmg_vort_dev.h"

using namespace pgmg;

namespace pgmg {

struct VortArgs {
    const double *p;    // element (0, 0) of psi, pitch Pp
    long long Pp;
    const double *w;    // element (0, 0) of omega, pitch Pw
    long long Pw;
    double *out;        // element (0, 0), pitch Po
    long long Po;
    double *partials;   // VMAX: one per workgroup
    double wgt, ih;     // 0.5 / h, 1.0 / (h * h)
    double dt, nu;
    int N;
    int band;           // rows per workgroup
};

template <bool VMAX>
__global__ __launch_bounds__(kBlock) void k_vort_step(VortArgs a)
{
    static_assert(kGradU >= 2, "the window is the tail of an iteration's rows");
    __shared__ double red[kBlock / 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N;
    const int npairs = (N - 1) >> 1;                 // pairs (1+2t, 2+2t) cover columns 1 .. N-1
    const int p0 = blockIdx.x * kBlock + wave * 64;  // the wave's first pair
    const int nw = min(max(npairs - p0, 0), 64);     // its pairs
    const int c = 1 + 2 * (p0 + lane);               // this lane's columns c, c + 1
    const bool act = lane < nw;
    const int cl = min(c, N - 2);                    // (a lane past the last pair loads the last)
    const bool firstl = p0 + lane == 0;              // owns columns 0, 1 and 2
    const bool lastl = p0 + lane == npairs - 1;      // owns columns N-2 and N-1
    const bool edge = act && (lane == 0 || lane == 63);
    const int ie = lane == 0 ? c - 1 : min(c + 2, N - 1);
    const double *__restrict__ P = a.p;
    const double *__restrict__ W = a.w;
    const long long Pp = a.Pp, Pw = a.Pw;
    const double wgt = a.wgt, ih = a.ih, dt = a.dt, nu = a.nu;
    double vm = 0.0;

    auto load = [&](const double *q) -> VRow {
        VRow v;
        v.o = ldvu<double>(q + cl);
        v.e = 0.0;
        if (edge) v.e = q[ie];
        return v;
    };
    // the values left of the pair's first column (.x) and right of its second (.y).  The moves
    // are unconditional: every lane of the wave is active here
    auto sides = [&](const VRow &ce) -> VD2 {
        const double l = dpp_shr(ce.o.y), r = dpp_shl(ce.o.x);
        return mk2<double>(lane == 0 ? ce.e : l, lane == 63 ? ce.e : r);
    };

    // (wave-uniform; a wave past the last column only joins the block maximum)
    if (nw > 0) {
        const int jb = blockIdx.y * a.band;
        const int je = min(jb + a.band, N);
        // s[0 .. 1]: the window, rows j-1 and j; s[2 ..]: this iteration's loads.  Rows are
        // clamped into the grid: a clamped row only feeds a row of the frame or one outside the
        // band, which take none of it
        VRow sp[2 + kGradU], sw[2 + kGradU];
        #pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = min(max(jb - 1 + k, 0), N - 1);
            sp[k] = load(P + r * Pp);
            sw[k] = load(W + r * Pw);
        }
        for (int j = jb; j < je; j += kGradU) {
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) {
                const int r = min(j + k + 1, N - 1);
                sp[2 + k] = load(P + r * Pp);
                sw[2 + k] = load(W + r * Pw);
            }
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) {
                const int r = j + k;   // this step's row (uniform over the workgroup)
                const VRow &pm = sp[k], &pc = sp[k + 1], &pq = sp[k + 2];
                const VRow &wm = sw[k], &wc = sw[k + 1], &wq = sw[k + 2];
                const VD2 ps = sides(pc), ws = sides(wc);
                const double pl = ps.x, pr = ps.y, wl = ws.x, wr = ws.y;
                if (r < je) {
                    VD2 o = wc.o;   // a row of the frame: omega's own words
                    if (r > 0 && r < N - 1) {
                        const double pxa = (pc.o.y - pl) * wgt, pxb = (pr - pc.o.x) * wgt;
                        const double pya = (pq.o.x - pm.o.x) * wgt, pyb = (pq.o.y - pm.o.y) * wgt;
                        const double wxa = (wc.o.y - wl) * wgt, wxb = (wr - wc.o.x) * wgt;
                        const double wya = (wq.o.x - wm.o.x) * wgt, wyb = (wq.o.y - wm.o.y) * wgt;
                        const double adva = pya * wxa - pxa * wya;
                        const double advb = pyb * wxb - pxb * wyb;
                        const double lapa = (wl + wc.o.y + wm.o.x + wq.o.x - 4.0 * wc.o.x) * ih;
                        const double lapb = (wc.o.x + wr + wm.o.y + wq.o.y - 4.0 * wc.o.y) * ih;
                        o.x = wc.o.x + dt * (nu * lapa - adva);
                        // (column N-1 is the frame)
                        o.y = lastl ? wc.o.y : wc.o.y + dt * (nu * lapb - advb);
                        if constexpr (VMAX) {
                            if (act) {
                                vm = fmax(vm, fabs(pxa) + fabs(pya));
                                if (!lastl) vm = fmax(vm, fabs(pxb) + fabs(pyb));
                            }
                        }
                    }
                    if (act) {
                        double *q = a.out + r * a.Po + c;
                        stvu<double>(q, o);
                        if (firstl) q[-1] = wc.e;   // column 0: the frame
                    }
                }
            }
            #pragma unroll
            for (int k = 0; k < 2; ++k) {
                sp[k] = sp[kGradU + k];
                sw[k] = sw[kGradU + k];
            }
        }
    }
    if constexpr (VMAX) {
        const double m = wave_max(vm);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            #pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) t = fmax(t, red[k]);
            a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

// out[0] = the maximum of the np workgroups' partials (none of them a NaN or negative)
__global__ __launch_bounds__(kBlock) void k_vort_max(const double *partials, int np, double *out)
{
    __shared__ double red[kBlock / 64];
    double m = 0.0;
    for (int k = threadIdx.x; k < np; k += kBlock) m = fmax(m, partials[k]);
    const double v = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        #pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) t = fmax(t, red[k]);
        out[0] = t;
    }
}

struct WallArgs {
    const double *p;   // element (0, 0) of psi, pitch Pp
    long long Pp;
    double *w;         // element (0, 0) of omega, pitch Pw
    long long Pw;
    double c, d;       // 2.0 * ih, 2.0 / h
    double ub, ut, vl, vr;
    int N;
    int free_slip;
};

// thread t: the frame's points (0, t), (N-1, t), (t, 0) and (t, N-1); t = 0 and N-1: the corners
__global__ __launch_bounds__(kBlock) void k_vort_wall(WallArgs a)
{
    const int N = a.N;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= N) return;
    const double *__restrict__ P = a.p;
    double *W = a.w;
    const long long Pp = a.Pp, Pw = a.Pw;
    const long long top = N - 1;
    if (a.free_slip || t == 0 || t == N - 1) {
        W[t] = 0.0;
        W[top * Pw + t] = 0.0;
        if (a.free_slip) {
            W[t * Pw] = 0.0;
            W[t * Pw + top] = 0.0;
        }
        return;
    }
    W[t] = (P[t] - P[Pp + t]) * a.c + a.ub * a.d;
    W[top * Pw + t] = (P[top * Pp + t] - P[(top - 1) * Pp + t]) * a.c - a.ut * a.d;
    W[t * Pw] = (P[t * Pp] - P[t * Pp + 1]) * a.c - a.vl * a.d;
    W[t * Pw + top] = (P[t * Pp + top] - P[t * Pp + top - 1]) * a.c + a.vr * a.d;
}

void launch_vort_step(const double *psi, long long Pp, const double *w, long long Pw, double *out,
                      long long Po, int N, double h, double dt, double nu, double *partials,
                      double *vmax, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    VortArgs a{};
    a.p = psi;
    a.Pp = Pp;
    a.w = w;
    a.Pw = Pw;
    a.out = out;
    a.Po = Po;
    a.partials = vmax != nullptr ? partials : nullptr;
    a.wgt = 0.5 / h;
    a.ih = 1.0 / (h * h);
    a.dt = dt;
    a.nu = nu;
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (vmax != nullptr) {
        k_vort_step<true><<<grid, dim3(kBlock), 0, s>>>(a);
        k_vort_max<<<dim3(1), dim3(kBlock), 0, s>>>(partials, g.tiles * g.bands, vmax);
    } else {
        k_vort_step<false><<<grid, dim3(kBlock), 0, s>>>(a);
    }
}

void launch_vort_wall(const double *psi, long long Pp, double *w, long long Pw, int N, double h,
                      int mode, const double walls[4], hipStream_t s)
{
    WallArgs a{};
    a.p = psi;
    a.Pp = Pp;
    a.w = w;
    a.Pw = Pw;
    a.c = 2.0 * (1.0 / (h * h));
    a.d = 2.0 / h;
    a.ub = walls[0];
    a.ut = walls[1];
    a.vl = walls[2];
    a.vr = walls[3];
    a.N = N;
    a.free_slip = mode == PGMG_WALL_FREE;
    k_vort_wall<<<dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(a);
}

// what the entries refuse in dt, nu, the mode and the wall speeds (nullptr: nothing)
const char *vort_step_error(double dt, double nu)
{
    if (!std::isfinite(dt) || !(dt > 0.0)) return "dt must be finite and > 0";
    if (!std::isfinite(nu) || !(nu >= 0.0)) return "nu must be finite and >= 0";
    return nullptr;
}
const char *vort_wall_error(int mode, const double walls[4])
{
    if (mode != PGMG_WALL_NOSLIP && mode != PGMG_WALL_FREE)
        return "mode must be PGMG_WALL_NOSLIP or PGMG_WALL_FREE";
    if (!walls) return "null walls";
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(walls[k])) return "a wall speed is not finite";
    return nullptr;
}

void launch_vort_max(const double *partials, int np, double *vmax, hipStream_t s)
{
    k_vort_max<<<dim3(1), dim3(kBlock), 0, s>>>(partials, np, vmax);
}

// the events of pgmg_vorticity_step and pgmg_vorticity_time
int vort_events(pgmg_ctx *c)
{
    for (hipEvent_t &e : c->vt_ev)
        if (!e) HIPC(hipEventCreate(&e));
    return PGMG_OK;
}

// what both context entries refuse after their arguments
int vort_state_check(pgmg_ctx *c, const std::string &who)
{
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    if (c->fp32) return set_err(PGMG_ERR_STATE, who + ": fp64 contexts only");
    return PGMG_OK;
}

// pgmg_vorticity_step (order 1) and pgmg_vorticity_step_rk (pgmg_vort_rk.hip): what they refuse,
// then nsteps steps of `order` stages each (include/pgmg.h "Runge-Kutta vorticity transport").
// Stage 1 is the Euler pass; order 1 runs nothing else
int vort_advance(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, double dt, double nu, int mode,
                 const double walls[4], int order, int nsteps, pgmg_vort_info *info,
                 const std::string &who)
{
    if (!c || !o || !walls || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (o->monitor & PGMG_MON_ERROR)
        return set_err(PGMG_ERR_ARG, who + ": PGMG_MON_ERROR needs the analytic problem; the "
                                           "right-hand side is the vorticity");
    PGMG_TRY(damp_omega_check(omega, who.c_str()));
    if (const char *bad = vort_step_error(dt, nu)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = vort_wall_error(mode, walls)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (nsteps < 1) return set_err(PGMG_ERR_ARG, who + ": nsteps must be at least 1");
    if (order < 1 || order > 3) return set_err(PGMG_ERR_ARG, who + ": order must be 1, 2 or 3");
    PGMG_TRY(vort_state_check(c, who));
    if (c->ext_phi)
        return set_err(PGMG_ERR_STATE, who + ": the problem is bound to the caller's arrays "
                                             "(pgmg_set_problem_device): its f is not the context's "
                                             "to write");
    const auto t0 = std::chrono::steady_clock::now();
    *info = pgmg_vort_info{};
    Level &L = c->lv[0];
    const int N = L.N;
    const double h = L.h;
    PGMG_TRY(vort_events(c));
    PGMG_TRY(stream_wait(c));
    // the scratch grid the step is written into: f's shape (the f grid's address is part of the
    // cycles' captured graphs, so the result is copied onto it instead of swapping the records)
    if (!c->vt_out.base) PGMG_TRY(alloc_grid(c->vt_out, L));
    // the grid a Runge-Kutta step keeps the omega it started from in (order > 1 only)
    if (order > 1 && !c->vt_w0.base) PGMG_TRY(alloc_grid(c->vt_w0, L));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    double *const total = c->grad_buf + c->grad_cap;
    double *const F = G<double>(L.F), *const out = G<double>(c->vt_out);
    double *const W0 = order > 1 ? G<double>(c->vt_w0) : nullptr;
    PGMG_TRY(check_span(F, L.P, 8, 0, N - 1, 0, N - 1, "k_vort_step omega"));
    PGMG_TRY(check_span(out, L.P, 8, 0, N - 1, 0, N - 1, "k_vort_step out"));
    if (W0) PGMG_TRY(check_span(W0, L.P, 8, 0, N - 1, 0, N - 1, "k_vort_stage omega0"));
    // (rows 0 .. N of a level-0 grid are one contiguous range: see pgmg_set_problem)
    const size_t bytes = (size_t)L.P * L.es * (size_t)N;
    // the Shu-Osher coefficients (a, b) of stages 2 and 3, by order (stage 1 is the Euler pass)
    const double K3 = 0x1.5555555555555p-2, B3 = 0x1.5555555555555p-1;
    const double coef[4][2][2] = {{}, {}, {{0.5, 0.5}, {}}, {{0.75, 0.25}, {K3, B3}}};
    info->worst_res = -1.0;
    double vmax = 0.0;
    for (int n = 0; n < nsteps; ++n) {
        for (int k = 0; k < order; ++k) {
            // 1. omega's frame from the current psi; 2. the stage, psi where it lies now (the
            // cross-fused cycles rotate the grids), and its copy back onto f
            const double *const psi = G<double>(L.A);
            PGMG_TRY(check_span(psi, L.P, 8, 0, N - 1, 0, N - 1, "k_vort_step psi"));
            HIPC(hipEventRecord(c->vt_ev[0], c->s));
            launch_vort_wall(psi, L.P, F, L.P, N, h, mode, walls, c->s);
            if (k == 0) {
                if (W0)
                    HIPC(hipMemcpyAsync(row_ptr(c->vt_w0, 0, L.P, L.es), row_ptr(L.F, 0, L.P, L.es),
                                        bytes, hipMemcpyDeviceToDevice, c->s));
                launch_vort_step(psi, L.P, F, L.P, out, L.P, N, h, dt, nu, c->grad_buf, total, c->s);
            } else {
                launch_vort_stage(psi, L.P, F, L.P, W0, L.P, out, L.P, N, h, dt, nu,
                                  coef[order][k - 1][0], coef[order][k - 1][1], c->grad_buf, total,
                                  c->s);
            }
            HIPC(hipGetLastError());
            HIPC(hipMemcpyAsync(row_ptr(L.F, 0, L.P, L.es), row_ptr(c->vt_out, 0, L.P, L.es), bytes,
                                hipMemcpyDeviceToDevice, c->s));
            HIPC(hipEventRecord(c->vt_ev[1], c->s));
            HIPC(hipMemcpyAsync(&vmax, total, sizeof(double), hipMemcpyDeviceToHost, c->s));
            PGMG_TRY(set_problem_rhs_on_device(c));   // (waits for the stream)
            float ms = 0.f;
            HIPC(hipEventElapsedTime(&ms, c->vt_ev[0], c->vt_ev[1]));
            info->step_ms += ms;
            // 3. the solve, warm-started from the previous psi
            PGMG_TRY(pgmg_solve_damped(c, o, omega, &info->last));
            long long sweeps = 0;
            PGMG_TRY(pgmg_stats(c, &sweeps, nullptr));
            info->cycles += info->last.cycles;
            info->sweeps += sweeps;
            info->solve_ms += info->last.elapsed_ms;
            // (a NaN residual compares false: it takes the place of any finite one, and keeps it)
            if (!(info->last.res <= info->worst_res) && !std::isnan(info->worst_res)) {
                info->worst_res = info->last.res;
                info->worst_reason = info->last.reason;
            }
        }
        info->steps = n + 1;
    }
    // the returned omega's frame belongs to the returned psi
    HIPC(hipEventRecord(c->vt_ev[0], c->s));
    launch_vort_wall(G<double>(L.A), L.P, F, L.P, N, h, mode, walls, c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->vt_ev[1], c->s));
    PGMG_TRY(stream_wait(c));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, c->vt_ev[0], c->vt_ev[1]));
    info->step_ms += ms;
    info->cfl = dt * vmax / std::fabs(h);
    info->diffusion = 4.0 * nu * dt / (h * h);
    info->elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_vorticity_step(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, double dt, double nu,
                        int mode, const double walls[4], int nsteps, pgmg_vort_info *info)
{
    return vort_advance(c, o, omega, dt, nu, mode, walls, 1, nsteps, info, "pgmg_vorticity_step");
}

int pgmg_vorticity_time(pgmg_ctx *c, int which, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_vorticity_time");
    if (!c || !ms_per_pass || reps <= 0 || (which != 0 && which != 1))
        return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(vort_state_check(c, who));
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    if (!c->vt_scr) {
        if (hipMalloc((void **)&c->vt_scr, 3 * elems * sizeof(double)) != hipSuccess) {
            c->vt_scr = nullptr;
            return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_vorticity_time's arrays");
        }
        register_alloc(c->vt_scr, 3 * elems * sizeof(double));
        HIPC(hipMemsetAsync(c->vt_scr, 0, 3 * elems * sizeof(double), c->s));
    }
    // psi, omega and out, all zero: the step then leaves omega as it is, pass after pass
    double *const p = c->vt_scr, *const w = p + elems, *const out = w + elems;
    for (double *q : {p, w, out}) PGMG_TRY(check_span(q, N, 8, 0, N - 1, 0, N - 1, "pgmg_vorticity_time"));
    PGMG_TRY(vort_events(c));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    const double dt = 0.25 * L.h * L.h;
    auto run = [&]() -> int {
        if (which == 0) {
            launch_vort_step(p, N, w, N, out, N, N, L.h, dt, 1.0, nullptr, nullptr, c->s);
            HIPC(hipMemcpyAsync(w, out, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        } else {
            launch_vort_step(p, N, w, N, out, N, N, L.h, dt, 1.0, c->grad_buf, c->grad_buf + c->grad_cap,
                             c->s);
        }
        return PGMG_OK;
    };
    for (int k = 0; k < 2; ++k) PGMG_TRY(run());
    HIPC(hipEventRecord(c->vt_ev[0], c->s));
    for (int k = 0; k < reps; ++k) PGMG_TRY(run());
    HIPC(hipEventRecord(c->vt_ev[1], c->s));
    HIPC(hipGetLastError());
    HIPC(hipEventSynchronize(c->vt_ev[1]));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->vt_ev[0], c->vt_ev[1]));
    *ms_per_pass = f / reps;
    if (bytes) *bytes = (double)elems * (which == 0 ? 40.0 : 24.0);
    return PGMG_OK;
}

}  // extern "C"
