// pgmg_boussinesq.hip — buoyancy-driven flow (include/pgmg.h "Buoyancy-driven flow"; DESIGN.md
// §4j): k_bouss_step, k_scalar_wall, pgmg_boussinesq_step and pgmg_boussinesq_time
// (pgmg_boussinesq_grid and pgmg_wall_scalar_grid, on the caller's arrays: pgmg_ops.hip), and
// bouss_advance, the time loop pgmg_boussinesq_step shares with pgmg_boussinesq_step_rk
// (pgmg_bouss_rk.hip).
//
// The vorticity transport of pgmg_vorticity.hip with a transported scalar T that feeds back:
//     w_t + u w_x + v w_y = nu lap(w) + (by T_x - bx T_y),    T_t + u T_x + v T_y = kappa lap(T).
// Both explicit Euler steps are one streaming pass in k_vort_step's shape and on its decomposition
// grad_grid(N): lane t of a wave owns the column pair (1 + 2t, 2 + 2t), column 0 rides with the
// lane that owns column 1, a workgroup marches down a band of rows with three-row windows of psi,
// w and T in registers, U rows of loads in flight; the x neighbours at +-1 are the neighbouring
// lanes' values, moved by DPP (lanes 0 and 63 load the one value past their wave).
//   k_bouss_step   wout = w + dt ((nu lap(w) - adv(w)) + (by T_x - bx T_y)) and tout = T + dt
//                  (kappa lap(T) - adv(T)) on the interior, their frames w's and T's, word for
//                  word; 24 B read and 16 B written per point.  VMAX: k_vort_step's per-workgroup
//                  maxima of |psi_x| + |psi_y|, combined by k_vort_max.
//   k_scalar_wall  the adiabatic walls of T by the second-order one-sided dT/dn = 0, in place:
//                  O(N) work, one thread per frame index; the corners are never written.
// Every value is formed as include/pgmg.h writes it: left to right, one rounding per operation.
#include <chrono>
#include <cmath>
#include <string>

#include "pgmg_host.h"
#include "pgmg_stop.h"
#include "pgmg_vort_dev.h"

using namespace pgmg;

namespace pgmg {

// rows of loads in flight per wave in k_bouss_step: with three windows kGradU = 4 rows cost
// 3 * 6 rows of registers; see DESIGN.md §4j for the register figures of both depths
constexpr int kBoussU = 4;

struct BoussArgs {
    const double *p;    // element (0, 0) of psi, pitch Pp
    long long Pp;
    const double *w;    // element (0, 0) of w, pitch Pw
    long long Pw;
    const double *t;    // element (0, 0) of T, pitch Pt
    long long Pt;
    double *wout;       // element (0, 0), pitch Pwo
    long long Pwo;
    double *tout;       // element (0, 0), pitch Pto
    long long Pto;
    double *partials;   // VMAX: one per workgroup
    double wgt, ih;     // 0.5 / h, 1.0 / (h * h)
    double dt, nu, kappa, bx, by;
    int N;
    int band;           // rows per workgroup
};

template <bool VMAX, int U>
__global__ __launch_bounds__(kBlock) void k_bouss_step(BoussArgs a)
{
    static_assert(U >= 2, "the window is the tail of an iteration's rows");
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
    const double *__restrict__ T = a.t;
    const long long Pp = a.Pp, Pw = a.Pw, Pt = a.Pt;
    const double wgt = a.wgt, ih = a.ih, dt = a.dt, nu = a.nu, kappa = a.kappa, bx = a.bx, by = a.by;
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
        VRow sp[2 + U], sw[2 + U], st[2 + U];
        #pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = min(max(jb - 1 + k, 0), N - 1);
            sp[k] = load(P + r * Pp);
            sw[k] = load(W + r * Pw);
            st[k] = load(T + r * Pt);
        }
        for (int j = jb; j < je; j += U) {
            #pragma unroll
            for (int k = 0; k < U; ++k) {
                const int r = min(j + k + 1, N - 1);
                sp[2 + k] = load(P + r * Pp);
                sw[2 + k] = load(W + r * Pw);
                st[2 + k] = load(T + r * Pt);
            }
            #pragma unroll
            for (int k = 0; k < U; ++k) {
                const int r = j + k;   // this step's row (uniform over the workgroup)
                const VRow &pm = sp[k], &pc = sp[k + 1], &pq = sp[k + 2];
                const VRow &wm = sw[k], &wc = sw[k + 1], &wq = sw[k + 2];
                const VRow &tm = st[k], &tc = st[k + 1], &tq = st[k + 2];
                const VD2 ps = sides(pc), ws = sides(wc), ts = sides(tc);
                const double pl = ps.x, pr = ps.y, wl = ws.x, wr = ws.y, tl = ts.x, tr = ts.y;
                if (r < je) {
                    VD2 ow = wc.o, ot = tc.o;   // a row of the frame: the inputs' own words
                    if (r > 0 && r < N - 1) {
                        const double pxa = (pc.o.y - pl) * wgt, pxb = (pr - pc.o.x) * wgt;
                        const double pya = (pq.o.x - pm.o.x) * wgt, pyb = (pq.o.y - pm.o.y) * wgt;
                        const double wxa = (wc.o.y - wl) * wgt, wxb = (wr - wc.o.x) * wgt;
                        const double wya = (wq.o.x - wm.o.x) * wgt, wyb = (wq.o.y - wm.o.y) * wgt;
                        const double txa = (tc.o.y - tl) * wgt, txb = (tr - tc.o.x) * wgt;
                        const double tya = (tq.o.x - tm.o.x) * wgt, tyb = (tq.o.y - tm.o.y) * wgt;
                        const double advwa = pya * wxa - pxa * wya, advwb = pyb * wxb - pxb * wyb;
                        const double advta = pya * txa - pxa * tya, advtb = pyb * txb - pxb * tyb;
                        const double lapwa = (wl + wc.o.y + wm.o.x + wq.o.x - 4.0 * wc.o.x) * ih;
                        const double lapwb = (wc.o.x + wr + wm.o.y + wq.o.y - 4.0 * wc.o.y) * ih;
                        const double lapta = (tl + tc.o.y + tm.o.x + tq.o.x - 4.0 * tc.o.x) * ih;
                        const double laptb = (tc.o.x + tr + tm.o.y + tq.o.y - 4.0 * tc.o.y) * ih;
                        const double srca = by * txa - bx * tya, srcb = by * txb - bx * tyb;
                        ow.x = wc.o.x + dt * ((nu * lapwa - advwa) + srca);
                        ot.x = tc.o.x + dt * (kappa * lapta - advta);
                        // (column N-1 is the frame)
                        ow.y = lastl ? wc.o.y : wc.o.y + dt * ((nu * lapwb - advwb) + srcb);
                        ot.y = lastl ? tc.o.y : tc.o.y + dt * (kappa * laptb - advtb);
                        if constexpr (VMAX) {
                            if (act) {
                                vm = fmax(vm, fabs(pxa) + fabs(pya));
                                if (!lastl) vm = fmax(vm, fabs(pxb) + fabs(pyb));
                            }
                        }
                    }
                    if (act) {
                        double *qw = a.wout + r * a.Pwo + c;
                        double *qt = a.tout + r * a.Pto + c;
                        stvu<double>(qw, ow);
                        stvu<double>(qt, ot);
                        if (firstl) {   // column 0: the frame
                            qw[-1] = wc.e;
                            qt[-1] = tc.e;
                        }
                    }
                }
            }
            #pragma unroll
            for (int k = 0; k < 2; ++k) {
                sp[k] = sp[U + k];
                sw[k] = sw[U + k];
                st[k] = st[U + k];
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

// thread t: the frame's points (0, t), (N-1, t), (t, 0) and (t, N-1) of T (pitch P), each written
// where its wall's bit is set; t = 0 and N-1 are the corners, which are never written.  Every value
// read lies on rows and columns 1, 2, N-3 and N-2 at an interior index t: no wall reads another
__global__ __launch_bounds__(kBlock) void k_scalar_wall(double *T, long long P, int N, unsigned mask)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t < 1 || t > N - 2) return;
    const double k3 = __longlong_as_double(0x3FD5555555555555LL);   // the double nearest 1/3
    const long long top = N - 1;
    const double b1 = T[P + t], b2 = T[2 * P + t];
    const double t1 = T[(top - 1) * P + t], t2 = T[(top - 2) * P + t];
    const double l1 = T[t * P + 1], l2 = T[t * P + 2];
    const double r1 = T[t * P + top - 1], r2 = T[t * P + top - 2];
    if (mask & PGMG_TWALL_BOTTOM) T[t] = b1 + (b1 - b2) * k3;
    if (mask & PGMG_TWALL_TOP) T[top * P + t] = t1 + (t1 - t2) * k3;
    if (mask & PGMG_TWALL_LEFT) T[t * P] = l1 + (l1 - l2) * k3;
    if (mask & PGMG_TWALL_RIGHT) T[t * P + top] = r1 + (r1 - r2) * k3;
}

void launch_bouss_step(const double *psi, long long Pp, const double *w, long long Pw, const double *T,
                       long long Pt, double *wout, long long Pwo, double *tout, long long Pto, int N,
                       double h, double dt, double nu, double kappa, const double buoy[2],
                       double *partials, double *vmax, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    BoussArgs a{};
    a.p = psi;
    a.Pp = Pp;
    a.w = w;
    a.Pw = Pw;
    a.t = T;
    a.Pt = Pt;
    a.wout = wout;
    a.Pwo = Pwo;
    a.tout = tout;
    a.Pto = Pto;
    a.partials = vmax != nullptr ? partials : nullptr;
    a.wgt = 0.5 / h;
    a.ih = 1.0 / (h * h);
    a.dt = dt;
    a.nu = nu;
    a.kappa = kappa;
    a.bx = buoy[0];
    a.by = buoy[1];
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (vmax != nullptr) {
        k_bouss_step<true, kBoussU><<<grid, dim3(kBlock), 0, s>>>(a);
        launch_vort_max(partials, g.tiles * g.bands, vmax, s);
    } else {
        k_bouss_step<false, kBoussU><<<grid, dim3(kBlock), 0, s>>>(a);
    }
}

void launch_scalar_wall(double *T, long long Pt, int N, unsigned adiabatic, hipStream_t s)
{
    if (adiabatic == 0u) return;   // nothing is written
    k_scalar_wall<<<dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(T, Pt, N, adiabatic);
}

// what the entries refuse in kappa, the buoyancy and the mask (nullptr: nothing)
const char *bouss_step_error(double kappa, const double buoy[2])
{
    if (!std::isfinite(kappa) || !(kappa >= 0.0)) return "kappa must be finite and >= 0";
    if (!buoy) return "null buoy";
    if (!std::isfinite(buoy[0]) || !std::isfinite(buoy[1])) return "a buoyancy component is not finite";
    return nullptr;
}
const char *scalar_wall_error(unsigned adiabatic)
{
    const unsigned all = PGMG_TWALL_BOTTOM | PGMG_TWALL_TOP | PGMG_TWALL_LEFT | PGMG_TWALL_RIGHT;
    if (adiabatic & ~all) return "adiabatic has a bit that is no PGMG_TWALL_*";
    return nullptr;
}

// n doubles of zeroed, registered device memory (the entries' scratch arrays)
int bouss_alloc(pgmg_ctx *c, double **q, size_t n, const char *what)
{
    if (*q) return PGMG_OK;
    if (hipMalloc((void **)q, n * sizeof(double)) != hipSuccess) {
        *q = nullptr;
        return set_err(PGMG_ERR_NOMEM, std::string("hipMalloc failed for ") + what);
    }
    register_alloc(*q, n * sizeof(double));
    HIPC(hipMemsetAsync(*q, 0, n * sizeof(double), c->s));
    return PGMG_OK;
}

// pgmg_boussinesq_step (order 1) and pgmg_boussinesq_step_rk (pgmg_bouss_rk.hip): what they
// refuse, then nsteps steps of `order` stages each (include/pgmg.h "Runge-Kutta buoyancy-driven
// flow").  Stage 1 is the Euler pass; order 1 runs nothing else
int bouss_advance(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, const pgmg_bouss_params *p,
                  double *d_T, int order, int nsteps, pgmg_bouss_info *info, const std::string &who)
{
    if (!c || !o || !p || !d_T || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (o->monitor & PGMG_MON_ERROR)
        return set_err(PGMG_ERR_ARG, who + ": PGMG_MON_ERROR needs the analytic problem; the "
                                           "right-hand side is the vorticity");
    PGMG_TRY(damp_omega_check(omega, who.c_str()));
    if (const char *bad = vort_step_error(p->dt, p->nu)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = bouss_step_error(p->kappa, p->buoy)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = vort_wall_error(p->mode, p->walls)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = scalar_wall_error(p->adiabatic)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (nsteps < 1) return set_err(PGMG_ERR_ARG, who + ": nsteps must be at least 1");
    if (order < 1 || order > 3) return set_err(PGMG_ERR_ARG, who + ": order must be 1, 2 or 3");
    if (!device_range(d_T, c->cfg.N)) return set_err(PGMG_ERR_ARG, who + ": T is not device memory");
    PGMG_TRY(vort_state_check(c, who));
    if (c->ext_phi)
        return set_err(PGMG_ERR_STATE, who + ": the problem is bound to the caller's arrays "
                                             "(pgmg_set_problem_device): its f is not the context's "
                                             "to write");
    const auto t0 = std::chrono::steady_clock::now();
    *info = pgmg_bouss_info{};
    pgmg_vort_info &fl = info->flow;
    Level &L = c->lv[0];
    const int N = L.N;
    const double h = L.h, dt = p->dt;
    const size_t elems = (size_t)N * N;
    PGMG_TRY(vort_events(c));
    PGMG_TRY(stream_wait(c));
    // the scratch grids the step is written into: f's shape for w (the f grid's address is part
    // of the cycles' captured graphs, so the result is copied onto it), dense for T
    if (!c->vt_out.base) PGMG_TRY(alloc_grid(c->vt_out, L));
    PGMG_TRY(bouss_alloc(c, &c->bq_tout, elems, "pgmg_boussinesq_step's T grid"));
    // the grids a Runge-Kutta step keeps the w and the T it started from in (order > 1 only)
    if (order > 1) {
        if (!c->vt_w0.base) PGMG_TRY(alloc_grid(c->vt_w0, L));
        PGMG_TRY(bouss_alloc(c, &c->bq_t0, elems, "pgmg_boussinesq_step_rk's saved T"));
    }
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    double *const total = c->grad_buf + c->grad_cap;
    double *const F = G<double>(L.F), *const out = G<double>(c->vt_out), *const tout = c->bq_tout;
    double *const W0 = order > 1 ? G<double>(c->vt_w0) : nullptr, *const T0 = order > 1 ? c->bq_t0 : nullptr;
    PGMG_TRY(check_span(F, L.P, 8, 0, N - 1, 0, N - 1, "k_bouss_step w"));
    PGMG_TRY(check_span(out, L.P, 8, 0, N - 1, 0, N - 1, "k_bouss_step wout"));
    PGMG_TRY(check_span(tout, N, 8, 0, N - 1, 0, N - 1, "k_bouss_step tout"));
    if (W0) {
        PGMG_TRY(check_span(W0, L.P, 8, 0, N - 1, 0, N - 1, "k_bouss_stage w0"));
        PGMG_TRY(check_span(T0, N, 8, 0, N - 1, 0, N - 1, "k_bouss_stage T0"));
    }
    // (rows 0 .. N of a level-0 grid are one contiguous range: see pgmg_set_problem)
    const size_t bytes = (size_t)L.P * L.es * (size_t)N;
    // the context's stream starts after the caller's work on T
    PGMG_TRY(order_after_caller(c));
    // the Shu-Osher coefficients (a, b) of stages 2 and 3, by order (stage 1 is the Euler pass)
    const double K3 = 0x1.5555555555555p-2, B3 = 0x1.5555555555555p-1;
    const double coef[4][2][2] = {{}, {}, {{0.5, 0.5}, {}}, {{0.75, 0.25}, {K3, B3}}};
    fl.worst_res = -1.0;
    double vmax = 0.0;
    for (int n = 0; n < nsteps; ++n) {
        for (int k = 0; k < order; ++k) {
            // 1. w's frame from the current psi and T's adiabatic walls; 2. the stage, psi where
            // it lies now (the cross-fused cycles rotate the grids), and its copies back onto f
            // and T
            const double *const psi = G<double>(L.A);
            PGMG_TRY(check_span(psi, L.P, 8, 0, N - 1, 0, N - 1, "k_bouss_step psi"));
            HIPC(hipEventRecord(c->vt_ev[0], c->s));
            launch_vort_wall(psi, L.P, F, L.P, N, h, p->mode, p->walls, c->s);
            launch_scalar_wall(d_T, N, N, p->adiabatic, c->s);
            if (k == 0) {
                if (W0) {
                    HIPC(hipMemcpyAsync(row_ptr(c->vt_w0, 0, L.P, L.es), row_ptr(L.F, 0, L.P, L.es),
                                        bytes, hipMemcpyDeviceToDevice, c->s));
                    HIPC(hipMemcpyAsync(T0, d_T, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
                }
                launch_bouss_step(psi, L.P, F, L.P, d_T, N, out, L.P, tout, N, N, h, dt, p->nu,
                                  p->kappa, p->buoy, c->grad_buf, total, c->s);
            } else {
                launch_bouss_stage(psi, L.P, F, L.P, d_T, N, W0, L.P, T0, N, out, L.P, tout, N, N, h,
                                   dt, p->nu, p->kappa, p->buoy, coef[order][k - 1][0],
                                   coef[order][k - 1][1], c->grad_buf, total, c->s);
            }
            HIPC(hipGetLastError());
            HIPC(hipMemcpyAsync(row_ptr(L.F, 0, L.P, L.es), row_ptr(c->vt_out, 0, L.P, L.es), bytes,
                                hipMemcpyDeviceToDevice, c->s));
            HIPC(hipMemcpyAsync(d_T, tout, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
            HIPC(hipEventRecord(c->vt_ev[1], c->s));
            HIPC(hipMemcpyAsync(&vmax, total, sizeof(double), hipMemcpyDeviceToHost, c->s));
            PGMG_TRY(set_problem_rhs_on_device(c));   // (waits for the stream)
            float ms = 0.f;
            HIPC(hipEventElapsedTime(&ms, c->vt_ev[0], c->vt_ev[1]));
            fl.step_ms += ms;
            // 3. the solve, warm-started from the previous psi
            PGMG_TRY(pgmg_solve_damped(c, o, omega, &fl.last));
            long long sweeps = 0;
            PGMG_TRY(pgmg_stats(c, &sweeps, nullptr));
            fl.cycles += fl.last.cycles;
            fl.sweeps += sweeps;
            fl.solve_ms += fl.last.elapsed_ms;
            // (a NaN residual compares false: it takes the place of any finite one, and keeps it)
            if (!(fl.last.res <= fl.worst_res) && !std::isnan(fl.worst_res)) {
                fl.worst_res = fl.last.res;
                fl.worst_reason = fl.last.reason;
            }
        }
        fl.steps = n + 1;
    }
    // the returned frames belong to the returned psi and T
    HIPC(hipEventRecord(c->vt_ev[0], c->s));
    launch_vort_wall(G<double>(L.A), L.P, F, L.P, N, h, p->mode, p->walls, c->s);
    launch_scalar_wall(d_T, N, N, p->adiabatic, c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->vt_ev[1], c->s));
    PGMG_TRY(stream_wait(c));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, c->vt_ev[0], c->vt_ev[1]));
    fl.step_ms += ms;
    fl.cfl = dt * vmax / std::fabs(h);
    fl.diffusion = 4.0 * p->nu * dt / (h * h);
    info->diffusion_t = 4.0 * p->kappa * dt / (h * h);
    fl.elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_boussinesq_step(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, const pgmg_bouss_params *p,
                         double *d_T, int nsteps, pgmg_bouss_info *info)
{
    return bouss_advance(c, o, omega, p, d_T, 1, nsteps, info, "pgmg_boussinesq_step");
}

int pgmg_boussinesq_time(pgmg_ctx *c, int which, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_boussinesq_time");
    if (!c || !ms_per_pass || reps <= 0 || (which != 0 && which != 1))
        return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(vort_state_check(c, who));
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    PGMG_TRY(bouss_alloc(c, &c->bq_scr, 5 * elems, "pgmg_boussinesq_time's arrays"));
    // psi, w, T and the two outputs, all zero: the step then leaves w and T as they are
    double *const p = c->bq_scr, *const w = p + elems, *const T = w + elems, *const wout = T + elems,
                 *const tout = wout + elems;
    for (double *q : {p, w, T, wout, tout})
        PGMG_TRY(check_span(q, N, 8, 0, N - 1, 0, N - 1, "pgmg_boussinesq_time"));
    PGMG_TRY(vort_events(c));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    const double dt = 0.25 * L.h * L.h;
    const double buoy[2] = {0.0, 1.0};
    auto run = [&]() -> int {
        if (which == 0) {
            launch_bouss_step(p, N, w, N, T, N, wout, N, tout, N, N, L.h, dt, 1.0, 1.0, buoy, nullptr,
                              nullptr, c->s);
            HIPC(hipMemcpyAsync(w, wout, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
            HIPC(hipMemcpyAsync(T, tout, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        } else {
            launch_bouss_step(p, N, w, N, T, N, wout, N, tout, N, N, L.h, dt, 1.0, 1.0, buoy,
                              c->grad_buf, c->grad_buf + c->grad_cap, c->s);
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
    if (bytes) *bytes = (double)elems * (which == 0 ? 72.0 : 40.0);
    return PGMG_OK;
}

}  // extern "C"
