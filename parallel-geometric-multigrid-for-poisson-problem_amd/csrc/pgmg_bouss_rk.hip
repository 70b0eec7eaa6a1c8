// pgmg_bouss_rk.hip — strong-stability-preserving Runge-Kutta time stepping of the buoyancy-driven
// flow (include/pgmg.h "Runge-Kutta buoyancy-driven flow"; DESIGN.md §4j "Runge-Kutta"):
// k_bouss_stage, pgmg_boussinesq_step_rk and pgmg_boussinesq_rk_time (pgmg_boussinesq_stage_grid,
// on the caller's arrays: pgmg_ops.hip; the time loop itself is bouss_advance,
// pgmg_boussinesq.hip).
//
// In Shu-Osher form every stage after the first is a convex combination of the fields the step
// started from, W0 and T0, and the explicit Euler steps EW and ET of the current w and T under
// the current psi:
//   k_bouss_stage  wout = a * W0 + b * EW and tout = a * T0 + b * ET on the interior, their frames
//                  w's and T's, word for word.  k_bouss_step's pass (pgmg_boussinesq.hip) on its
//                  decomposition grad_grid(N), with two more input streams: of W0 and T0 a lane
//                  reads its own column pair of the current row and nothing else, one unaligned
//                  vector load each per row issued with the windows' U rows of loads -- no window,
//                  no DPP, no edge load.  40 B read and 16 B written per point.  ew and et are
//                  formed by k_bouss_step's expressions, then a * W0, b * ew and their sum, one
//                  rounding each (the same for T).  VMAX as in k_bouss_step.
// Stage 1 of every order is k_bouss_step itself, not this pass with (a, b) = (0, 1).
#include <cmath>
#include <string>

#include "pgmg_host.h"
#include "pgmg_vort_dev.h"

using namespace pgmg;

namespace pgmg {

// rows of loads in flight per wave in k_bouss_stage: the depth the entries launch, and the other
// depth that is built beside it for pgmg_boussinesq_rk_time's comparison (DESIGN.md §4j has the
// registers and the times of both).  With vmax, which the time loop always takes, four rows cost
// 172 VGPRs and leave two waves per SIMD; two rows cost 116 and leave four
constexpr int kBoussStageU = 2;
constexpr int kBoussStageAltU = 4;

struct BoussStageArgs {
    const double *p;    // element (0, 0) of psi, pitch Pp
    long long Pp;
    const double *w;    // element (0, 0) of w, pitch Pw
    long long Pw;
    const double *t;    // element (0, 0) of T, pitch Pt
    long long Pt;
    const double *w0;   // element (0, 0) of the saved w, pitch Pw0
    long long Pw0;
    const double *t0;   // element (0, 0) of the saved T, pitch Pt0
    long long Pt0;
    double *wout;       // element (0, 0), pitch Pwo
    long long Pwo;
    double *tout;       // element (0, 0), pitch Pto
    long long Pto;
    double *partials;   // VMAX: one per workgroup
    double wgt, ih;     // 0.5 / h, 1.0 / (h * h)
    double dt, nu, kappa, bx, by;
    double a, b;        // wout = a * w0 + b * ew, tout = a * t0 + b * et
    int N;
    int band;           // rows per workgroup
};

template <bool VMAX, int U>
__global__ __launch_bounds__(kBlock) void k_bouss_stage(BoussStageArgs a)
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
    const double *W = a.w;     // (W0 may be W and T0 may be T: none of them is written)
    const double *T = a.t;
    const double *W0 = a.w0;
    const double *T0 = a.t0;
    const long long Pp = a.Pp, Pw = a.Pw, Pt = a.Pt, Pw0 = a.Pw0, Pt0 = a.Pt0;
    const double wgt = a.wgt, ih = a.ih, dt = a.dt, nu = a.nu, kappa = a.kappa, bx = a.bx, by = a.by;
    const double ca = a.a, cb = a.b;
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
            // s0w[k], s0t[k]: W0's and T0's pairs of row j + k, the row computed at step k.
            // Clamped into the interior rows: the frames of W0 and T0 have no part in any value
            VD2 s0w[U], s0t[U];
            #pragma unroll
            for (int k = 0; k < U; ++k) {
                const int r = min(j + k + 1, N - 1);
                sp[2 + k] = load(P + r * Pp);
                sw[2 + k] = load(W + r * Pw);
                st[2 + k] = load(T + r * Pt);
                const int r0 = min(max(j + k, 1), N - 2);
                s0w[k] = ldvu<double>(W0 + r0 * Pw0 + cl);
                s0t[k] = ldvu<double>(T0 + r0 * Pt0 + cl);
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
                        const double ewa = wc.o.x + dt * ((nu * lapwa - advwa) + srca);
                        const double eta = tc.o.x + dt * (kappa * lapta - advta);
                        const double ewb = wc.o.y + dt * ((nu * lapwb - advwb) + srcb);
                        const double etb = tc.o.y + dt * (kappa * laptb - advtb);
                        ow.x = ca * s0w[k].x + cb * ewa;
                        ot.x = ca * s0t[k].x + cb * eta;
                        // (column N-1 is the frame)
                        ow.y = lastl ? wc.o.y : ca * s0w[k].y + cb * ewb;
                        ot.y = lastl ? tc.o.y : ca * s0t[k].y + cb * etb;
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

// the launch at U rows in flight
template <int U>
static void launch_bouss_stage_u(const BoussStageArgs &a, const GradGrid &g, double *vmax, hipStream_t s)
{
    const dim3 grid(g.tiles, g.bands);
    if (vmax != nullptr) {
        k_bouss_stage<true, U><<<grid, dim3(kBlock), 0, s>>>(a);
        launch_vort_max(a.partials, g.tiles * g.bands, vmax, s);
    } else {
        k_bouss_stage<false, U><<<grid, dim3(kBlock), 0, s>>>(a);
    }
}

// depth: 0 the entries' depth kBoussStageU, 1 the other built depth (the timing entry only)
static void launch_bouss_stage_depth(int depth, const double *psi, long long Pp, const double *w,
                                     long long Pw, const double *T, long long Pt, const double *w0,
                                     long long Pw0, const double *T0, long long Pt0, double *wout,
                                     long long Pwo, double *tout, long long Pto, int N, double h,
                                     double dt, double nu, double kappa, const double buoy[2],
                                     double ca, double cb, double *partials, double *vmax, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    BoussStageArgs a{};
    a.p = psi;
    a.Pp = Pp;
    a.w = w;
    a.Pw = Pw;
    a.t = T;
    a.Pt = Pt;
    a.w0 = w0;
    a.Pw0 = Pw0;
    a.t0 = T0;
    a.Pt0 = Pt0;
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
    a.a = ca;
    a.b = cb;
    a.N = N;
    a.band = g.band;
    if (depth == 0)
        launch_bouss_stage_u<kBoussStageU>(a, g, vmax, s);
    else
        launch_bouss_stage_u<kBoussStageAltU>(a, g, vmax, s);
}

void launch_bouss_stage(const double *psi, long long Pp, const double *w, long long Pw, const double *T,
                        long long Pt, const double *w0, long long Pw0, const double *T0, long long Pt0,
                        double *wout, long long Pwo, double *tout, long long Pto, int N, double h,
                        double dt, double nu, double kappa, const double buoy[2], double ca, double cb,
                        double *partials, double *vmax, hipStream_t s)
{
    launch_bouss_stage_depth(0, psi, Pp, w, Pw, T, Pt, w0, Pw0, T0, Pt0, wout, Pwo, tout, Pto, N, h, dt,
                             nu, kappa, buoy, ca, cb, partials, vmax, s);
}

}  // namespace pgmg

extern "C" {

int pgmg_boussinesq_step_rk(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, const pgmg_bouss_params *p,
                            double *d_T, int order, int nsteps, pgmg_bouss_info *info)
{
    return bouss_advance(c, o, omega, p, d_T, order, nsteps, info, "pgmg_boussinesq_step_rk");
}

int pgmg_boussinesq_rk_time(pgmg_ctx *c, int which, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_boussinesq_rk_time");
    // (which = 2 and 3: 0 and 1 at the other built depth, kBoussStageAltU)
    if (!c || !ms_per_pass || reps <= 0 || which < 0 || which > 3)
        return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(vort_state_check(c, who));
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    PGMG_TRY(bouss_alloc(c, &c->bq_rk_scr, 7 * elems, "pgmg_boussinesq_rk_time's arrays"));
    // psi, w, T, the saved w and T and the two outputs, all zero: the stage then leaves w and T
    // as they are, pass after pass
    double *const p = c->bq_rk_scr, *const w = p + elems, *const T = w + elems, *const w0 = T + elems,
                 *const T0 = w0 + elems, *const wout = T0 + elems, *const tout = wout + elems;
    for (double *q : {p, w, T, w0, T0, wout, tout})
        PGMG_TRY(check_span(q, N, 8, 0, N - 1, 0, N - 1, "pgmg_boussinesq_rk_time"));
    PGMG_TRY(vort_events(c));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    const double dt = 0.25 * L.h * L.h;
    const double buoy[2] = {0.0, 1.0};
    const int depth = which >> 1;
    const bool copies = (which & 1) == 0;
    auto run = [&]() -> int {
        if (copies) {
            launch_bouss_stage_depth(depth, p, N, w, N, T, N, w0, N, T0, N, wout, N, tout, N, N, L.h, dt,
                                     1.0, 1.0, buoy, 0.75, 0.25, nullptr, nullptr, c->s);
            HIPC(hipMemcpyAsync(w, wout, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
            HIPC(hipMemcpyAsync(T, tout, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        } else {
            launch_bouss_stage_depth(depth, p, N, w, N, T, N, w0, N, T0, N, wout, N, tout, N, N, L.h, dt,
                                     1.0, 1.0, buoy, 0.75, 0.25, c->grad_buf, c->grad_buf + c->grad_cap,
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
    if (bytes) *bytes = (double)elems * (copies ? 88.0 : 56.0);
    return PGMG_OK;
}

}  // extern "C"
