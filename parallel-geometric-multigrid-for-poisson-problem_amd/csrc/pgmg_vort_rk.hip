// pgmg_vort_rk.hip — strong-stability-preserving Runge-Kutta time stepping of the vorticity
// transport (include/pgmg.h "Runge-Kutta vorticity transport"; DESIGN.md §4h "Runge-Kutta"):
// k_vort_stage, pgmg_vorticity_step_rk and pgmg_vorticity_rk_time (pgmg_vorticity_stage_grid, on
// the caller's arrays: pgmg_ops.hip; the time loop itself is vort_advance, pgmg_vorticity.hip).
//
// In Shu-Osher form every stage after the first is a convex combination of the omega the step
// started from, W0, and an explicit Euler step E of the current omega under the current psi:
//   k_vort_stage  out = a * W0 + b * E(psi, omega) on the interior, out's frame = omega's, word
//                 for word.  k_vort_step's pass (pgmg_vorticity.hip) on its decomposition
//                 grad_grid(N), with a third input stream: of W0 a lane reads its own column pair
//                 of the current row and nothing else, one unaligned vector load per row issued
//                 with the window's kGradU rows of loads -- no window, no DPP, no edge load.  24 B
//                 read and 8 B written per point.  e is formed by k_vort_step's expression, then
//                 a * W0, b * e and their sum, one rounding each.  VMAX as in k_vort_step.
// Stage 1 of every order is k_vort_step itself, not this pass with (a, b) = (0, 1).
#include <cmath>
#include <string>

#include "pgmg_host.h"
#include "pgmg_vort_dev.h"

using namespace pgmg;

namespace pgmg {

struct StageArgs {
    const double *p;    // element (0, 0) of psi, pitch Pp
    long long Pp;
    const double *w;    // element (0, 0) of omega, pitch Pw
    long long Pw;
    const double *w0;   // element (0, 0) of the saved omega, pitch P0
    long long P0;
    double *out;        // element (0, 0), pitch Po
    long long Po;
    double *partials;   // VMAX: one per workgroup
    double wgt, ih;     // 0.5 / h, 1.0 / (h * h)
    double dt, nu;
    double a, b;        // out = a * w0 + b * e
    int N;
    int band;           // rows per workgroup
};

template <bool VMAX>
__global__ __launch_bounds__(kBlock) void k_vort_stage(StageArgs a)
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
    const double *W = a.w;     // (W0 may be W: neither is written)
    const double *W0 = a.w0;
    const long long Pp = a.Pp, Pw = a.Pw, P0 = a.P0;
    const double wgt = a.wgt, ih = a.ih, dt = a.dt, nu = a.nu, ca = a.a, cb = a.b;
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
            // s0[k]: W0's pair of row j + k, the row computed at step k.  Clamped into the
            // interior rows: the frame of W0 has no part in any value
            VD2 s0[kGradU];
            #pragma unroll
            for (int k = 0; k < kGradU; ++k) {
                const int r = min(j + k + 1, N - 1);
                sp[2 + k] = load(P + r * Pp);
                sw[2 + k] = load(W + r * Pw);
                const int r0 = min(max(j + k, 1), N - 2);
                s0[k] = ldvu<double>(W0 + r0 * P0 + cl);
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
                        const double ea = wc.o.x + dt * (nu * lapa - adva);
                        const double eb = wc.o.y + dt * (nu * lapb - advb);
                        o.x = ca * s0[k].x + cb * ea;
                        // (column N-1 is the frame)
                        o.y = lastl ? wc.o.y : ca * s0[k].y + cb * eb;
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

void launch_vort_stage(const double *psi, long long Pp, const double *w, long long Pw,
                       const double *w0, long long P0, double *out, long long Po, int N, double h,
                       double dt, double nu, double ca, double cb, double *partials, double *vmax,
                       hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    StageArgs a{};
    a.p = psi;
    a.Pp = Pp;
    a.w = w;
    a.Pw = Pw;
    a.w0 = w0;
    a.P0 = P0;
    a.out = out;
    a.Po = Po;
    a.partials = vmax != nullptr ? partials : nullptr;
    a.wgt = 0.5 / h;
    a.ih = 1.0 / (h * h);
    a.dt = dt;
    a.nu = nu;
    a.a = ca;
    a.b = cb;
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (vmax != nullptr) {
        k_vort_stage<true><<<grid, dim3(kBlock), 0, s>>>(a);
        launch_vort_max(partials, g.tiles * g.bands, vmax, s);
    } else {
        k_vort_stage<false><<<grid, dim3(kBlock), 0, s>>>(a);
    }
}

}  // namespace pgmg

extern "C" {

int pgmg_vorticity_step_rk(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, double dt, double nu,
                           int mode, const double walls[4], int order, int nsteps,
                           pgmg_vort_info *info)
{
    return vort_advance(c, o, omega, dt, nu, mode, walls, order, nsteps, info,
                        "pgmg_vorticity_step_rk");
}

int pgmg_vorticity_rk_time(pgmg_ctx *c, int which, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_vorticity_rk_time");
    if (!c || !ms_per_pass || reps <= 0 || (which != 0 && which != 1))
        return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(vort_state_check(c, who));
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    if (!c->vt_rk_scr) {
        if (hipMalloc((void **)&c->vt_rk_scr, 4 * elems * sizeof(double)) != hipSuccess) {
            c->vt_rk_scr = nullptr;
            return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_vorticity_rk_time's arrays");
        }
        register_alloc(c->vt_rk_scr, 4 * elems * sizeof(double));
        HIPC(hipMemsetAsync(c->vt_rk_scr, 0, 4 * elems * sizeof(double), c->s));
    }
    // psi, omega, the saved omega and out, all zero: the stage then leaves omega as it is, pass
    // after pass
    double *const p = c->vt_rk_scr, *const w = p + elems, *const w0 = w + elems, *const out = w0 + elems;
    for (double *q : {p, w, w0, out})
        PGMG_TRY(check_span(q, N, 8, 0, N - 1, 0, N - 1, "pgmg_vorticity_rk_time"));
    PGMG_TRY(vort_events(c));
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    const double dt = 0.25 * L.h * L.h;
    auto run = [&]() -> int {
        if (which == 0) {
            launch_vort_stage(p, N, w, N, w0, N, out, N, N, L.h, dt, 1.0, 0.75, 0.25, nullptr, nullptr,
                              c->s);
            HIPC(hipMemcpyAsync(w, out, elems * sizeof(double), hipMemcpyDeviceToDevice, c->s));
        } else {
            launch_vort_stage(p, N, w, N, w0, N, out, N, N, L.h, dt, 1.0, 0.75, 0.25, c->grad_buf,
                              c->grad_buf + c->grad_cap, c->s);
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
    if (bytes) *bytes = (double)elems * (which == 0 ? 48.0 : 32.0);
    return PGMG_OK;
}

}  // extern "C"
