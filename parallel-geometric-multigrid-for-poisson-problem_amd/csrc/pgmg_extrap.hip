// pgmg_extrap.hip — fourth-order solves by Richardson extrapolation (include/pgmg.h "Fourth-order
// solves"): the injection k_inject, the two extrapolation passes k_extrap_diff and
// k_extrap_add, the half-resolution context and pgmg_solve_extrap.
//
// The solves are the existing entries (pgmg_fmg_bc, pgmg_solve_damped) on the context and on a
// half-resolution context it owns; what is new is one streaming operation on phi,
//     F <- F + C((F(2j, 2i) - Cg) * K3)      on the interior of F,
// in two passes because the update writes the coincident points that the difference of
// neighbouring workgroups reads: k_extrap_diff forms D on a coarse-sized scratch grid from the F
// of before the operation, k_extrap_add is pointwise in F and may write it in place.  fp64 only
// (pgmg.h: fp32 solves stall above the h^4 the extrapolation is after).
#include <chrono>
#include <string>

#include "pgmg_host.h"
#include "pgmg_stop.h"

using namespace pgmg;

namespace pgmg {

constexpr int kExU = 4;        // coarse rows of loads in flight per wave (k_interp_cubic's kCubU)
constexpr int kInjRows = 4;    // destination rows per workgroup of the strided copies

// dst(j, i) = src(2j, 2i), n x n destination points: a lane per destination column, kInjRows
// rows per workgroup.  Half of every source line read is used (the odd columns ride along);
// the odd source rows are never touched.
__global__ __launch_bounds__(kBlock) void k_inject(const double *__restrict__ src, long long Ps,
                                                   double *__restrict__ dst, long long Pd, int n)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j0 = blockIdx.y * kInjRows;
    #pragma unroll
    for (int u = 0; u < kInjRows; ++u) {
        const int j = j0 + u;
        if (j < n) dst[j * Pd + i] = src[2LL * j * Ps + 2 * i];
    }
}

// D(j, i) = (F(2j, 2i) - Cg(j, i)) * K3 on all Nc x Nc coarse points, frame included: one
// rounding for the difference, one for the product (-ffp-contract=off; a product and a
// difference cannot contract anyway).  The geometry of k_inject.
__global__ __launch_bounds__(kBlock) void k_extrap_diff(const double *__restrict__ F, long long Pf,
                                                        const double *__restrict__ Cg, long long Pc,
                                                        double *__restrict__ D, long long Pd, int Nc)
{
    const double k3 = __longlong_as_double(0x3FD5555555555555LL);   // the double nearest 1/3
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= Nc) return;
    const int j0 = blockIdx.y * kInjRows;
    #pragma unroll
    for (int u = 0; u < kInjRows; ++u) {
        const int j = j0 + u;
        if (j < Nc) D[j * Pd + i] = (F[2LL * j * Pf + 2 * i] - Cg[j * Pc + i]) * k3;
    }
}

struct ExtrapArgs {
    const double *d;     // element (0, 0) of D, pitch Pd
    double *f;           // element (0, 0) of the fine grid (2 Nc - 1 points per side), pitch Pf
    long long Pd, Pf;
    int Nc;
    int band;            // coarse rows per workgroup
};

// F(y, x) <- F(y, x) + C(D)(y, x) on 1 <= y, x <= Nf - 2.  The shape of k_interp_cubic
// (pgmg_fmg.hip), whose formulas and evaluation order these are: lane t of a workgroup owns coarse
// column i = 1 + 256 bx + t and the fine column pair (2i-1, 2i); a coarse row is interpolated
// along x in registers, c[i-1], c[i-2] and c[i+1] from the neighbouring lanes by DPP (lanes 0 and
// 63 load their halo columns; the moves are unconditional, outside every branch that could
// disable a source lane); the one-sided columns (fine 1 and Nf-2) are a second expression in the
// waves that hold them, a wave-uniform branch; the workgroup marches down its band of coarse
// rows j (fine rows 2j-1, 2j) with a four-row window of x-interpolated rows, kExU coarse rows
// loaded before the first is used; the one-sided rows (fine 1 and Nf-2) take their fourth row
// from one extra load in a workgroup-uniform branch.  What differs: the result is added to the
// fine pair, read with one 16-byte load before the store (element-aligned: the caller's array of
// the op has an odd pitch; on the context's grids the pair is 16-byte aligned and the same
// instruction); and the frame is skipped -- fine rows 0 and Nf-1 and fine column 0 are not
// computed at all, and the lane that owns i = Nc-1 stores its odd column alone (column Nf-1 is
// loaded, never stored).
__global__ __launch_bounds__(kBlock) void k_extrap_add(ExtrapArgs a)
{
    using T = double;
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
    const long long Pd = a.Pd, Pf = a.Pf;
    const T *__restrict__ C = a.d;
    T *F = a.f;
    const T k9 = T(9), k5 = T(5), k15 = T(15), s16 = T(0.0625);

    // what one coarse row contributes: the lane's loads ...
    struct RowLd {
        T own, hb, ha, hd, x3;
    };
    auto load_row = [&](int r) -> RowLd {
        const T *p = C + (long long)r * Pd;
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
    // ... and its x-interpolation: .x fine column 2i-1, .y fine column 2i
    auto xrow = [&](const RowLd &v) -> D2 {
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
        return mk2<T>(odd, v.own);
    };
    // fine row fr (1 .. Nf-2) += e on the lane's pair; the last lane's even column is the frame
    auto add = [&](int fr, D2 e) {
        if (!own) return;
        T *p = F + (long long)fr * Pf + 2 * i - 1;
        const D2 cur = ldvu(p);
        if (last) p[0] = cur.x + e.x;
        else stvu(p, mk2<T>(cur.x + e.x, cur.y + e.y));
    };

    const int jb = 1 + blockIdx.y * a.band;
    const int je = min(jb + a.band, Nc);   // coarse rows jb .. je-1 (at most Nc-1)
    D2 wa, wb, wc;                         // x-interpolated rows j-2, j-1, j
    {
        const RowLd ra = load_row(max(jb - 2, 0)), rb = load_row(jb - 1), rc = load_row(jb);
        wa = xrow(ra);
        wb = xrow(rb);
        wc = xrow(rc);
    }
    for (int j = jb; j < je; j += kExU) {
        RowLd ld[kExU];
        #pragma unroll
        for (int u = 0; u < kExU; ++u) ld[u] = load_row(min(j + u + 1, Nc - 1));
        #pragma unroll
        for (int u = 0; u < kExU; ++u) {
            const int r = j + u;   // this step's coarse row (uniform over the workgroup)
            const D2 wd = xrow(ld[u]);
            if (r < je) {
                D2 o;
                if (r == 1 || r == Nc - 1) {
                    // fine row 1: rows 0, 1, 2 and 3; fine row Nf-2: rows Nc-1 .. Nc-4
                    const RowLd rx = load_row(r == 1 ? 3 : Nc - 4);
                    const D2 wx = xrow(rx);
                    if (r == 1) {
                        o.x = (k5 * wb.x + k15 * wc.x - k5 * wd.x + wx.x) * s16;
                        o.y = (k5 * wb.y + k15 * wc.y - k5 * wd.y + wx.y) * s16;
                    } else {
                        o.x = (k5 * wc.x + k15 * wb.x - k5 * wa.x + wx.x) * s16;
                        o.y = (k5 * wc.y + k15 * wb.y - k5 * wa.y + wx.y) * s16;
                    }
                } else {
                    o.x = (k9 * (wb.x + wc.x) - (wa.x + wd.x)) * s16;
                    o.y = (k9 * (wb.y + wc.y) - (wa.y + wd.y)) * s16;
                }
                add(2 * r - 1, o);
                if (r < Nc - 1) add(2 * r, wc);   // (fine row Nf-1 is the frame)
            }
            wa = wb;
            wb = wc;
            wc = wd;
        }
    }
}

void launch_inject(const double *src, long long Ps, double *dst, long long Pd, int n, hipStream_t s)
{
    const dim3 g((n + kBlock - 1) / kBlock, (n + kInjRows - 1) / kInjRows);
    k_inject<<<g, dim3(kBlock), 0, s>>>(src, Ps, dst, Pd, n);
}

// (k_extrap_add's launch geometry is k_interp_cubic's: 256 coarse columns per workgroup in x,
// bands of 32 coarse rows, shorter while the grid has fewer than ~1024 workgroups)
void launch_extrap(double *fine, long long Pf, const double *coarse, long long Pc, double *D,
                   long long Pd, int Nc, hipStream_t s)
{
    const dim3 gd((Nc + kBlock - 1) / kBlock, (Nc + kInjRows - 1) / kInjRows);
    k_extrap_diff<<<gd, dim3(kBlock), 0, s>>>(fine, Pf, coarse, Pc, D, Pd, Nc);
    ExtrapArgs a{};
    a.d = D;
    a.f = fine;
    a.Pd = Pd;
    a.Pf = Pf;
    a.Nc = Nc;
    const int gx = (Nc - 1 + kBlock - 1) / kBlock;
    a.band = 32;
    while (a.band > 4 && gx * ((Nc - 1 + a.band - 1) / a.band) < 1024) a.band /= 2;
    const int gy = (Nc - 1 + a.band - 1) / a.band;
    k_extrap_add<<<dim3(gx, gy), dim3(kBlock), 0, s>>>(a);
}

int coarsest_n(int N, int n_coarse)
{
    while (N > n_coarse) N = (N - 1) / 2 + 1;
    return N;
}

// the half-resolution context, the scratch grid D and the two events, made on the first call
static int extrap_setup(pgmg_ctx *c)
{
    const int Nc = (c->cfg.N + 1) / 2;
    if (!c->ex_child) {
        pgmg_config cfg = c->cfg;
        cfg.N = Nc;
        // the child's mesh width is 2 * lv[0].h: the caller's h0 doubled, or (h0 = 0) left to
        // pgmg_create's a / (Nc - 1) = 2 * (a / (N - 1)) bit for bit (Nc - 1 = (N - 1) / 2; a
        // factor of two commutes with the division's rounding).  Not 2 * lv[0].h outright: with
        // a < 0 that is negative, and pgmg_create refuses a negative h0
        cfg.h0 = c->cfg.h0 > 0.0 ? 2 * c->cfg.h0 : 0.0;
        cfg.rank = 0;
        cfg.world = 1;
        cfg.nccl_unique_id = nullptr;
        PGMG_TRY(pgmg_create(&c->ex_child, &cfg));
        if (c->ex_child->lv[0].h != 2 * c->lv[0].h) {   // (an a at the edge of the double range)
            pgmg_destroy(c->ex_child);
            c->ex_child = nullptr;
            return set_err(PGMG_ERR_STATE, "pgmg_solve_extrap: the half-resolution context's mesh "
                                           "width is not twice the context's");
        }
    }
    if (!c->ex_D) {
        const size_t bytes = alloc_elems(Nc, Nc) * sizeof(double);
        if (hipMalloc((void **)&c->ex_D, bytes) != hipSuccess) {
            c->ex_D = nullptr;
            return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_solve_extrap's scratch grid");
        }
        register_alloc(c->ex_D, bytes);
    }
    if (!c->ex_ev0) HIPC(hipEventCreate(&c->ex_ev0));
    if (!c->ex_ev1) HIPC(hipEventCreate(&c->ex_ev1));
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_solve_extrap(pgmg_ctx *c, const pgmg_solve_opts *o, int nu, double omega,
                      pgmg_extrap_info *info)
{
    const std::string who("pgmg_solve_extrap");
    if (!c || !o || !info) return set_err(PGMG_ERR_ARG, "null argument");
    if (const char *bad = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (nu < 1) return set_err(PGMG_ERR_ARG, who + ": nu must be at least 1");
    // (omega = 0, pgmg_fmg_bc's undamped climb, is refused too: pgmg.h says why)
    PGMG_TRY(damp_omega_check(omega, "pgmg_solve_extrap"));
    const int N = c->cfg.N, Nc = (N + 1) / 2;
    if (N < 9)
        return set_err(PGMG_ERR_ARG, who + ": N must be at least 9 (a half-resolution grid of 5 "
                                           "points per side)");
    if (coarsest_n(N, c->cfg.n_coarse) < 5 || coarsest_n(Nc, c->cfg.n_coarse) < 5)
        return set_err(PGMG_ERR_ARG, who + ": the coarsest level of the grid and of the half-"
                                           "resolution grid need 5 points per side (n_coarse >= 5)");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    if (c->fp32)
        return set_err(PGMG_ERR_STATE, who + ": fp64 contexts only: fp32 solves stall at ||r|| / "
                                           "||f|| ~ 1e-5 .. 1e-3, a rounding floor that leaves the "
                                           "extrapolated error at 2e-7 .. 2e-6, no better than "
                                           "second order");
    if ((o->monitor & PGMG_MON_ERROR) && !c->analytic)
        return set_err(PGMG_ERR_STATE, who + ": PGMG_MON_ERROR needs the analytic problem (f = NULL)");
    const auto t0 = std::chrono::steady_clock::now();
    *info = pgmg_extrap_info{};
    PGMG_TRY(extrap_setup(c));
    pgmg_ctx *ch = c->ex_child;
    if (ch->cfg.eps != c->cfg.eps) PGMG_TRY(pgmg_set_eps(ch, c->cfg.eps));
    const Level &L = c->lv[0];
    // phi and the stored f where they lie NOW: the caller's arrays (pitch N) or the level-0 grids
    // (the cross-fused cycles rotate A / B / S: lv[0].A is read again after the solves)
    const long long Pf = c->ext_phi ? N : L.P;
    const double *const rhs = c->ext_f ? c->ext_f : G<double>(L.F);
    const long long Pr = c->ext_f ? N : L.P;
    // 2. the child's problem (every earlier call on c has left its stream idle or ordered)
    {
        const double *const phi = c->ext_phi ? c->ext_phi : G<double>(L.A);
        if (c->ext_phi) PGMG_TRY(order_after_caller(c));
        else PGMG_TRY(check_span(phi, Pf, 8, 0, N - 1, 0, N - 1, "pgmg_solve_extrap phi"));
        if (!c->ext_f) PGMG_TRY(check_span(rhs, Pr, 8, 0, N - 1, 0, N - 1, "pgmg_solve_extrap f"));
        PGMG_TRY(set_problem_injected(ch, phi, Pf, rhs, Pr, c->s));
    }
    // 3. and 4. the two solves
    pgmg_solve_opts oc = *o;
    oc.monitor = PGMG_MON_RESIDUAL;
    PGMG_TRY(pgmg_fmg_bc(ch, nu, omega));
    PGMG_TRY(pgmg_solve_damped(ch, &oc, omega, &info->coarse));
    PGMG_TRY(pgmg_stats(ch, &info->coarse_sweeps, &info->coarse_exits));
    PGMG_TRY(pgmg_fmg_bc(c, nu, omega));
    PGMG_TRY(pgmg_solve_damped(c, o, omega, &info->fine));
    // 5. the extrapolation (both solves are synchronous: the child's phi is final)
    const Level &Lc = ch->lv[0];
    double *const F = c->ext_phi ? c->ext_phi : G<double>(L.A);
    double *const D = c->ex_D + kOff;
    const long long Pd = pitch_for(Nc);
    if (!c->ext_phi) PGMG_TRY(check_span(F, Pf, 8, 0, N - 1, 0, N - 1, "k_extrap_add phi"));
    PGMG_TRY(check_span(G<double>(Lc.A), Lc.P, 8, 0, Nc - 1, 0, Nc - 1, "k_extrap_diff coarse phi"));
    PGMG_TRY(check_span(D, Pd, 8, 0, Nc - 1, 0, Nc - 1, "k_extrap_diff D"));
    c->carry = false;
    c->hist.reset(c->nb);
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    HIPC(hipEventRecord(c->ex_ev0, c->s));
    launch_extrap(F, Pf, G<double>(Lc.A), Lc.P, D, Pd, Nc, c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ex_ev1, c->s));
    PGMG_TRY(stream_wait(c));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, c->ex_ev0, c->ex_ev1));
    info->extrap_ms = ms;
    info->elapsed_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PGMG_OK;
}

}  // extern "C"
