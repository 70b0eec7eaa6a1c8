// pgmg_ops.hip — op-level C ABI on caller-owned device arrays (reference layout)
// mirroring Parallel::ComputeJacobi / ComputeResidual / ComputeRestriction /
// ComputeProlungator (3_part_parallel/Parallel_Method.cu:144-199), plus device
// memory helpers so host code can drive the library without HIP headers.
//
// Like the reference's, the Jacobi op updates the caller's x in place -- but race-free: its
// passes defer every tile-edge output another workgroup reads (pgmg_gops.hip "In-place
// sweeps"; the reference's jacobi_kernel races), so each sweep is exactly the
// out-of-place Jacobi sweep; with eps >= 0 it applies the CPU smoother's residual-norm early
// exit, so its result equals JacobiSmoother::smooth bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "pgmg_host.h"

using namespace pgmg;

namespace {

struct OpScratch {
    double *partials = nullptr;
    unsigned *flags = nullptr;
    unsigned long long *stats = nullptr;
    double *scalar = nullptr;
    double *tmp = nullptr;
    size_t tmp_elems = 0;
    double *side = nullptr;   // the in-place passes' deferred tile-edge outputs
    size_t side_elems = 0;
    double *mon = nullptr;    // pgmg_damp_grid: 3 partial sums per workgroup, then the 3 totals
    size_t mon_elems = 0;
    double *exd = nullptr;    // pgmg_extrap_grid: the coarse-sized difference grid D
    size_t exd_elems = 0;
    double *grad = nullptr;   // pgmg_gradient_grid: a partial sum per workgroup, then the total
    size_t grad_elems = 0;
};

// One scratch set per stream: ops enqueued on different streams never share partial sums,
// flags or the ping-pong buffer (the reference's ops are synchronous on the default stream;
// these are asynchronous on the caller's).  A set lives until pgmg_ops_release(stream).
std::mutex g_op_mu;
std::map<hipStream_t, OpScratch> g_ops;

int ensure_scratch(hipStream_t s, size_t tmp_elems, OpScratch **out)
{
    std::lock_guard<std::mutex> lk(g_op_mu);
    OpScratch &o = g_ops[s];
    if (!o.partials) {
        HIPC(hipMalloc((void **)&o.partials, kOpPartialsCap * sizeof(double)));
        HIPC(hipMalloc((void **)&o.flags, (kMaxSweeps + 2) * 128 * sizeof(unsigned)));
        HIPC(hipMalloc((void **)&o.stats, 4 * sizeof(unsigned long long)));
        HIPC(hipMalloc((void **)&o.scalar, 4 * sizeof(double)));
    }
    if (tmp_elems > o.tmp_elems) {
        if (o.tmp) {
            HIPC(hipStreamSynchronize(s));   // the old buffer may still be in use on s
            HIPC(hipFree(o.tmp));
        }
        o.tmp = nullptr;
        o.tmp_elems = 0;
        HIPC(hipMalloc((void **)&o.tmp, tmp_elems * sizeof(double)));
        o.tmp_elems = tmp_elems;
    }
    *out = &o;
    return PGMG_OK;
}

int ensure_side(hipStream_t s, OpScratch &o, size_t elems)
{
    std::lock_guard<std::mutex> lk(g_op_mu);
    if (elems <= o.side_elems) return PGMG_OK;
    if (o.side) {
        HIPC(hipStreamSynchronize(s));
        HIPC(hipFree(o.side));
    }
    o.side = nullptr;
    o.side_elems = 0;
    HIPC(hipMalloc((void **)&o.side, elems * sizeof(double)));
    o.side_elems = elems;
    return PGMG_OK;
}

int ensure_mon(hipStream_t s, OpScratch &o, size_t elems)
{
    std::lock_guard<std::mutex> lk(g_op_mu);
    if (elems <= o.mon_elems) return PGMG_OK;
    if (o.mon) {
        HIPC(hipStreamSynchronize(s));
        HIPC(hipFree(o.mon));
    }
    o.mon = nullptr;
    o.mon_elems = 0;
    HIPC(hipMalloc((void **)&o.mon, elems * sizeof(double)));
    o.mon_elems = elems;
    return PGMG_OK;
}

int ensure_exd(hipStream_t s, OpScratch &o, size_t elems)
{
    std::lock_guard<std::mutex> lk(g_op_mu);
    if (elems <= o.exd_elems) return PGMG_OK;
    if (o.exd) {
        HIPC(hipStreamSynchronize(s));
        HIPC(hipFree(o.exd));
    }
    o.exd = nullptr;
    o.exd_elems = 0;
    HIPC(hipMalloc((void **)&o.exd, elems * sizeof(double)));
    o.exd_elems = elems;
    return PGMG_OK;
}

int ensure_grad(hipStream_t s, OpScratch &o, size_t elems)
{
    std::lock_guard<std::mutex> lk(g_op_mu);
    if (elems <= o.grad_elems) return PGMG_OK;
    if (o.grad) {
        HIPC(hipStreamSynchronize(s));
        HIPC(hipFree(o.grad));
    }
    o.grad = nullptr;
    o.grad_elems = 0;
    HIPC(hipMalloc((void **)&o.grad, elems * sizeof(double)));
    o.grad_elems = elems;
    return PGMG_OK;
}

}  // namespace

extern "C" {

// scale * grad(phi) on the caller's arrays (pitch N): pgmg_gradient's pass (pgmg_gradient.hip),
// its decomposition and partial sums those of a context of that N
int pgmg_gradient_grid(const double *d_phi, double *d_gx, double *d_gy, int N, double h, int order,
                       double scale, double *norm, void *stream)
{
    if (!d_phi || N < 5 || ((N - 1) & (N - 2)) != 0 || !std::isfinite(h) || h == 0.0)
        return set_err(PGMG_ERR_ARG, "pgmg_gradient_grid: need phi, N = 2^k + 1 with k >= 2, a finite "
                                     "h that is not 0");
    if ((order != 2 && order != 4) || !std::isfinite(scale))
        return set_err(PGMG_ERR_ARG, "pgmg_gradient_grid: order must be 2 or 4, scale finite");
    if (const char *bad = gradient_arrays_error(d_phi, (size_t)N * N * sizeof(double), d_gx, d_gy, N))
        return set_err(PGMG_ERR_ARG, std::string("pgmg_gradient_grid: ") + bad);
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    int e = ensure_scratch(s, 0, &op);
    if (e) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (norm && (e = ensure_grad(s, *op, np + 1))) return e;
    double *sum = norm ? op->grad + np : nullptr;
    launch_gradient<double, double>(d_phi, N, d_gx, d_gy, N, gradient_weight(order, scale, h), order,
                                    op->grad, sum, s);
    HIPC(hipGetLastError());
    if (norm) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, sum, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *norm = std::sqrt(t);
    }
    return PGMG_OK;
}

// what both projection ops refuse in N, h, order and scale (pgmg_gradient_grid's rules)
static int project_op_check(const char *who, int N, double h, int order, double scale)
{
    if (N < 5 || ((N - 1) & (N - 2)) != 0 || !std::isfinite(h) || h == 0.0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": need N = 2^k + 1 with k >= 2, a finite h "
                                                        "that is not 0");
    if ((order != 2 && order != 4) || !std::isfinite(scale))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": order must be 2 or 4, scale finite");
    return PGMG_OK;
}

// out = dx(u) + dy(v) on the caller's arrays (pitch N): pgmg_project's divergence pass
// (pgmg_project.hip), its decomposition and partial sums k_gradient's
int pgmg_divergence_grid(const double *d_u, const double *d_v, double *d_out, int N, double h,
                         int order, double scale, double *norm, void *stream)
{
    const char *const who = "pgmg_divergence_grid";
    int e = project_op_check(who, N, h, order, scale);
    if (e) return e;
    if (!d_u || !d_v) return set_err(PGMG_ERR_ARG, std::string(who) + ": null u or v");
    if (!d_out && !norm) return set_err(PGMG_ERR_ARG, std::string(who) + ": both out and norm are null");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (d_out && !device_range(d_out, N))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": out is not device memory");
    if (d_out && (ranges_overlap(d_out, bytes, d_u, bytes) || ranges_overlap(d_out, bytes, d_v, bytes)))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": out overlaps u or v");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (norm && (e = ensure_grad(s, *op, np + 1))) return e;
    double *sum = norm ? op->grad + np : nullptr;
    launch_divergence(d_u, d_v, d_out, N, N, gradient_weight(order, scale, h), order, op->grad, sum, s);
    HIPC(hipGetLastError());
    if (norm) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, sum, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *norm = std::sqrt(t);
    }
    return PGMG_OK;
}

// u += gx(phi), v += gy(phi) on the caller's arrays (u, v: pitch N; phi: pitch_phi):
// pgmg_project's update pass (pgmg_project.hip)
int pgmg_gradient_add_grid(const double *d_phi, long long pitch_phi, double *d_u, double *d_v, int N,
                           double h, int order, double scale, void *stream)
{
    const char *const who = "pgmg_gradient_add_grid";
    int e = project_op_check(who, N, h, order, scale);
    if (e) return e;
    if (!d_phi || pitch_phi < N) return set_err(PGMG_ERR_ARG, std::string(who) + ": need phi, pitch_phi >= N");
    // the bytes of phi the pass reads: its first element to the last of row N-1
    const size_t pn = ((size_t)(N - 1) * (size_t)pitch_phi + (size_t)N) * sizeof(double);
    if (const char *bad = gradient_arrays_error(d_phi, pn, d_u, d_v, N))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": " + bad);
    launch_grad_update(d_phi, pitch_phi, d_u, d_v, N, gradient_weight(order, scale, h), order,
                       (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

// what both vorticity ops refuse in N and h (pgmg_divergence_grid's rules)
static int vort_op_check(const char *who, int N, double h)
{
    if (N < 5 || ((N - 1) & (N - 2)) != 0 || !std::isfinite(h) || h == 0.0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": need N = 2^k + 1 with k >= 2, a finite h "
                                                        "that is not 0");
    return PGMG_OK;
}

// out = the explicit Euler step of omega under psi on the caller's arrays (pitch N):
// pgmg_vorticity_step's pass (pgmg_vorticity.hip), its decomposition k_gradient's
int pgmg_vorticity_grid(const double *d_psi, const double *d_w, double *d_out, int N, double h,
                        double dt, double nu, double *vmax, void *stream)
{
    const char *const who = "pgmg_vorticity_grid";
    int e = vort_op_check(who, N, h);
    if (e) return e;
    if (const char *bad = vort_step_error(dt, nu)) return set_err(PGMG_ERR_ARG, std::string(who) + ": " + bad);
    if (!d_psi || !d_w || !d_out) return set_err(PGMG_ERR_ARG, std::string(who) + ": null psi, w or out");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_out, N))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": out is not device memory");
    if (ranges_overlap(d_out, bytes, d_psi, bytes) || ranges_overlap(d_out, bytes, d_w, bytes))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": out overlaps psi or w");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (vmax && (e = ensure_grad(s, *op, np + 1))) return e;
    double *top = vmax ? op->grad + np : nullptr;
    launch_vort_step(d_psi, N, d_w, N, d_out, N, N, h, dt, nu, op->grad, top, s);
    HIPC(hipGetLastError());
    if (vmax) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, top, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *vmax = t;
    }
    return PGMG_OK;
}

// out = a * w0 + b * (the explicit Euler step of omega under psi) on the caller's arrays (pitch
// N): pgmg_vorticity_step_rk's stage pass (pgmg_vort_rk.hip); w0 may be w
int pgmg_vorticity_stage_grid(const double *d_psi, const double *d_w, const double *d_w0,
                              double *d_out, int N, double h, double dt, double nu, double a,
                              double b, double *vmax, void *stream)
{
    const std::string who("pgmg_vorticity_stage_grid");
    int e = vort_op_check(who.c_str(), N, h);
    if (e) return e;
    if (const char *bad = vort_step_error(dt, nu)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (!std::isfinite(a) || !std::isfinite(b)) return set_err(PGMG_ERR_ARG, who + ": a and b must be finite");
    if (!d_psi || !d_w || !d_w0 || !d_out) return set_err(PGMG_ERR_ARG, who + ": null psi, w, w0 or out");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_out, N)) return set_err(PGMG_ERR_ARG, who + ": out is not device memory");
    for (const double *in : {d_psi, d_w, d_w0})
        if (ranges_overlap(d_out, bytes, in, bytes))
            return set_err(PGMG_ERR_ARG, who + ": out overlaps psi, w or w0");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (vmax && (e = ensure_grad(s, *op, np + 1))) return e;
    double *top = vmax ? op->grad + np : nullptr;
    launch_vort_stage(d_psi, N, d_w, N, d_w0, N, d_out, N, N, h, dt, nu, a, b, op->grad, top, s);
    HIPC(hipGetLastError());
    if (vmax) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, top, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *vmax = t;
    }
    return PGMG_OK;
}

// the frame of omega from psi on the caller's arrays (pitch N): pgmg_vorticity_step's wall pass
int pgmg_wall_vorticity_grid(const double *d_psi, double *d_w, int N, double h, int mode,
                             const double walls[4], void *stream)
{
    const char *const who = "pgmg_wall_vorticity_grid";
    int e = vort_op_check(who, N, h);
    if (e) return e;
    if (const char *bad = vort_wall_error(mode, walls)) return set_err(PGMG_ERR_ARG, std::string(who) + ": " + bad);
    if (!d_psi || !d_w) return set_err(PGMG_ERR_ARG, std::string(who) + ": null psi or w");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_w, N)) return set_err(PGMG_ERR_ARG, std::string(who) + ": w is not device memory");
    if (ranges_overlap(d_w, bytes, d_psi, bytes))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": w overlaps psi");
    launch_vort_wall(d_psi, N, d_w, N, N, h, mode, walls, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

// wout and Tout = the explicit Euler steps of w and T under psi with the buoyancy source, on the
// caller's arrays (pitch N): pgmg_boussinesq_step's pass (pgmg_boussinesq.hip)
int pgmg_boussinesq_grid(const double *d_psi, const double *d_w, const double *d_T, double *d_wout,
                         double *d_Tout, int N, double h, double dt, double nu, double kappa,
                         const double buoy[2], double *vmax, void *stream)
{
    const std::string who("pgmg_boussinesq_grid");
    int e = vort_op_check(who.c_str(), N, h);
    if (e) return e;
    if (const char *bad = vort_step_error(dt, nu)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = bouss_step_error(kappa, buoy)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (!d_psi || !d_w || !d_T || !d_wout || !d_Tout)
        return set_err(PGMG_ERR_ARG, who + ": null psi, w, T, wout or Tout");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_wout, N) || !device_range(d_Tout, N))
        return set_err(PGMG_ERR_ARG, who + ": an output is not device memory");
    if (ranges_overlap(d_wout, bytes, d_Tout, bytes)) return set_err(PGMG_ERR_ARG, who + ": the outputs overlap");
    for (const double *out : {d_wout, d_Tout})
        for (const double *in : {d_psi, d_w, d_T})
            if (ranges_overlap(out, bytes, in, bytes))
                return set_err(PGMG_ERR_ARG, who + ": an output overlaps psi, w or T");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (vmax && (e = ensure_grad(s, *op, np + 1))) return e;
    double *top = vmax ? op->grad + np : nullptr;
    launch_bouss_step(d_psi, N, d_w, N, d_T, N, d_wout, N, d_Tout, N, N, h, dt, nu, kappa, buoy,
                      op->grad, top, s);
    HIPC(hipGetLastError());
    if (vmax) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, top, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *vmax = t;
    }
    return PGMG_OK;
}

// wout = a * w0 + b * (the Euler step of w) and Tout = a * T0 + b * (the Euler step of T) on the
// caller's arrays (pitch N): pgmg_boussinesq_step_rk's stage pass (pgmg_bouss_rk.hip); w0 may be
// w and T0 may be T
int pgmg_boussinesq_stage_grid(const double *d_psi, const double *d_w, const double *d_T,
                               const double *d_w0, const double *d_T0, double *d_wout, double *d_Tout,
                               int N, double h, double dt, double nu, double kappa,
                               const double buoy[2], double a, double b, double *vmax, void *stream)
{
    const std::string who("pgmg_boussinesq_stage_grid");
    int e = vort_op_check(who.c_str(), N, h);
    if (e) return e;
    if (const char *bad = vort_step_error(dt, nu)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (const char *bad = bouss_step_error(kappa, buoy)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (!std::isfinite(a) || !std::isfinite(b)) return set_err(PGMG_ERR_ARG, who + ": a and b must be finite");
    if (!d_psi || !d_w || !d_T || !d_w0 || !d_T0 || !d_wout || !d_Tout)
        return set_err(PGMG_ERR_ARG, who + ": null psi, w, T, w0, T0, wout or Tout");
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!device_range(d_wout, N) || !device_range(d_Tout, N))
        return set_err(PGMG_ERR_ARG, who + ": an output is not device memory");
    if (ranges_overlap(d_wout, bytes, d_Tout, bytes)) return set_err(PGMG_ERR_ARG, who + ": the outputs overlap");
    for (const double *out : {d_wout, d_Tout})
        for (const double *in : {d_psi, d_w, d_T, d_w0, d_T0})
            if (ranges_overlap(out, bytes, in, bytes))
                return set_err(PGMG_ERR_ARG, who + ": an output overlaps psi, w, T, w0 or T0");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)gradient_blocks(N);
    if (vmax && (e = ensure_grad(s, *op, np + 1))) return e;
    double *top = vmax ? op->grad + np : nullptr;
    launch_bouss_stage(d_psi, N, d_w, N, d_T, N, d_w0, N, d_T0, N, d_wout, N, d_Tout, N, N, h, dt, nu,
                       kappa, buoy, a, b, op->grad, top, s);
    HIPC(hipGetLastError());
    if (vmax) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, top, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *vmax = t;
    }
    return PGMG_OK;
}

// T's adiabatic walls on the caller's array (pitch N): pgmg_boussinesq_step's scalar wall pass
int pgmg_wall_scalar_grid(double *d_T, int N, unsigned adiabatic, void *stream)
{
    const std::string who("pgmg_wall_scalar_grid");
    if (N < 5 || ((N - 1) & (N - 2)) != 0) return set_err(PGMG_ERR_ARG, who + ": need N = 2^k + 1 with k >= 2");
    if (const char *bad = scalar_wall_error(adiabatic)) return set_err(PGMG_ERR_ARG, who + ": " + bad);
    if (!d_T) return set_err(PGMG_ERR_ARG, who + ": null T");
    if (!device_range(d_T, N)) return set_err(PGMG_ERR_ARG, who + ": T is not device memory");
    launch_scalar_wall(d_T, N, N, adiabatic, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

// fine <- fine + C((fine(2j, 2i) - coarse) * K3) on the caller's arrays (pitches Nf and Nc): the
// two passes of pgmg_solve_extrap's extrapolation (pgmg_extrap.hip), D dense in the stream's set
int pgmg_extrap_grid(double *d_fine, const double *d_coarse, int Nf, void *stream)
{
    if (!d_fine || !d_coarse || Nf < 9 || ((Nf - 1) & (Nf - 2)) != 0)
        return set_err(PGMG_ERR_ARG, "pgmg_extrap_grid: need fine, coarse, Nf = 2^k + 1 with k >= 3");
    const int Nc = (Nf + 1) / 2;
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    int e = ensure_scratch(s, 0, &op);
    if (e) return e;
    if ((e = ensure_exd(s, *op, (size_t)Nc * Nc))) return e;
    launch_extrap(d_fine, Nf, d_coarse, Nc, op->exd, Nc, Nc, s);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

// One damping pass x <- x + w r on the caller's arrays (pitch N): the level-general launch of
// the context's damping pass (pgmg_monitor.hip), its decomposition and sums those of a context
// of that N.
int pgmg_damp_grid(double *d_x, const double *d_f, int N, double h, double omega, double *res_norm,
                   void *stream)
{
    if (!d_x || !d_f || N < 5 || ((N - 1) & (N - 2)) != 0 || !std::isfinite(h) || !(h > 0.0))
        return set_err(PGMG_ERR_ARG, "pgmg_damp_grid: need x, f, N = 2^k + 1 with k >= 2, h > 0");
    int e = damp_omega_check(omega, "pgmg_damp_grid");
    if (e) return e;
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)damp_grid_blocks(N);
    if ((e = ensure_side(s, *op, damp_grid_side_elems(N)))) return e;
    if ((e = ensure_mon(s, *op, 3 * np + 3))) return e;
    double *sums = res_norm ? op->mon + 3 * np : nullptr;
    launch_damp_grid<double>(d_x, N, d_f, N, N, 1.0 / (h * h), h, omega, nullptr, nullptr, op->mon,
                             op->side, sums, s);
    HIPC(hipGetLastError());
    if (res_norm) {
        double t[3];
        HIPC(hipMemcpyAsync(t, sums, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *res_norm = std::sqrt(t[0]);
    }
    return PGMG_OK;
}

// what both refinement ops refuse in N and scale
static int mixed_op_check(const char *who, int N, double scale)
{
    if (N < 5 || ((N - 1) & (N - 2)) != 0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": need N = 2^k + 1 with k >= 2");
    if (!std::isfinite(scale) || !(scale > 0.0))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": scale must be finite and > 0");
    return PGMG_OK;
}

// g = (float)(r * scale), r the fp64 residual of (x, f), on the caller's arrays (pitch N):
// pgmg_solve_mixed's defect pass (pgmg_mixed.hip), its decomposition and partial sums the
// monitor's of a context of that N
int pgmg_defect_grid(const double *d_x, const double *d_f, float *d_g, int N, double h, double scale,
                     double *res_norm, void *stream)
{
    const char *const who = "pgmg_defect_grid";
    int e = mixed_op_check(who, N, scale);
    if (e) return e;
    if (!std::isfinite(h) || h == 0.0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": need a finite h that is not 0");
    if (!d_x || !d_f || !d_g) return set_err(PGMG_ERR_ARG, std::string(who) + ": null x, f or g");
    const size_t bytes = (size_t)N * N * sizeof(double), gbytes = (size_t)N * N * sizeof(float);
    if (!device_range_f32(d_g, N))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": g is not device memory");
    if (ranges_overlap(d_g, gbytes, d_x, bytes) || ranges_overlap(d_g, gbytes, d_f, bytes))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": g overlaps x or f");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    if ((e = ensure_scratch(s, 0, &op))) return e;
    const size_t np = (size_t)damp_grid_blocks(N);
    if ((e = ensure_mon(s, *op, 3 * np + 3))) return e;
    double *sums = res_norm ? op->mon + 3 * np : nullptr;
    launch_defect(d_x, N, d_f, N, d_g, N, N, 1.0 / (h * h), scale, op->mon, sums, s);
    HIPC(hipGetLastError());
    if (res_norm) {
        double t = 0.0;
        HIPC(hipMemcpyAsync(&t, sums, sizeof(t), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        *res_norm = std::sqrt(t);
    }
    return PGMG_OK;
}

// x += (double)e * scale on the interior of the caller's arrays (pitch N): pgmg_solve_mixed's
// correction pass (pgmg_mixed.hip)
int pgmg_correct_grid(double *d_x, const float *d_e, int N, double scale, void *stream)
{
    const char *const who = "pgmg_correct_grid";
    int e = mixed_op_check(who, N, scale);
    if (e) return e;
    if (!d_x || !d_e) return set_err(PGMG_ERR_ARG, std::string(who) + ": null x or e");
    if (ranges_overlap(d_e, (size_t)N * N * sizeof(float), d_x, (size_t)N * N * sizeof(double)))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": e overlaps x");
    launch_correct(d_x, N, d_e, N, N, scale, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

int pgmg_jacobi(double *d_x, double *d_tmp, const double *d_f, int H, int W, double h, int v,
                double eps, int *sweeps_done, void *stream)
{
    if (!d_x || !d_f || H < 3 || W < 3 || v < 0) return set_err(PGMG_ERR_ARG, "pgmg_jacobi: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t L = (size_t)H * W;
    const int S = v + 1;
    const bool check = eps >= 0.0;
    // every sweep runs in place; only a checked call with v >= 1 needs a ping-pong buffer
    const bool need_tmp = check && S >= 2;
    OpScratch *op = nullptr;
    int e = ensure_scratch(s, (d_tmp || !need_tmp) ? 0 : L, &op);
    if (e) return e;
    OpScratch &g_op = *op;
    // the deferred-edge side buffer: only the passes that sweep in place use it (an unchecked
    // call, or the first sweep of a checked call with an odd count; an even checked count is
    // the ping-pong below)
    if ((!check || (S & 1)) && (e = ensure_side(s, g_op, g_defer_elems(H, W)))) return e;
    double *tmp = d_tmp ? d_tmp : g_op.tmp;
    // flag slots: a fresh block of S+1 words per call would need a ring; the op is
    // synchronous w.r.t. its own flags because every launch is stream-ordered.
    unsigned *D = g_op.flags;
    // the sweep counter is read back only for a caller that asks for it
    if (sweeps_done) HIPC(hipMemsetAsync(g_op.stats, 0, 4 * sizeof(unsigned long long), s));
    const double hh = h * h, ih = 1.0 / (h * h);
    const int nb = g_blocks(H, W);
    if (nb > kOpPartialsCap) return set_err(PGMG_ERR_STATE, "pgmg_jacobi: too many blocks");
    if (check && S >= (kMaxSweeps + 2) * 128)
        return set_err(PGMG_ERR_ARG, "pgmg_jacobi: v too large for the early-exit flags");
    auto finish = [&]() -> int {
        HIPC(hipGetLastError());
        if (sweeps_done) {
            unsigned long long st[4];
            HIPC(hipMemcpyAsync(st, g_op.stats, sizeof(st), hipMemcpyDeviceToHost, s));
            HIPC(hipStreamSynchronize(s));
            *sweeps_done = (int)st[0];
        }
        return PGMG_OK;
    };
    if (!check) {
        // the reference GPU op (ComputeJacobi decides nothing between its v+1 sweeps,
        // Parallel_Method.cu:144-160): every sweep on d_x itself, in pairs (k_op_sweep2_ip)
        // with an odd count's single sweep first (k_op_sweep_ip); no tmp, no copy-back
        int left = S;
        if (left & 1) {
            launch_g_sweep_ip(d_x, d_f, g_op.side, &D[1], g_op.stats, hh, H, W, s);
            left -= 1;
        }
        for (; left > 0; left -= 2) launch_g_sweep2_ip(d_x, d_f, g_op.side, g_op.stats, hh, H, W, s);
        return finish();
    }
    if (S & 1) {
        // JacobiSmoother::smooth's checks (Smoother.hpp:59-88) with an odd sweep count: sweep
        // 1 has no check and runs in place; sweeps k = 2 .. S alternate x -> tmp -> x, each
        // deciding the previous sweep's check (k_g_fixup undoes the sweep after a firing
        // check) and ending in x; the first of them also writes x's boundary into tmp (no
        // seed copy).  An even count is the ping-pong below, which ends in x by itself.
        launch_g_sweep_ip(d_x, d_f, g_op.side, &D[1], g_op.stats, hh, H, W, s);
        for (int k = 2; k <= S; ++k) {
            const double *in = (k & 1) ? tmp : d_x;
            double *out = (k & 1) ? d_x : tmp;
            launch_g_sweep(in, d_f, out, g_op.partials, &D[k - 1], nullptr, g_op.stats, hh, ih,
                           H, W, k == 2, s);
            launch_g_fixup(g_op.partials, nb, eps, &D[k - 1], &D[k], in, out, g_op.stats, H, W, s);
        }
        return finish();
    }
    // ping-pong (an even checked count): sweeps alternate x -> tmp -> x and end in x.  No
    // seed copy of tmp (Smoother.hpp:47 copies the whole grid into its output buffer): the first
    // sweep writes x's boundary into tmp besides the interior, which is all a later sweep reads
    for (int k = 1; k <= S; ++k) {
        const double *in = (k & 1) ? d_x : tmp;
        double *out = (k & 1) ? tmp : d_x;
        const bool with_check = check && k >= 2;
        launch_g_sweep(in, d_f, out, with_check ? g_op.partials : nullptr,
                       with_check ? &D[k - 1] : nullptr, k == 1 ? &D[1] : nullptr, g_op.stats, hh,
                       ih, H, W, k == 1, s);
        if (with_check)
            launch_g_fixup(g_op.partials, nb, eps, &D[k - 1], &D[k], in, out, g_op.stats, H, W, s);
    }
    return finish();
}

int pgmg_residual(double *d_r, const double *d_x, const double *d_f, int H, int W, double h,
                  void *stream)
{
    if (!d_r || !d_x || !d_f || H < 3 || W < 3) return set_err(PGMG_ERR_ARG, "pgmg_residual: bad argument");
    launch_g_residual(d_r, d_x, d_f, 1.0 / (h * h), H, W, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

int pgmg_restrict(const double *d_fine, double *d_coarse, int Nf, int Nc, void *stream)
{
    if (!d_fine || !d_coarse || Nc < 3 || Nf != 2 * Nc - 1)
        return set_err(PGMG_ERR_ARG, "pgmg_restrict: need Nf == 2*Nc - 1");
    launch_g_restrict(d_fine, d_coarse, Nf, Nc, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

int pgmg_prolong(const double *d_coarse, double *d_fine, int Nc, int Nf, int mode, void *stream)
{
    return pgmg_prolong_grid(d_coarse, d_fine, Nc, Nf, mode, 0, stream);
}

int pgmg_prolong_grid(const double *d_coarse, double *d_fine, int Nc, int Nf, int mode,
                      int num_thread, void *stream)
{
    if (!d_fine || !d_coarse || Nc < 3 || Nf != 2 * Nc - 1 || (mode != 0 && mode != 1) ||
        num_thread < 0)
        return set_err(PGMG_ERR_ARG, "pgmg_prolong: need Nf == 2*Nc - 1, mode 0|1, num_thread >= 0");
    // ComputeProlungator's launch: max(1, fine_N / num_thread) blocks of num_thread per side
    const int ext = num_thread > 0 ? std::max(1, Nf / num_thread) * num_thread : Nf;
    launch_g_prolong(d_coarse, d_fine, Nc, Nf, mode, ext, (hipStream_t)stream);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

int pgmg_norm(const double *d_v, long long n, double *result, void *stream)
{
    if (!d_v || n < 0 || !result) return set_err(PGMG_ERR_ARG, "pgmg_norm: bad argument");
    hipStream_t s = (hipStream_t)stream;
    OpScratch *op = nullptr;
    int e = ensure_scratch(s, 0, &op);
    if (e) return e;
    OpScratch &g_op = *op;
    long long nb = (n + kBlock - 1) / kBlock;
    if (nb > 1024) nb = 1024;   // <= kOpPartialsCap
    if (nb < 1) nb = 1;
    launch_g_sumsq(d_v, n, g_op.partials, (int)nb, s);
    launch_sum_partials(g_op.partials, (int)nb, g_op.scalar, s);
    double sum = 0.0;
    HIPC(hipMemcpyAsync(&sum, g_op.scalar, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    *result = std::sqrt(sum);
    return PGMG_OK;
}

int pgmg_rhs(double *d_f, int W, int H, double h, double a, double p, double q, void *stream)
{
    if (!d_f || W < 1 || H < 1) return set_err(PGMG_ERR_ARG, "pgmg_rhs: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const double factor = (M_PI * M_PI / (a * a)) * (p * p + q * q);  // DynamicGridUtils.hpp:113
    std::vector<double> t(W + H);
    for (int i = 0; i < W; ++i) t[i] = std::sin(p * M_PI * (i * h) / a);
    for (int j = 0; j < H; ++j) t[W + j] = std::sin(q * M_PI * (j * h) / a);
    double *d = nullptr;
    HIPC(hipMalloc((void **)&d, t.size() * sizeof(double)));
    HIPC(hipMemcpy(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    launch_g_rhs(d_f, d, d + W, factor, W, H, s);
    HIPC(hipStreamSynchronize(s));
    HIPC(hipFree(d));
    return PGMG_OK;
}

int pgmg_ops_release(void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    OpScratch o;
    {
        std::lock_guard<std::mutex> lk(g_op_mu);
        auto it = g_ops.find(s);
        if (it == g_ops.end()) return PGMG_OK;
        o = it->second;
        g_ops.erase(it);
    }
    HIPC(hipStreamSynchronize(s));   // ops still queued on s may use the set
    for (void *p : {(void *)o.partials, (void *)o.flags, (void *)o.stats, (void *)o.scalar,
                    (void *)o.tmp, (void *)o.side, (void *)o.mon, (void *)o.exd, (void *)o.grad})
        if (p) HIPC(hipFree(p));
    return PGMG_OK;
}

int pgmg_device_alloc(void **ptr, size_t bytes)
{
    if (!ptr) return set_err(PGMG_ERR_ARG, "null ptr");
    if (hipMalloc(ptr, bytes) != hipSuccess) return set_err(PGMG_ERR_NOMEM, "hipMalloc failed");
    return PGMG_OK;
}

int pgmg_device_free(void *ptr)
{
    HIPC(hipFree(ptr));
    return PGMG_OK;
}

int pgmg_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    HIPC(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PGMG_OK;
}

int pgmg_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PGMG_OK;
}

int pgmg_device_sync(void)
{
    HIPC(hipDeviceSynchronize());
    return PGMG_OK;
}

int pgmg_device_count(int *n)
{
    if (!n) return set_err(PGMG_ERR_ARG, "null n");
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) {
        *n = 0;
        return set_err(PGMG_ERR_HIP, hipGetErrorString(e));
    }
    return PGMG_OK;
}

}  // extern "C"
