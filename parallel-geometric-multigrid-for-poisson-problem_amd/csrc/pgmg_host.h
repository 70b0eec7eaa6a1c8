// pgmg_host.h — shared by the orchestration's files (mapped in pgmg_ctx.hip's header): error
// macros, the functions that cross a file boundary, the argument-block builders they share.  Host only.
#pragma once
#include "pgmg_ctx.h"
#include "pgmg_fused.h"

#define PGMG_TRY(expr)            \
    do {                          \
        const int e_ = (expr);    \
        if (e_) return e_;        \
    } while (0)
#define HIPC(expr) PGMG_HIPC(expr)

namespace pgmg {

// Wait for the context's stream.  On row strips through the transport's wait, which polls
// RCCL's asynchronous error state and gives up after cfg.comm_timeout_s instead of hanging
// on a dead or stuck peer.
inline int stream_wait(pgmg_ctx *c)
{
    if (c->comm) return c->comm->wait(c->s);
    PGMG_HIPC(hipStreamSynchronize(c->s));
    return PGMG_OK;
}

// held by run_cycles and pgmg_fcycle: c->call is clear again on every exit path
struct CallScope {
    pgmg_ctx *c;
    ~CallScope() { c->call = CallState{}; }
};

// --- pgmg_mem.hip
bool registered_span(intptr_t lo, intptr_t hi);   // is [lo, hi) inside ONE registered allocation?
bool is_device_ptr(const void *p);
// p lies in a shuffled (virtual-memory-mapped) grid: the runtime's 2D copies and memsets refuse
// those ranges, so every grid transfer checks and takes a kernel or a 1D copy instead
bool is_vmm(const void *p);

// --- pgmg_cycle.hip
// k_post row range of a fused level: the strip, or on distributed levels below the finest
// the strip plus kPostExt rows past each edge (see enqueue_fused_level)
struct PostRows {
    int jc0, jc1, row_lo, row_hi;
};
PostRows post_rows(const pgmg_ctx *c, int l);
// partial sums a tile pass of bulk level l writes on this rank (0: no tile pass there);
// pre: the rank's coarse rows, post: its k_post rows (post_rows)
int tile_np(const pgmg_ctx *c, int l, bool post);
struct StripRows {
    int jc0, jc1;         // coarse-row segments [jc0, jc1)
    int row_lo, row_hi;   // fine rows this rank writes
    int rc_lo, rc_hi;     // coarse rows this rank restricts into
    int x_lo, x_hi;       // rows of the rare-path scratch S (row_lo - 4 .. row_hi + 4)
};
StripRows strip_rows(const Level &L, const Level &C);
// A log slice for one check of mode `mode` (nullptr outside speculative calls; an in-stream
// check is logged -- its norm only, for the per-level policy -- on one GPU)
double *chk_log(pgmg_ctx *c, int np, int level, int mode);
// dispatchers on the element type (enqueue_cycle, enqueue_tail: pgmg_ctx.h)
int enqueue_smooth(pgmg_ctx *c, int l, int which, int v, bool x0_zero);
// pin: F-cycle climb; fr2_want: the finest k_post also forms level 2's restriction (k_post_r2)
int enqueue_fused_level(pgmg_ctx *c, int l, int gamma, bool x0_zero, bool pin, bool fr2_want);
int enqueue_last_post(pgmg_ctx *c);
int run_cycles_plain(pgmg_ctx *c, int ncycles, int gamma, bool rec0 = true);

// --- pgmg_spec.hip
// log doubles and checks of one visit of level l >= 1 (the tail decides in-kernel)
void spec_need_level(pgmg_ctx *c, int l, int gamma, long long *dbl, long long *nchk);
int spec_reserve(pgmg_ctx *c, long long dbl, long long nchk);
int spec_validate(pgmg_ctx *c, unsigned *h_out, bool *overflow_out, int n_any);
int run_cycles_spec(pgmg_ctx *c, int ncycles, int gamma);
// a speculative segment's opening: stats_bk = stats (4 words), flags[0, nflags) = 0
// (also opens the F-cycle's segments, pgmg_fcycle.hip)
void launch_spec_open(const unsigned long long *stats, unsigned long long *stats_bk, unsigned *flags,
                      int nflags, hipStream_t s);

// --- pgmg_ctx.hip
void sine_tables(const pgmg_config &cfg, int N, double h, std::vector<double> &sx,
                 std::vector<double> &sy, double &factor);
// a device-bound problem: the context's stream starts after the caller's null-stream work
int order_after_caller(pgmg_ctx *c);
int ext_stage_in(pgmg_ctx *c, bool inplace);
int ext_stage_out(pgmg_ctx *c);
// phi and f of c <- the injections (every second row and column) of two device arrays
int set_problem_injected(pgmg_ctx *c, const double *phi_src, long long Pphi, const double *f_src,
                         long long Pf, hipStream_t s);

// the level-0 right-hand side grid was written on the device (pgmg_project's divergence): the
// state pgmg_set_problem(the current phi, that f) leaves.  c's stream is idle
int set_problem_rhs_on_device(pgmg_ctx *c);
// its fp32 sibling (pgmg_solve_mixed's child): the level-0 f grid of the fp32, one-GPU,
// context-owned c holds the new f (written on another stream, which the host has waited for);
// phi becomes zero.  Enqueued on c's stream: nothing waits
int set_problem_zero_rhs_on_device_f32(pgmg_ctx *c);

// --- pgmg_extrap.hip
// points per side of the coarsest level below N
int coarsest_n(int N, int n_coarse);

// --- pgmg_gradient.hip
// c->grad_buf holds np partial sums and their total (at grad_buf + grad_cap)
int grad_reserve(pgmg_ctx *c, int np);

// --- pgmg_vorticity.hip
// The two passes of the vorticity transport (include/pgmg.h "Vorticity transport"), fp64, element
// (0, 0) and pitch (elements) of every array.  launch_vort_step: out = the explicit Euler step of
// omega (w) under psi on the interior, w's frame on the frame, on grad_grid(N); vmax non-null:
// gradient_blocks(N) per-workgroup maxima of |psi_x| + |psi_y| to `partials` and one more launch
// their maximum to vmax[0].  launch_vort_wall: w's frame from psi (mode PGMG_WALL_NOSLIP, walls =
// ub, ut, vl, vr) or +0.0 (PGMG_WALL_FREE).  No span checks here (launch_extrap's rule).
// vort_step_error / vort_wall_error: what the entries refuse in dt and nu, in the mode and the wall
// speeds (nullptr: nothing).
void launch_vort_step(const double *psi, long long Pp, const double *w, long long Pw, double *out,
                      long long Po, int N, double h, double dt, double nu, double *partials,
                      double *vmax, hipStream_t s);
void launch_vort_wall(const double *psi, long long Pp, double *w, long long Pw, int N, double h,
                      int mode, const double walls[4], hipStream_t s);
const char *vort_step_error(double dt, double nu);
const char *vort_wall_error(int mode, const double walls[4]);
// what pgmg_boussinesq.hip takes over: k_vort_max on np partials, the events c->vt_ev, and what
// the context entries refuse after their arguments (`who` names the entry)
void launch_vort_max(const double *partials, int np, double *vmax, hipStream_t s);
int vort_events(pgmg_ctx *c);
int vort_state_check(pgmg_ctx *c, const std::string &who);
// the time loop of pgmg_vorticity_step (order 1) and pgmg_vorticity_step_rk: every refusal of the
// two entries under the name `who`, then nsteps steps of `order` stages
int vort_advance(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, double dt, double nu, int mode,
                 const double walls[4], int order, int nsteps, pgmg_vort_info *info,
                 const std::string &who);

// --- pgmg_vort_rk.hip
// A Runge-Kutta stage in Shu-Osher form (include/pgmg.h "Runge-Kutta vorticity transport"), under
// launch_vort_step's conventions: out = a * w0 + b * (the Euler step of w under psi) on the
// interior, w's frame on the frame; w0 may be w; vmax as in launch_vort_step
void launch_vort_stage(const double *psi, long long Pp, const double *w, long long Pw,
                       const double *w0, long long P0, double *out, long long Po, int N, double h,
                       double dt, double nu, double a, double b, double *partials, double *vmax,
                       hipStream_t s);

// --- pgmg_boussinesq.hip
// The two passes of the buoyancy-driven flow (include/pgmg.h "Buoyancy-driven flow"), fp64,
// element (0, 0) and pitch (elements) of every array.  launch_bouss_step: wout and tout = the
// explicit Euler steps of w and T under psi with the buoyancy source in w's, on grad_grid(N);
// vmax as in launch_vort_step.  launch_scalar_wall: T's adiabatic walls (mask of PGMG_TWALL_*) in
// place.  No span checks here (launch_extrap's rule).  bouss_step_error / scalar_wall_error: what
// the entries refuse in kappa and buoy, in the mask (nullptr: nothing).
void launch_bouss_step(const double *psi, long long Pp, const double *w, long long Pw, const double *T,
                       long long Pt, double *wout, long long Pwo, double *tout, long long Pto, int N,
                       double h, double dt, double nu, double kappa, const double buoy[2],
                       double *partials, double *vmax, hipStream_t s);
void launch_scalar_wall(double *T, long long Pt, int N, unsigned adiabatic, hipStream_t s);
const char *bouss_step_error(double kappa, const double buoy[2]);
const char *scalar_wall_error(unsigned adiabatic);
// *q = n doubles of zeroed, registered device memory unless it is set already (the scratch arrays
// of the entries here and in pgmg_bouss_rk.hip; pgmg_destroy frees them)
int bouss_alloc(pgmg_ctx *c, double **q, size_t n, const char *what);
// the time loop of pgmg_boussinesq_step (order 1) and pgmg_boussinesq_step_rk: every refusal of
// the two entries under the name `who`, then nsteps steps of `order` stages
int bouss_advance(pgmg_ctx *c, const pgmg_solve_opts *o, double omega, const pgmg_bouss_params *p,
                  double *d_T, int order, int nsteps, pgmg_bouss_info *info, const std::string &who);

// --- pgmg_bouss_rk.hip
// A Runge-Kutta stage in Shu-Osher form (include/pgmg.h "Runge-Kutta buoyancy-driven flow"), under
// launch_bouss_step's conventions: wout = a * w0 + b * (the Euler step of w under psi and T) and
// tout = a * T0 + b * (the Euler step of T) on the interior, w's and T's frames on the frames; w0
// may be w and T0 may be T; vmax as in launch_vort_step.  No span checks here
void launch_bouss_stage(const double *psi, long long Pp, const double *w, long long Pw, const double *T,
                        long long Pt, const double *w0, long long Pw0, const double *T0, long long Pt0,
                        double *wout, long long Pwo, double *tout, long long Pto, int N, double h,
                        double dt, double nu, double kappa, const double buoy[2], double a, double b,
                        double *partials, double *vmax, hipStream_t s);

// --- pgmg_monitor.hip
// the damping pass on a level of the FMG pyramid (no norm, nothing waits); fmg_damp_reserve
// sizes the context's side buffer and partials for a level of N points beforehand
int fmg_damp_reserve(pgmg_ctx *c, int N);
int fmg_damp_level(pgmg_ctx *c, const Grid &u, const Grid &f, const Level &L, double omega, bool gen);
// c->mon_buf holds the partials of np workgroups and the three totals (at mon_buf + 3 * mon_cap);
// side: bytes of the damping pass's side buffer (0: none needed)
int mon_reserve(pgmg_ctx *c, int np, size_t side);

// the tail launch's arguments every caller shares (visits, x0_from_global, fmg_*: the caller's)
template <class T>
inline TailArgsT<T> tail_args(const pgmg_ctx *c)
{
    const Level &Lt = c->lv[c->nb];
    TailArgsT<T> t{};
    t.f_top = G<T>(Lt.F);
    t.e_top = G<T>(Lt.A);
    t.P_top = Lt.P;
    t.N_top = Lt.N;
    t.h_top = Lt.h;
    t.v1 = c->cfg.v1;
    t.v2 = c->cfg.v2;
    t.coarse_iter = c->cfg.coarse_iter;
    t.n_coarse = c->cfg.n_coarse;
    t.eps = c->cfg.eps;
    t.stats = c->stats;
    return t;
}

// level geometry of a fused pass's argument block on level L above C (its strip's rows)
template <class Args>
inline StripRows pass_geometry(Args &a, const Level &L, const Level &C)
{
    using T = decltype(a.hh);
    const StripRows sr = strip_rows(L, C);
    a.hh = (T)L.hh;
    a.ih = (T)L.ih;
    a.N = L.N;
    a.P = L.P;
    a.Nc = C.N;
    a.Pc = C.P;
    a.jc0 = sr.jc0;
    a.jc1 = sr.jc1;
    a.row_lo = sr.row_lo;
    a.row_hi = sr.row_hi;
    return sr;
}

// ... of a k_postpre-shaped pass (k_postpre, fused smooth(3))
template <class T>
inline void postpre_geometry(PostPreArgsT<T> &q, const Level &L, const Level &C)
{
    const StripRows sr = pass_geometry(q, L, C);
    q.rc_lo = sr.rc_lo;
    q.rc_hi = sr.rc_hi;
}

}  // namespace pgmg
