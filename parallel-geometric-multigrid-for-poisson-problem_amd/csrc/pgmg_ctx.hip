// pgmg_ctx.hip — the context behind the C ABI: creation, problems, the cycle entries, queries.
//
// Replaces the reference's ParallelMultiGridSolver (3_part_parallel/Parallel_Mg.cu)
// and the allocation/timing plumbing of ParallelTestRunner::run_v_cycle
// (3_part_parallel/ParallelTestRunner.cu:152-186), MI355X-first:
//   * the whole level pyramid is allocated once in HBM (no per-level, per-cycle
//     cudaMallocManaged, no unified-memory migration, no host sync per kernel);
//   * each bulk level (N > tail_n) is 2 pre sweeps + fused residual/restriction
//     + prolongation + 2 post sweeps on ping-pong buffers; the smoother's
//     per-sweep early exit (Smoother.hpp:75-88) is evaluated on the device by
//     speculating the next sweep and undoing it when the check fires;
//   * the coarse end (N <= tail_n) is one LDS-resident workgroup (pgmg_tail.hip);
//   * a V-cycle is captured once into a hipGraph and replayed.
//
// Row strips: every per-level array is addressed through a "virtual origin"
// pointer o with element (global row j, column i) at o[j*P + i]; a rank only
// allocates its owned rows plus two halo rows each side, so all kernels work in
// global row numbers and the fine/coarse row parity (j = 2 jc) is preserved.
//
// Map of the orchestration (host code, five files sharing pgmg_host.h) by section title:
//   pgmg_ctx.hip     create/destroy, set_problem*, device-resident problems (staging),
//                    run_cycles, set_eps, solution / statistics / timing queries, bench entries
//   pgmg_mem.hip     allocation registry, span checks, "Shuffled physical placement", grids
//   pgmg_cycle.hip   check log, "W-cycle plans", the V/W kernel sequences, cross-cycle fusion
//                    of the finest level and the "carry", run_cycles_plain
//   pgmg_spec.hip    "speculative calls": reply_wait and the pinned reply, the per-level policy
//                    and "predicted to fire", segment planning, run_cycles_spec, its queries
//   pgmg_fcycle.hip  the F-cycle, "speculative F-cycles", pgmg_fcycle
//   pgmg_monitor.hip the convergence monitor (its kernel too), pgmg_solve and its history; the
//                    stop rule itself is the HIP-free pgmg_stop.h
//   pgmg_fmg.hip     full multigrid for the problem's own f: the cubic interpolation pass (its
//                    kernel too), the restricted f chain, the climb, pgmg_fmg
//   pgmg_extrap.hip  fourth-order solves: the half-resolution context, the injection and the two
//                    extrapolation passes (their kernels too), pgmg_solve_extrap
#include <cxxabi.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pgmg_host.h"

using namespace pgmg;

static thread_local std::string g_err;

int pgmg::set_err(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

static bool is_pow2p1(int N)
{
    if (N < 3) return false;
    const int g = N - 1;
    return (g & (g - 1)) == 0;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char *pgmg_last_error(void) { return g_err.c_str(); }
const char *pgmg_version(void) { return "pgmg 0.2 (gfx950, fp64 | fp32, row-strip RCCL)"; }

int pgmg_config_default(pgmg_config *cfg, int N)
{
    if (!cfg) return set_err(PGMG_ERR_ARG, "null cfg");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->N = N;
    cfg->v1 = 1;           // MultiGrid.hpp:15
    cfg->v2 = 1;           // MultiGrid.hpp:16
    cfg->coarse_iter = 10; // MultiGrid.hpp:61
    cfg->n_coarse = 5;     // MultiGrid.hpp:19
    cfg->alpha = 3;        // 2_part_MG/main.cpp:15
    cfg->eps = 1e-7;       // 2_part_MG/main.cpp:12
    cfg->a = 1.0;          // globals.cpp:2-4
    cfg->p = 1.0;
    cfg->q = 1.0;
    cfg->tail_n = kTailMaxN;
    cfg->device = 0;
    cfg->flags = 0;
    cfg->rank = 0;
    cfg->world = 1;
    cfg->nccl_unique_id = nullptr;
    cfg->gather_n = 1025;
    cfg->precision = PGMG_PRECISION_FP64;
    cfg->cross_min_n = 2049;
    cfg->spec_segment = 0;
    cfg->comm_timeout_s = 600.0;
    cfg->h0 = 0.0;
    return PGMG_OK;
}

int pgmg_destroy(pgmg_ctx *c)
{
    if (!c) return PGMG_OK;
    if (c->s) (void)hipStreamSynchronize(c->s);
    if (c->gexec) (void)hipGraphExecDestroy(c->gexec);
    for (auto &L : c->lv) {
        free_grid(L.A);
        free_grid(L.B);
        free_grid(L.F);
    }
    if (c->partials) (void)hipFree(c->partials);
    if (c->partials2) (void)hipFree(c->partials2);
    if (c->partials3) (void)hipFree(c->partials3);
    if (c->rhs_tab) (void)hipFree(c->rhs_tab);
    if (c->mon_tab) (void)hipFree(c->mon_tab);
    if (c->mon_buf) (void)hipFree(c->mon_buf);
    if (c->mon_side) (void)hipFree(c->mon_side);
    if (c->fmg_gtab) (void)hipFree(c->fmg_gtab);
    if (c->uflags) (void)hipFree(c->uflags);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->plog) (void)hipFree(c->plog);
    if (c->chk_norm) (void)hipFree(c->chk_norm);
    if (c->mark_dev) (void)hipFree(c->mark_dev);
    if (c->stats_bk) (void)hipFree(c->stats_bk);
    free_grid(c->bk);
    free_grid(c->ftop);
    if (c->ppflags) (void)hipFree(c->ppflags);
    free_grid(c->S);
    free_grid(c->Ffmg);
    for (auto &g : c->Ffmg_l) free_grid(g);
    for (auto &g : c->fmg_F) free_grid(g);
    for (auto &g : c->fmg_U) free_grid(g);
    if (c->fmg_frame) {
        unregister_alloc(c->fmg_frame);
        (void)hipFree(c->fmg_frame);
    }
    if (c->ex_child) (void)pgmg_destroy(c->ex_child);
    if (c->ex_D) {
        unregister_alloc(c->ex_D);
        (void)hipFree(c->ex_D);
    }
    if (c->mx_child) (void)pgmg_destroy(c->mx_child);
    for (hipEvent_t e : c->mx_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->grad_buf) (void)hipFree(c->grad_buf);
    if (c->grad_out) {
        unregister_alloc(c->grad_out);
        (void)hipFree(c->grad_out);
    }
    if (c->pj_out) {
        unregister_alloc(c->pj_out);
        (void)hipFree(c->pj_out);
    }
    free_grid(c->vt_out);
    if (c->vt_scr) {
        unregister_alloc(c->vt_scr);
        (void)hipFree(c->vt_scr);
    }
    for (hipEvent_t e : c->vt_ev)
        if (e) (void)hipEventDestroy(e);
    free_grid(c->vt_w0);
    for (double *q : {c->vt_rk_scr, c->bq_tout, c->bq_scr, c->bq_t0, c->bq_rk_scr})
        if (q) {
            unregister_alloc(q);
            (void)hipFree(q);
        }
    if (c->pj_ev0) (void)hipEventDestroy(c->pj_ev0);
    if (c->pj_ev1) (void)hipEventDestroy(c->pj_ev1);
    if (c->ex_ev0) (void)hipEventDestroy(c->ex_ev0);
    if (c->ex_ev1) (void)hipEventDestroy(c->ex_ev1);
    if (c->fmg_tab) (void)hipFree(c->fmg_tab);
    if (c->flags) (void)hipFree(c->flags);
    if (c->stats) (void)hipFree(c->stats);
    if (c->scalar) (void)hipFree(c->scalar);
    for (auto &pool : c->tpool)
        for (auto e : pool.ev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_caller) (void)hipEventDestroy(c->ev_caller);
    delete c->comm;
    if (c->s) (void)hipStreamDestroy(c->s);
    delete c;
    return PGMG_OK;
}

int pgmg_create(pgmg_ctx **out, const pgmg_config *cfg)
{
    if (!out || !cfg) return set_err(PGMG_ERR_ARG, "null argument");
    *out = nullptr;
    if (!is_pow2p1(cfg->N) || cfg->N < 5)
        return set_err(PGMG_ERR_ARG, "N must be 2^k + 1 with N >= 5 (2_part_MG/main.cpp:6)");
    if (cfg->v1 < 0 || cfg->v2 < 0 || cfg->v1 + 1 >= kMaxSweeps || cfg->v2 + 1 >= kMaxSweeps ||
        cfg->coarse_iter < 0 || cfg->n_coarse < 3 || cfg->alpha < 1)
        return set_err(PGMG_ERR_ARG, "bad smoother/cycle parameters");
    // the tail's visit counters are 4 bits per level (pgmg_tail.hip, tail_gcycle): with
    // alpha >= 16 a count wraps to 0 and the W-cycle would never leave the level
    if (cfg->alpha > 15)
        return set_err(PGMG_ERR_ARG, "alpha must be at most 15 (include/pgmg.h)");
    {
        // the coarsest level (the first N_l <= n_coarse) is the smallest the tail's top level
        // can be, whatever tail_n says; the tail holds at most kTailMaxN points per side in LDS
        int Nl = cfg->N;
        while (Nl > cfg->n_coarse) Nl = (Nl - 1) / 2 + 1;
        if (Nl > kTailMaxN)
            return set_err(PGMG_ERR_ARG, "n_coarse too large: the coarsest level must have at "
                                         "most 65 points per side (include/pgmg.h)");
    }
    if (cfg->world < 1 || cfg->rank < 0 || cfg->rank >= cfg->world)
        return set_err(PGMG_ERR_ARG, "bad rank/world");
    if (cfg->precision != PGMG_PRECISION_FP64 && cfg->precision != PGMG_PRECISION_FP32)
        return set_err(PGMG_ERR_ARG, "precision must be PGMG_PRECISION_FP64 or _FP32");
    if (!(cfg->h0 >= 0.0) || !std::isfinite(cfg->h0))
        return set_err(PGMG_ERR_ARG, "h0 must be finite and >= 0 (0: a / (N - 1))");
    // a divides in every sine table and in the right-hand side's factor: a = 0 or a non-finite
    // a, p or q makes them NaN / Inf, and with them every result of the context
    if (!std::isfinite(cfg->a) || cfg->a == 0.0)
        return set_err(PGMG_ERR_ARG, "a must be finite and not 0 (include/pgmg.h)");
    if (!std::isfinite(cfg->p) || !std::isfinite(cfg->q))
        return set_err(PGMG_ERR_ARG, "p and q must be finite (include/pgmg.h)");
    if (cfg->flags & PGMG_FLAGS_RETIRED)
        return set_err(PGMG_ERR_ARG, "retired PGMG_FLAG_* bit (8192 / 16384; include/pgmg.h): "
                                     "PGMG_FLAG_NO_SPEC_FIRE is 32768 since r04");
    int ndev = 0;
    HIPC(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return set_err(PGMG_ERR_ARG, "bad device ordinal");
    HIPC(hipSetDevice(cfg->device));

    pgmg_ctx *c = new pgmg_ctx();
    c->cfg = *cfg;
    c->fp32 = cfg->precision == PGMG_PRECISION_FP32;
    // one GPU: the big grids from shuffled physical chunks (vmm_alloc); row strips keep plain
    // device memory (what RCCL's transfers were validated on)
    c->shuffle = cfg->world <= 1 && !(cfg->flags & PGMG_FLAG_NO_SHUFFLE);
    int tail_n = cfg->tail_n;
    if (tail_n > kTailMaxN) tail_n = kTailMaxN;
    if (tail_n < cfg->n_coarse) tail_n = cfg->n_coarse;
    c->cfg.tail_n = tail_n;

    // level sizes: bulk while N > tail_n, then the tail's top level
    int N = cfg->N;
    // MultiGridTestRunner.hpp:131, or the caller's h (MultiGrid.hpp:57's argument)
    double h = cfg->h0 > 0.0 ? cfg->h0 : cfg->a / (N - 1);
    for (;;) {
        Level L;
        L.N = N;
        L.es = c->fp32 ? 4 : 8;
        L.P = c->fp32 ? pitch_elems<float>(N) : pitch_elems<double>(N);
        L.h = h;
        L.hh = h * h;
        L.ih = 1.0 / (h * h);
        L.lo = 0;
        L.hi = N;
        L.u0 = 1;
        L.u1 = N - 1;
        c->lv.push_back(L);
        if (N <= tail_n || N <= cfg->n_coarse) break;
        N = (N - 1) / 2 + 1;
        h = 2 * h;  // MultiGrid.hpp:83
    }
    c->nb = (int)c->lv.size() - 1;

    int rc = PGMG_OK;
    if (cfg->world > 1) {
        c->comm = Comm::create(c, &rc);
        if (!c->comm) {
            pgmg_destroy(c);
            return rc;
        }
        rc = c->comm->plan(c);
        if (rc == 1) {  // grid too small to split: every rank runs an independent replica
            delete c->comm;
            c->comm = nullptr;
            rc = PGMG_OK;
        }
    }

    // (measurement build: PGMG_DUMMY_MB a dummy buffer of that size before every level grid:
    // placement probes)
    Grid dummy;
    if (tuning_int("PGMG_DUMMY_MB", 0) > 0) {
        Level Ld = c->lv[0];
        Ld.hi = Ld.lo + (int)(((size_t)tuning_int("PGMG_DUMMY_MB", 0) << 20) / ((size_t)Ld.P * Ld.es));
        rc = alloc_grid(dummy, Ld);
    }
    for (int l = 0; l < (int)c->lv.size() && rc == PGMG_OK; ++l) {
        Level &L = c->lv[l];
        if (!L.on_this_rank) continue;
        // (measurement build: PGMG_GRID_STAGGER bytes times a per-grid index of level 0)
        const size_t st = l == 0 ? (size_t)tuning_int("PGMG_GRID_STAGGER", 0) : 0;
        rc = alloc_grid(L.A, L, 0 * st, c->shuffle);
        if (rc == PGMG_OK) rc = alloc_grid(L.F, L, 1 * st, c->shuffle);
        if (rc == PGMG_OK && l < c->nb) rc = alloc_grid(L.B, L, 2 * st, c->shuffle);
    }
    c->fused = cfg->v1 == 1 && cfg->v2 == 1 && !(cfg->flags & PGMG_FLAG_UNFUSED);
    c->recompute = !(cfg->flags & PGMG_FLAG_NO_RECOMPUTE);
    {
        const int cross_min = cfg->cross_min_n > 0 ? cfg->cross_min_n : 2049;
        c->cross = c->fused && c->nb >= 1 && c->lv[0].N >= cross_min &&
                   !(cfg->flags & PGMG_FLAG_NO_CROSS);
    }
    int maxblocks = 256;
    for (int l = 0; l < c->nb; ++l) {
        int rpb, gx, gy;
        const Level &L = c->lv[l];
        int nbk = sweep_blocks(L.N, L.u0, L.u1, &rpb, &gx, &gy);
        if (nbk > maxblocks) maxblocks = nbk;
        nbk = fused_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2);
        if (nbk > maxblocks) maxblocks = nbk;
        const PostRows pr = post_rows(c, l);
        nbk = fused_blocks(L.N, pr.jc0, pr.jc1);
        if (nbk > maxblocks) maxblocks = nbk;
        nbk = postpre_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2);
        if (nbk > maxblocks) maxblocks = nbk;
        nbk = postpre_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2, true);
        if (nbk > maxblocks) maxblocks = nbk;
        nbk = std::max(tile_np(c, l, false), tile_np(c, l, true));
        if (nbk > maxblocks) maxblocks = nbk;
        // k_post_r2 (the finest k_post of consecutive F-cycles, 116-column stride): its
        // partials may land in c->partials when the check log is full
        if (l == 0) {
            nbk = post_r2_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2);
            if (nbk > maxblocks) maxblocks = nbk;
        }
    }
    const size_t st0 = (size_t)tuning_int("PGMG_GRID_STAGGER", 0);
    if (rc == PGMG_OK && c->cross) rc = alloc_grid(c->S, c->lv[0], 3 * st0, c->shuffle);
    (void)dummy;   // (the probe's dummy buffer stays allocated: the context leaks it)
    // partial sums of k_postpre's second and third checks (cross-cycle fusion, and the
    // F-cycle's fused smooth(3)), its decision flags
    if (rc == PGMG_OK && (hipMalloc((void **)&c->partials2, sizeof(double) * maxblocks) != hipSuccess ||
                          hipMalloc((void **)&c->partials3, sizeof(double) * maxblocks) != hipSuccess ||
                          hipMalloc((void **)&c->ppflags, 4 * sizeof(unsigned)) != hipSuccess))
        rc = set_err(PGMG_ERR_NOMEM, "cross-cycle buffers");
    c->partials_cap = maxblocks;
    if (rc == PGMG_OK && hipMalloc((void **)&c->partials, sizeof(double) * maxblocks) != hipSuccess)
        rc = set_err(PGMG_ERR_NOMEM, "partials");
    const size_t nflags = (size_t)(c->lv.size() + 1) * 2 * kMaxSweeps;
    if (rc == PGMG_OK && hipMalloc((void **)&c->flags, sizeof(unsigned) * nflags) != hipSuccess)
        rc = set_err(PGMG_ERR_NOMEM, "flags");
    if (rc == PGMG_OK && hipMalloc((void **)&c->stats, 4 * sizeof(unsigned long long)) != hipSuccess)
        rc = set_err(PGMG_ERR_NOMEM, "stats");
    if (rc == PGMG_OK && hipMalloc((void **)&c->scalar, 8 * sizeof(double)) != hipSuccess)
        rc = set_err(PGMG_ERR_NOMEM, "scalar");
    if (rc == PGMG_OK) {
        if (hipMemset(c->flags, 0, sizeof(unsigned) * nflags) != hipSuccess ||
            hipMemset(c->stats, 0, 4 * sizeof(unsigned long long)) != hipSuccess ||
            hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming) != hipSuccess)
            rc = set_err(PGMG_ERR_HIP, "stream/event setup failed");
    }
    if (rc == PGMG_OK && (cfg->flags & PGMG_FLAG_TIME_FINE)) {
        for (auto &pool : c->tpool) {
            pool.ev.resize(512);
            for (auto &e : pool.ev)
                if (hipEventCreate(&e) != hipSuccess) rc = set_err(PGMG_ERR_HIP, "event pool");
        }
    }
    if (rc == PGMG_OK && c->comm) rc = c->comm->setup(c);
    c->spec = c->fused && (c->cross || c->comm != nullptr) && !(cfg->flags & PGMG_FLAG_EXACT_DIST);
    if (rc != PGMG_OK) {
        pgmg_destroy(c);
        return rc;
    }
    *out = c;
    return PGMG_OK;
}

}  // extern "C"

// host sine tables -> bit-identical compute_rhs on the device
void pgmg::sine_tables(const pgmg_config &cfg, int N, double h, std::vector<double> &sx,
                       std::vector<double> &sy, double &factor)
{
    factor = (M_PI * M_PI / (cfg.a * cfg.a)) * (cfg.p * cfg.p + cfg.q * cfg.q);
    sx.resize(N);
    sy.resize(N);
    for (int i = 0; i < N; ++i) {
        const double x = i * h;
        sx[i] = std::sin(cfg.p * M_PI * x / cfg.a);
        sy[i] = std::sin(cfg.q * M_PI * x / cfg.a);
    }
}

// rows [r0, r1) of a dense host array (pitch N) -> grid g (the context's element type)
static int upload_rows(pgmg_ctx *c, const Level &L, const Grid &g, const double *host, int r0,
                       int r1)
{
    const int N = L.N;
    const size_t rows = (size_t)(r1 - r0);
    if (!c->fp32 && !is_vmm(g.base)) {
        HIPC(hipMemcpy2D(row_ptr(g, r0, L.P, 8), L.P * sizeof(double), host + (size_t)r0 * N,
                         N * sizeof(double), N * sizeof(double), rows, hipMemcpyHostToDevice));
        return PGMG_OK;
    }
    // fp32 (or a shuffled grid): stage the doubles on the device, narrow / place them there
    double *d = nullptr;
    HIPC(hipMalloc((void **)&d, rows * N * sizeof(double)));
    HIPC(hipMemcpy(d, host + (size_t)r0 * N, rows * N * sizeof(double), hipMemcpyHostToDevice));
    if (c->fp32) launch_from_double(d - (size_t)r0 * N, N, G<float>(g), L.P, r0, r1, c->s);
    else launch_from_double(d - (size_t)r0 * N, N, G<double>(g), L.P, r0, r1, c->s);
    HIPC(hipGetLastError());
    PGMG_TRY(stream_wait(c));
    HIPC(hipFree(d));
    return PGMG_OK;
}

int pgmg::download_grid(pgmg_ctx *c, const void *o, int P, int N, double *host)
{
    if (!c->fp32 && is_vmm(o)) {   // a shuffled grid: widen/copy on the device, then 1D
        double *d = nullptr;
        HIPC(hipMalloc((void **)&d, (size_t)N * N * sizeof(double)));
        launch_to_double(static_cast<const double *>(o), P, d, N, 0, N, c->s);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(host, d, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, c->s));
        PGMG_TRY(stream_wait(c));
        HIPC(hipFree(d));
        return PGMG_OK;
    }
    if (!c->fp32) {
        HIPC(hipMemcpy2DAsync(host, N * sizeof(double), o, P * sizeof(double), N * sizeof(double),
                              N, hipMemcpyDeviceToHost, c->s));
        PGMG_TRY(stream_wait(c));
        return PGMG_OK;
    }
    double *d = nullptr;
    HIPC(hipMalloc((void **)&d, (size_t)N * N * sizeof(double)));
    launch_to_double(static_cast<const float *>(o), P, d, N, 0, N, c->s);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(host, d, (size_t)N * N * sizeof(double), hipMemcpyDeviceToHost, c->s));
    PGMG_TRY(stream_wait(c));
    HIPC(hipFree(d));
    return PGMG_OK;
}

// statistics and speculation history of a new problem
static int problem_reset(pgmg_ctx *c)
{
    HIPC(hipMemset(c->stats, 0, 4 * sizeof(unsigned long long)));
    HIPC(hipDeviceSynchronize());
    c->have_problem = true;
    c->carry = false;
    c->hist.reset(c->nb);
    return PGMG_OK;
}

// A captured cycle (pgmg_cycle.hip, run_cycles_plain) holds the tables its level-0 passes
// regenerate f from, or none, in its kernel arguments: after a change between an analytic f and a
// stored one (old: c->rgfx of before the change) it is captured again
static int drop_graph_of_other_rhs(pgmg_ctx *c, const double *old)
{
    if (c->gexec && c->rgfx != old) {
        HIPC(hipGraphExecDestroy(c->gexec));
        c->gexec = nullptr;
    }
    return PGMG_OK;
}

// level-0 right-hand side rows [r0, r1): the host array f, or (f = NULL) the analytic RHS of
// compute_rhs, stored and, unless PGMG_FLAG_STORED_RHS, regenerated by the level-0 passes
static int setup_rhs(pgmg_ctx *c, const double *f, int r0, int r1)
{
    Level &L = c->lv[0];
    const int N = L.N;
    int e;
    c->gen_rhs = false;
    c->rgfx = c->rgsy = nullptr;
    c->analytic = f == nullptr;
    if (f) {
        if ((e = upload_rows(c, L, L.F, f, r0, r1))) return e;
    } else {
        std::vector<double> sx, sy;
        double factor;
        sine_tables(c->cfg, N, L.h, sx, sy, factor);
        double *d = nullptr;
        HIPC(hipMalloc((void **)&d, 2 * N * sizeof(double)));
        HIPC(hipMemcpy(d, sx.data(), N * sizeof(double), hipMemcpyHostToDevice));
        HIPC(hipMemcpy(d + N, sy.data(), N * sizeof(double), hipMemcpyHostToDevice));
        if (c->fp32) launch_rhs(G<float>(L.F), d, d + N, factor, N, L.P, r0, r1, c->s);
        else launch_rhs(G<double>(L.F), d, d + N, factor, N, L.P, r0, r1, c->s);
        HIPC(hipGetLastError());
        PGMG_TRY(stream_wait(c));
        HIPC(hipFree(d));
        // the exact solution's tables for the monitor's error sums (pgmg_monitor.hip): the
        // unscaled sx[i], sy[j] (compute_function's product), padded like the tables below
        {
            const int nx = 8 + N + 1024, ny = 8 + N + 16;
            std::vector<double> tab((size_t)nx + ny, 0.0);
            for (int i = 0; i < N; ++i) tab[8 + i] = sx[i];
            for (int j = 0; j < N; ++j) tab[(size_t)nx + 8 + j] = sy[j];
            if (!c->mon_tab) HIPC(hipMalloc((void **)&c->mon_tab, tab.size() * sizeof(double)));
            HIPC(hipMemcpy(c->mon_tab, tab.data(), tab.size() * sizeof(double),
                           hipMemcpyHostToDevice));
            c->mon_sx = c->mon_tab + 8;
            c->mon_sy = c->mon_tab + nx + 8;
        }
        // tables for regenerating f inside the level-0 passes: fx[i] = factor * sx[i]
        // (the first product of k_rhs's factor * sx[i] * sy[j]) and sy[j], zero-padded
        // past the grid (columns / rows -8 .. N + 1024 / N + 16, like the stored f's
        // zero padding)
        if (!(c->cfg.flags & PGMG_FLAG_STORED_RHS)) {
            const int nx = 8 + N + 1024, ny = 8 + N + 16;
            std::vector<double> tab((size_t)nx + ny, 0.0);
            for (int i = 0; i < N; ++i) tab[8 + i] = factor * sx[i];
            for (int j = 0; j < N; ++j) tab[(size_t)nx + 8 + j] = sy[j];
            if (!c->rhs_tab) HIPC(hipMalloc((void **)&c->rhs_tab, tab.size() * sizeof(double)));
            HIPC(hipMemcpy(c->rhs_tab, tab.data(), tab.size() * sizeof(double),
                           hipMemcpyHostToDevice));
            c->gfx = c->rhs_tab + 8;
            c->gsy = c->rhs_tab + nx + 8;
            c->gen_rhs = true;
            c->rgfx = c->gfx;
            c->rgsy = c->gsy;
        }
    }
    return PGMG_OK;
}

extern "C" {

int pgmg_set_problem(pgmg_ctx *c, const double *phi0, const double *f)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    Level &L = c->lv[0];
    const int N = L.N;
    if (!L.on_this_rank) return set_err(PGMG_ERR_STATE, "level 0 not on this rank");
    // owned rows + the halo rows the fused passes read (every rank has the full host arrays)
    const int r0 = L.lo - kHalo > 0 ? L.lo - kHalo : 0;
    const int r1 = L.hi + kHalo < N ? L.hi + kHalo : N;
    const size_t rows = (size_t)(r1 - r0);
    const size_t pitch = (size_t)L.P * L.es, width = (size_t)N * L.es;
    int e;
    PGMG_TRY(stream_wait(c));
    c->ext_phi = nullptr;   // host arrays: the problem lives in the context again
    c->ext_f = nullptr;
    // phi (and its boundary copy in the ping-pong buffer B)
    // (the rows r0 .. r1 of a level-0 grid are one contiguous range, padding included: zeroed
    // and copied whole with 1D operations, which shuffled grids accept)
    (void)width;
    if (phi0) {
        if ((e = upload_rows(c, L, L.A, phi0, r0, r1))) return e;
    } else {
        HIPC(hipMemset(row_ptr(L.A, r0, L.P, L.es), 0, pitch * rows));
    }
    auto mirror = [&](const Grid &g) -> int {
        HIPC(hipMemcpy(row_ptr(g, r0, L.P, L.es), row_ptr(L.A, r0, L.P, L.es), pitch * rows,
                       hipMemcpyDeviceToDevice));
        return PGMG_OK;
    };
    if (c->nb > 0) PGMG_TRY(mirror(L.B));
    // the cross-cycle rare-path scratch S mirrors phi's boundary too (its passes never
    // write boundary rows/columns, the k_pre that reads it passes them through)
    if (c->S.base) PGMG_TRY(mirror(c->S));
    const double *const old = c->rgfx;
    if ((e = setup_rhs(c, f, r0, r1))) return e;
    PGMG_TRY(drop_graph_of_other_rhs(c, old));
    return problem_reset(c);
}

int pgmg_set_problem_device(pgmg_ctx *c, double *phi, const double *f)
{
    if (!c || !phi) return set_err(PGMG_ERR_ARG, "null argument");
    if (c->comm) return set_err(PGMG_ERR_STATE, "pgmg_set_problem_device: one GPU only (world 1)");
    if (!is_device_ptr(phi) || (f && !is_device_ptr(f)))
        return set_err(PGMG_ERR_ARG, "pgmg_set_problem_device: phi and f must be device memory");
    Level &L = c->lv[0];
    const int N = L.N;
    PGMG_TRY(stream_wait(c));
    int e;
    const double *const old = c->rgfx;
    if (!f) {
        if ((e = setup_rhs(c, nullptr, 0, N))) return e;
    } else {
        c->gen_rhs = false;
        c->rgfx = c->rgsy = nullptr;
        c->analytic = false;
    }
    PGMG_TRY(drop_graph_of_other_rhs(c, old));
    // in place: a cross-fused fp64 context and phi inside an allocation that covers the rows
    // and columns the finest passes read past the grid (pgmg_alloc_grid's guard)
    const intptr_t o = (intptr_t)phi;
    const long long lo = -(long long)kHalo * N - 8, hi = (long long)(N + kHalo) * N + 8;
    c->ext_inplace = c->cross && !c->fp32 &&
                     registered_span(o + (intptr_t)(lo * 8), o + (intptr_t)(hi * 8));
    c->ext_phi = phi;
    c->ext_f = f;
    return problem_reset(c);
}

int pgmg_problem_device_info(pgmg_ctx *c, int *bound, int *inplace)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (bound) *bound = c->ext_phi != nullptr ? 1 : 0;
    if (inplace) *inplace = c->ext_phi != nullptr && c->ext_inplace ? 1 : 0;
    return PGMG_OK;
}

}  // extern "C"

// A problem from device grids (pgmg_solve_extrap's half-resolution problem): phi and f of the
// fp64, one-GPU context c become the injections phi(j, i) = phi_src(2j, 2i), f(j, i) =
// f_src(2j, 2i) of two device arrays with pitches Pphi and Pf, written on stream s (the stream
// that produced the sources; c's own is idle and waited for) into c's level-0 grids, phi's frame
// mirrored into B and S as pgmg_set_problem does.  The problem is one with a caller's f: nothing
// is regenerated in-kernel and it has no analytic solution.  Returns after s has finished, with
// the statistics and the speculation history reset.
int pgmg::set_problem_injected(pgmg_ctx *c, const double *phi_src, long long Pphi,
                               const double *f_src, long long Pf, hipStream_t s)
{
    if (c->fp32 || c->comm) return set_err(PGMG_ERR_STATE, "injected problem: fp64, one GPU only");
    Level &L = c->lv[0];
    const int N = L.N;
    PGMG_TRY(stream_wait(c));
    PGMG_TRY(check_span(G<double>(L.A), L.P, 8, 0, N - 1, 0, N - 1, "injected problem phi"));
    PGMG_TRY(check_span(G<double>(L.F), L.P, 8, 0, N - 1, 0, N - 1, "injected problem f"));
    c->ext_phi = nullptr;
    c->ext_f = nullptr;
    launch_inject(phi_src, Pphi, G<double>(L.A), L.P, N, s);
    launch_inject(f_src, Pf, G<double>(L.F), L.P, N, s);
    HIPC(hipGetLastError());
    // (rows 0 .. N of a level-0 grid are one contiguous range: see pgmg_set_problem)
    const size_t bytes = (size_t)L.P * L.es * (size_t)N;
    for (const Grid *g : {&L.B, &c->S})
        if (g->base)
            HIPC(hipMemcpyAsync(row_ptr(*g, 0, L.P, L.es), row_ptr(L.A, 0, L.P, L.es), bytes,
                                hipMemcpyDeviceToDevice, s));
    HIPC(hipStreamSynchronize(s));
    c->gen_rhs = false;
    c->rgfx = c->rgsy = nullptr;
    c->analytic = false;
    return problem_reset(c);
}

// A problem whose right-hand side was written on the device (pgmg_project): the level-0 f grid of
// the fp64, one-GPU context c already holds the new f and phi stays where it lies.  What
// pgmg_set_problem(the current phi, that f) does besides the uploads: phi mirrored into B and S,
// a problem with a caller's f (nothing regenerated, no analytic solution), the statistics and
// the speculation history reset, the carry dropped.  Returns with the device idle.
int pgmg::set_problem_rhs_on_device(pgmg_ctx *c)
{
    if (c->fp32 || c->comm || c->ext_phi)
        return set_err(PGMG_ERR_STATE, "device right-hand side: fp64, one GPU, context-owned only");
    Level &L = c->lv[0];
    const size_t bytes = (size_t)L.P * L.es * (size_t)L.N;
    for (const Grid *g : {&L.B, &c->S})
        if (g->base)
            HIPC(hipMemcpyAsync(row_ptr(*g, 0, L.P, L.es), row_ptr(L.A, 0, L.P, L.es), bytes,
                                hipMemcpyDeviceToDevice, c->s));
    PGMG_TRY(stream_wait(c));
    const double *const old = c->rgfx;
    c->ext_f = nullptr;
    c->gen_rhs = false;
    c->rgfx = c->rgsy = nullptr;
    c->analytic = false;
    PGMG_TRY(drop_graph_of_other_rhs(c, old));
    return problem_reset(c);
}

// The fp32 sibling for pgmg_solve_mixed's child (pgmg_mixed.hip): its level-0 f grid holds the
// scaled defect, written on the parent's stream, which the host has waited for.  The state
// pgmg_set_problem(zeros, that f) leaves -- phi zero, its (zero) frame in B and S, a problem with a
// caller's f, the statistics and the speculation history reset, the carry dropped -- but enqueued
// on c's own stream: the memsets run in stream order before whatever the caller enqueues next,
// and nothing waits.  The interiors of B and S are scratch no pass reads before writing.
int pgmg::set_problem_zero_rhs_on_device_f32(pgmg_ctx *c)
{
    if (!c->fp32 || c->comm)
        return set_err(PGMG_ERR_STATE, "device right-hand side (fp32): fp32, one GPU only");
    Level &L = c->lv[0];
    // (rows 0 .. N of a level-0 grid are one contiguous range: see pgmg_set_problem)
    const size_t bytes = (size_t)L.P * L.es * (size_t)L.N;
    HIPC(hipMemsetAsync(row_ptr(L.A, 0, L.P, L.es), 0, bytes, c->s));
    for (const Grid *g : {&L.B, &c->S})
        if (g->base) launch_zero_frame(G<float>(*g), L.P, L.N, c->s);
    HIPC(hipMemsetAsync(c->stats, 0, 4 * sizeof(unsigned long long), c->s));
    HIPC(hipGetLastError());
    const double *const old = c->rgfx;
    c->ext_phi = nullptr;
    c->ext_f = nullptr;
    c->gen_rhs = false;
    c->rgfx = c->rgsy = nullptr;
    c->analytic = false;
    PGMG_TRY(drop_graph_of_other_rhs(c, old));
    c->have_problem = true;
    c->carry = false;
    c->hist.reset(c->nb);
    return PGMG_OK;
}

// ---------------------------------------------------------------------------
// Device-resident problems (pgmg_set_problem_device): the reference's contract.
// ParallelMultiGridSolver::v_cycle(phi, f, N, h) (Parallel_Mg.cu:21-60) works on arrays the
// caller allocated in device-accessible memory (cudaMallocManaged, ParallelTestRunner.cu:
// 162-163) and updates phi in place; nothing crosses PCIe per call.  Here phi and f are
// device arrays in the reference layout (pitch N, double).
//   * in place (cross-fused fp64 contexts, phi from pgmg_alloc_grid): the call's first
//     finest-level pass (k_pre) reads phi where it lies and its last (k_post) writes the
//     result there (PreArgs::Px, PostArgs::Po = N); the level-0 grids only carry the
//     iterates in between, so a call moves the same bytes as on the context's own grids.
//     The passes read rows and columns past the grid (halos, tile margins): the guard rows
//     of pgmg_alloc_grid keep those reads inside the allocation (span-checked per launch).
//   * staged (any other device pointer, fp32, or contexts without cross-cycle fusion):
//     phi is copied device-to-device into the level-0 grid before the call and back after.
// f = NULL is the analytic RHS of compute_rhs, regenerated in-kernel (never read); a
// caller's f is copied into the level-0 RHS grid at every call (the caller may change it).
// ---------------------------------------------------------------------------
// the boundary of the caller's phi into every level-0 grid the passes pass it through
template <class T>
static void ext_frames(pgmg_ctx *c)
{
    Level &L = c->lv[0];
    const Grid *gs[3] = {&L.A, &L.B, &c->S};
    for (const Grid *g : gs)
        if (g->base) launch_copy_frame<T>(c->ext_phi, L.N, G<T>(*g), L.P, L.N, c->s);
}

// The reference's v_cycle is synchronous on the default stream; the context's stream is
// non-blocking, so a device-bound call first orders it after whatever the caller queued on
// the null stream (an async copy into phi, a kernel writing f).  Work on the caller's own
// non-blocking streams is the caller's to synchronise (include/pgmg.h).  The wait is skipped
// when the null stream is already idle (the usual case: the previous call synchronised).
// The null stream is the CALLING thread's current device's, so the record runs with the
// context's device made current (and the caller's restored): one thread may drive contexts on
// several devices.
int pgmg::order_after_caller(pgmg_ctx *c)
{
    int prev = -1;
    HIPC(hipGetDevice(&prev));
    const bool swap = prev != c->cfg.device;
    if (swap) HIPC(hipSetDevice(c->cfg.device));
    hipError_t e = hipEventRecord(c->ev_caller, nullptr);
    hipError_t q = e == hipSuccess ? hipEventQuery(c->ev_caller) : e;
    if (q == hipErrorNotReady) q = hipStreamWaitEvent(c->s, c->ev_caller, 0);
    if (swap) {
        const hipError_t r = hipSetDevice(prev);
        if (q == hipSuccess) q = r;
    }
    if (q != hipSuccess) return set_err(PGMG_ERR_HIP, hipGetErrorString(q));
    return PGMG_OK;
}

// before a call: the caller's f into the level-0 RHS grid (unless analytic) and phi's frame
// (in place) or all of phi (staged) into the level-0 grids
int pgmg::ext_stage_in(pgmg_ctx *c, bool inplace)
{
    PGMG_TRY(order_after_caller(c));
    Level &L = c->lv[0];
    const int N = L.N;
    if (c->ext_f) {
        if (c->fp32) launch_from_double(c->ext_f, N, G<float>(L.F), L.P, 0, N, c->s);
        else if (is_vmm(L.F.base)) launch_from_double(c->ext_f, N, G<double>(L.F), L.P, 0, N, c->s);
        else HIPC(hipMemcpy2DAsync(L.F.o, L.P * sizeof(double), c->ext_f, N * sizeof(double),
                                   N * sizeof(double), N, hipMemcpyDeviceToDevice, c->s));
    }
    if (!inplace) {
        if (c->fp32) launch_from_double(c->ext_phi, N, G<float>(L.A), L.P, 0, N, c->s);
        else if (is_vmm(L.A.base)) launch_from_double(c->ext_phi, N, G<double>(L.A), L.P, 0, N, c->s);
        else HIPC(hipMemcpy2DAsync(L.A.o, L.P * sizeof(double), c->ext_phi, N * sizeof(double),
                                   N * sizeof(double), N, hipMemcpyDeviceToDevice, c->s));
    }
    if (c->fp32) ext_frames<float>(c);
    else ext_frames<double>(c);
    HIPC(hipGetLastError());
    return PGMG_OK;
}

int pgmg::ext_stage_out(pgmg_ctx *c)
{
    Level &L = c->lv[0];
    const int N = L.N;
    if (c->fp32) launch_to_double(G<float>(L.A), L.P, c->ext_phi, N, 0, N, c->s);
    else if (is_vmm(L.A.base)) launch_to_double(G<double>(L.A), L.P, c->ext_phi, N, 0, N, c->s);
    else HIPC(hipMemcpy2DAsync(c->ext_phi, N * sizeof(double), L.A.o, L.P * sizeof(double),
                               N * sizeof(double), N, hipMemcpyDeviceToDevice, c->s));
    HIPC(hipGetLastError());
    return PGMG_OK;
}

static int run_cycles_core(pgmg_ctx *c, int ncycles, int gamma)
{
    // W-cycles revisit the coarse levels until their checks fire (the reference's W-cycle at
    // 129 exits 147 times in its first cycle): their speculative calls decide those checks
    // in-stream (chk_mode) and only predict converged levels to fire (one GPU, any N: a W-cycle
    // is never a captured graph, so the smaller grids gain as much)
    const bool w_spec = gamma > 1 && c->fused && c->comm == nullptr &&
                        !(c->cfg.flags & (PGMG_FLAG_NO_SPEC_FIRE | PGMG_FLAG_EXACT_DIST));
    // pgmg_spec_visit_modes: the counts are this call's (zeros after a V call, also one that
    // runs in-stream and never reaches run_cycles_spec)
    c->wcount[0] = c->wcount[1] = c->wcount[2] = 0;
    if (!c->hist.spec_off && (gamma == 1 ? c->spec : w_spec)) return run_cycles_spec(c, ncycles, gamma);
    return run_cycles_plain(c, ncycles, gamma);
}

// a call on a device-bound problem (pgmg_set_problem_device): synchronous, as the reference's
// v_cycle is (the caller reads phi when it returns)
static int run_cycles_ext(pgmg_ctx *c, int ncycles, int gamma)
{
    const bool inplace = c->ext_inplace;
    PGMG_TRY(ext_stage_in(c, inplace));
    if (inplace) {
        c->call.x_in = c->ext_phi;
        c->call.x_out = c->ext_phi;
        c->call.ext_P = c->lv[0].N;
    }
    PGMG_TRY(run_cycles_core(c, ncycles, gamma));
    if (!inplace) PGMG_TRY(ext_stage_out(c));
    PGMG_TRY(stream_wait(c));
    return PGMG_OK;
}

static int run_cycles(pgmg_ctx *c, int ncycles, int gamma)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (ncycles <= 0) return PGMG_OK;
    const CallScope scope{c};   // c->call is this call's: clear again on every way out
    // the carry is this call's to take (a V call on the context's own problem: the first
    // speculative segment starts from it) or gone; a call that runs in-stream drops it
    c->call.carry_use = c->carry && gamma == 1 && c->ext_phi == nullptr &&
                        tuning_int("PGMG_CARRY_TAKE", 1) != 0;   // (measurement build: 0 never takes)
    c->carry = false;
    return c->ext_phi ? run_cycles_ext(c, ncycles, gamma) : run_cycles_core(c, ncycles, gamma);
}

extern "C" {

int pgmg_comm_stats(pgmg_ctx *c, long long *groups, double *ms)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (!c->comm) {
        PGMG_TRY(stream_wait(c));
        if (groups) *groups = 0;
        if (ms) *ms = 0.0;
        return PGMG_OK;
    }
    return c->comm->comm_stats(c->s, groups, ms);
}

int pgmg_comm_ranks(pgmg_ctx *c, int *ranks)
{
    if (!c || !ranks) return set_err(PGMG_ERR_ARG, "null argument");
    if (!c->comm) return *ranks = 1, PGMG_OK;
    return c->comm->comm_ranks(ranks);
}

// JacobiSmoother(eps) (Smoother.hpp:38): a new threshold for the following calls.  The carried
// pre-smooth was checked against the old one, and the speculation history's predictions are
// relative to eps: both go (the statistics continue)
int pgmg_set_eps(pgmg_ctx *c, double eps)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return set_err(PGMG_ERR_ARG, "eps must be finite and >= 0");
    PGMG_TRY(stream_wait(c));
    c->cfg.eps = eps;
    c->carry = false;
    if (c->gexec) {   // a captured cycle holds the old eps in its kernel arguments
        HIPC(hipGraphExecDestroy(c->gexec));
        c->gexec = nullptr;
    }
    c->hist.reset(c->nb);
    return PGMG_OK;
}

int pgmg_vcycle(pgmg_ctx *c, int ncycles) { return run_cycles(c, ncycles, 1); }
int pgmg_wcycle(pgmg_ctx *c, int ncycles) { return run_cycles(c, ncycles, c ? c->cfg.alpha : 1); }

int pgmg_sync(pgmg_ctx *c)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    PGMG_TRY(stream_wait(c));
    return PGMG_OK;
}

int pgmg_last_elapsed_ms(pgmg_ctx *c, double *ms)
{
    if (!c || !ms) return set_err(PGMG_ERR_ARG, "null argument");
    HIPC(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = f;
    return PGMG_OK;
}

int pgmg_get_solution(pgmg_ctx *c, double *phi)
{
    return pgmg_gather_solution(c, -1, phi);
}

int pgmg_get_rhs(pgmg_ctx *c, double *f)
{
    if (!c || !f) return set_err(PGMG_ERR_ARG, "null argument");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1) return set_err(PGMG_ERR_STATE, "pgmg_get_rhs: one GPU only (world 1)");
    PGMG_TRY(stream_wait(c));
    const Level &L = c->lv[0];
    return download_grid(c, L.F.o, L.P, L.N, f);
}

int pgmg_gather_solution(pgmg_ctx *c, int root, double *phi)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    const int me = c->comm ? c->comm->rank() : 0;
    if (root >= c->cfg.world) return set_err(PGMG_ERR_ARG, "root >= world");
    // without strips every rank holds the whole solution: every root means this rank
    if (!phi && (root < 0 || root == me || !c->comm))
        return set_err(PGMG_ERR_ARG, "null phi on a receiving rank");
    if (c->comm) {
        int e = c->comm->wait(c->s);
        if (e) return e;
        return c->comm->gather_solution(c, phi, root);
    }
    PGMG_TRY(stream_wait(c));
    Level &L = c->lv[0];
    if (c->ext_phi) {   // a device-bound problem: the solution is the caller's array
        HIPC(hipMemcpy(phi, c->ext_phi, (size_t)L.N * L.N * sizeof(double), hipMemcpyDeviceToHost));
        return PGMG_OK;
    }
    return download_grid(c, L.A.o, L.P, L.N, phi);
}

// FNV-64 over the IEEE words of phi in the reference layout: the checksum the golden
// fixtures of the reference's runs carry (bench.py verifies the run it timed with it)
int pgmg_solution_hash(pgmg_ctx *c, int root, unsigned long long *out)
{
    if (!c || !out) return set_err(PGMG_ERR_ARG, "null argument");
    const int me = c->comm ? c->comm->rank() : 0;
    if (root >= c->cfg.world) return set_err(PGMG_ERR_ARG, "root >= world");
    const bool want = root < 0 || root == me || !c->comm;
    const long long n = (long long)c->lv[0].N * c->lv[0].N;
    std::vector<double> phi(want ? (size_t)n : 0);
    int e = pgmg_gather_solution(c, root, want ? phi.data() : nullptr);
    if (e) return e;
    unsigned long long h = 1469598103934665603ULL;
    if (want) {
        for (long long i = 0; i < n; ++i) {
            unsigned long long w;
            std::memcpy(&w, &phi[(size_t)i], 8);
            h = (h ^ w) * 1099511628211ULL;
        }
    }
    *out = want ? h : 0ULL;
    return PGMG_OK;
}

int pgmg_residual_norm(pgmg_ctx *c, double *out)
{
    if (!c || !out) return set_err(PGMG_ERR_ARG, "null argument");
    Level &L = c->lv[0];
    int nbk = c->partials_cap < 1024 ? c->partials_cap : 1024;
    // a device-bound problem: its phi (and a caller's f) into the level-0 grids first (the
    // analytic f is in L.F since pgmg_set_problem_device)
    if (c->ext_phi) PGMG_TRY(ext_stage_in(c, false));
    if (c->comm) {
        int e = c->comm->halo(L.A, L, 1, c->s);
        if (e) return e;
    }
    if (c->fp32)
        launch_resnorm_partials(G<float>(L.A), G<float>(L.F), c->partials, (float)L.ih, L.N, L.P,
                                L.u0, L.u1, nbk, c->s);
    else
        launch_resnorm_partials(G<double>(L.A), G<double>(L.F), c->partials, L.ih, L.N, L.P, L.u0,
                                L.u1, nbk, c->s);
    launch_sum_partials(c->partials, nbk, c->scalar, c->s);
    if (c->comm) {
        int e = c->comm->allreduce_sum(c->scalar, 1, c->s);
        if (e) return e;
    }
    double s = 0.0;
    HIPC(hipMemcpyAsync(&s, c->scalar, sizeof(double), hipMemcpyDeviceToHost, c->s));
    PGMG_TRY(stream_wait(c));
    *out = std::sqrt(s);
    return PGMG_OK;
}

int pgmg_stats(pgmg_ctx *c, long long *sweeps, long long *exits)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    unsigned long long h[4];
    PGMG_TRY(stream_wait(c));
    HIPC(hipMemcpy(h, c->stats, sizeof(h), hipMemcpyDeviceToHost));
    if (sweeps) *sweeps = (long long)h[0];
    if (exits) *exits = (long long)h[1];
    return PGMG_OK;
}

int pgmg_stats_detail(pgmg_ctx *c, long long *out4)
{
    if (!c || !out4) return set_err(PGMG_ERR_ARG, "null argument");
    unsigned long long h[4];
    PGMG_TRY(stream_wait(c));
    HIPC(hipMemcpy(h, c->stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out4[i] = (long long)h[i];
    out4[2] = c->cross ? out4[2] : -1;
    return PGMG_OK;
}

int pgmg_levels(pgmg_ctx *c, int *bulk, int *tail_top)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (bulk) *bulk = c->nb;
    if (tail_top) *tail_top = c->lv[c->nb].N;
    return PGMG_OK;
}

// algorithmic bytes of one V-cycle on this rank (DESIGN.md "Roofline accounting")
int pgmg_vcycle_bytes(pgmg_ctx *c, double *bytes)
{
    if (!c || !bytes) return set_err(PGMG_ERR_ARG, "null argument");
    double b = 0.0;
    for (int l = 0; l < c->nb; ++l) {
        const Level &L = c->lv[l];
        const Level &C = c->lv[l + 1];
        const double n = (double)(L.u1 - L.u0) * (L.N - 2);
        const double nc = (double)(C.u1 - C.u0) * (C.N - 2);
        if (c->fused) {
            if (l == 0 && c->cross) {                     // steady state: one k_postpre
                b += (c->rgfx ? 16.0 : 24.0) * n + 16.0 * nc;     // phi, (f,) ec in; x4, rc out
                continue;
            }
            if (l > 0 && c->recompute) {                  // x0 = 0, x2 recomputed
                b += 8.0 * n + 8.0 * nc;                  // k_pre: f in; rc out
                b += 16.0 * n + 8.0 * nc;                 // k_post: f, ec in; x2 out
                continue;
            }
            const double fb = (l == 0 && c->rgfx) ? 0.0 : 8.0;  // level 0: f regenerated
            b += (l == 0 ? 16.0 + fb : 16.0) * n + 8.0 * nc;   // k_pre: x0, f in; x2, rc out
            b += (16.0 + fb) * n + 8.0 * nc;                    // k_post: phi, f, ec in; x2 out
            continue;
        }
        const int S1 = c->cfg.v1 + 1, S2 = c->cfg.v2 + 1;
        b += (l == 0 ? 24.0 : 16.0) * n + 24.0 * n * (S1 - 1);  // pre-smooth
        b += 16.0 * n + 8.0 * nc;                                // residual + restriction
        b += 16.0 * n + 8.0 * nc;                                // prolongation (RMW fine)
        b += 24.0 * n * S2;                                      // post-smooth
        if (S1 & 1) b += 16.0 * n;
        if (S2 & 1) b += 16.0 * n;
    }
    const Level &Lt = c->lv[c->nb];
    b += 16.0 * (double)Lt.N * Lt.N;                             // tail: f in, e out
    *bytes = b * (c->lv[0].es / 8.0);                            // per-point figures are fp64
    return PGMG_OK;
}

int pgmg_fine_pass_bytes(pgmg_ctx *c, int pass, double *bytes)
{
    if (!c || !bytes || pass < 0 || pass > 5) return set_err(PGMG_ERR_ARG, "bad argument");
    if (c->nb == 0) return set_err(PGMG_ERR_STATE, "no bulk level");
    const Level &L = c->lv[0], &C = c->lv[1];
    const double n = (double)(L.u1 - L.u0) * (L.N - 2);
    const StripRows sr = strip_rows(L, C);
    const double nc = (double)(sr.rc_hi > sr.rc_lo ? sr.rc_hi - sr.rc_lo : 0) * (C.N - 2);
    double b = 0.0;
    // f is regenerated in-kernel (not read) by the level-0 passes
    const double fb = c->rgfx != nullptr ? 0.0 : 8.0;
    switch (pass) {
    case 0: b = 24.0 * n; break;                               // x, f in; x out
    case 1: b = (16.0 + fb) * n + 8.0 * nc; break;             // x0, (f) in; x2, rc out
    case 2: b = (16.0 + fb) * n + 8.0 * nc; break;             // phi, (f,) ec in; x2 out
    case 3: b = (16.0 + fb) * n + 16.0 * nc; break;            // phi, (f,) ec; x4, rc
    case 4: b = (16.0 + fb) * n + 16.0 * nc; break;            // carry pass: x2 for x4
    case 5: b = (16.0 + fb) * n + 16.0 * nc; break;            // recompute form: phi = x2
    }
    *bytes = b * (L.es / 8.0);
    return PGMG_OK;
}

int pgmg_precision(pgmg_ctx *c, int *precision, int *elem_bytes)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (precision) *precision = c->fp32 ? PGMG_PRECISION_FP32 : PGMG_PRECISION_FP64;
    if (elem_bytes) *elem_bytes = c->lv[0].es;
    return PGMG_OK;
}
int pgmg_phi_device(pgmg_ctx *c, double **ptr, int *pitch, int *row0, int *rows)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    Level &L = c->lv[0];
    c->carry = false;   // the pointer allows writes to phi
    if (ptr) *ptr = static_cast<double *>(L.A.o);
    if (pitch) *pitch = L.P;
    if (row0) *row0 = L.lo;
    if (rows) *rows = L.hi - L.lo;
    return PGMG_OK;
}

}  // extern "C"

template <class T>
static void bench_sweeps(pgmg_ctx *c, int reps)
{
    Level &L = c->lv[0];
    SweepArgsT<T> a{};
    a.f = G<T>(L.F);
    a.hh = (T)L.hh;
    a.inv_hh = (T)L.ih;
    a.W = L.N;
    a.P = L.P;
    a.row0 = L.u0;
    a.row1 = L.u1;
    for (int k = 0; k < reps; ++k) {
        a.xin = G<T>((k & 1) ? L.B : L.A);
        a.xout = G<T>((k & 1) ? L.A : L.B);
        launch_sweep(a, false, true, c->s);
    }
}

extern "C" {

int pgmg_bench_sweep(pgmg_ctx *c, int reps, double *ms)
{
    if (!c || !ms || reps <= 0) return set_err(PGMG_ERR_ARG, "bad argument");
    if (c->nb == 0) return set_err(PGMG_ERR_STATE, "no bulk level");
    c->carry = false;   // the sweeps overwrite phi
    auto run = [&](int n) { c->fp32 ? bench_sweeps<float>(c, n) : bench_sweeps<double>(c, n); };
    run(2);  // warm
    HIPC(hipEventRecord(c->ev0, c->s));
    run(reps);
    HIPC(hipEventRecord(c->ev1, c->s));
    HIPC(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = f / reps;
    return PGMG_OK;
}

int pgmg_fine_pass_time(pgmg_ctx *c, int pass, int *count, double *mean_ms)
{
    if (!c || pass < 0 || pass > 5) return set_err(PGMG_ERR_ARG, "bad argument");
    PGMG_TRY(stream_wait(c));
    auto &pool = c->tpool[pass];
    double tot = 0.0;
    const int n = pool.used / 2;
    for (int i = 0; i < n; ++i) {
        float f = 0.f;
        HIPC(hipEventElapsedTime(&f, pool.ev[2 * i], pool.ev[2 * i + 1]));
        tot += f;
    }
    if (count) *count = n;
    if (mean_ms) *mean_ms = n ? tot / n : 0.0;
    pool.used = 0;
    c->info_bytes[pass] = n ? c->tbytes[pass] / n : 0.0;
    c->info_kern[pass] = n ? c->tkern[pass] : nullptr;
    c->tbytes[pass] = 0.0;
    c->tkern[pass] = nullptr;
    return PGMG_OK;
}

int pgmg_fine_pass_info(pgmg_ctx *c, int pass, char *symbol, int len, double *bytes)
{
    if (!c || pass < 0 || pass > 5 || (symbol && len < 1)) return set_err(PGMG_ERR_ARG, "bad argument");
    if (bytes) *bytes = c->info_bytes[pass];
    if (symbol) {
        std::string name;
        if (c->info_kern[pass]) {
            const char *m = hipKernelNameRefByPtr(c->info_kern[pass], c->s);
            if (m) {
                int st = 0;
                char *d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
                name = (st == 0 && d) ? d : m;
                std::free(d);
            }
        }
        std::snprintf(symbol, (size_t)len, "%s", name.c_str());
    }
    return PGMG_OK;
}

int pgmg_fine_sweep_time(pgmg_ctx *c, int *count, double *mean_ms)
{
    return pgmg_fine_pass_time(c, 0, count, mean_ms);
}

int pgmg_fused(pgmg_ctx *c, int *fused)
{
    if (!c || !fused) return set_err(PGMG_ERR_ARG, "bad argument");
    *fused = c->fused ? 1 : 0;
    return PGMG_OK;
}

}  // extern "C"
