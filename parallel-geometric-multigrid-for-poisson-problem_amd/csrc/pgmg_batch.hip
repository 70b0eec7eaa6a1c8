// pgmg_batch.hip — many small Poisson problems in one launch, one workgroup each
// (include/pgmg.h "Batched small problems").
//
// At N <= 65 a whole V- or W-cycle is one workgroup's work in LDS (pgmg_tail_dev.h), and a solve
// through a context is bound by its launches and by the host waiting for a residual norm before
// every chunk of cycles.  k_tail_batch gives workgroup b problem b (phi + b N^2, f + b N^2, pitch
// N): it loads the problem into its own LDS pyramid, runs the tail's gamma-cycle on it, and in
// solve mode restates pgmg_solve_damped's loop and stop rule (pgmg_stop.h) on the device, every
// decision taken uniformly by the workgroup from a norm that all its threads hold bit for bit.
// Nothing is shared between workgroups: no atomics, no scratch in global memory, per-problem
// result words written with plain stores.  The host is not involved until the launch is over.
#include <climits>
#include <cmath>
#include <string>

#include "pgmg_ctx.h"
#include "pgmg_stop.h"
#include "pgmg_tail_dev.h"

namespace pgmg {

template <class Real>
struct BatchArgs {
    Real *phi;             // B problems, N * N elements each, updated in place
    const Real *f;
    int T_elems;           // elements of the scratch grid T behind the two pyramids
    int solve;             // 0: `ncycles` cycles; 1: the damped solve
    int ncycles;
    // solve mode: pgmg_solve_opts' fields and the damping weight (Real)(omega * 0.25 * (h * h))
    int max_cycles, check_every, stall_checks;
    double rtol, atol, stall_ratio;
    int damp;              // omega > 0
    Real w;
    // per-problem results, B entries each; any may be null
    int *cycles, *checks, *reason;
    double *res0, *res;
    long long *sweeps, *exits;
    double *history;       // B x history_cap
    int history_cap;
};

template <class Real>
__global__ __launch_bounds__(kTailThreads) void k_tail_batch(TailArgsDev<Real> d, BatchArgs<Real> b)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int S = d.S;
    double *red = lds;
    Real *E = reinterpret_cast<Real *>(lds + kTailRed);
    Real *F = E + S;
    Real *T = E + 2 * S;
    const TailLevel<Real> L0 = d.lv[0];
    const int N = L0.N, n = N * N;
    const long long pb = blockIdx.x;
    Real *phi = b.phi + pb * n;
    const Real *f = b.f + pb * n;

    // the whole LDS image is this workgroup's own: both pyramids and the scratch grid start at
    // +0, whatever an earlier workgroup left on this CU
    for (int k = threadIdx.x; k < 2 * S + b.T_elems; k += kTailThreads) E[k] = Real(0);
    __syncthreads();
    {
        // phi and f, frame included; every load of a thread issued before its first LDS store
        // (k_tail's load)
        constexpr int KU = (65 * 65 + kTailThreads - 1) / kTailThreads;   // N <= 65
        Real fv[KU], ev[KU];
        #pragma unroll
        for (int q = 0; q < KU; ++q) {
            // (clamped: a point past the grid re-reads the last one, never past the problem)
            const int k = min((int)threadIdx.x + q * kTailThreads, n - 1);
            fv[q] = f[k];
            ev[q] = phi[k];
        }
        #pragma unroll
        for (int q = 0; q < KU; ++q) {
            const int k = threadIdx.x + q * kTailThreads;
            if (k < n) {
                F[k] = fv[q];
                E[k] = ev[q];
            }
        }
    }
    __syncthreads();

    Cnt cnt;
    int par = 0;
    // pgmg_stop.h's StopState and the solve's results; every thread holds the same values
    int k_run = 0, checks = 0, streak = 0, reason = 0;
    double r0 = 0.0, prev = 0.0, rlast = 0.0;
    int run = b.solve ? 0 : b.ncycles;
    const int m = N - 2, mm = m * m;
    const float rm = 1.0f / (float)m;
    for (;;) {
        if (b.solve) {
            // check `checks`, after k_run cycles: r = f - ih (4x - x_l - x_r - x_u - x_d) on the
            // interior (pgmg_monitor's expression in Real), squared and summed in double -- a
            // thread's points in index order, then BlockTeam::sum's lane and wave order: the
            // bits depend on (phi, f, N, h) alone
            double acc = 0.0;
            for (int p = threadIdx.x; p < mm; p += kTailThreads) {
                const int jj = tail_row(p, rm);
                const int k = (1 + jj) * N + 1 + (p - jj * m);
                const Real r =
                    F[k] - L0.ih * (Real(4) * E[k] - E[k - 1] - E[k + 1] - E[k - N] - E[k + N]);
                acc += sq(r);
                T[k] = r;
            }
            // (its barrier: every r is in T; every thread holds the same bits, read out of lane 0
            // so that the rule's state below lives in scalar registers)
            const double s = readlane64(BlockTeam::sum(acc, red, par), 0);
            if (b.damp) {
                // x <- x + w r on the interior, every r from the x of before the update (T);
                // two roundings (-ffp-contract=off); the frame is never written
                for (int p = threadIdx.x; p < mm; p += kTailThreads) {
                    const int jj = tail_row(p, rm);
                    const int k = (1 + jj) * N + 1 + (p - jj * m);
                    const Real wr = b.w * T[k];
                    E[k] = E[k] + wr;
                }
            }
            __syncthreads();
            const double r = readlane64(__builtin_sqrt(s), 0);
            // stop_check (pgmg_stop.h), in its order
            const int i = checks++;
            const double pv = prev;
            if (i == 0) r0 = r;
            prev = r;
            rlast = r;
            if (threadIdx.x == 0 && b.history != nullptr && i < b.history_cap)
                b.history[pb * b.history_cap + i] = r;
            const double rel = b.rtol * r0;
            if (!__builtin_isfinite(r)) {
                reason = PGMG_STOP_NONFINITE;
            } else if (r <= (b.atol > rel ? b.atol : rel)) {
                reason = PGMG_STOP_CONVERGED;
            } else {
                if (i >= 1 && b.stall_ratio > 0.0) {
                    streak = r > b.stall_ratio * pv ? streak + 1 : 0;
                    if (streak >= b.stall_checks) reason = PGMG_STOP_STALLED;
                }
                if (reason == 0 && k_run >= b.max_cycles) reason = PGMG_STOP_MAX_CYCLES;
            }
            if (reason != 0) break;
            const int left = b.max_cycles - k_run;
            run = b.check_every < left ? b.check_every : left;
        }
        for (int v = 0; v < run; ++v) cnt += tail_gcycle<BlockTeam>(d, 0, 1, E, F, T, red, par);
        k_run += run;
        if (!b.solve) break;
    }

    for (int k = threadIdx.x; k < n; k += kTailThreads) phi[k] = E[k];
    // the slots of the history no check wrote (other slots than thread 0's stores above)
    if (b.solve && b.history != nullptr)
        for (int i = checks + threadIdx.x; i < b.history_cap; i += kTailThreads)
            b.history[pb * b.history_cap + i] = __builtin_nan("");
    if (threadIdx.x == 0) {
        if (b.sweeps != nullptr) b.sweeps[pb] = cnt.sweeps;
        if (b.exits != nullptr) b.exits[pb] = cnt.exits;
        if (b.solve) {
            if (b.cycles != nullptr) b.cycles[pb] = k_run;
            if (b.checks != nullptr) b.checks[pb] = checks;
            if (b.reason != nullptr) b.reason[pb] = reason;
            if (b.res0 != nullptr) b.res0[pb] = r0;
            if (b.res != nullptr) b.res[pb] = rlast;
        }
    }
}

// pseudo-random right-hand sides for pgmg_batch_time: interior values in [-1, 1), frame +0
template <class Real>
__global__ void k_batch_fill(Real *f, int N, long long total)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const int q = (int)(k % ((long long)N * N)), j = q / N, i = q - j * N;
    const unsigned hsh = (unsigned)k * 2654435761u;
    const bool in = i > 0 && j > 0 && i < N - 1 && j < N - 1;
    f[k] = in ? (Real)((double)(hsh >> 8) * (1.0 / 8388608.0) - 1.0) : Real(0);
}

namespace {

const char *batch_config_error(const pgmg_batch_config *cfg)
{
    if (!cfg) return "null cfg";
    const int N = cfg->N;
    if (N != 5 && N != 9 && N != 17 && N != 33 && N != 65) return "N must be 5, 9, 17, 33 or 65";
    if (cfg->v1 < 0 || cfg->v2 < 0 || cfg->v1 + 1 >= kMaxSweeps || cfg->v2 + 1 >= kMaxSweeps ||
        cfg->coarse_iter < 0 || cfg->n_coarse < 3 || cfg->alpha < 1)
        return "bad smoother/cycle parameters";
    if (cfg->alpha > 15) return "alpha must be at most 15";
    if (!std::isfinite(cfg->h) || cfg->h == 0.0) return "h must be finite and not 0";
    if (cfg->precision != PGMG_PRECISION_FP64 && cfg->precision != PGMG_PRECISION_FP32)
        return "precision must be PGMG_PRECISION_FP64 or _FP32";
    return nullptr;
}

// one launch of B workgroups; the level table as launch_tail_gamma builds it
template <class Real>
hipError_t launch_tail_batch(const pgmg_batch_config &cfg, int gamma, BatchArgs<Real> b, long long B,
                             hipStream_t s)
{
    static bool attr_set = false;
    TailArgsDev<Real> d{};
    d.a.P_top = cfg.N;
    d.a.N_top = cfg.N;
    d.a.h_top = cfg.h;
    d.a.x0_from_global = 1;
    d.a.v1 = cfg.v1;
    d.a.v2 = cfg.v2;
    d.a.coarse_iter = cfg.coarse_iter;
    d.a.n_coarse = cfg.n_coarse;
    d.a.eps = cfg.eps;
    d.gamma = gamma;
    d.eps2 = norm2_threshold(cfg.eps);
    int N = cfg.N;
    double h = cfg.h;
    int off = 0, nl = 0;
    for (; nl < kTailMaxLevels; ++nl) {
        d.lv[nl].N = N;
        d.lv[nl].off = off;
        d.lv[nl].hh = (Real)(h * h);
        d.lv[nl].ih = (Real)(1.0 / (h * h));
        d.lv[nl].rN = 1.0f / (float)N;
        off += N * N;
        if (N <= cfg.n_coarse) {
            ++nl;
            break;
        }
        N = (N - 1) / 2 + 1;
        h = 2 * h;
    }
    d.nl = nl;
    d.S = off;
    {
        static const int wave_n = tuning_int("PGMG_TAIL_WAVE_N", 9);
        d.wave_n = wave_n;
    }
    d.prof = nullptr;
    const size_t bytes = tail_lds_bytes<Real>(cfg.N, cfg.n_coarse);
    b.T_elems = (int)((bytes - kTailRed * sizeof(double)) / sizeof(Real)) - 2 * off;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void *)k_tail_batch<Real>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    k_tail_batch<Real><<<dim3((unsigned)B), dim3(kTailThreads), bytes, s>>>(d, b);
    return hipGetLastError();
}

int batch_common_check(const char *who, const pgmg_batch_config *cfg, const void *phi, const void *f,
                       long long B)
{
    if (const char *e = batch_config_error(cfg)) return set_err(PGMG_ERR_ARG, std::string(who) + ": " + e);
    if (!phi || !f) return set_err(PGMG_ERR_ARG, std::string(who) + ": null phi or f");
    if (B < 1 || B > INT_MAX)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": B must be in 1 .. 2^31 - 1");
    return PGMG_OK;
}

template <class Real>
int batch_cycle_t(const pgmg_batch_config &cfg, int gamma, int ncycles, void *phi, const void *f,
                  long long B, long long *sweeps, long long *exits, hipStream_t s)
{
    BatchArgs<Real> b{};
    b.phi = static_cast<Real *>(phi);
    b.f = static_cast<const Real *>(f);
    b.ncycles = ncycles;
    b.sweeps = sweeps;
    b.exits = exits;
    PGMG_HIPC(launch_tail_batch<Real>(cfg, gamma, b, B, s));
    return PGMG_OK;
}

template <class Real>
int batch_solve_t(const pgmg_batch_config &cfg, const pgmg_solve_opts &o, double omega, void *phi,
                  const void *f, long long B, const pgmg_batch_out *out, hipStream_t s)
{
    BatchArgs<Real> b{};
    b.phi = static_cast<Real *>(phi);
    b.f = static_cast<const Real *>(f);
    b.solve = 1;
    b.max_cycles = o.max_cycles;
    b.check_every = o.check_every;
    b.stall_checks = o.stall_checks;
    b.rtol = o.rtol;
    b.atol = o.atol;
    b.stall_ratio = o.stall_ratio;
    b.damp = omega > 0.0 ? 1 : 0;
    // omega * 0.25 * (h * h) in double, left to right, then the element type (pgmg_damp's w)
    b.w = (Real)(omega * 0.25 * (cfg.h * cfg.h));
    if (out) {
        b.cycles = out->cycles;
        b.checks = out->checks;
        b.reason = out->reason;
        b.res0 = out->res0;
        b.res = out->res;
        b.sweeps = out->sweeps;
        b.exits = out->exits;
        b.history = out->history;
        b.history_cap = out->history ? out->history_cap : 0;
    }
    PGMG_HIPC(launch_tail_batch<Real>(cfg, o.cycle == PGMG_CYCLE_W ? cfg.alpha : 1, b, B, s));
    return PGMG_OK;
}

template <class Real>
int batch_time_t(const pgmg_batch_config &cfg, int gamma, int ncycles, long long B, int reps,
                 double *ms_per_launch)
{
    const long long total = B * cfg.N * cfg.N;
    Real *phi = nullptr, *f = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&] {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (phi) (void)hipFree(phi);
        if (f) (void)hipFree(f);
    };
    auto run = [&]() -> int {
        if (hipMalloc((void **)&phi, total * sizeof(Real)) != hipSuccess ||
            hipMalloc((void **)&f, total * sizeof(Real)) != hipSuccess)
            return set_err(PGMG_ERR_NOMEM, "pgmg_batch_time: device allocation failed");
        PGMG_HIPC(hipEventCreate(&e0));
        PGMG_HIPC(hipEventCreate(&e1));
        PGMG_HIPC(hipMemsetAsync(phi, 0, total * sizeof(Real), nullptr));
        k_batch_fill<Real><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr>>>(f, cfg.N, total);
        PGMG_HIPC(hipGetLastError());
        BatchArgs<Real> b{};
        b.phi = phi;
        b.f = f;
        b.ncycles = ncycles;
        for (int i = 0; i < 2; ++i) PGMG_HIPC(launch_tail_batch<Real>(cfg, gamma, b, B, nullptr));
        PGMG_HIPC(hipEventRecord(e0, nullptr));
        for (int i = 0; i < reps; ++i) PGMG_HIPC(launch_tail_batch<Real>(cfg, gamma, b, B, nullptr));
        PGMG_HIPC(hipEventRecord(e1, nullptr));
        PGMG_HIPC(hipEventSynchronize(e1));
        float ms = 0.f;
        PGMG_HIPC(hipEventElapsedTime(&ms, e0, e1));
        *ms_per_launch = (double)ms / reps;
        return PGMG_OK;
    };
    const int rc = run();
    cleanup();
    return rc;
}

}  // namespace
}  // namespace pgmg

using namespace pgmg;

extern "C" {

int pgmg_batch_config_default(pgmg_batch_config *cfg, int N)
{
    if (!cfg) return set_err(PGMG_ERR_ARG, "pgmg_batch_config_default: null cfg");
    *cfg = pgmg_batch_config{};
    cfg->N = N;
    cfg->v1 = 1;
    cfg->v2 = 1;
    cfg->coarse_iter = 10;
    cfg->n_coarse = 5;
    cfg->alpha = 3;
    cfg->eps = 1e-7;
    cfg->h = N > 1 ? 1.0 / (N - 1) : 1.0;
    cfg->precision = PGMG_PRECISION_FP64;
    return PGMG_OK;
}

int pgmg_batch_cycle(const pgmg_batch_config *cfg, int cycle, int ncycles, void *d_phi, const void *d_f,
                     long long B, long long *d_sweeps, long long *d_exits, void *stream)
{
    const char *const who = "pgmg_batch_cycle";
    if (int e = batch_common_check(who, cfg, d_phi, d_f, B)) return e;
    if (cycle != PGMG_CYCLE_V && cycle != PGMG_CYCLE_W)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": cycle must be PGMG_CYCLE_V or PGMG_CYCLE_W "
                                                        "(an F-cycle rebuilds the analytic f)");
    if (ncycles < 0) return set_err(PGMG_ERR_ARG, std::string(who) + ": ncycles < 0");
    const int gamma = cycle == PGMG_CYCLE_W ? cfg->alpha : 1;
    hipStream_t s = (hipStream_t)stream;
    return cfg->precision == PGMG_PRECISION_FP32
               ? batch_cycle_t<float>(*cfg, gamma, ncycles, d_phi, d_f, B, d_sweeps, d_exits, s)
               : batch_cycle_t<double>(*cfg, gamma, ncycles, d_phi, d_f, B, d_sweeps, d_exits, s);
}

int pgmg_batch_solve(const pgmg_batch_config *cfg, const pgmg_solve_opts *o, double omega, void *d_phi,
                     const void *d_f, long long B, const pgmg_batch_out *out, void *stream)
{
    const char *const who = "pgmg_batch_solve";
    if (!o) return set_err(PGMG_ERR_ARG, std::string(who) + ": null opts");
    if (int e = batch_common_check(who, cfg, d_phi, d_f, B)) return e;
    if (!std::isfinite(omega) || omega < 0.0 || omega > 1.0)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": omega must be finite and in [0, 1]");
    if (const char *e = solve_opts_error(*o)) return set_err(PGMG_ERR_ARG, std::string(who) + ": " + e);
    if (o->cycle == PGMG_CYCLE_F)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": PGMG_CYCLE_F rebuilds the analytic f");
    if (o->monitor & PGMG_MON_ERROR)
        return set_err(PGMG_ERR_ARG, std::string(who) + ": PGMG_MON_ERROR needs an analytic problem");
    if (out && out->history_cap < 0) return set_err(PGMG_ERR_ARG, std::string(who) + ": history_cap < 0");
    hipStream_t s = (hipStream_t)stream;
    return cfg->precision == PGMG_PRECISION_FP32
               ? batch_solve_t<float>(*cfg, *o, omega, d_phi, d_f, B, out, s)
               : batch_solve_t<double>(*cfg, *o, omega, d_phi, d_f, B, out, s);
}

int pgmg_batch_time(const pgmg_batch_config *cfg, int cycle, int ncycles, long long B, int reps,
                    double *ms_per_launch)
{
    const char *const who = "pgmg_batch_time";
    if (const char *e = batch_config_error(cfg)) return set_err(PGMG_ERR_ARG, std::string(who) + ": " + e);
    if (!ms_per_launch || reps < 1 || ncycles < 0 || B < 1 || B > INT_MAX ||
        (cycle != PGMG_CYCLE_V && cycle != PGMG_CYCLE_W))
        return set_err(PGMG_ERR_ARG, std::string(who) + ": need ms_per_launch, reps >= 1, ncycles >= 0, "
                                                        "B in 1 .. 2^31 - 1 and a V or W cycle");
    const int gamma = cycle == PGMG_CYCLE_W ? cfg->alpha : 1;
    return cfg->precision == PGMG_PRECISION_FP32
               ? batch_time_t<float>(*cfg, gamma, ncycles, B, reps, ms_per_launch)
               : batch_time_t<double>(*cfg, gamma, ncycles, B, reps, ms_per_launch);
}

}  // extern "C"
