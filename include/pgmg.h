/*
 * pgmg.h — C ABI of the MI355X geometric-multigrid library (libpgmg.so).
 *
 * The drop-in boundary for the reference's GPU path.  Every entry point is
 * extern "C" with plain pointers, sizes and int return codes (0 = success,
 * negative = error; pgmg_last_error() gives the message).  No C++ exceptions
 * and no HIP/torch types cross it.  Host code that binds it: the C++ mirror of
 * the reference interface (host/Parallel_*.hpp, host/ParallelTestRunner.hpp,
 * host/gpu_exec.cpp) and the Python ctypes plumbing used by tests and bench.py.
 *
 * What each entry replaces in the reference (/root/reference/...):
 *
 *   cycle level (context API)
 *     pgmg_create / pgmg_set_problem / pgmg_vcycle / pgmg_get_solution
 *         ParallelMultiGridSolver::v_cycle(double*, double*, int, double)
 *             3_part_parallel/Parallel_Mg.cu:21-60, driven by
 *         ParallelTestRunner::run_v_cycle()  3_part_parallel/ParallelTestRunner.cu:152-186
 *         (numerics: MultigridSolver::v_cycle, 2_part_MG/MultiGrid.hpp:57-94)
 *     pgmg_wcycle
 *         ParallelMultiGridSolver::w_cycle  3_part_parallel/Parallel_Mg.cu:62-102
 *         (numerics: MultigridSolver::w_cycle, 2_part_MG/MultiGrid.hpp:96-136)
 *     pgmg_fcycle
 *         MultigridTestRunner::run_cycle("F-cycle") 2_part_MG/MultiGridTestRunner.hpp:192-205
 *         + MultigridSolver::f_cycle / compute_coarsest_grid, MultiGrid.hpp:28-55,138-183
 *
 *   op level (caller-owned device arrays in the reference's row-major layout,
 *   element (y, x) at p[y*W + x]; the optional `stream` is a hipStream_t)
 *     pgmg_jacobi    Parallel::ComputeJacobi       3_part_parallel/Parallel_Method.cu:144-160
 *                    (in place on d_x like the reference's, each sweep exactly the
 *                    out-of-place sweep; numerics of JacobiSmoother::smooth,
 *                    Smoother.hpp:38-116: v+1 sweeps with the residual-norm early exit)
 *     pgmg_residual  Parallel::ComputeResidual     Parallel_Method.cu:162-173
 *                    (DynamicGridUtils::compute_residual, DynamicGridUtils.hpp:59-69)
 *     pgmg_restrict  Parallel::ComputeRestriction  Parallel_Method.cu:175-186
 *                    (MultigridSolver::restrict_full_weighting, MultiGrid.hpp:187-205)
 *     pgmg_prolong   Parallel::ComputeProlungator  Parallel_Method.cu:188-199
 *                    (mode 0: MultigridSolver::prolongation, MultiGrid.hpp:208-226;
 *                     mode 1: the symmetric prolungator_kernel, Parallel_Method.cu:79-138)
 *     pgmg_norm      DynamicGridUtils::norm        DynamicGridUtils.hpp:21-27
 *     pgmg_rhs       DynamicGridUtils::compute_rhs DynamicGridUtils.hpp:111-124
 *
 * Special values.  The bit-for-bit promise holds for any input words, not only for ordinary
 * numbers: every output word that the reference (mg_cpu_exec) leaves non-NaN is bitwise the
 * reference's -- the sign of a zero, subnormals (nothing is flushed, in fp64 or fp32) and
 * +-Inf included -- and an output word is NaN exactly where the reference's is.  A NaN's sign
 * and payload are unspecified (x86 and CDNA produce different default NaNs, and a compiler may
 * commute the operands of an add), so pgmg_solution_hash of a grid that holds a NaN is not
 * comparable between the two.  Early-exit decisions, and with them the sweep and exit counts
 * of pgmg_stats, are the reference's for any norm: sqrt(sum r^2) < eps does not fire on a sum
 * that is NaN or that overflowed to Inf, and fires on a sum of exactly 0 unless eps is 0.
 * fp32 contexts follow the same rule against the fp32 restatement of the reference, and
 * convert the caller's doubles at the ABI by IEEE round-to-nearest-even (overflow to Inf,
 * gradual underflow, NaN stays NaN).  One deliberate exception to "converted at the ABI":
 * pgmg_set_problem_device only binds.  The solution of a device-bound problem is the caller's
 * array, so until the first call writes it pgmg_get_solution returns the caller's own doubles,
 * unrounded, also in an fp32 context; the first call reads them rounded as above and leaves the
 * fp32 result, frame included, in the array (tests/test_gpu_special_cycles.py::
 * test_abi_f32_conversion[device]).  Two things the reference's F-cycle does, kept as they are:
 * it reads no frame word of phi, and a -0 of phi leaves no trace in its result (test_f_cycles).
 * Pinned by tests/test_oracle_special.py (the restatement
 * against the compiled reference) and tests/test_gpu_special_ops.py, test_gpu_special_cycles.py
 * (the library against the restatement).
 *
 * Threading: a context is driven by one host thread; not thread-safe.
 */
#ifndef PGMG_H
#define PGMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGMG_OK 0
#define PGMG_ERR_ARG (-1)     /* bad argument (N not 2^k+1, null pointer, ...) */
#define PGMG_ERR_HIP (-2)     /* HIP runtime error                              */
#define PGMG_ERR_NOMEM (-3)   /* device allocation failed                       */
#define PGMG_ERR_COMM (-4)    /* RCCL error                                     */
#define PGMG_ERR_STATE (-5)   /* call out of order (e.g. vcycle before set_problem) */

/* prolongation flavours */
#define PGMG_PROLONG_REFERENCE 0 /* mg_cpu_exec: fine row/col 1 uncorrected */
#define PGMG_PROLONG_SYMMETRIC 1 /* gpu_exec's prolungator_kernel; fine boundary set 0  */

/* element type of every level grid (pgmg_config.precision) */
#define PGMG_PRECISION_FP64 0    /* bit-identical to mg_cpu_exec (the default)            */
#define PGMG_PRECISION_FP32 1    /* fp32 storage and arithmetic, half the HBM bytes; norms
                                    accumulated in fp64; parity stated as a tolerance
                                    against fp64 (the reference is fp64-only).
                                    Host arrays at the ABI stay double.                     */

/* config flags */
#define PGMG_FLAG_NO_GRAPH 1u    /* launch eagerly instead of replaying a hipGraph */
#define PGMG_FLAG_TIME_FINE 2u   /* eager launches + hipEvents around every finest-level
                                    pass (see pgmg_fine_pass_time)                  */
#define PGMG_FLAG_UNFUSED 4u     /* one kernel per smoother sweep even when v1 = v2 = 1
                                    (the general path; same results)                */
#define PGMG_FLAG_NO_CROSS 16u   /* do not fuse the finest level's post-smooth with the
                                    next cycle's pre-smooth (same results)           */
#define PGMG_FLAG_STORED_RHS 32u /* always stream f from HBM; by default, when f is the
                                    analytic RHS (set_problem f = NULL), the finest-level
                                    cross-cycle pass regenerates it in-kernel from two
                                    sine tables (bitwise the same values, 8 B/pt less) */
#define PGMG_FLAG_EXACT_DIST 64u /* decide every smoother early-exit check in-stream (a
                                    fix-up launch per check; on row strips an allreduce
                                    each) instead of speculatively (validated once per
                                    call, rollback on doubt; same results)            */
#define PGMG_FLAG_SOLO 128u     /* measurement only: world > 1 with a null transport — this
                                    rank's share of the strip work on one GPU, no messages
                                    (halos/gathered rows stale, allreduces local); results
                                    are meaningless, timings are one rank's compute     */
#define PGMG_FLAG_LOOPBACK 8u    /* world > 1 with ranks as threads of one process on
                                    one GPU: nccl_unique_id is a pgmg_loopback hub
                                    (test transport for the strip decomposition)    */
/* Alternative execution plans with the same results (each is bitwise-tested against the
 * default and the oracle; they exist to test the default's building blocks apart): */
#define PGMG_FLAG_NO_RECOMPUTE 256u /* coarse levels store their pre-smoothed iterate
                                       instead of recomputing it from f in k_post     */
#define PGMG_FLAG_NO_PIN 512u       /* F-cycle: a separate prolongation pass into the
                                       zeroed finer grid instead of k_pre computing it
                                       on the fly                                      */
#define PGMG_FLAG_NO_R2 1024u       /* F-cycle: one full-weighting level per restriction
                                       pass instead of two                             */
#define PGMG_FLAG_FAST 4096u    /* FAST mode: the finest
                                   level's cross-cycle pass shares each iterate's neighbour
                                   sum between its Jacobi sweep and its residual and forms
                                   the residuals with FMA — not the reference's expression
                                   order, so phi agrees with the EXACT default within
                                   1e-12 relative (after <= 10 cycles) instead of bitwise.
                                   One GPU (row strips ignore it); everything else exact */
#define PGMG_FLAG_NO_SPEC_FIRE 32768u /* speculative calls without segment planning,
                                       per-cycle speculation windows and levels predicted
                                       to fire (the r02 policy: a level that will fire
                                       decides in-stream from the call's start), and
                                       W-cycles without plans (every bulk check
                                       in-stream).  Results are identical either way.
                                       (8192u until r03.)                              */
/* Retired bits, rejected by pgmg_create with PGMG_ERR_ARG so that a caller built against an
   older header fails loudly instead of silently getting another option:
   8192u  -- PGMG_FLAG_L1POST until r02 (level 1's post-smooth inside the finest pass; removed
             in r03), then PGMG_FLAG_NO_SPEC_FIRE in r03;
   16384u -- the 129x129 level inside the tail's launch (built in r03, bitwise, measured
             slower: one CU's fp64 VALU needs ~1.2 us per pass over 129^2 points; removed) */
#define PGMG_FLAGS_RETIRED (8192u | 16384u)
#define PGMG_FLAG_NO_CTILE 65536u /* the small coarse levels (N <= 513, entered with x0 = 0)
                                     run the row-marching fused passes instead of the 2D LDS
                                     tile passes (r04).  Results are identical either way */
#define PGMG_FLAG_NO_CARRY 131072u /* do not carry the next call's pre-smooth across
                                      pgmg_vcycle calls (the carry: below pgmg_vcycle).  Results
                                      and statistics are identical either way */
#define PGMG_FLAG_FULL_CHECKS 2097152u /* one GPU: the finest level's cross-cycle pass sums its two
                                          early-exit checks over every row on speculative calls
                                          too, instead of over a sample of the rows (a lower
                                          bound, enough to show that a check cannot fire: below
                                          pgmg_spec_sampled_info).  Results and statistics are
                                          identical either way */
#define PGMG_FLAG_TIME_COMM 262144u /* world > 1: hipEvents around every collective group
                                       (grouped halo exchange, all-to-all, allreduce) on the
                                       context's stream, read by pgmg_comm_stats */
#define PGMG_FLAG_NO_SHUFFLE 524288u /* one GPU: allocate the grids of 256 MB and more with
                                        plain hipMalloc instead of from 2 MB physical chunks
                                        mapped in a shuffled order (the finest
                                        pass runs ~3-4 % faster in a process's first context) */
#define PGMG_FLAG_NO_SPIN 1048576u /* one GPU: a speculative call waits for its validation with a
                                      blocking stream wait instead of polling the reply word in
                                      pinned memory (pgmg_spec.hip reply_wait) */
#define PGMG_FLAG_HOST_TRANSPORT 2048u /* world > 1 without RCCL: nccl_unique_id points to
                                       a pgmg_host_transport; every message and reduction
                                       is staged through host memory and handed to the
                                       caller's functions (MPI, torch.distributed/gloo,
                                       ...; several ranks may share one GPU)           */

/* The caller's transport for PGMG_FLAG_HOST_TRANSPORT.  Every function is called by all
 * ranks in the same order (collective, blocking) and returns 0 on success; any other value
 * fails the library call with PGMG_ERR_COMM.
 *   exchange: one group of point-to-point messages: send send_bytes[i] bytes of host
 *     buffer send_buf[i] to rank send_peer[i], receive recv_bytes[i] bytes from
 *     recv_peer[i] into recv_buf[i]; messages between two ranks match in posting order
 *     (the semantics of the RCCL path's grouped ncclSend/ncclRecv).
 *   allreduce_sum_f64: v[i] = sum over ranks, in place; the sum taken in rank order
 *     (0.0 + v_0 + v_1 + ...) keeps every rank's decisions identical and equal to the
 *     in-process loopback transport's.
 *   allreduce_min_u32: v[i] = min over ranks, in place. */
typedef struct pgmg_host_transport {
    void *user;
    int (*exchange)(void *user, int nsend, const int *send_peer, const void *const *send_buf,
                    const unsigned long long *send_bytes, int nrecv, const int *recv_peer,
                    void *const *recv_buf, const unsigned long long *recv_bytes);
    int (*allreduce_sum_f64)(void *user, double *v, int n);
    int (*allreduce_min_u32)(void *user, unsigned *v, int n);
} pgmg_host_transport;

typedef struct pgmg_config {
    int N;             /* points per side incl. boundary; 2^k + 1, k >= 2        */
    int v1, v2;        /* pre/post smoother num_iter (v+1 sweeps), default 1, 1  */
    int coarse_iter;   /* num_iter on the coarsest grid, default 10 (11 sweeps); >= 0 */
    int n_coarse;      /* recursion floor N_coarse, default 5; >= 3.  The coarsest level,
                          the first N_l = (N_{l-1} - 1) / 2 + 1 with N_l <= n_coarse, runs in
                          the one-workgroup tail and may have at most 65 points per side:
                          pgmg_create returns PGMG_ERR_ARG otherwise (N 257 with n_coarse 129
                          or 200; N 257 with 100, 65 with 1000, 33 with 33 are legal)      */
    int alpha;         /* W-cycle recursion count, default 3; 1 .. 15 (the tail counts a
                          level's visits in 4 bits): pgmg_create returns PGMG_ERR_ARG above */
    double eps;        /* smoother early-exit tolerance, default 1e-7; <0: never */
    double a, p, q;    /* domain edge and RHS wave numbers, default 1, 1, 1: the reference's
                          globals (globals.cpp:2-4), f = pi^2 / a^2 (p^2 + q^2) u with
                          u = sin(p pi x / a) sin(q pi y / a).  a: finite and not 0 (a < 0
                          is legal: h < 0, h^2 > 0); p, q: finite -- negative, zero (f = 0,
                          then pgmg_monitor's exact_norm is 0 and rel_error is err_norm / 0:
                          NaN for phi = 0, Inf otherwise, as the reference prints) and
                          non-integer values (u != 0 on the far boundary, while phi's
                          boundary stays the caller's) are legal.  pgmg_create returns
                          PGMG_ERR_ARG for a = 0 and for a non-finite a, p or q           */
    int tail_n;        /* levels with N <= tail_n run in one workgroup (<= 65)   */
    int device;        /* HIP device ordinal, default 0                          */
    unsigned flags;    /* PGMG_FLAG_*                                            */
    /* row-strip domain decomposition over `world` ranks (one process per GPU). */
    int rank, world;   /* default 0, 1                                           */
    const void *nccl_unique_id;  /* 128-byte ncclUniqueId when world > 1      */
    int gather_n;      /* levels with N <= gather_n collapse to one grid, replicated
                          on every rank (world > 1)                               */
    int precision;     /* PGMG_PRECISION_FP64 (default) or PGMG_PRECISION_FP32    */
    int cross_min_n;   /* the finest level's post-smooth of cycle k and pre-smooth of
                          cycle k+1 are one pass from this N up (default 2049; small
                          values let tests exercise it on small grids)            */
    int spec_segment;  /* speculative calls: at most this many cycles per validated
                          segment (0 = sized by the log buffer; tests set it small) */
    double comm_timeout_s; /* row strips over RCCL: a stream wait that sees no progress
                          for this long aborts the communicator and returns
                          PGMG_ERR_COMM (default 600); RCCL's asynchronous error
                          state is polled while waiting                            */
    double h0;         /* finest-level mesh width; 0 (default): a / (N - 1).  The
                          reference's cycle entry points take h from the caller
                          (MultiGrid.hpp:57, Parallel_Mg.cu:21); coarse levels double
                          it (MultiGrid.hpp:83)                                    */
} pgmg_config;

typedef struct pgmg_ctx pgmg_ctx;

/* Fill `cfg` with the reference defaults for grid size N. */
int pgmg_config_default(pgmg_config *cfg, int N);

int pgmg_create(pgmg_ctx **ctx, const pgmg_config *cfg);
int pgmg_destroy(pgmg_ctx *ctx);

/* Upload phi0 (N*N, NULL -> zeros) and f (N*N, NULL -> the analytic RHS of
 * DynamicGridUtils::compute_rhs, generated on the device bit-identically from
 * host libm sine tables).  Host arrays in the reference layout (pitch N).  With
 * world > 1 every rank passes the full arrays (or NULLs) and keeps its strip. */
int pgmg_set_problem(pgmg_ctx *ctx, const double *phi0, const double *f);

/* Device-resident problem: the reference's memory contract.  ParallelMultiGridSolver::
 * v_cycle(phi, f, N, h) (3_part_parallel/Parallel_Mg.cu:21-60) updates in place arrays the
 * caller allocated in device-accessible memory (cudaMallocManaged,
 * ParallelTestRunner.cu:162-163).  After this call every pgmg_vcycle / wcycle / fcycle works
 * on the caller's DEVICE arrays in the reference layout (N*N doubles, pitch N): phi is read
 * and updated in place, synchronously (the call returns when phi holds the result), with no
 * host transfer.  f = NULL: the analytic RHS of compute_rhs (regenerated in-kernel, never
 * read); otherwise the caller's f, copied on the device into the context at every call (the
 * caller may change it between calls).  With phi from pgmg_alloc_grid on a cross-fused fp64
 * context (N >= cross_min_n) the finest-level passes read and write phi where it lies (the
 * same HBM bytes as a call on the context's own grids); any other device pointer is staged
 * with device-to-device copies before and after each call.  One GPU (world 1).  Resets the
 * statistics like pgmg_set_problem; pgmg_set_problem unbinds.  pgmg_get_solution /
 * pgmg_solution_hash / pgmg_residual_norm read the bound phi. */
int pgmg_set_problem_device(pgmg_ctx *ctx, double *phi, const double *f);
/* bound = a device problem is bound; inplace = its calls read / write phi in place */
int pgmg_problem_device_info(pgmg_ctx *ctx, int *bound, int *inplace);
/* An N*N device grid in the reference layout (pitch N, zeroed) with guard rows before and
 * after it, so the finest passes may read past its edges: what the in-place path of
 * pgmg_set_problem_device needs (the mirror's stand-in for cudaMallocManaged). */
int pgmg_alloc_grid(double **ptr, int N);
int pgmg_free_grid(double *ptr);
/* *serial = a number unique to this pgmg_alloc_grid allocation (never reused), 0 when ptr is
 * not a live pgmg_alloc_grid grid: lets a caller that caches a binding by pointer (the mirror's
 * ParallelMultiGridSolver) notice a grid freed and re-allocated at the same address. */
int pgmg_grid_serial(const double *ptr, unsigned long long *serial);
/* *is_device = 1 when p is device (or managed) memory of the HIP runtime. */
int pgmg_pointer_is_device(const void *p, int *is_device);

/* Enqueue `ncycles` cycles on the context's stream (asynchronous; a speculative call,
 * see pgmg_dist_info, returns after the device has finished it).
 * pgmg_fcycle: one F-cycle = restrict phi to n_coarse, then per level up smooth(3),
 * prolongation into a zeroed finer grid, analytic RHS of that grid (h chain starting at
 * 1/(n_coarse-1)), one V-cycle; the f given to pgmg_set_problem is left untouched
 * (MultiGridTestRunner.hpp:192-205).  On row strips as well (world > 1).  On one GPU an
 * F-cycle call is speculative too (its bulk checks recorded "does not fire" and validated once
 * after the call; a rollback reruns the call in-stream from the saved restricted grid and the
 * problem's later F calls decide in-stream); PGMG_FLAG_EXACT_DIST turns that off. */
/* The carry (r06; one GPU, cross-fused contexts, problems set with pgmg_set_problem): a
 * speculative V call ends with a finest-level pass that also runs the NEXT cycle's pre-smooth,
 * residual and restriction (MultiGrid.hpp:57-94's first half), keeps the restriction in a
 * context-owned buffer and checks it; the next pgmg_vcycle on the same problem starts from it
 * instead of running its own first pass (its first finest pass recomputes the pre-smooth from
 * phi in registers: no pass and no byte is added).  Entries that only read the problem (pgmg_get_solution, pgmg_solution_hash,
 * pgmg_residual_norm, pgmg_monitor, pgmg_history, pgmg_stats*, pgmg_sync ...) keep the carry
 * (pgmg_solve's checks between its one-cycle calls too); every entry that changes phi,
 * f, eps, the flags or the cycle kind (pgmg_set_problem*, pgmg_set_eps, pgmg_wcycle,
 * pgmg_fcycle, pgmg_fmg, pgmg_damp, pgmg_bench_sweep, pgmg_phi_device -- its pointer allows
 * writes -- ) drops it.
 * A carried pre-smooth whose early-exit check could fire is dropped, not rolled back.  Results
 * and statistics (its two sweeps count in the call that uses them) equal the uncarried ones,
 * bit for bit.  PGMG_FLAG_NO_CARRY turns it off; pgmg_carry_info counts it. */
int pgmg_vcycle(pgmg_ctx *ctx, int ncycles);
int pgmg_wcycle(pgmg_ctx *ctx, int ncycles);
int pgmg_fcycle(pgmg_ctx *ctx, int ncycles);
int pgmg_sync(pgmg_ctx *ctx);

/* Download phi (N*N, reference layout).  world > 1: every rank receives the
 * full grid (strips are gathered to all ranks). */
int pgmg_get_solution(pgmg_ctx *ctx, double *phi_host);
/* Download the level-0 right-hand side as the context stores it (N*N, reference layout, an fp32
 * context's values widened): the f given to pgmg_set_problem, the analytic RHS it generated for
 * f = NULL, the last staged copy of a device-bound problem's f, or the divergence pgmg_project
 * wrote.  One GPU (world 1), after pgmg_set_problem*; only reads the problem. */
int pgmg_get_rhs(pgmg_ctx *ctx, double *f_host);
/* The same with the strips gathered to rank `root` only (collective: every rank calls it;
 * ranks other than root may pass phi_host = NULL).  root < 0: every rank, as above. */
int pgmg_gather_solution(pgmg_ctx *ctx, int root, double *phi_host);

/* FNV-64-style hash of phi's IEEE words in the reference layout (h = 1469598103934665603,
 * h = (h ^ word) * 1099511628211 per element, row-major N*N): the checksum of the golden
 * fixtures (tests/golden/cycles.json).  Collective on row strips; the value lands on rank
 * `root` (root < 0: every rank), the others get 0. */
int pgmg_solution_hash(pgmg_ctx *ctx, int root, unsigned long long *hash);

/* sqrt(sum over interior of r^2) for the current phi (synchronous). */
int pgmg_residual_norm(pgmg_ctx *ctx, double *out);

/* ---- Convergence monitor and solve-to-tolerance ----------------------------------------
 * The counterpart of the reference driver's per-cycle history (MultigridTestRunner::run_cycle,
 * 2_part_MG/MultiGridTestRunner.hpp:190-244: compute_residual + norm after each cycle, and with
 * flag_err_norm_iteration ||phi - u|| / ||u||, :110-122 and :252-254).
 *
 * pgmg_monitor: one streaming pass over the current finest-level iterate, where it lies (the
 * context's grid, or the caller's device arrays of pgmg_set_problem_device: nothing is staged or
 * copied), gives up to three fp64 sums:
 *   PGMG_MON_RESIDUAL  res_norm = sqrt(sum over interior points of r^2), r = f - ih (4x - x_l -
 *                      x_r - x_u - x_d) in the expression order of DynamicGridUtils::
 *                      compute_residual (DynamicGridUtils.hpp:59-69), evaluated in the context's
 *                      element type, squared and summed in double;
 *   PGMG_MON_ERROR     err_norm = sqrt(sum over ALL N*N points, boundary included, of e^2),
 *                      e = (double)phi - u, u = sin(p pi x / a) sin(q pi y / a) from the host's
 *                      sine tables (compute_function's product); exact_norm = sqrt(sum u^2);
 *                      rel_error = err_norm / exact_norm.  Analytic problems only (f = NULL at
 *                      pgmg_set_problem*): PGMG_ERR_STATE otherwise.
 * Fields that were not asked for are NaN.  The sums are deterministic: per-workgroup partials in
 * a fixed lane and row order, added in index order by a second launch (no floating-point
 * atomics), the decomposition a function of N and the rank's rows only -- the same state gives
 * the same bits, eager or graph, context-owned or device-bound.  Per-point terms are the
 * reference's; only the summation order differs, so a norm agrees with the sequential sum within
 * N^2 * 2^-52 relative.  Synchronous; collective on row strips (one halo exchange of phi, one
 * rank-ordered allreduce of the three sums: every rank gets identical bits).
 * pgmg_monitor, pgmg_monitor_time and pgmg_history only read the problem: they keep the carry. */
#define PGMG_MON_RESIDUAL 1u
#define PGMG_MON_ERROR    2u   /* analytic problems only (f = NULL at set_problem*) */
typedef struct pgmg_monitor_out { double res_norm, err_norm, exact_norm, rel_error; } pgmg_monitor_out;
int pgmg_monitor(pgmg_ctx *ctx, unsigned what, pgmg_monitor_out *out);
/* Measurement: `reps` monitor passes (both launches each) back to back on the context's stream
 * between two hipEvents, after two warm ones; mean device ms per pass, and the algorithmic HBM
 * bytes of one pass (8 B per point of phi, + 8 B per interior point of a stored f; x elem/8). */
int pgmg_monitor_time(pgmg_ctx *ctx, unsigned what, int reps, double *ms_per_pass, double *bytes);

/* pgmg_solve: cycle until the residual norm meets a tolerance.  Check 0 happens before any
 * cycle; at check i, after k_i cycles, with norm r_i, in this order:
 *   1. r_i not finite                          -> PGMG_STOP_NONFINITE
 *   2. r_i <= max(atol, rtol * r_0)            -> PGMG_STOP_CONVERGED
 *   3. i >= 1 and stall_ratio > 0: r_i > stall_ratio * r_{i-1} extends a streak, anything else
 *      resets it; a streak of stall_checks     -> PGMG_STOP_STALLED
 *   4. k_i >= max_cycles                       -> PGMG_STOP_MAX_CYCLES
 * otherwise min(check_every, max_cycles - k_i) more cycles run, one pgmg_vcycle / pgmg_wcycle /
 * pgmg_fcycle call per chunk.  phi and pgmg_stats afterwards are bit for bit those of
 * info.cycles plain cycles of that kind (the monitor adds no sweep and writes nothing a cycle
 * reads); with check_every = 1 a V solve runs at the carried one-cycle-call rate.  Invalid
 * options (negative counts, check_every < 1, stall_checks < 1, negative or non-finite
 * tolerances, an unknown cycle or monitor bit) return PGMG_ERR_ARG before anything is enqueued;
 * PGMG_MON_ERROR on a problem with a caller's f returns PGMG_ERR_STATE.  Collective on row
 * strips: every rank sees the same norms and stops at the same check. */
#define PGMG_CYCLE_V 0
#define PGMG_CYCLE_W 1
#define PGMG_CYCLE_F 2
#define PGMG_STOP_CONVERGED 1
#define PGMG_STOP_MAX_CYCLES 2
#define PGMG_STOP_STALLED 3
#define PGMG_STOP_NONFINITE 4
typedef struct pgmg_solve_opts {
    int cycle, max_cycles, check_every;
    double rtol, atol;          /* target = max(atol, rtol * r0) */
    double stall_ratio;         /* 0 = no stall test */
    int stall_checks;
    unsigned monitor;           /* PGMG_MON_RESIDUAL always on; | PGMG_MON_ERROR records rel_error too */
} pgmg_solve_opts;
typedef struct pgmg_solve_info {
    int cycles, checks, reason;
    double res0, res, rel_error /* NaN when not monitored */, elapsed_ms /* host wall time of the call */;
} pgmg_solve_info;
/* V, 30 cycles, a check every cycle, rtol 1e-3, atol 0, no stall test (stall_checks 2) */
int pgmg_solve_opts_default(pgmg_solve_opts *o);
int pgmg_solve(pgmg_ctx *ctx, const pgmg_solve_opts *o, pgmg_solve_info *info);
/* The last pgmg_solve's checks, check 0 first: *n = their number; the first min(cap, *n) land
 * in cycle[] (cycles run before the check), res[] and rel_error[] (NaN when not monitored); any
 * of the arrays may be NULL. */
int pgmg_history(pgmg_ctx *ctx, int cap, int *cycle, double *res, double *rel_error, int *n);

/* ---- Damping pass and damped solve ------------------------------------------------------
 * The cycles' smoother is the reference's undamped Jacobi: its iteration matrix has the
 * eigenvalues lambda = (cos tx + cos ty) / 2, and the most oscillatory error (lambda ~ -1, the
 * checkerboard) passes through v1 + v2 sweeps and every coarse grid unchanged.  A right-hand side
 * that holds it (any but the smooth analytic one) stalls plain cycles at a factor of 0.94-0.96.
 *
 * pgmg_damp: ONE finest-level damped-Jacobi correction of the current iterate,
 *     phi <- phi + w * r,   r = f - ih (4x - x_l - x_r - x_u - x_d)   (pgmg_monitor's r),
 *     w = (T)(omega * 0.25 * (h0 * h0))   the double product taken left to right, then converted,
 * on every interior point, in the context's element type T with two roundings (no fused
 * multiply-add); boundary points are never written.  Every r is formed from the phi of before
 * the pass: the result is exactly the out-of-place formula, whatever the launch geometry.  It is
 * the monitor's pass (same reads, same decomposition, same partial sums) that also writes: with
 * res_norm != NULL it returns the residual norm of phi BEFORE the update, bit for bit what
 * pgmg_monitor(PGMG_MON_RESIDUAL) returns on that state.  At omega = 1/2 the factor on an error
 * mode is (1 + lambda) / 2: 0 on the checkerboard, ~1 on the smooth modes the cycle handles.
 * Context-owned grids and the caller's arrays of pgmg_set_problem_device (read as the monitor
 * reads them, written back as double) alike; fp64 and fp32.  Synchronous, like pgmg_monitor.  It
 * is an entry that changes phi: it drops the carry.  It keeps the speculation history
 * (validation and rollback protect the results either way) and leaves the sweep and early-exit
 * statistics untouched.
 *
 * pgmg_solve_damped: pgmg_solve's loop and stop rule with every check made by the damping pass.
 * At check i the pass yields r_i, the norm of the iterate as the cycles left it, and applies the
 * correction; then the rule decides; then the next chunk of cycles runs.  The correction of the
 * stopping check is applied too (the pass cannot know the decision), so phi afterwards is
 * damp(x_k), x_k the iterate info.res was measured on.  For 0 < omega <= 1 the update multiplies
 * the residual by I - omega (h^2/4) A, a symmetric matrix with its spectrum inside (-1, 1): in
 * exact arithmetic the returned phi's residual norm is <= info.res (observed 0.80-0.86 x at
 * omega = 1/2).  pgmg_history records the r_i; with PGMG_MON_ERROR rel_error is that of the
 * pre-update iterate (the same pass sums it).  Chunks after a damp start uncarried.
 *
 * Tested off the defaults, bitwise against tests/damp_model.py at the context's own mesh width
 * (tests/test_gpu_late_params.py): the pass with a = -2, 1e-3 .. 1000, negative, zero and
 * non-integer p, q and h0 = 0.7 / (N - 1), 1 / N, with the analytic f regenerated, with
 * PGMG_FLAG_STORED_RHS and with a caller's f, fp64 and fp32, context-owned and device-bound;
 * the solve with V-cycles, W-cycles at alpha 1, 2 and 4, F-cycles, check_every 2, PGMG_MON_ERROR
 * at a caller's h0, n_coarse 9 and tail_n 17.
 *
 * pgmg_damp_time: `reps` damping passes (the pass, the scatter of its deferred edges and the
 * reduction each) back to back between two hipEvents, after two warm ones; mean device ms per
 * pass and its algorithmic bytes (the monitor's model + one element per interior point
 * written).  Leaves phi changed.
 *
 * omega not finite, <= 0 or > 1, a null ctx / opts / info, invalid opts: PGMG_ERR_ARG.  Before
 * pgmg_set_problem*: PGMG_ERR_STATE.  world > 1: PGMG_ERR_STATE -- one GPU only, as pgmg_fmg.
 * PGMG_MON_ERROR with a caller's f: PGMG_ERR_STATE.  All before anything is enqueued. */
int pgmg_damp(pgmg_ctx *ctx, double omega, double *res_norm);
int pgmg_solve_damped(pgmg_ctx *ctx, const pgmg_solve_opts *o, double omega, pgmg_solve_info *info);
int pgmg_damp_time(pgmg_ctx *ctx, double omega, int reps, double *ms_per_pass, double *bytes);

/* ---- Full multigrid for the problem's own right-hand side -------------------------------
 * pgmg_fcycle is the reference's F-cycle: it rebuilds the ANALYTIC right-hand side on every
 * level, so a caller who passed an f of their own gets the answer to another problem.
 * pgmg_fmg(ctx, nu) replaces phi with the full-multigrid solution of the context's problem:
 *   levels  N_0 = N, N_{l+1} = (N_l - 1) / 2 + 1 down to the first N_L <= n_coarse;
 *           h_l = h_0 * 2^l (h_0: pgmg_config.h0, or a / (N - 1)).
 *   1. f_0 is the problem's level-0 right-hand side as stored: the caller's f, or the analytic
 *      RHS that pgmg_set_problem*(.., NULL) keeps.  f_{l+1} = full weighting of f_l on the
 *      interior points (1/4 centre + 1/8 edges + 1/16 corners, the order of compute_coarsest_grid,
 *      MultiGrid.hpp:28-55), boundary 0.
 *   2. u_L = 0, then nu x v_cycle(u_L, f_L, N_L, h_L) (MultiGrid.hpp:57-94; at N <= n_coarse
 *      that is the coarsest smoother call, coarse_iter + 1 sweeps).
 *   3. for l = L-1 .. 0: u_l = C(u_{l+1}), then nu x v_cycle(u_l, f_l, N_l, h_l).
 *   The current phi (boundary included) is ignored and overwritten with u_0, whose boundary
 *   is 0; f is left untouched.
 * C is the tensor-product cubic interpolation from Nc to Nf = 2 Nc - 1 points per side, every
 * fine point assigned: first along x on every coarse row, then along y on the x-interpolated
 * rows.  Along one line c[0 .. Nc-1] -> fine[0 .. Nf-1]:
 *   fine[2i]   = c[i]
 *   fine[k]    = (9.0 * (b + c) - (a + d)) * 0.0625            odd k, 3 <= k <= Nf-4, with
 *                a, b, c, d = c[(k-3)/2], c[(k-1)/2], c[(k+1)/2], c[(k+3)/2]
 *   fine[1]    = (5.0 * c[0] + 15.0 * c[1] - 5.0 * c[2] + c[3]) * 0.0625
 *   fine[Nf-2] = (5.0 * c[Nc-1] + 15.0 * c[Nc-2] - 5.0 * c[Nc-3] + c[Nc-4]) * 0.0625
 * evaluated left to right in the context's element type, one rounding per operation (no fused
 * multiply-add).  This needs N_L >= 5: with n_coarse < 5 (N_L = 3) the call returns
 * PGMG_ERR_ARG.  N = 5 is legal (no climb, step 2 only).  Bilinear interpolation would not do:
 * with a second-order discretisation its FMG error grows with N relative to the discretisation
 * error; cubic with nu = 2 lands at 0.9 x the discretisation error at every size
 * (tests/test_fmg_cpu.py) for about 8/3 finest-level V-cycles of work.
 * nu < 1 or a null context: PGMG_ERR_ARG.  Before pgmg_set_problem*: PGMG_ERR_STATE.  world > 1:
 * PGMG_ERR_STATE -- row strips are NOT supported by this entry (one GPU only).  fp64 and fp32
 * contexts; problems set with pgmg_set_problem and pgmg_set_problem_device (the result lands in
 * the caller's phi: the climb runs on the context's grids and is copied out, synchronous like
 * pgmg_fcycle on a bound problem).  Every early-exit check is decided in-stream, so results and
 * the sweep count are the model's; the call is asynchronous on the context's stream otherwise.
 * It is an entry that changes phi: it drops the carry and resets the speculation history as
 * pgmg_set_problem does; the sweep and early-exit statistics continue.  A later pgmg_vcycle /
 * pgmg_wcycle / pgmg_solve continues from u_0.  pgmg_last_elapsed_ms reports the call's device
 * time.  The restricted f chain and the grids of the levels below the tail's top are allocated
 * on the first call (about 1/3 of a level-0 grid). */
int pgmg_fmg(pgmg_ctx *ctx, int nu);
/* ---- Damped full multigrid --------------------------------------------------------------
 * pgmg_fmg's cycles use the undamped smoother, which leaves the checkerboard error of every
 * level untouched: on an f that holds it (any but the smooth analytic one) plain FMG stops at
 * ||r|| / ||f|| ~ 1e-1.  pgmg_fmg_damped(ctx, nu, omega) is pgmg_fmg with step 3 changed to
 *   3. for l = L-1 .. 0: u_l = C(u_{l+1}), then nu x { v_cycle(u_l, f_l, N_l, h_l);
 *                                                     u_l <- damp(u_l, f_l, h_l, omega) }
 * damp is pgmg_damp's formula on that level: u + w * r with r = f_l - ih_l (4u - ...),
 * w = (T)(omega * 0.25 * (h_l * h_l)), out-of-place semantics, the boundary never written, two
 * roundings, no fused multiply-add, in the context's element type.  The coarsest level (step 2)
 * is not damped.  With omega = 1/2 and nu = 2 the result has ||r|| / ||f|| ~ 1e-3 on a random f
 * (tests/test_fmg_damped_cpu.py: 80-150 times below plain FMG) and, on the analytic problem,
 * the same 0.9 x discretisation error as plain FMG, for 2 nu / (1 - 1/4) damping passes' worth
 * of extra finest-level traffic; a damped solve that starts from it needs 4-6 cycles to
 * rtol 1e-6 where one from zero needs 11-13.
 * Everything else is pgmg_fmg's contract: nu < 1, n_coarse < 5 (N_L = 3) or a null context:
 * PGMG_ERR_ARG; omega not finite, <= 0 or > 1: PGMG_ERR_ARG; before pgmg_set_problem*:
 * PGMG_ERR_STATE; world > 1: PGMG_ERR_STATE; all before anything is enqueued.  fp64 and fp32;
 * problems set with pgmg_set_problem and pgmg_set_problem_device (the climb and every damp run
 * on the context's grids, never on the caller's array; the result is copied out, synchronous).
 * Otherwise asynchronous on the context's stream: the damps compute no norm, copy nothing and
 * wait for nothing.  Every early-exit check is decided in-stream; the sweep and early-exit
 * statistics are those of the cycles alone.  It drops the carry and resets the speculation
 * history.  f is left untouched.  The damping pass's side buffer is allocated on the first
 * call.  Tested off the defaults, bitwise against tests/fmg_damped_model.py with h_l = h0 * 2^l
 * (tests/test_gpu_late_params.py): a = -2, 1e-3 .. 1000, asymmetric, negative and non-integer
 * p, q, h0 = 0.7 / (N - 1) and 1 / N, n_coarse 9, 17 and 1000 (no climb), coarse_iter 0 and 30,
 * (v1, v2) = (2, 3), tail_n 9 and 17, a cross-fused level 0, the analytic f regenerated on
 * level 0 and PGMG_FLAG_STORED_RHS, a caller's f, fp64 and fp32. */
int pgmg_fmg_damped(pgmg_ctx *ctx, int nu, double omega);
/* ---- Full multigrid with Dirichlet data -------------------------------------------------
 * pgmg_fmg and pgmg_fmg_damped start from u_L = 0 and end with a zero boundary: a problem whose
 * phi carries boundary data gets the answer to another problem.  pgmg_fmg_bc(ctx, nu, omega)
 * is the same climb with the boundary the caller set.  Let g be the frame of the CURRENT phi at
 * the time of the call: rows 0 and N-1 and columns 0 and N-1 of level 0 (the context's phi, or
 * the caller's device array of pgmg_set_problem_device, in the context's element type).  The
 * levels, h_l and the restricted f chain (step 1) are pgmg_fmg's; the frame of level l is the
 * injection of g, g_l(j, i) = g(2^l j, 2^l i) on the frame points of the N_l x N_l grid; the
 * interior of phi is ignored.
 *   2. u_L = 0 on the interior and g_L on the frame, then nu x v_cycle(u_L, f_L, N_L, h_L).
 *   3. for l = L-1 .. 0: u_l = C(u_{l+1}), the same cubic interpolation, frame included; the
 *      frame of u_l is then overwritten with g_l (the interpolated frame differs from it by
 *      O(h^4); the caller's data is exact); then
 *      nu x { v_cycle(u_l, f_l, N_l, h_l);  if omega > 0: u_l <- damp(u_l, f_l, h_l, omega) }.
 *   phi is overwritten with u_0, whose frame is bit for bit g; f is left untouched.
 * omega == 0.0 is the undamped climb of pgmg_fmg, omega in (0, 1] adds pgmg_fmg_damped's damping
 * pass (the same formula, the boundary never written; the coarsest level is not damped); any
 * other omega (not finite, < 0 or > 1): PGMG_ERR_ARG.  With a frame of +0.0 everywhere phi and
 * the statistics are bitwise those of pgmg_fmg (omega == 0) or pgmg_fmg_damped.  A non-finite
 * frame value is no error: it propagates, as it does through the cycles.  On the analytic
 * problem with non-integer p, q and the exact solution's frame, nu = 2 lands at 0.92 - 1.0 x the
 * discretisation error (tests/test_fmg_bc_cpu.py), where the zero-frame climb is orders of
 * magnitude above it.  The model is tests/fmg_bc_model.py.
 * Everything else is pgmg_fmg's contract: nu < 1, n_coarse < 5 (N_L = 3) or a null context:
 * PGMG_ERR_ARG; before pgmg_set_problem*: PGMG_ERR_STATE; world > 1: PGMG_ERR_STATE; all before
 * anything is enqueued.  fp64 and fp32; problems set with pgmg_set_problem and
 * pgmg_set_problem_device (the caller's phi is staged into the context's grids first, g is taken
 * from there, the result is copied out: synchronous; asynchronous on the context's stream
 * otherwise).  Every early-exit check is decided in-stream; the sweep and early-exit statistics
 * continue and are the model's.  It drops the carry and resets the speculation history.  A later
 * pgmg_vcycle / pgmg_wcycle / pgmg_solve continues from u_0 and keeps its frame.  The frame
 * buffer (4 N elements) is allocated on the first call.  Cost over pgmg_fmg: the frame's save, a
 * fill of the coarsest grid and one to five launches of O(N_l) elements per level.  Tested off
 * the defaults with omega 0 and 1/2 on the parameter values listed for pgmg_fmg_damped, the frame
 * being the exact solution's (of order one on the far boundary for non-integer p, q or a
 * caller's h0) or random (tests/test_gpu_late_params.py). */
int pgmg_fmg_bc(pgmg_ctx *ctx, int nu, double omega);
/* Measurement: `reps` cubic interpolation passes level 1 -> level 0 back to back on the
 * context's stream between two hipEvents, after two warm ones; mean device ms per pass and its
 * algorithmic bytes (one element per fine point written + one per coarse point read).  Needs
 * N >= 9, world 1.  Leaves phi changed (call set_problem again before parity checks). */
int pgmg_fmg_interp_time(pgmg_ctx *ctx, int reps, double *ms_per_pass, double *bytes);

/* ---- Fourth-order solves by Richardson extrapolation -------------------------------------
 * The 5-point discretisation is second order: for smooth data its solution is
 * u_h = u + h^2 c(x) + O(h^4).  pgmg_solve_extrap(ctx, opts, nu, omega, info) solves the same
 * continuous problem on the grid and on the grid of every second point and combines the two: at
 * the coincident points u_h + (u_h - u_2h) / 3 is O(h^4), and the correction (u_h - u_2h) / 3 is
 * a smooth field of size h^2 whose cubic interpolation to the fine grid is exact to O(h^6), so
 * the whole fine grid becomes fourth order.  Cost: a quarter-size solve and two streaming passes.
 * fp64, one GPU.  Synchronous.  Every step always runs; the stop reasons of the two solves are
 * reported, never acted on:
 *   1. The half-resolution context.  Owned by ctx, created on the first call, destroyed by
 *      pgmg_destroy: pgmg_create on a copy of ctx's config with N' = (N + 1) / 2 and a mesh
 *      width of 2 h_0 (h_0: pgmg_config.h0, or a / (N - 1); the doubling is exact, as on the
 *      context's own level 1), world 1, everything else equal.  The copy's h0 is 2 * h0 where
 *      the caller gave one and stays 0 otherwise: a / (N' - 1) is 2 (a / (N - 1)) bit for bit,
 *      also for a < 0, where the mesh width is negative and could not be stated as an h0.
 *      Before each call its eps is set to ctx's current eps if they differ.
 *   2. Its problem.  phi' = the injection of the current phi, phi'(j, i) = phi(2j, 2i), the
 *      whole grid, so its frame is the injected frame; f' = the injection of the level-0
 *      right-hand side as stored (the caller's f, or the analytic RHS that
 *      pgmg_set_problem*(.., NULL) keeps).  Both are written on the device.  The child's problem
 *      is one with a caller's f (nothing regenerated, no PGMG_MON_ERROR); its statistics and
 *      speculation history start over.
 *   3. pgmg_fmg_bc(child, nu, omega), then pgmg_solve_damped(child, opts', omega, &info->coarse),
 *      opts' = opts with monitor = PGMG_MON_RESIDUAL.
 *   4. pgmg_fmg_bc(ctx, nu, omega), then pgmg_solve_damped(ctx, opts, omega, &info->fine);
 *      pgmg_history afterwards is this solve's.
 *   5. The extrapolation, on phi where it lies (the level-0 grid, or the caller's array of
 *      pgmg_set_problem_device), F = phi (Nf = N points per side), Cg = the child's phi (Nc = N'):
 *        D(j, i) = (F(2j, 2i) - Cg(j, i)) * K3      0 <= j, i < Nc, frame included; K3 the double
 *                  nearest 1/3 (0x3FD5555555555555): one rounding for the difference, one for the
 *                  product (a product, so the result does not depend on how a division is lowered)
 *        E = C(D)                                   pgmg_fmg's cubic interpolation, its formulas
 *                                                   and evaluation order
 *        F(y, x) <- F(y, x) + E(y, x)               1 <= y, x <= Nf - 2, one rounding
 *      Every D comes from the F of before the operation (two passes: D into a coarse-sized
 *      scratch grid, allocated on the first call, then the pointwise update); no fused
 *      multiply-add.  The frame of F is never written: a -0.0 there stays -0.0.
 * Afterwards phi's frame is bit for bit the one it had and f is untouched.  The entry changes
 * phi: it drops the carry and resets the speculation history, as pgmg_fmg_bc does.  pgmg_stats of
 * ctx counts its own FMG and solve; the child's sweeps and early exits are in info.  A later
 * pgmg_vcycle continues from the extrapolated phi.
 * What to ask for.  Check 0 of both solves is the FMG iterate, whose residual is already small,
 * so rtol (relative to check 0) says little: state the target as atol.  The extrapolation needs
 * both solves converged well below the h^4 it is after, atol ~ 1e-10 ||f||_2; what fp64 can
 * reach is ||r|| / ||f|| ~ 0.4 N^2 2^-52.  With the default eps = 1e-7 the smoother's early
 * exits fire at loose tolerances and break the order (atol = 1e-8 ||f||: error ratios 2.9 and
 * 11.5 instead of 16 at N = 257); with atol = 1e-11 ||f|| the order is intact but the solves take
 * 18-25 cycles instead of 13-16.  The entry leaves eps alone; eps < 0 (pgmg_config.eps) is
 * recommended.  The gain is largest where fp64 has room: useful for N <= 2049; at N = 16385 h^4
 * is below fp64 rounding, the entry runs there and gains nothing.  The model is
 * tests/extrap_model.py.  Tested off the defaults, bitwise against it (tests/
 * test_gpu_late_params.py): a = -2, 3 and 1000, asymmetric and non-integer p, q, h0 =
 * 0.7 / (N - 1) and 1 / N (the child then runs at an h0' that is not 1 / (N' - 1)), n_coarse 9,
 * coarse_iter 0, (v1, v2) = (2, 3), and N = 129 with tail_n = 17, where the child has bulk
 * levels of its own; context-owned and device-bound, staged and in place.
 * Errors, all before anything is enqueued and before a child is created.  PGMG_ERR_ARG: a null
 * argument; invalid opts (pgmg_solve's rule); nu < 1; omega not finite, <= 0 or > 1; N < 9; a
 * context or a child whose coarsest level has fewer than 5 points per side.  omega = 0 (the
 * undamped climb and solve) is refused: the undamped smoother leaves ||r|| / ||f|| at 1e-4 after
 * 150 V-cycles, and that algebraic error swamps the h^4 term (extrapolated error ratios scatter
 * between 2.4 and 15).  PGMG_ERR_STATE: before pgmg_set_problem*; world > 1; an fp32 context
 * (fp32 solves stall at ||r|| / ||f|| ~ 1e-5 .. 1e-3, a rounding floor that leaves the
 * extrapolated error at 2e-7 .. 2e-6 from N = 65 up: no better than second order);
 * PGMG_MON_ERROR with a caller's f. */
typedef struct pgmg_extrap_info {
    pgmg_solve_info fine, coarse;            /* the two damped solves; check 0 is the FMG iterate */
    long long coarse_sweeps, coarse_exits;   /* the half-resolution context's pgmg_stats */
    double extrap_ms;                        /* device time of the two extrapolation passes */
    double elapsed_ms;                       /* host wall time of the call */
} pgmg_extrap_info;
int pgmg_solve_extrap(pgmg_ctx *ctx, const pgmg_solve_opts *o, int nu, double omega,
                      pgmg_extrap_info *info);

/* ---- Gradient of the solution ------------------------------------------------------------
 * pgmg_gradient(ctx, order, scale, d_gx, d_gy, norm): both components of scale * grad(phi) of the
 * current phi on all N x N points, frame included, from one read of phi where it lies (the
 * context's level-0 grid, or the caller's bound array of pgmg_set_problem_device: nothing is
 * staged).  h is the context's finest mesh width (pgmg_config.h0, or a / (N - 1); negative for
 * a < 0), T its element type.  Every expression is evaluated left to right as written, one
 * rounding per operation, no fused multiply-add.  The frame uses one-sided stencils of the same
 * order.  Along one line v[0 .. n-1], n = N >= 5:
 *   order 2:  w = (T)(scale * 0.5 / h)                  the double expression, left to right, then
 *                                                       converted
 *     g[k]   = (v[k+1] - v[k-1]) * w                                          1 <= k <= n-2
 *     g[0]   = (4.0 * v[1] - 3.0 * v[0] - v[2]) * w
 *     g[n-1] = (3.0 * v[n-1] - 4.0 * v[n-2] + v[n-3]) * w
 *   order 4:  w = (T)(scale / (12.0 * h))
 *     g[k]   = (8.0 * (v[k+1] - v[k-1]) - (v[k+2] - v[k-2])) * w              2 <= k <= n-3
 *     g[0]   = (48.0 * v[1] - 25.0 * v[0] - 36.0 * v[2] + 16.0 * v[3] - 3.0 * v[4]) * w
 *     g[1]   = (18.0 * v[2] - 10.0 * v[1] - 3.0 * v[0] - 6.0 * v[3] + v[4]) * w
 *     g[n-1] = (25.0 * v[n-1] - 48.0 * v[n-2] + 36.0 * v[n-3] - 16.0 * v[n-4] + 3.0 * v[n-5]) * w
 *     g[n-2] = (10.0 * v[n-2] - 18.0 * v[n-3] + 3.0 * v[n-1] + 6.0 * v[n-4] - v[n-5]) * w
 * gx(y, .) is this along x on every row y, gy(., x) along y on every column x, frame rows and
 * columns included.  scale = -1 gives E = -grad(phi).  d_gx and d_gy are caller-owned device
 * arrays of N x N doubles at pitch N; an fp32 context computes in fp32 (a bound array's doubles
 * converted on load, as pgmg_monitor reads them) and stores the values widened.  Either output
 * may be NULL: the other component alone is computed and summed.  norm (may be NULL) receives
 * sqrt(sum gx^2 + gy^2) over all points that were computed, every term the T value widened to
 * double, squared and summed in double, deterministic by the monitor's scheme: per-workgroup
 * partials in a fixed lane and row order, added in index order by a second launch, no
 * floating-point atomics, the decomposition a function of N alone; it agrees with the
 * sequential sum within N^2 * 2^-52 relative.  Synchronous.  The entry only reads the problem:
 * it keeps the carry, the speculation history and every statistic, like pgmg_monitor.  fp64 and
 * fp32 contexts.
 * Which order.  The field of a second-order solution is second order whatever the stencil, and
 * the second-order field of a fourth-order solution is second order too: order 4 only pays on
 * the result of pgmg_solve_extrap, where the field error falls by 16 per doubling of N and is
 * 2.5e3 to 4e4 times below the second-order pair's at N = 257 (tests/test_grad_cpu.py).  The
 * model is tests/grad_model.py.
 * PGMG_ERR_ARG, nothing enqueued and nothing written: a null context, an order other than 2 or 4,
 * a non-finite scale, both outputs NULL, an output that is not device memory, an output range
 * that overlaps the other output or phi.  PGMG_ERR_STATE, likewise: before pgmg_set_problem*;
 * world > 1 -- one GPU only, like pgmg_damp.
 * pgmg_gradient_time: `reps` passes (order 2 or 4, scale 1, both components and the norm: both
 * launches each) back to back between two hipEvents, after two warm ones, into two context-owned
 * output arrays allocated on the first call (16 N^2 bytes); mean device ms per pass and its
 * algorithmic bytes N^2 * (elem + 16), elem the bytes of a phi element as read (8, or 4 on the
 * grid of an fp32 context).  Leaves phi as it was. */
int pgmg_gradient(pgmg_ctx *ctx, int order, double scale, double *d_gx, double *d_gy, double *norm);
int pgmg_gradient_time(pgmg_ctx *ctx, int order, int reps, double *ms_per_pass, double *bytes);

/* ---- Projection ----------------------------------------------------------------------------
 * pgmg_project(ctx, opts, order, nu, omega, d_u, d_v, measure_after, info): the divergence-free
 * part of a velocity field (u*, v*) on the device, in place, without a host round trip:
 *     f = -div(u*, v*),   -lap(phi) = f with phi's frame as Dirichlet data (the problem every
 *     solve of the library solves),   (u, v) = (u*, v*) - grad(phi).
 * d_u and d_v are the caller's N x N device arrays of doubles at pitch N, element (j, i) at x =
 * i h, y = j h; h is the context's finest mesh width.  fp64, one GPU.  Synchronous.  The
 * expressions follow "Gradient of the solution" above: evaluated left to right as written, one
 * rounding per operation, no fused multiply-add; "the line formulas" are that section's g[k] of
 * order 2 and 4, one-sided points included, and w its factor (scale * 0.5 / h, or
 * scale / (12.0 * h)).
 *   The divergence, on all N x N points, frame included:
 *     dx(y, x) = the line formula along x on row y of u, times w
 *     dy(y, x) = the line formula along y on column x of v, times w
 *     out(y, x) = dx + dy            each of dx and dy rounded after its * w, then one add
 *   The update, on all N x N points, frame included:
 *     u(y, x) <- u(y, x) + gx(y, x),  v(y, x) <- v(y, x) + gy(y, x)
 *   gx, gy exactly pgmg_gradient's values for that phi, h, order and scale: one more rounding
 *   per component.  Each point reads and writes only its own u and v.
 * The steps:
 *   1. The stored level-0 right-hand side becomes the divergence of (u, v) at scale = -1.0,
 *      written by the pass straight into the context's f grid; info->div_before = sqrt(sum f^2)
 *      over all points from that pass's own sums (pgmg_gradient's scheme and decomposition).  The
 *      context's problem is then one with a caller's f: nothing is regenerated, PGMG_MON_ERROR is
 *      refused, the statistics and the speculation history start over and the carry is dropped --
 *      in every observable the state pgmg_set_problem(the current phi, that f downloaded)
 *      leaves.  phi is not touched: its frame is the Dirichlet data, its interior is ignored.
 *   2. order 2: pgmg_fmg_bc(ctx, nu, omega), then pgmg_solve_damped(ctx, opts, omega,
 *      &info->solve.fine).  order 4: pgmg_solve_extrap(ctx, opts, nu, omega, &info->solve).
 *   3. The update with phi where it lies, at scale = -1.0.
 *   4. measure_after != 0: info->div_after = the norm of step 1 on the corrected field, from a
 *      pass that stores nothing.
 * Afterwards phi is the potential, its frame bit for bit the one it had, and f stays the
 * divergence; a later pgmg_vcycle or pgmg_gradient continues from there.  The projection is
 * approximate: the div . grad of these stencils is not the 5-point Laplacian.  On (u*, v*) = w +
 * grad(psi), psi = sin(pi x) sin(pi y), w the divergence-free field of tests/test_proj_cpu.py,
 * solved with nu = 2, omega = 0.5, eps < 0, atol = 1e-10 ||f||, the relative error of (u, v)
 * against w falls from 2.1e-3 (N = 33) to 3.2e-5 (N = 257) at order 2, by 4 per doubling, and from
 * 9.0e-6 to 1.6e-9 at order 4, by 17 per doubling; ||div(u)|| / ||div(u*)|| is 8.6e-4 and 1.1e-7
 * at N = 257.  The model is tests/proj_model.py.
 * Errors, all before f or anything else is written.  PGMG_ERR_ARG: a null argument; invalid opts
 * (pgmg_solve's rule); an order other than 2 or 4; nu < 1; omega not finite, <= 0 or > 1 (the
 * undamped route stalls on a general f); u or v not device memory; u and v overlapping each other
 * or the context's grids; a coarsest level with fewer than 5 points per side; at order 4, N < 9
 * or a half-resolution grid whose coarsest level has fewer than 5.  PGMG_ERR_STATE: before
 * pgmg_set_problem; world > 1; an fp32 context; a device-bound problem (pgmg_set_problem_device:
 * its f is the caller's const array); PGMG_MON_ERROR in opts.
 * pgmg_project_time: `reps` passes back to back between two hipEvents, after two warm ones, on
 * three context-owned scratch arrays allocated on the first call (24 N^2 bytes): which = 0 the
 * divergence with out and norm (both launches), which = 1 the update of both components; mean
 * device ms per pass and its algorithmic bytes, 24 N^2 and 40 N^2.  Neither phi nor f is
 * written.  fp64, one GPU, after pgmg_set_problem*. */
typedef struct pgmg_project_info {
    pgmg_extrap_info solve;      /* order 4: as pgmg_solve_extrap fills it; order 2: .fine is the
                                    damped solve, every other field 0 */
    double div_before;           /* sqrt(sum f^2) over all points, from step 1's own pass */
    double div_after;            /* the same of the corrected field; NaN unless measure_after */
    double div_ms, update_ms;    /* device time of steps 1 and 3 */
    double elapsed_ms;           /* host wall time of the call */
} pgmg_project_info;
int pgmg_project(pgmg_ctx *ctx, const pgmg_solve_opts *o, int order, int nu, double omega,
                 double *d_u, double *d_v, int measure_after, pgmg_project_info *info);
int pgmg_project_time(pgmg_ctx *ctx, int which, int order, int reps, double *ms, double *bytes);

/* ---- Vorticity transport ---------------------------------------------------------------------
 * pgmg_vorticity_step(ctx, opts, omega, dt, nu, mode, walls, nsteps, info): 2D incompressible flow
 * in streamfunction-vorticity form, on the device, without a host round trip.  With u = psi_y,
 * v = -psi_x and w = v_x - u_y the flow obeys
 *     w_t + u w_x + v w_y = nu lap(w),      -lap(psi) = w,
 * and the second equation is exactly the problem every solve of the library solves: the
 * right-hand side f is the vorticity w and phi is the streamfunction psi, constant on solid walls
 * (a Dirichlet frame).  The velocity is divergence free by construction; no-slip walls and a
 * moving lid enter through the wall vorticity alone.  The state is the context's own problem:
 * start it with pgmg_set_problem(psi0, w0) (zeros: a cavity at rest).  fp64, one GPU.
 * Synchronous.  Element (j, i) is at x = i h, y = j h; h is the context's finest mesh width (a
 * negative h is used as written).  The expressions follow "Gradient of the solution" above:
 * evaluated left to right as written, one rounding per operation, no fused multiply-add.  P is
 * psi, W is w (not the solve's damping factor `omega`).
 *   The step, on the interior 1 <= y, x <= N - 2, with wgt = 0.5 / h and ih = 1.0 / (h * h):
 *     px  = (P[y][x+1] - P[y][x-1]) * wgt      py = (P[y+1][x] - P[y-1][x]) * wgt
 *     wx  = (W[y][x+1] - W[y][x-1]) * wgt      wy = (W[y+1][x] - W[y-1][x]) * wgt
 *     adv = py * wx - px * wy                            two products, one subtraction
 *     lap = (W[y][x-1] + W[y][x+1] + W[y-1][x] + W[y+1][x] - 4.0 * W[y][x]) * ih
 *     out[y][x] = W[y][x] + dt * (nu * lap - adv)        nu * lap, - adv, dt * (..), W + ..
 *   Every term comes from the P and W of before the pass.  The frame of out is the frame of W,
 *   word for word (a -0.0 stays -0.0).  The pass can also yield vmax = the maximum over the
 *   interior of |px| + |py|, NaN terms skipped as fmax skips them (per-workgroup maxima combined
 *   by a second launch; no atomics); cfl = dt * vmax / |h|.  16 B read and 8 B written per point.
 *   The wall pass, on the frame of W, with c = 2.0 * ih, d = 2.0 / h and the wall speeds walls[] =
 *   { ub, ut, vl, vr }: u on y = 0 and on y = (N-1) h, v on x = 0 and on x = (N-1) h (Thom's
 *   formula; psi's frame is read, not assumed 0):
 *     W[0][x]   = (P[0][x]   - P[1][x])   * c + ub * d      1 <= x <= N - 2
 *     W[N-1][x] = (P[N-1][x] - P[N-2][x]) * c - ut * d
 *     W[y][0]   = (P[y][0]   - P[y][1])   * c - vl * d      1 <= y <= N - 2
 *     W[y][N-1] = (P[y][N-1] - P[y][N-2]) * c + vr * d
 *     the four corners = +0.0                               (no interior stencil reads a corner)
 *   mode PGMG_WALL_FREE writes +0.0 on the whole frame instead (free slip; walls[] must still be
 *   finite).  Nothing in the solver reads f's frame.
 * Per step:
 *   1. The wall pass on f's frame, from the current phi.
 *   2. The step, f and phi read where they lie, into a scratch grid of f's shape (allocated on the
 *      first call) that is then copied onto f on the stream.  The context's problem is then one
 *      with a caller's f, in every observable the state pgmg_set_problem(the current phi, that f)
 *      leaves -- as after pgmg_project's step 1: the statistics and the speculation history start
 *      over and the carry is dropped.
 *   3. pgmg_solve_damped(ctx, opts, omega, &info->last), warm-started from the previous psi.  Its
 *      stop reason is reported, never acted on.  phi's frame is never written.
 * After the last step one more wall pass runs, so the returned f's frame belongs to the returned
 * phi, and the first wall pass of the next call reproduces it bit for bit: nsteps = 3 gives the
 * bits of three calls of one step.  A later pgmg_vcycle or pgmg_gradient continues from (phi, f);
 * the velocity is pgmg_gradient at order 2: u = gy at scale 1, v = gx at scale -1.
 * Stability is the caller's business: explicit Euler with central differences needs about
 * info->cfl <= 1 and info->diffusion = 4 nu dt / h^2 <= 1 (and a cell Reynolds number
 * |u| h / nu of at most about 2 for a monotone solution).  A non-finite cfl is no error.  The
 * scheme is first order in time and second order in space (orders 2 and 3 in time: "Runge-Kutta
 * vorticity transport" below).  The model is tests/vort_model.py.
 * Errors, all before anything is written.  PGMG_ERR_ARG: a null argument; invalid opts
 * (pgmg_solve's rule); PGMG_MON_ERROR in opts; omega not finite, <= 0 or > 1; dt not finite or
 * <= 0; nu not finite or < 0; a mode other than the two; a wall speed that is not finite; nsteps
 * < 1.  PGMG_ERR_STATE: before pgmg_set_problem; world > 1; an fp32 context; a device-bound
 * problem (pgmg_set_problem_device: its f is the caller's const array).
 * pgmg_vorticity_time: `reps` passes back to back between two hipEvents, after two warm ones, on
 * three context-owned scratch arrays allocated on the first call (24 N^2 bytes): which = 0 the
 * step with its copy back (40 N^2 bytes), which = 1 the step with vmax, both launches (24 N^2);
 * mean device ms per pass and those byte models.  Neither phi nor f is written.  fp64, one GPU,
 * after pgmg_set_problem*. */
#define PGMG_WALL_NOSLIP 0
#define PGMG_WALL_FREE 1
typedef struct pgmg_vort_info {
    int steps;                    /* steps taken */
    long long cycles, sweeps;     /* summed over the steps' solves */
    pgmg_solve_info last;         /* the last step's damped solve */
    int worst_reason;             /* the largest final residual norm of any step's solve (a NaN */
    double worst_res;             /* counts as the largest), and that solve's stop reason */
    double cfl, diffusion;        /* last step: dt * vmax / |h|;  4 * nu * dt / (h * h) */
    double step_ms, solve_ms;     /* summed: device time of the wall and step passes with the copy;
                                     the solves' elapsed_ms */
    double elapsed_ms;            /* host wall time of the call */
} pgmg_vort_info;
int pgmg_vorticity_step(pgmg_ctx *ctx, const pgmg_solve_opts *o, double omega, double dt, double nu,
                        int mode, const double walls[4], int nsteps, pgmg_vort_info *info);
int pgmg_vorticity_time(pgmg_ctx *ctx, int which, int reps, double *ms_per_pass, double *bytes);

/* ---- Runge-Kutta vorticity transport -----------------------------------------------------------
 * pgmg_vorticity_step_rk(ctx, opts, omega, dt, nu, mode, walls, order, nsteps, info): the flow of
 * "Vorticity transport" above advanced by a strong-stability-preserving Runge-Kutta scheme of
 * order 1, 2 or 3 in time (Shu and Osher's form: every stage is a convex combination of the
 * vorticity the step started from and one explicit Euler step).  Every convention is that
 * section's: the state is the context's problem (phi = psi, f = w), fp64, one GPU, synchronous,
 * expressions evaluated left to right as written, one rounding per operation, no fused
 * multiply-add.
 *   E(P, W) is that section's step with the dt and nu of the call: W[y][x] + dt * (nu * lap - adv)
 *   on the interior and W's frame on the frame -- word for word pgmg_vorticity_grid's output.
 *   A stage with the coefficients (a, b) and the saved field W0, with e = E(P, W)[y][x]:
 *     out[y][x] = a * W0[y][x] + b * e          1 <= y, x <= N - 2: a * W0, b * e, their sum
 *     out's frame = W's frame, word for word    (a -0.0 stays -0.0); W0's frame is never read
 *   24 B read and 8 B written per point; vmax is "Vorticity transport"'s, of P.
 *   The stages by order.  Stage 1 is always plain E (the pass of pgmg_vorticity_step itself, not
 *   the combination with (0, 1)); K3 is the double nearest 1/3 (0x3FD5555555555555) and B3 the
 *   double nearest 2/3 (0x3FE5555555555555):
 *     order 1   E
 *     order 2   E; (0.5, 0.5)                   Heun's method in Shu-Osher form
 *     order 3   E; (0.75, 0.25); (K3, B3)       Shu and Osher's third-order scheme
 * Per step, for stage k = 1 .. order:
 *   1. The wall pass of "Vorticity transport" on f's frame, from the current phi (mode, walls).
 *   2. k = 1 only: W0 := f, the whole grid as the wall pass left it (a context-owned grid of f's
 *      shape, allocated on the first call with order > 1, freed by pgmg_destroy).
 *   3. The stage -- E for k = 1, the combination of f and W0 otherwise --, f and phi read where
 *      they lie, into pgmg_vorticity_step's scratch grid, which is then copied onto f on the
 *      stream.  The context's problem is then one with a caller's f, exactly as step 2 of
 *      pgmg_vorticity_step leaves it.
 *   4. pgmg_solve_damped(ctx, opts, omega, &info->last), warm-started from the current phi.
 * After the last step one more wall pass runs.  So a step costs `order` solves; order 1 is bit
 * for bit pgmg_vorticity_step (phi, f and every field of info but the times); and nsteps = 3 gives
 * the bits of three calls of one step.  info keeps its layout: steps counts steps; cycles and
 * sweeps sum over all stage solves; last is the last stage's solve; worst_res and worst_reason
 * range over all stage solves; cfl comes from the vmax of the last step's last stage; diffusion
 * is 4 nu dt / h^2; step_ms sums the wall passes, the stages and the copies.
 * Stability is still the caller's business, but the orders differ in kind.  For w' = lambda w a
 * step multiplies w by R(z), z = lambda dt: R = 1 + z, 1 + z + z^2/2, 1 + z + z^2/2 + z^3/6.
 * Central advection has imaginary eigenvalues: of the frozen-velocity operator u d_x + v d_y they
 * are bounded by (|u| + |v|) / |h|, so |z| <= info->cfl.  On the imaginary axis |R(i s)|^2 is
 * 1 + s^2 (order 1), 1 + s^4 / 4 (order 2: Heun shares Euler's defect) and 1 - s^4 / 12 +
 * s^6 / 36 (order 3), which is <= 1 exactly for s <= sqrt(3).  The 5-point diffusion has real
 * eigenvalues in [-8 nu / h^2, 0], so z >= -2 * info->diffusion, and order 3's |R| <= 1 on the
 * real axis down to z = -2.51.  So order 3 holds for cfl <= sqrt(3) = 1.73 and diffusion <= 1.25,
 * each limit taken alone (a step near both at once is outside the region), whatever the
 * viscosity, nu = 0 included; orders 1 and 2 amplify every advective mode and need the viscosity
 * to damp it (about cfl <= 1, diffusion <= 1 and a cell Reynolds number of at most about 2, as
 * above).  The scheme is second order in space.  The model is tests/vort_rk_model.py.
 * Errors, all before anything is written: everything pgmg_vorticity_step refuses, with its
 * codes; an order outside 1 .. 3: PGMG_ERR_ARG.
 * pgmg_vorticity_rk_time: pgmg_vorticity_time's measurement of the stage pass on four
 * context-owned scratch arrays allocated on the first call (32 N^2 bytes): which = 0 the stage
 * with its copy back (48 N^2 bytes), which = 1 the stage with vmax, both launches (32 N^2).
 * Neither phi nor f is written. */
int pgmg_vorticity_step_rk(pgmg_ctx *ctx, const pgmg_solve_opts *o, double omega, double dt,
                           double nu, int mode, const double walls[4], int order, int nsteps,
                           pgmg_vort_info *info);
int pgmg_vorticity_rk_time(pgmg_ctx *ctx, int which, int reps, double *ms_per_pass, double *bytes);

/* ---- Buoyancy-driven flow ---------------------------------------------------------------------
 * pgmg_boussinesq_step(ctx, opts, omega, p, d_T, nsteps, info): the flow of "Vorticity transport"
 * above carrying a scalar T (a temperature) that feeds back into the vorticity equation, the
 * Boussinesq approximation:
 *     w_t + u w_x + v w_y = nu lap(w) + (by T_x - bx T_y)
 *     T_t + u T_x + v T_y = kappa lap(T)
 *     -lap(psi) = w,    u = psi_y,    v = -psi_x
 * (gravity along -y: bx = 0, by = g beta).  The state (psi, w) is the context's problem (phi, f),
 * as for pgmg_vorticity_step; d_T is the caller's device array, N x N doubles at pitch N, updated
 * in place.  Every convention is that section's: fp64, one GPU, context-owned problems,
 * synchronous; element (j, i) at x = i h, y = j h; h the context's finest mesh width (a negative h
 * is used as written); expressions evaluated left to right as written, one rounding per
 * operation, no fused multiply-add.  P is psi, W is w.
 *   The step, on the interior 1 <= y, x <= N - 2, with wgt = 0.5 / h and ih = 1.0 / (h * h); px,
 *   py, wx, wy and lapw are "Vorticity transport"'s px, py, wx, wy and lap:
 *     tx   = (T[y][x+1] - T[y][x-1]) * wgt        ty = (T[y+1][x] - T[y-1][x]) * wgt
 *     advw = py * wx - px * wy                     advt = py * tx - px * ty
 *     lapt = (T[y][x-1] + T[y][x+1] + T[y-1][x] + T[y+1][x] - 4.0 * T[y][x]) * ih
 *     src  = by * tx - bx * ty                     two products, one subtraction
 *     Wout[y][x] = W[y][x] + dt * ((nu * lapw - advw) + src)
 *     Tout[y][x] = T[y][x] + dt * (kappa * lapt - advt)
 *   Every term comes from the P, W and T of before the pass, which is one launch: 24 B read and
 *   16 B written per point.  The frame of Wout is W's frame and the frame of Tout is T's, word for
 *   word (a -0.0 stays -0.0; Dirichlet temperatures are simply never written).  vmax is
 *   "Vorticity transport"'s.  So Tout is bit for bit that section's step of T under P with kappa
 *   for nu, and with bx = by = 0 and finite inputs Wout equals its step of W as numbers (the
 *   added +0.0 can change the sign of a zero and nothing else).
 *   The scalar wall pass, on the frame of T: each bit of `adiabatic` makes its wall adiabatic by
 *   the second-order one-sided dT/dn = 0, written so that a constant field is kept exactly; K3 is
 *   the double nearest 1/3 (0x3FD5555555555555; a product, not a division):
 *     PGMG_TWALL_BOTTOM  T[0][x]   = T[1][x]   + (T[1][x]   - T[2][x])   * K3      1 <= x <= N - 2
 *     PGMG_TWALL_TOP     T[N-1][x] = T[N-2][x] + (T[N-2][x] - T[N-3][x]) * K3
 *     PGMG_TWALL_LEFT    T[y][0]   = T[y][1]   + (T[y][1]   - T[y][2])   * K3      1 <= y <= N - 2
 *     PGMG_TWALL_RIGHT   T[y][N-1] = T[y][N-2] + (T[y][N-2] - T[y][N-3]) * K3
 *   A wall whose bit is clear is Dirichlet and is not touched; the four corners are never written
 *   (no interior stencil reads them); mask 0 writes nothing.  Every value read is an interior
 *   value, so the four walls do not depend on each other.
 * Per step:
 *   1. The wall passes: "Vorticity transport"'s on f's frame from the current phi (p->mode,
 *      p->walls), and the scalar wall pass on d_T's frame.
 *   2. The step, phi, f and d_T read where they lie, into two scratch grids (f's for w, as
 *      pgmg_vorticity_step's; a context-owned N x N grid for T, allocated on the first call) that
 *      are then copied on the stream onto f and onto d_T.  The context's problem is then one with
 *      a caller's f, exactly as step 2 of pgmg_vorticity_step leaves it.
 *   3. pgmg_solve_damped(ctx, opts, omega, &info->flow.last), warm-started from the previous psi.
 * After the last step both wall passes run once more: nsteps = 3 gives the bits of three calls of
 * one step.  info->flow is filled as pgmg_vorticity_step fills its info (cfl from the last step's
 * vmax, diffusion = 4 nu dt / h^2); diffusion_t = 4 kappa dt / h^2.  Stability is the caller's
 * business: cfl, diffusion and diffusion_t at most about 1.  The scheme is first order in time
 * and second order in space (orders 2 and 3 in time: "Runge-Kutta buoyancy-driven flow" below).
 * The model is tests/bouss_model.py.
 * Errors, all before anything is written.  PGMG_ERR_ARG: everything pgmg_vorticity_step refuses
 * (dt, nu, mode and walls read from p); a null p or d_T; a d_T that is not device memory; kappa
 * not finite or < 0; a buoy component that is not finite; an adiabatic bit above 8.
 * PGMG_ERR_STATE: before pgmg_set_problem; world > 1; an fp32 context; a device-bound problem.
 * pgmg_boussinesq_time: pgmg_vorticity_time's measurement on five context-owned scratch arrays
 * allocated on the first call (40 N^2 bytes): which = 0 the step with both copies back (72 N^2
 * bytes), which = 1 the step with vmax, both launches (40 N^2).  Neither phi, f nor any caller
 * array is written. */
#define PGMG_TWALL_BOTTOM 1u
#define PGMG_TWALL_TOP 2u
#define PGMG_TWALL_LEFT 4u
#define PGMG_TWALL_RIGHT 8u
typedef struct pgmg_bouss_params {
    double dt, nu, kappa;
    double buoy[2];        /* bx, by: w_t += by T_x - bx T_y (gravity along -y: bx = 0, by = g beta) */
    int mode;              /* PGMG_WALL_NOSLIP | PGMG_WALL_FREE */
    double walls[4];       /* ub, ut, vl, vr as in pgmg_vorticity_step */
    unsigned adiabatic;    /* PGMG_TWALL_* */
} pgmg_bouss_params;
typedef struct pgmg_bouss_info {
    pgmg_vort_info flow;   /* as pgmg_vorticity_step fills it */
    double diffusion_t;    /* 4 * kappa * dt / (h * h) */
} pgmg_bouss_info;
int pgmg_boussinesq_step(pgmg_ctx *ctx, const pgmg_solve_opts *o, double omega,
                         const pgmg_bouss_params *p, double *d_T, int nsteps, pgmg_bouss_info *info);
int pgmg_boussinesq_time(pgmg_ctx *ctx, int which, int reps, double *ms_per_pass, double *bytes);

/* ---- Runge-Kutta buoyancy-driven flow -----------------------------------------------------------
 * pgmg_boussinesq_step_rk(ctx, opts, omega, p, d_T, order, nsteps, info): the flow of
 * "Buoyancy-driven flow" above advanced by the strong-stability-preserving Runge-Kutta schemes of
 * "Runge-Kutta vorticity transport", order 1, 2 or 3 in time.  Every convention is that of those
 * two sections: the state is the context's problem (phi = psi, f = w) and the caller's d_T, fp64,
 * one GPU, synchronous, expressions evaluated left to right as written, one rounding per
 * operation, no fused multiply-add.
 *   EW(P, W, T) and ET(P, W, T) are "Buoyancy-driven flow"'s Wout and Tout with the dt, nu, kappa
 *   and buoy of the call -- word for word pgmg_boussinesq_grid's outputs.
 *   A stage with the coefficients (a, b) and the saved fields W0 and T0, with ew = EW[y][x] and
 *   et = ET[y][x]:
 *     wout[y][x] = a * W0[y][x] + b * ew        1 <= y, x <= N - 2: a * W0, b * ew, their sum
 *     tout[y][x] = a * T0[y][x] + b * et        the same; one (a, b) serves both fields
 *     wout's frame = W's frame, tout's frame = T's frame, word for word (a -0.0 stays -0.0); the
 *     frames of W0 and T0 are never read
 *   40 B read and 16 B written per point; vmax is "Vorticity transport"'s, of P.
 *   The stages by order are "Runge-Kutta vorticity transport"'s: stage 1 is always the plain Euler
 *   pass (pgmg_boussinesq_step's own, not the combination with (0, 1)); order 2 adds (0.5, 0.5);
 *   order 3 adds (0.75, 0.25) and (K3, B3), K3 = 0x3FD5555555555555, B3 = 0x3FE5555555555555.
 * Per step, for stage k = 1 .. order:
 *   1. Both wall passes: "Vorticity transport"'s on f's frame from the current phi, and the
 *      scalar wall pass on d_T's frame.
 *   2. k = 1 only: W0 := f and T0 := d_T, the whole grids as the wall passes left them (W0 is
 *      pgmg_vorticity_step_rk's grid; T0 is a context-owned dense N x N grid, allocated on the
 *      first call with order > 1, freed by pgmg_destroy).
 *   3. The stage -- the Euler pass for k = 1, the combination otherwise --, phi, f and d_T read
 *      where they lie, into pgmg_boussinesq_step's two scratch grids, which are then copied on the
 *      stream onto f and onto d_T: d_T holds stage values during the call and the new temperature
 *      after it.  The context's problem is then one with a caller's f.
 *   4. pgmg_solve_damped(ctx, opts, omega, &info->flow.last), warm-started from the current phi.
 * After the last step both wall passes run once more.  So a step costs `order` solves; order 1 is
 * bit for bit pgmg_boussinesq_step (phi, f, T and every field of info but the times); and nsteps
 * = 3 gives the bits of three calls of one step.  info->flow is filled as pgmg_vorticity_step_rk
 * fills its info (steps counts steps; the sums and worst_* range over all stage solves; cfl comes
 * from the vmax of the last step's last stage); diffusion_t = 4 kappa dt / h^2.
 * Stability.  Beside the advective and diffusive eigenvalues of "Runge-Kutta vorticity transport"
 * the coupling w_t = by T_x, T_t = -v T_y is an oscillator (internal gravity waves): in a stable
 * stratification T_y = G a mode of wavenumbers (kx, ky) has the frequency n = sqrt(by G) kx /
 * |k| <= sqrt(by G), purely imaginary eigenvalues whatever nu and kappa are.  With s = n dt, a
 * step multiplies the mode by |R(i s)|^2 = 1 + s^2 at order 1 -- unstable for every s > 0 that the
 * diffusion does not reach --, by 1 + s^4 / 4 at order 2, a slow growth that a little diffusion
 * pays for, and by 1 - s^4 / 12 + s^6 / 36 <= 1 at order 3 for s <= sqrt(3).  So order 3 covers
 * buoyancy oscillations and advection up to cfl-like numbers of sqrt(3) = 1.73 and diffusion
 * numbers of 1.25 (each limit taken alone); order 1 needs cfl, diffusion and diffusion_t of at
 * most about 1 and enough diffusion to damp both.  The scheme is second order in space.  The
 * model is tests/bouss_rk_model.py.
 * Errors, all before anything is written: everything pgmg_boussinesq_step refuses, with its
 * codes; an order outside 1 .. 3: PGMG_ERR_ARG.
 * pgmg_boussinesq_rk_time: pgmg_boussinesq_time's measurement of the stage pass on seven
 * context-owned scratch arrays allocated on the first call (56 N^2 bytes): which = 0 the stage
 * with both copies back (88 N^2 bytes), which = 1 the stage with vmax, both launches (56 N^2);
 * which = 2 and 3 are 0 and 1 with the pass's other built depth of loads in flight (DESIGN.md §4j;
 * the entries never launch it).  Neither phi, f nor any caller array is written. */
int pgmg_boussinesq_step_rk(pgmg_ctx *ctx, const pgmg_solve_opts *o, double omega,
                            const pgmg_bouss_params *p, double *d_T, int order, int nsteps,
                            pgmg_bouss_info *info);
int pgmg_boussinesq_rk_time(pgmg_ctx *ctx, int which, int reps, double *ms_per_pass, double *bytes);

/* ---- Mixed-precision refinement ----------------------------------------------------------
 * pgmg_solve_mixed(ctx, opts, nu, omega, info): fp64 solutions from fp32 multigrid corrections
 * (defect correction).  The iterate phi and its residual stay in fp64 on the fp64 context ctx,
 * which runs no cycle at all; an fp32 context it owns solves every correction equation at the
 * fp32 rate.  fp64 context, one GPU.  Synchronous.
 *   The child.  Owned by ctx, created on the first call, destroyed by pgmg_destroy: pgmg_create on
 *   a copy of ctx's config -- the same N and h0 -- with precision = PGMG_PRECISION_FP32, eps =
 *   -1.0, world 1 and PGMG_FLAG_FAST cleared, everything else equal.  Its early exits are
 *   absolute thresholds on a scaled problem, so they are off; with them off the fp32 solve is
 *   exactly homogeneous in a power-of-two factor on f (short of overflow and underflow).
 *   The two passes, with s a power of two, t = 1 / s, ih = 1.0 / (h * h), evaluated left to right
 *   as written, one rounding per operation, no fused multiply-add:
 *     defect    r = f - ih (4x - x_l - x_r - x_u - x_d)   pgmg_monitor's r, in double, on every
 *               g(y, x) = (float)(r * s)                  interior point: one double product, then
 *                                                         IEEE round-to-nearest-even to fp32
 *                                                         (overflow to Inf, gradual underflow,
 *                                                         nothing flushed)
 *               g = +0.0f on the frame; sqrt(sum r^2) of the unscaled r by the monitor's
 *               decomposition and reduction: bit for bit pgmg_monitor(PGMG_MON_RESIDUAL)'s norm
 *               of that state.  x and f are read where they lie (the level-0 grids, or the
 *               caller's bound arrays), g is written elsewhere.  Bytes N^2 (8 + 8 + 4).
 *     correct   x(y, x) <- x(y, x) + ((double)e(y, x) * t)     1 <= y, x <= N - 2; the frame of x
 *               is never written (a -0.0 there stays -0.0).  Bytes N^2 (4 + 8 + 8).
 *   The loop.  opts is pgmg_solve's: max_cycles caps the refinement steps, check_every must be 1,
 *   cycle PGMG_CYCLE_V, monitor PGMG_MON_RESIDUAL.  rho_0 = pgmg_monitor's residual norm of the
 *   starting phi (one extra pass per call), rho_i = r_{i-1} for i >= 1.  At check i = 0, 1, ..:
 *     a. s_i = 2^(-ilogb(rho_i / (N - 2))), the exponent clamped to [-1022, 1022]; 1.0 when the
 *        quotient is 0 or not finite.  The defect pass writes g_i into the child's level-0 f grid
 *        and yields r_i (r_0 is bit for bit rho_0).
 *     b. pgmg_solve's rule decides on r_i, in its order: non-finite, converged, stalled,
 *        max_cycles.  On a stop nothing more is written: unlike pgmg_solve_damped, phi is exactly
 *        the iterate info.solve.res was measured on.
 *     c. The child's problem becomes (phi' = 0, f' = g_i): in every observable the state
 *        pgmg_set_problem(child, zeros, g_i) leaves, a problem with a caller's f and reset
 *        statistics.  Then pgmg_fmg_damped(child, nu, omega), asynchronous: nothing waits inside a
 *        step but the norm of (a).  The child's sweeps are added to info.inner_sweeps.
 *     d. The correction on phi where it lies, e = the child's phi, t = 1 / s_i.
 *   pgmg_history holds the checks, cycle[] the steps taken before each.  info.solve.cycles is the
 *   number of steps applied.  The fp64 residual norm falls by a factor that depends on nu alone,
 *   not on N or f, down to fp64's floor (tests/mixed_model.py on the CPU oracle, nu = 2, omega =
 *   0.5, N = 33 .. 257: 400 .. 3100 per step; the step that arrives at the floor gains what is
 *   left of it; nu = 3: 4500 .. 18000; nu = 1: 25 .. 56).
 * The entry changes phi: it drops the carry and resets the speculation history.  ctx's own sweep
 * and early-exit statistics are untouched (it runs no cycle); ctx's eps does not matter.  phi's
 * frame and f are bit for bit what they were.  A later pgmg_vcycle, pgmg_gradient or
 * pgmg_solve_extrap continues from the result.  Problems set with pgmg_set_problem (the analytic
 * f as stored, or a caller's f) and with pgmg_set_problem_device alike; a device-bound problem's
 * arrays are read and written where they lie, the stream ordered after the caller's as
 * pgmg_solve_extrap's is.
 * What to ask for.  State the target as atol: the floor of the fp64 residual is ||r|| ~ 0.4 N^2
 * 2^-52 ||f||, and rtol is relative to whatever phi the call started from.
 * Errors, all before anything is enqueued or created.  PGMG_ERR_ARG: a null argument; invalid opts
 * (pgmg_solve's rule); check_every != 1; a cycle other than PGMG_CYCLE_V; PGMG_MON_ERROR (call
 * pgmg_monitor afterwards); nu < 1; omega not finite, <= 0 or > 1; a coarsest level of fewer than
 * 5 points per side.  PGMG_ERR_STATE: before pgmg_set_problem*; world > 1; an fp32 context.
 * pgmg_mixed_time: `reps` passes back to back between two hipEvents, after two warm ones, between
 * ctx's phi and f and the child's grids (created if need be): which = 0 the defect pass with its
 * reduction (s = 1, g into the child's f grid), which = 1 the correction (e = the child's phi,
 * t = 1); mean device ms per pass and the byte models above.  Leaves phi changed, like
 * pgmg_damp_time. */
typedef struct pgmg_mixed_info {
    pgmg_solve_info solve;        /* cycles = refinement steps applied, checks, reason, res0, res */
    long long inner_sweeps;       /* the fp32 context's pgmg_stats sweeps, summed over the steps */
    double defect_ms, inner_ms, correct_ms;   /* device time, summed over the steps */
    double elapsed_ms;            /* host wall time of the call */
} pgmg_mixed_info;
int pgmg_solve_mixed(pgmg_ctx *ctx, const pgmg_solve_opts *o, int nu, double omega,
                     pgmg_mixed_info *info);
int pgmg_mixed_time(pgmg_ctx *ctx, int which, int reps, double *ms_per_pass, double *bytes);

/* Cumulative smoother sweeps and early exits since set_problem.  The sweeps are the
 * oracle's.  The early exits are those that cut a smoother call short: the check after a
 * call's last sweep cannot change the result and is not evaluated, so where the oracle's
 * early_exits also counts such a check firing (its last_exits), this counter does not. */
int pgmg_stats(pgmg_ctx *ctx, long long *sweeps, long long *early_exits);

/* [0] sweeps, [1] early exits, [2] k_postpre post-check rare paths taken (-1 when
 * cross-cycle fusion is off), [3] k_postpre pre-check rare paths taken. */
int pgmg_stats_detail(pgmg_ctx *ctx, long long *out4);

/* Device time of the last pgmg_vcycle/wcycle call in ms (hipEvents on the
 * context stream; synchronous). */
int pgmg_last_elapsed_ms(pgmg_ctx *ctx, double *ms);

/* Number of bulk (multi-kernel) levels and the tail's top N. */
int pgmg_levels(pgmg_ctx *ctx, int *bulk_levels, int *tail_top_n);

/* Algorithmic HBM bytes one V-cycle moves (per rank), summed per kernel. */
int pgmg_vcycle_bytes(pgmg_ctx *ctx, double *bytes);

/* Raw device pointer and pitch (in elements) of phi's element (0,0) on this
 * rank, for callers that want to read it in place.  The elements are double, or
 * float when the context was created with PGMG_PRECISION_FP32 (pgmg_precision). */
int pgmg_phi_device(pgmg_ctx *ctx, double **ptr, int *pitch, int *row0, int *rows);

/* Is rows [row0, row1] x columns [col0, col1] (inclusive, elements of elem_bytes, row pitch
 * `pitch` elements, relative to element (0,0) at `origin`) inside ONE device allocation of
 * this library (a level grid)?  PGMG_OK if so, PGMG_ERR_STATE otherwise.  The fused passes
 * run this check on every array before each launch (they read halo rows past their bands
 * and margin columns past their tiles); callers reading a grid in place through
 * pgmg_phi_device can use it too. */
int pgmg_check_span(const void *origin, long long pitch, int elem_bytes, long long row0,
                    long long row1, long long col0, long long col1);

/* Algorithmic HBM bytes of one launch of finest-level pass `pass` (numbering of
 * pgmg_fine_pass_time) on this rank: every input read once, every output written once
 * (24 B per fine point for x, f -> x; +8 B per coarse point per coarse array; 16 B when
 * k_postpre regenerates the analytic f in-kernel), times elem_bytes / 8. */
int pgmg_fine_pass_bytes(pgmg_ctx *ctx, int pass, double *bytes);

/* Whether V/W-cycle calls decide the smoother early-exit checks speculatively (1: the
 * checks are recorded, validated once after the call, and the call is rolled back and
 * rerun with in-stream decisions when one could fire; cross-fused or row-strip contexts
 * without PGMG_FLAG_EXACT_DIST) or in-stream (0), and how many calls (V, W or F) were rolled
 * back.  After a rollback the context decides in-stream until the next pgmg_set_problem. */
int pgmg_dist_info(pgmg_ctx *ctx, int *speculative, long long *rollbacks);

/* Which bulk levels decide their early-exit checks in-stream in the next speculative call:
 * bit l (l >= 1) = level l's checks fired or are predicted to fire soon; bit 0 = no
 * speculation at all (disabled, or a finest-level check fires). */
int pgmg_spec_levels(pgmg_ctx *ctx, unsigned long long *in_stream);
/* Of those, the levels whose checks are predicted to FIRE in the next speculative call (one
 * GPU; converged levels: each visit runs the one-sweep passes the in-stream rare paths would
 * run, and the validation confirms every such check fired, else the call is rolled back). */
int pgmg_spec_fire_levels(pgmg_ctx *ctx, unsigned long long *fire);
/* W-cycle plans (one GPU): how the last speculative W call enqueued the visits of its bulk
 * levels -- counts[0] recorded "does not fire", counts[1] predicted to fire, counts[2] decided
 * in-stream -- each visit planned from the same visit of the previous cycle.  Zeros after a
 * V call. */
int pgmg_spec_visit_modes(pgmg_ctx *ctx, long long counts[3]);

/* Row strips (world > 1): the collective groups enqueued since the last call and, with
 * PGMG_FLAG_TIME_COMM, the stream time spent inside them in ms (-1 without the flag; the
 * transfer plus any wait for a peer, i.e. the part of a rank's cycle not spent computing);
 * synchronous, resets both.  One GPU: 0 and 0. */
int pgmg_comm_stats(pgmg_ctx *ctx, long long *groups, double *ms);
/* The communicator's rank count (RCCL: ncclCommCount; the world for the loopback / host /
 * null transports; 1 without strips). */
int pgmg_comm_ranks(pgmg_ctx *ctx, int *ranks);

/* The carry (above pgmg_vcycle): out[0] calls that started from a carried pre-smooth, out[1]
 * carries made, out[2] carries dropped because their check could fire. */
int pgmg_carry_info(pgmg_ctx *ctx, long long out[3]);

/* Sampled checks.  On a speculative call (one GPU) the finest level's cross-cycle pass sums
 * its two early-exit checks over 1 row in 6 (1 in 4 with a caller's f and in the pass that
 * takes a carry): a lower bound of the full sum, which the validation needs only to show that
 * the check cannot fire.  A sampled check that could fire rolls the call back like any other and
 * the rerun decides from full sums; if no cross-cycle check fires then, the context keeps
 * speculating but its finest passes sum every row from then on, until pgmg_set_problem* or
 * pgmg_set_eps.  out[0]: finest passes launched in the sampled form; out[1]: rollbacks caused
 * only by sampled checks after which no such check fired; out[2]: 1 while the context is in that
 * full-sum mode.  PGMG_FLAG_FULL_CHECKS never samples.  Read-only. */
int pgmg_spec_sampled_info(pgmg_ctx *ctx, long long out[3]);

/* A new early-exit threshold (JacobiSmoother's eps, Smoother.hpp:38) for the following calls:
 * drops the carry and the speculation history (the statistics continue). */
int pgmg_set_eps(pgmg_ctx *ctx, double eps);

/* The context's PGMG_PRECISION_* and its grid element size in bytes (8 or 4). */
int pgmg_precision(pgmg_ctx *ctx, int *precision, int *elem_bytes);

/* Count and mean device duration (ms) of the finest-level kernels launched since
 * the last call (needs PGMG_FLAG_TIME_FINE; synchronous).  pass 0: plain Jacobi
 * sweep (unfused path), 1: fused pre-smooth+residual+restriction (k_pre),
 * 2: fused prolongation+post-smooth (k_post), 3: cross-cycle k_postpre, 4: the carry pass
 * (k_postpre that stores the call's result instead of the next pre-smooth), 5: the recompute
 * form (the first k_postpre of a call that took the carry). */
int pgmg_fine_pass_time(pgmg_ctx *ctx, int pass, int *count, double *mean_ms);
/* What the launches the last pgmg_fine_pass_time(pass) averaged were: the kernel symbol of the
 * last of them (demangled, e.g. "pgmg::k_postpre_lds<double, false, true, 2>"; "" when none was
 * timed) and the mean of their algorithmic bytes (the pgmg_fine_pass_bytes model applied to
 * what each launch actually read and wrote: an F-cycle's k_pre reads no x0, ...). */
int pgmg_fine_pass_info(pgmg_ctx *ctx, int pass, char *symbol, int len, double *bytes_per_launch);
int pgmg_fine_sweep_time(pgmg_ctx *ctx, int *count, double *mean_ms);  /* pass 0 */

/* 1 when the context runs the fused two-pass-per-level cycle (v1 = v2 = 1). */
int pgmg_fused(pgmg_ctx *ctx, int *fused);

/* Time `reps` back-to-back fine-grid Jacobi sweeps (the roofline kernel) on the
 * context's level-0 buffers with hipEvents; returns the mean per sweep in ms.
 * Leaves phi changed (call set_problem again before parity checks). */
int pgmg_bench_sweep(pgmg_ctx *ctx, int reps, double *ms_per_sweep);

/* ---- op level (device pointers, reference layout, pitch = W) ------------- */
/* v+1 sweeps on d_x IN PLACE (Parallel::ComputeJacobi, Parallel_Method.cu:144-160; each
 * sweep is exactly the out-of-place Jacobi sweep: tile-edge outputs another workgroup reads
 * are deferred and scattered after each pass).  eps < 0 disables the early exit.  d_tmp: W*H
 * scratch or NULL (allocated internally), used only by checked calls (eps >= 0) with v >= 1.
 * *sweeps_done (may be NULL) receives the sweep count (synchronous when non-NULL; NULL keeps
 * the call asynchronous on `stream`). */
int pgmg_jacobi(double *d_x, double *d_tmp, const double *d_f, int H, int W, double h, int v,
                double eps, int *sweeps_done, void *stream);
int pgmg_residual(double *d_r, const double *d_x, const double *d_f, int H, int W, double h,
                  void *stream);
int pgmg_restrict(const double *d_fine, double *d_coarse, int Nf, int Nc, void *stream);
int pgmg_prolong(const double *d_coarse, double *d_fine, int Nc, int Nf, int mode, void *stream);
/* The same with the reference's thread grid (Parallel::ComputeProlungator,
 * Parallel_Method.cu:188-199): only fine rows and columns below max(1, Nf / num_thread) *
 * num_thread are touched -- for Nf = 2^k + 1 > num_thread the last fine row and column keep
 * their values, as in the reference.  num_thread = 0: the whole grid (pgmg_prolong). */
int pgmg_prolong_grid(const double *d_coarse, double *d_fine, int Nc, int Nf, int mode,
                      int num_thread, void *stream);
int pgmg_norm(const double *d_v, long long n, double *result, void *stream);
int pgmg_rhs(double *d_f, int W, int H, double h, double a, double p, double q, void *stream);
/* One damping pass (pgmg_damp's formula, above) on caller-owned N x N device arrays, pitch N,
 * fp64:  x <- x + w * r,  r = f - ih (4x - x_l - x_r - x_u - x_d),  ih = 1.0 / (h * h),
 * w = omega * 0.25 * (h * h), on every interior point; out-of-place semantics (every r from the x
 * of before the pass), two roundings, the boundary never written.  It is the launch the damped
 * FMG runs on every level of its pyramid, so N = 2^k + 1 with k >= 2, and h is the level's
 * (h_0 * 2^l on level l).  res_norm != NULL: the residual norm of x BEFORE the update, bit for
 * bit what pgmg_monitor(PGMG_MON_RESIDUAL) returns for that state on a context of that N and h
 * (the decomposition is a function of N alone); the call is then synchronous.  res_norm == NULL:
 * asynchronous on `stream`.  Another N, omega not finite or outside (0, 1], h not finite or
 * <= 0, a null x or f: PGMG_ERR_ARG, nothing enqueued.  Its scratch (the deferred edges, the
 * partial sums) belongs to the per-stream set below. */
int pgmg_damp_grid(double *d_x, const double *d_f, int N, double h, double omega, double *res_norm,
                   void *stream);
/* The extrapolation of pgmg_solve_extrap (step 5 above) on caller-owned device arrays, fp64:
 * d_fine Nf x Nf, pitch Nf, updated in place on its interior (its frame is never written);
 * d_coarse Nc x Nc, Nc = (Nf + 1) / 2, pitch Nc, only read.  fine <- fine + C((fine(2j, 2i) -
 * coarse) * K3), every difference taken from the fine of before the call.  Asynchronous on
 * `stream`; the coarse-sized scratch grid belongs to the per-stream set below.  Nf not 2^k + 1
 * with k >= 3, or a null pointer: PGMG_ERR_ARG, nothing enqueued. */
int pgmg_extrap_grid(double *d_fine, const double *d_coarse, int Nf, void *stream);
/* pgmg_gradient (above) on caller-owned device arrays, fp64: d_phi N x N at pitch N, only read;
 * d_gx, d_gy N x N doubles at pitch N, either may be NULL.  N = 2^k + 1 with k >= 2; h finite and
 * not 0 (negative is legal).  norm == NULL: asynchronous on `stream`; otherwise synchronous, and
 * *norm is bit for bit pgmg_gradient's on a context of that N and h (the decomposition is a
 * function of N alone); the partial sums belong to the per-stream set below.  Another N, h of 0
 * or not finite, an order other than 2 or 4, a non-finite scale, a null phi, both outputs NULL,
 * an output that is not device memory or that overlaps the other output or phi: PGMG_ERR_ARG,
 * nothing enqueued. */
int pgmg_gradient_grid(const double *d_phi, double *d_gx, double *d_gy, int N, double h, int order,
                       double scale, double *norm, void *stream);
/* The divergence of pgmg_project ("Projection" above) on caller-owned device arrays, fp64:
 * out = dx(u) + dy(v) on all N x N points, d_u, d_v and d_out at pitch N, u and v only read.
 * d_out may be NULL when norm is not: the pass then stores nothing, reads 16 B per point and only
 * sums.  norm receives sqrt(sum out^2) over all points, by pgmg_gradient's scheme on its
 * decomposition (a function of N alone); the partial sums belong to the per-stream set below.
 * norm == NULL: asynchronous on `stream`; otherwise synchronous.  N not 2^k + 1 with k >= 2, h of
 * 0 or not finite (negative is legal), an order other than 2 or 4, a non-finite scale, a null u
 * or v, both out and norm NULL, an out that is not device memory or that overlaps u or v:
 * PGMG_ERR_ARG, nothing enqueued. */
int pgmg_divergence_grid(const double *d_u, const double *d_v, double *d_out, int N, double h,
                         int order, double scale, double *norm, void *stream);
/* The update of pgmg_project on caller-owned device arrays, fp64: u <- u + gx, v <- v + gy on all
 * N x N points, gx and gy exactly pgmg_gradient_grid's values for that phi, h, order and scale.
 * d_u and d_v at pitch N, either may be NULL (both: PGMG_ERR_ARG); d_phi at pitch_phi >= N, only
 * read.  Each point reads and writes only its own u and v: safe in place.  Asynchronous on
 * `stream`.  The other argument rules are pgmg_gradient_grid's; u, v and phi must not overlap one
 * another. */
int pgmg_gradient_add_grid(const double *d_phi, long long pitch_phi, double *d_u, double *d_v,
                           int N, double h, int order, double scale, void *stream);
/* The two passes of pgmg_vorticity_step ("Vorticity transport" above) on caller-owned device
 * arrays of doubles at pitch N, N = 2^k + 1 with k >= 2.
 * pgmg_vorticity_grid: d_out = the step of d_w under d_psi on the interior, d_w's frame on the
 * frame; d_psi and d_w are only read, d_out must not overlap either.  vmax == NULL: asynchronous
 * on `stream`; otherwise synchronous, *vmax = the maximum of |px| + |py| over the interior (its
 * per-workgroup partials belong to the per-stream set below).
 * pgmg_wall_vorticity_grid: the wall pass in place on d_w's frame, from d_psi (only read; the two
 * must not overlap); mode PGMG_WALL_NOSLIP or PGMG_WALL_FREE, walls = { ub, ut, vl, vr }.
 * Asynchronous on `stream`.
 * Another N, h of 0 or not finite (negative is legal), dt not finite or <= 0, nu not finite or
 * < 0, another mode, a wall speed that is not finite, a null pointer, an output that is not device
 * memory, overlapping arrays: PGMG_ERR_ARG, nothing enqueued. */
int pgmg_vorticity_grid(const double *d_psi, const double *d_w, double *d_out, int N, double h,
                        double dt, double nu, double *vmax, void *stream);
int pgmg_wall_vorticity_grid(const double *d_psi, double *d_w, int N, double h, int mode,
                             const double walls[4], void *stream);
/* The stage pass of pgmg_vorticity_step_rk ("Runge-Kutta vorticity transport" above) on
 * caller-owned device arrays of doubles at pitch N, under pgmg_vorticity_grid's contract: d_out =
 * a * d_w0 + b * E(d_psi, d_w) on the interior, d_w's frame on the frame.  d_psi, d_w and d_w0 are
 * only read; d_w0 may be d_w (or overlap it); d_out must overlap none of the three.  vmax as in
 * pgmg_vorticity_grid.  pgmg_vorticity_grid's argument errors, an a or b that is not finite, a
 * null d_w0: PGMG_ERR_ARG, nothing enqueued. */
int pgmg_vorticity_stage_grid(const double *d_psi, const double *d_w, const double *d_w0,
                              double *d_out, int N, double h, double dt, double nu, double a,
                              double b, double *vmax, void *stream);
/* The two passes of pgmg_boussinesq_step ("Buoyancy-driven flow" above) on caller-owned device
 * arrays of doubles at pitch N, N = 2^k + 1 with k >= 2, under the contract of the two entries
 * above.
 * pgmg_boussinesq_grid: d_wout and d_Tout = the steps of d_w and d_T under d_psi on the interior,
 * their frames on the frame; d_psi, d_w and d_T are only read; an output must not overlap an
 * input or the other output.  vmax == NULL: asynchronous on `stream`; otherwise synchronous.
 * pgmg_wall_scalar_grid: the scalar wall pass in place on d_T's frame; adiabatic = a mask of
 * PGMG_TWALL_*.  Asynchronous on `stream`.
 * The argument errors of the two entries above, kappa not finite or < 0, a null or non-finite
 * buoy, an adiabatic bit above 8: PGMG_ERR_ARG, nothing enqueued. */
int pgmg_boussinesq_grid(const double *d_psi, const double *d_w, const double *d_T, double *d_wout,
                         double *d_Tout, int N, double h, double dt, double nu, double kappa,
                         const double buoy[2], double *vmax, void *stream);
int pgmg_wall_scalar_grid(double *d_T, int N, unsigned adiabatic, void *stream);
/* The stage pass of pgmg_boussinesq_step_rk ("Runge-Kutta buoyancy-driven flow" above) on
 * caller-owned device arrays of doubles at pitch N, under pgmg_boussinesq_grid's contract: d_wout
 * = a * d_w0 + b * EW and d_Tout = a * d_T0 + b * ET on the interior, d_w's and d_T's frames on the
 * frames.  The five inputs are only read; d_w0 may be d_w and d_T0 may be d_T (or overlap them);
 * an output must not overlap an input or the other output.  vmax == NULL: asynchronous on
 * `stream`; otherwise synchronous.  pgmg_boussinesq_grid's argument errors, an a or b that is not
 * finite, a null d_w0 or d_T0: PGMG_ERR_ARG, nothing enqueued. */
int pgmg_boussinesq_stage_grid(const double *d_psi, const double *d_w, const double *d_T,
                               const double *d_w0, const double *d_T0, double *d_wout, double *d_Tout,
                               int N, double h, double dt, double nu, double kappa,
                               const double buoy[2], double a, double b, double *vmax, void *stream);
/* The two passes of pgmg_solve_mixed ("Mixed-precision refinement" above) on caller-owned device
 * arrays at pitch N, N = 2^k + 1 with k >= 2: x and f fp64, g and e fp32.
 * pgmg_defect_grid: g = (float)(r * scale) on the interior, +0.0f on the frame, r the fp64 residual
 * of (x, f) at mesh width h; x and f are only read.  res_norm == NULL: asynchronous on `stream`;
 * otherwise synchronous, and *res_norm is bit for bit pgmg_monitor(PGMG_MON_RESIDUAL)'s on a
 * context of that N and h holding x and f; its partial sums belong to the per-stream set below.
 * pgmg_correct_grid: x <- x + ((double)e * scale) on the interior (the caller passes 1 / s); the
 * frame of x is never written.  Asynchronous on `stream`.
 * Another N, h of 0 or not finite (negative is legal), a scale that is not finite or is <= 0, a
 * null pointer, a g that is not device memory or that overlaps x or f, an e that overlaps x:
 * PGMG_ERR_ARG, nothing enqueued. */
int pgmg_defect_grid(const double *d_x, const double *d_f, float *d_g, int N, double h, double scale,
                     double *res_norm, void *stream);
int pgmg_correct_grid(double *d_x, const float *d_e, int N, double scale, void *stream);
/* The op-level entries keep one scratch set (partial sums, flags, ping-pong buffer) per
 * stream they were called on; this waits for `stream` and frees its set (a later op on the
 * same stream allocates a fresh one).  Call it before destroying a stream the ops used. */
int pgmg_ops_release(void *stream);

/* ---- Batched small problems ------------------------------------------------------------------
 * Every entry above solves one problem per context, and the host steers each solve: at N <= 65 a
 * cycle is one launch of one workgroup, and a solve waits for a residual norm before every chunk of
 * cycles.  The batch entries run B independent problems of the same size N <= 65 in ONE launch,
 * one workgroup per problem: workgroup b loads problem b into LDS, cycles it there with the code of
 * the contexts' one-workgroup tail, in pgmg_batch_solve decides convergence by itself, and stores
 * phi.  No context, no host round trip inside the launch, nothing shared between the problems.
 *
 * Arrays.  d_phi and d_f are device arrays of B * N * N elements, problem b at element b * N * N
 * in the reference layout (pitch N): double for PGMG_PRECISION_FP64, float for _FP32 (unlike a
 * context's ABI, an fp32 batch reads and writes floats).  phi is updated in place, frame included
 * (the frame is the problem's Dirichlet data and is stored back bit for bit); f is only read.
 * Asynchronous on `stream` (a hipStream_t; NULL: the default stream), like the op-level entries.
 *
 * pgmg_batch_cycle: `ncycles` V-cycles (PGMG_CYCLE_V) or W-cycles with cfg->alpha visits
 * (PGMG_CYCLE_W) of every problem: bit for bit what pgmg_vcycle / pgmg_wcycle do to that problem on
 * a context of the same N, v1, v2, coarse_iter, n_coarse, alpha, eps, precision and h0 = h.
 * d_sweeps / d_exits (each may be NULL): B words, the problem's own sweeps and early exits, what
 * pgmg_stats counts for it.
 *
 * pgmg_batch_solve: per problem, pgmg_solve_damped's loop and stop rule (above: "Convergence
 * monitor and solve-to-tolerance", "Damping pass and damped solve") restated on the device.  At
 * check i, after k_i cycles:
 *   1. r_i = sqrt(sum over the interior of r^2), r = f - ih (4x - x_l - x_r - x_u - x_d) in the
 *      element type (pgmg_monitor's expression), squared and summed in double in a fixed order
 *      (a thread's points in index order, then lanes, then waves).  The bits are a function of
 *      (phi, f, N, h) alone: not of B, of the problem's index or of where the workgroup ran.  Only
 *      the summation order differs from the sequential sum: within N^2 2^-52 relative of it.
 *   2. omega > 0: x <- x + w r on the interior, w = (T)(omega * 0.25 * (h * h)), every r from the
 *      x of before the update, two roundings, no fused multiply-add, the frame never written:
 *      pgmg_damp's formula.  omega == 0: nothing is written, the loop is plain pgmg_solve's.
 *   3. pgmg_solve's rule in its order: r_i not finite -> PGMG_STOP_NONFINITE; r_i <= max(atol,
 *      rtol * r_0) -> _CONVERGED; the stall streak -> _STALLED; k_i >= max_cycles -> _MAX_CYCLES.
 *   4. otherwise min(check_every, max_cycles - k_i) cycles of opts->cycle, and the next check.
 * As in pgmg_solve_damped the stopping check's correction is applied.  Problems stop
 * independently; a problem whose data holds a NaN ends with PGMG_STOP_NONFINITE at check 0 and
 * touches nothing of its neighbours.  Tolerances are shared by the batch (state atol in the units
 * of the f's at hand).  opts->monitor is ignored apart from the PGMG_MON_ERROR refusal below.
 * out (may be NULL, as may any of its arrays): device arrays of B entries written by the launch --
 * cycles, checks, reason, res0 (r_0), res (the last r_i), sweeps, exits; history: B x history_cap
 * norms, check 0 first, slots past the problem's last check (and checks past history_cap: not
 * recorded) NaN.  Read them after the stream has finished.
 *
 * pgmg_batch_time (measurement): B problems of pseudo-random right-hand sides in arrays of its
 * own, `reps` launches of pgmg_batch_cycle(cycle, ncycles) back to back on the default stream
 * between two hipEvents after two warm ones; mean device ms per launch.  Synchronous.
 *
 * Sizes.  N = 65 in fp64 takes 122 KiB of a CU's 160 KiB of LDS, and at every N the kernel's
 * registers allow one workgroup per CU: a batch runs min(B, CUs) problems at a time and its time
 * grows in steps of that many problems.
 *
 * PGMG_ERR_ARG, before any HIP call: a null cfg, opts, phi or f; B < 1 (or above 2^31 - 1); N
 * other than 5, 9, 17, 33, 65; v1, v2, coarse_iter, n_coarse, alpha outside pgmg_create's bounds;
 * h zero or not finite (negative is legal); an unknown precision; omega not finite or outside
 * [0, 1]; options pgmg_solve refuses; PGMG_CYCLE_F (it rebuilds the analytic f); PGMG_MON_ERROR;
 * ncycles < 0; history_cap < 0.  The model is tests/batch_model.py. */
typedef struct pgmg_batch_config {
    int N;                      /* 5, 9, 17, 33 or 65 */
    int v1, v2, coarse_iter, n_coarse, alpha;   /* pgmg_config's meaning, defaults and bounds */
    double eps;                 /* smoother early exit; < 0: never */
    double h;                   /* mesh width, finite and not 0; default 1 / (N - 1) */
    int precision;              /* PGMG_PRECISION_FP64: double arrays; _FP32: float arrays */
} pgmg_batch_config;
int pgmg_batch_config_default(pgmg_batch_config *cfg, int N);

typedef struct pgmg_batch_out {         /* device arrays of B entries each; any may be NULL */
    int *cycles, *checks, *reason;      /* PGMG_STOP_* */
    double *res0, *res;
    long long *sweeps, *exits;          /* what pgmg_stats counts, per problem */
    double *history; int history_cap;   /* B x history_cap norms, check 0 first; unused slots NaN */
} pgmg_batch_out;

int pgmg_batch_cycle(const pgmg_batch_config *cfg, int cycle /* PGMG_CYCLE_V | _W */, int ncycles,
                     void *d_phi, const void *d_f, long long B,
                     long long *d_sweeps, long long *d_exits, void *stream);
int pgmg_batch_solve(const pgmg_batch_config *cfg, const pgmg_solve_opts *o, double omega,
                     void *d_phi, const void *d_f, long long B,
                     const pgmg_batch_out *out, void *stream);
int pgmg_batch_time(const pgmg_batch_config *cfg, int cycle, int ncycles, long long B, int reps,
                    double *ms_per_launch);   /* own scratch arrays, two warm launches, hipEvents */

/* ---- device memory helpers (for host code built without HIP headers) ----- */
int pgmg_device_alloc(void **ptr, size_t bytes);
int pgmg_device_free(void *ptr);
int pgmg_memcpy_h2d(void *dst, const void *src, size_t bytes);
int pgmg_memcpy_d2h(void *dst, const void *src, size_t bytes);
int pgmg_device_sync(void);
int pgmg_device_count(int *n);

/* RCCL bootstrap: fill a 128-byte buffer with a fresh ncclUniqueId (rank 0). */
int pgmg_comm_unique_id(void *out128);

/* Self-test of the RCCL transport on one GPU (a world-1 communicator): the strip path's
 * grouped send/recv, allreduce(sum, double) and allreduce(min, u32) on a stream; 0 = ok. */
int pgmg_rccl_selftest(const void *uid128, int device);
/* Latency floor of the strips' collectives on THIS device: a world-1 RCCL communicator
 * (unique id uid128) times, over `reps` repetitions after 3 warm ones with hipEvents on one
 * stream, us[0] one grouped send + recv of 2 rows of 16385 doubles to itself (the finest
 * level's halo at N = 16385), us[1] an allreduce(sum) of 3 doubles (k_postpre's decision),
 * us[2] an allreduce(min) of 9 u32 (the speculation marks); mean microseconds per call.  A
 * lower bound of the per-group cost between ranks (no xGMI hop, no peer to wait for). */
int pgmg_rccl_latency(const void *uid128, int device, int reps, double *us3);

/* Measurement (libpgmg_ab.so, built with -DPGMG_TUNING; the product library always
 * returns -1): with PGMG_TAIL_PROF=1 in the environment, the LDS tail accumulates shader-
 * clock cycles per stage kind ([0] wave-team hand-offs, [1] block smooth, [2] block
 * res+restrict, [3] block prolong, [4] whole kernel, [5] launches, [6] wave smooth, [7] wave
 * res+restrict+prolong); read (and reset) them.  -1 when the variable is unset. */
int pgmg_tail_prof(unsigned long long *out16, int reset);

/* In-process rank hub for PGMG_FLAG_LOOPBACK (tests of the strip decomposition). */
int pgmg_loopback_create(int world, void **hub);
int pgmg_loopback_destroy(void *hub);
/* Test hook: the at_group-th transport group (halo exchange, gather) rank `rank` starts
 * from now on fails with PGMG_ERR_COMM (0 = never). */
int pgmg_loopback_fail(void *hub, int rank, long long at_group);

/* Host-only strip plan: the finest-level rows [lo, hi) rank `rank` owns and the
 * number of strip-distributed levels (0: too small to split, replicas). */
int pgmg_plan_strips(int N, int world, int rank, int tail_n, int gather_n, int *lo, int *hi,
                     int *dist_levels);

const char *pgmg_last_error(void);
const char *pgmg_version(void);
/* First 16 hex digits of the sha256 of the sources this library was built from (the csrc .hip
 * and .h files, include/pgmg.h, concatenated in path order; Makefile "srchash"). */
const char *pgmg_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* PGMG_H */
