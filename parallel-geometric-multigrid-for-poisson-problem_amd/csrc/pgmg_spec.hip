// pgmg_spec.hip — "speculative calls": a call's early-exit checks recorded instead of decided
// in-stream and validated once after it (pinned reply, reply_wait), the per-level policy with
// "predicted to fire", segment planning, run_cycles_spec, the read-only queries.  Host code and
// the validation's three small kernels (k_verify_checks, k_spec_reply, k_spec_open).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pgmg_check.h"
#include "pgmg_host.h"

using namespace pgmg;

// ---------------------------------------------------------------------------
// Speculative calls.  Every smoother's early-exit check (MultiGrid.hpp via Smoother.hpp:
// 75-88, ||r(x1)|| < eps after the first of the two sweeps) needs a grid-wide sum, so the
// exact path follows each fused pass with a fix-up launch that reduces the pass's per-
// block partials, decides, and recomputes the reference result when the check fired
// (plus, at level 0 between cycles, a decision kernel and four conditional rare-path
// launches): ~22 launches per V-cycle of a few microseconds each that almost never do
// work.  A speculative call instead enqueues all its cycles with every check decided
// "does not fire": each pass writes its partials into a fresh slice of a per-call log and
// no fix-up is launched.  After the call one kernel re-reduces every recorded check
// exactly as the fix-ups would and flags those that could fire; on row strips a rank's
// partial is a lower bound of the all-rank sum (a sum of non-negative doubles never
// rounds below one of its terms, sqrt is monotonic), so one allreduce(min) of the flags
// finds the checks no rank could rule out.  If any check could fire, the call is rolled
// back (the level-0 solution -- untouched: the cross-fused cycles rotate through the
// scratch buffer S instead of writing A -- buffer roles and statistics restored) and run
// again with in-stream decisions, and the context stops speculating (a fired check means
// the solver is near convergence, where checks keep firing).  Results and statistics
// are therefore always the exact path's.  The call ends with one host synchronisation.
//
// Sampled checks (one GPU).  The finest level's cross-cycle pass spends a quarter of its
// arithmetic on the residuals of its two checks, whose only use on a speculative call is this
// proof that they cannot fire.  A sum over a subset of the rows proves it as well, by the
// strips' argument: the sampled partial adds a subsequence of the full partial's non-negative
// terms in the same order, every later reduction is the same tree over inputs that are no
// larger, and rounding and sqrt are monotonic -- so sqrt(sampled sum) <= sqrt(full sum), and
// could_fire = sqrt(s) < eps (1 + 1e-12) on the sampled sum stays a superset of "the full sum
// fires" (a NaN term in an unsampled row makes the full sum NaN, which does not fire either).
// Such a check is logged as a lower bound (CheckRef::bound) and may only be recorded "does not
// fire"; must_fire proves nothing from a bound.  A sampled check that could fire rolls the
// segment back as any other; the rerun launches the full-sum form and decides in-stream.  If a
// cross-cycle check then fires, the context stops speculating as before; if none does, the
// finest norm sits between eps and about sqrt(6) eps (1 row in 6 sampled): the context keeps
// speculating with full-sum finest passes (SpecHistory::full_sums) until the next problem or
// eps.  The level-0 norms of the reply (hnorm, lvl_hist[0]) are lower bounds then; nothing
// predicts from them (spec_mark_levels, spec_level_trend's callers and spec_plan_segment all
// start at level 1).  PGMG_FLAG_FULL_CHECKS launches the full-sum form everywhere.
// ---------------------------------------------------------------------------

namespace pgmg {

// Validation of a speculative call: one workgroup per recorded check re-reduces its
// partials with the sum every in-stream decision takes (partials_sum, pgmg_check.h: 256
// threads, strided, then the block sum) and flags the checks that could fire.  The 1e-12
// margin makes the flag a superset of "fires" whatever order the exact path sums in (an
// all-rank sum of row strips goes through launch_sum_partials + allreduce: relative
// differences below ~4e-13 for the <= 3072 non-negative terms of one rank).
// out[i] = 1 when check i's prediction may be wrong; norm[i] = sqrt(sum of its partials)
__global__ __launch_bounds__(256) void k_verify_checks(const CheckRef *checks, double eps,
                                                       unsigned *out, double *norm)
{
    __shared__ double red[4];
    const CheckRef c = checks[blockIdx.x];
    const double s = partials_sum(c.partials, c.np, red);
    if (threadIdx.x == 0) {
        // flag = the prediction may be wrong: "does not fire" checks that could fire, "fires"
        // checks that could not (same margin the other way); in-stream checks are logged
        // for the norms only
        // a lower bound (c.bound, sampled checks): could_fire is a superset of "the full sum
        // fires" all the same; must_fire would prove nothing, so any other record is flagged
        const bool could_fire = sqrt(s) < eps * (1.0 + 1e-12);
        const bool must_fire = sqrt(s) < eps * (1.0 - 1e-12);
        out[blockIdx.x] = c.expect == 0 ? (could_fire ? 1u : 0u)
                                        : (c.bound ? 1u : (c.expect == 1 ? (must_fire ? 0u : 1u) : 0u));
        norm[blockIdx.x] = sqrt(s);
    }
}

static void launch_verify_checks(const CheckRef *checks, int n, double eps, unsigned *out,
                                 double *norm, hipStream_t s)
{
    if (n > 0) k_verify_checks<<<dim3(n), dim3(256), 0, s>>>(checks, eps, out, norm);
}

// The validation's reply (after the all-rank MIN): any = 1 when one of the first n_any checks
// could fire on every rank, then every check's norm and verdict, each stored straight into
// the context's pinned host staging -- the call then waits for the stream once, with no copy
// operations between the kernels and the wait.
__global__ __launch_bounds__(256) void k_spec_reply(const unsigned *f, const double *norm, int n,
                                                    int n_any, unsigned *h_any, double *h_norm,
                                                    unsigned *h_flags, unsigned *h_seq, unsigned seq)
{
    __shared__ unsigned any;
    if (threadIdx.x == 0) any = 0u;
    __syncthreads();
    unsigned v = 0u;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const unsigned fk = f[k];
        if (k < n_any) v |= fk;
        h_flags[k] = fk;
        h_norm[k] = norm[k];
    }
    if (v) atomicOr(&any, 1u);
    __syncthreads();
    if (threadIdx.x == 0) *h_any = any;
    // every store above reaches the host before the sequence word (the host polls it)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// any = OR over the first n_any verdicts, and the n norms and verdicts themselves, straight
// into pinned host memory; then *h_seq = seq (system scope, after the rest)
static void launch_spec_reply(const unsigned *flags, const double *norm, int n, int n_any,
                              unsigned *h_any, double *h_norm, unsigned *h_flags, unsigned *h_seq,
                              unsigned seq, hipStream_t s)
{
    k_spec_reply<<<dim3(1), dim3(256), 0, s>>>(flags, norm, n, n_any, h_any, h_norm, h_flags, h_seq,
                                                seq);
}

// a speculative segment's opening: stats_bk = stats (4 words), flags[0, nflags) = 0
__global__ __launch_bounds__(256) void k_spec_open(const unsigned long long *stats,
                                                   unsigned long long *stats_bk, unsigned *flags,
                                                   int nflags)
{
    if (threadIdx.x < 4) stats_bk[threadIdx.x] = stats[threadIdx.x];
    for (int k = threadIdx.x; k < nflags; k += blockDim.x) flags[k] = 0u;
}

void launch_spec_open(const unsigned long long *stats, unsigned long long *stats_bk, unsigned *flags,
                      int nflags, hipStream_t s)
{
    k_spec_open<<<dim3(1), dim3(256), 0, s>>>(stats, stats_bk, flags, nflags);
}

}  // namespace pgmg

void pgmg::spec_need_level(pgmg_ctx *c, int l, int gamma, long long *dbl, long long *nchk)
{
    *dbl = 0;
    *nchk = 0;
    if (l >= c->nb) return;
    const Level &L = c->lv[l];
    // the small levels' tile passes (pgmg_coarse.hip) may write more partials than the
    // row-marching passes: reserve for the larger
    const int np = std::max(fused_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2),
                            tile_np(c, l, false));
    const PostRows pr = post_rows(c, l);
    const int npo = std::max(fused_blocks(L.N, pr.jc0, pr.jc1), tile_np(c, l, true));
    long long d, k;
    spec_need_level(c, l + 1, gamma, &d, &k);
    *dbl = (long long)np + npo + gamma * d;
    *nchk = 2 + gamma * k;
}

// the pinned validation staging (pgmg_ctx::pin) for cap checks: CheckRefs, norms, verdicts + any
static size_t pin_norm_off(long long cap) { return ((size_t)cap * sizeof(CheckRef) + 15) / 16 * 16; }
static size_t pin_flag_off(long long cap) { return pin_norm_off(cap) + (size_t)cap * sizeof(double); }
static size_t pin_seq_off(long long cap) { return pin_flag_off(cap) + ((size_t)cap + 1) * sizeof(unsigned); }
static size_t pin_bytes(long long cap) { return pin_seq_off(cap) + 64; }

// The validation's wait: poll the reply's sequence word in pinned memory (the call's
// critical path: a blocking stream wait wakes the host late -- tens of us on a busy host --
// and the next call's kernels queue behind that), asking the runtime every ~20 us whether the
// stream failed or drained.  Once the word arrives the call returns without a stream wait:
// everything the host reads next is in the pinned reply, and everything it writes next (the
// staging's CheckRefs) was read by k_verify_checks, which ran before the reply.  A fault
// surfaces at the runtime's query; a wait past 50 ms (a slow segment, a shared GPU) stops
// burning the core and blocks.  One GPU only (row strips wait through their transport).
static int reply_wait(pgmg_ctx *c, const unsigned *hseq, unsigned seq)
{
    if (c->comm == nullptr && !(c->cfg.flags & PGMG_FLAG_NO_SPIN)) {
        const auto t0 = std::chrono::steady_clock::now();
        auto next = t0 + std::chrono::microseconds(20);
        for (;;) {
            if (__atomic_load_n(hseq, __ATOMIC_ACQUIRE) == seq) return PGMG_OK;
            const auto now = std::chrono::steady_clock::now();
            if (now < next) continue;
            next = now + std::chrono::microseconds(20);
            const hipError_t q = hipStreamQuery(c->s);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) PGMG_HIPC(q);
            if (now - t0 > std::chrono::milliseconds(50)) break;
        }
    }
    return stream_wait(c);
}

int pgmg::spec_reserve(pgmg_ctx *c, long long dbl, long long nchk)
{
    if (dbl > c->plog_cap || nchk > c->chk_cap) {
        PGMG_TRY(stream_wait(c));
        if (dbl > c->plog_cap) {
            if (c->plog) HIPC(hipFree(c->plog));
            c->plog = nullptr;
            HIPC(hipMalloc((void **)&c->plog, dbl * sizeof(double)));
            c->plog_cap = dbl;
        }
        if (nchk > c->chk_cap) {
            if (c->uflags) HIPC(hipFree(c->uflags));
            if (c->chk_norm) HIPC(hipFree(c->chk_norm));
            c->uflags = nullptr;
            c->chk_norm = nullptr;
            HIPC(hipMalloc((void **)&c->uflags, (nchk + 1) * sizeof(unsigned)));
            HIPC(hipMalloc((void **)&c->chk_norm, nchk * sizeof(double)));
            if (c->pin) HIPC(hipHostFree(c->pin));
            c->pin = nullptr;
            HIPC(hipHostMalloc((void **)&c->pin, pin_bytes(nchk), hipHostMallocCoherent));
            // (a fresh staging area: its sequence word must not already hold the next seq)
            std::memset(c->pin, 0, pin_bytes(nchk));
            c->pin_seq = 0;
            c->chk_cap = nchk;
        }
    }
    if (!c->stats_bk) HIPC(hipMalloc((void **)&c->stats_bk, 4 * sizeof(unsigned long long)));
    if (c->comm && !c->mark_dev) HIPC(hipMalloc((void **)&c->mark_dev, (c->nb + 1) * sizeof(unsigned)));
    return PGMG_OK;
}

// last norm and decay of level l's checks (spec_mark_levels' prediction); false without history
static bool spec_level_trend(const pgmg_ctx *c, int l, double *last, double *rho)
{
    const std::vector<double> &h = c->hist.lvl_hist[l];
    const size_t m = h.size();
    if (m < 2) return false;
    *last = std::min(h[m - 1], h[m - 2]);
    *rho = 0.4;
    if (m >= 4) {
        const double prev = std::min(h[m - 3], h[m - 4]);
        if (prev > 0.0) *rho = std::min(*rho, std::max(1e-3, *last / prev));
    }
    return true;
}

// Per-level policy.  Residual norms of a level fall geometrically over the V-cycles (after
// a few cycles of growth from phi = 0) until they level off, and on the reference problem
// the levels just above the tail reach eps after ~27 cycles at every N >= 2049
// (scripts/spec_fire_probe.py, spec_trace.py: 0.32-0.35 per cycle in the steady phase).
// A rollback costs a whole segment, so a coarse level whose checks are predicted to fire
// within the next segment -- last norm x rho^cycles < 100 eps with rho = min(0.4, its
// measured decay) -- or did fire decides in-stream from then on (its two fix-ups per visit
// come back); the others keep speculating.  The finest
// level is not predicted (its norm levels off far above eps at these sizes: round-off of
// 1/h^2-scaled sums); if one of its checks does fire the context stops speculating.
// Row strips: each rank predicts from its own partials (a lower bound of the global norm,
// so earlier), then the ranks agree on the union of the marks (one allreduce).
//
// Predicted to fire (one GPU): a level whose last two visits' checks all had norms below
// eps / 4 -- it converged and fires at every check -- is enqueued with its checks decided
// "fires" (k_pre1 / k_post1: the one-sweep passes the in-stream rare paths would run, one
// launch each instead of two) and recorded the other way round: the validation flags a
// check that could NOT fire (sqrt(s) >= eps (1 - 1e-12)), the call is rolled back, and the
// level decides in-stream for the rest of the problem.  A level in that mode whose norm
// comes back above eps / 4 returns to in-stream decisions.
static int spec_mark_levels(pgmg_ctx *c, int cycles)
{
    const double lim = c->cfg.eps * 100.0;
    if (c->comm == nullptr && !(c->cfg.flags & PGMG_FLAG_NO_SPEC_FIRE) && c->call.spec_gamma == 1) {
        const double flim = c->cfg.eps * 0.25;
        for (int l = 1; l < c->nb; ++l) {
            const std::vector<double> &h = c->hist.lvl_hist[l];
            const size_t m = h.size();
            const size_t need = c->hist.lvl_fire[l] ? 2 : 4;
            bool below = !c->hist.lvl_fire_block[l] && m >= need;
            for (size_t i = m - std::min(m, need); i < m && below; ++i) below = h[i] < flim;
            c->hist.lvl_fire[l] = below ? 1 : 0;
            if (below) c->hist.lvl_exact[l] = 0;
            else if (m >= 2 && h[m - 1] < c->cfg.eps) c->hist.lvl_exact[l] = 1;   // fired: in-stream
        }
    }
    if (tuning_int("PGMG_SPEC_TRACE", 0))
        for (int l = 1; l < c->nb; ++l) {
            fprintf(stderr, "spec level %d N=%d exact %d fire %d block %d hist/eps", l, c->lv[l].N,
                    (int)c->hist.lvl_exact[l], (int)c->hist.lvl_fire[l], (int)c->hist.lvl_fire_block[l]);
            for (double v : c->hist.lvl_hist[l]) fprintf(stderr, " %.3g", v / c->cfg.eps);
            fprintf(stderr, "\n");
        }
    // keep[l]: the segment's first cycles in which level l records "does not fire" (its
    // predicted norm last * rho^k stays at or above 100 eps); 0: in-stream from the start
    std::vector<unsigned> keep(c->nb + 1, (unsigned)cycles);
    for (int l = 1; l < c->nb && c->call.spec_gamma == 1; ++l) {
        double last, rho;   // min over the last visit; decay per cycle
        if (c->hist.lvl_exact[l] || c->hist.lvl_fire[l] || !spec_level_trend(c, l, &last, &rho)) continue;
        const double k = last >= lim ? std::floor(std::log(lim / last) / std::log(rho)) : 0.0;
        keep[l] = (unsigned)std::max(0.0, std::min((double)cycles, k));
        // (PGMG_FLAG_NO_SPEC_FIRE, the r02 policy: in-stream for the whole segment instead)
        if ((c->cfg.flags & PGMG_FLAG_NO_SPEC_FIRE) && keep[l] < (unsigned)cycles) keep[l] = 0u;
        if (tuning_int("PGMG_SPEC_TRACE", 0))
            fprintf(stderr, "spec level %d N=%d last %.3e rho %.3f: speculates %u of %d cycles\n", l,
                    c->lv[l].N, last, rho, keep[l], cycles);
    }
    if (c->comm) {
        HIPC(hipMemcpyAsync(c->mark_dev, keep.data(), (c->nb + 1) * sizeof(unsigned),
                            hipMemcpyHostToDevice, c->s));
        int e = c->comm->allreduce_min_u32(c->mark_dev, c->nb + 1, c->s);
        if (e) return e;
        HIPC(hipMemcpyAsync(keep.data(), c->mark_dev, (c->nb + 1) * sizeof(unsigned),
                            hipMemcpyDeviceToHost, c->s));
        PGMG_TRY(stream_wait(c));
    }
    for (int l = 1; l < c->nb; ++l) {
        if (!keep[l]) c->hist.lvl_exact[l] = 1;
        c->hist.lvl_kx[l] = (int)keep[l];
    }
    return PGMG_OK;
}

// Segment planning (one GPU).  A level that decides in-stream (two launches of ~5 us per
// visit) can be predicted to fire -- one launch per visit -- only from the norms of a
// validated segment, so a long call (the 3 + 40 cycles of BASELINE configs[1] at N = 4097:
// the coarse levels cross eps at ~27 cycles) would keep it in-stream to its end.  The segment
// ends where such levels can be predicted to fire when that pays for the split: ~10 us per
// level and cycle saved against one more finest-level pass (the cross-fused call restarts:
// k_post + k_pre instead of one k_postpre, 16 B per fine point at ~5 TB/s) and one host
// round trip of the validation.  (A speculating level's crossing of 100 eps needs no split:
// spec_mark_levels gives it its speculating cycles within the segment.)
static int spec_plan_segment(pgmg_ctx *c, int seg)
{
    if (seg < 4 || (c->cfg.flags & PGMG_FLAG_NO_SPEC_FIRE) || c->call.spec_gamma > 1) return seg;
    // a new problem: a short first segment gathers every level's trend (without one, a long
    // first call speculated blind and rolled back at the first firing check, ~27 cycles in
    // on the reference problem); history sizes are the same on every rank
    if (seg > 8)
        for (int l = 1; l < c->nb; ++l)
            if (c->hist.lvl_hist[l].size() < 2 && !c->hist.lvl_exact[l]) return 3;
    if (c->comm != nullptr) return seg;   // (strips: every rank must agree)
    const double lim = c->cfg.eps * 100.0, flim = c->cfg.eps * 0.25;
    // cycles until last * rho^k falls below t; kNever where it never does: a norm of Inf (r^2
    // overflowed), t = 0 (eps = 0) or a decay that is NaN (Inf / Inf) give a quotient of Inf
    // or NaN, which must not reach the cast (undefined for a value no int holds)
    constexpr int kNever = 1 << 20;
    auto cycles_to = [](double last, double rho, double t) {
        if (!(last > t)) return 0;
        const double k = std::floor(std::log(t / last) / std::log(rho));
        return k < (double)kNever ? (int)std::max(k, 0.0) : kNever;
    };
    // candidate split points: a level's last cycle before it can be predicted to fire (its
    // norm under eps / 4 for two visits)
    struct Cand {
        int k, level;   // predicted to fire from cycle k
        double norm;
    };
    std::vector<Cand> cand;
    for (int l = 1; l < c->nb; ++l) {
        double last, rho;
        if (c->hist.lvl_fire[l] || !spec_level_trend(c, l, &last, &rho)) continue;
        bool exact = c->hist.lvl_exact[l] != 0;
        if (!exact) {
            // a speculating level records "does not fire" up to its crossing of 100 eps within
            // the segment anyway (spec_mark_levels); what a split can give it is the firing
            // prediction, from a segment that ends after its steep decay took it under eps / 4
            const int k = cycles_to(last, rho, lim);
            if (k >= seg) continue;
            if (k >= 2) {
                const int kf = k + cycles_to(lim, rho, flim) + 2;
                if (kf < seg && !c->hist.lvl_fire_block[l])
                    cand.push_back({kf, l, last * std::pow(rho, (double)kf)});
                continue;
            }
            exact = true;   // in-stream from this segment on
        }
        if (exact && !c->hist.lvl_fire_block[l]) {
            // the fire test looks at the LARGER check norm of a visit: its decay; a level whose
            // norm stagnates (the one above the finest typically hovers at 0.5-1 eps for good)
            // or that already had a split at a similar norm gets none
            const std::vector<double> &h = c->hist.lvl_hist[l];
            const size_t m = h.size();
            const double ml = std::max(h[m - 1], h[m - 2]);
            const double mp = m >= 4 ? std::max(h[m - 3], h[m - 4]) : 0.0;
            const double rm = mp > 0.0 ? ml / mp : 1.0;
            if (rm > 0.9 || (c->hist.lvl_fire_try[l] > 0.0 && ml > 0.5 * c->hist.lvl_fire_try[l])) continue;
            // (the decay slows near eps: ~0.7 per cycle on the reference problem, where the
            // steep phase shows ~0.33; a split that comes too early costs without paying)
            const int k = cycles_to(ml, std::max(rm, 0.7), flim) + 2;
            if (k < seg) cand.push_back({std::max(k, 2), l, ml});
        }
    }
    // level-cycles that avoid two in-stream launches (~10 us each) if the segment ends at
    // k: a level that can be predicted to fire by k does so for seg - k
    int best_k = seg;
    double best = 0.0;
    for (const auto &q : cand) {
        const int k = q.k;
        double saved = 0.0;
        for (const auto &p : cand) saved += p.k <= k ? seg - k : 0;
        if (saved > best) {
            best = saved;
            best_k = k;
        }
    }
    const double N0 = (double)c->lv[0].N;
    const double cost = 16.0 * N0 * N0 / 5e12 + 60e-6;
    if (tuning_int("PGMG_SPEC_TRACE", 0))
        fprintf(stderr, "spec plan: seg %d, %zu candidates, best split %d saves %.0f us vs %.0f us\n",
                seg, cand.size(), best_k, best * 10.0, cost * 1e6);
    if (!(best * 10e-6 > cost)) return seg;
    for (const auto &p : cand)
        if (p.k <= best_k) c->hist.lvl_fire_try[p.level] = p.norm;
    return best_k;
}

// (a level-0 norm of a sampled check -- hnorm[i] with chks[i].bound -- is a lower bound of the
// check's norm; lvl_hist[0] is kept for traces only: every reader below starts at level 1)
static void spec_record_norms(pgmg_ctx *c, int n)
{
    for (int i = 0; i < n; ++i) {
        std::vector<double> &h = c->hist.lvl_hist[c->chks[i].level];
        h.push_back(c->hnorm[i]);
        if (h.size() > 8) h.erase(h.begin(), h.end() - 4);
    }
    if (c->call.spec_gamma <= 1) return;
    // W-cycle plan: the norms of the segment's last cycle, per visit
    const int nv = c->call.wvisit, seg = c->call.wseg;
    const std::vector<double> pmin = c->hist.wplan_gamma == c->call.spec_gamma ? c->hist.wmin : std::vector<double>();
    const int pseg = c->hist.wplan_seg;
    c->hist.wmax.clear();
    c->hist.wmin.clear();
    c->hist.wrho.clear();
    c->hist.wplan_gamma = 0;
    if (nv == 0 || seg <= 0 || nv % seg != 0 || (int)c->chk_visit.size() != n) return;
    const int vc = nv / seg, v0 = nv - vc;
    c->hist.wmax.assign(vc, -1.0);
    c->hist.wmin.assign(vc, HUGE_VAL);
    for (int i = 0; i < n; ++i) {
        const int v = c->chk_visit[i];
        if (v < v0) continue;
        c->hist.wmax[v - v0] = std::max(c->hist.wmax[v - v0], c->hnorm[i]);
        c->hist.wmin[v - v0] = std::min(c->hist.wmin[v - v0], c->hnorm[i]);
    }
    // per-cycle decay of each visit's smaller norm since the previous plan (0: unknown; the
    // first cycles of a problem fall by orders of magnitude, so no "does not fire" without it)
    c->hist.wrho.assign(vc, 0.0);
    if ((int)pmin.size() == vc && pseg > 0)
        for (int i = 0; i < vc; ++i)
            if (pmin[i] > 0.0 && pmin[i] < HUGE_VAL && c->hist.wmin[i] < HUGE_VAL)
                c->hist.wrho[i] = std::min(1.0, std::pow(c->hist.wmin[i] / pmin[i], 1.0 / seg));
    c->hist.wplan_gamma = c->call.spec_gamma;
    c->hist.wplan_seg = seg;
    if (tuning_int("PGMG_SPEC_TRACE", 0)) {
        int f = 0, q = 0;
        for (int i = 0; i < vc; ++i) {
            f += c->hist.wmax[i] >= 0.0 && c->hist.wmax[i] < 0.25 * c->cfg.eps;
            q += c->hist.wrho[i] > 0.0 && c->hist.wmin[i] * c->hist.wrho[i] * 0.01 >= c->cfg.eps;
        }
        fprintf(stderr, "W plan: %d visits per cycle, %d predicted to fire, %d not (1 cycle)\n",
                vc, f, q);
        // per level: visits, both checks < eps/4, max < eps, and the first visits (in cycle
        // order) whose max norm is >= eps/4 (measurement trace)
        std::vector<int> vlev(vc, -1);
        for (int i = 0; i < n; ++i)
            if (c->chk_visit[i] >= v0) vlev[c->chk_visit[i] - v0] = c->chks[i].level;
        for (int l = 1; l < 32; ++l) {
            int tot = 0, f4 = 0, f1 = 0;
            std::string nf;
            for (int i = 0; i < vc; ++i) {
                if (vlev[i] != l) continue;
                const bool a = c->hist.wmax[i] >= 0.0 && c->hist.wmax[i] < 0.25 * c->cfg.eps;
                f4 += a;
                f1 += c->hist.wmax[i] >= 0.0 && c->hist.wmax[i] < c->cfg.eps;
                if (!a && nf.size() < 400) nf += " " + std::to_string(tot) + ":" + std::to_string(c->hist.wmax[i] / c->cfg.eps);
                ++tot;
            }
            if (tot) fprintf(stderr, "  level %d: %d visits, %d < eps/4, %d < eps; others (index:max/eps):%s\n",
                             l, tot, f4, f1, nf.c_str());
        }
    }
}

// Validation of a speculative call's check log (one host round trip): every recorded check
// re-reduced and compared with its recorded decision (k_verify_checks; row strips: the ranks
// agree by allreduce(min)).  *h = 1 when some check could not be confirmed -- the call must
// be rolled back -- or the log overflowed; per-check norms and verdicts land in hnorm / hflag.
// Only the first n_any checks decide the rollback (the carry pass logs one more).
int pgmg::spec_validate(pgmg_ctx *c, unsigned *h_out, bool *overflow_out, int n_any)
{
    const int n = (int)c->chks.size();
    bool overflow = false;
    for (const CheckRef &k : c->chks) overflow |= k.np < 0;
    unsigned h = overflow ? 1u : 0u;
    c->hnorm.assign(n, 0.0);
    c->hflag.assign(n, 1u);
    if (n > 0 && !overflow) {
        // through the pinned (coherent) staging area: k_verify_checks reads the CheckRefs from
        // it and k_spec_reply writes the verdicts, the norms and their OR into it -- two
        // kernels and one stream wait, no copy operations
        CheckRef *hc = reinterpret_cast<CheckRef *>(c->pin);
        double *hn = reinterpret_cast<double *>(c->pin + pin_norm_off(c->chk_cap));
        unsigned *hf = reinterpret_cast<unsigned *>(c->pin + pin_flag_off(c->chk_cap));
        std::memcpy(hc, c->chks.data(), n * sizeof(CheckRef));
        launch_verify_checks(hc, n, c->cfg.eps, c->uflags, c->chk_norm, c->s);
        int e;
        if (c->comm && (e = c->comm->allreduce_min_u32(c->uflags, n, c->s))) return e;
        // (the checks past n_any -- the carried pre-smooth's -- never roll the call back)
        unsigned *hseq = reinterpret_cast<unsigned *>(c->pin + pin_seq_off(c->chk_cap));
        const unsigned seq = ++c->pin_seq;
        launch_spec_reply(c->uflags, c->chk_norm, n, n_any, hf + c->chk_cap, hn, hf, hseq, seq, c->s);
        PGMG_TRY(reply_wait(c, hseq, seq));
        h = hf[c->chk_cap];
        std::memcpy(c->hnorm.data(), hn, n * sizeof(double));
        std::memcpy(c->hflag.data(), hf, n * sizeof(unsigned));
    } else {
        PGMG_TRY(stream_wait(c));
    }
    *h_out = h;
    *overflow_out = overflow;
    return PGMG_OK;
}

int pgmg::run_cycles_spec(pgmg_ctx *c, int ncycles, int gamma)
{
    Level &L0 = c->lv[0];
    const int np0 = fused_blocks(L0.N, L0.lo / 2, (L0.hi < L0.N ? L0.hi : L0.N - 1) / 2);
    // (k_postpre's partials, in any form: the recompute form's tiles are narrower)
    const int npp = c->cross ? std::max(postpre_blocks(L0.N, L0.lo / 2, (L0.hi < L0.N ? L0.hi : L0.N - 1) / 2),
                                        postpre_blocks(L0.N, L0.lo / 2, (L0.hi < L0.N ? L0.hi : L0.N - 1) / 2, true))
                             : 0;
    long long d1, k1;
    spec_need_level(c, 1, gamma, &d1, &k1);
    // (level 0 visits level 1 gamma times per cycle)
    const long long per_dbl = 2LL * std::max(np0, npp) + gamma * d1, per_chk = 2 + gamma * k1;
    // segments of at most 2^27 logged doubles (1 GiB) / 2^22 checks
    long long seg_max = std::min(((1LL << 27) - 2LL * std::max(np0, npp)) / per_dbl, ((1LL << 22) - 2) / per_chk);
    if (c->cfg.spec_segment > 0) seg_max = std::min<long long>(seg_max, c->cfg.spec_segment);
    if (seg_max < 1) return run_cycles_plain(c, ncycles, gamma);
    // the cross-fused cycles keep A intact (rotation through S); otherwise copy it
    const bool rotate = c->cross && c->S.base != nullptr;
    // an in-place device call (run_cycles_ext): the first segment reads the caller's phi, the
    // last writes it -- that final k_post only after the validation, since it overwrites the
    // call's input (a rollback reruns from it)
    const void *const ext_in = c->call.x_in;
    void *const ext_out = c->call.x_out;
    bool first = true;
    c->call.spec_gamma = gamma;
    c->wcount[0] = c->wcount[1] = c->wcount[2] = 0;
    while (ncycles > 0) {
        const int seg = spec_plan_segment(c, (int)std::min<long long>(ncycles, seg_max));
        c->call.x_in = first ? ext_in : nullptr;
        c->call.x_out = ext_out;
        int e = spec_reserve(c, seg * per_dbl + 2LL * std::max(np0, npp) + 64, seg * per_chk + 4);
        if (e) return e;
        if ((e = spec_mark_levels(c, seg))) return e;
        if (c->hist.spec_off) return run_cycles_plain(c, ncycles, gamma, first);
        const bool last = seg == ncycles;
        const bool seg_first = first;
        const Grid A0 = L0.A, B0 = L0.B, S0 = c->S;
        if (!rotate) {
            if (!c->bk.base && (e = alloc_grid(c->bk, L0))) return e;
            HIPC(hipMemcpyAsync(c->bk.base, L0.A.base, L0.A.bytes, hipMemcpyDeviceToDevice, c->s));
        }
        // stats backup + the coarse levels' "pre-smooth fired" flags (written by the skipped
        // fix-ups) = 0, one launch
        launch_spec_open(c->stats, c->stats_bk, c->flags, (int)(c->lv.size() + 1) * 2 * kMaxSweeps, c->s);
        c->call.lean = true;
        c->plog_used = 0;
        c->chks.clear();
        c->chk_visit.clear();
        c->call.wvisit = 0;
        c->call.wseg = seg;
        std::fill(c->hist.lvl_vis.begin(), c->hist.lvl_vis.end(), 0);
        if (!last) c->call.x_out = nullptr;   // intermediate segments end in the level-0 grids
        c->call.defer_post = ext_out != nullptr && last;
        // the carry: the last segment of a V call on the context's own grids ends with the
        // carry pass (enqueue_cross_cycles, "carry"); c->call.carry_use was set by run_cycles for
        // the first segment
        // (true on the staged device-bound path too, whose carry nobody can take)
        c->call.carry_make = last && gamma == 1 && ext_out == nullptr &&
                             !(c->cfg.flags & PGMG_FLAG_NO_CARRY) &&
                             tuning_int("PGMG_CARRY_MAKE", 1) != 0;   // (measurement build: 0 never makes)
        c->call.carry_chk = -1;
        e = run_cycles_plain(c, seg, gamma, first);
        // what a rollback's in-stream rerun of the rest of the call must not inherit
        c->call.defer_post = false;
        c->call.x_out = ext_out;
        c->call.lean = false;
        first = false;
        if (e) return e;
        int n = (int)c->chks.size();
        const bool made = c->call.carry_made && c->call.carry_chk == n - 1;
        if (c->call.carry_made && !made) return set_err(PGMG_ERR_STATE, "carry check out of place");
        unsigned h = 0;
        bool overflow = false;
        if ((e = spec_validate(c, &h, &overflow, made ? n - 1 : n))) return e;
        if (h) {
            // some check could fire: roll back this segment, rerun the rest of the call with
            // in-stream decisions; the levels whose checks could fire stay in-stream
            ++c->rollbacks;
            if (gamma > 1) {   // a W plan's prediction failed
                c->hist.wplan_off = true;
                c->hist.wmax.clear();
                c->hist.wmin.clear();
                c->hist.wrho.clear();
            }
            // a flagged finest-level check that is a lower bound (sampled) proves nothing yet:
            // the rerun's full sums decide below whether the context stops speculating
            bool bound_hit = false;
            for (int i = 0; i < n; ++i)
                if (c->hflag[i] || overflow) {
                    const int l = c->chks[i].level;
                    if (l == 0) {
                        if (c->chks[i].bound && !overflow) bound_hit = true;
                        else c->hist.spec_off = true;
                    } else {
                        c->hist.lvl_exact[l] = 1;
                        if (c->chks[i].expect == 1) {   // a "fires" prediction failed
                            c->hist.lvl_fire[l] = 0;
                            c->hist.lvl_fire_block[l] = 1;
                        }
                    }
                }
            L0.A = A0;
            L0.B = B0;
            c->S = S0;
            c->carry = false;
            if (!rotate)
                HIPC(hipMemcpyAsync(L0.A.base, c->bk.base, L0.A.bytes, hipMemcpyDeviceToDevice, c->s));
            HIPC(hipMemcpyAsync(c->stats, c->stats_bk, 4 * sizeof(unsigned long long),
                                hipMemcpyDeviceToDevice, c->s));
            c->call.x_in = seg_first ? ext_in : nullptr;
            if (!bound_hit || c->hist.spec_off) return run_cycles_plain(c, ncycles, gamma, false);
            // Only sampled checks could fire.  stats[2] / stats[3] count the cross-cycle checks
            // that k_postpre_decide let fire (nothing else writes them; the opening k_pre's and
            // the closing k_post's checks were logged as full sums and did not fire): unchanged
            // over the rerun, the finest norm is above eps but within the sample's factor of it.
            if ((e = run_cycles_plain(c, ncycles, gamma, false))) return e;
            PGMG_TRY(stream_wait(c));
            unsigned long long now[2] = {0, 0}, was[2] = {0, 0};
            HIPC(hipMemcpy(now, c->stats + 2, sizeof(now), hipMemcpyDeviceToHost));
            HIPC(hipMemcpy(was, c->stats_bk + 2, sizeof(was), hipMemcpyDeviceToHost));
            if (now[0] == was[0] && now[1] == was[1]) {
                c->hist.full_sums = true;
                ++c->sampled_n[1];
            } else {
                c->hist.spec_off = true;
            }
            return PGMG_OK;
        }
        if (seg_first && c->call.carry_took) ++c->carry_n[0];
        if (made) {
            // the carried pre-smooth: usable unless its check could fire (then dropped: the
            // next call runs its own k_pre); not one of this call's checks
            const bool ok = !overflow && c->hflag[n - 1] == 0u;
            c->carry = ok;
            ++c->carry_n[ok ? 1 : 2];
            --n;
            c->chks.pop_back();
            c->chk_visit.pop_back();
            c->hnorm.pop_back();
            c->hflag.pop_back();
        }
        spec_record_norms(c, n);
        if (ext_out != nullptr && last) {
            if ((e = enqueue_last_post(c))) return e;
        }
        ncycles -= seg;
    }
    return PGMG_OK;
}

extern "C" {   // what the speculation did (read-only)

int pgmg_carry_info(pgmg_ctx *c, long long out[3])
{
    if (!c || !out) return set_err(PGMG_ERR_ARG, "null argument");
    for (int i = 0; i < 3; ++i) out[i] = c->carry_n[i];
    return PGMG_OK;
}

int pgmg_spec_sampled_info(pgmg_ctx *c, long long out[3])
{
    if (!c || !out) return set_err(PGMG_ERR_ARG, "null argument");
    out[0] = c->sampled_n[0];
    out[1] = c->sampled_n[1];
    out[2] = c->hist.full_sums ? 1 : 0;
    return PGMG_OK;
}

int pgmg_dist_info(pgmg_ctx *c, int *speculative, long long *rollbacks)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (speculative) *speculative = c->spec ? 1 : 0;
    if (rollbacks) *rollbacks = c->rollbacks;
    return PGMG_OK;
}

int pgmg_spec_levels(pgmg_ctx *c, unsigned long long *in_stream)
{
    if (!c || !in_stream) return set_err(PGMG_ERR_ARG, "null argument");
    unsigned long long m = (!c->spec || c->hist.spec_off) ? 1ull : 0ull;
    for (int l = 1; l < (int)c->hist.lvl_exact.size() && l < 64; ++l)
        if (c->hist.lvl_exact[l] || c->hist.lvl_fire[l]) m |= 1ull << l;
    *in_stream = m;
    return PGMG_OK;
}

int pgmg_spec_visit_modes(pgmg_ctx *c, long long counts[3])
{
    if (!c || !counts) return set_err(PGMG_ERR_ARG, "null argument");
    for (int i = 0; i < 3; ++i) counts[i] = c->wcount[i];
    return PGMG_OK;
}

int pgmg_spec_fire_levels(pgmg_ctx *c, unsigned long long *fire)
{
    if (!c || !fire) return set_err(PGMG_ERR_ARG, "null argument");
    unsigned long long m = 0;
    for (int l = 1; l < (int)c->hist.lvl_fire.size() && l < 64; ++l)
        if (c->hist.lvl_fire[l]) m |= 1ull << l;
    *fire = m;
    return PGMG_OK;
}

}  // extern "C"
