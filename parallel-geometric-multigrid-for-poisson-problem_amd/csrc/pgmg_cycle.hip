// pgmg_cycle.hip — the kernel sequences of the V- and W-cycle: how a call's checks are
// enqueued and logged (check log, "W-cycle plans"), one level's passes, the cross-fused finest
// level with the "carry", run_cycles_plain.  Host code only: every kernel is behind a launcher.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>

#include "pgmg_host.h"
#include "pgmg_coarse.h"

using namespace pgmg;

// Speculative call: a fresh slice of the partials log for one early-exit check, recorded
// for the validation after the call (nullptr when the cycles being enqueued decide every
// check in-stream).  The log is sized beforehand (spec_need); running past it would be a
// bug: the check then writes the shared partials and the call is treated as failed
// validation (rolled back), never read out of bounds.
// How a speculative call enqueues level l's checks: 0 recorded as "does not fire" (no
// fix-up), 1 recorded as "fires" (the one-sweep passes, no fix-up), 2 decided in-stream (the
// fix-ups; outside speculative calls every check).
// W-cycles (gamma > 1): a bulk level's visits are planned one by one (w_visit_mode)
static int chk_mode(const pgmg_ctx *c, int level)
{
    if (c->call.lean && c->call.fspec) return 0;   // speculative F-cycles: every bulk check
    if (!c->call.lean || (c->call.spec_gamma > 1 && level > 0) || c->hist.lvl_exact[level]) return 2;
    return c->hist.lvl_fire[level] ? 1 : 0;
}

// W-cycle plans (one GPU).  A W-cycle visits level l 3^l times and every visit's checks are a
// different story: a visit right after its parent's restriction starts from a large residual,
// the later ones from a nearly solved one -- per level, some visits fire and some do not in
// every cycle, so the per-level policy of the V-cycles leaves every bulk check in-stream (a
// pass and a rare-path launch each, ~5 % of a W-cycle at 4097).  The visits of a cycle come
// in the same order every cycle and their norms fall from cycle to cycle (by ~0.15 at 4097 in
// the steady phase, by orders of magnitude in the first cycles), so visit v of the next cycle
// is planned from visit v of the last validated one: predicted to fire (k_pre1 / k_post1) when
// both of its checks were below eps / 4, recorded "does not fire" when both stay above eps
// with the decay the visit showed since the previous plan, per cycle of the new segment, and a
// further 100-fold margin; in-stream otherwise.  A failed prediction rolls the segment back and ends the plans for the
// problem.
static int w_visit_mode(pgmg_ctx *c, int l)
{
    if (!c->call.lean || c->call.spec_gamma <= 1 || l == 0) return -1;
    const int v = c->call.wvisit++;
    c->call.cur_visit = v;
    const int vc = (int)c->hist.wmax.size();
    int m = 2;
    if (!c->hist.wplan_off && c->hist.wplan_gamma == c->call.spec_gamma && vc > 0) {
        const int pos = v % vc;
        const double eps = c->cfg.eps;
        if (c->hist.wmax[pos] >= 0.0 && c->hist.wmax[pos] < 0.25 * eps) m = 1;
        else if (c->hist.wrho[pos] > 0.0 &&
                 c->hist.wmin[pos] * std::pow(c->hist.wrho[pos], (double)c->call.wseg) * 0.01 >= eps)
            m = 0;
    }
    ++c->wcount[m];
    return m;
}

double *pgmg::chk_log(pgmg_ctx *c, int np, int level, int mode)
{
    if (!c->call.lean || (mode == 2 && c->comm != nullptr)) return nullptr;
    c->chk_visit.push_back(level > 0 ? c->call.cur_visit : -1);
    if (c->plog_used + np > c->plog_cap) {
        c->chks.push_back({nullptr, -1, level, mode});
        return c->partials;
    }
    double *p = c->plog + c->plog_used;
    c->plog_used += np;
    c->chks.push_back({p, np, level, mode});
    return p;
}

// the slice of a check recorded as "does not fire" (nullptr: decide it in-stream)
static double *chk_partials(pgmg_ctx *c, int np, int level)
{
    return chk_mode(c, level) == 0 ? chk_log(c, np, level, 0) : nullptr;
}

// Sampled checks (pgmg_postpre_impl.h): may the finest pass being enqueued sum its two checks
// on a sample of its rows?  Only where both are recorded "does not fire" by a speculative V or
// W call on one GPU, and the context has not fallen back to full sums (pgmg_spec.hip, "sampled
// checks"); every pass decided in-stream -- k_postpre_decide -- launches the full-sum form.
static bool pp_sampled(const pgmg_ctx *c)
{
    return c->call.lean && !c->call.fspec && c->comm == nullptr && chk_mode(c, 0) == 0 &&
           !c->hist.full_sums && !(c->cfg.flags & (PGMG_FLAG_FULL_CHECKS | PGMG_FLAG_EXACT_DIST));
}

// The last n checks logged hold lower bounds of their sums (a sampled pass's): such a check
// can only be recorded "does not fire".
static int chk_mark_bound(pgmg_ctx *c, int n)
{
    if ((int)c->chks.size() < n) return set_err(PGMG_ERR_STATE, "sampled checks: not logged");
    for (size_t i = c->chks.size() - n; i < c->chks.size(); ++i) {
        if (c->chks[i].expect != 0)
            return set_err(PGMG_ERR_STATE, "sampled checks: a lower bound logged as anything but \"does not fire\"");
        c->chks[i].bound = 1;
    }
    return PGMG_OK;
}

// ---------------------------------------------------------------------------
// kernel sequences
// ---------------------------------------------------------------------------
static unsigned *smooth_flags(pgmg_ctx *c, int l, int which)
{
    return c->flags + ((size_t)l * 2 + which) * kMaxSweeps;
}

static int timed_begin(pgmg_ctx *c, int slot)
{
    auto &pool = c->tpool[slot];
    if (!(c->cfg.flags & PGMG_FLAG_TIME_FINE) || pool.used + 2 > (int)pool.ev.size()) return -1;
    HIPC(hipEventRecord(pool.ev[pool.used], c->s));
    return pool.used;
}

static int timed_end(pgmg_ctx *c, int slot, int idx)
{
    if (idx < 0) return PGMG_OK;
    auto &pool = c->tpool[slot];
    HIPC(hipEventRecord(pool.ev[idx + 1], c->s));
    pool.used = idx + 2;
    c->tbytes[slot] += g_last_launch.bytes;   // the launch just timed (LaunchNote)
    c->tkern[slot] = g_last_launch.kernel;
    return PGMG_OK;
}

// ---------------------------------------------------------------------------
// Level geometry and the fused passes' argument blocks.  strip_rows alone derives a pass's rows
// from a level; pre_args / post_args fill what follows from the context and the level, whoever
// launches the pass the rest: iterates, pin_ec, fired, cond, Px / Po, sw_adj, extended post rows.
// ---------------------------------------------------------------------------
StripRows pgmg::strip_rows(const Level &L, const Level &C)
{
    StripRows r;
    r.jc0 = L.lo / 2;
    r.jc1 = (L.hi < L.N ? L.hi : L.N - 1) / 2;
    r.row_lo = L.u0;
    r.row_hi = L.u1;
    // coarse rows this rank restricts into (its strip's rows; the fix-up honours them too)
    r.rc_lo = r.jc0 > 1 ? r.jc0 : 1;
    r.rc_hi = r.jc1 < C.N - 1 ? r.jc1 : C.N - 1;
    r.x_lo = L.u0 - 4 > 1 ? L.u0 - 4 : 1;
    r.x_hi = L.u1 + 4 < L.N - 1 ? L.u1 + 4 : L.N - 1;
    return r;
}

PostRows pgmg::post_rows(const pgmg_ctx *c, int l)
{
    const Level &L = c->lv[l];
    if (l > 0 && is_dist(c, l)) {
        const int r0 = std::max(L.lo - kPostExt, 0), r1 = std::min(L.hi + kPostExt, L.N - 1);
        return {r0 / 2, r1 / 2, std::max(r0, 1), r1};
    }
    const StripRows sr = strip_rows(L, c->lv[l + 1]);
    return {sr.jc0, sr.jc1, sr.row_lo, sr.row_hi};
}

int pgmg::tile_np(const pgmg_ctx *c, int l, bool post)
{
    if (l < 1 || l >= c->nb) return 0;
    const Level &L = c->lv[l];
    if (!coarse_tile_ok(L.N, is_dist(c, l))) return 0;
    const StripRows sr = strip_rows(L, c->lv[l + 1]);
    const PostRows pr = post_rows(c, l);
    return post ? coarse_tile_blocks_rows(L.N, std::max(pr.jc0, 1), std::min(pr.jc1, c->lv[l + 1].N - 1))
                : coarse_tile_blocks_rows(L.N, sr.rc_lo, sr.rc_hi);
}

// level 0 with an analytic RHS, or the F climb's current level: regenerate f in-kernel
static const double *gen_table(const pgmg_ctx *c, int l, const double *fine, const double *climb)
{
    return l == 0 ? fine : (l == c->call.gen_level ? climb : nullptr);
}

template <class T>
static PreArgsT<T> pre_args(const pgmg_ctx *c, int l)
{
    const Level &L = c->lv[l], &C = c->lv[l + 1];
    PreArgsT<T> pa{};
    pa.f = G<T>(L.F);
    pa.rc = G<T>(C.F);
    pa.partials = c->partials;
    pa.stats = c->stats;
    const StripRows sr = pass_geometry(pa, L, C);
    pa.rc_lo = sr.rc_lo;
    pa.rc_hi = sr.rc_hi;
    pa.gfx = gen_table(c, l, c->rgfx, c->call.lgfx);
    pa.gsy = gen_table(c, l, c->rgsy, c->call.lgsy);
    return pa;
}

template <class T>
static PostArgsT<T> post_args(const pgmg_ctx *c, int l)
{
    const Level &L = c->lv[l], &C = c->lv[l + 1];
    PostArgsT<T> po{};
    po.ec = G<T>(C.A);
    po.f = G<T>(L.F);
    po.partials = c->partials;
    po.stats = c->stats;
    pass_geometry(po, L, C);
    po.gfx = gen_table(c, l, c->rgfx, c->call.lgfx);
    po.gsy = gen_table(c, l, c->rgsy, c->call.lgsy);
    return po;
}

// the fix-up / rare-path block of a check with np partials, decided from the shared partials
static FixArgsF fix_args(const pgmg_ctx *c, int np)
{
    FixArgsF fa{};
    fa.partials = c->partials;
    fa.np = np;
    fa.eps = c->cfg.eps;
    fa.stats = c->stats;
    return fa;
}

template <class T> static int enqueue_children(pgmg_ctx *c, int l, int gamma);
template <class T> static int enqueue_cycle_t(pgmg_ctx *c, int l, int gamma, bool x0_zero);

// one JacobiSmoother::smooth(x = L.A, f = L.F, num_iter = v) on a bulk level
template <class T>
static int enqueue_smooth_t(pgmg_ctx *c, int l, int which, int v, bool x0_zero)
{
    Level &L = c->lv[l];
    const int S = v + 1;
    unsigned *D = smooth_flags(c, l, which);
    const bool fine = (l == 0);
    for (int k = 1; k <= S; ++k) {
        T *in = G<T>((k & 1) ? L.A : L.B);
        T *out = G<T>((k & 1) ? L.B : L.A);
        if (is_dist(c, l) && !(k == 1 && x0_zero)) PGMG_TRY(c->comm->halo((k & 1) ? L.A : L.B, L, 1, c->s));
        SweepArgsT<T> a{};
        a.xin = (k == 1 && x0_zero) ? nullptr : in;
        a.f = G<T>(L.F);
        a.xout = out;
        a.partials = (k >= 2) ? c->partials : nullptr;
        a.skip = (k >= 2) ? &D[k - 1] : nullptr;
        a.reset = (k == 1) ? &D[1] : nullptr;
        a.stats = c->stats;
        a.hh = (T)L.hh;
        a.inv_hh = (T)L.ih;
        a.W = L.N;
        a.P = L.P;
        a.row0 = L.u0;
        a.row1 = L.u1;
        const int ev = (fine && a.partials == nullptr && !(k == 1 && x0_zero)) ? timed_begin(c, 0) : -1;
        launch_sweep(a, k == 1 && x0_zero, l == 0, c->s);
        PGMG_TRY(timed_end(c, 0, ev));
        if (k >= 2) {
            int rpb, gx, gy;
            const int np = sweep_blocks(L.N, L.u0, L.u1, &rpb, &gx, &gy);
            FixupArgsT<T> f{};
            f.partials = c->partials;
            f.np = np;
            f.eps = c->cfg.eps;
            f.done_prev = &D[k - 1];
            f.done_next = &D[k];
            f.src = in;
            f.dst = out;
            f.stats = c->stats;
            f.W = L.N;
            f.P = L.P;
            f.row0 = L.u0;
            f.row1 = L.u1;
            f.global_sum = nullptr;
            if (is_dist(c, l)) {
                launch_sum_partials(c->partials, np, c->scalar, c->s);
                PGMG_TRY(c->comm->allreduce_sum(c->scalar, 1, c->s));
                f.global_sum = c->scalar;
            }
            launch_fixup(f, c->s);
        }
    }
    if (S & 1) launch_copy_rows(G<T>(L.B), G<T>(L.A), L.N, L.P, L.u0, L.u1, c->s);
    return PGMG_OK;
}

int pgmg::enqueue_smooth(pgmg_ctx *c, int l, int which, int v, bool x0_zero)
{
    return c->fp32 ? enqueue_smooth_t<float>(c, l, which, v, x0_zero)
                   : enqueue_smooth_t<double>(c, l, which, v, x0_zero);
}

template <class T>
static int enqueue_tail_t(pgmg_ctx *c, int gamma, bool x0_from_global, int visits = 1)
{
    TailArgsT<T> t = tail_args<T>(c);
    t.visits = visits;
    t.x0_from_global = x0_from_global ? 1 : 0;
    HIPC(launch_tail_gamma(t, gamma, c->s));
    return PGMG_OK;
}

int pgmg::enqueue_tail(pgmg_ctx *c, int gamma, bool x0_from_global)
{
    return c->fp32 ? enqueue_tail_t<float>(c, gamma, x0_from_global)
                   : enqueue_tail_t<double>(c, gamma, x0_from_global);
}

// children of level l: gamma cycles on level l+1 (on rank 0 alone if it is gathered)
template <class T>
static int enqueue_children(pgmg_ctx *c, int l, int gamma)
{
    if (c->comm && l + 1 == c->comm->gathered_level())
        return c->comm->run_gathered(c, l + 1, gamma, gamma);
    // the tail level: the gamma visits (same right-hand side, each from the previous one's
    // result; the first from zero) in one launch -- at N = 32769 a W-cycle launches the tail
    // 3^9 times, one launch per visit cost ~8 % of its time in launch overhead
    if (l + 1 == c->nb && gamma > 1 && tuning_int("PGMG_TAIL_VISITS", 1) != 0)
        return enqueue_tail_t<T>(c, gamma, false, gamma);
    for (int i = 0; i < gamma; ++i) PGMG_TRY(enqueue_cycle_t<T>(c, l + 1, gamma, i == 0));
    return PGMG_OK;
}

// global early-exit sum for a distributed level: local partial sum, then all ranks
static int global_sum(pgmg_ctx *c, int np, const double **out)
{
    launch_sum_partials(c->partials, np, c->scalar, c->s);
    *out = c->scalar;
    return c->comm->allreduce_sum(c->scalar, 1, c->s);
}

// the block of level l's in-stream decision after a pass with np partials: decided from the
// pass's log slice lp (a speculative call logs the norm) or the shared partials, on row strips
// from the all-rank sum; a tile pass's rare path reads the same from its own block
template <class T>
static int decide_args(pgmg_ctx *c, int l, int np, const double *lp, FixArgsF *fa, CoarseArgsT<T> *tile)
{
    *fa = fix_args(c, np);
    if (lp) fa->partials = lp;
    if (is_dist(c, l)) PGMG_TRY(global_sum(c, np, &fa->global_sum));
    if (tile == nullptr) return PGMG_OK;
    tile->global_sum = fa->global_sum;
    tile->dec_partials = fa->partials;
    tile->dec_np = fa->np;
    tile->eps = fa->eps;
    return PGMG_OK;
}

// The two halves of a fused level, each one checked pass: a log slice for the check (mode as
// chk_mode), the pass in its timed slot (finest level) -- the tile form (tile != nullptr), the
// one-sweep form (mode 1) or the full one -- and for an in-stream check (mode 2) the rare path,
// tile or row-marching, decided on strips from the global sum.
template <class T>
static int enqueue_pre_half(pgmg_ctx *c, int l, int mode, bool x0_zero, PreArgsT<T> pa,
                            CoarseArgsT<T> *tile, int np)
{
    const bool fine = (l == 0);
    double *lp = chk_log(c, np, l, mode);
    if (lp) pa.partials = lp;
    const int ev = fine ? timed_begin(c, 1) : -1;
    if (tile) {
        tile->partials = pa.partials;
        launch_pre_tile(*tile, mode == 1 ? 1 : 0, c->s);
        HIPC(hipGetLastError());
    } else {
        PGMG_TRY(mode == 1 ? launch_pre1(pa, x0_zero, c->s) : launch_pre(pa, x0_zero, fine, c->s));
    }
    PGMG_TRY(timed_end(c, 1, ev));
    if (mode != 2) return PGMG_OK;
    FixArgsF fa;
    PGMG_TRY(decide_args(c, l, np, lp, &fa, tile));
    if (tile) {
        launch_pre_tile(*tile, 2, c->s);
        HIPC(hipGetLastError());
        return PGMG_OK;
    }
    return launch_pre_rare(fa, pa, x0_zero, c->s);
}

// r2 (mode 0 only): the finest k_post that also restricts its result to level 2 (k_post_r2)
template <class T>
static int enqueue_post_half(pgmg_ctx *c, int l, int mode, PostArgsT<T> po, CoarseArgsT<T> *tile,
                             int np, bool r2)
{
    const bool fine = (l == 0);
    double *lp = chk_log(c, np, l, mode);
    if (lp) po.partials = lp;
    const int ev = fine ? timed_begin(c, 2) : -1;
    if (r2) {
        po.r2out = G<T>(c->lv[2].A);
        po.Pr2 = c->lv[2].P;
        po.Nr2 = c->lv[2].N;
        PGMG_TRY(launch_post_r2(po, c->s));
        c->call.fr2_made = true;
    } else if (tile) {
        tile->partials = po.partials;
        launch_post_tile(*tile, mode == 1 ? 1 : 0, c->s);
        HIPC(hipGetLastError());
    } else {
        PGMG_TRY(mode == 1 ? launch_post1(po, c->s) : launch_post(po, fine, c->s));
    }
    PGMG_TRY(timed_end(c, 2, ev));
    if (mode != 2) return PGMG_OK;
    FixArgsF fa;
    PGMG_TRY(decide_args(c, l, np, lp, &fa, tile));
    if (tile) {
        launch_post_tile(*tile, 2, c->s);
        HIPC(hipGetLastError());
        return PGMG_OK;
    }
    return launch_post_rare(fa, po, c->s);
}

// the tile passes' block of level l (pgmg_coarse.hip); its rows (k_pre's, then k_post's): the caller's
template <class T>
static CoarseArgsT<T> tile_args(const pgmg_ctx *c, int l, unsigned *fired)
{
    const Level &L = c->lv[l], &C = c->lv[l + 1];
    CoarseArgsT<T> ca{};
    ca.f = G<T>(L.F);
    ca.ec = G<T>(C.A);
    ca.rc = G<T>(C.F);
    ca.x2 = G<T>(L.A);
    ca.stats = c->stats;
    ca.fired = fired;
    ca.pre_fired = fired;
    ca.hh = (T)L.hh;
    ca.ih = (T)L.ih;
    ca.N = L.N;
    ca.P = L.P;
    ca.Nc = C.N;
    ca.Pc = C.P;
    return ca;
}

// fused level (v1 = v2 = 1): k_pre (+fixup), children, k_post (+fixup)
// pin (F-cycle climb, x0_zero false): the level's x0 is the prolongation of level l+1's
// grid into a zeroed grid; k_pre computes it on the fly instead of reading L.A
// fr2_want (speculative F-cycle followed by another): see r2 below
template <class T>
static int enqueue_fused_level_t(pgmg_ctx *c, int l, int gamma, bool x0_zero, bool pin = false,
                                 bool fr2_want = false)
{
    Level &L = c->lv[l];
    Level &C = c->lv[l + 1];
    const bool dist = is_dist(c, l);
    // entered with x0 = 0: the pre-smoothed iterate is a function of f alone, so k_pre
    // does not store it and k_post recomputes it (x1 = J(0) is pointwise)
    const bool recomp = x0_zero && l > 0 && c->recompute;
    unsigned *fired = smooth_flags(c, l, 0) + (kMaxSweeps - 1);
    // row strips, levels below the finest: k_post also computes kPostExt rows past each
    // strip edge (from deeper halos of f and phi, exchanged with the pre-smooth's anyway),
    // so the parent's prolongation reads this level's correction without an exchange
    const bool ext = dist && l > 0;
    if (dist) {
        if (!x0_zero && !pin) PGMG_TRY(c->comm->halo(L.A, L, 4, c->s));
        // f: 4 rows for k_pre, 3 + kPostExt for the extended k_post (RECOMP reads f 3 rows
        // past its first output row)
        if (l > 0) PGMG_TRY(c->comm->halo(L.F, L, 3 + kPostExt, c->s));
    }
    PreArgsT<T> pa = pre_args<T>(c, l);
    pa.x0 = G<T>(L.A);
    pa.x2 = recomp ? nullptr : G<T>(L.B);
    pa.fired = recomp ? fired : nullptr;
    pa.pin_ec = pin ? G<T>(C.A) : nullptr;
    // speculative call: record the check (mode 0: no fix-up; 1: predicted to fire, the
    // one-sweep passes; 2: in-stream, logged for its norm)
    int mode = chk_mode(c, l);
    // V-cycles: a speculating level records "does not fire" up to its predicted crossing of
    // 100 eps (spec_mark_levels), in-stream after it
    if (mode == 0 && l > 0 && c->call.spec_gamma == 1 && !c->call.fspec && c->hist.lvl_vis[l]++ >= c->hist.lvl_kx[l])
        mode = 2;
    const int wm = w_visit_mode(c, l);
    const int visit = c->call.cur_visit;   // (the children's visits move it)
    if (wm >= 0) mode = wm;
    if (mode == 1 && (dist || pin || (x0_zero && !recomp))) mode = 2;
    // the small coarse levels (pgmg_coarse.hip): both passes, their predicted-to-fire
    // one-sweep forms and their in-stream rare paths as 2D LDS tiles; the checks' partial
    // count is the tile count
    // (row strips too: the tiles cover the rank's coarse rows, its interior rows own the check)
    const bool tile = recomp && !pin && pa.gfx == nullptr &&
                      !(c->cfg.flags & PGMG_FLAG_NO_CTILE) && coarse_tile_ok(L.N, dist) &&
                      pa.rc_hi > pa.rc_lo;
    CoarseArgsT<T> ca = tile_args<T>(c, l, fired);
    ca.jt0 = pa.rc_lo;
    ca.jt1 = pa.rc_hi;
    ca.own_lo = L.u0;
    ca.own_hi = L.u1;
    PGMG_TRY(enqueue_pre_half(c, l, mode, x0_zero, pa, tile ? &ca : nullptr,
                              tile ? tile_np(c, l, false) : fused_blocks(L.N, pa.jc0, pa.jc1)));
    PGMG_TRY(enqueue_children<T>(c, l, gamma));
    // the correction of level l+1 is not exchanged: a distributed child's k_post computed
    // it kPostExt rows past its strip (a gathered child's is replicated)
    if (dist && !recomp) PGMG_TRY(c->comm->halo(L.B, L, ext ? 2 + kPostExt : 2, c->s));
    PostArgsT<T> po = post_args<T>(c, l);
    po.phi = G<T>(L.B);
    po.pre_fired = recomp ? fired : nullptr;
    po.x2 = G<T>(L.A);
    if (ext) {   // rows [lo - kPostExt, hi + kPostExt) written, the strip's rows summed
        const PostRows pr = post_rows(c, l);
        po.jc0 = pr.jc0;
        po.jc1 = pr.jc1;
        po.row_lo = pr.row_lo;
        po.row_hi = pr.row_hi;
        po.sum_lo = L.u0;
        po.sum_hi = L.u1;
    }
    // k_post's tile rows: the strip plus kPostExt rows (dist), its own rows summed
    ca.jt0 = std::max(po.jc0, 1);
    ca.jt1 = std::min(po.jc1, C.N - 1);
    ca.own_lo = po.row_lo;
    ca.own_hi = po.row_hi;
    ca.sum_lo = po.sum_hi > po.sum_lo ? po.sum_lo : po.row_lo;
    ca.sum_hi = po.sum_hi > po.sum_lo ? po.sum_hi : po.row_hi;
    c->call.cur_visit = visit;
    // speculative F-cycle followed by another: the finest k_post also restricts its result to
    // level 2 (the next F-cycle's first restriction step; only when its check is recorded
    // "does not fire", so x2 is the result); its 116-column tiles write more partials
    const bool r2 = l == 0 && mode == 0 && fr2_want && !dist && !recomp && c->nb >= 2 &&
                    !is_dist(c, 1) && tuning_int("PGMG_F_R2", 1) != 0;
    const int np = tile ? tile_np(c, l, true)
                        : r2 ? post_r2_blocks(L.N, po.jc0, po.jc1) : fused_blocks(L.N, po.jc0, po.jc1);
    return enqueue_post_half(c, l, mode, po, tile ? &ca : nullptr, np, r2);
}

int pgmg::enqueue_fused_level(pgmg_ctx *c, int l, int gamma, bool x0_zero, bool pin, bool fr2_want)
{
    return c->fp32 ? enqueue_fused_level_t<float>(c, l, gamma, x0_zero, pin, fr2_want)
                   : enqueue_fused_level_t<double>(c, l, gamma, x0_zero, pin, fr2_want);
}

// ---------------------------------------------------------------------------
// Cross-cycle fusion of the finest level (v1 = v2 = 1): for n consecutive cycles
// the finest level runs k_pre, (children, k_postpre) x (n-1), children, k_post.
// k_postpre reads the pre-smoothed solution of cycle k from one level-0 buffer and
// writes that of cycle k+1 into the other, so the buffers alternate; at the end the
// solution is moved back under L.A by swapping the host pointers (B always mirrors
// A's boundary, so either may play either role).
//
// Row strips (level 0 distributed): every pass covers the rank's rows; before
// k_postpre one grouped exchange brings 6 halo rows of phi and 4 of the coarse
// correction; k_postpre also sums r(x2)^2 (the pre check of rare path 1, which
// restarts the pre-smooth from x1: J(x1) = x2), so ONE allreduce of three sums
// decides every rare path on every rank.  The rare paths rebuild their scratch
// iterate S on the rows the following k_pre reads (4 past the strip) from the
// exchanged halos instead of exchanging S.
// ---------------------------------------------------------------------------
// The finest level while a call's cross-fused cycles are enqueued.  Building an argument block
// changes none of it: the step that launches a pass moves pr on and consumes sw_adj / recompute.
template <class T>
struct CrossState {
    Grid gA, gB, gS;   // lv[0].A, lv[0].B and the scratch c->S as the call found them
    T *A, *B, *S;
    // speculative call: no rare path can run, so the scratch S is free and the level-0
    // buffers rotate through B and S; A (the call's input) is never written and a rollback
    // restarts from it
    bool lean;
    T *pr;            // pre-smoothed solution of the current cycle (a taken carry: the solution A)
    int sw_adj;       // the carried pre-smooth's two sweeps: counted by the next finest pass
    bool recompute;   // the next finest pass recomputes pr's pre-smooth (k_postpre's recompute form)

    const Grid &grid_of(const T *p) const { return p == A ? gA : p == B ? gB : gS; }
    // (an external input is followed by B: the first k_pre writes B, then B <-> S (lean) or
    // B <-> A, both free of the input; a carried input -- A itself -- is followed by B as well)
    T *next_of(const T *p) const { return lean ? (p == B ? S : B) : (p == B ? A : B); }
};

// st.pr is final.  Its halo rows (6 for k_postpre, 2 for the last k_post) are read only
// after the whole coarse hierarchy: the exchange runs on the comm's side stream
// meanwhile (the coarse correction's halo rows are computed locally, kPostExt)
template <class T>
static int enqueue_descend(pgmg_ctx *c, const CrossState<T> &st, int gamma)
{
    if (is_dist(c, 0)) PGMG_TRY(c->comm->halo_begin(st.grid_of(st.pr), c->lv[0], 6, c->s));
    return enqueue_children<T>(c, 0, gamma);
}

// cycle 1: pre-smooth (+ residual, restriction) of the call's input (A, or the caller's
// array: pgmg_set_problem_device) into B
template <class T>
static int enqueue_first_pre(pgmg_ctx *c, CrossState<T> &st, int np)
{
    const bool dist = is_dist(c, 0);
    if (dist) PGMG_TRY(c->comm->halo(st.gA, c->lv[0], 4, c->s));
    PreArgsT<T> pa = pre_args<T>(c, 0);
    pa.x0 = c->call.x_in != nullptr ? static_cast<const T *>(c->call.x_in) : st.A;
    pa.x2 = st.B;
    if (c->call.x_in != nullptr) pa.Px = c->call.ext_P;
    double *lp = chk_partials(c, np, 0);
    if (lp) pa.partials = lp;
    const int ev = timed_begin(c, 1);
    PGMG_TRY(launch_pre(pa, false, true, c->s));
    PGMG_TRY(timed_end(c, 1, ev));
    if (!lp) {
        FixArgsF fa = fix_args(c, np);
        if (dist) PGMG_TRY(global_sum(c, np, &fa.global_sum));
        launch_pre_fixup(fa, pa, false, c->s);
    }
    st.pr = st.B;
    return PGMG_OK;
}

// a k_postpre block of the finest level; phi, x4 / x2, the partials, sw_adj and recompute are
// the launching step's
template <class T>
static PostPreArgsT<T> postpre_args(const pgmg_ctx *c)
{
    const Level &L = c->lv[0], &C = c->lv[1];
    PostPreArgsT<T> q{};
    q.ec = G<T>(C.A);
    q.f = G<T>(L.F);
    q.rc = G<T>(C.F);
    q.gfx = c->rgfx;
    q.gsy = c->rgsy;
    q.stats = c->stats;
    postpre_geometry(q, L, C);
    q.fast = (c->cfg.flags & PGMG_FLAG_FAST) != 0 && !is_dist(c, 0);
    return q;
}

// a rare path's fix-up block: runs when *cond is set, recomputes without deciding or counting
static FixArgsF forced_fix(const pgmg_ctx *c, int np, const unsigned *cond)
{
    FixArgsF f = fix_args(c, np);
    f.cond = cond;
    f.force = 1;
    f.stats = nullptr;
    return f;
}

// The in-stream step after k_postpre q (calls that decide their checks in-stream): the
// decision into ppflags (on strips from one allreduce of the three sums), then both rare
// paths, each conditional on its flag; they leave the pre-smoothed iterate in nx
template <class T>
static int enqueue_postpre_rare(pgmg_ctx *c, const CrossState<T> &st, const PostPreArgsT<T> &q, T *nx,
                                int np, int npp)
{
    const bool dist = is_dist(c, 0);
    const StripRows sr = strip_rows(c->lv[0], c->lv[1]);
    const double *g3 = nullptr;   // all-rank {post, pre, pre-from-x1} sums
    if (dist) {
        launch_sum_partials(q.partials1, npp, c->scalar, c->s);
        launch_sum_partials(q.partials2, npp, c->scalar + 1, c->s);
        launch_sum_partials(q.partials3, npp, c->scalar + 2, c->s);
        PGMG_TRY(c->comm->allreduce_sum(c->scalar, 3, c->s));
        g3 = c->scalar;
    }
    launch_postpre_decide(q.partials1, q.partials2, q.stats, npp, g3, c->cfg.eps, c->ppflags, c->s);
    // rare path 1 (post check fired): S = x1 of the post-smooth, then a full
    // pre-smooth from S (conditional k_pre + its own fix-up)
    PostArgsT<T> po = post_args<T>(c, 0);
    po.phi = st.pr;
    po.x2 = st.S;
    po.row_lo = sr.x_lo;
    po.row_hi = sr.x_hi;
    launch_post_fixup(forced_fix(c, np, &c->ppflags[0]), po, c->s);
    PreArgsT<T> p1 = pre_args<T>(c, 0);
    p1.x0 = st.S;
    p1.x2 = nx;
    p1.cond = &c->ppflags[0];
    PGMG_TRY(launch_pre(p1, false, false, c->s));
    FixArgsF f1b = fix_args(c, np);
    f1b.cond = &c->ppflags[0];
    f1b.global_sum = dist ? c->scalar + 2 : nullptr;
    launch_pre_fixup(f1b, p1, false, c->s);
    // rare path 2 (only the pre check fired): S = x2 of the post-smooth, then the
    // pre-smooth result is J(S) and rc = R r(J(S))
    PostArgsT<T> p2 = post_args<T>(c, 0);
    p2.phi = st.pr;
    p2.x2 = st.S;
    if (dist) {   // x2 on the strip and 4 rows past it, from the exchanged halos
        p2.row_lo = sr.x_lo;
        p2.row_hi = sr.x_hi;
        p2.fix_sweeps = 2;
        launch_post_fixup(forced_fix(c, np, &c->ppflags[1]), p2, c->s);
    } else {
        p2.cond = &c->ppflags[1];
        p2.stats = nullptr;
        PGMG_TRY(launch_post(p2, false, c->s));
    }
    PreArgsT<T> p3 = pre_args<T>(c, 0);
    p3.x0 = st.S;
    p3.x2 = nx;
    launch_pre_fixup(forced_fix(c, np, &c->ppflags[1]), p3, false, c->s);
    return PGMG_OK;
}

// the solution's buffer becomes L.A (every level-0 grid mirrors the boundary, so any may
// play any role); the other two keep their order as L.B and the scratch
template <class T>
static void set_roles(pgmg_ctx *c, const CrossState<T> &st, const T *sol)
{
    Level &L = c->lv[0];
    L.A = st.grid_of(sol);
    L.B = sol == st.A ? st.gB : st.gA;
    c->S = sol == st.A || sol == st.B ? st.gS : st.gB;
}

// the carry pass (see "The carry" below): x2 (the result) into a grid that is neither the
// input A nor pr (pr is A itself when this one pass also takes the carry); its post check is
// this call's, its pre check the carry's
template <class T>
static int enqueue_carry_pass(pgmg_ctx *c, CrossState<T> &st, int nq)
{
    T *const out = (st.pr == st.B) ? st.S : st.B;
    PostPreArgsT<T> q = postpre_args<T>(c);
    q.phi = st.pr;
    q.x2 = out;
    q.sw_adj = st.sw_adj - 2;   // the pre-smooth's sweeps count in the call that uses them
    q.recompute = st.recompute ? 1 : 0;
    q.partials1 = chk_partials(c, nq, 0);
    q.partials2 = chk_log(c, nq, 0, 0);
    c->call.carry_chk = (int)c->chks.size() - 1;
    if (q.partials1 == nullptr || q.partials2 == nullptr) return set_err(PGMG_ERR_STATE, "carry pass: check log");
    if (pp_sampled(c)) {
        PGMG_TRY(chk_mark_bound(c, 2));
        q.sampled = 1;
        ++c->sampled_n[0];
    }
    const int ev = timed_begin(c, 4);
    PGMG_TRY(launch_postpre(q, c->s));
    PGMG_TRY(timed_end(c, 4, ev));
    st.sw_adj = 0;   // consumed by this pass
    st.recompute = false;
    set_roles(c, st, out);
    c->call.carry_made = true;
    return PGMG_OK;
}

// last cycle: post-smooth into the next buffer, which takes L.A's role, or into the caller's
// array (an external output holds the solution instead; the level-0 grids keep their roles)
template <class T>
static int enqueue_closing_post(pgmg_ctx *c, const CrossState<T> &st, int np)
{
    const bool dist = is_dist(c, 0);
    T *const xout = static_cast<T *>(c->call.x_out);
    T *out = xout != nullptr ? xout : st.next_of(st.pr);
    if (dist) PGMG_TRY(c->comm->halo_end(c->s));
    PostArgsT<T> po = post_args<T>(c, 0);
    po.phi = st.pr;
    po.x2 = out;
    if (xout != nullptr) po.Po = c->call.ext_P;
    po.sw_adj = st.sw_adj;
    double *lp = chk_partials(c, np, 0);
    if (lp) po.partials = lp;
    const int ev = timed_begin(c, 2);
    PGMG_TRY(launch_post(po, true, c->s));
    PGMG_TRY(timed_end(c, 2, ev));
    if (!lp) {
        FixArgsF fa = fix_args(c, np);
        if (dist) PGMG_TRY(global_sum(c, np, &fa.global_sum));
        launch_post_fixup(fa, po, c->s);
    }
    if (xout == nullptr) set_roles(c, st, out);
    return PGMG_OK;
}

// ---------------------------------------------------------------------------
// The carry (r06).  A call's cycles are cross-fused (k_pre, k_postpre ..., k_post), but a
// caller that runs one cycle per call, or checks the residual between calls (the reference
// harness, ParallelTestRunner.cu:172-173), pays the opening k_pre and the closing k_post of
// every call: two passes over the finest grid where a multi-cycle call runs one k_postpre.
// So a speculative V call on the context's own grids (one GPU) ends with the CARRY PASS: the
// last cycle's k_postpre, which stores x2 -- the call's result -- where a k_postpre stores the
// next cycle's pre-smoothed iterate x4, and the next cycle's restricted residual into lv[1].F
// as usual (so it moves the bytes of a k_postpre).  The pre-smooth's early-exit check is
// logged beside the call's own checks and validated with them; it never rolls the call back: a
// carry whose check could fire is dropped (carry_n[2]) and the next call runs its own k_pre.
// The next pgmg_vcycle on the same problem starts from the carry: no k_pre, straight into the
// coarse levels (MultiGrid.hpp:57-94 from line 69 on); its first finest pass is the RECOMPUTE
// FORM of k_postpre, which reads the previous call's x2 (lv[0].A), runs the carried
// pre-smooth again in registers -- the carry pass's own expressions on the same values, so
// bitwise the x4 it did not store -- and goes on as a k_postpre; it counts the carried
// pre-smooth's two sweeps (sw_adj).  A one-cycle call that took the carry and makes the next
// runs one finest pass, both forms at once.  Every entry that changes phi, f, eps, the flags or
// the cycle kind drops the carry (run_cycles takes it or drops it at every call); caller-owned
// arrays (pgmg_set_problem_device) never carry: the caller may change them between calls.  A
// rollback of the call that took a carry reruns from lv[0].A, which no pass of the call writes,
// with its own k_pre.  Cost: none in bytes (the carry pass and the recompute form each move a
// k_postpre's); two more Jacobi stages per point in the recompute form.
// ---------------------------------------------------------------------------
template <class T>
static int enqueue_cross_cycles(pgmg_ctx *c, int n, int gamma)
{
    Level &L = c->lv[0];
    const bool dist = is_dist(c, 0);
    const StripRows sr = strip_rows(L, c->lv[1]);
    const bool lean = c->call.lean;
    const int np = fused_blocks(L.N, sr.jc0, sr.jc1);
    const int npp = postpre_blocks(L.N, sr.jc0, sr.jc1);
    const int npp_rc = postpre_blocks(L.N, sr.jc0, sr.jc1, true);   // the recompute form's
    // the carry: made (the call ends with the carry pass) / taken (it starts from lv[0].A's
    // pre-smooth and lv[1].F, its first finest pass the recompute form -- a k_postpre, so a
    // call of one cycle takes it only when it also makes the next); both only on speculative
    // calls on the context's own grids, one GPU
    const bool make = c->call.carry_make && lean && !dist && c->call.x_out == nullptr && !c->call.defer_post;
    const bool take = c->call.carry_use && lean && !dist && c->call.x_in == nullptr && (n > 1 || make);
    CrossState<T> st{L.A, L.B, c->S, G<T>(L.A), G<T>(L.B), G<T>(c->S), lean, nullptr, take ? 2 : 0, take};
    if (tuning_int("PGMG_ROLE_TRACE", 0))   // measurement build: which grids play which role
        fprintf(stderr, "roles A %p B %p S %p n %d take %d make %d\n", st.gA.base, st.gB.base, st.gS.base, n,
                (int)take, (int)make);
    c->call.carry_use = false;
    c->call.carry_made = false;
    c->call.carry_took = take;
    if (take) st.pr = st.A;
    else PGMG_TRY(enqueue_first_pre(c, st, np));
    PGMG_TRY(enqueue_descend(c, st, gamma));
    for (int k = 1; k < n; ++k) {
        T *nx = st.next_of(st.pr);
        if (dist) PGMG_TRY(c->comm->halo_end(c->s));
        const int nq = st.recompute ? npp_rc : npp;
        PostPreArgsT<T> q = postpre_args<T>(c);
        q.phi = st.pr;
        q.x4 = nx;
        q.sw_adj = st.sw_adj;
        q.recompute = st.recompute ? 1 : 0;
        q.partials1 = lean ? chk_partials(c, nq, 0) : c->partials;
        q.partials2 = lean ? chk_partials(c, nq, 0) : c->partials2;
        q.partials3 = (dist && !lean) ? c->partials3 : nullptr;   // lean: no rare path runs
        if (pp_sampled(c) && q.partials1 != nullptr && q.partials2 != nullptr) {
            PGMG_TRY(chk_mark_bound(c, 2));
            q.sampled = 1;
            ++c->sampled_n[0];
        }
        const int slot = q.recompute ? 5 : 3;   // (the recompute form: its own timed slot)
        const int ev = timed_begin(c, slot);
        PGMG_TRY(launch_postpre(q, c->s));
        PGMG_TRY(timed_end(c, slot, ev));
        st.sw_adj = 0;   // consumed by this pass
        st.recompute = false;
        if (!lean) PGMG_TRY(enqueue_postpre_rare(c, st, q, nx, np, npp));
        st.pr = nx;   // final (after the rare paths)
        PGMG_TRY(enqueue_descend(c, st, gamma));
    }
    if (c->call.defer_post) {   // the last k_post: enqueued by run_cycles_spec after the validation
        c->call.pend_pr = st.pr;
        return PGMG_OK;
    }
    if (make) return enqueue_carry_pass(c, st, st.recompute ? npp_rc : npp);
    if (st.recompute) return set_err(PGMG_ERR_STATE, "a taken carry without a k_postpre");
    return enqueue_closing_post(c, st, np);
}

// MultigridSolver::v_cycle / w_cycle (MultiGrid.hpp:57-136) on level l
template <class T>
static int enqueue_cycle_t(pgmg_ctx *c, int l, int gamma, bool x0_zero)
{
    if (l == c->nb) return enqueue_tail_t<T>(c, gamma, !x0_zero);
    if (c->fused) return enqueue_fused_level_t<T>(c, l, gamma, x0_zero);
    Level &L = c->lv[l];
    Level &C = c->lv[l + 1];
    const bool dist = is_dist(c, l);
    if (dist && l > 0) PGMG_TRY(c->comm->halo(L.F, L, 1, c->s));
    PGMG_TRY(enqueue_smooth_t<T>(c, l, 0, c->cfg.v1, x0_zero));
    if (dist) PGMG_TRY(c->comm->halo(L.A, L, 2, c->s));
    ResRestrictArgsT<T> r{};
    r.x = G<T>(L.A);
    r.f = G<T>(L.F);
    r.rc = G<T>(C.F);
    r.inv_hh = (T)L.ih;
    r.Wf = L.N;
    r.Pf = L.P;
    r.Wc = C.N;
    r.Pc = C.P;
    // coarse rows jc whose centre fine row 2jc this rank owns
    r.jc0 = L.lo / 2 > 1 ? L.lo / 2 : 1;
    r.jc1 = (L.hi + 1) / 2 < C.N - 1 ? (L.hi + 1) / 2 : C.N - 1;
    launch_res_restrict(r, c->s);
    PGMG_TRY(enqueue_children<T>(c, l, gamma));
    if (dist && is_dist(c, l + 1)) PGMG_TRY(c->comm->halo(C.A, C, 2, c->s));
    ProlongArgsT<T> p{};
    p.c = G<T>(C.A);
    p.fine = G<T>(L.A);
    p.Wf = L.N;
    p.Pf = L.P;
    p.Wc = C.N;
    p.Pc = C.P;
    p.row0 = L.u0 > 2 ? L.u0 : 2;
    p.row1 = L.u1 < L.N - 1 ? L.u1 : L.N - 1;
    if (p.row1 > p.row0) launch_prolong(p, c->s);
    return enqueue_smooth_t<T>(c, l, 1, c->cfg.v2, false);
}

int pgmg::enqueue_cycle(pgmg_ctx *c, int l, int gamma, bool x0_zero)
{
    return c->fp32 ? enqueue_cycle_t<float>(c, l, gamma, x0_zero)
                   : enqueue_cycle_t<double>(c, l, gamma, x0_zero);
}

// the last k_post of an in-place call whose speculative checks were validated first (its
// input survives until then): from the pre-smoothed iterate into the caller's phi, its own
// early-exit check decided in-stream
template <class T>
static int enqueue_last_post_t(pgmg_ctx *c)
{
    PostArgsT<T> po = post_args<T>(c, 0);
    po.phi = static_cast<const T *>(c->call.pend_pr);
    po.x2 = static_cast<T *>(c->call.x_out);
    po.Po = c->call.ext_P;
    const int ev = timed_begin(c, 2);
    PGMG_TRY(launch_post(po, true, c->s));
    PGMG_TRY(timed_end(c, 2, ev));
    launch_post_fixup(fix_args(c, fused_blocks(po.N, po.jc0, po.jc1)), po, c->s);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev1, c->s));
    c->call.pend_pr = nullptr;
    return PGMG_OK;
}

int pgmg::enqueue_last_post(pgmg_ctx *c)
{
    return c->fp32 ? enqueue_last_post_t<float>(c) : enqueue_last_post_t<double>(c);
}

// a call's (or a speculative segment's) cycles: graph replay, cross-fused, or cycle by cycle
int pgmg::run_cycles_plain(pgmg_ctx *c, int ncycles, int gamma, bool rec0)
{
    if (rec0) HIPC(hipEventRecord(c->ev0, c->s));
    const bool use_graph = gamma == 1 && !(c->cfg.flags & PGMG_FLAG_NO_GRAPH) &&
                           !(c->cfg.flags & PGMG_FLAG_TIME_FINE) && c->comm == nullptr &&
                           !c->cross;
    if (use_graph && !c->gexec) {
        // first cycle eagerly (sets kernel attributes), the rest from a captured graph
        PGMG_TRY(enqueue_cycle(c, 0, 1, false));
        HIPC(hipGetLastError());
        --ncycles;
        hipGraph_t g = nullptr;
        HIPC(hipStreamBeginCapture(c->s, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue_cycle(c, 0, 1, false);   // (the capture ends on every path)
        hipError_t ce = hipStreamEndCapture(c->s, &g);
        if (rc) return rc;
        if (ce != hipSuccess) return set_err(PGMG_ERR_HIP, std::string("capture: ") + hipGetErrorString(ce));
        HIPC(hipGraphInstantiate(&c->gexec, g, nullptr, nullptr, 0));
        HIPC(hipGraphDestroy(g));
    }
    if (c->cross && !use_graph) {
        PGMG_TRY(c->fp32 ? enqueue_cross_cycles<float>(c, ncycles, gamma)
                         : enqueue_cross_cycles<double>(c, ncycles, gamma));
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(c->ev1, c->s));
        return PGMG_OK;
    }
    for (int k = 0; k < ncycles; ++k) {
        if (use_graph) HIPC(hipGraphLaunch(c->gexec, c->s));
        else PGMG_TRY(enqueue_cycle(c, 0, gamma, false));
    }
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev1, c->s));
    return PGMG_OK;
}
