// pgmg_fcycle.hip — the F-cycle (full multigrid): the FMG h chain's tables, the fused
// smooth(3), one F-cycle's restriction chain and climb, "speculative F-cycles" and
// pgmg_fcycle.  Host code only.
#include <algorithm>
#include <utility>
#include <vector>

#include "pgmg_host.h"

using namespace pgmg;

// h of an N-point grid in the F-cycle's chain: 1/(n_coarse-1) halved once per level
// (MultiGridTestRunner.hpp:195, MultiGrid.hpp:171) — differs from a/(N-1) when a != 1
static double fmg_h(const pgmg_config &cfg, int N)
{
    double h = 1.0 / (cfg.n_coarse - 1);
    for (int n = cfg.n_coarse; n < N; n = 2 * n - 1) h /= 2;
    return h;
}

// sine tables of every level the F-cycle visits: bulk 0..nb-1, then the tail levels
static int fmg_tables(pgmg_ctx *c)
{
    if (c->fmg_tab) return PGMG_OK;
    std::vector<int> Ns;
    for (int l = 0; l < c->nb; ++l) Ns.push_back(c->lv[l].N);
    for (int N = c->lv[c->nb].N;; N = (N - 1) / 2 + 1) {
        Ns.push_back(N);
        if (N <= c->cfg.n_coarse) break;
    }
    std::vector<double> tab;
    c->fmg_off.clear();
    for (int N : Ns) {
        std::vector<double> sx, sy;
        double factor;
        sine_tables(c->cfg, N, fmg_h(c->cfg, N), sx, sy, factor);
        c->fmg_off.push_back((int)tab.size());
        tab.insert(tab.end(), sx.begin(), sx.end());
        tab.insert(tab.end(), sy.begin(), sy.end());
    }
    HIPC(hipMalloc((void **)&c->fmg_tab, tab.size() * sizeof(double)));
    HIPC(hipMemcpy(c->fmg_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    // the RHS of the FMG chain on every bulk level, regenerated in that level's passes like
    // set_problem's level-0 RHS: per level [8 | factor*sx (N) | 1024 | 8 | sy (N) | 16]
    if (c->nb > 0) {
        std::vector<double> g;
        c->fmg_goff.assign(c->nb, 0);
        for (int l = 0; l < c->nb; ++l) {
            const int N = c->lv[l].N;
            std::vector<double> sx, sy;
            double factor;
            sine_tables(c->cfg, N, fmg_h(c->cfg, N), sx, sy, factor);
            const size_t o = g.size(), nx = 8 + N + 1024, ny = 8 + N + 16;
            c->fmg_goff[l] = o;
            g.resize(o + nx + ny, 0.0);
            for (int i = 0; i < N; ++i) g[o + 8 + i] = factor * sx[i];
            for (int j = 0; j < N; ++j) g[o + nx + 8 + j] = sy[j];
        }
        HIPC(hipMalloc((void **)&c->fmg_gtab, g.size() * sizeof(double)));
        HIPC(hipMemcpy(c->fmg_gtab, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return PGMG_OK;
}

// smooth(3) of the F-cycle climb (MultiGrid.hpp:153) on a bulk level, fused: four sweeps in
// one pass into L.B with the three checks summed speculatively, the decision, the exact
// rare path (x_k from the untouched x0), then L.A and L.B trade places (both frames zero)
template <class T>
static int enqueue_smooth3_fused(pgmg_ctx *c, int l)
{
    Level &L = c->lv[l];
    const bool dist = is_dist(c, l);
    int e;
    // x0 is read 6 rows past the strip (the pass's pipeline), f is local (analytic)
    if (dist && (e = c->comm->halo(L.A, L, 6, c->s))) return e;
    PostPreArgsT<T> q{};
    q.phi = G<T>(L.A);
    q.f = G<T>(L.F);
    q.x4 = G<T>(L.B);
    q.gfx = l == c->call.gen_level ? c->call.lgfx : nullptr;   // the climb's level: f regenerated
    q.gsy = l == c->call.gen_level ? c->call.lgsy : nullptr;
    q.partials1 = c->partials;
    q.partials2 = c->partials2;
    q.partials3 = c->partials3;
    postpre_geometry(q, L, c->lv[l + 1]);
    q.rc_lo = 1;   // (nothing is restricted)
    q.rc_hi = 1;
    const int np = postpre_blocks(L.N, q.jc0, q.jc1);
    if (c->call.lean && c->call.fspec) {
        // speculative F-cycles: the three checks recorded "does not fire" (the pass books its
        // four sweeps), no decision or rare-path launch
        q.partials1 = chk_log(c, np, l, 0);
        q.partials2 = chk_log(c, np, l, 0);
        q.partials3 = chk_log(c, np, l, 0);
        q.stats = c->stats;
        if ((e = launch_smooth4(q, c->s))) return e;
        std::swap(L.A, L.B);
        c->fsmooth_swapped = true;
        return PGMG_OK;
    }
    if ((e = launch_smooth4(q, c->s))) return e;
    const double *g3 = nullptr;
    if (dist) {
        launch_sum_partials(q.partials1, np, c->scalar, c->s);
        launch_sum_partials(q.partials2, np, c->scalar + 1, c->s);
        launch_sum_partials(q.partials3, np, c->scalar + 2, c->s);
        if ((e = c->comm->allreduce_sum(c->scalar, 3, c->s))) return e;
        g3 = c->scalar;
    }
    launch_smooth4_finish(q, np, g3, c->cfg.eps, c->ppflags, c->stats, c->s);
    std::swap(L.A, L.B);
    c->fsmooth_swapped = true;
    return PGMG_OK;
}

// One level of the climb, while it is enqueued: its cached analytic RHS of the FMG chain
// (Ffmg_l[l]; level 0's is traded by pgmg_fcycle) stands in for L.F, and its passes regenerate
// that f in-kernel from the level's tables (bitwise the stored one; its rare paths and the
// coarser levels read theirs from memory; PGMG_FLAG_STORED_RHS: rgfx is null, every level
// streams its RHS).  Both are undone when the level is left, error returns included.
struct ClimbLevel {
    pgmg_ctx *c;
    int l;
    ClimbLevel(pgmg_ctx *c_, int l_) : c(c_), l(l_)
    {
        if (l > 0) std::swap(c->lv[l].F, c->Ffmg_l[l]);
        if (l == 0 || c->rgfx == nullptr) return;
        c->call.gen_level = l;
        c->call.lgfx = c->fmg_gtab + c->fmg_goff[l] + 8;
        c->call.lgsy = c->fmg_gtab + c->fmg_goff[l] + (8 + c->lv[l].N + 1024) + 8;
    }
    ~ClimbLevel()
    {
        c->call.gen_level = 0;
        c->call.lgfx = c->call.lgsy = nullptr;
        if (l > 0) std::swap(c->lv[l].F, c->Ffmg_l[l]);
    }
};

// One outer F-cycle (MultiGridTestRunner.hpp:192-205 -> MultigridSolver::f_cycle,
// MultiGrid.hpp:138-183) on the current solution A_0:
//   restrict phi to n_coarse (compute_coarsest_grid); then from the coarsest level up:
//   smooth(3); phi_fine = 0 + P phi; f_fine = analytic RHS; one V-cycle on the finer level.
// The levels at or below the tail's top run inside one k_tail launch; the bulk levels use
// the V-cycle kernels with the level's F replaced by the analytic RHS of the FMG chain.
// opt: kFSaveTop -- keep a copy of the tail top's restricted grid (a speculative call's first
// F-cycle); kFFromTop -- skip the restriction, start the climb from that copy (its rerun);
// kFR2Next -- another F-cycle follows: the finest k_post forms level 2's restriction
// (k_post_r2); kFR2Done -- the previous F-cycle did: start the restriction at level 2
constexpr int kFSaveTop = 1, kFFromTop = 2, kFR2Next = 4, kFR2Done = 8;

template <class T>
static int enqueue_fcycle(pgmg_ctx *c, int opt = 0)
{
    const int nb = c->nb;
    double factor;
    {
        std::vector<double> sx, sy;
        sine_tables(c->cfg, 1, 1.0, sx, sy, factor);
    }
    int e;
    const bool use_r2 = !(c->cfg.flags & PGMG_FLAG_NO_R2);   // two restriction steps per pass
    if (opt & kFFromTop)
        HIPC(hipMemcpyAsync(c->lv[nb].A.base, c->ftop.base, c->ftop.bytes, hipMemcpyDeviceToDevice, c->s));
    // level 2's values already formed by the previous F-cycle's finest k_post (k_post_r2:
    // the pair 0 -> 2 below, bitwise)
    const bool from2 = (opt & kFR2Done) && c->call.fr2_made && use_r2 && nb >= 2 && !is_dist(c, 0) &&
                       !is_dist(c, 1);
    c->call.fr2_made = false;   // (consumed; set again by this cycle's finest k_post_r2)
    for (int l = (opt & kFFromTop) ? nb : (from2 ? 2 : 0); l < nb; ++l) {
        Level &L = c->lv[l], &C = c->lv[l + 1];
        if (!is_dist(c, l)) {
            // the intermediate level's restricted values are dead (the climb overwrites that
            // level's grid before reading it), so two levels go in one pass
            if (use_r2 && l + 2 <= nb && !is_dist(c, l + 1)) {
                const Level &C2 = c->lv[l + 2];
                launch_restrict2_values(G<T>(L.A), L.P, G<T>(C2.A), C2.N, C2.P, c->s);
                ++l;
                continue;
            }
            launch_restrict_values(G<T>(L.A), L.N, L.P, G<T>(C.A), C.N, C.P, c->s);
            continue;
        }
        // row strips: the rank's coarse rows from its fine rows and one halo row each side
        const StripRows sr = strip_rows(L, C);
        if ((e = c->comm->halo(L.A, L, 1, c->s))) return e;
        launch_restrict_values(G<T>(L.A), L.N, L.P, G<T>(C.A), C.N, C.P, c->s, sr.rc_lo, sr.rc_hi);
        // first replicated level: every rank's rows to every rank
        if (!is_dist(c, l + 1) && (e = c->comm->allgather_rows(c, l + 1, C.A))) return e;
    }
    if (opt & kFSaveTop)
        HIPC(hipMemcpyAsync(c->ftop.base, c->lv[nb].A.base, c->ftop.bytes, hipMemcpyDeviceToDevice, c->s));
    {
        TailArgsT<T> t = tail_args<T>(c);
        t.x0_from_global = 1;
        t.fmg = 1;
        t.fmg_smooth_top = nb > 0 ? 1 : 0;
        t.fmg_tab = c->fmg_tab;
        for (int k = 0; k < 8 && nb + k < (int)c->fmg_off.size(); ++k)
            t.fmg_tab_off[k] = c->fmg_off[nb + k];
        t.fmg_factor = factor;
        HIPC(launch_tail_gamma(t, 1, c->s));
    }
    for (int l = nb - 1; l >= 0; --l) {
        Level &L = c->lv[l];
        Level &C = c->lv[l + 1];
        const double *sx = c->fmg_tab + c->fmg_off[l];
        const bool dist = is_dist(c, l);
        // rows this rank holds: all, or (row strips) its strip and the halo rows, where the
        // analytic RHS is computed locally instead of exchanged
        const int r0 = dist ? std::max(0, L.lo - kHalo) : 0;
        const int r1 = dist ? std::min(L.N, L.hi + kHalo) : L.N;
        // the level's analytic RHS of the FMG h chain is the same on every call: computed
        // once into its own grid (Ffmg for level 0, Ffmg_l[l] below), which stands in for
        // L.F while this level runs (the V-cycle's restriction writes the coarser level's
        // own F, not its cached RHS)
        const ClimbLevel climb(c, l);
        if (!c->fmg_rhs_ready)
            launch_rhs(G<T>(L.F), sx, sx + L.N, factor, L.N, L.P, r0, r1, c->s);
        // phi_fine = 0 + P phi_coarse (MultiGrid.hpp:159-164): the prolongation assigns the
        // interior, the frame (boundary, and row/column 1 the reference never corrects) is
        // zeroed; the ping-pong buffer's frame mirrors it
        launch_zero_frame(G<T>(L.A), L.P, L.N, c->s, r0, r1);
        launch_zero_frame(G<T>(L.B), L.P, L.N, c->s, r0, r1);
        if (l == 0 && c->S.base) launch_zero_frame(G<T>(c->S), L.P, L.N, c->s, r0, r1);   // S mirrors too
        const bool use_pin = !(c->cfg.flags & PGMG_FLAG_NO_PIN);
        if (c->fused && use_pin) {
            // the V-cycle's k_pre computes the prolongation on the fly (PIN): no separate
            // pass writing the zeroed fine grid; it reads 3 coarse rows past the strip
            if (dist && is_dist(c, l + 1) && (e = c->comm->halo(C.A, C, 3, c->s))) return e;
            const bool fr2_want = l == 0 && (opt & kFR2Next) && use_r2;
            if ((e = enqueue_fused_level(c, l, 1, false, true, fr2_want))) return e;
            if (l > 0 && (e = enqueue_smooth3_fused<T>(c, l))) return e;
            continue;
        }
        // the prolongation of the rank's rows reads one coarse row past its strip
        if (dist && is_dist(c, l + 1) && (e = c->comm->halo(C.A, C, 1, c->s))) return e;
        ProlongArgsT<T> p{};
        p.c = G<T>(C.A);
        p.fine = G<T>(L.A);
        p.Wf = L.N;
        p.Pf = L.P;
        p.Wc = C.N;
        p.Pc = C.P;
        p.row0 = dist ? std::max(L.u0, 2) : 2;
        p.row1 = dist ? std::min(L.u1, L.N - 1) : L.N - 1;
        p.assign = 1;
        if (p.row1 > p.row0) launch_prolong(p, c->s);
        if ((e = enqueue_cycle(c, l, 1, false))) return e;
        // the V-cycle above regenerated this level's f where its passes are fused; the
        // general smooth(3) below streams the cached RHS
        if (l > 0 && (e = enqueue_smooth(c, l, 0, 3, false))) return e;
    }
    return PGMG_OK;
}

// Speculative F-cycles (one GPU).  The climb's V-cycles and smooth(3) passes decide their
// early-exit checks in-stream by default: a decision launch after every bulk pass and every
// fused smooth(3), ~86 launches of ~5 us per F-cycle at N = 16385 (9 % of it), while on the
// reference problem no bulk check of an F-cycle fires (the F goldens: 0 exits).  A call of F
// cycles is therefore enqueued with every bulk check recorded "does not fire" (the V-cycles'
// mode 0; smooth(3)'s three checks too, its pass booking the four sweeps) and validated once
// after the call, like the V-cycles' speculative calls.  A rollback needs no copy of the
// level-0 solution: an F-cycle reads phi only through the restriction chain, whose one live
// result is the tail top's grid (the intermediate levels' values are dead, the climb
// overwrites them), so the first F-cycle's tail-top grid is kept (kFSaveTop) and the rerun --
// every F-cycle of the call decided in-stream, bitwise the in-stream call -- starts its first
// climb from it (kFFromTop).  The level buffers the smooth(3) passes swap and the statistics
// are restored first.  A rolled-back problem keeps its F-cycles in-stream (fspec_off).
template <class T>
static int run_fcycles_spec(pgmg_ctx *c, int ncycles)
{
    const int nb = c->nb;
    // log: per F-cycle, every climb level's V-cycle (the level and all below it) and the three
    // smooth(3) checks of the levels below the finest
    long long dbl = 64, nchk = 4;
    for (int l = 0; l < nb; ++l) {
        long long d, k;
        spec_need_level(c, l, 1, &d, &k);
        dbl += (long long)ncycles * d;
        nchk += (long long)ncycles * k;
        if (l == 0) {   // the finest k_post as k_post_r2 (more workgroups than k_post)
            const Level &L = c->lv[0];
            dbl += (long long)ncycles * post_r2_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2);
        }
        if (l > 0) {
            const Level &L = c->lv[l];
            dbl += 3LL * ncycles * postpre_blocks(L.N, L.lo / 2, (L.hi < L.N ? L.hi : L.N - 1) / 2);
            nchk += 3LL * ncycles;
        }
    }
    int e = spec_reserve(c, dbl, nchk);
    if (e) return e;
    if (!c->ftop.base && (e = alloc_grid(c->ftop, c->lv[nb]))) return e;
    std::vector<Grid> A0(nb + 1), B0(nb + 1);
    for (int l = 0; l <= nb; ++l) {
        A0[l] = c->lv[l].A;
        B0[l] = c->lv[l].B;
    }
    // stats backup + the coarse levels' "pre-smooth fired" flags (written by the skipped rare
    // paths) = 0
    launch_spec_open(c->stats, c->stats_bk, c->flags, (int)(c->lv.size() + 1) * 2 * kMaxSweeps, c->s);
    c->call.lean = true;
    c->call.fspec = true;
    c->call.spec_gamma = 1;
    c->plog_used = 0;
    c->chks.clear();
    c->chk_visit.clear();
    for (int k = 0; k < ncycles && !e; ++k) {
        // consecutive F-cycles: the finest k_post of one forms the next one's level 2
        const int opt = (k == 0 ? kFSaveTop : kFR2Done) | (k + 1 < ncycles ? kFR2Next : 0);
        e = enqueue_fcycle<T>(c, opt);
        if (!e) c->fmg_rhs_ready = true;
    }
    c->call.lean = false;   // (a rollback's rerun below is in-stream)
    c->call.fspec = false;
    if (e) return e;
    unsigned h = 0;
    bool overflow = false;
    if ((e = spec_validate(c, &h, &overflow, (int)c->chks.size()))) return e;
    if (!h) return PGMG_OK;
    ++c->rollbacks;
    c->hist.fspec_off = true;
    for (int l = 0; l <= nb; ++l) {
        c->lv[l].A = A0[l];
        c->lv[l].B = B0[l];
    }
    HIPC(hipMemcpyAsync(c->stats, c->stats_bk, 4 * sizeof(unsigned long long),
                        hipMemcpyDeviceToDevice, c->s));
    // (in-stream: no k_post_r2, every F-cycle restricts from level 0)
    for (int k = 0; k < ncycles && !e; ++k) e = enqueue_fcycle<T>(c, k == 0 ? kFFromTop : 0);
    return e;
}

extern "C" {

int pgmg_fcycle(pgmg_ctx *c, int ncycles)
{
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (ncycles <= 0) return PGMG_OK;
    c->carry = false;   // an F-cycle starts from phi itself
    int e = fmg_tables(c);
    if (e) return e;
    Level &L0 = c->lv[0];
    if (c->nb > 0 && !c->Ffmg.base && (e = alloc_grid(c->Ffmg, L0))) return e;
    if ((int)c->Ffmg_l.size() < c->nb) {
        c->Ffmg_l.resize(c->nb);
        for (int l = 1; l < c->nb; ++l)
            if ((e = alloc_grid(c->Ffmg_l[l], c->lv[l]))) return e;
    }
    // the F-cycle's levels use the FMG h chain and (level 0) the analytic RHS of that chain
    // (every level including the tail's top, whose h enqueue_tail passes on).  Everything
    // the F-cycle changes on the context is undone by the guard on EVERY exit path (an
    // error half-way through the climb included), so later V/W-cycles see the user's f,
    // h and no regenerated-RHS level (the climb's own level: ClimbLevel; the call state:
    // CallScope).
    const CallScope scope{c};
    struct Restore {
        pgmg_ctx *c;
        std::vector<Level> saved;
        const double *sgx, *sgy;
        bool f0_swapped = false;
        ~Restore()
        {
            if (f0_swapped) std::swap(c->lv[0].F, c->Ffmg);
            c->rgfx = sgx;
            c->rgsy = sgy;
            for (int l = 0; l <= c->nb; ++l) {
                c->lv[l].h = saved[l].h;
                c->lv[l].hh = saved[l].hh;
                c->lv[l].ih = saved[l].ih;
            }
        }
    } guard{c, c->lv, c->rgfx, c->rgsy};
    for (int l = 0; l <= c->nb; ++l) {
        Level &L = c->lv[l];
        const double h = fmg_h(c->cfg, L.N);
        L.h = h;
        L.hh = h * h;
        L.ih = 1.0 / (h * h);
    }
    if (c->nb > 0) {
        std::swap(L0.F, c->Ffmg);
        guard.f0_swapped = true;
    }
    const bool gen = c->nb > 0 && !(c->cfg.flags & PGMG_FLAG_STORED_RHS);
    c->rgfx = gen ? c->fmg_gtab + 8 : nullptr;
    c->rgsy = gen ? c->fmg_gtab + (8 + L0.N + 1024) + 8 : nullptr;
    // a device-bound problem (pgmg_set_problem_device): the F-cycle restricts and climbs on
    // the level-0 grids, so the caller's phi is staged into L.A first (after in-place V/W
    // calls L.A is stale: those calls read and write the caller's array) and the result is
    // copied back; synchronous, like the V/W calls on a bound problem
    const bool ext = c->ext_phi != nullptr;
    if (ext) PGMG_TRY(ext_stage_in(c, false));
    HIPC(hipEventRecord(c->ev0, c->s));
    // speculative F-cycles: one GPU, the fused climb (PIN), not EXACT_DIST, not after a rollback
    const bool fspec = c->nb > 0 && c->fused && c->comm == nullptr && !c->hist.fspec_off &&
                       !(c->cfg.flags & (PGMG_FLAG_EXACT_DIST | PGMG_FLAG_NO_PIN));
    if (fspec) {
        e = c->fp32 ? run_fcycles_spec<float>(c, ncycles) : run_fcycles_spec<double>(c, ncycles);
    } else {
        for (int k = 0; k < ncycles && !e; ++k) {
            e = c->fp32 ? enqueue_fcycle<float>(c) : enqueue_fcycle<double>(c);
            if (!e) c->fmg_rhs_ready = true;
        }
    }
    if (c->fsmooth_swapped && c->gexec) {   // its level buffers traded places: recapture
        PGMG_TRY(stream_wait(c));
        HIPC(hipGraphExecDestroy(c->gexec));
        c->gexec = nullptr;
    }
    c->fsmooth_swapped = false;
    if (e) return e;
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev1, c->s));
    if (ext) {
        PGMG_TRY(ext_stage_out(c));
        PGMG_TRY(stream_wait(c));
    }
    return PGMG_OK;
}

}  // extern "C"
