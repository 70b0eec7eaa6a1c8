// pgmg_gradient.hip — the field of the solution (include/pgmg.h "Gradient of the solution";
// DESIGN.md §4e): k_gradient, the reduction of its partial sums, pgmg_gradient and
// pgmg_gradient_time (pgmg_gradient_grid, on the caller's arrays: pgmg_ops.hip).
//
// One streaming pass over phi, read where it lies, that writes both components of
// scale * grad(phi) on all N x N points, frame included, as doubles at pitch N, by the second- or
// fourth-order central differences and one-sided differences of the same order on the frame (and,
// at order 4, next to it).  Shaped like the monitor's pass (pgmg_monitor.hip): lane t of a wave
// owns the column pair (1 + 2t, 2 + 2t) -- column 0 rides with the lane that owns column 1 -- a
// workgroup marches down a band of rows keeping a window of rows in registers for the y stencil
// (2 rows at order 2, 4 at order 4; kGradU more are loaded before the first is used), and the x
// neighbours at +-1 and +-2 are the neighbouring lanes' pairs, moved by DPP; lanes 0 and 63 load
// their halo pair, and the lane that owns columns N-2 and N-1 the one value its one-sided
// formulas reach past its left neighbour for.  The one-sided columns are a second expression in
// the waves that hold them (wave-uniform), the one-sided rows a branch on the row (uniform over
// the workgroup) that loads the rows of its stencil again -- four rows of the whole grid.
//
// The norm sqrt(sum gx^2 + gy^2) follows the monitor's scheme: every lane adds its terms in row
// order, the lanes of a wave in wave_sum's tree, the four waves in index order, the workgroups'
// partials with plain stores, added in index order by k_grad_reduce.  The decomposition (tiles of
// 512 columns, bands of grad_grid(N).band rows) is a function of N alone.
#include <cmath>
#include <string>

#include "pgmg_grad_dev.h"
#include "pgmg_host.h"

using namespace pgmg;

namespace pgmg {

template <class SX>
struct GradArgs {
    const SX *x;         // element (0, 0) of phi, pitch Px
    long long Px;
    double *gx, *gy;     // element (0, 0) of the outputs, pitch N; either may be null
    double *partials;    // one per workgroup, or null
    double w;            // scale * 0.5 / h (order 2), scale / (12 h) (order 4)
    int N;
    int band;            // rows per workgroup
};

// (kGradU and the one-sided line formulas os2_* / os4_*: pgmg_grad_dev.h)
template <class T, class SX, int ORDER>
__global__ __launch_bounds__(kBlock) void k_gradient(GradArgs<SX> a)
{
    static_assert(ORDER == 2 || ORDER == 4, "second or fourth order");
    constexpr int H = ORDER / 2;    // rows the central y stencil reaches either way
    constexpr int NR = ORDER + 1;   // points of a one-sided stencil
    static_assert(kGradU >= 2 * H, "the window is the tail of an iteration's rows");
    using D2 = V2<T>;
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
    const bool edge_wave = p0 == 0 || npairs <= p0 + 64;   // holds a one-sided column
    // the two values a lane loads beside its pair: lane 0 the pair to its left (column 0 twice
    // for the first lane), lane 63 the pair to its right, the last lane column N-1-ORDER
    const bool edge = act && (lane == 0 || lane == 63 || lastl);
    const int ix = lastl ? N - 1 - ORDER : (lane == 0 ? max(c - 2, 0) : min(c + 2, N - 1));
    const int iy = lastl ? N - 1 - ORDER : (lane == 0 ? c - 1 : min(c + 3, N - 1));
    const long long Px = a.Px;
    const SX *__restrict__ X = a.x;
    const T w = (T)a.w;
    const T k8 = T(8);
    double acc = 0.0;

    struct Row {
        D2 o;       // the lane's pair
        T hx, hy;   // the edge lanes' two values
    };
    auto load_row = [&](int r) -> Row {
        const SX *p = X + r * Px;
        Row v;
        const V2<SX> q = ldvu<SX>(p + cl);
        v.o = mk2<T>((T)q.x, (T)q.y);
        v.hx = v.hy = T(0);
        if (edge) {
            v.hx = (T)p[ix];
            v.hy = (T)p[iy];
        }
        return v;
    };
    // d/dx on the lane's pair of a row, and (g0, the first lane's) on column 0.  The moves are
    // unconditional: every lane of the wave is active here
    auto xgrad = [&](const Row &ce, T &g0) -> D2 {
        D2 l = mk2<T>(dpp_shr(ce.o.x), dpp_shr(ce.o.y));
        D2 r = mk2<T>(dpp_shl(ce.o.x), dpp_shl(ce.o.y));
        if (lane == 0) l = mk2<T>(ce.hx, ce.hy);
        if (lane == 63) r = mk2<T>(ce.hx, ce.hy);
        D2 g;
        g0 = T(0);
        if constexpr (ORDER == 4) {
            g.x = (k8 * (ce.o.y - l.y) - (r.x - l.x)) * w;
            g.y = (k8 * (r.x - ce.o.x) - (r.y - l.y)) * w;
            if (edge_wave) {
                // the first lane: columns 0 .. 4 are l.y, its pair and r; the last: columns
                // N-5 .. N-1 are hx, l and its pair
                const T f0 = os4_first(l.y, ce.o.x, ce.o.y, r.x, r.y) * w;
                const T f1 = os4_second(l.y, ce.o.x, ce.o.y, r.x, r.y) * w;
                const T e1 = os4_penult(ce.hx, l.x, l.y, ce.o.x, ce.o.y) * w;
                const T e0 = os4_last(ce.hx, l.x, l.y, ce.o.x, ce.o.y) * w;
                g0 = f0;
                g.x = firstl ? f1 : (lastl ? e1 : g.x);
                g.y = lastl ? e0 : g.y;
            }
        } else {
            g.x = (ce.o.y - l.y) * w;
            g.y = (r.x - ce.o.x) * w;
            if (edge_wave) {
                const T f0 = os2_first(l.y, ce.o.x, ce.o.y) * w;
                const T e0 = os2_last(l.y, ce.o.x, ce.o.y) * w;
                g0 = f0;
                g.y = lastl ? e0 : g.y;
            }
        }
        return g;
    };
    // one output row: both components on the lane's pair (and column 0), stored and summed
    auto emit = [&](int r, D2 gx, T gx0, D2 gy, T gy0) {
        if (!act) return;
        const long long at = (long long)r * N + c;
        if (a.gx != nullptr) {
            stvu<double>(a.gx + at, mk2<double>((double)gx.x, (double)gx.y));
            acc += sq(gx.x);
            acc += sq(gx.y);
            if (firstl) {
                a.gx[at - 1] = (double)gx0;
                acc += sq(gx0);
            }
        }
        if (a.gy != nullptr) {
            stvu<double>(a.gy + at, mk2<double>((double)gy.x, (double)gy.y));
            acc += sq(gy.x);
            acc += sq(gy.y);
            if (firstl) {
                a.gy[at - 1] = (double)gy0;
                acc += sq(gy0);
            }
        }
    };

    // (wave-uniform; a wave past the last column only joins the block sum)
    if (nw > 0) {
        const int jb = blockIdx.y * a.band;
        const int je = min(jb + a.band, N);
        // s[0 .. 2H-1]: the window, rows j-H .. j+H-1; s[2H ..]: this iteration's loads.  Rows
        // are clamped into the grid: a clamped row only feeds a row outside the grid or a
        // one-sided row, which takes its own
        Row s[2 * H + kGradU];
        #pragma unroll
        for (int k = 0; k < 2 * H; ++k) s[k] = load_row(min(max(jb - H + k, 0), N - 1));
        for (int j = jb; j < je; j += kGradU) {
            #pragma unroll
            for (int u = 0; u < kGradU; ++u) s[2 * H + u] = load_row(min(j + u + H, N - 1));
            #pragma unroll
            for (int u = 0; u < kGradU; ++u) {
                const int r = j + u;   // this step's row (uniform over the workgroup)
                T gx0;
                const D2 gx = xgrad(s[u + H], gx0);
                if (r < je) {
                    D2 gy;
                    T gy0;
                    if (r < H || r > N - 1 - H) {
                        Row q[NR];
                        const int base = r < H ? 0 : N - 1 - ORDER;
                        #pragma unroll
                        for (int k = 0; k < NR; ++k) q[k] = load_row(base + k);
                        if constexpr (ORDER == 4) {
                            if (r == 0) {
                                gy.x = os4_first(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
                                gy.y = os4_first(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
                                gy0 = os4_first(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
                            } else if (r == 1) {
                                gy.x = os4_second(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
                                gy.y = os4_second(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
                                gy0 = os4_second(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
                            } else if (r == N - 2) {
                                gy.x = os4_penult(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
                                gy.y = os4_penult(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
                                gy0 = os4_penult(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
                            } else {
                                gy.x = os4_last(q[0].o.x, q[1].o.x, q[2].o.x, q[3].o.x, q[4].o.x) * w;
                                gy.y = os4_last(q[0].o.y, q[1].o.y, q[2].o.y, q[3].o.y, q[4].o.y) * w;
                                gy0 = os4_last(q[0].hy, q[1].hy, q[2].hy, q[3].hy, q[4].hy) * w;
                            }
                        } else {
                            if (r == 0) {
                                gy.x = os2_first(q[0].o.x, q[1].o.x, q[2].o.x) * w;
                                gy.y = os2_first(q[0].o.y, q[1].o.y, q[2].o.y) * w;
                                gy0 = os2_first(q[0].hy, q[1].hy, q[2].hy) * w;
                            } else {
                                gy.x = os2_last(q[0].o.x, q[1].o.x, q[2].o.x) * w;
                                gy.y = os2_last(q[0].o.y, q[1].o.y, q[2].o.y) * w;
                                gy0 = os2_last(q[0].hy, q[1].hy, q[2].hy) * w;
                            }
                        }
                    } else if constexpr (ORDER == 4) {
                        const Row &m2 = s[u], &m1 = s[u + 1], &q1 = s[u + 3], &q2 = s[u + 4];
                        gy.x = (k8 * (q1.o.x - m1.o.x) - (q2.o.x - m2.o.x)) * w;
                        gy.y = (k8 * (q1.o.y - m1.o.y) - (q2.o.y - m2.o.y)) * w;
                        gy0 = (k8 * (q1.hy - m1.hy) - (q2.hy - m2.hy)) * w;
                    } else {
                        const Row &m1 = s[u], &q1 = s[u + 2];
                        gy.x = (q1.o.x - m1.o.x) * w;
                        gy.y = (q1.o.y - m1.o.y) * w;
                        gy0 = (q1.hy - m1.hy) * w;
                    }
                    emit(r, gx, gx0, gy, gy0);
                }
            }
            #pragma unroll
            for (int k = 0; k < 2 * H; ++k) s[k] = s[kGradU + k];
        }
    }
    if (a.partials == nullptr) return;   // (uniform over the grid)
    const double sw = wave_sum(acc);
    if (lane == 0) red[wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        #pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) t += red[k];
        a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// out[0] = the sum of the np workgroups' partials, in a fixed order (k_mon_reduce's)
__global__ __launch_bounds__(kBlock) void k_grad_reduce(const double *partials, int np, double *out)
{
    __shared__ double red[kBlock / 64];
    double s = 0.0;
    for (int k = threadIdx.x; k < np; k += kBlock) s += partials[k];
    const double v = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        #pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) t += red[k];
        out[0] = t;
    }
}

// 256 pairs per workgroup in x; bands of 64 rows, shorter while the grid has fewer than ~1024
// workgroups (k_extrap_add's rule).  A function of N alone: the partial sums depend on it
GradGrid grad_grid(int N)
{
    GradGrid g;
    g.tiles = ((N - 1) / 2 + kBlock - 1) / kBlock;
    g.band = 64;
    while (g.band > 8 && g.tiles * ((N + g.band - 1) / g.band) < 1024) g.band /= 2;
    g.bands = (N + g.band - 1) / g.band;
    return g;
}
int gradient_blocks(int N)
{
    const GradGrid g = grad_grid(N);
    return g.tiles * g.bands;
}

void launch_grad_reduce(const double *partials, int np, double *sum, hipStream_t s)
{
    k_grad_reduce<<<dim3(1), dim3(kBlock), 0, s>>>(partials, np, sum);
}

template <class T, class SX>
void launch_gradient(const SX *x, long long Px, double *gx, double *gy, int N, double w, int order,
                     double *partials, double *sum, hipStream_t s)
{
    const GradGrid g = grad_grid(N);
    GradArgs<SX> a{};
    a.x = x;
    a.Px = Px;
    a.gx = gx;
    a.gy = gy;
    a.partials = sum != nullptr ? partials : nullptr;
    a.w = w;
    a.N = N;
    a.band = g.band;
    const dim3 grid(g.tiles, g.bands);
    if (order == 4) k_gradient<T, SX, 4><<<grid, dim3(kBlock), 0, s>>>(a);
    else k_gradient<T, SX, 2><<<grid, dim3(kBlock), 0, s>>>(a);
    if (sum != nullptr) launch_grad_reduce(partials, g.tiles * g.bands, sum, s);
}
template void launch_gradient<double, double>(const double *, long long, double *, double *, int,
                                              double, int, double *, double *, hipStream_t);

// scale * 0.5 / h and scale / (12.0 * h), in double, left to right
double gradient_weight(int order, double scale, double h)
{
    return order == 4 ? scale / (12.0 * h) : scale * 0.5 / h;
}

// [p, p + n) and [q, q + m) share a byte
bool ranges_overlap(const void *p, size_t n, const void *q, size_t m)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + m && b < a + n;
}
// an output of N * N doubles: device memory from its first byte to its last
bool device_range(const double *p, int N)
{
    return is_device_ptr(p) && is_device_ptr(p + (size_t)N * N - 1);
}
// what pgmg_gradient_grid and pgmg_gradient refuse in their arrays (nullptr: nothing); phi: the
// bytes the pass reads, [phi, phi + phi_bytes)
const char *gradient_arrays_error(const void *phi, size_t phi_bytes, const double *gx,
                                  const double *gy, int N)
{
    const size_t bytes = (size_t)N * N * sizeof(double);
    if (!gx && !gy) return "both outputs are null";
    if ((gx && !device_range(gx, N)) || (gy && !device_range(gy, N)))
        return "an output is not device memory";
    if (gx && gy && ranges_overlap(gx, bytes, gy, bytes)) return "the outputs overlap";
    if ((gx && ranges_overlap(gx, bytes, phi, phi_bytes)) ||
        (gy && ranges_overlap(gy, bytes, phi, phi_bytes)))
        return "an output overlaps phi";
    return nullptr;
}

// the context's partial sums (np workgroups, then the total)
int grad_reserve(pgmg_ctx *c, int np)
{
    if (np <= c->grad_cap) return PGMG_OK;
    if (c->grad_buf) HIPC(hipFree(c->grad_buf));
    c->grad_buf = nullptr;
    c->grad_cap = 0;
    if (hipMalloc((void **)&c->grad_buf, sizeof(double) * ((size_t)np + 1)) != hipSuccess)
        return set_err(PGMG_ERR_NOMEM, "gradient partials");
    c->grad_cap = np;
    return PGMG_OK;
}

// Enqueue the pass on the current phi, read where it lies: the caller's array of a device-bound
// problem (pitch N, double, converted on load as the monitor converts it) or the level-0 grid.
// sum: the pass also writes its partials and the reduction their total to c->grad_buf + grad_cap
static int grad_enqueue(pgmg_ctx *c, int order, double w, double *gx, double *gy, bool sum)
{
    const Level &L = c->lv[0];
    const int N = L.N;
    PGMG_TRY(grad_reserve(c, gradient_blocks(N)));
    double *const total = sum ? c->grad_buf + c->grad_cap : nullptr;
    if (c->ext_phi != nullptr) {
        if (c->fp32) launch_gradient<float, double>(c->ext_phi, N, gx, gy, N, w, order, c->grad_buf, total, c->s);
        else launch_gradient<double, double>(c->ext_phi, N, gx, gy, N, w, order, c->grad_buf, total, c->s);
    } else if (c->fp32) {
        // every row and column the pass reads lies inside the level's grid
        PGMG_TRY(check_span(G<float>(L.A), L.P, 4, 0, N - 1, 0, N - 1, "k_gradient phi"));
        launch_gradient<float, float>(G<float>(L.A), L.P, gx, gy, N, w, order, c->grad_buf, total, c->s);
    } else {
        PGMG_TRY(check_span(G<double>(L.A), L.P, 8, 0, N - 1, 0, N - 1, "k_gradient phi"));
        launch_gradient<double, double>(G<double>(L.A), L.P, gx, gy, N, w, order, c->grad_buf, total, c->s);
    }
    HIPC(hipGetLastError());
    return PGMG_OK;
}

// what both context entries refuse after their arguments
static int grad_state_check(pgmg_ctx *c, const std::string &who)
{
    if (!c->have_problem) return set_err(PGMG_ERR_STATE, "pgmg_set_problem first");
    if (c->cfg.world > 1)
        return set_err(PGMG_ERR_STATE, who + ": one GPU only (world 1); row strips are not supported");
    return PGMG_OK;
}

}  // namespace pgmg

extern "C" {

int pgmg_gradient(pgmg_ctx *c, int order, double scale, double *d_gx, double *d_gy, double *norm)
{
    const std::string who("pgmg_gradient");
    if (!c) return set_err(PGMG_ERR_ARG, "null ctx");
    if (order != 2 && order != 4) return set_err(PGMG_ERR_ARG, who + ": order must be 2 or 4");
    if (!std::isfinite(scale)) return set_err(PGMG_ERR_ARG, who + ": scale must be finite");
    // phi's bytes: the bound array, or the whole allocation of the level-0 grid
    const Level &L = c->lv[0];
    const int N = L.N;
    const void *const pb = c->ext_phi ? (const void *)c->ext_phi : L.A.base;
    const size_t pn = c->ext_phi ? (size_t)N * N * sizeof(double) : L.A.bytes;
    if (const char *bad = gradient_arrays_error(pb, pn, d_gx, d_gy, N))
        return set_err(PGMG_ERR_ARG, who + ": " + bad);
    PGMG_TRY(grad_state_check(c, who));
    // the context's stream starts after the caller's work on phi and on the outputs
    PGMG_TRY(order_after_caller(c));
    PGMG_TRY(grad_enqueue(c, order, gradient_weight(order, scale, L.h), d_gx, d_gy, norm != nullptr));
    double t = 0.0;
    if (norm)
        HIPC(hipMemcpyAsync(&t, c->grad_buf + c->grad_cap, sizeof(double), hipMemcpyDeviceToHost, c->s));
    PGMG_TRY(stream_wait(c));
    if (norm) *norm = std::sqrt(t);
    return PGMG_OK;
}

int pgmg_gradient_time(pgmg_ctx *c, int order, int reps, double *ms_per_pass, double *bytes)
{
    const std::string who("pgmg_gradient_time");
    if (!c || !ms_per_pass || reps <= 0) return set_err(PGMG_ERR_ARG, "bad argument");
    if (order != 2 && order != 4) return set_err(PGMG_ERR_ARG, who + ": order must be 2 or 4");
    PGMG_TRY(grad_state_check(c, who));
    const Level &L = c->lv[0];
    const int N = L.N;
    const size_t elems = (size_t)N * N;
    if (!c->grad_out) {
        if (hipMalloc((void **)&c->grad_out, 2 * elems * sizeof(double)) != hipSuccess) {
            c->grad_out = nullptr;
            return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for pgmg_gradient_time's outputs");
        }
        register_alloc(c->grad_out, 2 * elems * sizeof(double));
    }
    double *const gx = c->grad_out, *const gy = c->grad_out + elems;
    PGMG_TRY(check_span(gx, N, 8, 0, N - 1, 0, N - 1, "k_gradient gx"));
    PGMG_TRY(check_span(gy, N, 8, 0, N - 1, 0, N - 1, "k_gradient gy"));
    const double w = gradient_weight(order, 1.0, L.h);
    if (c->ext_phi) PGMG_TRY(order_after_caller(c));
    for (int k = 0; k < 2; ++k) PGMG_TRY(grad_enqueue(c, order, w, gx, gy, true));
    HIPC(hipEventRecord(c->ev0, c->s));
    for (int k = 0; k < reps; ++k) PGMG_TRY(grad_enqueue(c, order, w, gx, gy, true));
    HIPC(hipEventRecord(c->ev1, c->s));
    HIPC(hipEventSynchronize(c->ev1));
    float f = 0.f;
    HIPC(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms_per_pass = f / reps;
    if (bytes) *bytes = (double)elems * ((c->ext_phi ? 8.0 : (double)L.es) + 16.0);
    return PGMG_OK;
}

}  // extern "C"
