// ref_harness.cpp — drives the REFERENCE's own CPU multigrid (TEST INFRASTRUCTURE).
//
// Compiled by oracle/Makefile directly against the reference headers where they lie
// (/root/reference/2_part_MG/MultiGrid.hpp, Smoother.hpp, DynamicGridUtils.hpp,
// globals.cpp); output goes to oracle/_ref/ only.  Nothing from the reference is
// copied into this repository.  Used to generate tests/golden/ and to pin
// oracle/pgmg_oracle.c bit for bit.
//
// Usage: ref_harness <V|W|F|G> <N> <cycles> <eps> [phi_out.bin|- [alpha [n_coarse [a p q [h]]]]]
//   G = FMG start + W-cycles (BASELINE config 5): cycle 1 is an F-cycle, later ones W
//   alpha    : the W-cycle's recursion count, MultigridSolver's constructor argument
//              (MultiGrid.hpp:22); absent: 3 (2_part_MG/main.cpp:15)
//   n_coarse : MultigridSolver::N_coarse (MultiGrid.hpp:19), set before the F-cycle's
//              coarsest size is read from it; absent: the reference's own 5
//   a p q    : the reference's problem constants, its globals a, p, q (globals.cpp:2-4), assigned
//              before anything reads them; absent: the reference's own 1, 1, 1
//   h        : the mesh width handed to compute_rhs, compute_exact_solution, v_cycle / w_cycle
//              (the h argument of MultiGrid.hpp:57) and compute_residual; "-" or absent:
//              a / (N - 1).  The F-cycle keeps its own chain from 1 / (n_coarse - 1).
//   phi_out.bin "-": no dump (a placeholder so the parameters can follow)
// Prints one line per cycle:
//   cycle <k> relerr <e> res <r> center <phi[(N/2)*N+N/2]> hash <fnv64> sweeps <s> exits <x>
//   seconds <wall time of the reference's cycle call alone>  (bench.py's cpu_baseline)
// and, if given, writes phi after the last cycle as raw little-endian doubles.
// Two more modes take their arrays from files: O (the op-level entries, op_mode) and P (V- or
// W-cycles on a caller's phi0 and f, problem_mode); their usage stands above each.
//
// operator new[] is calloc-backed: the reference reads the never-written
// boundary of `new double[L]` residual buffers (Smoother.hpp:75-76), which is
// undefined; zero is what it reads in practice and what we pin.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <new>
#include <string>
#include <vector>

// Leak reclaimer: JacobiSmoother::smooth allocates a residual buffer per sweep and never
// frees it (Smoother.hpp:75): 2 GB per sweep at N = 16385.  smooth() hands no
// pointer out, so every new[] made inside one smooth() call and still live when it
// returns is garbage; CountingJacobi frees it (this is what lets the harness run 30+
// cycles at 16385).  Values are unaffected: the buffers are dead.
static std::vector<void *> *g_track = nullptr;

void *operator new[](std::size_t n)
{
    void *p = std::calloc(n ? n : 1, 1);
    if (!p) throw std::bad_alloc();
    if (g_track) g_track->push_back(p);
    return p;
}
static void untrack(void *p)
{
    if (!g_track || !p) return;
    for (auto &q : *g_track)
        if (q == p) { q = g_track->back(); g_track->pop_back(); return; }
}
void operator delete[](void *p) noexcept { untrack(p); std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { untrack(p); std::free(p); }

#define private public
#include "2_part_MG/MultiGrid.hpp"
#undef private

struct CountingJacobi : public JacobiSmoother {
    using JacobiSmoother::JacobiSmoother;
    long long sweeps = 0, exits = 0;
    void smooth(double *x, double *f, int w, int hgt, double h, int num_iter,
                double *x_true = nullptr, std::vector<double> *residuals = nullptr,
                std::vector<double> *errors = nullptr) override
    {
        (void)residuals;
        std::vector<double> r;
        std::vector<void *> live;
        g_track = &live;
        JacobiSmoother::smooth(x, f, w, hgt, h, num_iter, x_true, &r, errors);
        g_track = nullptr;
        for (void *p : live) std::free(p);
        sweeps += (long long)r.size();
        if (!r.empty() && r.back() < epsilon) exits++;
    }
};

static uint64_t fnv(const double *v, long long n)
{
    uint64_t h = 1469598103934665603ULL;
    for (long long i = 0; i < n; ++i) {
        uint64_t w;
        std::memcpy(&w, &v[i], 8);
        h = (h ^ w) * 1099511628211ULL;
    }
    return h;
}

// Op mode: ref_harness O <N> <h> <eps> <in.bin> <out.bin>
// in.bin : x[N*N], f[N*N], e[Nc*Nc]  (doubles)
// out.bin: residual(x,f)[N*N] | restrict(x)[Nc*Nc] | x + P e [N*N] |
//          smooth(x,f,num_iter=1)[N*N] | smooth(x,f,num_iter=10)[N*N]
static int op_mode(int argc, char **argv)
{
    if (argc < 7) return 2;
    const int N = std::atoi(argv[2]);
    const double h = std::atof(argv[3]);
    const double eps = std::atof(argv[4]);
    const int Nc = (N - 1) / 2 + 1;
    const long long L = (long long)N * N, Lc = (long long)Nc * Nc;
    std::vector<double> in(2 * L + Lc);
    FILE *fp = std::fopen(argv[5], "rb");
    if (!fp || std::fread(in.data(), 8, in.size(), fp) != in.size()) return 3;
    std::fclose(fp);
    const double *x = in.data(), *f = in.data() + L, *e = in.data() + 2 * L;
    JacobiSmoother sm(eps);
    MultigridSolver mg(&sm, 3, N);
    std::vector<double> out;
    std::vector<double> r(L, 0.0);
    DynamicGridUtils::compute_residual(r.data(), x, f, N, N, h);
    out.insert(out.end(), r.begin(), r.end());
    std::vector<double> c(Lc, 0.0);
    mg.restrict_full_weighting(x, c.data(), N, Nc);
    out.insert(out.end(), c.begin(), c.end());
    std::vector<double> p(x, x + L);
    mg.prolongation(p.data(), e, N, Nc);
    out.insert(out.end(), p.begin(), p.end());
    for (int it : {1, 10}) {
        std::vector<double> s(x, x + L);
        sm.smooth(s.data(), const_cast<double *>(f), N, N, h, it);
        out.insert(out.end(), s.begin(), s.end());
    }
    fp = std::fopen(argv[6], "wb");
    if (!fp) return 3;
    std::fwrite(out.data(), 8, out.size(), fp);
    std::fclose(fp);
    return 0;
}

// Custom-problem mode: ref_harness P <V|W> <N> <cycles> <eps> <alpha> <n_coarse> <h> <in.bin> <out.bin>
// in.bin : phi0[N*N], f[N*N]  (doubles; any words: signed zeros, subnormals, Inf, NaN)
// out.bin: phi[N*N] after every cycle, `cycles` grids
// n_coarse 0: the reference's default; h "-": 1 / (N - 1)
// Prints one line per cycle: cycle <k> sweeps <s> exits <x>  (cumulative, as the cycle modes)
static int problem_mode(int argc, char **argv)
{
    if (argc < 11) return 2;
    const char kind = argv[2][0];
    const int N = std::atoi(argv[3]);
    const int cycles = std::atoi(argv[4]);
    const double eps = std::atof(argv[5]);
    const int alpha = std::atoi(argv[6]);
    const int n_coarse = std::atoi(argv[7]);
    const double h = std::strcmp(argv[8], "-") != 0 ? std::atof(argv[8]) : 1.0 / (N - 1);
    if ((kind != 'V' && kind != 'W') || N < 3 || cycles < 1 || alpha < 1) return 2;
    const long long L = (long long)N * N;
    std::vector<double> in(2 * L);
    FILE *fp = std::fopen(argv[9], "rb");
    if (!fp || std::fread(in.data(), 8, in.size(), fp) != in.size()) return 3;
    std::fclose(fp);
    double *phi = in.data(), *f = in.data() + L;
    CountingJacobi sm(eps);
    MultigridSolver mg(&sm, alpha, N);
    if (n_coarse > 0) mg.N_coarse = n_coarse;
    fp = std::fopen(argv[10], "wb");
    if (!fp) return 3;
    for (int k = 1; k <= cycles; ++k) {
        if (kind == 'V') mg.v_cycle(phi, f, N, h);
        else mg.w_cycle(phi, f, N, h);
        std::fwrite(phi, 8, (size_t)L, fp);
        std::printf("cycle %d sweeps %lld exits %lld\n", k, sm.sweeps, sm.exits);
    }
    std::fclose(fp);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && argv[1][0] == 'O') return op_mode(argc, argv);
    if (argc > 1 && argv[1][0] == 'P') return problem_mode(argc, argv);
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <V|W|F|G> <N> <cycles> <eps> [phi_out.bin|- [alpha [n_coarse "
                             "[a p q [h]]]]]\n", argv[0]);
        return 2;
    }
    const char kind = argv[1][0];
    const int N = std::atoi(argv[2]);
    const int cycles = std::atoi(argv[3]);
    const double eps = std::atof(argv[4]);
    const int alpha = argc > 6 ? std::atoi(argv[6]) : 3;
    const int n_coarse = argc > 7 ? std::atoi(argv[7]) : 0;   // 0: the reference's default
    if (alpha < 1 || (argc > 7 && n_coarse < 3)) {
        std::fprintf(stderr, "alpha must be >= 1 and n_coarse >= 3\n");
        return 2;
    }
    if (argc > 8 && argc < 11) {
        std::fprintf(stderr, "a, p and q come together\n");
        return 2;
    }
    if (argc > 10) {
        a = std::atof(argv[8]);
        p = std::atof(argv[9]);
        q = std::atof(argv[10]);
    }
    const long long L = (long long)N * N;
    const double h = argc > 11 && std::strcmp(argv[11], "-") != 0 ? std::atof(argv[11]) : a / (N - 1);

    double *phi = new double[L];
    double *f = new double[L];
    double *ex = new double[L];
    double *r = new double[L];
    DynamicGridUtils::initialize_zeros(phi, L);
    DynamicGridUtils::compute_rhs(f, N, N, h);
    DynamicGridUtils::compute_exact_solution(ex, h, N, N);

    CountingJacobi sm(eps);
    MultigridSolver mg(&sm, alpha, N);
    if (n_coarse > 0) mg.N_coarse = n_coarse;
    const int n0 = mg.N_coarse;
    const double h0 = 1.0 / (n0 - 1);
    double *f0 = new double[n0 * n0];
    DynamicGridUtils::compute_rhs(f0, n0, n0, h0);

    for (int k = 1; k <= cycles; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        if (kind == 'V') {
            mg.v_cycle(phi, f, N, h);
        } else if (kind == 'W' || (kind == 'G' && k > 1)) {
            mg.w_cycle(phi, f, N, h);
        } else {
            double *p0 = nullptr;
            mg.compute_coarsest_grid(phi, p0, N, n0);
            mg.f_cycle(p0, f0, n0, h0);
            std::memcpy(phi, mg.final_solution, sizeof(double) * L);
            delete[] p0;
        }
        const double secs =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        DynamicGridUtils::initialize_zeros(r, L);
        DynamicGridUtils::compute_residual(r, phi, f, N, N, h);
        double res = DynamicGridUtils::norm(r, L);
        double *e = new double[L];
        DynamicGridUtils::compute_error(e, phi, ex, L);
        double rel = DynamicGridUtils::norm(e, L) / DynamicGridUtils::norm(ex, L);
        delete[] e;
        std::printf("cycle %d relerr %.17g res %.17g center %.17g hash %016llx sweeps %lld exits %lld"
                    " seconds %.6f\n",
                    k, rel, res, phi[(long long)(N / 2) * N + N / 2],
                    (unsigned long long)fnv(phi, L), sm.sweeps, sm.exits, secs);
        std::fflush(stdout);
    }
    if (argc > 5 && std::strcmp(argv[5], "-") != 0) {
        FILE *fp = std::fopen(argv[5], "wb");
        if (!fp) return 3;
        std::fwrite(phi, sizeof(double), (size_t)L, fp);
        std::fclose(fp);
    }
    return 0;
}
