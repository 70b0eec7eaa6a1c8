// pgmg_mem.hip — device memory of the context and of callers: the allocation registry behind
// the span checks, shuffled physical placement of the large grids, the level grids and the
// caller's grids (pgmg_alloc_grid).  Host code only.
#include <atomic>
#include <cstdio>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "pgmg_host.h"

using namespace pgmg;

// ---------------------------------------------------------------------------
// allocation
// ---------------------------------------------------------------------------
namespace {
std::mutex g_alloc_mu;
std::map<uintptr_t, size_t> g_allocs;   // base -> bytes of every registered allocation
}  // namespace

void pgmg::register_alloc(const void *base, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    g_allocs[(uintptr_t)base] = bytes;
}

void pgmg::unregister_alloc(const void *base)
{
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    g_allocs.erase((uintptr_t)base);
}

bool pgmg::registered_span(intptr_t lo, intptr_t hi)
{
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    auto it = g_allocs.upper_bound((uintptr_t)lo);
    if (it == g_allocs.begin()) return false;
    --it;
    const intptr_t b = (intptr_t)it->first, e = b + (intptr_t)it->second;
    return lo >= b && hi <= e;
}

namespace {
std::mutex g_user_mu;
struct UserGrid {
    void *alloc;
    unsigned long long serial;   // distinct for every pgmg_alloc_grid call (pgmg_grid_serial)
};
std::map<uintptr_t, UserGrid> g_user_grids;   // pgmg_alloc_grid: element (0,0) -> allocation
unsigned long long g_user_serial = 0;
}  // namespace

bool pgmg::is_device_ptr(const void *p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   // unregistered host memory: not an error to keep
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

int pgmg::check_span(const void *o, long long P, int es, long long r0, long long r1,
                     long long c0, long long c1, const char *what)
{
    if (o == nullptr || r1 < r0 || c1 < c0) return PGMG_OK;
    const intptr_t org = (intptr_t)o;
    const intptr_t lo = org + (intptr_t)((r0 * P + c0) * es);
    const intptr_t hi = org + (intptr_t)((r1 * P + c1 + 1) * es);   // one past the last byte
    if (registered_span(lo, hi)) return PGMG_OK;
    char buf[256];
    std::snprintf(buf, sizeof(buf),
                  "%s: rows %lld..%lld, columns %lld..%lld (pitch %lld) outside the array's "
                  "allocation",
                  what, r0, r1, c0, c1, P);
    return set_err(PGMG_ERR_STATE, buf);
}

// ---------------------------------------------------------------------------
// Shuffled physical placement (large grids).  The finest pass streams two 2 GB grids at once
// (reads one, writes the other a few rows behind); how fast depends on where their PHYSICAL
// pages lie relative to each other (profiles/r06/probes/: the same kernel on the same data runs
// 1.02 or 1.09 ms depending on the context's allocation, 1.14-1.29 ms with physically
// contiguous grids).  A grid of this kind is instead built from physical chunks mapped into one
// virtual range in a fixed pseudo-random order (HIP virtual memory API): whatever the
// allocator hands out, consecutive chunks of a grid do not sit at a fixed physical distance from
// the chunks of the other grids the pass streams at the same time.
// ---------------------------------------------------------------------------
namespace {
struct VmmAlloc {
    size_t bytes = 0, chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> h;
};
std::mutex g_vmm_mu;
std::map<uintptr_t, VmmAlloc> g_vmm;   // reserved base -> its chunks
}  // namespace

bool pgmg::is_vmm(const void *p)
{
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    auto it = g_vmm.upper_bound((uintptr_t)p);
    if (it == g_vmm.begin()) return false;
    --it;
    return (uintptr_t)p < it->first + it->second.bytes;
}

static hipError_t vmm_free(void *base)
{
    VmmAlloc a;
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        auto it = g_vmm.find((uintptr_t)base);
        if (it == g_vmm.end()) return hipErrorInvalidValue;
        a = std::move(it->second);
        g_vmm.erase(it);
    }
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < a.h.size(); ++i) {
        if (a.h[i] == 0) continue;
        const hipError_t u = hipMemUnmap(static_cast<char *>(base) + i * a.chunk, a.chunk);
        const hipError_t r = hipMemRelease(a.h[i]);
        if (e == hipSuccess) e = u != hipSuccess ? u : r;
    }
    const hipError_t f = hipMemAddressFree(base, a.bytes);
    return e != hipSuccess ? e : f;
}

// `bytes` of device memory on the current device from chunks of `chunk_mb` MB (rounded to the
// allocation granularity) mapped in a fixed shuffled order; *out = nullptr on failure
static hipError_t vmm_alloc(void **out, size_t bytes, size_t chunk_mb)
{
    *out = nullptr;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if ((e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum)) != hipSuccess)
        return e;
    size_t chunk = std::max(gran, (chunk_mb << 20) / gran * gran);
    const size_t n = (bytes + chunk - 1) / chunk, total = n * chunk;
    void *base = nullptr;
    if ((e = hipMemAddressReserve(&base, total, 0, nullptr, 0)) != hipSuccess) return e;
    VmmAlloc a;
    a.bytes = total;
    a.chunk = chunk;
    a.h.assign(n, 0);
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        g_vmm[(uintptr_t)base] = a;
    }
    // the k-th physical chunk created goes to virtual slot (k * stride + shift) % n: a
    // multiplicative permutation (stride coprime to n) scattering consecutive chunks, different
    // for every grid (the relative placement of two grids' chunks at the same virtual offset --
    // what two streams of one pass touch together -- then varies from chunk to chunk)
    static std::atomic<unsigned> serial{0};
    const unsigned g = serial.fetch_add(1);
    const double phi = 0.6180339887 + 0.0731 * (double)(g % 7);
    size_t stride = ((size_t)(phi * (double)n) % n) | 1;
    while (std::gcd(stride, n) != 1) stride += 2;
    const size_t shift = ((size_t)g * 40503u) % n;
    for (size_t k = 0; k < n && e == hipSuccess; ++k) {
        const size_t slot = (k * stride + shift) % n;
        hipMemGenericAllocationHandle_t h = 0;
        if ((e = hipMemCreate(&h, chunk, &prop, 0)) != hipSuccess) break;
        {
            std::lock_guard<std::mutex> lk(g_vmm_mu);
            g_vmm[(uintptr_t)base].h[slot] = h;
        }
        e = hipMemMap(static_cast<char *>(base) + slot * chunk, chunk, 0, h, 0);
    }
    if (e == hipSuccess) {
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(base, total, &acc, 1);
    }
    if (e != hipSuccess) {
        (void)vmm_free(base);
        return e;
    }
    *out = base;
    return hipSuccess;
}

int pgmg::alloc_grid(Grid &g, const Level &L, size_t stagger, bool shuffle)
{
    // owned rows + kHalo halo rows each side (the fused passes read 4 rows past a
    // segment); the slack covers the last wave tile reading past the row end
    const int rows = (L.hi - L.lo) + 2 * kHalo;
    // column 1 of every row on a 128-byte boundary: 128/es - 1 elements before (0,0)
    const size_t off = (size_t)(128 / L.es - 1) + (stagger / 128) * (128 / L.es);
    const size_t n = off + (size_t)rows * L.P + 512;
    void *p = nullptr;
    // (measurement build: PGMG_CONTIG=1 asks for physically contiguous memory for grids of
    // 64 MB and more: a placement probe)
    // (measurement build: PGMG_CONTIG=1 physically contiguous grids, PGMG_SHUFFLE_MB the chunk
    // size of the shuffled ones, 0 = no shuffling)
    const bool contig = tuning_int("PGMG_CONTIG", 0) != 0 && n * L.es >= (64u << 20);
    const int shuffle_mb = tuning_int("PGMG_SHUFFLE_MB", 2);
    const bool shuffled = shuffle && shuffle_mb > 0 && n * L.es >= (256u << 20);
    hipError_t ae = hipErrorUnknown;
    if (shuffled) ae = vmm_alloc(&p, n * L.es, (size_t)shuffle_mb);
    if (shuffled && ae != hipSuccess) (void)hipGetLastError();   // no VMM here: plain memory
    if (ae == hipSuccess) {
    } else if (contig) ae = hipExtMallocWithFlags(&p, n * L.es, hipDeviceMallocContiguous);
    else ae = hipMalloc(&p, n * L.es);
    if (ae != hipSuccess)
        return set_err(PGMG_ERR_NOMEM, "hipMalloc failed for a level of N=" + std::to_string(L.N) + ": " +
                                           hipGetErrorString(ae));
    HIPC(hipMemset(p, 0, n * L.es));
    g.base = p;
    g.bytes = n * L.es;
    register_alloc(p, g.bytes);
    g.o = static_cast<char *>(p) + (off + (ptrdiff_t)(kHalo - L.lo) * L.P) * L.es;
    return PGMG_OK;
}

void pgmg::free_grid(Grid &g)
{
    if (g.base) {
        unregister_alloc(g.base);
        if (vmm_free(g.base) != hipSuccess) (void)hipFree(g.base);   // (not a shuffled grid)
    }
    g.base = g.o = nullptr;
    g.bytes = 0;
}

extern "C" {   // the caller's grids

int pgmg_alloc_grid(double **out, int N)
{
    if (!out || N < 3) return set_err(PGMG_ERR_ARG, "pgmg_alloc_grid: null pointer or N < 3");
    *out = nullptr;
    // (kHalo + 2) rows + 1024 elements before element (0,0) and after element (N-1, N-1);
    // column 1 of row 0 on a 128-byte boundary
    const size_t guard = (size_t)(kHalo + 2) * N + 1024 + 15;
    const size_t n = 2 * guard + (size_t)N * N;
    void *p = nullptr;
    if (hipMalloc(&p, n * sizeof(double)) != hipSuccess)
        return set_err(PGMG_ERR_NOMEM, "pgmg_alloc_grid: hipMalloc failed");
    HIPC(hipMemset(p, 0, n * sizeof(double)));
    register_alloc(p, n * sizeof(double));
    double *o = static_cast<double *>(p) + guard;
    {
        std::lock_guard<std::mutex> lk(g_user_mu);
        g_user_grids[(uintptr_t)o] = UserGrid{p, ++g_user_serial};
    }
    *out = o;
    return PGMG_OK;
}

int pgmg_free_grid(double *o)
{
    if (!o) return PGMG_OK;
    void *p = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_user_mu);
        auto it = g_user_grids.find((uintptr_t)o);
        if (it == g_user_grids.end()) return set_err(PGMG_ERR_ARG, "pgmg_free_grid: not from pgmg_alloc_grid");
        p = it->second.alloc;
        g_user_grids.erase(it);
    }
    unregister_alloc(p);
    HIPC(hipFree(p));
    return PGMG_OK;
}

int pgmg_grid_serial(const double *o, unsigned long long *serial)
{
    if (!serial) return set_err(PGMG_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g_user_mu);
    auto it = g_user_grids.find((uintptr_t)o);
    *serial = it == g_user_grids.end() ? 0ull : it->second.serial;
    return PGMG_OK;
}

int pgmg_pointer_is_device(const void *p, int *is_device)
{
    if (!is_device) return set_err(PGMG_ERR_ARG, "null argument");
    *is_device = (p != nullptr && is_device_ptr(p)) ? 1 : 0;
    return PGMG_OK;
}

int pgmg_check_span(const void *origin, long long pitch, int elem_bytes, long long row0,
                    long long row1, long long col0, long long col1)
{
    if (!origin || pitch <= 0 || elem_bytes <= 0 || row1 < row0 || col1 < col0)
        return set_err(PGMG_ERR_ARG, "pgmg_check_span: bad arguments");
    return check_span(origin, pitch, elem_bytes, row0, row1, col0, col1, "pgmg_check_span");
}

}  // extern "C"
