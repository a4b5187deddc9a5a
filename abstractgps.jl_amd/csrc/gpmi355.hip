// gpmi355.hip — host engine + C ABI (include/gpmi355.h) of libgpmi355.so.
//
// Host orchestration of the kernels in kernels.hpp:
//   assemble (kmat)  ->  right-looking blocked Cholesky with a recursive panel and look-ahead
//   (potf2_64 / trsm_64 / MFMA gemm_nt_sub)  ->  logdet + forward solve (carried as extra RHS rows
//   of the factorisation)  ->  backward substitution  ->  logpdf scalar and α.
// Mirrors, on the device, reference src/finite_gp_projection.jl:306-311 and
// src/exact_gpr_posterior.jl:29-35, 60-90 (see include/gpmi355.h for the per-entry citations).
#include "kernels.hpp"  // includes engine.hpp (shared structs, registry, error helpers)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

using namespace gpmi;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int32_t set_err_text(int32_t status, const std::string& msg) {
    g_err = msg;
    return status;
}
int32_t set_hip_err(hipError_t e, const char* what, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), what, line);
    g_err = buf;
    return -1000 - (int)e;
}
int32_t set_arg_err(int i, const char* msg) {
    g_err = std::string("invalid argument ") + std::to_string(i) + ": " + msg;
    return -i;
}
std::mutex g_reg_mu;
std::set<void*> g_live;
void reg_add(void* p) {
    std::lock_guard<std::mutex> l(g_reg_mu);
    g_live.insert(p);
}
bool reg_take(void* p) {
    std::lock_guard<std::mutex> l(g_reg_mu);
    return g_live.erase(p) > 0;
}
bool reg_has(void* p) {
    std::lock_guard<std::mutex> l(g_reg_mu);
    return g_live.count(p) > 0;
}
static void pool_drop(gp_ctx* c, size_t i) {
    c->pool_bytes -= c->pool[i].bytes;
    (void)hipFree(c->pool[i].p);
    c->pool.erase(c->pool.begin() + i);
}
// "alloc_poison": all-ones bytes (NaN as fp64 / fp32, −1 as int32) over a block before anyone sees it.  The blocks are used on the panel and third
// streams too, hence the wait (a diagnostic: nothing in the production path sets it).
static int32_t ctx_poison(gp_ctx* c, void* p, size_t bytes) {
    HIPCHK(hipMemsetAsync(p, 0xFF, bytes, c->sm));
    HIPCHK(hipStreamSynchronize(c->sm));
    return 0;
}
int32_t ctx_alloc(gp_ctx* c, size_t bytes, void** out) {
    size_t best = (size_t)-1;
    int bi = -1;
    for (size_t i = 0; i < c->pool.size(); ++i)
        if (c->pool[i].bytes >= bytes && c->pool[i].bytes < best && c->pool[i].bytes <= bytes + bytes / 4 + (1 << 20)) {
            best = c->pool[i].bytes;
            bi = (int)i;
        }
    if (bi >= 0) {
        *out = c->pool[bi].p;
        c->blk[*out] = c->pool[bi].bytes;  // the block keeps its true size
        c->pool_bytes -= c->pool[bi].bytes;
        c->pool.erase(c->pool.begin() + bi);
        if (c->alloc_poison) RC(ctx_poison(c, *out, c->blk[*out]));  // the block's true size
        return 0;
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {  // drop the cache and retry once
        (void)hipGetLastError();
        while (!c->pool.empty()) pool_drop(c, c->pool.size() - 1);
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) return set_hip_err(e, "hipMalloc", __LINE__);
    c->blk[*out] = bytes;
    if (c->alloc_poison) RC(ctx_poison(c, *out, bytes));
    return 0;
}
void ctx_release(gp_ctx* c, void* p, size_t /*requested*/) {
    if (!p) return;
    size_t bytes = 0;
    auto it = c->blk.find(p);
    if (it != c->blk.end()) {
        bytes = it->second;
        c->blk.erase(it);
    }
    if (c->dead || bytes == 0 || c->pool_cap == 0) {  // pool_cap_mb = 0: nothing is cached
        (void)hipFree(p);
        return;
    }
    if (bytes > c->pool_cap) {
        // ONE block larger than the cap may stay cached: the factor of N > 110 000 points is 100+ GB and re-allocating it costs seconds per fit (N = 131 072: 17.2 s per
        // pair with the block freed and allocated again against ≈ 12 s of work).  It takes the whole cache (everything else goes, a previous oversize block included);
        // ctx_alloc drops the cache and retries when an allocation fails, and gp_ctx_trim returns it like any other block.
        while (!c->pool.empty()) pool_drop(c, c->pool.size() - 1);
        c->pool.push_back({p, bytes});
        c->pool_bytes += bytes;
        return;
    }
    c->pool.push_back({p, bytes});
    c->pool_bytes += bytes;
    // bound the cache by bytes and by count (a VFE fit cycles through ~16 buffers, its gradient pass through ~25 more); oldest blocks go first — an oversize block (above) is the last to go and
    // keeps 4 GiB of room beside it for the small buffers of the calls that follow
    size_t big = 0;
    for (const auto& b : c->pool) big = std::max(big, b.bytes);
    const size_t limit = big > c->pool_cap ? big + ((size_t)4 << 30) : c->pool_cap;
    while (c->pool.size() > 1 && (c->pool_bytes > limit || c->pool.size() > 96)) pool_drop(c, (c->pool[0].bytes > c->pool_cap) ? 1 : 0);
}
void ctx_unref(gp_ctx* c) {
    if (--c->refs != 0) return;
    (void)hipSetDevice(c->device);
    for (auto& b : c->pool) (void)hipFree(b.p);
    for (auto& kv : c->blk) (void)hipFree(kv.first);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto e : c->ev_phase)
        if (e) (void)hipEventDestroy(e);
    if (c->info_dev) (void)hipFree(c->info_dev);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->plan_pin) (void)hipHostFree(c->plan_pin);
    if (c->plan_ev) (void)hipEventDestroy(c->plan_ev);
    if (c->ticket_dev) (void)hipFree(c->ticket_dev);
    if (c->w_ws) (void)hipFree(c->w_ws);
    if (c->scal_dev) (void)hipFree(c->scal_dev);
    if (c->sp) (void)hipStreamDestroy(c->sp);
    if (c->sq) (void)hipStreamDestroy(c->sq);
    if (c->own_sm && c->sm) (void)hipStreamDestroy(c->sm);
    delete c;
}
// the ctx's third stream (high priority, like the panel stream), created and primed on first use
int32_t ctx_third_stream(gp_ctx* c, hipStream_t* out) {
    if (!c->sq) {
        HIPCHK(hipSetDevice(c->device));
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIPCHK(hipStreamCreateWithPriority(&c->sq, hipStreamNonBlocking, hi));
        RC(ctx_prime_stream(c, c->sq));
    }
    *out = c->sq;
    return 0;
}
void* ctx_pinned(gp_ctx* c, size_t bytes) {
    if (bytes > ((size_t)1 << 30)) return nullptr;
    if (c->pin && c->pin_bytes >= bytes) return c->pin;
    if (c->pin) (void)hipHostFree(c->pin);
    c->pin = nullptr;
    c->pin_bytes = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&c->pin, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->pin = nullptr;
        return nullptr;
    }
    c->pin_bytes = want;
    return c->pin;
}
int32_t ctx_event(gp_ctx* c, hipEvent_t* out, bool timing) {
    // timing events are separate objects (created on demand, pooled)
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    (void)timing;
    *out = c->ev_pool[c->ev_used++];
    return 0;
}
int32_t ctx_scal(gp_ctx* c, long n) {
    if (c->scal_cap >= n) return 0;
    if (c->scal_dev) (void)hipFree(c->scal_dev);
    c->scal_cap = round_up(n, 1024);
    HIPCHK(hipMalloc((void**)&c->scal_dev, sizeof(double) * c->scal_cap));
    if (c->alloc_poison) RC(ctx_poison(c, c->scal_dev, sizeof(double) * c->scal_cap));
    return 0;
}

__global__ void prime_kernel(int* p) {
    if (p && threadIdx.x == 0) *p = 0;
}
// Everything a ctx creates lazily, created NOW: the workspaces (leaf tickets, info, scalars, trtri tiles for nb_hint columns) and
// — by launching one empty kernel on each stream — the hardware queues behind its streams.  HIP creates the HSA queue of a stream
// at its first use, and every queue creation makes the hardware scheduler unmap and remap ALL queues of the process (running waves
// are context-switched out and back in).  The multi-device driver primes every rank context when it is created, so that no queue
// appears while kernels of other ranks run (the first-fit item).
int32_t ctx_prime(gp_ctx* c, long nb_hint) {
    HIPCHK(hipSetDevice(c->device));
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 8 + 128));
    if (!c->ticket_dev) {
        HIPCHK(hipMalloc((void**)&c->ticket_dev, sizeof(int) * 64));
        HIPCHK(hipMemset(c->ticket_dev, 0, sizeof(int) * 64));
    }
    const size_t need = sizeof(double) * (size_t)(std::max(nb_hint, 256L) / 64 + 2) * 4096;
    if (c->w_ws_bytes < need) {
        if (c->w_ws) (void)hipFree(c->w_ws);
        c->w_ws_bytes = 0;
        HIPCHK(hipMalloc(&c->w_ws, need));
        HIPCHK(hipMemset(c->w_ws, 0, need));
        if (c->alloc_poison) RC(ctx_poison(c, c->w_ws, need));
        c->w_ws_bytes = need;
    }
    hipLaunchKernelGGL(prime_kernel, dim3(1), dim3(64), 0, c->sm, c->info_dev);
    hipLaunchKernelGGL(prime_kernel, dim3(1), dim3(64), 0, c->sp, (int*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->sm));
    HIPCHK(hipStreamSynchronize(c->sp));
    return 0;
}
int32_t ctx_prime_stream(gp_ctx* c, hipStream_t s) {
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(prime_kernel, dim3(1), dim3(64), 0, s, (int*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
// (lower_count: bulk_plan.hpp)

template <typename T, typename CT = T>
static int32_t launch_gemm(gp_ctx* c, hipStream_t s, CT* C, long ldc, const T* A, long lda, const T* B, long ldb,
                           long M, long N, long K, GridMap g) {
    static_assert(std::is_same<T, CT>::value, "operands and result share one dtype (fp64 sums of fp32 products are formed by the callers)");
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    gp_ctx::GemmRec rec{};
    const bool timed = c->time_kernels != 0;
    if (timed) {
        RC(ctx_event(c, &rec.a, true));
        RC(ctx_event(c, &rec.b, true));
        double elems = (g.lower && g.P == 1 && g.Q == 1) ? lower_count(M, N, g.row0, g.col0) : (double)M * (double)N;
        if (g.nbatch > 1) elems *= g.nbatch;
        rec.flops = g.ktri == 1 ? (double)N * (double)M * (double)(2 * g.ktri_off + M + 128)
                                : (g.ktri == 2 ? (g.ktri_off > 0 ? 2.0 * (double)g.ktri_off * (double)N * (double)K + (double)N * (double)K * (double)K
                                                                 : (double)M * (double)M * (double)M / 3.0)
                                               : (g.ktri == 3 ? (double)M * (double)N * (double)(N + 128) : 2.0 * (double)K * elems));
        rec.bytes = 2.0 * sizeof(CT) * elems * (g.c2off ? 2 : 1) + sizeof(T) * (double)K * (double)(M + N);
        rec.M = M; rec.N = N; rec.K = K;
        rec.stream = (s == c->sp);
        HIPCHK(hipEventRecord(rec.a, s));
    }
    dim3 grid((unsigned)((N + 127) / 128), (unsigned)((M + 127) / 128));
    const long tm = (M + 127) / 128, tn = (N + 127) / 128;
    const bool single_lower = g.lower && g.P == 1 && g.Q == 1 && g.row0 >= g.col0;
    const long dt = single_lower ? (g.row0 - g.col0 + 127) / 128 : 0;
    g.tm = (int)tm;
    g.tn = (int)tn;
    g.dt = (int)dt;
    if (c->xcd_swizzle && tm * tn >= c->xcd_min_tiles) {  // XCD-aware 8×8 super-tile order (kernels.hpp xcd_tile)
        const long tms = (tm + 7) / 8, tns = (tn + 7) / 8, dts = (dt + 7) / 8;
        long nsuper;
        if (single_lower) {
            const long tri = std::min(tms, std::max(0L, tns - dts));
            nsuper = tri * (dts + 1) + tri * (tri - 1) / 2 + (tms - tri) * tns;
            g.compact = 3;
        } else {
            nsuper = tms * tns;
            g.compact = 2;
        }
        grid = dim3((unsigned)(round_up(nsuper, 8) * 64), 1);
    } else if (single_lower) {  // enumerate only the tiles on/below the diagonal
        const long tri = std::min(tm, std::max(0L, tn - dt));
        const long total = tri * (dt + 1) + tri * (tri - 1) / 2 + (tm - tri) * tn;
        g.compact = 1;
        grid = dim3((unsigned)total, 1);
    }
    if (g.nbatch > 1) grid.z = (unsigned)g.nbatch;
    if (!c->deterministic && K >= c->sk_min_k && (c->gemm_streamk || c->sk_scope > 0) && !g.beta0 && !g.ktri && g.nbatch <= 1 && g.P == 1 && g.Q == 1 && g.compact <= 1 &&
        (g.compact == 1 ? (long)grid.x : tm * tn) <= c->sk_max_tiles) {
        // persistent grid + stream-K tail (kernels.hpp gemm_nt_sk_kernel)
        const long nk = K / (128 / (long)sizeof(T));  // BK = 16 (f64) / 32 (f32)
        const long ntiles = g.compact == 1 ? (long)grid.x : tm * tn;
        const long Gmax = 2L * c->num_cus;
        const long G = Gmax;  // fewer tiles than workgroups: every tile is cut along k
        const long R = ntiles - (ntiles / G) * G;
        // tail shares: never fewer workgroups than tail tiles; beyond that at least 16 k-steps per share
        long G2 = std::min(G, std::max(R, R * nk / 16));
        if (R == 0) G2 = 0;
        if (c->gemm_pipe)
            hipLaunchKernelGGL((gemm_nt_sk_kernel<T, 1>), dim3((unsigned)G), dim3(256), 0, s, (T*)C, ldc, A, lda, B, ldb, (int)M, (int)N,
                               (int)K, g, ntiles, (int)G2);
        else
            hipLaunchKernelGGL((gemm_nt_sk_kernel<T, 0>), dim3((unsigned)G), dim3(256), 0, s, (T*)C, ldc, A, lda, B, ldb, (int)M, (int)N,
                               (int)K, g, ntiles, (int)G2);
    } else {
        // residency: two workgroups per CU (fp64: measured best over a whole factorisation; fp32: since the pipelined k loop, "gemm_pad_f32");
        // a dynamic-LDS request of 20 KiB on top of the 64 KiB static image pins ONE per CU.  "gemm_pad_lds" overrides both.
        const long pad = c->gemm_pad_user ? c->gemm_pad_lds : (sizeof(T) == 4 ? c->gemm_pad_f32 : 0);
        if (pad > 0 && !c->gemm_pad_set) {
            HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_dma_kernel<double, double, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
            HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_dma_kernel<float, float, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
            HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_dma_kernel<double, double, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
            HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_dma_kernel<float, float, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
            c->gemm_pad_set = true;
        }
        if (c->gemm_pipe)
            hipLaunchKernelGGL((gemm_nt_dma_kernel<T, CT, 1>), grid, dim3(256), (size_t)pad, s, C, ldc, A, lda, B, ldb, (int)M, (int)N, (int)K, g);
        else
            hipLaunchKernelGGL((gemm_nt_dma_kernel<T, CT, 0>), grid, dim3(256), (size_t)pad, s, C, ldc, A, lda, B, ldb, (int)M, (int)N, (int)K, g);
    }
    HIPCHK(hipGetLastError());
    if (timed) {
        HIPCHK(hipEventRecord(rec.b, s));
        c->gemm_recs.push_back(rec);
    }
    return 0;
}

GridMap gpmi::plain_map(int lower, long row0, long col0) {
    GridMap g;
    g.lower = lower;
    g.P = 1; g.p = 0; g.Q = 1; g.q = 0;
    g.nb = 128;
    g.row0 = row0;
    g.col0 = col0;
    g.compact = 0;
    g.tn = 0;
    g.dt = 0;
    g.tm = 0;
    g.beta0 = 0;
    g.ktri = 0;
    g.nbatch = 1;
    g.cstride = 0;
    g.astride = 0;
    g.bstride = 0;
    g.ktri_off = 0;
    g.c2off = 0;
    g.c2stride = 0;
    g.s1 = 0;
    g.s2 = 0;
    return g;
}

// ------------------------------------------------------------------------------------------------
// Strassen form of the large off-diagonal products of the trailing update (fp64; ctx parameter "strassen_min_rows").
//   C(M×N) −= A·Bᵀ with every operand cut into 2×2 quadrants (rows, k) is seven products of (M/2)×(N/2)×(K/2) instead of eight: two launches of
//   strassen_sums_kernel write the ten operand sums into the workspace, then ordered launches of the tile GEMM accumulate each product from zero
//   and subtract it from its one or two target quadrants (GridMap c2off / s1 / s2), products with disjoint targets two to a launch: four launches.
//   No atomics, one stream: bitwise repeatable.
// ------------------------------------------------------------------------------------------------
struct StrassenWs {  // the ten sum panels, rows of K/2 + ldpad elements (the pad keeps the row stride off a power of two like every other operand's)
    double* p = nullptr;
    size_t elems = 0;
};
// (the shape rules live in bulk_plan.hpp: the plan of a grouped update and the launch sequence below split at the same points)
static size_t strassen_ws_elems(const gp_ctx* c, long M, long N, long K) { return strassen_ws_rule(c->ldpad, M, N, K); }
// shapes the Strassen form takes: quadrants of whole 128×128 tiles, whole k steps per half, operand rows movable as 16-byte pieces
static bool strassen_shape(const gp_ctx* c, long M, long N, long K) { return strassen_shape_rule(c->strassen_v, M, N, K); }
// side of the off-diagonal block the lower SYRK of side m is split at (multiple of 256); 0: no split
static long strassen_split(const gp_ctx* c, long m, long K) { return strassen_split_rule(c->strassen_v, m, K); }

static int32_t gemm_nt_strassen(gp_ctx* c, hipStream_t s, const StrassenWs& ws, double* C, long ldc, const double* A, long lda, const double* B, long ldb,
                                long M, long N, long K) {
    if (!strassen_shape(c, M, N, K) || !ws.p || ws.elems < strassen_ws_elems(c, M, N, K) || lda % 2 || ldb % 2 || (((uintptr_t)A | (uintptr_t)B) & 15))
        return launch_gemm<double>(c, s, C, ldc, A, lda, B, ldb, M, N, K, plain_map(0, 0, 0));
    const long mh = M / 2, nh = N / 2, kh = K / 2, lds = kh + c->ldpad;
    const long pa = mh * lds, pb = nh * lds;
    double* const SA = ws.p;            // A11+A22, A21+A22, A11+A12, A21−A11, A12−A22
    double* const SB = ws.p + 5 * pa;   // B11+B22, B21−B22, B12−B11, B11+B21, B12+B22
    hipLaunchKernelGGL(strassen_sums_kernel<double>, dim3((unsigned)((mh * (kh / 2) + 255) / 256)), dim3(256), 0, s, A, lda, (int)mh, (int)kh, (int)lds, 0, SA, pa);
    hipLaunchKernelGGL(strassen_sums_kernel<double>, dim3((unsigned)((nh * (kh / 2) + 255) / 256)), dim3(256), 0, s, B, ldb, (int)nh, (int)kh, (int)lds, 1, SB, pb);
    HIPCHK(hipGetLastError());
    // one launch: `nb` products with disjoint targets (product b: operands a + b·as, b + b·bs, first target c1 + b·cs, second target c2off + b·c2s from it)
    auto prod = [&](int nb, double* c1, long cs, long c2off, long c2s, int s1, int s2, const double* a, long la, long as, const double* b, long lb, long bs) -> int32_t {
        GridMap g = plain_map(0, 0, 0);
        g.beta0 = 1;
        g.c2off = c2off;
        g.c2stride = c2s;
        g.s1 = s1;
        g.s2 = s2;
        g.nbatch = nb;
        g.cstride = cs;
        g.astride = as;
        g.bstride = bs;
        return launch_gemm<double>(c, s, c1, ldc, a, la, b, lb, mh, nh, kh, g);
    };
    const long dn = nh, dm = mh * ldc;  // C11 = C, C12 = C + dn, C21 = C + dm, C22 = C + dm + dn
    // Products whose targets do not meet share a launch (a launch ends with a partly filled round of workgroups: four of them instead of seven); every quadrant
    // still receives its products in one fixed order.
    //   M1 = (A11+A22)(B11+B22)ᵀ -> C11, C22
    RC(prod(1, C, 0, dm + dn, 0, 1, 1, SA, lds, 0, SB, lds, 0));
    //   M2 = (A21+A22) B11ᵀ -> C21, −C22   |   M5 = (A11+A12) B22ᵀ -> C12, −C11
    RC(prod(2, C + dm, dn - dm, dn, -2 * dn, 1, -1, SA + pa, lds, pa, B, ldb, nh * ldb + kh));
    //   M3 = A11 (B21−B22)ᵀ -> C12, C22    |   M4 = A22 (B12−B11)ᵀ -> C11, C21
    RC(prod(2, C + dn, -dn, dm, 0, 1, 1, A, lda, mh * lda + kh, SB + pb, lds, pb));
    //   M6 = (A21−A11)(B11+B21)ᵀ -> C22    |   M7 = (A12−A22)(B12+B22)ᵀ -> C11
    RC(prod(2, C + dm + dn, -(dm + dn), 0, 0, 1, 0, SA + 3 * pa, lds, pa, SB + 3 * pb, lds, pb));
    return 0;
}

// Lower SYRK C(m×m) −= P·Pᵀ (P = mrows × K; rows [m, mrows) of C are the carried rows below the square, updated over all m columns; row0: the
// square's offset on the global diagonal).  Split by rows at h: two half-size SYRKs on the diagonal (recursively) and the block between them,
// which carries half the flops, in the Strassen form.  Below the threshold: the one launch this always was.
static int32_t syrk_lower_split(gp_ctx* c, hipStream_t s, const StrassenWs& ws, double* C, long ldc, const double* P, long ldp, long mrows, long m, long K,
                                long row0) {
    const long h = ws.p ? strassen_split(c, m, K) : 0;
    if (h == 0) return launch_gemm<double>(c, s, C, ldc, P, ldp, P, ldp, mrows, m, K, plain_map(1, row0, row0));
    const long b = m - h, bs = b / 256 * 256;  // rows below the split; the Strassen block takes whole 256-row pieces of them
    RC(syrk_lower_split(c, s, ws, C, ldc, P, ldp, h, h, K, row0));
    RC(gemm_nt_strassen(c, s, ws, C + h * ldc, ldc, P + h * ldp, ldp, P, ldp, bs, h, K));
    if (b > bs) RC(launch_gemm<double>(c, s, C + (h + bs) * ldc, ldc, P + (h + bs) * ldp, ldp, P, ldp, b - bs, h, K, plain_map(0, 0, 0)));
    RC(syrk_lower_split(c, s, ws, C + h * ldc + h, ldc, P + h * ldp, ldp, b, b, K, row0 + h));
    if (mrows > m) RC(launch_gemm<double>(c, s, C + m * ldc, ldc, P + m * ldp, ldp, P, ldp, mrows - m, m, K, plain_map(0, 0, 0)));
    return 0;
}
// workspace of the above for a SYRK of side m (its largest Strassen block has at most m/2 + 255 rows and m/2 columns); 0 bytes: nothing is split
static size_t syrk_split_ws_elems(const gp_ctx* c, long m, long K) {
    return strassen_split(c, m, K) ? strassen_ws_elems(c, m / 2 + 256, m / 2 + 256, K) : 0;
}

// ------------------------------------------------------------------------------------------------
// Grouped form of a bulk update ("strassen_group", "strassen_group_min_rows"; bulk_plan.hpp): the sums of every Strassen block, then FOUR launches of
// gemm_nt_grp_kernel over the tiles of all pieces of the update.  The tables of all grouped updates of a call are built before its first launch and
// travel in one async copy from page-locked memory.  In steady state no host wait lands between the Gram assembly and the first panel or inside the panel loop;
// the FIRST call on a ctx (and a later call with larger tables) allocates the page-locked staging buffer at that point, once.  "xcd_swizzle" keeps the per-block
// sequence: the grouped kernel enumerates row-major / compact_tile only.
// ------------------------------------------------------------------------------------------------
static bool group_applies(const gp_ctx* c, long m, long K, long ldp, const double* P) {
    return c->strassen_group && !c->xcd_swizzle && m >= c->strassen_group_min_rows && strassen_split(c, m, K) != 0 && ldp % 2 == 0 && ((uintptr_t)P & 15) == 0;
}
struct GroupedUpdate {
    BulkPlan plan;
    const double* P = nullptr;
    size_t tab0[4] = {0, 0, 0, 0};  // first entry of launch l in the call's table
};
struct PlanTables {
    std::vector<GroupedUpdate> upd;
    std::vector<GrpProb> host;
    size_t ws_elems = 0;  // the updates of a call are ordered on one stream and share the workspace: the largest plan's
    GrpProb* dev = nullptr;
    void add(const gp_ctx* c, long mrows, long m, long K, long row0, long ldc, const double* P, long ldp) {
        GroupedUpdate u;
        u.plan = bulk_plan_build(mrows, m, K, row0, ldc, ldp, c->strassen_v, c->ldpad);
        u.P = P;
        ws_elems = std::max(ws_elems, u.plan.ws_elems);
        upd.push_back(std::move(u));
    }
    // U1 of a panel step in the Strassen form (bulk_plan.hpp u1_plan_build): an update like the others — same tables, same upload, same run_grouped
    void add_u1(const gp_ctx* c, long mrows, long mrect, long nb1, long K, long row0, long ldc, const double* P, long ldp) {
        GroupedUpdate u;
        u.plan = u1_plan_build(mrows, mrect, nb1, K, row0, ldc, ldp, c->ldpad);
        u.P = P;
        ws_elems = std::max(ws_elems, u.plan.ws_elems);
        upd.push_back(std::move(u));
    }
    // the table entries (absolute pointers) and their upload on stream s, in front of everything that reads them
    int32_t upload(gp_ctx* c, hipStream_t s, DevBufs& bufs, const std::vector<double*>& Cs, const double* ws) {
        for (size_t i = 0; i < upd.size(); ++i)
            for (int l = 0; l < 4; ++l) {
                upd[i].tab0[l] = host.size();
                for (const PlanProb& e : upd[i].plan.list[l]) host.push_back(plan_entry(upd[i].plan, e, Cs[i], upd[i].P, ws));
            }
        if (host.empty()) return 0;
        const size_t bytes = host.size() * sizeof(GrpProb);
        void* p = nullptr;
        RC(bufs.get(bytes, &p));
        dev = (GrpProb*)p;
        if (!c->plan_ev) HIPCHK(hipEventCreateWithFlags(&c->plan_ev, hipEventDisableTiming));
        HIPCHK(hipEventSynchronize(c->plan_ev));  // the previous call's copy out of the staging buffer (long done: its call has returned its results)
        if (c->plan_pin_bytes < bytes) {
            if (c->plan_pin) (void)hipHostFree(c->plan_pin);
            c->plan_pin = nullptr;
            c->plan_pin_bytes = 0;
            HIPCHK(hipHostMalloc(&c->plan_pin, bytes + bytes / 4 + 4096, hipHostMallocDefault));
            c->plan_pin_bytes = bytes + bytes / 4 + 4096;
        }
        memcpy(c->plan_pin, host.data(), bytes);
        HIPCHK(hipMemcpyAsync(dev, c->plan_pin, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->plan_ev, s));
        return 0;
    }
};

// one grouped launch: the tiles [0, ntiles) of table entries [tab, tab + nprob)
static int32_t launch_gemm_grp(gp_ctx* c, hipStream_t s, const GrpProb* tab, long nprob, long ntiles, double flops, double bytes, long K) {
    if (nprob <= 0 || ntiles <= 0) return 0;
    gp_ctx::GemmRec rec{};
    const bool timed = c->time_kernels != 0;
    if (timed) {
        RC(ctx_event(c, &rec.a, true));
        RC(ctx_event(c, &rec.b, true));
        rec.flops = flops;
        rec.bytes = bytes;
        rec.M = 0; rec.N = 0; rec.K = K;  // no single shape: the problems and tiles are recorded instead (GPMI_DUMP_GEMM prints them)
        rec.nprob = nprob; rec.ntiles = ntiles;
        rec.stream = (s == c->sp);
        HIPCHK(hipEventRecord(rec.a, s));
    }
    const long pad = c->gemm_pad_user ? c->gemm_pad_lds : 0;  // "gemm_pad_lds" applies as in launch_gemm
    if (pad > 0 && !c->grp_pad_set) {
        HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_grp_kernel<double, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
        HIPCHK(hipFuncSetAttribute((const void*)gemm_nt_grp_kernel<double, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768));
        c->grp_pad_set = true;
    }
    if (c->gemm_pipe) hipLaunchKernelGGL((gemm_nt_grp_kernel<double, 1>), dim3((unsigned)ntiles), dim3(256), (size_t)pad, s, tab, (int)nprob);
    else hipLaunchKernelGGL((gemm_nt_grp_kernel<double, 0>), dim3((unsigned)ntiles), dim3(256), (size_t)pad, s, tab, (int)nprob);
    HIPCHK(hipGetLastError());
    if (timed) {
        HIPCHK(hipEventRecord(rec.b, s));
        c->gemm_recs.push_back(rec);
    }
    return 0;
}

static int32_t run_grouped(gp_ctx* c, hipStream_t s, const PlanTables& T, size_t i, double* ws) {
    const GroupedUpdate& u = T.upd[i];
    const BulkPlan& p = u.plan;
    for (const PlanSums& j : p.sums)  // P is not written by the update: every block's sums go first, each into its own slice
        hipLaunchKernelGGL(strassen_sums_kernel<double>, dim3((unsigned)((j.rh * (j.kh / 2) + 255) / 256)), dim3(256), 0, s, u.P + j.x_off, p.ldp, (int)j.rh, (int)j.kh,
                           (int)p.lds, j.side, ws + j.s_off, j.pstride);
    HIPCHK(hipGetLastError());
    for (int l = 0; l < 4; ++l)
        RC(launch_gemm_grp(c, s, T.dev + u.tab0[l], (long)p.list[l].size(), p.ntiles[l], p.flops[l], p.bytes[l], p.list[l].empty() ? 0 : p.list[l].front().K));
    return 0;
}

static long split_half(long n) {  // largest multiple of 64 that is <= n/2 (>= 64)
    long h = (n / 128) * 64;
    return h < 64 ? 64 : h;
}

// one fused 64-column leaf (panel64_kernel): tile Cholesky (replicated per workgroup) + X L⁻ᵀ of all rows below, after the
// in-leaf update by the kpre column tiles to its left
template <typename T>
static int32_t launch_leaf(gp_ctx* c, hipStream_t s, T* A, long lda, long j0, long mtot, int* info_dev, long gcol0, long n_valid,
                           double* logdet_dev, int kpre) {
    const long mrows = mtot - j0 - 64;
    const unsigned nblk = (unsigned)std::max(1L, (mrows + 127) / 128);
    if (!c->ticket_dev) {
        HIPCHK(hipMalloc((void**)&c->ticket_dev, sizeof(int) * 64));
        // null-stream memsets are not ordered against the (non-blocking) ctx streams: zero it and wait
        HIPCHK(hipMemset(c->ticket_dev, 0, sizeof(int) * 64));
        HIPCHK(hipDeviceSynchronize());
    }
    int* const tk = c->ticket_dev + (s == c->sp ? 32 : 0);
    if constexpr (std::is_same<T, double>::value) {
        if (c->leaf_v2) {  // register-resident leaf (leaf.hip: panel64v2_kernel)
            HIPCHK((hipError_t)launch_leaf_v2(s, (double*)(A + j0 * lda + j0), lda, mrows, info_dev, (int)(gcol0 + j0), (int)n_valid, logdet_dev, tk, kpre,
                                              c->leaf_xr, c->num_cus, 64));
            return 0;
        }
    }
    hipLaunchKernelGGL(panel64_kernel<T>, dim3(nblk), dim3(256), 0, s, A + j0 * lda + j0, lda, (int)mrows, info_dev,
                       (int)(gcol0 + j0), (int)n_valid, logdet_dev, tk, kpre);
    HIPCHK(hipGetLastError());
    return 0;
}

// Factor columns [j0, j0+n) of the row-major matrix A (n multiple of 64) including all rows below
// (rows [j0, mtot)).  Recursive: left half, MFMA update of the right half, right half.
template <typename T>
static int32_t potrf_rec(gp_ctx* c, hipStream_t s, T* A, long lda, long j0, long n, long mtot, int* info_dev,
                         long gcol0, long n_valid, double* logdet_dev) {
    if (n <= 64) return launch_leaf<T>(c, s, A, lda, j0, mtot, info_dev, gcol0, n_valid, logdet_dev, 0);
    if constexpr (std::is_same<T, double>::value) {
        if (n == 128 && c->leaf_v2 && c->leaf_cols == 128 && c->leaf_group >= 128) {  // one 128-column register-resident leaf (leaf.hip)
            if (!c->ticket_dev) {
                HIPCHK(hipMalloc((void**)&c->ticket_dev, sizeof(int) * 64));
                HIPCHK(hipMemset(c->ticket_dev, 0, sizeof(int) * 64));
                HIPCHK(hipDeviceSynchronize());
            }
            int* const tk = c->ticket_dev + (s == c->sp ? 32 : 0);
            HIPCHK((hipError_t)launch_leaf_v2(s, (double*)(A + j0 * lda + j0), lda, mtot - j0 - 128, info_dev, (int)(gcol0 + j0), (int)n_valid, logdet_dev, tk, 0,
                                              c->leaf_xr, c->num_cus, 128));
            return 0;
        }
    }
    if (n <= c->leaf_group) {  // left-looking group: leaf t first applies the t tiles to its left itself
        for (long t = 0; t < n / 64; ++t)
            RC(launch_leaf<T>(c, s, A, lda, j0 + 64 * t, mtot, info_dev, gcol0, n_valid, logdet_dev, (int)t));
        return 0;
    }
    const long h = split_half(n);
    RC(potrf_rec<T>(c, s, A, lda, j0, h, mtot, info_dev, gcol0, n_valid, logdet_dev));
    bool skinny = false;
    if constexpr (std::is_same<T, double>::value) {
        const long mrows = mtot - j0 - h;
        const bool k128 = h == 128 && n - h == 128 && c->upd128;
        const bool kmid = h >= 256 && h <= c->updk_max_k && h % 32 == 0 && (n - h) % 128 == 0 && n - h <= h && (h <= c->updk_tall_k || mrows <= c->updk_tall_m);
        if (c->leaf_v2 && (k128 || kmid)) {  // the skinny in-panel updates through the register chain (leaf.hip panel_updk_kernel)
            HIPCHK((hipError_t)launch_panel_updk(s, (double*)(A + (j0 + h) * lda + (j0 + h)), lda, (const double*)(A + (j0 + h) * lda + j0), lda, mrows, n - h, h,
                                                 c->updk_rt, c->num_cus));
            skinny = true;
        }
    }
    if (!skinny)
        RC(launch_gemm<T>(c, s, A + (j0 + h) * lda + (j0 + h), lda, A + (j0 + h) * lda + j0, lda,
                          A + (j0 + h) * lda + j0, lda, mtot - j0 - h, n - h, h, plain_map(1, j0 + h, j0 + h)));
    RC(potrf_rec<T>(c, s, A, lda, j0 + h, n - h, mtot, info_dev, gcol0, n_valid, logdet_dev));
    return 0;
}

// W_j = I − inv(L_jj) for every 64×64 diagonal tile of a lower factor (one batched launch; the 64-wide steps of the vector solves)
template <typename T> static int32_t trtri_tiles(gp_ctx* c, hipStream_t s, const T* L, long ldl, long n, T** Wout) {
    const size_t need = sizeof(T) * (size_t)(n / 64 + 2) * 4096;  // + slack tiles (B-operand over-read of gemm_nt)
    if (c->w_ws_bytes < need) {
        HIPCHK(hipStreamSynchronize(c->sm));
        HIPCHK(hipStreamSynchronize(c->sp));
        if (c->w_ws) (void)hipFree(c->w_ws);
        c->w_ws_bytes = 0;
        HIPCHK(hipMalloc(&c->w_ws, need));
        HIPCHK(hipMemsetAsync(c->w_ws, 0, need, s));  // same stream as the trtri launch that follows
        if (c->alloc_poison) {
            HIPCHK(hipStreamSynchronize(s));
            RC(ctx_poison(c, c->w_ws, need));
        }
        c->w_ws_bytes = need;
    }
    hipLaunchKernelGGL(trtri_64_kernel<T>, dim3((unsigned)(n / 64)), dim3(64), 0, s, L, ldl, (T*)c->w_ws);
    HIPCHK(hipGetLastError());
    *Wout = (T*)c->w_ws;
    return 0;
}
// 64-wide TRSM leaf on the matrix pipe (trsm64_mfma, one workgroup per 128 rows)
template <typename T>
static int32_t launch_trsm64(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, const T* L, long ldl) {
    (void)c;
    if (M <= 0) return 0;
    hipLaunchKernelGGL(trsm64_mfma_kernel<T>, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, s, X, ldx, (int)M, L, ldl);
    HIPCHK(hipGetLastError());
    return 0;
}

// Inverse diagonal blocks ("DIB") of a resident factor.  A forward solve X ← X L⁻ᵀ by recursion ends in N/64 latency-bound leaf launches
// and as many few-tile GEMMs (C4, 4 096 test points: 2 047 launches; the levels below 2 048 columns hold 3 % of the flops and a third of
// the time).  With W_b = −inv(L_bb) of every diagonal block (j0, n <= nbi) at hand, the leaf of the recursion at that size is ONE
// triangular-k MFMA GEMM  S = −X_b W_bᵀ = X_b L_bb⁻ᵀ  (B operand lower triangular: GridMap::ktri = 3) into a scratch panel that is copied
// back; everything above it stays the recursion's large-K GEMMs.  The blocks are the leaves the recursion itself reaches (dib_ranges).
template <typename T> struct DibArgs {
    const T* W = nullptr;  // −inv(L_bb), rows shifted along with L (block (j0, n): rows [j0, j0 + n), columns [0, n))
    long ldw = 0, nbi = 0;
    T* S = nullptr;        // scratch panel, at least (rows + 128) × lds
    long lds = 0;
};
static void dib_ranges(long j0, long n, long nbi, std::vector<std::pair<long, long>>& out) {
    if (n <= nbi) {
        out.push_back({j0, n});
        return;
    }
    const long h = split_half(n);
    dib_ranges(j0, h, nbi, out);
    dib_ranges(j0 + h, n - h, nbi, out);
}
// S = −X W_bᵀ (M × n), then X ← S
template <typename T>
static int32_t dib_apply(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, long n, const DibArgs<T>& dib) {
    if (M <= 0) return 0;
    GridMap g = plain_map(0, 0, 0);
    g.beta0 = 1;
    g.ktri = 3;
    RC(launch_gemm<T>(c, s, dib.S, dib.lds, X, ldx, dib.W, dib.ldw, M, n, n, g));
    HIPCHK(hipMemcpy2DAsync(X, sizeof(T) * ldx, dib.S, sizeof(T) * dib.lds, sizeof(T) * n, M, hipMemcpyDeviceToDevice, s));
    return 0;
}

// X[M×n] ← X · L⁻ᵀ with L the n×n row-major lower factor (n, M multiples of 64): left half; X_right −= X_left · L_21ᵀ (MFMA GEMM);
// right half; leaves: the explicit inverse block (dib, n <= nbi) or 64-wide trsm64_mfma.
template <typename T>
static int32_t trsm_rec_v(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, const T* L, long ldl, long n, DibArgs<T> dib = DibArgs<T>()) {
    if (dib.W && n <= dib.nbi) return dib_apply<T>(c, s, X, ldx, M, n, dib);
    if (n <= 64) return launch_trsm64<T>(c, s, X, ldx, M, L, ldl);
    const long h = split_half(n);
    RC(trsm_rec_v<T>(c, s, X, ldx, M, L, ldl, h, dib));
    RC(launch_gemm<T>(c, s, X + h, ldx, X, ldx, L + h * ldl, ldl, M, n - h, h, plain_map(0, 0, 0)));
    if (dib.W) dib.W += h * dib.ldw;
    RC(trsm_rec_v<T>(c, s, X + h, ldx, M, L + h * ldl + h, ldl, n - h, dib));
    return 0;
}
// W ← W L⁻ᵀ for W that is upper triangular on entry AND exit (W = I gives L⁻ᵀ): columns [j0, j0+n) only ever have
// non-zeros in rows [0, j0+n), so every step is restricted to those rows — N³/3 flops instead of the N³ of the general
// solve.  Same recursion as trsm_rec_v.  With dib (W indexed by GLOBAL row here): the diagonal blocks of X already hold L_bb⁻ᵀ (written
// by dib_build), a leaf only multiplies the rows above its block.
template <typename T>
static int32_t trsm_upper_rec(gp_ctx* c, hipStream_t s, T* X, long ldx, const T* L, long ldl, long j0, long n, DibArgs<T> dib = DibArgs<T>()) {
    if (dib.W && n <= dib.nbi) {
        DibArgs<T> d2 = dib;
        d2.W = dib.W + j0 * dib.ldw;
        return dib_apply<T>(c, s, X + j0, ldx, j0, n, d2);
    }
    if (n <= 64) return launch_trsm64<T>(c, s, X + j0, ldx, j0 + 64, L + j0 * ldl + j0, ldl);
    const long h = split_half(n);
    RC(trsm_upper_rec<T>(c, s, X, ldx, L, ldl, j0, h, dib));
    {
        // A = X[0 : j0+h, j0 : j0+h]: rows below j0 hold the h×h UPPER-triangular block just solved — its leading zeros are skipped on launches
        // large enough for the hardware-dispatched kernel (until round 5 this product ran over the whole k range: N³/2 flops for L⁻ᵀ instead
        // of N³/3; the few-tile launches keep the full range and their stream-K cut)
        GridMap g = plain_map(0, 0, 0);
        if (h >= 512 && ((j0 + h) / 128) * ((n - h + 127) / 128) > c->sk_max_tiles / 8) {
            g.ktri = 2;
            g.ktri_off = (int)j0;
        }
        RC(launch_gemm<T>(c, s, X + j0 + h, ldx, X + j0, ldx, L + (j0 + h) * ldl + j0, ldl, j0 + h, n - h, h, g));
    }
    RC(trsm_upper_rec<T>(c, s, X, ldx, L, ldl, j0 + h, n - h, dib));
    return 0;
}

template <typename T>
static int32_t trsm_rec(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, const T* L, long ldl, long n, DibArgs<T> dib = DibArgs<T>()) {
    if (M <= 0) return 0;
    return trsm_rec_v<T>(c, s, X, ldx, M, L, ldl, n, dib);
}

// W (rows [0, np + 128) × ldw, zero on entry is NOT required) ← −inv(L_bb) for every block of dib_ranges(0, np, nbi); Iw: scratch of the same
// shape.  Per block: Iw_b = I, Iw_b ← Iw_b L_bb⁻ᵀ (upper; the restricted-row recursion above, without dib), W_b = −Iw_bᵀ.  up != nullptr:
// the upper blocks L_bb⁻ᵀ are also written onto the diagonal of `up` (the gradient's L⁻ᵀ).
template <typename T>
static int32_t dib_build(gp_ctx* c, hipStream_t s, const T* L, long ldl, long np, long nbi, T* W, long ldw, T* Iw, T* up, long ldu) {
    std::vector<std::pair<long, long>> blocks;
    dib_ranges(0, np, nbi, blocks);
    HIPCHK(hipMemsetAsync(Iw, 0, sizeof(T) * (size_t)(np + 128) * ldw, s));
    HIPCHK(hipMemsetAsync(W, 0, sizeof(T) * (size_t)(np + 128) * ldw, s));
    bool uniform = blocks.size() > 1;
    for (const auto& b : blocks) uniform = uniform && b.second == blocks[0].second;
    if (uniform) {  // equal blocks (np a power-of-two multiple of the block): the whole batch per launch
        const long n = blocks[0].second, nb = (long)blocks.size(), xs = n * ldw, ls = n * ldl + n;
        hipLaunchKernelGGL(diag_ones_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)nb), dim3(256), 0, s, Iw, ldw, n, xs);
        HIPCHK(hipGetLastError());
        RC(trsm_upper_rec_batched<T>(c, s, Iw, ldw, L, ldl, 0, n, nb, xs, ls));
        hipLaunchKernelGGL(transpose_scale_kernel<T>, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32), (unsigned)nb), dim3(256), 0, s, (const T*)Iw, ldw,
                           W, ldw, n, T(-1), xs, xs);
        HIPCHK(hipGetLastError());
        if (up)
            for (const auto& b : blocks)
                HIPCHK(hipMemcpy2DAsync(up + b.first * ldu + b.first, sizeof(T) * ldu, Iw + b.first * ldw, sizeof(T) * ldw, sizeof(T) * n, n, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    for (const auto& b : blocks) {
        const long j0 = b.first, n = b.second;
        T* Ib = Iw + j0 * ldw;
        hipLaunchKernelGGL(identity_kernel<T>, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, s, Ib, ldw, n);
        HIPCHK(hipGetLastError());
        RC(trsm_upper_rec<T>(c, s, Ib, ldw, L + j0 * ldl + j0, ldl, 0, n));
        hipLaunchKernelGGL(transpose_scale_kernel<T>, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, s, (const T*)Ib, ldw,
                           W + j0 * ldw, ldw, n, T(-1));
        HIPCHK(hipGetLastError());
        if (up) HIPCHK(hipMemcpy2DAsync(up + j0 * ldu + j0, sizeof(T) * ldu, Ib, sizeof(T) * ldw, sizeof(T) * n, n, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// The restricted-row recursion of trsm_upper_rec for `nb` equal blocks at once (block b: X + b·xs against L + b·ls): every launch of the recursion
// carries the whole batch (trsm64 leaves: grid.y; GEMMs: grid.z with independent operand strides), so the inverse blocks of a factor cost the ≈ 63
// launches of ONE 2 048-column block instead of N/2 048 times that (C4: 32 × 0.6 ms of serial chains -> ≈ 1 ms).
template <typename T>
static int32_t trsm_upper_rec_batched(gp_ctx* c, hipStream_t s, T* X, long ldx, const T* L, long ldl, long j0, long n, long nb, long xs, long ls) {
    if (n <= 64) {
        hipLaunchKernelGGL(trsm64_mfma_kernel<T>, dim3((unsigned)((j0 + 64 + 127) / 128), (unsigned)nb), dim3(256), 0, s, X + j0, ldx, (int)(j0 + 64),
                           L + j0 * ldl + j0, ldl, xs, ls);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const long h = split_half(n);
    RC(trsm_upper_rec_batched<T>(c, s, X, ldx, L, ldl, j0, h, nb, xs, ls));
    GridMap g = plain_map(0, 0, 0);
    g.nbatch = (int)nb;
    g.cstride = xs;
    g.astride = xs;
    g.bstride = ls;
    RC(launch_gemm<T>(c, s, X + j0 + h, ldx, X + j0, ldx, L + (j0 + h) * ldl + j0, ldl, j0 + h, n - h, h, g));
    RC(trsm_upper_rec_batched<T>(c, s, X, ldx, L, ldl, j0 + h, n - h, nb, xs, ls));
    return 0;
}

// The forward solve X ← X L⁻ᵀ against a RESIDENT factor L (np × np, nvalid real rows) with the inverse diagonal blocks kept in `cache` beside it: built on
// first use (kept until the owner of the factor is freed), then the recursion runs with them.  X: M × np (+ 128 slack rows).
template <typename T>
static int32_t trsm_cached(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, const T* A, long ld, long np, long nvalid, DibCache& cache, DevBufs& bufs) {
    if (M <= 0) return 0;
    if (c->dib_nb < 128 || np < c->dib_nb || cache.nbi < 0) return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
    const long nbi = round_up(c->dib_nb, 128), ldw = nbi + c->ldpad;
    // a handful of rows never repays the build (≈ np·nbi elements allocated, zeroed and inverted: a sequential-conditioning loop with tiny batches would pay
    // it for every new handle): blocks that exist are used, new ones are built from 128 rows on
    if (!cache.w && M < 128) return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
    if (!cache.w) {
        // guard: a product with an explicit inverse carries an error of order cond(L_bb)·ε where substitution is backward stable.  max / min of the
        // factor's diagonal bounds cond(L) from below; beyond the limit — 1e5 in fp64 (cond(K + Σy) >= 1e10: interpolation-style fits with vanishing
        // noise), 300 ≈ √(1/ε)/10 in fp32 — this factor keeps the recursion with substitution leaves for good (nbi = −1)
        const double limit = sizeof(T) == 8 ? 1e5 : 300.0;
        RC(ctx_scal(c, 16));
        hipLaunchKernelGGL(diag_minmax_kernel<T>, dim3(1), dim3(1024), 0, s, A, ld, nvalid, c->scal_dev + 6);
        HIPCHK(hipGetLastError());
        double mm[2] = {1.0, 1.0};
        HIPCHK(hipMemcpyAsync(mm, c->scal_dev + 6, sizeof(mm), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!(mm[0] > 0.0) || mm[1] / mm[0] > limit) {
            cache.nbi = -1;
            return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
        }
    }
    const size_t wb = sizeof(T) * (size_t)(np + 128) * ldw;
    if (!cache.w || cache.nbi != nbi) {
        if (cache.w) ctx_release(c, cache.w, cache.bytes);
        cache.w = nullptr;
        void* w = nullptr;
        void* iw = nullptr;
        // no memory for the blocks (W) or the build's workspace (Iw): the solve itself needs neither — substitution leaves, this call only
        if (ctx_alloc(c, wb, &w) != 0) return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
        if (bufs.get(wb, &iw) != 0) {
            ctx_release(c, w, wb);
            return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
        }
        int32_t rc = dib_build<T>(c, s, A, ld, np, nbi, (T*)w, ldw, (T*)iw, (T*)nullptr, 0);
        if (rc != 0) {
            (void)hipStreamSynchronize(s);
            ctx_release(c, w, wb);
            return rc;
        }
        cache.w = w; cache.bytes = wb; cache.nbi = nbi; cache.ldw = ldw;
    }
    // S: ONE panel per API call (DevBufs::scratch), shared by the chunks of a large prediction — allocated per call of this function it grew with the
    // number of test points (70 MB per 4 096-row chunk: 17 GB beside the factor for 10⁶ points)
    void* S_v = nullptr;
    const long lds = nbi + c->ldpad;
    if (bufs.scratch(sizeof(T) * (size_t)(M + 128) * lds, &S_v) != 0) return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np);
    DibArgs<T> dib;
    dib.W = (const T*)cache.w; dib.ldw = ldw; dib.nbi = nbi; dib.S = (T*)S_v; dib.lds = lds;
    return trsm_rec_v<T>(c, s, X, ldx, M, A, ld, np, dib);
}
template <typename T>
static int32_t trsm_post(gp_post* post, hipStream_t s, T* X, long ldx, long M, DevBufs& bufs) {
    return trsm_cached<T>(post->ctx, s, X, ldx, M, (const T*)post->A, post->ld, post->np, post->n, post->dibc, bufs);
}

// The backward solve X (M × np, + 128 slack rows; Mvalid real rows) ← X L⁻¹ against the same resident factor, the counterpart of trsm_cached (with it a row of
// X becomes (C⁻¹k)ᵀ: the weights of the predictive variance's gradient).  It runs AFTER a forward solve on the handle and uses the inverse diagonal blocks that
// solve left in `cache`, walking the blocks of dib_ranges from the last to the first:
//   diagonal step      X_b ← X_b L_bb⁻¹ = −X_b W_b: ONE NT GEMM against the TRANSPOSED cached block (full k range: the transposed block is upper triangular, a
//                      shape no triangular-k map covers) into the forward solve's scratch panel, copied back;
//   off-diagonal step  X[:, 0:j0] −= X_b · L[b, 0:j0]: ONE NT GEMM whose B operand is the block row of L transposed into scratch.
// Both transposes (transpose_rect_kernel) go through ONE scratch of (np + 128) × ldw elements — the size of the cache, no second N×N buffer — that `ws`
// keeps for the chunks of a call (zeroed once: the GEMM over-reads B up to the next multiple of 128 rows).  No host synchronisation.
// Without blocks ("dib_nb" = 0, np < "dib_nb", or the conditioning guard nbi = −1) the rows go through the vector solve trsv(fwd = false) — they already are in
// its right-hand-side layout.  That path is SERIAL in the number of rows (one pass of the block sweep per row inside every launch), and it is also what a
// call falls back to when the transpose scratch or the S panel cannot be allocated.  The ratios measured against the forward solve (predict_grad_impl) are
// those of the BLOCKED path; the substitution path's cost grows with rows × np / 256 diagonal solves of ≈ 10 µs each (measured: include/gpmi355.h).
struct BackWs {
    void* bt = nullptr;
};
template <typename T>
static int32_t trsv(gp_ctx* c, hipStream_t s, const T* L, long ldl, long np, T* R, long ldr, int nrhs, bool fwd);
template <typename T>
static int32_t trsm_back_cached(gp_ctx* c, hipStream_t s, T* X, long ldx, long M, long Mvalid, const T* A, long ld, long np, const DibCache& cache,
                                DevBufs& bufs, BackWs& ws) {
    if (M <= 0 || Mvalid <= 0) return 0;
    if (!cache.w || cache.nbi < 128 || c->dib_nb < 128) return trsv<T>(c, s, A, ld, np, X, ldx, (int)Mvalid, false);
    const long nbi = cache.nbi, ldw = cache.ldw;
    if (!ws.bt) {
        const size_t wb = sizeof(T) * (size_t)(np + 128) * ldw;
        void* S_probe = nullptr;
        if (bufs.get(wb, &ws.bt) != 0 || bufs.scratch(sizeof(T) * (size_t)(M + 128) * ldw, &S_probe) != 0) {
            ws.bt = nullptr;
            return trsv<T>(c, s, A, ld, np, X, ldx, (int)Mvalid, false);
        }
        HIPCHK(hipMemsetAsync(ws.bt, 0, wb, s));
    }
    void* S_v = nullptr;
    RC(bufs.scratch(sizeof(T) * (size_t)(M + 128) * ldw, &S_v));
    T* Bt = (T*)ws.bt;
    T* S = (T*)S_v;
    const T* W = (const T*)cache.w;
    std::vector<std::pair<long, long>> blocks;
    dib_ranges(0, np, nbi, blocks);
    for (long bi = (long)blocks.size() - 1; bi >= 0; --bi) {
        const long j0 = blocks[bi].first, n = blocks[bi].second;
        hipLaunchKernelGGL(transpose_rect_kernel<T>, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, s, W + j0 * ldw, ldw, Bt, ldw, n, n, 1);
        HIPCHK(hipGetLastError());
        GridMap g = plain_map(0, 0, 0);
        g.beta0 = 1;
        RC(launch_gemm<T>(c, s, S, ldw, X + j0, ldx, Bt, ldw, M, n, n, g));
        HIPCHK(hipMemcpy2DAsync(X + j0, sizeof(T) * ldx, S, sizeof(T) * ldw, sizeof(T) * n, M, hipMemcpyDeviceToDevice, s));
        if (j0 > 0) {
            hipLaunchKernelGGL(transpose_rect_kernel<T>, dim3((unsigned)((j0 + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, s, A + j0 * ld, ld, Bt, ldw, n, j0, 0);
            HIPCHK(hipGetLastError());
            RC(launch_gemm<T>(c, s, X, ldx, X + j0, ldx, Bt, ldw, M, j0, n, plain_map(0, 0, 0)));
        }
    }
    return 0;
}

// Full factorisation of the np×np matrix (rows [np, mtot) are carried RHS rows): right-looking over panels of width nb with a
// one-panel look-ahead (potrf_full_la below); nb = 0: the plain recursion on one stream.
template <typename T>
static int32_t potrf_full_la(gp_ctx* c, T* A, long lda, long np, long mtot, int* info_dev, long n_valid, double* logdet_dev, DevBufs* bufs);

// bufs (the exact fit passes its own): owner of the Strassen workspace of the bulk trailing updates; without it they stay single launches
template <typename T>
static int32_t potrf_full(gp_ctx* c, T* A, long lda, long np, long mtot, int* info_dev, long n_valid,
                          double* logdet_dev, DevBufs* bufs = nullptr) {
    if (c->nb == 0) return potrf_rec<T>(c, c->sm, A, lda, 0, np, mtot, info_dev, 0, n_valid, logdet_dev);
    return potrf_full_la<T>(c, A, lda, np, mtot, info_dev, n_valid, logdet_dev, bufs);
}

// sched 0: right-looking over panels of width nb with a one-panel look-ahead: the whole next panel (recursive
// Cholesky of its columns including every row below) is factored on the panel stream while the rest of the
// trailing update still runs on the main stream.  (A variant with the two streams on disjoint CU sets was built in round 3
// and measured slower at every size in rounds 3 and 4 — profiles/r3/sweep_cusplit.jsonl, profiles/r4/nb_sweep.jsonl; it lives
// in the history at f1ed70e.)
template <typename T>
static int32_t potrf_full_la(gp_ctx* c, T* A, long lda, long np, long mtot, int* info_dev, long n_valid,
                             double* logdet_dev, DevBufs* bufs) {
    long nb = c->nb;
    // "strassen_min_rows_large": the Strassen threshold of the large fits — the ones that take the look-ahead schedule — unless the caller chose one
    c->strassen_v = (!c->strassen_min_rows_set && np >= c->lookahead_min_n) ? c->strassen_min_rows_large : c->strassen_min_rows;
    // below the look-ahead threshold the schedule is one stream anyway: panels of "nb_small" (4 096) columns halve the passes over the trailing matrix
    // (K = 4 096 updates) — C2 29.8-30.1 -> 29.0-29.2 ms on two boxes, N = 8 192 6.51 -> 6.43 (profiles/r5/nb_sweep.txt); from the threshold on
    // "nb_large" = 2 048 (C3's size: 2 048 and 4 096 measure the same, 3 072 and 6 144 slower).  An explicit "nb" >= 0 applies to every size.
    // From "nb_huge_min_n" on (0: no such tier) "nb_huge": the Strassen products of the bulk update then run at K/2 = nb_huge/2, and what a product costs
    // beyond its flops — the dual-target epilogue, the partly filled last round of a launch — does not grow with K (profiles/r26/nb_sweep.txt).
    if (nb < 0) nb = (c->nb_huge_min_n > 0 && np >= c->nb_huge_min_n) ? c->nb_huge : np < c->lookahead_min_n ? c->nb_small : c->nb_large;  // "nb" = −1: automatic
    if (nb <= 0 || nb >= np) return potrf_rec<T>(c, c->sm, A, lda, 0, np, mtot, info_dev, 0, n_valid, logdet_dev);
    nb = round_up(nb, 128);
    const bool la = c->lookahead != 0 && np >= c->lookahead_min_n;
    hipStream_t sM = c->sm, sP = la ? c->sp : c->sm;
    hipEvent_t ev_u1 = nullptr, ev_panel = nullptr;
    StrassenWs ws;  // one workspace of sum panels per fit, sized for the update that needs most; every launch that touches it is ordered on the main stream
    PlanTables tabs;          // the grouped bulk updates of the fit, planned and uploaded before the first panel
    std::vector<long> gidx;   // per panel step: index into tabs.upd, −1: the per-block launch sequence
    std::vector<long> uidx;   // per panel step: index into tabs.upd of U1 in the Strassen form ("strassen_u1_min_rows"), −1: the single launch
    if constexpr (std::is_same<T, double>::value) {
        if (bufs) {
            size_t el = 0;
            std::vector<double*> Cs;
            for (long k = 0; k < np; k += nb) {
                const long nbk = std::min(nb, np - k), k1 = k + nbk;
                if (k1 >= np) break;
                const long k2 = k1 + std::min(nb, np - k1);
                long gi = -1, ui = -1;
                if (k2 < np) {
                    // U1's rectangle below the next panel's square as one Strassen block.  Its sum panels share the fit's workspace with the bulk update of
                    // the same step: U1's sums and four launches, then the bulk update's, all on the main stream, in order.
                    const double* P1 = A + k1 * lda + k;
                    if (c->strassen_v > 0 && !c->xcd_swizzle && lda % 2 == 0 && ((uintptr_t)P1 & 15) == 0 &&
                        u1_block_rows(c->strassen_u1_min_rows, c->strassen_u1_min_k, np - k2, k2 - k1, nbk) > 0) {
                        ui = (long)tabs.upd.size();
                        tabs.add_u1(c, mtot - k1, np - k2, k2 - k1, nbk, k1, lda, P1, lda);
                        Cs.push_back(A + k1 * lda + k1);
                    }
                    const double* P = A + k2 * lda + k;
                    if (group_applies(c, np - k2, nbk, lda, P)) {
                        gi = (long)tabs.upd.size();
                        tabs.add(c, mtot - k2, np - k2, nbk, k2, lda, P, lda);
                        Cs.push_back(A + k2 * lda + k2);
                    } else
                        el = std::max(el, syrk_split_ws_elems(c, np - k2, nbk));
                }
                gidx.push_back(gi);
                uidx.push_back(ui);
            }
            el = std::max(el, tabs.ws_elems);
            if (el) {
                void* p = nullptr;
                RC(bufs->get(sizeof(double) * el, &p));
                ws.p = (double*)p;
                ws.elems = el;
            }
            RC(tabs.upload(c, c->sm, *bufs, Cs, ws.p));
        }
    }
    if (la) {  // the panel stream starts after everything queued so far on the main stream (assembly)
        RC(ctx_event(c, &ev_u1, false));
        HIPCHK(hipEventRecord(ev_u1, c->sm));
        HIPCHK(hipStreamWaitEvent(sP, ev_u1, 0));
    }
    for (long k = 0; k < np; k += nb) {
        const long nbk = std::min(nb, np - k);
        RC(potrf_rec<T>(c, sP, A, lda, k, nbk, mtot, info_dev, 0, n_valid, logdet_dev));
        const long k1 = k + nbk;
        if (la) {
            RC(ctx_event(c, &ev_panel, false));
            HIPCHK(hipEventRecord(ev_panel, sP));
            HIPCHK(hipStreamWaitEvent(sM, ev_panel, 0));
        }
        if (k1 >= np) break;  // RHS rows were already solved inside potrf_rec
        const long nb1 = std::min(nb, np - k1);
        // U1: next panel's columns, all rows below
        bool u1_grouped = false;
        if constexpr (std::is_same<T, double>::value) {
            const size_t step = (size_t)(k / nb);
            if (step < uidx.size() && uidx[step] >= 0) {
                RC(run_grouped(c, sM, tabs, (size_t)uidx[step], ws.p));
                u1_grouped = true;
            }
        }
        if (!u1_grouped)
            RC(launch_gemm<T>(c, sM, A + k1 * lda + k1, lda, A + k1 * lda + k, lda, A + k1 * lda + k, lda, mtot - k1, nb1, nbk, plain_map(1, k1, k1)));
        if (la) {  // the panel stream goes on after U1's last launch
            RC(ctx_event(c, &ev_u1, false));
            HIPCHK(hipEventRecord(ev_u1, sM));
            HIPCHK(hipStreamWaitEvent(sP, ev_u1, 0));
        }
        // U2: the rest of the trailing matrix
        const long k2 = k1 + nb1;
        if (k2 < np) {
            if constexpr (std::is_same<T, double>::value) {
                const size_t step = (size_t)(k / nb);
                if (step < gidx.size() && gidx[step] >= 0) RC(run_grouped(c, sM, tabs, (size_t)gidx[step], ws.p));
                else RC(syrk_lower_split(c, sM, ws, A + k2 * lda + k2, lda, A + k2 * lda + k, lda, mtot - k2, np - k2, nbk, k2));
            } else
                RC(launch_gemm<T>(c, sM, A + k2 * lda + k2, lda, A + k2 * lda + k, lda, A + k2 * lda + k, lda,
                                  mtot - k2, np - k2, nbk, plain_map(1, k2, k2)));
        }
    }
    return 0;
}

// Vector solves with the resident factor: R rows hold nrhs right-hand sides of length np.
// Blocks of trsv_nb (256) columns: a one-workgroup diagonal solve (trsv_diag2: the memory round trips of every 64-wide step are in
// flight before they are needed) and a many-workgroup, HBM-bound update of the remaining vector.
template <typename T>
static int32_t trsv(gp_ctx* c, hipStream_t s, const T* L, long ldl, long np, T* R, long ldr, int nrhs, bool fwd) {
    const int NBV = (int)c->trsv_nb;
    const bool k2 = NBV <= 256;
    const size_t smem = k2 ? sizeof(T) * (256 + 64 * 65 + 16 * 64 + 4 * 256) : sizeof(T) * (NBV + 64 * 65 + 16 * 64);
    const long nblk = (np + NBV - 1) / NBV;
    T* W = nullptr;
    RC(trtri_tiles<T>(c, s, L, ldl, np, &W));  // I − inv(L_jj) for every 64×64 diagonal tile, one batched launch
    for (long bb = 0; bb < nblk; ++bb) {
        const long b = fwd ? bb : (nblk - 1 - bb);
        const long b0 = b * NBV;
        const int nbv = (int)std::min<long>(NBV, np - b0);  // multiple of 64 (np is a multiple of 128)
        if (fwd) {
            if (k2)
                hipLaunchKernelGGL((trsv_diag2_kernel<T, true>), dim3(1), dim3(1024), smem, s, L, ldl, b0, nbv, R, ldr, nrhs, (const T*)W);
            else
                hipLaunchKernelGGL((trsv_diag_kernel<T, true>), dim3(1), dim3(1024), smem, s, L, ldl, b0, nbv, R, ldr, nrhs, (const T*)W);
            HIPCHK(hipGetLastError());
            const long lo = b0 + nbv;
            if (lo < np) {
                hipLaunchKernelGGL(trsv_upd_fwd_kernel<T>, dim3((unsigned)((np - lo + 3) / 4)), dim3(256), 0, s, L,
                                   ldl, b0, nbv, lo, np, R, ldr, nrhs);
                HIPCHK(hipGetLastError());
            }
        } else {
            if (k2)
                hipLaunchKernelGGL((trsv_diag2_kernel<T, false>), dim3(1), dim3(1024), smem, s, L, ldl, b0, nbv, R, ldr, nrhs, (const T*)W);
            else
                hipLaunchKernelGGL((trsv_diag_kernel<T, false>), dim3(1), dim3(1024), smem, s, L, ldl, b0, nbv, R, ldr, nrhs, (const T*)W);
            HIPCHK(hipGetLastError());
            if (b0 > 0) {
                hipLaunchKernelGGL(trsv_upd_bwd_kernel<T>, dim3((unsigned)((b0 + 255) / 256), c->deterministic ? 1u : (unsigned)(nbv / 64)),
                                   dim3(256), 0, s, L, ldl, b0, nbv, R, ldr, nrhs);
                HIPCHK(hipGetLastError());
            }
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// engine entry points for multi.hip (declared in engine.hpp)
// ------------------------------------------------------------------------------------------------
int32_t gpmi::eng_assemble(gp_ctx* c, hipStream_t s, int kind, double variance, const double* x_dev, long n_valid, long n_pad, int d,
                           const double* noise_dev, GridMap g, double* a_loc, long lda, long m_loc, long n_loc) {
    (void)c;
    dim3 grid((unsigned)(n_loc / 128), (unsigned)(m_loc / 128));
    if (grid.x == 0 || grid.y == 0) return 0;
    launch_kmat<double>(grid, s, a_loc, lda, x_dev, n_pad, x_dev, n_pad, d, kind, variance,
                       noise_dev, n_valid, n_valid, 1, g, (const double*)nullptr, (const double*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_potrf(gp_ctx* c, hipStream_t s, double* a, long lda, long m, long n, int* info_dev, long col0, long n_valid,
                        double* logdet_dev) {
    return potrf_rec<double>(c, s, a, lda, 0, n, m, info_dev, col0, n_valid, logdet_dev);
}
int32_t gpmi::eng_trsm(gp_ctx* c, hipStream_t s, double* x, long ldx, long m, const double* l, long ldl, long n) {
    return trsm_rec_v<double>(c, s, x, ldx, m, l, ldl, n);
}
// W ← −inv(L) for ONE nb×nb lower block (the multi-device driver's diagonal block).  W, iw (and v): nb × ldw; the caller keeps 128 finite slack rows below each
// (the operand over-read of the GEMM) and W zero above its diagonal.
//   nb = 64·2^m and a second scratch v given — LEVEL-WISE (round 6): −inv and its transpose of every 64×64 diagonal tile in one launch (trtri_64_neg), then per level
//   s = 64, 128, …, nb/2 and for ALL pairs of the level at once (batched launches): with An = −inv(L11), Cn = −inv(L22) of the level below (lower, in W) and their
//   transposes (upper, in iw),  V = −AnT·L21ᵀ (= (L21·inv(L11))ᵀ),  W21 = −Cn·Vᵀ (= inv(L22)·L21·inv(L11) = −(−inv(L))21),  WT12 = −V·Cnᵀ (its transpose):
//   1 + 3·log2(nb/64) launches (13 at nb = 1 024) where the restricted-row recursion on the identity takes nb/64 substitution leaves and as many few-tile GEMMs (33).
//   iw's lower-left and W's upper-right triangles are never written (the caller zeroed them once).
//   otherwise: Iw = I, Iw ← Iw L⁻ᵀ (upper; the restricted-row recursion), W = −Iwᵀ.
int32_t gpmi::eng_inv_lower(gp_ctx* c, hipStream_t s, const double* l, long ldl, long nb, double* w, long ldw, double* iw, double* v) {
    const long t64 = nb / 64;
    if (v && nb >= 128 && nb % 64 == 0 && (t64 & (t64 - 1)) == 0) {
        hipLaunchKernelGGL(trtri_64_neg_kernel<double>, dim3((unsigned)t64), dim3(64), 0, s, l, ldl, w, iw, ldw);
        HIPCHK(hipGetLastError());
        for (long sz = 64; sz < nb; sz *= 2) {
            GridMap g = plain_map(0, 0, 0);
            g.beta0 = 1;
            g.nbatch = (int)(nb / (2 * sz));
            const long sw = 2 * sz * ldw + 2 * sz, sl = 2 * sz * ldl + 2 * sz;  // pair p: diagonal position 2·p·sz in W / iw / v, and in l
            g.cstride = sw;
            g.astride = sw;
            g.bstride = sl;
            RC(launch_gemm<double>(c, s, v, ldw, iw, ldw, l + sz * ldl, ldl, sz, sz, sz, g));                        // V = −AnT · L21ᵀ
            g.bstride = sw;
            RC(launch_gemm<double>(c, s, w + sz * ldw, ldw, w + sz * ldw + sz, ldw, v, ldw, sz, sz, sz, g));         // W21 = −Cn · Vᵀ
            RC(launch_gemm<double>(c, s, iw + sz, ldw, v, ldw, w + sz * ldw + sz, ldw, sz, sz, sz, g));              // WT12 = −V · Cnᵀ
        }
        return 0;
    }
    hipLaunchKernelGGL(identity_kernel<double>, dim3((unsigned)((nb + 255) / 256), (unsigned)nb), dim3(256), 0, s, iw, ldw, nb);
    HIPCHK(hipGetLastError());
    RC(trsm_upper_rec<double>(c, s, iw, ldw, l, ldl, 0, nb));
    hipLaunchKernelGGL(transpose_scale_kernel<double>, dim3((unsigned)((nb + 31) / 32), (unsigned)((nb + 31) / 32)), dim3(256), 0, s, (const double*)iw, ldw, w, ldw,
                       nb, -1.0);
    HIPCHK(hipGetLastError());
    return 0;
}
// X (m × nb) ← X L⁻ᵀ as ONE triangular-k MFMA GEMM with w = −inv(L): S = −X wᵀ into the scratch sc ((m + 128) × lds), copied back over X
int32_t gpmi::eng_trsm_inv(gp_ctx* c, hipStream_t s, double* x, long ldx, long m, const double* w, long ldw, long nb, double* sc, long lds) {
    DibArgs<double> dib;
    dib.W = w; dib.ldw = ldw; dib.nbi = nb; dib.S = sc; dib.lds = lds;
    return dib_apply<double>(c, s, x, ldx, m, nb, dib);
}
int32_t gpmi::eng_gemm_nt(gp_ctx* c, hipStream_t s, double* cm, long ldc, const double* a, long lda, const double* b, long ldb,
                          long m, long n, long k, GridMap g) {
    return launch_gemm<double>(c, s, cm, ldc, a, lda, b, ldb, m, n, k, g);
}
int32_t gpmi::eng_trsv(gp_ctx* c, hipStream_t s, const double* l, long ldl, long np, double* r, long ldr, int nrhs, bool forward) {
    return trsv<double>(c, s, l, ldl, np, r, ldr, nrhs, forward);
}
int32_t gpmi::eng_gemv_t(gp_ctx* c, hipStream_t s, const double* l, long ldl, long nrows, long ncols, const double* a, double* r) {
    (void)c;
    if (nrows <= 0 || ncols <= 0) return 0;
    hipLaunchKernelGGL(gemv_t_kernel<double>, dim3((unsigned)((ncols + 255) / 256), (unsigned)((nrows + 63) / 64)), dim3(256), 0, s, l,
                       ldl, nrows, ncols, a, r);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_rowsumsq(gp_ctx* c, hipStream_t s, const double* x, long ldx, long nrows, long ncols, double* out_dev) {
    (void)c;
    if (nrows <= 0) return 0;
    hipLaunchKernelGGL(rowsumsq_kernel<double>, dim3((unsigned)nrows), dim3(256), 0, s, x, ldx, ncols, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_copy2d(gp_ctx* c, hipStream_t s, double* dst, long dld, const double* src, long sld, long rows, long cols) {
    (void)c;
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(copy2d_kernel, dim3((unsigned)std::min<long>(rows, 1024)), dim3(256), 0, s, dst, dld, src, sld, rows, cols);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_kcross(gp_ctx* c, hipStream_t s, int kind, double variance, const double* xr, long ldxr, long nr_valid, long nr_pad,
                         const double* xc, long ldxc, long nc_valid, long nc_pad, int d, double* out, long ld) {
    (void)c;
    dim3 grid((unsigned)(nc_pad / 128), (unsigned)(nr_pad / 128));
    if (grid.x == 0 || grid.y == 0) return 0;
    launch_kmat<double>(grid, s, out, ld, xr, ldxr, xc, ldxc, d, kind, variance, (const double*)nullptr, nr_valid,
                       nc_valid, 0, plain_map(0, 0, 0), (const double*)nullptr, (const double*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_kvec(gp_ctx* c, hipStream_t s, const double* xs, long ldxs, const double* x, long ldx, int d, int kind, double variance,
                       long n, const double* alpha, double* out, long nrows) {
    (void)c;
    if (nrows <= 0) return 0;
    hipLaunchKernelGGL(kvec_kernel<double>, dim3((unsigned)nrows), dim3(256), 0, s, xs, ldxs, x, ldx, d, kind, variance, n, alpha, out);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t gpmi::eng_add_vec(gp_ctx* c, hipStream_t s, double* dst, const double* src, long n) {
    (void)c;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, n);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// host-side input marshalling
// ------------------------------------------------------------------------------------------------
template <typename T> static T pt_get(const gp_points* x, long i, int dd) {
    const T* p = (const T*)x->data;
    if (x->layout == 0) return p[i];
    if (x->layout == 1) return p[(long)dd + i * x->d];
    return p[i + (long)dd * x->n];
}
int32_t check_kernel(const gp_kernel* k, int d, int argi) {
    if (!k) return set_arg_err(argi, "kernel is NULL");
    if (k->kind < 0 || k->kind > 3) return set_arg_err(argi, "kernel kind must be 0..3");
    if (k->dtype != 0 && k->dtype != 1) return set_arg_err(argi, "dtype must be 0 (f64) or 1 (f32)");
    if (!(k->variance > 0)) return set_arg_err(argi, "variance must be > 0");
    if (k->nscale != 0 && k->nscale != 1 && k->nscale != d) return set_arg_err(argi, "nscale must be 0, 1 or D");
    if (k->nscale != 0 && !k->scale) return set_arg_err(argi, "scale is NULL");
    return 0;
}
int32_t check_points(const gp_points* x, int argi) {
    if (!x || !x->data) return set_arg_err(argi, "points NULL");
    if (x->n <= 0) return set_arg_err(argi, "n must be > 0");
    if (x->d <= 0) return set_arg_err(argi, "d must be > 0");
    if (x->layout < 0 || x->layout > 2) return set_arg_err(argi, "layout must be 0..2");
    if (x->layout == 0 && x->d != 1) return set_arg_err(argi, "layout 0 requires d == 1");
    return 0;
}
// scaled, dimension-major, zero-padded copy [d][ldx]
template <typename T>
static void scale_points_into(const gp_kernel* k, const gp_points* x, long ldx, T* out);
template <typename T>
static void scale_points(const gp_kernel* k, const gp_points* x, long ldx, std::vector<T>& out) {
    out.resize((size_t)x->d * ldx);
    scale_points_into<T>(k, x, ldx, out.data());
}
template <typename T>
static void scale_points_into(const gp_kernel* k, const gp_points* x, long ldx, T* out) {  // out: [d][ldx], every element written (padding zero)
    const int d = x->d;
    for (int dd = 0; dd < d; ++dd) {
        T s = T(1);
        if (k->nscale == 1) s = (T)k->scale[0];
        else if (k->nscale > 1) s = (T)k->scale[dd];
        T* o = out + (size_t)dd * ldx;
        const T* p = (const T*)x->data;
        const long n = x->n;
        std::fill(o + n, o + ldx, T(0));
        if (x->layout == 1) {  // point-contiguous: stride d
            for (long i = 0; i < n; ++i) o[i] = s * p[(long)dd + i * d];
        } else {               // a vector, or dimension-contiguous: unit stride
            const T* q = x->layout == 0 ? p : p + (long)dd * n;
            for (long i = 0; i < n; ++i) o[i] = s * q[i];
        }
    }
}
// The points of one call on the device: scale_points' copy [d][ldx] in a block of the caller's DevBufs, its upload queued on the main stream.  The object
// owns the host copy, so it has to outlive that upload (declare it where the call's synchronise is in scope).  TD = double with T = float is the sparse
// path's form: inputs arrive in T and are scaled in T, as the fit did, then widened.
template <typename T, typename TD = T> struct StagedPoints {
    std::vector<TD> h;
    void* dev = nullptr;
    const TD* ptr() const { return (const TD*)dev; }
    int32_t stage(gp_ctx* c, DevBufs& bufs, const gp_kernel* k, const gp_points* x, long ldx) {
        if constexpr (std::is_same<T, TD>::value) {
            scale_points<T>(k, x, ldx, h);
        } else {
            std::vector<T> hT;
            scale_points<T>(k, x, ldx, hT);
            h.assign(hT.begin(), hT.end());
        }
        RC(bufs.get(sizeof(TD) * h.size(), &dev));
        HIPCHK(hipMemcpyAsync(dev, h.data(), sizeof(TD) * h.size(), hipMemcpyHostToDevice, c->sm));
        return 0;
    }
};
// The input scales of a single kind as the gradient kernels read them: max(nscale, 1) doubles on the device, 1.0 where the kind has no scale (same lifetime rule)
struct DevScales {
    std::vector<double> h;
    void* dev = nullptr;
    const double* ptr() const { return (const double*)dev; }
    int32_t stage(DevBufs& bufs, int nscale, const double* scale, hipStream_t s) {
        h.assign((size_t)std::max(nscale, 1), 1.0);
        for (int p = 0; p < nscale; ++p) h[p] = scale[p];
        RC(bufs.get(sizeof(double) * h.size(), &dev));
        HIPCHK(hipMemcpyAsync(dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, s));
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------
// posterior handle
// ------------------------------------------------------------------------------------------------

// Every place that evaluates a kernel (KDesc, engine.hpp) goes through gram() / kvec(); with a single kind they launch what they always launched.
template <typename T>
static void gram(const KDesc& k, dim3 grid, hipStream_t s, T* out, long ld, const T* xr, long ldxr, const T* xc, long ldxc, int d, const T* noise,
                 long nr_valid, long nc_valid, int sym, GridMap g) {
    if (k.ks) launch_kmat_sum<T>(grid, s, out, ld, xr, ldxr, xc, ldxc, d, *k.ks, noise, nr_valid, nc_valid, sym, g);
    else launch_kmat<T>(grid, s, out, ld, xr, ldxr, xc, ldxc, d, k.kind, (T)k.variance, noise, nr_valid, nc_valid, sym, g, (const T*)nullptr, (const T*)nullptr);
}
template <typename T>
static void kvec(const KDesc& k, long ns, hipStream_t s, const T* xs, long ldxs, const T* x, long ldx, int d, long n, const T* alpha, T* out) {
    if (k.ks) launch_kvec_sum<T>(ns, s, xs, ldxs, x, ldx, d, *k.ks, n, alpha, out);
    else hipLaunchKernelGGL(kvec_kernel<T>, dim3((unsigned)ns), dim3(256), 0, s, xs, ldxs, x, ldx, d, k.kind, (T)k.variance, n, alpha, out);
}
// How many workgroups share the training range of a kmul launch (kernels.hpp): with few tiles of 64 test points the strips of 32 training points are dealt
// out until about 512 workgroups exist, never fewer than 4 strips (128 training points) per workgroup.  The rule reads n and ns only, so the order of
// summation — and with it every bit of a column's result — is the same whatever S is.  Smallest case that splits: n = 225 (8 strips) with ns <= 32 704 (511 tiles).
static inline void kmul_split(long n, long ns, long& nsplit, long& sps) {
    const long tiles = (ns + KMUL_TM - 1) / KMUL_TM, nstrips = (n + KMUL_KS - 1) / KMUL_KS;
    nsplit = std::min((512 + tiles - 1) / tiles, std::max(1L, nstrips / 4));
    sps = (nstrips + nsplit - 1) / nsplit;
    nsplit = (nstrips + sps - 1) / sps;
}
// out[c][·] = K(xs, x) alpha[c][·] for c < S columns (alpha: [S][lda], out: [S][ldo]; xs padded to a multiple of 128 points): one kmul launch (+ the ordered
// sum of the partial slices when the training range is split).  Single kind with D > 16: S kvec launches (kmul holds the inputs of a point in registers, 16
// dimensions at most; such inputs are rare and kvec has no limit), not counted in "cols_kernel_calls".
template <typename T>
static int32_t kmul(gp_ctx* c, DevBufs& bufs, const KDesc& k, long ns, hipStream_t s, const T* xs, long ldxs, const T* x, long ldx, int d, long n,
                    const T* alpha, long lda, int S, T* out, long ldo) {
    if (!k.ks && d > 16) {
        for (int col = 0; col < S; ++col) kvec<T>(k, ns, s, xs, ldxs, x, ldx, d, n, alpha + (long)col * lda, out + (long)col * ldo);
        HIPCHK(hipGetLastError());
        return 0;
    }
    long nsplit, sps;
    kmul_split(n, ns, nsplit, sps);
    const long slice = (long)S * ldo;
    T* part = out;
    if (nsplit > 1) {
        void* p_v = nullptr;
        RC(bufs.get(sizeof(T) * (size_t)nsplit * slice, &p_v));
        part = (T*)p_v;
    }
    launch_kmul<T>(dim3((unsigned)((ns + KMUL_TM - 1) / KMUL_TM), (unsigned)nsplit), s, xs, ldxs, ns, x, ldx, d, k, n, alpha, lda, S, sps, part, ldo, slice);
    HIPCHK(hipGetLastError());
    if (nsplit > 1) {
        hipLaunchKernelGGL(kmul_reduce_kernel<T>, dim3((unsigned)((ns + 255) / 256), (unsigned)S), dim3(256), 0, s, (const T*)part, slice, (int)nsplit, ns, ldo, out);
        HIPCHK(hipGetLastError());
    }
    c->cols_kernel_calls++;
    c->cols_kernel_splits = nsplit;
    return 0;
}

template <typename T> static int32_t assemble_sym(gp_ctx* c, const KDesc& k, const T* xs_dev, long ldx, int d,
                                                  const T* noise_dev, long n, long np, T* A, long ld) {
    GridMap g = plain_map(1, 0, 0);
    dim3 grid((unsigned)(np / 128), (unsigned)(np / 128));
    gram<T>(k, grid, c->sm, A, ld, xs_dev, ldx, xs_dev, ldx, d, noise_dev, n, n, 1, g);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Dense Σy (gp_noise kind 2 / 3, include/gpmi355.h): the named triangle of the caller's n×n column-major host array is streamed onto the n×n block at A
// (row-major, lower tiles) in pieces of at most "dense_stage_mb" MiB: host array -> page-locked half (host threads) -> device half (panel stream) -> add
// kernel (main stream).  Two halves of each, so the three stages of neighbouring pieces overlap; no second N×N buffer exists anywhere.  kind 2: a piece is a
// block of device rows (= host columns, rows 0..i), kind 3 a block of device columns (= host columns, rows j..n−1).  Returns with the last adds queued on
// the main stream; every byte of the host array has been read by then.  TA: matrix type, TS: type of the host array.
// ------------------------------------------------------------------------------------------------
static inline bool noise_dense(const gp_noise* nz) { return nz && (nz->kind == 2 || nz->kind == 3); }
// the diagonal of kinds 0 / 1 as the Gram kernels take it; a dense Σy is added afterwards (dense_add), its vector is zero
template <typename TC, typename TIO> static inline TC noise_entry(const gp_noise* nz, long i) {
    return nz->kind == 0 ? (TC)nz->s : (nz->kind == 1 ? (TC)((const TIO*)nz->diag)[i] : TC(0));
}
static int dense_host_threads() {  // host threads that fill one page-locked piece (environment GPMI_DENSE_THREADS, 1..16; measured: profiles/r8/dense_threads_ab.json)
    static const int nt = []() {
        const char* e = getenv("GPMI_DENSE_THREADS");
        const int v = e ? atoi(e) : 4;
        return v < 1 ? 1 : (v > 16 ? 16 : v);
    }();
    return nt;
}
template <typename F> static void dense_host_runs(long cnt, size_t bytes, F&& f) {  // f(lo, hi) over the runs [0, cnt) of one piece
    const int nt = (bytes >= ((size_t)8 << 20) && cnt >= 16) ? dense_host_threads() : 1;
    if (nt == 1) {
        f(0L, cnt);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([&, t]() { f(cnt * t / nt, cnt * (t + 1) / nt); });
    f(0L, cnt / nt);
    for (auto& x : th) x.join();
}
static long dense_piece(gp_ctx* c, long n, size_t elt) {  // rows / columns per piece: a multiple of 128 within the staging budget, at least 128
    const long budget = (long)(((size_t)c->dense_stage_mb << 20) / elt);
    return std::max(128L, budget / round_up(n, 4) / 128 * 128);
}
template <typename TA, typename TS>
static int32_t dense_add(gp_ctx* c, DevBufs& bufs, TA* A, long ld, const gp_noise* nz, long n) {
    const TS* H = (const TS*)nz->diag;
    const bool by_rows = nz->kind == 2;
    const long pr = dense_piece(c, n, sizeof(TS));
    const size_t buf_b = (size_t)round_up((long)sizeof(TS) * std::min(pr, n) * round_up(n, 4), 256);
    void* dev_v = nullptr;
    RC(bufs.get(2 * buf_b, &dev_v));
    char* pin = (char*)ctx_pinned(c, 2 * buf_b);
    if (!pin) return set_err_text(-1000 - (int)hipErrorOutOfMemory, "dense noise: no page-locked staging (lower \"dense_stage_mb\")");
    hipEvent_t copied[2], added[2];
    for (int b = 0; b < 2; ++b) {
        RC(ctx_event(c, &copied[b], false));
        RC(ctx_event(c, &added[b], false));
    }
    constexpr int E = 16 / sizeof(TS);
    long p = 0;
    for (long p0 = 0; p0 < n; p0 += pr, ++p) {
        const int b = (int)(p & 1);
        const long cnt = std::min(pr, n - p0);
        TS* hp = (TS*)(pin + b * buf_b);
        TS* dp = (TS*)((char*)dev_v + b * buf_b);
        const long w = by_rows ? round_up(p0 + cnt, 4) : round_up(n - p0, 4);
        if (p >= 2) HIPCHK(hipEventSynchronize(copied[b]));  // the upload out of this page-locked half is done
        if (by_rows)
            dense_host_runs(cnt, sizeof(TS) * (size_t)cnt * w, [&](long lo, long hi) {
                for (long r = lo; r < hi; ++r) memcpy(hp + r * w, H + (size_t)(p0 + r) * n, sizeof(TS) * (size_t)(p0 + r + 1));
            });
        else
            dense_host_runs(cnt, sizeof(TS) * (size_t)cnt * w, [&](long lo, long hi) {
                for (long r = lo; r < hi; ++r) memcpy(hp + r * w + r, H + (size_t)(p0 + r) * n + (p0 + r), sizeof(TS) * (size_t)(n - p0 - r));
            });
        if (p >= 2) HIPCHK(hipStreamWaitEvent(c->sp, added[b], 0));  // the add that read this device half is done
        HIPCHK(hipMemcpyAsync(dp, hp, sizeof(TS) * (size_t)cnt * w, hipMemcpyHostToDevice, c->sp));
        HIPCHK(hipEventRecord(copied[b], c->sp));
        HIPCHK(hipStreamWaitEvent(c->sm, copied[b], 0));
        if (by_rows) {
            const long ncol = std::min(n, round_up(p0 + cnt, 128));
            hipLaunchKernelGGL((dense_add_rows_kernel<TA, TS>), dim3((unsigned)((ncol + 256 * E - 1) / (256 * E)), (unsigned)std::min(cnt, 65535L)), dim3(256), 0,
                               c->sm, A, ld, (const TS*)dp, w, p0, cnt, n);
        } else {
            hipLaunchKernelGGL((dense_add_cols_kernel<TA, TS>), dim3((unsigned)((cnt + 63) / 64), (unsigned)((n - p0 + 63) / 64)), dim3(256), 0, c->sm, A, ld,
                               (const TS*)dp, w, p0, n);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(added[b], c->sm));
    }
    return 0;
}
// G = ½(α αᵀ − C⁻¹) (n×n, symmetric: column-major == row-major) to the caller's host array in row blocks: kernel -> device half -> page-locked half on the
// stream, the copy into the pageable array on the host while the next block is on its way.  Cinv: −C⁻¹, lower, row-major.
template <typename T>
static int32_t dense_grad_out(gp_ctx* c, hipStream_t s, DevBufs& bufs, const T* Cinv, long ld, const T* alpha, long n, T* out) {
    const long budget = (long)(((size_t)c->dense_stage_mb << 20) / sizeof(T));
    const long pr = std::max(64L, budget / n / 64 * 64);
    const size_t buf_b = (size_t)round_up((long)sizeof(T) * std::min(pr, round_up(n, 64)) * n, 256);
    void* dev_v = nullptr;
    RC(bufs.get(2 * buf_b, &dev_v));
    char* pin = (char*)ctx_pinned(c, 2 * buf_b);
    if (!pin) return set_err_text(-1000 - (int)hipErrorOutOfMemory, "dense noise gradient: no page-locked staging (lower \"dense_stage_mb\")");
    hipEvent_t done[2];
    for (int b = 0; b < 2; ++b) RC(ctx_event(c, &done[b], false));
    const long np_ = (n + pr - 1) / pr;
    auto drain = [&](long q) -> int32_t {  // piece q: wait for its download, copy it to the caller
        const int b = (int)(q & 1);
        HIPCHK(hipEventSynchronize(done[b]));
        const long r0 = q * pr, cnt = std::min(pr, n - r0);
        memcpy(out + (size_t)r0 * n, pin + b * buf_b, sizeof(T) * (size_t)cnt * n);
        return 0;
    };
    for (long q = 0; q < np_; ++q) {
        const int b = (int)(q & 1);
        if (q >= 2) RC(drain(q - 2));
        const long r0 = q * pr, cnt = std::min(pr, n - r0);
        T* dp = (T*)((char*)dev_v + b * buf_b);
        hipLaunchKernelGGL(dense_grad_rows_kernel<T>, dim3((unsigned)((n + 63) / 64), (unsigned)((cnt + 63) / 64)), dim3(256), 0, s, Cinv, ld, alpha, n, r0, cnt, dp);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pin + b * buf_b, dp, sizeof(T) * (size_t)cnt * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(done[b], s));
    }
    for (long q = std::max(0L, np_ - 2); q < np_; ++q) RC(drain(q));
    return 0;
}

struct FitOut {
    std::vector<double> logpdf;  // per RHS column
    double logdet = 0;           // logdet(K + Σy)            (src/finite_gp_projection.jl:310)
    std::vector<double> sqmahal; // ‖U⁻ᵀ(y_s − m)‖² per column (src/finite_gp_projection.jl:325-326)
    int32_t info = 0;
};

// gp_timings of a finished call (the stream has been synchronised): the phases between the four ev_phase records ...
static int32_t phase_timings(gp_ctx* c) {
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_phase[0], c->ev_phase[1]));
    c->tm.assemble_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_phase[1], c->ev_phase[2]));
    c->tm.potrf_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_phase[2], c->ev_phase[3]));
    c->tm.solve_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_phase[0], c->ev_phase[3]));
    c->tm.total_ms = ms;
    return 0;
}
// ... and, for a fit (exact or sparse), the event-bracketed GEMM launches
static int32_t fit_timings(gp_ctx* c) {
    float ms;
    RC(phase_timings(c));
    c->tm.gemm_ms = 0;
    c->tm.gemm_flops = 0;
    c->tm.gemm_bytes = 0;
    c->tm.gemm_launches = (int64_t)c->gemm_recs.size();
    for (auto& r : c->gemm_recs) {
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        c->tm.gemm_ms += ms;
        c->tm.gemm_flops += r.flops;
        c->tm.gemm_bytes += r.bytes;
        if (getenv("GPMI_DUMP_GEMM")) {
            if (r.nprob) fprintf(stderr, "GEMM s%d grouped problems=%ld tiles=%ld Kmax=%ld ms=%.4f tflops=%.2f\n", r.stream, r.nprob, r.ntiles, r.K, ms, r.flops / ms / 1e9);
            else fprintf(stderr, "GEMM s%d M=%ld N=%ld K=%ld ms=%.4f tflops=%.2f\n", r.stream, r.M, r.N, r.K, ms, r.flops / ms / 1e9);
        }
    }
    return 0;
}

// Shared by gp_logpdf and gp_posterior_fit.  Y: n×ncols column-major host.  If post != NULL the factor
// is kept and α is computed for every column (post->alpha: [ncols][np]; alpha_out: n×ncols column-major, leading dimension n).  ks != NULL: a composite kernel (the *_sum calls) — k then scales nothing (nscale 0) and
// carries Σ_t σ_t² as its variance, the prior variance the predictions use.
template <typename T>
static int32_t fit_impl(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise,
                        const void* mean_or_null, const void* Yv, long ldy, int ncols, FitOut& out, gp_post* post,
                        void* alpha_out, const KSum* ks = nullptr) {
    const long n = x->n, np = round_up(n, 128);
    const int d = x->d;
    const long R = round_up(std::max(ncols, 1), 128);
    const long mtot = np + R;
    const long ld = np + c->ldpad;
    const T* Y = (const T*)Yv;
    const T* mean = (const T*)mean_or_null;

    c->ev_used = 0;
    c->gemm_recs.clear();
    for (auto& e : c->ev_phase)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 8 + R));

    // ---- host marshalling
    std::vector<T> xs_h;
    scale_points<T>(k, x, np, xs_h);
    std::vector<T> noise_h((size_t)np, T(0));
    for (long i = 0; i < n; ++i) noise_h[i] = noise_entry<T, T>(noise, i);
    std::vector<T> rhs_h((size_t)ncols * np, T(0));  // rows: δ_sᵀ = (Y[:,s] - m)ᵀ, zero padded
    for (int s = 0; s < ncols; ++s)
        for (long i = 0; i < n; ++i) rhs_h[(size_t)s * np + i] = Y[(size_t)s * ldy + i] - (mean ? mean[i] : T(0));

    // ---- device buffers (RAII: every exit path returns what is not handed to the posterior handle)
    void *A_v = nullptr, *xs_v = nullptr, *noise_v = nullptr, *alpha_v = nullptr;
    const size_t A_bytes = sizeof(T) * (size_t)(mtot + 128) * ld;
    const size_t xs_bytes = sizeof(T) * (size_t)d * np, nz_bytes = sizeof(T) * (size_t)np;
    DevBufs bufs(c);
    RC(bufs.get(A_bytes, &A_v));
    RC(bufs.get(xs_bytes, &xs_v));
    RC(bufs.get(nz_bytes, &noise_v));
    const size_t alpha_bytes = post ? nz_bytes * (size_t)ncols : nz_bytes;
    RC(bufs.get(alpha_bytes, &alpha_v));
    T* A = (T*)A_v;
    double logdet_half_out = 0;
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        HIPCHK(hipEventRecord(c->ev_phase[0], c->sm));
        HIPCHK(hipMemcpyAsync(xs_v, xs_h.data(), xs_bytes, hipMemcpyHostToDevice, c->sm));
        HIPCHK(hipMemcpyAsync(noise_v, noise_h.data(), nz_bytes, hipMemcpyHostToDevice, c->sm));
        HIPCHK(hipMemsetAsync(c->info_dev, 0, sizeof(int), c->sm));
        HIPCHK(hipMemsetAsync(c->scal_dev, 0, sizeof(double) * (8 + R), c->sm));
        // RHS rows (+ the 128 slack rows) zeroed, then δ rows copied in
        HIPCHK(hipMemsetAsync(A + np * ld, 0, sizeof(T) * (size_t)(R + 128) * ld, c->sm));
        HIPCHK(hipMemcpy2DAsync(A + np * ld, sizeof(T) * ld, rhs_h.data(), sizeof(T) * np, sizeof(T) * np, ncols,
                                hipMemcpyHostToDevice, c->sm));
        RC(assemble_sym<T>(c, KDesc{k->kind, k->variance, ks}, (const T*)xs_v, np, d, (const T*)noise_v, n, np, A, ld));
        if (noise_dense(noise)) RC((dense_add<T, T>(c, bufs, A, ld, noise, n)));  // all of Σy before the factorisation (counts into assemble_ms)
        HIPCHK(hipEventRecord(c->ev_phase[1], c->sm));
        RC(potrf_full<T>(c, A, ld, np, mtot, c->info_dev, n, c->scal_dev, &bufs));
        HIPCHK(hipEventRecord(c->ev_phase[2], c->sm));
        // sqmahal per RHS row: ‖z_s‖², z_sᵀ = δ_sᵀ L⁻ᵀ sits in row np+s
        hipLaunchKernelGGL(rowsumsq_kernel<T>, dim3((unsigned)ncols), dim3(256), 0, c->sm, A + np * ld, ld, np,
                           c->scal_dev + 8);
        HIPCHK(hipGetLastError());
        if (post && ncols == 1) {  // α = L⁻ᵀ z
            HIPCHK(hipMemcpyAsync(alpha_v, A + np * ld, sizeof(T) * np, hipMemcpyDeviceToDevice, c->sm));
            RC(trsv<T>(c, c->sm, A, ld, np, (T*)alpha_v, np, 1, false));
        } else if (post) {  // gp_posterior_fit_cols: every row z_sᵀ, one backward sweep for all of them (as solve_impl)
            HIPCHK(hipMemcpy2DAsync(alpha_v, sizeof(T) * np, A + np * ld, sizeof(T) * ld, sizeof(T) * np, ncols, hipMemcpyDeviceToDevice, c->sm));
            RC(trsv<T>(c, c->sm, A, ld, np, (T*)alpha_v, np, ncols, false));
        }
        HIPCHK(hipEventRecord(c->ev_phase[3], c->sm));
        int info_h = 0;
        std::vector<double> scal_h(8 + ncols);
        HIPCHK(hipMemcpyAsync(&info_h, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipMemcpyAsync(scal_h.data(), c->scal_dev, sizeof(double) * (8 + ncols), hipMemcpyDeviceToHost, c->sm));
        if (post && alpha_out && ncols == 1)
            HIPCHK(hipMemcpyAsync(alpha_out, alpha_v, sizeof(T) * n, hipMemcpyDeviceToHost, c->sm));
        else if (post && alpha_out)
            HIPCHK(hipMemcpy2DAsync(alpha_out, sizeof(T) * n, alpha_v, sizeof(T) * np, sizeof(T) * n, ncols, hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        out.info = info_h;
        out.logpdf.resize(ncols);
        out.sqmahal.resize(ncols);
        logdet_half_out = scal_h[0];
        const double logdet = 2.0 * scal_h[0];
        out.logdet = logdet;
        for (int s = 0; s < ncols; ++s) {
            out.sqmahal[s] = scal_h[8 + s];
            out.logpdf[s] = -0.5 * ((double)n * LOG2PI + logdet + scal_h[8 + s]);
        }
        return fit_timings(c);
    });
    if (rc != 0) return rc;
    if (out.info != 0 || !post) return out.info;
    bufs.keep(A_v);
    bufs.keep(xs_v);
    bufs.keep(alpha_v);
    post->dtype = k->dtype;
    post->n = n; post->np = np; post->ld = ld; post->mtot = mtot; post->d = d;
    post->kern = KernelRec(k, ks);
    post->A = A_v; post->A_bytes = A_bytes;
    post->xs = xs_v; post->xs_bytes = xs_bytes;
    post->alpha = alpha_v; post->alpha_bytes = alpha_bytes;
    post->ncols = ncols;
    post->logdet_half = logdet_half_out;
    return 0;
}

// ---- what the predictive calls on a resident exact posterior share (test points xs_dev: StagedPoints, [d][nsp]; work queued on s, no synchronise unless said) ----
// K_*x α into m_dev (nsp entries) and its download into m_h
template <typename T>
static int32_t post_mean(gp_post* post, hipStream_t s, const T* xs_dev, long ns, long nsp, T* m_dev, std::vector<T>& m_h) {
    kvec<T>(post->kern.desc(), ns, s, xs_dev, nsp, (const T*)post->xs, post->np, post->d, post->n, (const T*)post->alpha, m_dev);
    HIPCHK(hipGetLastError());
    m_h.resize((size_t)ns);
    HIPCHK(hipMemcpyAsync(m_h.data(), m_dev, sizeof(T) * (size_t)ns, hipMemcpyDeviceToHost, s));
    return 0;
}
// (after the synchronise) out = m(x*) + K_*x α, the sum taken in TO
template <typename T, typename TO> static void add_prior_mean(const T* prior_mean, const std::vector<T>& m_h, TO* out) {
    for (size_t i = 0; i < m_h.size(); ++i) out[i] = (TO)(prior_mean ? prior_mean[i] : T(0)) + (TO)m_h[i];
}
// X (rows × np, leading dimension ldx) = K(x*[r0 .. r0 + rows), x) L⁻ᵀ: the Gram block of one chunk of test points, then the forward solve with the resident factor
template <typename T>
static int32_t cross_solve(gp_post* post, hipStream_t s, DevBufs& bufs, const T* xs_dev, long ns, long nsp, long r0, long rows, T* X, long ldx) {
    GridMap g = plain_map(0, r0, 0);
    dim3 grid((unsigned)(post->np / 128), (unsigned)(rows / 128));
    gram<T>(post->kern.desc(), grid, s, X, ldx, xs_dev, nsp, (const T*)post->xs, post->np, post->d, (const T*)nullptr, ns, post->n, 0, g);
    HIPCHK(hipGetLastError());
    return trsm_post<T>(post, s, X, ldx, rows, bufs);
}
// vo[i] = k(x, x) − ‖X_i‖² for the first `valid` of the rows of a solved chunk: rowsumsq, its download, ONE synchronise (ss: host scratch of at least `rows`)
template <typename T>
static int32_t chunk_variance(gp_post* post, hipStream_t s, const T* X, long ldx, long rows, long valid, std::vector<double>& ss, T* vo) {
    gp_ctx* c = post->ctx;
    hipLaunchKernelGGL(rowsumsq_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, X, ldx, post->np, c->scal_dev + 8);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ss.data(), c->scal_dev + 8, sizeof(double) * rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (long i = 0; i < valid; ++i) vo[i] = (T)(post->kern.variance - ss[i]);  // k(x, x) = σ² (composite: Σ_t σ_t², every κ_f(x, x) = 1)
    return 0;
}

// cols: gp_posterior_predict_cols — the mean of every column of the handle (mean_out: ns×ncols column-major) by ONE kmul launch instead of kvec
template <typename T>
static int32_t predict_impl(gp_post* post, const gp_points* xs, const void* pm, int what, void* mean_out,
                            void* var_out, void* cov_out, bool cols) {
    gp_ctx* c = post->ctx;
    SkScope sk(c);
    const long n = post->n, np = post->np;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = post->d;
    const gp_kernel k = post->kern.view(post->dtype);
    StagedPoints<T> sx;
    DevBufs bufs(c);
    void *m_v = nullptr, *X_v = nullptr, *C_v = nullptr;
    const size_t m_bytes = sizeof(T) * (size_t)nsp;
    const T* prior_mean = (const T*)pm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    return run_drained(c, [&]() -> int32_t {
        RC(sx.stage(c, bufs, &k, xs, nsp));
        if ((what & 1) && cols) {
            const int S = post->ncols;
            RC(bufs.get(m_bytes * (size_t)S, &m_v));
            RC(kmul<T>(c, bufs, post->kern.desc(), ns, c->sm, sx.ptr(), nsp, (const T*)post->xs, np, d, n, (const T*)post->alpha, np, S, (T*)m_v, nsp));
            T* mo = (T*)mean_out;
            HIPCHK(hipMemcpy2DAsync(mo, sizeof(T) * ns, m_v, sizeof(T) * nsp, sizeof(T) * ns, S, hipMemcpyDeviceToHost, c->sm));
            HIPCHK(hipStreamSynchronize(c->sm));
            if (prior_mean)
                for (int col = 0; col < S; ++col)
                    for (long i = 0; i < ns; ++i) mo[(size_t)col * ns + i] += prior_mean[i];
        } else if (what & 1) {
            RC(bufs.get(m_bytes, &m_v));
            std::vector<T> m_h;
            RC(post_mean<T>(post, c->sm, sx.ptr(), ns, nsp, (T*)m_v, m_h));
            HIPCHK(hipStreamSynchronize(c->sm));
            add_prior_mean<T, T>(prior_mean, m_h, (T*)mean_out);
        }
        if (what & 6) {
            const bool want_cov = (what & 4) != 0;
            // test points are processed in row chunks of the cross-covariance X = K_*x (chunk × np);
            // the full covariance needs all of X at once.
            const long chunk = want_cov ? nsp : std::min<long>(nsp, 4096);
            const long ldx = np + c->ldpad;
            RC(bufs.get(sizeof(T) * (size_t)(chunk + 128) * ldx, &X_v));
            RC(ctx_scal(c, 8 + chunk));
            T* X = (T*)X_v;
            std::vector<double> ss(chunk);
            for (long r0 = 0; r0 < nsp; r0 += chunk) {
                const long rows = std::min(chunk, nsp - r0);
                RC(cross_solve<T>(post, c->sm, bufs, sx.ptr(), ns, nsp, r0, rows, X, ldx));
                if (what & 2) RC(chunk_variance<T>(post, c->sm, X, ldx, rows, std::min(rows, ns - r0), ss, (T*)var_out + r0));
            }
            if (want_cov) {
                const long ldc = nsp + c->ldpad;
                RC(bufs.get(sizeof(T) * (size_t)(nsp + 128) * ldc, &C_v));
                T* Cm = (T*)C_v;
                GridMap g = plain_map(0, 0, 0);
                dim3 grid((unsigned)(nsp / 128), (unsigned)(nsp / 128));
                gram<T>(post->kern.desc(), grid, c->sm, Cm, ldc, sx.ptr(), nsp, sx.ptr(), nsp, d, (const T*)nullptr, ns, ns, 0, g);
                HIPCHK(hipGetLastError());
                RC(launch_gemm<T>(c, c->sm, Cm, ldc, X, ldx, X, ldx, nsp, nsp, np, plain_map(0, 0, 0)));
                // symmetric: row-major == column-major
                HIPCHK(hipMemcpy2DAsync(cov_out, sizeof(T) * ns, Cm, sizeof(T) * ldc, sizeof(T) * ns, ns,
                                        hipMemcpyDeviceToHost, c->sm));
                HIPCHK(hipStreamSynchronize(c->sm));
            }
        }
        return 0;
    });
}

// gm / gv for `cnt` test points from j0 on (kernels.hpp kpgrad_kernel / kpgrad_sum_kernel): a composite kernel in one launch (D <= 16), a single kind once per
// chunk of 16 dimensions.  sc: the kind's input scales on the device (double [max(nscale, 1)]).
template <typename T>
static int32_t launch_kpgrad(const KDesc& k, int nscale, const double* sc, long cnt, hipStream_t s, const T* xs, long ldxs, const T* x, long ldx, int d, long n,
                             const T* alpha, const T* W, long ldw, double* gm, double* gv, long ldg, long j0) {
    if (cnt <= 0) return 0;
    if (k.ks) {
        launch_kpgrad_sum<T>(cnt, s, xs, ldxs, x, ldx, d, *k.ks, n, alpha, W, ldw, gm, gv, ldg, j0);
        HIPCHK(hipGetLastError());
        return 0;
    }
    for (int p0 = 0; p0 < d; p0 += 16) {
        hipLaunchKernelGGL(kpgrad_kernel<T>, dim3((unsigned)cnt), dim3(256), 0, s, xs, ldxs, x, ldx, d, k.kind, (T)k.variance, nscale, sc, n, alpha, W, ldw, gm, gv,
                           ldg, j0, p0);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// Predictive mean / variance AND their gradients w.r.t. the test inputs (include/gpmi355.h gp_posterior_predict_grad), next to predict_impl and in its
// chunks.  Mean side: the α-weighted kernels only (no Gram matrix, no solve).  Variance side, per chunk of 4 096 test points: Gram → forward solve
// (trsm_post; the variance falls out of rowsumsq as in predict_impl) → backward solve in place (trsm_back_cached: the rows become C⁻¹k_j) → kpgrad.
// Measured against gp_posterior_predict(what = 3) on the same handle and 4 096 test points (profiles/r17/predict_grad_profile.json), BLOCKED path: 2.07 at
// N = 16 384, 2.06 at N = 65 536 (the design predicts a ratio near 2: a second solve of the same flops — GEMM event times 17.3 ms forward, 17.6 ms backward at
// N = 16 384; kpgrad 0.69 ms and the 15 transposes 0.44 ms).  Back-substitution path (no inverse blocks): N = 1 920, 1.3 -> 282 ms, a ratio of 212.
template <typename T>
static int32_t predict_grad_impl(gp_post* post, const gp_points* xs, const void* pm, int what, void* mean_out, void* var_out, void* dmean_out,
                                 void* dvar_out) {
    gp_ctx* c = post->ctx;
    SkScope sk(c);
    const long n = post->n, np = post->np;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = post->d;
    const gp_kernel k = post->kern.view(post->dtype);
    const KDesc kd = post->kern.desc();
    const bool want_gm = (what & 1) && dmean_out, want_gv = (what & 2) && dvar_out, side_v = (what & 2) != 0;
    StagedPoints<T> sx;
    DevScales sc;
    void *m_v = nullptr, *X_v = nullptr, *g_v = nullptr;
    const size_t g_bytes = sizeof(double) * (size_t)2 * d * nsp;
    DevBufs bufs(c);
    std::vector<double> g_h((want_gm || want_gv) ? (size_t)2 * d * nsp : 0);
    c->ev_used = 0;
    c->gemm_recs.clear();
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        RC(sx.stage(c, bufs, &k, xs, nsp));
        RC(bufs.get(g_bytes, &g_v));
        RC(sc.stage(bufs, k.nscale, k.scale, c->sm));
        double* gm = want_gm ? (double*)g_v : nullptr;
        double* gv = want_gv ? (double*)g_v + (size_t)d * nsp : nullptr;
        if ((what & 1) && mean_out) {
            RC(bufs.get(sizeof(T) * (size_t)nsp, &m_v));
            std::vector<T> m_h;
            RC(post_mean<T>(post, c->sm, sx.ptr(), ns, nsp, (T*)m_v, m_h));
            HIPCHK(hipStreamSynchronize(c->sm));
            add_prior_mean<T, T>((const T*)pm, m_h, (T*)mean_out);
        }
        if (want_gm && !want_gv)  // the mean side alone: one launch over every test point
            RC(launch_kpgrad<T>(kd, k.nscale, sc.ptr(), ns, c->sm, sx.ptr(), nsp, (const T*)post->xs, np, d, n, (const T*)post->alpha,
                                (const T*)nullptr, 0, gm, (double*)nullptr, nsp, 0));
        if (side_v) {
            const long chunk = std::min<long>(nsp, 4096);
            const long ldx = np + c->ldpad;
            RC(bufs.get(sizeof(T) * (size_t)(chunk + 128) * ldx, &X_v));
            RC(ctx_scal(c, 8 + chunk));
            T* X = (T*)X_v;
            // the 128 slack rows below a chunk are operand over-read of the solves' GEMMs: finite, whatever the recycled block held
            HIPCHK(hipMemsetAsync(X + (size_t)chunk * ldx, 0, sizeof(T) * (size_t)128 * ldx, c->sm));
            std::vector<double> ss(chunk);
            T* vo = (T*)var_out;
            BackWs ws;
            for (long r0 = 0; r0 < nsp; r0 += chunk) {
                const long rows = std::min(chunk, nsp - r0), valid = std::min(rows, ns - r0);
                RC(cross_solve<T>(post, c->sm, bufs, sx.ptr(), ns, nsp, r0, rows, X, ldx));
                if (vo) RC(chunk_variance<T>(post, c->sm, X, ldx, rows, valid, ss, vo + r0));
                if (want_gv) {
                    RC(trsm_back_cached<T>(c, c->sm, X, ldx, rows, valid, (const T*)post->A, post->ld, np, post->dibc, bufs, ws));
                    RC(launch_kpgrad<T>(kd, k.nscale, sc.ptr(), valid, c->sm, sx.ptr(), nsp, (const T*)post->xs, np, d, n,
                                        (const T*)post->alpha, (const T*)X, ldx, gm, gv, nsp, r0));
                }
            }
        }
        if (want_gm || want_gv) {
            HIPCHK(hipMemcpyAsync(g_h.data(), g_v, g_bytes, hipMemcpyDeviceToHost, c->sm));
            HIPCHK(hipStreamSynchronize(c->sm));
        }
        return 0;
    });
    if (rc != 0) return rc;
    if (want_gm) grad_to_layout<T>(xs->layout, ns, d, g_h.data(), nsp, dmean_out);
    if (want_gv) grad_to_layout<T>(xs->layout, ns, d, g_h.data() + (size_t)d * nsp, nsp, dvar_out);
    return 0;
}

// W (np rows, leading dimension ld, written in full; the slack rows below are the caller's) = L⁻ᵀ (upper, row-major) of the lower factor L: I · L⁻ᵀ by
// the restricted-row recursion.  nbi > 0: with the inverse diagonal blocks of that width — dib_build (batched: one launch sequence for all blocks)
// writes L_bb⁻ᵀ onto W's diagonal and −L_bb⁻¹ into Wn; a leaf of the recursion is then ONE triangular-k GEMM over the rows above its block.  (With the
// blocks built one after the other this did not pay — C2 93.0 -> 95.6 ms, C4 4.71 -> 4.72 s: the serial chains cost what the leaves they replaced cost.)
template <typename T>
static int32_t upper_inverse(gp_ctx* c, hipStream_t s, DevBufs& bufs, const T* L, long ld, long np, long nbi, T* W) {
    hipLaunchKernelGGL(identity_kernel<T>, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, s, W, ld, np);
    HIPCHK(hipGetLastError());
    if (nbi <= 0) return trsm_upper_rec<T>(c, s, W, ld, L, ld, 0, np);  // W = I L⁻ᵀ down to the 64-wide leaves
    const long ldw = nbi + c->ldpad;
    const size_t wb = sizeof(T) * (size_t)(np + 128) * ldw;
    void *Wn_v = 0, *Iw_v = 0, *S_v = 0;
    RC(bufs.get(wb, &Wn_v));
    RC(bufs.get(wb, &Iw_v));
    RC(bufs.get(wb, &S_v));
    RC(dib_build<T>(c, s, L, ld, np, nbi, (T*)Wn_v, ldw, (T*)Iw_v, W, ld));
    DibArgs<T> dib;
    dib.W = (const T*)Wn_v; dib.ldw = ldw; dib.nbi = nbi; dib.S = (T*)S_v; dib.lds = ldw;
    return trsm_upper_rec<T>(c, s, W, ld, L, ld, 0, np, dib);
}

// W = L⁻ᵀ (upper, row-major, np rows + 128 zeroed slack rows the GEMMs over-read) from the factor a fit left in post.A: what gp_logpdf_grad and the
// leave-one-out calls both start from.  W is written in full by identity_kernel (until round 5 the block was zeroed first: 34 GB of writes at C4).
template <typename T>
static int32_t factor_inv_t(gp_ctx* c, hipStream_t s, DevBufs& bufs, const gp_post& post, T* W) {
    const long np = post.np, ld = post.ld;
    HIPCHK(hipMemsetAsync(W + np * ld, 0, sizeof(T) * (size_t)128 * ld, s));
    return upper_inverse<T>(c, s, bufs, (const T*)post.A, ld, np, (c->dib_nb >= 128 && np >= 2 * c->dib_nb) ? round_up(c->dib_nb, 128) : 0, W);
}

// The leave-one-out outputs of gp_loo / gp_loo_grad (host arrays of n entries in the kernel's dtype; any may be NULL)
struct LooOut {
    void *lp = nullptr, *mean = nullptr, *var = nullptr;
};
// Device side of the leave-one-out terms: c_i = [C⁻¹]_ii from W = L⁻ᵀ, then μ, v, ℓ into terms ([3][np]) and Σ ℓ_i into sum; with b / dsc also the
// vectors b_i = α_i/c_i and d_i = √(1/c_i + α_i²/c_i²) the gradient's weights are built from (kernels.hpp).  y_h: the n observations on the host.
template <typename T>
static int32_t loo_terms(gp_ctx* c, hipStream_t s, DevBufs& bufs, const gp_post& post, const T* W, const T* y_h, T** terms, T* b, T* dsc, double** sum) {
    const long n = post.n, np = post.np;
    void *cd_v = 0, *y_v = 0, *t_v = 0, *sum_v = 0;
    RC(bufs.get(sizeof(double) * (size_t)np, &cd_v));
    RC(bufs.get(sizeof(T) * (size_t)np, &y_v));
    RC(bufs.get(sizeof(T) * (size_t)3 * np, &t_v));
    RC(bufs.get(sizeof(double), &sum_v));
    HIPCHK(hipMemcpyAsync(y_v, y_h, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(loo_diag_kernel<T>, dim3((unsigned)np), dim3(256), 0, s, W, post.ld, np, (double*)cd_v);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(loo_terms_kernel<T>, dim3(1), dim3(256), 0, s, (const double*)cd_v, (const T*)post.alpha, (const T*)y_v, n, np, (T*)t_v, b, dsc,
                       (double*)sum_v);
    HIPCHK(hipGetLastError());
    *terms = (T*)t_v;
    *sum = (double*)sum_v;
    return 0;
}
// (after the stream has been synchronised) the downloaded terms to the caller's arrays
template <typename T>
static void loo_put(const LooOut& o, const std::vector<T>& terms_h, long n, long np) {
    if (o.mean) memcpy(o.mean, terms_h.data(), sizeof(T) * (size_t)n);
    if (o.var) memcpy(o.var, terms_h.data() + np, sizeof(T) * (size_t)n);
    if (o.lp) memcpy(o.lp, terms_h.data() + 2 * np, sizeof(T) * (size_t)n);
}

// A posterior that lives for one call (gp_loo, gp_logpdf_grad and their kin: fit, use, forget): fit_impl into a stack gp_post whose blocks go back to the
// cache with the object, after the synchronise or drain every path ends in.  Declare it BEHIND the call's DevBufs: its blocks then return first, the order
// the cache has always seen them in (which block a later call gets, and with it every address, depends on that order).  After a failed fit the destructor
// releases nothing: fit_impl assigns post->A / xs / alpha on success alone and ctx_release ignores NULL.  (dibc.w is set only by a forward solve against the
// handle, which no caller does today; it is released for completeness.)
template <typename T> struct TempPost {
    gp_post post{};
    FitOut fo;
    explicit TempPost(gp_ctx* c) { post.ctx = c; }
    TempPost(const TempPost&) = delete;
    int32_t fit(const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, long ldy, int ncols, void* alpha_out,
                const KSum* ks) {
        return fit_impl<T>(post.ctx, k, x, noise, mean, Y, ldy, ncols, fo, &post, alpha_out, ks);
    }
    ~TempPost() {
        ctx_release(post.ctx, post.A, post.A_bytes);
        ctx_release(post.ctx, post.xs, post.xs_bytes);
        ctx_release(post.ctx, post.alpha, post.alpha_bytes);
        if (post.dibc.w) ctx_release(post.ctx, post.dibc.w, post.dibc.bytes);
    }
};

// gp_loo / gp_loo_sum: the value path — one fit, W = L⁻ᵀ, two bandwidth-bound kernels; no product with C⁻¹
template <typename T>
static int32_t loo_impl(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out,
                        const LooOut& out, const KSum* ks) {
    const long n = x->n;
    DevBufs bufs(c);
    TempPost<T> tp(c);
    RC(tp.fit(k, x, noise, mean, y, n, 1, nullptr, ks));
    const gp_post& post = tp.post;
    SkScope sk(c);
    const long np = post.np, ld = post.ld;
    hipStream_t s = c->sm;
    std::vector<T> terms_h((size_t)3 * np);
    double sum_h = 0;
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        void* W_v = 0;
        RC(bufs.get(sizeof(T) * (size_t)(np + 128) * ld, &W_v));
        RC(factor_inv_t<T>(c, s, bufs, post, (T*)W_v));
        T* terms = nullptr;
        double* sum = nullptr;
        RC(loo_terms<T>(c, s, bufs, post, (const T*)W_v, (const T*)y, &terms, (T*)nullptr, (T*)nullptr, &sum));
        HIPCHK(hipMemcpyAsync(terms_h.data(), terms, sizeof(T) * (size_t)3 * np, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&sum_h, sum, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc != 0) return rc;
    *(T*)value_out = (T)sum_h;
    loo_put<T>(out, terms_h, n, np);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Value + gradient of an objective of one exact fit (include/gpmi355.h gp_logpdf_grad, gp_logpdf_grad_cols, gp_loo_grad and their *_sum forms): every
// gradient is a contraction Σ_ij (a_i a_j + Ci_ij) ∂K_ij of a weight matrix Ci (lower, row-major) and a vector a with the kernel's derivatives.  The
// drivers at the end put the stages together: (a) W = L⁻ᵀ and Ci = −C⁻¹; (b) / (c) an objective that is not logpdf of one column folds its weights into
// Ci and (d) contracts with a = 0; (e) the contraction; (f) the results to the caller's arrays.  Everything is queued on s; (e) ends in the synchronise.
// ------------------------------------------------------------------------------------------------
template <typename T> struct GradOut {  // what (e) produces: on the device, then on the host
    void *g_v = nullptr, *dn_v = nullptr, *gx_v = nullptr;
    DevScales sc;
    std::vector<double> g_h;   // [0] ∂/∂variance, [1] Σ_i ∂/∂Σy_ii, [2 + p] ∂/∂scale_p (∂/∂θ_p of a composite kernel)
    std::vector<T> dn_h;       // ∂/∂Σy_ii
    std::vector<double> gx_h;  // ∂/∂x as [d][np]; empty: not wanted
};
// The blocks of a call — W and Ci ((np + 128) × ld each) and those of the results — with the sums zeroed and the kind's scales uploaded
template <typename T>
static int32_t grad_open(hipStream_t s, DevBufs& bufs, const gp_post& post, bool want_dx, T** W, T** Ci, GradOut<T>& go) {
    const long np = post.np;
    const KSum* ks = post.kern.desc().ks;
    go.g_h.assign((size_t)(2 + (ks ? ks->nth : std::max(post.kern.nscale(), 1))), 0.0);
    go.dn_h.resize((size_t)post.n);
    go.gx_h.resize(want_dx ? (size_t)post.d * np : 0);
    const size_t M_b = sizeof(T) * (size_t)(np + 128) * post.ld;
    void *W_v = nullptr, *Ci_v = nullptr;
    RC(bufs.get(M_b, &W_v));
    RC(bufs.get(M_b, &Ci_v));
    RC(bufs.get(sizeof(double) * go.g_h.size(), &go.g_v));
    RC(bufs.get(sizeof(T) * (size_t)np, &go.dn_v));
    HIPCHK(hipMemsetAsync(go.g_v, 0, sizeof(double) * go.g_h.size(), s));
    RC(go.sc.stage(bufs, post.kern.nscale(), post.kern.scale.data(), s));  // (the scales' block in front of gx's: the order the cache has always seen)
    if (want_dx) RC(bufs.get(sizeof(double) * go.gx_h.size(), &go.gx_v));
    *W = (T*)W_v;
    *Ci = (T*)Ci_v;
    return 0;
}
// (a) W = L⁻ᵀ, Ci = −W Wᵀ = −C⁻¹ (lower; no sign fold: the kernels of (e) add what the product left — kernels.hpp).  Ci is written in full by the product
// (beta0: C is overwritten, not read), as W is by factor_inv_t: only the 128 slack rows the GEMM over-reads need defined values
template <typename T>
static int32_t grad_inverse(gp_ctx* c, hipStream_t s, DevBufs& bufs, const gp_post& post, T* W, T* Ci) {
    const long np = post.np, ld = post.ld;
    HIPCHK(hipMemsetAsync(Ci + np * ld, 0, sizeof(T) * (size_t)128 * ld, s));
    RC(factor_inv_t<T>(c, s, bufs, post, W));
    GridMap gw = plain_map(1, 0, 0);
    gw.ktri = 2;   // W upper: k starts at the row tile
    gw.beta0 = 1;  // Ci is overwritten (its upper tiles are never read)
    return launch_gemm<T>(c, s, Ci, ld, W, ld, W, ld, np, np, np, gw);
}
// (d) the vector a of a folded objective: np zeros
template <typename T>
static int32_t zeroed_alpha(hipStream_t s, DevBufs& bufs, long np, const T** a0) {
    void* a0_v = nullptr;
    RC(bufs.get(sizeof(T) * (size_t)np, &a0_v));
    HIPCHK(hipMemsetAsync(a0_v, 0, sizeof(T) * (size_t)np, s));
    *a0 = (const T*)a0_v;
    return 0;
}
// (b) Σ_s logpdf(fx, y[:, s]) over the post.ncols columns of the fit: Ci ← ncols·Ci + Σ_s α_s α_sᵀ (kernels.hpp cols_weight_kernel)
template <typename T>
static int32_t fold_cols(hipStream_t s, DevBufs& bufs, const gp_post& post, T* Ci, const T** a0) {
    const long np = post.np;
    hipLaunchKernelGGL(cols_weight_kernel<T>, dim3((unsigned)(np / 128), (unsigned)(np / 128)), dim3(256), 0, s, Ci, post.ld, (const T*)post.alpha, np, post.ncols);
    HIPCHK(hipGetLastError());
    return zeroed_alpha<T>(s, bufs, np, a0);
}
// (c) the leave-one-out objective L = Σ_i log p(y_i | y_−i): Ci ← 2G = −Z Zᵀ + β αᵀ + α βᵀ (kernels.hpp, loo_*).  W is used up (Z takes its block).
// The value and β = −∂L/∂y are on their way to `out` when it returns.
template <typename T> struct LooFold {
    std::vector<T> beta_h;
    double sum_h = 0;
};
template <typename T>
static int32_t fold_loo(gp_ctx* c, hipStream_t s, DevBufs& bufs, const gp_post& post, const T* y_h, T* W, T* Ci, LooFold<T>& out, const T** a0) {
    const long n = post.n, np = post.np, ld = post.ld;
    const T* L = (const T*)post.A;
    out.beta_h.resize((size_t)n);
    void *b_v = 0, *d_v = 0;
    RC(bufs.get(sizeof(T) * (size_t)np, &b_v));
    RC(bufs.get(sizeof(T) * (size_t)np, &d_v));
    T* terms = nullptr;
    double* sum = nullptr;
    RC(loo_terms<T>(c, s, bufs, post, (const T*)W, y_h, &terms, (T*)b_v, (T*)d_v, &sum));                        // c_i from W, before Z takes its place
    HIPCHK(hipMemcpyAsync(&out.sum_h, sum, sizeof(double), hipMemcpyDeviceToHost, s));
    RC(trsv<T>(c, s, L, ld, np, (T*)b_v, np, 1, true));                                                          // β = C⁻¹ b = L⁻ᵀ (L⁻¹ b), in place
    RC(trsv<T>(c, s, L, ld, np, (T*)b_v, np, 1, false));
    HIPCHK(hipMemcpyAsync(out.beta_h.data(), b_v, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s));
    hipLaunchKernelGGL(loo_mirror_scale_kernel<T>, dim3((unsigned)(np / 64), (unsigned)(np / 64)), dim3(256), 0, s, (const T*)Ci, ld, (const T*)d_v, W, ld);  // Z = Ci diag(d), full
    HIPCHK(hipGetLastError());
    GridMap gz = plain_map(1, 0, 0);
    gz.beta0 = 1;
    RC(launch_gemm<T>(c, s, Ci, ld, W, ld, W, ld, np, np, np, gz));                                              // Ci = −Z Zᵀ (lower)
    hipLaunchKernelGGL(loo_fold_kernel<T>, dim3((unsigned)(np / 128), (unsigned)(np / 128)), dim3(256), 0, s, Ci, ld, (const T*)post.alpha, (const T*)b_v);  // += β αᵀ + α βᵀ
    HIPCHK(hipGetLastError());
    return zeroed_alpha<T>(s, bufs, np, a0);
}
// What the contraction's kernels take: the weights Ci (−C⁻¹, row-major lower) and a, the pre-scaled dimension-major inputs xs ([d][np]), the kernel (a single
// kind with its scales on the device, or a composite one: ks).  launch_kgrad / launch_kgradx pick the instances — grad_contract and the device-level entry
// point gpd_grad_contract (include/gpmi355.h) both go through them.
template <typename T> struct ContractArgs {
    const T* Ci;
    long ld;
    const T* xs;
    long n, np;
    int d, kind;
    double variance;
    int nscale;
    const double* sc;
    const KSum* ks;
    const T* a;
    dim3 grid() const { return dim3((unsigned)(np / 128), (unsigned)(np / 128)); }
};
template <typename T> static ContractArgs<T> contract_args(const gp_post& post, const T* Ci, const T* a, const double* sc) {
    return ContractArgs<T>{Ci, post.ld, (const T*)post.xs, post.n, post.np, post.d, post.kern.kind, post.kern.variance, post.kern.nscale(), sc, post.kern.desc().ks, a};
}
template <typename T, int ND>
static void launch_kgrad_fast(hipStream_t s, const ContractArgs<T>& A, double* g) {
    hipLaunchKernelGGL((kgrad_fast_kernel<T, ND>), A.grid(), dim3(256), 0, s, A.Ci, A.ld, A.xs, A.np, A.d, A.kind, (T)A.variance, A.nscale, A.sc, A.a, A.n, g);
}
// g[0] += ∂/∂variance, g[2 + p] += ∂/∂scale_p (∂/∂θ_p), then dn[i] = ∂/∂Σy_ii and g[1] += Σ_i dn[i]
template <typename T>
static int32_t launch_kgrad(hipStream_t s, const ContractArgs<T>& A, double* g, T* dn) {
    const long n = A.n, ld = A.ld;
    const int d = A.d, nscale = A.nscale;
    if (A.ks) {  // composite kernel: one launch per chunk of 16 θ entries
        for (int p0 = 0; p0 < A.ks->nth; p0 += 16) {
            launch_kgrad_sum<T>(A.grid(), s, A.Ci, ld, A.xs, A.np, d, *A.ks, A.a, n, g, p0);
            HIPCHK(hipGetLastError());
        }
    } else if (d <= 16 && (ld * (long)sizeof(T)) % 16 == 0) {  // the scratch-free form (16-byte loads of the weights): a single launch whatever the scales are
        if (d <= 4) launch_kgrad_fast<T, 4>(s, A, g);
        else if (d <= 8) launch_kgrad_fast<T, 8>(s, A, g);
        else launch_kgrad_fast<T, 16>(s, A, g);
        HIPCHK(hipGetLastError());
    } else {  // one launch per chunk of 16 ARD scales
        for (int p0 = 0; p0 < std::max(nscale, 1); p0 += 16) {
            hipLaunchKernelGGL(kgrad_kernel<T>, A.grid(), dim3(256), 0, s, A.Ci, ld, A.xs, A.np, d, A.kind, (T)A.variance, nscale, A.sc, A.a, n, g, p0);
            HIPCHK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(noise_grad_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A.Ci, ld, A.a, n, dn, g + 1);
    HIPCHK(hipGetLastError());
    return 0;
}
// gx[p][i] += ∂/∂x_ip: full-square pass (the mirrored Ci entry serves the tiles above the diagonal), 16 dimensions per launch
template <typename T>
static int32_t launch_kgradx(hipStream_t s, const ContractArgs<T>& A, double* gx, long ldg) {
    if (A.ks) {  // composite kernel: xs holds the raw inputs, D <= 16 (pack_ksum), one launch
        launch_kgradx_sum<T>(A.grid(), s, A.Ci, A.ld, A.xs, A.np, A.d, *A.ks, A.a, A.n, gx, ldg);
        HIPCHK(hipGetLastError());
    } else {
        for (int p0 = 0; p0 < A.d; p0 += 16) {
            hipLaunchKernelGGL(kgradx_kernel<T>, A.grid(), dim3(256), 0, s, A.Ci, A.ld, A.xs, A.np, A.d, A.kind, (T)A.variance, A.nscale, A.sc, A.a, A.n, gx, ldg, p0);
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}
// (e) the contraction: ∂/∂variance and ∂/∂scale (∂/∂θ), ∂/∂Σy (a dense one straight to the caller's n×n array dnoise_dense), ∂/∂x when go has room for
// it; then the downloads and the synchronise
template <typename T>
static int32_t grad_contract(gp_ctx* c, hipStream_t s, DevBufs& bufs, const gp_post& post, const T* Ci, const T* a, T* dnoise_dense, GradOut<T>& go) {
    const long n = post.n, np = post.np, ld = post.ld;
    const ContractArgs<T> A = contract_args<T>(post, Ci, a, go.sc.ptr());
    double* g = (double*)go.g_v;
    RC(launch_kgrad<T>(s, A, g, (T*)go.dn_v));
    if (dnoise_dense) RC(dense_grad_out<T>(c, s, bufs, Ci, ld, a, n, dnoise_dense));  // G = ½(a aᵀ + Ci), n×n
    if (go.gx_v) {
        double* gx = (double*)go.gx_v;
        HIPCHK(hipMemsetAsync(gx, 0, sizeof(double) * go.gx_h.size(), s));
        RC(launch_kgradx<T>(s, A, gx, np));
        HIPCHK(hipMemcpyAsync(go.gx_h.data(), gx, sizeof(double) * go.gx_h.size(), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(go.g_h.data(), g, sizeof(double) * go.g_h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(go.dn_h.data(), go.dn_v, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}
// (f) the results to the caller's arrays (any may be NULL).  dy_neg: what ∂/∂y is the negative of — α (n × ncols) or β; dnoise by the noise's kind
// (a dense one was written by (e)); dx in the container layout of x (src/finite_gp_projection.jl:32-37)
template <typename T>
static void grad_scatter(const gp_post& post, const gp_points* x, const gp_noise* noise, const GradOut<T>& go, const std::vector<T>& dy_neg, double* dvar,
                         double* dscale, double* dtheta, void* dnoise, void* dy, void* dx) {
    const double* g = go.g_h.data();
    const KSum* ks = post.kern.desc().ks;
    if (dvar) *dvar = g[0];
    if (dscale)
        for (int p = 0; p < post.kern.nscale(); ++p) dscale[p] = g[2 + p];
    if (dtheta && ks)
        for (int p = 0; p < ks->nth; ++p) dtheta[p] = g[2 + p];
    if (dnoise && noise->kind == 0) *(T*)dnoise = (T)g[1];
    else if (dnoise && noise->kind == 1) memcpy(dnoise, go.dn_h.data(), sizeof(T) * (size_t)post.n);
    if (dy)
        for (size_t i = 0; i < dy_neg.size(); ++i) ((T*)dy)[i] = -dy_neg[i];
    if (dx) grad_to_layout<T>(x->layout, post.n, post.d, go.gx_h.data(), post.np, dx);
}

// gp_logpdf_grad (ncols = 1, ldy = n) and gp_logpdf_grad_cols (ks != NULL: their _sum forms, ∂/∂θ into dtheta): Y is n×ncols with leading dimension ldy, the gradients are those of
// Σ_s logpdf(fx, Y[:, s]); logpdf_out: ncols entries, dY: n×ncols.  One column has nothing to fold: the contraction runs on −C⁻¹ with α itself.  (ldy goes to fit_impl as given, also for ncols = 1 where the driver before this one passed n: a single column is never stepped over, the reads are the same.)
template <typename T>
static int32_t grad_logpdf_cols(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, long ldy, int ncols,
                                void* logpdf_out, double* dvar, double* dscale, void* dnoise, void* dY, void* dx, const KSum* ks, double* dtheta) {
    DevBufs bufs(c);
    TempPost<T> tp(c);
    std::vector<T> alpha_h((size_t)x->n * ncols);
    RC(tp.fit(k, x, noise, mean, Y, ldy, ncols, alpha_h.data(), ks));
    const gp_post& post = tp.post;
    SkScope sk(c);
    GradOut<T> go;
    RC(run_drained(c, [&]() -> int32_t {
        T *W = nullptr, *Ci = nullptr;
        const T* a = (const T*)post.alpha;
        RC(grad_open<T>(c->sm, bufs, post, dx != nullptr, &W, &Ci, go));
        RC(grad_inverse<T>(c, c->sm, bufs, post, W, Ci));
        if (ncols > 1) RC(fold_cols<T>(c->sm, bufs, post, Ci, &a));
        return grad_contract<T>(c, c->sm, bufs, post, Ci, a, noise_dense(noise) ? (T*)dnoise : nullptr, go);
    }));
    for (int col = 0; col < ncols; ++col) ((T*)logpdf_out)[col] = (T)tp.fo.logpdf[col];
    grad_scatter<T>(post, x, noise, go, alpha_h, dvar, dscale, dtheta, dnoise, dY, dx);
    return 0;
}
// gp_loo_grad: value_out = L = Σ_i log p(y_i | y_−i), dy = −β
template <typename T>
static int32_t grad_loo(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out,
                        double* dvar, double* dscale, void* dnoise, void* dy, void* dx, const KSum* ks, double* dtheta) {
    DevBufs bufs(c);
    TempPost<T> tp(c);
    std::vector<T> alpha_h((size_t)x->n);  // (the fit hands α back as it does for gp_logpdf_grad; nothing here reads it)
    RC(tp.fit(k, x, noise, mean, y, x->n, 1, alpha_h.data(), ks));
    const gp_post& post = tp.post;
    SkScope sk(c);
    GradOut<T> go;
    LooFold<T> lf;
    RC(run_drained(c, [&]() -> int32_t {
        T *W = nullptr, *Ci = nullptr;
        const T* a = nullptr;
        RC(grad_open<T>(c->sm, bufs, post, dx != nullptr, &W, &Ci, go));
        RC(grad_inverse<T>(c, c->sm, bufs, post, W, Ci));
        RC(fold_loo<T>(c, c->sm, bufs, post, (const T*)y, W, Ci, lf, &a));
        return grad_contract<T>(c, c->sm, bufs, post, Ci, a, noise_dense(noise) ? (T*)dnoise : nullptr, go);
    }));
    *(T*)value_out = (T)lf.sum_h;
    grad_scatter<T>(post, x, noise, go, lf.beta_h, dvar, dscale, dtheta, dnoise, dy, dx);
    return 0;
}

// Sequential conditioning: bordered Cholesky on the device (reference src/exact_gpr_posterior.jl:46-56,
// src/util/common_covmat_ops.jl:38-42).
template <typename T>
static int32_t update_impl(gp_post* old, const gp_points* x2, const gp_noise* noise2, const void* delta_all, gp_post* post,
                           void* alpha_out, double* logpdf_out) {
    gp_ctx* c = old->ctx;
    const long n1 = old->n, np1 = old->np, ld1 = old->ld;
    const long n2 = x2->n, n2p = round_up(n2, 128);
    const long n = n1 + n2, np = round_up(n, 128), ld = np + c->ldpad, mtot = np + 128;
    const int d = old->d;
    const gp_kernel k = old->kern.view(old->dtype);
    SkScope sk(c);
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 16));

    StagedPoints<T> sx2;  // [d][n2p]
    std::vector<T> noise_h((size_t)n2p, T(0));
    for (long i = 0; i < n2; ++i) noise_h[i] = noise_entry<T, T>(noise2, i);
    std::vector<T> delta_h((size_t)np, T(0));
    memcpy(delta_h.data(), delta_all, sizeof(T) * (size_t)n);

    void *A_v = 0, *xs_v = 0, *alpha_v = 0, *X_v = 0, *S_v = 0, *nz_v = 0;
    const long ldx = np1 + c->ldpad, lds = n2p + c->ldpad;
    const size_t A_b = sizeof(T) * (size_t)(mtot + 128) * ld, xs_b = sizeof(T) * (size_t)d * np, v_b = sizeof(T) * (size_t)np;
    const size_t X_b = sizeof(T) * (size_t)(n2p + 128) * ldx, S_b = sizeof(T) * (size_t)(n2p + 128) * lds;
    const size_t nz_b = sizeof(T) * (size_t)n2p;
    DevBufs bufs(c);
    RC(bufs.get(A_b, &A_v));
    RC(bufs.get(xs_b, &xs_v));
    RC(bufs.get(v_b, &alpha_v));
    RC(bufs.get(X_b, &X_v));
    RC(bufs.get(S_b, &S_v));
    T* A = (T*)A_v;
    T* X = (T*)X_v;
    T* S = (T*)S_v;
    const T* A1 = (const T*)old->A;
    int info_h = 0;
    double scal_h[16] = {0};
    int32_t rc = run_drained(c, [&]() -> int32_t {
        RC(sx2.stage(c, bufs, &k, x2, n2p));
        RC(bufs.get(nz_b, &nz_v));
        HIPCHK(hipMemcpyAsync(nz_v, noise_h.data(), nz_b, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(c->info_dev, 0, sizeof(int), s));
        HIPCHK(hipMemsetAsync(c->scal_dev, 0, sizeof(double) * 16, s));
        // combined scaled inputs [d][np]: old block, then the new points
        HIPCHK(hipMemsetAsync(xs_v, 0, xs_b, s));
        HIPCHK(hipMemcpy2DAsync(xs_v, sizeof(T) * np, old->xs, sizeof(T) * np1, sizeof(T) * n1, d, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync((T*)xs_v + n1, sizeof(T) * np, sx2.ptr(), sizeof(T) * n2p, sizeof(T) * n2, d, hipMemcpyDeviceToDevice, s));
        // X = K(x2, x1) (n2p × np1; padding rows / columns zero), then X ← X L11⁻ᵀ = U12ᵀ                  :39
        RC(cross_solve<T>(old, s, bufs, sx2.ptr(), n2, n2p, 0, n2p, X, ldx));
        // S = C22 − U12ᵀ U12 (lower), chol(S) = U22ᵀ                                                       :40
        {
            GridMap g = plain_map(1, 0, 0);
            dim3 grid((unsigned)(n2p / 128), (unsigned)(n2p / 128));
            gram<T>(old->kern.desc(), grid, s, S, lds, sx2.ptr(), n2p, sx2.ptr(), n2p, d, (const T*)nz_v, n2, n2, 1, g);
            HIPCHK(hipGetLastError());
        }
        RC(launch_gemm<T>(c, s, S, lds, X, ldx, X, ldx, n2p, n2p, np1, plain_map(1, 0, 0)));
        if (noise_dense(noise2)) RC((dense_add<T, T>(c, bufs, S, lds, noise2, n2)));                         // C22 = cov(prior, x2) + Σy2      :50
        RC(potrf_full<T>(c, S, lds, n2p, n2p, c->info_dev, n2, c->scal_dev));
        // new factor [L11 0; U12ᵀ U22ᵀ], identity padding, δ as the right-hand side                          :41
        HIPCHK(hipMemsetAsync(A + np * ld, 0, sizeof(T) * (size_t)(128 + 128) * ld, s));
        HIPCHK(hipMemcpy2DAsync(A, sizeof(T) * ld, A1, sizeof(T) * ld1, sizeof(T) * n1, n1, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(A + n1 * ld, sizeof(T) * ld, X, sizeof(T) * ldx, sizeof(T) * n1, n2, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpy2DAsync(A + n1 * ld + n1, sizeof(T) * ld, S, sizeof(T) * lds, sizeof(T) * n2, n2, hipMemcpyDeviceToDevice, s));
        if (np > n) {
            hipLaunchKernelGGL(pad_identity_kernel<T>, dim3((unsigned)((np + 255) / 256), (unsigned)(np - n)), dim3(256), 0, s, A,
                               ld, n, np);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(alpha_v, delta_h.data(), v_b, hipMemcpyHostToDevice, s));
        RC(trsv<T>(c, s, A, ld, np, (T*)alpha_v, np, 1, true));                                     // z = L⁻¹ δ
        hipLaunchKernelGGL(rowsumsq_kernel<T>, dim3(1), dim3(256), 0, s, (const T*)alpha_v, np, np, c->scal_dev + 8);
        HIPCHK(hipGetLastError());
        RC(trsv<T>(c, s, A, ld, np, (T*)alpha_v, np, 1, false));                                    // α = L⁻ᵀ z        :53
        HIPCHK(hipMemcpyAsync(&info_h, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(scal_h, c->scal_dev, sizeof(double) * 16, hipMemcpyDeviceToHost, s));
        if (alpha_out) HIPCHK(hipMemcpyAsync(alpha_out, alpha_v, sizeof(T) * n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc == 0 && info_h != 0) rc = (int32_t)n1 + info_h;  // order of the failing leading minor of the bordered matrix
    if (rc != 0) return rc;
    bufs.keep(A_v);
    bufs.keep(xs_v);
    bufs.keep(alpha_v);
    post->ctx = c;
    post->dtype = old->dtype;
    post->n = n; post->np = np; post->ld = ld; post->mtot = mtot; post->d = d;
    post->kern = old->kern;
    post->A = A_v; post->A_bytes = A_b;
    post->xs = xs_v; post->xs_bytes = xs_b;
    post->alpha = alpha_v; post->alpha_bytes = v_b;
    post->logdet_half = old->logdet_half + scal_h[0];
    if (logpdf_out) *logpdf_out = -0.5 * ((double)n * LOG2PI + 2.0 * post->logdet_half + scal_h[8]);
    return 0;
}

template <typename T> static int32_t factor_mul_impl(gp_post* post, const void* xi, int ncols, void* out) {
    gp_ctx* c = post->ctx;
    const long n = post->n, np = post->np;
    void *in_v = 0, *out_v = 0;
    const size_t b = sizeof(T) * (size_t)np * ncols;
    DevBufs bufs(c);
    RC(bufs.get(b, &in_v));
    RC(bufs.get(b, &out_v));
    hipStream_t s = c->sm;
    return run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemsetAsync(in_v, 0, b, s));
        HIPCHK(hipMemcpy2DAsync(in_v, sizeof(T) * np, xi, sizeof(T) * n, sizeof(T) * n, ncols, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(trmv_lower_kernel<T>, dim3((unsigned)n), dim3(256), 0, s, (const T*)post->A, post->ld, (const T*)in_v, np,
                           ncols, (T*)out_v);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy2DAsync(out, sizeof(T) * n, out_v, sizeof(T) * np, sizeof(T) * n, ncols, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// out[:, s] = C \ B[:, s] with the resident factor (forward + backward vector sweeps, all columns per sweep)
template <typename T> static int32_t solve_impl(gp_post* post, const void* B, int ncols, void* out) {
    gp_ctx* c = post->ctx;
    const long n = post->n, np = post->np;
    void* r_v = 0;
    const size_t b = sizeof(T) * (size_t)np * ncols;
    DevBufs bufs(c);
    RC(bufs.get(b, &r_v));
    hipStream_t s = c->sm;
    return run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemsetAsync(r_v, 0, b, s));
        HIPCHK(hipMemcpy2DAsync(r_v, sizeof(T) * np, B, sizeof(T) * n, sizeof(T) * n, ncols, hipMemcpyHostToDevice, s));
        RC(trsv<T>(c, s, (const T*)post->A, post->ld, np, (T*)r_v, np, ncols, true));
        RC(trsv<T>(c, s, (const T*)post->A, post->ld, np, (T*)r_v, np, ncols, false));
        HIPCHK(hipMemcpy2DAsync(out, sizeof(T) * n, r_v, sizeof(T) * np, sizeof(T) * n, ncols, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// Joint predictive distribution on the device: logpdf(post(x*, Σy*), y*) and rand(post(x*, Σy*)) without leaving HBM.
// Reference: a FiniteGP over a PosteriorGP goes through the generic path — mean_and_cov(fx) (src/finite_gp_projection.jl:133-136
// on top of src/exact_gpr_posterior.jl:78-83), cholesky (:308 / :235), logdet + _sqmahal (:310, :325-326) or m + C.U'ξ (:236).
// TC = compute type of the N*×N* side (the posterior's dtype; always fp64 for VFE), TIO = host array type.
// ------------------------------------------------------------------------------------------------
template <typename TC> struct Joint {
    void* C = nullptr;  // (nsp + R + 128) × ld, row-major lower triangle of cov(f_post, x*) + Σy*, identity padding; R RHS rows
    long ns = 0, nsp = 0, ld = 0, R = 0;
    std::vector<double> mean;  // m(x*) + K_*· α  (host)
};

template <typename TC, typename TIO>
static void noise_to(const gp_noise* noise, long ns, long nsp, std::vector<TC>& out) {
    out.assign((size_t)nsp, TC(0));
    if (!noise) return;
    for (long i = 0; i < ns; ++i) out[i] = noise_entry<TC, TIO>(noise, i);
}

template <typename T>
static int32_t post_joint(gp_post* post, const gp_points* xs, const void* pm, const gp_noise* noise, long R, DevBufs& bufs,
                          Joint<T>& J) {
    gp_ctx* c = post->ctx;
    SkScope sk(c);
    const long np = post->np;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = post->d;
    const gp_kernel k = post->kern.view(post->dtype);
    StagedPoints<T> sx;
    std::vector<T> nz_h, m_h;
    noise_to<T, T>(noise, ns, nsp, nz_h);
    const long ldx = np + c->ldpad, ldc = nsp + c->ldpad;
    void *m_v = 0, *X_v = 0, *nz_v = 0;
    RC(sx.stage(c, bufs, &k, xs, nsp));
    RC(bufs.get(sizeof(T) * (size_t)nsp, &m_v));
    RC(bufs.get(sizeof(T) * (size_t)nsp, &nz_v));
    RC(bufs.get(sizeof(T) * (size_t)(nsp + 128) * ldx, &X_v));
    RC(bufs.get(sizeof(T) * (size_t)(nsp + R + 128) * ldc, &J.C));
    J.ns = ns; J.nsp = nsp; J.ld = ldc; J.R = R;
    T* X = (T*)X_v;
    T* Cm = (T*)J.C;
    hipStream_t s = c->sm;
    c->ev_used = 0;
    c->gemm_recs.clear();
    HIPCHK(hipMemcpyAsync(nz_v, nz_h.data(), sizeof(T) * (size_t)nsp, hipMemcpyHostToDevice, s));
    RC(post_mean<T>(post, s, sx.ptr(), ns, nsp, (T*)m_v, m_h));                                                // K_*x α
    RC(cross_solve<T>(post, s, bufs, sx.ptr(), ns, nsp, 0, nsp, X, ldx));                                      // V ᵀ = K_*x L⁻ᵀ
    {
        GridMap g = plain_map(1, 0, 0);
        dim3 grid((unsigned)(nsp / 128), (unsigned)(nsp / 128));
        gram<T>(post->kern.desc(), grid, s, Cm, ldc, sx.ptr(), nsp, sx.ptr(), nsp, d, (const T*)nz_v, ns, ns, 1, g);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(Cm + nsp * ldc, 0, sizeof(T) * (size_t)(R + 128) * ldc, s));
    RC(launch_gemm<T>(c, s, Cm, ldc, X, ldx, X, ldx, nsp, nsp, np, plain_map(1, 0, 0)));                       // K** + Σy* − VᵀV
    if (noise_dense(noise)) RC((dense_add<T, T>(c, bufs, Cm, ldc, noise, ns)));                                // a dense Σy*
    HIPCHK(hipStreamSynchronize(s));
    J.mean.resize((size_t)ns);
    add_prior_mean<T, double>((const T*)pm, m_h, J.mean.data());
    return 0;
}

// The same joint for a multi-device posterior whose factor still lives as block-cyclic pieces (fp64): mean from α, V ᵀV from the
// forward solve ON the pieces (multi.hip: multi_predict_var) — the factor is not gathered.
static int32_t post_joint_dist(gp_post* post, const gp_points* xs, const void* pm, const gp_noise* noise, long R, DevBufs& bufs,
                               Joint<double>& J) {
    gp_ctx* c = post->ctx;
    const long ns = xs->n, nsp = round_up(ns, 128);
    const int d = post->d;
    const gp_kernel k = post->kern.view(0);
    std::vector<double> m_h((size_t)ns), xs_n, xs_p, nz_h;
    RC(predict_impl<double>(post, xs, pm, 1, m_h.data(), nullptr, nullptr, false));   // m(x*) + K_*x α (no factor involved)
    scale_points<double>(&k, xs, ns, xs_n);
    scale_points<double>(&k, xs, nsp, xs_p);
    noise_to<double, double>(noise, ns, nsp, nz_h);
    std::vector<double> sub((size_t)ns), csub((size_t)ns * ns);
    RC(multi_predict_var(post, xs_n.data(), ns, ns, sub.data(), csub.data()));
    const long ldc = nsp + c->ldpad;
    void *xs_v = 0, *nz_v = 0, *W_v = 0;
    RC(bufs.get(sizeof(double) * (size_t)d * nsp, &xs_v));
    RC(bufs.get(sizeof(double) * (size_t)nsp, &nz_v));
    RC(bufs.get(sizeof(double) * (size_t)nsp * ldc, &W_v));
    RC(bufs.get(sizeof(double) * (size_t)(nsp + R + 128) * ldc, &J.C));
    J.ns = ns; J.nsp = nsp; J.ld = ldc; J.R = R;
    double* Cm = (double*)J.C;
    std::vector<double> W((size_t)nsp * ldc, 0.0);
    for (long i = 0; i < ns; ++i)
        for (long j = 0; j < ns; ++j) W[(size_t)i * ldc + j] = -csub[(size_t)i * ns + j];
    hipStream_t s = c->sm;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(xs_v, xs_p.data(), sizeof(double) * xs_p.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(nz_v, nz_h.data(), sizeof(double) * (size_t)nsp, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(W_v, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice, s));
    {
        GridMap g = plain_map(1, 0, 0);
        dim3 grid((unsigned)(nsp / 128), (unsigned)(nsp / 128));
        launch_kmat<double>(grid, s, Cm, ldc, (const double*)xs_v, nsp, (const double*)xs_v, nsp, d, post->kern.kind,
                           post->kern.variance, (const double*)nz_v, ns, ns, 1, g, (const double*)nullptr, (const double*)nullptr);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(Cm + nsp * ldc, 0, sizeof(double) * (size_t)(R + 128) * ldc, s));
    RC(gpmi::eng_add_vec(c, s, Cm, (const double*)W_v, nsp * ldc));                                           // K** + Σy* − VᵀV
    if (noise_dense(noise)) RC((dense_add<double, double>(c, bufs, Cm, ldc, noise, ns)));                     // a dense Σy*
    HIPCHK(hipStreamSynchronize(s));
    J.mean.assign(m_h.begin(), m_h.end());
    return 0;
}

// logpdf of Y (ns × ncols column-major host, leading dimension ldy) under N(J.mean, J.C): factor J.C in place with δ rows riding along
template <typename TC, typename TIO>
static int32_t joint_logpdf(gp_ctx* c, Joint<TC>& J, const void* Yv, long ldy, int ncols, void* outv) {
    const long ns = J.ns, nsp = J.nsp, ld = J.ld;
    TC* Cm = (TC*)J.C;
    hipStream_t s = c->sm;
    const TIO* Y = (const TIO*)Yv;
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 8 + J.R));
    std::vector<TC> rhs((size_t)ncols * nsp, TC(0));
    for (int q = 0; q < ncols; ++q)
        for (long i = 0; i < ns; ++i) rhs[(size_t)q * nsp + i] = (TC)((double)Y[(size_t)q * ldy + i] - J.mean[i]);
    int info_h = 0;
    std::vector<double> scal_h(8 + ncols);
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemsetAsync(c->info_dev, 0, sizeof(int), s));
        HIPCHK(hipMemsetAsync(c->scal_dev, 0, sizeof(double) * (8 + J.R), s));
        HIPCHK(hipMemcpy2DAsync(Cm + nsp * ld, sizeof(TC) * ld, rhs.data(), sizeof(TC) * nsp, sizeof(TC) * nsp, ncols,
                                hipMemcpyHostToDevice, s));
        RC(potrf_full<TC>(c, Cm, ld, nsp, nsp + J.R, c->info_dev, ns, c->scal_dev));
        hipLaunchKernelGGL(rowsumsq_kernel<TC>, dim3((unsigned)ncols), dim3(256), 0, s, Cm + nsp * ld, ld, nsp, c->scal_dev + 8);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&info_h, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(scal_h.data(), c->scal_dev, sizeof(double) * (8 + ncols), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc != 0) return rc;
    if (info_h != 0) return info_h;
    for (int q = 0; q < ncols; ++q)
        ((TIO*)outv)[q] = (TIO)(-0.5 * ((double)ns * LOG2PI + 2.0 * scal_h[0] + scal_h[8 + q]));
    return 0;
}

// out[:, q] = J.mean + chol(J.C)ᵀ-factor product with xi[:, q]  (ns × ncols column-major host arrays, leading dimension ns)
template <typename TC, typename TIO>
static int32_t joint_rand(gp_ctx* c, Joint<TC>& J, DevBufs& bufs, const void* xiv, int ncols, void* outv) {
    const long ns = J.ns, nsp = J.nsp, ld = J.ld;
    TC* Cm = (TC*)J.C;
    hipStream_t s = c->sm;
    const TIO* xi = (const TIO*)xiv;
    if (!c->info_dev) HIPCHK(hipMalloc((void**)&c->info_dev, sizeof(int)));
    RC(ctx_scal(c, 16));
    std::vector<TC> in_h((size_t)ncols * nsp, TC(0)), out_h((size_t)ncols * nsp);
    for (int q = 0; q < ncols; ++q)
        for (long i = 0; i < ns; ++i) in_h[(size_t)q * nsp + i] = (TC)xi[(size_t)q * ns + i];
    void *in_v = 0, *out_v = 0;
    const size_t b = sizeof(TC) * (size_t)nsp * ncols;
    RC(bufs.get(b, &in_v));
    RC(bufs.get(b, &out_v));
    int info_h = 0;
    const int32_t rc = run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemsetAsync(c->info_dev, 0, sizeof(int), s));
        HIPCHK(hipMemsetAsync(c->scal_dev, 0, sizeof(double) * 16, s));
        HIPCHK(hipMemcpyAsync(in_v, in_h.data(), b, hipMemcpyHostToDevice, s));
        RC(potrf_full<TC>(c, Cm, ld, nsp, nsp, c->info_dev, ns, c->scal_dev));
        hipLaunchKernelGGL(trmv_lower_kernel<TC>, dim3((unsigned)ns), dim3(256), 0, s, (const TC*)Cm, ld, (const TC*)in_v, nsp, ncols,
                           (TC*)out_v);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&info_h, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_h.data(), out_v, b, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    });
    if (rc != 0) return rc;
    if (info_h != 0) return info_h;
    for (int q = 0; q < ncols; ++q)
        for (long i = 0; i < ns; ++i) ((TIO*)outv)[(size_t)q * ns + i] = (TIO)(J.mean[i] + (double)out_h[(size_t)q * nsp + i]);
    return 0;
}

#include "vfe.hpp"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int32_t gp_abi_version(void) { return GPMI355_ABI_VERSION; }
const char* gp_last_error(void) { return g_err.c_str(); }

int32_t gp_ctx_create(gp_ctx** out, int32_t device, void* stream_or_null) {
    if (!out) return set_arg_err(1, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_arg_err(2, "no such device");
    HIPCHK(hipSetDevice(device));
    gp_ctx* c = new gp_ctx();
    c->device = device;
    if (stream_or_null) {
        c->sm = (hipStream_t)stream_or_null;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->sm, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return set_hip_err(e, "hipStreamCreate", __LINE__);
        }
        c->own_sm = true;
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    }
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    hipError_t e = hipStreamCreateWithPriority(&c->sp, hipStreamNonBlocking, hi);
    if (e != hipSuccess) {
        if (c->own_sm) (void)hipStreamDestroy(c->sm);
        delete c;
        return set_hip_err(e, "hipStreamCreateWithPriority", __LINE__);
    }
    reg_add(c);
    *out = c;
    // GPMI_PARAMS="name=value,name=value": tuning overrides for experiments (same names as gp_ctx_set_param)
    if (const char* s = getenv("GPMI_PARAMS")) {
        std::string all(s);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t e = all.find(',', pos);
            if (e == std::string::npos) e = all.size();
            const std::string kv = all.substr(pos, e - pos);
            const size_t q = kv.find('=');
            if (q != std::string::npos) (void)gp_ctx_set_param(c, kv.substr(0, q).c_str(), atoll(kv.c_str() + q + 1));
            pos = e + 1;
        }
    }
    return 0;
}

int32_t gp_ctx_destroy(gp_ctx* c) {
    if (!c || !reg_take(c)) return set_arg_err(1, "not a live gp_ctx");
    gp_multi* multi = nullptr;
    {
        std::lock_guard<std::mutex> l(c->mu);
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->sm);
        (void)hipStreamSynchronize(c->sp);
        c->dead = true;
        multi = c->multi;
        c->multi = nullptr;
    }
    if (multi) multi_destroy(multi);  // rank contexts, comm streams, RCCL communicators (factor pieces still alive keep their rank ctx)
    (void)hipSetDevice(c->device);
    ctx_unref(c);
    return 0;
}

int32_t gp_ctx_set_param(gp_ctx* c, const char* name, int64_t v) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (!name) return set_arg_err(2, "name is NULL");
    if (c->multi && multi_set_param(c, name, v) == 0) return 0;  // (generic names are forwarded to the rank contexts too)
    if (!strcmp(name, "nb")) c->nb = v < 0 ? -1 : (v == 0 ? 0 : round_up(v, 128));
    else if (!strcmp(name, "nb_small")) c->nb_small = (v <= 0) ? 0 : round_up(v, 128);
    else if (!strcmp(name, "nb_large")) c->nb_large = (v <= 0) ? 0 : round_up(v, 128);
    else if (!strcmp(name, "nb_huge")) c->nb_huge = (v <= 0) ? 0 : round_up(v, 128);
    else if (!strcmp(name, "nb_huge_min_n")) c->nb_huge_min_n = std::max<int64_t>(0, v);
    else if (!strcmp(name, "lookahead")) c->lookahead = v != 0;
    else if (!strcmp(name, "lookahead_min_n")) c->lookahead_min_n = std::max<int64_t>(0, v);
    else if (!strcmp(name, "time_kernels")) c->time_kernels = v != 0;
    else if (!strcmp(name, "xcd_swizzle")) c->xcd_swizzle = v != 0;
    else if (!strcmp(name, "strassen_min_rows")) {
        c->strassen_min_rows = v <= 0 ? 0 : round_up(v, 256);
        c->strassen_min_rows_set = true;  // from here on it applies at every size ("strassen_min_rows_large" no longer does)
    } else if (!strcmp(name, "strassen_min_rows_large")) c->strassen_min_rows_large = v <= 0 ? 0 : round_up(v, 256);
    else if (!strcmp(name, "strassen_u1_min_rows")) c->strassen_u1_min_rows = v <= 0 ? 0 : round_up(v, 256);
    else if (!strcmp(name, "strassen_u1_min_k")) c->strassen_u1_min_k = std::max<int64_t>(0, v);
    else if (!strcmp(name, "strassen_group")) c->strassen_group = v != 0;
    else if (!strcmp(name, "strassen_group_min_rows")) c->strassen_group_min_rows = std::max<int64_t>(256, round_up(v, 256));
    else if (!strcmp(name, "gemm_streamk")) c->gemm_streamk = v != 0;
    else if (!strcmp(name, "sk_max_tiles")) c->sk_max_tiles = v;
    else if (!strcmp(name, "sk_min_k")) c->sk_min_k = v;
    else if (!strcmp(name, "gemm_pipe")) c->gemm_pipe = v != 0;
    else if (!strcmp(name, "kmat_rows")) g_kmat_rows = v != 0;
    else if (!strcmp(name, "dib_nb")) c->dib_nb = v <= 0 ? 0 : std::min<int64_t>(round_up(std::max<int64_t>(v, 128), 128), 8192);
    else if (!strcmp(name, "gemm_pad_f32")) c->gemm_pad_f32 = std::min<int64_t>(std::max<int64_t>(0, v), 32768);
    else if (!strcmp(name, "gemm_pad_lds")) {
        c->gemm_pad_lds = std::min<int64_t>(std::max<int64_t>(0, v), 32768);
        c->gemm_pad_user = true;
    }
    else if (!strcmp(name, "trsv_nb")) c->trsv_nb = v >= 1024 ? 1024 : (v >= 512 ? 512 : (v >= 256 ? 256 : 128));
    else if (!strcmp(name, "deterministic")) c->deterministic = v != 0;
    else if (!strcmp(name, "leaf_v2")) c->leaf_v2 = v != 0;
    else if (!strcmp(name, "leaf_xr")) c->leaf_xr = v == 64 ? 64 : (v == 128 ? 128 : 0);
    else if (!strcmp(name, "leaf_cols")) c->leaf_cols = v == 64 ? 64 : 128;
    else if (!strcmp(name, "updk_max_k")) c->updk_max_k = std::max<int64_t>(0, v);
    else if (!strcmp(name, "updk_rt")) c->updk_rt = (int)v;
    else if (!strcmp(name, "updk_tall_k")) c->updk_tall_k = std::max<int64_t>(0, v);
    else if (!strcmp(name, "updk_tall_m")) c->updk_tall_m = std::max<int64_t>(0, v);
    else if (!strcmp(name, "upd128")) c->upd128 = v != 0;
    else if (!strcmp(name, "leaf_group")) c->leaf_group = v < 128 ? 64 : (v >= 512 ? 512 : (v >= 256 ? 256 : 128));
    else if (!strcmp(name, "xcd_min_tiles")) c->xcd_min_tiles = v;
    else if (!strcmp(name, "ldpad")) c->ldpad = round_up(std::max<int64_t>(0, v), 16);
    else if (!strcmp(name, "dense_stage_mb")) c->dense_stage_mb = std::min<int64_t>(std::max<int64_t>(1, v), 256);
    else if (!strcmp(name, "vfe_ks")) c->vfe_ks = std::max<int64_t>(512, round_up(v, 512));
    else if (!strcmp(name, "vfe_sk")) c->vfe_sk = v != 0;
    else if (!strcmp(name, "vfe_dual")) c->vfe_dual = v != 0;
    else if (!strcmp(name, "vfe_inv_nb")) c->vfe_inv_nb = v <= 0 ? 0 : round_up(v, 128);
    else if (!strcmp(name, "vfe_overlap")) c->vfe_overlap = v != 0;
    else if (!strcmp(name, "vfe_chunk")) c->vfe_chunk = v <= 0 ? 0 : std::max<int64_t>(2048, round_up(v, 2048));
    else if (!strcmp(name, "pool_cap_mb")) c->pool_cap = (size_t)std::max<int64_t>(0, v) << 20;
    else if (!strcmp(name, "alloc_poison")) c->alloc_poison = v != 0;
    else if (!strcmp(name, "lookahead_depth") || !strcmp(name, "dist_nb") || !strcmp(name, "copy_kernel") || !strcmp(name, "multi_debug_sync") ||
             !strcmp(name, "multi_check") || !strcmp(name, "multi_verify") || !strcmp(name, "multi_inject_fault") || !strcmp(name, "multi_dist_predict") || !strcmp(name, "multi_window") || !strcmp(name, "multi_timeout_s") || !strcmp(name, "multi_gemm_streamk") || !strcmp(name, "multi_leaf_cols")) return c->multi ? 0 : set_arg_err(2, "multi-device parameter on a single-device ctx");
    else return set_arg_err(2, "unknown parameter");
    return 0;
}

int32_t gp_ctx_get_param(gp_ctx* c, const char* name, int64_t* out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (!name) return set_arg_err(2, "name is NULL");
    if (!out) return set_arg_err(3, "out is NULL");
    if (c->multi && multi_get_param(c, name, out) == 0) return 0;
    if (!strcmp(name, "batch_grad_kernel_problems")) {  // read-only state, not a parameter: how many problems the batched gradient kernels have served
        *out = c->batch_grad_problems;
        return 0;
    }
    if (!strcmp(name, "batch_pgrad_kernel_problems")) {  // the same for batch_pgrad_kernel (gp_predict_grad_batch / _sum)
        *out = c->batch_pgrad_problems;
        return 0;
    }
    if (!strcmp(name, "batch_gradx_kernel_problems")) {  // the same for batch_gradx_kernel (gp_logpdf_grad_batch_x / _sum_x with a dx array)
        *out = c->batch_gradx_problems;
        return 0;
    }
    if (!strcmp(name, "batch_loo_kernel_problems")) {  // the same for batch_loo_kernel (gp_loo_batch / _sum)
        *out = c->batch_loo_problems;
        return 0;
    }
    if (!strcmp(name, "batch_loo_grad_kernel_problems")) {  // the same for the kernels of gp_loo_grad_batch / _sum
        *out = c->batch_loo_grad_problems;
        return 0;
    }
    if (!strcmp(name, "cols_kernel_calls")) {  // kmul launches served by gp_posterior_predict_cols / gp_vfe_predict_cols since the ctx was created
        *out = c->cols_kernel_calls;
        return 0;
    }
    if (!strcmp(name, "cols_kernel_splits")) {  // workgroups along the training range of the last kmul launch (1: no partial sums; 0: none yet)
        *out = c->cols_kernel_splits;
        return 0;
    }
    if (!strcmp(name, "batch_joint_kernel_problems")) {  // the same for the kernels of gp_joint_batch / _sum (batch_jcov_kernel, batch_jfact_kernel)
        *out = c->batch_joint_problems;
        return 0;
    }
    const struct { const char* n; int64_t v; } tab[] = {
        {"nb", c->nb}, {"nb_small", c->nb_small}, {"nb_large", c->nb_large}, {"nb_huge", c->nb_huge}, {"nb_huge_min_n", c->nb_huge_min_n}, {"strassen_u1_min_rows", c->strassen_u1_min_rows}, {"strassen_u1_min_k", c->strassen_u1_min_k}, {"lookahead", c->lookahead}, {"lookahead_min_n", c->lookahead_min_n}, {"time_kernels", c->time_kernels},
        {"xcd_swizzle", c->xcd_swizzle}, {"strassen_min_rows", c->strassen_min_rows}, {"strassen_min_rows_large", c->strassen_min_rows_large}, {"strassen_group", c->strassen_group}, {"strassen_group_min_rows", c->strassen_group_min_rows}, {"xcd_min_tiles", c->xcd_min_tiles}, {"gemm_streamk", c->gemm_streamk},
        {"sk_max_tiles", c->sk_max_tiles}, {"sk_min_k", c->sk_min_k}, {"gemm_pipe", c->gemm_pipe}, {"gemm_pad_f32", c->gemm_pad_f32},
        {"gemm_pad_lds", c->gemm_pad_user ? c->gemm_pad_lds : 0}, {"trsv_nb", c->trsv_nb},  {"deterministic", c->deterministic},
        {"leaf_v2", c->leaf_v2}, {"leaf_xr", c->leaf_xr}, {"leaf_cols", c->leaf_cols}, {"updk_max_k", c->updk_max_k}, {"updk_rt", c->updk_rt},
        {"updk_tall_k", c->updk_tall_k}, {"updk_tall_m", c->updk_tall_m}, {"upd128", c->upd128}, {"leaf_group", c->leaf_group},
        {"ldpad", c->ldpad}, {"dense_stage_mb", c->dense_stage_mb}, {"vfe_ks", c->vfe_ks}, {"vfe_sk", c->vfe_sk}, {"vfe_dual", c->vfe_dual}, {"vfe_inv_nb", c->vfe_inv_nb}, {"vfe_overlap", c->vfe_overlap}, {"vfe_chunk", c->vfe_chunk},
        {"kmat_rows", g_kmat_rows.load()}, {"dib_nb", c->dib_nb}, {"pool_cap_mb", (int64_t)(c->pool_cap >> 20)}, {"alloc_poison", c->alloc_poison},
        {"pool_cached_mb", (int64_t)(c->pool_bytes >> 20)}, {"pool_blocks", (int64_t)c->pool.size()}};  // the last two are read-only
    for (const auto& e : tab)
        if (!strcmp(name, e.n)) {
            *out = e.v;
            return 0;
        }
    return set_arg_err(2, "unknown parameter");
}

int32_t gp_ctx_trim(gp_ctx* c) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->sm);
    (void)hipStreamSynchronize(c->sp);
    while (!c->pool.empty()) pool_drop(c, c->pool.size() - 1);
    if (c->multi) multi_trim(c);  // the rank contexts cache their own blocks (matrix pieces, operand buffers)
    return 0;
}

int32_t gp_get_timings(gp_ctx* c, gp_timings* out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (!out) return set_arg_err(2, "out is NULL");
    *out = c->tm;
    return 0;
}

// Validates a gp_ksum (limits and malformed descriptors: −argi with the reason) and packs it for the device.  kid: the single-kind descriptor
// the engine carries beside it — kind 0, no transform (the inputs stay raw), variance Σ_t σ_t² (the prior variance k(x, x)).
extern "C++" int32_t pack_ksum(const gp_ksum* k, int d, int argi, KSum& ks, gp_kernel& kid) {
    if (!k) return set_arg_err(argi, "kernel is NULL");
    if (k->dtype != 0 && k->dtype != 1) return set_arg_err(argi, "dtype must be 0 (f64) or 1 (f32)");
    if (k->nterms < 1 || k->nterms > KSum::MAXT) return set_arg_err(argi, "composite kernel: 1..8 terms");
    if (!k->terms) return set_arg_err(argi, "composite kernel: terms is NULL");
    if (d > KSum::MAXD) return set_arg_err(argi, "composite kernel: D must be <= 16");
    ks = KSum{};
    int nf = 0, nth = 0;
    double vsum = 0;
    const char* too_many = "composite kernel: at most 64 entries in theta";
    for (int t = 0; t < k->nterms; ++t) {
        const gp_kterm& tm = k->terms[t];
        if (!(tm.variance > 0)) return set_arg_err(argi, "composite kernel: term variance must be > 0");
        if (tm.nfactors < 1 || tm.nfactors > KSum::MAXFT) return set_arg_err(argi, "composite kernel: 1..4 factors per term");
        if (!tm.factors) return set_arg_err(argi, "composite kernel: factors is NULL");
        if (nf + tm.nfactors > KSum::MAXF) return set_arg_err(argi, "composite kernel: at most 16 factors in all");
        if (nth >= KSum::MAXTH) return set_arg_err(argi, too_many);
        ks.t0[t] = nf;
        ks.tv[t] = nth;
        ks.th[nth++] = tm.variance;
        vsum += tm.variance;
        for (int j = 0; j < tm.nfactors; ++j, ++nf) {
            const gp_kfactor& f = tm.factors[j];
            if (f.kind < 0 || f.kind > 6) return set_arg_err(argi, "composite kernel: factor kind must be 0..6");
            if (f.nscale != 0 && f.nscale != 1 && f.nscale != d) return set_arg_err(argi, "composite kernel: nscale must be 0, 1 or D");
            if (f.nscale > 0 && !f.scale) return set_arg_err(argi, "composite kernel: scale is NULL");
            if (f.kind == 6 && f.nscale != 0) return set_arg_err(argi, "composite kernel: WhiteKernel takes no transform");
            const int want = f.kind == 4 ? d : (f.kind == 5 ? 1 : 0);
            if (f.nparam != want)
                return set_arg_err(argi, "composite kernel: param holds D entries (r) for kind 4, 1 (alpha) for kind 5, none otherwise");
            if (want > 0 && !f.param) return set_arg_err(argi, "composite kernel: param is NULL");
            for (int q = 0; q < want; ++q)
                if (!(f.param[q] > 0)) return set_arg_err(argi, "composite kernel: Periodic r and RationalQuadratic alpha must be > 0");
            if (nth + f.nscale + want > KSum::MAXTH) return set_arg_err(argi, too_many);
            ks.kind[nf] = f.kind;
            ks.ns[nf] = f.nscale;
            ks.so[nf] = nth;
            for (int q = 0; q < f.nscale; ++q) ks.th[nth++] = f.scale[q];
            ks.po[nf] = nth;
            for (int q = 0; q < want; ++q) ks.th[nth++] = f.param[q];
        }
    }
    ks.t0[k->nterms] = nf;
    ks.nterms = k->nterms;
    ks.nth = nth;
    kid = gp_kernel{};
    kid.kind = 0;
    kid.dtype = k->dtype;
    kid.variance = vsum;
    kid.nscale = 0;
    kid.scale = nullptr;
    return 0;
}

// noise kinds (include/gpmi355.h): 0 σ²·I, 1 Diagonal, 2 / 3 dense (upper / lower triangle of a column-major n×n host array).  dense_ok = false: the sparse
// fits, where the reference needs cholesky(Σy) — an N×N factorisation that defeats the sparse cost (src/sparse_approximations.jl:61, :97) — and whose elbo
// has no trace term for a dense Σy at all (:307-313).
extern "C++" int32_t check_noise(const gp_noise* noise, int argi, bool dense_ok) {
    if (!noise) return set_arg_err(argi, "noise is NULL");
    if (noise->kind < 0 || noise->kind > 3) return set_arg_err(argi, "noise kind must be 0 (scalar), 1 (diagonal), 2 or 3 (dense, upper / lower triangle)");
    if (noise->kind >= 2 && !dense_ok)
        return set_arg_err(argi, "dense noise (kind 2 / 3) is not offered for VFE / DTC fits: the reference factors Σy there (an N×N Cholesky that defeats the sparse "
                                 "cost) and its elbo has no method for a dense Σy");
    if (noise->kind != 0 && !noise->diag) return set_arg_err(argi, noise->kind == 1 ? "noise diag is NULL" : "noise diag (the dense matrix) is NULL");
    return 0;
}

// The kernel of one call as the engine carries it.  Single kind: the caller's gp_kernel.  Composite (the *_sum calls): the packed terms `ks` beside the
// kind-0 descriptor without a transform (the inputs stay raw) whose variance is Σ_t σ_t² — what pack_ksum returns.
struct ResolvedKernel {
    gp_kernel k{};
    KSum ks;  // filled when composite
    bool composite = false;
    const KSum* sum() const { return composite ? &ks : nullptr; }
};
static int32_t resolve_kernel(const gp_kernel* k, int d, int argi, ResolvedKernel& rk) {
    RC(check_kernel(k, d, argi));
    rk.k = *k;
    return 0;
}
static int32_t resolve_kernel(const gp_ksum* k, int d, int argi, ResolvedKernel& rk) {
    rk.composite = true;
    return pack_ksum(k, d, argi, rk.ks, rk.k);
}

// One (logpdf, posterior) pair on whatever the ctx drives: the 2D block-cyclic driver (multi.hip) for fp64 single-kind fits with at most
// 128 right-hand sides on a multi-device ctx, the single-device engine (devices[0] of a multi-device ctx) for everything else — composite kernels and fits
// with a dense Σy (noise kind 2 / 3) among them: the block-cyclic driver is single-kind and takes a scalar or a vector noise only.
static int32_t fit_any(gp_ctx* c, const ResolvedKernel& rk, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y,
                       long ldy, int ncols, FitOut& fo, gp_post* p, void* alpha_out) {
    const gp_kernel* k = &rk.k;
    if (c->multi && !rk.composite && k->dtype == 0 && ncols <= 128 && !noise_dense(noise) && !(p && ncols > 1)) {  // (a column posterior: single-device engine)
        fo.logpdf.assign((size_t)ncols, 0.0);
        std::vector<double> terms((size_t)ncols + 1, 0.0);
        RC(multi_fit(c, k, x, noise, mean, Y, ldy, ncols, fo.logpdf.data(), terms.data(), p, alpha_out));
        fo.logdet = terms[0];
        fo.sqmahal.assign(terms.begin() + 1, terms.end());
        return 0;
    }
    return by_dtype(k->dtype, [&](auto t) { return fit_impl<decltype(t)>(c, k, x, noise, mean, Y, ldy, ncols, fo, p, alpha_out, rk.sum()); });
}

// ---- the bodies gp_X and gp_X_sum share (K: gp_kernel or gp_ksum; everything after the kernel argument's check is one path) ----
extern "C++" {
template <class K>
static int32_t check_fit_args(const K* k, const gp_points* x, const gp_noise* noise, ResolvedKernel& rk, bool dense_ok = true) {
    RC(check_points(x, 3));
    RC(resolve_kernel(k, x->d, 2, rk));
    return check_noise(noise, 4, dense_ok);
}

template <class K> static int32_t kernelmatrix_any(gp_ctx* c, const K* k, const gp_points* x, const gp_points* y, void* out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    RC(check_points(x, 3));
    ResolvedKernel rk;
    RC(resolve_kernel(k, x->d, 2, rk));
    if (y) {
        RC(check_points(y, 4));
        if (y->d != x->d) return set_arg_err(4, "x and y have different D");
    }
    if (!out) return set_arg_err(5, "out is NULL");
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(rk.k.dtype, [&](auto tag) -> int32_t {
        using T = decltype(tag);
        // device rows = y points (or x), device cols = x points: row-major (m×n) == column-major (n×m)
        const gp_points* rp = y ? y : x;
        const long n = x->n, m = rp->n, np = round_up(n, 128), mp = round_up(m, 128);
        const long ld = np + c->ldpad;
        StagedPoints<T> xc, xr;
        void* K_v = nullptr;
        DevBufs bufs(c);
        return run_drained(c, [&]() -> int32_t {
            RC(xc.stage(c, bufs, &rk.k, x, np));
            if (y) RC(xr.stage(c, bufs, &rk.k, y, mp));
            RC(bufs.get(sizeof(T) * (size_t)mp * ld, &K_v));
            GridMap g = plain_map(0, 0, 0);
            dim3 grid((unsigned)(np / 128), (unsigned)(mp / 128));
            gram<T>(KDesc{rk.k.kind, rk.k.variance, rk.sum()}, grid, c->sm, (T*)K_v, ld, y ? xr.ptr() : xc.ptr(), y ? mp : np, xc.ptr(), np,
                    x->d, (const T*)nullptr, m, n, 0, g);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy2DAsync(out, sizeof(T) * n, K_v, sizeof(T) * ld, sizeof(T) * n, m, hipMemcpyDeviceToHost,
                                    c->sm));
            HIPCHK(hipStreamSynchronize(c->sm));
            return 0;
        });
    });
}

template <class K>
static int32_t logpdf_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                          int32_t ncols, void* out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!Y) return set_arg_err(6, "Y is NULL");
    if (ncols < 1) return set_arg_err(8, "ncols must be >= 1");
    if (ldy < x->n) return set_arg_err(7, "ldy < n");
    if (!out) return set_arg_err(9, "out is NULL");
    HIPCHK(hipSetDevice(c->device));
    FitOut fo;
    RC(fit_any(c, rk, x, noise, mean, Y, ldy, ncols, fo, nullptr, nullptr));
    for (int s = 0; s < ncols; ++s) put(out, rk.k.dtype, s, fo.logpdf[s]);
    return 0;
}

template <class K>
static int32_t posterior_fit_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, gp_post** out,
                                 void* alpha_out, void* logpdf_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!y) return set_arg_err(6, "y is NULL");
    if (!out) return set_arg_err(7, "out is NULL");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    auto p = std::make_unique<gp_post>();
    p->ctx = c;
    FitOut fo;
    RC(fit_any(c, rk, x, noise, mean, y, x->n, 1, fo, p.get(), alpha_out));
    if (logpdf_out) put(logpdf_out, rk.k.dtype, 0, fo.logpdf[0]);
    publish(c, p, out);
    return 0;
}

// gp_posterior_fit_cols / _sum: posterior_fit_any for Y of ncols <= GPMI355_COLS_MAX columns; the handle keeps α for every column
template <class K>
static int32_t posterior_fit_cols_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                                      int32_t ncols, gp_post** out, void* alpha_out, void* logpdf_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!Y) return set_arg_err(6, "Y is NULL");
    if (ldy < x->n) return set_arg_err(7, "ldy < n");
    if (ncols < 1 || ncols > GPMI355_COLS_MAX) return set_arg_err(8, "ncols must be 1..GPMI355_COLS_MAX (128): split more columns into groups");
    if (!out) return set_arg_err(9, "out is NULL");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    auto p = std::make_unique<gp_post>();
    p->ctx = c;
    FitOut fo;
    RC(fit_any(c, rk, x, noise, mean, Y, ldy, ncols, fo, p.get(), alpha_out));
    if (logpdf_out)
        for (int s = 0; s < ncols; ++s) put(logpdf_out, rk.k.dtype, s, fo.logpdf[s]);
    publish(c, p, out);
    return 0;
}

// gp_logpdf_grad_cols / _sum: logpdf_grad_any for the sum over the columns of Y
template <class K>
static int32_t logpdf_grad_cols_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                                    int32_t ncols, void* logpdf_out, double* dvar, double* dscale, void* dnoise, void* dY, void* dx, double* dtheta) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!Y) return set_arg_err(6, "Y is NULL");
    if (ldy < x->n) return set_arg_err(7, "ldy < n");
    if (ncols < 1 || ncols > GPMI355_COLS_MAX) return set_arg_err(8, "ncols must be 1..GPMI355_COLS_MAX (128): split more columns into groups");
    if (!logpdf_out) return set_arg_err(9, "logpdf_out is NULL");
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(rk.k.dtype, [&](auto t) {
        return grad_logpdf_cols<decltype(t)>(c, &rk.k, x, noise, mean, Y, (long)ldy, ncols, logpdf_out, dvar, dscale, dnoise, dY, dx, rk.sum(), dtheta);
    });
}

// single kind: dvar / dscale / dx, dtheta NULL; composite: dtheta (one entry per θ entry) and dx, dvar / dscale NULL
template <class K>
static int32_t logpdf_grad_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* logpdf_out,
                               double* dvar, double* dscale, void* dnoise, void* dy, void* dx, double* dtheta, bool loo) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!y) return set_arg_err(6, "y is NULL");
    if (!logpdf_out) return set_arg_err(7, loo ? "value_out is NULL" : "logpdf_out is NULL");
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(rk.k.dtype, [&](auto t) {
        using T = decltype(t);
        if (loo) return grad_loo<T>(c, &rk.k, x, noise, mean, y, logpdf_out, dvar, dscale, dnoise, dy, dx, rk.sum(), dtheta);
        return grad_logpdf_cols<T>(c, &rk.k, x, noise, mean, y, x->n, 1, logpdf_out, dvar, dscale, dnoise, dy, dx, rk.sum(), dtheta);  // one column
    });
}

// gp_loo / gp_loo_sum: the leave-one-out predictions and Σ_i log p(y_i | y_−i) (argument checks as logpdf_grad_any)
template <class K>
static int32_t loo_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out, void* lp_out,
                       void* mean_out, void* var_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (!y) return set_arg_err(6, "y is NULL");
    if (!value_out) return set_arg_err(7, "value_out is NULL");
    HIPCHK(hipSetDevice(c->device));
    LooOut out;
    out.lp = lp_out; out.mean = mean_out; out.var = var_out;
    return by_dtype(rk.k.dtype, [&](auto t) { return loo_impl<decltype(t)>(c, &rk.k, x, noise, mean, y, value_out, out, rk.sum()); });
}

// logdet(cov(fx)) and sqmahal(fx, Y) — the two terms logpdf adds up (src/finite_gp_projection.jl:306-311): `logdetcov` is not in
// the reference's API by that name but `sqmahal` is (src/finite_gp_projection.jl:313-326), and `gradlogpdf` (:328-337) is −α of
// the posterior fit.  Y may be NULL (ncols ignored): logdet only.  Outputs in the kernel's dtype; either may be NULL.
template <class K>
static int32_t logpdf_terms_any(gp_ctx* c, const K* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                                int32_t ncols, void* logdet_out, void* sqmahal_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk));
    if (Y) {
        if (ncols < 1) return set_arg_err(8, "ncols must be >= 1");
        if (ldy < x->n) return set_arg_err(7, "ldy < n");
    } else if (sqmahal_out) {
        return set_arg_err(6, "sqmahal needs Y");
    }
    HIPCHK(hipSetDevice(c->device));
    FitOut fo;
    std::vector<char> zero;
    if (!Y) {
        // logdet only: the factorisation is all that is needed, but a multi-device fit verifies its result through the right-hand
        // side that rides along ((K + Σy) α = δ on every row) — an all-zero δ would make that check vacuous (α = 0 whatever the
        // factor holds).  A fixed pseudo-random probe in [−½, ½) rides instead; its sqmahal is discarded.
        zero.assign((size_t)x->n * (rk.k.dtype == 0 ? 8 : 4), 0);
        for (int64_t i = 0; i < x->n; ++i)
            put(zero.data(), rk.k.dtype, (size_t)i, (double)(((uint32_t)i * 2654435761u >> 8) & 0xffffu) / 65536.0 - 0.5 + 1.0 / 131072.0);
        ncols = 1;
        ldy = x->n;
    }
    RC(fit_any(c, rk, x, noise, Y ? mean : nullptr, Y ? Y : (const void*)zero.data(), ldy, ncols, fo, nullptr, nullptr));
    if (logdet_out) put(logdet_out, rk.k.dtype, 0, fo.logdet);
    if (sqmahal_out)
        for (int s = 0; s < ncols; ++s) put(sqmahal_out, rk.k.dtype, s, fo.sqmahal[s]);
    return 0;
}
}  // extern "C++"

int32_t gp_kernelmatrix(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_points* y, void* out) { return kernelmatrix_any(c, k, x, y, out); }
int32_t gp_kernelmatrix_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_points* y, void* out) { return kernelmatrix_any(c, k, x, y, out); }

int32_t gp_logpdf(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean,
                  const void* Y, int64_t ldy, int32_t ncols, void* out) {
    return logpdf_any(c, k, x, noise, mean, Y, ldy, ncols, out);
}
int32_t gp_logpdf_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                      int32_t ncols, void* out) {
    return logpdf_any(c, k, x, noise, mean, Y, ldy, ncols, out);
}

int32_t gp_posterior_fit(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean,
                         const void* y, gp_post** out, void* alpha_out, void* logpdf_out) {
    return posterior_fit_any(c, k, x, noise, mean, y, out, alpha_out, logpdf_out);
}
int32_t gp_posterior_fit_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, gp_post** out,
                             void* alpha_out, void* logpdf_out) {
    return posterior_fit_any(c, k, x, noise, mean, y, out, alpha_out, logpdf_out);
}

int32_t gp_posterior_fit_cols(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                              int32_t ncols, gp_post** out, void* alpha_out, void* logpdf_out) {
    return posterior_fit_cols_any(c, k, x, noise, mean, Y, ldy, ncols, out, alpha_out, logpdf_out);
}
int32_t gp_posterior_fit_cols_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                                  int32_t ncols, gp_post** out, void* alpha_out, void* logpdf_out) {
    return posterior_fit_cols_any(c, k, x, noise, mean, Y, ldy, ncols, out, alpha_out, logpdf_out);
}
int32_t gp_logpdf_grad_cols(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                            int32_t ncols, void* logpdf_out, double* dvar, double* dscale, void* dnoise, void* dY, void* dx) {
    return logpdf_grad_cols_any(c, k, x, noise, mean, Y, ldy, ncols, logpdf_out, dvar, dscale, dnoise, dY, dx, nullptr);
}
int32_t gp_logpdf_grad_cols_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                                int32_t ncols, void* logpdf_out, double* dtheta, void* dnoise, void* dY, void* dx) {
    return logpdf_grad_cols_any(c, k, x, noise, mean, Y, ldy, ncols, logpdf_out, nullptr, nullptr, dnoise, dY, dx, dtheta);
}

int32_t gp_logpdf_grad(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y,
                       void* logpdf_out, double* dvar, double* dscale, void* dnoise, void* dy, void* dx) {
    return logpdf_grad_any(c, k, x, noise, mean, y, logpdf_out, dvar, dscale, dnoise, dy, dx, nullptr, false);
}
int32_t gp_logpdf_grad_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y,
                           void* logpdf_out, double* dtheta, void* dnoise, void* dy) {
    return logpdf_grad_any(c, k, x, noise, mean, y, logpdf_out, nullptr, nullptr, dnoise, dy, nullptr, dtheta, false);
}

int32_t gp_logpdf_grad_sum_x(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y,
                             void* logpdf_out, double* dtheta, void* dnoise, void* dy, void* dx) {
    return logpdf_grad_any(c, k, x, noise, mean, y, logpdf_out, nullptr, nullptr, dnoise, dy, dx, dtheta, false);
}

int32_t gp_loo(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out, void* lp_out,
               void* mean_out, void* var_out) {
    return loo_any(c, k, x, noise, mean, y, value_out, lp_out, mean_out, var_out);
}
int32_t gp_loo_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out, void* lp_out,
                   void* mean_out, void* var_out) {
    return loo_any(c, k, x, noise, mean, y, value_out, lp_out, mean_out, var_out);
}
int32_t gp_loo_grad(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out,
                    double* dvar, double* dscale, void* dnoise, void* dy, void* dx) {
    return logpdf_grad_any(c, k, x, noise, mean, y, value_out, dvar, dscale, dnoise, dy, dx, nullptr, true);
}
int32_t gp_loo_grad_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* y, void* value_out,
                        double* dtheta, void* dnoise, void* dy, void* dx) {
    return logpdf_grad_any(c, k, x, noise, mean, y, value_out, nullptr, nullptr, dnoise, dy, dx, dtheta, true);
}

int32_t gp_logpdf_terms(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_noise* noise, const void* mean,
                        const void* Y, int64_t ldy, int32_t ncols, void* logdet_out, void* sqmahal_out) {
    return logpdf_terms_any(c, k, x, noise, mean, Y, ldy, ncols, logdet_out, sqmahal_out);
}
int32_t gp_logpdf_terms_sum(gp_ctx* c, const gp_ksum* k, const gp_points* x, const gp_noise* noise, const void* mean, const void* Y, int64_t ldy,
                            int32_t ncols, void* logdet_out, void* sqmahal_out) {
    return logpdf_terms_any(c, k, x, noise, mean, Y, ldy, ncols, logdet_out, sqmahal_out);
}

// ---- argument checks the exact and the sparse posterior share (argi: position of the first argument checked; the others follow it) ----
static int32_t check_test_points(const gp_points* xs, int d) {
    RC(check_points(xs, 2));
    if (xs->d != d) return set_arg_err(2, "xs has a different D than the training inputs");
    return 0;
}
static int32_t check_predict_out(int what, const void* mean_out, const void* var_out, const void* cov_out, int argi) {
    if (what <= 0 || what > 7) return set_arg_err(argi, "what must be a combination of 1|2|4");
    if ((what & 1) && !mean_out) return set_arg_err(argi + 1, "mean_out is NULL");
    if ((what & 2) && !var_out) return set_arg_err(argi + 2, "var_out is NULL");
    if ((what & 4) && !cov_out) return set_arg_err(argi + 3, "cov_out is NULL");
    return 0;
}
static int32_t check_joint_args(const gp_points* xs, int d, const gp_noise* noise) {
    RC(check_test_points(xs, d));
    return check_noise(noise, 4, true);
}
static int32_t check_heldout(const void* Y, int64_t ldy, int32_t ncols, const void* out, int64_t n, int argi) {
    if (!Y) return set_arg_err(argi, "Y is NULL");
    if (ldy < n) return set_arg_err(argi + 1, "ldy < n");
    if (ncols < 1) return set_arg_err(argi + 2, "ncols must be >= 1");
    if (!out) return set_arg_err(argi + 3, "out is NULL");
    return 0;
}
static int32_t check_draws(const void* xi, int32_t ncols, const void* out, int argi) {
    if (!xi) return set_arg_err(argi, "xi is NULL");
    if (ncols < 1) return set_arg_err(argi + 1, "ncols must be >= 1");
    if (!out) return set_arg_err(argi + 2, "out is NULL");
    return 0;
}

// What a handle of gp_posterior_fit_cols with more than one column cannot answer (one mean, one y): argument error on the handle, nothing written.
static int32_t cols_refused(const char* what) {
    return set_arg_err(1, (std::string(what) + ": the handle holds more than one column of observations (gp_posterior_fit_cols); its means come from "
                                               "gp_posterior_predict_cols").c_str());
}

// logdet(C) of a posterior's factor (C = cholesky(K + Σy), `post.data.C`): 2 Σ log L_ii kept from the fit.
int32_t gp_posterior_logdet(gp_post* post, double* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    if (!out) return set_arg_err(2, "out is NULL");
    *out = 2.0 * post->logdet_half;
    return 0;
}

int32_t gp_posterior_predict(gp_post* post, const gp_points* xs, const void* pm, int32_t what, void* mean_out,
                             void* var_out, void* cov_out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_test_points(xs, post->d));
    RC(check_predict_out(what, mean_out, var_out, cov_out, 4));
    if ((what & 1) && post->ncols > 1) return cols_refused("gp_posterior_predict (mean)");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if ((what & 6) && multi_can_solve(post) && (!(what & 4) || xs->n <= 4096)) {
        // multi-device fit whose factor still lives as block-cyclic pieces: variances and (up to 4 096 test points) the full
        // covariance come from a forward solve ON the pieces (multi.hip: multi_predict_var) — no gather; the mean needs α only
        if (what & 1) RC(predict_impl<double>(post, xs, pm, 1, mean_out, nullptr, nullptr, false));
        const gp_kernel k = post->kern.view(0);
        const long ns = xs->n;
        std::vector<double> xs_h;
        scale_points<double>(&k, xs, ns, xs_h);
        std::vector<double> sub((size_t)ns, 0.0), csub((what & 4) ? (size_t)ns * ns : 0, 0.0);
        RC(multi_predict_var(post, xs_h.data(), ns, ns, sub.data(), (what & 4) ? csub.data() : nullptr));
        if (what & 2)
            for (long i = 0; i < ns; ++i) ((double*)var_out)[i] = post->kern.variance - sub[i];  // k** = σ² for the stationary kernels of the path
        if (what & 4) {  // K** on the device (the ctx's own stream), minus X Xᵀ
            const long nsp = round_up(ns, 128), ldc = nsp + c->ldpad;
            std::vector<double> xsp((size_t)post->d * nsp, 0.0);
            for (int dd = 0; dd < post->d; ++dd) memcpy(&xsp[(size_t)dd * nsp], &xs_h[(size_t)dd * ns], sizeof(double) * (size_t)ns);
            DevBufs bufs(c);
            void *x_v = nullptr, *C_v = nullptr;
            RC(bufs.get(sizeof(double) * xsp.size(), &x_v));
            RC(bufs.get(sizeof(double) * (size_t)nsp * ldc, &C_v));
            HIPCHK(hipMemcpyAsync(x_v, xsp.data(), sizeof(double) * xsp.size(), hipMemcpyHostToDevice, c->sm));
            RC(gpmi::eng_kcross(c, c->sm, post->kern.kind, post->kern.variance, (const double*)x_v, nsp, ns, nsp, (const double*)x_v, nsp, ns, nsp, post->d,
                                (double*)C_v, ldc));
            double* co = (double*)cov_out;
            HIPCHK(hipMemcpy2DAsync(co, sizeof(double) * ns, C_v, sizeof(double) * ldc, sizeof(double) * ns, ns, hipMemcpyDeviceToHost, c->sm));
            HIPCHK(hipStreamSynchronize(c->sm));
            for (size_t i = 0; i < (size_t)ns * ns; ++i) co[i] -= csub[i];
        }
        return 0;
    }
    if (what & 6) RC(multi_gather(post));  // multi-device fit: the factor is assembled on this device on first need
    return by_dtype(post->dtype, [&](auto t) { return predict_impl<decltype(t)>(post, xs, pm, what, mean_out, var_out, cov_out, false); });
}

int32_t gp_posterior_ncols(gp_post* post, int32_t* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    if (!out) return set_arg_err(2, "out is NULL");
    *out = post->ncols;
    return 0;
}

int32_t gp_posterior_predict_cols(gp_post* post, const gp_points* xs, const void* pm, int32_t what, void* mean_out, void* var_out, void* cov_out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_test_points(xs, post->d));
    RC(check_predict_out(what, mean_out, var_out, cov_out, 4));
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if (what & 6) RC(multi_gather(post));  // (a one-column handle of a multi-device fit: the factor is assembled on this device on first need)
    return by_dtype(post->dtype, [&](auto t) { return predict_impl<decltype(t)>(post, xs, pm, what, mean_out, var_out, cov_out, true); });
}

// what: 1 mean side, 2 variance side; a side that is asked for needs its value or its gradient pointer (argi: position of `what`)
static int32_t check_predict_grad_out(int what, const void* mean_out, const void* var_out, const void* dmean_out, const void* dvar_out, int argi) {
    if (what <= 0 || what > 3) return set_arg_err(argi, "what must be a combination of 1|2");
    if ((what & 1) && !mean_out && !dmean_out) return set_arg_err(argi + 1, "mean_out and dmean_out are both NULL");
    if ((what & 2) && !var_out && !dvar_out) return set_arg_err(argi + 2, "var_out and dvar_out are both NULL");
    return 0;
}

int32_t gp_posterior_predict_grad(gp_post* post, const gp_points* xs, const void* pm, int32_t what, void* mean_out, void* var_out, void* dmean_out,
                                  void* dvar_out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_test_points(xs, post->d));
    RC(check_predict_grad_out(what, mean_out, var_out, dmean_out, dvar_out, 4));
    if ((what & 1) && post->ncols > 1) return cols_refused("gp_posterior_predict_grad (mean side)");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if (what & 2) RC(multi_gather(post));  // multi-device fit: the factor is assembled on this device (both solves run on the single-device path)
    return by_dtype(post->dtype, [&](auto t) { return predict_grad_impl<decltype(t)>(post, xs, pm, what, mean_out, var_out, dmean_out, dvar_out); });
}

int32_t gp_posterior_update(gp_post* old, const gp_points* x2, const gp_noise* noise2, const void* delta_all, gp_post** out,
                            void* alpha_out, void* logpdf_out) {
    Guard gd(old);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_points(x2, 2));
    if (x2->d != old->d) return set_arg_err(2, "x2 has a different D than the training inputs");
    RC(check_noise(noise2, 3, true));
    if (!delta_all) return set_arg_err(4, "delta_all is NULL");
    if (!out) return set_arg_err(5, "out is NULL");
    if (old->ncols > 1) return cols_refused("gp_posterior_update");
    *out = nullptr;
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if (old->dtype == 0 && multi_can_solve(old) && x2->n <= 4096 && !noise_dense(noise2)) {  // (a dense Σy2: gathered path, single-device engine)
        // multi-device posterior whose factor still lives as block-cyclic pieces: the factor is extended where it lives (multi.hip:
        // multi_update) — no gather; a failed forward / backward consistency check (-1991) falls back to the gathered path below
        auto p = std::make_unique<gp_post>();
        double lp = 0;
        const int32_t rc = multi_update(old, x2, noise2, delta_all, p.get(), alpha_out, &lp);
        if (rc == 0) {
            if (logpdf_out) *(double*)logpdf_out = lp;
            publish(c, p, out);
            return 0;
        }
        (void)hipSetDevice(c->device);
        if (rc != -1991) return rc;
    }
    RC(multi_gather(old));
    auto p = std::make_unique<gp_post>();
    double lp = 0;
    RC(by_dtype(old->dtype, [&](auto t) { return update_impl<decltype(t)>(old, x2, noise2, delta_all, p.get(), alpha_out, &lp); }));
    if (logpdf_out) put(logpdf_out, old->dtype, 0, lp);
    publish(c, p, out);
    return 0;
}

int32_t gp_posterior_factor_mul(gp_post* post, const void* xi, int32_t ncols, void* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    if (!xi) return set_arg_err(2, "xi is NULL");
    if (ncols < 1) return set_arg_err(3, "ncols must be >= 1");
    if (!out) return set_arg_err(4, "out is NULL");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if (post->dtype == 0 && multi_can_solve(post) && ncols <= 1024) return multi_factor_mul(post, (const double*)xi, ncols, (double*)out);  // on the pieces
    RC(multi_gather(post));
    return by_dtype(post->dtype, [&](auto t) { return factor_mul_impl<decltype(t)>(post, xi, ncols, out); });
}

int32_t gp_posterior_solve(gp_post* post, const void* B, int32_t ncols, void* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    if (!B) return set_arg_err(2, "B is NULL");
    if (ncols < 1) return set_arg_err(3, "ncols must be >= 1");
    if (!out) return set_arg_err(4, "out is NULL");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    if (post->dtype == 0 && multi_can_solve(post) && ncols <= 128) return multi_solve(post, (const double*)B, ncols, (double*)out);  // on the pieces
    RC(multi_gather(post));
    return by_dtype(post->dtype, [&](auto t) { return solve_impl<decltype(t)>(post, B, ncols, out); });
}

int64_t gp_posterior_n(gp_post* post) {
    Guard gd(post);
    if (!gd.ok) return -1;
    return post->n;
}

int32_t gp_posterior_get_factor(gp_post* post, void* U_out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    if (!U_out) return set_arg_err(2, "U_out is NULL");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    RC(multi_gather(post));
    const size_t es = post->dtype == 0 ? 8 : 4;
    const long n = post->n;
    // device row j (row-major lower L[j][0..j]) == host column j of the column-major upper U
    HIPCHK(hipMemcpy2DAsync(U_out, es * n, post->A, es * post->ld, es * n, n, hipMemcpyDeviceToHost, c->sm));
    HIPCHK(hipStreamSynchronize(c->sm));
    for (long j = 0; j < n; ++j) {  // strictly-lower part of U (i > j) is not part of the factor
        char* col = (char*)U_out + (size_t)j * n * es;
        if (j + 1 < n) memset(col + (size_t)(j + 1) * es, 0, (size_t)(n - j - 1) * es);
    }
    return 0;
}

int32_t gp_posterior_free(gp_post* post) {
    if (!post || !reg_take(post)) return set_arg_err(1, "not a live gp_post");
    gp_ctx* c = post->ctx;  // the handle holds a reference on its ctx: c is alive
    {
        std::lock_guard<std::mutex> l(c->mu);  // waits for any call still using the handle (Guard re-checks the registry under this lock)
        (void)hipSetDevice(c->device);
        multi_post_release(post);
        ctx_release(c, post->A, post->A_bytes);
        ctx_release(c, post->xs, post->xs_bytes);
        ctx_release(c, post->alpha, post->alpha_bytes);
        if (post->dibc.w) ctx_release(c, post->dibc.w, post->dibc.bytes);
        delete post;
    }
    ctx_unref(c);
    return 0;
}

// ---- VFE / DTC ---------------------------------------------------------------------------------------
// What a handle of gp_vfe_fit_cols with more than one column cannot answer (one α, one y): argument error on the handle, nothing written.
static int32_t vfe_cols_refused(const char* what) {
    return set_arg_err(1, (std::string(what) + ": the handle holds more than one column of observations (gp_vfe_fit_cols); use the gp_vfe_*_cols calls").c_str());
}

int32_t gp_vfe_fit(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_points* z, const gp_noise* noise,
                   double jitter, const void* mean, const void* y, int32_t approx, gp_vfe** out, void* objective_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk, false));
    RC(check_points(z, 4));
    if (z->d != x->d) return set_arg_err(4, "z has a different D than x");
    if (!(jitter >= 0)) return set_arg_err(6, "jitter must be >= 0");
    if (!y) return set_arg_err(8, "y is NULL");
    if (approx != 0 && approx != 1) return set_arg_err(9, "approx must be 0 (VFE) or 1 (DTC)");
    if (out) *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<gp_vfe> p(out ? new gp_vfe() : nullptr);  // out == NULL: the objective only, no handle
    if (p) p->ctx = c;
    double obj = 0;
    RC(by_dtype(k->dtype, [&](auto t) { return vfe_fit_impl<decltype(t)>(c, k, x, z, noise, jitter, mean, y, approx, p.get(), &obj, nullptr, VFE_FIT); }));
    if (objective_out) put(objective_out, k->dtype, 0, obj);
    if (p) publish(c, p, out);
    return 0;
}

int32_t gp_vfe_update(gp_vfe* old, const gp_points* x2, const gp_noise* noise2, const void* mean2, const void* y2, gp_vfe** out,
                      void* objective_out) {
    Guard gd(old);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (old->ncols > 1) return vfe_cols_refused("gp_vfe_update");
    RC(check_points(x2, 2));
    if (x2->d != old->d) return set_arg_err(2, "x2 has a different D than the training inputs");
    RC(check_noise(noise2, 3, false));
    if (!y2) return set_arg_err(5, "y2 is NULL");
    if (!out) return set_arg_err(6, "out is NULL");
    *out = nullptr;
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const gp_kernel k = old->kern.view(old->dtype);
    auto p = std::make_unique<gp_vfe>();
    p->ctx = c;
    double obj = 0;
    RC(by_dtype(old->dtype, [&](auto t) {
        return vfe_fit_impl<decltype(t)>(c, &k, x2, nullptr, noise2, 0.0, mean2, y2, old->approx, p.get(), &obj, old, VFE_UPDATE);
    }));
    if (objective_out) put(objective_out, old->dtype, 0, obj);
    publish(c, p, out);
    return 0;
}

int32_t gp_vfe_append(gp_vfe* old, const gp_points* z2, gp_vfe** out, void* objective_out) {
    Guard gd(old);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (old->ncols > 1) return vfe_cols_refused("gp_vfe_append");
    RC(check_points(z2, 2));
    if (z2->d != old->d) return set_arg_err(2, "z2 has a different D than the pseudo-points");
    if (!out) return set_arg_err(3, "out is NULL");
    *out = nullptr;
    if (old->segs.empty()) return set_arg_err(1, "gp_vfe holds no observations");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const gp_kernel k = old->kern.view(old->dtype);
    auto p = std::make_unique<gp_vfe>();
    p->ctx = c;
    double obj = 0;
    RC(by_dtype(old->dtype, [&](auto t) {
        return vfe_fit_impl<decltype(t)>(c, &k, nullptr, z2, nullptr, 0.0, nullptr, nullptr, old->approx, p.get(), &obj, old, VFE_APPEND);
    }));
    if (objective_out) put(objective_out, old->dtype, 0, obj);
    publish(c, p, out);
    return 0;
}

// ---- VFE / DTC for a matrix of observations (gp_vfe_fit_cols and its handle) -------------------------------
static void put_objectives(void* objective_out, int dtype, const std::vector<double>& obj) {
    if (objective_out)
        for (size_t i = 0; i < obj.size(); ++i) put(objective_out, dtype, i, obj[i]);
}

int32_t gp_vfe_fit_cols(gp_ctx* c, const gp_kernel* k, const gp_points* x, const gp_points* z, const gp_noise* noise, double jitter, const void* mean,
                        const void* Y, int64_t ldy, int32_t ncols, int32_t approx, gp_vfe** out, void* objective_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    ResolvedKernel rk;
    RC(check_fit_args(k, x, noise, rk, false));
    RC(check_points(z, 4));
    if (z->d != x->d) return set_arg_err(4, "z has a different D than x");
    if (!(jitter >= 0)) return set_arg_err(6, "jitter must be >= 0");
    if (!Y) return set_arg_err(8, "Y is NULL");
    if (ldy < x->n) return set_arg_err(9, "ldy < n");
    if (ncols < 1 || ncols > GPMI355_COLS_MAX) return set_arg_err(10, "ncols must be 1..GPMI355_COLS_MAX");
    if (approx != 0 && approx != 1) return set_arg_err(11, "approx must be 0 (VFE) or 1 (DTC)");
    if (out) *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<gp_vfe> p(out ? new gp_vfe() : nullptr);  // out == NULL: the objectives only, no handle
    if (p) p->ctx = c;
    std::vector<double> obj((size_t)ncols, 0.0);
    RC(by_dtype(k->dtype, [&](auto t) {
        return vfe_fit_impl<decltype(t)>(c, k, x, z, noise, jitter, mean, Y, approx, p.get(), obj.data(), nullptr, VFE_FIT, (long)ldy, ncols);
    }));
    put_objectives(objective_out, k->dtype, obj);
    if (p) publish(c, p, out);
    return 0;
}

int32_t gp_vfe_update_cols(gp_vfe* old, const gp_points* x2, const gp_noise* noise2, const void* mean2, const void* Y2, int64_t ldy2, gp_vfe** out,
                           void* objective_out) {
    Guard gd(old);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    RC(check_points(x2, 2));
    if (x2->d != old->d) return set_arg_err(2, "x2 has a different D than the training inputs");
    RC(check_noise(noise2, 3, false));
    if (!Y2) return set_arg_err(5, "Y2 is NULL");
    if (ldy2 < x2->n) return set_arg_err(6, "ldy2 < n2");
    if (!out) return set_arg_err(7, "out is NULL");
    *out = nullptr;
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const gp_kernel k = old->kern.view(old->dtype);
    auto p = std::make_unique<gp_vfe>();
    p->ctx = c;
    std::vector<double> obj((size_t)old->ncols, 0.0);
    RC(by_dtype(old->dtype, [&](auto t) {
        return vfe_fit_impl<decltype(t)>(c, &k, x2, nullptr, noise2, 0.0, mean2, Y2, old->approx, p.get(), obj.data(), old, VFE_UPDATE, (long)ldy2);
    }));
    put_objectives(objective_out, old->dtype, obj);
    publish(c, p, out);
    return 0;
}

int32_t gp_vfe_append_cols(gp_vfe* old, const gp_points* z2, gp_vfe** out, void* objective_out) {
    Guard gd(old);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    RC(check_points(z2, 2));
    if (z2->d != old->d) return set_arg_err(2, "z2 has a different D than the pseudo-points");
    if (!out) return set_arg_err(3, "out is NULL");
    *out = nullptr;
    if (old->segs.empty()) return set_arg_err(1, "gp_vfe holds no observations");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const gp_kernel k = old->kern.view(old->dtype);
    auto p = std::make_unique<gp_vfe>();
    p->ctx = c;
    std::vector<double> obj((size_t)old->ncols, 0.0);
    RC(by_dtype(old->dtype, [&](auto t) {
        return vfe_fit_impl<decltype(t)>(c, &k, nullptr, z2, nullptr, 0.0, nullptr, nullptr, old->approx, p.get(), obj.data(), old, VFE_APPEND);
    }));
    put_objectives(objective_out, old->dtype, obj);
    publish(c, p, out);
    return 0;
}

int32_t gp_vfe_ncols(gp_vfe* p, int32_t* out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (!out) return set_arg_err(2, "out is NULL");
    *out = p->ncols;
    return 0;
}

int32_t gp_vfe_predict_cols(gp_vfe* p, const gp_points* xs, const void* pm, int32_t what, void* mean_out, void* var_out, void* cov_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    RC(check_test_points(xs, p->d));
    RC(check_predict_out(what, mean_out, var_out, cov_out, 4));
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(p->dtype, [&](auto t) { return vfe_predict_cols_impl<decltype(t)>(p, xs, pm, what, mean_out, var_out, cov_out); });
}

int32_t gp_vfe_get_cols(gp_vfe* p, void* alpha_out, void* meps_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const long vst = (long)p->vrows * p->mp;
    std::vector<double> h((size_t)vst * 3);
    HIPCHK(hipMemcpy(h.data(), p->vec, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int col = 0; col < p->ncols; ++col)
        for (long i = 0; i < p->m; ++i) {
            if (alpha_out) put(alpha_out, p->dtype, (size_t)col * p->m + i, h[2 * vst + (long)col * p->mp + i]);
            if (meps_out) put(meps_out, p->dtype, (size_t)col * p->m + i, h[vst + (long)col * p->mp + i]);
        }
    return 0;
}

int32_t gp_vfe_get_by_cols(gp_vfe* p, void* B_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (!B_out) return set_arg_err(2, "B_out is NULL");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const size_t es = p->dtype == 0 ? 8 : 4;
    const size_t n_all = (size_t)p->n_obs;
    size_t off = 0;
    for (const auto& sg : p->segs) {  // one segment per fit / update, in arrival order; row s of a segment's b = column s
        if (sg->n > 0)
            HIPCHK(hipMemcpy2D((char*)B_out + off, es * n_all, sg->b, es * (size_t)sg->npad, es * (size_t)sg->n, (size_t)p->ncols, hipMemcpyDeviceToHost));
        off += es * (size_t)sg->n;
    }
    return 0;
}

int32_t gp_vfe_predict(gp_vfe* p, const gp_points* xs, const void* pm, int32_t what, void* mean_out, void* var_out, void* cov_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    RC(check_test_points(xs, p->d));
    RC(check_predict_out(what, mean_out, var_out, cov_out, 4));
    if ((what & 1) && p->ncols > 1) return vfe_cols_refused("gp_vfe_predict (mean)");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(p->dtype, [&](auto t) { return vfe_predict_impl<decltype(t)>(p, xs, pm, what, mean_out, var_out, cov_out); });
}

int32_t gp_vfe_predict_grad(gp_vfe* p, const gp_points* xs, const void* pm, int32_t what, void* mean_out, void* var_out, void* dmean_out, void* dvar_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if ((what & 1) && p->ncols > 1) return vfe_cols_refused("gp_vfe_predict_grad (mean side)");
    RC(check_test_points(xs, p->d));
    RC(check_predict_grad_out(what, mean_out, var_out, dmean_out, dvar_out, 4));
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(p->dtype, [&](auto t) { return vfe_predict_grad_impl<decltype(t)>(p, xs, pm, what, mean_out, var_out, dmean_out, dvar_out); });
}

int32_t gp_vfe_logpdf(gp_vfe* p, const gp_points* xs, const void* pm, const gp_noise* noise, const void* Y, int64_t ldy,
                      int32_t ncols, void* out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (p->ncols > 1) return vfe_cols_refused("gp_vfe_logpdf");
    RC(check_joint_args(xs, p->d, noise));
    RC(check_heldout(Y, ldy, ncols, out, xs->n, 5));
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    DevBufs bufs(c);
    Joint<double> J;
    const long R = round_up(ncols, 128);
    const int32_t rc = by_dtype(p->dtype, [&](auto t) -> int32_t {  // the M×M side and the joint are fp64 whatever the handle's dtype
        RC(vfe_joint<decltype(t)>(p, xs, pm, noise, R, bufs, J));
        return joint_logpdf<double, decltype(t)>(c, J, Y, ldy, ncols, out);
    });
    if (rc < 0) ctx_drain(c);  // (a positive status is a failed minor of the joint covariance, not an error)
    return rc;
}

int32_t gp_vfe_rand(gp_vfe* p, const gp_points* xs, const void* pm, const gp_noise* noise, const void* xi, int32_t ncols, void* out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (p->ncols > 1) return vfe_cols_refused("gp_vfe_rand");
    RC(check_joint_args(xs, p->d, noise));
    RC(check_draws(xi, ncols, out, 5));
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    DevBufs bufs(c);
    Joint<double> J;
    const int32_t rc = by_dtype(p->dtype, [&](auto t) -> int32_t {
        RC(vfe_joint<decltype(t)>(p, xs, pm, noise, 0, bufs, J));
        return joint_rand<double, decltype(t)>(c, J, bufs, xi, ncols, out);
    });
    if (rc < 0) ctx_drain(c);
    return rc;
}

int32_t gp_vfe_get(gp_vfe* p, void* alpha_out, void* meps_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (p->ncols > 1) return vfe_cols_refused("gp_vfe_get");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> h((size_t)p->mp * 3);
    HIPCHK(hipMemcpy(h.data(), p->vec, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (long i = 0; i < p->m; ++i) {
        if (alpha_out) put(alpha_out, p->dtype, i, h[2 * p->mp + i]);
        if (meps_out) put(meps_out, p->dtype, i, h[p->mp + i]);
    }
    return 0;
}

int32_t gp_vfe_get_factors(gp_vfe* p, void* U_out, void* LamU_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const long m = p->m;
    // device row j of the row-major lower factor == host column j of the column-major upper factor (always fp64 on the device)
    std::vector<double> h;
    const void* srcs[2] = {p->Lz, p->Ld};
    void* dsts[2] = {U_out, LamU_out};
    for (int which = 0; which < 2; ++which) {
        if (!dsts[which]) continue;
        if (!srcs[which]) return set_arg_err(1, "the posterior holds no factor (objective-only fit)");
        h.resize((size_t)m * (size_t)m);
        HIPCHK(hipMemcpy2DAsync(h.data(), sizeof(double) * m, srcs[which], sizeof(double) * p->ld, sizeof(double) * m, m,
                                hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        for (long j = 0; j < m; ++j)
            for (long i = 0; i < m; ++i) put(dsts[which], p->dtype, (size_t)j * m + i, i <= j ? h[(size_t)j * m + i] : 0.0);
    }
    return 0;
}

int64_t gp_vfe_n(gp_vfe* p) {
    Guard gd(p);
    if (!gd.ok) return -1;
    return p->n_obs;
}

int32_t gp_vfe_get_by(gp_vfe* p, void* by_out) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (p->ncols > 1) return vfe_cols_refused("gp_vfe_get_by");
    if (!by_out) return set_arg_err(2, "b_y_out is NULL");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const size_t es = p->dtype == 0 ? 8 : 4;
    size_t off = 0;
    for (const auto& sg : p->segs) {  // one segment per fit / update, in arrival order
        if (sg->n > 0) HIPCHK(hipMemcpy((char*)by_out + off, sg->b, es * (size_t)sg->n, hipMemcpyDeviceToHost));
        off += es * (size_t)sg->n;
    }
    return 0;
}

int32_t gp_vfe_grad(gp_vfe* p, double* dvariance, double* dscale, double* dnoise_sum, void* dnoise_diag, void* dy, double* dz, int32_t z_layout,
                    void* dx, int32_t x_layout) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (p->ncols > 1) return vfe_cols_refused("gp_vfe_grad");
    if (dz && p->dtype != 0)
        return set_arg_err(7, "pseudo-input gradients need an fp64 handle: the fp32-streamed B Bᵀ of an fp32 fit does not carry the cancellation between the K_zz and K_fz terms");
    if (dz && (z_layout < 0 || z_layout > 2 || (z_layout == 0 && p->d != 1))) return set_arg_err(8, "z_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)");
    if (dx && (x_layout < 0 || x_layout > 2 || (x_layout == 0 && p->d != 1))) return set_arg_err(10, "x_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(p->dtype, [&](auto t) { return vfe_grad_impl<decltype(t)>(p, dvariance, dscale, dnoise_sum, dnoise_diag, dy, dz, z_layout, dx, x_layout); });
}

int32_t gp_vfe_grad_cols(gp_vfe* p, double* dvariance, double* dscale, double* dnoise_sum, void* dnoise_diag, void* dY, double* dz, int32_t z_layout,
                         void* dx, int32_t x_layout) {
    Guard gd(p);
    if (!gd.ok) return set_arg_err(1, "not a live gp_vfe");
    if (dz && p->dtype != 0)
        return set_arg_err(7, "pseudo-input gradients need an fp64 handle: the fp32-streamed B Bᵀ of an fp32 fit does not carry the cancellation between the K_zz and K_fz terms");
    if (dz && (z_layout < 0 || z_layout > 2 || (z_layout == 0 && p->d != 1))) return set_arg_err(8, "z_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)");
    if (dx && (x_layout < 0 || x_layout > 2 || (x_layout == 0 && p->d != 1))) return set_arg_err(10, "x_layout must be 0 (vector, D = 1), 1 (ColVecs) or 2 (RowVecs)");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    return by_dtype(p->dtype, [&](auto t) { return vfe_grad_impl<decltype(t)>(p, dvariance, dscale, dnoise_sum, dnoise_diag, dY, dz, z_layout, dx, x_layout); });
}

int64_t gp_vfe_m(gp_vfe* p) {
    Guard gd(p);
    if (!gd.ok) return -1;
    return p->m;
}

int32_t gp_vfe_free(gp_vfe* p) {
    if (!p || !reg_take(p)) return set_arg_err(1, "not a live gp_vfe");
    gp_ctx* c = p->ctx;
    {
        std::lock_guard<std::mutex> l(c->mu);
        (void)hipSetDevice(c->device);
        vfe_release(p);
        delete p;
    }
    ctx_unref(c);
    return 0;
}

// ---- joint predictive logpdf / rand of an exact posterior --------------------------------------------------
int32_t gp_posterior_logpdf(gp_post* post, const gp_points* xs, const void* pm, const gp_noise* noise, const void* Y, int64_t ldy,
                            int32_t ncols, void* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_joint_args(xs, post->d, noise));
    RC(check_heldout(Y, ldy, ncols, out, xs->n, 5));
    if (post->ncols > 1) return cols_refused("gp_posterior_logpdf");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const bool dist = multi_can_solve(post) && xs->n <= 4096;  // held-out logpdf on the block-cyclic pieces: no gather
    if (!dist) RC(multi_gather(post));
    DevBufs bufs(c);
    const long R = round_up(ncols, 128);
    int32_t rc;
    if (post->dtype == 0) {
        Joint<double> J;
        rc = dist ? post_joint_dist(post, xs, pm, noise, R, bufs, J) : post_joint<double>(post, xs, pm, noise, R, bufs, J);
        if (rc == 0) rc = joint_logpdf<double, double>(c, J, Y, ldy, ncols, out);
    } else {
        Joint<float> J;
        rc = post_joint<float>(post, xs, pm, noise, R, bufs, J);
        if (rc == 0) rc = joint_logpdf<float, float>(c, J, Y, ldy, ncols, out);
    }
    if (rc < 0) ctx_drain(c);
    return rc;
}

int32_t gp_posterior_rand(gp_post* post, const gp_points* xs, const void* pm, const gp_noise* noise, const void* xi, int32_t ncols,
                          void* out) {
    Guard gd(post);
    if (!gd.ok) return set_arg_err(1, "not a live gp_post");
    RC(check_joint_args(xs, post->d, noise));
    RC(check_draws(xi, ncols, out, 5));
    if (post->ncols > 1) return cols_refused("gp_posterior_rand");
    gp_ctx* c = gd.c;
    HIPCHK(hipSetDevice(c->device));
    const bool dist = multi_can_solve(post) && xs->n <= 4096;  // posterior sampling on the block-cyclic pieces: no gather
    if (!dist) RC(multi_gather(post));
    DevBufs bufs(c);
    int32_t rc;
    if (post->dtype == 0) {
        Joint<double> J;
        rc = dist ? post_joint_dist(post, xs, pm, noise, 0, bufs, J) : post_joint<double>(post, xs, pm, noise, 0, bufs, J);
        if (rc == 0) rc = joint_rand<double, double>(c, J, bufs, xi, ncols, out);
    } else {
        Joint<float> J;
        rc = post_joint<float>(post, xs, pm, noise, 0, bufs, J);
        if (rc == 0) rc = joint_rand<float, float>(c, J, bufs, xi, ncols, out);
    }
    if (rc < 0) ctx_drain(c);
    return rc;
}

// ---- microbenchmarks / probes (tools/gpu_diag.py) ------------------------------------------------
int32_t gp_probe_mfma_f64(gp_ctx* c, const double* A_host, const double* B_host, double* D_host) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    double* buf;
    HIPCHK(hipMalloc((void**)&buf, sizeof(double) * (64 + 64 + 256)));
    HIPCHK(hipMemcpy(buf, A_host, sizeof(double) * 64, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(buf + 64, B_host, sizeof(double) * 64, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mfma_probe_f64_kernel, dim3(1), dim3(64), 0, c->sm, buf, buf + 64, buf + 128);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->sm));
    HIPCHK(hipMemcpy(D_host, buf + 128, sizeof(double) * 256, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(buf));
    return 0;
}
// the fp32 twin: D(16×16) = A(16×4)·B(4×16) through Tr<float> — the MFMA and the C/D row map every fp32 kernel uses
int32_t gp_probe_mfma_f32(gp_ctx* c, const float* A_host, const float* B_host, float* D_host) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    float* buf;
    HIPCHK(hipMalloc((void**)&buf, sizeof(float) * (64 + 64 + 256)));
    HIPCHK(hipMemcpy(buf, A_host, sizeof(float) * 64, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(buf + 64, B_host, sizeof(float) * 64, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mfma_probe_f32_kernel, dim3(1), dim3(64), 0, c->sm, buf, buf + 64, buf + 128);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->sm));
    HIPCHK(hipMemcpy(D_host, buf + 128, sizeof(float) * 256, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(buf));
    return 0;
}
// returns measured TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64 (all CUs, 2 blocks per CU)
int32_t gp_bench_mfma_f64(gp_ctx* c, int32_t iters, double* tflops_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    double* buf;
    HIPCHK(hipMalloc((void**)&buf, 64));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    const int blocks = prop.multiProcessorCount;  // one 1024-thread block per CU
    const size_t smem = 96 * 1024;
    HIPCHK(hipFuncSetAttribute((const void*)mfma_rate_f64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(mfma_rate_f64_kernel, dim3(blocks), dim3(1024), smem, c->sm, buf, 64);
    HIPCHK(hipEventRecord(a, c->sm));
    hipLaunchKernelGGL(mfma_rate_f64_kernel, dim3(blocks), dim3(1024), smem, c->sm, buf, iters);
    HIPCHK(hipEventRecord(b, c->sm));
    HIPCHK(hipStreamSynchronize(c->sm));
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double flops = (double)blocks * 16.0 * (double)iters * 4.0 * 2.0 * 16 * 16 * 4;
    *tflops_out = flops / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIPCHK(hipFree(buf));
    return 0;
}

// measured TFLOP/s of back-to-back fp32 MFMAs: variant 0 = v_mfma_f32_16x16x4_f32 (what the GEMM kernels issue), 1 = 32x32x2
int32_t gp_bench_mfma_f32(gp_ctx* c, int32_t variant, int32_t iters, double* tflops_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    float* buf;
    HIPCHK(hipMalloc((void**)&buf, 64));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    const int blocks = prop.multiProcessorCount;
    const size_t smem = 96 * 1024;
    auto run = [&](auto kern) -> int32_t {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(1024), smem, c->sm, buf, 64);
        HIPCHK(hipEventRecord(a, c->sm));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(1024), smem, c->sm, buf, iters);
        HIPCHK(hipEventRecord(b, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        return 0;
    };
    RC(variant == 0 ? run(mfma_rate_f32_kernel<0>) : run(mfma_rate_f32_kernel<1>));
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double per = variant == 0 ? 2.0 * 16 * 16 * 4 : 2.0 * 32 * 32 * 2;
    *tflops_out = (double)blocks * 16.0 * (double)iters * 4.0 * per / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    HIPCHK(hipFree(buf));
    return 0;
}

// ---- device-level building blocks (multi-process block-cyclic driver) ------------------------------
static GridMap to_map(const gp_grid* g, long row0, long col0) {
    GridMap m = plain_map(0, row0, col0);
    if (g) {
        m.lower = g->lower;
        m.P = g->P; m.p = g->p; m.Q = g->Q; m.q = g->q;
        m.nb = (long)g->tb * 128;
    }
    return m;
}

extern "C++" {
// Each building block with matrix / vector data of either dtype is ONE template (dev_*<T>) behind two extern "C" wrappers (gpd_X: fp64, gpd_X_f32).  The
// fp32 kernels move rows as 16-byte pieces = 4 floats where the fp64 ones move 2 doubles and step k by 32 instead of 16 (kernels.hpp BK): what the fp32
// instantiations need of their arguments is checked here (aligned4), what the fp64 entry points have always refused is unchanged.
template <typename T> static inline bool aligned4(const T* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

template <typename T>
static int32_t dev_assemble(gp_ctx* c, const gp_kernel* k, const T* x_dev, int64_t n_valid, int64_t n_pad, int32_t d, const T* noise_dev, const gp_grid* g,
                            T* a_loc, int64_t lda, int64_t m_loc, int64_t n_loc) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    RC(check_kernel(k, d, 2));
    if (m_loc % 128 || n_loc % 128) return set_arg_err(11, "m_loc, n_loc must be multiples of 128");
    if constexpr (sizeof(T) == 4) {  // the Gram kernel stores two columns (8 bytes) per lane
        if (((uintptr_t)a_loc & 7) != 0) return set_arg_err(9, "a_loc must be 8-byte aligned");
        if (lda % 2 != 0 || lda < n_loc) return set_arg_err(10, "lda must be even and >= n_loc");
    }
    HIPCHK(hipSetDevice(c->device));
    GridMap m = to_map(g, 0, 0);
    dim3 grid((unsigned)(n_loc / 128), (unsigned)(m_loc / 128));
    if (grid.x == 0 || grid.y == 0) return 0;
    launch_kmat<T>(grid, c->sm, a_loc, lda, x_dev, n_pad, x_dev, n_pad, d, k->kind, (T)k->variance, noise_dev, n_valid, n_valid, 1, m, (const T*)nullptr,
                   (const T*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

template <typename T>
static int32_t dev_potrf(gp_ctx* c, T* a, int64_t lda, int64_t m, int64_t n, int32_t* info_dev, int32_t col0, int64_t n_valid, double* logdet_dev) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (n % 64 || m % 64 || m < n) return set_arg_err(4, "m, n must be multiples of 64 with m >= n");
    // the leaf kernels (and, in fp64, the in-panel update kernel) move rows as 16-byte pieces (leaf.hpp ld4 / st4; kernels.hpp panel64 chunk_t)
    if (((uintptr_t)a & 15) != 0) return set_arg_err(2, "a must be 16-byte aligned");
    if constexpr (sizeof(T) == 8) {
        if (lda % 2 != 0 || lda < n) return set_arg_err(3, "lda must be even and >= n");
    } else {
        if (lda % 4 != 0 || lda < n) return set_arg_err(3, "lda must be a multiple of 4 and >= n");
    }
    HIPCHK(hipSetDevice(c->device));
    return potrf_rec<T>(c, c->sm, a, lda, 0, n, m, info_dev, col0, n_valid, logdet_dev);
}

template <typename T>
static int32_t dev_trsm(gp_ctx* c, T* x, int64_t ldx, int64_t m, const T* lmat, int64_t ldl, int64_t n) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (n % 64 || m % 64) return set_arg_err(4, "m, n must be multiples of 64");
    if constexpr (sizeof(T) == 4) {
        if (!aligned4(x, ldx)) return set_arg_err(2, "x must be 16-byte aligned and ldx a multiple of 4");
        if (!aligned4(lmat, ldl)) return set_arg_err(5, "l must be 16-byte aligned and ldl a multiple of 4");
    }
    if (m == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return trsm_rec<T>(c, c->sm, x, ldx, m, lmat, ldl, n);
}

template <typename T>
static int32_t dev_gemm_nt(gp_ctx* c, T* cm, int64_t ldc, const T* a, int64_t lda, const T* b, int64_t ldb, int64_t m, int64_t n, int64_t k, const gp_grid* g,
                           int64_t row0, int64_t col0) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if constexpr (sizeof(T) == 8) {
        if (m % 64 || n % 64 || k % 16) return set_arg_err(8, "m, n multiples of 64 and k multiple of 16 required");
    } else {
        if (m % 64 || n % 64 || k % 32) return set_arg_err(8, "m, n multiples of 64 and k multiple of 32 required");
        // operand rows travel to LDS as 16-byte pieces (global_load_lds_dwordx4); C is read and written element by element
        if (!aligned4(a, lda)) return set_arg_err(4, "a must be 16-byte aligned and lda a multiple of 4");
        if (!aligned4(b, ldb)) return set_arg_err(6, "b must be 16-byte aligned and ldb a multiple of 4");
    }
    HIPCHK(hipSetDevice(c->device));
    if constexpr (sizeof(T) == 8) {  // "strassen_min_rows": the same decomposition the factorisation's bulk update uses
        c->strassen_v = c->strassen_min_rows;
        const bool syrk = g && g->lower && g->P == 1 && g->Q == 1 && a == b && lda == ldb && row0 == col0 && m >= n;
        PlanTables tabs;  // the lower SYRK in the grouped form: one update, planned here
        if (syrk && group_applies(c, n, k, lda, a)) tabs.add(c, m, n, k, row0, ldc, a, lda);
        const size_t el = !tabs.upd.empty() ? tabs.ws_elems : (!g ? (strassen_shape(c, m, n, k) ? strassen_ws_elems(c, m, n, k) : 0) : (syrk ? syrk_split_ws_elems(c, n, k) : 0));
        if (el) {
            DevBufs bufs(c);
            void* p = nullptr;
            RC(bufs.get(sizeof(double) * el, &p));
            const StrassenWs ws{(double*)p, el};
            int32_t rc = 0;
            if (!tabs.upd.empty()) {
                rc = tabs.upload(c, c->sm, bufs, {cm}, ws.p);
                if (rc == 0) rc = run_grouped(c, c->sm, tabs, 0, ws.p);
            } else
                rc = syrk ? syrk_lower_split(c, c->sm, ws, cm, ldc, a, lda, m, n, k, row0) : gemm_nt_strassen(c, c->sm, ws, cm, ldc, a, lda, b, ldb, m, n, k);
            HIPCHK(hipStreamSynchronize(c->sm));  // the sum panels go back to the cache when this returns: nothing may still read them
            return rc;
        }
    }
    return launch_gemm<T>(c, c->sm, cm, ldc, a, lda, b, ldb, m, n, k, to_map(g, row0, col0));
}

template <typename T>
static int32_t dev_trsv(gp_ctx* c, const T* lmat, int64_t ldl, int64_t np, T* r, int64_t ldr, int32_t nrhs, int32_t forward) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (np % 128) return set_arg_err(4, "np must be a multiple of 128");
    if constexpr (sizeof(T) == 4) {  // the diagonal tiles are inverted from 16-byte row pieces (trtri_64)
        if (!aligned4(lmat, ldl)) return set_arg_err(2, "l must be 16-byte aligned and ldl a multiple of 4");
    }
    HIPCHK(hipSetDevice(c->device));
    return trsv<T>(c, c->sm, lmat, ldl, np, r, ldr, nrhs, forward != 0);
}

template <typename T>
static int32_t dev_gemv_t(gp_ctx* c, const T* lmat, int64_t ldl, int64_t nrows, int64_t ncols, const T* a, T* r) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (nrows <= 0 || ncols <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(gemv_t_kernel<T>, dim3((unsigned)((ncols + 255) / 256), (unsigned)((nrows + 63) / 64)), dim3(256),
                       0, c->sm, lmat, ldl, nrows, ncols, a, r);
    HIPCHK(hipGetLastError());
    return 0;
}

template <typename T>
static int32_t dev_rowsumsq(gp_ctx* c, const T* x, int64_t ldx, int64_t nrows, int64_t ncols, double* out_dev) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (nrows <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(rowsumsq_kernel<T>, dim3((unsigned)nrows), dim3(256), 0, c->sm, x, ldx, ncols, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the gradient contractions and the sparse path's N-long reductions on caller-supplied weights (include/gpmi355.h states each contract).  They launch through
// the functions production launches through — launch_kgrad / launch_kgradx (grad_contract), launch_vgrad (vfe_grad_impl), launch_ystats / launch_ystats_cols
// (vfe_fit_impl) — so the instance a shape gets here is the one it gets there.
template <typename T> static inline bool aligned16(const T* p) { return ((uintptr_t)p & 15) == 0; }
// The staged scales (a host vector and a cache block, both local to the call) must outlive their upload and every launch that reads them: the stream is drained on
// EVERY way out of the call, an early error return included (declared after them, so it runs first)
struct DrainOnExit {
    hipStream_t s;
    ~DrainOnExit() { (void)hipStreamSynchronize(s); }
};

// k (a single kind) or ksum (a composite kernel): exactly one is non-NULL.  The kind's scales are staged from k->scale; the stream is drained before the staging
// block goes back to the cache.
template <typename T>
static int32_t dev_grad_contract(gp_ctx* c, const gp_kernel* k, const gp_ksum* ksum, const T* ci, int64_t ld, const T* alpha, const T* x, int64_t n, int64_t np,
                                 int32_t d, double* g, T* dn, double* gx) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (d < 1) return set_arg_err(9, "d must be >= 1");
    KSum ks;
    gp_kernel kid{};
    if (ksum) RC(pack_ksum(ksum, d, 2, ks, kid));
    else RC(check_kernel(k, d, 2));
    const gp_kernel& kk = ksum ? kid : *k;
    if (kk.dtype != (sizeof(T) == 4 ? 1 : 0)) return set_arg_err(2, "kernel dtype does not match the entry point's element type");
    if (!ci || !aligned16(ci)) return set_arg_err(3, "ci must be non-NULL and 16-byte aligned");
    if (np < 128 || np % 128) return set_arg_err(8, "np must be a positive multiple of 128");
    if (n < 1 || n > np) return set_arg_err(7, "n must be in 1..np");
    if (ld < np) return set_arg_err(4, "ld must be >= np");
    if (!alpha) return set_arg_err(5, "alpha is NULL");
    if (!x) return set_arg_err(6, "x is NULL");
    if (!g) return set_arg_err(10, "g is NULL");
    if (!dn) return set_arg_err(11, "dn is NULL");
    HIPCHK(hipSetDevice(c->device));
    DevBufs bufs(c);
    DevScales sc;
    DrainOnExit drain{c->sm};
    RC(sc.stage(bufs, kk.nscale, kk.scale, c->sm));
    const ContractArgs<T> A{ci, ld, x, n, np, d, kk.kind, kk.variance, kk.nscale, sc.ptr(), ksum ? &ks : nullptr, alpha};
    RC(launch_kgrad<T>(c->sm, A, g, dn));
    if (gx) RC(launch_kgradx<T>(c->sm, A, gx, np));
    HIPCHK(hipStreamSynchronize(c->sm));  // the scales' block goes back to the cache when this returns
    return 0;
}

template <typename T>
static int32_t dev_vgrad(gp_ctx* c, const T* cm, int64_t ldc, int32_t explicit_w, const T* xr, int64_t ldxr, const T* xc, int64_t ldxc, int32_t d, const gp_kernel* k,
                         const T* rs, const T* bv, const double* nu, int64_t nr, int64_t nc, double* g, double* gz, int64_t ldgz, double zfac, double* rowq,
                         double* rowp, double* gx, int64_t ldgx) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (d < 1) return set_arg_err(9, "d must be >= 1");
    RC(check_kernel(k, d, 10));
    if (k->dtype != (sizeof(T) == 4 ? 1 : 0)) return set_arg_err(10, "kernel dtype does not match the entry point's element type");
    if (nr < 1 || nc < 1) return set_arg_err(14, "nr, nc must be >= 1");
    const long ncp = round_up(nc, 128), nrp = round_up(nr, 128);
    if (!cm || ((uintptr_t)cm & (2 * sizeof(T) - 1)) != 0) return set_arg_err(2, "cm must be non-NULL and aligned to two elements");
    if (ldc < ncp) return set_arg_err(3, "ldc must be >= nc rounded up to 128");
    if (explicit_w != 0 && explicit_w != 1) return set_arg_err(4, "explicit_w must be 0 or 1");
    if (!xr || ldxr < nrp) return set_arg_err(6, "xr is NULL or ldxr < nr rounded up to 128");
    if (!xc || ldxc < ncp) return set_arg_err(8, "xc is NULL or ldxc < nc rounded up to 128");
    if (!explicit_w && (!rs || !bv || !nu)) return set_arg_err(11, "rs, bv and nu are needed with explicit_w = 0");
    if (!g) return set_arg_err(16, "g is NULL");
    if (!gz || ldgz < nc) return set_arg_err(17, "gz is NULL or ldgz < nc");
    if ((rowq == nullptr) != (rowp == nullptr)) return set_arg_err(20, "rowq and rowp come together");
    if (gx && ldgx < nr) return set_arg_err(23, "ldgx < nr");
    HIPCHK(hipSetDevice(c->device));
    DevBufs bufs(c);
    DevScales sc;
    DrainOnExit drain{c->sm};
    RC(sc.stage(bufs, k->nscale, k->scale, c->sm));
    const dim3 grid((unsigned)(ncp / 128), (unsigned)(nrp / 128));
    if (gx)
        RC((launch_vgrad<T, true>(c->sm, grid, cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, k->kind, k->variance, k->nscale, sc.ptr(), rs, bv, nu, nr, nc, g, gz, ldgz,
                                  zfac, rowq, rowp, gx, ldgx)));
    else
        RC((launch_vgrad<T, false>(c->sm, grid, cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, k->kind, k->variance, k->nscale, sc.ptr(), rs, bv, nu, nr, nc, g, gz, ldgz,
                                   zfac, rowq, rowp, (double*)nullptr, 0L)));
    HIPCHK(hipStreamSynchronize(c->sm));  // the scales' block goes back to the cache when this returns
    return 0;
}

template <typename T>
static int32_t dev_ystats(gp_ctx* c, const T* y, int64_t ldy, int64_t ncols, const T* b, int64_t row_lo, int64_t nrows, double* cacc, double* rowss) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    constexpr int E = 16 / (int)sizeof(T);
    if (!y || !aligned16(y) || ldy % E != 0 || ldy < ncols) return set_arg_err(2, "y must be 16-byte aligned, ldy >= ncols with 16-byte rows");
    if (ncols < 1) return set_arg_err(4, "ncols must be >= 1");
    if (!b || !aligned16(b)) return set_arg_err(5, "b must be non-NULL and 16-byte aligned");
    if (row_lo < 0 || nrows < 0) return set_arg_err(6, "row_lo, nrows must be >= 0");
    if (!cacc || !rowss) return set_arg_err(8, "cacc / rowss is NULL");
    if (nrows == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return launch_ystats<T>(c->sm, y, ldy, ncols, b, row_lo, nrows, cacc, rowss);
}

template <typename T>
static int32_t dev_ystats_cols(gp_ctx* c, const T* y, int64_t ldy, int64_t ncols, const T* by, int64_t ldb, int32_t sb, int64_t row_lo, int64_t nrows, double* cacc,
                               int64_t ldc, double* rowss) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    constexpr int E = 16 / (int)sizeof(T);  // = Tr<T>::VEC: elements per 16-byte load
    if (!y || !aligned16(y) || ldy % E != 0 || ldy < ncols) return set_arg_err(2, "y must be 16-byte aligned, ldy >= ncols with 16-byte rows");
    if (ncols < 16 * E || ncols % (16 * E)) return set_arg_err(4, "ncols must be a positive multiple of 16 x (16 bytes / element size)");
    if (!by || !aligned16(by) || ldb % E != 0 || ldb < ncols) return set_arg_err(5, "by must be 16-byte aligned, ldb >= ncols with 16-byte rows");
    if (sb < 1 || sb > 8) return set_arg_err(7, "sb must be 1..8");
    if (row_lo < 0 || nrows < 0 || nrows % 16) return set_arg_err(9, "row_lo >= 0 and nrows a multiple of 16 required");
    if (!cacc || ldc < row_lo + nrows) return set_arg_err(10, "cacc is NULL or ldc < row_lo + nrows");
    if (!rowss) return set_arg_err(12, "rowss is NULL");
    if (nrows == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return launch_ystats_cols<T>(c->sm, y, ldy, ncols, by, ldb, sb, row_lo, nrows, cacc, ldc, rowss);
}
}  // extern "C++"

int32_t gpd_assemble(gp_ctx* c, const gp_kernel* k, const double* x_dev, int64_t n_valid, int64_t n_pad, int32_t d,
                     const double* noise_dev, const gp_grid* g, double* a_loc, int64_t lda, int64_t m_loc,
                     int64_t n_loc) {
    return dev_assemble<double>(c, k, x_dev, n_valid, n_pad, d, noise_dev, g, a_loc, lda, m_loc, n_loc);
}
int32_t gpd_assemble_f32(gp_ctx* c, const gp_kernel* k, const float* x_dev, int64_t n_valid, int64_t n_pad, int32_t d, const float* noise_dev,
                         const gp_grid* g, float* a_loc, int64_t lda, int64_t m_loc, int64_t n_loc) {
    return dev_assemble<float>(c, k, x_dev, n_valid, n_pad, d, noise_dev, g, a_loc, lda, m_loc, n_loc);
}

int32_t gpd_potrf(gp_ctx* c, double* a, int64_t lda, int64_t m, int64_t n, int32_t* info_dev, int32_t col0,
                  int64_t n_valid, double* logdet_dev) {
    return dev_potrf<double>(c, a, lda, m, n, info_dev, col0, n_valid, logdet_dev);
}
int32_t gpd_potrf_f32(gp_ctx* c, float* a, int64_t lda, int64_t m, int64_t n, int32_t* info_dev, int32_t col0, int64_t n_valid, double* logdet_dev) {
    return dev_potrf<float>(c, a, lda, m, n, info_dev, col0, n_valid, logdet_dev);
}

int32_t gpd_trsm(gp_ctx* c, double* x, int64_t ldx, int64_t m, const double* lmat, int64_t ldl, int64_t n) {
    return dev_trsm<double>(c, x, ldx, m, lmat, ldl, n);
}
int32_t gpd_trsm_f32(gp_ctx* c, float* x, int64_t ldx, int64_t m, const float* lmat, int64_t ldl, int64_t n) {
    return dev_trsm<float>(c, x, ldx, m, lmat, ldl, n);
}

int32_t gpd_inv_lower(gp_ctx* c, const double* lmat, int64_t ldl, int64_t nb, double* w, int64_t ldw, double* scratch1, double* scratch2) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (nb < 64 || nb % 64) return set_arg_err(4, "nb must be a multiple of 64");
    if (!lmat || !w || !scratch1) return set_arg_err(2, "l / w / scratch1 is NULL");
    HIPCHK(hipSetDevice(c->device));
    return gpmi::eng_inv_lower(c, c->sm, lmat, ldl, nb, w, ldw, scratch1, scratch2);
}
int32_t gpd_trsm_inv(gp_ctx* c, double* x, int64_t ldx, int64_t m, const double* w, int64_t ldw, int64_t nb, double* scratch, int64_t lds) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (nb % 64 || m % 64) return set_arg_err(3, "m, nb must be multiples of 64");
    if (m == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return gpmi::eng_trsm_inv(c, c->sm, x, ldx, m, w, ldw, nb, scratch, lds);
}

int32_t gpd_gemm_nt(gp_ctx* c, double* cm, int64_t ldc, const double* a, int64_t lda, const double* b, int64_t ldb,
                    int64_t m, int64_t n, int64_t k, const gp_grid* g, int64_t row0, int64_t col0) {
    return dev_gemm_nt<double>(c, cm, ldc, a, lda, b, ldb, m, n, k, g, row0, col0);
}
int32_t gpd_gemm_nt_f32(gp_ctx* c, float* cm, int64_t ldc, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t m, int64_t n, int64_t k,
                        const gp_grid* g, int64_t row0, int64_t col0) {
    return dev_gemm_nt<float>(c, cm, ldc, a, lda, b, ldb, m, n, k, g, row0, col0);
}

int32_t gpd_trsv(gp_ctx* c, const double* lmat, int64_t ldl, int64_t np, double* r, int64_t ldr, int32_t nrhs,
                 int32_t forward) {
    return dev_trsv<double>(c, lmat, ldl, np, r, ldr, nrhs, forward);
}
int32_t gpd_trsv_f32(gp_ctx* c, const float* lmat, int64_t ldl, int64_t np, float* r, int64_t ldr, int32_t nrhs, int32_t forward) {
    return dev_trsv<float>(c, lmat, ldl, np, r, ldr, nrhs, forward);
}

int32_t gpd_gemv_t(gp_ctx* c, const double* lmat, int64_t ldl, int64_t nrows, int64_t ncols, const double* a, double* r) {
    return dev_gemv_t<double>(c, lmat, ldl, nrows, ncols, a, r);
}
int32_t gpd_gemv_t_f32(gp_ctx* c, const float* lmat, int64_t ldl, int64_t nrows, int64_t ncols, const float* a, float* r) {
    return dev_gemv_t<float>(c, lmat, ldl, nrows, ncols, a, r);
}

int32_t gpd_rowsumsq(gp_ctx* c, const double* x, int64_t ldx, int64_t nrows, int64_t ncols, double* out_dev) {
    return dev_rowsumsq<double>(c, x, ldx, nrows, ncols, out_dev);
}
int32_t gpd_rowsumsq_f32(gp_ctx* c, const float* x, int64_t ldx, int64_t nrows, int64_t ncols, double* out_dev) {
    return dev_rowsumsq<float>(c, x, ldx, nrows, ncols, out_dev);
}

int32_t gpd_grad_contract(gp_ctx* c, const gp_kernel* k, const double* ci, int64_t ld, const double* alpha, const double* x, int64_t n, int64_t np, int32_t d,
                          double* g, double* dn, double* gx) {
    return dev_grad_contract<double>(c, k, nullptr, ci, ld, alpha, x, n, np, d, g, dn, gx);
}
int32_t gpd_grad_contract_f32(gp_ctx* c, const gp_kernel* k, const float* ci, int64_t ld, const float* alpha, const float* x, int64_t n, int64_t np, int32_t d,
                              double* g, float* dn, double* gx) {
    return dev_grad_contract<float>(c, k, nullptr, ci, ld, alpha, x, n, np, d, g, dn, gx);
}
int32_t gpd_grad_contract_sum(gp_ctx* c, const gp_ksum* k, const double* ci, int64_t ld, const double* alpha, const double* x, int64_t n, int64_t np, int32_t d,
                              double* g, double* dn, double* gx) {
    return dev_grad_contract<double>(c, nullptr, k, ci, ld, alpha, x, n, np, d, g, dn, gx);
}
int32_t gpd_grad_contract_sum_f32(gp_ctx* c, const gp_ksum* k, const float* ci, int64_t ld, const float* alpha, const float* x, int64_t n, int64_t np, int32_t d,
                                  double* g, float* dn, double* gx) {
    return dev_grad_contract<float>(c, nullptr, k, ci, ld, alpha, x, n, np, d, g, dn, gx);
}

int32_t gpd_vgrad(gp_ctx* c, const double* cm, int64_t ldc, int32_t explicit_w, const double* xr, int64_t ldxr, const double* xc, int64_t ldxc, int32_t d,
                  const gp_kernel* k, const double* rs, const double* bv, const double* nu, int64_t nr, int64_t nc, double* g, double* gz, int64_t ldgz, double zfac,
                  double* rowq, double* rowp, double* gx, int64_t ldgx) {
    return dev_vgrad<double>(c, cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, k, rs, bv, nu, nr, nc, g, gz, ldgz, zfac, rowq, rowp, gx, ldgx);
}
int32_t gpd_vgrad_f32(gp_ctx* c, const float* cm, int64_t ldc, int32_t explicit_w, const float* xr, int64_t ldxr, const float* xc, int64_t ldxc, int32_t d,
                      const gp_kernel* k, const float* rs, const float* bv, const double* nu, int64_t nr, int64_t nc, double* g, double* gz, int64_t ldgz, double zfac,
                      double* rowq, double* rowp, double* gx, int64_t ldgx) {
    return dev_vgrad<float>(c, cm, ldc, explicit_w, xr, ldxr, xc, ldxc, d, k, rs, bv, nu, nr, nc, g, gz, ldgz, zfac, rowq, rowp, gx, ldgx);
}

int32_t gpd_ystats(gp_ctx* c, const double* y, int64_t ldy, int64_t ncols, const double* b, int64_t row_lo, int64_t nrows, double* cacc, double* rowss) {
    return dev_ystats<double>(c, y, ldy, ncols, b, row_lo, nrows, cacc, rowss);
}
int32_t gpd_ystats_f32(gp_ctx* c, const float* y, int64_t ldy, int64_t ncols, const float* b, int64_t row_lo, int64_t nrows, double* cacc, double* rowss) {
    return dev_ystats<float>(c, y, ldy, ncols, b, row_lo, nrows, cacc, rowss);
}
int32_t gpd_ystats_cols(gp_ctx* c, const double* y, int64_t ldy, int64_t ncols, const double* by, int64_t ldb, int32_t sb, int64_t row_lo, int64_t nrows, double* cacc,
                        int64_t ldc, double* rowss) {
    return dev_ystats_cols<double>(c, y, ldy, ncols, by, ldb, sb, row_lo, nrows, cacc, ldc, rowss);
}
int32_t gpd_ystats_cols_f32(gp_ctx* c, const float* y, int64_t ldy, int64_t ncols, const float* by, int64_t ldb, int32_t sb, int64_t row_lo, int64_t nrows,
                            double* cacc, int64_t ldc, double* rowss) {
    return dev_ystats_cols<float>(c, y, ldy, ncols, by, ldb, sb, row_lo, nrows, cacc, ldc, rowss);
}

int32_t gpd_gemm_time(gp_ctx* c, double* ms_out, int64_t* launches_out) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->sm));
    double tot = 0;
    for (auto& r : c->gemm_recs) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        tot += ms;
    }
    if (ms_out) *ms_out = tot;
    if (launches_out) *launches_out = (int64_t)c->gemm_recs.size();
    c->gemm_recs.clear();
    c->ev_used = 0;
    return 0;
}

int32_t gpd_sync(gp_ctx* c) {
    Guard gd(c, false);  // no lock, as ever: the wait must not queue behind another thread's call on the ctx
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->sm));
    HIPCHK(hipStreamSynchronize(c->sp));
    return 0;
}

}  // extern "C"
