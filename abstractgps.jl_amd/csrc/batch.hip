// batch.hip — many small exact GPs in one call: gp_logpdf_batch / gp_logpdf_batch_sum, gp_predict_batch / gp_predict_batch_sum, gp_logpdf_grad_batch /
// gp_logpdf_grad_batch_sum, gp_predict_grad_batch / gp_predict_grad_batch_sum, gp_joint_batch / gp_joint_batch_sum (include/gpmi355.h) and the kernels behind them: the fit (batch_logpdf_kernel,
// below), the predictions at each problem's test points from the slices it leaves (batch_predict_kernel, further down), the gradient of logpdf from the same
// slices (batch_inv_kernel, batch_grad_kernel, batch_gsum_kernel, behind it; with the input gradient of gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x:
// batch_gradx_kernel, batch_gxsum_kernel) and the gradients of the predictions w.r.t. the test inputs from the strips the predict kernel leaves and the S of
// batch_inv_kernel (batch_pgrad_kernel), the joint predictive distribution from the same strips (batch_jcov_kernel, batch_jfact_kernel); last many small
// sparse GPs in one call (gp_vfe_batch: vfe_prelude_kernel, vfe_stream_kernel, vfe_final_kernel; gp_vfe_grad_batch: vfe_gmm_kernel, vfe_gstream_kernel,
// vfe_gfinish_kernel behind them; gp_vfe_predict_batch / gp_vfe_predict_grad_batch: vfe_pprep_kernel, vfe_predict_kernel; gp_vfe_joint_batch: the strip-writing
// variant of vfe_predict_kernel, vfe_jcov_kernel and batch_jfact_kernel; each described in front of its kernels).
//
// ONE workgroup owns ONE problem from its inputs to its scalar: it assembles the lower triangle of K + Σy into the problem's slice of a
// workspace (δ = y − m riding along as row np, as in the single path), factors it by a blocked right-looking Cholesky (64-column blocks:
// diagonal block in LDS, rows below by substitution in registers: rows_solve_b64; trailing update by v_mfma_f64_16x16x4_f64 on 32×32 wave tiles with
// register-resident operands: mfma_tile_k64), reads ‖L⁻¹δ‖² off the carried row and, when α is wanted, runs the backward sweep on the same slice.
// The tile operations the kernels share are defined once in front of the first kernel, the steps the host drivers share in front of the first driver.
// Workgroups never wait for one another (no flags, no tickets: blockIdx.x is the problem), every loop is bounded by the problem's size, no
// floating-point atomics are used and the schedule of a problem depends on that problem alone — its result is the same bits whatever
// batch it rides in.  The slice of a problem (its factor and the solved row) stays intact until the call ends.
//
// Problems the kernel does not take (fp32, a dense Σy, n > GPMI355_BATCH_MAX_N, D > 16) are answered inside the same call by the
// single path (gp_logpdf / gp_posterior_fit and their *_sum forms; for predictions gp_posterior_fit + gp_posterior_predict[_grad] + gp_posterior_free, for the
// joint with gp_posterior_logpdf / gp_posterior_rand in between); which
// path serves a problem depends on that problem alone.
#include "kfun.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

namespace gpmi {

enum {
    BT = 64,                    // block column of the in-workgroup Cholesky
    NT = 512,                   // threads per workgroup: eight waves, two per SIMD (one hides the other's memory latency)
    BTS = 65,                   // LDS row stride of the diagonal block (odd: column accesses are conflict-free)
    BATCH_KERNEL_MAX_N = 2048,  // what the kernel's LDS layout admits (the solved row of a problem lives in LDS during the backward sweep)
    BATCH_MAXD = 16,
    BATCH_WAVE_PROBLEMS = 2048,  // problems per launch at most
    TP = 128,                    // test points per workgroup of the predict kernel: eight 32×32 wave tiles per 64-column block, one per wave
    BATCH_PRED_TILES = 1024      // predict workgroups per launch at most: a wave with more tiles of test points runs several predict launches
};
static const size_t BATCH_WS_BYTES = (size_t)4 << 30;  // workspace per launch at most: a larger batch runs in waves
static const size_t BATCH_IN_BYTES = (size_t)3 << 28;  // packed input per wave at most, where a family counts it (WaveCost::in): with what every problem shares and the results it stays
                                                        // inside the page-locked staging of a ctx, so a wave's copies never take the pageable path
static const size_t JOINT_PIN_BYTES = (size_t)1 << 30;  // what the page-locked staging of a ctx takes (ctx_pinned): a wave of gp_joint_batch stays below it

// One problem of a wave, first thing in the packed input.  Offsets count doubles: *_off into the packed input (−1: absent), a_off into the
// workspace, alpha_off into the result buffer (−1: α not wanted).
struct BatchProb {
    long a_off, x_off, y_off, m_off, nz_off, ks_off, alpha_off;
    int n, np, ld, d, kind, nscale, slot, pad_;
    double variance, noise_s;
    double scale[BATCH_MAXD];
};
static_assert(sizeof(BatchProb) % 8 == 0, "descriptors are packed in front of double data");

// slice of a problem: rows [0, np) the matrix, row np the carried δ row, rows (np, np + 32) zero (the trailing update works on 32-row tiles)
__host__ __device__ static inline long batch_np(long n) { return (n + BT - 1) / BT * BT; }
__host__ __device__ static inline long batch_ld(long np) { return np + 16; }  // keeps power-of-two orders off one HBM channel
static inline long batch_slice(long n) { return (batch_np(n) + 32) * batch_ld(batch_np(n)); }

// ---- the tile operations the kernels below are made of: one definition each, inlined into every kernel that uses it ----------------------------------
// the inputs of point j of x (dimension-major [d][n]) in registers: zeros beyond d and beyond n
__device__ __forceinline__ void batch_load_point(const double* x, int n, int d, int j, double (&xj)[BATCH_MAXD]) {
#pragma unroll
    for (int p = 0; p < BATCH_MAXD; ++p) xj[p] = (p < d && j < n) ? x[(long)p * n + j] : 0.0;
}
// t = x_i − xj (point i of x, i < n; by scalar loads where i is wave-uniform)
__device__ __forceinline__ void batch_diff(const double* x, int n, int d, int i, const double (&xj)[BATCH_MAXD], double (&t)[BATCH_MAXD]) {
#pragma unroll
    for (int p = 0; p < BATCH_MAXD; ++p) t[p] = p < d ? x[(long)p * n + i] - xj[p] : 0.0;
}
// the kernel value of problem P at the difference vector t: the composite kernel behind the descriptor, or variance · κ(Σ_p (scale_p t_p)²)
template <bool SUM>
__device__ __forceinline__ double batch_kval(const double* in, const BatchProb* P, const double (&t)[BATCH_MAXD], int d) {
    if (SUM) return ksum_eval<double, BATCH_MAXD>(*reinterpret_cast<const KSum*>(in + P->ks_off), t, d);
    double d2 = 0.0;
#pragma unroll
    for (int p = 0; p < BATCH_MAXD; ++p) {
        const double u = (P->nscale == 0 ? 1.0 : P->scale[P->nscale == 1 ? 0 : p]) * t[p];
        d2 = fma(u, u, d2);
    }
    return P->variance * kappa<double>(P->kind, d2);
}

// The 2×2×4 fp64 accumulators of a 32×32 wave tile (v_mfma_f64_16x16x4_f64), from and to the tile of C whose corner is (i0, c0).
__device__ __forceinline__ void acc_zero(d4_t (&acc)[2][2]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) acc[h >> 1][h & 1] = 0.0;
}
__device__ __forceinline__ void acc_load(d4_t (&acc)[2][2], const double* C, int i0, int c0, long ld, int lane) {
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[h >> 1][h & 1][q] = C[(long)(i0 + 16 * (h >> 1) + Tr<double>::crow(lane, q)) * ld + c0 + 16 * (h & 1) + (lane & 15)];
}
__device__ __forceinline__ void acc_store(const d4_t (&acc)[2][2], double* C, int i0, int c0, long ld, int lane) {
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int q = 0; q < 4; ++q) C[(long)(i0 + 16 * (h >> 1) + Tr<double>::crow(lane, q)) * ld + c0 + 16 * (h & 1) + (lane & 15)] = acc[h >> 1][h & 1][q];
}
// The register-resident operands of one 64-wide k block of a wave tile: rows i0 … i0 + 31 of A and c0 … c0 + 31 of B, columns k0 … k0 + 63.  Lane l = (r = l & 15,
// g = l >> 4) holds 16 consecutive k of rows r and 16 + r of both operands (eight d2_t per half-row); MFMA step s multiplies the k-quadruple {16 g + s}: the sum
// over the block is complete after 16 steps, in a fixed order.  Row indices stay ints up to the product with ld, as the kernels always had them.
template <bool NEG_A>
__device__ __forceinline__ void tile_operands_k64(double (&a)[2][16], double (&b)[2][16], const double* A, int i0, const double* B, int c0, int k0, long ld, int lane) {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const d2_t* pa = reinterpret_cast<const d2_t*>(A + (long)(i0 + 16 * h + r) * ld + k0 + 16 * g);
        const d2_t* pb = reinterpret_cast<const d2_t*>(B + (long)(c0 + 16 * h + r) * ld + k0 + 16 * g);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const d2_t ta = pa[q], tb = pb[q];
            a[h][2 * q] = NEG_A ? -ta.x : ta.x;
            a[h][2 * q + 1] = NEG_A ? -ta.y : ta.y;
            b[h][2 * q] = tb.x;
            b[h][2 * q + 1] = tb.y;
        }
    }
}
__device__ __forceinline__ void tile_mfma_k64(d4_t (&acc)[2][2], const double (&a)[2][16], const double (&b)[2][16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
#pragma unroll
            for (int hj = 0; hj < 2; ++hj) acc[hi][hj] = Tr<double>::mfma(a[hi][s], b[hj][s], acc[hi][hj]);
}
// acc ±= A Bᵀ over one 64-wide k block: the operands, then the 16 steps
template <bool NEG_A>
__device__ __forceinline__ void mfma_tile_k64(d4_t (&acc)[2][2], const double* A, int i0, const double* B, int c0, int k0, long ld, int lane) {
    double a[2][16], b[2][16];
    tile_operands_k64<NEG_A>(a, b, A, i0, B, c0, k0, ld, lane);
    tile_mfma_k64(acc, a, b);
}

// X ← X L_bb⁻ᵀ for the rows row0 + tid, row0 + tid + NT, … < row0 + nrows of X, columns col0 … col0 + 63, one row per thread: its 64 entries in registers, the
// lower triangle of L_bb and 1 / L_jj in LDS.  Returns ss + Σ of the squares of the solved entries, in column order (unused, the chain is dropped).  The row
// loop is part of the helper: a helper for ONE row, the loop at the call sites, compiled to 256 VGPRs and 12.9 KB of scratch per lane (this form: none).
__device__ __forceinline__ double rows_solve_b64(double* X, long ld, int row0, int col0, int nrows, int tid, const double (*Ls)[BTS], const double* dinv, double ss) {
    for (int rr = tid; rr < nrows; rr += NT) {
        d2_t* row = reinterpret_cast<d2_t*>(X + (long)(row0 + rr) * ld + col0);
        double xv[BT];
#pragma unroll
        for (int q = 0; q < BT / 2; ++q) {
            const d2_t t = row[q];
            xv[2 * q] = t.x;
            xv[2 * q + 1] = t.y;
        }
#pragma unroll
        for (int j = 0; j < BT; ++j) {
            xv[j] *= dinv[j];
#pragma unroll
            for (int k2 = j + 1; k2 < BT; ++k2) {
                xv[k2] = fma(-xv[j], Ls[k2][j], xv[k2]);
                if ((k2 & 15) == 15) __builtin_amdgcn_sched_barrier(0);  // keeps the LDS reads of a step next to their fma: hoisted, they spill
            }
        }
#pragma unroll
        for (int q = 0; q < BT / 2; ++q) {
            d2_t t;
            t.x = xv[2 * q];
            t.y = xv[2 * q + 1];
            row[q] = t;
            ss = fma(t.x, t.x, ss);
            ss = fma(t.y, t.y, ss);
        }
    }
    return ss;
}

// V ← V L⁻ᵀ for a strip V of `rows` rows (at most NT; columns left of k_lo zero and never touched), left-looking by 64-column blocks:
// V[:, j0:j0+64] −= V[:, k_lo:j0] L[j0:j0+64, k_lo:j0]ᵀ on 32×32 wave tiles (the rows rounded up to 32), the k loop running inside the accumulators, then the
// diagonal block by rows_solve_b64, one row per thread.  sh holds L_bb [BT][BTS] and 1 / L_jj behind it.  Returns Σ_k V_{tid,k}² of the solved row tid.
__device__ __forceinline__ double strip_solve(double* V, const double* A, long ld, int k_lo, int nt, int rows, double* sh, int tid, int lane, int w) {
    double (*Ls)[BTS] = reinterpret_cast<double (*)[BTS]>(sh);
    double* dinv = sh + BT * BTS;
    double ss = 0.0;
    for (int kb = k_lo / BT; kb < nt; ++kb) {
        const int j0 = kb * BT;
        for (int tile = w; tile < (rows + 31) / 32 * 2 && j0 > k_lo; tile += 8) {
            const int i0 = 32 * (tile >> 1), c0 = j0 + 32 * (tile & 1);
            d4_t acc[2][2];
            acc_load(acc, V, i0, c0, ld, lane);
            for (int k0 = k_lo; k0 < j0; k0 += BT) mfma_tile_k64<true>(acc, V, i0, A, c0, k0, ld, lane);
            acc_store(acc, V, i0, c0, ld, lane);
        }
        // the diagonal block: its lower triangle in LDS (the rest of the tile is not the factor's)
        for (int e = tid; e < BT * BT; e += NT) {
            const int rr = e >> 6, cc = e & 63;
            Ls[rr][cc] = cc <= rr ? A[(long)(j0 + rr) * ld + j0 + cc] : 0.0;
        }
        __syncthreads();
        if (tid < BT) dinv[tid] = 1.0 / Ls[tid][tid];
        __syncthreads();
        ss = rows_solve_b64(V, ld, 0, j0, rows, tid, Ls, dinv, ss);
        __syncthreads();
    }
    return ss;
}

// S = L⁻ᵀ of the factor in the lower triangle of a slice (np rows and columns, identity padding), as a strip of np rows: strip_solve on the rows of the
// identity.  What the sparse kernels invert their two M×M factors by (L_z in vfe_prelude_kernel, the factor of Λ_ε in vfe_gmm_kernel and vfe_pprep_kernel).
__device__ __forceinline__ void strip_inverse_t(double* S, const double* A, long ld, int np, double* sh, int tid, int lane, int w) {
    for (int e = tid; e < np * np; e += NT) {
        const int i = e / np, cc = e - i * np;
        S[(long)i * ld + cc] = i == cc ? 1.0 : 0.0;
    }
    __syncthreads();
    (void)strip_solve(S, A, ld, 0, np / BT, np, sh, tid, lane, w);
}

// The blocked right-looking Cholesky of a slice in the batch_slice layout, by one workgroup of NT threads: 64-column blocks, the diagonal block in LDS, the rows
// below it (the carried row np included) by rows_solve_b64, the trailing update on 32×32 wave tiles dealt round-robin to the eight waves.  Ls, dinv and red
// are the workgroup's LDS ([BT][BTS], [BT], at least BT entries); logdet_half gains Σ log L_ii of the rows below n (thread 0 holds the sum).  Returns 0, or the
// order of the first leading minor that is not positive (the same value in every thread; the slice is then left half factored).
__device__ __forceinline__ int batch_chol(double* __restrict__ A, long ld, int n, int np, int tid, int lane, int w, double (*Ls)[BTS], double* dinv, double* red,
                                          double& logdet_half) {
    const int nt = np / BT;
    int failcol = 0;
    for (int kb = 0; kb < nt; ++kb) {
        const int j0 = kb * BT;
        for (int e = tid; e < BT * BT; e += NT) Ls[e >> 6][e & 63] = A[(long)(j0 + (e >> 6)) * ld + j0 + (e & 63)];
        __syncthreads();
        // diagonal block in LDS: column j stays unscaled until the block is done (the update multiplies by 1/√pivot on the fly: same roundings as a
        // stored scaled column, one barrier per step)
        for (int j = 0; j < BT; ++j) {
            const double p = Ls[j][j];
            if (!(p > 0.0)) {  // the same value in every thread
                failcol = j0 + j + 1;
                break;
            }
            const double rs = fast_rsqrt<double>(p);
            if (tid == 0) dinv[j] = rs;
            if (lane > j) {
                const double lc = Ls[lane][j] * rs;
                for (int i = w + 8 * ((j + 1 - w + 7) / 8); i < BT; i += 8)
                    if (i >= lane) Ls[i][lane] = fma(-(Ls[i][j] * rs), lc, Ls[i][lane]);
            }
            __syncthreads();
        }
        if (failcol) break;
        for (int e = tid; e < BT * BT; e += NT) {
            const int r = e >> 6, cc = e & 63;
            if (cc <= r) {
                const double v = Ls[r][cc] * dinv[cc];  // cc == r: pivot/√pivot = L_rr
                if (cc < r) Ls[r][cc] = v;
                A[(long)(j0 + r) * ld + j0 + cc] = v;
                if (cc == r) red[r] = (j0 + r < n) ? log(v) : 0.0;
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < BT; ++j) logdet_half += red[j];

        // rows below the block (the δ row np included): X ← X L⁻ᵀ, one row per thread in registers
        const int r_lo = j0 + BT;
        (void)rows_solve_b64(A, ld, r_lo, j0, np + 1 - r_lo, tid, Ls, dinv, 0.0);
        __syncthreads();

        // trailing update C −= P Pᵀ on 32×32 wave tiles (the lower triangle and the δ row's tiles), dealt round-robin to the eight waves
        const int ntr = (np + 32 - r_lo) / 32, ntc = (np - r_lo) / 32;
        int cnt = 0;
        for (int ti = 0; ti < ntr; ++ti)
            for (int tj = 0; tj <= ti && tj < ntc; ++tj) {
                if ((cnt++ & 7) != w) continue;
                const int i0 = r_lo + 32 * ti, c0 = r_lo + 32 * tj;
                double a[2][16], b[2][16];
                d4_t acc[2][2];
                tile_operands_k64<true>(a, b, A, i0, A, c0, j0, ld, lane);
                acc_load(acc, A, i0, c0, ld, lane);
                tile_mfma_k64(acc, a, b);
                acc_store(acc, A, i0, c0, ld, lane);
            }
        __syncthreads();
    }
    return failcol;
}

// zs ← L⁻ᵀ zs for the factor in the lower triangle of a slice (nt blocks of 64 columns), the vector in LDS: block after block from the last one, the diagonal
// block in LDS and solved by wave 0 (one lane per entry), then the entries left of it updated, one per thread.
__device__ __forceinline__ void back_sweep(const double* __restrict__ A, long ld, int nt, double* zs, double (*Ls)[BTS], int tid, int lane, int w) {
    for (int kb = nt - 1; kb >= 0; --kb) {
        const int j0 = kb * BT;
        for (int e = tid; e < BT * BT; e += NT) Ls[e >> 6][e & 63] = A[(long)(j0 + (e >> 6)) * ld + j0 + (e & 63)];
        __syncthreads();
        if (w == 0) {
            double v = zs[j0 + lane], out = 0.0;
#pragma unroll
            for (int j = BT - 1; j >= 0; --j) {
                const double aj = lane_bcast<double>(v, j) / Ls[j][j];
                if (lane == j) out = aj;
                if (lane < j) v = fma(-Ls[j][lane], aj, v);
            }
            zs[j0 + lane] = out;
        }
        __syncthreads();
        for (int cc = tid; cc < j0; cc += NT) {
            double s = zs[cc];
            for (int i = 0; i < BT; ++i) s = fma(-A[(long)(j0 + i) * ld + cc], zs[j0 + i], s);
            zs[cc] = s;
        }
        __syncthreads();
    }
}

template <bool SUM>
__global__ __launch_bounds__(NT) void batch_logpdf_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw) {
    __shared__ double Ls[BT][BTS];
    __shared__ double dinv[BT];
    __shared__ double red[NT];
    __shared__ double zs[BATCH_KERNEL_MAX_N];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);  // w in a scalar register: row inputs by scalar loads
    const int n = P.n, np = P.np, d = P.d;
    const long ld = P.ld;
    const int nt = np / BT;
    double* __restrict__ A = ws + P.a_off;
    const double* __restrict__ x = in + P.x_off;

    // ---- 1. lower triangle of K + Σy, 64×64 tiles (lane = column, the eight waves interleave the rows); identity padding
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
            const int j = tj * BT + lane;
            double xj[BATCH_MAXD];
            batch_load_point(x, n, d, j, xj);
            for (int rr = 0; rr < BT / 8; ++rr) {
                const int i = ti * BT + w + 8 * rr;  // wave-uniform
                double v;
                if (i >= n || j >= n) {
                    v = (i == j) ? 1.0 : 0.0;
                } else {
                    double t[BATCH_MAXD];
                    batch_diff(x, n, d, i, xj, t);
                    v = batch_kval<SUM>(in, &P, t, d);
                    if (i == j) v += P.nz_off >= 0 ? in[P.nz_off + i] : P.noise_s;
                }
                A[(long)i * ld + j] = v;
            }
        }
    {
        const double* y = in + P.y_off;
        for (int j = tid; j < np; j += NT) {
            A[(long)np * ld + j] = j < n ? y[j] - (P.m_off >= 0 ? in[P.m_off + j] : 0.0) : 0.0;
            for (int r = 1; r < 32; ++r) A[(long)(np + r) * ld + j] = 0.0;
        }
    }
    __syncthreads();

    // ---- 2. blocked right-looking Cholesky
    double logdet_half = 0.0;  // Σ log L_ii (thread 0)
    const int failcol = batch_chol(A, ld, n, np, tid, lane, w, Ls, dinv, red, logdet_half);

    double* alpha = P.alpha_off >= 0 ? res + P.alpha_off : nullptr;
    if (failcol) {  // per-problem failure is data: NaN and the first non-positive minor
        if (tid == 0) {
            res[P.slot] = __builtin_nan("");
            res[nw + P.slot] = (double)failcol;
        }
        if (alpha)
            for (int j = tid; j < n; j += NT) alpha[j] = __builtin_nan("");
        return;
    }

    // ---- 3. ‖L⁻¹δ‖² from the carried row (fixed order: strided partial sums, then a tree)
    {
        double s = 0.0;
        for (int j = tid; j < np; j += NT) {
            const double z = A[(long)np * ld + j];
            zs[j] = z;
            s = fma(z, z, s);
        }
        red[tid] = s;
        __syncthreads();
        for (int h = NT / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) {
            res[P.slot] = -0.5 * ((double)n * 1.8378770664093454835606594728112 + 2.0 * logdet_half + red[0]);
            res[nw + P.slot] = 0.0;
        }
    }
    if (!alpha) return;

    // ---- 4. α = L⁻ᵀ z: backward sweep, the solved row in LDS
    back_sweep(A, ld, nt, zs, Ls, tid, lane, w);
    for (int j = tid; j < n; j += NT) alpha[j] = zs[j];
}

// One tile of test points of one problem: the unit of work of batch_predict_kernel, in a table behind the data of the packed input.  Offsets count
// doubles: xs_off into the packed input (the problem's test points, dimension-major [d][ns]), strip_off into the workspace, mean_off / var_off into the
// result buffer (the problem's ns entries; −1: that side is not wanted).
struct BatchTile {
    long xs_off, strip_off, mean_off, var_off;
    int prob, ns, row0, rows;  // descriptor of the problem (position in the packed input), its test points, the tile's first one and how many it holds (1 … TP)
};
static_assert(sizeof(BatchTile) % 8 == 0, "the tile table is packed behind double data");

// Predictive mean and variance at the test points of a wave's problems, from the slices batch_logpdf_kernel left behind (launched behind it on the same
// stream).  ONE workgroup owns ONE tile of up to TP test points of one problem: the factor is read-only here, so a problem with many test points spreads
// over many workgroups and none of them waits for another.
//   1. cross-Gram rows K(x*_tile, x) into the workgroup's own strip (TP × ld, zeros in the padded columns and in the rows beyond the tile), the mean
//      Σ_i K*_ji α_i in the same pass: lane = training point, per-lane partial sums over the 64-column tiles in LDS, then a tree;
//   2. V ← V L⁻ᵀ by strip_solve from column 0: one test point per thread in the substitution;
//   3. var_j = k** − Σ_i V_ji², summed by the thread that owns the row, block after block.
// Every row's arithmetic touches no other row: a test point's results are the same bits wherever it sits.  A failed problem's tiles write NaN and never
// read the slice.  Only what this call wrote is read: the lower triangle of the slice rows [0, np), and of the strip the rows of the tile rounded up to 32.
template <bool SUM>
__global__ __launch_bounds__(NT) void batch_predict_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                           const BatchTile* __restrict__ tiles) {
    __shared__ double sh[TP * 64];  // step 1: the mean's partial sums [TP][64]; step 2: L_bb [BT][BTS] and 1 / L_jj behind it
    const BatchTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, d = P.d, ns = T.ns, rows = T.rows;
    const long ld = P.ld;
    const int nt = np / BT, rp = (rows + 31) / 32 * 32;  // the rows the MFMA tiles cover
    double* mean_o = T.mean_off >= 0 ? res + T.mean_off + T.row0 : nullptr;
    double* var_o = T.var_off >= 0 ? res + T.var_off + T.row0 : nullptr;
    if (res[nw + P.slot] != 0.0) {  // the fit failed: NaN, and the slice is not read
        if (tid < rows) {
            if (mean_o) mean_o[tid] = __builtin_nan("");
            if (var_o) var_o[tid] = __builtin_nan("");
        }
        return;
    }
    const double* __restrict__ A = ws + P.a_off;
    double* __restrict__ V = ws + T.strip_off;
    const double* __restrict__ x = in + P.x_off;
    const double* __restrict__ xs = in + T.xs_off + T.row0;
    const double* __restrict__ alpha = mean_o ? res + P.alpha_off : nullptr;

    // ---- 1. K(x*_tile, x): lane = training point, the eight waves interleave the test points
    for (int e = tid; e < rp * 64; e += NT) sh[e] = 0.0;
    __syncthreads();
    for (int tj = 0; tj < nt; ++tj) {
        const int j = tj * BT + lane;
        double xj[BATCH_MAXD];
        batch_load_point(x, n, d, j, xj);
        const double aj = (alpha && j < n) ? alpha[j] : 0.0;
        for (int rr = 0; rr < rp / 8; ++rr) {
            const int i = w + 8 * rr;  // wave-uniform
            double v = 0.0;
            if (i < rows && j < n) {
                double t[BATCH_MAXD];
                batch_diff(xs, ns, d, i, xj, t);
                v = batch_kval<SUM>(in, &P, t, d);
            }
            if (var_o) V[(long)i * ld + j] = v;
            if (alpha) sh[i * 64 + lane] = fma(v, aj, sh[i * 64 + lane]);
        }
    }
    __syncthreads();
    if (mean_o) {  // fixed order: the 64 partial sums of a row by a tree
        for (int h = 32; h > 0; h >>= 1) {
            for (int e = tid; e < rows * h; e += NT) {
                const int i = e / h, l = e - i * h;
                sh[i * 64 + l] += sh[i * 64 + l + h];
            }
            __syncthreads();
        }
        if (tid < rows) mean_o[tid] = sh[tid * 64];
        __syncthreads();
    }
    if (!var_o) return;

    // ---- 2. V ← V L⁻ᵀ; 3. Σ_i V_ji² by the thread that owns row j, block after block
    const double ss = strip_solve(V, A, ld, 0, nt, rows, sh, tid, lane, w);
    if (tid < rows) {
        double kss = P.variance;  // every κ(x, x) = 1: k** is the variance, Σ_t σ_t² for a composite kernel
        if (SUM) {
            const KSum& ks = *reinterpret_cast<const KSum*>(in + P.ks_off);
            kss = 0.0;
            for (int tt = 0; tt < ks.nterms; ++tt) kss += ks.th[ks.tv[tt]];
        }
        var_o[tid] = kss - ss;
    }
}

// ---- the gradient of logpdf: batch_inv_kernel, batch_grad_kernel, batch_gsum_kernel -----------------------------------------------------------------
// Launched behind batch_logpdf_kernel on the same stream, on the slices it left (L in the lower triangle of rows [0, np), α in the result buffer):
//   ∂logpdf/∂θ = ½ Σ_ij (α_i α_j − C⁻¹_ij) ∂C_ij/∂θ,   C⁻¹ = S Sᵀ with S = L⁻ᵀ (upper triangular).
// A problem spreads over many workgroups and launch boundaries are the only synchronisation: no flags, no tickets, no floating-point atomics; every sum
// runs in an order that the problem's size alone fixes, so a problem's gradient is the same bits alone, anywhere in any batch, and on repetition.
enum {
    GNT = 256,     // threads per workgroup of batch_grad_kernel: four waves, one 32×32 MFMA tile of the 64×64 tile each; the thread count ksum_grad's slots are sized for
    GRAD_NP = 16,  // θ entries of a composite kernel per pass over the tile (their per-thread sums live in LDS slots)
    GRAD_MAXG = 1 + KSum::MAXTH  // sums per problem at most: the noise sum, then the kernel's parameters
};

// What the gradient kernels know of a problem beyond its BatchProb; same position in its table as the descriptor in the packed input.  Offsets count doubles:
// s_off (the S strip, np rows of ld) and part_off (ntiles × ng per-tile sums) into the workspace, g_off (ng sums) and dn_off (n entries ½(α_i² − C⁻¹_ii) of a
// diagonal Σy; −1: scalar noise) into the result buffer.  The sums: [0] noise, then single-kind [1] variance, [2 + p] scale_p; composite [1 + q] θ_q.
struct GradProb {
    long s_off, part_off, g_off, dn_off;
    int ng, ntiles;
};
static_assert(sizeof(GradProb) % 8 == 0, "the tables are packed behind double data");
// One workgroup's work: tile ti of 128 rows of S (batch_inv_kernel), or the 64×64 tile (ti >= tj) of the lower triangle (batch_grad_kernel; idx = its place
// among the problem's tiles, ti (ti + 1) / 2 + tj)
struct GradTile {
    int prob, ti, tj, idx;
};
static_assert(sizeof(GradTile) % 8 == 0, "the tables are packed behind double data");

// Rows [r0, r0 + 128) of S = L⁻ᵀ into the problem's strip: strip_solve from column r0 with V = the identity rows of the tile.  S is upper triangular: the
// columns left of r0 are zero, never written and never read (the k loops start at r0; batch_grad_kernel reads row i from column 64·⌊i / 64⌋ ≥ r0 on).
// A failed problem's tiles return at once: nothing of it is read or written here.
__global__ __launch_bounds__(NT) void batch_inv_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                       const GradProb* __restrict__ gps, const GradTile* __restrict__ tiles) {
    __shared__ double sh[BT * BTS + BT];  // L_bb [BT][BTS] and 1 / L_jj behind it
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const GradProb& G = gps[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = P.np, r0 = T.ti * TP;
    const long ld = P.ld;
    const int nt = np / BT, rows = np - r0 < TP ? np - r0 : TP;  // 64 or 128
    const double* __restrict__ A = ws + P.a_off;
    double* __restrict__ V = ws + G.s_off + (long)r0 * ld;
    {
        const int wc = np - r0;
        for (int e = tid; e < rows * wc; e += NT) {
            const int i = e / wc, cc = e - i * wc;
            V[(long)i * ld + r0 + cc] = i == cc ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    (void)strip_solve(V, A, ld, r0, nt, rows, sh, tid, lane, w);
}

// What the leave-one-out kernels know of a problem beyond its BatchProb and GradProb; same position in its table as the descriptor.  Offsets count doubles:
// lpart_off (one partial Σ ℓ_i per 128-row tile), z_off (the Z strip, np rows of ld), d_off and e_off (d_i = √(2 a_i) and e_i = b_i / d_i, np entries each,
// zero from n on) into the workspace; lp_off / mean_off / var_off (n entries each) and beta_off (β, np entries) into the result buffer.  −1: not wanted
// (z_off, d_off, e_off and beta_off are all wanted, or none is: the value calls need none of them).
struct LooProb {
    long lpart_off, z_off, d_off, e_off, lp_off, mean_off, var_off, beta_off;
};
static_assert(sizeof(LooProb) % 8 == 0, "the tables are packed behind double data");

// The 64×64 tile (ti >= tj) of the lower triangle of one problem:
//   1. C⁻¹_tile = Σ_{k ≥ 64 ti} S[i, k] S[j, k] by mfma_tile_k64 straight from the strip, one 32×32 wave tile per wave; the weights
//      W_ij = (α_i α_j − C⁻¹_ij)·(i = j ? ½ : 1) of the pairs j ≤ i < n into LDS;
//   2. Σ W_ij ∂C_ij/∂θ with ∂C_ij/∂θ re-evaluated from the packed inputs: thread = (column j = lane, rows w, w + 4, …), the column's inputs in registers, the
//      row's by scalar loads.  Single-kind: variance and scales in registers (the sums of kgrad_kernel, the 1 / scale factor of ∂r² at the end); composite:
//      ksum_grad, GRAD_NP θ entries per pass in per-thread LDS slots.  The diagonal adds W_ii to the noise sum; a diagonal Σy's entries are stored directly.
//   3. the per-thread sums by a butterfly per wave, the four waves added in order, stored as this tile's ng sums (batch_gsum_kernel adds the tiles).
// A failed problem's tiles return at once (batch_gsum_kernel writes its NaN): neither slice nor strip is read.
// LOO: the gradient of the leave-one-out objective (gp_loo_grad_batch) from the same steps 2 and 3.  Step 1 reads the Z strip batch_loo_z_kernel left and the β
// of batch_loo_beta_kernel: the tile is Σ over ALL k of Z[i, k] Z[j, k] (Z is a full matrix), W_ij = (β_i α_j + α_i β_j − (Z Zᵀ)_ij)·(i = j ? ½ : 1) = 2 G_ij
// resp. G_ii: Σ W ∂C/∂θ over the lower triangle is ⟨G, ∂C/∂θ⟩, the noise sum tr G, a diagonal Σy's entries G_ii.
template <bool SUM, bool LOO>
__global__ __launch_bounds__(GNT) void batch_grad_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                        const GradProb* __restrict__ gps, const GradTile* __restrict__ tiles, const LooProb* __restrict__ lps) {
    __shared__ double Wt[BT][BT];
    __shared__ double acc[SUM ? GRAD_NP : 1][GNT];
    __shared__ double kf[SUM ? KSum::MAXFT : 1][GNT];
    __shared__ double red[4][2 + BATCH_MAXD];
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const GradProb& G = gps[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, d = P.d;
    const long ld = P.ld;
    const int it0 = T.ti * BT, jt0 = T.tj * BT;
    const double* __restrict__ S = ws + (LOO ? lps[T.prob].z_off : G.s_off);  // LOO: the Z strip
    const double* __restrict__ alpha = res + P.alpha_off;
    const double* __restrict__ beta = LOO ? res + lps[T.prob].beta_off : nullptr;
    const double* __restrict__ x = in + P.x_off;
    double* __restrict__ part = ws + G.part_off + (long)T.idx * G.ng;

    // ---- 1. the weights of the tile
    {
        const int wi = w >> 1, wj = w & 1;
        if (!(T.ti == T.tj && wj > wi)) {  // the wave tile strictly above the diagonal holds no pair j <= i
            const int r = lane & 15;
            const int i0 = it0 + 32 * wi, c0 = jt0 + 32 * wj;
            d4_t c4[2][2];
            acc_zero(c4);
            for (int k0 = LOO ? 0 : it0; k0 < np; k0 += BT) mfma_tile_k64<false>(c4, S, i0, S, c0, k0, ld, lane);
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj) {
                    const int gj = c0 + 16 * hj + r;
                    const double aj = gj < n ? alpha[gj] : 0.0;
                    const double bj = (LOO && gj < n) ? beta[gj] : 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int gi = i0 + 16 * hi + Tr<double>::crow(lane, q);
                        double wv = 0.0;
                        if (gi < n && gj <= gi) {
                            if (LOO) wv = (fma(beta[gi], aj, alpha[gi] * bj) - c4[hi][hj][q]) * (gi == gj ? 0.5 : 1.0);
                            else wv = (alpha[gi] * aj - c4[hi][hj][q]) * (gi == gj ? 0.5 : 1.0);
                        }
                        Wt[gi - it0][gj - jt0] = wv;
                    }
                }
        }
    }
    __syncthreads();

    // ---- 2. the contraction
    const int gj = jt0 + lane;
    double xj[BATCH_MAXD];
    batch_load_point(x, n, d, gj, xj);
    double gn = 0.0;  // Σ W_ii
    if (T.ti == T.tj) {
        const int gi = it0 + tid;
        if (tid < BT && gi < n) {
            gn = Wt[tid][tid];
            if (G.dn_off >= 0) res[G.dn_off + gi] = gn;
        }
    }
    if (!SUM) {
        double gv = 0.0, gs[BATCH_MAXD];
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) gs[p] = 0.0;
        const int nscale = P.nscale;
        for (int rr = 0; rr < BT / 4; ++rr) {
            const int li = w + 4 * rr, gi = it0 + li;  // wave-uniform
            if (gi >= n) continue;
            if (gj > gi) continue;  // gj <= gi < n
            const double wgt = Wt[li][lane];
            double u2[BATCH_MAXD], d2 = 0.0;
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p) {
                const double t = p < d ? x[(long)p * n + gi] - xj[p] : 0.0;
                const double u = (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * t;
                u2[p] = u * u;
                d2 = fma(u, u, d2);
            }
            double kap, dk;
            kappa_and_dr2<double>(P.kind, d2, kap, dk);
            gv = fma(wgt, kap, gv);
            const double wk = wgt * P.variance * dk * 2.0;
            if (nscale == 1) {
                gs[0] = fma(wk, d2, gs[0]);
            } else if (nscale > 1) {
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) gs[p] = fma(wk, u2[p], gs[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < 2 + BATCH_MAXD; ++p) {
            double v = p == 0 ? gn : (p == 1 ? gv : gs[p >= 2 ? p - 2 : 0]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) red[w][p] = v;
        }
        __syncthreads();
        if (tid < G.ng) {
            double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            if (tid >= 2) v /= P.scale[tid - 2];  // the 1 / s (1 / v_p) factor of ∂r²
            part[tid] = v;
        }
    } else {
        const KSum& ks = *reinterpret_cast<const KSum*>(in + P.ks_off);
        const int nth = ks.nth;
        for (int p0 = 0; p0 < nth; p0 += GRAD_NP) {
#pragma unroll
            for (int p = 0; p < GRAD_NP; ++p) acc[p][tid] = 0.0;
            auto add = [&](int idx, double v) {
                const unsigned q = (unsigned)(idx - p0);
                if (q < (unsigned)GRAD_NP) acc[q][tid] += v;
            };
#pragma unroll 1
            for (int rr = 0; rr < BT / 4; ++rr) {
                const int li = w + 4 * rr, gi = it0 + li;  // wave-uniform
                if (gi >= n) continue;
                if (gj > gi) continue;  // gj <= gi < n
                double t[BATCH_MAXD];
                batch_diff(x, n, d, gi, xj, t);
                ksum_grad<double, BATCH_MAXD>(ks, t, d, Wt[li][lane], add, kf, tid);
            }
            if (p0 == 0) {
                double v = gn;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red[w][GRAD_NP] = v;
            }
#pragma unroll
            for (int p = 0; p < GRAD_NP; ++p) {
                double v = acc[p][tid];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) red[w][p] = v;
            }
            __syncthreads();
            if (tid < GRAD_NP && p0 + tid < nth) part[1 + p0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            if (tid == GRAD_NP && p0 == 0) part[0] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            __syncthreads();
        }
    }
}

// The ng sums of every problem of a wave: one workgroup per problem adds its tiles in index order (thread = entry).  A failed problem gets NaN in every sum
// and in the entries of a diagonal Σy's gradient; nothing of its workspace is read.
__global__ __launch_bounds__(128) void batch_gsum_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                        const GradProb* __restrict__ gps) {
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[blockIdx.x];
    const GradProb& G = gps[blockIdx.x];
    const int tid = threadIdx.x;
    if (res[nw + P.slot] != 0.0) {
        if (tid < G.ng) res[G.g_off + tid] = __builtin_nan("");
        if (G.dn_off >= 0)
            for (int i = tid; i < P.n; i += 128) res[G.dn_off + i] = __builtin_nan("");
        return;
    }
    if (tid >= G.ng) return;
    const double* __restrict__ part = ws + G.part_off;
    double s = 0.0;
    for (int t = 0; t < G.ntiles; ++t) s += part[(long)t * G.ng + tid];
    res[G.g_off + tid] = s;
}

// ---- leave-one-out cross-validation: batch_loo_kernel, batch_loo_sum_kernel; for its gradient batch_loo_z_kernel, batch_loo_beta_kernel ---------------------
// Launched behind batch_logpdf_kernel and batch_inv_kernel on the same stream, on the α and the S strips they left.  With C⁻¹ = S Sᵀ, c_i = [C⁻¹]_ii = Σ_{k ≥ i} S_ik²:
//   μ_i = y_i − α_i / c_i,  v_i = 1 / c_i,  ℓ_i = −½ log 2π + ½ log c_i − ½ α_i² / c_i,  L = Σ ℓ_i;   a_i = ½(1/c_i + α_i²/c_i²),  b_i = α_i / c_i,  β = C⁻¹ b,
//   dL = ⟨G, dC⟩ with 2G = β αᵀ + α βᵀ − Z Zᵀ,  Z = C⁻¹ diag(d),  d_i = √(2 a_i)   (batch_grad_kernel<SUM, true> contracts it).
// Padding (n ≤ k < np): d_k = e_k = β_k = 0, so column k of Z is zero; the rows of S and C⁻¹ beyond n are those of the identity: nothing leaks either way.
// As everywhere in this unit: launch boundaries are the only synchronisation, one writer per entry, every sum in an order the problem's size alone fixes.

// 128 rows of one problem (the tile table of batch_inv_kernel): one wave per row at a time (rows w, w + 8, … of the tile), the lanes stride the row of S from
// the first column of the row's 64-block on (left of it the strip is not written), 64 partial sums of squares joined by a butterfly.  Lane 0 writes the row's
// terms; thread 0 adds the ℓ_i of the tile in row order into the tile's partial sum.  A failed problem's tiles return at once.
__global__ __launch_bounds__(NT) void batch_loo_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                       const GradProb* __restrict__ gps, const LooProb* __restrict__ lps, const GradTile* __restrict__ tiles) {
    __shared__ double ls[TP];
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const LooProb& Q = lps[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, r0 = T.ti * TP;
    const long ld = P.ld;
    const int rows = np - r0 < TP ? np - r0 : TP;  // 64 or 128
    const double* __restrict__ S = ws + gps[T.prob].s_off;
    const double* __restrict__ alpha = res + P.alpha_off;
    const double* __restrict__ y = in + P.y_off;
    for (int li = w; li < rows; li += 8) {
        const int i = r0 + li;  // wave-uniform
        double s = 0.0;
        if (i < n)
            for (int k = (i & ~(BT - 1)) + lane; k < np; k += 64) {
                const double t = S[(long)i * ld + k];
                s = fma(t, t, s);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) {
            double lp = 0.0, dv = 0.0, ev = 0.0;
            if (i < n) {
                const double c = s, al = alpha[i], v = 1.0 / c, bi = al * v;
                lp = -0.91893853320467274178032973640562 + 0.5 * log(c) - 0.5 * al * bi;
                if (Q.lp_off >= 0) res[Q.lp_off + i] = lp;
                if (Q.mean_off >= 0) res[Q.mean_off + i] = y[i] - bi;
                if (Q.var_off >= 0) res[Q.var_off + i] = v;
                dv = sqrt(fma(bi, bi, v));  // √(2 a_i), a_i = ½(v + b_i²)
                ev = bi / dv;
            }
            ls[li] = lp;
            if (Q.d_off >= 0) {
                ws[Q.d_off + i] = dv;
                ws[Q.e_off + i] = ev;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int li = 0; li < rows; ++li) s += ls[li];
        ws[Q.lpart_off + T.ti] = s;
    }
}

// L of every problem of a wave: one workgroup per problem, thread 0 adds the tiles' partial sums in tile order and stores L in place of the logpdf.  A failed
// problem gets NaN in L, in the three per-point outputs and in β; nothing of its workspace is read.
__global__ __launch_bounds__(128) void batch_loo_sum_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                           const LooProb* __restrict__ lps) {
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[blockIdx.x];
    const LooProb& Q = lps[blockIdx.x];
    const int tid = threadIdx.x;
    if (res[nw + P.slot] != 0.0) {
        const double nan = __builtin_nan("");
        if (tid == 0) res[P.slot] = nan;
        for (int i = tid; i < P.n; i += 128) {
            if (Q.lp_off >= 0) res[Q.lp_off + i] = nan;
            if (Q.mean_off >= 0) res[Q.mean_off + i] = nan;
            if (Q.var_off >= 0) res[Q.var_off + i] = nan;
            if (Q.beta_off >= 0) res[Q.beta_off + i] = nan;
        }
        return;
    }
    if (tid != 0) return;
    double s = 0.0;
    for (int t = 0; t < (P.np + TP - 1) / TP; ++t) s += ws[Q.lpart_off + t];
    res[P.slot] = s;
}

// The 64×64 tile (ti, tk) of the FULL square of Z = C⁻¹ diag(d) of one problem: C⁻¹_tile = Σ_{m ≥ 64·max(ti, tk)} S[i, m] S[k, m] by mfma_tile_k64 straight from
// the S strip, one 32×32 wave tile per wave (step 1 of batch_gradx_kernel), times d_k, into the Z strip: every entry of the np × np square is written, by one
// thread.  A failed problem's tiles return at once.
__global__ __launch_bounds__(GNT) void batch_loo_z_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                         const GradProb* __restrict__ gps, const LooProb* __restrict__ lps, const GradTile* __restrict__ tiles) {
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const LooProb& Q = lps[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = P.np;
    const long ld = P.ld;
    const int it0 = T.ti * BT, kt0 = T.tj * BT;
    const double* __restrict__ S = ws + gps[T.prob].s_off;
    const double* __restrict__ dv = ws + Q.d_off;
    double* __restrict__ Z = ws + Q.z_off;
    const int r = lane & 15;
    const int i0 = it0 + 32 * (w >> 1), c0 = kt0 + 32 * (w & 1);
    d4_t c4[2][2];
    acc_zero(c4);
    for (int k0 = T.ti > T.tj ? it0 : kt0; k0 < np; k0 += BT) mfma_tile_k64<false>(c4, S, i0, S, c0, k0, ld, lane);
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj) {
            const int gk = c0 + 16 * hj + r;
            const double dk = dv[gk];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = i0 + 16 * hi + Tr<double>::crow(lane, q);
                Z[(long)gi * ld + gk] = c4[hi][hj][q] * dk;
            }
        }
}

// β = C⁻¹ b of 128 rows of one problem (the tile table of batch_inv_kernel) from the Z strip: β_i = Σ_k Z_ik e_k with e_k = b_k / d_k (d_k > 0 below n, e_k = 0
// from n on), one wave per row at a time, the lanes stride the row, a butterfly joins them.  The rows from n on get 0.  A failed problem's tiles return at once.
__global__ __launch_bounds__(NT) void batch_loo_beta_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                            const LooProb* __restrict__ lps, const GradTile* __restrict__ tiles) {
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const LooProb& Q = lps[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, r0 = T.ti * TP;
    const long ld = P.ld;
    const int rows = np - r0 < TP ? np - r0 : TP;
    const double* __restrict__ Z = ws + Q.z_off;
    const double* __restrict__ ev = ws + Q.e_off;
    for (int li = w; li < rows; li += 8) {
        const int i = r0 + li;  // wave-uniform
        double s = 0.0;
        if (i < n)
            for (int k = lane; k < np; k += 64) s = fma(Z[(long)i * ld + k], ev[k], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) res[Q.beta_off + i] = s;
    }
}

// ---- the gradient of logpdf w.r.t. the inputs: batch_gradx_kernel, batch_gxsum_kernel ---------------------------------------------------------------------
// Launched behind batch_grad_kernel, for the problems of a gradient wave whose dx is wanted, on the S strips and the α the wave already holds:
//   ∂logpdf/∂x_ip = Σ_{j ≠ i} (α_i α_j − C⁻¹_ij) ∂k/∂t_p (t = x_i − x_j)    (both orders of the symmetric pair folded in; the diagonal contributes nothing).
// What the two kernels know of a problem beyond its BatchProb and GradProb; same position in its table as the descriptor.  Offsets count doubles: xpart_off
// (nt² tables of [d][64] row sums, tile (ti, tj) at ti · nt + tj) into the workspace, dx_off (the gradient, dimension-major [d][n]) into the result buffer.
struct GradXProb {
    long xpart_off, dx_off;
};
static_assert(sizeof(GradXProb) % 8 == 0, "the tables are packed behind double data");

// The 64×64 tile (ti, tj) of the FULL square of one problem (idx = ti · nt + tj), as kgradx_kernel of the single path walks it:
//   1. C⁻¹_tile = Σ_{k ≥ 64 max(ti, tj)} S[i, k] S[j, k] by mfma_tile_k64 straight from the strip, one 32×32 wave tile per wave (row i of the strip is valid from
//      column 64·⌊i / 64⌋ on, S is upper triangular: nothing left of max(ti, tj) contributes); the weights α_i α_j − C⁻¹_ij into LDS, zero where i >= n, j >= n or i = j;
//   2. the contraction: lane = column j with its inputs in registers, the rows w, w + 4, … of the tile with the row's inputs by scalar loads; every (row, p) is
//      summed over the 64 columns by a butterfly.  Single kind: the sums run over W κ'(r²) u_p with u = s ∘ t, ∂k/∂t_p = 2 σ² s_p κ' u_p applied at the end
//      (kappa_and_dr2: Matern12 at distance 0 is 0); composite: ksum_gradx with its per-thread LDS slots.
//   3. lane 0 of the row's wave stores the d sums of the row into this tile's table: one writer per entry, rows beyond n store 0.
// A failed problem's tiles return at once (batch_gxsum_kernel writes its NaN): neither strip nor α is read.
template <bool SUM>
__global__ __launch_bounds__(GNT) void batch_gradx_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                         const GradProb* __restrict__ gps, const GradXProb* __restrict__ gxs,
                                                         const GradTile* __restrict__ tiles) {
    __shared__ double Wt[BT][BT];
    __shared__ double kf[SUM ? KSum::MAXFT : 1][GNT];
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, d = P.d;
    const long ld = P.ld;
    const int it0 = T.ti * BT, jt0 = T.tj * BT;
    const double* __restrict__ S = ws + gps[T.prob].s_off;
    const double* __restrict__ alpha = res + P.alpha_off;
    const double* __restrict__ x = in + P.x_off;
    double* __restrict__ part = ws + gxs[T.prob].xpart_off + (long)T.idx * (BT * d);

    // ---- 1. the weights of the tile
    {
        const int r = lane & 15;
        const int i0 = it0 + 32 * (w >> 1), c0 = jt0 + 32 * (w & 1);
        d4_t c4[2][2];
        acc_zero(c4);
        for (int k0 = T.ti > T.tj ? it0 : jt0; k0 < np; k0 += BT) mfma_tile_k64<false>(c4, S, i0, S, c0, k0, ld, lane);
#pragma unroll
        for (int hi = 0; hi < 2; ++hi)
#pragma unroll
            for (int hj = 0; hj < 2; ++hj) {
                const int gj = c0 + 16 * hj + r;
                const double aj = gj < n ? alpha[gj] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gi = i0 + 16 * hi + Tr<double>::crow(lane, q);
                    double wv = 0.0;
                    if (gi < n && gj < n && gi != gj) wv = alpha[gi] * aj - c4[hi][hj][q];
                    Wt[gi - it0][gj - jt0] = wv;
                }
            }
    }
    __syncthreads();

    // ---- 2. the contraction, 3. the row sums
    double xj[BATCH_MAXD];
    batch_load_point(x, n, d, jt0 + lane, xj);
#pragma unroll 1
    for (int rr = 0; rr < BT / 4; ++rr) {
        const int li = w + 4 * rr, gi = it0 + li;  // wave-uniform
        double g[BATCH_MAXD];
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) g[p] = 0.0;
        if (gi < n) {
            const double wgt = Wt[li][lane];
            double t[BATCH_MAXD];
            batch_diff(x, n, d, gi, xj, t);
            if (SUM) {
                ksum_gradx<double, BATCH_MAXD>(*reinterpret_cast<const KSum*>(in + P.ks_off), t, d, wgt, g, kf, tid);
            } else {
                double d2 = 0.0;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) {
                    t[p] *= P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p];  // u = s ∘ t
                    d2 = fma(t[p], t[p], d2);
                }
                double kap, dk;
                kappa_and_dr2<double>(P.kind, d2, kap, dk);
                const double wk = wgt * dk;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) g[p] = wk * t[p];
            }
        }
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) {
            if (p >= d) break;  // d is the problem's: the same in every lane
            double v = g[p];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) {
                const double sp = SUM ? 1.0 : 2.0 * P.variance * (P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p]);
                part[p * BT + li] = sp * v;
            }
        }
    }
}

// One 64-row block of the input gradient of one problem: the nt tables of tile row ti added in tj order (thread = row, the dimensions one after the other),
// written dimension-major [d][n] into the result buffer.  A failed problem gets NaN; nothing of its workspace is read.
__global__ __launch_bounds__(BT) void batch_gxsum_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                        const GradXProb* __restrict__ gxs, const GradTile* __restrict__ tiles) {
    const GradTile& T = tiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const GradXProb& X = gxs[T.prob];
    const int n = P.n, d = P.d, nt = P.np / BT, gi = T.ti * BT + (int)threadIdx.x;
    if (gi >= n) return;
    double* __restrict__ out = res + X.dx_off;
    if (res[nw + P.slot] != 0.0) {
        for (int p = 0; p < d; ++p) out[(long)p * n + gi] = __builtin_nan("");
        return;
    }
    const double* __restrict__ part = ws + X.xpart_off + (long)T.ti * nt * (BT * d) + threadIdx.x;
    for (int p = 0; p < d; ++p) {
        double s = 0.0;
        for (int tj = 0; tj < nt; ++tj) s += part[(long)tj * (BT * d) + p * BT];
        out[(long)p * n + gi] = s;
    }
}

// ---- the gradients of the predictions w.r.t. the test inputs: batch_pgrad_kernel --------------------------------------------------------------------
// What batch_pgrad_kernel knows of a tile beyond its BatchTile; same position in its table as the tile in the tile table.  Offsets count doubles: s_off
// (the S strip of the problem, as GradProb's) into the workspace, dmean_off / dvar_off into the result buffer (the problem's gradients, dimension-major
// [d][ns]; −1: that side's gradient is not wanted).
struct PGradTile {
    long s_off, dmean_off, dvar_off;
};
static_assert(sizeof(PGradTile) % 8 == 0, "the tables are packed behind double data");

// Launched directly behind the batch_predict_kernel launch of the same tiles (the strips of a wave are shared by its launch groups), ONE workgroup per tile:
//   dmean[j, p] = Σ_i α_i ∂k(x*_j, x_i)/∂x*_p,   dvar[j, p] = −2 Σ_i W[j, i] ∂k(x*_j, x_i)/∂x*_p,   W = V Sᵀ  (w_j = C⁻¹ k_j = L⁻ᵀ (L⁻¹ k_j)).
//   1. (variance side) W[i, c] = Σ_{k ≥ c} V[i, k] S[c, k] IN PLACE on the strip the predict kernel left (V = K* L⁻ᵀ, rows of the tile rounded up to 32), by
//      64-column blocks j0 ascending, one 32×32 wave tile per wave, k0 = j0 … np − 64: S's row c is written from column 128⌊c / 128⌋ <= j0 on and zero left
//      of c, so only what batch_inv_kernel wrote is read.  The two column tiles of a block read each other's columns of V: every wave finishes its
//      accumulators, barrier, store, barrier; later blocks read only k >= their own j0.  Padded columns give W = 0 and the contraction runs over i < n.
//   2. the contraction, ∂k re-evaluated from the packed inputs: one wave per test point (w, w + waves, …), lanes striding over the training points, fp64 sums per
//      lane and dimension, a butterfly per wave, lane 0 writes.  Single kind: 2 s_p² σ² κ'(r²)(x*_p − x_p) (kappa_and_dr2); composite: ksum_gradx.
// No atomics, no waits between workgroups, every sum in an order the problem's size fixes: a test point's gradient is the same bits alone, among other test
// points, in any batch and on repetition.  Mean side alone: no strip, no S, no product.  A failed problem's tiles write NaN and read neither slice nor strip.
// Threads: NT (eight waves, one wave tile each) for a single kind; PGNT_SUM (four waves, two wave tiles each) for a composite kernel, whose element body
// with both sides' sums over 16 dimensions does not fit the 256 registers a lane of an eight-wave workgroup has (it spilled to scratch).  Each wave tile and
// each test point is summed by one wave in the same order either way.
enum { PGNT_SUM = 256 };
template <bool SUM>
__global__ __launch_bounds__(SUM ? PGNT_SUM : NT) void batch_pgrad_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res,
                                                                         int nw, const BatchTile* __restrict__ tiles,
                                                                         const PGradTile* __restrict__ ptiles) {
    constexpr int NTH = SUM ? PGNT_SUM : NT, NWV = NTH / 64, TPW = 8 / NWV;  // threads, waves, wave tiles per wave and 64-column block
    __shared__ double kf[SUM ? KSum::MAXFT : 1][NTH];
    const BatchTile& T = tiles[blockIdx.x];
    const PGradTile& G = ptiles[blockIdx.x];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[T.prob];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, np = P.np, d = P.d, ns = T.ns, rows = T.rows;
    const long ld = P.ld;
    double* dmean_o = G.dmean_off >= 0 ? res + G.dmean_off + T.row0 : nullptr;
    double* dvar_o = G.dvar_off >= 0 ? res + G.dvar_off + T.row0 : nullptr;
    if (res[nw + P.slot] != 0.0) {  // the fit failed: NaN, and neither slice nor strip is read
        for (int e = tid; e < rows * d; e += NTH) {
            const int p = e / rows, i = e - p * rows;
            if (dmean_o) dmean_o[(long)p * ns + i] = __builtin_nan("");
            if (dvar_o) dvar_o[(long)p * ns + i] = __builtin_nan("");
        }
        return;
    }
    double* __restrict__ V = ws + T.strip_off;
    const double* __restrict__ x = in + P.x_off;
    const double* __restrict__ xs = in + T.xs_off + T.row0;
    const double* __restrict__ alpha = dmean_o ? res + P.alpha_off : nullptr;

    // ---- 1. W = V Sᵀ in place
    if (dvar_o) {
        const double* __restrict__ S = ws + G.s_off;
        const int ntile = (rows + 31) / 32 * 2;  // wave tiles per 64-column block: at most eight
        for (int j0 = 0; j0 < np; j0 += BT) {
            d4_t acc[TPW][2][2];
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                const int tile = w + NWV * q;  // wave-uniform
                acc_zero(acc[q]);
                if (tile < ntile)
                    for (int k0 = j0; k0 < np; k0 += BT) mfma_tile_k64<false>(acc[q], V, 32 * (tile >> 1), S, j0 + 32 * (tile & 1), k0, ld, lane);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < TPW; ++q) {
                const int tile = w + NWV * q;
                if (tile < ntile) acc_store(acc[q], V, 32 * (tile >> 1), j0 + 32 * (tile & 1), ld, lane);
            }
            __syncthreads();
        }
    }

    // ---- 2. the contraction
    for (int i = w; i < rows; i += NWV) {  // wave-uniform
        double xv[BATCH_MAXD], am[BATCH_MAXD], av[BATCH_MAXD];
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) {
            xv[p] = p < d ? xs[(long)p * ns + i] : 0.0;
            am[p] = av[p] = 0.0;
        }
        const double* __restrict__ wrow = V + (long)i * ld;
        for (int j = lane; j < n; j += 64) {
            const double cm = alpha ? alpha[j] : 0.0;
            const double cv = dvar_o ? wrow[j] : 0.0;
            double t[BATCH_MAXD];
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p) t[p] = p < d ? xv[p] - x[(long)p * n + j] : 0.0;
            if (SUM) {
                double g[BATCH_MAXD];
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) g[p] = 0.0;
                ksum_gradx<double, BATCH_MAXD>(*reinterpret_cast<const KSum*>(in + P.ks_off), t, d, 1.0, g, kf, tid);
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) {
                    am[p] = fma(cm, g[p], am[p]);
                    av[p] = fma(cv, g[p], av[p]);
                }
            } else {
                double u[BATCH_MAXD], d2 = 0.0;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) {
                    u[p] = (P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p]) * t[p];
                    d2 = fma(u[p], u[p], d2);
                }
                double kap, dk;
                kappa_and_dr2<double>(P.kind, d2, kap, dk);
                const double gm = cm * dk, gv = cv * dk;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) {
                    am[p] = fma(gm, u[p], am[p]);
                    av[p] = fma(gv, u[p], av[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) {
            double a = am[p], b = av[p];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                b += __shfl_xor(b, o, 64);
            }
            if (lane == 0 && p < d) {
                // single kind: the sums ran over κ'(r²) u_p with u = s ∘ t; ∂k/∂x*_p = 2 σ² s_p κ' u_p
                const double sp = SUM ? 1.0 : 2.0 * P.variance * (P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p]);
                if (dmean_o) dmean_o[(long)p * ns + i] = sp * a;
                if (dvar_o) dvar_o[(long)p * ns + i] = -2.0 * sp * b;
            }
        }
    }
}

// ---- the joint predictive distribution at the test points: batch_jcov_kernel, batch_jfact_kernel ------------------------------------------------------
// Launched behind batch_predict_kernel, whose strips of one problem lie one after the other and stay alive: together they are the matrix V = K* L⁻ᵀ of the
// problem, (128 · tiles) × ld with row = test point.  Launch boundaries are the only synchronisation; every sum runs in an order the problem's sizes fix.
// What the two kernels know of a problem with test points; `prob` is the position of its BatchProb.  Offsets count doubles: v_off (the strips) and js_off (the
// joint slice in the batch_slice(ns) layout; −1: no factorisation wanted) into the workspace; cov_off (ns × ns, column-major; −1: not wanted), mean_off (the
// mean batch_predict_kernel wrote, without the prior mean; −1 without a joint slice), samp_off (ns × nsamp; −1) and jr_off (held-out logpdf, then the failed minor
// of the joint; −1) into the result buffer; xs_off, ysd_off (y* − m(x*); −1: zeros), nzs_off (a diagonal Σy*; −1: noise_s) and xi_off (ns × nsamp) into the input.
// slot: where the fit left the problem's status (res[nw + slot]) — batch_jfact_kernel reads nothing else of the fit, so it serves the sparse family too
// (gp_vfe_joint_batch: prob is the position of the problem's VfeProb, v_off the strip of B*, c_off that of C*, the mean includes the prior mean and ysd is y*).
struct JointProb {
    long v_off, c_off, js_off, cov_off, mean_off, samp_off, jr_off, xs_off, ysd_off, nzs_off, xi_off;
    int prob, ns, nsp, nsamp, slot, pad_;
    double noise_s;
};
static_assert(sizeof(JointProb) % 8 == 0, "the tables are packed behind double data");

// The 64×64 tile (ti >= tj) of the ns × ns matrix of one problem (GradTile: prob = its JointProb), four waves with one 32×32 wave tile each:
//   acc = K(x*_I, x*_J) evaluated from the packed test points through LDS (identity where a point lies beyond ns), then acc −= V_I V_Jᵀ over the np / 64 blocks of the
//   strips by mfma_tile_k64 — the latent covariance K** − V Vᵀ of gp_posterior_predict's bit 2.
// It is stored twice: into the covariance output, the tile and its mirror image (a diagonal tile computes the pairs j <= i only: both triangles hold the same
// bits by construction), and with Σy* on the diagonal into the lower triangle of the joint slice.  The workgroups of the tiles (ti, 0) also write their 64
// entries of the carried row δ* = y* − m(x*) − mean (row nsp) and of the 31 zero rows behind it.
// Only what this call wrote is read: batch_predict_kernel writes the rows of a strip rounded up to 32, so a wave tile that lies wholly beyond ns touches
// neither the strips nor the covariance.  A failed fit: NaN in the covariance; the joint slice is not written (batch_jfact_kernel does not read it then).
template <bool SUM>
__global__ __launch_bounds__(GNT) void batch_jcov_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                        const JointProb* __restrict__ jps, const GradTile* __restrict__ tiles) {
    __shared__ double Kt[BT * BTS];
    const GradTile& T = tiles[blockIdx.x];
    const JointProb& J = jps[T.prob];
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[J.prob];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = J.ns, nsp = J.nsp, d = P.d;
    const long lds = batch_ld(nsp);
    const bool diag = T.ti == T.tj;
    double* __restrict__ cov = J.cov_off >= 0 ? res + J.cov_off : nullptr;
    double* __restrict__ S = J.js_off >= 0 ? ws + J.js_off : nullptr;
    if (res[nw + P.slot] != 0.0) {
        for (int e = tid; e < BT * BT && cov; e += GNT) {
            const int gi = T.ti * BT + (e >> 6), gj = T.tj * BT + (e & 63);
            if (gi < ns && gj < ns) cov[gj + (long)gi * ns] = cov[gi + (long)gj * ns] = __builtin_nan("");
        }
        return;
    }
    if (S && T.tj == 0) {  // the carried row and the zero rows of the trailing update's 32-row tiles
        const double* mean = res + J.mean_off;
        for (int e = tid; e < BT * 32; e += GNT) {
            const int r = e >> 6, j = T.ti * BT + (e & 63);
            S[(long)(nsp + r) * lds + j] = (r == 0 && j < ns && J.ysd_off >= 0) ? in[J.ysd_off + j] - mean[j] : 0.0;
        }
    }
    {  // K(x*_I, x*_J) into LDS: lane = column with its inputs in registers, the four waves interleave the rows (wave-uniform: the row's inputs by scalar loads)
        const double* __restrict__ xs = in + J.xs_off;
        const int gj = T.tj * BT + lane;
        double xj[BATCH_MAXD];
        batch_load_point(xs, ns, d, gj, xj);
        for (int rr = 0; rr < BT / 4; ++rr) {
            const int li = w + 4 * rr, gi = T.ti * BT + li;
            double v;
            if (gi >= ns || gj >= ns) {
                v = (gi == gj) ? 1.0 : 0.0;
            } else {
                double t[BATCH_MAXD];
                batch_diff(xs, ns, d, gi, xj, t);
                v = batch_kval<SUM>(in, &P, t, d);
            }
            Kt[li * BTS + lane] = v;
        }
    }
    __syncthreads();
    const int wi = w >> 1, wj = w & 1;
    if (diag && wj > wi) return;  // the wave tile strictly above the diagonal: its mirror image computes it
    const int i0 = T.ti * BT + 32 * wi, c0 = T.tj * BT + 32 * wj, r = lane & 15;  // c0 <= i0
    d4_t acc[2][2];
    acc_load(acc, Kt, 32 * wi, 32 * wj, BTS, lane);
    if (i0 < ns) {  // rows i0 … i0 + 31 and c0 … c0 + 31 of the strips lie below ns rounded up to 32: written by this call
        const double* __restrict__ V = ws + J.v_off;
        for (int k0 = 0; k0 < P.np; k0 += BT) mfma_tile_k64<true>(acc, V, i0, V, c0, k0, P.ld, lane);
    }
    const bool lower_only = diag && wi == wj;  // the wave tile on the diagonal: the pairs j <= i, mirrored
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj) {
            const int gj = c0 + 16 * hj + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = i0 + 16 * hi + Tr<double>::crow(lane, q);
                if (lower_only && gj > gi) continue;
                const double v = acc[hi][hj][q];
                if (cov && gi < ns && gj < ns) {
                    cov[gj + (long)gi * ns] = v;
                    if (gi != gj) cov[gi + (long)gj * ns] = v;
                }
                if (S) {
                    const double nz = (gi == gj && gi < ns) ? (J.nzs_off >= 0 ? in[J.nzs_off + gi] : J.noise_s) : 0.0;
                    S[(long)gi * lds + gj] = v + nz;
                    if (diag && gi != gj) S[(long)gj * lds + gi] = v;  // the whole diagonal block is loaded into LDS by the factorisation
                }
            }
        }
}

// The joint slice of one problem per workgroup: batch_chol on C* + Σy* with δ* riding along as row nsp, then
//   hlogpdf = −½ (ns log 2π + 2 Σ log L*_ii + ‖L*⁻¹ δ*‖²)    off the carried row (strided partial sums, then a tree), and the samples
//   out[i, s] = mean_i + Σ_{j <= i} L*_ij ξ_js                  one wave per row i, the lanes striding over j, a butterfly, lane 0 the only writer.
// A non-positive pivot stores its order behind the logpdf, NaN in the logpdf and in the samples; so does a failed fit, with order 0.
__global__ __launch_bounds__(NT) void batch_jfact_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                        const JointProb* __restrict__ jps) {
    __shared__ double Ls[BT][BTS];
    __shared__ double dinv[BT];
    __shared__ double red[NT];
    const JointProb& J = jps[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = J.ns, nsp = J.nsp, nsamp = J.nsamp;
    const long lds = batch_ld(nsp);
    double* __restrict__ A = ws + J.js_off;
    double* __restrict__ out = J.samp_off >= 0 ? res + J.samp_off : nullptr;
    double* __restrict__ jr = res + J.jr_off;
    const bool fit_failed = res[nw + J.slot] != 0.0;  // the same value in every thread
    double logdet_half = 0.0;
    const int failcol = fit_failed ? 0 : batch_chol(A, lds, ns, nsp, tid, lane, w, Ls, dinv, red, logdet_half);
    if (fit_failed || failcol) {
        if (tid == 0) {
            jr[0] = __builtin_nan("");
            jr[1] = (double)failcol;
        }
        for (long e = tid; e < (long)ns * nsamp && out; e += NT) out[e] = __builtin_nan("");
        return;
    }
    {
        double s = 0.0;
        for (int j = tid; j < nsp; j += NT) {
            const double z = A[(long)nsp * lds + j];
            s = fma(z, z, s);
        }
        red[tid] = s;
        __syncthreads();
        for (int h = NT / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) {
            jr[0] = -0.5 * ((double)ns * 1.8378770664093454835606594728112 + 2.0 * logdet_half + red[0]);
            jr[1] = 0.0;
        }
    }
    if (!out) return;
    const double* __restrict__ xi = in + J.xi_off;
    const double* __restrict__ mean = res + J.mean_off;
    for (int i = w; i < ns; i += 8) {  // wave-uniform
        const double* row = A + (long)i * lds;
        for (int s = 0; s < nsamp; ++s) {
            const double* z = xi + (long)s * ns;
            double v = 0.0;
            for (int j = lane; j <= i; j += 64) v = fma(row[j], z[j], v);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) out[(long)s * ns + i] = mean[i] + v;
        }
    }
}

// ---- many small sparse GPs (VFE / DTC, gp_vfe_batch): vfe_prelude_kernel, vfe_stream_kernel, vfe_final_kernel ----------------------------------------------
// The formulation of vfe.hpp (S = Σy^-1/2, L_z L_zᵀ = K_zz + jitter·I):  B = L_z⁻¹ K_zx S,  G = B Bᵀ,  Λ_ε = I + G,  c = B b_y,  m_ε = Λ_ε \ c,  α = L_z⁻ᵀ m_ε,
//   dtc = −½ (n log 2π + log|Σy| + log|Λ_ε| + ‖b_y‖² − ‖L_D⁻¹ c‖²),   elbo = dtc − ½ (tr(K_ff Σy⁻¹) − tr G).
// Three launches on one stream, launch boundaries the only synchronisation: the M×M prelude per problem, the N-long pass per (problem, segment of VFE_SEG
// observations) and the M×M finalisation per problem, which adds the segments' partial sums in segment order.  No flags, no tickets, no floating-point atomics;
// every loop is bounded by the problem's sizes and every sum runs in an order they alone fix.
enum {
    VFE_SEG = GPMI355_VFE_BATCH_SEG,    // consecutive observations per workgroup of the stream kernel: 32 tiles — the 74 KB of W a workgroup loads and the 132 KB
                                        // of partial sums it stores cost about one tile's work each, and an n of 16 384 already spreads over eight workgroups
    VFE_MAXM = GPMI355_VFE_BATCH_MAX_M,
    VT = 64,                            // observations per tile: one per lane in the Gram evaluation
    KBS = 65,                           // LDS row stride of the tile K̃ / B (odd: the row-wise operand reads of B Bᵀ are conflict-free, like BTS)
    VFE_KERNEL_MAX_N = 1 << 24          // what the measurement override admits at most (the segment table of a problem stays small)
};
static_assert(VFE_SEG % VT == 0 && VFE_MAXM % BT == 0 && VFE_MAXM <= 128, "the stream kernel's wave mapping is laid out for M <= 128");

// One problem of a wave, in a table behind the packed data.  Offsets count doubles: z_off (the pseudo-inputs, scaled on the host as the sparse path scales
// them, [d][m]), x_off (raw, [d][n]: shared between problems with different transforms, so the kernel applies the scale at the load — the same product the
// host forms for the single path), y_off, m_off, nz_off (−1: absent) into the packed input; lz_off (the slice of L_z), w_off (the strip L_z⁻ᵀ, np rows of ld),
// d_off (the slice of Λ_ε) and part_off (nseg slots of vfe_part(np)) into the workspace; alpha_off / meps_off into the result buffer (−1: not wanted).
struct VfeProb {
    long z_off, x_off, y_off, m_off, nz_off, lz_off, w_off, d_off, part_off, alpha_off, meps_off;
    int n, m, np, ld, d, kind, nscale, slot, approx, nseg;
    double variance, noise_s, jitter;
    double scale[BATCH_MAXD];
};
static_assert(sizeof(VfeProb) % 8 == 0, "the tables are packed behind double data");
struct VfeSeg {
    int prob, seg;
};
static_assert(sizeof(VfeSeg) % 8 == 0, "the tables are packed behind double data");
// a segment's slot of partial sums: G (np × np, the 32×32 tiles of the lower triangle written), c (np), Σ b², Σ log σ², Σ variance / σ² (+ padding)
__host__ __device__ static inline long vfe_part(long np) { return np * np + np + 8; }

// variance · κ of the squared length of t (inputs scaled beforehand)
__device__ __forceinline__ double vfe_kval(const VfeProb& P, const double (&t)[BATCH_MAXD]) {
    double d2 = 0.0;
#pragma unroll
    for (int p = 0; p < BATCH_MAXD; ++p) d2 = fma(t[p], t[p], d2);
    return P.variance * kappa<double>(P.kind, d2);
}

// One workgroup per problem: the lower triangle of K_zz + jitter·I into the problem's slice (identity padding; the carried row and the 31 rows behind it zero),
// batch_chol, then W = L_z⁻¹ as the strip V = L_z⁻ᵀ = Wᵀ by the substitution of batch_inv_kernel (strip_solve on the identity rows).  A failed factor marks
// the problem (NaN and the minor's order in the result buffer): the later launches never read its slice.
__global__ __launch_bounds__(NT) void vfe_prelude_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                         const VfeProb* __restrict__ vps) {
    __shared__ double sh[BT * BTS + BT];  // L_bb [BT][BTS] and 1 / L_jj behind it
    __shared__ double red[BT];
    const VfeProb& P = vps[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = P.m, np = P.np, d = P.d;
    const long ld = P.ld;
    const int nt = np / BT;
    double* __restrict__ Lz = ws + P.lz_off;
    const double* __restrict__ z = in + P.z_off;
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
            const int j = tj * BT + lane;
            double zj[BATCH_MAXD];
            batch_load_point(z, m, d, j, zj);
            for (int rr = 0; rr < BT / 8; ++rr) {
                const int i = ti * BT + w + 8 * rr;  // wave-uniform
                double v;
                if (i >= m || j >= m) {
                    v = (i == j) ? 1.0 : 0.0;
                } else {
                    double t[BATCH_MAXD];
                    batch_diff(z, m, d, i, zj, t);
                    v = vfe_kval(P, t);
                    if (i == j) v += P.jitter;
                }
                Lz[(long)i * ld + j] = v;
            }
        }
    for (int j = tid; j < np; j += NT)
        for (int r = 0; r < 32; ++r) Lz[(long)(np + r) * ld + j] = 0.0;
    __syncthreads();
    double logdet_half = 0.0;
    const int failcol = batch_chol(Lz, ld, m, np, tid, lane, w, reinterpret_cast<double (*)[BTS]>(sh), sh + BT * BTS, red, logdet_half);
    if (tid == 0) {
        res[P.slot] = failcol ? __builtin_nan("") : 0.0;
        res[nw + P.slot] = (double)failcol;
    }
    if (failcol) return;
    strip_inverse_t(ws + P.w_off, Lz, ld, np, sh, tid, lane, w);
}

// (ti, tj) of the t-th 32×32 tile of a lower triangle counted row by row
__device__ __forceinline__ void lower_tile(int t, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}
// g4 += B[i0 … i0 + 31, :] B[c0 … c0 + 31, :]ᵀ over the 64 observations of the tile in LDS: step s multiplies the observations {4 s + g}, a fixed order
__device__ __forceinline__ void vfe_syrk_tile(d4_t (&g4)[2][2], const double* KB, int i0, int c0, int lane) {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < VT / 4; ++s) {
        const int k = 4 * s + g;
        const double a0 = KB[(i0 + r) * KBS + k], a1 = KB[(i0 + 16 + r) * KBS + k];
        const double b0 = KB[(c0 + r) * KBS + k], b1 = KB[(c0 + 16 + r) * KBS + k];
        g4[0][0] = Tr<double>::mfma(a0, b0, g4[0][0]);
        g4[0][1] = Tr<double>::mfma(a0, b1, g4[0][1]);
        g4[1][0] = Tr<double>::mfma(a1, b0, g4[1][0]);
        g4[1][1] = Tr<double>::mfma(a1, b1, g4[1][1]);
    }
}

// W = L_z⁻¹ out of the strip V = Wᵀ into LDS as the 16×16 blocks of its lower triangle, counted row by row, each k-major (Wt[blk][k][row]); the eight waves
// take the blocks round-robin, and the caller's barrier closes the load.  KS: doubles between the k rows of a block — 16, or 17 where the upper blocks are also
// read transposed out of the lower ones (vfe_predict_kernel<true>; the odd stride is meant to spread the transposed read over the banks, as GTS does in vfe_gstream_kernel — not measured)
template <int KS = 16>
__device__ __forceinline__ void vfe_load_wt(double* Wt, const double* __restrict__ V, long ld, int nb16, int w, int lane) {
    int cnt = 0;
    for (int bi = 0; bi < nb16; ++bi)
        for (int bk = 0; bk <= bi; ++bk, ++cnt) {
            if ((cnt & 7) != w) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = lane + 64 * q;  // e = 16 k + row
                Wt[cnt * (16 * KS) + (e >> 4) * KS + (e & 15)] = V[(long)(16 * bk + (e >> 4)) * ld + 16 * bi + (e & 15)];
            }
        }
}
// acc[q] = (T X)[row block (w >> 2) + 2 q, column block w & 3] for a lower-triangular T and the tile X in LDS (np rows, stride KBS): the k loop of row block bi
// runs over the blocks 0 … bi alone.  frag(bi, bk, k) is T[16 bi + r][16 bk + k], this lane's entry of the A operand.  Returns Σ of the squares of the lane's
// sixteen entries (q, then e: an order the lane's position in the tile does not enter).
template <class Frag>
__device__ __forceinline__ double vfe_tri_mm(d4_t (&acc)[4], const double* X, int nb16, int w, int lane, Frag&& frag) {
    const int r = lane & 15, g = lane >> 4, cb = w & 3;
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = 0.0;
        const int bi = (w >> 2) + 2 * q;
        if (bi < nb16)
            for (int bk = 0; bk <= bi; ++bk)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[q] = Tr<double>::mfma(frag(bi, bk, 4 * s + g), X[(16 * bk + 4 * s + g) * KBS + 16 * cb + r], acc[q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) sq = fma(acc[q][e], acc[q][e], sq);
    }
    return sq;
}
// The transposed counterpart: acc[q] = (T X)[row block (w >> 2) + 2 q, column block w & 3] for an UPPER-triangular T, so the k loop of row block bi runs over
// the blocks bi … nb16 − 1.  frag(bi, bk, k) is T[16 bi + r][16 bk + k] as above; same wave mapping, same order within a block.
template <class Frag>
__device__ __forceinline__ void vfe_triu_mm(d4_t (&acc)[4], const double* X, int nb16, int w, int lane, Frag&& frag) {
    const int r = lane & 15, g = lane >> 4, cb = w & 3;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = 0.0;
        const int bi = (w >> 2) + 2 * q;
        for (int bk = bi; bk < nb16; ++bk)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[q] = Tr<double>::mfma(frag(bi, bk, 4 * s + g), X[(16 * bk + 4 * s + g) * KBS + 16 * cb + r], acc[q]);
    }
}
// the accumulators of vfe_tri_mm back over the tile
__device__ __forceinline__ void vfe_tri_store(const d4_t (&acc)[4], double* X, int nb16, int w, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int bi = (w >> 2) + 2 * q;
        if (bi < nb16)
#pragma unroll
            for (int e = 0; e < 4; ++e) X[(16 * bi + Tr<double>::crow(lane, e)) * KBS + 16 * (w & 3) + (lane & 15)] = acc[q][e];
    }
}

// One workgroup per (problem, segment): the observations [seg·VFE_SEG, min(n, (seg + 1)·VFE_SEG)) in tiles of 64.  LDS (140.8 KB of the CU's 160: one workgroup,
// eight waves, per CU): W = L_z⁻¹ as the 16×16 blocks of its lower triangle, each stored k-major (Wt[blk][k][row]: what the strip V = Wᵀ holds row by row, and
// the MFMA's A operand reads 16 consecutive doubles of it: conflict-free) — 36 blocks, 73.7 KB at M = 128, resident for the whole segment; the tile buffer KB
// (np rows × 64 observations, stride 65, 66.6 KB), which holds K̃ and then B; the 64 entries of b_y.  Per tile:
//   1. K̃[i][j] = variance κ(z_i, x_j) σ_j⁻¹: lane = observation (its inputs scaled at the load, σ_j⁻¹ and b_j formed here; zeros beyond n), the eight waves
//      interleave the pseudo-points (wave-uniform: their inputs by scalar loads); rows from m on are zero.  Wave 0 keeps the three scalar sums per lane.
//   2. B = W K̃: wave w owns the column block w & 3 (16 observations) and the row blocks (w >> 2), (w >> 2) + 2, … — up to four 16×16 accumulators; the k loop
//      of row block bi runs over the blocks 0 … bi alone (W is lower triangular).  All waves finish reading K̃ before any writes B over it.
//   3. G += B Bᵀ on the 32×32 tiles of the lower triangle, accumulators in registers across the whole segment: ten tiles at np = 128 — wave w holds tile w, the
//      waves 6 and 7 also the tiles 8 and 9 (three at np = 64: the waves 0 … 2).  Eight waves and not ten: step 2 splits evenly over eight (4 column blocks × 2 row
//      parities), and the two double-loaded waves sit on different SIMDs (6 and 7 mod 4), so each SIMD's MFMA pipe serves at most three tiles of the ten.
//   4. c += B b_y: thread i < np owns c_i (the waves 0 and 1, which hold one tile each), the 64 products in observation order.
// The segment's G tiles, c and scalar sums go to its own slot.  A problem whose prelude failed returns at once.
__global__ __launch_bounds__(NT) void vfe_stream_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                        const VfeProb* __restrict__ vps, const VfeSeg* __restrict__ segs) {
    __shared__ double Wt[(VFE_MAXM / 16) * (VFE_MAXM / 16 + 1) / 2 * 256];
    __shared__ double KB[VFE_MAXM * KBS];
    __shared__ double bs[VT];
    const VfeSeg S = segs[blockIdx.x];
    const VfeProb& P = vps[S.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int n = P.n, m = P.m, np = P.np, d = P.d, nscale = P.nscale;
    const long ld = P.ld;
    const int nb16 = np / 16, ntl = (np / 32) * (np / 32 + 1) / 2;
    const double* __restrict__ z = in + P.z_off;
    const double* __restrict__ x = in + P.x_off;
    const double* __restrict__ y = in + P.y_off;
    vfe_load_wt(Wt, ws + P.w_off, ld, nb16, w, lane);
    // the wave's tiles of G
    int i0a = 0, c0a = 0, i0b = 0, c0b = 0;
    const bool has_a = w < ntl, has_b = w >= 6 && w + 2 < ntl;
    if (has_a) {
        int ti, tj;
        lower_tile(w, ti, tj);
        i0a = 32 * ti, c0a = 32 * tj;
    }
    if (has_b) {
        int ti, tj;
        lower_tile(w + 2, ti, tj);
        i0b = 32 * ti, c0b = 32 * tj;
    }
    d4_t ga[2][2], gb[2][2];
    acc_zero(ga);
    acc_zero(gb);
    double cacc = 0.0, sb2 = 0.0, slog = 0.0, sinv = 0.0;
    const long o0 = (long)S.seg * VFE_SEG;
    const int cnt = n - o0 < VFE_SEG ? (int)(n - o0) : (int)VFE_SEG;
    __syncthreads();
    for (int t0 = 0; t0 < cnt; t0 += VT) {
        // ---- 1. K̃ into LDS
        {
            const bool valid = t0 + lane < cnt;
            const long j = o0 + t0 + lane;
            double xj[BATCH_MAXD];
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p)
                xj[p] = (p < d && valid) ? (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * x[(long)p * n + j] : 0.0;
            double rs = 0.0;
            if (valid) {
                const double s2 = P.nz_off >= 0 ? in[P.nz_off + j] : P.noise_s;
                rs = 1.0 / sqrt(s2);
                if (w == 0) {
                    const double bj = (y[j] - (P.m_off >= 0 ? in[P.m_off + j] : 0.0)) * rs;
                    bs[lane] = bj;
                    sb2 = fma(bj, bj, sb2);
                    if (P.nz_off >= 0) {
                        slog += log(s2);
                        sinv += P.variance / s2;
                    }
                }
            } else if (w == 0) {
                bs[lane] = 0.0;
            }
            for (int rr = 0; rr < np / 8; ++rr) {
                const int i = w + 8 * rr;  // wave-uniform
                double v = 0.0;
                if (i < m && valid) {
                    double t[BATCH_MAXD];
                    batch_diff(z, m, d, i, xj, t);
                    v = vfe_kval(P, t) * rs;
                }
                KB[i * KBS + lane] = v;
            }
        }
        __syncthreads();
        // ---- 2. B = W K̃ over the non-zero k blocks, into registers; then over K̃
        {
            d4_t acc[4];
            (void)vfe_tri_mm(acc, KB, nb16, w, lane, [&](int bi, int bk, int k) { return Wt[(bi * (bi + 1) / 2 + bk) * 256 + k * 16 + r]; });
            __syncthreads();
            vfe_tri_store(acc, KB, nb16, w, lane);
        }
        __syncthreads();
        // ---- 3. G += B Bᵀ;  4. c += B b_y
        if (has_a) vfe_syrk_tile(ga, KB, i0a, c0a, lane);
        if (has_b) vfe_syrk_tile(gb, KB, i0b, c0b, lane);
        if (tid < np)
            for (int j = 0; j < VT; ++j) cacc = fma(KB[tid * KBS + j], bs[j], cacc);
        __syncthreads();
    }
    double* __restrict__ part = ws + P.part_off + (long)S.seg * vfe_part(np);
    if (has_a) acc_store(ga, part, i0a, c0a, np, lane);
    if (has_b) acc_store(gb, part, i0b, c0b, np, lane);
    if (tid < np) part[(long)np * np + tid] = cacc;
    if (w == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sb2 += __shfl_xor(sb2, o, 64);
            slog += __shfl_xor(slog, o, 64);
            sinv += __shfl_xor(sinv, o, 64);
        }
        if (lane == 0) {
            double* sc = part + (long)np * np + np;
            sc[0] = sb2;
            sc[1] = slog;
            sc[2] = sinv;
        }
    }
}

// One workgroup per problem: the segments' partial sums in segment order into the slice of Λ_ε = I + G (c as the carried row np, the layout batch_logpdf_kernel
// uses for δ), batch_chol, the objective from Σ log L_D,ii, ‖L_D⁻¹ c‖² (the carried row) and the scalar sums (a scalar σ²: n log σ² and n variance / σ², as the
// single path forms them), then m_ε = L_D⁻ᵀ (L_D⁻¹ c) and α = L_z⁻ᵀ m_ε by back_sweep where they are wanted.  A problem whose prelude failed gets NaN weights
// here (objective and info are the prelude's); a Λ_ε that is not positive definite is data in the same way.
__global__ __launch_bounds__(NT) void vfe_final_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                       const VfeProb* __restrict__ vps) {
    __shared__ double Ls[BT][BTS];
    __shared__ double dinv[BT];
    __shared__ double red[NT];
    __shared__ double zs[VFE_MAXM];
    const VfeProb& P = vps[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = P.n, m = P.m, np = P.np, nseg = P.nseg;
    const long ld = P.ld, psz = vfe_part(np);
    const int nt = np / BT;
    double* alpha = P.alpha_off >= 0 ? res + P.alpha_off : nullptr;
    double* meps = P.meps_off >= 0 ? res + P.meps_off : nullptr;
    auto nan_weights = [&] {
        if (tid < m) {
            if (alpha) alpha[tid] = __builtin_nan("");
            if (meps) meps[tid] = __builtin_nan("");
        }
    };
    if (res[nw + P.slot] != 0.0) {
        nan_weights();
        return;
    }
    double* __restrict__ D = ws + P.d_off;
    const double* __restrict__ part = ws + P.part_off;
    for (int e = tid; e < np * np; e += NT) {
        const int i = e / np, j = e - i * np;
        double s = 0.0;
        if ((j >> 5) <= (i >> 5))
            for (int sg = 0; sg < nseg; ++sg) s += part[sg * psz + e];
        if (i == j) {
            zs[i] = i < m ? s : 0.0;  // the diagonal of G, for its trace
            s += 1.0;
        }
        D[(long)i * ld + j] = s;
    }
    for (int j = tid; j < np; j += NT) {
        double s = 0.0;
        for (int sg = 0; sg < nseg; ++sg) s += part[sg * psz + (long)np * np + j];
        D[(long)np * ld + j] = s;
        for (int r = 1; r < 32; ++r) D[(long)(np + r) * ld + j] = 0.0;
    }
    double dd = 0.0, logdet_sy = 0.0, tr_kff = 0.0, tr_g = 0.0;  // thread 0
    __syncthreads();
    if (tid == 0) {
        for (int sg = 0; sg < nseg; ++sg) {
            const double* sc = part + sg * psz + (long)np * np + np;
            dd += sc[0];
            logdet_sy += sc[1];
            tr_kff += sc[2];
        }
        if (P.nz_off < 0) {
            logdet_sy = (double)n * log(P.noise_s);
            tr_kff = (double)n * (P.variance / P.noise_s);
        }
        for (int i = 0; i < m; ++i) tr_g += zs[i];
    }
    __syncthreads();
    double logdet_half = 0.0;
    const int failcol = batch_chol(D, ld, m, np, tid, lane, w, Ls, dinv, red, logdet_half);
    if (failcol) {
        if (tid == 0) {
            res[P.slot] = __builtin_nan("");
            res[nw + P.slot] = (double)failcol;
        }
        nan_weights();
        return;
    }
    {  // ‖L_D⁻¹ c‖² from the carried row, as batch_logpdf_kernel reads ‖L⁻¹δ‖²
        double s = 0.0;
        for (int j = tid; j < np; j += NT) {
            const double v = D[(long)np * ld + j];
            zs[j] = v;
            s = fma(v, v, s);
        }
        red[tid] = s;
        __syncthreads();
        for (int h = NT / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) {
            double obj = -0.5 * ((double)n * 1.8378770664093454835606594728112 + logdet_sy + 2.0 * logdet_half + dd - red[0]);
            if (P.approx == 0) obj -= 0.5 * (tr_kff - tr_g);
            res[P.slot] = obj;
        }
    }
    if (!alpha && !meps) return;
    back_sweep(D, ld, nt, zs, Ls, tid, lane, w);
    if (meps && tid < m) meps[tid] = zs[tid];
    if (!alpha) return;
    back_sweep(ws + P.lz_off, ld, nt, zs, Ls, tid, lane, w);
    if (tid < m) alpha[tid] = zs[tid];
}

// ---- value AND gradient of many small sparse GPs (gp_vfe_grad_batch): vfe_gmm_kernel, vfe_gstream_kernel, vfe_gfinish_kernel behind the three launches above ----
// The formulation of vfe.hpp's gradient (V = L_z⁻ᵀ, the strip the prelude left; A = Λ_ε, its factor left by vfe_final_kernel; G = B Bᵀ):
//   G_ψ = ½[V H_ψ Vᵀ − ααᵀ], H_ψ = I − A⁻¹ (VFE) | −A⁻¹ (DTC);   G_zz = ½[V H_zz Vᵀ − ααᵀ], H_zz = H_ψ − G (VFE) | H_ψ + I (DTC);
//   per (pseudo-point i, observation j), T = G_ψ K̃:  W_ij = σ_j⁻¹(2 T_ij + b_j α_i), ∂/∂variance += W κ, w_ij = 2 W variance κ′ weighs ∂r²_ij;
//   q_j = Σ_i variance κ_ij T_ij, p_j = Σ_i K̃_ij α_i  →  ∂/∂σ_j² and ∂/∂y_j as vgrad_finish_kernel forms them.
// What the problem's gradient lays out, in its wave's tables beside VfeProb: u_off (the strip Λ_ε.L⁻ᵀ), h_off (H_ψ, then H_zz), rt_off (V H), gpsi_off,
// gzz_off (np rows of ld each; gzz_off holds G until G_zz is written over it) and gpart_off (nseg slots of vfe_gpart(np, d)) into the workspace; gh_off
// (∂/∂variance, 16 × ∂/∂scale, Σ ∂/∂σ²), dz_off ([d][m]), dn_off ([n], −1 for a scalar σ²), dy_off ([n]) and dx_off ([d][n], −1: not wanted) into the results.
struct VfeGrad {
    long u_off, h_off, rt_off, gpsi_off, gzz_off, gpart_off, gh_off, dz_off, dn_off, dy_off, dx_off;
};
static_assert(sizeof(VfeGrad) % 8 == 0, "the tables are packed behind double data");
enum {
    VFE_GH = 20,   // the hyper-parameter block of a problem's results: [0] ∂/∂variance, [1 + p] ∂/∂scale_p, [17] Σ_j ∂/∂σ_j²
    GTS = 16 * 17  // a 16×16 block of G_ψ in LDS, k-major with row stride 17: read as stored and transposed (the upper blocks, through symmetry) without conflicts
};
// a segment's slot of gradient sums: Σ_j w_ij (z_i − x_j)_p and Σ_j w_ij (z_i − x_j)_p², both [d][np]; then Σ W κ, Σ_j ∂/∂σ_j², Σ_j σ_j⁻² (+ padding)
__host__ __device__ static inline long vfe_gpart(long np, long d) { return 2 * np * d + 8; }

// C = X Yᵀ on the 32×32 tiles (ti, tj) a workgroup's eight waves take round-robin, operands row-major with stride ld, from global memory through
// mfma_tile_k64; the k loop of a tile starts at the 64-block klo(i0, j0) (what lies left of it is zero in an upper-triangular operand).  lower_only: the
// tiles tj <= ti alone.  epi(i, j, v) gets every entry of the tile.
template <class KLo, class Epi>
__device__ __forceinline__ void vfe_mm_xyt(const double* X, const double* Y, long ld, int np, bool lower_only, int w, int lane, KLo&& klo, Epi&& epi) {
    const int n32 = np / 32;
    int cnt = 0;
    for (int ti = 0; ti < n32; ++ti)
        for (int tj = 0; tj < (lower_only ? ti + 1 : n32); ++tj) {
            if ((cnt++ & 7) != w) continue;
            const int i0 = 32 * ti, j0 = 32 * tj;
            d4_t acc[2][2];
            acc_zero(acc);
            for (int k0 = klo(i0, j0) / BT * BT; k0 < np; k0 += BT) mfma_tile_k64<false>(acc, X, i0, Y, j0, k0, ld, lane);
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q) epi(i0 + 16 * (h >> 1) + Tr<double>::crow(lane, q), j0 + 16 * (h & 1) + (lane & 15), acc[h >> 1][h & 1][q]);
        }
}

// One workgroup per problem, the M×M side: U = Λ_ε.L⁻ᵀ by strip_solve on identity rows (as the prelude forms V), G = B Bᵀ summed again from the segments'
// slots in segment order (vfe_final_kernel factored over its sum), then five products X Yᵀ on the fp64 MFMA in 32×32 wave tiles, zero 64-blocks of the
// triangular operands skipped:  A⁻¹ = U Uᵀ → H_ψ;  R = V H_ψ;  V Rᵀ → G_ψ;  H_zz in place;  R = V H_zz;  V Rᵀ → G_zz.  The two conjugations compute the
// lower tiles and write both halves: G_ψ and G_zz are symmetric to the bit.  Rows and columns from m on are written as zeros (V and A are the identity
// there, so nothing of the padding reaches the m × m block; the −1 the DTC H_ψ would keep on the padded diagonal is dropped with them).
__global__ __launch_bounds__(NT) void vfe_gmm_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                     const VfeProb* __restrict__ vps, const VfeGrad* __restrict__ gps) {
    __shared__ double sh[BT * BTS + BT];
    __shared__ double al[VFE_MAXM];
    const VfeProb& P = vps[blockIdx.x];
    const VfeGrad& Q = gps[blockIdx.x];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = P.m, np = P.np, nseg = P.nseg;
    const long ld = P.ld, psz = vfe_part(np);
    const double vfe = P.approx == 0 ? 1.0 : 0.0;
    double* __restrict__ U = ws + Q.u_off;
    double* __restrict__ H = ws + Q.h_off;
    double* __restrict__ R = ws + Q.rt_off;
    double* __restrict__ Gp = ws + Q.gpsi_off;
    double* __restrict__ Gz = ws + Q.gzz_off;
    const double* __restrict__ V = ws + P.w_off;
    const double* __restrict__ part = ws + P.part_off;
    for (int e = tid; e < np * np; e += NT) {
        const int i = e / np, j = e - i * np;
        const int src = (j >> 5) <= (i >> 5) ? e : j * np + i;  // the stream kernel wrote the 32×32 tiles of the lower triangle
        double s = 0.0;
        for (int sg = 0; sg < nseg; ++sg) s += part[sg * psz + src];
        Gz[(long)i * ld + j] = s;
    }
    if (tid < np) al[tid] = tid < m ? res[P.alpha_off + tid] : 0.0;
    strip_inverse_t(U, ws + P.d_off, ld, np, sh, tid, lane, w);  // its barrier also orders the sums above
    auto from_row = [](int i0, int) { return i0; };
    auto from_both = [](int i0, int j0) { return i0 > j0 ? i0 : j0; };
    auto to_R = [&](int i, int j, double v) { R[(long)i * ld + j] = v; };
    vfe_mm_xyt(U, U, ld, np, false, w, lane, from_both, [&](int i, int j, double v) { H[(long)i * ld + j] = (i < m && j < m) ? (i == j ? vfe : 0.0) - v : 0.0; });
    __syncthreads();
    auto conj_into = [&](double* G) {  // G = ½[V H Vᵀ − ααᵀ], both halves from the lower tiles
        vfe_mm_xyt(V, H, ld, np, false, w, lane, from_row, to_R);  // R = V H (H symmetric)
        __syncthreads();
        vfe_mm_xyt(V, R, ld, np, true, w, lane, from_row, [&](int i, int j, double v) {
            if (j > i) return;
            const double gv = (i < m && j < m) ? 0.5 * (v - al[i] * al[j]) : 0.0;
            G[(long)i * ld + j] = gv;
            G[(long)j * ld + i] = gv;
        });
        __syncthreads();
    };
    conj_into(Gp);
    for (int e = tid; e < m * m; e += NT) {
        const int i = e / m, j = e - i * m;
        H[(long)i * ld + j] += (i == j ? 1.0 - vfe : 0.0) - vfe * Gz[(long)i * ld + j];
    }
    __syncthreads();
    conj_into(Gz);
}

// One workgroup per (problem, segment), the table of the fit's stream kernel; tiles of 64 observations.  LDS, 159.7 KB of the CU's 160 — one workgroup per CU,
// as in the fit:  G_ψ as the 36 16×16 blocks of its lower triangle (GTS apart, 78.3 KB at M = 128; a full 128×128 copy, 131 KB, does not fit beside the tile
// buffer, so the upper blocks are read transposed out of the lower ones — the stride of 17 keeps both reads conflict-free), resident for the whole segment;
// the tile buffer KB (np × 64, stride 65, 66.6 KB), which holds K̃, then T, then w; the tile's scaled inputs xs [d][64]; α; per observation b_j and p_j;
// one [8][64] table for the two sums the eight waves add up per observation.  Per tile:
//   1. K̃ as in the fit (lane = observation, the waves interleave the pseudo-points) and, on the way, the wave's share of p_j = Σ_i K̃_ij α_i;
//   2. T = G_ψ K̃ by MFMA over all k blocks, wave mapping of the fit's B = W K̃; T overwrites K̃ once every wave has read it;
//   3. the elementwise pass, mapping of step 1: κ and κ′ again from (z_i − x_j) (kappa_and_dr2), W_ij, the thread's Σ W κ, the wave's share of q_j, and
//      w_ij over T_ij.  Wave 0 then finishes ∂/∂σ_j² and ∂/∂y_j of the tile's observations and writes them straight to the results;
//   4. the reductions over w: thread (i, p) — up to four pairs a thread, fixed for the segment, z_ip in a register — adds Σ_j w_ij t and Σ_j w_ij t² with
//      t = z_ip − x_jp formed from the difference itself, in observation order, into its accumulators; where ∂/∂x is wanted thread (j, p) adds
//      Σ_i w_ij (x_jp − z_ip) in pseudo-point order and writes it to the results.  K̃, T and w never reach HBM.
// The segment's sums go to its own slot; every order above is fixed by (m, d, the segment's range) alone.
__global__ __launch_bounds__(NT) void vfe_gstream_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                         const VfeProb* __restrict__ vps, const VfeGrad* __restrict__ gps, const VfeSeg* __restrict__ segs) {
    __shared__ double Gt[(VFE_MAXM / 16) * (VFE_MAXM / 16 + 1) / 2 * GTS];
    __shared__ double KB[VFE_MAXM * KBS];
    __shared__ double xs[BATCH_MAXD * VT];
    __shared__ double red[8 * VT];
    __shared__ double al[VFE_MAXM];
    __shared__ double bs[VT], pj[VT];
    const VfeSeg S = segs[blockIdx.x];
    const VfeProb& P = vps[S.prob];
    const VfeGrad& Q = gps[S.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int n = P.n, m = P.m, np = P.np, d = P.d, nscale = P.nscale;
    const long ld = P.ld;
    const int nb16 = np / 16;
    const double var = P.variance;
    const double* __restrict__ z = in + P.z_off;
    const double* __restrict__ x = in + P.x_off;
    const double* __restrict__ y = in + P.y_off;
    {
        const double* __restrict__ Gp = ws + Q.gpsi_off;
        int cnt = 0;
        for (int bi = 0; bi < nb16; ++bi)
            for (int bk = 0; bk <= bi; ++bk, ++cnt) {
                if ((cnt & 7) != w) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = lane + 64 * q;  // e = 16 row + k
                    Gt[cnt * GTS + (e & 15) * 17 + (e >> 4)] = Gp[(long)(16 * bi + (e >> 4)) * ld + 16 * bk + (e & 15)];
                }
            }
        if (tid < np) al[tid] = tid < m ? res[P.alpha_off + tid] : 0.0;
    }
    // the thread's (i, p) pairs: e = p np + i
    double zi[4], accz[4], accs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + NT * q, p = e / np, i = e - p * np;
        zi[q] = (p < d && i < m) ? z[(long)p * m + i] : 0.0;
        accz[q] = accs[q] = 0.0;
    }
    double vacc = 0.0, dnsum = 0.0, r2sum = 0.0;
    const long o0 = (long)S.seg * VFE_SEG;
    const int cnt = n - o0 < VFE_SEG ? (int)(n - o0) : (int)VFE_SEG;
    __syncthreads();
    for (int t0 = 0; t0 < cnt; t0 += VT) {
        const bool valid = t0 + lane < cnt;
        const long j = o0 + t0 + lane;
        double xj[BATCH_MAXD];
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p)
            xj[p] = (p < d && valid) ? (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * x[(long)p * n + j] : 0.0;
        double rs = 0.0;
        // ---- 1. K̃ into LDS, the wave's share of p_j
        {
            if (valid) rs = 1.0 / sqrt(P.nz_off >= 0 ? in[P.nz_off + j] : P.noise_s);
            if (w == 0) bs[lane] = valid ? (y[j] - (P.m_off >= 0 ? in[P.m_off + j] : 0.0)) * rs : 0.0;
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p)
                if ((p & 7) == w) xs[p * VT + lane] = xj[p];
            double pp = 0.0;
            for (int rr = 0; rr < np / 8; ++rr) {
                const int i = w + 8 * rr;  // wave-uniform
                double v = 0.0;
                if (i < m && valid) {
                    double t[BATCH_MAXD];
                    batch_diff(z, m, d, i, xj, t);
                    v = vfe_kval(P, t) * rs;
                    pp = fma(v, al[i], pp);
                }
                KB[i * KBS + lane] = v;
            }
            red[w * VT + lane] = pp;
        }
        __syncthreads();
        if (w == 1) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += red[q * VT + lane];
            pj[lane] = s;
        }
        // ---- 2. T = G_ψ K̃ into registers; then over K̃
        {
            const int cb = w & 3;
            d4_t acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q] = 0.0;
                const int bi = (w >> 2) + 2 * q;
                if (bi < nb16)
                    for (int bk = 0; bk < nb16; ++bk) {
                        const bool low = bk <= bi;
                        const double* gb = Gt + (low ? bi * (bi + 1) / 2 + bk : bk * (bk + 1) / 2 + bi) * GTS;
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc[q] = Tr<double>::mfma(low ? gb[(4 * s + g) * 17 + r] : gb[r * 17 + 4 * s + g], KB[(16 * bk + 4 * s + g) * KBS + 16 * cb + r], acc[q]);
                    }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int bi = (w >> 2) + 2 * q;
                if (bi < nb16)
#pragma unroll
                    for (int e = 0; e < 4; ++e) KB[(16 * bi + Tr<double>::crow(lane, e)) * KBS + 16 * cb + r] = acc[q][e];
            }
        }
        __syncthreads();
        // ---- 3. the elementwise pass: w over T, the wave's share of q_j
        {
            const double bj = bs[lane];
            double qq = 0.0;
            for (int rr = 0; rr < np / 8; ++rr) {
                const int i = w + 8 * rr;  // wave-uniform
                if (i >= m) break;
                double t[BATCH_MAXD];
                batch_diff(z, m, d, i, xj, t);
                double d2 = 0.0;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) d2 = fma(t[p], t[p], d2);
                double kap, dk;
                kappa_and_dr2<double>(P.kind, d2, kap, dk);
                const double T = KB[i * KBS + lane];
                const double W = rs * (2.0 * T + bj * al[i]);
                vacc = fma(W, kap, vacc);
                qq = fma(var * kap, T, qq);
                KB[i * KBS + lane] = valid ? 2.0 * W * var * dk : 0.0;
            }
            red[w * VT + lane] = qq;
        }
        __syncthreads();
        if (w == 0 && valid) {
            double rq = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) rq += red[q * VT + lane];
            const double b = bs[lane], r2 = rs * rs, pr = pj[lane];  // pr = σ_j⁻¹ Σ_i variance κ_ij α_i
            const double dn = -0.5 * r2 + 0.5 * b * b * r2 - rq * r2 * rs - pr * b * r2 + (P.approx == 0 ? 0.5 * var * r2 * r2 : 0.0);
            res[Q.dy_off + j] = -(b * rs - pr * rs);
            if (Q.dn_off >= 0) res[Q.dn_off + j] = dn;
            dnsum += dn;
            r2sum += r2;
        }
        // ---- 4. the reductions over w
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + NT * q, p = e / np, i = e - p * np;
            if (p < d && i < m) {
                const double* wr = KB + i * KBS;
                const double* xp = xs + p * VT;
                double az = accz[q], as = accs[q];
                for (int jj = 0; jj < VT; ++jj) {
                    const double t = zi[q] - xp[jj], wt = wr[jj] * t;
                    az += wt;
                    as = fma(wt, t, as);
                }
                accz[q] = az, accs[q] = as;
            }
        }
        if (Q.dx_off >= 0)
            for (int p = w; p < d; p += 8) {  // wave-uniform
                const double sp = nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p];
                const double xv = xs[p * VT + lane];
                double s = 0.0;
                for (int i = 0; i < m; ++i) s = fma(KB[i * KBS + lane], xv - z[(long)p * m + i], s);
                if (valid) res[Q.dx_off + (long)p * n + j] = sp * s;
            }
        __syncthreads();
    }
    double* __restrict__ part = ws + Q.gpart_off + (long)S.seg * vfe_gpart(np, d);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + NT * q;
        if (e < np * d) {
            part[e] = accz[q];
            part[(long)np * d + e] = accs[q];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        vacc += __shfl_xor(vacc, o, 64);
        dnsum += __shfl_xor(dnsum, o, 64);
        r2sum += __shfl_xor(r2sum, o, 64);
    }
    if (lane == 0) red[w] = vacc;
    __syncthreads();
    if (tid == 0) {
        double* sc = part + 2L * np * d;
        double v = 0.0;
        for (int q = 0; q < 8; ++q) v += red[q];
        sc[0] = v;
        sc[1] = dnsum;
        sc[2] = r2sum;
    }
}

// One workgroup per problem: the segments' sums in segment order, then the K_zz term — w_ij = 2 G_zz,ij variance κ′(z_i, z_j) over the full m × m square
// into LDS (lane = column, the waves interleave the rows, as in the stream kernel; Σ G_zz κ on the way), reduced by the same (i, p) threads with factor 2 on
// ∂/∂z (z_i enters K_zz through both arguments) — the trace term of the VFE objective on ∂/∂variance, and the problem's results: ∂/∂z as [d][m] times the
// scales, ∂/∂scale (ARD: per dimension, the rows in order; one Scale: all dimensions), ∂/∂variance and Σ_j ∂/∂σ_j².
__global__ __launch_bounds__(NT) void vfe_gfinish_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                         const VfeProb* __restrict__ vps, const VfeGrad* __restrict__ gps) {
    __shared__ double WK[VFE_MAXM * (VFE_MAXM + 1)];
    __shared__ double zl[BATCH_MAXD * VFE_MAXM];
    __shared__ double red[8];
    const VfeProb& P = vps[blockIdx.x];
    const VfeGrad& Q = gps[blockIdx.x];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = P.m, np = P.np, d = P.d, nseg = P.nseg, nscale = P.nscale;
    const long ld = P.ld, gsz = vfe_gpart(np, d);
    const int wks = np + 1;
    const double var = P.variance;
    const double* __restrict__ z = in + P.z_off;
    const double* __restrict__ Gz = ws + Q.gzz_off;
    const double* __restrict__ part = ws + Q.gpart_off;
    for (int e = tid; e < d * np; e += NT) {
        const int p = e / np, i = e - p * np;
        zl[e] = i < m ? z[(long)p * m + i] : 0.0;
    }
    double accz[4], accs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + NT * q;
        accz[q] = accs[q] = 0.0;
        if (e < np * d)
            for (int sg = 0; sg < nseg; ++sg) {
                accz[q] += part[sg * gsz + e];
                accs[q] += part[sg * gsz + (long)np * d + e];
            }
    }
    double vacc = 0.0;
    for (int j0 = 0; j0 < np; j0 += 64) {
        const int j = j0 + lane;
        double zj[BATCH_MAXD];
        batch_load_point(z, m, d, j, zj);
        for (int rr = 0; rr < np / 8; ++rr) {
            const int i = w + 8 * rr;  // wave-uniform
            double v = 0.0;
            if (i < m && j < m) {
                double t[BATCH_MAXD];
                batch_diff(z, m, d, i, zj, t);
                double d2 = 0.0;
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) d2 = fma(t[p], t[p], d2);
                double kap, dk;
                kappa_and_dr2<double>(P.kind, d2, kap, dk);
                const double W = Gz[(long)i * ld + j];
                vacc = fma(W, kap, vacc);
                v = 2.0 * W * var * dk;
            }
            WK[i * wks + j] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + NT * q, p = e / np, i = e - p * np;
        if (p < d && i < m) {
            const double zv = zl[e];
            double az = 0.0, as = 0.0;
            for (int j = 0; j < m; ++j) {
                const double t = zv - zl[p * np + j], wt = WK[i * wks + j] * t;
                az += wt;
                as = fma(wt, t, as);
            }
            accz[q] += 2.0 * az;
            accs[q] += as;
            res[Q.dz_off + (long)p * m + i] = (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * accz[q];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) vacc += __shfl_xor(vacc, o, 64);
    __syncthreads();
    if (lane == 0) red[w] = vacc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = tid + NT * q;
        if (e < np * d) WK[e] = accs[q];  // [d][np]; rows from m on hold zeros
    }
    __syncthreads();
    double* gh = res + Q.gh_off;
    if (tid == 0) {
        double v = 0.0, dns = 0.0, r2 = 0.0;
        for (int sg = 0; sg < nseg; ++sg) {
            const double* sc = part + sg * gsz + 2L * np * d;
            v += sc[0];
            dns += sc[1];
            r2 += sc[2];
        }
        for (int q = 0; q < 8; ++q) v += red[q];
        gh[0] = v - (P.approx == 0 ? 0.5 * r2 : 0.0);
        gh[17] = dns;
    }
    if (tid < (nscale == 1 ? 1 : nscale)) {
        double s = 0.0;
        for (int e = (nscale == 1 ? 0 : tid * np); e < (nscale == 1 ? d * np : (tid + 1) * np); ++e) s += WK[e];
        gh[1 + tid] = s / P.scale[tid];
    }
}

// ---- predictions of many small sparse GPs (gp_vfe_predict_batch): vfe_pprep_kernel, vfe_predict_kernel behind the fit's three launches ---------------------
// With k*_j = K(z, x*_j), W = L_z⁻¹ (the strip the prelude left), E = L_D⁻¹ (L_D the factor of Λ_ε vfe_final_kernel left) and α out of the result buffer:
//   mean_j = m(x*_j) + k*_jᵀ α,   var_j = k(x*_j, x*_j) − ‖W k*_j‖² + ‖E W k*_j‖²   (not clamped; the single path's formula, the same for VFE and DTC).
// The two norms and not one resident Q = Wᵀ(I − Λ_ε⁻¹)W: the explicit Q loses two to three digits of the variance where it is smallest (include/gpmi355.h).
enum {
    VFE_PSEG = GPMI355_VFE_PREDICT_BATCH_SEG,  // consecutive test points per workgroup of the predict kernel
    VFE_PRED_LAUNCH_SEGS = 1 << 16             // segments per predict launch at most
};
static_assert(VFE_PSEG % VT == 0, "a segment is whole tiles");
// What a problem's predictions lay out beside VfeProb: u_off, the strip E ᵀ = L_D⁻ᵀ (np rows of ld) in the workspace; −1 where no variance is asked for or the
// problem has no test points.  bs_off / cs_off (gp_vfe_joint_batch; −1 otherwise): the strips vfe_predict_kernel<false, true> stores B* and C* into, row = test
// point — ns rounded up to 64 rows of ld doubles each, the columns [0, np) of every row written (zeros from m on and in the rows from ns on).
struct VfePred {
    long u_off, bs_off, cs_off;
};
// One segment of test points: xs_off ([d][ns], raw) and pm_off (m(x*), −1: none) into the packed input, mean_off / var_off (arrays of ns; −1: not wanted) and
// dmean_off / dvar_off (gp_vfe_predict_grad_batch: the gradients w.r.t. the test inputs, dimension-major [d][ns]; −1: not wanted) into the result buffer; the
// points [row0, row0 + cnt) of the ns of problem `prob`.
struct VfePSeg {
    long xs_off, pm_off, mean_off, var_off, dmean_off, dvar_off;
    int prob, ns, row0, cnt;
};
static_assert(sizeof(VfePred) % 8 == 0 && sizeof(VfePSeg) % 8 == 0, "the tables are packed behind double data");

// One workgroup per problem: E = L_D⁻¹ as the strip U = L_D⁻ᵀ, the first step of vfe_gmm_kernel.  A problem whose fit failed, or that needs no strip, is skipped.
__global__ __launch_bounds__(NT) void vfe_pprep_kernel(const double* __restrict__ in, double* __restrict__ ws, const double* __restrict__ res, int nw,
                                                       const VfeProb* __restrict__ vps, const VfePred* __restrict__ pps) {
    __shared__ double sh[BT * BTS + BT];
    const VfeProb& P = vps[blockIdx.x];
    const long u_off = pps[blockIdx.x].u_off;
    if (u_off < 0 || res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    strip_inverse_t(ws + u_off, ws + P.d_off, P.ld, P.np, sh, tid, lane, w);
}

// One workgroup per (problem, segment of VFE_PSEG test points), tiles of 64.  LDS, 140 KB (one workgroup, eight waves, per CU): W in the blocked layout of
// vfe_stream_kernel, resident for the whole segment; the tile buffer KB (np × 64, stride 65), which holds K*, then B*; α; the partial column norms of the two
// row parities.  E does not fit beside them: its operand fragments come from global memory — the strip U = Eᵀ holds the sixteen rows of a fragment
// consecutively, at most 128 KB per problem and read by every workgroup of the problem, so it stays in L2.  Per tile:
//   1. K*[i][j] = variance κ(z_i, x*_j): lane = test point (its inputs scaled at the load; zeros beyond cnt), the eight waves interleave the pseudo-points;
//      rows from m on are zero.  Wave 0 then takes mean_j = m_j + Σ_i K*_ij α_i off the tile, in pseudo-point order.
//   2. B* = W K* (vfe_tri_mm, the stream kernel's product), written over K* once every wave has read it; ‖B*_j‖² out of the accumulators.
//   3. C* = E B* the same way, never stored: ‖C*_j‖² alone.
//   4. var_j = (variance − ‖B*_j‖²) + ‖C*_j‖², wave 0.
// The norm of a column is the sum of its lane's sixteen squares, then of the four lane groups by two exchanges, then of the two row parities: no step sees
// another column or the column's place in the tile, so a test point's results are the same bits in any company.  Padding rows of B* and C* are zero, padding
// test points are never written.  A problem whose fit failed returns at once (the host fills its NaN).
//
// GRAD (gp_vfe_predict_grad_batch) goes on per tile, with B* kept in the accumulators of step 2 and u_j = Wᵀ (B*_j − Eᵀ E B*_j):
//   5. C* over B* in the tile buffer (every wave has read B* by then); D* = B* − Eᵀ C* (vfe_triu_mm: Eᵀ is upper triangular, the k loop of row block bi runs over
//      bi … nb16 − 1; its fragments are the strip U read along its rows, sixteen rows a fragment, from L2), D* over C*.
//   6. U* = Wᵀ D* the same way, Wᵀ's fragments read transposed out of the resident lower blocks of W (k rows 17 apart instead of 16, so that the sixteen rows of this read
//      do not all fall on one bank as they would 16 apart — the intent, not measured; 78.3 KB instead of 73.7), U* over D*.
//   7. the contraction, in the mapping of step 1: lane = test point, the eight waves interleave the pseudo-points; κ′ of (z_i − x*_j) once per (i, j) for both
//      sides (kappa_and_dr2; Matern12 at distance 0 gives 0), Σ_i α_i κ′ t_p and Σ_i U*_ij κ′ t_p in 2 × 16 registers.  The eight waves' sums meet in the tile
//      buffer, free by then — [wave][dimension][point], 64 KB at D = 16, one side after the other — and thread (p, j) adds them in wave order and writes
//      dmean[j, p] = −2 σ² s_p Σ,  dvar[j, p] = 4 σ² s_p Σ  (t = z_i − s ∘ x*_j).  One writer per (j, p), no atomics; every order is fixed by m alone.
// Mean side alone: no W, no strip, no MFMA — steps 1 and 7.  The values take the steps above unchanged: they are gp_vfe_predict_batch's bits.
//
// STRIP (gp_vfe_joint_batch, vfe_predict_kernel<false, true>) runs steps 1 – 3 as they are — the chain always, the variance never — and stores the tile of B* out of
// the accumulators of step 2 and that of C* out of those of step 3 into the problem's two strips, TRANSPOSED: row = test point, so that vfe_jcov_kernel's tile
// products read both operands along rows, as batch_jcov_kernel reads V.  A lane holds four consecutive pseudo-point rows of one test point: 32 contiguous bytes
// of a strip row.  The stores go from registers to global memory and touch no LDS, so they stand behind the existing barriers of steps 2 and 3 and add none; a
// padding test point (beyond cnt, up to the tile's 64) has a zero column of K*, so its strip rows are written as the zeros the products read.
// Compiler report for gfx950 (VGPR / AGPR / LDS / scratch): <false> 150 / 0 / 143 360 B / 0; <true> 256 / 0 / 147 968 B / 0; <false, true> 155 / 0 / 143 360 B / 0.
// the accumulators of vfe_tri_mm into a strip whose row 0 is the tile's first test point: strip[16 cb + r][16 bi + 4 g + e]
__device__ __forceinline__ void vfe_strip_store(const d4_t (&acc)[4], double* __restrict__ strip, long ld, int nb16, int w, int lane) {
    double* row = strip + (long)(16 * (w & 3) + (lane & 15)) * ld + 4 * (lane >> 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int bi = (w >> 2) + 2 * q;
        if (bi < nb16)
#pragma unroll
            for (int e = 0; e < 4; ++e) row[16 * bi + e] = acc[q][e];
    }
}
static_assert(8 * BATCH_MAXD * VT <= VFE_MAXM * KBS, "the contraction's partial sums of one side fit in the tile buffer");
static_assert((long)VFE_MAXM * (VFE_MAXM + 16) < (1L << 31), "the strip index of step 5 (below np · batch_ld(np)) is formed in 32 bits");
// Step 7 of vfe_predict_kernel<true>.  On entry every wave may read KB (U* where dv); on exit KB is free again.
__device__ __forceinline__ void vfe_pgrad_contract(const VfeProb& P, const VfePSeg& S, const double* __restrict__ z, const double* __restrict__ xs, double* KB,
                                                   const double* al, double* __restrict__ res, int t0, bool dm, bool dv, int tid, int lane, int w) {
    const int m = P.m, d = P.d, nscale = P.nscale, ns = S.ns;
    const bool valid = t0 + lane < S.cnt;
    const long j = (long)S.row0 + t0 + lane;
    double xj[BATCH_MAXD], gm[BATCH_MAXD], gv[BATCH_MAXD];
#pragma unroll
    for (int p = 0; p < BATCH_MAXD; ++p) {
        xj[p] = (p < d && valid) ? (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * xs[(long)p * ns + j] : 0.0;
        gm[p] = gv[p] = 0.0;
    }
#pragma unroll 1
    for (int i = w; i < m; i += 8) {  // wave-uniform; one body at a time: two would not fit the registers beside the 2 × 16 sums
        double t[BATCH_MAXD];
        batch_diff(z, m, d, i, xj, t);
        double d2 = 0.0;
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) d2 = fma(t[p], t[p], d2);
        double kap, dk;
        kappa_and_dr2<double>(P.kind, d2, kap, dk);
        const double cm = dm ? al[i] * dk : 0.0, cv = dv ? KB[i * KBS + lane] * dk : 0.0;
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) {
            gm[p] = fma(cm, t[p], gm[p]);
            gv[p] = fma(cv, t[p], gv[p]);
        }
    }
    __syncthreads();
    auto reduce = [&](const double (&gs)[BATCH_MAXD], long off, double f) {
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p)
            if (p < d) KB[(w * BATCH_MAXD + p) * VT + lane] = gs[p];
        __syncthreads();
        for (int e = tid; e < d * VT; e += NT) {
            const int p = e >> 6, c = e & 63;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += KB[(q * BATCH_MAXD + p) * VT + c];
            if (t0 + c < S.cnt) res[off + (long)p * ns + S.row0 + t0 + c] = f * (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * s;
        }
        __syncthreads();
    };
    if (dm) reduce(gm, S.dmean_off, -2.0 * P.variance);
    if (dv) reduce(gv, S.dvar_off, 4.0 * P.variance);
}

template <bool GRAD, bool STRIP = false>
__global__ __launch_bounds__(NT) void vfe_predict_kernel(const double* __restrict__ in, const double* __restrict__ ws, double* __restrict__ res, int nw,
                                                         const VfeProb* __restrict__ vps, const VfePred* __restrict__ pps, const VfePSeg* __restrict__ segs) {
    constexpr int WKS = GRAD ? 17 : 16, WBS = 16 * WKS;  // W's blocks: doubles between k rows, and per block
    __shared__ double Wt[(VFE_MAXM / 16) * (VFE_MAXM / 16 + 1) / 2 * WBS];
    __shared__ double KB[VFE_MAXM * KBS];
    __shared__ double al[VFE_MAXM];
    __shared__ double nrm[2][2][VT];  // [B*, C*][row parity][test point]
    const VfePSeg S = segs[blockIdx.x];
    const VfeProb& P = vps[S.prob];
    if (res[nw + P.slot] != 0.0) return;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int m = P.m, np = P.np, d = P.d, nscale = P.nscale, ns = S.ns;
    const long ld = P.ld;
    const int nb16 = np / 16;
    const bool want_mean = S.mean_off >= 0, want_var = S.var_off >= 0;
    const bool want_dmean = GRAD && S.dmean_off >= 0, want_dvar = GRAD && S.dvar_off >= 0;
    const bool chain = STRIP || want_var || want_dvar;  // the products of steps 2 and 3
    // the two strips of the problem from this segment's first row on (the memory is the workspace's: const only in this kernel's other variants)
    double* __restrict__ Bs = STRIP ? const_cast<double*>(ws) + pps[S.prob].bs_off + (long)S.row0 * ld : nullptr;
    double* __restrict__ Cs = STRIP ? const_cast<double*>(ws) + pps[S.prob].cs_off + (long)S.row0 * ld : nullptr;
    const double* __restrict__ z = in + P.z_off;
    const double* __restrict__ xs = in + S.xs_off;
    const double* __restrict__ U = ws + (chain ? pps[S.prob].u_off : 0);
    if (chain) vfe_load_wt<WKS>(Wt, ws + P.w_off, ld, nb16, w, lane);
    if ((want_mean || want_dmean) && tid < np) al[tid] = tid < m ? res[P.alpha_off + tid] : 0.0;
    __syncthreads();
    for (int t0 = 0; t0 < S.cnt; t0 += VT) {
        const bool valid = t0 + lane < S.cnt;
        const long j = (long)S.row0 + t0 + lane;
        // ---- 1. K* into LDS, the mean off it
        {
            double xj[BATCH_MAXD];
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p)
                xj[p] = (p < d && valid) ? (nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p]) * xs[(long)p * ns + j] : 0.0;
            for (int rr = 0; rr < (!GRAD || want_mean || chain ? np / 8 : 0); ++rr) {  // the gradient of the mean alone needs no K*
                const int i = w + 8 * rr;  // wave-uniform
                double v = 0.0;
                if (i < m && valid) {
                    double t[BATCH_MAXD];
                    batch_diff(z, m, d, i, xj, t);
                    v = vfe_kval(P, t);
                }
                KB[i * KBS + lane] = v;
            }
        }
        __syncthreads();
        if (want_mean && w == 0 && valid) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) s = fma(KB[i * KBS + lane], al[i], s);
            res[S.mean_off + j] = S.pm_off >= 0 ? in[S.pm_off + j] + s : s;
        }
        if (!chain) {
            __syncthreads();  // the next tile's K*, or the contraction's sums, wait for the mean's reads
        } else {
            // ---- 2. B* = W K* over K*, its column norms
            d4_t accb[4], acc[4];
            double sq = vfe_tri_mm(accb, KB, nb16, w, lane, [&](int bi, int bk, int k) { return Wt[(bi * (bi + 1) / 2 + bk) * WBS + k * WKS + r]; });
            sq += __shfl_xor(sq, 16, 64);
            sq += __shfl_xor(sq, 32, 64);
            __syncthreads();
            vfe_tri_store(accb, KB, nb16, w, lane);
            if (g == 0) nrm[0][w >> 2][16 * (w & 3) + r] = sq;
            if (STRIP) vfe_strip_store(accb, Bs + (long)t0 * ld, ld, nb16, w, lane);
            __syncthreads();
            // ---- 3. C* = E B*: the column norms alone
            sq = vfe_tri_mm(acc, KB, nb16, w, lane, [&](int bi, int bk, int k) { return U[(long)(16 * bk + k) * ld + 16 * bi + r]; });
            sq += __shfl_xor(sq, 16, 64);
            sq += __shfl_xor(sq, 32, 64);
            if (g == 0) nrm[1][w >> 2][16 * (w & 3) + r] = sq;
            if (STRIP) vfe_strip_store(acc, Cs + (long)t0 * ld, ld, nb16, w, lane);
            __syncthreads();
            // ---- 4. the variance
            if (want_var && w == 0 && valid) res[S.var_off + j] = (P.variance - (nrm[0][0][lane] + nrm[0][1][lane])) + (nrm[1][0][lane] + nrm[1][1][lane]);
            if (want_dvar) {
                // ---- 5. C* over B*, D* = B* − Eᵀ C* over C*
                vfe_tri_store(acc, KB, nb16, w, lane);
                __syncthreads();
                // The index is formed in 32 bits on purpose: with 64-bit row offsets the kernel, which sits at the 256 registers a lane of an eight-wave
                // workgroup has, spilled two doubles to scratch.  It stays below np · ld <= 128 · batch_ld(128).
                vfe_triu_mm(acc, KB, nb16, w, lane, [&](int bi, int bk, int k) { return U[(16 * bi + r) * (int)ld + 16 * bk + k]; });
#pragma unroll
                for (int q = 0; q < 4; ++q) accb[q] -= acc[q];
                __syncthreads();
                vfe_tri_store(accb, KB, nb16, w, lane);
                __syncthreads();
                // ---- 6. U* = Wᵀ D* over D*
                vfe_triu_mm(acc, KB, nb16, w, lane, [&](int bi, int bk, int k) { return Wt[(bk * (bk + 1) / 2 + bi) * WBS + r * WKS + k]; });
                __syncthreads();
                vfe_tri_store(acc, KB, nb16, w, lane);
                __syncthreads();
            }
        }
        // ---- 7. the contraction with ∂k/∂x*
        if (want_dmean || want_dvar) vfe_pgrad_contract(P, S, z, xs, KB, al, res, t0, want_dmean, want_dvar, tid, lane, w);
    }
}

// ---- the joint predictive distribution of many small sparse GPs (gp_vfe_joint_batch): vfe_jcov_kernel, then batch_jfact_kernel ----------------------------------
// Launched behind vfe_predict_kernel<false, true>, whose two strips per problem hold B* = L_z⁻¹ K_z* and C* = L_D⁻¹ B* with row = test point.  The 64×64 tile
// (ti >= tj) of the ns × ns matrix of one problem (GradTile: prob = its JointProb), four waves with one 32×32 wave tile each, in the contract of batch_jcov_kernel:
//   acc = K(x*_I, x*_J) evaluated from the packed test points through LDS (the scale applied at the load, as the other sparse kernels do; identity where a point
//   lies beyond ns), then acc −= B_I B_Jᵀ over the np / 64 blocks of the first strip and acc += C_I C_Jᵀ over those of the second, by mfma_tile_k64 in its two
//   signs: (K** − B Bᵀ) + C Cᵀ, the order of gp_vfe_predict's bit 2 and of the oracle.
// Stored twice: into the covariance output, the tile and its mirror image (the wave tile on the diagonal computes the pairs j <= i only: both triangles hold
// the same bits by construction), and with Σy* on the diagonal into the joint slice (batch_slice(ns) layout) that batch_jfact_kernel factors; the workgroups of
// the tiles (ti, 0) also write the carried row δ* = y* − mean (the mean vfe_predict_kernel wrote includes m(x*)) and the 31 zero rows behind it.
// Placement of the operands: the two panels of a tile (2 × 64 × np doubles from each strip, np <= 128: at most 256 KB) are read as register fragments straight
// from global memory — sixteen consecutive doubles of a strip row per lane and 64-wide k block, 128 B — and not staged in LDS: every panel is read by at most
// ns / 64 <= 16 workgroups of the same problem, launched next to each other, so it stays in L2, and a wave reads each entry of its operands exactly once (nothing
// to reuse inside the workgroup but the two waves that share a row or a column panel).  The LDS placement was not built and not measured.
// Only what this call wrote is read: the strips have every row up to ns rounded up to 64 (zeros from ns on).  A failed fit: NaN in the covariance; the joint
// slice is not written (batch_jfact_kernel does not read it then).  No atomics, no waits; every sum runs in an order np alone fixes.
// Compiler report for gfx950 (VGPR / AGPR / LDS / scratch): 145 / 32 / 33 280 B / 0.
__global__ __launch_bounds__(GNT) void vfe_jcov_kernel(const double* __restrict__ in, double* __restrict__ ws, double* __restrict__ res, int nw,
                                                      const VfeProb* __restrict__ vps, const JointProb* __restrict__ jps, const GradTile* __restrict__ tiles) {
    __shared__ double Kt[BT * BTS];
    const GradTile& T = tiles[blockIdx.x];
    const JointProb& J = jps[T.prob];
    const VfeProb& P = vps[J.prob];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = J.ns, nsp = J.nsp, d = P.d, nscale = P.nscale;
    const long lds = batch_ld(nsp);
    const bool diag = T.ti == T.tj;
    double* __restrict__ cov = J.cov_off >= 0 ? res + J.cov_off : nullptr;
    double* __restrict__ S = J.js_off >= 0 ? ws + J.js_off : nullptr;
    if (res[nw + J.slot] != 0.0) {
        for (int e = tid; e < BT * BT && cov; e += GNT) {
            const int gi = T.ti * BT + (e >> 6), gj = T.tj * BT + (e & 63);
            if (gi < ns && gj < ns) cov[gj + (long)gi * ns] = cov[gi + (long)gj * ns] = __builtin_nan("");
        }
        return;
    }
    if (S && T.tj == 0) {  // the carried row and the zero rows of the trailing update's 32-row tiles
        const double* mean = res + J.mean_off;
        for (int e = tid; e < BT * 32; e += GNT) {
            const int r = e >> 6, j = T.ti * BT + (e & 63);
            S[(long)(nsp + r) * lds + j] = (r == 0 && j < ns && J.ysd_off >= 0) ? in[J.ysd_off + j] - mean[j] : 0.0;
        }
    }
    {  // K(x*_I, x*_J) into LDS: lane = column with its scaled inputs in registers, the four waves interleave the rows (wave-uniform: the row's inputs by scalar loads)
        const double* __restrict__ xs = in + J.xs_off;
        const int gj = T.tj * BT + lane;
        double sc[BATCH_MAXD], xj[BATCH_MAXD];
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) {
            sc[p] = nscale == 0 ? 1.0 : P.scale[nscale == 1 ? 0 : p];
            xj[p] = (p < d && gj < ns) ? sc[p] * xs[(long)p * ns + gj] : 0.0;
        }
        for (int rr = 0; rr < BT / 4; ++rr) {
            const int li = w + 4 * rr, gi = T.ti * BT + li;
            double v;
            if (gi >= ns || gj >= ns) {
                v = (gi == gj) ? 1.0 : 0.0;
            } else {
                double t[BATCH_MAXD];
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) t[p] = p < d ? sc[p] * xs[(long)p * ns + gi] - xj[p] : 0.0;
                v = vfe_kval(P, t);
            }
            Kt[li * BTS + lane] = v;
        }
    }
    __syncthreads();
    const int wi = w >> 1, wj = w & 1;
    if (diag && wj > wi) return;  // the wave tile strictly above the diagonal: its mirror image computes it
    const int i0 = T.ti * BT + 32 * wi, c0 = T.tj * BT + 32 * wj, r = lane & 15;  // c0 <= i0
    d4_t acc[2][2];
    acc_load(acc, Kt, 32 * wi, 32 * wj, BTS, lane);
    if (i0 < ns) {  // beyond ns the rows of both strips are zero: the identity stays
        const double* __restrict__ Bs = ws + J.v_off;
        const double* __restrict__ Cs = ws + J.c_off;
        for (int k0 = 0; k0 < P.np; k0 += BT) mfma_tile_k64<true>(acc, Bs, i0, Bs, c0, k0, P.ld, lane);
        for (int k0 = 0; k0 < P.np; k0 += BT) mfma_tile_k64<false>(acc, Cs, i0, Cs, c0, k0, P.ld, lane);
    }
    const bool lower_only = diag && wi == wj;  // the wave tile on the diagonal: the pairs j <= i, mirrored
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int hj = 0; hj < 2; ++hj) {
            const int gj = c0 + 16 * hj + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = i0 + 16 * hi + Tr<double>::crow(lane, q);
                if (lower_only && gj > gi) continue;
                const double v = acc[hi][hj][q];
                if (cov && gi < ns && gj < ns) {
                    cov[gj + (long)gi * ns] = v;
                    if (gi != gj) cov[gi + (long)gj * ns] = v;
                }
                if (S) {
                    const double nz = (gi == gj && gi < ns) ? (J.nzs_off >= 0 ? in[J.nzs_off + gi] : J.noise_s) : 0.0;
                    S[(long)gi * lds + gj] = v + nz;
                    if (diag && gi != gj) S[(long)gj * lds + gi] = v;  // the whole diagonal block is loaded into LDS by the factorisation
                }
            }
        }
}

}  // namespace gpmi

using namespace gpmi;

namespace {

struct BatchArgs {
    int32_t nb;
    const gp_kernel* k;   // single-kind call
    const gp_ksum* ks;    // composite call
    int32_t nx;
    const gp_points* x;
    const gp_noise* noise;
    const void* const* mean;
    int32_t ny;
    const void* const* y;
    void* logpdf_out;
    int32_t* info_out;
    void* const* alpha_out;
    int dtype;
    const gp_points& xb(int b) const { return x[nx == 1 ? 0 : b]; }
    const void* yb(int b) const { return y[ny == 1 ? 0 : b]; }
    const void* mb(int b) const { return mean ? mean[b] : nullptr; }
    void* ab(int b) const { return alpha_out ? alpha_out[b] : nullptr; }
};

// The leading arguments of every entry point.  The kernel array goes to the field of its type, so the two entry points of a pair build their arguments with
// the same text and differ in the type of `k` alone.
void set_kernels(BatchArgs& a, const gp_kernel* k) { a.k = k; }
void set_kernels(BatchArgs& a, const gp_ksum* ks) { a.ks = ks; }
template <class K>
BatchArgs base_args(int32_t nb, const K* k, int32_t nx, const gp_points* x, const gp_noise* noise, const void* const* mean, int32_t ny, const void* const* y,
                    void* logpdf_out, int32_t* info_out, void* const* alpha_out = nullptr) {
    BatchArgs a{nb, nullptr, nullptr, nx, x, noise, mean, ny, y, logpdf_out, info_out, alpha_out, 0};
    set_kernels(a, k);
    return a;
}

// a size limit of the header; the environment variable read at the call site overrides it for measurements (0 … what the kernels admit)
long env_capped(const char* env, long deflt, long cap = BATCH_KERNEL_MAX_N) { return std::max(0L, std::min<long>(env ? atol(env) : deflt, cap)); }
void fill_nan(void* out, int dtype, long n) {
    if (!out) return;
    if (dtype == 0) std::fill_n((double*)out, n, std::numeric_limits<double>::quiet_NaN());
    else std::fill_n((float*)out, n, std::numeric_limits<float>::quiet_NaN());
}

// x of one problem, dimension-major [d][n], raw (the kernel applies the transform to the differences)
void pack_points(const gp_points& x, double* out) {
    const double* p = (const double*)x.data;
    const long n = x.n;
    for (int dd = 0; dd < x.d; ++dd) {
        double* o = out + (size_t)dd * n;
        if (x.layout == 1)
            for (long i = 0; i < n; ++i) o[i] = p[(long)dd + i * x.d];
        else
            std::memcpy(o, x.layout == 0 ? p : p + (long)dd * n, sizeof(double) * n);
    }
}

void put_result(const BatchArgs& a, int b, double lp, int32_t info) {
    if (a.logpdf_out) put(a.logpdf_out, a.dtype, b, lp);  // gp_predict_batch may leave it out
    a.info_out[b] = info;
}

// the logpdf entry of problem b for the single path, zeroed (NULL where gp_predict_batch was given no logpdf_out)
void* logpdf_slot(const BatchArgs& a, int b) {
    if (!a.logpdf_out) return nullptr;
    put(a.logpdf_out, a.dtype, b, 0);
    return (char*)a.logpdf_out + (a.dtype == 0 ? 8 : 4) * (size_t)b;
}

// `len` doubles of a packed buffer whose next free offset is `top`: where they start
long take(long& top, long len) { return std::exchange(top, top + len); }

// An array that every problem brings, or that all of them share (count == 1): the shared one is laid out, and filled, once.
struct SharedOnce {
    bool shared, seen = false;
    long off = -1;
    bool claim() { return !(shared && std::exchange(seen, true)); }  // true for the problem that is to lay out / write the array: every one, or the first
    long place(long& top, long len) { return claim() ? off = take(top, len) : off; }  // layout: the problem's offset, `len` doubles taken at `top` by the claimant
};

// The packed input of one wave (doubles): descriptors | composite kernels | x | y | means | noise vectors, then whatever the caller appends at `off`;
// `ws` counts the slices, `roff` the result buffer (logpdf and failure column of every problem, then the α vectors).
struct WaveLayout {
    std::vector<BatchProb> pr;  // in the order of idx
    std::vector<int> order;     // the descriptors as they lie on the device: the widest problems first (the last workgroups to start are the shortest)
    std::vector<int> pos;       // the inverse of order: where the descriptor of problem t lies
    long off = 0, ws = 0, roff = 0;
};

// descriptors and offsets of the problems idx[0..nw); want_alpha(b): α of problem b goes to the result buffer
template <class F> void wave_layout(const BatchArgs& a, const int* idx, int nw, F&& want_alpha, WaveLayout& L) {
    std::vector<BatchProb>& pr = L.pr;
    pr.assign((size_t)nw, BatchProb{});
    long &off = L.off, &ws = L.ws, &roff = L.roff;
    off = (long)((size_t)nw * sizeof(BatchProb) / 8), ws = 0, roff = 2L * nw;
    const long ksd = (long)((sizeof(KSum) + 7) / 8);
    SharedOnce xo{a.nx == 1}, yo{a.ny == 1};
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& x = a.xb(b);
        BatchProb& p = pr[t];
        p.n = (int)x.n;
        p.np = (int)batch_np(x.n);
        p.ld = (int)batch_ld(p.np);
        p.d = x.d;
        p.slot = t;
        p.a_off = take(ws, batch_slice(x.n));
        p.ks_off = a.ks ? take(off, ksd) : -1;
        if (!a.ks) {
            const gp_kernel& k = a.k[b];
            p.kind = k.kind;
            p.nscale = k.nscale;
            p.variance = k.variance;
            for (int q = 0; q < k.nscale; ++q) p.scale[q] = k.scale[q];
        }
        p.x_off = xo.place(off, (long)x.d * x.n);
        p.y_off = yo.place(off, x.n);
        p.m_off = a.mb(b) ? take(off, x.n) : -1;
        p.noise_s = a.noise[b].s;
        p.nz_off = a.noise[b].kind == 1 ? take(off, x.n) : -1;
        p.alpha_off = want_alpha(b) ? take(roff, x.n) : -1;
    }
    L.order.resize((size_t)nw);
    for (int t = 0; t < nw; ++t) L.order[t] = t;
    std::stable_sort(L.order.begin(), L.order.end(), [&](int u, int v) { return pr[u].n > pr[v].n; });
    L.pos.resize((size_t)nw);
    for (int s = 0; s < nw; ++s) L.pos[L.order[s]] = s;
}

// fills the packed input of a laid-out wave: the descriptors in L.order, then every problem's data
void wave_fill(const BatchArgs& a, const std::vector<KSum>& packed, const int* idx, int nw, const WaveLayout& L, double* hin) {
    for (int t = 0; t < nw; ++t) std::memcpy((char*)hin + (size_t)t * sizeof(BatchProb), &L.pr[L.order[t]], sizeof(BatchProb));
    SharedOnce xo{a.nx == 1}, yo{a.ny == 1};
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& x = a.xb(b);
        const BatchProb& p = L.pr[t];
        if (a.ks) std::memcpy(hin + p.ks_off, &packed[b], sizeof(KSum));
        if (xo.claim()) pack_points(x, hin + p.x_off);
        if (yo.claim()) std::memcpy(hin + p.y_off, a.yb(b), sizeof(double) * x.n);
        if (p.m_off >= 0) std::memcpy(hin + p.m_off, a.mb(b), sizeof(double) * x.n);
        if (p.nz_off >= 0) std::memcpy(hin + p.nz_off, a.noise[b].diag, sizeof(double) * x.n);
    }
}

// Host and device memory of one wave: page-locked staging for both directions (pageable above the staging limit; packed input, then results) and the three
// device blocks, which return to the ctx cache with the wave.
struct WaveMem {
    gp_ctx* c;
    DevBufs bufs;
    std::vector<double> pageable;
    double *hin = nullptr, *hout = nullptr, *ws = nullptr, *res = nullptr;
    const double* in = nullptr;
    size_t in_bytes = 0, out_bytes = 0;
    explicit WaveMem(gp_ctx* c_) : c(c_), bufs(c_) {}
    int32_t alloc(long in_doubles, long ws_doubles, long out_doubles) {
        in_bytes = sizeof(double) * (size_t)in_doubles;
        out_bytes = sizeof(double) * (size_t)out_doubles;
        hin = (double*)ctx_pinned(c, in_bytes + out_bytes);
        if (!hin) {
            pageable.resize((size_t)(in_doubles + out_doubles));
            hin = pageable.data();
        }
        hout = hin + in_doubles;
        void *i = nullptr, *w = nullptr, *r = nullptr;
        RC(bufs.get(in_bytes, &i));
        RC(bufs.get(sizeof(double) * (size_t)ws_doubles, &w));
        RC(bufs.get(out_bytes, &r));
        in = (const double*)i, ws = (double*)w, res = (double*)r;
        return 0;
    }
    int32_t upload() {
        HIPCHK(hipMemcpyAsync((void*)in, hin, in_bytes, hipMemcpyHostToDevice, c->sm));
        return 0;
    }
    int32_t download_and_sync() {
        HIPCHK(hipMemcpyAsync(hout, res, out_bytes, hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        return 0;
    }
};

// A table the kernels of a wave read from its packed input: the host vector, its place behind whatever L.off has reached (the order of the place() calls is
// the order of the tables in the buffer), its copy into the staging buffer and its address on the device, from entry `first` on.
template <class T> struct Table {
    static_assert(sizeof(T) % 8 == 0, "the tables are packed behind double data");
    std::vector<T> v;
    long off = -1;
    void place(WaveLayout& L) { off = take(L.off, (long)(v.size() * sizeof(T) / 8)); }
    void fill(const WaveMem& m) const {
        if (!v.empty()) std::memcpy(m.hin + off, v.data(), v.size() * sizeof(T));
    }
    const T* dev(const WaveMem& m, size_t first = 0) const { return reinterpret_cast<const T*>(m.in + off) + first; }
};

// One launch of a wave on the ctx's main stream.  Every kernel takes (in, ws, res, nw) in front; W and R are double or const double as the kernel declares
// them, and the trailing arguments are converted to the kernel's own parameter types (hipLaunchKernelGGL deduces them twice and wants them equal).
template <class W, class R, class... P, class... A>
int32_t launch(const WaveMem& m, void (*kern)(const double*, W*, R*, int, P...), size_t grid, unsigned block, int nw, A... rest) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), 0, m.c->sm, m.in, static_cast<W*>(m.ws), static_cast<R*>(m.res), nw, static_cast<P>(rest)...);
    HIPCHK(hipGetLastError());
    return 0;
}
// The <SUM> dispatch of each kernel stands in one place (ks: the call brought composite kernels): here for the two kernels that several waves launch, at the
// one launch site of every other.
int32_t launch_fit(const WaveMem& m, bool ks, int nw) { return launch(m, ks ? batch_logpdf_kernel<true> : batch_logpdf_kernel<false>, nw, NT, nw); }
// lps: the LooProb table of a gp_loo_grad_batch wave (the weights of the leave-one-out objective), or NULL (those of logpdf)
int32_t launch_grad(const WaveMem& m, bool ks, int nw, const GradProb* gps, const Table<GradTile>& tiles, const LooProb* lps = nullptr) {
    auto kern = lps ? (ks ? batch_grad_kernel<true, true> : batch_grad_kernel<false, true>) : (ks ? batch_grad_kernel<true, false> : batch_grad_kernel<false, false>);
    return launch(m, kern, tiles.v.size(), GNT, nw, gps, tiles.dev(m), lps);
}

// one launch: the problems idx[0..nw) of the call, all taken by the kernel.  Caller holds the ctx lock.
int32_t run_wave(gp_ctx* c, const BatchArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [&](int b) { return a.ab(b) != nullptr; }, L);
    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        return m.download_and_sync();
    }));
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, m.hout[t], (int32_t)m.hout[nw + t]);
        if (L.pr[t].alpha_off >= 0) std::memcpy(a.ab(b), m.hout + L.pr[t].alpha_off, sizeof(double) * L.pr[t].n);
    }
    return 0;
}

// the arguments gp_logpdf_batch and gp_predict_batch share (nb > 0): the arrays, their counts and the y pointers
int32_t check_batch_head(const BatchArgs& a) {
    if (!a.k && !a.ks) return set_arg_err(3, "kernel array is NULL");
    if (a.nx != 1 && a.nx != a.nb) return set_arg_err(4, "nx must be 1 (one x shared by every problem) or nb");
    if (!a.x) return set_arg_err(5, "points array is NULL");
    if (!a.noise) return set_arg_err(6, "noise array is NULL");
    if (a.ny != 1 && a.ny != a.nb) return set_arg_err(8, "ny must be 1 (one y shared by every problem) or nb");
    if (!a.y) return set_arg_err(9, "y array is NULL");
    for (int b = 0; b < a.ny; ++b)
        if (!a.y[b]) return set_arg_err(9, "a y pointer is NULL");
    return 0;
}

// every problem's descriptor, points and noise; sets the call's dtype and packs the composite kernels
int32_t check_batch_problems(BatchArgs& a, std::vector<KSum>& packed) {
    a.dtype = a.ks ? a.ks[0].dtype : a.k[0].dtype;
    packed.resize(a.ks ? (size_t)a.nb : 0);
    for (int b = 0; b < a.nb; ++b) {
        const gp_points& x = a.xb(b);
        RC(check_points(&x, 5));
        if (a.ks) {
            gp_kernel kid;
            RC(pack_ksum(&a.ks[b], x.d, 3, packed[b], kid));
        } else {
            RC(check_kernel(&a.k[b], x.d, 3));
        }
        if ((a.ks ? a.ks[b].dtype : a.k[b].dtype) != a.dtype) return set_arg_err(3, "every descriptor of one batch call carries the same dtype");
        RC(check_noise(&a.noise[b], 6, true));
        if (a.ny == 1 && x.n != a.xb(0).n) return set_arg_err(8, "a shared y needs problems of one size");
    }
    return 0;
}

// which path serves a problem depends on that problem alone
bool batch_takes(const BatchArgs& a, int b, long max_n) {
    const gp_points& x = a.xb(b);
    return a.dtype == 0 && a.noise[b].kind <= 1 && x.n <= max_n && x.d <= BATCH_MAXD;
}

// the path of a problem depends on that problem alone: the kernels' (mine) or the single path's (routed)
void split_by_path(const BatchArgs& a, long max_n, std::vector<int>& mine, std::vector<int>& routed) {
    for (int b = 0; b < a.nb; ++b) (batch_takes(a, b, max_n) ? mine : routed).push_back(b);
}

// workspace bytes of one problem: `own` adds up over a wave, `shared` is needed once per wave, as wide as the widest problem asks for; `in`: the bytes the problem
// alone adds to the wave's packed input, where they are not small beside its workspace (gp_vfe_batch: n reaches 262 144; gp_vfe_grad_batch adds the n-long results it stages back) — they add up against the staging limit
struct WaveCost { size_t own, shared, in = 0; };
// The kernel's problems in waves bounded by the launch size and by the workspace budget (a wave holds at least one problem); run(idx, nw) serves one wave.
template <class Cost, class Run> int32_t for_each_wave(gp_ctx* c, const std::vector<int>& mine, Cost&& cost, Run&& run) {
    if (mine.empty()) return 0;
    HIPCHK(hipSetDevice(c->device));
    for (size_t i = 0, j; i < mine.size(); i = j) {
        size_t own = 0, shared = 0, in = 0;
        for (j = i; j < mine.size() && j - i < BATCH_WAVE_PROBLEMS; ++j) {
            const WaveCost w = cost(mine[j]);
            if (j > i && (own + w.own + std::max(shared, w.shared) > BATCH_WS_BYTES || in + w.in > BATCH_IN_BYTES)) break;
            own += w.own;
            in += w.in;
            shared = std::max(shared, w.shared);
        }
        RC(run(mine.data() + i, (int)(j - i)));
    }
    return 0;
}

// The single path's fit of problem b, by the kind of the call's descriptors (the routed loops: their calls take the ctx lock themselves).
int32_t routed_fit(gp_ctx* c, const BatchArgs& a, int b, gp_post** post, void* alpha, void* lp) {
    return a.ks ? gp_posterior_fit_sum(c, &a.ks[b], &a.xb(b), &a.noise[b], a.mb(b), a.yb(b), post, alpha, lp)
                : gp_posterior_fit(c, &a.k[b], &a.xb(b), &a.noise[b], a.mb(b), a.yb(b), post, alpha, lp);
}

// What every routed loop does with the status of problem b's single-path calls: an error ends the batch call; a failed factorisation is the problem's info,
// NaN in its logpdf and, by nan_fill(), in the family's other outputs.
template <class Fill> int32_t routed_done(const BatchArgs& a, int b, int32_t rc, Fill&& nan_fill) {
    if (rc < 0) return rc;
    a.info_out[b] = rc;
    if (rc > 0) {
        put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
        nan_fill();
    }
    return 0;
}

int32_t batch_impl(gp_ctx* c, BatchArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_batch_head(a));
    if (!a.logpdf_out) return set_arg_err(10, "logpdf_out is NULL");
    if (!a.info_out) return set_arg_err(11, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    std::vector<int> mine, routed;
    split_by_path(a, env_capped(getenv("GPMI_BATCH_MAX_N"), GPMI355_BATCH_MAX_N), mine, routed);
    RC(for_each_wave(c, mine, [&](int b) { return WaveCost{sizeof(double) * (size_t)batch_slice(a.xb(b).n), 0}; },
                     [&](const int* idx, int nw) { return run_wave(c, a, packed, idx, nw); }));
    // everything else: the single path, one problem at a time.  Each of those calls takes the ctx lock itself (std::mutex is not recursive): it is released
    // here; the ctx stays pinned by the Guard, and every call validates it again.
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        int32_t rc;
        void* lp = logpdf_slot(a, b);
        if (a.ab(b)) {
            gp_post* post = nullptr;
            rc = routed_fit(c, a, b, &post, a.ab(b), lp);
            if (post) (void)gp_posterior_free(post);
        } else {
            rc = a.ks ? gp_logpdf_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), x.n, 1, lp)
                      : gp_logpdf(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), x.n, 1, lp);
        }
        RC(routed_done(a, b, rc, [&] { fill_nan(a.ab(b), a.dtype, x.n); }));
    }
    return 0;
}

// ---- gp_predict_batch / gp_predict_batch_sum -----------------------------------------------------------------------------------------------------------
struct PredictArgs : BatchArgs {
    int32_t nxs;
    const gp_points* xs;
    const void* const* pm;  // m(x*) per problem, or NULL
    int32_t what;           // 1 mean | 2 var
    void* const* mean_out;
    void* const* var_out;
    // gp_predict_grad_batch / _sum only (grad): the gradient arrays; there each of the four arrays may be NULL, not both of a side that is asked for
    bool grad = false;
    void* const* dmean_out = nullptr;
    void* const* dvar_out = nullptr;
    const gp_points& xsb(int b) const { return xs[nxs == 1 ? 0 : b]; }
    const void* pmb(int b) const { return pm ? pm[b] : nullptr; }
    void* out_b(void* const* arr, int side, int b) const { return (arr && (what & side)) ? arr[b] : nullptr; }
    bool want_dmean() const { return grad && (what & 1) && dmean_out; }
    bool want_dvar() const { return grad && (what & 2) && dvar_out; }
};

// nxs and xs of a call over test points (arguments 10 and 11 in every exact family, `arg` and arg + 1 in gp_vfe_predict_batch)
template <class A> int32_t check_test_head(const A& a, int arg = 10) {
    if (a.nxs != 1 && a.nxs != a.nb) return set_arg_err(arg, "nxs must be 1 (one xs shared by every problem) or nb");
    if (!a.xs) return set_arg_err(arg + 1, "test points array is NULL");
    return 0;
}
// An array of per-problem pointers of such a call: a problem with test points needs its entry where the call asks for the array (wanted) and brought it.
struct PointerArray {
    const void* const* arr;
    bool wanted;
    int arg;
    const char* msg;
};
// every problem's test points, Σy* (gp_joint_batch: argument 13, gp_vfe_joint_batch: 17, else NULL) and entries of `arrays`, in that order
template <class A> int32_t check_test_points(const A& a, const gp_noise* noise_xs, std::initializer_list<PointerArray> arrays, int arg = 11, int nz_arg = 13) {
    for (int b = 0; b < a.nb; ++b) {
        const gp_points& xs = a.xsb(b);
        if (xs.n < 0) return set_arg_err(arg, "xs: n must be >= 0");
        if (xs.n == 0) continue;  // no test points: nothing of this problem's xs or outputs is touched
        RC(check_points(&xs, arg));
        if (xs.d != a.xb(b).d) return set_arg_err(arg, "xs has a different D than the training inputs");
        if (noise_xs) RC(check_noise(&noise_xs[b], nz_arg, true));
        for (const PointerArray& p : arrays)
            if (p.wanted && p.arr && !p.arr[b]) return set_arg_err(p.arg, p.msg);
    }
    return 0;
}

// The test points of a wave and the predict launches over them, for gp_predict_batch, gp_predict_grad_batch and gp_joint_batch: behind the fit's input the
// points (dimension-major, a shared set once) and the table of tiles of TP points; behind its results mean and variance of every problem.
struct TestPoints {
    std::vector<long> xs_off, mean_off, var_off;
    Table<BatchTile> tiles;
    std::vector<size_t> launch_end;  // a predict launch closes at BATCH_PRED_TILES tiles
    SharedOnce xso, xsf;             // layout, filling
    bool want_var;                   // the variance, and with it a strip of TP rows per tile
    TestPoints(const PredictArgs& a, int nw, bool want_var_)
        : xs_off((size_t)nw, -1), mean_off((size_t)nw, -1), var_off((size_t)nw, -1), xso{a.nxs == 1}, xsf{a.nxs == 1}, want_var(want_var_) {}

    // offsets of the problems with test points, in the order of idx; rest(t) lays out what else problem t brings or returns
    template <class Rest> void place(const PredictArgs& a, const int* idx, int nw, bool want_mean, WaveLayout& L, Rest&& rest) {
        for (int t = 0; t < nw; ++t) {
            const gp_points& xs = a.xsb(idx[t]);
            if (xs.n == 0) continue;
            xs_off[t] = xso.place(L.off, (long)xs.d * xs.n);
            if (want_mean) mean_off[t] = take(L.roff, xs.n);
            if (want_var) var_off[t] = take(L.roff, xs.n);
            rest(t);
        }
    }

    // The tiles, the widest problems first, their strips behind L.ws, and the table's place.  share: the launches of a wave run one after the other on one
    // stream, so every launch group starts over at the same strips, and a group also closes when its strips would pass the workspace budget
    // (gp_predict_batch, gp_predict_grad_batch).  Otherwise every tile keeps a strip of its own and after(t, first) — first: the strip of the problem's first
    // tile — may take what follows the problem's strips (gp_joint_batch, whose later kernels read them).
    template <class After> void tile(const PredictArgs& a, const int* idx, int nw, bool share, WaveLayout& L, After&& after) {
        const long base = L.ws;
        long top = base;
        size_t launch_begin = 0;
        for (int s = 0; s < nw; ++s) {
            const int t = L.order[s];
            const long ns = a.xsb(idx[t]).n, strip = want_var ? (long)TP * L.pr[t].ld : 0, first = L.ws;
            if (ns == 0) continue;
            for (long row0 = 0; row0 < ns; row0 += TP) {
                const size_t open = tiles.v.size() - launch_begin;
                if (open > 0 && (open == BATCH_PRED_TILES || (share && sizeof(double) * (size_t)(L.ws + strip) > BATCH_WS_BYTES))) {
                    launch_end.push_back(tiles.v.size());
                    launch_begin = tiles.v.size();
                    if (share) L.ws = base;
                }
                tiles.v.push_back(BatchTile{xs_off[t], take(L.ws, strip), mean_off[t], var_off[t], L.pos[t], (int)ns, (int)row0, (int)std::min<long>(TP, ns - row0)});
                top = std::max(top, L.ws);
            }
            if (!share) after(t, first);
            top = std::max(top, L.ws);
        }
        if (tiles.v.size() > launch_begin) launch_end.push_back(tiles.v.size());
        L.ws = top;
        tiles.place(L);
    }

    void fill(const PredictArgs& a, const int* idx, int nw, const WaveMem& m) {
        for (int t = 0; t < nw; ++t) {
            const gp_points& xs = a.xsb(idx[t]);
            if (xs.n > 0 && xsf.claim()) pack_points(xs, m.hin + xs_off[t]);
        }
        tiles.fill(m);
    }

    // The predict launches.  ptiles (gp_predict_grad_batch, else NULL): batch_pgrad_kernel directly behind each of them, over the same tiles — the strips are
    // shared by the launch groups, so the gradients of a group follow its own predict launch and precede the next one.
    int32_t launch_groups(const WaveMem& m, bool ks, int nw, const Table<PGradTile>* ptiles) const {
        size_t t0 = 0;
        for (size_t t1 : launch_end) {
            RC(launch(m, ks ? batch_predict_kernel<true> : batch_predict_kernel<false>, t1 - t0, NT, nw, tiles.dev(m, t0)));
            if (ptiles) RC(launch(m, ks ? batch_pgrad_kernel<true> : batch_pgrad_kernel<false>, t1 - t0, ks ? PGNT_SUM : NT, nw, tiles.dev(m, t0), ptiles->dev(m, t0)));
            t0 = t1;
        }
        return 0;
    }

    // the mean of problem b (the t-th of the wave) to the caller, the prior mean at the test points added
    void put_mean(const PredictArgs& a, int b, int t, const double* hout) const {
        double* mo = (double*)a.out_b(a.mean_out, 1, b);
        if (!mo) return;
        const double* pm = (const double*)a.pmb(b);
        for (long j = 0; j < a.xsb(b).n; ++j) mo[j] = pm ? pm[j] + hout[mean_off[t] + j] : hout[mean_off[t] + j];
    }
};

// The S = L⁻ᵀ strip of the s-th descriptor of a wave, beside the slices, and the tiles of 128 rows batch_inv_kernel fills it by; the launch over the tiles of
// every problem of the wave that has one.
void place_s_strip(WaveLayout& L, int s, GradProb& g, Table<GradTile>& itiles) {
    const BatchProb& p = L.pr[L.order[s]];
    g.s_off = take(L.ws, (long)p.np * p.ld);
    for (int r0 = 0; r0 < p.np; r0 += TP) itiles.v.push_back(GradTile{s, r0 / TP, 0, 0});
}
int32_t launch_inv(const WaveMem& m, int nw, const Table<GradProb>& gp, const Table<GradTile>& itiles) {
    return itiles.v.empty() ? 0 : launch(m, batch_inv_kernel, itiles.v.size(), NT, nw, gp.dev(m), itiles.dev(m));
}

long predict_strip(const PredictArgs& a, long n) { return (a.what & 2) ? (long)TP * batch_ld(batch_np(n)) : 0; }  // the mean alone needs no strip

// the S strip of a problem that has a variance-side gradient and test points (beside its slice, as in a gradient wave)
long pgrad_s(const PredictArgs& a, int b) {
    const long np = batch_np(a.xb(b).n);
    return (a.want_dvar() && a.xsb(b).n > 0) ? np * batch_ld(np) : 0;
}
// one wave: the fit launch of the problems idx[0..nw), then the predict launches against the slices it leaves — for a gradient call (a.grad) S = L⁻ᵀ of the
// problems that need it in front of them, and batch_pgrad_kernel directly behind each predict launch, over the same tiles.  Caller holds the ctx lock.
int32_t run_predict_wave(gp_ctx* c, const PredictArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [&](int b) { return (a.what & 1) && a.xsb(b).n > 0; }, L);
    TestPoints tp(a, nw, (a.what & 2) != 0);
    std::vector<long> dmean_off((size_t)nw, -1), dvar_off((size_t)nw, -1);
    tp.place(a, idx, nw, (a.what & 1) != 0, L, [&](int t) {
        const gp_points& xs = a.xsb(idx[t]);
        if (a.want_dmean()) dmean_off[t] = take(L.roff, (long)xs.d * xs.n);
        if (a.want_dvar()) dvar_off[t] = take(L.roff, (long)xs.d * xs.n);
    });
    // a gradient call: the table batch_inv_kernel reads, with an S strip for the problems that need one, and a PGradTile beside every tile
    Table<GradProb> gp;
    Table<GradTile> itiles;
    Table<PGradTile> ptiles;
    gp.v.assign(a.grad ? (size_t)nw : 0, GradProb{-1, -1, -1, -1, 0, 0});
    for (int s = 0; s < nw && a.grad; ++s)
        if (pgrad_s(a, idx[L.order[s]]) != 0) place_s_strip(L, s, gp.v[s], itiles);
    tp.tile(a, idx, nw, true, L, [](int, long) {});
    if (a.grad)
        for (const BatchTile& tl : tp.tiles.v) ptiles.v.push_back(PGradTile{gp.v[tl.prob].s_off, dmean_off[L.order[tl.prob]], dvar_off[L.order[tl.prob]]});
    ptiles.place(L);
    gp.place(L);
    itiles.place(L);

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    tp.fill(a, idx, nw, m);
    ptiles.fill(m);
    gp.fill(m);
    itiles.fill(m);
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        RC(launch_inv(m, nw, gp, itiles));
        RC(tp.launch_groups(m, a.ks != nullptr, nw, a.want_dmean() || a.want_dvar() ? &ptiles : nullptr));
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    if (a.grad) c->batch_pgrad_problems += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        const long ns = a.xsb(b).n;
        if (ns == 0) continue;
        tp.put_mean(a, b, t, hout);
        if (void* vo = a.out_b(a.var_out, 2, b)) std::memcpy(vo, hout + tp.var_off[t], sizeof(double) * (size_t)ns);
        const gp_points& q = a.xsb(b);  // the gradients lie dimension-major [d][ns] in the result buffer: into the container layout of xs
        if (dmean_off[t] >= 0) grad_to_layout<double>(q.layout, ns, q.d, hout + dmean_off[t], ns, a.dmean_out[b]);
        if (dvar_off[t] >= 0) grad_to_layout<double>(q.layout, ns, q.d, hout + dvar_off[t], ns, a.dvar_out[b]);
    }
    return 0;
}

int32_t predict_batch_impl(gp_ctx* c, PredictArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_batch_head(a));
    RC(check_test_head(a));
    if (a.what <= 0 || a.what > 3) return set_arg_err(13, "what must be a combination of 1|2");
    if ((a.what & 1) && !a.mean_out) return set_arg_err(14, "mean_out is NULL");
    if ((a.what & 2) && !a.var_out) return set_arg_err(15, "var_out is NULL");
    if (!a.info_out) return set_arg_err(17, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    RC(check_test_points(a, nullptr, {{a.mean_out, (a.what & 1) != 0, 14, "a mean_out pointer is NULL"}, {a.var_out, (a.what & 2) != 0, 15, "a var_out pointer is NULL"}}));
    std::vector<int> mine, routed;
    split_by_path(a, env_capped(getenv("GPMI_BATCH_MAX_N"), GPMI355_BATCH_MAX_N), mine, routed);
    // the slices of a wave and its widest strip fit in the budget: the predict launches of a wave run one after the other and share the strips
    auto cost = [&](int b) {
        const long n = a.xb(b).n;
        return WaveCost{sizeof(double) * (size_t)batch_slice(n), a.xsb(b).n > 0 ? sizeof(double) * (size_t)predict_strip(a, n) : 0};
    };
    RC(for_each_wave(c, mine, cost, [&](const int* idx, int nw) { return run_predict_wave(c, a, packed, idx, nw); }));
    // everything else: fit, predict and free on the single path, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& xs = a.xsb(b);
        gp_post* post = nullptr;
        int32_t rc = routed_fit(c, a, b, &post, nullptr, logpdf_slot(a, b));
        if (rc == 0 && xs.n > 0)
            rc = gp_posterior_predict(post, &xs, a.pmb(b), a.what, (a.what & 1) ? a.mean_out[b] : nullptr, (a.what & 2) ? a.var_out[b] : nullptr, nullptr);
        if (post) (void)gp_posterior_free(post);
        RC(routed_done(a, b, rc, [&] {
            if (xs.n <= 0) return;
            if (a.what & 1) fill_nan(a.mean_out[b], a.dtype, xs.n);
            if (a.what & 2) fill_nan(a.var_out[b], a.dtype, xs.n);
        }));
    }
    return 0;
}

// ---- gp_predict_grad_batch / gp_predict_grad_batch_sum ---------------------------------------------------------------------------------------------------
enum { PGRAD_GROUP_TILES = 256 };  // strips a wave of gp_predict_grad_batch keeps room for: one tile per CU in a launch group at least
// NaN in every output of problem b that the call was given
void pgrad_fill_nan(const PredictArgs& a, int b) {
    const gp_points& xs = a.xsb(b);
    if (xs.n <= 0) return;
    fill_nan(a.out_b(a.mean_out, 1, b), a.dtype, xs.n);
    fill_nan(a.out_b(a.var_out, 2, b), a.dtype, xs.n);
    fill_nan(a.out_b(a.dmean_out, 1, b), a.dtype, xs.n * xs.d);
    fill_nan(a.out_b(a.dvar_out, 2, b), a.dtype, xs.n * xs.d);
}

int32_t predict_grad_batch_impl(gp_ctx* c, PredictArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_batch_head(a));
    RC(check_test_head(a));
    if (a.what <= 0 || a.what > 3) return set_arg_err(13, "what must be a combination of 1|2");
    if ((a.what & 1) && !a.mean_out && !a.dmean_out) return set_arg_err(14, "mean_out and dmean_out are both NULL");
    if ((a.what & 2) && !a.var_out && !a.dvar_out) return set_arg_err(15, "var_out and dvar_out are both NULL");
    if (!a.info_out) return set_arg_err(19, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    const bool m1 = (a.what & 1) != 0, m2 = (a.what & 2) != 0;
    RC(check_test_points(a, nullptr, {{a.mean_out, m1, 14, "a mean_out pointer is NULL"}, {a.var_out, m2, 15, "a var_out pointer is NULL"},
                                      {a.dmean_out, m1, 16, "a dmean_out pointer is NULL"}, {a.dvar_out, m2, 17, "a dvar_out pointer is NULL"}}));
    std::vector<int> mine, routed;
    split_by_path(a, env_capped(getenv("GPMI_BATCH_PGRAD_MAX_N"), GPMI355_BATCH_PGRAD_MAX_N), mine, routed);
    // The slices and S strips of a wave fit in the budget beside PGRAD_GROUP_TILES predict strips of its widest problem (W overwrites V in the strip: no second
    // one).  Room for ONE strip, as gp_predict_batch leaves it, lets a wave that fills the budget run one tile per launch group — measured here at B = 512,
    // ns = 1 024: 6.1 s at n = 1 024 against 2.4 s at n = 1 536; a group of a tile per CU keeps the chip busy.
    auto cost = [&](int b) {
        const long n = a.xb(b).n;
        return WaveCost{sizeof(double) * (size_t)(batch_slice(n) + pgrad_s(a, b)),
                        a.xsb(b).n > 0 ? sizeof(double) * (size_t)(PGRAD_GROUP_TILES * predict_strip(a, n)) : 0};
    };
    RC(for_each_wave(c, mine, cost, [&](const int* idx, int nw) { return run_predict_wave(c, a, packed, idx, nw); }));
    // everything else: fit, predict_grad and free on the single path, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& xs = a.xsb(b);
        gp_post* post = nullptr;
        int32_t rc = routed_fit(c, a, b, &post, nullptr, logpdf_slot(a, b));
        if (rc == 0 && xs.n > 0)
            rc = gp_posterior_predict_grad(post, &xs, a.pmb(b), a.what, a.out_b(a.mean_out, 1, b), a.out_b(a.var_out, 2, b), a.out_b(a.dmean_out, 1, b),
                                           a.out_b(a.dvar_out, 2, b));
        if (post) (void)gp_posterior_free(post);
        RC(routed_done(a, b, rc, [&] { pgrad_fill_nan(a, b); }));
    }
    return 0;
}

// ---- gp_joint_batch / gp_joint_batch_sum ------------------------------------------------------------------------------------------------------------------
struct JointArgs : PredictArgs {  // what: 1 mean | 4 latent covariance | 8 held-out logpdf | 16 samples; var_out is not used
    const gp_noise* noise_xs;
    void* const* cov_out;
    const void* const* ys;
    void* hlogpdf_out;
    int32_t nsamp;
    const void* const* xi;
    void* const* samples_out;
    int32_t* info_joint;
    bool want_fact() const { return (what & 24) != 0; }
    bool want_mean() const { return (what & 25) != 0; }  // the held-out logpdf and the samples are built on it
    long draws(int b) const { return (what & 16) ? xsb(b).n * (long)nsamp : 0; }
    size_t esize() const { return dtype == 0 ? 8 : 4; }
};

// NaN in the held-out logpdf and the samples of problem b (a joint covariance that is not positive definite, or a failed fit)
template <class A> void joint_fill_nan(const A& a, int b) {  // JointArgs, or VfeJointArgs
    if (a.what & 8) put(a.hlogpdf_out, a.dtype, b, std::numeric_limits<double>::quiet_NaN());
    fill_nan(a.out_b(a.samples_out, 16, b), a.dtype, a.draws(b));
}

// workspace doubles of problem b beyond its slice: every predict strip (they stay alive for batch_jcov_kernel) and the joint slice
long joint_ws(const JointArgs& a, int b) {
    const long ns = a.xsb(b).n;
    if (ns == 0 || a.what == 1) return 0;
    return (ns + TP - 1) / TP * TP * batch_ld(batch_np(a.xb(b).n)) + (a.want_fact() ? batch_slice(ns) : 0);
}

// one wave: the fit, the predict launches with a strip per tile (none shared), batch_jcov_kernel over the 64×64 tiles of every problem's ns × ns matrix and
// batch_jfact_kernel on the joint slices.  Caller holds the ctx lock.
int32_t run_joint_wave(gp_ctx* c, const JointArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    const bool need_v = a.what != 1;
    WaveLayout L;
    wave_layout(a, idx, nw, [&](int b) { return a.want_mean() && a.xsb(b).n > 0; }, L);
    TestPoints tp(a, nw, need_v);  // the variance the predict kernel computes on its way to V: scratch
    std::vector<int> jp_of((size_t)nw, -1);
    Table<JointProb> jp;
    Table<GradTile> jtiles;
    tp.place(a, idx, nw, a.want_mean(), L, [&](int t) {
        if (!need_v) return;
        const int b = idx[t];
        const long ns = a.xsb(b).n;
        JointProb j{};
        j.prob = L.pos[t], j.slot = L.pr[t].slot, j.ns = (int)ns, j.nsp = (int)batch_np(ns), j.nsamp = a.nsamp;
        j.v_off = j.c_off = j.js_off = -1;
        j.xs_off = tp.xs_off[t], j.mean_off = tp.mean_off[t];
        j.cov_off = (a.what & 4) ? take(L.roff, ns * ns) : -1;
        j.jr_off = a.want_fact() ? take(L.roff, 2) : -1;
        j.samp_off = (a.what & 16) ? take(L.roff, a.draws(b)) : -1;
        j.ysd_off = (a.what & 8) ? take(L.off, ns) : -1;
        j.xi_off = (a.what & 16) ? take(L.off, a.draws(b)) : -1;
        const gp_noise* nz = a.noise_xs ? &a.noise_xs[b] : nullptr;
        j.noise_s = nz ? nz->s : 0.0;
        j.nzs_off = (nz && nz->kind == 1) ? take(L.off, ns) : -1;
        jp_of[t] = (int)jp.v.size();
        jp.v.push_back(j);
    });
    // a problem's tiles of TP test points lie one after the other, and so do their strips: V; behind them the joint slice
    tp.tile(a, idx, nw, false, L, [&](int t, long first) {
        if (jp_of[t] < 0) return;
        JointProb& j = jp.v[(size_t)jp_of[t]];
        j.v_off = first;
        if (a.want_fact()) j.js_off = take(L.ws, batch_slice(j.ns));
        for (int ti = 0; ti < j.nsp / BT; ++ti)
            for (int tj = 0; tj <= ti; ++tj) jtiles.v.push_back(GradTile{jp_of[t], ti, tj, 0});
    });
    jp.place(L);
    jtiles.place(L);

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    double* const hin = m.hin;
    wave_fill(a, packed, idx, nw, L, hin);
    tp.fill(a, idx, nw, m);
    for (int t = 0; t < nw; ++t) {
        if (jp_of[t] < 0) continue;
        const int b = idx[t];
        const long ns = a.xsb(b).n;
        const JointProb& j = jp.v[(size_t)jp_of[t]];
        if (j.ysd_off >= 0) {
            const double *ys = (const double*)a.ys[b], *pm = (const double*)a.pmb(b);
            for (long i = 0; i < ns; ++i) hin[j.ysd_off + i] = pm ? ys[i] - pm[i] : ys[i];
        }
        if (j.xi_off >= 0 && a.draws(b) > 0) std::memcpy(hin + j.xi_off, a.xi[b], sizeof(double) * (size_t)a.draws(b));
        if (j.nzs_off >= 0) std::memcpy(hin + j.nzs_off, a.noise_xs[b].diag, sizeof(double) * (size_t)ns);
    }
    jp.fill(m);
    jtiles.fill(m);
    const bool ks = a.ks != nullptr;
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, ks, nw));
        RC(tp.launch_groups(m, ks, nw, nullptr));
        if (!jtiles.v.empty()) RC(launch(m, ks ? batch_jcov_kernel<true> : batch_jcov_kernel<false>, jtiles.v.size(), GNT, nw, jp.dev(m), jtiles.dev(m)));
        if (a.want_fact() && !jp.v.empty()) RC(launch(m, batch_jfact_kernel, jp.v.size(), NT, nw, jp.dev(m)));
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    c->batch_joint_problems += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        if (a.info_joint) a.info_joint[b] = 0;
        const long ns = a.xsb(b).n;
        if (ns == 0) continue;
        tp.put_mean(a, b, t, hout);
        if (jp_of[t] < 0) continue;
        const JointProb& j = jp.v[(size_t)jp_of[t]];
        const double* pm = (const double*)a.pmb(b);
        if (void* co = a.out_b(a.cov_out, 4, b)) std::memcpy(co, hout + j.cov_off, sizeof(double) * (size_t)(ns * ns));
        if (j.jr_off >= 0) {
            if (a.what & 8) ((double*)a.hlogpdf_out)[b] = hout[j.jr_off];
            if (a.info_joint) a.info_joint[b] = (int32_t)hout[j.jr_off + 1];
        }
        if (double* so = (double*)a.out_b(a.samples_out, 16, b))
            for (long e = 0; e < a.draws(b); ++e) so[e] = pm ? pm[e % ns] + hout[j.samp_off + e] : hout[j.samp_off + e];
    }
    return 0;
}

int32_t joint_batch_impl(gp_ctx* c, JointArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_batch_head(a));
    RC(check_test_head(a));
    if (a.what <= 0 || (a.what & ~29)) return set_arg_err(14, "what must be a combination of 1|4|8|16 (marginal variances: gp_predict_batch)");
    if ((a.what & 1) && !a.mean_out) return set_arg_err(15, "mean_out is NULL");
    if ((a.what & 4) && !a.cov_out) return set_arg_err(16, "cov_out is NULL");
    if ((a.what & 8) && !a.ys) return set_arg_err(17, "ys array is NULL");
    if ((a.what & 8) && !a.hlogpdf_out) return set_arg_err(18, "hlogpdf_out is NULL");
    if (a.nsamp < 0) return set_arg_err(19, "nsamp must be >= 0");
    const bool sampling = (a.what & 16) && a.nsamp > 0;
    if (sampling && !a.xi) return set_arg_err(20, "xi array is NULL");
    if (sampling && !a.samples_out) return set_arg_err(21, "samples_out is NULL");
    if (!a.info_out) return set_arg_err(23, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    RC(check_test_points(a, a.noise_xs, {{a.mean_out, (a.what & 1) != 0, 15, "a mean_out pointer is NULL"}, {a.cov_out, (a.what & 4) != 0, 16, "a cov_out pointer is NULL"},
                                         {a.ys, (a.what & 8) != 0, 17, "a ys pointer is NULL"}, {a.xi, sampling, 20, "a xi pointer is NULL"},
                                         {a.samples_out, sampling, 21, "a samples_out pointer is NULL"}}));
    // which path serves a problem depends on that problem alone: gp_logpdf_batch's routing under the joint limits, and a Σy* the kernels take
    const long max_n = env_capped(getenv("GPMI_BATCH_JOINT_MAX_N"), GPMI355_BATCH_JOINT_MAX_N);
    const long max_ns = env_capped(getenv("GPMI_BATCH_JOINT_MAX_NS"), GPMI355_BATCH_JOINT_MAX_NS);
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) {
        const bool nz_ok = !a.noise_xs || a.xsb(b).n == 0 || a.noise_xs[b].kind <= 1;
        (batch_takes(a, b, max_n) && a.xsb(b).n <= max_ns && nz_ok ? mine : routed).push_back(b);
    }
    // slice + strips + joint slice per problem.  The covariances and the draws of a wave travel through the page-locked staging of the ctx, which takes
    // JOINT_PIN_BYTES: a wave that needs more is staged in pageable memory and copies at a quarter of the rate (measured: 512 problems of 64 points with 1 024 test points
    // each in waves of 222, 1 252 ms; in waves that fit, 267 ms).  Charging four times the staged bytes against the workspace budget (four times that limit) bounds both.
    static_assert(BATCH_WS_BYTES == 4 * JOINT_PIN_BYTES, "the factor below");
    auto cost = [&](int b) {
        const gp_points &x = a.xb(b), &xs = a.xsb(b);
        const long n = x.n, ns = xs.n, nts = batch_np(ns) / BT;
        const size_t ws = sizeof(double) * (size_t)(batch_slice(n) + joint_ws(a, b));
        const size_t staged = sizeof(double) * (size_t)(((a.what & 4) ? ns * ns : 0) + 2 * a.draws(b) + (ns + n) * (x.d + 4) + 8) + sizeof(BatchProb) + sizeof(KSum) +
                              sizeof(JointProb) + (size_t)((ns + TP - 1) / TP) * sizeof(BatchTile) + (size_t)(nts * (nts + 1) / 2) * sizeof(GradTile);
        return WaveCost{std::max(ws, 4 * staged), 0};
    };
    RC(for_each_wave(c, mine, cost, [&](const int* idx, int nw) { return run_joint_wave(c, a, packed, idx, nw); }));
    // everything else: gp_posterior_fit, _predict (bits 0 and 2), _logpdf, _rand and _free on the single path, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    const gp_noise zero_noise{0, 0.0, nullptr};
    for (int b : routed) {
        const gp_points& xs = a.xsb(b);
        const gp_noise* nz = a.noise_xs ? &a.noise_xs[b] : &zero_noise;
        gp_post* post = nullptr;
        int32_t rj = 0;
        int32_t rc = routed_fit(c, a, b, &post, nullptr, logpdf_slot(a, b));
        if (rc == 0 && xs.n > 0 && (a.what & 5))
            rc = gp_posterior_predict(post, &xs, a.pmb(b), a.what & 5, a.out_b(a.mean_out, 1, b), nullptr, a.out_b(a.cov_out, 4, b));
        if (rc == 0 && xs.n > 0 && (a.what & 8)) {
            rj = gp_posterior_logpdf(post, &xs, a.pmb(b), nz, a.ys[b], xs.n, 1, (char*)a.hlogpdf_out + a.esize() * (size_t)b);
            if (rj < 0) rc = rj;
        }
        if (rc == 0 && rj == 0 && xs.n > 0 && a.draws(b) > 0) {
            rj = gp_posterior_rand(post, &xs, a.pmb(b), nz, a.xi[b], a.nsamp, a.samples_out[b]);
            if (rj < 0) rc = rj;
        }
        if (post) (void)gp_posterior_free(post);
        RC(routed_done(a, b, rc, [&] {
            if (xs.n <= 0) return;
            fill_nan(a.out_b(a.mean_out, 1, b), a.dtype, xs.n);
            fill_nan(a.out_b(a.cov_out, 4, b), a.dtype, xs.n * xs.n);
        }));
        if (a.info_joint) a.info_joint[b] = rc == 0 ? rj : 0;
        if ((rc > 0 || rj > 0) && xs.n > 0) joint_fill_nan(a, b);
    }
    return 0;
}

// ---- gp_logpdf_grad_batch / gp_logpdf_grad_batch_sum ---------------------------------------------------------------------------------------------------
struct GradArgs : BatchArgs {
    double* dvar;             // single-kind: nb entries, or NULL
    double* const* dscale;    // single-kind: nb pointers, or NULL
    double* const* dtheta;    // composite: nb pointers, or NULL
    void* const* dnoise;
    void* const* dy;
    int arg0;                 // position of the first gradient argument (the reasons of the checks name the argument)
    void* const* dx = nullptr;  // gp_logpdf_grad_batch_x / _sum_x: nb pointers to n_b × d_b entries in the container layout of x_b, or NULL
    void* dnb(int b) const { return dnoise ? dnoise[b] : nullptr; }
    void* dyb(int b) const { return dy ? dy[b] : nullptr; }
    void* dxb(int b) const { return dx ? dx[b] : nullptr; }
};

// a gradient array that is given holds a pointer for every problem (dscale: wherever the problem has scales)
int32_t check_grad_pointers(const GradArgs& a) {
    const int a_dn = a.ks ? a.arg0 + 1 : a.arg0 + 2, a_dy = a_dn + 1;
    for (int b = 0; b < a.nb; ++b) {
        if (a.dscale && a.k[b].nscale > 0 && !a.dscale[b]) return set_arg_err(a.arg0 + 1, "a dscale_out pointer is NULL where the kernel has scales");
        if (a.dtheta && !a.dtheta[b]) return set_arg_err(a.arg0, "a dtheta_out pointer is NULL");
        if (a.dnoise && !a.dnoise[b]) return set_arg_err(a_dn, "a dnoise_out pointer is NULL");
        if (a.dy && !a.dy[b]) return set_arg_err(a_dy, "a dy_out pointer is NULL");
        if (a.dx && !a.dx[b]) return set_arg_err(a_dy + 1, "a dx_out pointer is NULL");
    }
    return 0;
}

// the kernel parameters of problem b: variance + scales, or the θ entries of its composite kernel
int grad_nkp(const GradArgs& a, const std::vector<KSum>& packed, int b) { return a.ks ? packed[b].nth : 1 + a.k[b].nscale; }
long grad_ntiles(long n) { return batch_np(n) / BT * (batch_np(n) / BT + 1) / 2; }
// the per-tile row sums of the input gradient: one [d][64] table per tile of the full square (an even count: what follows stays 16-byte aligned); 0 without dx
long gradx_part(const GradArgs& a, int b) {
    const long nt = batch_np(a.xb(b).n) / BT;
    return a.dxb(b) ? nt * nt * BT * a.xb(b).d : 0;
}
// workspace of a problem in a gradient wave: its slice, the S strip beside it and the per-tile sums
long grad_ws(const GradArgs& a, const std::vector<KSum>& packed, int b) {
    const long n = a.xb(b).n, np = batch_np(n);
    return batch_slice(n) + np * batch_ld(np) + ((grad_ntiles(n) * (1 + grad_nkp(a, packed, b)) + 1) & ~1L) + gradx_part(a, b);
}

// NaN in every gradient output of problem b (nkp kernel parameters)
void grad_fill_nan(const GradArgs& a, int b, int nkp) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const long n = a.xb(b).n;
    if (a.dvar) a.dvar[b] = nan;
    if (a.dscale && a.dscale[b]) std::fill_n(a.dscale[b], nkp - 1, nan);
    if (a.dtheta) std::fill_n(a.dtheta[b], nkp, nan);
    const int nk = a.noise[b].kind;
    fill_nan(a.dnb(b), a.dtype, nk == 0 ? 1 : (nk == 1 ? n : n * n));
    fill_nan(a.dyb(b), a.dtype, n);
    fill_nan(a.dxb(b), a.dtype, n * a.xb(b).d);
}

// The 64×64 tiles of the s-th descriptor's matrix of nt × nt tiles: its lower triangle, numbered ti (ti + 1) / 2 + tj, or the full square, numbered ti · nt + tj.
void push_tiles(std::vector<GradTile>& tiles, int s, int nt, bool square) {
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj < (square ? nt : ti + 1); ++tj) tiles.push_back(GradTile{s, ti, tj, square ? ti * nt + tj : ti * (ti + 1) / 2 + tj});
}
// The gradient half of the s-th descriptor's GradProb (nkp kernel parameters; diag: the noise is a vector): the per-tile sums in the workspace, the totals and
// the gradient of a diagonal noise in the results.
void place_grad(WaveLayout& L, int s, int nkp, bool diag, GradProb& g) {
    const BatchProb& p = L.pr[L.order[s]];
    const int nt = p.np / BT;
    g.ng = 1 + nkp;
    g.ntiles = nt * (nt + 1) / 2;
    g.part_off = take(L.ws, ((long)g.ntiles * g.ng + 1) & ~1L);  // the next strip stays 16-byte aligned
    g.g_off = take(L.roff, g.ng);
    g.dn_off = diag ? take(L.roff, p.n) : -1;
}
// the totals of problem b (n points) to the caller: G[0] noise, then the kernel's parameters
void put_grads(const GradArgs& a, int b, const GradProb& g, long n, const double* hout) {
    const double* G = hout + g.g_off;
    if (a.dvar) a.dvar[b] = G[1];
    if (a.dscale && a.dscale[b]) std::memcpy(a.dscale[b], G + 2, sizeof(double) * (size_t)(g.ng - 2));
    if (a.dtheta) std::memcpy(a.dtheta[b], G + 1, sizeof(double) * (size_t)(g.ng - 1));
    if (double* dn = (double*)a.dnb(b)) {
        if (g.dn_off >= 0) std::memcpy(dn, hout + g.dn_off, sizeof(double) * (size_t)n);
        else dn[0] = G[0];
    }
}

// one wave: the fit launch of the problems idx[0..nw) with α for every one of them, then S = L⁻ᵀ, the tile sums and their totals.  Caller holds the ctx lock.
int32_t run_grad_wave(gp_ctx* c, const GradArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [](int) { return true; }, L);
    // behind the fit's input: the GradProb table (in the order of the descriptors), the tiles of S and the tiles of the triangle, the widest problems first
    Table<GradProb> gp;
    Table<GradTile> itiles, gtiles;
    gp.v.assign((size_t)nw, GradProb{-1, -1, -1, -1, 0, 0});
    for (int s = 0; s < nw; ++s) {
        const int b = idx[L.order[s]];
        place_s_strip(L, s, gp.v[s], itiles);
        place_grad(L, s, grad_nkp(a, packed, b), a.noise[b].kind == 1, gp.v[s]);
        push_tiles(gtiles.v, s, L.pr[L.order[s]].np / BT, false);
    }
    // the problems whose dx is wanted: their tables of row sums behind everything else in the workspace, the gradient [d][n] behind the other results, the
    // tiles of the full square and the 64-row blocks batch_gxsum_kernel adds them up in.  Without any, the wave is laid out and launched as it always was.
    Table<GradXProb> gx;
    Table<GradTile> xtiles, xrows;
    int nwx = 0;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s], b = idx[t];
        if (!a.dxb(b)) continue;
        if (gx.v.empty()) gx.v.assign((size_t)nw, GradXProb{-1, -1});
        const BatchProb& p = L.pr[t];
        gx.v[s].xpart_off = take(L.ws, gradx_part(a, b));
        gx.v[s].dx_off = take(L.roff, (long)p.n * p.d);
        push_tiles(xtiles.v, s, p.np / BT, true);
        for (int ti = 0; ti < p.np / BT; ++ti) xrows.v.push_back(GradTile{s, ti, 0, 0});
        ++nwx;
    }
    gp.place(L);
    itiles.place(L);
    gtiles.place(L);
    gx.place(L);
    xtiles.place(L);
    xrows.place(L);

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    gp.fill(m);
    itiles.fill(m);
    gtiles.fill(m);
    gx.fill(m);
    xtiles.fill(m);
    xrows.fill(m);
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        RC(launch_inv(m, nw, gp, itiles));
        RC(launch_grad(m, a.ks != nullptr, nw, gp.dev(m), gtiles));
        RC(launch(m, batch_gsum_kernel, nw, 128, nw, gp.dev(m)));
        if (nwx) {
            RC(launch(m, a.ks ? batch_gradx_kernel<true> : batch_gradx_kernel<false>, xtiles.v.size(), GNT, nw, gp.dev(m), gx.dev(m), xtiles.dev(m)));
            RC(launch(m, batch_gxsum_kernel, xrows.v.size(), BT, nw, gx.dev(m), xrows.dev(m)));
        }
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    c->batch_grad_problems += nw;
    c->batch_gradx_problems += nwx;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const long n = L.pr[t].n;
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        put_grads(a, b, gp.v[L.pos[t]], n, hout);
        if (double* dy = (double*)a.dyb(b)) {
            const double* al = hout + L.pr[t].alpha_off;
            for (long j = 0; j < n; ++j) dy[j] = -al[j];
        }
        if (void* dx = a.dxb(b)) grad_to_layout<double>(a.xb(b).layout, n, a.xb(b).d, hout + gx.v[L.pos[t]].dx_off, n, dx);  // [d][n] -> the container layout of x
    }
    return 0;
}

int32_t grad_batch_impl(gp_ctx* c, GradArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_batch_head(a));
    if (!a.logpdf_out) return set_arg_err(10, "logpdf_out is NULL");
    if (!a.info_out) return set_arg_err(11, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    RC(check_grad_pointers(a));
    // which path serves a problem depends on that problem alone and on whether the call asks for dx: the input-gradient kernels have a limit of their own
    std::vector<int> mine, routed;
    split_by_path(a, a.dx ? env_capped(getenv("GPMI_BATCH_GRADX_MAX_N"), GPMI355_BATCH_GRADX_MAX_N)
                          : env_capped(getenv("GPMI_BATCH_GRAD_MAX_N"), GPMI355_BATCH_GRAD_MAX_N), mine, routed);
    RC(for_each_wave(c, mine, [&](int b) { return WaveCost{sizeof(double) * (size_t)grad_ws(a, packed, b), 0}; },  // slices, strips and tile sums count
                     [&](const int* idx, int nw) { return run_grad_wave(c, a, packed, idx, nw); }));
    // everything else: gp_logpdf_grad / gp_logpdf_grad_sum (gp_logpdf_grad_sum_x where dx is wanted), one problem at a time, after the lock is released (as
    // batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        void* lp = logpdf_slot(a, b);
        double* dth = a.dtheta ? a.dtheta[b] : nullptr;
        const int32_t rc = !a.ks       ? gp_logpdf_grad(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), lp, a.dvar ? &a.dvar[b] : nullptr,
                                                        a.dscale ? a.dscale[b] : nullptr, a.dnb(b), a.dyb(b), a.dxb(b))
                           : a.dxb(b) ? gp_logpdf_grad_sum_x(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), lp, dth, a.dnb(b), a.dyb(b), a.dxb(b))
                                      : gp_logpdf_grad_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), lp, dth, a.dnb(b), a.dyb(b));
        RC(routed_done(a, b, rc, [&] { grad_fill_nan(a, b, grad_nkp(a, packed, b)); }));
    }
    return 0;
}

// gp_logpdf_grad_batch_x / _sum_x: the body of gp_logpdf_grad_batch / _sum with a.dx set.  The entry points' own guard: the ctx is pinned for the whole call
// and the lock handed on, as it is to the single-path calls above (grad_batch_impl validates the ctx again and takes the lock itself).
int32_t gradx_batch_impl(gp_ctx* c, GradArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    gd.lk.unlock();
    return grad_batch_impl(c, a);
}

// ---- gp_loo_batch / gp_loo_batch_sum, gp_loo_grad_batch / gp_loo_grad_batch_sum ------------------------------------------------------------------------
struct LooArgs : GradArgs {  // logpdf_out is value_out; the value calls leave every gradient array NULL, the gradient calls the three per-point arrays
    bool grad;
    void* const* lp = nullptr;
    void* const* mean = nullptr;
    void* const* var = nullptr;
    void* lpb(int b) const { return lp ? lp[b] : nullptr; }
    void* meanb(int b) const { return mean ? mean[b] : nullptr; }
    void* varb(int b) const { return var ? var[b] : nullptr; }
};

long loo_tiles(long n) { return (batch_np(n) + TP - 1) / TP; }  // the 128-row tiles of a strip
// workspace of a problem in a leave-one-out wave: its slice, the S strip and the partial sums of L; for the gradient the Z strip, d and e and the per-tile sums
long loo_ws(const LooArgs& a, const std::vector<KSum>& packed, int b) {
    const long n = a.xb(b).n, np = batch_np(n);
    const long value = batch_slice(n) + np * batch_ld(np) + ((loo_tiles(n) + 1) & ~1L);
    return a.grad ? value + np * batch_ld(np) + 2 * np + ((grad_ntiles(n) * (1 + grad_nkp(a, packed, b)) + 1) & ~1L) : value;
}

// NaN in every output of problem b beyond its value
void loo_fill_nan(const LooArgs& a, int b, int nkp) {
    const long n = a.xb(b).n;
    fill_nan(a.lpb(b), a.dtype, n);
    fill_nan(a.meanb(b), a.dtype, n);
    fill_nan(a.varb(b), a.dtype, n);
    if (a.grad) grad_fill_nan(a, b, nkp);
}

// one wave: the fit launch of the problems idx[0..nw) with α for every one of them, S = L⁻ᵀ, the leave-one-out terms and their sum; for the gradient Z, β, the
// tile sums with the leave-one-out weights and their totals.  Caller holds the ctx lock.
int32_t run_loo_wave(gp_ctx* c, const LooArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [](int) { return true; }, L);
    // behind the fit's input: the GradProb and LooProb tables (in the order of the descriptors), the 128-row tiles of the strips, the tiles of the triangle and
    // of the full square, the widest problems first
    Table<GradProb> gp;
    Table<LooProb> lq;
    Table<GradTile> itiles, gtiles, ztiles;
    gp.v.assign((size_t)nw, GradProb{-1, -1, -1, -1, 0, 0});
    lq.v.assign((size_t)nw, LooProb{-1, -1, -1, -1, -1, -1, -1, -1});
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s], b = idx[t];
        const BatchProb& p = L.pr[t];
        LooProb& q = lq.v[s];
        place_s_strip(L, s, gp.v[s], itiles);
        q.lpart_off = take(L.ws, (loo_tiles(p.n) + 1) & ~1L);  // the next strip stays 16-byte aligned
        if (a.lpb(b)) q.lp_off = take(L.roff, p.n);
        if (a.meanb(b)) q.mean_off = take(L.roff, p.n);
        if (a.varb(b)) q.var_off = take(L.roff, p.n);
        if (!a.grad) continue;
        q.z_off = take(L.ws, (long)p.np * p.ld);
        q.d_off = take(L.ws, p.np);
        q.e_off = take(L.ws, p.np);
        place_grad(L, s, grad_nkp(a, packed, b), a.noise[b].kind == 1, gp.v[s]);
        q.beta_off = take(L.roff, p.np);
        push_tiles(gtiles.v, s, p.np / BT, false);
        push_tiles(ztiles.v, s, p.np / BT, true);
    }
    gp.place(L);
    lq.place(L);
    itiles.place(L);
    gtiles.place(L);
    ztiles.place(L);

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    gp.fill(m);
    lq.fill(m);
    itiles.fill(m);
    gtiles.fill(m);
    ztiles.fill(m);
    RC(run_drained(c, [&]() -> int32_t {
        const size_t nit = itiles.v.size();
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        RC(launch_inv(m, nw, gp, itiles));
        RC(launch(m, batch_loo_kernel, nit, NT, nw, gp.dev(m), lq.dev(m), itiles.dev(m)));
        RC(launch(m, batch_loo_sum_kernel, nw, 128, nw, lq.dev(m)));
        if (a.grad) {
            RC(launch(m, batch_loo_z_kernel, ztiles.v.size(), GNT, nw, gp.dev(m), lq.dev(m), ztiles.dev(m)));
            RC(launch(m, batch_loo_beta_kernel, nit, NT, nw, lq.dev(m), itiles.dev(m)));
            RC(launch_grad(m, a.ks != nullptr, nw, gp.dev(m), gtiles, lq.dev(m)));
            RC(launch(m, batch_gsum_kernel, nw, 128, nw, gp.dev(m)));
        }
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    (a.grad ? c->batch_loo_grad_problems : c->batch_loo_problems) += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const LooProb& q = lq.v[L.pos[t]];
        const long n = L.pr[t].n;
        const size_t bytes = sizeof(double) * (size_t)n;
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        if (q.lp_off >= 0) std::memcpy(a.lpb(b), hout + q.lp_off, bytes);
        if (q.mean_off >= 0) std::memcpy(a.meanb(b), hout + q.mean_off, bytes);
        if (q.var_off >= 0) std::memcpy(a.varb(b), hout + q.var_off, bytes);
        if (!a.grad) continue;
        put_grads(a, b, gp.v[L.pos[t]], n, hout);
        if (double* dy = (double*)a.dyb(b)) {
            const double* be = hout + q.beta_off;
            for (long j = 0; j < n; ++j) dy[j] = -be[j];
        }
    }
    return 0;
}

// the checks both bodies share, behind the ctx check: counts, arrays, problems; value_out and info_out are arguments 10 and 11
int32_t loo_check_head(LooArgs& a, std::vector<KSum>& packed) {
    RC(check_batch_head(a));
    if (!a.logpdf_out) return set_arg_err(10, "value_out is NULL");
    if (!a.info_out) return set_arg_err(11, "info_out is NULL");
    return check_batch_problems(a, packed);
}

// gp_loo_batch / gp_loo_batch_sum
int32_t loo_batch_impl(gp_ctx* c, LooArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    std::vector<KSum> packed;
    RC(loo_check_head(a, packed));
    for (int b = 0; b < a.nb; ++b) {  // an output array that is given holds a pointer for every problem
        if (a.lp && !a.lp[b]) return set_arg_err(12, "an lp_out pointer is NULL");
        if (a.mean && !a.mean[b]) return set_arg_err(13, "a mean_out pointer is NULL");
        if (a.var && !a.var[b]) return set_arg_err(14, "a var_out pointer is NULL");
    }
    std::vector<int> mine, routed;
    split_by_path(a, env_capped(getenv("GPMI_BATCH_LOO_MAX_N"), GPMI355_BATCH_LOO_MAX_N), mine, routed);
    RC(for_each_wave(c, mine, [&](int b) { return WaveCost{sizeof(double) * (size_t)loo_ws(a, packed, b), 0}; },  // slices, strips and partial sums count
                     [&](const int* idx, int nw) { return run_loo_wave(c, a, packed, idx, nw); }));
    // everything else: gp_loo / gp_loo_sum, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        void* val = logpdf_slot(a, b);
        const int32_t rc = a.ks ? gp_loo_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), val, a.lpb(b), a.meanb(b), a.varb(b))
                                : gp_loo(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), val, a.lpb(b), a.meanb(b), a.varb(b));
        RC(routed_done(a, b, rc, [&] { loo_fill_nan(a, b, 0); }));
    }
    return 0;
}

// gp_loo_grad_batch / gp_loo_grad_batch_sum.  A call that asks for dx runs on the single path, every problem of it: the kernels have no ∂/∂x yet.
int32_t loo_grad_batch_impl(gp_ctx* c, LooArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    std::vector<KSum> packed;
    RC(loo_check_head(a, packed));
    RC(check_grad_pointers(a));
    // which path serves a problem depends on that problem alone and on whether the call asks for dx
    std::vector<int> mine, routed;
    split_by_path(a, a.dx ? -1 : env_capped(getenv("GPMI_BATCH_LOO_GRAD_MAX_N"), GPMI355_BATCH_LOO_GRAD_MAX_N), mine, routed);
    RC(for_each_wave(c, mine, [&](int b) { return WaveCost{sizeof(double) * (size_t)loo_ws(a, packed, b), 0}; },  // slices, both strips and tile sums count
                     [&](const int* idx, int nw) { return run_loo_wave(c, a, packed, idx, nw); }));
    // everything else: gp_loo_grad / gp_loo_grad_sum, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        void* val = logpdf_slot(a, b);
        const int32_t rc = a.ks ? gp_loo_grad_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), val, a.dtheta ? a.dtheta[b] : nullptr, a.dnb(b), a.dyb(b), a.dxb(b))
                                : gp_loo_grad(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), val, a.dvar ? &a.dvar[b] : nullptr,
                                              a.dscale ? a.dscale[b] : nullptr, a.dnb(b), a.dyb(b), a.dxb(b));
        RC(routed_done(a, b, rc, [&] { loo_fill_nan(a, b, grad_nkp(a, packed, b)); }));
    }
    return 0;
}

// ---- gp_vfe_batch ------------------------------------------------------------------------------------------------------------------------------------------
struct VfeArgs : BatchArgs {  // logpdf_out is objective_out
    int32_t nz;
    const gp_points* z;
    const double* jitter;
    const int32_t* approx;
    void* const* meps_out;
    const gp_points& zb(int b) const { return z[nz == 1 ? 0 : b]; }
    void* eb(int b) const { return meps_out ? meps_out[b] : nullptr; }
};
// the gradient outputs of gp_vfe_grad_batch (arrays of nb; dscale, dz and dx may be NULL)
struct VfeGradOut {
    double* dvar;
    double* const* dscale;
    void* const* dnoise;
    void* const* dy;
    double* const* dz;
    void* const* dx;
};
// gp_vfe_predict_batch: the test side as PredictArgs carries it for gp_predict_batch (what: 1 mean | 2 var); objective_out may be NULL
struct VfePredictArgs : VfeArgs {
    int32_t nxs;
    const gp_points* xs;
    const void* const* pm;
    int32_t what;
    void* const* mean_out;
    void* const* var_out;
    // gp_vfe_predict_grad_batch only (grad): the gradient arrays; there each of the four arrays may be NULL, not both of a side that is asked for
    bool grad = false;
    void* const* dmean_out = nullptr;
    void* const* dvar_out = nullptr;
    const gp_points& xsb(int b) const { return xs[nxs == 1 ? 0 : b]; }
    const void* pmb(int b) const { return pm ? pm[b] : nullptr; }
    void* out_b(void* const* arr, int side, int b) const { return (arr && (what & side)) ? arr[b] : nullptr; }
};
// gp_vfe_joint_batch: the joint side as JointArgs carries it for gp_joint_batch (what: 1 mean | 4 latent covariance | 8 held-out logpdf | 16 samples; var_out is not used)
struct VfeJointArgs : VfePredictArgs {
    const gp_noise* noise_xs;
    void* const* cov_out;
    const void* const* ys;
    void* hlogpdf_out;
    int32_t nsamp;
    const void* const* xi;
    void* const* samples_out;
    int32_t* info_joint;
    bool want_strips() const { return (what & 28) != 0; }  // B* and C*: everything but the mean alone
    bool want_fact() const { return (what & 24) != 0; }
    bool want_mean() const { return (what & 25) != 0; }  // the held-out logpdf and the samples are built on it
    long draws(int b) const { return (what & 16) ? xsb(b).n * (long)nsamp : 0; }
    size_t esize() const { return dtype == 0 ? 8 : 4; }
};

// the pseudo-inputs of one problem, dimension-major [d][m], scaled as the sparse path scales its inputs on the host (one product per entry)
void pack_scaled_points(const gp_kernel& k, const gp_points& z, double* out) {
    pack_points(z, out);
    for (int dd = 0; dd < z.d && k.nscale > 0; ++dd) {
        const double s = k.scale[k.nscale == 1 ? 0 : dd];
        for (long i = 0; i < z.n; ++i) out[(size_t)dd * z.n + i] *= s;
    }
}

// obj_arg / info_arg: where the call has objective_out and info_out (obj_arg 0: the objective may be left out)
int32_t check_vfe_args(VfeArgs& a, int obj_arg = 14, int info_arg = 15) {
    if (!a.k) return set_arg_err(3, "kernel array is NULL");
    if (a.nx != 1 && a.nx != a.nb) return set_arg_err(4, "nx must be 1 (one x shared by every problem) or nb");
    if (!a.x) return set_arg_err(5, "points array is NULL");
    if (a.nz != 1 && a.nz != a.nb) return set_arg_err(6, "nz must be 1 (one z shared by every problem) or nb");
    if (!a.z) return set_arg_err(7, "pseudo-points array is NULL");
    if (!a.noise) return set_arg_err(8, "noise array is NULL");
    if (!a.jitter) return set_arg_err(9, "jitter array is NULL");
    if (a.ny != 1 && a.ny != a.nb) return set_arg_err(11, "ny must be 1 (one y shared by every problem) or nb");
    if (!a.y) return set_arg_err(12, "y array is NULL");
    for (int b = 0; b < a.ny; ++b)
        if (!a.y[b]) return set_arg_err(12, "a y pointer is NULL");
    if (!a.approx) return set_arg_err(13, "approx array is NULL");
    if (obj_arg && !a.logpdf_out) return set_arg_err(obj_arg, "objective_out is NULL");
    if (!a.info_out) return set_arg_err(info_arg, "info_out is NULL");
    a.dtype = a.k[0].dtype;
    for (int b = 0; b < a.nb; ++b) {
        const gp_points &x = a.xb(b), &z = a.zb(b);
        RC(check_points(&x, 5));
        RC(check_points(&z, 7));
        if (z.d != x.d) return set_arg_err(7, "z has a different D than x");
        RC(check_kernel(&a.k[b], x.d, 3));
        if (a.k[b].dtype != a.dtype) return set_arg_err(3, "every descriptor of one batch call carries the same dtype");
        RC(check_noise(&a.noise[b], 8, true));
        if (!(a.jitter[b] >= 0)) return set_arg_err(9, "jitter must be >= 0");
        if (a.ny == 1 && x.n != a.xb(0).n) return set_arg_err(11, "a shared y needs problems of one size");
        if (a.approx[b] != 0 && a.approx[b] != 1) return set_arg_err(13, "approx must be 0 (VFE) or 1 (DTC)");
    }
    return 0;
}

// which path serves a problem depends on that problem alone (a noise variance that is not positive is the single path's to report)
bool vfe_batch_takes(const VfeArgs& a, int b, long max_n) {
    const gp_points& x = a.xb(b);
    const gp_noise& nz = a.noise[b];
    if (a.dtype != 0 || nz.kind > 1 || x.d > BATCH_MAXD || a.zb(b).n > VFE_MAXM || x.n > max_n) return false;
    if (nz.kind == 0) return nz.s > 0;
    const double* dg = (const double*)nz.diag;
    return std::all_of(dg, dg + x.n, [](double v) { return v > 0; });
}

long vfe_nseg(long n) { return (n + VFE_SEG - 1) / VFE_SEG; }
// workspace doubles of one problem: the slices of L_z and Λ_ε, the strip L_z⁻ᵀ and a slot of partial sums per segment
long vfe_ws(const VfeArgs& a, int b) {
    const long m = a.zb(b).n, np = batch_np(m);
    return 2 * batch_slice(m) + np * batch_ld(np) + vfe_nseg(a.xb(b).n) * vfe_part(np);
}
// what the gradient adds: Λ_ε.L⁻ᵀ, H, V H, G_ψ and G_zz (np rows of ld each) and a slot of gradient sums per segment
long vfe_grad_ws(const VfeArgs& a, int b) {
    const long np = batch_np(a.zb(b).n);
    return 5 * np * batch_ld(np) + vfe_nseg(a.xb(b).n) * vfe_gpart(np, a.xb(b).d);
}

// doubles problem b alone adds to the packed input of its wave: its z, mean and noise vector, and its x and y where the problems do not share them
long vfe_in(const VfeArgs& a, int b) {
    const gp_points &x = a.xb(b), &z = a.zb(b);
    return (long)z.d * z.n + (a.nx == 1 ? 0 : (long)x.d * x.n) + (a.ny == 1 ? 0 : x.n) + (a.mb(b) ? x.n : 0) + (a.noise[b].kind == 1 ? x.n : 0);
}

// doubles problem b alone adds to the result buffer of a gradient wave (run_vfe_wave's layout): α, the sums, dz, dy and, where they exist, the dnoise vector and
// dx.  They are page-locked staging like the packed input and as long (dx: n·d per problem even where x is shared), so the wave bound counts them with it.
long vfe_grad_out(const VfeArgs& a, const VfeGradOut& go, int b) {
    const gp_points &x = a.xb(b), &z = a.zb(b);
    return 2 + z.n + VFE_GH + (long)z.d * z.n + x.n + (a.noise[b].kind == 1 ? x.n : 0) + (go.dx ? (long)x.d * x.n : 0);
}

// fills the data of a laid-out wave behind its tables: every problem's scaled z, then x and y (a shared one once), mean and noise vector
void vfe_wave_fill(const VfeArgs& a, const int* idx, int nw, const std::vector<VfeProb>& pr, double* hin) {
    SharedOnce xo{a.nx == 1}, yo{a.ny == 1};
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& x = a.xb(b);
        const VfeProb& p = pr[t];
        pack_scaled_points(a.k[b], a.zb(b), hin + p.z_off);
        if (xo.claim()) pack_points(x, hin + p.x_off);
        if (yo.claim()) std::memcpy(hin + p.y_off, a.yb(b), sizeof(double) * x.n);
        if (p.m_off >= 0) std::memcpy(hin + p.m_off, a.mb(b), sizeof(double) * x.n);
        if (p.nz_off >= 0) std::memcpy(hin + p.nz_off, a.noise[b].diag, sizeof(double) * x.n);
    }
}

// the test side of a prediction wave behind that: the test points (a shared set once) and prior mean of every problem that has a first segment, at its offsets
void vfe_test_fill(const VfePredictArgs& a, const int* idx, int nw, const std::vector<VfePSeg>& ps, const std::vector<long>& first_seg, double* hin) {
    SharedOnce xso{a.nxs == 1};
    for (int t = 0; t < nw; ++t) {
        if (first_seg[t] < 0) continue;
        const VfePSeg& s = ps[(size_t)first_seg[t]];
        if (xso.claim()) pack_points(a.xsb(idx[t]), hin + s.xs_off);
        if (s.pm_off >= 0) std::memcpy(hin + s.pm_off, a.pmb(idx[t]), sizeof(double) * s.ns);
    }
}

// the joint side of a gp_vfe_joint_batch wave behind that: y* (the mean on the device includes m(x*)), ξ and a diagonal Σy* of every problem that has a JointProb
void vfe_joint_fill(const VfeJointArgs& a, const int* idx, int nw, const std::vector<JointProb>& jp, const std::vector<int>& jp_of, double* hin) {
    for (int t = 0; t < nw; ++t) {
        if (jp_of[t] < 0) continue;
        const int b = idx[t];
        const JointProb& j = jp[(size_t)jp_of[t]];
        if (j.ysd_off >= 0) std::memcpy(hin + j.ysd_off, a.ys[b], sizeof(double) * (size_t)j.ns);
        if (j.xi_off >= 0 && a.draws(b) > 0) std::memcpy(hin + j.xi_off, a.xi[b], sizeof(double) * (size_t)a.draws(b));
        if (j.nzs_off >= 0) std::memcpy(hin + j.nzs_off, a.noise_xs[b].diag, sizeof(double) * (size_t)j.ns);
    }
}

// NaN in every gradient entry of problem b (the call's dtype: a routed fp32 problem has float arrays)
void vfe_grad_fill_nan(const VfeArgs& a, const VfeGradOut& go, int b) {
    const gp_points &x = a.xb(b), &z = a.zb(b);
    go.dvar[b] = std::numeric_limits<double>::quiet_NaN();
    if (go.dscale) fill_nan(go.dscale[b], 0, a.k[b].nscale);
    fill_nan(go.dnoise[b], a.dtype, a.noise[b].kind == 1 ? x.n : 1);
    fill_nan(go.dy[b], a.dtype, x.n);
    if (go.dz) fill_nan(go.dz[b], 0, (long)z.n * z.d);
    if (go.dx) fill_nan(go.dx[b], a.dtype, (long)x.n * x.d);
}

// test points per workgroup of the predict kernel (the segments are the host's: the kernel takes their bounds from the table); the environment variable
// GPMI_VFE_PREDICT_BATCH_SEG, read per call, overrides the header's value for measurements (whole tiles)
long vfe_pseg() { return std::max<long>(VT, env_capped(getenv("GPMI_VFE_PREDICT_BATCH_SEG"), VFE_PSEG, 1 << 20) / VT * VT); }

// three launches: the problems idx[0..nw) of the call, all taken by the kernels.  Caller holds the ctx lock.  With go (gp_vfe_grad_batch) three more behind them:
// α of every problem goes to the result buffer, whether the caller asked for it or not, and the gradient's tables and results are laid out beside the fit's.
// With pa (gp_vfe_predict_batch: a itself) the two prediction launches instead: α likewise, the test points and prior means behind the fit's input (a shared
// set once), the strip L_D⁻ᵀ of every problem whose variance is asked for behind its slices, mean and variance behind the fit's results.
// With ja (gp_vfe_joint_batch: a itself, pa the same object) the predict launches store the strips of B* and C* (vfe_predict_kernel<false, true>; the mean alone
// takes the plain variant), and vfe_jcov_kernel over the 64×64 tiles of every problem's ns × ns matrix and batch_jfact_kernel on the joint slices follow: both
// strips and the joint slice behind the problem's other workspace, covariance, held-out logpdf and samples behind its other results, y*, ξ and a diagonal Σy*
// behind its other input, as run_joint_wave lays them out.
int32_t run_vfe_wave(gp_ctx* c, const VfeArgs& a, const int* idx, int nw, const VfeGradOut* go = nullptr, const VfePredictArgs* pa = nullptr,
                     const VfeJointArgs* ja = nullptr) {
    WaveLayout L;
    L.roff = 2L * nw;
    Table<VfeProb> vp;
    Table<VfeSeg> sg;
    Table<VfeGrad> vg;
    Table<VfePred> vq;
    Table<VfePSeg> ps;
    Table<JointProb> jp;
    Table<GradTile> jtiles;
    std::vector<long> first_seg((size_t)nw, -1);  // a problem's first entry of ps: its offsets
    std::vector<int> jp_of((size_t)nw, -1);       // a problem's entry of jp
    const bool strips = ja && ja->want_strips();
    const long pseg = vfe_pseg();
    vp.v.assign((size_t)nw, VfeProb{});
    vp.place(L);
    if (pa) {
        vq.v.assign((size_t)nw, VfePred{-1, -1, -1});
        vq.place(L);
    }
    if (go) {
        vg.v.assign((size_t)nw, VfeGrad{});
        vg.place(L);
    }
    SharedOnce xo{a.nx == 1}, yo{a.ny == 1}, xso{pa && pa->nxs == 1};
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points &x = a.xb(b), &z = a.zb(b);
        const gp_kernel& k = a.k[b];
        VfeProb& p = vp.v[t];
        p.n = (int)x.n, p.m = (int)z.n, p.np = (int)batch_np(z.n), p.ld = (int)batch_ld(p.np), p.d = x.d;
        p.kind = k.kind, p.nscale = k.nscale, p.slot = t, p.approx = a.approx[b], p.nseg = (int)vfe_nseg(x.n);
        p.variance = k.variance, p.noise_s = a.noise[b].s, p.jitter = a.jitter[b];
        for (int q = 0; q < k.nscale; ++q) p.scale[q] = k.scale[q];
        p.z_off = take(L.off, (long)z.d * z.n);
        p.x_off = xo.place(L.off, (long)x.d * x.n);
        p.y_off = yo.place(L.off, x.n);
        p.m_off = a.mb(b) ? take(L.off, x.n) : -1;
        p.nz_off = a.noise[b].kind == 1 ? take(L.off, x.n) : -1;
        p.lz_off = take(L.ws, batch_slice(z.n));
        p.w_off = take(L.ws, (long)p.np * p.ld);
        p.d_off = take(L.ws, batch_slice(z.n));
        p.part_off = take(L.ws, p.nseg * vfe_part(p.np));
        p.alpha_off = (a.ab(b) || go || pa) ? take(L.roff, z.n) : -1;
        p.meps_off = a.eb(b) ? take(L.roff, z.n) : -1;
        for (int s = 0; s < p.nseg; ++s) sg.v.push_back(VfeSeg{t, s});
        if (go) {
            VfeGrad& q = vg.v[t];
            const long sq = (long)p.np * p.ld;
            q.u_off = take(L.ws, sq), q.h_off = take(L.ws, sq), q.rt_off = take(L.ws, sq), q.gpsi_off = take(L.ws, sq), q.gzz_off = take(L.ws, sq);
            q.gpart_off = take(L.ws, p.nseg * vfe_gpart(p.np, p.d));
            q.gh_off = take(L.roff, VFE_GH);
            q.dz_off = take(L.roff, (long)z.d * z.n);
            q.dn_off = a.noise[b].kind == 1 ? take(L.roff, x.n) : -1;
            q.dy_off = take(L.roff, x.n);
            q.dx_off = go->dx ? take(L.roff, (long)x.d * x.n) : -1;
        }
        if (pa && pa->xsb(b).n > 0) {
            const gp_points& xs = pa->xsb(b);
            const long ns = xs.n;
            if ((pa->what & 2) || strips) vq.v[t].u_off = take(L.ws, (long)p.np * p.ld);
            const long xs_off = xso.place(L.off, (long)xs.d * ns), pm_off = pa->pmb(b) ? take(L.off, ns) : -1;
            const long mean_off = (pa->out_b(pa->mean_out, 1, b) || (ja && ja->want_mean())) ? take(L.roff, ns) : -1, var_off = pa->out_b(pa->var_out, 2, b) ? take(L.roff, ns) : -1;
            const long dmean_off = pa->out_b(pa->dmean_out, 1, b) ? take(L.roff, ns * xs.d) : -1, dvar_off = pa->out_b(pa->dvar_out, 2, b) ? take(L.roff, ns * xs.d) : -1;
            first_seg[t] = (long)ps.v.size();
            for (long r0 = 0; r0 < ns; r0 += pseg)
                ps.v.push_back(VfePSeg{xs_off, pm_off, mean_off, var_off, dmean_off, dvar_off, t, (int)ns, (int)r0, (int)std::min<long>(pseg, ns - r0)});
            if (strips) {
                const long rows = (ns + VT - 1) / VT * VT;  // the predict kernel writes whole tiles of 64 test points
                JointProb j{};
                j.prob = j.slot = t, j.ns = (int)ns, j.nsp = (int)batch_np(ns), j.nsamp = ja->nsamp;
                j.v_off = vq.v[t].bs_off = take(L.ws, rows * p.ld);
                j.c_off = vq.v[t].cs_off = take(L.ws, rows * p.ld);
                j.js_off = ja->want_fact() ? take(L.ws, batch_slice(ns)) : -1;
                j.xs_off = xs_off, j.mean_off = mean_off;
                j.cov_off = (ja->what & 4) ? take(L.roff, ns * ns) : -1;
                j.jr_off = ja->want_fact() ? take(L.roff, 2) : -1;
                j.samp_off = (ja->what & 16) ? take(L.roff, ja->draws(b)) : -1;
                j.ysd_off = (ja->what & 8) ? take(L.off, ns) : -1;
                j.xi_off = (ja->what & 16) ? take(L.off, ja->draws(b)) : -1;
                const gp_noise* nz = ja->noise_xs ? &ja->noise_xs[b] : nullptr;
                j.noise_s = nz ? nz->s : 0.0;
                j.nzs_off = (nz && nz->kind == 1) ? take(L.off, ns) : -1;
                jp_of[t] = (int)jp.v.size();
                jp.v.push_back(j);
                for (int ti = 0; ti < j.nsp / BT; ++ti)
                    for (int tj = 0; tj <= ti; ++tj) jtiles.v.push_back(GradTile{jp_of[t], ti, tj, 0});
            }
        }
    }
    sg.place(L);
    ps.place(L);
    jp.place(L);
    jtiles.place(L);
    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    vp.fill(m);
    sg.fill(m);
    vg.fill(m);
    vq.fill(m);
    ps.fill(m);
    jp.fill(m);
    jtiles.fill(m);
    vfe_wave_fill(a, idx, nw, vp.v, m.hin);
    if (pa) vfe_test_fill(*pa, idx, nw, ps.v, first_seg, m.hin);
    if (ja) vfe_joint_fill(*ja, idx, nw, jp.v, jp_of, m.hin);
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch(m, vfe_prelude_kernel, nw, NT, nw, vp.dev(m)));
        RC(launch(m, vfe_stream_kernel, sg.v.size(), NT, nw, vp.dev(m), sg.dev(m)));
        RC(launch(m, vfe_final_kernel, nw, NT, nw, vp.dev(m)));
        if (go) {
            RC(launch(m, vfe_gmm_kernel, nw, NT, nw, vp.dev(m), vg.dev(m)));
            RC(launch(m, vfe_gstream_kernel, sg.v.size(), NT, nw, vp.dev(m), vg.dev(m), sg.dev(m)));
            RC(launch(m, vfe_gfinish_kernel, nw, NT, nw, vp.dev(m), vg.dev(m)));
        }
        if (pa && !ps.v.empty()) {
            if ((pa->what & 2) || strips) RC(launch(m, vfe_pprep_kernel, nw, NT, nw, vp.dev(m), vq.dev(m)));
            for (size_t s0 = 0; s0 < ps.v.size(); s0 += VFE_PRED_LAUNCH_SEGS)
                RC(launch(m, strips ? vfe_predict_kernel<false, true> : pa->grad ? vfe_predict_kernel<true> : vfe_predict_kernel<false>,
                          std::min<size_t>(VFE_PRED_LAUNCH_SEGS, ps.v.size() - s0), NT, nw, vp.dev(m), vq.dev(m), ps.dev(m, s0)));
            if (!jtiles.v.empty()) RC(launch(m, vfe_jcov_kernel, jtiles.v.size(), GNT, nw, vp.dev(m), jp.dev(m), jtiles.dev(m)));
            if (ja && ja->want_fact() && !jp.v.empty()) RC(launch(m, batch_jfact_kernel, jp.v.size(), NT, nw, jp.dev(m)));
        }
        return m.download_and_sync();
    }));
    (go ? c->vfe_grad_batch_problems : !pa ? c->vfe_batch_problems : ja ? c->vfe_joint_batch_problems : pa->grad ? c->vfe_predict_grad_batch_problems : c->vfe_predict_batch_problems) += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const VfeProb& p = vp.v[t];
        put_result(a, b, m.hout[t], (int32_t)m.hout[nw + t]);
        if (p.alpha_off >= 0 && a.ab(b)) std::memcpy(a.ab(b), m.hout + p.alpha_off, sizeof(double) * p.m);
        if (p.meps_off >= 0) std::memcpy(a.eb(b), m.hout + p.meps_off, sizeof(double) * p.m);
        if (first_seg[t] >= 0) {  // failure is data: the prediction kernels skipped the problem
            const VfePSeg& s = ps.v[first_seg[t]];
            const bool failed = m.hout[nw + t] != 0.0;
            for (int side = 1; side <= 2; ++side) {
                void* out = pa->out_b(side == 1 ? pa->mean_out : pa->var_out, side, b);
                if (!out) continue;
                if (failed) fill_nan(out, 0, s.ns);
                else std::memcpy(out, m.hout + (side == 1 ? s.mean_off : s.var_off), sizeof(double) * s.ns);
            }
            for (int side = 1; side <= 2; ++side) {  // the gradients: [d][ns] -> the container layout of xs
                void* out = pa->out_b(side == 1 ? pa->dmean_out : pa->dvar_out, side, b);
                if (!out) continue;
                if (failed) fill_nan(out, 0, (long)s.ns * p.d);
                else grad_to_layout<double>(pa->xsb(b).layout, s.ns, p.d, m.hout + (side == 1 ? s.dmean_off : s.dvar_off), s.ns, out);
            }
        }
        if (ja && ja->info_joint) ja->info_joint[b] = 0;
        if (jp_of[t] >= 0) {  // the kernels wrote the NaN of a failed fit, and of a failed joint factorisation, themselves
            const JointProb& j = jp.v[(size_t)jp_of[t]];
            if (void* co = ja->out_b(ja->cov_out, 4, b)) std::memcpy(co, m.hout + j.cov_off, sizeof(double) * (size_t)j.ns * j.ns);
            if (j.jr_off >= 0) {
                if (ja->what & 8) ((double*)ja->hlogpdf_out)[b] = m.hout[j.jr_off];
                if (ja->info_joint) ja->info_joint[b] = (int32_t)m.hout[j.jr_off + 1];
            }
            if (void* so = ja->out_b(ja->samples_out, 16, b)) std::memcpy(so, m.hout + j.samp_off, sizeof(double) * (size_t)ja->draws(b));
        }
        if (!go) continue;
        if (m.hout[nw + t] != 0.0) {  // failure is data: the gradient kernels skipped the problem
            vfe_grad_fill_nan(a, *go, b);
            continue;
        }
        const VfeGrad& q = vg.v[t];
        const double* gh = m.hout + q.gh_off;
        go->dvar[b] = gh[0];
        if (go->dscale && p.nscale > 0) std::memcpy(go->dscale[b], gh + 1, sizeof(double) * p.nscale);
        if (q.dn_off >= 0) std::memcpy(go->dnoise[b], m.hout + q.dn_off, sizeof(double) * p.n);
        else *(double*)go->dnoise[b] = gh[17];
        std::memcpy(go->dy[b], m.hout + q.dy_off, sizeof(double) * p.n);
        if (go->dz) grad_to_layout<double>(a.zb(b).layout, p.m, p.d, m.hout + q.dz_off, p.m, go->dz[b]);  // [d][m] -> the container layout of z
        if (go->dx) grad_to_layout<double>(a.xb(b).layout, p.n, p.d, m.hout + q.dx_off, p.n, go->dx[b]);
    }
    return 0;
}

int32_t vfe_batch_impl(gp_ctx* c, VfeArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_vfe_args(a));
    const long max_n = env_capped(getenv("GPMI_VFE_BATCH_MAX_N"), GPMI355_VFE_BATCH_MAX_N, VFE_KERNEL_MAX_N);
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) (vfe_batch_takes(a, b, max_n) ? mine : routed).push_back(b);
    RC(for_each_wave(c, mine, [&](int b) { return WaveCost{sizeof(double) * (size_t)vfe_ws(a, b), 0, sizeof(double) * (size_t)vfe_in(a, b)}; },
                     [&](const int* idx, int nw) { return run_vfe_wave(c, a, idx, nw); }));
    // everything else: gp_vfe_fit + gp_vfe_get + gp_vfe_free, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const bool weights = a.ab(b) || a.eb(b);
        gp_vfe* h = nullptr;
        int32_t rc = gp_vfe_fit(c, &a.k[b], &a.xb(b), &a.zb(b), &a.noise[b], a.jitter[b], a.mb(b), a.yb(b), a.approx[b], weights ? &h : nullptr, logpdf_slot(a, b));
        if (rc == 0 && h) rc = gp_vfe_get(h, a.ab(b), a.eb(b));
        if (h) (void)gp_vfe_free(h);
        RC(routed_done(a, b, rc, [&] {
            fill_nan(a.ab(b), a.dtype, a.zb(b).n);
            fill_nan(a.eb(b), a.dtype, a.zb(b).n);
        }));
    }
    return 0;
}

// gp_vfe_grad_batch: the body of vfe_batch_impl with the gradient behind the fit — three more launches per wave, gp_vfe_grad behind gp_vfe_fit for the rest
int32_t vfe_grad_batch_impl(gp_ctx* c, VfeArgs& a, const VfeGradOut& go) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_vfe_args(a));
    if (!go.dvar) return set_arg_err(16, "dvariance_out is NULL");
    if (!go.dnoise) return set_arg_err(18, "dnoise_out is NULL");
    if (!go.dy) return set_arg_err(19, "dy_out is NULL");
    for (int b = 0; b < a.nb; ++b) {
        if (go.dscale && a.k[b].nscale > 0 && !go.dscale[b]) return set_arg_err(17, "a dscale_out pointer is NULL where the kernel has scales");
        if (!go.dnoise[b]) return set_arg_err(18, "a dnoise_out pointer is NULL");
        if (!go.dy[b]) return set_arg_err(19, "a dy_out pointer is NULL");
        if (go.dz && !go.dz[b]) return set_arg_err(20, "a dz_out pointer is NULL");
        if (go.dx && !go.dx[b]) return set_arg_err(21, "a dx_out pointer is NULL");
    }
    const long max_n = env_capped(getenv("GPMI_VFE_GRAD_BATCH_MAX_N"), GPMI355_VFE_GRAD_BATCH_MAX_N, VFE_KERNEL_MAX_N);
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) (vfe_batch_takes(a, b, max_n) ? mine : routed).push_back(b);
    RC(for_each_wave(c, mine,
                     [&](int b) {  // the staging bound covers what goes in and what comes back
                         return WaveCost{sizeof(double) * (size_t)(vfe_ws(a, b) + vfe_grad_ws(a, b)), 0, sizeof(double) * (size_t)(vfe_in(a, b) + vfe_grad_out(a, go, b))};
                     },
                     [&](const int* idx, int nw) { return run_vfe_wave(c, a, idx, nw, &go); }));
    // everything else: gp_vfe_fit + gp_vfe_grad + gp_vfe_free, one problem at a time, after the lock is released; the single path's rules hold (dz on an
    // fp32 handle is refused there)
    gd.lk.unlock();
    for (int b : routed) {
        const bool diag = a.noise[b].kind == 1;
        gp_vfe* h = nullptr;
        double dns = 0.0;
        int32_t rc = gp_vfe_fit(c, &a.k[b], &a.xb(b), &a.zb(b), &a.noise[b], a.jitter[b], a.mb(b), a.yb(b), a.approx[b], &h, logpdf_slot(a, b));
        if (rc == 0 && h)
            rc = gp_vfe_grad(h, &go.dvar[b], go.dscale ? go.dscale[b] : nullptr, diag ? nullptr : &dns, diag ? go.dnoise[b] : nullptr, go.dy[b],
                             go.dz ? go.dz[b] : nullptr, a.zb(b).layout, go.dx ? go.dx[b] : nullptr, a.xb(b).layout);
        if (h) (void)gp_vfe_free(h);
        if (rc == 0 && !diag) put(go.dnoise[b], a.dtype, 0, dns);
        RC(routed_done(a, b, rc, [&] { vfe_grad_fill_nan(a, go, b); }));
    }
    return 0;
}

// doubles problem b alone adds to the workspace (the strip L_D⁻ᵀ) and to the page-locked staging of a prediction wave (its test points where they are not
// shared, prior mean, segment table, α, mean and variance and, with gradients, d entries per test point and side)
long vfe_predict_ws(const VfePredictArgs& a, int b) {
    const long np = batch_np(a.zb(b).n);
    return ((a.what & 2) && a.xsb(b).n > 0) ? np * batch_ld(np) : 0;
}
long vfe_predict_io(const VfePredictArgs& a, int b) {
    const gp_points& xs = a.xsb(b);
    const long nseg = (xs.n + vfe_pseg() - 1) / vfe_pseg();
    return a.zb(b).n + (a.nxs == 1 ? 0 : (long)xs.d * xs.n) + (a.pmb(b) ? xs.n : 0) + nseg * (long)(sizeof(VfePSeg) / 8) +
           ((a.what & 1) + (a.what >> 1)) * xs.n * (a.grad ? 1 + xs.d : 1);
}

// the test side of gp_vfe_predict_batch / gp_vfe_predict_grad_batch that needs neither the handle nor a device (arguments 14 … 19, … 21 with gradients)
int32_t check_vfe_test_head(const VfePredictArgs& a) {
    RC(check_test_head(a, 14));
    if (a.what <= 0 || a.what > 3) return set_arg_err(17, "what must be a combination of 1|2");
    if ((a.what & 1) && !a.mean_out && !a.dmean_out) return set_arg_err(18, a.grad ? "mean_out and dmean_out are both NULL" : "mean_out is NULL");
    if ((a.what & 2) && !a.var_out && !a.dvar_out) return set_arg_err(19, a.grad ? "var_out and dvar_out are both NULL" : "var_out is NULL");
    return 0;
}

// NaN in every output of problem b that the call was given (the call's dtype: a routed fp32 problem has float arrays)
void vfe_predict_fill_nan(const VfePredictArgs& a, int b) {
    const gp_points& xs = a.xsb(b);
    if (xs.n <= 0) return;
    fill_nan(a.out_b(a.mean_out, 1, b), a.dtype, xs.n);
    fill_nan(a.out_b(a.var_out, 2, b), a.dtype, xs.n);
    fill_nan(a.out_b(a.dmean_out, 1, b), a.dtype, xs.n * xs.d);
    fill_nan(a.out_b(a.dvar_out, 2, b), a.dtype, xs.n * xs.d);
}

// gp_vfe_predict_batch: the body of vfe_batch_impl with the predictions behind the fit — two more launches per wave, gp_vfe_predict behind gp_vfe_fit for the rest.
// gp_vfe_predict_grad_batch (a.grad): the same body with the gradient variant of the predict kernel and gp_vfe_predict_grad for the rest.
int32_t vfe_predict_batch_impl(gp_ctx* c, VfePredictArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_vfe_args(a, 0, a.grad ? 23 : 21));
    const bool m1 = (a.what & 1) != 0, m2 = (a.what & 2) != 0;
    RC(check_test_points(a, nullptr, {{a.mean_out, m1, 18, "a mean_out pointer is NULL"}, {a.var_out, m2, 19, "a var_out pointer is NULL"},
                                      {a.dmean_out, m1, 20, "a dmean_out pointer is NULL"}, {a.dvar_out, m2, 21, "a dvar_out pointer is NULL"}}, 15));
    const long max_n = a.grad ? env_capped(getenv("GPMI_VFE_PREDICT_GRAD_BATCH_MAX_N"), GPMI355_VFE_PREDICT_GRAD_BATCH_MAX_N, VFE_KERNEL_MAX_N)
                              : env_capped(getenv("GPMI_VFE_PREDICT_BATCH_MAX_N"), GPMI355_VFE_PREDICT_BATCH_MAX_N, VFE_KERNEL_MAX_N);
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) (vfe_batch_takes(a, b, max_n) ? mine : routed).push_back(b);
    RC(for_each_wave(c, mine,
                     [&](int b) {  // the staging bound covers what goes in and what comes back
                         return WaveCost{sizeof(double) * (size_t)(vfe_ws(a, b) + vfe_predict_ws(a, b)), 0, sizeof(double) * (size_t)(vfe_in(a, b) + vfe_predict_io(a, b))};
                     },
                     [&](const int* idx, int nw) { return run_vfe_wave(c, a, idx, nw, nullptr, &a); }));
    // everything else: gp_vfe_fit + gp_vfe_predict (gp_vfe_predict_grad) + gp_vfe_free, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    for (int b : routed) {
        const gp_points& xs = a.xsb(b);
        gp_vfe* h = nullptr;
        int32_t rc = gp_vfe_fit(c, &a.k[b], &a.xb(b), &a.zb(b), &a.noise[b], a.jitter[b], a.mb(b), a.yb(b), a.approx[b], xs.n > 0 ? &h : nullptr, logpdf_slot(a, b));
        if (rc == 0 && h)
            rc = a.grad ? gp_vfe_predict_grad(h, &xs, a.pmb(b), a.what, a.out_b(a.mean_out, 1, b), a.out_b(a.var_out, 2, b), a.out_b(a.dmean_out, 1, b),
                                              a.out_b(a.dvar_out, 2, b))
                        : gp_vfe_predict(h, &xs, a.pmb(b), a.what, a.out_b(a.mean_out, 1, b), a.out_b(a.var_out, 2, b), nullptr);
        if (h) (void)gp_vfe_free(h);
        RC(routed_done(a, b, rc, [&] { vfe_predict_fill_nan(a, b); }));
    }
    return 0;
}

// ---- gp_vfe_joint_batch ------------------------------------------------------------------------------------------------------------------------------------
// the test side of gp_vfe_joint_batch that needs neither the handle nor a device (arguments 14 … 25), in the order of joint_batch_impl's checks
int32_t check_vfe_joint_head(const VfeJointArgs& a) {
    RC(check_test_head(a, 14));
    if (a.what <= 0 || (a.what & ~29)) return set_arg_err(18, "what must be a combination of 1|4|8|16 (marginal variances: gp_vfe_predict_batch)");
    if ((a.what & 1) && !a.mean_out) return set_arg_err(19, "mean_out is NULL");
    if ((a.what & 4) && !a.cov_out) return set_arg_err(20, "cov_out is NULL");
    if ((a.what & 8) && !a.ys) return set_arg_err(21, "ys array is NULL");
    if ((a.what & 8) && !a.hlogpdf_out) return set_arg_err(22, "hlogpdf_out is NULL");
    if (a.nsamp < 0) return set_arg_err(23, "nsamp must be >= 0");
    if ((a.what & 16) && a.nsamp > 0 && !a.xi) return set_arg_err(24, "xi array is NULL");
    if ((a.what & 16) && a.nsamp > 0 && !a.samples_out) return set_arg_err(25, "samples_out is NULL");
    return 0;
}

// doubles problem b alone adds to the workspace (the strip L_D⁻ᵀ, the strips of B* and C*, the joint slice) and to the page-locked staging of a joint wave
// (what vfe_predict_io counts for the mean, then y*, ξ and a diagonal Σy* going in, covariance, status pair and draws coming back, and the tile table)
long vfe_joint_ws(const VfeJointArgs& a, int b) {
    const long ns = a.xsb(b).n, np = batch_np(a.zb(b).n);
    if (ns == 0 || !a.want_strips()) return 0;
    return np * batch_ld(np) + 2 * ((ns + VT - 1) / VT * VT) * batch_ld(np) + (a.want_fact() ? batch_slice(ns) : 0);
}
long vfe_joint_io(const VfeJointArgs& a, int b) {
    const gp_points& xs = a.xsb(b);
    const long ns = xs.n, nseg = (ns + vfe_pseg() - 1) / vfe_pseg(), nts = batch_np(ns) / BT;
    return a.zb(b).n + (a.nxs == 1 ? 0 : (long)xs.d * ns) + (a.pmb(b) ? ns : 0) + nseg * (long)(sizeof(VfePSeg) / 8) + 3 * ns + ((a.what & 4) ? ns * ns : 0) + 2 * a.draws(b) + 2 +
           (long)(sizeof(JointProb) / 8) + nts * (nts + 1) / 2 * (long)(sizeof(GradTile) / 8);
}

// gp_vfe_joint_batch: the body of vfe_predict_batch_impl with the joint side behind the predictions — the strip-writing predict kernel, vfe_jcov_kernel and
// batch_jfact_kernel per wave; gp_vfe_fit + gp_vfe_predict (bits 0 and 2) + gp_vfe_logpdf + gp_vfe_rand + gp_vfe_free for the rest
int32_t vfe_joint_batch_impl(gp_ctx* c, VfeJointArgs& a) {
    Guard gd(c);
    if (!gd.ok) return set_arg_err(1, "not a live gp_ctx");
    if (a.nb < 0) return set_arg_err(2, "nb must be >= 0");
    if (a.nb == 0) return 0;
    RC(check_vfe_args(a, 0, 27));
    const bool sampling = (a.what & 16) && a.nsamp > 0;
    RC(check_test_points(a, a.noise_xs, {{a.mean_out, (a.what & 1) != 0, 19, "a mean_out pointer is NULL"}, {a.cov_out, (a.what & 4) != 0, 20, "a cov_out pointer is NULL"},
                                         {a.ys, (a.what & 8) != 0, 21, "a ys pointer is NULL"}, {a.xi, sampling, 24, "a xi pointer is NULL"},
                                         {a.samples_out, sampling, 25, "a samples_out pointer is NULL"}}, 15, 17));
    // which path serves a problem depends on that problem alone: gp_vfe_batch's routing under the joint limits, and a Σy* the kernels take
    const long max_n = env_capped(getenv("GPMI_VFE_JOINT_BATCH_MAX_N"), GPMI355_VFE_JOINT_BATCH_MAX_N, VFE_KERNEL_MAX_N);
    const long max_ns = env_capped(getenv("GPMI_VFE_JOINT_BATCH_MAX_NS"), GPMI355_VFE_JOINT_BATCH_MAX_NS);
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) {
        const bool nz_ok = !a.noise_xs || a.xsb(b).n == 0 || a.noise_xs[b].kind <= 1;
        (vfe_batch_takes(a, b, max_n) && a.xsb(b).n <= max_ns && nz_ok ? mine : routed).push_back(b);
    }
    RC(for_each_wave(c, mine,
                     [&](int b) {  // the staging bound covers what goes in and what comes back
                         return WaveCost{sizeof(double) * (size_t)(vfe_ws(a, b) + vfe_joint_ws(a, b)), 0, sizeof(double) * (size_t)(vfe_in(a, b) + vfe_joint_io(a, b))};
                     },
                     [&](const int* idx, int nw) { return run_vfe_wave(c, a, idx, nw, nullptr, &a, &a); }));
    // everything else: the single-path sequence, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    const gp_noise zero_noise{0, 0.0, nullptr};
    for (int b : routed) {
        const gp_points& xs = a.xsb(b);
        const gp_noise* nz = a.noise_xs ? &a.noise_xs[b] : &zero_noise;
        gp_vfe* h = nullptr;
        int32_t rj = 0;
        int32_t rc = gp_vfe_fit(c, &a.k[b], &a.xb(b), &a.zb(b), &a.noise[b], a.jitter[b], a.mb(b), a.yb(b), a.approx[b], xs.n > 0 ? &h : nullptr, logpdf_slot(a, b));
        if (rc == 0 && h && (a.what & 5)) rc = gp_vfe_predict(h, &xs, a.pmb(b), a.what & 5, a.out_b(a.mean_out, 1, b), nullptr, a.out_b(a.cov_out, 4, b));
        if (rc == 0 && h && (a.what & 8)) {
            rj = gp_vfe_logpdf(h, &xs, a.pmb(b), nz, a.ys[b], xs.n, 1, (char*)a.hlogpdf_out + a.esize() * (size_t)b);
            if (rj < 0) rc = rj;
        }
        if (rc == 0 && rj == 0 && h && a.draws(b) > 0) {
            rj = gp_vfe_rand(h, &xs, a.pmb(b), nz, a.xi[b], a.nsamp, a.samples_out[b]);
            if (rj < 0) rc = rj;
        }
        if (h) (void)gp_vfe_free(h);
        RC(routed_done(a, b, rc, [&] {
            if (xs.n <= 0) return;
            fill_nan(a.out_b(a.mean_out, 1, b), a.dtype, xs.n);
            fill_nan(a.out_b(a.cov_out, 4, b), a.dtype, xs.n * xs.n);
        }));
        if (a.info_joint) a.info_joint[b] = rc == 0 ? rj : 0;
        if ((rc > 0 || rj > 0) && xs.n > 0) joint_fill_nan(a, b);
    }
    return 0;
}

}  // namespace

// The two entry points of a pair (gp_kernel / gp_ksum descriptors) have the same body: base_args() files `k` by its type.  The check of `k` stands in front of
// the body: it reports argument 3 before the handle is looked at.
extern "C" {

int32_t gp_logpdf_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                        const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                        void* const* alpha_out_or_null) {
    BatchArgs a = base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, alpha_out_or_null);
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return batch_impl(ctx, a);
}

int32_t gp_logpdf_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                            const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                            void* const* alpha_out_or_null) {
    BatchArgs a = base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, alpha_out_or_null);
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return batch_impl(ctx, a);
}

int32_t gp_predict_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                         const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                         void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what, mean_out, var_out};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_batch_impl(ctx, a);
}

int32_t gp_predict_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                             const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                             void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what, mean_out, var_out};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_batch_impl(ctx, a);
}

int32_t gp_predict_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                              const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                              void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what,
                  mean_out_or_null, var_out_or_null, true, dmean_out_or_null, dvar_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_grad_batch_impl(ctx, a);
}

int32_t gp_predict_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                  const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                                  const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                                  void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what,
                  mean_out_or_null, var_out_or_null, true, dmean_out_or_null, dvar_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_grad_batch_impl(ctx, a);
}

int32_t gp_joint_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                       const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                       const void* const* prior_mean_xs_or_null, const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null,
                       void* const* cov_out_or_null, const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp, const void* const* xi_or_null,
                       void* const* samples_out_or_null, void* logpdf_out_or_null, int32_t* info_out, int32_t* info_joint_out_or_null) {
    JointArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what, mean_out_or_null, nullptr},
                noise_xs_or_null, cov_out_or_null, ys_or_null, hlogpdf_out_or_null, nsamp, xi_or_null, samples_out_or_null, info_joint_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return joint_batch_impl(ctx, a);
}

int32_t gp_joint_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                           const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                           const void* const* prior_mean_xs_or_null, const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null,
                           void* const* cov_out_or_null, const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp,
                           const void* const* xi_or_null, void* const* samples_out_or_null, void* logpdf_out_or_null, int32_t* info_out,
                           int32_t* info_joint_out_or_null) {
    JointArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out), nxs, xs, prior_mean_xs_or_null, what, mean_out_or_null, nullptr},
                noise_xs_or_null, cov_out_or_null, ys_or_null, hlogpdf_out_or_null, nsamp, xi_or_null, samples_out_or_null, info_joint_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return joint_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                             double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                             void* const* dy_out_or_null) {
    GradArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out), dvariance_out_or_null, dscale_out_or_null, nullptr, dnoise_out_or_null, dy_out_or_null, 12};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return grad_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                 const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                 double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null) {
    GradArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out), nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null, dy_out_or_null, 12};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return grad_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_x(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                               const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                               double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                               void* const* dy_out_or_null, void* const* dx_out_or_null) {
    GradArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out), dvariance_out_or_null, dscale_out_or_null, nullptr, dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return gradx_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_sum_x(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                   const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                   double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                                   void* const* dx_out_or_null) {
    GradArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out), nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return gradx_batch_impl(ctx, a);
}

int32_t gp_loo_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                     const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                     void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null) {
    LooArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out), nullptr, nullptr, nullptr, nullptr, nullptr, 12}, false,
              lp_out_or_null, mean_out_or_null, var_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_batch_impl(ctx, a);
}

int32_t gp_loo_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                         void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null) {
    LooArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out), nullptr, nullptr, nullptr, nullptr, nullptr, 12}, false,
              lp_out_or_null, mean_out_or_null, var_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_batch_impl(ctx, a);
}

int32_t gp_loo_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                          const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                          double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                          void* const* dy_out_or_null, void* const* dx_out_or_null) {
    LooArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out), dvariance_out_or_null, dscale_out_or_null, nullptr,
               dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null}, true};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_grad_batch_impl(ctx, a);
}

int32_t gp_loo_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                              double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                              void* const* dx_out_or_null) {
    LooArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out), nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null,
               dy_out_or_null, 12, dx_out_or_null}, true};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_grad_batch_impl(ctx, a);
}

int32_t gp_vfe_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, int32_t nz, const gp_points* z,
                     const gp_noise* noise, const double* jitter, const void* const* mean_or_null, int32_t ny, const void* const* y,
                     const int32_t* approx, void* objective_out, int32_t* info_out, void* const* alpha_out_or_null, void* const* m_eps_out_or_null) {
    VfeArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, objective_out, info_out, alpha_out_or_null), nz, z, jitter, approx, m_eps_out_or_null};
    return vfe_batch_impl(ctx, a);
}

int32_t gp_vfe_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, int32_t nz, const gp_points* z,
                          const gp_noise* noise, const double* jitter, const void* const* mean_or_null, int32_t ny, const void* const* y,
                          const int32_t* approx, void* objective_out, int32_t* info_out, double* dvariance_out, double* const* dscale_out_or_null,
                          void* const* dnoise_out, void* const* dy_out, double* const* dz_out_or_null, void* const* dx_out_or_null) {
    VfeArgs a{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, objective_out, info_out), nz, z, jitter, approx, nullptr};
    return vfe_grad_batch_impl(ctx, a, VfeGradOut{dvariance_out, dscale_out_or_null, dnoise_out, dy_out, dz_out_or_null, dx_out_or_null});
}

// The checks of the test side stand in front of the body: they report their arguments before the handle is looked at.
int32_t gp_vfe_predict_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, int32_t nz, const gp_points* z,
                             const gp_noise* noise, const double* jitter, const void* const* mean_or_null, int32_t ny, const void* const* y,
                             const int32_t* approx, int32_t nxs, const gp_points* xs, const void* const* prior_mean_xs_or_null, int32_t what,
                             void* const* mean_out, void* const* var_out, void* objective_out_or_null, int32_t* info_out) {
    VfePredictArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, objective_out_or_null, info_out), nz, z, jitter, approx, nullptr},
                     nxs, xs, prior_mean_xs_or_null, what, mean_out, var_out};
    if (nb > 0) RC(check_vfe_test_head(a));
    return vfe_predict_batch_impl(ctx, a);
}

int32_t gp_vfe_predict_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, int32_t nz, const gp_points* z,
                                  const gp_noise* noise, const double* jitter, const void* const* mean_or_null, int32_t ny, const void* const* y,
                                  const int32_t* approx, int32_t nxs, const gp_points* xs, const void* const* prior_mean_xs_or_null, int32_t what,
                                  void* const* mean_out_or_null, void* const* var_out_or_null, void* const* dmean_out_or_null, void* const* dvar_out_or_null,
                                  void* objective_out_or_null, int32_t* info_out) {
    VfePredictArgs a{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, objective_out_or_null, info_out), nz, z, jitter, approx, nullptr},
                     nxs, xs, prior_mean_xs_or_null, what, mean_out_or_null, var_out_or_null, true, dmean_out_or_null, dvar_out_or_null};
    if (nb > 0) RC(check_vfe_test_head(a));
    return vfe_predict_batch_impl(ctx, a);
}

int32_t gp_vfe_joint_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, int32_t nz, const gp_points* z,
                           const gp_noise* noise, const double* jitter, const void* const* mean_or_null, int32_t ny, const void* const* y,
                           const int32_t* approx, int32_t nxs, const gp_points* xs, const void* const* prior_mean_xs_or_null,
                           const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* cov_out_or_null,
                           const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp, const void* const* xi_or_null,
                           void* const* samples_out_or_null, void* objective_out_or_null, int32_t* info_out, int32_t* info_joint_out_or_null) {
    VfeJointArgs a{{{base_args(nb, k, nx, x, noise, mean_or_null, ny, y, objective_out_or_null, info_out), nz, z, jitter, approx, nullptr},
                    nxs, xs, prior_mean_xs_or_null, what, mean_out_or_null, nullptr},
                   noise_xs_or_null, cov_out_or_null, ys_or_null, hlogpdf_out_or_null, nsamp, xi_or_null, samples_out_or_null, info_joint_out_or_null};
    if (nb > 0) RC(check_vfe_joint_head(a));
    return vfe_joint_batch_impl(ctx, a);
}
}
