// batch.hip — many small exact GPs in one call: gp_logpdf_batch / gp_logpdf_batch_sum, gp_predict_batch / gp_predict_batch_sum, gp_logpdf_grad_batch /
// gp_logpdf_grad_batch_sum, gp_predict_grad_batch / gp_predict_grad_batch_sum, gp_joint_batch / gp_joint_batch_sum (include/gpmi355.h) and the kernels behind them: the fit (batch_logpdf_kernel,
// below), the predictions at each problem's test points from the slices it leaves (batch_predict_kernel, further down), the gradient of logpdf from the same
// slices (batch_inv_kernel, batch_grad_kernel, batch_gsum_kernel, behind it; with the input gradient of gp_logpdf_grad_batch_x / gp_logpdf_grad_batch_sum_x:
// batch_gradx_kernel, batch_gxsum_kernel) and the gradients of the predictions w.r.t. the test inputs from the strips the predict kernel leaves and the S of
// batch_inv_kernel (batch_pgrad_kernel), last the joint predictive distribution from the same strips (batch_jcov_kernel, batch_jfact_kernel).
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
struct JointProb {
    long v_off, js_off, cov_off, mean_off, samp_off, jr_off, xs_off, ysd_off, nzs_off, xi_off;
    int prob, ns, nsp, nsamp;
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
    const BatchProb& P = reinterpret_cast<const BatchProb*>(in)[J.prob];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = J.ns, nsp = J.nsp, nsamp = J.nsamp;
    const long lds = batch_ld(nsp);
    double* __restrict__ A = ws + J.js_off;
    double* __restrict__ out = J.samp_off >= 0 ? res + J.samp_off : nullptr;
    double* __restrict__ jr = res + J.jr_off;
    const bool fit_failed = res[nw + P.slot] != 0.0;  // the same value in every thread
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

// a size limit of the header; the environment variable read at the call site overrides it for measurements (0 … what the kernels admit)
long env_capped(const char* env, long deflt) { return std::max(0L, std::min<long>(env ? atol(env) : deflt, BATCH_KERNEL_MAX_N)); }
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

// The launches of a wave on the ctx's main stream, the <SUM> dispatch of each kernel in one place (ks: the call brought composite kernels).
int32_t launch_fit(const WaveMem& m, bool ks, int nw) {
    hipLaunchKernelGGL(ks ? batch_logpdf_kernel<true> : batch_logpdf_kernel<false>, dim3((unsigned)nw), dim3(NT), 0, m.c->sm, m.in, m.ws, m.res, nw);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t launch_predict(const WaveMem& m, bool ks, int nw, const BatchTile* tiles, size_t ntiles) {
    hipLaunchKernelGGL(ks ? batch_predict_kernel<true> : batch_predict_kernel<false>, dim3((unsigned)ntiles), dim3(NT), 0, m.c->sm, m.in, m.ws, m.res, nw, tiles);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t launch_pgrad(const WaveMem& m, bool ks, int nw, const BatchTile* tiles, const PGradTile* ptiles, size_t ntiles) {
    hipLaunchKernelGGL(ks ? batch_pgrad_kernel<true> : batch_pgrad_kernel<false>, dim3((unsigned)ntiles), dim3(ks ? PGNT_SUM : NT), 0, m.c->sm, m.in, m.ws, m.res, nw, tiles, ptiles);
    HIPCHK(hipGetLastError());
    return 0;
}
// lps: the LooProb table of a gp_loo_grad_batch wave (the weights of the leave-one-out objective), or NULL (those of logpdf)
int32_t launch_grad(const WaveMem& m, bool ks, int nw, const GradProb* gps, const GradTile* tiles, size_t ntiles, const LooProb* lps = nullptr) {
    auto kern = lps ? (ks ? batch_grad_kernel<true, true> : batch_grad_kernel<false, true>) : (ks ? batch_grad_kernel<true, false> : batch_grad_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(GNT), 0, m.c->sm, m.in, m.ws, m.res, nw, gps, tiles, lps);
    HIPCHK(hipGetLastError());
    return 0;
}
int32_t launch_gradx(const WaveMem& m, bool ks, int nw, const GradProb* gps, const GradXProb* gxs, const GradTile* tiles, size_t ntiles) {
    hipLaunchKernelGGL(ks ? batch_gradx_kernel<true> : batch_gradx_kernel<false>, dim3((unsigned)ntiles), dim3(GNT), 0, m.c->sm, m.in, m.ws, (const double*)m.res, nw, gps, gxs, tiles);
    HIPCHK(hipGetLastError());
    return 0;
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

// workspace bytes of one problem: `own` adds up over a wave, `shared` is needed once per wave, as wide as the widest problem asks for
struct WaveCost { size_t own, shared; };
// The kernel's problems in waves bounded by the launch size and by the workspace budget (a wave holds at least one problem); run(idx, nw) serves one wave.
template <class Cost, class Run> int32_t for_each_wave(gp_ctx* c, const std::vector<int>& mine, Cost&& cost, Run&& run) {
    if (mine.empty()) return 0;
    HIPCHK(hipSetDevice(c->device));
    for (size_t i = 0, j; i < mine.size(); i = j) {
        size_t own = 0, shared = 0;
        for (j = i; j < mine.size() && j - i < BATCH_WAVE_PROBLEMS; ++j) {
            const WaveCost w = cost(mine[j]);
            if (j > i && own + w.own + std::max(shared, w.shared) > BATCH_WS_BYTES) break;
            own += w.own;
            shared = std::max(shared, w.shared);
        }
        RC(run(mine.data() + i, (int)(j - i)));
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
            rc = a.ks ? gp_posterior_fit_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, a.ab(b), lp)
                      : gp_posterior_fit(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, a.ab(b), lp);
            if (post) (void)gp_posterior_free(post);
        } else {
            rc = a.ks ? gp_logpdf_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), x.n, 1, lp)
                      : gp_logpdf(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), x.n, 1, lp);
        }
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            fill_nan(a.ab(b), a.dtype, x.n);
        }
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
    // behind the fit's input: the test points (dimension-major, a shared set once), then the tile table; behind its results: mean and var of every problem
    std::vector<long> xs_off((size_t)nw, -1), mean_off((size_t)nw, -1), var_off((size_t)nw, -1), dmean_off((size_t)nw, -1), dvar_off((size_t)nw, -1);
    SharedOnce xso{a.nxs == 1}, xsf{a.nxs == 1};  // layout, filling
    for (int t = 0; t < nw; ++t) {
        const gp_points& xs = a.xsb(idx[t]);
        if (xs.n == 0) continue;
        xs_off[t] = xso.place(L.off, (long)xs.d * xs.n);
        if (a.what & 1) mean_off[t] = take(L.roff, xs.n);
        if (a.what & 2) var_off[t] = take(L.roff, xs.n);
        if (a.want_dmean()) dmean_off[t] = take(L.roff, (long)xs.d * xs.n);
        if (a.want_dvar()) dvar_off[t] = take(L.roff, (long)xs.d * xs.n);
    }
    // a gradient call: the S strips beside the slices, their tiles of 128 rows and the table batch_inv_kernel reads (built as run_grad_wave builds them)
    std::vector<GradProb> gp(a.grad ? (size_t)nw : 0, GradProb{-1, -1, -1, -1, 0, 0});
    std::vector<GradTile> itiles;
    for (int s = 0; s < nw && a.grad; ++s) {
        const int t = L.order[s];
        const BatchProb& p = L.pr[t];
        if (pgrad_s(a, idx[t]) == 0) continue;
        gp[s].s_off = take(L.ws, (long)p.np * p.ld);
        for (int r0 = 0; r0 < p.np; r0 += TP) itiles.push_back(GradTile{s, r0 / TP, 0, 0});
    }
    // tiles of TP test points, the widest problems first; a launch closes at BATCH_PRED_TILES tiles or when its strips would pass the workspace budget
    std::vector<BatchTile> tiles;
    std::vector<PGradTile> ptiles;
    std::vector<size_t> launch_end;
    long cur = L.ws, ws_top = L.ws;
    size_t launch_begin = 0;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s];
        const long ns = a.xsb(idx[t]).n, strip = predict_strip(a, L.pr[t].n);
        for (long row0 = 0; row0 < ns; row0 += TP) {
            if (tiles.size() > launch_begin &&
                (tiles.size() - launch_begin == BATCH_PRED_TILES || sizeof(double) * (size_t)(cur + strip) > BATCH_WS_BYTES)) {
                launch_end.push_back(tiles.size());
                launch_begin = tiles.size();
                cur = L.ws;  // the launches of a wave run one after the other on one stream: they share the strips
            }
            BatchTile tl{xs_off[t], cur, mean_off[t], var_off[t], L.pos[t], (int)ns, (int)row0, (int)std::min<long>(TP, ns - row0)};
            tiles.push_back(tl);
            if (a.grad) ptiles.push_back(PGradTile{gp[s].s_off, dmean_off[t], dvar_off[t]});
            cur += strip;
            ws_top = std::max(ws_top, cur);
        }
    }
    if (tiles.size() > launch_begin) launch_end.push_back(tiles.size());
    const long tile_off = take(L.off, (long)(tiles.size() * sizeof(BatchTile) / 8));
    const long pt_off = take(L.off, (long)(ptiles.size() * sizeof(PGradTile) / 8));
    const long gp_off = take(L.off, (long)(gp.size() * sizeof(GradProb) / 8));
    const long it_off = take(L.off, (long)(itiles.size() * sizeof(GradTile) / 8));

    WaveMem m(c);
    RC(m.alloc(L.off, ws_top, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    for (int t = 0; t < nw; ++t) {
        const gp_points& xs = a.xsb(idx[t]);
        if (xs.n > 0 && xsf.claim()) pack_points(xs, m.hin + xs_off[t]);
    }
    if (!tiles.empty()) std::memcpy(m.hin + tile_off, tiles.data(), tiles.size() * sizeof(BatchTile));
    if (!ptiles.empty()) std::memcpy(m.hin + pt_off, ptiles.data(), ptiles.size() * sizeof(PGradTile));
    if (!gp.empty()) std::memcpy(m.hin + gp_off, gp.data(), gp.size() * sizeof(GradProb));
    if (!itiles.empty()) std::memcpy(m.hin + it_off, itiles.data(), itiles.size() * sizeof(GradTile));
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        if (!itiles.empty()) {
            hipLaunchKernelGGL(batch_inv_kernel, dim3((unsigned)itiles.size()), dim3(NT), 0, c->sm, m.in, m.ws, (const double*)m.res, nw,
                               reinterpret_cast<const GradProb*>(m.in + gp_off), reinterpret_cast<const GradTile*>(m.in + it_off));
            HIPCHK(hipGetLastError());
        }
        size_t t0 = 0;
        for (size_t t1 : launch_end) {
            const BatchTile* tl = reinterpret_cast<const BatchTile*>(m.in + tile_off) + t0;
            RC(launch_predict(m, a.ks != nullptr, nw, tl, t1 - t0));
            // the strips are shared by the launch groups: the gradients of a group follow its own predict launch and precede the next one
            if (a.want_dmean() || a.want_dvar()) RC(launch_pgrad(m, a.ks != nullptr, nw, tl, reinterpret_cast<const PGradTile*>(m.in + pt_off) + t0, t1 - t0));
            t0 = t1;
        }
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    if (a.grad) c->batch_pgrad_problems += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        const long ns = a.xsb(b).n;
        if (ns == 0) continue;
        if (double* mo = (double*)a.out_b(a.mean_out, 1, b)) {
            const double* pm = (const double*)a.pmb(b);
            for (long j = 0; j < ns; ++j) mo[j] = pm ? pm[j] + hout[mean_off[t] + j] : hout[mean_off[t] + j];
        }
        if (void* vo = a.out_b(a.var_out, 2, b)) std::memcpy(vo, hout + var_off[t], sizeof(double) * (size_t)ns);
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
    if (a.nxs != 1 && a.nxs != a.nb) return set_arg_err(10, "nxs must be 1 (one xs shared by every problem) or nb");
    if (!a.xs) return set_arg_err(11, "test points array is NULL");
    if (a.what <= 0 || a.what > 3) return set_arg_err(13, "what must be a combination of 1|2");
    if ((a.what & 1) && !a.mean_out) return set_arg_err(14, "mean_out is NULL");
    if ((a.what & 2) && !a.var_out) return set_arg_err(15, "var_out is NULL");
    if (!a.info_out) return set_arg_err(17, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    for (int b = 0; b < a.nb; ++b) {
        const gp_points& xs = a.xsb(b);
        if (xs.n < 0) return set_arg_err(11, "xs: n must be >= 0");
        if (xs.n == 0) continue;  // no test points: nothing of this problem's xs or outputs is touched
        RC(check_points(&xs, 11));
        if (xs.d != a.xb(b).d) return set_arg_err(11, "xs has a different D than the training inputs");
        if ((a.what & 1) && !a.mean_out[b]) return set_arg_err(14, "a mean_out pointer is NULL");
        if ((a.what & 2) && !a.var_out[b]) return set_arg_err(15, "a var_out pointer is NULL");
    }
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
        const gp_points& x = a.xb(b);
        const gp_points& xs = a.xsb(b);
        gp_post* post = nullptr;
        void* lp = logpdf_slot(a, b);
        int32_t rc = a.ks ? gp_posterior_fit_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp)
                          : gp_posterior_fit(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp);
        if (rc == 0 && xs.n > 0)
            rc = gp_posterior_predict(post, &xs, a.pmb(b), a.what, (a.what & 1) ? a.mean_out[b] : nullptr, (a.what & 2) ? a.var_out[b] : nullptr, nullptr);
        if (post) (void)gp_posterior_free(post);
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            if (xs.n > 0) {
                if (a.what & 1) fill_nan(a.mean_out[b], a.dtype, xs.n);
                if (a.what & 2) fill_nan(a.var_out[b], a.dtype, xs.n);
            }
        }
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
    if (a.nxs != 1 && a.nxs != a.nb) return set_arg_err(10, "nxs must be 1 (one xs shared by every problem) or nb");
    if (!a.xs) return set_arg_err(11, "test points array is NULL");
    if (a.what <= 0 || a.what > 3) return set_arg_err(13, "what must be a combination of 1|2");
    if ((a.what & 1) && !a.mean_out && !a.dmean_out) return set_arg_err(14, "mean_out and dmean_out are both NULL");
    if ((a.what & 2) && !a.var_out && !a.dvar_out) return set_arg_err(15, "var_out and dvar_out are both NULL");
    if (!a.info_out) return set_arg_err(19, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    for (int b = 0; b < a.nb; ++b) {
        const gp_points& xs = a.xsb(b);
        if (xs.n < 0) return set_arg_err(11, "xs: n must be >= 0");
        if (xs.n == 0) continue;  // no test points: nothing of this problem's xs or outputs is touched
        RC(check_points(&xs, 11));
        if (xs.d != a.xb(b).d) return set_arg_err(11, "xs has a different D than the training inputs");
        if ((a.what & 1) && a.mean_out && !a.mean_out[b]) return set_arg_err(14, "a mean_out pointer is NULL");
        if ((a.what & 2) && a.var_out && !a.var_out[b]) return set_arg_err(15, "a var_out pointer is NULL");
        if ((a.what & 1) && a.dmean_out && !a.dmean_out[b]) return set_arg_err(16, "a dmean_out pointer is NULL");
        if ((a.what & 2) && a.dvar_out && !a.dvar_out[b]) return set_arg_err(17, "a dvar_out pointer is NULL");
    }
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
        const gp_points& x = a.xb(b);
        const gp_points& xs = a.xsb(b);
        gp_post* post = nullptr;
        void* lp = logpdf_slot(a, b);
        int32_t rc = a.ks ? gp_posterior_fit_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp)
                          : gp_posterior_fit(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp);
        if (rc == 0 && xs.n > 0)
            rc = gp_posterior_predict_grad(post, &xs, a.pmb(b), a.what, a.out_b(a.mean_out, 1, b), a.out_b(a.var_out, 2, b), a.out_b(a.dmean_out, 1, b),
                                           a.out_b(a.dvar_out, 2, b));
        if (post) (void)gp_posterior_free(post);
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            pgrad_fill_nan(a, b);
        }
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
    void* out_ptr(void* const* arr, int bit, int b) const { return (arr && (what & bit)) ? arr[b] : nullptr; }
    size_t esize() const { return dtype == 0 ? 8 : 4; }
};

// NaN in the held-out logpdf and the samples of problem b (a joint covariance that is not positive definite, or a failed fit)
void joint_fill_nan(const JointArgs& a, int b) {
    if (a.what & 8) put(a.hlogpdf_out, a.dtype, b, std::numeric_limits<double>::quiet_NaN());
    fill_nan(a.out_ptr(a.samples_out, 16, b), a.dtype, a.draws(b));
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
    std::vector<long> xs_off((size_t)nw, -1), mean_off((size_t)nw, -1), var_off((size_t)nw, -1);
    std::vector<int> jp_of((size_t)nw, -1);
    std::vector<JointProb> jp;
    SharedOnce xso{a.nxs == 1}, xsf{a.nxs == 1};  // layout, filling
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& xs = a.xsb(b);
        const long ns = xs.n;
        if (ns == 0) continue;
        xs_off[t] = xso.place(L.off, (long)xs.d * ns);
        if (a.want_mean()) mean_off[t] = take(L.roff, ns);
        if (!need_v) continue;
        var_off[t] = take(L.roff, ns);  // the variance the predict kernel computes on its way to V: scratch
        JointProb j{};
        j.prob = L.pos[t], j.ns = (int)ns, j.nsp = (int)batch_np(ns), j.nsamp = a.nsamp;
        j.v_off = j.js_off = -1;
        j.xs_off = xs_off[t], j.mean_off = mean_off[t];
        j.cov_off = (a.what & 4) ? take(L.roff, ns * ns) : -1;
        j.jr_off = a.want_fact() ? take(L.roff, 2) : -1;
        j.samp_off = (a.what & 16) ? take(L.roff, a.draws(b)) : -1;
        j.ysd_off = (a.what & 8) ? take(L.off, ns) : -1;
        j.xi_off = (a.what & 16) ? take(L.off, a.draws(b)) : -1;
        const gp_noise* nz = a.noise_xs ? &a.noise_xs[b] : nullptr;
        j.noise_s = nz ? nz->s : 0.0;
        j.nzs_off = (nz && nz->kind == 1) ? take(L.off, ns) : -1;
        jp_of[t] = (int)jp.size();
        jp.push_back(j);
    }
    // a problem's tiles of TP test points lie one after the other, and so do their strips; a predict launch closes at BATCH_PRED_TILES tiles
    std::vector<BatchTile> tiles;
    std::vector<GradTile> jtiles;
    std::vector<size_t> launch_end;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s];
        const long ns = a.xsb(idx[t]).n, strip = need_v ? (long)TP * L.pr[t].ld : 0;
        if (ns == 0) continue;
        if (jp_of[t] >= 0) jp[(size_t)jp_of[t]].v_off = L.ws;
        for (long row0 = 0; row0 < ns; row0 += TP) {
            if (!tiles.empty() && (tiles.size() - (launch_end.empty() ? 0 : launch_end.back())) == BATCH_PRED_TILES) launch_end.push_back(tiles.size());
            tiles.push_back(BatchTile{xs_off[t], take(L.ws, strip), mean_off[t], var_off[t], L.pos[t], (int)ns, (int)row0, (int)std::min<long>(TP, ns - row0)});
        }
        if (jp_of[t] < 0) continue;
        JointProb& j = jp[(size_t)jp_of[t]];
        if (a.want_fact()) j.js_off = take(L.ws, batch_slice(ns));
        for (int ti = 0; ti < j.nsp / BT; ++ti)
            for (int tj = 0; tj <= ti; ++tj) jtiles.push_back(GradTile{jp_of[t], ti, tj, 0});
    }
    if (!tiles.empty()) launch_end.push_back(tiles.size());
    const long tile_off = take(L.off, (long)(tiles.size() * sizeof(BatchTile) / 8));
    const long jp_off = take(L.off, (long)(jp.size() * sizeof(JointProb) / 8));
    const long jt_off = take(L.off, (long)(jtiles.size() * sizeof(GradTile) / 8));

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& xs = a.xsb(b);
        if (xs.n == 0) continue;
        if (xsf.claim()) pack_points(xs, m.hin + xs_off[t]);
        if (jp_of[t] < 0) continue;
        const JointProb& j = jp[(size_t)jp_of[t]];
        if (j.ysd_off >= 0) {
            const double *ys = (const double*)a.ys[b], *pm = (const double*)a.pmb(b);
            for (long i = 0; i < xs.n; ++i) m.hin[j.ysd_off + i] = pm ? ys[i] - pm[i] : ys[i];
        }
        if (j.xi_off >= 0 && a.draws(b) > 0) std::memcpy(m.hin + j.xi_off, a.xi[b], sizeof(double) * (size_t)a.draws(b));
        if (j.nzs_off >= 0) std::memcpy(m.hin + j.nzs_off, a.noise_xs[b].diag, sizeof(double) * (size_t)xs.n);
    }
    if (!tiles.empty()) std::memcpy(m.hin + tile_off, tiles.data(), tiles.size() * sizeof(BatchTile));
    if (!jp.empty()) std::memcpy(m.hin + jp_off, jp.data(), jp.size() * sizeof(JointProb));
    if (!jtiles.empty()) std::memcpy(m.hin + jt_off, jtiles.data(), jtiles.size() * sizeof(GradTile));
    const bool ks = a.ks != nullptr;
    RC(run_drained(c, [&]() -> int32_t {
        RC(m.upload());
        RC(launch_fit(m, ks, nw));
        size_t t0 = 0;
        for (size_t t1 : launch_end) {
            RC(launch_predict(m, ks, nw, reinterpret_cast<const BatchTile*>(m.in + tile_off) + t0, t1 - t0));
            t0 = t1;
        }
        const JointProb* djp = reinterpret_cast<const JointProb*>(m.in + jp_off);
        if (!jtiles.empty()) {
            hipLaunchKernelGGL(ks ? batch_jcov_kernel<true> : batch_jcov_kernel<false>, dim3((unsigned)jtiles.size()), dim3(GNT), 0, c->sm, m.in, m.ws, m.res, nw, djp,
                               reinterpret_cast<const GradTile*>(m.in + jt_off));
            HIPCHK(hipGetLastError());
        }
        if (a.want_fact() && !jp.empty()) {
            hipLaunchKernelGGL(batch_jfact_kernel, dim3((unsigned)jp.size()), dim3(NT), 0, c->sm, m.in, m.ws, m.res, nw, djp);
            HIPCHK(hipGetLastError());
        }
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
        const double* pm = (const double*)a.pmb(b);
        if (double* mo = (double*)a.out_ptr(a.mean_out, 1, b))
            for (long j = 0; j < ns; ++j) mo[j] = pm ? pm[j] + hout[mean_off[t] + j] : hout[mean_off[t] + j];
        if (jp_of[t] < 0) continue;
        const JointProb& j = jp[(size_t)jp_of[t]];
        if (void* co = a.out_ptr(a.cov_out, 4, b)) std::memcpy(co, hout + j.cov_off, sizeof(double) * (size_t)(ns * ns));
        if (j.jr_off >= 0) {
            if (a.what & 8) ((double*)a.hlogpdf_out)[b] = hout[j.jr_off];
            if (a.info_joint) a.info_joint[b] = (int32_t)hout[j.jr_off + 1];
        }
        if (double* so = (double*)a.out_ptr(a.samples_out, 16, b))
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
    if (a.nxs != 1 && a.nxs != a.nb) return set_arg_err(10, "nxs must be 1 (one xs shared by every problem) or nb");
    if (!a.xs) return set_arg_err(11, "test points array is NULL");
    if (a.what <= 0 || (a.what & ~29)) return set_arg_err(14, "what must be a combination of 1|4|8|16 (marginal variances: gp_predict_batch)");
    if ((a.what & 1) && !a.mean_out) return set_arg_err(15, "mean_out is NULL");
    if ((a.what & 4) && !a.cov_out) return set_arg_err(16, "cov_out is NULL");
    if ((a.what & 8) && !a.ys) return set_arg_err(17, "ys array is NULL");
    if ((a.what & 8) && !a.hlogpdf_out) return set_arg_err(18, "hlogpdf_out is NULL");
    if (a.nsamp < 0) return set_arg_err(19, "nsamp must be >= 0");
    if ((a.what & 16) && a.nsamp > 0 && !a.xi) return set_arg_err(20, "xi array is NULL");
    if ((a.what & 16) && a.nsamp > 0 && !a.samples_out) return set_arg_err(21, "samples_out is NULL");
    if (!a.info_out) return set_arg_err(23, "info_out is NULL");
    std::vector<KSum> packed;
    RC(check_batch_problems(a, packed));
    for (int b = 0; b < a.nb; ++b) {
        const gp_points& xs = a.xsb(b);
        if (xs.n < 0) return set_arg_err(11, "xs: n must be >= 0");
        if (xs.n == 0) continue;  // no test points: nothing of this problem's xs or outputs is touched
        RC(check_points(&xs, 11));
        if (xs.d != a.xb(b).d) return set_arg_err(11, "xs has a different D than the training inputs");
        if (a.noise_xs) RC(check_noise(&a.noise_xs[b], 13, true));
        if ((a.what & 1) && !a.mean_out[b]) return set_arg_err(15, "a mean_out pointer is NULL");
        if ((a.what & 4) && !a.cov_out[b]) return set_arg_err(16, "a cov_out pointer is NULL");
        if ((a.what & 8) && !a.ys[b]) return set_arg_err(17, "a ys pointer is NULL");
        if ((a.what & 16) && a.nsamp > 0 && !a.xi[b]) return set_arg_err(20, "a xi pointer is NULL");
        if ((a.what & 16) && a.nsamp > 0 && !a.samples_out[b]) return set_arg_err(21, "a samples_out pointer is NULL");
    }
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
        const gp_points& x = a.xb(b);
        const gp_points& xs = a.xsb(b);
        const gp_noise* nz = a.noise_xs ? &a.noise_xs[b] : &zero_noise;
        gp_post* post = nullptr;
        void* lp = logpdf_slot(a, b);
        int32_t rj = 0;
        int32_t rc = a.ks ? gp_posterior_fit_sum(c, &a.ks[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp)
                          : gp_posterior_fit(c, &a.k[b], &x, &a.noise[b], a.mb(b), a.yb(b), &post, nullptr, lp);
        if (rc == 0 && xs.n > 0 && (a.what & 5))
            rc = gp_posterior_predict(post, &xs, a.pmb(b), a.what & 5, a.out_ptr(a.mean_out, 1, b), nullptr, a.out_ptr(a.cov_out, 4, b));
        if (rc == 0 && xs.n > 0 && (a.what & 8)) {
            rj = gp_posterior_logpdf(post, &xs, a.pmb(b), nz, a.ys[b], xs.n, 1, (char*)a.hlogpdf_out + a.esize() * (size_t)b);
            if (rj < 0) rc = rj;
        }
        if (rc == 0 && rj == 0 && xs.n > 0 && a.draws(b) > 0) {
            rj = gp_posterior_rand(post, &xs, a.pmb(b), nz, a.xi[b], a.nsamp, a.samples_out[b]);
            if (rj < 0) rc = rj;
        }
        if (post) (void)gp_posterior_free(post);
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (a.info_joint) a.info_joint[b] = rc == 0 ? rj : 0;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            if (xs.n > 0) {
                fill_nan(a.out_ptr(a.mean_out, 1, b), a.dtype, xs.n);
                fill_nan(a.out_ptr(a.cov_out, 4, b), a.dtype, xs.n * xs.n);
            }
        }
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

// one wave: the fit launch of the problems idx[0..nw) with α for every one of them, then S = L⁻ᵀ, the tile sums and their totals.  Caller holds the ctx lock.
int32_t run_grad_wave(gp_ctx* c, const GradArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [](int) { return true; }, L);
    // behind the fit's input: the GradProb table (in the order of the descriptors), the tiles of S and the tiles of the triangle, the widest problems first
    std::vector<GradProb> gp((size_t)nw);
    std::vector<GradTile> itiles, gtiles;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s], b = idx[t];
        const BatchProb& p = L.pr[t];
        GradProb& g = gp[s];
        const int nt = p.np / BT;
        g.ng = 1 + grad_nkp(a, packed, b);
        g.ntiles = nt * (nt + 1) / 2;
        g.s_off = take(L.ws, (long)p.np * p.ld);
        g.part_off = take(L.ws, ((long)g.ntiles * g.ng + 1) & ~1L);  // the next strip stays 16-byte aligned
        g.g_off = take(L.roff, g.ng);
        g.dn_off = a.noise[b].kind == 1 ? take(L.roff, p.n) : -1;
        for (int r0 = 0; r0 < p.np; r0 += TP) itiles.push_back(GradTile{s, r0 / TP, 0, 0});
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj <= ti; ++tj) gtiles.push_back(GradTile{s, ti, tj, ti * (ti + 1) / 2 + tj});
    }
    // the problems whose dx is wanted: their tables of row sums behind everything else in the workspace, the gradient [d][n] behind the other results, the
    // tiles of the full square and the 64-row blocks batch_gxsum_kernel adds them up in.  Without any, the wave is laid out and launched as it always was.
    std::vector<GradXProb> gx;
    std::vector<GradTile> xtiles, xrows;
    int nwx = 0;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s], b = idx[t];
        if (!a.dxb(b)) continue;
        if (gx.empty()) gx.assign((size_t)nw, GradXProb{-1, -1});
        const BatchProb& p = L.pr[t];
        const int nt = p.np / BT;
        gx[s].xpart_off = take(L.ws, gradx_part(a, b));
        gx[s].dx_off = take(L.roff, (long)p.n * p.d);
        for (int ti = 0; ti < nt; ++ti) {
            for (int tj = 0; tj < nt; ++tj) xtiles.push_back(GradTile{s, ti, tj, ti * nt + tj});
            xrows.push_back(GradTile{s, ti, 0, 0});
        }
        ++nwx;
    }
    const long gp_off = take(L.off, (long)(gp.size() * sizeof(GradProb) / 8));
    const long it_off = take(L.off, (long)(itiles.size() * sizeof(GradTile) / 8));
    const long gt_off = take(L.off, (long)(gtiles.size() * sizeof(GradTile) / 8));
    const long gx_off = take(L.off, (long)(gx.size() * sizeof(GradXProb) / 8));
    const long xt_off = take(L.off, (long)(xtiles.size() * sizeof(GradTile) / 8));
    const long xr_off = take(L.off, (long)(xrows.size() * sizeof(GradTile) / 8));

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    std::memcpy(m.hin + gp_off, gp.data(), gp.size() * sizeof(GradProb));
    std::memcpy(m.hin + it_off, itiles.data(), itiles.size() * sizeof(GradTile));
    std::memcpy(m.hin + gt_off, gtiles.data(), gtiles.size() * sizeof(GradTile));
    if (nwx) {
        std::memcpy(m.hin + gx_off, gx.data(), gx.size() * sizeof(GradXProb));
        std::memcpy(m.hin + xt_off, xtiles.data(), xtiles.size() * sizeof(GradTile));
        std::memcpy(m.hin + xr_off, xrows.data(), xrows.size() * sizeof(GradTile));
    }
    RC(run_drained(c, [&]() -> int32_t {
        const GradProb* gps = reinterpret_cast<const GradProb*>(m.in + gp_off);
        const GradTile* its = reinterpret_cast<const GradTile*>(m.in + it_off);
        const GradTile* gts = reinterpret_cast<const GradTile*>(m.in + gt_off);
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        hipLaunchKernelGGL(batch_inv_kernel, dim3((unsigned)itiles.size()), dim3(NT), 0, c->sm, m.in, m.ws, (const double*)m.res, nw, gps, its);
        HIPCHK(hipGetLastError());
        RC(launch_grad(m, a.ks != nullptr, nw, gps, gts, gtiles.size()));
        hipLaunchKernelGGL(batch_gsum_kernel, dim3((unsigned)nw), dim3(128), 0, c->sm, m.in, (const double*)m.ws, m.res, nw, gps);
        HIPCHK(hipGetLastError());
        if (nwx) {
            const GradXProb* gxs = reinterpret_cast<const GradXProb*>(m.in + gx_off);
            RC(launch_gradx(m, a.ks != nullptr, nw, gps, gxs, reinterpret_cast<const GradTile*>(m.in + xt_off), xtiles.size()));
            hipLaunchKernelGGL(batch_gxsum_kernel, dim3((unsigned)xrows.size()), dim3(BT), 0, c->sm, m.in, (const double*)m.ws, m.res, nw, gxs,
                               reinterpret_cast<const GradTile*>(m.in + xr_off));
            HIPCHK(hipGetLastError());
        }
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    c->batch_grad_problems += nw;
    c->batch_gradx_problems += nwx;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const GradProb& g = gp[L.pos[t]];
        const long n = L.pr[t].n;
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        const double* G = hout + g.g_off;  // [0] noise, then the kernel's parameters
        if (a.dvar) a.dvar[b] = G[1];
        if (a.dscale && a.dscale[b]) std::memcpy(a.dscale[b], G + 2, sizeof(double) * (size_t)(g.ng - 2));
        if (a.dtheta) std::memcpy(a.dtheta[b], G + 1, sizeof(double) * (size_t)(g.ng - 1));
        if (double* dn = (double*)a.dnb(b)) {
            if (g.dn_off >= 0) std::memcpy(dn, hout + g.dn_off, sizeof(double) * (size_t)n);
            else dn[0] = G[0];
        }
        if (double* dy = (double*)a.dyb(b)) {
            const double* al = hout + L.pr[t].alpha_off;
            for (long j = 0; j < n; ++j) dy[j] = -al[j];
        }
        if (void* dx = a.dxb(b)) grad_to_layout<double>(a.xb(b).layout, n, a.xb(b).d, hout + gx[L.pos[t]].dx_off, n, dx);  // [d][n] -> the container layout of x
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
    // a gradient array that is given holds a pointer for every problem (dscale: wherever the problem has scales)
    const int a_dn = a.ks ? a.arg0 + 1 : a.arg0 + 2, a_dy = a_dn + 1;
    for (int b = 0; b < a.nb; ++b) {
        if (a.dscale && a.k[b].nscale > 0 && !a.dscale[b]) return set_arg_err(a.arg0 + 1, "a dscale_out pointer is NULL where the kernel has scales");
        if (a.dtheta && !a.dtheta[b]) return set_arg_err(a.arg0, "a dtheta_out pointer is NULL");
        if (a.dnoise && !a.dnoise[b]) return set_arg_err(a_dn, "a dnoise_out pointer is NULL");
        if (a.dy && !a.dy[b]) return set_arg_err(a_dy, "a dy_out pointer is NULL");
        if (a.dx && !a.dx[b]) return set_arg_err(a_dy + 1, "a dx_out pointer is NULL");
    }
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
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            grad_fill_nan(a, b, grad_nkp(a, packed, b));
        }
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
    std::vector<GradProb> gp((size_t)nw);
    std::vector<LooProb> lq((size_t)nw);
    std::vector<GradTile> itiles, gtiles, ztiles;
    for (int s = 0; s < nw; ++s) {
        const int t = L.order[s], b = idx[t];
        const BatchProb& p = L.pr[t];
        GradProb& g = gp[s];
        LooProb& q = lq[s];
        const int nt = p.np / BT;
        g = GradProb{-1, -1, -1, -1, 0, 0};
        q = LooProb{-1, -1, -1, -1, -1, -1, -1, -1};
        g.s_off = take(L.ws, (long)p.np * p.ld);
        q.lpart_off = take(L.ws, (loo_tiles(p.n) + 1) & ~1L);  // the next strip stays 16-byte aligned
        if (a.lpb(b)) q.lp_off = take(L.roff, p.n);
        if (a.meanb(b)) q.mean_off = take(L.roff, p.n);
        if (a.varb(b)) q.var_off = take(L.roff, p.n);
        for (int r0 = 0; r0 < p.np; r0 += TP) itiles.push_back(GradTile{s, r0 / TP, 0, 0});
        if (!a.grad) continue;
        g.ng = 1 + grad_nkp(a, packed, b);
        g.ntiles = nt * (nt + 1) / 2;
        q.z_off = take(L.ws, (long)p.np * p.ld);
        q.d_off = take(L.ws, p.np);
        q.e_off = take(L.ws, p.np);
        g.part_off = take(L.ws, ((long)g.ntiles * g.ng + 1) & ~1L);
        g.g_off = take(L.roff, g.ng);
        g.dn_off = a.noise[b].kind == 1 ? take(L.roff, p.n) : -1;
        q.beta_off = take(L.roff, p.np);
        for (int ti = 0; ti < nt; ++ti) {
            for (int tj = 0; tj <= ti; ++tj) gtiles.push_back(GradTile{s, ti, tj, ti * (ti + 1) / 2 + tj});
            for (int tj = 0; tj < nt; ++tj) ztiles.push_back(GradTile{s, ti, tj, ti * nt + tj});
        }
    }
    const long gp_off = take(L.off, (long)(gp.size() * sizeof(GradProb) / 8));
    const long lq_off = take(L.off, (long)(lq.size() * sizeof(LooProb) / 8));
    const long it_off = take(L.off, (long)(itiles.size() * sizeof(GradTile) / 8));
    const long gt_off = take(L.off, (long)(gtiles.size() * sizeof(GradTile) / 8));
    const long zt_off = take(L.off, (long)(ztiles.size() * sizeof(GradTile) / 8));

    WaveMem m(c);
    RC(m.alloc(L.off, L.ws, L.roff));
    wave_fill(a, packed, idx, nw, L, m.hin);
    std::memcpy(m.hin + gp_off, gp.data(), gp.size() * sizeof(GradProb));
    std::memcpy(m.hin + lq_off, lq.data(), lq.size() * sizeof(LooProb));
    std::memcpy(m.hin + it_off, itiles.data(), itiles.size() * sizeof(GradTile));
    if (a.grad) {
        std::memcpy(m.hin + gt_off, gtiles.data(), gtiles.size() * sizeof(GradTile));
        std::memcpy(m.hin + zt_off, ztiles.data(), ztiles.size() * sizeof(GradTile));
    }
    RC(run_drained(c, [&]() -> int32_t {
        const GradProb* gps = reinterpret_cast<const GradProb*>(m.in + gp_off);
        const LooProb* lps = reinterpret_cast<const LooProb*>(m.in + lq_off);
        const GradTile* its = reinterpret_cast<const GradTile*>(m.in + it_off);
        const unsigned nit = (unsigned)itiles.size();
        RC(m.upload());
        RC(launch_fit(m, a.ks != nullptr, nw));
        hipLaunchKernelGGL(batch_inv_kernel, dim3(nit), dim3(NT), 0, c->sm, m.in, m.ws, (const double*)m.res, nw, gps, its);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(batch_loo_kernel, dim3(nit), dim3(NT), 0, c->sm, m.in, m.ws, m.res, nw, gps, lps, its);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(batch_loo_sum_kernel, dim3((unsigned)nw), dim3(128), 0, c->sm, m.in, (const double*)m.ws, m.res, nw, lps);
        HIPCHK(hipGetLastError());
        if (a.grad) {
            hipLaunchKernelGGL(batch_loo_z_kernel, dim3((unsigned)ztiles.size()), dim3(GNT), 0, c->sm, m.in, m.ws, (const double*)m.res, nw, gps, lps,
                               reinterpret_cast<const GradTile*>(m.in + zt_off));
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(batch_loo_beta_kernel, dim3(nit), dim3(NT), 0, c->sm, m.in, (const double*)m.ws, m.res, nw, lps, its);
            HIPCHK(hipGetLastError());
            RC(launch_grad(m, a.ks != nullptr, nw, gps, reinterpret_cast<const GradTile*>(m.in + gt_off), gtiles.size(), lps));
            hipLaunchKernelGGL(batch_gsum_kernel, dim3((unsigned)nw), dim3(128), 0, c->sm, m.in, (const double*)m.ws, m.res, nw, gps);
            HIPCHK(hipGetLastError());
        }
        return m.download_and_sync();
    }));
    const double* hout = m.hout;
    (a.grad ? c->batch_loo_grad_problems : c->batch_loo_problems) += nw;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const GradProb& g = gp[L.pos[t]];
        const LooProb& q = lq[L.pos[t]];
        const size_t bytes = sizeof(double) * (size_t)L.pr[t].n;
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        if (q.lp_off >= 0) std::memcpy(a.lpb(b), hout + q.lp_off, bytes);
        if (q.mean_off >= 0) std::memcpy(a.meanb(b), hout + q.mean_off, bytes);
        if (q.var_off >= 0) std::memcpy(a.varb(b), hout + q.var_off, bytes);
        if (!a.grad) continue;
        const double* G = hout + g.g_off;  // [0] noise, then the kernel's parameters
        if (a.dvar) a.dvar[b] = G[1];
        if (a.dscale && a.dscale[b]) std::memcpy(a.dscale[b], G + 2, sizeof(double) * (size_t)(g.ng - 2));
        if (a.dtheta) std::memcpy(a.dtheta[b], G + 1, sizeof(double) * (size_t)(g.ng - 1));
        if (double* dn = (double*)a.dnb(b)) {
            if (g.dn_off >= 0) std::memcpy(dn, hout + g.dn_off, bytes);
            else dn[0] = G[0];
        }
        if (double* dy = (double*)a.dyb(b)) {
            const double* be = hout + q.beta_off;
            for (long j = 0; j < L.pr[t].n; ++j) dy[j] = -be[j];
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
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            loo_fill_nan(a, b, 0);
        }
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
    const int a_dn = a.ks ? a.arg0 + 1 : a.arg0 + 2, a_dy = a_dn + 1;
    for (int b = 0; b < a.nb; ++b) {  // a gradient array that is given holds a pointer for every problem (dscale: wherever the problem has scales)
        if (a.dscale && a.k[b].nscale > 0 && !a.dscale[b]) return set_arg_err(a.arg0 + 1, "a dscale_out pointer is NULL where the kernel has scales");
        if (a.dtheta && !a.dtheta[b]) return set_arg_err(a.arg0, "a dtheta_out pointer is NULL");
        if (a.dnoise && !a.dnoise[b]) return set_arg_err(a_dn, "a dnoise_out pointer is NULL");
        if (a.dy && !a.dy[b]) return set_arg_err(a_dy, "a dy_out pointer is NULL");
        if (a.dx && !a.dx[b]) return set_arg_err(a_dy + 1, "a dx_out pointer is NULL");
    }
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
        if (rc < 0) return rc;
        a.info_out[b] = rc;
        if (rc > 0) {
            put_result(a, b, std::numeric_limits<double>::quiet_NaN(), rc);
            loo_fill_nan(a, b, grad_nkp(a, packed, b));
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int32_t gp_logpdf_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                        const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                        void* const* alpha_out_or_null) {
    BatchArgs a{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, alpha_out_or_null, 0};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return batch_impl(ctx, a);
}

int32_t gp_logpdf_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                            const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                            void* const* alpha_out_or_null) {
    BatchArgs a{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, alpha_out_or_null, 0};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return batch_impl(ctx, a);
}

int32_t gp_predict_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                         const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                         void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what, mean_out, var_out};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_batch_impl(ctx, a);
}

int32_t gp_predict_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                             const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out, void* const* var_out,
                             void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what, mean_out, var_out};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_batch_impl(ctx, a);
}

int32_t gp_predict_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                              const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                              void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what,
                  mean_out_or_null, var_out_or_null, true, dmean_out_or_null, dvar_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_grad_batch_impl(ctx, a);
}

int32_t gp_predict_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                  const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                                  const void* const* prior_mean_xs_or_null, int32_t what, void* const* mean_out_or_null, void* const* var_out_or_null,
                                  void* const* dmean_out_or_null, void* const* dvar_out_or_null, void* logpdf_out_or_null, int32_t* info_out) {
    PredictArgs a{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what,
                  mean_out_or_null, var_out_or_null, true, dmean_out_or_null, dvar_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return predict_grad_batch_impl(ctx, a);
}

int32_t gp_joint_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                       const void* const* mean_or_null, int32_t ny, const void* const* y, int32_t nxs, const gp_points* xs,
                       const void* const* prior_mean_xs_or_null, const gp_noise* noise_xs_or_null, int32_t what, void* const* mean_out_or_null,
                       void* const* cov_out_or_null, const void* const* ys_or_null, void* hlogpdf_out_or_null, int32_t nsamp, const void* const* xi_or_null,
                       void* const* samples_out_or_null, void* logpdf_out_or_null, int32_t* info_out, int32_t* info_joint_out_or_null) {
    JointArgs a{{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what,
                 mean_out_or_null, nullptr},
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
    JointArgs a{{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out_or_null, info_out, nullptr, 0}, nxs, xs, prior_mean_xs_or_null, what,
                 mean_out_or_null, nullptr},
                noise_xs_or_null, cov_out_or_null, ys_or_null, hlogpdf_out_or_null, nsamp, xi_or_null, samples_out_or_null, info_joint_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return joint_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                             const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                             double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                             void* const* dy_out_or_null) {
    GradArgs a{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, nullptr, 0}, dvariance_out_or_null, dscale_out_or_null, nullptr, dnoise_out_or_null, dy_out_or_null, 12};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return grad_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                 const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                 double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null) {
    GradArgs a{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, nullptr, 0}, nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null, dy_out_or_null, 12};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return grad_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_x(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                               const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                               double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                               void* const* dy_out_or_null, void* const* dx_out_or_null) {
    GradArgs a{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, nullptr, 0}, dvariance_out_or_null, dscale_out_or_null, nullptr, dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return gradx_batch_impl(ctx, a);
}

int32_t gp_logpdf_grad_batch_sum_x(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                                   const void* const* mean_or_null, int32_t ny, const void* const* y, void* logpdf_out, int32_t* info_out,
                                   double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                                   void* const* dx_out_or_null) {
    GradArgs a{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, logpdf_out, info_out, nullptr, 0}, nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return gradx_batch_impl(ctx, a);
}

int32_t gp_loo_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                     const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                     void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null) {
    LooArgs a{{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, value_out, info_out, nullptr, 0}, nullptr, nullptr, nullptr, nullptr, nullptr, 12}, false,
              lp_out_or_null, mean_out_or_null, var_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_batch_impl(ctx, a);
}

int32_t gp_loo_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                         const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                         void* const* lp_out_or_null, void* const* mean_out_or_null, void* const* var_out_or_null) {
    LooArgs a{{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out, nullptr, 0}, nullptr, nullptr, nullptr, nullptr, nullptr, 12}, false,
              lp_out_or_null, mean_out_or_null, var_out_or_null};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_batch_impl(ctx, a);
}

int32_t gp_loo_grad_batch(gp_ctx* ctx, int32_t nb, const gp_kernel* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                          const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                          double* dvariance_out_or_null, double* const* dscale_out_or_null, void* const* dnoise_out_or_null,
                          void* const* dy_out_or_null, void* const* dx_out_or_null) {
    LooArgs a{{{nb, k, nullptr, nx, x, noise, mean_or_null, ny, y, value_out, info_out, nullptr, 0}, dvariance_out_or_null, dscale_out_or_null, nullptr,
               dnoise_out_or_null, dy_out_or_null, 12, dx_out_or_null}, true};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_grad_batch_impl(ctx, a);
}

int32_t gp_loo_grad_batch_sum(gp_ctx* ctx, int32_t nb, const gp_ksum* k, int32_t nx, const gp_points* x, const gp_noise* noise,
                              const void* const* mean_or_null, int32_t ny, const void* const* y, void* value_out, int32_t* info_out,
                              double* const* dtheta_out_or_null, void* const* dnoise_out_or_null, void* const* dy_out_or_null,
                              void* const* dx_out_or_null) {
    LooArgs a{{{nb, nullptr, k, nx, x, noise, mean_or_null, ny, y, value_out, info_out, nullptr, 0}, nullptr, nullptr, dtheta_out_or_null, dnoise_out_or_null,
               dy_out_or_null, 12, dx_out_or_null}, true};
    if (nb > 0 && !k) return set_arg_err(3, "kernel array is NULL");
    return loo_grad_batch_impl(ctx, a);
}
}
