// batch.hip — many small exact GPs in one call: gp_logpdf_batch / gp_logpdf_batch_sum, gp_predict_batch / gp_predict_batch_sum (include/gpmi355.h) and the
// two kernels behind them: the fit (batch_logpdf_kernel, below) and the predictions at each problem's test points from the slices it leaves
// (batch_predict_kernel, further down).
//
// ONE workgroup owns ONE problem from its inputs to its scalar: it assembles the lower triangle of K + Σy into the problem's slice of a
// workspace (δ = y − m riding along as row np, as in the single path), factors it by a blocked right-looking Cholesky (64-column blocks:
// diagonal block in LDS, rows below by substitution in registers, trailing update by v_mfma_f64_16x16x4_f64 on 32×32 wave tiles with
// register-resident operands), reads ‖L⁻¹δ‖² off the carried row and, when α is wanted, runs the backward sweep on the same slice.
// Workgroups never wait for one another (no flags, no tickets: blockIdx.x is the problem), every loop is bounded by the problem's size, no
// floating-point atomics are used and the schedule of a problem depends on that problem alone — its result is the same bits whatever
// batch it rides in.  The slice of a problem (its factor and the solved row) stays intact until the call ends.
//
// Problems the kernel does not take (fp32, a dense Σy, n > GPMI355_BATCH_MAX_N, D > 16) are answered inside the same call by the
// single path (gp_logpdf / gp_posterior_fit and their *_sum forms; for predictions gp_posterior_fit + gp_posterior_predict + gp_posterior_free); which
// path serves a problem depends on that problem alone.
#include "kfun.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
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
#pragma unroll
            for (int p = 0; p < BATCH_MAXD; ++p) xj[p] = (p < d && j < n) ? x[(long)p * n + j] : 0.0;
            for (int rr = 0; rr < BT / 8; ++rr) {
                const int i = ti * BT + w + 8 * rr;  // wave-uniform
                double v;
                if (i >= n || j >= n) {
                    v = (i == j) ? 1.0 : 0.0;
                } else {
                    double t[BATCH_MAXD];
#pragma unroll
                    for (int p = 0; p < BATCH_MAXD; ++p) t[p] = p < d ? x[(long)p * n + i] - xj[p] : 0.0;
                    if (SUM) {
                        v = ksum_eval<double, BATCH_MAXD>(*reinterpret_cast<const KSum*>(in + P.ks_off), t, d);
                    } else {
                        double d2 = 0.0;
#pragma unroll
                        for (int p = 0; p < BATCH_MAXD; ++p) {
                            const double u = (P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p]) * t[p];
                            d2 = fma(u, u, d2);
                        }
                        v = P.variance * kappa<double>(P.kind, d2);
                    }
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
        for (int rr = tid; rr < np + 1 - r_lo; rr += NT) {
            d2_t* row = reinterpret_cast<d2_t*>(A + (long)(r_lo + rr) * ld + j0);
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
            }
        }
        __syncthreads();

        // trailing update C −= P Pᵀ on 32×32 wave tiles.  Lane l = (r = l & 15, g = l >> 4) holds 16 consecutive k of rows r and 16 + r of
        // both operands; MFMA step s multiplies the k-quadruple {16 g + s}: the sum over k is complete after 16 steps, in a fixed order.
        const int ntr = (np + 32 - r_lo) / 32, ntc = (np - r_lo) / 32;
        const int r = lane & 15, g = lane >> 4;
        int cnt = 0;
        for (int ti = 0; ti < ntr; ++ti)
            for (int tj = 0; tj <= ti && tj < ntc; ++tj) {
                if ((cnt++ & 7) != w) continue;
                const int i0 = r_lo + 32 * ti, c0 = r_lo + 32 * tj;
                double a[2][16], b[2][16];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d2_t* pa = reinterpret_cast<const d2_t*>(A + (long)(i0 + 16 * h + r) * ld + j0 + 16 * g);
                    const d2_t* pb = reinterpret_cast<const d2_t*>(A + (long)(c0 + 16 * h + r) * ld + j0 + 16 * g);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const d2_t ta = pa[q], tb = pb[q];
                        a[h][2 * q] = -ta.x;
                        a[h][2 * q + 1] = -ta.y;
                        b[h][2 * q] = tb.x;
                        b[h][2 * q + 1] = tb.y;
                    }
                }
                d4_t acc[2][2];
#pragma unroll
                for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                    for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[hi][hj][q] = A[(long)(i0 + 16 * hi + Tr<double>::crow(lane, q)) * ld + c0 + 16 * hj + r];
#pragma unroll
                for (int s = 0; s < 16; ++s)
#pragma unroll
                    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                        for (int hj = 0; hj < 2; ++hj) acc[hi][hj] = Tr<double>::mfma(a[hi][s], b[hj][s], acc[hi][hj]);
#pragma unroll
                for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                    for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            A[(long)(i0 + 16 * hi + Tr<double>::crow(lane, q)) * ld + c0 + 16 * hj + r] = acc[hi][hj][q];
            }
        __syncthreads();
    }

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
//   2. V ← V L⁻ᵀ left-looking by 64-column blocks: V[:, j0:j0+64] −= V[:, 0:j0] L[j0:j0+64, 0:j0]ᵀ by v_mfma_f64_16x16x4_f64 on 32×32 wave tiles (the operand
//      form of the fit kernel's trailing update, the k loop running over [0, j0) inside the accumulators), then the diagonal block by substitution: L_bb in
//      LDS, one test point per thread in registers;
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
#pragma unroll
        for (int p = 0; p < BATCH_MAXD; ++p) xj[p] = (p < d && j < n) ? x[(long)p * n + j] : 0.0;
        const double aj = (alpha && j < n) ? alpha[j] : 0.0;
        for (int rr = 0; rr < rp / 8; ++rr) {
            const int i = w + 8 * rr;  // wave-uniform
            double v = 0.0;
            if (i < rows && j < n) {
                double t[BATCH_MAXD];
#pragma unroll
                for (int p = 0; p < BATCH_MAXD; ++p) t[p] = p < d ? xs[(long)p * ns + i] - xj[p] : 0.0;
                if (SUM) {
                    v = ksum_eval<double, BATCH_MAXD>(*reinterpret_cast<const KSum*>(in + P.ks_off), t, d);
                } else {
                    double d2 = 0.0;
#pragma unroll
                    for (int p = 0; p < BATCH_MAXD; ++p) {
                        const double u = (P.nscale == 0 ? 1.0 : P.scale[P.nscale == 1 ? 0 : p]) * t[p];
                        d2 = fma(u, u, d2);
                    }
                    v = P.variance * kappa<double>(P.kind, d2);
                }
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

    // ---- 2. V ← V L⁻ᵀ, left-looking; 3. Σ_i V_ji² by the thread that owns row j
    double (*Ls)[BTS] = reinterpret_cast<double (*)[BTS]>(sh);
    double* dinv = sh + BT * BTS;
    const int r = lane & 15, g = lane >> 4;
    double ss = 0.0;
    for (int kb = 0; kb < nt; ++kb) {
        const int j0 = kb * BT;
        // Lane l = (r = l & 15, g = l >> 4) holds 16 consecutive k of rows r and 16 + r of both operands; MFMA step s multiplies the k-quadruple {16 g + s}.
        for (int tile = w; tile < (rp / 32) * 2 && kb > 0; tile += 8) {
            const int i0 = 32 * (tile >> 1), c0 = j0 + 32 * (tile & 1);
            d4_t acc[2][2];
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[hi][hj][q] = V[(long)(i0 + 16 * hi + Tr<double>::crow(lane, q)) * ld + c0 + 16 * hj + r];
            for (int k0 = 0; k0 < j0; k0 += BT) {
                double a[2][16], b[2][16];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d2_t* pa = reinterpret_cast<const d2_t*>(V + (long)(i0 + 16 * h + r) * ld + k0 + 16 * g);
                    const d2_t* pb = reinterpret_cast<const d2_t*>(A + (long)(c0 + 16 * h + r) * ld + k0 + 16 * g);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const d2_t ta = pa[q], tb = pb[q];
                        a[h][2 * q] = -ta.x;
                        a[h][2 * q + 1] = -ta.y;
                        b[h][2 * q] = tb.x;
                        b[h][2 * q + 1] = tb.y;
                    }
                }
#pragma unroll
                for (int s = 0; s < 16; ++s)
#pragma unroll
                    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                        for (int hj = 0; hj < 2; ++hj) acc[hi][hj] = Tr<double>::mfma(a[hi][s], b[hj][s], acc[hi][hj]);
            }
#pragma unroll
            for (int hi = 0; hi < 2; ++hi)
#pragma unroll
                for (int hj = 0; hj < 2; ++hj)
#pragma unroll
                    for (int q = 0; q < 4; ++q) V[(long)(i0 + 16 * hi + Tr<double>::crow(lane, q)) * ld + c0 + 16 * hj + r] = acc[hi][hj][q];
        }
        // the diagonal block: its lower triangle in LDS (the rest of the tile is not the factor's)
        for (int e = tid; e < BT * BT; e += NT) {
            const int rr = e >> 6, cc = e & 63;
            Ls[rr][cc] = cc <= rr ? A[(long)(j0 + rr) * ld + j0 + cc] : 0.0;
        }
        __syncthreads();
        if (tid < BT) dinv[tid] = 1.0 / Ls[tid][tid];
        __syncthreads();
        if (tid < rows) {  // X ← X L_bb⁻ᵀ, one test point per thread in registers
            d2_t* row = reinterpret_cast<d2_t*>(V + (long)tid * ld + j0);
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
                    if ((k2 & 15) == 15) __builtin_amdgcn_sched_barrier(0);  // as in the fit kernel: hoisted LDS reads spill
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
        __syncthreads();
    }
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

long batch_max_n() {  // GPMI355_BATCH_MAX_N; the environment variable GPMI_BATCH_MAX_N (0 … what the kernel admits) overrides it for measurements
    long v = GPMI355_BATCH_MAX_N;
    if (const char* e = getenv("GPMI_BATCH_MAX_N")) v = atol(e);
    return std::max(0L, std::min<long>(v, BATCH_KERNEL_MAX_N));
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

// The packed input of one wave (doubles): descriptors | composite kernels | x | y | means | noise vectors, then whatever the caller appends at `off`;
// `ws` counts the slices, `roff` the result buffer (logpdf and failure column of every problem, then the α vectors).
struct WaveLayout {
    std::vector<BatchProb> pr;  // in the order of idx
    std::vector<int> order;     // the descriptors as they lie on the device: the widest problems first (the last workgroups to start are the shortest)
    long off = 0, ws = 0, roff = 0;
};

// descriptors and offsets of the problems idx[0..nw); want_alpha(b): α of problem b goes to the result buffer
template <class F> void wave_layout(const BatchArgs& a, const int* idx, int nw, F&& want_alpha, WaveLayout& L) {
    std::vector<BatchProb>& pr = L.pr;
    pr.assign((size_t)nw, BatchProb{});
    long off = (long)((size_t)nw * sizeof(BatchProb) / 8), ws = 0, roff = 2L * nw;
    const long ksd = (long)((sizeof(KSum) + 7) / 8);
    long x_shared = -1, y_shared = -1;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& x = a.xb(b);
        BatchProb& p = pr[t];
        p.n = (int)x.n;
        p.np = (int)batch_np(x.n);
        p.ld = (int)batch_ld(p.np);
        p.d = x.d;
        p.slot = t;
        p.a_off = ws;
        ws += batch_slice(x.n);
        p.ks_off = -1;
        if (a.ks) {
            p.ks_off = off;
            off += ksd;
        } else {
            const gp_kernel& k = a.k[b];
            p.kind = k.kind;
            p.nscale = k.nscale;
            p.variance = k.variance;
            for (int q = 0; q < k.nscale; ++q) p.scale[q] = k.scale[q];
        }
        if (a.nx == 1 && x_shared >= 0) {
            p.x_off = x_shared;
        } else {
            p.x_off = x_shared = off;
            off += (long)x.d * x.n;
        }
        if (a.ny == 1 && y_shared >= 0) {
            p.y_off = y_shared;
        } else {
            p.y_off = y_shared = off;
            off += x.n;
        }
        p.m_off = -1;
        if (a.mb(b)) {
            p.m_off = off;
            off += x.n;
        }
        p.nz_off = -1;
        p.noise_s = a.noise[b].s;
        if (a.noise[b].kind == 1) {
            p.nz_off = off;
            off += x.n;
        }
        p.alpha_off = -1;
        if (want_alpha(b)) {
            p.alpha_off = roff;
            roff += x.n;
        }
    }
    L.order.resize((size_t)nw);
    for (int t = 0; t < nw; ++t) L.order[t] = t;
    std::stable_sort(L.order.begin(), L.order.end(), [&](int u, int v) { return pr[u].n > pr[v].n; });
    L.off = off;
    L.ws = ws;
    L.roff = roff;
}

// fills the packed input of a laid-out wave: the descriptors in L.order, then every problem's data
void wave_fill(const BatchArgs& a, const std::vector<KSum>& packed, const int* idx, int nw, const WaveLayout& L, double* hin) {
    for (int t = 0; t < nw; ++t) std::memcpy((char*)hin + (size_t)t * sizeof(BatchProb), &L.pr[L.order[t]], sizeof(BatchProb));
    bool x_done = false, y_done = false;
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        const gp_points& x = a.xb(b);
        const BatchProb& p = L.pr[t];
        if (a.ks) std::memcpy(hin + p.ks_off, &packed[b], sizeof(KSum));
        if (!(a.nx == 1 && x_done)) pack_points(x, hin + p.x_off);
        if (!(a.ny == 1 && y_done)) std::memcpy(hin + p.y_off, a.yb(b), sizeof(double) * x.n);
        x_done = y_done = true;
        if (p.m_off >= 0) std::memcpy(hin + p.m_off, a.mb(b), sizeof(double) * x.n);
        if (p.nz_off >= 0) std::memcpy(hin + p.nz_off, a.noise[b].diag, sizeof(double) * x.n);
    }
}

// page-locked staging of one wave for both directions (pageable above the staging limit)
double* wave_staging(gp_ctx* c, size_t doubles, std::vector<double>& pageable) {
    double* h = (double*)ctx_pinned(c, sizeof(double) * doubles);
    if (!h) {
        pageable.resize(doubles);
        h = pageable.data();
    }
    return h;
}

// one launch: the problems idx[0..nw) of the call, all taken by the kernel.  Caller holds the ctx lock.
int32_t run_wave(gp_ctx* c, const BatchArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [&](int b) { return a.ab(b) != nullptr; }, L);
    const std::vector<BatchProb>& pr = L.pr;
    const long off = L.off, ws = L.ws, roff = L.roff;
    const size_t in_bytes = sizeof(double) * (size_t)off, out_bytes = sizeof(double) * (size_t)roff;
    std::vector<double> pageable;
    double* hin = wave_staging(c, (size_t)(off + roff), pageable);
    double* hout = hin + off;
    wave_fill(a, packed, idx, nw, L, hin);
    DevBufs bufs(c);
    void *in_d = nullptr, *ws_d = nullptr, *res_d = nullptr;
    RC(bufs.get(in_bytes, &in_d));
    RC(bufs.get(sizeof(double) * (size_t)ws, &ws_d));
    RC(bufs.get(out_bytes, &res_d));
    RC(run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemcpyAsync(in_d, hin, in_bytes, hipMemcpyHostToDevice, c->sm));
        if (a.ks) hipLaunchKernelGGL(batch_logpdf_kernel<true>, dim3((unsigned)nw), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw);
        else hipLaunchKernelGGL(batch_logpdf_kernel<false>, dim3((unsigned)nw), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hout, res_d, out_bytes, hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        return 0;
    }));
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        if (pr[t].alpha_off >= 0) std::memcpy(a.ab(b), hout + pr[t].alpha_off, sizeof(double) * pr[t].n);
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
    // the path of a problem depends on that problem alone
    const long max_n = batch_max_n();
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) {
        (batch_takes(a, b, max_n) ? mine : routed).push_back(b);
    }
    if (!mine.empty()) {
        HIPCHK(hipSetDevice(c->device));
        size_t i = 0;
        while (i < mine.size()) {  // waves bounded by the workspace budget and by the launch size
            size_t j = i, bytes = 0;
            while (j < mine.size() && j - i < BATCH_WAVE_PROBLEMS) {
                const size_t s = sizeof(double) * (size_t)batch_slice(a.xb(mine[j]).n);
                if (j > i && bytes + s > BATCH_WS_BYTES) break;
                bytes += s;
                ++j;
            }
            RC(run_wave(c, a, packed, mine.data() + i, (int)(j - i)));
            i = j;
        }
    }
    // everything else: the single path, one problem at a time.  Each of those calls takes the ctx lock itself (std::mutex is not recursive): it is released
    // here; the ctx stays pinned by the Guard, and every call validates it again.
    gd.lk.unlock();
    const size_t es = a.dtype == 0 ? 8 : 4;
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        int32_t rc;
        put(a.logpdf_out, a.dtype, b, 0);
        void* lp = (char*)a.logpdf_out + es * (size_t)b;
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
            if (a.ab(b)) {
                if (a.dtype == 0) std::fill_n((double*)a.ab(b), x.n, std::numeric_limits<double>::quiet_NaN());
                else std::fill_n((float*)a.ab(b), x.n, std::numeric_limits<float>::quiet_NaN());
            }
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
    const gp_points& xsb(int b) const { return xs[nxs == 1 ? 0 : b]; }
    const void* pmb(int b) const { return pm ? pm[b] : nullptr; }
};

long predict_strip(const PredictArgs& a, long n) { return (a.what & 2) ? (long)TP * batch_ld(batch_np(n)) : 0; }  // the mean alone needs no strip

void fill_nan(void* out, int dtype, long n) {
    if (!out) return;
    if (dtype == 0) std::fill_n((double*)out, n, std::numeric_limits<double>::quiet_NaN());
    else std::fill_n((float*)out, n, std::numeric_limits<float>::quiet_NaN());
}

// one wave: the fit launch of the problems idx[0..nw), then the predict launches against the slices it leaves.  Caller holds the ctx lock.
int32_t run_predict_wave(gp_ctx* c, const PredictArgs& a, const std::vector<KSum>& packed, const int* idx, int nw) {
    WaveLayout L;
    wave_layout(a, idx, nw, [&](int b) { return (a.what & 1) && a.xsb(b).n > 0; }, L);
    // behind the fit's input: the test points (dimension-major, a shared set once), then the tile table; behind its results: mean and var of every problem
    std::vector<long> xs_off((size_t)nw, -1), mean_off((size_t)nw, -1), var_off((size_t)nw, -1);
    long xs_shared = -1;
    for (int t = 0; t < nw; ++t) {
        const gp_points& xs = a.xsb(idx[t]);
        if (xs.n == 0) continue;
        if (a.nxs == 1 && xs_shared >= 0) {
            xs_off[t] = xs_shared;
        } else {
            xs_off[t] = xs_shared = L.off;
            L.off += (long)xs.d * xs.n;
        }
        if (a.what & 1) {
            mean_off[t] = L.roff;
            L.roff += xs.n;
        }
        if (a.what & 2) {
            var_off[t] = L.roff;
            L.roff += xs.n;
        }
    }
    // tiles of TP test points, the widest problems first; a launch closes at BATCH_PRED_TILES tiles or when its strips would pass the workspace budget
    std::vector<int> pos((size_t)nw);
    for (int s = 0; s < nw; ++s) pos[L.order[s]] = s;
    std::vector<BatchTile> tiles;
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
            BatchTile tl{xs_off[t], cur, mean_off[t], var_off[t], pos[t], (int)ns, (int)row0, (int)std::min<long>(TP, ns - row0)};
            tiles.push_back(tl);
            cur += strip;
            ws_top = std::max(ws_top, cur);
        }
    }
    if (tiles.size() > launch_begin) launch_end.push_back(tiles.size());
    const long tile_off = L.off;
    L.off += (long)(tiles.size() * sizeof(BatchTile) / 8);

    const size_t in_bytes = sizeof(double) * (size_t)L.off, out_bytes = sizeof(double) * (size_t)L.roff;
    std::vector<double> pageable;
    double* hin = wave_staging(c, (size_t)(L.off + L.roff), pageable);
    double* hout = hin + L.off;
    wave_fill(a, packed, idx, nw, L, hin);
    bool xs_done = false;
    for (int t = 0; t < nw; ++t) {
        const gp_points& xs = a.xsb(idx[t]);
        if (xs.n == 0 || (a.nxs == 1 && xs_done)) continue;
        pack_points(xs, hin + xs_off[t]);
        xs_done = true;
    }
    if (!tiles.empty()) std::memcpy(hin + tile_off, tiles.data(), tiles.size() * sizeof(BatchTile));
    DevBufs bufs(c);
    void *in_d = nullptr, *ws_d = nullptr, *res_d = nullptr;
    RC(bufs.get(in_bytes, &in_d));
    RC(bufs.get(sizeof(double) * (size_t)ws_top, &ws_d));
    RC(bufs.get(out_bytes, &res_d));
    RC(run_drained(c, [&]() -> int32_t {
        HIPCHK(hipMemcpyAsync(in_d, hin, in_bytes, hipMemcpyHostToDevice, c->sm));
        if (a.ks) hipLaunchKernelGGL(batch_logpdf_kernel<true>, dim3((unsigned)nw), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw);
        else hipLaunchKernelGGL(batch_logpdf_kernel<false>, dim3((unsigned)nw), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw);
        HIPCHK(hipGetLastError());
        size_t t0 = 0;
        for (size_t t1 : launch_end) {
            const BatchTile* tl = reinterpret_cast<const BatchTile*>((const double*)in_d + tile_off) + t0;
            if (a.ks) hipLaunchKernelGGL(batch_predict_kernel<true>, dim3((unsigned)(t1 - t0)), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw, tl);
            else hipLaunchKernelGGL(batch_predict_kernel<false>, dim3((unsigned)(t1 - t0)), dim3(NT), 0, c->sm, (const double*)in_d, (double*)ws_d, (double*)res_d, nw, tl);
            HIPCHK(hipGetLastError());
            t0 = t1;
        }
        HIPCHK(hipMemcpyAsync(hout, res_d, out_bytes, hipMemcpyDeviceToHost, c->sm));
        HIPCHK(hipStreamSynchronize(c->sm));
        return 0;
    }));
    for (int t = 0; t < nw; ++t) {
        const int b = idx[t];
        put_result(a, b, hout[t], (int32_t)hout[nw + t]);
        const long ns = a.xsb(b).n;
        if (ns == 0) continue;
        if (a.what & 1) {
            double* mo = (double*)a.mean_out[b];
            const double* pm = (const double*)a.pmb(b);
            for (long j = 0; j < ns; ++j) mo[j] = pm ? pm[j] + hout[mean_off[t] + j] : hout[mean_off[t] + j];
        }
        if (a.what & 2) std::memcpy(a.var_out[b], hout + var_off[t], sizeof(double) * (size_t)ns);
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
    const long max_n = batch_max_n();
    std::vector<int> mine, routed;
    for (int b = 0; b < a.nb; ++b) (batch_takes(a, b, max_n) ? mine : routed).push_back(b);
    if (!mine.empty()) {
        HIPCHK(hipSetDevice(c->device));
        size_t i = 0;
        while (i < mine.size()) {  // waves bounded by the launch size and by the workspace budget: the slices and the widest strip of the wave fit in it
            size_t j = i, bytes = 0, strip = 0;
            while (j < mine.size() && j - i < BATCH_WAVE_PROBLEMS) {
                const long n = a.xb(mine[j]).n;
                const size_t s = sizeof(double) * (size_t)batch_slice(n);
                const size_t st = std::max(strip, a.xsb(mine[j]).n > 0 ? sizeof(double) * (size_t)predict_strip(a, n) : 0);
                if (j > i && bytes + s + st > BATCH_WS_BYTES) break;
                bytes += s;
                strip = st;
                ++j;
            }
            RC(run_predict_wave(c, a, packed, mine.data() + i, (int)(j - i)));
            i = j;
        }
    }
    // everything else: fit, predict and free on the single path, one problem at a time, after the lock is released (as batch_impl does)
    gd.lk.unlock();
    const size_t es = a.dtype == 0 ? 8 : 4;
    for (int b : routed) {
        const gp_points& x = a.xb(b);
        const gp_points& xs = a.xsb(b);
        gp_post* post = nullptr;
        void* lp = a.logpdf_out ? (char*)a.logpdf_out + es * (size_t)b : nullptr;
        if (lp) put(a.logpdf_out, a.dtype, b, 0);
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
}
