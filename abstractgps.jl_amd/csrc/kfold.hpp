// K-fold cross-validation of an exact GP from one factorisation (gp_kfold / gp_kfold_sum, include/gpmi355.h).  With P = C⁻¹ = W Wᵀ for W = L⁻ᵀ
// (upper, row-major), α = P(y − m) and a fold F (sorted index set):
//   y_F | y_−F ~ N(y_F − P_FF⁻¹ α_F, P_FF⁻¹),   log p(y_F | y_−F) = −½ α_Fᵀ P_FF⁻¹ α_F + ½ logdet P_FF − ½|F| log 2π,
//   [P_FF]_ij = Σ_{k ≥ max(i,j)} W_ik W_jk.
// Two kernels, fp64 arithmetic whatever T: kfold_gram_kernel forms every fold's P_FF from gathered rows of W on the MFMA, kfold_fact_kernel factors one
// fold per workgroup and writes that fold's terms.  No atomics: every sum's order is fixed by n and the fold's index set alone, so a fold's results do
// not depend on its label or on the other folds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kcommon.hpp"

namespace gpmi {

// One fold: its sorted indices are idx[off .. off + cnt); its workspace is npad + 64 rows of ldp doubles at P + poff — the npad×npad block (npad = cnt
// rounded up to 64; lower 64×64 tiles only) and a 64-row scratch panel behind it that the in-place inversion stages through.
struct KfFold {
    int64_t poff;
    int32_t off, cnt, npad, ldp;
};
// One lower 64×64 tile (I >= J) of one fold's block: the work of one kfold_gram_kernel workgroup.
struct KfTile {
    int32_t fold, I, J, pad_;
};

constexpr int KF_KC = 32;          // k chunk of the gram kernel
constexpr int KF_LS = KF_KC + 2;   // its LDS row stride: 16 rows × 2 k of a half-wave's operand read fall on 32 distinct 8-byte banks
constexpr int KF_DS = 65;          // row stride of the 64×64 LDS tiles of the factor kernel
constexpr int KF_NT = 1024;        // threads of the factor kernel (16 waves)

// P_FF = W_F W_Fᵀ, one workgroup per table entry (fold, I, J).  Four waves, each a 32×32 sub-tile in 2×2 v_mfma_f64_16x16x4_f64 accumulators.  The k
// loop starts at the first row index of tile I rounded down to the chunk (the indices are sorted: no row of either operand has anything valid before it)
// and ends at np.  A chunk is 64 + 64 gathered row segments of KF_KC elements, read coalesced along k, widened to fp64 and SELECTED to zero where
// k < the row's own index (W's strictly-lower part is never read) or the row lies past the fold's end; the next chunk's loads are in registers before
// the current one's MFMAs.  Rows past |F| come out as zero, with 1 on the diagonal.  The whole tile is written (a diagonal tile in full).
template <typename T>
__global__ __launch_bounds__(256, 2) void kfold_gram_kernel(const T* __restrict__ W, long ldw, int np, const KfTile* __restrict__ tiles,
                                                            const KfFold* __restrict__ folds, const int32_t* __restrict__ idx, double* __restrict__ P) {
    __shared__ double sm[2][64 * KF_LS];
    __shared__ int rows[128];
    const KfTile tl = tiles[blockIdx.x];
    const KfFold fo = folds[tl.fold];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
    if (t < 128) {
        const int r = (t < 64 ? tl.I * 64 + t : tl.J * 64 + t - 64);
        rows[t] = r < fo.cnt ? idx[fo.off + r] : -1;
    }
    __syncthreads();
    const int kcol = t & (KF_KC - 1), rsub = t >> 5;  // 8 row groups of 32 lanes
    int gi[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) gi[q] = rows[rsub + 8 * q];
    double pre[16];
    auto load = [&](int kk) {
        const int k = kk + kcol;
#pragma unroll
        for (int q = 0; q < 16; ++q) pre[q] = (gi[q] >= 0 && k >= gi[q]) ? (double)W[(long)gi[q] * ldw + k] : 0.0;
    };
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4_t)(0.0);
    const double* As = sm[0] + (wr * 32 + (l & 15)) * KF_LS + (l >> 4);
    const double* Bs = sm[1] + (wc * 32 + (l & 15)) * KF_LS + (l >> 4);
    const int k0 = rows[0] & ~(KF_KC - 1);
    load(k0);
    for (int kk = k0; kk < np; kk += KF_KC) {
        __syncthreads();  // the previous chunk's MFMAs have read the stage
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = rsub + 8 * q;
            sm[r >> 6][(r & 63) * KF_LS + kcol] = pre[q];
        }
        __syncthreads();
        if (kk + KF_KC < np) load(kk + KF_KC);
#pragma unroll
        for (int ks = 0; ks < KF_KC; ks += 4) {
            const double a0 = As[ks], a1 = As[16 * KF_LS + ks], b0 = Bs[ks], b1 = Bs[16 * KF_LS + ks];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double* Pf = P + fo.poff;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = tl.I * 64 + wr * 32 + i * 16 + (l >> 4) + 4 * r, col = tl.J * 64 + wc * 32 + j * 16 + (l & 15);
                Pf[(long)row * fo.ldp + col] = (row == col && row >= fo.cnt) ? 1.0 : acc[i][j][r];
            }
}

// Sum over the workgroup in a fixed order: a butterfly per wave, then the 16 wave sums added by every thread in wave order.  red: 16 doubles of LDS.
__device__ __forceinline__ double kf_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int i = 0; i < KF_NT / 64; ++i) s += red[i];
    return s;
}
// D (LDS, lower 64×64) from the tile at A, in full; the caller synchronises.
__device__ __forceinline__ void kf_load_tile(double* D, const double* A, long ld) {
    for (int e = threadIdx.x; e < 4096; e += KF_NT) D[(e >> 6) * KF_DS + (e & 63)] = A[(long)(e >> 6) * ld + (e & 63)];
}
// Di = D⁻¹ for the lower-triangular D, upper part zero: lane j of the first wave solves column j by forward substitution (D_ik is a broadcast read,
// Di_kj falls on 64 consecutive banks).  Each lane reads back only what it wrote; the caller synchronises.
__device__ __forceinline__ void kf_invert_tile(const double* D, double* Di) {
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;
        for (int i = 0; i < 64; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s = fma(-D[i * KF_DS + k], Di[k * KF_DS + j], s);
            Di[i * KF_DS + j] = i < j ? 0.0 : s / D[i * KF_DS + i];
        }
    }
}
// The tile at A (global, row stride ld) ← the LDS tile D: its lower part, zeros above the diagonal
__device__ __forceinline__ void kf_store_lower(double* A, long ld, const double* D) {
    for (int e = threadIdx.x; e < 4096; e += KF_NT) {
        const int i = e >> 6, k = e & 63;
        A[(long)i * ld + k] = k <= i ? D[i * KF_DS + k] : 0.0;
    }
}
// q-th 32×32 sub-tile (ti >= tj) of a lower triangle, row by row
__device__ __forceinline__ void kf_tri(int q, int& ti, int& tj) {
    ti = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= q) ++ti;
    while (ti * (ti + 1) / 2 > q) --ti;
    tj = q - ti * (ti + 1) / 2;
}

// One workgroup (16 waves) per fold, on the block kfold_gram_kernel left.
//   Blocked Cholesky P_FF = R Rᵀ in place, 64 columns at a time: the diagonal tile is factored in LDS (D) and inverted there (Di); the rows below become
//   X = A·Di ᵀ on the MFMA, 16 rows per wave, each wave holding its rows' 64 columns in registers before it overwrites them; the trailing lower triangle
//   takes −X Xᵀ in 32×32 sub-tiles per wave, operands from L2.  The forward solve u = R⁻¹ α_F rides along: u_p = Di v_p, v_below −= X u_p.
//   lp = −½‖u‖² + Σ log R_ii − ½|F| log 2π.
//   mean (want_mean): r = R⁻ᵀ u by a blocked backward solve — column sums of the tiles below, then the diagonal tile in LDS on one wave —
//     mean[idx] = y − r.
//   var (want_var): R⁻¹ in place, block row by block row: T = R_b,<b · R⁻¹_<b,<b into the scratch panel behind the block, then R⁻¹_b,<b = −Di·T and
//     R⁻¹_bb = Di; var[idx_i] = Σ_{k ≥ i} (R⁻¹)_ki².
// A pivot that is not positive sets info[fold] = 1 and ends the workgroup with nothing written.  Padded rows (identity in P_FF, zero in α_F) add nothing.
// mean / var: n doubles in the caller's order; lp, info: one entry per fold.
template <typename T>
__global__ __launch_bounds__(KF_NT) void kfold_fact_kernel(const KfFold* __restrict__ folds, const int32_t* __restrict__ idx, double* P,
                                                            const T* __restrict__ alpha, const T* __restrict__ y, int want_mean, int want_var,
                                                            double* __restrict__ lp, double* __restrict__ mean, double* __restrict__ var,
                                                            int32_t* __restrict__ info) {
    __shared__ double D[64 * KF_DS], Di[64 * KF_DS], u[1024], red[16 * 64], dg[64];
    const KfFold fo = folds[blockIdx.x];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, lr = l & 15, lk = l >> 4;
    const int m = fo.npad, nbk = m / 64, cnt = fo.cnt;
    const long ld = fo.ldp;
    double* A = P + fo.poff;
    const int32_t* ix = idx + fo.off;
    if (t == 0) info[blockIdx.x] = 0;
    u[t] = t < cnt ? (double)alpha[ix[t]] : 0.0;

    for (int p = 0; p < nbk; ++p) {
        const int c0 = 64 * p, below = m - c0 - 64;
        double* App = A + (long)c0 * ld + c0;
        kf_load_tile(D, App, ld);
        __syncthreads();
        for (int j = 0; j < 64; ++j) {
            const double d = D[j * KF_DS + j];  // written before the last barrier; nobody writes it in this step
            if (!(d > 0.0)) {                   // the same value in every thread: the whole workgroup leaves
                if (t == 0) info[blockIdx.x] = 1;
                return;
            }
            const double s = sqrt(d);
            if (t == j) dg[j] = s;
            else if (t > j && t < 64) D[t * KF_DS + j] /= s;
            __syncthreads();
            for (int e = t; e < 4096; e += KF_NT) {
                const int i = e >> 6, k = e & 63;
                if (k > j && i >= k) D[i * KF_DS + k] = fma(-D[i * KF_DS + j], D[k * KF_DS + j], D[i * KF_DS + k]);
            }
            __syncthreads();
        }
        if (t < 64) D[t * KF_DS + t] = dg[t];
        __syncthreads();
        kf_invert_tile(D, Di);
        kf_store_lower(App, ld, D);
        __syncthreads();
        if (t < 64) {  // u_p = Di v_p: every lane's reads are issued before the wave's store
            double s = 0;
            for (int k = 0; k <= t; ++k) s = fma(Di[t * KF_DS + k], u[c0 + k], s);
            u[c0 + t] = s;
        }
        // X = A_below Diᵀ, 16 rows per wave
        for (int st = w; st < below / 16; st += KF_NT / 64) {
            double* Ar = A + (long)(c0 + 64 + 16 * st) * ld + c0;
            double a[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) a[s] = Ar[(long)lr * ld + 4 * s + lk];
#pragma unroll 1
            for (int jb = 0; jb < 4; ++jb) {  // the 16 columns jb: all of a[] is in registers before the first store
                d4_t acc = (d4_t)(0.0);
#pragma unroll
                for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Di[(jb * 16 + lr) * KF_DS + 4 * s + lk], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) Ar[(long)(lk + 4 * r) * ld + jb * 16 + lr] = acc[r];
            }
        }
        __syncthreads();
        // v_below −= X u_p: 16 lanes per row, 4 columns each, 64 rows per pass
        for (int r0 = 0; r0 < below; r0 += 64) {
            const int row = c0 + 64 + r0 + (t >> 4);
            const double* xr = A + (long)row * ld + c0 + 4 * (t & 15);
            double s = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s = fma(xr[k], u[c0 + 4 * (t & 15) + k], s);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if ((t & 15) == 0) u[row] -= s;
        }
        // trailing lower triangle −= X Xᵀ
        const int nt = below / 32;
        for (int q = w; q < nt * (nt + 1) / 2; q += KF_NT / 64) {
            int ti, tj;
            kf_tri(q, ti, tj);
            const double* Xa = A + (long)(c0 + 64 + 32 * ti + lr) * ld + c0 + lk;
            const double* Xb = A + (long)(c0 + 64 + 32 * tj + lr) * ld + c0 + lk;
            d4_t acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = (d4_t)(0.0);
#pragma unroll 4
            for (int s = 0; s < 64; s += 4) {
                const double a0 = Xa[s], a1 = Xa[16 * ld + s], b0 = Xb[s], b1 = Xb[16 * ld + s];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
            double* Ct = A + (long)(c0 + 64 + 32 * ti) * ld + c0 + 64 + 32 * tj;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Ct[(long)(i * 16 + lk + 4 * r) * ld + j * 16 + lr] -= acc[i][j][r];
        }
        __syncthreads();
    }

    {
        const double term = t < m ? fma(-0.5 * u[t], u[t], log(A[(long)t * ld + t])) : 0.0;
        const double s = kf_block_sum(term, red);
        if (t == 0) lp[blockIdx.x] = s - 0.5 * 1.8378770664093454835606594728112 * cnt;
    }

    if (want_mean) {
        // r = R⁻ᵀ u, block by block from the end; r takes u's place
        __syncthreads();
        for (int p = nbk - 1; p >= 0; --p) {
            const int c0 = 64 * p;
            kf_load_tile(D, A + (long)c0 * ld + c0, ld);
            double s = 0;
            for (int i = c0 + 64 + w; i < m; i += KF_NT / 64) s = fma(A[(long)i * ld + c0 + l], u[i], s);
            red[w * 64 + l] = s;
            __syncthreads();
            if (t < 64) {
                double v = u[c0 + t];
#pragma unroll
                for (int g = 0; g < KF_NT / 64; ++g) v -= red[g * 64 + t];
                double x = 0;
                for (int j = 63; j >= 0; --j) {
                    const double xj = __shfl(v / D[j * KF_DS + j], j, 64);
                    if (t == j) x = xj;
                    else if (t < j) v = fma(-D[j * KF_DS + t], xj, v);
                }
                u[c0 + t] = x;
            }
            __syncthreads();
        }
        if (t < cnt) mean[ix[t]] = (double)y[ix[t]] - u[t];
    }

    if (want_var) {
        double* S = A + (long)m * ld;  // the scratch panel: 64 rows
        __syncthreads();
        for (int b = 0; b < nbk; ++b) {
            double* Ab = A + (long)(64 * b) * ld;
            kf_load_tile(D, Ab + 64 * b, ld);
            __syncthreads();
            kf_invert_tile(D, Di);
            // S = R_b,<b · R⁻¹_<b,<b: sub-tile (si, sj) sums over k from the start of sj's block column to the end of block b − 1
            for (int q = w; q < 4 * b; q += KF_NT / 64) {
                const int si = q & 1, sj = q >> 1;
                const double* Ra = Ab + (long)(32 * si + lr) * ld + lk;
                const double* Rb = A + (long)lk * ld + 32 * sj + lr;
                d4_t acc[2][2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = (d4_t)(0.0);
                for (int k = (sj >> 1) * 64; k < 64 * b; k += 4) {
                    const double a0 = Ra[k], a1 = Ra[16 * ld + k], b0 = Rb[(long)k * ld], b1 = Rb[(long)k * ld + 16];
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) S[(long)(32 * si + i * 16 + lk + 4 * r) * ld + 32 * sj + j * 16 + lr] = acc[i][j][r];
            }
            __syncthreads();
            // R⁻¹_b,<b = −Di·S;  R⁻¹_bb = Di
            for (int q = w; q < 4 * b; q += KF_NT / 64) {
                const int si = q & 1, sj = q >> 1;
                const double* Da = Di + (32 * si + lr) * KF_DS + lk;
                const double* Sb = S + (long)lk * ld + 32 * sj + lr;
                d4_t acc[2][2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = (d4_t)(0.0);
#pragma unroll 4
                for (int k = 0; k < 64; k += 4) {
                    const double a0 = Da[k], a1 = Da[16 * KF_DS + k], b0 = Sb[(long)k * ld], b1 = Sb[(long)k * ld + 16];
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) Ab[(long)(32 * si + i * 16 + lk + 4 * r) * ld + 32 * sj + j * 16 + lr] = -acc[i][j][r];
            }
            kf_store_lower(Ab + 64 * b, ld, Di);
            __syncthreads();
        }
        // var_i = Σ_{k ≥ i} (R⁻¹)_ki²: a column block at a time, 16 row groups, added in group order (the diagonal tile's upper part is zero)
        for (int cb = 0; cb < nbk; ++cb) {
            const int col = 64 * cb + l;
            double s = 0;
            for (int k = 64 * cb + w; k < m; k += KF_NT / 64) {
                const double v = A[(long)k * ld + col];
                s = fma(v, v, s);
            }
            red[w * 64 + l] = s;
            __syncthreads();
            if (t < 64 && col < cnt) {
                double v = 0;
#pragma unroll
                for (int g = 0; g < KF_NT / 64; ++g) v += red[g * 64 + t];
                var[ix[col]] = v;
            }
            __syncthreads();
        }
    }
}

}  // namespace gpmi
