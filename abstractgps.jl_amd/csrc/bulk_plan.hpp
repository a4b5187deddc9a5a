// bulk_plan.hpp — the plan of ONE bulk trailing update C(m×m, lower) −= P·Pᵀ (+ the carried rows below the square), host only.
//   Plain C++: no HIP header, nothing touches the device (tests/bulk_plan_check.cpp includes it with the host compiler alone).
//
//   The recursion is the one of syrk_lower_split / gemm_nt_strassen (gpmi355.hip): a lower SYRK of side m is cut by rows at h = ⌊m/2⌋ rounded down to
//   256 while an h×h block still has the Strassen shape; the block between the two half-size SYRKs takes whole 256-row pieces in the Strassen form
//   (seven half-size products in four ordered launches: M1, then M2|M5, M3|M4, M6|M7), the rest are classical pieces: leaf SYRKs (lower), the
//   b − bs remainder strip, the carried rows.
//
//   Launch i of one block and launch i of every other block of the same update write disjoint parts of C, and so do all classical pieces.  The
//   plan therefore puts the WHOLE update into four ordered lists of tile problems — one grouped launch each (kernels.hpp gemm_nt_grp_kernel) —
//   instead of four launches per block: four partly filled last rounds of workgroups per update, however deep the split.  Every quadrant still
//   receives its products in the fixed order; no tile's arithmetic changes.  All blocks of an update are live at once, so each has its own slice
//   of sum panels.
//
//   U1, the update of the next panel's columns, is the same kind of update with a square that is never split and a tall rectangle below it: u1_plan_build
//   puts the rectangle's whole quadrants through the same Builder::strassen and the rest through the same classical pieces and the same four lists
//   (tests/u1_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace gpmi {

// number of (r, c) in [row0,row0+M) × [col0,col0+N) with c <= r  (closed form)
static inline double lower_count(long M, long N, long row0, long col0) {
    const long a = row0 - col0 + 1;  // count in the first row before clamping to [0, N]
    const long i1 = std::min(std::max(1 - a, 0L), M);                // rows contributing 0
    const long i2 = std::max(i1, std::min(std::max(N - a, 0L), M));  // rows from i2 on contribute N
    const double mid = (double)(i2 - i1) * (double)a + 0.5 * (double)(i1 + i2 - 1) * (double)(i2 - i1);
    return mid + (double)(M - i2) * (double)N;
}

// shapes the Strassen form takes: quadrants of whole 128×128 tiles, whole k steps per half
static inline bool strassen_shape_rule(long min_rows, long M, long N, long K) {
    return min_rows > 0 && std::min(M, N) >= std::max(256L, min_rows) && M % 256 == 0 && N % 256 == 0 && K % 32 == 0;
}
// side of the off-diagonal block the lower SYRK of side m is split at (multiple of 256); 0: no split
static inline long strassen_split_rule(long min_rows, long m, long K) {
    const long h = (m / 2) / 256 * 256;
    return strassen_shape_rule(min_rows, h, h, K) ? h : 0;
}
static inline size_t strassen_ws_rule(long ldpad, long M, long N, long K) { return (size_t)5 * (size_t)(M / 2 + N / 2) * (size_t)(K / 2 + ldpad); }
// tiles a single launch enumerates: the compact lower trapezoid (dt = 0: the square sits on the diagonal) or the whole rectangle
static inline long plan_tiles(long M, long N, int lower) {
    const long tm = (M + 127) / 128, tn = (N + 127) / 128;
    if (!lower) return tm * tn;
    const long tri = std::min(tm, tn);
    return tri + tri * (tri - 1) / 2 + (tm - tri) * tn;
}

// One tile problem C −= A·Bᵀ of a grouped launch.  Offsets are in elements: c_off from the update's C, a_off / b_off from P (src 0, row stride ldp)
// or from the workspace (src 1, row stride lds).
struct PlanProb {
    long c_off, a_off, b_off;
    int a_src, b_src;
    long M, N, K;
    int lower;       // 1: leaf SYRK (row0 = col0 = the update's row0 + roff)
    long roff;       // lower: offset of the square on the update's diagonal
    int beta0;       // 1: a Strassen product — accumulated from zero, C[c_off + ·] −= s1·acc and, with c2off != 0, C[c_off + c2off + ·] −= s2·acc
    long c2off;
    int s1, s2;
    long tile0, ntiles;  // first tile index inside its launch / number of tiles
    int block, product;  // Strassen: index into BulkPlan::blocks and 1..7; classical: −1, 0
};
struct PlanSums {  // one launch of strassen_sums_kernel: X = P + x_off (rows × 2·kh, row stride ldp) -> five panels at ws + s_off, pstride apart, row stride lds
    long x_off, rh, kh;
    int side;
    long s_off, pstride;
};
struct PlanBlock {  // one Strassen block: C + c_off (M×N) −= (P + a_off)(P + b_off)ᵀ; its ten sum panels: ws + [s_off, s_off + s_elems)
    long c_off, a_off, b_off, M, N, K;
    long s_off, s_elems;
};
struct PlanLaunch {  // the ungrouped sequence (what syrk_lower_split issues without grouping): kind 0 tile GEMM (nbatch products), 1 sums
    int kind;
    long M, N, K;
    int nbatch, lower;
};
struct BulkPlan {
    long mrows = 0, m = 0, K = 0, row0 = 0, ldc = 0, ldp = 0, lds = 0;
    std::vector<PlanBlock> blocks;
    std::vector<PlanSums> sums;
    std::vector<PlanProb> list[4];
    long ntiles[4] = {0, 0, 0, 0};
    double flops[4] = {0, 0, 0, 0}, bytes[4] = {0, 0, 0, 0};  // per launch, summed over its problems as launch_gemm counts a single launch
    size_t ws_elems = 0;
    std::vector<PlanLaunch> ungrouped;
    size_t nprobs() const { return list[0].size() + list[1].size() + list[2].size() + list[3].size(); }
};

namespace plan_detail {
struct Builder {
    BulkPlan& p;
    long min_rows, ldpad;
    std::vector<PlanProb> classical;

    void rect(long c_off, long a_off, long b_off, long M, long N) {
        if (M <= 0 || N <= 0) return;
        PlanProb e{};
        e.c_off = c_off; e.a_off = a_off; e.b_off = b_off;
        e.M = M; e.N = N; e.K = p.K;
        e.block = -1;
        classical.push_back(e);
        p.ungrouped.push_back(PlanLaunch{0, M, N, p.K, 1, 0});
    }
    void product(int launch, int product, int block, long c_off, long c2off, int s1, int s2, int a_src, long a_off, int b_src, long b_off, long mh, long nh, long kh) {
        PlanProb e{};
        e.c_off = c_off; e.a_off = a_off; e.b_off = b_off;
        e.a_src = a_src; e.b_src = b_src;
        e.M = mh; e.N = nh; e.K = kh;
        e.beta0 = 1; e.c2off = c2off; e.s1 = s1; e.s2 = s2;
        e.block = block; e.product = product;
        p.list[launch].push_back(e);
    }
    // C + c_off (M×N) −= (P + a_off)(P + b_off)ᵀ in the Strassen form (gemm_nt_strassen: same panels, products, signs and targets)
    void strassen(long c_off, long a_off, long b_off, long M, long N) {
        const long K = p.K;
        if (!strassen_shape_rule(min_rows, M, N, K)) return rect(c_off, a_off, b_off, M, N);
        const long mh = M / 2, nh = N / 2, kh = K / 2, lds = p.lds, ldp = p.ldp;
        const long pa = mh * lds, pb = nh * lds;
        const int bi = (int)p.blocks.size();
        const long sa = (long)p.ws_elems, sb = sa + 5 * pa;
        p.blocks.push_back(PlanBlock{c_off, a_off, b_off, M, N, K, sa, 5 * (pa + pb)});
        p.ws_elems += (size_t)(5 * (pa + pb));
        p.sums.push_back(PlanSums{a_off, mh, kh, 0, sa, pa});  // A11+A22, A21+A22, A11+A12, A21−A11, A12−A22
        p.sums.push_back(PlanSums{b_off, nh, kh, 1, sb, pb});  // B11+B22, B21−B22, B12−B11, B11+B21, B12+B22
        const long dn = nh, dm = mh * p.ldc;                   // C11 = c, C12 = c + dn, C21 = c + dm, C22 = c + dm + dn
        product(0, 1, bi, c_off, dm + dn, 1, 1, 1, sa, 1, sb, mh, nh, kh);                              // M1 = (A11+A22)(B11+B22)ᵀ -> C11, C22
        product(1, 2, bi, c_off + dm, dn, 1, -1, 1, sa + pa, 0, b_off, mh, nh, kh);                     // M2 = (A21+A22) B11ᵀ -> C21, −C22
        product(1, 5, bi, c_off + dn, -dn, 1, -1, 1, sa + 2 * pa, 0, b_off + nh * ldp + kh, mh, nh, kh);  // M5 = (A11+A12) B22ᵀ -> C12, −C11
        product(2, 3, bi, c_off + dn, dm, 1, 1, 0, a_off, 1, sb + pb, mh, nh, kh);                      // M3 = A11 (B21−B22)ᵀ -> C12, C22
        product(2, 4, bi, c_off, dm, 1, 1, 0, a_off + mh * ldp + kh, 1, sb + 2 * pb, mh, nh, kh);       // M4 = A22 (B12−B11)ᵀ -> C11, C21
        product(3, 6, bi, c_off + dm + dn, 0, 1, 0, 1, sa + 3 * pa, 1, sb + 3 * pb, mh, nh, kh);        // M6 = (A21−A11)(B11+B21)ᵀ -> C22
        product(3, 7, bi, c_off, 0, 1, 0, 1, sa + 4 * pa, 1, sb + 4 * pb, mh, nh, kh);                  // M7 = (A12−A22)(B12+B22)ᵀ -> C11
        p.ungrouped.push_back(PlanLaunch{1, mh, kh, 0, 1, 0});
        p.ungrouped.push_back(PlanLaunch{1, nh, kh, 0, 1, 0});
        p.ungrouped.push_back(PlanLaunch{0, mh, nh, kh, 1, 0});
        for (int i = 0; i < 3; ++i) p.ungrouped.push_back(PlanLaunch{0, mh, nh, kh, 2, 0});
    }
    // one classical lower piece: the square of side m at offset roff on the update's diagonal with the mrows − m rows below it
    void leaf(long roff, long mrows, long m) {
        PlanProb e{};
        e.c_off = roff * p.ldc + roff; e.a_off = roff * p.ldp; e.b_off = roff * p.ldp;
        e.M = mrows; e.N = m; e.K = p.K;
        e.lower = 1; e.roff = roff;
        e.block = -1;
        classical.push_back(e);
        p.ungrouped.push_back(PlanLaunch{0, mrows, m, p.K, 1, 1});
    }
    // the square of side m at offset roff on the update's diagonal, mrows >= m rows in all (syrk_lower_split)
    void syrk(long roff, long mrows, long m) {
        const long K = p.K, ldc = p.ldc, ldp = p.ldp;
        const long h = strassen_split_rule(min_rows, m, K);
        if (h == 0) return leaf(roff, mrows, m);
        const long b = m - h, bs = b / 256 * 256;  // rows below the split; the Strassen block takes whole 256-row pieces of them
        syrk(roff, h, h);
        strassen((roff + h) * ldc + roff, (roff + h) * ldp, roff * ldp, bs, h);
        if (b > bs) rect((roff + h + bs) * ldc + roff, (roff + h + bs) * ldp, roff * ldp, b - bs, h);
        syrk(roff + h, b, b);
        if (mrows > m) rect((roff + m) * ldc + roff, (roff + m) * ldp, roff * ldp, mrows - m, m);
    }
};
// The four lists of a plan from the builder's products and classical pieces: balance, order, tile prefix sums, flops and bytes per launch.
static inline void finish(BulkPlan& p, Builder& bd, long row0) {
    // The classical pieces write parts of C nothing else of the update touches: each goes to the launch with the least work so far (tiles × k steps),
    // largest first.  Launch 1 holds one product per block against two in the others, so it takes most of them.
    double work[4];
    for (int l = 0; l < 4; ++l) {
        work[l] = 0;
        for (auto& e : p.list[l]) work[l] += (double)plan_tiles(e.M, e.N, e.lower) * (double)e.K;
    }
    std::stable_sort(bd.classical.begin(), bd.classical.end(), [](const PlanProb& a, const PlanProb& b) {
        return plan_tiles(a.M, a.N, a.lower) * a.K > plan_tiles(b.M, b.N, b.lower) * b.K;
    });
    for (auto& e : bd.classical) {
        int l = 0;
        for (int i = 1; i < 4; ++i)
            if (work[i] < work[l]) l = i;
        work[l] += (double)plan_tiles(e.M, e.N, e.lower) * (double)e.K;
        p.list[l].push_back(e);
    }
    for (int l = 0; l < 4; ++l) {
        // decreasing K, then decreasing size: the launch drains on its short tiles
        std::stable_sort(p.list[l].begin(), p.list[l].end(), [](const PlanProb& a, const PlanProb& b) {
            if (a.K != b.K) return a.K > b.K;
            return plan_tiles(a.M, a.N, a.lower) > plan_tiles(b.M, b.N, b.lower);
        });
        long t = 0;
        for (auto& e : p.list[l]) {
            e.tile0 = t;
            e.ntiles = plan_tiles(e.M, e.N, e.lower);
            t += e.ntiles;
            const double elems = e.lower ? lower_count(e.M, e.N, row0 + e.roff, row0 + e.roff) : (double)e.M * (double)e.N;
            p.flops[l] += 2.0 * (double)e.K * elems;
            p.bytes[l] += 16.0 * elems * (e.c2off ? 2 : 1) + 8.0 * (double)e.K * (double)(e.M + e.N);
        }
        p.ntiles[l] = t;
    }
}
}  // namespace plan_detail

// The plan of C(mrows × m; the m×m square lower, at row0 on the global diagonal) −= P·P[0:m]ᵀ, P = mrows × K.  min_rows: "strassen_min_rows".
static inline BulkPlan bulk_plan_build(long mrows, long m, long K, long row0, long ldc, long ldp, long min_rows, long ldpad) {
    BulkPlan p;
    p.mrows = mrows; p.m = m; p.K = K; p.row0 = row0; p.ldc = ldc; p.ldp = ldp;
    p.lds = K / 2 + ldpad;
    plan_detail::Builder bd{p, min_rows, ldpad, {}};
    bd.syrk(0, mrows, m);
    plan_detail::finish(p, bd, row0);
    return p;
}

// U1, the update of the next panel's columns: C(mrows × nb1; the nb1×nb1 square lower, at row0 on the global diagonal) −= P·P[0:nb1]ᵀ, P = mrows × K.
// Below the square lie the mrect rows of the matrix under the next panel and then the carried right-hand-side rows.  The whole 256-row quadrants of
// the rectangle (rows [nb1, nb1 + bs), bs = mrect rounded down to 256) are ONE Strassen block — A = P from row nb1 on, B = P[0:nb1] — when that
// block has at least u1_min_rows rows ("strassen_u1_min_rows"; 0: never), the panel at least u1_min_k columns ("strassen_u1_min_k": what a half-size
// product costs beyond its flops does not shrink with K/2) and the block the Strassen shape.
static inline long u1_block_rows(long u1_min_rows, long u1_min_k, long mrect, long nb1, long K) {
    const long bs = mrect / 256 * 256;
    return u1_min_rows > 0 && bs >= u1_min_rows && K >= u1_min_k && strassen_shape_rule(256, bs, nb1, K) ? bs : 0;
}
// The plan of U1 in that form: the square stays one classical lower piece, the block goes through Builder::strassen (the sums, products, signs, targets
// and launch order of every other block), the remainder strip and the carried rows are classical rectangles; finish() balances them over the same four
// lists.  Call it only where u1_block_rows() > 0.
static inline BulkPlan u1_plan_build(long mrows, long mrect, long nb1, long K, long row0, long ldc, long ldp, long ldpad) {
    BulkPlan p;
    p.mrows = mrows; p.m = nb1; p.K = K; p.row0 = row0; p.ldc = ldc; p.ldp = ldp;
    p.lds = K / 2 + ldpad;
    plan_detail::Builder bd{p, 256, ldpad, {}};
    const long bs = mrect / 256 * 256, carried = mrows - nb1 - mrect;
    bd.leaf(0, nb1, nb1);
    bd.strassen(nb1 * ldc, nb1 * ldp, 0, bs, nb1);
    bd.rect((nb1 + bs) * ldc, (nb1 + bs) * ldp, 0, mrect - bs, nb1);
    bd.rect((nb1 + mrect) * ldc, (nb1 + mrect) * ldp, 0, carried, nb1);
    plan_detail::finish(p, bd, row0);
    return p;
}

// One entry of the device table of a grouped launch (kernels.hpp gemm_nt_grp_kernel): a tile problem with absolute pointers.
struct GrpProb {
    double* C;
    const double* A;
    const double* B;
    long ldc, lda, ldb;
    long row0, col0;  // lower: position on the global diagonal
    long c2off;
    int M, N, K;
    int lower, tn, beta0, s1, s2;
    int tile0;        // first tile index of this problem in the launch (entries ascend)
    int pad_[5];
};
static_assert(sizeof(GrpProb) == 128, "one table entry is 128 bytes");

static inline GrpProb plan_entry(const BulkPlan& p, const PlanProb& e, double* C, const double* P, const double* ws) {
    GrpProb q{};
    q.C = C + e.c_off;
    q.A = (e.a_src ? ws : P) + e.a_off;
    q.B = (e.b_src ? ws : P) + e.b_off;
    q.ldc = p.ldc;
    q.lda = e.a_src ? p.lds : p.ldp;
    q.ldb = e.b_src ? p.lds : p.ldp;
    q.row0 = q.col0 = e.lower ? p.row0 + e.roff : 0;
    q.c2off = e.c2off;
    q.M = (int)e.M; q.N = (int)e.N; q.K = (int)e.K;
    q.lower = e.lower;
    q.tn = (int)((e.N + 127) / 128);
    q.beta0 = e.beta0; q.s1 = e.s1; q.s2 = e.s2;
    q.tile0 = (int)e.tile0;
    return q;
}

}  // namespace gpmi
