// Stand-alone check of csrc/bulk_plan.hpp (host only; built and run by tests/test_bulk_plan_cpu.py with the host compiler and
// -fsanitize=address,undefined).  For every case of a grid of update shapes it builds the plan and checks, independently of the builder's own bookkeeping:
//   disjoint   within each of the four lists all target rectangles are pairwise disjoint
//   order      every quadrant of every Strassen block receives its products in the fixed order (M1, M2|M5, M3|M4, M6|M7)
//   coverage   every 64×64 cell of the lower window and of the carried rows is updated over exactly the k range K, every other cell not at all; a Strassen
//              block counts only after its seven products, decoded from their operand and target OFFSETS and expanded on 2×2 blocks, sum to A·Bᵀ
//   workspace  the blocks' slices are disjoint and inside the reported size; every panel a product reads lies in its block's slice and is written by a sums job
//   tiles      first-tile prefix sums, tile counts and the grid size agree; entries are ordered by decreasing K
//   sequence   the ungrouped launch sequence has the count of an independent recursion, and the flops of both forms agree
// Output: one "FAIL <check> <case>: <what>" line per violation, "COUNT m K launches" lines for the pinned cases, and a last line "cases <n> fails <n>".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../abstractgps.jl_amd/csrc/bulk_plan.hpp"

using namespace gpmi;

static long g_fails = 0;
static std::string g_case;
static void fail(const char* check, const std::string& what) {
    ++g_fails;
    if (g_fails <= 200) printf("FAIL %s %s: %s\n", check, g_case.c_str(), what.c_str());
}
static std::string S(long v) { return std::to_string(v); }

struct Rect {
    long r0, r1, c0, c1;
    int idx;
};
static bool meet(const Rect& a, const Rect& b) { return a.r0 < b.r1 && b.r0 < a.r1 && a.c0 < b.c1 && b.c0 < a.c1; }

// GEMM launches of today's recursion (syrk_lower_split / gemm_nt_strassen), written out again
static long count_launches(long min_rows, long mrows, long m, long K) {
    const long h = strassen_split_rule(min_rows, m, K);
    if (h == 0) return 1;
    const long b = m - h, bs = b / 256 * 256;
    long n = count_launches(min_rows, h, h, K) + (strassen_shape_rule(min_rows, bs, h, K) ? 4 : 1) + (b > bs ? 1 : 0) + count_launches(min_rows, b, b, K);
    return n + (mrows > m ? 1 : 0);
}

// coefficients over (X11, X12, X21, X22) of the five panels strassen_sums_kernel writes (kernels.hpp), per side
static const int SUMS[2][5][4] = {{{1, 0, 0, 1}, {0, 0, 1, 1}, {1, 1, 0, 0}, {-1, 0, 1, 0}, {0, 1, 0, -1}},
                                  {{1, 0, 0, 1}, {0, 0, 1, -1}, {-1, 1, 0, 0}, {1, 0, 1, 0}, {0, 1, 0, 1}}};

static void check_case(long mrows, long m, long K, long min_rows, long ldpad) {
    const long row0 = 384, ldc = m + 40, ldp = K + 32;
    g_case = "m=" + S(m) + " mrows=" + S(mrows) + " K=" + S(K) + " min=" + S(min_rows);
    const BulkPlan p = bulk_plan_build(mrows, m, K, row0, ldc, ldp, min_rows, ldpad);
    const long R = mrows / 64, Cn = m / 64;
    std::vector<long> cover((size_t)R * (size_t)Cn, 0);
    auto paint = [&](long r0, long c0, long M, long N, long k, bool lower) {
        if (r0 < 0 || c0 < 0 || r0 + M > mrows || c0 + N > m || r0 % 64 || c0 % 64 || M % 64 || N % 64) return fail("coverage", "target outside the update or off the 64 grid");
        for (long r = r0 / 64; r < (r0 + M) / 64; ++r)
            for (long c = c0 / 64; c < (c0 + N) / 64; ++c)
                if (!lower || c <= r) cover[(size_t)r * Cn + c] += k;
    };

    // ---- workspace ----
    for (size_t i = 0; i < p.blocks.size(); ++i) {
        const PlanBlock& b = p.blocks[i];
        if (b.s_off < 0 || (size_t)(b.s_off + b.s_elems) > p.ws_elems) fail("workspace", "slice of block " + S((long)i) + " outside the reported size");
        for (size_t j = 0; j < i; ++j)
            if (b.s_off < p.blocks[j].s_off + p.blocks[j].s_elems && p.blocks[j].s_off < b.s_off + b.s_elems) fail("workspace", "slices of blocks " + S((long)j) + " and " + S((long)i) + " meet");
        const long mh = b.M / 2, nh = b.N / 2, kh = b.K / 2, pa = mh * p.lds, pb = nh * p.lds;
        if (p.lds < kh || b.s_elems != 5 * (pa + pb)) fail("workspace", "slice size of block " + S((long)i));
        int seen[2] = {0, 0};
        for (const PlanSums& s : p.sums) {
            if (s.side == 0 && s.s_off == b.s_off && s.x_off == b.a_off && s.rh == mh && s.kh == kh && s.pstride == pa) ++seen[0];
            if (s.side == 1 && s.s_off == b.s_off + 5 * pa && s.x_off == b.b_off && s.rh == nh && s.kh == kh && s.pstride == pb) ++seen[1];
        }
        if (seen[0] != 1 || seen[1] != 1) fail("workspace", "block " + S((long)i) + " has no or several sums jobs per side");
    }
    if (p.sums.size() != 2 * p.blocks.size()) fail("workspace", "sums jobs without a block");

    // ---- per list: tiles, disjoint targets; per block: order and the symbolic expansion ----
    struct Hit {
        int launch, product;
    };
    std::vector<std::vector<Hit>> hits(p.blocks.size() * 4);         // per (block, quadrant)
    std::vector<std::vector<long>> coef(p.blocks.size() * 4, std::vector<long>(16, 0));  // per (block, quadrant): coefficient of (A quadrant, B quadrant)
    std::vector<int> nprod(p.blocks.size(), 0);
    double flops = 0;
    for (int l = 0; l < 4; ++l) {
        std::vector<Rect> rects;
        long t = 0, lastK = 1L << 40;
        for (size_t i = 0; i < p.list[l].size(); ++i) {
            const PlanProb& e = p.list[l][i];
            if (e.tile0 != t || e.ntiles != plan_tiles(e.M, e.N, e.lower) || e.ntiles <= 0) fail("tiles", "launch " + S(l) + " entry " + S((long)i) + ": first tile / count");
            if (e.K > lastK) fail("tiles", "launch " + S(l) + " entry " + S((long)i) + ": K ascends");
            lastK = e.K;
            t += e.ntiles;
            const long r0 = e.c_off / ldc, c0 = e.c_off % ldc;
            rects.push_back(Rect{r0, r0 + e.M, c0, c0 + e.N, (int)i});
            if (e.block < 0) {  // classical piece
                if (e.beta0 || e.a_src || e.b_src || e.K != K || e.a_off != r0 * ldp || e.b_off != c0 * ldp) fail("coverage", "classical piece with wrong operands");
                if (e.lower && (r0 != c0 || e.roff != r0)) fail("coverage", "lower piece off the diagonal");
                paint(r0, c0, e.M, e.N, e.K, e.lower != 0);
                flops += 2.0 * (double)e.K * (e.lower ? lower_count(e.M, e.N, 0, 0) : (double)e.M * (double)e.N);
                continue;
            }
            const PlanBlock& b = p.blocks[(size_t)e.block];
            const long mh = b.M / 2, nh = b.N / 2, kh = b.K / 2, pa = mh * p.lds, pb = nh * p.lds;
            ++nprod[(size_t)e.block];
            flops += 2.0 * (double)e.K * (double)e.M * (double)e.N;
            if (e.M != mh || e.N != nh || e.K != kh || !e.beta0 || e.lower || (e.s1 != 1 && e.s1 != -1)) fail("coverage", "product shape");
            // operands, decoded from their offsets
            long ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
            if (e.a_src) {
                const long rel = e.a_off - b.s_off;
                if (rel < 0 || rel % pa || rel / pa > 4) fail("workspace", "A panel of a product outside its block's slice");
                else for (int q = 0; q < 4; ++q) ca[q] = SUMS[0][rel / pa][q];
            } else {
                const long rel = e.a_off - b.a_off, qi = rel / (mh * ldp), qk = rel - qi * mh * ldp;
                if (rel < 0 || qi > 1 || (qk != 0 && qk != kh)) fail("coverage", "A operand is no quadrant");
                else ca[qi * 2 + (qk ? 1 : 0)] = 1;
            }
            if (e.b_src) {
                const long rel = e.b_off - (b.s_off + 5 * pa);
                if (rel < 0 || rel % pb || rel / pb > 4) fail("workspace", "B panel of a product outside its block's slice");
                else for (int q = 0; q < 4; ++q) cb[q] = SUMS[1][rel / pb][q];
            } else {
                const long rel = e.b_off - b.b_off, qi = rel / (nh * ldp), qk = rel - qi * nh * ldp;
                if (rel < 0 || qi > 1 || (qk != 0 && qk != kh)) fail("coverage", "B operand is no quadrant");
                else cb[qi * 2 + (qk ? 1 : 0)] = 1;
            }
            const long br0 = b.c_off / ldc, bc0 = b.c_off % ldc;
            for (int tg = 0; tg < 2; ++tg) {
                if (tg == 1 && e.c2off == 0) break;
                const long off = e.c_off + (tg ? e.c2off : 0), tr = off / ldc - br0, tc = off % ldc - bc0;
                const int sgn = tg ? e.s2 : e.s1;
                if ((tr != 0 && tr != mh) || (tc != 0 && tc != nh) || (sgn != 1 && sgn != -1)) {
                    fail("coverage", "product target is no quadrant");
                    continue;
                }
                const size_t q = (size_t)e.block * 4 + (tr ? 2 : 0) + (tc ? 1 : 0);
                hits[q].push_back(Hit{l, e.product});
                for (int x = 0; x < 4; ++x)
                    for (int y = 0; y < 4; ++y) coef[q][x * 4 + y] += sgn * ca[x] * cb[y];
                if (tg) rects.push_back(Rect{br0 + tr, br0 + tr + mh, bc0 + tc, bc0 + tc + nh, (int)i});
            }
        }
        if (t != p.ntiles[l]) fail("tiles", "launch " + S(l) + ": grid size " + S(p.ntiles[l]) + " against " + S(t) + " tiles");
        for (size_t a = 0; a < rects.size(); ++a)
            for (size_t b = 0; b < a; ++b)
                if (meet(rects[a], rects[b])) fail("disjoint", "launch " + S(l) + ": targets of entries " + S(rects[b].idx) + " and " + S(rects[a].idx) + " meet");
    }
    static const int ORDER[4][4][2] = {{{0, 1}, {1, 5}, {2, 4}, {3, 7}}, {{1, 5}, {2, 3}, {-1, 0}, {-1, 0}}, {{1, 2}, {2, 4}, {-1, 0}, {-1, 0}}, {{0, 1}, {1, 2}, {2, 3}, {3, 6}}};
    for (size_t bi = 0; bi < p.blocks.size(); ++bi) {
        const PlanBlock& b = p.blocks[bi];
        bool ok = nprod[bi] == 7;
        if (!ok) fail("coverage", "block " + S((long)bi) + " has " + S(nprod[bi]) + " products");
        for (int q = 0; q < 4; ++q) {
            const auto& h = hits[bi * 4 + q];
            const size_t want = (q == 0 || q == 3) ? 4 : 2;
            bool good = h.size() == want;
            for (size_t i = 0; good && i < want; ++i) good = h[i].launch == ORDER[q][i][0] && h[i].product == ORDER[q][i][1];
            if (!good) fail("order", "block " + S((long)bi) + " quadrant " + S(q));
            // C_ij −= A_i1 B_j1ᵀ + A_i2 B_j2ᵀ: coefficient 1 on (A_ik, B_jk), 0 elsewhere
            const int i = q >> 1, j = q & 1;
            for (int x = 0; x < 4; ++x)
                for (int y = 0; y < 4; ++y) {
                    const long want_c = ((x >> 1) == i && (y >> 1) == j && (x & 1) == (y & 1)) ? 1 : 0;
                    if (coef[bi * 4 + q][x * 4 + y] != want_c) ok = false;
                }
        }
        if (!ok) fail("coverage", "block " + S((long)bi) + ": the products do not sum to A·Bᵀ");
        else paint(b.c_off / ldc, b.c_off % ldc, b.M, b.N, 2 * (b.K / 2), false);
    }
    long bad = 0;
    for (long r = 0; r < R; ++r)
        for (long c = 0; c < Cn; ++c) {
            const long want = (r >= Cn || c <= r) ? K : 0;
            if (cover[(size_t)r * Cn + c] != want) ++bad;
        }
    if (bad) fail("coverage", S(bad) + " cells of 64×64 are not updated over exactly K");

    // ---- the ungrouped sequence ----
    long launches = 0;
    double uflops = 0;
    for (const PlanLaunch& u : p.ungrouped)
        if (u.kind == 0) {
            ++launches;
            uflops += 2.0 * (double)u.K * (u.lower ? lower_count(u.M, u.N, 0, 0) : (double)u.M * (double)u.N) * u.nbatch;
        }
    if (launches != count_launches(min_rows, mrows, m, K)) fail("sequence", "ungrouped launches " + S(launches) + " against " + S(count_launches(min_rows, mrows, m, K)));
    if (uflops != flops || flops != p.flops[0] + p.flops[1] + p.flops[2] + p.flops[3]) fail("sequence", "flops of the two forms differ");
    if (K == 256 && min_rows == 256 && mrows == m + 128 && (m == 1024 || m == 1280)) printf("COUNT %ld %ld %ld\n", m, K, launches);
}

int main() {
    const long sides[] = {256, 512, 768, 1024, 1280, 1408, 1536, 1920, 2048, 2368, 4096, 5184, 8192, 12352, 16384, 20480, 28736, 32768, 45056, 61440};
    const long mins[] = {256, 512, 1024, 2048, 4096, 8192, 16384};
    long cases = 0;
    for (long m : sides)
        for (long mn : mins)
            for (long extra : {0L, 128L})
                for (long K : {256L, 2048L}) {
                    if (K == 2048 && (mn < 1024 || m < 4096) && m != 1408) continue;  // the production panel width on the production sizes
                    if (K == 256 && m > 8192) continue;
                    check_case(m + extra, m, K, mn, 32);
                    ++cases;
                }
    check_case(1024 + 128, 1024, 48, 256, 32);  // K no multiple of 32: nothing splits
    ++cases;
    printf("cases %ld fails %ld\n", cases, g_fails);
    return g_fails ? 1 : 0;
}
