// Stand-alone check of the U1 plan of csrc/bulk_plan.hpp (u1_plan_build / u1_block_rows; host only; built and run by tests/test_u1_plan_cpu.py with the host
// compiler and -fsanitize=address,undefined).  U1 is C(mrows × nb1; the nb1×nb1 square lower) −= P·P[0:nb1]ᵀ with mrows = nb1 + the rectangle's rows + the
// carried rows.  For every case of a grid it builds the plan and checks, independently of the builder's own bookkeeping:
//   disjoint   within each of the four lists all target rectangles are pairwise disjoint
//   order      every quadrant of the Strassen block receives its products in the fixed order (M1, M2|M5, M3|M4, M6|M7)
//   coverage   every 64×64 cell of the trapezoid and of the carried rows is updated over exactly the k range K, every other cell not at all; the block counts
//              only after its seven products, decoded from their operand and target OFFSETS and expanded on 2×2 blocks, sum to A·Bᵀ
//   workspace  the block's slice lies inside the reported size; every panel a product reads lies in it and is written by a sums job
//   tiles      first-tile prefix sums, tile counts and the grid size agree; entries are ordered by decreasing K
//   shape      one block — the whole 256-row quadrants of the rectangle, all nb1 columns — one lower piece — the square alone — at most one remainder strip
//              and one piece of carried rows, seven products in lists of 1, 2, 2, 2; the gate u1_block_rows is 0 exactly below the two floors and off the shape
// Output: one "FAIL <check> <case>: <what>" line per violation and a last line "cases <n> planned <n> fails <n>".
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

// coefficients over (X11, X12, X21, X22) of the five panels strassen_sums_kernel writes (kernels.hpp), per side
static const int SUMS[2][5][4] = {{{1, 0, 0, 1}, {0, 0, 1, 1}, {1, 1, 0, 0}, {-1, 0, 1, 0}, {0, 1, 0, -1}},
                                  {{1, 0, 0, 1}, {0, 0, 1, -1}, {-1, 1, 0, 0}, {1, 0, 1, 0}, {0, 1, 0, 1}}};

// returns whether the case was planned (the gate let it through)
static bool check_case(long nb1, long mrect, long carried, long K, long floor_rows, long ldpad, long floor_k = 256) {
    const long mrows = nb1 + mrect + carried, row0 = 384, ldc = nb1 + mrect + 40, ldp = K + 32;
    g_case = "nb1=" + S(nb1) + " rect=" + S(mrect) + " carried=" + S(carried) + " K=" + S(K) + " floor=" + S(floor_rows);
    const long bs = mrect / 256 * 256;
    const bool want_form = floor_rows > 0 && bs >= floor_rows && K >= floor_k && bs >= 256 && nb1 >= 256 && nb1 % 256 == 0 && K % 32 == 0;
    const long got = u1_block_rows(floor_rows, floor_k, mrect, nb1, K);
    if (got != (want_form ? bs : 0)) fail("shape", "u1_block_rows gives " + S(got));
    if (!want_form) return false;
    const BulkPlan p = u1_plan_build(mrows, mrect, nb1, K, row0, ldc, ldp, ldpad);
    const long R = mrows / 64, Cn = nb1 / 64;
    std::vector<long> cover((size_t)R * (size_t)Cn, 0);
    auto paint = [&](long r0, long c0, long M, long N, long k, bool lower) {
        if (r0 < 0 || c0 < 0 || r0 + M > mrows || c0 + N > nb1 || r0 % 64 || c0 % 64 || M % 64 || N % 64) return fail("coverage", "target outside the update or off the 64 grid");
        for (long r = r0 / 64; r < (r0 + M) / 64; ++r)
            for (long c = c0 / 64; c < (c0 + N) / 64; ++c)
                if (!lower || c <= r) cover[(size_t)r * Cn + c] += k;
    };

    // ---- shape of the plan: one block, and it is the rectangle's whole quadrants ----
    if (p.blocks.size() != 1) {
        fail("shape", S((long)p.blocks.size()) + " blocks");
        return true;
    }
    const PlanBlock& b = p.blocks[0];
    if (b.c_off != nb1 * ldc || b.a_off != nb1 * ldp || b.b_off != 0 || b.M != bs || b.N != nb1 || b.K != K) fail("shape", "the block is not rows [nb1, nb1 + bs) × all columns");
    if (p.list[0].empty() || p.list[1].empty() || p.list[2].empty() || p.list[3].empty()) fail("shape", "an empty list");

    // ---- workspace ----
    const long mh = b.M / 2, nh = b.N / 2, kh = b.K / 2, pa = mh * p.lds, pb = nh * p.lds;
    if (b.s_off < 0 || (size_t)(b.s_off + b.s_elems) > p.ws_elems) fail("workspace", "slice outside the reported size");
    if (p.lds < kh || b.s_elems != 5 * (pa + pb)) fail("workspace", "slice size");
    if (p.ws_elems != strassen_ws_rule(ldpad, b.M, b.N, b.K)) fail("workspace", "size is not the rule's for this block");
    int seen[2] = {0, 0};
    for (const PlanSums& s : p.sums) {
        if (s.side == 0 && s.s_off == b.s_off && s.x_off == b.a_off && s.rh == mh && s.kh == kh && s.pstride == pa) ++seen[0];
        if (s.side == 1 && s.s_off == b.s_off + 5 * pa && s.x_off == b.b_off && s.rh == nh && s.kh == kh && s.pstride == pb) ++seen[1];
    }
    if (seen[0] != 1 || seen[1] != 1 || p.sums.size() != 2) fail("workspace", "not one sums job per side");

    // ---- per list: tiles, disjoint targets; the block's order and symbolic expansion ----
    struct Hit {
        int launch, product;
    };
    std::vector<Hit> hits[4];                                            // per quadrant
    std::vector<std::vector<long>> coef(4, std::vector<long>(16, 0));  // per quadrant: coefficient of (A quadrant, B quadrant)
    int nprod = 0, nprod_l[4] = {0, 0, 0, 0}, nlower = 0, nstrip = 0, ncarried = 0;
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
                if (e.lower) {
                    ++nlower;
                    if (r0 != 0 || c0 != 0 || e.roff != 0 || e.M != nb1 || e.N != nb1) fail("shape", "the lower piece is not the square");
                } else if (r0 == nb1 + bs && e.M == mrect - bs && e.N == nb1 && c0 == 0) ++nstrip;
                else if (r0 == nb1 + mrect && e.M == carried && e.N == nb1 && c0 == 0) ++ncarried;
                else fail("shape", "a classical piece that is neither the square, the strip nor the carried rows");
                paint(r0, c0, e.M, e.N, e.K, e.lower != 0);
                continue;
            }
            ++nprod;
            ++nprod_l[l];
            if (e.block != 0 || e.M != mh || e.N != nh || e.K != kh || !e.beta0 || e.lower || (e.s1 != 1 && e.s1 != -1)) fail("coverage", "product shape");
            // operands, decoded from their offsets
            long ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
            if (e.a_src) {
                const long rel = e.a_off - b.s_off;
                if (rel < 0 || rel % pa || rel / pa > 4) fail("workspace", "A panel of a product outside the slice");
                else for (int q = 0; q < 4; ++q) ca[q] = SUMS[0][rel / pa][q];
            } else {
                const long rel = e.a_off - b.a_off, qi = rel / (mh * ldp), qk = rel - qi * mh * ldp;
                if (rel < 0 || qi > 1 || (qk != 0 && qk != kh)) fail("coverage", "A operand is no quadrant");
                else ca[qi * 2 + (qk ? 1 : 0)] = 1;
            }
            if (e.b_src) {
                const long rel = e.b_off - (b.s_off + 5 * pa);
                if (rel < 0 || rel % pb || rel / pb > 4) fail("workspace", "B panel of a product outside the slice");
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
                const int q = (tr ? 2 : 0) + (tc ? 1 : 0);
                hits[q].push_back(Hit{l, e.product});
                for (int x = 0; x < 4; ++x)
                    for (int y = 0; y < 4; ++y) coef[(size_t)q][(size_t)(x * 4 + y)] += sgn * ca[x] * cb[y];
                if (tg) rects.push_back(Rect{br0 + tr, br0 + tr + mh, bc0 + tc, bc0 + tc + nh, (int)i});
            }
        }
        if (t != p.ntiles[l]) fail("tiles", "launch " + S(l) + ": grid size " + S(p.ntiles[l]) + " against " + S(t) + " tiles");
        for (size_t a = 0; a < rects.size(); ++a)
            for (size_t c = 0; c < a; ++c)
                if (meet(rects[a], rects[c])) fail("disjoint", "launch " + S(l) + ": targets of entries " + S(rects[c].idx) + " and " + S(rects[a].idx) + " meet");
    }
    if (nlower != 1 || nstrip != (mrect > bs ? 1 : 0) || ncarried != (carried ? 1 : 0)) fail("shape", "classical pieces: " + S(nlower) + " lower, " + S(nstrip) + " strip, " + S(ncarried) + " carried");
    if (nprod_l[0] != 1 || nprod_l[1] != 2 || nprod_l[2] != 2 || nprod_l[3] != 2) fail("shape", "products per list are not 1, 2, 2, 2");
    static const int ORDER[4][4][2] = {{{0, 1}, {1, 5}, {2, 4}, {3, 7}}, {{1, 5}, {2, 3}, {-1, 0}, {-1, 0}}, {{1, 2}, {2, 4}, {-1, 0}, {-1, 0}}, {{0, 1}, {1, 2}, {2, 3}, {3, 6}}};
    bool ok = nprod == 7;
    if (!ok) fail("coverage", "the block has " + S(nprod) + " products");
    for (int q = 0; q < 4; ++q) {
        const auto& h = hits[q];
        const size_t want = (q == 0 || q == 3) ? 4 : 2;
        bool good = h.size() == want;
        for (size_t i = 0; good && i < want; ++i) good = h[i].launch == ORDER[q][i][0] && h[i].product == ORDER[q][i][1];
        if (!good) fail("order", "quadrant " + S(q));
        // C_ij −= A_i1 B_j1ᵀ + A_i2 B_j2ᵀ: coefficient 1 on (A_ik, B_jk), 0 elsewhere
        const int i = q >> 1, j = q & 1;
        for (int x = 0; x < 4; ++x)
            for (int y = 0; y < 4; ++y) {
                const long want_c = ((x >> 1) == i && (y >> 1) == j && (x & 1) == (y & 1)) ? 1 : 0;
                if (coef[(size_t)q][(size_t)(x * 4 + y)] != want_c) ok = false;
            }
    }
    if (!ok) fail("coverage", "the products do not sum to A·Bᵀ");
    else paint(b.c_off / ldc, b.c_off % ldc, b.M, b.N, 2 * (b.K / 2), false);
    long bad = 0;
    for (long r = 0; r < R; ++r)
        for (long c = 0; c < Cn; ++c) {
            const long want = (r >= Cn || c <= r) ? K : 0;
            if (cover[(size_t)r * Cn + c] != want) ++bad;
        }
    if (bad) fail("coverage", S(bad) + " cells of 64×64 are not updated over exactly K");
    return true;
}

int main() {
    const long widths[] = {256, 512, 1024, 4096};
    const long depths[] = {256, 512, 4096};
    const long heights[] = {256, 384, 512, 640, 1024, 1152, 1280, 1408, 1536, 4096, 8192, 12416, 16384, 28800, 30720, 45056, 57344, 61312, 61440};
    long cases = 0, planned = 0;
    for (long nb1 : widths)
        for (long K : depths)
            for (long h : heights)
                for (long carried : {0L, 128L})
                    for (long fl : {256L, 8192L}) {
                        if (fl == 8192 && (carried || h < 4096)) continue;  // the floor: on the heights around it, once
                        planned += check_case(nb1, h, carried, K, fl, 32) ? 1 : 0;
                        ++cases;
                    }
    planned += check_case(512, 1024, 128, 512, 0, 32) ? 1 : 0;    // floor 0: never
    planned += check_case(512, 1024, 128, 48, 256, 32) ? 1 : 0;   // K no multiple of 32
    planned += check_case(384, 1024, 128, 512, 256, 32) ? 1 : 0;  // a panel of no whole quadrants
    planned += check_case(512, 128, 0, 512, 256, 32) ? 1 : 0;     // a rectangle below one quadrant row
    planned += check_case(4096, 16384, 128, 512, 256, 32, 4096) ? 1 : 0;   // a panel below the floor on K ...
    planned += check_case(4096, 16384, 128, 4096, 256, 32, 4096) ? 1 : 0;  // ... and one on it
    cases += 6;
    printf("cases %ld planned %ld fails %ld\n", cases, planned, g_fails);
    return g_fails ? 1 : 0;
}
