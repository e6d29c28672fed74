// poly_rules_check.cpp — the rules of the two-stage form's polyphase launch (python-soxr_amd/csrc/poly_rules.h) against slow
// independent statements, over random stages and jobs and over real stages (the {T2, Ls, Ms, up} of rate pairs the GPU tests
// and the fuzzer use, HQ and VHQ).  No device, no library.  Exit status 0 = every check held (tests/test_poly_rules.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "poly_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

typedef __int128 i128;
typedef unsigned __int128 u128;

struct Stage { int T2; long long Ls, Ms; int up; };
static const int kTaps[10] = {8, 12, 16, 20, 24, 28, 32, 40, 48, 56};
// real stages: dev.Plan(in, out, HQ | VHQ) of tests/test_gpu_two_stage.py's and tests/fuzz/fuzz_two_stage.py's rate pairs,
// three to five per (T2, direction): smallest, median and largest Ls, smallest and largest Ms / Ls
static const Stage kReal[] = {
    {12, 29401LL, 16000LL, 0}, {12, 99999LL, 50000LL, 0}, {12, 108658LL, 58411LL, 0}, {12, 50123320LL, 31121991LL, 0}, {12, 207470044LL, 108510523LL, 0},
    {16, 15123LL, 12434LL, 0}, {16, 99999LL, 50000LL, 0}, {16, 108658LL, 58411LL, 0}, {16, 60828718LL, 50476275LL, 0}, {16, 207470044LL, 108510523LL, 0},
    {20, 11501LL, 11783LL, 0}, {20, 36679LL, 39161LL, 0}, {20, 999999LL, 1000000LL, 0}, {20, 50123320LL, 31121991LL, 0}, {20, 102682190LL, 93307217LL, 0},
    {20, 10601LL, 8617LL, 1}, {20, 92231LL, 20988LL, 1}, {20, 1000001LL, 2000000LL, 1}, {20, 3117186LL, 1276739LL, 1}, {20, 804787693LL, 204633014LL, 1},
    {24, 10031LL, 12997LL, 0}, {24, 6172839LL, 8000000LL, 0}, {24, 23570602LL, 19171067LL, 0}, {24, 33558140LL, 43547327LL, 0}, {24, 102682190LL, 93307217LL, 0},
    {28, 7735LL, 11799LL, 0}, {28, 100001LL, 100000LL, 0}, {28, 58351076LL, 55565949LL, 0}, {28, 84647014LL, 126160645LL, 0},
    {28, 10601LL, 8617LL, 1}, {28, 92231LL, 20988LL, 1}, {28, 1000001LL, 2000000LL, 1}, {28, 3000003LL, 2000000LL, 1}, {28, 804787693LL, 204633014LL, 1},
    {32, 6955LL, 11329LL, 0}, {32, 16015LL, 18487LL, 0}, {32, 5440703LL, 6929797LL, 0}, {32, 15063627LL, 26013905LL, 0}, {32, 39315796LL, 62980189LL, 0},
    {40, 7735LL, 11799LL, 0}, {40, 16603LL, 21483LL, 0}, {40, 100001LL, 150000LL, 0}, {40, 1000001LL, 2000000LL, 0}, {40, 84647014LL, 126160645LL, 0},
    {48, 6955LL, 11329LL, 0}, {48, 8927LL, 14366LL, 0}, {48, 30938LL, 55659LL, 0}, {48, 17119997LL, 31870749LL, 0},
};
static const int kNReal = (int)(sizeof kReal / sizeof kReal[0]);

static double unit_rand(std::mt19937_64 &r) { return (double)(r() >> 11) * (1. / 9007199254740992.); }
// Ms / Ls over (0.125, 2.1], terms up to 2^31, small Ls included
static Stage random_stage(std::mt19937_64 &r)
{
    Stage s;
    s.T2 = kTaps[r() % 10];
    s.up = (int)(r() & 1);
    for (;;) {
        static const long long lims[4] = {64, 5000, 100000, 1LL << 31};
        const long long lim = lims[r() % 4];
        s.Ls = 1 + (long long)(r() % (unsigned long long)lim);
        s.Ms = (long long)std::llround((.125 + (2.1 - .125) * unit_rand(r)) * (double)s.Ls);
        if (s.Ms < 1 || s.Ms > (1LL << 31)) continue;
        const double ratio = (double)s.Ms / (double)s.Ls;
        if (ratio > .125 && ratio <= 2.1) return s;
    }
}
static Stage pick_stage(std::mt19937_64 &r, int trial) { return trial < kNReal ? kReal[trial] : random_stage(r); }
static int64_t floor_div(i128 q, i128 d) { i128 n = q / d; return (int64_t)(n * d > q ? n - 1 : n); } // d > 0

// strides {clip, frame, channel}: interleaved, planar, padded frames, strided channels
static void random_strides(std::mt19937_64 &r, uint32_t ch, int64_t frames, int64_t str[3])
{
    switch (r() % 4) {
    case 0: str[2] = 1; str[1] = ch; str[0] = frames * ch; break;
    case 1: str[2] = frames; str[1] = 1; str[0] = frames * ch; break;
    case 2: str[2] = 1; str[1] = ch + 1 + (int64_t)(r() % 3); str[0] = frames * str[1] + (int64_t)(r() % 2); break;
    default: str[2] = 1 + (int64_t)(r() % 3); str[1] = str[2] * ch + (int64_t)(r() % 2); str[0] = frames * str[1] + (int64_t)(r() % 5);
    }
}

// the kernels' own position of output k (k_poly's float32 path, k_poly2): k_lo's exact position plus (k - k_lo) steps of
// Ms / Ls as a 64.64 binary fraction with step_fx truncated and k_lo's fraction through fx_per_rem
struct KernelPos {
    int64_t nK0, Mq, k_lo;
    uint64_t phK0, step_fx;
    KernelPos(int64_t k_lo_, int64_t Ms, int64_t Ls) : Mq(Ms / Ls), k_lo(k_lo_), step_fx(poly_step_fx(Ms, Ls))
    {
        nK0 = floor_div((i128)k_lo * Ms, Ls);
        phK0 = (uint64_t)((double)(k_lo * Ms - nK0 * Ls) * poly_fx_per_rem(Ls));
    }
    int64_t operator()(int64_t k) const
    {
        const uint64_t dk = (uint64_t)(k - k_lo), lo = dk * step_fx, ph = phK0 + lo;
        return nK0 + (int64_t)dk * Mq + (int64_t)(uint64_t)(((u128)dk * step_fx) >> 64) + (ph < lo ? 1 : 0);
    }
};

// ---- span: every tile's source span within span_max, by the kernels' arithmetic and by exact positions ------------------
static void check_span(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < kNReal + 1500; ++trial) {
        const Stage s = pick_stage(rng, trial);
        const double ratio = (double)s.Ms / (double)s.Ls;
        const bool two = s.T2 <= 40 && s.Ms / s.Ls <= 1 && rng() % 2;
        const size_t width = two || rng() % 2 ? 4 : 8, tab = poly_tab_bytes(width == 4 ? 64 : 128, s.T2 + 1, width);
        const int Rmax = poly_rmax(width, tab, two, s.T2, ratio, 0), R = 1 + (int)(rng() % (unsigned)Rmax), H = s.T2 / 2;
        int64_t n_out;
        switch (rng() % 4) {
        case 0: n_out = 1 + (int64_t)(rng() % 3000); break;
        case 1: n_out = 256LL * R * (1 + (int64_t)(rng() % 40)) + (int64_t)(rng() % 3) - 1; break; // at a tile's edge
        case 2: n_out = 1 + (int64_t)(rng() % (1ull << 30)); break;
        default: n_out = 8192 + (int64_t)(rng() % 500000);
        }
        const int64_t k_lo = rng() % 2 ? 0 : -8 * (1 + (int64_t)(rng() % 40)), per_tile = 256LL * R, n_tiles = poly_tiles(n_out, R), k_end = k_lo + n_out;
        const int span_max = poly_span_max(R, ratio, s.T2);
        const KernelPos pos(k_lo, s.Ms, s.Ls);
        CHECK(n_tiles == (n_out + per_tile - 1) / per_tile && (n_tiles - 1) * per_tile < n_out, "tiles");
        if (two) CHECK(span_max <= 12 * 256, "k_poly2 holds a span of %d frames in 12 x 256 registers: T2=%d R=%d ratio=%g", span_max, s.T2, R, ratio);
        std::vector<int64_t> tiles; // every tile of a launch of up to 600, else the first, the last two and 300 others
        if (n_tiles <= 600) for (int64_t t = 0; t < n_tiles; ++t) tiles.push_back(t);
        else {
            tiles = {0, n_tiles - 2, n_tiles - 1};
            for (int q = 0; q < 300; ++q) tiles.push_back((int64_t)(rng() % (uint64_t)n_tiles));
        }
        for (const int64_t t : tiles) {
            const int64_t kA = k_lo + t * per_tile, kB = std::min(kA + per_tile, k_end) - 1; // (the last tile is cut by the job's end)
            const int64_t nA = pos(kA) - (H - 1), nB = pos(kB) + H;
            CHECK(nB - nA + 1 <= span_max && nB >= nA, "kernel span %lld > span_max %d: T2=%d Ls=%lld Ms=%lld R=%d k_lo=%lld tile %lld", (long long)(nB - nA + 1), span_max, s.T2, s.Ls,
                  s.Ms, R, (long long)k_lo, (long long)t);
            const int64_t eA = floor_div((i128)kA * s.Ms, s.Ls), eB = floor_div((i128)kB * s.Ms, s.Ls);
            CHECK(eB + H - (eA - (H - 1)) + 1 <= span_max, "exact span %lld > span_max %d: T2=%d Ls=%lld Ms=%lld R=%d tile %lld", (long long)(eB - eA + s.T2), span_max, s.T2, s.Ls, s.Ms,
                  R, (long long)t);
            // the 64.64 position is never more than one sample off the exact one
            for (int q = 0; q < 4; ++q) {
                const int64_t k = q == 0 ? kA : q == 1 ? kB : kA + (int64_t)(rng() % (uint64_t)(kB - kA + 1));
                const int64_t d = floor_div((i128)k * s.Ms, s.Ls) - pos(k);
                CHECK(d >= -1 && d <= 1, "position of output %lld is %lld off: Ls=%lld Ms=%lld k_lo=%lld", (long long)k, (long long)d, s.Ls, s.Ms, (long long)k_lo);
            }
        }
    }
}

// ---- LDS and the run length -----------------------------------------------------------------------------------------------
static void check_lds_and_run(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < kNReal + 40000; ++trial) {
        const Stage s = pick_stage(rng, trial);
        const size_t width = rng() % 2 ? 4 : 8;
        const PolyStage st = poly_stage(s.T2, width == 4 ? 64 : 128, s.T2 + 1, s.Ls, s.Ms);
        const bool two = width == 4 && s.T2 <= 40 && s.Ms / s.Ls <= 1 && rng() % 2;
        const size_t tab = poly_tab_bytes(st.P, st.row, width), unit = poly_unit(width, two);
        CHECK(tab == (size_t)st.P * st.row * (width == 4 ? 16 : 32) && unit == (two ? 8u : width), "table / unit bytes");
        const int Rfree = poly_rmax(width, tab, two, s.T2, st.ratio, 0);
        CHECK(Rfree >= 1 && Rfree <= 12, "Rmax %d", Rfree);
        // Rmax > 1 lies within the budget, and Rmax + 1 would not (or is above 12, or above k_poly2's registers)
        if (Rfree > 1) CHECK(poly_lds_bytes(tab, Rfree, st.ratio, s.T2, unit) <= poly_lds_cap(width, tab, two, s.T2), "Rmax %d leaves the budget", Rfree);
        if (Rfree > 1 && two) CHECK(poly_span(Rfree, st.ratio, s.T2) <= 12. * 256., "Rmax %d leaves k_poly2's registers", Rfree);
        if (Rfree < 12)
            CHECK(poly_lds_bytes(tab, Rfree + 1, st.ratio, s.T2, unit) > poly_lds_cap(width, tab, two, s.T2) || (two && poly_span(Rfree + 1, st.ratio, s.T2) > 12. * 256.), "Rmax %d is not the longest", Rfree);
        CHECK(poly_lds_cap(width, tab, two, s.T2) <= 96u * 1024u && poly_lds_cap(width, tab, two, s.T2) >= 52u * 1024u, "budget");
        for (int d = 1; d <= 13; ++d) CHECK(poly_rmax(width, tab, two, s.T2, st.ratio, d) == std::min(Rfree, d), "dbg_poly_r = %d does not clamp", d);
        CHECK(poly_rmax(width, tab, two, s.T2, st.ratio, -3) == Rfree, "a negative dbg_poly_r is no clamp");
        // the tile is one definition: span_max + 257 R elements
        for (int R = 1; R <= 12; ++R) {
            CHECK(poly_tile_elems(R, st.ratio, s.T2) == (size_t)poly_span_max(R, st.ratio, s.T2) + 257u * (size_t)R, "tile elements");
            CHECK(poly_lds_bytes(tab, R, st.ratio, s.T2, unit) == tab + poly_tile_elems(R, st.ratio, s.T2) * unit, "LDS bytes");
            CHECK((double)poly_span_max(R, st.ratio, s.T2) <= poly_span(R, st.ratio, s.T2) && poly_span(R, st.ratio, s.T2) < (double)poly_span_max(R, st.ratio, s.T2) + 1., "span_max truncates");
        }
        // the run length of a job: 1 <= R <= Rmax, with any cost function; whenever the job was admitted the tile fits LDS
        const int dbg = rng() % 3 ? 0 : (int)(rng() % 13), Rmax = poly_rmax(width, tab, two, s.T2, st.ratio, dbg);
        const int64_t n = rng() % 8 ? 8192 + (int64_t)(rng() % 3000000) : 1 + (int64_t)(rng() % (1ull << 30));
        const int64_t n_out = s.up ? (int64_t)(((i128)4 * n * s.Ls + s.Ms) / (2 * (i128)s.Ms)) : (int64_t)(((i128)n * s.Ls + s.Ms) / (2 * (i128)s.Ms));
        const uint64_t col_lim = rng() % 4 ? 16 : 70000, cols = 1 + rng() % col_lim;
        static const int cus[4] = {256, 304, 64, 8};
        const int n_cu = cus[rng() % 4], occ = poly_occ_limit(width, two, s.T2);
        CHECK(occ >= 2 && occ <= 4, "occupancy limit");
        if (cols > kPolyMaxCols) { CHECK(!two_stage_admits(n, n_out, cols, width, st), "more columns than gridDim.y holds"); continue; }
        const int64_t slots = poly_slots(Rmax, tab, st.ratio, s.T2, unit, occ, n_cu, cols);
        CHECK(slots >= 1 && slots <= std::max<int64_t>(1, (int64_t)occ * n_cu / (int64_t)cols), "slots %lld", (long long)slots);
        const TwoStageMid m = two_stage_mid(s.up, s.T2, s.Ls, s.Ms, n, n_out, 1, false);
        const int64_t poly_out = s.up ? n_out : m.n_mid; // outputs of the polyphase launch (a split column counts fewer: also tried)
        const bool admitted = two_stage_admits(n, n_out, cols, width, st);
        CHECK(admitted == (n >= 8192 && n_out >= 8192 && n < (1LL << 30) && n_out < (1LL << 30) &&
                           tab + (size_t)(512. * (st.ratio + 1.01) + s.T2 + 4) * width <= 150u * 1024u), "admission");
        for (int64_t no : {poly_out, (poly_out + 1) / 2, (int64_t)1}) {
            if (no < 1) continue;
            unsigned seed = (unsigned)rng();
            const int R = poly_pick_run(Rmax, no, slots, [&](int r) { seed = seed * 1664525u + 1013904223u + (unsigned)r; return 1. + (double)(seed >> 20) / 4096. * 2.; });
            CHECK(R >= 1 && R <= Rmax, "R = %d of Rmax = %d", R, Rmax);
            if (admitted)
                CHECK(poly_lds_bytes(tab, R, st.ratio, s.T2, unit) <= kPolyLdsMax, "admitted, but R=%d needs %zu bytes of LDS: width=%zu two=%d T2=%d Ls=%lld Ms=%lld", R,
                      poly_lds_bytes(tab, R, st.ratio, s.T2, unit), width, (int)two, s.T2, s.Ls, s.Ms);
            // less than one round of tiles: the shortest run that still gives no more tiles than slots, at least min(Rmax, 2)
            if (poly_tiles(no, Rmax) < slots) CHECK(R >= std::min(Rmax, 2) && (R == std::min(Rmax, 2) || poly_tiles(no, R) <= slots), "short job: R=%d", R);
            else CHECK(R >= std::min(Rmax, std::max(2, Rmax / 3)), "long job: R=%d below the floor of Rmax=%d", R, Rmax);
        }
        // a cost of 1 (no conflicts) at Rmax ends the search there
        CHECK(poly_pick_run(Rmax, (int64_t)1 << 29, 1, [](int) { return 1.; }) == Rmax, "conflict-free Rmax is taken");
    }
}

// ---- the lane multiplier -----------------------------------------------------------------------------------------------------
// cycles of the 16 read groups of a workgroup over 16 starting phases: per group, the largest number of DISTINCT records on
// one bank quad — recounted plainly (sort and count) for one multiplier
static double recount(int P, int row, int halves, int r, double ratio, int am)
{
    double total = 0.;
    for (int ph = 0; ph < 16; ++ph)
        for (int wave = 0; wave < 4; ++wave)
            for (int g = 0; g < 4; ++g) {
                int on_quad[16][16], n_on[16] = {0};
                for (int q = 0; q < 16; ++q) {
                    const int tid = 64 * wave + kPolyLaneGroup[g][q], slot = (tid * am) & 255;
                    const double f = ph / 16. + .37 + (double)slot * r * ratio;
                    const int i = (int)((f - std::floor(f)) * P) % P;
                    const int quad = (halves * row * i) & 15;
                    on_quad[quad][n_on[quad]++] = i;
                }
                size_t worst = 1;
                for (int quad = 0; quad < 16; ++quad) {
                    std::sort(on_quad[quad], on_quad[quad] + n_on[quad]);
                    worst = std::max<size_t>(worst, (size_t)(std::unique(on_quad[quad], on_quad[quad] + n_on[quad]) - on_quad[quad]));
                }
                total += (double)worst;
            }
    return total;
}
static void check_lanes(std::mt19937_64 &rng)
{
    { // the lane groups partition a wave
        int seen[64] = {0};
        for (auto &g : kPolyLaneGroup) for (int l : g) ++seen[l];
        bool once = true;
        for (int v : seen) once = once && v == 1;
        CHECK(once, "lane groups");
    }
    for (int trial = 0; trial < 36; ++trial) {
        const Stage s = trial < 18 ? kReal[(trial * 7) % kNReal] : random_stage(rng);
        const int halves = 1 + (int)(rng() % 2), P = halves == 2 ? 128 : 64, row = s.T2 + 1, r = 1 + (int)(rng() % 12);
        const double ratio = (double)s.Ms / (double)s.Ls;
        const PolyLane ln = poly_lane_cost(P, row, halves, r, ratio);
        CHECK(ln.lane_mul % 2 == 1 && ln.lane_mul >= 1 && ln.lane_mul <= 255, "lane_mul %d", ln.lane_mul);
        int hit[256] = {0};
        for (int tid = 0; tid < 256; ++tid) ++hit[(tid * ln.lane_mul) & 255];
        bool bij = true;
        for (int v : hit) bij = bij && v == 1;
        CHECK(bij, "slot = tid * %d mod 256 is no bijection", ln.lane_mul);
        const double mine = recount(P, row, halves, r, ratio, ln.lane_mul);
        // (256 read groups of at least one cycle each, normalised by 256 x halves: a float64 table's cost starts at 1 / 2)
        CHECK(ln.conf == (float)(mine / (256. * halves)) && ln.conf * halves >= 1.f, "conf %g, recounted %g: T2=%d Ls=%lld Ms=%lld r=%d", (double)ln.conf, mine / (256. * halves), s.T2, s.Ls, s.Ms, r);
        for (int am = 1; am < ln.lane_mul; am += 2)
            CHECK(recount(P, row, halves, r, ratio, am) >= mine, "multiplier %d is cheaper than %d: T2=%d Ls=%lld Ms=%lld r=%d", am, ln.lane_mul, s.T2, s.Ls, s.Ms, r);
        if (ln.lane_mul < 255 && mine > 256. * halves) // not conflict-free: the search went through every multiplier
            for (int am = ln.lane_mul + 2; am < 256; am += 2 + 2 * (int)(rng() % 6))
                CHECK(recount(P, row, halves, r, ratio, am) >= mine, "multiplier %d beats %d", am, ln.lane_mul);
    }
}

// ---- the form: pairs, split columns, column groups ---------------------------------------------------------------------------
static void check_form(std::mt19937_64 &rng)
{
    long n_pair = 0, n_split = 0;
    for (int trial = 0; trial < kNReal + 60000; ++trial) {
        const Stage s = pick_stage(rng, trial);
        const size_t width = rng() % 4 ? 4 : 8;
        static const uint32_t usual[6] = {1, 2, 3, 4, 6, 8};
        const uint32_t ch = rng() % 4 == 0 ? 1 + (uint32_t)(rng() % 64) : usual[rng() % 6];
        const uint32_t clips = rng() % 4 ? 1 + (uint32_t)(rng() % 4) : 1 + (uint32_t)(rng() % 65535);
        int64_t n_out;
        switch (rng() % 4) {
        case 0: n_out = 1 + (int64_t)(rng() % 20000); break;
        case 1: n_out = std::max<int64_t>(1, std::min<int64_t>((1LL << 30), s.Ls * (int64_t)(1 + rng() % 9) + (int64_t)(rng() % 5) - 2)); break; // at period edges
        case 2: n_out = 1 + (int64_t)(rng() % (1ull << 30)); break;
        default: n_out = 8192 + (int64_t)(rng() % 2000000);
        }
        int64_t ss[3], ds[3];
        random_strides(rng, ch, n_out * 3, ss);
        random_strides(rng, ch, n_out, ds);
        if (rng() % 3 == 0) { ss[2] = ds[2] = 1; ss[1] = ds[1] = ch; ss[0] = 3 * n_out * ch; ds[0] = n_out * ch; } // both ends interleaved
        const uintptr_t bits = rng() % 3 ? 0 : 4 * (uintptr_t)(rng() % 4);
        const bool no_pair = rng() % 8 == 0;
        const int64_t Mq = s.Ms / s.Ls;
        const PolyForm f = poly_form(width, Mq, ch, ss, ds, bits, s.T2, no_pair, n_out, s.Ls, s.Ms);
        CHECK(!(f.pair && f.split), "a split column is never a pair");
        if (f.pair || f.split) CHECK(width == 4 && !no_pair && (Mq == 0 || Mq == 1) && s.T2 <= 40, "k_poly2 outside its instances: width=%zu Mq=%lld T2=%d", width, (long long)Mq, s.T2);
        if (f.pair) {
            ++n_pair;
            CHECK(ss[2] == 1 && ds[2] == 1 && ss[0] % 2 == 0 && ss[1] % 2 == 0 && ds[0] % 2 == 0 && ds[1] % 2 == 0 && bits % 8 == 0 && ch % 2 == 0, "pair on ch=%u strides %lld %lld %lld / %lld %lld %lld bits=%u", ch,
                  (long long)ss[0], (long long)ss[1], (long long)ss[2], (long long)ds[0], (long long)ds[1], (long long)ds[2], (unsigned)bits);
        }
        if (f.split) {
            ++n_split;
            CHECK(f.n1 + f.n2 == n_out && f.n1 % s.Ls == 0 && f.n1 >= s.Ls && f.n1 >= f.n2 && f.n2 >= 0 && 10 * f.n2 >= 7 * f.n1, "split %lld + %lld of %lld, Ls=%lld", (long long)f.n1, (long long)f.n2,
                  (long long)n_out, s.Ls);
            CHECK((i128)f.m2_shift * s.Ls == (i128)f.n1 * s.Ms && f.m2_shift < (1LL << 40), "segments are %lld samples apart: no whole number of periods (n1=%lld Ls=%lld Ms=%lld)", (long long)f.m2_shift,
                  (long long)f.n1, s.Ls, s.Ms);
            CHECK(f.m2_src == f.m2_shift * ss[1] && f.m2_dst == f.n1 * ds[1], "member 2's element offsets");
            for (int q = 0; q < 3; ++q) { // output k + n1 has output k's fraction, m2_shift samples on
                const int64_t k = q == 0 ? 0 : q == 1 ? f.n2 - 1 : (int64_t)(rng() % (uint64_t)std::max<int64_t>(1, f.n2));
                const i128 a = (i128)k * s.Ms, b = (i128)(k + f.n1) * s.Ms;
                CHECK(floor_div(b, s.Ls) - floor_div(a, s.Ls) == f.m2_shift && b - (i128)floor_div(b, s.Ls) * s.Ls == a - (i128)floor_div(a, s.Ls) * s.Ls, "fraction of output k + n1");
            }
        } else
            CHECK(f.n1 == n_out && f.n2 == n_out && f.m2_shift == 0 && f.m2_src == 0 && f.m2_dst == 0, "an unsplit column has one member");
        // a column not split though k_poly2 could take it: shorter than ~1.7 periods, or the shift too long
        if (!f.pair && !f.split && width == 4 && !no_pair && (Mq == 0 || Mq == 1) && s.T2 <= 40) {
            const int64_t h = (n_out + 2 * s.Ls - 1) / (2 * s.Ls), n1 = h * s.Ls;
            CHECK(10 * (n_out - n1) < 7 * n1 || (i128)h * s.Ms >= ((i128)1 << 40), "a column of %lld outputs (Ls=%lld) was not split", (long long)n_out, s.Ls);
        }
        // columns: the group (2^lg_cg channels, pairs: channel pairs) divides the channel count, so a group never straddles a clip
        const int64_t group = (int64_t)(f.pair ? 2 : 1) << f.lg_cg;
        CHECK(f.lg_cg >= 0 && f.lg_cg <= 2 && ch % group == 0, "a group of %lld channels does not divide %u", (long long)group, ch);
        CHECK(((uint64_t)clips * ch) % (uint64_t)group == 0 && poly_cols(clips, ch, f.pair, f.lg_cg) * (uint64_t)group == (uint64_t)clips * ch, "columns are no exact quotient");
        if (f.lg_cg > 0 && !f.pair) CHECK(ss[2] == 1 || ds[2] == 1, "channel groups on planar data");
    }
    CHECK(n_pair > 1000 && n_split > 1000, "the cases were reached: %ld pairs, %ld splits", n_pair, n_split);
}

// ---- the grid --------------------------------------------------------------------------------------------------------------
static void check_grid(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 200000; ++trial) {
        const int64_t n_tiles = rng() % 3 ? 1 + (int64_t)(rng() % 40) : 1 + (int64_t)(rng() % 5000000);
        static const int cus[5] = {256, 304, 64, 8, 1};
        const int per_cu = (int)(rng() % 5), n_cu = cus[rng() % 5];
        const uint64_t cols = rng() % 2 ? 1 + rng() % 8 : 1 + rng() % 65535;
        const unsigned gx = poly_grid_x(n_tiles, per_cu, n_cu, cols);
        const int64_t held = std::max<int64_t>(1, (int64_t)std::max(per_cu, 1) * n_cu / (int64_t)cols); // workgroups per column the chip holds at once
        CHECK(gx >= 1 && (int64_t)gx <= n_tiles && (int64_t)gx <= held, "gx=%u tiles=%lld held=%lld", gx, (long long)n_tiles, (long long)held);
        CHECK(gx <= 8 || gx % 8 == 0, "gx=%u above 8 is no multiple of 8", gx);
        // as many as the chip holds and the job has — above 8, the multiple of 8 below that
        const int64_t most = std::min(n_tiles, held);
        CHECK((int64_t)gx == (most > 8 ? most / 8 * 8 : most), "gx=%u of %lld", gx, (long long)most);
        if (held >= n_tiles && (n_tiles <= 8 || n_tiles % 8 == 0)) CHECK((int64_t)gx == n_tiles, "the chip holds every tile, but gx=%u of %lld", gx, (long long)n_tiles);
    }
}

// ---- the intermediate signal ---------------------------------------------------------------------------------------------------
static void check_mid(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < kNReal + 40000; ++trial) {
        const Stage s = pick_stage(rng, trial);
        const int64_t n = rng() % 4 ? 8192 + (int64_t)(rng() % 2000000) : 1 + (int64_t)(rng() % (1ull << 30));
        // the plan's output count of n inputs, round(n L / M), in the stage's terms: L / M = 2 Ls / Ms (up), Ls / (2 Ms) (down)
        const int64_t n_out = s.up ? (int64_t)(((i128)4 * n * s.Ls + s.Ms) / (2 * (i128)s.Ms)) : (int64_t)(((i128)n * s.Ls + s.Ms) / (2 * (i128)s.Ms));
        const uint32_t ch = 1 + (uint32_t)(rng() % 8);
        const bool inter = rng() % 2;
        const TwoStageMid m = two_stage_mid(s.up != 0, s.T2, s.Ls, s.Ms, n, n_out, ch, inter);
        const int H = s.T2 / 2;
        // half-width of the polyphase filter in intermediate samples: up H (it reads the intermediate), down ceil(H Ls / Ms)
        const int64_t half = s.up ? H : (int64_t)(((i128)H * s.Ls + s.Ms - 1) / s.Ms);
        CHECK(m.pad % 8 == 0 && m.pad >= half + 4 && m.pad < half + 4 + 8, "pad %lld for a half-width of %lld", (long long)m.pad, (long long)half);
        CHECK(m.n_core == (s.up ? 2 * n : 2 * n_out) && m.n_mid == m.n_core + 2 * m.pad, "core / whole length");
        if (inter) CHECK(m.mstr[0] == m.n_mid * ch && m.mstr[1] == ch && m.mstr[2] == 1, "[clip][frames][channel]");
        else CHECK(m.mstr[0] == m.n_mid * ch && m.mstr[1] == 1 && m.mstr[2] == m.n_mid, "[clip][channel][frames]");
        if (s.up && n_out >= 1) { // every source index the polyphase stage reads for outputs [0, n_out) lies in [-pad, n_core + pad)
            const int64_t first = floor_div(0, s.Ls) - (H - 1), last = floor_div((i128)(n_out - 1) * s.Ms, s.Ls) + H;
            CHECK(first >= -m.pad && last < m.n_core + m.pad, "up: reads [%lld, %lld] of [%lld, %lld)", (long long)first, (long long)last, (long long)-m.pad, (long long)(m.n_core + m.pad));
            const KernelPos pos(0, s.Ms, s.Ls);
            CHECK(pos(n_out - 1) + H < m.n_core + m.pad && pos(0) == 0, "up: the kernel's own last position");
        }
    }
}

int main()
{
    std::mt19937_64 rng(20261019);
    check_span(rng);
    check_lds_and_run(rng);
    check_lanes(rng);
    check_form(rng);
    check_grid(rng);
    check_mid(rng);
    std::printf("poly_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
