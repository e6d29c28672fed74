// adjoint_auto_rules_check.cpp — the rules of HIPSOXR_KERNEL_ADJOINT_AUTO (python-soxr_amd/csrc/adjoint_auto_rules.h) against
// slow independent statements: the decision table over plan kind x recipe x total outputs 8191 / 8192 x switches x form x
// admits; the refusals over both entries; and, over seeded random ADJOINT clip tables — n_y == 0, n_x == 0, truncated
// cotangents, 8191 / 8192 frames either side, 1-3 channels, both widths, both directions — the partition, the compacted short
// sub-table, and for every two-stage column the poly row and the transposed plan's FFT row against what two_stage_adj_run
// (twostage.hip) sets for that clip ALONE: the same pad, n_core, n_mid and in_abs0, offsets inside the range's intermediate,
// no two columns overlapping; ranges within the budget and 65535 columns.  No device, no library.  Exit status 0 = every
// check held (tests/test_adjoint_auto_rules.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "adjoint_auto_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

// ---- the decision table ---------------------------------------------------------------------------------------------------
static void check_decisions()
{
    long n = 0, fft = 0, two = 0;
    for (int phases = 0; phases < 2; ++phases)
        for (int below = 0; below < 2; ++below)
            for (int64_t total : {(int64_t)0, (int64_t)8191, (int64_t)8192, (int64_t)1 << 40})
                for (int no_fft = 0; no_fft < 2; ++no_fft)
                    for (int no_two = 0; no_two < 2; ++no_two)
                        for (int form = 0; form < 2; ++form)
                            for (int admits = 0; admits < 2; ++admits)
                                for (int entry = 0; entry < 2; ++entry) { // (the rule does not read the entry: the same answer on both)
                                    const AdjAutoJob q = {phases != 0, below != 0, total, no_fft != 0, no_two != 0, form != 0, admits != 0};
                                    // the slow statement: AUTO's forward, read off job_rules.h's comments
                                    AdjAutoEngine want = kAdjAutoExact;
                                    if (!phases) {
                                        if (total >= 8192 && !no_fft && !below) want = kAdjAutoFft;
                                    } else if (!no_fft && !no_two && form && admits) want = kAdjAutoTwoStage;
                                    const AdjAutoEngine got = adj_auto_engine(q);
                                    CHECK(got == want, "phases %d below %d total %lld no_fft %d no_two %d form %d admits %d entry %d: engine %d, want %d", phases, below,
                                          (long long)total, no_fft, no_two, form, admits, entry, (int)got, (int)want);
                                    ++n; fft += got == kAdjAutoFft; two += got == kAdjAutoTwoStage;
                                }
    CHECK(fft > 0 && two > 0 && n - fft - two > 0, "the table did not reach every engine");
    // the totals: frames over clips (or rows) and channels
    CHECK(adj_auto_total_equal(4096, 1, 2) == 8192 && adj_auto_total_equal(8191, 1, 1) == 8191 && adj_auto_total_equal(100, 0, 2) == 0, "equal-length total");
    const int64_t rows[12] = {0, 4000, 0, 4400, 9, 0, 9, 50, 7, 4191, 7, 4600};
    CHECK(adj_auto_total_table(rows, 3, 1) == 8191 && adj_auto_total_table(rows, 3, 2) == 16382 && adj_auto_total_table(rows, 0, 2) == 0, "table total");
    std::printf("decision table: %ld cases, %ld on the frequency-domain engine, %ld on the two-stage form\n", n, fft, two);
}

// ---- the refusals -----------------------------------------------------------------------------------------------------------
static void check_refusals()
{
    long refused = 0, served = 0;
    for (int ragged = 0; ragged < 2; ++ragged)
        for (int bits = 0; bits < 32; ++bits) {
            const AdjAutoAsk q = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0};
            if (q.half && q.real) continue; // (one element type)
            const char *e = adj_auto_refusal(ragged != 0, q);
            const bool want = (ragged && q.half) || !q.real || q.vr || q.window || (ragged ? !q.table : q.table);
            CHECK((e != nullptr) == want, "ragged %d bits %d: %s", ragged, bits, e ? e : "served");
            if (e) CHECK(std::strncmp(e, "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO", 40) == 0, "the text names the selector: %s", e);
            refused += e != nullptr; served += e == nullptr;
        }
    CHECK(served == 2, "one served combination per entry, got %ld", served);
    CHECK(std::strncmp(kAdjAutoForwardRefusal, "HIPSOXR_KERNEL_ADJOINT_AUTO", 27) == 0, "forward refusal names the selector");
    std::printf("refusals: %ld refused, %ld served\n", refused, served);
}

// ---- tables -----------------------------------------------------------------------------------------------------------------
struct Stage { int T2; long long Ls, Ms; int up; };
// real stages (tests/c/ragged_poly_rules_check.cpp kReal), both directions
static const Stage kReal[] = {
    {12, 29401LL, 16000LL, 0}, {16, 15123LL, 12434LL, 0}, {20, 999999LL, 1000000LL, 0}, {24, 10031LL, 12997LL, 0}, {28, 100001LL, 100000LL, 0},
    {32, 16015LL, 18487LL, 0}, {40, 100001LL, 150000LL, 0}, {48, 30938LL, 55659LL, 0}, {20, 10601LL, 8617LL, 1}, {20, 1000001LL, 2000000LL, 1},
    {28, 92231LL, 20988LL, 1}, {28, 3000003LL, 2000000LL, 1}, {28, 804787693LL, 204633014LL, 1}, {56, 100001LL, 150000LL, 0},
};
static const int kNReal = (int)(sizeof kReal / sizeof kReal[0]);

// the admission of a clip ALONE, restated: the forward's (8192 frames or more either side, fewer than 2^30, channels within one
// launch, table + a tile's span within 150 KiB) and an adjoint tile that fits 160 KiB at some run length
static bool admits_alone(int64_t n_x, int64_t n_y, uint32_t ch, size_t width, const Stage &st, int P)
{
    if (n_x < 8192 || n_y < 8192 || n_x >= 1073741824LL || n_y >= 1073741824LL || ch > 65535) return false;
    const double ratio = (double)st.Ms / (double)st.Ls;
    const size_t tab = (size_t)P * (size_t)(st.T2 + 1) * 4 * width;
    if (tab + (size_t)(512. * (ratio + 1.01) + st.T2 + 4) * width > 150u * 1024u) return false;
    for (int R = 4; R >= 1; R /= 2) {
        const size_t span = (size_t)(((int)((double)(256 * R + st.T2) / ratio) + 5) & ~1);
        if (tab + span * (2 * width + 8) + (size_t)256 * R * width <= 160u * 1024u) return true;
    }
    return false;
}

struct Table { std::vector<int64_t> rows; uint32_t n_clips, ch; int64_t gy_chs, gx_chs; };
static int64_t pick_frames(std::mt19937_64 &r)
{
    switch (r() % 9) {
    case 0: return 0;
    case 1: return 1 + (int64_t)(r() % 300);
    case 2: return 8191;
    case 3: return 8192;
    case 4: return 8193;
    case 5: return 4000;
    default: return 8192 + (int64_t)(r() % 300000);
    }
}
// adjoint rows {gy offset, n_y, gx offset, n_x}, n_y <= about the plan's output length for n_x; planar channels a buffer apart
static Table random_table(std::mt19937_64 &r, const Stage &st, uint32_t n_clips)
{
    Table t;
    t.n_clips = n_clips; t.ch = 1 + (uint32_t)(r() % 3);
    const double out_per_in = st.up ? 2. * (double)st.Ls / (double)st.Ms : .5 * (double)st.Ls / (double)st.Ms;
    std::vector<int64_t> nx(n_clips), ny(n_clips);
    int64_t sx = 0, sy = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        if (r() % 2) { // the cotangent's count drawn (8191 / 8192 on the gy side), the input count the least that reaches it
            ny[c] = pick_frames(r);
            nx[c] = (int64_t)std::ceil((double)ny[c] / out_per_in) + (int64_t)(r() % 2);
        } else {
            nx[c] = pick_frames(r);
            ny[c] = std::max<int64_t>(0, (int64_t)std::floor((double)nx[c] * out_per_in));
        }
        switch (r() % 8) {
        case 0: ny[c] = 0; break;                                  // no cotangent at all: gx is zeros
        case 1: ny[c] = std::max<int64_t>(0, ny[c] - 1000); break; // truncated by 1000
        case 2: ny[c] = std::max<int64_t>(0, ny[c] - 1); break;
        default: break;
        }
        if (nx[c] == 0) ny[c] = 0;
        sx += nx[c] + 3; sy += ny[c];
    }
    t.gy_chs = t.ch > 1 ? sy + (int64_t)(r() % 5) : 0;
    t.gx_chs = t.ch > 1 ? sx + (int64_t)(r() % 5) : 0;
    int64_t px = 0, py = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        const int64_t row[4] = {py, ny[c], px, nx[c]};
        t.rows.insert(t.rows.end(), row, row + 4);
        py += ny[c]; px += nx[c] + 3; // (three guard elements between clips on the gx side)
    }
    return t;
}

static long g_two = 0, g_short = 0, g_empty = 0, g_zero_y = 0, g_cut = 0;
static void check_table(const Stage &st, const Table &t, size_t width, int64_t budget, int fft_T)
{
    const int P = width == 4 ? 64 : 128;
    const PolyStage s = poly_stage(st.T2, P, st.T2 + 1, st.Ls, st.Ms);
    const bool up = st.up != 0;
    const RaggedPolyAdjPlan rp = ragged_poly_adj_plan(t.rows.data(), t.n_clips, t.ch, t.gy_chs, t.gx_chs, width, up, s, fft_T, budget);
    const RaggedPolyPlan &f = rp.fwd;

    // ---- the partition, by the statement of each class
    std::vector<int64_t> want_short;
    uint32_t n_two = 0;
    CHECK(f.cls.size() == t.n_clips, "one class per clip");
    for (uint32_t c = 0; c < t.n_clips; ++c) {
        const int64_t *row = &t.rows[4 * (size_t)c];
        const int64_t n_y = row[1], n_x = row[3];
        const bool empty = n_x == 0, two = !empty && admits_alone(n_x, n_y, t.ch, width, st, P);
        const int want = empty ? kRaggedPolyEmpty : two ? kRaggedPolyTwo : kRaggedPolyShort;
        CHECK(f.cls[c] == want, "clip %u (n_x %lld, n_y %lld): class %d, want %d", c, (long long)n_x, (long long)n_y, (int)f.cls[c], want);
        CHECK(two == poly_adj_admits(n_x, n_y, t.ch, width, s), "clip %u: not the equal-length selector's question of the clip alone", c);
        if (!empty && !two) want_short.insert(want_short.end(), row, row + 4);
        if (n_y == 0 && n_x > 0) { CHECK(want == kRaggedPolyShort, "a clip without cotangent is the exact adjoint's (zeros)"); ++g_zero_y; }
        n_two += two; g_empty += empty;
    }
    CHECK(rp.short_rows == want_short, "the short sub-table is the short clips' ADJOINT rows, compacted, in table order");
    g_short += rp.n_short(); g_two += n_two;
    const uint32_t n_cols = rp.n_cols();
    CHECK(n_cols == n_two * t.ch && rp.fft_rows.size() == 4 * (size_t)n_cols && f.poly_rows.size() == 4 * (size_t)n_cols, "%u columns for %u clips", n_cols, n_two);
    CHECK(rp.ranges.size() == f.ranges.size(), "one transposed range per range");
    CHECK(rp.n_lo == (up ? -f.pad : 0), "k_poly_adj's first sample");

    // ---- ranges and columns
    uint32_t next = 0;
    for (size_t r = 0; r < f.ranges.size() && r < rp.ranges.size(); ++r) {
        const RaggedPolyRange &g = f.ranges[r];
        CHECK(g.first == next && g.count >= 1 && g.count <= kPolyMaxCols, "range %zu: columns [%u, +%u)", r, g.first, g.count);
        CHECK(g.mid_elems * (int64_t)width <= budget || g.count == 1, "range %zu over the budget", r);
        next = g.first + g.count;
        if (next > n_cols) break;
        int64_t end = 0, src_longest = 0, fin = 0, fout = 0;
        for (uint32_t i = g.first; i < next; ++i) {
            const int64_t *row = &t.rows[4 * (size_t)f.col_clip[i]], *pr = &f.poly_rows[4 * (size_t)i], *fr = &rp.fft_rows[4 * (size_t)i];
            const int64_t n_y = row[1], n_x = row[3], off = f.col_off[i];
            const int64_t gy_col = row[0] + (int64_t)f.col_ch[i] * t.gy_chs, gx_col = row[2] + (int64_t)f.col_ch[i] * t.gx_chs;
            // what launch_adjoint_two_stage sets for the clip alone: the FORWARD job's intermediate (in_frames = n_x, out_frames = n_y)
            const TwoStageMid m = two_stage_mid(up, st.T2, st.Ls, st.Ms, n_x, two_stage_mid_outputs(up, st.Ls, st.Ms, n_x, n_y, fft_T), 1, false);
            CHECK(f.col_mid[i].pad == m.pad && f.col_mid[i].n_core == m.n_core && f.col_mid[i].n_mid == m.n_mid, "column %u: not two_stage_mid of the clip alone", i);
            // inside the range's intermediate, disjoint, packed
            CHECK(off % 8 == 0 && off == end && off + m.n_mid <= g.mid_elems, "column %u at %lld (+%lld) of %lld", i, (long long)off, (long long)m.n_mid, (long long)g.mid_elems);
            end = off + (m.n_mid + 7) / 8 * 8;
            if (up) {
                // two_stage_adj_run, up: pj.src = mid + pad (sample 0), n_lo = -pad, n_src = n_core + pad; pj.dst = gy, k_lo = 0, n_out = n_y;
                // fj.in = mid, in_abs0 = -pad, in_frames = n_mid (END = n_core + pad); fj.out = gx, out_frames = n_x
                CHECK(pr[0] == off + m.pad && pr[1] == m.n_core + m.pad && pr[2] == gy_col && pr[3] == n_y, "up poly row %u", i);
                CHECK(fr[0] == off && fr[1] == -m.pad + m.n_mid && fr[2] == gx_col && fr[3] == n_x, "up FFT row %u", i);
                CHECK(pr[1] - rp.n_lo == m.n_mid, "up: k_poly_adj writes the whole window");
            } else {
                // down: fj.in = gy, in_abs0 = pad / 2, in_frames = n_y (END = pad / 2 + n_y); fj.out = mid, out_frames = n_mid;
                // pj.src = gx, n_lo = 0, n_src = n_x; pj.dst = mid, k_lo = -pad, n_out = n_mid
                CHECK(fr[0] == gy_col && fr[1] == m.pad / 2 + n_y && fr[2] == off && fr[3] == m.n_mid, "down FFT row %u", i);
                CHECK(pr[0] == gx_col && pr[1] == n_x && pr[2] == off && pr[3] == m.n_mid, "down poly row %u", i);
            }
            src_longest = std::max(src_longest, pr[1] - rp.n_lo);
            fin = std::max(fin, up ? m.n_mid : n_y); fout = std::max(fout, up ? n_x : m.n_mid);
        }
        CHECK(end == g.mid_elems, "range %zu: %lld elements, its columns need %lld", r, (long long)g.mid_elems, (long long)end);
        CHECK(rp.ranges[r].src_longest == src_longest && rp.ranges[r].fft_in_longest == fin && rp.ranges[r].fft_out_longest == fout, "range %zu: the longest column's numbers", r);
        CHECK(src_longest > 0, "a range has something to write");
    }
    CHECK(next == n_cols, "ranges cover %u of %u columns", next, n_cols);
    g_cut += f.ranges.size() > 1;
}

// ---- the ragged grid: a column gets kPolyAdjRaggedOver times its share of the slots, at most its tiles, at least one -----------
static void check_grid()
{
    for (int64_t tiles : {(int64_t)1, (int64_t)7, (int64_t)469, (int64_t)1 << 20})
        for (int per_cu : {0, 1, 2, 3, 4})
            for (uint64_t cols : {(uint64_t)1, (uint64_t)64, (uint64_t)1024, (uint64_t)65535}) {
                const unsigned gx = poly_adj_grid_x_ragged(tiles, per_cu, 256, cols);
                const int64_t share = (int64_t)kPolyAdjRaggedOver * (per_cu > 0 ? per_cu : 1) * 256 / (int64_t)cols;
                CHECK(gx >= 1 && (int64_t)gx <= tiles, "tiles %lld per_cu %d cols %llu: grid x %u", (long long)tiles, per_cu, (unsigned long long)cols, gx);
                CHECK((int64_t)gx == std::max<int64_t>(1, std::min(tiles, share)), "tiles %lld per_cu %d cols %llu: grid x %u, share %lld", (long long)tiles, per_cu,
                      (unsigned long long)cols, gx, (long long)share);
            }
    CHECK(poly_adj_grid_x_ragged(469, 3, 256, 64) == 48 && poly_adj_grid_x(469, 3, 256, 64) == 8, "the 64-clip corpus of profiles/NOTES_adjoint_auto.md");
}

int main()
{
    check_decisions();
    check_refusals();
    check_grid();
    std::mt19937_64 r(20260113);
    const int kTrials = 3000;
    for (int trial = 0; trial < kTrials; ++trial) {
        const Stage st = kReal[r() % kNReal];
        const size_t width = (trial & 1) ? 8 : 4;
        const int64_t budget = trial % 4 == 0 ? kPolyMidBudget : (int64_t)1 << (16 + r() % 8);
        const Table t = random_table(r, st, (uint32_t)(r() % 13));
        check_table(st, t, width, budget, 8 * (1 + (int)(r() % 120)));
    }
    // more columns than one launch holds
    for (int up = 0; up < 2; ++up) {
        const Stage st = up ? kReal[9] : kReal[2];
        Table t;
        t.n_clips = 70000; t.ch = 1; t.gy_chs = t.gx_chs = 0;
        for (uint32_t c = 0; c < t.n_clips; ++c) {
            const int64_t row[4] = {(int64_t)c * 20001, up ? 16000 : 8192, (int64_t)c * 20000, up ? 8192 : 17000};
            t.rows.insert(t.rows.end(), row, row + 4);
        }
        check_table(st, t, 4, (int64_t)1 << 40, 400);
        const RaggedPolyAdjPlan rp = ragged_poly_adj_plan(t.rows.data(), t.n_clips, 1, 0, 0, 4, up != 0, poly_stage(st.T2, 64, st.T2 + 1, st.Ls, st.Ms), 400, (int64_t)1 << 40);
        CHECK(rp.ranges.size() == 2 && rp.fwd.ranges[0].count == kPolyMaxCols, "70 000 columns: %zu ranges", rp.ranges.size());
    }
    CHECK(g_two > 1000 && g_short > 1000 && g_empty > 100 && g_zero_y > 100 && g_cut > 100, "the tables did not reach the cases: %ld two-stage, %ld short, %ld empty, %ld without cotangent, %ld cut",
          g_two, g_short, g_empty, g_zero_y, g_cut);
    std::printf("adjoint_auto_rules_check: %d tables, %ld two-stage clips, %ld short, %ld empty, %ld without cotangent, %ld cut tables\n", kTrials, g_two, g_short, g_empty,
                g_zero_y, g_cut);
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
