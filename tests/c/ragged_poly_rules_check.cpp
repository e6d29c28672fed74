// ragged_poly_rules_check.cpp — the rules of the two-stage form on a clip table (python-soxr_amd/csrc/poly_rules.h
// ragged_poly_plan: the partition of the clips, each column's intermediate, the packed offsets, the rows of both stages in
// both directions, the ranges) against slow independent statements over seeded random tables: up and down, 1-3 channels,
// float32 and float64, empty clips, clips one frame either side of the 8192-frame admission edge, columns above the byte
// budget, more columns than one launch holds.  No device, no library.  Exit status 0 = every check held
// (tests/test_ragged_poly_rules.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

struct Stage { int T2; long long Ls, Ms; int up; };
// real stages (tests/c/poly_rules_check.cpp kReal: dev.Plan(in, out, HQ | VHQ) of the GPU tests' rate pairs), both directions
static const Stage kReal[] = {
    {12, 29401LL, 16000LL, 0}, {16, 15123LL, 12434LL, 0}, {20, 999999LL, 1000000LL, 0}, {24, 10031LL, 12997LL, 0}, {28, 100001LL, 100000LL, 0},
    {32, 16015LL, 18487LL, 0}, {40, 100001LL, 150000LL, 0}, {48, 30938LL, 55659LL, 0}, {20, 10601LL, 8617LL, 1}, {20, 1000001LL, 2000000LL, 1},
    {28, 92231LL, 20988LL, 1}, {28, 3000003LL, 2000000LL, 1}, {28, 804787693LL, 204633014LL, 1},
};
static const int kNReal = (int)(sizeof kReal / sizeof kReal[0]);
static const int kTaps[10] = {8, 12, 16, 20, 24, 28, 32, 40, 48, 56};

static double unit_rand(std::mt19937_64 &r) { return (double)(r() >> 11) * (1. / 9007199254740992.); }
static Stage random_stage(std::mt19937_64 &r)
{
    Stage s;
    s.T2 = kTaps[r() % 10];
    s.up = (int)(r() & 1);
    for (;;) {
        static const long long lims[4] = {64, 5000, 100000, 1LL << 31};
        s.Ls = 1 + (long long)(r() % (unsigned long long)lims[r() % 4]);
        s.Ms = (long long)std::llround((.125 + (2.1 - .125) * unit_rand(r)) * (double)s.Ls);
        const double ratio = (double)s.Ms / (double)s.Ls;
        if (s.Ms >= 1 && s.Ms <= (1LL << 31) && ratio > .125 && ratio <= 2.1) return s;
    }
}

// the admission of a clip ALONE, restated: 8192 frames or more either side, fewer than 2^30, its channels within one launch,
// table + one tile's span within 150 KiB
static bool admits_alone(int64_t n, int64_t n_out, uint32_t ch, size_t width, const Stage &st, int P)
{
    if (n < 8192 || n_out < 8192) return false;
    if (n >= 1073741824LL || n_out >= 1073741824LL) return false;
    if (ch > 65535) return false;
    const double ratio = (double)st.Ms / (double)st.Ls;
    const size_t tab = (size_t)P * (size_t)(st.T2 + 1) * 4 * width;
    const size_t tile = (size_t)(512. * (ratio + 1.01) + st.T2 + 4) * width;
    return tab + tile <= 150u * 1024u;
}

struct Table {
    std::vector<int64_t> rows;
    uint32_t n_clips, ch;
    int64_t in_chs, out_chs;
};
// frame counts around everything the rules branch on
static int64_t pick_frames(std::mt19937_64 &r, bool huge_ok)
{
    switch (r() % 10) {
    case 0: return 0;
    case 1: return 1 + (int64_t)(r() % 300);
    case 2: return 8191;
    case 3: return 8192;
    case 4: return 8193;
    case 5: return 8192 + (int64_t)(r() % 64);
    case 6: return huge_ok ? (int64_t)(1 << 27) + (int64_t)(r() % (3u << 28)) : 20000; // up to 2^27 + 3 2^28 > 2^29: a column above 1 GiB, some clips above 2^30
    default: return 8192 + (int64_t)(r() % 500000);
    }
}
static Table random_table(std::mt19937_64 &r, const Stage &st, uint32_t n_clips, bool huge_ok)
{
    Table t;
    t.n_clips = n_clips;
    t.ch = 1 + (uint32_t)(r() % 3);
    // output frames per input frame of the whole resampler: up 2 Ls / Ms, down Ls / (2 Ms)
    const double out_per_in = st.up ? 2. * (double)st.Ls / (double)st.Ms : .5 * (double)st.Ls / (double)st.Ms;
    std::vector<int64_t> n(n_clips), o(n_clips);
    int64_t si = 0, so = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        if (r() % 2) { // the output count drawn, the input count the least that reaches it (and a frame either side of that)
            o[c] = pick_frames(r, huge_ok);
            n[c] = std::max<int64_t>(0, (int64_t)std::ceil((double)o[c] / out_per_in) + (int64_t)(r() % 3) - 1);
            if (n[c] == 0) o[c] = 0;
        } else {
            n[c] = pick_frames(r, huge_ok);
            o[c] = std::max<int64_t>(0, (int64_t)std::floor((double)n[c] * out_per_in) - (int64_t)(r() % 9));
        }
        if (r() % 16 == 0) o[c] = 0; // an empty clip with input
        si += n[c]; so += o[c] + 1;
    }
    const bool split = r() % 2; // planar channels a whole buffer apart, or right behind each clip
    t.in_chs = split ? si + (int64_t)(r() % 5) : 0;
    t.out_chs = split ? so + (int64_t)(r() % 5) : 0;
    int64_t pi = 0, po = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        const int64_t row[4] = {pi, n[c], po, o[c]};
        t.rows.insert(t.rows.end(), row, row + 4);
        pi += split ? n[c] : n[c] * t.ch;
        po += split ? o[c] + 1 : (o[c] + 1) * t.ch;
    }
    if (!split) { t.in_chs = -1; t.out_chs = -1; } // (marked: per-clip channel strides cannot be one job's — use mono)
    return t;
}

static void check_table(const Stage &st, const Table &t, size_t width, int64_t budget, int fft_T)
{
    const int P = width == 4 ? 64 : 128;
    const PolyStage s = poly_stage(st.T2, P, st.T2 + 1, st.Ls, st.Ms);
    const bool up = st.up != 0;
    const RaggedPolyPlan rp = ragged_poly_plan(t.rows.data(), t.n_clips, t.ch, t.in_chs, t.out_chs, width, up, s, fft_T, budget);

    // ---- the partition: every clip in exactly one class, by the statement of each class
    CHECK(rp.cls.size() == t.n_clips, "one class per clip");
    std::vector<int64_t> want_short;
    uint32_t n_two = 0, n_empty = 0;
    for (uint32_t c = 0; c < t.n_clips; ++c) {
        const int64_t *row = &t.rows[4 * (size_t)c];
        const bool empty = row[3] == 0, two = !empty && admits_alone(row[1], row[3], t.ch, width, st, P), shrt = !empty && !two;
        CHECK((int)empty + (int)two + (int)shrt == 1, "clip %u in %d classes", c, (int)empty + (int)two + (int)shrt);
        const int want = empty ? kRaggedPolyEmpty : two ? kRaggedPolyTwo : kRaggedPolyShort;
        CHECK(rp.cls[c] == want, "clip %u (n %lld, n_out %lld): class %d, want %d", c, (long long)row[1], (long long)row[3], (int)rp.cls[c], want);
        CHECK(two == two_stage_admits(row[1], row[3], t.ch, width, s), "clip %u: not the admission of the clip alone", c);
        if (shrt) want_short.insert(want_short.end(), row, row + 4);
        n_two += two; n_empty += empty;
    }
    CHECK(rp.short_rows == want_short, "the short sub-table is the short clips' rows, compacted, in table order");
    CHECK(rp.n_short() + n_two + n_empty == t.n_clips, "classes do not add up");

    // ---- columns: the channels of each two-stage clip, clip-major; each column's intermediate is the clip's alone
    const uint32_t n_cols = rp.n_cols();
    CHECK(n_cols == n_two * t.ch, "%u columns for %u two-stage clips of %u channels", n_cols, n_two, t.ch);
    CHECK(rp.col_ch.size() == n_cols && rp.col_mid.size() == n_cols && rp.col_off.size() == n_cols && rp.poly_rows.size() == 4 * (size_t)n_cols &&
              rp.fft_rows.size() == 4 * (size_t)n_cols, "per-column tables of one length");
    {
        uint32_t i = 0;
        for (uint32_t c = 0; c < t.n_clips; ++c)
            for (uint32_t ch = 0; ch < t.ch && rp.cls[c] == kRaggedPolyTwo; ++ch, ++i)
                if (i < n_cols) CHECK(rp.col_clip[i] == c && rp.col_ch[i] == ch, "column %u is (clip %u, channel %u)", i, c, ch);
        CHECK(i == n_cols, "columns enumerate the two-stage clips' channels");
    }
    for (uint32_t i = 0; i < n_cols; ++i) {
        const int64_t *row = &t.rows[4 * (size_t)rp.col_clip[i]];
        // the outputs the clip ALONE sizes its intermediate for (launch_two_stage): its own count — or, down and truncated below the
        // plan's output length floor(n Ls / (2 Ms) + 1/2), as far past it as the FFT stage's filter reaches (fft_T / 2 samples of the
        // intermediate = fft_T / 4 outputs), the signal's end at the most
        int64_t sized = row[3];
        if (!up) {
            const int64_t full = (int64_t)(((__int128)row[1] * st.Ls + st.Ms) / (2 * (__int128)st.Ms));
            for (int64_t more = 0; 4 * more < fft_T && sized < full; ++more) ++sized;
            CHECK(sized == two_stage_mid_outputs(false, st.Ls, st.Ms, row[1], row[3], fft_T), "column %u: sized for %lld outputs", i, (long long)sized);
            CHECK(row[3] < full || sized == row[3], "a whole clip is sized by its own outputs");
            CHECK(2 * sized + rp.pad >= std::min(2 * full, 2 * (row[3] - 1) + fft_T / 2), "column %u: the FFT stage reads past the intermediate", i);
        } else
            CHECK(two_stage_mid_outputs(true, st.Ls, st.Ms, row[1], row[3], fft_T) == row[3], "up: sized by the outputs");
        for (int inter = 0; inter < 2; ++inter) { // (pad, n_core, n_mid of the clip alone do not depend on its layout)
            const TwoStageMid m = two_stage_mid(up, st.T2, st.Ls, st.Ms, row[1], sized, t.ch, inter != 0);
            CHECK(rp.col_mid[i].pad == m.pad && rp.col_mid[i].n_core == m.n_core && rp.col_mid[i].n_mid == m.n_mid, "column %u: not two_stage_mid of the clip alone", i);
        }
        CHECK(rp.col_mid[i].pad == rp.pad && rp.pad % 8 == 0, "pad is the plan's");
    }

    // ---- ranges: cover every column exactly once, in order; both caps; a column above the budget alone
    uint32_t next = 0;
    for (size_t r = 0; r < rp.ranges.size(); ++r) {
        const RaggedPolyRange &g = rp.ranges[r];
        CHECK(g.first == next && g.count >= 1, "range %zu starts at %u, want %u", r, g.first, next);
        CHECK(g.count <= kPolyMaxCols, "range %zu: %u columns", r, g.count);
        CHECK(g.mid_elems * (int64_t)width <= budget || g.count == 1, "range %zu: %lld bytes in %u columns over the budget %lld", r,
              (long long)(g.mid_elems * (int64_t)width), g.count, (long long)budget);
        next = g.first + g.count;
        if (next > n_cols) break;
        // (greedy: the next column would have broken a cap)
        if (next < n_cols)
            CHECK(g.count == kPolyMaxCols || (g.mid_elems + (rp.col_mid[next].n_mid + 7) / 8 * 8) * (int64_t)width > budget, "range %zu was cut early", r);
        // the columns' extents inside the range's intermediate: 8-element aligned, disjoint, inside the allocation, no gaps
        int64_t end = 0, poly_longest = 0, fin = 0, fout = 0;
        for (uint32_t i = g.first; i < g.first + g.count; ++i) {
            const TwoStageMid &m = rp.col_mid[i];
            const int64_t off = rp.col_off[i];
            CHECK(off % 8 == 0, "column %u at %lld: not 8-element aligned", i, (long long)off);
            CHECK(off >= end, "column %u overlaps the one before", i);
            CHECK(off + m.n_mid <= g.mid_elems, "column %u leaves the allocation", i);
            CHECK(off == end, "column %u: a gap in the packed intermediate", i);
            end = off + (m.n_mid + 7) / 8 * 8;
            // ---- the rows of both stages, restated per direction
            const int64_t *row = &t.rows[4 * (size_t)rp.col_clip[i]], *pr = &rp.poly_rows[4 * (size_t)i], *fr = &rp.fft_rows[4 * (size_t)i];
            const int64_t in_col = row[0] + (int64_t)rp.col_ch[i] * t.in_chs, out_col = row[2] + (int64_t)rp.col_ch[i] * t.out_chs;
            if (up) {
                // FFT stage: reads the caller's samples [0, n) as absolute samples [pad / 2, pad / 2 + n), writes n_mid outputs = the column
                CHECK(fr[0] == in_col && fr[1] - m.pad / 2 == row[1] && fr[2] == off && fr[3] == m.n_mid, "up FFT row %u", i);
                // polyphase stage: samples [-pad, n_core + pad) of the column are its n_mid elements; outputs = the clip's
                CHECK(pr[0] - m.pad == off && pr[1] + m.pad == m.n_mid && pr[2] == out_col && pr[3] == row[3], "up poly row %u", i);
            } else {
                // polyphase stage: reads the caller's samples [0, n), writes outputs [-pad, n_core + pad) = the column
                CHECK(pr[0] == in_col && pr[1] == row[1] && pr[2] == off && pr[3] == m.n_mid, "down poly row %u", i);
                // FFT stage: absolute samples [-pad, n_core + pad) are the column's n_mid elements; outputs = the clip's
                CHECK(fr[0] == off && fr[1] + m.pad == m.n_mid && fr[2] == out_col && fr[3] == row[3], "down FFT row %u", i);
            }
            poly_longest = std::max(poly_longest, pr[3]);
            fin = std::max(fin, up ? row[1] : m.n_mid); fout = std::max(fout, fr[3]);
        }
        CHECK(end == g.mid_elems, "range %zu: %lld elements, its columns need %lld", r, (long long)g.mid_elems, (long long)end);
        CHECK(g.poly_longest == poly_longest && g.fft_in_longest == fin && g.fft_out_longest == fout, "range %zu: the longest column's numbers", r);
    }
    CHECK(next == n_cols, "ranges cover %u of %u columns", next, n_cols);
    CHECK(n_cols != 0 || rp.ranges.empty(), "no column, no range");
}

int main()
{
    std::mt19937_64 r(20240611);
    const int kTrials = 4000;
    long two_seen = 0, cut_seen = 0, over_seen = 0;
    for (int trial = 0; trial < kTrials; ++trial) {
        const Stage st = trial < 4 * kNReal ? kReal[trial % kNReal] : random_stage(r);
        const size_t width = (trial & 1) ? 8 : 4;
        const bool real_budget = trial % 4 == 0; // the product's 1 GiB with huge clips; else a small budget that cuts ordinary tables
        const int64_t budget = real_budget ? kPolyMidBudget : (int64_t)1 << (16 + r() % 8);
        Table t = random_table(r, st, (uint32_t)(r() % 13), real_budget);
        if (t.in_chs < 0) { t.ch = 1; t.in_chs = t.out_chs = 0; } // (packed clips: mono)
        const int fft_T = 8 * (1 + (int)(r() % 120)); // (the FFT stage's taps: a multiple of 8, up to 960)
        check_table(st, t, width, budget, fft_T);
        const PolyStage s = poly_stage(st.T2, width == 4 ? 64 : 128, st.T2 + 1, st.Ls, st.Ms);
        const RaggedPolyPlan rp = ragged_poly_plan(t.rows.data(), t.n_clips, t.ch, t.in_chs, t.out_chs, width, st.up != 0, s, fft_T, budget);
        two_seen += rp.n_cols(); cut_seen += rp.ranges.size() > 1;
        for (const RaggedPolyRange &g : rp.ranges) over_seen += g.mid_elems * (int64_t)width > budget;
    }
    // more columns than one launch holds: 70 000 mono clips at the admission edge
    for (int up = 0; up < 2; ++up) {
        const Stage st = up ? kReal[9] : kReal[2];
        Table t;
        t.n_clips = 70000; t.ch = 1; t.in_chs = t.out_chs = 0;
        for (uint32_t c = 0; c < t.n_clips; ++c) {
            const int64_t row[4] = {(int64_t)c * 20000, up ? 8192 : 17000, (int64_t)c * 20001, up ? 16000 : 8192};
            t.rows.insert(t.rows.end(), row, row + 4);
        }
        check_table(st, t, 4, kPolyMidBudget, 400); // (4.7 GB of intermediate: the byte budget cuts first)
        const int64_t roomy = (int64_t)1 << 40; // ... and with room for all of it, the column cap does
        check_table(st, t, 4, roomy, 400);
        const RaggedPolyPlan rp = ragged_poly_plan(t.rows.data(), t.n_clips, 1, 0, 0, 4, up != 0, poly_stage(st.T2, 64, st.T2 + 1, st.Ls, st.Ms), 400, roomy);
        CHECK(rp.ranges.size() == 2 && rp.ranges[0].count == kPolyMaxCols, "70 000 columns: %zu ranges", rp.ranges.size());
    }
    CHECK(two_seen > 1000 && cut_seen > 100 && over_seen > 5, "the tables did not reach the cases: %ld columns, %ld cut tables, %ld columns above the budget", two_seen,
          cut_seen, over_seen);
    std::printf("ragged_poly_rules_check: %d tables, %ld two-stage columns, %ld cut tables, %ld ranges of one column above the budget\n", kTrials, two_seen, cut_seen,
                over_seen);
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
