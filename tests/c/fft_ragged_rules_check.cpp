// fft_ragged_rules_check.cpp — the rules of k_fft_strided2 on a clip table (python-soxr_amd/csrc/fft_ragged_rules.h) against
// slow, independent statements of them: over the grid of the longest clip, the work-item map — with and without the
// XCD-aware order — visits every (clip, unit, item) below a clip's own item count exactly once and nothing at or above it;
// the item count of a clip is the number of blocks (or block pairs) that hold one of its outputs; the table conditions agree
// with their restatements.  No device, no other source file.  Exit status 0 = every check held (tests/test_fft_ragged_rules.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fft_ragged_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

static const int64_t kCounts[] = {0, 1, 2, 7, 8, 9, 17};
static const uint32_t kUnits[] = {1, 2, 3, 4};

// ---- the item count of a clip --------------------------------------------------------------------------------------------
// slow statement: walk the outputs; block b holds outputs [b hop, (b + 1) hop); an item is a block, or blocks 2 i and 2 i + 1
static void check_items()
{
    for (int64_t hop : {(int64_t)1, (int64_t)3, (int64_t)8, (int64_t)50})
        for (int64_t n = 0; n <= 4 * hop + 9; ++n)
            for (int cp = 0; cp < 2; ++cp) {
                std::vector<char> seen;
                for (int64_t k = 0; k < n; ++k) {
                    const int64_t item = cp ? k / hop : (k / hop) / 2;
                    if ((int64_t)seen.size() <= item) seen.resize((size_t)item + 1, 0);
                    seen[(size_t)item] = 1;
                }
                CHECK(fft_clip_items(n, hop, cp != 0) == (int64_t)seen.size(), "n %ld hop %ld cp %d", (long)n, (long)hop, cp);
                // the kernel's early exit: item i has work iff its first output exists
                const int64_t items = fft_clip_items(n, hop, cp != 0);
                for (int64_t i = 0; i < items + 3; ++i) CHECK((i * (cp ? 1 : 2) * hop < n) == (i < items), "item %ld of %ld", (long)i, (long)items);
            }
    CHECK(fft_clip_items(-5, 8, true) == 0 && fft_clip_items(-5, 8, false) == 0, "a negative count");
}

// ---- the work-item map -------------------------------------------------------------------------------------------------
// A table of clips whose own item counts are `own`, launched on the grid of the longest: every workgroup id asks the map with
// its clip's OWN count (the one per_xcd source the kernel has — the clip's own item count).
static void check_xcd_map()
{
    for (uint32_t units : kUnits)
        for (int64_t longest : kCounts) {
            const int64_t gx = fft_xcd_grid_x(longest, units);
            CHECK(gx % (8 * units) == 0 && gx >= longest * units && gx < (longest + 8) * units, "grid %ld", (long)gx);
            for (int64_t own : kCounts) {
                if (own > longest) continue;
                std::vector<int> visits((size_t)(units * (own + 1)), 0);
                long dead = 0;
                for (int64_t x = 0; x < gx; ++x) {
                    const FftMapItem m = fft_xcd_map((uint32_t)x, units, own);
                    CHECK(m.unit < units, "unit %u of %u", m.unit, units);
                    if (!m.live) { ++dead; continue; }
                    CHECK((int64_t)m.item < own, "a live id at or above the clip's count: item %u of %ld", m.item, (long)own);
                    if ((int64_t)m.item < own) ++visits[(size_t)(m.unit * own + m.item)];
                    // an XCD's ids (x mod 8) hold a contiguous run of items: [xcd * per_xcd, (xcd + 1) * per_xcd)
                    const int64_t per_xcd = (own + 7) / 8;
                    CHECK((int64_t)m.item / per_xcd == x % 8, "item %u on XCD %ld", m.item, (long)(x % 8));
                }
                for (uint32_t u = 0; u < units; ++u)
                    for (int64_t i = 0; i < own; ++i) CHECK(visits[(size_t)(u * own + i)] == 1, "units %u own %ld longest %ld: (%u, %ld) visited %d times", units, (long)own, (long)longest, u, (long)i, visits[(size_t)(u * own + i)]);
                CHECK(dead == gx - own * units, "ids without work: %ld", dead);
                // the units of one item sit on ids that are congruent mod 8 and adjacent in dispatch order (8 apart)
                if (own > 0)
                    for (int64_t x = 0; x + 8 < gx; ++x) {
                        const FftMapItem a = fft_xcd_map((uint32_t)x, units, own), b = fft_xcd_map((uint32_t)(x + 8), units, own);
                        if (a.live && b.live && a.unit + 1 < units) CHECK(b.item == a.item && b.unit == a.unit + 1, "id %ld", (long)x);
                    }
            }
        }
}

static void check_plain_map()
{
    for (uint32_t units : kUnits)
        for (int64_t longest : kCounts)
            for (int64_t own : kCounts) {
                if (own > longest) continue;
                const uint32_t clips = 3;
                std::vector<int> visits((size_t)(clips * units * (own + 1)), 0);
                for (uint32_t y = 0; y < clips * units; ++y)
                    for (int64_t x = 0; x < longest; ++x) {
                        const FftMapItem m = fft_plain_map((uint32_t)x, y, units, own);
                        CHECK(m.unit == y % units, "unit");
                        CHECK(m.live == (x < own), "x %ld own %ld", (long)x, (long)own);
                        if (m.live) ++visits[(size_t)((y / units * units + m.unit) * own + m.item)];
                    }
                for (size_t i = 0; i < (size_t)(clips * units * own); ++i) CHECK(visits[i] == 1, "plain map: %zu visited %d times", i, visits[i]);
            }
}

// ---- the table conditions ------------------------------------------------------------------------------------------------
static void check_table()
{
    CHECK(fft_map_clips_ok(0) && fft_map_clips_ok(1) && fft_map_clips_ok(65535) && !fft_map_clips_ok(65536) && !fft_map_clips_ok(0xffffffffu), "clips in grid.y");
    // every pattern of offset parities over three clips (frame counts play no part)
    for (int bits = 0; bits < 64; ++bits) {
        int64_t rows[12];
        bool even = true;
        for (int c = 0; c < 3; ++c) {
            const int in_odd = (bits >> (2 * c)) & 1, out_odd = (bits >> (2 * c + 1)) & 1;
            rows[4 * c] = 100 * c + in_odd; rows[4 * c + 1] = 7 + c; rows[4 * c + 2] = 200 * c + out_odd; rows[4 * c + 3] = 5 + c;
            // slow statement: the byte address of the clip's first int16 pair, from a 4-byte aligned base, is 4-byte aligned
            if ((rows[4 * c] * 2) % 4 != 0 || (rows[4 * c + 2] * 2) % 4 != 0) even = false;
        }
        CHECK(fft_table_words_aligned(rows, 3) == even, "parities %d", bits);
        CHECK(fft_table_words_aligned(rows, 0), "an empty table");
    }
    for (int m = 0; m < 16; ++m) {
        const bool v2 = m & 1, cp = m & 2, st = m & 4, by_name = m & 8;
        const bool want = v2 ? true : ((cp || st) ? by_name : false);
        CHECK(fft_table_form_served(v2, cp, st, by_name) == want, "forms %d", m);
    }
}

int main()
{
    check_items();
    check_xcd_map();
    check_plain_map();
    check_table();
    std::printf("fft_ragged_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
