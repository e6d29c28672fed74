// ragged_rules_check.cpp — the integer rules of a ragged exact launch (python-soxr_amd/csrc/ragged_rules.h) against brute
// force over random clip tables and slab geometries.  No device, no library.  Exit status 0 = every check held
// (tests/test_ragged_rules.py).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ragged_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

// output k of a column lies in slab floor(floor(k / Lc) / pb): said one output at a time
static std::vector<char> slabs_with_outputs(int64_t out_frames, int64_t Lc, int32_t pb, int64_t n_slabs)
{
    std::vector<char> has((size_t)n_slabs + 1, 0); // (the last entry: outputs behind the grid)
    for (int64_t k = 0; k < out_frames; ++k) {
        const int64_t period = k / Lc, slab = period / pb;
        has[(size_t)(slab < n_slabs ? slab : n_slabs)] = 1;
    }
    return has;
}

static void check_tiles(std::mt19937_64 &rng)
{
    const int32_t pbs[4] = {16, 32, 64, 1};
    for (int trial = 0; trial < 400; ++trial) {
        const int64_t Lc = 1 + (int64_t)(rng() % 60);
        const int32_t pb = pbs[rng() % 4];
        const uint32_t n = 1 + (uint32_t)(rng() % 12), ch = 1 + (uint32_t)(rng() % 3);
        std::vector<int64_t> rows((size_t)n * 4, 0);
        const int64_t slab = Lc * pb;
        for (uint32_t c = 0; c < n; ++c) {
            int64_t len;
            switch (rng() % 6) { // lengths at and beside the slab and period edges, and anywhere
            case 0: len = 0; break;
            case 1: len = slab * (int64_t)(rng() % 4) + (int64_t)(rng() % 3) - 1; break;
            case 2: len = Lc * (int64_t)(rng() % 9) + (int64_t)(rng() % 3) - 1; break;
            case 3: len = 1; break;
            default: len = (int64_t)(rng() % (uint64_t)(4 * slab + 2));
            }
            rows[(size_t)c * 4 + 3] = len < 0 ? 0 : len;
            rows[(size_t)c * 4 + 1] = (int64_t)(rng() % 100);
        }
        int64_t longest = 0;
        for (uint32_t c = 0; c < n; ++c) longest = rows[(size_t)c * 4 + 3] > longest ? rows[(size_t)c * 4 + 3] : longest;
        CHECK(ragged_longest(rows.data(), n) == longest, "longest");
        const int64_t gx = ragged_grid_x(longest, Lc, pb);
        int64_t kept_total = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const int64_t of = rows[(size_t)c * 4 + 3];
            const std::vector<char> has = slabs_with_outputs(of, Lc, pb, gx);
            CHECK(has[(size_t)gx] == 0, "Lc=%ld pb=%d: outputs of a clip of %ld behind a grid of %ld slabs", (long)Lc, pb, (long)of, (long)gx);
            int64_t kept = 0, covered = 0;
            for (int64_t x = 0; x < gx; ++x) {
                const bool skip = ragged_skip(x, Lc, pb, of);
                // a block is skipped exactly when no output of its clip lies in it
                CHECK(skip == (has[(size_t)x] == 0), "Lc=%ld pb=%d out=%ld slab %ld of %ld: skip=%d, outputs there=%d", (long)Lc, pb, (long)of, (long)x,
                      (long)gx, (int)skip, (int)has[(size_t)x]);
                if (skip) continue;
                ++kept;
                // what a kept block writes: its slab's outputs below out_frames
                const int64_t lo = x * slab, hi = (x + 1) * slab < of ? (x + 1) * slab : of;
                CHECK(lo == covered, "kept blocks are not contiguous: Lc=%ld pb=%d out=%ld slab %ld", (long)Lc, pb, (long)of, (long)x);
                covered = hi;
            }
            // the blocks kept cover [0, out_frames) of every clip
            CHECK(covered == of, "Lc=%ld pb=%d: clip of %ld outputs covered to %ld by a grid of %ld", (long)Lc, pb, (long)of, (long)covered, (long)gx);
            CHECK(kept == ragged_slabs(of, Lc, pb), "slabs of a clip: %ld kept, rule %ld", (long)kept, (long)ragged_slabs(of, Lc, pb));
            kept_total += kept * ch;
        }
        CHECK(ragged_total_slabs(rows.data(), n, ch, Lc, pb) == kept_total, "total slabs %ld, counted %ld", (long)ragged_total_slabs(rows.data(), n, ch, Lc, pb),
              (long)kept_total);
        // the grid is no larger than the longest clip needs
        CHECK(gx == 0 ? longest == 0 : !ragged_skip(gx - 1, Lc, pb, longest), "grid of %ld slabs for a longest clip of %ld", (long)gx, (long)longest);
    }
}

static void check_gather(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 300; ++trial) {
        const uint32_t lanes = 1 + (uint32_t)(rng() % 4); // 1, or the channels of channel-fast data
        const uint32_t n = 1 + (uint32_t)(rng() % 8);
        std::vector<int64_t> of(n);
        int64_t longest = 0;
        for (auto &v : of) { v = (rng() % 5 == 0) ? 0 : (int64_t)(rng() % 1500); longest = v > longest ? v : longest; }
        const int64_t gx = ragged_gather_grid_x(longest, lanes);
        for (uint32_t c = 0; c < n; ++c) {
            std::vector<int> hit((size_t)of[c] * lanes, 0);
            for (int64_t e = 0; e < gx * 256; ++e) { // every lane of the grid, as k_gather decomposes it
                const int64_t idx = e / lanes, ch = e - idx * lanes;
                if (ragged_gather_skip(idx, of[c])) continue;
                ++hit[(size_t)(idx * lanes + ch)];
            }
            bool once = true;
            for (int h : hit) once = once && h == 1;
            CHECK(once, "gather: clip of %ld outputs x %u lanes under a grid of %ld workgroups", (long)of[c], lanes, (long)gx);
        }
    }
}

static void check_fold(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 3000; ++trial) {
        uint32_t ch, n;
        switch (trial % 4) {
        case 0: ch = 1; n = 65534 + (uint32_t)(rng() % 4); break;
        case 1: ch = 1 + (uint32_t)(rng() % 70000); n = 1 + (uint32_t)(rng() % 100); break;
        case 2: ch = 1 + (uint32_t)(rng() % 8); n = (uint32_t)(rng() % 200000); break;
        default: ch = 1 + (uint32_t)(rng() % 300); n = (uint32_t)(rng() % 3000);
        }
        const uint32_t step = ragged_fold_step(ch);
        if (ch > kMaxGridY) {
            CHECK(step == 0 && ragged_fold_range(n, ch, 0).count == 0, "a clip of %u channels does not fit one launch", ch);
            continue;
        }
        CHECK(step >= 1 && (uint64_t)step * ch <= kMaxGridY && (uint64_t)(step + 1) * ch > kMaxGridY, "fold step %u for %u channels", step, ch);
        // the folded ranges partition the clips: in order, without gaps or overlap, each within gridDim.y
        uint64_t next = 0;
        uint32_t r = 0;
        for (;; ++r) {
            const RaggedRange g = ragged_fold_range(n, ch, r);
            if (!g.count) break;
            CHECK(g.first == next, "range %u of %u clips x %u channels starts at %u, expected %lu", r, n, ch, g.first, (unsigned long)next);
            CHECK((uint64_t)g.count * ch <= kMaxGridY, "range %u holds %u clips x %u channels", r, g.count, ch);
            next = (uint64_t)g.first + g.count;
            if (r > 300000) break;
        }
        CHECK(next == n, "ranges end at %lu of %u clips (%u channels)", (unsigned long)next, n, ch);
        CHECK(ragged_fold_range(n, ch, r + 1).count == 0, "a range behind the last");
        CHECK(n > step || r <= 1, "a table that fits is one launch");
    }
}

int main()
{
    std::mt19937_64 rng(20261018);
    check_tiles(rng);
    check_gather(rng);
    check_fold(rng);
    std::printf("ragged_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
