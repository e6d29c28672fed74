// ragged_interp_rules_check.cpp — the integer rules of a ragged launch on an interpolated-phase plan
// (python-soxr_amd/csrc/ragged_rules.h: ragged_span_grid_x, ragged_span_skip, ragged_span_total, ragged_total_out) against
// brute force over random clip tables and outputs per workgroup U (32: k_interp_wave; KO: k_interp_tile).  No device, no
// library.  Exit status 0 = every check held (tests/test_ragged_interp_rules.py).
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

// output k of a column lies in workgroup floor(k / U): said one output at a time
static std::vector<char> wgs_with_outputs(int64_t out_frames, int64_t U, int64_t n_wgs)
{
    std::vector<char> has((size_t)n_wgs + 1, 0); // (the last entry: outputs behind the grid)
    for (int64_t k = 0; k < out_frames; ++k) {
        const int64_t x = k / U;
        has[(size_t)(x < n_wgs ? x : n_wgs)] = 1;
    }
    return has;
}

static void check_spans(std::mt19937_64 &rng)
{
    const int64_t us[8] = {32, 480, 960, 2048, 1, 7, 3840, 16384};
    for (int trial = 0; trial < 600; ++trial) {
        const int64_t U = trial % 3 == 0 ? 1 + (int64_t)(rng() % 700) : us[rng() % 8];
        const uint32_t n = 1 + (uint32_t)(rng() % 12), cols_per_clip = 1 + (uint32_t)(rng() % 3);
        std::vector<int64_t> rows((size_t)n * 4, 0);
        for (uint32_t c = 0; c < n; ++c) {
            int64_t len;
            switch (rng() % 7) { // lengths at and beside the workgroup edges, and anywhere
            case 0: len = 0; break;
            case 1: len = 1; break;
            case 2: len = U * (int64_t)(rng() % 5) + (int64_t)(rng() % 3) - 1; break;
            case 3: len = 3 * U + 5; break;
            case 4: len = U - 1; break;
            default: len = (int64_t)(rng() % (uint64_t)(4 * U + 2));
            }
            rows[(size_t)c * 4 + 3] = len < 0 ? 0 : len;
            rows[(size_t)c * 4 + 1] = (int64_t)(rng() % 100);
            rows[(size_t)c * 4 + 0] = (int64_t)(rng() % 1000); rows[(size_t)c * 4 + 2] = (int64_t)(rng() % 1000);
        }
        int64_t longest = 0, outs = 0;
        for (uint32_t c = 0; c < n; ++c) {
            longest = rows[(size_t)c * 4 + 3] > longest ? rows[(size_t)c * 4 + 3] : longest;
            for (int64_t k = 0; k < rows[(size_t)c * 4 + 3]; ++k) ++outs;
        }
        CHECK(ragged_longest(rows.data(), n) == longest, "longest");
        CHECK(ragged_total_out(rows.data(), n) == outs, "outputs of the table: rule %ld, counted %ld", (long)ragged_total_out(rows.data(), n), (long)outs);
        CHECK(ragged_tile_considered(rows.data(), n) == (outs >= 4096), "the tile form is weighed from 4096 outputs per channel: %ld", (long)outs);
        const int64_t gx = ragged_span_grid_x(longest, U);
        int64_t kept_total = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const int64_t of = rows[(size_t)c * 4 + 3];
            const std::vector<char> has = wgs_with_outputs(of, U, gx);
            CHECK(has[(size_t)gx] == 0, "U=%ld: outputs of a clip of %ld behind a grid of %ld workgroups", (long)U, (long)of, (long)gx);
            int64_t kept = 0, covered = 0;
            for (int64_t x = 0; x < gx; ++x) {
                const bool skip = ragged_span_skip(x, U, of);
                // a workgroup is skipped exactly when no output of its clip lies in it
                CHECK(skip == (has[(size_t)x] == 0), "U=%ld out=%ld workgroup %ld of %ld: skip=%d, outputs there=%d", (long)U, (long)of, (long)x, (long)gx,
                      (int)skip, (int)has[(size_t)x]);
                if (skip) continue;
                ++kept;
                // what a kept workgroup writes: its U outputs below out_frames (n_here of k_interp_tile: at least one)
                const int64_t lo = x * U, hi = (x + 1) * U < of ? (x + 1) * U : of;
                CHECK(hi - lo >= 1 && hi - lo <= U, "a kept workgroup of %ld outputs (U=%ld)", (long)(hi - lo), (long)U);
                CHECK(lo == covered, "kept workgroups are not contiguous: U=%ld out=%ld workgroup %ld", (long)U, (long)of, (long)x);
                covered = hi;
            }
            // the workgroups kept cover [0, out_frames) of every clip once
            CHECK(covered == of, "U=%ld: clip of %ld outputs covered to %ld by a grid of %ld", (long)U, (long)of, (long)covered, (long)gx);
            CHECK(kept == ragged_span_wgs(of, U), "workgroups of a clip: %ld kept, rule %ld", (long)kept, (long)ragged_span_wgs(of, U));
            kept_total += kept * cols_per_clip;
        }
        CHECK(ragged_span_total(rows.data(), n, cols_per_clip, U) == kept_total, "total workgroups %ld, counted %ld",
              (long)ragged_span_total(rows.data(), n, cols_per_clip, U), (long)kept_total);
        // the grid is no larger than the longest clip needs
        CHECK(gx == 0 ? longest == 0 : !ragged_span_skip(gx - 1, U, longest), "grid of %ld workgroups for a longest clip of %ld", (long)gx, (long)longest);
    }
}

// the largest launch: a clip of 2^30 outputs (longer tables stay clip by clip) at U = 1 and at the wave kernel's 32
static void check_limits()
{
    const int64_t big = (int64_t)1 << 30;
    CHECK(ragged_span_grid_x(big, 32) == big / 32 && ragged_span_grid_x(big + 1, 32) == big / 32 + 1, "grid of a 2^30 clip");
    CHECK(!ragged_span_skip(big / 32 - 1, 32, big) && ragged_span_skip(big / 32, 32, big), "skip at the end of a 2^30 clip");
    CHECK(ragged_span_skip(0, 32, 0) && ragged_span_skip(0, 16384, 0) && !ragged_span_skip(0, 16384, 1), "an empty clip skips workgroup 0");
    const int64_t rows[8] = {0, 0, 0, big, 0, 0, 0, big};
    CHECK(ragged_span_total(rows, 2, 3, 1) == 6 * big && ragged_total_out(rows, 2) == 2 * big, "totals beyond 2^32");
}

int main()
{
    std::mt19937_64 rng(20261019);
    check_spans(rng);
    check_limits();
    std::printf("ragged_interp_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
