// vr_adjoint_rules_check.cpp — the rules of the ragged variable-rate adjoint (python-soxr_amd/csrc/vr_adjoint_rules.h): the
// range of cotangent samples a gradient frame sums over, against a true 128-bit division (host only) and against its defining
// property on the neighbours of both ends; the grid; what is refused of a row.  No device, nothing to link.  Every range it
// evaluated is printed as a line "RANGE a H step_hi step_lo n_y k_lo k_hi", which tests/test_vr_adjoint_rules.py recomputes in
// Python integers and checks by brute force over k.  Exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vr_adjoint_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL; // fixed seed
static uint64_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

// k is in frame a's range  <=>  (a - H) 2^64 <= k S < (a + H) 2^64  and  0 <= k < n_y   (signed 128-bit: a - H may be negative)
static bool member(int64_t k, int64_t a, int32_t H, u128 S, int64_t n_y)
{
    if (k < 0 || k >= n_y) return false;
    const __int128 t = (__int128)((u128)(uint64_t)k * S);
    const __int128 one = (__int128)1 << 64;
    return (__int128)(a - H) * one <= t && t < (__int128)(a + H) * one;
}

static void one_range(int64_t a, int32_t H, u128 S, int64_t n_y)
{
    const VrAdjRange r = vr_adj_k_range(a, H, S, n_y);
    // the formula, with the host's own 128-bit division
    const u128 lo_n = a > H ? (u128)(uint64_t)(a - H) << 64 : 0, hi_n = (u128)(uint64_t)(a + H) << 64;
    const int64_t lo = (int64_t)((lo_n + S - 1) / S), hc = (int64_t)((hi_n + S - 1) / S), hi = (hc < n_y ? hc : n_y) - 1;
    CHECK(r.lo == lo && r.hi == hi, "a=%lld H=%d n_y=%lld: [%lld, %lld], by division [%lld, %lld]", (long long)a, H, (long long)n_y,
          (long long)r.lo, (long long)r.hi, (long long)lo, (long long)hi);
    // the property at both ends: the ends are members (a range that is not empty), their outer neighbours are not
    if (r.lo <= r.hi) CHECK(member(r.lo, a, H, S, n_y) && member(r.hi, a, H, S, n_y), "a=%lld n_y=%lld: an end outside", (long long)a, (long long)n_y);
    CHECK(!member(r.lo - 1, a, H, S, n_y) && !member(r.hi + 1, a, H, S, n_y), "a=%lld n_y=%lld: a neighbour inside", (long long)a, (long long)n_y);
    std::printf("RANGE %lld %d %llu %llu %lld %lld %lld\n", (long long)a, H, (unsigned long long)(uint64_t)(S >> 64), (unsigned long long)(uint64_t)S,
                (long long)n_y, (long long)r.lo, (long long)r.hi);
}

static void check_ranges()
{
    const double ratios[8] = {std::ldexp(1., -19), 0.5, 0.9070294784580499, 1.0, 1.1, 1.1 * (1. - std::ldexp(1., -40)), 3.0, std::ldexp(1., 19)};
    const int32_t Hs[2] = {108, 4};
    for (double ratio : ratios) {
        const u128 S = vr_ragged_step(ratio);
        for (int32_t H : Hs) {
            const int64_t as[] = {0, 1, H - 1, H, H + 1, 255, 256, 257, 700, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 257};
            for (int64_t a : as) {
                // n_y: none, one, the whole support, and cuts inside the range (its first, a middle and its last sample)
                const VrAdjRange full = vr_adj_k_range(a, H, S, kVrRaggedMaxOut);
                const int64_t mid = full.lo + (full.hi - full.lo) / 2;
                const int64_t ns[] = {0, 1, kVrRaggedMaxOut, full.lo, full.lo + 1, mid, full.hi, full.hi + 1, full.hi + 2};
                for (int64_t n_y : ns)
                    if (n_y >= 0 && n_y <= kVrRaggedMaxOut) one_range(a, H, S, n_y);
            }
        }
    }
    CHECK(vr_adj_ceil_q64(0, (u128)1 << 64) == 0 && vr_adj_ceil_q64(5, (u128)1 << 64) == 5 && vr_adj_ceil_q64(5, (u128)1 << 63) == 10,
          "whole quotients are themselves");
    CHECK(vr_adj_ceil_q64(5, ((u128)1 << 64) + 1) == 5 && vr_adj_ceil_q64(5, ((u128)1 << 64) - 1) == 6, "one unit of the step either side of a whole quotient");
    for (int i = 0; i < 4000; ++i) { // random triples: frames up to 2^32, steps between 2^-19 and 2^19 at every scale, any n_y
        const int64_t a = (int64_t)(rnd() >> (32 + rnd() % 32));
        const int sh = (int)(rnd() % 38);
        u128 S = ((((u128)(rnd() & 0x7FFFF)) << 64) | rnd()) >> sh;
        if (S < ((u128)1 << 45)) S |= (u128)1 << 45;
        const int32_t H = 4 * (1 + (int32_t)(rnd() % 92));
        const VrAdjRange full = vr_adj_k_range(a, H, S, kVrRaggedMaxOut);
        const int64_t pick[3] = {(int64_t)(rnd() % ((uint64_t)kVrRaggedMaxOut + 1)), full.lo + (int64_t)(rnd() % 5), full.hi - (int64_t)(rnd() % 5) + 2};
        const int64_t n_y = pick[rnd() % 3];
        one_range(a, H, S, n_y < 0 ? 0 : n_y > kVrRaggedMaxOut ? kVrRaggedMaxOut : n_y);
    }
}

static void check_grid_and_rows()
{
    AdjGrid g = vr_adj_grid(700, 9, 256);
    CHECK(g.ok && g.gx == 3 && g.gy == 9, "700 frames, 9 columns: %u x %u", g.gx, g.gy);
    g = vr_adj_grid(256, 65536 * 2, 256);
    CHECK(g.ok && g.gx == 1 && g.gy == kJobMaxCols, "more columns than a grid holds wrap in the kernel: %u x %u", g.gx, g.gy);
    g = vr_adj_grid(257, 1, 256);
    CHECK(g.ok && g.gx == 2, "one frame behind a tile edge");
    CHECK(!vr_adj_grid(((int64_t)INT32_MAX + 1) * 256, 1, 256).ok && vr_adj_grid((int64_t)INT32_MAX * 256, 1, 256).ok, "the grid's frame axis ends at 2^31 - 1 tiles");
    const u128 S = vr_ragged_step(1.0); // 100 frames: 100 outputs
    struct { int64_t row[4]; int64_t jin, jout; const char *word; } rows[] = {
        {{0, 100, 0, 100}, 100, 100, nullptr}, {{0, 0, 0, 100}, 100, 100, nullptr}, {{0, 0, 0, 0}, 0, 0, nullptr}, {{5, 93, 7, 100}, 100, 200, nullptr},
        {{-1, 100, 0, 100}, 100, 100, "negative"}, {{0, -1, 0, 0}, 100, 100, "negative"}, {{0, 100, -8, 100}, 100, 100, "negative"},
        {{0, 100, 0, -1}, 100, 100, "negative"}, {{0, 101, 0, 101}, 100, 101, "exceed the job's"}, {{0, 100, 0, 100}, 100, 99, "exceed the job's"},
        {{0, 101, 0, 100}, 101, 100, "hipsoxr_plan_vr_out_len"}, {{0, 1, 0, 0}, 1, 0, "hipsoxr_plan_vr_out_len"},
        {{0, ((int64_t)1 << 30) + 1, 0, ((int64_t)1 << 30) + 1}, (int64_t)1 << 31, (int64_t)1 << 31, "2^30"},
        {{0, (int64_t)1 << 30, 0, (int64_t)1 << 30}, (int64_t)1 << 31, (int64_t)1 << 31, nullptr},
    };
    for (auto &t : rows) {
        const char *e = vr_adj_row_refusal(t.row, t.jin, t.jout, S);
        CHECK((e != nullptr) == (t.word != nullptr) && (!e || (std::strstr(e, t.word) && std::strstr(e, "variable-rate ragged adjoint: ") == e)),
              "row {%lld, %lld, %lld, %lld}: %s", (long long)t.row[0], (long long)t.row[1], (long long)t.row[2], (long long)t.row[3], e ? e : "admitted");
    }
    const int64_t half[4] = {0, 200, 0, 100};
    CHECK(!vr_adj_row_refusal(half, 200, 100, vr_ragged_step(0.5)) && vr_adj_row_refusal(half, 200, 100, vr_ragged_step(0.51)), "the row's own step counts");
}

int main()
{
    check_ranges();
    check_grid_and_rows();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
