// vr_ragged_rules_check.cpp — the rules of a ragged variable-rate launch (python-soxr_amd/csrc/vr_ragged_rules.h) against the
// stream layer's own (stream_rules.h: vr_k_limit on a constant-step clock) and against tables written by hand.  No device:
// links plan.cpp alone.  Every (n_in, step, count) it compares is printed as a line "LEN n_in step_hi step_lo count", which
// tests/test_vr_ragged_rules.py checks once more in Python integers.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "plan.h"
#include "stream_rules.h"
#include "vr_ragged_rules.h"

using namespace hipsoxr;

namespace hipsoxr {
Plan::~Plan() {} // (the library's destructor releases device tables: there are none here)
}

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

static void one_length(const Plan &p, uint64_t n_in, u128 step)
{
    VrState v;
    v.on = true; v.t_s = 0; v.s0 = v.s1 = (i128)step; v.n_slew = 0; v.delta = 0; v.k_s = 0;
    const uint64_t want = vr_k_limit(p, v, n_in, 0, true), got = vr_const_out_len(n_in, step);
    CHECK(got == want, "n_in=%llu step=%llu:%llu: %llu, the stream's limit %llu", (unsigned long long)n_in, (unsigned long long)(uint64_t)(step >> 64),
          (unsigned long long)(uint64_t)step, (unsigned long long)got, (unsigned long long)want);
    std::printf("LEN %llu %llu %llu %llu\n", (unsigned long long)n_in, (unsigned long long)(uint64_t)(step >> 64), (unsigned long long)(uint64_t)step,
                (unsigned long long)got);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL; // fixed seed
static uint64_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

static void check_lengths()
{
    Plan p;
    const char *e = plan_design(17600., 16000., /*HQ*/ 4, &p, /*force_interp=*/true);
    CHECK(!e && p.phases > 0 && p.T >= 8, "variable-rate plan 17600 -> 16000: %s", e ? e : "ok");
    if (e) return;
    const uint64_t H = (uint64_t)p.T / 2;
    const uint64_t lens[7] = {0, 1, H - 1, H, H + 1, 1000, ((uint64_t)1 << 31) + 7};
    const double ratios[8] = {std::ldexp(1., -19), 0.5, 0.9070294784580499, 1.0, 1.1, 1.1 * (1. - std::ldexp(1., -40)), 3.0, std::ldexp(1., 19)};
    for (uint64_t n : lens)
        for (double r : ratios) one_length(p, n, vr_ragged_step(r));
    CHECK(vr_ragged_step(1.0) == ((u128)1 << 64) && vr_ragged_step(0.5) == ((u128)1 << 63), "the step of 1.0 and of 0.5");
    CHECK(vr_ragged_step(1.1) == (u128)q64(1.1), "the step is set_io_ratio's q64");
    for (uint64_t n : lens) CHECK(vr_const_out_len(n, 0) == 0 && vr_const_out_len(n, 1) == 0, "a step below 2 has no outputs");
    CHECK(vr_const_out_len(0, vr_ragged_step(1.0)) == 0, "no input, no output");
    // exact halves: n S + S/2 <= n_in 2^64 at S = 2^64 holds for k <= n_in - 1: n_in outputs
    CHECK(vr_const_out_len(1000, (u128)1 << 64) == 1000, "step 1.0: one output per input");
    CHECK(vr_const_out_len(1000, (u128)1 << 63) == 2000, "step 0.5: two outputs per input");
    CHECK(vr_const_out_len(1000, (u128)3 << 64) == 333, "step 3.0: k 3 + 1.5 <= 1000 for k <= 332");
    for (int i = 0; i < 4000; ++i) { // random pairs: lengths up to 2^33, steps between 2^-19 and 2^19 at every scale
        const int nsh = 31 + (int)(rnd() % 33);
        const uint64_t n = rnd() >> nsh;
        const int sh = (int)(rnd() % 38); // step < 2^(83 - sh) >= 2^45
        const uint64_t hi = rnd() & 0x7FFFF, lo = rnd();
        u128 step = (((u128)hi << 64) | lo) >> sh;
        if (step < ((u128)1 << 45)) step |= (u128)1 << 45;
        one_length(p, n, step);
    }
}

static void check_max_step()
{
    const uint64_t one[2] = {1, 0};
    CHECK(vr_ragged_max_step(one, 1) == 1. * (1. + 1e-9), "one clip at 1.0");
    const uint64_t three[6] = {0, (uint64_t)1 << 63, 1, (uint64_t)1 << 62, 0, ~(uint64_t)0}; // 0.5, 1.25, just below 1
    CHECK(vr_ragged_max_step(three, 3) == 1.25 * (1. + 1e-9), "the largest of 0.5, 1.25 and 1 - 2^-64");
    CHECK(vr_ragged_max_step(three, 1) == 0.5 * (1. + 1e-9), "a range of the table: its own largest");
    CHECK(vr_ragged_max_step(three + 4, 1) >= 1. - 1e-15 && vr_ragged_max_step(three + 4, 1) <= 1. + 2e-9, "just below 1");
    CHECK(vr_ragged_max_step(three, 0) == 0., "no clips");
    // never below the step itself: what a span is sized by covers every clip's
    for (int i = 0; i < 1000; ++i) {
        const uint64_t ck[2] = {rnd() & 0xFFFFF, rnd()};
        const double m = vr_ragged_max_step(ck, 1);
        const long double exact = (long double)ck[0] + (long double)ck[1] / 18446744073709551616.L;
        CHECK((long double)m >= exact, "max step %g below the step %Lg", m, exact);
    }
}

static void check_refusals()
{
    const double max_io = 1.1;
    struct { double r; bool refused; const char *word; } ratios[] = {
        {1.1, false, ""}, {1.0, false, ""}, {0.5, false, ""}, {1.1 * (1. + 0.5e-12), false, ""}, {1.1 * (1. + 4e-12), true, "exceeds the maximum"},
        {1.2, true, "exceeds the maximum"}, {std::ldexp(1., -20), true, "out of range"}, {std::ldexp(1., -19), false, ""}, {0., true, "out of range"},
        {-1., true, "out of range"}, {std::nan(""), true, "out of range"}, {std::ldexp(1., 20), true, "out of range"},
    };
    for (auto &t : ratios) {
        const char *e = vr_ragged_ratio_refusal(t.r, max_io);
        CHECK((e != nullptr) == t.refused && (!e || std::strstr(e, t.word)), "ratio %g: %s", t.r, e ? e : "admitted");
    }
    CHECK(std::strcmp(vr_ragged_ratio_refusal(1.2, 1.1), "io ratio exceeds the maximum given at creation (the filter would alias)") == 0,
          "set_io_ratio's own words");
    const u128 S = vr_ragged_step(1.0); // 100 frames in: 100 out
    struct { int64_t row[4]; int64_t jin, jout; const char *word; } rows[] = {
        {{0, 100, 0, 100}, 100, 100, nullptr}, {{0, 100, 0, 0}, 100, 100, nullptr}, {{0, 0, 0, 0}, 0, 0, nullptr}, {{5, 100, 7, 99}, 200, 100, nullptr},
        {{-1, 100, 0, 100}, 100, 100, "negative"}, {{0, -1, 0, 0}, 100, 100, "negative"}, {{0, 100, -8, 100}, 100, 100, "negative"},
        {{0, 100, 0, -1}, 100, 100, "negative"}, {{0, 101, 0, 100}, 100, 100, "exceed the job's"}, {{0, 100, 0, 100}, 100, 99, "exceed the job's"},
        {{0, 100, 0, 101}, 100, 101, "hipsoxr_plan_vr_out_len"}, {{0, 0, 0, 1}, 0, 1, "hipsoxr_plan_vr_out_len"},
        {{0, ((int64_t)1 << 30) + 1, 0, ((int64_t)1 << 30) + 1}, (int64_t)1 << 31, (int64_t)1 << 31, "2^30"},
        {{0, (int64_t)1 << 30, 0, (int64_t)1 << 30}, (int64_t)1 << 31, (int64_t)1 << 31, nullptr},
    };
    for (auto &t : rows) {
        const char *e = vr_ragged_row_refusal(t.row, t.jin, t.jout, S);
        CHECK((e != nullptr) == (t.word != nullptr) && (!e || std::strstr(e, t.word)), "row {%lld, %lld, %lld, %lld}: %s", (long long)t.row[0],
              (long long)t.row[1], (long long)t.row[2], (long long)t.row[3], e ? e : "admitted");
    }
    const int64_t half[4] = {0, 100, 0, 200};
    CHECK(!vr_ragged_row_refusal(half, 100, 200, vr_ragged_step(0.5)) && vr_ragged_row_refusal(half, 100, 200, vr_ragged_step(0.51)), "the row's own step counts");
}

int main()
{
    check_lengths();
    check_max_step();
    check_refusals();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
