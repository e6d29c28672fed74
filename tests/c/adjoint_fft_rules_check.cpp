// adjoint_fft_rules_check.cpp — the host rules of the adjoint on the frequency-domain engine
// (python-soxr_amd/csrc/adjoint_fft_rules.h) against slow, independent statements of them: every entry of the transposed
// bank read back against the forward bank through plan.h's locate(), every forward coefficient met exactly once; the tap
// count — a multiple of 8, and 8 fewer would lose a coefficient; the imaginary part of the transposed plan's frequency
// response against the forward plan's, by one and the same code (the paired kernels multiply by Re H alone); the refusals,
// texts and order, against the conditions written out on raw values.  No device: links plan.cpp alone.
// Exit status 0 = every check held (tests/test_adjoint_fft_rules.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adjoint_fft_rules.h"
#include "adjoint_rules.h" // adj_entry_refusal: the other selectors' answers, which this selector must not change
#include "plan.h"

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

static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

enum { HQ = 4, VHQ = 6 }; // include/soxr.h's recipes, restated

// the rate pairs of tests/test_gpu_adjoint.py CASES that are HQ or VHQ ...
struct Case { double in_rate, out_rate; int recipe; };
static const Case kCases[] = {{48000, 44100, VHQ}, {48000, 44100, HQ}, {44100, 48000, VHQ}, {44100, 48000, HQ}, {2, 1, HQ}, {44100, 16000, VHQ}, {16000, 44100, HQ}};
// ... and every (L, M) of fft.hip's fft_pairs with the periods per block of its full-size row (out/in = L/M), restated
struct Row { int64_t L, M; int k; };
static const Row kRows[] = {{147, 160, 32}, {160, 147, 32}, {160, 441, 16}, {441, 160, 16}, {1, 2, 2048}, {2, 1, 2048}, {1, 3, 1792}, {3, 1, 1792},
                            {2, 3, 1792}, {3, 2, 1792}, {1, 4, 1280}, {4, 1, 1280}, {1, 6, 896}, {6, 1, 896}, {320, 441, 16}, {441, 320, 16},
                            {80, 147, 32}, {147, 80, 32}, {147, 320, 16}, {320, 147, 16}, {80, 441, 16}, {441, 80, 16}, {147, 640, 8}, {640, 147, 8},
                            {640, 441, 8}, {441, 640, 8}, {40, 147, 32}, {147, 40, 32}, {4, 3, 1280}, {3, 4, 1280}};
static int row_k(int64_t L, int64_t M)
{
    for (const Row &r : kRows)
        if (r.L == L && r.M == M) return r.k;
    return 0;
}

// ---- the transposed bank -------------------------------------------------------------------------------------------------
// gx[a] <- gy[k] by the forward plan: bank[p_k][a - n0_k] where 0 <= a - n0_k < T, else 0 (locate())
static double coef_forward(const Plan &p, int64_t a, int64_t k, int64_t *at)
{
    int64_t n0, ph;
    locate(p, k, &n0, &ph);
    const int64_t j = a - n0;
    *at = (j >= 0 && j < p.T) ? ph * p.T + j : -1;
    return *at >= 0 ? p.bank[(size_t)*at] : 0.0;
}

static void check_bank(const Plan &p, const char *what)
{
    const int64_t L = p.L, M = p.M;
    const int32_t Tt = adj_fft_taps(L, M, p.T);
    const std::vector<double> bt = adj_fft_bank(p);
    CHECK(Tt % 8 == 0 && Tt >= 8 && (int64_t)bt.size() == M * Tt, "%s: T' %d, %zu entries", what, Tt, bt.size());
    // pt as a plan of its own: output a of pt (phase s = (a L) mod M, first tap at n0) multiplies its input k — the
    // cotangent sample gy[k] — by bank'[s][k - n0]
    Plan pt;
    pt.L = M; pt.M = L; pt.T = Tt;
    std::vector<int> met(p.bank.size(), 0);
    // one period of pt's outputs and one more, far enough from 0 that no tap reaches a negative k (locate() truncates):
    // a in [a0, a0 + 2 M) meets every phase; each forward coefficient is counted in the first period alone
    const int64_t a0 = M * ((Tt / 2 + 16) / L + 1);
    for (int64_t a = a0; a < a0 + 2 * M; ++a) {
        int64_t n0, s;
        locate(pt, a, &n0, &s);
        for (int64_t i = 0; i < Tt; ++i) {
            int64_t at;
            const double want = coef_forward(p, a, n0 + i, &at), got = bt[(size_t)(s * Tt + i)];
            CHECK(got == want, "%s: bank'[%ld][%ld] = %.17g, the forward bank has %.17g for gx[%ld] <- gy[%ld]", what, (long)s, (long)i, got, want, (long)a, (long)(n0 + i));
            if (at >= 0 && a < a0 + M) ++met[(size_t)at];
        }
        // ... and nothing of the forward's support lies outside the T' taps: 8 either side
        for (int64_t i = -8; i < Tt + 8; ++i) {
            if (i >= 0 && i < Tt) continue;
            int64_t at;
            (void)coef_forward(p, a, n0 + i, &at);
            CHECK(at < 0, "%s: gx[%ld] <- gy[%ld] has a forward coefficient outside bank' (tap %ld of %d)", what, (long)a, (long)(n0 + i), (long)i, Tt);
        }
    }
    long wrong = 0;
    for (int c : met) wrong += c != 1;
    CHECK(wrong == 0, "%s: %ld forward coefficients are not met exactly once", what, wrong);
    // T' - 8 would lose a coefficient: with 4 taps fewer at either end some output's support sticks out
    {
        Plan ps;
        ps.L = M; ps.M = L; ps.T = Tt - 8;
        bool lost = false;
        for (int64_t a = a0; a < a0 + M && !lost && ps.T > 0; ++a) {
            int64_t n0, s, at;
            locate(ps, a, &n0, &s);
            (void)coef_forward(p, a, n0 - 1, &at); lost = lost || at >= 0;
            (void)coef_forward(p, a, n0 + ps.T, &at); lost = lost || at >= 0;
        }
        CHECK(lost || Tt == 8, "%s: T' - 8 = %d taps would hold the whole support", what, Tt - 8);
    }
}

// ---- Im H ------------------------------------------------------------------------------------------------------------------
// max |Im H[q]| / max |Re H[q]| over 16 bins spread over [0, min(A, B)] of a block of k periods — fft.hip fft_build's H,
//     H[q] = sum_p sum_j bank[p][j] exp(-2 pi i q (L (T/2 - 1 - j) + p) / (L N_in)),
// with every angle reduced in integers first.
static double im_over_re(int64_t L, int64_t M, int32_t T, const double *bank, int k)
{
    const int64_t N_in = M * k, N_out = L * k, qmax = std::min(N_in, N_out) / 2, period = L * N_in;
    double re_max = 0., im_max = 0.;
    for (int n = 0; n < 16; ++n) {
        const int64_t q = qmax * n / 15;
        double hr = 0., hi = 0.;
        for (int64_t ph = 0; ph < L; ++ph)
            for (int64_t j = 0; j < T; ++j) {
                const int64_t u = L * (T / 2 - 1 - j) + ph;
                const int64_t m = (int64_t)(((__int128)q * u) % period);
                const double ang = -6.283185307179586476925286766559 * (double)m / (double)period, b = bank[(size_t)(ph * T + j)];
                hr += b * std::cos(ang); hi += b * std::sin(ang);
            }
        re_max = std::max(re_max, std::fabs(hr)); im_max = std::max(im_max, std::fabs(hi));
    }
    return im_max / re_max;
}

static void check_plan(double in_rate, double out_rate, int recipe, const char *what)
{
    Plan p;
    const char *err = plan_design(in_rate, out_rate, (unsigned long)recipe, &p);
    CHECK(!err && p.phases == 0, "%s: %s", what, err ? err : "an interpolated-phase plan");
    if (err || p.phases) return;
    check_bank(p, what);
    const int kf = row_k(p.L, p.M), kt = row_k(p.M, p.L);
    CHECK(kf && kt, "%s: L = %ld M = %ld is not in the restated table in both directions", what, (long)p.L, (long)p.M);
    if (!kf || !kt) return;
    const std::vector<double> bt = adj_fft_bank(p);
    const int32_t Tt = adj_fft_taps(p.L, p.M, p.T);
    const double fwd = im_over_re(p.L, p.M, p.T, p.bank.data(), kf), tr = im_over_re(p.M, p.L, Tt, bt.data(), kt);
    std::printf("%s: L %ld M %ld T %d -> T' %d   Im H / max Re H: forward %.3g, transposed %.3g\n", what, (long)p.L, (long)p.M, p.T, Tt, fwd, tr);
    CHECK(tr <= 10. * fwd, "%s: Im H' / max Re H' = %.3g, above 10 x the forward's %.3g", what, tr, fwd);
}

// ---- refusals --------------------------------------------------------------------------------------------------------------
// the list as the issue states it, on raw values
static const char *slow_refusal(bool ragged, int elem, bool vr, bool phases, double att_db, int64_t in_abs0, int64_t out_k0, bool table)
{
    const bool half = elem == 4 || elem == 5, real = elem == 0 || elem == 1; // hipsoxr_elem_t: F32 F64 I32 I16 F16 BF16
    if (ragged && half) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: ragged: float16 / bfloat16 clip tables are not served (half cotangents clip by clip through hipsoxr_run_device_adjoint)";
    if (!real) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT serves float32 or float64 elements (integer types have no gradient)";
    if (vr) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: variable-rate plans are not served";
    if (phases) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT needs an exact-bank plan (interpolated-phase plans are served by HIPSOXR_KERNEL_ADJOINT, on the exact engine)";
    if (att_db < 120.) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: the frequency-domain engine serves HQ and VHQ only (recipes below 120 dB are not 1e-6-class on it)";
    if (in_abs0 || out_k0) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: whole cotangents only (in_abs0 == 0, out_k0 == 0)";
    if (!ragged && table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: a clip_table is served by hipsoxr_run_device_adjoint_ragged, not by this entry";
    if (ragged && !table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: the ragged entry needs a clip_table (equal-length clips: hipsoxr_run_device_adjoint)";
    return nullptr;
}

static void check_refusals()
{
    const double atts[] = {0., 104., 119.9, 120., 128., 177.};
    const int64_t wins[][2] = {{0, 0}, {1, 0}, {0, 7}, {-3, 2}};
    long served = 0;
    for (int ragged = 0; ragged < 2; ++ragged)
        for (int elem = 0; elem < 6; ++elem)
            for (int kind = 0; kind < 3; ++kind) // exact bank, interpolated phases, variable rate (always interpolated)
                for (double att : atts)
                    for (const auto &w : wins)
                        for (int table = 0; table < 2; ++table) {
                            const bool vr = kind == 2, phases = kind != 0, half = elem == 4 || elem == 5;
                            // (the equal-length entry widens a half job and asks for the float32 one)
                            AdjFftAsk q;
                            q.half = half; q.real = elem == 0 || elem == 1 || (!ragged && half);
                            q.vr = vr; q.phases = phases; q.below_hq = att < kAdjFftMinAttDb;
                            q.window = w[0] != 0 || w[1] != 0; q.table = table != 0;
                            const char *got = adj_fft_refusal(ragged != 0, q);
                            const char *want = slow_refusal(ragged != 0, (!ragged && half) ? 0 : elem, vr, phases, att, w[0], w[1], table != 0);
                            CHECK(same(got, want), "ragged %d elem %d kind %d att %g window %ld %ld table %d: '%s', expected '%s'", ragged, elem, kind, att,
                                  (long)w[0], (long)w[1], table, got ? got : "(served)", want ? want : "(served)");
                            CHECK(!got || std::strstr(got, "HIPSOXR_KERNEL_ADJOINT_FFT"), "a refusal that does not name the selector: %s", got);
                            served += !got;
                            // the selectors the entries had keep their answers, and none of them names this one
                            for (int sel = 0; sel < 3; ++sel) { // AUTO / EXACT, ADJOINT, another
                                AdjAsk o;
                                o.half = half; o.real = q.real; o.by_name = sel == 1; o.auto_or_exact = sel == 0;
                                o.vr = vr; o.phases = phases; o.window = q.window; o.table = q.table;
                                const char *t = adj_entry_refusal(ragged ? kAdjRagged : kAdjEqual, o);
                                CHECK(!t || !std::strstr(t, "ADJOINT_FFT"), "adj_entry_refusal names the new selector: %s", t);
                                CHECK(sel != 2 || t, "another selector is served");
                            }
                        }
    // served: float32 / float64 (equal lengths: and the two half types), exact bank, 120 dB and above, no window, the entry's table rule
    CHECK(served == (2 + 4) * 3, "%ld combinations served", served);
    CHECK(std::strstr(kAdjFftUnavailable, "unavailable for this plan or layout") && std::strstr(kAdjFftUnavailable, "HIPSOXR_KERNEL_ADJOINT_FFT"), "the engine's no");
    CHECK(std::strstr(kAdjFftForwardRefusal, "HIPSOXR_KERNEL_ADJOINT_FFT") && std::strstr(kAdjFftForwardRefusal, "hipsoxr_run_device_adjoint"), "the forward entries' no");
}

int main()
{
    // the issue's own figures for T'
    CHECK(adj_fft_taps(147, 160, 296) == 272 && adj_fft_taps(160, 147, 272) == 304 && adj_fft_taps(160, 441, 536) == 200 && adj_fft_taps(2, 1, 200) == 408 &&
          adj_fft_taps(441, 160, 272) == 752, "T' of the five reference plans");
    char what[96];
    for (const Case &c : kCases) {
        std::snprintf(what, sizeof what, "%g -> %g recipe %d", c.in_rate, c.out_rate, c.recipe);
        check_plan(c.in_rate, c.out_rate, c.recipe, what);
    }
    for (const Row &r : kRows)
        for (int recipe : {HQ, VHQ}) {
            std::snprintf(what, sizeof what, "row L %ld M %ld recipe %d", (long)r.L, (long)r.M, recipe);
            check_plan((double)r.M, (double)r.L, recipe, what);
        }
    check_refusals();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
