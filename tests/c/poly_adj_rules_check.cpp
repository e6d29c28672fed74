// poly_adj_rules_check.cpp — the rules of the two-stage form's adjoint (python-soxr_amd/csrc/poly_adj_rules.h) against brute
// force: the closed-form bracket of outputs k that can reach a run of samples, against an enumeration of every k with its
// position taken BOTH ways — the exact rational floor(k Ms / Ls) and the kernels' truncated 64.64 step (poly_step_fx), which
// can put an integer position one sample lower; the staged-index range of a thread's run; the span bound; LDS bytes and
// admission; and the transposed plans of banks shaped like the FFT stage's (L/M = 2/1 and 1/2), read back entry for entry
// through plan.h's locate().  Stages: every (Ls, Ms) of the rate pairs of tests/test_gpu_adjoint_two_stage.py with every tap
// count, and small adversarial ones.  No device: links plan.cpp alone.  Exit status 0 = every check held
// (tests/test_poly_adj_rules.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "adjoint_fft_rules.h"
#include "plan.h"
#include "poly_adj_rules.h"

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

typedef __int128 i128;
typedef unsigned __int128 u128;
static int64_t floor_div128(i128 q, i128 d) { i128 n = q / d; return (int64_t)(n * d > q ? n - 1 : n); } // d > 0

static const int kTaps[10] = {8, 12, 16, 20, 24, 28, 32, 40, 48, 56};

// the kernels' own position of output k (k_poly's float32 path: poly_fx_origin and PolyPosFx of twostage.hip, restated)
struct KernelPos {
    int64_t nK0, Mq, k_lo;
    uint64_t phK0, step_fx;
    KernelPos(int64_t k_lo_, int64_t Ms, int64_t Ls) : Mq(Ms / Ls), k_lo(k_lo_), step_fx(poly_step_fx(Ms, Ls))
    {
        nK0 = floor_div128((i128)k_lo * Ms, Ls);
        phK0 = (uint64_t)((double)(k_lo * Ms - nK0 * Ls) * poly_fx_per_rem(Ls));
    }
    int64_t operator()(int64_t k) const
    {
        const uint64_t dk = (uint64_t)(k - k_lo), lo = dk * step_fx, ph = phK0 + lo;
        return nK0 + (int64_t)dk * Mq + (int64_t)(uint64_t)(((u128)dk * step_fx) >> 64) + (ph < lo ? 1 : 0);
    }
};

// k reaches a sample of [n_a, n_b] when 0 <= j = n - n_k + T2/2 - 1 < T2 for some n in it
static bool reaches(int64_t n_k, int64_t n_a, int64_t n_b, int T2) { return n_k + T2 / 2 >= n_a && n_k - T2 / 2 + 1 <= n_b; }

static long g_lower = 0; // positions the truncated step put one sample lower

// One tile [nA, nB] of a column whose stage outputs are [k_lo, k_lo + n_out): the bracket, the span bound, and every thread's run
static void check_tile(int T2, int64_t Ls, int64_t Ms, int64_t k_lo, int64_t n_out, int64_t nA, int64_t nB, int R, const char *what)
{
    const double ratio = (double)Ms / (double)Ls;
    const PolyAdjSpan sp = poly_adj_bracket(nA, nB, T2, Ls, Ms, k_lo, n_out);
    const int64_t cnt = sp.k_last - sp.k_first + 1;
    const int32_t span_max = poly_adj_span_max(poly_adj_tile(R), T2, ratio);
    CHECK(cnt <= span_max && span_max % 2 == 0, "%s: tile [%lld, %lld] stages %lld outputs, span_max %d", what, (long long)nA, (long long)nB, (long long)cnt, span_max);
    CHECK(cnt <= 0 || (sp.k_first >= k_lo && sp.k_last < k_lo + n_out), "%s: bracket [%lld, %lld] leaves the stage's outputs", what, (long long)sp.k_first, (long long)sp.k_last);
    // brute force: every k of the stage near the tile, both positions
    const KernelPos fx(k_lo, Ms, Ls);
    const int64_t guess = floor_div128((i128)nA * Ls, Ms), reach = (int64_t)((double)(nB - nA + 2 * T2 + 8) / ratio) + 8;
    const int64_t kb0 = std::max(k_lo, guess - reach), kb1 = std::min(k_lo + n_out - 1, guess + 2 * reach);
    std::vector<int64_t> ks, ne, nt;
    for (int64_t k = kb0; k <= kb1; ++k) {
        const int64_t n_exact = floor_div128((i128)k * Ms, Ls), n_trunc = fx(k);
        CHECK(n_trunc == n_exact || n_trunc == n_exact - 1, "%s: k %lld: truncated position %lld, exact %lld", what, (long long)k, (long long)n_trunc, (long long)n_exact);
        g_lower += n_trunc == n_exact - 1;
        const bool hit = reaches(n_exact, nA, nB, T2) || reaches(n_trunc, nA, nB, T2);
        if (hit) CHECK(k >= sp.k_first && k <= sp.k_last, "%s: k %lld reaches tile [%lld, %lld] outside the bracket [%lld, %lld]", what, (long long)k, (long long)nA, (long long)nB, (long long)sp.k_first, (long long)sp.k_last);
        if (k >= sp.k_first && k <= sp.k_last) { ks.push_back(k); ne.push_back(n_exact); nt.push_back(n_trunc); }
    }
    if (cnt <= 0) return;
    CHECK((int64_t)ks.size() == cnt, "%s: the enumeration missed part of the bracket (%zu of %lld)", what, ks.size(), (long long)cnt);
    // every thread's run: the staged indices that can reach it
    for (int t = 0; t < 256; ++t) {
        const int64_t n0 = nA + (int64_t)t * R, n1 = std::min(n0 + R - 1, nB);
        if (n0 > nB) break;
        int32_t sF = 0, sL = -1;
        poly_adj_run_span(n0, n1, T2, sp.k_first, Ls, Ms, (int32_t)cnt, &sF, &sL);
        CHECK(sF >= 0 && sL < cnt, "%s: run span [%d, %d] leaves the %lld staged outputs", what, sF, sL, (long long)cnt);
        for (size_t i = 0; i < ks.size(); ++i)
            if (reaches(ne[i], n0, n1, T2) || reaches(nt[i], n0, n1, T2))
                CHECK((int64_t)i >= sF && (int64_t)i <= sL, "%s: staged %zu (k %lld) reaches run [%lld, %lld] outside [%d, %d]", what, i, (long long)ks[i], (long long)n0, (long long)n1, sF, sL);
        // (the walk is short: no more than the run's own reach and the margins)
        CHECK(sL - sF + 1 <= (int32_t)((double)(n1 - n0 + T2 + 1) / ratio) + 5, "%s: run span [%d, %d] is longer than the reach allows", what, sF, sL);
    }
}

// A stage as the forward launches it, down (k_lo = -pad, samples [0, n)) and up (k_lo = 0, samples [-pad, n_core + pad))
static void check_stage(int T2, int64_t Ls, int64_t Ms, std::mt19937_64 &rng, const char *what)
{
    for (int up = 0; up < 2; ++up) {
        const int64_t n = 20000 + (int64_t)(rng() % 5000);
        const int64_t n_out_job = up ? (int64_t)((double)(2 * n) * (double)Ls / (double)Ms) : (int64_t)((double)n * (double)Ls / (double)Ms / 2.);
        if (n_out_job < 1 || n_out_job >= (1LL << 30)) continue;
        const TwoStageMid m = two_stage_mid(up != 0, T2, Ls, Ms, n, n_out_job, 1, false);
        const int64_t n_lo = up ? -m.pad : 0, n_src = up ? m.n_core + m.pad : n, k_lo = up ? 0 : -m.pad, n_out = up ? n_out_job : m.n_mid;
        for (int R = 1; R <= kPolyAdjRunMax; R *= 2) {
            const int64_t per = poly_adj_tile(R), tiles = poly_adj_tiles(n_src - n_lo, R);
            CHECK(tiles * per >= n_src - n_lo && (tiles - 1) * per < n_src - n_lo, "%s: %lld tiles of %lld", what, (long long)tiles, (long long)per);
            const int64_t pick[5] = {0, 1, tiles / 2, tiles - 2, tiles - 1};
            for (int64_t tile : pick) {
                if (tile < 0 || tile >= tiles) continue;
                const int64_t nA = n_lo + tile * per, nB = std::min(nA + per, n_src) - 1;
                check_tile(T2, Ls, Ms, k_lo, n_out, nA, nB, R, what);
            }
        }
    }
    // far into a long column (positions beyond 2^31 Ls / Ms outputs are not admitted: n < 2^30, the intermediate 2^31)
    {
        const int64_t n_src = (1LL << 31), n_out = std::min<int64_t>((1LL << 31) - 64, (int64_t)((double)n_src * (double)Ls / (double)Ms));
        const int64_t nA = (int64_t)((double)(n_out - 3000) * (double)Ms / (double)Ls) / 1024 * 1024;
        if (nA > 0) check_tile(T2, Ls, Ms, -64, n_out, nA, std::min(nA + 1024, n_src) - 1, 4, what);
    }
}

// ---- LDS and admission -----------------------------------------------------------------------------------------------------
static void check_admission(int T2, int64_t Ls, int64_t Ms, const char *what)
{
    for (size_t width = 4; width <= 8; width += 4) {
        const PolyStage s = poly_stage(T2, width == 4 ? 64 : 128, T2 + 1, Ls, Ms);
        const size_t tab = poly_tab_bytes(s.P, s.row, width);
        const int R = poly_adj_run(tab, T2, s.ratio, width);
        CHECK(R == 0 || R == 1 || R == 2 || R == 4, "%s: run %d", what, R);
        if (R) CHECK(poly_adj_lds_bytes(tab, R, T2, s.ratio, width) <= kPolyLdsMax, "%s: run %d takes %zu bytes", what, R, poly_adj_lds_bytes(tab, R, T2, s.ratio, width));
        for (int R2 = R ? 2 * R : 1; R2 <= kPolyAdjRunMax && R; R2 *= 2) // a longer run would not have fitted the budget that chose R
            CHECK(poly_adj_lds_bytes(tab, R2, T2, s.ratio, width) > (poly_adj_lds_bytes(tab, R, T2, s.ratio, width) <= kPolyAdjLdsTwo ? kPolyAdjLdsTwo : kPolyLdsMax),
                  "%s: run %d fits where %d was chosen", what, R2, R);
        const int64_t sizes[4] = {4000, 8192, 20000, (1LL << 30)};
        for (int64_t n_x : sizes)
            for (int64_t n_y : sizes)
                for (uint64_t cols : {(uint64_t)1, (uint64_t)65535, (uint64_t)65536}) {
                    const bool fwd = two_stage_admits(n_x, n_y, cols, width, s), adj = poly_adj_admits(n_x, n_y, cols, width, s);
                    CHECK(!adj || fwd, "%s: the adjoint admits a job the forward refuses", what);
                    CHECK(adj == (fwd && R > 0), "%s: admits %d, forward %d, run %d", what, (int)adj, (int)fwd, R);
                    if (adj) CHECK(poly_adj_lds_bytes(tab, R, T2, s.ratio, width) <= kPolyLdsMax, "%s: an admitted job's tile leaves LDS", what);
                }
    }
}

// ---- the transposed plan of an FFT-stage-shaped bank ---------------------------------------------------------------------
static double coef_forward(const Plan &p, int64_t a, int64_t k, int64_t *at)
{
    int64_t n0, ph;
    locate(p, k, &n0, &ph);
    const int64_t j = a - n0;
    *at = (j >= 0 && j < p.T) ? ph * p.T + j : -1;
    return *at >= 0 ? p.bank[(size_t)*at] : 0.0;
}
static void check_transposed(int64_t L, int64_t M, int32_t T)
{
    char what[64];
    std::snprintf(what, sizeof what, "bank L/M = %lld/%lld T = %d", (long long)L, (long long)M, T);
    Plan p;
    p.L = L; p.M = M; p.T = T;
    p.bank.resize((size_t)L * T);
    for (size_t i = 0; i < p.bank.size(); ++i) p.bank[i] = 1. + (double)i; // every entry its own value, none zero
    const int32_t Tt = adj_fft_taps(L, M, T);
    const std::vector<double> bt = adj_fft_bank(p);
    CHECK(Tt % 8 == 0 && (int64_t)bt.size() == M * Tt, "%s: T' %d, %zu entries", what, Tt, bt.size());
    Plan pt;
    pt.L = M; pt.M = L; pt.T = Tt;
    std::vector<int> met(p.bank.size(), 0);
    const int64_t a0 = M * ((Tt / 2 + 16) / L + 1);
    for (int64_t a = a0; a < a0 + 2 * M; ++a) {
        int64_t n0, s;
        locate(pt, a, &n0, &s);
        for (int64_t i = -8; i < Tt + 8; ++i) {
            int64_t at;
            const double want = coef_forward(p, a, n0 + i, &at);
            if (i < 0 || i >= Tt) { CHECK(at < 0, "%s: gx[%lld] <- gy[%lld] lies outside bank'", what, (long long)a, (long long)(n0 + i)); continue; }
            const double got = bt[(size_t)(s * Tt + i)];
            CHECK(got == want, "%s: bank'[%lld][%lld] = %g, the forward bank has %g", what, (long long)s, (long long)i, got, want);
            if (at >= 0 && a < a0 + M) ++met[(size_t)at];
        }
    }
    long wrong = 0;
    for (int c : met) wrong += c != 1;
    CHECK(wrong == 0, "%s: %ld forward coefficients are not met exactly once", what, wrong);
    std::printf("%s: T' = %d, %zu coefficients each met once\n", what, Tt, p.bank.size());
}

int main()
{
    std::mt19937_64 rng(20240607);
    // the polyphase stage's (Ls, Ms) of a rate pair: poly_design's reduction of M / (2 L) (down) or 2 M / L (up)
    struct Pair { double in_rate, out_rate; };
    static const Pair kPairs[] = {{48000, 44101}, {44101, 48000}, {44100, 16001}, {96000, 24001}, {8000, 44100.25}, {44100, 29401}, {48000, 47999}, {30000, 44101}, {44101, 11027}};
    for (const Pair &pr : kPairs) {
        int64_t L = 0, M = 0;
        const char *err = reduce_ratio(pr.in_rate, pr.out_rate, &L, &M);
        CHECK(!err, "%g -> %g: %s", pr.in_rate, pr.out_rate, err ? err : "");
        if (err) continue;
        const bool up = pr.out_rate > pr.in_rate;
        const int64_t a = up ? 2 * M : M, b = up ? L : 2 * L, g = std::gcd(a, b), Ms = a / g, Ls = b / g;
        char what[96];
        for (int T2 : kTaps) {
            std::snprintf(what, sizeof what, "%g -> %g (Ls %lld, Ms %lld) T2 %d", pr.in_rate, pr.out_rate, (long long)Ls, (long long)Ms, T2);
            check_stage(T2, Ls, Ms, rng, what);
            check_admission(T2, Ls, Ms, what);
        }
    }
    // adversarial stages: Ms a multiple of Ls (every position an integer: the truncated step's worst case is a remainder of
    // exactly 0 reached through a truncated fraction), Ls = 1, thirds, Ms / Ls just under 2 and just above 1/8
    static const int64_t kAdv[][2] = {{1, 1}, {1, 2}, {3, 3}, {3, 6}, {3, 1}, {3, 2}, {3, 4}, {7, 5}, {5, 9}, {1000001, 2000001}, {(1LL << 31) - 1, (1LL << 31)},
                                      {1000, 1999}, {8, 1}, {65537, 8193}, {(1LL << 31), (1LL << 31) - 1}, {6, 10}};
    for (const auto &lm : kAdv) {
        char what[96];
        for (int T2 : {8, 16, 56}) {
            std::snprintf(what, sizeof what, "adversarial Ls %lld Ms %lld T2 %d", (long long)lm[0], (long long)lm[1], T2);
            check_stage(T2, lm[0], lm[1], rng, what);
            check_admission(T2, lm[0], lm[1], what);
        }
    }
    CHECK(g_lower > 0, "no position was put one sample lower by the truncated step: the case the bracket's margin is for was not met");
    std::printf("%ld positions one sample lower by the truncated step\n", g_lower);
    // the FFT stage's banks: up 2/1 with the owner's taps, down 1/2 with its re-expressed taps, and a long down bank
    check_transposed(2, 1, 216);
    check_transposed(2, 1, 296);
    check_transposed(1, 2, 216);
    check_transposed(1, 2, 296);
    check_transposed(1, 2, 600);
    // the texts: each begins with the selector's name on the adjoint entry
    const PolyAdjAsk ok = {true, false, false, false, false};
    CHECK(poly_adj_refusal(ok) == nullptr, "a served job is refused");
    for (int f = 0; f < 5; ++f) {
        PolyAdjAsk q = ok;
        (f == 0 ? q.real : f == 1 ? q.vr : f == 2 ? q.exact_bank : f == 3 ? q.window : q.table) = f != 0;
        const char *t = poly_adj_refusal(q);
        CHECK(t && !std::strncmp(t, "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE", 45), "refusal %d: %s", f, t ? t : "(none)");
        if (f == 2) CHECK(t && std::strstr(t, "HIPSOXR_KERNEL_ADJOINT_FFT"), "the exact-bank refusal does not point to HIPSOXR_KERNEL_ADJOINT_FFT");
    }
    CHECK(!std::strncmp(kPolyAdjRaggedRefusal, "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE", 45) && std::strstr(kPolyAdjRaggedRefusal, "not served yet"), "ragged text");
    CHECK(!std::strncmp(kPolyAdjUnavailable, "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE", 45) && std::strstr(kPolyAdjUnavailable, "unavailable") &&
              std::strstr(kPolyAdjUnavailable, "HIPSOXR_KERNEL_ADJOINT runs the exact adjoint"), "unavailable text");
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
