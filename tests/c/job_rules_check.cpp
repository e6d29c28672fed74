// job_rules_check.cpp — the rules of the device-job dispatcher (python-soxr_amd/csrc/job_rules.h) against slow, independent
// statements of them: the fold's ranges against a transcription of the three loops launch_job had, covering every column
// once with no range above 65535 columns; the clip-row check against a brute-force predicate in both directions; the engine
// order as a truth table over selector x plan kind x element class x size x switches, written from the conditions
// launch_job spelled out on the raw selector values; job_wide_lane at its edges; the refusals' texts and order; a table and
// an equal-length job of equal totals under AUTO.  No device, no other source file but half_rules.h, whose AUTO rule must be
// this one.  Exit status 0 = every check held (tests/test_job_rules.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "half_rules.h"
#include "job_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

// the selector values of include/hipsoxr.h, restated (the header under test never sees them)
enum { AUTO = 0, GATHER = 1, TILE = 2, TILE_VALU = 3, TILE_MFMA = 4, FFT = 5, EXACT = 6, WAVE_DOT = 7, FFT_F64 = 8, FFT_PCM = 9, ADJOINT = 10 };
static JobSel sel_of(int k)
{
    JobSel s;
    s.want_fft = k == FFT || k == FFT_F64;
    s.want_pcm = k == FFT_PCM;
    s.is_auto = k == AUTO;
    s.exact_family = k == EXACT || k == GATHER;
    s.fft_f64 = k == FFT_F64;
    s.wave_dot = k == WAVE_DOT;
    return s;
}
static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

// ---- the fold ------------------------------------------------------------------------------------------------------------
struct Part { uint64_t clip0, n_clips, ch0, n_ch; };
// launch_job's three loops as they stood (counters widened to 64 bits: a 32-bit h0 += step could wrap at counts no buffer
// reaches), at most `limit` parts
static std::vector<Part> old_loops(uint32_t n_clips, uint32_t n_channels, size_t limit)
{
    std::vector<Part> v;
    if (n_channels == 1 || n_clips > 65535) {
        for (uint64_t c0 = 0; c0 < n_clips && v.size() < limit; c0 += 65535)
            v.push_back(Part{c0, std::min<uint64_t>(65535, n_clips - c0), 0, n_channels});
        return v;
    }
    const uint32_t step = 65535 / n_clips;
    for (uint64_t h0 = 0; h0 < n_channels && v.size() < limit; h0 += step)
        v.push_back(Part{0, n_clips, h0, std::min<uint64_t>(step, n_channels - h0)});
    return v;
}

static void check_fold_pair(uint32_t nc, uint32_t nh)
{
    const size_t kHead = 3000;
    const JobFold f = job_fold(nc, nh);
    const std::vector<Part> ref = old_loops(nc, nh, kHead);
    // order, ch0 and extents: the loops'
    for (size_t r = 0; r < ref.size(); ++r) {
        const JobRange g = job_fold_range(f, r);
        CHECK(g.clip0 == ref[r].clip0 && g.n_clips == ref[r].n_clips && g.ch0 == ref[r].ch0 && g.n_ch == ref[r].n_ch,
              "%u x %u range %zu: {%u %u %u %u}, the loops {%llu %llu %llu %llu}", nc, nh, r, g.clip0, g.n_clips, g.ch0, g.n_ch,
              (unsigned long long)ref[r].clip0, (unsigned long long)ref[r].n_clips, (unsigned long long)ref[r].ch0, (unsigned long long)ref[r].n_ch);
    }
    // every column exactly once: ranges along one axis, consecutive from 0 to its end, the other axis whole; counted
    // independently: ceil(n / per)
    const bool by_clip = nh == 1 || nc > 65535;
    const uint64_t n = by_clip ? nc : nh, per = by_clip ? 65535 : 65535 / nc, count = (n + per - 1) / per;
    auto check_at = [&](uint64_t r) {
        const JobRange g = job_fold_range(f, r);
        const uint64_t first = by_clip ? g.clip0 : g.ch0, len = by_clip ? g.n_clips : g.n_ch;
        CHECK(g.n_clips != 0 && g.n_ch != 0, "%u x %u: range %llu of %llu is empty", nc, nh, (unsigned long long)r, (unsigned long long)count);
        CHECK(first == r * per && len == std::min<uint64_t>(per, n - r * per), "%u x %u: range %llu starts at %llu with %llu", nc, nh, (unsigned long long)r,
              (unsigned long long)first, (unsigned long long)len);
        CHECK(by_clip ? (g.ch0 == 0 && g.n_ch == nh) : (g.clip0 == 0 && g.n_clips == nc), "%u x %u: range %llu cuts the other axis", nc, nh, (unsigned long long)r);
        // no launch above 65535 columns: a range of clips that keeps several channels re-enters and folds over channels
        const uint64_t cols = (uint64_t)g.n_clips * g.n_ch;
        if (cols > 65535) {
            CHECK(by_clip && nh > 1, "%u x %u: range %llu holds %llu columns", nc, nh, (unsigned long long)r, (unsigned long long)cols);
            const JobFold f2 = job_fold(g.n_clips, g.n_ch);
            const JobRange g2 = job_fold_range(f2, 0);
            CHECK(!f2.by_clip && (uint64_t)g2.n_clips * g2.n_ch <= 65535 && g2.n_ch >= 1, "%u x %u: the second fold", nc, nh);
        }
    };
    for (uint64_t r = 0; r < count && r < kHead; ++r) check_at(r);
    for (uint64_t k = 1; k <= 64 && k <= count; ++k) check_at(count - k);
    for (uint64_t r : {count, count + 1, (uint64_t)1 << 32, (uint64_t)1 << 48, (uint64_t)1 << 63, ~(uint64_t)0})
        CHECK(job_fold_range(f, r).n_clips == 0, "%u x %u: range %llu behind the last", nc, nh, (unsigned long long)r);
}

static void check_fold()
{
    const uint32_t edges[] = {1, 2, 3, 4, 5, 7, 255, 256, 257, 21844, 21845, 21846, 32767, 32768, 65534, 65535, 65536, 65537, 70000, 131069, 131070, 131071,
                              196605, 196606, 0x7fffffffu, 0x80000000u, 0xfffefffeu, 0xfffeffffu, 0xffff0000u, 0xffff0001u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t nc : edges)
        for (uint32_t nh : edges) check_fold_pair(nc, nh);
    // the cases launch_job meets in tests: 65536 channels, 21846 x 3, 65536 x 2, both wide
    const JobFold a = job_fold(1, 65536);
    CHECK(!a.by_clip && a.step == 65535 && job_fold_range(a, 1).ch0 == 65535 && job_fold_range(a, 1).n_ch == 1, "1 x 65536");
    const JobFold b = job_fold(21846, 3);
    CHECK(!b.by_clip && b.step == 2 && job_fold_range(b, 1).ch0 == 2 && job_fold_range(b, 1).n_ch == 1 && job_fold_range(b, 2).n_clips == 0, "21846 x 3");
    const JobFold c = job_fold(65536, 2);
    CHECK(c.by_clip && job_fold_range(c, 0).n_clips == 65535 && job_fold_range(c, 0).n_ch == 2 && job_fold_range(c, 1).clip0 == 65535 && job_fold_range(c, 1).n_clips == 1, "65536 x 2");
    CHECK(job_fold(70000, 70000).by_clip && !job_fold(65535, 70000).by_clip && job_fold(65535, 70000).step == 1, "70000 x 70000");
    CHECK(kJobMaxCols == 65535 && kHalfMaxCols == 65535, "the column limit");
}

// ---- clip rows -----------------------------------------------------------------------------------------------------------
static uint64_t len_rule(uint64_t n) { return (n * 147 + 159) / 160; } // some plan's output length: monotone, 0 for 0
static void check_rows()
{
    const int64_t job_in = 1000, job_out = 919; // (919 = len_rule(1000))
    CHECK(kRaggedRow == 4, "row width");
    std::vector<int64_t> offs = {-5, -1, 0, 1, 77, (int64_t)1 << 40}, ins, outs;
    for (int64_t v : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)160, (int64_t)161, job_in - 1, job_in, job_in + 1, (int64_t)918, (int64_t)919, (int64_t)920,
                      (int64_t)1088, (int64_t)1089, (int64_t)1 << 40, INT64_MIN, INT64_MAX}) {
        ins.push_back(v);
        outs.push_back(v);
    }
    for (int64_t v = 140; v <= 150; ++v) { ins.push_back(v); outs.push_back(v); } // around len_rule(160) = 147 and its inverse
    for (int dir = 0; dir < 2; ++dir)
        for (int64_t o0 : offs)
            for (int64_t o2 : offs)
                for (int64_t n1 : ins)
                    for (int64_t n3 : outs) {
                        const int64_t row[kRaggedRow] = {o0, n1, o2, n3};
                        // brute force: the three statements, each over every field it speaks of
                        bool neg = false;
                        for (int i = 0; i < 4; ++i) neg = neg || row[i] < 0;
                        const bool above_job = n1 > job_in || n3 > job_out;
                        JobRowFault want = neg ? kJobRowNegative : above_job ? kJobRowAboveJob : kJobRowOk;
                        CHECK(job_row_bounds(row, job_in, job_out) == want, "bounds of {%lld %lld %lld %lld}", (long long)o0, (long long)n1, (long long)o2, (long long)n3);
                        if (want == kJobRowOk) {
                            // forward: the clip's outputs are at most what its inputs yield; adjoint: the cotangent (in) is at
                            // most what the gradient's length (out) yields
                            const bool fits = dir == 0 ? (uint64_t)n3 <= len_rule((uint64_t)n1) : (uint64_t)n1 <= len_rule((uint64_t)n3);
                            if (!fits) want = kJobRowAbovePlan;
                        }
                        const JobRowFault got = job_row_check(row, job_in, job_out, dir == 0 ? kJobRowForward : kJobRowAdjoint, len_rule);
                        CHECK(got == want, "dir %d row {%lld %lld %lld %lld}: %d, brute force %d", dir, (long long)o0, (long long)n1, (long long)o2, (long long)n3, (int)got, (int)want);
                    }
}

// ---- engines -------------------------------------------------------------------------------------------------------------
static void check_engines()
{
    CHECK(kJobAutoFftMin == 8192 && kHalfAutoFftMin == kJobAutoFftMin, "the AUTO threshold");
    const int64_t totals[] = {0, 1, 8191, 8192, 8193, (int64_t)1 << 40};
    for (int k = 0; k <= ADJOINT; ++k)
        for (int phases = 0; phases < 2; ++phases)
            for (int el = 0; el < 4; ++el)
                for (int64_t total : totals)
                    for (int no_fft = 0; no_fft < 2; ++no_fft)
                        for (int no_two = 0; no_two < 2; ++no_two) {
                            const JobSel s = sel_of(k);
                            const JobElem e = (JobElem)el;
                            const bool is_float = e == kJobElemFloat, big = total >= (1 << 13);
                            // launch_job's table branch, on the raw values
                            const bool t_want_fft = k == FFT || k == FFT_F64 || k == FFT_PCM;
                            const bool t_try = t_want_fft || (k == AUTO && big && !no_fft);
                            // ... its plain branch (the FFT_PCM block behind it launches unconditionally)
                            const bool p_want_fft = k == FFT || k == FFT_F64;
                            const bool p_try = (p_want_fft || k == AUTO) && (p_want_fft || (big && !no_fft));
                            CHECK(job_try_fft(s, total, no_fft) == t_try, "try_fft k %d total %lld no_fft %d", k, (long long)total, no_fft);
                            if (k != FFT_PCM) CHECK(job_try_fft(s, total, no_fft) == p_try, "try_fft (plain) k %d total %lld no_fft %d", k, (long long)total, no_fft);
                            // two-stage: the table's owner (launch_ragged_job and the table branch), the equal-length gate
                            const bool t_two = phases && k == AUTO && is_float && !no_fft && !no_two;
                            const bool p_two = phases && (p_want_fft || (k == AUTO && !no_fft)) && is_float && !no_two;
                            CHECK(job_two_stage_table(phases, s, e, no_fft, no_two) == t_two, "two_stage_table k %d ph %d el %d %d %d", k, phases, el, no_fft, no_two);
                            CHECK(job_two_stage(phases, s, e, no_fft, no_two) == p_two, "two_stage k %d ph %d el %d %d %d", k, phases, el, no_fft, no_two);
                            // a half job's AUTO rule is this one
                            if (k == AUTO || k == FFT)
                                CHECK(half_wants_fft(k == FFT ? kHalfSelFft : kHalfSelAuto, total, no_fft) == job_try_fft(s, total, no_fft), "half k %d total %lld", k, (long long)total);
                        }
    // a table and an equal-length job of equal totals get the same AUTO answer: both hand the rule one number
    for (int no_fft = 0; no_fft < 2; ++no_fft)
        for (int64_t total = 8180; total <= 8200; ++total) {
            const int64_t rows[3] = {total / 2, total - total / 2 - 5, 5}; // three clips of one channel ...
            const int64_t table_total = (rows[0] + rows[1] + rows[2]) * 1;
            const bool even = total % 2 == 0;
            const int64_t plain_total = even ? (total / 2) * 1 * 2 : total; // ... against frames x clips x channels
            CHECK(job_try_fft(sel_of(AUTO), table_total, no_fft) == job_try_fft(sel_of(AUTO), plain_total, no_fft), "total %lld", (long long)total);
            CHECK(job_auto_fft(total, no_fft) == (total >= 8192 && !no_fft), "auto_fft %lld", (long long)total);
        }
}

// ---- job_wide_lane ---------------------------------------------------------------------------------------------------------
static void check_wide_lane()
{
    struct Shape { uint32_t clips, ch; };
    const Shape shapes[] = {{1, 65535}, {1, 65536}, {2, 32768}, {3, 21846}, {65535, 2}, {65536, 1}, {65536, 2}, {70000, 70000}, {1, 1u << 20}, {1, 524288}, {1, 524289}};
    const int64_t outs[] = {1, 4094, 4095, 4096, 4097, 2048};
    for (const Shape &sh : shapes)
        for (int64_t out : outs)
            for (int phases = 0; phases < 2; ++phases)
                for (int vr_or_res = 0; vr_or_res < 2; ++vr_or_res)
                    for (int64_t cs : {(int64_t)1, (int64_t)2, (int64_t)0})
                        for (int k = 0; k <= ADJOINT; ++k) {
                            const uint64_t cols = (uint64_t)sh.clips * sh.ch;
                            // the predicate as launch_job had it, on raw values
                            const bool want = cols > 65535 && phases && !vr_or_res && sh.clips <= 65535 && cs == 1 && out <= 4095 &&
                                              out * (int64_t)sh.ch < ((int64_t)1 << 31) && (k == AUTO || k == EXACT || k == GATHER);
                            CHECK(job_wide_lane(cols, phases, vr_or_res, sh.clips, cs, out, sh.ch, sel_of(k)) == want, "wide_lane %u x %u out %lld ph %d vr %d cs %lld k %d",
                                  sh.clips, sh.ch, (long long)out, phases, vr_or_res, (long long)cs, k);
                        }
    // (2^31 / 4095 = 524416.1: one channel either side)
    CHECK(job_wide_lane(524416, true, false, 1, 1, 4095, 524416, sel_of(AUTO)) && !job_wide_lane(524417, true, false, 1, 1, 4095, 524417, sel_of(AUTO)), "the 2^31 edge");
    CHECK(job_wide_lane(1u << 19, true, false, 1, 1, 4095, 1u << 19, sel_of(EXACT)) && !job_wide_lane(1u << 19, true, false, 1, 1, 4096, 1u << 19, sel_of(EXACT)), "kWideLaneMaxOut");
}

// ---- refusals --------------------------------------------------------------------------------------------------------------
static void check_refusals()
{
    const char *whole = "FFT engine: whole-signal device jobs only";
    const char *pcm_elem = "HIPSOXR_KERNEL_FFT_PCM serves int16 / int32 jobs (float jobs have HIPSOXR_KERNEL_FFT / HIPSOXR_KERNEL_FFT_F64)";
    const char *half_stream = "float16 / bfloat16 samples: device jobs only (streams take float32, float64, int32 and int16)";
    const char *half_f64 = "HIPSOXR_KERNEL_FFT_F64 serves float32 / float64 jobs (float16 / bfloat16 jobs compute in float32: HIPSOXR_KERNEL_FFT)";
    const char *half_wd = "HIPSOXR_KERNEL_WAVE_DOT serves float32, float64, int32 and int16 jobs (float16 / bfloat16 jobs are not served by the reference-point kernel)";
    const char *table_stream = "ragged batches: constant-rate device jobs only";
    const char *table_window = "ragged batches: whole signals only (in_abs0 == 0, out_k0 == 0)";
    CHECK(same(kJobPcmIneligible, "FFT engine (integer samples) needs a whole-signal job (in_abs0 == 0, out_k0 == 0) on an HQ/VHQ exact-ratio plan"), "pcm window text");
    CHECK(job_empty(0, 1, 1) && job_empty(-1, 1, 1) && job_empty(1, 0, 1) && job_empty(1, 1, 0) && !job_empty(1, 1, 1), "empty");
    CHECK(same(job_empty_refusal(true), "resident kernel: empty job") && !job_empty_refusal(false), "empty text");
    CHECK(same(job_resident_refusal(true, 65536), "resident kernel: too many columns") && !job_resident_refusal(true, 65535) && !job_resident_refusal(false, 65536), "resident");
    for (int k = 0; k <= ADJOINT; ++k)
        for (int el = 0; el < 4; ++el)
            for (int vr = 0; vr < 2; ++vr) {
                const JobSel s = sel_of(k);
                const JobElem e = (JobElem)el;
                const char *pcm = k != FFT_PCM ? nullptr : vr ? whole : e != kJobElemPcm ? pcm_elem : nullptr;
                CHECK(same(job_pcm_refusal(s, e, vr), pcm), "pcm k %d el %d vr %d", k, el, vr);
                const char *half = e != kJobElemHalf ? nullptr : vr ? half_stream : k == FFT_F64 ? half_f64 : k == WAVE_DOT ? half_wd : nullptr;
                CHECK(same(job_half_refusal(s, e, vr), half), "half k %d el %d vr %d", k, el, vr);
                CHECK(same(job_fft_stream_refusal(s, vr), (k == FFT || k == FFT_F64) && vr ? whole : nullptr), "fft on a stream k %d vr %d", k, vr);
            }
    for (int table = 0; table < 2; ++table)
        for (int vr = 0; vr < 2; ++vr)
            for (int64_t a : {(int64_t)0, (int64_t)1, (int64_t)-1})
                for (int64_t b : {(int64_t)0, (int64_t)7})
                    CHECK(same(job_table_refusal(table, vr, a, b), !table ? nullptr : vr ? table_stream : (a || b) ? table_window : nullptr), "table %d vr %d %lld %lld", table, vr,
                          (long long)a, (long long)b);
}

int main()
{
    check_fold();
    check_rows();
    check_engines();
    check_wide_lane();
    check_refusals();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
