// stream_rules_check.cpp — the stream layer's pure rules (python-soxr_amd/csrc/stream_rules.h) against slow, independent
// statements of them.  No device: links plan.cpp alone.  Exit status 0 = every check held (tests/test_stream_rules.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"
#include "stream_rules.h"

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

static int64_t gcd(int64_t a, int64_t b) { return b ? gcd(b, a % b) : a; }

// ---- k_avail: the count of k >= 0 with floor(k M / L) + T/2 <= N - 1 (the condition is monotonic in k) ----
static uint64_t k_avail_slow(int64_t L, int64_t M, int32_t T, int64_t N)
{
    uint64_t k = 0;
    while ((int64_t)k * M / L + T / 2 <= N - 1) ++k;
    return k;
}

static void check_k_avail()
{
    Plan p;
    const int32_t taps[3] = {2, 8, 30};
    for (int64_t L = 1; L <= 12; ++L)
        for (int64_t M = 1; M <= 12; ++M) {
            if (gcd(L, M) != 1) continue;
            for (int32_t T : taps)
                for (int64_t N = 0; N <= 200; ++N) {
                    p.L = L; p.M = M; p.T = T;
                    const uint64_t got = k_avail(p, (uint64_t)N), want = k_avail_slow(L, M, T, N);
                    CHECK(got == want, "k_avail L=%ld M=%ld T=%d N=%ld: %lu, brute force %lu", (long)L, (long)M, T, (long)N, (unsigned long)got, (unsigned long)want);
                }
        }
    // the product's ratios at the tap counts their designs have
    const double rates[4][2] = {{44100, 48000}, {48000, 44100}, {44100, 16000}, {16000, 48000}};
    const int64_t lm[4][2] = {{160, 147}, {147, 160}, {160, 441}, {3, 1}};
    for (int r = 0; r < 4; ++r) {
        Plan q;
        const char *e = plan_design(rates[r][0], rates[r][1], /*HQ*/ 4, &q);
        CHECK(!e && q.L == lm[r][0] && q.M == lm[r][1] && q.phases == 0, "plan %g -> %g: %s L=%ld M=%ld", rates[r][0], rates[r][1], e ? e : "ok", (long)q.L, (long)q.M);
        if (e) continue;
        for (int64_t N = 0; N <= 3000; ++N) {
            const uint64_t got = k_avail(q, (uint64_t)N), want = k_avail_slow(q.L, q.M, q.T, N);
            CHECK(got == want, "k_avail %ld/%ld T=%d N=%ld: %lu, brute force %lu", (long)q.L, (long)q.M, q.T, (long)N, (unsigned long)got, (unsigned long)want);
        }
    }
}

// ---- ring_keep ----
static void check_ring_keep()
{
    const int64_t bases[5] = {0, -37, 3, 1000, (int64_t)1 << 40}; // (the frequency-domain origin can be negative)
    for (int64_t in_base : bases)
        for (int64_t in_fill = 0; in_fill <= 20; ++in_fill)
            for (int64_t fn = in_base - 5; fn <= in_base + in_fill + 5; ++fn) {
                const RingKeep k = ring_keep(fn, in_base, (size_t)in_fill);
                CHECK(in_base <= k.keep_from && k.keep_from <= in_base + in_fill, "keep_from %ld outside [%ld, %ld]", (long)k.keep_from, (long)in_base, (long)(in_base + in_fill));
                if (fn >= in_base && fn <= in_base + in_fill) CHECK(k.keep_from == fn, "keep_from %ld, first needed %ld lies inside", (long)k.keep_from, (long)fn);
                CHECK((int64_t)(k.drop + k.keep) == in_fill, "drop %zu + keep %zu != fill %ld", k.drop, k.keep, (long)in_fill);
                CHECK((int64_t)k.drop == k.keep_from - in_base, "drop %zu, keep_from - base %ld", k.drop, (long)(k.keep_from - in_base));
            }
}

// ---- ring_grow / ring_grow_bounded: start value times a power of two, the smallest that is enough ----
static void check_grown(size_t cap, size_t in_cap, size_t need, const char *what)
{
    const size_t start = in_cap > 1024 ? in_cap : 1024;
    CHECK(cap >= in_cap, "%s: cap %zu below in_cap %zu", what, cap, in_cap);
    CHECK(cap % start == 0 && ((cap / start) & (cap / start - 1)) == 0, "%s: cap %zu is no power of two times %zu", what, cap, start);
    CHECK(cap >= need, "%s: cap %zu < need %zu", what, cap, need);
    CHECK(cap == start || cap / 2 < need, "%s: cap %zu is not the smallest (need %zu, start %zu)", what, cap, need, start);
}

static void check_ring_grow()
{
    const size_t caps[] = {0, 1, 1000, 1024, 1025, 3000, 4096, 100000, (size_t)1 << 24, ((size_t)1 << 24) + 7, (size_t)3 << 23};
    const size_t keeps[] = {0, 1, 37, 1023, 1024, 5000, 1 << 20, ((size_t)1 << 24) - 1000, (size_t)1 << 24, ((size_t)1 << 24) + 5, (size_t)1 << 26};
    const size_t ilens[] = {1, 7, 441, 4410, 20000, 1 << 20, 5 << 20};
    const size_t factors[] = {1, 4, 8, 16};
    for (size_t in_cap : caps)
        for (size_t keep : keeps)
            for (size_t ilen : ilens)
                for (size_t f : factors) {
                    const size_t room = f * ilen;
                    check_grown(ring_grow(in_cap, keep, room), in_cap, keep + room, "ring_grow"); // (no fallback, however large)
                    const size_t need = keep + room > ((size_t)1 << 24) ? keep + ilen : keep + room;
                    check_grown(ring_grow_bounded(in_cap, keep, room, ilen), in_cap, need, "ring_grow_bounded");
                }
}

// ---- emit_count, constant rate ----
static void check_emit_count_constant()
{
    Plan p;
    const int64_t lm[5][2] = {{160, 147}, {147, 160}, {2, 3}, {3, 1}, {1, 7}};
    const size_t olens[] = {0, 1, 64, 100, 441, (size_t)-1};
    for (auto &r : lm)
        for (int32_t T : {2, 8, 30}) {
            p.L = r[0]; p.M = r[1]; p.T = T;
            for (uint64_t N = 0; N <= 600; N += (N < 40 ? 1 : 13)) {
                const uint64_t avail = k_avail_slow(p.L, p.M, p.T, (int64_t)N), total = plan_out_len(p, N);
                for (uint64_t k_done = 0; k_done <= avail + 2; k_done += (k_done < 5 ? 1 : 17))
                    for (size_t olen : olens) {
                        const uint64_t due = avail > k_done ? avail - k_done : 0, due_end = total > k_done ? total - k_done : 0;
                        VrState off;
                        CHECK(emit_count(p, N, k_done, false, olen) == (size_t)(due < olen ? due : olen), "emit_count N=%lu k_done=%lu olen=%zu", (unsigned long)N, (unsigned long)k_done, olen);
                        CHECK(emit_count(p, N, k_done, true, olen) == (size_t)(due_end < olen ? due_end : olen), "emit_count (ended) N=%lu k_done=%lu olen=%zu", (unsigned long)N, (unsigned long)k_done, olen);
                        CHECK(emit_count(p, off, N, k_done, false, olen) == emit_count(p, N, k_done, false, olen) && !off.on && off.n_slew == 0, "emit_count with a clock that is off");
                    }
            }
        }
}

// ---- emit_count, variable rate: against a walk of the clock, one output at a time, in 128-bit integers ----
struct Walk {          // the clock at output k (the next one to emit)
    uint64_t k = 0;
    i128 t = 0, step = 0, delta = 0, s1 = 0;
    uint64_t n = 0, n_slew = 0; // outputs since the last change of ratio, of which the first n_slew slew

    void advance() { t += step; ++n; step = n < n_slew ? step + delta : s1; ++k; }
    void set_io_ratio(double ratio, uint64_t slew_len)
    {
        const i128 s_new = q64(ratio);
        s1 = s_new; n = 0; n_slew = slew_len;
        if (slew_len) delta = (s_new - step) / (i128)slew_len; else { step = s_new; delta = 0; }
    }
    bool ok(uint64_t n_in, int64_t H, bool ended) const
    {
        if (ended) return t + step / 2 <= ((i128)n_in << 64);
        return (int64_t)(t >> 64) + H <= (int64_t)n_in - 1;
    }
};
// what hipsoxr_stream_set_io_ratio does to the stream's VrState
static void state_set_io_ratio(VrState &v, uint64_t k_done, double ratio, uint64_t slew_len)
{
    const i128 t_now = v.pos(k_done), s_now = v.step(k_done), s_new = q64(ratio);
    v.k_s = k_done; v.t_s = t_now; v.s1 = s_new;
    if (slew_len > 0) { v.s0 = s_now; v.n_slew = slew_len; v.delta = (s_new - s_now) / (i128)slew_len; }
    else { v.s0 = s_new; v.n_slew = 0; v.delta = 0; }
}

struct VrEvent { int call; double ratio; uint64_t slew_len; }; // before call `call`: set_io_ratio
// expect_crossed: a call stops at the end of a slew and makes another pass; expect_exact_end: a pass begins exactly there
struct VrCase { const char *name; double io0; size_t ilen, olen; int calls; std::vector<VrEvent> events; bool expect_crossed, expect_exact_end; };

static void run_vr_case(const VrCase &c)
{
    Plan p;
    p.T = 16; p.phases = 64;
    const int64_t H = p.T / 2;
    VrState v;
    v.on = true; v.max_io = c.io0; v.s0 = v.s1 = q64(c.io0);
    Walk w;
    w.step = w.s1 = q64(c.io0);
    uint64_t n_in = 0, k_done = 0;
    bool crossed = false, exact_end = false;
    for (int call = 0; call <= c.calls; ++call) {
        const bool ended = call == c.calls; // the last call is the flush
        for (const VrEvent &e : c.events)
            if (e.call == call) { state_set_io_ratio(v, k_done, e.ratio, e.slew_len); w.set_io_ratio(e.ratio, e.slew_len); }
        if (!ended) n_in += c.ilen;
        for (int pass = 0; pass < 4; ++pass) { // (emit_passes: another pass only where one stopped at the end of a slew)
            // expected: walk until an output is not computable, olen is reached, or the slew ends
            Walk probe = w;
            const bool slewing = w.n < w.n_slew;
            const uint64_t slew_left = slewing ? w.n_slew - w.n : 0;
            size_t want = 0;
            while (want < c.olen && probe.ok(n_in, H, ended) && !(slewing && want == slew_left)) { probe.advance(); ++want; }
            const VrState before = v;
            const size_t n = emit_count(p, v, n_in, k_done, ended, c.olen);
            CHECK(n == want, "%s: call %d pass %d: emit_count %zu, the walk says %zu (k_done %lu)", c.name, call, pass, n, want, (unsigned long)k_done);
            if (before.n_slew && k_done < before.k_s + before.n_slew)
                CHECK(k_done + n <= before.k_s + before.n_slew, "%s: call %d crosses the end of the slew", c.name, call);
            if (before.n_slew && k_done == before.k_s + before.n_slew) { exact_end = true; CHECK(v.n_slew == 0 && v.k_s == k_done, "%s: no renormalisation at the end of a slew", c.name); }
            for (uint64_t k = k_done; k < k_done + 300; k += (k < k_done + 70 ? 1 : 23)) // the renormalised state: the same clock
                CHECK(v.pos(k) == before.pos(k) && v.step(k) == before.step(k), "%s: call %d: the state after emit_count has another clock at k=%lu", c.name, call, (unsigned long)k);
            // the clock of the launch against the walk: position and step at k_done, increment while the slew lasts
            const VrPos vp = vr_pos_at(v, k_done);
            const i128 d = w.n < w.n_slew ? w.delta : 0;
            CHECK(vp.t_hi == (uint64_t)((u128)w.t >> 64) && vp.t_lo == (uint64_t)(u128)w.t && vp.s_hi == (uint64_t)((u128)w.step >> 64) && vp.s_lo == (uint64_t)(u128)w.step &&
                  vp.d_hi == (uint64_t)((u128)d >> 64) && vp.d_lo == (uint64_t)(u128)d, "%s: call %d pass %d: vr_pos_at differs from the walk", c.name, call, pass);
            for (size_t i = 0; i < n; ++i) w.advance();
            k_done += n;
            CHECK(v.pos(k_done) == w.t && v.step(k_done) == w.step, "%s: call %d: VrState::pos / step differ from the walk at k=%lu", c.name, call, (unsigned long)k_done);
            if (!n || !slew_just_ended(v, k_done)) break;
            crossed = true;
        }
    }
    CHECK(k_done > 0, "%s: nothing was emitted", c.name);
    CHECK(crossed == c.expect_crossed, "%s: a call %s the end of a slew", c.name, crossed ? "stopped at" : "never stopped at");
    CHECK(exact_end == c.expect_exact_end, "%s: %s pass began exactly at the end of a slew", c.name, exact_end ? "a" : "no");
    std::printf("  %-28s %lu outputs from %lu frames%s%s\n", c.name, (unsigned long)k_done, (unsigned long)n_in, crossed ? ", a call crossed a slew end" : "", exact_end ? ", a call began at a slew end" : "");
}

// ---- the same scripts on a stream whose clock was moved (engine.cpp debug_stream_seek: k_s = out, t_s = in 2^64, the step
// untouched; counters n_in_total = in, k_done = out), side by side with the fresh one: the same counts in every pass, the
// limit moved by `out`, the launch's clock with a high word larger by `in` and nothing else changed — through every
// set_io_ratio, slew and renormalisation of the script ----
static void run_vr_case_moved(const VrCase &c, uint64_t in, uint64_t out)
{
    Plan p;
    p.T = 16; p.phases = 64;
    VrState v, m;
    v.on = true; v.max_io = c.io0; v.s0 = v.s1 = q64(c.io0);
    m = v; m.k_s = out; m.t_s = (i128)((u128)in << 64);
    uint64_t n_in = 0, k_done = 0;
    for (int call = 0; call <= c.calls; ++call) {
        const bool ended = call == c.calls;
        for (const VrEvent &e : c.events)
            if (e.call == call) { state_set_io_ratio(v, k_done, e.ratio, e.slew_len); state_set_io_ratio(m, k_done + out, e.ratio, e.slew_len); }
        if (!ended) n_in += c.ilen;
        for (int pass = 0; pass < 4; ++pass) {
            CHECK(vr_k_limit(p, m, n_in + in, k_done + out, ended) == vr_k_limit(p, v, n_in, k_done, ended) + out, "%s moved by (%lu, %lu): call %d: vr_k_limit", c.name,
                  (unsigned long)in, (unsigned long)out, call);
            const size_t n = emit_count(p, v, n_in, k_done, ended, c.olen), nm = emit_count(p, m, n_in + in, k_done + out, ended, c.olen);
            CHECK(n == nm, "%s moved by (%lu, %lu): call %d pass %d: emit_count %zu, fresh %zu", c.name, (unsigned long)in, (unsigned long)out, call, pass, nm, n);
            CHECK(m.k_s == v.k_s + out && m.n_slew == v.n_slew && m.t_s == v.t_s + (i128)((u128)in << 64) && m.s0 == v.s0 && m.s1 == v.s1 && m.delta == v.delta,
                  "%s moved by (%lu, %lu): call %d: the state is not the fresh one moved", c.name, (unsigned long)in, (unsigned long)out, call);
            for (uint64_t k : {k_done, k_done + n / 2, k_done + n}) {
                const VrPos a = vr_pos_at(v, k), b = vr_pos_at(m, k + out);
                CHECK(b.t_hi == a.t_hi + in && b.t_lo == a.t_lo && b.s_hi == a.s_hi && b.s_lo == a.s_lo && b.d_hi == a.d_hi && b.d_lo == a.d_lo,
                      "%s moved by (%lu, %lu): call %d: vr_pos_at at k=%lu", c.name, (unsigned long)in, (unsigned long)out, call, (unsigned long)k);
            }
            k_done += n;
            if (!n || !slew_just_ended(v, k_done)) break;
        }
    }
    CHECK(k_done > 0, "%s moved: nothing was emitted", c.name);
}

static void check_emit_count_vr()
{
    const std::vector<VrCase> cases = {
        {"constant", 1.5, 441, 1000, 6, {}, false, false},
        {"slew crossed inside a call", 1.5, 441, 1000, 8, {{3, 1.2, 50}}, true, true},
        {"slew ends exactly at k_done", 2.0, 400, 100, 12, {{2, 1.0, 100}}, true, true}, // olen = the slew's length: the call ends where it does
        {"slew_len 1", 1.5, 441, 1000, 6, {{2, 0.75, 1}, {4, 1.5, 1}}, true, true},
        {"step change, no slew", 1.5, 441, 64, 10, {{3, 0.5, 0}, {5, 1.5, 0}}, false, false},
        {"ratio changed inside a slew", 1.0, 300, 120, 10, {{2, 0.7, 500}, {4, 1.0, 50}}, true, true},
        {"long slew, small olen", 0.9, 441, 37, 30, {{1, 0.45, 333}}, true, true},
    };
    for (const VrCase &c : cases) run_vr_case(c);
    // any integer pair is a legal clock: outputs that cross 2^31 and 2^32 inside the script, inputs that cross 2^32 while
    // the outputs do not, both above 2^40, below 2^48, above 2^50
    const uint64_t moves[6][2] = {{((uint64_t)1 << 31) + 12345, ((uint64_t)1 << 31) - 700}, {((uint64_t)1 << 32) + 99, ((uint64_t)1 << 32) - 333},
                                  {((uint64_t)1 << 32) - 500, ((uint64_t)1 << 31) + 1000003}, {((uint64_t)1 << 40) + 7, ((uint64_t)1 << 40) + 1000003},
                                  {((uint64_t)1 << 48) - 40000, ((uint64_t)1 << 48) - 30000}, {((uint64_t)1 << 50) + 1000003, ((uint64_t)1 << 50) + 17}};
    for (const VrCase &c : cases)
        for (auto &mv : moves) run_vr_case_moved(c, mv[0], mv[1]);
}

// ---- the constant-rate rules at the counts of a stream that has run for hours or years: n_in_total, k_done and in_base
// around 2^31, 2^32, 2^40 and 2^50.  A walk from zero is out of reach there, so each rule is held against its DEFINING
// property, stated in 128-bit integers: the condition of k_avail is monotonic in k, so K is its value iff it holds at
// K - 1 and fails at K; locate's (n0, p) are the quotient and remainder of k M by L; the stream's length is
// floor(N L / M + 1/2).
static bool computable(int64_t L, int64_t M, int32_t T, i128 k, i128 N) { return k >= 0 && k * M / L + T / 2 <= N - 1; }
static uint64_t k_avail_big(int64_t L, int64_t M, int32_t T, uint64_t N)
{
    i128 k = ((i128)N * L) / M; // an estimate: within T/2 L/M + 2 of the answer, which the two loops then walk to
    while (k > 0 && !computable(L, M, T, k - 1, (i128)N)) --k;
    while (computable(L, M, T, k, (i128)N)) ++k;
    return (uint64_t)k;
}
static uint64_t out_len_big(int64_t L, int64_t M, uint64_t N) { return (uint64_t)((2 * (i128)N * L + M) / (2 * (i128)M)); }

static const int64_t kBigLM[7][2] = {{160, 147}, {147, 160}, {160, 441}, {2, 3}, {3, 1}, {1, 7}, {4800037, 4410000}};
static const uint64_t kBigAt[4] = {(uint64_t)1 << 31, (uint64_t)1 << 32, (uint64_t)1 << 40, (uint64_t)1 << 50};

static void check_large_counts()
{
    Plan p;
    const size_t olens[] = {0, 1, 441, (size_t)-1};
    for (auto &r : kBigLM)
        for (int32_t T : {2, 30, 736}) {
            p.L = r[0]; p.M = r[1]; p.T = T;
            for (uint64_t at : kBigAt)
                for (int64_t dn = -400; dn <= 400; dn += (dn >= -4 && dn < 4 ? 1 : 99)) {
                    // ---- k_avail and the stream's length with n_in_total around the power of two ----
                    const uint64_t N = at + (uint64_t)dn;
                    const uint64_t avail = k_avail(p, N), total = plan_out_len(p, N);
                    CHECK(computable(p.L, p.M, T, (i128)avail - 1, (i128)N) && !computable(p.L, p.M, T, (i128)avail, (i128)N),
                          "k_avail %ld/%ld T=%d N=%lu: %lu is not where the condition ends", (long)p.L, (long)p.M, T, (unsigned long)N, (unsigned long)avail);
                    CHECK(avail == k_avail_big(p.L, p.M, T, N), "k_avail %ld/%ld T=%d N=%lu: %lu, walked %lu", (long)p.L, (long)p.M, T, (unsigned long)N,
                          (unsigned long)avail, (unsigned long)k_avail_big(p.L, p.M, T, N));
                    CHECK(total == out_len_big(p.L, p.M, N), "plan_out_len %ld/%ld N=%lu: %lu, in 128 bits %lu", (long)p.L, (long)p.M, (unsigned long)N,
                          (unsigned long)total, (unsigned long)out_len_big(p.L, p.M, N));
                    // ---- emit_count with k_done a few outputs either side of what is due ----
                    for (int64_t dk : {-100000, -442, -441, -440, -1, 0, 1, 5}) {
                        for (int ended = 0; ended < 2; ++ended) {
                            const uint64_t k_end = ended ? out_len_big(p.L, p.M, N) : k_avail_big(p.L, p.M, T, N);
                            if ((int64_t)k_end + dk < 0) continue;
                            const uint64_t k_done = k_end + (uint64_t)dk;
                            const uint64_t due = k_end > k_done ? k_end - k_done : 0;
                            for (size_t olen : olens)
                                CHECK(emit_count(p, N, k_done, ended != 0, olen) == (size_t)(due < olen ? due : olen), "emit_count %ld/%ld T=%d N=%lu k_done=%lu ended=%d olen=%zu",
                                      (long)p.L, (long)p.M, T, (unsigned long)N, (unsigned long)k_done, ended, olen);
                        }
                    }
                }
            // ---- k_avail with the RESULT around the power of two (ratios far from 1: N is then elsewhere) ----
            for (uint64_t at : kBigAt) {
                const uint64_t N0 = (uint64_t)(((i128)at * p.M) / p.L) + (uint64_t)(T / 2);
                for (uint64_t N = N0 - 3; N <= N0 + 3; ++N) {
                    const uint64_t avail = k_avail(p, N);
                    CHECK(computable(p.L, p.M, T, (i128)avail - 1, (i128)N) && !computable(p.L, p.M, T, (i128)avail, (i128)N),
                          "k_avail %ld/%ld T=%d N=%lu (result near %lu): %lu", (long)p.L, (long)p.M, T, (unsigned long)N, (unsigned long)at, (unsigned long)avail);
                }
            }
            // ---- locate with k around the power of two: k M = L (n0 + T/2 - 1) + p, 0 <= p < L; consecutive outputs ----
            for (uint64_t at : kBigAt) {
                int64_t n0_prev = 0, ph_prev = 0;
                for (int64_t dk = -5; dk <= 5; ++dk) {
                    const int64_t k = (int64_t)at + dk;
                    int64_t n0 = 0, ph = 0;
                    locate(p, k, &n0, &ph);
                    const i128 q = (i128)n0 + (T / 2 - 1);
                    CHECK(ph >= 0 && ph < p.L && q * p.L + ph == (i128)k * p.M, "locate %ld/%ld T=%d k=%ld: n0=%ld p=%ld", (long)p.L, (long)p.M, T, (long)k, (long)n0, (long)ph);
                    if (dk > -5) { // the step from k - 1: the phase moves by M, the window by the carries
                        const int64_t carry = (ph_prev + p.M) / p.L;
                        CHECK(ph == (ph_prev + p.M) % p.L && n0 == n0_prev + carry, "locate %ld/%ld k=%ld: no step of M from k - 1", (long)p.L, (long)p.M, (long)k);
                    }
                    n0_prev = n0; ph_prev = ph;
                }
            }
        }
    // ---- ring_keep with the ring's base (and with it first_needed) around the powers of two: a ring that straddles one ----
    for (uint64_t at : kBigAt)
        for (int64_t in_base = (int64_t)at - 12; in_base <= (int64_t)at + 2; in_base += 7)
            for (int64_t in_fill = 0; in_fill <= 20; in_fill += 5)
                for (int64_t fn = in_base - 3; fn <= in_base + in_fill + 3; ++fn) {
                    const RingKeep k = ring_keep(fn, in_base, (size_t)in_fill);
                    const int64_t want = fn < in_base ? in_base : fn > in_base + in_fill ? in_base + in_fill : fn;
                    CHECK(k.keep_from == want && (int64_t)k.drop == want - in_base && (int64_t)k.keep == in_base + in_fill - want,
                          "ring_keep first_needed=%ld base=%ld fill=%ld: keep_from %ld drop %zu keep %zu", (long)fn, (long)in_base, (long)in_fill, (long)k.keep_from, k.drop, k.keep);
                }
    // ---- the chain the stream walks (engine.cpp first_needed -> ring_keep -> the job's in_abs0): a stream that has emitted
    // k_done outputs from n_in_total frames keeps the ring from locate(k_done)'s n0 on, and every output still due from the
    // input so far has its whole window [n0, n0 + T) inside [keep_from, n_in_total) ----
    for (auto &r : kBigLM) {
        p.L = r[0]; p.M = r[1]; p.T = 30;
        for (uint64_t at : kBigAt)
            for (int64_t back : {1, 441, 4410}) {
                const uint64_t N = at + 17, k_end = k_avail(p, N);
                if (k_end < (uint64_t)back) continue;
                const uint64_t k_done = k_end - (uint64_t)back;
                int64_t n0 = 0, ph = 0, n0_last = 0;
                locate(p, (int64_t)k_done, &n0, &ph);
                locate(p, (int64_t)k_end - 1, &n0_last, &ph);
                const int64_t in_base = n0 - 100;
                const RingKeep k = ring_keep(n0, in_base, (size_t)((int64_t)N - in_base));
                CHECK(k.keep_from == n0 && k.drop == 100 && (int64_t)k.keep == (int64_t)N - n0, "ring_keep in a stream at N=%lu", (unsigned long)N);
                CHECK(n0_last + p.T <= (int64_t)N && n0_last >= n0, "%ld/%ld N=%lu: the last output due reads [%ld, %ld), the ring holds [%ld, %lu)", (long)p.L, (long)p.M,
                      (unsigned long)N, (long)n0_last, (long)(n0_last + p.T), (long)n0, (unsigned long)N);
                CHECK(emit_count(p, N, k_done, false, (size_t)-1) == (size_t)back, "emit_count in a stream at N=%lu", (unsigned long)N);
            }
    }
}

// ---- the translation property (engine.cpp debug_stream_seek; tests/test_gpu_stream_positions.py rests on it): a
// constant-rate stream whose counters were moved by q whole periods — n_in_total, in_base by q M, k_done by q L — is the
// fresh stream moved: the same counts per call from N = 0 on (the start-up transient, where nothing is due yet, included),
// the same phases, windows and ring cuts moved by q M, the same frequency-domain blocks relative to the ring.  Exact integers;
// q puts the counts around 2^31, 2^32, 2^40, 2^48 and 2^50. ----
static const uint64_t kMoveAt[5] = {(uint64_t)1 << 31, (uint64_t)1 << 32, (uint64_t)1 << 40, (uint64_t)1 << 48, (uint64_t)1 << 50};

static void check_translation()
{
    Plan p;
    const size_t olens[] = {0, 1, 441, (size_t)-1};
    long moved = 0;
    for (auto &r : kBigLM)
        for (int32_t T : {2, 30, 736}) {
            p.L = r[0]; p.M = r[1]; p.T = T;
            for (uint64_t at : kMoveAt)
                for (int side = 0; side < 2; ++side) { // the outputs at the power of two, or the inputs
                    const uint64_t q = at / (uint64_t)(side ? p.M : p.L) - (side ? 0 : 1);
                    const uint64_t dN = q * (uint64_t)p.M, dk = q * (uint64_t)p.L;
                    if ((dN | dk) >> 62) continue;
                    ++moved;
                    // emit_count: N through the transient N <= T/2 and beyond; k_done around what is due and what the stream holds
                    std::vector<uint64_t> Ns;
                    for (uint64_t N = 0; N <= (uint64_t)T / 2 + 3; ++N) Ns.push_back(N);
                    for (uint64_t N : {441u, 4410u, 100003u}) Ns.push_back(N);
                    for (uint64_t N : Ns) {
                        const uint64_t avail = k_avail_big(p.L, p.M, T, N), total = out_len_big(p.L, p.M, N);
                        for (uint64_t k : {(uint64_t)0, (uint64_t)1, avail > 441 ? avail - 441 : 0, avail > 0 ? avail - 1 : 0, avail, avail + 1, total, total + 2})
                            for (int ended = 0; ended < 2; ++ended)
                                for (size_t olen : olens) {
                                    const size_t fresh = emit_count(p, N, k, ended != 0, olen);
                                    CHECK(emit_count(p, N + dN, k + dk, ended != 0, olen) == fresh, "emit_count %ld/%ld T=%d N=%lu k=%lu ended=%d olen=%zu moved by %lu periods: %zu, fresh %zu",
                                          (long)p.L, (long)p.M, T, (unsigned long)N, (unsigned long)k, ended, olen, (unsigned long)q, emit_count(p, N + dN, k + dk, ended != 0, olen), fresh);
                                }
                    }
                    // locate, the retire rule on what first_needed returns, and the frequency-domain block origin
                    for (uint64_t k = 0; k < 3 * (uint64_t)p.L + 700; k += (k < 40 ? 1 : (uint64_t)p.L / 3 + 17)) {
                        int64_t n0 = 0, ph = 0, n0m = 0, phm = 0;
                        locate(p, (int64_t)k, &n0, &ph);
                        locate(p, (int64_t)(k + dk), &n0m, &phm);
                        CHECK(n0m == n0 + (int64_t)dN && phm == ph, "locate %ld/%ld T=%d k=%lu moved by %lu periods: (%ld, %ld), fresh (%ld, %ld)", (long)p.L, (long)p.M, T,
                              (unsigned long)k, (unsigned long)q, (long)n0m, (long)phm, (long)n0, (long)ph);
                        for (int32_t lead : {1, 3}) {
                            const int64_t b = fft_block_origin(p, k, lead), bm = fft_block_origin(p, k + dk, lead);
                            CHECK(bm == b + (int64_t)dN, "fft_block_origin %ld/%ld k=%lu lead=%d moved by %lu periods", (long)p.L, (long)p.M, (unsigned long)k, lead, (unsigned long)q);
                            for (int64_t fn : {n0, b < n0 ? b : n0}) // (a fresh stream's first_needed is negative at first: clamped to the base)
                                for (int64_t base : {(int64_t)0, fn - 5, fn + 3})
                                    for (size_t fill : {(size_t)0, (size_t)7, (size_t)5000}) {
                                        if (base < 0) continue;
                                        const RingKeep a = ring_keep(fn, base, fill), c = ring_keep(fn + (int64_t)dN, base + (int64_t)dN, fill);
                                        CHECK(c.keep_from == a.keep_from + (int64_t)dN && c.drop == a.drop && c.keep == a.keep, "ring_keep moved by %lu periods: first needed %ld base %ld fill %zu",
                                              (unsigned long)q, (long)fn, (long)base, fill);
                                    }
                        }
                    }
                }
        }
    CHECK(moved >= 7 * 3 * 5, "translations run: %ld", moved);
}

// ---- resident_msg: a message is refused exactly where one of its numbers does not fit its words — in_abs0, out_k0,
// out_frames and d0 = floor(out_k0 M / L) in 48 bits, in_frames and p0 = out_k0 M mod L in 24 — restated in 128 bits ----
static void check_resident_msg()
{
    Plan p;
    const int64_t lim = (int64_t)1 << 48, edge[] = {0, 1, 441, ((int64_t)1 << 24) - 1, (int64_t)1 << 24, ((int64_t)1 << 31) + 5, ((int64_t)1 << 40) + 9,
                                                    lim - 4411, lim - 2, lim - 1, lim, lim + 1, ((int64_t)1 << 50) + 1000003, -1};
    long refused = 0, taken = 0;
    for (auto &r : kBigLM) {
        p.L = r[0]; p.M = r[1]; p.T = 30;
        for (int vr = 0; vr < 2; ++vr)
            for (int64_t in_abs0 : edge)
                for (int64_t out_k0 : edge)
                    for (int64_t in_frames : {(int64_t)0, (int64_t)441, ((int64_t)1 << 24) - 1, (int64_t)1 << 24})
                        for (int64_t out_frames : {(int64_t)1, (int64_t)441, lim - 1, lim}) {
                            const ResidentMsg m = resident_msg(p, in_abs0, in_frames, out_k0, out_frames, vr != 0);
                            const i128 kM = vr ? (i128)0 : (i128)out_k0 * p.M, d0 = kM / p.L, p0 = kM % p.L;
                            auto in48 = [&](i128 v) { return v >= 0 && v < (i128)lim; };
                            const bool want = in48(in_abs0) && in48(out_k0) && in48(out_frames) && in48(d0) && in_frames >= 0 && in_frames < (1 << 24) && p0 >= 0 && p0 < (1 << 24);
                            CHECK(m.fits == want, "resident_msg %ld/%ld vr=%d in_abs0=%ld in_frames=%ld out_k0=%ld out_frames=%ld: fits=%d", (long)p.L, (long)p.M, vr, (long)in_abs0,
                                  (long)in_frames, (long)out_k0, (long)out_frames, (int)m.fits);
                            if (m.fits) CHECK((i128)m.d0 == d0 && (i128)m.p0 == p0, "resident_msg %ld/%ld out_k0=%ld: d0 / p0", (long)p.L, (long)p.M, (long)out_k0);
                            if (m.fits) ++taken; else ++refused;
                            // below every limit a message is taken; at or above one it is refused
                            if (in_abs0 >= lim || out_k0 >= lim || out_frames >= lim || in_frames >= (1 << 24)) CHECK(!m.fits, "resident_msg takes a number at or above its limit");
                        }
    }
    CHECK(refused > 0 && taken > 0, "resident_msg: %ld refused, %ld taken", refused, taken);
}

// ---- delay_constant / delay_vr: a stream below 2^32 outputs gets the plain double expression on its counters, bit for bit;
// at any age the value is within 4e-6 of a frame of the exact one (the bound stream_rules.h derives: four roundings of 2^-53
// relative on magnitudes below 2^33), where the plain expression on the counters themselves is off by a tenth of a frame ----
static void check_delay()
{
    Plan p;
    double worst = 0, worst_plain = 0;
    for (auto &r : kBigLM) {
        p.L = r[0]; p.M = r[1]; p.T = 30;
        for (uint64_t N : {(uint64_t)0, (uint64_t)1, (uint64_t)441, (uint64_t)1000, (uint64_t)100003, (uint64_t)400000000}) {
            const uint64_t total = out_len_big(p.L, p.M, N);
            for (uint64_t back : {(uint64_t)0, (uint64_t)1, (uint64_t)27, (uint64_t)300}) {
                if (back > total) continue;
                const uint64_t k = total - back;
                const double plain = (double)N * (double)p.L / (double)p.M - (double)k, got = delay_constant(p, N, k);
                if (k < ((uint64_t)1 << 32)) CHECK(got == plain, "delay_constant %ld/%ld N=%lu k=%lu: %.17g, the plain expression %.17g", (long)p.L, (long)p.M, (unsigned long)N, (unsigned long)k, got, plain);
                for (uint64_t at : kMoveAt) {
                    const uint64_t q = at / (uint64_t)p.L + 1, Nq = N + q * (uint64_t)p.M, kq = k + q * (uint64_t)p.L;
                    if ((Nq | kq) >> 62) continue;
                    const double exact = (double)((i128)Nq * p.L - (i128)kq * p.M) / (double)p.M;
                    const double e = std::fabs(delay_constant(p, Nq, kq) - exact), ep = std::fabs((double)Nq * (double)p.L / (double)p.M - (double)kq - exact);
                    CHECK(e <= 4e-6, "delay_constant %ld/%ld N=%lu k=%lu: off by %g", (long)p.L, (long)p.M, (unsigned long)Nq, (unsigned long)kq, e);
                    if (e > worst) worst = e;
                    if (ep > worst_plain) worst_plain = ep;
                }
            }
        }
    }
    CHECK(worst_plain > 0.05, "the plain expression at 2^50 was expected to be off by a tenth of a frame: %g", worst_plain);
    std::printf("  delay_constant: worst error %.3g frames at counts up to 2^50 (the plain double expression: %.3g)\n", worst, worst_plain);
    // variable rate: the clock moved by an integer pair gives the value of the clock at zero, bit for bit; against the exact quotient
    VrState v;
    v.on = true; v.s0 = v.s1 = q64(2.75625);
    for (uint64_t n_in : {(uint64_t)441, (uint64_t)100003})
        for (uint64_t k : {(uint64_t)0, (uint64_t)63, (uint64_t)150}) {
            const double fresh = delay_vr(v, n_in, k);
            CHECK(std::fabs(fresh - ((double)n_in - 2.75625 * (double)k) / 2.75625) < 1e-9, "delay_vr n_in=%lu k=%lu: %.17g", (unsigned long)n_in, (unsigned long)k, fresh);
            for (uint64_t at : kMoveAt) {
                VrState m = v;
                m.k_s = at + 17; m.t_s = (i128)((u128)(at + 1000003) << 64);
                CHECK(delay_vr(m, n_in + at + 1000003, k + at + 17) == fresh, "delay_vr moved to 2^%d differs", (int)std::log2((double)at));
            }
        }
}

int main()
{
    check_delay();
    check_translation();
    check_resident_msg();
    check_large_counts();
    check_k_avail();
    check_ring_keep();
    check_ring_grow();
    check_emit_count_constant();
    check_emit_count_vr();
    std::printf("stream_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
