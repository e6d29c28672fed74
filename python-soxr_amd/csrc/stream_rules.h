// stream_rules.h — the rules of the stream layer (engine.cpp) that read nothing but numbers: the variable-rate clock, the
// outputs due, what of the input ring is still needed, how a ring grows.  No HIP, no globals (tests/c/stream_rules_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "plan.h"

namespace hipsoxr {

// Variable-rate launches: input position of local output i is the Q64.64 fixed-point quadratic
//   t(i) = T0 + i*S0 + D*i(i-1)/2     (128-bit two's-complement words, hi:lo)
struct VrPos {
    uint64_t t_hi, t_lo, s_hi, s_lo, d_hi, d_lo;
};

// Variable-rate state (SOXR_VR streams; reference: src/soxr_ext.cpp:74, :200-204).  Time is kept in
// Q64.64 fixed point.  The current segment starts at output k_s with input position t_s and step
// s0; during the first n_slew outputs the step grows by `delta` per output, afterwards it is s1:
//     t(k_s + n) = t_s + n*s0 + delta*n(n-1)/2                      n <= n_slew
//                = t(k_s + n_slew) + (n - n_slew)*s1                n >  n_slew
// All integer arithmetic: positions are exact, monotonic, and independent of how calls are cut.
typedef unsigned __int128 u128;
typedef __int128 i128;
struct VrState {
    bool on = false;
    double max_io = 0.;  // in_rate/out_rate at creation: the largest io ratio the filter allows
    uint64_t k_s = 0, n_slew = 0;
    i128 t_s = 0, s0 = 0, delta = 0, s1 = 0;

    i128 pos(uint64_t k) const
    {
        const u128 n = k - k_s;
        if (n <= n_slew) return t_s + (i128)n * s0 + delta * (i128)(n * (n - 1) / 2);
        const u128 N = n_slew;
        return t_s + (i128)N * s0 + delta * (i128)(N * (N - 1) / 2) + (i128)(n - N) * s1;
    }
    i128 step(uint64_t k) const
    {
        const u128 n = k - k_s;
        return n < n_slew ? s0 + (i128)n * delta : s1;
    }
};
inline i128 q64(double x) { return (i128)(u128)std::ldexp(x, 64); } // truncating, exact scaling

// A launch's (or resident message's) clock: position and step at its first output k_done, step increment while a slew lasts
inline VrPos vr_pos_at(const VrState &v, uint64_t k_done)
{
    const i128 T0 = v.pos(k_done), S0 = v.step(k_done), D = k_done < v.k_s + v.n_slew ? v.delta : 0;
    return VrPos{(uint64_t)((u128)T0 >> 64), (uint64_t)(u128)T0, (uint64_t)((u128)S0 >> 64), (uint64_t)(u128)S0,
                 (uint64_t)((u128)D >> 64), (uint64_t)(u128)D};
}

// Number of outputs computable from the first N input frames without zero-extension:
// output k needs inputs up to floor(k*M/L) + T/2.
inline uint64_t k_avail(const Plan &p, uint64_t N)
{
    const int64_t H = p.T / 2;
    if ((int64_t)N - 1 - H < 0) return 0;
    unsigned __int128 Q = (unsigned __int128)(N - 1 - (uint64_t)H);
    unsigned __int128 v = ((Q + 1) * (unsigned __int128)p.L - 1) / (unsigned __int128)p.M;
    return (uint64_t)v + 1;
}

// Variable rate: number of outputs [0, K) computable from N input frames without zero-extension
// (output k reads up to floor(t(k)) + T/2), or — at end of input — the total K with
// t(k) + step(k)/2 <= N (the constant-rate rule floor(N*L/M + 1/2), restated for a moving step).
inline uint64_t vr_k_limit(const Plan &p, const VrState &v, uint64_t n_in_total, uint64_t k_done, bool ended)
{
    const int64_t H = p.T / 2;
    const i128 N = (i128)n_in_total << 64;
    auto ok = [&](uint64_t k) -> bool {
        if (ended) return v.pos(k) + v.step(k) / 2 <= N;
        return (int64_t)(v.pos(k) >> 64) + H <= (int64_t)n_in_total - 1;
    };
    uint64_t lo = k_done; // invariant: every k < lo is ok (already emitted, or checked)
    if (!ok(lo)) return lo;
    uint64_t span = 1;
    while (ok(lo + span)) { lo += span; span <<= 1; } // t is strictly increasing: exponential + binary search
    uint64_t hi = lo + span;                           // ok(lo), !ok(hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ok(mid)) lo = mid; else hi = mid;
    }
    return hi;
}

// How many outputs a call may emit now, from k_done on, into room for olen.  Constant rate: everything the input so far
// determines, or — after the end of input — everything up to the stream's length.
inline size_t emit_count(const Plan &p, uint64_t n_in_total, uint64_t k_done, bool ended, size_t olen)
{
    const uint64_t k_end = ended ? plan_out_len(p, n_in_total) : k_avail(p, n_in_total);
    return k_end > k_done ? (size_t)std::min<uint64_t>(k_end - k_done, olen) : 0;
}
// ... and with the stream's clock, which is renormalised here once a slew lies behind k_done
inline size_t emit_count(const Plan &p, VrState &v, uint64_t n_in_total, uint64_t k_done, bool ended, size_t olen)
{
    if (!v.on) return emit_count(p, n_in_total, k_done, ended, olen);
    if (v.n_slew && k_done >= v.k_s + v.n_slew) { // slew finished: renormalise to a constant segment
        const uint64_t k1 = v.k_s + v.n_slew;
        v.t_s = v.pos(k1); v.k_s = k1; v.s0 = v.s1; v.delta = 0; v.n_slew = 0;
    }
    const uint64_t k_end = vr_k_limit(p, v, n_in_total, k_done, ended);
    size_t n = k_end > k_done ? (size_t)std::min<uint64_t>(k_end - k_done, olen) : 0;
    // one launch evaluates one quadratic: stop at the end of a slew (emit_passes comes back for the rest)
    if (v.n_slew && k_done + n > v.k_s + v.n_slew) n = (size_t)(v.k_s + v.n_slew - k_done);
    return n;
}
// a pass that stopped there: the one case in which a call makes another
inline bool slew_just_ended(const VrState &v, uint64_t k_done) { return v.on && v.n_slew && k_done == v.k_s + v.n_slew; }

// Output frames still owed for the input so far (hipsoxr_stream_delay), constant rate: n_in L / M - handed, where `handed` is
// what the caller has been given.  Both terms grow with the stream's age, their difference does not: formed in doubles on the
// counters themselves it is off by a quarter of a frame at 2^50.  So the whole periods that fit below the last multiple of
// 2^32 outputs handed out are taken off both counters first — in integers, which changes nothing of the value — and the
// expression is formed on what is left: fewer than 2^32 + L outputs, whatever the age, so four roundings of 2^-53 relative on
// magnitudes below 2^33 — 4e-6 of a frame at the most.  A stream below 2^32 outputs (a day of 48 kHz audio; every test of the
// suite) gets the plain expression on its own counters, bit for bit what it always got.
inline double delay_constant(const Plan &p, uint64_t n_in, uint64_t handed)
{
    const uint64_t q = (handed >> 32 << 32) / (uint64_t)p.L;
    const i128 n = (i128)n_in - (i128)q * p.M; // (may be a frame or two below zero: handed runs half an output ahead at the end)
    const uint64_t k = handed - q * (uint64_t)p.L;
    return (double)n * (double)p.L / (double)p.M - (double)k;
}
// ... variable rate: the input not yet passed by the output clock, in output samples at the current step.  The difference of
// the two Q64.64 positions in integers, then one conversion.
inline double delay_vr(const VrState &v, uint64_t n_in, uint64_t k_done)
{
    const i128 ahead = (i128)((u128)n_in << 64) - v.pos(k_done);
    return (double)ahead / (double)v.step(k_done);
}

// Retire rule: the ring holds frames [in_base, in_base + in_fill) and the next output needs first_needed and later ones.
// What stays is [keep_from, end): first_needed clamped into the ring; `drop` frames go, `keep` stay.
struct RingKeep { int64_t keep_from; size_t drop, keep; };
inline RingKeep ring_keep(int64_t first_needed, int64_t in_base, size_t in_fill)
{
    const int64_t keep_from = std::min<int64_t>(std::max<int64_t>(first_needed, in_base), in_base + (int64_t)in_fill);
    const size_t drop = (size_t)(keep_from - in_base);
    return RingKeep{keep_from, drop, in_fill - drop};
}

// Frequency-domain streams (engine.cpp first_needed): the engine's origin for outputs from k_done on is the period boundary
// P0 = floor(k_done / L), and block 0 begins `lead` periods in front of it — the first input frame the ring must still hold
inline int64_t fft_block_origin(const Plan &p, uint64_t k_done, int32_t lead)
{
    return ((int64_t)(k_done / (uint64_t)p.L) - lead) * p.M;
}

// What a message to a resident kernel may carry (device.h ResidentBox, kernels.hip resident_post): positions in 48-bit
// pieces, the two short counts in 24 bits.  A message beyond that is refused and its call takes the ordinary path.
// d0, p0: out_k0 M = L d0 + p0, in 128 bits (variable rate: 0 — positions come from the message's own clock).
static constexpr uint64_t kResidentPosLimit = 1ULL << 48, kResidentShortLimit = 1u << 24;
struct ResidentMsg { int64_t d0, p0; bool fits; };
inline ResidentMsg resident_msg(const Plan &p, int64_t in_abs0, int64_t in_frames, int64_t out_k0, int64_t out_frames, bool vr)
{
    const __int128 kM = vr ? (__int128)0 : (__int128)out_k0 * p.M;
    const int64_t d0 = (int64_t)(kM / p.L), p0 = (int64_t)(kM % p.L);
    const bool fits = (uint64_t)in_abs0 < kResidentPosLimit && (uint64_t)out_k0 < kResidentPosLimit && (uint64_t)d0 < kResidentPosLimit &&
                      (uint64_t)in_frames < kResidentShortLimit && (uint64_t)p0 < kResidentShortLimit && (uint64_t)out_frames < kResidentPosLimit;
    return ResidentMsg{d0, p0, fits};
}

// Growth rule: capacities are the present one (at least 1024 frames) times a power of two; the smallest that holds the
// kept frames and `room` more — the caller's policy: so many chunks, so that compaction runs only every so many calls.
inline size_t ring_grow(size_t in_cap, size_t keep, size_t room)
{
    size_t cap = std::max<size_t>(in_cap, 1024);
    while (cap < keep + room) cap <<= 1;
    return cap;
}
// ... for rings in device memory: past 2^24 frames the policy gives way to room for the chunk alone
inline size_t ring_grow_bounded(size_t in_cap, size_t keep, size_t room, size_t ilen)
{
    return ring_grow(in_cap, keep, keep + room > ((size_t)1 << 24) ? ilen : room);
}

} // namespace hipsoxr
