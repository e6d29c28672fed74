// vr_adjoint_rules.h — the rules of the ragged variable-rate adjoint (hipsoxr_run_device_vr_ragged_adjoint; adjoint.hip
// k_adj_interp<.., VR> and launch_adjoint_vr_ragged) that read nothing but numbers: which cotangent samples k a gradient frame
// a sums over at a clip's constant step, the launch's grid, what is refused of a row.  No HIP, no globals
// (tests/c/vr_adjoint_rules_check.cpp checks the range rule against brute force).
//
// Forward (kernels_interp.h, the VR branch with T0 = 0, D = 0): output k sits at tt = k S (Q64.64, 128-bit), q_k = tt >> 64,
// and reads x[q_k - (H - 1) + j], j < T = 2 H.  Frame a is read by output k through tap j = a - q_k + H - 1:
//     0 <= j < T   <=>   a - H <= q_k <= a + H - 1   <=>   (a - H) 2^64 <= k S < (a + H) 2^64,
// so  k_lo(a) = max(0, ceil((a - H) 2^64 / S)),   k_hi(a) = min(n_y, ceil((a + H) 2^64 / S)) - 1.
// There is no 128-bit division on the device (the forward has 128-bit products only): the quotient is estimated in double
// precision and corrected with exact 128-bit products, the idea of kernels_interp.h's divmod_small.
#pragma once
#include <algorithm>
#include <cstdint>

#include "adjoint_rules.h"   // AdjGrid, kAdjMaxGridX, kAdjTooLong
#include "vr_ragged_rules.h" // u128, vr_ragged_step, vr_const_out_len, kVrRaggedMaxOut

// (the range rule is what k_adj_interp itself calls: under a device compiler it is a device function too)
#if defined(__HIPCC__)
#define HIPSOXR_VR_ADJ_RULE __host__ __device__ inline
#else
#define HIPSOXR_VR_ADJ_RULE inline
#endif

namespace hipsoxr {

// ceil(n 2^64 / S) for n < 2^40 and an admitted step (2^44 < S < 2^84): the least k with k S >= n 2^64.  The estimate
// floor(n 2^64 / S) in doubles is off by the quotient's 2^-52 relative error and the truncation: within one of the answer
// while the answer stays below 2^30 (kVrRaggedMaxOut), within a few up to 2^52 — the two loops step to the exact answer
// from wherever it lands, every product below 2^125.
HIPSOXR_VR_ADJ_RULE uint64_t vr_adj_ceil_q64(uint64_t n, unsigned __int128 S)
{
    typedef unsigned __int128 u128_;
    const u128_ N = (u128_)n << 64;
    const double two64 = 18446744073709551616.;
    const double s = (double)(uint64_t)(S >> 64) * two64 + (double)(uint64_t)S;
    uint64_t k = (uint64_t)((double)n * two64 / s);
    while (k > 0 && (u128_)(k - 1) * S >= N) --k;
    while ((u128_)k * S < N) ++k;
    return k;
}

// The cotangent samples frame a of a clip sums over: k in [lo, hi], empty when lo > hi.  a >= 0, H = T / 2 > 0, S the
// clip's step, n_y >= 0 its cotangent's length (at most kVrRaggedMaxOut).
struct VrAdjRange { int64_t lo, hi; };
HIPSOXR_VR_ADJ_RULE VrAdjRange vr_adj_k_range(int64_t a, int32_t H, unsigned __int128 S, int64_t n_y)
{
    typedef unsigned __int128 u128_;
    VrAdjRange r;
    r.lo = a > H ? (int64_t)vr_adj_ceil_q64((uint64_t)(a - H), S) : 0; // (a - H <= 0: the ceiling is <= 0)
    // the upper end is cut at n_y: where all of the cotangent lies in front of (a + H) 2^64 there is nothing to estimate
    if ((u128_)(uint64_t)n_y * S < ((u128_)(uint64_t)(a + H) << 64)) r.hi = n_y - 1;
    else r.hi = (int64_t)vr_adj_ceil_q64((uint64_t)(a + H), S) - 1;
    return r;
}

// k_adj_interp<.., VR>: gx workgroups of `frames` gradient frames along the LONGEST clip, gy (clip, channel) columns — more
// columns than gridDim.y holds wrap in the kernel's column loop: one launch whatever the table.  ok == false: kAdjTooLong.
inline AdjGrid vr_adj_grid(int64_t n_x, uint64_t n_cols, int frames)
{
    AdjGrid r;
    const int64_t gx = (n_x + frames - 1) / frames;
    r.ok = gx <= kAdjMaxGridX;
    r.gx = (uint32_t)gx; r.gy = (uint32_t)std::min<uint64_t>(n_cols, kJobMaxCols);
    return r;
}

// What is refused of one row {gy offset, n_y, gx offset, n_x} at its clip's step, or nullptr.  A is the forward of n_x input
// frames at that step; the cotangent has at most as many samples as A has outputs.
inline const char *vr_adj_row_refusal(const int64_t *row, int64_t job_in_frames, int64_t job_out_frames, u128 step)
{
    const JobRowFault f = job_row_bounds(row, job_in_frames, job_out_frames);
    if (f == kJobRowNegative) return "variable-rate ragged adjoint: a clip's offset or frame count is negative";
    if (f == kJobRowAboveJob) return "variable-rate ragged adjoint: a clip's frame counts exceed the job's in_frames / out_frames (the largest per-clip n_y / n_x)";
    if ((uint64_t)row[1] > vr_const_out_len((uint64_t)row[3], step))
        return "variable-rate ragged adjoint: a clip's n_y (cotangent frames) exceeds hipsoxr_plan_vr_out_len of its n_x at its io ratio";
    if (row[1] > kVrRaggedMaxOut) return "variable-rate ragged adjoint: a clip of more than 2^30 cotangent samples is not served";
    return nullptr;
}

} // namespace hipsoxr
