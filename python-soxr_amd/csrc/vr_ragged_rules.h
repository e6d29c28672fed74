// vr_ragged_rules.h — the rules of a ragged variable-rate launch (hipsoxr_run_device_vr_ragged; kernels.hip launch_ragged_vr)
// that read nothing but numbers: how many outputs a clip has at its own constant step, the step that sizes the launch's
// geometry, what is refused of a ratio and of a row.  No HIP, no globals (tests/c/vr_ragged_rules_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "ragged_rules.h"
#include "stream_rules.h"

namespace hipsoxr {

// A launch's clock table: one row per clip, its Q64.64 step as two words {hi, lo} (T0 = 0, D = 0: a clip starts at input
// position 0 and keeps its step).
constexpr int kVrClockRow = 2;
// the step of an io ratio: what hipsoxr_stream_set_io_ratio makes of it (q64: truncating)
inline u128 vr_ragged_step(double io_ratio) { return (u128)q64(io_ratio); }

// Outputs of n_in input frames at the constant step S after end of input: the k >= 0 with k S + S/2 <= n_in 2^64 (S/2
// truncates, as VrState::step(k) / 2 does) — vr_k_limit(p, v, n_in, 0, true) for v = {t_s = 0, s0 = s1 = S, n_slew = 0} in
// closed form.  A step below 2 (no io ratio in range comes near it) has no outputs.
inline uint64_t vr_const_out_len(uint64_t n_in, u128 step)
{
    if (step < 2) return 0;
    const u128 N = (u128)n_in << 64, half = step / 2;
    if (half > N) return 0;
    return (uint64_t)((N - half) / step) + 1;
}

// The largest step of a clock table, in input samples per output: what sizes wave_geom and interp_tile_form for the whole
// launch (vr_max_step's value for D = 0, margin included)
inline double vr_ragged_max_step(const uint64_t *clock, uint32_t n)
{
    const double two64 = 18446744073709551616.;
    double m = 0;
    for (uint32_t c = 0; c < n; ++c)
        m = std::max(m, (double)clock[kVrClockRow * (size_t)c] + (double)clock[kVrClockRow * (size_t)c + 1] / two64);
    return m * (1. + 1e-9);
}

// Most outputs of one clip: a launch's frame axis stays one launch (launch_gather cuts an equal-length job there)
constexpr int64_t kVrRaggedMaxOut = (int64_t)1 << 30;

// What is refused of one clip's io ratio on a plan designed for max_io = in_rate / out_rate, or nullptr.  The limits are
// hipsoxr_stream_set_io_ratio's own (2^-20 < io ratio < 2^20; at most max_io (1 + 1e-12)), the second in its own words.
inline const char *vr_ragged_ratio_refusal(double io_ratio, double max_io)
{
    if (!(io_ratio > 9.5367431640625e-07) || !(io_ratio < 1048576.))
        return "variable-rate ragged batch: a clip's io ratio is out of range (2^-20 < io ratio < 2^20)";
    if (io_ratio > max_io * (1. + 1e-12)) return "io ratio exceeds the maximum given at creation (the filter would alias)";
    return nullptr;
}

// What is refused of one row {in offset, in frames, out offset, out frames} at its clip's step, or nullptr
inline const char *vr_ragged_row_refusal(const int64_t *row, int64_t job_in_frames, int64_t job_out_frames, u128 step)
{
    // (sign and bounds: job_rules.h's, as on every clip table; the length rule is the clip's own step's)
    const JobRowFault f = job_row_bounds(row, job_in_frames, job_out_frames);
    if (f == kJobRowNegative) return "variable-rate ragged batch: a clip's offset or frame count is negative";
    if (f == kJobRowAboveJob) return "variable-rate ragged batch: a clip's frame counts exceed the job's in_frames / out_frames (the largest per-clip counts)";
    if ((uint64_t)row[3] > vr_const_out_len((uint64_t)row[1], step))
        return "variable-rate ragged batch: a clip's out_frames exceed hipsoxr_plan_vr_out_len of its in_frames at its io ratio";
    if (row[3] > kVrRaggedMaxOut) return "variable-rate ragged batch: a clip of more than 2^30 outputs is not served";
    return nullptr;
}

} // namespace hipsoxr
