// ragged_rules.h — the integer rules of a ragged exact launch (kernels.hip launch_ragged, the `bool RAGGED` kernels of
// kernels_tile.h, kernels_interp.h and k_gather): how the grid's frame axis is sized, which workgroups and lanes skip, how
// many slabs / workgroups a clip table holds, how a table of more columns than gridDim.y folds into ranges of clips.  No HIP,
// no globals (tests/c/ragged_rules_check.cpp and tests/c/ragged_interp_rules_check.cpp check them against brute force).
#pragma once
#include <algorithm>
#include <cstdint>

#include "job_rules.h" // kRaggedRow (a clip table's row), kJobMaxCols

// (the skip tests are what the kernels themselves call: under a device compiler they are device functions too)
#if defined(__HIPCC__)
#define HIPSOXR_RULE __host__ __device__ inline
#else
#define HIPSOXR_RULE inline
#endif

namespace hipsoxr {

constexpr uint32_t kMaxGridY = kJobMaxCols;

// the longest clip of rows [0, n): what sizes the grid's frame axis and chooses the kernel family
inline int64_t ragged_longest(const int64_t *rows, uint32_t n)
{
    int64_t m = 0;
    for (uint32_t c = 0; c < n; ++c) m = std::max(m, rows[kRaggedRow * (size_t)c + 3]);
    return m;
}

// Tile kernels: a slab is pb periods of Lc outputs; slab x of a column holds outputs [x pb Lc, (x + 1) pb Lc).
// Slabs that hold an output of a clip of out_frames outputs: ceil(ceil(out_frames / Lc) / pb).
inline int64_t ragged_slabs(int64_t out_frames, int64_t Lc, int32_t pb)
{
    if (out_frames <= 0) return 0;
    return ((out_frames - 1) / Lc) / pb + 1;
}
// ... the frame axis of the grid: the longest clip's
inline int64_t ragged_grid_x(int64_t longest, int64_t Lc, int32_t pb) { return ragged_slabs(longest, Lc, pb); }
// ... the workgroup of slab x skips a clip none of whose outputs lie in the slab: its first period starts at or behind the end
HIPSOXR_RULE bool ragged_skip(int64_t x, int64_t Lc, int32_t pb, int64_t out_frames) { return x * pb * Lc >= out_frames; }
// ... slabs in all that do work, over the clips' columns: what the planar kernel's cost model is fed (not longest x clips)
inline int64_t ragged_total_slabs(const int64_t *rows, uint32_t n, uint32_t n_channels, int64_t Lc, int32_t pb)
{
    int64_t s = 0;
    for (uint32_t c = 0; c < n; ++c) s += ragged_slabs(rows[kRaggedRow * (size_t)c + 3], Lc, pb);
    return s * (int64_t)n_channels;
}

// k_gather: one lane per output (channel-fast data: per (output, channel) element), 256 lanes per workgroup
inline int64_t ragged_gather_grid_x(int64_t longest, uint32_t lanes_per_output) { return (longest * (int64_t)lanes_per_output + 255) / 256; }
HIPSOXR_RULE bool ragged_gather_skip(int64_t idx, int64_t out_frames) { return idx >= out_frames; }

// k_interp_wave (U = 32) and k_interp_tile (U = KO): workgroup x of a column holds that column's outputs [x U, (x + 1) U).
// Workgroups that hold an output of a clip of out_frames outputs: ceil(out_frames / U).
inline int64_t ragged_span_wgs(int64_t out_frames, int64_t U)
{
    if (out_frames <= 0) return 0;
    return (out_frames - 1) / U + 1;
}
// ... the frame axis of the grid: the longest clip's
inline int64_t ragged_span_grid_x(int64_t longest, int64_t U) { return ragged_span_wgs(longest, U); }
// ... workgroup x skips a clip none of whose outputs it holds: its first output lies at or behind the clip's end (an empty
// clip skips every workgroup).  Uniform over the workgroup: asked before the first barrier and before any position is located.
HIPSOXR_RULE bool ragged_span_skip(int64_t x, int64_t U, int64_t out_frames) { return x * U >= out_frames; }
// ... workgroups in all that do work, over the clips' columns (cols_per_clip: the channels, or the channel pairs): what the
// interpolated tile kernel's cost model is fed (not longest x clips)
inline int64_t ragged_span_total(const int64_t *rows, uint32_t n, uint32_t cols_per_clip, int64_t U)
{
    int64_t s = 0;
    for (uint32_t c = 0; c < n; ++c) s += ragged_span_wgs(rows[kRaggedRow * (size_t)c + 3], U);
    return s * (int64_t)cols_per_clip;
}
// ... the tile form is weighed at all from this many outputs per channel in the whole table (what launch_gather asks of one
// equal-length launch); below it the wave / lane kernels serve the table
constexpr int64_t kRaggedTileMinOut = 4096;
inline bool ragged_tile_considered(const int64_t *rows, uint32_t n);
// ... and the outputs in all of one channel of the table (the lane-per-output side of that model)
inline int64_t ragged_total_out(const int64_t *rows, uint32_t n)
{
    int64_t s = 0;
    for (uint32_t c = 0; c < n; ++c) s += rows[kRaggedRow * (size_t)c + 3];
    return s;
}
inline bool ragged_tile_considered(const int64_t *rows, uint32_t n) { return ragged_total_out(rows, n) >= kRaggedTileMinOut; }

// More (clip, channel) columns than gridDim.y holds: one launch per range of clips.  Clips per launch, or 0 where one
// clip's channels alone do not fit (such a job is served clip by clip, its channels folded there).
inline uint32_t ragged_fold_step(uint32_t n_channels) { return n_channels ? kMaxGridY / n_channels : 0; }
// range r of the fold: clips [first, first + count); count == 0 behind the last range
struct RaggedRange { uint32_t first, count; };
inline RaggedRange ragged_fold_range(uint32_t n_clips, uint32_t n_channels, uint32_t r)
{
    const uint32_t step = ragged_fold_step(n_channels);
    const uint64_t first = (uint64_t)r * step;
    if (!step || first >= n_clips) return RaggedRange{n_clips, 0};
    return RaggedRange{(uint32_t)first, (uint32_t)std::min<uint64_t>(step, n_clips - first)};
}

} // namespace hipsoxr
