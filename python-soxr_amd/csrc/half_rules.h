// half_rules.h — the two decisions of a float16 / bfloat16 device job (kernels.hip launch_job_half, fft.hip, half.hip): whether
// the conversion is FUSED into a kernel of the frequency-domain engine, and — where it is not — the float32 temporaries of
// the widening pass: their strides, their bytes, and the ranges of clips (or channels) a job is cut into so that the
// temporaries of one range stay within a byte limit.  No HIP, no globals, no switches() (tests/c/half_rules_check.cpp checks
// each rule against a slow statement of it).
//
// What the callers rely on: the strides of a HalfPack address every (clip, frame, channel) of its extents exactly once
// inside [0, elems); its dimension order is the caller's — so the float32 job on the temporaries sees the layout class
// (unit-stride columns, interleaved channels, planar channels) the caller's tensors have and picks the kernel form the
// float32 job on such tensors picks; the ranges partition clips x channels; a range is within the limit unless it is one
// single column, which is never cut.
#pragma once
#include <cstddef>
#include <cstdint>

#include "job_rules.h" // the AUTO threshold and the column limit: the dispatcher's, for every element type

namespace hipsoxr {

// ---- fused or not ---------------------------------------------------------------------------------------------------
// The selector as the rule sees it: the frequency-domain engine by name, AUTO, or anything else (EXACT, GATHER, TILE* —
// and the selectors a half job is refused under, which never get here).
enum HalfSelector { kHalfSelFft, kHalfSelAuto, kHalfSelOther };

// AUTO takes the frequency-domain engine under the float rule — job_auto_fft, from kJobAutoFftMin output samples in all —
// since a half job has no bit-exact legacy to keep; by name always.  total_out: output samples over all clips and channels;
// no_fft: HIPSOXR_NO_FFT.
constexpr int64_t kHalfAutoFftMin = kJobAutoFftMin;
inline bool half_wants_fft(HalfSelector sel, int64_t total_out, bool no_fft)
{
    return sel == kHalfSelFft || (sel == kHalfSelAuto && job_auto_fft(total_out, no_fft));
}

// Ask the engine for a fused launch at all?  eligible: fft_job_eligible (whole signal, HQ / VHQ exact-ratio plan);
// cols: (clip, channel) columns — the paired kernels index them through grid.y.
constexpr uint64_t kHalfMaxCols = kJobMaxCols;
inline bool half_try_fused(HalfSelector sel, int64_t total_out, bool no_fft, bool eligible, uint64_t cols)
{
    return half_wants_fft(sel, total_out, no_fft) && eligible && cols <= kHalfMaxCols;
}

// ... and the form the engine then takes, from the layout decision of the row the FLOAT32 job of the shape takes (fft_layout):
// v2ok = unit-stride columns (k_fft_pair2), cp2ok = interleaved channel pairs (k_fft_strided2, one 4-byte word per frame);
// a clip table is served on unit-stride columns alone; strided single columns (st2ok) have no half form.
enum HalfForm { kHalfNone, kHalfPair2, kHalfChanPair };
inline HalfForm half_fused_form(bool on_table_row, bool v2ok, bool cp2ok, bool clip_table)
{
    if (!on_table_row) return kHalfNone; // (ratios outside the schedule table: k_fft_block has no half form)
    if (v2ok) return kHalfPair2;
    if (cp2ok && !clip_table) return kHalfChanPair;
    return kHalfNone;
}

// ---- the temporaries of the widening pass ------------------------------------------------------------------------------
// Dimensions are numbered as the job's strides are: 0 = clip, 1 = frame, 2 = channel.
struct HalfPack {
    int64_t stride[3]; // elements; dense: the innermost dimension has stride 1, each next one the product of those inside it
    int order[3];      // the dimensions, innermost first
    int64_t elems;     // product of the extents
};
inline int64_t half_abs(int64_t v) { return v < 0 ? -v : v; }

// Pack `extent` densely in the order of the caller's strides (smallest first).  A dimension of extent 1 addresses nothing
// and its caller's stride means nothing (torch leaves anything there): channel and frame go innermost, clip outermost —
// what a contiguous [clips, frames, channels] tensor has.  Equal strides (broadcast dimensions): channel, frame, clip.
inline HalfPack half_pack(const int64_t extent[3], const int64_t caller_stride[3])
{
    HalfPack p;
    // sort key: (class, |stride|, natural rank); class 0 = extent-1 frame / channel, 1 = real dimension, 2 = extent-1 clip
    int cls[3];
    int64_t key[3];
    const int rank[3] = {2, 1, 0}; // natural innermost-first rank: channel 0, frame 1, clip 2
    for (int d = 0; d < 3; ++d) {
        cls[d] = extent[d] > 1 ? 1 : (d == 0 ? 2 : 0);
        key[d] = extent[d] > 1 ? half_abs(caller_stride[d]) : 0;
    }
    auto before = [&](int a, int b) {
        if (cls[a] != cls[b]) return cls[a] < cls[b];
        if (key[a] != key[b]) return key[a] < key[b];
        return rank[a] < rank[b];
    };
    p.order[0] = 2; p.order[1] = 1; p.order[2] = 0;
    for (int i = 0; i < 3; ++i) // (three elements: insertion sort)
        for (int k = i; k > 0 && before(p.order[k], p.order[k - 1]); --k) { const int t = p.order[k]; p.order[k] = p.order[k - 1]; p.order[k - 1] = t; }
    int64_t run = 1;
    for (int i = 0; i < 3; ++i) {
        p.stride[p.order[i]] = run;
        run *= extent[p.order[i]] > 0 ? extent[p.order[i]] : 0;
    }
    p.elems = run;
    return p;
}

// ---- ranges ----------------------------------------------------------------------------------------------------------
// One range of a job: clips [clip0, clip0 + n_clips) x channels [ch0, ch0 + n_ch).  n_clips == 0: past the last range.
struct HalfRange { uint32_t clip0 = 0, n_clips = 0, ch0 = 0, n_ch = 0; };
constexpr uint64_t kHalfTmpLimit = (uint64_t)1 << 30; // bytes of float32 temporaries (input + output) per range

// How a job is cut: clips_per clips at a time; when ONE clip is above the limit, ch_per of its channels at a time.
struct HalfCut { uint32_t clips_per = 1, ch_per = 1; uint64_t clip_ranges = 0, ch_ranges = 0; };
inline HalfCut half_cut(uint32_t n_clips, uint32_t n_ch, int64_t in_frames, int64_t out_frames, uint64_t limit)
{
    HalfCut c;
    if (n_clips == 0 || n_ch == 0) return c;
    const uint64_t per_col = ((uint64_t)in_frames + (uint64_t)out_frames) * sizeof(float); // one column's input and output
    const uint64_t per_clip = per_col * n_ch;
    c.clips_per = n_clips; c.ch_per = n_ch;
    if (per_clip * n_clips > limit) {
        const uint64_t fit = per_clip ? limit / per_clip : n_clips;
        c.clips_per = (uint32_t)(fit < 1 ? 1 : fit > n_clips ? n_clips : fit);
        if (fit < 1) { // one clip alone is above the limit: ranges of its channels (a single column is never cut)
            const uint64_t cfit = per_col ? limit / per_col : n_ch;
            c.ch_per = (uint32_t)(cfit < 1 ? 1 : cfit > n_ch ? n_ch : cfit);
        }
    }
    c.clip_ranges = ((uint64_t)n_clips + c.clips_per - 1) / c.clips_per;
    c.ch_ranges = ((uint64_t)n_ch + c.ch_per - 1) / c.ch_per;
    return c;
}
inline uint64_t half_range_count(const HalfCut &c) { return c.clip_ranges * c.ch_ranges; }
// range r < half_range_count: channel ranges innermost
inline HalfRange half_range(const HalfCut &c, uint32_t n_clips, uint32_t n_ch, uint64_t r)
{
    HalfRange g;
    if (r >= half_range_count(c)) return g;
    const uint64_t ci = r / c.ch_ranges, hi = r % c.ch_ranges;
    g.clip0 = (uint32_t)(ci * c.clips_per);
    g.n_clips = n_clips - g.clip0 < c.clips_per ? n_clips - g.clip0 : c.clips_per;
    g.ch0 = (uint32_t)(hi * c.ch_per);
    g.n_ch = n_ch - g.ch0 < c.ch_per ? n_ch - g.ch0 : c.ch_per;
    return g;
}
// float32 bytes of a range's two temporaries
inline uint64_t half_range_bytes(const HalfRange &g, int64_t in_frames, int64_t out_frames)
{
    return (uint64_t)g.n_clips * g.n_ch * ((uint64_t)in_frames + (uint64_t)out_frames) * sizeof(float);
}

// ---- the copy kernels' index walk ---------------------------------------------------------------------------------------
// Linear index i < pack.elems of the dense temporary -> its coordinates along pack.order[0], [1], [2] (n0, n1: the extents
// of the two inner ones): the kernels of half.hip walk the temporary linearly — consecutive lanes on the caller's innermost
// dimension — and address the caller's tensor by its strides, taken in the same order.
#if defined(__HIPCC__)
#define HIPSOXR_HALF_HD __host__ __device__
#else
#define HIPSOXR_HALF_HD
#endif
struct HalfIdx { int64_t c[3]; };
HIPSOXR_HALF_HD inline HalfIdx half_unpack(int64_t i, int64_t n0, int64_t n1)
{
    HalfIdx x;
    const int64_t q = i / n0;
    x.c[0] = i - q * n0;
    x.c[2] = q / n1;
    x.c[1] = q - x.c[2] * n1;
    return x;
}

} // namespace hipsoxr
