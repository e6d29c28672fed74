// fft_ragged_rules.h — the integer rules of k_fft_strided2 on a clip table (fft.hip): the work-item map the kernel itself
// walks — which (channel unit, item) a workgroup id stands for, with and without the XCD-aware order — how many items a
// clip of its own length has, how the grid is sized from the longest clip, and what a table must satisfy to be served by
// that kernel.  No HIP, no globals (tests/c/fft_ragged_rules_check.cpp checks each against a slow statement of it).
//
// What the kernel relies on: over the grid of the LONGEST clip, every (unit, item) below a clip's OWN item count is the
// answer for exactly one workgroup id, and no id answers with an item at or above it — so a workgroup that is told
// `live == false` leaves before the first barrier, on its id and its clip's row alone.
#pragma once
#include <cstddef>
#include <cstdint>

// (the map is what the kernel calls: under a device compiler it is a device function too)
#if defined(__HIPCC__)
#define HIPSOXR_FFT_RULE __host__ __device__ inline
#else
#define HIPSOXR_FFT_RULE inline
#endif

namespace hipsoxr {

constexpr uint32_t kFftXcds = 8;            // XCDs a grid's consecutive workgroup ids are dealt to, round-robin
constexpr uint32_t kFftMapMaxClips = 65535; // the clip is grid.y

// Work items of one channel unit of a clip with out_frames outputs on blocks of hop_out kept outputs: one per block
// (channel pairs) or one per pair of blocks (single columns).  An empty clip has none.
HIPSOXR_FFT_RULE int64_t fft_clip_items(int64_t out_frames, int64_t hop_out, bool chpair)
{
    if (out_frames <= 0) return 0;
    const int64_t blocks = (out_frames - 1) / hop_out + 1;
    return chpair ? blocks : (blocks + 1) / 2;
}

// grid.x of the XCD-aware map: every XCD gets the same number of items of every unit (the longest clip's, rounded up)
inline int64_t fft_xcd_grid_x(int64_t longest_items, int64_t units) { return (longest_items + kFftXcds - 1) / kFftXcds * kFftXcds * units; }

struct FftMapItem {
    uint32_t unit, item; // channel unit; block (channel pairs) or pair of blocks (single columns) of its columns
    bool live;           // false: the id is padding, or lies at or behind the clip's last item — nothing to do
};
// The XCD-aware map.  Workgroup ids are dealt round-robin to the XCDs, each with an L2 of its own: x = 8 * slot + xcd,
// slot = chunk * units + unit — the channel units of one block of frames share every cache line and get ids that are
// congruent mod 8 and adjacent in dispatch order — and each XCD takes a CONTIGUOUS run of the clip's items,
// item = xcd * per_xcd + chunk with per_xcd = ceil(items / 8), so that the input two neighbouring blocks share meets in
// one L2.  items: of the clip the workgroup belongs to — the job's for equal-length clips, the clip's OWN on a table: a
// short clip of a table is then spread over all eight XCDs like a long one, where per_xcd of the longest clip would put
// every short clip's items on the first XCDs alone.  (grid.x = fft_xcd_grid_x of the longest clip covers every chunk
// below ceil(items / 8) of every clip.)
HIPSOXR_FFT_RULE FftMapItem fft_xcd_map(uint32_t x, uint32_t units, int64_t items)
{
    const uint32_t xcd = x & (kFftXcds - 1), slot = x / kFftXcds;
    const uint32_t per_xcd = (uint32_t)((items + kFftXcds - 1) / kFftXcds);
    const uint32_t chunk = slot / units;
    FftMapItem m;
    m.unit = slot % units;
    m.item = xcd * per_xcd + chunk;
    m.live = chunk < per_xcd && (int64_t)m.item < items;
    return m;
}
// Without the map (one column, channels that are not interleaved, HIPSOXR_FFT_NO_XCD_MAP): items along grid.x, (clip,
// unit) columns along grid.y = clip * units + unit.
HIPSOXR_FFT_RULE FftMapItem fft_plain_map(uint32_t x, uint32_t y, uint32_t units, int64_t items)
{
    FftMapItem m;
    m.unit = y % units;
    m.item = x;
    m.live = (int64_t)x < items;
    return m;
}

// ---- what a clip table adds to the layout decision (fft_layout / fft_launch_row) ---------------------------------------
// the map: the clip index is grid.y
inline bool fft_map_clips_ok(uint32_t n_clips) { return n_clips <= kFftMapMaxClips; }
// 2-byte channel pairs are ONE 4-byte access per frame: with an even frame stride and 4-byte aligned base pointers (the
// equal-length conditions, unchanged), every clip's first pair is aligned when both of its row's offsets are even
inline bool fft_table_words_aligned(const int64_t *rows, uint32_t n_clips)
{
    for (uint32_t c = 0; c < n_clips; ++c)
        if ((rows[4 * (size_t)c] | rows[4 * (size_t)c + 2]) & 1) return false;
    return true;
}
// Which launch forms take a table: unit-stride columns (k_fft_pair2) under every selector that reaches the engine; the
// strided kernel's two forms BY NAME only — HIPSOXR_KERNEL_AUTO keeps interleaved and strided tables of an exact-bank plan
// on the exact engine's ragged launch, bit for bit (by_name: HIPSOXR_KERNEL_FFT / _FFT_F64 / _FFT_PCM, and the two-stage
// form's inner jobs, which name the engine).
inline bool fft_table_form_served(bool v2ok, bool cp2ok, bool st2ok, bool by_name)
{
    if (v2ok) return true;
    return (cp2ok || st2ok) && by_name;
}

} // namespace hipsoxr
