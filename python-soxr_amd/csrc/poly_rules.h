// poly_rules.h — the rules of the two-stage form's polyphase launch (twostage.hip: launch_poly, launch_two_stage) that read
// nothing but numbers: which kernel form a job takes, how large a tile is in LDS, how long a thread's run may be, which
// lane order reads the table with the fewest bank conflicts, how many workgroups a column gets, which jobs the form admits
// and how its intermediate signal is laid out; and, for a clip table (launch_two_stage_ragged), how the clips are
// partitioned, where each column's intermediate lies, what rows both stages read and how the columns are cut into ranges.
// Each thing once.  No HIP, no globals (tests/c/poly_rules_check.cpp and tests/c/ragged_poly_rules_check.cpp check them
// against slow independent statements).
//
// What k_poly / k_poly2 rely on and these rules provide (the check program holds each):
//   * span_max covers every tile's source span nB - nA + 1 (xs[] in LDS ends where ys[] begins);
//   * a k_poly2 tile's span is at most 12 * 256 frames (it is held in registers: NPF);
//   * the two segments of a split column are a whole number of phase periods apart (m2_shift * Ls == n1 * Ms);
//   * the column count is an exact quotient, and a channel group never straddles a clip.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hipsoxr {

// ---- the stage as numbers -------------------------------------------------------------------------------------------
// T2 taps, P table intervals, `row` records per table row, output k at k * Ms / Ls of the stage's input samples
struct PolyStage {
    int32_t T2, P, row;
    int64_t Ls, Ms;
    double ratio; // Ms / Ls: input samples per output
};
inline PolyStage poly_stage(int32_t T2, int32_t P, int32_t row, int64_t Ls, int64_t Ms) { return PolyStage{T2, P, row, Ls, Ms, (double)Ms / (double)Ls}; }

// the kernels' position arithmetic (float32 path): frac(Ms / Ls) in units of 2^-64, truncated; 2^64 / Ls
inline uint64_t poly_step_fx(int64_t Ms, int64_t Ls) { return (uint64_t)((((unsigned __int128)(uint64_t)(Ms % Ls)) << 64) / (unsigned __int128)(uint64_t)Ls); }
inline double poly_fx_per_rem(int64_t Ls) { return 18446744073709551616. / (double)Ls; }
inline int32_t poly_lg(int32_t P)
{
    int32_t lg = 0;
    while ((1 << lg) < P) ++lg;
    return lg;
}

// ---- the form: one channel per pass (k_poly), channel pairs (k_poly2 IL), a column split into two segments (k_poly2) ---
// n1 / n2: outputs of member 1 / member 2 (both the job's n_out when the column is not split: tiles are counted over
// member 1).  m2_*: member 2's sample n is the column's n + m2_shift; element offsets of its samples / outputs.
struct PolyForm {
    bool pair, split;
    int32_t lg_cg; // a workgroup takes 2^lg_cg neighbouring channels (pairs: channel pairs) of a tile one after the other
    int64_t n1, n2, m2_shift, m2_src, m2_dst;
};
// width: bytes per element; Mq = floor(Ms / Ls); strides {clip, frame, channel}; ptr_bits: src | dst as integers
inline PolyForm poly_form(size_t width, int64_t Mq, uint32_t n_channels, const int64_t sstr[3], const int64_t dstr[3], uintptr_t ptr_bits, int32_t T2, bool no_pair,
                          int64_t n_out, int64_t Ls, int64_t Ms)
{
    PolyForm f{false, false, 0, n_out, n_out, 0, 0, 0};
    // channels per workgroup: neighbouring channels of interleaved data (source or destination) share their lines
    f.lg_cg = (sstr[2] == 1 || dstr[2] == 1) ? (n_channels % 4 == 0 ? 2 : n_channels % 2 == 0 ? 1 : 0) : 0;
    // k_poly2 at all: float32, windows that move by at most two frames, two windows of at most 40 taps in registers
    const bool can_two = width == 4 && (Mq == 0 || Mq == 1) && T2 <= 40 && !no_pair;
    // both ends channel-interleaved with an even channel count and 8-byte aligned frames: channel PAIRS (one pass over the
    // data, table reads shared by the two channels)
    f.pair = can_two && n_channels % 2 == 0 && sstr[2] == 1 && dstr[2] == 1 && ((sstr[0] | sstr[1] | dstr[0] | dstr[1]) & 1) == 0 && (ptr_bits & 7) == 0;
    if (f.pair) f.lg_cg = n_channels % 8 == 0 ? 2 : n_channels % 4 == 0 ? 1 : 0;
    // Any other float32 column of more than ~1.7 phase periods (Ls outputs: integer rate pairs have at most 2 f_out of
    // them per period): split h periods in — output k + h Ls has output k's fraction — and the two segments run as the pair
    if (!f.pair && can_two) {
        const int64_t h = (n_out + 2 * Ls - 1) / (2 * Ls), n1 = h * Ls, n2 = n_out - n1; // (member 1 is the longer one)
        if (h >= 1 && 10 * n2 >= 7 * n1 && h * Ms < (1LL << 40)) {
            f.split = true;
            f.n1 = n1; f.n2 = n2; f.m2_shift = h * Ms; f.m2_src = f.m2_shift * sstr[1]; f.m2_dst = n1 * dstr[1];
        }
    }
    return f;
}
// channel groups = gridDim.y (an exact quotient: 2^lg_cg, doubled for pairs, divides the channel count)
inline uint64_t poly_cols(uint32_t n_clips, uint32_t n_channels, bool pair, int32_t lg_cg)
{
    const int cg = 1 << lg_cg;
    return (uint64_t)n_clips * n_channels / (uint64_t)(pair ? 2 * cg : cg);
}

// ---- the tile in LDS: [table][source span of span_max elements][R x 257 staged outputs] -------------------------------
// a tile is 256 runs of R outputs; its source span is 256 R Ms / Ls samples, a window, and 4 spare words behind the last
// window (the register-window kernels read two samples ahead)
inline double poly_span(int R, double ratio, int32_t T2) { return 256. * R * ratio + T2 + 4; }
inline int32_t poly_span_max(int R, double ratio, int32_t T2) { return (int32_t)poly_span(R, ratio, T2); }
inline size_t poly_tile_elems(int R, double ratio, int32_t T2) { return (size_t)poly_span_max(R, ratio, T2) + 257u * (size_t)R; }
// unit: bytes per staged source / output element (a frame of the pair on k_poly2)
inline size_t poly_unit(size_t width, bool two) { return two ? 2 * width : width; }
inline size_t poly_tab_bytes(int32_t P, int32_t row, size_t width) { return (size_t)P * row * 4 * width; }
inline size_t poly_lds_bytes(size_t tab_bytes, int R, double ratio, int32_t T2, size_t unit) { return tab_bytes + poly_tile_elems(R, ratio, T2) * unit; }
constexpr size_t kPolyLdsMax = 160 * 1024; // what a workgroup can have
// the budget that sizes the longest run: three or two (float) / one (double) workgroups per CU
inline size_t poly_lds_cap(size_t width, size_t tab_bytes, bool two, int32_t T2)
{
    return (size_t)(width == 4 ? (tab_bytes > 40 * 1024 || (two && T2 >= 32) ? 78 : 52) : 96) * 1024;
}
constexpr int kPolyRunMax = 12;
constexpr double kPoly2SpanMax = 12. * 256.; // k_poly2 holds a whole span in registers (NPF = 12 frames per thread)
// outputs per thread: as many as keep the tile within the budget (and a k_poly2 span within its registers); dbg_poly_r > 0
// (HIPSOXR_DEBUG_POLY_R) lowers it further
inline int poly_rmax(size_t width, size_t tab_bytes, bool two, int32_t T2, double ratio, int dbg_poly_r)
{
    const size_t unit = poly_unit(width, two), cap = poly_lds_cap(width, tab_bytes, two, T2);
    int Rmax = kPolyRunMax;
    while (Rmax > 1 && (poly_lds_bytes(tab_bytes, Rmax, ratio, T2, unit) > cap || (two && poly_span(Rmax, ratio, T2) > kPoly2SpanMax))) --Rmax;
    if (dbg_poly_r > 0) Rmax = std::min(Rmax, dbg_poly_r);
    return Rmax;
}
// workgroups per CU the registers allow: k_poly2's launch bounds, k_poly's ~108 / float64's ~200
inline int poly_occ_limit(size_t width, bool two, int32_t T2) { return two ? (T2 >= 32 ? 2 : 3) : width == 4 ? 4 : 2; }
// workgroups per column the chip holds at once with runs of r
inline int64_t poly_slots(int r, size_t tab_bytes, double ratio, int32_t T2, size_t unit, int occ_limit, int n_cu, uint64_t cols)
{
    const int per_cu = std::max(1, std::min(occ_limit, (int)(kPolyLdsMax / poly_lds_bytes(tab_bytes, r, ratio, T2, unit))));
    return std::max<int64_t>(1, (int64_t)per_cu * n_cu / (int64_t)cols);
}

// ---- the lane order ----------------------------------------------------------------------------------------------------
// Thread t owns R consecutive outputs starting ((t * lane_mul) mod 256) * R into the tile (lane_mul odd: a bijection).
// Lanes l, l + 1 of a wave are then lane_mul * R outputs apart and their table rows form the arithmetic progression
// floor(c + l s), s = frac(lane_mul R Ms / Ls) P.  A 16-byte LDS read serves a lane group in one cycle when its 16 lanes
// fall on 16 different bank quads — (row + tap) mod 16 with the table's odd row stride — and takes one more cycle per
// extra distinct record on a quad.  Random rows cost 2.5-3 cycles; s within ~0.02 of an odd integer costs 1.
// The lanes of a wave that a 16-byte LDS read serves together, in the order the hardware groups them (four groups of 16):
constexpr int kPolyLaneGroup[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
struct PolyLane {
    int lane_mul; // odd, 1..255
    float conf;   // LDS conflict cost: 1 = every 16-byte read group in one cycle
};
// the cycles the 16 read groups of a workgroup take over 16 starting phases with lane multiplier am (stops early once the
// sum has reached `stop`: the caller has a multiplier that cheap already); halves: 16-byte reads per record (double4: 2)
inline double poly_lane_cycles(int P, int row, int halves, int r, double ratio, int am, double stop)
{
    double cost = 0.;
    for (int ph = 0; ph < 16 && cost < stop; ++ph)
        for (int wave = 0; wave < 4; ++wave)
            for (int g = 0; g < 4; ++g) {
                int rows[16][16], cnt[16] = {0}, mx = 1; // distinct rows seen per quad
                for (int q = 0; q < 16; ++q) {
                    const int tid = 64 * wave + kPolyLaneGroup[g][q];
                    const double f = ph / 16. + .37 + (double)((tid * am) & 255) * r * ratio;
                    const int i = (int)((f - std::floor(f)) * P) % P;
                    const int quad = (halves * row * i) & 15;
                    bool seen = false;
                    for (int z = 0; z < cnt[quad]; ++z) seen |= rows[quad][z] == i;
                    if (!seen) { rows[quad][cnt[quad]++] = i; mx = std::max(mx, cnt[quad]); }
                }
                cost += mx;
            }
    return cost;
}
// the first odd multiplier of the lowest cost, by simulating the four lane groups of the four waves over 16 starting phases
inline PolyLane poly_lane_cost(int P, int row, int halves, int r, double ratio)
{
    const double floor_cost = 16. * 16. * halves; // every group in one cycle: nothing better to look for
    double best = 1e30;
    int best_am = 1;
    for (int am = 1; am < 256 && best > floor_cost; am += 2) {
        const double cost = poly_lane_cycles(P, row, halves, r, ratio, am, best);
        if (cost < best) { best = cost; best_am = am; }
    }
    return PolyLane{best_am, (float)(best / floor_cost)};
}

// ---- the run length ----------------------------------------------------------------------------------------------------
// R: as long as the tiles fill the workgroups the chip holds (`slots` per column with runs of Rmax), the longest run that
// fits (a tile's fixed cost is about two outputs' time: job time = a + b / R with b / a = 2.06 — and a partly filled last
// round costs its share, not a round: 60 / 90 / 120 s take 56 / 72 / 88 us) among them the one whose table reads conflict
// least; below that, runs short enough to give every resident workgroup a tile (5 / 10 s stereo 24.3 / 25.0 -> 20.0 /
// 22.2 us, 10 s mono 26.0 -> 20.2; profiles/r05_ab_experiments.txt §7).  cost(r): the conflict cost of runs of r.
template <typename Cost>
inline int poly_pick_run(int Rmax, int64_t n_out, int64_t slots, Cost &&cost)
{
    int R = Rmax;
    if ((n_out + 256LL * Rmax - 1) / (256LL * Rmax) >= slots) { // a round or more
        double best = 1e30;
        for (int r = Rmax; r >= std::min(Rmax, std::max(2, Rmax / 3)) && best > 1.; --r) {
            const double c = cost(r) * (1. + .02 * (Rmax - r)); // (a shorter run per thread: more tiles per output)
            if (c < best) { best = c; R = r; }
        }
    } else // less than one round: shorter runs spread the job over the workgroups the chip holds
        R = (int)std::max<int64_t>(std::min(Rmax, 2), std::min<int64_t>(Rmax, (n_out + 256 * slots - 1) / (256 * slots)));
    return R;
}
inline int64_t poly_tiles(int64_t n_out, int R) { return (n_out + 256LL * R - 1) / (256LL * R); }

// ---- the grid ----------------------------------------------------------------------------------------------------------
// workgroups walk tiles (the table is loaded once per workgroup): exactly as many as the chip holds at once — a partly
// filled second round of workgroups would double the launch.  Above 8, a multiple of 8: columns' workgroups of one tile
// index on ONE XCD (workgroup b -> XCD b mod 8): interleaved channels share their lines in its L2
inline unsigned poly_grid_x(int64_t n_tiles, int per_cu, int n_cu, uint64_t cols)
{
    const int64_t want = std::max<int64_t>(1, (int64_t)std::max(per_cu, 1) * n_cu / (int64_t)cols);
    unsigned gx = (unsigned)std::min<int64_t>(n_tiles, want);
    if (gx > 8) gx &= ~7u;
    return gx;
}

// ---- the job ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kPolyMaxCols = 65535; // gridDim.y
// The jobs the two-stage form takes: 8192 frames or more either side and fewer than 2^30 (the kernels' products of an
// output index and Ms <= 2^31 then fit 64 bits), columns within gridDim.y, and the polyphase table with one tile's source
// span in LDS in the job's precision (long stages in float64 do not fit: the exact engine keeps those).  The last
// approximates poly_lds_bytes at R = 2 (R = 1, where nothing longer fits, needs less) — 512 ratio of span and
// 2 x 257 staged outputs, rounded up to 512 x 1.01 — in elements of `width` bytes against 150 of the 160 KiB: once it has
// said yes, launch_poly must not answer "does not fit LDS" behind a queued FFT stage.
inline bool two_stage_admits(int64_t n, int64_t n_out, uint64_t cols, size_t width, const PolyStage &s)
{
    if (n_out < 8192 || n < 8192 || n >= (1LL << 30) || n_out >= (1LL << 30)) return false;
    if (cols > kPolyMaxCols) return false;
    return !(poly_tab_bytes(s.P, s.row, width) + (size_t)(512. * (s.ratio + 1.01) + s.T2 + 4) * width > 150u * 1024u);
}

// The intermediate signal runs PAST both ends of the job, as far as the second stage reads it: `pad` samples of it
// before sample 0 and after the last one (a multiple of 8: 16-byte phases of the columns are kept).
//   down: v[m], m in [-pad, 2 n_out + pad): pad >= polyphase half-width in v samples
//   up:   u[m], m in [-pad, 2 n + pad):     pad >= polyphase half-width (T2 / 2 u samples)
// Layout [clip][channel][frames] — or [clip][frames][channel] (inter) when the job's own data is interleaved with an even
// channel count: the FFT stage then takes its channel-pair form (one complex word per frame and pair, contiguous for
// stereo) instead of pairing blocks over strided columns.  mstr: {clip, frame, channel} strides in elements.
struct TwoStageMid {
    int64_t pad, n_core, n_mid, mstr[3];
};
inline TwoStageMid two_stage_mid(bool up, int32_t T2, int64_t Ls, int64_t Ms, int64_t n, int64_t n_out, uint32_t n_channels, bool inter)
{
    TwoStageMid m;
    const double half_mid = up ? .5 * T2 : .5 * T2 * (double)Ls / (double)Ms;
    m.pad = ((int64_t)std::ceil(half_mid) + 4 + 7) / 8 * 8;
    m.n_core = up ? 2 * n : 2 * n_out;
    m.n_mid = m.n_core + 2 * m.pad;
    m.mstr[0] = m.n_mid * (int64_t)n_channels; m.mstr[1] = inter ? (int64_t)n_channels : 1; m.mstr[2] = inter ? 1 : m.n_mid;
    return m;
}

// The outputs the intermediate is SIZED for.  Down, the FFT stage's filter (fft_T taps at the intermediate's rate) reads
// fft_T / 2 samples of the intermediate past output k's position 2 k: a job truncated below the plan's output length
// (n_out < the out_len of its n input frames) needs the intermediate that far past 2 n_out, where the signal goes on — sized
// by n_out alone, the intermediate ended pad samples behind 2 n_out and the last ~fft_T / 4 outputs were the response to a
// signal cut short (2e-5 relative RMS on the last 3000 outputs of a clip truncated by 7).  A whole job (n_out = out_len) gets
// n_out back: nothing moves for it.  Up, the intermediate follows the input: n_out as it is.
// (Ms / Ls = M / (2 L) down, so the plan's out_len(n) = floor(n L / M + 1/2) = floor((n Ls + Ms) / (2 Ms)).)
inline int64_t two_stage_mid_outputs(bool up, int64_t Ls, int64_t Ms, int64_t n, int64_t n_out, int32_t fft_T)
{
    if (up) return n_out;
    const int64_t full = (n * Ls + Ms) / (2 * Ms);
    return std::max(n_out, std::min(full, n_out + (fft_T + 3) / 4));
}

// ---- a clip table on the two-stage form (twostage.hip launch_two_stage_ragged) ------------------------------------------
// A float clip table of an interpolated-phase plan (unit-stride, interleaved or strided columns): a constant number of launches whatever the
// number of clips.  The table's rows are {in offset, in frames, out offset, out frames} (elements from in / out).
//   * partition: a clip is EMPTY (out frames == 0: nothing is launched for it), TWO-STAGE (two_stage_admits says yes for its
//     own frame counts with its own channels as the column count — the question launch_two_stage asks of the clip alone, so
//     the engine of a clip does not depend on the table around it) or SHORT (every other clip: ONE ragged launch of the exact
//     engine's interpolated kernels over the compacted sub-table short_rows — the engine, and the bits, of the clip alone);
//   * columns, not clips, are the rows of the inner launches: both stages run with one channel and one table row per
//     (clip, channel) column of a two-stage clip, clip-major, at the caller's row offset + ch * channel stride;
//   * the intermediate of a column is its own: two_stage_mid of the clip alone (pad, n_core, n_mid — one channel, planar;
//     sized, as for the clip alone, for two_stage_mid_outputs of its frame counts),
//     packed [column][n_mid rounded up to 8 elements: the 16-byte phases of the columns are kept];
//   * ranges: the columns are cut into runs of at most kPolyMaxCols columns and at most `budget` bytes of intermediate (a
//     single column above the budget is a range of its own) — one allocation, one launch pair and one free per range, where
//     the clip-by-clip loop held one clip's intermediate at a time (1024 clips of 1-10 s mono: about 2 GB in one piece);
//   * the rows of both stages, in the kernels' own coordinates:
//       poly row {src offset of sample 0, n_src, dst offset of output k_lo, n_out}      (k_poly<.., RAGGED>; n_lo, k_lo job-wide)
//         down: {caller's input column, n,         mid column,              n_mid}      n_lo = 0,    k_lo = -pad
//         up:   {mid column + pad,      n_core + pad, caller's output column, n_out}    n_lo = -pad, k_lo = 0
//       FFT row {offset of the first stored sample, END of the column as an absolute sample index, out offset, out frames}
//         — k_fft_pair2 compares absolute indices against FftArgs::in_lo (= the job's in_abs0) and the row's second word —
//         down: {mid column,            n_core + pad, caller's output column, n_out}    in_abs0 = -pad
//         up:   {caller's input column, pad / 2 + n,  mid column,             n_mid}    in_abs0 = pad / 2
constexpr int64_t kPolyMidBudget = (int64_t)1 << 30; // bytes of intermediate per range: a design choice, not a measurement
enum RaggedPolyClass { kRaggedPolyEmpty = 0, kRaggedPolyTwo = 1, kRaggedPolyShort = 2 };
inline RaggedPolyClass ragged_poly_class(int64_t n, int64_t n_out, uint32_t n_channels, size_t width, const PolyStage &s)
{
    if (n_out <= 0) return kRaggedPolyEmpty;
    return two_stage_admits(n, n_out, n_channels, width, s) ? kRaggedPolyTwo : kRaggedPolyShort;
}
inline int64_t ragged_poly_col_elems(int64_t n_mid) { return (n_mid + 7) / 8 * 8; }

struct RaggedPolyRange {
    uint32_t first, count;                   // columns [first, first + count) of the two-stage columns
    int64_t mid_elems;                       // elements of the range's intermediate
    int64_t poly_longest;                    // the longest n_out of its poly rows: what R and the grid's frame axis are sized by
    int64_t fft_in_longest, fft_out_longest; // the FFT stage's job-wide frame counts (the longest column's)
};
struct RaggedPolyPlan {
    int64_t pad = 0;                           // the plan's, the same for every clip
    std::vector<uint8_t> cls;                  // [clips]
    std::vector<int64_t> short_rows;           // [short clips][4]: the caller's rows, compacted, table order
    std::vector<uint32_t> col_clip, col_ch;    // [columns]: clip-major, channels inside
    std::vector<TwoStageMid> col_mid;          // [columns]: two_stage_mid of the clip alone
    std::vector<int64_t> col_off;              // [columns]: element offset of the column in ITS RANGE's intermediate
    std::vector<int64_t> poly_rows, fft_rows;  // [columns][4]
    std::vector<RaggedPolyRange> ranges;
    uint32_t n_short() const { return (uint32_t)(short_rows.size() / 4); }
    uint32_t n_cols() const { return (uint32_t)col_clip.size(); }
};
// rows: the caller's table; in_chs / out_chs: its channel strides (the frame strides are the launcher's: offsets here are of sample 0); fft_T: the FFT stage's taps; budget:
// kPolyMidBudget (the debug-switch build may lower it)
// ... over the partition `cls(in frames, out frames)` -> RaggedPolyClass: the forward's is ragged_poly_class (below); the
// transposed form asks its own question of the same table (adjoint_auto_rules.h) and takes everything else from here
template <typename ClassOf>
inline RaggedPolyPlan ragged_poly_plan_by(const int64_t *rows, uint32_t n_clips, uint32_t n_channels, int64_t in_chs, int64_t out_chs, size_t width, bool up,
                                          const PolyStage &s, int32_t fft_T, int64_t budget, ClassOf cls)
{
    RaggedPolyPlan r;
    r.pad = two_stage_mid(up, s.T2, s.Ls, s.Ms, 0, 0, 1, false).pad;
    r.cls.resize(n_clips);
    for (uint32_t c = 0; c < n_clips; ++c) {
        const int64_t *row = rows + 4 * (size_t)c;
        r.cls[c] = (uint8_t)cls(row[1], row[3]);
        if (r.cls[c] == kRaggedPolyShort) r.short_rows.insert(r.short_rows.end(), row, row + 4);
        if (r.cls[c] != kRaggedPolyTwo) continue;
        for (uint32_t ch = 0; ch < n_channels; ++ch) {
            r.col_clip.push_back(c); r.col_ch.push_back(ch);
            r.col_mid.push_back(two_stage_mid(up, s.T2, s.Ls, s.Ms, row[1], two_stage_mid_outputs(up, s.Ls, s.Ms, row[1], row[3], fft_T), 1, false));
        }
    }
    const uint32_t n = r.n_cols();
    r.col_off.resize(n); r.poly_rows.resize(4 * (size_t)n); r.fft_rows.resize(4 * (size_t)n);
    RaggedPolyRange g{0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        const TwoStageMid &m = r.col_mid[i];
        const int64_t *row = rows + 4 * (size_t)r.col_clip[i];
        const int64_t elems = ragged_poly_col_elems(m.n_mid);
        if (g.count && (g.count == kPolyMaxCols || (g.mid_elems + elems) * (int64_t)width > budget)) {
            r.ranges.push_back(g);
            g = RaggedPolyRange{i, 0, 0, 0, 0, 0};
        }
        const int64_t off = g.mid_elems, in_col = row[0] + (int64_t)r.col_ch[i] * in_chs, out_col = row[2] + (int64_t)r.col_ch[i] * out_chs;
        r.col_off[i] = off;
        int64_t *pr = &r.poly_rows[4 * (size_t)i], *fr = &r.fft_rows[4 * (size_t)i];
        if (up) {
            fr[0] = in_col; fr[1] = m.pad / 2 + row[1]; fr[2] = off; fr[3] = m.n_mid;
            pr[0] = off + m.pad; pr[1] = m.n_core + m.pad; pr[2] = out_col; pr[3] = row[3];
        } else {
            pr[0] = in_col; pr[1] = row[1]; pr[2] = off; pr[3] = m.n_mid;
            fr[0] = off; fr[1] = m.n_core + m.pad; fr[2] = out_col; fr[3] = row[3];
        }
        ++g.count; g.mid_elems += elems;
        g.poly_longest = std::max(g.poly_longest, pr[3]);
        g.fft_in_longest = std::max(g.fft_in_longest, up ? row[1] : m.n_mid);
        g.fft_out_longest = std::max(g.fft_out_longest, fr[3]);
    }
    if (g.count) r.ranges.push_back(g);
    return r;
}
inline RaggedPolyPlan ragged_poly_plan(const int64_t *rows, uint32_t n_clips, uint32_t n_channels, int64_t in_chs, int64_t out_chs, size_t width, bool up,
                                       const PolyStage &s, int32_t fft_T, int64_t budget)
{
    return ragged_poly_plan_by(rows, n_clips, n_channels, in_chs, out_chs, width, up, s, fft_T, budget,
                               [&](int64_t n, int64_t n_out) { return ragged_poly_class(n, n_out, n_channels, width, s); });
}
// the form of a ragged polyphase launch: k_poly, one column per grid row (k_poly2 has no ragged form)
inline PolyForm poly_form_ragged(int64_t longest) { return PolyForm{false, false, 0, longest, longest, 0, 0, 0}; }

} // namespace hipsoxr
