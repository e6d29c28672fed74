// poly_adj_rules.h — the rules of the two-stage form's ADJOINT (twostage.hip: k_poly_adj, launch_poly_adj,
// launch_adjoint_two_stage; HIPSOXR_KERNEL_ADJOINT_TWO_STAGE) that read nothing but numbers: which outputs k of the
// polyphase stage can reach a run of its input samples (the bracket), how large a tile of input-side samples is, how many
// cotangent elements it stages, what that takes in LDS, how many workgroups a column gets, which jobs the selector admits and
// what it refuses by name before the device is asked for anything.  Each thing once.  No HIP, no globals
// (tests/c/poly_adj_rules_check.cpp checks them against brute force over the kernels' own positions).
//
// The forward stage (k_poly):   dst[k] = sum_{j < T2} c_j(f_k) src[n_k - (T2/2 - 1) + j],   (n_k, f_k) = floor / frac of k Ms / Ls
// Its transpose (k_poly_adj):   gsrc[n] = sum over k with 0 <= j = n - n_k + T2/2 - 1 < T2 of c_j(f_k) gdst[k]
//
// What k_poly_adj relies on and these rules provide (the check program holds each):
//   * every k that reaches a sample of [n_a, n_b] lies in poly_adj_bracket(n_a, n_b, ..) — by the exact position
//     floor(k Ms / Ls) AND by the float32 path's truncated 64.64 step (poly_step_fx), which may put a position that is exactly
//     an integer one sample lower with f ~ 1: n_k is floor(k Ms / Ls) or one less, never more.  The bracket is closed-form and
//     conservative; membership is decided per k by 0 <= j < T2, never by the bracket;
//   * a tile's bracket holds at most poly_adj_span_max elements (gs[] in LDS ends where ni[] begins);
//   * every k that reaches a thread's run lies in poly_adj_run_span's staged indices;
//   * an admitted job's tile fits kPolyLdsMax in the job's width.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "poly_rules.h"

// (the bracket is what the kernel itself calls: under a device compiler these are device functions too)
#if defined(__HIPCC__)
#define HIPSOXR_POLY_ADJ_RULE __host__ __device__ inline
#else
#define HIPSOXR_POLY_ADJ_RULE inline
#endif

namespace hipsoxr {

// ---- the bracket -----------------------------------------------------------------------------------------------------------
HIPSOXR_POLY_ADJ_RULE int64_t poly_adj_ceil_div(int64_t q, int64_t d) // d > 0
{
    const int64_t n = q / d;
    return n * d < q ? n + 1 : n;
}
// Outputs [k_first, k_last] (closed; empty when k_last < k_first) that can reach samples [n_a, n_b]: k reaches n when
// n_k is in [n - T2/2, n + T2/2 - 1], and n_k is floor(k Ms / Ls) or one less, so floor(k Ms / Ls) lies in
// [n_a - T2/2, n_b + T2/2] — one k of margin either side — cut to the stage's outputs [k_lo, k_lo + n_out).
// (|n| <= 2^31 + pad and Ls <= 2^31: the products fit 64 bits — two_stage_admits takes no longer job.)
struct PolyAdjSpan { int64_t k_first, k_last; };
HIPSOXR_POLY_ADJ_RULE PolyAdjSpan poly_adj_bracket(int64_t n_a, int64_t n_b, int32_t T2, int64_t Ls, int64_t Ms, int64_t k_lo, int64_t n_out)
{
    const int64_t H = T2 / 2;
    PolyAdjSpan s;
    s.k_first = poly_adj_ceil_div((n_a - H) * Ls, Ms) - 1;
    s.k_last = poly_adj_ceil_div((n_b + H + 1) * Ls, Ms);
    if (s.k_first < k_lo) s.k_first = k_lo;
    if (s.k_last > k_lo + n_out - 1) s.k_last = k_lo + n_out - 1;
    return s;
}
// ... and what a tile of `tile` samples stages at most: ceil(Y) - ceil(X) + 2 <= Y - X + 3 with Y - X = (tile + T2) Ls / Ms;
// even, so that the arrays behind it keep their 16-byte phase
inline int32_t poly_adj_span_max(int32_t tile, int32_t T2, double ratio) { return ((int32_t)((double)(tile + T2) / ratio) + 4 + 1) & ~1; }

// A thread's run of samples [n_a, n_b] of a tile whose staged outputs start at k_first (cnt of them): the staged indices
// [*s_first, *s_last] that can reach the run.  Staged index s sits at p0 + s Ms / Ls samples behind the lowest position
// that reaches n_a (p0: an exact integer over Ls), and reaches the run while that is in [0, n_b - n_a + T2 + 1): in
// double, with one index of margin either side (the figures are tile-sized: the rounding is 1e-12 of an index).
HIPSOXR_POLY_ADJ_RULE void poly_adj_run_span(int64_t n_a, int64_t n_b, int32_t T2, int64_t k_first, int64_t Ls, int64_t Ms, int32_t cnt, int32_t *s_first, int32_t *s_last)
{
    const double inv = (double)Ls / (double)Ms;
    const double p0 = (double)(k_first * Ms - (n_a - T2 / 2) * Ls) / (double)Ls;
    const double w = (double)(n_b - n_a + T2 + 1);
    double lo = floor(-p0 * inv) - 1., hi = ceil((w - p0) * inv);
    if (lo < 0.) lo = 0.;
    if (hi > (double)(cnt - 1)) hi = (double)(cnt - 1);
    const bool none = hi < lo; // (a run no staged output reaches: [0, -1])
    *s_first = none ? 0 : (int32_t)lo;
    *s_last = none ? -1 : (int32_t)hi;
}

// ---- the tile in LDS: [table][span_max x {g, x}][span_max x {n_k - n_A, row offset}][tile staged results] ------------------
// a tile is 256 runs of R consecutive samples of one column; a staged output takes two elements and two 32-bit integers
constexpr int kPolyAdjRunMax = 4;
inline int32_t poly_adj_tile(int R) { return 256 * R; }
inline size_t poly_adj_lds_bytes(size_t tab_bytes, int R, int32_t T2, double ratio, size_t width)
{
    return tab_bytes + (size_t)poly_adj_span_max(poly_adj_tile(R), T2, ratio) * (2 * width + 8) + (size_t)poly_adj_tile(R) * width;
}
// the budget that sizes the run: two workgroups per CU where a run fits that (the table alone may take more), else one
constexpr size_t kPolyAdjLdsTwo = 78 * 1024;
// R: the longest run (a power of two: 4, 2, 1) whose tile fits two to a CU, else the longest that fits at all; 0: none
inline int poly_adj_run(size_t tab_bytes, int32_t T2, double ratio, size_t width)
{
    for (int R = kPolyAdjRunMax; R >= 1; R /= 2)
        if (poly_adj_lds_bytes(tab_bytes, R, T2, ratio, width) <= kPolyAdjLdsTwo) return R;
    for (int R = kPolyAdjRunMax; R >= 1; R /= 2)
        if (poly_adj_lds_bytes(tab_bytes, R, T2, ratio, width) <= kPolyLdsMax) return R;
    return 0;
}
inline int64_t poly_adj_tiles(int64_t n_samples, int R) { return (n_samples + poly_adj_tile(R) - 1) / poly_adj_tile(R); }
// the grid: workgroups walk tiles (the table is loaded once per workgroup) — the forward's rule, one column per grid row
inline unsigned poly_adj_grid_x(int64_t n_tiles, int per_cu, int n_cu, uint64_t cols) { return poly_grid_x(n_tiles, per_cu, n_cu, cols); }
// ... a clip table's columns are of unequal length, and the grid's x is the longest column's: with as many workgroups as the
// chip holds, the short columns' workgroups leave early and their slots stay empty until the longest column's have walked all
// its tiles (64 clips of 1-10 s: 41 % of the launch), and the forward's multiple-of-8 rule drops 12 workgroups per column to 8.
// So a column gets kPolyAdjRaggedOver times its share of the slots, no rounding: the workgroups behind the first round start
// as earlier columns finish, which levels the columns (the table is copied once per workgroup: 17-50 KB against the 4
// tiles or more each still walks).  n_tiles: the longest column's.
constexpr int kPolyAdjRaggedOver = 4;
inline unsigned poly_adj_grid_x_ragged(int64_t n_tiles, int per_cu, int n_cu, uint64_t cols)
{
    const int64_t want = std::max<int64_t>(1, (int64_t)kPolyAdjRaggedOver * std::max(per_cu, 1) * n_cu / (int64_t)cols);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, want));
}

// ---- the job ---------------------------------------------------------------------------------------------------------------
// The adjoint job in = gy (n_y frames), out = gx (n_x frames) transposes the forward job (in_frames = n_x, out_frames = n_y):
// admitted when the forward job is (two_stage_admits) and the adjoint tile fits LDS in the job's width.  Asked before
// anything is queued: once it has said yes, launch_poly_adj must not fail on LDS behind a queued FFT stage.
inline bool poly_adj_admits(int64_t n_x, int64_t n_y, uint64_t cols, size_t width, const PolyStage &s)
{
    if (!two_stage_admits(n_x, n_y, cols, width, s)) return false;
    return poly_adj_run(poly_tab_bytes(s.P, s.row, width), s.T2, s.ratio, width) > 0;
}

// ---- refusals that need no device state ------------------------------------------------------------------------------------
// What the equal-length entry asks of a job that names the selector, in this order (float16 / bfloat16 are widened first and
// ask for the float32 job).  real: float32 / float64; exact_bank: the plan has no interpolated phases; window: in_abs0 or
// out_k0 is not 0; table: the job has a clip_table.
struct PolyAdjAsk { bool real, vr, exact_bank, window, table; };
inline const char *poly_adj_refusal(const PolyAdjAsk &q)
{
    if (!q.real) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE serves float32 or float64 elements (integer types have no gradient)";
    if (q.vr) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: variable-rate plans are not served";
    if (q.exact_bank) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE needs an interpolated-phase plan (exact-bank plans are served by HIPSOXR_KERNEL_ADJOINT_FFT, on the frequency-domain engine)";
    if (q.window) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: whole cotangents only (in_abs0 == 0, out_k0 == 0)";
    if (q.table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: a clip_table is not served on this entry (nor on the ragged one yet: clip by clip)";
    return nullptr;
}
// ... the ragged entry, whatever the job
constexpr const char *kPolyAdjRaggedRefusal =
    "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: ragged clip tables are not served yet (clip by clip through hipsoxr_run_device_adjoint; "
    "HIPSOXR_KERNEL_ADJOINT serves a table in one launch)";
// ... a plan without the form, a job the form does not admit, an FFT stage that declines: never the exact adjoint in its place
constexpr const char *kPolyAdjUnavailable =
    "adjoint job: HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: the two-stage form is unavailable for this plan or job (recipes below HQ, a bank installed from outside, "
    "ratios steeper than 4:1, fewer than 8192 frames either side, too many columns, a tile that leaves LDS, or an FFT stage that declines); "
    "HIPSOXR_KERNEL_ADJOINT runs the exact adjoint";
// ... and what the forward entry answers to the selector
constexpr const char *kPolyAdjForwardRefusal =
    "HIPSOXR_KERNEL_ADJOINT_TWO_STAGE selects the transposed two-stage form: it is valid on hipsoxr_run_device_adjoint only (forward jobs of "
    "interpolated-phase plans run the form under HIPSOXR_KERNEL_AUTO)";

} // namespace hipsoxr
