// adjoint_auto_rules.h — the rules of HIPSOXR_KERNEL_ADJOINT_AUTO (adjoint_auto.hip; the ragged two-stage transpose in
// twostage.hip launch_adjoint_two_stage_ragged) that read nothing but numbers: what the selector refuses by name, which engine
// the transpose of AUTO's forward runs on, and how a clip table of an interpolated-phase plan is cut for the transposed
// two-stage form.  No HIP, no globals, no switches(): plan kind, recipe, element class and switches arrive as arguments
// (tests/c/adjoint_auto_rules_check.cpp sweeps the decision table and checks the partition and the rows against brute force).
//
// The selector is DEFINED as the transpose of the job the forward launches under HIPSOXR_KERNEL_AUTO for the same plan and
// shape, so every decision here is the forward's own rule, asked of the forward job (in = gx side, out = gy side):
//   exact-bank plan          job_auto_fft of the forward's total outputs, HQ / VHQ            -> the frequency-domain engine
//   interpolated-phase plan  job_two_stage, the plan has the form, poly_adj_admits            -> the transposed two-stage form
//   everything else                                                                           -> the exact adjoint
// and an engine that declines before anything is queued leaves the job to the exact adjoint: the selector never answers
// "unavailable".
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "job_rules.h"
#include "poly_adj_rules.h"

namespace hipsoxr {

// ---- refusals that need no device state -----------------------------------------------------------------------------------
// What HIPSOXR_KERNEL_ADJOINT refuses, under this selector's name, in the entries' order (ragged:
// hipsoxr_run_device_adjoint_ragged).  half: float16 / bfloat16 (the equal-length entry widens such a job and asks for the
// float32 one); real: float32 / float64; window: in_abs0 or out_k0 is not 0; table: the job has a clip_table.
struct AdjAutoAsk { bool half, real, vr, window, table; };
inline const char *adj_auto_refusal(bool ragged, const AdjAutoAsk &q)
{
    if (ragged && q.half)
        return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: ragged: float16 / bfloat16 clip tables are not served (half cotangents clip by clip through hipsoxr_run_device_adjoint)";
    if (!q.real) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO serves float32 or float64 elements (integer types have no gradient)";
    if (q.vr) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: variable-rate plans are not served";
    if (q.window) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: whole cotangents only (in_abs0 == 0, out_k0 == 0)";
    if (!ragged && q.table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: a clip_table is served by hipsoxr_run_device_adjoint_ragged, not by this entry";
    if (ragged && !q.table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: the ragged entry needs a clip_table (equal-length clips: hipsoxr_run_device_adjoint)";
    return nullptr;
}
// ... what the forward entry answers to the selector
constexpr const char *kAdjAutoForwardRefusal =
    "HIPSOXR_KERNEL_ADJOINT_AUTO selects the transpose of the job HIPSOXR_KERNEL_AUTO launches: it is valid on hipsoxr_run_device_adjoint and "
    "hipsoxr_run_device_adjoint_ragged only (forward jobs have HIPSOXR_KERNEL_AUTO itself)";
// ... and a ragged two-stage launch whose FFT stage declines BEHIND the first range (the first range's decline, before anything
// is queued, sends the whole table to the exact adjoint): gx is part written, and is not patched silently
constexpr const char *kAdjAutoLateDecline =
    "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: the FFT stage declined a later range of the clip table after an earlier one was queued (gx is incomplete; "
    "HIPSOXR_KERNEL_ADJOINT runs the exact adjoint over the whole table)";

// ... the caller's clip table on its way to the device, and the derived tables of the transposed two-stage form
constexpr const char *kAdjAutoTableNoMemory = "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: ragged: no device memory for the clip table";
constexpr const char *kAdjAutoTableUploadFailed = "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: ragged: clip table upload failed";
constexpr const char *kAdjAutoFormNoMemory = "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: ragged: no device memory for the two-stage form's tables or intermediate signal";
constexpr const char *kAdjAutoFormUploadFailed = "adjoint job: HIPSOXR_KERNEL_ADJOINT_AUTO: ragged: upload of the two-stage form's tables failed";

// ---- the engine -------------------------------------------------------------------------------------------------------------
enum AdjAutoEngine { kAdjAutoExact = 0, kAdjAutoFft = 1, kAdjAutoTwoStage = 2 };
// What the decision reads.  phases: interpolated-phase plan; below_hq: att_db under the frequency-domain engine's 120 dB
// (adj_fft_refusal's rule); total_out: the FORWARD job's outputs in all — the cotangent's frames summed over clips (or the
// table's rows) and channels; form_ok: the plan has the two-stage form (TwoStage::ok); admits: poly_adj_admits of the job
// (equal-length entry) — on the ragged entry the question is asked per clip (adj_auto_class) and `admits` says whether ANY clip
// is admitted.
struct AdjAutoJob { bool phases, below_hq; int64_t total_out; bool no_fft, no_two_stage, form_ok, admits; };
inline AdjAutoEngine adj_auto_engine(const AdjAutoJob &q)
{
    if (!q.phases) return !q.below_hq && job_auto_fft(q.total_out, q.no_fft) ? kAdjAutoFft : kAdjAutoExact;
    const JobSel as_auto = {false, false, true, false, false, false};
    if (!job_two_stage(true, as_auto, kJobElemFloat, q.no_fft, q.no_two_stage)) return kAdjAutoExact;
    return q.form_ok && q.admits ? kAdjAutoTwoStage : kAdjAutoExact;
}
inline int64_t adj_auto_total_equal(int64_t n_y, uint32_t n_clips, uint32_t n_channels) { return n_y * (int64_t)n_clips * (int64_t)n_channels; }
inline int64_t adj_auto_total_table(const int64_t *rows, uint32_t n_clips, uint32_t n_channels)
{
    int64_t s = 0;
    for (uint32_t c = 0; c < n_clips; ++c) s += rows[kRaggedRow * (size_t)c + 1];
    return s * (int64_t)n_channels;
}

// ---- a clip table on the transposed two-stage form ------------------------------------------------------------------------
// An adjoint row {gy offset, n_y, gx offset, n_x} is the forward row {gx offset, n_x, gy offset, n_y}.  A clip is
//   EMPTY      n_x == 0: nothing is written;
//   TWO-STAGE  poly_adj_admits(n_x, n_y, channels, width, stage): the question the equal-length selector asks of the clip
//              alone, so a clip's engine does not depend on the table around it;
//   SHORT      every other clip — n_y == 0 < n_x included: its gx is zeros, and the exact adjoint writes them — ONE ragged
//              launch of the exact adjoint over the compacted sub-table (adjoint rows, as the caller wrote them).
inline RaggedPolyClass adj_auto_class(int64_t n_x, int64_t n_y, uint32_t n_channels, size_t width, const PolyStage &s)
{
    if (n_x <= 0) return kRaggedPolyEmpty;
    return poly_adj_admits(n_x, n_y, n_channels, width, s) ? kRaggedPolyTwo : kRaggedPolyShort;
}
inline std::vector<int64_t> adj_auto_swapped(const int64_t *rows, uint32_t n_clips)
{
    std::vector<int64_t> f(kRaggedRow * (size_t)n_clips);
    for (uint32_t c = 0; c < n_clips; ++c) {
        const int64_t *a = rows + kRaggedRow * (size_t)c;
        int64_t *o = &f[kRaggedRow * (size_t)c];
        o[0] = a[2]; o[1] = a[3]; o[2] = a[0]; o[3] = a[1];
    }
    return f;
}
// Columns, intermediates, packing and ranges are ragged_poly_plan's (poly_rules.h), applied to the swapped table with the
// channel strides swapped, over this partition.  What the transpose adds:
//   * short_rows: the caller's ADJOINT rows of the short clips, compacted, table order;
//   * fft_rows: the rows of the FFT stage's TRANSPOSED plan, in k_fft_pair2's coordinates {offset of the first stored sample,
//     END of the column as an absolute sample index, out offset, out frames} — the two cases of two_stage_adj_run, per column:
//       down (forward x -> poly -> mid -> FFT 2:1 -> y):  {gy column, pad / 2 + n_y, mid column, n_mid}      in_abs0 = pad / 2
//       up:                                                {mid column, n_core + pad, gx column, n_x}         in_abs0 = -pad
//   * per range, the longest source span k_poly_adj writes (n_src - n_lo: what its grid's x axis is sized by) and the FFT
//     stage's job-wide frame counts.
// The poly rows are the forward's rows as they stand: k_poly_adj reads `dst` and writes `src`.
struct RaggedPolyAdjRange { int64_t src_longest, fft_in_longest, fft_out_longest; };
struct RaggedPolyAdjPlan {
    RaggedPolyPlan fwd;                    // of the swapped table: cls, columns, col_mid, col_off, poly_rows, ranges (its short_rows and fft_rows: the forward's, unused)
    std::vector<int64_t> short_rows;       // [short clips][4], adjoint rows
    std::vector<int64_t> fft_rows;         // [columns][4], the transposed plan's
    std::vector<RaggedPolyAdjRange> ranges; // [fwd.ranges]
    int64_t n_lo = 0;                      // k_poly_adj's job-wide first sample: 0 down, -pad up
    uint32_t n_short() const { return (uint32_t)(short_rows.size() / 4); }
    uint32_t n_cols() const { return fwd.n_cols(); }
};
// rows: the caller's adjoint table; gy_chs / gx_chs: its channel strides (in / out of the adjoint job)
inline RaggedPolyAdjPlan ragged_poly_adj_plan(const int64_t *rows, uint32_t n_clips, uint32_t n_channels, int64_t gy_chs, int64_t gx_chs, size_t width, bool up,
                                              const PolyStage &s, int32_t fft_T, int64_t budget)
{
    RaggedPolyAdjPlan r;
    const std::vector<int64_t> swapped = adj_auto_swapped(rows, n_clips);
    r.fwd = ragged_poly_plan_by(swapped.data(), n_clips, n_channels, gx_chs, gy_chs, width, up, s, fft_T, budget,
                                [&](int64_t n_x, int64_t n_y) { return adj_auto_class(n_x, n_y, n_channels, width, s); });
    r.n_lo = up ? -r.fwd.pad : 0;
    for (uint32_t c = 0; c < n_clips; ++c)
        if (r.fwd.cls[c] == kRaggedPolyShort) r.short_rows.insert(r.short_rows.end(), rows + kRaggedRow * (size_t)c, rows + kRaggedRow * (size_t)(c + 1));
    const uint32_t n = r.fwd.n_cols();
    r.fft_rows.resize(4 * (size_t)n);
    for (const RaggedPolyRange &g : r.fwd.ranges) {
        RaggedPolyAdjRange a{0, 0, 0};
        for (uint32_t i = g.first; i < g.first + g.count; ++i) {
            const TwoStageMid &m = r.fwd.col_mid[i];
            const int64_t *row = rows + kRaggedRow * (size_t)r.fwd.col_clip[i];
            const int64_t gy_col = row[0] + (int64_t)r.fwd.col_ch[i] * gy_chs, gx_col = row[2] + (int64_t)r.fwd.col_ch[i] * gx_chs, off = r.fwd.col_off[i];
            int64_t *fr = &r.fft_rows[4 * (size_t)i];
            if (up) { fr[0] = off; fr[1] = m.n_core + m.pad; fr[2] = gx_col; fr[3] = row[3]; }
            else { fr[0] = gy_col; fr[1] = m.pad / 2 + row[1]; fr[2] = off; fr[3] = m.n_mid; }
            a.src_longest = std::max(a.src_longest, r.fwd.poly_rows[4 * (size_t)i + 1] - r.n_lo);
            a.fft_in_longest = std::max(a.fft_in_longest, up ? m.n_mid : row[1]);
            a.fft_out_longest = std::max(a.fft_out_longest, fr[3]);
        }
        r.ranges.push_back(a);
    }
    return r;
}

} // namespace hipsoxr
