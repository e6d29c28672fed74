// job_rules.h — the rules of the device-job dispatcher (kernels.hip launch_job and the launches over a clip table beside it;
// adjoint.hip launch_adjoint_ragged): what is refused before the device is asked for anything, which engine a job is offered
// to and in which order, what a clip table's row must satisfy, how a job of more columns than gridDim.y holds is folded.
// No HIP, no globals, no switches(): selector, element class and switches arrive as arguments
// (tests/c/job_rules_check.cpp checks each rule against a slow statement of it).
//
// The order the dispatcher keeps: refusals; a clip table (frequency-domain engine, two-stage form, ragged exact launch, clip
// by clip); a half job (fused, or half.hip's passes); the column fold; then two-stage form, frequency-domain engine, that
// engine on integer samples, and the exact engine's typed launch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hipsoxr {

// ---- selector and element type as the dispatcher sees them -------------------------------------------------------------
struct JobSel {
    bool want_fft;     // HIPSOXR_KERNEL_FFT / HIPSOXR_KERNEL_FFT_F64: the frequency-domain engine by name, float samples
    bool want_pcm;     // HIPSOXR_KERNEL_FFT_PCM: that engine by name, integer samples
    bool is_auto;      // HIPSOXR_KERNEL_AUTO
    bool exact_family; // HIPSOXR_KERNEL_EXACT / HIPSOXR_KERNEL_GATHER: what launch_gather's lane-per-output kernel serves by name
    bool fft_f64;      // HIPSOXR_KERNEL_FFT_F64
    bool wave_dot;     // HIPSOXR_KERNEL_WAVE_DOT
};
enum JobElem { kJobElemFloat, kJobElemPcm, kJobElemHalf, kJobElemOther }; // float32 / float64; int16 / int32; float16 / bfloat16; invalid

// ---- engines -------------------------------------------------------------------------------------------------------------
// Frequency-domain engine: explicit request, or AUTO for whole-signal float jobs of kJobAutoFftMin outputs in all
// (over clips and channels; a clip table: the sum of its rows).  It is NOT bit-identical to the canonical order (about 2e-7
// relative RMS), so it is never chosen for HIPSOXR_KERNEL_EXACT — which is what the stream / one-shot host entry points pass.
// The same rule for equal-length jobs, clip tables and half jobs: engine choice — and with it bit-exactness — does not
// depend on whether a table is present.
constexpr int64_t kJobAutoFftMin = (int64_t)1 << 13; // even one block pair beats the tiled exact kernels (7 vs 10 us)
inline bool job_auto_fft(int64_t total_out, bool no_fft) { return total_out >= kJobAutoFftMin && !no_fft; }
// ... offer the job to the engine?  (eligibility — fft_job_eligible — and the column limit are the caller's to add)
inline bool job_try_fft(const JobSel &s, int64_t total_out, bool no_fft)
{
    return s.want_fft || s.want_pcm || (s.is_auto && job_auto_fft(total_out, no_fft));
}

// Ratios without an exact bank (interpolated-phase plans): the two-stage form — FFT engine at 1:2 / 2:1 plus a short
// polyphase stage — for whole-signal float jobs (1e-6 class, like the FFT engine itself; twostage.hip).
// ... a clip table: float clips under AUTO belong to that form (another precision class).  launch_job's table branch offers
// the table to launch_two_stage_ragged under this rule, and launch_ragged_job steps aside under the same one — all but the
// sub-table of clips the form does not admit, which are the exact engine's.
inline bool job_two_stage_table(bool phases, const JobSel &s, JobElem elem, bool no_fft, bool no_two_stage)
{
    return phases && s.is_auto && elem == kJobElemFloat && !no_fft && !no_two_stage;
}
// ... an equal-length job: the same rule, and by name (HIPSOXR_NO_FFT speaks of AUTO alone)
inline bool job_two_stage(bool phases, const JobSel &s, JobElem elem, bool no_fft, bool no_two_stage)
{
    if (s.want_fft) return phases && elem == kJobElemFloat && !no_two_stage;
    return job_two_stage_table(phases, s, elem, no_fft, no_two_stage);
}

// ---- refusals that need no device state -----------------------------------------------------------------------------------
// Each returns the text, or nullptr; job_entry_refusal (kernels.hip) asks them in this order.
constexpr uint32_t kJobMaxCols = 65535; // (clip, channel) columns of one launch: gridDim.y

inline bool job_empty(int64_t out_frames, uint32_t n_clips, uint32_t n_channels) { return out_frames <= 0 || n_clips == 0 || n_channels == 0; }
// (an empty job is done, not refused — but a resident instance needs the largest message it must serve)
inline const char *job_empty_refusal(bool res) { return res ? "resident kernel: empty job" : nullptr; }
inline const char *job_resident_refusal(bool res, uint64_t cols) { return res && cols > kJobMaxCols ? "resident kernel: too many columns" : nullptr; }

// HIPSOXR_KERNEL_FFT_PCM is an explicit request for the frequency-domain engine on integer samples: whatever it cannot
// serve is an error, never a quiet run of the exact engine (whose results differ in the last bit).
inline const char *job_pcm_refusal(const JobSel &s, JobElem elem, bool vr_or_res)
{
    if (!s.want_pcm) return nullptr;
    if (vr_or_res) return "FFT engine: whole-signal device jobs only";
    if (elem != kJobElemPcm) return "HIPSOXR_KERNEL_FFT_PCM serves int16 / int32 jobs (float jobs have HIPSOXR_KERNEL_FFT / HIPSOXR_KERNEL_FFT_F64)";
    return nullptr;
}
// ... and the window it needs (fft_job_eligible: the one refusal that reads the plan)
constexpr const char *kJobPcmIneligible = "FFT engine (integer samples) needs a whole-signal job (in_abs0 == 0, out_k0 == 0) on an HQ/VHQ exact-ratio plan";

// float16 / bfloat16 samples: device jobs in float32 arithmetic
inline const char *job_half_refusal(const JobSel &s, JobElem elem, bool vr_or_res)
{
    if (elem != kJobElemHalf) return nullptr;
    if (vr_or_res) return "float16 / bfloat16 samples: device jobs only (streams take float32, float64, int32 and int16)";
    if (s.fft_f64) return "HIPSOXR_KERNEL_FFT_F64 serves float32 / float64 jobs (float16 / bfloat16 jobs compute in float32: HIPSOXR_KERNEL_FFT)";
    if (s.wave_dot)
        return "HIPSOXR_KERNEL_WAVE_DOT serves float32, float64, int32 and int16 jobs (float16 / bfloat16 jobs are not served by the reference-point kernel)";
    return nullptr;
}
inline const char *job_table_refusal(bool table, bool vr_or_res, int64_t in_abs0, int64_t out_k0)
{
    if (!table) return nullptr;
    if (vr_or_res) return "ragged batches: constant-rate device jobs only";
    if (in_abs0 != 0 || out_k0 != 0) return "ragged batches: whole signals only (in_abs0 == 0, out_k0 == 0)";
    return nullptr;
}
inline const char *job_fft_stream_refusal(const JobSel &s, bool vr_or_res) { return s.want_fft && vr_or_res ? "FFT engine: whole-signal device jobs only" : nullptr; }

// ---- clip rows -------------------------------------------------------------------------------------------------------------
// A clip table's rows are {in offset, in frames, out offset, out frames}.
constexpr int kRaggedRow = 4;
enum JobRowFault { kJobRowOk, kJobRowNegative, kJobRowAboveJob, kJobRowAbovePlan }; // (the first that holds, in this order)
enum JobRowDir { kJobRowForward, kJobRowAdjoint };

// sign and bounds: no negative offset or count, no count above the job's (the largest per-clip values)
inline JobRowFault job_row_bounds(const int64_t *row, int64_t job_in_frames, int64_t job_out_frames)
{
    if (row[0] < 0 || row[1] < 0 || row[2] < 0 || row[3] < 0) return kJobRowNegative;
    if (row[1] > job_in_frames || row[3] > job_out_frames) return kJobRowAboveJob;
    return kJobRowOk;
}
// ... and the plan's length rule, out_len = plan_out_len of this plan: forward out <= out_len(in); adjoint — in = the
// cotangent's n_y frames, out = the gradient's n_x — n_y <= out_len(n_x)
template <typename OutLen>
inline JobRowFault job_row_check(const int64_t *row, int64_t job_in_frames, int64_t job_out_frames, JobRowDir dir, OutLen out_len)
{
    if (const JobRowFault f = job_row_bounds(row, job_in_frames, job_out_frames)) return f;
    const int64_t produced = dir == kJobRowForward ? row[3] : row[1], from = dir == kJobRowForward ? row[1] : row[3];
    return (uint64_t)produced > (uint64_t)out_len((uint64_t)from) ? kJobRowAbovePlan : kJobRowOk;
}

// ---- the column fold ---------------------------------------------------------------------------------------------------------
// Kernels index (clip, channel) columns through grid.y (<= kJobMaxCols).  Wider jobs — the Python surface
// admits 65536 channels like the reference, src/soxr/__init__.py:22 — are folded into several
// launches over channel (or clip) ranges; columns are independent, so the result is the same.
// Not folded: a short constant-rate job of an interpolated-phase plan on channel-fast data.  launch_gather serves it whole
// with lane-per-output k_interp — consecutive lanes on consecutive channels of one frame, every load coalesced, the clips
// in grid.y — where the fold would run k_chain twice over columns a frame apart in memory (kWideLaneMaxOut: measured).
constexpr int64_t kWideLaneMaxOut = 4095; // outputs per column up to which a wide channel-fast job stays whole
inline bool job_wide_lane(uint64_t cols, bool phases, bool vr_or_res, uint32_t n_clips, int64_t in_chan_stride, int64_t out_frames, uint32_t n_channels,
                          const JobSel &s)
{
    return cols > kJobMaxCols && phases && !vr_or_res && n_clips <= kJobMaxCols && in_chan_stride == 1 && out_frames <= kWideLaneMaxOut &&
           out_frames * (int64_t)n_channels < ((int64_t)1 << 31) && (s.is_auto || s.exact_family);
}

// One range of a folded job: clips [clip0, clip0 + n_clips) x channels [ch0, ch0 + n_ch).  n_clips == 0: past the last range.
struct JobRange { uint32_t clip0 = 0, n_clips = 0, ch0 = 0, n_ch = 0; };
// How a job is folded: one clip range at a time where there is one channel or the clips alone are too many (clips and
// channels both wide: a range keeps every channel and is folded again, over its channels, when it re-enters), else ranges
// of step = kJobMaxCols / n_clips channels.
struct JobFold { uint32_t n_clips = 0, n_channels = 0, step = 0; bool by_clip = false; };
inline JobFold job_fold(uint32_t n_clips, uint32_t n_channels)
{
    JobFold f;
    f.n_clips = n_clips; f.n_channels = n_channels;
    f.by_clip = n_channels == 1 || n_clips > kJobMaxCols;
    f.step = f.by_clip ? kJobMaxCols : (n_clips ? kJobMaxCols / n_clips : 0);
    return f;
}
inline JobRange job_fold_range(const JobFold &f, uint64_t r)
{
    JobRange g;
    const uint64_t first = r * f.step, n = f.by_clip ? f.n_clips : f.n_channels;
    if (!f.step || r > n / f.step || first >= n) return g; // (r > n / step: first cannot wrap)
    const uint32_t count = (uint32_t)(n - first < f.step ? n - first : f.step);
    if (f.by_clip) { g.clip0 = (uint32_t)first; g.n_clips = count; g.ch0 = 0; g.n_ch = f.n_channels; }
    else { g.clip0 = 0; g.n_clips = f.n_clips; g.ch0 = (uint32_t)first; g.n_ch = count; }
    return g;
}

} // namespace hipsoxr
