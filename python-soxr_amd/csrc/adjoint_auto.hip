// adjoint_auto.hip — HIPSOXR_KERNEL_ADJOINT_AUTO on hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged: the
// transpose of the job the forward launches under HIPSOXR_KERNEL_AUTO for the same plan and shape.  No kernel lives here and
// no launch: the entries make the selector's refusals by name (what HIPSOXR_KERNEL_ADJOINT refuses), ask adjoint_auto_rules.h
// which engine the forward job would run on, and call the inner function of that engine's adjoint launcher —
//   adj_fft_try                      (adjoint_fft.hip)  exact-bank plans the frequency-domain engine takes
//   launch_adjoint_two_stage_try     (twostage.hip)     equal-length jobs of interpolated-phase plans on the two-stage form
//   launch_adjoint_two_stage_ragged  (twostage.hip)     a clip table of such a plan: per clip, two-stage or exact
//   adj_exact_run                    (adjoint.hip)      the exact adjoint: everything else
// Each fast launcher reports "not handled" with nothing written to gx; the exact adjoint then computes the job, so the
// selector never answers "unavailable".  Where it resolves to a named selector the launch — and the bits — are that selector's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "adjoint_auto_rules.h"
#include "adjoint_fft_rules.h" // kAdjFftMinAttDb
#include "adjoint_rules.h"     // adj_extent_refusal, adj_row_refusal: the length rules are the exact adjoint's
#include "device.h"
#include "job_rules.h"

namespace hipsoxr {

static AdjAutoAsk adj_auto_ask(const Plan &p, const hipsoxr_job_t &j)
{
    AdjAutoAsk q;
    q.half = elem_is_half(j.elem);
    q.real = j.elem == HIPSOXR_F32 || j.elem == HIPSOXR_F64;
    q.vr = p.vr;
    q.window = j.in_abs0 != 0 || j.out_k0 != 0;
    q.table = j.clip_table != nullptr;
    return q;
}
// ... what both entries ask last, of a job that is not empty
static const char *adj_auto_device_refusal(const hipsoxr_job_t &j)
{
    if (!j.out || (j.in_frames > 0 && !j.in)) return "null buffer";
    return device_count() <= 0 ? kNoDevice : nullptr;
}
// the decision's inputs that do not depend on the entry (form_ok / admits: the two-stage launchers ask those themselves, of
// the plan's device-side form — true here means "offer the job")
static AdjAutoJob adj_auto_job(const Plan &p, int64_t total_out)
{
    return AdjAutoJob{p.phases != 0, p.att_db < kAdjFftMinAttDb, total_out, switches().no_fft, switches().no_two_stage, true, true};
}

const char *launch_adjoint_auto(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    if (elem_is_half(j.elem)) {
        // float16 / bfloat16: the float32 job of this selector on the widened cotangent, rounded once (half.hip) — the
        // refusals by name and the empty job first, asked of the float32 job without clips
        hipsoxr_job_t f = j;
        f.elem = HIPSOXR_F32; f.n_clips = 0;
        if (const char *e = launch_adjoint_auto(p, f, stream)) return e;
        if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
        if (const char *e = adj_auto_device_refusal(j)) return e;
        return launch_half(p, j, stream, true);
    }
    if (const char *e = adj_auto_refusal(false, adj_auto_ask(*p, j))) return e;
    if (const char *e = adj_extent_refusal(kAdjEqual, j.in_frames, j.out_frames, [&](uint64_t n) { return plan_out_len(*p, n); })) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_auto_device_refusal(j)) return e;
    const AdjAutoEngine engine = adj_auto_engine(adj_auto_job(*p, adj_auto_total_equal(j.in_frames, j.n_clips, j.n_channels)));
    bool handled = false;
    if (engine == kAdjAutoFft)
        if (const char *e = adj_fft_try(p, j, stream, nullptr, &handled)) return e;
    if (engine == kAdjAutoTwoStage)
        if (const char *e = launch_adjoint_two_stage_try(p, j, stream, &handled)) return e;
    return handled ? nullptr : adj_exact_run(p, j, stream, nullptr, false);
}

const char *launch_adjoint_auto_ragged(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    const auto out_len = [&](uint64_t n) { return plan_out_len(*p, n); };
    if (const char *e = adj_auto_refusal(true, adj_auto_ask(*p, j))) return e;
    for (uint32_t c = 0; c < j.n_clips; ++c)
        if (const char *e = adj_row_refusal(job_row_check(j.clip_table + kRaggedRow * (size_t)c, j.in_frames, j.out_frames, kJobRowAdjoint, out_len))) return e;
    if (const char *e = adj_extent_refusal(kAdjRagged, j.in_frames, j.out_frames, out_len)) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_auto_device_refusal(j)) return e;
    const AdjAutoEngine engine = adj_auto_engine(adj_auto_job(*p, adj_auto_total_table(j.clip_table, j.n_clips, j.n_channels)));
    bool handled = false;
    if (engine == kAdjAutoTwoStage) { // (derived tables of its own: the caller's device copy cannot serve)
        if (const char *e = launch_adjoint_two_stage_ragged(p, j, stream, &handled)) return e;
        if (handled) return nullptr;
    }
    // the frequency-domain engine and the exact adjoint read the DEVICE copy of the caller's table
    const int64_t *rows = nullptr;
    void *tmp = nullptr;
    static constexpr ClipTableTexts texts = {kAdjAutoTableNoMemory, kAdjAutoTableUploadFailed};
    if (const char *e = clip_table_device(j, stream, &rows, &tmp, texts)) return e;
    const char *e = nullptr;
    if (engine == kAdjAutoFft) e = adj_fft_try(p, j, stream, rows, &handled);
    if (!e && !handled) e = adj_exact_run(p, j, stream, rows, false);
    if (tmp) (void)hipFreeAsync(tmp, (hipStream_t)stream);
    return e;
}

} // namespace hipsoxr
