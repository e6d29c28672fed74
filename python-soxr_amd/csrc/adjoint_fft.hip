// adjoint_fft.hip — the transposed operator on the frequency-domain engine (HIPSOXR_KERNEL_ADJOINT_FFT on
// hipsoxr_run_device_adjoint and hipsoxr_run_device_adjoint_ragged).  No kernel lives here: gx = A^T gy is the FORWARD job of
// the plan's TRANSPOSED PLAN pt (adjoint_fft_rules.h: L' = M, M' = L, the prototype mirrored, the same float64 values), and
// fft.hip runs it — k_fft_pair2, k_fft_strided2, k_fft_wave, k_fft_block, whatever launch_fft serves for a float job of that
// shape by name (HIPSOXR_KERNEL_FFT semantics): unit-stride columns, channel pairs, strided columns, the one-round rows, a
// clip table in one launch.  fft_build derives H, the kept run and the row choice from pt's L, M, T and bank alone.
//
// The job is read in the adjoint's direction — in = gy (n_y frames, zero-extended), out = gx (n_x frames) — and n_y <=
// out_len(n_x) of the FORWARD plan is all that is asked of the lengths: pt's own forward length rule (fft_job_eligible) is
// not applied, n_x may exceed pt's output length for n_y.  The kernels bound every load by the column's n_y (a block behind
// the cotangent's end reads zeros through an empty buffer range) and every store by its n_x, so every element of gx is
// written and nothing outside it.  Where the engine declines (*handled == false) the call fails with kAdjFftUnavailable:
// the exact adjoint never runs in its place.  Precision: the forward engine's own class on pt, 1e-6 (float32) / 2e-9 VHQ,
// 1e-6 HQ (float64) relative RMS against the float64 direct form.
//
// pt is a real Plan (phases = 0; the forward's att_db, q and device), built on first use under the forward plan's mutex and
// kept beside the exact adjoint's tables: adjoint_release drops it — hipsoxr_plan_set_bank, hipsoxr_plan_broadcast, plan
// deletion — and its own FFT tables go with it (Plan::~Plan).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "adjoint_fft_rules.h"
#include "adjoint_rules.h" // adj_extent_refusal, adj_row_refusal: the length rules are the exact adjoint's
#include "device.h"
#include "job_rules.h"

namespace hipsoxr {

struct AdjFftPlan { const Plan *owner; Plan *pt; };
static std::mutex g_adjfft_mu;
static std::vector<AdjFftPlan> g_adjfft; // one per forward plan

void adjoint_fft_release(const Plan *p)
{
    Plan *pt = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_adjfft_mu);
        for (size_t i = 0; i < g_adjfft.size(); ++i)
            if (g_adjfft[i].owner == p) { pt = g_adjfft[i].pt; g_adjfft.erase(g_adjfft.begin() + i); break; }
    }
    delete pt; // (outside the lock: Plan::~Plan comes back here for pt itself)
}

// The transposed plan of an exact-bank plan (the two-stage form's adjoint builds its FFT stage's the same way)
Plan *adj_fft_transposed(const Plan &p)
{
    Plan *pt = new Plan();
    pt->in_rate = p.out_rate; pt->out_rate = p.in_rate;
    pt->recipe = p.recipe; pt->q = p.q; pt->att_db = p.att_db; pt->beta = p.beta;
    pt->L = p.M; pt->M = p.L; pt->T = adj_fft_taps(p.L, p.M, p.T);
    pt->phases = 0; pt->vr = false;
    pt->bank = adj_fft_bank(p);
    pt->custom_bank = p.custom_bank;
    pt->device = p.device;
    return pt;
}

// The plan's transposed plan, built on first use (exact-bank plans; the caller has checked).
static const char *adj_fft_ensure(Plan *p, Plan **out)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return kNoDevice;
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->device >= 0 && cur != p->device) return "this plan's device tables live on another device (one plan per device)";
    if (p->device < 0) p->device = cur;
    std::lock_guard<std::mutex> lk2(g_adjfft_mu);
    for (const AdjFftPlan &e : g_adjfft)
        if (e.owner == p) { *out = e.pt; return nullptr; }
    Plan *pt = adj_fft_transposed(*p);
    g_adjfft.push_back({p, pt});
    *out = pt;
    return nullptr;
}

static AdjFftAsk adj_fft_ask(const Plan &p, const hipsoxr_job_t &j)
{
    AdjFftAsk q;
    q.half = elem_is_half(j.elem);
    q.real = j.elem == HIPSOXR_F32 || j.elem == HIPSOXR_F64;
    q.vr = p.vr; q.phases = p.phases != 0;
    q.below_hq = p.att_db < kAdjFftMinAttDb;
    q.window = j.in_abs0 != 0 || j.out_k0 != 0;
    q.table = j.clip_table != nullptr;
    return q;
}
// ... what both entries ask last, of a job that is not empty
static const char *adj_fft_device_refusal(const hipsoxr_job_t &j)
{
    if (!j.out || (j.in_frames > 0 && !j.in)) return "null buffer";
    return device_count() <= 0 ? kNoDevice : nullptr;
}

// The float job of pt the engine runs: by name, no integer output stage.  rows: the device copy of a clip table, or NULL.
// *handled_out = false with no error: the engine declined before anything was queued (HIPSOXR_KERNEL_ADJOINT_AUTO then runs the
// exact adjoint: adjoint_auto.hip).
const char *adj_fft_try(Plan *p, const hipsoxr_job_t &j, void *stream, const int64_t *rows, bool *handled_out)
{
    *handled_out = false;
    Plan *pt = nullptr;
    if (const char *e = adj_fft_ensure(p, &pt)) return e;
    hipsoxr_job_t f = j;
    f.kernel = HIPSOXR_KERNEL_FFT;
    f.clip_counter = nullptr; f.dither = 0; f.dither_seed = 0;
    f.clip_table_dev = rows;
    bool handled = false;
    if (const char *e = launch_fft(pt, f, stream, &handled)) return e;
    *handled_out = handled;
    return nullptr;
}
// ... by name: a decline is an error
static const char *adj_fft_run(Plan *p, const hipsoxr_job_t &j, void *stream, const int64_t *rows)
{
    bool handled = false;
    if (const char *e = adj_fft_try(p, j, stream, rows, &handled)) return e;
    return handled ? nullptr : kAdjFftUnavailable;
}

const char *launch_adjoint_fft(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    if (elem_is_half(j.elem)) {
        // float16 / bfloat16: the float32 job of this selector on the widened cotangent, rounded once (half.hip) — the
        // refusals by name and the empty job first, asked of the float32 job without clips
        hipsoxr_job_t f = j;
        f.elem = HIPSOXR_F32; f.n_clips = 0;
        if (const char *e = launch_adjoint_fft(p, f, stream)) return e;
        if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
        if (const char *e = adj_fft_device_refusal(j)) return e;
        return launch_half(p, j, stream, true);
    }
    if (const char *e = adj_fft_refusal(false, adj_fft_ask(*p, j))) return e;
    if (const char *e = adj_extent_refusal(kAdjEqual, j.in_frames, j.out_frames, [&](uint64_t n) { return plan_out_len(*p, n); })) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_fft_device_refusal(j)) return e;
    return adj_fft_run(p, j, stream, nullptr);
}

// The ragged entry: rows { gy offset, n_y, gx offset, n_x } are the forward's rows { in offset, in frames, out offset, out
// frames } of a table of pt — one launch through the ragged forms the engine has.
const char *launch_adjoint_fft_ragged(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    const auto out_len = [&](uint64_t n) { return plan_out_len(*p, n); };
    if (const char *e = adj_fft_refusal(true, adj_fft_ask(*p, j))) return e;
    for (uint32_t c = 0; c < j.n_clips; ++c)
        if (const char *e = adj_row_refusal(job_row_check(j.clip_table + kRaggedRow * (size_t)c, j.in_frames, j.out_frames, kJobRowAdjoint, out_len))) return e;
    if (const char *e = adj_extent_refusal(kAdjRagged, j.in_frames, j.out_frames, out_len)) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_fft_device_refusal(j)) return e;
    const int64_t *rows = nullptr;
    void *tmp = nullptr;
    static constexpr ClipTableTexts texts = {"adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: ragged: no device memory for the clip table",
                                             "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: ragged: clip table upload failed"};
    if (const char *e = clip_table_device(j, stream, &rows, &tmp, texts)) return e;
    const char *e = adj_fft_run(p, j, stream, rows);
    if (tmp) (void)hipFreeAsync(tmp, (hipStream_t)stream);
    return e;
}

} // namespace hipsoxr
