// adjoint_fft_rules.h — the host rules of the adjoint on the frequency-domain engine (adjoint_fft.hip;
// HIPSOXR_KERNEL_ADJOINT_FFT): the TRANSPOSED PLAN of an exact-bank plan — its tap count and its bank — and what the two
// adjoint entries refuse of a job that names the selector, before the device is asked for anything.  No HIP, no globals, no
// switches(): the plan and the job's properties arrive as arguments (tests/c/adjoint_fft_rules_check.cpp reads every entry of
// the transposed bank back against the forward bank through plan.h's locate() and sweeps the refusals).
//
// Forward, per column:   y[k]  = sum_n x[n]  g(k M - n L),   g the prototype on the fine grid (L f_in = M f_out),
//                        bank[p][j] = g[L (T/2 - 1 - j) + p]                      (plan.h locate(): n = n0_k + j, p = (k M) mod L).
// Transpose:             gx[a] = sum_k gy[k] g(k M - a L) = sum_k gy[k] g'(a M' - k L'),   g'(u) = g(-u),  L' = M,  M' = L
// — the FORWARD of an ordinary exact-bank plan pt with out/in = L'/M' and bank'[s][i] = g'[L' (T'/2 - 1 - i) + s].  The forward
// bank occupies the fine-grid indices u in [-L T/2, L T/2 - 1]; g' occupies [-(L T/2 - 1), L T/2], and a bank of T' taps
// covers [-L' T'/2, L' T'/2 - 1]: T' is the smallest multiple of 8 with L' T'/2 >= max(u_max, 1 - u_min) = L T/2 + 1.
// bank' holds the same float64 values, each exactly once, and zeros where g has no sample: nothing is redesigned, so a
// bank installed from outside (hipsoxr_plan_set_bank) is honoured.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "job_rules.h"
#include "plan.h"

namespace hipsoxr {

// T' of the transposed plan of (L, M, T)
inline int32_t adj_fft_taps(int64_t L, int64_t M, int32_t T)
{
    const int64_t reach = L * (int64_t)(T / 2) + 1; // max(u_max, 1 - u_min) over the forward bank's fine-grid indices
    const int64_t half = (reach + M - 1) / M;       // T'/2 >= reach / L'
    return (int32_t)((2 * half + 7) / 8 * 8);
}

// bank' as [M][T'] float64 (exact-bank plans: p.phases == 0)
inline std::vector<double> adj_fft_bank(const Plan &p)
{
    const int64_t L = p.L, M = p.M, H = p.T / 2;
    const int32_t Tt = adj_fft_taps(L, M, p.T);
    std::vector<double> b((size_t)M * (size_t)Tt, 0.0);
    for (int64_t s = 0; s < M; ++s)
        for (int32_t i = 0; i < Tt; ++i) {
            const int64_t u = -(M * (int64_t)(Tt / 2 - 1 - i) + s); // g'(u') = g(-u')
            if (u < -L * H || u > L * H - 1) continue;                // g has no sample there
            const int64_t w = u + L * H, ph = w % L, j = p.T - 1 - w / L; // u = L (T/2 - 1 - j) + ph
            b[(size_t)s * (size_t)Tt + (size_t)i] = p.bank[(size_t)(ph * p.T + j)];
        }
    return b;
}

// ---- refusals that need no device state -----------------------------------------------------------------------------------
// What the entries ask of a job that names the selector, in this order (ragged: hipsoxr_run_device_adjoint_ragged).  half:
// float16 / bfloat16 (the equal-length entry widens such a job and asks for the float32 one); real: float32 / float64;
// below_hq: the recipe's stop band is above -120 dB; window: in_abs0 or out_k0 is not 0; table: the job has a clip_table.
struct AdjFftAsk { bool half, real, vr, phases, below_hq, window, table; };
constexpr double kAdjFftMinAttDb = 120.; // (fft.hip fft_job_eligible: what the method neglects is the stop band's aliasing)
constexpr const char *kAdjFftUnavailable =
    "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: the frequency-domain engine is unavailable for this plan or layout (the transposed ratio is outside its schedule "
    "table and k_fft_block does not take the job); HIPSOXR_KERNEL_AUTO runs the exact engine's adjoint";
inline const char *adj_fft_refusal(bool ragged, const AdjFftAsk &q)
{
    if (ragged && q.half) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: ragged: float16 / bfloat16 clip tables are not served (half cotangents clip by clip through hipsoxr_run_device_adjoint)";
    if (!q.real) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT serves float32 or float64 elements (integer types have no gradient)";
    if (q.vr) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: variable-rate plans are not served";
    if (q.phases) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT needs an exact-bank plan (interpolated-phase plans are served by HIPSOXR_KERNEL_ADJOINT, on the exact engine)";
    if (q.below_hq) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: the frequency-domain engine serves HQ and VHQ only (recipes below 120 dB are not 1e-6-class on it)";
    if (q.window) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: whole cotangents only (in_abs0 == 0, out_k0 == 0)";
    if (!ragged && q.table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: a clip_table is served by hipsoxr_run_device_adjoint_ragged, not by this entry";
    if (ragged && !q.table) return "adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT: the ragged entry needs a clip_table (equal-length clips: hipsoxr_run_device_adjoint)";
    return nullptr;
}
// ... and what the forward entries answer to the selector
constexpr const char *kAdjFftForwardRefusal =
    "HIPSOXR_KERNEL_ADJOINT_FFT selects the transposed operator on the frequency-domain engine: it is valid on hipsoxr_run_device_adjoint and "
    "hipsoxr_run_device_adjoint_ragged only (forward jobs have HIPSOXR_KERNEL_FFT)";

} // namespace hipsoxr
