// adjoint.hip — the transposed polyphase operator on CDNA4 (gfx950): gx = A^T gy for the forward job A that the exact
// engine computes on the same plan (hipsoxr_run_device_adjoint; the gradient of soxr_amd.device.resample_tensor).
// Hand-written HIP, host and device side in one translation unit, compiled with -ffp-contract=off like the exact engine.
//
// Forward, per column (plan.h locate()):   y[k] = sum_{j<T} c[p_k][j] x[n0_k + j],
//     n0_k = floor(k M / L) - (T/2 - 1),  p_k = (k M) mod L,  x zero outside [0, n_x).
// Adjoint:   gx[a] = sum over { k in [0, n_y) : 0 <= a - n0_k < T } of c[p_k][a - n0_k] gy[k].
// It is periodic in a with period M.  With a = q M + s (0 <= s < M) and k = q L + d the terms of phase s are
//     d_lo(s) = ceil((s - T/2) L / M)  <=  d  <=  d_hi(s) = ceil((s + T/2) L / M) - 1        (d may be negative or >= L)
//     tap j = s + T/2 - 1 - floor(d M / L),   forward phase (d M) mod L                      (mathematical floor and mod)
// at most Tt = max_s (d_hi(s) - d_lo(s) + 1) <= ceil(T L / M) + 1 of them.  A TRANSPOSED BANK ct (Tt entries per phase,
// zero behind a phase's last term) and the start table d_lo[M] turn the adjoint into a gather-form polyphase filter with M
// phases — no scatter, no atomics:
//     gx[q M + s] = sum_{i<Tt} ct[s][i] gy[q L + d_lo(s) + i],     gy zero outside [0, n_y).
//
// ARITHMETIC: every gx element is ONE fma chain in the element's own width over ascending k, started from +0.  The tables
// of the tiled kernel hold extra zeros in front of and behind a phase's terms; fma(0, gy, acc) == acc for finite gy, so FOR
// FINITE COTANGENTS both kernels below give the same bits and a result does not depend on layout, tiling or launch shape.
// The float32 tables are the float64 bank rounded to nearest — the values the float32 forward engine multiplies by: forward
// and adjoint are transposes of one matrix.
//
// REACH of a non-finite cotangent sample: 0 * inf = NaN, so an infinite or NaN gy[k] makes every gx[a] non-finite whose
// chain multiplies it, by a table zero or not.  The true support of gy[k] is 0 <= a - n0_k < T, i.e. |a - k M/L| <= T/2.
//   k_adj_gather  gx[a] reads gy[lo(a) .. lo(a) + Tt - 1], lo(a) = ceil((a - T/2) L / M): Tt is the maximum over phases,
//                 so a phase with fewer terms reads on behind its last one.  k >= lo(a) gives a <= k M/L + T/2, and
//                 k <= lo(a) + Tt - 1 with Tt <= ceil(T L/M) + 1 < T L/M + 2 gives a > k M/L + T/2 - Tt M/L:
//                     -(T/2 + 2 M/L) < a - k M/L <= T/2.
//   k_adj_tile    all 16 phases of a wave tile read gy[lo(a0) .. lo(a0) + I - 1], a0 <= a <= a0 + 15 the tile's first frame;
//                 I is the maximum over tiles of the span from the first term of the tile's first phase to the last term
//                 of its last, rounded up to a multiple of 4: I < (T + 15) L/M + 4.  The same two steps on a0 give
//                     -(T/2 + 15 + 4 M/L) < a - k M/L <= T/2 + 15.
// Every gx[a] outside these intervals (and every other column) never reads gy[k]: it has the bits it would have with any
// finite value there.  Which elements inside them turn non-finite depends on the kernel, hence on the launch form
// (tests/test_gpu_adjoint_forms.py pins both sides).
//
// Kernels:
//   k_adj_gather  one lane per gx element; transposed bank tap-major [Tt][M] (lanes of neighbouring phases read
//                 neighbouring words), gy straight from global memory.  Every exact-bank plan, layout and length; what
//                 short jobs and plans whose period does not fit LDS run on.
//   k_adj_tile    the period-tiled form (the k_tile family's shape, kernels_tile.h): a workgroup takes a span of whole input
//                 periods of one column — or of a group of interleaved channels, read as whole frames — and stages the gy
//                 slab those periods touch in LDS, zero-filled outside [0, n_y).  A lane owns one (period, channel); a
//                 wave owns 16 consecutive phases, whose coefficients travel on the scalar path (s_load -> SGPR operands
//                 of the FMAs) from a per-tile table [I][16] skewed to the tile's first gy sample and zero-padded: one
//                 LDS read feeds 16 FMAs.
//   k_adj_interp  interpolated-phase plans (Plan.phases != 0), asked for by name: HIPSOXR_KERNEL_ADJOINT.  There is no bank
//                 to transpose: the coefficient of gy[k] in gx[a] is tap j = a - q_k + T/2 - 1 of the cubic the forward
//                 evaluates for output k (kernels_interp.h k_interp: t = k M, q_k = t div L, r = t mod L, iv = (r P) div L,
//                 xx = (((r P) mod L) << SH) div L * 2^-SH, c_j = fma(fma(fma(a3, xx, a2), xx, a1), xx, a0) from the plan's
//                 device table [P][T]) — the same table, the same integer arithmetic, the same fma nesting, so the very bits
//                 the forward multiplies by.  Gather form:
//                     gx[a] = sum_{k = k_lo(a)}^{k_hi(a)} c_{a - q_k + T/2 - 1}(k) gy[k],
//                     k_lo(a) = max(0, ceil((a - T/2) L / M)),   k_hi(a) = min(n_y, ceil((a + T/2) L / M)) - 1,
//                 at most ceil(T L / M) + 1 terms, one fma chain over ascending k from +0.  A workgroup takes a tile of
//                 kAdjIW consecutive frames of one column and walks the tile's contiguous k range in chunks of kAdjIC: per
//                 chunk every thread locates ONE k (the 64-bit divisions are per k, not per (a, k)) and stages its record
//                 (q_k - a0, iv T, xx, gy[k]) in LDS — constant LDS whatever L / M.  Then each wave walks the UNION of its
//                 64 lanes' k ranges inside the chunk: at one k all lanes sit in ONE table row and lane a reads tap
//                 j(a) — 64 neighbouring 16- / 32-byte records, whole lines — and a lane whose j falls outside [0, T) keeps
//                 its sum (a select, not a multiplication by zero).
//                 REACH: 0 <= j < T is exactly a - T/2 <= q_k <= a + T/2 - 1, the true support of gy[k]: a lane never
//                 multiplies outside its own [k_lo, k_hi], there is no padding and no 0 * inf.  A non-finite gy[k] reaches
//                 the gx[a] of its true support and nothing else — tighter than the two exact-bank kernels above.
//
// RAGGED batches (hipsoxr_run_device_adjoint_ragged): every kernel has a second instantiation, `bool RAGGED`, that serves
// clips of unequal length in ONE launch.  A column's clip reads its row { gy offset, n_y, gx offset, n_x } from a device copy
// of the job's clip table; the row stands where the equal-length form has clip * ics, a.n_y, clip * ocs and a.n_x.  The
// grid's frame axis is sized by the LONGEST clip, and a workgroup (k_adj_gather: a lane) whose tile, periods or frame start
// at or behind its clip's n_x does nothing for that column — a decision that is uniform over the workgroup, so no barrier is
// ever met by part of one.  Every element of every clip's gx[0, n_x[c]) is written (zeros where n_y[c] == 0) and nothing
// else: not the elements between packed clips.  All offsets are 64-bit.  The equal-length instantiations are the code they
// were.  FORM: the tiled kernel when the plan has tile tables and the LONGEST clip has at least kAdjMinPeriods * Mc frames —
// the short clips of such a launch run on it too, it is correct at any length — else the lane-per-element kernel.  By
// ARITHMETIC above each clip has, for finite cotangents, the bits of the same clip run alone, whichever form either took.
// REACH of a non-finite gy[k] of clip c: inside clip c only, the interval above of the form THE RAGGED LAUNCH took (a short
// clip in a tiled launch has k_adj_tile's reach, although alone it would run k_adj_gather); k_adj_interp: the true support.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

#include "adjoint_rules.h" // kAdjRS, floor_div, ceil_div; the tables, the launch forms, the refusals
#include "device.h"
#include "job_rules.h"
#include "poly_adj_rules.h" // kPolyAdjRaggedRefusal
#include "vr_adjoint_rules.h" // vr_adj_k_range, vr_adj_grid

namespace hipsoxr {

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return hipGetErrorString(e_); \
    } while (0)

struct AdjArgs {
    const void *gy;
    void *gx;
    const void *ct;       // k_adj_gather: [Tt][M] Real
    const int32_t *d_lo;  // k_adj_gather: [M]
    const void *tab;      // k_adj_tile: [n_st][I][16] Real, constant address space
    const int32_t *e0;    // k_adj_tile: [n_st] first gy sample of a tile's table, relative to the slab's first
    int64_t L, M;         // out/in = L/M
    int64_t Lc, Mc;       // k_adj_tile: the period replicated c times (Mc inputs <- Lc cotangent samples)
    int32_t Tt, n_st, I, dmin;
    int32_t x_count;      // frames staged per workgroup
    int32_t pad;          // LDS row padding (frames): rows of Lc + pad frames, an odd number
    int32_t pb, cg;       // periods and channels per workgroup (pb * cg <= 64 lanes)
    int32_t cg_shift;     // log2(cg), or -1
    int32_t n_waves;      // waves that share a workgroup's phase tiles
    int32_t inter;        // k_adj_gather: channel index fastest (interleaved frames)
    uint32_t n_clips, n_channels, n_groups;
    int64_t ics, ifs, ichs, ocs, ofs, ochs;
    int64_t n_y, n_x;     // RAGGED: the largest per-clip values (n_x sizes the grid's frame axis)
};
// The RAGGED instantiations take the table behind the same arguments (the equal-length kernels keep their argument block).
struct AdjRaggedArgs : AdjArgs {
    const int64_t *rows;  // [n_clips][4] = gy offset, n_y, gx offset, n_x (device copy of hipsoxr_job_t::clip_table):
                          // a row replaces clip * ics, a.n_y, clip * ocs, a.n_x
};
template <bool RAGGED> struct AdjArgsOf { typedef AdjArgs type; };
template <> struct AdjArgsOf<true> { typedef AdjRaggedArgs type; };

__device__ __forceinline__ float fma_r(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---------------------------------------------------------------------------------------------
// k_adj_gather
// ---------------------------------------------------------------------------------------------
// RAGGED: the (frame, channel) of a lane is decomposed with the LONGEST clip's n_x (a.n_x); the clip loop strides gridDim.y,
// so one lane meets clips of different lengths and asks `fr < n_x[clip]` for each.
template <typename Real, bool RAGGED>
__global__ void __launch_bounds__(256) k_adj_gather(typename AdjArgsOf<RAGGED>::type a)
{
    const int64_t per_clip = a.n_x * (int64_t)a.n_channels;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= per_clip) return;
    int64_t fr, ch;
    if (a.inter) { fr = idx / a.n_channels; ch = idx - fr * a.n_channels; }
    else { ch = idx / a.n_x; fr = idx - ch * a.n_x; }
    const int64_t q = fr / a.M;
    const int64_t s = fr - q * a.M;
    const int64_t k0 = q * a.L + a.d_lo[s];
    const Real *c = (const Real *)a.ct + s;
    for (uint32_t clip = blockIdx.y; clip < a.n_clips; clip += gridDim.y) {
        const int64_t *row = nullptr; // the clip's row; the equal-length form has none
        if constexpr (RAGGED) row = a.rows + 4 * (int64_t)clip;
        if (RAGGED && fr >= row[3]) continue;
        const int64_t n_y = RAGGED ? row[1] : a.n_y;
        const Real *g = (const Real *)a.gy + (RAGGED ? row[0] : (int64_t)clip * a.ics) + ch * a.ichs;
        Real acc = 0;
        for (int32_t i = 0; i < a.Tt; ++i) {
            const int64_t k = k0 + i;
            const Real v = (k >= 0 && k < n_y) ? g[k * a.ifs] : (Real)0;
            acc = fma_r(c[(int64_t)i * a.M], v, acc);
        }
        ((Real *)a.gx)[(RAGGED ? row[2] : (int64_t)clip * a.ocs) + fr * a.ofs + ch * a.ochs] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// k_adj_tile
// ---------------------------------------------------------------------------------------------
// Geometry (host-built, adjoint_rules.h adj_tables): "period" is the replicated period, Mc = c M inputs <- Lc = c L
// cotangent samples, c such that Mc >= 16 and Lc >= 64.  Workgroup x takes periods [x pb, x pb + pb); its slab holds gy frames
// [x pb Lc + dmin, + x_count) of cg channels, frame n of it at LDS element (n + pad (n / Lc)) cg + channel: rows of
// Lc + pad frames — an odd count, so that the lanes of a wave (stride one row) fall on different banks.  Phase tile st
// (phases s = 16 st .. 16 st + 15) reads slab frames e0[st] + ii (ii < I) of its lane's period, coefficient tab[st][ii][s].
// RAGGED: a workgroup whose periods start at or behind its clip's n_x skips the column — a workgroup-uniform decision
// (blockIdx.x and the clip's row) — so the barrier in front of staging fires only once an earlier column of this workgroup
// has staged a slab.  A clip shorter than 4 Mc frames is served like any other: the kernel is correct at any length.
template <typename Real, bool RAGGED>
__global__ void __launch_bounds__(1024) k_adj_tile(typename AdjArgsOf<RAGGED>::type a)
{
    constexpr int RS = kAdjRS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Real *xs = reinterpret_cast<Real *>(smem_raw);
    typedef const __attribute__((address_space(4))) Real *CPtr;

    const int32_t Lc = (int32_t)a.Lc, Mc = (int32_t)a.Mc, pad = a.pad, cg = a.cg, pb = a.pb;
    const int64_t q0 = (int64_t)blockIdx.x * pb; // first period of this workgroup
    const int64_t g0 = q0 * a.Lc + a.dmin;       // gy frame of slab frame 0
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_all = (int)(blockDim.x >> 6);
    const int32_t per = a.cg_shift >= 0 ? lane >> a.cg_shift : lane / cg, c = lane - per * cg;
    const bool live = per < pb;
    const int32_t rows = (a.x_count + Lc - 1) / Lc;
    const int32_t row_elems = Lc * cg;
    [[maybe_unused]] bool staged = false; // RAGGED: an earlier column of this workgroup staged a slab (uniform)

    for (uint32_t y = blockIdx.y; y < a.n_clips * a.n_groups; y += gridDim.y) {
        // (run-time division goes through the vector ALU; readfirstlane keeps the results on the scalar side)
        const uint32_t clip = __builtin_amdgcn_readfirstlane(y / a.n_groups);
        const uint32_t ch0 = __builtin_amdgcn_readfirstlane((y - clip * a.n_groups) * (uint32_t)cg);
        const int32_t ncg = (int32_t)min((uint32_t)cg, a.n_channels - ch0); // channels of this group that exist
        const int64_t *row = nullptr; // the clip's row (clip is wave-uniform: scalar loads); the equal-length form has none
        if constexpr (RAGGED) row = a.rows + 4 * (int64_t)clip;
        if constexpr (RAGGED)
            if (q0 * a.Mc >= row[3]) continue; // nothing of this clip in this workgroup's periods
        const Real *g = (const Real *)a.gy + (RAGGED ? row[0] : (int64_t)clip * a.ics) + (int64_t)ch0 * a.ichs;
        if constexpr (RAGGED) {
            if (staged) __syncthreads(); // the slab of the column before — the last one not skipped — is still being read
            staged = true;
        } else if (y != blockIdx.y) __syncthreads(); // the slab of the column before is still being read

        // stage: a wave per slab row, lanes along the row's (frame, channel) elements — whole frames of an interleaved
        // tensor are read as they lie in memory
        for (int32_t r = wave; r < rows; r += n_all) {
            Real *dst = xs + (size_t)r * (size_t)((Lc + pad) * cg);
            for (int32_t e = lane; e < row_elems; e += 64) {
                const int32_t j = a.cg_shift >= 0 ? e >> a.cg_shift : e / cg, cc = e - j * cg;
                const int32_t n = r * Lc + j;
                if (n < a.x_count) {
                    const int64_t f = g0 + n;
                    dst[e] = (cc < ncg && f >= 0 && f < (RAGGED ? row[1] : a.n_y)) ? g[f * a.ifs + (int64_t)cc * a.ichs] : (Real)0;
                }
            }
        }
        __syncthreads();

        const Real *xl = xs + (size_t)((live ? per : 0) * (Lc + pad) * cg + c); // this lane's (period, channel)
        Real *const go = (Real *)a.gx + (RAGGED ? row[2] : (int64_t)clip * a.ocs) + (int64_t)(ch0 + c) * a.ochs;
        const int64_t a0 = (q0 + per) * a.Mc; // first input frame of this lane's period
        const bool store = live && c < ncg;

        // (few workgroups: the phase tiles of a slab are spread over gridDim.z workgroups, each staging the slab)
        for (int st_ = wave < a.n_waves ? wave + a.n_waves * (int)blockIdx.z : a.n_st; st_ < a.n_st; st_ += a.n_waves * (int)gridDim.z) {
            // keep the tile index (and everything derived from it) provably wave-uniform: the coefficient loads below
            // must be scalar (s_load), not per-lane
            const int st = __builtin_amdgcn_readfirstlane(st_);
            const int32_t e0 = __builtin_amdgcn_readfirstlane(a.e0[st]);
            CPtr t = (CPtr)((const Real *)a.tab + (size_t)st * a.I * RS);
            Real acc[RS];
#pragma unroll
            for (int rr = 0; rr < RS; ++rr) acc[rr] = 0;
            // slab frame m of this lane's period lies at element (m + pad * (m / Lc)) * cg of its row: m walks upwards, the
            // row crossings are counted on the scalar side
            const int32_t row0 = __builtin_amdgcn_readfirstlane(e0 / Lc);
            int32_t m = e0, next = (row0 + 1) * Lc, off = (e0 + pad * row0) * cg;
            for (int32_t qd = 0; qd < a.I; qd += 4) {
                Real x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[u] = xl[off];
                    ++m; off += cg;
                    if (m == next) { off += pad * cg; next += Lc; }
                }
                CPtr tq = t + (size_t)qd * RS;
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int rr = 0; rr < RS; ++rr) acc[rr] = fma_r(tq[u * RS + rr], x[u], acc[rr]);
            }
            const int32_t s0 = st * RS;
#pragma unroll
            for (int rr = 0; rr < RS; ++rr) {
                const int64_t fr = a0 + s0 + rr;
                if (store && s0 + rr < Mc && fr < (RAGGED ? row[3] : a.n_x)) go[fr * a.ofs] = acc[rr];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_adj_interp
// ---------------------------------------------------------------------------------------------
static constexpr int kAdjIW = 256; // gx frames per workgroup tile (one per thread)
static constexpr int kAdjIC = 256; // cotangent samples located and staged per chunk (one per thread)

struct AdjInterpArgs {
    const void *gy;
    void *gx;
    const void *tab; // the plan's device table [P][T] of Vec4<Real> (a0..a3), the forward's own
    int64_t L, M;
    int32_t T, P;
    uint64_t n_cols; // clips x channels
    uint32_t n_channels;
    int64_t ics, ifs, ichs, ocs, ofs, ochs;
    int64_t n_y, n_x;    // RAGGED: the largest per-clip values
};
struct AdjInterpRaggedArgs : AdjInterpArgs { const int64_t *rows; }; // as AdjRaggedArgs::rows
// VR (hipsoxr_run_device_vr_ragged_adjoint): a second table behind the arguments, a clip's clock — its Q64.64 step {hi, lo};
// T0 = 0, D = 0 — as kernels_interp.h's InterpArgsR::clock; L and M are not read
struct AdjInterpVrArgs : AdjInterpRaggedArgs {
    const uint64_t *clock; // [n_clips][2]
    int32_t lgP;           // P = 1 << lgP
};
template <bool RAGGED, bool VR = false> struct AdjInterpArgsOf { typedef AdjInterpArgs type; };
template <> struct AdjInterpArgsOf<true, false> { typedef AdjInterpRaggedArgs type; };
template <> struct AdjInterpArgsOf<true, true> { typedef AdjInterpVrArgs type; };

template <typename Real> struct AdjVec4;
template <> struct AdjVec4<float> { typedef float4 type; };
template <> struct AdjVec4<double> { typedef double4 type; };
// what the forward knows about output k, relative to the tile: q_k - a0, the row offset iv_k T, the cubic's argument, gy[k]
template <typename Real> struct AdjRec { int32_t dq, row; Real xx, g; };

// UNION: a wave walks the union of its lanes' k ranges (wave-uniform k: one table row per step, neighbouring records);
// else every lane walks its own [k_lo, k_hi] (no idle steps, 64 rows per step).  Same terms in the same order either way.
// RAGGED: the tile's frame and k ranges and the walks depend on the clip's n_x and n_y, so they are found per column; a
// tile at or behind its clip's n_x skips the column (workgroup-uniform: no barrier is met by some threads only), and a clip
// with n_y == 0 has an empty k range — no chunk, zeros written to all its frames.
// VR (&& RAGGED): every clip at its own constant step S, read from the clock table like its row.  The forward's VR branch
// with T0 = 0, D = 0 to the letter: tt = k S in 128 bits, q_k = tt >> 64, interval and residual are bit fields of the
// fraction — a multiplication and two shifts per k where the constant-rate branch divides.  The k range of a frame is
// vr_adjoint_rules.h's vr_adj_k_range (no 128-bit division), its lower end cut at n_y so that a tile behind the cotangent's
// reach has the empty range [n_y, n_y - 1].  wl / wh / dq stay int32: q_k - a0 lies within T of the tile, and a tile's k
// range holds at most (kAdjIW + T) / s + 1 < 2^31 samples at the smallest admitted io ratio s > 2^-20 (T <= ~740).
template <typename Real, bool UNION, bool RAGGED, bool VR = false>
__global__ void __launch_bounds__(kAdjIW) k_adj_interp(typename AdjInterpArgsOf<RAGGED, VR>::type a)
{
    static_assert(!VR || RAGGED, "the variable-rate form reads a clip table");
    typedef typename AdjVec4<Real>::type V4;
    constexpr int SH = sizeof(Real) == 4 ? 24 : 32;
    __shared__ AdjRec<Real> rec[kAdjIC];
    const int32_t T = a.T, H = T / 2;
    const int tid = (int)threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * kAdjIW, fr = a0 + tid;
    [[maybe_unused]] unsigned __int128 S = 0; // VR: the column's clip's step
    auto k_lo = [&](int64_t f, [[maybe_unused]] int64_t n_y) {
        if constexpr (VR) { const int64_t k = vr_adj_k_range(f, H, S, n_y).lo; return k < n_y ? k : n_y; }
        else { const int64_t k = ceil_div((f - H) * a.L, a.M); return k > 0 ? k : (int64_t)0; }
    };
    auto k_hi = [&](int64_t f, int64_t n_y) {
        if constexpr (VR) return vr_adj_k_range(f, H, S, n_y).hi;
        else { const int64_t k = ceil_div((f + H) * a.L, a.M); return (k < n_y ? k : n_y) - 1; }
    };
    // the tile's share of a clip of n_x frames and n_y cotangent samples (equal lengths: found once, here; RAGGED: per column)
    int64_t k_first = 0, k_end = 0;
    int32_t wl = 0, wh = -1;
    auto geo = [&](int64_t n_y, int64_t n_x) {
        const int64_t a_end = a0 + kAdjIW < n_x ? a0 + kAdjIW : n_x; // the tile's frames: [a0, a_end), never empty
        k_first = k_lo(a0, n_y); k_end = k_hi(a_end - 1, n_y) + 1;   // the tile reads gy[k_first, k_end)
        // this wave's (UNION) or this lane's walk, relative to k_first: [wl, wh], empty behind the signal's end
        const int64_t f0 = UNION ? a0 + (tid & ~63) : fr, f1 = UNION ? (f0 + 63 < a_end ? f0 + 63 : a_end - 1) : fr;
        int32_t l = 0, h = -1;
        if (f0 < a_end) { l = (int32_t)(k_lo(f0, n_y) - k_first); h = (int32_t)(k_hi(f1, n_y) - k_first); }
        if (UNION) { l = __builtin_amdgcn_readfirstlane(l); h = __builtin_amdgcn_readfirstlane(h); }
        wl = l; wh = h;
    };
    if (!RAGGED) geo(a.n_y, a.n_x);
    const int32_t jb = tid + H - 1; // tap of gy[k] in this lane's frame: fr - q_k + H - 1 = jb - (q_k - a0)
    const V4 *tab = (const V4 *)a.tab;

    for (uint64_t col = blockIdx.y; col < a.n_cols; col += gridDim.y) {
        const int64_t clip = (int64_t)(col / a.n_channels), ch = (int64_t)(col - (uint64_t)clip * a.n_channels);
        const int64_t *row = nullptr; // the clip's row; the equal-length form has none
        if constexpr (RAGGED) row = a.rows + 4 * clip;
        const int64_t n_x = RAGGED ? row[3] : a.n_x;
        if (RAGGED) {
            if (a0 >= n_x) continue; // nothing of this clip in this tile
            if constexpr (VR) S = ((unsigned __int128)a.clock[2 * clip] << 64) | a.clock[2 * clip + 1];
            geo(row[1], n_x);
        }
        const Real *g = (const Real *)a.gy + (RAGGED ? row[0] : clip * a.ics) + ch * a.ichs;
        Real acc = 0;
        for (int64_t kc = k_first; kc < k_end; kc += kAdjIC) {
            __syncthreads(); // the chunk before is still being read
            const int64_t k = kc + tid;
            if (k < k_end) { // k_interp's own arithmetic (kernels_interp.h, the constant-rate branch with p0 = d0 = 0)
                int64_t q;
                uint64_t iv, xq;
                if constexpr (VR) { // ... its VR branch with T0 = 0, D = 0
                    const unsigned __int128 tt = (unsigned __int128)(uint64_t)k * S;
                    const uint64_t frac = (uint64_t)tt;
                    q = (int64_t)(uint64_t)(tt >> 64);
                    iv = a.lgP ? frac >> (64 - a.lgP) : 0;
                    xq = (frac << a.lgP) >> (64 - SH);
                } else {
                    const int64_t t = k * a.M;
                    q = t / a.L;
                    const uint64_t r = (uint64_t)(t - q * a.L);
                    const uint64_t tp = r * (uint64_t)a.P, rem = tp % (uint64_t)a.L;
                    iv = tp / (uint64_t)a.L;
                    xq = (rem << SH) / (uint64_t)a.L;
                }
                AdjRec<Real> rc;
                rc.dq = (int32_t)(q - a0);
                rc.row = (int32_t)iv * T;
                rc.xx = (Real)xq * (Real)(1. / (double)(1ULL << SH));
                rc.g = g[k * a.ifs];
                rec[tid] = rc;
            }
            __syncthreads();
            const int64_t c0 = kc - k_first;
            const int32_t i0 = (int32_t)((wl > c0 ? wl : c0) - c0), i1 = (int32_t)((wh < c0 + kAdjIC - 1 ? wh : c0 + kAdjIC - 1) - c0);
#pragma unroll 4
            for (int32_t i = i0; i <= i1; ++i) {
                const AdjRec<Real> rc = rec[i];
                const int32_t j = jb - rc.dq;
                const bool mine = (uint32_t)j < (uint32_t)T; // a - H <= q_k <= a + H - 1: k in this lane's own [k_lo, k_hi]
                // (the load is unconditional, clamped into the row: a load under a condition is waited for at once)
                const V4 v = tab[rc.row + (j < 0 ? 0 : j < T ? j : T - 1)];
                const Real c = fma_r(fma_r(fma_r(v.w, rc.xx, v.z), rc.xx, v.y), rc.xx, v.x);
                acc = mine ? fma_r(c, rc.g, acc) : acc;
            }
        }
        if (fr < n_x) ((Real *)a.gx)[(RAGGED ? row[2] : clip * a.ocs) + fr * a.ofs + ch * a.ochs] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// host: transposed bank, cache, launch
// ---------------------------------------------------------------------------------------------
struct AdjBank : AdjGeom { // (tile: the period fits LDS, tab and e0 exist)
    const Plan *plan = nullptr;
    int device = -1;
    int64_t L = 1, M = 1;
    int32_t Tt = 0, dmin = 0, I = 0;
    void *ct[2] = {nullptr, nullptr};  // [Tt][M], 0 = f32, 1 = f64
    int32_t *d_lo = nullptr;           // [M]
    void *tab[2] = {nullptr, nullptr}; // [n_st][I][16]
    int32_t *e0 = nullptr;             // [n_st]
};

static std::mutex g_adj_mu;
static std::vector<AdjBank *> g_adj; // one per plan (a plan's device tables live on one device)

static void adj_free(AdjBank *b)
{
    for (int i = 0; i < 2; ++i) {
        if (b->ct[i]) (void)hipFree(b->ct[i]);
        if (b->tab[i]) (void)hipFree(b->tab[i]);
    }
    if (b->d_lo) (void)hipFree(b->d_lo);
    if (b->e0) (void)hipFree(b->e0);
    delete b;
}

void adjoint_release(const Plan *p)
{
    adjoint_fft_release(p); // (the transposed plan of HIPSOXR_KERNEL_ADJOINT_FFT lives and dies with these tables)
    std::lock_guard<std::mutex> lk(g_adj_mu);
    for (size_t i = 0; i < g_adj.size();)
        if (g_adj[i]->plan == p) {
            adj_free(g_adj[i]);
            g_adj.erase(g_adj.begin() + i);
        } else ++i;
}

template <typename Real>
static const char *adj_upload(void **dst, const std::vector<double> &src)
{
    std::vector<Real> v(src.size());
    for (size_t i = 0; i < src.size(); ++i) v[i] = (Real)src[i]; // float32: the float64 bank rounded to nearest
    HIP_TRY(hipMalloc(dst, std::max<size_t>(v.size(), 1) * sizeof(Real)));
    HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(Real), hipMemcpyHostToDevice));
    return nullptr;
}

// adj_tables' tables on the device: the transposed bank with d_lo, then — where the plan has them — the tile tables with e0
static const char *adj_build(const Plan &p, AdjBank *b)
{
    const AdjTables t = adj_tables(p.L, p.M, p.T, p.bank.data());
    const struct { const std::vector<double> &coef; const std::vector<int32_t> &first; void **d_coef; int32_t **d_first; } sets[2] = {
        {t.ct, t.lo, b->ct, &b->d_lo}, {t.tab, t.e0, b->tab, &b->e0}};
    for (int k = 0; k < (t.tile ? 2 : 1); ++k) {
        if (const char *e = adj_upload<float>(&sets[k].d_coef[0], sets[k].coef)) return e;
        if (const char *e = adj_upload<double>(&sets[k].d_coef[1], sets[k].coef)) return e;
        HIP_TRY(hipMalloc((void **)sets[k].d_first, sets[k].first.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(*sets[k].d_first, sets[k].first.data(), sets[k].first.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    static_cast<AdjGeom &>(*b) = t;
    b->L = p.L; b->M = p.M; b->Tt = t.Tt; b->dmin = t.dmin; b->I = t.I;
    return nullptr;
}

// The plan's transposed tables, built on first use (exact-bank plans; the caller has checked).
static const char *adj_ensure(Plan *p, AdjBank **out)
{
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->device >= 0 && cur != p->device) return "this plan's device tables live on another device (one plan per device)";
        if (p->device < 0) p->device = cur;
    }
    std::lock_guard<std::mutex> lk(g_adj_mu);
    for (AdjBank *b : g_adj)
        if (b->plan == p) { *out = b; return nullptr; }
    AdjBank *b = new AdjBank();
    b->plan = p; b->device = cur;
    if (const char *e = adj_build(*p, b)) { adj_free(b); return e; }
    g_adj.push_back(b);
    *out = b;
    return nullptr;
}

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): one line per launch, in the style of fft.hip's fft_launch_log — what
// tests/test_gpu_adjoint_forms.py reads the launch form from.
// A ragged launch (a.rows) appends " ragged=<n_clips>"; an equal-length launch writes its line as it always did.
static void adj_launch_log(const char *kernel, size_t width, const AdjBank &b, int lanes, size_t lds, const AdjRaggedArgs &a, dim3 grid, unsigned nt)
{
    FILE *f = fopen(switches().dbg_launch_log, "a");
    if (!f) return;
    fprintf(f, "kernel=%s width=%zu L=%lld M=%lld lanes=%d lds=%zu cg=%d pb=%d grid=%ux%ux%u block=%u n_st=%d", kernel, width,
            (long long)b.L, (long long)b.M, lanes, lds, a.cg, a.pb, grid.x, grid.y, grid.z, nt, b.n_st);
    if (a.rows) fprintf(f, " ragged=%u", a.n_clips);
    fputc('\n', f);
    fclose(f);
}
// ... and k_adj_interp's line (a variable-rate launch puts " vr=1" in front of its ragged=<n_clips>)
template <typename Real>
static void adj_interp_log(const Plan &p, bool per_lane, dim3 grid, const AdjInterpRaggedArgs &a, uint32_t n_clips, bool vr = false)
{
    FILE *f = fopen(switches().dbg_launch_log, "a");
    if (!f) return;
    fprintf(f, "kernel=adj_interp width=%zu L=%lld M=%lld T=%d P=%d tile=%d chunk=%d lds=%zu walk=%s grid=%ux%ux%u block=%u", sizeof(Real),
            (long long)p.L, (long long)p.M, p.T, p.phases, kAdjIW, kAdjIC, sizeof(AdjRec<Real>) * kAdjIC, per_lane ? "lane" : "union",
            grid.x, grid.y, grid.z, (unsigned)kAdjIW);
    if (vr) fputs(" vr=1", f);
    if (a.rows) fprintf(f, " ragged=%u", n_clips);
    fputc('\n', f);
    fclose(f);
}

// The launches proper, one call site per kernel: the RAGGED instantiation takes the whole argument block, the equal-length
// one the block it always took — the AdjArgs / AdjInterpArgs part.
template <typename Real, bool RAGGED>
static const char *adj_run_tile(const AdjRaggedArgs &a, dim3 grid, unsigned nt, size_t lds, hipStream_t st)
{
    if (const char *e = ensure_dyn_lds((const void *)k_adj_tile<Real, RAGGED>, lds)) return e;
    hipLaunchKernelGGL((k_adj_tile<Real, RAGGED>), grid, dim3(nt), lds, st, static_cast<const typename AdjArgsOf<RAGGED>::type &>(a));
    return nullptr;
}
template <typename Real, bool RAGGED>
static void adj_run_gather(const AdjRaggedArgs &a, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL((k_adj_gather<Real, RAGGED>), grid, dim3(kAdjGatherLanes), 0, st, static_cast<const typename AdjArgsOf<RAGGED>::type &>(a));
}
// (Args: AdjInterpRaggedArgs, or — the variable-rate form — AdjInterpVrArgs)
template <typename Real, bool UNION, bool RAGGED, bool VR = false, typename Args>
static void adj_run_interp(const Args &a, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL((k_adj_interp<Real, UNION, RAGGED, VR>), grid, dim3(kAdjIW), 0, st, static_cast<const typename AdjInterpArgsOf<RAGGED, VR>::type &>(a));
}

// The argument block of the exact-bank kernels, all but what the tile form decides.  rows: the device copy of a ragged job's
// clip table, or NULL (equal-length clips).  A ragged job's in_frames / out_frames are its largest clip's: the form is
// chosen by, and the grid's frame axis sized by, the LONGEST clip.
static AdjRaggedArgs adj_args(const AdjBank &b, int prec, const hipsoxr_job_t &j, const int64_t *rows)
{
    AdjRaggedArgs a{}; // (the equal-length kernels take its AdjArgs part)
    a.gy = j.in; a.gx = j.out;
    a.ct = b.ct[prec]; a.d_lo = b.d_lo; a.tab = b.tab[prec]; a.e0 = b.e0;
    a.L = b.L; a.M = b.M; a.Lc = b.Lc; a.Mc = b.Mc;
    a.Tt = b.Tt; a.n_st = b.n_st; a.I = b.I; a.dmin = b.dmin; a.pad = b.pad;
    a.n_clips = j.n_clips; a.n_channels = j.n_channels;
    a.ics = j.in_clip_stride; a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride;
    a.ocs = j.out_clip_stride; a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.n_y = j.in_frames; a.n_x = j.out_frames;
    a.rows = rows;
    a.inter = (j.n_channels > 1 && j.in_chan_stride == 1 && j.out_chan_stride == 1) ? 1 : 0; // frames of interleaved channels
    return a;
}

template <typename Real>
static const char *adj_launch_tile(const AdjBank &b, const AdjTileForm &f, AdjRaggedArgs a, hipStream_t st)
{
    a.cg_shift = f.cg_shift; a.n_groups = f.n_groups; a.n_waves = f.n_waves;
    const dim3 grid((uint32_t)f.gx, f.gy, (uint32_t)f.gz);
    const unsigned nt = (unsigned)f.n_waves * 64;
    if (const char *e = a.rows ? adj_run_tile<Real, true>(a, grid, nt, f.lds, st) : adj_run_tile<Real, false>(a, grid, nt, f.lds, st)) return e;
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) adj_launch_log("adj_tile", sizeof(Real), b, f.lanes, f.lds, a, grid, nt);
    return nullptr;
}

template <typename Real>
static const char *adj_launch_gather(const AdjBank &b, const hipsoxr_job_t &j, const AdjRaggedArgs &a, hipStream_t st)
{
    const AdjGrid g = adj_gather_grid(j.out_frames, j.n_clips, j.n_channels);
    if (!g.ok) return kAdjTooLong;
    const dim3 grid(g.gx, g.gy);
    if (a.rows) adj_run_gather<Real, true>(a, grid, st);
    else adj_run_gather<Real, false>(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) adj_launch_log("adj_gather", sizeof(Real), b, 0, 0, a, grid, kAdjGatherLanes);
    return nullptr;
}

// The exact-bank launch: the arguments, the form (adjoint_rules.h), the form's kernel.
template <typename Real>
static const char *adj_launch(const AdjBank &b, const hipsoxr_job_t &j, hipStream_t st, const int64_t *rows)
{
    AdjRaggedArgs a = adj_args(b, sizeof(Real) == 4 ? 0 : 1, j, rows);
    const AdjTileForm f = adj_tile_form(b, sizeof(Real), j.out_frames, j.n_clips, j.n_channels, a.inter != 0);
    a.cg = f.cg; a.pb = f.pb; a.x_count = f.x_count;
    return f.ok ? adj_launch_tile<Real>(b, f, a, st) : adj_launch_gather<Real>(b, j, a, st);
}

// k_adj_interp on the plan's own interpolation table (uploaded by device_bank_ensure, as for the forward).
template <typename Real>
static const char *adj_interp_launch(const Plan &p, const hipsoxr_job_t &j, hipStream_t st, const int64_t *rows)
{
    AdjInterpRaggedArgs a{};
    a.gy = j.in; a.gx = j.out; a.tab = p.dev[sizeof(Real) == 4 ? 0 : 1].interp_tab;
    a.L = p.L; a.M = p.M; a.T = p.T; a.P = p.phases;
    a.n_cols = (uint64_t)j.n_clips * j.n_channels; a.n_channels = j.n_channels;
    a.ics = j.in_clip_stride; a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride;
    a.ocs = j.out_clip_stride; a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.n_y = j.in_frames; a.n_x = j.out_frames;
    a.rows = rows;
    const AdjGrid g = adj_interp_grid(p.L, p.M, p.T, j.in_frames, j.out_frames, a.n_cols, kAdjIW);
    if (!g.ok) return kAdjTooLong;
    const dim3 grid(g.gx, g.gy);
    const bool per_lane = switches().adj_interp_per_lane;
    if (rows) per_lane ? adj_run_interp<Real, false, true>(a, grid, st) : adj_run_interp<Real, true, true>(a, grid, st);
    else per_lane ? adj_run_interp<Real, false, false>(a, grid, st) : adj_run_interp<Real, true, false>(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) adj_interp_log<Real>(p, per_lane, grid, a, j.n_clips);
    return nullptr;
}

// k_adj_interp<.., VR> over a whole clip table: rows and clock are the device copies of the clip table and of the clips' steps.
template <typename Real>
static const char *adj_interp_vr_launch(const Plan &p, const hipsoxr_job_t &j, hipStream_t st, const int64_t *rows, const uint64_t *clock)
{
    AdjInterpVrArgs a{};
    a.gy = j.in; a.gx = j.out; a.tab = p.dev[sizeof(Real) == 4 ? 0 : 1].interp_tab;
    a.L = p.L; a.M = p.M; a.T = p.T; a.P = p.phases;
    while ((1 << a.lgP) < a.P) ++a.lgP;
    if ((1 << a.lgP) != a.P) return "variable-rate needs a power-of-two phase count";
    a.n_cols = (uint64_t)j.n_clips * j.n_channels; a.n_channels = j.n_channels;
    a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride; // (a clip's place is its row's: the clip strides are not read)
    a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.n_y = j.in_frames; a.n_x = j.out_frames;
    a.rows = rows; a.clock = clock;
    const AdjGrid g = vr_adj_grid(j.out_frames, a.n_cols, kAdjIW);
    if (!g.ok) return kAdjTooLong;
    const dim3 grid(g.gx, g.gy);
    const bool per_lane = switches().adj_interp_per_lane;
    per_lane ? adj_run_interp<Real, false, true, true>(a, grid, st) : adj_run_interp<Real, true, true, true>(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) adj_interp_log<Real>(p, per_lane, grid, a, j.n_clips, true);
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// host: the two entries
// ---------------------------------------------------------------------------------------------
template <typename F> static const char *with_real(int elem, F f) { return elem == HIPSOXR_F32 ? f(float{}) : f(double{}); }

static AdjAsk adj_ask(const Plan &p, const hipsoxr_job_t &j)
{
    AdjAsk q;
    q.half = elem_is_half(j.elem);
    q.real = j.elem == HIPSOXR_F32 || j.elem == HIPSOXR_F64;
    q.by_name = j.kernel == HIPSOXR_KERNEL_ADJOINT; // every constant-rate plan: k_adj_interp where there is no exact bank
    q.auto_or_exact = j.kernel == HIPSOXR_KERNEL_AUTO || j.kernel == HIPSOXR_KERNEL_EXACT;
    q.vr = p.vr; q.phases = p.phases != 0;
    q.window = j.in_abs0 != 0 || j.out_k0 != 0;
    q.table = j.clip_table != nullptr;
    return q;
}
// ... what both entries ask last, of a job that is not empty
static const char *adj_device_refusal(const hipsoxr_job_t &j)
{
    if (!j.out || (j.in_frames > 0 && !j.in)) return "null buffer";
    return device_count() <= 0 ? kNoDevice : nullptr;
}

// The tables the job's kernel reads: the forward's interpolation table in the element's width (a fresh plan has none yet),
// or the transposed bank (*b).
static const char *adj_tables_ensure(Plan *p, const hipsoxr_job_t &j, AdjBank **b)
{
    return p->phases ? device_bank_ensure(p, engine_prec(j.elem)) : adj_ensure(p, b);
}
static const char *adj_run(const Plan &p, const AdjBank *b, const hipsoxr_job_t &j, hipStream_t st, const int64_t *rows)
{
    if (p.phases) return with_real(j.elem, [&](auto r) { return adj_interp_launch<decltype(r)>(p, j, st, rows); });
    return with_real(j.elem, [&](auto r) { return adj_launch<decltype(r)>(*b, j, st, rows); });
}

// (device.h) the exact adjoint behind the entries' refusals, for the launchers that resolve to it or hand it a sub-table
// (adjoint_auto.hip, twostage.hip): the tables, then — unless dry — the launch; rows: the device copy of a clip table, or NULL
const char *adj_exact_run(Plan *p, const hipsoxr_job_t &j, void *stream, const int64_t *rows, bool dry)
{
    AdjBank *b = nullptr;
    if (const char *e = adj_tables_ensure(p, j, &b)) return e;
    return dry ? nullptr : adj_run(*p, b, j, (hipStream_t)stream, rows);
}

const char *launch_adjoint(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    // the job is read in the adjoint's own direction: in = gy (in_frames = n_y), out = gx (out_frames = n_x)
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_FFT) return launch_adjoint_fft(p, j, stream); // the frequency-domain engine, by name
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_TWO_STAGE) return launch_adjoint_two_stage(p, j, stream); // the two-stage form's transpose, by name
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_AUTO) return launch_adjoint_auto(p, j, stream); // the transpose of AUTO's forward (adjoint_auto.hip)
    if (elem_is_half(j.elem)) {
        // float16 / bfloat16: the float32 adjoint on the widened cotangent, rounded once (half.hip) — under every selector
        // this entry serves for float32.  The refusals by name and the empty job first, asked of the float32 job without clips.
        hipsoxr_job_t f = j;
        f.elem = HIPSOXR_F32; f.n_clips = 0;
        if (const char *e = launch_adjoint(p, f, stream)) return e;
        if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
        if (const char *e = adj_device_refusal(j)) return e;
        return launch_half(p, j, stream, true);
    }
    if (const char *e = adj_entry_refusal(kAdjEqual, adj_ask(*p, j))) return e;
    if (const char *e = adj_extent_refusal(kAdjEqual, j.in_frames, j.out_frames, [&](uint64_t n) { return plan_out_len(*p, n); })) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_device_refusal(j)) return e;
    AdjBank *b = nullptr;
    if (const char *e = adj_tables_ensure(p, j, &b)) return e;
    return adj_run(*p, b, j, (hipStream_t)stream, nullptr);
}

// hipsoxr_run_device_adjoint_ragged: all clips of a clip table in ONE launch of the kernel's RAGGED form.  The refusals are
// made by name before the device is asked for, as in launch_adjoint.  More than 65535 columns: the kernels' gridDim.y
// loops wrap.
const char *launch_adjoint_ragged(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_FFT) return launch_adjoint_fft_ragged(p, j, stream);
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_TWO_STAGE) return kPolyAdjRaggedRefusal; // (poly_adj_rules.h: clip tables are not served yet)
    if (j.kernel == HIPSOXR_KERNEL_ADJOINT_AUTO) return launch_adjoint_auto_ragged(p, j, stream);
    const auto out_len = [&](uint64_t n) { return plan_out_len(*p, n); };
    if (const char *e = adj_entry_refusal(kAdjRagged, adj_ask(*p, j))) return e;
    for (uint32_t c = 0; c < j.n_clips; ++c)
        if (const char *e = adj_row_refusal(job_row_check(j.clip_table + kRaggedRow * (size_t)c, j.in_frames, j.out_frames, kJobRowAdjoint, out_len))) return e;
    if (const char *e = adj_extent_refusal(kAdjRagged, j.in_frames, j.out_frames, out_len)) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (const char *e = adj_device_refusal(j)) return e;
    AdjBank *b = nullptr;
    if (const char *e = adj_tables_ensure(p, j, &b)) return e;
    // The kernels read the DEVICE copy of the table; without one the host table, validated above, is uploaded in stream
    // order (clip_table_device: the buffer lives until the launch behind it has run).  A caller's copy is trusted.
    const hipStream_t st = (hipStream_t)stream;
    const int64_t *rows = nullptr;
    void *tmp = nullptr;
    static constexpr ClipTableTexts texts = {"adjoint job: ragged: no device memory for the clip table", "adjoint job: ragged: clip table upload failed"};
    if (const char *e = clip_table_device(j, stream, &rows, &tmp, texts)) return e;
    const char *e = adj_run(*p, b, j, st, rows);
    if (tmp) (void)hipFreeAsync(tmp, st);
    return e;
}

// hipsoxr_run_device_vr_ragged_adjoint (the entry, engine.cpp, has refused by name and validated the table): clip c's
// gx = A_c^T gy at its own step clock[c] = {hi, lo} (host memory), all clips in ONE launch of k_adj_interp<.., VR>.  The clock
// table and — where the caller gave no device copy — the clip table are uploaded in stream order and released behind the
// launch, as launch_vr_ragged and launch_adjoint_ragged do.
const char *launch_adjoint_vr_ragged(Plan *p, const hipsoxr_job_t &j, const uint64_t *clock, void *stream)
{
    const hipStream_t st = (hipStream_t)stream;
    if (const char *e = device_bank_ensure(p, engine_prec(j.elem))) return e;
    const int64_t *rows = nullptr;
    void *tmp = nullptr, *clk = nullptr;
    static constexpr ClipTableTexts texts = {"variable-rate ragged adjoint: no device memory for the clip table",
                                             "variable-rate ragged adjoint: clip table upload failed"};
    if (const char *e = clip_table_device(j, stream, &rows, &tmp, texts)) return e;
    const size_t bytes = (size_t)j.n_clips * kVrClockRow * sizeof(uint64_t);
    const char *err = nullptr;
    if (hipMallocAsync(&clk, bytes, st) != hipSuccess) { clk = nullptr; err = "variable-rate ragged adjoint: no device memory for the clock table"; }
    else if (hipMemcpyAsync(clk, clock, bytes, hipMemcpyHostToDevice, st) != hipSuccess) err = "variable-rate ragged adjoint: clock table upload failed";
    if (!err) err = with_real(j.elem, [&](auto r) { return adj_interp_vr_launch<decltype(r)>(*p, j, st, rows, (const uint64_t *)clk); });
    if (clk) (void)hipFreeAsync(clk, st);
    if (tmp) (void)hipFreeAsync(tmp, st);
    return err;
}

} // namespace hipsoxr
