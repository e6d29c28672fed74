// adjoint_rules.h — the host rules of the transposed operator (adjoint.hip): the transposed bank and the per-tile skewed
// tables of a plan, which launch form a job takes and with what grid, what the two entries refuse before the device is asked
// for anything.  No HIP, no globals, no switches(): the plan's numbers, the job's and the entry arrive as arguments
// (tests/c/adjoint_rules_check.cpp checks the tables against plan.h's locate() and each rule against a slow statement of it).
// The launch form decides more than speed: by adjoint.hip's REACH paragraph, which gx a non-finite cotangent poisons.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "job_rules.h" // kJobMaxCols, JobRowFault

// (floor_div and ceil_div are what k_adj_interp itself calls: under a device compiler they are device functions too)
#if defined(__HIPCC__)
#define HIPSOXR_ADJ_RULE __host__ __device__ static inline
#else
#define HIPSOXR_ADJ_RULE static inline
#endif

namespace hipsoxr {

constexpr int kAdjRS = 16;        // phases per wave tile of k_adj_tile
constexpr int kAdjMinPeriods = 4; // k_adj_tile from this many (replicated) periods of input up

HIPSOXR_ADJ_RULE int64_t floor_div(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; } // b > 0
HIPSOXR_ADJ_RULE int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

// ---- tables ----------------------------------------------------------------------------------------------------------------
// What a launch needs of k_adj_tile's geometry: the period replicated c times (Mc inputs <- Lc cotangent samples), the LDS row
// padding, the frames the widest tile reaches behind the slab's first (wmax), the phase tiles; tile: the plan has tile tables.
struct AdjGeom {
    int64_t Lc = 1, Mc = 1;
    int32_t pad = 0, wmax = 0, n_st = 0;
    bool tile = false;
};
// ... and the tables themselves, in float64 (the float32 ones are these rounded to nearest)
struct AdjTables : AdjGeom {
    int32_t Tt = 0, dmin = 0, I = 0;
    std::vector<int32_t> lo; // [M]            d_lo(s), non-decreasing
    std::vector<double> ct;  // [Tt][M]        ct[i][s]: coefficient of gy[q L + lo[s] + i] in gx[q M + s]
    std::vector<int32_t> e0; // [n_st]         first gy sample of a tile's table, relative to dmin
    std::vector<double> tab; // [n_st][I][16]  tab[st][ii][rr]: coefficient of gy[q Lc + dmin + e0[st] + ii] in gx[q Mc + 16 st + rr]
};
// 16 periods of float32 would not fit LDS above these: k_adj_gather serves the plan, it gets no tile tables
constexpr int64_t kAdjMaxLc = 8192, kAdjMaxMc = 65536;

// The exact transpose of locate(): bank is the forward's [L][T].  (adjoint.hip's header derives d_lo, d_hi and the tap.)
inline AdjTables adj_tables(int64_t L, int64_t M, int32_t T, const double *bank)
{
    AdjTables t;
    const int64_t H = T / 2;
    auto d_lo = [&](int64_t s) { return ceil_div((s - H) * L, M); };
    auto d_hi = [&](int64_t s) { return ceil_div((s + H) * L, M) - 1; };
    // coefficient of gy[q L + d] in gx[q M + s]: c[(d M) mod L][s + T/2 - 1 - floor(d M / L)], 0 outside the phase's terms
    auto coef = [&](int64_t s, int64_t d) -> double {
        if (d < d_lo(s) || d > d_hi(s)) return 0.0;
        const int64_t nfl = floor_div(d * M, L), ph = d * M - nfl * L, j = s + H - 1 - nfl;
        return (j >= 0 && j < T) ? bank[(size_t)(ph * T + j)] : 0.0;
    };
    int64_t Tt = 0;
    t.lo.resize((size_t)M);
    for (int64_t s = 0; s < M; ++s) {
        t.lo[(size_t)s] = (int32_t)d_lo(s);
        Tt = std::max(Tt, d_hi(s) - d_lo(s) + 1);
    }
    t.Tt = (int32_t)Tt;
    t.dmin = t.lo[0]; // d_lo is non-decreasing in s
    t.ct.resize((size_t)(Tt * M));
    for (int64_t s = 0; s < M; ++s)
        for (int64_t i = 0; i < Tt; ++i) t.ct[(size_t)(i * M + s)] = coef(s, t.lo[(size_t)s] + i);
    // k_adj_tile: the period replicated until a wave tile (16 phases) and a slab row (64 frames) are filled
    const int64_t c = std::max((kAdjRS + M - 1) / M, (64 + L - 1) / L);
    t.Lc = c * L; t.Mc = c * M;
    t.pad = (t.Lc & 1) ? 0 : 1;
    if (t.Lc > kAdjMaxLc || t.Mc > kAdjMaxMc) return t;
    const int32_t n_st = (int32_t)((t.Mc + kAdjRS - 1) / kAdjRS);
    int64_t I = 0;
    for (int32_t st = 0; st < n_st; ++st) {
        const int64_t s0 = (int64_t)st * kAdjRS, s1 = std::min<int64_t>(s0 + kAdjRS, t.Mc) - 1;
        I = std::max(I, d_hi(s1) - d_lo(s0) + 1);
    }
    I = (I + 3) / 4 * 4;
    t.e0.resize((size_t)n_st);
    t.tab.assign((size_t)n_st * (size_t)I * kAdjRS, 0.0);
    int64_t wmax = 0;
    for (int32_t st = 0; st < n_st; ++st) {
        const int64_t s0 = (int64_t)st * kAdjRS, first = d_lo(s0);
        t.e0[(size_t)st] = (int32_t)(first - t.dmin);
        wmax = std::max(wmax, first - t.dmin + I);
        for (int64_t ii = 0; ii < I; ++ii)
            for (int rr = 0; rr < kAdjRS; ++rr)
                if (s0 + rr < t.Mc) t.tab[((size_t)st * (size_t)I + (size_t)ii) * kAdjRS + rr] = coef(s0 + rr, first + ii);
    }
    t.n_st = n_st; t.I = (int32_t)I; t.wmax = (int32_t)wmax;
    t.tile = true;
    return t;
}

// ---- launch forms ----------------------------------------------------------------------------------------------------------
// n_x is the job's out_frames (a ragged job: its LONGEST clip's); the job is not empty.
constexpr const char *kAdjTooLong = "adjoint job: too long for one launch";
constexpr int64_t kAdjMaxGridX = INT32_MAX;

constexpr size_t kAdjLdsPair = (size_t)80 * 1024;   // a slab up to here leaves room for two workgroups per CU
constexpr size_t kAdjLdsWhole = (size_t)160 * 1024; // ... and up to here fits at all
constexpr int64_t kAdjWgTarget = 1024;              // workgroups that give the chip ~4 per CU
constexpr int kAdjMaxWaves = 16;                    // waves of a k_adj_tile workgroup

// k_adj_tile: lanes per workgroup slab — 64 (32, 16 where LDS demands), first under kAdjLdsPair, then under kAdjLdsWhole — as
// pb periods x cg channels (frames of interleaved channels: whole groups of channels, else one); a grid of gx period spans x
// gy (clip, channel group) columns x gz shares of a slab's phase tiles, n_waves waves each.  ok == false: the job runs on
// k_adj_gather — no tile tables, fewer than kAdjMinPeriods periods, no lane count fits, or too many spans.
struct AdjTileForm {
    bool ok = false;
    int lanes = 0;
    size_t lds = 0;
    int32_t cg = 0, pb = 0, x_count = 0; // (set with lanes: a form refused for its spans alone keeps them, as it always did)
    int32_t cg_shift = -1;               // log2(cg), or -1
    uint32_t n_groups = 0;
    int64_t gx = 0;
    uint32_t gy = 0;
    int gz = 0;
    int32_t n_waves = 0;
};
inline AdjTileForm adj_tile_form(const AdjGeom &g, size_t real_bytes, int64_t n_x, uint32_t n_clips, uint32_t n_channels, bool inter)
{
    AdjTileForm f;
    if (!g.tile || n_x < kAdjMinPeriods * g.Mc) return f;
    for (size_t limit : {kAdjLdsPair, kAdjLdsWhole}) {
        for (int ln : {64, 32, 16}) {
            const int32_t cg = inter ? (int32_t)std::min<uint32_t>(n_channels, (uint32_t)ln) : 1, pb = ln / cg;
            const int64_t xc = (int64_t)(pb - 1) * g.Lc + g.wmax, slab_rows = (xc + g.Lc - 1) / g.Lc;
            const size_t need = (size_t)(slab_rows * (g.Lc + g.pad)) * (size_t)cg * real_bytes;
            if (need <= limit) { f.lanes = ln; f.lds = need; f.cg = cg; f.pb = pb; f.x_count = (int32_t)xc; break; }
        }
        if (f.lanes) break;
    }
    if (!f.lanes) return f;
    const int64_t n_per = (n_x + g.Mc - 1) / g.Mc;
    f.gx = (n_per + f.pb - 1) / f.pb;
    if (f.gx > kAdjMaxGridX) return f;
    for (int sh = 0; sh < 7; ++sh)
        if ((1 << sh) == f.cg) f.cg_shift = sh;
    f.n_groups = (n_channels + (uint32_t)f.cg - 1) / (uint32_t)f.cg;
    f.gy = (uint32_t)std::min<uint64_t>((uint64_t)n_clips * f.n_groups, kJobMaxCols); // more columns: the kernel's loop wraps
    // few workgroups: spread a slab's phase tiles over z workgroups until the chip has kAdjWgTarget
    const int64_t wgs = f.gx * (int64_t)f.gy;
    int z = (int)std::min<int64_t>(g.n_st, std::max<int64_t>(1, kAdjWgTarget / wgs));
    f.n_waves = std::min(kAdjMaxWaves, (g.n_st + z - 1) / z);
    f.gz = std::min(z, (g.n_st + f.n_waves - 1) / f.n_waves);
    f.ok = true;
    return f;
}

// k_adj_gather and k_adj_interp: gx workgroups of `frames` elements along a column (k_adj_gather: along a clip's frames x
// channels), gy columns.  ok == false: kAdjTooLong.
struct AdjGrid { bool ok = false; uint32_t gx = 0, gy = 0; };
constexpr int kAdjGatherLanes = 256; // k_adj_gather's workgroup: one lane per gx element
inline AdjGrid adj_gather_grid(int64_t n_x, uint32_t n_clips, uint32_t n_channels)
{
    AdjGrid r;
    const int64_t per_clip = n_x * (int64_t)n_channels, gx = (per_clip + kAdjGatherLanes - 1) / kAdjGatherLanes;
    r.ok = gx <= kAdjMaxGridX;
    r.gx = (uint32_t)gx; r.gy = std::min<uint32_t>(n_clips, kJobMaxCols);
    return r;
}
// ... positions are 64-bit products, as in the forward: (frame + T/2) L and k M stay below 2^62
inline AdjGrid adj_interp_grid(int64_t L, int64_t M, int32_t T, int64_t n_y, int64_t n_x, uint64_t n_cols, int frames)
{
    AdjGrid r;
    const __int128 lim = (__int128)1 << 62;
    if ((__int128)(n_x + T) * L >= lim || (__int128)n_y * M >= lim) return r;
    const int64_t gx = (n_x + frames - 1) / frames;
    r.ok = gx <= kAdjMaxGridX;
    r.gx = (uint32_t)gx; r.gy = (uint32_t)std::min<uint64_t>(n_cols, kJobMaxCols);
    return r;
}

// ---- refusals that need no device state -----------------------------------------------------------------------------------
// The two entries: hipsoxr_run_device_adjoint (equal-length clips) and hipsoxr_run_device_adjoint_ragged (a clip table).
enum AdjEntry { kAdjEqual, kAdjRagged };
// What the entries ask of a job, in their order.  half: float16 / bfloat16 (the equal-length entry never asks with it: it
// widens such a job and asks for the float32 one); real: float32 / float64; by_name: HIPSOXR_KERNEL_ADJOINT; auto_or_exact:
// HIPSOXR_KERNEL_AUTO / _EXACT; window: in_abs0 or out_k0 is not 0; table: the job has a clip_table.
struct AdjAsk { bool half, real, by_name, auto_or_exact, vr, phases, window, table; };
// Each returns the text, or nullptr.  The entries differ in four places, on purpose: half elements, the variable-rate rule
// (the ragged entry refuses such a plan under every selector), the hint for interpolated-phase plans, and the clip table —
// refused here, demanded there, the ragged entry asking behind the selector.
inline const char *adj_entry_refusal(AdjEntry entry, const AdjAsk &q)
{
    const bool ragged = entry == kAdjRagged;
    if (ragged && q.half)
        return "adjoint job: ragged: float16 / bfloat16 clip tables are not served (float32 or float64; half cotangents clip by clip through hipsoxr_run_device_adjoint)";
    if (!q.real) return "adjoint job: float32 or float64 elements only (integer types have no gradient)";
    if (ragged ? q.vr : q.by_name && q.vr)
        return ragged ? "adjoint job: variable-rate plans are not served (ragged batches take constant-rate plans)"
                      : "adjoint job: variable-rate plans are not served (HIPSOXR_KERNEL_ADJOINT takes constant-rate plans)";
    if (q.phases && !q.by_name)
        return ragged ? "adjoint job: needs an exact-bank plan (interpolated-phase plans are served by name, HIPSOXR_KERNEL_ADJOINT)"
                      : "adjoint job: needs an exact-bank plan (interpolated-phase plans and the two-stage form are not served)";
    if (q.window) return "adjoint job: whole signals only (in_abs0 == 0, out_k0 == 0)";
    if (!ragged && q.table) return "adjoint job: ragged batches (clip_table) are served by hipsoxr_run_device_adjoint_ragged, not by this entry";
    if (!q.auto_or_exact && !q.by_name)
        return "adjoint job: the kernel selector must be AUTO or EXACT (the adjoint is the exact engine's; the frequency-domain engine has none)";
    if (ragged && !q.table) return "adjoint job: the ragged entry needs a clip_table (equal-length clips: hipsoxr_run_device_adjoint)";
    return nullptr;
}
// ... the ragged entry then asks every row of the table (job_row_check, adjoint direction) ...
inline const char *adj_row_refusal(JobRowFault f)
{
    switch (f) {
    case kJobRowOk: break;
    case kJobRowNegative: return "adjoint job: ragged: a clip's offset or frame count is negative";
    case kJobRowAboveJob: return "adjoint job: ragged: a clip's frame count is above the job's in_frames / out_frames (the largest per-clip values)";
    case kJobRowAbovePlan: return "adjoint job: ragged: a clip's n_y (cotangent frames) exceeds the plan's output length for its n_x";
    }
    return nullptr;
}
// ... and both the extent: in_frames is the cotangent's n_y, out_frames the gradient's n_x; out_len = plan_out_len of the
// plan.  (The ragged entry has no length rule here: its rows have answered it.)
template <typename OutLen>
inline const char *adj_extent_refusal(AdjEntry entry, int64_t in_frames, int64_t out_frames, OutLen out_len)
{
    if (in_frames < 0 || out_frames < 0) return "adjoint job: invalid job extent";
    if (entry == kAdjEqual && (uint64_t)in_frames > (uint64_t)out_len((uint64_t)out_frames))
        return "adjoint job: in_frames (cotangent frames) exceeds the plan's output length for out_frames";
    return nullptr;
}

} // namespace hipsoxr
