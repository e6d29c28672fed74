// kernels.hip — the soxr_process hot path on CDNA4 (gfx950): the EXACT (canonical-order) engine.
// Hand-written HIP; the f32 throughput kernels run the canonical fma chains on the f32-input matrix pipe.
//
// Replaces the inner product libsoxr runs inside soxr_process (reference call sites
// src/soxr_ext.cpp:163-166, :245-248, :328-331):
//     y[k] = sum_j bank[(k*M) mod L][j] * x[floor(k*M/L) - (T/2-1) + j]
// followed by the conversion to the I/O type (round-half-even, saturate, clip count, TPDF dither
// for int16).
//
// CANONICAL ARITHMETIC (shared with oracle/soxr_oracle.c *_port, bit for bit):
//     accL = 0; for j = 0 .. T/2-1 ascending : accL = fma(c[j], x[j], accL)
//     accR = 0; for j = T-1 .. T/2 descending: accR = fma(c[j], x[j], accR)
//     y = accL + accR
// in the engine precision Real (float for f32/i16 I/O, double for f64/i32 I/O).  Each output
// sample is one pair of serial FMA chains that depends on nothing but its own taps, so results are
// independent of chunking, tiling, launch geometry and kernel choice (the bit-exact invariances of
// reference tests test_divide_match / test_stream_length).  Zero-padded table entries contribute
// fma(0, x, acc) == acc exactly for finite x.
//
// Kernels (all bit-identical to each other and to the oracle; DESIGN.md §5.1 has the table):
//   k_gather        one lane per output sample; coefficients gathered from the tap-major bank
//                   [T][Lpad], input read straight from global memory.  Universal fallback: every
//                   ratio / layout / length.
//   k_chain         small launches (streaming chunks, < 4096 outputs): a workgroup stages the coefficient
//                   rows and the input span its outputs share into LDS in one round trip, then two waves run
//                   the two canonical half-chains of every output.  Exact, interpolated and variable-rate
//                   plans.  Reports completion through words in pinned host memory (ChainDone) when asked.
//   k_chain_resident  the same body as a RESIDENT kernel: launched once, fed through a mailbox (pinned host
//                   memory, or device memory the CPU stores into on large-BAR systems) — no HIP call per chunk.
//   k_interp(_tile) interpolated-phase plans (arbitrary ratios) and variable rate: per tap a cubic in
//                   the fractional position (Horner FMAs); lane per output (fallback) / outputs sorted by phase
//                   interval, large launches.
//   k_gather_wave   exact-bank launches of 4096 outputs and more that the period tiles do not take (too few periods for a
//                   slab; stream chunks written straight into host memory): a half-chain per QUAD of lanes on the
//                   phase-major bank, the chain by DPP — in place of lane-per-output k_gather.
//   k_interp_wave   the same for launches between 512 outputs and what fills the chip (a stream's 96 000-frame
//                   chunk, 1 s clips), and every large variable-rate launch: a half-chain per QUAD of lanes —
//                   lane k fetches and evaluates tap 4s + k, the chain takes the four coefficients by DPP.
//   k_tile          period-tiled VALU kernel: 64 (32, 16 where LDS demands) periods of one column staged in LDS, a wave = 16
//                   output phases whose coefficients travel on the scalar path (s_load -> SGPR operands
//                   of v_pk_fma_f32).  The f64 engine (float64 / int32 I/O); f32 A/B reference.
//   k_tile_mfma(_p) the same tiling on v_mfma_f32_16x16x4_f32 — on gfx950 the f32-input MFMA IS the
//                   k-ordered fmaf chain of the canonical arithmetic, bit for bit, at the vector ALU's
//                   peak rate, with both operands in VGPRs (prefetchable arbitrarily deep; SGPR-fed VALU
//                   FMAs top out at 47-61 TF here).  _p: k-de-interleaved LDS planes, 4-wave workgroups,
//                   software-pipelined half-chains.  The f32 engine for float32 / int16 I/O.
//   k_wave_dot      reference point only: the shape BASELINE.json's north star describes (one wavefront
//                   per output sample + shuffle reduction): 587 us where k_tile_mfma_p takes 32 —
//                   6 cross-lane steps and two LDS reads per ~4.6 FMAs.  Never chosen automatically.
// The frequency-domain engine (1e-6-class, not bit-identical: whole-signal float32/float64 device jobs)
// lives in fft.hip / fftwave.hip.
// Layout (round 6): this file holds the switches, the conversions, k_gather / k_wave_dot and the whole host side (tables,
// launchers); the kernel families are cut into kernels_interp.h, kernels_chain.h and kernels_tile.h, included below — one
// translation unit still (27 s of the build; the frequency-domain engine's three are the long pole).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "device.h"
#include "half_rules.h"
#include "job_rules.h"
#include "pcm_out.h"
#include "ragged_rules.h"
#include "tile_rules.h"
#include "vr_ragged_rules.h"

namespace hipsoxr {

const Switches &switches()
{
    static const Switches sw = [] {
        Switches w;
        auto on = [](const char *n) { return getenv(n) != nullptr; };
        auto num = [](const char *n) { const char *v = getenv(n); return v ? atoi(v) : 0; };
        w.no_fft = on("HIPSOXR_NO_FFT"); w.resident = on("HIPSOXR_RESIDENT"); w.auto_resident = on("HIPSOXR_AUTO_RESIDENT");
        if (getenv("HIPSOXR_RESIDENT_IDLE_US")) w.resident_idle_us = num("HIPSOXR_RESIDENT_IDLE_US");
#ifdef HIPSOXR_DEBUG_SWITCHES
        w.fft_no_pair = on("HIPSOXR_FFT_NO_PAIR"); w.fft_no_chpair = on("HIPSOXR_FFT_NO_CHPAIR"); w.fft_no_xcd_map = on("HIPSOXR_FFT_NO_XCD_MAP");
        w.fft_large_only = on("HIPSOXR_FFT_LARGE_ONLY"); w.fft_small_only = on("HIPSOXR_FFT_SMALL_ONLY"); w.fft_no_tiny = on("HIPSOXR_FFT_NO_TINY"); w.dbg_fft_k = num("HIPSOXR_DEBUG_FFT_K");
        w.fft_no_wave = on("HIPSOXR_FFT_NO_WAVE"); w.dbg_wave_min = num("HIPSOXR_DEBUG_WAVE_MIN"); w.dbg_wave_slots = num("HIPSOXR_DEBUG_WAVE_SLOTS");
        w.no_planes = on("HIPSOXR_NO_PLANES"); w.no_mfma64 = on("HIPSOXR_NO_MFMA64"); w.no_host_ring = on("HIPSOXR_NO_HOST_RING");
        w.no_chain = on("HIPSOXR_NO_CHAIN"); w.no_done_words = on("HIPSOXR_NO_DONE_WORDS"); w.direct_max = num("HIPSOXR_DEBUG_DIRECT_MAX");
        w.resident_no_bar = on("HIPSOXR_RESIDENT_NO_BAR"); w.no_xcd_split = on("HIPSOXR_NO_XCD_SPLIT"); w.no_tile_split = on("HIPSOXR_NO_TILE_SPLIT");
        w.no_interp_tile = on("HIPSOXR_NO_INTERP_TILE"); w.no_two_stage = on("HIPSOXR_NO_TWO_STAGE");
        w.no_interp_wave = on("HIPSOXR_NO_INTERP_WAVE"); w.no_gather_wave = on("HIPSOXR_NO_GATHER_WAVE"); w.dbg_gw_taps = num("HIPSOXR_DEBUG_GW_TAPS");
        w.dbg_flags = num("HIPSOXR_DEBUG_FLAGS"); w.dbg_nrt = num("HIPSOXR_DEBUG_NRT"); w.dbg_nw = num("HIPSOXR_DEBUG_NW");
        w.dbg_split = num("HIPSOXR_DEBUG_SPLIT"); w.dbg_chain_no = num("HIPSOXR_DEBUG_CHAIN_NO"); w.dbg_lds = (size_t)num("HIPSOXR_DEBUG_LDS");
        w.dbg_slab32 = on("HIPSOXR_DEBUG_SLAB32"); w.no_halves = on("HIPSOXR_DEBUG_NO_HALVES"); w.dbg_pad = on("HIPSOXR_DEBUG_PAD");
        w.dbg_slab64 = on("HIPSOXR_DEBUG_SLAB64"); w.dbg_mfma64_pb = num("HIPSOXR_DEBUG_MFMA64_PB"); w.dbg_mfma64_split = on("HIPSOXR_DEBUG_MFMA64_SPLIT");
        w.dbg_mfma64_lds = (size_t)num("HIPSOXR_DEBUG_MFMA64_LDS"); w.dbg_fft_lds = (size_t)num("HIPSOXR_DEBUG_FFT_LDS");
        w.dbg_tile_form = num("HIPSOXR_DEBUG_TILE_FORM"); w.dbg_poly_r = num("HIPSOXR_DEBUG_POLY_R"); w.dbg_poly_mid_budget = num("HIPSOXR_DEBUG_POLY_MID_BUDGET"); w.no_interp_pair = on("HIPSOXR_NO_INTERP_PAIR"); w.dbg_interp_pair_always = on("HIPSOXR_DEBUG_INTERP_PAIR_ALWAYS"); w.dbg_interp_no_twin = on("HIPSOXR_DEBUG_INTERP_NO_TWIN"); w.poly_no_pair = on("HIPSOXR_POLY_NO_PAIR"); w.adj_interp_per_lane = on("HIPSOXR_DEBUG_ADJ_INTERP_PER_LANE"); w.dbg_trace = getenv("HIPSOXR_DEBUG_TRACE"); w.dbg_launch_log = getenv("HIPSOXR_DEBUG_LAUNCH_LOG");
#endif
        return w;
    }();
    return sw;
}

} // namespace hipsoxr
// The debug-switch build's one export beyond include/hipsoxr.h (which does not declare it; a test sets its signature on the
// loaded library): device.h debug_stream_seek.
#ifdef HIPSOXR_DEBUG_SWITCHES
extern "C" HIPSOXR_API hipsoxr_error_t hipsoxr_debug_stream_seek(hipsoxr_stream_t *s, uint64_t in_frames, uint64_t out_frames)
{
    return hipsoxr::debug_stream_seek(s, in_frames, out_frames);
}
#endif
namespace hipsoxr {

// ---------------------------------------------------------------------------------------------
// conversions
// ---------------------------------------------------------------------------------------------
// (mix64 / dither_tpdf and the integer conversions: pcm_out.h, shared with the frequency-domain engine)
struct OutCtx {
    uint64_t *clip_counter;
    uint32_t dither, seed;
    uint32_t ch0; // channel index of the job's channel 0 in the caller's signal (jobs folded over channel ranges)
};
// set by launch_job while it issues the parts of a job folded over channel ranges: the dither of a
// channel is keyed by its index in the WHOLE signal
static thread_local uint32_t t_ch_base = 0;

// (Plain stores: a lane writes 2-8 bytes, a wave's instruction a part of each line it touches, and the L2's write combining
// is what turns that into whole-line traffic — non-temporal stores cost the 60 s clip 3 %, int32 6 %, 8-channel interleaved
// data 87 %; tools/nt_ab.sh, profiles/r04_cache_policy.txt.  The frequency-domain kernel's staged 16-byte stores are the
// case where they pay: fft.hip, FFT_STORE_AUX.)
template <typename T> __device__ __forceinline__ void put_out(T *p, T v) { *p = v; }
template <typename Real>
__device__ __forceinline__ void store_out(float *p, Real v, const OutCtx &, uint32_t, int64_t)
{
    put_out(p, (float)v);
}
template <typename Real>
__device__ __forceinline__ void store_out(double *p, Real v, const OutCtx &, uint32_t, int64_t)
{
    put_out(p, (double)v);
}
template <typename Real>
__device__ __forceinline__ void store_out(int16_t *p, Real v, const OutCtx &c, uint32_t ch, int64_t k)
{
    bool clip;
    const int16_t r = pcm_quantize_i16((float)v, c.dither != 0, c.seed, ch + c.ch0, k, clip);
    if (clip && c.clip_counter) atomicAdd((unsigned long long *)c.clip_counter, 1ULL);
    put_out(p, r);
}
template <typename Real>
__device__ __forceinline__ void store_out(int32_t *p, Real v, const OutCtx &c, uint32_t, int64_t)
{
    bool clip;
    const int32_t r = pcm_quantize_i32((double)v, clip);
    if (clip && c.clip_counter) atomicAdd((unsigned long long *)c.clip_counter, 1ULL);
    put_out(p, r);
}

__device__ __forceinline__ float fma_r(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---------------------------------------------------------------------------------------------
// k_gather
// ---------------------------------------------------------------------------------------------
struct GatherArgs {
    const void *in;
    void *out;
    const void *bank; // tap-major [T][Lpad] Real
    int64_t Lpad, L, M;
    int32_t T;
    uint32_t n_clips, n_channels;
    int64_t ics, ifs, ichs, ocs, ofs, ochs;
    int64_t in_abs0, in_frames;
    int64_t out_k0, out_frames;
    int64_t d0, p0; // out_k0*M = L*d0 + p0
    OutCtx oc;
    int32_t ch_fast; // 1: consecutive threads = consecutive channels of one frame
};

// RAGGED (a clip table on the exact engine, see kernels_tile.h): the table travels behind the arguments; a lane's clip —
// uniform over its workgroup — reads its row, and the lane asks idx < out_frames[clip].  The grid is the longest clip's.
struct GatherArgsR : GatherArgs {
    const int64_t *rows; // [n_clips][4] = in offset, in frames, out offset, out frames (elements from in / out)
};
template <bool RAGGED> struct GatherArgsOf { typedef GatherArgs type; };
template <> struct GatherArgsOf<true> { typedef GatherArgsR type; };
__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <typename IO> __device__ __forceinline__ const GatherArgs &clip_args(const GatherArgs &a, uint32_t, GatherArgs &) { return a; }
// the view of one clip: in, in_frames, out, out_frames are its row's
template <typename IO> __device__ __forceinline__ const GatherArgs &clip_view(const GatherArgs &g, const int64_t *rows, uint32_t clip, GatherArgs &v)
{
    const int64_t *row = rows + 4 * (int64_t)__builtin_amdgcn_readfirstlane(clip);
    v = g;
    v.in = (const IO *)g.in + uniform64(row[0]); v.in_frames = uniform64(row[1]);
    v.out = (IO *)g.out + uniform64(row[2]); v.out_frames = uniform64(row[3]);
    return v;
}
template <typename IO> __device__ __forceinline__ const GatherArgs &clip_args(const GatherArgsR &r, uint32_t clip, GatherArgs &v) { return clip_view<IO>(r, r.rows, clip, v); }

template <typename IO, typename Real, bool RAGGED = false>
__global__ void __launch_bounds__(256) k_gather(typename GatherArgsOf<RAGGED>::type a_)
{
    int64_t idx;
    uint32_t ch, clip;
    if (a_.ch_fast) {
        int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        idx = e / a_.n_channels;
        ch = (uint32_t)(e - idx * a_.n_channels);
        clip = blockIdx.y;
    } else {
        idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
        ch = blockIdx.y % a_.n_channels;
        clip = blockIdx.y / a_.n_channels;
    }
    [[maybe_unused]] GatherArgs row_view;
    const GatherArgs &a = clip_args<IO>(a_, clip, row_view);
    if (RAGGED ? ragged_gather_skip(idx, a.out_frames) : idx >= a.out_frames) return;
    // position: (out_k0 + idx)*M = L*d + p
    const int64_t t = a.p0 + idx * a.M;
    const int64_t q = t / a.L;
    const int64_t p = t - q * a.L;
    const int64_t n0 = a.d0 + q - (a.T / 2 - 1);  // absolute index of tap 0's input sample
    const int64_t loc0 = n0 - a.in_abs0;          // its index relative to in[frame 0]
    const IO *xin = (const IO *)a.in + (int64_t)clip * a.ics + (int64_t)ch * a.ichs;
    const Real *c = (const Real *)a.bank + p;
    const int32_t T = a.T, H = T / 2;
    Real accL = 0, accR = 0;
    // The two half-chains are independent: they advance together (each in its own canonical order),
    // eight taps of each per trip, so 32 loads are in flight per lane.  This kernel serves the small
    // launches of streaming calls, where its latency — a serial chain of T dependent FMAs fed by L2
    // loads — is the whole cost (81 us -> ~20 us for T = 736).
    if (loc0 >= 0 && loc0 + T <= a.in_frames) {
        const IO *xp = xin + loc0 * a.ifs;
#pragma unroll 8
        for (int i = 0; i < H; ++i) {
            const int jr = T - 1 - i;
            accL = fma_r(c[(int64_t)i * a.Lpad], (Real)xp[(int64_t)i * a.ifs], accL);
            accR = fma_r(c[(int64_t)jr * a.Lpad], (Real)xp[(int64_t)jr * a.ifs], accR);
        }
    } else {
#pragma unroll 4
        for (int i = 0; i < H; ++i) {
            const int jr = T - 1 - i;
            const int64_t ll = loc0 + i, lr = loc0 + jr;
            const Real xl = (ll >= 0 && ll < a.in_frames) ? (Real)xin[ll * a.ifs] : (Real)0;
            const Real xr = (lr >= 0 && lr < a.in_frames) ? (Real)xin[lr * a.ifs] : (Real)0;
            accL = fma_r(c[(int64_t)i * a.Lpad], xl, accL);
            accR = fma_r(c[(int64_t)jr * a.Lpad], xr, accR);
        }
    }
    IO *yo = (IO *)a.out + (int64_t)clip * a.ocs + idx * a.ofs + (int64_t)ch * a.ochs;
    store_out<Real>(yo, accL + accR, a.oc, ch, a.out_k0 + idx);
}

// ---------------------------------------------------------------------------------------------
// k_wave_dot — the shape BASELINE.json's north star describes, kept as a measured reference point:
// one wavefront per output sample, the taps of the phase spread over the 64 lanes (coefficient row
// and input window both read coalesced), partial dot products combined by a wavefront shuffle
// reduction.  NOT in the canonical order (a 64-way tree instead of two serial chains), so it is
// never chosen automatically and its results are 1e-6-class, not bit-identical.  Measured (DESIGN.md
// §6): far slower than the tiled kernels — six cross-lane steps and two loads per ~4.6 FMAs.
// ---------------------------------------------------------------------------------------------
template <typename IO, typename Real>
__global__ void __launch_bounds__(256) k_wave_dot(GatherArgs a, const Real *__restrict__ phase_major, int32_t per_wave)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t ch = blockIdx.y % a.n_channels, clip = blockIdx.y / a.n_channels;
    const IO *xin = (const IO *)a.in + (int64_t)clip * a.ics + (int64_t)ch * a.ichs;
    IO *yo = (IO *)a.out + (int64_t)clip * a.ocs + (int64_t)ch * a.ochs;
    const int32_t T = a.T, H = T / 2;
    for (int32_t o = 0; o < per_wave; ++o) {
        const int64_t idx = wave * per_wave + o;
        if (idx >= a.out_frames) return; // wave-uniform
        const int64_t t = a.p0 + idx * a.M, q = t / a.L, p = t - q * a.L;
        const int64_t loc0 = a.d0 + q - (H - 1) - a.in_abs0;
        const Real *c = phase_major + p * T;
        Real acc = 0;
        for (int j = lane; j < T; j += 64) {
            const int64_t l = loc0 + j;
            const Real xv = (l >= 0 && l < a.in_frames) ? (Real)xin[l * a.ifs] : (Real)0;
            acc = fma_r(c[j], xv, acc);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) store_out<Real>(yo + idx * a.ofs, acc, a.oc, ch, a.out_k0 + idx);
    }
}

#include "kernels_interp.h" // k_interp, k_gather_wave, k_interp_tile, k_interp_wave
#include "kernels_chain.h"  // k_chain, k_chain_multi, k_chain_resident
#include "kernels_tile.h"   // k_tile, k_tile_mfma, k_tile_mfma_p, k_tile_mfma64_p

// ---------------------------------------------------------------------------------------------
// host side: device tables
// ---------------------------------------------------------------------------------------------
#define HIP_TRY(expr)                                                    \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) return hipGetErrorString(e_);              \
    } while (0)

int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ensure_dyn_lds(const void *fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return nullptr;
    static std::mutex mu;
    struct Raised { const void *fn; int dev; size_t bytes; };
    static std::vector<Raised> done; // the limit each (function, device) has been raised to
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    Raised *r = nullptr;
    for (auto &e : done)
        if (e.fn == fn && e.dev == dev) { r = &e; break; }
    if (r && r->bytes >= bytes) return nullptr;
    // (the limit counts against 160 KB together with the kernel's STATIC LDS: raise to what is asked for, not to the maximum)
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (r) r->bytes = bytes;
    else done.push_back({fn, dev, bytes});
    return nullptr;
}

static inline int32_t floor4(int32_t v) { return v >= 0 ? (v / 4) * 4 : -(((-v) + 3) / 4) * 4; }

// (TileGeom, the geometry as numbers: tile_rules.h) ... and as the builders return it, with the tables' e0 words
struct TileBuild : TileGeom {
    std::vector<int32_t> e0;
};

static inline int32_t floor16(int32_t v) { return v >= 0 ? (v / 16) * 16 : -(((-v) + 15) / 16) * 16; }

// Geometry + coefficient table of k_tile_mfma_p (f32 engine, Mc % 16 == 0).
// Table: [n_rt][2][n_groups + 4][64 lanes][4 chunks]; lane (row j = l & 15, k = l >> 4), chunk c:
//   left : C'[row][i0L + 16*grp + 4*c + k]        right: C'[row][i1R - (16*grp + 4*c + k)]
// Real = double (k_tile_mfma64_p): the same table in float64, a slab of 32 periods (pb) instead of 64 — 8 bytes per
// sample — and plane rows of R doubles with R == 2 (mod 4): the 16 rows of a ds_read_b128 group then start in 16
// different 16-byte bank groups.
template <typename Real>
static TileBuild build_mfma_planes(const Plan &p, std::vector<Real> *tab)
{
    TileBuild g;
    g.variant = 2;
    g.pb = sizeof(Real) == 4 ? 64 : 32;
    const int64_t L = p.L, M = p.M;
    const int32_t T = p.T, H = T / 2;
    g.RT = 16;
    int c = 1;
    while (L * c < g.RT && c < 64) c *= 2;
    while ((M * c) % 16 != 0 && M * c * 2 <= 512 && c < 64) c *= 2;
    g.c = c; g.Lc = L * c; g.Mc = M * c;
    if (g.Mc % 16 != 0 || g.Mc > 4096 || g.Lc > 16384) return g;
    const int32_t Mc = (int32_t)g.Mc;
    g.n_rt = (int32_t)((g.Lc + 15) / 16);
    auto n_of = [&](int64_t r) { return (int32_t)((r * M) / L) - (H - 1); };
    auto p_of = [&](int64_t r) { return (r * M) % L; };
    std::vector<int32_t> i0L(g.n_rt), i1R(g.n_rt);
    int32_t I_h = 0;
    for (int rt = 0; rt < g.n_rt; ++rt) {
        int64_t r0 = (int64_t)rt * 16, r1 = std::min<int64_t>(r0 + 16, g.Lc) - 1;
        i0L[rt] = floor16(n_of(r0));
        i1R[rt] = floor16(n_of(r1) + T - 1) + 15;
        I_h = std::max(I_h, std::max(n_of(r1) + H - i0L[rt], i1R[rt] - (n_of(r0) + H) + 1));
    }
    I_h = (I_h + 15) / 16 * 16;
    g.I_h = I_h;
    int32_t i_min = INT32_MAX, i_max = INT32_MIN;
    for (int rt = 0; rt < g.n_rt; ++rt) { // +-16: the B operand of one group past either end is read too? no: only A is prefetched
        i_min = std::min(i_min, std::min(i0L[rt], i1R[rt] - I_h + 1));
        i_max = std::max(i_max, std::max(i0L[rt] + I_h - 1, i1R[rt]));
    }
    g.i_min = i_min; // multiples of 16 by construction
    g.span = i_max - i_min + 1;
    g.x_count = (g.pb - 1) * Mc + g.span;
    g.rowR = Mc / 4;
    if (sizeof(Real) == 4) while ((g.rowR % 8) != 4) ++g.rowR; // R/4 odd -> conflict-free ds_read_b128 across the 16 periods
    else while ((g.rowR % 4) != 2) ++g.rowR;                    // float64: R/2 odd
    g.pad = g.rowR - Mc / 4;
    const int32_t rows_total = (g.x_count + Mc - 1) / Mc + 3; // + slack rows: pipelined reads overrun by one group
    g.plane = (rows_total * g.rowR + 63) / 64 * 64;
    g.lds_bytes = ((size_t)g.plane * 4 + g.rowR) * sizeof(Real);
    // Groups a tile's half-chain really needs (bits 24..31 of its e0 word): the table rows are I_h long for every
    // tile — the longest span over all tiles, rounded to 16, from a start rounded down to 16 — but the groups past a
    // tile's own last tap hold only zero coefficients, and fma(0, x, acc) == acc: they are not issued (10-11 of 12
    // groups at 48k -> 44.1k VHQ).
    g.e0.resize((size_t)g.n_rt * 2);
    for (int rt = 0; rt < g.n_rt; ++rt) {
        const int64_t r0 = (int64_t)rt * 16, r1 = std::min<int64_t>(r0 + 16, g.Lc) - 1;
        const int32_t gl = (n_of(r1) + H - i0L[rt] + 15) / 16, gr = (i1R[rt] - (n_of(r0) + H) + 1 + 15) / 16;
        g.e0[rt * 2 + 0] = (i0L[rt] - i_min) | (std::min(gl, I_h / 16) << 24);
        g.e0[rt * 2 + 1] = (i1R[rt] - 15 - i_min) | (std::min(gr, I_h / 16) << 24);
    }
    if (g.lds_bytes > 160 * 1024 || g.x_count + I_h >= (1 << 24) || I_h / 16 > 127) return g;
    g.ok = true;
    if (tab) {
        const int ng = I_h / 16;
        tab->assign((size_t)g.n_rt * 2 * (ng + 4) * 256, (Real)0);
        for (int rt = 0; rt < g.n_rt; ++rt)
            for (int rr = 0; rr < 16; ++rr) {
                int64_t r = (int64_t)rt * 16 + rr;
                if (r >= g.Lc) continue;
                const int32_t nr = n_of(r);
                const double *cp = p.bank.data() + (size_t)(p_of(r) * T);
                for (int ii = 0; ii < I_h; ++ii) {
                    const int grp = ii / 16, cc = (ii % 16) / 4, k = ii % 4, lane = k * 16 + rr;
                    const size_t at = ((size_t)grp * 64 + lane) * 4 + cc;
                    int32_t jl = i0L[rt] + ii - nr;
                    if (jl >= 0 && jl < H) (*tab)[(size_t)(rt * 2 + 0) * (ng + 4) * 256 + at] = (Real)cp[jl];
                    int32_t jr = i1R[rt] - ii - nr;
                    if (jr >= H && jr < T) (*tab)[(size_t)(rt * 2 + 1) * (ng + 4) * 256 + at] = (Real)cp[jr];
                }
            }
    }
    return g;
}

// Tile geometry + (optionally) tables for one precision.
template <typename Real>
static TileBuild build_tile_tables(const Plan &p, std::vector<Real> *tab, int variant = 0)
{
    TileBuild g;
    g.variant = variant;
    const int64_t L = p.L, M = p.M;
    const int32_t T = p.T, H = T / 2;
    g.RT = 16;
    // replicate short periods so that a period holds at least one full tile
    int c = 1;
    while (L * c < g.RT && c < 64) c *= 2;
    // prefer an input period that is a multiple of 4 (b128 LDS reads) when the slab stays small
    if (variant == 0 && (M % 2 == 0 || M * 4 <= 256))
        while ((M * c) % 4 != 0 && M * c * 2 <= 256 && c < 64) c *= 2;
    g.c = c;
    g.Lc = L * c; g.Mc = M * c;
    if (g.Mc > 8192 || g.Lc > 16384) return g; // period too long for an LDS-resident slab
    g.aligned = variant == 0 && (g.Mc % 4 == 0);
    const int32_t Mc = (int32_t)g.Mc;
    if (variant == 1) {
        // k_tile_mfma: a 32-lane half reads x[(16 periods j)*S + (2 inputs k)] with ds_read_b32;
        // conflict-free iff the row stride S = Mc + pad is 2*odd (mod 32).
        g.pad = 0;
        while (((Mc + g.pad) % 4) != 2) ++g.pad;
        // Odd periods (441, 147 ...) run UNPADDED (round 3): a lane's LDS offset is then just its input index — no
        // period-boundary test and no second offset in the chain's inner step (five vector-ALU instructions per chunk
        // fewer, in a loop that is bound by exactly those) — at the price of two-way conflicts on about half the
        // banks of each B read (row stride odd: the sixteen periods start in sixteen different banks, their second
        // input collides with a neighbour's first).
        if (Mc % 2 == 1 && !switches().dbg_pad) g.pad = 0;
    } else if (g.aligned) { // row stride = 4*odd words -> conflict-free ds_read_b128 across lanes
        g.pad = ((Mc / 4) % 2 == 0) ? 4 : 0;
    } else {         // row stride odd -> conflict-free ds_read_b32
        g.pad = (Mc % 2 == 0) ? 1 : 0;
    }
    g.n_rt = (int32_t)((g.Lc + g.RT - 1) / g.RT);
    auto n_of = [&](int64_t r) { return (int32_t)((r * M) / L) - (H - 1); };
    auto p_of = [&](int64_t r) { return (r * M) % L; };
    std::vector<int32_t> i0L(g.n_rt), i1R(g.n_rt);
    int32_t I_h = 0;
    for (int rt = 0; rt < g.n_rt; ++rt) {
        int64_t r0 = (int64_t)rt * g.RT, r1 = std::min<int64_t>(r0 + g.RT, g.Lc) - 1;
        int32_t a0 = n_of(r0), a1 = n_of(r1) + T - 1;
        if (g.aligned) {
            a0 = floor4(a0);
            a1 = floor4(a1) + 3; // smallest value >= a1 that is == 3 (mod 4)
        }
        i0L[rt] = a0; i1R[rt] = a1;
        int32_t IL = n_of(r1) + H - a0;        // inputs a0 .. n_r1+H-1
        int32_t IR = a1 - (n_of(r0) + H) + 1;  // inputs n_r0+H .. a1
        I_h = std::max(I_h, std::max(IL, IR));
    }
    I_h = variant == 1 ? (I_h + 15) / 16 * 16 : (I_h + 3) / 4 * 4; // k_tile_mfma works in groups of 4 chunks
    g.I_h = I_h;
    int32_t i_min = INT32_MAX, i_max = INT32_MIN;
    for (int rt = 0; rt < g.n_rt; ++rt) {
        i_min = std::min(i_min, std::min(i0L[rt], i1R[rt] - I_h + 1));
        i_max = std::max(i_max, std::max(i0L[rt] + I_h - 1, i1R[rt]));
    }
    i_min = floor4(i_min); i_max = floor4(i_max) + 3; // slab = whole quads (vectorised staging)
    g.i_min = i_min;
    g.span = i_max - i_min + 1;
    // periods per slab: 64 (one per lane); the VALU kernel also runs with 32 or 16 (the other lanes idle) when the
    // slab would not fit — float64 at 44.1k -> 16k: 64 x 441 x 8 B = 226 KB — which still beats one lane per output
    // walking T dependent loads by 5x (60 s mono int32: 1015 us on k_gather)
    g.pb = 64;
    for (;;) {
        g.x_count = ((g.pb - 1) * Mc + (i_max - i_min + 1) + 3) / 4 * 4; // whole quads ((pb-1)*Mc may be odd)
        g.lds_bytes = ((size_t)g.x_count + (size_t)g.pad * (g.x_count / Mc + 1) + 8) * sizeof(Real);
        // (variant 1 in float64 — k_tile_mfma<IO, double, NG> — runs NG = pb / 16 groups of 16 periods: 4, 2 or 1)
        // Slab of the float64 MFMA kernel: a 64-period slab only when small (two or more workgroups per CU must fit: a lone
        // workgroup cannot hide its own staging — 48k -> 44.1k int32 60 s: 105 us on 83 KB slabs, 90 us on 42 KB ones),
        // else 32 periods up to 120 KB (44.1k -> 16k: 72 us on 116 KB against 84 us on 59 KB), else 16.
        const size_t limit = (variant == 1 && sizeof(Real) == 8)
                                 ? (g.pb == 64 ? 0 /* (four period groups of float64: 64 accumulator registers — the pipelined chain no longer fits; two groups it is) */
                                               : switches().dbg_mfma64_lds ? switches().dbg_mfma64_lds : 120 * 1024) : 160 * 1024;
        if (g.lds_bytes <= limit || (variant != 0 && sizeof(Real) == 4) || g.pb == 16) break;
        g.pb /= 2;
    }
    g.e0.resize((size_t)g.n_rt * 2);
    for (int rt = 0; rt < g.n_rt; ++rt) {
        g.e0[rt * 2 + 0] = i0L[rt] - i_min;
        g.e0[rt * 2 + 1] = i1R[rt] - 3 - i_min;
    }
    if (g.lds_bytes > 160 * 1024) return g;
    g.ok = true;
    if (tab) {
        const size_t rows = (size_t)I_h + (variant == 1 ? 16 : 0); // prefetch slack (zeros)
        tab->assign((size_t)g.n_rt * 2 * rows * g.RT, (Real)0);
        for (int rt = 0; rt < g.n_rt; ++rt) {
            Real *tl = tab->data() + (size_t)(rt * 2 + 0) * rows * g.RT;
            Real *tr = tab->data() + (size_t)(rt * 2 + 1) * rows * g.RT;
            for (int rr = 0; rr < g.RT; ++rr) {
                int64_t r = (int64_t)rt * g.RT + rr;
                if (r >= g.Lc) continue;
                const int32_t nr = n_of(r);
                const double *cp = p.bank.data() + (size_t)(p_of(r) * T);
                for (int ii = 0; ii < I_h; ++ii) {
                    int32_t jl = i0L[rt] + ii - nr;
                    if (jl >= 0 && jl < H) tl[(size_t)ii * g.RT + rr] = (Real)cp[jl];
                    int32_t jr = i1R[rt] - ii - nr;
                    if (jr >= H && jr < T) tr[(size_t)ii * g.RT + rr] = (Real)cp[jr];
                }
            }
        }
    }
    return g;
}

// a host table into device memory of its own
template <typename T>
static const char *upload(void **dst, const std::vector<T> &v)
{
    HIP_TRY(hipMalloc(dst, v.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return nullptr;
}

template <typename Real>
static const char *bank_upload(Plan *p, DeviceBank &d, TileGeom *geom_out, TileGeom *geom_m_out)
{
    const int64_t L = p->L;
    const int32_t T = p->T;
    if (p->phases) { // interpolated-phase plan: the cubic table in the engine precision, nothing else
        std::vector<Real> tb(p->bank.size());
        for (size_t i = 0; i < tb.size(); ++i) tb[i] = (Real)p->bank[i];
        return upload(&d.interp_tab, tb);
    }
    d.Lpad = (L + 15) / 16 * 16;
    std::vector<Real> tm((size_t)T * d.Lpad, (Real)0);
    for (int64_t ph = 0; ph < L; ++ph)
        for (int j = 0; j < T; ++j) tm[(size_t)j * d.Lpad + ph] = (Real)p->bank[(size_t)(ph * T + j)];
    if (const char *e = upload(&d.tap_major, tm)) return e;

    std::vector<Real> tab;
    TileBuild g = build_tile_tables<Real>(*p, &tab);
    if (g.ok) {
        if (const char *e = upload(&d.tile_tab, tab)) return e;
        if (const char *e = upload((void **)&d.tile_i0, g.e0)) return e;
        d.RT = g.RT; d.n_rt = g.n_rt; d.I_h = g.I_h;
    }
    *geom_out = g;
    // the MFMA tiles — float32: k_tile_mfma_p where the period admits planes, else k_tile_mfma; the float64 engine on
    // v_mfma_f64_16x16x4_f64: k_tile_mfma64_p, else k_tile_mfma<IO, double, NG>
    if (geom_m_out && !(sizeof(Real) == 8 && switches().no_mfma64)) {
        std::vector<Real> tabm;
        TileBuild gm = build_mfma_planes<Real>(*p, &tabm);
        if (!gm.ok || switches().no_planes) gm = build_tile_tables<Real>(*p, &tabm, 1);
        if (gm.ok) {
            if (const char *e = upload(&d.tile_tab_m, tabm)) return e;
            if (const char *e = upload((void **)&d.tile_i0_m, gm.e0)) return e;
        }
        *geom_m_out = gm;
    }
    return nullptr;
}

// geometry is cheap to recompute; keep it beside the bank in a side table keyed by (plan, prec)
static std::mutex g_geom_mu;
static std::vector<std::pair<std::pair<const Plan *, int>, TileGeom>> g_geoms; // key: (plan, prec*2+variant)

static TileGeom *geom_find(const Plan *p, int prec, int variant)
{
    for (auto &e : g_geoms)
        if (e.first.first == p && e.first.second == prec * 2 + variant) return &e.second;
    return nullptr;
}

const char *device_bank_ensure(Plan *p, int prec)
{
    std::lock_guard<std::mutex> lk(p->mu);
    DeviceBank &d = p->dev[prec];
    int cur = -1;
    if (p->device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != p->device)
        return "this plan's device tables live on another device (one plan per device)";
    if (d.ready) return nullptr;
    if (device_count() <= 0) return kNoDevice;
    if (p->device < 0 && hipGetDevice(&cur) == hipSuccess) p->device = cur; // tables are built on first use, here
    TileGeom g, gm;
    const char *e = prec == 0 ? bank_upload<float>(p, d, &g, &gm) : bank_upload<double>(p, d, &g, &gm);
    if (e) return e;
    {
        std::lock_guard<std::mutex> lk2(g_geom_mu);
        g_geoms.push_back({{p, prec * 2 + 0}, g});
        g_geoms.push_back({{p, prec * 2 + 1}, gm});
    }
    d.ready = true;
    return nullptr;
}

void device_bank_release(Plan *p)
{
    for (int i = 0; i < 2; ++i) {
        DeviceBank &d = p->dev[i];
        if (d.tap_major) (void)hipFree(d.tap_major);
        if (d.phase_major) (void)hipFree(d.phase_major);
        if (d.interp_tab) (void)hipFree(d.interp_tab);
        if (d.tile_tab) (void)hipFree(d.tile_tab);
        if (d.tile_i0) (void)hipFree(d.tile_i0);
        if (d.tile_tab_m) (void)hipFree(d.tile_tab_m);
        if (d.tile_i0_m) (void)hipFree(d.tile_i0_m);
        d = DeviceBank();
    }
    std::lock_guard<std::mutex> lk2(g_geom_mu);
    for (size_t i = 0; i < g_geoms.size();)
        if (g_geoms[i].first.first == p) g_geoms.erase(g_geoms.begin() + i);
        else ++i;
}

// ---------------------------------------------------------------------------------------------
// launch: what the launchers share
// ---------------------------------------------------------------------------------------------
template <typename Real> static DeviceBank &bank_of(Plan *p) { return p->dev[sizeof(Real) == 4 ? 0 : 1]; }

static inline int32_t log2_phases(int32_t P) { int32_t lg = 0; while ((1 << lg) < P) ++lg; return lg; }

// Outputs [k0, k0 + nf) of job j, the first of them out_offset elements behind j.out.
template <typename IO>
static GatherArgs make_gather_args(const Plan &p, const DeviceBank &d, const hipsoxr_job_t &j, int64_t k0, int64_t nf, int64_t out_offset)
{
    GatherArgs a;
    a.in = j.in;
    a.out = (char *)j.out + (size_t)out_offset * sizeof(IO);
    a.bank = d.tap_major; a.Lpad = d.Lpad; a.L = p.L; a.M = p.M; a.T = p.T;
    a.n_clips = j.n_clips; a.n_channels = j.n_channels;
    a.ics = j.in_clip_stride; a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride;
    a.ocs = j.out_clip_stride; a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.in_abs0 = j.in_abs0; a.in_frames = j.in_frames;
    a.out_k0 = k0; a.out_frames = nf;
    __int128 kM = (__int128)k0 * p.M;
    a.d0 = (int64_t)(kM / p.L); a.p0 = (int64_t)(kM % p.L);
    a.oc.clip_counter = j.clip_counter; a.oc.dither = j.dither; a.oc.seed = j.dither_seed; a.oc.ch0 = t_ch_base;
    a.ch_fast = (j.n_channels > 1 && j.in_chan_stride == 1) ? 1 : 0;
    return a;
}

static void set_interp_table(InterpArgs &x, const Plan &p, const DeviceBank &d) { x.tab = d.interp_tab; x.P = p.phases; x.lgP = log2_phases(p.phases); }

// The exact bank phase-major ([L][T], DeviceBank::phase_major), uploaded on first use.
template <typename Real>
static const char *ensure_phase_major(Plan *p)
{
    DeviceBank &d = bank_of<Real>(p);
    std::lock_guard<std::mutex> lk(p->mu);
    if (d.phase_major) return nullptr;
    std::vector<Real> pm(p->bank.size());
    for (size_t i = 0; i < pm.size(); ++i) pm[i] = (Real)p->bank[i];
    if (hipMalloc(&d.phase_major, pm.size() * sizeof(Real)) != hipSuccess) return "hipMalloc failed";
    if (hipMemcpy(d.phase_major, pm.data(), pm.size() * sizeof(Real), hipMemcpyHostToDevice) != hipSuccess) return "hipMemcpy failed";
    return nullptr;
}

// Variable rate: the clock at a launch's first output — (T0, S0) advanced by the `done` outputs in front of it.
static void vr_advance(const VrPos &vr, int64_t done, InterpArgs &x)
{
    typedef unsigned __int128 u128;
    const u128 T0 = ((u128)vr.t_hi << 64) | vr.t_lo, S0 = ((u128)vr.s_hi << 64) | vr.s_lo, D = ((u128)vr.d_hi << 64) | vr.d_lo;
    const u128 n = (u128)(uint64_t)done, m = n * (n - 1) / 2;
    const u128 T1 = T0 + n * S0 + D * (done ? m : 0), S1 = S0 + D * n;
    x.t_hi = (uint64_t)(T1 >> 64); x.t_lo = (uint64_t)T1;
    x.s_hi = (uint64_t)(S1 >> 64); x.s_lo = (uint64_t)S1;
    x.d_hi = vr.d_hi; x.d_lo = vr.d_lo;
}
// ... and the largest step (input samples per output) among the clock's first `upto` outputs
static double vr_max_step(const VrPos &vr, int64_t upto)
{
    const double two64 = 18446744073709551616.;
    const double s0 = (double)vr.s_hi + (double)vr.s_lo / two64;
    const double dd = (double)(int64_t)vr.d_hi + (double)vr.d_lo / two64;
    return std::max(s0, s0 + dd * (double)upto) * (1. + 1e-9);
}

// Geometry of k_chain / k_chain_multi for launches of at most n_out outputs per column: outputs per workgroup, LDS room for
// the shared input span (samples), LDS bytes.
struct ChainGeom { int NO; int32_t span_cap; size_t lds; bool ok; };
template <typename Real>
static ChainGeom chain_geom(const Plan &p, int64_t n_out)
{
    ChainGeom g;
    // few outputs per workgroup: the staging loop is then two or three trips of 16 loads per
    // thread (its latency is the kernel's latency), and there are enough workgroups anyway
    // (above 512 outputs 32 per workgroup: at most 64 workgroups then read their span over PCIe, poll the mailbox
    //  of the resident form, or report through completion words — 4410-frame chunks 25.3 -> 22.7 us per call)
    g.NO = n_out <= 512 ? 8 : 32;
    if (switches().dbg_chain_no) g.NO = switches().dbg_chain_no;
    // LDS: NO coefficient rows of T + V words, the shared input span (T + what NO-1 window shifts of at
    // most ceil(M/L) + 1 samples add; variable rate: the plan's ratio is the largest step), bookkeeping
    const int64_t shift = (p.M + p.L - 1) / p.L + 2;
    auto chain_lds = [&](int no) {
        const int64_t sc = (int64_t)p.T + (int64_t)no * shift + 4;
        g.span_cap = (int32_t)sc;
        return (size_t)no * (p.T + 16 / sizeof(Real)) * sizeof(Real) + (size_t)((sc + 3) & ~3) * sizeof(Real) + (size_t)no * 16;
    };
    while (g.NO > 2 && chain_lds(g.NO) > 150 * 1024) g.NO /= 2;
    g.lds = chain_lds(g.NO);
    g.ok = g.lds <= 150 * 1024 && shift < (1 << 20);
    return g;
}

// Geometry of the half-chain-per-quad kernels (k_gather_wave, k_interp_wave): a workgroup's 32 consecutive outputs reach over
// T inputs plus `reach`, what the 31 window shifts between them add.
struct WaveGeom { int64_t span = 0; size_t lds = 0; bool ok = false; };
template <typename Real>
static WaveGeom wave_geom(int64_t reach, int32_t T)
{
    WaveGeom g;
    g.span = (reach + T + 4 + 3) & ~(int64_t)3;
    g.lds = (size_t)(g.span + 32) * sizeof(Real);
    g.ok = g.lds <= 64 * 1024;
    return g;
}

// Completion words (ChainDone): a launch that is the whole job, of at most cd->cap workgroups, takes them.
static inline void claim_done_words(ChainDone *cd, bool whole_job, uint64_t wgs, uint32_t **words, uint32_t *seq)
{
    if (!cd || !whole_job || wgs > cd->cap) return;
    *words = cd->words; *seq = cd->seq;
    cd->n_wgs = (uint32_t)wgs;
}

// One launch's share of a job, as launch_gather hands it to the launcher of the form it chose.
struct GatherLaunch {
    const hipsoxr_job_t &j;
    hipStream_t st;
    const VrPos *vr;  // variable rate: the clock at the JOB's first output
    ChainDone *cd;    // completion words on offer, or nullptr
    int64_t done, nf; // outputs [done, done + nf) of the job
    uint64_t cols;    // (clip, channel) columns
    GatherArgs a;
    // a ragged launch (launch_ragged_interp): the device rows of the launch's j.n_clips clips — nf is then the longest clip's
    // out_frames, a.ics == a.ocs == 0 (a clip's place is its row's) — and the clip count the log line carries
    const int64_t *rows = nullptr;
    int64_t ragged = -1;
    // ... of a ragged variable-rate launch (launch_ragged_vr; vr then only says so): the device clock table, a step per clip
    const uint64_t *clock = nullptr;
    bool whole_job() const { return done == 0 && nf == j.out_frames; }
    // per_wg outputs of one column per workgroup
    dim3 grid(int per_wg) const { return dim3((unsigned)((nf + per_wg - 1) / per_wg), (unsigned)cols, 1); }
};

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): one line per launch of launch_gather's family, in the style of
// tile_launch_log — what tests/test_gpu_interp_forms.py and test_gpu_gather_forms.py read the form from.  `form`: its own fields.
#ifdef HIPSOXR_DEBUG_SWITCHES
template <typename IO, typename Real>
__attribute__((format(printf, 7, 8)))
static void gather_launch_log(const char *kernel, const Plan &p, const GatherLaunch &c, dim3 grid, unsigned block, size_t lds, const char *form, ...)
{
    FILE *fl = fopen(switches().dbg_launch_log, "a");
    if (!fl) return;
    fprintf(fl, "kernel=%s width=%zu io=%c%zu vr=%d L=%lld M=%lld T=%d P=%d done=%lld nf=%lld cols=%llu k0=%lld in_abs0=%lld grid=%ux%ux%u block=%u lds=%zu", kernel,
            sizeof(Real), std::is_integral<IO>::value ? 'i' : 'f', sizeof(IO) * 8, c.vr ? 1 : 0, (long long)p.L, (long long)p.M, (int)p.T, (int)p.phases,
            (long long)c.done, (long long)c.nf, (unsigned long long)c.cols, (long long)c.a.out_k0, (long long)c.a.in_abs0, grid.x, grid.y, grid.z, block, lds);
    if (*form) {
        va_list ap;
        va_start(ap, form);
        fputc(' ', fl);
        vfprintf(fl, form, ap);
        va_end(ap);
    }
    if (c.ragged >= 0) fprintf(fl, " ragged=%lld", (long long)c.ragged);
    fputc('\n', fl);
    fclose(fl);
}
#define GATHER_LAUNCH_LOG(...) do { if (switches().dbg_launch_log) gather_launch_log<IO, Real>(__VA_ARGS__); } while (0)
#else
#define GATHER_LAUNCH_LOG(...) ((void)0)
#endif

// ---- launch: one function per kernel form ----
template <typename IO, typename Real>
static const char *launch_gather_wave(Plan *p, const GatherLaunch &c, const WaveGeom &g)
{
    if (const char *e = ensure_phase_major<Real>(p)) return e;
    GatherWaveArgs ga;
    ga.g = c.a; ga.phase_major = bank_of<Real>(p).phase_major; ga.span_cap = (int32_t)g.span; ga.done_words = nullptr; ga.done_seq = 0;
    const dim3 grid = c.grid(32);
    claim_done_words(c.cd, c.whole_job(), (uint64_t)grid.x * grid.y, &ga.done_words, &ga.done_seq);
    GATHER_LAUNCH_LOG("gather_wave", *p, c, grid, 256, g.lds, "span_cap=%d cw=%d", (int)ga.span_cap, ga.done_words ? 1 : 0);
    hipLaunchKernelGGL((k_gather_wave<IO, Real>), grid, dim3(256), g.lds, c.st, ga);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// the resident form of k_chain: same staging, same chains, fed by messages (k_chain_resident)
template <typename IO, typename Real>
static const char *launch_chain_resident(Plan *p, const GatherLaunch &c, const ChainGeom &g, const ChainArgs &ca, ResidentLaunch *res)
{
    if (p->L >= (1 << 24) && !c.vr) return "resident kernel: ratio numerator too large";
    void (*rk)(ResidentArgs) = c.vr ? k_chain_resident<IO, Real, 2> : p->phases ? k_chain_resident<IO, Real, 1> : k_chain_resident<IO, Real, 0>;
    const dim3 grid = c.grid(g.NO);
    const int64_t wgs = (int64_t)grid.x * grid.y;
    // every workgroup must be on the chip at once (they wait for each other): a quarter of the slots at most
    int occ = 0, dev = 0, cus = 0;
    if (const char *e = ensure_dyn_lds((const void *)rk, g.lds)) return e;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)rk, 256, g.lds));
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (occ < 1 || wgs > (int64_t)occ * cus / 4 || wgs > (int64_t)kResidentMaxWgs) return "resident kernel: message too large";
    // process-wide budget in CU capacity (engine.cpp): all resident instances together hold at most half the chip
    res->cost_mcu = (uint32_t)((wgs * 1024 + occ - 1) / occ);
    if (res->used_mcu + (int64_t)res->cost_mcu > ((int64_t)cus * 1024) >> res->budget_shift) { res->over_budget = true; return "resident kernel: over the budget"; }
    ResidentArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.ca = ca; ra.box = res->box; ra.words = res->words; ra.ctl = res->ctl; ra.base_seq = res->base_seq; ra.epoch = res->epoch;
    ra.idle_ticks = res->idle_us * 100; // wall_clock64: 100 MHz
    ra.n_wgs = (uint32_t)wgs;
    res->n_wgs = ra.n_wgs; res->max_out = (int64_t)grid.x * g.NO;
    GATHER_LAUNCH_LOG("chain_resident", *p, c, grid, 256, g.lds, "NO=%d span_cap=%d mode=%d", g.NO, (int)g.span_cap, c.vr ? 2 : p->phases ? 1 : 0);
    hipLaunchKernelGGL(rk, grid, dim3(256), g.lds, c.st, ra);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// k_chain — exact, interpolated and variable-rate plans; res: as the resident kernel instead
template <typename IO, typename Real>
static const char *launch_chain(Plan *p, const GatherLaunch &c, const ChainGeom &g, ResidentLaunch *res)
{
    ChainArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.ia.g = c.a; ca.NO = g.NO; ca.span_cap = g.span_cap;
    void (*ck)(ChainArgs) = nullptr;
    if (p->phases) {
        set_interp_table(ca.ia, *p, bank_of<Real>(p));
        if (c.vr && (1 << ca.ia.lgP) != ca.ia.P) return "variable-rate needs a power-of-two phase count";
        if (c.vr) vr_advance(*c.vr, c.done, ca.ia);
        ck = c.vr ? k_chain<IO, Real, 2> : k_chain<IO, Real, 1>;
    } else {
        if (const char *e = ensure_phase_major<Real>(p)) return e;
        ca.phase_major = bank_of<Real>(p).phase_major;
        ck = k_chain<IO, Real, 0>;
    }
    if (res) return launch_chain_resident<IO, Real>(p, c, g, ca, res);
    if (const char *e = ensure_dyn_lds((const void *)ck, g.lds)) return e;
    const dim3 grid = c.grid(g.NO);
    claim_done_words(c.cd, c.whole_job(), (uint64_t)grid.x * grid.y, &ca.done_words, &ca.done_seq);
    GATHER_LAUNCH_LOG("chain", *p, c, grid, 256, g.lds, "NO=%d span_cap=%d mode=%d cw=%d", g.NO, (int)g.span_cap, c.vr ? 2 : p->phases ? 1 : 0, ca.done_words ? 1 : 0);
    hipLaunchKernelGGL(ck, grid, dim3(256), g.lds, c.st, ca);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// a half-chain per quad of lanes (k_interp_wave)
template <typename IO, typename Real>
static const char *launch_interp_wave(const Plan &p, const GatherLaunch &c, const InterpArgs &ia, const WaveGeom &g)
{
    InterpWaveArgs wa;
    wa.ia = ia; wa.span_cap = (int32_t)g.span; wa.done_words = nullptr; wa.done_seq = 0;
    if (c.rows) { // the ragged form: the frame axis is the longest clip's (c.nf), no completion words
        InterpWaveArgsR wr;
        (InterpWaveArgs &)wr = wa;
        wr.rows = c.rows; wr.clock = c.clock;
        const dim3 rgrid((unsigned)ragged_span_grid_x(c.nf, 32), (unsigned)c.cols, 1);
        void (*rk)(InterpWaveArgsR) = c.vr ? k_interp_wave<IO, Real, true, true> : k_interp_wave<IO, Real, false, true>;
        GATHER_LAUNCH_LOG("interp_wave", p, c, rgrid, 256, g.lds, "span_cap=%d", (int)wa.span_cap);
        hipLaunchKernelGGL(rk, rgrid, dim3(256), g.lds, c.st, wr);
        HIP_TRY(hipGetLastError());
        return nullptr;
    }
    const dim3 grid = c.grid(32);
    claim_done_words(c.cd, c.whole_job(), (uint64_t)grid.x * grid.y, &wa.done_words, &wa.done_seq);
    void (*wk)(InterpWaveArgs) = c.vr ? k_interp_wave<IO, Real, true> : k_interp_wave<IO, Real, false>;
    GATHER_LAUNCH_LOG("interp_wave", p, c, grid, 256, g.lds, "span_cap=%d", (int)wa.span_cap);
    hipLaunchKernelGGL(wk, grid, dim3(256), g.lds, c.st, wa);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// k_interp_tile, the throughput kernel for large interpolated launches: KO outputs per workgroup, as many as LDS allows
// (input span + 2 bytes of bookkeeping per output), at least ~32 outputs per interval.  KO == 0: not this kernel.
struct InterpTileForm {
    int64_t KO = 0, span_cap = 0;
    int pair_mode = 0;           // 0 one output per lane, 1 channel pairs, 2 the column's two halves
    bool twin = false;           // ... pairs with the span staged twice (float: 16-byte aligned reads)
    int64_t split_h = 0, nf_t = 0; // (outputs the tiles are counted over: member 1's)
};
// The form for nf outputs per column at `step` input samples per output, against the lane-per-output kernels' cost
// (wave_ok: k_interp_wave is the alternative, else k_interp).  rows: a ragged launch over the j.n_clips clips of that table —
// nf is the longest clip's (what sizes KO), the two costs are fed the table's real numbers (the workgroups that do work and
// the outputs, summed over the clips: ragged_span_total, ragged_total_out), not longest x clips; pair modes {0, 1}.
template <typename Real>
static InterpTileForm interp_tile_form(const Plan &p, const hipsoxr_job_t &j, int64_t nf, double step, bool vr, bool wave_ok,
                                       const int64_t *rows = nullptr)
{
    InterpTileForm f;
    f.nf_t = nf;
    // a bucket (outputs of one interval) is served 64 at a time: aim at a mean of 60 per
    // interval (30, 15 when LDS cannot hold that many outputs and their input span)
    // (round 3: among the sizes that fit, the one that leaves the fewest workgroup-layers x outputs per
    //  workgroup on the 256 CUs — 48000 -> 44101 stereo 60 s: 60 per interval are 346 workgroups, two layers
    //  of which the second is a third full; 41 per interval are 506)
    // two outputs per lane (InterpTileArgs): neighbouring channels of an even channel count, else — constant rate —
    // the column's own second half, split h periods of L outputs in when that half has >= 0.7 of the first's outputs
    // — taken when the launch's workgroup layers x outputs per workgroup come out cheaper than with one output
    // per lane (a pair workgroup takes ~1.7x a single one: 60 s stereo 393 -> 348 us, 8 channels 1622 -> 1120,
    // mono 232 -> 190; a 10 s stereo job has too few workgroups to halve them)
    constexpr double kPairWg = 1.7, kTwinWg = 1.4; // (... 1.4 with the span staged twice for 16-byte reads: stereo 348 -> 296, mono 190 -> 145)
    int cand_mode = 0;
    int64_t cand_h = 0, cand_nf = nf;
    if (!switches().no_interp_pair) {
        if (j.n_channels % 2 == 0) cand_mode = 1;
        else if (!vr && !rows) {
            const int64_t h = (nf + 2 * p.L - 1) / (2 * p.L), n1 = h * p.L;
            if (h >= 1 && n1 < nf && 10 * (nf - n1) >= 7 * n1 && h * p.M < ((int64_t)1 << 40)) { cand_mode = 2; cand_h = h; cand_nf = n1; }
        }
    }
    double best_cost = 1e300, cols_ = (double)j.n_clips * j.n_channels;
    for (int mode : {0, cand_mode}) {
        if (mode == 0 && cand_mode && switches().dbg_interp_pair_always) continue;
        const int nm = mode ? 2 : 1;
        const int64_t nft = mode == 2 ? cand_nf : nf;
        const double cols_m = (double)j.n_clips * j.n_channels / (mode == 1 ? 2 : 1);
        for (int tw = 0; tw <= (mode && sizeof(Real) == 4 && !switches().dbg_interp_no_twin ? 1 : 0); ++tw) // float pairs: one or two copies of the span
            for (int per = 64; per >= 15; --per) {
                const int64_t k = (int64_t)per * p.phases;
                if (k > 16384 || k > nft) continue;
                const int64_t sc = (int64_t)std::ceil((double)k * step) + p.T + 8;
                const int64_t bytes = (tw ? 2 * (sc + 4) : sc) * nm * (int64_t)sizeof(Real) + k * 2 + (2 * p.phases + 2) * 4 + 64;
                if (bytes > 150 * 1024) continue;
                const double wgs_ = rows ? (double)ragged_span_total(rows, j.n_clips, j.n_channels / (mode == 1 ? 2 : 1), k)
                                         : std::ceil((double)nft / (double)k) * cols_m;
                const double cost = std::ceil(wgs_ / 256.) * (double)k * (per >= 30 ? 1. : 30. / per) * (tw ? kTwinWg : mode ? kPairWg : 1.); // (thin buckets: idle lanes)
                if (cost < best_cost) { best_cost = cost; f.KO = k; f.span_cap = sc; f.pair_mode = mode; f.twin = tw != 0; f.split_h = mode == 2 ? cand_h : 0; f.nf_t = nft; cols_ = cols_m; }
            }
        if (!cand_mode) break;
    }
    // ... which pays off once the launch fills the chip.  A workgroup of it is long (KO outputs x T taps one
    // interval at a time: ~130 us at VHQ, 1.5 ms with the variable-rate clock), so a launch of a few of them
    // loses to lane-per-output k_interp, whose time grows with the work instead (measured, us per output x tap:
    // k_interp 2.5e-6; a k_interp_tile workgroup 6.3e-5 constant rate, 2.9e-4 variable rate; 256 CUs):
    // 96 000-frame variable-rate chunk 1.5 ms -> 0.1 ms on k_interp; 10 s stereo constant rate 134 us on
    // the tile kernel (503 on k_interp); 1 s stereo 75 us on k_interp (127 on the tile kernel).
    constexpr double kWaveUsPerTap = 1.0e-6; // k_interp_wave: us per output x tap, 256 CUs
    if (f.KO) {
        const double wgs = rows ? (double)ragged_span_total(rows, j.n_clips, j.n_channels / (f.pair_mode == 1 ? 2 : 1), f.KO)
                                : (double)((f.nf_t + f.KO - 1) / f.KO) * cols_;
        const double t_tile = std::ceil(wgs / 256.) * (double)f.KO * p.T * (vr ? 2.9e-4 : 6.3e-5) * (f.twin ? kTwinWg : f.pair_mode ? kPairWg : 1.);
        const double outs = rows ? (double)ragged_total_out(rows, j.n_clips) * j.n_channels : (double)nf * ((double)j.n_clips * j.n_channels);
        const double t_lane = (wave_ok ? kWaveUsPerTap : 2.5e-6) * outs * p.T;
        if (t_lane < t_tile) f.KO = 0;
    }
    return f;
}

template <typename IO, typename Real>
static const char *launch_interp_tile(const Plan &p, const GatherLaunch &c, const InterpArgs &ia, const InterpTileForm &f)
{
    const hipsoxr_job_t &j = c.j;
    InterpTileArgs ta;
    ta.ia = ia; ta.KO = (int32_t)f.KO; ta.span_cap = (int32_t)((f.span_cap + 1) / 2 * 2);
    ta.cols_per_clip = f.pair_mode == 1 ? j.n_channels / 2 : j.n_channels; ta.ch_step = f.pair_mode == 1 ? 2 : 1;
    ta.m2_in = ta.m2_out = ta.m2_l = ta.m2_k = 0; ta.m2_n = c.nf; ta.m2_dch = 0;
    if (f.pair_mode == 1) { ta.m2_in = j.in_chan_stride; ta.m2_out = j.out_chan_stride; ta.m2_dch = 1; }
    if (f.pair_mode == 2) {
        ta.m2_l = f.split_h * p.M; ta.m2_k = f.split_h * p.L; ta.m2_in = ta.m2_l * j.in_frame_stride; ta.m2_out = ta.m2_k * j.out_frame_stride;
        ta.m2_n = c.nf - f.nf_t; ta.ia.g.out_frames = f.nf_t;
    }
    const size_t lds = (size_t)(f.twin ? 2 * (ta.span_cap + 2) : ta.span_cap) * (f.pair_mode ? 2 : 1) * sizeof(Real) + (size_t)f.KO * 2 + (size_t)(2 * p.phases + 2) * 4 + 64;
    const dim3 tgrid((unsigned)((f.nf_t + f.KO - 1) / f.KO), (unsigned)((uint64_t)j.n_clips * ta.cols_per_clip), 1);
    void (*tk)(InterpTileArgs) = f.pair_mode ? (c.vr ? k_interp_tile<IO, Real, true, true> : k_interp_tile<IO, Real, false, true>)
                                             : (c.vr ? k_interp_tile<IO, Real, true, false> : k_interp_tile<IO, Real, false, false>);
    if constexpr (sizeof(Real) == 4)
        if (f.twin) tk = c.vr ? k_interp_tile<IO, Real, true, true, true> : k_interp_tile<IO, Real, false, true, true>;
    if (c.rows) { // the ragged form (pair modes 0 and 1): the frame axis is the longest clip's (f.nf_t == c.nf)
        InterpTileArgsR tr;
        (InterpTileArgs &)tr = ta;
        tr.rows = c.rows; tr.clock = c.clock;
        void (*rk)(InterpTileArgsR) = f.pair_mode ? (c.vr ? k_interp_tile<IO, Real, true, true, false, true> : k_interp_tile<IO, Real, false, true, false, true>)
                                                  : (c.vr ? k_interp_tile<IO, Real, true, false, false, true> : k_interp_tile<IO, Real, false, false, false, true>);
        if constexpr (sizeof(Real) == 4)
            if (f.twin) rk = c.vr ? k_interp_tile<IO, Real, true, true, true, true> : k_interp_tile<IO, Real, false, true, true, true>;
        if (const char *e = ensure_dyn_lds((const void *)rk, lds)) return e;
        const dim3 rgrid((unsigned)ragged_span_grid_x(f.nf_t, f.KO), tgrid.y, 1);
        GATHER_LAUNCH_LOG("interp_tile", p, c, rgrid, 1024, lds, "KO=%d pair=%d twin=%d h=%lld nf_t=%lld m2_n=%lld span_cap=%d", (int)ta.KO, f.pair_mode, f.twin ? 1 : 0,
                          (long long)f.split_h, (long long)f.nf_t, (long long)ta.m2_n, (int)ta.span_cap);
        hipLaunchKernelGGL(rk, rgrid, dim3(1024), lds, c.st, tr);
        HIP_TRY(hipGetLastError());
        return nullptr;
    }
    if (const char *e = ensure_dyn_lds((const void *)tk, lds)) return e;
    GATHER_LAUNCH_LOG("interp_tile", p, c, tgrid, 1024, lds, "KO=%d pair=%d twin=%d h=%lld nf_t=%lld m2_n=%lld span_cap=%d", (int)ta.KO, f.pair_mode, f.twin ? 1 : 0,
                      (long long)f.split_h, (long long)f.nf_t, (long long)ta.m2_n, (int)ta.span_cap);
    hipLaunchKernelGGL(tk, tgrid, dim3(1024), lds, c.st, ta);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// one lane per output: k_interp (ia: interpolated-phase plans and variable rate), else k_gather — every ratio, layout and length
template <typename IO, typename Real>
static const char *launch_lane(const Plan &p, const GatherLaunch &c, const InterpArgs *ia)
{
    const dim3 block(256), grid = c.a.ch_fast ? dim3((unsigned)((c.nf * (int64_t)c.j.n_channels + 255) / 256), c.j.n_clips, 1) : c.grid(256);
    if (c.rows) { // the ragged form of k_interp (k_gather's: launch_ragged_gather)
        if (!ia) return "ragged batches: no such lane kernel";
        const int64_t gx = ragged_gather_grid_x(c.nf, c.a.ch_fast ? c.j.n_channels : 1);
        if (gx > kTileMaxGridX) return kTileTooLong;
        InterpArgsR ir;
        (InterpArgs &)ir = *ia;
        ir.rows = c.rows; ir.clock = c.clock;
        const dim3 rgrid((unsigned)gx, grid.y, 1);
        GATHER_LAUNCH_LOG("interp", p, c, rgrid, 256, (size_t)0, "ch_fast=%d", (int)c.a.ch_fast);
        if (c.vr) hipLaunchKernelGGL((k_interp<IO, Real, true, true>), rgrid, block, 0, c.st, ir);
        else hipLaunchKernelGGL((k_interp<IO, Real, false, true>), rgrid, block, 0, c.st, ir);
        HIP_TRY(hipGetLastError());
        return nullptr;
    }
    GATHER_LAUNCH_LOG(ia ? "interp" : "gather", p, c, grid, 256, (size_t)0, "ch_fast=%d", (int)c.a.ch_fast);
    if (ia && c.vr) hipLaunchKernelGGL((k_interp<IO, Real, true>), grid, block, 0, c.st, *ia);
    else if (ia) hipLaunchKernelGGL((k_interp<IO, Real, false>), grid, block, 0, c.st, *ia);
    else hipLaunchKernelGGL((k_gather<IO, Real>), grid, block, 0, c.st, c.a);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// ---- launch: the dispatcher of everything but the period tiles.  Decision order, per launch of at most 2^30 outputs:
//   k_gather_wave -> k_chain (res: k_chain_resident) -> interpolated plans: k_interp_wave / k_interp_tile / k_interp -> k_gather
template <typename IO, typename Real>
static const char *launch_gather(Plan *p, const hipsoxr_job_t &j, hipStream_t st, const VrPos *vr = nullptr, ResidentLaunch *res = nullptr,
                                 ChainDone *cd = nullptr)
{
    if (cd) cd->n_wgs = 0;
    const DeviceBank &d = bank_of<Real>(p);
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    const bool cols_fit = cols <= 65535; // (every kernel but the lane-per-output ones on channel-fast data has the columns in grid.y)
    // split so that idx*M stays far below 2^63 and grid.x below 2^31
    const int64_t max_chunk = (int64_t)1 << 30;
    for (int64_t done = 0; done < j.out_frames; done += max_chunk) {
        const int64_t nf = std::min<int64_t>(max_chunk, j.out_frames - done);
        const GatherLaunch c{j, st, vr, cd, done, nf, cols, make_gather_args<IO>(*p, d, j, j.out_k0 + done, nf, done * j.out_frame_stride)};
        if (c.a.ch_fast && j.n_clips > 65535) return "too many clips for one launch (max 65535)";
        if (!c.a.ch_fast && !cols_fit) return "too many (clip, channel) columns for one launch (max 65535)";
        const char *err = nullptr;

        // exact-bank launches of 4096 outputs and more that come here (launch_typed: periods too few for a slab, or a
        // stream chunk whose result goes straight to host memory): k_gather_wave instead of lane-per-output k_gather
        if (!p->phases && !res && !vr && !switches().no_gather_wave && nf >= 4096 && p->T >= 32 && cols_fit) {
            const WaveGeom gw = wave_geom<Real>(31 * ((p->M + p->L - 1) / p->L + 1), p->T); // 31 window shifts of at most ceil(M/L) + T
            if (gw.ok) {
                if ((err = launch_gather_wave<IO, Real>(p, c, gw))) return err;
                continue;
            }
        }

        // interpolated plans: the launch's largest step, and whether k_interp_wave can take it (in place of lane-per-output
        // k_interp): it needs a (clip, channel) grid dimension and LDS for the span of 32 consecutive outputs at that step
        double step = 0;
        WaveGeom iw;
        if (p->phases) {
            step = vr ? vr_max_step(*vr, done + nf) : (double)p->M / (double)p->L; // input samples per output
            if (!switches().no_interp_wave && cols_fit && step < 1e6) iw = wave_geom<Real>((int64_t)std::ceil(31. * step), p->T);
        }

        // small launches (streaming chunks): the low-latency chain kernel (interpolated plans above 512 outputs: k_interp_wave —
        // 4410-frame variable-rate calls 29.0 -> 27.0 us; 441-frame calls are 2.5 us faster here: 20 short workgroups against 5)
        if (!switches().no_chain && nf < 4096 && cols_fit && !(iw.ok && !res && nf > 512)) {
            const ChainGeom cg = chain_geom<Real>(*p, nf);
            if (cg.ok) {
                if ((err = launch_chain<IO, Real>(p, c, cg, res))) return err;
                continue; // (the resident kernel is up: a launch this small is the job's only one)
            }
        }
        if (res) return "resident kernel: unavailable for this job";

        if (p->phases) {
            InterpArgs ia;
            std::memset(&ia, 0, sizeof ia);
            ia.g = c.a;
            set_interp_table(ia, *p, d);
            if (vr) {
                if ((1 << ia.lgP) != ia.P) return "variable-rate needs a power-of-two phase count";
                vr_advance(*vr, done, ia);
            }
            InterpTileForm tf; // large launches: k_interp_tile where its cost model beats the lane-per-output kernels
            if (!switches().no_interp_tile && nf >= 4096 && cols_fit) tf = interp_tile_form<Real>(*p, j, nf, step, vr != nullptr, iw.ok);
            if (!tf.KO && iw.ok) err = launch_interp_wave<IO, Real>(*p, c, ia, iw);
            else if (tf.KO) err = launch_interp_tile<IO, Real>(*p, c, ia, tf);
            else err = launch_lane<IO, Real>(*p, c, &ia);
        } else {
            err = launch_lane<IO, Real>(*p, c, nullptr);
        }
        if (err) return err;
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// The tile launch.  Every decision that reads nothing but numbers is a function of tile_rules.h (TileForm: the result of all
// of them for one launch); here: the switches the rules read (tile_switches), the plan's two geometries (tile_geoms), the
// job into TileArgs / TileArgsR (tile_args), the kernel instance (tile_kernel), the trace buffer, the launch-log line, and
// launch_tile, which puts them in order — as launch_ragged does further down for a clip table.
// ---------------------------------------------------------------------------------------------
static TileSwitches tile_switches()
{
    const Switches &w = switches();
    TileSwitches s;
    s.dbg_slab32 = w.dbg_slab32; s.dbg_slab64 = w.dbg_slab64; s.no_halves = w.no_halves; s.no_xcd_split = w.no_xcd_split;
    s.no_tile_split = w.no_tile_split; s.dbg_mfma64_split = w.dbg_mfma64_split; s.dbg_tile_form = w.dbg_tile_form;
    s.dbg_mfma64_pb = w.dbg_mfma64_pb; s.dbg_nrt = w.dbg_nrt; s.dbg_nw = w.dbg_nw; s.dbg_split = w.dbg_split; s.dbg_lds = w.dbg_lds;
    return s;
}

// a plan's VALU-tile and MFMA-tile geometries (the MFMA one: planes where the period admits them, else the general-period form)
struct TileGeoms { TileGeom gv, gm; };
static TileGeoms tile_geoms(const Plan *p, int prec)
{
    TileGeoms t;
    std::lock_guard<std::mutex> lk(g_geom_mu);
    if (TileGeom *gp = geom_find(p, prec, 0)) t.gv = *gp;
    if (TileGeom *gp = geom_find(p, prec, 1)) t.gm = *gp;
    return t;
}

static TileSelector tile_selector(int kernel)
{
    switch (kernel) {
    case HIPSOXR_KERNEL_AUTO: return kSelAuto;
    case HIPSOXR_KERNEL_GATHER: return kSelGather;
    case HIPSOXR_KERNEL_TILE: return kSelTile;
    case HIPSOXR_KERNEL_TILE_VALU: return kSelTileValu;
    case HIPSOXR_KERNEL_TILE_MFMA: return kSelTileMfma;
    default: return kSelOther;
    }
}

// The arguments of a launch of form f.  An equal-length job: its window and clip strides.  A ragged one (`ragged`): whole
// signals, a clip's place and frame counts its row's — zero clip strides, zero window fields; the caller adds TileArgsR::rows.
static void tile_args(TileArgs &a, const DeviceBank &d, const TileGeom &g, const TileForm &f, const hipsoxr_job_t &j, bool ragged)
{
    a.in = j.in; a.out = j.out;
    a.tab = g.variant >= 1 ? d.tile_tab_m : d.tile_tab;
    a.e0 = g.variant >= 1 ? d.tile_i0_m : d.tile_i0;
    a.Lc = g.Lc; a.Mc = g.Mc; a.n_rt = f.n_rt; a.I_h = g.I_h;
    a.pad = g.pad; a.i_min = g.i_min; a.x_count = f.slab.x_count; a.pb = f.slab.pb;
    a.n_clips = j.n_clips; a.n_channels = j.n_channels;
    a.ics = ragged ? 0 : j.in_clip_stride; a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride;
    a.ocs = ragged ? 0 : j.out_clip_stride; a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.in_abs0 = ragged ? 0 : j.in_abs0; a.in_frames = ragged ? 0 : j.in_frames;
    a.out_k0 = ragged ? 0 : j.out_k0; a.out_frames = ragged ? 0 : j.out_frames;
    a.b_first = ragged ? 0 : tile_first_period(j.out_k0, g.Lc);
    a.oc.clip_counter = j.clip_counter; a.oc.dither = j.dither; a.oc.seed = j.dither_seed; a.oc.ch0 = t_ch_base;
    a.n_waves = f.n_waves;
    a.dbg = ragged ? 0 : switches().dbg_flags;
    a.rowR = g.rowR; a.plane = f.slab.plane;
    a.halves = f.halves; a.scratch_off = f.scratch_off;
    a.xz = f.xz; a.nx = f.nx;
    a.trace = nullptr;
}

// the only place on the launch side that names a tile kernel instance (in the order of first use the object's kernels have
// had since launch_tile and launch_ragged named them: profiles/NOTES_launch_refactor.md §1)
template <typename IO, typename Real, bool RAGGED>
static void (*tile_kernel(const TileForm &f, bool aligned))(typename TileArgsOf<RAGGED>::type)
{
    const int pb = f.slab.pb;
    if constexpr (!RAGGED) {
        void (*kern)(TileArgs) = aligned ? k_tile<IO, Real, 16, true> : k_tile<IO, Real, 16, false>;
        if constexpr (sizeof(Real) == 4) {
            if (f.kind == kTileMfma) kern = pb == 64 ? k_tile_mfma<IO, float, 4> : pb == 32 ? k_tile_mfma<IO, float, 2> : k_tile_mfma<IO, float, 1>;
            if (f.kind == kTileMfmaP) kern = k_tile_mfma_p<IO>;
        } else {
            if (f.kind == kTileMfma) kern = pb == 32 ? k_tile_mfma<IO, double, 2> : k_tile_mfma<IO, double, 1>; // (pb = 64 is never chosen for float64: build_tile_tables)
            if (f.kind == kTileMfma64P) kern = pb == 16 ? k_tile_mfma64_p<IO, 1, 16> : f.ng == 1 ? k_tile_mfma64_p<IO, 1, 32> : k_tile_mfma64_p<IO, 2, 32>;
        }
        return kern;
    } else { // (the plan's own slabs: float32 64 periods, float64 32 or 16 — tile_form_ragged refuses any other)
        void (*kern)(TileArgsR) = nullptr;
        if constexpr (sizeof(Real) == 4) {
            if (f.kind == kTileMfmaP) kern = k_tile_mfma_p<IO, true>;
            if (f.kind == kTileMfma) kern = k_tile_mfma<IO, float, 4, true>;
        } else {
            if (f.kind == kTileMfma64P) kern = k_tile_mfma64_p<IO, 2, 32, true>;
            if (f.kind == kTileMfma) kern = pb == 32 ? k_tile_mfma<IO, double, 2, true> : k_tile_mfma<IO, double, 1, true>;
        }
        if (f.kind == kTile) kern = aligned ? k_tile<IO, Real, 16, true, true> : k_tile<IO, Real, 16, false, true>;
        return kern;
    }
}

// (HIPSOXR_DEBUG_TRACE, planar kernels: per-wave time stamps [workgroup][wave][16], dumped synchronously behind the launch —
//  a debugging aid)
static const char *tile_trace_begin(TileArgs &a, const TileForm &f, size_t *n)
{
    *n = (size_t)f.grid[0] * f.grid[1] * f.grid[2] * 4 * 16;
    if (!switches().dbg_trace || (f.kind != kTileMfmaP && f.kind != kTileMfma64P)) return nullptr;
    HIP_TRY(hipMalloc((void **)&a.trace, *n * 8));
    HIP_TRY(hipMemset(a.trace, 0, *n * 8));
    return nullptr;
}
static const char *tile_trace_dump(const TileArgs &a, size_t n, hipStream_t st)
{
    if (!a.trace) return nullptr;
    std::vector<unsigned long long> h(n);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(h.data(), a.trace, n * 8, hipMemcpyDeviceToHost));
    if (FILE *f = fopen(switches().dbg_trace, "wb")) { fwrite(h.data(), 8, n, f); fclose(f); }
    (void)hipFree(a.trace);
    return nullptr;
}

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): one line per tile launch — an equal-length job's, or (ragged_clips >= 0,
// `ragged=<clips>` at the end; g == nullptr: its k_gather form) a ragged launch's — in the style of adj_launch_log: what
// tests/test_gpu_tile_forms.py and tests/test_gpu_ragged_exact.py read the launch form from.
template <typename IO, typename Real>
static void tile_launch_log(const char *kernel, const Plan &p, const TileGeom *g, const TileForm &f, int64_t ragged_clips)
{
    FILE *fl = fopen(switches().dbg_launch_log, "a");
    if (!fl) return;
    fprintf(fl, "kernel=%s width=%zu io=%c%zu L=%lld M=%lld Lc=%lld Mc=%lld pb=%d n_rt=%d nw=%d split=%d halves=%d xz=%d lds=%zu grid=%ux%ux%u block=%u", kernel,
            sizeof(Real), std::is_integral<IO>::value ? 'i' : 'f', sizeof(IO) * 8, (long long)p.L, (long long)p.M, (long long)(g ? g->Lc : 0),
            (long long)(g ? g->Mc : 0), g ? (int)f.slab.pb : 0, g ? f.n_rt : 0, f.n_waves, f.split, f.halves, (int)f.xz, f.lds, f.grid[0], f.grid[1], f.grid[2], f.block);
    if (ragged_clips >= 0) fprintf(fl, " ragged=%lld", (long long)ragged_clips);
    fputc('\n', fl);
    fclose(fl);
}

template <typename IO, typename Real>
static const char *launch_tile(Plan *p, const hipsoxr_job_t &j, hipStream_t st, const TileGeom &g)
{
    const TileForm f = tile_form(sizeof(Real), g, j.out_k0, j.out_frames, (uint64_t)j.n_clips * j.n_channels, tile_switches());
    if (f.err) return f.err;
    TileArgs a;
    tile_args(a, bank_of<Real>(p), g, f, j, false);
    void (*kern)(TileArgs) = tile_kernel<IO, Real, false>(f, g.aligned);
    if (const char *e = ensure_dyn_lds((const void *)kern, f.lds)) return e;
    size_t trace_n = 0;
    if (const char *e = tile_trace_begin(a, f, &trace_n)) return e;
    hipLaunchKernelGGL(kern, dim3(f.grid[0], f.grid[1], f.grid[2]), dim3(f.block), f.lds, st, a);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) tile_launch_log<IO, Real>(tile_kind_name(f.kind), *p, &g, f, -1);
    return tile_trace_dump(a, trace_n, st);
}

template <typename IO, typename Real>
static const char *launch_wave_dot(Plan *p, const hipsoxr_job_t &j, hipStream_t st)
{
    const DeviceBank &d = bank_of<Real>(p);
    if (p->phases) return "wave-dot kernel needs an exact-bank plan";
    if (const char *e = ensure_phase_major<Real>(p)) return e;
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > 65535) return "too many (clip, channel) columns for one launch (max 65535)";
    if (j.out_frames > ((int64_t)1 << 30)) return "job too long for the wave-dot kernel";
    GatherArgs a = make_gather_args<IO>(*p, d, j, j.out_k0, j.out_frames, 0);
    a.bank = nullptr; a.Lpad = 0; a.ch_fast = 0; // (the phase-major bank travels beside the arguments; columns always in grid.y)
    const int32_t per_wave = 16;
    const int64_t waves = (j.out_frames + per_wave - 1) / per_wave;
    hipLaunchKernelGGL((k_wave_dot<IO, Real>), dim3((unsigned)((waves + 3) / 4), (unsigned)cols, 1), dim3(256), 0, st, a,
                       (const Real *)d.phase_major, per_wave);
    HIP_TRY(hipGetLastError());
    return nullptr;
}

static constexpr double kGatherWaveTaps = 16e6;
template <typename IO, typename Real>
static const char *launch_typed(Plan *p, const hipsoxr_job_t &j, hipStream_t st, const VrPos *vr, ResidentLaunch *res = nullptr,
                                ChainDone *cd = nullptr)
{
    if (res) return launch_gather<IO, Real>(p, j, st, vr, res);
    const TileGeoms t = tile_geoms(p, sizeof(Real) == 4 ? 0 : 1);
    int kernel = j.kernel;
    if (kernel == HIPSOXR_KERNEL_WAVE_DOT) return vr ? "wave-dot kernel does not do variable rate" : launch_wave_dot<IO, Real>(p, j, st);
    if (kernel == HIPSOXR_KERNEL_EXACT || kernel == HIPSOXR_KERNEL_FFT) kernel = HIPSOXR_KERNEL_AUTO;
    if (p->phases) { // interpolated-phase plan: one kernel (k_interp, dispatched by launch_gather)
        if (kernel != HIPSOXR_KERNEL_AUTO && kernel != HIPSOXR_KERNEL_GATHER) return kTileUnavailable;
        return launch_gather<IO, Real>(p, j, st, vr, nullptr, cd);
    }
    if (vr) return "variable-rate needs an interpolated-phase plan";
    const TileGeom &g = t.gm.ok ? t.gm : t.gv;
    bool big = tile_big(g.ok, g.Lc, j.out_frames);
    // ... except for a stream chunk whose result the kernel writes straight into pinned host memory (`cd`: engine.cpp's
    // direct path) while it is far too small to fill the chip with slabs.  As a kernel k_gather_wave is the slower one
    // even there (96 000 frames at 44.1k -> 16k: 17.5 against 15.6 us; back to back on device buffers 15.0 against 9.6),
    // but the CALL is shorter with it — its outputs leave as runs of 16 neighbouring samples, the tiles' as one sample
    // per lane of a row tile: 20 000-frame int16 calls 35 against 41 us, 48 000-frame 43.5 against 45.6, 96 000-frame
    // the same (interleaved A/B on one box, tools/gw_time.sh).  Up to kGatherWaveTaps output x tap products.
    if (big && cd && !switches().no_gather_wave && p->T >= 32 &&
        (double)j.out_frames * j.n_clips * j.n_channels * p->T < (switches().dbg_gw_taps ? switches().dbg_gw_taps * 1e6 : kGatherWaveTaps))
        big = false;
    switch (tile_family(tile_selector(kernel), t.gv.ok, t.gm.ok, big)) {
    case kFamRefused: return kTileUnavailable;
    case kFamTileMfma: return launch_tile<IO, Real>(p, j, st, t.gm);
    case kFamTileValu: return launch_tile<IO, Real>(p, j, st, t.gv);
    default: return launch_gather<IO, Real>(p, j, st, nullptr, nullptr, cd);
    }
}

// ---------------------------------------------------------------------------------------------
// Ragged batches on the exact engine: all clips of a clip table (or of one range of it) in ONE launch of a kernel's RAGGED
// form.  ONE form is picked from the table for the whole launch — any is correct, every exact kernel computes the canonical
// order — with the plan's own slab geometry: AUTO / EXACT take the MFMA tile family where the plan has one, else k_tile,
// when the LONGEST clip passes launch_typed's `big` test (short clips ride along), otherwise k_gather; the family
// selectors force theirs.  Not in ragged form: the small-job forms of launch_tile (halves, z-splits, 16-period float64
// slabs) and the trace.  Interpolated-phase plans: launch_ragged_interp below.  *handled stays false for what is not this
// path's (float clips of an interpolated-phase plan under AUTO: the two-stage form's — twostage.hip launch_two_stage_ragged,
// which hands its short clips back through launch_ragged_short — or, interleaved, the clip-by-clip loop's; the wave-dot
// kernel; a table with a clip of more than 2^30 outputs: launch_ragged_job).
// ---------------------------------------------------------------------------------------------
// k_gather's ragged form: one lane per output of the longest clip
template <typename IO, typename Real>
static const char *launch_ragged_gather(Plan *p, const hipsoxr_job_t &j, hipStream_t st, int64_t longest, uint64_t cols)
{
    hipsoxr_job_t jj = j;
    jj.in_clip_stride = jj.out_clip_stride = 0; // (a clip's place is its row's)
    GatherArgsR a;
    (GatherArgs &)a = make_gather_args<IO>(*p, bank_of<Real>(p), jj, 0, longest, 0);
    a.rows = j.clip_table_dev;
    const int64_t gx = ragged_gather_grid_x(longest, a.ch_fast ? j.n_channels : 1);
    if (gx > kTileMaxGridX) return kTileTooLong;
    TileForm f;
    f.grid[0] = (unsigned)gx; f.grid[1] = a.ch_fast ? j.n_clips : (unsigned)cols;
    f.block = 256; f.split = 0; // (the log line's fields: no slab, no split)
    hipLaunchKernelGGL((k_gather<IO, Real, true>), dim3(f.grid[0], f.grid[1], 1), dim3(f.block), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) tile_launch_log<IO, Real>("gather", *p, nullptr, f, j.n_clips);
    return nullptr;
}

// Interpolated-phase plans: ONE form for the whole table, in launch_gather's order — k_interp_tile where its cost model, fed
// the table's real numbers, beats the lane-per-output kernels, else k_interp_wave, else k_interp.  (k_chain has no ragged
// form: the wave kernel serves even a single output.)  The debug switches act as on launch_gather.
template <typename IO, typename Real>
static const char *launch_ragged_interp(Plan *p, const hipsoxr_job_t &j, hipStream_t st)
{
    const int64_t longest = ragged_longest(j.clip_table, j.n_clips);
    if (longest == 0) return nullptr; // nothing to write
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > kMaxGridY) return kTileTooManyCols;
    hipsoxr_job_t jj = j;
    jj.in_clip_stride = jj.out_clip_stride = 0; // (a clip's place is its row's)
    GatherLaunch c{jj, st, nullptr, nullptr, 0, longest, cols, make_gather_args<IO>(*p, bank_of<Real>(p), jj, 0, longest, 0)};
    c.rows = j.clip_table_dev; c.ragged = j.n_clips;
    InterpArgs ia;
    std::memset(&ia, 0, sizeof ia);
    ia.g = c.a;
    set_interp_table(ia, *p, bank_of<Real>(p));
    const double step = (double)p->M / (double)p->L; // input samples per output
    WaveGeom iw;
    if (!switches().no_interp_wave && step < 1e6) iw = wave_geom<Real>((int64_t)std::ceil(31. * step), p->T);
    InterpTileForm tf; // (launch_gather's threshold, here on the table's outputs per channel)
    if (!switches().no_interp_tile && ragged_tile_considered(j.clip_table, j.n_clips))
        tf = interp_tile_form<Real>(*p, jj, longest, step, false, iw.ok, j.clip_table);
    if (tf.KO) return launch_interp_tile<IO, Real>(*p, c, ia, tf);
    if (iw.ok) return launch_interp_wave<IO, Real>(*p, c, ia, iw);
    return launch_lane<IO, Real>(*p, c, &ia);
}

// j: the job of one launch — clip_table the host rows of its n_clips clips, clip_table_dev their device copy
template <typename IO, typename Real>
static const char *launch_ragged(Plan *p, const hipsoxr_job_t &j, hipStream_t st, bool *handled)
{
    *handled = false;
    if (j.kernel == HIPSOXR_KERNEL_WAVE_DOT) return nullptr;
    if (p->phases) { // the selectors launch_typed admits for such a plan
        if (j.kernel != HIPSOXR_KERNEL_AUTO && j.kernel != HIPSOXR_KERNEL_EXACT && j.kernel != HIPSOXR_KERNEL_GATHER) return kTileUnavailable;
        *handled = true;
        return launch_ragged_interp<IO, Real>(p, j, st);
    }
    const TileGeoms t = tile_geoms(p, sizeof(Real) == 4 ? 0 : 1);
    const int64_t longest = ragged_longest(j.clip_table, j.n_clips);
    const TileGeom &g0 = t.gm.ok ? t.gm : t.gv;
    const TileFamily fam = tile_family(tile_selector(j.kernel == HIPSOXR_KERNEL_EXACT ? HIPSOXR_KERNEL_AUTO : j.kernel), t.gv.ok, t.gm.ok,
                                       tile_big(g0.ok, g0.Lc, longest));
    if (fam == kFamRefused) return kTileUnavailable;
    if (fam == kFamOther) return nullptr;
    *handled = true;
    if (longest == 0) return nullptr; // nothing to write
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > kMaxGridY) return kTileTooManyCols;
    if (fam == kFamGather) return launch_ragged_gather<IO, Real>(p, j, st, longest, cols);

    const TileGeom &g = fam == kFamTileMfma ? t.gm : t.gv;
    const TileForm f = tile_form_ragged(sizeof(Real), g, cols, tile_switches(), [&](int32_t pb) { return ragged_grid_x(longest, g.Lc, pb); },
                                        [&](int32_t pb) { return ragged_total_slabs(j.clip_table, j.n_clips, j.n_channels, g.Lc, pb); });
    if (f.err) return f.err;
    TileArgsR a;
    tile_args(a, bank_of<Real>(p), g, f, j, true);
    a.rows = j.clip_table_dev;
    void (*kern)(TileArgsR) = tile_kernel<IO, Real, true>(f, g.aligned);
    if (const char *e = ensure_dyn_lds((const void *)kern, f.lds)) return e;
    hipLaunchKernelGGL(kern, dim3(f.grid[0], f.grid[1], f.grid[2]), dim3(f.block), f.lds, st, a);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) tile_launch_log<IO, Real>(tile_kind_name(f.kind), *p, &g, f, j.n_clips);
    return nullptr;
}

// The device copy of a ragged job's clip table: the caller's (clip_table_dev, trusted to equal the host table), or — NULL —
// the host table, already validated, uploaded here in stream order (stream-ordered allocation: the buffer lives until the
// launches behind it have run).  *tmp: what the caller frees with hipFreeAsync behind its launches.  texts: the caller's
// words for the two failures.
const char *clip_table_device(const hipsoxr_job_t &j, void *stream, const int64_t **rows, void **tmp, const ClipTableTexts &texts)
{
    hipStream_t st = (hipStream_t)stream;
    *tmp = nullptr;
    *rows = j.clip_table_dev;
    if (*rows) return nullptr;
    const size_t bytes = (size_t)j.n_clips * kRaggedRow * sizeof(int64_t);
    if (hipMallocAsync(tmp, bytes, st) != hipSuccess) { *tmp = nullptr; return texts.no_memory; }
    if (hipMemcpyAsync(*tmp, j.clip_table, bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        (void)hipFreeAsync(*tmp, st);
        *tmp = nullptr;
        return texts.upload_failed;
    }
    *rows = (const int64_t *)*tmp;
    return nullptr;
}

// The element type of a job as the kernels' template arguments: f(IO{}, Real{}) with the sample type and the engine's
// arithmetic type (float for float32 / int16 samples, double for float64 / int32).  invalid: what any other type is answered.
template <typename F>
static const char *with_elem(int elem, F f, const char *invalid = "invalid element type")
{
    switch (elem) {
    case HIPSOXR_F32: return f(float{}, float{});
    case HIPSOXR_F64: return f(double{}, double{});
    case HIPSOXR_I32: return f(int32_t{}, double{});
    case HIPSOXR_I16: return f(int16_t{}, float{});
    }
    return invalid;
}
// ... and selector and element type as the dispatcher's rules see them (job_rules.h)
static JobSel job_sel(int kernel)
{
    JobSel s;
    s.want_fft = kernel == HIPSOXR_KERNEL_FFT || kernel == HIPSOXR_KERNEL_FFT_F64;
    s.want_pcm = kernel == HIPSOXR_KERNEL_FFT_PCM;
    s.is_auto = kernel == HIPSOXR_KERNEL_AUTO;
    s.exact_family = kernel == HIPSOXR_KERNEL_EXACT || kernel == HIPSOXR_KERNEL_GATHER;
    s.fft_f64 = kernel == HIPSOXR_KERNEL_FFT_F64;
    s.wave_dot = kernel == HIPSOXR_KERNEL_WAVE_DOT;
    return s;
}
static JobElem job_elem(int elem)
{
    if (elem == HIPSOXR_F32 || elem == HIPSOXR_F64) return kJobElemFloat;
    if (elem == HIPSOXR_I16 || elem == HIPSOXR_I32) return kJobElemPcm;
    return elem_is_half(elem) ? kJobElemHalf : kJobElemOther;
}

// The ragged exact launch of a whole table: one launch, or — more columns than gridDim.y holds — one per range of clips
// (a sub-range of the table is a pointer offset, in the host table and in its device copy).
static const char *launch_ragged_job(Plan *p, const hipsoxr_job_t &j, hipStream_t st, bool *handled, bool two_stage_short = false)
{
    *handled = false;
    if (j.kernel == HIPSOXR_KERNEL_WAVE_DOT || ragged_fold_step(j.n_channels) == 0) return nullptr;
    // a table the two-stage form owns (job_rules.h) — all but the sub-table of clips that form does not admit
    // (two_stage_short: launch_two_stage_ragged's), which are the exact engine's
    if (job_two_stage_table(p->phases, job_sel(j.kernel), job_elem(j.elem), switches().no_fft, switches().no_two_stage) && !two_stage_short) return nullptr;
    if (ragged_longest(j.clip_table, j.n_clips) > ((int64_t)1 << 30)) return nullptr; // (launch_gather cuts such a clip into several launches)
    if (const char *e = device_bank_ensure(p, engine_prec(j.elem))) return e;
    const int64_t *rows = nullptr;
    void *tmp = nullptr;
    if (const char *e = clip_table_device(j, st, &rows, &tmp)) return e;
    const char *err = nullptr;
    bool all = true;
    for (uint32_t r = 0;; ++r) {
        const RaggedRange rg = ragged_fold_range(j.n_clips, j.n_channels, r);
        if (!rg.count) break;
        hipsoxr_job_t part = j;
        part.n_clips = rg.count;
        part.clip_table = j.clip_table + kRaggedRow * (size_t)rg.first;
        part.clip_table_dev = rows + kRaggedRow * (size_t)rg.first;
        bool h = false;
        err = with_elem(j.elem, [&](auto io, auto real) { return launch_ragged<decltype(io), decltype(real)>(p, part, st, &h); });
        if (err) break;
        if (!h) { all = false; break; } // (decided by plan and selector: the same for every range)
    }
    if (tmp) (void)hipFreeAsync(tmp, st);
    if (err) return err;
    *handled = all;
    return nullptr;
}
const char *launch_ragged_short(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    return launch_ragged_job(p, j, (hipStream_t)stream, handled, true);
}

// ---------------------------------------------------------------------------------------------
// Ragged variable-rate batches (hipsoxr_run_device_vr_ragged): clip c of a clip table at its own constant step, ONE launch of
// the VR && RAGGED form of k_interp_tile, k_interp_wave or k_interp.  The decisions and their order are
// launch_ragged_interp's, with vr = true and the LARGEST step of the clock table (vr_ragged_rules.h) where that one has the
// plan's M / L: it sizes the span of 32 outputs, KO and span_cap for every clip (a slower clip's spans are shorter).
// clock / clock_dev: host and device copy of the launch's [n_clips][2] steps.
// ---------------------------------------------------------------------------------------------
template <typename IO, typename Real>
static const char *launch_ragged_vr(Plan *p, const hipsoxr_job_t &j, hipStream_t st, const uint64_t *clock, const uint64_t *clock_dev)
{
    const int64_t longest = ragged_longest(j.clip_table, j.n_clips);
    if (longest == 0) return nullptr; // nothing to write
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > kMaxGridY) return kTileTooManyCols;
    hipsoxr_job_t jj = j;
    jj.in_clip_stride = jj.out_clip_stride = 0; // (a clip's place is its row's)
    static const VrPos per_clip = {0, 0, 0, 0, 0, 0}; // (GatherLaunch::vr says "variable rate": the clocks are the table's)
    GatherLaunch c{jj, st, &per_clip, nullptr, 0, longest, cols, make_gather_args<IO>(*p, bank_of<Real>(p), jj, 0, longest, 0)};
    c.rows = j.clip_table_dev; c.ragged = j.n_clips; c.clock = clock_dev;
    InterpArgs ia;
    std::memset(&ia, 0, sizeof ia);
    ia.g = c.a;
    set_interp_table(ia, *p, bank_of<Real>(p));
    if ((1 << ia.lgP) != ia.P) return "variable-rate needs a power-of-two phase count";
    const double step = vr_ragged_max_step(clock, j.n_clips); // input samples per output, at most
    WaveGeom iw;
    if (!switches().no_interp_wave && step < 1e6) iw = wave_geom<Real>((int64_t)std::ceil(31. * step), p->T);
    InterpTileForm tf;
    if (!switches().no_interp_tile && ragged_tile_considered(j.clip_table, j.n_clips))
        tf = interp_tile_form<Real>(*p, jj, longest, step, true, iw.ok, j.clip_table);
    if (tf.KO) return launch_interp_tile<IO, Real>(*p, c, ia, tf);
    if (iw.ok) return launch_interp_wave<IO, Real>(*p, c, ia, iw);
    return launch_lane<IO, Real>(*p, c, &ia);
}

// The whole table (validated by the entry; clock: its n_clips steps, host memory): the clip table as on ragged jobs
// (clip_table_dev honoured), the clock table uploaded here in stream order and released behind the launches; one launch, or —
// more columns than gridDim.y holds — one per range of clips, a range offsetting both tables.
const char *launch_vr_ragged(Plan *p, const hipsoxr_job_t &j, const uint64_t *clock, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (ragged_fold_step(j.n_channels) == 0) return "variable-rate ragged batch: more than 65535 channels are not served";
    if (const char *e = device_bank_ensure(p, engine_prec(j.elem))) return e;
    const int64_t *rows = nullptr;
    void *tmp = nullptr, *clk = nullptr;
    if (const char *e = clip_table_device(j, st, &rows, &tmp)) return e;
    const size_t bytes = (size_t)j.n_clips * kVrClockRow * sizeof(uint64_t);
    const char *err = nullptr;
    if (hipMallocAsync(&clk, bytes, st) != hipSuccess) { clk = nullptr; err = "variable-rate ragged batch: no device memory for the clock table"; }
    else if (hipMemcpyAsync(clk, clock, bytes, hipMemcpyHostToDevice, st) != hipSuccess) err = "variable-rate ragged batch: clock table upload failed";
    for (uint32_t r = 0; !err; ++r) {
        const RaggedRange rg = ragged_fold_range(j.n_clips, j.n_channels, r);
        if (!rg.count) break;
        hipsoxr_job_t part = j;
        part.n_clips = rg.count;
        part.clip_table = j.clip_table + kRaggedRow * (size_t)rg.first;
        part.clip_table_dev = rows + kRaggedRow * (size_t)rg.first;
        const uint64_t *ck = clock + kVrClockRow * (size_t)rg.first, *ck_dev = (const uint64_t *)clk + kVrClockRow * (size_t)rg.first;
        err = with_elem(j.elem, [&](auto io, auto real) { return launch_ragged_vr<decltype(io), decltype(real)>(p, part, st, ck, ck_dev); });
    }
    if (clk) (void)hipFreeAsync(clk, st);
    if (tmp) (void)hipFreeAsync(tmp, st);
    return err;
}

bool resident_post(const Plan &p, volatile uint64_t *w, uint32_t seq, int64_t in_abs0, int64_t in_frames, int64_t out_k0, int64_t out_frames,
                   const VrPos *vr)
{
    const ResidentMsg m = resident_msg(p, in_abs0, in_frames, out_k0, out_frames, vr != nullptr); // (stream_rules.h: what the words can carry)
    if (!m.fits) return false;
    const int64_t d0 = m.d0, p0 = m.p0;
    const uint64_t tag = (uint64_t)(seq & 0xffffu) << 48;
    // the words validate themselves (k_chain_resident): no order is needed among them — they may sit in
    // write-combining device memory — only everything the message refers to must have left before them
    __builtin_ia32_sfence();
    w[0] = tag | (uint64_t)in_abs0;
    w[1] = tag | (uint64_t)out_k0;
    w[2] = tag | (uint64_t)d0;
    w[3] = tag | ((uint64_t)in_frames << 24) | (uint64_t)p0;
    w[4] = tag | (uint64_t)out_frames;
    if (vr) { // the variable-rate clock of this message: position, step, step increment (Q64.64), 48 + 48 + 32 bits each
        auto put = [&](int i, uint64_t hi, uint64_t lo) {
            w[i] = tag | (lo & kResidentMask48);
            w[i + 1] = tag | ((lo >> 48) | ((hi & 0xffffffffULL) << 16));
            w[i + 2] = tag | (hi >> 32);
        };
        put(5, vr->t_hi, vr->t_lo); put(8, vr->s_hi, vr->s_lo); put(11, vr->d_hi, vr->d_lo);
    }
    __builtin_ia32_sfence();
    return true;
}
void resident_leave(volatile uint64_t *w, uint32_t epoch)
{
    w[15] = (uint64_t)epoch;
    __builtin_ia32_sfence();
}

// a chunk appended to a stream's device ring (engine.cpp device_process): 16 bytes per thread where both ends allow it
__global__ void __launch_bounds__(256) k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t n16)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_copy2(uint16_t *__restrict__ dst, const uint16_t *__restrict__ src, size_t n2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) dst[i] = src[i];
}
const char *launch_copy(void *dst, const void *src, size_t bytes, void *stream)
{
    if (!bytes) return nullptr;
    hipStream_t st = (hipStream_t)stream;
    if ((((uintptr_t)dst | (uintptr_t)src | bytes) & 15) == 0) {
        const size_t n = bytes / 16;
        hipLaunchKernelGGL(k_copy16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint4 *)dst, (const uint4 *)src, n);
    } else if ((((uintptr_t)dst | (uintptr_t)src | bytes) & 1) == 0) { // (frames are at least two bytes)
        const size_t n = bytes / 2;
        hipLaunchKernelGGL(k_copy2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint16_t *)dst, (const uint16_t *)src, n);
    } else {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return nullptr;
    }
    HIP_TRY(hipGetLastError());
    return nullptr;
}

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): the line of a k_chain_multi launch, in the style of gather_launch_log
// (there is no GatherLaunch here: the items are the streams' own) — what tests/test_gpu_gather_forms.py reads.  moving: items
// whose ring moves in this launch (ring_dst != ring); empty: items without an output due, which still append their chunk.
#ifdef HIPSOXR_DEBUG_SWITCHES
template <typename IO, typename Real>
static void chain_multi_launch_log(const Plan &p, const ChainItem *items, uint32_t n_items, uint32_t nch, int64_t max_out, dim3 grid, unsigned block,
                                   const ChainGeom &g)
{
    FILE *fl = fopen(switches().dbg_launch_log, "a");
    if (!fl) return;
    unsigned moving = 0, empty = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        if (items[i].ring_dst != items[i].ring) ++moving;
        if (items[i].out_frames == 0) ++empty;
    }
    fprintf(fl, "kernel=chain_multi width=%zu io=%c%zu L=%lld M=%lld T=%d P=%d items=%u nch=%u max_out=%lld grid=%ux%ux%u block=%u lds=%zu NO=%d span_cap=%d mode=%d moving=%u empty=%u\n",
            sizeof(Real), std::is_integral<IO>::value ? 'i' : 'f', sizeof(IO) * 8, (long long)p.L, (long long)p.M, (int)p.T, (int)p.phases, n_items, nch,
            (long long)max_out, grid.x, grid.y, grid.z, block, g.lds, g.NO, (int)g.span_cap, p.phases ? 1 : 0, moving, empty);
    fclose(fl);
}
#define CHAIN_MULTI_LAUNCH_LOG(...) do { if (switches().dbg_launch_log) chain_multi_launch_log<IO, Real>(__VA_ARGS__); } while (0)
#else
#define CHAIN_MULTI_LAUNCH_LOG(...) ((void)0)
#endif

template <typename IO, typename Real>
static const char *launch_chain_items_typed(Plan *p, uint32_t nch, bool dither, const ChainItem *items, const ChainItem *items_dev, uint32_t n_items,
                                            hipStream_t st, bool *handled)
{
    int64_t max_out = 0;
    for (uint32_t i = 0; i < n_items; ++i) max_out = std::max(max_out, items[i].out_frames);
    if (max_out >= 4096 || (uint64_t)n_items * nch > kJobMaxCols || switches().no_chain) return nullptr;
    const DeviceBank &d = bank_of<Real>(p);
    const ChainGeom g = chain_geom<Real>(*p, max_out);
    if (!g.ok) return nullptr;
    ChainMultiArgs m;
    std::memset(&m, 0, sizeof m);
    // a stream's own layout: interleaved frames; pointers, positions and seeds are the items'
    hipsoxr_job_t lay{};
    lay.n_clips = 1; lay.n_channels = nch; lay.dither = dither ? 1u : 0u;
    lay.in_frame_stride = lay.out_frame_stride = nch; lay.in_chan_stride = lay.out_chan_stride = 1;
    GatherArgs &a = m.ca.ia.g;
    a = make_gather_args<IO>(*p, d, lay, 0, 0, 0);
    a.oc.ch0 = 0; a.ch_fast = 0;
    m.ca.NO = g.NO; m.ca.span_cap = g.span_cap;
    m.n_channels = nch;
    void (*ck)(ChainMultiArgs) = nullptr;
    if (p->phases) {
        set_interp_table(m.ca.ia, *p, d);
        ck = k_chain_multi<IO, Real, 1>;
    } else {
        if (const char *e = ensure_phase_major<Real>(p)) return e;
        m.ca.phase_major = d.phase_major;
        ck = k_chain_multi<IO, Real, 0>;
    }
    if (n_items == 1) m.one = items[0];
    else if (!items_dev) return "internal: a many-streams launch needs a device-readable item table";
    else m.items = items_dev;
    if (const char *e = ensure_dyn_lds((const void *)ck, g.lds)) return e;
    const unsigned gx = (unsigned)std::max<int64_t>(1, (max_out + g.NO - 1) / g.NO);
    CHAIN_MULTI_LAUNCH_LOG(*p, items, n_items, nch, max_out, dim3(gx, (unsigned)(n_items * nch), 1), 256, g);
    hipLaunchKernelGGL(ck, dim3(gx, (unsigned)(n_items * nch), 1), dim3(256), g.lds, st, m);
    HIP_TRY(hipGetLastError());
    *handled = true;
    return nullptr;
}

const char *launch_chain_items(Plan *p, int elem, uint32_t n_channels, bool dither, const ChainItem *items, const ChainItem *items_dev,
                               uint32_t n_items, void *stream, bool *handled)
{
    *handled = false;
    if (!n_items || !n_channels) return nullptr;
    if (const char *e = device_bank_ensure(p, engine_prec(elem))) return e;
    hipStream_t st = (hipStream_t)stream;
    return with_elem(elem, [&](auto io, auto real) { // (dither: int16 samples alone)
        using IO = decltype(io);
        return launch_chain_items_typed<IO, decltype(real)>(p, n_channels, dither && std::is_same<IO, int16_t>::value, items, items_dev, n_items, st, handled);
    }, "unknown element type");
}

// ---------------------------------------------------------------------------------------------
// The dispatcher of device jobs: launch_job and one function per decision.  What is refused, which engine is offered a job
// and in which order, what a clip row must satisfy and how wide jobs fold are job_rules.h's; here are the calls.
// ---------------------------------------------------------------------------------------------
static const char *job_entry_refusal(const Plan &p, const hipsoxr_job_t &j, bool vr_or_res, bool res)
{
    const JobSel s = job_sel(j.kernel);
    const JobElem el = job_elem(j.elem);
    if (const char *e = job_resident_refusal(res, (uint64_t)j.n_clips * j.n_channels)) return e;
    if (const char *e = job_pcm_refusal(s, el, vr_or_res)) return e;
    if (s.want_pcm && !fft_job_eligible(p, j)) return kJobPcmIneligible;
    if (const char *e = job_half_refusal(s, el, vr_or_res)) return e;
    return job_table_refusal(j.clip_table != nullptr, vr_or_res, j.in_abs0, j.out_k0);
}

// every row of a clip table against the job and the plan; *total_out: the outputs of one channel, over all clips
static const char *job_table_rows(const Plan &p, const hipsoxr_job_t &j, int64_t *total_out)
{
    *total_out = 0;
    for (uint32_t c = 0; c < j.n_clips; ++c) {
        const int64_t *r = j.clip_table + kRaggedRow * (size_t)c;
        if (job_row_check(r, j.in_frames, j.out_frames, kJobRowForward, [&](uint64_t n) { return plan_out_len(p, n); }) != kJobRowOk)
            return "ragged batches: a clip's offsets or frame counts are negative, exceed the job's, or exceed the plan's output length";
        *total_out += r[3];
    }
    return nullptr;
}

// a table on the frequency-domain engine: one launch, the kernel reading its clip's row from the device copy of the table
static const char *launch_table_fft(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    if (const char *e = device_bank_ensure(p, engine_prec(j.elem))) return e;
    hipsoxr_job_t jj = j;
    void *tmp = nullptr;
    if (const char *e = clip_table_device(j, stream, &jj.clip_table_dev, &tmp)) return e;
    const char *e = launch_fft(p, jj, stream, handled, t_ch_base);
    if (tmp) (void)hipFreeAsync(tmp, (hipStream_t)stream);
    return e;
}

// a table clip by clip through the ordinary path, each non-empty clip re-entering as a plain job (float16 / bfloat16 clips:
// as a plain half job — the elements between packed clips are never written)
static const char *launch_table_clips(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    const size_t es = elem_size(j.elem);
    for (uint32_t c = 0; c < j.n_clips; ++c) {
        const int64_t *r = j.clip_table + kRaggedRow * (size_t)c;
        if (r[3] == 0) continue;
        hipsoxr_job_t one = j;
        one.clip_table = one.clip_table_dev = nullptr;
        one.n_clips = 1;
        one.in = (const char *)j.in + r[0] * (int64_t)es;
        one.out = (char *)j.out + r[2] * (int64_t)es;
        one.in_frames = r[1]; one.out_frames = r[3];
        if (const char *e = launch_job(p, one, stream)) return e;
    }
    return nullptr;
}

// Ragged batch (hipsoxr_job_t::clip_table): one launch of the frequency-domain engine when it can take the job
// (unit-stride columns under AUTO or by name, interleaved and strided ones by name), else — float clips of an
// interpolated-phase plan under AUTO, at any frame stride — the two-stage form over the table (one ragged polyphase launch
// and one ragged FFT-stage launch per range of columns, one ragged launch of the exact engine for the clips too short for
// the form: twostage.hip launch_two_stage_ragged), else one launch of the exact engine's ragged form (exact-bank and
// interpolated-phase plans alike), else — the wave-dot kernel, float clips the two-stage form handed back, half clips no
// fused launch took — clip by clip.  Clips are independent and each keeps the engine it has alone: bit-exact engines stay bit-exact.
static const char *launch_job_table(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    int64_t total_out = 0;
    if (const char *e = job_table_rows(*p, j, &total_out)) return e;
    const JobSel s = job_sel(j.kernel);
    const Switches &sw = switches();
    bool handled = false;
    if (job_try_fft(s, total_out * (int64_t)j.n_channels, sw.no_fft) && (uint64_t)j.n_clips * j.n_channels <= kJobMaxCols && fft_job_eligible(*p, j)) {
        if (const char *e = launch_table_fft(p, j, stream, &handled)) return e;
        if (handled) return nullptr;
    }
    if (s.want_fft) return "FFT engine unavailable for this ragged job (served: unit-stride, interleaved and strided float32 / float64 columns of a tabled ratio; not HIPSOXR_KERNEL_FFT_F64 on strided float32 data, not ratios outside the schedule table)";
    if (s.want_pcm) return "FFT engine (integer samples) unavailable for this ragged job (served: unit-stride int16 / int32 columns and interleaved int16 channel pairs at even offsets, of a tabled ratio; not int32 channel pairs, not int16 with an odd channel count, not ratios outside the schedule table)";
    if (job_two_stage_table(p->phases, s, job_elem(j.elem), sw.no_fft, sw.no_two_stage)) {
        if (const char *e = launch_two_stage_ragged(p, j, stream, &handled)) return e;
        if (handled) return nullptr;
    }
    if (!elem_is_half(j.elem)) {
        if (const char *e = launch_ragged_job(p, j, (hipStream_t)stream, &handled)) return e;
        if (handled) return nullptr;
    }
    return launch_table_clips(p, j, stream);
}

// float16 / bfloat16 samples: device jobs in float32 arithmetic — fused into the frequency-domain engine's paired kernels
// where the float32 job of the shape runs them (half_rules.h: the engine by name, or AUTO under the float rule, on a
// whole-signal job of an HQ / VHQ exact-ratio plan — launch_fft then takes it on the row the float32 job takes, or leaves
// it: no fused form for the layout or the ratio), else a widening pass, the float32 job and a narrowing pass (half.hip)
static const char *launch_job_half(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    const HalfSelector sel = j.kernel == HIPSOXR_KERNEL_FFT ? kHalfSelFft : j.kernel == HIPSOXR_KERNEL_AUTO ? kHalfSelAuto : kHalfSelOther;
    const int64_t total_out = (int64_t)j.out_frames * j.n_clips * j.n_channels;
    if (half_try_fused(sel, total_out, switches().no_fft, fft_job_eligible(*p, j), (uint64_t)j.n_clips * j.n_channels)) {
        if (const char *e = device_bank_ensure(p, 0)) return e;
        bool handled = false;
        if (const char *e = launch_fft(p, j, stream, &handled)) return e;
        if (handled) return nullptr;
    }
    return launch_half(p, j, stream, false); // (the float32 job inside refuses what a float32 job is refused)
}

// more columns than one launch holds: range by range (job_fold), each re-entering; the dither of a channel stays keyed by
// its index in the whole signal (t_ch_base)
static const char *launch_job_folded(Plan *p, const hipsoxr_job_t &j, void *stream, const VrPos *vr)
{
    const int64_t es = (int64_t)elem_size(j.elem);
    const JobFold fold = job_fold(j.n_clips, j.n_channels);
    const uint32_t saved = t_ch_base;
    const char *e = nullptr;
    for (uint64_t r = 0; !e; ++r) {
        const JobRange g = job_fold_range(fold, r);
        if (!g.n_clips) break;
        hipsoxr_job_t part = j;
        part.n_clips = g.n_clips; part.n_channels = g.n_ch;
        part.in = (const char *)j.in + ((int64_t)g.clip0 * j.in_clip_stride + (int64_t)g.ch0 * j.in_chan_stride) * es;
        part.out = (char *)j.out + ((int64_t)g.clip0 * j.out_clip_stride + (int64_t)g.ch0 * j.out_chan_stride) * es;
        t_ch_base = saved + g.ch0;
        e = launch_job(p, part, stream, vr);
    }
    t_ch_base = saved;
    return e;
}

// The 1e-6-class engines in front of the exact one, in job_rules.h's order: the two-stage form, the frequency-domain engine
// (HIPSOXR_KERNEL_FFT_F64: with float64 arithmetic whatever the I/O type), that engine on integer samples by name.
// *handled = false and no text: the exact engine's job.
static const char *launch_job_engines(Plan *p, const hipsoxr_job_t &j, void *stream, bool vr_or_res, bool *handled)
{
    const JobSel s = job_sel(j.kernel);
    const Switches &sw = switches();
    if (const char *e = job_fft_stream_refusal(s, vr_or_res)) return e;
    if (!vr_or_res && job_two_stage(p->phases, s, job_elem(j.elem), sw.no_fft, sw.no_two_stage)) {
        if (const char *e = launch_two_stage(p, j, stream, handled)) return e;
        if (*handled) return nullptr;
        if (s.want_fft) return "FFT engine unavailable for this plan (the two-stage form serves HQ / VHQ ratios down to 4:1, whole signals of >= ~5000 frames)";
    }
    if (!vr_or_res && (s.want_fft || s.is_auto)) {
        const bool eligible = fft_job_eligible(*p, j);
        if (s.want_fft && !eligible)
            return "FFT engine needs a whole-signal float32 or float64 job (in_abs0 == 0, out_k0 == 0) on an HQ/VHQ exact-ratio plan";
        if (eligible && job_try_fft(s, (int64_t)j.out_frames * j.n_clips * j.n_channels, sw.no_fft)) {
            if (const char *e = launch_fft(p, j, stream, handled)) return e;
            if (*handled) return nullptr;
            if (s.want_fft) return s.fft_f64 ? "FFT engine (float64 arithmetic) unavailable for this plan or layout (unit-stride columns of a tabled ratio)"
                                             : "FFT engine unavailable for this plan";
        }
    }
    if (s.want_pcm) { // (eligible: checked on entry)
        if (const char *e = launch_fft(p, j, stream, handled, t_ch_base)) return e;
        if (*handled) return nullptr;
        return "FFT engine (integer samples) unavailable for this plan or layout (unit-stride columns, or int16 interleaved channel pairs, of a tabled ratio)";
    }
    return nullptr;
}

const char *launch_job(Plan *p, const hipsoxr_job_t &j, void *stream, const VrPos *vr, ResidentLaunch *res, ChainDone *cd)
{
    if (cd) cd->n_wgs = 0;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return job_empty_refusal(res != nullptr);
    const bool vr_or_res = vr || res;
    if (const char *e = job_entry_refusal(*p, j, vr_or_res, res != nullptr)) return e;
    if (j.clip_table) return launch_job_table(p, j, stream);
    if (elem_is_half(j.elem)) return launch_job_half(p, j, stream);
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > kJobMaxCols && !job_wide_lane(cols, p->phases != 0, vr_or_res, j.n_clips, j.in_chan_stride, j.out_frames, j.n_channels, job_sel(j.kernel)))
        return launch_job_folded(p, j, stream, vr);
    if (const char *e = device_bank_ensure(p, engine_prec(j.elem))) return e;
    bool handled = false;
    if (const char *e = launch_job_engines(p, j, stream, vr_or_res, &handled)) return e;
    if (handled) return nullptr;
    return with_elem(j.elem, [&](auto io, auto real) { return launch_typed<decltype(io), decltype(real)>(p, j, (hipStream_t)stream, vr, res, cd); });
}

} // namespace hipsoxr
