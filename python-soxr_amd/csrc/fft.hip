// fft.hip — frequency-domain engine: rational overlap-save resampling.
//
// Same filter as the exact engine (kernels.hip), different evaluation.  The direct form spends 2*T flops per output
// (592 at VHQ 48k->44.1k) and is FMA-bound at <= 28 % of the HBM roofline.  Here the plan's own prototype g is applied
// in the frequency domain:
//
//   block of N_in = M*k input samples  --FFT-->  X[q]
//   Y[q] = X[q] * H[q]  for |q| <= min(N_in, N_out)/2, else 0     (H = DTFT of g at the bin frequencies; truncating /
//   zero-extending the spectrum IS the rate change: bins of both grids are f_in/N_in = f_out/N_out apart)
//   Y  --inverse FFT of size N_out = L*k-->  L*k output samples
//
// with overlap-save: blocks start on period boundaries (input index multiple of M <-> output index multiple of L),
// overlap by more than the filter length, and only the outputs whose whole filter support lies inside the block are
// kept.  ~70 flop per output instead of 592.  What is neglected is the aliasing of g's stop band (<= -176 dB for VHQ):
// against the direct form 2.5e-10 relative RMS in float64, ~2e-7 in float32 (FFT rounding) — inside the 1e-6 bar but
// NOT bit-identical to the canonical order, so this engine serves whole-signal device jobs (hipsoxr_run_device) —
// float32 / float64 ones, and int16 / int32 ones that name it (HIPSOXR_KERNEL_FFT_PCM) — and device-chunk streams that
// name it at creation (HIPSOXR_STREAM_FFT: every chunk a job WINDOW on the paired kernels, launch_fft_window); the host
// surface (soxr.resample / ResampleStream), every other stream and integer I/O under AUTO stay on the exact engine.
//
// Kernels:
//   k_fft_block     general path, any 7-smooth plan: one workgroup per block, run-time radix schedule, real FFT through
//                   a half-length complex transform (untangle * H * tangle).
//   k_fft_pair2     two real blocks ride as the real and imaginary part of ONE complex signal through
//                   FFT -> *H -> truncate -> inverse FFT (the chain is linear and real-to-real; H is real); compile-time
//                   three-pass schedules for the standard audio ratios; unit-stride columns (mono, planar, batches):
//                   raw buffer loads with the hardware range check, output runs staged through LDS and stored as
//                   16-byte granules.  float32, float64 and float32-on-float64 instances; int16-on-float32 and
//                   int32-on-float64 ones (HIPSOXR_KERNEL_FFT_PCM) with the exact engine's output stage in the store loop;
//                   float16- and bfloat16-on-float32 ones (HIPSOXR_F16 / HIPSOXR_BF16 jobs) with one rounding there.
//   k_fft_strided2  the same chain for columns with a frame stride: interleaved data paired by channel (CP = true:
//                   one (Real, Real) word per frame) or strided columns paired by block (CP = false).
// Build switches: -DFFT2_TRACE (per-wave s_memtime stamps of k_fft_pair2, tools/trace_pair2.py).  The experiments of
// rounds 1-4 (first-generation kernel, resident workgroups + queue, LDS-DMA staging, wave-local DIF schedule, early
// table loads, interleaved stores, ablation bits; two block pairs per workgroup, hand-packed complex arithmetic, the
// thread-count sweep) are in git history (tags r3-fft-experiments, r4-fft-experiments) and profiles/r03_* / r04_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

#include "device.h"
#ifndef FFT_FORCE_PK
#define FFT_NO_PK // (the packed-FMA forms of fft_dev.h: +8 % on k_fft_pair2 — 124 against 114 us — and -7 % on k_fft_wave, which alone uses them)
#endif
#include "fft_dev.h"
#include "pcm_out.h"
#include "half_rules.h"
#include "fft_ragged_rules.h"

namespace hipsoxr {

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return hipGetErrorString(e_); \
    } while (0)


// One Stockham pass of a length-N transform with a run-time schedule (k_fft_block), IN PLACE in a single LDS buffer:
// every thread reads the inputs of its butterflies into registers, the workgroup synchronises, then results are written
// to their autosort positions.  Radix R, Ns = product of earlier radices, NB = max butterflies per thread.
// W = table exp(SIGN*2*pi*i*m/N), m = 0..N-1 (L1/L2 resident); the t = 1 twiddle of a butterfly is loaded — from radix 5
// the t = 4 one as well — and the other powers are formed in registers.
template <int R, int SIGN, int NB>
__device__ __forceinline__ void fft_pass(cf *buf, int N, int Ns, const cf *W)
{
    const int nb = N / R, wstep = N / (Ns * R);
    cf u[NB][R];
    int dst[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = threadIdx.x + i * blockDim.x;
        dst[i] = -1;
        if (j < nb) {
            const int grp = j / Ns, k = j - grp * Ns;
            dst[i] = grp * Ns * R + k;
#pragma unroll
            for (int t = 0; t < R; ++t) u[i][t] = buf[j + t * nb];
            if (Ns > 1) {
                // w^t from w and, for the radices with t >= 4, a second entry w^4: w^(4a+b) = (w^4)^a w^b — t rounded
                // products of ONE entry carry t times its phase error, which at the peak of an impulse (crest factor 70)
                // is 4.6e-5 of the column's RMS with radix 16; with the second entry the factor is a + b <= 6
                // (profiles/NOTES_fft_block.md; fft_pass_ct does the same from radix 10)
                cf pw[4], w4 = make_float2(1.f, 0.f), base = w4;
                pw[1] = W[k * wstep];
                if (R >= 5) w4 = W[4 * k * wstep]; // 4 k wstep < 4 N / R < N
#pragma unroll
                for (int t = 1; t < R; ++t) {
                    const int a4 = t / 4, b4 = t % 4;
                    if (a4 == 0) {
                        if (t > 1) pw[t] = cmul(pw[t - 1], pw[1]);
                        u[i][t] = cmul(u[i][t], pw[t]);
                    } else {
                        if (b4 == 0) base = a4 == 1 ? w4 : cmul(base, w4);
                        u[i][t] = cmul(u[i][t], b4 == 0 ? base : cmul(base, pw[b4]));
                    }
                }
            }
            dft_r<R, SIGN>(u[i]);
        }
    }
    __syncthreads(); // all inputs of this pass are in registers
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (dst[i] >= 0) {
            cf *o = buf + dst[i];
#pragma unroll
            for (int t = 0; t < R; ++t) o[t * Ns] = u[i][t];
        }
    }
    __syncthreads();
}

// Compile-time specialised pass (N, Ns, R constants): no divisions, fully unrolled.
// `load(j, t)` supplies input t of butterfly j — element j + t * N/R of the pass input (LDS, or global memory for the
// first pass) — and `store(o, t, v)` consumes element o + t * Ns of its output (LDS, or the staging layout for the last
// pass), so the first pass streams straight from HBM without an extra LDS round trip.  Loaders and storers get the
// butterfly's own index and the COMPILE-TIME input number apart: everything that depends on t alone (offsets, which side
// of the spectrum a bin is on) folds into immediates, and a thread's addresses are a base register plus a constant.
// The in-place barrier stands straight behind the pass's LDS reads, not behind its butterflies: what it must guarantee
// is that every thread HOLDS its inputs, not that it has finished computing.
// Twiddles: any power formed from ONE rounded table entry inherits t times its phase error ((w(1+e))^t ~ w^t (1+te)),
// so for the large radices a second entry, w^4, is read and w^(4a+b) = (w^4)^a w^b: the error factor drops from R-1 to
// <= a+b for the same number of complex products (engine error 3.5e-7 -> 2.2e-7 relative RMS).
// `tid` = the thread's index among the NT threads that share ONE transform (threadIdx.x; an experiment of round 5 interleaved
// the transforms of four channel pairs across the lanes of one workgroup: profiles/NOTES_r05.md §3).
// Tw (one-round kernels, PassTabs): every factor w^(t k) of the pass comes from a per-pass table laid out [t][k] instead —
// correctly rounded constants of the plan, R - 1 loads at ONE per-thread offset (k) plus a constant each, issued where
// w1 / w4 are loaded (in flight during the LDS reads and the barrier); no powers are formed.  `tw_at` = the pass's first
// entry in the transform's table.
struct NoTabs { static constexpr bool on = false; };
struct PassTabs { static constexpr bool on = true; __amdgpu_buffer_rsrc_t r; };
template <int N, int Ns, int R, int SIGN, int NT, bool SYNC_BEFORE_STORE, int tw_at = 0, typename C, typename Load, typename Store, typename Tw = NoTabs>
__device__ __forceinline__ void fft_pass_ct(const C *W, Load load, Store store, const int tid, Tw tw = Tw())
{
    constexpr int nb = N / R, wstep = N / (Ns * R), NB = (nb + NT - 1) / NT;
    typedef real_of<C> T;
    C u[NB][R];
    if constexpr (Tw::on && Ns > 1) {
        static_assert(sizeof(C) == 8, "per-pass twiddle tables: float32 kernels");
        C f[NB][R];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = tid + i * NT;
            if (NB * NT == nb || j < nb) {
                const int k = j % Ns;
#pragma unroll
                for (int t = 1; t < R; ++t)
                    f[i][t] = __builtin_bit_cast(C, __builtin_amdgcn_raw_buffer_load_b64(tw.r, k * (int)sizeof(C), (tw_at + (t - 1) * Ns) * (int)sizeof(C), 0));
#pragma unroll
                for (int t = 0; t < R; ++t) u[i][t] = load(j, t);
            }
        }
        if (SYNC_BEFORE_STORE) __syncthreads(); // in place: every input of the pass is in registers
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int j = tid + i * NT;
            if (NB * NT == nb || j < nb) {
                const int k = j % Ns, o = (j - k) * R + k;
#pragma unroll
                for (int t = 1; t < R; ++t) u[i][t] = cmul(u[i][t], f[i][t]);
                dft_r<R, SIGN>(u[i]);
#pragma unroll
                for (int t = 0; t < R; ++t) store(o, t, u[i][t]);
            }
        }
        return;
    }
    C w1s[NB], w4s[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = tid + i * NT;
        w1s[i] = C((T)1, (T)0); w4s[i] = w1s[i];
        if (NB * NT == nb || j < nb) {
            const int k = j % Ns;
            if (Ns > 1) w1s[i] = W[k * wstep];
            if (Ns > 1 && R >= 10) w4s[i] = W[4 * k * wstep]; // 4*k*wstep < 4N/R <= N
#pragma unroll
            for (int t = 0; t < R; ++t) u[i][t] = load(j, t);
        }
    }
    if (SYNC_BEFORE_STORE) __syncthreads(); // in place: every input of the pass is in registers
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int j = tid + i * NT;
        if (NB * NT == nb || j < nb) {
            const int k = j % Ns, o = (j - k) * R + k;
            if (Ns > 1) {
                C pw[R];
                const C w1 = w1s[i];
                pw[1] = w1;
                if constexpr (R >= 10) {
                    const C w4 = w4s[i];
#pragma unroll
                    for (int t = 2; t < R; ++t) {
                        const int a4 = t / 4, b4 = t % 4;
                        if (a4 == 0) pw[t] = cmul(pw[t - 1], w1);
                        else if (b4 == 0) pw[t] = a4 == 1 ? w4 : (a4 % 2 == 0 ? cmul(pw[t / 2], pw[t / 2]) : cmul(pw[t - 4], w4));
                        else pw[t] = cmul(pw[4 * a4], pw[b4]);
                    }
                } else {
#pragma unroll
                    for (int t = 2; t < R; ++t) pw[t] = (t & 1) ? cmul(pw[t - 1], w1) : cmul(pw[t / 2], pw[t / 2]);
                }
#pragma unroll
                for (int t = 1; t < R; ++t) u[i][t] = cmul(u[i][t], pw[t]);
            }
            dft_r<R, SIGN>(u[i]);
#pragma unroll
            for (int t = 0; t < R; ++t) store(o, t, u[i][t]);
        }
    }
}

// own += s * other in place for n consecutive floats of v, `other` = the neighbouring lane's (lane ^ 1) value through DPP.
// By hand: before register allocation the product is a three-address v_fma_f32, which has no DPP encoding on gfx950, so
// the compiler leaves __builtin_amdgcn_update_dpp as a v_mov_b32_dpp in front of every v_fmac (two instructions per
// real).  One block, so that ONE s_nop covers the two wait states a DPP read needs behind the vector instruction that
// wrote its source (the hazard recogniser does not look into inline assembly); no instruction of the block reads what
// another one wrote.
#define FFT_PAIR_X(n) "v_fmac_f32_dpp %" #n ", %" #n ", %[s] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
__device__ __forceinline__ void pair_exchange(float2 (&u)[7], float s)
{
    asm volatile("s_nop 1\n\t" FFT_PAIR_X(0) FFT_PAIR_X(1) FFT_PAIR_X(2) FFT_PAIR_X(3) FFT_PAIR_X(4) FFT_PAIR_X(5) FFT_PAIR_X(6)
                 FFT_PAIR_X(7) FFT_PAIR_X(8) FFT_PAIR_X(9) FFT_PAIR_X(10) FFT_PAIR_X(11) FFT_PAIR_X(12) FFT_PAIR_X(13)
                 : "+v"(u[0].x), "+v"(u[0].y), "+v"(u[1].x), "+v"(u[1].y), "+v"(u[2].x), "+v"(u[2].y), "+v"(u[3].x), "+v"(u[3].y),
                   "+v"(u[4].x), "+v"(u[4].y), "+v"(u[5].x), "+v"(u[5].y), "+v"(u[6].x), "+v"(u[6].y)
                 : [s] "v"(s));
}
__device__ __forceinline__ void pair_exchange(float2 (&u)[8], float s)
{
    asm volatile("s_nop 1\n\t" FFT_PAIR_X(0) FFT_PAIR_X(1) FFT_PAIR_X(2) FFT_PAIR_X(3) FFT_PAIR_X(4) FFT_PAIR_X(5) FFT_PAIR_X(6)
                 FFT_PAIR_X(7) FFT_PAIR_X(8) FFT_PAIR_X(9) FFT_PAIR_X(10) FFT_PAIR_X(11) FFT_PAIR_X(12) FFT_PAIR_X(13) FFT_PAIR_X(14) FFT_PAIR_X(15)
                 : "+v"(u[0].x), "+v"(u[0].y), "+v"(u[1].x), "+v"(u[1].y), "+v"(u[2].x), "+v"(u[2].y), "+v"(u[3].x), "+v"(u[3].y),
                   "+v"(u[4].x), "+v"(u[4].y), "+v"(u[5].x), "+v"(u[5].y), "+v"(u[6].x), "+v"(u[6].y), "+v"(u[7].x), "+v"(u[7].y)
                 : [s] "v"(s));
}
#undef FFT_PAIR_X

// Lane-pair form of a radix-14 pass (one-round float32 kernels, where a pass of N/14 butterflies leaves two of five waves
// idle at the barrier): lanes 2j and 2j + 1 share butterfly j.  14 = 2 x 7 by the Good-Thomas maps of dft_pfa<2, 7>, the
// two dimensions taken in the other order: lane a (= tid & 1) holds the residue class n1 = a — inputs
// t = (7a + 2i) mod 14, i < 7 — twiddles them, runs dft_r<7>, and the 2-point stage is one v_fmac_f32 per real whose
// multiplicand comes from the neighbour through DPP (quad_perm [1,0,3,2]): no LDS trip, no barrier.  Lane a keeps
// output k1 = a: X[(7a + 8i) mod 14] = y0[i] + (-1)^a y1[i].  Lane 1 carries -y1 (its twiddles are read half a turn
// further on in W), so both lanes compute own + s * other with s = -1 / +1: one instruction stream.
// Everything that depends on t is base + immediate: t = 2i + 7a (i <= 3) or 2i - 7a (i >= 4), so a lane has two input
// bases (n_lo, n_hi); output m = 8i mod 14 + 7a (i even) or - 7a (i odd), two output bases (all kept non-negative).  `load_at(n)` / `store_at(n, v)`
// take element indices of the pass input / output.
// Twiddles w^(t k): three table entries per lane — g = w^2, b_lo = w^(7a), b_hi = w^(8 - 7a), each rounded once — and
// w^t = b_lo g^i (i <= 3) or b_hi g^(i - 4): seven products instead of twelve, error factor <= 1 + 3 (see fft_pass_ct: <= 5).
template <int N, int Ns, int SIGN, int NT, bool SYNC_BEFORE_STORE, typename C, typename LoadAt, typename StoreAt>
__device__ __forceinline__ void fft_pass_pair14(const C *W, LoadAt load_at, StoreAt store_at, const int tid)
{
    constexpr int R = 14, nb = N / R, wstep = N / (Ns * R);
    static_assert(sizeof(C) == 8 && N % 2 == 0 && Ns > 1 && 2 * nb <= NT, "lane-pair radix-14 pass: float32, a twiddled pass, one half-butterfly per thread");
    const int j = tid >> 1, a = tid & 1;
    const bool live = 2 * nb == NT || j < nb; // (2 nb is even: both lanes of a pair are in or out)
    const int k = j % Ns;
    C u[7], g, b_lo, b_hi;
    if (live) {
        const int kw = k * wstep, half = a * (N / 2);
        g = W[2 * kw];
        b_lo = W[7 * a * kw + half];       // 1 or -w^7
        b_hi = W[(8 - 7 * a) * kw + half]; // w^8 or -w
        const int n_lo = j + 7 * a * nb, n_hi = j + (8 - 7 * a) * nb; // inputs 0 / 7 and 8 / 1: non-negative bases
#pragma unroll
        for (int i = 0; i < 7; ++i) u[i] = i <= 3 ? load_at(n_lo + 2 * i * nb) : load_at(n_hi + (2 * i - 8) * nb);
    }
    if (SYNC_BEFORE_STORE) __syncthreads(); // in place: every input of the pass is in registers
    if (live) {
        const C g2 = cmul(g, g), g3 = cmul(g2, g);
        u[0] = cmul(u[0], b_lo); u[1] = cmul(u[1], cmul(b_lo, g)); u[2] = cmul(u[2], cmul(b_lo, g2)); u[3] = cmul(u[3], cmul(b_lo, g3));
        u[4] = cmul(u[4], b_hi); u[5] = cmul(u[5], cmul(b_hi, g)); u[6] = cmul(u[6], cmul(b_hi, g2));
        dft_r<7, SIGN>(u);
        const float s = a ? 1.f : -1.f;
        pair_exchange(u, s);
        const int o = (j - k) * R + k, o_ev = o + 7 * a * Ns, o_od = o + (8 - 7 * a) * Ns; // outputs 0 / 7 and 8 / 1
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i % 2 == 0) store_at(o_ev + ((8 * i) % R) * Ns, u[i]);
            else store_at(o_od + ((8 * i) % R - 8) * Ns, u[i]);
        }
    }
}

// Lane-pair form of a radix-16 FIRST pass (Ns = 1: no external twiddles; its N/16 butterflies fill little more than two of
// five waves): 16 = 2 x 8 by decimation in time.  Lane a of the pair of butterfly j loads inputs t = 2i + a, i < 8 —
// `load(j + a N/16, 2i)`: half the loads per lane — runs dft_r<8>, multiplies by the internal factors (lane 0: 1; lane 1:
// -w16^q, per-lane constants), and X[q + 8a] = own + s * other as in fft_pass_pair14.  `store(j, a, q, v)` takes output q + 8a.
template <int N, int SIGN, int NT, bool SYNC_BEFORE_STORE, typename C, typename Load, typename Store>
__device__ __forceinline__ void fft_pass_pair16(Load load, Store store, const int tid)
{
    constexpr int nb = N / 16;
    constexpr double PI2 = 6.283185307179586476925286766559;
    static_assert(sizeof(C) == 8 && 2 * nb <= NT, "lane-pair radix-16 pass: float32, one half-butterfly per thread");
    const int j = tid >> 1, a = tid & 1;
    const bool live = 2 * nb == NT || j < nb;
    C u[8];
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) u[i] = load(j + a * nb, 2 * i);
    }
    if (SYNC_BEFORE_STORE) __syncthreads();
    if (live) {
        dft_r<8, SIGN>(u);
        const float s = a ? 1.f : -1.f;
        u[0] = C(-s * u[0].x, -s * u[0].y);
#pragma unroll
        for (int q = 1; q < 8; ++q) {
            const float wr = -(float)__builtin_cos(PI2 * q / 16), wi = -(float)(SIGN * __builtin_sin(PI2 * q / 16));
            u[q] = cmul(u[q], C(a ? wr : 1.f, a ? wi : 0.f));
        }
        pair_exchange(u, s);
#pragma unroll
        for (int q = 0; q < 8; ++q) store(j, a, q, u[q]);
    }
}

// Three-pass transform: first pass input from `first_load`, last pass output to `last_store`, in place in between.
// LDS bank conflicts: pass loads are contiguous across lanes (conflict-free); pass stores run in groups of Ns consecutive
// elements, so only the FIRST pass (Ns = 1: lane stride = R0 elements) can conflict.  An odd-ish R0 (5, 21: stride 40 /
// 168 bytes) is conflict-free as it is; for R0 = 16 (stride 128 bytes = every lane on the same two banks) the buffer
// between pass 1 and pass 2 is kept in a swizzled layout  n -> n ^ ((n >> 4) & 15)  (SWZ).  What the swizzle costs in
// address arithmetic (round 5): pass 1 stores element t of butterfly j at 16 j + (t ^ (j & 15)) — one XOR per element;
// pass 2 reads element j + t * N/R1, whose mask ((j >> 4) + t * N/(16 R1)) & 15 takes only 16 / gcd(16, N/(16 R1))
// different values over t (four for 5120 = 16 * 16 * 20): that many base addresses per thread, every read an immediate
// offset from one of them (it was an add, a shift-and-mask and an XOR per element: 65 -> 16 vector instructions).
#ifdef FFT2_TRACE
#define FFT_STAMP() do { if (g_tr && (threadIdx.x & 63) == 0 && g_tri < 16) g_tr[g_tri] = __builtin_amdgcn_s_memtime(); ++g_tri; } while (0)
#define FFT_STAMP_DECL unsigned long long *g_tr, int &g_tri,
#define FFT_STAMP_ARGS g_tr, g_tri,
#else
#define FFT_STAMP() ((void)0)
#define FFT_STAMP_DECL
#define FFT_STAMP_ARGS
#endif
// (last_store_alt / use_alt: a second form of the last pass's consumer behind ONE wave-uniform branch around the whole pass)
// tw (PassTabs): the twiddled passes named by TABS (bit 0: pass 2, bit 1: pass 3) read their factors from the
// transform's per-pass tables — pass 2's [t][k] block of (R1 - 1) R0 entries, then pass 3's of (R2 - 1) R0 R1 (host side:
// pass_tables, which lays out both whatever TABS says) — instead of forming them from W.
// SPLIT: the passes that run in the lane-pair form (bit 0: a radix-16 pass 1, fft_pass_pair16; bit 1: a radix-14 pass 2,
// fft_pass_pair14).
template <int N, int SIGN, int NT, int R0, int R1, int R2, bool SWZ, bool LASTSYNC, int TABS = 3, int SPLIT = 0, typename C, typename Load, typename Store, typename StoreAlt, typename Tw = NoTabs>
__device__ __forceinline__ void fft_ct3(FFT_STAMP_DECL C *buf, const C *W, Load first_load, Store last_store, bool first_in_lds, StoreAlt last_store_alt,
                                        bool use_alt, const int tid, Tw tw = Tw())
{
    static_assert(R0 * R1 * R2 == N, "radix schedule");
    static_assert(!SWZ || R0 == 16, "the swizzled layout is the radix-16 first pass's");
    constexpr int nb1 = N / R1, nb2 = N / R2;
    auto lds_load2 = [&](int j, int t) -> C { return buf[j + t * nb2]; };
    auto lds_store1 = [&](int o, int t, C v) { buf[o + t * R0] = v; };
    auto swz_load = [&](int j, int t) -> C {
        if constexpr (!SWZ) return buf[j + t * nb1];
        else if constexpr (nb1 % 16 == 0) // the element's row (n >> 4) = (j >> 4) + t * nb1 / 16: its low four bits repeat over t
            return buf[(j & ~15) + t * nb1 + ((j & 15) ^ (((j >> 4) + ((t * (nb1 / 16)) & 15)) & 15))];
        else { const int n = j + t * nb1; return buf[n ^ ((n >> 4) & 15)]; }
    };
    auto swz_store = [&](int o, int t, C v) { // pass 0: Ns = 1, o = R0 j
        // 16 j + (t ^ (j & 15)) = (16 j | (j & 15)) ^ t: one XOR of a per-thread byte offset with a constant per element
        if constexpr (SWZ) *reinterpret_cast<C *>(reinterpret_cast<char *>(buf) + ((unsigned)((o | ((o >> 4) & 15)) * (int)sizeof(C)) ^ (unsigned)(t * (int)sizeof(C)))) = v;
        else buf[o + t] = v;
    };
    // pass 0 (Ns = 1): when its input is not in LDS nothing has to be protected before storing
    if constexpr ((SPLIT & 1) != 0) {
        static_assert(R0 == 16 && SWZ, "lane-pair pass 1: radix 16 into the swizzled layout");
        // swz_store's element 16 j + ((q + 8 a) ^ (j & 15)): the lane's byte offset XOR 64 a, then XOR a constant per output
        auto pair_store = [&](int j, int a, int q, C v) {
            *reinterpret_cast<C *>(reinterpret_cast<char *>(buf) + (((unsigned)((16 * j | (j & 15)) * (int)sizeof(C)) ^ (unsigned)(a * 8 * (int)sizeof(C))) ^ (unsigned)(q * (int)sizeof(C)))) = v;
        };
        if (first_in_lds) fft_pass_pair16<N, SIGN, NT, true, C>(first_load, pair_store, tid);
        else fft_pass_pair16<N, SIGN, NT, false, C>(first_load, pair_store, tid);
    } else if (first_in_lds) fft_pass_ct<N, 1, R0, SIGN, NT, true>(W, first_load, swz_store, tid);
    else fft_pass_ct<N, 1, R0, SIGN, NT, false>(W, first_load, swz_store, tid);
    FFT_STAMP();
    __syncthreads();
    FFT_STAMP();
    if constexpr ((SPLIT & 2) != 0) {
        static_assert(R1 == 14 && !(TABS & 1), "lane-pair pass 2: radix 14, powers formed in registers");
        fft_pass_pair14<N, R0, SIGN, NT, true>(W, [&](int n) -> C { if constexpr (SWZ) return buf[n ^ ((n >> 4) & 15)]; else return buf[n]; },
                                               [&](int n, C v) { buf[n] = v; }, tid); // (lds_store1's layout: element o + t * R0)
    } else if constexpr (TABS & 1) fft_pass_ct<N, R0, R1, SIGN, NT, true, 0>(W, swz_load, lds_store1, tid, tw);
    else fft_pass_ct<N, R0, R1, SIGN, NT, true>(W, swz_load, lds_store1, tid);
    FFT_STAMP();
    __syncthreads();
    FFT_STAMP();
    if constexpr (TABS & 2) {
        if (use_alt) fft_pass_ct<N, R0 * R1, R2, SIGN, NT, LASTSYNC, (R1 - 1) * R0>(W, lds_load2, last_store_alt, tid, tw);
        else fft_pass_ct<N, R0 * R1, R2, SIGN, NT, LASTSYNC, (R1 - 1) * R0>(W, lds_load2, last_store, tid, tw);
    } else {
        if (use_alt) fft_pass_ct<N, R0 * R1, R2, SIGN, NT, LASTSYNC>(W, lds_load2, last_store_alt, tid);
        else fft_pass_ct<N, R0 * R1, R2, SIGN, NT, LASTSYNC>(W, lds_load2, last_store, tid);
    }
    FFT_STAMP();
}


// butterflies per thread are bounded by N/(R*256) rounded up; lengths up to 4096
template <int SIGN>
__device__ __forceinline__ void run_passes(cf *buf, int N, int n_pass, const int32_t *rad, const cf *W)
{
    int Ns = 1;
    for (int p = 0; p < n_pass; ++p) {
        const int R = rad[p];
        const int per = (N / R + (int)blockDim.x - 1) / (int)blockDim.x; // wave-uniform
        // butterflies per thread (256 threads, N <= 4096): R=16: 1, R=8: <=2, R=7: <=3, R=5,4: <=4, R=3: <=6, R=2: <=8
        switch (R) {
        case 16: fft_pass<16, SIGN, 1>(buf, N, Ns, W); break;
        case 8: if (per <= 1) fft_pass<8, SIGN, 1>(buf, N, Ns, W); else fft_pass<8, SIGN, 2>(buf, N, Ns, W); break;
        case 7: if (per <= 2) fft_pass<7, SIGN, 2>(buf, N, Ns, W); else fft_pass<7, SIGN, 3>(buf, N, Ns, W); break;
        case 5: if (per <= 2) fft_pass<5, SIGN, 2>(buf, N, Ns, W); else fft_pass<5, SIGN, 4>(buf, N, Ns, W); break;
        case 4: if (per <= 2) fft_pass<4, SIGN, 2>(buf, N, Ns, W); else fft_pass<4, SIGN, 4>(buf, N, Ns, W); break;
        case 3: if (per <= 4) fft_pass<3, SIGN, 4>(buf, N, Ns, W); else fft_pass<3, SIGN, 6>(buf, N, Ns, W); break;
        default: fft_pass<2, SIGN, 8>(buf, N, Ns, W); break;
        }
        Ns *= R;
    }
}

// ---------------------------------------------------------------------------------------------
// General path: one block per workgroup, run-time radix schedule, any 7-smooth plan (ratios outside the table below).
// ---------------------------------------------------------------------------------------------
#if !defined(FFT_PART) || FFT_PART == 0 // (not a template: one translation unit only)
__global__ void __launch_bounds__(256, 2) k_fft_block(FftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int32_t A = a.A, B = a.B;
    cf *cur = reinterpret_cast<cf *>(smem_raw); // single buffer of max(A, B) + 1 complex values

    const uint32_t col = blockIdx.y;
    const uint32_t ch = col % a.n_channels, clip = col / a.n_channels;
    const int64_t blk = blockIdx.x;
    const int64_t p0 = blk * a.hop_periods - a.lead_periods; // first period of the block (may be < 0)
    const int64_t in0 = p0 * a.M, out0 = p0 * a.L;          // absolute indices of local sample 0
    const float *xin = (const float *)a.in + (int64_t)clip * a.ics + (int64_t)ch * a.ichs;

    // ---- load: z[n] = x[2n] + i x[2n+1], zero outside the signal; forward complex FFT of length A
    for (int n = threadIdx.x; n < A; n += blockDim.x) {
        const int64_t l = in0 + 2 * (int64_t)n;
        float re = (l >= a.in_lo && l < a.in_frames) ? xin[l * a.ifs] : 0.f;
        float im = (l + 1 >= a.in_lo && l + 1 < a.in_frames) ? xin[(l + 1) * a.ifs] : 0.f;
        cur[n] = make_float2(re, im);
    }
    __syncthreads();
    run_passes<-1>(cur, A, a.nA, a.radA, a.WA);
    __syncthreads();

    // ---- untangle the real FFT, apply the filter, tangle for the inverse real FFT — in registers:
    //      X[q] = (Z[q] + conj Z[A-q])/2 - i/2 P[q] (Z[q] - conj Z[A-q]),   P[q] = exp(-2 pi i q / N_in)
    //      Y[q] = X[q] Hs[q]  (q <= min(A, B), else 0)
    //      W[q] = (Y[q] + conj Y[B-q]) + i Q[q] (Y[q] - conj Y[B-q]),       Q[q] = exp(+2 pi i q / N_out)
    // thread handles the pair (q, B-q): it needs Z[q], Z[A-q], Z[B-q], Z[A-B+q].
    {
        const int qmax = A < B ? A : B;
        auto spectrum = [&](int q) -> cf { // Y[q]
            if (q > qmax) return make_float2(0.f, 0.f);
            const cf zq = cur[q == A ? 0 : q], zc = cconj(cur[q == 0 ? 0 : A - q]);
            const cf s = cadd(zq, zc), d = cmul(a.P[q], csub(zq, zc));
            const cf x = make_float2(0.5f * (s.x + d.y), 0.5f * (s.y - d.x));
            return cmul(x, a.Hs[q]);
        };
        constexpr int NP = (4096 / 2 + 1 + 255) / 256; // pairs per thread: B/2 + 1 <= 256 * NP (B <= 4096)
        cf wq[NP], wr[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = threadIdx.x + i * blockDim.x;
            if (q <= B / 2) {
                const cf yq = spectrum(q), yr = spectrum(B - q);
                // W[q] from (Y[q], Y[B-q]);  W[B-q] from (Y[B-q], Y[q])
                cf s = cadd(yq, cconj(yr)), d = cmul(a.Q[q], csub(yq, cconj(yr)));
                wq[i] = make_float2(s.x - d.y, s.y + d.x);
                if (q != 0 && q != B - q) {
                    s = cadd(yr, cconj(yq)); d = cmul(a.Q[B - q], csub(yr, cconj(yq)));
                    wr[i] = make_float2(s.x - d.y, s.y + d.x);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int q = threadIdx.x + i * blockDim.x;
            if (q <= B / 2) {
                cur[q] = wq[i];
                if (q != 0 && q != B - q) cur[B - q] = wr[i];
            }
        }
    }
    __syncthreads();

    // ---- inverse complex FFT of length B (unnormalised; the scale lives in Hs) and store of the kept outputs:
    //      element n of the result holds local outputs 2n (re) and 2n+1 (im)
    float *yo = (float *)a.out + (int64_t)clip * a.ocs + (int64_t)ch * a.ochs;
    const int32_t v0 = a.v0, v1 = a.v0 + a.hop_out;
    run_passes<+1>(cur, B, a.nB, a.radB, a.WB);
    for (int n = threadIdx.x; n < B; n += blockDim.x) {
        const cf w = cur[n];
        const int32_t i0 = 2 * n;
        const int64_t k0 = out0 + i0;
        if (i0 >= v0 && i0 < v1 && k0 >= 0 && k0 < a.out_frames) yo[k0 * a.ofs] = w.x;
        if (i0 + 1 >= v0 && i0 + 1 < v1 && k0 + 1 >= 0 && k0 + 1 < a.out_frames) yo[(k0 + 1) * a.ofs] = w.y;
    }
}
#endif

// ---------------------------------------------------------------------------------------------
// Paired-block kernels.  The whole chain  FFT -> multiply by H -> truncate -> inverse FFT  maps real signals to real
// signals and is linear, so it processes TWO real blocks at once as the real and imaginary part of one complex signal:
// z = x_a + i x_b  ->  y_a + i y_b  (H is Hermitian — real, in fact: the prototype is symmetric about the output instant
// and blocks are cut on period boundaries — and the truncation symmetric).  No real-FFT untangle/tangle stages; the
// filter multiply rides on the loads of the first inverse pass; with radix-16/20/21 butterflies 3 + 3 LDS passes per
// pair of blocks.
// Schedules: N_in = A0*A1*A2 (forward), N_out = B0*B1*B2 (inverse); *SWZ = swizzled layout after a power-of-two first
// radix (see fft_ct3).  NT >= the largest butterfly count of any pass.
// ---------------------------------------------------------------------------------------------
// TABS_: which twiddled passes of both transforms take their factors from per-pass tables (FftArgs::TWA / TWB, float32;
// the one-round kernels; bits as FFT_ONE_ROUND_TABS).  fwd / inv_staged then get the transform's PassTabs; everything
// else leaves the argument out.
// Which passes of the one-round float32 kernels run in the lane-pair form (fft_pass_pair16 / fft_pass_pair14): bit 0 / 1 =
// forward pass 1 / 2, bit 2 / 3 = inverse pass 1 / 2.  What a kernel HAS: 2240 x 2058 a radix-16 forward pass 1 from HBM
// and both radix-14 passes 2 (11); 2058 x 2240 both passes 2 (10) — its radix-16 pass is the inverse's first, whose loader
// decides the side of the spectrum per compile-time input: not built.  The kernels of 20 periods keep the plain passes:
// 2940 / 14 = 210 butterflies are 420 halves, two rounds of the 320 threads — no shorter than one round of whole
// butterflies — and 3200 = 16 * 20 * 10 has no radix-14 pass.
// What a kernel KEEPS is what was measured to gain (k = 14 forced, 60 s mono, us per launch, three alternated runs each,
// spread <= 0.03: profiles/NOTES_one_round_split.md):
//   2240 x 2058  parent 9.86; forward pass 1 alone 10.60, forward pass 2 alone 10.70, inverse pass 2 alone 9.56, all 10.62
//   2058 x 2240  parent 9.70; forward pass 2 alone 9.79, inverse pass 2 alone 9.56, both 9.45
// The forward passes of 2240 read and write LDS rows a multiple of 256 bytes apart from the two lanes of a pair (two-way
// bank conflicts on every access); why the conflict-free radix-16 pass loses as much is not understood.
// -DFFT_ONE_ROUND_SPLIT=mask (A/B builds): that mask in both kernels instead, cut down to what each has.
#ifdef FFT_ONE_ROUND_SPLIT
constexpr int pair_split(int NA, int NB) { return (NA == 2240 && NB == 2058 ? 11 : NA == 2058 && NB == 2240 ? 10 : 0) & (FFT_ONE_ROUND_SPLIT); }
#else
constexpr int pair_split(int NA, int NB) { return NA == 2240 && NB == 2058 ? 8 : NA == 2058 && NB == 2240 ? 10 : 0; }
#endif
template <int NA_, int NB_, int NT_, int A0, int A1, int A2, bool ASWZ, int B0, int B1, int B2, bool BSWZ, int TABS_ = 0>
struct PairSpec {
    static constexpr int NA = NA_, NB = NB_, NT = NT_;
    static constexpr int RA0 = A0, RA2 = A2, RB0 = B0, RB2 = B2;
    static constexpr int TABS = TABS_; // bit 0: pass 2, bit 1: pass 3
    static constexpr int SPLIT = pair_split(NA_, NB_); // lane-pair passes (float32 one-round kernels): bits 0-1 forward pass 1, 2; bits 2-3 inverse pass 1, 2
    static constexpr int TWA_N = (A1 - 1) * A0 + (A2 - 1) * A0 * A1, TWB_N = (B1 - 1) * B0 + (B2 - 1) * B0 * B1; // entries of the per-pass tables
    template <int SPLIT2 = 0, typename C, typename Ld, typename St, typename Tw = NoTabs> static __device__ __forceinline__ void fwd(FFT_STAMP_DECL C *b, const C *W, Ld ld, St st, int tid = (int)threadIdx.x, Tw tw = Tw())
    { fft_ct3<NA, -1, NT, A0, A1, A2, ASWZ, false, TABS, SPLIT2>(FFT_STAMP_ARGS b, W, ld, st, false, st, false, tid, tw); }
    template <typename C, typename Ld, typename St> static __device__ __forceinline__ void inv(FFT_STAMP_DECL C *b, const C *W, Ld ld, St st, int tid = (int)threadIdx.x)
    { fft_ct3<NB, +1, NT, B0, B1, B2, BSWZ, false>(FFT_STAMP_ARGS b, W, ld, st, true, st, false, tid); }
    // last pass stores into LDS in another layout (output staging): all its inputs must be in registers first
    template <int SPLIT2 = 0, typename C, typename Ld, typename St, typename StAlt, typename Tw = NoTabs> static __device__ __forceinline__ void inv_staged(FFT_STAMP_DECL C *b, const C *W, Ld ld, St st, StAlt st_alt, bool use_alt, Tw tw = Tw())
    { fft_ct3<NB, +1, NT, B0, B1, B2, BSWZ, true, TABS, SPLIT2>(FFT_STAMP_ARGS b, W, ld, st, true, st_alt, use_alt, (int)threadIdx.x, tw); }
};
// Three-pass schedule of each transform length in use (first radix 21: conflict-free as it is; first radix 16:
// swizzled layout between pass 1 and 2).  4410 = 21*14*15 is the order the product runs (configs[2] 47 us, against
// 52 us with the radix-15 pass first).
template <int N> struct Sched;
#define HIPSOXR_SCHED_LIST(X)                                                                                        \
    X(7056, 21, 16, 21, false) X(5376, 21, 16, 16, false) X(5120, 16, 16, 20, true) X(4704, 21, 16, 14, false)       \
    X(4410, 21, 14, 15, false) X(4096, 16, 16, 16, true) X(3840, 16, 16, 15, true) X(3584, 14, 16, 16, false)        \
    X(3528, 21, 12, 14, false) X(2688, 21, 16, 8, false) X(2560, 16, 16, 10, true) X(2352, 21, 16, 7, false)         \
    X(2048, 16, 16, 8, true) X(1792, 7, 16, 16, false) X(1024, 16, 8, 8, true) X(1600, 16, 10, 10, true)             \
    X(1280, 5, 16, 16, false) X(1176, 21, 8, 7, false) X(896, 7, 16, 8, false)
// ... and the lengths of the one-round float32 kernels (HIPSOXR_PART5_SPECS): twiddles from per-pass tables
#ifndef FFT_ONE_ROUND_TABS
// Which twiddled passes read the tables: bit 0 = pass 2, bit 1 = pass 3.  Pass 3 alone: its [t][k] rows are Ns = R0 R1
// consecutive entries, one contiguous run per wave and load; pass 2 has Ns = R0 = 16 or 21 — every load of a wave
// fetches the same 16 or 21 entries four times over, 13 loads against the 12 products they replace, and the launch gets
// SLOWER (60 s clip, us per launch: parent 11.04, pass 2 alone 11.52, pass 3 alone 10.82, both 11.70:
// profiles/NOTES_one_round_chain.md).
#define FFT_ONE_ROUND_TABS 2
#endif
#define HIPSOXR_SCHED_TABS_LIST(X) \
    X(2240, 16, 14, 10, true) X(2058, 21, 14, 7, false) X(3200, 16, 20, 10, true) X(2940, 21, 14, 10, false)
#define HIPSOXR_SCHED(N, r0, r1, r2, swz) \
    template <> struct Sched<N> { static constexpr int R0 = r0, R1 = r1, R2 = r2; static constexpr bool SWZ = swz; static constexpr int TABS = 0; };
HIPSOXR_SCHED_LIST(HIPSOXR_SCHED)
#undef HIPSOXR_SCHED
#define HIPSOXR_SCHED(N, r0, r1, r2, swz) \
    template <> struct Sched<N> { static constexpr int R0 = r0, R1 = r1, R2 = r2; static constexpr bool SWZ = swz; static constexpr int TABS = FFT_ONE_ROUND_TABS; };
HIPSOXR_SCHED_TABS_LIST(HIPSOXR_SCHED)
#undef HIPSOXR_SCHED
// ... in the kernel where they were measured to gain: 2240 x 2058 (48k -> 44.1k, 14 periods: 60 s mono 10.31 -> 10.12 us,
// 2 x 30 s 9.95 -> 9.75).  3200 x 2940 is unchanged by them to 0.01 us, and both 44.1k -> 48k kernels get 0.1-0.25 us
// SLOWER (2 x 20 s 8.62 -> 8.86, 2 x 45 s 11.83 -> 11.96): those three keep forming their powers.
constexpr int pair_tabs(int NA, int NB, int a, int b) { return NA == 2240 && NB == 2058 ? (a & b) : 0; }
template <int NA, int NB, int NT>
using PairOf = PairSpec<NA, NB, NT, Sched<NA>::R0, Sched<NA>::R1, Sched<NA>::R2, Sched<NA>::SWZ, Sched<NB>::R0, Sched<NB>::R1,
                        Sched<NB>::R2, Sched<NB>::SWZ, pair_tabs(NA, NB, Sched<NA>::TABS, Sched<NB>::TABS)>;


// Input t of butterfly j of the FIRST INVERSE pass: bin n = j + t * NB/RB0 of the output grid <- bin n (non-negative
// frequencies, n <= NB/2) or n + NA - NB (negative ones) of the input grid in `buf`, times the real filter gain of
// |frequency| — read through the descriptor `rh` over Hr[0 .. NB/2] with the t-dependent part of the offset in the scalar
// operand.  Which side of the spectrum a bin lies on is known at compile time for all but the one t that straddles NB/2.
template <typename Spec, typename Real, typename C>
__device__ __forceinline__ C spectrum_load(const C *buf, __amdgpu_buffer_rsrc_t rh, int j, int t)
{
    constexpr int NA = Spec::NA, NB = Spec::NB, nbB = NB / Spec::RB0, RS = (int)sizeof(Real);
    const int lo = t * nbB, hi = lo + nbB - 1; // the bins this input can be, over all butterflies (j < nbB)
    const int n = j + lo;
    if constexpr (NA >= NB) {
        if (hi <= NB / 2) {        // non-negative frequencies
            const Real h = buf_load_real<Real>(rh, j * RS, lo * RS);
            const C x = buf[n];
            return C(x.x * h, x.y * h);
        } else if (lo > NB / 2) {  // negative frequencies: |q| = NB - n = (NB - lo - nbB) + (nbB - j)
            const Real h = buf_load_real<Real>(rh, (nbB - j) * RS, (NB - lo - nbB) * RS);
            const C x = buf[n + (NA - NB)];
            return C(x.x * h, x.y * h);
        } else {                   // the butterfly input that straddles the middle
            const bool neg = n > NB / 2;
            const Real h = buf_load_real<Real>(rh, (neg ? NB - n : n) * RS, 0);
            const C x = buf[neg ? n + (NA - NB) : n];
            return C(x.x * h, x.y * h); // (the Nyquist bin's alias term is dropped with Im H: stop band, < -170 dB)
        }
    } else {
        const bool neg = n > NB / 2;
        const int q = neg ? NB - n : n; // |frequency| in bins
        const bool in_band = q < NA / 2;
        const Real h = buf_load_real<Real>(rh, q * RS, 0);
        const C x = buf[in_band ? (neg ? NA - q : q) : 0];
        return in_band ? C(x.x * h, x.y * h) : C((Real)0, (Real)0);
    }
}

// ---------------------------------------------------------------------------------------------
// k_fft_pair2: unit-stride columns (mono / planar data; batches).  How it touches HBM:
//   * input: raw buffer loads whose descriptor covers [first sample of the item's first block, end of the column): the
//     hardware range check returns 0 past the end of the signal (no per-element bounds code, one path for interior and
//     last items), and the per-butterfly offsets t*N/R0 (+ block * hop) ride in the instruction's scalar offset instead
//     of 64-bit vector address arithmetic;
//   * output: the last inverse pass writes its kept outputs into LDS as the contiguous run they are in memory (block a
//     then block b of the pair: 2 hop_out consecutive elements of the column), index-shifted so that LDS and memory
//     agree on 16-byte phase, and the workgroup then stores the run with 16-byte buffer stores — every wave writes 1 KB
//     of whole 16-byte granules (write traffic = algorithmic bytes).
// Real = float: float32 device jobs.  Real = double: float64 device jobs — libsoxr's own VHQ engine is a float64 one
// (SURVEY.md §0.3); the same chain in double2 (LDS 16 bytes per point), results within the method's own floor of the
// float64 direct form (the neglected stop-band aliasing, ~3e-10 for VHQ).  IO = the signal's element type when it
// differs from the arithmetic: <double, float> is float32 I/O on float64 arithmetic — what libsoxr's VHQ recipe itself
// does for float32 clients (reference src/soxr_ext.cpp:74,228) — selected by HIPSOXR_KERNEL_FFT_F64.
// One work item = a pair of blocks of one column: item (col, bx) = blocks 2 bx, 2 bx + 1.  An item beyond its clip's
// last pair (ragged batches) leaves at once.
// Round 5, instruction diet (tools/isa_stats.py; the launch runs at the board's power cap, so instructions are energy):
// the filter values come through a buffer descriptor too (offsets in the scalar operand; which side of the spectrum a
// bin lies on is decided at compile time for all but the one butterfly input that straddles the middle: 97 -> ~50
// vector instructions in front of the first inverse butterfly), and the staging stores test their range per butterfly
// OUTPUT in the scalar unit — only the two outputs that can straddle an end of the kept run compare per lane.
// ---------------------------------------------------------------------------------------------
// Integer samples (IO = int16_t on float arithmetic, int32_t on double: HIPSOXR_KERNEL_FFT_PCM).  Loads widen exactly;
// the output stage is the exact engine's (pcm_out.h): dither keyed by (seed, channel, absolute output index k), round
// half to even, saturate, count.  The value that goes into it must be the one the float kernel stores — that identity is
// what tests/test_gpu_fft_pcm.py holds the engine to — and with contraction allowed that is a matter of code shape:
// a multiply and an add fuse only inside one basic block, so control flow behind a butterfly decides which of its
// last products fuse.  k_fft_pair2 therefore keeps the float kernel's last pass as it is and converts on the way out of
// LDS; k_fft_strided2, which has no staging, converts in the storer (this function), with `v` pinned in its register
// first: a value that is a bare product would otherwise fuse with the dither into one FMA.
// exists: output k is part of the signal — the kernels also convert values past the end of their column, which are
// dropped by the stores' range check and must not count as clips.
template <typename IO, typename Real>
__device__ __forceinline__ IO pcm_stage(Real v, const FftArgs &a, uint32_t ch, int64_t k, bool exists)
{
    static_assert((sizeof(IO) == 2 && sizeof(Real) == 4) || (sizeof(IO) == 4 && sizeof(Real) == 8), "int16 on float32, int32 on float64");
    asm("" : "+v"(v));
    bool clip;
    IO r;
    if constexpr (sizeof(IO) == 2) r = pcm_quantize_i16(v, a.dither != 0, a.seed, ch + a.ch0, k, clip);
    else r = pcm_quantize_i32(v, clip);
    if (clip && exists && a.clip_counter) atomicAdd((unsigned long long *)a.clip_counter, 1ULL);
    return r;
}

template <typename Spec, typename Real, typename IO>
__device__ __forceinline__ void pair2_item(const FftArgs &a, unsigned char *smem_raw, uint32_t col, int64_t bx)
{
    typedef typename PairTabs<Real>::C C;
    typedef typename PairTabs<IO>::V16 V16;
    constexpr int ES = (int)sizeof(IO), EPS = 16 / ES; // element size, elements per 16-byte store
    constexpr int NA = Spec::NA, NB = Spec::NB, NT = Spec::NT, nbA = NA / Spec::RA0;
    constexpr int NsL = NB / Spec::RB2;   // the last inverse pass writes element o + t * NsL, o < NsL
    constexpr int LB = NA > NB ? NA : NB; // complex points of the transform buffer
    C *buf = reinterpret_cast<C *>(smem_raw);
    // integer samples: the run is staged as the arithmetic's own values — up to there the kernel is the float kernel,
    // line for line — and converted on its way out of LDS (the store loop below)
    // float16 / bfloat16 samples (HALF; float arithmetic): the same staging — the kernel is the float32 kernel up to the
    // store loop, which rounds each staged value once to the half type: no dither, no clip count
    constexpr bool PCM = std::is_integral<IO>::value, HALF = is_half_io<IO>::value, CONV = PCM || HALF;
    // lane-pair passes (the one-round block sizes: float arithmetic only) — their float16 / bfloat16 forms take them too:
    // a half job is the float32 job's arithmetic up to the store loop (tests/test_gpu_fft_table_half.py holds them to it)
    constexpr int SPLIT = std::is_same<Real, float>::value ? Spec::SPLIT : 0;
    static_assert(!HALF || std::is_same<Real, float>::value, "float16 / bfloat16 samples: float32 arithmetic");
    typedef typename std::conditional<CONV, Real, IO>::type ST;
    ST *stage = reinterpret_cast<ST *>(smem_raw);
#ifdef FFT2_TRACE
    unsigned long long *g_tr = a.trace ? a.trace + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (NT / 64) + threadIdx.x / 64) * 16 : nullptr;
    int g_tri = 0;
    FFT_STAMP();
#endif

    const uint32_t ch = __builtin_amdgcn_readfirstlane(col % a.n_channels);
    const uint32_t clip = __builtin_amdgcn_readfirstlane(col / a.n_channels);
    const int64_t pa = 2 * bx * a.hop_periods - a.lead_periods; // first period of the pair's first block; the second starts hop_periods later
    const int64_t ina = pa * a.M, outa = pa * a.L;
    const int32_t hop_in = (int32_t)(a.hop_periods * a.M);
    // ragged batch: this clip's own place and length (four scalar loads; the grid spans the longest clip, so a
    // workgroup beyond its clip's last pair has nothing to do)
    int64_t clip_in = (int64_t)clip * a.ics, clip_out = (int64_t)clip * a.ocs, in_frames = a.in_frames, out_frames = a.out_frames;
    if (a.clip_tab) {
        const int64_t *row = a.clip_tab + 4 * (size_t)clip;
        clip_in = row[0]; in_frames = row[1]; clip_out = row[2]; out_frames = row[3];
    }
    if (outa + a.v0 >= out_frames) return;
    const IO *xin = (const IO *)a.in + clip_in + (int64_t)ch * a.ichs;
    auto last_fwd_store = [&](int o, int t, C v) { buf[o + t * (NA / Spec::RA2)] = v; };
    // per-pass twiddle tables (Spec::TABS): one descriptor per transform, the range check over exactly its entries
    auto pass_tabs = [](const float2 *p, int n) {
        if constexpr (Spec::TABS) return PassTabs{__builtin_amdgcn_make_buffer_rsrc(uniform_ptr((void *)p), 0, n * (int)sizeof(float2), 0x00020000)};
        else return NoTabs{};
    };
    const auto twa = pass_tabs(a.TWA, Spec::TWA_N), twb = pass_tabs(a.TWB, Spec::TWB_N);

    // ---- forward: z[n] = x_a[n] + i x_b[n], first pass straight from HBM --------------------------
    if (ina >= a.in_lo) {
        const int64_t left = (in_frames - ina) * ES; // bytes from the first block's first sample to the end of the column
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr((void *)(xin + ina)), 0, __builtin_amdgcn_readfirstlane((int)(left < 0 ? 0 : left > 0x40000000 ? 0x40000000 : left)), 0x00020000);
        Spec::template fwd<SPLIT & 3>(FFT_STAMP_ARGS buf, PairTabs<Real>::wa(a), [&](int j, int t) -> C { // (the butterfly's own offset: one VGPR for all t)
            return C((Real)buf_load_real<IO>(rs, j * ES, t * nbA * ES), (Real)buf_load_real<IO>(rs, j * ES, (t * nbA + hop_in) * ES));
        }, last_fwd_store, (int)threadIdx.x, twa);
    } else { // the first item of a column reaches before its start: explicit zero-extension
        Spec::template fwd<SPLIT & 3>(FFT_STAMP_ARGS buf, PairTabs<Real>::wa(a), [&](int j, int t) -> C {
            const int64_t la = ina + j + t * nbA, lb = la + hop_in;
            return C((la >= a.in_lo && la < in_frames) ? (Real)xin[la] : (Real)0, (lb >= a.in_lo && lb < in_frames) ? (Real)xin[lb] : (Real)0);
        }, last_fwd_store, (int)threadIdx.x, twa);
    }
    // the filter, |frequency| in bins -> real gain, through a descriptor of its own: Hr[0 .. NB/2]
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr((void *)PairTabs<Real>::hr(a)), 0,
                                                                         (NB / 2 + 1) * (int)sizeof(Real), 0x00020000);
    __syncthreads();
    FFT_STAMP();

    // ---- inverse: bin n of the output grid <- bin n or n + NA - NB of the input grid, times (real) H; the last pass
    //      writes into the staging layout.  Input t of butterfly j is bin n = j + t * nbB: bins up to NB/2 are the
    //      non-negative frequencies, the rest the negative ones — for all but one t that is known at compile time.
    const int32_t v0 = a.v0, v1 = a.v0 + a.hop_out, hop_out = a.hop_out;
    IO *ybase = (IO *)a.out + clip_out + (int64_t)ch * a.ochs + (outa + v0); // run[0]; outa + v0 >= 0
    // LDS element index == run index + sh: the 16-byte phases of staging and memory agree
    const int32_t sh = (int32_t)((reinterpret_cast<uintptr_t>(ybase) / ES) & (EPS - 1));
    auto h_load = [&](int j, int t) -> C { return spectrum_load<Spec, Real>(buf, rh, j, t); };
    // Staging stores: output n = o + t * NsL (o < NsL) of both blocks is kept iff v0 <= n < v1.  In every geometry in use
    // the kept run begins inside the first stride of outputs and ends inside the last one (`typical`, wave-uniform):
    // then only outputs t = 0 and t = RB2 - 1 compare per lane, the others are stored as they are.
    const bool typical = v0 >= 0 && v0 <= NsL && v1 >= NB - NsL && v1 <= NB;
    Spec::template inv_staged<(SPLIT >> 2) & 3>(FFT_STAMP_ARGS buf, PairTabs<Real>::wb(a), h_load,
        [&](int o, int t, C w) { // typical geometry
            ST *const sa = stage + (o - v0 + sh) + t * NsL, *const sb = sa + hop_out;
            if (t == 0) { if (o >= v0) { *sa = (ST)w.x; *sb = (ST)w.y; } }
            else if (t == Spec::RB2 - 1) { if (o < v1 - t * NsL) { *sa = (ST)w.x; *sb = (ST)w.y; } }
            else { *sa = (ST)w.x; *sb = (ST)w.y; }
        },
        [&](int o, int t, C w) { // any geometry
            ST *const sa = stage + (o - v0 + sh) + t * NsL, *const sb = sa + hop_out;
            if ((unsigned)(o + t * NsL - v0) < (unsigned)hop_out) { *sa = (ST)w.x; *sb = (ST)w.y; }
        }, !typical, twb);
    __syncthreads();
    FFT_STAMP();

    // ---- store the run: elements [0, valid) of it exist in the column ----------------------------------
    const int64_t remain = out_frames - (outa + v0);
    const int32_t valid = (int32_t)(remain < 0 ? 0 : remain > 2 * (int64_t)hop_out ? 2 * (int64_t)hop_out : remain);
    // Job window (a.out_lo, stream chunks): the column's outputs below out_lo are not this job's — the first run of a
    // chunk begins in the middle of a run and of a 16-byte granule, and the bytes in front of it are the caller's (the
    // previous chunk's result, or somebody else's memory).  Run elements [lo, valid) are the job's.  lo != 0 only in the
    // pair that holds out_lo (the host keeps out_lo < hop_out: the first pair of a launch), which stores its run element
    // by element; every other pair — every pair of a whole-signal job — takes the granule path below as it was
    // (wave-uniform: one scalar branch).
    const int64_t below = a.out_lo - (outa + v0);
    const int32_t lo = (int32_t)(below <= 0 ? 0 : below > valid ? valid : below);
    // 16-byte buffer stores: the descriptor starts at the 16-byte granule that holds run[0] (sh elements before it)
    // and ends with the run, so the hardware range check drops what lies beyond the column (and the trips past the
    // run: no trip count, no branches — every LDS read and every store of the thread is in flight at once).  The
    // first granule's sh leading elements belong to the previous run: that one granule goes element by element.
    if constexpr (!CONV) {
        if (lo != 0) {
            for (int e = lo + (int)threadIdx.x; e < valid; e += NT) ybase[e] = stage[e + sh];
        } else {
            const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr((void *)(ybase - sh)), 0,
                                                                                 __builtin_amdgcn_readfirstlane((valid + sh) * ES), 0x00020000);
            constexpr int QMAX = (2 * (NB - 1) + EPS - 1 + EPS) / EPS; // 2 hop_out < 2 NB elements, + sh
            constexpr int LQ = (int)((size_t)LB * sizeof(C) / 16);     // 16-byte granules of the LDS buffer
            const int tid_out = (int)threadIdx.x;
#pragma unroll
            for (int it = 0; it < (QMAX + NT - 1) / NT; ++it) {
                const int q = tid_out + it * NT;
                const V16 v = *reinterpret_cast<const V16 *>(stage + EPS * (q < LQ ? q : LQ - 1));
                if (q == 0 && sh != 0) {
                    const IO *e = reinterpret_cast<const IO *>(&v);
#pragma unroll
                    for (int c = 0; c < EPS; ++c)
                        if (c >= sh && c - sh < valid) ybase[c - sh] = e[c];
                } else {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, v), ro, q * 16, 0, FFT_STORE_AUX);
                }
            }
        }
    } else {
        // Integer samples: the same granules of the column — EPS staged values (32 bytes of LDS) become one 16-byte store
        // through the exact engine's output stage (pcm_out.h): staged element e is run element e - sh, output
        // outa + v0 + e - sh of the column.  float16 / bfloat16 samples: the same walk with a plain cast for the stage.  Only run elements [0, valid) exist: the others are converted like the rest
        // (whatever the LDS holds there), dropped by the range check, and not counted as clips.
        // 2-byte elements: the range check works on whole dwords, so the descriptor ends with the last WHOLE dword of
        // the run and an odd last element goes out by itself — never half a dword more or less than the run.
        const int run_bytes = ES == 2 ? ((valid + sh) * ES) & ~3 : (valid + sh) * ES;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr((void *)(ybase - sh)), 0,
                                                                             __builtin_amdgcn_readfirstlane(run_bytes), 0x00020000);
        constexpr int QMAX = (2 * (NB - 1) + EPS - 1 + EPS) / EPS;
        constexpr int LQ = (int)((size_t)LB * sizeof(C) / (EPS * sizeof(ST))); // granules' worth of staged values in the LDS buffer
        const int64_t k_run = a.out_abs0 + outa + v0 - sh; // ABSOLUTE output index of staged element 0 (the dither key)
        const bool dither = a.dither != 0;
        const uint32_t dch = ch + a.ch0;
        unsigned nclip = 0;
        auto conv = [&](ST v, int e) -> IO {
            if constexpr (HALF) return (IO)v;
            else {
                bool clip;
                IO r;
                if constexpr (ES == 2) r = pcm_quantize_i16(v, dither, a.seed, dch, k_run + e, clip);
                else r = pcm_quantize_i32(v, clip);
                nclip += (clip && e >= sh + lo && e - sh < valid) ? 1u : 0u; // (only stored elements count)
                return r;
            }
        };
        if (lo != 0) { // the pair that holds the job's lower bound: element by element (see `lo`)
            for (int e = lo + (int)threadIdx.x; e < valid; e += NT) ybase[e] = conv(stage[e + sh], e + sh);
        } else {
            if (ES == 2 && ((valid + sh) & 1) && valid > 0 && threadIdx.x == NT - 1) {
                const unsigned keep = nclip; // (its granule's thread counts it)
                ybase[valid - 1] = conv(stage[valid - 1 + sh], valid - 1 + sh);
                nclip = keep;
            }
            const int tid_out = (int)threadIdx.x;
#pragma unroll
            for (int it = 0; it < (QMAX + NT - 1) / NT; ++it) {
                const int q = tid_out + it * NT;
                const ST *src = stage + EPS * (q < LQ ? q : LQ - 1);
                IO e[EPS];
#pragma unroll
                for (int c = 0; c < EPS; c += 16 / (int)sizeof(ST)) {
                    const typename PairTabs<Real>::V16 v = *reinterpret_cast<const typename PairTabs<Real>::V16 *>(src + c);
                    const ST *pv = reinterpret_cast<const ST *>(&v);
#pragma unroll
                    for (int i = 0; i < 16 / (int)sizeof(ST); ++i) e[c + i] = conv(pv[i], q * EPS + c + i);
                }
                if (q == 0 && sh != 0) {
#pragma unroll
                    for (int c = 0; c < EPS; ++c)
                        if (c >= sh && c - sh < valid) ybase[c - sh] = e[c];
                } else {
                    v4u_t v;
                    __builtin_memcpy(&v, e, 16);
                    __builtin_amdgcn_raw_buffer_store_b128(v, ro, q * 16, 0, FFT_STORE_AUX);
                }
            }
        }
        if constexpr (PCM)
            if (nclip && a.clip_counter) atomicAdd((unsigned long long *)a.clip_counter, (unsigned long long)nclip);
    }
#ifdef FFT2_TRACE
    if (g_tr && (threadIdx.x & 63) == 0) { // where the wave ran: HW_ID (wave/simd/cu/sh/se fields) and the XCC id
        g_tr[13] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        g_tr[14] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
    g_tri = 15;
    FFT_STAMP();
#endif
}

template <typename Spec, typename Real, typename IO = Real>
__global__ void __launch_bounds__(Spec::NT) k_fft_pair2(FftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    pair2_item<Spec, Real, IO>(a, smem_raw, blockIdx.y, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// k_fft_strided2: columns with a frame stride.
// CP = true, CHANNEL-PAIR mode: interleaved data with an even channel count.  The two real signals of a transform are
// the same block of two neighbouring channels — one aligned (Real, Real) word per frame: one 8- or 16-byte raw buffer
// load per element (descriptor over [first frame of the block, end of the column), hardware range check instead of
// per-element bounds code, the per-butterfly offset t*N/R0*frame in the instruction's scalar operand) and one
// range-checked buffer store per kept output.
// CP = false: strided columns that cannot be paired by channel (odd channel counts of interleaved data, a channel slice
// with a frame stride): two consecutive blocks of ONE column are paired, as in k_fft_pair2, each element a 4/8-byte
// buffer load or store at the column's frame stride.
// Workgroup ids are XCD-aware for interleaved data (a.xcd_map): consecutive ids are dealt round-robin to the 8 XCDs,
// each with a private L2, while the channel units of one block of frames share every cache line — so they get ids that
// are congruent mod 8 and adjacent in dispatch order (x = 8 * slot + xcd, slot = chunk * units + unit,
// item = xcd * ceil(items / 8) + chunk).  Without it each line is fetched and (partially) written once per channel unit: 2.3x / 4x
// the algorithmic bytes at 8 channels.  (The derived indices need readfirstlane: a run-time integer division goes
// through the vector ALU, and the compiler then keeps every address in VGPRs.)
// RAGGED batches (a.clip_tab != nullptr, a wave-uniform run-time test as in k_fft_pair2: no further instances): a workgroup
// takes its clip's place and lengths from its row of the table instead of clip * a.ics, clip * a.ocs, a.in_frames and
// a.out_frames; a.in_lo and a.out_lo stay job-wide.  Both descriptors end at the clip's OWN last frame — the hardware range
// check zero-extends past it and drops the stores behind it — and the dither key is the output index within the clip.
// The grid is the longest clip's; the work-item map (fft_ragged_rules.h) runs on the clip's own item count.
// ---------------------------------------------------------------------------------------------
template <typename Real> struct CpIo;
template <> struct CpIo<float> {
    static __device__ __forceinline__ float2 load(__amdgpu_buffer_rsrc_t r, int voff, int soff)
    {
        return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
    }
    static __device__ __forceinline__ void store(float2 v, __amdgpu_buffer_rsrc_t r, int voff)
    {
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u_t, v), r, voff, 0, 0);
    }
};
template <> struct CpIo<double> {
    static __device__ __forceinline__ double2 load(__amdgpu_buffer_rsrc_t r, int voff, int soff)
    {
        return __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
    }
    static __device__ __forceinline__ void store(double2 v, __amdgpu_buffer_rsrc_t r, int voff)
    {
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, v), r, voff, 0, 0);
    }
};

// IO = int16_t (CP only, HIPSOXR_KERNEL_FFT_PCM): the common [frames, 2 c] int16 layout — one aligned 4-byte (l, r) word
// per frame in, the output stage of pcm_stage on both halves and one 4-byte word out.  IO = _Float16 / __bf16 (CP only,
// HIPSOXR_F16 / HIPSOXR_BF16 jobs): the same word, under the same alignment rule, each half rounded once.
template <typename Spec, typename Real, bool CP, typename IO = Real>
__global__ void __launch_bounds__(Spec::NT) k_fft_strided2(FftArgs a)
{
    typedef typename PairTabs<Real>::C C;
    constexpr bool PCM = !std::is_same<IO, Real>::value, HALF = is_half_io<IO>::value; // (PCM: a 2-byte sample type on float arithmetic — int16, or HALF)
    static_assert(!PCM || (CP && (std::is_same<IO, int16_t>::value || HALF) && std::is_same<Real, float>::value), "2-byte samples: int16 / float16 / bfloat16 channel pairs");
    constexpr int ES = (int)sizeof(IO);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    C *cur = reinterpret_cast<C *>(smem_raw);
    constexpr int NA = Spec::NA, NB = Spec::NB, R0 = Spec::RA0, nbA = NA / R0;
#ifdef FFT2_TRACE
    unsigned long long *g_tr = a.trace ? a.trace + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (Spec::NT / 64) + threadIdx.x / 64) * 16 : nullptr;
    int g_tri = 0;
    FFT_STAMP();
#endif
    // XCD-aware ids: x = 8 * slot + xcd, slot = chunk * units + unit;
    // or (a.xcd_map == 0: one column per grid row) items along x, columns along y
    const uint32_t units = CP ? a.n_channels / 2 : a.n_channels;
    const bool xm = a.xcd_map != 0;
    const uint32_t clip = __builtin_amdgcn_readfirstlane(xm ? blockIdx.y : blockIdx.y / units);
    // ragged batch: this clip's own place and lengths — the row convention of pair2_item: {in offset, END of the column as
    // an absolute sample index, out offset, out frames}; four scalar loads at a wave-uniform address — and its own item
    // count (one division per workgroup; the vector ALU does it, so the result goes back to the scalar side)
    int64_t clip_in = (int64_t)clip * a.ics, clip_out = (int64_t)clip * a.ocs, in_frames = a.in_frames, out_frames = a.out_frames;
    int64_t items = a.pairs_per_col;
    if (a.clip_tab) {
        const int64_t *row = a.clip_tab + 4 * (size_t)clip;
        clip_in = row[0]; in_frames = row[1]; clip_out = row[2]; out_frames = row[3];
        items = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)fft_clip_items(out_frames, a.hop_out, CP));
    }
    // ... and each XCD takes a CONTIGUOUS run of the column's blocks (item = xcd * per_xcd + chunk), so that the input two
    // neighbouring blocks share — 17.7 % of a 4410-frame block at 44.1k -> 16k — meets in ONE L2 instead of being fetched
    // from HBM by two (round 4; with item = 8 * chunk + xcd every XCD saw blocks b, b + 8, b + 16 ...: configs[2] HBM
    // traffic 137.3 MB = 1.19x the algorithmic bytes -> 116.0 MB = 1.005x, launch time unchanged: tools/c2_traffic.sh)
    // The map itself is fft_ragged_rules.h (the CPU checks it): grid.x is the longest clip's, padded to a multiple of 8
    // items per unit; an id that is padding, or at or behind this clip's last item, leaves here — before the first
    // barrier, on the id and the row alone
    const FftMapItem mi = xm ? fft_xcd_map(blockIdx.x, units, items) : fft_plain_map(blockIdx.x, blockIdx.y, units, items);
    if (!__builtin_amdgcn_readfirstlane((int)mi.live)) return;
    const uint32_t cu = __builtin_amdgcn_readfirstlane(mi.unit);
    const int64_t bx = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane(mi.item);
    const uint32_t ch = CP ? 2 * cu : cu;
    const int32_t hop_in = (int32_t)(a.hop_periods * a.M), hop_out = a.hop_out;
    const IO *xin = (const IO *)a.in + clip_in + (int64_t)ch * a.ichs;
    const int32_t ifb = (int32_t)a.ifs * ES, ofb = (int32_t)a.ofs * ES; // bytes per frame (launcher: 2 N * frame < 2^30)
    auto last_fwd_store = [&](int o, int t, C v) { cur[o + t * (NA / Spec::RA2)] = v; };
    const int32_t v0 = a.v0, v1 = a.v0 + hop_out;
    const int64_t pa = (CP ? 1 : 2) * bx * a.hop_periods - a.lead_periods; // first period of the (first) block
    const int64_t ina = pa * a.M, outa = pa * a.L;
    // job window (a.out_lo, stream chunks): local outputs below vlo are not the job's and are not stored (v0 for every
    // block but the one that holds out_lo; the host keeps out_lo < hop_out, so of a pair of blocks only the first is cut)
    const int64_t below = a.out_lo - outa;
    const int32_t vlo = (int32_t)(below <= v0 ? v0 : below > v1 ? v1 : below);

    // ---- forward: z[n] = x_c[n] + i x_{c+1}[n]  (CP)  or  x_a[n] + i x_b[n]  (two blocks), first pass straight from HBM
    if (ina >= a.in_lo) {
        const int64_t left = (in_frames - ina) * (int64_t)ifb; // bytes from the block's first frame to the end of the column
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr((void *)(xin + ina * a.ifs)), 0, __builtin_amdgcn_readfirstlane((int)(left < 0 ? 0 : left > 0x40000000 ? 0x40000000 : left)), 0x00020000);
        const int32_t stepb = nbA * ifb; // one butterfly input further: N/R0 frames
        Spec::fwd(FFT_STAMP_ARGS cur, PairTabs<Real>::wa(a), [&](int j, int t) -> C {
            if constexpr (PCM) {
                const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(rs, j * ifb, t * stepb, 0);
                if constexpr (HALF) return C((Real)__builtin_bit_cast(IO, (uint16_t)(w & 0xffffu)), (Real)__builtin_bit_cast(IO, (uint16_t)(w >> 16)));
                else return C((Real)(int16_t)(w & 0xffffu), (Real)(int16_t)(w >> 16));
            } else if constexpr (CP) return CpIo<Real>::load(rs, j * ifb, t * stepb);
            else return C(buf_load_real<Real>(rs, j * ifb, t * stepb), buf_load_real<Real>(rs, j * ifb, t * stepb + hop_in * ifb));
        }, last_fwd_store);
    } else { // the first block of a column reaches before its start: explicit zero-extension
        Spec::fwd(FFT_STAMP_ARGS cur, PairTabs<Real>::wa(a), [&](int j, int t) -> C {
            const int64_t l = ina + j + t * nbA, lb = l + hop_in;
            if constexpr (CP) {
                C v = C((Real)0, (Real)0);
                if (l >= a.in_lo && l < in_frames) v = C((Real)xin[l * a.ifs], (Real)xin[l * a.ifs + 1]);
                return v;
            } else {
                return C((l >= a.in_lo && l < in_frames) ? xin[l * a.ifs] : (Real)0, (lb >= a.in_lo && lb < in_frames) ? xin[lb * a.ifs] : (Real)0);
            }
        }, last_fwd_store);
    }
    __syncthreads();
    FFT_STAMP();

    // ---- inverse (see k_fft_pair2), outputs straight to HBM -----------------------------------------
    IO *ybase = (IO *)a.out + clip_out + (int64_t)ch * a.ochs + (outa + v0) * a.ofs; // outa + v0 >= 0
    const int64_t oleft = (out_frames - (outa + v0)) * (int64_t)ofb;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr((void *)ybase), 0, __builtin_amdgcn_readfirstlane((int)(oleft < 0 ? 0 : oleft > 0x40000000 ? 0x40000000 : oleft)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr((void *)PairTabs<Real>::hr(a)), 0,
                                                                         (NB / 2 + 1) * (int)sizeof(Real), 0x00020000);
    auto h_load = [&](int j, int t) -> C { return spectrum_load<Spec, Real>(cur, rh, j, t); };
    Spec::inv(FFT_STAMP_ARGS cur, PairTabs<Real>::wb(a), h_load, [&](int o, int t, C wv) {
        const int n = o + t * (NB / Spec::RB2);
        if (n >= (CP ? vlo : v0) && n < v1) {
            if constexpr (HALF) { // one rounding per half, one 4-byte word out (`v` pinned first, as pcm_stage does)
                float l = wv.x, r = wv.y;
                asm("" : "+v"(l));
                asm("" : "+v"(r));
                __builtin_amdgcn_raw_buffer_store_b32((unsigned)half_bits<IO>(l) | ((unsigned)half_bits<IO>(r) << 16), ro, (n - v0) * ofb, 0, 0);
            } else if constexpr (PCM) {
                const int64_t k = outa + n; // (>= 0: n >= v0); the dither key is the ABSOLUTE index
                const uint16_t l = (uint16_t)pcm_stage<IO>(wv.x, a, ch, a.out_abs0 + k, k < out_frames), r = (uint16_t)pcm_stage<IO>(wv.y, a, ch + 1, a.out_abs0 + k, k < out_frames);
                __builtin_amdgcn_raw_buffer_store_b32((unsigned)l | ((unsigned)r << 16), ro, (n - v0) * ofb, 0, 0);
            } else if constexpr (CP) {
                CpIo<Real>::store(wv, ro, (n - v0) * ofb); // frame outa + n holds (y_c, y_{c+1})
            } else {
                if (n >= vlo) buf_store_real(wv.x, ro, (n - v0) * ofb); // block a
                buf_store_real(wv.y, ro, (n - v0 + hop_out) * ofb);   // block b: hop_out frames further
            }
        }
    });
#ifdef FFT2_TRACE
    if (g_tr && (threadIdx.x & 63) == 0) { g_tr[13] = __builtin_amdgcn_s_getreg((31 << 11) | 4); g_tr[14] = __builtin_amdgcn_s_getreg((31 << 11) | 20); }
    g_tri = 15;
    FFT_STAMP();
#endif
}

// ---------------------------------------------------------------------------------------------
// Three translation units.  Every schedule of the table below is 7 kernels (k_fft_pair2 in float32, float64 and
// float32-on-float64, k_fft_strided2 x 2 in float32 and float64); compiled in one piece they are the build's critical
// path.  build.sh compiles this file three times: -DFFT_PART=0 = everything except the kernels of the schedules listed
// here (declared extern), -DFFT_PART=1 / =2 = the templates above plus exactly the kernels of one of the two lists, no
// host code (=3 / =4: the integer-sample kernels of the same lists, =5: the float32-only block sizes of one-round jobs,
// below; =6 / =7: the float16 / bfloat16 kernels of the two lists, =8: those of the table's other rows and of the
// one-round block sizes).  Without FFT_PART: one piece.
// ---------------------------------------------------------------------------------------------
#define HIPSOXR_PART1_SPECS(X) X(4096, 2048, 256) X(2048, 4096, 256) X(2048, 1024, 256) X(1024, 2048, 256) X(5376, 1792, 384) X(1792, 5376, 384) X(5376, 3584, 384) X(3584, 5376, 384) X(2688, 896, 384) X(896, 2688, 384) X(2688, 1792, 384) X(1792, 2688, 384) X(5120, 1280, 320) X(1280, 5120, 320) X(5376, 896, 384) X(896, 5376, 384)
#define HIPSOXR_PART2_SPECS(X) X(7056, 5120, 448) X(5120, 7056, 448) X(4704, 2560, 384) X(2560, 4704, 384) X(5120, 2352, 384) X(2352, 5120, 384) X(7056, 1280, 448) X(1280, 7056, 448) X(5120, 1176, 320) X(1176, 5120, 320) X(3528, 5120, 384) X(5120, 3528, 384) X(4704, 1280, 384) X(1280, 4704, 384) X(3840, 5120, 384) X(5120, 3840, 384)
#define HIPSOXR_INST(NA, NB, NT)                                                                        \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float>(FftArgs);             \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, double>(FftArgs);            \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, double, float>(FftArgs);     \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, float, true>(FftArgs);    \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, double, true>(FftArgs);   \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, float, false>(FftArgs);   \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, double, false>(FftArgs);
// ... and three more for integer samples (HIPSOXR_KERNEL_FFT_PCM): units of their own, FFT_PART=3 / =4, over the same
// two lists — shorter than the float units, so the parallel build's longest unit stays what it was
#define HIPSOXR_INST_PCM(NA, NB, NT)                                                                             \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float, int16_t>(FftArgs);             \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, double, int32_t>(FftArgs);            \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, float, true, int16_t>(FftArgs);
// ... and four more for float16 / bfloat16 samples (HIPSOXR_F16 / HIPSOXR_BF16): units of their own again, FFT_PART=6 / =7,
// over the same two lists, float arithmetic only
#define HIPSOXR_INST_HALF(NA, NB, NT)                                                                            \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float, _Float16>(FftArgs);            \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float, __bf16>(FftArgs);              \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, float, true, _Float16>(FftArgs);   \
    HIPSOXR_EXTERN template __global__ void k_fft_strided2<PairOf<NA, NB, NT>, float, true, __bf16>(FftArgs);
// ... and ONE for the block sizes that exist for one-round float32 jobs only (48k <-> 44.1k at 14 and 20 periods, see
// "one-round jobs" below): unit-stride float32 columns, nothing else — a unit of its own, FFT_PART=5, four kernels.
// Threads: the largest butterfly count of any pass is 294 (2058 = 21*14*7: 98 / 147 / 294; 2240: 140 / 160 / 224) and
// 320 (3200 = 16*20*10: 200 / 160 / 320; 2940: 140 / 210 / 294) — five waves.
#ifndef FFT_ONE_ROUND_NT
#define FFT_ONE_ROUND_NT 320
#endif
#define HIPSOXR_PART5_SPECS(X) X(2240, 2058, FFT_ONE_ROUND_NT) X(2058, 2240, FFT_ONE_ROUND_NT) X(3200, 2940, FFT_ONE_ROUND_NT) X(2940, 3200, FFT_ONE_ROUND_NT)
#define HIPSOXR_INST_F32(NA, NB, NT) HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float>(FftArgs);
// The rows of the table that are in neither list (their float and integer kernels are instantiated where the table names
// them, in unit 0): the float16 / bfloat16 forms of those go into unit FFT_PART=8 ...
#define HIPSOXR_PART8_SPECS(X) X(5120, 4704, 384) X(4704, 5120, 384) X(2560, 2352, 384) X(2352, 2560, 384) X(1280, 1176, 256) X(1176, 1280, 256) X(7056, 2560, 448) X(2560, 7056, 448) X(4410, 1600, 320) X(1600, 4410, 320)
// ... together with those of the one-round block sizes (a half job takes the row the float32 job takes)
#define HIPSOXR_INST_F32_HALF(NA, NB, NT)                                                                \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float, _Float16>(FftArgs);    \
    HIPSOXR_EXTERN template __global__ void k_fft_pair2<PairOf<NA, NB, NT>, float, __bf16>(FftArgs);
#if defined(FFT_PART) && FFT_PART == 0
#define HIPSOXR_EXTERN extern
HIPSOXR_PART1_SPECS(HIPSOXR_INST)
HIPSOXR_PART2_SPECS(HIPSOXR_INST)
HIPSOXR_PART1_SPECS(HIPSOXR_INST_PCM)
HIPSOXR_PART2_SPECS(HIPSOXR_INST_PCM)
HIPSOXR_PART5_SPECS(HIPSOXR_INST_F32)
HIPSOXR_PART1_SPECS(HIPSOXR_INST_HALF)
HIPSOXR_PART2_SPECS(HIPSOXR_INST_HALF)
HIPSOXR_PART8_SPECS(HIPSOXR_INST_HALF)
HIPSOXR_PART5_SPECS(HIPSOXR_INST_F32_HALF)
#elif defined(FFT_PART) && FFT_PART == 1
#define HIPSOXR_EXTERN
HIPSOXR_PART1_SPECS(HIPSOXR_INST)
#elif defined(FFT_PART) && FFT_PART == 2
#define HIPSOXR_EXTERN
HIPSOXR_PART2_SPECS(HIPSOXR_INST)
#elif defined(FFT_PART) && FFT_PART == 3
#define HIPSOXR_EXTERN
HIPSOXR_PART1_SPECS(HIPSOXR_INST_PCM)
#elif defined(FFT_PART) && FFT_PART == 4
#define HIPSOXR_EXTERN
HIPSOXR_PART2_SPECS(HIPSOXR_INST_PCM)
#elif defined(FFT_PART) && FFT_PART == 5
#define HIPSOXR_EXTERN
HIPSOXR_PART5_SPECS(HIPSOXR_INST_F32)
#elif defined(FFT_PART) && FFT_PART == 6
#define HIPSOXR_EXTERN
HIPSOXR_PART1_SPECS(HIPSOXR_INST_HALF)
#elif defined(FFT_PART) && FFT_PART == 7
#define HIPSOXR_EXTERN
HIPSOXR_PART2_SPECS(HIPSOXR_INST_HALF)
#elif defined(FFT_PART) && FFT_PART == 8
#define HIPSOXR_EXTERN
HIPSOXR_PART8_SPECS(HIPSOXR_INST_HALF)
HIPSOXR_PART5_SPECS(HIPSOXR_INST_F32_HALF)
#endif

#if !defined(FFT_PART) || FFT_PART == 0
// ---------------------------------------------------------------------------------------------
// host: geometry, tables
// ---------------------------------------------------------------------------------------------
struct FftGeom {
    bool ok = false;
    int k = 0;
    int32_t N_in = 0, N_out = 0, A = 0, B = 0;
    int32_t radA[8] = {1, 1, 1, 1, 1, 1, 1, 1}, radB[8] = {1, 1, 1, 1, 1, 1, 1, 1}, nA = 0, nB = 0; // (plain arrays: the cached geometry is copied per launch)
    int32_t lead_periods = 0, hop_periods = 0, v0 = 0, hop_out = 0;
    size_t lds_bytes = 0;
    float2 *dev = nullptr; // the float32 tables, laid out as fft_tabs says, then the per-pass tables
    size_t twa = 0, twb = 0; // per-pass twiddle tables of the one-round kernels: their places in `dev` (0: none)
    double2 *devd = nullptr; // float64 instance of the paired kernel: WA2d, WB2d, Hrd (fft_tabs)
};

static bool factor_radices(int n, std::vector<int> &rad)
{
    rad.clear();
    int twos = 0;
    while (n % 2 == 0) { n /= 2; ++twos; }
    for (int pr : {7, 5, 3})
        while (n % pr == 0) { n /= pr; rad.push_back(pr); }
    if (n != 1) return false;
    while (twos >= 4) { rad.push_back(16); twos -= 4; }
    if (twos == 3) rad.push_back(8);
    else if (twos == 2) rad.push_back(4);
    else if (twos == 1) rad.push_back(2);
    // small radices first keeps the early (small-Ns) passes cheap in LDS bank conflicts
    std::sort(rad.begin(), rad.end());
    return rad.size() <= 8 && !rad.empty();
}

static std::mutex g_fft_mu;
static std::vector<std::pair<std::pair<const Plan *, int>, FftGeom>> g_fft; // key: (plan, geometry variant)

void fft_release(const Plan *p)
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    for (size_t i = 0; i < g_fft.size();)
        if (g_fft[i].first.first == p) {
            if (g_fft[i].second.dev) (void)hipFree(g_fft[i].second.dev);
            if (g_fft[i].second.devd) (void)hipFree(g_fft[i].second.devd);
            g_fft.erase(g_fft.begin() + i);
        } else ++i;
}

// Where each table lies in FftGeom::dev (float2 units; Hr: B + 1 floats) and FftGeom::devd (double2 units; Hrd: B + 1
// doubles): fft_build fills through it, fft_args_geom points through it.  Per-pass tables follow behind `n` (twa / twb).
struct FftTabs {
    size_t WA, WB, P, Q, Hs, WA2, WB2, Hr, n; // dev
    size_t WA2d, WB2d, Hrd, nd;               // devd
};
static FftTabs fft_tabs(const FftGeom &g)
{
    FftTabs t;
    const size_t A = (size_t)g.A, B = (size_t)g.B, h = (B + 2) / 2 + 1; // (h: B + 1 real values in complex units, rounded up)
    t.WA = 0; t.WB = t.WA + A; t.P = t.WB + B; t.Q = t.P + (A + 1); t.Hs = t.Q + B;
    t.WA2 = t.Hs + (B + 1); t.WB2 = t.WA2 + (size_t)g.N_in; t.Hr = t.WB2 + (size_t)g.N_out; t.n = t.Hr + h;
    t.WA2d = 0; t.WB2d = t.WA2d + (size_t)g.N_in; t.Hrd = t.WB2d + (size_t)g.N_out; t.nd = t.Hrd + h;
    return t;
}

// The kept run of a block of k periods.  A block discards ceil((T/2+2) L/M) outputs at either end — the filter support
// [n_k, n_k + T) of a kept output lies inside the block — in whole periods at its front (lead_periods: a function of the
// plan alone, the same for every block size of a ratio), and keeps a whole number of periods (hop_periods).  False: no
// period is kept — or, with need_half, fewer than half of the block's outputs are (long filters on short blocks).
struct KeptRun { int32_t lead_periods = 0, hop_periods = 0; };
static bool fft_kept_run(const Plan &p, int64_t k, bool need_half, KeptRun *r)
{
    const int64_t disc = ((int64_t)(p.T / 2 + 2) * p.L + p.M - 1) / p.M;
    r->lead_periods = (int32_t)((disc + p.L - 1) / p.L);
    r->hop_periods = (int32_t)((k * p.L - disc - (int64_t)r->lead_periods * p.L) / p.L);
    if (r->hop_periods < 1) return false;
    return !need_half || 2 * (int64_t)r->hop_periods * p.L >= k * p.L;
}
// Outputs a block of k periods keeps (fft_geometry's hop_out for a forced k, arithmetic only); 0: no such block.
// (The half-kept refusal holds here whatever the caller: this is asked about forced block sizes alone.)
static int64_t fft_hop_out(const Plan &p, int k)
{
    KeptRun r;
    return fft_kept_run(p, k, true, &r) ? (int64_t)r.hop_periods * p.L : 0;
}

// Block geometry (arithmetic only; fft_build adds the device tables).  False: no admissible block.
static bool fft_geometry(const Plan &p, FftGeom &g, bool small, int force_k)
{
    const int64_t L = p.L, M = p.M;
    const int32_t T = p.T;
    if (p.q.bits == 0.) return false; // QQ: not worth a transform
    // block of k periods: candidates are power-of-two k with 7-smooth even half-lengths; take the largest block whose
    // transforms stay <= 2600 points (one 20 KB LDS buffer, least overlap waste), else the smallest admissible one
    for (int k = force_k ? force_k : 1; k <= (force_k ? force_k : 4096); k *= 2) {
        const int64_t Nin = M * k, Nout = L * k;
        if ((Nin % 2 || Nout % 2) && !force_k) continue; // (the half-length tables of k_fft_block; the paired kernels take odd lengths)
        if (!force_k && Nin < 6 * (int64_t)T) continue;
        if (Nin / 2 > 4096 || Nout / 2 > 4096) break;
        std::vector<int> ra, rb;
        if (!factor_radices((int)(Nin / 2), ra) || !factor_radices((int)(Nout / 2), rb)) {
            if (!force_k) continue;
            ra.clear(); rb.clear(); // (k_fft_block's run-time schedule of the half lengths: a forced geometry belongs to a paired kernel, which has its own)
        }
        if (!force_k && g.k && (small || std::max(Nin, Nout) / 2 > 2600)) break;
        g.k = k; g.N_in = (int32_t)Nin; g.N_out = (int32_t)Nout; g.A = g.N_in / 2; g.B = g.N_out / 2;
        g.nA = (int32_t)ra.size(); g.nB = (int32_t)rb.size();
        for (int i = 0; i < 8; ++i) { g.radA[i] = i < g.nA ? ra[i] : 1; g.radB[i] = i < g.nB ? rb[i] : 1; }
    }
    if (!g.k) return false;
    // a block must keep a worthwhile share of its outputs — asked of a FORCED block size only: the search above takes
    // what it finds
    KeptRun r;
    if (!fft_kept_run(p, g.k, force_k != 0, &r)) return false;
    g.lead_periods = r.lead_periods; g.hop_periods = r.hop_periods;
    g.v0 = (int32_t)(g.lead_periods * L);
    g.hop_out = (int32_t)(g.hop_periods * L);
    g.lds_bytes = (size_t)(std::max(g.A, g.B) + 8) * sizeof(float2);
    return g.lds_bytes <= 150 * 1024;
}

// Per-pass twiddle tables of a length with a Sched<N>::TABS schedule (the one-round float32 kernels): for pass 2 and
// pass 3 every factor exp(sign 2 pi i t k / (Ns R)) a butterfly applies, laid out [t][k] (t = 1 .. R - 1, k < Ns) —
// computed in double and rounded ONCE, where the kernels of the other lengths form w^t from one or two rounded entries.
// False: N has no such schedule.
static bool pass_tables(int N, int sign, std::vector<float2> *tw)
{
    int r[3] = {0, 0, 0};
#define HIPSOXR_SCHED(n, r0, r1, r2, swz) if (N == n) { r[0] = r0; r[1] = r1; r[2] = r2; }
    HIPSOXR_SCHED_TABS_LIST(HIPSOXR_SCHED)
#undef HIPSOXR_SCHED
    if (!r[0]) return false;
    const double PI2 = 6.283185307179586476925286766559;
    tw->clear();
    for (int pass = 1, Ns = r[0]; pass < 3; Ns *= r[pass], ++pass)
        for (int t = 1; t < r[pass]; ++t)
            for (int k = 0; k < Ns; ++k) {
                const double ang = PI2 * (double)(t * k) / (double)(Ns * r[pass]);
                tw->push_back(make_float2((float)std::cos(ang), (float)(sign * std::sin(ang))));
            }
    return true;
}

// w[m] = exp(sign 2 pi i m / N), m < n: computed in double, rounded once to the table's type
template <typename C>
static void fill_twiddles(C *w, int n, int N, int sign)
{
    typedef decltype(w->x) T;
    const double PI2 = 6.283185307179586476925286766559;
    for (int m = 0; m < n; ++m) { w[m].x = (T)std::cos(PI2 * m / N); w[m].y = (T)(sign * std::sin(PI2 * m / N)); }
}

static const char *fft_build(const Plan &p, FftGeom *out, bool small, int force_k = 0)
{
    FftGeom g;
    if (!fft_geometry(p, g, small, force_k)) { *out = g; return nullptr; }
    const int64_t L = p.L;
    const int32_t T = p.T;
    const int A = g.A, B = g.B;
    const FftTabs at = fft_tabs(g);
    std::vector<float2> tab(at.n);
    std::vector<float2> twa, twb;
    if (pass_tables(g.N_in, -1, &twa) && pass_tables(g.N_out, +1, &twb)) { // (behind everything else: 16-byte aligned or not, the loads are 8 bytes)
        g.twa = tab.size(); g.twb = g.twa + twa.size();
        tab.resize(g.twb + twb.size());
    } else {
        // one length alone has a table schedule (k_fft_block at N_in = 3200, say, beside any N_out but 2940): no per-pass
        // tables — `twa`, filled by the first call, must not reach the copy below, which would lay it over WA and WB at g.twa = 0
        twa.clear(); twb.clear();
    }
    float2 *Hs = tab.data() + at.Hs;
    float *Hr = reinterpret_cast<float *>(tab.data() + at.Hr);
    fill_twiddles(tab.data() + at.WA2, g.N_in, g.N_in, -1);
    fill_twiddles(tab.data() + at.WB2, g.N_out, g.N_out, +1);
    fill_twiddles(tab.data() + at.WA, A, A, -1);
    fill_twiddles(tab.data() + at.WB, B, B, +1);
    fill_twiddles(tab.data() + at.P, A + 1, g.N_in, -1);
    fill_twiddles(tab.data() + at.Q, B, g.N_out, +1);
    // H[q] = sum_p sum_j bank[p][j] exp(-2 pi i q (L*(T/2-1-j) + p) / (L*N_in)), scaled by 1/(N_in*L)
    const double PI2 = 6.283185307179586476925286766559;
    const double scale = 1.0 / ((double)g.N_in * (double)L);
    const int qmax = std::min(A, B);
    std::vector<double2> td(at.nd); // the float64 instance's tables (small: N_in + N_out + B/2 double2)
    double *Hrd = reinterpret_cast<double *>(td.data() + at.Hrd); // Re H in float64
    for (int q = 0; q <= B; ++q) {
        if (q > qmax) { Hs[q] = make_float2(0.f, 0.f); continue; }
        double hr = 0., hi = 0.;
        const double wj = PI2 * (double)q / (double)g.N_in; // per tap j the angle grows by +wj
        const double cwj = std::cos(wj), swj = std::sin(wj);
        for (int64_t ph = 0; ph < L; ++ph) {
            // angle for j = 0: -2 pi q (L*(T/2-1) + ph) / (L*N_in)
            const double a0 = -PI2 * (double)q * ((double)(L * (int64_t)(T / 2 - 1) + ph)) / ((double)L * g.N_in);
            double cr = std::cos(a0), ci = std::sin(a0);
            const double *b = p.bank.data() + (size_t)(ph * T);
            for (int j = 0; j < T; ++j) {
                hr += b[j] * cr; hi += b[j] * ci;
                const double nr = cr * cwj - ci * swj; ci = cr * swj + ci * cwj; cr = nr;
            }
        }
        Hs[q] = make_float2((float)(hr * scale), (float)(hi * scale));
        // The prototype is symmetric about the output instant (zero latency) and blocks are cut on period
        // boundaries, so H is real: |Im H| <= 2e-13 |Re H| in the pass band (the one unpaired sample of the
        // even-length support, g[-L T/2], is a window-edge value ~1e-11).  The paired kernels use Re H alone:
        // half the table reads and a real x complex product per bin.
        Hr[q] = (float)(hr * scale);
        Hrd[q] = hr * scale;
    }
    std::copy(twa.begin(), twa.end(), tab.begin() + g.twa);
    std::copy(twb.begin(), twb.end(), tab.begin() + g.twb);
    HIP_TRY(hipMalloc((void **)&g.dev, tab.size() * sizeof(float2)));
    HIP_TRY(hipMemcpy(g.dev, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
    fill_twiddles(td.data() + at.WA2d, g.N_in, g.N_in, -1);
    fill_twiddles(td.data() + at.WB2d, g.N_out, g.N_out, +1);
    HIP_TRY(hipMalloc((void **)&g.devd, td.size() * sizeof(double2)));
    HIP_TRY(hipMemcpy(g.devd, td.data(), td.size() * sizeof(double2), hipMemcpyHostToDevice));
    g.ok = true;
    *out = g;
    return nullptr;
}

// geometry cache, key (plan, variant): 0 = default search, 1 = small-block search, 2 + i = forced k of row i of fft_pairs,
// 1000 + k = k_fft_wave's forced k
static const char *fft_geom_cached(Plan *p, int variant, int force_k, FftGeom *g)
{
    std::lock_guard<std::mutex> lk(g_fft_mu);
    for (auto &e : g_fft)
        if (e.first.first == p && e.first.second == variant) { *g = e.second; return nullptr; }
    if (const char *err = fft_build(*p, g, variant == 1, force_k)) return err;
    g_fft.push_back({{p, variant}, *g});
    return nullptr;
}

// ---- paired-block kernels: compile-time schedules for the common ratios -------------------
struct PairEntry {
    int64_t L, M; int k; int small; /* 0: full-size blocks, 1: half-size (small jobs), 2: quarter-size (smaller still), 3: one-round float32 jobs only (kern2 alone) */
    unsigned nt;
    void (*kern2)(FftArgs); void (*kern2d)(FftArgs); // unit-stride columns, float32 / float64
    void (*kern2fd)(FftArgs);                        // float32 I/O on float64 arithmetic (HIPSOXR_KERNEL_FFT_F64)
    void (*kcp)(FftArgs); void (*kcpd)(FftArgs);     // channel-pair mode (interleaved data), float32 / float64
    void (*kst)(FftArgs); void (*kstd)(FftArgs);     // strided columns, two blocks per transform
    void (*kern2i16)(FftArgs); void (*kern2i32)(FftArgs); // integer samples (HIPSOXR_KERNEL_FFT_PCM): unit-stride columns,
    void (*kcpi16)(FftArgs);                         // int16 on float32 / int32 on float64 arithmetic; int16 channel pairs
};
#define HIPSOXR_PAIR(L, M, k, small, NA, NB, NT) \
    {L, M, k, small, NT, k_fft_pair2<PairOf<NA, NB, NT>, float>, k_fft_pair2<PairOf<NA, NB, NT>, double>, \
     k_fft_pair2<PairOf<NA, NB, NT>, double, float>, \
     k_fft_strided2<PairOf<NA, NB, NT>, float, true>, k_fft_strided2<PairOf<NA, NB, NT>, double, true>, \
     k_fft_strided2<PairOf<NA, NB, NT>, float, false>, k_fft_strided2<PairOf<NA, NB, NT>, double, false>, \
     k_fft_pair2<PairOf<NA, NB, NT>, float, int16_t>, k_fft_pair2<PairOf<NA, NB, NT>, double, int32_t>, \
     k_fft_strided2<PairOf<NA, NB, NT>, float, true, int16_t>}
// ... float32 unit-stride columns only: every other pointer null (taken by the one-round rule, fft_one_round_pick, alone)
#define HIPSOXR_PAIR_F32(L, M, k, NA, NB) \
    {L, M, k, 3, FFT_ONE_ROUND_NT, k_fft_pair2<PairOf<NA, NB, FFT_ONE_ROUND_NT>, float>, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}
static const PairEntry *fft_pairs(int *n)
{
    static const PairEntry pairs[] = {
        // L, M (out/in = L/M), periods per block, small-job variant, N_in, N_out, threads
        HIPSOXR_PAIR(147, 160, 32, false, 5120, 4704, 384), HIPSOXR_PAIR(147, 160, 16, true, 2560, 2352, 384),   // 48k -> 44.1k
        HIPSOXR_PAIR(160, 147, 32, false, 4704, 5120, 384), HIPSOXR_PAIR(160, 147, 16, true, 2352, 2560, 384),   // 44.1k -> 48k
        HIPSOXR_PAIR(147, 160, 8, 2, 1280, 1176, 256), HIPSOXR_PAIR(160, 147, 8, 2, 1176, 1280, 256),           // ... quarter-size blocks: jobs of a few hundred pairs
        HIPSOXR_PAIR_F32(147, 160, 14, 2240, 2058), HIPSOXR_PAIR_F32(160, 147, 14, 2058, 2240),                 // ... 14 and 20 periods: block sizes between those three for
        HIPSOXR_PAIR_F32(147, 160, 20, 3200, 2940), HIPSOXR_PAIR_F32(160, 147, 20, 2940, 3200),                 //     float32 jobs that run as ONE round of co-resident workgroups
        HIPSOXR_PAIR(160, 441, 16, false, 7056, 2560, 448), HIPSOXR_PAIR(441, 160, 16, false, 2560, 7056, 448),  // 44.1k <-> 16k
        HIPSOXR_PAIR(160, 441, 10, true, 4410, 1600, 320), HIPSOXR_PAIR(441, 160, 10, true, 1600, 4410, 320),    // ... 35 KB blocks: 4 workgroups per CU
        HIPSOXR_PAIR(1, 2, 2048, false, 4096, 2048, 256), HIPSOXR_PAIR(2, 1, 2048, false, 2048, 4096, 256),      // 2:1, 1:2
        HIPSOXR_PAIR(1, 2, 1024, true, 2048, 1024, 256), HIPSOXR_PAIR(2, 1, 1024, true, 1024, 2048, 256),        // ... half-size blocks: small jobs (10 s mono 7.5 -> 6.6 us), float64
        HIPSOXR_PAIR(1, 3, 1792, false, 5376, 1792, 384), HIPSOXR_PAIR(3, 1, 1792, false, 1792, 5376, 384),      // 48k <-> 16k
        HIPSOXR_PAIR(2, 3, 1792, false, 5376, 3584, 384), HIPSOXR_PAIR(3, 2, 1792, false, 3584, 5376, 384),      // 48k <-> 32k
        HIPSOXR_PAIR(1, 3, 896, true, 2688, 896, 384), HIPSOXR_PAIR(3, 1, 896, true, 896, 2688, 384),            // ... half-size blocks for both:
        HIPSOXR_PAIR(2, 3, 896, true, 2688, 1792, 384), HIPSOXR_PAIR(3, 2, 896, true, 1792, 2688, 384),          //     small jobs, float64
        HIPSOXR_PAIR(1, 4, 1280, false, 5120, 1280, 320), HIPSOXR_PAIR(4, 1, 1280, false, 1280, 5120, 320),      // 4:1, 1:4
        HIPSOXR_PAIR(1, 6, 896, false, 5376, 896, 384), HIPSOXR_PAIR(6, 1, 896, false, 896, 5376, 384),          // 48k <-> 8k
        HIPSOXR_PAIR(320, 441, 16, false, 7056, 5120, 448), HIPSOXR_PAIR(441, 320, 16, false, 5120, 7056, 448),  // 44.1k <-> 32k
        HIPSOXR_PAIR(80, 147, 32, false, 4704, 2560, 384), HIPSOXR_PAIR(147, 80, 32, false, 2560, 4704, 384),    // 88.2k <-> 48k
        HIPSOXR_PAIR(147, 320, 16, false, 5120, 2352, 384), HIPSOXR_PAIR(320, 147, 16, false, 2352, 5120, 384),  // 96k <-> 44.1k
        HIPSOXR_PAIR(80, 441, 16, false, 7056, 1280, 448), HIPSOXR_PAIR(441, 80, 16, false, 1280, 7056, 448),    // 44.1k <-> 8k
        HIPSOXR_PAIR(147, 640, 8, false, 5120, 1176, 320), HIPSOXR_PAIR(640, 147, 8, false, 1176, 5120, 320),    // 192k <-> 44.1k
        HIPSOXR_PAIR(640, 441, 8, false, 3528, 5120, 384), HIPSOXR_PAIR(441, 640, 8, false, 5120, 3528, 384),    // 22.05k <-> 32k, 11.025k <-> 16k
        HIPSOXR_PAIR(40, 147, 32, false, 4704, 1280, 384), HIPSOXR_PAIR(147, 40, 32, false, 1280, 4704, 384),    // 44.1k <-> 12k, 88.2k <-> 24k
        HIPSOXR_PAIR(4, 3, 1280, false, 3840, 5120, 384), HIPSOXR_PAIR(3, 4, 1280, false, 5120, 3840, 384),      // 24k <-> 32k, 12k <-> 16k, 48k <-> 64k
    };
    *n = (int)(sizeof pairs / sizeof pairs[0]);
    return pairs;
}
#undef HIPSOXR_PAIR
#undef HIPSOXR_PAIR_F32

// The float16 / bfloat16 forms of a row (HIPSOXR_F16 / HIPSOXR_BF16 jobs; float32 arithmetic): a table of its own, keyed by
// the row's transform lengths and thread count and written from the instantiation lists — every row that has a `kern2` has
// both unit-stride forms, every row that has a `kcp` both channel-pair forms (tests/test_half_host.py holds the lists to it).
struct HalfKernels { int NA, NB; unsigned nt; void (*kern2h)(FftArgs); void (*kern2bf)(FftArgs); void (*kcph)(FftArgs); void (*kcpbf)(FftArgs); };
#define HIPSOXR_HALF_ROW(NA, NB, NT) \
    {NA, NB, NT, k_fft_pair2<PairOf<NA, NB, NT>, float, _Float16>, k_fft_pair2<PairOf<NA, NB, NT>, float, __bf16>, \
     k_fft_strided2<PairOf<NA, NB, NT>, float, true, _Float16>, k_fft_strided2<PairOf<NA, NB, NT>, float, true, __bf16>},
#define HIPSOXR_HALF_ROW_F32(NA, NB, NT) \
    {NA, NB, NT, k_fft_pair2<PairOf<NA, NB, NT>, float, _Float16>, k_fft_pair2<PairOf<NA, NB, NT>, float, __bf16>, nullptr, nullptr},
static const HalfKernels *fft_half_kernels(const PairEntry &e)
{
    static const HalfKernels halves[] = {
        HIPSOXR_PART1_SPECS(HIPSOXR_HALF_ROW) HIPSOXR_PART2_SPECS(HIPSOXR_HALF_ROW) HIPSOXR_PART8_SPECS(HIPSOXR_HALF_ROW)
        HIPSOXR_PART5_SPECS(HIPSOXR_HALF_ROW_F32)
    };
    for (const HalfKernels &h : halves)
        if (h.NA == e.M * e.k && h.NB == e.L * e.k && h.nt == e.nt) return &h;
    return nullptr;
}
#undef HIPSOXR_HALF_ROW
#undef HIPSOXR_HALF_ROW_F32

// ---- one-round jobs: block size by per-CU load ------------------------------------------------------------
// A float32 job of unit-stride columns below the throughput rule's size (a clip of 20 s to a few minutes, a few
// channels) is ONE round: every workgroup is resident from the start, and the launch ends when the most loaded CU does.
// What a block size k costs there is
//     chain(k) + queue(k) * (workgroups on the most loaded CU - 1),    the most loaded CU holding ceil(workgroups / CUs):
// chain = one launch with at most one workgroup per CU (launch + loads + six passes + store), queue = what every further
// workgroup that shares the CU adds.  Microseconds, least-squares fits per k over the mono and 2-column clips of 10 .. 90 s
// below the throughput rule's size, k forced (tools/one_round_sweep.py; rows and fit: profiles/NOTES_one_round.md §3,
// profiles/one_round_forced_k.json).
// The k = 14 rows: refitted to the kernels with lane-pair passes (the same rows, one visit: profiles/NOTES_one_round_split.md §4).
// More candidate block sizes of a ratio are more rows here and more entries in fft_pairs — no code.
struct OneRoundCost { int64_t L, M; int k; float chain_us, queue_us; };
static const OneRoundCost kOneRoundCost[] = {
    {147, 160, 8, 6.29f, 0.79f}, {147, 160, 14, 7.65f, 1.06f}, {147, 160, 16, 8.01f, 1.24f}, {147, 160, 20, 8.72f, 1.57f}, {147, 160, 32, 9.72f, 2.85f}, // 48k -> 44.1k
    {160, 147, 8, 6.81f, 0.89f}, {160, 147, 14, 7.21f, 1.20f}, {160, 147, 16, 8.02f, 1.29f}, {160, 147, 20, 8.56f, 1.48f}, {160, 147, 32, 9.93f, 2.63f}, // 44.1k -> 48k
};
// A candidate must beat the size rules' choice by more than this: the run-to-run spread of one row of that sweep (a tie
// goes to the choice the thresholds make, so that nothing changes where nothing is gained)
static const double kOneRoundTieUs = 0.10;
static const OneRoundCost *one_round_cost(const PairEntry &e)
{
    for (const OneRoundCost &c : kOneRoundCost)
        if (c.L == e.L && c.M == e.M && c.k == e.k) return &c;
    return nullptr;
}
// What the rule needs to know about the device, asked once per device: CUs, LDS bytes and threads a CU holds.
struct CuShape { int cus = 0; int64_t lds = 0, threads = 0; };
static bool cu_shape(CuShape *out)
{
    static std::mutex mu;
    static std::vector<std::pair<int, CuShape>> seen;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : seen)
        if (e.first == d) { *out = e.second; return e.second.cus > 0; }
    CuShape c;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess) c.cus = v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, d) == hipSuccess) c.lds = v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxThreadsPerMultiProcessor, d) == hipSuccess) c.threads = v;
    if (c.lds <= 0 || c.threads <= 0) c.cus = 0; // (no rule without the whole picture: the thresholds' choice stands)
    seen.push_back({d, c});
    *out = c;
    return c.cus > 0;
}

// Whole-signal float32 / float64 job (or an int16 / int32 one that names the engine)?  (zero-extended signal starting at absolute index 0, all outputs)
bool fft_job_eligible(const Plan &p, const hipsoxr_job_t &j)
{
    // what the method neglects is the aliasing of the filter's stop band: only recipes whose stop band
    // is far below the 1e-6 bar qualify (HQ 128 dB, VHQ 177 dB; MQ/LQ at 104 dB do not)
    // (integer samples only by name — HIPSOXR_KERNEL_FFT_PCM: AUTO keeps them on the canonical order, bit for bit)
    // (float16 / bfloat16: wherever the float32 job of the same shape is — they compute in float32)
    const bool elem_ok = j.kernel == HIPSOXR_KERNEL_FFT_PCM ? (j.elem == HIPSOXR_I16 || j.elem == HIPSOXR_I32)
                                                            : (j.elem == HIPSOXR_F32 || j.elem == HIPSOXR_F64 || elem_is_half(j.elem));
    return p.phases == 0 && p.att_db >= 120. && elem_ok && j.in_abs0 == 0 &&
           j.out_k0 == 0 && (uint64_t)j.out_frames <= plan_out_len(p, (uint64_t)j.in_frames);
}

// Rows of fft_pairs that serve a ratio (indices; -1: none); cand: every block size — what the one-round rule chooses among
struct RatioRows { int big = -1, sml = -1, tiny = -1, cand[8], n_cand = 0; };
static RatioRows fft_ratio_rows(const Plan &p)
{
    RatioRows r;
    int n = 0;
    const PairEntry *pairs = fft_pairs(&n);
    for (int i = 0; i < n; ++i)
        if (pairs[i].L == p.L && pairs[i].M == p.M) {
            if (r.n_cand < 8) r.cand[r.n_cand++] = i;
            if (pairs[i].small == 3) continue; // (one-round float32 jobs only: fft_one_round_pick)
            if (pairs[i].small == 2) r.tiny = i;
            else if (pairs[i].small) r.sml = i;
            else r.big = i;
        }
    return r;
}

// byte offsets over `blocks` blocks at a frame stride fit the kernels' 32-bit operands
static bool fft_offsets_fit(const FftGeom &g, int blocks, int64_t frame_stride, size_t esz)
{
    return blocks * (int64_t)std::max(g.N_in, g.N_out) * frame_stride * (int64_t)esz < (1LL << 30);
}

// block pairs (the paired kernels' work items) over `span` outputs, all columns
static int64_t fft_pair_items(int64_t span, int64_t hop_out, uint64_t cols)
{
    return ((span + hop_out - 1) / hop_out + 1) / 2 * (int64_t)cols;
}

// Streams on this engine (HIPSOXR_STREAM_FFT): what it cannot serve is refused when the stream is created, by name.
// The chunks of a stream are windows of one column (launch_fft_window), served by the paired kernels alone — so the
// ratio must be in their schedule table for every element type, and the layout one they take: interleaved frames of
// `ch` channels = unit-stride columns (mono), channel pairs (even counts) or strided columns (odd counts, floats).
// *lead_periods: periods a block starts before its first kept output (what the stream's ring must keep, engine.cpp).
const char *fft_stream_refusal(const Plan &p, int elem, uint32_t ch, int32_t *lead_periods)
{
    *lead_periods = 0;
    if (p.phases) return "STREAM_FFT stream: the ratio has no exact polyphase bank (interpolated-phase plan); the frequency-domain engine serves streams of exact-ratio plans";
    if (p.att_db < 120.) return "STREAM_FFT stream: the frequency-domain engine serves HQ and VHQ only (recipes below 120 dB are not 1e-6-class on it)";
    if (elem == HIPSOXR_I32 && ch > 1) return "STREAM_FFT stream: int32 streams are served with one channel only (as HIPSOXR_KERNEL_FFT_PCM: unit-stride columns)";
    if (elem == HIPSOXR_I16 && ch > 1 && ch % 2) return "STREAM_FFT stream: int16 streams are served with one channel or an even channel count (as HIPSOXR_KERNEL_FFT_PCM: interleaved channel pairs)";
    int n = 0;
    const PairEntry *pairs = fft_pairs(&n);
    const int big = fft_ratio_rows(p).big;
    FftGeom g;
    if (big < 0 || !fft_geometry(p, g, false, pairs[big].k))
        return "STREAM_FFT stream: the ratio is outside the paired-kernel schedule table of the frequency-domain engine (fft.hip)";
    // the kernels' 32-bit byte offsets over a pair of blocks at the frame stride (fft_layout: cp2 / st2ok)
    if (!fft_offsets_fit(g, 2, (int64_t)ch, elem_size(elem)))
        return "STREAM_FFT stream: too many channels for the frequency-domain engine's interleaved kernels";
    *lead_periods = g.lead_periods; // (fft_kept_run: the same for every block size of the ratio)
    return nullptr;
}

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build): one text line per call of launch_fft_impl, appended to that file — what
// was launched for the job (tests/test_gpu_fft_table.py asserts it).  form: pair2 / strided2_cp / strided2_st (a row of
// fft_pairs: L M k small are the row's), wave (k_fft_wave: its own k; grid = block pairs x columns, the work items of its
// persistent waves), block (k_fft_block: the geometry's k), none (nothing launched, *handled == false; the row chosen so
// far, if any).  small = -1: not a row of the table.  A launch over a clip table appends ragged=<columns>; lines of
// equal-length jobs are as they were.
static void fft_launch_log(const char *form, int64_t L, int64_t M, int k, int small, const char *kind, unsigned nt, size_t lds,
                           dim3 grid, int64_t hop_out, int64_t n_blocks, bool window, uint64_t ragged = 0)
{
    FILE *f = fopen(switches().dbg_launch_log, "a");
    if (!f) return;
    fprintf(f, "form=%s L=%lld M=%lld k=%d small=%d kind=%s nt=%u lds=%zu grid=%ux%ux%u hop_out=%lld n_blocks=%lld window=%d", form,
            (long long)L, (long long)M, k, small, kind, nt, lds, grid.x, grid.y, grid.z, (long long)hop_out, (long long)n_blocks, window ? 1 : 0);
    if (ragged) fprintf(f, " ragged=%llu", (unsigned long long)ragged); // (a clip table: its columns; n_blocks: the longest column's)
    fprintf(f, "\n");
    fclose(f);
}

// ---- the job as the launch code sees it -------------------------------------------------------------------
// (job.in_abs0 != 0 — in[0] is sample in_abs0 of a column that is zero outside [in_abs0, in_abs0 + in_frames) — is served
// for the two-stage form's inner calls; the public paths come here through fft_job_eligible, which wants 0.)
// window (launch_fft_window, stream chunks): the job is outputs [out_k0, out_k0 + out_frames) of the column.  The paired
// kernels get their origin moved to the period boundary P0 = floor(out_k0 / L): `in` / `out` are shifted by P0 M / P0 L
// frames, so block 0 starts lead_periods before P0 and the block arithmetic is the whole-signal job's; the one thing the
// kernels do for it is drop the outputs below out_lo = out_k0 - P0 L (< L <= hop_out: inside the first block's run) and
// key the dither by P0 L + local index.  Served by k_fft_pair2 / k_fft_strided2 only: *handled stays false otherwise.
struct FftJobView {
    bool window;
    int64_t P0, out_lo, span; // span: outputs from the origin to the end of the job — what blocks are counted over
    uint64_t cols;
    // f64: the ARITHMETIC is float64 (block size, LDS bytes per point, table set) — float64 jobs, float32 jobs that ask
    // for libsoxr's own VHQ width with HIPSOXR_KERNEL_FFT_F64 (wide32), and int32 samples.  pcm: integer samples
    // (HIPSOXR_KERNEL_FFT_PCM), int16 on float32 and int32 on float64 arithmetic — every size rule is the float job's of
    // that arithmetic width.  kind: the launch log's name of the instance.
    // half: float16 / bfloat16 samples on float32 arithmetic (bf16: which) — every size rule is the float32 job's.
    bool io64, wide32, pcm, pcm32, f64, half, bf16;
    const char *kind;
    size_t esz;
};
static FftJobView fft_job_view(const Plan &p, const hipsoxr_job_t &j, bool window)
{
    FftJobView v;
    v.window = window;
    v.P0 = window ? j.out_k0 / p.L : 0; v.out_lo = window ? j.out_k0 - v.P0 * p.L : 0;
    v.span = v.out_lo + j.out_frames;
    v.cols = (uint64_t)j.n_clips * j.n_channels;
    v.io64 = j.elem == HIPSOXR_F64; v.wide32 = !v.io64 && j.kernel == HIPSOXR_KERNEL_FFT_F64;
    v.pcm = j.elem == HIPSOXR_I16 || j.elem == HIPSOXR_I32; v.pcm32 = j.elem == HIPSOXR_I32;
    v.half = elem_is_half(j.elem); v.bf16 = j.elem == HIPSOXR_BF16;
    v.f64 = v.io64 || v.wide32 || v.pcm32;
    v.kind = v.pcm ? (v.pcm32 ? "i32" : "i16") : v.half ? (v.bf16 ? "bf16" : "f16") : v.io64 ? "f64" : v.wide32 ? "f32on64" : "f32";
    v.esz = elem_size(j.elem);
    return v;
}

// ---- row choice --------------------------------------------------------------------------------------------
struct FftRow { const PairEntry *use = nullptr; FftGeom g; }; // use == nullptr: no row of the table serves the job

// One-round jobs (see kOneRoundCost): float32 unit-stride columns — exactly the jobs that run `kern2` (v2ok, not f64,
// not pcm), and the float16 / bfloat16 jobs that run its half forms: they take the row the float32 job takes, on the
// float32 cost figures (their own are unmeasured), so that a half job is the float32 job's arithmetic at every size
// — as whole signals, where the throughput rule left the large blocks.  Every other element type, layout and the
// stream path keep the size rules' choice `use`; so does this one under HIPSOXR_FFT_LARGE_ONLY / _SMALL_ONLY (they name a
// block size), and HIPSOXR_FFT_NO_TINY takes k = 8 away.  Ties go to `use`.  HIPSOXR_DEBUG_FFT_K (debug builds): k > 0
// forces that block size for every such job, whatever its size; k < 0 turns the rule off.
// -> the index of the row to take instead of `use`, or -1: the size rules' choice stands.
static int fft_one_round_pick(const Plan *p, const hipsoxr_job_t &j, const FftJobView &v, const RatioRows &rows, const PairEntry *use, bool use_is_big)
{
    int n_pairs = 0;
    const PairEntry *pairs = fft_pairs(&n_pairs);
    const bool plain_cols = j.in_frame_stride == 1 && j.out_frame_stride == 1 &&
                            (j.n_channels == 1 || j.in_chan_stride != 1 || j.out_chan_stride != 1); // (=> no XCD map, no channel pairs)
    const int force_k1 = switches().dbg_fft_k;
    if (!((!use_is_big || force_k1 > 0) && plain_cols && (j.elem == HIPSOXR_F32 || v.half) && !v.wide32 && !v.window && force_k1 >= 0 &&
          ((!switches().fft_large_only && !switches().fft_small_only) || force_k1 > 0)))
        return -1;
    // a candidate's cost; < 0: not a candidate (no figures, no such block, or not co-resident on this device)
    auto cost_of = [&](const PairEntry &e, const CuShape &cu) -> double {
        const OneRoundCost *c = one_round_cost(e);
        const int64_t hop = fft_hop_out(*p, e.k);
        if (!c || !hop || !e.kern2) return -1.;
        const int64_t lds = std::max(e.k * p->L, e.k * p->M) * (int64_t)sizeof(float2);
        if (2 * hop * (int64_t)sizeof(float) + 16 > lds) return -1.; // (the staged run must fit the transform buffer: v2ok)
        const int64_t slots = std::min(cu.lds / lds, cu.threads / (int64_t)e.nt);
        const int64_t per_cu = (fft_pair_items(v.span, hop, v.cols) + cu.cus - 1) / cu.cus;
        if (per_cu > slots) return -1.;
        return (double)c->chain_us + (double)c->queue_us * (double)(per_cu - 1);
    };
    // (the answer depends on the plan, the job's size and the size rules' choice alone: the last one is kept per thread,
    //  so that a loop over one job — 10 us a launch, as long as the kernel runs — pays for the rule once)
    struct Memo { const Plan *p; int64_t L, M, span; int32_t T; uint64_t cols; const PairEntry *from; bool no_tiny; int dev, pick; };
    static thread_local Memo memo = {nullptr, 0, 0, 0, 0, 0, nullptr, false, -1, -1};
    int dev_now = -1;
    (void)hipGetDevice(&dev_now);
    const bool memo_hit = force_k1 == 0 && memo.p == p && memo.L == p->L && memo.M == p->M && memo.T == p->T && memo.span == v.span &&
                          memo.cols == v.cols && memo.from == use && memo.dev == dev_now && memo.no_tiny == switches().fft_no_tiny;
    if (memo_hit) return memo.pick;
    int pick = -1;
    CuShape cu;
    if (force_k1 > 0) {
        for (int c = 0; c < rows.n_cand; ++c)
            if (pairs[rows.cand[c]].k == force_k1 && pairs[rows.cand[c]].kern2) pick = rows.cand[c];
    } else if (cu_shape(&cu)) {
        double best = cost_of(*use, cu);
        for (int c = 0; c < rows.n_cand && best >= 0.; ++c) { // (the size rules' choice outside the model: it stands)
            const PairEntry &e = pairs[rows.cand[c]];
            if (&e == use || (e.small == 2 && switches().fft_no_tiny)) continue;
            const double cst = cost_of(e, cu);
            if (cst >= 0. && cst < best - (pick < 0 ? kOneRoundTieUs : 0.)) { best = cst; pick = rows.cand[c]; }
        }
    }
    if (force_k1 == 0) memo = {p, p->L, p->M, v.span, p->T, v.cols, use, switches().fft_no_tiny, dev_now, pick};
    return pick;
}

// The row a job runs on, with its geometry: full-size, half-size for few work items, quarter-size for fewer still, then
// the one-round rule — the geometry cache is asked in that order, and only for the rows the rules reach.
static const char *fft_choose_row(Plan *p, const hipsoxr_job_t &j, const FftJobView &v, FftRow *row)
{
    int n_pairs = 0;
    const PairEntry *pairs = fft_pairs(&n_pairs);
    const RatioRows rows = fft_ratio_rows(*p);
    if (rows.big < 0) return nullptr;
    const PairEntry *big = &pairs[rows.big], *sml = rows.sml < 0 ? nullptr : &pairs[rows.sml], *tiny = rows.tiny < 0 ? nullptr : &pairs[rows.tiny];
    FftGeom g;
    if (const char *err = fft_geom_cached(p, 2 + rows.big, big->k, &g)) return err;
    const PairEntry *use = g.ok ? big : nullptr;
    if (g.ok && sml) {
        // few work items (one 60 s clip = 300 pairs): half-size blocks give twice as many,
        // shorter workgroups, at the price of more overlap
        const int64_t wgs = fft_pair_items(v.span, g.hop_out, v.cols);
        // (float64: LDS is 16 bytes per point — the half-size blocks keep four workgroups per CU)
        // (7056-point blocks: 56 KB of LDS, two workgroups per CU — the 35 KB blocks of the k = 10 geometry keep
        //  four and win at every size: 44.1k -> 16k VHQ, 8 x 60 s planar 41 vs 68 us, 80 x 60 s 427 vs 638 us)
        const bool big_lds = big->nt > 384;
        if (((wgs < 480 || big_lds) && !switches().fft_large_only) || switches().fft_small_only || v.f64) { // measured crossover: ~470 pairs of large blocks
            FftGeom gs;
            if (const char *err = fft_geom_cached(p, 2 + rows.sml, sml->k, &gs)) return err;
            if (gs.ok) { g = gs; use = sml; }
        }
    }
    // Fewer still (a 60 s clip is 612 pairs of half-size blocks on 2048 workgroup slots): the launch is the
    // latency of one workgroup plus what queues behind it; quarter-size blocks (10 KB of LDS, 32 % overlap)
    // shorten both: 2 s clip 7.4 -> 6.5 us, 10 s HQ 7.6 -> 6.2 us, 30 s 9.0 -> 7.7 us (60 s: 10.85 vs 10.73 us).
    if (use == sml && tiny && !switches().fft_large_only && !switches().fft_no_tiny) {
        // (float32: at 612 pairs — the 60 s clip — the two sizes are within 1 %.  float64: 16 bytes per point, and
        //  the 20 KB blocks win at every size — 60 s mono 27.1 -> 21.6 us, 64 x 10 s 236 -> 202 us, stereo 60 s 47 -> 37 us)
        if (v.f64 || fft_pair_items(v.span, g.hop_out, v.cols) <= 500) {
            FftGeom gt;
            if (const char *err = fft_geom_cached(p, 2 + rows.tiny, tiny->k, &gt)) return err;
            if (gt.ok) { g = gt; use = tiny; }
        }
    }
    if (use) {
        const int pick = fft_one_round_pick(p, j, v, rows, use, use == big);
        if (pick >= 0 && &pairs[pick] != use) {
            FftGeom gc;
            if (const char *err = fft_geom_cached(p, 2 + pick, pairs[pick].k, &gc)) return err;
            if (gc.ok) { g = gc; use = &pairs[pick]; }
        }
    }
    row->use = use; row->g = g;
    return nullptr;
}

// ---- layout decision ----------------------------------------------------------------------------------------
// Which kernel form a job takes on a geometry, and its launch shape — arithmetic alone (cf. kernels.hip interp_tile_form).
//   v2ok   unit-stride columns (mono / planar): k_fft_pair2 — buffer loads, staged aligned stores
//   cp2ok  interleaved data with an even channel count: k_fft_strided2<CP = true>, one (Real, Real) word per frame
//   st2ok  other strided columns (odd channel counts, channel slices): k_fft_strided2<CP = false>, two blocks per transform
// None of the three: not the paired kernels' job (the caller's error, or the exact engine).
struct FftLayout {
    int32_t chpair = 0, xcd_map = 0;
    int64_t n_blocks = 0, items = 0, units = 0; // items: work items per channel unit — blocks (channel pairs) or pairs of blocks (single channels)
    dim3 grid;
    bool v2ok = false, cp2ok = false, st2ok = false;
    size_t lds = 0;
};
static const char *fft_layout(const hipsoxr_job_t &j, const FftJobView &v, const FftGeom &g, const Switches &sw, FftLayout *out)
{
    FftLayout y;
    y.n_blocks = (v.span + g.hop_out - 1) / g.hop_out;
    if (y.n_blocks > 2147483647LL) return "job too long for one launch";
    // interleaved data with an even channel count: pair channels (one (Real, Real) word per frame)
    const bool cp_layout = j.n_channels % 2 == 0 && j.in_chan_stride == 1 && j.out_chan_stride == 1 && !sw.fft_no_chpair;
    // ... when a block's byte offsets fit the kernel's 32-bit operands (buffer loads: element alignment is enough)
    // (int16 / float16 / bfloat16: the (l, r) word is ONE 4-byte access — every pair of every frame of every clip must be 4-byte aligned)
    const bool cp_pcm_ok = !(v.pcm || v.half) || (!v.pcm32 && (((uintptr_t)j.in | (uintptr_t)j.out) & 3) == 0 &&
                                      ((j.in_frame_stride | j.out_frame_stride | (j.n_clips > 1 ? j.in_clip_stride | j.out_clip_stride : 0)) & 1) == 0 &&
                                      // (a clip table: the clips lie at their rows' offsets — both even, fft_ragged_rules.h)
                                      (!j.clip_table || fft_table_words_aligned(j.clip_table, j.n_clips)));
    const int64_t fstride = std::max(j.in_frame_stride, j.out_frame_stride);
    const bool cp2 = !v.wide32 && cp_pcm_ok && fft_offsets_fit(g, 1, fstride, v.esz);
    // (channel pairing rides on the XCD-aware work-item map: decided together, so that a job without the
    //  map — HIPSOXR_FFT_NO_XCD_MAP, or too many work items — runs unpaired on the strided kernel instead of failing)
    const int64_t cp_items8 = (y.n_blocks + 7) / 8 * 8;
    const bool cp_map_ok = j.n_channels > 1 && fft_map_clips_ok(j.n_clips) && cp_items8 * (int64_t)(j.n_channels / 2) <= 2147483647LL && !sw.fft_no_xcd_map;
    y.chpair = (cp_layout && cp_map_ok && cp2) ? 1 : 0;
    y.lds = std::max((size_t)std::max(g.N_in, g.N_out) * (v.f64 ? sizeof(double2) : sizeof(float2)), sw.dbg_fft_lds);
    *out = y;
    if (v.f64 && y.lds > 160 * 1024) return nullptr; // (no form: the block does not fit LDS in float64)
    y.items = y.chpair ? y.n_blocks : (y.n_blocks + 1) / 2;
    const int64_t items8 = (y.items + 7) / 8 * 8;
    y.units = y.chpair ? j.n_channels / 2 : j.n_channels;
    y.xcd_map = (j.n_channels > 1 && j.in_chan_stride == 1 && j.out_chan_stride == 1 && fft_map_clips_ok(j.n_clips) &&
                 items8 * y.units <= 2147483647LL && !sw.fft_no_xcd_map) ? 1 : 0;
    if (y.chpair && !y.xcd_map) return "internal: channel pairing needs the XCD map"; // (cannot happen: cp_map_ok above)
    y.grid = y.xcd_map ? dim3((unsigned)fft_xcd_grid_x(y.items, y.units), j.n_clips, 1) : dim3((unsigned)((y.n_blocks + 1) / 2), (unsigned)v.cols, 1);
    // (integer samples are staged as the arithmetic's values, up to 7 elements into the run's first granule)
    const size_t stage_bytes = (v.pcm || v.half) ? 2 * (size_t)g.hop_out * (v.f64 ? sizeof(double) : sizeof(float)) + 32 : 2 * (size_t)g.hop_out * v.esz + 16;
    y.v2ok = !y.xcd_map && !y.chpair && j.in_frame_stride == 1 && j.out_frame_stride == 1 && stage_bytes <= y.lds;
    y.cp2ok = y.chpair && y.xcd_map && cp2;
    // ... when the byte offsets of a PAIR of blocks fit the 32-bit operands
    y.st2ok = !v.wide32 && !v.pcm && !v.half && !y.chpair && !y.v2ok && fft_offsets_fit(g, 2, fstride, v.esz);
    *out = y;
    return nullptr;
}

// ---- kernel arguments ---------------------------------------------------------------------------------------
// table pointers and geometry members of a launch on `g` (nA / nB / radA / radB: empty — fft_launch_block fills them)
static void fft_args_geom(FftArgs &a, const FftGeom &g)
{
    const FftTabs t = fft_tabs(g);
    a.WA = g.dev + t.WA; a.WB = g.dev + t.WB; a.P = g.dev + t.P; a.Q = g.dev + t.Q; a.Hs = g.dev + t.Hs;
    a.WA2 = g.dev + t.WA2; a.WB2 = g.dev + t.WB2; a.Hr = reinterpret_cast<const float *>(g.dev + t.Hr);
    a.WA2d = g.devd + t.WA2d; a.WB2d = g.devd + t.WB2d; a.Hrd = reinterpret_cast<const double *>(g.devd + t.Hrd);
    a.TWA = g.twa ? g.dev + g.twa : nullptr; a.TWB = g.twb ? g.dev + g.twb : nullptr;
    a.A = g.A; a.B = g.B; a.nA = a.nB = 0;
    for (int i = 0; i < 8; ++i) a.radA[i] = a.radB[i] = 1;
    a.lead_periods = g.lead_periods; a.hop_periods = g.hop_periods; a.v0 = g.v0; a.hop_out = g.hop_out;
}
// ... and the job's part, the same for every form: sample 0 of the columns (window: frame P0 M / P0 L of them.  int16
// channel pairs: the shift is a whole number of frames, so with the even frame strides cp_pcm_ok asks for, the 4-byte
// alignment it checks on j.in / j.out holds for the shifted pointers too)
static FftArgs fft_args(const Plan &p, const hipsoxr_job_t &j, const FftJobView &v, const FftGeom &g, uint32_t ch0)
{
    FftArgs a;
    fft_args_geom(a, g);
    a.in_lo = j.in_abs0 - v.P0 * p.M; a.in_frames = a.in_lo + j.in_frames; a.out_frames = v.span;
    a.in = (const char *)j.in - a.in_lo * j.in_frame_stride * (int64_t)v.esz;
    a.out = (char *)j.out - v.out_lo * j.out_frame_stride * (int64_t)v.esz;
    a.out_lo = v.out_lo; a.out_abs0 = v.P0 * p.L;
    a.L = p.L; a.M = p.M;
    a.n_clips = j.n_clips; a.n_channels = j.n_channels;
    a.ics = j.in_clip_stride; a.ifs = j.in_frame_stride; a.ichs = j.in_chan_stride;
    a.ocs = j.out_clip_stride; a.ofs = j.out_frame_stride; a.ochs = j.out_chan_stride;
    a.clip_tab = j.clip_table_dev;
    a.clip_counter = v.pcm ? j.clip_counter : nullptr; a.dither = j.dither; a.seed = j.dither_seed; a.ch0 = ch0;
    a.chpair = 0; a.xcd_map = 0; a.pairs_per_col = 0; a.trace = nullptr;
    return a;
}

// ---- one launcher per form ------------------------------------------------------------------------------------
// (-DFFT2_TRACE: per-wave time stamps of the paired kernels, dumped synchronously behind the launch)
#ifdef FFT2_TRACE
static const char *fft_trace_begin(FftArgs &a, dim3 grid, unsigned nt, size_t *n)
{
    *n = 0;
    if (!switches().dbg_trace) return nullptr;
    *n = (size_t)grid.x * grid.y * (nt / 64) * 16;
    HIP_TRY(hipMalloc((void **)&a.trace, *n * 8));
    HIP_TRY(hipMemset(a.trace, 0, *n * 8));
    return nullptr;
}
static const char *fft_trace_dump(const FftArgs &a, size_t n, void *stream)
{
    if (!a.trace) return nullptr;
    std::vector<unsigned long long> h(n);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(h.data(), a.trace, n * 8, hipMemcpyDeviceToHost));
    if (FILE *f = fopen(switches().dbg_trace, "wb")) { fwrite(h.data(), 8, n, f); fclose(f); }
    (void)hipFree(a.trace);
    return nullptr;
}
#else
static const char *fft_trace_begin(FftArgs &, dim3, unsigned, size_t *) { return nullptr; }
static const char *fft_trace_dump(const FftArgs &, size_t, void *) { return nullptr; }
#endif

// Throughput form (fftwave.hip): one wave per pair of 24-period blocks, two register passes per transform — float32
// unit-stride columns with enough pairs to fill the chip's 2048 wave slots four times over (below that the last, partly
// filled round costs more than the form gains; and a single pair's latency is longer than on the 6-wave workgroups of
// k_fft_pair2).  Never a window, and never a column with frames missing in FRONT — a.in_lo > 0, data-dependent front
// extension: k_fft_wave's front guard covers the lead-in of block 0 only.  *handled stays false: not this form's job.
static const char *fft_try_wave(Plan *p, const hipsoxr_job_t &j, const FftJobView &v, const FftLayout &lay, FftArgs a, void *stream, bool *handled)
{
    FftWaveKernel wk;
    if (!(lay.v2ok && !v.f64 && !v.pcm && !v.half && !v.window && a.in_lo <= 0 && !switches().fft_no_wave && fft_wave_pick(p->L, p->M, &wk))) return nullptr;
    // (the job size first, from the kernel's own constants: its geometry — a host DFT of the filter and two
    //  device allocations — is built only for a job that can take it; 48k -> 44.1k never does)
    const int64_t pairs_w = ((j.out_frames + wk.hop - 1) / wk.hop + 1) / 2;
    const int64_t wave_min = switches().dbg_wave_min ? switches().dbg_wave_min : wk.min_pairs;
    FftGeom gw;
    if (pairs_w * (int64_t)v.cols >= wave_min && pairs_w * (int64_t)v.cols <= 2147483000LL) // (item numbers are 32-bit; a larger job stays on k_fft_pair2)
        if (const char *err = fft_geom_cached(p, 1000 + wk.k, wk.k, &gw)) return err;
    if (!(gw.ok && gw.v0 == wk.v0 && gw.hop_out == wk.hop && gw.hop_periods == wk.hop_periods)) return nullptr;
    fft_args_geom(a, gw);
    if (const char *e = fft_wave_launch(wk, a, (unsigned)pairs_w, (unsigned)v.cols, stream)) return e;
    if (switches().dbg_launch_log)
        fft_launch_log("wave", p->L, p->M, wk.k, -1, v.kind, 64, 0, dim3((unsigned)pairs_w, (unsigned)v.cols, 1), gw.hop_out, 2 * pairs_w, v.window, a.clip_tab ? v.cols : 0);
    *handled = true;
    return nullptr;
}

static const char *fft_launch_paired(const PairEntry &e, const FftGeom &g, const FftJobView &v, const FftLayout &lay, FftArgs a, void *stream, bool *handled)
{
    void (*kern)(FftArgs) = nullptr;
    const HalfKernels *hk = v.half ? fft_half_kernels(e) : nullptr;
    if (v.half && !hk) return "internal: a row of the schedule table has no float16 / bfloat16 kernels"; // (cannot happen: the instantiation lists cover the table)
    if (lay.v2ok) kern = v.pcm ? (v.pcm32 ? e.kern2i32 : e.kern2i16) : v.half ? (v.bf16 ? hk->kern2bf : hk->kern2h) : v.io64 ? e.kern2d : v.wide32 ? e.kern2fd : e.kern2;
    else kern = v.pcm ? e.kcpi16 : v.half ? (v.bf16 ? hk->kcpbf : hk->kcph) : lay.cp2ok ? (v.f64 ? e.kcpd : e.kcp) : (v.f64 ? e.kstd : e.kst); // (pcm: cp2ok — st2ok wants floats)
    if (!kern) return "internal: a float32-only block size was chosen for another kind of job"; // (cannot happen: plain_cols of fft_one_round_pick)
    if (const char *err = ensure_dyn_lds((const void *)kern, lay.lds)) return err;
    size_t trace_n = 0;
    if (const char *err = fft_trace_begin(a, lay.grid, e.nt, &trace_n)) return err;
    hipLaunchKernelGGL(kern, lay.grid, dim3(e.nt), lay.lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log)
        fft_launch_log(lay.v2ok ? "pair2" : lay.cp2ok ? "strided2_cp" : "strided2_st", e.L, e.M, e.k, e.small, v.kind, e.nt, lay.lds, lay.grid, g.hop_out, lay.n_blocks, v.window, a.clip_tab ? v.cols : 0);
    if (const char *err = fft_trace_dump(a, trace_n, stream)) return err;
    *handled = true;
    return nullptr;
}

// A job on a row of the table: the wave form where it wins, else the row's paired kernel (*handled stays false: no form)
static const char *fft_launch_row(Plan *p, const hipsoxr_job_t &j, const FftJobView &v, const FftRow &row, void *stream, uint32_t ch0, bool *handled)
{
    if (v.out_lo >= row.g.hop_out) return "internal: the job window starts beyond the first block"; // (cannot happen: out_lo < L <= hop_out)
    FftLayout lay;
    if (const char *err = fft_layout(j, v, row.g, switches(), &lay)) return err;
    FftArgs a = fft_args(*p, j, v, row.g, ch0);
    a.chpair = lay.chpair; a.xcd_map = lay.xcd_map; a.pairs_per_col = lay.items;
    if (const char *err = fft_try_wave(p, j, v, lay, a, stream, handled)) return err;
    if (*handled) return nullptr;
    if (!lay.v2ok && !lay.cp2ok && !lay.st2ok) return nullptr;
    // ragged batches: every paired kernel reads its clip's row; the strided forms by name only (fft_ragged_rules.h: AUTO keeps
    // interleaved tables of an exact-bank plan on the exact engine, bit for bit)
    if (j.clip_table && !fft_table_form_served(lay.v2ok, lay.cp2ok, lay.st2ok, j.kernel != HIPSOXR_KERNEL_AUTO)) return nullptr;
    // float16 / bfloat16: the fused forms alone (half_rules.h) — what they do not take is the widening pass's, not an error
    if (v.half && half_fused_form(true, lay.v2ok, lay.cp2ok, j.clip_table != nullptr) == kHalfNone) return nullptr;
    return fft_launch_paired(*row.use, row.g, v, lay, a, stream, handled);
}

// General path: one block per workgroup — float32 whole signals of any 7-smooth plan, no ragged batches
static const char *fft_launch_block(Plan *p, const hipsoxr_job_t &j, const FftJobView &v, void *stream, bool *handled)
{
    if (v.f64 || v.pcm || v.half || j.clip_table || v.window) return nullptr;
    FftGeom g;
    if (const char *err = fft_geom_cached(p, 0, 0, &g)) return err;
    if (g.ok) {
        const int64_t wgs = ((j.out_frames + g.hop_out - 1) / g.hop_out) * (int64_t)j.n_clips * j.n_channels;
        if ((wgs < 8 * 256 && !switches().fft_large_only) || switches().fft_small_only) {
            FftGeom gs;
            if (const char *err = fft_geom_cached(p, 1, 0, &gs)) return err;
            if (gs.ok && gs.k < g.k) g = gs;
        }
    }
    if (!g.ok) return nullptr;
    FftArgs a = fft_args(*p, j, v, g, 0);
    a.nA = g.nA; a.nB = g.nB;
    for (int i = 0; i < 8; ++i) { a.radA[i] = g.radA[i]; a.radB[i] = g.radB[i]; }
    const int64_t n_blocks = (j.out_frames + g.hop_out - 1) / g.hop_out;
    if (v.cols > 65535) return "too many (clip, channel) columns for one launch (max 65535)";
    if (n_blocks > 2147483647LL) return "job too long for one launch";
    const size_t lds = std::max(g.lds_bytes, switches().dbg_fft_lds);
    const dim3 grid((unsigned)n_blocks, (unsigned)v.cols, 1);
    if (const char *e = ensure_dyn_lds((const void *)k_fft_block, lds)) return e;
    hipLaunchKernelGGL(k_fft_block, grid, dim3(256), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    if (switches().dbg_launch_log) fft_launch_log("block", p->L, p->M, g.k, -1, v.kind, 256, lds, grid, g.hop_out, n_blocks, v.window);
    *handled = true;
    return nullptr;
}

// ---- dispatcher ---------------------------------------------------------------------------------------------
// The forms in order: the wave form and the paired kernels on a row of the table, else k_fft_block.  float64 arithmetic
// and integer samples: the paired kernels only — else the exact engine (integer samples: the caller's error).
static const char *launch_fft_impl(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled, uint32_t ch0, bool window)
{
    *handled = false;
    const FftJobView v = fft_job_view(*p, j, window);
    const bool paired = !switches().fft_no_pair && v.cols <= 65535;
    FftRow row;
    const char *err = nullptr;
    if (paired) err = fft_choose_row(p, j, v, &row);
    if (row.use) err = fft_launch_row(p, j, v, row, stream, ch0, handled);
    else if (!err && (paired || (!v.f64 && !v.pcm))) err = fft_launch_block(p, j, v, stream, handled);
    if (!*handled && switches().dbg_launch_log) // leaving without a launch: the log says so, with the row chosen so far
        fft_launch_log("none", p->L, p->M, row.use ? row.use->k : 0, row.use ? row.use->small : -1, v.kind, 0, 0, dim3(0, 0, 0), 0, 0, window);
    return err;
}

const char *launch_fft(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled, uint32_t ch0)
{
    return launch_fft_impl(p, j, stream, handled, ch0, false);
}

const char *launch_fft_window(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled, uint32_t ch0)
{
    return launch_fft_impl(p, j, stream, handled, ch0, true);
}

#endif // host part (FFT_PART != 1)
} // namespace hipsoxr
