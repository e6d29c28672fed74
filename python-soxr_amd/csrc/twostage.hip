// twostage.hip — arbitrary rate ratios at reduced cost: the frequency-domain engine + a short polyphase stage.
//
// Ratios outside the exact-bank range (random integer or float rates: reference tests/test_random.py:21-25) get an
// interpolated-phase plan, and the canonical-order engine evaluates its 296-tap (VHQ) direct form with a cubic per tap:
// 48000 -> 44101 stereo 60 s took 402 us against 70 us for its rational neighbour.  libsoxr itself serves such ratios at
// near-constant cost with an FFT stage at a fixed ratio plus a short interpolated polyphase stage (SURVEY.md §0.3 / §A.4,
// upstream-unverified).  The MI355X form, for whole-signal float32 / float64 device jobs under HIPSOXR_KERNEL_AUTO /
// _FFT (1e-6 class; the host surface, streams and integer I/O keep the bit-exact k_interp / k_interp_tile):
//
//   up   (out > in):  x --[FFT engine 1:2, the plan's OWN prototype sampled on the half-sample grid]--> u at 2 f_in
//                       --[k_poly: T2-tap interpolated polyphase, transparent on [0, f_in/2], stop from 1.5 f_in]--> y
//   down (out < in):  x --[k_poly: transparent on [0, f_out/2], stop from 1.5 f_out]--> v at 2 f_out
//                       --[FFT engine 2:1, the plan's own prototype re-expressed at 2 f_out]--> y
//
// The sharp filter of the composite IS the plan's prototype h (plan_proto), so the result equals the single-stage
// filter's to the polyphase stage's ripple (designed 6 dB below the recipe) and the FFT engine's own floor — on any input,
// not only band-limited ones: <= 1e-6 of the oracle's float64 direct form (tests/test_gpu_random_rates.py).
// The polyphase stage's cubic table ([P2][T2] records of 16 bytes: 12-50 KB) lives in LDS, which ends the 423 MB stream of
// coefficient records through the scalar cache that bounds k_interp_tile.
// Ends: the intermediate signal is produced a few samples PAST both ends of the job (as far as the second stage reads it;
// hipsoxr_job_t::in_abs0 places it for the FFT engine), so every output, the first and last included, is the composite
// filter's response to the zero-extended signal: two launches in all.  A thread of k_poly keeps its source window in
// registers from one output to the next (see MQ), so the table records are the stage's only per-tap LDS traffic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <mutex>
#include <vector>

#include "adjoint_auto_rules.h" // ragged_poly_adj_plan: a clip table on the transposed form
#include "adjoint_rules.h" // adj_extent_refusal: the adjoint's length rule is the exact adjoint's
#include "device.h"
#include "job_rules.h"     // job_empty
#include "poly_adj_rules.h"
#include "poly_rules.h"
#include "ragged_rules.h" // ragged_span_skip

namespace hipsoxr {

#define HIP_TRY(expr)                                       \
    do {                                                    \
        hipError_t e_ = (expr);                             \
        if (e_ != hipSuccess) return hipGetErrorString(e_); \
    } while (0)

// tap counts the polyphase kernel is instantiated for (poly_design rounds its design up to the next one)
#define HIPSOXR_POLY_TAPS(X) X(8) X(12) X(16) X(20) X(24) X(28) X(32) X(40) X(48) X(56)
#define HIPSOXR_POLY2_TAPS(X) X(8) X(12) X(16) X(20) X(24) X(28) X(32) X(40) // k_poly2 (two windows in registers: longer ones spill)

struct TwoStage {
    bool ok = false, up = false;
    Plan fft;                 // the FFT stage's plan: L/M = 2/1 (up) or 1/2 (down), bank from the owner's prototype
    int32_t T2 = 0, P2 = 0, P2f = 0, row = 0; // polyphase stage: taps, table intervals (float64 / float32 table), records per table row (T2 + 1: bank spreading)
    int64_t Ls = 1, Ms = 1;   // polyphase stage: output k sits at k * Ms / Ls of ITS input samples
    // poly_lanes' cache, [float32 / float64 / float32 on k_poly2][R]: the lane order of runs of R outputs per thread
    // (lane_mul 0 = not simulated yet).  Written behind a const TwoStage & under g_lanes_mu.
    mutable PolyLane lanes[3][16] = {};
    void *tab_f = nullptr, *tab_d = nullptr; // device: [P2f][row] float4 / [P2][row] double4 records (a0..a3 of the cubic in x in [0, 1))
    Plan *fft_t = nullptr;    // the transposed plan of `fft` (HIPSOXR_KERNEL_ADJOINT_TWO_STAGE: built on first use, released with this)
};

void twostage_release(Plan *p)
{
    if (!p->two) return;
    if (p->two->tab_f) (void)hipFree(p->two->tab_f);
    if (p->two->tab_d) (void)hipFree(p->two->tab_d);
    delete p->two->fft_t;
    delete p->two; // (the FFT stage's plan releases its own device tables: Plan::~Plan)
    p->two = nullptr;
}

static int64_t gcd64(int64_t a, int64_t b)
{
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// Kaiser-windowed sinc of the polyphase stage in units of ITS input samples: cut-off fc (cycles per sample), half width W
struct PolyProto {
    double fc, W, beta, inv_i0, scale;
    double operator()(double tau) const
    {
        const double u = tau / W;
        double w = 1. - u * u;
        if (w <= 0.) return 0.;
        const double s = tau == 0. ? 2. * fc : std::sin(2. * M_PI * fc * tau) / (M_PI * tau);
        return s * bessel_i0(beta * std::sqrt(w)) * inv_i0 * scale;
    }
};

// the FFT stage's plan: the owner's prototype H(tau) (tau in the OWNER's input samples) on the 2x grid; rho: owner-input
// samples per sample of the intermediate signal (down)
static void twostage_fft_plan(const Plan *p, bool up, double rho, Plan &f)
{
    const double fi = p->in_rate, fo = p->out_rate;
    f.recipe = p->recipe; f.q = p->q; f.att_db = p->att_db; f.beta = p->beta; f.phases = 0;
    if (up) { // u[m] = sum_n x[n] H(m/2 - n): bank[ph][j] = H(ph/2 + T/2 - 1 - j)
        f.in_rate = fi; f.out_rate = 2. * fi; f.L = 2; f.M = 1; f.T = p->T;
        f.bank.assign((size_t)2 * f.T, 0.);
        for (int ph = 0; ph < 2; ++ph)
            for (int j = 0; j < f.T; ++j) f.bank[(size_t)ph * f.T + j] = plan_proto(*p, .5 * ph + (double)(f.T / 2 - 1 - j));
    } else {  // y[k] = sum_m v[m] g(2k - m), g(s) = H(s rho) rho (v at 2 f_out: rho owner-input samples per v sample)
        f.in_rate = 2. * fo; f.out_rate = fo; f.L = 1; f.M = 2;
        const int64_t tb = (int64_t)std::ceil((double)p->T / rho) + 2;
        f.T = (int32_t)((tb + 7) / 8 * 8);
        f.bank.assign((size_t)f.T, 0.);
        for (int j = 0; j < f.T; ++j) f.bank[j] = plan_proto(*p, (double)(f.T / 2 - 1 - j) * rho) * rho;
    }
}

// The polyphase stage: transparent over the band the FFT stage passes, stop band where its images begin.  Fills the
// stage's numbers in *ts and its prototype *h; false: no stage for this plan (too many taps, a table that would leave LDS,
// a ratio whose terms leave 2^31).
static bool poly_design(const Plan *p, TwoStage *ts, PolyProto *h)
{
    const double fi = p->in_rate, fo = p->out_rate;
    // in cycles per sample of ITS input: up: input at 2 f_in: pass 0.25 (= f_in/2), stop 0.75; down: input at f_in: pass
    // f_out/2, stop 1.5 f_out
    const double fpass = ts->up ? .25 : .5 * fo / fi, fstop = ts->up ? .75 : 1.5 * fo / fi;
    const double A = p->att_db + 6.;
    const double n_taps = (A - 7.95) / (2.285 * 2. * M_PI * (fstop - fpass)) + 1.;
    ts->T2 = 0;
#define HIPSOXR_POLY_T(t) if (!ts->T2 && t >= (int)std::ceil(n_taps)) ts->T2 = t;
    HIPSOXR_POLY_TAPS(HIPSOXR_POLY_T) // the kernel's instances, in rising order: the first that holds the design
#undef HIPSOXR_POLY_T
    if (!ts->T2) return false;
    // intervals of the cubic table: the interpolation error of a Chebyshev cubic over 1/P of a sample of this prototype is
    // about 0.03 / P^4 of full scale: 1.2e-10 at 128 (float64 table), 1.9e-9 at 64 (float32 table: two orders under the
    // float32 engine's floor, half the LDS — which is what lets several workgroups share a CU)
    ts->P2 = 128; ts->P2f = 64;
    ts->row = ts->T2 + 1;
    if ((size_t)ts->P2 * ts->row * 16 > 100 * 1024) return false;
    // output k of the polyphase stage at k * Ms / Ls input samples: up: from 2 f_in to f_out: 2 M / L; down: from f_in to
    // 2 f_out: M / (2 L)
    const int64_t a = ts->up ? 2 * p->M : p->M, b = ts->up ? p->L : 2 * p->L, g = gcd64(a, b);
    ts->Ms = a / g; ts->Ls = b / g;
    if (ts->Ms > (1LL << 31) || ts->Ls > (1LL << 31)) return false;
    h->fc = .5 * (fpass + fstop); h->W = .5 * ts->T2; h->beta = .1102 * (A - 8.7); h->inv_i0 = 1. / bessel_i0(h->beta); h->scale = 1.;
    double sum = 0.;
    for (int64_t m = -32 * ts->T2; m < 32 * ts->T2; ++m) sum += (*h)((double)m / 64.);
    h->scale = 64. / sum;
    return true;
}

// [P][row] records a0..a3: the cubic per (interval, tap) through the four Chebyshev nodes of the interval, monomials in x
// in [0, 1).  (plan.cpp fits its interpolated banks the same way but associates the products differently — d012 * p01
// there, d012 * node[0] * node[1] here — so sharing the fit would move this table's bits: the two stay apart.)
static std::vector<double> poly_cubic_table(const PolyProto &h, int P, int T2, int row)
{
    double node[4];
    for (int c = 0; c < 4; ++c) node[c] = .5 - .5 * std::cos((double)(2 * c + 1) * M_PI / 8.);
    std::vector<double> tab((size_t)P * row * 4, 0.);
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < T2; ++j) {
            double v[4];
            for (int c = 0; c < 4; ++c) v[c] = h(((double)i + node[c]) / P + (double)(T2 / 2 - 1 - j));
            const double d01 = (v[1] - v[0]) / (node[1] - node[0]), d12 = (v[2] - v[1]) / (node[2] - node[1]), d23 = (v[3] - v[2]) / (node[3] - node[2]);
            const double d012 = (d12 - d01) / (node[2] - node[0]), d123 = (d23 - d12) / (node[3] - node[1]);
            const double d3 = (d123 - d012) / (node[3] - node[0]);
            double *a = &tab[((size_t)i * row + j) * 4];
            a[3] = d3;
            a[2] = d012 - d3 * (node[0] + node[1] + node[2]);
            a[1] = d01 - d012 * (node[0] + node[1]) + d3 * (node[0] * node[1] + node[0] * node[2] + node[1] * node[2]);
            a[0] = v[0] - d01 * node[0] + d012 * node[0] * node[1] - d3 * node[0] * node[1] * node[2];
        }
    return tab;
}

template <typename T>
static const char *upload(void **dev, const std::vector<T> &host)
{
    HIP_TRY(hipMalloc(dev, host.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return nullptr;
}

static const char *twostage_build(Plan *p)
{
    TwoStage *ts = new TwoStage;
    p->two = ts;
    if (!p->phases || p->q.bits < 20. || p->proto_scale == 0. || p->custom_bank) return nullptr; // HQ / VHQ windowed-sinc interpolated plans only
    const double fi = p->in_rate, fo = p->out_rate;
    ts->up = fo > fi;
    const double rho = ts->up ? 1. : fi / (2. * fo); // polyphase stage: input samples per output sample is rho (down) / Ms/Ls (up)
    if (!ts->up && fi / fo > 4.) return nullptr;      // (long polyphase filters: the table would leave LDS)
    twostage_fft_plan(p, ts->up, rho, ts->fft);
    PolyProto h;
    if (!poly_design(p, ts, &h)) return nullptr;
    const std::vector<double> tab = poly_cubic_table(h, ts->P2, ts->T2, ts->row), tab64 = poly_cubic_table(h, ts->P2f, ts->T2, ts->row);
    const std::vector<float> tabf(tab64.begin(), tab64.end());
    if (const char *e = upload(&ts->tab_f, tabf)) return e;
    if (const char *e = upload(&ts->tab_d, tab)) return e;
    ts->ok = true;
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// k_poly: outputs [k_lo, k_lo + n_out) of one column per workgroup tile; output k at src position k * Ms / Ls;
//   y[k] = sum_j c_j(frac) src[floor(pos) - (T/2 - 1) + j],   c_j(f) = cubic of table[floor(f P)][j] at x = f P - floor(f P)
// The table and the tile's source span live in LDS; a thread owns R consecutive outputs (position by one 64-bit division,
// then increments).
// ---------------------------------------------------------------------------------------------
struct PolyArgs {
    const void *src; void *dst; const void *tab;
    int32_t T, P, row, R, span_max, lane_mul, lgP;
    int32_t lg_cg;     // a workgroup takes 2^lg_cg neighbouring channels of a tile one after the other (interleaved data: their parts of a line meet in one L2)
    unsigned long long *trace; // -DPOLY_TRACE builds: per-wave cycle sums [workgroup][wave][8]
    uint64_t step_fx;  // frac(Ms / Ls) in units of 2^-64 (float32 path of k_poly)
    double fx_per_rem; // 2^64 / Ls
    int64_t Ls, Ms, Mq, Mr; // Ms = Mq * Ls + Mr
    int64_t n_lo, n_src, k_lo, n_out; // the source column holds samples [n_lo, n_src) (src points at sample 0; zero outside); outputs [k_lo, k_lo + n_out), k_lo may be < 0
    int64_t scs, sfs, schs, dcs, dfs, dchs;
    uint32_t n_channels;
    // k_poly2<.., IL = false>: member 2 of a split column — element offsets of its sample n / output k from the column's,
    // its sample n = the column's n + m2_shift, and how many outputs it has (member 1 has n_out)
    int64_t m2_src, m2_dst, m2_shift, m2_n_out;
};

struct PolyArgsR : PolyArgs {
    const int64_t *rows; // [columns][4] = src offset of sample 0, n_src, dst offset, n_out (device; elements from src / dst)
};
template <bool RAGGED> struct PolyArgsOf { typedef PolyArgs type; };
template <> struct PolyArgsOf<true> { typedef PolyArgsR type; };
__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the arguments as one column's kernel sees them: the equal-length block itself, or a copy with the column's row put in
// (the launcher passes one channel, no channel group and clip strides of 0: column = blockIdx.y)
template <typename Real> __device__ __forceinline__ const PolyArgs &poly_column_args(const PolyArgs &a, PolyArgs &) { return a; }
template <typename Real> __device__ __forceinline__ const PolyArgs &poly_column_args(const PolyArgsR &r, PolyArgs &v)
{
    const int64_t *row = r.rows + 4 * (int64_t)blockIdx.y;
    v = r;
    v.src = (const Real *)r.src + uniform64(row[0]); v.n_src = uniform64(row[1]);
    v.dst = (Real *)r.dst + uniform64(row[2]); v.n_out = uniform64(row[3]);
    return v;
}

__device__ __forceinline__ int64_t poly_floor_div(int64_t q, int64_t d) // d > 0
{
    const int64_t n = q / d;
    return n * d > q ? n - 1 : n;
}
template <typename Real> struct Rec4;
template <> struct Rec4<float> { typedef float4 type; };
template <> struct Rec4<double> { typedef double4 type; };

// The position arithmetic of the polyphase stage, shared by k_poly, k_poly2 and k_poly_adj — one definition per element width,
// so that the transpose multiplies by the coefficients of the very (n_k, interval, x) the forward used.
// float32 path: output k sits at k_lo's exact position (one 64-bit division per thread and launch) plus (k - k_lo) steps of
// Ms / Ls as a 64.64 binary fraction (step_fx is truncated: at most 2^-33 of a sample short after 2^31 outputs — a position
// that is exactly an integer may land one sample lower with a fraction just under 1).
struct PolyFx { int64_t nK0; uint64_t phK0; };
__device__ __forceinline__ PolyFx poly_fx_origin(const PolyArgs &a)
{
    PolyFx o;
    o.nK0 = poly_floor_div(a.k_lo * a.Ms, a.Ls);
    o.phK0 = (uint64_t)((double)(a.k_lo * a.Ms - o.nK0 * a.Ls) * a.fx_per_rem); // remainder / Ls in units of 2^-64
    return o;
}
// ... output k's sample n_k (returned) and fraction `ph`, from the origin: a closure over the kernel's own variables (this shape,
// and each helper's below, is the one that leaves k_poly's instances instruction for instruction what they were)
struct PolyPosFx {
    const PolyArgs &a; const int64_t &nK0; const uint64_t &phK0;
    __device__ int64_t operator()(int64_t k, uint64_t &ph) const
    {
        const uint64_t dk = (uint64_t)(k - a.k_lo), lo = dk * a.step_fx;
        ph = phK0 + lo;
        return nK0 + (int64_t)dk * a.Mq + (int64_t)__umul64hi(dk, a.step_fx) + (ph < lo ? 1 : 0);
    }
};
// ... the table interval and the cubic's argument of a 64-bit fraction
__device__ __forceinline__ void poly_fx_interval(uint64_t phase, int lg, uint32_t &i, float &x)
{
    const uint32_t hi = (uint32_t)(phase >> 32);
    i = hi >> (32 - lg);
    x = (float)(uint32_t)(hi << lg) * 0x1p-32f;
}
// float64 path (and float32 beyond MQ = 1): the exact rational position, k Ms = n Ls + rem, and the interval of rem / Ls
__device__ __forceinline__ int64_t poly_exact_n(const PolyArgs &a, int64_t k) { return poly_floor_div(k * a.Ms, a.Ls); }
__device__ __forceinline__ int64_t poly_exact_rem(const PolyArgs &a, int64_t k, int64_t n) { return k * a.Ms - n * a.Ls; }
// ... f P, the interval floor(f P) — guarded against f P == P by rounding — and the cubic's argument.  (k_poly applies the
// guard in its own text, the two lines of poly_exact_interval: moved into a function there, it reorders operands of two of
// that kernel's additions.)
__device__ __forceinline__ double poly_exact_fp(int64_t rem, double invL, int P) { return (double)rem * invL * (double)P; }
template <typename Real> __device__ __forceinline__ Real poly_exact_x(double fP, int i) { return (Real)(fP - (double)i); }
template <typename Real>
__device__ __forceinline__ void poly_exact_interval(int64_t rem, double invL, int P, int &i, Real &x)
{
    const double fP = poly_exact_fp(rem, invL, P);
    i = (int)fP;
    if (i >= P) i = P - 1;
    x = poly_exact_x<Real>(fP, i);
}

// TT = taps (compile time: the tap loop unrolls and every LDS read of an output is in flight at once).
// MQ = floor(Ms / Ls) when that is 0 or 1 (every ratio the two-stage form takes but down-sampling beyond 2:1): consecutive
// outputs' source windows then differ by MQ or MQ + 1 samples, and the thread keeps its window in REGISTERS, shifted by
// v_cndmask between outputs, with two fresh samples read per output instead of TT — the table records are then the only
// per-tap LDS traffic.  MQ = -1: the window is re-read from LDS for every output.
//
// RAGGED (a clip table on the two-stage form, launch_two_stage_ragged): a second instantiation, `bool RAGGED`, whose argument
// block carries a device table behind the usual arguments (the equal-length instances keep theirs, instruction for
// instruction).  The launch has one channel and one grid row per (clip, channel) COLUMN; a workgroup's column reads its row
// {src offset of sample 0, n_src, dst offset, n_out} — four int64, elements, built by the library (poly_rules.h
// ragged_poly_plan) — in place of the job-wide n_src / n_out and the clip and channel strides; n_lo and k_lo stay job-wide
// (they depend on the plan's pad alone).  The row address is wave-uniform (blockIdx.y) and its values stay on the scalar
// side.  R, the lane order and the LDS size are the launch's, chosen from the LONGEST column, and so is the grid's x: the
// tile count is the column's own, the persistent walk breaks at it, and a workgroup whose first tile lies at or behind its
// column's end leaves before the table is copied to LDS and before the first barrier — a decision on block index and row
// alone, so no barrier is met by part of a workgroup.
template <typename Real, int TT, int MQ, bool RAGGED = false>
__global__ void __launch_bounds__(256) k_poly(typename PolyArgsOf<RAGGED>::type a_)
{
    typedef typename Rec4<Real>::type R4;
    PolyArgs a_row;
    const PolyArgs &a = poly_column_args<Real>(a_, a_row);
    if (RAGGED && ragged_span_skip(blockIdx.x, 256LL * a.R, a.n_out)) return; // (uniform: none of this column's tiles is this workgroup's)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R4 *tab = reinterpret_cast<R4 *>(smem);
    Real *xs = reinterpret_cast<Real *>(smem + (size_t)a.P * a.row * sizeof(R4));
    Real *ys = xs + a.span_max; // the tile's outputs, staged [R][257] so that they leave as whole lines whatever the lane order
    const int cg = 1 << a.lg_cg;
    const uint32_t col = blockIdx.y << a.lg_cg, ch = col % a.n_channels, clip = col / a.n_channels; // first channel of the group
    const Real *src0 = (const Real *)a.src + (int64_t)clip * a.scs + (int64_t)ch * a.schs;
    Real *dst = (Real *)a.dst + (int64_t)clip * a.dcs + (int64_t)ch * a.dchs;
    const int tid = (int)threadIdx.x;
    {
        const R4 *g = (const R4 *)a.tab;
        for (int i = tid; i < a.P * a.row; i += 256) tab[i] = g[i];
    }
    const int64_t per_tile = 256LL * a.R, n_tiles = (a.n_out + per_tile - 1) / per_tile;
    constexpr int H = TT / 2;
    constexpr int CH = TT % 16 == 0 ? 16 : TT % 12 == 0 ? 12 : TT % 8 == 0 ? 8 : 4; // taps whose LDS reads are in flight together
#ifdef POLY_TRACE
    unsigned long long tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tq = __builtin_amdgcn_s_memtime();
    const unsigned long long tq0 = tq;
#define POLY_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tr[i] += t_ - tq; tq = t_; } while (0)
#else
#define POLY_STAMP(i) ((void)0)
#endif
    constexpr bool FAST = sizeof(Real) == 4 && MQ >= 0;
    // float32 path: output k sits at k_lo's exact position (one 64-bit division per thread and launch) plus (k - k_lo) steps of
    // Ms / Ls as a 64.64 binary fraction (step_fx is truncated: at most 2^-33 of a sample short after 2^31 outputs); the tile's
    // span and every thread's window come from the same arithmetic
    int64_t nK0 = 0;
    uint64_t phK0 = 0;
    if constexpr (FAST) {
        const PolyFx o = poly_fx_origin(a);
        nK0 = o.nK0; phK0 = o.phK0;
    }
    const PolyPosFx position{a, nK0, phK0};
    const int slot = (tid * a.lane_mul) & 255; // this thread's run of R outputs within a tile
    constexpr int NPF = FAST ? 8 : 0; // float32 path: samples per thread of the NEXT tile's span held in registers
    Real pf[NPF > 0 ? NPF : 1];
    auto fetch = [&](int64_t tile, int c) {
        const Real *src = src0 + (int64_t)c * a.schs;
        const int64_t kA = a.k_lo + tile * per_tile, kEnd = a.k_lo + a.n_out, kB = (kA + per_tile < kEnd ? kA + per_tile : kEnd) - 1;
        uint64_t ph;
        const int64_t nA = position(kA, ph) - (H - 1), nB = position(kB, ph) + H;
#pragma unroll
        for (int q = 0; q < NPF; ++q) {
            const int64_t n = nA + q * 256 + tid;
            pf[q] = (n <= nB && n >= a.n_lo && n < a.n_src) ? src[n * a.sfs] : (Real)0;
        }
    };
    if constexpr (FAST)
        if ((int64_t)blockIdx.x < n_tiles) fetch(blockIdx.x, 0);
    // work items: (tile, channel of the group), channels innermost
    for (int64_t item = 0;; ++item) {
        const int64_t tile = blockIdx.x + (item >> a.lg_cg) * gridDim.x;
        if (tile >= n_tiles) break;
        const int c = (int)(item & (cg - 1));
        const Real *src = src0 + (int64_t)c * a.schs;
        Real *ysc = ys;
        const int64_t kA = a.k_lo + tile * per_tile;
        const int64_t kEnd = a.k_lo + a.n_out, kB = (kA + per_tile < kEnd ? kA + per_tile : kEnd) - 1;
        // (|k| < 2^31 and Ms <= 2^31: the products fit 64 bits — launch_two_stage admits no larger job)
        int64_t nA, nB;
        if constexpr (FAST) {
            uint64_t ph;
            nA = position(kA, ph) - (H - 1); nB = position(kB, ph) + H;
        } else {
            nA = poly_floor_div(kA * a.Ms, a.Ls) - (H - 1); nB = poly_floor_div(kB * a.Ms, a.Ls) + H;
        }
        const int span = (int)(nB - nA + 1);
        if constexpr (FAST) { // the first NPF * 256 samples were fetched while the tile before was being computed
#pragma unroll
            for (int q = 0; q < NPF; ++q)
                if (q * 256 + tid < span) xs[q * 256 + tid] = pf[q];
        }
        for (int i = NPF * 256 + tid; i < span; i += 256) {
            const int64_t n = nA + i;
            xs[i] = (n >= a.n_lo && n < a.n_src) ? src[n * a.sfs] : (Real)0;
        }
        POLY_STAMP(0); // span staged (loads issued and written)
        __syncthreads();
        POLY_STAMP(1); // barrier
        if constexpr (FAST) { // the next item's span: in flight behind this item's arithmetic
            const int64_t tn = blockIdx.x + ((item + 1) >> a.lg_cg) * gridDim.x;
            if (tn < n_tiles) fetch(tn, (int)((item + 1) & (cg - 1)));
        }
        const int64_t k1 = kA + (int64_t)slot * a.R;
        if constexpr (sizeof(Real) == 4 && MQ >= 0) {
            // float32, window in registers: the position is a 64-bit binary fraction stepped by frac(Ms / Ls) 2^64 (its
            // carry moves the window on), the sums over taps are taken per cubic coefficient — S_d = sum_j a_d[j] u[j],
            // two coefficients per v_pk_fma_f32 straight from the 16-byte record, the sample broadcast by op_sel — and
            // y = S0 + x (S1 + x (S2 + x S3)): two packed instructions per tap instead of four scalar ones.
            typedef float v2f __attribute__((ext_vector_type(2)));
            typedef float v4f __attribute__((ext_vector_type(4)));
            if (k1 <= kB) {
                uint64_t phase;
                const int64_t n0 = position(k1, phase);
                const float *w = xs + (n0 - nA - (H - 1));
                v2f u[TT / 2];
#pragma unroll
                for (int j = 0; j < TT / 2; ++j) { u[j].x = w[2 * j]; u[j].y = w[2 * j + 1]; }
                const float *wtop = w + (TT - 2);
                const v4f *tabv = reinterpret_cast<const v4f *>(tab);
                float *yo = ysc + slot; // staged [run index][slot] with rows of 257: conflict-free writes
                const int lg = a.lgP;
                int left = (int)(kB - k1 + 1 < (int64_t)a.R ? kB - k1 + 1 : (int64_t)a.R);
                for (; left > 0; --left) {
                    uint32_t i;
                    float x;
                    poly_fx_interval(phase, lg, i, x);
                    const v4f *row = tabv + i * (uint32_t)a.row;
                    v2f s01e = {0.f, 0.f}, s23e = {0.f, 0.f}, s01o = {0.f, 0.f}, s23o = {0.f, 0.f};
#pragma unroll
                    for (int j0 = 0; j0 < TT; j0 += CH) {
                        v4f c[CH];
#pragma unroll
                        for (int j = 0; j < CH; ++j) c[j] = row[j0 + j];
#pragma unroll
                        for (int j = 0; j < CH; j += 2) {
                            const v2f a01 = __builtin_shufflevector(c[j], c[j], 0, 1), a23 = __builtin_shufflevector(c[j], c[j], 2, 3);
                            const v2f b01 = __builtin_shufflevector(c[j + 1], c[j + 1], 0, 1), b23 = __builtin_shufflevector(c[j + 1], c[j + 1], 2, 3);
                            const v2f up = u[(j0 + j) / 2];
                            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(s01e) : "v"(a01), "v"(up), "v"(s01e));
                            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(s23e) : "v"(a23), "v"(up), "v"(s23e));
                            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(s01o) : "v"(b01), "v"(up), "v"(s01o));
                            asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(s23o) : "v"(b23), "v"(up), "v"(s23o));
                        }
                    }
                    const float S0 = s01e.x + s01o.x, S1 = s01e.y + s01o.y, S2 = s23e.x + s23o.x, S3 = s23e.y + s23o.y;
                    *yo = ((S3 * x + S2) * x + S1) * x + S0;
                    yo += 257;
                    const uint64_t next = phase + a.step_fx;
                    const bool adv = next < phase; // the fraction wrapped: one more sample
                    phase = next;
                    wtop += MQ + (adv ? 1 : 0);
                    const float e0 = wtop[0], e1 = wtop[1]; // (the span has 4 spare words behind the last window)
                    float f[TT];
#pragma unroll
                    for (int j = 0; j < TT / 2; ++j) { f[2 * j] = u[j].x; f[2 * j + 1] = u[j].y; }
#pragma unroll
                    for (int j = 0; j < TT - 2; ++j) f[j] = adv ? f[j + MQ + 1] : f[j + MQ];
                    f[TT - 2] = e0; f[TT - 1] = e1;
#pragma unroll
                    for (int j = 0; j < TT / 2; ++j) { u[j].x = f[2 * j]; u[j].y = f[2 * j + 1]; }
                }
            }
        } else
        if (k1 <= kB) {
            int64_t n = poly_exact_n(a, k1);
            int64_t rem = poly_exact_rem(a, k1, n);
            const double invL = 1. / (double)a.Ls;
            Real u[TT];
            if constexpr (MQ >= 0) {
                const Real *w = xs + (n - nA - (H - 1));
#pragma unroll
                for (int j = 0; j < TT; ++j) u[j] = w[j];
            }
            for (int r = 0; r < a.R && k1 + r <= kB; ++r) {
                const double fP = poly_exact_fp(rem, invL, a.P);
                int i = (int)fP;
                if (i >= a.P) i = a.P - 1;
                const Real x = poly_exact_x<Real>(fP, i);
                const R4 *row = tab + (size_t)i * a.row;
                const Real *w = xs + (n - nA - (H - 1));
                Real acc0 = (Real)0, acc1 = (Real)0;
#pragma unroll
                for (int j0 = 0; j0 < TT; j0 += CH) {
                    R4 c[CH];
                    Real v[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        c[j] = row[j0 + j];
                        if constexpr (MQ >= 0) v[j] = u[j0 + j];
                        else v[j] = w[j0 + j];
                    }
#pragma unroll
                    for (int j = 0; j < CH; j += 2) {
                        acc0 += (((c[j].w * x + c[j].z) * x + c[j].y) * x + c[j].x) * v[j];
                        acc1 += (((c[j + 1].w * x + c[j + 1].z) * x + c[j + 1].y) * x + c[j + 1].x) * v[j + 1];
                    }
                }
                ysc[r * 257 + slot] = acc0 + acc1;
                n += a.Mq; rem += a.Mr;
                const bool adv = rem >= a.Ls;
                if (adv) { rem -= a.Ls; ++n; }
                if constexpr (MQ >= 0) { // the window moves on by MQ or MQ + 1 samples (the span has 4 spare words behind the last window)
                    const Real *wn = xs + (n - nA - (H - 1));
                    const Real e0 = wn[TT - 2], e1 = wn[TT - 1];
#pragma unroll
                    for (int j = 0; j < TT - 2; ++j) u[j] = adv ? u[j + MQ + 1] : u[j + MQ];
                    u[TT - 2] = e0; u[TT - 1] = e1;
                }
            }
        }
        POLY_STAMP(2); // outputs computed
        __syncthreads(); // the tile's outputs are staged (and its source span is free for the next tile)
        POLY_STAMP(3); // barrier
        { // (the channels of a group leave one after the other from the same workgroup: their halves of a line meet in its XCD's L2)
            Real *yo = dst + (kA - a.k_lo) * a.dfs + (int64_t)c * a.dchs;
            const int cnt = (int)(kB - kA + 1);
            const float invR = 1.f / (float)a.R;
            for (int i = tid; i < cnt; i += 256) {
                const int sl = (int)(((float)i + .5f) * invR), r = i - sl * a.R; // output i of the tile: run index r of slot sl
                yo[(int64_t)i * a.dfs] = ys[r * 257 + sl];
            }
        }
        POLY_STAMP(4); // outputs stored
    }
#ifdef POLY_TRACE
    if (a.trace && (tid & 63) == 0) {
        unsigned long long *o = a.trace + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid / 64) * 8;
        for (int i = 0; i < 5; ++i) o[i] = tr[i];
        o[5] = tq0; o[6] = tq; o[7] = __builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); // HW_ID, XCC_ID
    }
#endif
}

// k_poly2: the float32 register-window form of k_poly for a PAIR of interleaved channels (both ends of the stage channel-
// interleaved, e.g. stereo): a thread produces R consecutive FRAMES of the pair.  The two channels of a frame share the
// position, the table row and the cubic's argument, so one set of 16-byte record reads serves both (half the per-tap LDS
// traffic of two k_poly passes), the packed FMAs run over the channel pair — s_d += a_d[j] * (left, right)[j], the
// coefficient broadcast by op_sel — and source frames / output frames move as 8-byte words (whole lines in ONE pass over
// the data instead of half lines in two).  Same arithmetic per channel as k_poly's (sums per cubic coefficient, then
// Horner), in tap order instead of even / odd halves: results agree to rounding.
// IL = false — any OTHER column (mono, planar, odd channel counts): the pair is two SEGMENTS OF ONE COLUMN a whole number of
// phase periods apart.  Output k + h Ls sits exactly h Ms source samples behind output k (positions are k Ms / Ls), so the
// two have the same fraction — the same table row and argument — for every k: member 2 of the pair is the column from
// output h Ls on (PolyArgs::m2_*; launch_poly picks h = half the job's periods), read and written as 4-byte words.
template <int TT, int MQ, bool IL>
#ifndef POLY2_OCC
#define POLY2_OCC 3
#endif
__global__ void __launch_bounds__(256, TT >= 32 ? 2 : POLY2_OCC) k_poly2(PolyArgs a) // (two windows of 32+ frames: 2 workgroups per CU, launch_poly sizes the tile for that)
{
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v4f *tab = reinterpret_cast<v4f *>(smem);
    v2f *xs = reinterpret_cast<v2f *>(smem + (size_t)a.P * a.row * sizeof(v4f));
    v2f *ys = xs + a.span_max; // the tile's output frames, staged [R][257]
    const int cg = 1 << a.lg_cg; // channel PAIRS (IL) / channels a workgroup takes one after the other
    const uint32_t col = (blockIdx.y << a.lg_cg) * (IL ? 2 : 1), ch = col % a.n_channels, clip = col / a.n_channels; // first channel of the group
    const int64_t c_src = IL ? 2 : a.schs, c_dst = IL ? 2 : a.dchs; // from one item of the group to the next
    const float *src0 = (const float *)a.src + (int64_t)clip * a.scs + (int64_t)ch * (IL ? 1 : a.schs);
    float *dst0 = (float *)a.dst + (int64_t)clip * a.dcs + (int64_t)ch * (IL ? 1 : a.dchs);
    const int tid = (int)threadIdx.x;
    const int64_t per_tile = 256LL * a.R, n_tiles = (a.n_out + per_tile - 1) / per_tile;
    constexpr int H = TT / 2;
#ifdef POLY2_CH
    constexpr int CH = TT % POLY2_CH == 0 ? POLY2_CH : 4;
#else
    constexpr int CH = TT % 16 == 0 ? 16 : TT % 12 == 0 ? 12 : TT % 8 == 0 ? 8 : 4; // taps whose LDS reads are in flight together
#endif
    const int64_t nK0 = poly_floor_div(a.k_lo * a.Ms, a.Ls); // (poly_fx_origin's two lines)
    const uint64_t phK0 = (uint64_t)((double)(a.k_lo * a.Ms - nK0 * a.Ls) * a.fx_per_rem);
    const PolyPosFx position{a, nK0, phK0}; // (as in k_poly)
    const int slot = (tid * a.lane_mul) & 255;
#ifdef POLY_TRACE
    unsigned long long tr[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tq = __builtin_amdgcn_s_memtime();
    const unsigned long long tq0 = tq;
#endif
    constexpr int NPF = 12; // frames per thread of the NEXT tile's span held in registers (launch_poly keeps the span within 12 x 256)
    v2f pf[NPF];
    const v2f zero = {0.f, 0.f};
    // one frame of the pair at a source position: 8 bytes (IL) or a sample of each member, each with its own range
    auto load2 = [&](const float *q, bool in1, bool in2) -> v2f {
        if constexpr (IL) return in1 ? *reinterpret_cast<const v2f *>(q) : zero;
        else { v2f r; r.x = in1 ? q[0] : 0.f; r.y = in2 ? q[a.m2_src] : 0.f; return r; }
    };
    auto fetch = [&](int64_t tile, int c) {
        const float *src = src0 + c * c_src;
        const int64_t kA = a.k_lo + tile * per_tile, kEnd = a.k_lo + a.n_out, kB = (kA + per_tile < kEnd ? kA + per_tile : kEnd) - 1;
        uint64_t ph;
        const int64_t nA = position(kA, ph) - (H - 1), nB = position(kB, ph) + H;
        // frames [lo, hi) of the span exist (uniform, 32-bit from here on: one unsigned compare and one pointer step per load)
        const int64_t lo64 = a.n_lo - nA, hi64 = (nB + 1 < a.n_src ? nB + 1 : a.n_src) - nA;
        const int lo = (int)(lo64 < 0 ? 0 : lo64 > NPF * 256 ? NPF * 256 : lo64), hi = (int)(hi64 < lo ? lo : hi64 > NPF * 256 ? NPF * 256 : hi64);
        // (member 2 of a split column: its sample n is the column's n + m2_shift)
        const int64_t lo64b = lo64 - a.m2_shift, hi64b = (nB + 1 < a.n_src - a.m2_shift ? nB + 1 : a.n_src - a.m2_shift) - nA;
        const int lo2 = IL ? 0 : (int)(lo64b < 0 ? 0 : lo64b > NPF * 256 ? NPF * 256 : lo64b), hi2 = IL ? 0 : (int)(hi64b < lo2 ? lo2 : hi64b > NPF * 256 ? NPF * 256 : hi64b);
        const float *p = src + (nA + tid) * a.sfs;
        const int64_t step = 256 * a.sfs;
#pragma unroll
        for (int q = 0; q < NPF; ++q, p += step)
            pf[q] = load2(p, (unsigned)(q * 256 + tid - lo) < (unsigned)(hi - lo), (unsigned)(q * 256 + tid - lo2) < (unsigned)(hi2 - lo2));
    };
    if ((int64_t)blockIdx.x < n_tiles) fetch(blockIdx.x, 0);
    { // (the table behind the first span's loads: one round trip for both)
        const v4f *g = (const v4f *)a.tab;
        for (int i = tid; i < a.P * a.row; i += 256) tab[i] = g[i];
    }
    // (staging the next span BEFORE this tile's stores — gfx9 retires loads and stores through one in-order counter — was
    //  measured: no gain at 16 taps, 50 -> 55 us at 40; profiles/r05_ab_experiments.txt §7)
    for (int64_t item = 0;; ++item) { // work items: (tile, channel pair of the group), pairs innermost
        const int64_t tile = blockIdx.x + (item >> a.lg_cg) * gridDim.x;
        if (tile >= n_tiles) break;
        const int c = (int)(item & (cg - 1));
        const float *src = src0 + c * c_src;
        const int64_t kA = a.k_lo + tile * per_tile;
        const int64_t kEnd = a.k_lo + a.n_out, kB = (kA + per_tile < kEnd ? kA + per_tile : kEnd) - 1;
        uint64_t ph_;
        const int64_t nA = position(kA, ph_) - (H - 1), nB = position(kB, ph_) + H;
        const int span = (int)(nB - nA + 1);
#pragma unroll
        for (int q = 0; q < NPF; ++q)
            if (q * 256 + tid < span) xs[q * 256 + tid] = pf[q];
        for (int i = NPF * 256 + tid; i < span; i += 256) { // (not reached with launch_poly's run lengths)
            const int64_t n = nA + i;
            xs[i] = load2(src + n * a.sfs, n >= a.n_lo && n < a.n_src, n >= a.n_lo - a.m2_shift && n < a.n_src - a.m2_shift);
        }
        POLY_STAMP(0);
        __syncthreads();
        POLY_STAMP(1);
        {
            const int64_t tn = blockIdx.x + ((item + 1) >> a.lg_cg) * gridDim.x;
            if (tn < n_tiles) fetch(tn, (int)((item + 1) & (cg - 1)));
        }
        const int64_t k1 = kA + (int64_t)slot * a.R;
        if (k1 <= kB) {
            uint64_t phase;
            const int64_t n0 = position(k1, phase);
            const v2f *w = xs + (n0 - nA - (H - 1));
            v2f u[TT];
#pragma unroll
            for (int j = 0; j < TT; ++j) u[j] = w[j];
            const v2f *wtop = w + (TT - 2);
            v2f *yo = ys + slot;
            const int lg = a.lgP;
            int left = (int)(kB - k1 + 1 < (int64_t)a.R ? kB - k1 + 1 : (int64_t)a.R);
            for (; left > 0; --left) {
                uint32_t i;
                float x;
                poly_fx_interval(phase, lg, i, x);
                const v4f *row = tab + i * (uint32_t)a.row;
                // the cubic per tap ONCE for both channels (three scalar FMAs), then one packed FMA over the channel pair
                // with the coefficient broadcast: 3 + 1 instructions per tap against k_poly's 2 x 2 for two channels
                v2f y0 = zero, y1 = zero;
#pragma unroll
                for (int j0 = 0; j0 < TT; j0 += CH) {
                    v4f cf[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) cf[j] = row[j0 + j];
#pragma unroll
                    for (int j = 0; j < CH; j += 2) { // (the value lands in the record's first register: its pair is the operand, low half broadcast)
                        cf[j].x = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(cf[j].w, x, cf[j].z), x, cf[j].y), x, cf[j].x);
                        cf[j + 1].x = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(cf[j + 1].w, x, cf[j + 1].z), x, cf[j + 1].y), x, cf[j + 1].x);
                        const v2f c0 = __builtin_shufflevector(cf[j], cf[j], 0, 1), c1 = __builtin_shufflevector(cf[j + 1], cf[j + 1], 0, 1);
                        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(y0) : "v"(c0), "v"(u[j0 + j]), "v"(y0));
                        asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(y1) : "v"(c1), "v"(u[j0 + j + 1]), "v"(y1));
                    }
                }
                *yo = y0 + y1;
                yo += 257;
                const uint64_t next = phase + a.step_fx;
                const bool adv = next < phase; // the fraction wrapped: one more frame
                phase = next;
                wtop += MQ + (adv ? 1 : 0);
                const v2f e0 = wtop[0], e1 = wtop[1]; // (the span has 4 spare frames behind the last window)
                // (explicit selects: left to the compiler, a select between two elements of the window becomes a dynamically
                //  indexed extract — a compare and a select per ELEMENT of the array.  v_cndmask with its mask in a scalar pair
                //  issues at half rate on gfx950, and so does v_bfi_b32 on a mask in a vector register — 4.4 and 4.7 cycles
                //  against 2.7 for v_fma_f32, tools/ubench/valu_ops.hip: the shift is a quarter of the loop's issue time)
                const uint64_t advm = __builtin_amdgcn_ballot_w64(adv);
#pragma unroll
                for (int j = 0; j < TT - 2; ++j) {
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(u[j].x) : "v"(u[j + MQ].x), "v"(u[j + MQ + 1].x), "s"(advm));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(u[j].y) : "v"(u[j + MQ].y), "v"(u[j + MQ + 1].y), "s"(advm));
                }
                u[TT - 2] = e0; u[TT - 1] = e1;
            }
        }
        POLY_STAMP(2);
        __syncthreads(); // the tile's outputs are staged and its source span is free
        POLY_STAMP(3);
        {
            float *yo = dst0 + c * c_dst + (kA - a.k_lo + tid) * a.dfs;
            const int64_t step = 256 * a.dfs;
            const int cnt = (int)(kB - kA + 1);
            const int64_t left2 = a.m2_n_out - (kA - a.k_lo); // (member 2 of a split column may end inside the tile)
            const int cnt2 = (int)(left2 < 0 ? 0 : left2 > cnt ? cnt : left2);
            const float invR = 1.f / (float)a.R;
            for (int i = tid; i < cnt; i += 256, yo += step) {
                const int sl = (int)(((float)i + .5f) * invR), r = i - sl * a.R; // frame i of the tile: run index r of slot sl
                const v2f y = ys[r * 257 + sl];
                if constexpr (IL) *reinterpret_cast<v2f *>(yo) = y;
                else {
                    yo[0] = y.x;
                    if (i < cnt2) yo[a.m2_dst] = y.y;
                }
            }
        }
        POLY_STAMP(4);
    }
#ifdef POLY_TRACE
    if (a.trace && (tid & 63) == 0) {
        unsigned long long *o = a.trace + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid / 64) * 8;
        for (int i = 0; i < 5; ++i) o[i] = tr[i];
        o[5] = tq0; o[6] = tq; o[7] = 0;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// k_poly_adj: the transpose of k_poly (HIPSOXR_KERNEL_ADJOINT_TWO_STAGE), in gather form — no atomics, a fixed order of
// additions: bitwise reproducible.  The argument block is k_poly's, read in the forward's direction: `dst` is the stage's
// output side and holds the cotangent gdst[k], k in [k_lo, k_lo + n_out) (READ here); `src` is its input side, and
// gsrc[n] is WRITTEN for every n in [n_lo, n_src):
//   gsrc[n] = sum over k in [k_lo, k_lo + n_out) with 0 <= j = n - n_k + T/2 - 1 < T  of  c_j(f_k) gdst[k]
// with (n_k, interval, x) from the forward's own device functions for the element width (poly_fx_* where k_poly takes its
// float32 path, poly_exact_* otherwise) — zeros where no output reaches.  A workgroup takes tiles of 256 R consecutive
// samples of one column (grid row = column, tiles walked by the workgroup: the table is copied to LDS once):
//   1. the outputs that can reach the tile (poly_adj_rules.h poly_adj_bracket: closed-form, conservative) are staged in LDS,
//      one per lane and pass: {gdst[k], x} and {n_k - n_A, row offset of the interval};
//   2. a thread owns R consecutive samples and walks the staged outputs that can reach them (poly_adj_run_span);
//      membership is decided per (k, sample) by 0 <= j < T, and the record [interval][j] gives the coefficient;
//   3. the tile's results are staged and leave as whole lines.
// Work: T Ls / Ms contributions per sample — the forward's multiply-accumulates for the same job.
// ---------------------------------------------------------------------------------------------
template <typename Real> struct Rec2;
template <> struct Rec2<float> { typedef float2 type; };
template <> struct Rec2<double> { typedef double2 type; };

// RAGGED (a clip table on the transposed form, launch_adjoint_two_stage_ragged): as for k_poly, a second instantiation whose
// argument block carries the device rows behind the usual arguments — the equal-length instances keep theirs, instruction for
// instruction.  One grid row per (clip, channel) COLUMN (blockIdx.y; one channel, clip strides 0); the column's row {src offset
// of sample 0, n_src, dst offset of output k_lo, n_out} — the FORWARD's poly row as it stands: dst is read, src written —
// replaces the job-wide n_src / n_out; n_lo and k_lo stay job-wide.  R and the LDS size do not depend on length
// (poly_adj_run), the grid's x axis is the longest column's: a workgroup whose first tile lies at or behind its column's end
// leaves before the table is copied and before the first barrier, and the tile loop's bound is the column's own — both
// uniform over the workgroup (block index and row alone), so no barrier is met by part of a workgroup.
template <typename Real, int TT, bool RAGGED = false>
__global__ void __launch_bounds__(256) k_poly_adj(typename PolyArgsOf<RAGGED>::type a_)
{
    typedef typename Rec4<Real>::type R4;
    typedef typename Rec2<Real>::type R2;
    PolyArgs a_row;
    const PolyArgs a = poly_column_args<Real>(a_, a_row); // (a copy: through a reference the equal-length instances' tile-count select changes by one instruction)
    if (RAGGED && ragged_span_skip(blockIdx.x, 256LL * a.R, a.n_src - a.n_lo)) return; // (uniform: none of this column's tiles is this workgroup's)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    R4 *tab = reinterpret_cast<R4 *>(smem);
    R2 *gs = reinterpret_cast<R2 *>(smem + (size_t)a.P * a.row * sizeof(R4)); // [span_max] {gdst[k], x}
    int2 *ni = reinterpret_cast<int2 *>(gs + a.span_max);                     // [span_max] {n_k - n_A, interval * row}
    Real *ys = reinterpret_cast<Real *>(ni + a.span_max);                     // [256 R] the tile's results
    const uint32_t col = blockIdx.y, ch = col % a.n_channels, clip = col / a.n_channels;
    Real *gsrc = const_cast<Real *>((const Real *)a.src) + (int64_t)clip * a.scs + (int64_t)ch * a.schs;
    const Real *gdst = (const Real *)a.dst + (int64_t)clip * a.dcs + (int64_t)ch * a.dchs;
    const int tid = (int)threadIdx.x;
    {
        const R4 *g = (const R4 *)a.tab;
        for (int i = tid; i < a.P * a.row; i += 256) tab[i] = g[i];
    }
    constexpr int H = TT / 2;
    const bool fast = sizeof(Real) == 4 && (a.Mq == 0 || a.Mq == 1); // k_poly's FAST instances
    PolyFx fx0 = {0, 0};
    if (fast) fx0 = poly_fx_origin(a);
    const PolyPosFx position{a, fx0.nK0, fx0.phK0};
    const double invL = 1. / (double)a.Ls;
    const int R = a.R;
    const int64_t per_tile = 256LL * R, n_tiles = (a.n_src - a.n_lo + per_tile - 1) / per_tile;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t nA = a.n_lo + tile * per_tile, nB = (nA + per_tile < a.n_src ? nA + per_tile : a.n_src) - 1;
        const PolyAdjSpan sp = poly_adj_bracket(nA, nB, TT, a.Ls, a.Ms, a.k_lo, a.n_out);
        const int64_t cnt64 = sp.k_last - sp.k_first + 1;
        const int cnt = (int)(cnt64 < 0 ? 0 : cnt64 > a.span_max ? a.span_max : cnt64); // (never above span_max: poly_adj_span_max)
        for (int s = tid; s < cnt; s += 256) {
            const int64_t k = sp.k_first + s;
            int64_t n;
            int i;
            Real x;
            if (fast) {
                uint64_t ph;
                uint32_t iu;
                float xf;
                n = position(k, ph);
                poly_fx_interval(ph, a.lgP, iu, xf);
                i = (int)iu; x = (Real)xf;
            } else {
                n = poly_exact_n(a, k);
                poly_exact_interval<Real>(poly_exact_rem(a, k, n), invL, a.P, i, x);
            }
            R2 g;
            g.x = gdst[(k - a.k_lo) * a.dfs]; g.y = x;
            gs[s] = g;
            ni[s] = make_int2((int)(n - nA), i * a.row);
        }
        __syncthreads();
        const int64_t n0 = nA + (int64_t)tid * R;
        Real acc[kPolyAdjRunMax];
#pragma unroll
        for (int r = 0; r < kPolyAdjRunMax; ++r) acc[r] = (Real)0;
        if (n0 <= nB && cnt > 0) {
            const int64_t n1 = n0 + R - 1 < nB ? n0 + R - 1 : nB;
            int sF, sL;
            poly_adj_run_span(n0, n1, TT, sp.k_first, a.Ls, a.Ms, cnt, &sF, &sL);
            const int base = (int)(n0 - nA) + H - 1;
            for (int s = sF; s <= sL; ++s) {
                const int2 q = ni[s];
                const R2 g = gs[s];
                const int j0 = base - q.x; // j of the run's first sample
#pragma unroll
                for (int r = 0; r < kPolyAdjRunMax; ++r) {
                    // (no branch: a tap outside [0, T) reads record T of the row — the table's spreading record, all zeros.
                    //  Samples r >= R of a shorter run are computed and not stored.)
                    const int j = j0 + r, jj = (unsigned)j < (unsigned)TT ? j : TT;
                    const R4 c = tab[q.y + jj];
                    acc[r] += (((c.w * g.y + c.z) * g.y + c.y) * g.y + c.x) * g.x;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kPolyAdjRunMax; ++r)
            if (r < R) ys[tid * R + r] = acc[r];
        __syncthreads(); // the tile's results are staged (and its staged outputs are free for the next tile)
        {
            Real *go = gsrc + nA * a.sfs;
            const int n_res = (int)(nB - nA + 1);
            for (int i = tid; i < n_res; i += 256) go[(int64_t)i * a.sfs] = ys[i];
        }
    }
}

// k_poly_adj's instances: one per tap count of HIPSOXR_POLY_TAPS and element type
template <typename Real, bool RAGGED = false>
static void (*poly_adj_kernel(int T2))(typename PolyArgsOf<RAGGED>::type)
{
    switch (T2) {
#define HIPSOXR_POLY_T(t) case t: return k_poly_adj<Real, t, RAGGED>;
        HIPSOXR_POLY_TAPS(HIPSOXR_POLY_T)
#undef HIPSOXR_POLY_T
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// The polyphase launch.  Every decision that reads nothing but numbers is a function of poly_rules.h; here: the stage and
// the job into PolyArgs (poly_args), the lane-order cache (poly_lanes), the kernel instance (poly_kernel), the trace
// buffer of -DPOLY_TRACE builds, the launch-log line, and launch_poly, which puts them in order.
// ---------------------------------------------------------------------------------------------
// one polyphase launch: the source column holds samples [n_lo, n_src) (src points at sample 0; zero outside), outputs
// [k_lo, k_lo + n_out) go to dst; strides {clip, frame, channel} in elements
struct PolyJob {
    const void *src; void *dst;
    int64_t n_lo, n_src, k_lo, n_out;
    uint32_t n_clips, n_channels;
    const int64_t *sstr, *dstr;
    // a ragged launch (launch_two_stage_ragged): the device rows of its n_clips COLUMNS (n_channels == 1, clip strides 0, the
    // caller's frame stride on the caller's side and 1 on the intermediate's) — n_src / n_out are then the longest column's
    const int64_t *rows = nullptr;
};

static PolyArgs poly_args(const PolyStage &s, const void *tab, const PolyForm &f, const PolyJob &j)
{
    PolyArgs a;
    a.src = j.src; a.dst = j.dst; a.tab = tab;
    a.T = s.T2; a.P = s.P; a.row = s.row;
    a.Ls = s.Ls; a.Ms = s.Ms; a.Mq = s.Ms / s.Ls; a.Mr = s.Ms % s.Ls;
    a.n_lo = j.n_lo; a.n_src = j.n_src; a.k_lo = j.k_lo; a.n_out = f.n1;
    a.lgP = poly_lg(s.P);
    a.step_fx = poly_step_fx(s.Ms, s.Ls);
    a.fx_per_rem = poly_fx_per_rem(s.Ls);
    a.scs = j.sstr[0]; a.sfs = j.sstr[1]; a.schs = j.sstr[2]; a.dcs = j.dstr[0]; a.dfs = j.dstr[1]; a.dchs = j.dstr[2];
    a.n_channels = j.n_channels;
    a.lg_cg = f.lg_cg;
    a.m2_src = f.m2_src; a.m2_dst = f.m2_dst; a.m2_shift = f.m2_shift; a.m2_n_out = f.n2;
    a.trace = nullptr;
    return a; // (R, span_max and lane_mul: launch_poly, once the run length is known)
}

// The lane order for runs of r outputs per thread, simulated once per plan, table (`which`: 0 float32, 1 float64,
// 2 float32 on k_poly2 — three tables of one TwoStage) and r.  One mutex for every plan and element type.
static std::mutex g_lanes_mu;
static PolyLane poly_lanes(const TwoStage &ts, const PolyStage &s, int which, int r)
{
    std::lock_guard<std::mutex> lk(g_lanes_mu);
    PolyLane &l = ts.lanes[which][r];
    if (!l.lane_mul) l = poly_lane_cost(s.P, s.row, which == 1 ? 2 : 1, r, s.ratio); // (a double4 record is two 16-byte reads)
    return l;
}

// the only place the instance lists expand: MQ = Mq where that is 0 or 1, else -1 (k_poly alone).  RAGGED: k_poly's ragged
// instances — every tap count, MQ and element type (k_poly2 has none: pair and split are false there)
template <typename Real, bool RAGGED = false>
static void (*poly_kernel(int T2, int64_t Mq, bool pair, bool split))(typename PolyArgsOf<RAGGED>::type)
{
    void (*kern)(typename PolyArgsOf<RAGGED>::type) = nullptr;
    switch (T2) {
#define HIPSOXR_POLY_T(t) case t: kern = Mq == 0 ? k_poly<Real, t, 0, RAGGED> : Mq == 1 ? k_poly<Real, t, 1, RAGGED> : k_poly<Real, t, -1, RAGGED>; break;
        HIPSOXR_POLY_TAPS(HIPSOXR_POLY_T)
#undef HIPSOXR_POLY_T
    }
    if constexpr (sizeof(Real) == 4 && !RAGGED)
        if (pair || split) switch (T2) {
#define HIPSOXR_POLY_T(t) case t: kern = pair ? (Mq == 0 ? k_poly2<t, 0, true> : k_poly2<t, 1, true>) : (Mq == 0 ? k_poly2<t, 0, false> : k_poly2<t, 1, false>); break;
            HIPSOXR_POLY2_TAPS(HIPSOXR_POLY_T)
#undef HIPSOXR_POLY_T
        }
    return kern;
}
// (-DPOLY_TRACE: per-wave cycle sums [workgroup][wave][8], dumped synchronously behind the launch — a debugging aid)
#ifdef POLY_TRACE
static const char *poly_trace_begin(PolyArgs &a, dim3 grid, size_t *n)
{
    *n = (size_t)grid.x * grid.y * 4 * 8;
    if (!switches().dbg_trace) return nullptr;
    HIP_TRY(hipMalloc((void **)&a.trace, *n * 8));
    HIP_TRY(hipMemset(a.trace, 0, *n * 8));
    return nullptr;
}
static const char *poly_trace_dump(const PolyArgs &a, size_t n, hipStream_t st)
{
    if (!a.trace) return nullptr;
    std::vector<unsigned long long> h(n);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(h.data(), a.trace, n * 8, hipMemcpyDeviceToHost));
    if (FILE *f = fopen(switches().dbg_trace, "wb")) { fwrite(h.data(), 8, n, f); fclose(f); }
    (void)hipFree(a.trace);
    return nullptr;
}
#else
static const char *poly_trace_begin(PolyArgs &, dim3, size_t *) { return nullptr; }
static const char *poly_trace_dump(const PolyArgs &, size_t, hipStream_t) { return nullptr; }
#endif

// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): one line per polyphase launch, in the style of adjoint.hip's
// adj_launch_log — what tests/test_gpu_two_stage_forms.py reads the launch form from.
// A ragged launch appends ragged=<columns> (tiles, n_out: the longest column's).
static void poly_launch_log(size_t width, const PolyArgs &a, const PolyForm &f, const PolyLane &ln, size_t lds, uint64_t cols, int64_t n_tiles, dim3 grid, bool ragged)
{
    FILE *fl = fopen(switches().dbg_launch_log, "a");
    if (!fl) return;
    fprintf(fl, "kernel=%s width=%zu T=%d MQ=%d il=%d split=%d R=%d lane_mul=%d conf=%.4f lds=%zu lg_cg=%d cols=%llu tiles=%lld grid=%ux%ux%u block=256 n_out=%lld m2_n_out=%lld",
            f.pair || f.split ? "poly2" : "poly", width, a.T, a.Mq == 0 || a.Mq == 1 ? (int)a.Mq : -1, (int)f.pair, (int)f.split, a.R, ln.lane_mul, (double)ln.conf, lds,
            a.lg_cg, (unsigned long long)cols, (long long)n_tiles, grid.x, grid.y, grid.z, (long long)a.n_out, (long long)a.m2_n_out);
    if (ragged) fprintf(fl, " ragged=%llu", (unsigned long long)cols);
    fprintf(fl, "\n");
    fclose(fl);
}

template <typename Real>
static const char *launch_poly(const TwoStage &ts, const PolyJob &j, hipStream_t st)
{
    if (j.n_out <= 0) return nullptr;
    constexpr size_t W = sizeof(Real);
    const PolyStage s = poly_stage(ts.T2, W == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms);
    const PolyForm f = j.rows ? poly_form_ragged(j.n_out)
                              : poly_form(W, s.Ms / s.Ls, j.n_channels, j.sstr, j.dstr, (uintptr_t)j.src | (uintptr_t)j.dst, s.T2, switches().poly_no_pair, j.n_out, s.Ls, s.Ms);
    PolyArgs a = poly_args(s, W == 4 ? ts.tab_f : ts.tab_d, f, j);
    const bool two = f.pair || f.split; // k_poly2
    const size_t unit = poly_unit(W, two), tab_bytes = poly_tab_bytes(s.P, s.row, W);
    const int Rmax = poly_rmax(W, tab_bytes, two, s.T2, s.ratio, switches().dbg_poly_r);
    const uint64_t cols = poly_cols(j.n_clips, j.n_channels, f.pair, f.lg_cg);
    if (cols > kPolyMaxCols) return "two-stage: too many columns";
    int dev = 0, n_cu = 256;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    // the run length, and the lane order that goes with it
    const int which = two ? 2 : W == 8;
    const int64_t slots = poly_slots(Rmax, tab_bytes, s.ratio, s.T2, unit, poly_occ_limit(W, two, s.T2), n_cu, cols);
    a.R = poly_pick_run(Rmax, a.n_out, slots, [&](int r) -> double { return poly_lanes(ts, s, which, r).conf; });
    const PolyLane ln = poly_lanes(ts, s, which, a.R);
    a.lane_mul = ln.lane_mul;
    a.span_max = poly_span_max(a.R, s.ratio, s.T2);
    const size_t lds = poly_lds_bytes(tab_bytes, a.R, s.ratio, s.T2, unit);
    if (lds > kPolyLdsMax) return "two-stage: polyphase tile does not fit LDS";
    const int64_t n_tiles = poly_tiles(a.n_out, a.R);
    // (a ragged launch: R, the lane order and the LDS size above and the grid below are the LONGEST column's)
    void (*kern)(PolyArgs) = j.rows ? nullptr : poly_kernel<Real>(s.T2, a.Mq, f.pair, f.split);
    void (*kern_r)(PolyArgsR) = j.rows ? poly_kernel<Real, true>(s.T2, a.Mq, false, false) : nullptr;
    const void *fn = j.rows ? (const void *)kern_r : (const void *)kern;
    if (!fn) return "two-stage: no polyphase instance for this tap count";
    if (const char *e = ensure_dyn_lds(fn, lds)) return e;
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
    const dim3 grid(poly_grid_x(n_tiles, per_cu, n_cu, cols), (unsigned)cols, 1);
    size_t trace_n = 0;
    if (const char *e = poly_trace_begin(a, grid, &trace_n)) return e;
    if (switches().dbg_launch_log) poly_launch_log(W, a, f, ln, lds, cols, n_tiles, grid, j.rows != nullptr);
    if (j.rows) {
        PolyArgsR ar;
        (PolyArgs &)ar = a;
        ar.rows = j.rows;
        hipLaunchKernelGGL(kern_r, grid, dim3(256), lds, st, ar);
    } else
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return poly_trace_dump(a, trace_n, st);
}

// one polyphase launch in the job's element type
static const char *run_poly(int elem, const TwoStage &ts, const PolyJob &j, hipStream_t st)
{
    return elem == HIPSOXR_F32 ? launch_poly<float>(ts, j, st) : launch_poly<double>(ts, j, st);
}

// The two launches of an admitted job around its intermediate signal `mid` (m: its layout).  The stage that writes the
// intermediate produces its `pad` samples either side like any others (its own input zero-extended), the stage that reads
// it sees zeros beyond them — so the composite is the prototype's response to the zero-extended signal at EVERY output,
// ends included, and no third engine patches the ends.  *handled = false with no error: the FFT engine declined its stage —
// up: nothing but the intermediate was touched; down: the queued polyphase launch wrote the intermediate only — and the
// caller's ordinary path computes the job.
static const char *two_stage_run(Plan *p, const hipsoxr_job_t &j, const TwoStageMid &m, void *mid, void *stream, bool *handled)
{
    const TwoStage &ts = *p->two;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const int64_t n = j.in_frames, n_out = j.out_frames;
    const int64_t istr[3] = {j.in_clip_stride, j.in_frame_stride, j.in_chan_stride};
    const int64_t ostr[3] = {j.out_clip_stride, j.out_frame_stride, j.out_chan_stride};
    hipsoxr_job_t fj = j;
    fj.kernel = j.kernel == HIPSOXR_KERNEL_FFT_F64 ? HIPSOXR_KERNEL_FFT_F64 : HIPSOXR_KERNEL_FFT;
    fj.clip_counter = nullptr; fj.dither = 0;
    PolyJob pj;
    pj.n_clips = j.n_clips; pj.n_channels = j.n_channels;
    if (ts.up) { // FFT stage 1:2 over the input delayed by pad / 2 samples (its output m' is u[m' - pad]), then u -> y
        fj.in_abs0 = m.pad / 2;
        fj.out = mid; fj.out_clip_stride = m.mstr[0]; fj.out_frame_stride = m.mstr[1]; fj.out_chan_stride = m.mstr[2];
        fj.in_frames = n; fj.out_frames = m.n_mid;
        pj.src = (char *)mid + (size_t)(m.pad * m.mstr[1]) * es; // sample 0 of the first column
        pj.dst = j.out; pj.n_lo = -m.pad; pj.n_src = m.n_core + m.pad; pj.k_lo = 0; pj.n_out = n_out; pj.sstr = m.mstr; pj.dstr = ostr;
    } else {     // x -> v [-pad, 2 n_out + pad), then the FFT stage 2:1 over it
        pj.src = j.in; pj.dst = mid; pj.n_lo = 0; pj.n_src = n; pj.k_lo = -m.pad; pj.n_out = m.n_mid; pj.sstr = istr; pj.dstr = m.mstr;
        fj.in = mid; fj.in_abs0 = -m.pad; fj.in_clip_stride = m.mstr[0]; fj.in_frame_stride = m.mstr[1]; fj.in_chan_stride = m.mstr[2];
        fj.in_frames = m.n_mid; fj.out_frames = n_out;
    }
    if (const char *err = device_bank_ensure(&p->two->fft, engine_prec(j.elem))) return err;
    bool fft_done = false;
    if (ts.up) {
        const char *err = launch_fft(&p->two->fft, fj, stream, &fft_done);
        if (err || !fft_done) return err;
    }
    if (const char *err = run_poly(j.elem, ts, pj, (hipStream_t)stream)) return err;
    if (!ts.up) {
        const char *err = launch_fft(&p->two->fft, fj, stream, &fft_done);
        if (err || !fft_done) return err;
    }
    *handled = true;
    return nullptr;
}

// Whole-signal float job on an interpolated-phase plan: FFT stage + polyphase stage.  *handled = false
// (nothing launched) when the plan or the job is not one the two-stage form serves: the caller's ordinary path takes it.
const char *launch_two_stage(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    *handled = false;
    if (!p->phases || (j.elem != HIPSOXR_F32 && j.elem != HIPSOXR_F64) || j.in_abs0 != 0 || j.out_k0 != 0 || j.clip_table) return nullptr;
    if ((uint64_t)j.out_frames > plan_out_len(*p, (uint64_t)j.in_frames)) return nullptr;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (!p->two)
            if (const char *e = twostage_build(p)) return e;
    }
    const TwoStage &ts = *p->two;
    if (!ts.ok) return nullptr;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (!two_stage_admits(j.in_frames, j.out_frames, cols, es, poly_stage(ts.T2, es == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms))) return nullptr;
    const bool inter = j.n_channels % 2 == 0 && j.in_chan_stride == 1 && j.out_chan_stride == 1;
    // (a truncated job down: the intermediate as far as its last outputs' FFT-stage filter reaches — two_stage_mid_outputs)
    const TwoStageMid m = two_stage_mid(ts.up, ts.T2, ts.Ls, ts.Ms, j.in_frames, two_stage_mid_outputs(ts.up, ts.Ls, ts.Ms, j.in_frames, j.out_frames, ts.fft.T),
                                        j.n_channels, inter);
    hipStream_t st = (hipStream_t)stream;
    void *mid = nullptr;
    HIP_TRY(hipMallocAsync(&mid, (size_t)cols * (size_t)m.n_mid * es, st));
    const char *err = two_stage_run(p, j, m, mid, stream, handled);
    (void)hipFreeAsync(mid, st); // (behind whatever was queued: success, error and a declined FFT stage alike)
    return err;
}

// ---------------------------------------------------------------------------------------------
// The adjoint of the two-stage form (HIPSOXR_KERNEL_ADJOINT_TWO_STAGE on hipsoxr_run_device_adjoint): gx = A^T gy, A the
// forward job launch_two_stage runs for (in_frames = n_x, out_frames = n_y) — the same TwoStage, the same TwoStageMid, the
// same intermediate window [-pad, n_core + pad) with zeros outside it: the structural transpose of the forward as launched.
//   down (forward x --k_poly--> v --FFT 2:1, in_abs0 = -pad--> y):  gv = F^T gy, the forward float job of the FFT stage's
//        TRANSPOSED PLAN (1:2; adjoint_fft_rules.h) with in_abs0 = pad / 2 into the intermediate; gx = P^T gv: k_poly_adj.
//   up   (forward x --FFT 1:2, in_abs0 = pad / 2--> u --k_poly--> y):  gu = P^T gy: k_poly_adj over the whole window; gx =
//        F^T gu, the transposed plan (2:1) with in_abs0 = -pad.
// Every decision that reads only numbers is poly_adj_rules.h; the refusals are made by name before the device is asked for
// anything, and a plan or job the form does not take fails with kPolyAdjUnavailable — never the exact adjoint.
// ---------------------------------------------------------------------------------------------
// HIPSOXR_DEBUG_LAUNCH_LOG (debug-switch build only): k_poly_adj's line, in poly_launch_log's style
// A ragged launch appends ragged=1 (tiles, n_src, n_out: the longest column's).
static void poly_adj_launch_log(size_t width, const PolyArgs &a, size_t lds, uint64_t cols, int64_t n_tiles, dim3 grid, bool ragged)
{
    FILE *fl = fopen(switches().dbg_launch_log, "a");
    if (!fl) return;
    fprintf(fl, "kernel=poly_adj width=%zu T=%d MQ=%d R=%d span_max=%d lds=%zu cols=%llu tiles=%lld grid=%ux%ux%u block=256 n_lo=%lld n_src=%lld k_lo=%lld n_out=%lld%s\n",
            width, a.T, a.Mq == 0 || a.Mq == 1 ? (int)a.Mq : -1, a.R, a.span_max, lds, (unsigned long long)cols, (long long)n_tiles, grid.x, grid.y, grid.z,
            (long long)a.n_lo, (long long)a.n_src, (long long)a.k_lo, (long long)a.n_out, ragged ? " ragged=1" : "");
    fclose(fl);
}

// One k_poly_adj launch; j in the FORWARD's direction (src: the stage's input side, written; dst: its output side, read).
// dry: everything but the launch — the run, the instance, the LDS attribute — so that nothing can fail behind a queued stage.
// j.rows (launch_adjoint_two_stage_ragged): the ragged instance over the table's columns, j.n_src the longest column's.
template <typename Real>
static const char *launch_poly_adj(const TwoStage &ts, const PolyJob &j, hipStream_t st, bool dry)
{
    constexpr size_t W = sizeof(Real);
    const PolyStage s = poly_stage(ts.T2, W == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms);
    PolyArgs a = poly_args(s, W == 4 ? ts.tab_f : ts.tab_d, poly_form_ragged(j.n_out), j);
    const size_t tab_bytes = poly_tab_bytes(s.P, s.row, W);
    a.R = poly_adj_run(tab_bytes, s.T2, s.ratio, W);
    if (a.R <= 0) return kPolyAdjUnavailable; // (poly_adj_admits has asked: not reached)
    a.lane_mul = 1;
    a.span_max = poly_adj_span_max(poly_adj_tile(a.R), s.T2, s.ratio);
    const size_t lds = poly_adj_lds_bytes(tab_bytes, a.R, s.T2, s.ratio, W);
    void (*kern)(PolyArgs) = j.rows ? nullptr : poly_adj_kernel<Real>(s.T2);
    void (*kern_r)(PolyArgsR) = j.rows ? poly_adj_kernel<Real, true>(s.T2) : nullptr;
    const void *fn = j.rows ? (const void *)kern_r : (const void *)kern;
    if (!fn) return "two-stage: no polyphase instance for this tap count";
    if (const char *e = ensure_dyn_lds(fn, lds)) return e;
    if (dry || j.n_src <= j.n_lo) return nullptr;
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    if (cols > kPolyMaxCols) return "two-stage: too many columns"; // (poly_adj_admits / the ranges have asked: not reached)
    int dev = 0, n_cu = 256, per_cu = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds));
    const int64_t n_tiles = poly_adj_tiles(j.n_src - j.n_lo, a.R);
    const dim3 grid(j.rows ? poly_adj_grid_x_ragged(n_tiles, per_cu, n_cu, cols) : poly_adj_grid_x(n_tiles, per_cu, n_cu, cols), (unsigned)cols, 1);
    if (switches().dbg_launch_log) poly_adj_launch_log(W, a, lds, cols, n_tiles, grid, j.rows != nullptr);
    if (j.rows) {
        PolyArgsR ar;
        (PolyArgs &)ar = a;
        ar.rows = j.rows;
        hipLaunchKernelGGL(kern_r, grid, dim3(256), lds, st, ar);
    } else
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return nullptr;
}
static const char *run_poly_adj(int elem, const TwoStage &ts, const PolyJob &j, hipStream_t st, bool dry)
{
    return elem == HIPSOXR_F32 ? launch_poly_adj<float>(ts, j, st, dry) : launch_poly_adj<double>(ts, j, st, dry);
}

// The two launches of an admitted adjoint job around the intermediate `mid` (m: the FORWARD job's layout).  *handled = false
// with no error: the FFT stage declined — down: before anything was queued; up: behind k_poly_adj, which wrote the
// intermediate only — and gx is untouched either way.
static const char *two_stage_adj_run(Plan *p, const hipsoxr_job_t &j, const TwoStageMid &m, void *mid, void *stream, bool *handled)
{
    const TwoStage &ts = *p->two;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const int64_t n_y = j.in_frames, n_x = j.out_frames;
    const int64_t ystr[3] = {j.in_clip_stride, j.in_frame_stride, j.in_chan_stride};
    const int64_t xstr[3] = {j.out_clip_stride, j.out_frame_stride, j.out_chan_stride};
    hipsoxr_job_t fj = j; // the FFT stage's transposed plan, forward, by name
    fj.kernel = HIPSOXR_KERNEL_FFT;
    fj.clip_counter = nullptr; fj.dither = 0; fj.dither_seed = 0; fj.clip_table = nullptr; fj.clip_table_dev = nullptr;
    PolyJob pj;
    pj.n_clips = j.n_clips; pj.n_channels = j.n_channels;
    if (ts.up) { // gu = P^T gy over the whole window, then gx = F^T gu
        pj.src = (char *)mid + (size_t)(m.pad * m.mstr[1]) * es; pj.n_lo = -m.pad; pj.n_src = m.n_core + m.pad; pj.sstr = m.mstr;
        pj.dst = const_cast<void *>(j.in); pj.k_lo = 0; pj.n_out = n_y; pj.dstr = ystr;
        fj.in = mid; fj.in_abs0 = -m.pad; fj.in_clip_stride = m.mstr[0]; fj.in_frame_stride = m.mstr[1]; fj.in_chan_stride = m.mstr[2];
        fj.in_frames = m.n_mid; fj.out_frames = n_x;
    } else {     // gv = F^T gy into the window, then gx = P^T gv
        fj.in_abs0 = m.pad / 2;
        fj.out = mid; fj.out_clip_stride = m.mstr[0]; fj.out_frame_stride = m.mstr[1]; fj.out_chan_stride = m.mstr[2];
        fj.in_frames = n_y; fj.out_frames = m.n_mid;
        pj.src = j.out; pj.n_lo = 0; pj.n_src = n_x; pj.sstr = xstr;
        pj.dst = mid; pj.k_lo = -m.pad; pj.n_out = m.n_mid; pj.dstr = m.mstr;
    }
    if (const char *e = run_poly_adj(j.elem, ts, pj, (hipStream_t)stream, true)) return e; // (nothing queued yet)
    bool fft_done = false;
    if (!ts.up) {
        if (const char *e = launch_fft(ts.fft_t, fj, stream, &fft_done)) return e;
        if (!fft_done) return nullptr;
    }
    if (const char *e = run_poly_adj(j.elem, ts, pj, (hipStream_t)stream, false)) return e;
    if (ts.up) {
        if (const char *e = launch_fft(ts.fft_t, fj, stream, &fft_done)) return e;
        if (!fft_done) return nullptr;
    }
    *handled = true;
    return nullptr;
}

// the plan's two-stage form with the transposed plan of its FFT stage, built on first use under the plan's mutex
static const char *two_stage_adj_ensure(Plan *p)
{
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->two)
        if (const char *e = twostage_build(p)) return e;
    TwoStage *ts = p->two;
    if (ts->ok && !ts->fft_t) {
        ts->fft_t = adj_fft_transposed(ts->fft);
        ts->fft_t->device = p->device;
    }
    return nullptr;
}

const char *launch_adjoint_two_stage(Plan *p, const hipsoxr_job_t &j, void *stream)
{
    if (elem_is_half(j.elem)) {
        // float16 / bfloat16: the float32 job of this selector on the widened cotangent, rounded once (half.hip) — the
        // refusals by name and the empty job first, asked of the float32 job without clips
        hipsoxr_job_t f = j;
        f.elem = HIPSOXR_F32; f.n_clips = 0;
        if (const char *e = launch_adjoint_two_stage(p, f, stream)) return e;
        if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
        if (!j.out || (j.in_frames > 0 && !j.in)) return "null buffer";
        if (device_count() <= 0) return kNoDevice;
        return launch_half(p, j, stream, true);
    }
    const PolyAdjAsk q = {j.elem == HIPSOXR_F32 || j.elem == HIPSOXR_F64, p->vr, p->phases == 0, j.in_abs0 != 0 || j.out_k0 != 0, j.clip_table != nullptr};
    if (const char *e = poly_adj_refusal(q)) return e;
    if (const char *e = adj_extent_refusal(kAdjEqual, j.in_frames, j.out_frames, [&](uint64_t n) { return plan_out_len(*p, n); })) return e;
    if (job_empty(j.out_frames, j.n_clips, j.n_channels)) return nullptr;
    if (!j.out || (j.in_frames > 0 && !j.in)) return "null buffer";
    if (device_count() <= 0) return kNoDevice;
    bool handled = false;
    if (const char *e = launch_adjoint_two_stage_try(p, j, stream, &handled)) return e;
    return handled ? nullptr : kPolyAdjUnavailable;
}

// ... behind the refusals: a float32 / float64 whole-cotangent job of an interpolated-phase plan, not empty, buffers and device
// asked for.  *handled = false with no error and gx untouched — a plan without the form, a job poly_adj_admits does not take,
// an FFT stage that declines: by name that is kPolyAdjUnavailable (above), under HIPSOXR_KERNEL_ADJOINT_AUTO the exact
// adjoint's job (adjoint_auto.hip).
const char *launch_adjoint_two_stage_try(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    *handled = false;
    if (const char *e = two_stage_adj_ensure(p)) return e;
    const TwoStage &ts = *p->two;
    if (!ts.ok) return nullptr;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const uint64_t cols = (uint64_t)j.n_clips * j.n_channels;
    const int64_t n_y = j.in_frames, n_x = j.out_frames;
    if (!poly_adj_admits(n_x, n_y, cols, es, poly_stage(ts.T2, es == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms))) return nullptr;
    const bool inter = j.n_channels % 2 == 0 && j.in_chan_stride == 1 && j.out_chan_stride == 1;
    const TwoStageMid m = two_stage_mid(ts.up, ts.T2, ts.Ls, ts.Ms, n_x, two_stage_mid_outputs(ts.up, ts.Ls, ts.Ms, n_x, n_y, ts.fft.T), j.n_channels, inter);
    hipStream_t st = (hipStream_t)stream;
    void *mid = nullptr;
    HIP_TRY(hipMallocAsync(&mid, (size_t)cols * (size_t)m.n_mid * es, st));
    const char *err = two_stage_adj_run(p, j, m, mid, stream, handled);
    (void)hipFreeAsync(mid, st); // (behind whatever was queued)
    return err;
}

// ---------------------------------------------------------------------------------------------
// A clip table on the two-stage form: a constant number of launches whatever the number of clips.  Every decision that
// reads only numbers — the partition into empty, two-stage and short clips, each column's intermediate (two_stage_mid of
// the clip alone), its place in the packed intermediate, the rows of both stages, the ranges — is poly_rules.h
// ragged_poly_plan; here: the served layouts, ONE upload of every derived table, and per range one allocation, the two
// launches in the direction's order and one free, in stream order; the short clips' launch last.
// Served: float32 / float64, HIPSOXR_KERNEL_AUTO, any positive frame stride on the caller's side (mono clips, planar channels
// at any channel stride: the ragged k_fft_pair2; interleaved channels, channel slices: the ragged k_fft_strided2, one column
// per (clip, channel), the intermediate library-owned and unit-stride either way).  The caller's clip_table_dev cannot serve: the inner launches read derived
// tables (columns, not clips; intermediate offsets), and the short clips a compacted one.
// *handled = false with no error — a layout not served, a plan without the form, a short clip the ragged exact launch does not
// take, or the FFT stage declined — and the caller's clip-by-clip loop computes every clip.  (The FFT stage's answer follows
// the plan, the layout and the range's sizes: it is expected in the first range, before the caller's output is touched, but a
// later range is not excluded.  Either way the loop rewrites every clip, and the inner jobs carry no clip counter.)
// ---------------------------------------------------------------------------------------------
// A range's intermediate (up to kPolyMidBudget) comes from the device's default stream-ordered pool, whose release threshold is
// 0 by default: memory it holds unused may go back to the system, and the next launch then acquires it anew.  The pool is asked
// to keep as much as the largest range seen needs (never lowered; one query per call, one set when it grows).
static void mid_pool_retain(uint64_t bytes)
{
    static std::mutex mu;
    static uint64_t kept[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    std::lock_guard<std::mutex> lk(mu);
    if (kept[dev] >= bytes) return;
    hipMemPool_t pool = nullptr;
    uint64_t cur = 0;
    if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess || hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, &cur) != hipSuccess) return;
    if (cur < bytes && hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &bytes) != hipSuccess) return;
    kept[dev] = std::max(cur, bytes);
}
const char *launch_two_stage_ragged(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    *handled = false;
    if (!p->phases || !j.clip_table || (j.elem != HIPSOXR_F32 && j.elem != HIPSOXR_F64) || j.kernel != HIPSOXR_KERNEL_AUTO) return nullptr;
    if (j.in_frame_stride < 1 || j.out_frame_stride < 1 || j.in_abs0 != 0 || j.out_k0 != 0 || j.n_channels > kPolyMaxCols) return nullptr;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (!p->two)
            if (const char *e = twostage_build(p)) return e;
    }
    const TwoStage &ts = *p->two;
    if (!ts.ok) return nullptr;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const PolyStage s = poly_stage(ts.T2, es == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms);
    const int64_t budget = switches().dbg_poly_mid_budget > 0 ? (int64_t)switches().dbg_poly_mid_budget : kPolyMidBudget;
    const RaggedPolyPlan rp = ragged_poly_plan(j.clip_table, j.n_clips, j.n_channels, j.in_chan_stride, j.out_chan_stride, es, ts.up, s, ts.fft.T, budget);
    const uint32_t n_short = rp.n_short(), n_cols = rp.n_cols();
    if (!n_short && !n_cols) { *handled = true; return nullptr; } // nothing to write
    if (ragged_longest(rp.short_rows.data(), n_short) > ((int64_t)1 << 30)) return nullptr; // (launch_ragged_job leaves such a clip to the loop)
    hipStream_t st = (hipStream_t)stream;
    if (n_cols)
        if (const char *err = device_bank_ensure(&p->two->fft, engine_prec(j.elem))) return err;
    {
        int64_t peak = 0;
        for (const RaggedPolyRange &g : rp.ranges) peak = std::max(peak, g.mid_elems);
        mid_pool_retain((uint64_t)peak * es);
    }
    // every derived table in one host buffer and one upload: [short rows][poly rows][FFT rows].  (`host` is pageable and dies
    // at return: this relies on hipMemcpyAsync having read pageable host memory into its staging buffers before it returns —
    // clip_table_device relies on the same for a caller's table that may be a temporary.)
    std::vector<int64_t> host(rp.short_rows);
    host.insert(host.end(), rp.poly_rows.begin(), rp.poly_rows.end());
    host.insert(host.end(), rp.fft_rows.begin(), rp.fft_rows.end());
    int64_t *tabs = nullptr;
    if (hipMallocAsync((void **)&tabs, host.size() * sizeof(int64_t), st) != hipSuccess) return "ragged batches: no device memory for the two-stage form's tables";
    const int64_t *short_dev = tabs, *poly_dev = tabs + 4 * (size_t)n_short, *fft_dev = poly_dev + 4 * (size_t)n_cols;
    const char *err = nullptr;
    bool all = true;
    if (hipMemcpyAsync(tabs, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice, st) != hipSuccess) err = "ragged batches: table upload failed";
    // columns: no clip stride, one channel; the intermediate's frames are unit-stride, the caller's lie at the caller's frame
    // stride (interleaved channels, channel slices): the polyphase kernel multiplies by it, the FFT stage runs its strided form
    const int64_t unit[3] = {0, 1, 0}, cin[3] = {0, j.in_frame_stride, 0}, cout[3] = {0, j.out_frame_stride, 0};
    for (size_t r = 0; r < rp.ranges.size() && !err && all; ++r) {
        const RaggedPolyRange &g = rp.ranges[r];
        void *mid = nullptr;
        if (hipMallocAsync(&mid, (size_t)g.mid_elems * es, st) != hipSuccess) { err = "two-stage: no device memory for the intermediate signal"; break; }
        PolyJob pj;
        pj.n_clips = g.count; pj.n_channels = 1; pj.sstr = unit; pj.dstr = unit;
        pj.rows = poly_dev + 4 * (size_t)g.first; pj.n_out = g.poly_longest;
        hipsoxr_job_t fj = j;
        fj.kernel = HIPSOXR_KERNEL_FFT; fj.clip_counter = nullptr; fj.dither = 0;
        fj.n_clips = g.count; fj.n_channels = 1;
        fj.in_clip_stride = fj.out_clip_stride = 0; fj.in_chan_stride = fj.out_chan_stride = 0;
        fj.clip_table = rp.fft_rows.data() + 4 * (size_t)g.first; fj.clip_table_dev = fft_dev + 4 * (size_t)g.first;
        fj.in_frames = g.fft_in_longest; fj.out_frames = g.fft_out_longest;
        if (ts.up) { // x --FFT 1:2--> mid --poly--> y
            fj.in_abs0 = rp.pad / 2; fj.out = mid; fj.out_frame_stride = 1;
            pj.src = mid; pj.dst = j.out; pj.dstr = cout; pj.n_lo = -rp.pad; pj.k_lo = 0; pj.n_src = 0;
        } else {     // x --poly--> mid --FFT 2:1--> y
            pj.src = j.in; pj.sstr = cin; pj.dst = mid; pj.n_lo = 0; pj.k_lo = -rp.pad; pj.n_src = 0;
            fj.in = mid; fj.in_abs0 = -rp.pad; fj.in_frame_stride = 1;
        }
        bool fft_done = false;
        if (ts.up) {
            err = launch_fft(&p->two->fft, fj, stream, &fft_done);
            if (!err && !fft_done) all = false;
        }
        if (!err && all) err = run_poly(j.elem, ts, pj, st);
        if (!err && all && !ts.up) {
            err = launch_fft(&p->two->fft, fj, stream, &fft_done);
            if (!err && !fft_done) all = false;
        }
        (void)hipFreeAsync(mid, st); // (behind whatever was queued)
    }
    if (!err && all && n_short) { // the clips the form does not admit: the exact engine's ragged launch over the compacted sub-table
        hipsoxr_job_t sj = j;
        sj.n_clips = n_short; sj.clip_table = rp.short_rows.data(); sj.clip_table_dev = short_dev;
        bool h = false;
        err = launch_ragged_short(p, sj, stream, &h);
        if (!err && !h) all = false;
    }
    (void)hipFreeAsync(tabs, st);
    if (err) return err;
    *handled = all;
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// A clip table on the TRANSPOSED two-stage form (HIPSOXR_KERNEL_ADJOINT_AUTO on hipsoxr_run_device_adjoint_ragged;
// adjoint_auto.hip has made the refusals, validated the rows and asked for buffers and device): launch_two_stage_ragged in the
// adjoint's order.  Every decision that reads only numbers is adjoint_auto_rules.h ragged_poly_adj_plan — the partition
// (adj_auto_class), ragged_poly_plan's columns, intermediates, packing and ranges on the swapped table, the forward's poly
// rows, the transposed plan's FFT rows; here: a dry pass, ONE upload of every derived table, per range one allocation, the two
// launches (down: FFT^T into the intermediate, then k_poly_adj; up: k_poly_adj over the whole window, then FFT^T) and one
// free, in stream order; the short clips' ONE ragged launch of the exact adjoint last.
// *handled = false with no error and gx untouched — a layout not served, a plan without the form, no clip the form admits, a
// short clip too long for one launch, or an FFT stage that declines the FIRST range (down: before anything is queued; up:
// behind a k_poly_adj that wrote the intermediate alone) — and the caller runs the exact ragged adjoint over the whole table.
// A decline behind the first range is an error by name: gx is part written.
// ---------------------------------------------------------------------------------------------
const char *launch_adjoint_two_stage_ragged(Plan *p, const hipsoxr_job_t &j, void *stream, bool *handled)
{
    *handled = false;
    if (j.in_frame_stride < 1 || j.out_frame_stride < 1 || j.n_channels > kPolyMaxCols) return nullptr;
    if (const char *e = two_stage_adj_ensure(p)) return e;
    const TwoStage &ts = *p->two;
    if (!ts.ok) return nullptr;
    const size_t es = j.elem == HIPSOXR_F32 ? 4 : 8;
    const PolyStage s = poly_stage(ts.T2, es == 4 ? ts.P2f : ts.P2, ts.row, ts.Ls, ts.Ms);
    const int64_t budget = switches().dbg_poly_mid_budget > 0 ? (int64_t)switches().dbg_poly_mid_budget : kPolyMidBudget;
    const RaggedPolyAdjPlan rp = ragged_poly_adj_plan(j.clip_table, j.n_clips, j.n_channels, j.in_chan_stride, j.out_chan_stride, es, ts.up, s, ts.fft.T, budget);
    const uint32_t n_short = rp.n_short(), n_cols = rp.n_cols();
    if (!n_cols) return nullptr; // (every clip empty or short: the exact adjoint's one launch over the table as it stands)
    for (uint32_t c = 0; c < n_short; ++c) // (a clip the exact adjoint may answer kAdjTooLong for: asked of the whole table, before anything is queued)
        if (std::max(rp.short_rows[4 * (size_t)c + 1], rp.short_rows[4 * (size_t)c + 3]) > ((int64_t)1 << 30)) return nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int64_t unit[3] = {0, 1, 0}, cy[3] = {0, j.in_frame_stride, 0}, cx[3] = {0, j.out_frame_stride, 0};
    hipsoxr_job_t sj = j; // the short clips' job: the exact adjoint by name over the compacted sub-table
    sj.kernel = HIPSOXR_KERNEL_ADJOINT; sj.n_clips = n_short; sj.clip_table = rp.short_rows.data();
    PolyJob pj; // (what every range shares: columns — no clip stride, one channel; the intermediate unit-stride, the caller's sides at the caller's frame strides)
    pj.n_channels = 1; pj.n_lo = rp.n_lo; pj.k_lo = ts.up ? 0 : -rp.fwd.pad;
    pj.src = ts.up ? nullptr : j.out; pj.sstr = ts.up ? unit : cx;
    pj.dst = ts.up ? const_cast<void *>(j.in) : nullptr; pj.dstr = ts.up ? cy : unit;
    { // the dry pass: the instance and its LDS attribute, the FFT stage's tables, the exact adjoint's — nothing is queued yet
        PolyJob dj = pj;
        dj.rows = rp.fwd.poly_rows.data(); dj.n_clips = 1; dj.n_src = 0; dj.n_out = 0;
        if (const char *e = run_poly_adj(j.elem, ts, dj, st, true)) return e;
        if (const char *e = device_bank_ensure(ts.fft_t, engine_prec(j.elem))) return e;
        if (n_short)
            if (const char *e = adj_exact_run(p, sj, stream, nullptr, true)) return e;
        int64_t peak = 0;
        for (const RaggedPolyRange &g : rp.fwd.ranges) peak = std::max(peak, g.mid_elems);
        mid_pool_retain((uint64_t)peak * es);
    }
    // every derived table in one host buffer and one upload: [short rows][poly rows][FFT rows] (pageable: as launch_two_stage_ragged)
    std::vector<int64_t> host(rp.short_rows);
    host.insert(host.end(), rp.fwd.poly_rows.begin(), rp.fwd.poly_rows.end());
    host.insert(host.end(), rp.fft_rows.begin(), rp.fft_rows.end());
    int64_t *tabs = nullptr;
    if (hipMallocAsync((void **)&tabs, host.size() * sizeof(int64_t), st) != hipSuccess) return kAdjAutoFormNoMemory;
    const int64_t *short_dev = tabs, *poly_dev = tabs + 4 * (size_t)n_short, *fft_dev = poly_dev + 4 * (size_t)n_cols;
    const char *err = nullptr;
    bool all = true;
    if (hipMemcpyAsync(tabs, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice, st) != hipSuccess) err = kAdjAutoFormUploadFailed;
    for (size_t r = 0; r < rp.fwd.ranges.size() && !err && all; ++r) {
        const RaggedPolyRange &g = rp.fwd.ranges[r];
        const RaggedPolyAdjRange &ga = rp.ranges[r];
        void *mid = nullptr;
        if (hipMallocAsync(&mid, (size_t)g.mid_elems * es, st) != hipSuccess) { err = kAdjAutoFormNoMemory; break; }
        pj.n_clips = g.count; pj.rows = poly_dev + 4 * (size_t)g.first;
        pj.n_src = rp.n_lo + ga.src_longest; pj.n_out = g.poly_longest;
        if (ts.up) pj.src = mid; // (the rows carry each column's offset of sample 0 in the range's intermediate)
        else pj.dst = mid;
        hipsoxr_job_t fj = j; // the FFT stage's transposed plan, forward, by name, over the range's columns
        fj.kernel = HIPSOXR_KERNEL_FFT; fj.clip_counter = nullptr; fj.dither = 0; fj.dither_seed = 0;
        fj.n_clips = g.count; fj.n_channels = 1;
        fj.in_clip_stride = fj.out_clip_stride = 0; fj.in_chan_stride = fj.out_chan_stride = 0;
        fj.clip_table = rp.fft_rows.data() + 4 * (size_t)g.first; fj.clip_table_dev = fft_dev + 4 * (size_t)g.first;
        fj.in_frames = ga.fft_in_longest; fj.out_frames = ga.fft_out_longest;
        if (ts.up) { fj.in = mid; fj.in_frame_stride = 1; fj.in_abs0 = -rp.fwd.pad; }       // gu --FFT^T 2:1--> gx
        else { fj.out = mid; fj.out_frame_stride = 1; fj.in_abs0 = rp.fwd.pad / 2; }       // gy --FFT^T 1:2--> gv
        bool fft_done = false;
        if (!ts.up) {
            err = launch_fft(ts.fft_t, fj, stream, &fft_done);
            if (!err && !fft_done) all = false;
        }
        if (!err && all) err = run_poly_adj(j.elem, ts, pj, st, false);
        if (!err && all && ts.up) {
            err = launch_fft(ts.fft_t, fj, stream, &fft_done);
            if (!err && !fft_done) all = false;
        }
        (void)hipFreeAsync(mid, st); // (behind whatever was queued)
        if (!err && !all && r > 0) err = kAdjAutoLateDecline;
    }
    if (!err && all && n_short) { // the clips the form does not admit: the exact adjoint's ragged launch over the compacted sub-table
        sj.clip_table_dev = short_dev;
        err = adj_exact_run(p, sj, stream, short_dev, false);
    }
    (void)hipFreeAsync(tabs, st);
    if (err) return err;
    *handled = all;
    return nullptr;
}

} // namespace hipsoxr
