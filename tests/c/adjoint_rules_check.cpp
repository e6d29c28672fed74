// adjoint_rules_check.cpp — the host rules of the transposed operator (python-soxr_amd/csrc/adjoint_rules.h) against slow,
// independent statements of them: the transposed bank (ct, lo) and the per-tile skewed tables (tab, e0) read by the indexing
// the kernels' comments state, against the forward bank through plan.h's locate(); the bounds adjoint.hip's REACH paragraph
// promises; the launch form of every case of tests/test_gpu_adjoint_forms.py against the numbers its launch logs showed on the
// GPU, and over a sweep against its properties and a transcription of the loops adj_launch had; both entries' refusals,
// texts and order, against the conditions written out on raw values.  No device: links plan.cpp alone.
// Exit status 0 = every check held (tests/test_adjoint_rules.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "adjoint_rules.h"
#include "plan.h"

using namespace hipsoxr;

namespace hipsoxr {
Plan::~Plan() {} // (the library's destructor releases device tables: there are none here)
}

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

static bool same(const char *a, const char *b) { return (!a && !b) || (a && b && !std::strcmp(a, b)); }

// ---- the plans of tests/test_gpu_adjoint_forms.py --------------------------------------------------------------------------
enum { QQ = 0, LQ = 1, HQ = 4 }; // include/soxr.h's recipes, restated
enum PlanId { DOWN_QQ, DOWN_LQ, UP_640, UP_441, PRIME, TRIPLE, NF_CASE, N_PLANS };
struct Case { double in_rate, out_rate; int recipe; };
static const Case kPlans[N_PLANS] = {{44100, 8000, QQ}, {48000, 11025, LQ}, {11025, 48000, LQ}, {8000, 44100, LQ}, {9973, 12289, QQ}, {16000, 48000, QQ}, {48000, 44100, HQ}};
static Plan g_plan[N_PLANS];
static AdjTables g_tab[N_PLANS];

static int64_t fdiv(int64_t a, int64_t b) { return (a >= 0 ? a : a - (b - 1)) / b; } // floor, b > 0 (not the header's)

// ---- transpose and bounds ----------------------------------------------------------------------------------------------------
// gx[a] = sum_k C(a, k) gy[k].  C by the forward: bank[p_k T + a - n0_k] where 0 <= a - n0_k < T, else 0.
static double coef_forward(const Plan &p, int64_t a, int64_t k)
{
    int64_t n0, ph;
    locate(p, k, &n0, &ph);
    const int64_t j = a - n0;
    return (j >= 0 && j < p.T) ? p.bank[(size_t)(ph * p.T + j)] : 0.0;
}
// k_adj_gather: a = q M + s reads gy[q L + lo[s] + i], i < Tt, coefficient ct[i M + s]
static double coef_gather(const Plan &p, const AdjTables &t, int64_t a, int64_t k)
{
    const int64_t q = a / p.M, s = a - q * p.M, i = k - (q * p.L + t.lo[(size_t)s]);
    return (i >= 0 && i < t.Tt) ? t.ct[(size_t)(i * p.M + s)] : 0.0;
}
// k_adj_tile: a = q Mc + 16 st + rr reads slab frames e0[st] + ii, ii < I, of its period — slab frame 0 is gy[q Lc + dmin] —
// coefficient tab[st][ii][rr]
static double coef_tile(const AdjTables &t, int64_t a, int64_t k)
{
    const int64_t q = a / t.Mc, sc = a - q * t.Mc, st = sc / 16, rr = sc % 16, ii = k - (q * t.Lc + t.dmin + t.e0[(size_t)st]);
    return (ii >= 0 && ii < t.I) ? t.tab[(size_t)((st * t.I + ii) * 16 + rr)] : 0.0;
}

static void check_tables(int id)
{
    const Plan &p = g_plan[id];
    const AdjTables &t = g_tab[id];
    const int64_t L = p.L, M = p.M, T = p.T;
    CHECK(t.tile == (id != PRIME), "plan %d: tile tables %d", id, (int)t.tile);
    CHECK((int64_t)t.lo.size() == M && (int64_t)t.ct.size() == t.Tt * M && t.dmin == t.lo[0], "plan %d: sizes", id);
    CHECK(t.Tt <= fdiv(T * L + M - 1, M) + 1 && t.Tt >= 1, "plan %d: Tt %d above ceil(T L / M) + 1", id, t.Tt);
    for (int64_t s = 1; s < M; ++s) CHECK(t.lo[(size_t)s] >= t.lo[(size_t)s - 1], "plan %d: lo decreases at %ld", id, (long)s);
    CHECK(t.Lc % L == 0 && t.Mc % M == 0 && t.Lc / L == t.Mc / M && t.Mc >= 16 && t.Lc >= 64 && ((t.Lc + t.pad) & 1), "plan %d: Lc %ld Mc %ld pad %d", id, (long)t.Lc, (long)t.Mc, t.pad);
    if (t.tile) {
        CHECK(t.n_st == (t.Mc + 15) / 16 && (int64_t)t.e0.size() == t.n_st && (int64_t)t.tab.size() == (int64_t)t.n_st * t.I * 16, "plan %d: tile sizes", id);
        CHECK(t.I % 4 == 0 && (int64_t)t.I * M < (T + 15) * L + 4 * M, "plan %d: I %d not below (T + 15) L / M + 4", id, t.I);
        int64_t reach = 0;
        for (int32_t st = 0; st < t.n_st; ++st) {
            CHECK(t.e0[(size_t)st] >= 0 && t.e0[(size_t)st] + t.I <= t.wmax, "plan %d: tile %d reaches %d, wmax %d", id, st, t.e0[(size_t)st] + t.I, t.wmax);
            reach = std::max<int64_t>(reach, t.e0[(size_t)st] + t.I);
        }
        CHECK(reach == t.wmax, "plan %d: wmax %d, the widest tile reaches %ld", id, t.wmax, (long)reach);
    } else {
        CHECK(t.n_st == 0 && t.I == 0 && t.wmax == 0 && t.e0.empty() && t.tab.empty(), "plan %d: tile fields without tile tables", id);
        CHECK(t.Lc > 8192 || t.Mc > 65536, "plan %d: the cut-off", id);
    }
    // every k where the whole matrix is small; else every k a table or the true support could touch, and 8 either side
    const int64_t n_a = 3 * t.Mc, n_k = fdiv((n_a + T) * L, M) + 8;
    const bool whole = n_a * n_k <= 4000000;
    const int64_t span = (t.tile ? std::max<int64_t>(t.I, t.Tt) : t.Tt) + 8;
    for (int64_t a = 0; a < n_a; ++a) {
        const int64_t mid = fdiv(a * L, M), half = fdiv((T / 2 + 16) * L, M) + span;
        const int64_t k0 = whole ? 0 : std::max<int64_t>(0, mid - half), k1 = whole ? n_k : mid + half;
        for (int64_t k = k0; k < k1; ++k) {
            const double want = coef_forward(p, a, k), got = coef_gather(p, t, a, k);
            CHECK(got == want, "plan %d: ct / lo give %.17g for gx[%ld] <- gy[%ld], the forward bank %.17g", id, got, (long)a, (long)k, want);
            if (t.tile) {
                const double got2 = coef_tile(t, a, k);
                CHECK(got2 == want, "plan %d: tab / e0 give %.17g for gx[%ld] <- gy[%ld], the forward bank %.17g", id, got2, (long)a, (long)k, want);
            }
        }
    }
}

// ---- forms -------------------------------------------------------------------------------------------------------------------
// adj_launch's tile branch as it stood (literals and all), on the geometry's raw numbers
struct OldForm { bool tile = false; int lanes = 0; size_t lds = 0; int32_t cg = 0, pb = 0, xc = 0, shift = 0, nw = 0; uint32_t groups = 0, gy = 0; int64_t gx = 0; int z = 0; };
static OldForm old_form(const AdjTables &b, size_t width, int64_t out_frames, uint32_t n_clips, uint32_t n_channels, bool inter)
{
    OldForm o;
    if (b.tile && out_frames >= 4 * b.Mc) {
        for (size_t limit : {(size_t)80 * 1024, (size_t)160 * 1024}) {
            for (int ln : {64, 32, 16}) {
                const int32_t cg = inter ? (int32_t)std::min<uint32_t>(n_channels, (uint32_t)ln) : 1, pb = ln / cg;
                const int64_t xc = (int64_t)(pb - 1) * b.Lc + b.wmax, rows = (xc + b.Lc - 1) / b.Lc;
                const size_t need = (size_t)(rows * (b.Lc + b.pad)) * (size_t)cg * width;
                if (need <= limit) { o.lanes = ln; o.lds = need; o.cg = cg; o.pb = pb; o.xc = (int32_t)xc; break; }
            }
            if (o.lanes) break;
        }
        const int64_t n_per = (out_frames + b.Mc - 1) / b.Mc;
        const int64_t gx = o.lanes ? (n_per + o.pb - 1) / o.pb : 0;
        if (o.lanes && gx <= 2147483647LL) {
            o.shift = -1;
            for (int sh = 0; sh < 7; ++sh)
                if ((1 << sh) == o.cg) o.shift = sh;
            o.groups = (n_channels + (uint32_t)o.cg - 1) / (uint32_t)o.cg;
            const uint64_t cols = (uint64_t)n_clips * o.groups;
            o.gy = (uint32_t)std::min<uint64_t>(cols, 65535);
            const int64_t wgs = gx * (int64_t)o.gy;
            int z = (int)std::min<int64_t>(b.n_st, std::max<int64_t>(1, 1024 / wgs));
            int nw = std::min(16, (b.n_st + z - 1) / z);
            z = std::min(z, (b.n_st + nw - 1) / nw);
            o.gx = gx; o.z = z; o.nw = nw; o.tile = true;
        }
    }
    return o;
}

// tests/test_gpu_adjoint_forms.py's FORMS: what each case's launch log showed on the GPU (-1: the table does not name it)
struct FormCase { const char *name; int plan; int64_t n_x; uint32_t clips, ch; size_t width; bool tile; int block, gz, n_st, cg, pb, lanes; long lds; long gx, gy; };
static const FormCase kForms[] = {
    {"a_f32", DOWN_QQ, 3533, 40, 1, 4, true, 128, 14, -1, -1, -1, -1, -1, -1, -1},
    {"a_f64", DOWN_QQ, 3533, 40, 1, 8, true, 128, 14, -1, -1, -1, -1, -1, -1, -1},
    {"b_f32", DOWN_QQ, 3533, 600, 1, 4, true, 1024, 1, 28, -1, -1, -1, -1, -1, -1},
    {"b_f64", DOWN_QQ, 3533, 600, 1, 8, true, 1024, 1, 28, -1, -1, -1, -1, -1, -1},
    {"c_f32", DOWN_LQ, 3205, 600, 1, 4, true, 1024, 1, 40, -1, -1, -1, -1, -1, -1},
    {"d2_f64", DOWN_QQ, 3533, 300, 2, 8, true, 640, -1, -1, 2, 32, -1, -1, -1, -1},
    {"d4_f32", DOWN_QQ, 3533, 300, 4, 4, true, 640, -1, -1, 4, 16, -1, -1, -1, -1},
    {"d5_f64", DOWN_QQ, 3533, 200, 5, 8, true, 384, -1, -1, 5, 12, -1, -1, -1, -1},
    {"e_f32", DOWN_QQ, 3533, 40, 70, 4, true, -1, 1, -1, 64, -1, 64, -1, -1, 80},
    {"e_f64", DOWN_QQ, 3533, 40, 70, 8, true, -1, -1, -1, 32, -1, 32, -1, -1, 120},
    {"f_f64", UP_640, 597, 1, 1, 8, true, -1, -1, -1, -1, -1, 16, 87176, -1, -1},
    {"g_f64", UP_441, 329, 1, 8, 8, true, -1, -1, -1, -1, -1, 32, 141120, -1, -1},
    {"h_f64", UP_640, 597, 1, 64, 8, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"i_f32", PRIME, 2 * 9973 + 5, 1, 1, 4, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"i_f64", PRIME, 2 * 9973 + 5, 1, 1, 8, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"i3_f32", PRIME, 2 * 9973 + 5, 1, 3, 4, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"i3_f64", PRIME, 2 * 9973 + 5, 1, 3, 8, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"j_f32", TRIPLE, 91, 65600, 1, 4, true, -1, -1, -1, -1, -1, -1, -1, -1, 65535},
    {"k_f32", TRIPLE, 5, 65600, 1, 4, false, -1, -1, -1, -1, -1, -1, -1, -1, 65535},
    {"l87_f64", TRIPLE, 87, 1, 1, 8, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"l88_f64", TRIPLE, 88, 1, 1, 8, true, -1, -1, -1, -1, -1, -1, -1, 1, -1},
    {"l1408_f64", TRIPLE, 1408, 1, 1, 8, true, -1, -1, -1, -1, 64, -1, -1, 1, -1},
    {"l1409_f64", TRIPLE, 1409, 1, 1, 8, true, -1, -1, -1, -1, 64, -1, -1, 2, -1},
    // the non-finite cotangent jobs (NF_JOBS): 4000 frames tiled, 600 (< 4 Mc = 640) lane per element
    {"nf_tile_f32", NF_CASE, 4000, 1, 1, 4, true, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"nf_tile_f64", NF_CASE, 4000, 1, 1, 8, true, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"nf_gather_f32", NF_CASE, 600, 1, 1, 4, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {"nf_gather_f64", NF_CASE, 600, 1, 1, 8, false, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};

static void check_form_cases()
{
    for (const FormCase &c : kForms) {
        const AdjTables &t = g_tab[c.plan];
        const AdjTileForm f = adj_tile_form(t, c.width, c.n_x, c.clips, c.ch, c.ch > 1); // (the test's tensors: channel index fastest)
        CHECK(f.ok == c.tile, "%s: kernel %s", c.name, f.ok ? "adj_tile" : "adj_gather");
        if (!c.tile) {
            const AdjGrid g = adj_gather_grid(c.n_x, c.clips, c.ch);
            CHECK(g.ok && g.gx == (uint64_t)(c.n_x * c.ch + 255) / 256 && (c.gy < 0 || g.gy == (uint32_t)c.gy), "%s: gather grid %u x %u", c.name, g.gx, g.gy);
            continue;
        }
        if (!f.ok) continue;
        CHECK(c.block < 0 || f.n_waves * 64 == c.block, "%s: block %d", c.name, f.n_waves * 64);
        CHECK(c.gz < 0 || f.gz == c.gz, "%s: gz %d", c.name, f.gz);
        CHECK(c.n_st < 0 || t.n_st == c.n_st, "%s: n_st %d", c.name, t.n_st);
        CHECK(c.cg < 0 || f.cg == c.cg, "%s: cg %d", c.name, f.cg);
        CHECK(c.pb < 0 || f.pb == c.pb, "%s: pb %d", c.name, f.pb);
        CHECK(c.lanes < 0 || f.lanes == c.lanes, "%s: lanes %d", c.name, f.lanes);
        CHECK(c.lds < 0 || f.lds == (size_t)c.lds, "%s: lds %zu", c.name, f.lds);
        CHECK(c.gx < 0 || f.gx == c.gx, "%s: gx %ld", c.name, (long)f.gx);
        CHECK(c.gy < 0 || f.gy == (uint32_t)c.gy, "%s: gy %u", c.name, f.gy);
        // what the test asserts of every tiled launch
        CHECK(0 < f.cg * f.pb && f.cg * f.pb <= f.lanes && f.gy == std::min<uint64_t>((uint64_t)c.clips * ((c.ch + f.cg - 1) / f.cg), 65535), "%s: cg %d pb %d gy %u", c.name, f.cg, f.pb, f.gy);
    }
    // the shapes the test's comments name: Mc and the phase tiles
    CHECK(g_tab[DOWN_QQ].Mc == 441 && g_tab[DOWN_QQ].n_st == 28 && g_tab[DOWN_LQ].Mc == 640 && g_tab[DOWN_LQ].n_st == 40, "the downsamplers' periods");
    CHECK(g_tab[UP_640].Lc == 640 && g_tab[UP_441].Lc == 441 && g_tab[PRIME].Lc == 12289 && g_tab[TRIPLE].Mc == 22 && g_tab[NF_CASE].Mc == 160, "the upsamplers' periods");
}

// need(ln): the slab of ln lanes, stated from the geometry (not through the header)
static size_t slab_bytes(const AdjTables &t, int ln, uint32_t ch, bool inter, size_t width)
{
    const int64_t cg = inter ? std::min<int64_t>(ch, ln) : 1, pb = ln / cg, frames = (pb - 1) * t.Lc + t.wmax, rows = (frames + t.Lc - 1) / t.Lc;
    return (size_t)(rows * (t.Lc + t.pad) * cg) * width;
}

static void check_form_sweep()
{
    const int plans[] = {DOWN_QQ, DOWN_LQ, UP_640, UP_441, TRIPLE, NF_CASE, PRIME};
    const uint32_t clip_counts[] = {1, 3, 40, 600, 65535, 65600};
    for (int id : plans) {
        const AdjTables &t = g_tab[id];
        const int64_t Mc = t.Mc, lens[] = {1, 4 * Mc - 1, 4 * Mc, 4 * Mc + 1, 5 * Mc, 63 * Mc + 1, 64 * Mc, 64 * Mc + 1, 1000 * Mc + 7, ((int64_t)1 << 33) * Mc,
                                        (int64_t)2147483647 * 64 * Mc, (int64_t)2147483647 * 64 * Mc + 1, ((int64_t)1 << 37) * Mc + 1}; // (mono: 2^31 - 1 spans, one more)
        for (int64_t n_x : lens)
            for (uint32_t ch = 1; ch <= 130; ++ch)
                for (size_t width : {(size_t)4, (size_t)8})
                    for (int inter = 0; inter < (ch > 1 ? 2 : 1); ++inter)
                        for (uint32_t clips : clip_counts) {
                            const AdjTileForm f = adj_tile_form(t, width, n_x, clips, ch, inter);
                            const OldForm o = old_form(t, width, n_x, clips, ch, inter);
                            CHECK(f.ok == o.tile && f.lanes == o.lanes && f.lds == o.lds && f.cg == o.cg && f.pb == o.pb && f.x_count == o.xc,
                                  "plan %d n_x %ld ch %u width %zu inter %d clips %u: lanes %d lds %zu cg %d pb %d, the loops %d %zu %d %d", id, (long)n_x, ch, width, inter, clips,
                                  f.lanes, f.lds, f.cg, f.pb, o.lanes, o.lds, o.cg, o.pb);
                            if (!f.ok) {
                                CHECK(!t.tile || n_x < 4 * Mc || !f.lanes || f.gx > 2147483647LL, "plan %d n_x %ld ch %u: no tile form", id, (long)n_x, ch);
                                if (t.tile && n_x >= 4 * Mc && !f.lanes)
                                    for (int ln : {64, 32, 16}) CHECK(slab_bytes(t, ln, ch, inter, width) > 160 * 1024, "plan %d ch %u: %d lanes fit", id, ch, ln);
                                continue;
                            }
                            CHECK(f.cg_shift == o.shift && f.n_groups == o.groups && f.gx == o.gx && f.gy == o.gy && f.gz == o.z && f.n_waves == o.nw,
                                  "plan %d n_x %ld ch %u width %zu inter %d clips %u: grid %ld x %u x %d of %d waves, the loops %ld x %u x %d of %d", id, (long)n_x, ch, width, inter, clips,
                                  (long)f.gx, f.gy, f.gz, f.n_waves, (long)o.gx, o.gy, o.z, o.nw);
                            // the slab fits its limit, and a smaller limit or more lanes would not have done
                            CHECK(f.lds == slab_bytes(t, f.lanes, ch, inter, width) && f.lds <= 160 * 1024, "plan %d ch %u: lds %zu", id, ch, f.lds);
                            const size_t limit = f.lds <= 80 * 1024 ? 80 * 1024 : 160 * 1024;
                            for (int ln : {64, 32, 16}) {
                                if (limit > 80 * 1024) CHECK(slab_bytes(t, ln, ch, inter, width) > 80 * 1024, "plan %d ch %u: %d lanes fit 80 KB", id, ch, ln);
                                if (ln > f.lanes) CHECK(slab_bytes(t, ln, ch, inter, width) > limit, "plan %d ch %u: %d lanes fit", id, ch, ln);
                            }
                            CHECK(f.pb * f.cg == f.lanes || (f.cg == (int32_t)ch && (int)ch < f.lanes && f.pb == f.lanes / f.cg), "plan %d ch %u: pb %d cg %d lanes %d", id, ch, f.pb, f.cg, f.lanes);
                            CHECK(inter ? f.cg == (int32_t)std::min<uint32_t>(ch, f.lanes) : f.cg == 1, "plan %d ch %u inter %d: cg %d", id, ch, inter, f.cg);
                            CHECK(f.cg_shift < 0 ? (f.cg & (f.cg - 1)) != 0 : (1 << f.cg_shift) == f.cg, "plan %d: cg %d shift %d", id, f.cg, f.cg_shift);
                            CHECK((uint64_t)f.n_groups * f.cg >= ch && (uint64_t)(f.n_groups - 1) * f.cg < ch, "plan %d ch %u: %u groups of %d", id, ch, f.n_groups, f.cg);
                            CHECK(f.x_count == (f.pb - 1) * t.Lc + t.wmax, "plan %d: x_count %d", id, f.x_count);
                            // every period and every phase tile has a workgroup and a wave; the grid's limits
                            CHECK(f.gx * f.pb * Mc >= n_x && (f.gx - 1) * f.pb * Mc < n_x && f.gx <= 2147483647LL, "plan %d n_x %ld: gx %ld of %d periods", id, (long)n_x, (long)f.gx, f.pb);
                            CHECK(f.gy >= 1 && f.gy <= 65535 && f.gy == std::min<uint64_t>((uint64_t)clips * f.n_groups, 65535), "plan %d: gy %u", id, f.gy);
                            // a wave per phase tile over the z workgroups of a slab — or, at the cap of 16 waves, the kernel's tile loop
                            // wraps (case b of the GPU module: 16 waves, gz 1, 28 tiles) — and no workgroup without a tile
                            CHECK(f.gz >= 1 && f.n_waves >= 1 && f.n_waves <= 16 && ((int64_t)f.gz * f.n_waves >= t.n_st || f.n_waves == 16) && (int64_t)(f.gz - 1) * f.n_waves < t.n_st,
                                  "plan %d: gz %d x %d waves for %d tiles", id, f.gz, f.n_waves, t.n_st);
                            // z workgroups per slab only while the grid stays at the target
                            CHECK(f.gz == 1 || f.gx * f.gy * f.gz <= 1024, "plan %d: %ld x %u x %d workgroups", id, (long)f.gx, f.gy, f.gz);
                        }
    }
    // a slab that meets a limit exactly fits it (no designed geometry does: Lc + pad is odd — these two are made up)
    AdjGeom g;
    g.tile = true; g.Mc = 16; g.n_st = 1; g.pad = 1; g.wmax = 100;
    g.Lc = 319;
    const AdjTileForm at80 = adj_tile_form(g, 4, 64, 1, 1, false);
    CHECK(at80.ok && at80.lanes == 64 && at80.lds == 80 * 1024, "a slab of 80 KB: %d lanes, %zu bytes", at80.lanes, at80.lds);
    g.Lc = 2559;
    const AdjTileForm at160 = adj_tile_form(g, 4, 64, 1, 1, false);
    CHECK(at160.ok && at160.lanes == 16 && at160.lds == 160 * 1024, "a slab of 160 KB: %d lanes, %zu bytes", at160.lanes, at160.lds);
    CHECK(kAdjMinPeriods == 4 && kAdjRS == 16 && kAdjMaxWaves == 16 && kAdjWgTarget == 1024 && kAdjLdsPair == 81920 && kAdjLdsWhole == 163840 && kAdjMaxGridX == 2147483647LL, "the constants");
}

static void check_grids()
{
    CHECK(same(kAdjTooLong, "adjoint job: too long for one launch"), "the text");
    const int64_t lens[] = {1, 255, 256, 257, 65536, ((int64_t)1 << 31) * 256 - 256, ((int64_t)1 << 31) * 256 - 255, (int64_t)2147483647 * 256, (int64_t)2147483647 * 256 + 1, (int64_t)1 << 45};
    for (int64_t n_x : lens)
        for (uint32_t ch : {1u, 2u, 3u, 256u})
            for (uint32_t clips : {1u, 65535u, 65536u, 70000u}) {
                const AdjGrid g = adj_gather_grid(n_x, clips, ch);
                const __int128 elems = (__int128)n_x * ch, gx = (elems + 255) / 256;
                CHECK(g.ok == (gx <= 2147483647), "gather n_x %ld ch %u", (long)n_x, ch);
                if (g.ok) CHECK(g.gx == (uint64_t)gx && g.gy == (clips < 65535 ? clips : 65535), "gather grid n_x %ld ch %u clips %u: %u x %u", (long)n_x, ch, clips, g.gx, g.gy);
            }
    // k_adj_interp: 256 frames per workgroup; (n_x + T) L and n_y M below 2^62
    struct Ratio { int64_t L, M; int32_t T; };
    const Ratio ratios[] = {{1, 1, 8}, {44101, 48000, 32}, {(int64_t)1 << 40, 3, 16}, {3, (int64_t)1 << 40, 16}};
    const int64_t ilens[] = {1, 255, 256, 257, ((int64_t)1 << 22) - 17, ((int64_t)1 << 22) - 16, (int64_t)2147483647 * 256, (int64_t)2147483647 * 256 + 1, (int64_t)1 << 45}; // (2^22 - 16 + T) 2^40 = 2^62
    for (const Ratio &r : ratios)
        for (int64_t n_x : ilens)
            for (int64_t n_y : {(int64_t)0, (int64_t)1, (int64_t)1 << 22, ((int64_t)1 << 22) + 1, (int64_t)1 << 45})
                for (uint64_t cols : {(uint64_t)1, (uint64_t)65535, (uint64_t)65536, (uint64_t)1 << 40}) {
                    const AdjGrid g = adj_interp_grid(r.L, r.M, r.T, n_y, n_x, cols, 256);
                    const __int128 lim = (__int128)1 << 62, gx = ((__int128)n_x + 255) / 256;
                    const bool want = (__int128)(n_x + r.T) * r.L < lim && (__int128)n_y * r.M < lim && gx <= 2147483647;
                    CHECK(g.ok == want, "interp L %ld M %ld n_x %ld n_y %ld", (long)r.L, (long)r.M, (long)n_x, (long)n_y);
                    if (g.ok) CHECK(g.gx == (uint64_t)gx && g.gy == (cols < 65535 ? cols : 65535), "interp grid %u x %u", g.gx, g.gy);
                }
}

// ---- refusals --------------------------------------------------------------------------------------------------------------
// include/hipsoxr.h's values, restated (the header under test never sees them)
enum { F32 = 0, F64 = 1, I32 = 2, I16 = 3, F16 = 4, BF16 = 5 };
enum { AUTO = 0, GATHER = 1, TILE = 2, TILE_VALU = 3, TILE_MFMA = 4, FFT = 5, EXACT = 6, WAVE_DOT = 7, FFT_F64 = 8, FFT_PCM = 9, ADJOINT = 10 };
struct Raw { int elem, kernel; bool vr; int phases; int64_t in_abs0, out_k0; bool table; int64_t in_frames, out_frames; };
static uint64_t len_rule(uint64_t n) { return (n * 147 + 159) / 160; } // some plan's output length

// the two entries' lists as they stood, on the raw values (the ragged entry's rows are valid here: job_rules_check has them)
static const char *old_equal(Raw j)
{
    if (j.elem == F16 || j.elem == BF16) j.elem = F32; // asked of the float32 job
    const bool by_name = j.kernel == ADJOINT;
    if (j.elem != F32 && j.elem != F64) return "adjoint job: float32 or float64 elements only (integer types have no gradient)";
    if (by_name && j.vr) return "adjoint job: variable-rate plans are not served (HIPSOXR_KERNEL_ADJOINT takes constant-rate plans)";
    if (j.phases && !by_name) return "adjoint job: needs an exact-bank plan (interpolated-phase plans and the two-stage form are not served)";
    if (j.in_abs0 != 0 || j.out_k0 != 0) return "adjoint job: whole signals only (in_abs0 == 0, out_k0 == 0)";
    if (j.table) return "adjoint job: ragged batches (clip_table) are served by hipsoxr_run_device_adjoint_ragged, not by this entry";
    if (j.kernel != AUTO && j.kernel != EXACT && !by_name)
        return "adjoint job: the kernel selector must be AUTO or EXACT (the adjoint is the exact engine's; the frequency-domain engine has none)";
    if (j.in_frames < 0 || j.out_frames < 0) return "adjoint job: invalid job extent";
    if ((uint64_t)j.in_frames > len_rule((uint64_t)j.out_frames)) return "adjoint job: in_frames (cotangent frames) exceeds the plan's output length for out_frames";
    return nullptr;
}
static const char *old_ragged(const Raw &j)
{
    const bool by_name = j.kernel == ADJOINT;
    if (j.elem == F16 || j.elem == BF16)
        return "adjoint job: ragged: float16 / bfloat16 clip tables are not served (float32 or float64; half cotangents clip by clip through hipsoxr_run_device_adjoint)";
    if (j.elem != F32 && j.elem != F64) return "adjoint job: float32 or float64 elements only (integer types have no gradient)";
    if (j.vr) return "adjoint job: variable-rate plans are not served (ragged batches take constant-rate plans)";
    if (j.phases && !by_name) return "adjoint job: needs an exact-bank plan (interpolated-phase plans are served by name, HIPSOXR_KERNEL_ADJOINT)";
    if (j.in_abs0 != 0 || j.out_k0 != 0) return "adjoint job: whole signals only (in_abs0 == 0, out_k0 == 0)";
    if (j.kernel != AUTO && j.kernel != EXACT && !by_name)
        return "adjoint job: the kernel selector must be AUTO or EXACT (the adjoint is the exact engine's; the frequency-domain engine has none)";
    if (!j.table) return "adjoint job: the ragged entry needs a clip_table (equal-length clips: hipsoxr_run_device_adjoint)";
    if (j.in_frames < 0 || j.out_frames < 0) return "adjoint job: invalid job extent";
    return nullptr;
}
// ... and as the entries ask the header now (adjoint.hip: adj_ask, launch_adjoint, launch_adjoint_ragged)
static const char *new_entry(AdjEntry entry, Raw j)
{
    if (entry == kAdjEqual && (j.elem == F16 || j.elem == BF16)) j.elem = F32;
    AdjAsk q;
    q.half = j.elem == F16 || j.elem == BF16;
    q.real = j.elem == F32 || j.elem == F64;
    q.by_name = j.kernel == ADJOINT;
    q.auto_or_exact = j.kernel == AUTO || j.kernel == EXACT;
    q.vr = j.vr; q.phases = j.phases != 0;
    q.window = j.in_abs0 != 0 || j.out_k0 != 0;
    q.table = j.table;
    if (const char *e = adj_entry_refusal(entry, q)) return e;
    return adj_extent_refusal(entry, j.in_frames, j.out_frames, len_rule);
}

static void check_refusals()
{
    const int64_t extents[] = {-1, 0, 1, 160, 161, 1000};
    const int elems[] = {F32, F64, I32, I16, F16, BF16, 9};
    for (int elem : elems)
        for (int kernel = AUTO; kernel <= ADJOINT; ++kernel)
            for (int vr = 0; vr < 2; ++vr)
                for (int phases : {0, 64})
                    for (int w = 0; w < 4; ++w)
                        for (int table = 0; table < 2; ++table)
                            for (int64_t n_y : extents)
                                for (int64_t n_x : extents) {
                                    const Raw j = {elem, kernel, vr != 0, phases, (w & 1) ? 3 : 0, (w & 2) ? -2 : 0, table != 0, n_y, n_x};
                                    const char *e0 = old_equal(j), *e1 = new_entry(kAdjEqual, j);
                                    CHECK(same(e0, e1), "equal-length entry, elem %d kernel %d vr %d phases %d window %d table %d n_y %ld n_x %ld: \"%s\", was \"%s\"", elem, kernel, vr, phases, w,
                                          table, (long)n_y, (long)n_x, e1 ? e1 : "", e0 ? e0 : "");
                                    const char *r0 = old_ragged(j), *r1 = new_entry(kAdjRagged, j);
                                    CHECK(same(r0, r1), "ragged entry, elem %d kernel %d vr %d phases %d window %d table %d n_y %ld n_x %ld: \"%s\", was \"%s\"", elem, kernel, vr, phases, w, table,
                                          (long)n_y, (long)n_x, r1 ? r1 : "", r0 ? r0 : "");
                                }
    CHECK(!adj_row_refusal(kJobRowOk) && same(adj_row_refusal(kJobRowNegative), "adjoint job: ragged: a clip's offset or frame count is negative"), "row texts");
    CHECK(same(adj_row_refusal(kJobRowAboveJob), "adjoint job: ragged: a clip's frame count is above the job's in_frames / out_frames (the largest per-clip values)"), "row texts");
    CHECK(same(adj_row_refusal(kJobRowAbovePlan), "adjoint job: ragged: a clip's n_y (cotangent frames) exceeds the plan's output length for its n_x"), "row texts");
}

int main()
{
    for (int id = 0; id < N_PLANS; ++id) {
        const char *e = plan_design(kPlans[id].in_rate, kPlans[id].out_rate, (unsigned long)kPlans[id].recipe, &g_plan[id]);
        CHECK(!e && g_plan[id].phases == 0, "plan %g -> %g: %s", kPlans[id].in_rate, kPlans[id].out_rate, e ? e : "no exact bank");
        if (e || g_plan[id].phases) { std::printf("%ld checks, %ld failed\n", g_checks, g_failed); return 1; }
        g_tab[id] = adj_tables(g_plan[id].L, g_plan[id].M, g_plan[id].T, g_plan[id].bank.data());
    }
    for (int id = 0; id < N_PLANS; ++id) check_tables(id);
    check_form_cases();
    check_form_sweep();
    check_grids();
    check_refusals();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
