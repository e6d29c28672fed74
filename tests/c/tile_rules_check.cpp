// tile_rules_check.cpp — the rules of a tile launch on the exact engine (python-soxr_amd/csrc/tile_rules.h) against slow,
// independent statements: every period of a job in exactly one block, the kernels' own walks (kernels_tile.h: k_tile,
// k_tile_mfma with its halves form, the planar kernels with their XCD-aware ids) replayed over the chosen form, the waves
// rule against a recount, planes_form against its cost formula, the LDS figures, the family truth table, a ragged launch of
// equal clips against the equal-length job.  A table of real geometries (recorded from build_tile_tables / build_mfma_planes)
// leads every group of random ones.  No device, no library.  Exit status 0 = every check held (tests/test_tile_rules.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "ragged_rules.h"
#include "tile_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

// {width, variant, aligned, n_rt, pad, x_count, Lc, Mc, lds_bytes, rowR, plane, span, pb}: what the builders gave for the plan named
struct Real { int width, variant, aligned, n_rt, pad, x_count; long Lc, Mc; long lds_bytes; int rowR, plane, span, pb; };
static const Real kReal[] = {
    {4, 0, 1, 1, 4, 784, 16, 8, 4752, 0, 0, 280, 64}, // 100 -> 200 VHQ
    {4, 0, 1, 1, 4, 560, 16, 8, 3408, 0, 0, 56, 64}, // 100 -> 200 LQ
    {4, 0, 1, 10, 4, 10536, 147, 160, 43232, 0, 0, 456, 64}, // 48000 -> 44100 VHQ
    {4, 0, 1, 10, 4, 10456, 147, 160, 42912, 0, 0, 376, 64}, // 48000 -> 44100 HQ
    {4, 0, 0, 10, 0, 9460, 160, 147, 37872, 0, 0, 196, 64}, // 44100 -> 48000 LQ
    {4, 0, 0, 10, 0, 28960, 160, 441, 115872, 0, 0, 1176, 64}, // 44100 -> 16000 VHQ
    {4, 0, 0, 10, 0, 28760, 160, 441, 115072, 0, 0, 976, 64}, // 44100 -> 16000 HQ
    {4, 0, 0, 20, 0, 9460, 320, 147, 37872, 0, 0, 196, 64}, // 44100 -> 96000 LQ
    {4, 0, 0, 20, 0, 9572, 320, 147, 38320, 0, 0, 308, 64}, // 44100 -> 96000 MQ
    {4, 0, 0, 20, 0, 28592, 320, 441, 114400, 0, 0, 808, 64}, // 44100 -> 32000 VHQ
    {4, 0, 0, 20, 0, 28496, 320, 441, 114016, 0, 0, 712, 64}, // 44100 -> 32000 HQ
    {4, 0, 0, 20, 0, 28232, 320, 441, 112960, 0, 0, 448, 64}, // 44100 -> 32000 QQ
    {4, 0, 1, 28, 4, 20528, 441, 320, 83184, 0, 0, 368, 64}, // 32000 -> 44100 LQ
    {4, 0, 1, 28, 4, 20640, 441, 320, 83632, 0, 0, 480, 64}, // 32000 -> 44100 MQ
    {8, 0, 1, 1, 4, 560, 16, 8, 6816, 0, 0, 56, 64}, // 100 -> 200 LQ
    {8, 0, 1, 10, 4, 10536, 147, 160, 86464, 0, 0, 456, 64}, // 48000 -> 44100 VHQ
    {8, 0, 1, 10, 4, 10456, 147, 160, 85824, 0, 0, 376, 64}, // 48000 -> 44100 HQ
    {8, 0, 1, 10, 4, 10664, 147, 320, 86464, 0, 0, 744, 32}, // 48000 -> 22050 HQ
    {8, 0, 0, 10, 0, 14848, 160, 441, 118848, 0, 0, 1176, 32}, // 44100 -> 16000 VHQ
    {8, 0, 0, 10, 0, 14648, 160, 441, 117248, 0, 0, 976, 32}, // 44100 -> 16000 HQ
    {8, 0, 0, 20, 0, 9460, 320, 147, 75744, 0, 0, 196, 64}, // 44100 -> 96000 LQ
    {8, 0, 0, 20, 0, 14480, 320, 441, 115904, 0, 0, 808, 32}, // 44100 -> 32000 VHQ
    {8, 0, 0, 20, 0, 14384, 320, 441, 115136, 0, 0, 712, 32}, // 44100 -> 32000 HQ
    {8, 0, 0, 40, 0, 14124, 640, 441, 113056, 0, 0, 452, 32}, // 22050 -> 32000 QQ
    {4, 1, 0, 10, 2, 10536, 147, 160, 42704, 0, 0, 456, 64}, // 48000 -> 44100 VHQ
    {4, 1, 0, 10, 2, 10456, 147, 160, 42384, 0, 0, 376, 64}, // 48000 -> 44100 HQ
    {4, 1, 0, 10, 0, 9460, 160, 147, 37872, 0, 0, 196, 64}, // 44100 -> 48000 LQ
    {4, 1, 0, 10, 0, 28960, 160, 441, 115872, 0, 0, 1176, 64}, // 44100 -> 16000 VHQ
    {4, 1, 0, 10, 0, 28760, 160, 441, 115072, 0, 0, 976, 64}, // 44100 -> 16000 HQ
    {4, 1, 0, 20, 0, 9460, 320, 147, 37872, 0, 0, 196, 64}, // 44100 -> 96000 LQ
    {4, 1, 0, 20, 0, 28592, 320, 441, 114400, 0, 0, 808, 64}, // 44100 -> 32000 VHQ
    {4, 1, 0, 20, 0, 28496, 320, 441, 114016, 0, 0, 712, 64}, // 44100 -> 32000 HQ
    {4, 1, 0, 20, 0, 28448, 320, 441, 113824, 0, 0, 664, 64}, // 44100 -> 32000 MQ
    {4, 1, 0, 28, 2, 20752, 441, 320, 83560, 0, 0, 592, 64}, // 32000 -> 44100 VHQ
    {4, 1, 0, 40, 0, 28428, 640, 441, 113744, 0, 0, 644, 64}, // 22050 -> 32000 HQ
    {8, 1, 0, 1, 2, 1416, 16, 32, 12112, 0, 0, 424, 32}, // 44100 -> 22050 HQ
    {8, 1, 0, 10, 2, 5416, 147, 160, 43936, 0, 0, 456, 32}, // 48000 -> 44100 VHQ
    {8, 1, 0, 10, 2, 5336, 147, 160, 43296, 0, 0, 376, 32}, // 48000 -> 44100 HQ
    {8, 1, 0, 10, 2, 10284, 147, 320, 82864, 0, 0, 364, 32}, // 48000 -> 22050 QQ
    {8, 1, 0, 10, 0, 14848, 160, 441, 118848, 0, 0, 1176, 32}, // 44100 -> 16000 VHQ
    {8, 1, 0, 10, 0, 14648, 160, 441, 117248, 0, 0, 976, 32}, // 44100 -> 16000 HQ
    {8, 1, 0, 20, 0, 4908, 320, 147, 39328, 0, 0, 348, 32}, // 44100 -> 96000 HQ
    {8, 1, 0, 20, 0, 14480, 320, 441, 115904, 0, 0, 808, 32}, // 44100 -> 32000 VHQ
    {8, 1, 0, 20, 0, 14384, 320, 441, 115136, 0, 0, 712, 32}, // 44100 -> 32000 HQ
    {8, 1, 0, 28, 2, 10400, 441, 320, 83792, 0, 0, 480, 32}, // 32000 -> 44100 MQ
    {4, 2, 0, 2, 0, 1312, 32, 16, 6160, 4, 384, 304, 64}, // 100 -> 200 VHQ
    {4, 2, 0, 2, 0, 1184, 32, 16, 5136, 4, 320, 176, 64}, // 100 -> 200 MQ
    {4, 2, 0, 3, 0, 1184, 48, 16, 5136, 4, 320, 176, 64}, // 16000 -> 48000 MQ
    {4, 2, 0, 3, 0, 1088, 48, 16, 5136, 4, 320, 80, 64}, // 16000 -> 48000 LQ
    {4, 2, 0, 10, 4, 10560, 147, 160, 49328, 44, 3072, 480, 64}, // 48000 -> 44100 VHQ
    {4, 2, 0, 10, 4, 10464, 147, 160, 49328, 44, 3072, 384, 64}, // 48000 -> 44100 HQ
    {8, 2, 0, 1, 2, 1440, 16, 32, 16464, 10, 512, 448, 32}, // 44100 -> 22050 HQ
    {8, 2, 0, 10, 2, 5440, 147, 160, 51536, 42, 1600, 480, 32}, // 48000 -> 44100 VHQ
    {8, 2, 0, 10, 2, 5344, 147, 160, 51536, 42, 1600, 384, 32}, // 48000 -> 44100 HQ
    {8, 2, 0, 10, 2, 5312, 147, 160, 51536, 42, 1600, 352, 32}, // 48000 -> 44100 MQ
    {8, 2, 0, 28, 2, 10304, 441, 320, 96912, 82, 3008, 384, 32}, // 32000 -> 44100 LQ
};
static const int kNReal = (int)(sizeof kReal / sizeof *kReal);

static TileGeom geom_of(const Real &r)
{
    TileGeom g;
    g.variant = r.variant; g.aligned = r.aligned != 0; g.n_rt = r.n_rt; g.pad = r.pad; g.x_count = r.x_count; g.Lc = r.Lc; g.Mc = r.Mc;
    g.lds_bytes = (size_t)r.lds_bytes; g.rowR = r.rowR; g.plane = r.plane; g.span = r.span; g.pb = r.pb; g.I_h = 64; g.ok = true;
    return g;
}
// a random geometry with the builders' own relations between its numbers
static TileGeom random_geom(std::mt19937_64 &rng, size_t width)
{
    TileGeom g;
    g.variant = (int)(rng() % 3);
    g.Lc = 16 + (int64_t)(rng() % (rng() % 4 ? 700 : 4000));
    g.Mc = g.variant == 2 ? 16 * (1 + (int64_t)(rng() % 30)) : 1 + (int64_t)(rng() % 600);
    g.aligned = g.variant == 0 && g.Mc % 4 == 0;
    g.n_rt = (int32_t)((g.Lc + 15) / 16);
    g.I_h = 64; g.pad = (int32_t)(rng() % 5); g.span = 4 * (10 + (int32_t)(rng() % 200));
    g.pb = g.variant == 2 ? (width == 4 ? 64 : 32) : (width == 8 || g.variant == 0) ? (16 << (rng() % 3)) : 64;
    g.rowR = (int32_t)g.Mc / 4 + (int32_t)(rng() % 8);
    if (g.variant == 2) {
        const TileSlab s = planes_slab(g, g.pb, width);
        g.x_count = s.x_count; g.plane = s.plane; g.lds_bytes = s.lds_bytes;
    } else {
        g.x_count = ((g.pb - 1) * (int32_t)g.Mc + g.span + 3) / 4 * 4;
        g.lds_bytes = ((size_t)g.x_count + (size_t)g.pad * (g.x_count / g.Mc + 1) + 8) * width;
    }
    g.ok = true;
    return g;
}

static int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// ---- blocks: every period floor(k0 / Lc) .. floor((k0 + n - 1) / Lc) in exactly one block x < n_blocks, no block empty ----
static void check_blocks(std::mt19937_64 &rng)
{
    const int32_t pbs[3] = {16, 32, 64};
    for (int trial = 0; trial < 3000; ++trial) {
        const int64_t Lc = trial < kNReal ? kReal[trial].Lc : 1 + (int64_t)(rng() % 700);
        const int32_t pb = pbs[rng() % 3];
        const int64_t k0 = rng() % 3 == 0 ? 0 : (int64_t)(rng() % (uint64_t)(200 * Lc));
        int64_t n;
        switch (rng() % 4) {
        case 0: n = 1 + (int64_t)(rng() % (uint64_t)Lc); break;
        case 1: n = Lc * pb * (int64_t)(1 + rng() % 5) + (int64_t)(rng() % 3) - 1 - k0 % Lc; break; // at a slab's edge
        default: n = 1 + (int64_t)(rng() % (uint64_t)(Lc * pb * 6));
        }
        if (n < 1) n = 1;
        const int64_t first = floordiv(k0, Lc), last = floordiv(k0 + n - 1, Lc);
        const int64_t periods = tile_periods(k0, n, Lc), nb = tile_blocks(periods, pb);
        CHECK(tile_first_period(k0, Lc) == first && periods == last - first + 1, "k0=%ld n=%ld Lc=%ld: periods %ld", (long)k0, (long)n, (long)Lc, (long)periods);
        std::vector<int> held((size_t)nb, 0);
        bool each_once = true;
        for (int64_t per = first; per <= last; ++per) { // block x holds periods first + x pb .. first + x pb + pb - 1: said one period at a time
            int in = 0;
            for (int64_t x = 0; x < nb; ++x)
                if (per >= first + x * pb && per < first + (x + 1) * pb) { ++in; ++held[(size_t)x]; }
            each_once = each_once && in == 1;
        }
        CHECK(each_once, "k0=%ld n=%ld Lc=%ld pb=%d: a period outside the %ld blocks, or in two", (long)k0, (long)n, (long)Lc, pb, (long)nb);
        bool none_empty = true;
        for (int h : held) none_empty = none_empty && h > 0;
        CHECK(none_empty, "k0=%ld n=%ld Lc=%ld pb=%d: an empty block among %ld", (long)k0, (long)n, (long)Lc, pb, (long)nb);
        // the two spellings the launcher had: (b_hi - b_lo + pb) / pb, and for float64 planar slabs (b_hi - b_lo + 32) / 32
        CHECK(nb == (last - first + pb) / pb, "n_blocks spelling");
        CHECK(tile_blocks(periods, 32) == (last - first + 32) / 32, "float64 slab spelling");
        const int64_t cols = 1 + (int64_t)(rng() % 9);
        CHECK(tile_slabs(periods, pb, cols) == nb * cols, "slabs over columns");
        // a whole signal: the ragged rule counts the same slabs
        CHECK(tile_blocks(tile_periods(0, n, Lc), pb) == ragged_slabs(n, Lc, pb), "ragged_slabs(%ld, %ld, %d)", (long)n, (long)Lc, pb);
    }
}

// ---- waves: n_rt <= 16: one per row tile; above: least waste among 8..16, among ties the most waves ----
static void check_waves()
{
    for (int n_rt = 1; n_rt <= 1100; ++n_rt) {
        const int w = tile_waves(n_rt);
        if (n_rt <= 16) { CHECK(w == n_rt, "n_rt=%d: %d waves", n_rt, w); continue; }
        CHECK(w >= 8 && w <= 16, "n_rt=%d: %d waves", n_rt, w);
        const int waste = (n_rt + w - 1) / w * w - n_rt;
        for (int v = 8; v <= 16; ++v) {
            const int wv = (n_rt + v - 1) / v * v - n_rt;
            CHECK(waste < wv || (waste == wv && w >= v), "n_rt=%d: %d waves waste %d, %d waves waste %d", n_rt, w, waste, v, wv);
        }
    }
}

// ---- planes_form: the cost formula of the comment, recomputed; lowest of the four candidates ----
static double slow_cost(int pb, bool split, int64_t slabs, int n_rt)
{
    const int units = pb == 64 ? 2 * n_rt : n_rt;
    const int wg_per_slab = split ? (units + 3) / 4 : 1;
    int upw = 0; // units per wave: four waves per workgroup
    while (upw * 4 * wg_per_slab < units) ++upw;
    const double wgs = (double)slabs * wg_per_slab;
    double layers = std::ceil(wgs / 256.);
    if (upw > 1) layers = 0.5 * (layers + wgs / 256.);
    else if (pb == 64 && wgs > 384. && wgs <= 768.) layers = 3.;
    const double c0 = pb == 32 ? (upw == 1 ? 1.15 : 2.35) : (upw == 1 ? 1.25 : 3.32);
    const double k = pb == 32 ? (upw == 1 ? 1.153 : 0.958) : (upw == 1 ? 1.41 : 1.052);
    return c0 + layers * upw * k;
}
static void check_planes_form(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 20000; ++trial) {
        const int n_rt = trial < kNReal ? kReal[trial].n_rt : 1 + (int)(rng() % 60);
        const int64_t periods = 1 + (int64_t)(rng() % (rng() % 2 ? 3000 : 300000)), cols = 1 + (int64_t)(rng() % 12);
        const int64_t s64 = tile_slabs(periods, 64, cols), s32 = tile_slabs(periods, 32, cols);
        const PlanesForm f = planes_form(s64, s32, n_rt, false, 0);
        CHECK((f.pb == 64 || f.pb == 32) && (f.split == 1 || f.split == ((f.pb / 32) * n_rt + 3) / 4), "pb=%d split=%d", f.pb, f.split);
        if (s64 >= 2048) { CHECK(f.pb == 64 && f.split == 1, "%ld slabs of 64: pb=%d split=%d", (long)s64, f.pb, f.split); }
        else {
            const double mine = slow_cost(f.pb, f.split > 1, f.pb == 64 ? s64 : s32, n_rt);
            for (int pb : {64, 32})
                for (int sp = 0; sp < 2; ++sp)
                    CHECK(mine <= slow_cost(pb, sp != 0, pb == 64 ? s64 : s32, n_rt), "slabs %ld/%ld n_rt=%d: chose %d/%d at %.4f, %d/%s costs %.4f", (long)s64, (long)s32,
                          n_rt, f.pb, f.split, mine, pb, sp ? "split" : "whole", slow_cost(pb, sp != 0, pb == 64 ? s64 : s32, n_rt));
        }
        for (int force = 1; force <= 4; ++force) { // each forced form gives what its number says
            const PlanesForm ff = planes_form(s64, s32, n_rt, false, force);
            const int pb = force <= 2 ? 64 : 32, full = ((pb / 32) * n_rt + 3) / 4;
            CHECK(ff.pb == pb && ff.split == (force % 2 ? 1 : full), "forced form %d: pb=%d split=%d", force, ff.pb, ff.split);
        }
        CHECK(planes_form(s64, s32, n_rt, true, 0).pb == 32, "dbg_slab32");
    }
}

// ---- the walks of kernels_tile.h, replayed ----
// k_tile (line 171) and k_tile_mfma (lines 328-334): hits[rt][side], side 0 / 1: a half-chain, 2: both
static void walk_rows(const TileForm &f, bool mfma, std::vector<int> &hits)
{
    hits.assign((size_t)f.n_rt * 3, 0);
    const int n_waves = f.n_waves, gz = (int)f.grid[2];
    for (int z = 0; z < gz; ++z)
        for (int wave = 0; wave < (int)f.block / 64; ++wave) {
            if (!mfma) {
                for (int rt = wave < n_waves ? wave + n_waves * z : f.n_rt; rt < f.n_rt; rt += n_waves * gz) ++hits[(size_t)rt * 3 + 2];
                continue;
            }
            const bool halves = f.halves != 0;
            const int units = halves ? n_waves >> 1 : n_waves;
            const int pw = halves ? wave >> 1 : wave, side = halves ? wave & 1 : 2;
            const int stride_rt = units * gz;
            const int rounds = halves ? (f.n_rt + stride_rt - 1) / stride_rt : 0;
            int round = 0;
            for (int rt = wave < n_waves ? pw + units * z : f.n_rt; halves ? round < rounds : rt < f.n_rt; rt += stride_rt, ++round)
                if (rt < f.n_rt) ++hits[(size_t)rt * 3 + side];
        }
}
// the planar kernels (lines 634-637 / 804-806: the id decode; 672 / 830: the unit walk): hits[slab][unit]; false: an id decoded twice
static bool walk_planar(const TileForm &f, int units, std::vector<int> &hits)
{
    hits.assign((size_t)f.nx * units, 0);
    std::vector<int> pair_seen((size_t)f.nx * (f.xz ? f.xz : (int)f.grid[2]), 0);
    bool ok = true;
    for (unsigned bx = 0; bx < f.grid[0]; ++bx)
        for (unsigned gz = 0; gz < f.grid[2]; ++gz) {
            uint32_t bxi = bx, bz = gz, nz = f.grid[2];
            if (f.xz) {
                const uint32_t slot = bx >> 3;
                nz = (uint32_t)f.xz;
                bz = slot % nz;
                bxi = (slot / nz) * 8 + (bx & 7u);
                if (bxi >= (uint32_t)f.nx) continue; // an idle id of the padded grid
            }
            if (bxi >= (uint32_t)f.nx || bz >= nz) { ok = false; continue; }
            if (++pair_seen[(size_t)bxi * nz + bz] != 1) ok = false;
            for (int wave = 0; wave < (int)f.block / 64; ++wave)
                for (int u = wave + f.n_waves * (int)bz; u < units; u += f.n_waves * (int)nz) ++hits[(size_t)bxi * units + u];
        }
    for (int s : pair_seen) ok = ok && s == 1;
    return ok;
}

static void check_form_walk(const TileForm &f, const TileGeom &g, size_t width, const char *what)
{
    CHECK(f.block <= 1024 && f.block % 64 == 0 && f.n_waves <= 16 && f.n_waves >= 1, "%s: block %u, %d waves", what, f.block, f.n_waves);
    CHECK(f.lds <= 160 * 1024, "%s: %zu bytes of LDS (Lc=%ld Mc=%ld pb=%d)", what, f.lds, (long)g.Lc, (long)g.Mc, (int)f.slab.pb);
    CHECK(f.nx == f.n_blocks && f.grid[1] >= 1, "%s: nx", what);
    std::vector<int> hits;
    if (g.variant == 2) {
        const int units = width == 4 ? (f.slab.pb >> 5) * f.n_rt : (f.slab.pb / (16 * f.ng)) * f.n_rt; // hp x n_rt; UPT x n_rt
        CHECK(f.block == 256 && f.n_waves == 4, "%s: a planar workgroup is four waves", what);
        CHECK(f.xz ? (f.grid[2] == 1 && f.xz == f.split && f.grid[0] == (unsigned)((f.n_blocks + 7) / 8 * 8 * f.split)) : (f.grid[2] == (unsigned)f.split && f.grid[0] == (unsigned)f.n_blocks),
              "%s: grid %ux%ux%u xz=%d split=%d", what, f.grid[0], f.grid[1], f.grid[2], (int)f.xz, f.split);
        CHECK(f.split <= (units + 3) / 4, "%s: %d workgroups for %d units", what, f.split, units);
        const bool ids_ok = walk_planar(f, units, hits);
        CHECK(ids_ok, "%s: an id of the grid decodes to no (slab, part) pair or to one twice", what);
        bool once = true;
        for (int h : hits) once = once && h == 1;
        CHECK(once, "%s: a unit of a slab computed twice or not at all (pb=%d split=%d xz=%d)", what, (int)f.slab.pb, f.split, (int)f.xz);
    } else {
        CHECK(f.grid[0] == (unsigned)f.n_blocks && f.grid[2] == (unsigned)f.split && f.xz == 0, "%s: grid", what);
        if (f.split > 1 || f.halves) CHECK(f.block >= 256, "%s: %u threads stage the slab of a split workgroup", what, f.block);
        CHECK(f.halves ? f.n_waves % 2 == 0 && f.n_waves / 2 <= 8 : true, "%s: halves on %d waves", what, f.n_waves);
        walk_rows(f, g.variant == 1, hits);
        bool once = true;
        for (int rt = 0; rt < f.n_rt; ++rt)
            once = once && (f.halves ? hits[(size_t)rt * 3] == 1 && hits[(size_t)rt * 3 + 1] == 1 && hits[(size_t)rt * 3 + 2] == 0
                                     : hits[(size_t)rt * 3] == 0 && hits[(size_t)rt * 3 + 1] == 0 && hits[(size_t)rt * 3 + 2] == 1);
        CHECK(once, "%s: a row tile computed twice or not at all (n_rt=%d nw=%d z=%u halves=%d)", what, f.n_rt, f.n_waves, f.grid[2], f.halves);
        if (f.halves) { // the scratch behind the slab: 64-element aligned, per_wg x 4 x 64 elements
            const int per_wg = f.n_waves / 2;
            CHECK((size_t)f.scratch_off * width >= f.slab.lds_bytes && f.scratch_off % 64 == 0 && f.slab.pb == 16, "%s: scratch at %d, slab %zu bytes", what, (int)f.scratch_off,
                  f.slab.lds_bytes);
            CHECK(f.lds == ((size_t)f.scratch_off + (size_t)per_wg * 4 * 64) * width, "%s: LDS of the halves form", what);
        }
    }
}

// the switches that leave results alone, each alone and a few together
static TileSwitches some_switches(std::mt19937_64 &rng)
{
    TileSwitches sw;
    if (rng() % 2) return sw;
    if (rng() % 4 == 0) sw.dbg_slab32 = true;
    if (rng() % 4 == 0) sw.dbg_slab64 = true;
    if (rng() % 4 == 0) sw.no_halves = true;
    if (rng() % 4 == 0) sw.no_xcd_split = true;
    if (rng() % 4 == 0) sw.no_tile_split = true;
    if (rng() % 4 == 0) sw.dbg_mfma64_split = true;
    if (rng() % 4 == 0) sw.dbg_tile_form = 1 + (int)(rng() % 4);
    if (rng() % 4 == 0) sw.dbg_mfma64_pb = rng() % 2 ? 16 : 32;
    return sw;
}

static int64_t some_periods(std::mt19937_64 &rng, int64_t cols)
{
    static const int64_t edges[] = {96 * 64, 2048 * 64, 4096 * 64, 1536 * 32, 512 * 64, 512 * 32, 512 * 16, 128 * 64, 128 * 32, 128 * 16, 384 * 64, 768 * 64};
    switch (rng() % 4) {
    case 0: return 1 + (int64_t)(rng() % 70);
    case 1: return 1 + (int64_t)(rng() % 3000);
    case 2: return std::max<int64_t>(1, edges[rng() % (sizeof edges / sizeof *edges)] / cols + (int64_t)(rng() % 130) - 65);
    default: return 1 + (int64_t)(rng() % 40000);
    }
}

static void check_forms(std::mt19937_64 &rng)
{
    for (int trial = 0; trial < 40 * kNReal + 6000; ++trial) {
        const bool real = trial < 40 * kNReal;
        const size_t width = real ? (size_t)kReal[trial % kNReal].width : (rng() % 2 ? 4 : 8);
        const TileGeom g = real ? geom_of(kReal[trial % kNReal]) : random_geom(rng, width);
        const uint64_t cols = rng() % 3 == 0 ? 1 : 1 + (uint64_t)(rng() % (rng() % 2 ? 4 : 300));
        const int64_t periods = some_periods(rng, (int64_t)cols);
        const int64_t k0 = rng() % 2 ? 0 : (int64_t)(rng() % (uint64_t)(50 * g.Lc));
        const int64_t n = std::max<int64_t>(1, periods * g.Lc - (int64_t)(rng() % (uint64_t)g.Lc) - k0 % g.Lc);
        const TileSwitches sw = some_switches(rng);
        const TileForm f = tile_form(width, g, k0, n, cols, sw);
        CHECK(!f.err, "a job of %ld outputs x %lu columns refused: %s", (long)n, (unsigned long)cols, f.err ? f.err : "");
        if (f.err) continue;
        CHECK(f.n_blocks == tile_blocks(tile_periods(k0, n, g.Lc), f.slab.pb) && f.grid[1] == cols, "blocks of the form");
        if (!real && f.lds > 160 * 1024) continue; // (a random geometry need not fit; a real one must: check_form_walk)
        if (f.n_blocks * (int64_t)f.split > 40000) continue; // (the replay is per id)
        check_form_walk(f, g, width, real ? "real geometry" : "random geometry");
        // the slab's figures are the plan's own, or re-derived for the slab size taken
        if (g.variant == 2) { const TileSlab s = planes_slab(g, f.slab.pb, width); CHECK(s.x_count == f.slab.x_count && s.plane == f.slab.plane && s.lds_bytes == f.slab.lds_bytes, "planar slab"); }
        if (g.variant == 2 && f.slab.pb == g.pb) CHECK(f.slab.x_count == g.x_count && f.slab.plane == g.plane && f.slab.lds_bytes == g.lds_bytes, "planes_slab(own pb) is the builder's");
        if (g.variant != 2 && f.slab.pb == g.pb) CHECK(f.slab.x_count == g.x_count && f.slab.lds_bytes == g.lds_bytes, "own slab");
        if (g.variant == 1 && g.pb == 16) CHECK(general_slab16(g, width).x_count == g.x_count && general_slab16(g, width).lds_bytes == g.lds_bytes, "general_slab16 is the builder's 16-period slab");
        if (g.variant != 1) CHECK(!f.halves, "halves on another kernel");
        if (f.halves) CHECK(tile_slabs(tile_periods(k0, n, g.Lc), 64, (int64_t)cols) <= 96 || sw.dbg_slab32, "halves on a large job");
    }
    // refusals
    const TileGeom g = geom_of(kReal[0]);
    CHECK(tile_form(4, g, 0, 100000, 65536, TileSwitches()).err == kTileTooManyCols && !tile_form(4, g, 0, 100000, 65535, TileSwitches()).err, "65536 columns");
    TileSwitches s64; s64.dbg_slab64 = true;
    CHECK(tile_form(4, g, 0, g.Lc * 64 * 2147483648LL, 1, s64).err == kTileTooLong && !tile_form(4, g, 0, g.Lc * 64 * 2147483647LL, 1, s64).err, "2^31 blocks");
}

// ---- LDS: every form the rules can choose for a real geometry fits a workgroup's 160 KiB ----
static void check_lds()
{
    for (int i = 0; i < kNReal; ++i) {
        const Real &r = kReal[i];
        const TileGeom g = geom_of(r);
        const size_t width = (size_t)r.width;
        CHECK(g.lds_bytes <= 160 * 1024, "own slab");
        if (g.variant == 2) {
            for (int32_t pb : {64, 32, 16}) {
                if ((width == 4) == (pb == 16)) continue; // float32: 64 or 32; float64: 32 or 16
                CHECK(planes_slab(g, pb, width).lds_bytes <= 160 * 1024, "planar slab of %d periods: %zu bytes", pb, planes_slab(g, pb, width).lds_bytes);
            }
            CHECK(planes_slab(g, g.pb, width).lds_bytes == g.lds_bytes, "planes_slab(own pb) is the builder's figure");
        } else if (g.variant == 1) {
            const TileSlab s = general_slab16(g, width);
            CHECK(s.lds_bytes <= g.lds_bytes || g.pb == 16, "a 16-period slab is no larger than the plan's");
            for (int want = 1; want <= 16; ++want) {
                const HalvesForm h = halves_form(want, g.n_rt, 16, s.lds_bytes, width);
                CHECK(h.lds_bytes <= 160 * 1024 && h.per_wg <= 8 && h.per_wg >= 1 && h.n_waves == 2 * h.per_wg && h.block >= 256 && h.block <= 1024, "halves form: %zu bytes, %d per workgroup", h.lds_bytes, h.per_wg);
                CHECK((size_t)h.scratch_off * width >= s.lds_bytes && h.scratch_off % 64 == 0 && h.lds_bytes == ((size_t)h.scratch_off + (size_t)h.per_wg * 4 * 64) * width, "scratch");
            }
        }
    }
}

// ---- family: selector x gv.ok x gm.ok x big against a literal table ----
static void check_family()
{
    // rows: selector; columns: (gv_ok, gm_ok, big) = 000 001 010 011 100 101 110 111.  G gather, M MFMA tile, V VALU tile, O other, R refused
    static const char *want[6] = {
        /* AUTO      */ "G-GMGVGM", // (-: big without a geometry does not occur: tile_big)
        /* GATHER    */ "GGGGGGGG",
        /* TILE      */ "RRMMVVMM",
        /* TILE_VALU */ "RRRRVVVV",
        /* TILE_MFMA */ "RRMMRRMM",
        /* other     */ "OOOOOOOO",
    };
    const TileSelector sels[6] = {kSelAuto, kSelGather, kSelTile, kSelTileValu, kSelTileMfma, kSelOther};
    for (int s = 0; s < 6; ++s)
        for (int c = 0; c < 8; ++c) {
            if (want[s][c] == '-') continue;
            const TileFamily f = tile_family(sels[s], (c & 4) != 0, (c & 2) != 0, (c & 1) != 0);
            const char got = f == kFamGather ? 'G' : f == kFamTileMfma ? 'M' : f == kFamTileValu ? 'V' : f == kFamOther ? 'O' : 'R';
            CHECK(got == want[s][c], "selector %d, gv/gm/big %d%d%d: %c, table %c", s, (c >> 2) & 1, (c >> 1) & 1, c & 1, got, want[s][c]);
        }
    for (int64_t Lc : {16, 147, 160, 256, 257, 4000}) { // big: at least 16 periods and 4096 outputs
        CHECK(tile_big(true, Lc, 16 * Lc) == (16 * Lc >= 4096) && !tile_big(true, Lc, 16 * Lc - 1), "16 Lc, Lc=%ld", (long)Lc);
        CHECK(tile_big(true, Lc, 4096) == (4096 >= 16 * Lc) && !tile_big(true, Lc, 4095), "4096, Lc=%ld", (long)Lc);
        CHECK(!tile_big(false, Lc, 1 << 30), "no geometry");
    }
}

// ---- the thresholds of the small-job rules, each at its edge ----
static void check_thresholds()
{
    // float64 planar slabs: 16 periods below 6 x 256 slabs of 32; the overrides
    CHECK(mfma64_pb(1535, 0) == 16 && mfma64_pb(1536, 0) == 32 && mfma64_pb(1, 32) == 32 && mfma64_pb(100000, 16) == 16, "mfma64_pb");
    CHECK(units_per_slab(4, 64, 10, false) == 20 && units_per_slab(4, 32, 10, true) == 10 && units_per_slab(8, 32, 10, false) == 10 && units_per_slab(8, 32, 10, true) == 20 &&
              units_per_slab(8, 16, 10, true) == 10, "units_per_slab");
    // general-period kernel: small up to 96 slabs of 64; mid below 4096 where 16-period layers are cheaper
    CHECK(v1_small(96, false) && !v1_small(97, false) && v1_small(5000, true), "v1_small");
    CHECK(!v1_mid(4096, 4096, 16384, 64, false) && !v1_mid(127, 127, 508, 64, true), "v1_mid off");
    CHECK(v1_mid(127, 127, 508, 64, false), "127 slabs: 0.04 + 0.276 x 2 < 0.82");   // (tools/slab16_ab.sh: 127 slabs 45 -> 33 us)
    CHECK(!v1_mid(250, 250, 1000, 64, false), "250 slabs stay: 0.04 + 0.276 x 4 > 1"); // (250 and 500 stay)
    CHECK(v1_mid(300, 300, 1200, 64, false) && !v1_mid(500, 500, 2000, 64, false), "300 go, 500 stay");
    CHECK(v1_mid(127, 127, 254, 32, false) && !v1_mid(200, 200, 400, 32, false), "a 32-period plan: 0.53 per layer");
    // planar unit split: none from 512 workgroups on; else up to ceil(units / 4), as many as 2 x 3 x 256 workgroups allow
    CHECK(planar_split(20, 512, 0, 0) == 1 && planar_split(20, 511, 0, 0) == 3 && planar_split(20, 282, 0, 0) == 5 && planar_split(20, 400, 0, 0) == 3 && planar_split(20, 1, 0, 0) == 5,
          "planar_split");
    CHECK(planar_split(20, 100, 4, 0) == 4 && planar_split(20, 100, 4, 2) == 2 && planar_split(20, 100000, 0, 0) == 1, "planar_split overrides");
    // row-tile split: below 128 workgroups, as many parts as fill 256
    TileSwitches sw;
    CHECK(row_tile_split(128, 10, sw) == 1 && row_tile_split(127, 10, sw) == 2 && row_tile_split(4, 10, sw) == 10 && row_tile_split(40, 10, sw) == 6 && row_tile_split(4, 1, sw) == 1, "row_tile_split");
    sw.no_tile_split = true;
    CHECK(row_tile_split(4, 10, sw) == 1, "no_tile_split");
    const RowSplit r = row_split(40, 2);
    CHECK(r.per_wg == 16 && r.block == 1024 && r.z == 3, "row_split(40, 2): %d per workgroup, block %d, z %d", r.per_wg, r.block, r.z);
    const RowSplit r2 = row_split(10, 6);
    CHECK(r2.per_wg == 2 && r2.block == 256 && r2.z == 5, "row_split(10, 6)");
    const HalvesForm h = halves_form(10, 10, 16, 1000 * 4, 4);
    CHECK(h.per_wg == 5 && h.n_waves == 10 && h.block == 640 && h.z == 2 && h.scratch_off == 1024 && h.lds_bytes == (1024 + 5 * 256) * 4, "halves_form(10)");
    const XcdGrid x = xcd_grid(282, 5, false), y = xcd_grid(282, 5, true), z = xcd_grid(282, 1, false);
    CHECK(x.x == 288 * 5 && x.z == 1 && x.xz == 5 && y.x == 282 && y.z == 5 && y.xz == 0 && z.x == 282 && z.z == 1 && z.xz == 0, "xcd_grid");
}

// ---- a ragged launch of n equal clips is the equal-length job's launch, where that takes none of the small-job forms ----
static void check_ragged(std::mt19937_64 &rng)
{
    int compared = 0;
    for (int trial = 0; trial < 200 * kNReal; ++trial) {
        const Real &r = kReal[trial % kNReal];
        const TileGeom g = geom_of(r);
        const size_t width = (size_t)r.width;
        const uint32_t clips = 1 + (uint32_t)(rng() % 200), ch = 1 + (uint32_t)(rng() % 2);
        const uint64_t cols = (uint64_t)clips * ch;
        const int64_t n = std::max<int64_t>(1, some_periods(rng, (int64_t)cols) * g.Lc - (int64_t)(rng() % (uint64_t)g.Lc));
        std::vector<int64_t> rows((size_t)clips * 4, 0);
        for (uint32_t c = 0; c < clips; ++c) rows[(size_t)c * 4 + 3] = n;
        TileSwitches sw;
        if (rng() % 4 == 0) sw.no_xcd_split = true;
        const TileForm e = tile_form(width, g, 0, n, cols, sw);
        const TileForm f = tile_form_ragged(width, g, cols, sw, [&](int32_t pb) { return ragged_grid_x(n, g.Lc, pb); },
                                            [&](int32_t pb) { return ragged_total_slabs(rows.data(), clips, ch, g.Lc, pb); });
        CHECK(ragged_total_slabs(rows.data(), clips, ch, g.Lc, 32) == tile_slabs(tile_periods(0, n, g.Lc), 32, (int64_t)cols), "slabs of equal clips");
        if (e.err || f.err) { CHECK(!e.err && !f.err, "refused: %s / %s", e.err ? e.err : "", f.err ? f.err : ""); continue; }
        check_form_walk(f, g, width, "ragged launch");
        if (e.halves || (g.variant != 2 && e.split > 1) || (g.variant == 1 && e.slab.pb != g.pb) || (g.variant == 2 && width == 8 && e.slab.pb != 32)) continue; // a small-job form
        ++compared;
        CHECK(f.kind == e.kind && f.slab.pb == e.slab.pb && f.slab.x_count == e.slab.x_count && f.slab.plane == e.slab.plane && f.split == e.split && f.n_waves == e.n_waves &&
                  f.n_rt == e.n_rt && f.xz == e.xz && f.nx == e.nx && f.grid[0] == e.grid[0] && f.grid[1] == e.grid[1] && f.grid[2] == e.grid[2] && f.block == e.block && f.lds == e.lds,
              "variant %d width %zu, %u clips of %ld: ragged pb=%d split=%d nw=%d grid %ux%ux%u lds %zu; equal-length pb=%d split=%d nw=%d grid %ux%ux%u lds %zu", g.variant, width, clips,
              (long)n, (int)f.slab.pb, f.split, f.n_waves, f.grid[0], f.grid[1], f.grid[2], f.lds, (int)e.slab.pb, e.split, e.n_waves, e.grid[0], e.grid[1], e.grid[2], e.lds);
    }
    CHECK(compared > 50 * kNReal, "only %d ragged launches compared", compared);
    // float32 general-period slabs are 64 periods, float64 ones 32 or 16: any other geometry has no ragged kernel
    TileGeom g = geom_of(kReal[0]);
    g.variant = 1; g.pb = 32;
    CHECK(tile_form_ragged(4, g, 1, TileSwitches(), [](int32_t) { return (int64_t)1; }, [](int32_t) { return (int64_t)1; }).err == kTileNoRaggedKernel, "float32 general-period slab of 32");
}

int main()
{
    std::mt19937_64 rng(20261019);
    check_blocks(rng);
    check_waves();
    check_planes_form(rng);
    check_forms(rng);
    check_lds();
    check_family();
    check_thresholds();
    check_ragged(rng);
    std::printf("tile_rules_check: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
