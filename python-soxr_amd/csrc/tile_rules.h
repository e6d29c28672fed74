// tile_rules.h — the rules of a tile launch on the exact engine (kernels.hip launch_typed, launch_tile, launch_ragged; the
// kernels k_tile, k_tile_mfma, k_tile_mfma_p, k_tile_mfma64_p of kernels_tile.h): which kernel family a job takes, how many
// periods, slabs and blocks an output range touches, the waves of a workgroup, the slab size and unit split of the planar
// kernels, the small and mid forms of the general-period kernel, the splits over grid.z and the XCD-aware ids — and
// TileForm, the result of all of them for one launch.  No HIP, no globals, no switches(): the few switch values a rule reads
// come in as TileSwitches, which kernels.hip fills in one place (tests/c/tile_rules_check.cpp checks the rules against slow
// statements and against the kernels' own walks).
//
// What the kernels rely on: every period floor(k0 / Lc) .. floor((k0 + n - 1) / Lc) lies in exactly one block x < n_blocks;
// a workgroup has at most 16 computing waves (1024 threads), and at least 256 threads where it stages a slab for part of
// its row tiles; the (n_waves, grid.z or xz, halves) it is given make the kernel's walk visit every row tile — or planar
// unit — of a slab exactly once; the LDS bytes hold the slab (and, in the halves form, the scratch behind it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace hipsoxr {

// Geometry of a plan's tile tables for one precision (kernels.hip build_tile_tables / build_mfma_planes).
struct TileGeom {
    int RT = 16, c = 1;
    int variant = 0; // 0: k_tile (coefficients on the scalar path), 1: k_tile_mfma, 2: k_tile_mfma_p / k_tile_mfma64_p (planes)
    bool aligned = false;
    int32_t n_rt = 0, I_h = 0, pad = 0, i_min = 0, x_count = 0;
    int32_t pb = 64; // periods per slab (k_tile: 32 or 16 when a 64-period slab does not fit LDS — float64, long periods)
    int64_t Lc = 0, Mc = 0;
    size_t lds_bytes = 0;
    int32_t rowR = 0, plane = 0; // variant 2 (k_tile_mfma_p)
    int32_t span = 0;            // variant 2: inputs one period's tiles reach over (i_max - i_min + 1): x_count = (pb - 1) Mc + span
    bool ok = false;
};

// The switches the rules read (device.h `Switches`, same names, same meaning): all zero in a product build.
struct TileSwitches {
    bool dbg_slab32 = false, dbg_slab64 = false, no_halves = false, no_xcd_split = false, no_tile_split = false, dbg_mfma64_split = false;
    int dbg_tile_form = 0, dbg_mfma64_pb = 0, dbg_nrt = 0, dbg_nw = 0, dbg_split = 0;
    size_t dbg_lds = 0;
};

constexpr int64_t kTileMaxGridX = 2147483647LL;
constexpr uint64_t kTileMaxCols = 65535;
constexpr const char *kTileUnavailable = "tile kernel unavailable for this plan";
constexpr const char *kTileTooManyCols = "too many (clip, channel) columns for one launch (max 65535)";
constexpr const char *kTileTooLong = "job too long for one launch";

// ---- family selection (launch_typed, launch_ragged) ------------------------------------------------------------------
// The selector as the rule sees it (the callers map hipsoxr_kernel_t: both read EXACT as AUTO; launch_typed FFT too).
enum TileSelector { kSelAuto, kSelGather, kSelTile, kSelTileValu, kSelTileMfma, kSelOther };
// kFamOther: a selector that names none of the three (launch_typed: k_gather's dispatcher; launch_ragged: not its job)
enum TileFamily { kFamGather, kFamTileMfma, kFamTileValu, kFamOther, kFamRefused };

// a tile kernel pays off once a job spans a few thousand outputs per column (`frames`: out_frames, or the longest clip of a table)
inline bool tile_big(bool g_ok, int64_t Lc, int64_t frames) { return g_ok && frames >= 16 * Lc && frames >= 4096; }

// gv_ok / gm_ok: the plan has a VALU-tile / an MFMA-tile geometry; big: tile_big of the MFMA geometry where there is one, else of
// the VALU one (launch_typed takes its stream-chunk exception out of it first).  kFamRefused: kTileUnavailable.
inline TileFamily tile_family(TileSelector sel, bool gv_ok, bool gm_ok, bool big)
{
    if (sel == kSelTileValu && !gv_ok) return kFamRefused;
    if (sel == kSelTileMfma && !gm_ok) return kFamRefused;
    if (sel == kSelTile) {
        if (!gv_ok && !gm_ok) return kFamRefused;
        sel = gm_ok ? kSelTileMfma : kSelTileValu;
    }
    if (sel == kSelAuto) sel = !big ? kSelGather : gm_ok ? kSelTileMfma : kSelTileValu;
    return sel == kSelTileMfma ? kFamTileMfma : sel == kSelTileValu ? kFamTileValu : sel == kSelGather ? kFamGather : kFamOther;
}

// ---- periods, slabs, blocks -------------------------------------------------------------------------------------------
// periods touched by outputs [k0, k0 + n): floor(k0 / Lc) .. floor((k0 + n - 1) / Lc)
inline int64_t tile_first_period(int64_t k0, int64_t Lc) { return k0 / Lc; }
inline int64_t tile_periods(int64_t k0, int64_t n, int64_t Lc) { return (k0 + n - 1) / Lc - k0 / Lc + 1; }
// slabs of pb periods that hold them, per column (= n_blocks, the grid's frame axis: block x holds periods
// first + x pb .. first + x pb + pb - 1) ...
inline int64_t tile_blocks(int64_t periods, int32_t pb) { return (periods + pb - 1) / pb; }
// ... and over all columns: what the cost models are fed
inline int64_t tile_slabs(int64_t periods, int32_t pb, int64_t cols) { return tile_blocks(periods, pb) * cols; }

// ---- waves per workgroup: one row tile per wave when n_rt <= 16, else the even split with most waves ------------------
inline int tile_waves(int n_rt)
{
    if (n_rt <= 16) return n_rt;
    int best = 16, best_waste = 1 << 30;
    for (int w = 16; w >= 8; --w) {
        const int rounds = (n_rt + w - 1) / w, waste = rounds * w - n_rt;
        if (waste < best_waste) { best_waste = waste; best = w; }
    }
    return best;
}

// ---- float32 planar kernel (k_tile_mfma_p): slab size and unit split by job size --------------------------------------
// A slab of 64 periods (41 KB of LDS, three workgroups per CU) has 2 n_rt units (row tile x 32 periods), one of 32 periods
// (20 KB, seven per CU) n_rt; either runs as ONE workgroup (four waves, the units dealt round-robin) or SPLIT over
// ceil(units / 4) workgroups of one unit per wave, each staging the slab for itself.  What a job of few slabs costs is decided
// by how many workgroups deep the CUs are stacked ("layers": the dispatcher fills 256 CUs evenly only in whole layers) times
// what one workgroup does serially, plus staging; the constants are fitted to tools/slab_ab.sh sweeps (10 .. 6016 slabs,
// 48k -> 44.1k VHQ, profiles/r03_ab_experiments.txt), in units of one unit's MFMA time:
//     cost = c0 + layers x (units per wave) x k;   (pb, one unit per wave): c0, k = 32: 1.15, 1.153 | 64: 1.25, 1.41
//                                                  (pb, several)          :         32: 2.35, 0.958 | 64: 3.32, 1.052
// e.g. 47 slabs (a 10 s clip): 64/split (235 workgroups, one layer); 20: 32/split (120 workgroups staging half as much);
// 376: 32/whole (752 workgroups, 3 layers of 3 units: 35 us where round 2's 64/4 took 51); from 512 slabs of 64 on the
// whole-slab form is the rule again (12 waves per CU stream coefficients for 20 units each).
// slabs64 / slabs32: the job's slabs of 64 / of 32 periods over all its columns — a ragged job feeds the slabs its table
// really holds (ragged_total_slabs), not longest clip x clips.
struct PlanesForm { int pb, split; };
inline double planes_cost(int pb, int split, int64_t slabs, int n_rt)
{
    const int units = (pb / 32) * n_rt;
    const int upw = (units + 4 * split - 1) / (4 * split);
    const double wgs_ = (double)(slabs * split);
    double layers = std::ceil(wgs_ / 256.);
    // (a partly filled last layer of multi-unit workgroups costs less than a full one: half-way;
    //  64-period slabs split into single units, three per CU: between 1.5 and 3 x 256 workgroups the
    //  dispatcher stacks them three deep on the CUs it has started on — refit after the round-3 kernels)
    if (upw > 1) layers = 0.5 * (layers + wgs_ / 256.);
    else if (pb == 64 && wgs_ > 384. && wgs_ <= 768.) layers = 3.;
    const double c0 = pb == 32 ? (upw == 1 ? 1.15 : 2.35) : (upw == 1 ? 1.25 : 3.32);
    const double k = pb == 32 ? (upw == 1 ? 1.153 : 0.958) : (upw == 1 ? 1.41 : 1.052);
    return c0 + layers * upw * k;
}
inline PlanesForm planes_form(int64_t slabs64, int64_t slabs32, int n_rt, bool dbg_slab32, int dbg_tile_form)
{
    PlanesForm f{64, 1};
    if (slabs64 < 2048 || dbg_slab32) {
        double best = 1e300;
        for (int pb = dbg_slab32 ? 32 : 64; pb >= 32; pb -= 32) {
            const int units = (pb / 32) * n_rt, full = (units + 3) / 4;
            for (int split : {1, full}) {
                const double cost = planes_cost(pb, split, pb == 64 ? slabs64 : slabs32, n_rt);
                if (cost < best) { best = cost; f.pb = pb; f.split = split; }
            }
        }
    }
    // HIPSOXR_DEBUG_TILE_FORM (debug builds): 1 = 64 periods whole, 2 = 64 split, 3 = 32 whole, 4 = 32 split — what
    // tests/test_gpu_launch_forms.py::test_chosen_form_is_near_the_best compares the rule above against.
    // (Round 4 also built a fifth form — 512 workgroups each WALKING an equal share of a column's units, slab after
    //  slab — on the theory that 282 slabs on 256 CUs lose a fifth to layer quantisation.  They do not any more: the
    //  split forms already give every SIMD its 6-7 units, all resident at once; walk 33.7 us vs 28.9 (32 split) on the
    //  60 s clip, never ahead at any of eight sizes — profiles/r04_ab_experiments.txt §6.  Removed.)
    if (dbg_tile_form >= 1 && dbg_tile_form <= 4) {
        f.pb = dbg_tile_form <= 2 ? 64 : 32;
        const int units = (f.pb / 32) * n_rt;
        f.split = (dbg_tile_form & 1) ? 1 : (units + 3) / 4;
    }
    return f;
}

// ---- LDS figures of a slab ---------------------------------------------------------------------------------------------
struct TileSlab { int32_t pb, x_count, plane; size_t lds_bytes; };
// the plan's own slab
inline TileSlab tile_slab_of(const TileGeom &g) { return TileSlab{g.pb, g.x_count, g.plane, g.lds_bytes}; }
// the planar geometry's figures re-derived for slabs of pb periods (same tables); width: sizeof(Real)
inline TileSlab planes_slab(const TileGeom &g, int32_t pb, size_t width)
{
    TileSlab s{pb, (pb - 1) * (int32_t)g.Mc + g.span, 0, 0};
    const int32_t rows_total = (s.x_count + (int32_t)g.Mc - 1) / (int32_t)g.Mc + 3;
    s.plane = (rows_total * g.rowR + 63) / 64 * 64;
    s.lds_bytes = ((size_t)s.plane * 4 + g.rowR) * width;
    return s;
}
// a 16-period slab of the general-period kernel (k_tile_mfma<.., 1>)
inline TileSlab general_slab16(const TileGeom &g, size_t width)
{
    TileSlab s{16, (15 * (int32_t)g.Mc + g.span + 3) / 4 * 4, g.plane, 0};
    s.lds_bytes = ((size_t)s.x_count + (size_t)g.pad * (s.x_count / g.Mc + 1) + 8) * width;
    return s;
}

// ---- float64 planar kernel (k_tile_mfma64_p): a job of few 32-period slabs runs on 16-period ones (<.., PB = 16>) — same
// tables, half the slab.  slabs32: the job's slabs of 32 periods over all its columns.
inline int mfma64_pb(int64_t slabs32, int dbg_mfma64_pb) { return (slabs32 < 6 * 256 || dbg_mfma64_pb == 16) && dbg_mfma64_pb != 32 ? 16 : 32; }
// Units of a planar slab, dealt round-robin to a workgroup's four waves (one per SIMD) — float32: row tile x half of 64
// periods; float64: row tile x all periods of the slab, or row tile x 16 periods (HIPSOXR_DEBUG_MFMA64_SPLIT, 32-period slabs)
inline int units_per_slab(size_t width, int32_t pb, int n_rt, bool dbg_mfma64_split)
{
    return width == 4 ? (pb / 32) * n_rt : (pb == 32 && dbg_mfma64_split) ? 2 * n_rt : n_rt;
}

// ---- float32 / float64 MFMA kernel in its general form (k_tile_mfma: input periods that are no multiple of 16, e.g.
// 44.1k -> 16k): a job of few 64-period slabs — a 96 000-frame stream chunk is four — runs on 16-period ones: four times as
// many workgroups, each staging a quarter and walking a chain a quarter as long (one wave does a row tile x ALL the slab's
// periods, and its ~880 k-steps cost the same whether they feed four MFMAs or one: the chain is bound by its per-step
// address arithmetic).  96 000-frame chunk, int16 44.1k -> 16k: kernel 53.6 -> 26.5 us, the stream call 108 -> 81 us.
// The small-job form (16-period slabs, half-chains on two waves) — up to 96 slabs of 64 periods: 8 x 96 workgroups of 10
// waves are what the chip holds at once (tools/slab16_ab.sh: 50 slabs 54 -> 33 us, 100 slabs 65 -> 63, 127 slabs 66 -> 76)
inline bool v1_small(int64_t slabs64, bool dbg_slab32) { return slabs64 <= 96 || dbg_slab32; }
// Beyond that: 16-period slabs WITHOUT the half-chain split where four times as many, four times shorter workgroups fill
// the chip's layers better than 64-period ones — a layer of 256 workgroups of the 16-period form costs 0.276 of a 64-period
// layer (not 0.25), a last 64-period layer that is at most half full 0.82 (tools/slab16_ab.sh: 127 slabs 45 -> 33 us,
// 300: 108 -> 77, 800: 213 -> 190; 250 and 500 stay).  (In layers of the plan's own slab size — 64 periods, or 32 where a
// float64 slab of 64 does not fit LDS, whose layer a 16-period one costs 0.53 of.)  slabs_own / slabs16: the job's slabs of
// the plan's own pb / of 16 periods over all its columns.
inline bool v1_mid(int64_t slabs64, int64_t slabs_own, int64_t slabs16, int32_t pb_own, bool no_halves)
{
    if (!(slabs64 < 4096) || no_halves) return false;
    const double s0 = (double)slabs_own;
    const double l0 = std::ceil(s0 / 256.), frac = s0 / 256. - (l0 - 1.);
    const double est0 = (l0 - 1.) + (frac <= 0.5 ? 0.82 : 1.0);
    const double est16 = 0.04 + (pb_own == 64 ? 0.276 : 0.53) * std::ceil((double)slabs16 / 256.);
    return est16 < est0;
}

// ---- splits ------------------------------------------------------------------------------------------------------------
// Planar kernels, few slabs (e.g. one 60 s mono clip = 282): spread each slab's units over up to ceil(units / 4) workgroups
// so that every CU gets an equal share (3 resident per CU).  (From two workgroups per CU on, splitting only adds staging:
// measured 80 vs 92 us on a 60 s stereo clip.)  wgs: slabs over all columns; f32_split: the float32 kernel's, chosen with
// its slab size (planes_form), 0: none.
inline int planar_split(int units, int64_t wgs, int f32_split, int dbg_split)
{
    int split = wgs >= 512 ? 1 : (int)std::min<int64_t>((units + 3) / 4, (2 * 3 * 256) / std::max<int64_t>(wgs, 1));
    if (f32_split) split = f32_split;
    if (dbg_split) split = dbg_split;
    return std::max(1, split);
}
// ... as XCD-aware 1-D ids instead of the z dimension (kernels_tile.h: id = 8 (chunk Z + z) + xcd <-> slab = 8 chunk + xcd):
// grid.x = ceil8(n_blocks) x split and xz = split, else grid.z = split and xz = 0
struct XcdGrid { int64_t x; int z; int32_t xz; };
inline XcdGrid xcd_grid(int64_t n_blocks, int split, bool no_xcd_split)
{
    const int64_t ids = (n_blocks + 7) / 8 * 8 * (int64_t)split;
    if (split > 1 && !no_xcd_split && ids < kTileMaxGridX) return XcdGrid{ids, 1, split};
    return XcdGrid{n_blocks, split, 0};
}
// k_tile / k_tile_mfma, few slabs (one column of a stream chunk: 96 000 frames at 44.1k -> 16k are 4 slabs on 256 CUs): the
// row tiles of a slab go to several workgroups of fewer computing waves, each staging the slab for itself — as many
// workgroups as fill the chip once: every one of them stages the whole slab.  Returns the parts wanted (1: none).
inline int row_tile_split(int64_t wgs, int n_rt, const TileSwitches &sw)
{
    int split = 1;
    if (wgs < 128 && n_rt > 1 && !sw.dbg_nw && !sw.no_tile_split) split = (int)std::min<int64_t>(n_rt, 256 / wgs);
    if (sw.dbg_split) split = std::min(sw.dbg_split, n_rt);
    return split;
}
// ... the workgroups of a slab split in `split` parts: row tiles (= computing waves) per workgroup — a block holds 16 waves —
// the block (at least four waves stage the slab) and grid.z
struct RowSplit { int per_wg, block, z; };
inline RowSplit row_split(int n_rt, int split)
{
    const int per_wg = std::min(16, (n_rt + split - 1) / split);
    return RowSplit{per_wg, std::max(256, 64 * per_wg), (n_rt + per_wg - 1) / per_wg};
}
// Small jobs on 16-period slabs of k_tile_mfma: a row tile's two half-chains on two waves (a.halves).  want: the row tiles a
// workgroup has (after a row-tile split: its per_wg; else n_rt); at most 8 per workgroup (two waves each), evenly.  The
// half-sums meet in LDS behind the slab: scratch_off (elements, 64-aligned), per_wg x (pb / 16) x 4 x 64 elements.
struct HalvesForm { int per_wg, n_waves, block, z; int32_t scratch_off; size_t lds_bytes; };
inline HalvesForm halves_form(int want, int n_rt, int32_t pb, size_t slab_bytes, size_t width)
{
    HalvesForm h;
    const int parts = (want + 7) / 8;
    h.per_wg = (want + parts - 1) / parts;
    h.n_waves = 2 * h.per_wg;
    h.block = std::max(256, 64 * h.n_waves);
    h.z = (n_rt + h.per_wg - 1) / h.per_wg;
    h.scratch_off = (int32_t)((slab_bytes / width + 63) / 64 * 64);
    h.lds_bytes = ((size_t)h.scratch_off + (size_t)h.per_wg * (pb / 16) * 4 * 64) * width;
    return h;
}

// ---- the launch form -----------------------------------------------------------------------------------------------------
enum TileKind { kTile, kTileMfma, kTileMfmaP, kTileMfma64P };
inline TileKind tile_kind(int variant, size_t width) { return variant == 0 ? kTile : variant == 1 ? kTileMfma : width == 4 ? kTileMfmaP : kTileMfma64P; }
inline const char *tile_kind_name(TileKind k) { return k == kTile ? "tile" : k == kTileMfma ? "tile_mfma" : k == kTileMfmaP ? "tile_mfma_p" : "tile_mfma64_p"; }

struct TileForm {
    const char *err = nullptr; // a refusal: nothing else is valid
    TileKind kind = kTile;
    TileSlab slab{};           // pb, x_count, plane and the slab's LDS bytes
    int ng = 2;                // k_tile_mfma64_p: groups of 16 periods per unit (1 on 16-period slabs and under dbg_mfma64_split)
    int n_rt = 0, n_waves = 0; // as the kernel is told them
    int split = 1;             // workgroups per slab: the planar unit split, or the row-tile parts on grid.z
    int halves = 0;
    int32_t scratch_off = 0, xz = 0, nx = 0;
    int64_t n_blocks = 0;
    unsigned grid[3] = {1, 1, 1}, block = 0;
    size_t lds = 0;
};

// An equal-length job: outputs [k0, k0 + n) of `cols` (clip, channel) columns on geometry g; width: sizeof(Real).
// (HIPSOXR_DEBUG_* are timing experiments only; results may be wrong when they are set)
inline TileForm tile_form(size_t width, const TileGeom &g, int64_t k0, int64_t n, uint64_t cols, const TileSwitches &sw)
{
    TileForm f;
    f.kind = tile_kind(g.variant, width);
    f.slab = tile_slab_of(g);
    const int64_t periods = tile_periods(k0, n, g.Lc), icols = (int64_t)cols;
    int f32_split = 0;
    bool small = false;
    if (f.kind == kTileMfma64P) {
        if (mfma64_pb(tile_slabs(periods, 32, icols), sw.dbg_mfma64_pb) == 16) f.slab = planes_slab(g, 16, width);
        f.ng = f.slab.pb == 16 || sw.dbg_mfma64_split ? 1 : 2;
    } else if (f.kind == kTileMfmaP && !sw.dbg_slab64) {
        const PlanesForm pf = planes_form(tile_slabs(periods, 64, icols), tile_slabs(periods, 32, icols), g.n_rt, sw.dbg_slab32, sw.dbg_tile_form);
        f32_split = pf.split;
        if (pf.pb == 32) f.slab = planes_slab(g, 32, width);
    } else if (f.kind == kTileMfma && g.pb > 16 && !sw.dbg_slab64) { // (float64 too: k_tile_mfma<IO, double, 1>)
        const int64_t s64 = tile_slabs(periods, 64, icols);
        small = v1_small(s64, sw.dbg_slab32);
        if (small || v1_mid(s64, tile_slabs(periods, g.pb, icols), tile_slabs(periods, 16, icols), g.pb, sw.no_halves)) f.slab = general_slab16(g, width);
    }
    f.n_blocks = tile_blocks(periods, f.slab.pb);
    if (cols > kTileMaxCols) { f.err = kTileTooManyCols; return f; }
    if (f.n_blocks > kTileMaxGridX) { f.err = kTileTooLong; return f; }
    const bool planar = g.variant == 2;
    f.n_rt = g.n_rt;
    f.n_waves = planar ? 4 : tile_waves(g.n_rt); // (planar: one wave per SIMD, the slab's units dealt round-robin)
    if (sw.dbg_nrt) f.n_rt = f.n_waves = sw.dbg_nrt;
    if (sw.dbg_nw) f.n_waves = sw.dbg_nw;
    f.nx = (int32_t)f.n_blocks;
    f.grid[0] = (unsigned)f.n_blocks; f.grid[1] = (unsigned)cols;
    f.block = 64u * (unsigned)f.n_waves;
    f.lds = f.slab.lds_bytes;
    const int64_t wgs = f.n_blocks * icols;
    if (planar) {
        f.split = planar_split(units_per_slab(width, f.slab.pb, g.n_rt, sw.dbg_mfma64_split), wgs, f32_split, sw.dbg_split);
        const XcdGrid x = xcd_grid(f.n_blocks, f.split, sw.no_xcd_split);
        f.grid[0] = (unsigned)x.x; f.grid[2] = (unsigned)x.z; f.xz = x.xz;
    } else {
        const int parts = row_tile_split(wgs, g.n_rt, sw);
        if (parts > 1) {
            const RowSplit r = row_split(g.n_rt, parts);
            f.n_waves = r.per_wg; f.block = (unsigned)r.block; f.split = r.z;
        }
        if (f.kind == kTileMfma && small && !sw.dbg_nw && !sw.dbg_nrt && !sw.no_halves) {
            const HalvesForm h = halves_form(f.split > 1 ? f.n_waves : g.n_rt, g.n_rt, f.slab.pb, f.slab.lds_bytes, width);
            f.n_waves = h.n_waves; f.halves = 1; f.block = (unsigned)h.block; f.split = h.z;
            f.scratch_off = h.scratch_off; f.lds = h.lds_bytes;
        }
        f.grid[2] = (unsigned)f.split;
    }
    f.lds = std::max(f.lds, sw.dbg_lds); // occupancy experiments
    return f;
}

// A ragged launch: the clips of a table on the plan's own slab geometry — not in ragged form: the small-job forms (halves,
// row-tile splits, 16-period float64 slabs).  The table's two figures come from ragged_rules.h: grid_x(pb), the slabs of pb
// periods of its longest clip (ragged_grid_x: the grid's frame axis — tile_blocks of a whole signal of that length), and
// total_slabs(pb), the slabs it really holds over its columns (ragged_total_slabs) — what the planar cost models are fed.
constexpr const char *kTileNoRaggedKernel = "internal: tile geometry without a ragged kernel";
template <typename GridX, typename Slabs>
inline TileForm tile_form_ragged(size_t width, const TileGeom &g, uint64_t cols, const TileSwitches &sw, GridX grid_x, Slabs total_slabs)
{
    TileForm f;
    f.kind = tile_kind(g.variant, width);
    f.slab = tile_slab_of(g);
    f.n_rt = g.n_rt;
    f.n_waves = g.variant == 2 ? 4 : tile_waves(g.n_rt);
    if (f.kind == kTileMfmaP) { // slab size and unit split by the slabs the table holds
        const PlanesForm pf = planes_form(total_slabs(64), total_slabs(32), g.n_rt, sw.dbg_slab32, sw.dbg_tile_form);
        if (pf.pb == 32) f.slab = planes_slab(g, 32, width);
        f.split = std::max(1, pf.split);
    } else if (f.kind == kTileMfma64P) { // 32-period slabs, a row tile per unit
        f.split = planar_split(units_per_slab(width, g.pb, g.n_rt, false), total_slabs(g.pb), 0, 0);
    } else if (f.kind == kTileMfma && (width == 4 ? g.pb != 64 : (g.pb != 32 && g.pb != 16))) { // (float32 slabs are 64 periods: build_tile_tables)
        f.err = kTileNoRaggedKernel;
        return f;
    }
    f.n_blocks = grid_x(f.slab.pb);
    if (f.n_blocks > kTileMaxGridX) { f.err = kTileTooLong; return f; }
    f.nx = (int32_t)f.n_blocks;
    const XcdGrid x = g.variant == 2 ? xcd_grid(f.n_blocks, f.split, sw.no_xcd_split) : XcdGrid{f.n_blocks, 1, 0};
    f.grid[0] = (unsigned)x.x; f.grid[1] = (unsigned)cols; f.grid[2] = (unsigned)x.z; f.xz = x.xz;
    f.block = 64u * (unsigned)f.n_waves;
    f.lds = f.slab.lds_bytes;
    return f;
}

} // namespace hipsoxr
