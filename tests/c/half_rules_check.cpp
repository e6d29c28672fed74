// half_rules_check.cpp — the rules of a float16 / bfloat16 device job (python-soxr_amd/csrc/half_rules.h) against slow,
// independent statements of them: the temporaries' strides address every element exactly once, in the caller's dimension
// order; the copy kernels' index walk inverts them; the ranges cover every (clip, channel) once and stay within the byte
// limit unless they are one column; the fused decision agrees with its restatement.  No device, no other source file.
// Exit status 0 = every check held (tests/test_half_rules.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "half_rules.h"

using namespace hipsoxr;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                  \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

// ---- half_pack / half_unpack ------------------------------------------------------------------------------------------
// the caller's strides of a dense tensor whose dimensions are nested in `perm` (innermost first), times `gap` (a view
// that steps over elements: same order, not dense)
static void dense_strides(const int64_t ext[3], const int perm[3], int64_t gap, int64_t out[3])
{
    int64_t run = gap;
    for (int i = 0; i < 3; ++i) { out[perm[i]] = run; run *= ext[perm[i]]; }
}

static void check_pack()
{
    const int perms[6][3] = {{2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {0, 1, 2}};
    const int64_t sizes[] = {1, 2, 3, 5, 8};
    for (const auto &perm : perms)
        for (int64_t nc : sizes)
            for (int64_t nf : sizes)
                for (int64_t nh : sizes)
                    for (int64_t gap : {(int64_t)1, (int64_t)2, (int64_t)7}) {
                        const int64_t ext[3] = {nc, nf, nh};
                        int64_t cs[3];
                        dense_strides(ext, perm, gap, cs);
                        for (int d = 0; d < 3; ++d)
                            if (ext[d] == 1) cs[d] = (int64_t)(rnd() % 1000); // (an extent-1 dimension's stride means nothing)
                        const HalfPack p = half_pack(ext, cs);
                        CHECK(p.elems == nc * nf * nh, "elems %ld", (long)p.elems);
                        // every element exactly once inside [0, elems)
                        std::vector<int> hit((size_t)p.elems, 0);
                        bool in_range = true;
                        for (int64_t c = 0; c < nc; ++c)
                            for (int64_t f = 0; f < nf; ++f)
                                for (int64_t h = 0; h < nh; ++h) {
                                    const int64_t at = c * p.stride[0] + f * p.stride[1] + h * p.stride[2];
                                    if (at < 0 || at >= p.elems) { in_range = false; continue; }
                                    ++hit[(size_t)at];
                                }
                        bool once = in_range;
                        for (int v : hit) once = once && v == 1;
                        CHECK(once, "strides (%ld %ld %ld) of extents (%ld %ld %ld) do not address each element once", (long)p.stride[0],
                              (long)p.stride[1], (long)p.stride[2], (long)nc, (long)nf, (long)nh);
                        // the caller's order: of two real dimensions the one with the smaller caller stride has the smaller stride here
                        for (int a = 0; a < 3; ++a)
                            for (int b = 0; b < 3; ++b)
                                if (ext[a] > 1 && ext[b] > 1 && cs[a] < cs[b])
                                    CHECK(p.stride[a] < p.stride[b], "order: dims %d %d caller %ld %ld packed %ld %ld", a, b, (long)cs[a], (long)cs[b],
                                          (long)p.stride[a], (long)p.stride[b]);
                        // extent-1 dimensions: what a contiguous [clips, frames, channels] tensor has
                        if (nh == 1) CHECK(p.stride[2] == 1, "channel stride %ld", (long)p.stride[2]);
                        if (nf == 1) CHECK(p.stride[1] == 1, "frame stride %ld", (long)p.stride[1]);
                        if (nc == 1) CHECK(p.stride[0] == p.elems, "clip stride %ld", (long)p.stride[0]);
                        // the kernels' walk: index i -> coordinates along order[0..2] -> i again
                        for (int64_t i = 0; i < p.elems; ++i) {
                            const HalfIdx x = half_unpack(i, ext[p.order[0]], ext[p.order[1]]);
                            int64_t at = 0;
                            bool ok = true;
                            for (int k = 0; k < 3; ++k) {
                                ok = ok && x.c[k] >= 0 && x.c[k] < ext[p.order[k]];
                                at += x.c[k] * p.stride[p.order[k]];
                            }
                            CHECK(ok && at == i, "unpack %ld -> %ld", (long)i, (long)at);
                        }
                    }
    // the common layouts by name: mono, interleaved, planar
    {
        const int64_t ext[3] = {1, 100, 1}, cs[3] = {100, 1, 1};
        const HalfPack p = half_pack(ext, cs);
        CHECK(p.stride[0] == 100 && p.stride[1] == 1 && p.stride[2] == 1, "mono");
    }
    {
        const int64_t ext[3] = {4, 100, 2}, cs[3] = {200, 2, 1};
        const HalfPack p = half_pack(ext, cs);
        CHECK(p.stride[0] == 200 && p.stride[1] == 2 && p.stride[2] == 1, "interleaved");
    }
    {
        const int64_t ext[3] = {4, 100, 2}, cs[3] = {200, 1, 100};
        const HalfPack p = half_pack(ext, cs);
        CHECK(p.stride[0] == 200 && p.stride[1] == 1 && p.stride[2] == 100, "planar");
    }
    {
        const int64_t ext[3] = {3, 100, 2}, cs[3] = {1000, 4, 2}; // a view that steps over elements: packed as interleaved
        const HalfPack p = half_pack(ext, cs);
        CHECK(p.stride[0] == 200 && p.stride[1] == 2 && p.stride[2] == 1, "strided view");
    }
}

// ---- ranges -----------------------------------------------------------------------------------------------------------
static void check_ranges()
{
    const uint32_t clips[] = {1, 2, 3, 7, 64};
    const uint32_t chans[] = {1, 2, 3, 8};
    const int64_t frames[][2] = {{0, 1}, {10, 9}, {1000, 919}, {48000, 44100}};
    const uint64_t limits[] = {1, 64, 4096, 100000, 1000000, (uint64_t)1 << 30};
    for (uint32_t nc : clips)
        for (uint32_t nh : chans)
            for (const auto &fr : frames)
                for (uint64_t limit : limits) {
                    const HalfCut cut = half_cut(nc, nh, fr[0], fr[1], limit);
                    const uint64_t n = half_range_count(cut);
                    CHECK(n >= 1, "no range");
                    std::vector<int> hit((size_t)nc * nh, 0);
                    const uint64_t per_col = (uint64_t)(fr[0] + fr[1]) * 4;
                    for (uint64_t r = 0; r < n; ++r) {
                        const HalfRange g = half_range(cut, nc, nh, r);
                        CHECK(g.n_clips >= 1 && g.n_ch >= 1 && g.clip0 + g.n_clips <= nc && g.ch0 + g.n_ch <= nh, "range %lu out of the job", (unsigned long)r);
                        for (uint32_t c = g.clip0; c < g.clip0 + g.n_clips && c < nc; ++c)
                            for (uint32_t h = g.ch0; h < g.ch0 + g.n_ch && h < nh; ++h) ++hit[(size_t)c * nh + h];
                        const uint64_t bytes = half_range_bytes(g, fr[0], fr[1]);
                        CHECK(bytes == (uint64_t)g.n_clips * g.n_ch * per_col, "bytes");
                        // within the limit, unless the range is one single column (never cut)
                        CHECK(bytes <= limit || (g.n_clips == 1 && g.n_ch == 1), "range of %u clips x %u channels: %lu bytes above %lu", g.n_clips, g.n_ch,
                              (unsigned long)bytes, (unsigned long)limit);
                        // channels are cut only where one clip alone is above the limit
                        if (g.n_ch < nh) CHECK(per_col * nh > limit && g.n_clips == 1, "channels cut needlessly");
                    }
                    bool once = true;
                    for (int v : hit) once = once && v == 1;
                    CHECK(once, "ranges do not cover every (clip, channel) once: %u x %u limit %lu", nc, nh, (unsigned long)limit);
                    CHECK(half_range(cut, nc, nh, n).n_clips == 0, "a range past the last");
                    if (per_col * nh * nc <= limit) CHECK(n == 1, "a job within the limit is one range");
                }
    const HalfCut none = half_cut(0, 2, 10, 10, 100);
    CHECK(half_range_count(none) == 0, "no clips: no range");
}

// ---- fused or not -------------------------------------------------------------------------------------------------------
static void check_fused()
{
    for (int sel = 0; sel < 3; ++sel)
        for (int64_t total : {(int64_t)0, (int64_t)1, (int64_t)8191, (int64_t)8192, (int64_t)8193, (int64_t)1 << 30})
            for (int no_fft = 0; no_fft < 2; ++no_fft)
                for (int eligible = 0; eligible < 2; ++eligible)
                    for (uint64_t cols : {(uint64_t)1, (uint64_t)65535, (uint64_t)65536}) {
                        // restated: by name always; AUTO from 8192 output samples unless the engine is switched off; never
                        // for the canonical-order selectors; only eligible jobs whose columns fit grid.y
                        bool want = false;
                        if (sel == kHalfSelFft) want = true;
                        if (sel == kHalfSelAuto && !no_fft && total > 8191) want = true;
                        const bool expect = want && eligible && cols < 65536;
                        CHECK(half_wants_fft((HalfSelector)sel, total, no_fft != 0) == want, "wants sel=%d total=%ld", sel, (long)total);
                        CHECK(half_try_fused((HalfSelector)sel, total, no_fft != 0, eligible != 0, cols) == expect, "try sel=%d total=%ld no_fft=%d el=%d cols=%lu",
                              sel, (long)total, no_fft, eligible, (unsigned long)cols);
                    }
    for (int row = 0; row < 2; ++row)
        for (int v2 = 0; v2 < 2; ++v2)
            for (int cp = 0; cp < 2; ++cp)
                for (int tab = 0; tab < 2; ++tab) {
                    HalfForm expect = kHalfNone;
                    if (row && cp && !tab) expect = kHalfChanPair;
                    if (row && v2) expect = kHalfPair2; // (unit-stride columns first; a table: those alone)
                    CHECK(half_fused_form(row != 0, v2 != 0, cp != 0, tab != 0) == expect, "form row=%d v2=%d cp=%d table=%d", row, v2, cp, tab);
                }
}

int main()
{
    check_pack();
    check_ranges();
    check_fused();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
