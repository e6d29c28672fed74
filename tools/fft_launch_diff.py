#!/usr/bin/env python3
"""Host-only differential check of the launch layer of csrc/fft.hip after launch_fft_impl was split by form
(profiles/NOTES_fft_launch_refactor.md §2): the text of the function as it stood before the split is pasted beside the
new functions into three stand-alone programs, compiled with hipcc's host pass and run on the CPU — no device.

    git show a359e85:python-soxr_amd/csrc/fft.hip > /tmp/fft_old.hip
    python tools/fft_launch_diff.py /tmp/fft_old.hip [python-soxr_amd/csrc/fft.hip] [--keep DIR]

1. geometry: fft_geometry / fft_hop_out / fft_lead_periods old against new (fft_kept_run), the table layout (fft_tabs)
   against the old pointer chain and element counts, fill_twiddles against the old loops bit for bit;
2. layout: the old inline lines from n_blocks to st2ok against fft_layout on random jobs;
3. FftArgs: the old paired fill and the old k_fft_block fill against fft_args.
The old blocks are found by their first and last statements, so OLD must be the file of commit a359e85 (or one whose
launch_fft_impl still has that text).  Not covered: row choice, one-round rule, form order (they need a device)."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")


def func(s, sig):
    """The definition that starts with `sig`, up to its closing brace."""
    a = s.index(sig)
    i = s.index("{", a)
    d = 0
    while True:
        d += {"{": 1, "}": -1}.get(s[i], 0)
        if d == 0:
            return s[a:i + 1]
        i += 1


HEAD = """#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "device.h"
#define FFT_NO_PK
#include "fft_dev.h"
using namespace hipsoxr;
"""


def geometry_program(old, new):
    geom = func(old, "struct FftGeom {") + ";\n" + func(old, "static bool factor_radices")
    o = "\n".join([func(old, "static int32_t fft_lead_periods"), func(old, "static bool fft_geometry"), func(old, "static int64_t fft_hop_out")])
    n = "\n".join([func(new, "struct FftTabs {") + ";", func(new, "static FftTabs fft_tabs"), func(new, "struct KeptRun {") + ";", func(new, "static bool fft_kept_run"),
                   func(new, "static int64_t fft_hop_out"), func(new, "static bool fft_geometry"), "template <typename C>", func(new, "static void fill_twiddles")])
    return HEAD + geom + "\nnamespace O {\n" + o + "\n}\nnamespace N {\n" + n + "\n}\n" + MAIN_GEOMETRY


def layout_program(old, new):
    n = "\n".join([func(old, "struct FftGeom {") + ";", func(new, "static bool fft_offsets_fit"), func(new, "struct FftJobView {") + ";", func(new, "static FftJobView fft_job_view"),
                   func(new, "struct FftLayout {") + ";", func(new, "static const char *fft_layout")])
    first = old.index("const int64_t n_blocks = (span + g.hop_out - 1) / g.hop_out;")
    blk = old[old.rindex("\n", 0, first) + 1:old.index("\n", old.index("< (1LL << 30);", old.index("const bool st2ok")))]
    blk = (blk.replace("switches()", "sw").replace("return nullptr;", 'return "NONE";').replace("a.chpair", "chpair").replace("a.xcd_map", "xcd_map")
           .replace("a.pairs_per_col = items;", ""))
    return HEAD + n + OLD_LAYOUT_HEAD + blk + OLD_LAYOUT_TAIL + MAIN_LAYOUT


def args_program(old, new):
    n = "\n".join([func(old, "struct FftGeom {") + ";", func(new, "struct FftTabs {") + ";", func(new, "static FftTabs fft_tabs"), func(new, "struct FftJobView {") + ";",
                   func(new, "static FftJobView fft_job_view"), func(new, "static void fft_args_geom"), func(new, "static FftArgs fft_args(")])
    first = old.index("FftArgs a;")
    paired = old[old.rindex("\n", 0, first) + 1:old.index("\n", old.index("a.clip_counter = pcm ?", first))]
    paired = "\n".join(l for l in paired.split("\n") if "internal: the job window" not in l)
    second = old.index("FftArgs a;", first + 1)
    block = old[old.rindex("\n", 0, second) + 1:old.index("\n", old.index("a.in_lo = j.in_abs0; a.in_frames", second))]
    return HEAD + n + OLD_ARGS_HEAD + paired + OLD_ARGS_MID + block + "\n    return a;\n}\n" + MAIN_ARGS


OLD_LAYOUT_HEAD = """
struct OldOut { int chpair = 0, xcd_map = 0; int64_t n_blocks = 0, items = 0, units = 0; dim3 grid; bool v2ok = false, cp2ok = false, st2ok = false; size_t lds1 = 0; };
static const char *old_layout(const Plan *p, const hipsoxr_job_t &j, const FftGeom &g, const Switches &sw, bool window, OldOut *o)
{
    const int64_t P0 = window ? j.out_k0 / p->L : 0, out_lo = window ? j.out_k0 - P0 * p->L : 0;
    const int64_t span = out_lo + j.out_frames;
    const uint64_t cols_p = (uint64_t)j.n_clips * j.n_channels;
    const bool io64 = j.elem == HIPSOXR_F64, wide32 = !io64 && j.kernel == HIPSOXR_KERNEL_FFT_F64;
    const bool pcm = j.elem == HIPSOXR_I16 || j.elem == HIPSOXR_I32, pcm32 = j.elem == HIPSOXR_I32;
    const bool f64 = io64 || wide32 || pcm32;
    int chpair = 0, xcd_map = 0;
    *o = OldOut();
"""
OLD_LAYOUT_TAIL = """
    o->chpair = chpair; o->xcd_map = xcd_map; o->n_blocks = n_blocks; o->items = items; o->units = units; o->grid = grid;
    o->v2ok = v2ok; o->cp2ok = cp2ok; o->st2ok = st2ok; o->lds1 = lds1;
    return nullptr;
}
"""
OLD_ARGS_HEAD = """
static FftArgs old_paired(const Plan *p, const hipsoxr_job_t &j, const FftGeom &g, uint32_t ch0, bool window)
{
    const int64_t P0 = window ? j.out_k0 / p->L : 0, out_lo = window ? j.out_k0 - P0 * p->L : 0;
    const int64_t span = out_lo + j.out_frames;
    const bool pcm = j.elem == HIPSOXR_I16 || j.elem == HIPSOXR_I32;
"""
OLD_ARGS_MID = """
    a.chpair = 0; a.xcd_map = 0; a.pairs_per_col = 0;   // (set from the layout afterwards, in both)
    return a;
}
static FftArgs old_block(const Plan *p, const hipsoxr_job_t &j, const FftGeom &g)
{
"""
MAIN_GEOMETRY = r"""int main()
{
    long bad = 0, n = 0, ok_geoms = 0;
    const long LM[][2] = {{147,160},{160,147},{160,441},{441,160},{1,2},{2,1},{1,3},{3,1},{2,3},{3,2},{1,4},{4,1},{1,6},{6,1},{320,441},{441,320},{80,147},{147,80},{147,320},{320,147},{80,441},{441,80},{147,640},{640,147},{640,441},{441,640},{40,147},{147,40},{4,3},{3,4},{5,6},{6,5},{7,9},{25,24},{11,13}};
    const int ks[] = {0, 8, 10, 14, 16, 20, 24, 32, 896, 1024, 1280, 1792, 2048, 3, 5000};
    for (auto &lm : LM) for (int T = 16; T <= 2000; T += 4) for (int k : ks) for (int small = 0; small < 2; ++small) {
        static Plan &p = *new Plan; p.L = lm[0]; p.M = lm[1]; p.T = T; p.q.bits = 20.;
        FftGeom a, b;
        const bool ra = O::fft_geometry(p, a, small, k), rb = N::fft_geometry(p, b, small, k);
        ++n;
        if (ra != rb) { ++bad; continue; }
        if (k && O::fft_hop_out(p, k) != N::fft_hop_out(p, k)) ++bad;
        if (!ra) continue;
        ++ok_geoms;
        if (a.k != b.k || a.N_in != b.N_in || a.N_out != b.N_out || a.A != b.A || a.B != b.B || a.nA != b.nA || a.nB != b.nB || memcmp(a.radA, b.radA, 32) || memcmp(a.radB, b.radB, 32) ||
            a.lead_periods != b.lead_periods || a.hop_periods != b.hop_periods || a.v0 != b.v0 || a.hop_out != b.hop_out || a.lds_bytes != b.lds_bytes) ++bad;
        if (a.lead_periods != O::fft_lead_periods(p)) ++bad;
        // the table layout against the old pointer chain and element counts
        const N::FftTabs t = N::fft_tabs(b);
        const size_t A = a.A, B = a.B;
        const size_t WB = A, P = WB + B, Q = P + (A + 1), Hs = Q + B, WA2 = Hs + (B + 1), WB2 = WA2 + a.N_in, Hr = WB2 + a.N_out;
        const size_t total = (size_t)A + B + (A + 1) + B + (B + 1) + a.N_in + a.N_out + (B + 2) / 2 + 1, totald = (size_t)a.N_in + a.N_out + (B + 2) / 2 + 1;
        if (t.WA != 0 || t.WB != WB || t.P != P || t.Q != Q || t.Hs != Hs || t.WA2 != WA2 || t.WB2 != WB2 || t.Hr != Hr || t.n != total ||
            t.WA2d != 0 || t.WB2d != (size_t)a.N_in || t.Hrd != (size_t)a.N_in + a.N_out || t.nd != totald) ++bad;
    }
    // twiddles, bit for bit, against the old loops
    const double PI2 = 6.283185307179586476925286766559;
    for (int N_ : {2560, 2352, 5120, 4704, 7056, 1280, 1176, 2058, 2240, 3200, 2940, 4096, 1792, 5376, 3, 640}) for (int sign : {-1, +1}) {
        std::vector<float2> f(N_ + 1), g(N_ + 1); std::vector<double2> d(N_), e(N_);
        for (int half = 0; half < 2; ++half) { // count = N (W tables) and count = N/2 + 1 over N (P / Q tables)
            const int cnt = half ? N_ / 2 + 1 : N_;
            for (int m = 0; m < cnt; ++m) g[m] = sign < 0 ? make_float2((float)std::cos(PI2 * m / N_), (float)-std::sin(PI2 * m / N_)) : make_float2((float)std::cos(PI2 * m / N_), (float)std::sin(PI2 * m / N_));
            N::fill_twiddles(f.data(), cnt, N_, sign);
            if (memcmp(f.data(), g.data(), cnt * sizeof(float2))) ++bad;
        }
        for (int m = 0; m < N_; ++m) e[m] = sign < 0 ? make_double2(std::cos(PI2 * m / N_), -std::sin(PI2 * m / N_)) : make_double2(std::cos(PI2 * m / N_), std::sin(PI2 * m / N_));
        N::fill_twiddles(d.data(), N_, N_, sign);
        if (memcmp(d.data(), e.data(), N_ * sizeof(double2))) ++bad;
    }
    printf("%ld geometry cases (%ld admissible), %ld mismatches\n", n, ok_geoms, bad);
    return bad != 0;
}
"""
MAIN_LAYOUT = r"""int main()
{
    std::mt19937_64 r(7);
    auto pick = [&](std::initializer_list<int64_t> v) { return *(v.begin() + r() % v.size()); };
    long bad = 0, n = 0, none = 0, errs = 0, forms[3] = {0, 0, 0};
    static Plan &p = *new Plan;
    for (long it = 0; it < 3000000; ++it) {
        p.L = pick({147, 160, 1, 2, 441, 640}); p.M = 160;
        FftGeom g; g.N_in = (int32_t)pick({1280, 2560, 5120, 7056, 2058, 3200, 4096, 896}); g.N_out = (int32_t)pick({1176, 2352, 4704, 2560, 2240, 2940, 2048, 5376});
        g.hop_out = (int32_t)pick({882, 2058, 4410, 1764, 2940, 1600, 100000, 3000});
        hipsoxr_job_t j; memset(&j, 0, sizeof j);
        j.elem = (int)pick({HIPSOXR_F32, HIPSOXR_F32, HIPSOXR_F64, HIPSOXR_I16, HIPSOXR_I32});
        j.kernel = (hipsoxr_kernel_t)pick({HIPSOXR_KERNEL_FFT, HIPSOXR_KERNEL_AUTO, HIPSOXR_KERNEL_FFT_F64, HIPSOXR_KERNEL_FFT_PCM});
        j.n_clips = (uint32_t)pick({1, 1, 2, 3, 65535, 65536, 100000}); j.n_channels = (uint32_t)pick({1, 1, 2, 3, 4, 5, 8, 1000, 65535});
        j.in_frame_stride = pick({1, 1, (int64_t)j.n_channels, (int64_t)j.n_channels, 4, 7, 100000, 3000000}); j.out_frame_stride = pick({1, j.in_frame_stride, j.in_frame_stride, (int64_t)j.n_channels, 2});
        j.in_chan_stride = pick({1, 1, 12345}); j.out_chan_stride = pick({1, 1, j.in_chan_stride, 777});
        j.in_clip_stride = pick({0, 1000, 1001}); j.out_clip_stride = pick({0, 900, 901});
        j.in = (const void *)(uintptr_t)pick({4096, 4098, 4097}); j.out = (void *)(uintptr_t)pick({8192, 8194});
        j.out_frames = pick({1, 1765, 5000, 100000, 1LL << 33, 1LL << 45, 300000000000000LL}); j.out_k0 = pick({0, 0, 146, 147, 1000003});
        Switches sw; sw.fft_no_chpair = r() % 8 == 0; sw.fft_no_xcd_map = r() % 8 == 0; sw.dbg_fft_lds = r() % 8 == 0 ? 200000 : 0;
        const bool window = r() % 4 == 0;
        if (!window) j.out_k0 = 0;
        OldOut o; FftLayout y;
        const char *eo = old_layout(&p, j, g, sw, window, &o);
        const FftJobView v = fft_job_view(p, j, window);
        const char *en = fft_layout(j, v, g, sw, &y);
        ++n;
        const bool new_none = !en && !y.v2ok && !y.cp2ok && !y.st2ok;
        if (eo && !strcmp(eo, "NONE")) {                 // the parent's two silent returns: f64 LDS, or no form
            ++none; if (!new_none) ++bad;
            continue;
        }
        if (eo || en) { ++errs; if (!eo || !en || strcmp(eo, en)) ++bad; continue; }
        // the parent went on to the wave attempt / launch with these values
        if (!o.v2ok && !o.cp2ok && !o.st2ok) { ++none; if (!new_none) ++bad; }
        if (o.chpair != y.chpair || o.xcd_map != y.xcd_map || o.n_blocks != y.n_blocks || o.items != y.items || o.units != y.units || o.grid.x != y.grid.x || o.grid.y != y.grid.y ||
            o.grid.z != y.grid.z || o.v2ok != y.v2ok || o.cp2ok != y.cp2ok || o.st2ok != y.st2ok || o.lds1 != y.lds) ++bad;
        forms[0] += y.v2ok; forms[1] += y.cp2ok; forms[2] += y.st2ok;
    }
    printf("%ld layouts: %ld no form, %ld errors, v2ok %ld cp2ok %ld st2ok %ld; %ld mismatches\n", n, none, errs, forms[0], forms[1], forms[2], bad);
    return bad != 0;
}
"""
MAIN_ARGS = r"""#define CMP(m) if (memcmp(&x.m, &y.m, sizeof x.m)) { ++bad; if (bad < 5) printf("differs: %s\n", #m); }
int main()
{
    std::mt19937_64 r(11);
    auto pick = [&](std::initializer_list<int64_t> v) { return *(v.begin() + r() % v.size()); };
    long bad = 0, n = 0;
    static Plan &p = *new Plan;
    static float2 dev[1]; static double2 devd[1];
    for (long it = 0; it < 1000000; ++it) {
        p.L = pick({147, 160, 1, 2, 441}); p.M = pick({160, 147, 2, 1, 640});
        FftGeom g; g.N_in = (int32_t)pick({1280, 2560, 5120, 2058}); g.N_out = (int32_t)pick({1176, 2352, 4704, 2240}); g.A = g.N_in / 2; g.B = g.N_out / 2;
        g.nA = 3; g.nB = 4; for (int i = 0; i < 8; ++i) { g.radA[i] = (int32_t)(r() % 16 + 1); g.radB[i] = (int32_t)(r() % 16 + 1); }
        g.lead_periods = (int32_t)(r() % 9); g.hop_periods = (int32_t)(r() % 30 + 1); g.v0 = (int32_t)(r() % 3000); g.hop_out = (int32_t)pick({882, 2058, 4410});
        g.dev = dev; g.devd = devd; g.twa = r() % 2 ? 0 : 12345; g.twb = g.twa ? 23456 : 0;
        hipsoxr_job_t j; memset(&j, 0, sizeof j);
        j.elem = (int)pick({HIPSOXR_F32, HIPSOXR_F64, HIPSOXR_I16, HIPSOXR_I32});
        j.kernel = (hipsoxr_kernel_t)pick({HIPSOXR_KERNEL_FFT, HIPSOXR_KERNEL_FFT_F64, HIPSOXR_KERNEL_FFT_PCM});
        j.n_clips = (uint32_t)(r() % 5 + 1); j.n_channels = (uint32_t)(r() % 5 + 1);
        j.in_frame_stride = pick({1, 2, 3, 7}); j.out_frame_stride = pick({1, 2, 3, 5}); j.in_chan_stride = pick({1, 999}); j.out_chan_stride = pick({1, 888});
        j.in_clip_stride = (int64_t)(r() % 100000); j.out_clip_stride = (int64_t)(r() % 100000);
        j.in = (const void *)(uintptr_t)(1 << 20); j.out = (void *)(uintptr_t)(1 << 22);
        j.in_abs0 = pick({0, 0, -40, 20, 100000}); j.in_frames = (int64_t)(r() % 1000000); j.out_frames = (int64_t)(r() % 1000000 + 1); j.out_k0 = (int64_t)(r() % 10000000);
        j.clip_table_dev = r() % 2 ? nullptr : (const int64_t *)(uintptr_t)4096; j.clip_counter = (uint64_t *)(uintptr_t)8192; j.dither = (uint32_t)(r() % 2); j.dither_seed = (uint32_t)r();
        const bool window = r() % 2; const uint32_t ch0 = (uint32_t)(r() % 7);
        if (!window) j.out_k0 = 0;
        ++n;
        { // the paired forms (and the wave form, which starts from the same fill): every member
            FftArgs x = old_paired(&p, j, g, ch0, window), y = fft_args(p, j, fft_job_view(p, j, window), g, ch0);
            CMP(in) CMP(out) CMP(WA) CMP(WB) CMP(P) CMP(Q) CMP(Hs) CMP(WA2) CMP(WB2) CMP(Hr) CMP(WA2d) CMP(WB2d) CMP(Hrd) CMP(trace) CMP(A) CMP(B) CMP(nA) CMP(nB) CMP(radA) CMP(radB)
            CMP(L) CMP(M) CMP(lead_periods) CMP(hop_periods) CMP(v0) CMP(hop_out) CMP(n_clips) CMP(n_channels) CMP(ics) CMP(ifs) CMP(ichs) CMP(ocs) CMP(ofs) CMP(ochs)
            CMP(in_frames) CMP(out_frames) CMP(in_lo) CMP(clip_tab) CMP(chpair) CMP(pairs_per_col) CMP(xcd_map) CMP(clip_counter) CMP(dither) CMP(seed) CMP(ch0) CMP(out_lo) CMP(out_abs0) CMP(TWA) CMP(TWB)
        }
        if (j.elem == HIPSOXR_F32 && !window && !j.clip_table_dev) { // k_fft_block's jobs: the members it reads, and those that keep their zeros
            FftArgs x = old_block(&p, j, g), y = fft_args(p, j, fft_job_view(p, j, false), g, 0);
            y.nA = g.nA; y.nB = g.nB; for (int i = 0; i < 8; ++i) { y.radA[i] = g.radA[i]; y.radB[i] = g.radB[i]; }
            CMP(in) CMP(out) CMP(WA) CMP(WB) CMP(P) CMP(Q) CMP(Hs) CMP(WA2) CMP(WB2) CMP(Hr) CMP(trace) CMP(A) CMP(B) CMP(nA) CMP(nB) CMP(radA) CMP(radB)
            CMP(L) CMP(M) CMP(lead_periods) CMP(hop_periods) CMP(v0) CMP(hop_out) CMP(n_clips) CMP(n_channels) CMP(ics) CMP(ifs) CMP(ichs) CMP(ocs) CMP(ofs) CMP(ochs)
            CMP(in_frames) CMP(out_frames) CMP(in_lo) CMP(clip_tab) CMP(chpair) CMP(pairs_per_col) CMP(xcd_map) CMP(clip_counter) CMP(ch0) CMP(out_lo) CMP(out_abs0)
        }
    }
    printf("%ld argument fills, %ld mismatches\n", n, bad);
    return bad != 0;
}
"""


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        raise SystemExit(__doc__)
    old = open(args[0]).read()
    new = open(args[1] if len(args) > 1 else os.path.join(CSRC, "fft.hip")).read()
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    work = keep or tempfile.mkdtemp(prefix="fft_launch_diff_")
    os.makedirs(work, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    bad = 0
    for name, text in (("geometry", geometry_program(old, new)), ("layout", layout_program(old, new)), ("args", args_program(old, new))):
        src, exe = os.path.join(work, name + ".cpp"), os.path.join(work, name)
        with open(src, "w") as f:
            f.write(text)
        # (build.sh's FFT flags: contraction as in the product, so that the twiddle comparison is the product's arithmetic)
        subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=fast", "-fno-slp-vectorize",
                               "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
        bad += subprocess.call([exe]) != 0
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
