// half.hip — float16 / bfloat16 device jobs that no fused kernel takes (DESIGN.md §5.2 "Half-precision samples"): small
// jobs, recipes below HQ, ratios outside the frequency-domain engine's schedule table, interpolated-phase plans, odd
// interleaved channel counts and strided columns, HIPSOXR_KERNEL_EXACT / _GATHER / _TILE*, job windows, and every job of
// hipsoxr_run_device_adjoint.  Such a job is
//     k_widen   caller's half tensor (any strides)  ->  a dense float32 temporary, exact
//     the float32 job of the same selector on the temporaries
//     k_narrow  dense float32 temporary  ->  caller's half tensor: ONE round-to-nearest-even conversion per output element,
//               exactly the job's output elements and nothing else
// so it is, bit for bit, the float32 job on the widened samples followed by one rounding — the contract the fused kernels
// of fft.hip keep too.  The temporaries are stream-ordered allocations (as clip_table_device's and the two-stage form's),
// packed in the caller's dimension order (half_rules.h half_pack): the float32 job sees the caller's layout class and
// chooses the kernel form the float32 job on such tensors chooses.  Ranges of clips — with one clip, of channels — keep
// the temporaries of a range within kHalfTmpLimit.
// The conversions are plain casts: (float)h widens exactly (subnormals included); (_Float16)v is v_cvt_f16_f32,
// (__bf16)v is v_cvt_pk_bf16_f32 on gfx950 — round to nearest even, NaN stays NaN, overflow gives +-inf.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "half_rules.h"

namespace hipsoxr {

// One copy pass: the dense float32 temporary on one side (walked linearly), the caller's tensor on the other.
struct HalfCopy {
    const void *src;
    void *dst;
    int64_t s[3];   // the caller's strides (elements), in the temporary's dimension order: innermost first
    int64_t n0, n1; // extents of the temporary's two inner dimensions
    int64_t elems;
};

template <typename H>
__global__ void __launch_bounds__(256) k_widen(HalfCopy a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.elems) return;
    const HalfIdx x = half_unpack(i, a.n0, a.n1);
    const H *src = (const H *)a.src;
    ((float *)a.dst)[i] = (float)src[x.c[0] * a.s[0] + x.c[1] * a.s[1] + x.c[2] * a.s[2]];
}

template <typename H>
__global__ void __launch_bounds__(256) k_narrow(HalfCopy a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.elems) return;
    const HalfIdx x = half_unpack(i, a.n0, a.n1);
    H *dst = (H *)a.dst;
    dst[x.c[0] * a.s[0] + x.c[1] * a.s[1] + x.c[2] * a.s[2]] = (H)((const float *)a.src)[i];
}

static HalfCopy half_copy(const HalfPack &pk, const int64_t extent[3], const int64_t stride[3])
{
    HalfCopy c;
    c.src = nullptr; c.dst = nullptr;
    for (int i = 0; i < 3; ++i) c.s[i] = stride[pk.order[i]];
    c.n0 = extent[pk.order[0]]; c.n1 = extent[pk.order[1]];
    c.elems = pk.elems;
    return c;
}

template <typename H>
static const char *half_range_run(Plan *p, const hipsoxr_job_t &j, hipStream_t st, bool adjoint)
{
    const int64_t in_ext[3] = {(int64_t)j.n_clips, j.in_frames, (int64_t)j.n_channels};
    const int64_t out_ext[3] = {(int64_t)j.n_clips, j.out_frames, (int64_t)j.n_channels};
    const int64_t in_str[3] = {j.in_clip_stride, j.in_frame_stride, j.in_chan_stride};
    const int64_t out_str[3] = {j.out_clip_stride, j.out_frame_stride, j.out_chan_stride};
    const HalfPack pi = half_pack(in_ext, in_str), po = half_pack(out_ext, out_str);
    if (pi.elems > ((int64_t)1 << 38) || po.elems > ((int64_t)1 << 38)) return "float16 / bfloat16 job: a single column is too long for the widening pass";
    void *tin = nullptr, *tout = nullptr;
    if (hipMallocAsync(&tin, (size_t)(pi.elems > 0 ? pi.elems : 1) * sizeof(float), st) != hipSuccess)
        return "float16 / bfloat16 job: no device memory for the float32 temporaries";
    if (hipMallocAsync(&tout, (size_t)po.elems * sizeof(float), st) != hipSuccess) {
        (void)hipFreeAsync(tin, st);
        return "float16 / bfloat16 job: no device memory for the float32 temporaries";
    }
    const char *err = nullptr;
    if (pi.elems > 0) {
        HalfCopy w = half_copy(pi, in_ext, in_str);
        w.src = j.in; w.dst = tin;
        hipLaunchKernelGGL(k_widen<H>, dim3((unsigned)((pi.elems + 255) / 256)), dim3(256), 0, st, w);
        if (hipGetLastError() != hipSuccess) err = "float16 / bfloat16 job: the widening pass did not launch";
    }
    if (!err) {
        hipsoxr_job_t f = j;
        f.elem = HIPSOXR_F32;
        f.in = tin; f.out = tout;
        f.in_clip_stride = pi.stride[0]; f.in_frame_stride = pi.stride[1]; f.in_chan_stride = pi.stride[2];
        f.out_clip_stride = po.stride[0]; f.out_frame_stride = po.stride[1]; f.out_chan_stride = po.stride[2];
        f.clip_counter = nullptr; f.dither = 0; // (ignored, as for float jobs)
        err = adjoint ? launch_adjoint(p, f, st) : launch_job(p, f, st);
    }
    if (!err) {
        HalfCopy n = half_copy(po, out_ext, out_str);
        n.src = tout; n.dst = j.out;
        hipLaunchKernelGGL(k_narrow<H>, dim3((unsigned)((po.elems + 255) / 256)), dim3(256), 0, st, n);
        if (hipGetLastError() != hipSuccess) err = "float16 / bfloat16 job: the narrowing pass did not launch";
    }
    (void)hipFreeAsync(tin, st);
    (void)hipFreeAsync(tout, st);
    return err;
}

const char *launch_half(Plan *p, const hipsoxr_job_t &j, void *stream, bool adjoint)
{
    if (!elem_is_half(j.elem)) return "internal: the widening pass serves float16 / bfloat16 jobs";
    if (j.clip_table) return "internal: the widening pass takes one clip of a table at a time";
    if (j.out_frames <= 0 || j.n_clips == 0 || j.n_channels == 0) return nullptr;
    const size_t es = elem_size(j.elem);
    const HalfCut cut = half_cut(j.n_clips, j.n_channels, j.in_frames, j.out_frames, kHalfTmpLimit);
    for (uint64_t r = 0; r < half_range_count(cut); ++r) {
        const HalfRange g = half_range(cut, j.n_clips, j.n_channels, r);
        hipsoxr_job_t part = j;
        part.n_clips = g.n_clips; part.n_channels = g.n_ch;
        part.in = (const char *)j.in + ((int64_t)g.clip0 * j.in_clip_stride + (int64_t)g.ch0 * j.in_chan_stride) * (int64_t)es;
        part.out = (char *)j.out + ((int64_t)g.clip0 * j.out_clip_stride + (int64_t)g.ch0 * j.out_chan_stride) * (int64_t)es;
        const char *e = j.elem == HIPSOXR_F16 ? half_range_run<_Float16>(p, part, (hipStream_t)stream, adjoint)
                                              : half_range_run<__bf16>(p, part, (hipStream_t)stream, adjoint);
        if (e) return e;
    }
    return nullptr;
}

} // namespace hipsoxr
