// pcm_out.h — the integer output stage shared by both engines (kernels.hip: store_out; fft.hip: the staging stores of
// HIPSOXR_KERNEL_FFT_PCM): TPDF dither keyed by (seed, channel, absolute output index), round half to even, saturate,
// and say whether the value saturated.  oracle.quantize() is the host restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace hipsoxr {

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
// TPDF dither in (-1, 1) LSB: pure function of (seed, channel, absolute output index).
__device__ __forceinline__ float dither_tpdf(uint32_t seed, uint32_t ch, int64_t k)
{
    uint64_t z = mix64((uint64_t)k * 0x9E3779B97F4A7C15ULL + (((uint64_t)ch << 32) | seed));
    int32_t u1 = (int32_t)(z & 0xFFFFFF), u2 = (int32_t)((z >> 24) & 0xFFFFFF);
    return (float)(u1 - u2) * (1.f / 16777216.f);
}

// engine value (LSB units) -> int16: dither (ch = the channel's index in the caller's WHOLE signal), rint, saturate
__device__ __forceinline__ int16_t pcm_quantize_i16(float a, bool dither, uint32_t seed, uint32_t ch, int64_t k, bool &clip)
{
    if (dither) a = a + dither_tpdf(seed, ch, k);
    float r = __builtin_rintf(a);
    clip = false;
    if (r > 32767.f) { r = 32767.f; clip = true; }
    else if (r < -32768.f) { r = -32768.f; clip = true; }
    return (int16_t)r;
}
// ... -> int32 (no dither: the float64 engine's error is far below an LSB)
__device__ __forceinline__ int32_t pcm_quantize_i32(double v, bool &clip)
{
    double r = __builtin_rint(v);
    clip = false;
    if (r > 2147483647.) { r = 2147483647.; clip = true; }
    else if (r < -2147483648.) { r = -2147483648.; clip = true; }
    return (int32_t)r;
}

} // namespace hipsoxr
