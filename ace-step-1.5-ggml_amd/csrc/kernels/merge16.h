// The 16-bit <-> f32 conversions of the adapter merge kernels (lora.hip, lokr.hip): bf16 / fp16 words of a weight
// image widened exactly, and f32 results rounded to nearest even (a NaN stays a quiet NaN).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace acemi {

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 64u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint16_t f32_to_16(bool f16, float f) {
    if (f16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    return f32_to_bf16_rne(f);
}
__device__ __forceinline__ float f16_to_f32(bool f16, uint16_t v) {
    if (f16) return (float)__builtin_bit_cast(_Float16, v);
    return __uint_as_float((uint32_t)v << 16);
}

}  // namespace acemi
