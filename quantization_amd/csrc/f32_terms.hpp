// What the exact-score kernels of the original vectors share (f32.hip: id lists; f32_scan.hip: the whole store): one
// term of DistanceType::distance (quantization/src/encoded_vectors.rs:37-45) and the exact widening of 16-bit rows.
#pragma once

#include "common.hpp"

namespace qamd {

template <int METRIC> __device__ __forceinline__ float term(float q, float v) {
    if (METRIC == QAMD_DOT) return q * v;
    const float d = q - v;
    return METRIC == QAMD_L1 ? __builtin_fabsf(d) : d * d;
}

// The two 16-bit values of a packed dword, widened exactly to f32.
template <int DTYPE> __device__ __forceinline__ float widen_lo(uint32_t w) {
    if (DTYPE == QAMD_DTYPE_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu));
    return __uint_as_float(w << 16);
}
template <int DTYPE> __device__ __forceinline__ float widen_hi(uint32_t w) {
    if (DTYPE == QAMD_DTYPE_F16) return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
    return __uint_as_float(w & 0xFFFF0000u);
}

// f32 -> f16 / bf16: round to nearest even, overflow to +-inf, NaN stays NaN, subnormal results kept.
template <int DTYPE> __device__ __forceinline__ uint32_t narrow(float x) {
    if (DTYPE == QAMD_DTYPE_F16) return __builtin_bit_cast(uint16_t, (_Float16)x);  // v_cvt_f16_f32 in the default mode
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;  // a NaN whose payload sits in the low bits stays one
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                    // the carry out of the mantissa is the overflow to inf
}

}  // namespace qamd
