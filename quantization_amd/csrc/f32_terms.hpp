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

}  // namespace qamd
