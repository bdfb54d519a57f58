// The randomized Hadamard rotation of a row in registers or in LDS, shared by the binary quantizer's
// rotation kernels (bin.hip) and the scalar-u8 quantizer's rotated encoders (u8.hip).  Device code only; the
// translation unit that includes it compiles with contraction off, and every add below is one f32 operation.
//
// y = H (signs * x): the sign of y_i from a fixed hash of i, then the butterflies of stages s = 1, 2, 4, ... in that
// order - (a, b) = (y_j, y_{j+s}) -> (a + b, a - b).  A stage reads only the stage before it, so any split of the work
// gives the same bits; the ORDER of the stages is part of the definition (f32 addition is not associative).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace qamd {
namespace rot {

constexpr int kRotThreads = 256;         // the workgroup of every rotation kernel
constexpr uint32_t kRotWaveMax = 2048;   // the widest row a wave holds in registers: 32 values per lane
constexpr uint64_t kRotMaxDim = 16384;   // a rotated row is at most 64 KiB of f32: the LDS the workgroup form asks for
constexpr uint64_t kRotBlockMin = 64;    // block-rotated rows (3.2h): dim is a multiple of it, so no block is smaller

__device__ __forceinline__ float rot_signed(float v, uint32_t i) {
    uint32_t h = i * 0x9E3779B1u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) ^ (h << 31));
}

// The value lane (l ^ M) holds.  Inside a DPP row of 16 lanes a DPP move: quad_perm for 1 and 2, row_ror:8 for 8, and for
// 4 the two rotations by 12 and 4 (lane i reads lane (i + 4) % 16 and (i - 4) % 16), of which a lane keeps the one its
// bit 2 asks for.  Across rows __shfl_xor (ds_bpermute).
template <int M> __device__ __forceinline__ float lane_xor(float v, int lane) {
    const int x = __builtin_bit_cast(int, v);
    int r;
    if constexpr (M == 1) {
        r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);
    } else if constexpr (M == 2) {
        r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);
    } else if constexpr (M == 4) {
        const int up = __builtin_amdgcn_update_dpp(0, x, 0x12C, 0xF, 0xF, false);
        const int dn = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, false);
        r = (lane & 4) ? dn : up;
    } else if constexpr (M == 8) {
        r = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false);
    } else {
        r = __shfl_xor(x, M);
    }
    return __builtin_bit_cast(float, r);
}
// One stage whose pairs sit M lanes apart: the lower lane keeps a + b, the upper a - b = a + (-b).
template <int M> __device__ __forceinline__ float lane_butterfly(float v, int lane) {
    const float p = lane_xor<M>(v, lane);
    return p + ((lane & M) ? -v : v);
}
__device__ __forceinline__ void butterfly(float &a, float &b) {
    const float s = a + b, d = a - b;
    a = s, b = d;
}

// A streamed-once 16-byte load: `global_load_dwordx4 ... nt`.
typedef uint32_t rot_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 rot_ld_nt(const uint4 *p) {
    rot_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const rot_u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

// Four adjacent values of a row from index i0 on: one 16-byte load where the host found dim % 4 == 0 and an aligned
// source (`vec`), else four guarded dword loads; +0.0 from dim on; then the signs and, the four being adjacent, stages 1
// and 2.
__device__ __forceinline__ void load_chunk(const float *__restrict__ src, uint32_t i0, uint32_t dim, int vec, float (&y)[4]) {
    if (vec) {
        const float4 t = i0 < dim ? __builtin_bit_cast(float4, rot_ld_nt(reinterpret_cast<const uint4 *>(src + i0)))
                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) y[e] = i0 + e < dim ? src[i0 + e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) y[e] = rot_signed(y[e], i0 + e);
    butterfly(y[0], y[1]);
    butterfly(y[2], y[3]);
    butterfly(y[0], y[2]);
    butterfly(y[1], y[3]);
}

// Block rotation of one row of dim <= 2048 values (dim % 64 == 0) by a wave, the row in registers: B = the largest power
// of two that divides dim, dim / B Hadamard transforms of size B side by side.  K = ceil(dim / 256); lane l holds the
// 4-value chunk k * 64 + l in y[k], values (k * 64 + l) * 4 + e.  Stages 1 and 2 are load_chunk's; the lane stage M pairs
// values 4 M apart and runs while 4 M < B (M <= 8 always, B >= 64); the chunk stage s pairs chunks 64 s apart, values
// 256 s apart, and runs while 256 s < B.  A dim that is no power of two has B <= 512 here (B = 1024 first at 3072), so
// of the chunk stages only s = 1 is left for it (dim = 1536 = 3 x 512, K = 6: chunk k pairs with k + 1 for every even
// k).  POW2 adds the chunk stages 2 and 4, which only dim = B = 1024 (K = 4) and 2048 (K = 8) reach; a caller that sends
// those dims elsewhere (bin.hip) leaves it off and pays no registers for them.
// dim % 256 != 0: the lanes from dim / 4 - 64 (K - 1) on of the last chunk hold +-0.0 and stay active for the DPP reads.
// B divides dim, so a pair lies in one B-aligned block, wholly below dim or wholly at or above it: an idle lane never
// meets a live value (and B <= 128 there: no chunk stage).  B is wave-uniform: every test on it is a scalar branch.
template <int K, bool POW2 = false>
__device__ __forceinline__ void rotate_blocks_wave(const float *src, uint32_t dim, uint32_t B, int vec, int lane,
                                                   float (&y)[K][4]) {
    static_assert(K >= 1 && K <= 8, "a lane holds at most 32 values");
#pragma unroll
    for (int k = 0; k < K; k++) load_chunk(src, (uint32_t)(k * 64 + lane) * 4, dim, vec, y[k]);
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float v = y[k][e];
            v = lane_butterfly<1>(v, lane);
            v = lane_butterfly<2>(v, lane);
            v = lane_butterfly<4>(v, lane);
            v = lane_butterfly<8>(v, lane);
            y[k][e] = v;
        }
    }
    // (one branch per stage, not per value: the 4 K ds_bpermute of a stage stay in one block and overlap)
    if (64u < B) {
#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int e = 0; e < 4; e++) y[k][e] = lane_butterfly<16>(y[k][e], lane);
        }
    }
    if (128u < B) {
#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int e = 0; e < 4; e++) y[k][e] = lane_butterfly<32>(y[k][e], lane);
        }
    }
    if (256u < B) {
#pragma unroll
        for (int k = 0; k + 1 < K; k += 2) {
#pragma unroll
            for (int e = 0; e < 4; e++) butterfly(y[k][e], y[k + 1][e]);
        }
    }
    if constexpr (POW2) {
#pragma unroll
        for (int s = 2; s < K; s <<= 1) {
            if (256u * s < B) {  // B == dim == 256 K
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if ((k & s) || k + s >= K) continue;
#pragma unroll
                    for (int e = 0; e < 4; e++) butterfly(y[k][e], y[k + s][e]);
                }
            }
        }
    }
}

// Block rotation of one row of 2048 < dim <= 16384 values (dim % 64 == 0) by a workgroup of kRotThreads, the row in
// `row` (4 dim bytes of LDS): every thread loads 4-value chunks (stages 1 and 2 in registers) into the LDS row, the
// stages from 4 on run there - dim / 2 pairs per stage over the threads, a barrier between stages; pair b is (j, j + s)
// with j = 2 s (b / s) + b % s, and 2 s <= B divides dim, so j + s < dim.  The row is complete, and visible to every
// thread, on return.
__device__ __forceinline__ void rotate_blocks_lds(const float *src, uint32_t dim, uint32_t B, int vec, float *row) {
    const uint32_t chunks = dim / 4;
    for (uint32_t c = threadIdx.x; c < chunks; c += kRotThreads) {
        float y[4];
        load_chunk(src, c * 4, dim, vec, y);
        reinterpret_cast<float4 *>(row)[c] = make_float4(y[0], y[1], y[2], y[3]);
    }
    for (uint32_t s = 4; s < B; s <<= 1) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < dim / 2; b += kRotThreads) {
            const uint32_t j = ((b & ~(s - 1)) << 1) | (b & (s - 1));
            float a = row[j], d = row[j + s];
            butterfly(a, d);
            row[j] = a, row[j + s] = d;
        }
    }
    __syncthreads();
}

}  // namespace rot
}  // namespace qamd
