// The randomized Hadamard rotation of a row in registers or in LDS, shared by the binary quantizer's
// rotation sinks (bin.hip) and the scalar-u8 quantizer's rotated encoders (u8.hip): the transform, the two
// kernel frames around it (a wave per row, a workgroup per row) and their launcher.  The translation unit that includes
// it compiles with contraction off, and every add below is one f32 operation.
//
// One geometry describes every rotation here: `src_dim` values are read per source row, +0.0 from there on; the rotated
// row has `width` values (width % 64 == 0); B, a power of two that divides width, cuts the stages off after B / 2:
// width / B Hadamard transforms of size B side by side.  The padded encoding of 3.2g is src_dim <= width = B = P; the
// block encodings (3.2h, 3.1x) are src_dim = width = dim and B the largest power of two that divides dim.
//
// y = H (signs * x): the sign of y_i from a fixed hash of i, then the butterflies of stages s = 1, 2, 4, ... in that
// order - (a, b) = (y_j, y_{j+s}) -> (a + b, a - b).  A stage reads only the stage before it, so any split of the work
// gives the same bits; the ORDER of the stages is part of the definition (f32 addition is not associative).
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "common.hpp"

namespace qamd {
namespace rot {

constexpr int kRotThreads = 256;         // the workgroup of every rotation kernel
constexpr uint32_t kRotWaveMax = 2048;   // the widest row a wave holds in registers: 32 values per lane
constexpr uint64_t kRotMaxDim = 16384;   // a rotated row is at most 64 KiB of f32: the LDS the workgroup form asks for
constexpr uint64_t kRotBlockMin = 64;    // block-rotated rows (3.2h): dim is a multiple of it, so no block is smaller

// B of a block rotation: the largest power of two that divides dim (dim != 0)
inline uint64_t rot_block(uint64_t dim) { return dim & (~dim + 1); }

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

// Four adjacent values of a row from index i0 on: one 16-byte load where the host found src_dim % 4 == 0 and an aligned
// source (`vec`), else four guarded dword loads; +0.0 from src_dim on; then the signs and, the four being adjacent,
// stages 1 and 2.
__device__ __forceinline__ void load_chunk(const float *__restrict__ src, uint32_t i0, uint32_t src_dim, int vec, float (&y)[4]) {
    if (vec) {
        const float4 t = i0 < src_dim ? __builtin_bit_cast(float4, rot_ld_nt(reinterpret_cast<const uint4 *>(src + i0)))
                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        y[0] = t.x, y[1] = t.y, y[2] = t.z, y[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) y[e] = i0 + e < src_dim ? src[i0 + e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) y[e] = rot_signed(y[e], i0 + e);
    butterfly(y[0], y[1]);
    butterfly(y[2], y[3]);
    butterfly(y[0], y[2]);
    butterfly(y[1], y[3]);
}

// Rotation of one row of width <= 2048 values by a wave, the row in registers.  K = ceil(width / 256); lane l holds the
// 4-value chunk k * 64 + l in y[k], values (k * 64 + l) * 4 + e.  Stages 1 and 2 are load_chunk's; the lane stage M pairs
// values 4 M apart and runs while 4 M < B (M <= 8 always, B >= 64); the chunk stage s pairs chunks 64 s apart, values
// 256 s apart, and runs while 256 s < B.  A width that is no power of two has B <= 512 here (B = 1024 first at 3072), so
// of the chunk stages only s = 1 is left for it (width = 1536 = 3 x 512, K = 6: chunk k pairs with k + 1 for every even
// k).  The chunk stages 2 and 4 are reached by width = B = 1024 (K = 4) and 2048 (K = 8) alone, and only K = 4 and
// K = 8 hold them.
// width % 256 != 0: the lanes from width / 4 - 64 (K - 1) on of the last chunk hold +-0.0 and stay active for the DPP
// reads.  B divides width, so a pair lies in one B-aligned block, wholly below width or wholly at or above it: an idle
// lane never meets a live value (and B <= 128 there: no chunk stage).  B is wave-uniform: every test on it is a scalar
// branch.
template <int K>
__device__ __forceinline__ void rotate_blocks_wave(const float *src, uint32_t src_dim, uint32_t B, int vec, int lane,
                                                   float (&y)[K][4]) {
    static_assert(K >= 1 && K <= 8, "a lane holds at most 32 values");
#pragma unroll
    for (int k = 0; k < K; k++) load_chunk(src, (uint32_t)(k * 64 + lane) * 4, src_dim, vec, y[k]);
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
    if constexpr (K == 4 || K == 8) {
#pragma unroll
        for (int s = 2; s < K; s <<= 1) {
            if (256u * s < B) {  // B == width == 256 K
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

// Rotation of one row of 2048 < width <= 16384 values by a workgroup of kRotThreads, the row in `row` (4 width bytes of
// LDS): every thread loads 4-value chunks (stages 1 and 2 in registers) into the LDS row, the stages from 4 on run
// there - width / 2 pairs per stage over the threads, a barrier between stages; pair b is (j, j + s) with
// j = 2 s (b / s) + b % s, and 2 s <= B divides width, so j + s < width.  The row is complete, and visible to every
// thread, on return.
__device__ __forceinline__ void rotate_blocks_lds(const float *src, uint32_t src_dim, uint32_t width, uint32_t B, int vec,
                                                  float *row) {
    const uint32_t chunks = width / 4;
    for (uint32_t c = threadIdx.x; c < chunks; c += kRotThreads) {
        float y[4];
        load_chunk(src, c * 4, src_dim, vec, y);
        reinterpret_cast<float4 *>(row)[c] = make_float4(y[0], y[1], y[2], y[3]);
    }
    for (uint32_t s = 4; s < B; s <<= 1) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < width / 2; b += kRotThreads) {
            const uint32_t j = ((b & ~(s - 1)) << 1) | (b & (s - 1));
            float a = row[j], d = row[j + s];
            butterfly(a, d);
            row[j] = a, row[j + s] = d;
        }
    }
    __syncthreads();
}

// ---- the two kernel frames ----
// A frame holds the row loop, the rotation and the idle-lane rule; what happens to a finished row is its SINK's, a small
// trivially-copyable struct passed by value.  A sink derives from RotSink and defines
//     chunk(st, r, ch, lane, y, keep)   chunk `ch` (values 4 ch .. 4 ch + 3, in y) of row r; called for live chunks only,
//                                       by the lane (thread % 64) that holds it.  `keep` is a word of the frame's that
//                                       lasts until the row's epilogue: a register of the wave form, the chunk's own
//                                       first LDS word (already read) of the workgroup form
// and, where it needs them, a per-thread State (default-constructed before the first row), the row epilogues of the two
// forms and `finish`, called once after the thread's last row.
struct RotSink {
    struct State {};
    template <int K, class S> __device__ void row_wave(S &, uint64_t, int, const uint32_t (&)[K]) const {}
    template <class S> __device__ void row_lds(S &, uint64_t, uint32_t *) const {}
    template <class S> __device__ void finish(S &, uint64_t, int) const {}
};

// A wave per row and pass of a grid-stride loop, width <= kRotWaveMax, K = ceil(width / 256); all 64 lanes stay active
// through the rotation (the DPP moves read their neighbours).  Only the last chunk can hold idle lanes: the chunks before
// it go to the sink without a branch, so that its loads for them issue together (behind a branch each load waits for the
// one before it).  width / 4 is a multiple of 16, so the live/idle cut of the last chunk falls on whole 8-lane groups,
// which a sink may fold with DPP.  FULL (width == 256 K): no lane is idle and the last chunk goes without the branch too -
// a sink's loads for it that do not depend on the row can then leave the row loop with the others.  The launcher takes
// it for the one-block rows of 256, 512 and 1024 values; wider rows and rows of several blocks keep the branch, without
// which the two-bit sink of bin.hip loses a wave per SIMD to the registers of the hoisted loads (K = 3, 6, 8).  A wave
// that has no row returns before `finish`.
template <int K, bool FULL, class SINK>
__global__ __launch_bounds__(kRotThreads) void rot_wave_kernel(const float *__restrict__ data, uint64_t n_rows, uint32_t src_dim,
                                                              uint32_t width, uint32_t B, int vec, SINK sink) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kRotThreads + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kRotThreads) >> 6;
    if (wave >= n_rows) return;
    const uint32_t chunks = width / 4;
    typename SINK::State st;
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        float y[K][4];
        rotate_blocks_wave<K>(data + r * src_dim, src_dim, B, vec, lane, y);
        uint32_t kept[K] = {};
#pragma unroll
        for (int k = 0; k < K - 1; k++) sink.chunk(st, r, (uint32_t)(k * 64 + lane), lane, y[k], kept[k]);
        const uint32_t last = (uint32_t)((K - 1) * 64 + lane);
        if (FULL || last < chunks) sink.chunk(st, r, last, lane, y[K - 1], kept[K - 1]);
        sink.template row_wave<K>(st, r, lane, kept);
    }
    sink.finish(st, wave, lane);
}

// A workgroup per row and pass for kRotWaveMax < width <= kRotMaxDim, the row in 4 width bytes of dynamic LDS.  Thread t
// takes the chunks t, t + 256, ...: a wave 64 consecutive chunks at a time, the last pass cut along 8-lane groups as
// above.  A workgroup always has a row (the grid is at most n_rows).
template <class SINK>
__global__ __launch_bounds__(kRotThreads) void rot_lds_kernel(const float *__restrict__ data, uint64_t n_rows, uint32_t src_dim,
                                                             uint32_t width, uint32_t B, int vec, SINK sink) {
    extern __shared__ float rot_row[];
    const int lane = threadIdx.x & 63;
    const uint32_t chunks = width / 4;
    typename SINK::State st;
    for (uint64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        rotate_blocks_lds(data + r * src_dim, src_dim, width, B, vec, rot_row);
        for (uint32_t ch = threadIdx.x; ch < chunks; ch += kRotThreads) {
            const float4 t = reinterpret_cast<const float4 *>(rot_row)[ch];
            const float y[4] = {t.x, t.y, t.z, t.w};
            sink.chunk(st, r, ch, lane, y, reinterpret_cast<uint32_t *>(rot_row)[ch * 4]);
        }
        sink.row_lds(st, r, reinterpret_cast<uint32_t *>(rot_row));
        __syncthreads();  // the next row's chunks overwrite the LDS row
    }
    sink.finish(st, (uint64_t)blockIdx.x * (kRotThreads / 64) + (threadIdx.x >> 6), lane);
}

// `n` rows of `src_dim` floats from `src` (device memory) through `sink`: the wave form up to kRotWaveMax values of
// width, eight workgroups of four waves per CU at most, and the workgroup form above, as many workgroups per CU as
// 160 KiB of LDS hold rows.
template <class SINK>
void launch_rot(const SINK &sink, const float *src, uint64_t n, uint32_t src_dim, uint32_t width, uint32_t B, hipStream_t s) {
    static_assert(std::is_trivially_copyable<SINK>::value, "a sink is a kernel argument");
    const int vec = src_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const auto grid = [&](uint64_t per_block, uint32_t blocks_per_cu) {
        const uint64_t want = (n + per_block - 1) / per_block, cap = (uint64_t)device_info().cu_count * blocks_per_cu;
        return dim3((unsigned)(want < 1 ? 1 : want > cap ? cap : want));
    };
    if (width > kRotWaveMax) {
        hipLaunchKernelGGL(rot_lds_kernel<SINK>, grid(1, 160 * 1024 / (width * 4)), dim3(kRotThreads), width * 4, s, src, n,
                           src_dim, width, B, vec, sink);
        return;
    }
    const auto wave = [&](auto k) {
        constexpr int K = decltype(k)::value;
        auto kernel = rot_wave_kernel<K, false, SINK>;
        if constexpr (K == 1 || K == 2 || K == 4)
            if (width == B && width == 256u * K) kernel = rot_wave_kernel<K, true, SINK>;
        hipLaunchKernelGGL(kernel, grid(kRotThreads / 64, 8), dim3(kRotThreads), 0, s, src, n, src_dim, width, B, vec, sink);
    };
    switch ((width + 255) / 256) {
    case 1: wave(std::integral_constant<int, 1>()); break;
    case 2: wave(std::integral_constant<int, 2>()); break;
    case 3: wave(std::integral_constant<int, 3>()); break;
    case 4: wave(std::integral_constant<int, 4>()); break;
    case 5: wave(std::integral_constant<int, 5>()); break;
    case 6: wave(std::integral_constant<int, 6>()); break;
    case 7: wave(std::integral_constant<int, 7>()); break;
    default: wave(std::integral_constant<int, 8>()); break;
    }
}

}  // namespace rot
}  // namespace qamd
