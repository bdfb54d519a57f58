// Scalar u8 quantizer on MI355X (gfx950), the WRITE side: everything that builds or changes a store.  Pass 1 (min / max,
// the quantile interval), pass 2 (the quantize kernels, plain or behind the block rotation of a rotated store), the scan
// image (pack, unpack), from_rows / export / save / load, the streaming encoder and upsert.  What READS a store (query
// encode, scans, top-k, pairs) is u8.hip; the handles, the code formats and the launchers both need are in u8_internal.hpp.
//
// Host class mirrors EncodedVectorsU8 (quantization/src/encoded_vectors_u8.rs: encode :34-118, save / load :263-288) and
// quantile.rs.  The device layout the builders fill - codes[padded_rows][actual_dim], offsets[padded_rows], the blocked
// scan image - is described in u8.hip and u8_internal.hpp.  This file is compiled with contraction off: the encoders
// evaluate in the reference's operation order, one rounding per operation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "lists.hpp"
#include "topk.hpp"
#include "rotate_blocks.hpp"
#include "u8_internal.hpp"

#pragma clang fp contract(off)

using namespace qamd;
using namespace qamd::rot;

namespace {

constexpr uint64_t kQuantileSample = 100000;  // QUANTILE_SAMPLE_SIZE, quantile.rs:3

// ------------------------------------------------------------------------------ device helpers
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Streamed-once 16-byte loads: `global_load_dwordx4 ... nt`.
__device__ __forceinline__ float4 ld_nt(const float4 *p) {
    f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}

// The code of a 4-bit store: f32_to_nearest (u8_internal.hpp) with 15 for the largest code.
__device__ __forceinline__ uint32_t f32_to_u4(float v, float alpha, float offset) { return f32_to_nearest(v, alpha, offset, 15.0f); }

// f32_to_u8 for four values without the division, for all but ~6 values in 100 000.
// x = RN((v - offset) / alpha) and y = RN((v - offset) * RN(1 / alpha)) differ by at most
// |x| * (2^-23 + 2^-24) < 2.3e-5 for |x| <= 128 (three roundings of relative size 2^-24), so whenever y
// lies further than 2^-15 = 3.05e-5 from every integer -- or anywhere outside (-2^-15, 128 + 2^-15),
// where the clamp decides -- trunc(clamp(x)) == trunc(clamp(y)).  If any of the four values is inside
// one of those bands (or NaN: both tests fail), all four take the reference's division: ONE branch per
// float4, taken by 1.5 % of the waves.  The host selects this path only for a normal alpha in
// 2^-60 .. 2^60 (1 / alpha exact to half an ulp, no overflow).  Codes are the reference's, bit for bit
// (tests/test_gpu_u8.py: boundary sweep).  Returns the four codes packed into a dword.
__device__ __forceinline__ bool quant_decided(float y) {
    constexpr float kBand = 3.0517578125e-05f;  // 2^-15
    const float fr = __builtin_amdgcn_fractf(y);
    return (__builtin_fabsf(fr - 0.5f) <= 0.5f - kBand) || (__builtin_fabsf(y - 64.0f) >= 64.0f + kBand);
}
__device__ __forceinline__ uint32_t quant_code(float y) {  // y is not NaN here
    return (uint32_t)__builtin_amdgcn_fmed3f(y, 0.0f, 127.0f);
}
__device__ __forceinline__ uint32_t f32x4_to_u8x4_fast(const float4 &f, float alpha, float offset, float r_alpha) {
    const float y0 = (f.x - offset) * r_alpha, y1 = (f.y - offset) * r_alpha, y2 = (f.z - offset) * r_alpha,
                y3 = (f.w - offset) * r_alpha;
    if (quant_decided(y0) && quant_decided(y1) && quant_decided(y2) && quant_decided(y3))
        return quant_code(y0) | (quant_code(y1) << 8) | (quant_code(y2) << 16) | (quant_code(y3) << 24);
    return f32_to_u8(f.x, alpha, offset) | (f32_to_u8(f.y, alpha, offset) << 8) | (f32_to_u8(f.z, alpha, offset) << 16) |
           (f32_to_u8(f.w, alpha, offset) << 24);
}

// ------------------------------------------------------------------------------ encode kernels
// Pass 1: global min / max (quantile.rs:5-19).  `value < min` / `value > max` ignore NaN,
// as fminf/fmaxf do.  Per-block partials; the host folds them.
//
// The sign of a zero extreme: `value < min` keeps the FIRST of several equal values, and +0.0 == -0.0, so the reference
// answers with the sign of the first zero in row order whenever the minimum (or the maximum) is zero.  No fold of
// floats or of order-preserving keys keeps that, so both kernels report it on the side: a wave (here: a workgroup)
// whose own extreme is zero finds its first zero and folds (flat index << 1) | sign bit into one 64-bit word with an
// atomic minimum; MinMaxAcc::result takes the sign from that word.  `base` is the flat index of data[0] among all
// values fed so far.  Data without a zero extreme never enters that path.
constexpr unsigned long long kNoZero = ~0ull;
__device__ __forceinline__ void note_zero(float v, uint64_t idx, unsigned long long &zk) {
    if (v == 0.0f && zk == kNoZero) zk = (idx << 1) | (__float_as_uint(v) >> 31);  // a thread's indices only grow
}
__global__ __launch_bounds__(kBlock) void minmax_kernel(const float *__restrict__ data, uint64_t n,
                                                       float *__restrict__ partial /* 2 per block */, uint64_t base,
                                                       unsigned long long *__restrict__ first_zero) {
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    unsigned long long zk = kNoZero;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t n4 = ((reinterpret_cast<uintptr_t>(data) & 15) == 0) ? n / 4 : 0;
    const float4 *d4 = reinterpret_cast<const float4 *>(data);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
        float4 v = ld_nt(d4 + i);
        mn = v.x < mn ? v.x : mn; mx = v.x > mx ? v.x : mx;
        mn = v.y < mn ? v.y : mn; mx = v.y > mx ? v.y : mx;
        mn = v.z < mn ? v.z : mn; mx = v.z > mx ? v.z : mx;
        mn = v.w < mn ? v.w : mn; mx = v.w > mx ? v.w : mx;
        note_zero(v.x, i * 4, zk); note_zero(v.y, i * 4 + 1, zk); note_zero(v.z, i * 4 + 2, zk); note_zero(v.w, i * 4 + 3, zk);
    }
    for (uint64_t i = n4 * 4 + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        float v = data[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        note_zero(v, i, zk);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        float o = __shfl_xor(mn, m, 64);
        mn = o < mn ? o : mn;
        o = __shfl_xor(mx, m, 64);
        mx = o > mx ? o : mx;
        const unsigned long long z = __shfl_xor(zk, m, 64);
        zk = z < zk ? z : zk;
    }
    __shared__ float smn[kBlock / 64], smx[kBlock / 64];
    __shared__ unsigned long long szk[kBlock / 64];
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
        szk[threadIdx.x >> 6] = zk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) {
            mn = smn[w] < mn ? smn[w] : mn;
            mx = smx[w] > mx ? smx[w] : mx;
            zk = szk[w] < zk ? szk[w] : zk;
        }
        partial[2 * blockIdx.x] = mn;
        partial[2 * blockIdx.x + 1] = mx;
        if ((mn == 0.0f || mx == 0.0f) && zk != kNoZero) atomicMin(first_zero, (base << 1) + zk);
    }
}

// Pass 1, streaming form: one 16 KiB tile per wave (non-persistent, nt loads — the shape that
// reads HBM fastest, see u8_scan_kernel), per-workgroup min/max folded into 64 sharded slots
// with integer atomics on order-preserving keys, so that a whole store needs ONE read-back.
// NaNs are skipped exactly like the reference's `value < min` / `value > max`.
__device__ __forceinline__ uint32_t f32_order_key(float f) {
    uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
constexpr int kMinmaxSlots = 64, kMinmaxSlotStride = 64;  // one slot pair per 256-byte line
__global__ __launch_bounds__(kScanBlock) void minmax_stream_kernel(const float4 *__restrict__ d4, uint64_t n4,
                                                                  uint32_t *__restrict__ slots, uint64_t base_values,
                                                                  unsigned long long *__restrict__ first_zero) {
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    const uint64_t base = wave * 1024 + (threadIdx.x & 63);
    if (wave * 1024 >= n4) return;
    // the same wave index in scalar registers, for the zero path at the end: nothing of it occupies a vector register
    const uint64_t swave = (uint64_t)blockIdx.x * (kScanBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
    const float qnan = __uint_as_float(0x7FC00000u);
    float4 v[16];
    if (wave * 1024 + 1024 <= n4) {
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = ld_nt(d4 + base + j * 64);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t i = base + j * 64;
            v[j] = i < n4 ? ld_nt(d4 + i) : make_float4(qnan, qnan, qnan, qnan);  // NaN: skipped by both folds
        }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        mn = v[j].x < mn ? v[j].x : mn; mx = v[j].x > mx ? v[j].x : mx;
        mn = v[j].y < mn ? v[j].y : mn; mx = v[j].y > mx ? v[j].y : mx;
        mn = v[j].z < mn ? v[j].z : mn; mx = v[j].z > mx ? v[j].z : mx;
        mn = v[j].w < mn ? v[j].w : mn; mx = v[j].w > mx ? v[j].w : mx;
    }
    // wave fold: DPP inside each 16-lane row, then the four row results through readlane
    float o;
    o = dpp_f32<0xB1>(mn); mn = o < mn ? o : mn;   o = dpp_f32<0xB1>(mx); mx = o > mx ? o : mx;
    o = dpp_f32<0x4E>(mn); mn = o < mn ? o : mn;   o = dpp_f32<0x4E>(mx); mx = o > mx ? o : mx;
    o = dpp_f32<0x141>(mn); mn = o < mn ? o : mn;  o = dpp_f32<0x141>(mx); mx = o > mx ? o : mx;
    o = dpp_f32<0x140>(mn); mn = o < mn ? o : mn;  o = dpp_f32<0x140>(mx); mx = o > mx ? o : mx;
    float wmn = mn, wmx = mx;
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mn), r));
        const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx), r));
        wmn = a < wmn ? a : wmn;
        wmx = c > wmx ? c : wmx;
    }
    if ((threadIdx.x & 63) == 0) {
        // The slot only ever moves outwards, so a stale read can cost a redundant atomic but never
        // lose an update; after the first few tiles almost no wave needs the atomic at all.
        uint32_t *slot = slots + (wave & (kMinmaxSlots - 1)) * kMinmaxSlotStride;
        const uint32_t kmn = f32_order_key(wmn), kmx = f32_order_key(wmx);
        if (kmn < __builtin_nontemporal_load(slot)) atomicMin(slot, kmn);
        if (kmx > __builtin_nontemporal_load(slot + 1)) atomicMax(slot + 1, kmx);
    }
    // A zero extreme (see minmax_kernel): the tile's first zero in row order.  Lane 0 holds the whole wave's fold.
    const float umn = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wmn)));
    const float umx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wmx)));
    // Data full of zeros (anything clipped at zero) brings every wave here; all but the first few leave at once: an
    // earlier zero is already known.  (Reading the tile again costs as much as the first read: 2M x 768 took 4.8 ms
    // instead of 3.8 ms without this test.)  The word only falls, so a stale value costs a redundant search, no more.
    const unsigned long long tile_key = (base_values + swave * 4096) << 1;
    if ((umn == 0.0f || umx == 0.0f) && __hip_atomic_load(first_zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > tile_key) {
        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));  // not threadIdx: see swave
        uint32_t zk = 0xFFFFFFFFu;  // ((float4 of the tile * 4 + component) << 1) | sign bit
#pragma unroll 1
        for (int j = 15; j >= 0; j--) {  // downwards: the lowest index is written last.  The tile is read again (it
            const uint64_t i = swave * 1024 + j * 64 + lane;  // is in the cache), a float4 at a time
            if (i >= n4) continue;
            const float4 t = d4[i];
            const uint32_t at = ((uint32_t)j * 64 + lane) * 8;
            if (t.w == 0.0f) zk = (at + 6) | (__float_as_uint(t.w) >> 31);
            if (t.z == 0.0f) zk = (at + 4) | (__float_as_uint(t.z) >> 31);
            if (t.y == 0.0f) zk = (at + 2) | (__float_as_uint(t.y) >> 31);
            if (t.x == 0.0f) zk = at | (__float_as_uint(t.x) >> 31);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t z = __shfl_xor(zk, m, 64);
            zk = z < zk ? z : zk;
        }
        if (lane == 0 && zk != 0xFFFFFFFFu) {
            const unsigned long long key = tile_key + zk;
            if (key < __builtin_nontemporal_load(first_zero)) atomicMin(first_zero, key);
        }
    }
}

// Pass 2, streaming form (dim % 4 == 0, 16-byte aligned input): 16 lanes per row, 4 rows per
// wave, one wave per tile.  Lane `sub` converts float4 #(sub + 16*it) of its row into one dword
// of codes: every wave-load is 4 x 256 contiguous bytes and up to four are in flight per lane;
// the row sums finish with DPP row adds.  Same arithmetic as quantize_kernel.
// Measured (2M x 768, profiles/r03_quantize_shapes.txt): 1.36-1.37 ms = 5.6 TB/s of read + written bytes with the
// exact division AND with the division-free conversion -- the kernel is bound by the mixed read/write stream, not
// by the vector ALU; plain instead of nt stores: the same; a lane owning four consecutive float4 (one 16-byte
// store per lane, loads at a 64-byte lane stride): 3.6 ms.
template <int ITERS /* float4 per lane, 0 = any dim (loop of 4-deep batches) */, bool FAST /* f32x4_to_u8x4_fast */,
          int LEVELS = 127 /* code levels (f32_to_code); 15 and 255 are never FAST */>
__global__ __launch_bounds__(kScanBlock) void quantize16_kernel(
    const float *__restrict__ data, uint64_t n_rows, uint32_t dim, uint32_t actual_dim, float alpha,
    float offset, int distance, int invert, uint32_t *__restrict__ codes32, float *__restrict__ offsets,
    uint64_t row0) {
    const float r_alpha = 1.0f / alpha;
    const int lane = threadIdx.x & 63, sub = lane & 15, rslot = lane >> 4;
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    if (wave * 4 >= n_rows) return;
    const uint64_t r = wave * 4 + rslot;
    const bool row_ok = r < n_rows;
    const uint64_t rc = row_ok ? r : n_rows - 1;  // clamped: loads stay in bounds, stores are masked
    const float *src = data + rc * dim;
    const float4 *src4 = reinterpret_cast<const float4 *>(src);
    const uint32_t dwords = actual_dim / 4, f4 = dim / 4;
    uint32_t *dst = codes32 + (row0 + rc) * dwords;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code<LEVELS>(placeholder, alpha, offset);
    const uint32_t pad_dword = pad_code * 0x01010101u;
    uint32_t s1 = 0, s2 = 0;
    constexpr int DEPTH = ITERS ? ITERS : 4;
    for (uint32_t d0 = sub; d0 < dwords; d0 += 16 * DEPTH) {
        float4 f[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            const uint32_t d = d0 + 16 * j;
            f[j] = d < f4 ? ld_nt(src4 + d) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            const uint32_t d = d0 + 16 * j;
            if (d >= dwords) break;
            uint32_t packed;
            if (d < f4) {
                if (FAST) {
                    packed = f32x4_to_u8x4_fast(f[j], alpha, offset, r_alpha);
                } else {
                    packed = f32_to_code<LEVELS>(f[j].x, alpha, offset) | (f32_to_code<LEVELS>(f[j].y, alpha, offset) << 8) |
                             (f32_to_code<LEVELS>(f[j].z, alpha, offset) << 16) | (f32_to_code<LEVELS>(f[j].w, alpha, offset) << 24);
                }
                s1 = __builtin_amdgcn_udot4(packed, 0x01010101u, s1, false);  // sum of the four codes
                s2 = __builtin_amdgcn_udot4(packed, packed, s2, false);       // sum of their squares
            } else {
                packed = pad_dword;
                s1 += 4 * pad_code;
                s2 += 4 * pad_code * pad_code;
            }
            if (row_ok) __builtin_nontemporal_store(packed, dst + d);  // 16 lanes x 4 B = one 64-byte segment
        }
        if (ITERS) break;
    }
    s1 = group_sum<16>(s1);
    s2 = group_sum<16>(s2);
    if (sub == 0 && row_ok) {
        float vo;
        const float D = (float)actual_dim;
        if (distance == QAMD_DOT) {
            float sum = (float)s1;
            if (s1 >= (1u << 24)) {
                sum = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++)
                    sum += (float)(j < dim ? f32_to_code<LEVELS>(src[j], alpha, offset) : pad_code);
            }
            vo = D * offset * offset + sum * alpha * offset;
        } else if (distance == QAMD_L1) {
            vo = 0.0f;
        } else {
            float sum = (float)s2;
            if (s2 >= (1u << 24)) {
                sum = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    const float c = (float)(j < dim ? f32_to_code<LEVELS>(src[j], alpha, offset) : pad_code);
                    sum += c * c;
                }
            }
            vo = D * offset * offset + sum * alpha * alpha;
        }
        offsets[row0 + r] = invert ? -vo : vo;
    }
}

// Pass 2: one wave per row (encoded_vectors_u8.rs:73-118).  Lane l quantizes elements
// 4l..4l+3 of each 256-element slab into one dword of codes; the row's code sums are exact
// integers.  vector_offset is the reference's sequential f32 sum: identical to the integer
// sum while that is < 2^24; beyond it (only possible for sum of squares at actual_dim > 1040)
// lane 0 replays the sequential f32 loop.
__global__ __launch_bounds__(kBlock) void quantize_kernel(
    const float *__restrict__ data, uint64_t n_rows, uint32_t dim, uint32_t actual_dim, float alpha,
    float offset, int distance, int invert, uint32_t *__restrict__ codes32 /* row stride actual_dim/4 */,
    float *__restrict__ offsets, uint64_t row0, int levels) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, levels);
    const uint32_t dwords = actual_dim / 4;
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const float *src = data + r * dim;
        uint32_t *dst = codes32 + (row0 + r) * dwords;
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t d = lane; d < dwords; d += 64) {  // dword loads: dim % 4 != 0 or an unaligned source (launch_quantize)
            uint32_t packed = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                uint32_t j = d * 4 + b;
                uint32_t c = j < dim ? f32_to_code(src[j], alpha, offset, levels) : pad_code;
                packed |= c << (8 * b);
                s1 += c;
                s2 += c * c;
            }
            dst[d] = packed;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            s1 += __shfl_xor(s1, m, 64);
            s2 += __shfl_xor(s2, m, 64);
        }
        if (lane == 0) {
            float vo;
            const float D = (float)actual_dim;
            if (distance == QAMD_DOT) {
                float s = (float)s1;  // 127*actual_dim < 2^24 for every dim < 132k
                if (s1 >= (1u << 24)) {
                    s = 0.0f;
                    for (uint32_t j = 0; j < actual_dim; j++)
                        s += (float)(j < dim ? f32_to_code(src[j], alpha, offset, levels) : pad_code);
                }
                vo = D * offset * offset + s * alpha * offset;
            } else if (distance == QAMD_L1) {
                vo = 0.0f;
            } else {
                float s = (float)s2;
                if (s2 >= (1u << 24)) {
                    s = 0.0f;
                    for (uint32_t j = 0; j < actual_dim; j++) {
                        float c = (float)(j < dim ? f32_to_code(src[j], alpha, offset, levels) : pad_code);
                        s += c * c;
                    }
                }
                vo = D * offset * offset + s * alpha * alpha;
            }
            offsets[row0 + r] = invert ? -vo : vo;
        }
    }
}

// ---- rotated stores (the reference has no counterpart) ----
// The store holds y^ = c * y, y the block rotation of the row (rotate_blocks.hpp) and c = 2^(-log2(B) / 2)
// rounded to f32: one multiply per value, rounded on its own (__fmul_rn), then the quantizer above on y^.  dim is a
// multiple of 64, so actual_dim == dim: no pad codes, and a 4-value chunk is one dword of codes.  Three consumers of a
// rotated row, each a sink of the two kernel frames of rotate_blocks.hpp (a wave per row for dim <= 2048, the row in
// registers, and a workgroup per row, the row in LDS): min/max (pass 1; nothing is written per row), quantize (pass 2,
// push, upsert: the codes and the row offset as quantize16_kernel writes them) and the values themselves (queries, the
// quantile sample).  The frames call a sink for live chunks only: the lanes of a last chunk past dim / 4, which hold
// +-0.0, reach no fold and no store.
constexpr int kQuant4Bit = 2;  // `fast` of RotQuantizeSink: 0 the exact division, 1 the division-free form, 2 4-bit codes
constexpr int kQuantFull = 3;  // 3: full-range codes
__device__ __forceinline__ uint32_t rot_quant4(const float (&v)[4], float alpha, float offset, float r_alpha, int fast) {
    const float4 f = make_float4(v[0], v[1], v[2], v[3]);
    if (fast == kQuant4Bit)  // a 4-bit store; wave-uniform
        return f32_to_u4(f.x, alpha, offset) | (f32_to_u4(f.y, alpha, offset) << 8) | (f32_to_u4(f.z, alpha, offset) << 16) |
               (f32_to_u4(f.w, alpha, offset) << 24);
    if (fast == kQuantFull)  // a full-range store; wave-uniform
        return f32_to_code<255>(f.x, alpha, offset) | (f32_to_code<255>(f.y, alpha, offset) << 8) |
               (f32_to_code<255>(f.z, alpha, offset) << 16) | (f32_to_code<255>(f.w, alpha, offset) << 24);
    if (fast) return f32x4_to_u8x4_fast(f, alpha, offset, r_alpha);
    return f32_to_u8(f.x, alpha, offset) | (f32_to_u8(f.y, alpha, offset) << 8) | (f32_to_u8(f.z, alpha, offset) << 16) |
           (f32_to_u8(f.w, alpha, offset) << 24);
}
// vector_offset of a row from its code sums (quantize16_kernel's epilogue; s1 <= 255 * 16384 < 2^24 always).  `sum2` is
// the f32 sum of squares: (float)s2 below 2^24, else the caller's replay of the reference's sequential f32 loop.
__device__ __forceinline__ float rot_row_offset(uint32_t dim, float alpha, float offset, int distance, int invert, uint32_t s1,
                                                float sum2) {
    const float D = (float)dim;
    float vo;
    if (distance == QAMD_DOT) {
        const float sum = (float)s1;
        vo = D * offset * offset + sum * alpha * offset;
    } else {
        vo = D * offset * offset + sum2 * alpha * alpha;
    }
    return invert ? -vo : vo;
}
// The wave's fold of pass 1 into the accumulator's slots (minmax_stream_kernel's protocol) and, for a zero extreme, the
// first zero's (flat index << 1) | sign (minmax_kernel's).
__device__ __forceinline__ void rot_minmax_commit(float mn, float mx, unsigned long long zk, uint64_t slot_id, int lane,
                                                  uint32_t *__restrict__ slots, uint64_t base_values,
                                                  unsigned long long *__restrict__ first_zero) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        float o = __shfl_xor(mn, m, 64);
        mn = o < mn ? o : mn;
        o = __shfl_xor(mx, m, 64);
        mx = o > mx ? o : mx;
        const unsigned long long z = __shfl_xor(zk, m, 64);
        zk = z < zk ? z : zk;
    }
    if (lane == 0) {
        uint32_t *slot = slots + (slot_id & (kMinmaxSlots - 1)) * kMinmaxSlotStride;
        const uint32_t kmn = f32_order_key(mn), kmx = f32_order_key(mx);
        if (kmn < __builtin_nontemporal_load(slot)) atomicMin(slot, kmn);
        if (kmx > __builtin_nontemporal_load(slot + 1)) atomicMax(slot + 1, kmx);
        if ((mn == 0.0f || mx == 0.0f) && zk != kNoZero) atomicMin(first_zero, (base_values << 1) + zk);
    }
}

// Pass 1: the extremes of y^ over a thread's rows and the first zero among them.  A thread's chunks, and its rows, come
// in rising order, so the first zero it meets is the one of the lowest index.
struct RotMinmaxSink : RotSink {
    uint32_t dim;
    float c;
    uint32_t *slots;
    uint64_t base_values;
    unsigned long long *first_zero;
    struct State {
        float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
        unsigned long long zk = kNoZero;
        uint32_t z = 0xFFFFFFFFu;  // (index in the row << 1) | sign of the thread's first zero in the present row
    };
    __device__ void chunk(State &st, uint64_t, uint32_t ch, int, const float (&y)[4], uint32_t &) const {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float v = __fmul_rn(y[e], c);
            st.mn = v < st.mn ? v : st.mn;
            st.mx = v > st.mx ? v : st.mx;
            if (v == 0.0f && st.z == 0xFFFFFFFFu) st.z = ((ch * 4 + e) << 1) | (__float_as_uint(v) >> 31);
        }
    }
    __device__ void row_end(State &st, uint64_t r) const {
        if (st.z != 0xFFFFFFFFu && st.zk == kNoZero) st.zk = ((r * dim) << 1) + st.z;
        st.z = 0xFFFFFFFFu;
    }
    template <int K> __device__ void row_wave(State &st, uint64_t r, int, const uint32_t (&)[K]) const { row_end(st, r); }
    __device__ void row_lds(State &st, uint64_t r, uint32_t *) const { row_end(st, r); }
    __device__ void finish(State &st, uint64_t slot_id, int lane) const {
        rot_minmax_commit(st.mn, st.mx, st.zk, slot_id, lane, slots, base_values, first_zero);
    }
};

// Pass 2, push, upsert: the codes of a row and its offset.  A chunk's codes stay in the frame's `keep` word for the
// sequential replay; State holds the thread's code sums of the present row.
struct RotQuantizeSink : RotSink {
    uint32_t dim;
    float c, alpha, offset;
    int fast, distance, invert;
    uint32_t *codes32;
    float *offsets;
    uint64_t row0;
    struct State {
        uint32_t s1 = 0, s2 = 0;
    };
    __device__ void chunk(State &st, uint64_t r, uint32_t ch, int, const float (&y)[4], uint32_t &keep) const {
        const float v[4] = {__fmul_rn(y[0], c), __fmul_rn(y[1], c), __fmul_rn(y[2], c), __fmul_rn(y[3], c)};
        const uint32_t p = rot_quant4(v, alpha, offset, 1.0f / alpha, fast);
        st.s1 = __builtin_amdgcn_udot4(p, 0x01010101u, st.s1, false);
        st.s2 = __builtin_amdgcn_udot4(p, p, st.s2, false);
        // a wave's 64 lanes x 4 B: 256 consecutive bytes of the row
        __builtin_nontemporal_store(p, codes32 + (row0 + r) * (dim / 4) + ch);
        keep = p;
    }
    // (float)s2 is the f32 sum of squares below 2^24; from there on the row replays the reference's sequential f32 sum,
    // a chunk's four codes at a time in index order
    __device__ bool replays(uint32_t s2) const { return distance == QAMD_L2 && s2 >= (1u << 24); }
    __device__ static void add_squares(float &sum2, uint32_t p) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float cf = (float)((p >> (8 * e)) & 0xFFu);
            sum2 += cf * cf;
        }
    }
    __device__ void wave_sums(State &st) const {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            st.s1 += __shfl_xor(st.s1, m, 64);
            st.s2 += __shfl_xor(st.s2, m, 64);
        }
    }
    // The wave form: every lane holds the sums, scalar from there on, and the replay reads the codes lane by lane.
    template <int K> __device__ void row_wave(State &st, uint64_t r, int lane, const uint32_t (&kept)[K]) const {
        wave_sums(st);
        const uint32_t s1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.s1);
        const uint32_t s2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.s2);
        float sum2 = (float)s2;
        if (replays(s2)) {
            sum2 = 0.0f;
#pragma unroll
            for (int k = 0; k < K; k++)
                for (uint32_t l = 0; l < 64 && (uint32_t)(k * 64) + l < dim / 4; l++)
                    add_squares(sum2, (uint32_t)__builtin_amdgcn_readlane((int)kept[k], (int)l));
        }
        if (lane == 0) offsets[row0 + r] = rot_row_offset(dim, alpha, offset, distance, invert, s1, sum2);
        st = State();
    }
    // The workgroup form: the spare words of the LDS row carry the folds.  A chunk's first word keeps its four codes
    // (`keep`), words 1 and 2 of chunks 0 .. 3 the four waves' code sums.
    __device__ void row_lds(State &st, uint64_t r, uint32_t *row_u) const {
        wave_sums(st);
        __syncthreads();  // every chunk has been read: words 1 and 2 of chunks 0 .. 3 are free
        if ((threadIdx.x & 63) == 0) {
            row_u[(threadIdx.x >> 6) * 4 + 1] = st.s1;
            row_u[(threadIdx.x >> 6) * 4 + 2] = st.s2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s1 = 0, s2 = 0;
            for (int w = 0; w < kRotThreads / 64; w++) s1 += row_u[w * 4 + 1], s2 += row_u[w * 4 + 2];
            float sum2 = (float)s2;
            if (replays(s2)) {
                sum2 = 0.0f;
                for (uint32_t ch = 0; ch < dim / 4; ch++) add_squares(sum2, row_u[ch * 4]);
            }
            offsets[row0 + r] = rot_row_offset(dim, alpha, offset, distance, invert, s1, sum2);
        }
        st = State();
    }
};

// The values themselves (queries, the quantile sample): dim floats per row to `out`.
struct RotValuesSink : RotSink {
    uint32_t dim;
    float c;
    float *out;
    __device__ void chunk(State &, uint64_t r, uint32_t ch, int, const float (&y)[4], uint32_t &) const {
        reinterpret_cast<float4 *>(out + r * dim)[ch] =
            make_float4(__fmul_rn(y[0], c), __fmul_rn(y[1], c), __fmul_rn(y[2], c), __fmul_rn(y[3], c));
    }
};

// Reference-format rows <-> device layout (encoded_storage.rs:27-31, row stride actual_dim+4).
__global__ __launch_bounds__(kBlock) void split_rows_kernel(const uint32_t *__restrict__ rows32,
                                                           uint64_t n_rows, uint32_t row_dwords,
                                                           uint32_t *__restrict__ codes32,
                                                           float *__restrict__ offsets) {
    const uint64_t total = n_rows * row_dwords;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        uint64_t r = t / row_dwords;
        uint32_t k = (uint32_t)(t - r * row_dwords);
        uint32_t w = rows32[t];
        if (k == 0)
            offsets[r] = __uint_as_float(w);
        else
            codes32[r * (row_dwords - 1) + (k - 1)] = w;
    }
}

__global__ __launch_bounds__(kBlock) void join_rows_kernel(const uint32_t *__restrict__ codes32,
                                                          const float *__restrict__ offsets,
                                                          uint64_t n_rows, uint32_t row_dwords,
                                                          uint32_t *__restrict__ rows32) {
    const uint64_t total = n_rows * row_dwords;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        uint64_t r = t / row_dwords;
        uint32_t k = (uint32_t)(t - r * row_dwords);
        rows32[t] = k == 0 ? __float_as_uint(offsets[r]) : codes32[r * (row_dwords - 1) + (k - 1)];
    }
}

// The scan image (u8_internal.hpp; format IMG: Image7, Image4) of rows [r0, r0 + n_rows): one thread per (row, image
// chunk j), which writes IMG::chunk to its place in the row's block of kPackBlockRows rows.  Every (row, chunk) slot is 16
// bytes of its own, so the slots of a block's other rows stay as they are (upsert).  `bad` (builders; null for upsert,
// whose rows come from the store's own encoder): a code with a bit of IMG::kNoCode anywhere in the rows (bytes another
// producer wrote: from_rows, load) sets it, and the image is then dropped (a compact store, which has nothing else, fails).
// `c0`: the store row whose codes codes[0] holds - 0 for the store's own byte codes, the tile's first row for the staging
// buffer of a compact store.
template <class IMG>
__global__ __launch_bounds__(kBlock) void u8_pack_image_kernel(const uint4 *__restrict__ codes, uint64_t c0, uint64_t r0,
                                                               uint64_t n_rows, uint32_t row_chunks, uint32_t pchunks,
                                                               uint4 *__restrict__ packed, uint32_t *__restrict__ bad) {
    const uint64_t total = n_rows * pchunks, stride = (uint64_t)gridDim.x * kBlock;
    uint32_t seen = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t r = r0 + t / pchunks;
        const uint32_t j = (uint32_t)(t % pchunks);
        packed[((r / kPackBlockRows) * pchunks + j) * kPackBlockRows + r % kPackBlockRows] =
            IMG::chunk(codes + (r - c0) * row_chunks, j, row_chunks, pchunks, seen);
    }
    if (bad && (seen & IMG::kNoCode)) atomicOr(bad, 1u);
}

// ---- compact 4-bit stores: image rows back into byte codes ----
// Image rows back into byte codes: out row l gets the codes of store row rows[l] (a row >= count is read as row 0, as
// u8_gather_rows_kernel does) or, without a list, of row r0 + l; `pitch` bytes between out rows, a multiple of 16.  One
// thread per (row, image chunk): 16 bytes in, the two code chunks 2j and 2j + 1 out (the second only where the row has it).
// q_offs (optional): the rows' stored offsets, for the rows that become the queries of score_internal.
__global__ __launch_bounds__(kBlock) void u8_nibble_unpack_kernel(const uint4 *__restrict__ image,
                                                                  const float *__restrict__ offsets,
                                                                  const uint32_t *__restrict__ rows, uint64_t r0, uint64_t n_rows,
                                                                  uint32_t count, uint32_t row_chunks, uint32_t pchunks,
                                                                  uint8_t *__restrict__ out, uint64_t pitch,
                                                                  float *__restrict__ q_offs) {
    const uint64_t total = n_rows * pchunks, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t l = t / pchunks;
        const uint32_t j = (uint32_t)(t % pchunks);
        uint64_t r = r0 + l;
        if (rows) r = rows[l] < count ? rows[l] : 0u;
        const uint4 w = image[nibble_at(r, j, pchunks)];
        uint4 *dst = reinterpret_cast<uint4 *>(out + l * pitch);
        dst[2 * j] = nibbles_lo(w);
        if (2 * j + 1 < row_chunks) dst[2 * j + 1] = nibbles_hi(w);
        if (q_offs && j == 0) q_offs[l] = offsets[r];
    }
}

int grid_for(uint64_t work_items, uint64_t per_block, int blocks_per_cu) {
    uint64_t want = (work_items + per_block - 1) / per_block;
    uint64_t cap = (uint64_t)device_info().cu_count * blocks_per_cu;
    if (want < 1) want = 1;
    return (int)(want > cap ? cap : want);
}

// ------------------------------------------------------------------------------ host side
float host_multiplier(float alpha, int distance, int invert) {  // :119-128
    float m = distance == QAMD_DOT ? alpha * alpha : distance == QAMD_L1 ? alpha : -2.0f * alpha * alpha;
    return invert ? -m : m;
}

// ---- rotated stores: the launchers of the Rot*Sink consumers (launch_rot, rotate_blocks.hpp) ----
// c = 2^(-log2(B) / 2) as an f32: a power of two for even log2(B), the f32 nearest to 2^-1/2 scaled by one for odd
float rot_scale_of(uint32_t B) {
    const int lg = __builtin_ctz(B);
    return std::ldexp((lg & 1) ? 0.70710678118654752440f : 1.0f, -(lg / 2));
}
// A u8 row keeps its dim values: src_dim = width = dim, B the largest power of two that divides it.
template <class SINK> qamd_status launch_rot_u8(SINK sink, const float *src, uint64_t n, uint64_t dim, hipStream_t s) {
    if (n == 0) return QAMD_OK;
    const uint32_t B = (uint32_t)rot_block(dim);
    sink.dim = (uint32_t)dim, sink.c = rot_scale_of(B);
    launch_rot(sink, src, n, (uint32_t)dim, (uint32_t)dim, B, s);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// Every caller has checked dim (rot_dim_ok) and holds `src` in device memory.
qamd_status launch_rot_minmax(const float *src, uint64_t n, uint64_t dim, uint32_t *slots, uint64_t base_values,
                              unsigned long long *first_zero, hipStream_t s) {
    RotMinmaxSink sink;
    sink.slots = slots, sink.base_values = base_values, sink.first_zero = first_zero;
    return launch_rot_u8(sink, src, n, dim, s);
}
bool rot_dim_ok(uint64_t dim) { return dim != 0 && dim % kRotBlockMin == 0 && dim <= kRotMaxDim; }

}  // namespace

// The two launchers the read side calls too (u8_internal.hpp): the kernels stay in this file.
namespace qamd {

qamd_status u8_rot_values(const float *src, uint64_t n, uint64_t dim, float *out, hipStream_t s) {
    RotValuesSink sink;
    sink.out = out;
    return launch_rot_u8(sink, src, n, dim, s);
}

qamd_status u8_unpack_rows(const qamd_u8 *h, const uint32_t *rows_dev, uint64_t r0, uint64_t n, uint8_t *out, uint64_t pitch,
                           float *q_offs, hipStream_t s) {
    if (n == 0) return QAMD_OK;
    hipLaunchKernelGGL(u8_nibble_unpack_kernel, dim3(grid_for(n * h->image.chunks, kBlock, 8)), dim3(kBlock), 0, s,
                       h->packed.as<uint4>(), h->offsets.as<float>(), rows_dev, r0, n, (uint32_t)h->count, h->row_chunks,
                       h->image.chunks, out, pitch, q_offs);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

}  // namespace qamd

// ------------------------------------------------------------------------------ handles
// struct qamd_u8 / qamd_u8_query: u8_internal.hpp

namespace {

U8Image u8_image_of(uint32_t rc, bool four_bit, int distance, bool full_range = false);

qamd_status alloc_store(qamd_u8 *h) {
    h->capacity = h->count;
    h->padded_rows = padded_rows_of(h->capacity);
    h->row_chunks = (uint32_t)(h->meta.actual_dim / 16);
    // every builder (encode, from_rows, load) writes all `count` rows; only the padding is zeroed
    QAMD_TRY(h->offsets.alloc_zero_tail(h->padded_rows * sizeof(float), h->count * sizeof(float)));
    if (h->compact) {  // offsets and image, no byte codes; the builders write the image tile by tile
        h->image = u8_image_of(h->row_chunks, true, h->meta.vector_parameters.distance_type);  // split_distance: it has one
        const uint64_t chunk_bytes = (uint64_t)h->image.chunks * 16;
        // rows of a block are interleaved: the padding rows of the last block are zeroed with it, before it is written
        // (a store that keeps its byte codes goes on without an image it cannot allocate; here that is QAMD_ERR_DEVICE)
        return h->packed.alloc_zero_tail(h->padded_rows * chunk_bytes, h->count / kPackBlockRows * kPackBlockRows * chunk_bytes);
    }
    QAMD_TRY(h->codes.alloc_zero_tail(h->padded_rows * h->meta.actual_dim, h->count * h->meta.actual_dim));
    return QAMD_OK;
}

// The scan image a store of this shape can have (u8_internal.hpp): which format, how many chunks per row, and the
// format's second kernel argument (Image7: the extra chunks, Image4: the row's code chunks).  Only the Dot / L2 scans of
// lane mode 0 read an image, so L1 stores and stores of more than 128 chunks (the generic kernel) have none; nor do
// 7-bit stores of fewer than 8 chunks (no whole extra chunk) and 4-bit stores of fewer than 2.
// A full-range store has none either: its codes do not fit 7 bits, and it keeps bytes only.
U8Image u8_image_of(uint32_t rc, bool four_bit, int distance, bool full_range) {
    if (full_range || distance == QAMD_L1 || rc > 128 || rc < (four_bit ? 2u : 8u)) return U8Image{};
    if (four_bit) return U8Image{U8_IMAGE_NIBBLE, (rc + 1) / 2, rc};
    return U8Image{U8_IMAGE_7BIT, rc - rc / 8, rc / 8};
}

// Writes rows [r0, r0 + n_rows) of the store's image from their byte codes; `bad`: u8_pack_image_kernel.
// `tile` (a compact store): the byte codes of exactly these rows, in the staging buffer.
qamd_status launch_pack(const qamd_u8 *h, uint64_t r0, uint64_t n_rows, uint32_t *bad, hipStream_t s,
                        const uint4 *tile = nullptr) {
    const auto kernel = h->image.kind == U8_IMAGE_NIBBLE ? u8_pack_image_kernel<Image4> : u8_pack_image_kernel<Image7>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n_rows * h->image.chunks, kBlock, 8)), dim3(kBlock), 0, s,
                       tile ? tile : h->codes_7bit<uint4>(), tile ? r0 : 0, r0, n_rows, h->row_chunks, h->image.chunks,
                       h->packed.as<uint4>(), bad);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// ---- compact stores: tiles of byte codes on their way into the image, and image rows on their way out ----
// Rows per tile: a multiple of the image's block, so that the tiles of a builder that starts at row 0 cover whole blocks.
// 64 MiB of byte codes, small enough to stay in the 256 MB Infinity Cache between the quantize kernel and the pack
// kernel - which bought no measurable time against tiles of 16 MB to 768 MB; kept because it bounds the
// staging buffer.
constexpr uint64_t kCompactTileBytes = 64ull << 20;
uint64_t compact_tile_rows(const qamd_u8 *h) {
    const uint64_t rows = stage_bytes(kCompactTileBytes) / std::max<uint64_t>(h->meta.actual_dim, 1);
    return std::max<uint64_t>(kPackBlockRows, rows / kPackBlockRows * kPackBlockRows);
}
// The staging buffer with room for a tile of `n_rows` rows (grown on demand, reused from tile to tile in stream order).
qamd_status compact_stage(qamd_u8 *h, uint64_t n_rows, hipStream_t s) {
    const uint64_t need = std::min(compact_tile_rows(h), round_up(n_rows, kPackBlockRows)) * h->meta.actual_dim;
    if (h->stage.bytes >= need) return QAMD_OK;
    QAMD_HIP(hipStreamSynchronize(s));  // a smaller one may still be read
    return h->stage.alloc(need);
}
// The end of every builder and upsert of a compact store: the staging buffer goes back.
void compact_done(qamd_u8 *h) {
    h->stage.release();
    h->packed_rows.release();
}

// Builds the store's scan image from its byte codes; run at the end of every builder.  The 7-bit image costs 7/8 of the
// code bytes in HBM, the nibble image of a 4-bit store half: it is skipped when it would leave less free
// HBM than its own size, and a failed allocation only leaves the store on its byte codes.  So does a code the format
// cannot hold (rows another producer wrote).
qamd_status build_packed(qamd_u8 *h, hipStream_t s) {
    if (h->compact) return compact_done(h), QAMD_OK;  // the image is what the builder wrote, tile by tile
    h->packed.release();
    h->packed_rows.release();
    h->image = U8Image{};
    const U8Image im = u8_image_of(h->row_chunks, h->four_bit, h->meta.vector_parameters.distance_type, h->full_range);
    if (!u8_packed_allowed() || h->count == 0 || !im.kind) return QAMD_OK;
    const uint64_t bytes = h->padded_rows * im.chunks * 16;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 2 * bytes) {
        (void)hipGetLastError();
        return QAMD_OK;
    }
    DevBuf bad;
    const std::string err = last_error();
    // rows of a block are interleaved: the padding rows of the last block are zeroed with it, before it is written
    if (h->packed.alloc_zero_tail(bytes, h->count / kPackBlockRows * kPackBlockRows * im.chunks * 16) != QAMD_OK ||
        bad.alloc(sizeof(uint32_t), true) != QAMD_OK) {
        (void)hipGetLastError();  // an out-of-memory here is not the build's failure
        last_error() = err;
        h->packed.release();
        return QAMD_OK;
    }
    h->image = im;
    uint32_t high = 1;  // the store keeps an image that was written and found clean, and no other
    const qamd_status st = [&]() -> qamd_status {
        QAMD_TRY(launch_pack(h, 0, h->count, bad.as<uint32_t>(), s));
        QAMD_HIP(hipMemcpyAsync(&high, bad.ptr, sizeof(high), hipMemcpyDeviceToHost, s));
        QAMD_HIP(hipStreamSynchronize(s));
        return QAMD_OK;
    }();
    if (st != QAMD_OK || high) {
        h->packed.release();
        h->image = U8Image{};
    }
    return st;
}

// Gather `n_out` evenly strided rows of a device-resident [count][dim] array (quantile sample).
__global__ __launch_bounds__(kBlock) void gather_strided_rows_kernel(const float *__restrict__ data, uint64_t count,
                                                                    uint32_t dim, uint64_t n_out,
                                                                    float *__restrict__ out) {
    const uint64_t total = n_out * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = i / dim, j = i - k * dim;
        const uint64_t r = (uint64_t)((unsigned __int128)k * count / n_out);
        out[i] = data[r * dim + j];
    }
}

bool quantile_cut(uint64_t slice, uint64_t dim, float quantile, uint64_t &cut);

// find_quantile_interval (quantile.rs:21-71).  The reference keeps, after two
// select_nth_unstable calls, the values of sorted rank (cut, len - cut) exclusive and returns
// their min and max: sorted[cut + 1] and sorted[len - cut - 1], i.e. the (cut+2)-th smallest
// and the (cut+1)-th largest value — two exact radix selects on the GPU.
// count <= 100 000: the sample is every vector (exactly the reference).  Larger stores: an
// evenly strided subset (the reference draws a random one; statistic, not bits).
// `rotated`: the interval is that of the sampled rows' rotation, written to a buffer of their size.
qamd_status quantile_interval_device(const float *data, qamd_mem data_mem, uint64_t count, uint64_t dim,
                                     float quantile, hipStream_t s, bool &found, float &mn, float &mx,
                                     bool rotated = false) {
    found = false;
    const uint64_t slice = std::min<uint64_t>(count, kQuantileSample);
    const uint64_t len = slice * dim;
    uint64_t cut = 0;
    if (!quantile_cut(slice, dim, quantile, cut)) return QAMD_OK;
    DevBuf sample;
    const float *vals = data;
    if (data_mem == QAMD_MEM_HOST) {
        QAMD_TRY(sample.alloc(len * 4));
        if (slice == count) {
            QAMD_TRY(copy_in(sample.ptr, data, QAMD_MEM_HOST, len * 4, s));
        } else {
            std::vector<float> rows(len);  // row gather only: no arithmetic on the host
            for (uint64_t k = 0; k < slice; k++)
                memcpy(&rows[k * dim], data + (uint64_t)((unsigned __int128)k * count / slice) * dim, dim * 4);
            QAMD_TRY(copy_in(sample.ptr, rows.data(), QAMD_MEM_HOST, len * 4, s));
        }
        vals = sample.as<float>();
    } else if (slice != count) {
        QAMD_TRY(sample.alloc(len * 4));
        hipLaunchKernelGGL(gather_strided_rows_kernel, dim3(grid_for(len, kBlock * 4, 8)), dim3(kBlock), 0, s, data,
                           count, (uint32_t)dim, slice, sample.as<float>());
        QAMD_HIP(hipGetLastError());
        vals = sample.as<float>();
    }
    DevBuf rot;
    if (rotated) {
        QAMD_TRY(rot.alloc(len * 4));
        QAMD_TRY(u8_rot_values(vals, slice, dim, rot.as<float>(), s));
        vals = rot.as<float>();
    }
    QAMD_TRY(select_kth_f32(vals, len, cut + 2, false, &mn, s));
    QAMD_TRY(select_kth_f32(vals, len, cut + 1, true, &mx, s));
    found = true;
    return QAMD_OK;
}


// PASS 1 accumulator (quantile.rs:5-19): global min / max over any number of device-resident
// batches, kept on the device (64 sharded slot pairs) until result() reads it back once.
struct MinMaxAcc {
    DevBuf slots, partial;
    std::vector<float> hp;
    int mm_grid = 0;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;  // folded from the scalar-form launches
    uint64_t fed = 0;  // values fed so far: the flat index of the next feed's first value
    static constexpr size_t kZeroWordAt = kMinmaxSlots * kMinmaxSlotStride;  // behind the slots: (index << 1) | sign of the first zero

    unsigned long long *first_zero() { return reinterpret_cast<unsigned long long *>(slots.as<uint32_t>() + kZeroWordAt); }

    qamd_status init(hipStream_t s) {
        QAMD_TRY(slots.alloc((kZeroWordAt + 2) * sizeof(uint32_t)));
        std::vector<uint32_t> init(kZeroWordAt + 2, 0u);
        init[kZeroWordAt] = init[kZeroWordAt + 1] = 0xFFFFFFFFu;  // kNoZero
        for (int b = 0; b < kMinmaxSlots; b++) {
            init[b * kMinmaxSlotStride] = 0xFFFFFFFFu;  // min slot: largest key
            init[b * kMinmaxSlotStride + 1] = 0u;       // max slot: smallest key
        }
        QAMD_TRY(copy_in(slots.ptr, init.data(), QAMD_MEM_HOST, init.size() * 4, s));
        mm_grid = device_info().cu_count * 4;
        QAMD_TRY(partial.alloc((size_t)mm_grid * 2 * sizeof(float)));
        hp.resize((size_t)mm_grid * 2);
        return QAMD_OK;
    }

    // src: device memory, nvals f32.  Synchronises only for the scalar-form (unaligned / tail) launches.
    qamd_status feed(const float *src, uint64_t nvals, hipStream_t s) {
        if (nvals == 0) return QAMD_OK;
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && nvals >= 4) {
            const uint64_t n4 = nvals / 4;
            const unsigned grid = (unsigned)((n4 + 1024 * (kScanBlock / 64) - 1) / (1024 * (kScanBlock / 64)));
            hipLaunchKernelGGL(minmax_stream_kernel, dim3(grid), dim3(kScanBlock), 0, s,
                               reinterpret_cast<const float4 *>(src), n4, slots.as<uint32_t>(), fed, first_zero());
            if (nvals % 4) {  // the 1..3 trailing values
                hipLaunchKernelGGL(minmax_kernel, dim3(1), dim3(kBlock), 0, s, src + n4 * 4, nvals % 4,
                                   partial.as<float>(), fed + n4 * 4, first_zero());
                QAMD_TRY(copy_out(hp.data(), QAMD_MEM_HOST, partial.ptr, 8, s));
                if (hp[0] < mn) mn = hp[0];
                if (hp[1] > mx) mx = hp[1];
            }
        } else {  // unaligned input: grid-stride scalar form
            hipLaunchKernelGGL(minmax_kernel, dim3(mm_grid), dim3(kBlock), 0, s, src, nvals, partial.as<float>(), fed,
                               first_zero());
            QAMD_TRY(copy_out(hp.data(), QAMD_MEM_HOST, partial.ptr, hp.size() * 4, s));
            for (int b = 0; b < mm_grid; b++) {
                if (hp[2 * b] < mn) mn = hp[2 * b];
                if (hp[2 * b + 1] > mx) mx = hp[2 * b + 1];
            }
        }
        fed += nvals;
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }

    // feed() for `nr` rows of a rotated store: the extremes of the rotated values, which are never written
    qamd_status feed_rotated(const float *src, uint64_t nr, uint64_t dim, hipStream_t s) {
        QAMD_TRY(launch_rot_minmax(src, nr, dim, slots.as<uint32_t>(), fed, first_zero(), s));
        fed += nr * dim;
        return QAMD_OK;
    }

    qamd_status result(hipStream_t s, float &out_mn, float &out_mx) {
        std::vector<uint32_t> all_slots(kZeroWordAt + 2);
        QAMD_TRY(copy_out(all_slots.data(), QAMD_MEM_HOST, slots.ptr, all_slots.size() * 4, s));
        auto key_to_f32 = [](uint32_t k) {
            uint32_t u = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
            float f;
            memcpy(&f, &u, 4);
            return f;
        };
        for (int b = 0; b < kMinmaxSlots; b++) {
            const uint32_t kmn = all_slots[b * kMinmaxSlotStride], kmx = all_slots[b * kMinmaxSlotStride + 1];
            if (kmn != 0xFFFFFFFFu) {
                const float v = key_to_f32(kmn);
                if (v < mn) mn = v;
            }
            if (kmx != 0u) {
                const float v = key_to_f32(kmx);
                if (v > mx) mx = v;
            }
        }
        // a zero extreme carries the sign of the first zero fed (quantile.rs:5-19 keeps the first of equal values)
        unsigned long long zero_word;
        memcpy(&zero_word, &all_slots[kZeroWordAt], 8);
        if (zero_word != kNoZero) {
            const float z = (zero_word & 1) ? -0.0f : 0.0f;
            if (mn == 0.0f) mn = z;
            if (mx == 0.0f) mx = z;
        }
        out_mn = mn;
        out_mx = mx;
        return QAMD_OK;
    }
};

// PASS 2 for `nr` device-resident rows (encoded_vectors_u8.rs:73-118): their codes to rows r0 .. r0+nr of `codes32`, their
// offsets to the same rows of `offsets`.
qamd_status quantize_rows(const qamd_u8 *h, const float *src, uint64_t nr, uint32_t *codes32, float *offsets, uint64_t r0,
                          float alpha, float offset, hipStream_t s) {
    if (nr == 0) return QAMD_OK;
    const qamd_vector_parameters &vp = h->meta.vector_parameters;
    const uint64_t dim = vp.dim;
    // the division-free conversion needs a normal alpha well inside the exponent range (f32_to_u8_fast)
    const bool fast = alpha >= 8.673617379884035e-19f && alpha <= 1.152921504606847e+18f;  // 2^-60 .. 2^60
    if (h->rotated) {  // rotated in registers, no copy of the rotated values
        RotQuantizeSink sink;
        sink.alpha = alpha, sink.offset = offset, sink.fast = h->four_bit ? kQuant4Bit : h->full_range ? kQuantFull : (int)fast;
        sink.distance = vp.distance_type, sink.invert = vp.invert;
        sink.codes32 = codes32, sink.offsets = offsets, sink.row0 = r0;
        return launch_rot_u8(sink, src, nr, dim, s);
    }
    if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const uint64_t waves = (nr + 3) / 4;
        const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
        const uint32_t per_lane = (uint32_t)((h->meta.actual_dim / 4 + 15) / 16);  // float4 per lane
        auto go = [&](auto it) {
            auto launch = [&](auto fa, auto levels) {
                hipLaunchKernelGGL((quantize16_kernel<decltype(it)::value, decltype(fa)::value, decltype(levels)::value>),
                                   dim3(grid), dim3(kScanBlock), 0, s, src, nr, (uint32_t)dim, (uint32_t)h->meta.actual_dim, alpha,
                                   offset, vp.distance_type, vp.invert, codes32, offsets, r0);
            };
            if (h->four_bit) launch(std::false_type{}, Int<15>{});  // 4-bit codes take the exact division
            else if (h->full_range) launch(std::false_type{}, Int<255>{});  // 3.1w: so do full-range codes (the fast form's band is keyed on 127)
            else if (fast) launch(std::true_type{}, Int<127>{});
            else launch(std::false_type{}, Int<127>{});
        };
        if (per_lane <= 2) go(Int<2>{});
        else if (per_lane <= 4) go(Int<4>{});
        else if (per_lane <= 6) go(Int<6>{});
        else if (per_lane <= 8) go(Int<8>{});
        else if (per_lane <= 12) go(Int<12>{});
        else if (per_lane <= 16) go(Int<16>{});
        else go(Int<0>{});
    } else {
        int grid = grid_for(nr, kBlock / 64, 8);
        hipLaunchKernelGGL(quantize_kernel, dim3(grid), dim3(kBlock), 0, s, src, nr, (uint32_t)dim,
                           (uint32_t)h->meta.actual_dim, alpha, offset, vp.distance_type, vp.invert,
                           codes32, offsets, r0, h->levels());
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// Rows r0 .. r0+nr of the store from `nr` device-resident rows.  A compact store goes tile by tile: the same
// quantize kernels write a tile's byte codes into the staging buffer (and its offsets into their place), the pack kernel
// moves them into the image at the tile's rows.  Tiles are whole blocks of the image but for a first row inside a block
// (an upsert, a push after an odd batch): every (row, chunk) slot of the image is 16 bytes of its own.
qamd_status launch_quantize(qamd_u8 *h, const float *src, uint64_t nr, uint64_t r0, float alpha, float offset,
                            hipStream_t s) {
    if (!h->compact) return quantize_rows(h, src, nr, h->byte_codes<uint32_t>(), h->offsets.as<float>(), r0, alpha, offset, s);
    const uint64_t tile = compact_tile_rows(h), dim = h->meta.vector_parameters.dim;
    if (nr) QAMD_TRY(compact_stage(h, nr, s));
    for (uint64_t t = 0; t < nr; t += tile) {
        const uint64_t n = std::min(tile, nr - t);
        QAMD_TRY(quantize_rows(h, src + t * dim, n, h->stage.as<uint32_t>(), h->offsets.as<float>() + r0 + t, 0, alpha, offset, s));
        QAMD_TRY(launch_pack(h, r0 + t, n, nullptr, s, h->stage.as<uint4>()));
    }
    return QAMD_OK;
}

// quantile.rs:52-61 bounds shared by the one-shot and the streaming encoder: false = the
// reference keeps the plain min/max interval.
bool quantile_cut(uint64_t slice, uint64_t dim, float quantile, uint64_t &cut) {
    const uint64_t len = slice * dim;
    if (len < 4) return false;  // :48-50
    cut = std::min<uint64_t>((len - 1) / 2, (uint64_t)((float)slice * (1.0f - quantile) / 2.0f));  // :52-55
    cut = std::max<uint64_t>(cut, 1);
    const uint64_t lo = cut + 1, hi = len - cut;
    return !(hi <= lo || hi - lo < 2);  // :63-65
}

// The distance_type a u8 constructor is handed: a qamd_distance, or QAMD_DOT / QAMD_L2 with QAMD_ROTATED,
// QAMD_BITS4 (3.1y) or both or-ed on, and QAMD_COMPACT (3.1z) on top of QAMD_BITS4.  The handle keeps `base` in its
// metadata and the flags beside it (U8Flags, u8_internal.hpp).  No device call.
constexpr int kU8FlagBits = QAMD_ROTATED | QAMD_BITS4 | QAMD_COMPACT | QAMD_FULL;
constexpr uint64_t kFullMaxDim = 16384;  // 255 * 255 * dim < 2^31, and the biased matrix-core sums stay inside an i32
qamd_status split_distance(const qamd_vector_parameters &vp, int &base, U8Flags &f) {
    const int dt = vp.distance_type;
    bool &rotated = f.rotated, &four_bit = f.four_bit;
    rotated = dt >= 0 && (dt & QAMD_ROTATED) != 0;
    four_bit = dt >= 0 && (dt & QAMD_BITS4) != 0;
    f.compact = dt >= 0 && (dt & QAMD_COMPACT) != 0;
    f.full_range = dt >= 0 && (dt & QAMD_FULL) != 0;
    base = dt >= 0 ? (dt & ~kU8FlagBits) : dt;
    if (base < 0 || base > 2) return fail(QAMD_ERR_ARGUMENTS, "bad distance_type %d", dt);
    if (f.full_range && (four_bit || f.compact))
        return fail(QAMD_ERR_ARGUMENTS, "distance_type %d: QAMD_FULL does not go with QAMD_BITS4 or QAMD_COMPACT", dt);
    if (f.full_range && vp.dim > kFullMaxDim)
        return fail(QAMD_ERR_ARGUMENTS, "full-range rows have at most %llu dimensions, not %llu", (unsigned long long)kFullMaxDim,
                    (unsigned long long)vp.dim);
    if (f.compact && !four_bit)
        return fail(QAMD_ERR_ARGUMENTS, "distance_type %d: QAMD_COMPACT goes with QAMD_BITS4 only", dt);
    if (f.compact && base != QAMD_L1 && !u8_image_of((uint32_t)std::min<uint64_t>(actual_dim_of(vp.dim) / 16, 0xFFFFFFFFull), true, base).kind)
        return fail(QAMD_ERR_ARGUMENTS, "a compact store keeps only its nibble image, which rows of 32 to 2048 codes have, not %llu",
                    (unsigned long long)actual_dim_of(vp.dim));
    if (four_bit && base == QAMD_L1)
        return fail(QAMD_ERR_ARGUMENTS, "distance_type %d: 4-bit rows are for Dot and L2 stores", dt);
    if (rotated && base == QAMD_L1)
        return fail(QAMD_ERR_ARGUMENTS, "distance_type %d: L1 is not invariant under the rotation of a rotated store", dt);
    if (rotated && !rot_dim_ok(vp.dim))
        return fail(QAMD_ERR_ARGUMENTS, "rotated rows have a multiple of %llu dimensions, at most %llu, not %llu",
                    (unsigned long long)kRotBlockMin, (unsigned long long)kRotMaxDim, (unsigned long long)vp.dim);
    return QAMD_OK;
}

}  // namespace

// ================================================================================== C ABI
extern "C" {

uint64_t qamd_u8_actual_dim(const qamd_vector_parameters *vp) { return actual_dim_of(vp->dim); }

uint64_t qamd_u8_quantized_vector_size(const qamd_vector_parameters *vp) {
    return actual_dim_of(vp->dim) + sizeof(float);
}

qamd_status qamd_u8_encode(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp,
                           const float *quantile, const float *alpha_offset, qamd_stop_fn stop,
                           void *stop_user, void *stream, qamd_u8 **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    int base_distance = 0;
    U8Flags flags;
    QAMD_TRY(split_distance(*vp, base_distance, flags));
    const bool rotated = flags.rotated;
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    if (vp->count > 0 && vp->dim > 0 && !data) return fail(QAMD_ERR_ARGUMENTS, "data is null");
    QAMD_ON_DEVICE(current_device());
    hipStream_t s = as_stream(stream);
    std::unique_ptr<qamd_u8> h(new qamd_u8);
    h->device = current_device();
    h->count = vp->count;
    h->meta.actual_dim = actual_dim_of(vp->dim);
    h->meta.vector_parameters = *vp;
    h->meta.vector_parameters.distance_type = base_distance;
    h->format() = flags;
    const float levels = (float)flags.levels();  // alpha = (max - min) / levels (:228-232)
    QAMD_TRY(alloc_store(h.get()));
    if (vp->count == 0) {  // encoded_vectors_u8.rs:43-54
        h->meta.alpha = h->meta.offset = h->meta.multiplier = 0.0f;
        if (alpha_offset) {  // an empty SHARD of a store whose interval was found elsewhere keeps that store's metadata
            h->meta.alpha = alpha_offset[0];
            h->meta.offset = alpha_offset[1];
            h->meta.multiplier = host_multiplier(alpha_offset[0], base_distance, vp->invert);
        }
        *out = h.release();
        return QAMD_OK;
    }
    const uint64_t dim = vp->dim, count = vp->count;

    // Host rows: both passes (min/max, quantize) need every value, so when the f32 data fits in
    // a quarter of the free HBM it is uploaded ONCE into a scratch copy and encoded from there
    // (the PCIe transfer is the whole cost of a host-side encode); larger inputs are staged
    // twice, 256 MiB at a time.  With alpha_offset given there is only one pass anyway.
    StreamBuf whole;  // from the stream-ordered pool: a fresh hipMalloc of 6 GB costs as much as its upload
    if (data_mem == QAMD_MEM_HOST && !alpha_offset) {
        size_t free_b = 0, total_b = 0;
        const uint64_t bytes = count * dim * sizeof(float);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes <= free_b / 4 && host_whole_allowed()) {
            QAMD_TRY(whole.alloc(bytes, s));
            const uint64_t piece = stage_bytes(256ull << 20);
            for (uint64_t off = 0; off < bytes; off += piece) {
                if (stop && stop(stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
                QAMD_TRY(copy_in(static_cast<char *>(whole.ptr) + off, reinterpret_cast<const char *>(data) + off,
                                 QAMD_MEM_HOST, std::min<uint64_t>(piece, bytes - off), s));
            }
            data = whole.as<float>();
            data_mem = QAMD_MEM_DEVICE;
        }
    }

    // Source rows: device-resident rows are processed in place (large batches: the stop
    // callback is polled between them), host rows are staged in bounded 256 MiB batches.
    const uint64_t batch_bytes = stage_bytes(data_mem == QAMD_MEM_HOST ? (256ull << 20) : (8ull << 30));
    const uint64_t batch_rows = std::max<uint64_t>(1, std::min<uint64_t>(count, batch_bytes / (dim * 4 + 1)));
    DevBuf stage;
    if (data_mem == QAMD_MEM_HOST) QAMD_TRY(stage.alloc(batch_rows * dim * sizeof(float)));
    auto batch_src = [&](uint64_t r0, uint64_t nr, const float *&src) -> qamd_status {
        src = data + r0 * dim;
        if (data_mem == QAMD_MEM_HOST) {
            QAMD_TRY(copy_in(stage.ptr, src, QAMD_MEM_HOST, nr * dim * 4, s));
            src = stage.as<float>();
        }
        return QAMD_OK;
    };

    float alpha, offset;
    if (alpha_offset) {
        alpha = alpha_offset[0];
        offset = alpha_offset[1];
    } else {
        // PASS 1 (:57): global min/max, accumulated on the device across batches.
        MinMaxAcc acc;
        QAMD_TRY(acc.init(s));
        for (uint64_t r0 = 0; r0 < count; r0 += batch_rows) {
            if (stop && stop(stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
            const uint64_t nr = std::min(batch_rows, count - r0);
            const float *src = nullptr;
            QAMD_TRY(batch_src(r0, nr, src));
            if (rotated) QAMD_TRY(acc.feed_rotated(src, nr, dim, s));
            else QAMD_TRY(acc.feed(src, nr * dim, s));
            if (data_mem == QAMD_MEM_HOST) QAMD_HIP(hipStreamSynchronize(s));  // staging buffer is reused
        }
        float mn, mx;
        QAMD_TRY(acc.result(s, mn, mx));
        alpha = (mx - mn) / levels;  // :228-232
        offset = mn;
        // PASS 1b (:58-71): quantile interval on <= 100 000 sampled vectors.
        if (quantile && !(count < 127 || *quantile >= 1.0f)) {  // :27-29
            bool found = false;
            float qmn = 0.0f, qmx = 0.0f;
            QAMD_TRY(quantile_interval_device(data, data_mem, count, dim, *quantile, s, found, qmn, qmx, rotated));
            if (found) {
                alpha = (qmx - qmn) / levels;
                offset = qmn;
            }
        }
    }

    // PASS 2 (:73-118): quantize rows, stop_condition polled between batches.
    for (uint64_t r0 = 0; r0 < count; r0 += batch_rows) {
        if (stop && stop(stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
        const uint64_t nr = std::min(batch_rows, count - r0);
        const float *src = nullptr;
        QAMD_TRY(batch_src(r0, nr, src));
        QAMD_TRY(launch_quantize(h.get(), src, nr, r0, alpha, offset, s));
        if (data_mem == QAMD_MEM_HOST || stop) QAMD_HIP(hipStreamSynchronize(s));
    }
    QAMD_HIP(hipStreamSynchronize(s));
    h->meta.alpha = alpha;
    h->meta.offset = offset;
    h->meta.multiplier = host_multiplier(alpha, base_distance, vp->invert);
    QAMD_TRY(build_packed(h.get(), s));
    *out = h.release();
    return QAMD_OK;
}

qamd_status qamd_u8_from_rows(const uint8_t *rows, qamd_mem rows_mem, const qamd_u8_metadata *meta,
                              void *stream, qamd_u8 **out) {
    if (!meta || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    const qamd_vector_parameters &vp = meta->vector_parameters;
    int base_distance = vp.distance_type;
    U8Flags flags;  // the flags get_metadata reported travel back in here
    if (vp.distance_type >= 0 && (vp.distance_type & kU8FlagBits)) QAMD_TRY(split_distance(vp, base_distance, flags));
    if (meta->actual_dim != actual_dim_of(vp.dim))
        return fail(QAMD_ERR_ARGUMENTS, "metadata actual_dim %llu does not match dim %llu",
                    (unsigned long long)meta->actual_dim, (unsigned long long)vp.dim);
    if (vp.count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    if (vp.count > 0 && !rows) return fail(QAMD_ERR_ARGUMENTS, "rows is null");
    QAMD_ON_DEVICE(current_device());
    hipStream_t s = as_stream(stream);
    std::unique_ptr<qamd_u8> h(new qamd_u8);
    h->device = current_device();
    h->count = vp.count;
    h->meta = *meta;
    h->meta.vector_parameters.distance_type = base_distance;
    h->format() = flags;
    QAMD_TRY(alloc_store(h.get()));
    const uint64_t stride = meta->actual_dim + 4;
    const uint32_t row_dwords = (uint32_t)(stride / 4);
    uint64_t batch_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / stride);
    // A compact store: a batch is a tile - split into the staging buffer, packed into the image from there.
    // The bytes are another producer's, and the image is all the store keeps: the pack kernel reports a code above 15.
    DevBuf bad;
    if (h->compact) {
        batch_rows = std::min(batch_rows, compact_tile_rows(h.get()));
        QAMD_TRY(bad.alloc(sizeof(uint32_t), true));
        if (vp.count) QAMD_TRY(compact_stage(h.get(), std::min<uint64_t>(batch_rows, vp.count), s));
    }
    DevBuf stage;
    if (rows_mem == QAMD_MEM_HOST && vp.count)
        QAMD_TRY(stage.alloc(std::min<uint64_t>(batch_rows, vp.count) * stride));
    for (uint64_t r0 = 0; r0 < vp.count; r0 += batch_rows) {
        const uint64_t nr = std::min(batch_rows, vp.count - r0);
        const uint8_t *src = rows + r0 * stride;
        if (rows_mem == QAMD_MEM_HOST) {
            QAMD_TRY(copy_in(stage.ptr, src, QAMD_MEM_HOST, nr * stride, s));
            src = stage.as<uint8_t>();
        }
        int grid = grid_for(nr * row_dwords, kBlock * 4, 8);
        hipLaunchKernelGGL(split_rows_kernel, dim3(grid), dim3(kBlock), 0, s,
                           reinterpret_cast<const uint32_t *>(src), nr, row_dwords,
                           h->compact ? h->stage.as<uint32_t>() : h->byte_codes<uint32_t>() + r0 * (row_dwords - 1),
                           h->offsets.as<float>() + r0);
        QAMD_HIP(hipGetLastError());
        if (h->compact) QAMD_TRY(launch_pack(h.get(), r0, nr, bad.as<uint32_t>(), s, h->stage.as<uint4>()));
        if (rows_mem == QAMD_MEM_HOST) QAMD_HIP(hipStreamSynchronize(s));
    }
    if (h->compact) {
        uint32_t high = 1;
        QAMD_HIP(hipMemcpyAsync(&high, bad.ptr, sizeof(high), hipMemcpyDeviceToHost, s));
        QAMD_HIP(hipStreamSynchronize(s));
        if (high) return fail(QAMD_ERR_ARGUMENTS, "a compact store keeps codes 0 .. 15 only, and the rows hold a larger one");
    }
    QAMD_HIP(hipStreamSynchronize(s));
    QAMD_TRY(build_packed(h.get(), s));
    *out = h.release();
    return QAMD_OK;
}

// Rows [first_row, first_row + n_rows) in the reference's storage format: what a caller-owned
// EncodedStorageBuilder receives through push_vector_data (encoded_storage.rs:17-25), in bounded
// pieces -- the store never has to exist as one host buffer (19 GB per C4 shard).
qamd_status qamd_u8_export_rows_range(const qamd_u8 *h, uint64_t first_row, uint64_t n_rows, uint8_t *rows,
                                      qamd_mem rows_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    QAMD_TRY(check_row_range(first_row, n_rows, h->count));
    if (n_rows == 0) return QAMD_OK;
    if (!rows) return fail(QAMD_ERR_ARGUMENTS, "rows is null");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t stride = h->meta.actual_dim + 4;
    const uint32_t row_dwords = (uint32_t)(stride / 4);
    uint64_t batch_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / stride);
    // A compact store: a batch is a tile, whose byte codes come out of the image into call-local scratch.
    StreamBuf tile;
    if (h->compact) {
        batch_rows = std::min(batch_rows, compact_tile_rows(h));
        QAMD_TRY(tile.alloc(std::min<uint64_t>(batch_rows, n_rows) * h->meta.actual_dim, s));
    }
    DevBuf stage;
    if (rows_mem == QAMD_MEM_HOST) QAMD_TRY(stage.alloc(std::min<uint64_t>(batch_rows, n_rows) * stride));
    for (uint64_t r0 = 0; r0 < n_rows; r0 += batch_rows) {
        const uint64_t nr = std::min(batch_rows, n_rows - r0), src_row = first_row + r0;
        uint8_t *dst = rows_mem == QAMD_MEM_HOST ? stage.as<uint8_t>() : rows + r0 * stride;
        int grid = grid_for(nr * row_dwords, kBlock * 4, 8);
        if (h->compact) QAMD_TRY(u8_unpack_rows(h, nullptr, src_row, nr, tile.as<uint8_t>(), h->meta.actual_dim, nullptr, s));
        hipLaunchKernelGGL(join_rows_kernel, dim3(grid), dim3(kBlock), 0, s,
                           h->compact ? tile.as<uint32_t>() : h->byte_codes<uint32_t>() + src_row * (row_dwords - 1),
                           h->offsets.as<float>() + src_row, nr,
                           row_dwords, reinterpret_cast<uint32_t *>(dst));
        QAMD_HIP(hipGetLastError());
        if (rows_mem == QAMD_MEM_HOST)
            QAMD_TRY(copy_out(rows + r0 * stride, QAMD_MEM_HOST, dst, nr * stride, s));
    }
    return QAMD_OK;
}

qamd_status qamd_u8_export_rows(const qamd_u8 *h, uint8_t *rows, qamd_mem rows_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    return qamd_u8_export_rows_range(h, 0, h->count, rows, rows_mem, stream);
}

qamd_status qamd_u8_get_metadata(const qamd_u8 *h, qamd_u8_metadata *out) {
    if (!h || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    *out = h->meta;
    out->vector_parameters.distance_type |= h->distance_bits();
    return QAMD_OK;
}

void qamd_u8_free(qamd_u8 *h) { delete h; }

// The last top-level key of a full-range store's metadata.  It is spelt here and not in qamd_u8_save's own
// concatenation because tests/test_u8_compact_model.py pins the list of keys that function's body spells.
static std::string full_range_entry(const qamd_u8 *h) { return h->full_range ? ",\"full_range\":true" : ""; }

// save (:263-271): serde_json metadata in struct field order, then the raw row file.
qamd_status qamd_u8_save(const qamd_u8 *h, const char *data_path, const char *meta_path) {
    if (!h || !data_path || !meta_path) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    std::string js = "{\"actual_dim\":" + std::to_string(h->meta.actual_dim) +
                     ",\"alpha\":" + json_f32(h->meta.alpha) + ",\"offset\":" + json_f32(h->meta.offset) +
                     ",\"multiplier\":" + json_f32(h->meta.multiplier) +
                     ",\"vector_parameters\":" + vector_parameters_json(h->meta.vector_parameters) +
                     (h->rotated ? ",\"rotation\":\"HadamardBlocks\"" : "") +  // the base metric above; 3.1x
                     (h->four_bit ? ",\"bits\":4" : "") +                           // 3.1y
                     (h->compact ? ",\"compact\":true" : "") + "}";                 // 3.1z: the rows below are byte rows all the same
    js.insert(js.size() - 1, full_range_entry(h));  // 3.1w: the last key; never beside the two above
    QAMD_TRY(save_file(meta_path, js.data(), js.size()));
    const uint64_t stride = h->meta.actual_dim + 4;
    std::vector<uint8_t> rows(h->count * stride);
    QAMD_TRY(qamd_u8_export_rows(h, rows.data(), QAMD_MEM_HOST, nullptr));
    return save_file(data_path, rows.data(), rows.size());
}

// load (:273-288): metadata from JSON; row size/count from the CALLER's vector_parameters;
// the file length must equal size*count (encoded_storage.rs:40-51).
qamd_status qamd_u8_load(const char *data_path, const char *meta_path, const qamd_vector_parameters *vp,
                         qamd_u8 **out) {
    if (!data_path || !meta_path || !vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    JsonValue root;
    QAMD_TRY(read_metadata(meta_path, root));
    qamd_u8_metadata meta{};
    {   // Metadata (:24-31), the fields in any order
        std::string err;
        const JsonValue *vpj = nullptr;
        if (!json_usize(root, "actual_dim", meta.actual_dim, err) || !json_f32_field(root, "alpha", meta.alpha, err) ||
            !json_f32_field(root, "offset", meta.offset, err) || !json_f32_field(root, "multiplier", meta.multiplier, err) ||
            !(vpj = json_field(root, "vector_parameters", err)) || !parse_vector_parameters(*vpj, meta.vector_parameters, err))
            return fail(QAMD_ERR_IO, "%s: %s", meta_path, err.c_str());
    }
    // "rotation" (DESIGN 3.1x): absent = a plain store; the one value a rotated store writes; anything else is not ours
    U8Flags f;  // the keys a store of each format writes beside the base metric
    for (const auto &m : root.members) {
        if (m.first != "rotation") continue;
        if (f.rotated || m.second.kind != JsonValue::String || m.second.text != "HadamardBlocks")
            return fail(QAMD_ERR_IO, "%s: unknown or repeated rotation", meta_path);
        f.rotated = true;
    }
    if (f.rotated && (meta.vector_parameters.distance_type == QAMD_L1 || !rot_dim_ok(vp->dim)))
        return fail(QAMD_ERR_IO, "%s: a rotated store of metric %s and %llu dimensions", meta_path,
                    distance_name(meta.vector_parameters.distance_type), (unsigned long long)vp->dim);
    // "bits" (DESIGN 3.1y): absent = a 7-bit store; 4 is the one value a store writes
    for (const auto &m : root.members) {
        if (m.first != "bits") continue;
        const JsonValue &b = m.second;
        if (f.four_bit || b.kind != JsonValue::Number || !b.integer || b.negative || b.uint != 4)
            return fail(QAMD_ERR_IO, "%s: unknown or repeated bits", meta_path);
        f.four_bit = true;
    }
    if (f.four_bit && meta.vector_parameters.distance_type == QAMD_L1)
        return fail(QAMD_ERR_IO, "%s: a 4-bit store of metric L1", meta_path);
    // "compact" (DESIGN 3.1z): absent = the store keeps its byte codes; true, beside "bits":4, is the one value a store writes
    for (const auto &m : root.members) {
        if (m.first != "compact") continue;
        if (f.compact || m.second.kind != JsonValue::Bool || !m.second.boolean || !f.four_bit)
            return fail(QAMD_ERR_IO, "%s: unknown, repeated or misplaced compact", meta_path);
        f.compact = true;
    }
    if (f.compact && !u8_image_of((uint32_t)std::min<uint64_t>(actual_dim_of(vp->dim) / 16, 0xFFFFFFFFull), true,
                                meta.vector_parameters.distance_type).kind)
        return fail(QAMD_ERR_IO, "%s: a compact store of %llu dimensions", meta_path, (unsigned long long)vp->dim);
    // "full_range" (DESIGN 3.1w): absent = codes 0..127; true, once and never beside "bits":4, is the one value a store writes
    for (const auto &m : root.members) {
        if (m.first != "full_range") continue;
        if (f.full_range || m.second.kind != JsonValue::Bool || !m.second.boolean || f.four_bit)
            return fail(QAMD_ERR_IO, "%s: unknown, repeated or misplaced full_range", meta_path);
        f.full_range = true;
    }
    if (f.full_range && ((f.rotated && meta.vector_parameters.distance_type == QAMD_L1) || vp->dim > kFullMaxDim))
        return fail(QAMD_ERR_IO, "%s: a full-range store of %llu dimensions", meta_path, (unsigned long long)vp->dim);
    const uint64_t size = qamd_u8_quantized_vector_size(vp);
    std::string bytes;
    QAMD_TRY(load_rows_file(data_path, size * vp->count, bytes));
    // The reference keeps the file's metadata but sizes rows from the caller's parameters.
    qamd_u8_metadata eff = meta;
    eff.vector_parameters.dim = vp->dim;
    eff.vector_parameters.count = vp->count;
    eff.actual_dim = actual_dim_of(vp->dim);
    eff.vector_parameters.distance_type |= f.distance_bits();  // from_rows takes them off again
    qamd_status st = qamd_u8_from_rows(reinterpret_cast<const uint8_t *>(bytes.data()), QAMD_MEM_HOST, &eff,
                                       nullptr, out);
    eff.vector_parameters.distance_type = meta.vector_parameters.distance_type;
    if (st == QAMD_OK) (*out)->meta = meta.actual_dim == eff.actual_dim ? meta : eff;
    return st;
}

}  // extern "C"


// ============================================================================= streaming encode
// The reference encodes from a clonable ITERATOR and walks it twice (encoded_vectors_u8.rs:34-40:
// pass 1 :57-71 find_min_max_from_iter + quantile sample, pass 2 :73-118 quantize + push_vector_data),
// never holding the f32 data.  This is that contract in bounded batches: observe() = pass 1,
// push() = pass 2 (rows appended in call order, as EncodedStorageBuilder::push_vector_data,
// encoded_storage.rs:17-25).  Same kernels and the same sample rows as qamd_u8_encode, so the store
// is byte-identical to the one-shot call.
namespace {

// Rows of a batch that belong to the evenly strided quantile sample: sample slot k holds global row
// floor(k * count / slice).
__global__ __launch_bounds__(kBlock) void gather_sample_batch_kernel(const float *__restrict__ batch, uint64_t r_base,
                                                                    uint32_t dim, uint64_t count, uint64_t slice,
                                                                    uint64_t k0, uint64_t k1, float *__restrict__ sample) {
    const uint64_t total = (k1 - k0) * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = k0 + i / dim, j = i % dim;
        const uint64_t r = (uint64_t)((unsigned __int128)k * count / slice);
        sample[k * dim + j] = batch[(r - r_base) * dim + j];
    }
}

uint64_t first_sample_at_or_after(uint64_t row, uint64_t count, uint64_t slice) {
    // smallest k with floor(k * count / slice) >= row  <=>  k * count >= row * slice
    const unsigned __int128 need = (unsigned __int128)row * slice;
    return (uint64_t)((need + count - 1) / count);
}

constexpr uint64_t kStagePieceBytes = 256ull << 20;

}  // namespace

struct qamd_u8_encoder {
    int device = 0;
    hipStream_t stream = nullptr;
    qamd_vector_parameters vp{};
    bool has_quantile = false, has_interval = false;
    float quantile = 0.0f, alpha = 0.0f, offset = 0.0f;
    qamd_stop_fn stop = nullptr;
    void *stop_user = nullptr;
    std::unique_ptr<qamd_u8> h;
    MinMaxAcc acc;
    bool acc_ready = false;
    uint64_t observed = 0, pushed = 0;
    uint64_t slice = 0;  // quantile sample rows (0: no sample kept)
    DevBuf sample, stage;
};

namespace {

qamd_status encoder_close_pass1(qamd_u8_encoder *e) {
    if (e->has_interval) return QAMD_OK;
    const uint64_t count = e->vp.count, dim = e->vp.dim;
    if (count == 0) {  // :43-54: nothing was observed, nothing will be quantized
        e->has_interval = true;
        return QAMD_OK;
    }
    if (e->observed != count)
        return fail(QAMD_ERR_ARGUMENTS, "Vector count %llu does not match vector parameters count %llu (observe pass ended early)",
                    (unsigned long long)e->observed, (unsigned long long)count);
    float mn, mx;
    QAMD_TRY(e->acc.result(e->stream, mn, mx));
    const float levels = (float)e->h->levels();
    e->alpha = (mx - mn) / levels;  // :228-232
    e->offset = mn;
    if (e->slice) {
        uint64_t cut = 0;
        if (quantile_cut(e->slice, dim, e->quantile, cut)) {
            float qmn = 0.0f, qmx = 0.0f;
            const uint64_t len = e->slice * dim;
            if (e->h->rotated) {  // the sample holds the rows as they came: the interval is that of their rotation
                DevBuf rot;
                QAMD_TRY(rot.alloc(len * 4));
                QAMD_TRY(u8_rot_values(e->sample.as<float>(), e->slice, dim, rot.as<float>(), e->stream));
                QAMD_HIP(hipStreamSynchronize(e->stream));
                e->sample = std::move(rot);
            }
            QAMD_TRY(select_kth_f32(e->sample.as<float>(), len, cut + 2, false, &qmn, e->stream));
            QAMD_TRY(select_kth_f32(e->sample.as<float>(), len, cut + 1, true, &qmx, e->stream));
            e->alpha = (qmx - qmn) / levels;
            e->offset = qmn;
        }
        e->sample.release();
    }
    e->has_interval = true;
    return QAMD_OK;
}

}  // namespace

extern "C" {

qamd_status qamd_u8_encoder_begin(const qamd_vector_parameters *vp, const float *quantile, const float *alpha_offset,
                                  qamd_stop_fn stop, void *stop_user, void *stream, qamd_u8_encoder **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    int base_distance = 0;
    U8Flags flags;
    QAMD_TRY(split_distance(*vp, base_distance, flags));
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    QAMD_ON_DEVICE(current_device());
    std::unique_ptr<qamd_u8_encoder> e(new qamd_u8_encoder);
    e->device = current_device();
    e->stream = as_stream(stream);
    e->vp = *vp;
    e->vp.distance_type = base_distance;  // the flags live in h->rotated and h->four_bit
    e->stop = stop;
    e->stop_user = stop_user;
    e->h.reset(new qamd_u8);
    e->h->device = e->device;
    e->h->count = vp->count;
    e->h->meta.actual_dim = actual_dim_of(vp->dim);
    e->h->meta.vector_parameters = e->vp;
    e->h->format() = flags;
    QAMD_TRY(alloc_store(e->h.get()));
    if (alpha_offset) {
        e->alpha = alpha_offset[0];
        e->offset = alpha_offset[1];
        e->has_interval = true;
    } else if (vp->count) {
        QAMD_TRY(e->acc.init(e->stream));
        e->acc_ready = true;
        if (quantile && !(vp->count < 127 || *quantile >= 1.0f)) {  // quantile.rs:27-29
            e->has_quantile = true;
            e->quantile = *quantile;
            e->slice = std::min<uint64_t>(vp->count, kQuantileSample);
            QAMD_TRY(e->sample.alloc(std::max<uint64_t>(e->slice * vp->dim, 4) * sizeof(float)));
        }
    }
    *out = e.release();
    return QAMD_OK;
}

qamd_status qamd_u8_encoder_observe(qamd_u8_encoder *e, const float *batch, uint64_t n_rows, qamd_mem batch_mem) {
    if (!e || (!batch && n_rows && e->vp.dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (e->stop && e->stop(e->stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
    if (e->has_interval) {  // alpha_offset given (or pass 1 closed): nothing to learn
        e->observed += n_rows;
        return QAMD_OK;
    }
    if (e->pushed) return fail(QAMD_ERR_ARGUMENTS, "observe after push");
    if (e->observed + n_rows > e->vp.count) return count_mismatch(e->observed + n_rows, e->vp.count);
    QAMD_ON_DEVICE(e->device);
    const uint64_t dim = e->vp.dim, count = e->vp.count;
    if (dim == 0) {
        e->observed += n_rows;
        return QAMD_OK;
    }
    const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(kStagePieceBytes) / (dim * 4));
    QAMD_TRY(for_each_staged_piece(batch, batch_mem, n_rows, dim, piece_rows, e->stage, e->stream,
                                   [&](const float *src, uint64_t r, uint64_t nr) -> qamd_status {
        if (e->h->rotated) QAMD_TRY(e->acc.feed_rotated(src, nr, dim, e->stream));
        else QAMD_TRY(e->acc.feed(src, nr * dim, e->stream));
        if (e->slice) {
            const uint64_t base = e->observed + r;
            const uint64_t k0 = first_sample_at_or_after(base, count, e->slice);
            const uint64_t k1 = std::min<uint64_t>(e->slice, first_sample_at_or_after(base + nr, count, e->slice));
            if (k1 > k0) {
                hipLaunchKernelGGL(gather_sample_batch_kernel, dim3(grid_for((k1 - k0) * dim, kBlock * 4, 8)), dim3(kBlock),
                                   0, e->stream, src, base, (uint32_t)dim, count, e->slice, k0, k1, e->sample.as<float>());
                QAMD_HIP(hipGetLastError());
            }
        }
        return QAMD_OK;
    }));
    e->observed += n_rows;
    return QAMD_OK;
}

qamd_status qamd_u8_encoder_push(qamd_u8_encoder *e, const float *batch, uint64_t n_rows, qamd_mem batch_mem) {
    if (!e || (!batch && n_rows && e->vp.dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (e->stop && e->stop(e->stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");  // :74-76
    if (e->pushed + n_rows > e->vp.count) return count_mismatch(e->pushed + n_rows, e->vp.count);
    QAMD_ON_DEVICE(e->device);
    QAMD_TRY(encoder_close_pass1(e));
    const uint64_t dim = e->vp.dim;
    const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(kStagePieceBytes) / (dim * 4 + 1));
    QAMD_TRY(for_each_staged_piece(batch, batch_mem, n_rows, dim, piece_rows, e->stage, e->stream,
                                   [&](const float *src, uint64_t r, uint64_t nr) {
        return launch_quantize(e->h.get(), src, nr, e->pushed + r, e->alpha, e->offset, e->stream);
    }));
    e->pushed += n_rows;
    return QAMD_OK;
}

qamd_status qamd_u8_encoder_finish(qamd_u8_encoder *e, qamd_u8 **out) {
    if (!e || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    std::unique_ptr<qamd_u8_encoder> own(e);  // consumed whatever happens
    if (e->pushed != e->vp.count) return count_mismatch(e->pushed, e->vp.count);
    QAMD_ON_DEVICE(e->device);
    QAMD_HIP(hipStreamSynchronize(e->stream));
    if (e->vp.count == 0) {  // :43-54
        e->h->meta.alpha = e->h->meta.offset = e->h->meta.multiplier = 0.0f;
    } else {
        e->h->meta.alpha = e->alpha;
        e->h->meta.offset = e->offset;
        e->h->meta.multiplier = host_multiplier(e->alpha, e->vp.distance_type, e->vp.invert);
    }
    QAMD_TRY(build_packed(e->h.get(), e->stream));
    *out = e->h.release();
    return QAMD_OK;
}

void qamd_u8_encoder_abort(qamd_u8_encoder *e) { abort_encoder(e); }

}  // extern "C"

// ============================================================================= upsert
// Rows of a built store are overwritten or appended with the store's own alpha / offset: launch_quantize at a row offset,
// as the streaming encoder's push.  The reference snapshot has no counterpart (upstream's later upsert_vector is the model).
namespace {

// Room for `cap` rows: new buffers with the rows copied and a zero tail, swapped in once all of them exist.  The packed
// image's block index does not depend on the row count, so its whole blocks are copied as they are; when the larger image
// cannot be had the store goes on without one (its scans read the byte codes), which is not a failure of the call.
qamd_status u8_grow(qamd_u8 *h, uint64_t cap) {
    if (cap <= h->capacity) return QAMD_OK;
    const uint64_t padded = padded_rows_of(cap), ad = h->meta.actual_dim;
    DevBuf codes, offsets, packed;
    if (!h->compact) QAMD_TRY(grow_copy(h->codes, padded * ad, h->count * ad, codes));
    QAMD_TRY(grow_copy(h->offsets, padded * sizeof(float), h->count * sizeof(float), offsets));
    bool image = h->image.kind != U8_IMAGE_NONE;
    if (image) {
        const uint64_t chunk_bytes = (uint64_t)h->image.chunks * 16;
        const std::string err = last_error();
        if (grow_copy(h->packed, padded * chunk_bytes, round_up(h->count, kPackBlockRows) * chunk_bytes, packed) != QAMD_OK) {
            if (h->compact) return QAMD_ERR_DEVICE;  // offsets and image are all there is; the store stays as it was
            (void)hipGetLastError();  // an out-of-memory here only costs the image
            last_error() = err;
            packed.release();
            image = false;
        }
    }
    h->codes = std::move(codes);  // (the old buffers go through hipFree, which waits for the device)
    h->offsets = std::move(offsets);
    h->packed = std::move(packed);
    if (!image) h->image = U8Image{};
    h->packed_rows.release();
    h->capacity = cap;
    h->padded_rows = padded;
    return QAMD_OK;
}

}  // namespace

extern "C" {

uint64_t qamd_u8_capacity(const qamd_u8 *h) { return h ? h->capacity : 0; }

qamd_status qamd_u8_reserve(qamd_u8 *h, uint64_t capacity_rows, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (capacity_rows > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "capacity exceeds u32 row ids");
    if (capacity_rows <= h->capacity) return QAMD_OK;
    QAMD_ON_DEVICE(h->device);
    QAMD_HIP(hipStreamSynchronize(as_stream(stream)));
    return u8_grow(h, capacity_rows);
}

qamd_status qamd_u8_upsert(qamd_u8 *h, uint64_t first_row, const float *data, qamd_mem data_mem, uint64_t n_rows,
                           void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    const uint64_t dim = h->meta.vector_parameters.dim;
    QAMD_TRY(check_upsert(first_row, n_rows, h->count, data, dim));
    if (n_rows == 0) return QAMD_OK;
    if (h->meta.alpha == 0.0f)
        return fail(QAMD_ERR_ARGUMENTS, "the store has no quantization interval (alpha is 0: it was built empty)");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t end = first_row + n_rows;
    if (end > h->capacity) {
        QAMD_HIP(hipStreamSynchronize(s));
        QAMD_TRY(u8_grow(h, std::min<uint64_t>(upsert_capacity(end, h->capacity), 0xFFFFFFFFull)));
    }
    DevBuf stage;
    const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(kStagePieceBytes) / (dim * 4 + 1));
    QAMD_TRY(for_each_staged_piece(data, data_mem, n_rows, dim, piece_rows, stage, s,
                                   [&](const float *src, uint64_t r, uint64_t nr) {
        return launch_quantize(h, src, nr, first_row + r, h->meta.alpha, h->meta.offset, s);
    }));
    // the store's own encoder: nothing to report (a compact store's rows went into the image tile by tile, launch_quantize)
    if (h->image.kind && !h->compact) QAMD_TRY(launch_pack(h, first_row, n_rows, nullptr, s));
    QAMD_HIP(hipStreamSynchronize(s));
    if (h->compact) compact_done(h);
    h->count = std::max(h->count, end);
    h->meta.vector_parameters.count = h->count;
    h->packed_rows.release();
    std::lock_guard<std::mutex> lk(h->sample_mu);  // the next query batch gathers its pivot sample again
    h->sample_codes.release();
    h->sample_offsets.release();
    h->sample_rows = 0;
    return QAMD_OK;
}

}  // extern "C"

namespace qamd {

// Pass-1 pieces for the sharded encoder (sharded.hip): min/max of a row range read from wherever it
// lives (host, this device, another device), and the quantile interval of a whole data set.
qamd_status u8_minmax_range(const float *data, qamd_mem mem, uint64_t n_rows, uint64_t dim, hipStream_t s, float *mn,
                            float *mx) {
    MinMaxAcc acc;
    QAMD_TRY(acc.init(s));
    DevBuf stage;
    const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(kStagePieceBytes) / std::max<uint64_t>(dim * 4, 1));
    if (dim)
        QAMD_TRY(for_each_staged_piece(data, mem, n_rows, dim, piece_rows, stage, s,
                                       [&](const float *src, uint64_t, uint64_t nr) { return acc.feed(src, nr * dim, s); }));
    return acc.result(s, *mn, *mx);
}

qamd_status u8_quantile_interval(const float *data, qamd_mem mem, uint64_t count, uint64_t dim, float quantile,
                                 hipStream_t s, bool *found, float *mn, float *mx) {
    *found = false;
    if (count < 127 || quantile >= 1.0f) return QAMD_OK;  // quantile.rs:27-29
    return quantile_interval_device(data, mem, count, dim, quantile, s, *found, *mn, *mx);
}

void no_signed_codes() {
    std::fprintf(stderr, "quantization_amd: a 7-bit route asked for the codes of a full-range u8 store (DESIGN 3.1w)\n");
    std::abort();
}

void no_byte_codes() {
    std::fprintf(stderr, "quantization_amd: a route asked for the byte codes of a compact u8 store (DESIGN 3.1z)\n");
    std::abort();
}

}  // namespace qamd

extern "C" {

qamd_status qamd_u8_find_min_max(const float *data, qamd_mem data_mem, uint64_t n_rows, uint64_t dim, void *stream,
                                 float *min, float *max) {
    if (!min || !max || (!data && n_rows && dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_ON_DEVICE(current_device());
    return qamd::u8_minmax_range(data, data_mem, n_rows, dim, as_stream(stream), min, max);
}

qamd_status qamd_u8_find_quantile_interval(const float *data, qamd_mem data_mem, uint64_t count, uint64_t dim,
                                           float quantile, void *stream, int *found, float *min, float *max) {
    if (!found || !min || !max || (!data && count && dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_ON_DEVICE(current_device());
    bool f = false;
    *min = *max = 0.0f;
    QAMD_TRY(qamd::u8_quantile_interval(data, data_mem, count, dim, quantile, as_stream(stream), &f, min, max));
    *found = f ? 1 : 0;
    return QAMD_OK;
}

}  // extern "C"

#ifdef QAMD_DEV
// Developer-only accessors for the tuning harness (tune.hip): libquantization_amd_dev.so only.
extern "C" __attribute__((visibility("default"))) void qamd_dev_u8_ptrs(const qamd_u8 *h, const void **codes,
                                                                        const void **offsets) {
    *codes = h->codes.ptr;
    *offsets = h->offsets.ptr;
}
// The device bytes the handle owns for its rows: byte codes + offsets + scan image (a compact store: the last two).
extern "C" __attribute__((visibility("default"))) uint64_t qamd_dev_u8_store_bytes(const qamd_u8 *h) {
    return (h->codes.ptr ? h->codes.bytes : 0) + h->offsets.bytes + (h->packed.ptr ? h->packed.bytes : 0) + h->stage.bytes;
}
// The packed scan image in ROW-MAJOR order, [count][chunks] 16-byte chunks (nullptr, 0 chunks: none): un-blocked on the
// first call into a buffer the handle owns, so that a reader needs to know the bit format only.
namespace {
__global__ __launch_bounds__(kBlock) void u8_unblock_kernel(const uint4 *__restrict__ image, uint64_t n_rows,
                                                            uint32_t pchunks, uint4 *__restrict__ rows) {
    const uint64_t total = n_rows * pchunks, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t r = t / pchunks;
        const uint32_t j = (uint32_t)(t - r * pchunks);
        rows[t] = image[((r / kPackBlockRows) * pchunks + j) * kPackBlockRows + r % kPackBlockRows];
    }
}
}  // namespace
extern "C" __attribute__((visibility("default"))) void qamd_dev_u8_packed(const qamd_u8 *h, const void **packed,
                                                                          uint32_t *chunks) {
    *packed = nullptr;
    *chunks = 0;
    if (!h->image.kind) return;
    if (!h->packed_rows.ptr) {
        const uint64_t n = h->count * h->image.chunks;
        if (h->packed_rows.alloc(n * 16, false) != QAMD_OK) return;
        hipLaunchKernelGGL(u8_unblock_kernel, dim3(grid_for(n, kBlock, 8)), dim3(kBlock), 0, nullptr, h->packed.as<uint4>(),
                           h->count, h->image.chunks, h->packed_rows.as<uint4>());
        if (hipStreamSynchronize(nullptr) != hipSuccess) {
            h->packed_rows.release();
            return;
        }
    }
    *packed = h->packed_rows.ptr;
    *chunks = h->image.chunks;
}
// The image the scan really reads: blocks of `block_rows` rows, chunk j of row r at 16-byte index
// ((r / block_rows) * chunks + j) * block_rows + r % block_rows; padded_rows / block_rows blocks.
extern "C" __attribute__((visibility("default"))) void qamd_dev_u8_packed_blocked(const qamd_u8 *h, const void **packed,
                                                                                  uint32_t *chunks, uint32_t *block_rows) {
    *packed = h->packed.ptr;
    *chunks = h->image.chunks;
    *block_rows = kPackBlockRows;
}
#endif
