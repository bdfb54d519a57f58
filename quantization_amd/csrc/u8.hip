// Scalar u8 quantizer on MI355X (gfx950): encode, query encode, and the query-vs-store scan.
//
// Host class mirrors EncodedVectorsU8 (quantization/src/encoded_vectors_u8.rs); the kernels
// replace the per-pair SIMD FFI (quantization/cpp/avx2.c:25-122) by whole-store launches.
//
// HBM layout (library-owned copy).  The reference row is AoS [vector_offset f32][codes]
// with stride actual_dim+4 (772 B at dim 768: only 4-byte aligned).  On device it is split
// into  codes[count_padded][actual_dim]  (rows 16-byte aligned, contiguous) and
// offsets[count] f32.  Same 772 algorithmic bytes per scored row; every code load is an
// aligned 16-byte `global_load_dwordx4`.  Dot / L2 stores also keep a packed scan image of the
// codes at 7 bits each, in blocks of 64 rows (u8_internal.hpp, build_packed), which their
// single-query scans read with a row per lane (u8_scan_image_kernel<Image7>): 676 instead of 772 bytes
// per row at dim 768.  A 4-bit store (QAMD_BITS4, DESIGN 3.1y: codes 0..15, rounded to nearest) keeps a nibble image in its
// place, two codes per byte, read by the same kernel as Image4: 388 bytes per row.
//
// Scan mapping of the byte codes (HBM-bound integer work, no MFMA): a row is read by G = min(16, pow2(chunks))
// adjacent lanes, 16 B per lane per iteration, so one wave-load covers 64/G consecutive rows
// = fully used 128-B lines.  The query's 16-byte chunks live in VGPRs for the whole kernel.
// v_dot4_u32_u8 accumulates in 32-bit integers (exact), a log2(G)-step cross-lane add
// finishes the row, and the f32 epilogue is evaluated in the reference's order
// ((multiplier*s) + q.offset) + vector_offset  (encoded_vectors_u8.rs:347), no FMA.
//
// Exactness: codes <= 127 => the integer sum is what every reference kernel computes; the
// reference converts lane sums to f32 before adding them (avx2.c:59-62), which is the same
// number whenever the sum is < 2^24 (always for actual_dim <= 1040).  Above that the GPU
// returns the exact integer rounded ONCE to f32 (= the reference's scalar path,
// encoded_vectors_u8.rs:158), or — mode QAMD_U8_LANES_AVX2 — reproduces avx2.c's 8-lane f32
// summation bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "lists.hpp"
#include "multi_reduce.hpp"
#include "topk.hpp"
#include "topk_device.hpp"
#include "rescore.hpp"
#include "rotate_blocks.hpp"
#include "u8_internal.hpp"

#pragma clang fp contract(off)

using namespace qamd;
using namespace qamd::rot;

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 512;  // scan workgroup (tuning sweep: 512 and 1024 tie, 256 is ~1% behind)
constexpr uint64_t kQuantileSample = 100000;  // QUANTILE_SAMPLE_SIZE, quantile.rs:3

enum Epilogue : int { EPI_POINT = 0, EPI_INTERNAL = 1 };

// ------------------------------------------------------------------------------ device helpers
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Streamed-once 16-byte loads: `global_load_dwordx4 ... nt`.
__device__ __forceinline__ uint4 ld_nt(const uint4 *p) {
    u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float4 ld_nt(const float4 *p) {
    f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ uint32_t dot16(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    acc = __builtin_amdgcn_udot4(a.w, b.w, acc, false);
    return acc;
}

__device__ __forceinline__ uint32_t sad16(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc = __builtin_amdgcn_sad_u8(a.x, b.x, acc);
    acc = __builtin_amdgcn_sad_u8(a.y, b.y, acc);
    acc = __builtin_amdgcn_sad_u8(a.z, b.z, acc);
    acc = __builtin_amdgcn_sad_u8(a.w, b.w, acc);
    return acc;
}

// Sum over the G (<= 16) adjacent lanes of a row group, result in every lane.  DPP only
// (quad_perm xor-1 / xor-2, row_half_mirror, row_mirror): four VALU adds for G = 16, instead
// of the ds_bpermute round trips __shfl_xor compiles to.
template <int CTRL> __device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int G> __device__ __forceinline__ uint32_t group_sum(uint32_t v) {
    static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "row group is at most one DPP row");
    if (G >= 2) v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
    if (G >= 4) v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
    if (G >= 8) v = dpp_add<0x141>(v);  // row_half_mirror
    if (G >= 16) v = dpp_add<0x140>(v); // row_mirror
    return v;
}

// encoded_vectors_u8.rs:347 / :409 on the pair sum as an f32 (sf).
__device__ __forceinline__ float epilogue_f(float multiplier, float sf, float q_off, float v_off, float diff, int mode) {
    float ms = multiplier * sf;
    if (mode == EPI_POINT) return (ms + q_off) + v_off;
    return ms + ((q_off + v_off) - diff);
}
// s is the exact integer pair sum (lane mode 0: rounded once).
__device__ __forceinline__ float epilogue(float multiplier, uint32_t s, float q_off, float v_off,
                                          float diff, int mode) {
    return epilogue_f(multiplier, (float)(int32_t)s, q_off, v_off, diff, mode);
}

// Lane mode 1 (avx2.c lane order, any dim): lane k of the reference's 8 x i32 accumulator gets byte pairs p with
// p % 8 == k of every 32-byte block (avx2.c:41-45) and bytes 2k, 2k+1 of a 16-byte tail (:49-58).  A block has 16
// pairs, so in both 16-byte pieces of a block dword j holds pairs that go to lanes 2j (bytes 0, 1) and 2j+1 (bytes
// 2, 3), and so does the tail: eight integer accumulators, acc[2j] += the low-half products of dword j, acc[2j+1] +=
// the high-half ones.
__device__ __forceinline__ void dot16_lanes(const uint4 &v, const uint4 &q, uint32_t (&acc)[8]) {
    const uint32_t vd[4] = {v.x, v.y, v.z, v.w};
    const uint32_t qd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        acc[2 * j] = __builtin_amdgcn_udot4(vd[j], qd[j] & 0x0000FFFFu, acc[2 * j], false);
        acc[2 * j + 1] = __builtin_amdgcn_udot4(vd[j], qd[j] & 0xFFFF0000u, acc[2 * j + 1], false);
    }
}
// Each lane summed over the row group, converted to f32 and added ((l0+l4)+(l2+l6))+((l1+l5)+(l3+l7)) (HSUM256_PS).
template <int G> __device__ __forceinline__ float avx2_lane_sum(uint32_t (&acc)[8]) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) f[k] = (float)(int32_t)group_sum<G>(acc[k]);
    float a0 = f[0] + f[4], a1 = f[1] + f[5], a2 = f[2] + f[6], a3 = f[3] + f[7];
    return (a0 + a2) + (a1 + a3);
}

// encoded_vectors_u8.rs:234-237  ((v-offset)/alpha).clamp(0,127) as u8
__device__ __forceinline__ uint32_t f32_to_u8(float v, float alpha, float offset) {
    float x = (v - offset) / alpha;  // IEEE division (hipcc: correctly rounded f32 divide)
    x = (x < 0.0f) ? 0.0f : x;
    x = (x > 127.0f) ? 127.0f : x;
    return (x != x) ? 0u : (uint32_t)x;
}

// The code of a 4-bit store (the reference has no counterpart): 16 levels, rounded to nearest.  Three f32
// operations, each rounded on its own - subtract, IEEE divide, add (this file is compiled with contraction off) - then the
// clamp and the truncation of f32_to_u8.  NaN gives 0.  No division-free form: every 4-bit encoder takes this one.
__device__ __forceinline__ uint32_t f32_to_u4(float v, float alpha, float offset) {
    float x = (v - offset) / alpha + 0.5f;
    x = (x < 0.0f) ? 0.0f : x;
    x = (x > 15.0f) ? 15.0f : x;
    return (x != x) ? 0u : (uint32_t)x;
}
template <bool FOUR> __device__ __forceinline__ uint32_t f32_to_code(float v, float alpha, float offset) {
    return FOUR ? f32_to_u4(v, alpha, offset) : f32_to_u8(v, alpha, offset);
}
// The same choice at run time (`four` is a kernel argument: wave-uniform), for the kernels where no time is at stake.
__device__ __forceinline__ uint32_t f32_to_code(float v, float alpha, float offset, int four) {
    return four ? f32_to_u4(v, alpha, offset) : f32_to_u8(v, alpha, offset);
}

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

// ------------------------------------------------------------------------------ scan kernel
// One wave covers ONE tile of (64/G)*UNROLL consecutive rows and exits; the grid is one wave
// per tile.  Measured on MI355X (10M x 768, tools/tune_u8.py): this non-persistent form
// streams at 6.5-6.7 TB/s, a persistent grid-stride loop over the same body at 5.9-6.4 —
// workgroups are dispatched in order, so the resident waves always cover one compact, moving
// window of the store.  ITERS = ceil(row_chunks / G).
// EXACT: row_chunks == G*ITERS, so no lane is ever past the row end.  Otherwise loads stay
// unconditional (clamped address + select) so that they still issue back to back.
// FILTER: fused top-k mode — no score is written; rows at least as good as the pivot are
// appended to the candidate buffer (topk_device.hpp).
// EPI (every whole-store kernel below has it): EPI_POINT scores an encoded query; EPI_INTERNAL is score_internal against
// the whole store - the "query" is a stored row (qcodes / q_off_p point into codes / offsets, which are only
// read) and the epilogue takes `diff`.  A compile-time switch: the EPI_POINT code never sees `diff`.
template <int G, int ITERS, int UNROLL, bool IS_L1, bool EXACT, bool FILTER, int EPI = EPI_POINT>
__global__ __launch_bounds__(kScanBlock) void u8_scan_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets,
    const uint4 *__restrict__ qcodes, const float *__restrict__ q_off_p, float multiplier,
    uint32_t n_rows, uint32_t row_chunks, float *__restrict__ out, TopkFilter filt, float diff) {
    constexpr int RW = 64 / G;
    constexpr int TILE = RW * UNROLL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G;
    const int rslot = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    const uint64_t base = wave * TILE;
    if (base >= n_rows) return;

    uint4 v[UNROLL][ITERS];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        const uint64_t row = base + u * RW + rslot;
        const uint4 *p = codes + row * row_chunks;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            if (EXACT) {
                v[u][it] = ld_nt(p + c);
            } else {
                const uint32_t cc = c < row_chunks ? c : row_chunks - 1;
                uint4 t = ld_nt(p + cc);
                const bool in = c < row_chunks;
                v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
        }
    }
    uint4 q[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const uint32_t c = sub + it * G;
        if (EXACT) {
            q[it] = qcodes[c];  // unconditional: no branch around the load
        } else {
            const uint4 t = qcodes[c < row_chunks ? c : row_chunks - 1];
            const bool in = c < row_chunks;
            q[it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
        }
    }
    const float q_off = *q_off_p;
    // Score stores: lane (rslot, sub = u % G) keeps row u's score, so that each group of G
    // tiles rows leaves the wave as ONE store of (64/G)*G = 64 consecutive floats at most —
    // whole 64-byte segments, which is what makes the nontemporal store a win (+2.8 %);
    // nt stores of the 16-byte per-row-group pieces were 15 % slower than plain ones.
    constexpr int NGROUPS = (UNROLL + G - 1) / G;
    float v_off[NGROUPS];
#pragma unroll
    for (int g = 0; g < NGROUPS; g++)  // offsets[] is padded like codes[]: no guard needed
        v_off[g] = offsets[base + (uint64_t)(g * G + sub) * RW + rslot];
    float mine = 0.0f;
    uint32_t pivot = 0;
    if (FILTER) pivot = *filt.pivot_key;
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        uint32_t acc = 0;
#pragma unroll
        for (int it = 0; it < ITERS; it++) acc = IS_L1 ? sad16(v[u][it], q[it], acc) : dot16(v[u][it], q[it], acc);
        acc = group_sum<G>(acc);
        if (sub == (u % G)) mine = epilogue(multiplier, acc, q_off, v_off[u / G], EPI == EPI_POINT ? 0.0f : diff, EPI);
        if ((u % G) == G - 1 || u == UNROLL - 1) {
            constexpr int dummy = 0;
            (void)dummy;
            const int first = (u / G) * G;
            const uint64_t row = base + (uint64_t)(first + sub) * RW + rslot;
            if (sub <= u - first && row < n_rows) {
                if (FILTER) topk_offer(filt, pivot, mine, (uint32_t)row);
                else __builtin_nontemporal_store(mine, out + row);
            }
        }
    }
}

// ------------------------------------------------------------------------------ blocked scan of a scan image
// The scan of a Dot / L2 store that has a scan image (u8_internal.hpp, build_packed): P chunks per row instead of the rc
// chunks of byte codes, in a format IMG (Image7, Image4 below).  Rows lie in blocks of kPackBlockRows = 64: chunk j of
// the 64 rows of block b is the kilobyte at 16-byte index (b * P + j) * 64, one chunk per row.
//
// Mapping: `split` (1, 2, 4, 8) waves per block, lane l owns row 64 * b + l.  Every wave-load is one whole, 1 KB-aligned
// kilobyte (eight 128-byte lines, each requested once); no lane is ever past a row end, so one instantiation serves
// every rc up to 128.  The query chunks of a load are the same for all 64 lanes: they are read at wave-uniform
// addresses (scalar loads through the constant cache) and occupy no vector register.  Same exact integer as the byte
// codes give, added in another order; no cross-lane reduction.  The row is walked in whole groups of IMG::R chunks -
// IMG::init says how many - and then one rest group of the chunks left.  One group (R loads, 4 R VGPRs) is in flight
// per lane: a chunk's registers are refilled from the next group right behind their last use.  8 waves per SIMD; two
// groups in flight do not fit the 64 registers that 8 waves allow.
// split > 1 (stores too small to fill the GPU with one wave per block): the waves of a block take contiguous shares of
// the groups, their partial integer sums meet in LDS behind one barrier and the first wave finishes the rows.
//
// A format carries what differs: R; init(P, aux) -> whole groups; group(qcodes, g) before the R calls full(w, i) of
// whole group g; rest_group(qcodes, c0) before the calls rest(w, c0, i) of the chunks from c0 on; sum().  For the pack
// kernel (u8_pack_image_kernel) it has chunk(), the 16 bytes of image chunk j of a row, which also gathers the bits of
// the code chunks it read, and kNoCode, the bits no code of the format has.
constexpr uint32_t kPackBlockRows = 64;
constexpr uint32_t kPackBlockChunk = kPackBlockRows;  // uint4 between two chunks of one row

__device__ __forceinline__ uint4 and16(const uint4 &v, uint32_t m) { return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m); }
__device__ __forceinline__ uint32_t or16(const uint4 &v) { return v.x | v.y | v.z | v.w; }

// 7-bit image: P = rc - rc / 8 chunks, aux = n_extra = rc / 8.  Chunk j has chunk j's codes in bits 0..6 and, in bit 7,
// bit plane j % 7 of extra chunk P + j / 7 (j < 7 * n_extra); the last rc % 8 chunks carry no plane and are the rest
// group.  A whole group is the 7 chunks that share one extra chunk, so the plane shift is a constant of the unrolled
// group and the extra query chunk is loaded once per group:
//   dot(v & 0x7F.., q_j) + (dot(v & 0x80.., q_extra) >> (7 - j % 7))
// (the second dot is a multiple of 128 << plane).  28 VGPRs in flight, 40 in all.
struct Image7 {
    static constexpr int R = 7;
    static constexpr uint32_t kNoCode = 0x80808080u;
    uint32_t pchunks, acc = 0;
    const uint4 *q;
    uint4 qx;
    __device__ __forceinline__ uint32_t init(uint32_t p, uint32_t n_extra) {
        pchunks = p;
        return n_extra;
    }
    __device__ __forceinline__ void group(const uint4 *qcodes, uint32_t g) {
        q = qcodes + 7 * g;
        qx = qcodes[pchunks + g];
    }
    __device__ __forceinline__ void full(const uint4 &w, int i) {
        acc = dot16(and16(w, 0x7F7F7F7Fu), q[i], acc) + (dot16(and16(w, 0x80808080u), qx, 0) >> (7 - i));
    }
    __device__ __forceinline__ void rest_group(const uint4 *qcodes, uint32_t c0) { q = qcodes + c0; }
    __device__ __forceinline__ void rest(const uint4 &w, uint32_t, int i) { acc = dot16(and16(w, 0x7F7F7F7Fu), q[i], acc); }  // bit 7 is zero
    __device__ __forceinline__ uint32_t sum() const { return acc; }
    static __device__ __forceinline__ uint4 chunk(const uint4 *row, uint32_t j, uint32_t rc, uint32_t p, uint32_t &seen) {
        uint4 w = row[j];
        seen |= or16(w);
        w = and16(w, 0x7F7F7F7Fu);
        if (j < 7 * (rc - p)) {
            const uint4 x = row[p + j / 7];
            const uint32_t b = j % 7;
            seen |= or16(x);
            w = make_uint4(w.x | ((x.x >> b) & 0x01010101u) << 7, w.y | ((x.y >> b) & 0x01010101u) << 7,
                           w.z | ((x.z >> b) & 0x01010101u) << 7, w.w | ((x.w >> b) & 0x01010101u) << 7);
        }
        return w;
    }
};

// Nibble image of a 4-bit store: P = ceil(rc / 2) chunks, aux = rc.  Byte b of chunk j =
// codes[32 j + b] | codes[32 j + 16 + b] << 4.  Per image chunk
//   lo += dot(v & 0x0F.., q[2j]),  hi += dot(v & 0xF0.., q[2j + 1])
// and the row's sum is lo + (hi >> 4): hi is a multiple of 16 and at most 240 * 15 * 2048 < 2^23, so the shift is
// exact and happens once per wave.  The n_full = rc / 2 chunks with two code chunks each are walked in groups of R;
// what is left - fewer than R full chunks and, for an odd rc, the last chunk, whose high nibbles are zero and whose
// second query chunk does not exist and is not read - is the rest group.  R = 8: 32 VGPRs in flight, 45 in all (DESIGN
// 3.1y has the compiler's resource report).
struct Image4 {
    static constexpr int R = 8;
    static constexpr uint32_t kNoCode = 0xF0F0F0F0u;
    uint32_t n_full, lo = 0, hi = 0;
    const uint4 *q;
    __device__ __forceinline__ uint32_t init(uint32_t, uint32_t row_chunks) {
        n_full = row_chunks / 2;
        return n_full / R;
    }
    __device__ __forceinline__ void group(const uint4 *qcodes, uint32_t g) { q = qcodes + 2 * R * g; }
    __device__ __forceinline__ void full(const uint4 &w, int i) {
        lo = dot16(and16(w, 0x0F0F0F0Fu), q[2 * i], lo);
        hi = dot16(and16(w, 0xF0F0F0F0u), q[2 * i + 1], hi);
    }
    __device__ __forceinline__ void rest_group(const uint4 *qcodes, uint32_t c0) { q = qcodes + 2 * c0; }
    __device__ __forceinline__ void rest(const uint4 &w, uint32_t c0, int i) {
        lo = dot16(and16(w, 0x0F0F0F0Fu), q[2 * i], lo);
        if (c0 + i < n_full) hi = dot16(and16(w, 0xF0F0F0F0u), q[2 * i + 1], hi);
    }
    __device__ __forceinline__ uint32_t sum() const { return lo + (hi >> 4); }
    static __device__ __forceinline__ uint4 chunk(const uint4 *row, uint32_t j, uint32_t rc, uint32_t, uint32_t &seen) {
        const uint4 a = row[2 * j];
        const uint4 b = 2 * j + 1 < rc ? row[2 * j + 1] : make_uint4(0, 0, 0, 0);
        seen |= or16(a) | or16(b);
        return make_uint4((a.x & 0x0F0F0F0Fu) | ((b.x & 0x0F0F0F0Fu) << 4), (a.y & 0x0F0F0F0Fu) | ((b.y & 0x0F0F0F0Fu) << 4),
                          (a.z & 0x0F0F0F0Fu) | ((b.z & 0x0F0F0F0Fu) << 4), (a.w & 0x0F0F0F0Fu) | ((b.w & 0x0F0F0F0Fu) << 4));
    }
};

template <class IMG, bool FILTER, int EPI = EPI_POINT>
__global__ __launch_bounds__(kScanBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void u8_scan_image_kernel(
    const uint4 *__restrict__ image, const float *__restrict__ offsets, const uint4 *__restrict__ qcodes,
    const float *__restrict__ q_off_p, float multiplier, uint32_t n_rows, uint32_t pchunks, uint32_t aux,
    uint32_t split, float *__restrict__ out, TopkFilter filt, float diff) {
    constexpr int R = IMG::R;
    __shared__ uint32_t partial[kScanBlock];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t part = wave & (split - 1);
    const uint64_t block = (uint64_t)blockIdx.x * ((kScanBlock / 64) / split) + wave / split;
    const uint64_t row = block * kPackBlockRows + lane;
    const bool live = block * kPackBlockRows < n_rows;  // wave-uniform; offsets[] and the image are padded past every block
    // the groups of a row: n_ring whole groups of R chunks, then one of the n_rest chunks left
    IMG img;
    const uint32_t n_ring = img.init(pchunks, aux), n_rest = pchunks - R * n_ring, n_groups = n_ring + (n_rest ? 1 : 0);
    const uint32_t g_begin = live ? n_groups * part / split : 0, g_end = live ? n_groups * (part + 1) / split : 0;
    // chunk c of the block: a wave-uniform base plus the lane's 16 bytes
    const uint4 *blk = image + block * pchunks * kPackBlockChunk;
    const uint32_t lane16 = lane * 16;
    auto chunk_ptr = [&](uint32_t c) {
        return reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(blk + (uint64_t)c * kPackBlockChunk) + lane16);
    };
    // this wave's whole groups [g_begin, gf_end) and whether the rest group is in its share
    const uint32_t gf_end = g_end < n_ring ? g_end : n_ring;
    const bool has_rest = g_end > n_ring;

    uint4 v[R];
    // adds whole group g, held in v; REFILL: each chunk's registers are reloaded from group g + 1 behind their last use
    auto eat = [&](uint32_t g, auto refill) {
        img.group(qcodes, g);
#pragma unroll
        for (int i = 0; i < R; i++) {
            img.full(v[i], i);
            if (decltype(refill)::value) {  // pinned here, so that the load reuses the chunk's registers
                __builtin_amdgcn_sched_barrier(0);
                v[i] = ld_nt(chunk_ptr(R * (g + 1) + i));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (g_begin < gf_end) {
#pragma unroll
        for (int i = 0; i < R; i++) v[i] = ld_nt(chunk_ptr(R * g_begin + i));
    }
    const float v_off = offsets[row];
    const float q_off = *q_off_p;
    uint32_t pivot = 0;
    if (FILTER) pivot = *filt.pivot_key;
    if (g_begin < gf_end) {
        for (uint32_t g = g_begin; g + 1 < gf_end; g++) eat(g, std::true_type{});
        eat(gf_end - 1, std::false_type{});
    }
    if (has_rest) {
        const uint32_t c0 = R * n_ring;
        img.rest_group(qcodes, c0);
#pragma unroll
        for (int i = 0; i < R; i++)
            if ((uint32_t)i < n_rest) v[i] = ld_nt(chunk_ptr(c0 + i));
#pragma unroll
        for (int i = 0; i < R; i++)
            if ((uint32_t)i < n_rest) img.rest(v[i], c0, i);
    }
    uint32_t acc = img.sum();
    if (split > 1) {
        partial[threadIdx.x] = acc;
        __syncthreads();
        if (part == 0)
            for (uint32_t p = 1; p < split; p++) acc += partial[threadIdx.x + 64 * p];
    }
    if (part == 0 && row < n_rows) {
        const float score = epilogue(multiplier, acc, q_off, v_off, EPI == EPI_POINT ? 0.0f : diff, EPI);
        if (FILTER) topk_offer(filt, pivot, score, (uint32_t)row);
        else __builtin_nontemporal_store(score, out + row);
    }
}

// NQ (2, 4, 8) queries per row read on the vector ALU -- the route of qamd_u8_topk_batch /
// score_batch for a handful of queries over a large store, where the matrix-core kernel is bound
// by what its LDS-DMA path moves (4.6 TB/s of row bytes: 1.67 ms per 10M x 768 whatever the batch)
// while this one streams the rows like the single-query scan: the row's 16-byte pieces are loaded
// once (nt) and v_dot4'd against NQ query rows held in registers (NQ * ITERS * 4 VGPRs).  Lane
// (row slot, sub = j) keeps query j's score of the row.  Same integer sum and the same f32
// epilogue as u8_scan_kernel => the same score bits.  G >= NQ.
// FILTER: no score is written; the lane offers its row to query j's candidate lists (slices).
// EPI_INTERNAL: the "queries" are stored rows gathered into a [NQ][q_pitch] block with their stored offsets
// (u8_gather_rows_kernel), the epilogue is score_internal's; `diff` is wave-uniform and used after the row loop's sums only.
template <int G, int ITERS, int UNROLL, int NQ, bool IS_L1, bool EXACT, bool FILTER, int EPI = EPI_POINT>
__global__ __launch_bounds__(kScanBlock) void u8_scan_multi_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets, const uint8_t *__restrict__ qcodes,
    uint32_t q_pitch, const float *__restrict__ q_offs, uint32_t nq_valid /* <= NQ: queries really there */,
    float multiplier, uint32_t n_rows, uint32_t row_chunks, float *__restrict__ out /* [NQ][out_pitch] */,
    uint64_t out_pitch, TopkFilterSlices slices, float diff) {
    static_assert(G >= NQ, "one lane of the row group per query");
    constexpr int RW = 64 / G;
    constexpr int TILE = RW * UNROLL;
    // A wave walks kMultiTiles consecutive tiles: the NQ query rows (NQ * ITERS 16-byte loads per lane)
    // are fetched once per wave, so they must be amortised over more rows than one tile holds
    // (with one tile per wave the query loads were as many bytes as the rows themselves).
    constexpr int TPW = NQ;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    if (wave * TILE * TPW >= n_rows) return;
    uint4 q[NQ][ITERS];
#pragma unroll
    for (int j = 0; j < NQ; j++) {  // an unused slot (3 queries in a 4-wide pass) re-reads the last query
        const uint4 *qj = reinterpret_cast<const uint4 *>(qcodes + (size_t)((uint32_t)j < nq_valid ? j : nq_valid - 1) * q_pitch);
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            const bool in = EXACT || c < row_chunks;
            const uint4 t = qj[in ? c : row_chunks - 1];
            q[j][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
        }
    }
    // lane (row slot, sub) ends up with the total of query multi_query_of<NQ>(sub) (multi_reduce.hpp)
    const int my_q = multi_query_of<NQ>(sub);
    const bool owner = sub < NQ && (uint32_t)my_q < nq_valid;
    const float q_off = q_offs[owner ? my_q : 0];
    for (int tile = 0; tile < TPW; tile++) {
        const uint64_t base = (wave * TPW + tile) * TILE;
        if (base >= n_rows) break;
        uint4 v[UNROLL][ITERS];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint4 *p = codes + (base + u * RW + rslot) * row_chunks;  // rows are padded: no guard
#pragma unroll
            for (int it = 0; it < ITERS; it++) {
                const uint32_t c = sub + it * G;
                const bool in = EXACT || c < row_chunks;
                const uint4 t = ld_nt(p + (in ? c : row_chunks - 1));
                v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint64_t row = base + (uint64_t)u * RW + rslot;
            const float v_off = offsets[row];  // padded like codes[]
            uint32_t acc[NQ];
#pragma unroll
            for (int j = 0; j < NQ; j++) {
                acc[j] = 0;
#pragma unroll
                for (int it = 0; it < ITERS; it++)
                    acc[j] = IS_L1 ? sad16(v[u][it], q[j][it], acc[j]) : dot16(v[u][it], q[j][it], acc[j]);
            }
            const float mine = epilogue(multiplier, multi_reduce<G, NQ>(acc, sub), q_off, v_off, EPI == EPI_POINT ? 0.0f : diff, EPI);
            if (owner && row < n_rows) {
                if (FILTER) {
                    const TopkFilter f = topk_filter_of(slices, (uint32_t)my_q);
                    topk_offer(f, *f.pivot_key, mine, (uint32_t)row);
                } else {
                    __builtin_nontemporal_store(mine, out + (uint64_t)my_q * out_pitch + row);
                }
            }
        }
    }
}

// Single-launch top-k for small stores (topk.hpp small_topk): workgroup b scores rows
// [b * rows_per_wg, (b + 1) * rows_per_wg) exactly like u8_scan_kernel (same loads, same integer
// sum, same f32 epilogue => the same score bits), but a score never goes to HBM: it becomes a
// 64-bit key (order-preserving score bits << 32 | row) in the wave's LDS staging row, and the wave /
// workgroup / last-arriver merges of topk_device.hpp keep the best k.  100k x 768: one launch
// replaces the sample / pivot / filtering-scan / sort chain (66 us).
// The body, given the query's pieces in registers (q) and its offset:
template <int G, int ITERS, bool IS_L1, bool EXACT, int EPI = EPI_POINT>
__device__ __forceinline__ void u8_topk_small_body(const uint4 *__restrict__ codes, const float *__restrict__ offsets,
                                                   const uint4 (&q)[ITERS], float q_off, float multiplier, uint32_t n_rows,
                                                   uint32_t row_chunks, uint32_t rows_per_wg, const SmallTopk &p,
                                                   unsigned long long (*lds)[64], float diff = 0.0f) {
    unsigned long long(*lists)[64] = lds;
    constexpr int RW = 64 / G;
    constexpr int UNROLL = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % G, rslot = lane / G;
    unsigned long long *stage = lds[kSmallTopkWaves + wave];
    const uint64_t wg_base = (uint64_t)blockIdx.x * rows_per_wg;
    SmallTopkWave acc_list;
    for (uint32_t tile = wave * UNROLL; tile * RW < rows_per_wg; tile += kSmallTopkWaves * UNROLL) {
        uint4 v[UNROLL][ITERS];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            // rows past the workgroup's range or the store still load from a valid address
            const uint64_t row = wg_base + (uint64_t)(tile + u) * RW + rslot;
            const uint64_t rc = row < n_rows ? row : (uint64_t)n_rows - 1;
            const uint4 *src = codes + rc * row_chunks;
#pragma unroll
            for (int it = 0; it < ITERS; it++) {
                const uint32_t c = sub + it * G;
                const uint4 t = ld_nt(src + ((EXACT || c < row_chunks) ? c : row_chunks - 1));
                const bool in = EXACT || c < row_chunks;
                v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint32_t local = (tile + u) * RW + rslot;
            const uint64_t row = wg_base + local;
            uint32_t acc = 0;
#pragma unroll
            for (int it = 0; it < ITERS; it++) acc = IS_L1 ? sad16(v[u][it], q[it], acc) : dot16(v[u][it], q[it], acc);
            acc = group_sum<G>(acc);
            if (sub == 0) {
                unsigned long long key = ~0ull;
                if (local < rows_per_wg && row < n_rows) {
                    const float sc = epilogue(multiplier, acc, q_off, offsets[row], EPI == EPI_POINT ? 0.0f : diff, EPI);
                    key = ((unsigned long long)topk_ordered_bits(sc, p.largest != 0) << 32) | (uint32_t)row;
                }
                stage[acc_list.fill + rslot] = key;
            }
            acc_list.fill += RW;
            if (acc_list.fill == 64) small_topk_flush(acc_list, stage, lane);
        }
    }
    if (acc_list.fill) small_topk_flush(acc_list, stage, lane);
    small_topk_finish(acc_list.best, lists, p);
}

template <int G, int ITERS, bool IS_L1, bool EXACT, int EPI = EPI_POINT>
__global__ __launch_bounds__(1024) void u8_topk_small_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets, const uint4 *__restrict__ qcodes,
    const float *__restrict__ q_off_p, float multiplier, uint32_t n_rows, uint32_t row_chunks, uint32_t rows_per_wg,
    SmallTopk p, float diff) {
    __shared__ unsigned long long lds[2 * kSmallTopkWaves][64];  // [0, 16): tournament lists, [16, 32): staging rows
    const int lane = threadIdx.x & 63, sub = lane % G;
    uint4 q[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const uint32_t c = sub + it * G;
        const uint4 t = qcodes[(EXACT || c < row_chunks) ? c : row_chunks - 1];
        const bool in = EXACT || c < row_chunks;
        q[it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
    }
    u8_topk_small_body<G, ITERS, IS_L1, EXACT, EPI>(codes, offsets, q, *q_off_p, multiplier, n_rows, row_chunks, rows_per_wg, p,
                                                    lds, diff);
}

// encode_query FOLDED INTO the single-launch top-k: one launch per search on a small store.  The f32
// query arrives BY VALUE in the kernel arguments (<= 896 values: the argument block is 4 KiB), so no
// copy call, no mapped-memory read over PCIe and no second, dependent launch stands in front of the
// scan.  Every workgroup quantises the query itself -- thread t makes dword t of the codes with the
// encoder's own f32_to_u8 and padding (encoded_vectors_u8.rs:290-329), the code sums are exact
// integers (127^2 * 896 < 2^24), the offset is formed in the reference's order -- keeps the codes in
// LDS, and goes on as u8_topk_small_kernel: same codes and offset => the same score bits.  Workgroup 0
// also leaves offset + codes in the query object's buffer, so after this launch the object is an
// ordinary encoded query for whoever uses it next.
constexpr uint32_t kFusedQueryDims = 896;
struct QueryByValue {
    float v[kFusedQueryDims];
};
template <int G, int ITERS, bool IS_L1, bool EXACT>
__global__ __launch_bounds__(1024) void u8_topk_small_fused_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets, const QueryByValue qv, uint32_t qdim,
    uint32_t actual_dim, float alpha, float offset, int distance, int invert, uint8_t *__restrict__ qbuf, float multiplier,
    uint32_t n_rows, uint32_t row_chunks, uint32_t rows_per_wg, SmallTopk p) {
    __shared__ unsigned long long lds[2 * kSmallTopkWaves][64];
    __shared__ __attribute__((aligned(16))) uint32_t qc_lds[kFusedQueryDims / 4];
    __shared__ uint32_t qsum[2];
    const uint32_t t = threadIdx.x;
    const int lane = threadIdx.x & 63, sub = lane % G;
    if (t < 2) qsum[t] = 0;
    __syncthreads();
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_u8(placeholder, alpha, offset);
    uint32_t s1 = 0, s2 = 0;
    if (t < actual_dim / 4) {
        uint32_t packed = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t j = 4 * t + b;
            const uint32_t c = j < qdim ? f32_to_u8(qv.v[j], alpha, offset) : pad_code;
            packed |= c << (8 * b);
            s1 += c;
            s2 += c * c;
        }
        qc_lds[t] = packed;
    }
    if (t < 256) {  // actual_dim / 4 <= 224: the first four waves hold everything
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            s1 += __shfl_xor(s1, m, 64);
            s2 += __shfl_xor(s2, m, 64);
        }
        if (lane == 0) {
            atomicAdd(&qsum[0], s1);
            atomicAdd(&qsum[1], s2);
        }
    }
    __syncthreads();
    float q_off;
    if (distance == QAMD_DOT) q_off = (float)qsum[0] * alpha * offset;
    else if (distance == QAMD_L1) q_off = 0.0f;
    else q_off = (float)qsum[1] * alpha * alpha;
    if (invert) q_off = -q_off;
    if (blockIdx.x == 0) {  // the query object becomes an encoded query (layout: encode_query_kernel)
        if (t == 0) *reinterpret_cast<float *>(qbuf) = q_off;
        if (t < actual_dim / 4) reinterpret_cast<uint32_t *>(qbuf + 16)[t] = qc_lds[t];
    }
    uint4 q[ITERS];
    const uint4 *qc4 = reinterpret_cast<const uint4 *>(qc_lds);
#pragma unroll
    for (int it = 0; it < ITERS; it++) {
        const uint32_t c = sub + it * G;
        const uint4 v = qc4[(EXACT || c < row_chunks) ? c : row_chunks - 1];
        const bool in = EXACT || c < row_chunks;
        q[it] = make_uint4(in ? v.x : 0, in ? v.y : 0, in ? v.z : 0, in ? v.w : 0);
    }
    u8_topk_small_body<G, ITERS, IS_L1, EXACT>(codes, offsets, q, q_off, multiplier, n_rows, row_chunks, rows_per_wg, p, lds);
}

// Generic dims (row_chunks > 16*8): runtime chunk loop, query re-read through L1/L2.
template <bool IS_L1, int EPI = EPI_POINT>
__global__ __launch_bounds__(kBlock) void u8_scan_generic_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets,
    const uint4 *__restrict__ qcodes, const float *__restrict__ q_off_p, float multiplier,
    uint32_t n_rows, uint32_t row_chunks, float *__restrict__ out, float diff) {
    constexpr int G = 16, RW = 4;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * kBlock) >> 6;
    const float q_off = *q_off_p;
    for (uint64_t base = (uint64_t)wave * RW; base < n_rows; base += (uint64_t)n_waves * RW) {
        const uint64_t row = base + rslot;
        const uint4 *p = codes + row * row_chunks;
        uint32_t acc = 0;
        for (uint32_t c = sub; c < row_chunks; c += G) {
            uint4 v = ld_nt(p + c);
            uint4 qv = qcodes[c];
            acc = IS_L1 ? sad16(v, qv, acc) : dot16(v, qv, acc);
        }
        acc = group_sum<G>(acc);
        if (sub == 0 && row < n_rows)
            out[row] = epilogue(multiplier, acc, q_off, offsets[row], EPI == EPI_POINT ? 0.0f : diff, EPI);
    }
}

// Lane mode 1 scan (any dim): dot16_lanes / avx2_lane_sum, the scan's epilogue on that f32 sum.
template <bool DUMMY, int EPI = EPI_POINT>
__global__ __launch_bounds__(kBlock) void u8_scan_avx2_lanes_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets,
    const uint4 *__restrict__ qcodes, const float *__restrict__ q_off_p, float multiplier,
    uint32_t n_rows, uint32_t row_chunks, float *__restrict__ out, float diff) {
    constexpr int G = 16, RW = 4;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * kBlock) >> 6;
    const float q_off = *q_off_p;
    for (uint64_t base = (uint64_t)wave * RW; base < n_rows; base += (uint64_t)n_waves * RW) {
        const uint64_t row = base + rslot;
        const uint4 *p = codes + row * row_chunks;
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c = sub; c < row_chunks; c += G) dot16_lanes(ld_nt(p + c), qcodes[c], acc);
        const float s = avx2_lane_sum<G>(acc);
        if (sub == 0 && row < n_rows)
            out[row] = epilogue_f(multiplier, s, q_off, offsets[row], EPI == EPI_POINT ? 0.0f : diff, EPI);
    }
}

// Random access: out[k] = score(query of pair k, ids[k]).  One 16-lane group per pair; ITERS =
// ceil(row_chunks / 16) is a template parameter so that all of a row's 16-byte pieces (and the query's)
// are in flight at once with no clamped duplicate loads (ITERS = 0: any row length, four-deep batches).
// Which query a pair is scored against:
//   lists == nullptr            one query for every pair (score_ids): q_single / q_off_single, which
//                               may point into the store itself (score_internal: "query" = row i);
//   lists, list_rows == nullptr query l of a batch for the pairs of list l (score_ids_batch);
//   lists, list_rows            stored row list_rows[l] for the pairs of list l (score_internal_ids_batch).
// A workgroup takes `pairs_per_block` consecutive pairs; with lists it finds the list of its first pair
// by ONE binary search (thread 0, through LDS) and every group then walks forward from there as its
// pair index grows -- a binary search per pair was ten dependent loads in front of every row fetch
// (1M random pairs: 0.26 ms; this form: profiles/r03_bursts.jsonl).
// Same integer sum and the same f32 epilogue as the scan => the same score bits.  LANES (lane mode 1, Dot / L2, any
// row length through ITERS = 0): the lane-mode-1 scan's arithmetic instead (dot16_lanes, avx2_lane_sum, epilogue_f),
// so score_internal's `diff` epilogue is unchanged.
template <bool IS_L1, int ITERS, bool LANES = false>
__global__ __launch_bounds__(kBlock) void u8_score_pairs_kernel(
    const uint4 *__restrict__ codes, const float *__restrict__ offsets, const uint4 *q_single, const float *q_off_single,
    const uint8_t *__restrict__ q_batch, uint32_t q_pitch, const float *__restrict__ q_offs,
    const uint32_t *__restrict__ lists, uint32_t n_lists, const uint32_t *__restrict__ list_rows, float multiplier,
    float diff, int mode, const uint32_t *__restrict__ ids, uint64_t n_ids, uint32_t n_rows, uint32_t row_chunks,
    uint32_t pairs_per_block, float *__restrict__ out) {
    static_assert(!LANES || ITERS == 0, "the lane-order form is the any-length loop");
    constexpr int G = 16, GROUPS = kBlock / G;
    __shared__ uint32_t first_list;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, group = threadIdx.x / G;
    const uint64_t p0 = (uint64_t)blockIdx.x * pairs_per_block;
    const uint64_t p1 = p0 + pairs_per_block < n_ids ? p0 + pairs_per_block : n_ids;
    uint32_t l = lists ? first_list_of_block(lists, n_lists, p0, &first_list) : 0u;
    const float q_off_one = lists ? 0.0f : *q_off_single;
    for (uint64_t k = p0 + group; k < p1; k += GROUPS) {
        const uint32_t row = ids[k];
        bool ok = row < n_rows;
        const uint4 *qp = q_single;
        float q_off = q_off_one;
        if (lists) {
            l = advance_list(lists, n_lists, l, k);  // the pair index only grows: a step or two
            if (list_rows) {
                const uint32_t qr = list_rows[l];
                ok = ok && qr < n_rows;
                const uint32_t qc = qr < n_rows ? qr : 0u;
                qp = codes + (uint64_t)qc * row_chunks;
                q_off = offsets[qc];
            } else {
                qp = reinterpret_cast<const uint4 *>(q_batch + (size_t)l * q_pitch);
                q_off = q_offs[l];
            }
        }
        const uint4 *p = codes + (uint64_t)(ok ? row : 0u) * row_chunks;
        uint32_t acc = 0;
        if (ITERS > 0) {
            uint4 v[ITERS > 0 ? ITERS : 1], qv[ITERS > 0 ? ITERS : 1];
#pragma unroll
            for (int j = 0; j < ITERS; j++) {
                const uint32_t c = sub + j * G, cc = c < row_chunks ? c : row_chunks - 1;  // only the last piece can be clamped
                v[j] = p[cc];
                qv[j] = qp[cc];
            }
#pragma unroll
            for (int j = 0; j < ITERS; j++)
                if (j + 1 < ITERS || sub + j * G < row_chunks) acc = IS_L1 ? sad16(v[j], qv[j], acc) : dot16(v[j], qv[j], acc);
        } else {
            uint32_t lanes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t c0 = sub; c0 < row_chunks; c0 += 4 * G) {
                uint4 v[4], qv[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {  // unconditional loads (clamped address): all four issue back to back
                    const uint32_t c = c0 + j * G, cc = c < row_chunks ? c : row_chunks - 1;
                    v[j] = p[cc];
                    qv[j] = qp[cc];
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (c0 + j * G >= row_chunks) continue;
                    if constexpr (LANES) dot16_lanes(v[j], qv[j], lanes);
                    else acc = IS_L1 ? sad16(v[j], qv[j], acc) : dot16(v[j], qv[j], acc);
                }
            }
            if constexpr (LANES) {
                static_assert(!IS_L1, "lane mode 1 changes Dot and L2 only");
                const float s = avx2_lane_sum<G>(lanes);
                if (sub == 0) out[k] = ok ? epilogue_f(multiplier, s, q_off, offsets[row], diff, mode) : __builtin_nanf("");
                continue;
            }
        }
        acc = group_sum<G>(acc);
        if (sub == 0) out[k] = ok ? epilogue(multiplier, acc, q_off, offsets[row], diff, mode) : __builtin_nanf("");
    }
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
          bool FOUR = false /* 4-bit codes (f32_to_u4); never FAST */>
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
    const uint32_t pad_code = f32_to_code<FOUR>(placeholder, alpha, offset);
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
                    packed = f32_to_code<FOUR>(f[j].x, alpha, offset) | (f32_to_code<FOUR>(f[j].y, alpha, offset) << 8) |
                             (f32_to_code<FOUR>(f[j].z, alpha, offset) << 16) | (f32_to_code<FOUR>(f[j].w, alpha, offset) << 24);
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
                    sum += (float)(j < dim ? f32_to_code<FOUR>(src[j], alpha, offset) : pad_code);
            }
            vo = D * offset * offset + sum * alpha * offset;
        } else if (distance == QAMD_L1) {
            vo = 0.0f;
        } else {
            float sum = (float)s2;
            if (s2 >= (1u << 24)) {
                sum = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    const float c = (float)(j < dim ? f32_to_code<FOUR>(src[j], alpha, offset) : pad_code);
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
    float *__restrict__ offsets, uint64_t row0, int four) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, four);
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
                uint32_t c = j < dim ? f32_to_code(src[j], alpha, offset, four) : pad_code;
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
                        s += (float)(j < dim ? f32_to_code(src[j], alpha, offset, four) : pad_code);
                }
                vo = D * offset * offset + s * alpha * offset;
            } else if (distance == QAMD_L1) {
                vo = 0.0f;
            } else {
                float s = (float)s2;
                if (s2 >= (1u << 24)) {
                    s = 0.0f;
                    for (uint32_t j = 0; j < actual_dim; j++) {
                        float c = (float)(j < dim ? f32_to_code(src[j], alpha, offset, four) : pad_code);
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
__device__ __forceinline__ uint32_t rot_quant4(const float (&v)[4], float alpha, float offset, float r_alpha, int fast) {
    const float4 f = make_float4(v[0], v[1], v[2], v[3]);
    if (fast == kQuant4Bit)  // a 4-bit store; wave-uniform
        return f32_to_u4(f.x, alpha, offset) | (f32_to_u4(f.y, alpha, offset) << 8) | (f32_to_u4(f.z, alpha, offset) << 16) |
               (f32_to_u4(f.w, alpha, offset) << 24);
    if (fast) return f32x4_to_u8x4_fast(f, alpha, offset, r_alpha);
    return f32_to_u8(f.x, alpha, offset) | (f32_to_u8(f.y, alpha, offset) << 8) | (f32_to_u8(f.z, alpha, offset) << 16) |
           (f32_to_u8(f.w, alpha, offset) << 24);
}
// vector_offset of a row from its code sums (quantize16_kernel's epilogue; s1 <= 127 * 16384 < 2^24 always).  `sum2` is
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

// encode_query on device (encoded_vectors_u8.rs:290-329): one wave.
// qbuf: [0] offset f32, [16..] codes.
__global__ __launch_bounds__(64) void encode_query_kernel(const float *__restrict__ query,
                                                         uint32_t qdim, uint32_t actual_dim,
                                                         float alpha, float offset, int distance,
                                                         int invert, uint8_t *__restrict__ qbuf, int four) {
    const int lane = threadIdx.x;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, four);
    uint8_t *codes = qbuf + 16;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t j = lane; j < actual_dim; j += 64) {
        uint32_t c = j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code;
        codes[j] = (uint8_t)c;
        s1 += c;
        s2 += c * c;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
    }
    if (lane == 0) {
        float off;
        if (distance == QAMD_DOT) {
            float s = (float)s1;
            if (s1 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++)
                    s += (float)(j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code);
            }
            off = s * alpha * offset;
        } else if (distance == QAMD_L1) {
            off = 0.0f;
        } else {
            float s = (float)s2;
            if (s2 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    float c = (float)(j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code);
                    s += c * c;
                }
            }
            off = s * alpha * alpha;
        }
        *reinterpret_cast<float *>(qbuf) = invert ? -off : off;
    }
}

// Batch form of encode_query_kernel: one wave per query, separate code / offset arrays
// (the layout the multi-query MFMA path reads, u8_batch.hip).
__global__ __launch_bounds__(64) void encode_queries_kernel(const float *__restrict__ queries, uint32_t qdim,
                                                           uint32_t actual_dim, float alpha, float offset,
                                                           int distance, int invert, uint8_t *__restrict__ codes_out,
                                                           uint32_t code_pitch, float *__restrict__ offsets_out, int four) {
    const int lane = threadIdx.x;
    const float *query = queries + (size_t)blockIdx.x * qdim;
    uint8_t *codes = codes_out + (size_t)blockIdx.x * code_pitch;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, four);
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t j = lane; j < actual_dim; j += 64) {
        uint32_t c = j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code;
        codes[j] = (uint8_t)c;
        s1 += c;
        s2 += c * c;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
    }
    if (lane == 0) {
        float off;
        if (distance == QAMD_DOT) {
            float s = (float)s1;
            if (s1 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++)
                    s += (float)(j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code);
            }
            off = s * alpha * offset;
        } else if (distance == QAMD_L1) {
            off = 0.0f;
        } else {
            float s = (float)s2;
            if (s2 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    float c = (float)(j < qdim ? f32_to_code(query[j], alpha, offset, four) : pad_code);
                    s += c * c;
                }
            }
            off = s * alpha * alpha;
        }
        offsets_out[blockIdx.x] = invert ? -off : off;
    }
}

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

// ---- compact 4-bit stores: the two kernels that read the nibble image where the others read byte codes ----
// 16-byte index of image chunk j of row r (u8_internal.hpp).
__device__ __forceinline__ uint64_t nibble_at(uint64_t r, uint32_t j, uint32_t pchunks) {
    return ((r / kPackBlockRows) * pchunks + j) * kPackBlockRows + r % kPackBlockRows;
}
__device__ __forceinline__ uint4 nibbles_lo(const uint4 &w) { return and16(w, 0x0F0F0F0Fu); }
__device__ __forceinline__ uint4 nibbles_hi(const uint4 &w) {
    return make_uint4((w.x >> 4) & 0x0F0F0F0Fu, (w.y >> 4) & 0x0F0F0F0Fu, (w.z >> 4) & 0x0F0F0F0Fu, (w.w >> 4) & 0x0F0F0F0Fu);
}

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

// u8_score_pairs_kernel over the nibble image: out[k] = score(query of pair k, ids[k]), the same three ways to name the
// query (one byte-code query for every pair; query l of a byte-code batch for list l; stored row list_rows[l] for list l)
// and the same walk through the lists.  One 16-lane group per pair; lane `sub` takes image chunks sub, sub + 16, ... of
// the row - ITERS = ceil(pchunks / 16) <= 4, all of them in flight at once.  A row's chunks lie a kilobyte apart (the
// image is laid out for the scan, a row per lane), so a pair costs `pchunks` 64-byte sectors where the byte codes cost
// actual_dim / 64.  A chunk is expanded as the scan's Image4 reads it: low nibbles against code chunk 2j, high nibbles
// against 2j + 1, which a row of odd row_chunks does not have (its high nibbles are zero; the query chunk is not read).
// For a stored-row query the other side is expanded the same way.  The integer sum is the one the byte codes give (at
// most 2048 * 15 * 15 < 2^24: exact in f32 in either lane mode), the epilogue is u8_score_pairs_kernel's: the same bits.
template <int ITERS>
__global__ __launch_bounds__(kBlock) void u8_nibble_pairs_kernel(
    const uint4 *__restrict__ image, const float *__restrict__ offsets, const uint4 *__restrict__ q_single,
    const float *__restrict__ q_off_single, const uint8_t *__restrict__ q_batch, uint32_t q_pitch,
    const float *__restrict__ q_offs, const uint32_t *__restrict__ lists, uint32_t n_lists,
    const uint32_t *__restrict__ list_rows, float multiplier, float diff, int mode, const uint32_t *__restrict__ ids,
    uint64_t n_ids, uint32_t n_rows, uint32_t row_chunks, uint32_t pchunks, uint32_t pairs_per_block, float *__restrict__ out) {
    constexpr int G = 16, GROUPS = kBlock / G;
    __shared__ uint32_t first_list;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, group = threadIdx.x / G;
    const uint64_t p0 = (uint64_t)blockIdx.x * pairs_per_block;
    const uint64_t p1 = p0 + pairs_per_block < n_ids ? p0 + pairs_per_block : n_ids;
    uint32_t l = lists ? first_list_of_block(lists, n_lists, p0, &first_list) : 0u;
    const float q_off_one = lists ? 0.0f : *q_off_single;
    for (uint64_t k = p0 + group; k < p1; k += GROUPS) {
        const uint32_t row = ids[k];
        bool ok = row < n_rows;
        const uint4 *qp = q_single;
        float q_off = q_off_one;
        uint32_t qrow = 0;
        if (lists) {
            l = advance_list(lists, n_lists, l, k);
            if (list_rows) {
                const uint32_t qr = list_rows[l];
                ok = ok && qr < n_rows;
                qrow = qr < n_rows ? qr : 0u;
                q_off = offsets[qrow];
            } else {
                qp = reinterpret_cast<const uint4 *>(q_batch + (size_t)l * q_pitch);
                q_off = q_offs[l];
            }
        }
        const uint32_t r = ok ? row : 0u;
        uint4 v[ITERS], qa[ITERS], qb[ITERS];
#pragma unroll
        for (int it = 0; it < ITERS; it++) {  // unconditional loads (clamped chunk): all of them issue back to back
            const uint32_t j = sub + it * G, jc = j < pchunks ? j : pchunks - 1;
            v[it] = image[nibble_at(r, jc, pchunks)];
            if (list_rows) {
                const uint4 wq = image[nibble_at(qrow, jc, pchunks)];
                qa[it] = nibbles_lo(wq);
                qb[it] = nibbles_hi(wq);
            } else {
                qa[it] = qp[2 * jc];
                qb[it] = qp[2 * jc + 1 < row_chunks ? 2 * jc + 1 : 2 * jc];  // no such chunk: dotted with zero nibbles
            }
        }
        uint32_t acc = 0;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            if (sub + it * G < pchunks) {
                acc = dot16(nibbles_lo(v[it]), qa[it], acc);
                acc = dot16(nibbles_hi(v[it]), qb[it], acc);
            }
        }
        acc = group_sum<G>(acc);
        if (sub == 0) out[k] = ok ? epilogue(multiplier, acc, q_off, offsets[row], diff, mode) : __builtin_nanf("");
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

uint64_t actual_dim_of(uint64_t dim) { return dim + (16 - dim % 16) % 16; }  // :257-259

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
qamd_status launch_rot_values(const float *src, uint64_t n, uint64_t dim, float *out, hipStream_t s) {
    RotValuesSink sink;
    sink.out = out;
    return launch_rot_u8(sink, src, n, dim, s);
}
bool rot_dim_ok(uint64_t dim) { return dim != 0 && dim % kRotBlockMin == 0 && dim <= kRotMaxDim; }

}  // namespace

// ------------------------------------------------------------------------------ handles
// struct qamd_u8 / qamd_u8_query: u8_internal.hpp

namespace {

U8Image u8_image_of(uint32_t rc, bool four_bit, int distance);

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
U8Image u8_image_of(uint32_t rc, bool four_bit, int distance) {
    if (distance == QAMD_L1 || rc > 128 || rc < (four_bit ? 2u : 8u)) return U8Image{};
    if (four_bit) return U8Image{U8_IMAGE_NIBBLE, (rc + 1) / 2, rc};
    return U8Image{U8_IMAGE_7BIT, rc - rc / 8, rc / 8};
}

// Writes rows [r0, r0 + n_rows) of the store's image from their byte codes; `bad`: u8_pack_image_kernel.
// `tile` (a compact store): the byte codes of exactly these rows, in the staging buffer.
qamd_status launch_pack(const qamd_u8 *h, uint64_t r0, uint64_t n_rows, uint32_t *bad, hipStream_t s,
                        const uint4 *tile = nullptr) {
    const auto kernel = h->image.kind == U8_IMAGE_NIBBLE ? u8_pack_image_kernel<Image4> : u8_pack_image_kernel<Image7>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n_rows * h->image.chunks, kBlock, 8)), dim3(kBlock), 0, s,
                       tile ? tile : h->byte_codes<uint4>(), tile ? r0 : 0, r0, n_rows, h->row_chunks, h->image.chunks,
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

// Byte codes of image rows [r0, r0 + n) or, with a device list, of rows[0 .. n): u8_nibble_unpack_kernel.
qamd_status launch_unpack(const qamd_u8 *h, const uint32_t *rows_dev, uint64_t r0, uint64_t n, uint8_t *out, uint64_t pitch,
                          float *q_offs, hipStream_t s) {
    if (n == 0) return QAMD_OK;
    hipLaunchKernelGGL(u8_nibble_unpack_kernel, dim3(grid_for(n * h->image.chunks, kBlock, 8)), dim3(kBlock), 0, s,
                       h->packed.as<uint4>(), h->offsets.as<float>(), rows_dev, r0, n, (uint32_t)h->count, h->row_chunks,
                       h->image.chunks, out, pitch, q_offs);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// Stored row i as the query of a whole-store call or of score_internal_ids: its byte codes and where its offset lies.
// A store with byte codes points into them; a compact one unpacks the row into `tmp`, which lives until the caller's
// launches are enqueued (freed in stream order).
qamd_status stored_row_query(const qamd_u8 *h, uint32_t i, StreamBuf &tmp, hipStream_t s, const uint4 *&qc, const float *&qo) {
    qo = h->offsets.as<float>() + i;
    if (!h->compact) {
        qc = h->byte_codes<uint4>() + (uint64_t)i * h->row_chunks;
        return QAMD_OK;
    }
    QAMD_TRY(tmp.alloc(h->meta.actual_dim, s, i >= h->count));
    qc = tmp.as<uint4>();
    if (i >= h->count) return QAMD_OK;  // (an empty store's top-k names a row that no kernel will read)
    return launch_unpack(h, nullptr, i, 1, tmp.as<uint8_t>(), h->meta.actual_dim, nullptr, s);
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
    const U8Image im = u8_image_of(h->row_chunks, h->four_bit, h->meta.vector_parameters.distance_type);
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

// The epilogue of a whole-store launch: an encoded query (EPI_POINT, the default) or, for score_internal against the whole
// store, a stored row with score_internal's `diff` (internal_epi).
struct ScanEpi {
    float diff = 0.0f;
    int mode = EPI_POINT;
    uint64_t rows = 0;  // the scan covers rows [0, rows) of the store (a null id list of n_ids rows); 0 = all of them
};
// Rows a whole-store launch covers.
inline uint64_t scan_rows(const qamd_u8 *h, const ScanEpi &e) { return e.rows ? e.rows : h->count; }

// A run-time flag of a whole-store launch as a compile-time constant: f gets std::true_type / std::false_type, or the
// EPI_* of e.mode as a std::integral_constant, and names the kernel instantiation with it.
template <class F> void with_bool(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F> void with_epi(int mode, F &&f) {
    if (mode == EPI_POINT) f(std::integral_constant<int, EPI_POINT>{});
    else f(std::integral_constant<int, EPI_INTERNAL>{});
}

template <bool IS_L1> struct ScanLaunch {
    template <int G, int ITERS, int UNROLL>
    static void go(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out, const TopkFilter *filt, hipStream_t s,
                   const ScanEpi &e) {
        constexpr int TILE = (64 / G) * UNROLL;
        const uint64_t waves = (scan_rows(h, e) + TILE - 1) / TILE;  // one wave per tile
        const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
        with_bool(h->row_chunks == (uint32_t)(G * ITERS), [&](auto ex) {
            with_bool(filt != nullptr, [&](auto fi) {
                with_epi(e.mode, [&](auto epi) {
                    hipLaunchKernelGGL((u8_scan_kernel<G, ITERS, UNROLL, IS_L1, ex, fi, epi>), dim3(grid), dim3(kScanBlock), 0,
                                       s, h->byte_codes<uint4>(), h->offsets.as<float>(), qc, qo, h->meta.multiplier,
                                       (uint32_t)scan_rows(h, e), h->row_chunks, out, filt ? *filt : TopkFilter{}, e.diff);
                });
            });
        });
    }
};

// Waves per block of the blocked scan: one, unless the store's blocks are too few to give every SIMD four waves (half
// of what it holds); then the smallest of 2, 4, 8 that does, else 8.
uint32_t blocked_split(uint64_t count) {
    const uint64_t blocks = (count + kPackBlockRows - 1) / kPackBlockRows;
    const uint64_t want = (uint64_t)device_info().cu_count * 16;
    uint32_t split = 1;
    while (split < 8 && blocks * split < want) split *= 2;
    return split;
}

// The Dot / L2 scan of a store that has a scan image: u8_scan_image_kernel, in the image's format, over its blocks.
void launch_scan_image(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out, const TopkFilter *filt,
                       hipStream_t s, const ScanEpi &e) {
    const uint64_t n_rows = scan_rows(h, e);
    const uint32_t split = blocked_split(n_rows), blocks_per_wg = (kScanBlock / 64) / split;
    const uint64_t blocks = (n_rows + kPackBlockRows - 1) / kPackBlockRows;
    const unsigned grid = (unsigned)((blocks + blocks_per_wg - 1) / blocks_per_wg);
    h->last_scan_split.store((int)split, std::memory_order_relaxed);
    with_bool(h->image.kind == U8_IMAGE_NIBBLE, [&](auto nibble) {
        using IMG = std::conditional_t<nibble, Image4, Image7>;
        with_bool(filt != nullptr, [&](auto fi) {
            with_epi(e.mode, [&](auto epi) {
                hipLaunchKernelGGL((u8_scan_image_kernel<IMG, fi, epi>), dim3(grid), dim3(kScanBlock), 0, s,
                                   h->packed.as<uint4>(), h->offsets.as<float>(), qc, qo, h->meta.multiplier, (uint32_t)n_rows,
                                   h->image.chunks, h->image.aux, split, out, filt ? *filt : TopkFilter{}, e.diff);
            });
        });
    });
}

// Returns false when the store's row size has no templated kernel (caller uses the generic one).
// The Dot / L2 scans read the scan image when the store has one (its rows are 7/8 or half as long; an L1 store has none).
template <bool IS_L1>
bool launch_scan(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out, const TopkFilter *filt,
                 hipStream_t s, const ScanEpi &e) {
    using L = ScanLaunch<IS_L1>;
    h->last_scan_packed.store(h->image.kind, std::memory_order_relaxed);
    if (h->image.kind) return launch_scan_image(h, qc, qo, out, filt, s, e), true;
    const uint32_t rc = h->row_chunks;
    if (rc == 1) return L::template go<1, 1, 4>(h, qc, qo, out, filt, s, e), true;
    if (rc == 2) return L::template go<2, 1, 4>(h, qc, qo, out, filt, s, e), true;
    if (rc <= 4) return L::template go<4, 1, 8>(h, qc, qo, out, filt, s, e), true;
    if (rc <= 8) return L::template go<8, 1, 8>(h, qc, qo, out, filt, s, e), true;
    switch ((rc + 15) / 16) {
        case 1: return L::template go<16, 1, 8>(h, qc, qo, out, filt, s, e), true;
        case 2: return L::template go<16, 2, 4>(h, qc, qo, out, filt, s, e), true;
        case 3: return L::template go<16, 3, 4>(h, qc, qo, out, filt, s, e), true;
        case 4: return L::template go<16, 4, 2>(h, qc, qo, out, filt, s, e), true;
        case 5: return L::template go<16, 5, 2>(h, qc, qo, out, filt, s, e), true;
        case 6: return L::template go<16, 6, 2>(h, qc, qo, out, filt, s, e), true;
        case 7: return L::template go<16, 7, 2>(h, qc, qo, out, filt, s, e), true;
        case 8: return L::template go<16, 8, 2>(h, qc, qo, out, filt, s, e), true;
        default: break;
    }
    return false;
}

template <bool IS_L1>
void launch_scan_generic(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out, hipStream_t s, const ScanEpi &e) {
    uint64_t waves = (scan_rows(h, e) + 3) / 4;  // one wave per 4-row tile (non-persistent, see u8_scan_kernel)
    unsigned grid = (unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64));
    with_epi(e.mode, [&](auto epi) {
        hipLaunchKernelGGL((u8_scan_generic_kernel<IS_L1, epi>), dim3(grid), dim3(kBlock), 0, s, h->byte_codes<uint4>(),
                           h->offsets.as<float>(), qc, qo, h->meta.multiplier, (uint32_t)scan_rows(h, e), h->row_chunks, out,
                           e.diff);
    });
}

template <bool IS_L1> struct SmallLaunch {
    template <int G, int ITERS>
    static qamd_status go(const qamd_u8 *h, const uint4 *qc, const float *qo, const FusedQuery *fq, const SmallTopkPlan &pl,
                          const SmallTopk &p, hipStream_t s, const ScanEpi &e) {
        const bool exact = h->row_chunks == (uint32_t)(G * ITERS);
        if constexpr (G * ITERS * 16 > (int)kFusedQueryDims + 15 * 16) {
            if (fq) return fail(QAMD_ERR_ARGUMENTS, "fused query does not fit the kernel arguments");
        } else if (fq) {
            QueryByValue qv;
            memcpy(qv.v, fq->values, (size_t)fq->qdim * 4);
            const qamd_vector_parameters &vp = h->meta.vector_parameters;
            with_bool(exact, [&](auto ex) {
                hipLaunchKernelGGL((u8_topk_small_fused_kernel<G, ITERS, IS_L1, ex>), dim3(pl.workgroups), dim3(1024), 0, s,
                                   h->byte_codes<uint4>(), h->offsets.as<float>(), qv, fq->qdim, (uint32_t)h->meta.actual_dim,
                                   h->meta.alpha, h->meta.offset, vp.distance_type, vp.invert, fq->qbuf, h->meta.multiplier,
                                   (uint32_t)h->count, h->row_chunks, pl.rows_per_wg, p);
            });
            QAMD_HIP(hipGetLastError());
            return QAMD_OK;
        }
        with_bool(exact, [&](auto ex) {
            with_epi(e.mode, [&](auto epi) {
                hipLaunchKernelGGL((u8_topk_small_kernel<G, ITERS, IS_L1, ex, epi>), dim3(pl.workgroups), dim3(1024), 0, s,
                                   h->byte_codes<uint4>(), h->offsets.as<float>(), qc, qo, h->meta.multiplier,
                                   (uint32_t)h->count, h->row_chunks, pl.rows_per_wg, p, e.diff);
            });
        });
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
};

// Row group of the small top-k kernel for this store's row size; 0 = no templated shape.
int small_group(uint32_t rc) { return rc == 1 ? 1 : rc == 2 ? 2 : rc <= 4 ? 4 : rc <= 8 ? 8 : rc <= 128 ? 16 : 0; }

template <bool IS_L1>
qamd_status launch_small(const qamd_u8 *h, const uint4 *qc, const float *qo, const FusedQuery *fq, const SmallTopkPlan &pl,
                         const SmallTopk &p, hipStream_t s, const ScanEpi &e = ScanEpi{}) {
    using L = SmallLaunch<IS_L1>;
    const uint32_t rc = h->row_chunks;
    h->last_scan_packed.store(0, std::memory_order_relaxed);
    if (rc == 1) return L::template go<1, 1>(h, qc, qo, fq, pl, p, s, e);
    if (rc == 2) return L::template go<2, 1>(h, qc, qo, fq, pl, p, s, e);
    if (rc <= 4) return L::template go<4, 1>(h, qc, qo, fq, pl, p, s, e);
    if (rc <= 8) return L::template go<8, 1>(h, qc, qo, fq, pl, p, s, e);
    switch ((rc + 15) / 16) {
        case 1: return L::template go<16, 1>(h, qc, qo, fq, pl, p, s, e);
        case 2: return L::template go<16, 2>(h, qc, qo, fq, pl, p, s, e);
        case 3: return L::template go<16, 3>(h, qc, qo, fq, pl, p, s, e);
        case 4: return L::template go<16, 4>(h, qc, qo, fq, pl, p, s, e);
        case 5: return L::template go<16, 5>(h, qc, qo, fq, pl, p, s, e);
        case 6: return L::template go<16, 6>(h, qc, qo, fq, pl, p, s, e);
        case 7: return L::template go<16, 7>(h, qc, qo, fq, pl, p, s, e);
        case 8: return L::template go<16, 8>(h, qc, qo, fq, pl, p, s, e);
        default: break;
    }
    return fail(QAMD_ERR_ARGUMENTS, "no small top-k kernel for %u chunks", rc);
}

// ---- several queries per pass (u8_scan_multi_kernel) -------------------------------------------
template <bool IS_L1, int G, int ITERS, int UNROLL, int NQ>
void launch_multi_shape(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq_valid,
                        float *out, const TopkFilterSlices *slices, hipStream_t s, const ScanEpi &e) {
    constexpr int TILE = (64 / G) * UNROLL * NQ;  // NQ tiles per wave (u8_scan_multi_kernel TPW)
    const uint64_t n_rows = scan_rows(h, e);  // also the pitch of `out`
    const uint64_t waves = (n_rows + TILE - 1) / TILE;
    const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
    const bool exact = h->row_chunks == (uint32_t)(G * ITERS);
    h->last_scan_packed.store(0, std::memory_order_relaxed);
#define QAMD_U8_MULTI(EX, FI, EPI)                                                                                 \
    hipLaunchKernelGGL((u8_scan_multi_kernel<G, ITERS, UNROLL, NQ, IS_L1, EX, FI, EPI>), dim3(grid), dim3(kScanBlock), 0, s, \
                       h->byte_codes<uint4>(), h->offsets.as<float>(), qcodes, (uint32_t)q_pitch, q_offs, nq_valid,   \
                       h->meta.multiplier, (uint32_t)n_rows, h->row_chunks, out, n_rows,                           \
                       slices ? *slices : TopkFilterSlices{}, e.diff)
    if (e.mode == EPI_INTERNAL) {  // score_internal of gathered rows: scores only (no filtering form is instantiated)
        if (exact) QAMD_U8_MULTI(true, false, EPI_INTERNAL);
        else QAMD_U8_MULTI(false, false, EPI_INTERNAL);
    } else if (slices) {
        if (exact) QAMD_U8_MULTI(true, true, EPI_POINT);
        else QAMD_U8_MULTI(false, true, EPI_POINT);
    } else {
        if (exact) QAMD_U8_MULTI(true, false, EPI_POINT);
        else QAMD_U8_MULTI(false, false, EPI_POINT);
    }
#undef QAMD_U8_MULTI
}

// Lane mode 1 on a Dot / L2 store: every score comes from the avx2.c lane-order kernels (u8_scan_avx2_lanes_kernel,
// u8_score_pairs_kernel<.., LANES>); the kernels that sum the exact integer (single- and multi-query scans, the fused
// and single-launch top-k, the matrix cores) are not used.  L1 has no lane order: both modes are the exact sum.
// A compact store has no lane order either: its pair sums stay below 2^24, where both modes give the same
// bits, so mode 1 is accepted and its image routes go on serving.
bool lane_order(const qamd_u8 *h) {
    return h->lane_mode == 1 && h->meta.vector_parameters.distance_type != QAMD_L1 && !h->compact;
}

// Widest pass of the multi-query scan for this row size: 4 queries (2 for rows of more than 96
// pieces), 0 = none.  Measured on 10M x 768 / 12.5M x 1536, top-30 per query, whole call: 2 queries
// 1.24 / 2.93 ms and 4 queries 1.38 / 3.50 ms against 1.65 / 3.85 ms on the matrix-core path; an
// 8-wide pass (96 query VGPRs, 3 waves per SIMD) took 1.97 ms at dim 768 -- worse than the matrix
// cores -- so batches of 5 and more stay there.  L1 has no matrix form: its batches are served by this kernel alone,
// and there the 8-wide pass is the better one (8 queries per 1.97 ms against two 4-wide passes of 1.38 ms; rows of up
// to 768 bytes: 96 query registers).
uint32_t multi_width(const qamd_u8 *h) {
    const uint32_t rc = h->row_chunks, iters = (rc + 15) / 16;
    const bool l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
    if (rc < 9 || iters > 8 || lane_order(h) || h->compact) return 0;  // (the multi-query scan reads byte codes)
    return l1 && iters <= 3 ? 8 : iters <= 6 ? 4 : 2;
}

// One pass for `nq_valid` (2 .. multi_width) queries; false = unsupported.
template <bool IS_L1>
bool launch_multi(const qamd_u8 *h, uint32_t nq_valid, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs,
                  float *out, const TopkFilterSlices *slices, hipStream_t s, const ScanEpi &e = ScanEpi{}) {
    const uint32_t iters = (h->row_chunks + 15) / 16, width = multi_width(h);
    if (nq_valid < 2 || nq_valid > width || (slices && e.mode != EPI_POINT)) return false;
#define QAMD_U8_MULTI_IT(IT, UN)                                                                              \
    case IT:                                                                                                  \
        if constexpr (IS_L1 && IT <= 3) {                                                                     \
            if (nq_valid > 4) {                                                                               \
                launch_multi_shape<IS_L1, 16, IT, UN, 8>(h, qcodes, q_pitch, q_offs, nq_valid, out, slices, s, e); \
                return true;                                                                                  \
            }                                                                                                 \
        }                                                                                                     \
        if (nq_valid > 2) launch_multi_shape<IS_L1, 16, IT, UN, (IT <= 6 ? 4 : 2)>(h, qcodes, q_pitch, q_offs, nq_valid, out, slices, s, e); \
        else launch_multi_shape<IS_L1, 16, IT, UN, 2>(h, qcodes, q_pitch, q_offs, nq_valid, out, slices, s, e); \
        return true;
    switch (iters) {
        QAMD_U8_MULTI_IT(1, 4) QAMD_U8_MULTI_IT(2, 2) QAMD_U8_MULTI_IT(3, 2) QAMD_U8_MULTI_IT(4, 2)
        QAMD_U8_MULTI_IT(5, 1) QAMD_U8_MULTI_IT(6, 1) QAMD_U8_MULTI_IT(7, 1) QAMD_U8_MULTI_IT(8, 1)
        default: break;
    }
#undef QAMD_U8_MULTI_IT
    return false;
}

bool fused_capable(const qamd_u8 *h) { return !lane_order(h) && h->row_chunks <= 128; }

// The single-launch top-k serves this store and k (and, for a fused query, these dims): its plan.
bool u8_small_plan(const qamd_u8 *h, uint32_t k, SmallTopkPlan &plan) {
    const int g = small_group(h->row_chunks);
    if (!g || !fused_capable(h) || h->compact) return false;  // (it reads byte codes: a compact store has none)
    const uint32_t tile = 2 * (64 / g);
    const uint32_t least = (uint32_t)std::max<uint64_t>(16 * tile, (128 * 1024) / std::max<uint64_t>(h->meta.actual_dim, 1));
    return small_topk_plan(h->count, k, tile, least, plan);
}

// qc: the query's actual_dim codes (16-byte aligned), qo: its f32 offset -- inside a qamd_u8_query
// or straight out of a query batch ([q][pitch] codes, [q] offsets).
qamd_status scan_ptrs(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out_dev, hipStream_t s,
                      const TopkFilter *filt = nullptr, const ScanEpi &e = ScanEpi{}) {
    if (h->count == 0) return QAMD_OK;
    const bool is_l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
    h->last_scan_packed.store(0, std::memory_order_relaxed);  // launch_scan reports the packed image
    if (lane_order(h)) {
        uint64_t waves = (scan_rows(h, e) + 3) / 4;
        unsigned grid = (unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64));
        with_epi(e.mode, [&](auto epi) {
            hipLaunchKernelGGL((u8_scan_avx2_lanes_kernel<true, epi>), dim3(grid), dim3(kBlock), 0, s, h->byte_codes<uint4>(),
                               h->offsets.as<float>(), qc, qo, h->meta.multiplier, (uint32_t)scan_rows(h, e), h->row_chunks,
                               out_dev, e.diff);
        });
    } else if (is_l1) {
        if (!launch_scan<true>(h, qc, qo, out_dev, filt, s, e)) launch_scan_generic<true>(h, qc, qo, out_dev, s, e);
    } else {
        if (!launch_scan<false>(h, qc, qo, out_dev, filt, s, e)) launch_scan_generic<false>(h, qc, qo, out_dev, s, e);
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

qamd_status scan_into(const qamd_u8 *h, const qamd_u8_query *q, float *out_dev, hipStream_t s,
                      const TopkFilter *filt = nullptr) {
    return scan_ptrs(h, reinterpret_cast<const uint4 *>(q->buf.as<uint8_t>() + 16), q->buf.as<float>(), out_dev, s, filt);
}

qamd_status check_query(const qamd_u8 *h, const qamd_u8_query *q) {
    if (!h || !q) return fail(QAMD_ERR_ARGUMENTS, "null handle or query");
    if (q->actual_dim != h->meta.actual_dim)
        return fail(QAMD_ERR_ARGUMENTS, "query has %llu codes, store rows have %llu",
                    (unsigned long long)q->actual_dim, (unsigned long long)h->meta.actual_dim);
    return QAMD_OK;
}

// One launch of u8_score_pairs_kernel.  lists == nullptr: the single query (qc, qo) for every id.
template <bool IS_L1>
qamd_status launch_pairs(const qamd_u8 *h, const uint4 *qc, const float *qo, const uint8_t *q_batch, uint32_t q_pitch,
                         const float *q_offs, const uint32_t *lists, uint32_t n_lists, const uint32_t *list_rows, float diff,
                         int mode, const uint32_t *ids_dev, uint64_t n_ids, float *out_dev, hipStream_t s) {
    const uint64_t ppb = pairs_per_block(n_ids, 16);  // 16 lane groups per workgroup
    const unsigned grid = (unsigned)((n_ids + ppb - 1) / ppb);
    const uint32_t iters = (h->row_chunks + 15) / 16;
#define QAMD_U8_PAIRS(IT)                                                                                                \
    hipLaunchKernelGGL((u8_score_pairs_kernel<IS_L1, IT>), dim3(grid), dim3(kBlock), 0, s, h->byte_codes<uint4>(),         \
                       h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows,              \
                       h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks, (uint32_t)ppb, \
                       out_dev)
    if (!IS_L1 && lane_order(h)) {
        hipLaunchKernelGGL((u8_score_pairs_kernel<false, 0, true>), dim3(grid), dim3(kBlock), 0, s, h->byte_codes<uint4>(),
                           h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows,
                           h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks, (uint32_t)ppb,
                           out_dev);
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
    switch (iters) {
        case 1: QAMD_U8_PAIRS(1); break;
        case 2: QAMD_U8_PAIRS(2); break;
        case 3: QAMD_U8_PAIRS(3); break;
        case 4: QAMD_U8_PAIRS(4); break;
        case 5: QAMD_U8_PAIRS(5); break;
        case 6: QAMD_U8_PAIRS(6); break;
        case 7: QAMD_U8_PAIRS(7); break;
        case 8: QAMD_U8_PAIRS(8); break;
        default: QAMD_U8_PAIRS(0); break;
    }
#undef QAMD_U8_PAIRS
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

qamd_status score_pairs_dev(const qamd_u8 *h, const uint4 *qc, const float *qo, const uint8_t *q_batch, uint32_t q_pitch,
                            const float *q_offs, const uint32_t *lists, uint32_t n_lists, const uint32_t *list_rows,
                            float diff, int mode, const uint32_t *ids_dev, uint64_t n_ids, float *out_dev, hipStream_t s) {
    if (n_ids == 0) return QAMD_OK;
    if (h->compact) {  // the pairs are gathered from the nibble image
        const uint64_t ppb = pairs_per_block(n_ids, 16);
        const unsigned grid = (unsigned)((n_ids + ppb - 1) / ppb);
#define QAMD_U8_NIBBLE_PAIRS(IT)                                                                                          \
    hipLaunchKernelGGL((u8_nibble_pairs_kernel<IT>), dim3(grid), dim3(kBlock), 0, s, h->packed.as<uint4>(),               \
                       h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows,               \
                       h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks, h->image.chunks, \
                       (uint32_t)ppb, out_dev)
        switch ((h->image.chunks + 15) / 16) {  // at most 64 chunks (u8_image_of)
            case 1: QAMD_U8_NIBBLE_PAIRS(1); break;
            case 2: QAMD_U8_NIBBLE_PAIRS(2); break;
            case 3: QAMD_U8_NIBBLE_PAIRS(3); break;
            default: QAMD_U8_NIBBLE_PAIRS(4); break;
        }
#undef QAMD_U8_NIBBLE_PAIRS
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
    if (h->meta.vector_parameters.distance_type == QAMD_L1)
        return launch_pairs<true>(h, qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows, diff, mode, ids_dev, n_ids, out_dev, s);
    return launch_pairs<false>(h, qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows, diff, mode, ids_dev, n_ids, out_dev, s);
}

qamd_status score_ids_dev(const qamd_u8 *h, const uint4 *qc, const float *qo, float diff, int mode,
                          const uint32_t *ids_dev, uint64_t n_ids, float *out_dev, hipStream_t s) {
    return score_pairs_dev(h, qc, qo, nullptr, 0, nullptr, nullptr, 0, nullptr, diff, mode, ids_dev, n_ids, out_dev, s);
}

// encoded_vectors_u8.rs:389-395: the `diff` of score_internal, actual_dim * offset * offset (negated if invert)
float internal_diff(const qamd_u8 *h) {
    float diff = (float)h->meta.actual_dim * h->meta.offset * h->meta.offset;
    return h->meta.vector_parameters.invert ? -diff : diff;
}

// out[k] = score of (query (qc, qo), ids[k]) for host or device ids / outputs (run_ids, lists.hpp): the body of
// score_ids and, with (qc, qo) = row i of the store and the internal epilogue, of score_internal_ids.
qamd_status score_ids_any(const qamd_u8 *h, const uint4 *qc, const float *qo, float diff, int mode, const uint32_t *ids,
                          uint64_t n_ids, qamd_mem ids_mem, float *out, qamd_mem out_mem, hipStream_t s) {
    return run_ids(ids, n_ids, ids_mem, out, out_mem, h->count, s, [&](const uint32_t *ids_dev, uint64_t n, float *out_dev) {
        return score_ids_dev(h, qc, qo, diff, mode, ids_dev, n, out_dev, s);
    });
}

// ---- score_internal of many stored rows against the rows 0 .. n_ids - 1 (the null-list burst) ----
// Workgroup l copies the byte codes of stored row rows[l] into qcodes[l][..] and its stored offset into q_offs[l]: the
// block the scans read as their queries.  `rows` is device memory (no read-back); a row >= count (device rows cannot be
// validated) is clamped to row 0, and its list is overwritten with NaN afterwards (null_list_nan_kernel).
__global__ __launch_bounds__(64) void u8_gather_rows_kernel(const uint4 *__restrict__ codes, const float *__restrict__ offsets,
                                                            const uint32_t *__restrict__ rows, uint32_t count,
                                                            uint32_t row_chunks, uint4 *__restrict__ qcodes,
                                                            float *__restrict__ q_offs) {
    const uint32_t l = blockIdx.x;
    uint32_t r = rows[l];
    if (r >= count) r = 0;
    const uint4 *src = codes + (uint64_t)r * row_chunks;
    uint4 *dst = qcodes + (uint64_t)l * row_chunks;
    for (uint32_t c = threadIdx.x; c < row_chunks; c += 64) dst[c] = src[c];
    if (threadIdx.x == 0) q_offs[l] = offsets[r];
}

// Rows per launch group of the null-list burst: what the gathered block may take (8 MiB of codes), 4096 at the most.
uint32_t internal_batch_group(const qamd_u8 *h) {
    return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(8, (8ull << 20) / std::max<uint64_t>(h->meta.actual_dim, 1)));
}

// out_dev[l * n_ids + j] = score_internal(rows_dev[l], j) for l < n, j < n_ids <= count.  The rows are gathered once;
// then passes of multi_width(h) rows (u8_scan_multi_kernel with score_internal's epilogue: the integer sum and the f32
// epilogue of the single-row scan, so the same bits), a remainder of one row and every row size without a multi form
// (fewer than 9 or more than 128 pieces, lane order) through the single-row scan.  Enqueues only.
qamd_status score_internal_rows_dev(const qamd_u8 *h, const uint32_t *rows_dev, uint32_t n, uint64_t n_ids, float *out_dev,
                                    hipStream_t s) {
    const uint64_t pitch = h->meta.actual_dim;  // 16 * row_chunks
    const size_t code_bytes = (size_t)n * pitch;
    StreamBuf stage;
    QAMD_TRY(stage.alloc(code_bytes + (size_t)n * 4, s));
    uint8_t *qcodes = stage.as<uint8_t>();
    float *q_offs = reinterpret_cast<float *>(qcodes + code_bytes);
    if (h->compact) {  // the rows come out of the image; every one of them then takes the image scan (width 0)
        QAMD_TRY(launch_unpack(h, rows_dev, 0, n, qcodes, pitch, q_offs, s));
    } else {
        hipLaunchKernelGGL(u8_gather_rows_kernel, dim3(n), dim3(64), 0, s, h->byte_codes<uint4>(), h->offsets.as<float>(),
                           rows_dev, (uint32_t)h->count, h->row_chunks, reinterpret_cast<uint4 *>(qcodes), q_offs);
        QAMD_HIP(hipGetLastError());
    }
    const ScanEpi e{internal_diff(h), EPI_INTERNAL, n_ids};
    const bool is_l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
    const uint32_t width = multi_width(h);
    for (uint32_t l = 0; l < n;) {
        const uint32_t nq = std::min(width, n - l);
        const uint8_t *qc = qcodes + (uint64_t)l * pitch;
        float *o = out_dev + (uint64_t)l * n_ids;
        const bool ok = nq >= 2 && (is_l1 ? launch_multi<true>(h, nq, qc, pitch, q_offs + l, o, nullptr, s, e)
                                          : launch_multi<false>(h, nq, qc, pitch, q_offs + l, o, nullptr, s, e));
        if (ok) {
            l += nq;
        } else {
            QAMD_TRY(scan_ptrs(h, reinterpret_cast<const uint4 *>(qc), q_offs + l, o, s, nullptr, e));
            l += 1;
        }
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
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
        QAMD_TRY(launch_rot_values(vals, slice, dim, rot.as<float>(), s));
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
        sink.alpha = alpha, sink.offset = offset, sink.fast = h->four_bit ? kQuant4Bit : (int)fast;
        sink.distance = vp.distance_type, sink.invert = vp.invert;
        sink.codes32 = codes32, sink.offsets = offsets, sink.row0 = r0;
        return launch_rot_u8(sink, src, nr, dim, s);
    }
    if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const uint64_t waves = (nr + 3) / 4;
        const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
        const uint32_t per_lane = (uint32_t)((h->meta.actual_dim / 4 + 15) / 16);  // float4 per lane
#define QAMD_Q16(IT)                                                                                          \
    do {                                                                                                      \
        if (h->four_bit)  /* 4-bit codes take the exact division */                              \
            hipLaunchKernelGGL((quantize16_kernel<IT, false, true>), dim3(grid), dim3(kScanBlock), 0, s, src, nr, \
                               (uint32_t)dim, (uint32_t)h->meta.actual_dim, alpha, offset, vp.distance_type,  \
                               vp.invert, codes32, offsets, r0);                                              \
        else if (fast)                                                                                        \
            hipLaunchKernelGGL((quantize16_kernel<IT, true>), dim3(grid), dim3(kScanBlock), 0, s, src, nr,    \
                               (uint32_t)dim, (uint32_t)h->meta.actual_dim, alpha, offset, vp.distance_type,  \
                               vp.invert, codes32, offsets, r0);                                              \
        else                                                                                                  \
            hipLaunchKernelGGL((quantize16_kernel<IT, false>), dim3(grid), dim3(kScanBlock), 0, s, src, nr,   \
                               (uint32_t)dim, (uint32_t)h->meta.actual_dim, alpha, offset, vp.distance_type,  \
                               vp.invert, codes32, offsets, r0);                                              \
    } while (0)
        if (per_lane <= 2) QAMD_Q16(2);
        else if (per_lane <= 4) QAMD_Q16(4);
        else if (per_lane <= 6) QAMD_Q16(6);
        else if (per_lane <= 8) QAMD_Q16(8);
        else if (per_lane <= 12) QAMD_Q16(12);
        else if (per_lane <= 16) QAMD_Q16(16);
        else QAMD_Q16(0);
#undef QAMD_Q16
    } else {
        int grid = grid_for(nr, kBlock / 64, 8);
        hipLaunchKernelGGL(quantize_kernel, dim3(grid), dim3(kBlock), 0, s, src, nr, (uint32_t)dim,
                           (uint32_t)h->meta.actual_dim, alpha, offset, vp.distance_type, vp.invert,
                           codes32, offsets, r0, (int)h->four_bit);
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
// metadata and the flags beside it.  No device call.
struct U8Flags {
    bool rotated = false, four_bit = false, compact = false;
};
constexpr int kU8FlagBits = QAMD_ROTATED | QAMD_BITS4 | QAMD_COMPACT;
qamd_status split_distance(const qamd_vector_parameters &vp, int &base, U8Flags &f) {
    const int dt = vp.distance_type;
    bool &rotated = f.rotated, &four_bit = f.four_bit;
    rotated = dt >= 0 && (dt & QAMD_ROTATED) != 0;
    four_bit = dt >= 0 && (dt & QAMD_BITS4) != 0;
    f.compact = dt >= 0 && (dt & QAMD_COMPACT) != 0;
    base = dt >= 0 ? (dt & ~kU8FlagBits) : dt;
    if (base < 0 || base > 2) return fail(QAMD_ERR_ARGUMENTS, "bad distance_type %d", dt);
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
    const bool rotated = flags.rotated, four_bit = flags.four_bit;
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
    h->rotated = rotated;
    h->four_bit = four_bit;
    h->compact = flags.compact;
    const float levels = four_bit ? 15.0f : 127.0f;  // alpha = (max - min) / levels (:228-232)
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
    h->rotated = flags.rotated;
    h->four_bit = flags.four_bit;
    h->compact = flags.compact;
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
        if (h->compact) QAMD_TRY(launch_unpack(h, nullptr, src_row, nr, tile.as<uint8_t>(), h->meta.actual_dim, nullptr, s));
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
    if (h->rotated) out->vector_parameters.distance_type |= QAMD_ROTATED;
    if (h->four_bit) out->vector_parameters.distance_type |= QAMD_BITS4;
    if (h->compact) out->vector_parameters.distance_type |= QAMD_COMPACT;
    return QAMD_OK;
}

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
    bool rotated = false;
    for (const auto &m : root.members) {
        if (m.first != "rotation") continue;
        if (rotated || m.second.kind != JsonValue::String || m.second.text != "HadamardBlocks")
            return fail(QAMD_ERR_IO, "%s: unknown or repeated rotation", meta_path);
        rotated = true;
    }
    if (rotated && (meta.vector_parameters.distance_type == QAMD_L1 || !rot_dim_ok(vp->dim)))
        return fail(QAMD_ERR_IO, "%s: a rotated store of metric %s and %llu dimensions", meta_path,
                    distance_name(meta.vector_parameters.distance_type), (unsigned long long)vp->dim);
    // "bits" (DESIGN 3.1y): absent = a 7-bit store; 4 is the one value a store writes
    bool four_bit = false;
    for (const auto &m : root.members) {
        if (m.first != "bits") continue;
        const JsonValue &b = m.second;
        if (four_bit || b.kind != JsonValue::Number || !b.integer || b.negative || b.uint != 4)
            return fail(QAMD_ERR_IO, "%s: unknown or repeated bits", meta_path);
        four_bit = true;
    }
    if (four_bit && meta.vector_parameters.distance_type == QAMD_L1)
        return fail(QAMD_ERR_IO, "%s: a 4-bit store of metric L1", meta_path);
    // "compact" (DESIGN 3.1z): absent = the store keeps its byte codes; true, beside "bits":4, is the one value a store writes
    bool compact = false;
    for (const auto &m : root.members) {
        if (m.first != "compact") continue;
        if (compact || m.second.kind != JsonValue::Bool || !m.second.boolean || !four_bit)
            return fail(QAMD_ERR_IO, "%s: unknown, repeated or misplaced compact", meta_path);
        compact = true;
    }
    if (compact && !u8_image_of((uint32_t)std::min<uint64_t>(actual_dim_of(vp->dim) / 16, 0xFFFFFFFFull), true,
                                meta.vector_parameters.distance_type).kind)
        return fail(QAMD_ERR_IO, "%s: a compact store of %llu dimensions", meta_path, (unsigned long long)vp->dim);
    const uint64_t size = qamd_u8_quantized_vector_size(vp);
    std::string bytes;
    QAMD_TRY(load_rows_file(data_path, size * vp->count, bytes));
    // The reference keeps the file's metadata but sizes rows from the caller's parameters.
    qamd_u8_metadata eff = meta;
    eff.vector_parameters.dim = vp->dim;
    eff.vector_parameters.count = vp->count;
    eff.actual_dim = actual_dim_of(vp->dim);
    if (rotated) eff.vector_parameters.distance_type |= QAMD_ROTATED;  // from_rows takes it off again
    if (four_bit) eff.vector_parameters.distance_type |= QAMD_BITS4;
    if (compact) eff.vector_parameters.distance_type |= QAMD_COMPACT;
    qamd_status st = qamd_u8_from_rows(reinterpret_cast<const uint8_t *>(bytes.data()), QAMD_MEM_HOST, &eff,
                                       nullptr, out);
    eff.vector_parameters.distance_type = meta.vector_parameters.distance_type;
    if (st == QAMD_OK) (*out)->meta = meta.actual_dim == eff.actual_dim ? meta : eff;
    return st;
}

}  // extern "C"

namespace {

// Runs the encode kernel for `query` (host or device f32) into q's buffer on stream s.
qamd_status encode_now(const qamd_u8_query *q, const float *query, uint64_t qdim, qamd_mem query_mem, hipStream_t s) {
    const uint64_t ad = q->actual_dim;
    // The query is always encoded on the device (one implementation, no CPU arithmetic in the
    // product): a host query is uploaded first (qdim * 4 bytes; the buffer keeps room for it
    // behind the codes).
    const float *q_dev = query;
    bool via_scratch = false;
    if (query_mem == QAMD_MEM_HOST && qdim) {
        // through the thread's mapped host scratch when it fits: one memcpy on the host, the kernel
        // reads the values over PCIe itself -- no copy call, no synchronisation
        const float *dev_view = nullptr;
        if (float *hq = host_query_acquire(qdim, &dev_view)) {
            memcpy(hq, query, qdim * 4);
            q_dev = dev_view;
            via_scratch = true;
        } else {
            float *stage = reinterpret_cast<float *>(q->buf.as<uint8_t>() + 16 + round_up(ad, 16));
            QAMD_TRY(copy_in(stage, query, QAMD_MEM_HOST, qdim * 4, s));
            q_dev = stage;
        }
    }
    if (q->rotated) {  // the rotated values go behind the staging area, and the encoder reads those
        float *rot = reinterpret_cast<float *>(q->buf.as<uint8_t>() + 16 + round_up(ad, 16) + ad * 4);
        QAMD_TRY(launch_rot_values(q_dev, 1, qdim, rot, s));
        q_dev = rot;
    }
    hipLaunchKernelGGL(encode_query_kernel, dim3(1), dim3(64), 0, s, q_dev, (uint32_t)qdim, (uint32_t)ad, q->alpha,
                       q->offset, q->distance, q->invert, q->buf.as<uint8_t>(), (int)q->four_bit);
    QAMD_HIP(hipGetLastError());
    if (via_scratch) host_query_release(s);
    return q->ready.record(s);
}

// A deferred host query (qamd_u8_query::host_f32) is encoded now, on the consumer's stream.
qamd_status ensure_encoded(const qamd_u8_query *q, hipStream_t s) {
    if (!q->deferred.load(std::memory_order_acquire)) return QAMD_OK;
    std::lock_guard<std::mutex> lk(q->encode_mu);
    if (!q->deferred.load(std::memory_order_relaxed)) return QAMD_OK;
    QAMD_TRY(encode_now(q, q->host_f32.data(), q->host_f32.size(), QAMD_MEM_HOST, s));
    q->deferred.store(false, std::memory_order_release);
    return QAMD_OK;
}

}  // namespace

extern "C" {

qamd_status qamd_u8_encode_query(const qamd_u8 *h, const float *query, uint64_t qdim, qamd_mem query_mem,
                                 void *stream, qamd_u8_query **query_io) {
    if (!h || !query_io || (!query && qdim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (h->rotated && qdim != h->meta.vector_parameters.dim)
        return fail(QAMD_ERR_ARGUMENTS, "a query of %llu dimensions against rotated rows of %llu", (unsigned long long)qdim,
                    (unsigned long long)h->meta.vector_parameters.dim);
    const uint64_t ad = actual_dim_of(qdim);
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    qamd_u8_query *q = *query_io;
    std::unique_ptr<qamd_u8_query> fresh;
    if (!q) {
        fresh.reset(new qamd_u8_query);
        q = fresh.get();
        q->device = h->device;
    }
    // offset | codes | f32 staging | the rotated values of a rotated store's query
    const size_t buf_bytes = 16 + round_up(ad, 16) + ad * 4 + 16 + (h->rotated ? ad * 4 : 0);
    if (q->actual_dim != ad || !q->buf.ptr || q->buf.bytes < buf_bytes) {
        if (q->pooled) query_buf_put(q->buf, false);
        QAMD_TRY(query_buf_get(buf_bytes, q->buf));
        q->pooled = true;
        q->actual_dim = ad;
    }
    q->rotated = h->rotated;
    q->four_bit = h->four_bit;
    q->alpha = h->meta.alpha;
    q->offset = h->meta.offset;
    q->distance = h->meta.vector_parameters.distance_type;
    q->invert = h->meta.vector_parameters.invert;
    // (the fused top-k neither rotates nor makes 4-bit codes)
    if (query_mem == QAMD_MEM_HOST && u8_host_encode_is_lazy(qdim) && !h->rotated && !h->four_bit) {
        // Deferred: the values are kept, nothing is launched.  On a small store the top-k kernel takes them
        // by value and quantises them itself (u8_topk_small_fused_kernel); any other consumer encodes first.
        std::lock_guard<std::mutex> lk(q->encode_mu);
        q->host_f32.assign(query, query + qdim);
        q->deferred.store(true, std::memory_order_release);
    } else {
        {
            std::lock_guard<std::mutex> lk(q->encode_mu);
            q->deferred.store(false, std::memory_order_release);
        }
        QAMD_TRY(encode_now(q, query, qdim, query_mem, s));
    }
    if (fresh) *query_io = fresh.release();
    return QAMD_OK;
}

qamd_status qamd_u8_query_read(const qamd_u8_query *q, float *offset, uint8_t *codes, uint64_t capacity,
                               uint64_t *codes_len) {
    if (!q) return fail(QAMD_ERR_ARGUMENTS, "null query");
    QAMD_ON_DEVICE(q->device);
    if (codes_len) *codes_len = q->actual_dim;
    QAMD_TRY(ensure_encoded(q, nullptr));
    QAMD_TRY(q->ready.wait(nullptr));
    if (offset) QAMD_TRY(copy_out(offset, QAMD_MEM_HOST, q->buf.ptr, 4, nullptr));
    if (codes) {
        if (capacity < q->actual_dim) return fail(QAMD_ERR_ARGUMENTS, "codes buffer too small");
        QAMD_TRY(copy_out(codes, QAMD_MEM_HOST, q->buf.as<uint8_t>() + 16, q->actual_dim, nullptr));
    }
    return QAMD_OK;
}

void qamd_u8_query_free(qamd_u8_query *q) { delete q; }

qamd_status qamd_u8_score_all(const qamd_u8 *h, const qamd_u8_query *q, float *out, qamd_mem out_mem,
                              void *stream) {
    QAMD_TRY(check_query(h, q));
    if (h->count == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "out is null");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    QAMD_TRY(ensure_encoded(q, s));
    QAMD_TRY(q->ready.wait(s));
    if (out_mem == QAMD_MEM_DEVICE) {
        q->async_used.store(true, std::memory_order_relaxed);
        return scan_into(h, q, out, s);
    }
    return score_all_to_host(h->count, out, s, [&](float *scores) { return scan_into(h, q, scores, s); });
}

qamd_status qamd_u8_score_ids(const qamd_u8 *h, const qamd_u8_query *q, const uint32_t *ids, uint64_t n_ids,
                              qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream) {
    QAMD_TRY(check_query(h, q));
    if (n_ids == 0) return QAMD_OK;
    if (!ids || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    QAMD_TRY(ensure_encoded(q, s));
    QAMD_TRY(q->ready.wait(s));
    if (out_mem == QAMD_MEM_DEVICE) q->async_used.store(true, std::memory_order_relaxed);
    return score_ids_any(h, reinterpret_cast<const uint4 *>(q->buf.as<uint8_t>() + 16), q->buf.as<float>(), 0.0f, EPI_POINT,
                         ids, n_ids, ids_mem, out, out_mem, s);
}

// score_internal (:386-453) for one stored row against many: out[k] = score_internal(i, ids[k]).
qamd_status qamd_u8_score_internal_ids(const qamd_u8 *h, uint32_t i, const uint32_t *ids, uint64_t n_ids,
                                       qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (n_ids == 0) return QAMD_OK;
    if (!ids) QAMD_TRY(check_null_ids(n_ids, out, h->count));  // a null list stands for the rows 0 .. n_ids - 1
    else if (!out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (i >= h->count) return fail(QAMD_ERR_OUT_OF_RANGE, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint4 *qc = nullptr;
    const float *qo = nullptr;
    StreamBuf row;
    QAMD_TRY(stored_row_query(h, i, row, s, qc, qo));
    if (!ids) {  // score_internal_all's scan over a prefix of the store
        const ScanEpi e{internal_diff(h), EPI_INTERNAL, n_ids};
        if (out_mem == QAMD_MEM_DEVICE) return scan_ptrs(h, qc, qo, out, s, nullptr, e);
        return score_all_to_host(n_ids, out, s, [&](float *scores) { return scan_ptrs(h, qc, qo, scores, s, nullptr, e); });
    }
    return score_ids_any(h, qc, qo, internal_diff(h), EPI_INTERNAL, ids, n_ids, ids_mem, out, out_mem, s);
}

// Many stored rows, each against its own id list, in one launch (lists.hpp):
// out[p] = score_internal(rows[l], ids[p]) for p in [list_offsets[l], list_offsets[l + 1]).
qamd_status qamd_u8_score_internal_ids_batch(const qamd_u8 *h, const uint32_t *rows, const uint32_t *list_offsets,
                                             uint32_t n_lists, const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem,
                                             float *out, qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (n_lists && !rows) return fail(QAMD_ERR_ARGUMENTS, "rows is null");
    if (!ids && n_lists && n_ids) {  // the null-list form: every list is the rows 0 .. n_ids - 1 (lists.hpp)
        QAMD_TRY(check_null_lists(rows, list_offsets, n_lists, n_ids, lists_mem, out, out_mem, h->count));
        QAMD_ON_DEVICE(h->device);
        hipStream_t s = as_stream(stream);
        return run_null_lists(rows, n_lists, n_ids, lists_mem, out, out_mem, h->count, internal_batch_group(h), s,
                              [&](const uint32_t *rows_dev, uint32_t n, float *out_dev) {
                                  return score_internal_rows_dev(h, rows_dev, n, n_ids, out_dev, s);
                              });
    }
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    return run_lists(list_offsets, n_lists, ids, n_ids, rows, lists_mem, out, out_mem, h->count, s, [&](const ListArgs &a) {
        return score_pairs_dev(h, nullptr, nullptr, nullptr, 0, nullptr, a.offsets, a.n_lists, a.rows, internal_diff(h),
                               EPI_INTERNAL, a.ids, a.n_pairs, a.out, s);
    });
}

qamd_status qamd_u8_score_point(const qamd_u8 *h, const qamd_u8_query *q, uint32_t i, float *out) {
    return qamd_u8_score_ids(h, q, &i, 1, QAMD_MEM_HOST, out, QAMD_MEM_HOST, nullptr);
}

qamd_status qamd_u8_score_internal(const qamd_u8 *h, uint32_t i, uint32_t j, float *out) {
    if (!h || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    return qamd_u8_score_internal_ids(h, i, &j, 1, QAMD_MEM_HOST, out, QAMD_MEM_HOST, nullptr);
}

qamd_status qamd_u8_topk(const qamd_u8 *h, const qamd_u8_query *q, uint32_t k, int largest, uint32_t *out_ids,
                         float *out_scores, qamd_mem out_mem, void *stream) {
    QAMD_TRY(check_query(h, q));
    qamd_status args = QAMD_OK;
    if (!topk_wanted(k, 1, out_ids, out_scores, args)) return args;
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    if (q->deferred.load(std::memory_order_acquire)) {
        // a host query that has not been encoded yet: on a small store the search is ONE launch, the
        // top-k kernel quantises the query (passed by value) in its prologue and leaves the codes in the
        // query object
        std::unique_lock<std::mutex> lk(q->encode_mu);
        SmallTopkPlan plan;
        if (q->deferred.load(std::memory_order_relaxed) && u8_small_plan(h, k, plan)) {
            FusedQuery fq{q->host_f32.data(), (uint32_t)q->host_f32.size(), q->buf.as<uint8_t>()};
            if (out_mem == QAMD_MEM_DEVICE) q->async_used.store(true, std::memory_order_relaxed);
            qamd_status st = u8_topk_ptrs(h, q->buf.as<uint8_t>() + 16, q->buf.as<float>(), k, largest, out_ids, out_scores,
                                          out_mem, s, &fq);
            if (st == QAMD_OK) {
                st = q->ready.record(s);  // the codes are in the object once this launch has run
                q->deferred.store(false, std::memory_order_release);
            }
            return st;
        }
        lk.unlock();
        QAMD_TRY(ensure_encoded(q, s));
    }
    QAMD_TRY(q->ready.wait(s));
    if (out_mem == QAMD_MEM_DEVICE) q->async_used.store(true, std::memory_order_relaxed);
    return u8_topk_ptrs(h, q->buf.as<uint8_t>() + 16, q->buf.as<float>(), k, largest, out_ids, out_scores, out_mem, s);
}

void qamd_u8_free(qamd_u8 *h) { delete h; }

uint64_t qamd_u8_scan_bytes_per_row(const qamd_u8 *h) {
    if (h && h->image.kind == U8_IMAGE_NIBBLE) return 16ull * h->image.chunks + 4;  // the nibble image
    return h ? h->meta.actual_dim + 4 : 0;
}

// Selects how sums above 2^24 are rounded (0: once, 1: avx2.c lane order).  Not part of the
// reference surface; see the header of this file.
qamd_status qamd_u8_set_lane_mode(qamd_u8 *h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(QAMD_ERR_ARGUMENTS, "bad lane mode");
    h->lane_mode = mode;
    return QAMD_OK;
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
    const float levels = e->h->four_bit ? 15.0f : 127.0f;
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
                QAMD_TRY(launch_rot_values(e->sample.as<float>(), e->slice, dim, rot.as<float>(), e->stream));
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
    e->h->rotated = flags.rotated;
    e->h->four_bit = flags.four_bit;
    e->h->compact = flags.compact;
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

namespace qamd {

qamd_status u8_encode_queries_device(const qamd_u8 *h, const float *queries_dev, uint64_t n_queries, uint64_t qdim,
                                     uint8_t *codes_dev, uint64_t code_pitch, float *offsets_dev, hipStream_t stream) {
    if (n_queries == 0) return QAMD_OK;
    const qamd_vector_parameters &vp = h->meta.vector_parameters;
    StreamBuf rot;  // a rotated store: the codes come from the rotated queries, held until the encoder has run
    if (h->rotated) {
        if (qdim != vp.dim)
            return fail(QAMD_ERR_ARGUMENTS, "queries of %llu dimensions against rotated rows of %llu", (unsigned long long)qdim,
                        (unsigned long long)vp.dim);
        QAMD_TRY(rot.alloc(n_queries * qdim * sizeof(float), stream));
        QAMD_TRY(launch_rot_values(queries_dev, n_queries, qdim, rot.as<float>(), stream));
        queries_dev = rot.as<float>();
    }
    hipLaunchKernelGGL(encode_queries_kernel, dim3((unsigned)n_queries), dim3(64), 0, stream, queries_dev,
                       (uint32_t)qdim, (uint32_t)actual_dim_of(qdim), h->meta.alpha, h->meta.offset,
                       vp.distance_type, vp.invert, codes_dev, (uint32_t)code_pitch, offsets_dev, (int)h->four_bit);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// The top-k of one query given as raw device pointers (its codes and its offset): the body of
// qamd_u8_topk, also the per-query route of the batch API, which hands in rows of a query batch
// without copying them into a query object.  Runs on the current device.
// `e`: the epilogue of every route - an encoded query's, or score_internal's with (codes_dev, qo) a stored row
// (qamd_u8_topk_internal); the routing predicates are the same for both.
static qamd_status topk_ptrs_epi(const qamd_u8 *h, const uint8_t *codes_dev, const float *qo, uint32_t k, int largest,
                                 uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t s, const FusedQuery *fq,
                                 const ScanEpi &e) {
    const uint4 *qc = reinterpret_cast<const uint4 *>(codes_dev);
    FusedScan scan;
    scan.scan_scores = [&](float *scores, hipStream_t st) { return scan_ptrs(h, qc, qo, scores, st, nullptr, e); };
    scan.scan_filter = [&](const TopkFilter &f, hipStream_t st) { return scan_ptrs(h, qc, qo, nullptr, st, &f, e); };
    scan.score_ids = [&](const uint32_t *ids, uint64_t n_ids, float *out, hipStream_t st) {
        return score_ids_dev(h, qc, qo, e.diff, e.mode, ids, n_ids, out, st);
    };
    {   // small stores: one launch, no status read-back (device outputs only enqueue)
        SmallTopkPlan plan;
        if (u8_small_plan(h, k, plan)) {
            const bool is_l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
            return small_topk(plan, k, largest, out_ids, out_scores, out_mem, s,
                              [&](const SmallTopk &p, hipStream_t st) {
                                  return is_l1 ? launch_small<true>(h, qc, qo, fq, plan, p, st, e)
                                               : launch_small<false>(h, qc, qo, fq, plan, p, st, e);
                              });
        }
    }
    if (fq) return fail(QAMD_ERR_ARGUMENTS, "a deferred query needs the single-launch path");
    if (!fused_capable(h)) {  // rare layouts: classic path only
        return topk_classic(h->count, k, largest, out_ids, out_scores, out_mem, s,
                            [&](float *scores) { return scan_ptrs(h, qc, qo, scores, s, nullptr, e); });
    }
    return fused_topk(h->count, k, largest, out_ids, out_scores, out_mem, s, scan);
}

qamd_status u8_topk_ptrs(const qamd_u8 *h, const uint8_t *codes_dev, const float *qo, uint32_t k, int largest,
                         uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t s, const FusedQuery *fq) {
    return topk_ptrs_epi(h, codes_dev, qo, k, largest, out_ids, out_scores, out_mem, s, fq, ScanEpi{});
}

// score_internal (encoded_vectors_u8.rs:386-453) against the whole store: the "query" is row i of the byte
// codes with its stored offset - the packed image's scan reads its query as byte codes too - and every route ends in
// score_internal's epilogue.
static ScanEpi internal_epi(const qamd_u8 *h) { return ScanEpi{internal_diff(h), EPI_INTERNAL}; }

static qamd_status u8_score_internal_all(const qamd_u8 *h, uint32_t i, float *out, qamd_mem out_mem, hipStream_t s) {
    const uint4 *qc = nullptr;
    const float *qo = nullptr;
    StreamBuf row;  // a compact store unpacks row i out of its image
    QAMD_TRY(stored_row_query(h, i, row, s, qc, qo));
    const ScanEpi e = internal_epi(h);
    if (out_mem == QAMD_MEM_DEVICE) return scan_ptrs(h, qc, qo, out, s, nullptr, e);
    return score_all_to_host(h->count, out, s, [&](float *scores) { return scan_ptrs(h, qc, qo, scores, s, nullptr, e); });
}

static qamd_status u8_topk_internal(const qamd_u8 *h, uint32_t i, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                             qamd_mem out_mem, hipStream_t s) {
    const uint4 *qc = nullptr;
    const float *qo = nullptr;
    StreamBuf row;
    QAMD_TRY(stored_row_query(h, i, row, s, qc, qo));
    return topk_ptrs_epi(h, reinterpret_cast<const uint8_t *>(qc), qo, k, largest, out_ids, out_scores, out_mem, s, nullptr,
                         internal_epi(h));
}

// The batch API for the metrics with no matrix form (L1: sum |q - v| is not a contraction): the
// per-query fused pipelines of all queries enqueued back to back (fused_topk_batch), one status
// read-back per 32 queries.  codes_dev: [Q][pitch], offsets_dev: [Q].
qamd_status u8_topk_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                uint32_t n_queries, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                                qamd_mem out_mem, hipStream_t stream) {
    auto qc = [&](uint32_t q) { return reinterpret_cast<const uint4 *>(codes_dev + (uint64_t)q * pitch); };
    BatchScan scan;
    scan.filter_capable = fused_capable(h);
    scan.scan_scores = [&](uint32_t q, float *scores, hipStream_t st) { return scan_ptrs(h, qc(q), offsets_dev + q, scores, st); };
    scan.scan_filter = [&](uint32_t q, const TopkFilter &f, hipStream_t st) {
        return scan_ptrs(h, qc(q), offsets_dev + q, nullptr, st, &f);
    };
    scan.score_ids = [&](uint32_t q, const uint32_t *ids, uint64_t n_ids, float *out, hipStream_t st) {
        return score_ids_dev(h, qc(q), offsets_dev + q, 0.0f, EPI_POINT, ids, n_ids, out, st);
    };
    const bool is_l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
    const uint32_t width = multi_width(h);
    if (width)  // one filtering pass over the rows for up to `width` queries
        scan.scan_filter_multi = [&, width, is_l1](uint32_t q, uint32_t left, const TopkFilterSlices &sl, hipStream_t st,
                                                   qamd_status &status) -> uint32_t {
            const uint32_t nq = std::min(left, width);
            if (nq < 2) return 0;
            const uint8_t *qcodes = codes_dev + (uint64_t)q * pitch;
            const bool ok = is_l1 ? launch_multi<true>(h, nq, qcodes, pitch, offsets_dev + q, nullptr, &sl, st)
                                  : launch_multi<false>(h, nq, qcodes, pitch, offsets_dev + q, nullptr, &sl, st);
            if (ok && hipGetLastError() != hipSuccess) status = fail(QAMD_ERR_DEVICE, "u8 multi-query filter launch failed");
            return ok ? nq : 0;
        };
    return fused_topk_batch(h->count, n_queries, k, largest, out_ids, out_scores, out_mem, stream, scan);
}

bool u8_host_encode_is_lazy(uint64_t qdim) { return qdim > 0 && actual_dim_of(qdim) <= kFusedQueryDims; }

// score_ids_batch: query l of a batch ([q][pitch] codes, [q] offsets) against list l (lists.hpp).
qamd_status u8_score_lists(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                           const ListArgs &a, hipStream_t stream) {
    return score_pairs_dev(h, nullptr, nullptr, codes_dev, (uint32_t)pitch, offsets_dev, a.offsets, a.n_lists, nullptr, 0.0f,
                           EPI_POINT, a.ids, a.n_pairs, a.out, stream);
}

// How many queries the vector-ALU multi-query scan takes per pass for this store (0: none).
uint32_t u8_multi_width(const qamd_u8 *h) { return multi_width(h); }

// Lane mode 1 on a Dot / L2 store: the batch API must take the per-query scans (the matrix cores sum exactly).  So must
// a compact store: the matrix-core kernels and the multi-query scan read byte codes, which it has not.
bool u8_batch_by_scans(const qamd_u8 *h) { return lane_order(h) || h->compact; }

void no_byte_codes() {
    std::fprintf(stderr, "quantization_amd: a route asked for the byte codes of a compact u8 store (DESIGN 3.1z)\n");
    std::abort();
}

// out[j * count + row] for queries [0, n_queries) of a batch through the multi-query scan (groups of
// `width`, then smaller groups, then single scans).
qamd_status u8_score_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                 uint32_t n_queries, float *out_dev, hipStream_t stream) {
    const bool is_l1 = h->meta.vector_parameters.distance_type == QAMD_L1;
    const uint32_t width = multi_width(h);
    uint32_t q = 0;
    while (q < n_queries) {
        const uint32_t nq = std::min(width, n_queries - q);
        const uint8_t *qcodes = codes_dev + (uint64_t)q * pitch;
        float *o = out_dev + (uint64_t)q * h->count;
        const bool ok = nq >= 2 && (is_l1 ? launch_multi<true>(h, nq, qcodes, pitch, offsets_dev + q, o, nullptr, stream)
                                          : launch_multi<false>(h, nq, qcodes, pitch, offsets_dev + q, o, nullptr, stream));
        if (ok) {
            q += nq;
        } else {
            QAMD_TRY(scan_ptrs(h, reinterpret_cast<const uint4 *>(qcodes), offsets_dev + q, o, stream));
            q += 1;
        }
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// Exact single-query top-k for one member of a query batch (its per-query fallback): no copy, no
// allocation; on small stores (single-launch path) with device outputs it only enqueues.
qamd_status u8_topk_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, uint32_t k,
                           int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t stream) {
    return u8_topk_ptrs(h, codes_dev, offset_dev, k, largest, out_ids, out_scores, out_mem, stream, nullptr);
}

// score_all for one member of a query batch (the L1 route of the batch API: L1 has no MFMA form).
qamd_status u8_score_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, float *out_dev,
                            hipStream_t stream) {
    return scan_ptrs(h, reinterpret_cast<const uint4 *>(codes_dev), offset_dev, out_dev, stream);
}

}  // namespace qamd

extern "C" {

qamd_status qamd_u8_score_internal_all(const qamd_u8 *h, uint32_t i, float *out, qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (h->count == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "out is null");
    if (i >= h->count) return fail(QAMD_ERR_ARGUMENTS, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    return u8_score_internal_all(h, i, out, out_mem, as_stream(stream));
}

qamd_status qamd_u8_topk_internal(const qamd_u8 *h, uint32_t i, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                                  qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    qamd_status args = QAMD_OK;
    if (!topk_wanted(k, 1, out_ids, out_scores, args)) return args;
    if (h->count && i >= h->count)
        return fail(QAMD_ERR_ARGUMENTS, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    return u8_topk_internal(h, i, k, largest, out_ids, out_scores, out_mem, as_stream(stream));
}

}  // extern "C"

#ifdef QAMD_DEV
// Developer-only accessors for the tuning harness (tune.hip): libquantization_amd_dev.so only.
extern "C" __attribute__((visibility("default"))) void qamd_dev_u8_ptrs(const qamd_u8 *h, const void **codes,
                                                                        const void **offsets) {
    *codes = h->codes.ptr;
    *offsets = h->offsets.ptr;
}
extern "C" __attribute__((visibility("default"))) const void *qamd_dev_u8_query_ptr(const qamd_u8_query *q) {
    return q->buf.ptr;
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
// Which image the store's last scan launch read (U8Image::kind), and how many waves per block its last blocked scan took.
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_scan_split(const qamd_u8 *h) {
    return h->last_scan_split.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_scan_packed(const qamd_u8 *h) {
    return h->last_scan_packed.load(std::memory_order_relaxed);
}
#endif

// ============================================================================= rescoring with the original vectors
// rerank(orig, query_f32, ids of topk(h, q, candidates, largest), k): one body for the three quantizers (rescore.hpp).
extern "C" qamd_status qamd_u8_topk_rescored(const qamd_u8 *h, const qamd_u8_query *q, const qamd_f32 *orig,
                                              const float *query_f32, uint64_t qdim, qamd_mem query_mem, uint32_t k,
                                              uint32_t candidates, int largest, uint32_t *out_ids, float *out_scores,
                                              qamd_mem out_mem, void *stream) {
    if (!h || !q) return qamd::fail(QAMD_ERR_ARGUMENTS, "null handle or query");
    return qamd::topk_rescored(h->device, h->meta.vector_parameters, orig, query_f32, 1, qdim, query_mem, k, candidates, largest, out_ids,
                               out_scores, out_mem, qamd::as_stream(stream), [&](uint32_t *ids_dev, float *scores_dev) {
                                   return qamd_u8_topk(h, q, candidates, largest, ids_dev, scores_dev, QAMD_MEM_DEVICE, stream);
                               });
}
