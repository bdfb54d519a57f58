// Binary quantizer on MI355X (gfx950): sign-bit packing and the XOR+popcount scan.
//
// Host side mirrors EncodedVectorsBin (quantization/src/encoded_vectors_binary.rs); the scan
// replaces impl_xor_popcnt_sse_uint{128,64,32} (quantization/cpp/sse.c:49-106), which the
// reference calls once per (query, row) pair.
//
// HBM layout: rows keep the reference's byte layout (bit i of a vector = byte i/8, bit i%8,
// identical for the u8 and u128 store types on little-endian, :193-208).  Device stride `ds`
// is the reference's row size for rows >= 8 bytes (always a multiple of 8; of 16 above 128
// dims, e.g. 128 B at dim 1024) and 4 bytes for the tiny rows (dim <= 32, 0..4 bytes).  Pad
// bits are zero in rows and query alike, so they never reach the popcount (:36-37).
//
// Scan mapping: as the u8 scan — G lanes read one row in 16-byte pieces, one wave-load covers
// 64/G consecutive rows — with v_xor + v_bcnt_u32_b32 instead of v_dot4.  All integer, exact;
// the f32 metric (:219-253) is exact for dim < 2^23.
//
// Many queries at once run on the matrix cores, where popcount(q AND v) is a dot product of 0/1 values: from 12 queries
// bin_gemm_rs_kernel (bits expanded to bytes in registers, int8 MFMA), from 129 queries on rows of 512 / 768 / 1024 / 1536
// bits bin_gemm_qs4_kernel (bits expanded once per row block to E2M1 nibbles in LDS, FP4 MFMA with exact f32 counts, the
// batch streamed past the block).  Both end in the reference's calculate_metric on the integer count: bit-identical.
#include <algorithm>
#include <memory>
#include <vector>

#include <mutex>

#include "batch_common.hpp"
#include "bin_batch_route.hpp"
#include "common.hpp"
#include "lists.hpp"
#include "multi_reduce.hpp"
#include "topk.hpp"
#include "topk_device.hpp"
#include "rescore.hpp"
#include "rotate_blocks.hpp"

#pragma clang fp contract(off)

using namespace qamd;
using namespace qamd::rot;

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 512;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_nt(const uint4 *p) {
    u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ uint32_t xpop16(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc += __popc(a.x ^ b.x);
    acc += __popc(a.y ^ b.y);
    acc += __popc(a.z ^ b.z);
    acc += __popc(a.w ^ b.w);
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

// encoded_vectors_binary.rs:237-252 calculate_metric
__device__ __forceinline__ float metric(uint32_t x, float dim_f, int is_dot, int invert) {
    const float xor_product = (float)x;
    const float zeros_count = dim_f - xor_product;
    const bool zx = (is_dot != 0) != (invert != 0);  // Dot,!invert and L1/L2,invert -> zeros - xor
    return zx ? zeros_count - xor_product : xor_product - zeros_count;
}

// Scalar queries (the reference has no counterpart): the query is PLANES bit planes of 4- or 8-bit
// codes, plane b one device row stride after plane b - 1, and a row's X = sum_b 2^b popcount(plane_b xor row).
// One 16-byte piece (or dword) of a row against the same piece of every plane:
// PLANES x (4 v_xor + 4 v_bcnt) and one v_lshl_add into the row's single accumulator.
template <int PLANES> __device__ __forceinline__ uint32_t xpop16_planes(const uint4 &v, const uint4 (&q)[PLANES], uint32_t acc) {
#pragma unroll
    for (int b = 0; b < PLANES; b++) acc += xpop16(v, q[b], 0u) << b;
    return acc;
}
template <int PLANES> __device__ __forceinline__ uint32_t xpop_planes(uint32_t v, const uint32_t *q, uint32_t stride, uint32_t acc) {
#pragma unroll
    for (int b = 0; b < PLANES; b++) acc += (uint32_t)__popc(v ^ q[(size_t)b * stride]) << b;
    return acc;
}

// Rows of ds >= 16 bytes (row_chunks = ds/16).  One wave per tile of (64/G)*UNROLL rows,
// non-persistent grid (same reasoning and measurements as u8_scan_kernel in u8.hip).
// PLANES > 1: qbits holds the planes of a scalar query at a stride of row_chunks pieces and dim_f is dim * (2^PLANES - 1).
// The planes are used one piece index at a time, PLANES x 4 registers, and read through L1 / L2 (the query is at most 8 rows
// long); the compiler is free to fetch them early and does for the long rows, which then run at 2-3 waves per SIMD
// instead of 7-8 - still without scratch (resource report).
template <int G, int ITERS, int UNROLL, bool EXACT, bool FILTER, int PLANES = 1>
__global__ __launch_bounds__(kScanBlock) void bin_scan_kernel(const uint4 *__restrict__ rows,
                                                             const uint4 *__restrict__ qbits, float dim_f,
                                                             int is_dot, int invert, uint32_t n_rows,
                                                             uint32_t row_chunks, float *__restrict__ out,
                                                             TopkFilter filt) {
    constexpr int RW = 64 / G;
    constexpr int TILE = RW * UNROLL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    const uint64_t base = wave * TILE;
    if (base >= n_rows) return;
    uint4 q[ITERS];
    if (PLANES == 1) {
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            if (EXACT) {
                q[it] = qbits[c];
            } else {
                const uint4 t = qbits[c < row_chunks ? c : row_chunks - 1];
                const bool in = c < row_chunks;
                q[it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
        }
    }
    uint4 v[UNROLL][ITERS];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        const uint64_t row = base + u * RW + rslot;
        const uint4 *p = rows + row * row_chunks;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            if (EXACT) {
                v[u][it] = ld_nt(p + c);
            } else {  // masked lane: read the row's last chunk, then xor against itself -> 0 bits
                const bool in = c < row_chunks;
                uint4 t = ld_nt(p + (in ? c : row_chunks - 1));
                if (PLANES == 1) v[u][it] = in ? t : q[it];
                else v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);  // and zero plane pieces
            }
        }
    }
    uint32_t x[UNROLL];
    if (PLANES > 1) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) x[u] = 0;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            const bool in = EXACT || c < row_chunks;
            uint4 qp[PLANES];
#pragma unroll
            for (int b = 0; b < PLANES; b++) {
                const uint4 t = qbits[(size_t)b * row_chunks + (in ? c : row_chunks - 1)];
                qp[b] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) x[u] = xpop16_planes<PLANES>(v[u][it], qp, x[u]);
        }
    }
    float mine = 0.0f;  // lane (rslot, sub = u % G) keeps row u's score: one coalesced nt store per G rows-groups
    uint32_t pivot = 0;
    if (FILTER) pivot = *filt.pivot_key;
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        uint32_t acc = 0;
        if (PLANES == 1) {
#pragma unroll
            for (int it = 0; it < ITERS; it++) acc = xpop16(v[u][it], q[it], acc);
        } else {
            acc = x[u];
        }
        acc = group_sum<G>(acc);
        if (sub == (u % G)) mine = metric(acc, dim_f, is_dot, invert);
        if ((u % G) == G - 1 || u == UNROLL - 1) {
            const int first = (u / G) * G;
            const uint64_t row = base + (uint64_t)(first + sub) * RW + rslot;
            if (sub <= u - first && row < n_rows) {
                if (FILTER) topk_offer(filt, pivot, mine, (uint32_t)row);
                else __builtin_nontemporal_store(mine, out + row);
            }
        }
    }
}

// NQ queries per row read (qamd_bin_score_batch): the row's 16-byte pieces are loaded once and
// xor-popcounted against NQ query rows held in registers, so the HBM bytes per (query, row) pair fall
// from ds + 4 to ds / NQ + 4 and the scan turns from HBM-bound into popcount-bound.
// Lane (row slot, sub = j) keeps query j's score of the row: one store instruction per row slot
// writes NQ segments of 64/G consecutive floats.  G >= NQ.
// FILTER: no score is written; lane (row slot, sub = j) offers its row to query j's candidate lists
// (fused top-k of NQ queries in one pass: qamd_bin_topk_batch).
template <int G, int ITERS, int UNROLL, int NQ, bool EXACT, bool FILTER>
__global__ __launch_bounds__(kScanBlock) void bin_scan_multi_kernel(const uint4 *__restrict__ rows,
                                                                   const uint4 *__restrict__ qbits /* [NQ][q_stride] */,
                                                                   uint32_t q_stride, float dim_f, int is_dot, int invert,
                                                                   uint32_t n_rows, uint32_t row_chunks,
                                                                   float *__restrict__ out /* [NQ][out_pitch] */,
                                                                   uint64_t out_pitch, TopkFilterSlices slices) {
    static_assert(G >= NQ, "one lane of the row group per query");
    constexpr int RW = 64 / G;
    constexpr int TILE = RW * UNROLL;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kScanBlock + threadIdx.x) >> 6;
    const uint64_t base = wave * TILE;
    if (base >= n_rows) return;
    uint4 q[NQ][ITERS];
#pragma unroll
    for (int j = 0; j < NQ; j++) {
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            const bool in = EXACT || c < row_chunks;
            const uint4 t = qbits[(size_t)j * q_stride + (in ? c : row_chunks - 1)];
            q[j][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
        }
    }
    uint4 v[UNROLL][ITERS];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        const uint64_t row = base + u * RW + rslot;
        const uint4 *p = rows + row * row_chunks;
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            const bool in = EXACT || c < row_chunks;
            const uint4 t = ld_nt(p + (in ? c : row_chunks - 1));
            v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
        }
    }
    // lane (row slot, sub) ends up with the total of query multi_query_of<NQ>(sub) (multi_reduce.hpp):
    // the lanes whose sub is below NQ own one query each
    const int my_q = multi_query_of<NQ>(sub);
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
        uint32_t acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            acc[j] = 0;
#pragma unroll
            for (int it = 0; it < ITERS; it++) acc[j] = xpop16(v[u][it], q[j][it], acc[j]);
        }
        const float mine = metric(multi_reduce<G, NQ>(acc, sub), dim_f, is_dot, invert);
        const uint64_t row = base + (uint64_t)u * RW + rslot;
        if (sub < NQ && row < n_rows) {
            if (FILTER) {
                const TopkFilter f = topk_filter_of(slices, (uint32_t)my_q);
                topk_offer(f, *f.pivot_key, mine, (uint32_t)row);  // the pivot is an L2-resident word, re-read per row slot
            } else {
                __builtin_nontemporal_store(mine, out + (uint64_t)my_q * out_pitch + row);
            }
        }
    }
}

// Single-launch top-k for small stores (topk.hpp small_topk; the scalar-u8 twin in u8.hip explains
// the structure): workgroup b scores rows [b * rows_per_wg, (b + 1) * rows_per_wg) with
// bin_scan_kernel's arithmetic; scores become 64-bit keys in the wave's LDS staging row and the
// wave / workgroup / last-arriver merges of topk_device.hpp keep the best k.  Exact under any
// number of ties (keys are distinct: score bits << 32 | row), which the sampled-pivot path is not
// good at for binary scores (few distinct values -> candidate lists overflow -> classic fallback).
template <int G, int ITERS, bool EXACT, int PLANES = 1>
__global__ __launch_bounds__(1024) void bin_topk_small_kernel(const uint4 *__restrict__ rows,
                                                              const uint4 *__restrict__ qbits, float dim_f, int is_dot,
                                                              int invert, uint32_t n_rows, uint32_t row_chunks,
                                                              uint32_t rows_per_wg, SmallTopk p) {
    __shared__ unsigned long long lds[2 * kSmallTopkWaves][64];
    unsigned long long(*lists)[64] = lds;
    constexpr int RW = 64 / G;
    constexpr int UNROLL = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % G, rslot = lane / G;
    unsigned long long *stage = lds[kSmallTopkWaves + wave];
    uint4 q[ITERS];
    if (PLANES == 1) {
#pragma unroll
        for (int it = 0; it < ITERS; it++) {
            const uint32_t c = sub + it * G;
            const bool in = EXACT || c < row_chunks;
            const uint4 t = qbits[in ? c : row_chunks - 1];
            q[it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
        }
    }
    const uint64_t wg_base = (uint64_t)blockIdx.x * rows_per_wg;
    SmallTopkWave acc_list;
    for (uint32_t tile = wave * UNROLL; tile * RW < rows_per_wg; tile += kSmallTopkWaves * UNROLL) {
        uint4 v[UNROLL][ITERS];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint64_t row = wg_base + (uint64_t)(tile + u) * RW + rslot;
            const uint64_t rc = row < n_rows ? row : (uint64_t)n_rows - 1;
            const uint4 *src = rows + rc * row_chunks;
#pragma unroll
            for (int it = 0; it < ITERS; it++) {
                const uint32_t c = sub + it * G;
                const bool in = EXACT || c < row_chunks;
                const uint4 t = ld_nt(src + (in ? c : row_chunks - 1));
                v[u][it] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
            }
        }
        uint32_t x[UNROLL];
        if (PLANES > 1) {  // as in bin_scan_kernel: the planes of one piece at a time
#pragma unroll
            for (int u = 0; u < UNROLL; u++) x[u] = 0;
#pragma unroll
            for (int it = 0; it < ITERS; it++) {
                const uint32_t c = sub + it * G;
                const bool in = EXACT || c < row_chunks;
                uint4 qp[PLANES];
#pragma unroll
                for (int b = 0; b < PLANES; b++) {
                    const uint4 t = qbits[(size_t)b * row_chunks + (in ? c : row_chunks - 1)];
                    qp[b] = make_uint4(in ? t.x : 0, in ? t.y : 0, in ? t.z : 0, in ? t.w : 0);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; u++) x[u] = xpop16_planes<PLANES>(v[u][it], qp, x[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint32_t local = (tile + u) * RW + rslot;
            const uint64_t row = wg_base + local;
            uint32_t acc = 0;
            if (PLANES == 1) {
#pragma unroll
                for (int it = 0; it < ITERS; it++) acc = xpop16(v[u][it], q[it], acc);
            } else {
                acc = x[u];
            }
            acc = group_sum<G>(acc);
            if (sub == 0) {
                unsigned long long key = ~0ull;
                if (local < rows_per_wg && row < n_rows)
                    key = ((unsigned long long)topk_ordered_bits(metric(acc, dim_f, is_dot, invert), p.largest != 0) << 32) |
                          (uint32_t)row;
                stage[acc_list.fill + rslot] = key;
            }
            acc_list.fill += RW;
            if (acc_list.fill == 64) small_topk_flush(acc_list, stage, lane);
        }
    }
    if (acc_list.fill) small_topk_flush(acc_list, stage, lane);
    small_topk_finish(acc_list.best, lists, p);
}

// Any row size, dword granularity: used for tiny rows (ds 4 or 8), very long rows and the
// random-access entry points.  ids == nullptr scans rows [0, n).  PLANES > 1: plane b of a scalar query is at
// qbits + b * row_words.
template <int PLANES = 1>
__global__ __launch_bounds__(kBlock) void bin_words_kernel(const uint32_t *__restrict__ rows,
                                                          const uint32_t *qbits, float dim_f, int is_dot,
                                                          int invert, const uint32_t *__restrict__ ids,
                                                          uint64_t n, uint32_t n_rows, uint32_t row_words,
                                                          float *__restrict__ out) {
    constexpr int G = 16, RW = 4;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, rslot = lane / G;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t base = wave * RW; base < n; base += n_waves * RW) {
        const uint64_t k = base + rslot;
        const uint32_t row = k < n ? (ids ? ids[k] : (uint32_t)k) : 0xFFFFFFFFu;
        const bool ok = row < n_rows;
        uint32_t acc = 0;
        if (ok) {
            const uint32_t *p = rows + (uint64_t)row * row_words;
            if (PLANES == 1) {
                for (uint32_t w = sub; w < row_words; w += G) acc += __popc(p[w] ^ qbits[w]);
            } else {
                for (uint32_t w = sub; w < row_words; w += G) acc = xpop_planes<PLANES>(p[w], qbits + w, row_words, acc);
            }
        }
        acc = group_sum<G>(acc);
        if (sub == 0 && k < n) out[k] = ok ? metric(acc, dim_f, is_dot, invert) : __builtin_nanf("");
    }
}

// Random access for bursts of pairs (lists.hpp): out[k] = metric(row ids[k] xor the query of pair k).
// Which query: `lists` == nullptr -> q_single for every pair (it may be a stored row: score_internal is
// the same metric on two stored rows, encoded_vectors_binary.rs:302-314); lists, list_rows == nullptr ->
// bit row l of a query batch for the pairs of list l; lists and list_rows -> stored row list_rows[l].
// VEC16 (ds % 16 == 0): 8 lanes per pair, 16-byte pieces, up to four in flight per lane; else 16 lanes
// per pair at dword granularity (rows of 4 and 8 bytes).
// PLANES > 1: the query is the planes of a scalar query, plane b at + b * row_words dwords: q_single, or with lists the
// planes of query l of a scalar batch at q_batch + l * q_stride.  A stored row (score_internal, list_rows) is one plane.
template <bool VEC16, int PLANES = 1>
__global__ __launch_bounds__(kBlock) void bin_pairs_kernel(const uint32_t *__restrict__ rows, const uint32_t *q_single,
                                                          const uint8_t *__restrict__ q_batch, uint32_t q_stride,
                                                          const uint32_t *__restrict__ lists, uint32_t n_lists,
                                                          const uint32_t *__restrict__ list_rows, float dim_f, int is_dot,
                                                          int invert, const uint32_t *__restrict__ ids, uint64_t n,
                                                          uint32_t n_rows, uint32_t row_words, uint32_t pairs_per_block,
                                                          float *__restrict__ out) {
    constexpr int G = VEC16 ? 8 : 16, GROUPS = kBlock / G;
    __shared__ uint32_t first_list;
    const int lane = threadIdx.x & 63;
    const int sub = lane % G, group = threadIdx.x / G;
    const uint64_t p0 = (uint64_t)blockIdx.x * pairs_per_block;
    const uint64_t p1 = p0 + pairs_per_block < n ? p0 + pairs_per_block : n;
    uint32_t l = lists ? first_list_of_block(lists, n_lists, p0, &first_list) : 0u;  // (lists.hpp)
    for (uint64_t k = p0 + group; k < p1; k += GROUPS) {
        const uint32_t row = ids[k];
        bool ok = row < n_rows;
        const uint32_t *qp = q_single;
        if (lists) {
            l = advance_list(lists, n_lists, l, k);
            if (list_rows) {
                const uint32_t qr = list_rows[l];
                ok = ok && qr < n_rows;
                qp = rows + (uint64_t)(qr < n_rows ? qr : 0u) * row_words;
            } else {
                qp = reinterpret_cast<const uint32_t *>(q_batch + (size_t)l * q_stride);
            }
        }
        const uint32_t *p = rows + (uint64_t)(ok ? row : 0u) * row_words;
        uint32_t acc = 0;
        if (VEC16) {
            const uint32_t chunks = row_words / 4;
            const uint4 *p4 = reinterpret_cast<const uint4 *>(p), *q4 = reinterpret_cast<const uint4 *>(qp);
            if (PLANES > 1) {
                for (uint32_t c = sub; c < chunks; c += G) {
                    const uint4 v = p4[c];
                    uint4 qp[PLANES];
#pragma unroll
                    for (int b = 0; b < PLANES; b++) qp[b] = q4[(size_t)b * chunks + c];
                    acc = xpop16_planes<PLANES>(v, qp, acc);
                }
            } else if (chunks <= (uint32_t)G) {  // the common rows (<= 1024 bits): one 16-byte piece per lane
                if ((uint32_t)sub < chunks) acc = xpop16(p4[sub], q4[sub], acc);
            } else {
                for (uint32_t c0 = sub; c0 < chunks; c0 += 4 * G) {
                    uint4 v[4], qv[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t c = c0 + j * G, cc = c < chunks ? c : chunks - 1;
                        v[j] = p4[cc];
                        qv[j] = q4[cc];
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (c0 + j * G < chunks) acc = xpop16(v[j], qv[j], acc);
                }
            }
        } else if (PLANES > 1) {
            for (uint32_t w = sub; w < row_words; w += G) acc = xpop_planes<PLANES>(p[w], qp + w, row_words, acc);
        } else {
            for (uint32_t w = sub; w < row_words; w += G) acc += __popc(p[w] ^ qp[w]);
        }
        acc = group_sum<G>(acc);
        if (sub == 0) out[k] = ok ? metric(acc, dim_f, is_dot, invert) : __builtin_nanf("");
    }
}

// encode_vector (:193-208): one wave per row, 64 elements per ballot; lane (step % 64) keeps
// the ballot of `step`, so after <= 64 steps every lane owns 8 output bytes (coalesced store).
__global__ __launch_bounds__(kBlock) void bin_encode_kernel(const float *__restrict__ data, uint64_t n_rows,
                                                           uint32_t dim, uint32_t row_words,
                                                           uint32_t *__restrict__ rows, uint64_t row0) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint32_t steps = (dim + 63) / 64;
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const float *src = data + r * dim;
        uint32_t *dst = rows + (row0 + r) * row_words;
        unsigned long long mine = 0;
        for (uint32_t st = 0; st < steps; st++) {
            const uint32_t j = st * 64 + lane;
            const float v = j < dim ? src[j] : 0.0f;
            const unsigned long long b = __ballot(v > 0.0f);
            if ((st & 63u) == (uint32_t)lane) mine = b;
            if ((st & 63u) == 63u || st + 1 == steps) {
                const uint32_t w = ((st & ~63u) + lane) * 2;  // this lane's first dword
                if (w < row_words) dst[w] = (uint32_t)mine;
                if (w + 1 < row_words) dst[w + 1] = (uint32_t)(mine >> 32);
                mine = 0;
            }
        }
    }
}

// encode_vector, streaming form for stores whose rows are whole 128-bit words with no row
// padding (dim % 128 == 0): the batch is one flat stream of floats -> bits.  One wave per
// 16 KiB tile; wave-load j reads 64 consecutive float4 (nt), each lane turns its four signs
// into a nibble at bit 4*(lane%8), a 3-step DPP add over the 8-lane group (disjoint fields, so
// add == or) hands every lane of the group the finished dword, and lane 8g+t keeps the one of
// wave-load t (and t+8): after 16 loads a lane owns two dwords and the wave writes 2 x 256 B.
__global__ __launch_bounds__(kBlock) void bin_encode_flat_kernel(const float4 *__restrict__ d4, uint64_t n4,
                                                                uint32_t *__restrict__ words /* n4/8 dwords */) {
    const int lane = threadIdx.x & 63, t = lane & 7, g = lane >> 3;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t base = wave * 1024;
    if (base >= n4) return;
    float4 v[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint64_t i = base + j * 64 + lane;
        v[j] = i < n4 ? __builtin_bit_cast(float4, ld_nt(reinterpret_cast<const uint4 *>(d4) + i))
                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    uint32_t keep[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        uint32_t nib = (v[j].x > 0.0f ? 1u : 0u) | (v[j].y > 0.0f ? 2u : 0u) | (v[j].z > 0.0f ? 4u : 0u) |
                       (v[j].w > 0.0f ? 8u : 0u);
        const uint32_t dw = group_sum<8>(nib << (4 * t));
        if ((j & 7) == t) keep[j >> 3] = dw;
    }
    const uint64_t n_words = n4 / 8;
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const uint64_t w = wave * 128 + hf * 64 + t * 8 + g;  // wave-load (hf*8 + t), group g
        if (w < n_words) words[w] = keep[hf];
    }
}

// ---- two-bit rows (the reference has no counterpart) ----
// Per-dimension statistics.  The definition fixes the order of every addition, so the result does not depend on how a
// caller batches the rows: column i's rows are cut into blocks of kStatRows by row index, a block's S = sum (double)x and
// Q = sum (double)x * (double)x run in row order from +0.0 over its finite entries (n counts them), and the block sums are
// added in block order (bin_stats_fold_kernel).  No floating-point atomics, no tree.
// One workgroup of 64 lanes takes block blockIdx.x of the launch and 256 columns; a lane owns four adjacent columns and
// walks the block's rows, eight rows in flight: consecutive lanes read consecutive 16-byte pieces of a row.  VEC: dim % 4 ==
// 0 and a 16-byte aligned source; otherwise four guarded dword loads.  The eight loads of a step must all be issued
// before the first wait: nothing conditional may stand between them and the adds.  A non-finite entry adds +0.0, which leaves a sum
// that started at +0.0 unchanged bit for bit (it can never be -0.0).
// `fill` rows of the launch's first block came with earlier launches: their sums are the carry the block starts from, and
// the block takes only kStatRows - fill rows here.
constexpr uint32_t kStatRows = 4096;

template <bool VEC>
__global__ __launch_bounds__(64) void bin_stats_kernel(const float *__restrict__ data, uint64_t n_rows, uint32_t dim,
                                                      uint32_t fill, const double *__restrict__ carry_s,
                                                      const double *__restrict__ carry_q,
                                                      const uint32_t *__restrict__ carry_n, double *__restrict__ part_s,
                                                      double *__restrict__ part_q, uint32_t *__restrict__ part_n) {
    const uint64_t b = blockIdx.x;
    const uint32_t c0 = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (c0 >= dim) return;
    const uint64_t r0 = b ? b * kStatRows - fill : 0;
    const uint64_t r1 = (b + 1) * kStatRows - fill < n_rows ? (b + 1) * kStatRows - fill : n_rows;
    const float inf = __builtin_huge_valf();
    double s[4], q[4];
    uint32_t n[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool take = b == 0 && fill != 0 && c0 + e < dim;
        s[e] = take ? carry_s[c0 + e] : 0.0;
        q[e] = take ? carry_q[c0 + e] : 0.0;
        n[e] = take ? carry_n[c0 + e] : 0u;
    }
    for (uint64_t r = r0; r < r1; r += 8) {
        float v[8][4];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint64_t rr = r + u < r1 ? r + u : r1 - 1;
            const float *p = data + rr * dim + c0;
            if (VEC) {
                const float4 t = __builtin_bit_cast(float4, ld_nt(reinterpret_cast<const uint4 *>(p)));
                v[u][0] = t.x, v[u][1] = t.y, v[u][2] = t.z, v[u][3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) v[u][e] = c0 + e < dim ? p[e] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {  // (no early exit: a branch here lets the compiler sink each load behind it)
            const bool row = r + u < r1;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool finite = row && fabsf(v[u][e]) < inf;  // NaN fails; a row past the block adds +0.0 like it
                const double d = finite ? (double)v[u][e] : 0.0;
                s[e] += d;
                q[e] += d * d;  // the product of two f32 values is exact in f64
                n[e] += finite ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (c0 + e < dim) {
            part_s[b * dim + c0 + e] = s[e];
            part_q[b * dim + c0 + e] = q[e];
            part_n[b * dim + c0 + e] = n[e];
        }
    }
}

// The launch's blocks into the running totals, in block order; a last block that is not full yet becomes the carry.
__global__ __launch_bounds__(kBlock) void bin_stats_fold_kernel(const double *__restrict__ part_s,
                                                               const double *__restrict__ part_q,
                                                               const uint32_t *__restrict__ part_n, uint64_t n_blocks,
                                                               uint32_t dim, int last_open, double *__restrict__ tot_s,
                                                               double *__restrict__ tot_q,
                                                               unsigned long long *__restrict__ tot_n,
                                                               double *__restrict__ carry_s, double *__restrict__ carry_q,
                                                               uint32_t *__restrict__ carry_n) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= dim) return;
    double s = tot_s[c], q = tot_q[c];
    unsigned long long n = tot_n[c];
    const uint64_t full = n_blocks - (last_open ? 1 : 0);
    for (uint64_t b = 0; b < full; b++) {
        s += part_s[b * dim + c];
        q += part_q[b * dim + c];
        n += part_n[b * dim + c];
    }
    tot_s[c] = s;
    tot_q[c] = q;
    tot_n[c] = n;
    if (last_open) {
        carry_s[c] = part_s[full * dim + c];
        carry_q[c] = part_q[full * dim + c];
        carry_n[c] = part_n[full * dim + c];
    }
}

// Threshold encoder for rows, the single query (a grid of one) and query batches: bit i of a row is x_i > lo_i, bit
// dim + i is x_i > hi_i (thr = lo | hi, 2 dim floats), strict f32 compares, so NaN and -inf give (0,0) and +inf (1,1).
// bin_encode_kernel's mapping - one wave per row, 64 values per step - with every float read once and two ballots per
// step.  The ballot of the low plane is 64-bit word `st` of the row as it stands; the high plane starts at bit dim, so
// with s = dim % 64 != 0 its ballot is shifted by s and merged with what the previous step left over (`carry`).  Lane
// (st % 64) keeps the two finished words of step st and the wave stores them every 64 steps.  Word dim / 64 holds the
// end of the low plane (known at the last step) and the start of the high one (known at the first): lane 0 writes it
// after the loop, with the last carry behind it.  Every dword of the row is written, pad bits as zeros.
__global__ __launch_bounds__(kBlock) void bin_encode_thr_kernel(const float *__restrict__ data, uint64_t n_rows,
                                                               uint32_t dim, uint32_t row_words,
                                                               const float *__restrict__ thr,
                                                               uint32_t *__restrict__ rows, uint64_t row0) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    const uint32_t full = dim / 64, s = dim % 64, steps = (dim + 63) / 64;
    auto put = [row_words](uint32_t *dst, uint32_t word64, unsigned long long v) {
        const uint32_t w = word64 * 2;
        if (w < row_words) dst[w] = (uint32_t)v;
        if (w + 1 < row_words) dst[w + 1] = (uint32_t)(v >> 32);
    };
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const float *src = data + r * dim;
        uint32_t *dst = rows + (row0 + r) * row_words;
        unsigned long long mine0 = 0, mine1 = 0, carry = 0, first1 = 0, last0 = 0;
        for (uint32_t st = 0; st < steps; st++) {
            const uint32_t j = st * 64 + lane;
            const bool in = j < dim;
            const float v = in ? src[j] : 0.0f;
            const float lo = in ? thr[j] : 0.0f, hi = in ? thr[dim + j] : 0.0f;
            const unsigned long long b0 = __ballot(in && v > lo), b1 = __ballot(in && v > hi);
            const unsigned long long m1 = s ? carry | (b1 << s) : b1;  // word full + st of the row
            carry = s ? b1 >> (64 - s) : 0ull;
            if (st == 0) first1 = m1;
            if (st == full) last0 = b0;  // (only with s != 0: the low plane's last, partial word)
            if ((st & 63u) == (uint32_t)lane) {
                mine0 = b0;
                mine1 = m1;
            }
            if ((st & 63u) == 63u || st + 1 == steps) {
                const uint32_t k = (st & ~63u) + lane;  // the step this lane kept
                if (k <= st) {
                    if (k < full) put(dst, k, mine0);
                    if (s == 0 || k > 0) put(dst, full + k, mine1);
                }
                mine0 = mine1 = 0;
            }
        }
        uint32_t done = full + steps;  // 64-bit words written so far
        if (s) {
            if (lane == 0) {
                put(dst, full, last0 | first1);
                put(dst, full + steps, carry);
            }
            done += 1;
        }
        for (uint32_t w = done * 2 + lane; w < row_words; w += 64) dst[w] = 0;
    }
}

// Scalar query encoding (the reference has no counterpart), one workgroup per query: a = max |v_i| over the
// finite values v_i = q_i (a NaN counts as 0), then c_i = min(L, (u32)((v_i + a) * (L / (a + a)) + 0.5f)) with
// L = 2^bits - 1 - single f32 operations in this order, the division hipcc's correctly rounded one - and plane b = bit b
// of the code at every bit position of a row, position i that of dimension i (one ballot per plane and 64 positions).
// Every dword of every plane is written, pad bits as zeros.
// WEIGHTED (two-bit rows): v_i = w_i = q_i * (hi_i - lo_i) (thr = lo | hi, 2 dim floats; hi_i - lo_i counts
// as 0 when it is not finite: every row is at level 1 there), and the code of dimension i sits at BOTH bit i and bit
// dim + i of every plane, the row's two planes; lane j of the second copy reads q, lo and hi again (L2 hits) rather than
// shift and merge as bin_encode_thr_kernel does.  The product and the sum after it stay two instructions (no v_fma).
// Workgroup g takes query g: its floats at query + g * dim, its planes at planes + g * plane_words, its max_abs at
// max_abs[g].  codes != nullptr (a query batch): also the matrix-core image of the query at codes + g * code_pitch - the
// centred codes d = c - (L + 1) / 2 as int8, one byte per bit position, zero bytes from there to code_pitch - 16, and C =
// the sum of every position's code as a u32 at code_pitch - 16 (bin_gemm_rs_kernel copies the whole pitch into its LDS tile).
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void bin_encode_scalar_kernel(const float *__restrict__ query, uint32_t dim,
                                                                  const float *__restrict__ thr, uint32_t row_words,
                                                                  uint32_t bits, uint32_t *__restrict__ planes,
                                                                  uint32_t plane_words, float *__restrict__ max_abs,
                                                                  int8_t *__restrict__ codes, uint32_t code_pitch) {
    __shared__ float wave_max[kBlock / 64];
    __shared__ uint32_t wave_sum[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inf = __builtin_huge_valf();
    query += (size_t)blockIdx.x * dim;
    planes += (size_t)blockIdx.x * plane_words;
    auto value = [&](uint32_t i) {
        if constexpr (WEIGHTED) {
            float h = thr[dim + i] - thr[i];
            if (!(fabsf(h) < inf)) h = 0.0f;  // inf, and NaN from inf - inf
            const float w = query[i] * h;
            return w != w ? 0.0f : w;  // (inf * 0 too)
        } else {
            const float v = query[i];
            return v != v ? 0.0f : v;
        }
    };
    float a = 0.0f;
    for (uint32_t i = threadIdx.x; i < dim; i += kBlock) {
        const float v = fabsf(value(i));
        if (v < inf && v > a) a = v;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    if (lane == 0) wave_max[wave] = a;
    __syncthreads();
    a = wave_max[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++) a = fmaxf(a, wave_max[w]);
    if (threadIdx.x == 0) max_abs[blockIdx.x] = a;
    const uint32_t L = (1u << bits) - 1u, code_bits = WEIGHTED ? 2u * dim : dim;
    const float scale = a == 0.0f ? 0.0f : (float)L / (a + a);
    // 64 bit positions per step; the code image is at least as long as a plane (whole 128-entry blocks)
    const uint32_t steps = codes ? (code_pitch - 16) / 64 : (row_words + 1) / 2;
    uint32_t csum = 0;
    for (uint32_t st = wave; st < steps; st += kBlock / 64) {
        const uint32_t j = st * 64 + lane;
        uint32_t c = 0;
        if (j < code_bits) {
            const float v = value(WEIGHTED && j >= dim ? j - dim : j);
            if (a == 0.0f) {
                c = (L + 1u) / 2u;
            } else {
                const float t = (v + a) * scale;
                const uint32_t r = (uint32_t)(t + 0.5f);
                c = r < L ? r : L;
            }
            if (v == inf) c = L;
            if (v == -inf) c = 0;
        }
        if (codes) {
            codes[(size_t)blockIdx.x * code_pitch + j] = j < code_bits ? (int8_t)((int)c - (int)((L + 1u) / 2u)) : (int8_t)0;
            csum += c;
        }
        unsigned long long mine = 0;
        for (uint32_t b = 0; b < bits; b++) {
            const unsigned long long m = __ballot((c >> b) & 1u);
            if ((uint32_t)lane == b) mine = m;
        }
        if ((uint32_t)lane < bits) {
            uint32_t *dst = planes + (size_t)lane * row_words;
            const uint32_t w = st * 2;
            if (w < row_words) dst[w] = (uint32_t)mine;
            if (w + 1 < row_words) dst[w + 1] = (uint32_t)(mine >> 32);
        }
    }
    if (codes) {  // C <= 255 * 1118481 < 2^32 (weighted: 255 * 4992 on the matrix route, < 2^24 anywhere)
#pragma unroll
        for (int o = 32; o; o >>= 1) csum += (uint32_t)__shfl_xor((int)csum, o);
        if (lane == 0) wave_sum[wave] = csum;
        __syncthreads();
        if (threadIdx.x < 4) {
            uint32_t total = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; w++) total += wave_sum[w];
            // the last 16 bytes of the pitch: C, then three zero dwords
            reinterpret_cast<uint32_t *>(codes + (size_t)blockIdx.x * code_pitch + (code_pitch - 16))[threadIdx.x] =
                threadIdx.x == 0 ? total : 0u;
        }
    }
}

// ---- rotated rows (the reference has no counterpart) ----
// y = H_P (signs * pad(x)): P the power of two at or above dim, the sign of y_i from a fixed hash of i, then the
// butterflies of stages s = 1, 2, 4, ..., P / 2 in that order - (a, b) = (y_j, y_{j+s}) -> (a + b, a - b), one f32
// operation each (this file compiles with contraction off).  A stage reads only the stage before it, so any split of
// the work gives the same bits; the ORDER of the stages is part of the definition (f32 addition is not associative).
// Block-rotated rows take no pad and cut the network off after stage B / 2, B the largest power of two
// that divides dim: dim / B transforms of size B side by side.  The transform, the two kernel frames (a wave per row, a
// workgroup per row) and their launcher: rotate_blocks.hpp, with width = B = P here and width = dim for blocks.

// What becomes of a finished row, P its width.  MODE 0: the P rotated floats to `out` (statistics, scalar-code
// encoders).  MODE 1: bit i = y_i > 0.  MODE 2: bit i = y_i > lo_i, bit P + i = y_i > hi_i (thr = lo | hi, 2 P floats).
// emit_chunks: 64 lanes hold the 64 consecutive 4-value chunks c0 .. c0 + 63 of a row of P >= 256 values, lane l chunk
// c0 + l.  A lane's four compares are a nibble at bit 4 (l % 8) of dword (c0 + l) / 8; the 8-lane DPP sum of
// bin_encode_flat_kernel (disjoint fields, add == or) finishes the dword and the group's first lane stores it.
template <int MODE>
__device__ __forceinline__ void emit_chunks(const float (&y)[4], uint32_t c0, int lane, uint32_t P, const float *__restrict__ thr,
                                            float *__restrict__ out_row, uint32_t *__restrict__ dst) {
    const uint32_t c = c0 + lane;
    if constexpr (MODE == 0) {
        reinterpret_cast<float4 *>(out_row)[c] = make_float4(y[0], y[1], y[2], y[3]);
    } else {
        float lo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (MODE == 2) {
            const float4 t = reinterpret_cast<const float4 *>(thr)[c];
            lo[0] = t.x, lo[1] = t.y, lo[2] = t.z, lo[3] = t.w;
        }
        const int t8 = lane & 7;
        uint32_t nib = (y[0] > lo[0] ? 1u : 0u) | (y[1] > lo[1] ? 2u : 0u) | (y[2] > lo[2] ? 4u : 0u) | (y[3] > lo[3] ? 8u : 0u);
        const uint32_t d0 = group_sum<8>(nib << (4 * t8));
        if (t8 == 0) dst[c >> 3] = d0;
        if constexpr (MODE == 2) {
            const float4 t = reinterpret_cast<const float4 *>(thr + P)[c];
            nib = (y[0] > t.x ? 1u : 0u) | (y[1] > t.y ? 2u : 0u) | (y[2] > t.z ? 4u : 0u) | (y[3] > t.w ? 8u : 0u);
            const uint32_t d1 = group_sum<8>(nib << (4 * t8));
            if (t8 == 0) dst[P / 32 + (c >> 3)] = d1;
        }
    }
}

// A finished row of `width` values (P, or dim of a block-rotated row) from the two frames of rotate_blocks.hpp, for
// width >= 256 and for every block-rotated row that is no power of two: emit_chunks per live chunk, then the row's dwords
// past its bits as zeros.
template <int MODE> struct BinRotSink : RotSink {
    uint32_t width;
    const float *thr;  // MODE 2: lo | hi, 2 width floats
    float *out;        // MODE 0: width floats per row
    uint32_t *rows;    // MODE 1 / 2: bit rows of row_words dwords, row r at row0 + r
    uint32_t row_words;
    uint64_t row0;
    __device__ uint32_t *dst(uint64_t r) const { return rows + (row0 + r) * row_words; }
    __device__ void chunk(State &, uint64_t r, uint32_t ch, int lane, const float (&y)[4], uint32_t &) const {
        if constexpr (MODE == 2) __builtin_assume_separate_storage(thr, rows);
        emit_chunks<MODE>(y, ch - lane, lane, width, thr, MODE == 0 ? out + r * width : nullptr, MODE == 0 ? nullptr : dst(r));
    }
    __device__ void pad(uint64_t r, uint32_t t, uint32_t threads) const {
        if constexpr (MODE != 0)
            for (uint32_t w = (MODE == 2 ? width / 16 : width / 32) + t; w < row_words; w += threads) dst(r)[w] = 0;
    }
    template <int K> __device__ void row_wave(State &, uint64_t r, int lane, const uint32_t (&)[K]) const { pad(r, lane, 64); }
    __device__ void row_lds(State &, uint64_t r, uint32_t *) const { pad(r, threadIdx.x, kRotThreads); }
};

// Rows of P <= 128 values, another algorithm: a wave per row, lane l holds value 64 k + l in y[k] (K = 1 or 2), the six
// lane stages (lane_butterfly) and, K = 2, one stage across the lane's two values.  P < 64 (K = 1) leaves the lanes from
// P on idle and stops at stage P / 2.  One row per wave and pass of a grid-stride loop, all 64 lanes active throughout
// (the DPP moves read their neighbours).
// MODE 1 / 2: one ballot per plane and 64 values; the row is at most four 64-bit words, every lane puts them together
// and lane j stores dword j of the row's row_words, pad dwords as zeros.
template <int K, int MODE>
__global__ __launch_bounds__(kBlock) void bin_rotate_small_kernel(const float *__restrict__ data, uint64_t n_rows, uint32_t dim,
                                                                 uint32_t P, const float *__restrict__ thr,
                                                                 float *__restrict__ out, uint32_t *__restrict__ rows,
                                                                 uint32_t row_words, uint64_t row0) {
    static_assert(K == 1 || K == 2, "rows of at most 128 values");
    constexpr bool kFull = K > 1;  // P == 64 K: all six lane stages; K = 1 serves every P <= 64 and asks P
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kBlock) >> 6;
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const float *src = data + r * dim;
        float y[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t i = k * 64 + lane;
            float v = rot_signed(i < dim ? src[i] : 0.0f, i);
            if (kFull || 1u < P) v = lane_butterfly<1>(v, lane);
            if (kFull || 2u < P) v = lane_butterfly<2>(v, lane);
            if (kFull || 4u < P) v = lane_butterfly<4>(v, lane);
            if (kFull || 8u < P) v = lane_butterfly<8>(v, lane);
            if (kFull || 16u < P) v = lane_butterfly<16>(v, lane);
            if (kFull || 32u < P) v = lane_butterfly<32>(v, lane);
            y[k] = v;
        }
        if constexpr (K == 2) butterfly(y[0], y[1]);
        if constexpr (MODE == 0) {
#pragma unroll
            for (int k = 0; k < K; k++)
                if ((uint32_t)(k * 64 + lane) < P) out[r * P + k * 64 + lane] = y[k];
        } else {
            uint32_t *dst = rows + (row0 + r) * row_words;
            unsigned long long b0[K], b1[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t i = k * 64 + lane;
                const bool in = i < P;
                const float lo = MODE == 2 && in ? thr[i] : 0.0f, hi = MODE == 2 && in ? thr[P + i] : 0.0f;
                b0[k] = __ballot(in && y[k] > lo);
                b1[k] = MODE == 2 ? __ballot(in && y[k] > hi) : 0ull;
            }
            unsigned long long w0 = b0[0], w1 = K == 2 ? b0[K - 1] : 0ull, w2 = 0, w3 = 0;
            if constexpr (MODE == 2) {
                if (K == 2) w2 = b1[0], w3 = b1[K - 1];
                else if (P == 64) w1 = b1[0];
                else w0 |= b1[0] << P;
            }
            if ((uint32_t)lane < row_words) {
                const unsigned long long w = lane < 2 ? w0 : lane < 4 ? w1 : lane < 6 ? w2 : lane < 8 ? w3 : 0ull;
                dst[lane] = (lane & 1) ? (uint32_t)(w >> 32) : (uint32_t)w;
            }
            for (uint32_t w = 64 + lane; w < row_words; w += 64) dst[w] = 0;
        }
    }
}

int grid_for(uint64_t work_items, uint64_t per_block, int blocks_per_cu) {
    uint64_t want = (work_items + per_block - 1) / per_block;
    uint64_t cap = (uint64_t)device_info().cu_count * blocks_per_cu;
    if (want < 1) want = 1;
    return (int)(want > cap ? cap : want);
}

// get_storage_size * size_of (:99-116 u8, :152-159 u128, :210-213)
uint64_t row_bytes_of(uint64_t dim, int store) {
    if (store == QAMD_BITS_U128) return (dim / 128 + (dim % 128 != 0)) * 16;
    const uint64_t bytes_count = dim > 128 ? 16 : dim > 64 ? 8 : dim > 32 ? 4 : 1;
    const uint64_t bits = 8 * bytes_count;
    return (dim / bits + (dim % bits != 0)) * bytes_count;
}

uint64_t device_stride_of(uint64_t nb) { return nb >= 8 ? nb : 4; }

}  // namespace

struct qamd_bin {
    int device = 0;
    qamd_vector_parameters vp{};
    int store = 0;
    uint64_t count = 0;
    uint64_t capacity = 0;  // rows there is room for: count after every builder, more after reserve / upsert
    uint64_t nb = 0;  // reference row bytes
    uint64_t ds = 0;  // device row stride (bytes)
    DevBuf rows;      // [round_up(capacity, 1024) + 1024][ds], zero from row count on
    // Two-bit rows: a row holds code_bits = 2 dim bits and is scored as a one-bit row of that length;
    // vp.dim stays the vectors' dimension (thresholds, queries, the originals of a rescored top-k).
    // Rotated rows: the encoders see y = H_P (signs * pad(x)) of edim = P values in place of x; everything
    // after them - thresholds, code_bits, the scans - is that of a plain store of P dimensions.
    // Block-rotated rows: y has edim = dim values, dim / B transforms of size B, and the store is a plain
    // one of dim dimensions.
    int encoding = QAMD_BIN_ONE_BIT;
    uint64_t edim = 0;            // what the bit encoders see: dim, or P of a (padded) rotated store
    uint64_t code_bits = 0;       // bits of a row: edim, or 2 edim
    std::vector<float> thr_host;  // two-bit: lo[edim] | hi[edim]
    bool two() const { return (encoding & QAMD_BIN_TWO_BITS) != 0; }
    bool rotated() const { return (encoding & QAMD_BIN_ROTATED) != 0; }
    bool blocks() const { return (encoding & QAMD_BIN_BLOCKS) != 0; }
    DevBuf thr;                   // the same, for the encoders of rows and queries
    // the batched top-k's pivot sample (rows hash(j) of the store, j < sample_count, then 512 zero rows);
    // gathered on first use (count / 64 rows at most), discarded by an upsert
    mutable std::mutex sample_mu;
    mutable DevBuf sample_rows;
    mutable uint32_t sample_count = 0;
};

struct qamd_bin_query {
    int device = 0;
    uint64_t nb = 0, ds = 0, qdim_cap = 0;
    DevBuf buf;  // ds bytes (+ padding); a scalar query: `bits` planes of ds bytes, the f32 max_abs 16 bytes after them
    uint32_t bits = 1;  // 1: the reference's binary query; 4 / 8: bit planes of a scalar query
    ReadyEvent ready;  // the last encode_query
};

namespace {

// P of DESIGN 3.2g: the smallest power of two >= dim, 1 for dim = 1 (and no dimension stays none)
uint64_t rot_dim(uint64_t dim) {
    if (dim == 0) return 0;
    uint64_t p = 1;
    while (p < dim) p <<= 1;
    return p;
}

// The dimension the bit encoders of `encoding` see for vectors of `dim`: block rotation (3.2h) does not pad.
uint64_t encoder_dim(uint64_t dim, int encoding) {
    return (encoding & QAMD_BIN_ROTATED) && !(encoding & QAMD_BIN_BLOCKS) ? rot_dim(dim) : dim;
}

qamd_status alloc_store(qamd_bin *h) {
    h->edim = encoder_dim(h->vp.dim, h->encoding);
    h->code_bits = h->two() ? 2 * h->edim : h->edim;
    h->nb = row_bytes_of(h->code_bits, h->store);
    h->ds = device_stride_of(h->nb);
    h->capacity = h->count;
    return h->rows.alloc(padded_rows_of(h->capacity) * h->ds, true);
}

// calculate_metric's `dim` for a query of `planes` bit planes: the row's bits * (2^planes - 1), exact in f32
// (encode_query refuses scalar dims past 2^24, two-bit rows dims past 2^23)
float metric_dim(const qamd_bin *h, uint32_t planes) { return (float)(h->code_bits * ((1ull << planes) - 1)); }

template <int G, int ITERS, int UNROLL, int PLANES = 1>
void launch_bin(const qamd_bin *h, const uint4 *qb, float *out, const TopkFilter *filt, hipStream_t s, uint64_t n_rows) {
    constexpr int TILE = (64 / G) * UNROLL;
    const uint32_t rc = (uint32_t)(h->ds / 16);
    const int is_dot = h->vp.distance_type == QAMD_DOT;
    const uint64_t waves = (n_rows + TILE - 1) / TILE;
    const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
    const bool exact = rc == (uint32_t)(G * ITERS);
#define QAMD_BIN_GO(EX, FI)                                                                                  \
    hipLaunchKernelGGL((bin_scan_kernel<G, ITERS, UNROLL, EX, FI, PLANES>), dim3(grid), dim3(kScanBlock), 0, s,      \
                       h->rows.as<uint4>(), qb, metric_dim(h, PLANES), is_dot, h->vp.invert, (uint32_t)n_rows, rc, \
                       out, filt ? *filt : TopkFilter{})
    if (filt) {
        if (exact) QAMD_BIN_GO(true, true);
        else QAMD_BIN_GO(false, true);
    } else {
        if (exact) QAMD_BIN_GO(true, false);
        else QAMD_BIN_GO(false, false);
    }
#undef QAMD_BIN_GO
}

qamd_status words_launch(const qamd_bin *h, const uint32_t *qbits, const uint32_t *ids_dev, uint64_t n,
                         float *out_dev, hipStream_t s, uint32_t planes = 1) {
    if (n == 0) return QAMD_OK;
    int grid = grid_for((n + 3) / 4, kBlock / 64, 8);
#define QAMD_BIN_WORDS(P)                                                                                     \
    hipLaunchKernelGGL(bin_words_kernel<P>, dim3(grid), dim3(kBlock), 0, s, h->rows.as<uint32_t>(), qbits,    \
                       metric_dim(h, P), (int)(h->vp.distance_type == QAMD_DOT), h->vp.invert, ids_dev, n,    \
                       (uint32_t)h->count, (uint32_t)(h->ds / 4), out_dev)
    if (planes == 8) QAMD_BIN_WORDS(8);
    else if (planes == 4) QAMD_BIN_WORDS(4);
    else QAMD_BIN_WORDS(1);
#undef QAMD_BIN_WORDS
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// One launch of bin_pairs_kernel (lists == nullptr: the single query bit row for every id).
qamd_status pairs_launch(const qamd_bin *h, const uint32_t *q_single, const uint8_t *q_batch, uint64_t q_stride,
                         const uint32_t *lists, uint32_t n_lists, const uint32_t *list_rows, const uint32_t *ids_dev,
                         uint64_t n, float *out_dev, hipStream_t s, uint32_t planes = 1) {
    if (n == 0) return QAMD_OK;
    if (planes != 1 && (list_rows || !(q_single || q_batch))) return fail(QAMD_ERR_ARGUMENTS, "bit planes only come with a query");
    const bool vec16 = h->ds % 16 == 0;
    const uint32_t ppb = pairs_per_block(n, vec16 ? 32 : 16);  // lane groups per workgroup
    const unsigned grid = (unsigned)((n + ppb - 1) / ppb);
#define QAMD_BIN_PAIRS(V, P)                                                                                       \
    hipLaunchKernelGGL((bin_pairs_kernel<V, P>), dim3(grid), dim3(kBlock), 0, s, h->rows.as<uint32_t>(), q_single, q_batch, \
                       (uint32_t)q_stride, lists, n_lists, list_rows, metric_dim(h, P),                            \
                       (int)(h->vp.distance_type == QAMD_DOT), h->vp.invert, ids_dev, n, (uint32_t)h->count,        \
                       (uint32_t)(h->ds / 4), ppb, out_dev)
    if (planes == 8) {
        if (vec16) QAMD_BIN_PAIRS(true, 8);
        else QAMD_BIN_PAIRS(false, 8);
    } else if (planes == 4) {
        if (vec16) QAMD_BIN_PAIRS(true, 4);
        else QAMD_BIN_PAIRS(false, 4);
    } else if (vec16) QAMD_BIN_PAIRS(true, 1);
    else QAMD_BIN_PAIRS(false, 1);
#undef QAMD_BIN_PAIRS
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// out[k] = metric(query bit row `qbits`, row ids[k]) for host or device ids / outputs (run_ids, lists.hpp): the body
// of score_ids and, with qbits = stored row i, of score_internal_ids.
qamd_status score_ids_any(const qamd_bin *h, const uint32_t *qbits, const uint32_t *ids, uint64_t n_ids, qamd_mem ids_mem,
                          float *out, qamd_mem out_mem, hipStream_t s, uint32_t planes = 1) {
    return run_ids(ids, n_ids, ids_mem, out, out_mem, h->count, s, [&](const uint32_t *ids_dev, uint64_t n, float *out_dev) {
        return pairs_launch(h, qbits, nullptr, 0, nullptr, 0, nullptr, ids_dev, n, out_dev, s, planes);
    });
}

bool fused_capable(const qamd_bin *h) { return bin_fused_rows(h->ds); }

// The scan of a query's planes (1: its bit row), bin_scan_kernel's mapping per row length; the 8-lane rows of a scalar
// query scan half the rows per wave, to leave the registers their 16-row tile takes to the planes of a piece.
template <int PLANES>
void scan_planes(const qamd_bin *h, const uint4 *qb, float *out_dev, hipStream_t s, const TopkFilter *filt, uint64_t n) {
    const uint32_t rc = (uint32_t)(h->ds / 16);
    if (rc == 1) launch_bin<1, 1, 4, PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc == 2) launch_bin<2, 1, 4, PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc <= 4) launch_bin<4, 1, 8, PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc <= 8) launch_bin<8, 1, (PLANES == 1 ? 16 : 8), PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc <= 16) launch_bin<16, 1, 8, PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc <= 32) launch_bin<16, 2, 4, PLANES>(h, qb, out_dev, filt, s, n);
    else if (rc <= 48) launch_bin<16, 3, 4, PLANES>(h, qb, out_dev, filt, s, n);
    else launch_bin<16, 4, 2, PLANES>(h, qb, out_dev, filt, s, n);
}

// n_rows: the scan covers rows [0, n_rows) of the store (a null id list of n_ids rows); 0 = all of them.
qamd_status scan_bits(const qamd_bin *h, const void *qbits_dev, float *out_dev, hipStream_t s,
                      const TopkFilter *filt = nullptr, uint32_t planes = 1, uint64_t n_rows = 0) {
    if (h->count == 0) return QAMD_OK;
    const uint64_t n = n_rows ? n_rows : h->count;
    if (!fused_capable(h))
        return words_launch(h, static_cast<const uint32_t *>(qbits_dev), nullptr, n, out_dev, s, planes);
    const uint4 *qb = static_cast<const uint4 *>(qbits_dev);
    if (planes == 8) scan_planes<8>(h, qb, out_dev, s, filt, n);
    else if (planes == 4) scan_planes<4>(h, qb, out_dev, s, filt, n);
    else scan_planes<1>(h, qb, out_dev, s, filt, n);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

template <int G, int ITERS, int PLANES>
qamd_status launch_bin_small(const qamd_bin *h, const uint4 *qb, const SmallTopkPlan &pl, const SmallTopk &p, hipStream_t s) {
    const uint32_t rc = (uint32_t)(h->ds / 16);
    const bool exact = rc == (uint32_t)(G * ITERS);
#define QAMD_BIN_SMALL(EX)                                                                                         \
    hipLaunchKernelGGL((bin_topk_small_kernel<G, ITERS, EX, PLANES>), dim3(pl.workgroups), dim3(1024), 0, s, h->rows.as<uint4>(), \
                       qb, metric_dim(h, PLANES), (int)(h->vp.distance_type == QAMD_DOT), h->vp.invert, (uint32_t)h->count, rc, \
                       pl.rows_per_wg, p)
    if (exact) QAMD_BIN_SMALL(true);
    else QAMD_BIN_SMALL(false);
#undef QAMD_BIN_SMALL
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

int bin_small_group(uint32_t rc) { return rc == 1 ? 1 : rc == 2 ? 2 : rc <= 4 ? 4 : rc <= 8 ? 8 : rc <= 64 ? 16 : 0; }

template <int PLANES>
qamd_status launch_small(const qamd_bin *h, const uint4 *qb, const SmallTopkPlan &pl, const SmallTopk &p, hipStream_t s) {
    const uint32_t rc = (uint32_t)(h->ds / 16);
    if (rc == 1) return launch_bin_small<1, 1, PLANES>(h, qb, pl, p, s);
    if (rc == 2) return launch_bin_small<2, 1, PLANES>(h, qb, pl, p, s);
    if (rc <= 4) return launch_bin_small<4, 1, PLANES>(h, qb, pl, p, s);
    if (rc <= 8) return launch_bin_small<8, 1, PLANES>(h, qb, pl, p, s);
    if (rc <= 16) return launch_bin_small<16, 1, PLANES>(h, qb, pl, p, s);
    // 1024 threads leave 128 registers: several pieces per lane times several planes spill (bin_topk_small sends those on)
    if constexpr (PLANES > 1) {
        return fail(QAMD_ERR_ARGUMENTS, "no single-launch top-k for bit planes on rows of more than 16 pieces");
    } else {
        if (rc <= 32) return launch_bin_small<16, 2, PLANES>(h, qb, pl, p, s);
        if (rc <= 48) return launch_bin_small<16, 3, PLANES>(h, qb, pl, p, s);
        return launch_bin_small<16, 4, PLANES>(h, qb, pl, p, s);
    }
}

// Whether the single-launch top-k applies to this store, k and kind of query, and its plan.
bool bin_small_plan(const qamd_bin *h, uint32_t k, uint32_t planes, SmallTopkPlan &plan) {
    const int g = bin_small_group((uint32_t)(h->ds / 16));
    if (!g || !fused_capable(h)) return false;
    if (planes != 1 && h->ds / 16 > 16) return false;  // scalar queries on long rows: the fused / classic routes
    const uint32_t tile = 2 * (64 / g), least = (uint32_t)std::max<uint64_t>(16 * tile, (128 * 1024) / h->ds);
    return small_topk_plan(h->count, k, tile, least, plan);
}

// The single-launch top-k when the store qualifies (<= 2M rows, k <= 64, 16-byte row pieces): false = not applicable.
bool bin_topk_small(const qamd_bin *h, const void *qbits_dev, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                    qamd_mem out_mem, hipStream_t s, qamd_status &st, uint32_t planes = 1) {
    SmallTopkPlan plan;
    if (!bin_small_plan(h, k, planes, plan)) return false;
    st = small_topk(plan, k, largest, out_ids, out_scores, out_mem, s, [&](const SmallTopk &p, hipStream_t stt) {
        const uint4 *qb = static_cast<const uint4 *>(qbits_dev);
        return planes == 8 ? launch_small<8>(h, qb, plan, p, stt)
               : planes == 4 ? launch_small<4>(h, qb, plan, p, stt) : launch_small<1>(h, qb, plan, p, stt);
    });
    return true;
}

qamd_status check_query(const qamd_bin *h, const qamd_bin_query *q) {
    if (!h || !q) return fail(QAMD_ERR_ARGUMENTS, "null handle or query");
    if (q->nb != h->nb) return fail(QAMD_ERR_ARGUMENTS, "query has %llu bytes, rows have %llu",
                                    (unsigned long long)q->nb, (unsigned long long)h->nb);
    return QAMD_OK;
}

// Host rows at stride nb -> device stride ds (differs only for the tiny rows).
qamd_status upload_rows(qamd_bin *h, const uint8_t *rows, qamd_mem mem, hipStream_t s) {
    if (h->count == 0) return QAMD_OK;
    if (h->nb == h->ds) return copy_in(h->rows.ptr, rows, mem, h->count * h->nb, s);
    std::vector<uint8_t> host(h->count * h->nb), wide(h->count * h->ds, 0);
    if (h->nb) {
        if (mem == QAMD_MEM_DEVICE) QAMD_TRY(copy_out(host.data(), QAMD_MEM_HOST, rows, host.size(), s));
        else memcpy(host.data(), rows, host.size());
    }
    for (uint64_t r = 0; r < h->count; r++) memcpy(&wide[r * h->ds], &host[r * h->nb], h->nb);
    return copy_in(h->rows.ptr, wide.data(), QAMD_MEM_HOST, wide.size(), s);
}

// The bit encoder for a one-bit or two-bit store: `n` vectors of `dim` floats into bit rows of `row_words` dwords, the
// first at row r0 of dst - the store's rows, a query's bit row, a batch's (one "row" per query, :288-291 is encode_vector
// itself).
// The rotation of `n` vectors of `dim` floats.  MODE 0: `width` floats per vector to `out`; MODE 1 / 2: the fused row
// encoder - bit rows of `row_words` dwords from row r0 of `rows` on, thr = lo | hi for MODE 2.  Padded:
// width = B = P = rot_dim(dim).  `blocks` (dim % 64 == 0, checked by every caller's check_enc_args):
// width = dim, B = rot_block(dim); a power-of-two dim has B == dim == P, the same transform.  Rows of one block of at
// most 128 values take the small kernel, every other row the frames of rotate_blocks.hpp.
template <int MODE>
void launch_rotate(const float *src, uint64_t n, uint64_t dim, bool blocks, const float *thr, float *out, uint32_t *rows,
                   uint64_t row_words, uint64_t r0, hipStream_t s) {
    if (n == 0 || dim == 0) return;
    const uint32_t width = (uint32_t)(blocks ? dim : rot_dim(dim)), B = (uint32_t)(blocks ? rot_block(dim) : width);
    if (width == B && width <= 128) {
        const auto small = width <= 64 ? bin_rotate_small_kernel<1, MODE> : bin_rotate_small_kernel<2, MODE>;
        hipLaunchKernelGGL(small, dim3(grid_for(n, kBlock / 64, 8)), dim3(kBlock), 0, s, src, n, (uint32_t)dim, width, thr, out,
                           rows, (uint32_t)row_words, r0);
        return;
    }
    BinRotSink<MODE> sink;
    sink.width = width, sink.thr = thr, sink.out = out, sink.rows = rows, sink.row_words = (uint32_t)row_words, sink.row0 = r0;
    launch_rot(sink, src, n, (uint32_t)dim, width, B, s);
}

void launch_bit_encoder(const qamd_bin *h, const float *src, uint64_t n, uint64_t dim, uint64_t row_words, uint32_t *dst,
                        uint64_t r0, hipStream_t s) {
    if (n == 0 || dim == 0) return;
    if (h->rotated()) {  // (dim is the handle's: every caller has checked it)
        if (h->two()) launch_rotate<2>(src, n, dim, h->blocks(), h->thr.as<float>(), nullptr, dst, row_words, r0, s);
        else launch_rotate<1>(src, n, dim, h->blocks(), nullptr, nullptr, dst, row_words, r0, s);
        return;
    }
    const int grid = grid_for(n, kBlock / 64, 8);
    if (h->two())
        hipLaunchKernelGGL(bin_encode_thr_kernel, dim3(grid), dim3(kBlock), 0, s, src, n, (uint32_t)dim, (uint32_t)row_words,
                           h->thr.as<float>(), dst, r0);
    else
        hipLaunchKernelGGL(bin_encode_kernel, dim3(grid), dim3(kBlock), 0, s, src, n, (uint32_t)dim, (uint32_t)row_words, dst, r0);
}

// The scalar encoder for a one-bit or two-bit (weighted) store: `n` queries of `dim` floats, one workgroup
// each.  The single query has no code image: codes = nullptr.
qamd_status launch_scalar_encoder(const qamd_bin *h, const float *src, uint64_t n, uint64_t dim, uint64_t ds, uint32_t bits,
                           uint32_t *planes, uint64_t p_stride, float *max_abs, int8_t *codes, uint64_t code_pitch,
                           hipStream_t s) {
    StreamBuf rot;  // a rotated store: the codes come from y, P (blocks: dim) floats per query, held
                    // until `s` has used them
    if (h->rotated() && n && dim) {
        const uint64_t P = encoder_dim(dim, h->encoding);
        QAMD_TRY(rot.alloc(n * P * 4, s));
        launch_rotate<0>(src, n, dim, h->blocks(), nullptr, rot.as<float>(), nullptr, 0, 0, s);
        src = rot.as<float>();
        dim = P;
    }
    if (h->two())
        hipLaunchKernelGGL(bin_encode_scalar_kernel<true>, dim3((unsigned)n), dim3(kBlock), 0, s, src, (uint32_t)dim,
                           h->thr.as<float>(), (uint32_t)(ds / 4), bits, planes, (uint32_t)(p_stride / 4), max_abs, codes,
                           (uint32_t)code_pitch);
    else
        hipLaunchKernelGGL(bin_encode_scalar_kernel<false>, dim3((unsigned)n), dim3(kBlock), 0, s, src, (uint32_t)dim,
                           static_cast<const float *>(nullptr), (uint32_t)(ds / 4), bits, planes, (uint32_t)(p_stride / 4),
                           max_abs, codes, (uint32_t)code_pitch);
    return QAMD_OK;
}

// encode_vector (:193-208) for `nr` device-resident rows: rows r0 .. r0+nr of the store.
qamd_status launch_bin_encode(qamd_bin *h, const float *src, uint64_t nr, uint64_t r0, hipStream_t s) {
    const uint64_t dim = h->vp.dim;
    if (nr == 0 || dim == 0) return QAMD_OK;
    if (h->encoding == QAMD_BIN_ONE_BIT && dim % 128 == 0 && h->ds * 8 == dim && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const uint64_t n4 = nr * dim / 4;
        const unsigned grid = (unsigned)((n4 + 1024 * (kBlock / 64) - 1) / (1024 * (kBlock / 64)));
        hipLaunchKernelGGL(bin_encode_flat_kernel, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const float4 *>(src),
                           n4, h->rows.as<uint32_t>() + r0 * (h->ds / 4));
    } else {
        launch_bit_encoder(h, src, nr, dim, h->ds / 4, h->rows.as<uint32_t>(), r0, s);
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// The rows of a one-shot encode: host rows are staged 256 MiB at a time; device rows are read in place, 8 GiB per launch.
qamd_status encode_all(qamd_bin *h, const float *data, qamd_mem data_mem, qamd_stop_fn stop, void *stop_user, hipStream_t s) {
    const uint64_t dim = h->vp.dim, count = h->count;
    if (count && dim) {
        const uint64_t batch_bytes = stage_bytes(data_mem == QAMD_MEM_HOST ? (256ull << 20) : (8ull << 30));
        const uint64_t batch_rows = std::max<uint64_t>(1, std::min<uint64_t>(count, batch_bytes / (dim * 4)));
        DevBuf stage;
        if (data_mem == QAMD_MEM_HOST) QAMD_TRY(stage.alloc(batch_rows * dim * 4));
        for (uint64_t r0 = 0; r0 < count; r0 += batch_rows) {
            if (stop && stop(stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");  // :174-176
            const uint64_t nr = std::min(batch_rows, count - r0);
            const float *src = data + r0 * dim;
            if (data_mem == QAMD_MEM_HOST) {
                QAMD_TRY(copy_in(stage.ptr, src, QAMD_MEM_HOST, nr * dim * 4, s));
                src = stage.as<float>();
            }
            QAMD_TRY(launch_bin_encode(h, src, nr, r0, s));
            if (data_mem == QAMD_MEM_HOST || stop) QAMD_HIP(hipStreamSynchronize(s));
        }
        QAMD_HIP(hipStreamSynchronize(s));
    } else if (stop && count && stop(stop_user)) {
        return fail(QAMD_ERR_STOPPED, "Stopped");
    }
    return QAMD_OK;
}

// ---- two-bit rows: statistics, thresholds, arguments
constexpr uint64_t kTwoBitMaxDim = 1ull << 23;  // 2 dim <= 2^24: every count and score is an exact f32 integer
constexpr double kTwoBitDefaultT = 0.43;

// The running statistics of a sequence of row batches (bin_stats_kernel): totals of the closed blocks and the open
// block's sums on the device, `fill` = rows the open block holds.  The batches' cuts do not show in the result.
struct BinStats {
    uint64_t dim = 0;
    uint32_t fill = 0;
    DevBuf state;  // tot_s, tot_q (f64), tot_n (u64), carry_s, carry_q (f64), carry_n (u32): [dim] each

    double *tot_s() const { return state.as<double>(); }
    double *tot_q() const { return tot_s() + dim; }
    unsigned long long *tot_n() const { return reinterpret_cast<unsigned long long *>(tot_q() + dim); }
    double *carry_s() const { return tot_s() + 3 * dim; }
    double *carry_q() const { return tot_s() + 4 * dim; }
    uint32_t *carry_n() const { return reinterpret_cast<uint32_t *>(tot_s() + 5 * dim); }

    qamd_status begin(uint64_t d) {
        dim = d;
        fill = 0;
        return state.alloc(std::max<uint64_t>(dim, 1) * 44, true);
    }
    // `n` rows at `src` (readable on the current device), enqueued on `s`
    qamd_status add(const float *src, uint64_t n, hipStream_t s) {
        if (n == 0 || dim == 0) return QAMD_OK;
        const uint64_t blocks = (n + fill + kStatRows - 1) / kStatRows;
        if (blocks > 0x7FFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "too many rows in one statistics launch");
        StreamBuf part;  // the launch's block sums: part_s, part_q (f64), part_n (u32), [blocks][dim] each
        QAMD_TRY(part.alloc(blocks * dim * 20, s));
        double *ps = part.as<double>(), *pq = ps + blocks * dim;
        uint32_t *pn = reinterpret_cast<uint32_t *>(pq + blocks * dim);
        const dim3 grid((unsigned)blocks, (unsigned)((dim + 255) / 256));
        if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0)
            hipLaunchKernelGGL(bin_stats_kernel<true>, grid, dim3(64), 0, s, src, n, (uint32_t)dim, fill, carry_s(), carry_q(),
                               carry_n(), ps, pq, pn);
        else
            hipLaunchKernelGGL(bin_stats_kernel<false>, grid, dim3(64), 0, s, src, n, (uint32_t)dim, fill, carry_s(), carry_q(),
                               carry_n(), ps, pq, pn);
        const uint32_t new_fill = (uint32_t)((n + fill) % kStatRows);
        hipLaunchKernelGGL(bin_stats_fold_kernel, dim3((unsigned)((dim + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ps, pq, pn,
                           blocks, (uint32_t)dim, new_fill != 0 ? 1 : 0, tot_s(), tot_q(), tot_n(), carry_s(), carry_q(), carry_n());
        QAMD_HIP(hipGetLastError());
        fill = new_fill;
        return QAMD_OK;
    }
    // The open block closes as the last one.  Host outputs of `dim` entries.
    qamd_status finish(hipStream_t s, uint64_t *n, double *sum, double *sumsq) {
        if (dim == 0) return QAMD_OK;
        std::vector<uint8_t> host(dim * 44);
        QAMD_TRY(copy_out(host.data(), QAMD_MEM_HOST, state.ptr, host.size(), s));
        QAMD_HIP(hipStreamSynchronize(s));
        const double *ts = reinterpret_cast<const double *>(host.data()), *tq = ts + dim, *cs = ts + 3 * dim, *cq = ts + 4 * dim;
        const uint64_t *tn = reinterpret_cast<const uint64_t *>(ts + 2 * dim);
        const uint32_t *cn = reinterpret_cast<const uint32_t *>(ts + 5 * dim);
        for (uint64_t i = 0; i < dim; i++) {
            sum[i] = fill ? ts[i] + cs[i] : ts[i];
            sumsq[i] = fill ? tq[i] + cq[i] : tq[i];
            n[i] = fill ? tn[i] + cn[i] : tn[i];
        }
        return QAMD_OK;
    }
};

// A batch of rows, in host or device memory, into the statistics: in pieces as the encoders stage them.
// `stop` is polled before every piece, as the row pass polls it.
// raw_dim != 0 (rotated rows): the rows have raw_dim floats and the statistics are those of their rotation,
// st.dim = P columns (`blocks`, 3.2h: raw_dim columns) - a piece of at most 256 MiB is rotated into a stream-ordered
// buffer and added from there.
qamd_status stats_feed(BinStats &st, const float *data, qamd_mem mem, uint64_t n_rows, DevBuf &stage, hipStream_t s,
                       qamd_stop_fn stop = nullptr, void *stop_user = nullptr, uint64_t raw_dim = 0, bool blocks = false) {
    if (st.dim == 0 || n_rows == 0) return QAMD_OK;
    const uint64_t piece_bytes = stage_bytes(mem == QAMD_MEM_HOST || raw_dim ? (256ull << 20) : (8ull << 30));
    const uint64_t piece_rows = std::max<uint64_t>(1, piece_bytes / (st.dim * 4));
    return for_each_staged_piece(data, mem, n_rows, raw_dim ? raw_dim : st.dim, piece_rows, stage, s,
                                 [&](const float *src, uint64_t, uint64_t nr) -> qamd_status {
        if (stop && stop(stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
        if (!raw_dim) return st.add(src, nr, s);
        StreamBuf rot;
        QAMD_TRY(rot.alloc(nr * st.dim * 4, s));
        launch_rotate<0>(src, nr, raw_dim, blocks, nullptr, rot.as<float>(), nullptr, 0, 0, s);
        return st.add(rot.as<float>(), nr, s);
    });
}

// Host only, f64, single operations in the order of DESIGN 3.2e (this file compiles with contraction off).
void thresholds_of(uint64_t dim, const uint64_t *n, const double *sum, const double *sumsq, double t, float *lo, float *hi) {
    for (uint64_t i = 0; i < dim; i++) {
        double mean = 0.0, var = 0.0;
        if (n[i] != 0) {
            const double cnt = (double)n[i];
            mean = sum[i] / cnt;
            const double m2 = mean * mean;
            var = sumsq[i] / cnt - m2;
        }
        if (!(var > 0.0)) var = 0.0;
        const double sd = std::sqrt(var);
        const double w = t * sd;
        lo[i] = (float)(mean - w);
        hi[i] = (float)(mean + w);
    }
}

// What every *_enc entry point checks before it needs a device.  `required`: two-bit rows cannot do without thresholds.
qamd_status check_enc_args(const qamd_vector_parameters *vp, int encoding, const float *lo, const float *hi, bool required) {
    if ((encoding & ~(QAMD_BIN_TWO_BITS | QAMD_BIN_ROTATED | QAMD_BIN_BLOCKS)) != 0 || encoding < 0 ||
        ((encoding & QAMD_BIN_BLOCKS) && !(encoding & QAMD_BIN_ROTATED)))  // blocks are blocks of a rotation
        return fail(QAMD_ERR_ARGUMENTS, "unknown binary encoding %d", encoding);
    if ((lo == nullptr) != (hi == nullptr)) return fail(QAMD_ERR_ARGUMENTS, "thresholds: lo and hi come together");
    if ((encoding & QAMD_BIN_ROTATED) && vp->dim > kRotMaxDim)
        return fail(QAMD_ERR_ARGUMENTS, "rotated rows have at most %llu dimensions, not %llu", (unsigned long long)kRotMaxDim,
                    (unsigned long long)vp->dim);
    if ((encoding & QAMD_BIN_BLOCKS) && vp->dim % kRotBlockMin != 0)
        return fail(QAMD_ERR_ARGUMENTS, "block-rotated rows have a multiple of %llu dimensions, not %llu",
                    (unsigned long long)kRotBlockMin, (unsigned long long)vp->dim);
    if (!(encoding & QAMD_BIN_TWO_BITS)) {
        if (lo) return fail(QAMD_ERR_ARGUMENTS, "one-bit rows take no thresholds");
        return QAMD_OK;
    }
    if (vp->dim > kTwoBitMaxDim)
        return fail(QAMD_ERR_ARGUMENTS, "two-bit rows have at most %llu dimensions, not %llu", (unsigned long long)kTwoBitMaxDim,
                    (unsigned long long)vp->dim);
    if (!lo && required) return fail(QAMD_ERR_ARGUMENTS, "two-bit rows need their thresholds");
    const uint64_t edim = encoder_dim(vp->dim, encoding);  // given thresholds have P entries for (padded) rotated rows
    for (uint64_t i = 0; lo && i < edim; i++) {
        if (lo[i] != lo[i] || hi[i] != hi[i]) return fail(QAMD_ERR_ARGUMENTS, "threshold %llu is NaN", (unsigned long long)i);
        if (lo[i] > hi[i]) return fail(QAMD_ERR_ARGUMENTS, "threshold %llu: lo %g > hi %g", (unsigned long long)i, lo[i], hi[i]);
    }
    return QAMD_OK;
}

qamd_status set_thresholds(qamd_bin *h, const float *lo, const float *hi, hipStream_t s) {
    const uint64_t dim = h->edim;
    h->thr_host.resize(2 * dim);
    if (dim == 0) return QAMD_OK;
    memcpy(h->thr_host.data(), lo, dim * 4);
    memcpy(h->thr_host.data() + dim, hi, dim * 4);
    QAMD_TRY(h->thr.alloc(2 * dim * 4));
    QAMD_TRY(copy_in(h->thr.ptr, h->thr_host.data(), QAMD_MEM_HOST, 2 * dim * 4, s));
    QAMD_HIP(hipStreamSynchronize(s));  // (thr_host may be resized by no one, but the copy reads pageable memory)
    return QAMD_OK;
}

qamd_status set_thresholds_from_stats(qamd_bin *h, BinStats &st, hipStream_t s) {
    const uint64_t dim = h->edim;
    std::vector<uint64_t> n(dim);
    std::vector<double> sum(dim), sumsq(dim);
    std::vector<float> lo(dim), hi(dim);
    QAMD_TRY(st.finish(s, n.data(), sum.data(), sumsq.data()));
    thresholds_of(dim, n.data(), sum.data(), sumsq.data(), kTwoBitDefaultT, lo.data(), hi.data());
    return set_thresholds(h, lo.data(), hi.data(), s);
}

qamd_status new_store(const qamd_vector_parameters *vp, int store, int encoding, std::unique_ptr<qamd_bin> &h) {
    h.reset(new qamd_bin);
    h->device = current_device();
    h->vp = *vp;
    h->store = store;
    h->count = vp->count;
    h->encoding = encoding;
    return alloc_store(h.get());
}

}  // namespace

extern "C" {

uint64_t qamd_bin_quantized_vector_size(const qamd_vector_parameters *vp, qamd_bits_store store) {
    return row_bytes_of(vp->dim, store);
}

uint64_t qamd_bin_quantized_vector_size_enc(const qamd_vector_parameters *vp, qamd_bits_store store, qamd_bin_encoding encoding) {
    const uint64_t edim = encoder_dim(vp->dim, encoding);
    return row_bytes_of((encoding & QAMD_BIN_TWO_BITS) ? 2 * edim : edim, store);
}

qamd_status qamd_bin_find_stats(const float *data, qamd_mem data_mem, uint64_t n_rows, uint64_t dim, void *stream, uint64_t *n,
                                double *sum, double *sumsq) {
    if (dim && (!n || !sum || !sumsq)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (!data && n_rows && dim) return fail(QAMD_ERR_ARGUMENTS, "data is null");
    if (dim > kTwoBitMaxDim) return fail(QAMD_ERR_ARGUMENTS, "at most %llu dimensions", (unsigned long long)kTwoBitMaxDim);
    if (n_rows == 0 || dim == 0) {  // nothing to read: no device either
        for (uint64_t i = 0; i < dim; i++) n[i] = 0, sum[i] = 0.0, sumsq[i] = 0.0;
        return QAMD_OK;
    }
    QAMD_ON_DEVICE(current_device());
    hipStream_t s = as_stream(stream);
    BinStats st;
    DevBuf stage;
    QAMD_TRY(st.begin(dim));
    QAMD_TRY(stats_feed(st, data, data_mem, n_rows, stage, s));
    return st.finish(s, n, sum, sumsq);
}

qamd_status qamd_bin_thresholds_from_stats(uint64_t dim, const uint64_t *n, const double *sum, const double *sumsq, double t,
                                           float *lo, float *hi) {
    if (dim && (!n || !sum || !sumsq || !lo || !hi)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (t != t) return fail(QAMD_ERR_ARGUMENTS, "t is NaN");
    thresholds_of(dim, n, sum, sumsq, t, lo, hi);
    return QAMD_OK;
}

qamd_status qamd_bin_encode_enc(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp, qamd_bits_store store,
                                qamd_bin_encoding encoding, const float *lo, const float *hi, qamd_stop_fn stop,
                                void *stop_user, void *stream, qamd_bin **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_TRY(refuse_u8_flags(vp));
    QAMD_TRY(check_enc_args(vp, encoding, lo, hi, false));
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    if (vp->count > 0 && vp->dim > 0 && !data) return fail(QAMD_ERR_ARGUMENTS, "data is null");
    QAMD_ON_DEVICE(current_device());
    hipStream_t s = as_stream(stream);
    std::unique_ptr<qamd_bin> h;
    QAMD_TRY(new_store(vp, store, encoding, h));
    if (lo) {
        QAMD_TRY(set_thresholds(h.get(), lo, hi, s));
    } else if (h->two()) {  // one pass over the data (rotated rows: over y) for the statistics, then the rows
        BinStats st;
        DevBuf stage;
        QAMD_TRY(st.begin(h->edim));
        QAMD_TRY(stats_feed(st, data, data_mem, vp->count, stage, s, stop, stop_user, h->rotated() ? vp->dim : 0, h->blocks()));
        QAMD_TRY(set_thresholds_from_stats(h.get(), st, s));
    }
    QAMD_TRY(encode_all(h.get(), data, data_mem, stop, stop_user, s));
    *out = h.release();
    return QAMD_OK;
}

qamd_status qamd_bin_from_rows_enc(const uint8_t *rows, qamd_mem rows_mem, const qamd_vector_parameters *vp,
                                   qamd_bits_store store, qamd_bin_encoding encoding, const float *lo, const float *hi,
                                   void *stream, qamd_bin **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_TRY(refuse_u8_flags(vp));
    QAMD_TRY(check_enc_args(vp, encoding, lo, hi, true));
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    QAMD_ON_DEVICE(current_device());
    std::unique_ptr<qamd_bin> h;
    QAMD_TRY(new_store(vp, store, encoding, h));
    if (h->count && h->nb && !rows) return fail(QAMD_ERR_ARGUMENTS, "rows is null");
    if (lo) QAMD_TRY(set_thresholds(h.get(), lo, hi, as_stream(stream)));
    QAMD_TRY(upload_rows(h.get(), rows, rows_mem, as_stream(stream)));
    QAMD_HIP(hipStreamSynchronize(as_stream(stream)));
    *out = h.release();
    return QAMD_OK;
}

qamd_status qamd_bin_get_encoding(const qamd_bin *h, qamd_bin_encoding *encoding, uint64_t *code_bits) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (encoding) *encoding = (qamd_bin_encoding)h->encoding;
    if (code_bits) *code_bits = h->code_bits;
    return QAMD_OK;
}

qamd_status qamd_bin_get_thresholds(const qamd_bin *h, float *lo, float *hi) {
    if (!h || !lo || !hi) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (!h->two()) return fail(QAMD_ERR_ARGUMENTS, "one-bit rows have no thresholds");
    const uint64_t dim = h->edim;
    if (dim) {
        memcpy(lo, h->thr_host.data(), dim * 4);
        memcpy(hi, h->thr_host.data() + dim, dim * 4);
    }
    return QAMD_OK;
}

qamd_status qamd_bin_encode(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp,
                            qamd_bits_store store, qamd_stop_fn stop, void *stop_user, void *stream,
                            qamd_bin **out) {
    return qamd_bin_encode_enc(data, data_mem, vp, store, QAMD_BIN_ONE_BIT, nullptr, nullptr, stop, stop_user, stream, out);
}

qamd_status qamd_bin_from_rows(const uint8_t *rows, qamd_mem rows_mem, const qamd_vector_parameters *vp,
                               qamd_bits_store store, void *stream, qamd_bin **out) {
    return qamd_bin_from_rows_enc(rows, rows_mem, vp, store, QAMD_BIN_ONE_BIT, nullptr, nullptr, stream, out);
}

// Rows [first_row, first_row + n_rows) as the reference's storage holds them (push_vector_data,
// encoded_storage.rs:17-25), in bounded pieces.
qamd_status qamd_bin_export_rows_range(const qamd_bin *h, uint64_t first_row, uint64_t n_rows, uint8_t *rows,
                                       qamd_mem rows_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    QAMD_TRY(check_row_range(first_row, n_rows, h->count));
    if (n_rows == 0 || h->nb == 0) return QAMD_OK;
    if (!rows) return fail(QAMD_ERR_ARGUMENTS, "rows is null");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint8_t *src = h->rows.as<uint8_t>() + first_row * h->ds;
    if (h->nb == h->ds) return copy_out(rows, rows_mem, src, n_rows * h->nb, s);
    // rows of <= 32 dims are held at a 4-byte stride on the device: re-stride on the way out
    std::vector<uint8_t> wide(n_rows * h->ds), host(n_rows * h->nb);
    QAMD_TRY(copy_out(wide.data(), QAMD_MEM_HOST, src, wide.size(), s));
    for (uint64_t r = 0; r < n_rows; r++) memcpy(&host[r * h->nb], &wide[r * h->ds], h->nb);
    if (rows_mem == QAMD_MEM_HOST) memcpy(rows, host.data(), host.size());
    else QAMD_TRY(copy_in(rows, host.data(), QAMD_MEM_HOST, host.size(), s));
    return QAMD_OK;
}

qamd_status qamd_bin_export_rows(const qamd_bin *h, uint8_t *rows, qamd_mem rows_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    return qamd_bin_export_rows_range(h, 0, h->count, rows, rows_mem, stream);
}

// save/load (:260-286): Metadata{vector_parameters} as serde_json + raw row bytes.
qamd_status qamd_bin_save(const qamd_bin *h, const char *data_path, const char *meta_path) {
    if (!h || !data_path || !meta_path) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    for (float t : h->thr_host)
        if (!(fabsf(t) < __builtin_huge_valf())) return fail(QAMD_ERR_IO, "an infinite threshold has no form in the metadata file");
    std::string js = "{\"vector_parameters\":" + vector_parameters_json(h->vp);
    if (h->encoding != QAMD_BIN_ONE_BIT)  // (a one-bit file stays the reference's, byte for byte)
        js += std::string(",\"encoding\":\"") + (h->two() ? "TwoBits" : "OneBit") + (h->rotated() ? "Rotated" : "") +
              (h->blocks() ? "Blocks" : "") + "\"";
    if (h->two()) {
        js += ",\"thresholds\":{";
        for (int side = 0; side < 2; side++) {
            js += side ? ",\"hi\":[" : "\"lo\":[";
            for (uint64_t i = 0; i < h->edim; i++) {
                if (i) js += ",";
                js += json_f32(h->thr_host[side * h->edim + i]);
            }
            js += "]";
        }
        js += "}";
    }
    js += "}";
    QAMD_TRY(save_file(meta_path, js.data(), js.size()));
    std::vector<uint8_t> rows(h->count * h->nb);
    QAMD_TRY(qamd_bin_export_rows(h, rows.data(), QAMD_MEM_HOST, nullptr));
    return save_file(data_path, rows.data(), rows.size());
}

qamd_status qamd_bin_load(const char *data_path, const char *meta_path, const qamd_vector_parameters *vp,
                          qamd_bits_store store, qamd_bin **out) {
    if (!data_path || !meta_path || !vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_TRY(refuse_u8_flags(vp));
    JsonValue root;
    QAMD_TRY(read_metadata(meta_path, root));
    qamd_vector_parameters file_vp{};
    {   // Metadata{vector_parameters} (encoded_vectors_binary.rs:21-24)
        std::string err;
        const JsonValue *vpj = json_field(root, "vector_parameters", err);
        if (!vpj || !parse_vector_parameters(*vpj, file_vp, err)) return fail(QAMD_ERR_IO, "%s: %s", meta_path, err.c_str());
    }
    // "encoding": absent or "OneBit" is the reference's file; "TwoBits" comes with its thresholds.  Every
    // refusal below is made before a device is needed.
    int encoding = QAMD_BIN_ONE_BIT;
    std::vector<float> thr;
    for (const auto &m : root.members) {
        if (m.first != "encoding") continue;
        if (m.second.kind == JsonValue::String && m.second.text == "TwoBits") encoding = QAMD_BIN_TWO_BITS;
        else if (m.second.kind == JsonValue::String && m.second.text == "OneBitRotated") encoding = QAMD_BIN_ONE_BIT_ROTATED;
        else if (m.second.kind == JsonValue::String && m.second.text == "TwoBitsRotated") encoding = QAMD_BIN_TWO_BITS_ROTATED;
        else if (m.second.kind == JsonValue::String && m.second.text == "OneBitRotatedBlocks") encoding = QAMD_BIN_ONE_BIT_ROTATED_BLOCKS;
        else if (m.second.kind == JsonValue::String && m.second.text == "TwoBitsRotatedBlocks") encoding = QAMD_BIN_TWO_BITS_ROTATED_BLOCKS;
        else if (m.second.kind != JsonValue::String || m.second.text != "OneBit")
            return fail(QAMD_ERR_IO, "%s: unknown encoding", meta_path);
    }
    if ((encoding & QAMD_BIN_ROTATED) && vp->dim > kRotMaxDim)
        return fail(QAMD_ERR_IO, "%s: rotated rows of %llu dimensions", meta_path, (unsigned long long)vp->dim);
    if ((encoding & QAMD_BIN_BLOCKS) && vp->dim % kRotBlockMin != 0)
        return fail(QAMD_ERR_IO, "%s: block-rotated rows of %llu dimensions, not a multiple of %llu", meta_path,
                    (unsigned long long)vp->dim, (unsigned long long)kRotBlockMin);
    const uint64_t edim = encoder_dim(vp->dim, encoding);  // thresholds of a rotated file have P entries, dim of a
                                                           // block-rotated one (3.2h)
    if (encoding & QAMD_BIN_TWO_BITS) {
        std::string err;
        const JsonValue *tj = json_field(root, "thresholds", err);
        if (!tj) return fail(QAMD_ERR_IO, "%s: TwoBits: %s", meta_path, err.c_str());
        if (vp->dim > kTwoBitMaxDim) return fail(QAMD_ERR_IO, "%s: two-bit rows of %llu dimensions", meta_path, (unsigned long long)vp->dim);
        thr.resize(2 * edim);
        for (int side = 0; side < 2; side++) {
            const JsonValue *a = json_field(*tj, side ? "hi" : "lo", err);
            if (!a) return fail(QAMD_ERR_IO, "%s: thresholds: %s", meta_path, err.c_str());
            if (a->kind != JsonValue::Array || a->items.size() != edim)
                return fail(QAMD_ERR_IO, "%s: thresholds: expected %llu values per side", meta_path, (unsigned long long)edim);
            for (uint64_t i = 0; i < edim; i++)
                if (!json_number_as_f32(a->items[i], thr[side * edim + i], err))
                    return fail(QAMD_ERR_IO, "%s: thresholds: %s", meta_path, err.c_str());
        }
        for (uint64_t i = 0; i < edim; i++)
            if (!(thr[i] <= thr[edim + i])) return fail(QAMD_ERR_IO, "%s: thresholds: lo > hi at %llu", meta_path, (unsigned long long)i);
    }
    std::string bytes;
    const uint64_t code_bits = (encoding & QAMD_BIN_TWO_BITS) ? 2 * edim : edim;
    QAMD_TRY(load_rows_file(data_path, row_bytes_of(code_bits, store) * vp->count, bytes));  // :277-279
    qamd_vector_parameters eff = file_vp;  // metadata rules the metric, the caller's params the sizes
    eff.dim = vp->dim;
    eff.count = vp->count;
    if (encoding != QAMD_BIN_ONE_BIT)
        return qamd_bin_from_rows_enc(reinterpret_cast<const uint8_t *>(bytes.data()), QAMD_MEM_HOST, &eff, store,
                                      (qamd_bin_encoding)encoding, thr.empty() ? nullptr : thr.data(),
                                      thr.empty() ? nullptr : thr.data() + edim, nullptr, out);
    return qamd_bin_from_rows(reinterpret_cast<const uint8_t *>(bytes.data()), QAMD_MEM_HOST, &eff, store, nullptr,
                              out);
}

// Where a query keeps max_abs, and behind it its f32 staging area, after `bits` planes of ds bytes.
static uint64_t scalar_max_abs_at(uint64_t ds, uint32_t bits) { return round_up(bits * ds, 16) + 16; }

// The most dimensions a `bits`-bit scalar query may have: code_bits * (2^bits - 1) and every sum below it must be exact
// in f32, so the row's bits stay at or under 65 792 (8 bits) / 1 118 481 (4 bits) - half as many dimensions on two-bit rows.
static uint64_t scalar_max_dim(uint32_t bits, bool two) { return (bits == 8 ? 65792u : 1118481u) / (two ? 2u : 1u); }

// Every single-query encode.  bits = 1: the reference's binary query, one plane from the row encoder.  bits = 4 / 8 have
// no counterpart there: DESIGN 3.2d is the specification, 3.2f that of `weighted` on two-bit rows (codes from
// q_i * (hi_i - lo_i), sized by code_bits); on one-bit rows both are the same call.
static qamd_status encode_query(const qamd_bin *h, const float *query, uint64_t qdim, qamd_mem query_mem, uint32_t bits,
                                bool weighted, void *stream, qamd_bin_query **query_io) {
    if (bits != 1 && bits != 4 && bits != 8) return fail(QAMD_ERR_ARGUMENTS, "query bits must be 1, 4 or 8, not %u", bits);
    if (!h || !query_io || (!query && qdim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    const bool two = h->two();  // the row's thresholds and layout
    if (bits != 1 && two && !weighted)
        return fail(QAMD_ERR_ARGUMENTS, "two-bit rows take scalar queries through qamd_bin_encode_query_scalar_w");
    if (two && qdim != h->vp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "a query of %llu dimensions against thresholds of %llu", (unsigned long long)qdim,
                    (unsigned long long)h->vp.dim);
    if (h->rotated() && qdim != h->vp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "a query of %llu dimensions against rotated rows of %llu", (unsigned long long)qdim,
                    (unsigned long long)h->vp.dim);
    const uint64_t edim = encoder_dim(qdim, h->encoding);  // a rotated query is encoded as P values
    const uint64_t max_dim = scalar_max_dim(bits, two);
    if (bits != 1 && edim > max_dim)
        return fail(QAMD_ERR_ARGUMENTS, "a %u-bit query has at most %llu dimensions, not %llu", bits,
                    (unsigned long long)max_dim, (unsigned long long)edim);
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t nb = row_bytes_of(two ? 2 * edim : edim, h->store), ds = device_stride_of(nb);
    const uint64_t max_abs_at = scalar_max_abs_at(ds, bits), need = max_abs_at + 16 + qdim * 4 + 16;
    qamd_bin_query *q = *query_io;
    std::unique_ptr<qamd_bin_query> fresh;
    if (!q) {
        fresh.reset(new qamd_bin_query);
        q = fresh.get();
        q->device = h->device;
    }
    if (q->ds != ds || q->qdim_cap < qdim || !q->buf.ptr || q->buf.bytes < need) {
        QAMD_TRY(q->buf.alloc(need, true));  // planes | max_abs | f32 staging
        q->qdim_cap = qdim;
        q->nb = nb;
        q->ds = ds;
    }
    q->bits = bits;
    // Always encoded on the device (one implementation); a host query is uploaded first.
    const float *q_dev = query;
    if (qdim && query_mem == QAMD_MEM_HOST) {
        float *stage = reinterpret_cast<float *>(q->buf.as<uint8_t>() + max_abs_at + 16);
        QAMD_TRY(copy_in(stage, query, QAMD_MEM_HOST, qdim * 4, s));
        q_dev = stage;
    }
    if (bits == 1)
        launch_bit_encoder(h, q_dev, 1, qdim, ds / 4, q->buf.as<uint32_t>(), 0, s);
    else
        QAMD_TRY(launch_scalar_encoder(h, q_dev, 1, qdim, ds, bits, q->buf.as<uint32_t>(), 0,
                                       reinterpret_cast<float *>(q->buf.as<uint8_t>() + max_abs_at), nullptr, 0, s));
    QAMD_HIP(hipGetLastError());
    QAMD_TRY(q->ready.record(s));
    if (fresh) *query_io = fresh.release();
    return QAMD_OK;
}

qamd_status qamd_bin_encode_query(const qamd_bin *h, const float *query, uint64_t qdim, qamd_mem query_mem,
                                  void *stream, qamd_bin_query **query_io) {
    return encode_query(h, query, qdim, query_mem, 1, false, stream, query_io);
}

qamd_status qamd_bin_encode_query_scalar(const qamd_bin *h, const float *query, uint64_t qdim, qamd_mem query_mem,
                                         uint32_t bits, void *stream, qamd_bin_query **query_io) {
    return encode_query(h, query, qdim, query_mem, bits, false, stream, query_io);
}

qamd_status qamd_bin_encode_query_scalar_w(const qamd_bin *h, const float *query, uint64_t qdim, qamd_mem query_mem,
                                           uint32_t bits, void *stream, qamd_bin_query **query_io) {
    return encode_query(h, query, qdim, query_mem, bits, true, stream, query_io);
}

qamd_status qamd_bin_query_info(const qamd_bin_query *q, uint32_t *bits, float *max_abs) {
    if (!q) return fail(QAMD_ERR_ARGUMENTS, "null query");
    if (bits) *bits = q->bits;
    if (max_abs) {
        *max_abs = 0.0f;
        if (q->bits != 1) {
            QAMD_ON_DEVICE(q->device);
            QAMD_TRY(q->ready.wait(nullptr));
            QAMD_TRY(copy_out(max_abs, QAMD_MEM_HOST, q->buf.as<uint8_t>() + scalar_max_abs_at(q->ds, q->bits), 4, nullptr));
        }
    }
    return QAMD_OK;
}

qamd_status qamd_bin_query_read(const qamd_bin_query *q, uint8_t *bits, uint64_t capacity, uint64_t *len) {
    if (!q) return fail(QAMD_ERR_ARGUMENTS, "null query");
    const uint64_t total = q->bits * q->nb;  // a scalar query: its planes, plane 0 first, nb bytes each
    if (len) *len = total;
    if (bits) {
        if (capacity < total) return fail(QAMD_ERR_ARGUMENTS, "bits buffer too small");
        QAMD_ON_DEVICE(q->device);
        QAMD_TRY(q->ready.wait(nullptr));
        if (q->bits == 1 || q->nb == q->ds) {
            QAMD_TRY(copy_out(bits, QAMD_MEM_HOST, q->buf.ptr, total, nullptr));
        } else {  // tiny rows: planes are held at the 4-byte device stride
            std::vector<uint8_t> wide(q->bits * q->ds);
            QAMD_TRY(copy_out(wide.data(), QAMD_MEM_HOST, q->buf.ptr, wide.size(), nullptr));
            for (uint32_t b = 0; b < q->bits; b++) memcpy(bits + b * q->nb, &wide[b * q->ds], q->nb);
        }
    }
    return QAMD_OK;
}

void qamd_bin_query_free(qamd_bin_query *q) { delete q; }

}  // extern "C"

namespace {  // the null-list burst of score_internal (defined with the multi-query scans below)
uint32_t internal_batch_group(const qamd_bin *h);
qamd_status score_internal_rows_dev(const qamd_bin *h, const uint32_t *rows_dev, uint32_t n, uint64_t n_ids, float *out_dev,
                                    hipStream_t s);
}  // namespace

extern "C" {

// score_all for a device pointer to query bits (`planes` planes): an encoded query's buffer or, for score_internal_all,
// a stored row of the image the scan reads.
static qamd_status score_all_bits(const qamd_bin *h, const void *qbits, uint32_t planes, float *out, qamd_mem out_mem,
                                  hipStream_t s) {
    if (out_mem == QAMD_MEM_DEVICE) return scan_bits(h, qbits, out, s, nullptr, planes);
    return score_all_to_host(h->count, out, s, [&](float *scores) { return scan_bits(h, qbits, scores, s, nullptr, planes); });
}

qamd_status qamd_bin_score_all(const qamd_bin *h, const qamd_bin_query *q, float *out, qamd_mem out_mem,
                               void *stream) {
    QAMD_TRY(check_query(h, q));
    if (h->count == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "out is null");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    QAMD_TRY(q->ready.wait(s));
    return score_all_bits(h, q->buf.ptr, q->bits, out, out_mem, s);
}

qamd_status qamd_bin_score_ids(const qamd_bin *h, const qamd_bin_query *q, const uint32_t *ids, uint64_t n_ids,
                               qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream) {
    QAMD_TRY(check_query(h, q));
    if (n_ids == 0) return QAMD_OK;
    if (!ids || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    QAMD_TRY(q->ready.wait(s));
    return score_ids_any(h, q->buf.as<uint32_t>(), ids, n_ids, ids_mem, out, out_mem, s, q->bits);
}

qamd_status qamd_bin_score_point(const qamd_bin *h, const qamd_bin_query *q, uint32_t i, float *out) {
    return qamd_bin_score_ids(h, q, &i, 1, QAMD_MEM_HOST, out, QAMD_MEM_HOST, nullptr);
}

// score_internal (:302-314) for one stored row against many: out[k] = score_internal(i, ids[k]).
qamd_status qamd_bin_score_internal_ids(const qamd_bin *h, uint32_t i, const uint32_t *ids, uint64_t n_ids,
                                        qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (n_ids == 0) return QAMD_OK;
    if (!ids) QAMD_TRY(check_null_ids(n_ids, out, h->count));  // a null list stands for the rows 0 .. n_ids - 1
    else if (!out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (i >= h->count) return fail(QAMD_ERR_OUT_OF_RANGE, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    if (!ids) {  // score_internal_all's scan over a prefix of the store
        hipStream_t s = as_stream(stream);
        const uint8_t *qbits = h->rows.as<uint8_t>() + (uint64_t)i * h->ds;
        if (out_mem == QAMD_MEM_DEVICE) return scan_bits(h, qbits, out, s, nullptr, 1, n_ids);
        return score_all_to_host(n_ids, out, s, [&](float *scores) { return scan_bits(h, qbits, scores, s, nullptr, 1, n_ids); });
    }
    return score_ids_any(h, h->rows.as<uint32_t>() + (uint64_t)i * (h->ds / 4), ids, n_ids, ids_mem, out, out_mem,
                         as_stream(stream));
}

qamd_status qamd_bin_score_internal(const qamd_bin *h, uint32_t i, uint32_t j, float *out) {
    if (!h || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (j >= h->count) return fail(QAMD_ERR_OUT_OF_RANGE, "row id out of range (count %llu)", (unsigned long long)h->count);
    return qamd_bin_score_internal_ids(h, i, &j, 1, QAMD_MEM_HOST, out, QAMD_MEM_HOST, nullptr);
}

// Many stored rows, each against its own id list, in one launch (lists.hpp).
qamd_status qamd_bin_score_internal_ids_batch(const qamd_bin *h, const uint32_t *rows, const uint32_t *list_offsets,
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
        return pairs_launch(h, nullptr, nullptr, 0, a.offsets, a.n_lists, a.rows, a.ids, a.n_pairs, a.out, s);
    });
}

// The routes of topk for a device pointer to query bits, as score_all_bits.
static qamd_status topk_bits(const qamd_bin *h, const void *qbits, uint32_t planes, uint32_t k, int largest, uint32_t *out_ids,
                             float *out_scores, qamd_mem out_mem, hipStream_t s) {
    {   // small stores: one launch, exact under any number of ties, no status read-back
        qamd_status st = QAMD_OK;
        if (bin_topk_small(h, qbits, k, largest, out_ids, out_scores, out_mem, s, st, planes)) return st;
    }
    if (!fused_capable(h)) {
        return topk_classic(h->count, k, largest, out_ids, out_scores, out_mem, s,
                            [&](float *scores) { return scan_bits(h, qbits, scores, s, nullptr, planes); });
    }
    FusedScan scan;
    scan.scan_scores = [&](float *scores, hipStream_t st) { return scan_bits(h, qbits, scores, st, nullptr, planes); };
    scan.scan_filter = [&](const TopkFilter &f, hipStream_t st) { return scan_bits(h, qbits, nullptr, st, &f, planes); };
    scan.score_ids = [&](const uint32_t *ids, uint64_t n_ids, float *out, hipStream_t st) {
        return words_launch(h, static_cast<const uint32_t *>(qbits), ids, n_ids, out, st, planes);
    };
    return fused_topk(h->count, k, largest, out_ids, out_scores, out_mem, s, scan);
}

qamd_status qamd_bin_topk(const qamd_bin *h, const qamd_bin_query *q, uint32_t k, int largest, uint32_t *out_ids,
                          float *out_scores, qamd_mem out_mem, void *stream) {
    QAMD_TRY(check_query(h, q));
    qamd_status args = QAMD_OK;
    if (!topk_wanted(k, 1, out_ids, out_scores, args)) return args;
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    QAMD_TRY(q->ready.wait(s));
    return topk_bits(h, q->buf.ptr, q->bits, k, largest, out_ids, out_scores, out_mem, s);
}

// score_internal (:302-314) against the whole store: the metric of score_point with stored row i as the one-plane query,
// for one-bit and two-bit rows alike.  The query pointer is row i of the image every route scans (16-byte aligned wherever
// the 16-byte kernels run: ds % 16 == 0 there); every kernel only reads both, and reads the query within its ds bytes.
qamd_status qamd_bin_score_internal_all(const qamd_bin *h, uint32_t i, float *out, qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (h->count == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "out is null");
    if (i >= h->count) return fail(QAMD_ERR_ARGUMENTS, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    return score_all_bits(h, h->rows.as<uint8_t>() + (uint64_t)i * h->ds, 1, out, out_mem, as_stream(stream));
}

qamd_status qamd_bin_topk_internal(const qamd_bin *h, uint32_t i, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                                   qamd_mem out_mem, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    qamd_status args = QAMD_OK;
    if (!topk_wanted(k, 1, out_ids, out_scores, args)) return args;
    if (h->count && i >= h->count) return fail(QAMD_ERR_ARGUMENTS, "row id %u out of range (count %llu)", i, (unsigned long long)h->count);
    QAMD_ON_DEVICE(h->device);
    return topk_bits(h, h->rows.as<uint8_t>() + (uint64_t)i * h->ds, 1, k, largest, out_ids, out_scores, out_mem,
                     as_stream(stream));
}

void qamd_bin_free(qamd_bin *h) { delete h; }

}  // extern "C"


// ============================================================================= many queries at once
// The caller's outer loop over queries (demos/src/ann_benchmark.rs:245-260).  score_batch reads every
// row ONCE for up to 8 queries (bin_scan_multi_kernel); topk_batch enqueues the per-query fused
// pipelines back to back (fused_topk_batch: one status read-back per 32 queries).
struct qamd_bin_query_batch {
    int device = 0;
    uint64_t nb = 0, ds = 0, n_queries = 0;
    uint32_t qbits = 1;       // bits per query dimension: 1 (the reference's binary query), 4 or 8
    uint64_t p_stride = 0;    // bytes between two queries' planes (multiple of 16); a query's planes as in qamd_bin_query
    DevBuf planes;            // [n_queries][p_stride]: a binary batch is a batch of one plane, the query's bit row
    // a batch of scalar queries (qamd_bin_encode_query_batch_scalar) holds a second image for the matrix cores:
    uint64_t code_pitch = 0;  // bytes between two queries' centred int8 codes: bin_gemm_rs_kernel's LDS pitch of this row length
    DevBuf codes;             // [n_queries][code_pitch]: d_i, zero bytes, C = sum c_i in the last 16
    DevBuf max_abs;           // [n_queries] f32
};

// Query q of the batch as scan_bits / words_launch / bin_topk_small take it: its planes (its bit row at qbits = 1).
static const uint8_t *bin_batch_query(const qamd_bin_query_batch *b, uint64_t q) {
    return b->planes.as<uint8_t>() + q * b->p_stride;
}

namespace {

template <int G, int ITERS, int UNROLL, int NQ>
void launch_bin_multi(const qamd_bin *h, const uint8_t *qbits, uint64_t q_stride, float *out, hipStream_t s,
                      const TopkFilterSlices *slices = nullptr, uint64_t n_rows = 0) {
    constexpr int TILE = (64 / G) * UNROLL;
    const uint32_t rc = (uint32_t)(h->ds / 16);
    const uint64_t n = n_rows ? n_rows : h->count;  // rows scanned, also the pitch of `out`
    const uint64_t waves = (n + TILE - 1) / TILE;
    const unsigned grid = (unsigned)((waves + kScanBlock / 64 - 1) / (kScanBlock / 64));
    const bool exact = rc == (uint32_t)(G * ITERS);
#define QAMD_BIN_MULTI(EX, FI)                                                                                    \
    hipLaunchKernelGGL((bin_scan_multi_kernel<G, ITERS, UNROLL, NQ, EX, FI>), dim3(grid), dim3(kScanBlock), 0, s, \
                       h->rows.as<uint4>(), reinterpret_cast<const uint4 *>(qbits), (uint32_t)(q_stride / 16),    \
                       metric_dim(h, 1), (int)(h->vp.distance_type == QAMD_DOT), h->vp.invert, (uint32_t)n,       \
                       rc, out, n, slices ? *slices : TopkFilterSlices{})
    if (slices) {
        if (exact) QAMD_BIN_MULTI(true, true);
        else QAMD_BIN_MULTI(false, true);
    } else {
        if (exact) QAMD_BIN_MULTI(true, false);
        else QAMD_BIN_MULTI(false, false);
    }
#undef QAMD_BIN_MULTI
}

// The rows bin_scan_multi_kernel has forms for: 8 .. 64 pieces (every such store has the 4- and 2-query forms).
bool multi_rows(const qamd_bin *h) { return h->ds % 16 == 0 && h->ds / 16 >= 8 && h->ds / 16 <= 64; }

// Queries [q0, q0 + nq) with nq in {8, 4, 2}: rows of 8 .. 64 pieces (dims 1024 .. 8192 at the u128 granule).
template <int NQ> bool multi_step(const qamd_bin *h, const uint8_t *qbits, uint64_t q_stride, float *out, hipStream_t s,
                                  const TopkFilterSlices *slices = nullptr, uint64_t n_rows = 0) {
    const uint32_t rc = (uint32_t)(h->ds / 16);
    if (!multi_rows(h)) return false;
    if (rc == 8) launch_bin_multi<8, 1, 8, NQ>(h, qbits, q_stride, out, s, slices, n_rows);
    else if (rc <= 16) launch_bin_multi<16, 1, 4, NQ>(h, qbits, q_stride, out, s, slices, n_rows);
    else if (rc <= 32) launch_bin_multi<16, 2, 2, NQ>(h, qbits, q_stride, out, s, slices, n_rows);
    else if (NQ <= 4) launch_bin_multi<16, 4, 2, NQ>(h, qbits, q_stride, out, s, slices, n_rows);
    else return false;
    return true;
}

// ---- score_internal of many stored rows against the rows 0 .. n_ids - 1 (the null-list burst) ----
// Workgroup l copies the ds bytes of stored row rows[l] to qbits[l][..]: the contiguous [n][ds] block the scans read as
// one-plane queries.  `rows` is device memory (no read-back); a row >= count is clamped to row 0 and its list becomes NaN
// afterwards (null_list_nan_kernel).
__global__ __launch_bounds__(64) void bin_gather_rows_kernel(const uint32_t *__restrict__ store, const uint32_t *__restrict__ rows,
                                                             uint32_t count, uint32_t row_words, uint32_t *__restrict__ qbits) {
    const uint32_t l = blockIdx.x;
    uint32_t r = rows[l];
    if (r >= count) r = 0;
    const uint32_t *src = store + (uint64_t)r * row_words;
    uint32_t *dst = qbits + (uint64_t)l * row_words;
    for (uint32_t w = threadIdx.x; w < row_words; w += 64) dst[w] = src[w];
}

uint32_t internal_batch_group(const qamd_bin *h) {
    return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(8, (8ull << 20) / std::max<uint64_t>(h->ds, 1)));
}

// out_dev[l * n_ids + j] = score_internal(rows_dev[l], j) for l < n, j < n_ids <= count: score_internal is the metric of
// a one-plane query whose bits are the stored row, so the gathered rows go through the multi-query passes (8, 4, 2 rows
// per read of the store; rows of 8 .. 64 pieces) and the rest - remainders, other row sizes - through scan_bits per row.
qamd_status score_internal_rows_dev(const qamd_bin *h, const uint32_t *rows_dev, uint32_t n, uint64_t n_ids, float *out_dev,
                                    hipStream_t s) {
    StreamBuf stage;
    QAMD_TRY(stage.alloc((size_t)n * h->ds, s));
    const uint8_t *qbits = stage.as<uint8_t>();
    hipLaunchKernelGGL(bin_gather_rows_kernel, dim3(n), dim3(64), 0, s, h->rows.as<uint32_t>(), rows_dev, (uint32_t)h->count,
                       (uint32_t)(h->ds / 4), stage.as<uint32_t>());
    QAMD_HIP(hipGetLastError());
    for (uint32_t l = 0; l < n;) {
        const uint32_t left = n - l;
        const uint8_t *qb = qbits + (uint64_t)l * h->ds;
        float *o = out_dev + (uint64_t)l * n_ids;
        if (left >= 8 && multi_step<8>(h, qb, h->ds, o, s, nullptr, n_ids)) l += 8;
        else if (left >= 4 && multi_step<4>(h, qb, h->ds, o, s, nullptr, n_ids)) l += 4;
        else if (left >= 2 && multi_step<2>(h, qb, h->ds, o, s, nullptr, n_ids)) l += 2;
        else {
            QAMD_TRY(scan_bits(h, qb, o, s, nullptr, 1, n_ids));
            l += 1;
        }
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

}  // namespace

// ============================================================================= many queries on the matrix cores
// A binary store is a u8 store in disguise: bits as 0/1 bytes, a = popcount(q AND v) as the int8 contraction,
// xor = pop(q) + pop(v) - 2a, and the reference's metric (calculate_metric, :237-252)
//   zeros - xor = dim - 2 xor = (4a + (dim - 2 pop_q)) + (-2 pop_v)        (Dot, or L1/L2 inverted)
//   xor - zeros = 2 xor - dim = (-4a + (2 pop_q - dim)) + (2 pop_v)        (the other two cases)
// is the u8 epilogue (multiplier * s + q_offset) + v_offset with integer operands below 2^23: every f32 in it is
// exact, so the scores are the reference's bit for bit.  bin_gemm_rs_kernel is u8_gemm_rs_kernel's structure
// (csrc/u8_batch.hip: query tile resident in LDS, every wave streams its own 64 rows, no barrier after the
// set-up) with the rows kept as BITS up to the registers: lane (r, h) loads the 8 bytes [16 kb + 8h, +8) of row
// r per 128-bit K-block and expands 16 bits to 16 operand bytes (umul24(nibble, 0x00204081) & 0x01010101) right before
// the MFMAs that use them; the row's popcount falls out of the same loads.  HBM sees 1/8 of the bytes the
// contraction works on, so the kernel is matrix-pipe / VALU-bound from the first query tile on.
// The pre-filter starts the accumulators at -B_q and compares against the row's bound after the K loop (the
// row term is only known once the row has been read); the rest - pivots from a sample, wave-private candidate
// lists, scatter, emit - is batch_common.hpp's, as for u8.
namespace {

//
// CODES (a batch of 4- or 8-bit scalar queries): the same contraction with another byte per dimension.  With
// the centred codes d_i = c_i - (L + 1) / 2 (int8: [-8, 7] or [-128, 127]), A = sum_i s_i d_i, C = sum c_i and P = pop_v,
//   X = sum_b 2^b popcount(plane_b xor row) = C - P - 2A
//   dim L - 2X = (4A + (dim L - 2C)) + 2P        2X - dim L = (-4A + (2C - dim L)) - 2P
// - the epilogue above with q_offset from C and the OTHER sign of the row term.  `qbits` is then the batch's code image
// (bin_encode_scalar_kernel: q_stride = this kernel's LDS pitch, d_i bytes, C in the last 16 bytes), copied into the
// tile 16 bytes at a time, and dim_f is dim * L.  4- and 8-bit queries are both one int8 per dimension: one instantiation
// serves both.  Exact for the same reason: |4A| <= 512 dim, |q_offset| <= 255 dim, 2P <= 2 dim, and the route takes rows
// of at most 4992 bits (bin_mfma_frags), so every operand and partial sum stays below 769 * 4992 < 2^22.
template <int MODE, bool LOW, int MI, bool CODES = false>  // MODE 0: scores out; 1 / 2: filter for the largest / smallest
__global__ __launch_bounds__(512) void bin_gemm_rs_kernel(const uint8_t *__restrict__ rows, uint32_t ds,
                                                         const uint8_t *__restrict__ qbits, uint32_t q_stride, float dim_f,
                                                         int zx, uint32_t n_rows, uint32_t n_queries, uint32_t q0,
                                                         float *__restrict__ out, uint64_t out_pitch, BatchFilter filt) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[];
    constexpr int MJ = 2, TQ = 32 * MI, CHUNK = 64;
    constexpr bool FILTER = MODE != 0, LARGEST = MODE == 1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 31, h = lane >> 5;
    const uint32_t nkb = __builtin_amdgcn_readfirstlane(ds / 16);  // 128-bit K-blocks per row
    const uint32_t PA = nkb * 128 + 16;                            // LDS pitch of a query (one byte per bit)
    const float multiplier = zx ? 4.0f : -4.0f;
    float *q_off_s = reinterpret_cast<float *>(lds_raw + (size_t)TQ * PA);  // [64]
    float *pivot_s = q_off_s + 64;                                          // [64]
    int *bq_s = reinterpret_cast<int *>(pivot_s + 64);                      // [64]
    uint32_t *wcount_s = reinterpret_cast<uint32_t *>(bq_s + 64) + wave;
    if (FILTER && lane == 0) *wcount_s = 0;
    auto expand = [](uint32_t bits16) {  // 16 bits -> 16 bytes of 0 / 1
        // nibble * (1 + 2^7 + 2^14 + 2^21) puts bit j at position 8j; both factors fit the full-rate 24-bit
        // multiply (v_mul_u32_u24: 4 cycles; v_mul_lo_u32 is quarter rate and made this the kernel's bound)
        v4i v;
        v.x = (int)(__umul24(bits16 & 0xFu, 0x00204081u) & 0x01010101u);
        v.y = (int)(__umul24((bits16 >> 4) & 0xFu, 0x00204081u) & 0x01010101u);
        v.z = (int)(__umul24((bits16 >> 8) & 0xFu, 0x00204081u) & 0x01010101u);
        v.w = (int)(__umul24((bits16 >> 12) & 0xFu, 0x00204081u) & 0x01010101u);
        return v;
    };
    // the query tile as bytes (queries past the batch: zero), its offsets and integer bounds
    if (CODES) {
        for (uint32_t idx = t; idx < (uint32_t)TQ * (PA / 16); idx += 512) {  // 16 code bytes each: q_stride == PA
            const uint32_t q = idx / (PA / 16), piece = idx % (PA / 16);
            v4i d = {0, 0, 0, 0};
            if (q0 + q < n_queries) d = *reinterpret_cast<const v4i *>(qbits + (uint64_t)(q0 + q) * q_stride + piece * 16);
            *reinterpret_cast<v4i *>(lds_raw + q * PA + piece * 16) = d;
        }
    } else
    for (uint32_t idx = t; idx < (uint32_t)TQ * nkb * 8; idx += 512) {  // 16 bits each
        const uint32_t q = idx / (nkb * 8), piece = idx % (nkb * 8);
        uint32_t bits16 = 0;
        if (q0 + q < n_queries) bits16 = *reinterpret_cast<const uint16_t *>(qbits + (uint64_t)(q0 + q) * q_stride + piece * 2);
        *reinterpret_cast<v4i *>(lds_raw + q * PA + piece * 16) = expand(bits16);
    }
    if (t < TQ) {
        uint32_t pq = 0;  // CODES: C = sum c_i, kept behind the query's code bytes
        if (CODES) {
            if (q0 + t < n_queries) pq = *reinterpret_cast<const uint32_t *>(qbits + (uint64_t)(q0 + t) * q_stride + nkb * 128);
        } else
        if (q0 + t < n_queries)
            for (uint32_t w = 0; w < nkb * 4; w++) pq += __popc(*reinterpret_cast<const uint32_t *>(qbits + (uint64_t)(q0 + t) * q_stride + w * 4));
        const float qo = zx ? dim_f - 2.0f * (float)pq : 2.0f * (float)pq - dim_f;
        q_off_s[t] = qo;
        if (FILTER) {
            const float pv = q0 + t < n_queries ? filt.pivot_scores[q0 + t] : (LARGEST ? __builtin_huge_valf() : -__builtin_huge_valf());
            pivot_s[t] = pv;
            int bq = pp_bound<LOW>(pv - qo, fabsf(pv) + fabsf(qo), multiplier, 1);
            if (__builtin_isinf(pv)) bq = ((pv > 0.0f) == LARGEST) == LOW ? -(int)kPpLim : (int)kPpLim;
            bq_s[t] = bq;
        }
    }
    __syncthreads();

    const uint32_t n_chunks = (n_rows + CHUNK - 1) / CHUNK, stride = gridDim.x * 8;
    const uint8_t *a_base = lds_raw + r * PA + 64 * h;
    uint2 cur[MJ][8];  // up to 8 K-blocks in registers at a time (rows of up to 1024 bits per pass)
    for (uint32_t chunk = blockIdx.x * 8 + wave; chunk < n_chunks; chunk += stride) {
        const uint64_t row0 = (uint64_t)chunk * CHUNK;
        v16i acc[MI][MJ];
        uint32_t pop[MJ] = {0, 0};
#pragma unroll
        for (int i = 0; i < MI; i++)
#pragma unroll
            for (int gq = 0; gq < 4; gq++) {
                v4i b4 = {0, 0, 0, 0};
                if (FILTER) b4 = *reinterpret_cast<const v4i *>(bq_s + i * 32 + 8 * gq + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int jj = 0; jj < MJ; jj++) acc[i][jj][4 * gq + e] = -b4[e];
            }
        for (uint32_t kb0 = 0; kb0 < nkb; kb0 += 8) {  // the store's rows are padded: reads past a row stay in bounds
            const uint32_t nk = nkb - kb0 < 8 ? nkb - kb0 : 8;
#pragma unroll
            for (int jj = 0; jj < MJ; jj++) {
                const uint8_t *p = rows + (row0 + jj * 32 + r) * ds + (size_t)kb0 * 16 + 8 * h;
#pragma unroll
                for (int kb = 0; kb < 8; kb++)
                    cur[jj][kb] = (uint32_t)kb < nk ? *reinterpret_cast<const uint2 *>(p + 16 * kb) : make_uint2(0, 0);
            }
#pragma unroll
            for (int kb = 0; kb < 8; kb++) {
                if ((uint32_t)kb >= nk) break;
#pragma unroll
                for (int jj = 0; jj < MJ; jj++) pop[jj] += __popc(cur[jj][kb].x) + __popc(cur[jj][kb].y);
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    v4i bf[MJ];
#pragma unroll
                    for (int jj = 0; jj < MJ; jj++) {
                        const uint32_t word = (x < 2) ? cur[jj][kb].x : cur[jj][kb].y;
                        bf[jj] = expand((word >> (16 * (x & 1))) & 0xFFFFu);
                    }
#pragma unroll
                    for (int i = 0; i < MI; i++) {
                        const v4i a = *reinterpret_cast<const v4i *>(a_base + (uint32_t)i * 32u * PA + (kb0 + kb) * 128 + 16 * x);
#pragma unroll
                        for (int jj = 0; jj < MJ; jj++) acc[i][jj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bf[jj], acc[i][jj], 0, 0, 0);
                    }
                }
            }
        }
        // ---- epilogue: rows on the lanes (r; the two halves h hold the two halves of every K-block's bits)
        uint4 *wave_list = FILTER ? filt.wave_cand + (uint64_t)(filt.wave_base + blockIdx.x * 8 + wave) * filt.wave_cap : nullptr;
#pragma unroll
        for (int jj = 0; jj < MJ; jj++) {
            const uint32_t pv = pop[jj] + (uint32_t)__shfl_xor((int)pop[jj], 32);
            const uint64_t row = row0 + jj * 32 + r;
            const bool row_ok = row < n_rows;
            const float v_off = ((zx != 0) != CODES) ? -2.0f * (float)pv : 2.0f * (float)pv;  // CODES: the row term's sign is the other one
            int br = 0;
            // (a row past the end gets the bound of "never"; the accumulators of CODES can be negative and fall below
            // -2^29 next to an "always" query bound, so there it is INT_MIN / INT_MAX, which no accumulator reaches)
            constexpr int kNever = CODES ? 0x7FFFFFFF : (int)kPpLim;
            if (FILTER) br = row_ok ? pp_bound<LOW>(-v_off, fabsf(v_off), multiplier, 0) : (LOW ? -kNever - (CODES ? 1 : 0) : kNever);
#pragma unroll
            for (int i = 0; i < MI; i++) {
                if (FILTER) {  // "some accumulator of the tile may pass": the largest is >= the row bound (LOW: the smallest <)
                    int ext = acc[i][jj][0];
#pragma unroll
                    for (int e = 1; e < 15; e += 2)
                        ext = LOW ? min(min(ext, acc[i][jj][e]), acc[i][jj][e + 1]) : max(max(ext, acc[i][jj][e]), acc[i][jj][e + 1]);
                    ext = LOW ? min(ext, acc[i][jj][15]) : max(ext, acc[i][jj][15]);
                    if (!__builtin_amdgcn_readfirstlane(__ballot(LOW ? ext < br : ext >= br) != 0)) continue;
                }
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const uint32_t ql = i * 32 + 8 * gq + 4 * h;
                    const float4 qo4 = *reinterpret_cast<const float4 *>(q_off_s + ql);
                    const float qo[4] = {qo4.x, qo4.y, qo4.z, qo4.w};
                    if (!FILTER) {
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float sc = (multiplier * (float)acc[i][jj][4 * gq + e] + qo[e]) + v_off;
                            const uint32_t q = q0 + ql + e;
                            if (row_ok && q < n_queries) out[(uint64_t)q * out_pitch + row] = sc;
                        }
                    } else {
                        const v4i bq4 = *reinterpret_cast<const v4i *>(bq_s + ql);
                        const float4 pv4 = *reinterpret_cast<const float4 *>(pivot_s + ql);
                        const float pvt[4] = {pv4.x, pv4.y, pv4.z, pv4.w};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int av = acc[i][jj][4 * gq + e];
                            if (LOW ? av < br : av >= br) {  // may pass: the exact f32 comparison decides
                                const float sc = (multiplier * (float)(av + bq4[e]) + qo[e]) + v_off;
                                const float d = LARGEST ? sc - pvt[e] : pvt[e] - sc;
                                if (d >= 0.0f) {
                                    const uint32_t pos = atomicAdd(wcount_s, 1u);
                                    if (pos < filt.wave_cap)
                                        wave_list[pos] = make_uint4(topk_ordered_bits(sc, LARGEST), (uint32_t)row, q0 + ql + e, 0u);
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (FILTER && lane == 0) filt.wave_counts[filt.wave_base + blockIdx.x * 8 + wave] = *wcount_s;
}

// ------------------------------------------------------------------------------------------
// Many queries on the FP4 matrix cores (round 3).  popcount(q AND v) is a dot product of 0/1 values, and 0 and 1 are
// exact in every MFMA input format: as E2M1 nibbles (0b0010 = 1.0) through v_mfma_scale_f32_16x16x128_f8f6f4 (both
// scales 2^0) a k-step covers 128 BITS per instruction and the part runs it at 8.85 POP/s and 2.35 GHz in a bare loop
// (the int8 instructions: 3.6-4.4 POP/s at 1.85-2.2 GHz); the f32 accumulators hold the exact counts (< 2^24).  What made
// bin_gemm_rs_kernel vector-ALU-bound was expanding every row's bits once per 64-query tile in every wave; here the
// structure is u8_gemm_qs16_kernel's (csrc/u8_batch.hip): a workgroup expands a block of 128 rows ONCE into LDS
// (nibbles: 4 x the row bytes, pitch = whole 256-byte bank rows, 16-byte chunks XOR (row & 15)) and streams the whole
// batch past it - up to 2048 queries per launch, their nibble image prepared once per call in fragment order
// (bin_frag4_kernel: per 16 queries and 128-bit k-step one 1 KiB piece, lane (i, g) = bits [128 s + 32 g, +32) of query
// i).  Same epilogue arithmetic as bin_gemm_rs_kernel: the scores are the reference's bit for bit.  Rows of 512 / 768 / 1024 /
// 1536 bits.
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

// 32 bits -> 32 E2M1 nibbles (1.0 = 0b0010 where set).  Rows and queries go through the same function and a k-step sums
// over all 32 places of a dword's chunk, so ANY fixed placement of the bits inside the chunk does: dword p of the result
// holds bit pairs p of the four bytes (bits 2 p, 2 p + 1 of byte j at nibbles 2 j, 2 j + 1).  Per output dword one shift,
// one mask - four byte-sized selectors 0..3 - and one v_perm_b32 that looks each selector up in the four-byte table
// {0x00, 0x02, 0x20, 0x22}: 11 vector-ALU operations per 32 bits.  (Round 3 spread every nibble of every byte with 24-bit
// multiplies: ~38 operations, 1.1 us of the 3.3 us a 128-row block cost.)
__device__ __forceinline__ uint4 nib32(uint32_t w) {
    constexpr uint32_t kPairs = 0x03030303u, kTable = 0x22200200u;
    return make_uint4(__builtin_amdgcn_perm(0u, kTable, w & kPairs), __builtin_amdgcn_perm(0u, kTable, (w >> 2) & kPairs),
                      __builtin_amdgcn_perm(0u, kTable, (w >> 4) & kPairs), __builtin_amdgcn_perm(0u, kTable, (w >> 6) & kPairs));
}

// out[(t16 * nsteps + s) * 64 + lane] = nibbles of bits [128 s + 32 g, +32) of query 16 t16 + i (lane = 16 g + i); also the
// query's offset and, given its pivot, the integer bound of the pre-filter (as bin_gemm_rs_kernel computes them per tile)
template <bool LOW>
__global__ __launch_bounds__(256) void bin_frag4_kernel(const uint8_t *__restrict__ qbits, uint32_t q_stride, uint32_t n_queries,
                                                       uint32_t q_pad, uint32_t nsteps, float dim_f, int zx, int largest,
                                                       const float *__restrict__ pivots, uint4 *__restrict__ out,
                                                       float *__restrict__ q_off, int *__restrict__ bq) {
    const uint64_t total = (uint64_t)(q_pad / 16) * nsteps * 64;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256) {
        const uint32_t lane = (uint32_t)(idx & 63u);
        const uint64_t ts = idx >> 6;
        const uint32_t sx = (uint32_t)(ts % nsteps), t16 = (uint32_t)(ts / nsteps);
        const uint32_t q = 16u * t16 + (lane & 15u), g = lane >> 4;
        uint32_t w = 0;
        if (q < n_queries) w = *reinterpret_cast<const uint32_t *>(qbits + (uint64_t)q * q_stride + 16u * sx + 4u * g);
        out[idx] = nib32(w);
    }
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < q_pad) {
        uint32_t pq = 0;
        if (q < n_queries)
            for (uint32_t w = 0; w < nsteps * 4; w++) pq += __popc(*reinterpret_cast<const uint32_t *>(qbits + (uint64_t)q * q_stride + w * 4));
        const float qo = zx ? dim_f - 2.0f * (float)pq : 2.0f * (float)pq - dim_f;
        const float multiplier = zx ? 4.0f : -4.0f;
        const bool lg = largest != 0;
        const float pv = q < n_queries ? pivots[q] : (lg ? __builtin_huge_valf() : -__builtin_huge_valf());
        int b = pp_bound<LOW>(pv - qo, fabsf(pv) + fabsf(qo), multiplier, 1);
        if (__builtin_isinf(pv)) b = ((pv > 0.0f) == lg) == LOW ? -(int)kPpLim : (int)kPpLim;
        q_off[q] = qo;
        bq[q] = b;
    }
}

// IT: 16-query tiles per wave and chunk - 4 (64 queries), 2 for batches of up to 256 queries, 1 up to 128 (a chunk for every wave)
// JT: 16-row tiles per block - 8 (128 rows; rows of up to 1024 bits), 6 (96 rows of 1536 bits: two 72 KiB slabs)
template <int MODE, bool LOW, int IT, int JT>  // MODE 1 / 2: filter for the largest / smallest scores
__global__ __launch_bounds__(512) void bin_gemm_qs4_kernel(const uint8_t *__restrict__ rows, uint32_t ds,
                                                          const uint4 *__restrict__ qfrag, const float *__restrict__ q_offsets,
                                                          const int *__restrict__ bq_all, int zx, uint32_t n_rows,
                                                          uint32_t n_queries, BatchFilter filt) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[];
    constexpr int JH = JT / 2, QS_ROWS = 16 * JT, CQ = 16 * IT, MAXSTEPS = JT == 8 ? 8 : 12;
    constexpr bool LARGEST = MODE == 1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t i16 = (uint32_t)lane & 15u, g4 = (uint32_t)lane >> 4;
    const uint32_t nsteps = __builtin_amdgcn_readfirstlane(ds / 16);  // k-steps of 128 bits
    const uint32_t PA = ((ds * 4 + 255) / 256) * 256;                 // LDS pitch of a row's nibble image: whole 256-byte bank rows
                                                                      // (768-bit rows: 384 bytes of nibbles on a 512-byte pitch; the
                                                                      // places past the image are only multiplied with zero nibbles)
    const float multiplier = zx ? 4.0f : -4.0f;
    const uint32_t n_blocks = (n_rows + QS_ROWS - 1) / QS_ROWS;
    const uint32_t live_chunks = (n_queries + CQ - 1) / CQ;
    // TWO row blocks in LDS (a block of 128 rows is only 16 KiB of bits: the cost of changing blocks is latency, and with a
    // single slab it was 3.9 us per block whatever the batch): the next block's bits are requested into 8 registers when
    // this block starts, expanded into the other slab when this block's chunks are done - one barrier per block
    const uint32_t SLAB = QS_ROWS * PA;
    float *voff_s = reinterpret_cast<float *>(lds_raw + 2 * (size_t)SLAB);  // [2][128]
    int *br_s = reinterpret_cast<int *>(voff_s + 2 * QS_ROWS);              // [2][128]
    uint32_t *wcount_s = reinterpret_cast<uint32_t *>(br_s + 2 * QS_ROWS) + wave;
    int *bq_s = reinterpret_cast<int *>(br_s + 2 * QS_ROWS) + 16;           // [CQ * live_chunks]
    // (expanding through a 256-entry byte -> nibbles table in LDS instead of the multiplies was measured: no faster)
    if (lane == 0) *wcount_s = 0;
    // the "always" / "never" sentinels of the bounds (+-2^29) are brought to +-2^23: still far beyond any count, and the
    // accumulators (count - bound, f32) stay exact integers
    for (uint32_t i = t; i < CQ * live_chunks; i += 512) bq_s[i] = max(min(bq_all[i], 1 << 23), -(1 << 23));

    v4i Q0[IT], Q1[IT], Q2[IT];
    auto load_step = [&](v4i(&a)[IT], uint32_t c, uint32_t j) {
        const uint4 *p = qfrag + ((uint64_t)(IT * c) * nsteps + j) * 64 + lane;
#pragma unroll
        for (int it = 0; it < IT; it++) {
            const uint4 v = p[(uint64_t)it * nsteps * 64];
            a[it] = v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
    };
    // Small batches (IT < 4: at most one chunk per wave): the wave's query fragments for all (at most 8) k-steps stay in
    // registers for the whole launch.  Streamed, a chunk of 16 or 32 queries is 8 short k-steps behind an L2 round trip
    // each - a 4 us floor per row block whatever the batch.
    constexpr bool QREG = IT < 4;
    v4i Qr[QREG ? MAXSTEPS : 1][IT];
    if (QREG) {
#pragma unroll
        for (int j = 0; j < MAXSTEPS; j++)
#pragma unroll
            for (int it = 0; it < IT; it++) Qr[j][it] = v4i{0, 0, 0, 0};
        if ((uint32_t)wave < live_chunks) {
#pragma unroll
            for (int j = 0; j < MAXSTEPS; j++)
                if ((uint32_t)j < nsteps) load_step(Qr[j], (uint32_t)wave, (uint32_t)j);
        }
    }
    const uint32_t b_row = i16 * PA, b_gi = (g4 ^ i16) * 16u;
    // Row-block fill: the block is 128 * ds contiguous bytes of the store; thread t takes the 16-byte (128-bit) pieces
    // t, t + 512, ... (ds / 16 * 128 / 512 = ds / 64 of them: 2 at 1024 bits), requested before the barrier that frees the
    // LDS rows, expanded and written after it: piece pc of row r = nibble chunks 4 pc .. 4 pc + 3, each at place
    // chunk ^ (r & 15).  The row's popcount (its offset in the score) is the sum over its ds / 16 pieces, which sit in
    // adjacent lanes.
    const uint32_t per = ds / 16;                        // 128-bit pieces per row: 4, 6, 8 or 12
    const uint32_t sper = per <= 4 ? 4u : per <= 8 ? 8u : 16u;  // lanes per row (a power of two: the row's popcount is a butterfly sum)
    const uint32_t n_pieces = __builtin_amdgcn_readfirstlane(QS_ROWS * sper / 512);  // rounds: rows * sper lanes / 512 threads
    constexpr int MAXP = JT == 8 ? 2 : 3;  // 128 rows x 8 lanes / 512; 96 x 16 / 512
    // TWO register sets: a block's bits are requested one block before they are expanded.  `vmcnt` retires in order and
    // the K loop waits for its query fragments at every k-step, so a request in front of a K loop stalls it for an HBM
    // round trip (measured: a 3.9 us floor per block); the request is placed behind the last query loads of the wave's
    // last chunk instead, and the data is not needed before the END of the following block.
    // (Round 4: up to FOUR register sets, the request four blocks ahead.  With two, a workgroup had at most two 16 KiB blocks in
    // flight - 32 KiB per CU against the ~64 KiB that 8 TB/s x ~2 us of HBM latency ask for: a launch with the K loop cut
    // out still took 3.2 ms for the 6.4 GB of a 50M x 1024-bit store, 2 TB/s, and that was the floor of every small batch.)
    // The streamed-query forms (IT = 4) and the 96-row form with IT = 2 sit at the 256-register limit and keep two sets:
    // their blocks last long enough (MFMA-bound) for one block of look-ahead.
    constexpr int DEPTH = (IT == 4 || (IT == 2 && JT == 6)) ? 2 : 4;
    uint4 st[DEPTH][MAXP];
    auto fill_request = [&](uint4(&st)[MAXP], uint32_t blk) {
        const uint8_t *p = rows + (uint64_t)blk * QS_ROWS * ds;
#pragma unroll
        for (int i = 0; i < MAXP; i++) {
            const uint32_t ii = (uint32_t)i < n_pieces ? (uint32_t)i : n_pieces - 1;  // wave-uniform
            const uint32_t slot = (uint32_t)t + 512u * ii, row = slot / sper, pc = slot % sper;
            st[i] = pc < per ? ld_nt(reinterpret_cast<const uint4 *>(p + (size_t)row * ds + (size_t)pc * 16)) : make_uint4(0, 0, 0, 0);
        }
    };
    auto fill_write = [&](const uint4(&st)[MAXP], uint64_t row0, uint32_t par) {
        uint8_t *slab = lds_raw + par * SLAB;
#pragma unroll
        for (int i = 0; i < MAXP; i++) {
            if ((uint32_t)i >= n_pieces) break;
            const uint32_t slot = (uint32_t)t + 512u * i, row = slot / sper, pc = slot % sper;
            const uint32_t w[4] = {st[i].x, st[i].y, st[i].z, st[i].w};
            if (pc < per) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t chunk = 4u * pc + k;
                    *reinterpret_cast<uint4 *>(slab + row * PA + ((chunk ^ (row & 15u)) * 16u)) = nib32(w[k]);
                }
            }
            // popcount of the row: pieces of a row are in `per` adjacent lanes of this round (per divides 64)
            uint32_t pop = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
            for (uint32_t d = 1; d < sper; d <<= 1) pop += (uint32_t)__shfl_xor((int)pop, (int)d);  // (lanes past the row's pieces hold zeros)
            if (pc == 0) {
                const bool ok = row0 + row < n_rows;
                const float v_off = zx ? -2.0f * (float)pop : 2.0f * (float)pop;
                voff_s[par * QS_ROWS + row] = v_off;
                br_s[par * QS_ROWS + row] = ok ? pp_bound<LOW>(-v_off, fabsf(v_off), multiplier, 0) : (LOW ? -(int)kPpLim : (int)kPpLim);
            }
        }
    };
    const uint32_t my_first = wave;
    const uint32_t first_blk = blockIdx.x < n_blocks ? blockIdx.x : 0u;
    auto clamp_blk = [&](uint32_t blk) { return blk < n_blocks ? blk : first_blk; };  // past the end: a harmless re-read
    // set (i mod DEPTH) holds the bits of the workgroup's i-th block from its request until they are expanded
#pragma unroll
    for (int d = 0; d < DEPTH; d++) fill_request(st[d], clamp_blk(first_blk + (uint32_t)d * gridDim.x));
    fill_write(st[0], (uint64_t)first_blk * QS_ROWS, 0u);
    if (!QREG && my_first < live_chunks) {
        load_step(Q0, my_first, 0);
        load_step(Q1, my_first, 1);
    }
    __syncthreads();
    uint4 *wave_list = filt.wave_cand + (uint64_t)(filt.wave_base + blockIdx.x * 8 + wave) * filt.wave_cap;

    // one row block: slab `par` holds it, st_use the next block's bits (requested three blocks ago), st_req takes the bits of
    // the block after that
    auto block_body = [&](uint32_t blk, uint32_t par, const uint4(&st_use)[MAXP], uint4(&st_req)[MAXP]) {
        const uint64_t row0 = (uint64_t)blk * QS_ROWS;
        const uint32_t next_blk = clamp_blk(blk + gridDim.x), next2_blk = clamp_blk(blk + (uint32_t)DEPTH * gridDim.x);
        bool requested = false;
        const uint8_t *slab = lds_raw + par * SLAB;
        const float *voff_cur = voff_s + par * QS_ROWS;
        const int *br_cur = br_s + par * QS_ROWS;
        for (uint32_t c = wave; c < live_chunks; c += 8) {
            const uint32_t c_next = c + 8 < live_chunks ? c + 8 : my_first;
            v4f_t acc[IT][JT];
#pragma unroll
            for (int it = 0; it < IT; it++) {
                const v4i bq4 = *reinterpret_cast<const v4i *>(bq_s + CQ * c + 16 * it + 4 * g4);
#pragma unroll
                for (int jt = 0; jt < JT; jt++)
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[it][jt][e] = -(float)bq4[e];  // |bound| <= dim or the 2^29 sentinel: exact
            }
            auto compute = [&](const v4i(&a)[IT], uint32_t j) {
                uint32_t lane_addr = b_row + (b_gi ^ ((j & 3u) * 64u)) + (j >> 2) * 256u;
                asm volatile("" : "+v"(lane_addr));
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    v4i bf[JH];
#pragma unroll
                    for (int j4 = 0; j4 < JH; j4++)
                        bf[j4] = *reinterpret_cast<const v4i *>(slab + lane_addr + (uint32_t)(JH * hf + j4) * 16u * PA);
#pragma unroll
                    for (int it = 0; it < IT; it++) {
                        const v8i_t a8 = {a[it].x, a[it].y, a[it].z, a[it].w, 0, 0, 0, 0};
#pragma unroll
                        for (int j4 = 0; j4 < JH; j4++) {
                            const v8i_t b8 = {bf[j4].x, bf[j4].y, bf[j4].z, bf[j4].w, 0, 0, 0, 0};
                            acc[it][JH * hf + j4] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, acc[it][JH * hf + j4], 4, 4, 0, 127, 0, 127);
                        }
                    }
                }
            };
            auto request = [&](v4i(&a)[IT], uint32_t j) {
                if (j < nsteps) load_step(a, c, j);
                else load_step(a, c_next, j - nsteps);
            };
            if (((c >> 3) + ((uint32_t)wave >> 2)) & 1u) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(0);
            uint32_t j = 0;
            if (QREG) {
#pragma unroll
                for (int jj = 0; jj < MAXSTEPS; jj++)
                    if ((uint32_t)jj < nsteps) compute(Qr[jj], (uint32_t)jj);
                j = nsteps;
            }
            for (; !QREG && j + 2 < nsteps; j += 3) {
                request(Q2, j + 2);
                __builtin_amdgcn_sched_barrier(0);
                compute(Q0, j);
                __builtin_amdgcn_sched_barrier(0);
                request(Q0, j + 3);
                __builtin_amdgcn_sched_barrier(0);
                compute(Q1, j + 1);
                __builtin_amdgcn_sched_barrier(0);
                request(Q1, j + 4);
                __builtin_amdgcn_sched_barrier(0);
                compute(Q2, j + 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t left = QREG ? 0u : nsteps - j;
            if (left >= 1) {
                request(Q2, j + 2);
                __builtin_amdgcn_sched_barrier(0);
                compute(Q0, j);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (left == 2) {
                request(Q0, j + 3);
                __builtin_amdgcn_sched_barrier(0);
                compute(Q1, j + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            if (c + 8 >= live_chunks) {  // this wave's last chunk of the block: no wait for younger loads follows before the block ends
                fill_request(st_req, next2_blk);
                requested = true;
            }
            // ---- epilogue: lane (i16, g4) holds, per (it, jt), queries CQ c + 16 it + 4 g4 + e against row 16 jt + i16
            uint32_t c_e = c, lane_e = (uint32_t)lane;
            asm volatile("" : "+s"(c_e), "+v"(lane_e));
            const uint32_t i_e = lane_e & 15u, g_e = lane_e >> 4;
            // "some accumulator may pass": acc = count - query bound; the row bound decides (as in bin_gemm_rs_kernel)
            bool any_lane = false;
#pragma unroll
            for (int jt = 0; jt < JT; jt++) {
                const float brf = (float)br_cur[jt * 16 + i_e];
                float ext = acc[0][jt][0];
#pragma unroll
                for (int it = 0; it < IT; it++)
#pragma unroll
                    for (int e = 0; e < 4; e++) ext = LOW ? fminf(ext, acc[it][jt][e]) : fmaxf(ext, acc[it][jt][e]);
                any_lane |= LOW ? ext < brf : ext >= brf;
            }
            if (__builtin_amdgcn_readfirstlane(__ballot(any_lane) != 0)) {
#pragma unroll
                for (int jt = 0; jt < JT; jt++) {
                    __builtin_amdgcn_sched_barrier(0);
                    const uint64_t row = row0 + jt * 16 + i_e;
                    const int br = br_cur[jt * 16 + i_e];
                    const float v_off = voff_cur[jt * 16 + i_e];
#pragma unroll
                    for (int it = 0; it < IT; it++) {
                        const uint32_t q = CQ * c_e + 16 * it + 4 * g_e;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int av = (int)acc[it][jt][e];
                            if (LOW ? av < br : av >= br) {  // may pass: the exact f32 comparison decides
                                const float qo = q_offsets[q + e];
                                const float pvt = filt.pivot_scores[q + e];
                                const float sc = (multiplier * (float)(av + bq_s[q + e]) + qo) + v_off;
                                const float d = LARGEST ? sc - pvt : pvt - sc;
                                if (d >= 0.0f) {
                                    const uint32_t pos = atomicAdd(wcount_s, 1u);
                                    if (pos < filt.wave_cap)
                                        wave_list[pos] = make_uint4(topk_ordered_bits(sc, LARGEST), (uint32_t)row, filt.query_base + q + e, 0u);
                                }
                            }
                        }
                    }
                }
            }
            if (left == 1) {
#pragma unroll
                for (int it = 0; it < IT; it++) {
                    Q0[it] = Q1[it];
                    Q1[it] = Q2[it];
                }
            } else if (left == 2) {
#pragma unroll
                for (int it = 0; it < IT; it++) {
                    const v4i k1 = Q0[it];
                    Q0[it] = Q2[it];
                    Q1[it] = k1;
                }
            }
        }
        if (!requested) fill_request(st_req, next2_blk);  // a wave without chunks
        fill_write(st_use, (uint64_t)next_blk * QS_ROWS, par ^ 1u);  // the other slab: last read a block ago, a barrier has passed since
        __syncthreads();
    };
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += 4 * gridDim.x) {  // block i: expands set (i + 1) mod DEPTH, refills set i mod DEPTH
        block_body(blk, 0u, st[1 % DEPTH], st[0]);
        if (blk + gridDim.x >= n_blocks) break;
        block_body(blk + gridDim.x, 1u, st[2 % DEPTH], st[1 % DEPTH]);
        if (blk + 2 * gridDim.x >= n_blocks) break;
        block_body(blk + 2 * gridDim.x, 0u, st[3 % DEPTH], st[2 % DEPTH]);
        if (blk + 3 * gridDim.x >= n_blocks) break;
        block_body(blk + 3 * gridDim.x, 1u, st[0], st[3 % DEPTH]);
    }
    if (lane == 0) filt.wave_counts[filt.wave_base + blockIdx.x * 8 + wave] = *wcount_s;
}

// ------------------------------------------------------------------------------------------
// FP4 matrix cores, ROW-STREAMING form (round 4): batches whose whole nibble image fits in LDS - 256 queries of 1024 bits
// are 128 KiB.  bin_gemm_qs4_kernel keeps ROWS in LDS and pays per 128-row block an expansion phase, an epilogue phase and
// a barrier during which the matrix pipes idle (timeline, profiles/r04_bin_batch.txt: at 256 queries the K loop is 35 % of
// a block, at 128 queries less; no amount of look-ahead on the row loads moved it).  Here the roles are swapped, as in
// bin_gemm_rs_kernel / u8_gemm_rs_kernel: the QUERIES are resident (fragment order: the A operand of k-step s of a
// 16-query tile is one lane-linear 1 KiB piece, conflict-free by construction), every wave streams its OWN rows - 32 per
// trip, loaded two trips ahead, expanded to nibbles ONCE per row into 64 registers, then multiplied with every query tile -
// and after the set-up there is no barrier: each SIMD's two waves drift apart and fill each other's vector-ALU phases with
// MFMAs.  A lane owns NS consecutive dwords of its row (lane (i, g): dwords [NS g, NS g + NS) of row i: whole 16-byte
// loads, every line fetched once); k-step s multiplies dword NS g + s of the row with the same dword of the query, which is
// where the staging copy puts it (any pairing of K positions is the same dot product).  Arithmetic, bounds and candidate
// lists are bin_gemm_qs4_kernel's.
// (its batch sizes, passes and waves per workgroup: bin_batch_route.hpp)
template <int MODE, bool LOW, int NS>  // MODE 1 / 2: filter for the largest / smallest scores; NS = k-steps = ds / 16
__global__ __launch_bounds__(64 * rs4_waves(NS)) void bin_gemm_rs4_kernel(const uint8_t *__restrict__ rows, const uint4 *__restrict__ qfrag,
                                                          const float *__restrict__ q_offsets, const int *__restrict__ bq_all,
                                                          int zx, uint32_t n_rows, uint32_t n_tiles /* even */, BatchFilter filt) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[];
    constexpr int RT = 2, QP = 2, DS = 16 * NS, WAVES = rs4_waves(NS), THREADS = 64 * WAVES;
    constexpr bool LARGEST = MODE == 1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t i16 = (uint32_t)lane & 15u, g4 = (uint32_t)lane >> 4;
    const float multiplier = zx ? 4.0f : -4.0f;
    uint4 *img = reinterpret_cast<uint4 *>(lds_raw);                                      // [n_tiles][NS][64] x 16 B
    float *nbq_s = reinterpret_cast<float *>(lds_raw + (size_t)n_tiles * NS * 1024);      // [16 n_tiles]: MINUS the query bounds
    uint32_t *wcount_s = reinterpret_cast<uint32_t *>(nbq_s + 16 * n_tiles) + wave;
    if (lane == 0) *wcount_s = 0;
    for (uint32_t idx = t; idx < n_tiles * NS * 64; idx += THREADS) {  // position (tile, s, lane (i, g)) <- the query's dword NS g + s
        const uint32_t tile = idx / (NS * 64), rem = idx % (NS * 64), sx = rem >> 6, i = rem & 15u, g = (rem >> 4) & 3u;
        const uint32_t d = NS * g + sx;
        img[idx] = qfrag[((uint64_t)tile * NS + d / 4) * 64 + 16 * (d % 4) + i];
    }
    // (the "always" / "never" sentinels of the bounds, +-2^29, are brought to +-2^23: far beyond any count, and exact in f32)
    // stored negated and as f32: a tile's accumulators START at -bound, and the first MFMA of a chain takes these four
    // values as its C operand straight from the LDS read - no conversion, no copy per tile
    for (uint32_t i = t; i < 16 * n_tiles; i += THREADS) nbq_s[i] = -(float)max(min(bq_all[i], 1 << 23), -(1 << 23));
    __syncthreads();

    const uint32_t n_chunks = (n_rows + 16 * RT - 1) / (16 * RT), stride = gridDim.x * WAVES;
    uint32_t raw[RT][NS], raw2[RT][NS];  // the rows of this trip and of the next; the trip after that is requested into `raw`
                                         // as soon as it has been expanded (two trips = 8 KiB per wave in flight)
    auto load_rows = [&](uint32_t (&raw)[RT][NS], uint32_t chunk) {  // rows past the store are its zero padding
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            const uint8_t *p = rows + ((uint64_t)chunk * (16 * RT) + rt * 16 + i16) * DS + 4 * NS * g4;
            if (NS % 4 == 0) {
#pragma unroll
                for (int v = 0; v < NS / 4; v++) {
                    const uint4 x = reinterpret_cast<const uint4 *>(p)[v];
                    raw[rt][4 * v] = x.x, raw[rt][4 * v + 1] = x.y, raw[rt][4 * v + 2] = x.z, raw[rt][4 * v + 3] = x.w;
                }
            } else {
#pragma unroll
                for (int v = 0; v < NS / 2; v++) {
                    const uint2 x = reinterpret_cast<const uint2 *>(p)[v];
                    raw[rt][2 * v] = x.x, raw[rt][2 * v + 1] = x.y;
                }
            }
        }
    };
    uint4 *wave_list = filt.wave_cand + (uint64_t)(filt.wave_base + blockIdx.x * WAVES + wave) * filt.wave_cap;
    const uint32_t first = blockIdx.x * WAVES + wave;
    auto clamp_chunk = [&](uint32_t c) { return c < n_chunks ? c : (first < n_chunks ? first : 0u); };  // past the end: a harmless re-read
    load_rows(raw, clamp_chunk(first));
    load_rows(raw2, clamp_chunk(first + stride));
    auto trip = [&](uint32_t chunk, uint32_t (&raw)[RT][NS]) {
        v8i_t B[RT][NS];
        uint32_t pop[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            pop[rt] = 0;
#pragma unroll
            for (int sx = 0; sx < NS; sx++) {
                const uint4 nb = nib32(raw[rt][sx]);
                B[rt][sx] = v8i_t{(int)nb.x, (int)nb.y, (int)nb.z, (int)nb.w, 0, 0, 0, 0};
                pop[rt] += __popc(raw[rt][sx]);
            }
        }
        const uint64_t row0 = (uint64_t)chunk * (16 * RT);
        load_rows(raw, clamp_chunk(chunk + 2 * stride));  // two trips ahead, behind this trip's MFMAs
        float v_off[RT], brf[RT];
        int br[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {  // the row's popcount: its four lanes (i, 0..3)
            uint32_t pv = pop[rt] + (uint32_t)__shfl_xor((int)pop[rt], 16);
            pv += (uint32_t)__shfl_xor((int)pv, 32);
            v_off[rt] = zx ? -2.0f * (float)pv : 2.0f * (float)pv;
            const bool ok = row0 + rt * 16 + i16 < n_rows;
            br[rt] = ok ? pp_bound<LOW>(-v_off[rt], fabsf(v_off[rt]), multiplier, 0) : (LOW ? -(int)kPpLim : (int)kPpLim);
            brf[rt] = (float)br[rt];
        }
        for (uint32_t qt = 0; qt < n_tiles; qt += QP) {
            v4f_t acc[QP][RT];
            const uint4 *a_base = img + (size_t)qt * NS * 64 + lane;
#pragma unroll
            for (int sx = 0; sx < NS; sx++) {
#pragma unroll
                for (int qp = 0; qp < QP; qp++) {
                    const uint4 a = a_base[(qp * NS + sx) * 64];
                    const v8i_t a8 = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
                    const v4f_t start = *reinterpret_cast<const v4f_t *>(nbq_s + 16 * (qt + qp) + 4 * g4);  // (used at sx == 0 only)
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
                        acc[qp][rt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, B[rt][sx], sx == 0 ? start : acc[qp][rt], 4, 4, 0, 127, 0, 127);
                }
            }
            // ---- epilogue: lane (i, g) holds queries 16 (qt + qp) + 4 g + e against row 16 rt + i of the trip
            bool any_lane = false;
#pragma unroll
            for (int qp = 0; qp < QP; qp++)
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    const float ext = LOW ? fminf(fminf(acc[qp][rt][0], acc[qp][rt][1]), fminf(acc[qp][rt][2], acc[qp][rt][3]))
                                          : fmaxf(fmaxf(acc[qp][rt][0], acc[qp][rt][1]), fmaxf(acc[qp][rt][2], acc[qp][rt][3]));
                    any_lane |= LOW ? ext < brf[rt] : ext >= brf[rt];
                }
            if (__builtin_amdgcn_readfirstlane(__ballot(any_lane) != 0)) {
#pragma unroll
                for (int qp = 0; qp < QP; qp++)
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        const uint32_t q = 16 * (qt + qp) + 4 * g4;
                        const uint64_t row = row0 + rt * 16 + i16;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int av = (int)acc[qp][rt][e];
                            if (LOW ? av < br[rt] : av >= br[rt]) {  // may pass: the exact f32 comparison decides
                                const float qo = q_offsets[q + e];
                                const float pvt = filt.pivot_scores[q + e];
                                const float sc = (multiplier * (float)(av - (int)nbq_s[q + e]) + qo) + v_off[rt];
                                const float d = LARGEST ? sc - pvt : pvt - sc;
                                if (d >= 0.0f) {
                                    const uint32_t pos = atomicAdd(wcount_s, 1u);
                                    if (pos < filt.wave_cap)
                                        wave_list[pos] = make_uint4(topk_ordered_bits(sc, LARGEST), (uint32_t)row, filt.query_base + q + e, 0u);
                                }
                            }
                        }
                    }
            }
        }
    };
    for (uint32_t chunk = first; chunk < n_chunks; chunk += 2 * stride) {
        trip(chunk, raw);
        if (chunk + stride >= n_chunks) break;
        trip(chunk + stride, raw2);
    }
    if (lane == 0) filt.wave_counts[filt.wave_base + blockIdx.x * WAVES + wave] = *wcount_s;
}

// Sample rows for the pivots (rows only; the golden-ratio scatter of topk.hip), then `pad` zero rows.
__global__ __launch_bounds__(256) void bin_gather_rows_kernel(const uint4 *__restrict__ rows, uint32_t row_chunks, uint64_t n_rows,
                                                             uint32_t n, uint32_t pad, uint4 *__restrict__ out) {
    const uint64_t total = (uint64_t)(n + pad) * row_chunks;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = (uint32_t)(i / row_chunks), c = (uint32_t)(i % row_chunks);
        if (j >= n) {
            out[i] = make_uint4(0, 0, 0, 0);
            continue;
        }
        const unsigned long long hsh = (unsigned long long)j * 0x9E3779B97F4A7C15ull;
        const uint64_t src = ((hsh >> 32) * n_rows) >> 32;
        out[i] = rows[src * row_chunks + c];
    }
}

}  // namespace


namespace {

// The developer switches of the batch route, read once per process (tools/lib build; all-default in the product library).
const BinBatchSwitches &bin_batch_switches() {
    static const BinBatchSwitches switches = [] {
        auto number = [](const char *name) {
            const char *e = dev_env(name);
            return BinBatchSwitches::Number{e != nullptr, e ? (uint64_t)atoll(e) : 0};
        };
        auto is_off = [](const char *name) {
            const char *e = dev_env(name);
            return e && e[0] == '0';
        };
        BinBatchSwitches d;
        d.fp4 = !is_off("QAMD_BIN4");
        d.fp4_min = number("QAMD_BIN4_MIN");
        d.rs4 = !is_off("QAMD_BIN_RS4");
        if (const char *e = dev_env("QAMD_BIN_RS4_PASSES")) d.rs4_passes = {true, (uint32_t)atoi(e)};
        d.mfma_min = number("QAMD_BIN_MFMA_MIN");
        d.scalar_mfma_min = dev_env_u64("QAMD_BIN_SCALAR_MFMA_MIN", 0);
        return d;
    }();
    return switches;
}

// The route (bin_batch_route.hpp) of score_batch (k = 0) or topk_batch(k) for this store and batch.
BinBatchRoute bin_route(const qamd_bin *h, const qamd_bin_query_batch *b, uint32_t k) {
    BinBatchInputs in;
    in.ds = h->ds;
    in.code_bits = h->code_bits;
    in.count = h->count;
    in.n_queries = b->n_queries;
    in.qbits = b->qbits;
    in.k = k;
    in.waves_per_launch = pp_waves_per_launch();
    return bin_batch_route(in, bin_batch_switches());
}

inline bool bin_zx(const qamd_bin *h) { return (h->vp.distance_type == QAMD_DOT) != (h->vp.invert != 0); }  // multiplier = zx ? +4 : -4
inline uint32_t bin_persistent_grid() { return (uint32_t)std::max(1, device_info().cu_count / 8) * 8; }

// One launch of bin_gemm_rs_kernel: rows [0, n_rows) against the tile of 32 * mi queries that starts at query q0.
// MODE 0: scores out; 1 / 2: filter for the largest / smallest.
struct BinRsCall {
    const qamd_bin *h;
    const qamd_bin_query_batch *b;
    const uint8_t *rows;
    uint64_t n_rows;
    uint32_t q0;
    int mi;
    float *out;
    uint64_t out_pitch;
    BatchFilter filt;
    hipStream_t s;
};
template <int MODE, bool LOW, int MI, bool CODES>
qamd_status launch_bin_rs_as(const BinRsCall &c) {
    const qamd_bin *h = c.h;
    const qamd_bin_query_batch *b = c.b;
    const size_t lds = (size_t)32 * c.mi * ((h->ds / 16) * 128 + 16) + 3 * 64 * 4 + 64;
    QAMD_LDS_OPT_IN((&bin_gemm_rs_kernel<MODE, LOW, MI, CODES>), 160 * 1024);
    // a binary batch: its bit rows (the one plane); a scalar batch: its code image at the kernel's own LDS pitch, and
    // dim * L for dim (never its planes, never as bits)
    hipLaunchKernelGGL((bin_gemm_rs_kernel<MODE, LOW, MI, CODES>), dim3(bin_persistent_grid()), dim3(512), lds, c.s, c.rows,
                       (uint32_t)h->ds, CODES ? b->codes.as<uint8_t>() : b->planes.as<uint8_t>(),
                       (uint32_t)(CODES ? b->code_pitch : b->p_stride), metric_dim(h, b->qbits), bin_zx(h) ? 1 : 0, (uint32_t)c.n_rows,
                       (uint32_t)b->n_queries, c.q0, c.out, c.out_pitch, c.filt);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}
template <int MODE>
qamd_status launch_bin_rs(const BinRsCall &c) {
    const bool codes = c.b->qbits != 1;
    if (codes) {
        if (c.b->code_pitch != (c.h->ds / 16) * 128 + 16) return fail(QAMD_ERR_ARGUMENTS, "the batch's code image has another pitch");
        // The filter runs on 32-query tiles only (bin_batch_route): the 64-query filter forms need 20 bytes of scratch
        // per lane at 256 registers - the binary ones have since they were written - and are not instantiated for codes.
        if (MODE != 0 && c.mi != 1) return fail(QAMD_ERR_ARGUMENTS, "scalar batches filter on 32-query tiles");
    }
    return with_low<MODE>(bin_zx(c.h) ? 4.0f : -4.0f, [&](auto low) -> qamd_status {
        constexpr bool LOW = decltype(low)::value;
        if (codes) {
            if constexpr (MODE == 0) {
                if (c.mi == 2) return launch_bin_rs_as<MODE, LOW, 2, true>(c);
            }
            return launch_bin_rs_as<MODE, LOW, 1, true>(c);
        }
        if (c.mi == 2) return launch_bin_rs_as<MODE, LOW, 2, false>(c);
        return launch_bin_rs_as<MODE, LOW, 1, false>(c);
    });
}

// One launch of an FP4 filter kernel: the rows of the store against queries [q_base, q_base + nq) of the batch's nibble
// image (bin_frag4_kernel: fragments, offsets and integer bounds of every query).  MODE 1 / 2: largest / smallest.
struct BinFp4Call {
    const qamd_bin *h;
    const uint4 *frag;
    const float *q_off;
    const int *bq;
    uint64_t q_base;
    uint32_t nq;
    BatchFilter filt;
    hipStream_t s;
};
template <int MODE, bool LOW, int NS>
qamd_status launch_bin_rs4_as(const BinFp4Call &c) {
    const qamd_bin *h = c.h;
    const uint32_t n_tiles = (uint32_t)(round_up(c.nq, 32) / 16);
    const size_t lds = (size_t)n_tiles * h->ds * 64 + (size_t)n_tiles * 64 + 64;
    QAMD_LDS_OPT_IN((&bin_gemm_rs4_kernel<MODE, LOW, NS>), 160 * 1024);
    hipLaunchKernelGGL((bin_gemm_rs4_kernel<MODE, LOW, NS>), dim3(bin_persistent_grid()), dim3(64 * rs4_waves(NS)), lds, c.s,
                       h->rows.as<uint8_t>(), c.frag + (c.q_base / 16) * NS * 64, c.q_off + c.q_base, c.bq + c.q_base, bin_zx(h) ? 1 : 0,
                       (uint32_t)h->count, n_tiles, c.filt);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}
template <int MODE>
qamd_status launch_bin_rs4(const BinBatchRoute &rt, const BinFp4Call &c) {
    return with_low<MODE>(bin_zx(c.h) ? 4.0f : -4.0f, [&](auto low) -> qamd_status {
        constexpr bool LOW = decltype(low)::value;
        switch (rt.rs4_ns) {
            case 4: return launch_bin_rs4_as<MODE, LOW, 4>(c);
            case 6: return launch_bin_rs4_as<MODE, LOW, 6>(c);
            case 8: return launch_bin_rs4_as<MODE, LOW, 8>(c);
            case 12: return launch_bin_rs4_as<MODE, LOW, 12>(c);
        }
        return fail(QAMD_ERR_ARGUMENTS, "no %s for rows of %d k-steps", rt.name, rt.rs4_ns);
    });
}
template <int MODE, bool LOW, int IT, int JT>
qamd_status launch_bin_qs4_as(const BinFp4Call &c) {
    const qamd_bin *h = c.h;
    const size_t qs_rows = 16 * JT;
    const size_t lds = 2 * qs_rows * round_up(h->ds * 4, 256) + 4 * qs_rows * 4 + 64 + kQs4Slice * 4;
    QAMD_LDS_OPT_IN((&bin_gemm_qs4_kernel<MODE, LOW, IT, JT>), 160 * 1024);
    hipLaunchKernelGGL((bin_gemm_qs4_kernel<MODE, LOW, IT, JT>), dim3(bin_persistent_grid()), dim3(512), lds, c.s, h->rows.as<uint8_t>(),
                       (uint32_t)h->ds, c.frag + (c.q_base / 16) * (h->ds / 16) * 64, c.q_off + c.q_base, c.bq + c.q_base,
                       bin_zx(h) ? 1 : 0, (uint32_t)h->count, c.nq, c.filt);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}
template <int MODE>
qamd_status launch_bin_qs4(const BinBatchRoute &rt, const BinFp4Call &c) {
    return with_low<MODE>(bin_zx(c.h) ? 4.0f : -4.0f, [&](auto low) -> qamd_status {
        constexpr bool LOW = decltype(low)::value;
        switch (rt.qs4_it * 10 + rt.qs4_jt) {
            case 16: return launch_bin_qs4_as<MODE, LOW, 1, 6>(c);
            case 18: return launch_bin_qs4_as<MODE, LOW, 1, 8>(c);
            case 26: return launch_bin_qs4_as<MODE, LOW, 2, 6>(c);
            case 28: return launch_bin_qs4_as<MODE, LOW, 2, 8>(c);
            case 46: return launch_bin_qs4_as<MODE, LOW, 4, 6>(c);
            case 48: return launch_bin_qs4_as<MODE, LOW, 4, 8>(c);
        }
        return fail(QAMD_ERR_ARGUMENTS, "no %s of shape %d x %d", rt.name, rt.qs4_it, rt.qs4_jt);
    });
}

// The pivot sample of a store, gathered once per handle: every call uses a prefix (see sample_store in u8_batch.hip).
qamd_status bin_sample_rows(const qamd_bin *h, uint32_t rows_all, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->sample_mu);
    if (h->sample_count < rows_all) {
        DevBuf c;
        QAMD_TRY(c.alloc((uint64_t)(rows_all + 512) * h->ds));
        hipLaunchKernelGGL(bin_gather_rows_kernel, dim3(device_info().cu_count * 8), dim3(256), 0, s, h->rows.as<uint4>(),
                           (uint32_t)(h->ds / 16), h->count, rows_all, 512u, c.as<uint4>());
        QAMD_HIP(hipGetLastError());
        QAMD_HIP(hipStreamSynchronize(s));
        h->sample_rows = std::move(c);
        h->sample_count = rows_all;
    }
    return QAMD_OK;
}

// The batch on the matrix cores: per-query pivot from a cached row sample, the filtering pass of the route (`rt`, of
// this store, batch and k), candidates scattered to per-query lists, one emit.  status[q] != 0: query q must be redone
// by the exact path (its list over- or underflowed: heavy ties, an unlucky sample).
qamd_status bin_topk_batch_mfma(const qamd_bin *h, const qamd_bin_query_batch *b, const BinBatchRoute &rt, uint32_t k, int largest,
                                uint32_t *ids_dev, float *sc_dev, std::vector<uint32_t> &status, hipStream_t s) {
    const uint64_t Q = b->n_queries, n = h->count;
    const uint32_t TQ = 32u * (uint32_t)rt.mi;
    const uint64_t q_pad = round_up(Q, 64);
    const BatchSamplePlan plan = batch_sample_plan(n, Q, k);
    const uint32_t S = plan.S, r = plan.r;
    if (r > 64) {  // (tiny stores are not routed here)
        std::fill(status.begin(), status.end(), 1u);
        return QAMD_OK;
    }
    QAMD_TRY(bin_sample_rows(h, plan.rows_all, s));
    const double per_wave = 2.0 * plan.target * (double)rt.per_wave_queries / (double)pp_waves_per_launch();
    // (at least 1024 slots: queries of one batch can be near-duplicates, and then a passing row appends to every
    // query's list at once - 64 entries in one wave's list per such row)
    const uint32_t wave_cap = (uint32_t)std::min<double>(1u << 20, std::max<double>(1024.0, 16.0 * per_wave));
    BatchTopkPass pass(n, Q, q_pad, k, largest, rt.n_lists, wave_cap, s);
    const size_t o_scores = pass.reserve(Q * (uint64_t)S * 4);
    QAMD_TRY(pass.alloc());
    // sample scores of every query, then every query's pivot
    float *s_scores = pass.at<float>(o_scores);
    for (uint32_t q0 = 0; q0 < Q; q0 += TQ)
        QAMD_TRY(launch_bin_rs<0>({h, b, h->sample_rows.as<uint8_t>(), S, q0, rt.mi, s_scores, S, BatchFilter{}, s}));
    pass.pivots(s_scores, S, S, r);
    const BatchFilter f = pass.filter();
    if (rt.kernel == BinBatchKernel::Rs) {
        for (uint32_t q0 = 0; q0 < Q; q0 += TQ) {  // one pass over the rows per query tile; its lists are scattered right away
            const BinRsCall c{h, b, h->rows.as<uint8_t>(), n, q0, rt.mi, nullptr, 0, f, s};
            QAMD_TRY(largest ? launch_bin_rs<1>(c) : launch_bin_rs<2>(c));
            pass.scatter();
        }
    } else {  // the FP4 forms: the batch's nibble image once, a launch per pass or slice, then one scatter
        const bool zx = bin_zx(h);
        const bool low = (!zx) != (largest == 0);  // multiplier = zx ? +4 : -4; MODE 2 (smallest) flips
        const uint32_t nsteps = (uint32_t)(h->ds / 16);
        StreamBuf prep;
        const size_t frag_bytes = (size_t)q_pad * h->ds * 4;
        QAMD_TRY(prep.alloc(frag_bytes + q_pad * 8, s));
        uint4 *frag = prep.as<uint4>();
        float *q_off = reinterpret_cast<float *>(prep.as<char>() + frag_bytes);
        int *bq = reinterpret_cast<int *>(q_off + q_pad);
        const unsigned pgrid = (unsigned)std::max<uint64_t>((q_pad + 255) / 256, std::min<uint64_t>(2048, (frag_bytes / 16 + 255) / 256));
        if (low)
            hipLaunchKernelGGL(bin_frag4_kernel<true>, dim3(pgrid), dim3(256), 0, s, b->planes.as<uint8_t>(), (uint32_t)b->p_stride, (uint32_t)Q,
                               (uint32_t)q_pad, nsteps, metric_dim(h, 1), zx ? 1 : 0, largest, pass.pivot_scores(), frag, q_off, bq);
        else
            hipLaunchKernelGGL(bin_frag4_kernel<false>, dim3(pgrid), dim3(256), 0, s, b->planes.as<uint8_t>(), (uint32_t)b->p_stride, (uint32_t)Q,
                               (uint32_t)q_pad, nsteps, metric_dim(h, 1), zx ? 1 : 0, largest, pass.pivot_scores(), frag, q_off, bq);
        const bool rs4 = rt.kernel == BinBatchKernel::Rs4;
        const uint64_t per_launch = rs4 ? rt.rs4_per_pass : kQs4Slice;
        const uint32_t lists_per_launch = rs4 ? rt.n_lists / rt.rs4_passes : pp_waves_per_launch();
        for (uint64_t q_base = 0; q_base < Q; q_base += per_launch) {
            BinFp4Call c{h, frag, q_off, bq, q_base, (uint32_t)std::min<uint64_t>(per_launch, Q - q_base), f, s};
            c.filt.pivot_scores += q_base;
            c.filt.query_base = (uint32_t)q_base;
            c.filt.wave_base = (uint32_t)(q_base / per_launch) * lists_per_launch;
            if (rs4) QAMD_TRY(largest ? launch_bin_rs4<1>(rt, c) : launch_bin_rs4<2>(rt, c));
            else QAMD_TRY(largest ? launch_bin_qs4<1>(rt, c) : launch_bin_qs4<2>(rt, c));
        }
        pass.scatter();
    }
    QAMD_TRY(pass.emit(ids_dev, sc_dev));
    QAMD_TRY(pass.read_status(status));
    char tail[32] = "";  // a scalar batch adds its bit count behind the fields the binary line has
    if (b->qbits != 1) snprintf(tail, sizeof tail, ", query bits %u", b->qbits);
    pass.debug_line("[qamd bin topk_batch]", r, rt.name, tail, status);
    return QAMD_OK;
}

}  // namespace


// Every batch encode: query q of the batch is the single-query encode of row q of `queries` (the same kernels, one bit
// "row" or one workgroup per query), kept as its planes and, for 4 / 8 bits, as the matrix cores' int8
// image.  `weighted` on two-bit rows: DESIGN 3.2f, the planes and the image sized by code_bits.
static qamd_status encode_query_batch(const qamd_bin *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                      qamd_mem queries_mem, uint32_t bits, bool weighted, void *stream,
                                      qamd_bin_query_batch **batch_io) {
    if (bits != 1 && bits != 4 && bits != 8) return fail(QAMD_ERR_ARGUMENTS, "query bits must be 1, 4 or 8, not %u", bits);
    if (!h || !batch_io || (!queries && n_queries && qdim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    const bool two = h->two();
    if (bits != 1 && two && !weighted)
        return fail(QAMD_ERR_ARGUMENTS, "two-bit rows take scalar queries through qamd_bin_encode_query_batch_scalar_w");
    if (two && n_queries && qdim != h->vp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "queries of %llu dimensions against thresholds of %llu", (unsigned long long)qdim,
                    (unsigned long long)h->vp.dim);
    if (h->rotated() && n_queries && qdim != h->vp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "queries of %llu dimensions against rotated rows of %llu", (unsigned long long)qdim,
                    (unsigned long long)h->vp.dim);
    const uint64_t edim = encoder_dim(qdim, h->encoding);  // rotated queries are encoded as P values
    const uint64_t max_dim = scalar_max_dim(bits, two);  // as the single query: code_bits * L stays exact in f32
    if (bits != 1 && edim > max_dim)
        return fail(QAMD_ERR_ARGUMENTS, "a %u-bit query has at most %llu dimensions, not %llu", bits,
                    (unsigned long long)max_dim, (unsigned long long)edim);
    if (bits != 1 && n_queries > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "too many queries");  // one workgroup each
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t nb = row_bytes_of(two ? 2 * edim : edim, h->store), ds = device_stride_of(nb);
    if (n_queries && nb != h->nb)
        return fail(QAMD_ERR_ARGUMENTS, "queries have %llu bytes, rows have %llu", (unsigned long long)nb,
                    (unsigned long long)h->nb);
    qamd_bin_query_batch *b = *batch_io;
    std::unique_ptr<qamd_bin_query_batch> fresh;
    if (!b) {
        fresh.reset(new qamd_bin_query_batch);
        b = fresh.get();
        b->device = h->device;
    }
    const uint64_t p_stride = round_up(bits * ds, 16);
    const uint64_t code_pitch = round_up(ds, 16) * 8 + 16;  // ds / 16 K-blocks of 128 bytes + 16: bin_gemm_rs_kernel's PA
    const size_t need_p = std::max<size_t>(p_stride * n_queries, 16), need_c = std::max<size_t>(code_pitch * n_queries, 16);
    // zeroed planes whenever their layout changes: a reused batch of any earlier kind behaves as a fresh one
    if (b->planes.bytes < need_p || b->p_stride != p_stride || b->qbits != bits) QAMD_TRY(b->planes.alloc(need_p, true));
    if (bits != 1) {  // (the encoder writes every byte of a query's pitch and its max_abs)
        if (b->codes.bytes < need_c) QAMD_TRY(b->codes.alloc(need_c, true));
        if (b->max_abs.bytes < std::max<size_t>(n_queries * 4, 16)) QAMD_TRY(b->max_abs.alloc(std::max<size_t>(n_queries * 4, 16), true));
    }
    b->nb = nb;
    b->ds = ds;
    b->n_queries = n_queries;
    b->qbits = bits;
    b->p_stride = p_stride;
    b->code_pitch = code_pitch;
    if (n_queries) {
        DevBuf qtmp;
        const void *qd = nullptr;
        bool staged = false;
        if (qdim) QAMD_TRY(local_view(queries, queries_mem, n_queries * qdim * 4, qtmp, s, &qd, &staged));
        if (bits == 1)
            launch_bit_encoder(h, static_cast<const float *>(qd), n_queries, qdim, p_stride / 4, b->planes.as<uint32_t>(), 0, s);
        else
            QAMD_TRY(launch_scalar_encoder(h, static_cast<const float *>(qd), n_queries, qdim, ds, bits, b->planes.as<uint32_t>(),
                                           p_stride, b->max_abs.as<float>(), b->codes.as<int8_t>(), code_pitch, s));
        QAMD_HIP(hipGetLastError());
        if (staged) QAMD_HIP(hipStreamSynchronize(s));
    }
    if (fresh) *batch_io = fresh.release();
    return QAMD_OK;
}

extern "C" {

qamd_status qamd_bin_encode_query_batch(const qamd_bin *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                        qamd_mem queries_mem, void *stream, qamd_bin_query_batch **batch_io) {
    return encode_query_batch(h, queries, n_queries, qdim, queries_mem, 1, false, stream, batch_io);
}

qamd_status qamd_bin_encode_query_batch_scalar(const qamd_bin *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                               qamd_mem queries_mem, uint32_t bits, void *stream,
                                               qamd_bin_query_batch **batch_io) {
    return encode_query_batch(h, queries, n_queries, qdim, queries_mem, bits, false, stream, batch_io);
}

// on two-bit rows query q is qamd_bin_encode_query_scalar_w of row q of `queries`, its int8 image one byte
// per bit position of a row; on one-bit rows the call above.
qamd_status qamd_bin_encode_query_batch_scalar_w(const qamd_bin *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                                 qamd_mem queries_mem, uint32_t bits, void *stream,
                                                 qamd_bin_query_batch **batch_io) {
    return encode_query_batch(h, queries, n_queries, qdim, queries_mem, bits, true, stream, batch_io);
}

qamd_status qamd_bin_query_batch_info(const qamd_bin_query_batch *b, uint32_t *bits, uint64_t *n_queries) {
    if (!b) return fail(QAMD_ERR_ARGUMENTS, "null query batch");
    if (bits) *bits = b->qbits;
    if (n_queries) *n_queries = b->n_queries;
    return QAMD_OK;
}

qamd_status qamd_bin_query_batch_read(const qamd_bin_query_batch *b, uint64_t q, uint8_t *bits, uint64_t capacity, uint64_t *len) {
    if (!b) return fail(QAMD_ERR_ARGUMENTS, "null query batch");
    if (q >= b->n_queries) return fail(QAMD_ERR_OUT_OF_RANGE, "query %llu of %llu", (unsigned long long)q, (unsigned long long)b->n_queries);
    const uint64_t total = b->qbits * b->nb;  // as qamd_bin_query_read: the planes, plane 0 first, nb bytes each
    if (len) *len = total;
    if (bits) {
        if (capacity < total) return fail(QAMD_ERR_ARGUMENTS, "bits buffer too small");
        QAMD_ON_DEVICE(b->device);
        std::vector<uint8_t> wide(b->qbits * b->ds);  // planes are held at the device stride (4 bytes for the tiny rows)
        if (!wide.empty()) QAMD_TRY(copy_out(wide.data(), QAMD_MEM_HOST, bin_batch_query(b, q), wide.size(), nullptr));
        for (uint32_t pl = 0; pl < b->qbits; pl++) memcpy(bits + pl * b->nb, &wide[pl * b->ds], b->nb);
    }
    return QAMD_OK;
}

void qamd_bin_query_batch_free(qamd_bin_query_batch *b) { delete b; }

static qamd_status bin_check_batch(const qamd_bin *h, const qamd_bin_query_batch *b) {
    if (!h || !b) return fail(QAMD_ERR_ARGUMENTS, "null handle or query batch");
    if (b->n_queries && b->nb != h->nb)
        return fail(QAMD_ERR_ARGUMENTS, "queries have %llu bytes, rows have %llu", (unsigned long long)b->nb,
                    (unsigned long long)h->nb);
    if (b->qbits != 1 && b->qbits != 4 && b->qbits != 8) return fail(QAMD_ERR_ARGUMENTS, "query batch of %u bits", b->qbits);
    if (b->n_queries && b->qbits != 1 && (b->ds != h->ds || !b->planes.ptr || !b->codes.ptr))
        return fail(QAMD_ERR_ARGUMENTS, "scalar query batch without its planes or codes");
    return QAMD_OK;
}

// ---- routing: ONE route (bin_route -> bin_batch_route.hpp, with the gates and the measurements behind them), read by the
// entry points and by qamd_bin_batch_kernel
const char *qamd_bin_batch_kernel(const qamd_bin *h, const qamd_bin_query_batch *b, uint32_t k) {
    if (bin_check_batch(h, b) != QAMD_OK) return nullptr;
    const BinBatchRoute route = bin_route(h, b, k);
    if (route.mfma) return route.name;
    // the per-query routes: small stores take the single-launch top-k; binary queries share a pass over the rows
    SmallTopkPlan small;
    if (k != 0 && h->count <= (2u << 20) && bin_small_plan(h, k, b->qbits, small)) return "bin_topk_small_kernel";
    if (b->qbits == 1 && b->n_queries >= 2 && multi_rows(h)) return "bin_scan_multi_kernel";
    return fused_capable(h) ? "bin_scan_kernel" : "bin_words_kernel";
}

// Many (query, id list) pairs in one launch (lists.hpp): out[p] = score_point(query l, ids[p]).
qamd_status qamd_bin_score_ids_batch(const qamd_bin *h, const qamd_bin_query_batch *b, const uint32_t *list_offsets,
                                     uint32_t n_lists, const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem, float *out,
                                     qamd_mem out_mem, void *stream) {
    QAMD_TRY(bin_check_batch(h, b));
    if (n_lists > b->n_queries)
        return fail(QAMD_ERR_ARGUMENTS, "%u lists, but the batch holds %llu queries", n_lists, (unsigned long long)b->n_queries);
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    return run_lists(list_offsets, n_lists, ids, n_ids, nullptr, lists_mem, out, out_mem, h->count, s, [&](const ListArgs &a) {
        // list l against the planes of query l
        return pairs_launch(h, nullptr, b->planes.as<uint8_t>(), b->p_stride, a.offsets, a.n_lists, nullptr, a.ids, a.n_pairs,
                            a.out, s, b->qbits);
    });
}

qamd_status qamd_bin_score_batch(const qamd_bin *h, const qamd_bin_query_batch *b, float *out, qamd_mem out_mem,
                                 void *stream) {
    QAMD_TRY(bin_check_batch(h, b));
    if (h->count == 0 || b->n_queries == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "out is null");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    StreamBuf tmp;
    float *out_dev = out;
    if (out_mem == QAMD_MEM_HOST) {
        QAMD_TRY(tmp.alloc(b->n_queries * h->count * 4, s));
        out_dev = tmp.as<float>();
    }
    uint64_t q = 0;
    // 5 queries and more: tiles of 32 / 64 queries on the matrix cores (same scores bit for bit: every f32
    // of the epilogue is an exact integer); the row bits are read once per tile instead of once per 8 queries
    // (measured at 50M x 1024: one 32-query tile 2.28 ms whatever the batch; the vector-ALU passes 1.81 ms for 4
    // queries, 2.6 for 8, and from there 2.6 ms per 8)
    const BinBatchRoute route = bin_route(h, b, 0);
    if (route.mfma) {
        for (; q < b->n_queries; q += 32 * route.mi)  // (a partly filled last tile computes zero queries and stores nothing for them)
            QAMD_TRY(launch_bin_rs<0>({h, b, h->rows.as<uint8_t>(), h->count, (uint32_t)q, route.mi, out_dev, h->count, BatchFilter{}, s}));
    }
    for (; b->qbits != 1 && q < b->n_queries; q++)  // scalar queries off the matrix cores: one scan of the planes each
        QAMD_TRY(scan_bits(h, bin_batch_query(b, q), out_dev + q * h->count, s, nullptr, b->qbits));
    while (q < b->n_queries) {
        const uint64_t left = b->n_queries - q;
        const uint8_t *qb = bin_batch_query(b, q);
        float *o = out_dev + q * h->count;
        if (left >= 8 && multi_step<8>(h, qb, b->p_stride, o, s)) q += 8;
        else if (left >= 4 && multi_step<4>(h, qb, b->p_stride, o, s)) q += 4;
        else if (left >= 2 && multi_step<2>(h, qb, b->p_stride, o, s)) q += 2;
        else {
            QAMD_TRY(scan_bits(h, qb, o, s));
            q += 1;
        }
    }
    QAMD_HIP(hipGetLastError());
    if (out_mem == QAMD_MEM_HOST) return copy_out(out, QAMD_MEM_HOST, out_dev, b->n_queries * h->count * 4, s);
    return QAMD_OK;
}

qamd_status qamd_bin_topk_batch(const qamd_bin *h, const qamd_bin_query_batch *b, uint32_t k, int largest,
                                uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream) {
    QAMD_TRY(bin_check_batch(h, b));
    qamd_status args = QAMD_OK;
    if (!topk_wanted(k, b->n_queries, out_ids, out_scores, args)) return args;
    QAMD_ON_DEVICE(h->device);
    const uint64_t qs = b->p_stride;  // (a binary batch: the stride of its bit rows)
    const uint32_t planes = b->qbits;  // 1: query q is its bit row; 4 / 8: its planes (bin_batch_query)
    BatchScan scan;
    scan.filter_capable = fused_capable(h);
    scan.scan_scores = [&](uint32_t q, float *scores, hipStream_t st) { return scan_bits(h, bin_batch_query(b, q), scores, st, nullptr, planes); };
    scan.scan_filter = [&](uint32_t q, const TopkFilter &f, hipStream_t st) {
        return scan_bits(h, bin_batch_query(b, q), nullptr, st, &f, planes);
    };
    scan.score_ids = [&](uint32_t q, const uint32_t *ids, uint64_t n_ids, float *out, hipStream_t st) {
        return words_launch(h, reinterpret_cast<const uint32_t *>(bin_batch_query(b, q)), ids, n_ids, out, st, planes);
    };
    scan.topk_small = [&](uint32_t q, uint32_t *ids, float *sc, hipStream_t st, qamd_status &status) {
        return bin_topk_small(h, bin_batch_query(b, q), k, largest, ids, sc, QAMD_MEM_DEVICE, st, status, planes);
    };
    // up to 8 binary queries share one pass over the rows (the filtering form of bin_scan_multi_kernel)
    if (planes == 1) {
        scan.scan_filter_multi = [&](uint32_t q, uint32_t left, const TopkFilterSlices &sl, hipStream_t st, qamd_status &status) -> uint32_t {
            const uint8_t *qb = bin_batch_query(b, q);
            uint32_t took = 0;
            if (left >= 8 && multi_step<8>(h, qb, qs, nullptr, st, &sl)) took = 8;
            else if (left >= 4 && multi_step<4>(h, qb, qs, nullptr, st, &sl)) took = 4;
            else if (left >= 2 && multi_step<2>(h, qb, qs, nullptr, st, &sl)) took = 2;
            if (took && hipGetLastError() != hipSuccess) status = fail(QAMD_ERR_DEVICE, "binary multi-query filter launch failed");
            return took;
        };
    }
    // 12 queries and more on stores of 32k rows and more (below that the filtering vector-ALU passes, 0.22 ms per
    // query at 50M rows, are cheaper than one matrix-core pass): bin_gemm_rs_kernel; queries whose
    // candidate list over- or underflowed there (heavy ties at small dims) go through the path below one by one
    const uint64_t Q = b->n_queries;
    hipStream_t s = as_stream(stream);
    const BinBatchRoute route = bin_route(h, b, k);
    if (route.mfma) {
        BatchTopkOutputs out;
        QAMD_TRY(out.begin(Q, k, out_ids, out_scores, out_mem, s));
        QAMD_TRY(bin_topk_batch_mfma(h, b, route, k, largest, out.ids_dev, out.sc_dev, out.status, s));
        return out.finish([&](uint64_t q, uint32_t *ids_dev, float *sc_dev) {
            BatchScan one;
            one.filter_capable = scan.filter_capable;
            one.scan_scores = [&, q](uint32_t, float *scores, hipStream_t st) { return scan.scan_scores((uint32_t)q, scores, st); };
            one.scan_filter = [&, q](uint32_t, const TopkFilter &f, hipStream_t st) { return scan.scan_filter((uint32_t)q, f, st); };
            one.score_ids = [&, q](uint32_t, const uint32_t *ids, uint64_t n_ids, float *out1, hipStream_t st) {
                return scan.score_ids((uint32_t)q, ids, n_ids, out1, st);
            };
            one.topk_small = [&, q](uint32_t, uint32_t *ids, float *sc, hipStream_t st, qamd_status &status1) {
                return scan.topk_small((uint32_t)q, ids, sc, st, status1);
            };
            return fused_topk_batch(h->count, 1, k, largest, ids_dev, sc_dev, QAMD_MEM_DEVICE, s, one);
        });
    }
    return fused_topk_batch(h->count, (uint32_t)b->n_queries, k, largest, out_ids, out_scores, out_mem, s, scan);
}

}  // extern "C"


// ============================================================================= streaming encode
// EncodedVectorsBin::encode (:165-191) walks its iterator ONCE, pushing one packed row per vector
// (EncodedStorageBuilder::push_vector_data, encoded_storage.rs:17-25); here in bounded batches.
struct qamd_bin_encoder {
    int device = 0;
    hipStream_t stream = nullptr;
    qamd_stop_fn stop = nullptr;
    void *stop_user = nullptr;
    std::unique_ptr<qamd_bin> h;
    uint64_t pushed = 0;
    DevBuf stage;
    // two-bit rows without given thresholds: every row is observed before the first push
    bool learns = false;    // set by begin
    bool learning = false;  // the observe pass is open
    uint64_t observed = 0;
    BinStats stats;
};

// The end of the observe pass: the statistics of all vp.count rows become the store's thresholds.
static qamd_status bin_encoder_close_observe(qamd_bin_encoder *e) {
    if (!e->learning) return QAMD_OK;
    if (e->observed != e->h->count)
        return fail(QAMD_ERR_ARGUMENTS, "%llu of %llu rows were observed before the first push", (unsigned long long)e->observed,
                    (unsigned long long)e->h->count);
    QAMD_TRY(set_thresholds_from_stats(e->h.get(), e->stats, e->stream));
    e->learning = false;
    return QAMD_OK;
}

extern "C" {

qamd_status qamd_bin_encoder_begin(const qamd_vector_parameters *vp, qamd_bits_store store, qamd_stop_fn stop,
                                   void *stop_user, void *stream, qamd_bin_encoder **out) {
    return qamd_bin_encoder_begin_enc(vp, store, QAMD_BIN_ONE_BIT, nullptr, nullptr, stop, stop_user, stream, out);
}

qamd_status qamd_bin_encoder_begin_enc(const qamd_vector_parameters *vp, qamd_bits_store store, qamd_bin_encoding encoding,
                                       const float *lo, const float *hi, qamd_stop_fn stop, void *stop_user, void *stream,
                                       qamd_bin_encoder **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    QAMD_TRY(refuse_u8_flags(vp));
    QAMD_TRY(check_enc_args(vp, encoding, lo, hi, false));
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "count exceeds u32 row ids");
    QAMD_ON_DEVICE(current_device());
    std::unique_ptr<qamd_bin_encoder> e(new qamd_bin_encoder);
    e->device = current_device();
    e->stream = as_stream(stream);
    e->stop = stop;
    e->stop_user = stop_user;
    QAMD_TRY(new_store(vp, store, encoding, e->h));
    if (lo) {
        QAMD_TRY(set_thresholds(e->h.get(), lo, hi, e->stream));
    } else if (e->h->two()) {
        e->learns = e->learning = true;
        QAMD_TRY(e->stats.begin(e->h->edim));
    }
    *out = e.release();
    return QAMD_OK;
}

qamd_status qamd_bin_encoder_observe(qamd_bin_encoder *e, const float *batch, uint64_t n_rows, qamd_mem batch_mem) {
    if (!e || (!batch && n_rows && e->h->vp.dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (e->stop && e->stop(e->stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");
    if (!e->learns) return QAMD_OK;  // one bit, or thresholds given: nothing to learn
    if (!e->learning) return fail(QAMD_ERR_ARGUMENTS, "observe after push");
    if (e->observed + n_rows > e->h->count) return count_mismatch(e->observed + n_rows, e->h->count);
    QAMD_ON_DEVICE(e->device);
    QAMD_TRY(stats_feed(e->stats, batch, batch_mem, n_rows, e->stage, e->stream, e->stop, e->stop_user,
                        e->h->rotated() ? e->h->vp.dim : 0, e->h->blocks()));
    e->observed += n_rows;
    return QAMD_OK;
}

qamd_status qamd_bin_encoder_push(qamd_bin_encoder *e, const float *batch, uint64_t n_rows, qamd_mem batch_mem) {
    if (!e || (!batch && n_rows && e->h->vp.dim)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (e->stop && e->stop(e->stop_user)) return fail(QAMD_ERR_STOPPED, "Stopped");  // :174-176
    if (e->pushed + n_rows > e->h->count) return count_mismatch(e->pushed + n_rows, e->h->count);
    QAMD_ON_DEVICE(e->device);
    QAMD_TRY(bin_encoder_close_observe(e));
    const uint64_t dim = e->h->vp.dim;
    const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / std::max<uint64_t>(dim * 4, 1));
    if (dim)
        QAMD_TRY(for_each_staged_piece(batch, batch_mem, n_rows, dim, piece_rows, e->stage, e->stream,
                                       [&](const float *src, uint64_t r, uint64_t nr) {
            return launch_bin_encode(e->h.get(), src, nr, e->pushed + r, e->stream);
        }));
    e->pushed += n_rows;
    return QAMD_OK;
}

qamd_status qamd_bin_encoder_finish(qamd_bin_encoder *e, qamd_bin **out) {
    if (!e || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    std::unique_ptr<qamd_bin_encoder> own(e);
    if (e->pushed != e->h->count) return count_mismatch(e->pushed, e->h->count);
    QAMD_ON_DEVICE(e->device);
    QAMD_TRY(bin_encoder_close_observe(e));  // (a store of no rows: thresholds of no statistics)
    QAMD_HIP(hipStreamSynchronize(e->stream));
    *out = e->h.release();
    return QAMD_OK;
}

void qamd_bin_encoder_abort(qamd_bin_encoder *e) { abort_encoder(e); }

// ---- upsert: rows overwritten or appended with the store's own encoding and thresholds - launch_bin_encode
// at a row offset, as the streaming encoder's push.  The reference snapshot has no counterpart.
static qamd_status bin_grow(qamd_bin *h, uint64_t cap) {
    if (cap <= h->capacity) return QAMD_OK;
    DevBuf rows;
    QAMD_TRY(grow_copy(h->rows, padded_rows_of(cap) * h->ds, h->count * h->ds, rows));
    h->rows = std::move(rows);  // (the old buffer goes through hipFree, which waits for the device)
    h->capacity = cap;
    return QAMD_OK;
}

uint64_t qamd_bin_capacity(const qamd_bin *h) { return h ? h->capacity : 0; }

qamd_status qamd_bin_reserve(qamd_bin *h, uint64_t capacity_rows, void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (capacity_rows > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "capacity exceeds u32 row ids");
    if (capacity_rows <= h->capacity) return QAMD_OK;
    QAMD_ON_DEVICE(h->device);
    QAMD_HIP(hipStreamSynchronize(as_stream(stream)));
    return bin_grow(h, capacity_rows);
}

qamd_status qamd_bin_upsert(qamd_bin *h, uint64_t first_row, const float *data, qamd_mem data_mem, uint64_t n_rows,
                            void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    const uint64_t dim = h->vp.dim;
    QAMD_TRY(check_upsert(first_row, n_rows, h->count, data, dim));
    if (n_rows == 0) return QAMD_OK;
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t end = first_row + n_rows;
    if (end > h->capacity) {
        QAMD_HIP(hipStreamSynchronize(s));
        QAMD_TRY(bin_grow(h, std::min<uint64_t>(upsert_capacity(end, h->capacity), 0xFFFFFFFFull)));
    }
    if (dim) {
        DevBuf stage;
        const uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / (dim * 4));
        QAMD_TRY(for_each_staged_piece(data, data_mem, n_rows, dim, piece_rows, stage, s,
                                       [&](const float *src, uint64_t r, uint64_t nr) {
            return launch_bin_encode(h, src, nr, first_row + r, s);
        }));
    }
    QAMD_HIP(hipStreamSynchronize(s));
    h->count = std::max(h->count, end);
    h->vp.count = h->count;
    std::lock_guard<std::mutex> lk(h->sample_mu);  // the next query batch gathers its pivot sample again
    h->sample_rows.release();
    h->sample_count = 0;
    return QAMD_OK;
}

}  // extern "C"

#ifdef QAMD_DEV
// Developer-only accessors for the tuning harness (tune.hip): libquantization_amd_dev.so only.
extern "C" __attribute__((visibility("default"))) const void *qamd_dev_bin_rows(const qamd_bin *h) { return h->rows.ptr; }
extern "C" __attribute__((visibility("default"))) const void *qamd_dev_bin_query_ptr(const qamd_bin_query *q) {
    return q->buf.ptr;
}
#endif

// ============================================================================= rescoring with the original vectors
// rerank(orig, query_f32, ids of topk(h, q, candidates, largest), k): one body for the three quantizers (rescore.hpp).
extern "C" qamd_status qamd_bin_topk_rescored(const qamd_bin *h, const qamd_bin_query *q, const qamd_f32 *orig,
                                              const float *query_f32, uint64_t qdim, qamd_mem query_mem, uint32_t k,
                                              uint32_t candidates, int largest, uint32_t *out_ids, float *out_scores,
                                              qamd_mem out_mem, void *stream) {
    if (!h || !q) return qamd::fail(QAMD_ERR_ARGUMENTS, "null handle or query");
    return qamd::topk_rescored(h->device, h->vp, orig, query_f32, 1, qdim, query_mem, k, candidates, largest, out_ids,
                               out_scores, out_mem, qamd::as_stream(stream), [&](uint32_t *ids_dev, float *scores_dev) {
                                   return qamd_bin_topk(h, q, candidates, largest, ids_dev, scores_dev, QAMD_MEM_DEVICE, stream);
                               });
}

extern "C" qamd_status qamd_bin_topk_batch_rescored(const qamd_bin *h, const qamd_bin_query_batch *b, const qamd_f32 *orig,
                                                    const float *queries_f32, uint64_t n_queries, uint64_t qdim,
                                                    qamd_mem queries_mem, uint32_t k, uint32_t candidates, int largest,
                                                    uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream) {
    if (!h || !b) return qamd::fail(QAMD_ERR_ARGUMENTS, "null handle or query batch");
    if (n_queries != b->n_queries)
        return qamd::fail(QAMD_ERR_ARGUMENTS, "%llu f32 queries, but the batch holds %llu", (unsigned long long)n_queries,
                          (unsigned long long)b->n_queries);
    return qamd::topk_rescored(h->device, h->vp, orig, queries_f32, n_queries, qdim, queries_mem, k, candidates, largest,
                               out_ids, out_scores, out_mem, qamd::as_stream(stream), [&](uint32_t *ids_dev, float *scores_dev) {
                                   return qamd_bin_topk_batch(h, b, candidates, largest, ids_dev, scores_dev, QAMD_MEM_DEVICE, stream);
                               });
}
