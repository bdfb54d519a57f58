// The original f32 vectors beside a quantized store, and exact scoring of id lists against them.
//
// The caller of the reference over-fetches k' > k candidates from the quantized scan and scores them again with
// DistanceType::distance (quantization/src/encoded_vectors.rs:37-45): the SEQUENTIAL f32 sum of a*b, |a-b| or
// (a-b)*(a-b) over the dimensions, starting at +0.0.  That order leaves no parallelism inside one (query, row)
// pair, so a lane owns a pair and walks its row in order; the parallelism is across pairs.
//
// f32_pairs_kernel: a wave takes 64 pairs.  Per 32-value segment of the rows, each half-wave reads one row's
// 128 bytes coalesced (dword loads: rows are only 4-byte aligned when dim % 4 != 0), 32 such loads per lane
// cover the 64 rows; the tile goes through LDS with a row stride of 33 dwords (ds_write_b32 and ds_read_b32
// bank = dword address mod 32 over groups of 32 lanes: the writes of a half-wave hit 32 consecutive dwords, the
// reads of lanes r hit r * 33 + c - both conflict-free), and lane r then adds its row's 32 terms in order,
// carrying the partial sum from segment to segment.  The loads of the next segment are issued before the adds
// of the current one.  The query value of a step is wave-uniform when all 64 pairs belong to one list (a scalar
// load); a wave that straddles lists reads it per lane.
//
// half_pairs_kernel: the same scheme for rows kept as f16 or bf16 (qamd_f32_from_data_typed).  A score is the same
// sequential f32 sum over the row WIDENED EXACTLY to f32 (v_cvt_f32_f16, which keeps f16 subnormals: they are f32
// normals; a bf16 is the upper half of an f32: a shift or a mask), so every product or difference is still rounded to
// f32 before its add and the result equals qo_metric_f32 of the widened row bit for bit.  The tile is redesigned for
// 2-byte elements: 128 coalesced bytes of a row are 64 values, so a segment is 64 values and a row needs half as many
// passes, loads and LDS operations per value as an f32 row.
//  * Loads.  dim even (and a dword-aligned base): every row starts on a dword, lane j of a half-wave loads the
//    packed pair (2j, 2j + 1) with one dword load - 32 dword loads per lane cover the wave's 64 rows, as for f32.
//    dim odd: every other row starts 2 bytes off a dword, so the same dword loads are issued at 2-byte aligned
//    addresses (global memory takes them: the compiler emits them for an align-2 copy of 4 bytes; such a load costs a
//    second cache-line access only where it straddles one), and only pairs that lie inside the row are loaded: the
//    last value of an odd row is read once by the lane that owns the row, a 2-byte load.  Only this shape pays for it.
//  * LDS.  The tile holds the PACKED dwords, not widened f32: 64 rows x 33 dwords per wave, the f32 kernel's 8448
//    bytes for twice the values (widened values would need 65 dwords per row: 2 workgroups per CU less).  Bank
//    arithmetic as above: ds_write_b32 / ds_read_b32 bank = dword address mod 32 over groups of 32 lanes; a
//    half-wave writes the 32 consecutive dwords (2i + half) * 33 + col, col = 0..31: 32 banks; lane r reads
//    r * 33 + c, bank (r + c) mod 32: 32 banks over r = 0..31 and over r = 32..63.  Both conflict-free.  Lane r
//    widens the low half, adds its term, widens the high half, adds its term: the row's order.
//  * The loads of the next segment are issued before the adds of the current one; the wave-uniform (scalar) query
//    path and the per-lane path are those of the f32 kernel.
// A NULL id list in qamd_f32_score_ids / qamd_f32_rerank / qamd_f32_rerank_batch stands for the rows 0 .. n_ids - 1 and
// takes the whole-store scan of f32_scan.hip instead (rerank_scan below): rows in order, 1 to 8 queries per pass.
// narrow_kernel: the F32 -> F16 / BF16 copy of qamd_f32_from_data_typed, a streaming kernel (16-byte loads, 8-byte
// stores where the piece is aligned for them).
#include "rescore.hpp"

#include "f32_terms.hpp"
#include "lists.hpp"
#include "topk.hpp"

#include <memory>

namespace qamd {
namespace {

constexpr int kBlock = 256;      // 4 waves, each with its own tile
constexpr int kSeg = 32;         // values of a row per pass
constexpr int kTileStride = 33;  // dwords between two rows of a tile

// out[p] = distance(query of pair p, row ids[p]), negated for `invert`; NaN for an id >= count.
// Pair p belongs to list l: offsets[l] <= p < offsets[l + 1], or l = p / per_list when offsets is null.
template <int METRIC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void f32_pairs_kernel(const float *__restrict__ data, uint32_t dim, uint32_t count,
                                                          const float *__restrict__ queries,
                                                          const uint32_t *__restrict__ offsets, uint32_t n_lists,
                                                          uint32_t per_list, const uint32_t *__restrict__ ids,
                                                          uint32_t n_pairs, int invert, float *__restrict__ out) {
    __shared__ float tiles[kBlock / 64][64 * kTileStride];
    __shared__ uint32_t first_list;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *tile = tiles[wave];
    const uint32_t p0 = blockIdx.x * (uint32_t)kBlock;
    const uint32_t p = p0 + threadIdx.x;
    const bool in_range = p < n_pairs;
    uint32_t l = 0;
    if (offsets) {
        l = first_list_of_block(offsets, n_lists, p0, &first_list);
        if (in_range) l = advance_list(offsets, n_lists, l, p);
    } else if (in_range) {
        l = p / per_list;
    }
    const uint32_t id = in_range ? ids[p] : 0xFFFFFFFFu;
    const bool valid = id < count;
    // the lists of the wave's first and last pair in range: equal = one query for the whole wave
    const uint32_t n_here = n_pairs - min(n_pairs, p0 + (uint32_t)wave * 64u);  // pairs at or after the wave's first
    const int last_lane = n_here >= 64 ? 63 : (n_here ? (int)n_here - 1 : 0);
    const uint32_t l_first = (uint32_t)__shfl((int)l, 0, 64), l_last = (uint32_t)__shfl((int)l, last_lane, 64);
    const bool one_query = l_first == l_last;
    const float *__restrict__ q_wave = queries + (size_t)__builtin_amdgcn_readfirstlane((int)l_first) * dim;
    const float *__restrict__ q_lane = queries + (size_t)l * dim;

    // lane j loads column (j & 31) of the rows 2i + (j >> 5), i = 0..31
    const int col = lane & 31, half = lane >> 5;
    uint32_t row_id[kSeg];
#pragma unroll
    for (int i = 0; i < kSeg; i++) row_id[i] = (uint32_t)__shfl((int)id, 2 * i + half, 64);
    float next[kSeg];
    auto load_segment = [&](uint32_t d0) {
        const uint32_t d = d0 + (uint32_t)col;
#pragma unroll
        for (int i = 0; i < kSeg; i++)
            next[i] = (row_id[i] < count && d < dim) ? data[(size_t)row_id[i] * dim + d] : 0.0f;
    };
    float sum = 0.0f;
    load_segment(0);
    for (uint32_t d0 = 0; d0 < dim; d0 += kSeg) {
#pragma unroll
        for (int i = 0; i < kSeg; i++) tile[(2 * i + half) * kTileStride + col] = next[i];
        __syncthreads();
        if (d0 + kSeg < dim) load_segment(d0 + kSeg);
        const float *mine = tile + lane * kTileStride;
        const uint32_t n = min((uint32_t)kSeg, dim - d0);
        if (one_query) {
            if (n == kSeg) {
#pragma unroll
                for (int c = 0; c < kSeg; c++) sum += term<METRIC>(q_wave[d0 + c], mine[c]);
            } else {
                for (uint32_t c = 0; c < n; c++) sum += term<METRIC>(q_wave[d0 + c], mine[c]);
            }
        } else if (in_range) {
            for (uint32_t c = 0; c < n; c++) sum += term<METRIC>(q_lane[d0 + c], mine[c]);
        }
        __syncthreads();
    }
    if (in_range) out[p] = valid ? (invert ? -sum : sum) : __builtin_nanf("");
}

constexpr int kHalfSeg = 64;  // values of an f16 / bf16 row per pass: 128 bytes, 32 packed dwords

// f32_pairs_kernel for rows of 16-bit values (DTYPE: QAMD_DTYPE_F16 or QAMD_DTYPE_BF16).  ALIGNED: dim is even and
// `data` is dword aligned, so every row starts on a dword.
template <int METRIC, int DTYPE, bool ALIGNED>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void half_pairs_kernel(
    const uint16_t *__restrict__ data, uint32_t dim, uint32_t count, const float *__restrict__ queries,
    const uint32_t *__restrict__ offsets, uint32_t n_lists, uint32_t per_list, const uint32_t *__restrict__ ids,
    uint32_t n_pairs, int invert, float *__restrict__ out) {
    __shared__ uint32_t tiles[kBlock / 64][64 * kTileStride];
    __shared__ uint32_t first_list;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *tile = tiles[wave];
    const uint32_t p0 = blockIdx.x * (uint32_t)kBlock;
    const uint32_t p = p0 + threadIdx.x;
    const bool in_range = p < n_pairs;
    uint32_t l = 0;
    if (offsets) {
        l = first_list_of_block(offsets, n_lists, p0, &first_list);
        if (in_range) l = advance_list(offsets, n_lists, l, p);
    } else if (in_range) {
        l = p / per_list;
    }
    const uint32_t id = in_range ? ids[p] : 0xFFFFFFFFu;
    const bool valid = id < count;
    const uint32_t n_here = n_pairs - min(n_pairs, p0 + (uint32_t)wave * 64u);  // pairs at or after the wave's first
    const int last_lane = n_here >= 64 ? 63 : (n_here ? (int)n_here - 1 : 0);
    const uint32_t l_first = (uint32_t)__shfl((int)l, 0, 64), l_last = (uint32_t)__shfl((int)l, last_lane, 64);
    const bool one_query = l_first == l_last;
    const float *__restrict__ q_wave = queries + (size_t)__builtin_amdgcn_readfirstlane((int)l_first) * dim;
    const float *__restrict__ q_lane = queries + (size_t)l * dim;

    // lane j loads the packed pair (2 * (j & 31), + 1) of the rows 2i + (j >> 5), i = 0..31
    const int col = lane & 31, half = lane >> 5;
    uint32_t row_id[kSeg];
#pragma unroll
    for (int i = 0; i < kSeg; i++) row_id[i] = (uint32_t)__shfl((int)id, 2 * i + half, 64);
    uint32_t next[kSeg];
    auto load_segment = [&](uint32_t d0) {
        const uint32_t d = d0 + 2u * (uint32_t)col;
#pragma unroll
        for (int i = 0; i < kSeg; i++) {
            const size_t at = (size_t)row_id[i] * dim + d;
            uint32_t w = 0;
            if (row_id[i] < count && d + 1 < dim) {  // a pair inside the row; the last value of an odd dim is `last`
                if (ALIGNED) w = reinterpret_cast<const uint32_t *>(data)[at >> 1];  // dim and d are even: so is `at`
                else __builtin_memcpy(&w, data + at, 4);  // one dword load at a 2-byte aligned address
            }
            next[i] = w;
        }
    };
    // odd dim: the row's last value has no partner; its lane loads it once
    const float last = (valid && (dim & 1u)) ? widen_lo<DTYPE>(data[(size_t)id * dim + (dim - 1)]) : 0.0f;
    float sum = 0.0f;
    // the n values from d0 on, in the row's order: low half, then high half of each packed dword
    auto add_terms = [&](const float *__restrict__ q, const uint32_t *mine, uint32_t d0, uint32_t n) {
        uint32_t c = 0;
        for (; c + 1 < n; c += 2) {
            const uint32_t w = mine[c >> 1];
            sum += term<METRIC>(q[d0 + c], widen_lo<DTYPE>(w));
            sum += term<METRIC>(q[d0 + c + 1], widen_hi<DTYPE>(w));
        }
        if (c < n) sum += term<METRIC>(q[d0 + c], last);  // n is odd only at the end of a row of odd dim
    };
    load_segment(0);
    for (uint32_t d0 = 0; d0 < dim; d0 += kHalfSeg) {
#pragma unroll
        for (int i = 0; i < kSeg; i++) tile[(2 * i + half) * kTileStride + col] = next[i];
        __syncthreads();
        if (d0 + kHalfSeg < dim) load_segment(d0 + kHalfSeg);
        const uint32_t *mine = tile + lane * kTileStride;
        const uint32_t n = min((uint32_t)kHalfSeg, dim - d0);
        if (one_query) {
            if (n == kHalfSeg) {
#pragma unroll
                for (int c = 0; c < kSeg; c++) {
                    const uint32_t w = mine[c];
                    sum += term<METRIC>(q_wave[d0 + 2 * c], widen_lo<DTYPE>(w));
                    sum += term<METRIC>(q_wave[d0 + 2 * c + 1], widen_hi<DTYPE>(w));
                }
            } else {
                add_terms(q_wave, mine, d0, n);
            }
        } else if (in_range) {
            add_terms(q_lane, mine, d0, n);
        }
        __syncthreads();
    }
    if (in_range) out[p] = valid ? (invert ? -sum : sum) : __builtin_nanf("");
}

// f32 -> f16 / bf16: round to nearest even, overflow to +-inf, NaN stays NaN, subnormal results kept.
template <int DTYPE> __device__ __forceinline__ uint32_t narrow(float x) {
    if (DTYPE == QAMD_DTYPE_F16) return __builtin_bit_cast(uint16_t, (_Float16)x);  // v_cvt_f16_f32 in the default mode
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x0040u;  // a NaN whose payload sits in the low bits stays one
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                    // the carry out of the mantissa is the overflow to inf
}

// dst[i] = narrow(src[i]), i < n.  VEC: src is 16-byte and dst 8-byte aligned.
template <int DTYPE, bool VEC>
__global__ __launch_bounds__(kBlock) void narrow_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t done = 0;
    if (VEC) {
        const uint64_t n4 = n / 4;
        for (uint64_t i = t; i < n4; i += stride) {
            const float4 v = reinterpret_cast<const float4 *>(src)[i];
            uint2 o;
            o.x = narrow<DTYPE>(v.x) | (narrow<DTYPE>(v.y) << 16);
            o.y = narrow<DTYPE>(v.z) | (narrow<DTYPE>(v.w) << 16);
            reinterpret_cast<uint2 *>(dst)[i] = o;
        }
        done = n4 * 4;
    }
    for (uint64_t i = done + t; i < n; i += stride) dst[i] = (uint16_t)narrow<DTYPE>(src[i]);
}

qamd_status narrow_launch(const float *src, uint16_t *dst, uint64_t n, qamd_dtype to, hipStream_t s) {
    if (n == 0) return QAMD_OK;
    const bool vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 8 == 0;
    const uint64_t per_block = (uint64_t)kBlock * (vec ? 4 : 1);
    const unsigned grid = (unsigned)std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)device_info().cu_count * 16);
#define QAMD_NARROW_GO(T, V) hipLaunchKernelGGL((narrow_kernel<T, V>), dim3(grid), dim3(kBlock), 0, s, src, dst, n)
    if (to == QAMD_DTYPE_F16) {
        if (vec) QAMD_NARROW_GO(QAMD_DTYPE_F16, true);
        else QAMD_NARROW_GO(QAMD_DTYPE_F16, false);
    } else {
        if (vec) QAMD_NARROW_GO(QAMD_DTYPE_BF16, true);
        else QAMD_NARROW_GO(QAMD_DTYPE_BF16, false);
    }
#undef QAMD_NARROW_GO
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

template <int DTYPE>
void half_pairs_go(const qamd_f32 *h, unsigned grid, const float *queries_dev, const uint32_t *offsets, uint32_t n_lists,
                   uint32_t per_list, const uint32_t *ids_dev, uint32_t n_pairs, float *out_dev, hipStream_t s) {
    const bool aligned = h->vp.dim % 2 == 0 && reinterpret_cast<uintptr_t>(h->data) % 4 == 0;
#define QAMD_HALF_GO(M, A)                                                                                              \
    hipLaunchKernelGGL((half_pairs_kernel<M, DTYPE, A>), dim3(grid), dim3(kBlock), 0, s,                                \
                       static_cast<const uint16_t *>(h->data), (uint32_t)h->vp.dim, (uint32_t)h->vp.count, queries_dev, \
                       offsets, n_lists, per_list, ids_dev, n_pairs, (int)(h->vp.invert != 0), out_dev)
#define QAMD_HALF_GO_M(M)              \
    do {                               \
        if (aligned) QAMD_HALF_GO(M, true); \
        else QAMD_HALF_GO(M, false);   \
    } while (0)
    if (h->vp.distance_type == QAMD_DOT) QAMD_HALF_GO_M(QAMD_DOT);
    else if (h->vp.distance_type == QAMD_L1) QAMD_HALF_GO_M(QAMD_L1);
    else QAMD_HALF_GO_M(QAMD_L2);
#undef QAMD_HALF_GO_M
#undef QAMD_HALF_GO
}

qamd_status pairs_launch(const qamd_f32 *h, const float *queries_dev, const uint32_t *offsets, uint32_t n_lists,
                         uint32_t per_list, const uint32_t *ids_dev, uint64_t n_pairs, float *out_dev, hipStream_t s) {
    if (n_pairs == 0) return QAMD_OK;
    const unsigned grid = (unsigned)((n_pairs + kBlock - 1) / kBlock);
    if (h->dtype != QAMD_DTYPE_F32) {
        if (h->dtype == QAMD_DTYPE_F16)
            half_pairs_go<QAMD_DTYPE_F16>(h, grid, queries_dev, offsets, n_lists, per_list, ids_dev, (uint32_t)n_pairs, out_dev, s);
        else
            half_pairs_go<QAMD_DTYPE_BF16>(h, grid, queries_dev, offsets, n_lists, per_list, ids_dev, (uint32_t)n_pairs, out_dev, s);
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
#define QAMD_F32_GO(M)                                                                                                  \
    hipLaunchKernelGGL(f32_pairs_kernel<M>, dim3(grid), dim3(kBlock), 0, s, static_cast<const float *>(h->data),        \
                       (uint32_t)h->vp.dim, (uint32_t)h->vp.count, queries_dev, offsets, n_lists, per_list, ids_dev,    \
                       (uint32_t)n_pairs, (int)(h->vp.invert != 0), out_dev)
    if (h->vp.distance_type == QAMD_DOT) QAMD_F32_GO(QAMD_DOT);
    else if (h->vp.distance_type == QAMD_L1) QAMD_F32_GO(QAMD_L1);
    else QAMD_F32_GO(QAMD_L2);
#undef QAMD_F32_GO
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

qamd_status check_queries(const qamd_f32 *h, const float *queries, uint64_t qdim) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (!queries) return fail(QAMD_ERR_ARGUMENTS, "query is null");
    if (qdim != h->vp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "query has %llu values, the vectors have %llu", (unsigned long long)qdim,
                    (unsigned long long)h->vp.dim);
    return QAMD_OK;
}

// n_rows <= count: what every null-list form checks before its first launch.
qamd_status check_prefix(const qamd_f32 *h, uint64_t n_rows) {
    if (n_rows > h->vp.count)
        return fail(QAMD_ERR_OUT_OF_RANGE, "rows 0 .. %llu asked for, the store has %llu", (unsigned long long)n_rows,
                    (unsigned long long)h->vp.count);
    return QAMD_OK;
}

// Queries of a batch that share one pass over the rows and one score workspace of group * n_rows * 4 bytes: 8, or as
// many as keep that workspace within kScanScoreCap, and at least 1.
uint32_t scan_group(uint64_t n_queries, uint64_t n_rows) {
    const uint64_t fit = kScanScoreCap / (std::max<uint64_t>(n_rows, 1) * 4);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({8, n_queries, fit}));
}

// The re-rank entry points with a null id list: the k best of the rows 0 .. n_rows - 1 for every query, by one scan of
// the rows per group of queries (f32_scan.hip) and the exact radix select over the group's scores.
qamd_status rerank_scan(const qamd_f32 *h, const float *queries, uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                        uint32_t n_rows, uint32_t k, int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                        hipStream_t s) {
    QAMD_TRY(check_queries(h, queries, qdim));
    QAMD_TRY(check_prefix(h, n_rows));
    if (n_queries > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 queries per call");
    QAMD_ON_DEVICE(h->device);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(queries, n_queries * qdim, queries_mem, qstage, s, &q_dev));
    if (n_queries == 1)
        return topk_classic(n_rows, k, largest, out_ids, out_scores, out_mem, s,
                            [&](float *scores) { return f32_scan_launch(h, q_dev, 1, n_rows, scores, n_rows, s); });
    const uint32_t group = scan_group(n_queries, n_rows);
    const size_t n_out = (size_t)n_queries * k;
    StreamBuf res;  // host outputs: results are assembled on the device, one download at the end
    uint32_t *ids_dev = out_ids;
    float *sc_dev = out_scores;
    if (out_mem == QAMD_MEM_HOST) {
        QAMD_TRY(res.alloc(n_out * 8, s));
        ids_dev = res.as<uint32_t>();
        sc_dev = reinterpret_cast<float *>(ids_dev + n_out);
    }
    float *scores = nullptr;
    QAMD_TRY(thread_ws_acquire(WS_SCORES, (size_t)group * n_rows * 4, s, reinterpret_cast<void **>(&scores)));
    void *sel = nullptr;
    qamd_status st = thread_ws_acquire(WS_SELECT, round_up(topk_workspace_bytes(k), 256), s, &sel);
    if (st != QAMD_OK) {
        thread_ws_release(WS_SCORES, s);
        return st;
    }
    for (uint64_t q0 = 0; q0 < n_queries && st == QAMD_OK; q0 += group) {  // the score workspace is reused in stream order
        const uint32_t g = (uint32_t)std::min<uint64_t>(group, n_queries - q0);
        st = f32_scan_launch(h, q_dev + q0 * qdim, g, n_rows, scores, n_rows, s);
        for (uint32_t j = 0; j < g && st == QAMD_OK; j++)
            st = topk_f32(scores + (size_t)j * n_rows, n_rows, k, largest != 0, ids_dev + (q0 + j) * k, sc_dev + (q0 + j) * k, sel, s);
    }
    bool synced = false;
    if (st == QAMD_OK && out_mem == QAMD_MEM_HOST) {
        std::vector<uint32_t> host(2 * n_out);
        st = copy_out(host.data(), QAMD_MEM_HOST, ids_dev, n_out * 8, s);  // synchronises `s`
        if (st == QAMD_OK) {
            memcpy(out_ids, host.data(), n_out * 4);
            memcpy(out_scores, host.data() + n_out, n_out * 4);
            synced = true;
        }
    }
    thread_ws_release(WS_SELECT, s, synced);
    thread_ws_release(WS_SCORES, s, synced);
    return st;
}

// The re-rank entry points: ids [n_queries][n_ids] from the caller, host or device.
qamd_status rerank_any(const qamd_f32 *h, const float *queries, uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                       const uint32_t *ids, uint32_t n_ids, qamd_mem ids_mem, uint32_t k, int largest, uint32_t *out_ids,
                       float *out_scores, qamd_mem out_mem, hipStream_t s) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (k == 0 || n_queries == 0) return QAMD_OK;
    if (k > 1024) return fail(QAMD_ERR_ARGUMENTS, "rerank: k=%u exceeds 1024", k);
    if (ids && n_ids > kRerankMaxIds)  // what one candidate sort takes; the scan of a null list has no such limit
        return fail(QAMD_ERR_ARGUMENTS, "rerank: %u ids per query exceed %u", n_ids, kRerankMaxIds);
    if (!out_ids || !out_scores) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (!ids && n_ids)  // a null list stands for the rows 0 .. n_ids - 1
        return rerank_scan(h, queries, n_queries, qdim, queries_mem, n_ids, k, largest, out_ids, out_scores, out_mem, s);
    QAMD_TRY(check_queries(h, queries, qdim));
    const uint64_t n_pairs = n_queries * n_ids;
    if (n_pairs > 0xFFFFFFFFull || n_queries > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 ids per call");
    if (ids_mem == QAMD_MEM_HOST)
        for (uint64_t p = 0; p < n_pairs; p++)
            if (ids[p] != kRerankPad && ids[p] >= h->vp.count)
                return fail(QAMD_ERR_OUT_OF_RANGE, "row id %u out of range (count %llu)", ids[p], (unsigned long long)h->vp.count);
    QAMD_ON_DEVICE(h->device);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(queries, n_queries * qdim, queries_mem, qstage, s, &q_dev));
    const size_t off_rerank = ids_mem == QAMD_MEM_HOST ? round_up(n_pairs * 4, 256) : 0;
    char *ws = nullptr;
    QAMD_TRY(thread_ws_acquire(WS_RESCORE, off_rerank + rerank_ws_bytes((uint32_t)n_queries, n_ids, k, out_mem), s,
                               reinterpret_cast<void **>(&ws)));
    const uint32_t *ids_dev = ids;
    qamd_status st = QAMD_OK;
    if (ids_mem == QAMD_MEM_HOST) {
        st = copy_in(ws, ids, QAMD_MEM_HOST, n_pairs * 4, s);
        ids_dev = reinterpret_cast<const uint32_t *>(ws);
    }
    if (st == QAMD_OK)
        st = rerank_device(h, q_dev, (uint32_t)n_queries, ids_dev, n_ids, ws + off_rerank, k, largest, out_ids, out_scores,
                           out_mem, s);
    thread_ws_release(WS_RESCORE, s, st == QAMD_OK && out_mem == QAMD_MEM_HOST);  // the download synchronised the stream
    return st;
}

}  // namespace

qamd_status rescore_queries_view(const float *queries, uint64_t n_floats, qamd_mem mem, StreamBuf &stage, hipStream_t s,
                                 const float **out) {
    *out = queries;
    if (mem == QAMD_MEM_DEVICE || n_floats == 0) return QAMD_OK;
    QAMD_TRY(stage.alloc(n_floats * 4, s));
    QAMD_TRY(copy_in(stage.ptr, queries, QAMD_MEM_HOST, n_floats * 4, s));
    *out = stage.as<float>();
    return QAMD_OK;
}

qamd_status rerank_device(const qamd_f32 *orig, const float *queries_dev, uint32_t n_queries, const uint32_t *ids_dev,
                          uint32_t n_ids, void *ws, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                          qamd_mem out_mem, hipStream_t s) {
    float *scores = static_cast<float *>(ws);
    const size_t n_out = (size_t)n_queries * k;
    uint32_t *ids_out = out_ids;
    float *sc_out = out_scores;
    if (out_mem == QAMD_MEM_HOST) {  // ids, then scores: one download
        ids_out = reinterpret_cast<uint32_t *>(static_cast<char *>(ws) + round_up((size_t)n_queries * n_ids * 4, 256));
        sc_out = reinterpret_cast<float *>(ids_out + n_out);
    }
    QAMD_TRY(pairs_launch(orig, queries_dev, nullptr, n_queries, n_ids, ids_dev, (uint64_t)n_queries * n_ids, scores, s));
    QAMD_TRY(rerank_sort_emit(ids_dev, scores, n_queries, n_ids, k, largest, ids_out, sc_out, s));
    if (out_mem == QAMD_MEM_HOST) {
        std::vector<uint32_t> host(2 * n_out);
        QAMD_TRY(copy_out(host.data(), QAMD_MEM_HOST, ids_out, n_out * 8, s));
        memcpy(out_ids, host.data(), n_out * 4);
        memcpy(out_scores, host.data() + n_out, n_out * 4);
    }
    return QAMD_OK;
}

}  // namespace qamd

using namespace qamd;

namespace {

size_t dtype_size(qamd_dtype t) { return t == QAMD_DTYPE_F32 ? 4 : 2; }
const char *dtype_name(qamd_dtype t) { return t == QAMD_DTYPE_F32 ? "f32" : t == QAMD_DTYPE_F16 ? "f16" : "bf16"; }
bool dtype_known(qamd_dtype t) { return t == QAMD_DTYPE_F32 || t == QAMD_DTYPE_F16 || t == QAMD_DTYPE_BF16; }

// The originals of a store: `distance_type` and `invert` of `vp` fix what a score is - DistanceType::distance
// (encoded_vectors.rs:37-45) of (query, row widened to f32), negated for invert: the quantity every quantizer's score
// approximates.  `data` holds `data_dtype` values; the handle keeps `store_dtype`.
qamd_status from_data_any(const void *data, qamd_dtype data_dtype, qamd_mem data_mem, const qamd_vector_parameters *vp,
                          qamd_dtype store_dtype, int borrow, void *stream, qamd_f32 **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    *out = nullptr;
    if (vp->distance_type != QAMD_DOT && vp->distance_type != QAMD_L1 && vp->distance_type != QAMD_L2)
        return fail(QAMD_ERR_ARGUMENTS, "unknown distance type %d", (int)vp->distance_type);
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 vectors");  // 0xFFFFFFFF is the padding id
    if (vp->dim > 0x7FFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^31 - 1 dimensions");
    if (!dtype_known(data_dtype) || !dtype_known(store_dtype))
        return fail(QAMD_ERR_ARGUMENTS, "unknown element type (data %d, store %d)", (int)data_dtype, (int)store_dtype);
    if (data_dtype != store_dtype && data_dtype != QAMD_DTYPE_F32)
        return fail(QAMD_ERR_ARGUMENTS, "%s data cannot be kept as %s: only f32 data is converted", dtype_name(data_dtype),
                    dtype_name(store_dtype));
    const uint64_t n = vp->count * vp->dim;
    if (n && !data) return fail(QAMD_ERR_ARGUMENTS, "data is null");
    if (borrow && data_mem != QAMD_MEM_DEVICE)
        return fail(QAMD_ERR_ARGUMENTS, "only device memory can be borrowed: host originals are copied (borrow = 0)");
    if (borrow && data_dtype != store_dtype)
        return fail(QAMD_ERR_ARGUMENTS, "borrowed %s data cannot be kept as %s: a borrowed buffer is read in place",
                    dtype_name(data_dtype), dtype_name(store_dtype));
    const size_t esize = dtype_size(store_dtype);
    if (borrow && reinterpret_cast<uintptr_t>(data) % esize)
        return fail(QAMD_ERR_ARGUMENTS, "borrowed %s data must be aligned to %zu bytes", dtype_name(store_dtype), esize);
    const int device = current_device();
    QAMD_ON_DEVICE(device);
    if (borrow && n) {
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, data) != hipSuccess) {
            (void)hipGetLastError();
            return fail(QAMD_ERR_ARGUMENTS, "borrowed data is not device memory");
        }
        if (attr.type != hipMemoryTypeDevice || attr.device != device)
            return fail(QAMD_ERR_ARGUMENTS, "borrowed data must be device memory of the current device (%d)", device);
    }
    std::unique_ptr<qamd_f32> h(new qamd_f32);
    h->device = device;
    h->vp = *vp;
    h->dtype = store_dtype;
    if (borrow) {
        h->data = data;
    } else {
        hipStream_t s = as_stream(stream);
        QAMD_TRY(h->owned.alloc(std::max<uint64_t>(n, 1) * esize));
        if (data_dtype == store_dtype) {
            QAMD_TRY(copy_in(h->owned.ptr, data, data_mem, n * esize, s));
        } else if (n) {  // narrowed on the device, piece by piece: pieces of a multiple of 4 rows keep the 8-byte stores
            uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / (vp->dim * 4));
            if (piece_rows > 4) piece_rows -= piece_rows % 4;
            DevBuf stage;
            uint16_t *dst = h->owned.as<uint16_t>();
            QAMD_TRY(for_each_staged_piece(static_cast<const float *>(data), data_mem, vp->count, vp->dim, piece_rows, stage, s,
                                           [&](const float *src, uint64_t first_row, uint64_t nr) {
                                               return narrow_launch(src, dst + first_row * vp->dim, nr * vp->dim, store_dtype, s);
                                           }));
        }
        // the caller may free its copy on return, and `stage` goes out of scope
        if (data_mem == QAMD_MEM_DEVICE || data_dtype != store_dtype) QAMD_HIP(hipStreamSynchronize(s));
        h->data = h->owned.ptr;
    }
    h->capacity = vp->count;
    *out = h.release();
    return QAMD_OK;
}

// upsert: room for `cap` rows of an owned store.  No kernel reads past row count, so the tail is only kept
// zero for the sake of one rule for all four stores.
qamd_status f32_grow(qamd_f32 *h, uint64_t cap) {
    if (cap <= h->capacity) return QAMD_OK;
    const uint64_t row_bytes = h->vp.dim * dtype_size(h->dtype);
    DevBuf rows;
    QAMD_TRY(grow_copy(h->owned, std::max<uint64_t>(padded_rows_of(cap) * row_bytes, 1), h->vp.count * row_bytes, rows));
    h->owned = std::move(rows);  // (the old buffer goes through hipFree, which waits for the device)
    h->data = h->owned.ptr;
    h->capacity = cap;
    return QAMD_OK;
}

qamd_status check_owned(const qamd_f32 *h) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (!h->owned.ptr) return fail(QAMD_ERR_ARGUMENTS, "a borrowed store cannot be written: its buffer is the caller's");
    return QAMD_OK;
}

}  // namespace

extern "C" {

qamd_status qamd_f32_from_data(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp, int borrow,
                               void *stream, qamd_f32 **out) {
    return from_data_any(data, QAMD_DTYPE_F32, data_mem, vp, QAMD_DTYPE_F32, borrow, stream, out);
}

qamd_status qamd_f32_from_data_typed(const void *data, qamd_dtype data_dtype, qamd_mem data_mem,
                                     const qamd_vector_parameters *vp, qamd_dtype store_dtype, int borrow, void *stream,
                                     qamd_f32 **out) {
    return from_data_any(data, data_dtype, data_mem, vp, store_dtype, borrow, stream, out);
}

qamd_status qamd_f32_get_dtype(const qamd_f32 *h, qamd_dtype *out) {
    if (!h || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    *out = h->dtype;
    return QAMD_OK;
}

qamd_status qamd_f32_get_parameters(const qamd_f32 *h, qamd_vector_parameters *out) {
    if (!h || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    *out = h->vp;
    return QAMD_OK;
}

void qamd_f32_free(qamd_f32 *h) { delete h; }

qamd_status qamd_f32_score_ids(const qamd_f32 *h, const float *query, uint64_t qdim, qamd_mem query_mem, const uint32_t *ids,
                               uint64_t n_ids, qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream) {
    QAMD_TRY(check_queries(h, query, qdim));
    if (n_ids == 0) return QAMD_OK;
    if (!out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (!ids) QAMD_TRY(check_prefix(h, n_ids));  // a null list stands for the rows 0 .. n_ids - 1
    if (n_ids > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 ids per call");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(query, qdim, query_mem, qstage, s, &q_dev));
    if (!ids) {  // the whole-store scan: no id array, the rows in order (f32_scan.hip)
        auto scan = [&](float *out_dev) { return f32_scan_launch(h, q_dev, 1, n_ids, out_dev, n_ids, s); };
        return out_mem == QAMD_MEM_DEVICE ? scan(out) : score_all_to_host(n_ids, out, s, scan);
    }
    return run_ids(ids, n_ids, ids_mem, out, out_mem, h->vp.count, s, [&](const uint32_t *ids_dev, uint64_t n, float *out_dev) {
        return pairs_launch(h, q_dev, nullptr, 1, (uint32_t)n, ids_dev, n, out_dev, s);
    });
}

qamd_status qamd_f32_score_ids_batch(const qamd_f32 *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                     qamd_mem queries_mem, const uint32_t *list_offsets, uint32_t n_lists,
                                     const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem, float *out, qamd_mem out_mem,
                                     void *stream) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (n_lists > n_queries)
        return fail(QAMD_ERR_ARGUMENTS, "%u lists, but there are %llu queries", n_lists, (unsigned long long)n_queries);
    if (n_lists == 0 || n_ids == 0) return QAMD_OK;
    QAMD_TRY(check_queries(h, queries, qdim));
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(queries, (uint64_t)n_lists * qdim, queries_mem, qstage, s, &q_dev));
    return run_lists(list_offsets, n_lists, ids, n_ids, nullptr, lists_mem, out, out_mem, h->vp.count, s, [&](const ListArgs &a) {
        return pairs_launch(h, q_dev, a.offsets, a.n_lists, 0, a.ids, a.n_pairs, a.out, s);
    });
}

qamd_status qamd_f32_rerank(const qamd_f32 *h, const float *query, uint64_t qdim, qamd_mem query_mem, const uint32_t *ids,
                            uint32_t n_ids, qamd_mem ids_mem, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                            qamd_mem out_mem, void *stream) {
    return rerank_any(h, query, 1, qdim, query_mem, ids, n_ids, ids_mem, k, largest, out_ids, out_scores, out_mem,
                      as_stream(stream));
}

qamd_status qamd_f32_rerank_batch(const qamd_f32 *h, const float *queries, uint64_t n_queries, uint64_t qdim,
                                  qamd_mem queries_mem, const uint32_t *ids, uint32_t n_ids, qamd_mem ids_mem, uint32_t k,
                                  int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream) {
    return rerank_any(h, queries, n_queries, qdim, queries_mem, ids, n_ids, ids_mem, k, largest, out_ids, out_scores, out_mem,
                      as_stream(stream));
}

uint64_t qamd_f32_capacity(const qamd_f32 *h) { return h ? (h->owned.ptr ? h->capacity : h->vp.count) : 0; }

qamd_status qamd_f32_reserve(qamd_f32 *h, uint64_t capacity_rows, void *stream) {
    QAMD_TRY(check_owned(h));
    if (capacity_rows > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 vectors");
    if (capacity_rows <= h->capacity) return QAMD_OK;
    QAMD_ON_DEVICE(h->device);
    QAMD_HIP(hipStreamSynchronize(as_stream(stream)));
    return f32_grow(h, capacity_rows);
}

// Rows [first_row, first_row + n_rows) of an owned store become `data` (the store's element type, or f32 narrowed to it
// as in qamd_f32_from_data_typed); rows past the end extend it.
qamd_status qamd_f32_upsert(qamd_f32 *h, uint64_t first_row, const void *data, qamd_dtype data_dtype, qamd_mem data_mem,
                            uint64_t n_rows, void *stream) {
    QAMD_TRY(check_owned(h));
    const uint64_t dim = h->vp.dim;
    QAMD_TRY(check_upsert(first_row, n_rows, h->vp.count, data, dim));
    if (!dtype_known(data_dtype)) return fail(QAMD_ERR_ARGUMENTS, "unknown element type (data %d)", (int)data_dtype);
    if (data_dtype != h->dtype && data_dtype != QAMD_DTYPE_F32)
        return fail(QAMD_ERR_ARGUMENTS, "%s data cannot be kept as %s: only f32 data is converted", dtype_name(data_dtype),
                    dtype_name(h->dtype));
    if (n_rows == 0) return QAMD_OK;
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    const uint64_t end = first_row + n_rows;
    if (end > h->capacity) {
        QAMD_HIP(hipStreamSynchronize(s));
        QAMD_TRY(f32_grow(h, std::min<uint64_t>(upsert_capacity(end, h->capacity), 0xFFFFFFFFull)));
    }
    const size_t esize = dtype_size(h->dtype);
    char *dst = h->owned.as<char>() + first_row * dim * esize;
    if (data_dtype == h->dtype) {
        QAMD_TRY(copy_in(dst, data, data_mem, n_rows * dim * esize, s));
    } else if (dim) {  // narrowed on the device, piece by piece (from_data_any)
        uint64_t piece_rows = std::max<uint64_t>(1, stage_bytes(256ull << 20) / (dim * 4));
        if (piece_rows > 4) piece_rows -= piece_rows % 4;
        DevBuf stage;
        QAMD_TRY(for_each_staged_piece(static_cast<const float *>(data), data_mem, n_rows, dim, piece_rows, stage, s,
                                       [&](const float *src, uint64_t r, uint64_t nr) {
                                           return narrow_launch(src, reinterpret_cast<uint16_t *>(dst) + r * dim, nr * dim, h->dtype, s);
                                       }));
    }
    QAMD_HIP(hipStreamSynchronize(s));
    h->vp.count = std::max(h->vp.count, end);
    return QAMD_OK;
}

}  // extern "C"
