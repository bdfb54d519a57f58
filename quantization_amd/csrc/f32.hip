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
#include "rescore.hpp"

#include "lists.hpp"
#include "topk.hpp"

#include <memory>

namespace qamd {
namespace {

constexpr int kBlock = 256;      // 4 waves, each with its own tile
constexpr int kSeg = 32;         // values of a row per pass
constexpr int kTileStride = 33;  // dwords between two rows of a tile

template <int METRIC> __device__ __forceinline__ float term(float q, float v) {
    if (METRIC == QAMD_DOT) return q * v;
    const float d = q - v;
    return METRIC == QAMD_L1 ? __builtin_fabsf(d) : d * d;
}

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

qamd_status pairs_launch(const qamd_f32 *h, const float *queries_dev, const uint32_t *offsets, uint32_t n_lists,
                         uint32_t per_list, const uint32_t *ids_dev, uint64_t n_pairs, float *out_dev, hipStream_t s) {
    if (n_pairs == 0) return QAMD_OK;
    const unsigned grid = (unsigned)((n_pairs + kBlock - 1) / kBlock);
#define QAMD_F32_GO(M)                                                                                                  \
    hipLaunchKernelGGL(f32_pairs_kernel<M>, dim3(grid), dim3(kBlock), 0, s, h->data, (uint32_t)h->vp.dim,               \
                       (uint32_t)h->vp.count, queries_dev, offsets, n_lists, per_list, ids_dev, (uint32_t)n_pairs,      \
                       (int)(h->vp.invert != 0), out_dev)
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

// The re-rank entry points: ids [n_queries][n_ids] from the caller, host or device.
qamd_status rerank_any(const qamd_f32 *h, const float *queries, uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                       const uint32_t *ids, uint32_t n_ids, qamd_mem ids_mem, uint32_t k, int largest, uint32_t *out_ids,
                       float *out_scores, qamd_mem out_mem, hipStream_t s) {
    if (!h) return fail(QAMD_ERR_ARGUMENTS, "null handle");
    if (k == 0 || n_queries == 0) return QAMD_OK;
    if (k > 1024) return fail(QAMD_ERR_ARGUMENTS, "rerank: k=%u exceeds 1024", k);
    if (n_ids > kRerankMaxIds) return fail(QAMD_ERR_ARGUMENTS, "rerank: %u ids per query exceed %u", n_ids, kRerankMaxIds);
    if (!out_ids || !out_scores || (n_ids && !ids)) return fail(QAMD_ERR_ARGUMENTS, "null argument");
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

extern "C" {

// The originals of a store: `distance_type` and `invert` of `vp` fix what a score is - DistanceType::distance
// (encoded_vectors.rs:37-45) of (query, row), negated for invert: the quantity every quantizer's score approximates.
qamd_status qamd_f32_from_data(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp, int borrow,
                               void *stream, qamd_f32 **out) {
    if (!vp || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    *out = nullptr;
    if (vp->distance_type != QAMD_DOT && vp->distance_type != QAMD_L1 && vp->distance_type != QAMD_L2)
        return fail(QAMD_ERR_ARGUMENTS, "unknown distance type %d", (int)vp->distance_type);
    if (vp->count > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 vectors");  // 0xFFFFFFFF is the padding id
    if (vp->dim > 0x7FFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^31 - 1 dimensions");
    const uint64_t n = vp->count * vp->dim;
    if (n && !data) return fail(QAMD_ERR_ARGUMENTS, "data is null");
    if (borrow && data_mem != QAMD_MEM_DEVICE)
        return fail(QAMD_ERR_ARGUMENTS, "only device memory can be borrowed: host originals are copied (borrow = 0)");
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
    if (borrow) {
        h->data = data;
    } else {
        hipStream_t s = as_stream(stream);
        QAMD_TRY(h->owned.alloc(std::max<uint64_t>(n, 1) * 4));
        QAMD_TRY(copy_in(h->owned.ptr, data, data_mem, n * 4, s));
        if (data_mem == QAMD_MEM_DEVICE) QAMD_HIP(hipStreamSynchronize(s));  // the caller may free its copy on return
        h->data = h->owned.as<float>();
    }
    *out = h.release();
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
    if (!ids || !out) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    if (n_ids > 0xFFFFFFFFull) return fail(QAMD_ERR_ARGUMENTS, "at most 2^32 - 1 ids per call");
    QAMD_ON_DEVICE(h->device);
    hipStream_t s = as_stream(stream);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(query, qdim, query_mem, qstage, s, &q_dev));
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

}  // extern "C"
