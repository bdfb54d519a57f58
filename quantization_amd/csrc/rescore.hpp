// Rescoring with the original vectors, kept as f32, f16 or bf16 (f32.hip): the store of originals, the device-side
// re-rank that the fused calls feed, and the one body of qamd_{u8,pq,bin}_topk_rescored / _topk_batch_rescored.
//
// The caller of the reference over-fetches from the quantized scan and scores the candidates again with
// DistanceType::distance (quantization/src/encoded_vectors.rs:37-45) on the original vectors
// (demos/src/ann_benchmark_data.rs:151-185 measures exactly what that step recovers).
#pragma once

#include "common.hpp"
#include "topk_device.hpp"

// The originals: count x dim values of `dtype` (f32, or f16 / bf16 as 16-bit patterns), row-major, in HBM of
// `device`.  `data` is `owned.ptr` (borrow = 0) or the caller's pointer (borrow = 1: the caller keeps it alive).
struct qamd_f32 {
    int device = 0;
    qamd_vector_parameters vp{};
    qamd_dtype dtype = QAMD_DTYPE_F32;
    const void *data = nullptr;
    qamd::DevBuf owned;
    uint64_t capacity = 0;  // rows `owned` has room for: count after from_data, more after reserve / upsert
};

namespace qamd {

constexpr uint32_t kRerankMaxIds = kTopkCandCap;  // ids per query: what one LDS sort takes (topk.hip)
constexpr uint32_t kRerankPad = 0xFFFFFFFFu;      // the padding id of every top-k output: skipped
// The score workspace of a null-list qamd_f32_rerank_batch: the queries of one pass over the rows (up to 8) keep
// group * n_ids * 4 bytes of scores; the group shrinks, down to 1 query, so that this stays within the cap.
constexpr uint64_t kScanScoreCap = 512ull << 20;

// Exact best k of ids_dev[q][0..n_ids) for each of the n_queries queries (device memory, queries_dev
// [n_queries][dim]), by the exact score; outputs [n_queries][k] in host or device memory, ordering contract of
// the *_topk entry points.  `ws`: rerank_ws_bytes() of device scratch - the exact scores [n_queries][n_ids] first,
// then the staging of host outputs.  Host outputs are downloaded once (synchronises `s`); device outputs only enqueue.
inline size_t rerank_ws_bytes(uint32_t n_queries, uint32_t n_ids, uint32_t k, qamd_mem out_mem) {
    return round_up((size_t)n_queries * n_ids * 4, 256) + (out_mem == QAMD_MEM_HOST ? (size_t)n_queries * k * 8 : 0);
}
qamd_status rerank_device(const qamd_f32 *orig, const float *queries_dev, uint32_t n_queries, const uint32_t *ids_dev,
                          uint32_t n_ids, void *ws, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                          qamd_mem out_mem, hipStream_t s);

// The whole-store scan (f32_scan.hip): out_dev[q * pitch + row] = the exact score of query q and row `row`, for the
// n_queries queries at queries_dev [n_queries][dim] and the rows 0 .. n_rows - 1 (n_rows <= count, the caller's check).
// The rows are read once per 8 queries (a remainder in passes of 4, 2, 1).  Device memory; only enqueues on `s`.
qamd_status f32_scan_launch(const qamd_f32 *orig, const float *queries_dev, uint32_t n_queries, uint64_t n_rows, float *out_dev,
                            uint64_t pitch, hipStream_t s);

// `queries` ([n_queries][dim] f32, host or device) as device memory: used in place, or staged into `stage`.
qamd_status rescore_queries_view(const float *queries, uint64_t n_floats, qamd_mem mem, StreamBuf &stage, hipStream_t s,
                                 const float **out);

// qamd_{u8,pq,bin}_topk_rescored and _topk_batch_rescored: rerank(orig, queries_f32, ids of topk(h, q, candidates), k).
// `hvp`: the quantized store's vector parameters; `topk(ids_dev, scores_dev)` runs the store's existing *_topk /
// *_topk_batch with k = candidates and DEVICE outputs [n_queries][candidates] (it synchronises `s`).  The candidate
// ids never leave the device: they sit in the calling thread's rescoring workspace and feed the re-rank launches.
template <class Topk>
qamd_status topk_rescored(int device, const qamd_vector_parameters &hvp, const qamd_f32 *orig, const float *queries_f32,
                          uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem, uint32_t k, uint32_t candidates,
                          int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t s, Topk &&topk) {
    if (!orig) return fail(QAMD_ERR_ARGUMENTS, "topk_rescored: the store of original vectors is null");
    if (k == 0 || n_queries == 0) return QAMD_OK;
    if (k > candidates || candidates > 1024)
        return fail(QAMD_ERR_ARGUMENTS, "topk_rescored: need k <= candidates <= 1024, got k=%u candidates=%u", k, candidates);
    if (!queries_f32 || !out_ids || !out_scores) return fail(QAMD_ERR_ARGUMENTS, "null argument");
    const qamd_vector_parameters &ovp = orig->vp;
    if (ovp.count != hvp.count || ovp.dim != hvp.dim || ovp.distance_type != hvp.distance_type ||
        (ovp.invert != 0) != (hvp.invert != 0) || orig->device != device)
        return fail(QAMD_ERR_ARGUMENTS,
                    "topk_rescored: the originals (count %llu, dim %llu, distance %d, invert %d, device %d) do not belong "
                    "to this store (count %llu, dim %llu, distance %d, invert %d, device %d)",
                    (unsigned long long)ovp.count, (unsigned long long)ovp.dim, (int)ovp.distance_type, (int)ovp.invert,
                    orig->device, (unsigned long long)hvp.count, (unsigned long long)hvp.dim, (int)hvp.distance_type,
                    (int)hvp.invert, device);
    if (qdim != ovp.dim)
        return fail(QAMD_ERR_ARGUMENTS, "query has %llu values, the vectors have %llu", (unsigned long long)qdim,
                    (unsigned long long)ovp.dim);
    if (n_queries > 0xFFFFFFFFull / candidates) return fail(QAMD_ERR_ARGUMENTS, "topk_rescored: too many queries");
    QAMD_ON_DEVICE(device);
    StreamBuf qstage;
    const float *q_dev = nullptr;
    QAMD_TRY(rescore_queries_view(queries_f32, n_queries * qdim, queries_mem, qstage, s, &q_dev));
    const size_t n_cand = (size_t)n_queries * candidates;
    char *ws = nullptr;
    const size_t off_rerank = round_up(n_cand * 4, 256);
    QAMD_TRY(thread_ws_acquire(WS_RESCORE, off_rerank + rerank_ws_bytes((uint32_t)n_queries, candidates, k, out_mem), s,
                               reinterpret_cast<void **>(&ws)));
    uint32_t *cand_ids = reinterpret_cast<uint32_t *>(ws);
    float *cand_scores = reinterpret_cast<float *>(ws + off_rerank);  // the scan's scores; the exact ones replace them
    qamd_status st = topk(cand_ids, cand_scores);
    if (st == QAMD_OK)
        st = rerank_device(orig, q_dev, (uint32_t)n_queries, cand_ids, candidates, ws + off_rerank, k, largest, out_ids,
                           out_scores, out_mem, s);
    if (st == QAMD_OK && out_mem != QAMD_MEM_HOST && hipStreamSynchronize(s) != hipSuccess)
        st = fail(QAMD_ERR_DEVICE, "topk_rescored: stream synchronisation failed");
    thread_ws_release(WS_RESCORE, s, st == QAMD_OK);  // both ways out synchronised the stream
    return st;
}

}  // namespace qamd
