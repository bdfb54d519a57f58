// Handle layouts of the scalar-u8 quantizer, shared by u8.hip (single-query path) and
// u8_batch.hip (multi-query MFMA path).  Not part of the C ABI.
#pragma once
#include <atomic>
#include <mutex>

#include "common.hpp"
#include "lists.hpp"

// The scan image of a store (qamd_u8::image): its format, its 16-byte chunks per row and the format's second kernel
// argument.  The kinds are what qamd_dev_u8_last_scan_packed reports.
enum : int { U8_IMAGE_NONE = 0, U8_IMAGE_7BIT = 1, U8_IMAGE_NIBBLE = 2 };
struct U8Image {
    int kind = U8_IMAGE_NONE;
    uint32_t chunks = 0, aux = 0;
};

namespace qamd {
[[noreturn]] void no_byte_codes();  // u8.hip: says what happened and aborts (qamd_u8::byte_codes)
}

struct qamd_u8 {
    int device = 0;
    qamd_u8_metadata meta{};
    uint64_t count = 0;
    uint64_t capacity = 0;     // rows there is room for: count after every builder, more after reserve / upsert
    uint64_t padded_rows = 0;  // round_up(capacity, 1024) + 1024; rows from count on are zero: tiles never need a load guard
    uint32_t row_chunks = 0;   // actual_dim / 16
    int lane_mode = 0;         // 0: integer sum rounded once; 1: avx2.c lane order
    // A rotated store: the rows are codes of the block rotation of what the caller handed in, and so are
    // the queries.  meta.vector_parameters.distance_type keeps the BASE metric (QAMD_DOT or QAMD_L2), so no kernel, route
    // or multiplier knows; QAMD_ROTATED is added back where metadata leaves the library (get_metadata).
    bool rotated = false;
    // A 4-bit store: the byte codes hold 0..15, alpha is a fifteenth of the interval and the encoders round
    // to nearest.  Like `rotated` it lives beside the base metric and goes back on in get_metadata; only the encoders,
    // the query encoders and build_packed read it - the scans see the image that build_packed left (image.kind).
    bool four_bit = false;
    // A compact 4-bit store: `codes` is never allocated; the store is `offsets` and the nibble image, which
    // every builder writes tile by tile through `stage`, and every route reads (u8.hip: the image scan, u8_nibble_pairs_kernel,
    // u8_nibble_unpack_kernel).  Like the two flags above it goes back onto the metric in get_metadata.
    bool compact = false;
    // The byte codes, for every kernel argument: the one place that hands the pointer out.  A compact store has none and
    // no route of it may ask (u8.hip routes by `compact` before it gets here), so a request is a routing bug: it stops on
    // the host, before a kernel can be launched on a null pointer.
    template <typename T> T *byte_codes() const {
        if (compact) qamd::no_byte_codes();
        return codes.as<T>();
    }
    qamd::DevBuf stage;        // compact builders: the byte codes of the tile in flight; released when a build or upsert ends
    qamd::DevBuf codes;        // [padded_rows][actual_dim]; a compact store: empty
    qamd::DevBuf offsets;      // [padded_rows] f32
    // Scan image (u8.hip build_packed), `image.chunks` 16-byte chunks per row in the format `image.kind`; u8.hip
    // u8_image_of is the one place that says which image a store can have and how long its rows are.
    //   U8_IMAGE_7BIT: the codes at 7 bits each.  Chunk j < chunks keeps chunk j's codes in bits 0..6 of its bytes and, in
    //     bit 7, bit plane j % 7 of chunk chunks + j / 7 (aux = row_chunks / 8 such chunks).
    //   U8_IMAGE_NIBBLE (4-bit stores; never both): chunks = ceil(row_chunks / 2), byte b of chunk j = codes[32 j + b] |
    //     codes[32 j + 16 + b] << 4 (high nibbles of the last chunk zero when row_chunks is odd); aux = row_chunks.
    // Rows lie in blocks of 64 (kPackBlockRows): chunk j of row r is at 16-byte index ((r / 64) * chunks + j) * 64 + r % 64,
    // so that chunk j of a block's 64 rows is one aligned kilobyte, which one wave of u8_scan_image_kernel loads.
    // padded_rows is a multiple of 1024: blocks are whole, and padding rows are zero.  Only the Dot / L2 scans of lane
    // mode 0 read it; every other kernel reads `codes`.  `packed` is empty and `image` is {} when the store has none (L1,
    // fewer than 8 - nibble: 2 - or more than 128 chunks, a code above 127 - nibble: 15 -, too little free HBM).
    // A compact store always has its nibble image (a build that cannot have one fails), and all its routes read it.
    qamd::DevBuf packed;
    U8Image image;
    mutable std::atomic<int> last_scan_packed{0};  // image.kind of the image the last scan launch read (developer report)
    mutable std::atomic<int> last_scan_split{0};   // waves per block of the last blocked scan launch (developer report)
    mutable qamd::DevBuf packed_rows;              // developer report: the image un-blocked, [count][image.chunks]
    // The batched top-k's pivot sample (u8_batch.hip): rows hash(j) of the store, j < sample_rows, then 512
    // zero rows; gathered on first use (count / 64 rows at most: 1.6 % of the store), discarded by an upsert.
    mutable std::mutex sample_mu;
    mutable qamd::DevBuf sample_codes, sample_offsets;
    mutable uint32_t sample_rows = 0;
};

struct qamd_u8_query {
    int device = 0;
    uint64_t actual_dim = 0;
    qamd::DevBuf buf;  // [0..4) offset f32, [16..16+actual_dim) codes
    mutable qamd::ReadyEvent ready;  // the last encode_query (stream order for consumers on other streams)
    // A HOST query of up to kFusedQueryDims values is not encoded by encode_query itself: its f32 values
    // wait here until the first consumer.  The single-launch top-k of a small store takes them BY VALUE in
    // its kernel arguments and quantises them in its prologue (one launch per search instead of two, no
    // PCIe read by the GPU); any other consumer runs the encode kernel first (u8.hip ensure_encoded).
    mutable std::vector<float> host_f32;
    float alpha = 0.0f, offset = 0.0f;  // of the store the query was (or will be) encoded for
    int distance = 0, invert = 0;
    bool rotated = false;  // of a rotated store: the values are rotated before they are encoded
    bool four_bit = false; // of a 4-bit store: 16 levels, rounded to nearest
    mutable std::atomic<bool> deferred{false};
    mutable std::mutex encode_mu;  // two threads may consume one deferred query
    bool pooled = false;     // buf came from / goes back to the query buffer cache
    mutable std::atomic<bool> async_used{false};  // a consumer call only ENQUEUED (device outputs)
    ~qamd_u8_query() {
        if (pooled) qamd::query_buf_put(buf, !async_used.load(std::memory_order_relaxed) && ready.complete());
    }
};

// Pass-1 pieces used by the sharded encoder; defined in u8.hip.
namespace qamd {
qamd_status u8_minmax_range(const float *data, qamd_mem mem, uint64_t n_rows, uint64_t dim, hipStream_t s, float *mn,
                            float *mx);
qamd_status u8_quantile_interval(const float *data, qamd_mem mem, uint64_t count, uint64_t dim, float quantile,
                                 hipStream_t s, bool *found, float *mn, float *mx);
}  // namespace qamd

// encode_query for one query per wave (device-resident f32 queries); defined in u8.hip.
namespace qamd {
qamd_status u8_encode_queries_device(const qamd_u8 *h, const float *queries_dev, uint64_t n_queries, uint64_t qdim,
                                     uint8_t *codes_dev /* [n][code_pitch], actual_dim written */, uint64_t code_pitch,
                                     float *offsets_dev /* [n] */,
                                     hipStream_t stream);
bool u8_host_encode_is_lazy(uint64_t qdim);  // encode_query(host query of qdim values) launches nothing
// A host query the single-launch top-k quantises itself (qamd_u8_query::host_f32) and where its codes go.
struct FusedQuery {
    const float *values = nullptr;
    uint32_t qdim = 0;
    uint8_t *qbuf = nullptr;
};
qamd_status u8_topk_ptrs(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, uint32_t k, int largest,
                         uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t stream,
                         const FusedQuery *fq = nullptr);
qamd_status u8_topk_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                uint32_t n_queries, uint32_t k, int largest, uint32_t *out_ids, float *out_scores,
                                qamd_mem out_mem, hipStream_t stream);
uint32_t u8_multi_width(const qamd_u8 *h);
bool u8_batch_by_scans(const qamd_u8 *h);  // lane mode 1 on Dot / L2, or a compact store: batches go query by query
qamd_status u8_score_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                 uint32_t n_queries, float *out_dev, hipStream_t stream);
qamd_status u8_score_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, float *out_dev,
                            hipStream_t stream);
qamd_status u8_score_lists(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                           const ListArgs &a, hipStream_t stream);
qamd_status u8_topk_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, uint32_t k,
                           int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t stream);
}  // namespace qamd
