// The scalar-u8 quantizer's internals, shared by u8_store.hip (what writes a store), u8.hip (what reads one: the
// single-query path), u8_batch.hip / u8_full_batch.hip (the multi-query MFMA paths) and sharded.hip: the handle layouts,
// the store's code format, the few host functions that cross a file boundary and, at the end, the device helpers that
// the writers and the readers of the codes and of the scan image both inline.  Not part of the C ABI.
#pragma once
#include <atomic>
#include <mutex>
#include <type_traits>

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
[[noreturn]] void no_byte_codes();  // u8_store.hip: says what happened and aborts (qamd_u8::byte_codes)
[[noreturn]] void no_signed_codes();  // u8_store.hip: the same for qamd_u8::codes_7bit
}

// The code format of a store: what a u8 constructor's distance_type carries beside the base metric (u8_store.hip
// split_distance).  meta.vector_parameters.distance_type keeps the BASE metric (QAMD_DOT, QAMD_L1 or QAMD_L2), so no
// kernel, route or multiplier knows; the flags go back on where metadata leaves the library (distance_bits).
struct U8Flags {
    // A rotated store: the rows are codes of the block rotation of what the caller handed in, and so are
    // the queries.
    bool rotated = false;
    // A 4-bit store: the byte codes hold 0..15, alpha is a fifteenth of the interval and the encoders round
    // to nearest.  Only the encoders, the query encoders and build_packed read it - the scans see the image that
    // build_packed left (image.kind).
    bool four_bit = false;
    // A compact 4-bit store: `codes` is never allocated; the store is `offsets` and the nibble image, which
    // every builder writes tile by tile through `stage`, and every route reads (u8.hip: the image scan,
    // u8_nibble_pairs_kernel; u8_store.hip: u8_nibble_unpack_kernel).
    bool compact = false;
    // A full-range store: the byte codes hold 0..255, alpha is a 255th of the interval and the encoders round
    // to nearest.  It keeps no scan image (u8_image_of).  The routes that read bytes with unsigned 32-bit arithmetic (scans,
    // pairs, the multi-query scan, the single-launch top-k, export) serve it as they are; batches beyond the multi-query
    // scan take u8_full_batch_kernel.
    bool full_range = false;
    // The code levels of the quantizer: 127 (the reference's truncating code), 15 or 255 (3.1w).
    int levels() const { return four_bit ? 15 : full_range ? 255 : 127; }
    // The flags as bits of a distance_type: what get_metadata adds to the base metric, and load hands to from_rows.
    int distance_bits() const {
        return (rotated ? QAMD_ROTATED : 0) | (four_bit ? QAMD_BITS4 : 0) | (compact ? QAMD_COMPACT : 0) |
               (full_range ? QAMD_FULL : 0);
    }
};

// The format is a base: its flags read as h->rotated, h->four_bit, h->compact and h->full_range on every route; a
// constructor sets all of them at once through format().
struct qamd_u8 : U8Flags {
    U8Flags &format() { return *this; }
    const U8Flags &format() const { return *this; }
    int device = 0;
    qamd_u8_metadata meta{};
    uint64_t count = 0;
    uint64_t capacity = 0;     // rows there is room for: count after every builder, more after reserve / upsert
    uint64_t padded_rows = 0;  // round_up(capacity, 1024) + 1024; rows from count on are zero: tiles never need a load guard
    uint32_t row_chunks = 0;   // actual_dim / 16
    int lane_mode = 0;         // 0: integer sum rounded once; 1: avx2.c lane order
    // The byte codes, for every kernel argument: the one place that hands the pointer out.  A compact store has none and
    // no route of it may ask (u8.hip routes by `compact` before it gets here), so a request is a routing bug: it stops on
    // the host, before a kernel can be launched on a null pointer.
    template <typename T> T *byte_codes() const {
        if (compact) qamd::no_byte_codes();
        return codes.as<T>();
    }
    // The byte codes for a kernel that assumes codes <= 127: a signed-operand route (every MFMA form of u8_batch.hip), the
    // 7-bit pack kernel, a lane-order kernel.  A full-range store must never get here - u8.hip / u8_batch.hip route by
    // `full_range` first - so a request is a routing bug: it stops on the host, before a kernel launch.
    template <typename T> T *codes_7bit() const {
        if (full_range) qamd::no_signed_codes();
        return byte_codes<T>();
    }
    qamd::DevBuf stage;        // compact builders: the byte codes of the tile in flight; released when a build or upsert ends
    qamd::DevBuf codes;        // [padded_rows][actual_dim]; a compact store: empty
    qamd::DevBuf offsets;      // [padded_rows] f32
    // Scan image (u8_store.hip build_packed), `image.chunks` 16-byte chunks per row in the format `image.kind`; u8_store.hip
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
    mutable std::atomic<int> last_scan_queries{0}; // queries the last blocked scan launch served (developer report)
    // queries the last u8_full_batch_kernel call served; 0 after a multi-query scan launch (developer report)
    mutable std::atomic<int> last_full_batch{0};
    // queries of the last topk_batch call that went through the kernel's filter form (0: the scans, or the score-block
    // route, served it), and how many of those were redone exactly (developer report)
    mutable std::atomic<int> last_full_filter{0}, last_full_redone{0};
    // The same three for u8_compact_batch_kernel: 0 when the image passes served the call.
    mutable std::atomic<int> last_compact_batch{0}, last_compact_filter{0}, last_compact_redone{0};
    mutable qamd::DevBuf packed_rows;              // developer report: the image un-blocked, [count][image.chunks]
    // The batched top-k's pivot sample (u8_batch.hip): rows hash(j) of the store, j < sample_rows, then 512
    // zero rows; gathered on first use (count / 64 rows at most: 1.6 % of the store), discarded by an upsert.
    // A compact store keeps the same rows as a small blocked nibble image of whole blocks (u8_compact_batch.hip).
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
    U8Flags fmt;  // of that store: a rotated store's queries are rotated before they are encoded, into fmt.levels() levels
    mutable std::atomic<bool> deferred{false};
    mutable std::mutex encode_mu;  // two threads may consume one deferred query
    bool pooled = false;     // buf came from / goes back to the query buffer cache
    mutable std::atomic<bool> async_used{false};  // a consumer call only ENQUEUED (device outputs)
    ~qamd_u8_query() {
        if (pooled) qamd::query_buf_put(buf, !async_used.load(std::memory_order_relaxed) && ready.complete());
    }
};

// Pass-1 pieces used by the sharded encoder, and the two launchers of u8_store.hip that the read side needs; defined in
// u8_store.hip.
namespace qamd {
// A number as a type: how a launcher of either file hands a run-time choice to a lambda that names a kernel instantiation.
template <int N> using Int = std::integral_constant<int, N>;
inline uint64_t actual_dim_of(uint64_t dim) { return dim + (16 - dim % 16) % 16; }  // encoded_vectors_u8.rs:257-259
// The scaled block rotation of n rows of dim f32 values, dim floats per row to `out`: what a rotated
// store's encoders quantize, for its queries and its quantile sample.  dim passed rot_dim_ok; src is device memory.
qamd_status u8_rot_values(const float *src, uint64_t n, uint64_t dim, float *out, hipStream_t s);
// Byte codes of image rows [r0, r0 + n) of a compact store or, with a device list, of rows[0 .. n): `pitch` bytes between
// out rows; q_offs (optional) gets the rows' stored offsets (u8_nibble_unpack_kernel).
qamd_status u8_unpack_rows(const qamd_u8 *h, const uint32_t *rows_dev, uint64_t r0, uint64_t n, uint8_t *out, uint64_t pitch,
                           float *q_offs, hipStream_t s);
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
// Lane mode 1 on Dot / L2: batches go query by query.  A compact store: up to 8 queries per pass over its nibble image
// (u8_scan_image_multi_kernel) below u8_compact_batch_min, u8_compact_batch_kernel from there on.
bool u8_batch_by_scans(const qamd_u8 *h);
// Full-range batches on the int8 matrix cores (u8_full_batch.hip): out[q * out_pitch + row] for queries
// [0, nq) ([q][q_pitch] byte codes, [q] offsets, device memory) against rows [0, n_rows) of the store, in passes of 15
// queries.  mode / diff: the epilogue (0: an encoded query, 1: score_internal's with `diff`).  Enqueues only.
qamd_status u8_full_batch_scores(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                 uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream);
// The pieces of it for topk_batch from the filter gate on, which builds the batch's query images once, in scratch of its
// own (u8_full_images_bytes of device memory), scores a gathered sample of the store with them and then filters the
// store: u8_full_batch_filter, one launch per pass of 15 queries, appends every (query, row) whose score is at least as
// good as the query's pivot to the per-query candidate lists of batch_common.hpp (counters: [q * 16], candidates:
// [q][kTopkCandCap], key << 32 | row).  actual_dim <= 8256 and a finite non-zero multiplier (u8_gemm_route.hpp).
struct U8FullImages {
    const uint4 *image = nullptr;  // [pass][nkb][64]
    const int *sums = nullptr;     // [pass][16]
    const float *offs = nullptr;   // [pass][16]
    uint32_t nq = 0, nkb = 0;
};
size_t u8_full_images_bytes(const qamd_u8 *h, uint32_t nq);
qamd_status u8_full_images_build(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                 void *scratch, hipStream_t stream, U8FullImages *out);
qamd_status u8_full_batch_scores_of(const qamd_u8 *h, const U8FullImages &im, const uint8_t *codes, const float *v_offsets,
                                    uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream);
qamd_status u8_full_batch_filter(const qamd_u8 *h, const U8FullImages &im, const float *pivot_scores, uint32_t *counters,
                                 unsigned long long *candidates, int largest, hipStream_t stream);
// Smallest batch the full-range matrix-core kernel takes (smaller ones stay on the multi-query scan).
uint32_t u8_full_batch_min(const qamd_u8 *h);
// Compact batches on the int8 matrix cores (u8_compact_batch.hip): the same pieces for a compact store, whose
// rows the kernel reads from the blocked nibble image, in passes of 16, 32 or 64 queries.  `rows` of _scores_of is such
// an image of whole blocks (the store's, or its pivot sample's) with its offsets.
struct U8CompactImages {
    const uint4 *image = nullptr;  // [pass] pass_stride uint4: [step][lo / hi][qt][64]
    const float *offs = nullptr;   // [pass][64]
    uint32_t nq = 0, nsteps = 0, passes = 0, qt_full = 0, qt_last = 0;  // tiles of 16 queries per pass, and of the last pass
    size_t pass_stride = 0;
};
size_t u8_compact_images_bytes(const qamd_u8 *h, uint32_t nq);
qamd_status u8_compact_images_build(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                    void *scratch, hipStream_t stream, U8CompactImages *out);
qamd_status u8_compact_batch_scores_of(const qamd_u8 *h, const U8CompactImages &im, const void *rows, const float *v_offsets,
                                       uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream);
qamd_status u8_compact_batch_scores(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                    uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream);
qamd_status u8_compact_batch_filter(const qamd_u8 *h, const U8CompactImages &im, const float *pivot_scores, uint32_t *counters,
                                    unsigned long long *candidates, int largest, hipStream_t stream);
// The pivot sample as a blocked nibble image (u8_nibble_gather_kernel): its bytes for `rows` sample rows, the gather into
// scratch of the caller's, and the handle's cached one (sample_mu), which serves every call as a prefix.
size_t u8_compact_sample_bytes(const qamd_u8 *h, uint32_t rows);
qamd_status u8_compact_sample_gather(const qamd_u8 *h, uint32_t rows, void *image, float *offsets, hipStream_t stream);
qamd_status u8_compact_sample_store(const qamd_u8 *h, uint32_t rows_all, hipStream_t s, const void **image, const float **offs);
// Smallest batch u8_compact_batch_kernel takes from this store; 0: none (not compact, L1, a multiplier that is zero or not
// finite, or the route switched off).  u8.hip, beside u8_batch_by_scans.
uint32_t u8_compact_batch_min(const qamd_u8 *h);
qamd_status u8_score_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                 uint32_t n_queries, float *out_dev, hipStream_t stream);
qamd_status u8_score_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, float *out_dev,
                            hipStream_t stream);
qamd_status u8_score_lists(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                           const ListArgs &a, hipStream_t stream);
qamd_status u8_topk_single(const qamd_u8 *h, const uint8_t *codes_dev, const float *offset_dev, uint32_t k,
                           int largest, uint32_t *out_ids, float *out_scores, qamd_mem out_mem, hipStream_t stream);
}  // namespace qamd

// ------------------------------------------------------------------------------ device helpers of both u8 files
// What the writers of a store (u8_store.hip: quantize, pack, unpack) and its readers (u8.hip: query encode, scans, pairs)
// must agree on, inlined by the kernels of both: the value -> code rule, the row-group sum, and the two scan image
// formats with the index of a chunk in the blocked image.  In an unnamed namespace like the kernels that name them: a
// translation unit's device code is its own.
namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 512;  // scan workgroup (tuning sweep: 512 and 1024 tie, 256 is ~1% behind)

__device__ __forceinline__ uint32_t dot16(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    acc = __builtin_amdgcn_udot4(a.w, b.w, acc, false);
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

// encoded_vectors_u8.rs:234-237  ((v-offset)/alpha).clamp(0,127) as u8
__device__ __forceinline__ uint32_t f32_to_u8(float v, float alpha, float offset) {
    float x = (v - offset) / alpha;  // IEEE division (hipcc: correctly rounded f32 divide)
    x = (x < 0.0f) ? 0.0f : x;
    x = (x > 127.0f) ? 127.0f : x;
    return (x != x) ? 0u : (uint32_t)x;
}

// The code of a 4-bit store (the reference has no counterpart): 16 levels, rounded to nearest.  Three f32
// operations, each rounded on its own - subtract, IEEE divide, add (every file that includes this header is compiled
// with contraction off: the Makefile's -ffp-contract=off) - then the clamp and the truncation of f32_to_u8.  NaN gives 0.
// No division-free form: every 4-bit encoder takes this one.
// A full-range store takes the same rule with 255 for 15: `top` is the largest code.
__device__ __forceinline__ uint32_t f32_to_nearest(float v, float alpha, float offset, float top) {
    float x = (v - offset) / alpha + 0.5f;
    x = (x < 0.0f) ? 0.0f : x;
    x = (x > top) ? top : x;
    return (x != x) ? 0u : (uint32_t)x;
}
// LEVELS (U8Flags::levels() above): 127 = the reference's truncating code, 15 and 255 = rounded to nearest.
template <int LEVELS> __device__ __forceinline__ uint32_t f32_to_code(float v, float alpha, float offset) {
    static_assert(LEVELS == 127 || LEVELS == 15 || LEVELS == 255, "code levels");
    return LEVELS == 127 ? f32_to_u8(v, alpha, offset) : f32_to_nearest(v, alpha, offset, (float)LEVELS);
}
// The same choice at run time (`levels` is a kernel argument: wave-uniform), for the kernels where no time is at stake.
__device__ __forceinline__ uint32_t f32_to_code(float v, float alpha, float offset, int levels) {
    return levels == 127 ? f32_to_u8(v, alpha, offset) : f32_to_nearest(v, alpha, offset, (float)levels);
}

// ---- the scan image (qamd_u8::packed): u8_pack_image_kernel writes it, u8_scan_image_kernel reads it ----
// A format carries what differs between the two images.  For the scan (the walk is described at u8_scan_image_kernel): R;
// init(P, aux) -> whole groups; group(qcodes, g) before the R calls full(w, i) of whole group g; rest_group(qcodes, c0)
// before the calls rest(w, c0, i) of the chunks from c0 on; sum().  For the pack kernel: chunk(), the 16 bytes of image
// chunk j of a row, which also gathers the bits of the code chunks it read, and kNoCode, the bits no code of the format has.
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

// 16-byte index of image chunk j of row r (the blocks of 64 rows described at qamd_u8::packed).
__device__ __forceinline__ uint64_t nibble_at(uint64_t r, uint32_t j, uint32_t pchunks) {
    return ((r / kPackBlockRows) * pchunks + j) * kPackBlockRows + r % kPackBlockRows;
}
__device__ __forceinline__ uint4 nibbles_lo(const uint4 &w) { return and16(w, 0x0F0F0F0Fu); }
__device__ __forceinline__ uint4 nibbles_hi(const uint4 &w) {
    return make_uint4((w.x >> 4) & 0x0F0F0F0Fu, (w.y >> 4) & 0x0F0F0F0Fu, (w.z >> 4) & 0x0F0F0F0Fu, (w.w >> 4) & 0x0F0F0F0Fu);
}

}  // namespace
