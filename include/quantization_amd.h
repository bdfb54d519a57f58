/*
 * quantization_amd.h — C ABI of the MI355X-native encode-and-score path.
 *
 * This is the drop-in boundary for qdrant/quantization's hot path.  The reference's own
 * FFI is per (query, vector) PAIR — 7 x86 symbols declared at
 *   quantization/src/encoded_vectors_u8.rs:476-483    impl_score_{dot,l1}_{avx,sse}
 *   quantization/src/encoded_vectors_binary.rs:317-324 impl_xor_popcnt_sse_uint{128,64,32}
 * — far too fine for a GPU (one launch per pair).  The boundary therefore moves up one
 * level to the Rust methods that call them: one opaque handle per encoded store, with the
 * methods of `trait EncodedVectors` (quantization/src/encoded_vectors.rs:21-35) plus the
 * batched form of the caller loop `for i in 0..n { score_point(q, i) }`
 * (demos/src/ann_benchmark.rs:247-252) as `*_score_all`.  Each entry point cites the
 * reference interface it replaces.  INTEGRATION.md shows the Rust `extern "C"` block and
 * the `impl EncodedVectors for ...` a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns a qamd_status.
 *   - `qamd_mem` says whether a caller buffer is host or device (HBM) memory.  Device
 *     buffers must belong to the handle's device.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls that take
 *     a stream only ENQUEUE when every buffer is device memory; host buffers make the call
 *     synchronous.
 *   - *_topk (all three quantizers) and *_topk_batch always synchronise `stream` before they
 *     return, device outputs included: the fused selection reads one status word back to decide
 *     whether the exact fallback has to run.  They cannot be captured into a hipGraph; score_all can.
 *   - every call runs on the handle's device and leaves the calling thread's current HIP device
 *     as it found it.
 *   - a call that only enqueues keeps using the calling thread's cached workspace until its work has
 *     run: the next call of that thread waits for it on the device (an event), whatever its stream.
 *     A hipGraph that captured such a call must not be replayed concurrently with other calls of the
 *     capturing thread.
 *   - handles own device memory; row bytes handed in stay caller-owned.
 *   - all score_* / topk calls are thread-safe on a shared handle (no interior mutation),
 *     matching `&self` in the reference.
 *   - no CPU fallback: every function fails with QAMD_ERR_DEVICE when no GPU is usable.
 */
#ifndef QUANTIZATION_AMD_H
#define QUANTIZATION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QAMD_API __attribute__((visibility("default")))

/* quantization/src/lib.rs:18-24 EncodingError{IOError,EncodingError,ArgumentsError,Stopped},
 * plus std::io::Error for save/load (-> QAMD_ERR_IO), the slice-index panic of
 * encoded_storage.rs:29 (-> QAMD_ERR_OUT_OF_RANGE) and HIP failures. */
typedef enum {
    QAMD_OK = 0,
    QAMD_ERR_IO = 1,
    QAMD_ERR_ENCODING = 2,
    QAMD_ERR_ARGUMENTS = 3,
    QAMD_ERR_STOPPED = 4,
    QAMD_ERR_OUT_OF_RANGE = 5,
    QAMD_ERR_DEVICE = 6
} qamd_status;

/* quantization/src/encoded_vectors.rs:6-11 */
typedef enum { QAMD_DOT = 0, QAMD_L1 = 1, QAMD_L2 = 2 } qamd_distance;
enum { QAMD_ROTATED = 8,   /* flag: or-ed onto QAMD_DOT or QAMD_L2 in qamd_vector_parameters.distance_type */
       QAMD_DOT_ROTATED = 8, QAMD_L2_ROTATED = 10 };
enum { QAMD_BITS4 = 32,    /* flag: or-ed onto QAMD_DOT or QAMD_L2, plain or rotated, in distance_type (16 is no flag) */
       QAMD_DOT_BITS4 = 32, QAMD_L2_BITS4 = 34, QAMD_DOT_ROTATED_BITS4 = 40, QAMD_L2_ROTATED_BITS4 = 42 };
enum { QAMD_COMPACT = 128, /* flag: or-ed onto a QAMD_BITS4 metric, plain or rotated; the legal values are the four below */
       QAMD_DOT_BITS4_COMPACT = 160, QAMD_L2_BITS4_COMPACT = 162, QAMD_DOT_ROTATED_BITS4_COMPACT = 168,
       QAMD_L2_ROTATED_BITS4_COMPACT = 170 };
/* A ROTATED scalar-u8 store (no counterpart in the reference).  qamd_u8_encode, qamd_u8_encoder_begin and
 * qamd_u8_from_rows take QAMD_DOT_ROTATED or QAMD_L2_ROTATED as distance_type: every row - and every query, inside
 * qamd_u8_encode_query / qamd_u8_encode_query_batch - goes through a fixed randomized Hadamard block rotation (blocks of
 * B = the largest power of two dividing dim, scaled by 2^(-log2(B)/2)) before the quantizer sees it.  The rotation is
 * orthonormal, so scores approximate the same Dot / L2 as a plain store's, but no single dimension of large magnitude
 * stretches the quantization interval.  dim must be a multiple of 64, at most 16384; QAMD_L1 | QAMD_ROTATED is refused
 * (L1 is not rotation invariant), and so is the flag on every qamd_pq_*, qamd_bin_*, qamd_f32_* and qamd_*_sharded_*
 * constructor (QAMD_ERR_ARGUMENTS, before any device call).  qamd_u8_get_metadata reports the flagged value, so
 * get_metadata -> from_rows round-trips; qamd_u8_save writes the base metric plus "rotation":"HadamardBlocks".
 * qamd_u8_upsert rotates what it is handed; qamd_u8_topk_rescored compares the BASE metric with the originals', which
 * stay plain.  qamd_u8_find_min_max / qamd_u8_find_quantile_interval see no parameters and stay plain.  The feature adds
 * no symbol: this header still declares 192 entry points. */
/* A 4-BIT scalar-u8 store (no counterpart in the reference).  The same three constructors take the metric
 * with QAMD_BITS4 or-ed on, with or without QAMD_ROTATED.  Rows keep the reference's format - [offset f32][actual_dim
 * code bytes] - but a code is one of 16 levels: alpha = (max - min) / 15 and code(v) = trunc(clamp((v - offset) / alpha
 * + 0.5, 0, 15)), rounded to nearest where the 7-bit code truncates; queries are encoded with the same code().  Offsets,
 * multiplier and every score formula are the reference's with this alpha.  A 15-level code over one interval only
 * ranks well when every coordinate has about the same spread: use it with QAMD_ROTATED unless the data is isotropic
 * already, and with the originals behind it (qamd_u8_topk_rescored).  QAMD_L1 | QAMD_BITS4 and any other bit beyond 8,
 * 32 and QAMD_COMPACT's 128 (below) are refused, and so is the flag on every qamd_pq_*, qamd_bin_*, qamd_f32_* and qamd_*_sharded_* constructor
 * (QAMD_ERR_ARGUMENTS, before any device call).  qamd_u8_get_metadata reports the flagged value; qamd_u8_save writes
 * the base metric plus a last key "bits":4 (after "rotation"), and a file without the key is a 7-bit store.
 * qamd_u8_upsert quantizes what it is handed with the handle's form.  A store of 32 to 2048 dims keeps, instead of the
 * 7-bit scan image below, a nibble image: two codes per byte, 16 * ceil(actual_dim / 32) bytes per row in blocks of 64
 * rows, which the single-query scans read (388 bytes per row at dim 768, qamd_u8_scan_bytes_per_row, against 676).
 * Byte codes plus image are 1156 bytes per row at dim 768, against 1444 for a 7-bit store; the byte codes still serve
 * every other route (pairs, bursts, batches, export, save).  No new symbol: still 192 entry points. */
/* A COMPACT 4-bit store.  QAMD_COMPACT or-ed onto a QAMD_BITS4 metric (160, 162, 168, 170), in the same
 * three constructors and, through the metadata file, in qamd_u8_load: the store keeps its f32 row offsets and the nibble
 * image and nothing else - 388 instead of 1156 bytes of HBM per row at dim 768 - and every answer it gives is, bit for
 * bit, that of the 4-bit store built from the same arguments without the flag.  Builders, qamd_u8_upsert and
 * qamd_u8_reserve write the image tile by tile through a staging buffer of byte codes; pairs and bursts gather a row's
 * pieces from the image, exports and qamd_u8_save unpack it (the files hold the reference's byte rows and the base
 * metric, then "bits":4, then a last key "compact":true - the only value qamd_u8_load accepts for it, and only beside
 * "bits":4; a file without the key is not compact), and query batches take one image scan per query: the matrix cores
 * read byte codes.  Refused with QAMD_ERR_ARGUMENTS before any device call: the flag without QAMD_BITS4, with QAMD_L1,
 * with any unknown bit, with an actual_dim that has no nibble image (below 32 or above 2048), and on every qamd_pq_*,
 * qamd_bin_*, qamd_f32_* and qamd_*_sharded_* constructor.  A build whose image cannot be allocated fails with
 * QAMD_ERR_DEVICE (there are no byte codes to fall back to), and qamd_u8_from_rows of a row with a code above 15 with
 * QAMD_ERR_ARGUMENTS.  qamd_u8_get_metadata reports the flagged value, so get_metadata -> from_rows round-trips;
 * qamd_u8_scan_bytes_per_row is unchanged.  qamd_u8_set_lane_mode(h, 1) is accepted and changes nothing: a 4-bit pair
 * sum is at most 2048 * 15 * 15 < 2^24, where both modes give the same bits.  No new symbol: still 192 entry points. */

typedef enum { QAMD_MEM_HOST = 0, QAMD_MEM_DEVICE = 1 } qamd_mem;

/* quantization/src/encoded_vectors.rs:13-19 VectorParameters */
typedef struct {
    uint64_t dim;
    uint64_t count;
    int32_t distance_type; /* qamd_distance */
    int32_t invert;        /* bool */
} qamd_vector_parameters;

/* stop_condition: impl Fn() -> bool (encoded_vectors_u8.rs:39, _binary.rs:169, _pq.rs:62).
 * Polled between device batches; non-zero => the encode returns QAMD_ERR_STOPPED. */
typedef int (*qamd_stop_fn)(void *user);

/* Last error text of the calling thread (the String inside EncodingError / io::Error). */
QAMD_API const char *qamd_last_error(void);
QAMD_API const char *qamd_version(void);
/* Number of visible HIP devices (0 => nothing in this library can run). */
QAMD_API int qamd_device_count(void);
/* Device used by handles created afterwards on this thread (default 0). */
QAMD_API qamd_status qamd_set_device(int device);
QAMD_API int qamd_get_device(void);
/* Frees what the CALLING thread has cached on the GPUs (per-device workspaces of score_all /
 * topk with host outputs, the pinned result scratch).  They are also freed when the thread exits;
 * call this from a long-lived thread that is done querying. */
QAMD_API void qamd_thread_release(void);

/* ===================================================================================
 * Scalar u8 quantizer — quantization/src/encoded_vectors_u8.rs
 * =================================================================================== */
typedef struct qamd_u8 qamd_u8;             /* EncodedVectorsU8<TStorage>  (:14-17) */
typedef struct qamd_u8_query qamd_u8_query; /* EncodedQueryU8              (:19-22) */

/* Metadata (:24-31), serde field order. */
typedef struct {
    uint64_t actual_dim;
    float alpha;
    float offset;
    float multiplier;
    qamd_vector_parameters vector_parameters;
} qamd_u8_metadata;

/* get_quantized_vector_size (:252-255) and get_actual_dim (:257-259). */
QAMD_API uint64_t qamd_u8_quantized_vector_size(const qamd_vector_parameters *vp);
QAMD_API uint64_t qamd_u8_actual_dim(const qamd_vector_parameters *vp);

/* Memory of a u8 store.  Every builder below (encode, encoder_finish, from_rows and so load) keeps the byte codes and,
 * for a Dot or L2 store of 128 to 2048 dims, a packed scan image beside them: the codes at 7 bits each, laid out in
 * blocks of 64 rows, which the single-query scans read instead of the bytes, a row per lane (12 % fewer bytes per row at
 * dim 768).  The image costs a further 0.875 x
 * the code bytes (6.7 GB on 10M x 768).  It is skipped when it would leave less free HBM than its own size, when its
 * allocation fails, and when a row holds a code above 127 (rows another producer wrote); the store then scans its
 * bytes, with the same results. */

/* EncodedVectorsU8::encode (:34-140).  data: count*dim f32, row-major (the reference's
 * `orig_data` iterator flattened).  quantile: NULL = None.  For count > 100 000 the
 * reference draws a random sample (quantile.rs:31-34); here the sample is 100 000 evenly
 * strided rows — same statistic, not the same bits.
 * `alpha_offset` non-NULL overrides the interval search with {alpha, offset}
 * (conditional parity for that sampled case). */
QAMD_API qamd_status qamd_u8_encode(const float *data, qamd_mem data_mem,
                                    const qamd_vector_parameters *vp, const float *quantile,
                                    const float *alpha_offset, qamd_stop_fn stop, void *stop_user,
                                    void *stream, qamd_u8 **out);

/* Streaming form of encode: the reference takes a clonable ITERATOR and walks it twice
 * (encoded_vectors_u8.rs:34-40: pass 1 :57-71 min/max + quantile sample, pass 2 :73-118 quantize,
 * rows appended one by one through EncodedStorageBuilder::push_vector_data,
 * encoded_storage.rs:17-25), never holding the f32 data.  Same contract in bounded batches:
 *   begin(vp{count = rows that will come}, quantile | alpha_offset, stop)
 *   observe(batch) ...   every vector once, any batch sizes          (skip when alpha_offset given)
 *   push(batch) ...      every vector again, same order: rows are appended
 *   finish(&handle)      consumes the encoder; abort() drops it.
 * stop_condition is polled once per observe/push call (-> QAMD_ERR_STOPPED).  The result is
 * byte-identical to qamd_u8_encode on the concatenated data. */
typedef struct qamd_u8_encoder qamd_u8_encoder;
QAMD_API qamd_status qamd_u8_encoder_begin(const qamd_vector_parameters *vp, const float *quantile,
                                           const float *alpha_offset, qamd_stop_fn stop, void *stop_user,
                                           void *stream, qamd_u8_encoder **out);
QAMD_API qamd_status qamd_u8_encoder_observe(qamd_u8_encoder *e, const float *batch, uint64_t n_rows,
                                             qamd_mem batch_mem);
QAMD_API qamd_status qamd_u8_encoder_push(qamd_u8_encoder *e, const float *batch, uint64_t n_rows,
                                          qamd_mem batch_mem);
QAMD_API qamd_status qamd_u8_encoder_finish(qamd_u8_encoder *e, qamd_u8 **out);
QAMD_API void qamd_u8_encoder_abort(qamd_u8_encoder *e);

/* The two global statistics of encode's pass 1 ON THEIR OWN, for a host that holds the rows in several places (one
 * process per GPU, quantization_amd/sharded.py; the single-process qamd_u8_sharded_encode does the same inside).  The
 * reference finds ONE (alpha, offset) over all data before any row is quantised (encoded_vectors_u8.rs:57-71):
 *   - qamd_u8_find_min_max = find_min_max_from_iter (quantile.rs:5-19) over the caller's n_rows x dim values (NaN never
 *     wins a compare; no rows: (f32::MAX, f32::MIN), the reference's start values).  Every holder runs it on its rows,
 *     the holders fold the results with min / max - order-free, hence the bits of the single-handle encode - and hand
 *     alpha_offset_from_min_max (encoded_vectors_u8.rs:228-232: alpha = (max - min) / 127.0f, offset = min) to
 *     qamd_u8_encode / qamd_u8_encoder_begin as `alpha_offset`.
 *   - qamd_u8_find_quantile_interval = find_quantile_interval (quantile.rs:21-71) over `count` vectors; *found = 0 is the
 *     reference's None (keep the min / max interval).  Its sample is every vector for count <= 100 000 and the rows
 *     floor(k * count / 100 000), k < 100 000, beyond (the reference draws a random one there): a distributed host
 *     gathers exactly those rows, in k order, to one holder and calls this with count = the number gathered. */
QAMD_API qamd_status qamd_u8_find_min_max(const float *data, qamd_mem data_mem, uint64_t n_rows, uint64_t dim,
                                          void *stream, float *min, float *max);
QAMD_API qamd_status qamd_u8_find_quantile_interval(const float *data, qamd_mem data_mem, uint64_t count, uint64_t dim,
                                                    float quantile, void *stream, int *found, float *min, float *max);

/* Adopt rows already in the reference's storage format — what
 * EncodedStorage::get_vector_data serves (encoded_storage.rs:27-31): count rows of
 * [vector_offset f32 ne][actual_dim codes].  Used by load and by callers holding a store
 * encoded by the reference.  The rows are copied/re-laid-out into library-owned HBM. */
QAMD_API qamd_status qamd_u8_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                       const qamd_u8_metadata *meta, void *stream, qamd_u8 **out);

/* The inverse: write the reference-format row bytes (count * quantized_vector_size). */
QAMD_API qamd_status qamd_u8_export_rows(const qamd_u8 *h, uint8_t *rows, qamd_mem rows_mem,
                                         void *stream);
/* Rows [first_row, first_row + n_rows) only: the caller-owned-storage half of encode.  The reference's
 * encode pushes every row into the CALLER's store (storage_builder.push_vector_data,
 * encoded_vectors_u8.rs:34-40,117; encoded_storage.rs:17-25); a binding feeds its EncodedStorageBuilder
 * from bounded ranges (e.g. 64k rows) after encode / encoder_finish, so the store never has to exist
 * as one host buffer.  QAMD_ERR_OUT_OF_RANGE when the range leaves [0, count]. */
QAMD_API qamd_status qamd_u8_export_rows_range(const qamd_u8 *h, uint64_t first_row, uint64_t n_rows,
                                               uint8_t *rows, qamd_mem rows_mem, void *stream);
QAMD_API qamd_status qamd_u8_get_metadata(const qamd_u8 *h, qamd_u8_metadata *out);

/* EncodedVectors::save / load (:263-288): raw row file + serde_json metadata file. */
QAMD_API qamd_status qamd_u8_save(const qamd_u8 *h, const char *data_path, const char *meta_path);
QAMD_API qamd_status qamd_u8_load(const char *data_path, const char *meta_path,
                                  const qamd_vector_parameters *vp, qamd_u8 **out);

/* EncodedVectors::encode_query (:290-329).  *query is created when NULL and re-used
 * otherwise (no allocation on the hot loop).  qdim is `query.len()`. */
QAMD_API qamd_status qamd_u8_encode_query(const qamd_u8 *h, const float *query, uint64_t qdim,
                                          qamd_mem query_mem, void *stream, qamd_u8_query **query_io);
/* Inspect an encoded query: offset and the actual_dim code bytes (host buffers). */
QAMD_API qamd_status qamd_u8_query_read(const qamd_u8_query *q, float *offset, uint8_t *codes,
                                        uint64_t codes_capacity, uint64_t *codes_len);
QAMD_API void qamd_u8_query_free(qamd_u8_query *q);

/* EncodedVectors::score_point (:331-384) and score_internal (:386-453). */
QAMD_API qamd_status qamd_u8_score_point(const qamd_u8 *h, const qamd_u8_query *q, uint32_t i,
                                         float *out);
QAMD_API qamd_status qamd_u8_score_internal(const qamd_u8 *h, uint32_t i, uint32_t j, float *out);

/* score_internal (:386-453) for ONE stored row against many: out[k] = score_internal(i, ids[k]) -- what
 * graph construction asks (a new node against its candidate list), one launch instead of one per pair.
 * Host or device ids / outputs; with device ids and outputs the call only enqueues.
 * The null id list: ids == NULL stands for the rows 0 .. n_ids - 1, served by *_score_internal_all's scan over that
 * prefix of the store (out[j] has the bits of *_score_internal(h, i, j)); ids_mem is ignored, n_ids > count is
 * QAMD_ERR_OUT_OF_RANGE, and the output synchronises as *_score_internal_all's does. */
QAMD_API qamd_status qamd_u8_score_internal_ids(const qamd_u8 *h, uint32_t i, const uint32_t *ids, uint64_t n_ids,
                                                qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream);
/* ... and for MANY stored rows, each against its own id list, in one launch: list l is
 * ids[list_offsets[l] .. list_offsets[l + 1]) (list_offsets: n_lists + 1 entries from 0, n_ids =
 * list_offsets[n_lists]); out[p] = score_internal(rows[l], ids[p]) for every p of list l.
 * `lists_mem` says where rows, list_offsets and ids live (one kind for the three).  Host lists are
 * validated (QAMD_ERR_OUT_OF_RANGE as score_internal) and bursts of up to ~1000 ids travel through the
 * calling thread's mapped scratch (one launch + one synchronisation, no allocation, no copy call);
 * device lists need a device output and only enqueue: an id or row out of range scores NaN.
 * The null-list form (many stored rows against the whole store; no entry point of its own): ids == NULL stands, for
 * EVERY list, for the rows 0 .. n_ids - 1, and n_ids is then the length of each list, not the total:
 * out[l * n_ids + j] has the bits of *_score_internal(h, rows[l], j).  Row rows[l] itself is included; duplicates in rows
 * are allowed.  The store is read once per group of rows (u8: 4 rows a pass, 2 for rows of 97 to 128 16-byte pieces, 8
 * for L1 rows of up to 48; binary: 8, 4 or 2; PQ: one launch builds the group's tables, then a scan per row).
 *   - list_offsets must be NULL too: list_offsets without ids is QAMD_ERR_ARGUMENTS (the caller forgot the ids).
 *   - n_ids > count is QAMD_ERR_OUT_OF_RANGE before any launch; n_lists == 0 or n_ids == 0 is QAMD_OK and nothing is
 *     written; a null handle is refused before any device call; NULL rows with n_lists > 0 is QAMD_ERR_ARGUMENTS.
 *   - rows lives in lists_mem.  Host rows are validated: a row >= count is QAMD_ERR_OUT_OF_RANGE before any launch.
 *     Device rows cannot be: a row >= count gives NaN in all n_ids outputs of its list, the other lists are untouched.
 *   - Device rows need a device output, and the call then only enqueues.  Host rows with a device output synchronise
 *     `stream` once the rows have been read, as the list form does; a host output synchronises `stream`.
 *   - A host output is produced in groups of rows through the calling thread's score workspace: a group's scores stay
 *     within 512 MiB (one row if need be), and the call never allocates n_lists * n_ids * 4 bytes.
 *   - u8: lane mode holds as everywhere (mode 1 on a Dot / L2 store takes the lane-order kernel row by row).  PQ: a
 *     handle without centroids is QAMD_ERR_ARGUMENTS.
 * Every call with a given id list behaves as before. */
QAMD_API qamd_status qamd_u8_score_internal_ids_batch(const qamd_u8 *h, const uint32_t *rows,
                                                      const uint32_t *list_offsets, uint32_t n_lists,
                                                      const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem,
                                                      float *out, qamd_mem out_mem, void *stream);

/* score_internal against the WHOLE store (all three quantizers; with these six the header declares 192 entry points):
 *   *_score_internal_all: out[j] has the bits of *_score_internal(h, i, j) for every j < count.  Row i itself is included;
 *     callers drop it.
 *   *_topk_internal: the k best of exactly those scores under the one ordering stated at qamd_u8_topk (the total order on
 *     the score bits, ties to the lower id, best first, NaN rule included).  k <= 1024; k == 0 is QAMD_OK.
 * What "the rows most like stored row i" needs (recommend-by-id, near-duplicate detection, the exact neighbour lists a
 * graph builder checks its links against) in one bandwidth-bound scan, not count pairs through *_score_internal_ids.  A
 * stored row cannot be passed off as a query: score_point and score_internal differ in arithmetic (u8: the epilogue, PQ:
 * the table and the summation order), and no query can be built from stored codes.
 * The arithmetic is the reference's score_internal - encoded_vectors_u8.rs:386-453, encoded_vectors_pq.rs:566-593,
 * encoded_vectors_binary.rs:302-314 - pair by pair; the whole-store form has no counterpart there.
 *   - i >= count is QAMD_ERR_ARGUMENTS, refused before any launch; a null handle is refused before any device call;
 *     an empty store is QAMD_OK (nothing is written; topk_internal writes the padding of a short list).
 *   - Host and device outputs synchronise exactly as *_score_all / *_topk do: score_internal_all with a device output
 *     only enqueues, topk_internal always synchronises `stream`.
 *   - u8: lane mode (qamd_u8_set_lane_mode) holds as for every other call.  PQ: a handle without centroids is
 *     QAMD_ERR_ARGUMENTS.
 * Out of scope: Sharded handles have no whole-store score_internal.  There is no batched topk_internal_batch entry
 * point: the scores of many rows come from the null-list form of *_score_internal_ids_batch, and ranking them is
 * qamd_topk_scores per row.  There is no rescored variant (topk_internal followed by a re-rank with the original vectors). */
QAMD_API qamd_status qamd_u8_score_internal_all(const qamd_u8 *h, uint32_t i, float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_u8_topk_internal(const qamd_u8 *h, uint32_t i, uint32_t k, int largest,
                                           uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream);

/* NEW (batched caller loop, demos/src/ann_benchmark.rs:247-252):
 * out[i] = score_point(q, i) for i in [0, count). */
QAMD_API qamd_status qamd_u8_score_all(const qamd_u8 *h, const qamd_u8_query *q, float *out,
                                       qamd_mem out_mem, void *stream);
/* Random-access form (demos/benches/encode.rs "score random access"): out[k] = score_point(q, ids[k]). */
QAMD_API qamd_status qamd_u8_score_ids(const qamd_u8 *h, const qamd_u8_query *q,
                                       const uint32_t *ids, uint64_t n_ids, qamd_mem ids_mem,
                                       float *out, qamd_mem out_mem, void *stream);
/* Fused scan + selection (demos/src/ann_benchmark_data.rs:151-167 keeps the best 30 in a
 * heap).  largest != 0 keeps the k largest scores, else the k smallest; ties break to the
 * lower index; results are sorted best-first.  k <= 1024.
 * Order of scores (every *_topk, *_topk_batch, *_sharded_topk*, *_topk_rescored, qamd_f32_rerank*, qamd_topk_scores
 * and qamd_topk_merge): rows are ranked by one total order on the f32 bit pattern of the score, not by a float
 * compare.  Ascending it reads -NaN < -inf < negative finite < -0 < +0 < positive finite < +inf < +NaN; among NaNs of
 * one sign a larger payload lies further out.  `largest` takes that order from the top, smallest-first from the
 * bottom: a +NaN score is the best row of a `largest` call and the worst of a smallest-first call, a -NaN score the
 * reverse.  Equal bit patterns go to the lower id.  A returned score is the row's own score bits: a NaN keeps its
 * sign and payload.  (The padding of a short list, id 0xFFFFFFFF with -inf / +inf, comes after every row.) */
QAMD_API qamd_status qamd_u8_topk(const qamd_u8 *h, const qamd_u8_query *q, uint32_t k,
                                  int largest, uint32_t *out_ids, float *out_scores,
                                  qamd_mem out_mem, void *stream);
QAMD_API void qamd_u8_free(qamd_u8 *h);

/* Multi-query form: many queries against the store at once (the caller's OUTER loop over
 * queries, demos/src/ann_benchmark.rs:245-260, with its per-query 30-entry heap,
 * demos/src/ann_benchmark_data.rs:151-167).  On the GPU this is a dense u8 x u8 -> i32
 * contraction on the matrix cores; every score is bit-identical to qamd_u8_score_all for the
 * same query.  Dot and L2 run the reference's dot kernel (encoded_vectors_u8.rs:339-341) as that
 * contraction; L1 (sum |q - v|, no matrix form) is served by the single-query kernel per query. */
typedef struct qamd_u8_query_batch qamd_u8_query_batch; /* n x EncodedQueryU8 */
/* queries: n_queries x qdim f32, row-major.  *batch_io is created when NULL, else re-used. */
QAMD_API qamd_status qamd_u8_encode_query_batch(const qamd_u8 *h, const float *queries,
                                                uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                                                void *stream, qamd_u8_query_batch **batch_io);
QAMD_API void qamd_u8_query_batch_free(qamd_u8_query_batch *b);
/* out[q * count + i] = score_point(query q, i): n_queries * count f32 (mind the size). */
QAMD_API qamd_status qamd_u8_score_batch(const qamd_u8 *h, const qamd_u8_query_batch *b, float *out,
                                         qamd_mem out_mem, void *stream);
/* score_point (:331-384) for many (query, id list) pairs in ONE launch -- one hop of every in-flight
 * HNSW search: list l (ids[list_offsets[l] .. list_offsets[l + 1])) is scored against query l of the
 * batch; out[p] = score_point(query l, ids[p]).  n_lists <= n_queries.  Buffers as
 * qamd_u8_score_internal_ids_batch. */
QAMD_API qamd_status qamd_u8_score_ids_batch(const qamd_u8 *h, const qamd_u8_query_batch *b,
                                             const uint32_t *list_offsets, uint32_t n_lists, const uint32_t *ids,
                                             uint64_t n_ids, qamd_mem lists_mem, float *out, qamd_mem out_mem,
                                             void *stream);
/* out_ids / out_scores: n_queries x k, per query as qamd_u8_topk.  Synchronises the stream. */
/* (A device that does not report 256 CUs - a partitioned MI355X - never takes the rq kernels u8_gemm_rq16_kernel /
 * u8_gemm_rk16_kernel; every grid is sized by its own CU count.  The answer is the same on every route.) */
QAMD_API qamd_status qamd_u8_topk_batch(const qamd_u8 *h, const qamd_u8_query_batch *b, uint32_t k,
                                        int largest, uint32_t *out_ids, float *out_scores,
                                        qamd_mem out_mem, void *stream);

/* Extension (no reference counterpart): how a pair sum >= 2^24 (only possible for
 * actual_dim > 1040) becomes f32.  0 (default): exact integer, rounded once — what the
 * reference's scalar path does (encoded_vectors_u8.rs:158).  1: the 8-lane f32 summation
 * order of impl_score_dot_avx (quantization/cpp/avx2.c:41-62), bit for bit.
 * The mode holds for the whole handle: score_point, score_internal, score_all, score_ids,
 * score_internal_ids, both bursts (*_ids_batch), topk, score_batch and topk_batch.  In mode 1
 * the batch calls take per-query scans instead of the matrix cores.
 * Mode 1 changes Dot and L2 only; L1 is the exact sum in both modes (impl_score_l1_avx's u16
 * lanes wrap from actual_dim 8272 on: not reproduced).  Mode 1's claim holds for codes <= 127,
 * what the encoder writes.  Up to actual_dim 2080 the two modes give the same bits (each f32
 * half sum of the lane order stays below 2^24); they can differ from 2096 on.  Sharded handles
 * have no lane switch: they always answer in mode 0. */
QAMD_API qamd_status qamd_u8_set_lane_mode(qamd_u8 *h, int mode);

/* ===================================================================================
 * Binary quantizer — quantization/src/encoded_vectors_binary.rs
 * =================================================================================== */
typedef struct qamd_bin qamd_bin;             /* EncodedVectorsBin<TBitsStoreType,TStorage> (:11-15) */
typedef struct qamd_bin_query qamd_bin_query; /* EncodedBinVector (:17-19) */

typedef enum { QAMD_BITS_U8 = 0, QAMD_BITS_U128 = 1 } qamd_bits_store; /* BitsStoreType impls :44,:119 */

/* get_quantized_vector_size_from_params (:210-213), bytes per row. */
QAMD_API uint64_t qamd_bin_quantized_vector_size(const qamd_vector_parameters *vp,
                                                 qamd_bits_store store);
/* EncodedVectorsBin::encode (:165-191). */
QAMD_API qamd_status qamd_bin_encode(const float *data, qamd_mem data_mem,
                                     const qamd_vector_parameters *vp, qamd_bits_store store,
                                     qamd_stop_fn stop, void *stop_user, void *stream,
                                     qamd_bin **out);
/* Streaming form (EncodedVectorsBin::encode walks its iterator once, :165-191): begin, push
 * batches in row order, finish.  See qamd_u8_encoder_*. */
typedef struct qamd_bin_encoder qamd_bin_encoder;
QAMD_API qamd_status qamd_bin_encoder_begin(const qamd_vector_parameters *vp, qamd_bits_store store,
                                            qamd_stop_fn stop, void *stop_user, void *stream,
                                            qamd_bin_encoder **out);
QAMD_API qamd_status qamd_bin_encoder_push(qamd_bin_encoder *e, const float *batch, uint64_t n_rows,
                                           qamd_mem batch_mem);
QAMD_API qamd_status qamd_bin_encoder_finish(qamd_bin_encoder *e, qamd_bin **out);
QAMD_API void qamd_bin_encoder_abort(qamd_bin_encoder *e);
QAMD_API qamd_status qamd_bin_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                        const qamd_vector_parameters *vp, qamd_bits_store store,
                                        void *stream, qamd_bin **out);
QAMD_API qamd_status qamd_bin_export_rows(const qamd_bin *h, uint8_t *rows, qamd_mem rows_mem,
                                          void *stream);
/* Ranged form (storage_builder.push_vector_data, encoded_vectors_binary.rs:165-191 via
 * encoded_storage.rs:17-25); see qamd_u8_export_rows_range. */
QAMD_API qamd_status qamd_bin_export_rows_range(const qamd_bin *h, uint64_t first_row, uint64_t n_rows,
                                                uint8_t *rows, qamd_mem rows_mem, void *stream);
QAMD_API qamd_status qamd_bin_save(const qamd_bin *h, const char *data_path, const char *meta_path);
QAMD_API qamd_status qamd_bin_load(const char *data_path, const char *meta_path,
                                   const qamd_vector_parameters *vp, qamd_bits_store store,
                                   qamd_bin **out);
/* Two-bit rows: per dimension i two strict f32 compares against thresholds lo_i <= hi_i taken from the data.  The
 * reference has NO counterpart (its snapshot predates upstream's two-bit encoding); DESIGN.md 3.2e is the specification.
 *   - A row holds code_bits = 2 * dim bits in the one-bit layout (byte j / 8, bit j % 8): bit i = x_i > lo_i, bit
 *     dim + i = x_i > hi_i - the second plane starts at bit dim, aligned or not.  NaN and -inf give (0,0), +inf (1,1); the
 *     reachable codes (0,0), (1,0), (1,1) are levels 0, 1, 2 and their Hamming distance is the difference in level.  Row
 *     bytes are qamd_bin_quantized_vector_size_enc = the one-bit size of a vector of code_bits dimensions; pad bits are 0.
 *   - A score is calculate_metric (:237-252) on the xor-popcount of two such rows with code_bits in place of dim.  dim is
 *     at most 2^23 (QAMD_ERR_ARGUMENTS beyond), so every score is an exact f32 integer.
 *   - qamd_bin_encode_query / _encode_query_batch on a two-bit handle encode the query like a row (qdim must be the
 *     handle's dim); every scoring call, every batch route and the rescored top-k then serve the store as they serve a
 *     one-bit store of code_bits dimensions.  The vectors' dimension stays vp.dim: originals of a rescored top-k have dim.
 *   - Statistics (bit-exact, independent of how a caller batches the rows): column i's rows are cut into blocks of 4096
 *     by row index; within a block S = sum (double)x and Q = sum (double)x * (double)x accumulate in row order from +0.0
 *     over the finite entries, n counts them; the block sums are added in block order.
 *   - Thresholds (host, f64, single operations): mean = S / n, var = Q / n - mean * mean (both 0 for n = 0), var = 0
 *     unless var > 0, sd = sqrt(var), lo = (float)(mean - t * sd), hi = (float)(mean + t * sd).  Default t = 0.43 (near
 *     the terciles of a normal column; not validated on real embeddings).
 * Out of scope: the qamd_bin_sharded_* handles stay one-bit; a 1.5-bit encoding; bench.py (it measures one-bit stores).
 * Scalar (4- / 8-bit) queries against two-bit rows come from qamd_bin_encode_query_scalar_w / _batch_scalar_w below
 * (DESIGN.md 3.2f); the unweighted qamd_bin_encode_query_scalar / _batch_scalar refuse a two-bit handle
 * (QAMD_ERR_ARGUMENTS).
 *
 * Rotated rows: a randomized Hadamard rotation before the sign and threshold bits.  The reference has NO counterpart;
 * DESIGN.md 3.2g is the specification.  QAMD_BIN_ROTATED is a flag or-ed onto one of the two encodings above; it rides
 * the `encoding` argument of the four *_enc calls and the handle carries it from there (no entry point of its own).
 * Values 2, 3, 6, 7 and above (but for the two block values after the typedef) are QAMD_ERR_ARGUMENTS before any device
 * call.
 *   - P = the smallest power of two >= dim (1 for dim <= 1); a rotated handle has dim <= 16384 (QAMD_ERR_ARGUMENTS beyond,
 *     before any device call).  y_i = x_i for i < dim and +0.0f up to P; y_i's sign bit is flipped iff h & 1 after, in
 *     u32 arithmetic, h = i * 0x9E3779B1; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *     (a fixed seed: nothing is stored per handle); then for s = 1, 2, 4, .., P / 2 in this order and every j with
 *     (j & s) == 0: (y_j, y_{j+s}) = (y_j + y_{j+s}, y_j - y_{j+s}), one f32 operation each, round to nearest even,
 *     subnormals kept, no normalisation; NaN and +-inf spread as IEEE 754 says.
 *   - Everything downstream sees a vector of P dimensions.  One bit: bit i = y_i > 0, code_bits = P.  Two bits: the
 *     two-bit rows above on y with lo, hi of P entries, code_bits = 2 P, the statistics over the P rotated columns.  Row
 *     bytes are the one-bit size of code_bits dimensions; qamd_bin_get_encoding returns the flagged value;
 *     qamd_bin_get_thresholds and the lo / hi arguments of the *_enc calls have P entries (they can come from another
 *     rotated handle).  qamd_bin_find_stats stays a raw-data call: it does not rotate.
 *   - Queries have qdim == dim and are rotated the same way first: qamd_bin_encode_query / _batch then encode as a row,
 *     qamd_bin_encode_query_scalar / _batch_scalar serve rotated one-bit handles with codes from y (their dimension limit
 *     applies to P), the _w calls rotated two-bit handles with w_i = y_i * (hi_i - lo_i).
 *   - Scores, every route, score_internal, topk_internal, rescoring, upsert, save / load: a rotated store of dim is
 *     served exactly as a plain store of code_bits bits; vp.dim stays the vectors' dimension for originals.  Metadata
 *     says "encoding":"OneBitRotated" or "TwoBitsRotated", the latter with thresholds of P entries.
 * Out of scope: sharded binary handles; seeds other than the fixed one; more than one round; block-diagonal rotations
 * with blocks of unequal size, and dims that are not a multiple of 64 (equal blocks: below); bench.py. */
typedef enum { QAMD_BIN_ONE_BIT = 0, QAMD_BIN_TWO_BITS = 1,
               QAMD_BIN_ROTATED = 4,            /* flag: or-ed onto one of the two above */
               QAMD_BIN_ONE_BIT_ROTATED = 4, QAMD_BIN_TWO_BITS_ROTATED = 5 } qamd_bin_encoding;
/* Block-rotated rows: the rotation above without the pad, so a row of 768 or 1536 dimensions keeps 768 or 1536 bits.
 * DESIGN.md 3.2h is the specification.  QAMD_BIN_BLOCKS is a second flag, legal only together with QAMD_BIN_ROTATED: the
 * two values below are qamd_bin_encoding values for every call that takes or returns one.  QAMD_BIN_BLOCKS alone (16) and
 * 17 are refused like every unknown value (QAMD_ERR_ARGUMENTS, "unknown binary encoding"), as are 18, 19 and all above 21.
 *   - dim % 64 == 0 and dim <= 16384, QAMD_ERR_ARGUMENTS otherwise before any device call.  B = the largest power of two
 *     that divides dim (B >= 64).
 *   - y_i = x_i for i < dim, no pad; the signs of the rotation above for i < dim; its stages s = 1, 2, 4, .., B / 2 in
 *     this order over every j < dim with (j & s) == 0, one f32 operation each, no normalisation.  No pair leaves its
 *     B-aligned block: these are dim / B Hadamard transforms of size B, all of one size so that every column carries the
 *     same scale sqrt(B).
 *   - Everything downstream sees a vector of dim dimensions: code_bits = dim or 2 dim, thresholds, lo / hi arguments and
 *     qamd_bin_get_thresholds of dim entries, the statistics over the dim rotated columns, scalar queries' limits on dim.
 *     Rows are those of a plain store's size; every item of the rotated rows above holds with dim in place of P.
 *   - Metadata says "encoding":"OneBitRotatedBlocks" or "TwoBitsRotatedBlocks"; qamd_bin_load refuses a dim that is not a
 *     multiple of 64 under these names, and arrays whose length is not dim, as QAMD_ERR_IO before any device call.
 *   - A power-of-two dim >= 64 has B = dim: rows, thresholds and query codes are byte-identical to the ROTATED encodings';
 *     only the reported encoding value and the file's name differ. */
enum { QAMD_BIN_BLOCKS = 16,                    /* flag: or-ed onto one of the two ROTATED values, never alone */
       QAMD_BIN_ONE_BIT_ROTATED_BLOCKS = 20, QAMD_BIN_TWO_BITS_ROTATED_BLOCKS = 21 };
QAMD_API uint64_t qamd_bin_quantized_vector_size_enc(const qamd_vector_parameters *vp, qamd_bits_store store,
                                                     qamd_bin_encoding encoding);
/* The statistics above over ONE contiguous block of n_rows x dim values (blocks of 4096 counted from the call's first
 * row); n, sum, sumsq: dim host entries each.  On its own for the reason qamd_u8_find_min_max is: a host that holds the
 * rows in several places adds the three arrays of its holders and derives ONE set of thresholds with
 * qamd_bin_thresholds_from_stats.  Unlike min / max, a sum of per-holder sums is NOT bit-equal to the single-handle
 * result (f64 addition is not associative): every holder must then be given the same derived thresholds.
 * A raw-data call: it never rotates.  Thresholds for rotated two-bit rows (P entries) come from qamd_bin_encode_enc /
 * _encoder_begin_enc with NULL thresholds, or from a rotated handle's qamd_bin_get_thresholds. */
QAMD_API qamd_status qamd_bin_find_stats(const float *data, qamd_mem data_mem, uint64_t n_rows, uint64_t dim,
                                         void *stream, uint64_t *n, double *sum, double *sumsq);
/* Host only: never touches a device and works on a machine without one. */
QAMD_API qamd_status qamd_bin_thresholds_from_stats(uint64_t dim, const uint64_t *n, const double *sum,
                                                    const double *sumsq, double t, float *lo, float *hi);
/* qamd_bin_encode with an encoding.  lo, hi: dim host floats each, or both NULL = qamd_bin_find_stats over `data`, then
 * qamd_bin_thresholds_from_stats with t = 0.43.  QAMD_ERR_ARGUMENTS for exactly one NULL, any NaN, lo_i > hi_i and
 * dim > 2^23.  QAMD_BIN_ONE_BIT: lo and hi must be NULL and the call is qamd_bin_encode. */
QAMD_API qamd_status qamd_bin_encode_enc(const float *data, qamd_mem data_mem,
                                         const qamd_vector_parameters *vp, qamd_bits_store store,
                                         qamd_bin_encoding encoding, const float *lo, const float *hi,
                                         qamd_stop_fn stop, void *stop_user, void *stream, qamd_bin **out);
/* Streaming form.  Two bits with NULL thresholds: observe all vp.count rows (any batch sizes; the open block's sums are
 * carried from call to call), then push them again in the same order; a push after too few observed rows and an observe
 * after a push are QAMD_ERR_ARGUMENTS.  With thresholds given, or one bit, observe is an accepted no-op.  Thresholds and
 * rows are byte-identical to qamd_bin_encode_enc on the concatenated data, whatever the batch sizes.  push, finish and
 * abort are those of qamd_bin_encoder_begin. */
QAMD_API qamd_status qamd_bin_encoder_begin_enc(const qamd_vector_parameters *vp, qamd_bits_store store,
                                                qamd_bin_encoding encoding, const float *lo, const float *hi,
                                                qamd_stop_fn stop, void *stop_user, void *stream,
                                                qamd_bin_encoder **out);
QAMD_API qamd_status qamd_bin_encoder_observe(qamd_bin_encoder *e, const float *batch, uint64_t n_rows,
                                              qamd_mem batch_mem);
/* Two bits: thresholds are required (queries need them). */
QAMD_API qamd_status qamd_bin_from_rows_enc(const uint8_t *rows, qamd_mem rows_mem,
                                            const qamd_vector_parameters *vp, qamd_bits_store store,
                                            qamd_bin_encoding encoding, const float *lo, const float *hi,
                                            void *stream, qamd_bin **out);
/* Either pointer may be NULL.  *code_bits = the bits of a row: dim, or 2 * dim.  Rotated rows: the flagged encoding
 * (4 or 5) and P, or 2 * P; block-rotated rows: 20 or 21 and dim, or 2 * dim. */
QAMD_API qamd_status qamd_bin_get_encoding(const qamd_bin *h, qamd_bin_encoding *encoding, uint64_t *code_bits);
/* dim host floats each (P each for rotated two-bit rows, dim for block-rotated ones); QAMD_ERR_ARGUMENTS on a one-bit
 * handle. */
QAMD_API qamd_status qamd_bin_get_thresholds(const qamd_bin *h, float *lo, float *hi);
/* qamd_bin_save of a two-bit handle writes {"vector_parameters":{..},"encoding":"TwoBits","thresholds":{"lo":[..],
 * "hi":[..]}} (infinite thresholds have no JSON form: QAMD_ERR_IO); a one-bit file is the reference's, unchanged.
 * qamd_bin_load: no "encoding" key, or "OneBit", is one bit; rows are sized by the file's encoding, thresholds restored
 * bit for bit; QAMD_ERR_IO before any device call for an unknown encoding, "TwoBits" without thresholds, arrays whose
 * length is not the caller's dim, and lo > hi. */

/* encode_query (:288-291). */
QAMD_API qamd_status qamd_bin_encode_query(const qamd_bin *h, const float *query, uint64_t qdim,
                                           qamd_mem query_mem, void *stream,
                                           qamd_bin_query **query_io);
/* Scalar ("asymmetric") queries: the stored rows stay one bit per dimension, the query keeps 4 or 8.  The reference
 * has NO counterpart (its snapshot predates upstream's asymmetric binary quantization); DESIGN.md 3.2d is the
 * specification: codes c_i = min(L, (u32)((q_i + a) * (L / (a + a)) + 0.5f)) with L = 2^bits - 1 and a = max |q_i|,
 * held as `bits` bit planes in the rows' layout, and the score calculate_metric(sum_b 2^b popcount(plane_b xor row))
 * with dim * L in place of dim.  bits = 1 is qamd_bin_encode_query; other values than 1, 4, 8 and dims whose dim * L
 * would leave f32's exact integers (above 65 792 at 8 bits, 1 118 481 at 4) are QAMD_ERR_ARGUMENTS.  *query_io is
 * reused as by qamd_bin_encode_query and may change its bit count from call to call.  qamd_bin_score_point / _ids /
 * _all, qamd_bin_topk and qamd_bin_topk_rescored take either kind of query; a qamd_bin_query_batch holds scalar queries
 * through qamd_bin_encode_query_batch_scalar below.
 * Deliberately left out: the qamd_bin_sharded_* query types are separate structs and stay binary-only. */
QAMD_API qamd_status qamd_bin_encode_query_scalar(const qamd_bin *h, const float *query, uint64_t qdim,
                                                  qamd_mem query_mem, uint32_t bits, void *stream,
                                                  qamd_bin_query **query_io);
/* Weighted scalar queries: 4- or 8-bit queries against TWO-BIT rows.  The reference has NO counterpart; DESIGN.md 3.2f is
 * the specification.  A two-bit row stands for about mean_i + sd_i * (level_i - 1) in column i, and sd_i is proportional to
 * h_i = hi_i - lo_i, so the codes come from w_i = q_i * h_i (h_i = 0 where it is not finite, a NaN w_i = 0) exactly as
 * qamd_bin_encode_query_scalar takes them from q_i (a = max |w_i| over the finite w_i), and the code of dimension i sits
 * at bit i AND bit dim + i of each of the `bits` planes, which are rows of code_bits = 2 dim bits.  Every scoring call
 * then serves the query as it serves a scalar query against one-bit rows of code_bits dimensions: X = sum_b 2^b
 * popcount(plane_b xor row) adds 2 c_i, L or 2 (L - c_i) for a dimension at level 0, 1 or 2, and the score is
 * calculate_metric on X with code_bits * L for dim.  qdim must be the handle's dim; dims above 32 896 at 8 bits and
 * 559 240 at 4 (code_bits * L past f32's exact integers) and bits other than 1, 4, 8 are QAMD_ERR_ARGUMENTS; bits = 1 is
 * qamd_bin_encode_query.  On a one-bit handle the call IS qamd_bin_encode_query_scalar (h_i = 1), bit for bit, so a
 * caller need not branch on the encoding.  Arguments and reuse of *query_io as there; one object may move between bit
 * counts and between the two calls.  Recall in a numpy model on synthetic data only: not validated on
 * real embeddings. */
QAMD_API qamd_status qamd_bin_encode_query_scalar_w(const qamd_bin *h, const float *query, uint64_t qdim,
                                                    qamd_mem query_mem, uint32_t bits, void *stream,
                                                    qamd_bin_query **query_io);
/* No counterpart in the reference: *bits = the number of bit planes, *max_abs = a; a query from
 * qamd_bin_encode_query gives 1 and 0.  Either pointer may be NULL. */
QAMD_API qamd_status qamd_bin_query_info(const qamd_bin_query *q, uint32_t *bits, float *max_abs);
/* *len = the bytes of the encoded query: one row of bits, or for a scalar query bits x row bytes, plane 0 (the least
 * significant) first. */
QAMD_API qamd_status qamd_bin_query_read(const qamd_bin_query *q, uint8_t *bits,
                                         uint64_t capacity, uint64_t *len);
QAMD_API void qamd_bin_query_free(qamd_bin_query *q);
/* score_point (:293-300), score_internal (:302-314). */
QAMD_API qamd_status qamd_bin_score_point(const qamd_bin *h, const qamd_bin_query *q, uint32_t i,
                                          float *out);
QAMD_API qamd_status qamd_bin_score_internal(const qamd_bin *h, uint32_t i, uint32_t j, float *out);
/* Bursts of pairs in one launch (score_internal :302-314 is the metric of score_point on two stored
 * rows); arguments as qamd_u8_score_internal_ids / _ids_batch, the null id list (ids == NULL: the rows 0 .. n_ids - 1)
 * as stated at qamd_u8_score_internal_ids and qamd_u8_score_internal_ids_batch. */
QAMD_API qamd_status qamd_bin_score_internal_ids(const qamd_bin *h, uint32_t i, const uint32_t *ids, uint64_t n_ids,
                                                 qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_score_internal_ids_batch(const qamd_bin *h, const uint32_t *rows,
                                                       const uint32_t *list_offsets, uint32_t n_lists,
                                                       const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem,
                                                       float *out, qamd_mem out_mem, void *stream);
/* score_internal (:302-314) against the whole store, contract as qamd_u8_score_internal_all / _topk_internal: the metric of
 * score_point with stored row i as the one-plane query, one-bit and two-bit rows alike. */
QAMD_API qamd_status qamd_bin_score_internal_all(const qamd_bin *h, uint32_t i, float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_topk_internal(const qamd_bin *h, uint32_t i, uint32_t k, int largest,
                                            uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_score_all(const qamd_bin *h, const qamd_bin_query *q, float *out,
                                        qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_score_ids(const qamd_bin *h, const qamd_bin_query *q,
                                        const uint32_t *ids, uint64_t n_ids, qamd_mem ids_mem,
                                        float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_topk(const qamd_bin *h, const qamd_bin_query *q, uint32_t k,
                                   int largest, uint32_t *out_ids, float *out_scores,
                                   qamd_mem out_mem, void *stream);
QAMD_API void qamd_bin_free(qamd_bin *h);

/* Many queries at once (the caller's outer loop, demos/src/ann_benchmark.rs:245-260; BASELINE config
 * 3/4 shape).  score_batch reads every row once for up to 8 queries; topk_batch runs the per-query
 * fused selections back to back with one status read-back per 32 queries.  Every score and list is
 * bit-identical to the single-query calls.  topk_batch synchronises the stream. */
typedef struct qamd_bin_query_batch qamd_bin_query_batch; /* n x EncodedBinVector */
QAMD_API qamd_status qamd_bin_encode_query_batch(const qamd_bin *h, const float *queries, uint64_t n_queries,
                                                 uint64_t qdim, qamd_mem queries_mem, void *stream,
                                                 qamd_bin_query_batch **batch_io);
/* A batch of scalar queries.  The reference has NO counterpart; DESIGN.md 3.2d is the specification.  Query q of the batch
 * is exactly what qamd_bin_encode_query_scalar gives for row q of `queries` (a = max |q_i| per query, never across the
 * batch; NaN, +-inf and the all-zero query as there), and every batch call below - qamd_bin_score_batch, _score_ids_batch,
 * _topk_batch, _topk_batch_rescored - gives for it, bit for bit, what the single-query call gives for that query.  bits = 1
 * is qamd_bin_encode_query_batch; other values than 1, 4, 8 and the dims qamd_bin_encode_query_scalar refuses are
 * QAMD_ERR_ARGUMENTS.  *batch_io is reused as by qamd_bin_encode_query_batch and may change its bit count from call to
 * call.  From 5 (score_batch) / 12 (topk_batch) queries on, on rows of whole 16-byte pieces, 64 .. 4992 bits, a scalar batch is one int8
 * contraction per 32 / 64 queries on the matrix cores (bin_gemm_rs_kernel); elsewhere its queries are scanned one by one.
 * Out of scope: the qamd_bin_sharded_* query types (binary-only), bench.py (it measures binary batches) and any tuning of
 * the int8 kernel.  Measured against a loop of single-query calls (profiles/bin_scalar_batch.txt, 50M x 1024): 3.9 - 4.4 x
 * at 8 queries (score_batch), 12 - 18 x from 32 queries on (both calls); the two thresholds are the binary route's and
 * batches of 2 .. 7 (topk_batch: 2 .. 11) queries have not been timed on the matrix cores. */
QAMD_API qamd_status qamd_bin_encode_query_batch_scalar(const qamd_bin *h, const float *queries, uint64_t n_queries,
                                                        uint64_t qdim, qamd_mem queries_mem, uint32_t bits, void *stream,
                                                        qamd_bin_query_batch **batch_io);
/* A batch of weighted scalar queries: query q is exactly what qamd_bin_encode_query_scalar_w gives for row
 * q of `queries` (a per query), and every batch call gives for it what the single-query call gives.  The matrix-core
 * image holds one int8 per bit position of a row (d_i at byte i and byte dim + i) and C = 2 sum c_i, so the gates and
 * routes above hold with code_bits for dim: rows of 64 .. 4992 bits, that is dim <= 2496.  On a one-bit handle the call
 * is qamd_bin_encode_query_batch_scalar. */
QAMD_API qamd_status qamd_bin_encode_query_batch_scalar_w(const qamd_bin *h, const float *queries, uint64_t n_queries,
                                                          uint64_t qdim, qamd_mem queries_mem, uint32_t bits, void *stream,
                                                          qamd_bin_query_batch **batch_io);
/* No counterpart in the reference: *bits = bits per query dimension (1 for a batch from
 * qamd_bin_encode_query_batch), *n_queries = the queries it holds.  Either pointer may be NULL. */
QAMD_API qamd_status qamd_bin_query_batch_info(const qamd_bin_query_batch *b, uint32_t *bits, uint64_t *n_queries);
/* Query q of the batch as qamd_bin_query_read gives a single query: *len = bits x row bytes, plane 0 first (one row of
 * bits for a binary batch).  For tests and bindings; synchronises. */
QAMD_API qamd_status qamd_bin_query_batch_read(const qamd_bin_query_batch *b, uint64_t q, uint8_t *bits,
                                               uint64_t capacity, uint64_t *len);
/* Which kernel qamd_bin_score_batch (k = 0) or the filter of qamd_bin_topk_batch (k > 0) takes for THIS store and batch,
 * binary or scalar, as a static string: "bin_gemm_rs_kernel" (int8 matrix cores), "bin_gemm_rs4_kernel" /
 * "bin_gemm_qs4_kernel" (FP4 matrix cores: binary batches only), "bin_scan_multi_kernel" (2 .. 8 binary queries per pass
 * over the rows), or the per-query routes "bin_scan_kernel", "bin_words_kernel" (rows that are not whole 16-byte pieces,
 * or longer than 64 of them) and, for k > 0 on small stores, "bin_topk_small_kernel".  NULL for a batch that does not
 * belong to the store.  For measurement harnesses, as qamd_pq_scan_kernel: the entry points and this accessor call the
 * same routing predicates. */
QAMD_API const char *qamd_bin_batch_kernel(const qamd_bin *h, const qamd_bin_query_batch *b, uint32_t k);
QAMD_API void qamd_bin_query_batch_free(qamd_bin_query_batch *b);
/* out[q * count + i] = score_point(query q, i). */
QAMD_API qamd_status qamd_bin_score_batch(const qamd_bin *h, const qamd_bin_query_batch *b, float *out,
                                          qamd_mem out_mem, void *stream);
/* score_point for many (query, id list) pairs in one launch; as qamd_u8_score_ids_batch. */
QAMD_API qamd_status qamd_bin_score_ids_batch(const qamd_bin *h, const qamd_bin_query_batch *b,
                                              const uint32_t *list_offsets, uint32_t n_lists, const uint32_t *ids,
                                              uint64_t n_ids, qamd_mem lists_mem, float *out, qamd_mem out_mem,
                                              void *stream);
QAMD_API qamd_status qamd_bin_topk_batch(const qamd_bin *h, const qamd_bin_query_batch *b, uint32_t k,
                                         int largest, uint32_t *out_ids, float *out_scores,
                                         qamd_mem out_mem, void *stream);

/* ===================================================================================
 * Product quantizer — quantization/src/encoded_vectors_pq.rs
 * =================================================================================== */
typedef struct qamd_pq qamd_pq;             /* EncodedVectorsPQ<TStorage> (:27-30) */
typedef struct qamd_pq_query qamd_pq_query; /* EncodedQueryPQ{lut}        (:35-37) */

#define QAMD_PQ_CENTROIDS 256 /* CENTROIDS_COUNT (:25) */

/* get_quantized_vector_size (:109-114) == number of chunks. */
QAMD_API uint64_t qamd_pq_quantized_vector_size(const qamd_vector_parameters *vp,
                                                uint64_t chunk_size);
/* EncodedVectorsPQ::encode (:56-107).  centroids: NULL => find_centroids (:278-342)
 * runs (count <= 256: the vectors themselves, exactly as :290-297; otherwise k-means on a
 * 10 000-row sample, kmeans.rs).  The reference picks the sample rows at random (:300-302) and
 * re-seeds an empty cluster from thread_rng (kmeans.rs:111-118); here the sample is the evenly
 * strided rows floor(k * count / S) and the re-seed a fixed hash.  Everything else -- assignment,
 * f64 sums split over `max_kmeans_threads` contiguous row ranges and merged in worker order
 * (kmeans.rs:77-107), f32 shift sum, stopping rule -- is the reference's arithmetic in the
 * reference's order: given the same sample rows and no empty cluster the centroids are
 * bit-identical.  Non-NULL centroids: 256 x dim f32, centroid-major (Metadata.centroids,
 * :39-44), host memory; encode_storage (:136-226) then runs with them. */
QAMD_API qamd_status qamd_pq_encode(const float *data, qamd_mem data_mem,
                                    const qamd_vector_parameters *vp, uint64_t chunk_size,
                                    const float *centroids, uint32_t max_kmeans_threads,
                                    qamd_stop_fn stop, void *stop_user, void *stream,
                                    qamd_pq **out);
/* How the last k-means went: iterations of the slowest chunk (0: centroids were given or
 * count <= 256) and the number of empty-cluster re-seeds (0 => centroid parity holds, see above). */
QAMD_API qamd_status qamd_pq_kmeans_info(const qamd_pq *h, uint32_t *iterations, uint32_t *empty_clusters);
/* Which kernel the whole-store scan (score_all / topk; the caller loop of demos/src/ann_benchmark.rs:245-252 over
 * score_point, encoded_vectors_pq.rs:549-561) takes for THIS store, as a static string - "pq_scan_skew_kernel" (rows of
 * 16 .. 128 chunks with m % 4 == 0), "pq_scan_skew_kernel<SLICED>" (longer rows with m % 32 == 0: one launch per LUT slice of
 * the store's planar scan image), "pq_scan_fast_kernel" (other row lengths), "pq_scan_kernel" (fewer than 4096 rows) - and
 * in *n_launches how many launches one scan is.  For measurement harnesses: bench.py names the kernel it times and picks
 * its roofline bound from this instead of re-deriving the library's dispatch.  A store of at least 2^28 rows keeps no
 * planar scan image, and a store of at least 2^30 rows does not use pq_scan_skew_kernel: both then take
 * "pq_scan_fast_kernel" (rows of m > 144 chunks in ceil(m / 128) launches). */
QAMD_API const char *qamd_pq_scan_kernel(const qamd_pq *h, uint32_t *n_launches);
/* Streaming form (the reference walks its iterator twice: find_centroids :278-342, then
 * encode_storage :136-226): begin, observe every vector once (skipped when centroids are given),
 * push every vector again in the same order, finish.  See qamd_u8_encoder_*. */
typedef struct qamd_pq_encoder qamd_pq_encoder;
QAMD_API qamd_status qamd_pq_encoder_begin(const qamd_vector_parameters *vp, uint64_t chunk_size,
                                           const float *centroids, uint32_t max_kmeans_threads,
                                           qamd_stop_fn stop, void *stop_user, void *stream,
                                           qamd_pq_encoder **out);
QAMD_API qamd_status qamd_pq_encoder_observe(qamd_pq_encoder *e, const float *batch, uint64_t n_rows,
                                             qamd_mem batch_mem);
QAMD_API qamd_status qamd_pq_encoder_push(qamd_pq_encoder *e, const float *batch, uint64_t n_rows,
                                          qamd_mem batch_mem);
QAMD_API qamd_status qamd_pq_encoder_finish(qamd_pq_encoder *e, qamd_pq **out);
QAMD_API void qamd_pq_encoder_abort(qamd_pq_encoder *e);

/* find_centroids (encoded_vectors_pq.rs:278-342) ON ITS OWN: the 256 x dim centroids qamd_pq_encode would train for
 * `data` (vp->count rows), written to host memory `centroids`.  For a host that holds the rows in several places: the
 * k-means sample is the rows floor(k * count / S), k < S = min(10 000, count) (the reference draws a random Permutor
 * sample, :300-307); the holders gather exactly those rows, in k order, to one of them, which calls this with
 * vp->count = S and broadcasts the result; every holder then encodes its rows with `centroids` given.  count <= 256:
 * the vectors themselves, zero-filled (:290-297).  iterations / empty_clusters as qamd_pq_kmeans_info (may be NULL). */
QAMD_API qamd_status qamd_pq_find_centroids(const float *data, qamd_mem data_mem, const qamd_vector_parameters *vp,
                                            uint64_t chunk_size, uint32_t max_kmeans_threads, qamd_stop_fn stop,
                                            void *stop_user, void *stream, float *centroids, uint32_t *iterations,
                                            uint32_t *empty_clusters);
QAMD_API qamd_status qamd_pq_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                       const qamd_vector_parameters *vp, uint64_t chunk_size,
                                       const float *centroids, void *stream, qamd_pq **out);
QAMD_API qamd_status qamd_pq_export_rows(const qamd_pq *h, uint8_t *rows, qamd_mem rows_mem,
                                         void *stream);
/* Ranged form (storage_builder.push_vector_data, encoded_vectors_pq.rs:136-226 via
 * encoded_storage.rs:17-25); see qamd_u8_export_rows_range. */
QAMD_API qamd_status qamd_pq_export_rows_range(const qamd_pq *h, uint64_t first_row, uint64_t n_rows,
                                               uint8_t *rows, qamd_mem rows_mem, void *stream);
/* Metadata.centroids (256 x dim f32, host). */
QAMD_API qamd_status qamd_pq_get_centroids(const qamd_pq *h, float *centroids);
QAMD_API qamd_status qamd_pq_save(const qamd_pq *h, const char *data_path, const char *meta_path);
QAMD_API qamd_status qamd_pq_load(const char *data_path, const char *meta_path,
                                  const qamd_vector_parameters *vp, qamd_pq **out);
/* encode_query (:525-547): builds the chunk-major LUT (what qamd_pq_query_read returns: EncodedQueryPQ.lut).  For stores
 * whose whole-store scan runs without LDS bank conflicts (m % 32 == 0) the object also keeps a [code][chunk] copy. */
QAMD_API qamd_status qamd_pq_encode_query(const qamd_pq *h, const float *query, uint64_t qdim,
                                          qamd_mem query_mem, void *stream,
                                          qamd_pq_query **query_io);
QAMD_API qamd_status qamd_pq_query_read(const qamd_pq_query *q, float *lut, uint64_t capacity,
                                        uint64_t *len);
QAMD_API void qamd_pq_query_free(qamd_pq_query *q);
/* score_point (:549-561 -> score_point_sse :405-440 summation order), score_internal (:566-593). */
QAMD_API qamd_status qamd_pq_score_point(const qamd_pq *h, const qamd_pq_query *q, uint32_t i,
                                         float *out);
QAMD_API qamd_status qamd_pq_score_internal(const qamd_pq *h, uint32_t i, uint32_t j, float *out);
/* Bursts of pairs in one launch (score_internal :566-593: both rows decoded to centroid sub-vectors, the
 * chunk metrics summed in chunk order); arguments as qamd_u8_score_internal_ids / _ids_batch, the null id list
 * (ids == NULL: the rows 0 .. n_ids - 1) as stated at qamd_u8_score_internal_ids and qamd_u8_score_internal_ids_batch;
 * with a null list a handle without centroids is QAMD_ERR_ARGUMENTS. */
QAMD_API qamd_status qamd_pq_score_internal_ids(const qamd_pq *h, uint32_t i, const uint32_t *ids, uint64_t n_ids,
                                                qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_score_internal_ids_batch(const qamd_pq *h, const uint32_t *rows,
                                                      const uint32_t *list_offsets, uint32_t n_lists,
                                                      const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem,
                                                      float *out, qamd_mem out_mem, void *stream);
/* score_internal (:566-593) against the whole store, contract as qamd_u8_score_internal_all / _topk_internal: row i's table
 * of centroid-to-centroid chunk metrics, summed per row strictly in chunk order and negated (invert) once after the sum -
 * not the four-lane order of score_point. */
QAMD_API qamd_status qamd_pq_score_internal_all(const qamd_pq *h, uint32_t i, float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_topk_internal(const qamd_pq *h, uint32_t i, uint32_t k, int largest,
                                           uint32_t *out_ids, float *out_scores, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_score_all(const qamd_pq *h, const qamd_pq_query *q, float *out,
                                       qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_score_ids(const qamd_pq *h, const qamd_pq_query *q,
                                       const uint32_t *ids, uint64_t n_ids, qamd_mem ids_mem,
                                       float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_topk(const qamd_pq *h, const qamd_pq_query *q, uint32_t k,
                                  int largest, uint32_t *out_ids, float *out_scores,
                                  qamd_mem out_mem, void *stream);
QAMD_API void qamd_pq_free(qamd_pq *h);

/* Many queries at once (BASELINE config 4's PQ leg): all LUTs are built by one launch, the per-query
 * LDS-LUT scans are enqueued back to back (the scan is LDS-gather-bound, one LUT fills the LDS, so
 * queries cannot share a pass); topk_batch reads statuses back once per 32 queries and synchronises
 * the stream.  Bit-identical to the single-query calls. */
typedef struct qamd_pq_query_batch qamd_pq_query_batch; /* n x EncodedQueryPQ */
QAMD_API qamd_status qamd_pq_encode_query_batch(const qamd_pq *h, const float *queries, uint64_t n_queries,
                                                uint64_t qdim, qamd_mem queries_mem, void *stream,
                                                qamd_pq_query_batch **batch_io);
QAMD_API void qamd_pq_query_batch_free(qamd_pq_query_batch *b);
QAMD_API qamd_status qamd_pq_score_batch(const qamd_pq *h, const qamd_pq_query_batch *b, float *out,
                                         qamd_mem out_mem, void *stream);
/* score_point for many (query, id list) pairs in one launch (LUT l for list l); as qamd_u8_score_ids_batch. */
QAMD_API qamd_status qamd_pq_score_ids_batch(const qamd_pq *h, const qamd_pq_query_batch *b,
                                             const uint32_t *list_offsets, uint32_t n_lists, const uint32_t *ids,
                                             uint64_t n_ids, qamd_mem lists_mem, float *out, qamd_mem out_mem,
                                             void *stream);
/* Top-k of every query of the batch, as qamd_pq_topk.  A device that does not report 256 CUs (a partitioned MI355X) runs
 * the filter passes query by query, never side by side; so does a store without a planar scan image (2^28 rows and more)
 * whose rows have more than 144 chunks.  The answer is the same either way. */
QAMD_API qamd_status qamd_pq_topk_batch(const qamd_pq *h, const qamd_pq_query_batch *b, uint32_t k,
                                        int largest, uint32_t *out_ids, float *out_scores,
                                        qamd_mem out_mem, void *stream);

/* ===================================================================================
 * Row-sharded stores: ONE process, several GPUs of a node behind one handle.
 *
 * No reference counterpart (the crate is single-device); the caller it serves is the one
 * process of demos/src/ann_benchmark.rs:245-260 (score every row, keep the best 30:
 * ann_benchmark_data.rs:151-167).  Shard g of G owns rows [g*N/G, (g+1)*N/G) as an ordinary
 * handle on devices[g]; global row id = shard base + local id; metadata is replicated.
 * `devices` may repeat a device (logical shards on one GPU).  Every call is synchronous: it
 * posts one job per shard (served by worker threads bound to the shard's device, each with its own
 * stream), waits for ITS jobs, and does ONE exchange -- score_all: each shard's scores land in their
 * slice of `out` (host: one D2H per GPU; device: peer copy of 4 B/row over xGMI to the device owning
 * `out`); topk: G*k (id, score) pairs are peer-copied to devices[0] and merged by one kernel there
 * with the single-handle ordering (best first, ties to the lower global id).  Results are
 * bit-identical to the same call on a single handle holding all rows.  Host buffers or device
 * buffers; a device output of topk must live on devices[0].
 * Threads: encode_query / score_all / topk / topk_batch may be called from any number of threads on
 * one sharded handle at once, like the `&self` methods they stand for (encoded_vectors.rs:21-35):
 * there is no per-handle lock, the callers' jobs interleave on the shards' queues and each call
 * leases its own exchange buffers.
 * `stream`: the hipStream_t that produced the call's device INPUT buffers / still uses the buffers
 * its device OUTPUTS overwrite (NULL = the null stream of the device owning the buffer).  It is
 * synchronised on entry when a buffer of the call is device memory (the workers run on their own
 * streams, which nothing else orders against the caller's); ignored for host buffers.  At return
 * every output is complete.
 * Deployment knob: the environment variable QAMD_SHARD_LANES (1..8, default 3) is the number of worker threads
 * ("lanes") per shard, read once per process: while one lane waits for its kernel the others enqueue.  It is the
 * only environment variable the product library reads.
 * Peer access: the exchanges between a shard's device and devices[0] are device-to-device copies.  At construction
 * the handle tries hipDeviceEnablePeerAccess in both directions for every such pair and RECORDS the outcome
 * (qamd_*_sharded_peer_access); where it is unavailable or fails the same hipMemcpyAsync calls still work, staged
 * through host memory by the runtime - slower, never wrong.
 * =================================================================================== */
/* How shard g's device reaches devices[0] (qamd_*_sharded_peer_access): */
typedef enum {
    QAMD_PEER_SAME_DEVICE = 0, /* the shard lives on devices[0] itself (or is a logical shard of it) */
    QAMD_PEER_ENABLED = 1,     /* direct peer copies (xGMI) in both directions */
    QAMD_PEER_UNAVAILABLE = 2, /* hipDeviceCanAccessPeer said no: copies are staged by the runtime */
    QAMD_PEER_FAILED = 3       /* hipDeviceEnablePeerAccess failed (*reason = the HIP error): staged copies */
} qamd_peer_state;
typedef struct qamd_u8_sharded qamd_u8_sharded;
typedef struct qamd_u8_sharded_query qamd_u8_sharded_query;
typedef struct qamd_u8_sharded_query_batch qamd_u8_sharded_query_batch;
/* encode (encoded_vectors_u8.rs:34-140): global min/max (or quantile interval) first, then
 * every shard quantizes its own rows.  `data` is host memory or device memory of any one GPU. */
QAMD_API qamd_status qamd_u8_sharded_encode(const float *data, qamd_mem data_mem,
                                            const qamd_vector_parameters *vp, const float *quantile,
                                            const float *alpha_offset, qamd_stop_fn stop, void *stop_user,
                                            const int *devices, uint32_t n_shards, void *stream,
                                             qamd_u8_sharded **out);
QAMD_API qamd_status qamd_u8_sharded_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                               const qamd_u8_metadata *meta, const int *devices,
                                               uint32_t n_shards, void *stream,
                                             qamd_u8_sharded **out);
QAMD_API uint32_t qamd_u8_sharded_shard_count(const qamd_u8_sharded *h);
/* *state = a qamd_peer_state for shard g; *reason (may be NULL) = a static or handle-owned string saying why. */
QAMD_API qamd_status qamd_u8_sharded_peer_access(const qamd_u8_sharded *h, uint32_t g, int *state, const char **reason);
/* Borrow shard g (owned by the sharded handle): its single-device handle, first global row, device.  The pointer is
 * `const` (here and for the binary and PQ handles): a shard cannot be upserted or reserved, the row bases are fixed. */
QAMD_API qamd_status qamd_u8_sharded_shard(const qamd_u8_sharded *h, uint32_t g, const qamd_u8 **shard,
                                           uint64_t *row_begin, int *device);
QAMD_API qamd_status qamd_u8_sharded_get_metadata(const qamd_u8_sharded *h, qamd_u8_metadata *out);
QAMD_API qamd_status qamd_u8_sharded_encode_query(qamd_u8_sharded *h, const float *query, uint64_t qdim,
                                                  qamd_mem query_mem, void *stream,
                                             qamd_u8_sharded_query **query_io);
QAMD_API void qamd_u8_sharded_query_free(qamd_u8_sharded_query *q);
QAMD_API qamd_status qamd_u8_sharded_score_all(qamd_u8_sharded *h, const qamd_u8_sharded_query *q, float *out,
                                               qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_u8_sharded_topk(qamd_u8_sharded *h, const qamd_u8_sharded_query *q, uint32_t k,
                                          int largest, uint32_t *out_ids, float *out_scores,
                                          qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_u8_sharded_encode_query_batch(qamd_u8_sharded *h, const float *queries,
                                                        uint64_t n_queries, uint64_t qdim,
                                                        qamd_mem queries_mem, void *stream,
                                             qamd_u8_sharded_query_batch **batch_io);
QAMD_API void qamd_u8_sharded_query_batch_free(qamd_u8_sharded_query_batch *b);
/* n_queries x k; shards x k <= 8192. */
QAMD_API qamd_status qamd_u8_sharded_topk_batch(qamd_u8_sharded *h, const qamd_u8_sharded_query_batch *b,
                                                uint32_t k, int largest, uint32_t *out_ids,
                                                float *out_scores, qamd_mem out_mem, void *stream);
QAMD_API void qamd_u8_sharded_free(qamd_u8_sharded *h);

typedef struct qamd_bin_sharded qamd_bin_sharded;
typedef struct qamd_bin_sharded_query qamd_bin_sharded_query;
QAMD_API qamd_status qamd_bin_sharded_encode(const float *data, qamd_mem data_mem,
                                             const qamd_vector_parameters *vp, qamd_bits_store store,
                                             qamd_stop_fn stop, void *stop_user, const int *devices,
                                             uint32_t n_shards, void *stream,
                                             qamd_bin_sharded **out);
QAMD_API qamd_status qamd_bin_sharded_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                                const qamd_vector_parameters *vp, qamd_bits_store store,
                                                const int *devices, uint32_t n_shards, void *stream,
                                             qamd_bin_sharded **out);
QAMD_API uint32_t qamd_bin_sharded_shard_count(const qamd_bin_sharded *h);
/* *state = a qamd_peer_state for shard g; *reason (may be NULL) = a static or handle-owned string saying why. */
QAMD_API qamd_status qamd_bin_sharded_peer_access(const qamd_bin_sharded *h, uint32_t g, int *state, const char **reason);
QAMD_API qamd_status qamd_bin_sharded_shard(const qamd_bin_sharded *h, uint32_t g, const qamd_bin **shard,
                                            uint64_t *row_begin, int *device);
QAMD_API qamd_status qamd_bin_sharded_encode_query(qamd_bin_sharded *h, const float *query, uint64_t qdim,
                                                   qamd_mem query_mem, void *stream,
                                             qamd_bin_sharded_query **query_io);
QAMD_API void qamd_bin_sharded_query_free(qamd_bin_sharded_query *q);
QAMD_API qamd_status qamd_bin_sharded_score_all(qamd_bin_sharded *h, const qamd_bin_sharded_query *q,
                                                float *out, qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_bin_sharded_topk(qamd_bin_sharded *h, const qamd_bin_sharded_query *q, uint32_t k,
                                           int largest, uint32_t *out_ids, float *out_scores,
                                           qamd_mem out_mem, void *stream);
typedef struct qamd_bin_sharded_query_batch qamd_bin_sharded_query_batch;
QAMD_API qamd_status qamd_bin_sharded_encode_query_batch(qamd_bin_sharded *h, const float *queries,
                                                         uint64_t n_queries, uint64_t qdim,
                                                         qamd_mem queries_mem, void *stream,
                                             qamd_bin_sharded_query_batch **batch_io);
QAMD_API void qamd_bin_sharded_query_batch_free(qamd_bin_sharded_query_batch *b);
QAMD_API qamd_status qamd_bin_sharded_topk_batch(qamd_bin_sharded *h, const qamd_bin_sharded_query_batch *b,
                                                 uint32_t k, int largest, uint32_t *out_ids,
                                                 float *out_scores, qamd_mem out_mem, void *stream);
QAMD_API void qamd_bin_sharded_free(qamd_bin_sharded *h);

typedef struct qamd_pq_sharded qamd_pq_sharded;
typedef struct qamd_pq_sharded_query qamd_pq_sharded_query;
/* centroids NULL: find_centroids runs once (on the device holding `data`, else devices[0]). */
QAMD_API qamd_status qamd_pq_sharded_encode(const float *data, qamd_mem data_mem,
                                            const qamd_vector_parameters *vp, uint64_t chunk_size,
                                            const float *centroids, uint32_t max_kmeans_threads,
                                            qamd_stop_fn stop, void *stop_user, const int *devices,
                                            uint32_t n_shards, void *stream,
                                             qamd_pq_sharded **out);
QAMD_API qamd_status qamd_pq_sharded_from_rows(const uint8_t *rows, qamd_mem rows_mem,
                                               const qamd_vector_parameters *vp, uint64_t chunk_size,
                                               const float *centroids, const int *devices,
                                               uint32_t n_shards, void *stream,
                                             qamd_pq_sharded **out);
QAMD_API uint32_t qamd_pq_sharded_shard_count(const qamd_pq_sharded *h);
/* *state = a qamd_peer_state for shard g; *reason (may be NULL) = a static or handle-owned string saying why. */
QAMD_API qamd_status qamd_pq_sharded_peer_access(const qamd_pq_sharded *h, uint32_t g, int *state, const char **reason);
QAMD_API qamd_status qamd_pq_sharded_shard(const qamd_pq_sharded *h, uint32_t g, const qamd_pq **shard,
                                           uint64_t *row_begin, int *device);
QAMD_API qamd_status qamd_pq_sharded_get_centroids(const qamd_pq_sharded *h, float *centroids);
QAMD_API qamd_status qamd_pq_sharded_encode_query(qamd_pq_sharded *h, const float *query, uint64_t qdim,
                                                  qamd_mem query_mem, void *stream,
                                             qamd_pq_sharded_query **query_io);
QAMD_API void qamd_pq_sharded_query_free(qamd_pq_sharded_query *q);
QAMD_API qamd_status qamd_pq_sharded_score_all(qamd_pq_sharded *h, const qamd_pq_sharded_query *q, float *out,
                                               qamd_mem out_mem, void *stream);
QAMD_API qamd_status qamd_pq_sharded_topk(qamd_pq_sharded *h, const qamd_pq_sharded_query *q, uint32_t k,
                                          int largest, uint32_t *out_ids, float *out_scores,
                                          qamd_mem out_mem, void *stream);
typedef struct qamd_pq_sharded_query_batch qamd_pq_sharded_query_batch;
QAMD_API qamd_status qamd_pq_sharded_encode_query_batch(qamd_pq_sharded *h, const float *queries,
                                                        uint64_t n_queries, uint64_t qdim,
                                                        qamd_mem queries_mem, void *stream,
                                             qamd_pq_sharded_query_batch **batch_io);
QAMD_API void qamd_pq_sharded_query_batch_free(qamd_pq_sharded_query_batch *b);
QAMD_API qamd_status qamd_pq_sharded_topk_batch(qamd_pq_sharded *h, const qamd_pq_sharded_query_batch *b,
                                                uint32_t k, int largest, uint32_t *out_ids,
                                                float *out_scores, qamd_mem out_mem, void *stream);
QAMD_API void qamd_pq_sharded_free(qamd_pq_sharded *h);

/* ===================================================================================
 * Rescoring with the original f32 vectors.
 *
 * The caller of the reference over-fetches candidates from a quantized scan, scores them again
 * with the original vectors and keeps the best k (demos/src/ann_benchmark_data.rs:151-185 counts
 * what the quantized scan alone recovers).  The exact score is `DistanceType::distance`
 * (quantization/src/encoded_vectors.rs:37-45, pub): the SEQUENTIAL f32 sum, from +0.0, of a*b
 * (Dot), |a-b| (L1) or (a-b)*(a-b) (L2) over the dimensions, a = query, b = row -- negated when
 * `invert` is set, which is the quantity every quantizer's score approximates, so `largest` means
 * here what it means for the *_topk of the quantized store.  Every score is that sum bit for bit
 * (no FMA contraction, no reassociation, subnormals kept).
 *
 * The originals may be kept as f16 or bf16 (qamd_f32_from_data_typed): half the resident bytes
 * and half the bytes of the row gather.  The handle carries its element type; queries stay f32.
 * A score is then the SAME function, `DistanceType::distance` (encoded_vectors.rs:37-45), of the
 * f32 query and the row WIDENED EXACTLY to f32: the sequential f32 sum from +0.0, each product or
 * difference rounded to f32 before its add, negated for `invert` -- bit for bit, no tolerance.
 * Widening loses nothing: every f16 and bf16 value is an f32 value.  f16 subnormals widen to f32
 * normals and are not flushed; bf16 subnormals are f32 subnormals and are kept.
 *
 * Out of scope: sharded handles (re-rank per shard with the shard's rows, or after the merge on
 * one device); encoders that read f16 / bf16 source data (the quantizers encode from f32);
 * originals resident in host memory (host `data` is copied to HBM); bench.py does not measure
 * these calls.
 * =================================================================================== */
typedef struct qamd_f32 qamd_f32; /* count x dim rows (f32, f16 or bf16) in HBM + VectorParameters (:13-19) */

/* Element types of the originals.  F16 = IEEE binary16, BF16 = the upper 16 bits of an f32. */
typedef enum { QAMD_DTYPE_F32 = 0, QAMD_DTYPE_F16 = 1, QAMD_DTYPE_BF16 = 2 } qamd_dtype;

/* `data`: count x dim f32, row-major.  borrow = 0 copies it into library-owned HBM (host or
 * device source).  borrow = 1 keeps the CALLER's pointer: legal only for device memory of the
 * current device, which the caller keeps alive and unchanged while the handle is used (a 30 GB
 * tensor is not duplicated); with host memory it returns QAMD_ERR_ARGUMENTS.  Rows need no
 * alignment beyond 4 bytes.  vp->distance_type / invert fix the metric and its sign
 * (encoded_vectors.rs:37-45); count < 2^32, dim < 2^31. */
QAMD_API qamd_status qamd_f32_from_data(const float *data, qamd_mem data_mem,
                                        const qamd_vector_parameters *vp, int borrow, void *stream,
                                        qamd_f32 **out);
/* The same with element types: `data` holds count x dim values of `data_dtype`, the handle keeps
 * them as `store_dtype`.  Allowed pairs: data_dtype == store_dtype (any of the three: the bytes are
 * copied or borrowed as they are), F32 -> F16 and F32 -> BF16; any other pair returns
 * QAMD_ERR_ARGUMENTS.  The narrowing pairs run on the device, piece by piece through the staging
 * buffer for host data: round to nearest even, overflow to +-inf, NaN stays NaN (quiet), results
 * in the subnormal range of the store type are kept.  borrow = 1 keeps its rules above, needs
 * data_dtype == store_dtype and a pointer aligned to the element size.  qamd_f32_from_data is
 * (F32, F32).  Every qamd_f32_* scoring call and the six *_rescored calls take such a handle:
 * scores are `DistanceType::distance` (encoded_vectors.rs:37-45) of the f32 query and the row
 * widened exactly to f32. */
QAMD_API qamd_status qamd_f32_from_data_typed(const void *data, qamd_dtype data_dtype, qamd_mem data_mem,
                                              const qamd_vector_parameters *vp, qamd_dtype store_dtype,
                                              int borrow, void *stream, qamd_f32 **out);
QAMD_API qamd_status qamd_f32_get_parameters(const qamd_f32 *h, qamd_vector_parameters *out);
/* The element type the handle keeps its rows in. */
QAMD_API qamd_status qamd_f32_get_dtype(const qamd_f32 *h, qamd_dtype *out);
QAMD_API void qamd_f32_free(qamd_f32 *h);

/* out[p] = distance(query, row ids[p]) (encoded_vectors.rs:37-45), sign flipped for invert.
 * Buffer rules of the quantizers' *_score_ids: host ids are validated (an id >= count returns
 * QAMD_ERR_OUT_OF_RANGE), a device id >= count scores NaN; ids and out both in device memory and
 * a device query only enqueue.  A host query is copied first (synchronises `stream`).
 *
 * The whole store (score_all): a NULL id list stands for the rows 0, 1, ..., n_ids - 1, with n_ids <= count --
 * `ids = NULL` makes out[j] the exact score of row j for j < n_ids, and n_ids = count scores every row.  The rows are
 * then read in order by one scan (16-byte loads where the rows allow them) instead of gathered by id; every score is
 * the list form's, bit for bit.  `ids_mem` is ignored.  n_ids > count returns QAMD_ERR_OUT_OF_RANGE before any launch;
 * n_ids == 0 stays QAMD_OK.  A device query with a device `out` only enqueues; a host `out` goes through the calling
 * thread's score workspace and synchronises `stream`.  qamd_f32_rerank and qamd_f32_rerank_batch take the same
 * convention (below); qamd_f32_score_ids_batch does not.  Out of scope for the null-list forms: sharded handles (scan
 * each shard's originals and merge with qamd_topk_merge); qamd_f32_score_ids_batch, which keeps requiring its lists;
 * a scores-of-all-queries output (a batch returns its k best only: call this once per query for the scores);
 * *_topk_rescored and *_topk_batch_rescored, which are unchanged. */
QAMD_API qamd_status qamd_f32_score_ids(const qamd_f32 *h, const float *query, uint64_t qdim,
                                        qamd_mem query_mem, const uint32_t *ids, uint64_t n_ids,
                                        qamd_mem ids_mem, float *out, qamd_mem out_mem, void *stream);
/* Many (query, id list) pairs in one launch, as *_score_ids_batch: list l =
 * ids[list_offsets[l] .. list_offsets[l + 1]) is scored against query l of `queries`
 * ([n_queries][qdim] f32, n_lists <= n_queries); out[p] = distance(query l, row ids[p])
 * (encoded_vectors.rs:37-45).  Device lists need a device output.  The lists are required here: the null-list
 * convention of qamd_f32_score_ids does not extend to this call (null lists with n_ids > 0 return QAMD_ERR_ARGUMENTS). */
QAMD_API qamd_status qamd_f32_score_ids_batch(const qamd_f32 *h, const float *queries,
                                              uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                                              const uint32_t *list_offsets, uint32_t n_lists,
                                              const uint32_t *ids, uint64_t n_ids, qamd_mem lists_mem,
                                              float *out, qamd_mem out_mem, void *stream);

/* The best k of the given ids by exact score (encoded_vectors.rs:37-45): ordering contract of the
 * *_topk entry points -- best first, ties to the lower id, padded with id 0xFFFFFFFF and -inf
 * (largest) / +inf when fewer than k ids are given.  k <= 1024, n_ids <= 8192 (the capacity of
 * the candidate sort).  Id 0xFFFFFFFF, the padding *_topk writes, is skipped; any other host id
 * >= count returns QAMD_ERR_OUT_OF_RANGE, such a device id takes part with a NaN score.  An id
 * listed twice is returned twice.  Order of scores: as stated at qamd_u8_topk - one total order on the f32 bit
 * pattern (ascending -NaN < -inf < negative finite < -0 < +0 < positive finite < +inf < +NaN, equal bit patterns to
 * the lower id); exact scores of rows that hold inf or NaN, and the NaN of an id past the end, are ranked by it like
 * any other, and a returned score is the row's own score bits.  With every buffer in device memory the call only enqueues;
 * host outputs cost one download and synchronise `stream`.
 *
 * The whole store (an exact top-k): a NULL id list stands for the rows 0, 1, ..., n_ids - 1, with n_ids <= count --
 * `ids = NULL` returns the k best of the rows [0, n_ids) under the same ordering contract (the total order on score
 * bits, ties to the lower id, best first, padding 0xFFFFFFFF with -inf / +inf when k > n_ids), from one scan of the
 * rows and the exact select of *_topk over the calling thread's score workspace.  `ids_mem` is ignored; n_ids > count
 * returns QAMD_ERR_OUT_OF_RANGE before any launch.  The limit of 8192 ids holds only for a list that is given;
 * k <= 1024 holds for both.  This form may synchronise `stream` as *_topk does (host outputs always do).  Out of scope:
 * sharded handles; qamd_f32_score_ids_batch; a scores-of-all-queries output; *_topk_rescored, which is unchanged
 * (see qamd_f32_score_ids). */
QAMD_API qamd_status qamd_f32_rerank(const qamd_f32 *h, const float *query, uint64_t qdim,
                                     qamd_mem query_mem, const uint32_t *ids, uint32_t n_ids,
                                     qamd_mem ids_mem, uint32_t k, int largest, uint32_t *out_ids,
                                     float *out_scores, qamd_mem out_mem, void *stream);
/* The same for n_queries queries at once (encoded_vectors.rs:37-45): ids [n_queries][n_ids],
 * outputs [n_queries][k].  With `ids = NULL` every one of the n_queries queries is ranked against the rows [0, n_ids),
 * n_ids <= count (the convention of qamd_f32_rerank); the limit n_queries * n_ids < 2^32 of the list form does not
 * apply.  The queries go in groups of up to 8 that share one pass over the rows; a group's scores take
 * group * n_ids * 4 bytes of the calling thread's score workspace, and the group shrinks, down to 1 query, so that
 * this stays within 512 MiB (more only when one query's n_ids * 4 bytes alone exceed it) -- never
 * n_queries * n_ids. */
QAMD_API qamd_status qamd_f32_rerank_batch(const qamd_f32 *h, const float *queries, uint64_t n_queries,
                                           uint64_t qdim, qamd_mem queries_mem, const uint32_t *ids,
                                           uint32_t n_ids, qamd_mem ids_mem, uint32_t k, int largest,
                                           uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                           void *stream);

/* The fused call: rerank(orig, query_f32, ids of *_topk(h, q, candidates, largest), k) -- the
 * over-fetch and exact re-scoring of a caller of ann_benchmark_data.rs:151-185, scores by
 * encoded_vectors.rs:37-45.  `q` is the encoded form of `query_f32` (the caller encodes it as for
 * *_topk).  k <= candidates <= 1024.  `orig` must agree with `h` in count, dim, distance type,
 * invert and device, else QAMD_ERR_ARGUMENTS.  The candidate ids stay on the device (the calling
 * thread's workspace); host outputs cost one download.  Like *_topk, the call synchronises
 * `stream`.  Output contract as qamd_f32_rerank. */
QAMD_API qamd_status qamd_u8_topk_rescored(const qamd_u8 *h, const qamd_u8_query *q, const qamd_f32 *orig,
                                           const float *query_f32, uint64_t qdim, qamd_mem query_mem,
                                           uint32_t k, uint32_t candidates, int largest,
                                           uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                           void *stream);
QAMD_API qamd_status qamd_pq_topk_rescored(const qamd_pq *h, const qamd_pq_query *q, const qamd_f32 *orig,
                                           const float *query_f32, uint64_t qdim, qamd_mem query_mem,
                                           uint32_t k, uint32_t candidates, int largest,
                                           uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                           void *stream);
QAMD_API qamd_status qamd_bin_topk_rescored(const qamd_bin *h, const qamd_bin_query *q, const qamd_f32 *orig,
                                            const float *query_f32, uint64_t qdim, qamd_mem query_mem,
                                            uint32_t k, uint32_t candidates, int largest,
                                            uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                            void *stream);
/* The fused call over *_topk_batch (ann_benchmark_data.rs:151-185, encoded_vectors.rs:37-45):
 * queries_f32 [n_queries][qdim] are the f32 forms of the batch's queries, n_queries that of the
 * batch; outputs [n_queries][k]. */
QAMD_API qamd_status qamd_u8_topk_batch_rescored(const qamd_u8 *h, const qamd_u8_query_batch *b,
                                                 const qamd_f32 *orig, const float *queries_f32,
                                                 uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                                                 uint32_t k, uint32_t candidates, int largest,
                                                 uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                                 void *stream);
QAMD_API qamd_status qamd_pq_topk_batch_rescored(const qamd_pq *h, const qamd_pq_query_batch *b,
                                                 const qamd_f32 *orig, const float *queries_f32,
                                                 uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                                                 uint32_t k, uint32_t candidates, int largest,
                                                 uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                                 void *stream);
QAMD_API qamd_status qamd_bin_topk_batch_rescored(const qamd_bin *h, const qamd_bin_query_batch *b,
                                                  const qamd_f32 *orig, const float *queries_f32,
                                                  uint64_t n_queries, uint64_t qdim, qamd_mem queries_mem,
                                                  uint32_t k, uint32_t candidates, int largest,
                                                  uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                                  void *stream);

/* ===================================================================================
 * Upsert: overwrite and append rows of a built store, in place.
 *
 * The reference snapshot this library was written against has NO counterpart: its
 * EncodedVectors are immutable once `encode` returns.  Upstream has since gained
 * `upsert_vector(id, vector)` (encode with the store's existing parameters, write at `id`,
 * grow the storage when `id` is past the end); this header and DESIGN.md 3.9 are the
 * specification of the form kept here: one call for a contiguous row range.
 *
 * Range.  `data` holds n_rows x vp.dim values; row first_row + r becomes the encoding of
 *   data[r].  first_row <= count is required (a hole is QAMD_ERR_ARGUMENTS); rows below
 *   count are overwritten, rows at and past count extend the store: count and
 *   vector_parameters.count become max(count, first_row + n_rows) for *_get_metadata, save
 *   and the count check of *_topk_rescored.  n_rows == 0 is QAMD_OK and touches nothing.
 *   A new count above 0xFFFFFFFF is QAMD_ERR_ARGUMENTS.
 * Parameters are the store's own; nothing is learnt again.  u8: metadata alpha / offset
 *   (values outside the interval saturate as in the encoder; codes stay <= 127).  PQ: the
 *   handle's centroids.  Binary: one bit, or the handle's lo / hi thresholds.  f32: the
 *   handle's element type (f32 data is narrowed for f16 / bf16 stores; the source / store type
 *   pairs are those of qamd_f32_from_data_typed).
 * Refused with QAMD_ERR_ARGUMENTS: a u8 handle whose alpha is 0 (the metadata of an empty
 *   store: there is no interval to encode with), a PQ handle without centroids, a borrowed
 *   qamd_f32 (borrow = 1: the buffer is the caller's), a PQ store with a planar scan image
 *   (several LUT slices, m % 32 == 0) that would reach 2^28 rows (its row stride would change).
 *   Sharded handles and their shards cannot be upserted: qamd_*_sharded_shard hands out
 *   `const` pointers, and the sharded handle's row bases are fixed.
 * Derived images follow: the u8 offsets and 7-bit blocked scan image (kept when the store has
 *   one; if growing it fails the store drops it and serves from its byte codes: the call still
 *   succeeds), the PQ planar image, and the lazily gathered top-k pivot samples (discarded; the
 *   next query batch gathers them again).  Lane mode, encoding and thresholds are untouched.
 * Capacity.  A handle has room for *_capacity rows; every builder leaves capacity = count, so
 *   a handle that is never upserted allocates what it always did.  reserve(c) with
 *   c > capacity reallocates to c rows (internally round_up(c, 1024) + 1024, zero-filled past
 *   count) and copies the rows device to device; c <= capacity is a no-op.  An upsert that
 *   needs more than capacity first reserves max(needed, capacity + capacity / 2).  A failed
 *   allocation is QAMD_ERR_DEVICE and leaves the handle as it was.
 * Concurrency.  upsert and reserve are WRITERS: no other call on the same handle may be
 *   running, or enqueued and unfinished, when they start.  They return after the rows are in
 *   place (`stream` is synchronised).  Encoded queries and query batches made before an upsert
 *   stay valid.
 * =================================================================================== */
QAMD_API qamd_status qamd_u8_upsert(qamd_u8 *h, uint64_t first_row, const float *data, qamd_mem data_mem,
                                    uint64_t n_rows, void *stream);
QAMD_API qamd_status qamd_pq_upsert(qamd_pq *h, uint64_t first_row, const float *data, qamd_mem data_mem,
                                    uint64_t n_rows, void *stream);
QAMD_API qamd_status qamd_bin_upsert(qamd_bin *h, uint64_t first_row, const float *data, qamd_mem data_mem,
                                     uint64_t n_rows, void *stream);
QAMD_API qamd_status qamd_f32_upsert(qamd_f32 *h, uint64_t first_row, const void *data, qamd_dtype data_dtype,
                                     qamd_mem data_mem, uint64_t n_rows, void *stream);
QAMD_API qamd_status qamd_u8_reserve(qamd_u8 *h, uint64_t capacity_rows, void *stream);
QAMD_API qamd_status qamd_pq_reserve(qamd_pq *h, uint64_t capacity_rows, void *stream);
QAMD_API qamd_status qamd_bin_reserve(qamd_bin *h, uint64_t capacity_rows, void *stream);
QAMD_API qamd_status qamd_f32_reserve(qamd_f32 *h, uint64_t capacity_rows, void *stream);
/* Rows the handle has room for without reallocating (0 for a null handle; count for a borrowed qamd_f32). */
QAMD_API uint64_t qamd_u8_capacity(const qamd_u8 *h);
QAMD_API uint64_t qamd_pq_capacity(const qamd_pq *h);
QAMD_API uint64_t qamd_bin_capacity(const qamd_bin *h);
QAMD_API uint64_t qamd_f32_capacity(const qamd_f32 *h);

/* ===================================================================================
 * Selection over an existing score array (device memory), e.g. after a multi-GPU gather.
 * Same ordering contract as the *_topk entry points.
 * =================================================================================== */
QAMD_API qamd_status qamd_topk_scores(const float *scores_dev, uint64_t n, uint32_t k, int largest,
                                      uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                      void *stream);

/* The exchange step of a row-sharded top-k on its own, for callers that shard across PROCESSES
 * (one rank per GPU, quantization_amd/sharded.py over torch.distributed / RCCL): after the
 * all-gather of every rank's [n_queries][k] (local id, score) lists into device memory, one kernel
 * per query block merges them -- global id = row_bases[shard] + local id, best first, ties to the
 * lower global id: exactly what a single handle over all rows returns.
 * ids_dev / scores_dev: shard g's lists start at + g * shard_stride elements; n_shards * k <= 8192.
 * row_bases: host array.  Synchronises `stream`. */
QAMD_API qamd_status qamd_topk_merge(const uint32_t *ids_dev, const float *scores_dev,
                                     uint64_t shard_stride, const uint64_t *row_bases,
                                     uint32_t n_shards, uint32_t n_queries, uint32_t k, int largest,
                                     uint32_t *out_ids, float *out_scores, qamd_mem out_mem,
                                     void *stream);

/* ===================================================================================
 * Measurement helper (bench.py's roofline arithmetic).
 * =================================================================================== */
/* Per-row store traffic of the u8 scan kernel: bytes read per scored row (codes + offset). */
QAMD_API uint64_t qamd_u8_scan_bytes_per_row(const qamd_u8 *h);

#ifdef __cplusplus
}
#endif
#endif /* QUANTIZATION_AMD_H */
