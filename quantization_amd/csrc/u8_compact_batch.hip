// Batches of a COMPACT 4-bit scalar-u8 store (QAMD_COMPACT) on the int8 matrix cores of gfx950, straight from
// the store's blocked nibble image.
//
// Row codes and query codes of a 4-bit store are 0..15: valid signed bytes as they are, so v_mfma_i32_16x16x64_i8 sums
// the pair products exactly with no bias and no ones column, and a tile holds 16 real queries.  A row's sum is at most
// 2048 * 225 < 2^19; converted once it goes through the f32 epilogue of the image scan (full_epilogue of u8_full_batch.hip,
// epilogue() of u8.hip): the same bits.
//
// Design (u8_compact_batch_kernel<QT, EPI, FILTER, LOW>).  The kernel streams rows and holds queries:
//   * Rows.  A wave's 64 rows are one image block; a K step is four image chunks (128 codes).  Chunk j of a block's 64 rows
//     is one aligned KiB, 16 bytes per row, so lane (i, g) of row tile t loads the 16 bytes at nibble_at(row0 + 16 t + i,
//     4 s + g, P) with one global_load_dwordx4: already a B fragment but for the nibbles.  lo = w & 0x0F.. and hi =
//     (w >> 4) & 0x0F.. are two B fragments (three vector ops per dword): lo of lane (i, g) is code chunk 2 (4 s + g) of
//     its row, hi is code chunk 2 (4 s + g) + 1.  Any pairing of K positions gives the same sum if the query fragment
//     pairs the same way, and it does (below).  The four loads of the next step - the first step of the wave's next block
//     after the last - are in flight while the current step is multiplied.  Chunks at or past P in the last step: the
//     address is clamped and the fragment zeroed.  Blocks are whole and padding rows are zero, so no load tests a row.
//   * Queries.  u8_compact_query_image_kernel writes every pass's queries once per call in A-fragment order, [step][lo /
//     hi][tile][lane] 16 bytes, with zeros for a code chunk the rows do not have (an odd row_chunks; the last step) and for
//     the columns past the batch.  A pass serves QT tiles of 16 queries (QT = 1, 2, 4).  A workgroup of four waves copies
//     its pass's image into LDS once (QT x 16 x actual_dim bytes rounded up to whole steps: 48 KiB at dim 768 and QT 4,
//     128 KiB at the longest row) and takes one barrier; no barrier after that.  Every fragment read is a lane-linear
//     ds_read_b128.  A workgroup walks `blocks_per_wg` consecutive blocks, its waves interleaved, so that the copy stays a
//     small share of the row bytes it reads (launch_pass).
//   * Inner step: the four row tiles are expanded once (8 fragments); then, per query tile, two LDS reads and eight MFMAs.
//     Accumulators: QT x 4 v4i.  Lane (i, g) of accumulator (qt, t) holds queries 16 qt + 4 g + e, e < 4, against row
//     16 t + i: the 16 lanes of a query store 64 contiguous bytes.
//   * The FILTER form (1 largest-first, 2 smallest-first) is u8_full_batch_kernel's: d = (s - B_q) - B_row with the integer
//     bounds of batch_common.hpp, one wave-wide vote per block, the exact f32 epilogue alone decides, and the passing
//     (query, row) pairs are appended to the query's list with one atomic on its counter (BatchTopkPass with n_lists = 0).
//     The helpers assume 0 <= s < 2^29; the sums here stay below 2^19.
//
// Compiled with -packed-fp32-ops off like u8_full_batch.hip (Makefile).
#include <algorithm>

#include "batch_common.hpp"
#include "common.hpp"
#include "u8_internal.hpp"

#pragma clang fp contract(off)

using namespace qamd;

namespace {

constexpr int kCompactBlock = 256;       // four waves
constexpr uint32_t kStepChunks = 4;      // image chunks of one K step: one per lane group g
constexpr uint32_t kMaxSteps = 16;       // actual_dim <= 2048: 64 image chunks
constexpr uint32_t kBlocksPerWg = 32;    // blocks a workgroup walks in a large store (launch_pass)

// The images of all passes of a batch: workgroup p writes pass p.  Pass p holds queries [p * 16 qt_full, ...), in `qt`
// tiles (qt_full, the last pass qt_last).  image: [pass] pass_stride uint4, of which [step][2][qt][64] are written;
// offs: [pass][64] f32, 0 for the columns past the batch.  No code chunk at or past row_chunks is read from qcodes.
__global__ __launch_bounds__(kCompactBlock) void u8_compact_query_image_kernel(const uint8_t *__restrict__ qcodes, uint64_t q_pitch,
                                                                               const float *__restrict__ q_offs, uint32_t nq,
                                                                               uint32_t row_chunks, uint32_t nsteps, uint32_t qt_full,
                                                                               uint32_t qt_last, uint64_t pass_stride,
                                                                               uint4 *__restrict__ image, float *__restrict__ offs) {
    const uint32_t pass = blockIdx.x, q0 = pass * 16 * qt_full, qt = pass + 1 == gridDim.x ? qt_last : qt_full;
    uint4 *img = image + (uint64_t)pass * pass_stride;
    for (uint32_t s = threadIdx.x; s < nsteps * 2 * qt * 64; s += kCompactBlock) {
        const uint32_t l = s % 64, tile = (s / 64) % qt, half = (s / (64 * qt)) % 2, step = s / (128 * qt);
        const uint32_t q = q0 + 16 * tile + l % 16, cc = 2 * (kStepChunks * step + l / 16) + half;
        uint4 w = make_uint4(0, 0, 0, 0);
        if (q < nq && cc < row_chunks) w = *reinterpret_cast<const uint4 *>(qcodes + (uint64_t)q * q_pitch + 16 * cc);
        img[s] = w;
    }
    if (threadIdx.x < 64) offs[pass * 64 + threadIdx.x] = threadIdx.x < 16 * qt && q0 + threadIdx.x < nq ? q_offs[q0 + threadIdx.x] : 0.0f;
}

// The pivot sample of a compact store: sample row j < n is store row hash(j) (gather_rows_kernel's hash), copied 16 bytes
// at a time into a blocked nibble image of `n_padded` rows (whole blocks; the tail is zero), and its offset.
__global__ __launch_bounds__(256) void u8_nibble_gather_kernel(const uint4 *__restrict__ image, const float *__restrict__ offsets,
                                                              uint32_t pchunks, uint64_t n_rows, uint32_t n, uint32_t n_padded,
                                                              uint4 *__restrict__ out_image, float *__restrict__ out_offsets) {
    const uint64_t total = (uint64_t)n_padded * pchunks;
    for (uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (uint64_t)gridDim.x * 256) {
        const uint32_t c = (uint32_t)((o / kPackBlockRows) % pchunks);
        const uint32_t j = (uint32_t)(o / ((uint64_t)kPackBlockRows * pchunks) * kPackBlockRows + o % kPackBlockRows);
        if (j >= n) {
            out_image[o] = make_uint4(0, 0, 0, 0);
            if (c == 0) out_offsets[j] = 0.0f;
            continue;
        }
        const unsigned long long hsh = (unsigned long long)j * 0x9E3779B97F4A7C15ull;
        const uint64_t src = ((hsh >> 32) * n_rows) >> 32;
        out_image[o] = image[nibble_at(src, c, pchunks)];
        if (c == 0) out_offsets[j] = offsets[src];
    }
}

__device__ __forceinline__ v4i as_v4i(const uint4 &w) { return v4i{(int)w.x, (int)w.y, (int)w.z, (int)w.w}; }

// u8.hip epilogue() on the exact integer pair sum, converted once.
__device__ __forceinline__ float compact_epilogue(float multiplier, int s, float q_off, float v_off, float diff, int mode) {
    const float ms = multiplier * (float)s;
    if (mode == 0) return (ms + q_off) + v_off;
    return ms + ((q_off + v_off) - diff);
}

// One pass: out[q * out_pitch + row] for the pass's nq (<= 16 QT) queries and rows [0, n_rows) of the blocked nibble image
// `rows` (pchunks chunks per row, whole blocks) with the offsets v_offsets.  EPI: 0 an encoded query, 1 score_internal's
// epilogue with `diff`.  qimage / q_offs: the pass's own.  Dynamic LDS: nsteps * 2 * QT KiB + 64 QT bytes.
// FILTER != 0 (EPI 0 only): nothing goes to `out`; filt.pivot_scores is the pass's own ([q], q < nq), filt.query_base the
// batch index of its query 0, which filt.counters and filt.candidates are indexed by.  LOW: the pre-filter's direction.
template <int QT, int EPI, int FILTER, bool LOW>
__global__ __launch_bounds__(kCompactBlock) __attribute__((amdgpu_waves_per_eu(QT == 4 ? 2 : QT == 2 ? 3 : 4))) void u8_compact_batch_kernel(const uint4 *__restrict__ rows, const float *__restrict__ v_offsets,
                                                                         const uint4 *__restrict__ qimage, const float *__restrict__ q_offs,
                                                                         uint32_t nq, float multiplier, float diff, uint32_t n_rows,
                                                                         uint32_t pchunks, uint32_t nsteps, uint32_t blocks_per_wg,
                                                                         float *__restrict__ out, uint64_t out_pitch, BatchFilter filt) {
    extern __shared__ uint4 q_lds[];  // [step][lo / hi][QT][64], then the filter form's integer query bounds [16 QT]
    const uint32_t n_frag = nsteps * 2 * QT * 64;
    for (uint32_t s = threadIdx.x; s < n_frag; s += kCompactBlock) q_lds[s] = qimage[s];
    int *bq_lds = reinterpret_cast<int *>(q_lds + n_frag);
    if constexpr (FILTER != 0) {
        if (threadIdx.x < 16 * QT)
            bq_lds[threadIdx.x] = pp_query_bound<LOW>(threadIdx.x < nq ? filt.pivot_scores[threadIdx.x] : 0.0f, q_offs[threadIdx.x],
                                                      multiplier, threadIdx.x < nq);
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63, i16 = lane & 15, g4 = lane >> 4;
    const uint32_t n_blocks = (n_rows + kPackBlockRows - 1) / kPackBlockRows;
    const uint32_t blk0 = blockIdx.x * blocks_per_wg + (threadIdx.x >> 6), blk_end = min(blockIdx.x * blocks_per_wg + blocks_per_wg, n_blocks);
    if (blk0 >= blk_end) return;

    // lane (i, g)'s 16 bytes of the four row tiles of block `blk` at step s; zero where the row has no chunk
    auto load = [&](uint4 (&b)[4], uint32_t blk, uint32_t s) {
        const uint32_t c = kStepChunks * s + g4;
        const bool in = c < pchunks;
        const uint4 *p = rows + ((uint64_t)blk * pchunks + (in ? c : pchunks - 1)) * kPackBlockRows + i16;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint4 w = p[16 * t];
            b[t] = in ? w : make_uint4(0, 0, 0, 0);
        }
    };

    uint4 cur[4], nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    load(cur, blk0, 0);
    for (uint32_t blk = blk0; blk < blk_end; blk += kCompactBlock / 64) {
        const uint64_t row0 = (uint64_t)blk * kPackBlockRows;
        float v_off[4];
#pragma unroll
        for (int t = 0; t < 4; t++) v_off[t] = v_offsets[row0 + 16 * t + i16];  // (inside the padding: blocks are whole)
        v4i acc[QT][4];
#pragma unroll
        for (int qt = 0; qt < QT; qt++) {
#pragma unroll
            for (int t = 0; t < 4; t++) acc[qt][t] = v4i{0, 0, 0, 0};
        }
        for (uint32_t s = 0; s < nsteps; s++) {
            if (s + 1 < nsteps) load(nxt, blk, s + 1);
            else if (blk + kCompactBlock / 64 < blk_end) load(nxt, blk + kCompactBlock / 64, 0);
            const uint4 *frag = q_lds + (uint64_t)s * 2 * QT * 64 + lane;
            // the low nibbles of the four row tiles against every query tile, then the high ones (the shifted form: w & 0xF0..
            // would be a negative byte): four fragments live at a time, and four independent MFMAs per LDS read
#pragma unroll
            for (int half = 0; half < 2; half++) {
                v4i b[4];
#pragma unroll
                for (int t = 0; t < 4; t++) b[t] = as_v4i(half ? nibbles_hi(cur[t]) : nibbles_lo(cur[t]));
#pragma unroll
                for (int qt = 0; qt < QT; qt++) {
                    const v4i a = as_v4i(frag[(half * QT + qt) * 64]);
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[qt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[t], acc[qt][t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t++) cur[t] = nxt[t];
        }
        // The per-query constants are read here, once per block (one 16-byte read per query tile: the four queries of a
        // lane are adjacent), so that nothing but the accumulators and the row fragments lives across the K loop.
        if constexpr (FILTER != 0) {
            constexpr bool LARGEST = FILTER == 1;
            // ext: the most passing d of the lane's 16 QT, over the rows that exist
            int br[4], ext = LOW ? 0x7FFFFFFF : (int)0x80000000;
#pragma unroll
            for (int t = 0; t < 4; t++) br[t] = pp_row_bound<LOW>(v_off[t], multiplier);
#pragma unroll
            for (int qt = 0; qt < QT; qt++) {
                const int4 bq = *reinterpret_cast<const int4 *>(bq_lds + 16 * qt + 4 * g4);
                const int b4[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const bool row_ok = row0 + 16 * t + i16 < n_rows;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int d = (acc[qt][t][e] - b4[e]) - br[t];  // 0 <= s < 2^19, |B_q| <= 2^29, |B_row| <= 2^30: inside an int
                        if (row_ok) ext = LOW ? min(ext, d) : max(ext, d);
                    }
                }
            }
            if (!__builtin_amdgcn_readfirstlane(__ballot(LOW ? ext < 0 : ext >= 0) != 0)) continue;
#pragma unroll
            for (int qt = 0; qt < QT; qt++) {
                const int4 bq = *reinterpret_cast<const int4 *>(bq_lds + 16 * qt + 4 * g4);
                const int b4[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const uint64_t row = row0 + 16 * t + i16;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const uint32_t q = 16 * qt + 4 * g4 + e;
                        const int d = (acc[qt][t][e] - b4[e]) - br[t];
                        // (by index too: a non-finite row's bound beats the "nothing passes" of a padding column)
                        if ((LOW ? d < 0 : d >= 0) && q < nq && row < n_rows) {
                            const float sc = compact_epilogue(multiplier, acc[qt][t][e], q_offs[q], v_off[t], 0.0f, 0);
                            if (batch_filter_pass<LARGEST>(sc, filt.pivot_scores[q])) {
                                const uint32_t gq = filt.query_base + q;
                                const uint32_t pos = atomicAdd(filt.counters + (uint64_t)gq * kCounterStride, 1u);
                                if (pos < kBatchCap)
                                    filt.candidates[(uint64_t)gq * kBatchCap + pos] =
                                        ((unsigned long long)topk_ordered_bits(sc, LARGEST) << 32) | (uint32_t)row;
                            }
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int qt = 0; qt < QT; qt++) {
                const float4 qo = *reinterpret_cast<const float4 *>(q_offs + 16 * qt + 4 * g4);
                const float q4[4] = {qo.x, qo.y, qo.z, qo.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t q = 16 * qt + 4 * g4 + e;
                    float *o = out + (uint64_t)q * out_pitch + row0 + i16;  // the 16 lanes of a query: 64 contiguous bytes per row tile
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        if (q < nq && row0 + 16 * t + i16 < n_rows)
                            o[16 * t] = compact_epilogue(multiplier, acc[qt][t][e], q4[e], v_off[t], EPI ? diff : 0.0f, EPI);
                    }
                }
            }
        }
    }
}

// QAMD_DEV_U8_COMPACT_QT (developer library): the pass width, 1, 2 or 4 tiles of 16 queries, for the A/B of DESIGN 3.1z.
uint32_t compact_qt_full() {
    static const uint64_t v = dev_env_u64("QAMD_DEV_U8_COMPACT_QT", 4);
    return v == 1 || v == 2 ? (uint32_t)v : 4;
}

// One pass over rows [0, n_rows) of the blocked image (rows, v_offsets): pass p of the images `im`.
struct CompactPass {
    const qamd_u8 *h;
    const U8CompactImages &im;
    uint32_t p;
    const uint4 *rows;
    const float *v_offsets;
    uint64_t n_rows;
    hipStream_t s;
};

template <int QT, int EPI, int FILTER, bool LOW>
qamd_status launch_pass(const CompactPass &c, float diff, float *out, uint64_t out_pitch, const BatchFilter &filt) {
    QAMD_LDS_OPT_IN((&u8_compact_batch_kernel<QT, EPI, FILTER, LOW>), kMaxSteps * 2 * QT * 1024 + 16 * QT * 4);
    // A workgroup's image copy is nsteps * 2 QT KiB, about QT / 2 blocks' worth of rows: over kBlocksPerWg = 32 blocks it
    // is QT / 64 of the row bytes the workgroup reads (1/16 at QT 4).  A small store takes fewer blocks per workgroup,
    // down to one per wave, to fill the device.
    const uint64_t blocks = (c.n_rows + kPackBlockRows - 1) / kPackBlockRows;
    const uint32_t per_wg = (uint32_t)std::min<uint64_t>(kBlocksPerWg, std::max<uint64_t>(kCompactBlock / 64, blocks / (4 * (uint64_t)device_info().cu_count)));
    const unsigned grid = (unsigned)((blocks + per_wg - 1) / per_wg);
    const uint32_t q0 = c.p * 16 * c.im.qt_full, nq = std::min<uint32_t>(16 * QT, c.im.nq - q0);
    hipLaunchKernelGGL((u8_compact_batch_kernel<QT, EPI, FILTER, LOW>), dim3(grid), dim3(kCompactBlock), (size_t)c.im.nsteps * 2 * QT * 1024 + 16 * QT * 4,
                       c.s, c.rows, c.v_offsets, c.im.image + (size_t)c.p * c.im.pass_stride, c.im.offs + c.p * 64, nq,
                       c.h->meta.multiplier, diff, (uint32_t)c.n_rows, c.h->image.chunks, c.im.nsteps, per_wg, out, out_pitch, filt);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// fn(Int<QT>): the instantiation for pass p
template <typename Fn>
qamd_status with_qt(const U8CompactImages &im, uint32_t p, Fn &&fn) {
    const uint32_t qt = p + 1 == im.passes ? im.qt_last : im.qt_full;
    return qt == 1 ? fn(Int<1>{}) : qt == 2 ? fn(Int<2>{}) : fn(Int<4>{});
}

// The passes of nq queries: whole passes of qt_full tiles, then a last pass of the smallest QT that holds the rest.
void compact_plan(const qamd_u8 *h, uint32_t nq, U8CompactImages *im) {
    im->nq = nq;
    im->nsteps = (h->image.chunks + kStepChunks - 1) / kStepChunks;
    im->qt_full = compact_qt_full();
    im->passes = (nq + 16 * im->qt_full - 1) / (16 * im->qt_full);
    const uint32_t rest = nq - (im->passes - 1) * 16 * im->qt_full;
    im->qt_last = rest <= 16 ? 1 : rest <= 32 ? 2 : 4;
    im->pass_stride = (size_t)im->nsteps * 2 * im->qt_full * 64;
}

}  // namespace

namespace qamd {

size_t u8_compact_images_bytes(const qamd_u8 *h, uint32_t nq) {
    U8CompactImages im;
    compact_plan(h, nq, &im);
    return im.passes * (im.pass_stride * sizeof(uint4) + 64 * 4);
}

qamd_status u8_compact_images_build(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                    void *scratch, hipStream_t stream, U8CompactImages *out) {
    if (!h->compact || h->image.kind != U8_IMAGE_NIBBLE || h->image.chunks > kMaxSteps * kStepChunks)
        return fail(QAMD_ERR_ARGUMENTS, "u8_compact_batch_kernel serves compact stores of up to 2048 codes per row");
    compact_plan(h, nq, out);
    uint4 *image = static_cast<uint4 *>(scratch);
    float *offs = reinterpret_cast<float *>(image + (size_t)out->passes * out->pass_stride);
    hipLaunchKernelGGL(u8_compact_query_image_kernel, dim3(out->passes), dim3(kCompactBlock), 0, stream, qcodes, q_pitch, q_offs, nq,
                       h->row_chunks, out->nsteps, out->qt_full, out->qt_last, (uint64_t)out->pass_stride, image, offs);
    QAMD_HIP(hipGetLastError());
    out->image = image, out->offs = offs;
    return QAMD_OK;
}

qamd_status u8_compact_batch_scores_of(const qamd_u8 *h, const U8CompactImages &im, const void *rows, const float *v_offsets,
                                       uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream) {
    for (uint32_t p = 0; p < im.passes; p++) {
        const CompactPass c{h, im, p, static_cast<const uint4 *>(rows), v_offsets, n_rows, stream};
        float *o = out + (uint64_t)p * 16 * im.qt_full * out_pitch;
        QAMD_TRY(with_qt(im, p, [&](auto qt) {
            constexpr int QT = decltype(qt)::value;
            return mode == 0 ? launch_pass<QT, 0, 0, false>(c, diff, o, out_pitch, BatchFilter{})
                             : launch_pass<QT, 1, 0, false>(c, diff, o, out_pitch, BatchFilter{});
        }));
    }
    return QAMD_OK;
}

qamd_status u8_compact_batch_scores(const qamd_u8 *h, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, uint32_t nq,
                                    uint64_t n_rows, float *out, uint64_t out_pitch, int mode, float diff, hipStream_t stream) {
    if (nq == 0 || n_rows == 0) return QAMD_OK;
    if (n_rows > h->count) return fail(QAMD_ERR_ARGUMENTS, "%llu rows of a store of %llu", (unsigned long long)n_rows,
                                       (unsigned long long)h->count);
    StreamBuf buf;  // freed in stream order, behind the passes that read it
    QAMD_TRY(buf.alloc(u8_compact_images_bytes(h, nq), stream));
    U8CompactImages im;
    QAMD_TRY(u8_compact_images_build(h, qcodes, q_pitch, q_offs, nq, buf.as<uint8_t>(), stream, &im));
    QAMD_TRY(u8_compact_batch_scores_of(h, im, h->packed.ptr, h->offsets.as<float>(), n_rows, out, out_pitch, mode, diff, stream));
    h->last_compact_batch.store((int)nq, std::memory_order_relaxed);
    return QAMD_OK;
}

qamd_status u8_compact_batch_filter(const qamd_u8 *h, const U8CompactImages &im, const float *pivot_scores, uint32_t *counters,
                                    unsigned long long *candidates, int largest, hipStream_t stream) {
    for (uint32_t p = 0; p < im.passes; p++) {
        const CompactPass c{h, im, p, h->packed.as<uint4>(), h->offsets.as<float>(), h->count, stream};
        BatchFilter f{};
        f.pivot_scores = pivot_scores + p * 16 * im.qt_full;
        f.counters = counters;
        f.candidates = candidates;
        f.largest = largest;
        f.query_base = p * 16 * im.qt_full;
        f.n_queries = im.nq;
        QAMD_TRY(with_qt(im, p, [&](auto qt) {
            constexpr int QT = decltype(qt)::value;
            if (largest)
                return with_low<1>(h->meta.multiplier, [&](auto low) { return launch_pass<QT, 0, 1, decltype(low)::value>(c, 0.0f, nullptr, 0, f); });
            return with_low<2>(h->meta.multiplier, [&](auto low) { return launch_pass<QT, 0, 2, decltype(low)::value>(c, 0.0f, nullptr, 0, f); });
        }));
    }
    return QAMD_OK;
}

size_t u8_compact_sample_bytes(const qamd_u8 *h, uint32_t rows) {
    return (size_t)round_up((uint64_t)rows, kPackBlockRows) * h->image.chunks * sizeof(uint4);
}

qamd_status u8_compact_sample_gather(const qamd_u8 *h, uint32_t rows, void *image, float *offsets, hipStream_t stream) {
    hipLaunchKernelGGL(u8_nibble_gather_kernel, dim3(device_info().cu_count * 8), dim3(256), 0, stream, h->packed.as<uint4>(),
                       h->offsets.as<float>(), h->image.chunks, h->count, rows, (uint32_t)round_up((uint64_t)rows, kPackBlockRows),
                       static_cast<uint4 *>(image), offsets);
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

qamd_status u8_compact_sample_store(const qamd_u8 *h, uint32_t rows_all, hipStream_t s, const void **image, const float **offs) {
    std::lock_guard<std::mutex> lk(h->sample_mu);
    if (h->sample_rows < rows_all) {
        qamd::DevBuf c, o;
        QAMD_TRY(c.alloc(u8_compact_sample_bytes(h, rows_all)));
        QAMD_TRY(o.alloc(round_up((uint64_t)rows_all, kPackBlockRows) * 4));
        QAMD_TRY(u8_compact_sample_gather(h, rows_all, c.ptr, o.as<float>(), s));
        QAMD_HIP(hipStreamSynchronize(s));  // once per handle: every later call, on any stream, just reads it
        h->sample_codes = std::move(c);
        h->sample_offsets = std::move(o);
        h->sample_rows = rows_all;
    }
    *image = h->sample_codes.ptr;
    *offs = h->sample_offsets.as<float>();
    return QAMD_OK;
}

}  // namespace qamd
