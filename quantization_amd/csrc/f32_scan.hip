// Exact scores of EVERY row of the originals (rows 0 .. n_rows - 1) against 1, 2, 4 or 8 queries in one pass: the
// null-id-list form of qamd_f32_score_ids / qamd_f32_rerank / qamd_f32_rerank_batch (f32.hip).
//
// A score is the sequential f32 sum of f32.hip's header comment, so a lane owns a row and adds its terms in the row's
// order, as in f32_pairs_kernel.  What the whole-store form changes:
//  * Rows.  A wave takes 64 CONSECUTIVE rows: no id array, and no row test per load - a row index is clamped to
//    n_rows - 1 (a partial last wave loads its last row again and does not store), so no load leaves the rows
//    [0, n_rows): a borrowed buffer ends at the last byte of row n_rows - 1.
//  * Loads.  VEC (the base is 16-byte aligned and a row is a multiple of 16 bytes: dim % 4 == 0 for f32, dim % 8 == 0
//    for f16 / bf16): a 128-byte segment of a row is 8 pieces of 16 bytes; lane j loads piece j & 7 of the rows
//    8i + (j >> 3), i = 0..7 - 8 loads of 16 bytes per lane cover the wave's 64 rows, where the dword form needs 32.
//    Any other dim, and a borrowed base that is only element-aligned: the dword loads of the pairs kernels (lane j loads
//    dword j & 31 of the rows 2i + (j >> 5), i = 0..31; for an f16 / bf16 row at a 2-byte aligned address, only pairs
//    that lie inside the row, the last value of an odd dim once by the lane that owns the row).
//  * LDS, VEC: the tile keeps a row stride of 36 dwords (144 bytes: rows stay 16-byte aligned).
//    ds_write_b128 is serviced 8 contiguous lanes at a time, bank = dword address mod 32: the lanes 8g .. 8g + 7 hold
//    the 8 pieces of ONE row, dwords row * 36 + 0 .. 31: 32 consecutive dwords, 32 banks, for every stride.
//    ds_read_b128 is serviced in four 16-lane groups, bank = dword address mod 64: lane r reads row r's piece c, dwords
//    r * 36 + 4c .. + 3, the 16-byte slot (r * 9 + c) mod 16 of the 256-byte bank row.  9 is odd, so r -> r * 9 mod 16
//    is a bijection on r mod 16, and each of the groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47,
//    52-59}, {36-43, 48-51, 60-63} holds every residue mod 16 once: 16 distinct slots, conflict-free.  (Stride 32
//    would put all 16 lanes on one slot; 33 is not 16-byte aligned.)
//    Dword form: stride 33 with ds_write_b32 / ds_read_b32, the arithmetic of f32.hip's header.
//    f16 / bf16 tiles hold the PACKED dwords (a segment is 64 values) and are widened after the read.
//  * Queries.  NQ queries share the pass: each lane keeps NQ running sums, each the sequential chain of its own query,
//    so the rows leave HBM once per NQ queries.  A query value is wave-uniform: scalar loads, issued piece by piece
//    (8 queries x 32 values do not fit the SGPR file at once).
//  * The loads of the next segment are issued before the adds of the current one.
// out[q * pitch + row], negated once for `invert`.
#include "rescore.hpp"

#include "f32_terms.hpp"

namespace qamd {
namespace {

constexpr int kBlock = 256;  // 4 waves, each with its own tile of 64 rows
constexpr int kSegDwords = 32;  // dwords of a row per pass: 32 f32 values, 64 f16 / bf16 values

template <int METRIC, int DTYPE, int NQ, bool VEC>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(VEC ? 4 : 3, 4))) void f32_scan_kernel(
    const void *__restrict__ data, uint32_t dim, uint32_t n_rows, const float *__restrict__ queries, int invert,
    float *__restrict__ out, uint64_t pitch) {
    constexpr bool HALF = DTYPE != QAMD_DTYPE_F32;
    constexpr int EPD = HALF ? 2 : 1;       // values per dword
    constexpr int STRIDE = VEC ? 36 : 33;   // dwords between two rows of a tile
    constexpr int kSegVals = kSegDwords * EPD;
    __shared__ __attribute__((aligned(16))) uint32_t tiles[kBlock / 64][64 * STRIDE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *tile = tiles[wave];
    // the wave's rows: first + 0 .. 63, clamped to the last row (a wave past the end scores the last row and stores nothing)
    const uint64_t first64 = (uint64_t)blockIdx.x * kBlock + (uint64_t)wave * 64u;
    const uint32_t last_row = n_rows - 1;
    const uint32_t first = (uint32_t)min(first64, (uint64_t)last_row), room = last_row - first;
    auto row_of = [&](uint32_t x) { return first + min(x, room); };
    const size_t row_bytes = (size_t)dim * (HALF ? 2 : 4);
    const char *bytes = static_cast<const char *>(data);
    const uint16_t *data16 = static_cast<const uint16_t *>(data);  // (a 4-byte copy from it is one dword load, 2-byte aligned)

    uint4 next4[VEC ? 8 : 1];
    uint32_t next[VEC ? 1 : kSegDwords];
    const int piece = lane & 7, sub = lane >> 3;    // VEC: piece `piece` of the rows 8i + sub
    const int col = lane & 31, half = lane >> 5;    // dword form: dword `col` of the rows 2i + half
    auto load_segment = [&](uint32_t d0) {  // d0: the segment's first value
        if constexpr (VEC) {
            const uint32_t d = d0 + (uint32_t)(piece * 4 * EPD);  // whole pieces: dim is a multiple of 4 * EPD
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint4 w = make_uint4(0, 0, 0, 0);
                if (d < dim)
                    w = *reinterpret_cast<const uint4 *>(bytes + (size_t)row_of(8 * i + sub) * row_bytes + (size_t)d * (HALF ? 2 : 4));
                next4[i] = w;
            }
        } else if constexpr (!HALF) {
            const uint32_t d = d0 + (uint32_t)col;
#pragma unroll
            for (int i = 0; i < kSegDwords; i++) {
                uint32_t w = 0;
                if (d < dim) w = *reinterpret_cast<const uint32_t *>(bytes + (size_t)row_of(2 * i + half) * row_bytes + (size_t)d * 4);
                next[i] = w;
            }
        } else {
            const uint32_t d = d0 + 2u * (uint32_t)col;
#pragma unroll
            for (int i = 0; i < kSegDwords; i++) {
                uint32_t w = 0;
                if (d + 1 < dim)  // a pair inside the row, one dword load at a 2-byte aligned address
                    __builtin_memcpy(&w, data16 + (size_t)row_of(2 * i + half) * dim + d, 4);
                next[i] = w;
            }
        }
    };
    // odd dim of a 16-bit row (dword form only): the row's last value has no partner; its lane loads it once
    float last = 0.0f;
    if constexpr (HALF && !VEC)
        if (dim & 1u)
            last = widen_lo<DTYPE>(data16[(size_t)row_of(lane) * dim + (dim - 1)]);

    float sum[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) sum[q] = 0.0f;
    // one dword of the row at value d: its 1 or 2 terms, in the row's order, into every query's chain
    auto add_dword = [&](uint32_t d, uint32_t w) {
        if constexpr (!HALF) {
#pragma unroll
            for (int q = 0; q < NQ; q++) sum[q] += term<METRIC>(queries[(size_t)q * dim + d], __uint_as_float(w));
        } else {
            const float lo = widen_lo<DTYPE>(w), hi = widen_hi<DTYPE>(w);
#pragma unroll
            for (int q = 0; q < NQ; q++) sum[q] += term<METRIC>(queries[(size_t)q * dim + d], lo);
#pragma unroll
            for (int q = 0; q < NQ; q++) sum[q] += term<METRIC>(queries[(size_t)q * dim + d + 1], hi);
        }
    };
    auto add_piece = [&](uint32_t d, const uint4 &w) {
        add_dword(d, w.x);
        add_dword(d + EPD, w.y);
        if constexpr (HALF && NQ == 8) __builtin_amdgcn_sched_barrier(0);
        add_dword(d + 2 * EPD, w.z);
        add_dword(d + 3 * EPD, w.w);
        // the scheduler may not gather the scalar query loads of the whole segment in front of it: NQ x 32 values would
        // spill the SGPR file; a piece's NQ x 4 (x 8 for 16-bit rows, halved again at NQ = 8) fit
        __builtin_amdgcn_sched_barrier(0);
    };

    load_segment(0);
    for (uint32_t d0 = 0; d0 < dim; d0 += kSegVals) {
        if constexpr (VEC) {
#pragma unroll
            for (int i = 0; i < 8; i++) *reinterpret_cast<uint4 *>(tile + (8 * i + sub) * STRIDE + 4 * piece) = next4[i];
        } else {
#pragma unroll
            for (int i = 0; i < kSegDwords; i++) tile[(2 * i + half) * STRIDE + col] = next[i];
        }
        __syncthreads();
        if (d0 + kSegVals < dim) load_segment(d0 + kSegVals);
        const uint32_t *mine = tile + lane * STRIDE;
        const uint32_t n = min((uint32_t)kSegVals, dim - d0);  // values of this segment
        if constexpr (VEC) {
            const uint4 *mine4 = reinterpret_cast<const uint4 *>(mine);
            if (n == kSegVals) {
#pragma unroll
                for (int c = 0; c < 8; c++) add_piece(d0 + c * 4 * EPD, mine4[c]);
            } else {
                for (uint32_t c = 0; c * 4 * EPD < n; c++) add_piece(d0 + c * 4 * EPD, mine4[c]);
            }
        } else {
            if (n == kSegVals) {
#pragma unroll
                for (int c = 0; c < kSegDwords; c++) {
                    add_dword(d0 + c * EPD, mine[c]);
                    if (c % (HALF && NQ == 8 ? 2 : 4) == 1) __builtin_amdgcn_sched_barrier(0);  // as in add_piece
                }
            } else {
                const uint32_t whole = n / EPD;
                for (uint32_t c = 0; c < whole; c++) add_dword(d0 + c * EPD, mine[c]);
                if constexpr (HALF)
                    if (n & 1u) {  // only at the end of a row of odd dim
#pragma unroll
                        for (int q = 0; q < NQ; q++) sum[q] += term<METRIC>(queries[(size_t)q * dim + (dim - 1)], last);
                    }
            }
        }
        __syncthreads();
    }
    const uint64_t row = first64 + (uint64_t)lane;
    if (row < n_rows) {
#pragma unroll
        for (int q = 0; q < NQ; q++) out[(size_t)q * pitch + row] = invert ? -sum[q] : sum[q];
    }
}

struct ScanArgs {
    const void *data;
    uint32_t dim, n_rows;
    const float *queries;
    int invert;
    float *out;
    uint64_t pitch;
    unsigned grid;
    hipStream_t s;
};

template <int METRIC, int DTYPE, int NQ> void scan_go_vec(const ScanArgs &a, bool vec) {
    if (vec)
        hipLaunchKernelGGL((f32_scan_kernel<METRIC, DTYPE, NQ, true>), dim3(a.grid), dim3(kBlock), 0, a.s, a.data, a.dim, a.n_rows,
                           a.queries, a.invert, a.out, a.pitch);
    else
        hipLaunchKernelGGL((f32_scan_kernel<METRIC, DTYPE, NQ, false>), dim3(a.grid), dim3(kBlock), 0, a.s, a.data, a.dim, a.n_rows,
                           a.queries, a.invert, a.out, a.pitch);
}
template <int METRIC, int DTYPE> void scan_go_nq(const ScanArgs &a, bool vec, uint32_t nq) {
    if (nq == 8) scan_go_vec<METRIC, DTYPE, 8>(a, vec);
    else if (nq == 4) scan_go_vec<METRIC, DTYPE, 4>(a, vec);
    else if (nq == 2) scan_go_vec<METRIC, DTYPE, 2>(a, vec);
    else scan_go_vec<METRIC, DTYPE, 1>(a, vec);
}
template <int METRIC> void scan_go_dtype(const ScanArgs &a, bool vec, uint32_t nq, qamd_dtype t) {
    if (t == QAMD_DTYPE_F32) scan_go_nq<METRIC, QAMD_DTYPE_F32>(a, vec, nq);
    else if (t == QAMD_DTYPE_F16) scan_go_nq<METRIC, QAMD_DTYPE_F16>(a, vec, nq);
    else scan_go_nq<METRIC, QAMD_DTYPE_BF16>(a, vec, nq);
}

}  // namespace

qamd_status f32_scan_launch(const qamd_f32 *h, const float *queries_dev, uint32_t n_queries, uint64_t n_rows, float *out_dev,
                            uint64_t pitch, hipStream_t s) {
    if (n_rows == 0 || n_queries == 0) return QAMD_OK;
    const size_t row_bytes = (size_t)h->vp.dim * (h->dtype == QAMD_DTYPE_F32 ? 4 : 2);
    const bool vec = reinterpret_cast<uintptr_t>(h->data) % 16 == 0 && row_bytes % 16 == 0;
    ScanArgs a{h->data, (uint32_t)h->vp.dim, (uint32_t)n_rows, queries_dev, (int)(h->vp.invert != 0), out_dev, pitch,
               (unsigned)((n_rows + kBlock - 1) / kBlock), s};
    for (uint32_t q = 0; q < n_queries;) {  // 8 queries per pass, the remainder in the forms 4, 2, 1
        const uint32_t left = n_queries - q, nq = left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
        a.queries = queries_dev + (size_t)q * h->vp.dim;
        a.out = out_dev + (size_t)q * pitch;
        if (h->vp.distance_type == QAMD_DOT) scan_go_dtype<QAMD_DOT>(a, vec, nq, h->dtype);
        else if (h->vp.distance_type == QAMD_L1) scan_go_dtype<QAMD_L1>(a, vec, nq, h->dtype);
        else scan_go_dtype<QAMD_L2>(a, vec, nq, h->dtype);
        q += nq;
    }
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

}  // namespace qamd
