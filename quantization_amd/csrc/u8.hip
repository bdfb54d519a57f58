// Scalar u8 quantizer on MI355X (gfx950), the READ side: query encode, the query-vs-store scans, top-k, pair scoring and
// rescoring of a built store.  What WRITES a store (the encoders, the scan image, save / load, upsert) is u8_store.hip;
// the two share the handles, the code formats and a few launchers through u8_internal.hpp.
//
// Host class mirrors EncodedVectorsU8 (quantization/src/encoded_vectors_u8.rs); the kernels
// replace the per-pair SIMD FFI (quantization/cpp/avx2.c:25-122) by whole-store launches.
//
// HBM layout (library-owned copy).  The reference row is AoS [vector_offset f32][codes]
// with stride actual_dim+4 (772 B at dim 768: only 4-byte aligned).  On device it is split
// into  codes[count_padded][actual_dim]  (rows 16-byte aligned, contiguous) and
// offsets[count] f32.  Same 772 algorithmic bytes per scored row; every code load is an
// aligned 16-byte `global_load_dwordx4`.  Dot / L2 stores also keep a packed scan image of the
// codes at 7 bits each, in blocks of 64 rows (u8_internal.hpp; u8_store.hip build_packed), which their
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
#include "u8_internal.hpp"

#pragma clang fp contract(off)

using namespace qamd;

namespace {

enum Epilogue : int { EPI_POINT = 0, EPI_INTERNAL = 1 };

// ------------------------------------------------------------------------------ device helpers
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Streamed-once 16-byte loads: `global_load_dwordx4 ... nt`.
__device__ __forceinline__ uint4 ld_nt(const uint4 *p) {
    u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ uint32_t sad16(const uint4 &a, const uint4 &b, uint32_t acc) {
    acc = __builtin_amdgcn_sad_u8(a.x, b.x, acc);
    acc = __builtin_amdgcn_sad_u8(a.y, b.y, acc);
    acc = __builtin_amdgcn_sad_u8(a.z, b.z, acc);
    acc = __builtin_amdgcn_sad_u8(a.w, b.w, acc);
    return acc;
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
// A format (Image7, Image4: u8_internal.hpp, beside what the pack kernel of u8_store.hip needs of it) carries what differs.

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

// NQ (2, 4, 8) queries per pass over the nibble image: the batch route of a compact 4-bit store, which has
// no byte codes for u8_scan_multi_kernel or the matrix cores to read.  The frame is u8_scan_image_kernel<Image4>'s, line
// for line: `split` waves per block of 64 rows, lane l owns row 64 b + l, every wave-load is one aligned kilobyte, one
// ring of R = 8 chunks in flight and refilled behind its last use, then the rest group.  What changes is the inner step:
// a loaded chunk is masked ONCE into its low and its (unshifted) high nibbles, and each of the NQ queries then adds
//   lo[j] += dot(w & 0x0F.., q_j[2c]),  hi[j] += dot(w & 0xF0.., q_j[2c + 1])
// with q_j = qcodes + j * q_pitch read at wave-uniform addresses: scalar loads through the constant cache, no vector
// register per query.  Per 16-byte chunk a lane issues 8 `and` and 8 NQ v_dot4 instead of NQ * (8 + 8): the scan's idle
// vector ALU pays for the extra queries while the image is read from HBM once.  Row sum j = lo[j] + (hi[j] >> 4), the
// single kernel's exact integer (same bounds), and the same f32 epilogue, so the same score bits.  32 ring registers,
// 2 NQ accumulators, 8 for the two masked copies.
// An unused slot (3 queries in a 4-wide pass) re-reads the last valid query and writes nothing.  For an odd row_chunks the
// second query chunk of the last image chunk is not read for any j: the last query of a batch ends there.
// split > 1: the NQ partial sums of a lane meet in LDS (NQ * kScanBlock words) behind one barrier.
// FILTER: no score is written; the lane offers its row to query j's candidate lists (slices).  EPI_INTERNAL: the queries
// are stored rows unpacked into a [NQ][q_pitch] block with their stored offsets (u8_nibble_unpack_kernel).
template <int NQ, bool FILTER, int EPI = EPI_POINT>
__global__ __launch_bounds__(kScanBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void u8_scan_image_multi_kernel(
    const uint4 *__restrict__ image, const float *__restrict__ offsets, const uint8_t *__restrict__ qcodes, uint32_t q_pitch,
    const float *__restrict__ q_offs, uint32_t nq_valid /* 2 .. NQ: queries really there */, float multiplier,
    uint32_t n_rows, uint32_t pchunks, uint32_t row_chunks, uint32_t split, float *__restrict__ out /* [NQ][out_pitch] */,
    uint64_t out_pitch, TopkFilterSlices slices, float diff) {
    constexpr int R = Image4::R;
    __shared__ uint32_t partial[NQ][kScanBlock];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t part = wave & (split - 1);
    const uint64_t block = (uint64_t)blockIdx.x * ((kScanBlock / 64) / split) + wave / split;
    const uint64_t row = block * kPackBlockRows + lane;
    const bool live = block * kPackBlockRows < n_rows;  // wave-uniform; offsets[] and the image are padded past every block
    // the groups of a row, as in u8_scan_image_kernel: n_ring whole groups of R full chunks, then one of the n_rest left
    const uint32_t n_full = row_chunks / 2, n_ring = n_full / R, n_rest = pchunks - R * n_ring;
    const uint32_t n_groups = n_ring + (n_rest ? 1 : 0);
    const uint32_t g_begin = live ? n_groups * part / split : 0, g_end = live ? n_groups * (part + 1) / split : 0;
    const uint4 *blk = image + block * pchunks * kPackBlockChunk;
    const uint32_t lane16 = lane * 16;
    auto chunk_ptr = [&](uint32_t c) {
        return reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(blk + (uint64_t)c * kPackBlockChunk) + lane16);
    };
    const uint32_t gf_end = g_end < n_ring ? g_end : n_ring;
    const bool has_rest = g_end > n_ring;

    const uint4 *q[NQ];  // wave-uniform
#pragma unroll
    for (int j = 0; j < NQ; j++)
        q[j] = reinterpret_cast<const uint4 *>(qcodes + (size_t)((uint32_t)j < nq_valid ? (uint32_t)j : nq_valid - 1) * q_pitch);
    uint32_t lo[NQ], hi[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) lo[j] = hi[j] = 0;
    // image chunk c against query chunks 2c and, when the row has it, 2c + 1
    auto add = [&](const uint4 &w, uint32_t c, bool second) {
        const uint4 l = and16(w, 0x0F0F0F0Fu), u = and16(w, 0xF0F0F0F0u);
        uint32_t at = 32 * c;  // bytes into a query
        // NQ = 8: the 32 query bytes of one image chunk are 64 SGPRs.  Left alone, the compiler fuses the scalar loads of two
        // neighbouring chunks into 64-byte ones, needs 128, and spills them lane by lane into vector registers (and those to
        // scratch).  An offset it cannot see through keeps the loads of a chunk apart from the next chunk's.
        if constexpr (NQ == 8) asm volatile("" : "+s"(at));
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const uint4 *qc = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(q[j]) + at);
            lo[j] = dot16(l, qc[0], lo[j]);
            if (second) hi[j] = dot16(u, qc[1], hi[j]);
        }
    };

    uint4 v[R];
    auto eat = [&](uint32_t g, auto refill) {
#pragma unroll
        for (int i = 0; i < R; i++) {
            add(v[i], R * g + i, true);
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
    if (g_begin < gf_end) {
        for (uint32_t g = g_begin; g + 1 < gf_end; g++) eat(g, std::true_type{});
        eat(gf_end - 1, std::false_type{});
    }
    if (has_rest) {
        const uint32_t c0 = R * n_ring;
#pragma unroll
        for (int i = 0; i < R; i++)
            if ((uint32_t)i < n_rest) v[i] = ld_nt(chunk_ptr(c0 + i));
#pragma unroll
        for (int i = 0; i < R; i++)
            if ((uint32_t)i < n_rest) add(v[i], c0 + i, c0 + i < n_full);
    }
    uint32_t acc[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) acc[j] = lo[j] + (hi[j] >> 4);
    if (split > 1) {
#pragma unroll
        for (int j = 0; j < NQ; j++) partial[j][threadIdx.x] = acc[j];
        __syncthreads();
        if (part == 0)
            for (uint32_t p = 1; p < split; p++) {
#pragma unroll
                for (int j = 0; j < NQ; j++) acc[j] += partial[j][threadIdx.x + 64 * p];
            }
    }
    if (part == 0 && row < n_rows) {
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            if ((uint32_t)j >= nq_valid) break;
            const float score = epilogue(multiplier, acc[j], q_offs[j], v_off, EPI == EPI_POINT ? 0.0f : diff, EPI);
            if (FILTER) {
                const TopkFilter f = topk_filter_of(slices, (uint32_t)j);
                topk_offer(f, *f.pivot_key, score, (uint32_t)row);
            } else {
                __builtin_nontemporal_store(score, out + (uint64_t)j * out_pitch + row);
            }
        }
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

// ------------------------------------------------------------------------------ query encode kernels
// encode_query on device (encoded_vectors_u8.rs:290-329): one wave.
// qbuf: [0] offset f32, [16..] codes.
__global__ __launch_bounds__(64) void encode_query_kernel(const float *__restrict__ query,
                                                         uint32_t qdim, uint32_t actual_dim,
                                                         float alpha, float offset, int distance,
                                                         int invert, uint8_t *__restrict__ qbuf, int levels) {
    const int lane = threadIdx.x;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, levels);
    uint8_t *codes = qbuf + 16;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t j = lane; j < actual_dim; j += 64) {
        uint32_t c = j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code;
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
                    s += (float)(j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code);
            }
            off = s * alpha * offset;
        } else if (distance == QAMD_L1) {
            off = 0.0f;
        } else {
            float s = (float)s2;
            if (s2 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    float c = (float)(j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code);
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
                                                           uint32_t code_pitch, float *__restrict__ offsets_out, int levels) {
    const int lane = threadIdx.x;
    const float *query = queries + (size_t)blockIdx.x * qdim;
    uint8_t *codes = codes_out + (size_t)blockIdx.x * code_pitch;
    const float placeholder = (distance == QAMD_DOT) ? 0.0f : offset;
    const uint32_t pad_code = f32_to_code(placeholder, alpha, offset, levels);
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t j = lane; j < actual_dim; j += 64) {
        uint32_t c = j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code;
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
                    s += (float)(j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code);
            }
            off = s * alpha * offset;
        } else if (distance == QAMD_L1) {
            off = 0.0f;
        } else {
            float s = (float)s2;
            if (s2 >= (1u << 24)) {
                s = 0.0f;
                for (uint32_t j = 0; j < actual_dim; j++) {
                    float c = (float)(j < qdim ? f32_to_code(query[j], alpha, offset, levels) : pad_code);
                    s += c * c;
                }
            }
            off = s * alpha * alpha;
        }
        offsets_out[blockIdx.x] = invert ? -off : off;
    }
}

// ---- compact 4-bit stores: pair scoring out of the nibble image ----
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

// ------------------------------------------------------------------------------ launchers
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
    return u8_unpack_rows(h, nullptr, i, 1, tmp.as<uint8_t>(), h->meta.actual_dim, nullptr, s);
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

// The row-length ladder of the byte-code kernels, in one place: row_chunks as a compile-time shape.  f gets a
// RowShape{}: G = min(16, pow2(rc)) lanes per row, ITERS = ceil(rc / G) 16-byte pieces per lane and UNROLL, the rows in
// flight per row slot of u8_scan_kernel (the other kernels have an unroll of their own and take G and ITERS only).
// false, and f not called: rows of more than 128 chunks, which have no templated shape.
template <int G_, int ITERS_, int UNROLL_> struct RowShape {
    static constexpr int G = G_, ITERS = ITERS_, UNROLL = UNROLL_;
};
template <class F> bool with_row_shape(uint32_t rc, F &&f) {
    if (rc == 1) return f(RowShape<1, 1, 4>{}), true;
    if (rc == 2) return f(RowShape<2, 1, 4>{}), true;
    if (rc <= 4) return f(RowShape<4, 1, 8>{}), true;
    if (rc <= 8) return f(RowShape<8, 1, 8>{}), true;
    switch ((rc + 15) / 16) {
        case 1: return f(RowShape<16, 1, 8>{}), true;
        case 2: return f(RowShape<16, 2, 4>{}), true;
        case 3: return f(RowShape<16, 3, 4>{}), true;
        case 4: return f(RowShape<16, 4, 2>{}), true;
        case 5: return f(RowShape<16, 5, 2>{}), true;
        case 6: return f(RowShape<16, 6, 2>{}), true;
        case 7: return f(RowShape<16, 7, 2>{}), true;
        case 8: return f(RowShape<16, 8, 2>{}), true;
        default: return false;
    }
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
    h->last_scan_queries.store(1, std::memory_order_relaxed);
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

// ---- several queries per pass over the nibble image (u8_scan_image_multi_kernel) ----------------
// Widest pass for this store: 8 queries for a compact store (the only one whose batches have no byte codes to read),
// 0 = none.  DESIGN 3.1z has the measurements the width rests on.  QAMD_DEV_U8_IMAGE_MULTI (developer library) caps it
// at 2 or 4, or turns the route off (1), for the A/B of tools/time_u8_compact_batch.py.
uint32_t image_multi_width(const qamd_u8 *h) {
    static const uint32_t cap = (uint32_t)dev_env_u64("QAMD_DEV_U8_IMAGE_MULTI", 8);
    if (h->image.kind != U8_IMAGE_NIBBLE || !h->compact) return 0;
    return cap >= 8 ? 8 : cap >= 4 ? 4 : cap >= 2 ? 2 : 0;
}

// One pass for `nq_valid` (2 .. image_multi_width) queries ([q][q_pitch] codes, [q] offsets) over the rows the epilogue
// covers, in the smallest NQ that holds them; out is [nq_valid][scan_rows].  false = not served (the caller scans singly).
bool launch_image_multi(const qamd_u8 *h, uint32_t nq_valid, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs,
                        float *out, const TopkFilterSlices *slices, hipStream_t s, const ScanEpi &e = ScanEpi{}) {
    if (nq_valid < 2 || nq_valid > image_multi_width(h) || (slices && e.mode != EPI_POINT)) return false;
    const uint64_t n_rows = scan_rows(h, e);  // also the pitch of `out`
    const uint32_t split = blocked_split(n_rows), blocks_per_wg = (kScanBlock / 64) / split;
    const uint64_t blocks = (n_rows + kPackBlockRows - 1) / kPackBlockRows;
    const unsigned grid = (unsigned)((blocks + blocks_per_wg - 1) / blocks_per_wg);
    h->last_scan_packed.store(h->image.kind, std::memory_order_relaxed);
    h->last_scan_split.store((int)split, std::memory_order_relaxed);
    h->last_scan_queries.store((int)nq_valid, std::memory_order_relaxed);
    h->last_compact_batch.store(0, std::memory_order_relaxed);
    auto go = [&](auto nq) {
        with_bool(slices != nullptr, [&](auto fi) {
            with_epi(e.mode, [&](auto epi) {
                if constexpr (!(fi && epi == EPI_INTERNAL))  // (no filtering form of score_internal is instantiated)
                    hipLaunchKernelGGL((u8_scan_image_multi_kernel<nq, fi, epi>), dim3(grid), dim3(kScanBlock), 0, s,
                                       h->packed.as<uint4>(), h->offsets.as<float>(), qcodes, (uint32_t)q_pitch, q_offs, nq_valid,
                                       h->meta.multiplier, (uint32_t)n_rows, h->image.chunks, h->image.aux, split, out, n_rows,
                                       slices ? *slices : TopkFilterSlices{}, e.diff);
            });
        });
    };
    if (nq_valid <= 2) go(std::integral_constant<int, 2>{});
    else if (nq_valid <= 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 8>{});
    return true;
}

// Returns false when the store's row size has no templated kernel (caller uses the generic one).
// The Dot / L2 scans read the scan image when the store has one (its rows are 7/8 or half as long; an L1 store has none).
template <bool IS_L1>
bool launch_scan(const qamd_u8 *h, const uint4 *qc, const float *qo, float *out, const TopkFilter *filt,
                 hipStream_t s, const ScanEpi &e) {
    using L = ScanLaunch<IS_L1>;
    h->last_scan_packed.store(h->image.kind, std::memory_order_relaxed);
    if (h->image.kind) return launch_scan_image(h, qc, qo, out, filt, s, e), true;
    return with_row_shape(h->row_chunks, [&](auto sh) {
        using S = decltype(sh);
        L::template go<S::G, S::ITERS, S::UNROLL>(h, qc, qo, out, filt, s, e);
    });
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
                                   h->codes_7bit<uint4>() /* its prologue quantises with f32_to_u8 */, h->offsets.as<float>(), qv, fq->qdim, (uint32_t)h->meta.actual_dim,
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
    qamd_status st = QAMD_OK;
    const bool shaped = with_row_shape(rc, [&](auto sh) {  // (G and ITERS only: the kernel's unroll is its own)
        st = L::template go<decltype(sh)::G, decltype(sh)::ITERS>(h, qc, qo, fq, pl, p, s, e);
    });
    return shaped ? st : fail(QAMD_ERR_ARGUMENTS, "no small top-k kernel for %u chunks", rc);
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
    h->last_full_batch.store(0, std::memory_order_relaxed);
    h->last_full_filter.store(0, std::memory_order_relaxed);
    h->last_full_redone.store(0, std::memory_order_relaxed);
    h->last_scan_queries.store((int)nq_valid, std::memory_order_relaxed);
    with_bool(exact, [&](auto ex) {
        with_bool(slices != nullptr && e.mode == EPI_POINT, [&](auto fi) {  // score_internal of gathered rows: scores only
            with_epi(e.mode, [&](auto epi) {
                if constexpr (!(fi && epi == EPI_INTERNAL))  // (no filtering form of score_internal is instantiated)
                    hipLaunchKernelGGL((u8_scan_multi_kernel<G, ITERS, UNROLL, NQ, IS_L1, ex, fi, epi>), dim3(grid),
                                       dim3(kScanBlock), 0, s, h->byte_codes<uint4>(), h->offsets.as<float>(), qcodes,
                                       (uint32_t)q_pitch, q_offs, nq_valid, h->meta.multiplier, (uint32_t)n_rows, h->row_chunks,
                                       out, n_rows, slices ? *slices : TopkFilterSlices{}, e.diff);
            });
        });
    });
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
    if (nq_valid < 2 || nq_valid > multi_width(h) || (slices && e.mode != EPI_POINT)) return false;
    bool launched = false;  // only the 16-lane shapes have a multi-query form: narrower rows launch nothing and say so
    with_row_shape(h->row_chunks, [&](auto sh) {
        if constexpr (decltype(sh)::G == 16) {
            constexpr int IT = decltype(sh)::ITERS;
            constexpr int UN = IT == 1 ? 4 : IT <= 4 ? 2 : 1;  // this kernel's unroll: it holds NQ queries beside the rows
            auto go = [&](auto nq) {
                launch_multi_shape<IS_L1, 16, IT, UN, decltype(nq)::value>(h, qcodes, q_pitch, q_offs, nq_valid, out, slices, s, e);
                launched = true;
            };
            if constexpr (IS_L1 && IT <= 3) {  // the 8-wide pass: L1 rows of up to 768 bytes only
                if (nq_valid > 4) return go(Int<8>{});
            }
            if (nq_valid > 2) go(Int<(IT <= 6 ? 4 : 2)>{});
            else go(Int<2>{});
        }
    });
    return launched;
}

// What the batch callers below walk their queries with: the widest pass of the store - over the nibble image for a
// compact store, over the byte codes otherwise - and one such pass for 2 .. pass_width queries (false = unsupported).
uint32_t pass_width(const qamd_u8 *h) {
    const uint32_t image_width = image_multi_width(h);
    return image_width ? image_width : multi_width(h);
}
bool launch_pass(const qamd_u8 *h, uint32_t nq_valid, const uint8_t *qcodes, uint64_t q_pitch, const float *q_offs, float *out,
                 const TopkFilterSlices *slices, hipStream_t s, const ScanEpi &e = ScanEpi{}) {
    if (image_multi_width(h)) return launch_image_multi(h, nq_valid, qcodes, q_pitch, q_offs, out, slices, s, e);
    return h->meta.vector_parameters.distance_type == QAMD_L1 ? launch_multi<true>(h, nq_valid, qcodes, q_pitch, q_offs, out, slices, s, e)
                                                              : launch_multi<false>(h, nq_valid, qcodes, q_pitch, q_offs, out, slices, s, e);
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
            hipLaunchKernelGGL((u8_scan_avx2_lanes_kernel<true, epi>), dim3(grid), dim3(kBlock), 0, s, h->codes_7bit<uint4>(),
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
    auto go = [&](auto it) {
        hipLaunchKernelGGL((u8_score_pairs_kernel<IS_L1, decltype(it)::value>), dim3(grid), dim3(kBlock), 0, s,
                           h->byte_codes<uint4>(), h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists,
                           list_rows, h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks,
                           (uint32_t)ppb, out_dev);
    };
    if (!IS_L1 && lane_order(h)) {
        hipLaunchKernelGGL((u8_score_pairs_kernel<false, 0, true>), dim3(grid), dim3(kBlock), 0, s, h->codes_7bit<uint4>(),
                           h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists, list_rows,
                           h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks, (uint32_t)ppb,
                           out_dev);
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
    // ITERS = ceil(row_chunks / 16) of the shape (a row group of fewer than 16 lanes has 1); longer rows, and rows of
    // no chunk at all (a dim-0 store: the ITERS forms load a row's last chunk unasked): the any-length loop
    if (h->row_chunks == 0 || !with_row_shape(h->row_chunks, [&](auto sh) { go(Int<decltype(sh)::ITERS>{}); })) go(Int<0>{});
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
        auto go = [&](auto it) {
            hipLaunchKernelGGL((u8_nibble_pairs_kernel<decltype(it)::value>), dim3(grid), dim3(kBlock), 0, s,
                               h->packed.as<uint4>(), h->offsets.as<float>(), qc, qo, q_batch, q_pitch, q_offs, lists, n_lists,
                               list_rows, h->meta.multiplier, diff, mode, ids_dev, n_ids, (uint32_t)h->count, h->row_chunks,
                               h->image.chunks, (uint32_t)ppb, out_dev);
        };
        switch ((h->image.chunks + 15) / 16) {  // IMAGE chunks, at most 64 (u8_image_of): a ladder of its own
            case 1: go(Int<1>{}); break;
            case 2: go(Int<2>{}); break;
            case 3: go(Int<3>{}); break;
            default: go(Int<4>{}); break;
        }
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
// then passes of pass_width(h) rows (u8_scan_multi_kernel or, for a compact store, u8_scan_image_multi_kernel, with
// score_internal's epilogue: the integer sum and the f32 epilogue of the single-row scan, so the same bits), a remainder
// of one row and every row size without a multi form (fewer than 9 or more than 128 pieces, lane order) through the
// single-row scan.  Enqueues only.
qamd_status score_internal_rows_dev(const qamd_u8 *h, const uint32_t *rows_dev, uint32_t n, uint64_t n_ids, float *out_dev,
                                    hipStream_t s) {
    const uint64_t pitch = h->meta.actual_dim;  // 16 * row_chunks
    const size_t code_bytes = (size_t)n * pitch;
    StreamBuf stage;
    QAMD_TRY(stage.alloc(code_bytes + (size_t)n * 4, s));
    uint8_t *qcodes = stage.as<uint8_t>();
    float *q_offs = reinterpret_cast<float *>(qcodes + code_bytes);
    if (h->compact) {  // the rows come out of the image, and then take the image scan up to 8 at a time
        QAMD_TRY(u8_unpack_rows(h, rows_dev, 0, n, qcodes, pitch, q_offs, s));
    } else {
        hipLaunchKernelGGL(u8_gather_rows_kernel, dim3(n), dim3(64), 0, s, h->byte_codes<uint4>(), h->offsets.as<float>(),
                           rows_dev, (uint32_t)h->count, h->row_chunks, reinterpret_cast<uint4 *>(qcodes), q_offs);
        QAMD_HIP(hipGetLastError());
    }
    const ScanEpi e{internal_diff(h), EPI_INTERNAL, n_ids};
    // A full-range store: more rows than the multi-query scan takes go to the matrix cores, 15 per pass
    if (h->full_range && h->meta.vector_parameters.distance_type != QAMD_L1 && n >= u8_full_batch_min(h))
        return u8_full_batch_scores(h, qcodes, pitch, q_offs, n, n_ids, out_dev, n_ids, EPI_INTERNAL, e.diff, s);
    // A compact store: from its gate on, the unpacked rows are the queries of u8_compact_batch_kernel
    if (const uint32_t cmin = u8_compact_batch_min(h); cmin && n >= cmin)
        return u8_compact_batch_scores(h, qcodes, pitch, q_offs, n, n_ids, out_dev, n_ids, EPI_INTERNAL, e.diff, s);
    const uint32_t width = pass_width(h);
    for (uint32_t l = 0; l < n;) {
        const uint32_t nq = std::min(width, n - l);
        const uint8_t *qc = qcodes + (uint64_t)l * pitch;
        float *o = out_dev + (uint64_t)l * n_ids;
        const bool ok = nq >= 2 && launch_pass(h, nq, qc, pitch, q_offs + l, o, nullptr, s, e);
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

// ------------------------------------------------------------------------------ query encode
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
    if (q->fmt.rotated) {  // the rotated values go behind the staging area, and the encoder reads those
        float *rot = reinterpret_cast<float *>(q->buf.as<uint8_t>() + 16 + round_up(ad, 16) + ad * 4);
        QAMD_TRY(u8_rot_values(q_dev, 1, qdim, rot, s));
        q_dev = rot;
    }
    hipLaunchKernelGGL(encode_query_kernel, dim3(1), dim3(64), 0, s, q_dev, (uint32_t)qdim, (uint32_t)ad, q->alpha,
                       q->offset, q->distance, q->invert, q->buf.as<uint8_t>(), q->fmt.levels());
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
    q->fmt = h->format();
    q->alpha = h->meta.alpha;
    q->offset = h->meta.offset;
    q->distance = h->meta.vector_parameters.distance_type;
    q->invert = h->meta.vector_parameters.invert;
    // (the fused top-k neither rotates nor makes 4-bit or full-range codes)
    if (query_mem == QAMD_MEM_HOST && u8_host_encode_is_lazy(qdim) && !h->rotated && !h->four_bit && !h->full_range) {
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
        QAMD_TRY(u8_rot_values(queries_dev, n_queries, qdim, rot.as<float>(), stream));
        queries_dev = rot.as<float>();
    }
    hipLaunchKernelGGL(encode_queries_kernel, dim3((unsigned)n_queries), dim3(64), 0, stream, queries_dev,
                       (uint32_t)qdim, (uint32_t)actual_dim_of(qdim), h->meta.alpha, h->meta.offset,
                       vp.distance_type, vp.invert, codes_dev, (uint32_t)code_pitch, offsets_dev, h->levels());
    QAMD_HIP(hipGetLastError());
    return QAMD_OK;
}

// ------------------------------------------------------------------------------ top-k and batch routes
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
    const uint32_t width = pass_width(h);
    if (width)  // one filtering pass over the rows for up to `width` queries
        scan.scan_filter_multi = [&, width](uint32_t q, uint32_t left, const TopkFilterSlices &sl, hipStream_t st,
                                            qamd_status &status) -> uint32_t {
            const uint32_t nq = std::min(left, width);
            if (nq < 2) return 0;
            const uint8_t *qcodes = codes_dev + (uint64_t)q * pitch;
            const bool ok = launch_pass(h, nq, qcodes, pitch, offsets_dev + q, nullptr, &sl, st);
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
// a compact store: the matrix-core kernels and u8_scan_multi_kernel read byte codes, which it has not; its
// batches share passes over the nibble image instead (u8_scan_image_multi_kernel, pass_width).
bool u8_batch_by_scans(const qamd_u8 *h) { return lane_order(h) || h->compact; }

// The one gate of u8_compact_batch_kernel: a compact Dot / L2 store whose multiplier the integer pre-filter
// can divide by sends batches of kCompactBatchMin queries and more to the matrix cores; smaller ones keep the image passes
// (the measured crossover is in DESIGN 3.1z).  QAMD_DEV_U8_COMPACT_MIN (developer library) overrides the constant; 0
// switches the route off.
constexpr uint32_t kCompactBatchMin = 18;
uint32_t u8_compact_batch_min(const qamd_u8 *h) {
    static const uint32_t gate = [] {
        const char *e = dev_env("QAMD_DEV_U8_COMPACT_MIN");
        return e && *e ? (uint32_t)strtoul(e, nullptr, 10) : kCompactBatchMin;
    }();
    const float m = h->meta.multiplier;
    if (!h->compact || h->image.kind != U8_IMAGE_NIBBLE || h->meta.vector_parameters.distance_type == QAMD_L1) return 0;
    if (!(fabsf(m) < __builtin_huge_valf()) || m == 0.0f) return 0;
    return gate;
}

// out[j * count + row] for queries [0, n_queries) of a batch through the multi-query scan (groups of
// `width`, then smaller groups, then single scans).
qamd_status u8_score_batch_scans(const qamd_u8 *h, const uint8_t *codes_dev, uint64_t pitch, const float *offsets_dev,
                                 uint32_t n_queries, float *out_dev, hipStream_t stream) {
    const uint32_t width = pass_width(h);
    uint32_t q = 0;
    while (q < n_queries) {
        const uint32_t nq = std::min(width, n_queries - q);
        const uint8_t *qcodes = codes_dev + (uint64_t)q * pitch;
        float *o = out_dev + (uint64_t)q * h->count;
        const bool ok = nq >= 2 && launch_pass(h, nq, qcodes, pitch, offsets_dev + q, o, nullptr, stream);
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

// ================================================================================== C ABI: scoring and top-k
extern "C" {

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

uint64_t qamd_u8_scan_bytes_per_row(const qamd_u8 *h) {
    if (h && h->image.kind == U8_IMAGE_NIBBLE) return 16ull * h->image.chunks + 4;  // the nibble image
    return h ? h->meta.actual_dim + 4 : 0;
}

// Selects how sums above 2^24 are rounded (0: once, 1: avx2.c lane order).  Not part of the
// reference surface; see the header of this file.
qamd_status qamd_u8_set_lane_mode(qamd_u8 *h, int mode) {
    if (!h || mode < 0 || mode > 1) return fail(QAMD_ERR_ARGUMENTS, "bad lane mode");
    if (mode == 1 && h->full_range)  // the lane order restates an AVX2 kernel that cannot run codes above 127
        return fail(QAMD_ERR_ARGUMENTS, "lane mode 1 restates the AVX2 kernel, which a full-range store's codes saturate");
    h->lane_mode = mode;
    return QAMD_OK;
}

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
// Developer-only reports of the read side: libquantization_amd_dev.so only.
extern "C" __attribute__((visibility("default"))) const void *qamd_dev_u8_query_ptr(const qamd_u8_query *q) {
    return q->buf.ptr;
}
// Which image the store's last scan launch read (U8Image::kind), and how many waves per block its last blocked scan took
// and how many queries it served (1: u8_scan_image_kernel; 2 .. 8: one pass of u8_scan_image_multi_kernel).
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_scan_split(const qamd_u8 *h) {
    return h->last_scan_split.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_scan_queries(const qamd_u8 *h) {
    return h->last_scan_queries.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_full_batch(const qamd_u8 *h) {
    return h->last_full_batch.load(std::memory_order_relaxed);
}
// Queries of the store's last topk_batch call that went through the filter form of u8_full_batch_kernel (0: the scans
// served it), and how many of those were then redone exactly.
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_full_filter(const qamd_u8 *h) {
    return h->last_full_filter.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_full_redone(const qamd_u8 *h) {
    return h->last_full_redone.load(std::memory_order_relaxed);
}
// Queries u8_compact_batch_kernel served in the store's last batch call (0: the image passes served it), the queries of its
// last topk_batch that went through the kernel's filter form, and how many of those were then redone exactly.
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_compact_batch(const qamd_u8 *h) {
    return h->last_compact_batch.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_compact_filter(const qamd_u8 *h) {
    return h->last_compact_filter.load(std::memory_order_relaxed);
}
extern "C" __attribute__((visibility("default"))) int qamd_dev_u8_last_compact_redone(const qamd_u8 *h) {
    return h->last_compact_redone.load(std::memory_order_relaxed);
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
