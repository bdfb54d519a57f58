// OriginalVectors.topk_batch for f16 / bf16 Dot stores and 16 or more queries: a matrix-core filter pass over the rows,
// then the exact score of the survivors decides.  Reached through qamd_f32_rerank_batch with a null id list
// (f32.hip, rerank_scan); ids and score bits are those of the groups-of-8 scan route.
//
//   1. f32_mfma_query_kernel: the f32 queries rounded to the store's element type (nearest even) into an image
//      [queries padded to 128][dim], with ||q||_1 and the flag "cannot be bounded" per query.
//   2. amax = max |x| over the store, kept in the handle (f32_mfma_amax_kernel at first use; upsert folds new rows in).
//   3. tau_q = the exact k-th best score of S rows spread evenly over the store (the pair kernels and the radix select).
//   4. f32_mfma_filter_kernel: a GEMM whose output is never written.  A workgroup of 4 waves owns 128 rows x 128 queries;
//      workgroups that share a row tile are neighbours in the grid (query tile fastest), so a row tile leaves HBM about
//      once and its other readers find it in L2 / Infinity Cache, whichever XCD they run on.  The query image (nq * dim * 2
//      bytes, 1.5 MiB for 1024 x 768) is served from L2.
//      K loop: tiles of 64 values, both operands through LDS, two buffers: the 16-byte global loads of tile t + 1 are
//      issued before the MFMAs of tile t and stored after them, one barrier per tile.  dim % 8 == 0, so a 16-byte piece is
//      inside the row or wholly past it: pieces past dim are zero (the K tail).  Row indices are clamped to n_rows - 1, the
//      query image is padded: no load leaves either array.
//      LDS: [2][256 operand rows][72 values]: 144 bytes per operand row (128 + 16), 73 728 bytes, two workgroups per CU.
//      Writes: 8 consecutive lanes store the 8 pieces of one operand row, 128 contiguous bytes.  Reads (ds_read_b128, four
//      16-lane groups, f32_scan.hip's arithmetic): lane r reads operand row r, the 16-byte slot (9 r + c) mod 16; 9 is odd,
//      so 16 rows take 16 slots: conflict-free.
//      MFMA: v_mfma_f32_32x32x16_{f16,bf16}: per LDS byte read it does twice the work of the 16x16x32 form ((32 + 32) x 16
//      values for 16 K MACs against (16 + 16) x 32 for 8 K), and LDS reads are this kernel's second limit.  A wave owns
//      64 rows x 64 queries = 2 x 2 instruction tiles, 64 accumulator registers; rows are the A operand, queries the B
//      operand, so a lane's 16 accumulators of a tile belong to ONE query (column lane % 32) and the rows
//      8 (i / 4) + 4 (lane / 32) + i % 4.
//      Epilogue: a row is appended to its query's list unless its sum is provably worse than tau_q by more than E_q
//      (f32_mfma_bound.hpp): written as the negation, so a NaN sum survives.  The append is a vector atomic on the
//      query's counter; a counter past the capacity marks the query as overflowed (and is then left alone).
//   5. The lists, padded with 0xFFFFFFFF, go through the list-form exact re-rank (rerank_device).
//   6. Queries that were flagged, or whose list overflowed - all of them when amax is not finite - are answered by the scan
//      route and assembled with the others.
#include "rescore.hpp"

#include "f32_mfma_bound.hpp"
#include "f32_terms.hpp"
#include "topk.hpp"

#include <vector>

namespace qamd {
namespace {

constexpr int kBlock = 256;
constexpr int kTileRows = 128, kTileQueries = 128, kTileK = 64;
constexpr int kLdsStride = kTileK + 8;  // values between two operand rows
constexpr size_t kFilterLds = 2ull * (kTileRows + kTileQueries) * kLdsStride * 2;
constexpr uint32_t kListCap = kRerankMaxIds;
constexpr uint32_t kMinQueries = 16, kMinRows = 32768, kMinSample = 8192;
constexpr uint64_t kWsBudget = 384ull << 20;  // with the scan route's scores of a redo, within the 512 MiB rule

__global__ __launch_bounds__(kBlock) void fill_u32_kernel(uint32_t *dst, uint64_t n, uint32_t value) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) dst[i] = value;
}

// ids[q][j] = the j-th of S rows spread evenly over 0 .. n_rows - 1 (S <= n_rows: distinct), for every query.
__global__ __launch_bounds__(kBlock) void sample_ids_kernel(uint32_t *ids, uint32_t n_queries, uint32_t S, uint32_t n_rows) {
    const uint64_t total = (uint64_t)n_queries * S;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock)
        ids[i] = (uint32_t)((i % S) * n_rows / S);
}

__global__ __launch_bounds__(kBlock) void gather_tau_kernel(const float *scores, uint32_t n_queries, uint32_t k, float *tau) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q < n_queries) tau[q] = scores[(size_t)q * k + (k - 1)];
}

// Workgroup b: query b of the image.  b >= n_queries: a padding row of zeros.
template <int DTYPE>
__global__ __launch_bounds__(kBlock) void f32_mfma_query_kernel(const float *__restrict__ queries, uint32_t n_queries, uint32_t dim,
                                                               uint16_t *__restrict__ image, float *__restrict__ l1,
                                                               uint32_t *__restrict__ flag) {
    __shared__ float part[kBlock / 64];
    __shared__ uint32_t bad_any;
    const uint32_t q = blockIdx.x;
    uint16_t *dst = image + (size_t)q * dim;
    if (q >= n_queries) {
        for (uint32_t d = threadIdx.x; d < dim; d += kBlock) dst[d] = 0;
        return;
    }
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    float sum = 0.0f;
    bool bad = false;
    for (uint32_t d = threadIdx.x; d < dim; d += kBlock) {
        const float v = queries[(size_t)q * dim + d];
        const uint32_t h = narrow<DTYPE>(v);
        dst[d] = (uint16_t)h;
        sum += __builtin_fabsf(v);
        bad |= !(__builtin_fabsf(v) < __builtin_huge_valf()) || (h & 0x7FFFu) >= (DTYPE == QAMD_DTYPE_F16 ? 0x7C00u : 0x7F80u);
    }
    for (int m = 32; m; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    if (bad) atomicOr(&bad_any, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        l1[q] = (part[0] + part[1]) + (part[2] + part[3]);
        flag[q] = bad_any;
    }
}

// *out (zero before the launch) = max over data[0 .. n) of the 16-bit pattern without its sign: for f16 and bf16 alike the
// order of those patterns is the order of |x|, and every NaN lies above infinity.
__global__ __launch_bounds__(kBlock) void f32_mfma_amax_kernel(const uint16_t *__restrict__ data, uint64_t n, uint32_t *out) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t head = std::min<uint64_t>(n, ((16 - (reinterpret_cast<uintptr_t>(data) & 15)) & 15) / 2);  // values before a 16-byte line
    const uint64_t n8 = (n - head) / 8;
    uint32_t m = 0;
    const uint4 *data4 = reinterpret_cast<const uint4 *>(data + head);
    for (uint64_t i = t; i < n8; i += stride) {
        const uint4 w = data4[i];
        const uint32_t a = max(w.x & 0x7FFF7FFFu, w.y & 0x7FFF7FFFu), b = max(w.z & 0x7FFF7FFFu, w.w & 0x7FFF7FFFu);
        // the high halves compare first; the low halves are folded in on their own
        m = max(m, max(max(a >> 16, b >> 16), max(max(w.x & 0x7FFFu, w.y & 0x7FFFu), max(w.z & 0x7FFFu, w.w & 0x7FFFu))));
    }
    for (uint64_t i = t; i < head; i += stride) m = max(m, data[i] & 0x7FFFu);
    for (uint64_t i = head + n8 * 8 + t; i < n; i += stride) m = max(m, data[i] & 0x7FFFu);
    for (int s = 32; s; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

template <int DTYPE> __device__ __forceinline__ void mfma_step(const uint4 &a, const uint4 &b, float (&c)[16]) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = c[i];
    if constexpr (DTYPE == QAMD_DTYPE_F16) {
        typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
    } else {
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) c[i] = acc[i];
}

// Workgroup b: query tile b % n_qtiles, row tile b / n_qtiles.  image: [n_qtiles * 128][dim]; thr, skip: per query of the
// image.  negate: the score is minus the sum (invert).  below: a score under thr is provably worse (largest), else one over it.
template <int DTYPE>
__global__ __launch_bounds__(kBlock) void f32_mfma_filter_kernel(const uint16_t *__restrict__ rows, uint32_t dim, uint32_t n_rows,
                                                                const uint16_t *__restrict__ image, uint32_t n_queries,
                                                                uint32_t n_qtiles, const float *__restrict__ thr,
                                                                const uint32_t *__restrict__ skip, int negate, int below,
                                                                uint32_t *__restrict__ counts, uint32_t *__restrict__ lists) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    constexpr int kBuf = (kTileRows + kTileQueries) * kLdsStride;  // values of one buffer: the row tile, then the query tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;  // the wave's 64 rows x 64 queries inside the tile
    const uint32_t qt = blockIdx.x % n_qtiles, rt = blockIdx.x / n_qtiles;
    const uint32_t row0 = rt * (uint32_t)kTileRows, q0 = qt * (uint32_t)kTileQueries;

    // thread t loads piece t & 7 (8 values) of the operand rows (t >> 3) + 32 i, i = 0..3, of both operands
    const int piece = threadIdx.x & 7, sub = threadIdx.x >> 3;
    const uint16_t *src_a[4], *src_b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        src_a[i] = rows + (size_t)min(row0 + (uint32_t)(sub + 32 * i), n_rows - 1) * dim + piece * 8;
        src_b[i] = image + (size_t)(q0 + (uint32_t)(sub + 32 * i)) * dim + piece * 8;
    }
    uint4 next_a[4], next_b[4];
    auto load_tile = [&](uint32_t d0) {
        const bool in = d0 + (uint32_t)piece * 8u < dim;  // whole pieces: dim % 8 == 0
#pragma unroll
        for (int i = 0; i < 4; i++) {
            next_a[i] = in ? *reinterpret_cast<const uint4 *>(src_a[i] + d0) : make_uint4(0, 0, 0, 0);
            next_b[i] = in ? *reinterpret_cast<const uint4 *>(src_b[i] + d0) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_tile = [&](int buf) {
        uint16_t *base = lds + buf * kBuf;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<uint4 *>(base + (sub + 32 * i) * kLdsStride + piece * 8) = next_a[i];
            *reinterpret_cast<uint4 *>(base + (kTileRows + sub + 32 * i) * kLdsStride + piece * 8) = next_b[i];
        }
    };

    float acc[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[a][b][i] = 0.0f;

    // lane: operand row lane % 32 of an instruction tile, the 8 values (lane / 32) * 8 .. + 7 of a K step of 16
    const int frag = (lane & 31) * kLdsStride + (lane >> 5) * 8;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t d0 = 0; d0 < dim; d0 += kTileK, buf ^= 1) {
        const bool more = d0 + kTileK < dim;
        if (more) load_tile(d0 + kTileK);
        const uint16_t *a_base = lds + buf * kBuf + (wm * 64) * kLdsStride + frag;
        const uint16_t *b_base = lds + buf * kBuf + (kTileRows + wn * 64) * kLdsStride + frag;
#pragma unroll
        for (int kk = 0; kk < kTileK / 16; kk++) {
            uint4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                fa[t] = *reinterpret_cast<const uint4 *>(a_base + t * 32 * kLdsStride + kk * 16);
                fb[t] = *reinterpret_cast<const uint4 *>(b_base + t * 32 * kLdsStride + kk * 16);
            }
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) mfma_step<DTYPE>(fa[a], fb[b], acc[a][b]);
        }
        if (more) store_tile(buf ^ 1);  // last read before the barrier that ended the previous tile
        __syncthreads();
    }

#pragma unroll
    for (int b = 0; b < 2; b++) {
        const uint32_t q = q0 + (uint32_t)(wn * 64 + b * 32 + (lane & 31));
        if (q >= n_queries || skip[q]) continue;
        const float t = thr[q];
        uint32_t *count = counts + q;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t row = row0 + (uint32_t)(wm * 64 + a * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3));
                const float s = negate ? -acc[a][b][i] : acc[a][b][i];
                const bool worse = below ? s < t : s > t;  // false for a NaN sum or threshold: the row survives
                if (row < n_rows && !worse && __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= kListCap) {
                    const uint32_t pos = atomicAdd(count, 1u);
                    if (pos < kListCap) lists[(size_t)q * kListCap + pos] = row;
                }
            }
    }
}

bool route_on() {
    static const bool on = [] { const char *e = dev_env("QAMD_F32_MFMA"); return !(e && e[0] == '0'); }();  // developer A/B: 0 = off
    return on;
}

float widen_host(qamd_dtype t, uint32_t bits) {
    if (t == QAMD_DTYPE_BF16) {
        const uint32_t w = bits << 16;
        float f;
        memcpy(&f, &w, 4);
        return f;
    }
    const int e = (int)(bits >> 10) & 31, m = (int)bits & 1023;
    return e ? std::ldexp((float)(m + 1024), e - 25) : std::ldexp((float)m, -24);
}

// max |x| over the values [first, first + n) of the store; +inf when one of them is infinite or a NaN.  Synchronises `s`.
qamd_status amax_of(const qamd_f32 *h, uint64_t first, uint64_t n, uint32_t *scratch_dev, hipStream_t s, float *out) {
    *out = 0.0f;
    if (n == 0) return QAMD_OK;
    hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(kBlock), 0, s, scratch_dev, (uint64_t)1, 0u);
    const unsigned grid = (unsigned)std::min<uint64_t>((n + kBlock * 8 - 1) / (kBlock * 8), (uint64_t)device_info().cu_count * 16);
    hipLaunchKernelGGL(f32_mfma_amax_kernel, dim3(grid), dim3(kBlock), 0, s, static_cast<const uint16_t *>(h->data) + first, n, scratch_dev);
    QAMD_HIP(hipGetLastError());
    uint32_t bits = 0;
    QAMD_TRY(copy_out(&bits, QAMD_MEM_HOST, scratch_dev, 4, s));
    *out = bits >= (h->dtype == QAMD_DTYPE_F16 ? 0x7C00u : 0x7F80u) ? HUGE_VALF : widen_host(h->dtype, bits);
    return QAMD_OK;
}

uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// The workspace of a chunk of C queries (Cp = C rounded up to the query tile), S sample rows each.
struct Layout {
    size_t image, samp_ids, samp_scores, lists, rerank, small, total;
    Layout(uint32_t C, uint32_t S, uint32_t dim, uint32_t k) {
        const size_t Cp = round_up(C, kTileQueries);
        size_t at = 0;
        auto take = [&](size_t bytes) { const size_t o = at; at += round_up(bytes, 256); return o; };
        image = take(Cp * dim * 2);
        samp_ids = take((size_t)C * S * 4);
        samp_scores = take((size_t)C * S * 4);
        lists = take((size_t)C * kListCap * 4);
        rerank = take(rerank_ws_bytes(C, kListCap, k, QAMD_MEM_DEVICE));
        small = take(Cp * 4 * 6);  // l1, flag, tau | thr, skip | counts
        total = at;
    }
};

}  // namespace

// THE gate of the matrix-core route (the issue's conditions, in one place), and what it fixes: the sample size S and how
// many queries share one workspace.  S: the filter keeps about k n / S rows per query (the sample's k-th best is the
// threshold), and that is to stay a quarter of a list: S = 4 k n / 8192, at least 8192, a multiple of 256.  Two conditions
// come from cost, not from correctness: the sample is scored pair by pair, so past n / 8 rows (k > 256 on a big store) it
// costs what the scan route costs; and a chunk of at least 16 queries must fit the workspace.
bool f32_mfma_plan(const qamd_f32 *h, uint64_t n_queries, uint32_t n_rows, uint32_t k, uint32_t *sample, uint32_t *chunk) {
    if (!route_on()) return false;
    if (h->dtype != QAMD_DTYPE_F16 && h->dtype != QAMD_DTYPE_BF16) return false;
    if (h->vp.distance_type != QAMD_DOT) return false;
    if (n_queries < kMinQueries || n_rows < kMinRows || k > 1024) return false;
    if (h->vp.dim % 8 || h->vp.dim == 0 || h->vp.dim > kMfmaBoundMaxDim || reinterpret_cast<uintptr_t>(h->data) % 16) return false;
    const uint64_t want = round_up(4ull * k * n_rows / kListCap, 256);
    const uint64_t S = std::max<uint64_t>(want, kMinSample);
    if (S > std::max<uint64_t>(kMinSample, n_rows / 8)) return false;
    const uint64_t C = std::min<uint64_t>(n_queries, 1024);
    uint64_t fit = C;
    while (fit >= kMinQueries && Layout((uint32_t)fit, (uint32_t)S, (uint32_t)h->vp.dim, k).total > kWsBudget) fit /= 2;
    if (fit < kMinQueries) return false;
    *sample = (uint32_t)S;
    *chunk = (uint32_t)fit;
    return true;
}

void f32_mfma_fold_amax(qamd_f32 *h, uint64_t first_row, uint64_t n_rows, hipStream_t s) {
    const uint32_t known = h->amax_bits.load(std::memory_order_relaxed);
    if (known == kAmaxUnknown) return;  // computed over the whole store at first use
    float old, fresh = HUGE_VALF;
    memcpy(&old, &known, 4);
    DevBuf scratch;
    if (scratch.alloc(256) != QAMD_OK || amax_of(h, first_row * h->vp.dim, n_rows * h->vp.dim, scratch.as<uint32_t>(), s, &fresh) != QAMD_OK) {
        h->amax_bits.store(kAmaxUnknown, std::memory_order_relaxed);  // computed again at the next use
        return;
    }
    h->amax_bits.store(bits_of(std::max(old, fresh)), std::memory_order_relaxed);  // never lowered
}

qamd_status f32_mfma_topk_batch(const qamd_f32 *h, const float *q_dev, uint32_t n_queries, uint32_t n_rows, uint32_t k, int largest,
                                uint32_t S, uint32_t chunk, uint32_t *ids_dev, float *sc_dev, hipStream_t s,
                                const std::function<qamd_status(uint32_t q0, uint32_t n)> &scan_route) {
    static const bool debug = dev_env("QAMD_DEBUG_TOPK") != nullptr;
    const uint32_t dim = (uint32_t)h->vp.dim;
    const bool f16 = h->dtype == QAMD_DTYPE_F16, invert = h->vp.invert != 0;
    const char *name = f16 ? "f32_mfma_filter_kernel<f16>" : "f32_mfma_filter_kernel<bf16>";
    if (f16) QAMD_LDS_OPT_IN((&f32_mfma_filter_kernel<QAMD_DTYPE_F16>), kFilterLds);
    else QAMD_LDS_OPT_IN((&f32_mfma_filter_kernel<QAMD_DTYPE_BF16>), kFilterLds);
    const Layout lay(chunk, S, dim, k);
    char *ws = nullptr;
    QAMD_TRY(thread_ws_acquire(WS_RESCORE, lay.total, s, reinterpret_cast<void **>(&ws)));
    void *sel = nullptr;
    qamd_status st = thread_ws_acquire(WS_SELECT, round_up(topk_workspace_bytes(k), 256), s, &sel);
    if (st != QAMD_OK) {
        thread_ws_release(WS_RESCORE, s);
        return st;
    }
    const size_t Cp = round_up(chunk, kTileQueries);
    uint16_t *image = reinterpret_cast<uint16_t *>(ws + lay.image);
    uint32_t *samp_ids = reinterpret_cast<uint32_t *>(ws + lay.samp_ids), *lists = reinterpret_cast<uint32_t *>(ws + lay.lists);
    float *samp_scores = reinterpret_cast<float *>(ws + lay.samp_scores);
    uint32_t *small = reinterpret_cast<uint32_t *>(ws + lay.small);  // 6 arrays of Cp words
    uint32_t *counts = small + 5 * Cp;

    std::vector<uint8_t> redo(n_queries, 0);
    uint32_t n_redo = 0, surv_min = 0xFFFFFFFFu, surv_max = 0;
    uint64_t surv_sum = 0;
    // stage 2: the store's magnitude
    uint32_t amax_bits = h->amax_bits.load(std::memory_order_relaxed);
    float amax = 0.0f;
    if (amax_bits == kAmaxUnknown) {
        st = amax_of(h, 0, h->vp.count * h->vp.dim, counts, s, &amax);
        if (st == QAMD_OK) h->amax_bits.store(bits_of(amax), std::memory_order_relaxed);
    } else {
        memcpy(&amax, &amax_bits, 4);
    }
    const bool usable = st == QAMD_OK && amax < HUGE_VALF;
    if (st == QAMD_OK && !usable) {
        std::fill(redo.begin(), redo.end(), 1);
        n_redo = n_queries;
    }
    if (usable) {
        hipLaunchKernelGGL(sample_ids_kernel, dim3(device_info().cu_count * 8), dim3(kBlock), 0, s, samp_ids, chunk, S, n_rows);
        st = hipGetLastError() == hipSuccess ? QAMD_OK : fail(QAMD_ERR_DEVICE, "f32 topk_batch: launch failed");
    }
    std::vector<uint32_t> host(5 * Cp);
    const MfmaElem elem = f16 ? kMfmaF16 : kMfmaBF16;
    for (uint32_t c0 = 0; usable && c0 < n_queries && st == QAMD_OK; c0 += chunk) {
        const uint32_t C = std::min(chunk, n_queries - c0), n_qtiles = (C + kTileQueries - 1) / kTileQueries;
        const float *q_chunk = q_dev + (size_t)c0 * dim;
        uint32_t *ids_chunk = ids_dev + (size_t)c0 * k;
        float *sc_chunk = sc_dev + (size_t)c0 * k;
        // stage 1: the query image
        if (f16)
            hipLaunchKernelGGL(f32_mfma_query_kernel<QAMD_DTYPE_F16>, dim3(n_qtiles * kTileQueries), dim3(kBlock), 0, s, q_chunk, C, dim,
                               image, reinterpret_cast<float *>(small), small + Cp);
        else
            hipLaunchKernelGGL(f32_mfma_query_kernel<QAMD_DTYPE_BF16>, dim3(n_qtiles * kTileQueries), dim3(kBlock), 0, s, q_chunk, C, dim,
                               image, reinterpret_cast<float *>(small), small + Cp);
        // stage 3: tau = the exact k-th best of the sample (the outputs serve as scratch: the re-rank writes them last)
        st = rescore_pairs_launch(h, q_chunk, C, S, samp_ids, samp_scores, s);
        for (uint32_t q = 0; q < C && st == QAMD_OK; q++)
            st = topk_f32(samp_scores + (size_t)q * S, S, k, largest != 0, ids_chunk + (size_t)q * k, sc_chunk + (size_t)q * k, sel, s);
        if (st != QAMD_OK) break;
        hipLaunchKernelGGL(gather_tau_kernel, dim3((C + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc_chunk, C, k,
                           reinterpret_cast<float *>(small + 2 * Cp));
        if ((st = copy_out(host.data(), QAMD_MEM_HOST, small, 3 * Cp * 4, s)) != QAMD_OK) break;
        // stage 5: thresholds; a score is -sum for invert, and bounds are symmetric
        for (uint32_t q = 0; q < C; q++) {
            float l1, tau;
            memcpy(&l1, &host[q], 4);
            memcpy(&tau, &host[2 * Cp + q], 4);
            const double E = f32_mfma_bound(elem, dim, l1, amax);
            const bool skip = host[Cp + q] != 0 || !(E < HUGE_VAL);
            const float thr = skip ? 0.0f : f32_mfma_threshold(tau, E, largest != 0);
            host[3 * Cp + q] = bits_of(thr);
            host[4 * Cp + q] = skip;
        }
        if ((st = copy_in(small + 3 * Cp, host.data() + 3 * Cp, QAMD_MEM_HOST, 2 * Cp * 4, s)) != QAMD_OK) break;
        // stage 4: the filter pass
        const unsigned fill_grid = device_info().cu_count * 8;
        hipLaunchKernelGGL(fill_u32_kernel, dim3(fill_grid), dim3(kBlock), 0, s, lists, (uint64_t)C * kListCap, kRerankPad);
        hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(kBlock), 0, s, counts, (uint64_t)C, 0u);
        const unsigned grid = n_qtiles * ((n_rows + kTileRows - 1) / kTileRows);
        if (f16) {
            hipLaunchKernelGGL(f32_mfma_filter_kernel<QAMD_DTYPE_F16>, dim3(grid), dim3(kBlock), kFilterLds, s,
                               static_cast<const uint16_t *>(h->data), dim, n_rows, image, C, n_qtiles,
                               reinterpret_cast<const float *>(small + 3 * Cp), small + 4 * Cp, (int)invert, largest != 0, counts, lists);
        } else {
            hipLaunchKernelGGL(f32_mfma_filter_kernel<QAMD_DTYPE_BF16>, dim3(grid), dim3(kBlock), kFilterLds, s,
                               static_cast<const uint16_t *>(h->data), dim, n_rows, image, C, n_qtiles,
                               reinterpret_cast<const float *>(small + 3 * Cp), small + 4 * Cp, (int)invert, largest != 0, counts, lists);
        }
        if (hipGetLastError() != hipSuccess) {
            st = fail(QAMD_ERR_DEVICE, "f32 topk_batch: launch failed");
            break;
        }
        if ((st = copy_out(host.data(), QAMD_MEM_HOST, counts, (size_t)C * 4, s)) != QAMD_OK) break;
        // stage 6: the exact score of the survivors decides
        st = rerank_device(h, q_chunk, C, lists, kListCap, ws + lay.rerank, k, largest, ids_chunk, sc_chunk, QAMD_MEM_DEVICE, s);
        for (uint32_t q = 0; q < C; q++) {
            if (host[4 * Cp + q] || host[q] > kListCap) {
                redo[c0 + q] = 1;
                n_redo++;
            } else {
                surv_min = std::min(surv_min, host[q]), surv_max = std::max(surv_max, host[q]), surv_sum += host[q];
            }
        }
    }
    thread_ws_release(WS_SELECT, s);
    thread_ws_release(WS_RESCORE, s);
    if (debug && st == QAMD_OK) {
        const uint32_t kept = n_queries - n_redo;
        fprintf(stderr, "[qamd f32_topk_batch] filter %s, S = %u, survivors min/mean/max = %u/%llu/%u, %u queries redone\n", name, S,
                kept ? surv_min : 0, (unsigned long long)(kept ? surv_sum / kept : 0), surv_max, n_redo);
    }
    // stage 7: runs of queries that the filter could not serve take the scan route, after the re-rank in stream order
    for (uint32_t q = 0; q < n_queries && st == QAMD_OK;) {
        if (!redo[q]) {
            q++;
            continue;
        }
        uint32_t end = q;
        while (end < n_queries && redo[end]) end++;
        st = scan_route(q, end - q);
        q = end;
    }
    return st;
}

}  // namespace qamd
