// Pieces shared by the many-queries-at-once paths (csrc/u8_batch.hip; the binary matrix-core path): the
// candidate-filter descriptor, the integer pre-filter bound, and the per-query kernels around a filtering
// pass (pivot sample gather, pivot selection, scatter of the wave-private candidate lists, emit), and the host side of
// such a pass: BatchTopkPass (scratch arena, pivots, scatter, emit, status read-back) and BatchTopkOutputs (staging of
// host outputs, exact redo of the queries the pass could not serve).
// Internal linkage: every translation unit that includes this gets its own copies.
#pragma once
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "topk.hpp"
#include "topk_device.hpp"

#pragma clang fp contract(off)

namespace qamd {
namespace {

constexpr uint32_t kBatchCap = kTopkCandCap;  // candidate slots per query
constexpr uint32_t kCounterStride = 16;       // u32: one counter per 64-byte line

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

struct BatchFilter {
    const float *pivot_scores;       // [Qpad] pivot as a score; +-inf for padding queries (nothing passes)
    uint32_t *counters;              // [Qpad * kCounterStride]
    unsigned long long *candidates;  // [Qpad][kBatchCap]
    int largest;
    // ping-pong kernel: candidates are first appended to wave-private lists (no global atomic in
    // the GEMM's epilogue), then distributed to the per-query lists by wave_scatter_kernel
    uint4 *wave_cand;       // [n_waves][wave_cap]  {key, row, query, 0}
    uint32_t *wave_counts;  // [n_waves] entries appended (may exceed wave_cap: overflow)
    uint32_t wave_cap;
    uint32_t wave_base;     // first wave list of this launch
    uint32_t query_base;    // global index of the launch's query 0
    int *query_bounds;      // [Qpad] scratch for the query-streaming kernel's integer bounds
    uint32_t n_queries;     // queries of the whole batch: a padding query (global index >= n_queries) never appends
};

// The exact epilogue's filter: "key <= pivot key" (topk_ordered_bits), decided by ONE float compare wherever the
// compare is ordered - only the rare passing element pays for the key - and by the keys themselves where it is not (a
// NaN score or a NaN pivot).  So a NaN on the winning side of the order passes (+NaN in a `largest` query) and one
// on the losing side does not, and the number of appended candidates stays what the emit kernels take it for: rows
// at least as good as the pivot (batch_emit_kernel's `pushed < k` under-flow test).  The one superset left is -0
// against a +0 pivot.  Compared directly, not through the sign of a difference: inf - inf is NaN, and a row as
// good as an infinite pivot is a tie like any other.  Padding rows and padding queries carry infinite `never` offsets
// and pivots, which tie with an infinite counterpart here: the caller keeps them out by index (row < n_rows,
// query < n_queries).
template <bool LARGEST> __device__ __forceinline__ bool batch_filter_pass(float sc, float pv) {
    if (LARGEST ? sc >= pv : sc <= pv) return true;
    if (sc == sc && pv == pv) return false;
    return topk_ordered_bits(sc, LARGEST) <= topk_ordered_bits(pv, LARGEST);
}


// Integer pre-filter (MODE 1/2).  The filter "score at least as good as the pivot" is, in exact
// arithmetic, s >= P_q + R_row (or <=, template LOW: when multiplier < 0 xor smallest-first) with
// P_q = (pivot_q - q_offset_q) / multiplier and R_row = -v_offset_row / multiplier.  Both are
// rounded to integers on the safe side by more than the f32 epilogue can be off (pp_bound), and
// the accumulators START at -(B_q + B_row): after the K loop "may pass" is a sign test on the
// AND (OR) of four accumulators; only groups that may pass run the exact f32 epilogue, which
// alone decides.  A wrong bound could only cost time, never a result... provided it is on the
// safe side, which is what pp_bound's slack is for:
//   |computed score - real score| <= 2^-21 (|m s| + |q_off| + |v_off|)  (four roundings), and for a
//   candidate the filter rejects, either |m s| <= 2 (|pivot| + |q_off| + |v_off|), which the 2^-19
//   terms cover, or the real score misses the pivot by more than |m s| / 2 >> that error.
constexpr float kPpLim = 536870912.0f;  // 2^29: |B_q| + |B_row| + s < 2^31 for actual_dim <= 32768
template <bool LOW>
__device__ __forceinline__ int pp_bound(float num /* pivot - q_off, or -v_off */, float mag /* |pivot|+|q_off| or |v_off| */,
                                        float m, int extra) {
    const float x = num / m;
    const float slack = 1.0f + (mag * 0x1p-19f) / fabsf(m) + fabsf(x) * 0x1p-22f;
    float t = LOW ? ceilf(x + slack) + (float)extra : floorf(x - slack);
    const float all = LOW ? kPpLim : -kPpLim;
    if (!(t == t)) t = all;  // NaN: let the exact epilogue decide
    t = fminf(fmaxf(t, -kPpLim), kPpLim);
    return (int)t;
}
// Non-finite inputs, walked (the bound may only ever be too permissive; `all` is the bound every s passes):
//   num NaN (a NaN pivot or q_off; pivot and q_off infinite alike: inf - inf)   x = NaN -> t = NaN -> all
//   num +-inf, m finite     x = +-inf and slack = +inf: x -+ slack is +-inf on the permissive side (clamped to all) or
//                           inf - inf = NaN -> all
//   v_off NaN or +-inf      never gets here: pp_row_bound gives such a row a bound that beats every query's
//   m NaN                   x = NaN -> all
//   m = +-inf, num finite   x = +-0, slack = 1: a finite bound near 0 - but then every score is m * s = +-inf (s > 0) or
//                           NaN (s = 0), so is every sample score and with them the pivot: the query's bound is `all`
//                           (pp_query_bound) and cancels nothing.  (Such a store has no pre-filter anyway: u8_gemm_route
//                           sends multiplier 0 and inf to u8_gemm_kernel.)
//   m = 0                   x = +-inf or 0 / 0, slack = inf or NaN: as above, all
// The bound of a ROW.  A row whose offset is NaN or infinite has a NaN or infinite score whatever s is, and must reach
// the exact epilogue against EVERY query bound, a clamped "nothing passes" (+-kPpLim) included: its bound is 2 kPpLim on
// the permissive side, which no query bound cancels (s - B_q - B_row stays inside an int: |B_q| <= 2^29, s < 2^29).
template <bool LOW>
__device__ __forceinline__ int pp_row_bound(float v_off, float m) {
    if (!(fabsf(v_off) < __builtin_huge_valf())) return LOW ? 2 * (int)kPpLim : -2 * (int)kPpLim;
    return pp_bound<LOW>(-v_off, fabsf(v_off), m, 0);
}
// The bound of a QUERY.  A padding query (not `real`) gets the bound nothing passes.  An infinite pivot gets `all`: at
// the worst end of the order everything passes anyway, and at the best end (more sampled rows than the pivot rank
// score +-inf) the rows that tie with it or beat it - the same infinity, a NaN of that sign - must reach the exact
// epilogue, and a row's permissive bound cannot be relied on to cancel a query's "never" (LOW: the sum would have
// to exceed every s).  Such a query pays the exact epilogue for every row and, with that many ties, usually ends
// in the exact single-query path.
template <bool LOW>
__device__ __forceinline__ int pp_query_bound(float pivot, float q_off, float m, bool real) {
    int b = pp_bound<LOW>(pivot - q_off, fabsf(pivot) + fabsf(q_off), m, 1);  // LOW: s <= T  <=>  s - (T + 1) < 0
    if (__builtin_isinf(pivot)) b = LOW ? (int)kPpLim : -(int)kPpLim;
    if (!real) b = LOW ? -(int)kPpLim : (int)kPpLim;
    return b;
}


// Gather `n` sampled rows (codes + offsets) into a dense sub-store for the pivot pass, followed by
// `pad` zero rows (the GEMM kernels read whole row tiles).
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4 *__restrict__ codes,
                                                         const float *__restrict__ offsets, uint32_t row_chunks,
                                                         uint64_t n_rows, uint32_t n, uint32_t pad,
                                                         uint4 *__restrict__ out_codes,
                                                         float *__restrict__ out_offsets) {
    const uint64_t total = (uint64_t)(n + pad) * row_chunks;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = (uint32_t)(i / row_chunks), c = (uint32_t)(i % row_chunks);
        if (j >= n) {
            out_codes[i] = make_uint4(0, 0, 0, 0);
            if (c == 0) out_offsets[j] = 0.0f;
            continue;
        }
        const unsigned long long hsh = (unsigned long long)j * 0x9E3779B97F4A7C15ull;
        const uint64_t src = ((hsh >> 32) * n_rows) >> 32;  // same golden-ratio scatter as topk.hip
        out_codes[i] = codes[src * row_chunks + c];
        if (c == 0) out_offsets[j] = offsets[src];
    }
}

// Wave-private candidate lists -> per-query lists (grid = wave lists).  A list that overflowed
// sets *overflow: the caller then redoes every query exactly.
__global__ __launch_bounds__(256) void wave_scatter_kernel(const uint4 *__restrict__ wave_cand,
                                                          const uint32_t *__restrict__ wave_counts, uint32_t wave_cap,
                                                          uint32_t *__restrict__ counters,
                                                          unsigned long long *__restrict__ candidates,
                                                          uint32_t *__restrict__ overflow) {
    const uint32_t w = blockIdx.x;
    uint32_t count = wave_counts[w];
    if (count > wave_cap) {
        if (threadIdx.x == 0) *overflow = 1;
        count = wave_cap;
    }
    const uint4 *list = wave_cand + (uint64_t)w * wave_cap;
    for (uint32_t i = threadIdx.x; i < count; i += 256) {
        const uint4 c = list[i];
        const uint32_t pos = atomicAdd(counters + (uint64_t)c.z * kCounterStride, 1u);
        if (pos < kBatchCap) candidates[(uint64_t)c.z * kBatchCap + pos] = ((unsigned long long)c.x << 32) | c.y;
    }
}

// The same with the global atomics aggregated: a workgroup takes a range of wave lists, counts its entries per
// query in LDS, reserves one range per (workgroup, query) with ONE global atomic and places the entries by
// LDS ranks.  Same-address global atomics serialise at ~25 ns each: one per candidate was 15-50 us of every
// call (1024-2048 per query); this way a query's counter sees one add per workgroup.  n_queries <= 4096.
__global__ __launch_bounds__(1024) void wave_scatter_grouped_kernel(const uint4 *__restrict__ wave_cand,
                                                                   const uint32_t *__restrict__ wave_counts,
                                                                   uint32_t wave_cap, uint32_t n_lists, uint32_t n_queries,
                                                                   uint32_t *__restrict__ counters,
                                                                   unsigned long long *__restrict__ candidates,
                                                                   uint32_t *__restrict__ overflow) {
    extern __shared__ uint32_t scatter_lds[];
    uint32_t *hist = scatter_lds, *base = scatter_lds + n_queries;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (uint32_t i = t; i < n_queries; i += 1024) hist[i] = 0;
    __syncthreads();
    const uint32_t l0 = (uint32_t)((uint64_t)blockIdx.x * n_lists / gridDim.x);
    const uint32_t l1 = (uint32_t)((uint64_t)(blockIdx.x + 1) * n_lists / gridDim.x);
    for (uint32_t l = l0 + wave; l < l1; l += 16) {  // one wave per list
        uint32_t count = wave_counts[l];
        if (count > wave_cap) {
            if (lane == 0) *overflow = 1;
            count = wave_cap;
        }
        const uint4 *list = wave_cand + (uint64_t)l * wave_cap;
        for (uint32_t i = lane; i < count; i += 64) atomicAdd(&hist[list[i].z], 1u);
    }
    __syncthreads();
    for (uint32_t i = t; i < n_queries; i += 1024) {
        const uint32_t cnt = hist[i];
        base[i] = cnt ? atomicAdd(counters + (uint64_t)i * kCounterStride, cnt) : 0u;
        hist[i] = 0;
    }
    __syncthreads();
    for (uint32_t l = l0 + wave; l < l1; l += 16) {
        const uint32_t count = min(wave_counts[l], wave_cap);
        const uint4 *list = wave_cand + (uint64_t)l * wave_cap;
        for (uint32_t i = lane; i < count; i += 64) {
            const uint4 c = list[i];
            const uint32_t pos = base[c.z] + atomicAdd(&hist[c.z], 1u);
            if (pos < kBatchCap) candidates[(uint64_t)c.z * kBatchCap + pos] = ((unsigned long long)c.x << 32) | c.y;
        }
    }
}

// Per-query pivot (grid = queries): r-th best of 1024 per-thread bests of the query's sample
// scores (see pivot_kernel in topk.hip), and counter reset.
__global__ __launch_bounds__(1024) void batch_pivot_kernel(const float *__restrict__ sample, uint32_t S,
                                                          uint64_t pitch, uint32_t r, int largest,
                                                          uint32_t n_queries, float *__restrict__ pivot_scores,
                                                          uint32_t *__restrict__ counters) {
    __shared__ unsigned long long lists[kSmallTopkWaves][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (blockIdx.x >= n_queries) {  // padding query of the last tile: nothing may pass
        if (t == 0) pivot_scores[blockIdx.x] = largest ? __builtin_huge_valf() : -__builtin_huge_valf();
        return;
    }
    const float *mine_row = sample + (uint64_t)blockIdx.x * pitch;
    uint32_t mine = 0xFFFFFFFFu;
    for (uint32_t i = t; i < S; i += 1024) {
        const uint32_t key = topk_ordered_bits(mine_row[i], largest != 0);
        mine = key < mine ? key : mine;
    }
    // the r-th best (r <= 64) of the 1024 per-thread bests: a sort per wave, the 16 waves folded pairwise
    // (21 + 4 x 6 register stages instead of the 55 barrier stages of a 1024-key bitonic sort)
    unsigned long long best = wave_sort64((unsigned long long)mine << 32, lane);
    best = small_topk_fold_waves(best, lists, wave, lane);
    r = r < 1 ? 1 : (r > 64 ? 64 : r);
    if (wave == 0 && lane == (int)r - 1) {
        pivot_scores[blockIdx.x] = topk_score_of_key((uint32_t)(best >> 32), largest != 0);
        counters[(uint64_t)blockIdx.x * kCounterStride] = 0;
    }
}

// Per-query emit (grid = queries): sort the query's candidates, write its k best; status 1
// when the list over- or under-flowed (that query is redone exactly by the caller).
__global__ __launch_bounds__(1024) void batch_emit_kernel(const unsigned long long *__restrict__ cand,
                                                         const uint32_t *__restrict__ counters, uint64_t n,
                                                         uint32_t k, int largest, uint32_t *__restrict__ out_ids,
                                                         float *__restrict__ out_scores,
                                                         uint32_t *__restrict__ status) {
    __shared__ unsigned long long s[kBatchCap];
    const int t = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t pushed = counters[(uint64_t)q * kCounterStride];
    const uint32_t k_eff = n < k ? (uint32_t)n : k;
    if (pushed > kBatchCap || pushed < k_eff) {
        if (t == 0) status[q] = 1;
        return;
    }
    uint32_t N = 64;
    while (N < pushed) N <<= 1;
    const unsigned long long *mine = cand + (uint64_t)q * kBatchCap;
    for (uint32_t i = t; i < N; i += 1024) s[i] = i < pushed ? mine[i] : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= N; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = t; i < N / 2; i += 1024) {
                const uint32_t a = 2 * i - (i & (stride - 1));
                const uint32_t bb = a + stride;
                const bool up = (a & size) == 0;
                const unsigned long long x = s[a], y = s[bb];
                if ((x > y) == up) {
                    s[a] = y;
                    s[bb] = x;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = t; i < k; i += 1024) {
        if (i < k_eff) {
            out_ids[(uint64_t)q * k + i] = (uint32_t)(s[i] & 0xFFFFFFFFull);
            out_scores[(uint64_t)q * k + i] = topk_score_of_key((uint32_t)(s[i] >> 32), largest != 0);
        } else {
            out_ids[(uint64_t)q * k + i] = 0xFFFFFFFFu;
            out_scores[(uint64_t)q * k + i] = largest ? -__builtin_huge_valf() : __builtin_huge_valf();
        }
    }
    if (t == 0) status[q] = 0;
}

// The same for k <= 64 without the full sort: every wave keeps the 64 best of its share of the candidates
// (wave_sort64 of 64 at a time + a 6-stage merge, all in registers), the 16 waves fold pairwise through
// LDS: ~30 DPP/LDS stages instead of the 66-91 barrier stages of the bitonic sort above (15-40 us per
// call whatever the batch size, since the queries' workgroups run side by side).
__global__ __launch_bounds__(1024) void batch_emit_wave_kernel(const unsigned long long *__restrict__ cand,
                                                              const uint32_t *__restrict__ counters, uint64_t n,
                                                              uint32_t k, int largest, uint32_t *__restrict__ out_ids,
                                                              float *__restrict__ out_scores,
                                                              uint32_t *__restrict__ status) {
    __shared__ unsigned long long lists[kSmallTopkWaves][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t q = blockIdx.x;
    const uint32_t pushed = counters[(uint64_t)q * kCounterStride];
    const uint32_t k_eff = n < k ? (uint32_t)n : k;
    if (pushed > kBatchCap || pushed < k_eff) {
        if (t == 0) status[q] = 1;
        return;
    }
    const unsigned long long *mine = cand + (uint64_t)q * kBatchCap;
    unsigned long long best = ~0ull;
    for (uint32_t base = (uint32_t)wave * 64; base < pushed; base += 1024) {
        unsigned long long v = base + lane < pushed ? mine[base + lane] : ~0ull;
        v = wave_sort64(v, lane);
        best = wave_merge64_rev(best, shfl_u64(v, 63 - lane), lane);
    }
    best = small_topk_fold_waves(best, lists, wave, lane);
    if (wave == 0) {
        for (uint32_t i = lane; i < k; i += 64) {
            if (i < k_eff) {
                out_ids[(uint64_t)q * k + i] = (uint32_t)(best & 0xFFFFFFFFull);
                out_scores[(uint64_t)q * k + i] = topk_score_of_key((uint32_t)(best >> 32), largest != 0);
            } else {
                out_ids[(uint64_t)q * k + i] = 0xFFFFFFFFu;
                out_scores[(uint64_t)q * k + i] = largest ? -__builtin_huge_valf() : __builtin_huge_valf();
            }
        }
        if (lane == 0) status[q] = 0;
    }
}


// waves (= candidate lists) of one launch of a persistent 8-wave-per-CU matrix-core kernel
inline uint32_t pp_waves_per_launch() { return (uint32_t)std::max(1, device_info().cu_count / 8) * 8 * 8; }

// fn(std::bool_constant<LOW>): LOW is the direction of the integer pre-filter of MODE 1 / 2 - "may pass" is s <= bound
// when the score falls with s (multiplier < 0) xor smallest-first.  The other modes have no pre-filter (LOW = false).
template <int MODE, typename Fn>
qamd_status with_low(float multiplier, Fn &&fn) {
    if constexpr (MODE == 1 || MODE == 2) {
        if ((multiplier < 0.0f) != (MODE == 2)) return fn(std::true_type{});
    }
    return fn(std::false_type{});
}

// QAMD_DEBUG_TOPK (tools/lib build): one line per matrix-core topk_batch call on stderr.
inline bool batch_debug_topk() {
    static const bool on = dev_env("QAMD_DEBUG_TOPK") != nullptr;
    return on;
}

// The host side of one matrix-core topk_batch pass, used in a straight line:
//     BatchTopkPass pass(n, Q, q_pad, k, largest, n_lists, wave_cap, stream);
//     off = pass.reserve(bytes) ...             the quantizer's own scratch (sample scores, ...)
//     pass.alloc()                              one allocation, one memset
//     <sample GEMM>  pass.pivots(...)  <filter GEMM with pass.filter()>  pass.scatter()
//     pass.emit(ids, scores)  pass.read_status(status)  pass.debug_line(...)
// n_lists = 0: the filter kernel appends to the per-query lists itself (no wave-private lists, no scatter).
struct BatchTopkPass {
    const uint64_t n, Q, q_pad;
    const uint32_t k;
    const int largest;
    const uint32_t n_lists, wave_cap;
    const hipStream_t s;
    // ONE stream-ordered allocation for all scratch of the call, carved up here: hipFreeAsync
    // costs ~65 us per buffer on this runtime, and ten buffers were a third of a small batch's time.
    StreamBuf arena;
    size_t arena_bytes = 0, zero_bytes = 0;
    size_t o_pivots, o_counters, o_wcounts, o_cand = 0, o_status = 0, o_bounds = 0, o_wcand = 0;
    char *base = nullptr;
    HostScratch hs;
    uint32_t *status_dev = nullptr;  // [Q] per-query status, then the wave-list overflow flag

    BatchTopkPass(uint64_t n_, uint64_t Q_, uint64_t q_pad_, uint32_t k_, int largest_, uint32_t n_lists_, uint32_t wave_cap_,
                  hipStream_t s_)
        : n(n_), Q(Q_), q_pad(q_pad_), k(k_), largest(largest_), n_lists(n_lists_), wave_cap(wave_cap_), s(s_) {
        // zero-initialised part first (one memset): pivots, counters, wave counts
        o_pivots = reserve(q_pad * 4);
        o_counters = reserve(q_pad * kCounterStride * 4);
        o_wcounts = reserve((uint64_t)n_lists * 4);
        zero_bytes = arena_bytes;
    }
    size_t reserve(size_t bytes) {
        const size_t off = arena_bytes;
        arena_bytes += round_up(std::max<size_t>(bytes, 16), 256);
        return off;
    }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    // query_bounds: the filter kernel wants [q_pad] words of scratch for its integer bounds (BatchFilter::query_bounds)
    qamd_status alloc(bool query_bounds = false) {
        o_cand = reserve(Q * (uint64_t)kBatchCap * 8);
        o_status = reserve((Q + 1) * 4);
        if (query_bounds) o_bounds = reserve(q_pad * 4);
        o_wcand = reserve((uint64_t)n_lists * wave_cap * sizeof(uint4));
        QAMD_TRY(arena.alloc(arena_bytes, s));
        base = arena.as<char>();
        QAMD_HIP(hipMemsetAsync(base, 0, zero_bytes, s));
        // The per-query status words and the overflow flag come back through the calling thread's mapped
        // host scratch when they fit (the kernels write host memory directly: one stream sync, no copy
        // calls), else through one copy from the arena.
        hs = Q + 1 <= 2048 ? host_scratch() : HostScratch{};
        status_dev = hs.dev ? hs.dev : at<uint32_t>(o_status);
        if (hs.host) hs.host[Q] = 0;
        else QAMD_HIP(hipMemsetAsync(status_dev + Q, 0, 4, s));
        return QAMD_OK;
    }
    float *pivot_scores() const { return at<float>(o_pivots); }
    uint32_t *counters() const { return at<uint32_t>(o_counters); }
    unsigned long long *candidates() const { return at<unsigned long long>(o_cand); }
    BatchFilter filter() const {
        BatchFilter f{};
        f.pivot_scores = pivot_scores();
        f.counters = counters();
        f.candidates = candidates();
        f.largest = largest;
        f.n_queries = (uint32_t)Q;
        if (o_bounds) f.query_bounds = at<int>(o_bounds);
        if (n_lists) {
            f.wave_cap = wave_cap;
            f.wave_cand = at<uint4>(o_wcand);
            f.wave_counts = at<uint32_t>(o_wcounts);
        }
        return f;
    }
    // every query's pivot: the r-th best of its `cols` sample scores (or block bests) in scores[q * pitch ...]
    void pivots(const float *scores, uint32_t cols, uint64_t pitch, uint32_t r) {
        hipLaunchKernelGGL(batch_pivot_kernel, dim3((unsigned)q_pad), dim3(1024), 0, s, scores, cols, pitch, r, largest, (uint32_t)Q,
                           pivot_scores(), counters());
    }
    // wave-private lists -> per-query lists.  Nothing to do for a pass without wave lists.
    void scatter() {
        if (!n_lists) return;
        if (Q <= 4096)
            hipLaunchKernelGGL(wave_scatter_grouped_kernel, dim3(std::min<uint32_t>(n_lists, 128)), dim3(1024), (size_t)Q * 8, s,
                               at<uint4>(o_wcand), at<uint32_t>(o_wcounts), wave_cap, n_lists, (uint32_t)Q, counters(), candidates(),
                               status_dev + Q);
        else
            hipLaunchKernelGGL(wave_scatter_kernel, dim3(n_lists), dim3(256), 0, s, at<uint4>(o_wcand), at<uint32_t>(o_wcounts), wave_cap,
                               counters(), candidates(), status_dev + Q);
    }
    qamd_status emit(uint32_t *ids_dev, float *sc_dev) {
        if (k <= kSmallTopkMaxK)
            hipLaunchKernelGGL(batch_emit_wave_kernel, dim3((unsigned)Q), dim3(1024), 0, s, candidates(), counters(), n, k, largest,
                               ids_dev, sc_dev, status_dev);
        else
            hipLaunchKernelGGL(batch_emit_kernel, dim3((unsigned)Q), dim3(1024), 0, s, candidates(), counters(), n, k, largest, ids_dev,
                               sc_dev, status_dev);
        QAMD_HIP(hipGetLastError());
        return QAMD_OK;
    }
    // status[q] != 0: query q must be redone exactly (its list over- or underflowed).  Synchronises the stream.
    qamd_status read_status(std::vector<uint32_t> &status) {
        uint32_t overflow = 0;
        if (hs.host) {
            QAMD_HIP(hipStreamSynchronize(s));
            std::copy(hs.host, hs.host + Q, status.begin());
            overflow = hs.host[Q];
        } else {
            std::vector<uint32_t> back(Q + 1);
            QAMD_TRY(copy_out(back.data(), QAMD_MEM_HOST, status_dev, (Q + 1) * 4, s));  // synchronises
            std::copy(back.begin(), back.begin() + Q, status.begin());
            overflow = back[Q];
        }
        // A wave list overflowed: redo all exactly.  Only the two scatter kernels write the flag (alloc() clears it), so a
        // pass without wave lists, which runs neither, reads 0 here: no test of n_lists is needed.
        if (overflow) std::fill(status.begin(), status.end(), 1u);
        return QAMD_OK;
    }
    void debug_line(const char *tag, uint32_t r, const char *kernel_name, const char *tail, const std::vector<uint32_t> &status) {
        if (!batch_debug_topk()) return;
        std::vector<uint32_t> cnt(q_pad * kCounterStride);
        (void)hipMemcpy(cnt.data(), counters(), cnt.size() * 4, hipMemcpyDeviceToHost);
        uint32_t mx = 0, mn = ~0u, redo = 0;
        uint64_t sum = 0;
        for (uint64_t q = 0; q < Q; q++) {
            const uint32_t c = cnt[q * kCounterStride];
            mx = std::max(mx, c);
            mn = std::min(mn, c);
            sum += c;
            redo += status[q] != 0;
        }
        fprintf(stderr, "%s Q=%llu r=%u candidates min/mean/max = %u/%llu/%u, filter %s, %u queries redone%s\n", tag,
                (unsigned long long)Q, r, mn, (unsigned long long)(sum / Q), mx, kernel_name, redo, tail);
    }
};

// The outputs of a topk_batch whose matrix-core pass may leave queries to an exact single-query path: host outputs are
// staged in device memory, status[q] != 0 marks the queries to redo (all of them until a pass says otherwise).
struct BatchTopkOutputs {
    StreamBuf ids_tmp, sc_tmp;
    uint32_t *ids_dev = nullptr;  // [Q][k], device memory: the caller's own, or the staging copy
    float *sc_dev = nullptr;
    std::vector<uint32_t> status;
    uint64_t Q = 0;
    uint32_t k = 0;
    uint32_t *out_ids = nullptr;
    float *out_scores = nullptr;
    qamd_mem out_mem = QAMD_MEM_DEVICE;
    hipStream_t s = nullptr;

    qamd_status begin(uint64_t Q_, uint32_t k_, uint32_t *out_ids_, float *out_scores_, qamd_mem out_mem_, hipStream_t s_) {
        Q = Q_, k = k_, out_ids = out_ids_, out_scores = out_scores_, out_mem = out_mem_, s = s_;
        ids_dev = out_ids;
        sc_dev = out_scores;
        if (out_mem == QAMD_MEM_HOST) {
            QAMD_TRY(ids_tmp.alloc(Q * k * 4, s));
            QAMD_TRY(sc_tmp.alloc(Q * k * 4, s));
            ids_dev = ids_tmp.as<uint32_t>();
            sc_dev = sc_tmp.as<float>();
        }
        status.assign(Q, 1);
        return QAMD_OK;
    }
    // redo(q, ids_dev, scores_dev): the quantizer's exact top-k of query q into device memory
    template <class Redo>
    qamd_status finish(Redo &&redo) {
        for (uint64_t q = 0; q < Q; q++) {
            if (!status[q]) continue;
            QAMD_TRY(redo(q, ids_dev + q * k, sc_dev + q * k));
        }
        if (out_mem == QAMD_MEM_HOST) {
            QAMD_TRY(copy_out(out_ids, QAMD_MEM_HOST, ids_dev, Q * k * 4, s));
            QAMD_TRY(copy_out(out_scores, QAMD_MEM_HOST, sc_dev, Q * k * 4, s));
        } else {
            QAMD_HIP(hipStreamSynchronize(s));  // scratch buffers are released on return
        }
        return QAMD_OK;
    }
};

}  // namespace
}  // namespace qamd
