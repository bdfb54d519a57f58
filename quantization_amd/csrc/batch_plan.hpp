// The pivot sample of a matrix-core topk_batch (u8_batch.hip, bin.hip): how many rows to sample, which rank of them is
// the pivot, how many rows are then expected to pass the filter.  A pure function of plain numbers; host only, plain
// C++17 with no HIP header, so tests/cpu/bin_batch_route_dump.cpp prints it with g++ alone
// (tests/golden/bin_batch_route_table.txt).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace qamd {

constexpr uint32_t kTopkSample = 16384;  // sampled rows of a fused top-k (topk.hpp) on stores of 2^20 rows and more

struct BatchSamplePlan {
    double want = 0;        // rows that should pass the filter, per query
    double s_min = 0;       // the smallest sample
    uint32_t S = 0;         // sampled rows
    double target = 0;      // rows expected to pass with this sample (>= want)
    uint32_t r = 0;         // pivot rank among the S sample scores (0 for an empty store)
    uint32_t rows_all = 0;  // the sample a handle caches: the largest any call can ask for; every call uses a prefix
};

constexpr uint64_t plan_round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

inline BatchSamplePlan batch_sample_plan(uint64_t n, uint64_t Q, uint32_t k) {
    // Pivot rank r of S sampled rows: the number of rows at least as good as the pivot is about
    // n*Beta(r, S-r+1): mean n*r/S, relative spread 1/sqrt(r).  With many queries per call both tails
    // matter (a list that overflows kBatchCap or holds fewer than k rows sends its query to the exact
    // single-query path, milliseconds each), and so does the mean: every passing (query, row) pair
    // costs an exact epilogue + a list append inside the GEMM (2048 expected per query instead of 512
    // measured +7..10 % on the whole call).  So: about max(512, 3k) rows expected to pass at pivot
    // rank >= 8 (P(fewer than k) < 1e-7, P(more than 8192) ~ 0); S = 8 n / that, capped at 524288
    // sampled rows (beyond 33M rows the expected count grows instead of r shrinking).
    // Few queries: a smaller sample (cheaper pivot pass) and more candidates per query instead (measured at
    // 10M x 768, 5-128 queries: 1024 expected beats 512 by 0.01-0.02 ms and 2048 by 0.03-0.08 ms - the
    // per-query scatter and sort of the candidates grow faster than the sample pass shrinks).
    const double want = std::max<double>(Q <= 128 ? 1024.0 : 512.0, 3.0 * k);
    // small stores (Qdrant segments: 1e5..1e6 rows) take the same route with a smaller sample: the
    // per-query fallback costs a launch chain per query, the matrix-core pass one for the whole batch
    const double s_min = n < (1u << 20) ? 2048.0 : (double)kTopkSample;
    const double s_mem_cap = std::max<double>(s_min, std::floor((double)(6ull << 30) / (4.0 * (double)Q) / 256.0) * 256.0);  // <= 6 GB of sample scores
    const uint32_t S = (uint32_t)std::min<double>(std::min<double>(524288.0, s_mem_cap),
                                                  std::max<double>(s_min, plan_round_up((uint64_t)(8.0 * (double)n / want), 256)));
    const double target = std::max<double>(want, 8.0 * (double)n / (double)S);
    const uint32_t r = n ? (uint32_t)std::ceil((double)S * target / (double)n) : 0;
    // (the sample scores are Q x S f32: 0.6 GB at 1024 queries and 10M rows, 5 GB at 8192 queries)
    const uint32_t rows_all = (uint32_t)std::min<double>(524288.0, std::max<double>(s_min, (double)plan_round_up((uint64_t)(8.0 * (double)n / 512.0), 256)));
    return {want, s_min, S, target, r, rows_all};
}

}  // namespace qamd
