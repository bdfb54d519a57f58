// The arithmetic of the packed 8-bit filter tables of the PQ batch top-k (pq.hip: pq_lut_pack4_kernel builds them,
// pq_scan_pack4_kernel scans with them - rows of up to 128 chunks whole, rows of 160 .. 256 chunks slice by slice).  Plain C++17 for host and device, so that the bound can be checked on a CPU
// (tests/cpu/pq_pack4_bound.cpp).
//
// A filter pass only has to REJECT rows safely; the exact f32 score of the few survivors decides.  One byte per table entry
// puts four queries' tables into the LDS space of one f32 table, and one `ds_read_b32` gather then serves four queries.
//
// All of it is written for a largest-first search over L' = sgn * L (sgn = +1: largest first, -1: smallest first; the
// negation is exact), L the query's f32 table [chunk][code]:
//   lo[c]   = min_code L'[c][code]                      base = sum_c lo[c]   (double)
//   step    = max_c (max_code L'[c] - lo[c]) / 255      ONE step per query, so that integer sums add up
//   e[c][code] = ceil((L'[c][code] - lo[c]) / step), clamped to 0 .. 255
// so that  sum_c L'[c][code_c]  <=  base + step * (sum_c e[c][code_c] + eps)  in real numbers: the double roundings of the
// quotient (and a clamp of 255 + a rounding) lose less than 255 * 2^-51 of a step per chunk, eps < 1e-10 for m <= 256
// (256 * 255 * 2^-51 = 2.9e-11; the sum of a row's per-slice integer sums IS the row's sum, so slices change nothing here).
// The reference adds the m entries in f32, four lane sums of m / 4 terms and two combining adds: its score is within
//   slack = (m / 4 + 3) * 2^-24 * sum_c max_code |L[c][code]|
// of the real sum (first order (m / 4 + 1) u sum |x|; the two spare units cover the higher orders and the double roundings
// of base).  A row whose f32 score s' = sgn * s reaches the pivot p' therefore has
//   sum_c e  >=  (p' - base) / step - slack / step - eps,
// and the scan admits every row with  sum_c e >= floor((p' - base) / step - slack / step - 1).
// A query that cannot be bounded - a table entry that is not finite, step 0 (a constant table: every score the same) or
// not finite, sums that may overflow f32 - or a pivot that is NaN or infinite gets a threshold no sum reaches: the filter
// then keeps nothing, the candidate list underflows and the query is redone by the exact classic top-k.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define QAMD_PACK4_HD __host__ __device__ inline
#else
#define QAMD_PACK4_HD inline
#endif

namespace qamd {

constexpr uint32_t kPack4Never = 0xFFFFFFFFu;  // a threshold no sum of at most 256 * 255 = 65280 (a 16-bit field) reaches

struct Pack4Query {  // per (query, direction), four doubles in memory
    double base, step, slack, bad;  // bad != 0: the query cannot be bounded
};

// One chunk's 256 entries, folded into the query's running statistics (in the order c = 0, 1, ...).
struct Pack4Stats {
    double sum_min = 0.0, sum_max = 0.0, max_range = 0.0, sum_abs = 0.0;
    bool finite = true;
};
QAMD_PACK4_HD void pack4_add_chunk(Pack4Stats &s, float mn, float mx, bool finite) {
    s.sum_min += (double)mn;
    s.sum_max += (double)mx;
    const double range = (double)mx - (double)mn;
    s.max_range = range > s.max_range ? range : s.max_range;
    s.sum_abs += std::fmax(std::fabs((double)mn), std::fabs((double)mx));
    s.finite = s.finite && finite;
}

// m: chunks of a row (m % 4 == 0).  largest != 0: largest first.
QAMD_PACK4_HD Pack4Query pack4_params(const Pack4Stats &s, uint32_t m, int largest) {
    Pack4Query p;
    p.base = largest ? s.sum_min : -s.sum_max;
    p.step = s.max_range / 255.0;
    p.slack = (double)(m / 4 + 3) * 0x1p-24 * s.sum_abs * (1.0 + 0x1p-50);  // rounded up
    const bool ok = s.finite && p.step > 0.0 && std::isfinite(p.step) && s.sum_abs < 0x1p126;
    p.bad = ok ? 0.0 : 1.0;
    return p;
}

// The byte of entry v of a chunk whose extremes are mn / mx.
QAMD_PACK4_HD uint32_t pack4_entry(float v, float mn, float mx, double step, int largest) {
    const double up = largest ? (double)v - (double)mn : (double)mx - (double)v;  // L' - lo
    const double e = std::ceil(up / step);
    return e >= 255.0 ? 255u : e >= 1.0 ? (uint32_t)e : 0u;  // (NaN: 0 - such a query is `bad`)
}

// Rows whose integer sum is >= the result may reach `pivot` (the score at the filter's pivot key).
QAMD_PACK4_HD uint32_t pack4_threshold(const Pack4Query &p, float pivot, int largest) {
    if (p.bad != 0.0 || !std::isfinite(pivot)) return kPack4Never;
    const double pv = largest ? (double)pivot : -(double)pivot;
    const double t = std::floor((pv - p.base) / p.step - p.slack / p.step - 1.0);
    if (!(t > 0.0)) return 0u;  // every row passes (NaN cannot arise from finite operands and step > 0; it would land here, the safe side)
    return t >= 1e9 ? kPack4Never : (uint32_t)t;
}

}  // namespace qamd
