// E_q of the matrix-core filter of OriginalVectors.topk_batch (f32_mfma.hip): how far the filter's sum for
// (query q, any row x) can lie from the exact score of that pair.  Compiles on the host: the kernel's host side and
// tests/cpu/f32_mfma_bound.cpp share it.
//
// exact = the sequential f32 chain of fl(q_i * x_i) (f32.hip), q in f32, x widened exactly.
// filter = a sum of the products qh_i * x_i in f32, qh = q rounded to the element type (nearest even), added in ANY
//          order, each add rounded to nearest or toward zero, subnormal inputs or results possibly flushed to zero.
// With u the unit roundoff of the element type, t the smallest normal of the element type, eps = 2^-23, |x_i| <= amax:
//   query rounding     |qh_i - q_i| <= max(u |q_i|, u t)                  -> u L1 amax + dim u t amax
//   flushed x_i        |x_i| < t: the term qh_i x_i is lost               -> (1 + u) L1 min(amax, t)
//   flushed qh_i       |qh_i| < t: the term is lost                       -> dim t amax
//   filter's adds      n = dim + 1 adds (one into the zero accumulator, or one product rounding), each within eps relative:
//                      gamma_n sum |qh_i x_i| <= (1 + d) n eps (1 + u) L1 amax,  d = n eps / (1 - n eps)
//   exact chain        dim products and dim adds to nearest (2^-24 each): (1 + d) (dim + 1) (eps / 2) L1 amax
//   f32 underflow      a flushed or subnormal f32 product or partial sum, either chain: 2^-126 each, 4 (dim + 1) of them
//   L1 itself          the kernel's f32 sum of |q_i|, any order, is at least L1 (1 - dim eps / 2)
// dim <= 65536 keeps n eps <= 2^-7, so (1 + d)(1 + u)(1 + dim eps) <= 1.02 and the two chains together stay below
// c (dim + 2) eps L1 amax with c = 2 (1.02 * 1.5 = 1.53); the rest of c pays for the L1 slack on the u term.  Hence
//   E_q = (u + 2 (dim + 2) 2^-23) L1 amax  +  (1 + u) L1 min(amax, t) + (1 + u) dim t amax + 4 (dim + 1) 2^-126,
// evaluated in double and widened by 2^-20 for that evaluation.  Partial sums stay finite when L1 amax < 2^126; a larger
// product, a non-finite input, or dim > 65536 gives +inf: the query "cannot be bounded" and takes the exact route.
#pragma once

#include <cmath>
#include <cstdint>

namespace qamd {

constexpr uint32_t kMfmaBoundMaxDim = 65536;

struct MfmaElem {
    double u;  // unit roundoff
    double t;  // smallest normal
};
constexpr MfmaElem kMfmaF16{0x1p-11, 0x1p-14}, kMfmaBF16{0x1p-8, 0x1p-126};

// l1: the f32 sum of |q_i| in any order; amax: max |x| over the rows.
inline double f32_mfma_bound(MfmaElem e, uint32_t dim, float l1, float amax) {
    const double L = l1, a = amax;
    if (!(L >= 0.0) || !(a >= 0.0) || std::isinf(L) || std::isinf(a) || dim > kMfmaBoundMaxDim || !(L * a < 0x1p126))
        return HUGE_VAL;
    const double rel = (e.u + 2.0 * (dim + 2.0) * 0x1p-23) * L * a;
    const double abs = (1.0 + e.u) * (L * (a < e.t ? a : e.t) + dim * e.t * a) + 4.0 * (dim + 1.0) * 0x1p-126;
    return (rel + abs) * (1.0 + 0x1p-20);
}

// The f32 threshold the filter compares with: the exact tau -/+ E rounded AWAY from tau, so that rounding never rejects a row
// the real-number test keeps.  below: for "largest" (a sum under it is provably worse), else the mirrored one.
inline float f32_mfma_threshold(float tau, double E, bool below) {
    const double t = below ? (double)tau - E : (double)tau + E;  // exact enough: 53 bits against E's 2^-20 slack
    float f = (float)t;
    if (below ? (double)f > t : (double)f < t) f = std::nextafterf(f, below ? -HUGE_VALF : HUGE_VALF);
    return f;
}

}  // namespace qamd
