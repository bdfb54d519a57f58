// E_q of csrc/f32_mfma_bound.hpp against models of the matrix unit: the products of the ROUNDED query and the row summed in three
// orders, adds to nearest or toward zero, inputs below the smallest normal flushed or not; all within E_q of the exact f32 score.
#include "../../quantization_amd/csrc/f32_mfma_bound.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace qamd;

static float round_bf16(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    memcpy(&v, &u, 4);
    return v;
}
static float round_f16(float v) {  // nearest even on the f16 grid (subnormals kept), overflow to infinity
    if (v == 0.0f) return v;
    if (std::fabs(v) >= 65520.0f) return std::copysign(HUGE_VALF, v);
    const int e = std::ilogb(v) < -14 ? -14 : std::ilogb(v);
    const float quantum = std::ldexp(1.0f, e - 10);
    return std::nearbyint(v / quantum) * quantum;
}

static float add(float a, float b, bool truncate) {
    if (!truncate) return a + b;
    const double d = (double)a + (double)b;
    float f = (float)d;
    if (std::fabs((double)f) > std::fabs(d)) f = std::nextafterf(f, 0.0f);
    return f;
}
static float sum_range(const std::vector<float> &p, size_t lo, size_t hi, int order, bool truncate) {
    if (order == 1 && hi - lo > 1) {  // pairwise
        const size_t mid = lo + (hi - lo) / 2;
        return add(sum_range(p, lo, mid, order, truncate), sum_range(p, mid, hi, order, truncate), truncate);
    }
    float s = 0.0f;
    for (size_t i = lo; i < hi; i++) s = add(s, p[i], truncate);
    return s;
}
static float model(const std::vector<float> &p, int order, bool truncate) {
    if (order != 2) return sum_range(p, 0, p.size(), order, truncate);
    float s = 0.0f;  // blocks of 16, block sums added in order
    for (size_t b = 0; b < p.size(); b += 16) s = add(s, sum_range(p, b, std::min(p.size(), b + 16), 0, truncate), truncate);
    return s;
}

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    double worst = 0.0;
    for (int f16 = 0; f16 < 2; f16++) {
        const MfmaElem elem = f16 ? kMfmaF16 : kMfmaBF16;
        auto rnd = [&](float v) { return f16 ? round_f16(v) : round_bf16(v); };
        for (uint32_t dim : {8u, 24u, 264u, 768u})
            for (int kind = 0; kind < 3; kind++) {  // uniform; one huge coordinate; the element type's subnormal range
                std::vector<std::vector<float>> rows(64, std::vector<float>(dim));
                float amax = 0.0f;
                for (auto &x : rows) {
                    for (auto &v : x) v = rnd(uni(rng) * (kind == 2 ? (float)elem.t : 1.0f));
                    if (kind == 1) x[rng() % dim] = rnd(f16 ? 1000.0f : 1.0e4f);
                    for (float v : x) amax = std::max(amax, std::fabs(v));
                }
                for (int qi = 0; qi < 4; qi++) {
                    std::vector<float> q(dim), qh(dim);
                    float l1 = 0.0f;
                    for (uint32_t i = 0; i < dim; i++) {
                        q[i] = uni(rng) * (qi == 3 ? 1.0e-5f : 1.0f);
                        qh[i] = rnd(q[i]);
                        l1 += std::fabs(q[i]);
                    }
                    const double E = f32_mfma_bound(elem, dim, l1, amax);
                    if (!(E < HUGE_VAL)) return printf("unbounded: f16 %d dim %u kind %d\n", f16, dim, kind), 1;
                    for (const auto &x : rows) {
                        float exact = 0.0f;
                        for (uint32_t i = 0; i < dim; i++) {
                            volatile float p = q[i] * x[i];  // rounded to f32 before its add: no contraction
                            exact += p;
                        }
                        for (int flush = 0; flush < 2; flush++) {
                            std::vector<float> p(dim);
                            for (uint32_t i = 0; i < dim; i++) {
                                const bool lost = flush && (std::fabs(qh[i]) < elem.t || std::fabs(x[i]) < elem.t);
                                p[i] = lost ? 0.0f : (float)((double)qh[i] * (double)x[i]);
                                if (flush && std::fabs(p[i]) < 0x1p-126f) p[i] = 0.0f;
                            }
                            for (int order = 0; order < 3; order++)
                                for (int truncate = 0; truncate < 2; truncate++) {
                                    const double err = std::fabs((double)model(p, order, truncate != 0) - (double)exact);
                                    if (!(err <= E))
                                        return printf("f16 %d dim %u kind %d order %d truncate %d flush %d: error %g > E %g\n", f16, dim,
                                                      kind, order, truncate, flush, err, E), 1;
                                    worst = std::max(worst, err / E);
                                }
                        }
                    }
                    const float tau = uni(rng) * l1 * amax;
                    if ((double)f32_mfma_threshold(tau, E, true) > (double)tau - E || (double)f32_mfma_threshold(tau, E, false) < (double)tau + E)
                        return printf("threshold inside the bound\n"), 1;
                }
            }
    }
    printf("largest error / E = %.3f\nok\n", worst);
    return 0;
}
