// The packed 8-bit filter bound of the PQ batch top-k (csrc/pq_pack4.hpp) on the CPU: no row whose f32 score, summed in the
// reference's order (lane sums of chunks k, k + 4, ..., then (l0 + l2) + (l1 + l3)), reaches the pivot may fail the integer
// test.  Random tables - uniform, mixed signs, chunk scales 2^-20 .. 2^20, the same on large offsets - random rows, both
// directions, pivots that ARE rows' scores (a tie at the pivot is the tightest case).  Exits 1 when a bound is violated.
#include <cstdio>
#include <random>
#include <vector>
#include "../../quantization_amd/csrc/pq_pack4.hpp"
using namespace qamd;

static Pack4Stats stats_of(const std::vector<float> &lut, uint32_t m, std::vector<float> &mn, std::vector<float> &mx) {
    Pack4Stats s;
    mn.assign(m, 0.0f), mx.assign(m, 0.0f);
    for (uint32_t c = 0; c < m; c++) {
        bool finite = true;
        mn[c] = mx[c] = lut[(size_t)c * 256];
        for (uint32_t k = 0; k < 256; k++) {
            const float v = lut[(size_t)c * 256 + k];
            finite = finite && std::isfinite(v);
            mn[c] = v < mn[c] ? v : mn[c];
            mx[c] = v > mx[c] ? v : mx[c];
        }
        pack4_add_chunk(s, mn[c], mx[c], finite);
    }
    return s;
}

int main() {
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    std::normal_distribution<float> nrm(0.0f, 1.0f);
    const uint32_t n_rows = 4000;
    int failures = 0;
    std::vector<float> mn, mx, score(n_rows);
    for (uint32_t m : {16u, 96u, 128u}) {
        std::vector<uint8_t> rows((size_t)n_rows * m);
        for (auto &b : rows) b = (uint8_t)(rng() & 255u);
        std::vector<float> lut((size_t)m * 256);
        for (int trial = 0; trial < 24; trial++) {
            const int kind = trial % 4;  // 0: [0, 1); 1: mixed signs; 2: chunk scales 2^-20 .. 2^20; 3: the same on a large offset
            for (uint32_t c = 0; c < m; c++) {
                const float scale = kind >= 2 ? std::ldexp(1.0f, (int)(rng() % 41) - 20) : 1.0f, offset = kind == 3 ? 1.0e6f * nrm(rng) : 0.0f;
                for (uint32_t k = 0; k < 256; k++) lut[(size_t)c * 256 + k] = kind == 0 ? uni(rng) : offset + scale * nrm(rng);
            }
            const Pack4Stats st = stats_of(lut, m, mn, mx);
            for (uint32_t r = 0; r < n_rows; r++) {
                float l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (uint32_t c = 0; c < m; c++) l[c & 3] += lut[(size_t)c * 256 + rows[(size_t)r * m + c]];
                score[r] = (l[0] + l[2]) + (l[1] + l[3]);
            }
            for (int largest = 0; largest < 2; largest++) {
                const Pack4Query p = pack4_params(st, m, largest);
                if (p.bad != 0.0) failures++, std::printf("m=%u kind=%d: a finite table with a range was flagged\n", m, kind);
                std::vector<uint32_t> sum(n_rows, 0);
                for (uint32_t r = 0; r < n_rows; r++)
                    for (uint32_t c = 0; c < m; c++)
                        sum[r] += pack4_entry(lut[(size_t)c * 256 + rows[(size_t)r * m + c]], mn[c], mx[c], p.step, largest);
                for (int pv = 0; pv < 8; pv++) {
                    const float pivot = score[rng() % n_rows];
                    const uint32_t thr = pack4_threshold(p, pivot, largest);
                    for (uint32_t r = 0; r < n_rows; r++)
                        if ((largest ? score[r] >= pivot : score[r] <= pivot) && sum[r] < thr && failures++ < 10)
                            std::printf("VIOLATED m=%u kind=%d largest=%d row %u: sum %u threshold %u\n", m, kind, largest, r, sum[r], thr);
                }
            }
        }
        lut.assign((size_t)m * 256, 0.0f);  // what cannot be bounded: a constant table (step 0), a pivot that is not finite, an infinite entry
        failures += pack4_threshold(pack4_params(stats_of(lut, m, mn, mx), m, 1), 0.0f, 1) != kPack4Never;
        lut[77] = 1.0f;
        const Pack4Query fine = pack4_params(stats_of(lut, m, mn, mx), m, 0);
        failures += fine.bad != 0.0 || pack4_threshold(fine, INFINITY, 0) != kPack4Never || pack4_threshold(fine, NAN, 0) != kPack4Never;
        lut[5] = INFINITY;
        failures += pack4_params(stats_of(lut, m, mn, mx), m, 1).bad == 0.0;
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
