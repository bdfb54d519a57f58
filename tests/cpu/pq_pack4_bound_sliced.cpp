// The packed filter bound (csrc/pq_pack4.hpp) for rows of 160 .. 256 chunks, which pq_scan_pack4_kernel<SLICED> sums slice by
// slice (128 + 32, 96 + 96, 128 + 96, 128 + 128): no row whose f32 score - lane sums of chunks k, k + 4, ..., then
// (l0 + l2) + (l1 + l3) - reaches the pivot may have per-slice integer sums that add up to less than the threshold, and the
// largest sum a row can reach fits a 16-bit field.  Tables with mixed signs and chunk scales 2^-20 .. 2^20, both directions,
// pivots that are rows' scores.  Exits 1 when a bound is violated.
#include <cstdio>
#include <random>
#include <vector>
#include "../../quantization_amd/csrc/pq_pack4.hpp"
using namespace qamd;

int main() {
    std::mt19937_64 rng(20240917);
    std::normal_distribution<float> nrm(0.0f, 1.0f);
    const uint32_t n_rows = 3000;
    int failures = 0;
    std::vector<float> score(n_rows);
    for (uint32_t m : {160u, 192u, 224u, 256u}) {
        const uint32_t first = (m % 96 == 0) ? 96u : 128u;  // chunks of the first slice
        std::vector<uint8_t> rows((size_t)n_rows * m);
        for (auto &b : rows) b = (uint8_t)(rng() & 255u);
        std::vector<float> lut((size_t)m * 256), mn(m), mx(m);
        for (int trial = 0; trial < 8; trial++) {
            Pack4Stats st;
            for (uint32_t c = 0; c < m; c++) {
                const float scale = trial % 2 ? std::ldexp(1.0f, (int)(rng() % 41) - 20) : 1.0f;
                for (uint32_t k = 0; k < 256; k++) lut[(size_t)c * 256 + k] = scale * nrm(rng);
                mn[c] = mx[c] = lut[(size_t)c * 256];
                for (uint32_t k = 1; k < 256; k++) {
                    mn[c] = std::fmin(mn[c], lut[(size_t)c * 256 + k]);
                    mx[c] = std::fmax(mx[c], lut[(size_t)c * 256 + k]);
                }
                pack4_add_chunk(st, mn[c], mx[c], true);
            }
            for (uint32_t r = 0; r < n_rows; r++) {
                float l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (uint32_t c = 0; c < m; c++) l[c & 3] += lut[(size_t)c * 256 + rows[(size_t)r * m + c]];
                score[r] = (l[0] + l[2]) + (l[1] + l[3]);
            }
            for (int largest = 0; largest < 2; largest++) {
                const Pack4Query p = pack4_params(st, m, largest);
                failures += p.bad != 0.0;
                uint32_t reach = 0;  // the largest sum any row could have
                for (uint32_t c = 0; c < m; c++) reach += pack4_entry(largest ? mx[c] : mn[c], mn[c], mx[c], p.step, largest);
                if (reach > 65535u) failures++, std::printf("m=%u: a row can reach %u, past 16 bits\n", m, reach);
                std::vector<uint32_t> sum(n_rows);
                for (uint32_t r = 0; r < n_rows; r++) {
                    uint32_t slice[2] = {0, 0};
                    for (uint32_t c = 0; c < m; c++)
                        slice[c >= first] += pack4_entry(lut[(size_t)c * 256 + rows[(size_t)r * m + c]], mn[c], mx[c], p.step, largest);
                    sum[r] = slice[0] + slice[1];
                }
                for (int pv = 0; pv < 8; pv++) {
                    const float pivot = score[rng() % n_rows];
                    const uint32_t thr = pack4_threshold(p, pivot, largest);
                    for (uint32_t r = 0; r < n_rows; r++)
                        if ((largest ? score[r] >= pivot : score[r] <= pivot) && sum[r] < thr && failures++ < 10)
                            std::printf("VIOLATED m=%u trial=%d largest=%d row %u: sum %u threshold %u\n", m, trial, largest, r, sum[r], thr);
                }
            }
        }
    }
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
