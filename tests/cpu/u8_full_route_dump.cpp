// u8_full_route() of one full-range batch: argv = pass (0 score, 1 sample, 2 filter), rows, actual_dim, multiplier (strtof),
// n_queries, multi_width; prints by_scans, wave_lists, sample_block_rows, slice_queries (tests/test_u8_full_filter_route.py).
#include <cstdio>
#include <cstdlib>

#include "../../quantization_amd/csrc/u8_gemm_route.hpp"

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    U8GemmInputs in;
    in.full_range = true;
    in.pass = (U8GemmPass)atoi(argv[1]);
    in.rows = strtoull(argv[2], nullptr, 10), in.actual_dim = strtoull(argv[3], nullptr, 10), in.multiplier = strtof(argv[4], nullptr);
    in.n_queries = strtoull(argv[5], nullptr, 10), in.multi_width = (uint32_t)atoi(argv[6]);
    const U8GemmRoute r = u8_gemm_route(in, U8GemmSwitches{});
    printf("%d %d %u %llu\n", (int)r.by_scans, (int)r.wave_lists, r.sample_block_rows, (unsigned long long)r.slice_queries);
    return 0;
}
