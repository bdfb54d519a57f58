// Prints the kernel u8_gemm_route() gives the FILTER pass of topk_batch over a whole store on a 256-CU device, one word
// per argument "actual_dim:rows:multiplier:n_queries" (multiplier: a float, or "inf").  tests/test_topk_order_model.py
// builds it with g++ alone and checks that the u8 batch shapes of tests/test_gpu_topk_special_scores.py reach the
// kernel families they are named after.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../quantization_amd/csrc/u8_gemm_route.hpp"

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        unsigned long long ad = 0, rows = 0, nq = 0;
        char mult[32] = {0};
        if (sscanf(argv[a], "%llu:%llu:%31[^:]:%llu", &ad, &rows, mult, &nq) != 4) return 2;
        U8GemmInputs in;
        in.actual_dim = ad;
        in.rows = rows;
        in.multiplier = strcmp(mult, "inf") == 0 ? std::numeric_limits<float>::infinity() : (float)atof(mult);
        in.n_queries = nq;
        in.q_pad = (nq + 255) / 256 * 256;  // what qamd_u8_encode_query_batch pads to
        const uint32_t nkb = (uint32_t)((ad + 127) / 128);
        in.frag_nkb = nkb <= 12 ? nkb : 0;  // ... and the rows it makes a fragment copy for
        in.cu_count = 256;
        in.pass = U8GemmPass::Filter;
        in.whole_store = true;
        printf("%s\n", u8_gemm_route(in, U8GemmSwitches{}).name);
    }
    return 0;
}
