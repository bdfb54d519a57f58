// Whether the matrix cores serve a batch of binary (or 4- / 8-bit scalar) queries, with which kernel and in what shape:
// decided here, once per call, by a pure function of plain numbers.  bin.hip fills BinBatchInputs, calls
// bin_batch_route() and reads the answer wherever it used to re-derive it: qamd_bin_batch_kernel (the name),
// qamd_bin_score_batch and qamd_bin_topk_batch (the gate), the matrix pass (the launch shapes, the candidate lists).
// Host only, plain C++17: no HIP header, no device query, no environment read, so tests/cpu/bin_batch_route_dump.cpp
// prints the whole table with g++ alone (tests/golden/bin_batch_route_table.txt).
//
// Everything has internal linkage: the header belongs to the one translation unit that launches these kernels (and to
// the dump program).
#pragma once
#include <algorithm>
#include <cstdint>

namespace {

enum class BinBatchKernel { None /* the per-query routes of bin.hip */, Rs, Rs4, Qs4 };

inline const char *bin_batch_kernel_name(BinBatchKernel k) {
    switch (k) {
        case BinBatchKernel::Rs: return "bin_gemm_rs_kernel";
        case BinBatchKernel::Rs4: return "bin_gemm_rs4_kernel";
        case BinBatchKernel::Qs4: return "bin_gemm_qs4_kernel";
        default: return nullptr;
    }
}

struct BinBatchInputs {
    uint64_t ds = 0;         // device stride of a row, bytes
    uint64_t code_bits = 0;  // bits of a row that carry code
    uint64_t count = 0;      // rows of the store
    uint64_t n_queries = 0;
    uint32_t qbits = 1;  // 1: binary queries; 4 / 8: scalar queries
    uint32_t k = 0;      // 0: score_batch, else topk_batch(k)
    uint32_t waves_per_launch = 0;  // waves (= candidate lists) of one launch of a persistent 8-wave-per-CU kernel
};

// Developer A/B switches (tools/lib build only; the product library leaves every one at its default).
struct BinBatchSwitches {
    struct Number {
        bool set = false;
        uint64_t value = 0;
    };
    bool fp4 = true;            // QAMD_BIN4=0: without the FP4 forms
    Number fp4_min;             // QAMD_BIN4_MIN: the smallest batch of the query-streaming fp4 form
    bool rs4 = true;            // QAMD_BIN_RS4=0: without the row-streaming fp4 form
    Number rs4_passes;          // QAMD_BIN_RS4_PASSES: the most passes the row-streaming form may take
    Number mfma_min;            // QAMD_BIN_MFMA_MIN: the smallest binary batch whose top-k the matrix cores take
    uint64_t scalar_mfma_min = 0;  // QAMD_BIN_SCALAR_MFMA_MIN: the smallest scalar batch they take, 0: the default
};

struct BinBatchRoute {
    bool mfma = false;  // the matrix cores take the call (else: the per-query routes)
    BinBatchKernel kernel = BinBatchKernel::None;  // score_batch: the kernel; topk_batch: the FILTER (the sample pass is Rs)
    const char *name = nullptr;
    int mi = 0;  // query fragments (of 32 queries) per tile of bin_gemm_rs_kernel: the score or sample pass, the Rs filter
    // Rs4: so many passes over the rows, the queries spread evenly (whole tile pairs); <NS> and the waves of a workgroup
    uint32_t rs4_passes = 0, rs4_per_pass = 0;
    int rs4_ns = 0, rs4_waves = 0;
    // Qs4 <IT, JT>, rows of a block in LDS
    int qs4_it = 0, qs4_jt = 0;
    uint32_t qs4_rows = 0;
    // topk_batch: wave-private candidate lists of the whole call, and the queries that `per_wave` (the expected appends
    // to one list) counts: those of one launch
    uint32_t n_lists = 0;
    uint64_t per_wave_queries = 0;
};

// Rows the filtering scans and the matrix cores take: whole 16-byte pieces, at most 64 of them.
inline bool bin_fused_rows(uint64_t ds) { return ds % 16 == 0 && ds / 16 <= 64; }

// Query fragments per workgroup tile that fit in LDS for this row length (0: none).
inline int bin_mfma_frags(uint64_t ds, uint64_t n_queries = ~0ull) {
    const uint64_t nkb = ds / 16;
    if (n_queries > 32 && (size_t)64 * (nkb * 128 + 16) + 2048 <= 160 * 1024) return 2;
    if ((size_t)32 * (nkb * 128 + 16) + 2048 <= 160 * 1024) return 1;
    return 0;
}

// Rows of 512 / 768 / 1024 / 1536 bits: the lengths the FP4 kernels are instantiated for.
inline bool bin_fp4_rows(uint64_t ds) { return ds == 64 || ds == 96 || ds == 128 || ds == 192; }

constexpr uint64_t kQs4Slice = 2048, kQs4MinQueries = 129;  // queries per launch of bin_gemm_qs4_kernel; from where it is used
constexpr uint32_t kRs4MinQueries = 12;  // (the int8 matrix-core form; the fp4 form takes 3 and 5+ queries)
constexpr uint32_t kRs4MaxPasses = 4;  // (measured: profiles/r04_bin_batch.txt; four passes tie with the query-streaming form)
inline uint32_t rs4_max_queries(uint64_t ds) {  // whole 32-query tile pairs whose nibble image + bounds fit the CU's LDS
    return (uint32_t)((160 * 1024 - 1024) / (ds * 4 + 4) / 32 * 32);
}
// Waves per workgroup: 12 (three per SIMD: 166 registers at NS = 8) where the registers allow, else 8 - a third wave covers
// more of the other two's vector-ALU phases with MFMAs.
constexpr int rs4_waves(int ns) { return ns <= 8 ? 12 : 8; }

inline BinBatchRoute bin_batch_route(const BinBatchInputs &in, const BinBatchSwitches &sw) {
    BinBatchRoute r;
    const uint64_t Q = in.n_queries;
    // The matrix gate: the query tile must fit LDS (bin_mfma_frags != 0: rows of at most 39 K-blocks = 4992 bits), and at
    // that length every operand and partial sum of the f32 epilogue is an integer below 2^23 - binary: 4 * 4992 + 2 * 4992;
    // scalar: 512 dim + 255 dim + 2 dim = 769 * 4992 < 2^22 - so the scores are those of the scan kernels bit for bit.
    const bool capable = bin_fused_rows(in.ds) && bin_mfma_frags(in.ds) != 0 && in.code_bits >= 64;
    // The smallest scalar batch the matrix cores take: the values of the binary int8 route, 5 for score_batch and
    // kRs4MinQueries = 12 for topk_batch.  Measured (profiles/bin_scalar_batch.txt, 50M x 1024, 4 / 8 bits, batch against a loop
    // of single-query calls on the same handle; min-max within 5 % of every median): score_batch of 8 queries 2.15 / 2.24 ms
    // against 8.46 / 9.76 (3.9 x / 4.4 x), 32 queries 12.5 x / 14.1 x, 64 queries 16.5 x / 18.4 x; topk_batch(30) of 32 queries
    // 2.28 / 2.41 ms against 31.0 / 37.6 (13.6 x / 15.6 x), 64 queries 13.7 x / 16.2 x; 8 queries are under the topk gate and
    // tie with the loop (1.01 x).  A tile costs about 2.2 ms at 50M rows whatever its fill and one scalar scan 1.0 - 1.2 ms, so
    // the crossover is probably near 3 queries for both calls; batches of 2 .. 7 were not timed, so the gates stay at the
    // smallest sizes the table supports.  QAMD_BIN_SCALAR_MFMA_MIN: developer A/B, next to QAMD_BIN_MFMA_MIN.
    auto scalar_mfma_min = [&](uint64_t dflt) { return sw.scalar_mfma_min ? sw.scalar_mfma_min : dflt; };

    if (in.k == 0) {  // score_batch: tiles of 32 / 64 queries of bin_gemm_rs_kernel
        const uint64_t least = in.qbits == 1 ? 5 : scalar_mfma_min(5);
        r.mfma = Q >= least && in.count >= 4096 && capable;
        if (!r.mfma) return r;
        r.kernel = BinBatchKernel::Rs;
        r.name = bin_batch_kernel_name(r.kernel);
        r.mi = bin_mfma_frags(in.ds, Q);
        return r;
    }

    bool enough;
    if (in.qbits != 1) {
        enough = Q >= scalar_mfma_min(kRs4MinQueries);
    } else {
        // rows of 512 / 768 / 1024 / 1536 bits: a pass of the row-streaming fp4 kernel costs 1.4-1.5 ms per 50M x 1024 whatever the batch,
        // the vector-ALU scan 1.04 / 1.98 / 1.26 / 2.2 / 1.8 / 3.7 ms at 2 / 3 / 4 / 5 / 8 / 11 queries (profiles/r04_bin_batch.txt)
        enough = sw.mfma_min.set ? Q >= sw.mfma_min.value : (bin_fp4_rows(in.ds) ? (Q == 3 || Q >= 5) : Q >= kRs4MinQueries);
    }
    r.mfma = enough && in.count >= 32768 && in.k <= 1024 && capable;
    if (!r.mfma) return r;

    // Which filter the matrix-core top-k runs.  Scalar batches take the int8 kernel only - centred codes are not exact in
    // E2M1 - and on 32-query tiles: the 64-query filter forms are not instantiated for codes (launch_bin_rs).
    r.mi = in.qbits != 1 ? 1 : bin_mfma_frags(in.ds, Q);
    bool rs4 = false, fp4 = false;
    if (in.qbits == 1) {
        // rows of 512 / 1024 / 2048 bits, enough queries: the FP4 query-streaming form
        const bool fp4_shape = bin_fp4_rows(in.ds) && sw.fp4;
        // the whole batch's nibble image in LDS: the row-streaming fp4 form (one pass, no barriers); larger batches: query-streaming
        // A batch of up to kRs4MaxPasses LDS images goes through that form in as many passes over the rows, the queries spread evenly
        // (50M x 1024 bits: 289 queries = two passes of 160: 6.4 ms against the query-streaming form's 10.1; 576 = 2 x 288: 10.4 / 15.7)
        const uint32_t rs4_cap = rs4_max_queries(in.ds), rs4_most = sw.rs4_passes.set ? (uint32_t)sw.rs4_passes.value : kRs4MaxPasses;
        r.rs4_passes = rs4_cap ? (uint32_t)(((Q + 31) / 32 * 32 + rs4_cap - 1) / rs4_cap) : 0u;
        rs4 = fp4_shape && sw.rs4 && r.rs4_passes >= 1 && r.rs4_passes <= rs4_most;
        r.rs4_per_pass = rs4 ? (uint32_t)(((Q + r.rs4_passes - 1) / r.rs4_passes + 31) / 32 * 32) : 0u;  // queries per pass (whole tile pairs)
        fp4 = rs4 || (fp4_shape && Q >= (sw.fp4_min.set ? sw.fp4_min.value : kQs4MinQueries));
    }
    if (!rs4) r.rs4_passes = 0;
    r.kernel = rs4 ? BinBatchKernel::Rs4 : fp4 ? BinBatchKernel::Qs4 : BinBatchKernel::Rs;
    r.name = bin_batch_kernel_name(r.kernel);
    if (rs4) {
        r.rs4_ns = (int)(in.ds / 16);
        r.rs4_waves = rs4_waves(r.rs4_ns);
    } else if (fp4) {
        r.qs4_it = Q <= 128 ? 1 : Q <= 256 ? 2 : 4;
        r.qs4_jt = in.ds > 128 ? 6 : 8;
        r.qs4_rows = in.ds > 128 ? 96 : 128;
    }
    // One candidate list per wave of a launch: Rs4 a launch per pass, Qs4 a launch per slice, Rs one launch at a time (every
    // tile's lists are scattered before the next tile runs).
    r.n_lists = rs4 ? r.rs4_passes * (in.waves_per_launch / 8 * (uint32_t)r.rs4_waves)
                    : in.waves_per_launch * (fp4 ? (uint32_t)((Q + kQs4Slice - 1) / kQs4Slice) : 1u);
    r.per_wave_queries = std::min<uint64_t>(Q, fp4 ? kQs4Slice : 32u * (uint32_t)r.mi);
    return r;
}

}  // namespace
