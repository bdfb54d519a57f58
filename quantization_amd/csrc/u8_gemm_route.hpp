// Which matrix-core kernel serves a batch of u8 queries, and in what shape: decided here, once per pass, by a pure
// function of plain numbers.  u8_batch.hip fills the two structs, calls u8_gemm_route() and reads the answer everywhere
// it used to re-derive it: the launcher (kernel and template shape), the sample pass (block bests or the full score
// matrix), the wave-private candidate lists (whether they exist, how many), the debug line, and the places that weigh
// the VALU scans against the GEMM.  Host only, plain C++17: no HIP header, no device query, no environment read, so
// tests/cpu/u8_gemm_route_dump.cpp prints the whole table with g++ alone (tests/golden/u8_gemm_route_table.txt).
//
// Everything has internal linkage: the header belongs to the one translation unit that launches these kernels (and to
// the dump program), and RqGeometry is a kernel parameter there.
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>

namespace {

enum class U8GemmPass {
    Score,   // every score out (MODE 0): qamd_u8_score_batch
    Sample,  // the pivot sample of topk_batch: MODE 3 (block bests) where the filter pass takes a query-streaming form, else MODE 0
    Filter,  // the filter pass of topk_batch (MODE 1 / 2)
};

enum class U8GemmKernel { Gemm, Pp, Rs, Qs16, Qr16, Rq16, Rk16 };

inline const char *u8_gemm_kernel_name(U8GemmKernel k) {
    switch (k) {
        case U8GemmKernel::Pp: return "u8_gemm_pp_kernel";
        case U8GemmKernel::Rs: return "u8_gemm_rs_kernel";
        case U8GemmKernel::Qs16: return "u8_gemm_qs16_kernel";
        case U8GemmKernel::Qr16: return "u8_gemm_qr16_kernel";
        case U8GemmKernel::Rq16: return "u8_gemm_rq16_kernel";
        case U8GemmKernel::Rk16: return "u8_gemm_rk16_kernel";
        default: return "u8_gemm_kernel";
    }
}

struct U8GemmInputs {
    uint64_t actual_dim = 0;  // code bytes per row (a multiple of 16)
    uint64_t rows = 0;        // rows of the store (not of the sample)
    float multiplier = 0.0f;
    uint64_t n_queries = 0;
    uint64_t q_pad = 0;     // queries the batch is padded to
    uint32_t frag_nkb = 0;  // 128-byte K-blocks per query of the batch's fragment copy, 0: it has none
    int cu_count = 0;
    U8GemmPass pass = U8GemmPass::Score;
    bool whole_store = true;  // the pass runs over the store itself, not over a gathered sample of it
};

// Developer A/B switches (tools/lib build only; the product library leaves every one at its default).
struct U8GemmSwitches {
    struct Number {
        bool set = false;
        uint64_t value = 0;
    };
    bool forced = false;  // QAMD_GEMM_CFG is set: only the family `family` may run, wherever it can
    char family = 0;      // r row-streaming, q query-streaming, g queries in registers, s resident queries, p ping-pong, else u8_gemm_kernel
    bool rq = true;       // QAMD_RQ=0: without the resident-queries kernels
    bool rq_k = true;     // QAMD_RQ_K=0: the tile-outer form (rq16) on 768-byte rows as well
    Number rq_groups;     // QAMD_RQ_GROUPS
    Number qr_min, qr_max, rq_min, rq_max;  // QAMD_QR_MIN / _MAX, QAMD_RQ_MIN / _MAX: the batch sizes of those kernels
};

struct RqGeometry {
    uint32_t groups, pairs_lo /* tile pairs of every group */, pairs_extra /* the first so many groups take one more */,
        streams_per_xcd, n_tiles /* of the batch, even */;
};

struct U8GemmRoute {
    U8GemmKernel kernel = U8GemmKernel::Gemm;
    const char *name = "u8_gemm_kernel";
    // the template shape of `kernel` (the others stay 0)
    int tile = 0;          // Gemm: 128 = <128,128,2,2,128>, 256 = <256,256,2,4,128>
    int mi = 0, mj = 0;    // Pp <MI, MJ>; Rs <MI, NT>
    bool nt = false;       // Rs: one query tile, every row byte is read exactly once
    int jt = 0, it = 0;    // Qs16 <JT, IT>
    int nsteps = 0;        // Qr16, Rq16, Rk16: 64-byte k-steps per row
    int nt_tiles = 0;      // Rk16 <.., NT>
    uint64_t slice_queries = 0;  // queries per launch, 0: the whole batch in one launch
    // Filter pass only
    bool wave_lists = false;     // the kernel appends to wave-private candidate lists
    uint32_t list_launches = 0;  // the lists are sized for so many launches (0 without lists)
    // Sample pass only: the kernel hands back the best score of every block of so many sample rows, 0: the Q x S matrix
    uint32_t sample_block_rows = 0;
    int rs_frags = 0;    // query fragments per workgroup of the row-streaming kernel for this batch (0: no tile fits)
    bool rs_ok = false;  // the row-streaming kernel suits this batch: where the GEMM is preferred to the VALU multi-query scans
    RqGeometry rq{};     // Rq16 / Rk16
};

constexpr uint64_t route_round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }
inline uint32_t route_cus_per_xcd(int cu_count) { return (uint32_t)(cu_count / 8 > 1 ? cu_count / 8 : 1); }

// ---- ping-pong kernel: 128-query tiles up to 128 queries, else 256-query tiles; one launch per cus_per_xcd tiles
inline uint32_t pp_launches(uint64_t n_queries, int cu_count) {
    const uint64_t per = (uint64_t)route_cus_per_xcd(cu_count) * (n_queries <= 128 ? 128 : 256);
    return (uint32_t)((n_queries + per - 1) / per);
}

// ---- row-streaming kernel: query fragments per workgroup (0: the tile does not fit, use another kernel)
inline int rs_frags(uint64_t n_queries, uint64_t ad) {
    const uint64_t lds_max = 160 * 1024;
    for (int mi : {1, 2, 4})  // the smallest tile that holds the whole batch, else the largest that fits
        if (n_queries <= (uint64_t)32 * mi && (uint64_t)32 * mi * (route_round_up(ad, 128) + 16) + 2048 + 32768 <= lds_max) return mi;
    for (int mi : {4, 2, 1})
        if ((uint64_t)32 * mi * (route_round_up(ad, 128) + 16) + 2048 + 32768 <= lds_max) return mi;
    return 0;
}

// ---- query-streaming kernel (u8_gemm_qs16_kernel): slices of kQsSlice queries (the slice's fragment-order codes,
// 1.5 MiB at 768-byte rows, stay in every XCD's L2); up to kQs16SmallBatch queries in chunks of 32, a chunk for every wave.
constexpr uint64_t kQsSlice = 2048;
constexpr uint64_t kQs16SmallBatch = 256;
// Batch size from which the query-streaming kernel is preferred, by 128-byte K-blocks per row (measured, whole
// topk_batch(30) calls at 7.68 GB of rows; below it several 128-query tiles of the row-streaming kernel, or the
// ping-pong kernel where only 64-query tiles fit).  Round 3, with the 16x16x64 form of the kernel for rows of up to
// 1024 bytes (profiles/r03_qs_experiments.txt), ms, row-streaming / query-streaming:
//   rows of 256 B,  30M:   257 q  3.96 / 4.45    385 q  5.10 / 4.73    704 q  7.81 / 6.98    960 q  9.80 / 8.07
//   rows of 384 B,  20M:   257 q  3.64 / 3.69    385 q  4.60 / 3.97    704 q  7.07 / 5.98    960 q  8.96 / 7.16
//   rows of 512 B,  15M:   192 q  2.34 / 2.73    257 q  3.44 / 3.30    385 q  4.35 / 3.70    704 q  6.77 / 5.53
//   rows of 768 B,  10M:   192 q  2.19 / 2.35    257 q  3.24 / 2.88    385 q  4.10 / 3.39    704 q  6.36 / 5.07
//   rows of 1024 B, 7.5M:  192 q  2.22 / 2.21    257 q  3.41 / 2.74    385 q  4.76 / 3.25    704 q  8.61 / 4.89
//   rows <= 1536 B: 12.5M x 1536: 256 q  pp 5.84 qs 6.34; 384 q  pp 10.3 qs 8.8; 640 q  pp 16.1 qs 13.8   (round 2)
// i.e. from the third 128-query tile on (the fourth for rows of up to 384 bytes); the round-2 thresholds (960 / 704)
// dated from before that round's block-change and epilogue work and this round's matrix instruction.  With chunks of 32
// queries for batches of up to 256 (a chunk for every wave) the second tile goes the same way on rows past 768 bytes:
//   rows of 768 B,  10M:   129 q  2.18 / 2.06    192 q  2.2-2.5 / 2.20    256 q  2.31 / 2.49     (kept on row-streaming)
//   rows of 1024 B, 7.5M:  129 q  2.22 / 2.02    192 q  2.26 / 2.11       256 q  2.80 / 2.37
//   rows of 1536 B, 12.5M: 129 q  5.44 / 4.88    192 q  5.53 / 5.23       256 q  6.87 / 5.90
inline uint64_t qs_min_queries(uint32_t nkb) { return nkb <= 3 ? 385 : nkb <= 6 ? 257 : 129; }

// ---- queries in registers, rows through a double-buffered LDS slab (u8_gemm_qr16_kernel): batches cut into passes of
// kQrQueries.  QAMD_GEMM_CFG=g forces it where it can run (developer A/B); QAMD_QR_MIN / QAMD_QR_MAX move its range.
// Measured (profiles/r03_qs_experiments.txt §7), whole topk_batch(30) ms, row-streaming passes / this kernel:
//   10M x 768:    129 q 2.17 / 1.65   192 q 2.21 / 1.75   256 q 2.26 / 1.91     (two passes: 512 q 3.81 against 3.66 query-streaming)
//   7.5M x 1024:   65 q 1.52 / 1.23   129 q 2.18 / 1.55   256 q 2.75 / 1.84
//   15M x 512:    129 q 2.28 / 1.76   256 q 2.41 / 2.08       30M x 256:  129 q 2.68 / 2.44   256 q 2.84 / 2.55
// -> one pass only: 129 .. 256 queries (from 65 on 1024-byte rows, where the row-streaming kernel needs two 64-query tiles).
constexpr uint64_t kQrQueries = 256;

// ---- queries resident, rows streamed (u8_gemm_rq16_kernel, u8_gemm_rk16_kernel): the filter pass of topk_batch for
// batches of kRqMinQueries and more on rows of 256 / 384 / 512 / 768 bytes, in groups of query tiles that run side by
// side on the CUs of an XCD.  QAMD_GEMM_CFG=s forces it where it can run, QAMD_RQ=0 switches it off (developer A/B).
constexpr uint64_t kRqMinQueries = 129;
constexpr uint32_t rq_tile_cap(uint32_t nsteps) { return ((160u * 1024u - 2048u) / (nsteps * 1024u + 64u)) & ~1u; }
inline RqGeometry rq_geometry(uint64_t n_queries, uint32_t nsteps, const U8GemmSwitches::Number &forced_groups = {}) {
    // the fewest groups whose tile pairs fit a CU's LDS, the pairs spread evenly; 32 / G row streams per XCD (QAMD_RQ_GROUPS:
    // developer A/B).  More groups than needed only add L2 -> CU traffic: at 10M x 768, 1024 queries, 6 groups 8.3 ms, 8 groups 8.7.
    RqGeometry g{};
    g.n_tiles = (uint32_t)(route_round_up(n_queries, 32) / 16);
    const uint32_t pairs = g.n_tiles / 2, cap_pairs = rq_tile_cap(nsteps) / 2;
    g.groups = forced_groups.set ? (uint32_t)forced_groups.value : (pairs + cap_pairs - 1) / cap_pairs;
    if (g.groups == 0 || g.groups > 8 || g.groups > pairs || (pairs + g.groups - 1) / g.groups > cap_pairs) {
        g.groups = 0;
        return g;
    }
    g.pairs_lo = pairs / g.groups;
    g.pairs_extra = pairs % g.groups;
    g.streams_per_xcd = 32u / g.groups;
    return g;
}

inline U8GemmRoute u8_gemm_route(const U8GemmInputs &in, const U8GemmSwitches &sw) {
    const uint64_t ad = in.actual_dim, nq = in.n_queries;
    const bool usable_multiplier = std::isfinite(in.multiplier) && in.multiplier != 0.0f;  // the integer pre-filter needs one
    const bool frag = in.frag_nkb != 0;
    const int mi = rs_frags(nq, ad);
    const bool rq_rows = ad == 256 || ad == 384 || ad == 512 || ad == 768;
    const RqGeometry geo = rq_rows ? rq_geometry(nq, (uint32_t)(ad / 64), sw.rq_groups) : RqGeometry{};
    auto only = [&](char family) { return !sw.forced || sw.family == family; };

    // Queries in registers: one pass of 129 .. 256 queries (from 65 on 1024-byte rows).
    auto qr_wanted = [&](bool filter) {
        if (!only('g') || (filter && !usable_multiplier)) return false;
        if (!(frag && (ad == 256 || ad == 384 || ad == 512 || ad == 768 || ad == 1024))) return false;
        if (sw.forced) return true;
        // a store of fewer than ~4 slabs per workgroup (a small Qdrant segment) leaves this persistent grid a ragged tail too:
        // the same guard as qs_wanted (the row-streaming tiles split such a store evenly)
        if (!sw.qr_min.set && !sw.qr_max.set && in.rows < 131072 && ad <= 1152) return false;
        const uint64_t q_min = sw.qr_min.set ? sw.qr_min.value : (ad == 1024 ? 65 : 129);
        const uint64_t q_max = sw.qr_max.set ? sw.qr_max.value : kQrQueries;
        return nq >= q_min && nq <= q_max;
    };
    // Queries resident (filter pass only; its sample pass takes the query-streaming forms).
    auto rq_wanted = [&]() {
        if (!only('s') || !sw.rq || !usable_multiplier || !frag) return false;
        if (!rq_rows) return false;
        if (in.cu_count != 256 || in.q_pad < route_round_up(nq, 32)) return false;  // (8 XCDs of 32 CUs: the group / stream map)
        if (geo.groups == 0) return false;  // (more than eight LDS images)
        if (sw.forced) return true;
        if (in.rows < 131072) return false;  // (a small store: the row-streaming tiles split it evenly)
        if (sw.rq_min.set || sw.rq_max.set)
            return nq >= (sw.rq_min.set ? sw.rq_min.value : kRqMinQueries) && nq <= (sw.rq_max.set ? sw.rq_max.value : ~0ull);
        if (nq < kRqMinQueries) return false;
        // Measured, whole topk_batch(30) ms, before / this kernel (tools/experiments/u8_rq_sweep.sh, profiles/r04_u8_rq.txt):
        //   15M x 512:  129 q 1.95 / 1.49  288 q 3.42 / 2.19 | 289 q 3.40 / 2.64  576 q 5.32 / 4.14 | 768 q 5.84 / 5.48  1152 q 7.91 / 7.61
        //   30M x 256:  129 q 2.75 / 1.60  608 q 7.04 / 4.77 | 609 q 7.05 / 5.10  1216 q 10.6 / 8.89 | 1800 q 14.0 / 12.5  2400 q 19.7 / 16.6
        // 768-byte rows, the K-outer form (u8_gemm_rk16_kernel), before / with it:  129 q 1.64 / 1.49   192 q 1.78 / 1.54 | 193-256 q (two
        // groups) 1.92-2.03 / 2.33-2.38: the queries-in-registers kernel keeps those | 257 q 2.94 / 2.50  288 q 2.99 / 2.51  384 q 3.26 / 2.62 |
        // three groups: 400 q 3.52 / 3.65  512 q 3.83 / 3.91 (no), 576 q 4.80 / 4.00 (past the query-streaming kernel's step at 513) |
        // four: 640 q 5.07 / 4.71  768 q 5.50 / 5.08 | five and more (30 of an XCD's 32 CUs, or half-empty groups): 832 q 5.85 / 6.25,
        // 1024 q in eight groups of eight tiles 6.44 / 6.44
        if (ad == 768)
            return geo.groups == 1 || (geo.groups == 2 && nq > kQrQueries) || (geo.groups == 3 && nq > 512) || geo.groups == 4;
        return geo.groups <= 4;
    };
    // The query-streaming family (qs16, and the two above, which are forms of it): rows short enough for a 128-row block
    // in LDS, a fragment-order copy in the batch, enough queries to keep the 8 waves of a workgroup busy.
    auto qs_wanted = [&](bool filter) {
        if (qr_wanted(filter) || (filter && rq_wanted())) return true;
        if (!only('q') || (filter && !usable_multiplier) || !frag || in.frag_nkb > 12) return false;
        if (sw.forced) return true;
        // a store of fewer than ~4 row blocks per workgroup (a small Qdrant segment) leaves the persistent workgroups a
        // ragged tail; the row-streaming tiles split such a store evenly (100k x 768, 1024 queries: 0.24 against 0.28 ms)
        if (in.rows < 131072 && ad <= 1152) return false;
        return nq >= qs_min_queries(in.frag_nkb);
    };
    // The row-streaming kernel: where the ping-pong kernel could run (same pre-filter conditions), the query tile fits
    // in LDS, and the batch is small enough to be HBM-bound.
    auto rs_wanted = [&](bool filter) {
        if (!only('r') || (filter && !usable_multiplier) || mi == 0 || ad > 32768) return false;
        if (sw.forced) return true;
        // One query tile: every row byte leaves HBM once, at the plain scan's rate.  Several tiles re-read the
        // rows (at HBM pace a line lives ~5 us in the XCD's L2, too short for the tiles' workgroups to share
        // it), which still beats the ping-pong kernel for 128-query tiles up to 768 queries (measured at
        // 10M x 768: 160 q 2.22 vs 2.41 ms, 384 q 3.39 vs 4.51, 512 q 4.29 vs 4.66, 1024 q 8.64 vs 8.70)
        // and loses with the 64-query tiles of longer rows (12.5M x 1536: 96 q 3.88 vs 3.74, 256 q 6.83 vs 5.58).
        const uint64_t tiles = (nq + 32 * mi - 1) / (32 * mi);
        return tiles == 1 || (mi == 4 && !qs_wanted(filter));
    };
    // The ping-pong kernel: rows of at least three 64-byte K-tiles, a usable multiplier for its integer pre-filter.
    auto pp_wanted = [&](bool filter) { return only('p') && ad > 128 && ad <= 32768 && (!filter || usable_multiplier); };

    // The sample pass follows the filter pass into the query-streaming family (block bests, MODE 3); otherwise it is
    // a score pass over the sample (the full matrix, MODE 0), chosen as one: without the filter's multiplier condition.
    const bool block_bests = in.pass == U8GemmPass::Sample && qs_wanted(true);
    const bool filter = in.pass == U8GemmPass::Filter || block_bests;
    const uint32_t cus_per_xcd = route_cus_per_xcd(in.cu_count);

    U8GemmRoute r;
    r.rs_frags = mi;
    r.rs_ok = rs_wanted(filter);
    const bool qs = qs_wanted(filter), rs = !qs && r.rs_ok, pp = !qs && !rs && pp_wanted(filter);
    if (qs && in.pass == U8GemmPass::Filter && in.whole_store && rq_wanted()) {
        r.nsteps = (int)(ad / 64);
        r.rq = geo;
        const uint32_t max_tiles = 2 * (geo.pairs_lo + (geo.pairs_extra ? 1 : 0));
        if (r.nsteps == 12 && sw.rq_k) {  // the K-outer form: all tiles' accumulators in registers
            r.kernel = U8GemmKernel::Rk16;
            r.nt_tiles = max_tiles <= 8 ? 8 : max_tiles <= 10 ? 10 : 12;
        } else {
            r.kernel = U8GemmKernel::Rq16;
        }
    } else if (qs && qr_wanted(filter)) {
        r.kernel = U8GemmKernel::Qr16;
        r.nsteps = in.frag_nkb == 2 ? 4 : in.frag_nkb == 3 ? 6 : in.frag_nkb == 4 ? 8 : in.frag_nkb == 6 ? 12 : 16;
        r.slice_queries = kQrQueries;
    } else if (qs) {
        r.kernel = U8GemmKernel::Qs16;
        r.jt = in.frag_nkb <= 8 ? 8 : 6;  // 128 resident rows of up to 1024 bytes, else 96
        r.it = nq <= kQs16SmallBatch ? 2 : 4;
        r.slice_queries = kQsSlice;
    } else if (rs) {
        r.kernel = U8GemmKernel::Rs;
        r.mi = mi;
        r.nt = nq <= (uint64_t)32 * mi;
        r.slice_queries = (uint64_t)cus_per_xcd * 32 * mi;
    } else if (pp) {
        r.kernel = U8GemmKernel::Pp;
        r.mi = nq <= 128 ? 2 : 4;  // 128-query tile: the store is streamed once, HBM-bound
        r.mj = nq <= 128 ? 4 : 2;
        r.slice_queries = (uint64_t)cus_per_xcd * 64 * r.mi;
    } else {
        r.tile = nq > 128 ? 256 : 128;  // (q_pad is a multiple of 256 and the row padding of every store covers a 256-row tile)
    }
    r.name = u8_gemm_kernel_name(r.kernel);

    if (in.pass == U8GemmPass::Filter && (qs || rs || pp)) {
        r.wave_lists = true;
        // One list per wave of a launch.  The query-streaming branch also counts the resident-queries kernels, which
        // launch ONCE (wave_base 0) whatever the batch: past 2048 queries they get lists that are never written.
        // Kept as it is: wave_cap, and with it how often a list overflows and the batch is redone, depends on it.
        if (qs && qr_wanted(true)) r.list_launches = (uint32_t)((nq + kQrQueries - 1) / kQrQueries);
        else if (qs) r.list_launches = (uint32_t)((nq + kQsSlice - 1) / kQsSlice);
        else if (rs) r.list_launches = (uint32_t)((nq + r.slice_queries - 1) / r.slice_queries);
        else r.list_launches = pp_launches(nq, in.cu_count);
    }
    if (block_bests) r.sample_block_rows = r.kernel == U8GemmKernel::Qr16 ? 64 : r.jt == 8 ? 128 : 96;
    return r;
}

}  // namespace
