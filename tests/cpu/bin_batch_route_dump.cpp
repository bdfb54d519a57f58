// Prints what bin_batch_route() returns over a grid of stores, batches and developer switches, as change points along
// n_queries (for every key, one line per first n_queries in 1 .. 9000 at which any printed field differs from the line
// before; keys with the same change lines are listed together above one copy of them, as in u8_gemm_route_dump.cpp),
// and then batch_sample_plan() over a grid of store sizes, batch sizes and k.  tests/test_bin_batch_route.py builds this
// with g++ alone and compares the output byte for byte with tests/golden/bin_batch_route_table.txt, which was generated
// from the predicates and the sample arithmetic bin.hip and u8_batch.hip had before the route and the plan were one
// function each: any difference is a change of which kernel serves a batch, of its launch shape, of its candidate lists
// or of its pivot sample.
//
// Grid line:   == grid (product, or the developer switch set)
// Key lines:   @ a list of ds (row bytes)
//              | every code_bits/count/qbits/k at which those row lengths have the change lines below
// Change line: n_queries, then "-" (the per-query routes) or
//              score_batch:  kernel mi
//              topk_batch:   kernel mi  rs4 passes/per pass/NS/waves (or -)  qs4 IT/JT/rows (or -)  n_lists  per-wave queries (Q: the batch)
// Kernels: rs rs4 qs4 (bin_gemm_<name>_kernel).
// Plan line:   plan n Q k: want s_min S target r rows_all
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../quantization_amd/csrc/batch_plan.hpp"
#include "../../quantization_amd/csrc/bin_batch_route.hpp"

namespace {

struct Key {
    uint64_t ds, code_bits, count, n_queries;
    uint32_t qbits, k;
};
constexpr uint32_t kWavesPerLaunch = 2048;  // 256 CUs

struct Fields {
    bool mfma = false;
    std::string kernel;
    int mi = 0;
    bool rs4 = false, qs4 = false;
    uint32_t rs4_passes = 0, rs4_per_pass = 0;
    int rs4_ns = 0, rs4_waves = 0;
    int it = 0, jt = 0;
    uint32_t rows = 0;
    uint32_t n_lists = 0;
    uint64_t per_wave_queries = 0;
};
struct PlanFields {
    double want, s_min, target;
    uint32_t S, r, rows_all;
};

// ---- evaluation: the one part that knows the code under test
Fields evaluate(const Key &key, const BinBatchSwitches &sw) {
    BinBatchInputs in;
    in.ds = key.ds;
    in.code_bits = key.code_bits;
    in.count = key.count;
    in.n_queries = key.n_queries;
    in.qbits = key.qbits;
    in.k = key.k;
    in.waves_per_launch = kWavesPerLaunch;
    const BinBatchRoute r = bin_batch_route(in, sw);
    Fields f;
    f.mfma = r.mfma;
    if (!r.mfma) return f;
    f.kernel = r.name;
    f.mi = r.mi;
    f.rs4 = r.kernel == BinBatchKernel::Rs4;
    f.qs4 = r.kernel == BinBatchKernel::Qs4;
    f.rs4_passes = r.rs4_passes;
    f.rs4_per_pass = r.rs4_per_pass;
    f.rs4_ns = r.rs4_ns;
    f.rs4_waves = r.rs4_waves;
    f.it = r.qs4_it;
    f.jt = r.qs4_jt;
    f.rows = r.qs4_rows;
    f.n_lists = r.n_lists;
    f.per_wave_queries = r.per_wave_queries;
    return f;
}
PlanFields evaluate_plan(uint64_t n, uint64_t Q, uint32_t k) {
    const qamd::BatchSamplePlan p = qamd::batch_sample_plan(n, Q, k);
    return {p.want, p.s_min, p.target, p.S, p.r, p.rows_all};
}
// ---- end of evaluation

std::string format(const Key &key, const Fields &f) {
    if (!f.mfma) return "-";
    std::string k = f.kernel;  // bin_gemm_rs4_kernel -> rs4
    k = k.substr(0, k.size() - strlen("_kernel")).substr(strlen("bin_gemm_"));
    char buf[200];
    int n = snprintf(buf, sizeof buf, "%s %d", k.c_str(), f.mi);
    if (key.k == 0) return buf;
    if (f.rs4) n += snprintf(buf + n, sizeof buf - n, " %u/%u/%d/%d", f.rs4_passes, f.rs4_per_pass, f.rs4_ns, f.rs4_waves);
    else n += snprintf(buf + n, sizeof buf - n, " -");
    if (f.qs4) n += snprintf(buf + n, sizeof buf - n, " %d/%d/%u", f.it, f.jt, f.rows);
    else n += snprintf(buf + n, sizeof buf - n, " -");
    // (the per-wave queries are min(n_queries, a tile or a slice): "Q" while they are the batch itself, so that they do
    // not make every batch size a change point)
    if (f.per_wave_queries == key.n_queries) snprintf(buf + n, sizeof buf - n, " %u Q", f.n_lists);
    else snprintf(buf + n, sizeof buf - n, " %u %llu", f.n_lists, (unsigned long long)f.per_wave_queries);
    return buf;
}

// The keys of the current grid by their change lines, in the order the change lines were first seen.
struct Group {
    std::string changes;
    std::vector<std::string> prefixes;  // "code_bits/count/qbits/k", in the order first seen
    std::vector<std::string> ds_of;     // per prefix: its row lengths
};
std::string g_grid;
std::vector<Group> g_groups;
std::map<std::string, size_t> g_group_of;

void flush() {
    if (!g_groups.empty()) printf("== %s\n", g_grid.c_str());
    for (const Group &g : g_groups) {
        std::vector<bool> done(g.prefixes.size(), false);
        for (size_t i = 0; i < g.prefixes.size(); i++) {
            if (done[i]) continue;
            printf("@%s", g.ds_of[i].c_str());
            int on_line = 0;
            for (size_t j = i; j < g.prefixes.size(); j++) {
                if (g.ds_of[j] != g.ds_of[i]) continue;
                printf("%s%s", on_line++ % 8 == 0 ? "\n|" : "", (" " + g.prefixes[j]).c_str());
                done[j] = true;
            }
            printf("\n");
        }
        fputs(g.changes.c_str(), stdout);
    }
    g_groups.clear();
    g_group_of.clear();
}

struct Row {
    uint64_t ds, code_bits;
};

void sweep(const char *grid, const BinBatchSwitches &sw, const std::vector<Row> &rows) {
    if (g_grid != grid) flush();
    g_grid = grid;
    for (uint64_t count : {4095ull, 4096ull, 32767ull, 32768ull})
        for (uint32_t qbits : {1u, 4u, 8u})
            for (uint32_t k : {0u, 30u, 1024u, 1025u})
                for (const Row &row : rows) {
                    std::string last, changes;
                    for (uint64_t nq = 1; nq <= 9000; nq++) {
                        const Key key{row.ds, row.code_bits, count, nq, qbits, k};
                        const std::string now = format(key, evaluate(key, sw));
                        if (now == last) continue;
                        changes += "  " + std::to_string(nq) + " " + now + "\n";
                        last = now;
                    }
                    auto at = g_group_of.find(changes);
                    if (at == g_group_of.end()) {
                        at = g_group_of.emplace(changes, g_groups.size()).first;
                        g_groups.push_back({changes, {}, {}});
                    }
                    Group &g = g_groups[at->second];
                    const std::string prefix = (row.code_bits == row.ds * 8 ? std::string("all") : std::to_string(row.code_bits)) + "/" +
                                               std::to_string(count) + "/" + std::to_string(qbits) + "/" + std::to_string(k);
                    size_t i = 0;
                    while (i < g.prefixes.size() && g.prefixes[i] != prefix) i++;
                    if (i == g.prefixes.size()) {
                        g.prefixes.push_back(prefix);
                        g.ds_of.emplace_back();
                    }
                    g.ds_of[i] += " " + std::to_string(row.ds);
                }
}

}  // namespace

int main() {
    // every row length of whole 16-byte pieces up to the 64-piece limit (the four fp4 lengths, the 39-block LDS limit
    // at 624 and one beyond among them), 8-byte rows, and 16-byte rows of 63 and 64 code bits
    std::vector<Row> rows = {{8, 64}, {16, 63}, {16, 64}};
    for (uint64_t ds = 16; ds <= 1024; ds += 16) rows.push_back({ds, ds * 8});
    // the product: every switch at its default
    sweep("product", {}, rows);

    // one developer switch at a time
    const std::vector<Row> few = {{64, 512}, {96, 768}, {128, 1024}, {192, 1536}, {256, 2048}, {624, 4992}};
    {
        BinBatchSwitches sw;
        sw.fp4 = false;
        sweep("QAMD_BIN4=0", sw, few);
    }
    {
        BinBatchSwitches sw;
        sw.fp4_min = {true, 40};
        sw.rs4 = false;
        sweep("QAMD_BIN4_MIN=40,QAMD_BIN_RS4=0", sw, few);
    }
    {
        BinBatchSwitches sw;
        sw.rs4 = false;
        sweep("QAMD_BIN_RS4=0", sw, few);
    }
    {
        BinBatchSwitches sw;
        sw.rs4_passes = {true, 1};
        sweep("QAMD_BIN_RS4_PASSES=1", sw, few);
    }
    {
        BinBatchSwitches sw;
        sw.mfma_min = {true, 2};
        sweep("QAMD_BIN_MFMA_MIN=2", sw, few);
    }
    {
        BinBatchSwitches sw;
        sw.scalar_mfma_min = 3;
        sweep("QAMD_BIN_SCALAR_MFMA_MIN=3", sw, few);
    }
    flush();

    printf("== sample plan\n");
    for (uint64_t n : {32768ull, 100003ull, (1ull << 20) - 1, 1ull << 20, 10000000ull, 50000000ull, (1ull << 32) - 1})
        for (uint64_t Q : {1ull, 128ull, 129ull, 1024ull, 8192ull})
            for (uint32_t k : {1u, 30u, 64u, 65u, 342u, 1024u}) {
                const PlanFields p = evaluate_plan(n, Q, k);
                printf("plan %llu %llu %u: %.17g %.17g %u %.17g %u %u\n", (unsigned long long)n, (unsigned long long)Q, k, p.want, p.s_min,
                       p.S, p.target, p.r, p.rows_all);
            }
    return 0;
}
