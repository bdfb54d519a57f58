// Prints what u8_gemm_route() returns over a grid of stores, devices, passes and developer switches, as change points
// along n_queries: for every key, one line per first n_queries (1 .. 9000) at which any printed field differs from the
// line before.  Most keys share their change lines with others (the sign of the multiplier, the store size below the
// small-store guard, ... do not matter to them), so within a grid the keys with the same change lines are listed
// together above one copy of those lines.  tests/test_u8_gemm_route.py builds this with g++ alone and compares the
// output byte for byte with tests/golden/u8_gemm_route_table.txt, which was generated from the selection predicates
// u8_batch.hip had before the route existed: any difference is a change of which kernel serves a batch, or of its
// bookkeeping.
//
// Grid line:   == grid (product, or the developer switch set)
// Key lines:   @ a list of actual_dim
//              | every cu_count/multiplier/pass/store rows at which those row lengths have the change lines below
// Change line: n_queries  kernel  wave lists  list launches  slice queries  sample block rows  rs_frags  rs_ok
//              rq groups/pairs_lo/pairs_extra/streams_per_xcd (or -)
// Kernels: gemm pp rs qs16 qr16 rq16 rk16 (u8_gemm_<name>_kernel; gemm is u8_gemm_kernel).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../quantization_amd/csrc/u8_gemm_route.hpp"

namespace {

struct Fields {
    std::string kernel;
    bool lists = false;
    uint32_t launches = 0;
    uint64_t slice = 0;
    uint32_t block_rows = 0;
    int frags = 0;
    bool rs_ok = false;
    bool has_rq = false;
    uint32_t rq[4] = {0, 0, 0, 0};
};

// ---- evaluation: the one part that knows the code under test
Fields evaluate(const U8GemmInputs &in, const U8GemmSwitches &sw) {
    const U8GemmRoute r = u8_gemm_route(in, sw);
    Fields f;
    f.kernel = r.name;
    f.lists = r.wave_lists;
    f.launches = r.list_launches;
    f.slice = r.slice_queries;
    f.block_rows = r.sample_block_rows;
    f.frags = r.rs_frags;
    f.rs_ok = r.rs_ok;
    f.has_rq = r.kernel == U8GemmKernel::Rq16 || r.kernel == U8GemmKernel::Rk16;
    if (f.has_rq) {
        f.rq[0] = r.rq.groups;
        f.rq[1] = r.rq.pairs_lo;
        f.rq[2] = r.rq.pairs_extra;
        f.rq[3] = r.rq.streams_per_xcd;
    }
    return f;
}
// ---- end of evaluation

std::string format(const Fields &f) {
    std::string k = f.kernel;  // u8_gemm_rs_kernel -> rs, u8_gemm_kernel -> gemm
    k = k.substr(0, k.size() - strlen("_kernel")).substr(strlen("u8_"));
    if (k != "gemm") k = k.substr(strlen("gemm_"));
    char buf[160];
    int n = snprintf(buf, sizeof buf, "%s %d %u %llu %u %d %d ", k.c_str(), (int)f.lists, f.launches, (unsigned long long)f.slice,
                     f.block_rows, f.frags, (int)f.rs_ok);
    if (f.has_rq) snprintf(buf + n, sizeof buf - n, "%u/%u/%u/%u", f.rq[0], f.rq[1], f.rq[2], f.rq[3]);
    else snprintf(buf + n, sizeof buf - n, "-");
    return buf;
}

struct Config {
    const char *grid;
    int cu_count;
    float multiplier;
    const char *multiplier_text;
    U8GemmSwitches sw;
};

// The keys of the current grid by their change lines, in the order the change lines were first seen.
struct Group {
    std::string changes;
    std::vector<std::string> prefixes;     // "cu/multiplier/pass/rows", in the order first seen
    std::vector<std::string> dims_of;      // per prefix: its row lengths
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
            printf("@%s", g.dims_of[i].c_str());
            int on_line = 0;
            for (size_t j = i; j < g.prefixes.size(); j++) {
                if (g.dims_of[j] != g.dims_of[i]) continue;
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

void sweep(const Config &c, const std::vector<uint64_t> &dims) {
    if (g_grid != c.grid) flush();
    g_grid = c.grid;
    const U8GemmPass passes[3] = {U8GemmPass::Score, U8GemmPass::Sample, U8GemmPass::Filter};
    const char *pass_names[3] = {"score", "sample", "filter"};
    for (uint64_t rows : {1000ull, 131071ull, 131072ull})
        for (uint64_t ad : dims)
            for (int p = 0; p < 3; p++) {
                std::string last, changes;
                for (uint64_t nq = 1; nq <= 9000; nq++) {
                    U8GemmInputs in;
                    in.actual_dim = ad;
                    in.rows = rows;
                    in.multiplier = c.multiplier;
                    in.n_queries = nq;
                    in.q_pad = (nq + 255) / 256 * 256;  // what qamd_u8_encode_query_batch pads to
                    const uint32_t nkb = (uint32_t)((ad + 127) / 128);
                    in.frag_nkb = nkb <= 12 ? nkb : 0;  // ... and the rows it makes a fragment copy for
                    in.cu_count = c.cu_count;
                    in.pass = passes[p];
                    in.whole_store = true;
                    const std::string now = format(evaluate(in, c.sw));
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
                const std::string prefix = std::to_string(c.cu_count) + "/" + c.multiplier_text + "/" + pass_names[p] + "/" + std::to_string(rows);
                size_t i = 0;
                while (i < g.prefixes.size() && g.prefixes[i] != prefix) i++;
                if (i == g.prefixes.size()) {
                    g.prefixes.push_back(prefix);
                    g.dims_of.emplace_back();
                }
                g.dims_of[i] += " " + std::to_string(ad);
            }
}

}  // namespace

int main() {
    const std::vector<uint64_t> dims = {16,   64,   96,   128,  144,  208,  256,  384,  512,  640,  768,   896,
                                        1024, 1040, 1152, 1168, 1536, 1552, 2304, 2320, 4608, 4624, 32768, 32784};
    const float inf = std::numeric_limits<float>::infinity();
    // the product: every switch at its default
    sweep({"product", 256, 0.5f, "0.5", {}}, dims);
    sweep({"product", 256, -0.5f, "-0.5", {}}, dims);
    sweep({"product", 256, 0.0f, "0", {}}, dims);
    sweep({"product", 256, inf, "inf", {}}, dims);
    for (int cu : {128, 64, 40, 32}) sweep({"product", cu, 0.5f, "0.5", {}}, dims);

    // one developer switch at a time
    const std::vector<uint64_t> few = {256, 768, 1024, 1536, 4608};
    for (const char *family : {"r", "q", "p", "g", "s", "0"}) {
        U8GemmSwitches sw;
        sw.forced = true;
        sw.family = family[0];
        const std::string grid = std::string("QAMD_GEMM_CFG=") + family;
        sweep({grid.c_str(), 256, 0.5f, "0.5", sw}, few);
    }
    {
        U8GemmSwitches sw;
        sw.rq = false;
        sweep({"QAMD_RQ=0", 256, 0.5f, "0.5", sw}, few);
    }
    {
        U8GemmSwitches sw;
        sw.rq_k = false;
        sweep({"QAMD_RQ_K=0", 256, 0.5f, "0.5", sw}, few);
    }
    {
        U8GemmSwitches sw;
        sw.rq_groups = {true, 6};
        sweep({"QAMD_RQ_GROUPS=6", 256, 0.5f, "0.5", sw}, few);
    }
    {
        U8GemmSwitches sw;
        sw.qr_min = {true, 3};
        sw.qr_max = {true, 512};
        sweep({"QAMD_QR_MIN=3,QAMD_QR_MAX=512", 256, 0.5f, "0.5", sw}, few);
    }
    {
        U8GemmSwitches sw;
        sw.rq_min = {true, 3};
        sw.rq_max = {true, 600};
        sweep({"QAMD_RQ_MIN=3,QAMD_RQ_MAX=600", 256, 0.5f, "0.5", sw}, few);
    }
    flush();
    return 0;
}
