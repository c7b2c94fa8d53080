// scan_plan_walk.cpp -- host-only walk of the scan launch plan (vmambair_amd/csrc/oss_scan_plan.h) over the grid of
// tests/test_scan_plan_host.py, meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scan_plan_walk.cpp -o scan_plan_walk && ./scan_plan_walk
// It needs no GPU and no HIP.  Every plan made with a workspace of exactly the queried size must be OSS_OK, fit that workspace
// and the LDS, and carry consistent segment numbers; exit status 0 and a count when all do.
#include "../vmambair_amd/csrc/oss_scan_plan.h"

#include <cstdio>
#include <cstring>

using namespace oss;

static long g_bad = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_bad++ < 20) std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
    } while (0)

static void check_segs(const ScanSegs &s, int n_chunks) {
    CHECK((s.n_seg - 1) * s.cps < n_chunks && n_chunks <= s.n_seg * s.cps);
    CHECK(s.ccps == (s.cps + s.csub - 1) / s.csub && (s.csub - 1) * s.ccps < s.cps);
    CHECK(s.n_cseg == s.n_seg * s.csub && s.n_cseg <= scan_max_slots(n_chunks));
}

int main() {
    static float stand_in[1];   // addresses that are never dereferenced
    const int batches[] = {1, 2, 8}, seqlens[] = {1, 255, 257, 512, 513, 1061, 2085, 3000, 4096, 6600, 16384, 33000};
    const int dim_groups[][2] = {{24, 2}, {26, 2}, {48, 4}, {384, 4}, {96, 1}, {12, 1}, {7, 7}};
    const int dstates[] = {1, 5, 16, 40, 64, 72, 250}, seg_reqs[] = {-1, 0, 2, 3, 7, 64}, splits[] = {0, 1, 2, 4, 64};
    const int fwd_variants[] = {0, 1, 2, 3, 4, 6, 5, 99}, bwd_variants[] = {1, 10, 11, 12, 13, 0, 9, 99};
    long plans = 0;
    for (int split : splits) {
        g_carry_split.store(split);
        for (int B : batches) for (auto &dg : dim_groups) for (int L : seqlens) for (int N : dstates) for (int req : seg_reqs)
            for (int dtw = 0; dtw < 2; ++dtw) {
                const int dim = dg[0], G = dg[1];
                oss_scan_bwd_params q;
                std::memset(&q, 0, sizeof(q));
                oss_scan_fwd_params &f = q.f;
                f.batch = B; f.dim = dim; f.seqlen = L; f.dstate = N; f.n_groups = G;
                if (dtw) { f.dt_weight = stand_in; f.dt_rank = 5; q.ddt = stand_in; q.ddt_weight = stand_in; }
                const size_t fq = scan_fwd_workspace_bytes(B, dim, L, N, G), bq = scan_bwd_workspace_bytes(B, dim, L, N, G);
                for (int v : fwd_variants) {
                    f.workspace = stand_in; f.workspace_bytes = fq;
                    ScanFwdPlan pl;
                    CHECK(scan_fwd_plan(f, OSS_BF16, v, req, pl) == OSS_OK);
                    CHECK(pl.need_bytes <= fq && pl.lds_bytes <= kMaxLdsBytes);
                    check_segs(pl.seg, pl.n_chunks);
                    ++plans;
                }
                f.workspace = nullptr; f.workspace_bytes = 0;
                for (int v : bwd_variants) for (int hs = 0; hs < 2; ++hs) {
                    f.hs = hs ? stand_in : nullptr;
                    q.tune_partials = hs ? 0 : 2;
                    q.workspace = stand_in; q.workspace_bytes = bq;
                    ScanBwdPlan pl;
                    const int rc = scan_bwd_plan(q, OSS_BF16, v, req, pl);
                    ++plans;
                    if (dtw && N > 64) { CHECK(rc == OSS_ERR_SHAPE); continue; }
                    CHECK(rc == OSS_OK);
                    CHECK(pl.ws.need_bytes <= bq && pl.lds_bytes <= kMaxLdsBytes);
                    CHECK(pl.ws.bc <= pl.ws.dA && pl.ws.dA <= pl.ws.dD && pl.ws.dD < pl.ws.db && pl.ws.db < pl.ws.dW && pl.ws.dW <= pl.ws.carry);
                    CHECK(pl.ws.carry * sizeof(float) <= pl.ws.need_bytes);
                    check_segs(pl.seg, pl.n_chunks);
                    q.workspace_bytes = pl.ws.need_bytes - 1;   // one byte short: the next rung of the ladder, or an error
                    ScanBwdPlan lower;
                    const int rc2 = scan_bwd_plan(q, OSS_BF16, v, req, lower);
                    CHECK(rc2 == OSS_ERR_WORKSPACE ? pl.seg.n_seg == 1 : (rc2 == OSS_OK && lower.ws.need_bytes < pl.ws.need_bytes));
                }
            }
    }
    g_carry_split.store(0);
    std::printf("%ld plans, %ld violations\n", plans, g_bad);
    return g_bad ? 1 : 0;
}
