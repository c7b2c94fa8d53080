// conv1x1_plan_walk.cpp -- host-only walk of the 1x1-convolution launch plan (vmambair_amd/csrc/oss_conv1x1_plan.h) over a denser
// grid than tests/test_conv1x1_plan_host.py, with random strides and alignments, meant to be built with the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/conv1x1_plan_walk.cpp -o conv1x1_plan_walk && ./conv1x1_plan_walk
// It needs no GPU and no HIP.  Every accepted plan must cover the call, respect the grid and LDS limits and pick only kernels whose
// preconditions the call meets; exit status 0 and a count when all do.
#include "../vmambair_amd/csrc/oss_conv1x1_plan.h"

#include <cstdio>
#include <random>

using namespace oss;

static long g_bad = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond) && g_bad++ < 20) std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
    } while (0)

static void check(const Conv1x1Call &c, const Conv1x1Plan &pl) {
    const bool f32 = pl.family >= CONV1X1_F32_TILE64, wg = pl.family == CONV1X1_WG;
    const bool pairs = pl.family == CONV1X1_PAIR || pl.family == CONV1X1_PAIRW || pl.family == CONV1X1_PAIRK;
    CHECK((long)pl.grid[0] * pl.pt >= c.P && (long)(pl.grid[0] - 1) * pl.pt < c.P);
    CHECK(pl.grid[0] >= 1 && pl.grid[1] >= 1 && pl.grid[2] >= 1 && pl.grid[1] <= 65535 && pl.grid[2] <= 65535);
    CHECK(pl.lds_bytes <= 160 * 1024 && (pl.block == 256 || (f32 && pl.family != CONV1X1_F32_SPLITK && pl.block == 64)));
    CHECK(f32 == (c.io == OSS_F32));
    if (f32) {
        CHECK((long)pl.grid[1] * pl.mt * 32 >= c.M && pl.grid[2] == (unsigned)c.B && pl.per == pl.mt && (pl.mt == 1 || pl.mt == 2));
        CHECK(pl.x3 == c.f32_split && c.P % 4 == 0 && ((c.x_lo | c.y_lo | c.res_lo) & 15u) == 0 && c.xsb % 4 == 0 && c.xsk % 4 == 0);
        CHECK((pl.family == CONV1X1_F32_SPLITK) == (pl.lds_bytes != 0));
        CHECK(pl.family != CONV1X1_F32_SPLITK || c.K >= (pl.x3 ? 64 : 32));
        return;
    }
    CHECK(pl.grid[1] == (unsigned)c.B && (long)pl.grid[2] * pl.per * 32 >= c.M && pl.per >= 1);
    CHECK(wg || (long)(pl.grid[2] - 1) * pl.per * 32 < c.M);
    CHECK(!pl.x3 && pl.ln == c.ln);
    if (pl.family == CONV1X1_WG || pl.family == CONV1X1_PAIR || pl.family == CONV1X1_REUSE) CHECK(pl.ks * 16 >= c.K);
    if (wg) {
        CHECK(c.ln || c.wg_on);
        CHECK(conv1x1_wg_takes(c.io, c.M, c.K, c.P, c.xsb, c.xsk, c.x_lo | c.y_lo | c.w_lo | c.res_lo, c.has_res) && !c.has_res && !pl.res);
        CHECK(pl.ks * 16 == c.K && (pl.pt == 64 || pl.pt == 128) && (!c.wg_pixels || pl.pt == c.wg_pixels) && pl.nz == (int)pl.grid[2]);
        CHECK(pl.lds_bytes == conv1x1_wg_lds_bytes(c.K, pl.pt, false) && c.wimg_lo == 0 && pl.wimg == c.has_wimg);
        CHECK(pl.wt == (c.ws_m == 1 && c.ws_k == c.M));
    } else {
        CHECK(pl.lds_bytes == 0 && !c.ln);
        CHECK(!c.wg_on || !((c.ws_m == 1 && c.ws_k == c.M) || (c.ws_k == 1 && c.ws_m == c.K)) ||
              !conv1x1_wg_takes(c.io, c.M, c.K, c.P, c.xsb, c.xsk, c.x_lo | c.y_lo | c.w_lo | c.res_lo, c.has_res));
    }
    if (pl.wvec || pl.family == CONV1X1_PAIRW) CHECK(c.w_lo == 0 && c.ws_k == 1 && c.ws_m == c.K);
    if (pl.wvec) CHECK(c.K % 8 == 0 && !pl.wt && !pl.wimg);
    if (pairs) CHECK(c.P % 2 == 0 && c.xsk % 2 == 0 && c.xsb % 2 == 0 && ((c.x_lo | c.y_lo) & 3u) == 0 && c.xsk < (1 << 24));
    if (pl.wimg) CHECK(c.has_wimg && (wg || ((pl.family == CONV1X1_PAIR || pl.family == CONV1X1_PAIRK) && !pl.wt && !pl.wvec)));
    if (pl.family == CONV1X1_PAIRW) CHECK(!c.has_wimg && c.K <= 512 && pl.per == 1);
    if (pl.family == CONV1X1_PAIRK) CHECK(pl.ks == 8 && pl.mt == pl.per && pl.mt >= 1 && pl.mt <= 3 && c.K > 192);
    if (pl.family == CONV1X1_PAIR) CHECK(pl.res == c.has_res && pl.pf == conv1x1_pair_pf(pl.ks, pl.wimg));
    if (pl.family == CONV1X1_REUSE) CHECK((pl.ks == 6 || pl.ks == 12) && (pl.wt || (c.w_lo == 0 && c.K % 8 == 0)));
    if (pl.wt) CHECK(c.ws_m == 1 && c.ws_k == c.M);
}

int main() {
    const oss_dtype ios[] = {OSS_BF16, OSS_F16, OSS_F32};
    const int batches[] = {1, 2, 3, 4, 8, 32, 255, 256, 65535, 65536};
    const int rows[] = {1, 31, 32, 33, 40, 48, 96, 127, 192, 254, 255, 510, 765, 1024, 32 * 65535, 32 * 65535 + 1};
    const int ks[] = {1, 8, 16, 30, 32, 40, 48, 49, 64, 80, 96, 97, 112, 127, 128, 129, 176, 192, 193, 255, 256, 510, 512, 513, 520};
    const int pixels[] = {1, 2, 4, 62, 63, 64, 126, 128, 256, 1000, 1024, 4096, 16384, 25600, 65536};
    const int overrides[][2] = {{1, 0}, {0, 0}, {1, 64}, {1, 128}, {0, 128}};
    std::mt19937 rng(1);
    long plans = 0, accepted = 0;
    for (oss_dtype io : ios) for (int dgrad = 0; dgrad < 2; ++dgrad) for (int B : batches) for (int M : rows) for (int K : ks) for (int P : pixels)
        for (auto &ov : overrides) for (int rep = 0; rep < 6; ++rep) {
            // the shape as an entry point hands it over; now and then strides the entry points never produce
            const unsigned r = rng();
            Conv1x1Call c{};
            c.io = io; c.B = B; c.M = M; c.K = K; c.P = P;
            const int pads[] = {0, 0, 1, 2, 4, 8, 128, 3}, pad = pads[r & 7];
            c.xsk = P + pad; c.xsb = (int64_t)c.xsk * (K + ((r >> 3) & 1));
            c.ws_m = dgrad ? 1 : K; c.ws_k = dgrad ? M : 1;
            if (((r >> 4) & 31) == 0) { c.ws_m = K + 8; c.ws_k = 1; }
            const unsigned lows[] = {0, 0, 0, 2, 4, 8, 1, 12};
            c.x_lo = lows[(r >> 9) & 7]; c.y_lo = lows[(r >> 12) & 7]; c.w_lo = lows[(r >> 15) & 7] & ~3u;
            c.has_bias = !dgrad && ((r >> 18) & 1);
            c.has_res = !dgrad && ((r >> 19) & 1);
            c.res_lo = c.has_res ? lows[(r >> 20) & 7] : 0;
            c.has_wimg = io != OSS_F32 && ((r >> 23) & 1);
            c.wimg_lo = 0;   // the entry points refuse an unaligned image
            c.f32_split = io == OSS_F32 && ((r >> 24) & 1);
            c.ln = !dgrad && io != OSS_F32 && ((r >> 25) & 7) == 0;
            c.wg_on = ov[0]; c.wg_pixels = ov[1];
            Conv1x1Plan pl;
            const int rc = conv1x1_plan(c, pl);
            ++plans;
            CHECK(rc == OSS_OK || rc == OSS_ERR_SHAPE);
            if (rc != OSS_OK) {
                // refusals: fp32 rules, the grid limits, a LayerNorm call the workgroup-level kernel does not take
                CHECK(io == OSS_F32 || c.ln || B > 65535 || (M + 31) / 32 > 65535);
                continue;
            }
            ++accepted;
            check(c, pl);
        }
    std::printf("%ld plans (%ld accepted), %ld violations\n", plans, accepted, g_bad);
    return g_bad ? 1 : 0;
}
