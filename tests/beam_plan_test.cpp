// beam_plan.h on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_host_beam.py builds and runs this): the tiles walked
// as k_beam walks them over a mock of its output row, the stage fetch's indices inside the eigenvector matrix and the LDS regions, the
// item loop of a capped grid covering every (model, tile) once, the refusals, the finiteness look at a table.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "beam_plan.h"

using namespace sp;

static int fails = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                         \
        }                                                    \
    } while (0)

// walks one call as the kernel does: who writes which output, what a stage reads, what of the LDS is indexed
static void walk(int m, int64_t nk, int64_t nmodels, int method, int p, int64_t grid_force) {
    const BeamPlan b = beam_plan_of(m, nk, nmodels, method, p, grid_force);
    CHECK(b.tiles * BEAM_TQ >= nk && (b.tiles - 1) * BEAM_TQ < nk);
    CHECK(b.items == nmodels * b.tiles && b.grid >= 1 && b.grid <= b.items && b.grid <= BEAM_MAX_GRID);
    CHECK(b.per_wg * b.grid >= b.items && (b.per_wg - 1) * b.grid < b.items);
    if (grid_force > 0) CHECK(b.grid <= grid_force);
    const int k_lo = beam_first(method, p), nn = m - k_lo;
    CHECK(nn >= 1 && b.stages == (nn + BEAM_KS - 1) / BEAM_KS && b.stages * BEAM_KS <= beam_gw_len());
    // the LDS regions in bytes: steer, vec, part, gw
    const int64_t o_vec = (int64_t)m * BEAM_TQ * 16, o_part = o_vec + (int64_t)m * BEAM_KS * 16, o_gw = o_part + BEAM_WAVES * BEAM_TQ * 8;
    CHECK(o_gw + beam_gw_len() * 8 == b.lds_bytes && b.lds_bytes <= 160 * 1024 && o_vec % 16 == 0 && o_part % 16 == 0);
    std::vector<int> written((size_t)(nmodels * nk), 0);
    std::vector<char> vmat((size_t)m * m, 0);                          // which elements of V the stages read
    int64_t most = 0;
    for (int64_t wg = 0; wg < b.grid; ++wg) {
        int64_t mine = 0;
        for (int64_t item = wg; item < b.items; item += b.grid, ++mine) {
            const int64_t model = item / b.tiles, tile = item - model * b.tiles, q0 = tile * BEAM_TQ;
            CHECK(model >= 0 && model < nmodels);
            for (int lane = 0; lane < BEAM_TQ; ++lane)
                if (q0 + lane < nk) ++written[(size_t)(model * nk + q0 + lane)];
            if (item == 0)
                for (int st = 0; st < b.stages; ++st) {
                    const int k0 = st * BEAM_KS, kc = nn - k0 < BEAM_KS ? nn - k0 : BEAM_KS;
                    CHECK(kc >= 1);
                    for (int tid = 0; tid < BEAM_WG; ++tid)
                        for (int j = 0; j < BEAM_MAX_M * BEAM_KS / BEAM_WG; ++j) {
                            const int idx = tid + j * BEAM_WG, i = idx / BEAM_KS, kk = idx - i * BEAM_KS;
                            if (i < m && kk < kc) {
                                const int k = k_lo + k0 + kk;
                                CHECK(k < m);
                                ++vmat[(size_t)i * m + k];
                            }
                            if (idx < m * BEAM_KS) CHECK(o_vec + (int64_t)idx * 16 + 16 <= o_part);
                        }
                    for (int wv = 0; wv < BEAM_WAVES; ++wv)
                        if (wv * BEAM_KB < kc) CHECK(k0 + wv * BEAM_KB + BEAM_KB <= beam_gw_len() && wv * BEAM_KB + BEAM_KB <= BEAM_KS);
                }
        }
        if (mine > most) most = mine;
    }
    CHECK(most == b.per_wg);
    for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1);
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < m; ++k) CHECK(vmat[(size_t)i * m + k] == (k >= k_lo ? 1 : 0));
}

int main() {
    const int ms[] = {2, 3, 23, 32, 33, 63, 64};
    const int64_t nks[] = {1, 63, 64, 65, 300};
    for (int m : ms)
        for (int64_t nk : nks)
            for (int method = 0; method < 4; ++method)
                for (int p : {0, 1, m - 1})
                    for (int64_t force : {0, 1, 3}) walk(m, nk, 3, method, p, force);
    walk(64, 1024, 40, BEAM_MUSIC, 2, 0);
    // the largest shapes: no overflow on the way to the figures
    BeamPlan b = beam_plan_of(64, 0x7fffffff, 1 << 14, BEAM_CAPON, 0, 0);
    CHECK(b.tiles == ((int64_t)1 << 25) && b.items == ((int64_t)1 << 39) && b.grid == BEAM_MAX_GRID && b.per_wg == ((int64_t)1 << 23));
    CHECK(beam_lds(64) == 64 * 96 * 16 + 8 * 64 * 8 + 64 * 8 && beam_lds(2) == 2 * 96 * 16 + 4096 + 512);
    CHECK(beam_plan_of(8, 100, 0, BEAM_BARTLETT, 0, 0).grid == 0 && beam_plan_of(8, 100, 0, BEAM_BARTLETT, 0, 0).per_wg == 0);
    // the refusals
    CHECK(!beam_shape(2, 1, 1, 0, 0, 0) && !beam_shape(64, 3, 0x7fffffff, 1 << 15, 3, 63) && !beam_shape(8, 1, 10, 1, 0, 99) && !beam_shape(8, 1, 10, 1, 1, -5));
    CHECK(beam_shape(1, 1, 10, 1, 0, 0) && beam_shape(65, 1, 10, 1, 0, 0) && beam_shape(8, 0, 10, 1, 0, 0) && beam_shape(8, 4, 10, 1, 0, 0));
    CHECK(beam_shape(8, 1, 0, 1, 0, 0) && beam_shape(8, 1, (int64_t)1 << 31, 1, 0, 0) && beam_shape(8, 1, 10, 1, -1, 0) && beam_shape(8, 1, 10, 1, 4, 0));
    CHECK(beam_shape(8, 1, 10, 1, 2, -1) && beam_shape(8, 1, 10, 1, 2, 8) && beam_shape(8, 1, 10, 1, 3, 8) && beam_shape(8, 1, 10, -1, 0, 0));
    CHECK(beam_shape(64, 1, 0x7fffffff, ((int64_t)1 << 15) + 1, 0, 0) && beam_shape(8, 1, 1, ((int64_t)1 << 40) + 1, 0, 0) && !beam_shape(8, 1, 1, (int64_t)1 << 40, 0, 0));
    // the look at a table
    std::vector<double> t(100, 1.5);
    CHECK(beam_finite(t.data(), 100) && beam_finite(t.data(), 0));
    t[99] = NAN;
    CHECK(!beam_finite(t.data(), 100) && beam_finite(t.data(), 99));
    t[0] = -INFINITY;
    CHECK(!beam_finite(t.data(), 1));
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("beam plan ok\n");
    return 0;
}
