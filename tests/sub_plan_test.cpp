// sub_plan_test.cpp -- pyfft_amd/csrc/sub_plan.h on the CPU, as its own program under AddressSanitizer and UndefinedBehaviorSanitizer:
// the tiles of every length cover the segment, the staged samples and the shares of k_cov_row stay inside its LDS, the scratch of a
// pass stays within its budget, the passes cover the segments, and the shapes the entries refuse.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "sub_plan.h"

using namespace sp;

static int fails = 0;
#define CHECK(c)                                                                                                 \
    do {                                                                                                         \
        if (!(c)) {                                                                                              \
            printf("FAIL line %d: %s\n", __LINE__, #c);                                                          \
            ++fails;                                                                                             \
        }                                                                                                        \
    } while (0)

// the loops of k_cov_row over one tile, marking every (t, share) it sums and every slot of the stage it touches
static void walk_tile(int64_t n, int m, const SubPlan &p, int64_t tile, std::vector<unsigned char> &seen, int64_t base) {
    const int64_t c0 = tile * p.chunk, c1 = c0 + p.chunk < n ? c0 + p.chunk : n;
    std::vector<int> stage(SUB_HALO + AR_STAGE, 0);
    for (int64_t sb = c0; sb < c1; sb += AR_STAGE) {
        const int len = c1 - sb < AR_STAGE ? (int)(c1 - sb) : AR_STAGE;
        const int t0 = sb >= m - 1 ? 0 : (int)(m - 1 - sb);
        for (int q = -(m - 1); q < len; ++q) {
            CHECK(sb + q < n);
            stage.at(SUB_HALO + q) = sb + q >= 0 ? 1 : 0;             // .at(): a slot outside the stage throws
        }
        if (t0 >= len) continue;
        const int run = (len - t0 + p.nsub - 1) / p.nsub;
        for (int u = 0; u < p.nsub; ++u) {
            const int q0 = t0 + u * run, q1 = q0 + run < len ? q0 + run : len;
            for (int q = q0; q < q1; ++q) {
                CHECK(stage.at(SUB_HALO + q) == 1 && stage.at(SUB_HALO + q - (m - 1)) == 1);   // the sample and its farthest partner exist
                if (sb + q >= base && sb + q - base < (int64_t)seen.size()) ++seen[sb + q - base];
            }
        }
    }
}

int main() {
    // every sample t = m - 1 .. n - 1 is summed exactly once, at short lengths and around the seams
    const int64_t lens[] = {2, 3, 8, 63, 64, 65, 333, 2047, 2048, 2049, 2048 + 7, 2 * 2048 + 63, 3 * 2048, 100003};
    const int ms[] = {2, 3, 7, 8, 24, 32, 63, 64};
    for (int64_t n : lens)
        for (int m : ms) {
            if (m > n) continue;
            for (int cplx = 0; cplx < 2; ++cplx) {
                const SubPlan p = sub_plan_of(SUB_WHAT_COVMAT, cplx, n, m, 3, 0);
                CHECK(p.chunk >= AR_STAGE && p.chunk % AR_STAGE == 0 && p.tiles >= 1 && p.tiles <= AR_MAX_TILES);
                CHECK(p.tiles * p.chunk >= n && (p.tiles - 1) * p.chunk < n);
                CHECK(p.nsub >= 4 && p.nsub * m <= 256);
                CHECK(p.lds_bytes == (int64_t)(SUB_HALO + AR_STAGE + 256) * (cplx ? 16 : 8) && p.lds_bytes <= 64 * 1024);
                CHECK(p.seg_bytes == p.tiles * m * (cplx ? 16 : 8));
                std::vector<unsigned char> seen(n, 0);
                for (int64_t t = 0; t < p.tiles; ++t) walk_tile(n, m, p, t, seen, 0);
                for (int64_t t = 0; t < n; ++t) CHECK(seen[t] == (t >= m - 1 ? 1 : 0));
            }
        }
    // the largest segment: tiles and chunk stay in range, the first and the last tile are walked
    {
        const int64_t n = YULE_MAX_N;
        const SubPlan p = sub_plan_of(SUB_WHAT_LS, true, n, 64, 5, 0);
        CHECK(p.tiles <= AR_MAX_TILES && p.tiles * p.chunk >= n && (p.tiles - 1) * p.chunk < n);
        CHECK(p.seg_bytes == p.tiles * 64 * 16 + 64 * 64 * 16);
        std::vector<unsigned char> head(4096, 0), tail(4096, 0);
        walk_tile(n, 64, p, 0, head, 0);
        walk_tile(n, 64, p, p.tiles - 1, tail, n - 4096);
        for (int t = 0; t < 4096; ++t) CHECK(head[t] == (t >= 63 ? 1 : 0) && tail[t] == 1);
    }
    // passes: they cover the segments, a pass stays within the scratch, the hook caps it
    const int64_t segs[] = {0, 1, 7, 11, 1000, (int64_t)1 << 20, ((int64_t)1 << 20) + 1, (int64_t)1 << 31, (int64_t)1 << 40};
    for (int what = 0; what < 2; ++what)
        for (int64_t n : {(int64_t)64, (int64_t)4096, (int64_t)100003, (int64_t)YULE_MAX_N})
            for (int m : {2, 16, 64})
                for (int64_t s : segs)
                    for (int64_t hook : {(int64_t)0, (int64_t)7}) {
                        const SubPlan p = sub_plan_of(what, true, n, m, s, hook);
                        CHECK(p.spp >= 1 && p.spp <= AR_PASS_SEGS);
                        CHECK(s == 0 ? p.passes == 0 : (p.passes * p.spp >= s && (p.passes - 1) * p.spp < s));
                        CHECK(p.spp == 1 || (size_t)p.spp * (size_t)p.seg_bytes <= SUB_SCRATCH_BYTES);
                        CHECK(hook == 0 || p.spp <= hook);
                        CHECK(p.workgroups == s * p.tiles);
                        CHECK(p.spp * p.tiles <= 0x7fffffff);
                    }
    // refusals
    CHECK(!sub_shape(0, 2, 2, 1, 1) && !sub_shape(0, 64, 64, 0, 0) && !sub_shape(1, 126, 64, 1, 1) && !sub_shape(0, YULE_MAX_N, 64, 1, 1));
    CHECK(sub_shape(2, 64, 8, 1, 1) && sub_shape(0, 64, 1, 1, 1) && sub_shape(0, 64, 65, 1, 1) && sub_shape(0, 7, 8, 1, 1));
    CHECK(sub_shape(1, 125, 64, 1, 1) && sub_shape(1, 64, 1, 1, 1) && sub_shape(1, 1000, 65, 1, 1) && sub_shape(0, 1, 2, 1, 1));
    CHECK(sub_shape(0, (int64_t)1 << 31, 8, 1, 1) && sub_shape(0, 64, 8, -1, 1) && sub_shape(0, 64, 8, 1, -1));
    CHECK(sub_shape(0, 64, 8, (int64_t)1 << 31, 1) && sub_shape(0, 64, 8, (int64_t)1 << 30, (int64_t)1 << 11));
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("sub plan ok\n");
    return 0;
}
