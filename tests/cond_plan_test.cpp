// cond_plan.h on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_host_mimo.py builds and runs this): the LDS
// regions indexed as k_cond indexes them inside a mock of the workgroup's LDS, the batch loop of a capped grid covering every matrix once,
// the 64 KiB line, the refusals, the permutation check.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "cond_plan.h"

using namespace sp;

static int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                           \
        }                                                      \
    } while (0)

// walks one call as the kernel does: what of the LDS is indexed, which workgroup takes which matrix
static void walk(int n, int q, int64_t count, unsigned want, int64_t grid_force) {
    CHECK(cond_shape(n, q, count, want) == nullptr);
    const CondPlan p = cond_plan_of(n, count, want, grid_force);
    const bool wantP = (want & COND_WANT_P) != 0;
    const int LD = cond_pitch(n), lg = cond_lg(n), msk = (1 << lg) - 1;
    CHECK(p.pitch == LD && (LD & 1) == 1 && LD >= n && LD <= n + 1);
    CHECK((1 << lg) >= n && (lg == 0 || (1 << (lg - 1)) < n));
    CHECK(p.wg == cond_wg(n) && p.wg % 64 == 0 && p.wg <= 512 && p.wg >= n);
    CHECK(p.lds_bytes == cond_lds(n, wantP) && p.lds_bytes <= COND_LDS_MAX && p.raised == (p.lds_bytes > 65536 ? 1 : 0));
    CHECK(cond_off_w(n) % 16 == 0 && cond_off_diag(n, wantP) % 16 == 0);
    CHECK(cond_off_diag(n, wantP) == (wantP ? 2 : 1) * (int64_t)n * LD * 16 && cond_off_diag(n, wantP) + COND_MAX_N * 8 + 16 == p.lds_bytes);
    // the regions inside a mock of the LDS: every element the kernel touches lies in its own region
    std::vector<unsigned char> lds((size_t)p.lds_bytes, 0);
    unsigned char *base = lds.data();
    for (int e = 0; e < (n << lg); ++e) {
        const int i = e >> lg, k = e & msk;
        CHECK(i < n);
        if (k > i) continue;
        const int64_t a_off = ((int64_t)i * LD + k) * 16;
        CHECK(a_off + 16 <= cond_off_w(n));
        base[a_off] |= 1;
        if (wantP) {
            const int64_t w_off = cond_off_w(n) + a_off;
            CHECK(w_off + 16 <= cond_off_diag(n, true));
            base[w_off] |= 2;
        }
    }
    for (int i = 0; i < n; ++i) {
        const int64_t d_off = cond_off_diag(n, wantP) + (int64_t)i * 8;
        CHECK(d_off + 8 <= p.lds_bytes);
        CHECK(base[d_off] == 0);
        base[d_off] |= 4;
    }
    // a column walked by the lanes of a 16-lane group lands on 16 distinct 16 B slots of the 256 B bank row
    if (n >= 16) {
        unsigned seen = 0;
        for (int i = 0; i < 16; ++i) seen |= 1u << ((i * LD) % 16);
        CHECK(seen == 0xffffu);
    }
    // the batch loop
    CHECK(p.grid <= COND_MAX_GRID && (count == 0 ? p.grid == 0 : p.grid >= 1) && p.grid <= count);
    if (grid_force > 0) CHECK(p.grid <= grid_force);
    if (count <= (1 << 20)) {
        std::vector<int> taken((size_t)count, 0);
        int64_t most = 0;
        for (int64_t wg = 0; wg < p.grid; ++wg) {
            int64_t mine = 0;
            for (int64_t b = wg; b < count; b += p.grid, ++mine) ++taken[(size_t)b];
            if (mine > most) most = mine;
        }
        for (int64_t b = 0; b < count; ++b) CHECK(taken[(size_t)b] == 1);
        CHECK(most == p.per_wg);
    }
}

int main() {
    const unsigned wants[] = {COND_WANT_H, COND_WANT_GC, COND_WANT_MCOH, COND_WANT_PIV, COND_WANT_P, COND_WANT_ALL, COND_WANT_ALL & ~COND_WANT_P};
    for (int n = 1; n <= COND_MAX_N; ++n)
        for (unsigned w : wants)
            for (int q : {0, 1, n / 2, n - 1, n})
                if (q >= 0 && q <= n) walk(n, q, 3, w, 0);
    walk(64, 32, 2049, COND_WANT_ALL, 0);
    walk(16, 8, 513, COND_WANT_ALL, 0);
    walk(4, 2, 65536, COND_WANT_ALL, 0);
    walk(4, 2, 65537, COND_WANT_ALL, 0);
    walk(4, 2, (int64_t)1 << 20, COND_WANT_H, 0);
    walk(5, 2, 5, COND_WANT_ALL, 1);
    walk(5, 2, 5, COND_WANT_ALL, 2);
    walk(5, 2, 5, COND_WANT_ALL, 99);
    walk(7, 7, 0, COND_WANT_P, 0);
    walk(64, 0, COND_MAX_COUNT, COND_WANT_PIV, 0);
    // the 64 KiB line: with P between orders 45 and 46, without it between 63 and 64
    CHECK(cond_plan_of(45, 1, COND_WANT_P, 0).raised == 0 && cond_plan_of(46, 1, COND_WANT_P, 0).raised == 1);
    CHECK(cond_plan_of(63, 1, COND_WANT_H, 0).raised == 0 && cond_plan_of(64, 1, COND_WANT_H, 0).raised == 1);
    CHECK(cond_plan_of(64, 1, COND_WANT_ALL, 0).lds_bytes == 2 * 64 * 65 * 16 + 528);
    // refusals
    CHECK(cond_shape(0, 0, 1, 1) && cond_shape(65, 0, 1, 1) && cond_shape(-1, 0, 1, 1));
    CHECK(cond_shape(8, -1, 1, 1) && cond_shape(8, 9, 1, 1) && !cond_shape(8, 8, 1, 1) && !cond_shape(8, 0, 1, 1));
    CHECK(cond_shape(8, 4, -1, 1) && cond_shape(8, 4, COND_MAX_COUNT + 1, 1) && !cond_shape(8, 4, 0, 1));
    CHECK(cond_shape(8, 4, 1, 0) && cond_shape(8, 4, 1, 32) && cond_shape(8, 4, 1, 0x80000000u) && !cond_shape(8, 4, 1, 31));
    // permutations
    {
        std::vector<int32_t> o(64);
        for (int i = 0; i < 64; ++i) o[(size_t)i] = 63 - i;
        CHECK(cond_is_perm(o.data(), 64));
        o[5] = o[6];
        CHECK(!cond_is_perm(o.data(), 64));
        o[5] = 64;
        CHECK(!cond_is_perm(o.data(), 64));
        o[5] = -1;
        CHECK(!cond_is_perm(o.data(), 64));
        const int32_t one[1] = {0}, bad[1] = {1}, three[3] = {2, 0, 1};
        CHECK(cond_is_perm(one, 1) && !cond_is_perm(bad, 1) && cond_is_perm(three, 3));
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("cond_plan ok\n");
    return 0;
}
