// CPU unit test of the autoregressive fits' host arithmetic (pyfft_amd/csrc/ar_plan.h); built and run by
// tests/test_host_parametric.py::test_plan_arithmetic_under_sanitizers with g++ (no HIP) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  A segment's slots are a std::vector of exactly the planned size, so that a slot past them is a report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ar_plan.h"

using namespace sp;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

// every length takes a form that holds it, with the samples in the last n slots and every sample's predecessor one slot before it
static void test_forms() {
    for (int force = 0; force <= 2; ++force)
        for (int64_t n = 2; n <= BURG_MAX_N; n += (n < 2100 ? 1 : 97)) {
            int spl = 0, nw = 0;
            burg_form(n, force, &spl, &nw);
            CHECK(spl >= 1 && spl <= 16 && nw >= 1 && nw <= 16 && (int64_t)64 * nw * spl >= n);
            CHECK((nw == 1) == (n <= BURG_WAVE_MAX && force != 2));
            if (nw == 1 && spl > 1) CHECK((int64_t)64 * (spl / 2) < n);      // the smallest that holds it
            std::vector<int64_t> slot((size_t)64 * nw * spl, -1);
            const int64_t off = (int64_t)slot.size() - n;
            for (int64_t t = 0; t < 64 * nw; ++t)
                for (int j = 0; j < spl; ++j) {
                    const int64_t i = t * spl + j - off;
                    if (i >= 0) slot.at((size_t)(t * spl + j)) = i;
                }
            CHECK(slot.back() == n - 1 && slot.at((size_t)off) == 0 && (off == 0 || slot.at((size_t)off - 1) == -1));
        }
    int spl, nw;
    burg_form(1024, 0, &spl, &nw);
    CHECK(spl == 16 && nw == 1);
    burg_form(1025, 0, &spl, &nw);
    CHECK(spl == 8 && nw == 4);
    burg_form(1024, 2, &spl, &nw);
    CHECK(spl == 8 && nw == 4);
    burg_form(16384, 1, &spl, &nw);
    CHECK(spl == 16 && nw == 16);
    burg_form(64, 0, &spl, &nw);
    CHECK(spl == 1 && nw == 1);
    burg_form(65, 0, &spl, &nw);
    CHECK(spl == 2 && nw == 1);
}

static void test_tiles() {
    const int64_t ns[] = {2, 2047, 2048, 2049, 100003, 3 * 2048 + 5, (int64_t)1 << 21, ((int64_t)1 << 21) + 1, (int64_t)1 << 30, YULE_MAX_N};
    for (int64_t n : ns) {
        const int64_t c = ar_chunk(n), tiles = (n + c - 1) / c;
        CHECK(c >= AR_STAGE && c % AR_STAGE == 0 && tiles >= 1 && tiles <= AR_MAX_TILES && tiles * c >= n && (tiles - 1) * c < n);
    }
    CHECK(ar_chunk(100003) == 2048 && ar_chunk((int64_t)1 << 21) == 2048 && ar_chunk(((int64_t)1 << 21) + 1) == 4096);
    CHECK(ar_chunk(YULE_MAX_N) == ((int64_t)1 << 21));
}

static void test_plans() {
    ArPlan p = ar_plan_of(AR_METHOD_BURG, false, 256, 16, 15, 0, 0);
    CHECK(p.form == AR_FORM_WAVE && p.spl == 4 && p.nw == 1 && p.segs_per_wg == 4 && p.threads == 256 && p.spp == 15 && p.passes == 1 && p.workgroups == 4);
    CHECK(p.lds_bytes == 4 * 2 * 16 * 8);                             // two buffers of `order` coefficients per segment
    p = ar_plan_of(AR_METHOD_BURG, true, 256, 16, 15, 0, 7);
    CHECK(p.spp == 7 && p.passes == 3 && p.workgroups == 2 + 2 + 1 && p.lds_bytes == 4 * 2 * 16 * 16);
    p = ar_plan_of(AR_METHOD_BURG, true, 16384, 256, 3, 0, 0);
    CHECK(p.form == AR_FORM_WG && p.threads == 1024 && p.workgroups == 3 && p.lds_bytes == 2 * 256 * 16 + 2 * 16 * (32 + 16) && p.lds_bytes <= 64 * 1024);
    p = ar_plan_of(AR_METHOD_YULE, false, 100003, 20, 2, 0, 0);
    CHECK(p.form == AR_FORM_LAGS && p.tiles == 49 && p.chunk == 2048 && p.workgroups == 98 && p.passes == 1);
    CHECK(p.lds_bytes == (2048 + 256) * 4 + 2 * 256 * 8 && p.lds_bytes <= 64 * 1024);
    p = ar_plan_of(AR_METHOD_YULE, true, YULE_MAX_N, 256, 5, 0, 0);   // 1024 tiles of 257 complex lags: 4 MiB a segment, 63 to a pass
    CHECK(p.tiles == 1024 && p.spp == 5 && p.passes == 1 && (size_t)p.spp * p.tiles * 257 * 16 <= AR_SCRATCH_BYTES);
    p = ar_plan_of(AR_METHOD_YULE, true, YULE_MAX_N, 256, 100, 0, 0);
    CHECK(p.spp == 63 && p.passes == 2 && p.workgroups == 100 * 1024);
    p = ar_plan_of(AR_METHOD_BURG, false, 64, 4, ((int64_t)1 << 40), 0, 0);      // the most segments
    CHECK(p.spp == AR_PASS_SEGS && p.passes == ((int64_t)1 << 20) && p.workgroups == ((int64_t)1 << 38));
    p = ar_plan_of(AR_METHOD_BURG, false, 64, 4, 0, 0, 0);
    CHECK(p.passes == 0 && p.workgroups == 0 && p.spp == 1);
}

static void test_refusals() {
    CHECK(!ar_shape(AR_METHOD_BURG, 64, 4, 1, 1) && !ar_shape(AR_METHOD_BURG, BURG_MAX_N, AR_MAX_ORDER, 0, 0));
    CHECK(!ar_shape(AR_METHOD_YULE, YULE_MAX_N, AR_MAX_ORDER, 1, 1) && !ar_shape(AR_METHOD_BURG, 2, 1, 1, 1));
    CHECK(ar_shape(2, 64, 4, 1, 1) && ar_shape(AR_METHOD_BURG, 64, 0, 1, 1) && ar_shape(AR_METHOD_BURG, 1024, 257, 1, 1));
    CHECK(ar_shape(AR_METHOD_BURG, 64, 33, 1, 1) && ar_shape(AR_METHOD_BURG, 65, 33, 1, 1) && !ar_shape(AR_METHOD_BURG, 66, 33, 1, 1));
    CHECK(ar_shape(AR_METHOD_BURG, BURG_MAX_N + 1, 4, 1, 1) && !ar_shape(AR_METHOD_YULE, BURG_MAX_N + 1, 4, 1, 1));
    CHECK(ar_shape(AR_METHOD_YULE, YULE_MAX_N + 1, 4, 1, 1) && ar_shape(AR_METHOD_YULE, 1, 1, 1, 1));
    CHECK(ar_shape(AR_METHOD_BURG, 64, 4, -1, 1) && ar_shape(AR_METHOD_BURG, 64, 4, 1, -1) && ar_shape(AR_METHOD_BURG, 64, 4, (int64_t)1 << 31, 1));
    CHECK(ar_shape(AR_METHOD_BURG, 64, 4, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) - 1));
}

int main() {
    test_forms();
    test_tiles();
    test_plans();
    test_refusals();
    printf("ar plan ok\n");
    return 0;
}
