// CPU unit test of the type-1 NUFFT's host arithmetic (pyfft_amd/csrc/nufft_plan.h); built and run by
// tests/test_host_nufft.py::test_plan_arithmetic_under_sanitizers with g++ (no HIP) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  The tile lists are std::vectors of exactly the planned size, so that an entry past a list is a report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "nufft_plan.h"

using namespace sp;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            exit(1);                                                     \
        }                                                                \
    } while (0)

static void test_grid_and_plan() {
    CHECK(nufft_nf(1) == 1024 && nufft_nf(512) == 1024 && nufft_nf(513) == 2048 && nufft_nf(3000) == 8192 && nufft_nf(5000) == 16384);
    CHECK(nufft_nf(NUFFT_MAX_M) == ((int64_t)1 << 25) && nufft_nf(NUFFT_MAX_M) <= NUFFT_MAX_NF);
    const size_t budget = (size_t)256 << 20;
    NufftPlan p = nufft_plan_of(3000, 3, budget, 0);
    CHECK(p.nf == 8192 && p.tiles == 8 && p.rpp == 3 && p.passes == 1 && p.workgroups == 8);
    p = nufft_plan_of(130, 17, budget, 2);
    CHECK(p.nf == 1024 && p.tiles == 1 && p.rpp == 2 && p.passes == 9 && p.workgroups == 9);
    p = nufft_plan_of(130, 17, budget, 0);
    CHECK(p.rpp == 17 && p.passes == 1 && p.workgroups == 6);
    p = nufft_plan_of(1 << 20, 9, budget, 0);                    // nf 2^21: 16 MiB a row
    CHECK(p.nf == (1 << 21) && p.rpp == 9 && p.passes == 1 && p.workgroups == 2048 * 3);
    p = nufft_plan_of(NUFFT_MAX_M, 65536, budget, 0);            // nf 2^25: 256 MiB a row, one row per pass
    CHECK(p.rpp == 1 && p.passes == 65536 && p.workgroups == (int64_t)65536 * 32768);
    p = nufft_plan_of(100, 0, budget, 0);
    CHECK(p.passes == 0 && p.workgroups == 0 && p.rpp == 1);
    p = nufft_plan_of(100, 5, 0, 0);                             // no budget at all: still one row per pass
    CHECK(p.rpp == 1 && p.passes == 5);
}

// N = 2^31 - 1 samples in one cell, every one at the row's largest magnitude: the sum stays below 2^62, and the quantum stays finer
// than float32's at the row's largest magnitude
static void test_shift_bound() {
    const int64_t Ns[] = {1, 2, 3, 1000, ((int64_t)1 << 20) + 1, ((int64_t)1 << 31) - 1};
    const int es[] = {-148, -126, -10, 0, 1, 20, 127, 128};
    for (int64_t N : Ns)
        for (int e : es) {
            const int sh = nufft_shift(e, N);
            const float cmax = nextafterf(ldexpf(1.f, e > 127 ? 127 : e) * (e > 127 ? 2.f : 1.f), 0.f);        // just under 2^e
            const double v = 2.0 * (double)cmax;                 // |c| phi <= |re| + |im| <= 2 cmax
            const long long one = llrint(ldexp(v, sh));
            CHECK(one > 0);
            const __int128 total = (__int128)N * one;
            CHECK(total < ((__int128)1 << 62));
            CHECK(sh + e >= 28);                                 // 2^-shift <= 2^-28 2^e: four bits under float32's ulp at cmax
            CHECK(nufft_ceil_log2(N) <= 31);
        }
    CHECK(nufft_shift(0, ((int64_t)1 << 31) - 1) == 29 && nufft_shift(1, 1) == 59);
    CHECK(nufft_ceil_log2(1) == 0 && nufft_ceil_log2(2) == 1 && nufft_ceil_log2(3) == 2 && nufft_ceil_log2(1024) == 10 && nufft_ceil_log2(1025) == 11);
}

static void test_frac() {
    CHECK(nufft_frac(0.25, 2.0) == 0.5 && nufft_frac(-0.25, 1.0) == 0.75 && nufft_frac(3.0, 5.0) == 0.0 && nufft_frac(0.0, 7.0) == 0.0);
    CHECK(nufft_frac(-1e-30, 1.0) <= 1.0 && nufft_frac(-1e-30, 1.0) > 0.999);        // rounds up to the periodic end, never beyond
    // a far product: q tau = 2^40 + 1 + 2^-3 + 2^-43 exactly, of which the float64 product keeps 2^40 + 1 + 2^-3
    const double q = ldexp(1.0, 20) + ldexp(1.0, -20), tau = ldexp(1.0, 20) + ldexp(1.0, -23);
    CHECK(q * tau == ldexp(1.0, 40) + 1.125);
    CHECK(nufft_frac(q, tau) == 0.125 + ldexp(1.0, -43));
    for (int i = 0; i < 1000; ++i) {
        const double r = nufft_frac(-0.0123 * (i + 1), 1e9 / (i + 3));
        CHECK(r >= 0.0 && r <= 1.0);
    }
}

// every cell of a footprint belongs to one of the two tiles the sample is listed in; the lists, built as the kernels build them
// (count, scan, fill), hold every sample once per tile and never more than 2 N entries
static void check_lists(const std::vector<double> &pos, int64_t nf) {
    const int64_t tiles = nf / NUFFT_TILE, N = (int64_t)pos.size();
    std::vector<unsigned> count((size_t)tiles, 0);
    std::vector<NufftCell> cl;
    for (double p : pos) {
        const NufftCell c = nufft_cell(p, nf);
        CHECK(c.i0 >= 0 && c.i0 < nf && c.dx >= 0.f && c.dx <= 1.f);
        cl.push_back(c);
        int64_t a, b;
        nufft_tiles(c.i0, nf, &a, &b);
        CHECK(a >= 0 && a < tiles && b >= 0 && b < tiles);
        CHECK(b == a || b == (a + 1) % tiles);
        ++count[(size_t)a];
        if (b != a) ++count[(size_t)b];
        for (int l = 0; l < NUFFT_W; ++l) {
            const int64_t t = ((c.i0 + l) & (nf - 1)) / NUFFT_TILE;
            CHECK(t == a || t == b);
        }
        // the footprint's z runs over [-1, 1]
        CHECK((c.dx - NUFFT_W / 2) * (2.f / NUFFT_W) >= -1.f && (c.dx + NUFFT_W - 1 - NUFFT_W / 2) * (2.f / NUFFT_W) <= 1.f);
    }
    std::vector<int64_t> off((size_t)tiles + 1, 0);
    for (int64_t i = 0; i < tiles; ++i) off[(size_t)i + 1] = off[(size_t)i] + count[(size_t)i];
    CHECK(off[(size_t)tiles] <= 2 * N);
    std::vector<int> list((size_t)off[(size_t)tiles], -1);
    std::vector<unsigned> cur((size_t)tiles, 0);
    for (int64_t j = 0; j < N; ++j) {
        int64_t a, b;
        nufft_tiles(cl[(size_t)j].i0, nf, &a, &b);
        list[(size_t)(off[(size_t)a] + cur[(size_t)a]++)] = (int)j;
        if (b != a) list[(size_t)(off[(size_t)b] + cur[(size_t)b]++)] = (int)j;
    }
    for (int v : list) CHECK(v >= 0 && v < N);
    for (int64_t i = 0; i < tiles; ++i) CHECK(cur[(size_t)i] == count[(size_t)i]);
}

static void test_cells_and_seams() {
    for (int64_t nf : {(int64_t)1024, (int64_t)2048, (int64_t)8192, NUFFT_MAX_NF}) {
        const int64_t tiles = nf / NUFFT_TILE;
        NufftCell c = nufft_cell(0.0, nf);                       // the footprint wraps to the top of the grid
        CHECK(c.i0 == nf - NUFFT_W / 2 && c.dx == 0.f);
        int64_t a, b;
        nufft_tiles(c.i0, nf, &a, &b);
        CHECK(a == tiles - 1 && b == 0);
        c = nufft_cell(1.0, nf);                                 // frac may round up to 1: the same cells as 0
        CHECK(c.i0 == nf - NUFFT_W / 2 && c.dx == 0.f);
        c = nufft_cell(nextafter(1.0, 0.0), nf);
        CHECK(c.i0 == nf - NUFFT_W / 2 && c.dx >= 0.f && c.dx < 1e-3f);
        c = nufft_cell(1e-12, nf);                               // just over an integer edge: the next cell, a whole cell away
        CHECK(c.i0 == nf - NUFFT_W / 2 + 1 && c.dx > 0.999f && c.dx <= 1.f);
        std::vector<double> pos = {0.0, 1.0, nextafter(1.0, 0.0), 1e-12, 0.5};
        for (int64_t t = 0; t < tiles; t += tiles > 64 ? tiles / 7 : 1)
            for (int64_t cell : {t * NUFFT_TILE, t * NUFFT_TILE - NUFFT_W + 1, t * NUFFT_TILE - NUFFT_W, t * NUFFT_TILE + 1}) {
                const double x = ((double)cell + 0.5 * NUFFT_W) / (double)nf;        // the footprint's first cell is `cell`
                if (x < 0.0 || x > 1.0) continue;
                c = nufft_cell(x, nf);
                CHECK(c.i0 == ((cell % nf) + nf) % nf && c.dx == 0.f);
                pos.push_back(x);
                if (x > 0.0) pos.push_back(nextafter(x, 0.0));
                if (x < 1.0) pos.push_back(nextafter(x, 1.0));
            }
        for (int i = 0; i < 500; ++i) pos.push_back((double)((i * 2654435761u) % 1000003u) / 1000003.0);
        check_lists(pos, nf);
        std::vector<double> pile(300, 0.123456);                 // one cell takes every sample
        check_lists(pile, nf);
    }
}

// the Gauss-Legendre sum against Simpson's rule on a fine mesh, at the centre and at the largest mode a grid carries (k = nf / 4)
static void test_kernel_transform() {
    for (int64_t nf : {(int64_t)1024, (int64_t)16384}) {
        const NufftQuad q = nufft_quad(nf);
        for (int64_t k : {(int64_t)0, (int64_t)1, nf / 8, nf / 4, -nf / 4}) {
            const int n = 1 << 20;
            const double pi = 3.14159265358979323846, xi = pi * NUFFT_W * (double)k / (double)nf;
            double s = 0.0;
            for (int i = 0; i <= n; ++i) {
                const double z = -1.0 + 2.0 * i / n, u = 1.0 - z * z;
                const double f = exp(NUFFT_BETA * (sqrt(u > 0 ? u : 0) - 1.0)) * cos(xi * z);
                s += f * (i == 0 || i == n ? 1.0 : (i & 1 ? 4.0 : 2.0));
            }
            s *= (2.0 / n) / 3.0 * (NUFFT_W / 2);
            CHECK(fabs(nufft_phihat(q, k) - s) <= 2e-9 * nufft_phihat(q, 0));
            CHECK(nufft_phihat(q, k) > 0.02 * nufft_phihat(q, 0));          // the division is well conditioned over the modes kept
        }
    }
    CHECK(nufft_phi(0.f) == 1.f && nufft_phi(1.f) > 0.f && nufft_phi(1.f) < 2e-8f && nufft_phi(-1.f) == nufft_phi(1.f));
}

int main() {
    test_grid_and_plan();
    test_shift_bound();
    test_frac();
    test_cells_and_seams();
    test_kernel_transform();
    printf("nufft plan ok\n");
    return 0;
}
