// dwt_plan_test.cpp -- pyfft_amd/csrc/dwt_plan.h on the CPU, as its own program under AddressSanitizer and UndefinedBehaviorSanitizer:
// the index maps against the arrays they stand for, every level's length and offset for all modes and parities, the tiles of both
// directions walked as the kernels walk them (every output exactly once, every staged slot inside the LDS, the halo arithmetic in
// 64 bits at the largest row), the row form's buffers and its limit, the scratch and the passes, and the refusals.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "dwt_plan.h"

using namespace sp;

static int fails = 0;
#define CHECK(c)                                                                                                 \
    do {                                                                                                         \
        if (!(c)) {                                                                                              \
            printf("FAIL line %d: %s\n", __LINE__, #c);                                                          \
            ++fails;                                                                                             \
        }                                                                                                        \
    } while (0)

// the extension of 0 .. n - 1 built the slow way, one period to each side at a time, as far as `reach`
static std::vector<int64_t> extended(int64_t n, int mode, int64_t reach) {
    std::vector<int64_t> e;
    for (int64_t i = -reach; i < n + reach; ++i) {
        int64_t v;
        if (i >= 0 && i < n) v = i;
        else if (mode == DWT_ZERO) v = -1;
        else if (mode == DWT_CONSTANT) v = i < 0 ? 0 : n - 1;
        else if (mode == DWT_PERIODIC) v = ((i % n) + n) % n;
        else if (mode == DWT_PER) {
            const int64_t np = n + (n & 1), r = ((i % np) + np) % np;
            v = r == n ? n - 1 : r;
        } else if (mode == DWT_SYMMETRIC) {           // fold until inside: ... 1 0 | 0 1 .. n-1 | n-1 n-2 ...
            int64_t j = i;
            while (j < 0 || j >= n) j = j < 0 ? -1 - j : 2 * n - 1 - j;
            v = j;
        } else {                                      // reflect: ... 2 1 | 0 1 .. n-1 | n-2 ...
            int64_t j = i;
            if (n == 1) j = 0;
            while (j < 0 || j >= n) j = j < 0 ? -j : 2 * n - 2 - j;
            v = j;
        }
        e.push_back(v);
    }
    return e;
}

// k_dwt_tile's walk of one level: marks every output, checks every staged slot and every read
static void walk_ana(int64_t n, int L, int mode, std::vector<unsigned char> *seen) {
    const int64_t K = dwt_coeff_len(n, L, mode), tiles = (K + DWT_TILE - 1) / DWT_TILE;
    const int c = dwt_center(L, mode);
    for (int64_t t = 0; t < tiles; ++t) {
        const int64_t k0 = t * DWT_TILE, ib = dwt_tile_first(t, L, mode);
        const int Tk = (int)(K - k0 < DWT_TILE ? K - k0 : DWT_TILE), NI = 2 * Tk + L - 2;
        CHECK((int64_t)NI * 8 <= dwt_tile_lds(DWT_WHAT_DWT, true, L) && ib == 2 * k0 + c - (L - 1));
        std::vector<int64_t> X(NI);
        for (int i = 0; i < NI; ++i) {
            X.at(i) = dwt_ext(ib + i, n, mode);
            CHECK(X[i] >= -1 && X[i] < n);
        }
        for (int k = 0; k < Tk; ++k) {
            for (int m = 0; m < L; ++m) CHECK(X.at(2 * k + L - 1 - m) == dwt_ext(2 * (k0 + k) + c - m, n, mode));
            if (seen) ++seen->at(k0 + k);
        }
    }
}

// k_idwt_tile's walk: every output once, every staged coefficient inside the LDS and the one the formula names
static void walk_syn(int64_t n, int L, int mode, std::vector<unsigned char> *seen) {
    const int64_t K = dwt_coeff_len(n, L, mode), tiles = (n + DWT_TILE - 1) / DWT_TILE;
    const int shift = dwt_syn_shift(L, mode), NKmax = DWT_TILE / 2 + L / 2 + 1;
    CHECK(2 * (int64_t)NKmax * 8 == dwt_tile_lds(DWT_WHAT_IDWT, true, L));
    for (int64_t t = 0; t < tiles; ++t) {
        const int64_t i0 = t * DWT_TILE, kb = dwt_syn_first(t, L, mode);
        const int Ti = (int)(n - i0 < DWT_TILE ? n - i0 : DWT_TILE);
        const int NK = (int)(((i0 + Ti - 1 + shift) >> 1) - kb + 1);
        CHECK(NK >= 1 && NK <= NKmax && kb == ((i0 + shift) >> 1) - (L / 2 - 1));
        std::vector<int64_t> XA(NKmax, -7);
        for (int q = 0; q < NK; ++q) {
            int64_t s = kb + q;
            if (mode == DWT_PER) s = dwt_mod(s, K);
            CHECK(s >= 0 && s < K);                      // no zero is ever staged: the formula's sums stay inside 0 .. K - 1
            XA.at(q) = s;
        }
        for (int i = 0; i < Ti; ++i) {
            const int64_t tt = i0 + i + shift;
            const int p = (int)(tt & 1), k0 = (int)((tt >> 1) - kb);
            for (int j = p, q = 0; j < L; j += 2, ++q) {
                const int64_t want = mode == DWT_PER ? dwt_mod((tt >> 1) - q, K) : (tt >> 1) - q;
                CHECK(XA.at(k0 - q) == want);
            }
            if (seen) ++seen->at(i0 + i);
        }
    }
}

int main() {
    const int Ls[] = {2, 4, 8, 20, 64};
    const int64_t ns[] = {1, 2, 3, 5, 8, 17, 37, 64, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 6139, 6140};
    // the index maps: inside the array, periodic, and equal to the slow construction well past one wrap
    for (int mode = 0; mode < DWT_NMODES; ++mode)
        for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)5, (int64_t)8, (int64_t)17}) {
            const int64_t reach = 5 * n + 70;
            const std::vector<int64_t> e = extended(n, mode, reach);
            for (int64_t i = -reach; i < n + reach; ++i) CHECK(dwt_ext(i, n, mode) == e[i + reach]);
        }
    CHECK(dwt_ext(-((int64_t)1 << 40), DWT_MAX_N, DWT_SYMMETRIC) >= 0 && dwt_ext(((int64_t)1 << 40), DWT_MAX_N, DWT_REFLECT) < DWT_MAX_N);
    CHECK(dwt_mod(-1, 5) == 4 && dwt_mod(-5, 5) == 0 && dwt_mod(7, 5) == 2 && dwt_mod(-((int64_t)1 << 29), 5) == 3);

    // lengths and offsets of every level, all modes and parities; the walks of both directions
    for (int L : Ls)
        for (int mode = 0; mode < DWT_NMODES; ++mode)
            for (int64_t n : ns) {
                const int top = dwt_max_levels(n, L, mode);
                CHECK(top >= 1 && top <= DWT_MAX_LEVELS && !dwt_shape(0, n, L, mode, top, 1));
                CHECK(top == DWT_MAX_LEVELS || dwt_shape(0, n, L, mode, top + 1, 1));
                for (int levels : {1, 2, top}) {
                    if (levels > top) continue;
                    for (int what = 0; what < 2; ++what)
                        for (int form : {DWT_FORM_AUTO, DWT_FORM_TILE}) {
                            const DwtPlan p = dwt_plan_of(what, false, n, L, mode, levels, 3, form, 0);
                            CHECK(p.nent == levels + 1 && p.lv.len[0] == n && p.max_levels == top);
                            int64_t o = 0;
                            for (int e = 0; e <= levels; ++e) {
                                const int j = e == 0 ? levels : levels - e + 1;
                                CHECK(p.len[e] == p.lv.len[j] && p.off[e] == o && (e == 0 || p.lv.off[j] == o));
                                o += p.len[e];
                            }
                            CHECK(p.total == o);
                            for (int j = 1; j <= levels; ++j) {
                                const int64_t a = p.lv.len[j - 1], K = p.lv.len[j];
                                CHECK(K == (mode == DWT_PER ? (a + 1) / 2 : (a + L - 1) / 2) && K >= 1);
                                const int64_t full = mode == DWT_PER ? 2 * K : 2 * K - L + 2;      // what one synthesis level gives
                                CHECK(full == a || full == a + 1);
                                CHECK(K <= (n > L - 1 ? n : L - 1) && a + 2 * (L - 1) <= p.cap && 2 * K <= p.cap);   // both row kernels' buffers
                                if (form == DWT_FORM_TILE && j < levels) CHECK(p.buf[j & 1] >= K);
                            }
                            CHECK(p.form == (form == DWT_FORM_TILE ? DWT_FORM_TILE : DWT_FORM_ROW));
                            if (p.form == DWT_FORM_ROW) CHECK(p.lds_bytes == DWT_FILT_BYTES + 2 * p.rpw * p.cap * 4 && p.lds_bytes <= DWT_LDS_MAX && p.launches == 1 && p.workgroups == (3 + p.rpw - 1) / p.rpw);
                            else CHECK(p.launches == levels && p.passes == 1 && p.rpp == 3 && p.scratch_bytes == 3 * (p.buf[0] + p.buf[1]) * 4);
                        }
                }
                std::vector<unsigned char> ka(dwt_coeff_len(n, L, mode), 0), ks(n, 0);
                walk_ana(n, L, mode, &ka);
                walk_syn(n, L, mode, &ks);
                for (unsigned char v : ka) CHECK(v == 1);
                for (unsigned char v : ks) CHECK(v == 1);
            }
    // the largest row: the first and the last tile's arithmetic stays in 64 bits (the walks above, without the marks, would take hours:
    // the last tiles are checked by hand)
    for (int mode : {DWT_SYMMETRIC, DWT_PER}) {
        const int64_t n = DWT_MAX_N, K = dwt_coeff_len(n, 64, mode), tiles = (K + DWT_TILE - 1) / DWT_TILE;
        const int64_t ib = dwt_tile_first(tiles - 1, 64, mode);
        CHECK(ib > ((int64_t)1 << 31) - 4096 && ib + 2 * DWT_TILE + 62 > n && dwt_ext(ib + 2 * DWT_TILE + 61, n, mode) >= 0 && dwt_ext(ib + 2 * DWT_TILE + 61, n, mode) < n);
        const DwtPlan p = dwt_plan_of(DWT_WHAT_DWT, true, n, 64, mode, 31, 5, DWT_FORM_AUTO, 0);
        CHECK(p.form == DWT_FORM_TILE && !p.row_fits && p.rpp == 1 && p.passes == 5 && p.launches == 5 * 31 && p.total > n && p.lv.len[31] >= 1);
        CHECK(p.scratch_bytes == (p.buf[0] + p.buf[1]) * 8 && p.buf[1] == p.lv.len[1] && p.buf[0] == p.lv.len[2]);
    }
    // the row form's limit: two buffers of max(n, L - 1) + 2 (L - 1) elements a row, four rows up to 1024 samples
    for (int L : Ls)
        for (int cplx = 0; cplx < 2; ++cplx) {
            const int64_t el = cplx ? 8 : 4, most = (DWT_LDS_MAX - DWT_FILT_BYTES) / (2 * el) - 2 * (L - 1);
            CHECK(dwt_plan_of(0, cplx, most, L, DWT_SYMMETRIC, 1, 1, DWT_FORM_AUTO, 0).form == DWT_FORM_ROW);
            CHECK(dwt_plan_of(0, cplx, most + 1, L, DWT_SYMMETRIC, 1, 1, DWT_FORM_AUTO, 0).form == DWT_FORM_TILE);
            CHECK(!dwt_plan_of(2, cplx, most + 1, L, 0, 1, 1, DWT_FORM_ROW, 0).row_fits);
            CHECK(dwt_row_pack(1024) == 4 && dwt_row_pack(1025) == 1 && dwt_row_lds(cplx, 1024, L) == 512 + 2 * 4 * (1024 + 2 * (L - 1)) * el);
            CHECK(dwt_row_lds(cplx, 1, L) == 512 + 2 * 4 * 3 * (int64_t)(L - 1) * el);
        }
    CHECK((DWT_LDS_MAX - DWT_FILT_BYTES) / 8 - 2 * 7 == 20402);
    // the MODWT: planes, passes and the hook
    for (int64_t rows : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)257, (int64_t)DWT_MAX_N})
        for (int64_t hook : {(int64_t)0, (int64_t)2}) {
            const DwtPlan p = dwt_plan_of(DWT_WHAT_MODWT, false, 100000, 8, 0, 5, rows, DWT_FORM_AUTO, hook);
            CHECK(p.form == DWT_FORM_TILE && p.buf[0] == 100000 && p.buf[1] == 100000 && p.nent == 6 && p.off[5] == 5 * rows * 100000 && p.len[5] == 100000);
            CHECK(rows == 0 ? p.passes == 0 : (p.passes * p.rpp >= rows && (p.passes - 1) * p.rpp < rows));
            CHECK(p.rpp >= 1 && (hook == 0 || p.rpp <= hook) && (p.rpp == 1 || p.rpp * 800000 <= DWT_SCRATCH_BYTES) && p.rpp * 98 <= DWT_MAX_N);
            CHECK(p.workgroups == rows * 5 * 98 && p.launches == p.passes * 5);
        }
    // refusals
    CHECK(!dwt_shape(0, 1, 2, 0, 1, 0) && !dwt_shape(1, DWT_MAX_N, 64, 5, 31, DWT_MAX_N) && !dwt_shape(2, 5, 20, -1, 4, 1) && !dwt_shape(3, 1, 2, 0, 30, 1));
    CHECK(dwt_shape(4, 8, 2, 0, 1, 1) && dwt_shape(-1, 8, 2, 0, 1, 1) && dwt_shape(0, 8, 3, 0, 1, 1) && dwt_shape(0, 8, 0, 0, 1, 1) && dwt_shape(0, 8, 66, 0, 1, 1));
    CHECK(dwt_shape(0, 0, 2, 0, 1, 1) && dwt_shape(0, (int64_t)1 << 31, 2, 0, 1, 1) && dwt_shape(0, 8, 2, 0, 1, -1) && dwt_shape(0, 8, 2, 0, 1, (int64_t)1 << 31));
    CHECK(dwt_shape(0, 8, 2, 6, 1, 1) && dwt_shape(0, 8, 2, -1, 1, 1) && dwt_shape(0, 8, 2, 0, 0, 1) && dwt_shape(0, 8, 2, 5, 4, 1) && !dwt_shape(0, 8, 2, 5, 3, 1));
    CHECK(dwt_shape(0, 1000, 20, 2, 33, 1) && !dwt_shape(0, 1000, 20, 2, 32, 1));
    CHECK(dwt_shape(2, 8, 2, 0, 0, 1) && dwt_shape(2, 8, 2, 0, 31, 1) && dwt_shape(2, 8, 64, 0, 27, 1) && !dwt_shape(2, 8, 64, 0, 26, 1) && dwt_shape(3, 8, 6, 0, 30, 1) && !dwt_shape(3, 8, 4, 0, 30, 1));
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("dwt plan ok\n");
    return 0;
}
