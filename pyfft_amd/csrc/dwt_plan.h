// dwt_plan.h -- the arithmetic of the discrete wavelet transforms (k_dwt.hip; include/spectral_dwt.h) that the host decides, and the
// index maps both sides share: the extension modes as maps of an index, the length and offset of every level, which of the two
// kernel forms a call takes, what the row form takes of the LDS, how a level is cut into tiles, what the approximations between the
// levels take of the scratch and how many rows a pass holds.  No HIP call: tests/dwt_plan_test.cpp holds it on the CPU under
// AddressSanitizer and UndefinedBehaviorSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DWT_HD __host__ __device__
#else
#define DWT_HD
#endif

namespace sp {

#define DWT_MAX_L 64                         // the longest filter
#define DWT_MAX_LEVELS 32                    // the deepest pyramid (a row of 2^31 - 1 samples has one coefficient at level 31)
#define DWT_MODWT_MAX_LEVELS 30
#define DWT_TILE 1024                        // outputs of a tile of the tile form: four per thread
#define DWT_ROW_PACK 4                       // rows a workgroup of the row form shares where a row is short
#define DWT_ROW_PACK_N 1024                  // ... that is, up to this many samples
#define DWT_LDS_MAX ((int64_t)160 * 1024)    // = SP_LDS_MAX (launch.h asserts it)
#define DWT_SCRATCH_BYTES ((int64_t)512 << 20)   // the approximations between the levels of a pass of the tile form
#define DWT_MAX_N 0x7fffffff
#define DWT_FILT_BYTES (2 * DWT_MAX_L * 4)        // the two filters in front of the row form's buffers: in the dynamic LDS, since static LDS beside a raised
                                              // limit is refused (the decimated analysis reads its taps as scalars and leaves the region unused)

enum { DWT_ZERO = 0, DWT_CONSTANT = 1, DWT_SYMMETRIC = 2, DWT_REFLECT = 3, DWT_PERIODIC = 4, DWT_PER = 5, DWT_NMODES = 6 };
enum { DWT_WHAT_DWT = 0, DWT_WHAT_IDWT = 1, DWT_WHAT_MODWT = 2, DWT_WHAT_IMODWT = 3 };
enum { DWT_FORM_AUTO = 0, DWT_FORM_ROW = 1, DWT_FORM_TILE = 2 };

// i mod n in 0 .. n - 1 for any i
DWT_HD inline int64_t dwt_mod(int64_t i, int64_t n) {
    const int64_t r = i % n;
    return r < 0 ? r + n : r;
}

// the extension of an array of n samples as a map of the index: where sample i of the extended array is read, or -1 for a zero
DWT_HD inline int64_t dwt_ext(int64_t i, int64_t n, int mode) {
    if (i >= 0 && i < n) return i;
    switch (mode) {
    case DWT_ZERO: return -1;
    case DWT_CONSTANT: return i < 0 ? 0 : n - 1;
    case DWT_SYMMETRIC: {
        const int64_t r = dwt_mod(i, 2 * n);
        return r < n ? r : 2 * n - 1 - r;
    }
    case DWT_REFLECT: {
        if (n == 1) return 0;
        const int64_t P = 2 * n - 2, r = dwt_mod(i, P);
        return r < n ? r : P - r;
    }
    case DWT_PERIODIC: return dwt_mod(i, n);
    default: {                               // periodization: an odd length repeats its last sample first
        const int64_t r = dwt_mod(i, n + (n & 1));
        return r < n ? r : n - 1;
    }
    }
}

// coefficients of one analysis level of n samples, and the offset c of cA[k] = sum_m lo[m] xe[2k + c - m]
DWT_HD inline int64_t dwt_coeff_len(int64_t n, int L, int mode) { return mode == DWT_PER ? (n + 1) / 2 : (n + L - 1) / 2; }
DWT_HD inline int dwt_center(int L, int mode) { return mode == DWT_PER ? L / 2 : 1; }
// the shift t = i + shift of one synthesis level: output i meets the taps j = (t & 1) + 2q at the coefficients (t >> 1) - q
DWT_HD inline int dwt_syn_shift(int L, int mode) { return mode == DWT_PER ? L / 2 - 1 : L - 2; }

// the deepest level: the one at which a row has one coefficient, DWT_MAX_LEVELS at the most
inline int dwt_max_levels(int64_t n, int L, int mode) {
    int j = 0;
    while (j < DWT_MAX_LEVELS) {
        n = dwt_coeff_len(n, L, mode);
        ++j;
        if (n <= 1) break;
    }
    return j;
}

// the filters as the kernels take them (float32), and the levels of a row form's call
struct DwtFilt {
    float lo[DWT_MAX_L], hi[DWT_MAX_L];
    int L;
};
struct DwtLv {
    int64_t off[DWT_MAX_LEVELS + 1];         // off[j], j = 1 .. levels: where cD_j starts in a row of the pyramid
    int len[DWT_MAX_LEVELS + 1];             // len[j], j = 0 .. levels: samples of the approximation of level j (len[0] = n)
};

// nullptr, or why a shape is refused (the words follow the entry's name in sp_last_error)
inline const char *dwt_shape(int what, int64_t n, int L, int mode, int levels, int64_t batch) {
    if (what < DWT_WHAT_DWT || what > DWT_WHAT_IMODWT) return "what must be 0 (dwt), 1 (idwt), 2 (modwt) or 3 (imodwt)";
    if (L < 2 || L > DWT_MAX_L || (L & 1)) return "the filter length L must be even and lie in 2 .. 64";
    if (n < 1 || n > DWT_MAX_N) return "n must lie in 1 .. 2^31 - 1";
    if (batch < 0 || batch > DWT_MAX_N) return "batch must lie in 0 .. 2^31 - 1";
    if (what >= DWT_WHAT_MODWT) {
        if (levels < 1 || levels > DWT_MODWT_MAX_LEVELS) return "levels must lie in 1 .. 30";
        if (((int64_t)1 << (levels - 1)) * (L - 1) >= ((int64_t)1 << 31)) return "levels: the dilated filter 2^(levels-1) (L - 1) must stay below 2^31";
        return nullptr;
    }
    if (mode < 0 || mode >= DWT_NMODES) return "mode must be 0 (zero), 1 (constant), 2 (symmetric), 3 (reflect), 4 (periodic) or 5 (periodization)";
    if (levels < 1) return "levels must be at least 1";
    if (levels > dwt_max_levels(n, L, mode)) return "levels reach beyond the level at which a row has one coefficient";
    return nullptr;
}

struct DwtPlan {
    int form;                                // DWT_FORM_ROW or DWT_FORM_TILE
    int rpw;                                 // rows of a workgroup (row form)
    int64_t cap;                             // elements of one of the two LDS buffers of a row (row form)
    int64_t tile;                            // outputs of a tile (tile form)
    int64_t lds_bytes, workgroups, launches, passes, scratch_bytes, rpp;
    int64_t buf[2];                          // elements of a row in the two scratch buffers (tile form)
    int max_levels, nent;                    // entries of the output: levels + 1
    int64_t len[DWT_MAX_LEVELS + 1], off[DWT_MAX_LEVELS + 1];   // of every entry, in the order of the output
    int64_t total;                           // elements of a row of the pyramid (MODWT: of a plane's row, n)
    DwtLv lv;
    bool row_fits;
};

inline int dwt_row_pack(int64_t n) { return n <= DWT_ROW_PACK_N ? DWT_ROW_PACK : 1; }
// one LDS buffer of a row holds the longest level and a halo of L - 1 on both sides
inline int64_t dwt_row_cap(int64_t n, int L) { return (n > L - 1 ? n : L - 1) + 2 * (int64_t)(L - 1); }
inline int64_t dwt_row_lds(bool cplx, int64_t n, int L) { return DWT_FILT_BYTES + 2 * dwt_row_pack(n) * dwt_row_cap(n, L) * (cplx ? 8 : 4); }
// LDS of a tile: the staged span of the analysis, both coefficient spans of the synthesis, nothing for the MODWT (it reads through L2)
inline int64_t dwt_tile_lds(int what, bool cplx, int L) {
    const int64_t el = cplx ? 8 : 4;
    if (what == DWT_WHAT_DWT) return (2 * (int64_t)DWT_TILE + L - 2) * el;
    if (what == DWT_WHAT_IDWT) return 2 * ((int64_t)DWT_TILE / 2 + L / 2 + 1) * el;
    return 0;
}

// the shape must have passed dwt_shape; rows_force > 0 caps the rows of a pass (test hook: SP_DWT_ROWS)
inline DwtPlan dwt_plan_of(int what, bool cplx, int64_t n, int L, int mode, int levels, int64_t batch, int form, int64_t rows_force) {
    DwtPlan p{};
    const int64_t el = cplx ? 8 : 4;
    const bool mo = what >= DWT_WHAT_MODWT;
    p.max_levels = mo ? DWT_MODWT_MAX_LEVELS : dwt_max_levels(n, L, mode);
    p.nent = levels + 1;
    p.lv.len[0] = (int)n;
    for (int j = 1; j <= levels; ++j) p.lv.len[j] = mo ? (int)n : (int)dwt_coeff_len(p.lv.len[j - 1], L, mode);
    if (mo) {
        for (int e = 0; e <= levels; ++e) p.len[e] = n, p.off[e] = (int64_t)e * batch * n;
        p.total = n;
    } else {
        int64_t o = 0;
        for (int e = 0; e <= levels; ++e) {                   // cA_J, cD_J, .., cD_1
            const int j = e == 0 ? levels : levels - e + 1;
            p.len[e] = p.lv.len[j], p.off[e] = o;
            if (e > 0) p.lv.off[j] = o;
            o += p.len[e];
        }
        p.total = o;
    }
    p.rpw = dwt_row_pack(n), p.cap = dwt_row_cap(n, L);
    p.row_fits = dwt_row_lds(cplx, n, L) <= DWT_LDS_MAX;
    p.form = form == DWT_FORM_TILE ? DWT_FORM_TILE : (p.row_fits ? DWT_FORM_ROW : DWT_FORM_TILE);
    p.tile = DWT_TILE;
    if (p.form == DWT_FORM_ROW) {
        p.lds_bytes = dwt_row_lds(cplx, n, L);
        p.workgroups = (batch + p.rpw - 1) / p.rpw;
        p.launches = batch > 0 ? 1 : 0, p.passes = batch > 0 ? 1 : 0, p.rpp = batch > 0 ? batch : 1;
        return p;
    }
    p.lds_bytes = dwt_tile_lds(what, cplx, L);
    // the approximation of level j lives in buffer j & 1 (the first level reads the caller's rows, the last writes the caller's)
    int64_t tiles = 0, most = 1;
    for (int j = 1; j <= levels; ++j) {
        const int64_t outs = what == DWT_WHAT_IDWT ? p.lv.len[j - 1] : p.lv.len[j], t = (outs + DWT_TILE - 1) / DWT_TILE;
        tiles += t;
        if (t > most) most = t;
        if (j < levels && p.lv.len[j] > p.buf[j & 1]) p.buf[j & 1] = p.lv.len[j];
    }
    const int64_t row_bytes = (p.buf[0] + p.buf[1]) * el;
    int64_t fit = row_bytes > 0 ? DWT_SCRATCH_BYTES / row_bytes : DWT_MAX_N;
    if (fit < 1) fit = 1;
    if (fit > DWT_MAX_N / most) fit = DWT_MAX_N / most;       // rows x tiles of a launch stay below 2^31
    if (rows_force > 0 && rows_force < fit) fit = rows_force;
    p.rpp = batch < 1 ? 1 : (batch < fit ? batch : fit);
    p.passes = batch < 1 ? 0 : (batch + p.rpp - 1) / p.rpp;
    p.launches = p.passes * levels;
    p.workgroups = batch < 1 ? 0 : batch * tiles;
    p.scratch_bytes = batch < 1 ? 0 : p.rpp * row_bytes;
    return p;
}

// the first sample a tile of the analysis stages (may be negative), in 64 bits: tile t of a level with offset c
inline int64_t dwt_tile_first(int64_t t, int L, int mode) { return 2 * t * (int64_t)DWT_TILE + dwt_center(L, mode) - (L - 1); }
// the first coefficient a tile of the synthesis stages (may be negative for periodization)
inline int64_t dwt_syn_first(int64_t t, int L, int mode) { return ((t * (int64_t)DWT_TILE + dwt_syn_shift(L, mode)) >> 1) - (L / 2 - 1); }

}   // namespace sp
