// ar_plan.h -- the arithmetic of the autoregressive fits (k_burg.hip; include/spectral_ar.h) that the host decides: which form of
// k_burg a segment length takes, how a Yule-Walker segment is cut into tiles, how many segments a pass holds.  No HIP call:
// tests/ar_plan_test.cpp holds it on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer.
//
// k_burg<cplx, SPL, NW>: a segment of n samples lies in the last n of 64 NW SPL slots, SPL consecutive slots to a lane, NW waves to a
// segment.  NW == 1 is the wave form (BURG_WAVE_SEGS segments to a workgroup, no workgroup barrier), NW > 1 the workgroup form.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sp {

#define AR_MAX_ORDER 256
#define BURG_MAX_N 16384
#define BURG_WAVE_MAX 1024                // the longest segment of the wave form: 64 lanes x 16 samples
#define BURG_WAVE_SEGS 4                  // segments (waves) of a workgroup of the wave form
#define YULE_MAX_N ((int64_t)2147483647)
#define AR_STAGE 2048                     // samples k_ar_lags stages in LDS at a time, behind AR_MAX_ORDER samples of halo
#define AR_MAX_TILES 1024                 // tiles of one Yule-Walker segment at the most
#define AR_PASS_SEGS ((int64_t)1 << 20)   // segments of a pass at the most
#define AR_SCRATCH_BYTES ((size_t)256 << 20)  // per-tile partial lags of a pass
#define AR_METHOD_BURG 0
#define AR_METHOD_YULE 1
#define AR_FORM_WAVE 0
#define AR_FORM_WG 1
#define AR_FORM_LAGS 2

// nullptr, or why a fit is refused (the words follow the entry's name in sp_last_error)
inline const char *ar_shape(int method, int64_t n, int64_t order, int64_t batch, int64_t nframes) {
    if (method != AR_METHOD_BURG && method != AR_METHOD_YULE) return "method must be 0 (Burg) or 1 (Yule-Walker)";
    if (order < 1 || order > AR_MAX_ORDER) return "order must lie in 1 .. 256";
    if (n < 2 || n > YULE_MAX_N) return "n must lie in 2 .. 2^31 - 1";
    if (method == AR_METHOD_BURG && n > BURG_MAX_N) return "n must not exceed 16384 for a Burg fit";
    if (order > n / 2) return "order must not exceed n / 2";
    if (batch < 0 || batch > ((int64_t)1 << 31) - 1) return "batch must lie in 0 .. 2^31 - 1";
    if (nframes < 0 || nframes > ((int64_t)1 << 31) - 1) return "nframes must lie in 0 .. 2^31 - 1";
    if (batch > 0 && nframes > (((int64_t)1 << 40)) / batch) return "batch x nframes must not exceed 2^40 segments";
    return nullptr;
}

struct ArPlan {
    int form;                             // AR_FORM_*
    int spl, nw;                          // k_burg: samples per lane, waves per segment (0 for Yule-Walker)
    int segs_per_wg, threads;
    int64_t lds_bytes;
    int64_t chunk, tiles;                 // Yule-Walker: samples of a tile (a multiple of AR_STAGE), tiles of a segment (1, 1 for Burg)
    int64_t spp, passes, workgroups;      // segments per pass, passes, workgroups of the main kernel over all passes
};

// form_force: 0 by length, 1 the wave form where it can (n <= BURG_WAVE_MAX), 2 the workgroup form
inline void burg_form(int64_t n, int form_force, int *spl, int *nw) {
    if (n <= BURG_WAVE_MAX && form_force != 2) {
        int s = 1;
        while (64 * s < n) s <<= 1;
        *spl = s, *nw = 1;
    } else if (n <= 2048) *spl = 8, *nw = 4;
    else if (n <= 4096) *spl = 16, *nw = 4;
    else if (n <= 8192) *spl = 16, *nw = 8;
    else *spl = 16, *nw = 16;
}

inline int64_t ar_chunk(int64_t n) {
    int64_t per = (n + AR_MAX_TILES - 1) / AR_MAX_TILES;
    int64_t c = (per + AR_STAGE - 1) / AR_STAGE * AR_STAGE;
    return c < AR_STAGE ? AR_STAGE : c;
}

// segs_force > 0 caps the segments of a pass (test hook)
inline ArPlan ar_plan_of(int method, bool cplx, int64_t n, int order, int64_t segs, int form_force, int64_t segs_force) {
    ArPlan p{};
    const int64_t el = cplx ? 16 : 8;     // bytes of a float64 coefficient
    int64_t fit = AR_PASS_SEGS;
    if (method == AR_METHOD_BURG) {
        burg_form(n, form_force, &p.spl, &p.nw);
        p.form = p.nw == 1 ? AR_FORM_WAVE : AR_FORM_WG;
        p.segs_per_wg = p.nw == 1 ? BURG_WAVE_SEGS : 1;
        p.threads = p.nw == 1 ? 64 * BURG_WAVE_SEGS : 64 * p.nw;
        // two coefficient buffers of `order` entries per segment; the workgroup form adds two sets of reduction slots (4 doubles a wave) and boundary samples
        p.lds_bytes = (int64_t)p.segs_per_wg * 2 * order * el + (p.nw > 1 ? 2 * p.nw * (4 * 8 + 2 * el / 2) : 0);
        p.chunk = ar_chunk(n), p.tiles = (n + p.chunk - 1) / p.chunk;
    } else {
        p.form = AR_FORM_LAGS;
        p.segs_per_wg = 1, p.threads = 256;
        p.chunk = ar_chunk(n), p.tiles = (n + p.chunk - 1) / p.chunk;
        p.lds_bytes = (int64_t)(AR_STAGE + AR_MAX_ORDER) * (el / 2) + 2 * AR_MAX_ORDER * el;
        const int64_t per_seg = p.tiles * (order + 1) * el;
        fit = (int64_t)(AR_SCRATCH_BYTES / (size_t)per_seg);
        if (fit < 1) fit = 1;
        if (fit > AR_PASS_SEGS) fit = AR_PASS_SEGS;
    }
    if (segs_force > 0 && segs_force < fit) fit = segs_force;
    p.spp = segs < 1 ? 1 : (segs < fit ? segs : fit);
    p.passes = segs < 1 ? 0 : (segs + p.spp - 1) / p.spp;
    p.workgroups = 0;
    for (int64_t s0 = 0; s0 < segs; s0 += p.spp) {
        const int64_t ns = segs - s0 < p.spp ? segs - s0 : p.spp;
        p.workgroups += method == AR_METHOD_BURG ? (ns + p.segs_per_wg - 1) / p.segs_per_wg : ns * p.tiles;
    }
    return p;
}

}   // namespace sp
