// sub_plan.h -- the arithmetic of the data covariance matrix, the covariance least-squares fits and the pseudospectrum
// (k_subspace.hip; include/spectral_sub.h) that the host decides: how a segment is cut into tiles (the geometry of k_ar_lags:
// ar_chunk of ar_plan.h), what a segment takes of the scratch, how many segments a pass holds.  No HIP call:
// tests/sub_plan_test.cpp holds it on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ar_plan.h"

namespace sp {

#define SUB_MAX_M 64                      // the largest matrix order: what k_eigh takes, and what k_ls_chol holds in LDS
#define SUB_HALO (SUB_MAX_M - 1)          // samples k_cov_row stages in front of a stage of AR_STAGE
#define SUB_SCRATCH_BYTES ((size_t)256 << 20)  // the partial rows (and, for the fits, the matrices) of a pass
#define SUB_PSEUDO_VECS 32                // noise vectors k_pseudo stages in LDS at a time
#define SUB_WHAT_COVMAT 0
#define SUB_WHAT_LS 1

// nullptr, or why a shape is refused (the words follow the entry's name in sp_last_error); m is the matrix order (order + 1 for a fit)
inline const char *sub_shape(int what, int64_t n, int64_t m, int64_t batch, int64_t nframes) {
    if (what != SUB_WHAT_COVMAT && what != SUB_WHAT_LS) return "what must be 0 (covmat) or 1 (the least-squares fit)";
    if (what == SUB_WHAT_LS && (m < 2 || m > SUB_MAX_M)) return "order must lie in 1 .. 63";
    if (m < 2 || m > SUB_MAX_M) return "m must lie in 2 .. 64";
    if (n < 2 || n > YULE_MAX_N) return "n must lie in 2 .. 2^31 - 1";
    if (what == SUB_WHAT_LS && m - 1 > n / 2) return "order must not exceed n / 2";
    if (m > n) return "m must not exceed n";
    if (batch < 0 || batch > ((int64_t)1 << 31) - 1) return "batch must lie in 0 .. 2^31 - 1";
    if (nframes < 0 || nframes > ((int64_t)1 << 31) - 1) return "nframes must lie in 0 .. 2^31 - 1";
    if (batch > 0 && nframes > (((int64_t)1 << 40)) / batch) return "batch x nframes must not exceed 2^40 segments";
    return nullptr;
}

struct SubPlan {
    int64_t chunk, tiles;                 // samples of a tile (a multiple of AR_STAGE), tiles of a segment
    int nsub;                             // shares of a stage: a thread of k_cov_row is (column, share)
    int64_t lds_bytes;                    // of k_cov_row
    int64_t seg_bytes;                    // scratch of one segment: its tiles' partial rows, and for a fit its matrix
    int64_t spp, passes, workgroups;      // segments per pass, passes, workgroups of k_cov_row over all passes
};

inline int64_t sub_row_lds(bool cplx) {
    const int64_t el = cplx ? 16 : 8;     // the staged sample and a partial sum are float64 / complex128
    return (int64_t)(SUB_HALO + AR_STAGE) * el + 256 * el;
}

// segs_force > 0 caps the segments of a pass (test hook: SP_AR_SEGS)
inline SubPlan sub_plan_of(int what, bool cplx, int64_t n, int m, int64_t segs, int64_t segs_force) {
    SubPlan p{};
    const int64_t el = cplx ? 16 : 8;
    p.chunk = ar_chunk(n), p.tiles = (n + p.chunk - 1) / p.chunk;
    p.nsub = 256 / m;
    p.lds_bytes = sub_row_lds(cplx);
    p.seg_bytes = p.tiles * m * el + (what == SUB_WHAT_LS ? (int64_t)m * m * 16 : 0);
    int64_t fit = (int64_t)(SUB_SCRATCH_BYTES / (size_t)p.seg_bytes);
    if (fit < 1) fit = 1;
    if (fit > AR_PASS_SEGS) fit = AR_PASS_SEGS;
    if (segs_force > 0 && segs_force < fit) fit = segs_force;
    p.spp = segs < 1 ? 1 : (segs < fit ? segs : fit);
    p.passes = segs < 1 ? 0 : (segs + p.spp - 1) / p.spp;
    p.workgroups = segs < 1 ? 0 : segs * p.tiles;
    return p;
}

}   // namespace sp
