// beam_plan.h -- the arithmetic of the array wavenumber-frequency scan (k_beam.hip; include/spectral_array.h) that the host decides:
// what a shape is refused for, how the steering vectors of a model are cut into tiles, what a workgroup takes of the LDS, how many
// workgroups are launched and how many (model, tile) items each walks.  No HIP call: tests/beam_plan_test.cpp holds it on the CPU
// under AddressSanitizer and UndefinedBehaviorSanitizer.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BEAM_HD __host__ __device__       // what the kernel asks too
#else
#define BEAM_HD
#endif

namespace sp {

#define BEAM_MAX_M 64                     // the largest array: what k_eigh decomposes
#define BEAM_TQ 64                        // steering vectors of a tile: one per lane of a wave
#define BEAM_WAVES 8                      // waves of a workgroup: each takes BEAM_KB vectors of a stage
#define BEAM_KB 4                         // eigenvectors a lane projects its steering vector on at a time
#define BEAM_KS (BEAM_WAVES * BEAM_KB)    // eigenvectors of a stage
#define BEAM_WG (BEAM_WAVES * 64)
#define BEAM_MAX_GRID ((int64_t)1 << 16)  // workgroups of a launch; beyond it a workgroup walks several items
#define BEAM_MAX_ITEMS ((int64_t)1 << 40)
#define BEAM_BARTLETT 0
#define BEAM_CAPON 1
#define BEAM_MUSIC 2
#define BEAM_EV 3

// nullptr, or why a shape is refused (the words follow the entry's name in sp_last_error)
inline const char *beam_shape(int m, int ndim, int64_t nk, int64_t nmodels, int method, int p) {
    if (m < 2 || m > BEAM_MAX_M) return "m must lie in 2 .. 64";
    if (ndim < 1 || ndim > 3) return "ndim must lie in 1 .. 3";
    if (nk < 1 || nk > 0x7fffffff) return "nk must lie in 1 .. 2^31 - 1";
    if (method < BEAM_BARTLETT || method > BEAM_EV) return "method must be 0 (bartlett), 1 (capon), 2 (music) or 3 (ev)";
    if ((method == BEAM_MUSIC || method == BEAM_EV) && (p < 0 || p > m - 1)) return "p must lie in 0 .. m - 1";
    if (nmodels < 0) return "nmodels must not be negative";
    if (nmodels > 0 && (nk + BEAM_TQ - 1) / BEAM_TQ > BEAM_MAX_ITEMS / nmodels) return "nmodels x ceil(nk / 64) must not exceed 2^40";
    return nullptr;
}

// a table the host hands over is finite throughout
inline bool beam_finite(const double *t, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!isfinite(t[i])) return false;
    return true;
}

// the first eigenvector a method sums over: the noise subspace for MUSIC and EV, every vector otherwise
BEAM_HD inline int beam_first(int method, int p) { return method == BEAM_MUSIC || method == BEAM_EV ? p : 0; }

// LDS of a workgroup: the steering tile [m][TQ] and the stage [m][KS] in complex128, the waves' partial sums [WAVES][TQ], the weights
// padded to whole stages
inline int64_t beam_gw_len(void) { return (int64_t)(BEAM_MAX_M + BEAM_KS - 1) / BEAM_KS * BEAM_KS; }
inline int64_t beam_lds(int m) { return (int64_t)m * (BEAM_TQ + BEAM_KS) * 16 + (int64_t)BEAM_WAVES * BEAM_TQ * 8 + beam_gw_len() * 8; }

struct BeamPlan {
    int tq, ks;                           // steering vectors of a tile, eigenvectors of a stage
    int64_t tiles;                        // tiles of a model
    int64_t stages;                       // stages a tile streams the eigenvectors in
    int64_t lds_bytes;
    int64_t items, grid, per_wg;          // (model, tile) items, workgroups launched, the most items one of them walks
};

// grid_force > 0 caps the workgroups (test hook: SP_BEAM_GRID)
inline BeamPlan beam_plan_of(int m, int64_t nk, int64_t nmodels, int method, int p, int64_t grid_force) {
    BeamPlan b{};
    b.tq = BEAM_TQ, b.ks = BEAM_KS;
    b.tiles = (nk + BEAM_TQ - 1) / BEAM_TQ;
    b.stages = (m - beam_first(method, p) + BEAM_KS - 1) / BEAM_KS;
    b.lds_bytes = beam_lds(m);
    b.items = nmodels * b.tiles;
    b.grid = b.items < BEAM_MAX_GRID ? b.items : BEAM_MAX_GRID;
    if (grid_force > 0 && grid_force < b.grid) b.grid = grid_force;
    b.per_wg = b.grid > 0 ? (b.items + b.grid - 1) / b.grid : 0;
    return b;
}

}   // namespace sp
