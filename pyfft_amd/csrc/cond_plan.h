// cond_plan.h -- the arithmetic of the conditioned spectral analysis (k_cond.hip; include/spectral_mimo.h) that the host decides: what a
// shape is refused for, how the LDS of a workgroup is cut into regions, how many threads a workgroup has, how many workgroups are launched
// and how many matrices each walks.  No HIP call: tests/cond_plan_test.cpp holds it on the CPU under AddressSanitizer and
// UndefinedBehaviorSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define COND_HD __host__ __device__       // what the kernel asks too
#else
#define COND_HD
#endif

namespace sp {

#define COND_MAX_N 64                     // the largest matrix: what csd_matrix forms and k_eigh decomposes
#define COND_WANT_H 1u                    // the bits of `want`
#define COND_WANT_GC 2u
#define COND_WANT_MCOH 4u
#define COND_WANT_PIV 8u
#define COND_WANT_P 16u
#define COND_WANT_ALL 31u
#define COND_MAX_GRID ((int64_t)1 << 16)  // workgroups of a launch; beyond it a workgroup walks several matrices
#define COND_MAX_COUNT ((int64_t)1 << 40)
#define COND_LDS_MAX ((int64_t)160 * 1024)

// nullptr, or why a shape is refused (the words follow the entry's name in sp_last_error)
inline const char *cond_shape(int n, int q, int64_t count, unsigned want) {
    if (n < 1 || n > COND_MAX_N) return "n must lie in 1 .. 64";
    if (q < 0 || q > n) return "q must lie in 0 .. n";
    if (count < 0 || count > COND_MAX_COUNT) return "count must lie in 0 .. 2^40";
    if (want == 0 || (want & ~COND_WANT_ALL)) return "want must be a non-empty set of the bits 1 (H), 2 (Gc), 4 (mcoh), 8 (piv), 16 (P)";
    return nullptr;
}

// order[0 .. n - 1] is a permutation of 0 .. n - 1
inline bool cond_is_perm(const int32_t *order, int n) {
    uint64_t seen = 0;
    for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || ((seen >> order[i]) & 1)) return false;
        seen |= (uint64_t)1 << order[i];
    }
    return true;
}

// Rows of the matrix (and of the inverse factor) are `pitch` complex128 elements apart.  An odd pitch: the lanes that walk a column of L
// then read 16 B slots that are distinct modulo the 16 slots of the LDS's 256 B bank row, where a pitch of n = 64 would put all of them
// on one.
COND_HD inline int cond_pitch(int n) { return n | 1; }
// the smallest power of two >= n, as a shift: element e of a region's index space is row e >> lg, column e & ((1 << lg) - 1)
COND_HD inline int cond_lg(int n) {
    int lg = 0;
    while ((1 << lg) < n) ++lg;
    return lg;
}
// threads of a workgroup: one wave up to order 16, four up to 32, eight beyond
COND_HD inline int cond_wg(int n) { return n <= 16 ? 64 : n <= 32 ? 256 : 512; }

// LDS of a workgroup, in bytes: [A: n x pitch complex128][W: the same, only when P is wanted][the loaded diagonal: 64 float64][16 spare]
COND_HD inline int64_t cond_mat_bytes(int n) { return (int64_t)n * cond_pitch(n) * 16; }
COND_HD inline int64_t cond_off_w(int n) { return cond_mat_bytes(n); }
COND_HD inline int64_t cond_off_diag(int n, bool wantP) { return cond_mat_bytes(n) * (wantP ? 2 : 1); }
COND_HD inline int64_t cond_lds(int n, bool wantP) { return cond_off_diag(n, wantP) + COND_MAX_N * 8 + 16; }

struct CondPlan {
    int pitch, wg;
    int64_t lds_bytes;
    int raised;                           // the request is above 64 KiB: the launch goes through lds_raise
    int64_t grid, per_wg;                 // workgroups launched, the most matrices one of them walks
};

// grid_force > 0 caps the workgroups (test hook: SP_COND_GRID)
inline CondPlan cond_plan_of(int n, int64_t count, unsigned want, int64_t grid_force) {
    CondPlan p{};
    p.pitch = cond_pitch(n);
    p.wg = cond_wg(n);
    p.lds_bytes = cond_lds(n, (want & COND_WANT_P) != 0);
    p.raised = p.lds_bytes > 64 * 1024 ? 1 : 0;
    p.grid = count < COND_MAX_GRID ? count : COND_MAX_GRID;
    if (grid_force > 0 && grid_force < p.grid) p.grid = grid_force;
    p.per_wg = p.grid > 0 ? (count + p.grid - 1) / p.grid : 0;
    return p;
}

}   // namespace sp
