// nufft_plan.h -- the arithmetic of the type-1 NUFFT (k_nufft.hip; include/spectral_nufft.h) that the host decides, and the small
// per-sample functions host and device must agree on.  No HIP call: tests/nufft_plan_test.cpp holds it on the CPU under
// AddressSanitizer and UndefinedBehaviorSanitizer.
//
// The transform: F[m] = sum_j c_j e((f0 + m df) tau_j), m = 0 .. M - 1, as modes k = m - M / 2 around the centre frequency
// fc = f0 + (M / 2) df.  A sample lies at p = frac(-df tau) on a periodic fine grid of nf = next_pow2(2 M) cells and carries
// c_j e(fc tau_j); it is spread onto the NUFFT_W cells around nf p with the kernel phi(z) = exp(beta (sqrt(1 - z^2) - 1)),
// z = (cell - nf p) / (NUFFT_W / 2), beta = 2.30 NUFFT_W; one forward transform over the grid follows, and bin k is divided by the
// kernel's transform (NUFFT_W / 2) phi^(pi NUFFT_W k / nf), a Gauss-Legendre sum in float64.
// The spread adds 64-bit integers llrint(v 2^shift) in LDS, so that no order of the samples changes a bit: nufft_shift.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define NUFFT_HD __host__ __device__
#else
#define NUFFT_HD
#endif

namespace sp {

#define NUFFT_W 8                         // kernel width in cells
#define NUFFT_TILE 1024                   // cells of a tile: one workgroup owns one tile of one row group
#define NUFFT_RG 3                        // rows of a row group: NUFFT_RG * NUFFT_TILE * 16 bytes = 48 KiB of int64 sums in LDS
#define NUFFT_MAX_M (1 << 24)
#define NUFFT_MAX_NF ((int64_t)1 << 26)   // the longest multi-pass transform
#define NUFFT_QUAD 32                     // nodes on [0, 1]: the positive half of a 64-point Gauss-Legendre rule
#define NUFFT_BETA (2.30 * NUFFT_W)

inline int64_t nufft_nf(int64_t M) {
    int64_t nf = NUFFT_TILE;              // the floor: one tile
    while (nf < 2 * M) nf <<= 1;
    return nf;
}

struct NufftPlan {
    int64_t nf, tiles;
    int64_t rpp, passes;                  // rows per pass over the grid budget, passes over the rows
    int64_t workgroups;                   // of the spread kernel, over all passes
};
// rows per pass: what keeps grid[rows][nf] complex64 within grid_bytes, at least one; rows_force > 0 caps them (test hook)
inline NufftPlan nufft_plan_of(int64_t M, int64_t rows, size_t grid_bytes, int64_t rows_force) {
    NufftPlan p;
    p.nf = nufft_nf(M);
    p.tiles = p.nf / NUFFT_TILE;
    int64_t fit = (int64_t)(grid_bytes / (8 * (size_t)p.nf));
    if (fit < 1) fit = 1;
    if (rows_force > 0 && rows_force < fit) fit = rows_force;
    p.rpp = rows < 1 ? 1 : (rows < fit ? rows : fit);
    p.passes = rows < 1 ? 0 : (rows + p.rpp - 1) / p.rpp;
    p.workgroups = 0;
    for (int64_t r0 = 0; r0 < rows; r0 += p.rpp) {
        const int64_t nr = rows - r0 < p.rpp ? rows - r0 : p.rpp;
        p.workgroups += p.tiles * ((nr + NUFFT_RG - 1) / NUFFT_RG);
    }
    return p;
}

// The fixed-point shift of a row whose largest component magnitude is below 2^e (frexp's exponent), over N samples.  A component of
// one contribution is at most |c| phi <= 2 cmax < 2^(e + 1) in magnitude; a cell takes at most one contribution per sample, so its
// sum of llrint(v 2^shift) stays below N (2^(e + 1 + shift) + 1/2) <= 2^61 + 2^30 < 2^62 for any clustering of the samples.
NUFFT_HD inline int nufft_ceil_log2(int64_t n) {
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}
NUFFT_HD inline int nufft_shift(int e, int64_t N) { return 60 - e - nufft_ceil_log2(N); }

// frac(q tau) in [0, 1]: the product's rounding error kept by an FMA, so that a position is good to 2^-53 turns whatever |q tau|
NUFFT_HD inline double nufft_frac(double q, double tau) {
    const double p = q * tau;
    const double lo = fma(q, tau, -p);
    double r = (p - rint(p)) + lo;
    r -= floor(r);
    return r;
}

// the first of the NUFFT_W cells a sample at p touches, wrapped into 0 .. nf - 1, and the float32 offset dx in [0, 1] from the
// footprint's lower edge nf p - NUFFT_W / 2 up to it: cell l of the footprint lies at z = (dx + l - NUFFT_W / 2) / (NUFFT_W / 2)
struct NufftCell {
    int64_t i0;
    float dx;
};
NUFFT_HD inline NufftCell nufft_cell(double p, int64_t nf) {
    const double lo = p * (double)nf - 0.5 * NUFFT_W;
    const double c = ceil(lo);
    NufftCell r;
    r.dx = (float)(c - lo);                       // 1 where the rounding to float32 reaches it: the last cell then lies at z = 1
    r.i0 = (int64_t)c & (nf - 1);                 // nf is a power of two: the mask wraps a negative cell as well
    return r;
}
// the tiles of the footprint's first and last cell: a sample is listed in both where they differ
NUFFT_HD inline void nufft_tiles(int64_t i0, int64_t nf, int64_t *a, int64_t *b) {
    *a = i0 / NUFFT_TILE;
    *b = ((i0 + NUFFT_W - 1) & (nf - 1)) / NUFFT_TILE;
}

NUFFT_HD inline float nufft_phi(float z) {
    const float u = (1.f - z) * (1.f + z);
    return expf((float)NUFFT_BETA * (sqrtf(u > 0.f ? u : 0.f) - 1.f));
}

// The kernel's transform as a sum: the spectrum of the grid at mode k is that of the samples times
//   Phi(k) = (W / 2) int_-1^1 phi(z) cos(pi W k z / nf) dz = sum_q amp[q] cos(k ang[q]),
// amp[q] = W w_q phi(z_q), ang[q] = pi W z_q / nf over the NUFFT_QUAD positive nodes z_q (weights w_q) of the 64-point Gauss-Legendre rule.
struct NufftQuad {
    double amp[NUFFT_QUAD], ang[NUFFT_QUAD];
};
inline NufftQuad nufft_quad(int64_t nf) {
    NufftQuad q;
    const int n = 2 * NUFFT_QUAD;
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < NUFFT_QUAD; ++i) {
        double x = cos(pi * (i + 0.75) / (n + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = x;
            for (int k = 2; k <= n; ++k) {
                const double p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
                p0 = p1, p1 = p2;
            }
            dp = n * (x * p1 - p0) / (x * x - 1.0);
            const double dx = p1 / dp;
            x -= dx;
            if (fabs(dx) < 1e-16) break;
        }
        const double wq = 2.0 / ((1.0 - x * x) * dp * dp);
        q.amp[i] = NUFFT_W * wq * exp(NUFFT_BETA * (sqrt(1.0 - x * x) - 1.0));
        q.ang[i] = pi * NUFFT_W * x / (double)nf;
    }
    return q;
}
NUFFT_HD inline double nufft_phihat(const NufftQuad &q, int64_t k) {
    double s = 0.0;
    for (int i = 0; i < NUFFT_QUAD; ++i) s += q.amp[i] * cos((double)k * q.ang[i]);
    return s;
}

}   // namespace sp
