/* spectral_nufft.h -- C ABI of libspectral.so, ninth table: the non-uniform FFT of type 1 and the Lomb-Scargle sums on a uniform
 * frequency grid built on it.  The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device
 * pointers, 0 = ok, < 0 = error with the message in sp_last_error(), which starts with the entry's name).
 */
#ifndef SPECTRAL_NUFFT_H
#define SPECTRAL_NUFFT_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_NUFFT_BAD_RECORD (-2)

/* ---- The type-1 NUFFT: the spectrum of an unevenly sampled complex record on a uniform frequency grid.  With e(p) = exp(2 pi i p),
 *      times t (float64 [N], shared by the rows, any order, duplicates allowed), strengths c (complex64 [batch][N], rows c_ld
 *      elements apart) and sign = +1 or -1:
 *        F_r[m] = sum_j c_r[j] e( sign (f0 + m df) (t_j - t_ref) ),    m = 0 .. M - 1        out: complex64 [batch][M]
 *      f0 is any finite float64, df finite and not zero; the plain "integer modes" transform is df = 1, f0 = k0.  t, c and out follow
 *      `mem`.
 *      The path (Dutt & Rokhlin 1993; Greengard & Lee 2004; the kernel of Barnett, Magland & af Klinteberg 2019): the transform runs
 *      over the modes k = m - M / 2 around fc = f0 + (M / 2) df.  Per sample, in float64, the position p = frac(-sign df tau) (the
 *      product's rounding error kept by an FMA) on a periodic grid of nf = next_pow2(2 M) cells (1024 at least) and the phase
 *      e(sign fc tau), rounded to float32 and multiplied onto the strength; the product is spread onto the 8 cells around nf p with
 *      phi(z) = exp(beta (sqrt(1 - z^2) - 1)), beta = 18.4, evaluated in float32; one forward complex64 transform of nf points; bin k
 *      divided by the kernel's transform, a 64-point Gauss-Legendre sum in float64.  Method error: 4e-8 of sum_j |c_r[j]| at the most
 *      (one sample), under 1e-8 for records of hundreds of samples; with the float32 kernel values and transform about 1e-7.
 *      The spread adds 64-bit integers llrint(v 2^shift_r) in LDS, the shift taken from the row's largest component and N so that no
 *      sum reaches 2^62 however the samples cluster; every grid cell is written once by the workgroup that owns its tile.  No float
 *      atomics and no global atomics on data: two calls agree bitwise, and A PERMUTATION OF THE SAMPLES CHANGES NO BIT of out.
 *      Rows beyond what 256 MiB of fine grids hold go in passes (SP_NUFFT_ROWS caps the rows per pass); sp_last_passes(6) reports
 *      the passes of the last call.  A record piled into one tile of 1024 cells is correct and slow: one workgroup takes it.
 *      Refused (-1, the device is not touched, the outputs are untouched): N outside 1 .. 2^31 - 1; M outside 1 .. 2^24; nf beyond
 *      2^26; batch outside 0 .. 65535; c_ld < N; t_ref, f0 or df not finite; df == 0; sign not +1 or -1; t, c or out NULL.
 *      batch == 0 returns 0 and launches nothing.  A t or c that is not finite (or a time whose products with df and fc leave
 *      float64) is found by the preparing kernels before anything is written: SP_NUFFT_BAD_RECORD (-2).
 *
 *      sp_lomb_sums_grid: exactly the outputs and meaning of sp_lomb_sums (spectral_uneven.h) for f[m] = f0 + m df -- float64 common
 *      [M][4] = C, S, C2, S2; rows [batch][M][2] = YC', YS'; totals [1 + 2 batch]; sp_lomb_finish takes them unchanged -- from three
 *      transforms of the record sp_lomb_sums prepares (the same kernel, so the totals are bitwise the same): A1 and the B_r are 1 +
 *      batch real rows w32, wy32_r under one set of positions, A2 is w32 at (2 f0, 2 df) on the same grid length.  They differ from
 *      sp_lomb_sums' by rounding only (tests/nufft_ref.py).  batch == 0 (y, mean, rows unused) gives the spectral window alone.
 *      mean: HOST float64 [batch] or NULL; wnorm as in sp_lomb_sums.  A permutation of the samples changes no bit of common and rows
 *      where the weights are equal or wnorm is given (w32 depends on the weight sum, which is added in the order of the samples;
 *      so are the totals).  Refused as above, with y_ld for c_ld, a mean or wnorm that is not finite, and common, totals or (batch >
 *      0) rows NULL; what the record must not hold is sp_lomb_sums': -2.
 *
 *      sp_nufft1_plan (host only, never touches the device): out[8] = nf, the kernel width in cells, tiles, cells of a tile, rows
 *      per pass, passes, workgroups of the spread kernel over all passes, and the N M from which ls_periodogram's method="auto"
 *      takes the fast path.  N does not enter the rest.  < 0 for a shape sp_nufft1 refuses, or out NULL. */
int sp_nufft1(const double *t, const void *c, int64_t c_ld, int64_t N, int64_t batch, double t_ref, double f0, double df, int64_t M,
              int sign, void *out, int mem);
int sp_lomb_sums_grid(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, double wnorm,
                      double f0, double df, int64_t M, const double *mean, double *common, double *rows, double *totals, int mem);
int sp_nufft1_plan(int64_t N, int64_t M, int64_t batch, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
