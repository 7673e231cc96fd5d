/* spectral_nufft2.h -- C ABI of libspectral.so, tenth table: the non-uniform FFT of type 2, the adjoint of spectral_nufft.h's
 * transform.  The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers,
 * 0 = ok, < 0 = error with the message in sp_last_error(), which starts with the entry's name).
 */
#ifndef SPECTRAL_NUFFT2_H
#define SPECTRAL_NUFFT2_H

#include "spectral_nufft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The type-2 NUFFT: a spectrum on a uniform frequency grid evaluated at uneven times.  With e(p) = exp(2 pi i p), times t
 *      (float64 [N], shared by the rows, any order, duplicates allowed), modes F (complex64 [batch][M], rows F_ld elements apart)
 *      and sign = +1 or -1:
 *        c_r[j] = sum_m F_r[m] e( sign (f0 + m df) (t_j - t_ref) ),    j = 0 .. N - 1        out: complex64 [batch][N], rows out_ld apart
 *      f0, df, t_ref and the limits are sp_nufft1's; t, F and out follow `mem`.  The columns N .. out_ld - 1 of out are left as they
 *      are.
 *      The path is sp_nufft1's run the other way, with the same positions p = frac(-sign df tau), first cells, offsets, centre phases
 *      e(sign fc tau), kernel, fine grid of nf = next_pow2(2 M) cells and tile lists: F_r[m] divided in float64 by the kernel's
 *      transform at k = m - M / 2 is placed at cell k mod nf of a grid that is zero elsewhere; one forward complex64 transform of nf
 *      points; every sample sums the 8 cells from its first cell on, weighted with the float32 kernel values, in float32 and in the
 *      order of the cells, and the sum is multiplied by the sample's centre phase.  No factor 1 / nf.  Method error: 4e-8 of
 *      sum_m |F_r[m]| at the most; with the float32 kernel values and transform under 1e-6 (tests/nufft2_ref.py).
 *      One workgroup takes one tile of 1024 cells and a group of 4 rows, stages the tile and the 7 cells behind it in LDS and serves
 *      the samples whose first cell lies in the tile.  No atomics on data: an output depends on its own sample alone, so two calls
 *      agree bitwise and A PERMUTATION OF THE SAMPLES PERMUTES out BIT FOR BIT.
 *      Rows beyond what 256 MiB of fine grids hold go in passes (SP_NUFFT_ROWS caps the rows per pass); sp_last_passes(6) reports
 *      the passes of the last call.  A record piled into one tile is correct and slow: one workgroup per row group takes it.
 *      Refused (-1, the device is not touched, the outputs are untouched): N outside 1 .. 2^31 - 1; M outside 1 .. 2^24; nf beyond
 *      2^26; batch outside 0 .. 65535; F_ld < M; out_ld < N; t_ref, f0 or df not finite; df == 0; sign not +1 or -1; t, F or out
 *      NULL.  batch == 0 returns 0 and launches nothing.  A t or F that is not finite (or a time whose products with df and fc leave
 *      float64) is found by the preparing kernels before anything is written: SP_NUFFT_BAD_RECORD (-2).
 *
 *      sp_nufft2_plan (host only, never touches the device): out[8] = nf, the kernel width in cells, tiles, cells of a tile, rows
 *      per pass, passes, workgroups of the interpolation kernel over all passes, rows of a row group.  N does not enter the rest.
 *      < 0 for a shape sp_nufft2 refuses, or out NULL. */
int sp_nufft2(const double *t, const void *F, int64_t F_ld, int64_t N, int64_t batch, double t_ref, double f0, double df, int64_t M,
              int sign, void *out, int64_t out_ld, int mem);
int sp_nufft2_plan(int64_t N, int64_t M, int64_t batch, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
