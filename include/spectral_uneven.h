/* spectral_uneven.h -- C ABI of libspectral.so, sixth table: spectra of unevenly sampled records.  The conventions are those of
 * spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST pointers,
 * 0 = ok, < 0 = error with the message in sp_last_error()).
 */
#ifndef SPECTRAL_UNEVEN_H
#define SPECTRAL_UNEVEN_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_LOMB_BAD_RECORD (-2)

/* ---- The generalised Lomb-Scargle periodogram (Lomb 1976; Scargle 1982; Zechmeister & Kuerster 2009), as scipy.signal.lombscargle
 *      of scipy 1.15 defines it, with all its options.
 *      t (float64 [N]) are the sample times, shared by the rows; w (float64 [N], NULL = equal weights) non-negative weights; y
 *      (float32 [batch][N], rows y_ld samples apart) the values; f (HOST float64 [M]) frequencies in cycles per unit of t; mean
 *      (HOST float64 [batch], NULL = zeros) an offset m_r per row.  t, w, y and the outputs follow `mem`.
 *      With e(p) = exp(2 pi i p), phi = f (t - t_ref), wn = w / sum w, d_r = y_r - m_r, w32 = float32(wn) and
 *      wy32_r = float32(wn d_r) (the product formed in float64), the device takes per frequency, in one pass over the samples,
 *        A1 = sum w32 e(phi) = C + iS     A2 = sum w32 e(2 phi) = C2 + iS2     B_r = sum wy32_r e(phi) = YC' + iYS'
 *      and once per call W = sum w32, Y'_r = sum wy32_r, YY'_r = sum wy32_r d_r.  All that scipy's body computes follows from
 *      these in float64 after a division by W: its second pass at the offset tau is a rotation of the same sums.  m_r only
 *      conditions the float32 products -- the result is that of y itself (YC = YC' + m C, Y = Y' + m W, YY = YY' + 2 m Y' + m^2 W);
 *      pass the row's mean.  The phase f (t - t_ref) is a float64 product reduced by p - rint(p) in float64 and rounded to a
 *      float32 turn, so a far time origin costs nothing once t_ref is near the record; sums run in float32 over sub-runs of 256
 *      samples and in float64 across them.
 *      normalize: 0 "power" (scipy's default, P N / 4), 1 "normalize" (0 .. 1), 2 "amplitude" (complex: (a + ib) e^{i tau}, referred
 *      to the origin of t itself whatever t_ref is).  floating_mean != 0 fits a constant beside the sinusoid.
 *      P: float32 [batch][M], complex64 for normalize = 2.
 *      No atomics: two calls agree bitwise.  The frequency list is cut into passes so that the partial sums of a pass stay within
 *      256 MiB (SP_LOMB_FREQS caps the frequencies per pass); sp_last_passes(3) reports the passes of the last call.  A record is
 *      dealt to sample runs where the frequencies alone do not fill the device (SP_LOMB_SPLIT sets the runs).
 *      Refused (< 0, sp_last_error() starts with the entry's name and names the argument, the device is not touched, the outputs
 *      are untouched): N < 1 or >= 2^31; M outside 1 .. 2^24; batch outside 0 .. 65535; y_ld < N; an f, t_ref or mean that is not
 *      finite; normalize outside 0 .. 2; t, f, P or (with batch > 0) y NULL.  batch == 0 returns 0 and launches nothing.
 *      A non-finite t or y, a weight that is negative or not finite, and a weight sum that is not positive are found by the
 *      kernel that prepares the record: the call then returns SP_LOMB_BAD_RECORD (-2; every other error is -1) with no output
 *      written and the message in sp_last_error().
 *
 *      sp_lomb_sums writes the sums themselves, float64, as they stand before the division by W: common [M][4] = C, S, C2, S2;
 *      rows [batch][M][2] = YC', YS'; totals [1 + 2 batch] = W, then (Y'_r, YY'_r) row by row.  They are bitwise the sums sp_lomb
 *      hands its own finish step, so sp_lomb_finish of them reproduces sp_lomb bitwise.  batch == 0 (y, mean and rows unused)
 *      gives the sums of the spectral window alone.  wnorm > 0 divides the weights by wnorm in place of their own sum: the sums of
 *      the parts of a record cut anywhere, or dealt out sample by sample, then add up to the whole's.  THE CALLER must give every
 *      part the same m_r, the same t_ref and the same wnorm (the whole record's weight sum; N of the whole for equal weights).
 *      sp_lomb_finish produces P from such sums (N: the samples of the whole record, which only normalize = 0 uses).
 *      sp_lomb_plan (host only, never touches the device): out[5] = rows per group, frequencies per pass, passes, sample runs,
 *      workgroups of the sums kernel over all passes.  The CU count is the device's once the library is initialised and 256
 *      before.  < 0 for a shape sp_lomb refuses, or out NULL. */
int sp_lomb(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, const double *f,
            int64_t M, const double *mean, int floating_mean, int normalize, void *P, int mem);
int sp_lomb_sums(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, double wnorm,
                 const double *f, int64_t M, const double *mean, double *common, double *rows, double *totals, int mem);
int sp_lomb_finish(const double *common, const double *rows, const double *totals, int64_t N, int64_t batch, double t_ref,
                   const double *f, int64_t M, const double *mean, int floating_mean, int normalize, void *P, int mem);
int sp_lomb_plan(int64_t N, int64_t M, int64_t batch, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
