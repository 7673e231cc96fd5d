/* spectral_ext.h -- C ABI of libspectral.so, second table: the entries added after the set of include/spectral.h was recorded in the
 * engine trace.  The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers,
 * small parameter tables always HOST pointers, 0 = ok, < 0 = error with the message in sp_last_error()); its constants (SP_DTYPE_*,
 * SP_CWT_MORLET, SP_CWT_PAUL) are used here.
 */
#ifndef SPECTRAL_EXT_H
#define SPECTRAL_EXT_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Cross-wavelet spectra and wavelet coherence (Torrence & Webster 1999; what pycwt.xwt and pycwt.wct give) on the overlap-save
 *      frames of sp_cwt.  For every row of a batch and every scale s' (in samples), with Wx and Wy the transforms sp_cwt defines:
 *        Wxy[s][n] = Wx[s][n] conj(Wy[s][n])                                        the cross-wavelet transform (no normalisation)
 *        a, b, c   = |Wx|^2 / s', |Wy|^2 / s', Wxy / s' for 0 <= n < nsig, zero outside the row
 *        A_t, B_t, C_t = a, b, c convolved along n (linearly, nothing wraps) with the kernel whose DFT is exp(-(s' w_k)^2 / 2), w_k the
 *                    signed bin frequency: a unit-gain Gaussian of standard deviation s' samples (pycwt's Morlet.smooth)
 *        A, B, C   = A_t, B_t, C_t summed over neighbouring scales: scipy.signal.convolve2d(., taps[:, None], 'same'); rows outside
 *                    the scale set count as zero
 *        R2 = |C|^2 / (A B),  phase = atan2(Im C, Re C);  both 0 where A B == 0.
 *      sp_wct_time: frames of L samples, L a power of two in 256 .. 8192, margin M = Mw + Mg on either side (Mw: the reach of the
 *      wavelets g_s, Mg: that of the Gaussians; the caller chooses both so that what lies beyond is negligible for every scale of the
 *      call), hop = L - 2 M >= L / 4.  Per frame x and y are read once and transformed; per scale two filtered inverse transforms,
 *      and for the coherence four more (forward, Gaussian, inverse for a + i b and for c).  x, y: rows of nsig samples of ONE dtype
 *      (float32 or complex64), row strides x_ld, y_ld >= nsig; scales: HOST float64 [nscales].  Exactly one output:
 *        T     float32   [batch][nscales][nsig][4] = (A_t, B_t, Re C_t, Im C_t), 16-byte aligned; SP_CWT_MORLET only (the smoothing
 *              operator is Morlet's)
 *        Wxy   complex64 [batch][nscales][nsig]; Mg must be 0; SP_CWT_MORLET or SP_CWT_PAUL
 *      No atomics, a fixed order of operations: two calls agree bitwise, whatever the chunking of the scales.  x, y and the output
 *      follow `mem`; device-resident x and y need only their natural alignment.
 *      Refused (< 0, sp_last_error() names sp_wct_time and the argument, the device is not touched, the outputs are untouched): L not
 *      a power of two in 256 .. 8192; Mw < 0, Mg < 0, 2 (Mw + Mg) >= L or hop < L / 4; nscales < 1 or > 65535; a scale that is not
 *      positive or not finite; an unknown family, SP_CWT_PAUL with T, or a parameter outside its range; an unknown dtype; nsig < 1,
 *      batch < 0, batch > 65535, x_ld or y_ld < nsig; both or neither of T and Wxy; Wxy with Mg != 0; T not 16-byte aligned; x, y or
 *      scales NULL.  batch == 0 returns 0 and launches nothing.
 *      sp_wct_scale: T as sp_wct_time leaves it (rows of any origin may be mixed) -> R2, phase float32 [batch][nscales][nsig] and, all
 *      three or none, A, B float32 and C complex64 of the same shape.  taps: HOST float32 [ntaps]; row s - ntaps / 2 + j takes
 *      taps[ntaps - 1 - j], the rows are added in ascending order.  Refused: nscales < 1 or > 65535, nsig < 1, batch < 0 or > 65535,
 *      ntaps < 1 or > 4096, taps that are not finite, T not 16-byte aligned, T, taps, R2 or phase NULL, some but not all of A, B, C.
 *      sp_wct_plan (host only, never touches the device; xwt != 0: the plan of a Wxy call): out[5] = hop, frames per row, scales per
 *      workgroup (as few as bring the grid to about four workgroups per CU), workgroups launched, LDS bytes of a workgroup.  The CU
 *      count is the device's once the library is initialised and 256 before.  < 0 for a shape sp_wct_time refuses, or out NULL. */
int sp_wct_time(const void *x, int64_t x_ld, const void *y, int64_t y_ld, int dtype, int64_t nsig, int64_t batch, const double *scales,
                int nscales, int family, double p0, int L, int Mw, int Mg, void *T, void *Wxy, int mem);
int sp_wct_scale(const void *T, int64_t nsig, int nscales, int64_t batch, const float *taps, int ntaps, float *R2, float *phase, float *A,
                 float *B, void *C, int mem);
int sp_wct_plan(int64_t nsig, int nscales, int64_t batch, int L, int Mw, int Mg, int xwt, int64_t out[5]);

/* ---- Loop passes of the last call (for the tests of the host loops; never touches the device).  The library cuts long work into
 *      chunks of frames (segments beyond one workgroup transform: sp_welch_psd, sp_welch_csd, sp_stft, sp_stft_cog, sp_zoom_welch;
 *      sp_csd_matrix and sp_bispectrum at every length) and batches of long transforms into slices of rows (sp_fft_c2c, sp_czt and
 *      every transform inside a frame chunk).  which = 0: the passes the outermost frame-chunk loop of the last API call made;
 *      which = 1: the most slice passes one batch of long transforms made inside it; which = 2: the passes sp_cyclic
 *      (spectral_cyclo.h) made over its list of cycle frequencies; which = 3: the passes sp_lomb and sp_lomb_sums
 *      (spectral_uneven.h) made over their list of frequencies; which = 4: the most launches the row groups of one such pass
 *      were dealt to; which = 5: the passes sp_fam (spectral_fam.h) made over its blocks; which = 6: the passes sp_nufft1, sp_nufft2 (spectral_nufft2.h) and
 *      sp_lomb_sums_grid (spectral_nufft.h) made over their rows (for the latter 1 + batch of them: the weights' row and the values').
 *      which = 7: the passes sp_burg and sp_yule (spectral_ar.h) made over their segments.
 *      which = 8: the passes sp_covmat and sp_ar_ls (spectral_sub.h) made over their segments.
 *      which = 9: the passes the tile form of sp_dwt, sp_idwt, sp_modwt and sp_imodwt (spectral_dwt.h) made over their rows (SP_DWT_ROWS caps a pass).
 *      0 where the call had no such loop, or for another `which`.
 *      All are reset where a call that touches the device begins.  The budgets behind the loops can be capped
 *      through the environment, read on every call (unset or <= 0: no cap): SP_LONG_CHUNK_FRAMES (frames of a long chunk),
 *      SP_LONG_SLICE_ROWS (rows of a slice), SP_CSDM_CHUNK_FRAMES (frames of a chunk of sp_csd_matrix, before its chunks are
 *      equalised and rounded to 32). */
int sp_last_passes(int which);

#ifdef __cplusplus
}
#endif
#endif
