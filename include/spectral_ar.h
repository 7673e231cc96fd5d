/* spectral_ar.h -- C ABI of libspectral.so, eleventh table: autoregressive (maximum-entropy) models and their spectra: Burg's method,
 * Yule-Walker, and the power spectrum of an all-pole model.  The conventions are those of spectral.h (extern "C", caller-owned
 * buffers, `mem` 0 = host / 1 = device pointers, 0 = ok, < 0 = error with the message in sp_last_error(), which starts with the
 * entry's name).
 */
#ifndef SPECTRAL_AR_H
#define SPECTRAL_AR_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_AR_BAD_RECORD (-2) /* a sample of a segment is not finite: found before anything is written */
#define SP_AR_MAX_ORDER 256
#define SP_BURG_MAX_N 16384

/* ---- Fits.  x: float32 (dtype SP_DTYPE_F32) or complex64 (SP_DTYPE_C64) rows, [batch] rows of nsig samples, x_ld elements apart.
 *      Segment g = 0 .. nframes - 1 of a row is x[first + g hop + i], i = 0 .. n - 1, less the detrend: SP_DETREND_SEGMEAN the segment's
 *      own mean (formed in float64), SP_DETREND_CONST the constant mean_re + i mean_im (0, 0: nothing).  Model s = row * nframes + g:
 *        a     [s * out_ld + j], j = 0 .. order      the polynomial, a[0] = 1      float64 for float32 rows, complex128 for complex64 rows
 *        evar  [s * out_ld + m], m = 0 .. order      the prediction-error power by order, E_0 = (1 / n) sum |x|^2      float64
 *        k     [s * out_ld + m - 1], m = 1 .. order  the reflection coefficients                                         as a
 *      out_ld >= order + 1 counts elements of each array; what lies between the models is left as it is.
 *
 *      sp_burg is MATLAB's arburg.  f_0 = b_0 = x; for m = 1 .. order over i = m .. n - 1:
 *        num = sum f_{m-1}[i] conj(b_{m-1}[i-1]),  den = sum |f_{m-1}[i]|^2 + |b_{m-1}[i-1]|^2,  k_m = -2 num / den  (den == 0: k_m = 0,
 *        and so is every later one: never NaN),  f_m[i] = f_{m-1}[i] + k_m b_{m-1}[i-1],  b_m[i] = b_{m-1}[i-1] + conj(k_m) f_{m-1}[i],
 *        a_m[j] = a_{m-1}[j] + k_m conj(a_{m-1}[m-j]),  E_m = E_{m-1} (1 - |k_m|^2).
 *      With float32 products a nearly noiseless segment can give |k_m| a rounding above 1: E_m is then set to 0, never below it,
 *      as sp_yule does, so that sp_ar_psd gives zeros there and never a negative density.
 *      f and b are float32 in registers, the products float32, every sum float64 in a fixed order, k, a and E float64: two calls agree
 *      bitwise.  n <= 1024 takes the wave form of the kernel (one wave per segment, several segments per workgroup, no workgroup
 *      barrier), longer segments the workgroup form (one barrier per order); SP_BURG_FORM = 1 / 2 in the environment forces a form
 *      where the length allows it.
 *
 *      sp_yule: the biased lags r[l] = (1 / n) sum_{i=l}^{n-1} x[i] conj(x[i-l]), l = 0 .. order (float32 products, float64 sums, by
 *      tiles of the segment whose partial lags are added in order) and Levinson-Durbin in float64, which gives the same triple.
 *      r[0] == 0 gives the zero model (a = 1, 0 ..; E = 0; k = 0).
 *
 *      Segments beyond what a pass holds go in passes (SP_AR_SEGS caps the segments of a pass); sp_last_passes(7) reports them.
 *      Refused (-1, the device is not touched, the outputs are untouched): order outside 1 .. 256 or above n / 2; n below 2, above
 *      16384 (sp_burg) or 2^31 - 1 (sp_yule); hop < 1; first < 0; frames that reach outside the nsig samples of a row; x_ld < nsig;
 *      out_ld < order + 1; a dtype or detrend not named above; a mean that is not finite; batch or nframes negative; x, a, evar or
 *      k NULL.  batch == 0 or nframes == 0 returns 0 and launches nothing.  A sample that is not finite is found by a pass over
 *      the segments before anything is written: SP_AR_BAD_RECORD (-2). */
int sp_burg(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
            int order, int detrend, double mean_re, double mean_im, void *a, double *evar, void *k, int64_t out_ld, int mem);
int sp_yule(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
            int order, int detrend, double mean_re, double mean_im, void *a, double *evar, void *k, int64_t out_ld, int mem);

/* ---- The spectrum of models: P[s * P_ld + q] = scale e[s * e_ld] / |sum_{j=0}^{order} a[s * a_ld + j] exp(-2 pi i j nu_q)|^2 at
 *      nu_q = start + q step cycles per sample, q = 0 .. m - 1 (the start, step, m of sp_czt).  a: float64 (cplx 0) or complex128
 *      (cplx 1); e: one float64 per model, e_ld apart (evar + order with e_ld = out_ld takes the last of a fit's powers).  Float64
 *      throughout: nu_q is reduced to its fraction of a turn in float64 and the polynomial is summed by Horner's rule on the unit
 *      circle; P is float32, or float64 with out64.  e == 0 gives zeros.  A row of a padded with zeros is a model of lower order.
 *      Refused (-1): order outside 0 .. 256; a_ld < order + 1; e_ld < 1; P_ld < m; m outside 1 .. 2^31 - 1; nmodels negative or
 *      nmodels x ceil(m / 256) beyond 2^31 - 1; start, step or scale not finite; a, e or P NULL.  nmodels == 0 returns 0. */
int sp_ar_psd(const void *a, int cplx, int64_t a_ld, const double *e, int64_t e_ld, int order, int64_t nmodels, int64_t m, double start,
              double step, double scale, int out64, void *P, int64_t P_ld, int mem);

/* ---- sp_ar_plan (host only, never touches the device): method 0 = Burg, 1 = Yule-Walker.  out[8] = the form (0 the wave form of
 *      k_burg, 1 its workgroup form, 2 lags and Levinson), segments per workgroup, samples per lane (k_burg) or per tile (lags), LDS
 *      bytes of the main kernel, its workgroups over all passes, passes, threads of a workgroup, tiles of a segment.
 *      < 0 for a shape the fit refuses, or out NULL. */
int sp_ar_plan(int method, int dtype, int64_t n, int order, int64_t batch, int64_t nframes, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
