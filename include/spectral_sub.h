/* spectral_sub.h -- C ABI of libspectral.so, twelfth table: the data covariance matrix of a segment, the covariance and
 * modified-covariance least-squares autoregressive fits (MATLAB's arcov / armcov), and the MUSIC / eigenvector pseudospectrum.
 * The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, 0 = ok, < 0 =
 * error with the message in sp_last_error(), which starts with the entry's name).
 */
#ifndef SPECTRAL_SUB_H
#define SPECTRAL_SUB_H

#include "spectral_ar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_SUB_MAX_M 64
#define SP_SUB_MUSIC 0 /* weighting: g_k = 1 */
#define SP_SUB_EV 1    /* weighting: g_k = 1 / w_k */

/* ---- The data covariance matrix.  The record arguments (x, dtype, x_ld, nsig, batch, n, hop, first, nframes, detrend, mean_re,
 *      mean_im) are those of sp_burg (spectral_ar.h): segment s = row * nframes + g is s[t] = x[first + g hop + t] less the detrend,
 *      t = 0 .. n - 1.  Here the detrended sample stays float64; products and sums are float64 in a fixed order: two calls agree
 *      bitwise.  With N = n - m + 1 snapshots, 2 <= m <= 64, m <= n:
 *        fb = 0 (covariance):       C[i,j] = (1 / N) sum_{t=m-1}^{n-1} conj(s[t-i]) s[t-j],  i, j = 0 .. m - 1
 *        fb = 1 (modified):         C_fb = (C + J conj(C) J) / 2, J the exchange matrix
 *      which is X'X of MATLAB's corrmtx(x, m - 1, 'covariance' | 'modified').  C: complex128, matrix s at C[s * C_ld + i m + j],
 *      C_ld >= m m counts complex elements; what lies between the matrices is left as it is.  The output is exactly Hermitian with
 *      a real diagonal (zero imaginary parts for float32 rows).  Row 0 is summed by tiles of the segment whose partial rows are
 *      added in order; the rest follows diagonal by diagonal from
 *        C[i+1,j+1] = C[i,j] + conj(s[m-2-i]) s[m-2-j] - conj(s[n-1-i]) s[n-1-j]
 *      so the work is O(n m + m^2) per segment.  Segments beyond what the scratch holds go in passes (SP_AR_SEGS caps the segments
 *      of a pass); sp_last_passes(8) reports them.
 *      Refused (-1, the device is not touched, the outputs are untouched): m outside 2 .. 64 or above n; fb not 0 or 1; C_ld < m m;
 *      C NULL; and everything sp_burg refuses about the record (n, hop, first, frames that reach outside a row, x_ld, dtype,
 *      detrend, a mean that is not finite, batch or nframes negative, x NULL).  batch == 0 or nframes == 0 returns 0 and launches
 *      nothing.  A sample that is not finite: SP_AR_BAD_RECORD (-2), nothing is written. */
int sp_covmat(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
              int m, int fb, int detrend, double mean_re, double mean_im, void *C, int64_t C_ld, int mem);

/* ---- The least-squares fits of order p = m - 1, 1 <= order <= 63, order <= n / 2 (fb = 0: arcov, fb = 1: armcov): with C of sp_covmat
 *      at m = order + 1 (formed in scratch), solve sum_{j=1}^{p} C[i,j] a_j = -C[i,0], i = 1 .. p, by Cholesky in complex128;
 *      a_0 = 1 and e = Re(C[0,0] + sum_j C[0,j] a_j).
 *        a      [s * out_ld + j], j = 0 .. order     float64 for float32 rows, complex128 for complex64 rows; out_ld >= order + 1
 *        e      [s]                                   float64
 *        status [s]                                   int32: 0, or the 1-based index j of the first pivot d_j <= m 2^-52 C[j,j]; then
 *                                                     a = (1, 0 ..) and e = 0: never NaN
 *      Refused as sp_covmat, and: order outside 1 .. 63 or above n / 2; out_ld < order + 1; a, e or status NULL. */
int sp_ar_ls(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
             int order, int fb, int detrend, double mean_re, double mean_im, void *a, double *e, int32_t *status, int64_t out_ld, int mem);

/* ---- The pseudospectrum of nmodels eigendecompositions as sp_eigh writes them: V complex128, component i of vector k of model s at
 *      V[(s m + i) V_ld + k], V_ld >= m; w[s m + k] float64, descending.  With the signal dimension 0 <= p < m and the steering vector
 *      e(nu)[i] = exp(+2 pi i nu i):
 *        P[s * P_ld + q] = 1 / sum_{k=p}^{m-1} g_k |sum_i V[.. i, k] exp(-2 pi i nu_q i)|^2,  nu_q = start + q step, q = 0 .. nbins - 1
 *      weighting SP_SUB_MUSIC: g_k = 1; SP_SUB_EV: g_k = 1 / w_k, and where w_k <= 0, g_k = 0 and status[s] = 1 (else 0; always 0 for
 *      MUSIC).  A sum of zero gives P = 0, never NaN.  float64 throughout, the phase reduced as sp_ar_psd does; P is float32, or
 *      float64 with out64.
 *      Refused (-1): m outside 2 .. 64; p outside 0 .. m - 1; V_ld < m; weighting not named above; nbins outside 1 .. 2^31 - 1;
 *      P_ld < nbins; nmodels negative or nmodels x ceil(nbins / 256) beyond 2^31 - 1; start or step not finite; V, w, P or status
 *      NULL.  nmodels == 0 returns 0. */
int sp_pseudospectrum(const void *V, int64_t V_ld, const double *w, int m, int p, int64_t nmodels, int weighting, int64_t nbins, double start,
                      double step, int out64, void *P, int64_t P_ld, int32_t *status, int mem);

/* ---- sp_sub_plan (host only, never touches the device): what 0 = sp_covmat, 1 = sp_ar_ls (m = order + 1).  out[8] = samples of a
 *      tile, tiles of a segment, shares of a stage (k_cov_row), LDS bytes of k_cov_row, its workgroups over all passes, passes, scratch
 *      bytes of a segment, segments of a pass.  < 0 for a shape the call refuses, or out NULL. */
int sp_sub_plan(int what, int dtype, int64_t n, int m, int64_t batch, int64_t nframes, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
