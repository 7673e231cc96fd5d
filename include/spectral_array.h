/* spectral_array.h -- C ABI of libspectral.so, fourteenth table: the wavenumber (mode-number, slowness) scan of a sensor array from the
 * eigendecompositions of its cross-spectral-density matrices: the Bartlett, Capon (MVDR), MUSIC and eigenvector estimators.
 * The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, 0 = ok, < 0 =
 * error with the message in sp_last_error(), which starts with the entry's name).
 */
#ifndef SPECTRAL_ARRAY_H
#define SPECTRAL_ARRAY_H

#include "spectral_sub.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_BEAM_MAX_M 64
#define SP_BEAM_BARTLETT 0 /* g_k = w_k;               P = D / m^2 */
#define SP_BEAM_CAPON 1    /* g_k = 1 / (w_k + delta);  P = 1 / D,  delta = loading max(sum_k w_k, 0) / m */
#define SP_BEAM_MUSIC 2    /* g_k = 1 for k >= p;       P = 1 / D */
#define SP_BEAM_EV 3       /* g_k = 1 / w_k for k >= p; P = 1 / D */

/* ---- The scan of nmodels eigendecompositions as sp_eigh writes them (a model is a frequency bin): V complex128, component i of vector k
 *      of model s at V[(s m + i) V_ld + k], V_ld >= m; w[s m + k] float64, descending.  The tables are HOST arrays whatever `mem` says, as
 *      windows and filters are: pos[m][ndim] the sensor positions, kv[nk][ndim] the scan vectors in turns per unit of pos, scale[nmodels]
 *      or NULL (= 1; a slowness scan passes the bins' frequencies).  ndim is 1, 2 or 3.  The steering vector of scan point q in model s:
 *        t = pos[i][0] kv[q][0];  t = t + pos[i][1] kv[q][1];  ..;  phi = scale[s] t;  fr = phi - floor(phi)
 *        a_q[i] = (cos 2 pi fr, sin 2 pi fr)
 *      every product and every sum rounded on its own in float64 (no fused multiply-add), the sine and cosine by sincospi.  With
 *      pos[i] = i, ndim = 1 and kv[q] = nu_q this is the steering vector of sp_pseudospectrum.  Then
 *        D[s, q] = sum_k g_k(s) |a_q(s)^H v_k(s)|^2
 *      under the weights named above (every weight not named is 0), and P[s * P_ld + q], q = 0 .. nk - 1, P_ld >= nk, is D / m^2 or
 *      1 / D; a sum of exactly zero gives P = 0, never NaN.  P is float32, or float64 with out64; what lies between the rows is left as
 *      it is.  status[s] (int32) is 1 where a weight that was needed had a denominator <= 0 (that weight is then 0), else 0; always 0
 *      for Bartlett and MUSIC.  float64 throughout, every sum in a fixed order (sensors ascending inside a projection, vectors ascending
 *      inside a wave's share, the shares in wave order): two calls agree bitwise, and scale = NULL gives the bits of scale = ones.
 *      p is looked at by MUSIC and EV only; loading by Capon only (it is judged for every method).
 *      Refused (-1, the device is not touched, the outputs are untouched): m outside 2 .. 64; V_ld < m; ndim outside 1 .. 3; nk outside
 *      1 .. 2^31 - 1; P_ld < nk; a method not named above; p outside 0 .. m - 1 for MUSIC and EV; loading negative or not finite; pos,
 *      kv or scale not finite; V, w, pos, kv, P or status NULL; nmodels negative, or nmodels x ceil(nk / 64) beyond 2^40.
 *      nmodels == 0 returns 0 and launches nothing. */
int sp_beamscan(const void *V, int64_t V_ld, const double *w, int m, int64_t nmodels, const double *pos, int ndim, const double *kv, int64_t nk,
                const double *scale, int method, int p, double loading, int out64, void *P, int64_t P_ld, int32_t *status, int mem);

/* ---- sp_beamscan_plan (host only, never touches the device).  out[8] = steering vectors of a tile, tiles of a model, eigenvectors of a
 *      stage, LDS bytes of a workgroup, workgroups launched, the most (model, tile) items one of them walks, stages of a tile, 0.
 *      < 0 for a shape the call refuses, or out NULL. */
int sp_beamscan_plan(int m, int ndim, int64_t nk, int64_t nmodels, int method, int p, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
