/* spectral_quad.h -- C ABI of libspectral.so, fourth table: quadratic time-frequency distributions (Cohen's class).  The conventions
 * are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST
 * pointers, 0 = ok, < 0 = error with the message in sp_last_error()).
 */
#ifndef SPECTRAL_QUAD_H
#define SPECTRAL_QUAD_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The smoothed pseudo Wigner-Ville distribution (Flandrin 1984; Auger & Flandrin 1995).
 *      x and y are complex64 rows of nsig samples, x_ld samples apart (both), zero outside 0 .. nsig - 1.  h is a real lag window of
 *      nh = 2 Lh + 1 taps, g a real time window of ng = 2 Lg + 1 taps, both HOST float32 tables, odd, centred and indexed -L .. L.
 *      The column times are n_j = first + j hop, j < ntimes; first may be negative.
 *        K[j][tau] = h[tau] sum_{mu = -Lg .. Lg} g[mu] x[n_j + mu + tau] conj(y[n_j + mu - tau]),   tau = -Lh .. Lh, 0 for the other lags
 *        W[j][k]   = scale sum_tau K[j][tau] exp(-2 pi i k tau / nfft),                              k = 0 .. nfft - 1
 *      The lag is 2 tau samples: bin k stands for the frequency k fs / (2 nfft), and W has the period fs / 2.  g = [1] is the pseudo
 *      Wigner-Ville distribution, and a rectangular h over the whole record the Wigner-Ville distribution itself.
 *      y == NULL (auto): y = x, and W float32 [batch][ntimes][nb] is the REAL PART of the definition, which is all of it for a
 *      symmetric h (K is then Hermitian in tau); for any other h it is the distribution under (h[tau] + h[-tau]) / 2.
 *      y != NULL (cross): W complex64 [batch][ntimes][nb].
 *      The band is the nb bins from b0 on, modulo nfft.  A column whose time window n_j - Lg .. n_j + Lg misses the record is zero.
 *      One fused kernel; K never exists in memory.  In the auto case the columns 2p and 2p + 1 of a row share one transform, whatever
 *      the partition into runs, and the last column of an odd count is paired with itself.  No atomics: two calls agree bitwise, and so
 *      do calls under different columns per run (the environment variable SP_WVD_CPR forces that number).
 *      x, y and W follow `mem`; device-resident arrays need only their natural alignment.
 *      Refused (< 0, sp_last_error() starts with "sp_wvd: " and names the argument, the device is not touched, the outputs are
 *      untouched): nfft not a power of two in 32 .. 8192; nh even, < 1 or > nfft - 1; ng even, < 1 or > 255; hop < 1; ntimes < 0;
 *      batch < 0 or > 65535; nsig < 1; x_ld < nsig; nb < 1 or > nfft; b0 outside 0 .. nfft - 1; a scale that is not finite; x, h, g or
 *      W NULL; columns that lie beyond 2^40 samples; a shape whose LDS does not fit a workgroup (sp_wvd_plan tells).
 *      batch == 0 or ntimes == 0 returns 0 and launches nothing.
 *      sp_wvd_plan (host only, never touches the device): out[5] = columns per run, workgroups launched, LDS bytes of a workgroup,
 *      transforms per run, 1 if the shape fits else 0.  LDS: max(1, 4096 / nfft) transform images of (nfft + 16) * 8 bytes, and 8
 *      bytes per staged sample: (c - 1) hop + nh + ng - 1 of them, c = the columns per run (auto: rounded up to even), at most
 *      ntimes.  The columns per run are cut down to what fits 160 KiB; a shape that does not fit with one column (auto: two) is
 *      refused, as is a forced number that does not fit.  The CU count is the device's once the library is initialised and 256
 *      before.  < 0 for a shape that is refused for another reason than its LDS, or out NULL. */
int sp_wvd(const void *x, const void *y, int64_t x_ld, int64_t nsig, int64_t batch, const float *h, int nh, const float *g, int ng,
           int nfft, int64_t hop, int64_t first, int64_t ntimes, int b0, int nb, double scale, void *W, int mem);
int sp_wvd_plan(int cross, int nfft, int nh, int ng, int64_t hop, int64_t ntimes, int64_t batch, int nb, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
