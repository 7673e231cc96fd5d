/* spectral_tfr.h -- C ABI of libspectral.so, third table: time-frequency reassignment.  The conventions are those of spectral.h
 * (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST pointers, 0 = ok,
 * < 0 = error with the message in sp_last_error()); its constants (SP_DTYPE_*) are used here.
 */
#ifndef SPECTRAL_TFR_H
#define SPECTRAL_TFR_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The synchrosqueezed STFT and the reassignment operators (Auger & Flandrin 1995; Daubechies, Lu & Wu 2011; Thakur & Wu 2011).
 *      Frame g of a row is the n samples from first + g hop on, zero outside the row (first may be negative); with segmean != 0 the
 *      mean of these n values is removed from all of them.  n is a power of two in 32 .. 8192, c = n / 2.  With the HOST float32
 *      tables h, dh (dh/dj per sample) and th ((j - c) h), n values each:
 *        X_h, X_d, X_t = the n-point DFTs of h x, dh x, th x over the frame (phase at the frame's start)
 *        khat[g][k] = k - (n / 2 pi) Im(X_d conj X_h) / |X_h|^2        the instantaneous frequency, in bins
 *        that[g][k] = Re(X_t conj X_h) / |X_h|^2                       the group delay, in samples from the frame's centre
 *        used(g, k) = |X_h[g][k]| > max(gamma, rel max_k |X_h[g][k]|)
 *        Xc[g][k]   = (-1)^k X_h[g][k]                                 the phase referred to the frame's centre
 *      The source bins k are 0 .. n - 1 for complex64 rows and 0 .. n / 2 for float32 rows.  The target m = rint(khat) (ties to even)
 *      is taken modulo n for complex rows; for real rows targets outside 0 .. n / 2 are dropped (and for complex rows cells with
 *      |khat| >= 2^30).
 *      sp_ssq: any non-empty subset of
 *        T  complex64 [batch][nframes][nb]   T[g][m - b0] = sum over the used k with target m of Xc[g][k]
 *        P  float32   [batch][nframes][nb]   the same sum of |X_h[g][k]|^2
 *        IF float32   [batch][nframes][nb]   khat at the SOURCE bin b0 + j, NaN where the cell is not used
 *        GD float32   [batch][nframes][nb]   that likewise
 *      over the band of nb bins from b0 on (modulo n for complex rows; inside 0 .. n / 2 for real rows); targets outside the band are
 *      dropped.  IF and GD need th (one more transform per frame); th is ignored without them.
 *      The sums are exact in fixed point: per frame every coefficient is scaled by 2^(48 - e), e the binary exponent of the frame's
 *      largest |Re X_h| or |Im X_h| (for P: of its largest |X_h|^2), rounded to a 64-bit integer and added as an integer, so a sum is
 *      the exact sum of the float32 coefficients as rounded to 2^-48 of the frame's largest, rounded once to float32, and the same
 *      bits for any order.
 *      No float atomics: two calls agree bitwise, whatever the partition into runs.
 *      sp_ssq_bands: the same front end, and per frame and band b < nbands <= 8, without forming T,
 *        out complex64 [batch][nbands][nframes]   out[b][g] = scale * sum over the used k with lo[b][g] <= khat < hi[b][g] of Xc[g][k]
 *      with the un-rounded khat; the edges in bins, exactly one of: edges HOST float64 [nbands][2] = (lo, hi), constant over the
 *      frames, or edges_t float32 [nbands][nframes][2], following `mem`.  With first = -n / 2 and hop = 1, out / (n h[c]) is the band's
 *      analytic waveform; for hop > 1 it is that waveform sampled at the frame centres, carrier included.
 *      sp_ssq_sum: the same band sums over an existing T [batch][nframes][nb] whose first bin is b0 of an n-point transform:
 *        out[b][g] = scale * sum over lo <= m < hi of w_m T[g][j],   m = (b0 + j) mod n the absolute bin of column j (a band that wraps
 *        past n - 1 continues at bin 0; the edges are compared with m, so they lie in 0 .. n),   w = 1/2 at the bins 0 and n / 2 when
 *        half != 0, else 1.
 *      x, T, P, IF, GD, edges_t and out follow `mem`; device-resident arrays need only their natural alignment.
 *      Refused (< 0, sp_last_error() names the entry and the argument, the device is not touched, the outputs are untouched): n not a
 *      power of two in 32 .. 8192; hop < 1; nframes < 0; batch < 0 or > 65535; an unknown dtype; nsig < 1; x_ld < nsig; no output;
 *      IF or GD without th; nb < 1 or a band outside the bins; gamma or rel negative or not finite; nbands outside 1 .. 8; both or
 *      neither of edges and edges_t, edges that are not finite; a scale that is not finite; a shape whose LDS does not fit a
 *      workgroup (sp_ssq_plan tells); x, h or dh NULL.  batch == 0 or nframes == 0 returns 0 and launches nothing.
 *      sp_ssq_plan (host only, never touches the device): what = 1 (T) | 2 (P) | 4 (IF / GD) for sp_ssq, 8 for sp_ssq_bands;
 *      out[5] = frames per run, workgroups launched, LDS bytes of a workgroup, transforms per frame, 1 if the shape fits else 0.  LDS:
 *      (n + 16) * 8 bytes per transform and 16 bytes per bin of the band for T, 8 for P, per transform group, max(1, 4096 / n) groups.
 *      The CU count is the device's once the library is initialised and 256 before.  < 0 for a shape that is refused for another
 *      reason than its LDS, or out NULL. */
int sp_ssq(const void *x, int64_t x_ld, int dtype, int64_t nsig, int64_t batch, const float *h, const float *dh, const float *th, int n,
           int hop, int64_t first, int64_t nframes, int segmean, double gamma, double rel, int b0, int nb, void *T, float *P, float *IF,
           float *GD, int mem);
int sp_ssq_bands(const void *x, int64_t x_ld, int dtype, int64_t nsig, int64_t batch, const float *h, const float *dh, int n, int hop,
                 int64_t first, int64_t nframes, int segmean, double gamma, double rel, int nbands, const double *edges,
                 const float *edges_t, double scale, void *out, int mem);
int sp_ssq_sum(const void *T, int64_t nframes, int nb, int64_t batch, int n, int b0, int nbands, const double *edges, const float *edges_t,
               int half, double scale, void *out, int mem);
int sp_ssq_plan(int cplx, int n, int64_t nframes, int64_t batch, int nb, int what, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
