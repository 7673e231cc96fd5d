/* spectral_dwt.h -- C ABI of libspectral.so, thirteenth table: the discrete wavelet transform.  The decimated pyramid of a filter bank
 * (dwt / wavedec and their inverses, six extension modes), its single level with separate outputs (what wavelet packets are built on),
 * and the undecimated circular MODWT and its inverse.  The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem`
 * 0 = host / 1 = device pointers, 0 = ok, < 0 = error with the message in sp_last_error(), which starts with the entry's name).
 *
 * Filters.  Every entry takes the two filters it uses as HOST float64 arrays of one even length L, 2 <= L <= 64, whatever `mem` is; they
 * are rounded once to float32.  In the order of pywt's Wavelet.filter_bank = (dec_lo, dec_hi, rec_lo, rec_hi): the analysis entries take
 * (dec_lo, dec_hi), the synthesis entries (rec_lo, rec_hi), both MODWT entries (rec_lo, rec_hi), which they scale by 1 / sqrt(2) in
 * float64 before the rounding.
 *
 * Modes (SP_DWT_*), an index map ext(i, n) of the array of the level being read plus a zero flag: ZERO 0 outside; CONSTANT the clamped
 * index; SYMMETRIC the half-sample mirror, period 2n; REFLECT the whole-sample mirror, period 2n - 2 (n = 1: index 0); PERIODIC i mod n;
 * PERIODIZATION (i mod n') with n' = n + (n odd), the last sample repeated.  The maps are periodic: a row shorter than the filter is
 * extended as often as needed.
 *
 * One analysis level of n samples, xe the extended array:  K = floor((n + L - 1) / 2), c = 1; PERIODIZATION: K = ceil(n / 2), c = L / 2
 *     cA[k] = sum_{m<L} dec_lo[m] xe[2k + c - m],   cD[k] = sum_{m<L} dec_hi[m] xe[2k + c - m],   k = 0 .. K - 1
 * One synthesis level, t = i + L - 2 (PERIODIZATION: t = i + L / 2 - 1), p = t mod 2, k0 = floor(t / 2):
 *     x[i] = sum_{q<L/2} rec_lo[p + 2q] cA[k0 - q] + sum_{q<L/2} rec_hi[p + 2q] cD[k0 - q]       (PERIODIZATION: k0 - q taken mod K)
 *   for i = 0 .. n - 1, where K is the coefficient length of n: of the 2K - L + 2 (2K) samples the formula gives, the last one is
 *   dropped where n is odd, as pywt's waverec does.
 * MODWT, circular, V_0 = x, g = rec_lo / sqrt 2, h = rec_hi / sqrt 2, s = 2^(j-1):
 *     W_j[t] = sum_{l<L} h[l] V_{j-1}[(t - s l) mod n],   V_j[t] the same with g
 *     V_{j-1}[t] = sum_l h[l] W_j[(t + s l) mod n] + sum_l g[l] V_j[(t + s l) mod n]
 * Arithmetic: float32 FMAs, the taps in ascending order (m, q, l), one accumulator per filter, the two sums of a synthesis added last;
 * complex rows use the same real taps on both parts; the approximations between levels are float32; no atomics.  One device function
 * computes a coefficient in every kernel form: two calls agree bitwise, host arrays and device pointers give the same bits, and so do
 * the two forms.
 *
 * Forms (`form`: SP_DWT_AUTO, SP_DWT_ROW, SP_DWT_TILE).  ROW: one launch; a workgroup stages a row (four rows of up to 1024 samples) in
 * LDS once and runs every level there, writing every detail and the last approximation; it fits where two buffers of
 * max(n, L - 1) + 2 (L - 1) elements per row and 512 bytes of filters fit 160 KiB of LDS (about 20 K float32 or 10 K complex64 samples).  TILE: one launch per
 * level, any n up to 2^31 - 1; the approximations between levels live in the library's scratch, and rows beyond what it holds go in
 * passes (sp_last_passes(9); SP_DWT_ROWS caps the rows of a pass).  AUTO takes ROW wherever it fits.
 */
#ifndef SPECTRAL_DWT_H
#define SPECTRAL_DWT_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_DWT_MAX_L 64
#define SP_DWT_ZERO 0
#define SP_DWT_CONSTANT 1
#define SP_DWT_SYMMETRIC 2
#define SP_DWT_REFLECT 3
#define SP_DWT_PERIODIC 4
#define SP_DWT_PERIODIZATION 5
#define SP_DWT_AUTO 0
#define SP_DWT_ROW 1
#define SP_DWT_TILE 2

/* ---- The pyramid of `levels` levels of every row x[b * x_ld + i], i < n, b < batch (dtype SP_DTYPE_F32 or SP_DTYPE_C64; pitches count
 *      elements): out[b * out_ld + ..] = [cA_J | cD_J | .. | cD_1] at the offsets sp_dwt_plan gives, out_ld >= their sum; what lies
 *      between the rows of out is left as it is.
 *      Refused (-1, before the device is touched, the outputs untouched): dtype; L odd or outside 2 .. 64; a filter NULL or not finite; an
 *      unknown mode; levels < 1 or beyond the level at which a row has one coefficient (32 at the most); n outside 1 .. 2^31 - 1; batch
 *      negative; x_ld < n; out_ld too small; form not named above, or SP_DWT_ROW for a row that does not fit; x or out NULL.
 *      batch == 0 returns 0 and launches nothing. */
int sp_dwt(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *dec_lo, const double *dec_hi, int L, int mode, int levels,
           void *out, int64_t out_ld, int form, int mem);

/* ---- One level with separate outputs: cA[b * a_ld + k], cD[b * d_ld + k], k < K; a_ld, d_ld >= K.  The two may interleave in one
 *      device buffer (cD = cA + K, a_ld = d_ld = 2K: the children of a packet node side by side); with mem = 0 they must not overlap.
 *      Refused as sp_dwt (levels is 1). */
int sp_dwt_level(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *dec_lo, const double *dec_hi, int L, int mode,
                 void *cA, int64_t a_ld, void *cD, int64_t d_ld, int form, int mem);

/* ---- The inverse of sp_dwt: the rows of n samples from pyramids laid out as sp_dwt writes them for the same (n, L, mode, levels). */
int sp_idwt(const void *coef, int dtype, int64_t c_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int mode, int levels,
            void *x, int64_t x_ld, int form, int mem);

/* ---- The inverse of sp_dwt_level: x[b * x_ld + i], i < n, from the K coefficients of cA and of cD that n samples have. */
int sp_idwt_level(const void *cA, int64_t a_ld, const void *cD, int64_t d_ld, int dtype, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi,
                  int L, int mode, void *x, int64_t x_ld, int form, int mem);

/* ---- The MODWT: W[(j - 1) * batch * w_ld + b * w_ld + t] = W_j[t], j = 1 .. levels, and V_levels in the plane behind them (levels + 1
 *      planes of batch rows, w_ld >= n).  Any n >= 1.  The row form keeps V in LDS; the tile form reads V_{j-1} through L2.
 *      Refused as sp_dwt, but: levels outside 1 .. 30, or 2^(levels-1) (L - 1) >= 2^31; there is no mode. */
int sp_modwt(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int levels, void *W,
             int64_t w_ld, int form, int mem);

/* ---- The inverse of sp_modwt, from planes laid out as it writes them. */
int sp_imodwt(const void *W, int dtype, int64_t w_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int levels, void *x,
              int64_t x_ld, int form, int mem);

/* ---- sp_dwt_plan (host only, never touches the device): what 0 = sp_dwt, 1 = sp_idwt, 2 = sp_modwt, 3 = sp_imodwt (mode is not looked
 *      at for 2 and 3).  out[0 .. 9] = the form taken (1 row, 2 tile), outputs of a tile, LDS bytes of a workgroup, workgroups over all
 *      launches, launches, passes, scratch bytes, rows of a pass, the deepest level this (n, L, mode) takes, rows of a workgroup (row form);
 *      then for every entry e = 0 .. levels of the output, in its order (cA_J, cD_J, .., cD_1; MODWT: W_1, .., W_J, V_J):
 *      out[10 + 2e] = its length, out[11 + 2e] = its offset in a row of the pyramid (MODWT: of the plane, in elements, at w_ld = n).
 *      < 0 for a shape the call refuses, or out NULL. */
int sp_dwt_plan(int what, int dtype, int64_t n, int L, int mode, int levels, int64_t batch, int form, int64_t out[80]);

#ifdef __cplusplus
}
#endif
#endif
