/* spectral_fam.h -- C ABI of libspectral.so, eighth table: the FFT accumulation method.  The conventions are those of spectral.h
 * (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST pointers, 0 = ok,
 * < 0 = error with the message in sp_last_error()).
 */
#ifndef SPECTRAL_FAM_H
#define SPECTRAL_FAM_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FFT accumulation method (FAM; Roberts, Brown & Loomis, IEEE SP Magazine 8(2), 1991): the spectral correlation of the whole
 *      (f, alpha) plane at once, where sp_cyclic (spectral_cyclo.h) estimates it at cycle frequencies the caller already knows.
 *      Units are cycles per sample, e(t) = exp(2 pi i t).
 *      x is a row of nsig samples, float32 or complex64 (dtype); y an optional second row of the same dtype, NULL: y = x.  a is a real
 *      channelizer window of np taps, hop the frame step, g a real taper of P taps over the frames of a block (a, g: HOST float32).
 *      mean_x, mean_y: HOST float64 (re, im), NULL = 0, rounded to float32 before they are subtracted (a real row ignores im).
 *      Frame p is the np samples from p hop on.  Block b is the frames bP .. bP + P - 1: blocks are disjoint, and nblocks P frames
 *      must lie inside the row.  Channel k (fft order) has the signed frequency f_k = k / np for k < np / 2, else (k - np) / np.
 *      Q = P hop / (2 np).
 *        X[p][k] = e(-k p hop / np) DFT_np( a[j] (x[p hop + j] - m_x) )[k]        (demodulated to absolute time; Y alike from y)
 *        T_b[q]  = sum_{p < P} g[p] Y[bP + p][k] conj(X[bP + p][l]) e(-q p / P)   (conj != 0: ... X[bP + p][l], no conjugate)
 *        S[i][j] = scale sum_b T_b[q = j - Q],  j = 0 .. 2Q - 1,  for the pair i = (k, l) of the HOST int32 table pairs[npairs][2]
 *        Pwx[k]  = scale sum_b sum_p g[p] |X[bP + p][k]|^2                        (float32 [np]; Pwy alike from Y)
 *      Cell (i, j) of the plain form stands for f = (f_k + f_l) / 2 and alpha = f_k - f_l + (j - Q) / (P hop); of the conjugate form
 *      (conj != 0) for f = (f_k - f_l) / 2 and alpha = f_k + f_l + (j - Q) / (P hop).  The 2Q bins kept per pair are exactly the ones
 *      within half a channel spacing of the pair's own alpha: the tiles of all pairs with one k - l (or k + l) cover the alpha axis
 *      without overlap, at the cyclic resolution 1 / (P hop).
 *      Two facts (checked in float64 on the host: np 32, hop 8, P 64, 3 blocks; tests/test_host_fam.py):
 *      1. The demodulation is a shift.  P hop is a multiple of np, so the factor e(-(k - l) p hop / np) only moves the output bin:
 *         S[i][j] = F[(j - Q + (k - l) P hop / np) mod P] of the P-point transform F of the un-demodulated product (the conjugate
 *         form: k + l); agreement 1.8e-16.  The kernel holds no phase table and reads the frame-referenced STFT as it is.
 *      2. Blocks add with no `first`.  Everything is periodic in P hop samples: the S (scale 1) of the parts of a record cut at block
 *         starts add up to the whole's; in float64 the difference is exactly 0.
 *      The call walks the blocks in passes.  Per pass the STFT kernel of sp_stft writes the frames of Y and X bin-major into library
 *      scratch (np P 8 bytes per block and record: 32 bytes per sample at hop = np / 4, 64 in the cross form), held to 256 MiB, one block
 *      at the least; the environment variable SP_FAM_BLOCKS caps the blocks of a pass (a test hook), and sp_last_passes(5) reports
 *      the passes of the last call.  The pair kernel (k_fam.hip) gives a transform group one pair: per block it loads P frames of row k
 *      of Y and of row l of X, multiplies them under g, runs one P-point forward transform and keeps the 2Q shifted bins.  Sums: float32
 *      over the blocks of a pass in ascending order, float64 across passes (16 bytes per cell of S, only in a call of several passes);
 *      Pwx and Pwy in float64 throughout.  `scale` is applied once at the end, in float64.  No atomics and a fixed order: two calls
 *      agree bitwise; the same record under another pass plan agrees to rounding.
 *      Outputs: S complex64 [npairs][2Q], Pwx, Pwy float32 [np] (Pwy of y = x when y is NULL); any may be NULL, not all.  x, y and the
 *      outputs follow `mem`; device pointers need only their natural alignment.
 *      Refused (< 0, sp_last_error() starts with "sp_fam: " and names the argument, the device is not touched, the outputs are
 *      untouched): np or P that is no power of two in 32 .. 8192; hop that is no power of two in 1 .. np; P hop < 2 np; nblocks < 0; a
 *      frame outside the row; npairs outside 1 .. 2^22; a pair index outside 0 .. np - 1; a dtype that is neither float32 (0) nor
 *      complex64 (1); scale or a mean that is not finite; x, a, g or pairs NULL; all outputs NULL; and, beyond the list of the other
 *      entries, a call of more than one pass whose float64 sums (npairs 2Q 16 bytes) are above 2 GiB.  nblocks == 0 returns 0 and
 *      launches nothing.
 *      sp_fam_plan (host only, never touches the device; cross: y is given): out[5] = Q, blocks per pass, passes, workgroups of the
 *      pair kernel over all passes, bytes of the bin-major frames of a pass (the transposition behind the STFT kernel stages through
 *      a frame-major buffer of one record's share besides).  < 0 for a shape sp_fam refuses, or out NULL. */
int sp_fam(const void *x, const void *y, int dtype, int64_t nsig, const float *a, int np, int64_t hop, const float *g, int P,
           int64_t nblocks, const int32_t *pairs, int64_t npairs, int conj, const double *mean_x, const double *mean_y, double scale,
           void *S, void *Pwx, void *Pwy, int mem);
int sp_fam_plan(int dtype, int cross, int np, int64_t hop, int P, int64_t nblocks, int64_t npairs, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
