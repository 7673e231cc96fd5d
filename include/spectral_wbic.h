/* spectral_wbic.h -- C ABI of libspectral.so, seventh table: the wavelet bispectrum.  The conventions are those of spectral.h
 * (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST pointers, 0 = ok,
 * < 0 = error with the message in sp_last_error()).
 */
#ifndef SPECTRAL_WBIC_H
#define SPECTRAL_WBIC_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Wavelet bispectrum and bicoherence (van Milligen, Hidalgo & Sanchez, Phys. Plasmas 2, 3017, 1995), resolved in time.
 *      x, y, z are records of nsig samples, float32 or complex64, all of one dtype; y == NULL or y == x: y = x, z == NULL or z == x:
 *      z = x (records that are the same pointer are transformed once: 1, 2 or 3 transforms per scale).  scales[nscales] (HOST
 *      float64, in samples) are the scales of the rows i = 0 .. S - 1, whose frequencies the caller has chosen as (k_lo + i) df, so
 *      that the frequencies of the rows i and j add up to that of the row m = i + j + k_lo; the pair is valid when m <= S - 1.  With
 *      Wx, Wy, Wz the transforms sp_cwt defines (family, p0, frames of L samples with margin M), block b covers the T = block samples
 *      from n0 + b step on, b < nblocks, and
 *        B [b][i][j] = (1/T) sum_n Wx[i][n] Wy[j][n] conj(Wz[m][n])      complex128 (re, im)
 *        b2[b][i][j] = |B|^2 / (D P[b][m]),  D = (1/T) sum_n |Wx[i][n] Wy[j][n]|^2      float64, 0 where D P = 0
 *        P [b][m]    = (1/T) sum_n |Wz[m][n]|^2                          float64
 *      B and b2 are NaN at the invalid pairs.  Either step >= block (disjoint blocks; a cell is a block) or block % step == 0
 *      (overlapping blocks; a cell is `step` samples and a block the sum of block / step consecutive cells).  With y = x the result
 *      is symmetric in (i, j): only the tiles with tj <= ti are computed and the others mirrored.
 *      The transforms never exist as a whole: the call walks the record in passes.  A cell is cut into groups of at most 2048
 *      samples; a pass is a run of whole groups that spans at most 128 MiB / (8 S records) samples (the environment variable
 *      SP_WBIC_CHUNK caps the samples of a pass; one group is never cut) and at most 32768 groups, and whose fp32 partial sums
 *      (48 KiB per tile and group) stay within 128 MiB.  Per pass the kernels of sp_cwt transform the samples [a - M, b + M) of
 *      every distinct record, clipped to the record, into scratch, and one tile kernel contracts the samples [a, b) of it; float64
 *      sums per cell (96 KiB per tile and cell) outlive the passes, and after the last one the blocks are formed from them.  No
 *      atomics and a fixed order: two calls agree bitwise.  A pass starts its frames at a - M, so the same block computed under
 *      another pass plan agrees to rounding, not bitwise.  *passes (may be NULL) receives the passes made.
 *      x, y, z, B, b2 and P follow `mem`; device-resident arrays need only their natural alignment.
 *      Refused (< 0, sp_last_error() starts with "sp_wbic: ", the device is not touched, the outputs are untouched): nscales
 *      outside 2 .. 512; k_lo < 1; a scale that is not finite or not positive; M above 3072, or L and M that sp_cwt refuses; a family
 *      or parameter sp_cwt refuses; block < 1, step < 1, or neither step >= block nor block % step == 0; nblocks < 1; n0 < 0 or a
 *      block outside the record; nblocks S^2 24 bytes above 1 GiB; float64 cell sums above 2 GiB; a dtype that is neither float32
 *      nor complex64, or dtypes that differ; x, scales, B, b2 or P NULL.
 *      sp_wbic_plan (host only, never touches the device; nrec = the distinct records 1 .. 3, sym: y is x): out[8] = cells, samples
 *      of a cell, groups, passes, tile workgroups over all passes, scratch bytes (transforms, partials and cell sums), samples a pass
 *      may span, tiles.  < 0 for a shape sp_wbic refuses, or out NULL. */
int sp_wbic(const void *x, const void *y, const void *z, int x_dtype, int y_dtype, int z_dtype, int64_t nsig, const double *scales,
            int nscales, int k_lo, int family, double p0, int L, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks, void *B,
            double *b2, double *P, int *passes, int mem);
int sp_wbic_plan(int64_t nsig, int nscales, int k_lo, int L, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks, int nrec,
                 int sym, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
