/* spectral_mimo.h -- C ABI of libspectral.so, fifteenth table: conditioned spectral analysis (Bendat & Piersol) of cross-spectral-density
 * matrices: the frequency responses of several outputs to several correlated inputs, multiple and partial coherence, the conditioned
 * (residual) spectra of the outputs and the ordered conditioned autospectra, all read off one Cholesky factor per matrix.
 * The conventions are those of spectral.h (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, 0 = ok, < 0 =
 * error with the message in sp_last_error(), which starts with the entry's name).
 */
#ifndef SPECTRAL_MIMO_H
#define SPECTRAL_MIMO_H

#include "spectral_array.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SP_COND_MAX_N 64
#define SP_COND_H 1    /* bits of `want` */
#define SP_COND_GC 2
#define SP_COND_MCOH 4
#define SP_COND_PIV 8
#define SP_COND_P 16

/* ---- `count` Hermitian matrices of order n, complex128, row-major, matrix s at G + s G_ld (G_ld >= n^2, in elements), with the
 *      convention G[i][j] = E[X_i conj X_j].  Only the lower triangle and the real part of the diagonal are read.  `order` is a HOST array
 *      of n int32 whatever `mem` says, a permutation of 0 .. n - 1, or NULL for the identity: its first q entries name the inputs, the
 *      other r = n - q the outputs.  With
 *        A = G[order][:, order] + delta I,   delta = loading max(Re trace A, 0) / n,   A = L L^H (L lower triangular, diagonal > 0),
 *        L = [[L_xx, 0], [L_yx, L_yy]]
 *      the outputs that `want` names are written, matrix s at pointer + s x its leading dimension (in elements of its type):
 *        H     complex128 [r][q]   L_yx L_xx^-1 = A_yx A_xx^-1, the least-squares response in Y = H X + N          H_ld >= r q
 *        Gc    complex128 [r][r]   L_yy L_yy^H = A_yy - A_yx A_xx^-1 A_xy, exactly Hermitian                      Gc_ld >= r r
 *        mcoh  float64 [r]         sum_{k<q} |L_{q+i,k}|^2 / A_{q+i,q+i}; 0 where that diagonal is <= 0            mcoh_ld >= r
 *        piv   float64 [n]         L_jj^2: the autospectrum of channel order[j] conditioned on those before it   piv_ld >= n
 *        P     complex128 [n][n]   A^-1 = L^-H L^-1, exactly Hermitian                                            P_ld >= n n
 *      What lies between the matrices' outputs is left as it is; pointers of outputs that are not wanted may be NULL.
 *      status[s] (int32) is 0, or the 1-based position j in `order` of the first pivot that is not above n 2^-52 A_jj (a NaN fails it):
 *        j <= q   the inputs are collinear: H, Gc, mcoh and P are zeros and piv is zero from position j on; never NaN;
 *        j > q    that pivot and the column of L under it are set to zero and the factorisation goes on (an output that its inputs
 *                 and the outputs before it explain completely): H and mcoh are as without it, P is zeros.
 *                 "Never NaN" is promised for j <= q only: a NaN among the elements of the output rows is no collinearity of the inputs;
 *                 it fails the pivot it reaches (j > q), H, mcoh and the pivots before j are as without it, and the rows and columns
 *                 of Gc that it touched carry it on.
 *      float64 throughout, no atomics, every sum in a fixed order: two calls agree bitwise, host and device pointers give the same bits.
 *      Refused (-1, the device is not touched, the outputs are untouched): n outside 1 .. 64; q outside 0 .. n; count negative or beyond
 *      2^40; want empty or with a bit not named above; G_ld or a wanted output's leading dimension too small; loading negative or not
 *      finite; an order that is no permutation; G, status or a wanted output NULL (an output without elements, r = 0 or q = 0, may be).
 *      count == 0 returns 0 and launches nothing. */
int sp_cond(const void *G, int64_t G_ld, int n, int64_t count, const int32_t *order, int q, unsigned want, double loading, void *H, int64_t H_ld,
            void *Gc, int64_t Gc_ld, double *mcoh, int64_t mcoh_ld, double *piv, int64_t piv_ld, void *P, int64_t P_ld, int32_t *status, int mem);

/* ---- sp_cond_plan (host only, never touches the device).  out[8] = the row pitch in elements, threads of a workgroup, LDS bytes of a
 *      workgroup, 1 if that is above 64 KiB (the launch raises the kernel's limit), workgroups launched, the most matrices one of them
 *      walks, the byte offset of the inverse factor's region (0 without P), the byte offset of the kept diagonal.
 *      < 0 for a shape the call refuses, or out NULL. */
int sp_cond_plan(int n, int q, int64_t count, unsigned want, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
