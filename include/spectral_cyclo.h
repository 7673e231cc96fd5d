/* spectral_cyclo.h -- C ABI of libspectral.so, fifth table: cyclostationary analysis.  The conventions are those of spectral.h
 * (extern "C", caller-owned buffers, `mem` 0 = host / 1 = device pointers, small parameter tables always HOST pointers, 0 = ok,
 * < 0 = error with the message in sp_last_error()).
 */
#ifndef SPECTRAL_CYCLO_H
#define SPECTRAL_CYCLO_H

#include "spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Spectral correlation and its two spectra by the averaged cyclic periodogram (Gardner 1986; Antoni 2007): for every cycle
 *      frequency a Welch cross spectrum between the record shifted down and up by half of it.
 *      x and y are rows of nsig samples, x_ld samples apart (both), float32 or complex64, both of the same dtype.  nu[A] (HOST
 *      float64) are the cycle frequencies in cycles per sample, |nu| <= 1; nu_h = nu / 2; e(t) = exp(2 pi i t).  Sample j of a row has
 *      the absolute index first + j.  Frame g < nframes is the n samples from g hop on and must lie inside the row; w is a real window
 *      of n taps (HOST float32).  mean_x, mean_y (HOST float64 [batch][2] = re, im; NULL = zeros) are subtracted; they are rounded to
 *      float32.  With s = g hop:
 *        Z+[g][k] = DFT_n( w[j] (y[s + j] - m_y) e(-nu_h (first + s + j)) )
 *        Z-[g][k] = DFT_n( w[j] (x'[s + j] - m_x') e(+nu_h (first + s + j)) ),   x' = conj(x), m_x' = conj(m_x) when conj != 0, else x, m_x
 *        S [a][k] = scale sum_g Z+ conj(Z-)    complex64   S_yx at f_k = k / n (two-sided, fft order): y at f_k + nu / 2 against x at f_k - nu / 2
 *        Pp[a][k] = scale sum_g |Z+|^2         float32     the PSD of y at f_k + nu / 2
 *        Pm[a][k] = scale sum_g |Z-|^2         float32     the PSD of x' at f_k - nu / 2
 *      y == NULL (auto): y = x and mean_y is not read.  S, Pp, Pm are [batch][A][nb], the nb bins from b0 on, modulo n; any of them may
 *      be NULL, not all.
 *      Phases are exact: nu_h is rounded ONCE to a multiple of 2^-64 turn (to nearest, ties to even), and nu_h (first + s + j) is a
 *      64-bit integer product whose wrap is the reduction modulo one turn.  The table w[j] e(-+nu_h j) is float64 sincospi rounded to
 *      float32; the factor of the frame's origin comes from a float64 sincospi of the exact phase and multiplies the product
 *      Z+ conj(Z-) as e(-nu (first + s)): it never touches Pp and Pm.  So a record cut at a frame start gives parts whose
 *      un-normalised S add up to the whole's, each part called with its own `first`.
 *      Transforms per (frame, nu): ONE in the mirrored form -- a real row, or a complex row with conj != 0, y == NULL -- where
 *      Z-[k] = conj(Z+[(n - k) mod n]), so S[k] = sum Z+[k] Z+[n - k] and Pm[k] = Pp[n - k]; two otherwise.
 *      One fused kernel and a float64 finish kernel that sums the groups of frames in a fixed order; no atomics: two calls agree
 *      bitwise.  A long nu list is cut into passes so that the partial sums of a pass stay within 256 MiB (the environment variable
 *      SP_CYCLIC_CHUNK caps the cycle frequencies per pass), and sp_last_passes(2) reports the passes of the last call.  Only the
 *      nu list is cut: a pass holds at least one nu of EVERY row, 48 .. 192 KiB per row (3 or 4 planes -- 6 for two transforms at
 *      8192 points -- of max(n, 4096) floats), so that beyond some 1400 .. 5400 rows one pass exceeds the 256 MiB, and 65535 rows
 *      ask for 3 .. 12 GiB of scratch; batch the rows by call where that is too much.  SP_CYCLIC_FPG sets the frames per group
 *      (a test hook: small shapes then walk the frame loop).
 *      x, y, S, Pp and Pm follow `mem`; device-resident arrays need only their natural alignment.
 *      Refused (< 0, sp_last_error() starts with "sp_cyclic: " and names the argument, the device is not touched, the outputs are
 *      untouched): n not a power of two in 32 .. 8192; hop < 1; nframes < 0; a frame outside the row ((nframes - 1) hop + n > nsig);
 *      A outside 1 .. 65535; batch outside 0 .. 65535; a nu that is not finite or has |nu| > 1; a dtype that is neither float32 nor
 *      complex64, y_dtype != x_dtype with y given; nb < 1 or > n, b0 outside 0 .. n - 1; a scale or a mean that is not finite;
 *      x_ld < nsig; first beyond +-2^62; x, w or nu NULL; S, Pp and Pm all NULL.
 *      batch == 0 or nframes == 0 returns 0 and launches nothing.
 *      sp_cyclic_plan (host only, never touches the device): out[5] = frames per group, workgroups over all passes, cycle
 *      frequencies per pass, passes, transforms per (frame, nu).  cross: y is given.  The CU count is the device's once the library is
 *      initialised and 256 before.  < 0 for a shape sp_cyclic refuses, or out NULL. */
int sp_cyclic(const void *x, const void *y, int x_dtype, int y_dtype, int64_t x_ld, int64_t nsig, int64_t batch, const float *w, int n,
              int64_t hop, int64_t nframes, int64_t first, const double *nu, int A, int conj, const double *mean_x, const double *mean_y,
              int b0, int nb, double scale, void *S, void *Pp, void *Pm, int mem);
int sp_cyclic_plan(int dtype, int cross, int conj, int n, int64_t hop, int64_t nframes, int A, int64_t batch, int64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
