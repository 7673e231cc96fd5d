/* spectral.h -- C ABI of libspectral.so: MI355X (gfx950) spectral-analysis kernels.
 *
 * This is the drop-in boundary underneath the Python modules in pyfft_amd/ that mirror
 * gmweir/PYFFT's numpy-array function signatures.  The reference has no FFI of its own
 * (it is pure Python over numpy.fft); each entry point below names the reference call
 * site(s) whose arithmetic it replaces.  Reference paths are relative to the reference
 * checkout (file:line).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Caller owns every buffer.
 *  - `mem`: 0 = all data pointers are host memory (library stages through its own device
 *    scratch, synchronously); 1 = all data pointers are device memory on the current
 *    device (nothing is copied; work is enqueued on the stream set by sp_set_stream and
 *    the call returns after enqueueing -- small parameter tables (window, filter taps)
 *    are ALWAYS host pointers.
 *  - complex = interleaved float re,im (numpy complex64).  Reduced spectra (Welch
 *    accumulators) are returned in double.
 *  - return value: 0 = ok, <0 = error; sp_last_error() gives the message (thread-local).
 *  - a call's results depend on its arguments alone, never on what the library ran before it (other shapes, NaN or huge
 *    samples, other streams), and a refused call leaves no trace.
 *  - one global context per process / one device per process (multi-GPU = one process per
 *    GPU, torch.distributed/RCCL reduces the accumulators; see pyfft_amd/dist.py).
 *  - Transform convention (dft.py:108-133, :242-290): forward unnormalised e^{-j2pi nk/N},
 *    inverse scaled 1/N.
 */
#ifndef SPECTRAL_H
#define SPECTRAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_DTYPE_F32 0 /* real float32 samples    */
#define SP_DTYPE_C64 1 /* complex64 samples (re,im) */

#define SP_SIDED_ONE 1 /* reference one-sided: bins [0,N/2), x2 on [1:-1] (Nyquist dropped; Q1) */
#define SP_SIDED_TWO 2 /* two-sided, fftshift-ed                                               */
#define SP_SIDED_RAW 3 /* two-sided, natural FFT order, no doubling                            */
#define SP_SIDED_HALF 4 /* bins 0..nfft/2 (numpy rfft layout), no doubling                        */

/* ---- context ------------------------------------------------------------------------ */
int sp_init(int device_id);          /* select device, create context (idempotent)          */
void sp_shutdown(void);              /* free plan cache + scratch                           */
const char *sp_last_error(void);
/* Concurrency contract: one global context under one lock -- calls from several threads serialise.  All launches go to
 * ONE stream (the one set last); scratch buffers, the device-table cache and the pending state between sp_welch_accum and
 * sp_welch_finish are shared by all calls.  sp_set_stream orders the new stream behind the work already queued on the
 * old one (event), so consecutive calls from different streams are safe; truly concurrent use from two streams is not
 * supported.  The table cache (windows, FFT(window), filter spectra; 64 entries, LRU) never evicts a table the current
 * call obtained nor the tables a pending sp_welch_accum holds. */
int sp_set_stream(void *hip_stream); /* hipStream_t for mem=1 calls (NULL = default stream) */
int sp_synchronize(void);            /* wait for the library's stream                       */
int sp_version(void);
int sp_max_wg_fft(void);             /* largest power-of-two FFT done inside one workgroup  */
/* Measurement hook: when enabled, the dominant kernel of each Welch call (k_welch) is bracketed by HIP events
 * recorded on the launch stream; sp_profile_last_ms() waits for them and returns the kernel's duration. */
int sp_profile_enable(int on);
int sp_profile_last_ms(double *ms);
const char *sp_profile_last_kernel(void); /* name of the kernel the last Welch call dispatched (also set by the pipeline paths of sp_stft_cog and sp_csd_matrix) */
/* device properties used by the host to size grids: out[0]=CU count, out[1]=LDS bytes/CU,
 * out[2]=clock kHz, out[3]=wavefront size */
int sp_device_info(int64_t out[4]);

/* ---- A7: fftanal.fft / .ifft  (fft_analysis.py:2096-2116 -> np.fft.fft/ifft) ---------- */
/* batch x n-point C2C transforms, rows contiguous.  n: any length >= 1 (powers of two up
 * to sp_max_wg_fft() run in one workgroup; longer powers of two use the multi-pass
 * four-step path; other lengths use Bluestein's chirp-z on top of those).
 * direction: -1 forward, +1 inverse (scaled 1/n). in == out allowed. */
int sp_fft_c2c(const void *in, void *out, int64_t n, int64_t batch, int direction, int mem);

/* ---- A3+A4: fftanal.fft_win -> Pstft -> averagewins (fft_analysis.py:2126-2203,
 *      :1944-1990), the fused Welch PSD: per frame g, X_g = FFT(win * (x[g*hop : g*hop+nfft] - trend));
 *      pxx[k] = scale/nframes * sum_g |X_g[k]|^2 with the sidedness permutation/doubling.
 *      nfft: any length >= 2.  Powers of two up to sp_max_wg_fft() and other lengths up to half of it run in ONE fused
 *      kernel (Bluestein inside the workgroup); longer segments -- the reference's default regime, Navr = 8 ->
 *      nwins = floor(nsig / 4.5), fft_analysis.py:2412-2418 -- go through the multi-kernel long-segment path (pack ->
 *      batched multi-pass FFT / chirp-z -> float64 accumulate; k_long.hip), up to a 2^26-point transform.  The same
 *      holds for sp_welch_csd, sp_stft and sp_stft_cog.
 *      detrend (global detrend over x[0:nsig], fft_analysis.py:2148, :2539-2549):
 *        SP_DETREND_CONST  (0) subtract the given constant mean_re + i mean_im (0,0 = no detrend),
 *        SP_DETREND_MEAN   (1) the library computes and subtracts the mean (one extra pass over x),
 *        SP_DETREND_LINEAR (2) the library fits and subtracts the least-squares line,
 *        SP_DETREND_SEGMEAN (3) every segment's own mean is removed before the window (the per-segment detrend of the
 *                              matplotlib.mlab estimators behind fft_analysis.psd/csd/coh, :1060-1155); sp_welch_psd,
 *                              sp_welch_csd, sp_stft (fft_win's detrendwin=True) and sp_stft_cog,
 *        SP_DETREND_SEGLINEAR (4) the same with every segment's own least-squares line.
 *      nbins = Nnyquist for SP_SIDED_ONE (nfft/2, or (nfft+1)/2 when odd), nfft otherwise. */
#define SP_DETREND_CONST 0
#define SP_DETREND_NONE 0 /* SP_DETREND_CONST for the entries that take no constant: nothing is subtracted */
#define SP_DETREND_MEAN 1
#define SP_DETREND_LINEAR 2
#define SP_DETREND_SEGMEAN 3
#define SP_DETREND_SEGLINEAR 4
int sp_welch_psd(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop,
                 int64_t nframes, int detrend, double mean_re, double mean_im, int sided,
                 double scale, double *pxx_out, int mem);

/* ---- the same path split in two for segment-sharded multi-process runs (one process per GPU): every process
 *      accumulates its own frames against a local estimate of the mean, the processes all-reduce sum_out (2 doubles)
 *      to get the global mean of the stream, and each finishes with it; the finished spectra (scaled by
 *      scale/frames_total) then add up to the Welch PSD of the whole stream.  Shapes: any segment of one workgroup
 *      transform (powers of two up to sp_max_wg_fft(), other lengths up to half of it) and any hop >= 1; a shard owns at
 *      most nframes*hop + nfft - 1 samples (nmean).  One accumulation may be pending at a time; x must
 *      stay valid until sp_welch_finish when mem=1.
 *      nmean: this shard's own samples x[0:nmean] (halo excluded) -> sum_out[2] = sum of them.
 *      mean: [2] doubles (host if mem=0, device if mem=1), or NULL = the shard's own mean sum_out/nmean. */
int sp_welch_accum(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                   int64_t nmean, double *sum_out, int mem);
int sp_welch_finish(const double *mean, int64_t frames_total, int sided, double scale, double *pxx_out, int mem);
/*      One-collective form of the same split.  sp_welch_export leaves this shard's ADDITIVE state in
 *      state[5*nfft + 8] (doubles): sum|X|^2, sum X and conj(mu0) sum X per bin (spectra taken against the shard's
 *      own mean estimate mu0), M mu0, M |mu0|^2, the sum of its nmean own samples, M and nmean.  The states of all
 *      shards are summed with ONE all-reduce and sp_welch_apply turns the sum into the PSD of the whole stream
 *      detrended by its global mean (same output conventions as sp_welch_finish).  Shapes: as sp_welch_accum. */
int sp_welch_export(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop,
                    int64_t nframes, int64_t nmean, double *state, int mem);
int sp_welch_apply(const double *state, const float *win, int nfft, int64_t frames_total, int sided, double scale,
                   double *pxx_out, int mem);

/* ---- the same path as a STREAM of steps, on one GPU or across the GPUs of one node, without the host in the loop (device
 *      pointers only).  SURVEY section 8b sketched `sp_init(device_count, device_ids)` + an `ngpu` argument; the MI355X-native
 *      form is one process per GPU with the library owning an RCCL communicator.
 *      Communicator (optional): every process sp_init(its device); rank 0 calls sp_comm_unique_id and hands the
 *      SP_COMM_ID_BYTES to the others by any means (the Python layer: one torch.distributed broadcast; a C host: MPI / a file /
 *      a socket); all call sp_comm_init(id, world, rank) (collective).  RCCL is resolved at run time (dlopen "librccl.so.1":
 *      the copy already in the process if there is one), so the library loads without it.
 *      sp_welch_dist_submit(step k): this shard's main kernel on the launch stream; its epilogue on the library's own stream
 *      behind an event -- without communicator the finished PSD, with one the shard's additive state (sp_welch_export), ONE
 *      ncclAllReduce (sum, double, 5 nfft + 8 values) and the sp_welch_apply, folded into the next step's epilogue launch --
 *      so the epilogue and the collective run BESIDE the next step's main kernel.  pxx_out[nbins] (device) receives THIS
 *      step's PSD of the whole stream; it is valid on the launch stream once a later call has reported it: *ndone = how many
 *      earlier submits' outputs became valid with this call, in submit order (without communicator: step k-1 at submit k;
 *      with: step k-2).  sp_welch_dist_flush reports the rest.  x, win contents and pxx_out of a step must stay alive until
 *      it is reported.  K submits + one flush = K Welch PSDs; no host synchronisation.  frames_total = frames of the WHOLE
 *      stream (the normalisation); nmean = this shard's own samples (halo excluded).  sp_welch_psd_dist = submit + flush.
 *      Shapes: as sp_welch_export.  Reference path: the same as sp_welch_psd (fft_analysis.py:2126-2203, :1944-1990) over
 *      segments dealt out to the ranks.
 *      With a communicator of more than one rank the library asks RCCL for at most 4 workgroups per collective
 *      (ncclCommInitRankConfig; SP_DIST_RCCL_CTAS) and partitions its main kernels over all but 8 CUs (SP_DIST_RESERVE_CUS), so
 *      that RCCL's kernel -- which cannot share a CU with the main kernel -- runs beside it instead of delaying the next one. */
#define SP_COMM_ID_BYTES 128
int sp_comm_unique_id(void *id_out /* SP_COMM_ID_BYTES */);
int sp_comm_init(const void *id, int world, int rank);
int sp_comm_info(int out[2] /* world (0 = no communicator), rank */);
int sp_comm_destroy(void);
int sp_welch_dist_submit(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                         int64_t nmean, int64_t frames_total, int sided, double scale, double *pxx_out, int *ndone);
int sp_welch_dist_flush(int *ndone);
int sp_welch_psd_dist(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                      int64_t nmean, int64_t frames_total, int sided, double scale, double *pxx_out);

/* ---- A5: fft_pwelch numeric core (fft_analysis.py:339-446): reference x against nch
 *      channels y[c][0:nsig] (channel-major, row stride y_ld samples).
 *      pxx[nbins], pyy[nch][nbins], pxy[nch][nbins] complex (re,im doubles) = Y_c * conj(X)
 *      (function-path conjugation, :393; the class path's X*conj(Y), :1960, is its conjugate).
 *      detrend as above (per signal); SP_DETREND_CONST subtracts mean_x / mean_y[nch] (NULL = 0). */
int sp_welch_csd(const void *x, const void *y, int dtype, int64_t nsig, int nch, int64_t y_ld,
                 const float *win, int nfft, int hop, int64_t nframes, int detrend,
                 const double *mean_x /*[2]*/, const double *mean_y /*[nch][2]*/, int sided,
                 double scale, double *pxx, double *pyy, double *pxy, int mem);

/* ---- cfg5: full cross-spectral-density matrix of nch real channels x[c][0:nsig]
 *      (generalises the ref x channel loop fft_analysis.py:387-393 / HeatPulse_Funcs.py:576-583).
 *      g_out[nfft/2+1][nch][nch] complex double, = scale/nframes * sum_g X_i conj(X_j), no doubling. */
int sp_csd_matrix(const float *x, int nch, int64_t nsig, int64_t x_ld, const float *win, int nfft,
                  int hop, int64_t nframes, int detrend, double scale, double *g_out, int mem);
/*      The same with the per-channel constants to remove given by the caller (HOST array means[nch], like
 *      mean_y of sp_welch_csd): a frame-sharded CSD matrix detrends every shard with the mean of the WHOLE
 *      record (fft_analysis.py:2148 semantics), obtained from sp_channel_means + an all-reduce. */
int sp_csd_matrix_means(const float *x, int nch, int64_t nsig, int64_t x_ld, const float *win, int nfft,
                        int hop, int64_t nframes, const double *means, double scale, double *g_out, int mem);
/*      means_out[c] = mean of x[c][0:nsig]  (nch real channels, row stride x_ld); means_out follows `mem`. */
int sp_channel_means(const float *x, int nch, int64_t nsig, int64_t x_ld, double *means_out, int mem);

/* ---- A8/A9: spectrogram.stft -> fftanal.fft_win (spectrogram.py:140-168, fft_analysis.py:2126-2203)
 *      and spectrogram.specgram (spectrogram.py:91-112).
 *      out_kind 0: complex64 amp_scale * X_g[k] (sqrt(2) on [1:-1] for SP_SIDED_ONE);
 *      out_kind 1: float32 power amp_scale * |X_g[k]|^2 (no doubling).
 *      out_major 0: [nframes][nbins] (fftanal Xseg); 1: [nbins][nframes] (specgram).
 *      pseg_out (may be NULL): float64[nframes] = trapz(|win*(x-mean)|^2) with unit spacing (:2174; host
 *      multiplies by dt and divides by S2). */
int sp_stft(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
            int detrend, double mean_re, double mean_im, int sided, double amp_scale, int out_kind,
            int out_major, void *out, double *pseg_out, int mem);

/* ---- inverse STFT: overlap-add synthesis, the inverse of sp_stft's frames (scipy.signal.istft's arithmetic).
 *      Frames Z_g, g = 0 .. M-1 (M = nframes), window win[0:nfft], 1 <= hop <= nfft:
 *        x_g    = ifft_nfft(Z_g)                                  (1/nfft normalisation)
 *        L      = (M-1)*hop + nfft
 *        num[n] = sum_g win[n - g*hop] * x_g[n - g*hop]           0 <= n < L
 *        env[n] = sum_g win[n - g*hop]^2
 *        y[n]   = scale * num[n] / env[n]  where env[n] > 1e-10,  scale * num[n] elsewhere
 *      and the call writes y[skip : skip + nout].  scale = sum(win), skip = nfft/2, nout = L - 2*(nfft/2) is
 *      scipy.signal.istft(boundary=True); skip = 0, nout = L is boundary=False.
 *      sided SP_SIDED_HALF: one-sided spectra, nb = nfft/2 + 1 bins, y float32 (the imaginary parts of bin 0 and, for even
 *      nfft, bin nfft/2 are ignored as irfft does); SP_SIDED_RAW: two-sided spectra in fftfreq order, nb = nfft, y complex64.
 *      in_major 0: Z[nch][M][nb] (sp_stft's out_major 0), 1: Z[nch][nb][M] (out_major 1, scipy's layout).
 *      nch >= 1 independent records, contiguous: y[nch][nout].
 *      nfft: what runs in one workgroup transform (powers of two up to sp_max_wg_fft(), other lengths up to half of it).
 *      env is summed in float64 on the host.  No atomics: every output sample is summed by one workgroup in frame order, so the
 *      result is bitwise reproducible.  A bad argument returns < 0 with sp_last_error() set and leaves y untouched.
 *      Every pointer but win follows `mem`. */
int sp_istft(const void *Z, int sided, int in_major, int nch, int64_t nframes, const float *win, int nfft, int hop,
             double scale, int64_t skip, int64_t nout, void *y, int mem);

/* ---- bispectrum and bicoherence (Kim & Powers 1979) over the frames of sp_stft: frame g = win * (x[g*hop : g*hop+nfft] - trend),
 *      detrend SP_DETREND_CONST (mean_re + i mean_im), SP_DETREND_MEAN or SP_DETREND_LINEAR over the whole record, unnormalised
 *      forward FFTs X_g, Y_g, Z_g of x, y, z.  Real float32 input: bins 0 .. nfft/2 (SP_SIDED_HALF), nb = nfft/2 + 1, sum bin
 *      s = i + j; complex64 input: two-sided fftshift-ed bins (SP_SIDED_TWO, bin nfft/2 is frequency 0), nb = nfft,
 *      s = i + j - nfft/2.  A pair (i, j) is valid when 0 <= s < nb.  With M = nframes, on the nb x nb grid:
 *        B_out[i][j]  = (1/M) sum_g X_g(i) Y_g(j) conj(Z_g(s))          complex128
 *        b2_out[i][j] = |B|^2 / (D P[s]), D = (1/M) sum_g |X_g(i) Y_g(j)|^2; 0 where D P = 0
 *        pzz_out[s]   = P[s] = (1/M) sum_g |Z_g(s)|^2                    float64 [nb], may be NULL
 *      B and b2 are NaN outside the valid region.  y = z = NULL: the auto bispectrum of x (computed for j <= i and mirrored:
 *      exactly symmetric); otherwise y and z (NULL = x) are records of x's length and dtype.  8 <= nfft <= 4096.  Every
 *      pointer follows `mem`.  Deterministic: the frame sums are reduced in a fixed order. */
int sp_bispectrum(const void *x, const void *y, const void *z, int x_dtype, int64_t nsig, const float *win, int nfft, int hop,
                  int64_t nframes, int detrend, double mean_re, double mean_im, void *B_out, double *b2_out, double *pzz_out,
                  int mem);

/* ---- Thomson multitaper spectra: the frames of sp_welch_psd / sp_welch_csd under K tapers in ONE pass over the record:
 *        X_{g,k} = FFT(tapers[k] * (x[g*hop : g*hop+nfft] - trend)), Y_{g,k} likewise (y = NULL: the PSD only)
 *        weights == NULL:  pxx[f] = scale/nframes * sum_k sum_g |X_{g,k}[f]|^2, pyy likewise, pxy = ... conj(X_{g,k}) Y_{g,k}
 *                          (the caller folds sqrt(c_k) / sqrt(sum tapers[k]^2) into the taper rows)
 *        weights != NULL:  the eigenspectra skx[k][f] = scale/nframes * sum_g |X_{g,k}[f]|^2 (sky likewise; float64 [K][nb], required)
 *                          and pxx = sum_k c_k skx[k], pyy, pxy likewise, c = weights / sum(weights), all in float64
 *                          (the caller folds only 1 / sqrt(sum tapers[k]^2) into the rows; weights: K host doubles >= 0, not all 0)
 *      tapers: HOST float32 [K][nfft] (device table cache, like the windows), 1 <= K <= 32.  nfft: 8 .. what one workgroup
 *      transform takes (powers of two up to sp_max_wg_fft(), other lengths up to half of it).  detrend SP_DETREND_CONST (mean_x /
 *      mean_y: 2 doubles re, im, or NULL for none), SP_DETREND_MEAN or SP_DETREND_LINEAR over the whole record.
 *      Outputs in float64, raw bin order, nothing doubled: real float32 input -> bins 0 .. nfft/2 (SP_SIDED_HALF, nb = nfft/2 + 1),
 *      complex64 input -> natural FFT order (SP_SIDED_RAW, nb = nfft); pxy is [nb][2] (re, im).  pyy, pxy, sky are not touched when
 *      y == NULL.  x, y and the outputs follow `mem`.  No atomics: group partials are summed in float64 in a fixed order, so two calls
 *      agree bitwise.  A bad argument returns < 0 with sp_last_error() set before the device is touched. */
int sp_multitaper(const void *x, const void *y, int dtype, int64_t nsig, const float *tapers, int ntapers, int nfft, int hop,
                  int64_t nframes, int detrend, const double *mean_x, const double *mean_y, const double *weights, double scale,
                  double *pxx, double *pyy, double *pxy, double *skx, double *sky, int mem);

/* ---- Chirp-z transform on an arc of the unit circle (scipy.signal.czt / zoom_fft with |w| = |a| = 1):
 *        X[k] = sum_{j<n} x[j] exp(-2 pi i (start + k step) j),  k < m;   start, step in cycles per sample (float64)
 *      so start = f1 / fs and step = (f2 - f1) / (m fs) give m bins over [f1, f2).  Bluestein: two L-point transforms,
 *      L = next_pow2(n + m - 1), inside one workgroup up to L = sp_max_wg_fft() and through the multi-pass transform up to 2^26.
 *      sp_czt: batch rows of n float32 / complex64 samples (row stride x_ld >= n) -> out[batch][m] complex64; x and out follow `mem`.
 *      sp_zoom_welch: the frames of sp_welch_psd / sp_welch_csd (win: HOST float32 [nfft]; detrend SP_DETREND_CONST with mean_x /
 *      mean_y = 2 doubles or NULL, SP_DETREND_MEAN or SP_DETREND_LINEAR over the whole record), each transformed on the arc:
 *        frames != NULL:  frames[g][k] = scale X_g[k], complex64 [nframes][m] (y must be NULL; pxx, pyy, pxy are not touched)
 *        otherwise:       pxx[k] = scale / nframes sum_g |X_g[k]|^2 and, with y, pyy likewise and pxy[k] = ... conj(X_g[k]) Y_g[k]
 *                         as [m][2]; float64, nothing doubled; pyy and pxy are not touched when y == NULL
 *      x, y and the outputs follow `mem`.  No atomics: partial sums are reduced in float64 in a fixed order, so two calls agree
 *      bitwise.  Refused (< 0, the message names the entry point, the device is not touched): n or nfft < 1, m < 1, a start or step
 *      that is not finite, n + m - 1 beyond 2^26 points after rounding up to a power of two, hop < 1, frames that overrun the record.
 *      sp_czt_chirp: the table phases for checking, host only (no device call): cs_out[c] = (cos, sin) of
 *      exp(-2 pi i (start i + step i^2 / 2)) at i = i0 + c, c < count, reduced modulo one turn in 128-bit fixed point. */
int sp_czt(const void *x, int x_dtype, int64_t n, int64_t x_ld, int64_t batch, int64_t m, double start, double step, void *out,
           int mem);
int sp_zoom_welch(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                  int detrend, const double *mean_x, const double *mean_y, int64_t m, double start, double step, double scale,
                  double *pxx, double *pyy, double *pxy, void *frames, int mem);
int sp_czt_chirp(int64_t i0, int64_t count, double step, double start, float *cs_out);

/* ---- Digital down-converter: mix with a carrier, low-pass, decimate -- one pass over every row of a batch:
 *        v[n] = x[n] exp(-2 pi i nu (n0 + n)),  n < nsig, 0 outside the row;   nu in cycles per sample (float64)
 *        y[k] = sum_{j<ntaps} h[j] v[k q + (ntaps - 1) / 2 - j],  k < ceil(nsig / q)
 *      which is scipy.signal.resample_poly(v, 1, q, window=h) for an odd ntaps.  x: float32 or complex64 rows of nsig samples, row
 *      stride x_ld >= nsig; h: HOST float32 [ntaps], real; out: complex64 [batch][ceil(nsig / q)]; x and out follow `mem`.
 *      n0 is the absolute index of every row's first sample: the chunks of one stream, each with its own n0, continue the oscillator
 *      without a phase jump.  nu n0 is reduced modulo one turn in 128-bit fixed point on the host and advanced on the device in
 *      64-bit fixed point (<= 2^-33 turns over a launch); nu = 0 (or any integer) skips the mixer and filters the input as it is.
 *      Limits of one launch: 1 <= q <= 64; ntaps odd, 1 .. 4095; 1 <= nsig <= 2^32; |n0| <= 2^40; nu and h finite.
 *      Anything else returns < 0 with sp_last_error() naming the entry point, before the device is touched.
 *      sp_ddc_tile: the outputs one workgroup of sp_ddc produces for this q (0 outside 1 .. 64); a tile consumes q times as many
 *      samples.  Host only. */
int sp_ddc(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, double nu, int64_t n0, int q, const float *h,
           int ntaps, void *out, int mem);
int sp_ddc_tile(int q);

/* ---- Rational resampler (scipy.signal.upfirdn): zero-stuff by `up`, filter with h, keep every `down`-th sample -- one pass over
 *      every row of a batch.  With xu[i up] = x[i] for 0 <= i < nsig and xu = 0 elsewhere,
 *        y[m] = sum_{j<ntaps} h[j] xu[m down - j] = sum_p h[phi + p up] x[i0 - p],   i0 = floor(m down / up), phi = (m down) mod up
 *        out[b][k] = y_b[m0 + k],  k < nout,  row stride nout.
 *      x: float32 or complex64 rows of nsig samples, row stride x_ld >= nsig; h: HOST float32 [ntaps], real; out has the dtype of x
 *      (real rows stay real); x and out follow `mem`.  Outputs beyond the full length ceil(((nsig - 1) up + ntaps) / down) are zero
 *      by the definition, not an error.  The caller reduces up / down by their gcd.  No atomics, a fixed summation order: two calls
 *      agree bitwise.  nout = 0 or batch = 0 returns 0 and launches nothing.
 *      Limits of one launch: 1 <= up, down <= 256; 1 <= ntaps <= 8191; h finite; nsig >= 1; m0, nout >= 0;
 *      (m0 + nout) down < 2^62; batch * ceil(nout / tile) fits 31 bits.
 *      Anything else returns < 0 with sp_last_error() naming sp_upfirdn, before the device is touched, and leaves out untouched.
 *      sp_upfirdn_tile: the outputs one workgroup produces for this shape (cplx != 0: complex64 rows), 0 outside the limits.
 *      Host only. */
int sp_upfirdn(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, const float *h, int ntaps, int up, int down,
               int64_t m0, int64_t nout, void *out, int on_device);
int sp_upfirdn_tile(int up, int down, int ntaps, int cplx);

/* ---- Polyphase filter-bank channelizer (weighted overlap-add DFT bank): every row of a batch split into M uniformly spaced
 *      bands under a prototype filter of ntaps = P*M real taps, longer than the transform.  For one row x[0:nsig], zero outside
 *      the row, and frame m = 0 .. nframes-1 with s = first + m*hop (first: the row index of frame 0's first sample, may be < 0):
 *        X[m][k] = sum_{n<ntaps} h[n] * x[s+n] * exp(-2 pi i k (n + rho_m) / M),   k < M
 *        rho_m   = 0                       phase_ref 0 ("frame": bin P*k of an ntaps-point STFT under the window h)
 *        rho_m   = (r0 + m*hop) mod M      phase_ref 1 ("time": the caller passes r0 = (n0 + first) mod M, n0 the absolute index of
 *                                          the row's sample 0; a tone at k/M cycles per sample is then constant in channel k)
 *      computed as a fold and ONE M-point transform:  u[i] = sum_{p<P} h[p*M+j] * x[s+p*M+j],  j = (i - rho_m) mod M,
 *      X[m][:] = FFT_M(u); the sum over p runs in the order p = 0 .. P-1 with fused multiply-adds.  Each channel is a baseband
 *      series with one sample per hop input samples.
 *      x: float32 or complex64 rows of nsig samples, row stride x_ld >= nsig; h: HOST float32 [ntaps] (device table cache, like
 *      the windows); complex input -> nb = M bins in natural FFT order; real input -> the bins 0 .. M/2, nb = M/2 + 1.
 *      out_kind 0: the frames, complex64, out_major 0 = [batch][nframes][nb], 1 = [batch][nb][nframes] (scipy's layout); scale is
 *                  not applied.  A frame's bits do not depend on how the frames are dealt out to workgroups, nor on the other
 *                  frames of the call.
 *      out_kind 1: the accumulated power pxx[batch][nb] = scale/nframes * sum_m |X[m][k]|^2, float64, nothing doubled (out_major
 *                  ignored).  No atomics: group partials are summed in float64 in a fixed order, so two calls agree bitwise.
 *      x and out follow `mem`.
 *      Limits of one launch: M a power of two, 2 .. sp_max_wg_fft(); ntaps = P*M with 1 <= P <= 32; hop >= 1; nframes >= 1;
 *      0 <= r0 < M; h and scale finite; every frame touches at least one sample of the row (first > -ntaps and
 *      first + (nframes-1)*hop < nsig); x_ld >= nsig >= 1; batch * ceil(nframes / frames per workgroup) fits 31 bits.
 *      out_major 1: nframes <= 65535*32.
 *      Anything else returns < 0 with sp_last_error() naming sp_pfb, before the device is touched, and leaves out untouched. */
int sp_pfb(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, const float *h, int ntaps, int M, int hop,
           int64_t first, int64_t nframes, int phase_ref, int r0, int out_kind, int out_major, double scale, void *out, int mem);

/* ---- Polyphase synthesis bank: the adjoint of sp_pfb's fold, the way back from its frames to a waveform.  Same symbols as sp_pfb:
 *      frames X[m][k], m < nframes, on M channels, s_m = first + m*hop, rho_m = 0 (phase_ref 0) or (r0 + m*hop) mod M (phase_ref 1),
 *      a synthesis prototype g[0:ntaps], ntaps = P*M:
 *        v_m[i] = sum_{k<M} X[m][k] * exp(+2 pi i k i / M)                     (unnormalised inverse transform)
 *        y[a]   = sum_{m : 0 <= a - s_m < ntaps} tap[a - s_m] * v_m[(a - s_m + rho_m) mod M],   0 <= a < nout
 *        tap[n] = float32(g[n] * scale / M)                                    (rounded once on the host)
 *      The sum over m runs in ascending frame order from zero with one fused multiply-add per component, which fixes a sample's bits:
 *      they depend neither on how the frames are dealt out to workgroups nor on the path (below), and two calls agree bitwise.
 *      Frames that lie partly or wholly outside [0, nout) contribute what falls inside; a sample that no frame reaches is zero; every
 *      one of the nout samples is written.  With the analysis prototype h of sp_pfb and scale = 1,
 *      y[a] = sum_q T[q][(a - first) mod hop] * x[a + q*M], T[q][r] = sum_j g[r + j*hop] * h[r + j*hop + q*M], on the samples whose
 *      frames all belong to the call: g reconstructs when T = delta_q (pyfft_amd.channelizer.pfb_dual designs such a g for hop < M).
 *      sided SP_SIDED_HALF: nb = M/2 + 1 bins, Hermitian-extended, the imaginary parts of bins 0 and M/2 ignored -> y float32;
 *      SP_SIDED_RAW: nb = M bins in natural FFT order -> y complex64.  in_major 0: X[batch][nframes][nb]; 1: X[batch][nb][nframes]
 *      (sp_pfb's two out_major layouts; the second is transposed into library scratch of the input's size).  g: HOST float32 [ntaps]
 *      (device table cache, like the windows); X and y follow `mem`; y is [batch][nout].
 *      Two paths with the same bits: where the exchange images and a ring of ntaps accumulators per transform group fit the 160 KiB
 *      of LDS a workgroup may take, one fused kernel overlap-adds in LDS (no scratch, no atomics); otherwise the inverse transforms go
 *      to library scratch [batch][nframes][M] and a second kernel sums every output sample from the frames that reach it.
 *      Limits of one launch: M a power of two, 2 .. sp_max_wg_fft(); ntaps = P*M with 1 <= P <= 32; hop >= 1; nframes >= 1; nout >= 1;
 *      batch >= 0; 0 <= r0 < M; g, scale and every tap finite; |first|, nframes*hop and nout within 2^40;
 *      batch * ceil(nframes / frames per workgroup) fits 31 bits; X, g and y not NULL.
 *      Anything else returns < 0 with sp_last_error() naming sp_pfb_synth, before the device is touched, and leaves y untouched. */
int sp_pfb_synth(const void *X, int sided, int in_major, int64_t batch, int64_t nframes, const float *g, int ntaps, int M, int hop,
                 int64_t first, int phase_ref, int r0, double scale, int64_t nout, void *y, int mem);
/*      sp_pfb_synth_plan: what sp_pfb_synth would do by default at this shape, for tools: out[5] = { 1 fused / 0 composed, the transform
 *      groups of a workgroup whose ring fits the LDS (0: not one), the groups per workgroup, the frames per run of the fused path, its
 *      halo frames }.  Initialises the device (the run length depends on its CU count); SP_PFBS_PATH and SP_PFBS_FPG are not applied. */
int sp_pfb_synth_plan(int sided, int64_t batch, int64_t nframes, int ntaps, int M, int hop, int64_t *out);

/* ---- N3: Doppler.cog applied per STFT frame (Doppler.py:43-58; the loop body of cogspec, Doppler.py:73-81):
 *      cog_out[g] = sum_k f_k |X_g[k]|^2 / sum_k |X_g[k]|^2 over the two-sided spectrum of frame g, f_k = fftfreq(nfft, 1/fs),
 *      restricted to fmin <= |f_k| <= fmax (fmin = 0, fmax >= fs/2: every bin); 0 where the band holds no power.  The
 *      spectrogram is never written: the moments are reduced inside the transform kernel.  float64[nframes], follows `mem`.
 *      Frame g = win * detrended x[g*hop : g*hop+nfft]; a boxcar window with SP_DETREND_CONST (0,0) is cog(x[frame], fs). */
int sp_stft_cog(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                int detrend, double mean_re, double mean_im, double fs, double fmin, double fmax, double *cog_out, int mem);

/* ---- A10: hilbert.hilbert / hilbert_1d (hilbert.py:22-112): rows of n_in real samples (row stride
 *      x_ld), transform length nfft (zero-pad / truncate like np.fft.fft(n=nfft)), one-sided mask with the
 *      reference's odd-length convention (bin nyq untouched), inverse; out[batch][nfft] complex64. */
int sp_hilbert(const float *x, int64_t n_in, int64_t x_ld, int64_t nfft, int64_t batch, void *out, int mem);

/* ---- A5, nT-model branch of fft_pwelch (fft_analysis.py:169-176, :346-393: a one-window model signal against every
 *      window of the long channels): out[ch][n] = sum_g detrended(x[ch][g*hop + n]), n < nfft -- the time-domain sum of
 *      all frames, from which sum_g FFT(win * frame_g) = FFT(win * out) follows by linearity (no spectrum is written).
 *      nch channels with row stride x_ld; detrend 0 none, 1 each channel's mean over [0:nsig], 2 its least-squares line;
 *      out float64 [nch][nfft][2] (re, im), follows `mem`. */
int sp_frame_sum(const void *x, int x_dtype, int64_t nsig, int nch, int64_t x_ld, int nfft, int hop, int64_t nframes,
                 int detrend, double *out, int mem);

/* ---- N4: frequency-domain response applied to real rows: out = IFFT(H * FFT(x, nfft)) -- the transform pair of
 *      fft_deriv (fft_analysis.py:1526-1546: `real(ifft(wavenumber * fft(sig)))`), the Hilbert kernel with the mask
 *      replaced by a table.  H: complex64[nfft], always a HOST array (like the window tables); x rows of n_in real
 *      samples (row stride x_ld), zero-padded / truncated to nfft; out[batch][nfft] complex64 (x, out follow `mem`). */
int sp_spectral_filter(const float *x, int64_t n_in, int64_t x_ld, int64_t nfft, int64_t batch, const void *H, void *out,
                       int mem);

/* ---- A11: ccf.ccf (ccf.py:66-77): normalised cross-covariance of two real length-n signals at all
 *      2n-1 lags, via zero-padded FFTs; co_out[2n-1] float32 in np.correlate(...,'full') order. */
int sp_xcorr(const float *x1, const float *x2, int64_t n, float *co_out, int mem);

/* ---- Short-time cross-correlation (ccf.ccf_sh, ccf.py: the correlation inside a sliding window, averaged over the windows; the
 *      window layout is this build's: complete windows at a fixed hop) and the delay track read off it.
 *      Two records x, y of nsig samples, both float32 or both complex64.  Frame g < nframes takes a = x[g hop : g hop + nw] and b
 *      likewise from y, (nframes - 1) hop + nw <= nsig.  detrend SP_DETREND_SEGMEAN subtracts each window's own mean from a and from b
 *      (the reference's ccf), SP_DETREND_CONST subtracts nothing.  An optional taper win[nw] then multiplies a and b (NULL: boxcar).
 *      With L = max(32, next_pow2(nw + maxlag)), 0 <= maxlag <= nw - 1:
 *        A = FFT_L(a), B = FFT_L(b)  (zero-padded, unnormalised);   S[k] = A[k] conj(B[k]);   E = sqrt(sum |a|^2 * sum |b|^2)
 *        beta == 0:  S'[k] = W[k] S[k];  c = IFFT_L(S')        norm SP_XC_RAW
 *                                        c = IFFT_L(S') / E    norm SP_XC_COEFF  (a frame with E = 0 gives 0)
 *        beta  > 0:  S'[k] = W[k] S[k] / (|S[k]| + beta E);  c = IFFT_L(S')   regularised PHAT, norm must be SP_XC_COEFF
 *        c_g[l] = c[l mod L],  -maxlag <= l <= maxlag,  stored at index l + maxlag
 *      so that with W = 1 and beta = 0, c_g[l] = sum_n a[n + l] conj(b[n]): the order of np.correlate(a, b, 'full') and of sp_xcorr.
 *      weight: W, an optional HOST float32 table of L real weights in natural FFT order (NULL: all ones): band limits, or SCOT / ML
 *      weights from averaged spectra.  For real input only the real part of the inverse transform is kept, so the table must be even,
 *      W[k] == W[L - k]; one that is not is refused.  win and weight go through the device table cache, like the windows.
 *      Outputs, each may be NULL, at least one is required, one launch serves them all:
 *        frames  [nframes][2 maxlag + 1], float32 for real input, complex64 for complex input
 *        avg     float64 [2 maxlag + 1] ([..][2] re, im for complex input): the mean of c_g over the frames (ccf_sh's csh).  Transform
 *                groups accumulate their run of frames in float32 registers, a finish kernel sums the partials in float64 in a fixed
 *                order: no atomics, two calls agree bitwise.
 *        peak    float32 [nframes][2].  q[l] = c[l] (real input) or |c[l]| (complex input); l* = the smallest l attaining max q;
 *                d = q[l*-1] - 2 q[l*] + q[l*+1];  delta = (q[l*-1] - q[l*+1]) / (2 d) if |l*| < maxlag and d < 0, else 0;
 *                peak[g] = (l* + delta, q[l*] - (q[l*-1] - q[l*+1]) delta / 4): the parabola through the top three lags.
 *      x, y and the three outputs follow `mem`.  Real input costs one forward (z = a + i b) and one inverse transform per frame, complex
 *      input two forward and one inverse, all inside one workgroup.
 *      Refused (< 0, sp_last_error() names sp_xcorr_frames, the device is not touched, the outputs are untouched): nw < 2; maxlag outside
 *      [0, nw - 1]; L > sp_max_wg_fft(); hop < 1; nframes < 1; frames that overrun the record; an unknown dtype, detrend or norm;
 *      beta < 0 or not finite; beta > 0 with SP_XC_RAW; x or y NULL; all three outputs NULL; a weight that is not even with real input.
 *      sp_xcorr_frames_len: L for this (nw, maxlag), or < 0 where sp_xcorr_frames would refuse them.  Host only. */
#define SP_XC_RAW 0
#define SP_XC_COEFF 1
int sp_xcorr_frames(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nw, int hop, int64_t nframes,
                    int maxlag, int detrend, int norm, double beta, const float *weight, void *frames, double *avg, float *peak,
                    int mem);
int sp_xcorr_frames_len(int nw, int maxlag);

/* ---- Two-point wavenumber-frequency spectrum S(k, f) (Beall, Kim & Powers 1982; build-defined, the reference has no counterpart).
 *      Two records x, y of nsig samples, both float32 or both complex64, from probes a distance dx apart.  Frame g < nframes is
 *      a = win (x[g hop : g hop + nfft] - m), b likewise from y, (nframes - 1) hop + nfft <= nsig; m is the frame's own mean
 *      (SP_DETREND_SEGMEAN) or 0 (SP_DETREND_NONE); win is a HOST float32 [nfft] (device table cache) or NULL (boxcar).  X, Y are the
 *      unnormalised forward transforms, nfft a power of two in 32 .. 4096.  For every frame and every bin f of the band:
 *        theta = arg(X[f] conj(Y[f])) in [-pi, pi]    (y[n] = x[n - d] gives theta = +2 pi f d / fs for f > 0);  theta = k dx
 *        j = floor((theta / 2 pi + 1/2) nk) mod nk     (nk equal bins over [-pi, pi); theta = pi wraps to bin 0), 2 <= nk <= 1024
 *        p = (|X|^2 + |Y|^2) / 2  (SP_SKF_MEAN)   or   |X| |Y|  (SP_SKF_CROSS)
 *        s_out[f - b0][j] = scale / nframes * sum_g p          float64 [nb][nk], nothing doubled
 *      so that sum_j s_out[.][j] is (Pxx + Pyy) / 2 of sp_welch_csd at the same scale (SP_SKF_MEAN).  The band is the nb bins from b0
 *      on in natural FFT order: b0 + nb <= nfft / 2 + 1 for real input; for complex input counted modulo nfft, so that it may run
 *      through zero (b0 = 200, nb = 112 at nfft = 256 is bins 200 .. 255, 0 .. 55).  Bin j is centred on the wavenumber
 *      k_j = (j + 1/2 - nk / 2) 2 pi / (nk dx).
 *      The histogram of a workgroup's run of frames lives in LDS, every cell with one writer and a fixed order of additions; float32
 *      partials per run are summed in float64 in a fixed order: no atomics on memory, two calls agree bitwise.  A band with more cells
 *      nb x nk than the LDS tile holds is cut into frequency tiles and the transforms are repeated per tile (sp_skf_plan).
 *      x, y and s_out follow `mem`.
 *      Refused (< 0, sp_last_error() names sp_skf, the device is not touched, s_out is untouched): nfft not a power of two in
 *      32 .. 4096; nk outside 2 .. 1024; nb < 1 or a band outside the bins; hop < 1; nframes < 1; frames that overrun the record; a
 *      dtype other than float32 / complex64; a detrend other than NONE / SEGMEAN; an unknown power; a scale that is not finite; x, y
 *      or s_out NULL.
 *      sp_skf_plan (host only): out[4] = frequency tiles, bins per tile, LDS bytes of a workgroup, transforms per frame (tiles for
 *      real input, 2 tiles for complex); < 0 for an nfft, nk or nb that sp_skf refuses. */
#define SP_SKF_MEAN 0
#define SP_SKF_CROSS 1
int sp_skf(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes, int detrend,
           int power, int b0, int nb, int nk, double scale, double *s_out, int mem);
int sp_skf_plan(int cplx, int nfft, int nb, int nk, int64_t *out);

/* ---- Time-resolved Welch spectra (build-defined; the reference's __init__.py tries to import CECE for this question): the PSD of x,
 *      and with y the PSDs of nch records y_c (row c at y + c y_ld, y_ld >= nsig) and their cross spectra with x, over blocks of navg
 *      consecutive frames, block after block along the record: the running spectra behind a coherogram and a running cross-phase.
 *      Frame g < nframes is a_g = win (x[g hop : g hop + nfft] - m_g), b_g likewise from y_c, (nframes - 1) hop + nfft <= nsig; m_g is
 *      the frame's own mean (SP_DETREND_SEGMEAN, scipy's detrend='constant') or 0 (SP_DETREND_NONE); win is a HOST float32 [nfft]
 *      (device table cache) or NULL (boxcar); X_g, Y_g are the unnormalised forward transforms, nfft a power of two in
 *      32 .. sp_max_wg_fft().  Block b < nblocks = (nframes - navg) / step + 1 holds the frames b step .. b step + navg - 1:
 *        pxx[b][k]    = s_k / navg sum_g |X_g[k]|^2                 float32 [nblocks][nb]
 *        pyy[c][b][k] = s_k / navg sum_g |Y_g[k]|^2                 float32 [nch][nblocks][nb]
 *        pxy[c][b][k] = s_k / navg sum_g conj(X_g[k]) Y_g[k]        complex64 [nch][nblocks][nb]   (scipy.signal.csd's conjugation)
 *      s_k = scale; for float32 records with doubled != 0 twice that on the bins 1 .. nfft/2 - 1.  float32 records give the bins
 *      0 .. nfft/2 (nb = nfft/2 + 1), complex64 records the natural FFT order (nb = nfft), nothing doubled.  So block b is
 *      scipy.signal.welch / csd of the samples b step hop .. b step hop + (navg - 1) hop + nfft - 1 with nperseg = nfft and
 *      noverlap = nfft - hop.  step == navg: disjoint blocks; step < navg: overlapping blocks; step > navg: gaps.  Frames left over
 *      behind the last block are not used.
 *      One kernel forms the sums of runs of q frames inside its frame loop (q = navg for step >= navg, then it writes the outputs;
 *      else q = gcd(navg, step), float32 run sums, and a second kernel adds the navg / q runs of every block in float64): every
 *      frame is transformed once whatever the block overlap.  Every record has its own transform (float32 records as a + 0i), so a
 *      channel 10^4 below the other keeps its own accuracy, a single frame's coherence is 1 to rounding, and pxx is bitwise the
 *      same whatever y and nch are.  No atomics: every value has one writer and a
 *      fixed order of additions that does not depend on where in the record the block lies -- two calls agree bitwise, and so does
 *      a block with block 0 of the call on the record cut to start there.
 *      x, y and the outputs follow `mem`.
 *      Refused (< 0, sp_last_error() names sp_welch_blocks and the argument, the device is not touched, the outputs are untouched):
 *      nfft not a power of two in 32 .. sp_max_wg_fft(); hop < 1 or hop > nfft; navg < 1; step < 1; nframes < navg; nsig shorter than
 *      (nframes - 1) hop + nfft; with y: nch < 1, nch > 65535 or y_ld < nsig; a dtype other than float32 / complex64; a detrend
 *      other than NONE / SEGMEAN; a scale that is not finite; x or pxx NULL; pyy or pxy NULL when y is given.
 *      sp_welch_blocks_plan (host only; nch = 0: no y): out[8] = nblocks, nb, q, runs, transforms (frames transformed x 2 pairs, x and
 *      y_c of every pair (x 4 pairs for complex64 pairs at 8192 points, whose bins two workgroups share), or x 1 without y; frames
 *      transformed = runs x q = nframes when neither gaps nor leftovers exist), scratch bytes (the run
 *      sums), workgroups, LDS bytes of a workgroup.  The CU count behind the workgroups is the device's once the library is
 *      initialised and 256 before.  < 0 for a shape that sp_welch_blocks refuses, or out NULL. */
int sp_welch_blocks(const void *x, const void *y, int dtype, int64_t nsig, int nch, int64_t y_ld, const float *win, int nfft, int hop,
                    int64_t nframes, int navg, int step, int detrend, double scale, int doubled, float *pxx, float *pyy, void *pxy,
                    int mem);
int sp_welch_blocks_plan(int cplx, int nfft, int hop, int64_t nframes, int navg, int step, int nch, int64_t out[8]);

/* ---- Continuous wavelet transform by overlap-save (Torrence & Compo 1998, analytic wavelets): for every row of a batch and every scale
 *      s' (in samples)
 *        W[s][n] = sum_m g_s[m] x[n - m]  over the zero-extended row (a linear convolution, no wrap-around),  g_s = IDFT(H_s),
 *        H_s[k]  = sqrt(2 pi s') psi0^(s' w_k),  w_k = 2 pi k / L for 0 < k <= L/2,  0 at k = 0 and k > L/2
 *        family SP_CWT_MORLET (p0 = w0 > 0):   psi0^(u) = pi^(-1/4) exp(-(u - w0)^2 / 2)
 *        family SP_CWT_PAUL   (p0 = m >= 1):   psi0^(u) = 2^m / sqrt(m Gamma(2m)) u^m exp(-u);   p1 is reserved and must be 0.
 *      Frames of L samples, L a power of two in 256 .. 8192; frame g covers the samples [g hop - M, g hop - M + L), hop = L - 2 M, and
 *      yields the samples g hop .. g hop + hop - 1: the caller chooses the margin M so that |g_s| beyond +-M is negligible for every scale
 *      of the call.  One forward transform per frame (and scale chunk), one filtered inverse transform per scale, the filter evaluated
 *      on the fly.  x: float32 or complex64 rows of nsig samples, row stride x_ld >= nsig (float32 rows run as x + 0i); scales: HOST
 *      float64 [nscales].  Outputs, any combination, NULL skips one (at least one is required):
 *        W        complex64 [batch][nscales][nsig]
 *        gws      float64   [batch][nscales]   sum_n |W[s][n]|^2: float32 sums per frame, added in float64 in frame order
 *        recon    complex64 [batch][nsig]      sum_s wrec[s] W[s][n]        (wrec: HOST float32 [nscales], required with recon)
 *        bandpow  float32   [batch][nsig]      sum_s wband[s] |W[s][n]|^2   (wband: HOST float32 [nscales], required with bandpow)
 *      recon and bandpow are accumulated in registers across the scale loop and written once: W is never formed.  No atomics, a fixed
 *      order of additions: two calls agree bitwise, and W does not depend on how the scales are dealt to workgroups.
 *      x and the outputs follow `mem`; a device-resident x needs only its natural alignment.
 *      Refused (< 0, sp_last_error() names sp_cwt, the device is not touched, the outputs are untouched): L not a power of two in
 *      256 .. 8192; M < 0, 2 M >= L or hop < L / 4; nscales < 1; a scale that is not positive or not finite; an unknown family or a
 *      parameter outside its range; an unknown dtype; nsig < 1, batch < 0, batch > 65535, x_ld < nsig; no output; recon without wrec or
 *      bandpow without wband, or weights that are not finite; x or scales NULL.  batch == 0 returns 0 and launches nothing.
 *      sp_cwt_plan (host only, never touches the device; outputs: bit 0 W, 1 gws, 2 recon, 3 bandpow): out[5] = hop, frames per row,
 *      scales per workgroup (the whole set with recon or bandpow; else as few as bring the grid to about four workgroups per CU),
 *      workgroups launched, scratch bytes (the per-frame sums behind gws).  The CU count is the device's once the library is
 *      initialised and 256 before.  < 0 for a shape sp_cwt refuses, or out NULL.
 *      sp_icwt: out[b][n] = sum_s w[s] W[b][s][n], ascending s (w: HOST float32 [nscales]; W, out follow `mem`): the sum behind the
 *      reconstruction (T&C eq. 11) from a materialised W.  Refused: nscales < 1, nsig < 1, batch < 0 or > 65535, NULL pointers,
 *      weights that are not finite. */
#define SP_CWT_MORLET 0
#define SP_CWT_PAUL 1
int sp_cwt(const void *x, int dtype, int64_t nsig, int64_t x_ld, int64_t batch, const double *scales, int nscales, int family, double p0,
           double p1, int L, int M, const float *wrec, const float *wband, void *W, double *gws, void *recon, float *bandpow, int mem);
int sp_cwt_plan(int64_t nsig, int nscales, int64_t batch, int L, int M, int outputs, int64_t out[5]);
int sp_icwt(const void *W, int64_t nsig, int nscales, int64_t batch, const float *w, void *out, int mem);

/* ---- Batched Hermitian eigensolver (build-defined; the piece the reference's PCA.py takes from numpy.linalg.eigh): the
 *      eigendecomposition of `batch` matrices of order n, 1 <= n <= 64, e.g. the cross-spectral-density matrix of sp_csd_matrix at
 *      every bin (spectral POD).  a[batch][n][n] complex128 as (re, im) doubles, row-major.  Only the LOWER triangle (row >= column)
 *      and the real part of the diagonal are read: numpy.linalg.eigh's UPLO = 'L'; the upper triangle may hold anything.
 *        w[batch][n]         float64 eigenvalues, DESCENDING (ties in the order of the solver's internal index)
 *        v[batch][n][nvec]   complex128, column j the unit eigenvector of w[j]; only the nvec leading ones, 0 <= nvec <= n.  Each is
 *                            turned so that its component of largest modulus (the first on ties) is real and positive, so a real
 *                            symmetric matrix gives vectors real to rounding.  nvec == 0: v may be NULL and no vectors are formed.
 *        sweeps[batch]       int32 Jacobi sweeps used, 0 for a matrix that is diagonal already.  A matrix that has not converged
 *                            after max_sweeps sweeps (30 is ample: 8 for random CSD matrices of order 64, 17 at most on clustered
 *                            spectra), or that holds a NaN or an infinity where it is read, reports max_sweeps + 1; its w and v are
 *                            unspecified, the other matrices of the batch are unaffected, and the call still returns 0.
 *      Parallel cyclic Jacobi in float64, one matrix per workgroup, held in LDS at the order padded to 8, 16, 32 or 64; stops when
 *      sqrt(sum_{i<j} |a_ij|^2) <= n eps ||A||_F.  Each matrix is scaled by an exact power of two first, so entries of 1e+-150 are
 *      safe.  No atomics: two calls agree bitwise.  a, w, v, sweeps follow `mem`.
 *      Refused (< 0, sp_last_error() names sp_eigh, the device is not touched): n < 1 or n > 64; nvec outside 0 .. n; batch < 0;
 *      max_sweeps < 1; a, w or sweeps NULL, or v NULL with nvec > 0.  batch == 0 returns 0 and touches nothing.
 *      A deliberate deviation from "a rotation is skipped when a_pq == 0 exactly": a pair is skipped unless |a_pq| >= 2^-1000 of the
 *      scaled matrix (largest component in [1, 2)).  That covers the exact zeros of the padding, keeps a NaN from rotating anything,
 *      and keeps the phase a_pq / |a_pq| away from subnormal operands; an entry below 2^-1000 is left where it is, 700 orders of
 *      magnitude under the stopping threshold.
 *      sp_eigh_plan (host only, never touches the device): out[4] = padded order NP, LDS bytes of a workgroup, workgroups per CU
 *      (what the LDS, the threads and the registers of a CU allow), workgroups launched = min(batch, workgroups per CU x CUs).
 *      The CU count is that of the device once the library is initialised (sp_init or any call that runs on the device) and 256, an
 *      MI355X, before: out[3] may differ between the two on another part.  < 0 for an n, nvec or batch that sp_eigh refuses, or
 *      out NULL. */
int sp_eigh(const double *a, int n, int64_t batch, int nvec, int max_sweeps, double *w, double *v, int32_t *sweeps, int mem);
int sp_eigh_plan(int n, int nvec, int64_t batch, int64_t out[4]);

/* ---- F1 (build-defined; nearest reference code filters.py:282, ccf.py:283): causal FIR
 *      y = lfilter(h, 1, x)[0:n] by overlap-save with nfft-point blocks (nfft power of two > ntaps;
 *      0 = choose). */
int sp_fftfilt(const float *h, int ntaps, const float *x, int64_t n, int nfft, float *y, int mem);

/* ---- A6 / N1: the fft_pwelch epilogue on device-resident averaged spectra (fft_analysis.py:489-648, Cxy_Cxy2 :1662-1688):
 *      complex coherence, mean-squared coherence, cross-phase, linear amplitude spectra (:526-540), and the correlations
 *      Rxx, Ryy, Rxy, iCxy = sqrt(nfft) ifft(spectrum) (one-sided input: [1:-1] halved, irfft semantics; two-sided:
 *      ifftshift first), fftshifted (:544-597), corrcoef = Rxy / sqrt(Ex Ey).  Inputs as sp_welch_csd leaves them:
 *      pxx[nb], pyy[nch][nb], pxy[nch][nb][2] float64.  `out` holds sp_csd_epilogue_doubles(nch, nb, nfft) float64:
 *        cxy[nch][nb][2] | cxy2[nch][nb] | phi[nch][nb] | lxx[nb] | lyy[nch][nb] | lxy[nch][nb] |
 *        rxx[nfft][2] | ryy[nch][nfft][2] | rxy[nch][nfft][2] | icxy[nch][nfft][2] | corrcoef[nch][nfft][2] | e[1+nch][2]
 *      (e = the zero-lag values Ex, Ey_c; imaginary parts are zero for one-sided input). */
int64_t sp_csd_epilogue_doubles(int nch, int nb, int nfft);
int sp_csd_epilogue(const double *pxx, const double *pyy, const double *pxy, int nch, int nb, int nfft, int onesided, double enbw,
                    double *out, int mem);

/* ---- F2 (build-defined): application of the second-order sections the reference only designs (notch_filter.py:19-241
 *      iirnotch / iirpeak return (b, a) and nothing in the reference applies them; its scipy application sites for
 *      other filters are filters.py:328 lfilter and :347 filtfilt).  y = scipy.signal.lfilter(b, a, x) for one biquad,
 *      b[3], a[3] float64 HOST arrays (a[0] != 0), x and y float32 [n] (follow `mem`).  The recurrence is evaluated
 *      exactly (float64 state, blocked scan of the affine state maps), not as a truncated FIR. */
int sp_biquad(const double *b, const double *a, const float *x, int64_t n, float *y, int mem);

/* ---- F3: cascades of second-order sections (scipy.signal.sosfilt / sosfiltfilt; the reference's application sites
 *      filters.py:328 lfilter, :347 and :355-356 filtfilt).  sos[nsec][6] float64 HOST array (b0 b1 b2 a0 a1 a2 per
 *      section, a0 != 0, 1 <= nsec <= 8, every pole radius <= 1), applied along each of nrows float32 rows of n samples
 *      (x, y [nrows][n]).  The recurrence is evaluated exactly (float64 state, blocked scan of the affine state maps).
 *      sp_sosfilt: zi / zf [nrows][nsec][2] float64 in sosfilt's convention, or NULL (rest / not wanted).
 *      sp_sosfiltfilt: zero-phase, forward then backward from the steady state (sosfilt_zi) times the first sample of each
 *      pass, over the record extended by padlen samples (padtype 0 none, 1 odd, 2 even, 3 constant; n > padlen).
 *      x, y, zi, zf follow `mem`. */
int sp_sosfilt(const double *sos, int nsec, const float *x, int64_t nrows, int64_t n, const double *zi, float *y, double *zf,
               int mem);
int sp_sosfiltfilt(const double *sos, int nsec, const float *x, int64_t nrows, int64_t n, int padtype, int64_t padlen, float *y,
                   int mem);

/* ---- helper: mean of a float32 / complex64 vector in double (fft_analysis.py:2148 detrend) */
int sp_mean(const void *x, int x_dtype, int64_t n, double out[2], int mem);

#ifdef __cplusplus
}
#endif
#endif
