// k_fft.hip -- batched C2C, Hilbert, FIR, cross-covariance launchers
#include "launch.h"
namespace sp {

// complex transpose with out = scale * (conj ? conj(in) : in): first / last pass of the large FFT
// blockIdx.z: matrix of a batch (contiguous rows*cols apart)
static __global__ void k_transpose_c(const cf *__restrict__ in, cf *__restrict__ out, int64_t rows, int64_t cols,
                                     int conj, float scale) {
    __shared__ cf tile[32][33];
    in += (int64_t)blockIdx.z * rows * cols;
    out += (int64_t)blockIdx.z * rows * cols;
    const int64_t c0 = (int64_t)blockIdx.x * 32, r0 = (int64_t)blockIdx.y * 32;
    const float sg = conj ? -scale : scale;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int64_t r = r0 + j, c = c0 + threadIdx.x;
        if (r < rows && c < cols) {
            const cf a = in[r * cols + c];
            tile[j][threadIdx.x] = mk(scale * a.x, sg * a.y);
        }
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int64_t c = c0 + j, r = r0 + threadIdx.x;
        if (r < rows && c < cols) out[c * rows + r] = tile[threadIdx.x][j];
    }
}

// out[i] = i < n_in ? (x[i] - mean, 0) : 0   for i < L   (real -> zero-padded complex)
static __global__ void k_pack_real(const float *__restrict__ x, int64_t n_in, const double *__restrict__ mean, int64_t L,
                                   cf *__restrict__ out) {
    const float m = mean ? (float)mean[0] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = i < n_in ? mk(x[i] - m, 0.f) : mk(0.f, 0.f);
}

// out[i] = a[i] * b[i] (optionally conj(a*b)), i < n
// blockIdx.y: row of a batch (a and out n apart, b shared)
static __global__ void k_cmul_vec(const cf *__restrict__ a, const cf *__restrict__ b, int64_t n, int conj_out,
                                  cf *__restrict__ out) {
    a += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf p = cmul(a[i], b[i]);
        out[i] = conj_out ? cconj(p) : p;
    }
}

// Bluestein pre-multiply with zero padding: out[i] = i < n ? in[i]*chirp[i] : 0, i < L  (conj_in: use conj(in))
// blockIdx.y: row of a batch (in n apart, out L apart)
static __global__ void k_blue_pre(const cf *__restrict__ in, const cf *__restrict__ chirp, int64_t n, int64_t L,
                                  int conj_in, cf *__restrict__ out) {
    in += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * L;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n) {
            const cf a = in[i];
            out[i] = cmul(conj_in ? cconj(a) : a, chirp[i]);
        } else {
            out[i] = mk(0.f, 0.f);
        }
    }
}

// Bluestein post-multiply: out[i] = scale * conj?(in[i] * chirp[i]),  i < n
// blockIdx.y: row of a batch (in in_ld apart, out n apart)
static __global__ void k_blue_post(const cf *__restrict__ in, const cf *__restrict__ chirp, int64_t n, int conj_out,
                                   float scale, cf *__restrict__ out, int64_t in_ld) {
    in += (int64_t)blockIdx.y * in_ld;
    out += (int64_t)blockIdx.y * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cf p = cmul(in[i], chirp[i]);
        out[i] = mk(scale * p.x, conj_out ? -scale * p.y : scale * p.y);
    }
}

// analytic-signal mask (hilbert.py:63-64) in place: k=0 and k=nyq x1, 1..nyq-1 x2, > nyq x0
static __global__ void k_hilbert_mask(cf *__restrict__ X, int64_t n) {
    const int64_t nyq = (n & 1) ? (n + 1) / 2 : n / 2;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const float h = (k == 0 || k == nyq) ? 1.f : (k < nyq ? 2.f : 0.f);
        X[k] = h * X[k];
    }
}

// c[ch][n] = sum_g detrended(x[ch][g*hop + n]), n < nfft: the time-domain sum of all frames of each channel.  By linearity
// sum_g FFT(win * frame_g) = FFT(win * c): the mean spectrum of the nT-model branch of fft_pwelch (fft_analysis.py:346-393)
// without writing one spectrum.  grid (ceil(nfft/256), frame slices, channels); every slice writes its own partial
// part[slice][ch][n][2] (float64), k_frame_sum_reduce adds the slices in a fixed order: deterministic (round 1 used
// float64 atomics).
template <bool LIN>
static __global__ void k_frame_sum(const void *__restrict__ x, int cplx, int64_t x_ld, int nfft, int hop, int64_t nframes,
                                   const float *__restrict__ trend, double *__restrict__ part) {
    const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int ch = blockIdx.z;
    const int64_t per = (nframes + gridDim.y - 1) / gridDim.y;
    const int64_t g0 = (int64_t)blockIdx.y * per, g1 = g0 + per < nframes ? g0 + per : nframes;
    if (n >= nfft) return;
    const Trend tr = load_trend(trend + 4 * ch);
    const int64_t off = (int64_t)ch * x_ld;
    double sr = 0.0, si = 0.0;
    for (int64_t g = g0; g < g1; ++g) {
        const int64_t i = g * hop + n;
        const cf v = detrended<LIN>(load_sample(x, off + i, cplx != 0), tr, i);
        sr += (double)v.x;
        si += (double)v.y;
    }
    double *p = part + 2 * (((int64_t)blockIdx.y * gridDim.z + ch) * nfft + n);
    p[0] = sr;
    p[1] = si;
}

static __global__ void k_frame_sum_reduce(const double *__restrict__ part, int slices, int64_t count /* nch*nfft*2 */,
                                          double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int q = 0; q < slices; ++q) s += part[(int64_t)q * count + e];
    out[e] = s;
}

// X[k] *= H[k] in place (long-row form of sp_spectral_filter)
static __global__ void k_spec_mul(cf *__restrict__ X, const cf *__restrict__ H, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        X[k] = cmul(X[k], H[k]);
}

// z = (x1-m1) + i (x2-m2), zero-padded to L;  mom[0]=m1, mom[1]=m2
static __global__ void k_xc_pack(const float *__restrict__ x1, const float *__restrict__ x2, int64_t n, int64_t L,
                                 const double *__restrict__ mom, cf *__restrict__ z) {
    const float m1 = (float)mom[0], m2 = (float)mom[1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (int64_t)gridDim.x * blockDim.x)
        z[i] = i < n ? mk(x1[i] - m1, x2[i] - m2) : mk(0.f, 0.f);
}

// R[k] = A conj(B) from Z = FFT(a + i b):  Im(Z[k] Z[L-k])/2 + i (|Z[k]|^2 - |Z[L-k]|^2)/4 ; stored CONJUGATED
static __global__ void k_xc_mid(const cf *__restrict__ Z, int64_t L, cf *__restrict__ R) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += (int64_t)gridDim.x * blockDim.x) {
        const cf z = Z[k], zm = Z[(L - k) & (L - 1)];
        const cf zz = cmul(z, zm);
        R[k] = mk(0.5f * zz.y, -0.25f * (cnorm(z) - cnorm(zm)));
    }
}

// ccf with a half-length inverse (the correlation is real): from Z = FFT_L(a + i b), R(k) = A conj(B) as in k_xc_mid, and
// Z'[k] = ((R(k) + conj R(M-k)) + i conj(w) (R(k) - conj R(M-k)))/2, M = L/2, w = exp(-2 pi i k / L): the M-point spectrum of
// z'[n] = r[2n] + i r[2n+1].  Stored CONJUGATED (the inverse runs as a forward transform of the conjugate).
static __global__ void k_xc_mid_half(const cf *__restrict__ Z, int64_t L, BigTw bt, cf *__restrict__ Zp) {
    const int64_t M = L / 2;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < M; k += (int64_t)gridDim.x * blockDim.x) {
        const cf a = Z[k], am = Z[(L - k) & (L - 1)], b = Z[M - k], bm = Z[M + k];
        const cf za = cmul(a, am), zb = cmul(b, bm);
        const cf rk = mk(0.5f * za.y, 0.25f * (cnorm(a) - cnorm(am)));
        const cf rmc = mk(0.5f * zb.y, -0.25f * (cnorm(b) - cnorm(bm)));              // conj R(M-k)
        const cf w = cmul(bt.hi[k >> bt.lb], bt.lo[k & ((1 << bt.lb) - 1)]);          // W_L^k
        const cf s = rk + rmc, d = rk - rmc;
        const cf t = cmul(cconj(w), d);                                               // i t = (-t.y, t.x)
        Zp[k] = mk(0.5f * (s.x - t.y), -0.5f * (s.y + t.x));
    }
}

// half-length Hilbert, middle step, in place: Z = FFT_M(x[2n] + i x[2n+1]) (M = N/2) -> Z'[k] = (conj(w)(Z[k] + conj Z[M-k]) -
// w (Z[k] - conj Z[M-k]))/2, w = exp(-2 pi i k / N), Z'[0] = 0: the half-length spectrum of y = Im(analytic signal), i.e. the
// real-FFT split, the analytic mask (hilbert.py:63-64: DC and Nyquist contribute to the real part only) and the inverse
// real-FFT merge in one step.  A thread owns the pair (k, M-k).
static __global__ void k_hilbert_mid(cf *__restrict__ Z, int64_t M, BigTw bt) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= M / 2; k += (int64_t)gridDim.x * blockDim.x) {
        if (k == 0) {
            Z[0] = mk(0.f, 0.f);
            continue;
        }
        const int64_t km = M - k;
        const cf a = Z[k], b = Z[km];
        const cf w = cmul(bt.hi[k >> bt.lb], bt.lo[k & ((1 << bt.lb) - 1)]);          // W_N^k
        const cf p = mk(a.x + b.x, a.y - b.y), q = mk(a.x - b.x, a.y + b.y);          // a + conj b, a - conj b
        const cf r = cmul(cconj(w), p) - cmul(w, q);
        Z[k] = mk(0.5f * r.x, 0.5f * r.y);
        if (km != k) {
            // for M-k: w' = -conj(w), p' = conj p, q' = -conj q  ->  conj(w') p' - w' q' = -w conj(p) - conj(w) conj(q)
            const cf r2 = cmul(w, cconj(p)) + cmul(cconj(w), cconj(q));
            Z[km] = mk(-0.5f * r2.x, -0.5f * r2.y);
        }
    }
}

// co[j], j < 2n-1, 'full' order from r = real(FFT(conj R))/L:  lag >= 0 -> r[lag], lag < 0 -> r[L+lag]; times mom[2]
static __global__ void k_xc_out(const cf *__restrict__ r, int64_t n, int64_t L, const double *__restrict__ mom,
                                float *__restrict__ co) {
    const float nrm = (float)(mom[2] / (double)L);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < 2 * n - 1; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lag = j - (n - 1);
        co[j] = nrm * r[lag >= 0 ? lag : L + lag].x;
    }
}

// one block of 256.  out_d[0..1] = mean, out_d[2] = sum|x|^2, out_d[3..4] = sum i*x.
// trend_f[4] (optional): mode 1 -> (mean, 0 slope); mode 2 -> least-squares line m + s*i
// blockIdx.x = signal number (partials / outputs strided accordingly)
static __global__ __launch_bounds__(256) void k_moments_finish(const double *__restrict__ partial, int nblocks, int64_t n,
                                                         int mode, double *__restrict__ out_d,
                                                         float *__restrict__ trend_f) {
    __shared__ double sh[SP_MOM][256];
    partial += (int64_t)blockIdx.x * nblocks * 8;
    if (out_d) out_d += (int64_t)blockIdx.x * 8;
    if (trend_f) trend_f += (int64_t)blockIdx.x * 4;
    double s[SP_MOM] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
        for (int j = 0; j < SP_MOM; ++j) s[j] += partial[b * 8 + j];
    }
#pragma unroll
    for (int j = 0; j < SP_MOM; ++j) sh[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int j = 0; j < SP_MOM; ++j) sh[j][threadIdx.x] += sh[j][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double N = (double)n;
        const double mr = sh[0][0] / N, mi = sh[1][0] / N;
        if (out_d) {
            out_d[0] = mr;
            out_d[1] = mi;
            out_d[2] = sh[2][0];
            out_d[3] = sh[3][0];
            out_d[4] = sh[4][0];
        }
        if (trend_f) {
            if (mode == 2 && n > 1) {
                // least squares on i = 0..n-1:  slope = (sum i x - ibar sum x) / sum (i-ibar)^2
                const double ibar = 0.5 * (N - 1.0);
                const double sxx = N * (N * N - 1.0) / 12.0;
                const double sr = (sh[3][0] - ibar * sh[0][0]) / sxx, si = (sh[4][0] - ibar * sh[1][0]) / sxx;
                trend_f[0] = (float)(mr - sr * ibar);
                trend_f[1] = (float)(mi - si * ibar);
                trend_f[2] = (float)sr;
                trend_f[3] = (float)si;
            } else {
                trend_f[0] = (float)mr;
                trend_f[1] = (float)mi;
                trend_f[2] = 0.f;
                trend_f[3] = 0.f;
            }
        }
    }
}

// ccf (ccf.py:74-76): both signals' moment records finished by ONE block and the normalisation record [mean1, mean2, 1 / (n std1
// std2), 0] written behind them -- k_moments_finish x2 + k_xcorr_norm in one launch (two kernel boundaries less per call)
static __global__ __launch_bounds__(256) void k_moments_finish_xc(const double *__restrict__ partial, int nblocks, int64_t n,
                                                            double *__restrict__ out_d, double *__restrict__ xc_out) {
    __shared__ double sh[3][256];
    double mean[2], ssq[2];
    for (int sig = 0; sig < 2; ++sig) {
        const double *pp = partial + (int64_t)sig * nblocks * 8;
        double s0 = 0, s2 = 0;
        for (int b = threadIdx.x; b < nblocks; b += 256) {
            s0 += pp[b * 8 + 0];
            s2 += pp[b * 8 + 2];
        }
        sh[0][threadIdx.x] = s0;
        sh[2][threadIdx.x] = s2;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
                sh[2][threadIdx.x] += sh[2][threadIdx.x + o];
            }
            __syncthreads();
        }
        mean[sig] = sh[0][0] / (double)n;
        ssq[sig] = sh[2][0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int sig = 0; sig < 2; ++sig) {
            out_d[sig * 8 + 0] = mean[sig];
            out_d[sig * 8 + 1] = 0.0;
            out_d[sig * 8 + 2] = ssq[sig];
            out_d[sig * 8 + 3] = 0.0;
            out_d[sig * 8 + 4] = 0.0;
        }
        const double v1 = ssq[0] / (double)n - mean[0] * mean[0], v2 = ssq[1] / (double)n - mean[1] * mean[1];
        xc_out[0] = mean[0];
        xc_out[1] = mean[1];
        xc_out[2] = 1.0 / ((double)n * sqrt(v1 > 0 ? v1 : 0) * sqrt(v2 > 0 ? v2 : 0));
        xc_out[3] = 0;
    }
}

int launch_fft_c2c(LaunchCtx c, const cf *in, cf *out, int64_t batch, int inverse, const Xf &xf, BigTw bt) {
    const int blocks = strided_blocks(xf.L, batch, c.ncu, xf.L == 4096 && !xf.blue ? 12 : 4);
#define M_(XT)                                                                                        \
    hipLaunchKernelGGL((k_fft_c2c<XT>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, batch, \
                       inverse, xf.tb, bt);
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

// three-pass long transform pieces (power-of-two lengths; ncols is a multiple of the columns per workgroup)
int launch_fft_cols(LaunchCtx c, const cf *in, cf *out, int64_t ncols, int64_t nouter, int64_t es, int64_t os, int64_t twmul,
                    int conj_in, const Xf &xf, BigTw bt, int64_t hmask_n, ColsIn ci, int tw_outer) {
    if (xf.blue) return -1;
    const int fpw = fpw_of(xf.L);
    if (ncols % fpw || nouter < 1) return -1;
    const int64_t ncb = ncols / fpw, total = ncb * nouter;
    // (a multiple of the 2 or 3 workgroups a CU holds, so that the last round is a full one)
    const int64_t cap = (int64_t)c.ncu * 6;       // several blocks per workgroup amortise its twiddle set-up
    const unsigned grid = (unsigned)(total < cap ? total : cap);
    // real samples in (kind 1 / 4: 64-byte pieces per row and array): pair neighbouring column blocks on one XCD
    if ((ci.kind == 1 || ci.kind == 4) && total % 16 == 0 && grid % 16 == 0) tw_outer |= 2;
    // kind 1 whose samples end exactly at the middle row: the predicate-free form
    const bool half_exact = ci.kind == 1 && ci.r2 && ci.mom && nouter == 1 && xf.L >= 32 && ci.nreal == (int64_t)(xf.L / 2) * es &&
                            !env_flag("SP_COLS_NOHALF");
#define M_(XT)                                                                                        \
    if (half_exact) hipLaunchKernelGGL((k_fft_cols<XT::L, 4>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, \
                                       ncb, nouter, es, os, twmul, conj_in, xf.tb, bt, hmask_n, ci, tw_outer);       \
    else if (ci.kind == 1) hipLaunchKernelGGL((k_fft_cols<XT::L, 1>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, \
                                         ncb, nouter, es, os, twmul, conj_in, xf.tb, bt, hmask_n, ci, tw_outer);       \
    else if (ci.kind == 3) hipLaunchKernelGGL((k_fft_cols<XT::L, 3>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, \
                                              out, ncb, nouter, es, os, twmul, conj_in, xf.tb, bt, hmask_n, ci, tw_outer); \
    else if (hmask_n > 0) hipLaunchKernelGGL((k_fft_cols<XT::L, 0, true>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                                             in, out, ncb, nouter, es, os, twmul, conj_in, xf.tb, bt, hmask_n, ci, tw_outer); \
    else hipLaunchKernelGGL((k_fft_cols<XT::L, 0>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, ncb, nouter, \
                            es, os, twmul, conj_in, xf.tb, bt, hmask_n, ci, tw_outer);
    SP_DISPATCH_P(xf, M_)
#undef M_
    return 0;
}

int launch_fft_rows_rev(LaunchCtx c, const cf *in, cf *out, int64_t A, int64_t B, int conj_out, float scale, const Xf &xf,
                        RowsOut ro) {
    if (xf.blue) return -1;
    const int fpw = fpw_of(xf.L);
    if (A % fpw) return -1;
    const int64_t total = A * B / fpw, cap = (int64_t)c.ncu * 4;
    const unsigned grid = (unsigned)(total < cap ? total : cap);
#define M_(XT)                                                                                        \
    if (ro.co != nullptr && ro.kind == 2)                                                             \
        hipLaunchKernelGGL((k_fft_rows_rev<XT::L, 2>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, A, B, \
                           conj_out, scale, xf.tb, ro);                                               \
    else if (ro.co != nullptr && ro.kind == 3)                                                        \
        hipLaunchKernelGGL((k_fft_rows_rev<XT::L, 3>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, A, B, \
                           conj_out, scale, xf.tb, ro);                                               \
    else if (ro.co != nullptr)                                                                        \
        hipLaunchKernelGGL((k_fft_rows_rev<XT::L, 1>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, A, B, \
                           conj_out, scale, xf.tb, ro);                                               \
    else hipLaunchKernelGGL((k_fft_rows_rev<XT::L, 0>), dim3(grid), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, in, out, A, B, \
                            conj_out, scale, xf.tb, ro);
    SP_DISPATCH_P(xf, M_)
#undef M_
    return 0;
}

int launch_hilbert_rowsmid(LaunchCtx c, cf *Tm, int64_t A, int64_t B, const Xf &xc, BigTw btN, const cf *tw2c) {
    if (xc.blue || A < 2 || B < 2) return -1;
    const int64_t nslots = A * B / 2;
#define RM_(LL)                                                                                        \
    case LL: {                                                                                        \
        constexpr int HP = WgCfg<LL>::FPW / 2;                                                        \
        const int64_t iters = (nslots + HP - 1) / HP, cap = (int64_t)c.ncu * 4;                       \
        hipLaunchKernelGGL((k_hilbert_rowsmid<LL>), dim3((unsigned)(iters < cap ? iters : cap)), dim3(WgCfg<LL>::WG),   \
                           WgCfg<LL>::lds_bytes(1), c.stream, Tm, A, B, xc.tb, btN, tw2c);            \
        return 0;                                                                                     \
    }
    switch (xc.L) {
        RM_(32) RM_(64) RM_(128) RM_(256) RM_(512) RM_(1024) RM_(2048)
        default: return -1;
    }
#undef RM_
}

int launch_xc_rowsmid(LaunchCtx c, cf *Tm, int64_t A, int64_t B, const Xf &xc, const Xf &xc2, BigTw btL, BigTw btM) {
    if (xc.blue || xc2.blue || xc2.L * 2 != xc.L || A < 2 || B < 2) return -1;
    const int64_t nslots = A * B / 2;
#define XR_(LL)                                                                                        \
    case LL: {                                                                                        \
        constexpr int HP = WgCfg<LL>::FPW / 2;                                                        \
        const int64_t iters = (nslots + HP - 1) / HP, cap = (int64_t)c.ncu * 4;                       \
        const size_t lds = sizeof(cf) * (size_t)WgCfg<LL>::FPW * (LL + 32);                          \
        hipLaunchKernelGGL((k_xc_rowsmid<LL>), dim3((unsigned)(iters < cap ? iters : cap)), dim3(WgCfg<LL>::WG), lds, c.stream, Tm, A, B, \
                           xc.tb, xc2.tb, btL, btM);                                                  \
        return 0;                                                                                     \
    }
    switch (xc.L) {
        XR_(64) XR_(128) XR_(256) XR_(512) XR_(1024) XR_(2048)
        default: return -1;
    }
#undef XR_
}

int launch_fft_cols_lag(LaunchCtx c, const cf *in, int64_t ncols, int64_t nouter, int64_t es, int64_t os, const Xf &xf, RowsOut ro) {
    if (xf.blue) return -1;
    const int fpw = fpw_of(xf.L);
    if (ncols % fpw || nouter < 1) return -1;
    const int64_t ncb = ncols / fpw, total = ncb * nouter, cap = (int64_t)c.ncu * 6;
    const unsigned grid = (unsigned)(total < cap ? total : cap);
    if (total % 16 == 0 && grid % 16 == 0) ro.kind |= 16;
#define CL_(LL)                                                                                        \
    case LL:                                                                                          \
        hipLaunchKernelGGL((k_fft_cols_lag<LL>), dim3(grid), dim3(WgCfg<LL>::WG), WgCfg<LL>::lds_bytes(1), c.stream, in, ncb, nouter, es, os, \
                           xf.tb, ro);                                                                \
        return 0;
    switch (xf.L) {
        CL_(64) CL_(128) CL_(256)
        default: return -1;
    }
#undef CL_
}

int launch_fft_cols_inv(LaunchCtx c, const cf *in, cf *out, int64_t ncols, int64_t nouter, int64_t es, int64_t os, int64_t twmul,
                        const Xf &xf, BigTw bt, float scale, const RowsOut *analytic) {
    if (xf.blue) return -1;
    const int fpw = fpw_of(xf.L);
    if (ncols % fpw || nouter < 1) return -1;
    const int64_t ncb = ncols / fpw, total = ncb * nouter, cap = (int64_t)c.ncu * 6;
    const unsigned grid = (unsigned)(total < cap ? total : cap);
    const RowsOut ro = analytic ? *analytic : RowsOut{nullptr, 0, 0, nullptr};
    // the whole row holds samples and pairs are 8-byte aligned: the predicate-free output form
    const bool full = analytic && ro.n == ro.Ltot && (((uintptr_t)ro.rx) & 7) == 0 && !env_flag("SP_COLS_NOHALF");
#define CI_(LL)                                                                                        \
    case LL:                                                                                          \
        if (analytic && full) hipLaunchKernelGGL((k_fft_cols_inv<LL, 3>), dim3(grid), dim3(WgCfg<LL>::WG), WgCfg<LL>::lds_bytes(1), c.stream, in, out, \
                                         ncb, nouter, es, os, twmul, xf.tb, bt, scale, ro);           \
        else if (analytic) hipLaunchKernelGGL((k_fft_cols_inv<LL, 2>), dim3(grid), dim3(WgCfg<LL>::WG), WgCfg<LL>::lds_bytes(1), c.stream, in, out, \
                                         ncb, nouter, es, os, twmul, xf.tb, bt, scale, ro);           \
        else hipLaunchKernelGGL((k_fft_cols_inv<LL, 0>), dim3(grid), dim3(WgCfg<LL>::WG), WgCfg<LL>::lds_bytes(1), c.stream, in, out, ncb, \
                                nouter, es, os, twmul, xf.tb, bt, scale, ro);                         \
        return 0;
    switch (xf.L) {
        CI_(64) CI_(128) CI_(256)
        default: return -1;
    }
#undef CI_
}

int launch_hilbert_mid(LaunchCtx c, cf *Z, int64_t M, BigTw bt) {
    const int64_t n = M / 2 + 1;
    const int64_t cap = (int64_t)c.ncu * 16;
    const int64_t b = (n + 255) / 256;
    hipLaunchKernelGGL(k_hilbert_mid, dim3((unsigned)(b < cap ? b : cap)), dim3(256), 0, c.stream, Z, M, bt);
    return 0;
}

int launch_hilbert(LaunchCtx c, const float *x, int64_t n_in, int64_t x_ld, int64_t batch, const Xf &xf, cf *out,
                   const cf *H) {
    const int blocks = strided_blocks(xf.L, batch, c.ncu, xf.L == 4096 && !xf.blue && !H ? 3 : 4);
#define M_(XT)                                                                                        \
    if (H) hipLaunchKernelGGL((k_hilbert<XT, true>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, n_in, \
                              x_ld, batch, xf.tb, out, H);                                            \
    else hipLaunchKernelGGL((k_hilbert<XT, false>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, n_in, \
                            x_ld, batch, xf.tb, out, H);
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

int launch_fftfilt(LaunchCtx c, const float *x, int64_t n, int ntaps, const cf *Hs, const Xf &xf, float *y) {
    const int64_t Lb = xf.L - (ntaps - 1);
    const int64_t npairs = ((n + Lb - 1) / Lb + 1) / 2;
    // interior pairs: both blocks and their outputs wholly inside [0, n): pair p reads [2pLb-(P-1), 2pLb+Lb+N-(P-1))
    int64_t pi0 = 1, pi1 = 0;
    if (npairs >= 3) {
        // largest p with 2 p Lb - (P-1) + Lb + N <= n
        pi1 = (n - xf.L - Lb + (ntaps - 1)) / (2 * Lb) + 1;
        if (pi1 > npairs) pi1 = npairs;
        if (pi1 < pi0) pi1 = pi0;
    } else {
        pi0 = pi1 = 0;
    }
#define M_(XT)                                                                                        \
    if (pi1 > pi0) {                                                                                  \
        const int blocks = strided_blocks(xf.L, pi1 - pi0, c.ncu, 6);      /* (three resident per CU) */ \
        hipLaunchKernelGGL((k_fftfilt<XT::L, false>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, n, \
                           ntaps, Hs, xf.tb, y, pi0, pi1);                                            \
    }                                                                                                 \
    if (pi0 > 0 || pi1 <= pi0) {                                                                      \
        const int64_t e1 = pi1 > pi0 ? pi0 : npairs;                                                  \
        hipLaunchKernelGGL((k_fftfilt<XT::L, true>), dim3(strided_blocks(xf.L, e1, c.ncu)), dim3(XT::C::WG),     \
                           XT::C::lds_bytes(1), c.stream, x, n, ntaps, Hs, xf.tb, y, (int64_t)0, e1);   \
    }                                                                                                 \
    if (pi1 > pi0 && pi1 < npairs) {                                                                  \
        hipLaunchKernelGGL((k_fftfilt<XT::L, true>), dim3(strided_blocks(xf.L, npairs - pi1, c.ncu)), dim3(XT::C::WG), \
                           XT::C::lds_bytes(1), c.stream, x, n, ntaps, Hs, xf.tb, y, pi1, npairs);      \
    }
    SP_DISPATCH_P(xf, M_)
#undef M_
    return 0;
}

int launch_xcorr(LaunchCtx c, const float *x1, const float *x2, int64_t n, const double *mom, const Xf &xf, float *co) {
#define M_(XT)                                                                                        \
    hipLaunchKernelGGL((k_xcorr<XT::L>), dim3(1), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x1, x2, n, mom, \
                       xf.tb, co);
    SP_DISPATCH_P(xf, M_)
#undef M_
    return 0;
}

int launch_moments(LaunchCtx c, const void *x, bool cplx, int64_t n, int mode, double *partial, double *out_d,
                   float *trend_f, int nsignals, int64_t x_cs) {
    int64_t nb = (n + 256 * 16 - 1) / (256 * 16);
    const int64_t cap = nsignals > 1 ? (4096 / nsignals < 8 ? 8 : 4096 / nsignals) : 4096;   // partial scratch: 4096 records
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    if ((int64_t)nsignals * nb > 4096) return -1;
    const bool lin = mode == 2;
    const dim3 grid((unsigned)nb, (unsigned)nsignals);
    if (cplx) {
        if (lin) hipLaunchKernelGGL((k_moments_partial<true, true>), grid, dim3(256), 0, c.stream, x, n, partial, x_cs);
        else hipLaunchKernelGGL((k_moments_partial<true, false>), grid, dim3(256), 0, c.stream, x, n, partial, x_cs);
    } else {
        if (lin) hipLaunchKernelGGL((k_moments_partial<false, true>), grid, dim3(256), 0, c.stream, x, n, partial, x_cs);
        else hipLaunchKernelGGL((k_moments_partial<false, false>), grid, dim3(256), 0, c.stream, x, n, partial, x_cs);
    }
    hipLaunchKernelGGL(k_moments_finish, dim3(nsignals), dim3(256), 0, c.stream, partial, (int)nb, n, mode, out_d, trend_f);
    return 0;
}

// ccf: means / sums of squares of two real signals (x_cs samples apart) and the normalisation record xc_out[4] in two launches
int launch_moments_xc(LaunchCtx c, const float *x, int64_t n, double *partial, double *out_d, double *xc_out, int64_t x_cs) {
    int64_t nb = (n + 256 * 16 - 1) / (256 * 16);
    if (nb > 2048) nb = 2048;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL((k_moments_partial<false, false>), dim3((unsigned)nb, 2), dim3(256), 0, c.stream, x, n, partial, x_cs);
    hipLaunchKernelGGL(k_moments_finish_xc, dim3(1), dim3(256), 0, c.stream, partial, (int)nb, n, out_d, xc_out);
    return 0;
}

int launch_transpose(LaunchCtx c, const void *in, void *out, int64_t rows, int64_t cols, int elem_bytes) {
    dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32));
    if (elem_bytes == 4)
        hipLaunchKernelGGL((k_transpose<float>), grid, dim3(32, 8), 0, c.stream, (const float *)in, (float *)out, rows, cols);
    else if (elem_bytes == 8)
        hipLaunchKernelGGL((k_transpose<cf>), grid, dim3(32, 8), 0, c.stream, (const cf *)in, (cf *)out, rows, cols);
    else
        return -1;
    return 0;
}

static int ew_blocks(int64_t n, int ncu) {
    int64_t b = (n + 255) / 256;
    const int64_t cap = (int64_t)ncu * 16;
    return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

int launch_transpose_c(LaunchCtx c, const cf *in, cf *out, int64_t rows, int64_t cols, int conj, float scale, int64_t batch) {
    if (batch < 1 || batch > 65535 || (rows + 31) / 32 > 65535) return -1;
    dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batch);
    hipLaunchKernelGGL(k_transpose_c, grid, dim3(32, 8), 0, c.stream, in, out, rows, cols, conj, scale);
    return 0;
}
int launch_pack_real(LaunchCtx c, const float *x, int64_t n_in, const double *mean, int64_t L, cf *out) {
    hipLaunchKernelGGL(k_pack_real, dim3(ew_blocks(L, c.ncu)), dim3(256), 0, c.stream, x, n_in, mean, L, out);
    return 0;
}
int launch_cmul_vec(LaunchCtx c, const cf *a, const cf *b, int64_t n, int conj_out, cf *out, int64_t batch) {
    if (batch < 1 || batch > 65535) return -1;
    hipLaunchKernelGGL(k_cmul_vec, dim3(ew_blocks(n, c.ncu), (unsigned)batch), dim3(256), 0, c.stream, a, b, n, conj_out, out);
    return 0;
}
int launch_blue_pre(LaunchCtx c, const cf *in, const cf *chirp, int64_t n, int64_t L, int conj_in, cf *out, int64_t batch) {
    if (batch < 1 || batch > 65535) return -1;
    hipLaunchKernelGGL(k_blue_pre, dim3(ew_blocks(L, c.ncu), (unsigned)batch), dim3(256), 0, c.stream, in, chirp, n, L, conj_in, out);
    return 0;
}
int launch_blue_post(LaunchCtx c, const cf *in, const cf *chirp, int64_t n, int conj_out, float scale, cf *out, int64_t batch,
                     int64_t in_ld) {
    if (batch < 1 || batch > 65535) return -1;
    hipLaunchKernelGGL(k_blue_post, dim3(ew_blocks(n, c.ncu), (unsigned)batch), dim3(256), 0, c.stream, in, chirp, n, conj_out, scale,
                       out, in_ld);
    return 0;
}
int launch_hilbert_mask(LaunchCtx c, cf *X, int64_t n) {
    hipLaunchKernelGGL(k_hilbert_mask, dim3(ew_blocks(n, c.ncu)), dim3(256), 0, c.stream, X, n);
    return 0;
}
int frame_sum_slices(int ncu, int nch, int nfft, int64_t nframes) {
    const int nb = (nfft + 255) / 256;
    int64_t slices = (8 * (int64_t)ncu + (int64_t)nb * nch - 1) / ((int64_t)nb * nch);
    if (slices > (nframes + 7) / 8) slices = (nframes + 7) / 8;
    if (slices < 1) slices = 1;
    if (slices > 65535) slices = 65535;
    return (int)slices;
}
// part: scratch of frame_sum_slices(...) * nch * nfft * 2 doubles
int launch_frame_sum(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int nch, int nfft, int hop, int64_t nframes,
                     const float *trend, bool lin, double *out, double *part) {
    // enough frame slices to fill the chip, each at least 8 frames long
    const int nb = (nfft + 255) / 256;
    const int slices = frame_sum_slices(c.ncu, nch, nfft, nframes);
    const dim3 grid(nb, (unsigned)slices, nch);
    if (lin) hipLaunchKernelGGL((k_frame_sum<true>), grid, dim3(256), 0, c.stream, x, cplx ? 1 : 0, x_ld, nfft, hop, nframes, trend, part);
    else hipLaunchKernelGGL((k_frame_sum<false>), grid, dim3(256), 0, c.stream, x, cplx ? 1 : 0, x_ld, nfft, hop, nframes, trend, part);
    const int64_t count = (int64_t)nch * nfft * 2;
    hipLaunchKernelGGL(k_frame_sum_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c.stream, (const double *)part, slices,
                       count, out);
    return 0;
}
int launch_spec_mul(LaunchCtx c, cf *X, const cf *H, int64_t n) {
    hipLaunchKernelGGL(k_spec_mul, dim3(ew_blocks(n, c.ncu)), dim3(256), 0, c.stream, X, H, n);
    return 0;
}
int launch_xc_pack(LaunchCtx c, const float *x1, const float *x2, int64_t n, int64_t L, const double *mom, cf *z) {
    hipLaunchKernelGGL(k_xc_pack, dim3(ew_blocks(L, c.ncu)), dim3(256), 0, c.stream, x1, x2, n, L, mom, z);
    return 0;
}
int launch_xc_mid_half(LaunchCtx c, const cf *Z, int64_t L, BigTw bt, cf *Zp) {
    const int64_t b = (L / 2 + 255) / 256, cap = (int64_t)c.ncu * 16;
    hipLaunchKernelGGL(k_xc_mid_half, dim3((unsigned)(b < cap ? b : cap)), dim3(256), 0, c.stream, Z, L, bt, Zp);
    return 0;
}
int launch_xc_mid(LaunchCtx c, const cf *Z, int64_t L, cf *R) {
    hipLaunchKernelGGL(k_xc_mid, dim3(ew_blocks(L, c.ncu)), dim3(256), 0, c.stream, Z, L, R);
    return 0;
}
int launch_xc_out(LaunchCtx c, const cf *r, int64_t n, int64_t L, const double *mom, float *co) {
    hipLaunchKernelGGL(k_xc_out, dim3(ew_blocks(2 * n - 1, c.ncu)), dim3(256), 0, c.stream, r, n, L, mom, co);
    return 0;
}

}   // namespace sp
