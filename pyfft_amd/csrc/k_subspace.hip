// k_subspace.hip -- the data covariance matrix of a segment, the covariance and modified-covariance least-squares fits, and the
// MUSIC / eigenvector pseudospectrum (include/spectral_sub.h; the host's arithmetic in sub_plan.h).  A segment is that of k_burg.hip
// (k_ar_scan and k_ar_mean look at it and form its mean), but here the detrended sample stays float64: products and sums are float64
// in a fixed order.  C[i,j] = (1 / N) sum_{t=m-1}^{n-1} conj(s[t-i]) s[t-j], N = n - m + 1.
// Kernels:
//   k_cov_row    one workgroup per (segment, tile), the tiles of k_ar_lags: AR_STAGE samples behind m - 1 samples of halo staged in LDS
//           (detrended, float64); a thread owns a column j of row 0 and a share of the stage; the shares are added in order and the
//           tile's m partial sums go to scratch.  The only O(n m) step.
//   k_cov_fill   one wave per segment: lane d adds the tiles' partial C[0,d] in order and walks diagonal d serially,
//           C[i+1,j+1] = C[i,j] + conj(s[m-2-i]) s[m-2-j] - conj(s[n-1-i]) s[n-1-j], from the 2 (m - 1) edge samples; the forward-backward
//           fold (C + J conj(C) J) / 2 mirrors a diagonal onto itself, so the lane that walked it folds it, divides by N and writes the
//           element and its conjugate mirror: exactly Hermitian, a real diagonal, every element written once.
//   k_ls_chol    one matrix per workgroup: the block C[1.., 1..] in LDS, right-looking Cholesky and two triangular solves in complex128.
//           A pivot at or below m 2^-52 C[j,j] stops the fit: status = j, a = (1, 0 ..), e = 0.
//   k_pseudo     one workgroup per (model, 256 bins), one lane per bin: the noise vectors staged in LDS SUB_PSEUDO_VECS at a time and read
//           wave-uniformly, the phase reduced in float64 as k_ar_psd does, one Horner pass per vector.
// Every output element is written once, by one thread, and nothing is cleared first.  No atomics.
#include "launch.h"
namespace sp {

template <bool C> struct SubT;
template <> struct SubT<false> {
    typedef float S;
    typedef double D;
};
template <> struct SubT<true> {
    typedef float2 S;
    typedef double2 D;
};

static __device__ __forceinline__ double sb_cj(double a) { return a; }
static __device__ __forceinline__ double2 sb_cj(double2 a) { return make_double2(a.x, -a.y); }
static __device__ __forceinline__ double sb_mul(double a, double b) { return a * b; }
static __device__ __forceinline__ double2 sb_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
static __device__ __forceinline__ double sb_add(double a, double b) { return a + b; }
static __device__ __forceinline__ double2 sb_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
static __device__ __forceinline__ double sb_sub(double a, double b) { return a - b; }
static __device__ __forceinline__ double2 sb_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
static __device__ __forceinline__ double sb_wide(float a) { return (double)a; }
static __device__ __forceinline__ double2 sb_wide(float2 a) { return make_double2((double)a.x, (double)a.y); }
static __device__ __forceinline__ double sb_re(double a) { return a; }
static __device__ __forceinline__ double sb_re(double2 a) { return a.x; }
static __device__ __forceinline__ double sb_im(double) { return 0.0; }
static __device__ __forceinline__ double sb_im(double2 a) { return a.y; }
static __device__ __forceinline__ void sb_set(double &d, double re, double) { d = re; }
static __device__ __forceinline__ void sb_set(double2 &d, double re, double im) { d = make_double2(re, im); }
static __device__ __forceinline__ double2 sb_over(double2 a, double s) { return make_double2(a.x / s, a.y / s); }

template <bool C> static __device__ __forceinline__ const typename SubT<C>::S *sub_segment(const ArArgs &A, int64_t sl) {
    const int64_t s = A.seg0 + sl, r = s / A.nframes, g = s - r * A.nframes;
    return (const typename SubT<C>::S *)A.x + r * A.x_ld + A.first + g * A.hop;
}

// ---- row 0 of the forward sum, by tiles -----------------------------------------------------------------------------------------------
template <bool C> static __global__ __launch_bounds__(256) void k_cov_row(CovArgs K, int64_t chunk, int64_t tiles, const double *mean, void *part_) {
    typedef typename SubT<C>::S S;
    typedef typename SubT<C>::D D;
    extern __shared__ __attribute__((aligned(16))) unsigned char sub_lds[];
    D *stage = (D *)sub_lds;                                             // [SUB_HALO + AR_STAGE]: sample sb + q at SUB_HALO + q
    D *share = stage + SUB_HALO + AR_STAGE;                              // [nsub][m]
    const int tid = threadIdx.x, m = K.m;
    const int64_t sl = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - sl * tiles, n = K.A.n;
    const S *x = sub_segment<C>(K.A, sl);
    D nmu;
    sb_set(nmu, -mean[2 * sl], -mean[2 * sl + 1]);
    const int64_t c0 = tile * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    const int nsub = 256 / m, items = nsub * m;                          // m <= 64: at least four shares, one item to a thread
    const int u = tid / m, j = tid - u * m;
    D acc;
    sb_set(acc, 0.0, 0.0);
    for (int64_t sb = c0; sb < c1; sb += AR_STAGE) {
        const int len = c1 - sb < AR_STAGE ? (int)(c1 - sb) : AR_STAGE;
        const int t0 = sb >= m - 1 ? 0 : (int)(m - 1 - sb);            // the sum starts at sample m - 1
        __syncthreads();
        for (int q = tid - (m - 1); q < len; q += 256) {
            const int64_t i = sb + q;
            D v;
            sb_set(v, 0.0, 0.0);
            if (i >= 0) v = sb_add(sb_wide(x[i]), nmu);
            stage[SUB_HALO + q] = v;
        }
        __syncthreads();
        if (tid < items && t0 < len) {
            const int run = (len - t0 + nsub - 1) / nsub, q0 = t0 + u * run, q1 = q0 + run < len ? q0 + run : len;
            for (int q = q0; q < q1; ++q) acc = sb_add(acc, sb_mul(sb_cj(stage[SUB_HALO + q]), stage[SUB_HALO + q - j]));
        }
    }
    __syncthreads();
    if (tid < items) share[tid] = acc;
    __syncthreads();
    if (tid < m) {
        D s = share[tid];
        for (int v = 1; v < nsub; ++v) s = sb_add(s, share[v * m + tid]);
        ((D *)part_)[(int64_t)blockIdx.x * m + tid] = s;
    }
}

// ---- the matrix from its first row and the edge samples ---------------------------------------------------------------------------------
template <bool C> static __global__ __launch_bounds__(64) void k_cov_fill(CovArgs K, int64_t tiles, const double *mean, const void *part_) {
    typedef typename SubT<C>::S S;
    typedef typename SubT<C>::D D;
    extern __shared__ __attribute__((aligned(16))) unsigned char sub_lds[];
    const int lane = threadIdx.x, m = K.m;
    D *tri = (D *)sub_lds;                                               // diagonal d: m - d entries from d m - d (d - 1) / 2 on
    D *edge = tri + m * (m + 1) / 2;                                     // s[0 .. m-2], then s[n-m+1 .. n-1]
    const int64_t sl = blockIdx.x, n = K.A.n;
    const S *x = sub_segment<C>(K.A, sl);
    D nmu;
    sb_set(nmu, -mean[2 * sl], -mean[2 * sl + 1]);
    for (int q = lane; q < 2 * (m - 1); q += 64) edge[q] = sb_add(sb_wide(x[q < m - 1 ? (int64_t)q : n - 2 * (m - 1) + q]), nmu);
    __syncthreads();
    if (lane >= m) return;
    const int d = lane, len = m - d;
    const D *part = (const D *)part_ + sl * tiles * m;
    D c = part[d];
    for (int64_t t = 1; t < tiles; ++t) c = sb_add(c, part[t * m + d]);
    if (d == 0) sb_set(c, sb_re(c), 0.0);
    D *dg = tri + d * m - d * (d - 1) / 2;
    dg[0] = c;
    for (int i = 0; i + 1 < len; ++i) {                                  // C[i+1, i+1+d] from C[i, i+d]
        const int j = i + d;
        const D head = sb_mul(sb_cj(edge[m - 2 - i]), edge[m - 2 - j]);
        const D tail = sb_mul(sb_cj(edge[2 * m - 3 - i]), edge[2 * m - 3 - j]);
        c = sb_sub(sb_add(c, head), tail);
        if (d == 0) sb_set(c, sb_re(c), 0.0);
        dg[i + 1] = c;
    }
    const double N = (double)(n - m + 1);
    double2 *out = (double2 *)K.C + sl * K.C_ld;
    for (int i = 0; i < len; ++i) {
        D v = dg[i];
        if (K.fb) {
            const D w = sb_add(v, dg[len - 1 - i]);                      // J conj(C) J mirrors the diagonal onto itself
            sb_set(v, 0.5 * sb_re(w), 0.5 * sb_im(w));
        }
        const double re = sb_re(v) / N, im = sb_im(v) / N;
        out[i * m + i + d] = make_double2(re, im);
        if (d) out[(i + d) * m + i] = make_double2(re, -im);
    }
}

// ---- the least-squares fit: sum_j C[i,j] a_j = -C[i,0], i, j = 1 .. p -------------------------------------------------------------------
template <bool CO> static __global__ __launch_bounds__(256) void k_ls_chol(const double2 *Cm, int64_t C_ld, int m, void *a_, double *e, int *status,
                                                                           int64_t out_ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sub_lds[];
    const int tid = threadIdx.x, p = m - 1;
    double2 *L = (double2 *)sub_lds;                                     // [p][p]: the lower triangle; a diagonal keeps its pivot d_j, unrooted
    double2 *b = L + p * p;                                              // [p]
    double *dg = (double *)(b + p);                                      // [p]: the diagonal as it came
    const double2 *Cs = Cm + (int64_t)blockIdx.x * C_ld;
    for (int q = tid; q < p * p; q += 256) {
        const int i = q / p, k = q - i * p;
        L[q] = Cs[(i + 1) * m + k + 1];
    }
    for (int q = tid; q < p; q += 256) {
        const double2 v = Cs[(q + 1) * m];
        b[q] = make_double2(-v.x, -v.y);
        dg[q] = Cs[(q + 1) * m + q + 1].x;
    }
    __syncthreads();
    int st = 0;
    for (int j = 0; j < p; ++j) {
        const double dj = L[j * p + j].x;                                // every thread reads the same pivot: the branch is uniform
        if (!(dj > (double)m * 0x1p-52 * dg[j])) {
            st = j + 1;
            break;
        }
        const double r = sqrt(dj);
        for (int i = j + 1 + tid; i < p; i += 256) L[i * p + j] = sb_over(L[i * p + j], r);
        __syncthreads();
        const int w = p - j - 1;
        for (int q = tid; q < w * w; q += 256) {
            const int i = j + 1 + q / w, k = j + 1 + q % w;
            if (k <= i) L[i * p + k] = sb_sub(L[i * p + k], sb_mul(L[i * p + j], sb_cj(L[k * p + j])));
        }
        __syncthreads();
    }
    const int64_t o = (int64_t)blockIdx.x * out_ld;
    if (st) {                                                            // never NaN: the model of no prediction, and where it stopped
        for (int j = tid; j <= p; j += 256) {
            if (CO) ((double2 *)a_)[o + j] = make_double2(j ? 0.0 : 1.0, 0.0);
            else ((double *)a_)[o + j] = j ? 0.0 : 1.0;
        }
        if (tid == 0) e[blockIdx.x] = 0.0, status[blockIdx.x] = st;
        return;
    }
    // L y = b; step j reads element j and writes the ones below it
    for (int j = 0; j < p; ++j) {
        const double2 yj = sb_over(b[j], sqrt(L[j * p + j].x));
        for (int i = j + 1 + tid; i < p; i += 256) b[i] = sb_sub(b[i], sb_mul(L[i * p + j], yj));
        __syncthreads();
    }
    for (int i = tid; i < p; i += 256) b[i] = sb_over(b[i], sqrt(L[i * p + i].x));
    __syncthreads();
    // L^H a = y; step j reads element j and writes the ones above it
    for (int j = p - 1; j >= 1; --j) {
        const double2 aj = sb_over(b[j], sqrt(L[j * p + j].x));
        for (int i = tid; i < j; i += 256) b[i] = sb_sub(b[i], sb_mul(sb_cj(L[j * p + i]), aj));
        __syncthreads();
    }
    for (int j = tid; j <= p; j += 256) {
        double2 v = make_double2(1.0, 0.0);
        if (j) v = sb_over(b[j - 1], sqrt(L[(j - 1) * p + j - 1].x));
        if (CO) ((double2 *)a_)[o + j] = v;
        else ((double *)a_)[o + j] = v.x;
    }
    if (tid == 0) {
        double acc = Cs[0].x;
        for (int j = 1; j <= p; ++j) {
            const double2 aj = sb_over(b[j - 1], sqrt(L[(j - 1) * p + j - 1].x)), c = Cs[j];
            acc += c.x * aj.x - c.y * aj.y;
        }
        e[blockIdx.x] = acc;
        status[blockIdx.x] = 0;
    }
}

// ---- the pseudospectrum ---------------------------------------------------------------------------------------------------------------
template <bool O64> static __global__ __launch_bounds__(256) void k_pseudo(const double2 *V_, int64_t V_ld, const double *w_, int m, int p, int ev, int64_t bpm,
                                                                           int64_t nbins, double start, double step, void *P_, int64_t P_ld, int *status) {
    __shared__ double2 vec[SUB_PSEUDO_VECS * SUB_MAX_M];                 // vector kk of the group at kk m
    __shared__ double gw[SUB_MAX_M];
    const int tid = threadIdx.x, nn = m - p;
    const int64_t model = (int64_t)blockIdx.x / bpm, blk = (int64_t)blockIdx.x - model * bpm, q = blk * 256 + tid;
    const double2 *V = V_ + model * m * V_ld;
    const double *w = w_ + model * m;
    for (int k = tid; k < nn; k += 256) {
        const double wk = w[p + k];
        gw[k] = ev ? (wk > 0.0 ? 1.0 / wk : 0.0) : 1.0;
    }
    if (blk == 0 && tid == 0) {
        int flag = 0;
        if (ev)
            for (int k = p; k < m; ++k) flag |= !(w[k] > 0.0);
        status[model] = flag;
    }
    const bool live = q < nbins;
    double sn = 0.0, cs = 1.0;
    if (live) {
        const double nu = __dadd_rn(start, __dmul_rn((double)q, step));   // two roundings, as the definition's: no fused multiply-add
        const double fr = nu - floor(nu);                               // the phase of a turn, reduced in float64
        sincospi(-2.0 * fr, &sn, &cs);
    }
    double den = 0.0;
    for (int k0 = 0; k0 < nn; k0 += SUB_PSEUDO_VECS) {
        const int kc = nn - k0 < SUB_PSEUDO_VECS ? nn - k0 : SUB_PSEUDO_VECS;
        __syncthreads();
        for (int idx = tid; idx < kc * m; idx += 256) {
            const int i = idx / kc, kk = idx - i * kc;
            vec[kk * m + i] = V[i * V_ld + p + k0 + kk];
        }
        __syncthreads();
        if (live)
            for (int kk = 0; kk < kc; ++kk) {
                const double2 *v = vec + kk * m;
                double2 acc = v[m - 1];
                for (int i = m - 2; i >= 0; --i) {
                    const double2 c = v[i];
                    acc = make_double2(acc.x * cs - acc.y * sn + c.x, acc.x * sn + acc.y * cs + c.y);
                }
                den += gw[k0 + kk] * (acc.x * acc.x + acc.y * acc.y);
            }
    }
    if (!live) return;
    const double out = den > 0.0 ? 1.0 / den : 0.0;                       // no noise vector with a weight: zeros, never NaN
    if (O64) ((double *)P_)[model * P_ld + q] = out;
    else ((float *)P_)[model * P_ld + q] = (float)out;
}

// ---- launch glue -------------------------------------------------------------------------------------------------------------------------
static bool cov_args_ok(const CovArgs &k) {
    const ArArgs &a = k.A;
    return a.x && a.n >= 2 && a.n <= YULE_MAX_N && k.m >= 2 && k.m <= SUB_MAX_M && k.m <= a.n && a.nseg >= 1 && a.nseg <= AR_PASS_SEGS && a.nframes >= 1 &&
           a.seg0 >= 0 && a.hop >= 1 && a.first >= 0 && a.detrend >= 0 && a.detrend <= 2 && k.C && k.C_ld >= (int64_t)k.m * k.m;
}

static bool cov_tiles_ok(const CovArgs &k, int64_t chunk, int64_t tiles) {
    return chunk >= AR_STAGE && chunk % AR_STAGE == 0 && tiles >= 1 && tiles <= AR_MAX_TILES && tiles * chunk >= k.A.n && (tiles - 1) * chunk < k.A.n &&
           k.A.nseg * tiles <= 0x7fffffff;
}

int launch_cov_row(LaunchCtx c, const CovArgs &k, int64_t chunk, int64_t tiles, const double *mean, void *part) {
    if (!cov_args_ok(k) || !cov_tiles_ok(k, chunk, tiles) || !mean || !part) return -1;
    const dim3 grid((unsigned)(k.A.nseg * tiles));
    const size_t lds = (size_t)sub_row_lds(k.A.cplx);
    static_assert((size_t)(SUB_HALO + AR_STAGE + 256) * 16 <= 64 * 1024, "k_cov_row stays within the LDS a launch gets unasked");
    if (k.A.cplx) hipLaunchKernelGGL(k_cov_row<true>, grid, dim3(256), lds, c.stream, k, chunk, tiles, mean, part);
    else hipLaunchKernelGGL(k_cov_row<false>, grid, dim3(256), lds, c.stream, k, chunk, tiles, mean, part);
    return 0;
}

int launch_cov_fill(LaunchCtx c, const CovArgs &k, int64_t tiles, const double *mean, const void *part) {
    if (!cov_args_ok(k) || tiles < 1 || tiles > AR_MAX_TILES || !mean || !part) return -1;
    const size_t lds = (size_t)(k.m * (k.m + 1) / 2 + 2 * (k.m - 1)) * (k.A.cplx ? 16 : 8);
    static_assert((size_t)(SUB_MAX_M * (SUB_MAX_M + 1) / 2 + 2 * (SUB_MAX_M - 1)) * 16 <= 64 * 1024, "k_cov_fill stays within the LDS a launch gets unasked");
    const dim3 grid((unsigned)k.A.nseg);
    if (k.A.cplx) hipLaunchKernelGGL(k_cov_fill<true>, grid, dim3(64), lds, c.stream, k, tiles, mean, part);
    else hipLaunchKernelGGL(k_cov_fill<false>, grid, dim3(64), lds, c.stream, k, tiles, mean, part);
    return 0;
}

int launch_ls_chol(LaunchCtx c, const void *C, int64_t C_ld, int m, int64_t nmodels, bool cplx, void *a, double *e, int *status, int64_t out_ld) {
    if (!C || !a || !e || !status || m < 2 || m > SUB_MAX_M || C_ld < (int64_t)m * m || nmodels < 1 || nmodels > 0x7fffffff || out_ld < m) return -1;
    const int p = m - 1;
    const size_t lds = (size_t)p * p * 16 + (size_t)p * 16 + (size_t)p * 8;
    static_assert((size_t)(SUB_MAX_M - 1) * (SUB_MAX_M - 1) * 16 + (SUB_MAX_M - 1) * 24 <= 64 * 1024, "k_ls_chol stays within the LDS a launch gets unasked");
    const dim3 grid((unsigned)nmodels);
    if (cplx) hipLaunchKernelGGL(k_ls_chol<true>, grid, dim3(256), lds, c.stream, (const double2 *)C, C_ld, m, a, e, status, out_ld);
    else hipLaunchKernelGGL(k_ls_chol<false>, grid, dim3(256), lds, c.stream, (const double2 *)C, C_ld, m, a, e, status, out_ld);
    return 0;
}

int launch_pseudo(LaunchCtx c, const void *V, int64_t V_ld, const double *w, int m, int p, int64_t nmodels, bool ev, int64_t nbins, double start, double step,
                  bool out64, void *P, int64_t P_ld, int *status) {
    if (!V || !w || !P || !status || m < 2 || m > SUB_MAX_M || p < 0 || p >= m || V_ld < m || nmodels < 1 || nbins < 1 || P_ld < nbins) return -1;
    const int64_t bpm = (nbins + 255) / 256;
    if (bpm > 0x7fffffff / nmodels) return -1;
    const dim3 grid((unsigned)(bpm * nmodels));
    if (out64) hipLaunchKernelGGL(k_pseudo<true>, grid, dim3(256), 0, c.stream, (const double2 *)V, V_ld, w, m, p, ev ? 1 : 0, bpm, nbins, start, step, P, P_ld, status);
    else hipLaunchKernelGGL(k_pseudo<false>, grid, dim3(256), 0, c.stream, (const double2 *)V, V_ld, w, m, p, ev ? 1 : 0, bpm, nbins, start, step, P, P_ld, status);
    return 0;
}

}   // namespace sp
