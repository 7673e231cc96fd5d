// k_burg.hip -- autoregressive (maximum-entropy) models and their spectra: Burg's recursion, Yule-Walker by biased lags and
// Levinson-Durbin, and the power spectrum of an all-pole model (include/spectral_ar.h; the host's arithmetic in ar_plan.h).
// A segment is n samples of a row, real or complex, less its own mean, a given constant or nothing.
// Kernels:
//   k_ar_scan    one workgroup per (segment, tile): the float64 sum of the tile's samples and a flag where one is not finite.
//   k_ar_mean    one wave per segment: the tiles' sums added in order over n (or the given constant, or zero).
//   k_burg<cplx, SPL, NW>   Burg's recursion with the forward and backward errors f, b in registers: the segment lies in the last n of
//           64 NW SPL slots, SPL consecutive slots to a lane.  b is held one sample late (b[slot of i] = b_{m-1}[i - 1]), so an order is
//           products and updates of a lane's own registers, then a shift by one slot: inside a lane by renaming, across lanes by a
//           neighbour-lane exchange.  Sample m - 1 leaves the sums at order m: its f is set to zero, which keeps its b zero from
//           then on.  Products are float32, every sum is float64 (per lane, then a butterfly over the wave whose result is the same
//           bits in every lane, then over the waves in their order).  k, a, E are float64 / complex128; the step-up of a runs beside
//           the recursion in two LDS buffers that alternate.
//           NW == 1, the wave form: BURG_WAVE_SEGS segments to a workgroup, one wave each, no workgroup barrier.
//           NW > 1, the workgroup form: before an order's one barrier every wave leaves its sums and its last lane's last f and b in
//           the order's set of slots (two sets alternate); after it every thread adds the sums in the waves' order and lane 0 of a
//           wave forms the b that crosses into it from the wave before, with the arithmetic that wave uses itself.
//   k_ar_lags    one workgroup per (segment, tile): AR_STAGE samples behind AR_MAX_ORDER samples of halo staged in LDS (detrended,
//           float32); a thread owns a lag and a share of the stage: float32 products, float64 sums; the shares are added in order and
//           the tile's p + 1 partial lags go to scratch in float64.
//   k_levinson   one wave per model: the tiles' partial lags added in order, over n; Levinson-Durbin in float64 with the sum over j
//           and the step-up spread over the lanes.
//   k_ar_psd     one lane per bin: the model's coefficients broadcast from LDS, the phase reduced in float64, Horner on the unit circle.
// Every output element is written once, by one thread, and nothing is cleared first.
#include "launch.h"
namespace sp {

template <bool C> struct ArT;
template <> struct ArT<false> {
    typedef float S;
    typedef double D;
};
template <> struct ArT<true> {
    typedef float2 S;
    typedef double2 D;
};

static __device__ __forceinline__ float ar_cj(float a) { return a; }
static __device__ __forceinline__ float2 ar_cj(float2 a) { return make_float2(a.x, -a.y); }
static __device__ __forceinline__ double ar_cj(double a) { return a; }
static __device__ __forceinline__ double2 ar_cj(double2 a) { return make_double2(a.x, -a.y); }
static __device__ __forceinline__ float ar_mul(float a, float b) { return a * b; }
static __device__ __forceinline__ float2 ar_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
static __device__ __forceinline__ double ar_mul(double a, double b) { return a * b; }
static __device__ __forceinline__ double2 ar_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
static __device__ __forceinline__ float ar_add(float a, float b) { return a + b; }
static __device__ __forceinline__ float2 ar_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
static __device__ __forceinline__ double ar_add(double a, double b) { return a + b; }
static __device__ __forceinline__ double2 ar_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
static __device__ __forceinline__ float ar_nrm(float a) { return a * a; }
static __device__ __forceinline__ float ar_nrm(float2 a) { return a.x * a.x + a.y * a.y; }
static __device__ __forceinline__ double ar_nrm(double a) { return a * a; }
static __device__ __forceinline__ double ar_nrm(double2 a) { return a.x * a.x + a.y * a.y; }
static __device__ __forceinline__ double ar_wide(float a) { return (double)a; }
static __device__ __forceinline__ double2 ar_wide(float2 a) { return make_double2((double)a.x, (double)a.y); }
static __device__ __forceinline__ float ar_narrow(double a) { return (float)a; }
static __device__ __forceinline__ float2 ar_narrow(double2 a) { return make_float2((float)a.x, (float)a.y); }
static __device__ __forceinline__ double ar_scale(double a, double s) { return a * s; }
static __device__ __forceinline__ double2 ar_scale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }
static __device__ __forceinline__ double ar_over(double a, double s) { return a / s; }
static __device__ __forceinline__ double2 ar_over(double2 a, double s) { return make_double2(a.x / s, a.y / s); }
static __device__ __forceinline__ double ar_re(double a) { return a; }
static __device__ __forceinline__ double ar_re(double2 a) { return a.x; }
static __device__ __forceinline__ double ar_im(double) { return 0.0; }
static __device__ __forceinline__ double ar_im(double2 a) { return a.y; }
static __device__ __forceinline__ void ar_set(double &d, double re, double) { d = re; }
static __device__ __forceinline__ void ar_set(double2 &d, double re, double im) { d = make_double2(re, im); }
static __device__ __forceinline__ void ar_set(float &d, float re, float) { d = re; }
static __device__ __forceinline__ void ar_set(float2 &d, float re, float im) { d = make_float2(re, im); }
static __device__ __forceinline__ bool ar_finite(float a) { return isfinite(a); }
static __device__ __forceinline__ bool ar_finite(float2 a) { return isfinite(a.x) && isfinite(a.y); }

// the sum over the wave's 64 lanes: a butterfly, so every lane ends with the same bits
static __device__ __forceinline__ double ar_wsum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ double2 ar_wsum(double2 v) { return make_double2(ar_wsum(v.x), ar_wsum(v.y)); }
static __device__ __forceinline__ float ar_up(float v) { return __shfl_up(v, 1, 64); }
static __device__ __forceinline__ float2 ar_up(float2 v) { return make_float2(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64)); }
// orders the LDS traffic of one wave's lanes where no workgroup barrier stands between a write and another lane's read
static __device__ __forceinline__ void ar_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool C> static __device__ __forceinline__ const typename ArT<C>::S *ar_segment(const ArArgs &A, int64_t sl) {
    const int64_t s = A.seg0 + sl, r = s / A.nframes, g = s - r * A.nframes;
    return (const typename ArT<C>::S *)A.x + r * A.x_ld + A.first + g * A.hop;
}

// ---- the record: sums of the tiles and the check for values that are not finite --------------------------------------------------
template <bool C> static __global__ __launch_bounds__(256) void k_ar_scan(ArArgs A, int64_t chunk, int64_t tiles, double *sums, int *flag) {
    typedef typename ArT<C>::S S;
    typedef typename ArT<C>::D D;
    __shared__ double red[4][2];
    const int64_t sl = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - sl * tiles;
    const S *x = ar_segment<C>(A, sl);
    const int64_t c0 = tile * chunk, c1 = c0 + chunk < A.n ? c0 + chunk : A.n;
    D s;
    ar_set(s, 0.0, 0.0);
    bool bad = false;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += 256) {
        const S v = x[i];
        bad |= !ar_finite(v);
        s = ar_add(s, ar_wide(v));
    }
    if (bad) *flag = 1;
    if (!sums) return;
    s = ar_wsum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = ar_re(s), red[threadIdx.x >> 6][1] = ar_im(s);
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        sums[2 * blockIdx.x + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

static __global__ __launch_bounds__(64) void k_ar_mean(ArArgs A, int64_t tiles, const double *sums, double *mean) {
    const int64_t sl = blockIdx.x;
    double re = 0.0, im = 0.0;
    if (A.detrend == 1) {
        for (int64_t t = threadIdx.x; t < tiles; t += 64) re += sums[2 * (sl * tiles + t)], im += sums[2 * (sl * tiles + t) + 1];
        re = ar_wsum(re) / (double)A.n, im = ar_wsum(im) / (double)A.n;
    } else if (A.detrend == 2)
        re = A.mre, im = A.mim;
    if (threadIdx.x == 0) mean[2 * sl] = re, mean[2 * sl + 1] = im;
}

// ---- Burg ---------------------------------------------------------------------------------------------------------------------------
template <bool C, int SPL, int NW> static __global__ __launch_bounds__(NW == 1 ? 64 * BURG_WAVE_SEGS : 64 * NW) void k_burg(ArArgs A) {
    typedef typename ArT<C>::S S;
    typedef typename ArT<C>::D D;
    constexpr int SEGS = NW == 1 ? BURG_WAVE_SEGS : 1, NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sw = NW == 1 ? wave : 0, t = NW == 1 ? lane : tid;
    const int64_t sl = (int64_t)blockIdx.x * SEGS + sw;
    if (sl >= A.nseg) return;                                           // the wave form's ragged last workgroup: whole waves leave
    const int n = (int)A.n, p = A.p, off = NT * SPL - n;
    D *abuf = (D *)ar_lds + (size_t)sw * 2 * p;                          // [2][p]: a[j] at j - 1; the launch sizes the LDS by the order
    double *red = (double *)((D *)ar_lds + 2 * p);                       // NW > 1: [2][NW][4]
    S *bnd = (S *)(red + 2 * NW * 4);                                    // NW > 1: [2][NW][2]
    const S *x = ar_segment<C>(A, sl);
    const int64_t o = sl * A.out_ld;                                     // the pointers are the pass's own
    D *a_out = (D *)A.a + o, *k_out = (D *)A.k + o;
    double *e_out = A.e + o;

    S f[SPL], b[SPL];
    const int i0 = t * SPL - off;                                       // the sample in this lane's first slot; below zero: no sample
    S before = x[i0 > 0 ? i0 - 1 : 0];
#pragma unroll
    for (int j = 0; j < SPL; ++j) f[j] = x[i0 + j > 0 ? i0 + j : 0];
    D mu;
    ar_set(mu, 0.0, 0.0);
    if (A.detrend == 1) {
        D s;
        ar_set(s, 0.0, 0.0);
#pragma unroll
        for (int j = 0; j < SPL; ++j)
            if (i0 + j >= 0) s = ar_add(s, ar_wide(f[j]));
        s = ar_wsum(s);
        if (NW > 1) {
            if (lane == 0) red[wave * 4] = ar_re(s), red[wave * 4 + 1] = ar_im(s);
            __syncthreads();
            double re = 0.0, im = 0.0;
            for (int w = 0; w < NW; ++w) re += red[w * 4], im += red[w * 4 + 1];
            ar_set(s, re, im);
        }
        mu = ar_over(s, (double)n);                                      // a division: the mean of a constant record is that constant
    } else if (A.detrend == 2)
        ar_set(mu, A.mre, A.mim);
    const D nmu = ar_scale(mu, -1.0);
    double e0 = 0.0;
    S zero;
    ar_set(zero, 0.f, 0.f);
    before = i0 >= 1 ? ar_narrow(ar_add(ar_wide(before), nmu)) : zero;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        f[j] = i0 + j >= 0 ? ar_narrow(ar_add(ar_wide(f[j]), nmu)) : zero;
        e0 += (double)ar_nrm(f[j]);
    }
#pragma unroll
    for (int j = SPL - 1; j >= 1; --j) b[j] = f[j - 1];                 // b is held one sample late
    b[0] = before;
    e0 = ar_wsum(e0);
    if (NW > 1) {
        if (lane == 0) red[(NW + wave) * 4] = e0;                        // the second set: order 1 takes the first again
        __syncthreads();
        e0 = 0.0;
        for (int w = 0; w < NW; ++w) e0 += red[(NW + w) * 4];
    }
    double E = e0 / (double)n;
    if (t == 0) e_out[0] = E;

#pragma unroll 1
    for (int m = 1; m <= p; ++m) {
        const int z = off + m - 1 - t * SPL;                            // sample m - 1 leaves the sums
        if (z >= 0 && z < SPL) {
#pragma unroll
            for (int j = 0; j < SPL; ++j)
                if (j == z) ar_set(f[j], 0.f, 0.f);
        }
        D num;
        ar_set(num, 0.0, 0.0);
        double den = 0.0;
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            num = ar_add(num, ar_wide(ar_mul(f[j], ar_cj(b[j]))));
            den += (double)(ar_nrm(f[j]) + ar_nrm(b[j]));
        }
        num = ar_wsum(num);
        den = ar_wsum(den);
        const int par = (m & 1) ^ 1;
        if (NW > 1) {
            double *rs = red + (par * NW + wave) * 4;
            S *bs = bnd + (par * NW + wave) * 2;
            if (lane == 0) rs[0] = ar_re(num), rs[1] = ar_im(num), rs[2] = den;
            if (lane == 63) bs[0] = f[SPL - 1], bs[1] = b[SPL - 1];
            __syncthreads();                                            // the order's one barrier
            double re = 0.0, im = 0.0;
            den = 0.0;
            for (int w = 0; w < NW; ++w) {
                const double *r = red + (par * NW + w) * 4;
                re += r[0], im += r[1], den += r[2];
            }
            ar_set(num, re, im);
        }
        D k;
        ar_set(k, 0.0, 0.0);
        if (den > 0.0) k = ar_scale(num, -2.0 / den);
        E *= 1.0 - ar_nrm(k);
        if (!(E > 0.0)) E = 0.0;                                        // float32 products can put |k| a rounding above 1: never a negative power
        // the step-up, beside the recursion: order m - 1 in one buffer, order m into the other
        const D *ao = abuf + ((m & 1) ? 0 : p);
        D *an = abuf + ((m & 1) ? p : 0);
        for (int j = t + 1; j <= m; j += NT) an[j - 1] = j == m ? k : ar_add(ao[j - 1], ar_mul(k, ar_cj(ao[m - j - 1])));
        if (t == 0) k_out[m - 1] = k, e_out[m] = E;
        const S ks = ar_narrow(k), kc = ar_cj(ks);
        S bn[SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            bn[j] = ar_add(b[j], ar_mul(kc, f[j]));
            f[j] = ar_add(f[j], ar_mul(ks, b[j]));
        }
        S in = ar_up(bn[SPL - 1]);
        if (lane == 0) {
            ar_set(in, 0.f, 0.f);
            if (NW > 1 && wave > 0) {
                const S *bs = bnd + (par * NW + wave - 1) * 2;
                in = ar_add(bs[1], ar_mul(kc, bs[0]));
            }
        }
#pragma unroll
        for (int j = SPL - 1; j >= 1; --j) b[j] = bn[j - 1];
        b[0] = in;
        if (NW == 1) ar_wave_sync();
    }
    if (NW > 1) __syncthreads();
    const D *af = abuf + ((p & 1) ? p : 0);
    for (int j = t; j <= p; j += NT) {
        D v;
        ar_set(v, 1.0, 0.0);
        if (j) v = af[j - 1];
        a_out[j] = v;
    }
}

// ---- Yule-Walker ---------------------------------------------------------------------------------------------------------------------
template <bool C> static __global__ __launch_bounds__(256) void k_ar_lags(ArArgs A, int64_t chunk, int64_t tiles, const double *mean, void *part_) {
    typedef typename ArT<C>::S S;
    typedef typename ArT<C>::D D;
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_lds[];
    S *stage = (S *)ar_lds;                                              // [AR_MAX_ORDER + AR_STAGE]: sample sb + j at AR_MAX_ORDER + j
    D *share = (D *)(stage + AR_MAX_ORDER + AR_STAGE);                   // [nsub][p + 1]
    const int tid = threadIdx.x, p = A.p, L = p + 1;
    const int64_t sl = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - sl * tiles;
    const S *x = ar_segment<C>(A, sl);
    D nmu;
    ar_set(nmu, -mean[2 * sl], -mean[2 * sl + 1]);
    const int64_t c0 = tile * chunk, c1 = c0 + chunk < A.n ? c0 + chunk : A.n;
    const int nsub = L >= 256 ? 1 : 256 / L, items = nsub * L;           // items <= 257: two to a thread at the most
    D acc[2];
    ar_set(acc[0], 0.0, 0.0);
    ar_set(acc[1], 0.0, 0.0);
    for (int64_t sb = c0; sb < c1; sb += AR_STAGE) {
        const int len = c1 - sb < AR_STAGE ? (int)(c1 - sb) : AR_STAGE, run = (len + nsub - 1) / nsub;
        __syncthreads();
        for (int j = tid - p; j < len; j += 256) {
            const int64_t i = sb + j;
            S v;
            ar_set(v, 0.f, 0.f);
            if (i >= 0 && i < c1) v = ar_narrow(ar_add(ar_wide(x[i]), nmu));
            stage[AR_MAX_ORDER + j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int item = tid + 256 * q;
            if (item >= items) break;
            const int u = item / L, l = item - u * L;
            const int j1 = (u + 1) * run < len ? (u + 1) * run : len;
            D s = acc[q];
            for (int j = u * run; j < j1; ++j) s = ar_add(s, ar_wide(ar_mul(stage[AR_MAX_ORDER + j], ar_cj(stage[AR_MAX_ORDER + j - l]))));
            acc[q] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (tid + 256 * q < items) share[tid + 256 * q] = acc[q];
    __syncthreads();
    D *part = (D *)part_ + ((int64_t)blockIdx.x) * L;
    for (int l = tid; l < L; l += 256) {
        D s = share[l];
        for (int u = 1; u < nsub; ++u) s = ar_add(s, share[u * L + l]);
        part[l] = s;
    }
}

template <bool C> static __global__ __launch_bounds__(256) void k_levinson(ArArgs A, int64_t tiles, const void *part_) {
    typedef typename ArT<C>::D D;
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = A.p, L = p + 1;
    const int64_t sl = (int64_t)blockIdx.x * 4 + wave;
    if (sl >= A.nseg) return;                                           // whole waves leave; there is no workgroup barrier below
    D *r = (D *)ar_lds + (size_t)wave * (3 * p + 2);                     // [p + 2] lags, then [2][p] coefficients: sized by the order
    D *abuf = r + p + 2;
    const D *part = (const D *)part_ + sl * tiles * L;
    const int64_t o = sl * A.out_ld;
    D *a_out = (D *)A.a + o, *k_out = (D *)A.k + o;
    double *e_out = A.e + o;
    for (int l = lane; l < L; l += 64) {
        D s = part[l];
        for (int64_t t = 1; t < tiles; ++t) s = ar_add(s, part[t * L + l]);
        r[l] = ar_over(s, (double)A.n);
    }
    ar_wave_sync();
    double E = ar_re(r[0]);
    if (!(E > 0.0)) E = 0.0;                                            // the zero record: the zero model
    if (lane == 0) e_out[0] = E;
    for (int m = 1; m <= p; ++m) {
        const D *ao = abuf + ((m & 1) ? 0 : p);
        D *an = abuf + ((m & 1) ? p : 0);
        D acc;
        ar_set(acc, 0.0, 0.0);
        for (int j = lane; j < m; j += 64) acc = ar_add(acc, j ? ar_mul(ao[j - 1], r[m - j]) : r[m]);
        acc = ar_wsum(acc);
        D k;
        ar_set(k, 0.0, 0.0);
        if (E > 0.0) k = ar_scale(acc, -1.0 / E);
        E *= 1.0 - ar_nrm(k);
        if (!(E > 0.0)) E = 0.0;
        for (int j = lane + 1; j <= m; j += 64) an[j - 1] = j == m ? k : ar_add(ao[j - 1], ar_mul(k, ar_cj(ao[m - j - 1])));
        if (lane == 0) k_out[m - 1] = k, e_out[m] = E;
        ar_wave_sync();
    }
    const D *af = abuf + ((p & 1) ? p : 0);
    for (int j = lane; j <= p; j += 64) {
        D v;
        ar_set(v, 1.0, 0.0);
        if (j) v = af[j - 1];
        a_out[j] = v;
    }
}

// ---- the spectrum of a model -----------------------------------------------------------------------------------------------------------
template <bool C, bool O64> static __global__ __launch_bounds__(256) void k_ar_psd(const void *a_, int64_t a_ld, const double *e, int64_t e_ld, int p,
                                                                                    int64_t bpm, int64_t m, double start, double step, double scale,
                                                                                    void *P_, int64_t P_ld) {
    typedef typename ArT<C>::D D;
    __shared__ double2 coef[AR_MAX_ORDER + 1];
    const int64_t model = (int64_t)blockIdx.x / bpm, q = ((int64_t)blockIdx.x - model * bpm) * 256 + threadIdx.x;
    const D *a = (const D *)a_ + model * a_ld;
    for (int j = threadIdx.x; j <= p; j += 256) {
        const D v = a[j];
        coef[j] = make_double2(ar_re(v), ar_im(v));
    }
    __syncthreads();
    if (q >= m) return;
    const double E = e[model * e_ld];
    double out = 0.0;
    if (E != 0.0) {
        const double nu = __dadd_rn(start, __dmul_rn((double)q, step));   // two roundings, as the definition's: no fused multiply-add
        const double fr = nu - floor(nu);                               // the phase of a turn, reduced in float64
        double sn, cs;
        sincospi(-2.0 * fr, &sn, &cs);
        double2 acc = coef[p];
        for (int j = p - 1; j >= 0; --j) {
            const double2 c = coef[j];
            acc = make_double2(acc.x * cs - acc.y * sn + c.x, acc.x * sn + acc.y * cs + c.y);
        }
        out = scale * E / (acc.x * acc.x + acc.y * acc.y);
    }
    if (O64) ((double *)P_)[model * P_ld + q] = out;
    else ((float *)P_)[model * P_ld + q] = (float)out;
}

// ---- launch glue -------------------------------------------------------------------------------------------------------------------------
static bool ar_args_ok(const ArArgs &a) {
    return a.x && a.a && a.e && a.k && a.n >= 2 && a.n <= YULE_MAX_N && a.p >= 1 && a.p <= AR_MAX_ORDER && a.p <= a.n / 2 && a.nseg >= 1 &&
           a.nseg <= AR_PASS_SEGS && a.nframes >= 1 && a.seg0 >= 0 && a.hop >= 1 && a.first >= 0 && a.out_ld >= a.p + 1 && a.detrend >= 0 &&
           a.detrend <= 2;
}

int launch_ar_scan(LaunchCtx c, const ArArgs &a, int64_t chunk, int64_t tiles, double *sums, int *flag) {
    if (!ar_args_ok(a) || !flag || chunk < 1 || tiles < 1 || tiles * chunk < a.n || (tiles - 1) * chunk >= a.n || a.nseg * tiles > 0x7fffffff) return -1;
    const dim3 grid((unsigned)(a.nseg * tiles));
    if (a.cplx) hipLaunchKernelGGL(k_ar_scan<true>, grid, dim3(256), 0, c.stream, a, chunk, tiles, sums, flag);
    else hipLaunchKernelGGL(k_ar_scan<false>, grid, dim3(256), 0, c.stream, a, chunk, tiles, sums, flag);
    return 0;
}

int launch_ar_mean(LaunchCtx c, const ArArgs &a, int64_t tiles, const double *sums, double *mean) {
    if (!ar_args_ok(a) || !mean || (a.detrend == 1 && !sums) || tiles < 1) return -1;
    hipLaunchKernelGGL(k_ar_mean, dim3((unsigned)a.nseg), dim3(64), 0, c.stream, a, tiles, sums, mean);
    return 0;
}

template <bool C, int SPL, int NW> static int burg_go(LaunchCtx c, const ArArgs &a) {
    typedef typename ArT<C>::S S;
    typedef typename ArT<C>::D D;
    constexpr int SEGS = NW == 1 ? BURG_WAVE_SEGS : 1;
    if (a.n > (int64_t)64 * NW * SPL) return -1;
    const size_t lds = (size_t)SEGS * 2 * a.p * sizeof(D) + (NW > 1 ? (size_t)2 * NW * (4 * sizeof(double) + 2 * sizeof(S)) : 0);
    static_assert((size_t)BURG_WAVE_SEGS * 2 * AR_MAX_ORDER * 16 + 2 * 16 * 48 <= 64 * 1024, "k_burg stays within the LDS a launch gets unasked");
    hipLaunchKernelGGL((k_burg<C, SPL, NW>), dim3((unsigned)((a.nseg + SEGS - 1) / SEGS)), dim3(NW == 1 ? 64 * SEGS : 64 * NW), lds, c.stream, a);
    return 0;
}

template <bool C> static int burg_pick(LaunchCtx c, const ArArgs &a, int spl, int nw) {
    switch (nw * 100 + spl) {
    case 101: return burg_go<C, 1, 1>(c, a);
    case 102: return burg_go<C, 2, 1>(c, a);
    case 104: return burg_go<C, 4, 1>(c, a);
    case 108: return burg_go<C, 8, 1>(c, a);
    case 116: return burg_go<C, 16, 1>(c, a);
    case 408: return burg_go<C, 8, 4>(c, a);
    case 416: return burg_go<C, 16, 4>(c, a);
    case 816: return burg_go<C, 16, 8>(c, a);
    case 1616: return burg_go<C, 16, 16>(c, a);
    }
    return -1;
}

int launch_burg(LaunchCtx c, const ArArgs &a, int spl, int nw) {
    if (!ar_args_ok(a) || a.n > BURG_MAX_N) return -1;
    return a.cplx ? burg_pick<true>(c, a, spl, nw) : burg_pick<false>(c, a, spl, nw);
}

int launch_ar_lags(LaunchCtx c, const ArArgs &a, int64_t chunk, int64_t tiles, const double *mean, void *part) {
    if (!ar_args_ok(a) || !mean || !part || chunk < AR_STAGE || chunk % AR_STAGE || tiles < 1 || tiles > AR_MAX_TILES || tiles * chunk < a.n ||
        (tiles - 1) * chunk >= a.n || a.nseg * tiles > 0x7fffffff)
        return -1;
    const dim3 grid((unsigned)(a.nseg * tiles));
    const size_t el = a.cplx ? 16 : 8;
    const size_t lds = (size_t)(AR_STAGE + AR_MAX_ORDER) * (el / 2) + (size_t)2 * AR_MAX_ORDER * el;
    static_assert((size_t)(AR_STAGE + AR_MAX_ORDER) * 8 + 2 * AR_MAX_ORDER * 16 <= 64 * 1024, "k_ar_lags stays within the LDS a launch gets unasked");
    if (a.cplx) hipLaunchKernelGGL(k_ar_lags<true>, grid, dim3(256), lds, c.stream, a, chunk, tiles, mean, part);
    else hipLaunchKernelGGL(k_ar_lags<false>, grid, dim3(256), lds, c.stream, a, chunk, tiles, mean, part);
    return 0;
}

int launch_levinson(LaunchCtx c, const ArArgs &a, int64_t tiles, const void *part) {
    if (!ar_args_ok(a) || !part || tiles < 1 || tiles > AR_MAX_TILES) return -1;
    const size_t lds = (size_t)4 * (3 * a.p + 2) * (a.cplx ? 16 : 8);
    static_assert((size_t)4 * (3 * AR_MAX_ORDER + 2) * 16 <= 64 * 1024, "k_levinson stays within the LDS a launch gets unasked");
    const dim3 grid((unsigned)((a.nseg + 3) / 4));
    if (a.cplx) hipLaunchKernelGGL(k_levinson<true>, grid, dim3(256), lds, c.stream, a, tiles, part);
    else hipLaunchKernelGGL(k_levinson<false>, grid, dim3(256), lds, c.stream, a, tiles, part);
    return 0;
}

int launch_ar_psd(LaunchCtx c, const void *a, bool cplx, int64_t a_ld, const double *e, int64_t e_ld, int p, int64_t nmodels, int64_t m,
                  double start, double step, double scale, bool out64, void *P, int64_t P_ld) {
    if (!a || !e || !P || p < 0 || p > AR_MAX_ORDER || a_ld < p + 1 || e_ld < 1 || nmodels < 1 || m < 1 || P_ld < m) return -1;
    const int64_t bpm = (m + 255) / 256;
    if (bpm > 0x7fffffff / nmodels) return -1;
    const dim3 grid((unsigned)(bpm * nmodels));
#define AR_PSD_GO(CC, OO) hipLaunchKernelGGL((k_ar_psd<CC, OO>), grid, dim3(256), 0, c.stream, a, a_ld, e, e_ld, p, bpm, m, start, step, scale, P, P_ld)
    if (cplx && out64) AR_PSD_GO(true, true);
    else if (cplx) AR_PSD_GO(true, false);
    else if (out64) AR_PSD_GO(false, true);
    else AR_PSD_GO(false, false);
#undef AR_PSD_GO
    return 0;
}

}   // namespace sp
