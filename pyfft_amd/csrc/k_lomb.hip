// k_lomb.hip -- the generalised Lomb-Scargle periodogram of an unevenly sampled record (Lomb 1976; Scargle 1982; Zechmeister &
// Kuerster 2009; scipy.signal.lombscargle of scipy 1.15 with all its options).  Times t[N] (float64) are shared by the rows y[r][N];
// with e(p) = exp(2 pi i p), phi = f (t - t_ref), normalised weights wn and d_r = y_r - m_r everything scipy computes follows from
// three complex sums per frequency, taken in ONE pass over the samples:
//   A1 = sum w32 e(phi) = C + iS     A2 = sum w32 e(2 phi) = C2 + iS2     B_r = sum wy32_r e(phi) = YC' + iYS'
// and from the totals W = sum w32, Y'_r = sum wy32_r, YY'_r = sum wy32_r d_r (launch.h).  scipy's second pass at the offset tau is a
// rotation of the same sums (k_lomb_finish).  m_r is a conditioning offset only: YC = YC' + m C, Y = Y' + m W, and so on.
// Kernels:
//   k_lomb_wsum, k_lomb_prep, k_lomb_totals   the record prepared once per call: t - t_ref in float64, w32, wy32 (the product formed
//           in float64), the totals by a two-stage reduction in a fixed order, and a status word for what a record must not hold.
//   k_lomb_sums   the hot path.  One lane owns one frequency; a workgroup owns 256 frequencies, one group of R rows and one run of
//           samples.  The samples are wave-uniform: a sub-run of LOMB_SUB of them is staged in LDS and read back as broadcasts, 16
//           bytes of (t', w32) and 16 or 32 of the rows' products per sample.  Per (sample, frequency): one float64 product, its
//           reduction p - rint(p) in float64, the turn rounded to float32, the hardware sine and cosine of a turn, e(2 phi) from
//           c^2 - s^2 and 2cs, and 4 + 2R float32 FMAs.  Sums run in float32 inside a sub-run and in float64 registers across.
//   k_lomb_reduce  the runs of a frequency added in ascending order in float64: the sums sp_lomb_sums hands out.
//   k_lomb_finish  scipy's body on those sums, in float64, one thread per (row, frequency).
// No atomics anywhere: two calls agree bitwise.
#include "launch.h"
namespace sp {

typedef float f2v __attribute__((ext_vector_type(2)));

// the block's sum of one value per thread, added pairwise in a fixed order; every thread gets it
static __device__ __forceinline__ double lomb_block_sum(double *red, double v) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

static __global__ __launch_bounds__(256) void k_lomb_wsum(LombPrepArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t n0 = blockIdx.x * a.len;
    const int64_t n1 = n0 + a.len < a.N ? n0 + a.len : a.N;
    double s = 0.0;
    bool bad_t = false, bad_w = false;
    for (int64_t n = n0 + tid; n < n1; n += 256) {
        bad_t |= !isfinite(a.t[n]);
        const double wv = a.w ? a.w[n] : 1.0;
        bad_w |= !(wv >= 0.0) || !isfinite(wv);
        s += wv;
    }
    if (bad_t) a.status[0] = 1;
    if (bad_w) a.status[1] = 1;
    s = lomb_block_sum(red, s);
    if (tid == 0) a.wpart[blockIdx.x] = s;
}

// column c0 + blockIdx.y of the prepared record.  Column 0: the heads and the sum of w32; column 1 + q: column q of the padded rows
// (group q / RP, place q % RP).  65535 rows are 65537 columns, more than a grid's y: the launcher deals the columns to launches.
static __global__ __launch_bounds__(256) void k_lomb_prep(LombPrepArgs a, int64_t c0) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double wsum = a.wnorm;
    if (!(wsum > 0.0)) {
        wsum = 0.0;
        for (int64_t b = 0; b < a.blocks; ++b) wsum += a.wpart[b];
    }
    const bool ok = wsum > 0.0 && isfinite(wsum);
    if (!ok && tid == 0) a.status[2] = 1;
    const double inv = ok ? 1.0 / wsum : 0.0;
    const int64_t n0 = blockIdx.x * a.len;
    const int64_t n1 = n0 + a.len < a.npad ? n0 + a.len : a.npad;
    const int64_t col = c0 + blockIdx.y;
    if (col == 0) {
        double s = 0.0;
        for (int64_t n = n0 + tid; n < n1; n += 256) {
            LombHead h{0.0, 0.f, 0.f};
            if (n < a.N) {
                h.t = a.t[n] - a.t_ref;
                h.w = (float)((a.w ? a.w[n] : 1.0) * inv);
                s += (double)h.w;
            }
            a.head[n] = h;
        }
        s = lomb_block_sum(red, s);
        if (tid == 0) a.tpart[blockIdx.x] = s;
        return;
    }
    const int64_t q = col - 1;
    const int64_t grp = q / a.RP;
    const int k = (int)(q % a.RP);
    const int64_t row = grp * a.R + k;
    float *dst = a.wy + grp * a.npad * a.RP + k;
    if (k >= a.R || row >= a.batch) {                  // padding: a place or a row that does not exist
        for (int64_t n = n0 + tid; n < n1; n += 256) dst[n * a.RP] = 0.f;
        return;
    }
    const double m = a.mean ? a.mean[row] : 0.0;
    const float *yr = a.y + row * a.y_ld;
    double s1 = 0.0, s2 = 0.0;
    bool bad_y = false;
    for (int64_t n = n0 + tid; n < n1; n += 256) {
        float v = 0.f;
        if (n < a.N) {
            const float yv = yr[n];
            bad_y |= !isfinite(yv);
            const double d = (double)yv - m;
            v = (float)((a.w ? a.w[n] : 1.0) * inv * d);
            s1 += (double)v;
            s2 += (double)v * d;
        }
        dst[n * a.RP] = v;
    }
    if (bad_y) a.status[3] = 1;
    s1 = lomb_block_sum(red, s1);
    s2 = lomb_block_sum(red, s2);
    if (tid == 0) {
        a.tpart[(1 + 2 * row) * a.blocks + blockIdx.x] = s1;
        a.tpart[(2 + 2 * row) * a.blocks + blockIdx.x] = s2;
    }
}

static __global__ __launch_bounds__(256) void k_lomb_totals(LombPrepArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 1 + 2 * a.batch) return;
    double s = 0.0;
    for (int64_t b = 0; b < a.blocks; ++b) s += a.tpart[i * a.blocks + b];
    a.totals[i] = s;
}

template <int R>
static __global__ __launch_bounds__(LOMB_WG) void k_lomb_sums(LombSumArgs a) {
    constexpr int RP = lomb_rp(R), NV = lomb_nv(R), RA = R ? R : 1;
    __shared__ LombHead sh[LOMB_SUB];
    __shared__ float4 swy[RP ? LOMB_SUB * RP / 4 : 1];
    const int tid = threadIdx.x;
    const int j = blockIdx.x * LOMB_WG + tid;
    const double f = a.f[j < a.fcount ? j : a.fcount - 1];          // a lane past the list repeats the last frequency and stores nothing
    const int64_t s0 = (int64_t)blockIdx.y * a.run_len;
    const int64_t s1 = s0 + a.run_len < a.N4 ? s0 + a.run_len : a.N4;
    const float *wyg = a.wy + (int64_t)blockIdx.z * a.npad * RP;
    double d1r = 0.0, d1i = 0.0, d2r = 0.0, d2i = 0.0, dbr[RA], dbi[RA];
#pragma unroll
    for (int r = 0; r < RA; ++r) dbr[r] = dbi[r] = 0.0;
    for (int64_t pos = s0; pos < s1; pos += LOMB_SUB) {
        const int cnt = s1 - pos < LOMB_SUB ? (int)(s1 - pos) : LOMB_SUB;         // a multiple of 4
        // the whole piece is inside the arrays (npad = N4 + LOMB_SUB); what lies past the run's end is loaded and not used
        __syncthreads();
        sh[tid] = a.head[pos + tid];
        if constexpr (R > 0) {
            const float4 *src = (const float4 *)(wyg + pos * RP);
#pragma unroll
            for (int k = 0; k < RP / 4; ++k) swy[tid + LOMB_WG * k] = src[tid + LOMB_WG * k];
        }
        __syncthreads();
        f2v a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, b[RA];
#pragma unroll
        for (int r = 0; r < RA; ++r) b[r] = f2v{0.f, 0.f};
        for (int i0 = 0; i0 < cnt; i0 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u;
                const LombHead h = sh[i];
                double p = f * h.t;
                p -= rint(p);
                const float pf = (float)p;
                const float s = __builtin_amdgcn_sinf(pf), c = __builtin_amdgcn_cosf(pf);        // of a turn: |pf| <= 1/2
                const f2v e1 = {c, s};
                const f2v e2 = {fmaf(c, c, -(s * s)), 2.f * c * s};
                a1 += h.w * e1;
                a2 += h.w * e2;
                if constexpr (R > 0) {
                    float wv[RP];
#pragma unroll
                    for (int k = 0; k < RP / 4; ++k) {
                        const float4 q = swy[i * (RP / 4) + k];
                        wv[4 * k] = q.x, wv[4 * k + 1] = q.y, wv[4 * k + 2] = q.z, wv[4 * k + 3] = q.w;
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) b[r] += wv[r] * e1;
                }
            }
        }
        d1r += (double)a1.x, d1i += (double)a1.y, d2r += (double)a2.x, d2i += (double)a2.y;
        if constexpr (R > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) dbr[r] += (double)b[r].x, dbi[r] += (double)b[r].y;
        }
    }
    if (j >= a.fcount) return;
    double *p = a.partial + (((int64_t)blockIdx.z * a.split + blockIdx.y) * NV) * a.fcount + j;
    p[0] = d1r;
    p[(int64_t)a.fcount] = d1i;
    p[(int64_t)2 * a.fcount] = d2r;
    p[(int64_t)3 * a.fcount] = d2i;
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            p[(int64_t)(4 + 2 * r) * a.fcount] = dbr[r];
            p[(int64_t)(5 + 2 * r) * a.fcount] = dbi[r];
        }
    }
}

static __global__ __launch_bounds__(256) void k_lomb_reduce(const double *__restrict__ partial, int R, int64_t split, int fcount, int64_t g0,
                                                            int64_t batch, double *__restrict__ common, double *__restrict__ rows,
                                                            int64_t rows_ld) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= fcount) return;
    const int64_t g = blockIdx.y;
    const int nv = lomb_nv(R);
    const double *base = partial + g * split * nv * fcount + j;
    auto total = [&](int k) {
        double s = 0.0;
        for (int64_t r = 0; r < split; ++r) s += base[(r * nv + k) * fcount];
        return s;
    };
    if (g == 0 && common)
        for (int k = 0; k < 4; ++k) common[4 * (int64_t)j + k] = total(k);
    for (int r = 0; r < R; ++r) {
        const int64_t row = (g0 + g) * R + r;
        if (row >= batch) break;
        double *o = rows + 2 * (row * rows_ld + j);
        o[0] = total(4 + 2 * r);
        o[1] = total(5 + 2 * r);
    }
}

// scipy.signal.lombscargle's body on the sums, which are first divided by W: the weights then sum to one as scipy's do.  With a
// floating mean the offset m never enters: YC - Y C = YC' - Y' C.
static __global__ __launch_bounds__(256) void k_lomb_finish(const double *__restrict__ common, const double *__restrict__ rows, int64_t rows_ld,
                                                            const double *__restrict__ totals, const double *__restrict__ mean,
                                                            const double *__restrict__ f, int fcount, int64_t N, double t_ref, int fm,
                                                            int normalize, void *__restrict__ P, int64_t p_ld) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= fcount) return;
    const int64_t row = blockIdx.y;
    const double iw = 1.0 / totals[0];
    const double C = common[4 * (int64_t)j] * iw, S = common[4 * (int64_t)j + 1] * iw;
    const double C2 = common[4 * (int64_t)j + 2] * iw, S2 = common[4 * (int64_t)j + 3] * iw;
    const double *rw = rows + 2 * (row * rows_ld + j);
    const double Yp = totals[1 + 2 * row] * iw, YYp = totals[2 + 2 * row] * iw;
    const double m = mean ? mean[row] : 0.0;
    double YC = rw[0] * iw, YS = rw[1] * iw;
    double CC = 0.5 * (1.0 + C2), CS = 0.5 * S2;
    double SS = 1.0 - CC;
    if (fm) {
        YC -= Yp * C, YS -= Yp * S;
        CC -= C * C, SS -= S * S, CS -= C * S;
    } else {
        YC += m * C, YS += m * S;
    }
    const double tau = 0.5 * atan2(2.0 * CS, CC - SS);
    double st, ct;
    sincos(tau, &st, &ct);
    const double c2t = ct * ct - st * st, s2t = 2.0 * st * ct;
    const double YCt = YC * ct + YS * st, YSt = YS * ct - YC * st;
    double CCt = 0.5 * (1.0 + C2 * c2t + S2 * s2t);
    double SSt = 1.0 - CCt;
    if (fm) {
        const double Ct = C * ct + S * st, St = S * ct - C * st;
        CCt -= Ct * Ct, SSt -= St * St;
    }
    const double epsneg = 1.1102230246251565e-16;           // numpy.finfo(float64).epsneg
    if (CCt < epsneg) CCt = epsneg;
    if (SSt < epsneg) SSt = epsneg;
    const double av = YCt / CCt, bv = YSt / SSt;
    const double pg = 2.0 * (av * YCt + bv * YSt);
    const int64_t o = row * p_ld + j;
    if (normalize == 0) {
        ((float *)P)[o] = (float)(pg * ((double)N * 0.25));
    } else if (normalize == 1) {
        const double YY = fm ? YYp - Yp * Yp : YYp + 2.0 * m * Yp + m * m;
        ((float *)P)[o] = (float)(pg * (0.5 / YY));
    } else {
        // (a + ib) e^{i tau}, and the time origin put back: e(f t_ref), the product's rounding error kept by an FMA
        const double pr = f[j] * t_ref;
        const double turn = (pr - rint(pr)) + fma(f[j], t_ref, -pr);
        double so, co;
        sincospi(2.0 * turn, &so, &co);
        const double zr = av * ct - bv * st, zi = av * st + bv * ct;
        ((cf *)P)[o] = mk((float)(zr * co - zi * so), (float)(zr * so + zi * co));
    }
}

int launch_lomb_prep(LaunchCtx c, const LombPrepArgs &a) {
    if (a.N < 1 || a.batch < 0 || a.batch > 65535 || a.blocks < 1 || a.blocks > LOMB_PREP_BLOCKS || a.len < 1 || a.blocks * a.len < a.npad ||
        a.npad < a.N || !a.t || !a.wpart || !a.head || !a.tpart || !a.totals || !a.status || (a.batch > 0 && (!a.y || !a.wy || a.R < 1 || a.RP != lomb_rp(a.R))) ||
        a.rows_padded < 0 || a.rows_padded > 65536)
        return -1;
    hipLaunchKernelGGL(k_lomb_wsum, dim3((unsigned)a.blocks), dim3(256), 0, c.stream, a);
    for (int64_t c0 = 0; c0 < 1 + a.rows_padded; c0 += LOMB_PREP_COLS) {
        const int64_t nc = 1 + a.rows_padded - c0 < LOMB_PREP_COLS ? 1 + a.rows_padded - c0 : LOMB_PREP_COLS;
        hipLaunchKernelGGL(k_lomb_prep, dim3((unsigned)a.blocks, (unsigned)nc), dim3(256), 0, c.stream, a, c0);
    }
    hipLaunchKernelGGL(k_lomb_totals, dim3((unsigned)((1 + 2 * a.batch + 255) / 256)), dim3(256), 0, c.stream, a);
    return 0;
}

int launch_lomb_sums(LaunchCtx c, const LombSumArgs &a, int R, int64_t groups) {
    if (a.fcount < 1 || a.fcount > LOMB_MAX_M || a.split < 1 || a.split > 65535 || groups < 1 || groups > 65535 || a.run_len < 4 ||
        a.run_len % 4 || a.N4 % 4 || a.npad < a.N4 + LOMB_SUB || a.split * a.run_len < a.N4 || !a.head || !a.f || !a.partial ||
        (R > 0 && !a.wy))
        return -1;
    const dim3 grid((unsigned)((a.fcount + LOMB_WG - 1) / LOMB_WG), (unsigned)a.split, (unsigned)groups);
#define L_(RV)                                                                                          \
    case RV: hipLaunchKernelGGL(k_lomb_sums<RV>, grid, dim3(LOMB_WG), 0, c.stream, a); return 0;
    switch (R) {
        L_(0) L_(1) L_(4) L_(8)
    }
#undef L_
    return -1;
}

int launch_lomb_reduce(LaunchCtx c, const double *partial, int R, int64_t groups, int64_t split, int fcount, int64_t g0, int64_t batch,
                       double *common, double *rows, int64_t rows_ld) {
    if (fcount < 1 || groups < 1 || groups > 65535 || split < 1 || !partial || (R > 0 && !rows) || (R == 0 && !common)) return -1;
    hipLaunchKernelGGL(k_lomb_reduce, dim3((unsigned)((fcount + 255) / 256), (unsigned)groups), dim3(256), 0, c.stream, partial, R, split,
                       fcount, g0, batch, common, rows, rows_ld);
    return 0;
}

int launch_lomb_finish(LaunchCtx c, const double *common, const double *rows, int64_t rows_ld, const double *totals, const double *mean,
                       const double *f, int fcount, int64_t batch, int64_t N, double t_ref, int floating_mean, int normalize, void *P,
                       int64_t p_ld) {
    if (fcount < 1 || batch < 1 || batch > 65535 || normalize < 0 || normalize > 2 || !common || !rows || !totals || !f || !P) return -1;
    hipLaunchKernelGGL(k_lomb_finish, dim3((unsigned)((fcount + 255) / 256), (unsigned)batch), dim3(256), 0, c.stream, common, rows, rows_ld,
                       totals, mean, f, fcount, N, t_ref, floating_mean ? 1 : 0, normalize, P, p_ld);
    return 0;
}

}   // namespace sp
