// k_welch_opx.hip -- one-pass sharded Welch state for any segment that fits one workgroup transform and any hop
// (the shapes the carry / pipeline kernels do not take: non-power-of-two lengths through the in-workgroup Bluestein,
// hops that do not divide nfft, hop > nfft).
//
// Three launches behind k_op_estimate's mean estimate mu0:
//   k_welch_opx   per transform group: sum |X_g|^2 of its frames (X_g = FFT(w (x_g - mu0))) and the time-domain column sums
//                 c[j] = sum_g (x[g hop + j] - mu0) of the same frames -- float32 partials per group
//   k_opx_reduce  the column sums of both partial matrices in float64; and the corrections that turn sum_{j < own} c[j]
//                 (own = min(hop, n): the samples of each frame that no later frame starts on, i.e. every sample of
//                 [0, M hop) for hop <= n) into the sum of (x_i - mu0) over the shard's own samples i < nmean -- the gaps of
//                 hop > n and the tail up to nmean added, the frames' own samples at or past nmean removed, read directly
//   k_opx_finish  one workgroup: B = FFT(w c) = sum_g X_g (linearity), then the state of k_op_finish<EXPORT> over the n bins
//                 (k_welch.hip; applied by k_op_apply)
// The per-group partials are float32 (a group sums at most a few hundred frames); everything across groups is float64.
#include "launch.h"
#include <type_traits>
namespace sp {

#define SP_OPX_TOT_BLOCKS 32          // blocks of k_opx_reduce that sum the own-sample partials and the uncovered samples

template <class X, bool CPLX, bool PAIR>
__global__ __launch_bounds__(X::C::WG) void k_welch_opx(const void *__restrict__ x, const float *__restrict__ win, int hop,
                                                         int64_t nframes, int64_t fpg, const float *__restrict__ trend,
                                                         XfTables tb, float *__restrict__ partial, cf *__restrict__ cpart) {
    SP_KERNEL_PROLOGUE(X)
    // Bluestein (n <= L / 2): only the first half of a thread's slots holds samples -- window, loads and column sums of the other
    // half are never needed (XfBlue::fwd zeroes slots >= n).  Real input: the column sums are real.
    constexpr int RV = X::EXACT ? C::R : C::R / 2;
    using CS = typename std::conditional<CPLX, cf, float>::type;
    float w[RV], acc[C::R];
    CS cs[RV];
#pragma unroll
    for (int t = 0; t < C::R; ++t) acc[t] = 0.f;
#pragma unroll
    for (int t = 0; t < RV; ++t) {
        const int i = tid + C::T * t;
        w[t] = (X::EXACT || i < n) ? win[i] : 0.f;
        cs[t] = CS{};
    }
    const Trend tr = load_trend(trend);
    const int64_t gid = (int64_t)blockIdx.x * C::FPW + grp;
    // PAIR (real input): unit u is the frame pair (2u, 2u + 1) in one complex transform, z = f_a + i f_b
    const int64_t nunits = PAIR ? (nframes + 1) / 2 : nframes;
    for (int64_t i = 0; i < fpg; ++i) {
        const int64_t u = gid * fpg + i;
        // units past the end are clamped to the last one and weighted 0: every load is unconditional
        const bool on = u < nunits;
        const int64_t ga = PAIR ? 2 * (on ? u : nunits - 1) : (on ? u : nunits - 1);
        const bool has_b = PAIR && on && ga + 1 < nframes;
        const int64_t base_a = ga * hop, base_b = (has_b ? ga + 1 : ga) * hop;
        const float ka = on ? 1.f : 0.f, kb = has_b ? 1.f : 0.f;
        cf v[C::R];
#pragma unroll
        for (int t = RV; t < C::R; ++t) v[t] = mk(0.f, 0.f);
#pragma unroll
        for (int t = 0; t < RV; ++t) {
            const int j = tid + C::T * t;
            const int jj = (X::EXACT || j < n) ? j : n - 1;
            if constexpr (PAIR) {
                const float *xr = reinterpret_cast<const float *>(x);
                v[t] = mk(xr[base_a + jj], xr[base_b + jj]);
            } else {
                v[t] = load_sample(x, base_a + jj, CPLX);
            }
        }
#pragma unroll
        for (int t = 0; t < RV; ++t) {
            const int j = tid + C::T * t;
            const bool inb = X::EXACT || j < n;
            if constexpr (PAIR) {
                const float a = v[t].x - tr.m.x, b = v[t].y - tr.m.x;
                cs[t] += (inb ? ka : 0.f) * a + (inb ? kb : 0.f) * b;
                v[t] = mk(w[t] * a, kb * w[t] * b);
            } else {
                const cf d = v[t] - tr.m;
                const float kc = inb ? ka : 0.f;
                if constexpr (CPLX) cs[t] = cs[t] + kc * d;
                else cs[t] += kc * d.x;
                v[t] = w[t] * d;
            }
        }
        fwd_row(xf, v, lds, tid, n);
#pragma unroll
        for (int t = 0; t < C::R; ++t) acc[t] += ka * cnorm(v[t]);
    }
#pragma unroll
    for (int t = 0; t < C::R; ++t) partial[gid * X::L + tid + C::T * t] = acc[t];
#pragma unroll
    for (int t = 0; t < RV; ++t) {
        const int j = tid + C::T * t;
        if constexpr (CPLX) {
            if (X::EXACT || j < n) cpart[gid * n + j] = cs[t];
        } else {
            if (X::EXACT || j < n) cpart[gid * n + j] = mk(cs[t], 0.f);
        }
    }
}

// blocks [0, nbA): A[k] = sum_g partial[g][k] (k < n, row stride L); [nbA, nbA + nbC): csum = column sums of cpart[G][n]
// seen as [G][2n] floats; then SP_OPX_TOT_BLOCKS blocks, one (re, im) pair each into tpart: + the own samples (i < nmean)
// that no frame owns (u < ugap: gap samples g hop + own + j of hop > n; then the tail [M hop, nmean)), - the frames' own
// samples at or past nmean (j = i mod hop < own for i in [nmean, M hop)).
// 1024 threads: 32 columns x 32 row slices, 4 loads in flight per thread; deterministic order.
template <bool CPLX>
static __global__ __launch_bounds__(1024) void k_opx_reduce(const float *__restrict__ partial, int L, int n,
                                                             const float *__restrict__ cpart, int64_t G,
                                                             const void *__restrict__ x, const float *__restrict__ trend, int hop,
                                                             int64_t M, int64_t nmean, double *__restrict__ A,
                                                             double *__restrict__ csum, double *__restrict__ tpart) {
    __shared__ double sh[2][1024];
    const int nbA = (n + 31) / 32, nbC = (2 * n + 31) / 32;
    const int b = blockIdx.x;
    if (b < nbA + nbC) {
        const bool second = b >= nbA;
        const float *__restrict__ m = second ? cpart : partial;
        const int ld = second ? 2 * n : L, cols = second ? 2 * n : n;
        double *__restrict__ o = second ? csum : A;
        const int lane = threadIdx.x % 32, sl = threadIdx.x / 32;
        const int k = (b - (second ? nbA : 0)) * 32 + lane;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (k < cols) {
            int64_t g = sl;
            for (; g + 96 < G; g += 128) {
                const float a0 = m[g * ld + k], a1 = m[(g + 32) * ld + k], a2 = m[(g + 64) * ld + k], a3 = m[(g + 96) * ld + k];
                s0 += (double)a0;
                s1 += (double)a1;
                s2 += (double)a2;
                s3 += (double)a3;
            }
            for (; g < G; g += 32) s0 += (double)m[g * ld + k];
        }
        sh[0][sl * 32 + lane] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (sl == 0 && k < cols) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 32; ++q) t += sh[0][q * 32 + lane];
            o[k] = t;
        }
        return;
    }
    const int tb = b - nbA - nbC, nbt = (int)gridDim.x - nbA - nbC;
    const int64_t stride = (int64_t)nbt * 1024;
    double a = 0.0, c = 0.0;
    const cf mu = mk(trend[0], trend[1]);
    const int own = hop < n ? hop : n, gap = hop - own;
    const int64_t ugap = (int64_t)gap * M, cov = M * (int64_t)hop;
    const int64_t uend = ugap + (nmean > cov ? nmean - cov : 0);
    for (int64_t u = (int64_t)tb * 1024 + threadIdx.x; u < uend; u += stride) {
        const int64_t i = u < ugap ? (u / gap) * hop + own + (u % gap) : cov + (u - ugap);
        if (i < nmean) {
            const cf v = load_sample(x, i, CPLX) - mu;
            a += (double)v.x;
            c += (double)v.y;
        }
    }
    for (int64_t i = nmean + (int64_t)tb * 1024 + threadIdx.x; i < cov; i += stride) {
        if (i % hop < own) {
            const cf v = load_sample(x, i, CPLX) - mu;
            a -= (double)v.x;
            c -= (double)v.y;
        }
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = c;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tpart[2 * tb] = sh[0][0];
        tpart[2 * tb + 1] = sh[1][0];
    }
}

// one workgroup: B = FFT_n(w csum) = sum_g X_g, and the shard state (layout of k_op_finish<EXPORT>, k_welch.hip) over n bins.
// sym: the main kernel ran on frame pairs -- A[k] = (sum |Z[k]|^2 + sum |Z[n - k]|^2) / 2
template <class X>
static __global__ __launch_bounds__(X::C::WG) void k_opx_finish(const float *__restrict__ win, const double *__restrict__ A,
                                                                 const double *__restrict__ csum, const double *__restrict__ tpart,
                                                                 int nbt, const float *__restrict__ trend, int hop, int64_t M,
                                                                 int64_t nmean, int sym, XfTables tb, double *__restrict__ out) {
    SP_KERNEL_PROLOGUE(X)
    __shared__ double red[32][2];
    const int own = hop < n ? hop : n;
    cf v[C::R];
    double sr = 0.0, si = 0.0;                  // sum_{j < own} c[j]
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int i = tid + C::T * t;
        const bool ok = grp == 0 && (X::EXACT || i < n);
        const int ic = ok ? i : 0;
        const double wn = ok ? (double)win[ic] : 0.0;
        const double cr = csum[2 * ic], ci = csum[2 * ic + 1];
        if (ok && i < own) {
            sr += cr;
            si += ci;
        }
        v[t] = mk((float)(wn * cr), (float)(wn * ci));
    }
    sr = wave_sum64d(sr);
    si = wave_sum64d(si);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = sr;
        red[threadIdx.x >> 6][1] = si;
    }
    __syncthreads();
    xf.fwd(v, lds, tid, n);
    const double mr = (double)trend[0], mi = (double)trend[1];
    if (grp == 0) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int k = tid + C::T * t;
            if (!X::EXACT && k >= n) continue;
            const double a = sym ? 0.5 * (A[k] + A[k ? n - k : 0]) : A[k];
            const double br = (double)v[t].x, bi = (double)v[t].y;
            out[k] = a;
            out[n + 2 * k] = br;
            out[n + 2 * k + 1] = bi;
            out[3 * n + 2 * k] = mr * br + mi * bi;          // conj(mu0) B
            out[3 * n + 2 * k + 1] = mr * bi - mi * br;
        }
    }
    if (threadIdx.x == 0) {
        double tr = 0.0, ti = 0.0;
        for (int q = 0; q < ((int)blockDim.x + 63) / 64; ++q) {
            tr += red[q][0];
            ti += red[q][1];
        }
        for (int q = 0; q < nbt; ++q) {
            tr += tpart[2 * q];
            ti += tpart[2 * q + 1];
        }
        double *sc = out + 5 * (int64_t)n;
        sc[0] = (double)M * mr;
        sc[1] = (double)M * mi;
        sc[2] = (double)M * (mr * mr + mi * mi);
        sc[3] = tr + (double)nmean * mr;
        sc[4] = ti + (double)nmean * mi;
        sc[5] = (double)M;
        sc[6] = (double)nmean;
        sc[7] = 0.0;
    }
}

int launch_welch_opx(LaunchCtx c, const void *x, bool cplx, bool pair, const float *win, int hop, int64_t nframes,
                     const float *trend, const Xf &xf, const RunPart &rp, float *partial, cf *cpart) {
    if (pair && cplx) return -1;
#define M_(XT)                                                                                        \
    if (pair)                                                                                         \
        hipLaunchKernelGGL((k_welch_opx<XT, false, true>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                           x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, cpart); \
    else if (cplx)                                                                                    \
        hipLaunchKernelGGL((k_welch_opx<XT, true, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                           x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, cpart); \
    else                                                                                              \
        hipLaunchKernelGGL((k_welch_opx<XT, false, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                           x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, cpart);
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

int launch_opx_reduce(LaunchCtx c, const float *partial, const cf *cpart, int64_t G, const Xf &xf, const void *x, bool cplx,
                      const float *trend, int hop, int64_t nframes, int64_t nmean, double *A, double *csum, double *tpart) {
    const int n = xf.tb.n;
    const dim3 grid((n + 31) / 32 + (2 * n + 31) / 32 + SP_OPX_TOT_BLOCKS);
    if (cplx)
        hipLaunchKernelGGL((k_opx_reduce<true>), grid, dim3(1024), 0, c.stream, partial, xf.L, n,
                           reinterpret_cast<const float *>(cpart), G, x, trend, hop, nframes, nmean, A, csum, tpart);
    else
        hipLaunchKernelGGL((k_opx_reduce<false>), grid, dim3(1024), 0, c.stream, partial, xf.L, n,
                           reinterpret_cast<const float *>(cpart), G, x, trend, hop, nframes, nmean, A, csum, tpart);
    return 0;
}

int opx_tot_blocks() { return SP_OPX_TOT_BLOCKS; }

int launch_opx_finish(LaunchCtx c, const float *win, const double *A, const double *csum, const double *tpart, const float *trend,
                      int hop, int64_t nframes, int64_t nmean, bool sym, const Xf &xf, double *out) {
#define M_(XT)                                                                                        \
    hipLaunchKernelGGL((k_opx_finish<XT>), dim3(1), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, win, A, csum, tpart, \
                       SP_OPX_TOT_BLOCKS, trend, hop, nframes, nmean, sym ? 1 : 0, xf.tb, out);
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

}   // namespace sp
