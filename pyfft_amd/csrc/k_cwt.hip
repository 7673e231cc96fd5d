// k_cwt.hip -- continuous wavelet transform by overlap-save: every scale of a stretch of record from ONE forward transform.
//   W[s][n] = sum_m g_s[m] x[n - m] over the zero-extended record,  g_s = IDFT(H_s),
//   H_s[k] = sqrt(2 pi s') psi0^(s' w_k),  w_k = 2 pi k / L for 0 < k <= L / 2, 0 elsewhere (analytic wavelets).
// All scales of a call share one geometry: frames of L samples, M = the largest margin, hop = L - 2 M.  Frame g covers the samples
// [g hop - M, g hop - M + L); samples outside the record are zero (clamped loads, selected to 0: every load is unconditional and every
// barrier is met, as in k_xcorr_frames).  A transform group loads its frame once, transforms it and keeps the spectrum -- in registers
// below 2048 points, in an LDS image of its own from there on (a thread reads back only what it wrote: no barrier) -- and then for
// every scale of its chunk multiplies by H_s, inverse-transforms (conj . forward . conj, as XfCzt::fwd) and uses the elements
// M .. M + hop - 1, the samples n = g hop .. < N.  Real records run as x + 0 i.  Grid: frame blocks x scale chunks x rows.
// The filter is evaluated on the fly, one v_exp_f32 per bin (one v_log_f32 more where p != 0), never read from an S x L table:
//   H_s[k] = exp(c_s + p ln u - a d^2 - b d),  u = k step_s,  d = u - u0,  step_s = 2 pi s' / L,  c_s = ln(norm sqrt(2 pi s') / L)
//   Morlet(w0): p = 0, a = 1/2, b = 0, u0 = w0;   Paul(m): p = m, a = 0, b = 1, u0 = 0
// (d is formed before it is squared: c + w0 u - u^2 / 2 - w0^2 / 2 would cancel 2e6 against 2e6 at the long scales.)
// Outputs, any combination, a uniform run-time branch each:
//   W        complex64 [rows][S][N], non-temporal stores;
//   gpart    sum over the frame's samples of |W|^2, one float per (row, scale, frame), summed in float64 in frame order by
//            k_cwt_gws_finish (no atomics);
//   recon    sum_s wr[s] W[s][n], complex64 [rows][N];  bandpow  sum_s wb[s] |W[s][n]|^2, float [rows][N]: accumulated in registers
//            across the scale loop and written once -- the ACC instantiations; the chunk is then the whole scale set.
#include "launch.h"
namespace sp {

constexpr bool cwt_stash(int L) { return L >= 2048; }
template <class C> constexpr size_t cwt_lds_bytes(int L) {
    return sizeof(cf) * (size_t)C::FPW * ((size_t)C::LDS_PER + (cwt_stash(L) ? (size_t)L : 0));
}

// sum of one value per thread over the T threads of a transform group, every thread gets it: inside a wave without LDS; the waves of a
// longer transform meet in the group's exchange image (every thread of the workgroup must call it then: barriers)
template <class C> __device__ __forceinline__ float cwt_group_sum(float v, cf *lds, int tid) {
    constexpr int W = C::T < 64 ? C::T : 64;
    v = group_lane_sum<W>(v);
    if constexpr (C::T > 64) {
        float *f = reinterpret_cast<float *>(lds);
        __syncthreads();                  // the image may still be read by the transform
        if ((tid & 63) == 0) f[tid >> 6] = v;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int j = 0; j < C::T / 64; ++j) tot += f[j];
        v = tot;                          // (the next transform's first barrier comes before its first write)
    }
    return v;
}

template <class X, bool ACC> __global__ __launch_bounds__(X::C::WG) void k_cwt(CwtArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 256, "power-of-two transforms of at least 256 points");
    constexpr int L = X::L;
    constexpr bool STASH = cwt_stash(L);
    const int64_t g = (int64_t)blockIdx.x * C::FPW + grp;
    // groups past the last frame repeat it and write nothing
    const bool act = g < a.nframes;
    const int64_t n0 = (act ? g : a.nframes - 1) * a.hop;              // the frame's first output sample
    const int row = blockIdx.z;
    const int s_lo = blockIdx.y * a.chunk, s_hi = s_lo + a.chunk < a.S ? s_lo + a.chunk : a.S;
    const int64_t N = a.nsig;
    cf *stash = STASH ? smem + C::FPW * C::LDS_PER + grp * L : nullptr;
    cf xs[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int64_t i = n0 - a.M + tid + C::T * t;
        const int64_t ic = i < 0 ? 0 : (i < N ? i : N - 1);
        const cf s = load_sample(a.x, (int64_t)row * a.x_ld + ic, a.cplx != 0);
        xs[t] = i == ic ? s : mk(0.f, 0.f);
    }
    fwd_row(xf, xs, lds, tid, n);
    if constexpr (STASH) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) stash[tid + C::T * t] = xs[t];
    }
    cf racc[ACC ? C::R : 1];
    float bacc[ACC ? C::R : 1];
    if constexpr (ACC) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            racc[t] = mk(0.f, 0.f);
            bacc[t] = 0.f;
        }
    }
    const float fp = a.p, fa = a.a, fb = a.b, u0 = a.u0;
    for (int s = s_lo; s < s_hi; ++s) {
        const float step = a.sc[2 * s], c = a.sc[2 * s + 1];
        // the thread's index, opaque to the compiler in every scale: what depends on it alone (the bins as floats, the masks, the
        // sample offsets) would otherwise be hoisted out of the scale loop and held in registers across the transform
        int tq = tid;
        asm volatile("" : "+v"(tq));
        cf v[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int k = tq + C::T * t;
            const float u = (float)k * step, d = fmaf((float)k, step, -u0);
            float e = fmaf(-fa * d, d, fmaf(-fb, d, c));
            if (fp != 0.f) e = fmaf(fp, __logf(u), e);
            const float h = (k >= 1 && k <= L / 2) ? __expf(e) : 0.f;
            cf z = xs[t];
            if constexpr (STASH) z = stash[k];
            v[t] = mk(h * z.x, -h * z.y);                              // the first conj of conj . forward . conj
        }
        fwd_row(xf, v, lds, tid, n);
        const float wr = ACC && a.wr != nullptr ? a.wr[s] : 0.f, wb = ACC && a.wb != nullptr ? a.wb[s] : 0.f;
        cf *__restrict__ Wrow = a.W != nullptr ? a.W + ((int64_t)row * a.S + s) * N : nullptr;
        float pw = 0.f;
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int j = tq + C::T * t;
            const int64_t nn = n0 - a.M + j;
            const bool ok = act && j >= a.M && j < a.M + a.hop && nn < N;
            const cf y = mk(v[t].x, -v[t].y);
            const float q = cnorm(y);
            pw += ok ? q : 0.f;
            if constexpr (ACC) {
                racc[t] = mk(fmaf(wr, y.x, racc[t].x), fmaf(wr, y.y, racc[t].y));
                bacc[t] = fmaf(wb, q, bacc[t]);
            }
            if (Wrow != nullptr && ok) st_stream(Wrow + nn, y);
        }
        if (a.gpart != nullptr) {
            pw = cwt_group_sum<C>(pw, lds, tid);
            if (tid == 0 && act) a.gpart[((int64_t)row * a.S + s) * a.nframes + g] = pw;
        }
    }
    if constexpr (ACC) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int j = tid + C::T * t;
            const int64_t nn = n0 - a.M + j;
            const bool ok = act && j >= a.M && j < a.M + a.hop && nn < N;
            if (a.recon != nullptr && ok) st_stream(a.recon + (int64_t)row * N + nn, racc[t]);
            if (a.bandpow != nullptr && ok) st_stream(a.bandpow + (int64_t)row * N + nn, bacc[t]);
        }
    }
}

// gws[r] = sum over the frames of gpart[r][g], r = (row, scale), in float64 and in a fixed order: thread j of the workgroup takes the
// frames j, j + 256, .. in ascending order, thread 0 adds the 256 sums in ascending order
static __global__ __launch_bounds__(256) void k_cwt_gws_finish(const float *__restrict__ gpart, int64_t nframes, double *__restrict__ gws) {
    __shared__ double part[256];
    const float *p = gpart + (int64_t)blockIdx.x * nframes;
    double s = 0.0;
    for (int64_t gq = threadIdx.x; gq < nframes; gq += 256) s += (double)p[gq];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int j = 0; j < 256; ++j) tot += part[j];
        gws[blockIdx.x] = tot;
    }
}

// out[row][n] = sum_s w[s] W[row][s][n], ascending s (the sum behind icwt)
static __global__ __launch_bounds__(256) void k_icwt(const cf *__restrict__ W, const float *__restrict__ w, int S, int64_t N,
                                                     cf *__restrict__ out) {
    const int64_t row = blockIdx.y;
    const cf *__restrict__ Wr = W + row * S * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        cf acc = mk(0.f, 0.f);
        for (int s = 0; s < S; ++s) {
            const cf y = ld_stream(Wr + (int64_t)s * N + i);
            const float ws = w[s];
            acc = mk(fmaf(ws, y.x, acc.x), fmaf(ws, y.y, acc.y));
        }
        st_stream(out + row * N + i, acc);
    }
}

int launch_cwt(LaunchCtx c, const CwtArgs &a, int L, const cf *tw, const CwtPlan &pl, int64_t rows) {
    const bool acc = a.recon != nullptr || a.bandpow != nullptr;
    if (a.nframes < 1 || a.S < 1 || a.chunk < 1 || a.M < 0 || a.hop != L - 2 * a.M || a.hop < 1 || rows < 1 || rows > 65535 ||
        pl.nchunks < 1 || pl.nchunks > 65535 || pl.blocks_x < 1 || pl.blocks_x > INT_MAX || (acc && a.chunk < a.S))
        return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
    const dim3 grid((unsigned)pl.blocks_x, (unsigned)pl.nchunks, (unsigned)rows);
#define L_(AC)                                                                                        \
    {                                                                                                 \
        if (lds_raise<k_cwt<XT, AC>>(lds)) return -1;                                                 \
        hipLaunchKernelGGL((k_cwt<XT, AC>), grid, dim3(XT::C::WG), lds, c.stream, a, tb);             \
    }
    return for_pow2<SP_CWT_MIN_L, SP_CWT_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        const size_t lds = cwt_lds_bytes<typename XT::C>(XT::L);
        if (acc) L_(true) else L_(false)
        return 0;
    });
#undef L_
}

int launch_cwt_gws_finish(LaunchCtx c, const float *gpart, int64_t rows_x_scales, int64_t nframes, double *gws) {
    if (rows_x_scales < 1 || rows_x_scales > INT_MAX || nframes < 1) return -1;
    hipLaunchKernelGGL(k_cwt_gws_finish, dim3((unsigned)rows_x_scales), dim3(256), 0, c.stream, gpart, nframes, gws);
    return 0;
}

int launch_icwt(LaunchCtx c, const cf *W, const float *w, int S, int64_t N, int64_t rows, cf *out) {
    if (S < 1 || N < 1 || rows < 1 || rows > 65535) return -1;
    int64_t bx = (N + 255) / 256;
    const int64_t cap = (int64_t)c.ncu * 16;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(k_icwt, dim3((unsigned)bx, (unsigned)rows), dim3(256), 0, c.stream, W, w, S, N, out);
    return 0;
}

}   // namespace sp
