// k_czt.hip -- chirp-z transform on an arc of the unit circle, and the zoom spectra built on it.
//   X[k] = sum_{j<n} x[j] e(-(start + k step) j),  k < m,  e(t) = exp(2 pi i t); start, step in cycles per sample
// Bluestein split, jk = (j^2 + k^2 - (k - j)^2) / 2:
//   pre[j]  = e(-start j - step j^2 / 2), j < n;   post[k] = e(-step k^2 / 2), k < m;
//   kern[i] = e(+step i^2 / 2), i in [-(n-1), m-1], wrapped into L >= n + m - 1 points;   bf = FFT_L(kern) / L
//   X[k]    = post[k] IFFT_L(FFT_L(x pre) . FFT_L(kern))[k]
// XfCzt<L> is XfBlue<L> with the contour freed: n inputs in, m outputs out, both L-point transforms in one workgroup.
//
//   k_czt_rows   batched rows (float32 or complex64, row stride x_ld) -> [batch][m] complex64, row-mapped like k_fft_c2c.
//   k_zoom       the Welch / STFT form, modelled on k_welch / k_mtaper: a transform group owns a run of consecutive frames of the
//                signal (never materialised), removes the whole-record trend, applies the window and runs XfCzt.
//                  ZM_PSD   |X|^2 accumulated in fp32 registers, one partial per group in k_welch_finish's layout;
//                  ZM_PAIR  |X|^2, |Y|^2, Y conj(X) of two records, partials in k_csd_finish's layout (4 planes);
//                  ZM_STFT  m bins per frame streamed out with non-temporal stores.
//                In the two accumulating modes the post-multiply is dropped: |post[k]| = 1, and it cancels in all three
//                products.  Frames past the end are clamped to the last one and weighted 0: every load is unconditional and
//                every barrier is met.  No atomics; the float64 finish kernels sum the partials in a fixed order.
//                The real-pair tricks of k_welch_rp / MT_XRP do NOT carry over: they separate two real signals through the
//                mirror bin Z[L - k], and the mirror of a bin of a zoom arc (frequency -(start + k step)) is not on the arc.
//                A real frame costs one transform (two L-point passes) per signal.
//   k_czt_pre / k_czt_post / k_zoom_acc   the elementwise ends of the multi-pass form (n + m - 1 beyond one workgroup transform),
//                composed by spectral.hip around dev_fft_big_pow2 and launch_cmul_vec as dev_fft_any composes Bluestein.
#include "launch.h"
namespace sp {

template <int L_> struct XfCzt {
    static constexpr int L = L_;
    static constexpr bool EXACT = false;
    using C = WgCfg<L_>;
    WgFft<L_> f;
    const cf *pre, *post, *bf;
    int m;
    __device__ __forceinline__ void init(const CztTables &tb, int tid) {
        f.load_twiddles(tb.tw, tid);
        pre = tb.pre;
        post = tb.post;
        bf = tb.bf;
        m = tb.m;
    }
    // register contract of XfBlue::fwd: v[t] <-> element tid + T t; valid for indices < n on entry and < m on exit.
    // POST = false leaves out the unit-modulus post-multiply.
    template <bool POST> __device__ __forceinline__ void fwd(cf (&v)[C::R], cf *lds, int tid, int n) const {
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int i = tid + C::T * t;
            const cf c = pre[i < n ? i : 0];
            v[t] = i < n ? cmul(v[t], c) : mk(0.f, 0.f);
        }
        f.template run<true>(v, lds, lds, tid);
#pragma unroll
        for (int t = 0; t < C::R; ++t) v[t] = cconj(cmul(v[t], bf[tid + C::T * t]));     // conj: inverse via forward
        f.template run<true>(v, lds, lds, tid);
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            if constexpr (POST) {
                const int k = tid + C::T * t;
                v[t] = cmul(cconj(v[t]), post[k < m ? k : 0]);
            } else {
                v[t] = cconj(v[t]);
            }
        }
    }
};

template <class X, bool CPLX>
__global__ __launch_bounds__(X::C::WG) void k_czt_rows(const void *__restrict__ x, int64_t x_ld, int64_t batch, CztTables tb,
                                                        cf *__restrict__ out) {
    SP_KERNEL_PROLOGUE(X)
    const int m = tb.m;
    const int64_t stride = (int64_t)gridDim.x * C::FPW;
    for (int64_t b0 = (int64_t)blockIdx.x * C::FPW; b0 < batch; b0 += stride) {
        const int64_t b = b0 + grp;
        const bool act = b < batch;
        const int64_t bl = act ? b : batch - 1;          // clamped: loads stay unconditional
        cf v[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int i = tid + C::T * t;
            v[t] = load_sample(x, bl * x_ld + (i < n ? i : n - 1), CPLX);
        }
        xf.template fwd<true>(v, lds, tid, n);
        if (act) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int k = tid + C::T * t;
                if (k < m) st_stream(out + b * m + k, v[t]);
            }
        }
    }
}

enum { ZM_PSD = 0, ZM_PAIR = 1, ZM_STFT = 2 };

template <class X, int MODE, bool CPLX, bool LIN>
__global__ __launch_bounds__(X::C::WG) void k_zoom(const void *__restrict__ x, const void *__restrict__ y,
                                                    const float *__restrict__ win, int hop, int64_t nframes, int64_t fpg,
                                                    const float *__restrict__ trend /*x, y*/, CztTables tb, float amp,
                                                    float *__restrict__ partial, cf *__restrict__ frames) {
    SP_KERNEL_PROLOGUE(X)
    const int m = tb.m;
    float w[C::R], a0[C::R], a1[C::R];
    cf cc[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int j = tid + C::T * t;
        const float wv = win[j < n ? j : 0];
        w[t] = j < n ? wv : 0.f;
        a0[t] = a1[t] = 0.f;
        cc[t] = mk(0.f, 0.f);
    }
    const Trend trx = load_trend(trend), try_ = load_trend(trend + 4);
    const int64_t gid = (int64_t)blockIdx.x * C::FPW + grp;
    const int64_t g0 = gid * fpg;
    for (int64_t i = 0; i < fpg; ++i) {
        const int64_t g = g0 + i;
        // frames past the end are clamped to the last one and weighted 0: every load is unconditional and every barrier is met
        const bool act = g < nframes;
        const float keep = act ? 1.f : 0.f;
        const int64_t base = (act ? g : nframes - 1) * hop;
        cf vx[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int j = tid + C::T * t;
            vx[t] = load_sample(x, base + (j < n ? j : n - 1), CPLX);
        }
#pragma unroll
        for (int t = 0; t < C::R; ++t) vx[t] = (keep * w[t]) * detrended<LIN>(vx[t], trx, base + tid + C::T * t);
        if constexpr (MODE == ZM_PAIR) {
            cf vy[C::R];
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tid + C::T * t;
                vy[t] = load_sample(y, base + (j < n ? j : n - 1), CPLX);
            }
#pragma unroll
            for (int t = 0; t < C::R; ++t) vy[t] = (keep * w[t]) * detrended<LIN>(vy[t], try_, base + tid + C::T * t);
            xf.template fwd<false>(vx, lds, tid, n);
            xf.template fwd<false>(vy, lds, tid, n);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                a0[t] += cnorm(vx[t]);
                a1[t] += cnorm(vy[t]);
                cc[t] = cc[t] + cmulc(vy[t], vx[t]);          // Y conj(X)
            }
        } else if constexpr (MODE == ZM_PSD) {
            xf.template fwd<false>(vx, lds, tid, n);
#pragma unroll
            for (int t = 0; t < C::R; ++t) a0[t] += cnorm(vx[t]);
        } else {
            xf.template fwd<true>(vx, lds, tid, n);
            if (act) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int k = tid + C::T * t;
                    if (k < m) st_stream(frames + g * m + k, amp * vx[t]);
                }
            }
        }
    }
    if constexpr (MODE == ZM_PSD) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) partial[gid * X::L + tid + C::T * t] = a0[t];
    } else if constexpr (MODE == ZM_PAIR) {
        float *p = partial + gid * 4 * X::L;
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int kk = tid + C::T * t;
            p[kk] = a0[t];
            p[X::L + kk] = a1[t];
            p[2 * X::L + kk] = cc[t].x;
            p[3 * X::L + kk] = cc[t].y;
        }
    }
}

// ---- the multi-pass form ------------------------------------------------------------------------------------------
// A[b][i] = i < n ? src(b, i) pre[i] : 0, i < L; blockIdx.y = b.  win == null: src = row b of x (row stride ld, batched czt);
// otherwise src = win[i] * (frame f0 + b of the signal x, hop ld, minus the whole-record trend).
template <bool CPLX>
static __global__ __launch_bounds__(256) void k_czt_pre(const void *__restrict__ x, int64_t ld, int64_t f0,
                                                         const float *__restrict__ win, const float *__restrict__ trend, int lin,
                                                         const cf *__restrict__ pre, int64_t n, int64_t L, cf *__restrict__ A) {
    const int64_t base = (f0 + blockIdx.y) * ld;
    cf *row = A + (int64_t)blockIdx.y * L;
    cf tm = mk(0.f, 0.f), ts = mk(0.f, 0.f);
    if (win != nullptr) {
        tm = mk(trend[0], trend[1]);
        ts = mk(trend[2], trend[3]);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        if (i < n) {
            cf v = load_sample(x, base + i, CPLX);
            if (win != nullptr) {
                if (lin) {
                    const float fi = (float)(base + i);
                    v = mk(v.x - (tm.x + ts.x * fi), v.y - (tm.y + ts.y * fi));
                } else {
                    v = v - tm;
                }
                v = win[i] * v;
            }
            row[i] = cmul(v, pre[i]);
        } else {
            row[i] = mk(0.f, 0.f);
        }
    }
}
// out[(f0 + b) m + k] = amp A[b][k] post[k], k < m
static __global__ __launch_bounds__(256) void k_czt_post(const cf *__restrict__ A, int64_t L, const cf *__restrict__ post, int64_t m,
                                                          float amp, int64_t f0, cf *__restrict__ out) {
    const cf *row = A + (int64_t)blockIdx.y * L;
    cf *o = out + (f0 + blockIdx.y) * m;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < m; k += (int64_t)gridDim.x * 256)
        st_stream(o + k, amp * cmul(row[k], post[k]));
}
// acc[0][k] += sum_b |Sx[b][k]|^2 and, with Sy, acc[1][k] += |Sy|^2, acc[2][k], acc[3][k] += Re, Im of Sy conj(Sx); k < m, rows L
// apart, float64, rows in order: deterministic
static __global__ __launch_bounds__(256) void k_zoom_acc(const cf *__restrict__ Sx, const cf *__restrict__ Sy, int64_t rows, int64_t L,
                                                          int64_t m, double *__restrict__ acc) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    double axx = acc[k];
    if (Sy == nullptr) {
        for (int64_t b = 0; b < rows; ++b) axx += (double)cnorm(Sx[b * L + k]);
        acc[k] = axx;
        return;
    }
    double ayy = acc[m + k], cr = acc[2 * m + k], ci = acc[3 * m + k];
    for (int64_t b = 0; b < rows; ++b) {
        const cf X = Sx[b * L + k], Y = Sy[b * L + k];
        axx += (double)cnorm(X);
        ayy += (double)cnorm(Y);
        cr += (double)Y.x * (double)X.x + (double)Y.y * (double)X.y;
        ci += (double)Y.y * (double)X.x - (double)Y.x * (double)X.y;
    }
    acc[k] = axx;
    acc[m + k] = ayy;
    acc[2 * m + k] = cr;
    acc[3 * m + k] = ci;
}
// pxx[k] = scale acc[0][k]; with pyy: pyy[k] = scale acc[1][k], pxy[k] = scale (acc[2][k], acc[3][k])
static __global__ __launch_bounds__(256) void k_zoom_acc_out(const double *__restrict__ acc, int64_t m, double scale,
                                                              double *__restrict__ pxx, double *__restrict__ pyy,
                                                              double *__restrict__ pxy) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    pxx[k] = scale * acc[k];
    if (pyy != nullptr) {
        pyy[k] = scale * acc[m + k];
        pxy[2 * k] = scale * acc[2 * m + k];
        pxy[2 * k + 1] = scale * acc[3 * m + k];
    }
}

#define SP_CASE_Z(Lv, MACRO) case Lv: { MACRO(XfCzt<Lv>) } break;
#define SP_DISPATCH_Z(Lval, MACRO)                                                                    \
    switch (Lval) {                                                                                   \
        SP_CASE_Z(512, MACRO) SP_CASE_Z(1024, MACRO) SP_CASE_Z(2048, MACRO) SP_CASE_Z(4096, MACRO)    \
        SP_CASE_Z(8192, MACRO)                                                                        \
        default: return -1;                                                                           \
    }

int launch_czt_rows(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t batch, int L, const CztTables &tb, cf *out) {
    if (batch < 1 || tb.n < 1 || tb.m < 1 || (int64_t)tb.n + tb.m - 1 > L) return -1;
    const int blocks = strided_blocks(L, batch, c.ncu);
#define M_(XT)                                                                                        \
    if (cplx) hipLaunchKernelGGL((k_czt_rows<XT, true>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, x_ld, batch, tb, out); \
    else hipLaunchKernelGGL((k_czt_rows<XT, false>), dim3(blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, x_ld, batch, tb, out);
    SP_DISPATCH_Z(L, M_)
#undef M_
    return 0;
}

int launch_zoom(LaunchCtx c, const void *x, const void *y, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                bool lin, int L, const CztTables &tb, const RunPart &rp, float amp, float *partial, cf *frames) {
    if (nframes < 1 || tb.n < 1 || tb.m < 1 || (int64_t)tb.n + tb.m - 1 > L) return -1;
#define L_(XT, MODE, CP, LN)                                                                          \
    hipLaunchKernelGGL((k_zoom<XT, MODE, CP, LN>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, y, win, hop, \
                       nframes, rp.fpg, trend, tb, amp, partial, frames)
#define LL_(XT, MODE)                                                                                 \
    if (cplx) {                                                                                       \
        if (lin) L_(XT, MODE, true, true);                                                            \
        else L_(XT, MODE, true, false);                                                               \
    } else {                                                                                          \
        if (lin) L_(XT, MODE, false, true);                                                           \
        else L_(XT, MODE, false, false);                                                              \
    }
    if (frames != nullptr) {
#define M_(XT) LL_(XT, ZM_STFT)
        SP_DISPATCH_Z(L, M_)
#undef M_
    } else if (y != nullptr) {
#define M_(XT) LL_(XT, ZM_PAIR)
        SP_DISPATCH_Z(L, M_)
#undef M_
    } else {
#define M_(XT) LL_(XT, ZM_PSD)
        SP_DISPATCH_Z(L, M_)
#undef M_
    }
#undef LL_
#undef L_
    return 0;
}

static unsigned row_blocks(int64_t len, int64_t rows, int ncu) {
    // enough workgroups along the row to fill the chip when there are few rows
    int64_t bx = (len + 255) / 256;
    const int64_t want = ((int64_t)ncu * 8 + rows - 1) / rows;
    if (bx > want) bx = want < 1 ? 1 : want;
    return (unsigned)(bx < 1 ? 1 : bx);
}
int launch_czt_pre(LaunchCtx c, const void *x, bool cplx, int64_t ld, int64_t f0, int64_t rows, const float *win, const float *trend,
                   bool lin, const cf *pre, int64_t n, int64_t L, cf *A) {
    if (rows < 1 || rows > 65535 || n > L) return -1;
    const dim3 grid(row_blocks(L, rows, c.ncu), (unsigned)rows);
    if (cplx) hipLaunchKernelGGL((k_czt_pre<true>), grid, dim3(256), 0, c.stream, x, ld, f0, win, trend, lin ? 1 : 0, pre, n, L, A);
    else hipLaunchKernelGGL((k_czt_pre<false>), grid, dim3(256), 0, c.stream, x, ld, f0, win, trend, lin ? 1 : 0, pre, n, L, A);
    return 0;
}
int launch_czt_post(LaunchCtx c, const cf *A, int64_t L, int64_t rows, const cf *post, int64_t m, float amp, int64_t f0, cf *out) {
    if (rows < 1 || rows > 65535 || m > L) return -1;
    hipLaunchKernelGGL(k_czt_post, dim3(row_blocks(m, rows, c.ncu), (unsigned)rows), dim3(256), 0, c.stream, A, L, post, m, amp, f0, out);
    return 0;
}
int launch_zoom_acc(LaunchCtx c, const cf *Sx, const cf *Sy, int64_t rows, int64_t L, int64_t m, double *acc) {
    if (rows < 1 || m > L) return -1;
    hipLaunchKernelGGL(k_zoom_acc, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c.stream, Sx, Sy, rows, L, m, acc);
    return 0;
}
int launch_zoom_acc_out(LaunchCtx c, const double *acc, int64_t m, double scale, double *pxx, double *pyy, double *pxy) {
    hipLaunchKernelGGL(k_zoom_acc_out, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c.stream, acc, m, scale, pxx, pyy, pxy);
    return 0;
}

}   // namespace sp
