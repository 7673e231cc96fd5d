// k_mtaper.hip -- Thomson multitaper spectra: k_welch with a taper loop inside the frame loop.
//   X_{g,k} = FFT(v_k (x[g hop : g hop + n] - trend)),  sums over the frames g and the tapers k of |X|^2, |Y|^2, Y conj(X)
// A transform group owns a run of consecutive units (frames, or pairs of frames), loads a unit's samples into registers ONCE,
// removes the trend, and for each taper multiplies, transforms and adds into fp32 register accumulators.  One partial per
// (taper block, group) goes to HBM in the layout of the Welch / CSD kernels, so that their float64 finish kernels (k_welch_finish,
// k_csd_rp_finish, k_csd_finish: a fixed order, no atomics) reduce it.  The weights sqrt(c_k) and 1 / sqrt(energy_k) are inside the
// taper table, so the sums over tapers are plain sums.
//
// Modes (what a unit is and what is accumulated):
//   MT_PSD, real input   : a unit is a PAIR of frames, z = v_k f_g + i v_k f_{g+1}; |Z|^2 is accumulated and symmetrised by
//                          k_welch_finish (sym), as k_welch_rp does.  K M / 2 transforms for any K -- two TAPERS of one frame in one
//                          transform would cost ceil(K / 2) M, a third more at K = 3 than K calls of the real-pair Welch kernel.
//   MT_PSD, complex input: a unit is a frame, one transform per taper.
//   MT_XRP  (real x and y, power-of-two n >= 32): z = v_k x + i v_k y, a = |Z|^2 and c = Z[k] Z[n - k] through one mirrored LDS
//                          read, separated into Pxx, Pyy, Pxy on the sums by k_csd_rp_finish (k_welch_csd_rp's algebra, linear in
//                          the sums, so it holds across tapers as it does across frames).
//   MT_XGEN (complex pairs, other lengths): one transform per taper per signal.  The unit's samples are NOT held: two raw frames, two
//                          transforms in flight and four accumulators do not fit in 256 VGPRs; the samples of the second and later
//                          tapers come from L1 / L2.
// grid.y = taper blocks of `ktap` tapers each: 1 block of K tapers for the weighted spectra; K blocks of one taper for the
// eigenspectra (one partial per (taper, group); the run's samples are read once per taper, from L2 after the first).
#include "launch.h"
namespace sp {

enum { MT_PSD = 0, MT_XRP = 1, MT_XGEN = 2 };

template <class X, int MODE, bool CPLX, bool LIN>
__global__ __launch_bounds__(X::C::WG) void k_mtaper(const void *__restrict__ x, const void *__restrict__ y,
                                                      const float *__restrict__ tapers, int ktap, int hop, int64_t nframes,
                                                      int64_t upg /*units per group*/, const float *__restrict__ trend /*x, y*/,
                                                      XfTables tb, float *__restrict__ partial, int64_t groups_total) {
    SP_KERNEL_PROLOGUE(X)
    constexpr bool PAIR = MODE == MT_PSD && !CPLX;
    constexpr int NP = MODE == MT_PSD ? 1 : (MODE == MT_XRP ? 3 : 4);
    static_assert(MODE != MT_XRP || (X::EXACT && !CPLX), "the x + i y form is for real records and power-of-two lengths");
    const float *__restrict__ tp = tapers + (int64_t)blockIdx.y * ktap * n;
    const Trend trx = load_trend(trend), try_ = load_trend(trend + 4);
    const float *xr = reinterpret_cast<const float *>(x), *yr = reinterpret_cast<const float *>(y);
    float a0[C::R], a1[C::R];
    cf cc[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        a0[t] = a1[t] = 0.f;
        cc[t] = mk(0.f, 0.f);
    }
    const int64_t nunits = PAIR ? (nframes + 1) / 2 : nframes;
    const int64_t gid = (int64_t)blockIdx.x * C::FPW + grp;
    const int64_t u0 = gid * upg;
    for (int64_t i = 0; i < upg; ++i) {
        const int64_t u = u0 + i;
        // units past the end are clamped to the last one and weighted 0: every load is unconditional and every barrier is met
        const float keep = u < nunits ? 1.f : 0.f;
        const int64_t uc = u < nunits ? u : nunits - 1;
        const int64_t base = (PAIR ? 2 * uc : uc) * hop;
        cf raw[C::R];
        if constexpr (PAIR) {
            const bool has_b = 2 * uc + 1 < nframes;          // a lone last frame: zero imaginary part
            const int64_t base_b = base + (has_b ? hop : 0);
            const float kb = has_b ? keep : 0.f;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tid + C::T * t;
                const int jj = (X::EXACT || j < n) ? j : n - 1;
                raw[t] = mk(xr[base + jj], xr[base_b + jj]);
            }
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tid + C::T * t;
                const cf a = detrended<LIN>(mk(raw[t].x, 0.f), trx, base + j);
                const cf b = detrended<LIN>(mk(raw[t].y, 0.f), trx, base_b + j);
                raw[t] = mk(keep * a.x, kb * b.x);
            }
        } else if constexpr (MODE == MT_XRP) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) raw[t] = mk(xr[base + tid + C::T * t], yr[base + tid + C::T * t]);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int64_t idx = base + tid + C::T * t;
                const cf a = detrended<LIN>(mk(raw[t].x, 0.f), trx, idx);
                const cf b = detrended<LIN>(mk(raw[t].y, 0.f), try_, idx);
                raw[t] = mk(keep * a.x, keep * b.x);
            }
        } else if constexpr (MODE == MT_PSD) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tid + C::T * t;
                raw[t] = load_sample(x, base + ((X::EXACT || j < n) ? j : n - 1), true);
            }
#pragma unroll
            for (int t = 0; t < C::R; ++t) raw[t] = keep * detrended<LIN>(raw[t], trx, base + tid + C::T * t);
        }
        for (int k = 0; k < ktap; ++k) {
            const float *__restrict__ wk = tp + (int64_t)k * n;
            float w[C::R];
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tid + C::T * t;
                const float wv = wk[(X::EXACT || j < n) ? j : 0];
                w[t] = (X::EXACT || j < n) ? wv : 0.f;
            }
            if constexpr (MODE == MT_XGEN) {
                cf vx[C::R], vy[C::R];
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int j = tid + C::T * t;
                    const int64_t idx = base + ((X::EXACT || j < n) ? j : n - 1);
                    vx[t] = load_sample(x, idx, CPLX);
                    vy[t] = load_sample(y, idx, CPLX);
                }
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int64_t idx = base + tid + C::T * t;
                    vx[t] = (keep * w[t]) * detrended<LIN>(vx[t], trx, idx);
                    vy[t] = (keep * w[t]) * detrended<LIN>(vy[t], try_, idx);
                }
                fwd_row(xf, vx, lds, tid, n);
                fwd_row(xf, vy, lds, tid, n);
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    a0[t] += cnorm(vx[t]);
                    a1[t] += cnorm(vy[t]);
                    cc[t] = cc[t] + cmulc(vy[t], vx[t]);          // Y conj(X)
                }
            } else {
                cf v[C::R];
#pragma unroll
                for (int t = 0; t < C::R; ++t) v[t] = w[t] * raw[t];
                fwd_row(xf, v, lds, tid, n);
                if constexpr (MODE == MT_XRP) {
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < C::R; ++t) lds[tid + C::T * t] = v[t];
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < C::R; ++t) {
                        const int kk = tid + C::T * t;
                        const cf zm = lds[(X::L - kk) & (X::L - 1)];
                        a0[t] += cnorm(v[t]);
                        cc[t] = cc[t] + cmul(v[t], zm);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < C::R; ++t) a0[t] += cnorm(v[t]);
                }
            }
        }
    }
    float *p = partial + ((int64_t)blockIdx.y * groups_total + gid) * NP * X::L;
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int kk = tid + C::T * t;
        p[kk] = a0[t];
        if constexpr (MODE == MT_XRP) {
            p[X::L + kk] = cc[t].x;
            p[2 * X::L + kk] = cc[t].y;
        } else if constexpr (MODE == MT_XGEN) {
            p[X::L + kk] = a1[t];
            p[2 * X::L + kk] = cc[t].x;
            p[3 * X::L + kk] = cc[t].y;
        }
    }
}

// out[b] = sum_k c[k] sk[k][b], b < nb, float64, tapers in order: the weighted spectra from the eigenspectra
struct MtWeights {
    double c[SP_MTAPER_MAXK];
};
static __global__ __launch_bounds__(256) void k_mtaper_combine(const double *__restrict__ sk, int K, int64_t nb, MtWeights wt,
                                                               double *__restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += wt.c[k] * sk[(int64_t)k * nb + b];
    out[b] = s;
}

bool mtaper_xrp_eligible(const Xf &xf, bool cplx) { return !cplx && !xf.blue && xf.L >= 32; }
int mtaper_partial_planes(const Xf &xf, bool cplx, bool cross) { return !cross ? 1 : (mtaper_xrp_eligible(xf, cplx) ? 3 : 4); }

int launch_mtaper(LaunchCtx c, const void *x, const void *y, bool cplx, const float *tapers, int nblocks, int ktap, int hop,
                  int64_t nframes, const float *trend, bool lin, const Xf &xf, float *partial, const RunPart &rp) {
#define L_(XT, MODE, CP, LN)                                                                          \
    hipLaunchKernelGGL((k_mtaper<XT, MODE, CP, LN>), dim3(rp.blocks, nblocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, y, \
                       tapers, ktap, hop, nframes, rp.fpg, trend, xf.tb, partial, rp.groups)
#define LL_(XT, MODE, CP)                                                                             \
    if (lin) L_(XT, MODE, CP, true);                                                                  \
    else L_(XT, MODE, CP, false);
    if (y == nullptr) {
#define M_(XT)                                                                                        \
    if (cplx) { LL_(XT, MT_PSD, true) } else { LL_(XT, MT_PSD, false) }
        SP_DISPATCH_X(xf, M_)
#undef M_
    } else if (mtaper_xrp_eligible(xf, cplx)) {
#define M_(XT)                                                                                        \
    if constexpr (XT::L >= 32) { LL_(XT, MT_XRP, false) } else { return -1; }
        SP_DISPATCH_P(xf, M_)
#undef M_
    } else {
#define M_(XT)                                                                                        \
    if (cplx) { LL_(XT, MT_XGEN, true) } else { LL_(XT, MT_XGEN, false) }
        SP_DISPATCH_X(xf, M_)
#undef M_
    }
#undef LL_
#undef L_
    return 0;
}

int launch_mtaper_combine(LaunchCtx c, const double *sk, int K, int64_t nb, const double *weights, double *out) {
    if (K < 1 || K > SP_MTAPER_MAXK) return -1;
    MtWeights wt;
    for (int k = 0; k < SP_MTAPER_MAXK; ++k) wt.c[k] = k < K ? weights[k] : 0.0;
    hipLaunchKernelGGL(k_mtaper_combine, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c.stream, sk, K, nb, wt, out);
    return 0;
}

}   // namespace sp
