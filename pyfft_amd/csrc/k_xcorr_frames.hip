// k_xcorr_frames.hip -- short-time cross-correlation: the lags of every frame pair, their average over the frames, and the peak track.
//   a = win (x[g hop : g hop + nw] - mean),  b likewise from y,  zero-padded to L >= nw + maxlag
//   S = FFT_L(a) conj(FFT_L(b));  S' = W S  (x 1 / E for the coefficient form)  or  W S / (|S| + beta E);  E = sqrt(sum |a|^2 sum |b|^2)
//   c = IFFT_L(S');  the lags -maxlag .. maxlag are c[l mod L]: c[l] = sum_n a[n + l] conj(b[n])
// Modelled on k_zoom: a transform group owns a run of consecutive frames (never materialised); frames past the end are clamped to the
// last one and weighted 0, so that every load is unconditional and every barrier is met.  Nothing but the lags is written:
//   frames  the 2 maxlag + 1 lags of every frame, non-temporal stores;
//   partial the group's sum over its run, fp32 registers -> one row of L per group, summed in float64 in a fixed order by
//           k_xcorr_frames_finish (no atomics);
//   peak    (l* + delta, height) per frame: the parabola through the top three lags, 8 bytes per frame.
// Which of the three is wanted is a uniform run-time branch: one instantiation per (L, real / complex).
// Real records: z = a + i b, ONE forward transform; with P = Z[k] and Q = conj(Z[L - k]) (one mirrored LDS read, as MT_XRP: unit
// stride downwards, conflict-free like the upward write), A = (P + Q) / 2 and B = (P - Q) / 2i give
//   Re S = Im(P conj Q) / 2,  Im S = (|P|^2 - |Q|^2) / 4.
// Complex records: two forward transforms.  The inverse is conj . forward . conj, as XfCzt::fwd.
// The window mean, the two energies and the peak's argmax are reductions over the T = L / 16 threads of a group; at L <= 512 several
// groups share a wave, so they go through the group's own exchange image (as group_mean), never across the wave.
#include "launch.h"
#include <type_traits>
namespace sp {

// LDS plan.  Complex records from 2048 points: the first spectrum is parked in a second image (the stash) while the second is made -- 32
// registers that cost a wave per SIMD at 2048 and spill at 8192.  At L = 8192 a workgroup is 512 threads, so a wave has 256 registers
// and no AGPRs, and a complex frame, 16 complex accumulators and the transform's constants still do not fit: the first XCF_NLA
// accumulators of every thread live in what is left of the 160 KiB (the stash loses its row padding for it), updated by their owner
// alone like the stash -- no barrier, no atomics, the same sums in the same order.
constexpr bool xcf_stash(bool cplx, int L) { return cplx && L >= 2048; }
constexpr int xcf_nla(bool cplx, int L) { return cplx && L == 8192 ? 7 : 0; }
template <class C> constexpr size_t xcf_lds_bytes(bool cplx, int L) {
    return xcf_nla(cplx, L) > 0 ? sizeof(cf) * ((size_t)C::LDS_PER + L + (size_t)xcf_nla(cplx, L) * C::T)
                                : C::lds_bytes(xcf_stash(cplx, L) ? 2 : 1);
}

// (height, lag) candidates of the peak search: the higher wins, the smaller lag on a tie
__device__ __forceinline__ cf xc_better(cf a, cf b) { return (b.x > a.x || (b.x == a.x && b.y < a.y)) ? b : a; }

template <class X, bool CPLX>
__global__ __launch_bounds__(X::C::WG) void k_xcorr_frames(XcfArgs a, int64_t fpg, XfTables tb, void *__restrict__ frames_,
                                                            void *__restrict__ partial_, float *__restrict__ peak) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32, "power-of-two transforms of at least 32 points");
    constexpr int L = X::L;
    using Lag = typename std::conditional<CPLX, cf, float>::type;
    const float *__restrict__ xr = reinterpret_cast<const float *>(a.x), *__restrict__ yr = reinterpret_cast<const float *>(a.y);
    const cf *__restrict__ xc = reinterpret_cast<const cf *>(a.x), *__restrict__ yc = reinterpret_cast<const cf *>(a.y);
    const float *__restrict__ weight = a.weight;
    Lag *__restrict__ frames = reinterpret_cast<Lag *>(frames_);
    const int nw = a.nw, maxlag = a.maxlag, nl = 2 * maxlag + 1;
    const float beta = a.beta, invL = 1.f / (float)L;
    const float *__restrict__ win = a.win;
    // where element j of the inverse transform goes among the 2 maxlag + 1 lags, or -1
    auto slot_of = [&](int j) __attribute__((always_inline)) { return j <= maxlag ? j + maxlag : (j >= L - maxlag ? j - L + maxlag : -1); };
    // the taper at sample j, 0 in the padding; read again for every frame (the table stays in L1): 16 registers less than keeping it.
    // (The uniform branch per element is deliberate, here and at the weights: with the 16 loads in one block the compiler keeps them
    // all in flight and complex L = 8192 spills 29 registers.)
    auto taper = [&](int j) __attribute__((always_inline)) {
        const float wv = win != nullptr ? win[j < nw ? j : 0] : 1.f;
        return j < nw ? wv : 0.f;
    };
    constexpr bool STASH = xcf_stash(CPLX, L);
    constexpr int NLA = xcf_nla(CPLX, L);             // accumulators t < NLA live in LDS (FPW = 1 there)
    static_assert(NLA == 0 || C::FPW == 1, "the LDS accumulators are laid out for one group per workgroup");
    cf *stash = STASH ? smem + (NLA > 0 ? C::LDS_PER : (C::FPW + grp) * C::LDS_PER) : nullptr;
    Lag *accl = reinterpret_cast<Lag *>(smem + C::LDS_PER + L);
    Lag acc[C::R - NLA];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        Lag zero;
        if constexpr (CPLX) zero = mk(0.f, 0.f);
        else zero = 0.f;
        if (t < NLA) accl[t * C::T + tid] = zero;
        else acc[t - NLA] = zero;
    }
    const int64_t gid = (int64_t)blockIdx.x * C::FPW + grp;
    const int64_t g0 = gid * fpg;
    for (int64_t i = 0; i < fpg; ++i) {
        const int64_t g = g0 + i;
        // frames past the end are clamped to the last one and weighted 0: every load is unconditional and every barrier is met
        const bool act = g < a.nframes;
        const float keep = act ? 1.f : 0.f;
        const int64_t base = (act ? g : a.nframes - 1) * a.hop;
        // the thread's index, opaque to the compiler in every frame: what depends on it alone (the taper, the weights, the lag slots, the
        // clamped sample offsets, the masks of the mean: some 80 values) would otherwise be hoisted out of the frame loop and held in
        // registers across the transforms.  The transforms themselves keep tid: their constants are meant to stay.
        int tq = tid;
        asm volatile("" : "+v"(tq));
        // the mean of the nw samples of a frame (the padding's slots hold a clamped sample: left out)
        auto frame_mean = [&](const cf (&r)[C::R]) __attribute__((always_inline)) {
            cf sm = mk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < C::R; ++t) sm = sm + (tq + C::T * t < nw ? 1.f : 0.f) * r[t];
            return (1.f / (float)nw) * group_image_sum<C>(sm, lds, tq);
        };
        cf v[C::R];                       // real records: (a, b) packed; complex: a, then the cross spectrum
        float E;
        if constexpr (!CPLX) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tq + C::T * t;
                const int64_t idx = base + (j < nw ? j : nw - 1);
                v[t] = mk(xr[idx], yr[idx]);
            }
            if (a.segmean) {
                const cf m = frame_mean(v);
#pragma unroll
                for (int t = 0; t < C::R; ++t) v[t] = v[t] - m;
            }
            cf e = mk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                v[t] = taper(tq + C::T * t) * v[t];
                e = e + mk(v[t].x * v[t].x, v[t].y * v[t].y);
            }
            e = group_image_sum<C>(e, lds, tq);
            E = sqrtf(e.x) * sqrtf(e.y);
            fwd_row(xf, v, lds, tid, n);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < C::R; ++t) lds[tq + C::T * t] = v[t];
            __syncthreads();
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int kk = tq + C::T * t;
                const cf p = v[t], zm = lds[(L - kk) & (L - 1)];          // Q = conj(zm)
                v[t] = mk(0.5f * (p.x * zm.y + p.y * zm.x), 0.25f * (cnorm(p) - cnorm(zm)));
            }
        } else {
            // one record's frame: loaded, its own mean removed, tapered; -> this thread's share of its energy
            auto prep = [&](const cf *__restrict__ src, cf (&r)[C::R]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int j = tq + C::T * t;
                    r[t] = src[base + (j < nw ? j : nw - 1)];
                }
                if (a.segmean) {
                    const cf m = frame_mean(r);
#pragma unroll
                    for (int t = 0; t < C::R; ++t) r[t] = r[t] - m;
                }
                float e = 0.f;
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    r[t] = taper(tq + C::T * t) * r[t];
                    e += cnorm(r[t]);
                }
                return e;
            };
            const float ex = prep(xc, v);
            fwd_row(xf, v, lds, tid, n);
            if constexpr (STASH) {
                // A waits in LDS while B is made: a thread reads back only what it wrote itself, so no barrier
#pragma unroll
                for (int t = 0; t < C::R; ++t) stash[tq + C::T * t] = v[t];
            }
            cf u[C::R];
            const float ey = prep(yc, u);
            const cf e = group_image_sum<C>(mk(ex, ey), lds, tq);
            E = sqrtf(e.x) * sqrtf(e.y);
            fwd_row(xf, u, lds, tid, n);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                cf av = v[t];
                if constexpr (STASH) av = stash[tq + C::T * t];
                v[t] = cmulc(av, u[t]);                                    // A conj(B)
            }
        }
        // the weighting, the 1 / L of the inverse, and the first conj of conj . forward . conj
        const float flat = (a.coeff ? (E > 0.f ? 1.f / E : 0.f) : 1.f) * invL;
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const float wk = weight != nullptr ? weight[tq + C::T * t] : 1.f;
            float s = wk * flat;
            if (beta > 0.f) {
                const float den = sqrtf(cnorm(v[t])) + beta * E;
                s = den > 0.f ? wk * invL / den : 0.f;
            }
            v[t] = mk(s * v[t].x, -s * v[t].y);
        }
        fwd_row(xf, v, lds, tid, n);
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            Lag c;
            if constexpr (CPLX) c = mk(v[t].x, -v[t].y);
            else c = v[t].x;
            if (t < NLA) accl[t * C::T + tq] = accl[t * C::T + tq] + keep * c;
            else acc[t - NLA] = acc[t - NLA] + keep * c;
            const int o = slot_of(tq + C::T * t);
            if (frames != nullptr && act && o >= 0) st_stream(frames + g * nl + o, c);
        }
        if (peak != nullptr) {
            // q over the lags: an image of L floats in the first half of the exchange image, the candidates behind it
            float *qimg = reinterpret_cast<float *>(lds);
            cf *cand = lds + L / 2;
            cf best = mk(-INFINITY, 1e9f);
            __syncthreads();              // the image may still be read by the inverse transform
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const float q = CPLX ? sqrtf(cnorm(v[t])) : v[t].x;
                qimg[tq + C::T * t] = q;
                const int o = slot_of(tq + C::T * t);
                if (o >= 0) best = xc_better(best, mk(q, (float)(o - maxlag)));
            }
            cand[tq] = best;
            __syncthreads();
            constexpr int W = C::T < 16 ? C::T : 16;
            if (tq < W) {
                for (int j = tq + W; j < C::T; j += W) best = xc_better(best, cand[j]);
            }
            __syncthreads();
            if (tq < W) cand[tq] = best;
            __syncthreads();
            if (tq == 0 && act) {
#pragma unroll
                for (int j = 1; j < W; ++j) best = xc_better(best, cand[j]);
                const int l = (int)best.y;
                float pos = best.y, top = best.x;
                if (l > -maxlag && l < maxlag) {
                    const float qm = qimg[(l - 1) & (L - 1)], qp = qimg[(l + 1) & (L - 1)];
                    const float d = qm - 2.f * top + qp;
                    if (d < 0.f) {
                        const float delta = 0.5f * (qm - qp) / d;
                        pos += delta;
                        top -= 0.25f * (qm - qp) * delta;
                    }
                }
                st_stream(reinterpret_cast<cf *>(peak) + g, mk(pos, top));
            }
        }
    }
    if (partial_ != nullptr) {
        Lag *p = reinterpret_cast<Lag *>(partial_) + gid * L;
#pragma unroll
        for (int t = 0; t < C::R; ++t) p[tid + C::T * t] = t < NLA ? accl[t * C::T + tid] : acc[t < NLA ? 0 : t - NLA];
    }
}

// avg[o] = (1 / nframes) sum over the G groups of partial[g][(o - maxlag) mod L], o < 2 maxlag + 1 (re and im for complex records), in
// float64 and in a fixed order: a workgroup owns 16 consecutive output floats, its 64 slices take the groups s, s + 64, .. in
// ascending order, and the slices are added in ascending order.  (One thread per output walking all the groups one after the other
// took 0.6 ms for 257 lags over 2048 groups, half as long again as the main kernel's 1.1 ms.)
#define XCF_FIN_E 16
#define XCF_FIN_S 64
static __global__ __launch_bounds__(XCF_FIN_E * XCF_FIN_S) void k_xcorr_frames_finish(const float *__restrict__ partial, int ncomp,
                                                                                       int64_t G, int L, int maxlag, double inv,
                                                                                       double *__restrict__ avg) {
    __shared__ double part[XCF_FIN_S][XCF_FIN_E];
    const int ex = threadIdx.x % XCF_FIN_E, sl = threadIdx.x / XCF_FIN_E;
    const int e = blockIdx.x * XCF_FIN_E + ex, total = (2 * maxlag + 1) * ncomp;
    double s = 0.0;
    if (e < total) {
        const int o = e / ncomp, c = e - o * ncomp;
        const int64_t i = (int64_t)((o - maxlag) & (L - 1)) * ncomp + c, row = (int64_t)L * ncomp;
        for (int64_t gq = sl; gq < G; gq += XCF_FIN_S) s += (double)partial[gq * row + i];
    }
    part[sl][ex] = s;
    __syncthreads();
    if (sl == 0 && e < total) {
        double tot = 0.0;
        for (int j = 0; j < XCF_FIN_S; ++j) tot += part[j][ex];
        avg[e] = tot * inv;
    }
}

int launch_xcorr_frames(LaunchCtx c, const XcfArgs &a, bool cplx, int L, const cf *tw, const RunPart &rp, void *frames, void *partial,
                        float *peak) {
    if (a.nframes < 1 || a.nw < 2 || a.maxlag < 0 || a.maxlag > a.nw - 1 || (int64_t)a.nw + a.maxlag > L) return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(CP)                                                                                        \
    {                                                                                                 \
        const size_t lds = xcf_lds_bytes<typename XT::C>(CP, XT::L);                                  \
        if (lds_raise<k_xcorr_frames<XT, CP>>(lds)) return -1;                                        \
        hipLaunchKernelGGL((k_xcorr_frames<XT, CP>), dim3(rp.blocks), dim3(XT::C::WG), lds, c.stream, a, rp.fpg, tb, frames, partial, peak); \
    }
    return for_pow2<32, 8192>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (cplx) L_(true) else L_(false)
        return 0;
    });
#undef L_
}

int launch_xcorr_frames_finish(LaunchCtx c, const void *partial, bool cplx, int64_t G, int L, int maxlag, int64_t nframes, double *avg) {
    if (G < 1 || nframes < 1 || maxlag < 0 || 2 * maxlag + 1 > L) return -1;
    const int ncomp = cplx ? 2 : 1, total = (2 * maxlag + 1) * ncomp;
    hipLaunchKernelGGL(k_xcorr_frames_finish, dim3((unsigned)((total + XCF_FIN_E - 1) / XCF_FIN_E)), dim3(XCF_FIN_E * XCF_FIN_S), 0,
                       c.stream, (const float *)partial, ncomp, G, L, maxlag, 1.0 / (double)nframes, avg);
    return 0;
}

}   // namespace sp
