// k_skf.hip -- two-point wavenumber-frequency spectrum S(k, f) (Beall, Kim & Powers 1982): the local wavenumber of every frame and
// bin, theta = arg(X conj Y) = k dx, histogrammed with the frame's power as the weight.
//   a = win (x[g hop : g hop + L] - mean),  b likewise from y,  X = FFT_L(a),  Y = FFT_L(b)
//   j = floor((theta / 2 pi + 1/2) nk) mod nk,   p = (|X|^2 + |Y|^2) / 2  or  |X| |Y|,   S[f][j] += p
// Modelled on k_xcorr_frames: frames are never materialised, frames past the end are clamped to the last one so that every load is
// unconditional and every barrier is met (they are transformed and then left out of the histogram).  A workgroup owns a run of
// consecutive frames and one frequency tile of the band; a round deals FPW frames of the run to its FPW transform groups.
// Real records: z = a + i b, ONE transform; with P = Z[k] and zm = Z[L - k] (Q = conj(zm), the mirrored read of k_xcorr_frames)
//   X conj Y = Im(P zm) / 2 + i (|P|^2 - |zm|^2) / 4,   (|X|^2 + |Y|^2) / 2 = (|P|^2 + |zm|^2) / 4.
// Complex records: two transforms, the first spectrum parked in a second image.
// The histogram is a scatter, and the project has no float atomics on memory and bitwise-reproducible results.  Both are met by
// ownership: once every group has left its spectrum in its image (natural order), one barrier, then thread t of the WORKGROUP walks
// bins t, t + WG, .. of the tile and for each goes through the round's frames in frame order.  A cell hist[j][bin] has exactly one
// writer and its additions a fixed order (rounds ascending, frames ascending), whatever the tiling.  The addition is an LDS float add
// without return (nothing waits for it; operations of one wave on one address stay in order).
// Banks: an LDS add is banked by dword address mod 32 in two groups of 32 lanes.  Rows are `stride` floats, a multiple of 32, so the
// bank of hist[j * stride + bin] is bin mod 32: the 32 consecutive bins of a lane group never meet, however j scatters.
// At the end the tile goes out as one float32 partial [run][nk][nb] (phase-major like the tile: LDS read and store both unit stride);
// k_skf_finish sums the runs in float64 in ascending order and transposes to s_out[nb][nk].
#include "launch.h"
namespace sp {

// phase -> histogram row: nk equal bins over [-pi, pi), pi wraps to row 0; always inside 0 .. nk - 1 (a NaN phase lands in row 0)
__device__ __forceinline__ int skf_row(float re, float im, int nk) {
    const float th = atan2f(im, re);
    int j = (int)floorf((th * 0.15915494309189535f + 0.5f) * (float)nk);
    j = j >= nk ? j - nk : j;
    return j < 0 ? 0 : (j > nk - 1 ? nk - 1 : j);
}

template <class X, bool CPLX>
__global__ __launch_bounds__(X::C::WG) void k_skf(SkfArgs a, XfTables tb, float *__restrict__ partial) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= SP_SKF_MAX_L, "power-of-two transforms of 32 .. 4096 points");
    constexpr int L = X::L;
    const float *__restrict__ xr = reinterpret_cast<const float *>(a.x), *__restrict__ yr = reinterpret_cast<const float *>(a.y);
    const cf *__restrict__ xc = reinterpret_cast<const cf *>(a.x), *__restrict__ yc = reinterpret_cast<const cf *>(a.y);
    const float *__restrict__ win = a.win;
    cf *park = smem + (C::FPW + grp) * C::LDS_PER;                       // complex records: this group's X while Y is made
    float *hist = reinterpret_cast<float *>(smem + (CPLX ? 2 : 1) * C::FPW * C::LDS_PER);
    const int wt = (int)threadIdx.x, nk = a.nk, stride = a.stride;
    const int t0 = (int)blockIdx.y * a.tile_bins;                        // first bin of this tile within the band
    const int tbins = a.nb - t0 < a.tile_bins ? a.nb - t0 : a.tile_bins;
    for (int e = wt; e < nk * stride; e += C::WG) hist[e] = 0.f;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * a.fpr;
    const int64_t r1 = r0 + a.fpr < a.nframes ? r0 + a.fpr : a.nframes;  // the run's frames: r0 .. r1 - 1
    for (int64_t f0 = r0; f0 < r1; f0 += C::FPW) {
        const int64_t g = f0 + grp;
        // frames past the end of the run are clamped to the record's last one: every load is unconditional and every barrier is met
        const int64_t base = (g < r1 ? g : a.nframes - 1) * a.hop;
        // the thread's index, opaque to the compiler in every round (as in k_xcorr_frames: the taper and the offsets are not hoisted)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        auto taper = [&](int j) __attribute__((always_inline)) { return win != nullptr ? win[j] : 1.f; };
        auto frame_mean = [&](const cf (&r)[C::R]) __attribute__((always_inline)) {
            cf sm = mk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < C::R; ++t) sm = sm + r[t];
            return (1.f / (float)L) * group_image_sum<C>(sm, lds, tq);
        };
        cf v[C::R];
        if constexpr (!CPLX) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int64_t idx = base + tq + C::T * t;
                v[t] = mk(xr[idx], yr[idx]);
            }
            if (a.segmean) {
                const cf m = frame_mean(v);
#pragma unroll
                for (int t = 0; t < C::R; ++t) v[t] = v[t] - m;
            }
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = taper(tq + C::T * t) * v[t];
        } else {
            auto prep = [&](const cf *__restrict__ src, cf (&r)[C::R]) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) r[t] = src[base + tq + C::T * t];
                if (a.segmean) {
                    const cf m = frame_mean(r);
#pragma unroll
                    for (int t = 0; t < C::R; ++t) r[t] = r[t] - m;
                }
#pragma unroll
                for (int t = 0; t < C::R; ++t) r[t] = taper(tq + C::T * t) * r[t];
            };
            prep(xc, v);
            fwd_row(xf, v, lds, tid, n);
            // X waits in the second image, in natural order; nobody reads it before the barrier in front of the binning
#pragma unroll
            for (int t = 0; t < C::R; ++t) park[tq + C::T * t] = v[t];
            prep(yc, v);
        }
        fwd_row(xf, v, lds, tid, n);
        __syncthreads();                  // the image may still be read by the transform
#pragma unroll
        for (int t = 0; t < C::R; ++t) lds[tq + C::T * t] = v[t];
        __syncthreads();                  // every group's spectrum is in its image
        // binning: ownership by workgroup thread, frames in frame order
        const int nact = r1 - f0 < C::FPW ? (int)(r1 - f0) : C::FPW;
        for (int b = wt; b < tbins; b += C::WG) {
            int kk = a.b0 + t0 + b;
            if constexpr (CPLX) kk &= L - 1;
            float *col = hist + b;
            for (int q = 0; q < nact; ++q) {
                const cf *img = smem + q * C::LDS_PER;
                float re, im, pw;
                if constexpr (!CPLX) {
                    const cf p = img[kk], zm = img[(L - kk) & (L - 1)];
                    const float np = cnorm(p), nz = cnorm(zm);
                    re = 0.5f * (p.x * zm.y + p.y * zm.x);
                    im = 0.25f * (np - nz);
                    pw = a.cross ? sqrtf(re * re + im * im) : 0.25f * (np + nz);
                } else {
                    const cf xs = img[C::FPW * C::LDS_PER + kk], ys = img[kk];
                    const cf s = cmulc(xs, ys);
                    re = s.x;
                    im = s.y;
                    pw = a.cross ? sqrtf(cnorm(xs) * cnorm(ys)) : 0.5f * (cnorm(xs) + cnorm(ys));
                }
                const int j = skf_row(re, im, nk);
                __hip_atomic_fetch_add(col + j * stride, pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();                  // the images are free for the next round
    }
    // the tile -> partial[run][j][t0 + b]
    float *out = partial + (int64_t)blockIdx.x * nk * a.nb + t0;
    for (int e = wt; e < nk * tbins; e += C::WG) {
        const int j = e / tbins, b = e - j * tbins;
        out[(int64_t)j * a.nb + b] = hist[j * stride + b];
    }
}

// s_out[f][j] = mult * sum over the runs of partial[r][j][f], in float64 and in a fixed order: a workgroup owns 32 consecutive bins
// of one phase row, its 8 slices take the runs s, s + 8, .. in ascending order, and the slices are added in ascending order
#define SKF_FIN_E 32
#define SKF_FIN_S 8
static __global__ __launch_bounds__(SKF_FIN_E * SKF_FIN_S) void k_skf_finish(const float *__restrict__ partial, int64_t runs, int nb,
                                                                              int nk, double mult, double *__restrict__ s_out) {
    __shared__ double part[SKF_FIN_S][SKF_FIN_E];
    const int ex = threadIdx.x % SKF_FIN_E, sl = threadIdx.x / SKF_FIN_E;
    const int f = blockIdx.x * SKF_FIN_E + ex, j = blockIdx.y;
    double s = 0.0;
    if (f < nb) {
        const int64_t row = (int64_t)nk * nb;
        for (int64_t r = sl; r < runs; r += SKF_FIN_S) s += (double)partial[r * row + (int64_t)j * nb + f];
    }
    part[sl][ex] = s;
    __syncthreads();
    if (sl == 0 && f < nb) {
        double tot = 0.0;
        for (int q = 0; q < SKF_FIN_S; ++q) tot += part[q][ex];
        s_out[(int64_t)f * nk + j] = tot * mult;
    }
}

int launch_skf(LaunchCtx c, const SkfArgs &a, bool cplx, int L, const cf *tw, int64_t runs, const SkfPlan &pl, float *partial) {
    if (a.nframes < 1 || a.fpr < 1 || !runs_cover(a.nframes, a.fpr, runs)) return -1;
    if (a.nk < 2 || a.nk > SP_SKF_MAX_NK || !band_in_transform(cplx, L, a.b0, a.nb)) return -1;
    if (pl.tiles < 1 || pl.tiles > 65535 || a.tile_bins != pl.tile_bins || a.stride != pl.stride || pl.tile_bins < 1 ||
        pl.stride < pl.tile_bins || (int64_t)pl.tiles * pl.tile_bins < a.nb || (int64_t)(pl.tiles - 1) * pl.tile_bins >= a.nb ||
        pl.lds_bytes > SP_LDS_MAX || pl.lds_bytes != skf_image_bytes(cplx, L) + sizeof(float) * (size_t)a.nk * (size_t)pl.stride)
        return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(CP)                                                                                        \
    {                                                                                                 \
        if (lds_raise<k_skf<XT, CP>>(pl.lds_bytes)) return -1;                                        \
        hipLaunchKernelGGL((k_skf<XT, CP>), dim3((unsigned)runs, (unsigned)pl.tiles), dim3(XT::C::WG), pl.lds_bytes, c.stream, a, tb, partial); \
    }
    return for_pow2<32, SP_SKF_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (cplx) L_(true) else L_(false)
        return 0;
    });
#undef L_
}

int launch_skf_finish(LaunchCtx c, const float *partial, int64_t runs, int nb, int nk, double mult, double *s_out) {
    if (runs < 1 || nb < 1 || nk < 1 || nk > 65535) return -1;
    hipLaunchKernelGGL(k_skf_finish, dim3((unsigned)((nb + SKF_FIN_E - 1) / SKF_FIN_E), (unsigned)nk), dim3(SKF_FIN_E * SKF_FIN_S), 0,
                       c.stream, partial, runs, nb, nk, mult, s_out);
    return 0;
}

}   // namespace sp
