// k_ssq.hip -- the synchrosqueezed STFT and the reassignment operators of its cells (Auger & Flandrin 1995; Daubechies, Lu & Wu 2011;
// Thakur & Wu 2011).  Frame g of a row is the L samples from first + g hop on, zero outside the row; with h, dh = dh/dj and
// th = (j - L/2) h the three windows,
//   X_h, X_d, X_t = FFT_L(h x), FFT_L(dh x), FFT_L(th x)
//   khat = k - (L / 2 pi) Im(X_d conj X_h) / |X_h|^2          the instantaneous frequency of cell (g, k), in bins
//   that = Re(X_t conj X_h) / |X_h|^2                         its group delay, in samples from the frame's centre
//   used = |X_h| > max(gamma, rel max_k |X_h|),   Xc = (-1)^k X_h   (the phase referred to the frame's centre)
//   MODE 0:  T[g][m] = sum over the used k with rint(khat) = m of Xc,  P[g][m] likewise of |X_h|^2,  IF = khat, GD = that
//   MODE 1:  out[b][g] = scale * sum over the used k with lo[b][g] <= khat < hi[b][g] of Xc      (modes without forming T)
// Modelled on k_skf: frames are never materialised, a workgroup owns a run of consecutive frames of one row, a round deals FPW frames
// to its FPW transform groups, and frames past the end of the run are clamped so that every barrier is met.  The frame's samples are
// read once and kept in registers across its transforms.
// Real records: z = h x + i dh x, ONE transform; with P = Z[k] and zm = Z[L - k]:  X_h = (P + conj zm) / 2,  X_d = (P - conj zm) / 2i.
// The fields add one transform, of th x.  Complex records: two transforms, three with the fields.  Every transform has an image of
// its own and leaves its spectrum there in natural order; after one barrier thread t of the GROUP walks the bins t, t + T, ..
// Sums.  Many source bins land in one target bin (for a clean tone all of them), so no ownership order exists.  The sums are made
// independent of the order instead: with e the binary exponent of the frame's largest |Re X_h| or |Im X_h|, every used coefficient
// is scaled by 2^(48 - e) (exact), rounded to a 64-bit integer and added into the group's accumulator in LDS with an integer atomic
// add without return.  Integer addition commutes: the result is the exact sum of the coefficients as rounded to 2^-48 of the
// frame's largest, rounded once to float32 on the way out, the same bits for any lane order and any partition into runs.  8192 terms below 2^49 stay below 2^62.  P does the
// same with one integer per bin and the exponent of the largest |X_h|^2.
// Reductions over a group (the frame's largest cell, a band's sum, the frame's mean) are an xor butterfly inside the wave -- float
// addition commutes, so every lane ends with the same bits -- and, where a group spans several waves, the waves' values through the
// 16 spare elements behind an image's spectrum, combined in ascending order.
#include <type_traits>
#include "launch.h"
namespace sp {

enum { SSQ_SUM = 0, SSQ_MAX = 1 };

// over the T threads of a transform group; every lane gets the same bits.  slots: 8 elements of LDS nobody else uses meanwhile (groups
// of more than one wave only, where every thread of the workgroup must call it: barriers)
template <class C, int OP> __device__ __forceinline__ cf ssq_group_reduce(cf s, cf *slots, int tid) {
    constexpr int W = C::T < 64 ? C::T : 64;
    auto op = [](cf p, cf q) __attribute__((always_inline)) {
        if constexpr (OP == SSQ_MAX) return mk(fmaxf(p.x, q.x), fmaxf(p.y, q.y));
        else return p + q;
    };
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) s = op(s, mk(__shfl_xor(s.x, o), __shfl_xor(s.y, o)));
    if constexpr (C::T > 64) {
        if ((tid & 63) == 0) slots[tid >> 6] = s;
        __syncthreads();
        cf tot = slots[0];
#pragma unroll
        for (int j = 1; j < C::T / 64; ++j) tot = op(tot, slots[j]);
        __syncthreads();                  // the slots are free again
        s = tot;
    }
    return s;
}

// the binary exponent of a positive float (-127 for a subnormal)
__device__ __forceinline__ int ssq_exponent(float v) { return ((__float_as_int(v) >> 23) & 0xff) - 127; }
__device__ __forceinline__ unsigned long long ssq_fixed(float v, int sh) { return (unsigned long long)__float2ll_rn(ldexpf(v, sh)); }
// one rounding: int64 -> float to nearest, then an exact power of two
__device__ __forceinline__ float ssq_float(long long v, int sh) { return ldexpf(__ll2float_rn(v), sh); }

template <class X, bool CPLX, int MODE>
__global__ __launch_bounds__(X::C::WG) void k_ssq(SsqArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= SP_SSQ_MAX_L, "power-of-two transforms of 32 .. 8192 points");
    constexpr int L = X::L, NSRC = CPLX ? L : L / 2 + 1;
    using S = std::conditional_t<CPLX, cf, float>;
    const bool fields = MODE == 0 && a.th != nullptr;                    // uniform over the grid
    const int nimg = (CPLX ? 2 : 1) + (fields ? 1 : 0);
    cf *img0 = smem + (size_t)grp * nimg * C::LDS_PER, *img1 = img0 + C::LDS_PER, *imgt = img0 + (nimg - 1) * C::LDS_PER;
    (void)lds;
    const bool wantT = MODE == 0 && a.T != nullptr, wantP = MODE == 0 && a.P != nullptr;
    const int nb = a.nb, per = (wantT ? 2 * nb : 0) + (wantP ? nb : 0);
    long long *acc = reinterpret_cast<long long *>(smem + (size_t)C::FPW * nimg * C::LDS_PER) + (size_t)grp * per;
    long long *accP = acc + (wantT ? 2 * nb : 0);
    const S *__restrict__ xrow = reinterpret_cast<const S *>(a.x) + (int64_t)blockIdx.y * a.x_ld;
    const float *__restrict__ wh = a.h, *__restrict__ wd = a.dh, *__restrict__ wt = a.th;
    if constexpr (MODE == 0) {
        for (int j = tid; j < per; j += C::T) acc[j] = 0;
        __syncthreads();
    }
    const float c1 = (float)L * 0.15915494309189535f;
    const int64_t r0 = (int64_t)blockIdx.x * a.fpr;
    const int64_t r1 = r0 + a.fpr < a.nframes ? r0 + a.fpr : a.nframes;  // the run's frames: r0 .. r1 - 1
    for (int64_t f0 = r0; f0 < r1; f0 += C::FPW) {
        const int64_t g = f0 + grp;
        const bool act = g < r1;
        // frames past the end of the run are clamped to the row's last one: every barrier is met
        const int64_t gc = act ? g : a.nframes - 1;
        const int64_t base = a.first + gc * a.hop;
        int tq = tid;                     // opaque in every round (as in k_skf: the windows and the offsets are not hoisted)
        asm volatile("" : "+v"(tq));
        S xs[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int64_t idx = base + tq + C::T * t;
            const bool in = idx >= 0 && idx < a.nsig;                    // zeros outside the row
            S z{};
            if (in) z = xrow[idx];
            xs[t] = z;
        }
        if (a.segmean) {
            cf sm = mk(0.f, 0.f);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                if constexpr (CPLX) sm = sm + xs[t];
                else sm.x += xs[t];
            }
            const cf m = (1.f / (float)L) * ssq_group_reduce<C, SSQ_SUM>(sm, img0, tid);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                if constexpr (CPLX) xs[t] = xs[t] - m;
                else xs[t] -= m.x;
            }
        }
        cf v[C::R];
        auto park = [&](cf *img) __attribute__((always_inline)) {
            fwd_row(xf, v, img, tid, n);
            __syncthreads();              // the image may still be read by the transform
#pragma unroll
            for (int t = 0; t < C::R; ++t) img[tq + C::T * t] = v[t];
        };
        if constexpr (!CPLX) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = mk(wh[tq + C::T * t] * xs[t], wd[tq + C::T * t] * xs[t]);
            park(img0);
            if (fields) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) v[t] = mk(wt[tq + C::T * t] * xs[t], 0.f);
                park(imgt);
            }
        } else {
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = wh[tq + C::T * t] * xs[t];
            park(img0);
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = wd[tq + C::T * t] * xs[t];
            park(img1);
            if (fields) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) v[t] = wt[tq + C::T * t] * xs[t];
                park(imgt);
            }
        }
        __syncthreads();                  // the group's spectra are in their images
        auto spec = [&](int k, cf &xh, cf &xd) __attribute__((always_inline)) {
            if constexpr (!CPLX) {
                const cf p = img0[k], zm = img0[(L - k) & (L - 1)];
                xh = mk(0.5f * (p.x + zm.x), 0.5f * (p.y - zm.y));
                xd = mk(0.5f * (p.y + zm.y), 0.5f * (zm.x - p.x));
            } else {
                xh = img0[k];
                xd = img1[k];
            }
        };
        // the frame's largest |X_h|^2 and largest component
        cf mx = mk(0.f, 0.f);
        for (int k = tq; k < NSRC; k += C::T) {
            cf xh, xd;
            spec(k, xh, xd);
            mx.x = fmaxf(mx.x, cnorm(xh));
            mx.y = fmaxf(mx.y, fmaxf(fabsf(xh.x), fabsf(xh.y)));
        }
        mx = ssq_group_reduce<C, SSQ_MAX>(mx, img0 + L, tid);
        const float thr = fmaxf(a.gamma, a.rel * sqrtf(mx.x));
        if constexpr (MODE == 0) {
            const int shT = 48 - ssq_exponent(mx.y), shP = 48 - ssq_exponent(mx.x);
            const int64_t orow = ((int64_t)blockIdx.y * a.nframes + gc) * nb;
            if (act) {
                for (int k = tq; k < NSRC; k += C::T) {
                    cf xh, xd;
                    spec(k, xh, xd);
                    const float np = cnorm(xh);
                    const bool used = sqrtf(np) > thr;
                    const float kh = (float)k - c1 * ((xd.y * xh.x - xd.x * xh.y) / np);
                    int jb = k - a.b0;
                    if constexpr (CPLX) jb &= L - 1;
                    if (fields && (unsigned)jb < (unsigned)nb) {
                        const cf xt = imgt[k];
                        if (a.IF) st_stream(a.IF + orow + jb, used ? kh : __builtin_nanf(""));
                        if (a.GD) st_stream(a.GD + orow + jb, used ? (xt.x * xh.x + xt.y * xh.y) / np : __builtin_nanf(""));
                    }
                    if (used && per > 0) {
                        const float mf = rintf(kh);
                        const bool ok = CPLX ? fabsf(mf) < 1073741824.f : (mf >= 0.f && mf <= (float)(L / 2));
                        int jt = (ok ? (int)mf : 0) - a.b0;
                        if constexpr (CPLX) jt &= L - 1;
                        if (ok && (unsigned)jt < (unsigned)nb) {
                            if (wantT) {
                                const float sg = (k & 1) ? -1.f : 1.f;
                                atomicAdd(reinterpret_cast<unsigned long long *>(acc + jt), ssq_fixed(sg * xh.x, shT));
                                atomicAdd(reinterpret_cast<unsigned long long *>(acc + nb + jt), ssq_fixed(sg * xh.y, shT));
                            }
                            if (wantP) atomicAdd(reinterpret_cast<unsigned long long *>(accP + jt), ssq_fixed(np, shP));
                        }
                    }
                }
            }
            __syncthreads();              // the group's sums are complete
            if (act) {
                for (int j = tq; j < nb; j += C::T) {
                    if (wantT) {
                        st_stream(a.T + orow + j, mk(ssq_float(acc[j], -shT), ssq_float(acc[nb + j], -shT)));
                        acc[j] = 0;
                        acc[nb + j] = 0;
                    }
                    if (wantP) {
                        st_stream(a.P + orow + j, ssq_float(accP[j], -shP));
                        accP[j] = 0;
                    }
                }
            }
        } else {
            cf bs[SP_SSQ_MAX_BANDS];
            float lo[SP_SSQ_MAX_BANDS], hi[SP_SSQ_MAX_BANDS];
#pragma unroll
            for (int b = 0; b < SP_SSQ_MAX_BANDS; ++b) {
                bs[b] = mk(0.f, 0.f);
                lo[b] = 1.f;
                hi[b] = 0.f;              // an empty band
                if (b < a.nbands) {
                    if (a.per_frame) {
                        const float *e = a.edges + ((int64_t)b * a.nframes + gc) * 2;
                        lo[b] = e[0];
                        hi[b] = e[1];
                    } else {
                        lo[b] = a.edges_c.v[2 * b];
                        hi[b] = a.edges_c.v[2 * b + 1];
                    }
                }
            }
            for (int k = tq; k < NSRC; k += C::T) {
                cf xh, xd;
                spec(k, xh, xd);
                const float np = cnorm(xh);
                const bool used = sqrtf(np) > thr;
                const float kh = (float)k - c1 * ((xd.y * xh.x - xd.x * xh.y) / np);
                const float sg = (k & 1) ? -1.f : 1.f;
#pragma unroll
                for (int b = 0; b < SP_SSQ_MAX_BANDS; ++b)
                    if (used && kh >= lo[b] && kh < hi[b]) bs[b] = bs[b] + sg * xh;
            }
#pragma unroll
            for (int b = 0; b < SP_SSQ_MAX_BANDS; ++b) {
                if (b < a.nbands) {
                    const cf s = ssq_group_reduce<C, SSQ_SUM>(bs[b], img0 + L, tid);
                    if (act && tq == 0) a.out[((int64_t)blockIdx.y * a.nbands + b) * a.nframes + g] = a.scale * s;
                }
            }
        }
        __syncthreads();                  // the images and the accumulator are free for the next round
    }
}

// out[row][b][g] = scale * sum over lo <= m < hi of w_m T[row][g][j], m = (b0 + j) mod n the absolute bin of column j (w = 1/2 at the
// bins 0 and n / 2 when `half`): a wave per frame, lane l takes the bins l, l + 64, .. in ascending order, then the xor butterfly
#define SSQ_SUM_FRAMES 4
static __global__ __launch_bounds__(64 * SSQ_SUM_FRAMES) void k_ssq_sum(const cf *__restrict__ T, int64_t nframes, int nb, int n, int b0,
                                                                        int nbands, int per_frame, const float *__restrict__ edges,
                                                                        SsqEdges ec, int half, float scale, cf *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * SSQ_SUM_FRAMES + (threadIdx.x >> 6);
    if (g >= nframes) return;
    const cf *t = T + ((int64_t)blockIdx.y * nframes + g) * nb;
    for (int b = 0; b < nbands; ++b) {
        float lo = ec.v[2 * b], hi = ec.v[2 * b + 1];
        if (per_frame) {
            const float *e = edges + ((int64_t)b * nframes + g) * 2;
            lo = e[0];
            hi = e[1];
        }
        cf s = mk(0.f, 0.f);
        for (int j = lane; j < nb; j += 64) {
            const int m = (b0 + j) & (n - 1);
            if ((float)m >= lo && (float)m < hi) s = s + ((half && (m == 0 || m == n / 2)) ? 0.5f : 1.f) * t[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = s + mk(__shfl_xor(s.x, o), __shfl_xor(s.y, o));
        if (lane == 0) out[((int64_t)blockIdx.y * nbands + b) * nframes + g] = scale * s;
    }
}

int launch_ssq(LaunchCtx c, const SsqArgs &a, bool cplx, int L, const cf *tw, int64_t runs, int64_t rows, size_t lds_bytes) {
    const bool bands = a.out != nullptr;
    if (a.nframes < 1 || a.fpr < 1 || !runs_cover(a.nframes, a.fpr, runs)) return -1;
    if (rows < 1 || rows > 65535 || a.hop < 1 || a.nsig < 1 || a.x_ld < a.nsig || !a.x || !a.h || !a.dh) return -1;
    if (bands) {
        if (a.nbands < 1 || a.nbands > SP_SSQ_MAX_BANDS || (a.per_frame && !a.edges) || a.T || a.P || a.IF || a.GD || a.th) return -1;
    } else {
        if (!a.T && !a.P && !a.IF && !a.GD) return -1;
        if ((a.IF || a.GD) && !a.th) return -1;
        if (!band_in_transform(cplx, L, a.b0, a.nb)) return -1;
    }
    const bool fields = !bands && a.th != nullptr;
    if (lds_bytes > SP_LDS_MAX || lds_bytes != ssq_lds_bytes(cplx, L, bands ? 0 : a.nb, a.T != nullptr, a.P != nullptr, fields)) return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(CP, MD)                                                                                    \
    {                                                                                                 \
        if (lds_raise<k_ssq<XT, CP, MD>>(lds_bytes)) return -1;                                       \
        hipLaunchKernelGGL((k_ssq<XT, CP, MD>), dim3((unsigned)runs, (unsigned)rows), dim3(XT::C::WG), lds_bytes, c.stream, a, tb); \
    }
    return for_pow2<32, SP_SSQ_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (cplx) {
            if (bands) L_(true, 1) else L_(true, 0)
        } else {
            if (bands) L_(false, 1) else L_(false, 0)
        }
        return 0;
    });
#undef L_
}

int launch_ssq_sum(LaunchCtx c, const cf *T, int64_t nframes, int nb, int n, int b0, int nbands, int per_frame, const float *edges,
                   const SsqEdges &ec, int half, float scale, int64_t rows, cf *out) {
    const int64_t blocks = (nframes + SSQ_SUM_FRAMES - 1) / SSQ_SUM_FRAMES;
    if (nframes < 1 || blocks > 0x7fffffff || nb < 1 || nbands < 1 || rows < 1 || rows > 65535 || !T || (per_frame && !edges) || !out) return -1;
    hipLaunchKernelGGL(k_ssq_sum, dim3((unsigned)blocks, (unsigned)rows), dim3(64 * SSQ_SUM_FRAMES), 0, c.stream, T, nframes, nb, n, b0,
                       nbands, per_frame, edges, ec, half, scale, out);
    return 0;
}

}   // namespace sp
