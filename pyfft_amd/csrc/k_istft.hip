// k_istft.hip -- inverse STFT: inverse transforms of consecutive frames overlap-added into one output stream
#include "launch.h"
#include <type_traits>
namespace sp {

// y[a] = rcp[a] * sum_g wsc[a - g hop] * ifft(Z_g)[a - g hop],  wsc = win * scale / n  (spectral.h, sp_istft).
//
// A transform group (T threads, SP_KERNEL_PROLOGUE) owns the run of frames [g0, g1) and the output span [g0 hop, g1 hop) of it.  It
// keeps an n-entry accumulator ring in LDS behind the exchange images: ring slot (r0 + j) mod n holds output sample g hop + j while
// frame g is the newest one added.  Per frame: conj, forward transform, conj (the inverse), add wsc * x into the ring, barrier,
// stream out the `hop` samples no later frame reaches times the reciprocal envelope, clear them, advance r0 by hop, barrier.
// To make its span complete the run first transforms the `halo` >= ceil(n/hop) - 1 frames before g0 and only accumulates them.
// The run that ends at the last frame also writes the tail [M hop, L).  No atomics, no scratch: every output sample is summed by
// one group in frame order, whatever the partition, so the result does not depend on the run length and repeats bit for bit.
//
// MODE 0: two-sided spectra [n] (fftfreq order) -> complex output.
// MODE 1: one-sided spectra [n/2 + 1] -> real output, one frame per transform (any length).
// MODE 2: the same, two frames per transform (power-of-two n >= 32): V = A + iB with both Hermitian-extended, frame g comes out as
//         the real part and frame g + 1 as the imaginary part -- the mirror of k_stft_rp.  g0, halo and fpg are even.
// The imaginary parts of bin 0 and (even n) bin n/2 of a one-sided spectrum are ignored, as irfft does.
//
// rcp = [period: hop][head: head_len][tail: n - hop, or none when head_len covers the whole output]: the reciprocal envelope is
// periodic with period hop except in the first and last n - hop samples (sp_istft builds the three pieces).
// Z holds the frames zbase .. (frame-major, nb bins each); blockIdx.y = channel: Z += y * z_cs, out += y * nout.
template <class X, int MODE>
__global__ __launch_bounds__(X::C::WG) void k_istft(const cf *__restrict__ Z, int64_t z_cs, int64_t zbase, int64_t M, int64_t fbeg,
                                                     int64_t fend, int64_t fpg, int halo, const float *__restrict__ win, float wscale,
                                                     int hop, XfTables tb, const float *__restrict__ rcp, int64_t head_len,
                                                     int64_t skip, int64_t nout, void *__restrict__ yout, int emit_tail) {
    SP_KERNEL_PROLOGUE(X)
    using E = std::conditional_t<MODE == 0, cf, float>;
    constexpr int FR = MODE == 2 ? 2 : 1;
    const int nr = (n + 3) & ~3;
    E *ring = reinterpret_cast<E *>(smem + C::FPW * C::LDS_PER) + grp * nr;
    // the scaled window stays in registers for the power-of-two transforms; the chirp-z forms, which hold a second set of
    // constants, re-read it per frame (cache-resident) instead of spilling
    constexpr bool WREG = X::EXACT;
    float w[WREG ? C::R : 1];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int i = tid + C::T * t;
        if constexpr (WREG) w[t] = win[i] * wscale;
        if (X::EXACT || i < n) ring[i] = E{};
    }
    __syncthreads();
    Z += (int64_t)blockIdx.y * z_cs;
    E *y = reinterpret_cast<E *>(yout) + (int64_t)blockIdx.y * nout;
    const int nh = n / 2, nb = MODE == 0 ? n : nh + 1;
    const float *period = rcp, *head = rcp + hop, *tail = head + head_len;
    const int64_t gid = (int64_t)blockIdx.x * C::FPW + grp;
    const int64_t g0 = fbeg + gid * fpg;
    const int64_t g1 = g0 + fpg < fend ? g0 + fpg : fend;          // g1 <= g0: a group past the end (it only keeps the barriers)
    const int64_t steps = (fpg + halo) / FR;
    int r0 = 0;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t ga = g0 - halo + it * FR;
        bool act[FR];
#pragma unroll
        for (int f = 0; f < FR; ++f) act[f] = ga + f >= 0 && ga + f < g1;
        cf v[C::R];
        if (act[0] || act[FR - 1]) {
            const cf *za = Z + (ga - zbase) * nb;
            if constexpr (MODE == 0) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int k = tid + C::T * t;
                    v[t] = cconj(ld_stream(za + ((X::EXACT || k < n) ? k : 0)));
                }
            } else {
                const cf *zb = za + (act[FR - 1] ? (FR - 1) * nb : 0);
                if (!act[0]) za = zb;
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int k = tid + C::T * t;
                    const bool low = k <= nh;
                    const int idx = (X::EXACT || k < n) ? (low ? k : n - k) : 0;
                    const bool edge = k == 0 || 2 * k == n;
                    cf a = ld_stream(za + idx);
                    a.y = edge ? 0.f : (low ? -a.y : a.y);                    // conj of the Hermitian extension
                    if constexpr (MODE == 2) {
                        cf b = ld_stream(zb + idx);
                        b.y = edge ? 0.f : (low ? -b.y : b.y);
                        if (!act[0]) a = mk(0.f, 0.f);
                        if (!act[1]) b = mk(0.f, 0.f);
                        v[t] = mk(a.x + b.y, a.y - b.x);                      // conj(A) - i conj(B) = conj(A + iB)
                    } else {
                        v[t] = a;
                    }
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = mk(0.f, 0.f);
        }
        fwd_row(xf, v, lds, tid, n);                                          // v = n conj(ifft(V))
#pragma unroll
        for (int f = 0; f < FR; ++f) {
            const int64_t g = ga + f;
            if (act[f]) {
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int j = tid + C::T * t;
                    if (!X::EXACT && j >= n) continue;
                    int p = r0 + j;
                    p = p >= n ? p - n : p;
                    float wj;
                    if constexpr (WREG) wj = w[t];
                    else wj = win[j] * wscale;
                    if constexpr (MODE == 0) {
                        const cf s = ring[p];
                        ring[p] = mk(s.x + wj * v[t].x, s.y - wj * v[t].y);
                    } else {
                        ring[p] += wj * (f == 0 ? v[t].x : -v[t].y);
                    }
                }
            }
            __syncthreads();
            if (g < g1) {        // a frame before the record (g < 0) only turns the empty ring; past the run the ring is kept for the tail
                const bool emit = act[f] && g >= g0;
                const int64_t a0 = g * hop;
                for (int i = tid; i < hop; i += C::T) {
                    int p = r0 + i;
                    p = p >= n ? p - n : p;
                    const E s = ring[p];
                    ring[p] = E{};
                    const int64_t a = a0 + i, o = a - skip;
                    if (emit && o >= 0 && o < nout) st_stream(y + o, (a < head_len ? head[a] : period[i]) * s);
                }
                r0 += hop;
                r0 = r0 >= n ? r0 - n : r0;
            }
            __syncthreads();
        }
    }
    if (emit_tail && g1 == M && g0 < g1) {
        const int64_t a0 = M * hop;
        for (int i = tid; i < n - hop; i += C::T) {
            int p = r0 + i;
            p = p >= n ? p - n : p;
            const int64_t a = a0 + i, o = a - skip;
            if (o >= 0 && o < nout) st_stream(y + o, (a < head_len ? head[a] : tail[i]) * ring[p]);
        }
    }
}

// bin-major spectra in[ch][nb][M] -> frame-major out[ch][m][nb] for the frames f0 .. f0 + m - 1 (32 x 32 tiles through LDS)
static __global__ __launch_bounds__(256) void k_istft_gather(const cf *__restrict__ in, int64_t M, int nb, int64_t f0, int64_t m,
                                                            cf *__restrict__ out) {
    __shared__ cf tile[32][33];
    in += (int64_t)blockIdx.z * nb * M;
    out += (int64_t)blockIdx.z * m * nb;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t fb = (int64_t)blockIdx.x * 32;
    const int kb = blockIdx.y * 32;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int k = kb + r;
        const int64_t f = fb + tx;
        if (k < nb && f < m) tile[r][tx] = ld_stream(in + (int64_t)k * M + f0 + f);
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int64_t f = fb + r;
        const int k = kb + tx;
        if (k < nb && f < m) out[f * nb + k] = tile[tx][r];
    }
}

static size_t istft_lds(const Xf &xf, int mode) {
    const int fpw = fpw_of(xf.L);
    const size_t nr = (size_t)((xf.tb.n + 3) & ~3);
    return (size_t)fpw * nr * (mode == 0 ? sizeof(cf) : sizeof(float));
}

// mode 2 needs a power-of-two transform of at least 32 points
#define ISTFT_KERNEL_(XT, MD) (k_istft<XT, MD>)
int istft_resident(const Xf &xf, int mode) {
    const size_t ring = istft_lds(xf, mode);
#define R_(XT)                                                                                        \
    {                                                                                                 \
        const size_t lds = XT::C::lds_bytes(1) + ring;                                                \
        if (mode == 0) return resident_per_cu((const void *)ISTFT_KERNEL_(XT, 0), XT::C::WG, lds);    \
        if (mode == 1) return resident_per_cu((const void *)ISTFT_KERNEL_(XT, 1), XT::C::WG, lds);    \
        if constexpr (XT::EXACT && XT::L >= 32) return resident_per_cu((const void *)ISTFT_KERNEL_(XT, 2), XT::C::WG, lds); \
        return -1;                                                                                    \
    }
    SP_DISPATCH_X(xf, R_)
#undef R_
    return -1;
}

int launch_istft(LaunchCtx c, const cf *Z, int64_t z_cs, int64_t zbase, int64_t M, int64_t fbeg, int64_t fend, int64_t fpg, int halo,
                 const float *win, float wscale, int hop, const Xf &xf, int mode, const float *rcp, int64_t head_len, int64_t skip,
                 int64_t nout, void *y, int nch, int emit_tail) {
    if (fend <= fbeg || fpg < 1 || nch < 1 || mode < 0 || mode > 2) return -1;
    if (mode == 2 && ((fbeg | fpg | halo) & 1)) return -1;
    const int fpw = fpw_of(xf.L);
    const int64_t groups = (fend - fbeg + fpg - 1) / fpg;
    const dim3 grid((unsigned)((groups + fpw - 1) / fpw), (unsigned)nch);
    const size_t ring = istft_lds(xf, mode);
#define L_(XT, MD)                                                                                    \
    hipLaunchKernelGGL((k_istft<XT, MD>), grid, dim3(XT::C::WG), XT::C::lds_bytes(1) + ring, c.stream, Z, z_cs, zbase, M, fbeg, \
                       fend, fpg, halo, win, wscale, hop, xf.tb, rcp, head_len, skip, nout, y, emit_tail)
#define M_(XT)                                                                                        \
    if (mode == 0) L_(XT, 0);                                                                         \
    else if (mode == 1) L_(XT, 1);                                                                    \
    else {                                                                                            \
        if constexpr (XT::EXACT && XT::L >= 32) L_(XT, 2);                                            \
        else return -1;                                                                               \
    }
    SP_DISPATCH_X(xf, M_)
#undef M_
#undef L_
    return 0;
}

int launch_istft_gather(LaunchCtx c, const cf *in, int64_t M, int nb, int64_t f0, int64_t m, cf *out, int nch) {
    if (m < 1 || nb < 1 || nch < 1) return -1;
    hipLaunchKernelGGL(k_istft_gather, dim3((unsigned)((m + 31) / 32), (unsigned)((nb + 31) / 32), (unsigned)nch), dim3(256), 0,
                       c.stream, in, M, nb, f0, m, out);
    return 0;
}

}   // namespace sp
