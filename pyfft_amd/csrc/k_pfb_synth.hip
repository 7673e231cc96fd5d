// k_pfb_synth.hip -- polyphase synthesis bank, the adjoint of k_pfb's fold: inverse transforms of consecutive frames, spread over
// P M samples under the synthesis taps and overlap-added into one output stream.
//   v_m[i] = sum_{k<M} X[m][k] exp(+2 pi i k i / M)
//   y[a]   = sum_{m : 0 <= a - s_m < ntaps} tap[a - s_m] v_m[(a - s_m + rho_m) mod M],   s_m = first + m hop,   0 <= a < nout
//   rho_m  = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1);  tap = float32(g scale / M), rounded once on the host
// (spectral.h, sp_pfb_synth).  The sum over m runs in ascending frame order from zero with one fused multiply-add per component, in
// both paths below, so a sample's bits depend neither on the path nor on how the frames are dealt out to groups.
//
// k_pfb_synth<X, CPLX, true>, the fused path.  The mirror of k_istft with a ring of ntaps entries instead of n.  A transform group
// (T threads, SP_KERNEL_PROLOGUE) owns the run of frames [g0, g1) of one row and the output span [s_g0, s_g1); the first run of a row
// also owns [0, s_0) and the last one everything from s_g1 on.  It keeps ntaps accumulators (float, or cf for two-sided input) in LDS
// behind the exchange images: ring slot (ro + n) mod ntaps holds output sample s_m + n while frame m is the newest one added.
// Per frame: load the bins, conj, forward transform, conj (the inverse); thread tid holds i = tid + T t, so j = (i - rho) mod M and
// it adds tap[p M + j] v[i] for every p < P (distinct slots for distinct threads); barrier; stream out the `hop` samples no later
// frame reaches and clear them; advance ro by hop; barrier.  A run first accumulates the halo = ceil(ntaps / hop) - 1 frames before
// g0 without writing anything.  No atomics, no scratch.  Where the rings of all FPW groups of a workgroup do not fit its LDS only the
// first `ag` groups own frames and a ring (pfb_synth_groups); the others keep the barriers.
//
// k_pfb_synth<X, CPLX, false> + k_pfb_synth_gather, the composed path for rings that do not fit the LDS of one workgroup: the same
// loads and transforms, v_m stored to scratch [row][frame][M] (cf, or float for one-sided input), then one thread per output sample
// walks the <= ceil(ntaps / hop) frames that reach it in ascending order with the same multiply-adds; consecutive threads take
// consecutive samples, the overlap is re-read through L2.
//
// One-sided input (CPLX false, nb = M/2 + 1) is Hermitian-extended while loading; the imaginary parts of bins 0 and M/2 are ignored.
// blockIdx.x = row * blocks + block of the row (a grid of one dimension: the row count is not bounded by 65535).
#include "launch.h"
#include <type_traits>
namespace sp {

template <class X, bool CPLX, bool FUSED>
__global__ __launch_bounds__(X::C::WG) void k_pfb_synth(const cf *__restrict__ Xin, int64_t nframes, const float *__restrict__ taps,
                                                         int P, int hop, int64_t first, int64_t fpg, int halo, int blocks,
                                                         int ag, int phase_ref, int r0, XfTables tb, int64_t nout, void *__restrict__ yout,
                                                         void *__restrict__ vout) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT, "power-of-two transforms only");
    using E = std::conditional_t<CPLX, cf, float>;
    constexpr int M = X::L, NH = M / 2, NB = CPLX ? M : NH + 1;
    const int64_t row = (int64_t)blockIdx.x / blocks;
    const int blk = (int)((int64_t)blockIdx.x % blocks);
    const bool idle = grp >= ag;                                     // a group without a ring: it owns no frames
    const int64_t gid = (int64_t)blk * ag + grp;
    const int64_t g0 = idle ? nframes : gid * fpg;
    const int64_t g1 = g0 + fpg < nframes ? g0 + fpg : nframes;    // g1 <= g0: a group past the end (it only keeps the barriers)
    const bool owner = g0 < g1;                                      // (its halo frames belong to other groups: it skips them too)
    const int ntaps = P * M;
    const cf *Xr = Xin + row * nframes * NB;
    E *ring = nullptr, *y = nullptr;
    if constexpr (FUSED) {
        ring = reinterpret_cast<E *>(smem + C::FPW * C::LDS_PER) + (size_t)(idle ? 0 : grp) * ntaps;
        y = reinterpret_cast<E *>(yout) + row * nout;
        if (!idle)
            for (int i = tid; i < ntaps; i += C::T) ring[i] = E{};
        if (g0 == 0) {                                               // nothing reaches the samples before frame 0
            const int64_t z = first < nout ? first : nout;
            for (int64_t a = tid; a < z; a += C::T) st_stream(y + a, E{});
        }
        __syncthreads();
    }
    const int hopm = hop % ntaps;
    const int64_t steps = FUSED ? fpg + halo : fpg;
    int ro = 0;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t m = g0 - (FUSED ? halo : 0) + it;
        const bool act = owner && m >= 0 && m < g1;
        cf v[C::R];
        if (act) {
            const cf *za = Xr + m * NB;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int k = tid + C::T * t;
                if constexpr (CPLX) {
                    v[t] = cconj(ld_stream(za + k));
                } else {
                    const bool low = k <= NH;
                    const bool edge = k == 0 || 2 * k == M;
                    cf a = ld_stream(za + (low ? k : M - k));
                    a.y = edge ? 0.f : (low ? -a.y : a.y);                    // conj of the Hermitian extension
                    v[t] = a;
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = mk(0.f, 0.f);
        }
        fwd_row(xf, v, lds, tid, n);                                          // v = conj(unnormalised inverse transform)
        if constexpr (!FUSED) {
            if (act) {
                E *o = reinterpret_cast<E *>(vout) + (row * nframes + m) * M;
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    if constexpr (CPLX) o[tid + C::T * t] = mk(v[t].x, -v[t].y);
                    else o[tid + C::T * t] = v[t].x;
                }
            }
        } else {
            if (act) {
                const int rho = phase_ref ? (int)(((int64_t)r0 + m * hop) & (M - 1)) : 0;
#pragma unroll
                for (int t = 0; t < C::R; ++t) {
                    const int j = (tid + C::T * t - rho) & (M - 1);
                    for (int p = 0; p < P; ++p) {
                        const int nn = p * M + j;
                        int s = ro + nn;
                        s = s >= ntaps ? s - ntaps : s;
                        const float w = taps[nn];
                        if constexpr (CPLX) {
                            const cf c = ring[s];
                            ring[s] = mk(__builtin_fmaf(w, v[t].x, c.x), __builtin_fmaf(w, -v[t].y, c.y));
                        } else {
                            ring[s] = __builtin_fmaf(w, v[t].x, ring[s]);
                        }
                    }
                }
            }
            __syncthreads();
            if (act) {            // a frame before the record leaves the empty ring as it is; past the run the ring is kept for the tail
                const bool emit = m >= g0;
                const int64_t a0 = first + m * hop;
                for (int i = tid; i < hop; i += C::T) {
                    E sv = E{};
                    if (i < ntaps) {                                          // hop > ntaps: the samples in between are zero
                        int s = ro + i;
                        s = s >= ntaps ? s - ntaps : s;
                        sv = ring[s];
                        ring[s] = E{};
                    }
                    const int64_t a = a0 + i;
                    if (emit && a >= 0 && a < nout) st_stream(y + a, sv);
                }
                ro += hopm;
                ro = ro >= ntaps ? ro - ntaps : ro;
            }
            __syncthreads();
        }
    }
    if constexpr (FUSED) {
        if (g1 == nframes && owner) {                                      // the last run: what is left in the ring, then zeros
            const int64_t a0 = first + nframes * hop;
            const int64_t left = (int64_t)ntaps - hop;
            for (int64_t a = (a0 > 0 ? a0 : 0) + tid; a < nout; a += C::T) {
                const int64_t i = a - a0;
                E sv = E{};
                if (i < left) {
                    int s = ro + (int)i;
                    s = s >= ntaps ? s - ntaps : s;
                    sv = ring[s];
                }
                st_stream(y + a, sv);
            }
        }
    }
}

// y[row][a] from the inverse transforms V[row][frame][M]: the frames that reach a in ascending order, one fused multiply-add per
// component; bpr blocks per row, a block strides over the row
template <bool CPLX>
static __global__ __launch_bounds__(256) void k_pfb_synth_gather(const void *__restrict__ V, int64_t nframes,
                                                                  const float *__restrict__ taps, int ntaps, int M, int hop,
                                                                  int64_t first, int phase_ref, int r0, int64_t nout, int bpr,
                                                                  void *__restrict__ yout) {
    using E = std::conditional_t<CPLX, cf, float>;
    const int64_t row = (int64_t)blockIdx.x / bpr;
    const int blk = (int)((int64_t)blockIdx.x % bpr);
    const E *Vr = reinterpret_cast<const E *>(V) + row * nframes * M;
    E *y = reinterpret_cast<E *>(yout) + row * nout;
    for (int64_t a = (int64_t)blk * 256 + threadIdx.x; a < nout; a += (int64_t)bpr * 256) {
        E acc = E{};
        const int64_t d = a - first;
        if (d >= 0) {
            int64_t mhi = d / hop;
            mhi = mhi < nframes - 1 ? mhi : nframes - 1;
            const int64_t e = d - (ntaps - 1);
            const int64_t mlo = e <= 0 ? 0 : (e + hop - 1) / hop;
            for (int64_t m = mlo; m <= mhi; ++m) {
                const int nn = (int)(d - m * hop);
                const int rho = phase_ref ? (int)(((int64_t)r0 + m * hop) & (M - 1)) : 0;
                const float w = taps[nn];
                const E c = Vr[m * M + ((nn + rho) & (M - 1))];
                if constexpr (CPLX) acc = mk(__builtin_fmaf(w, c.x, acc.x), __builtin_fmaf(w, c.y, acc.y));
                else acc = __builtin_fmaf(w, c, acc);
            }
        }
        st_stream(y + a, acc);
    }
}

// groups of a workgroup that get a ring in the fused form at this shape: as many of the FPW as fit the LDS behind the exchange images,
// 0 when not even one ring fits (host only)
int pfb_synth_groups(int M, int ntaps, bool cplx, size_t *lds_out) {
    const size_t ring = (size_t)ntaps * (cplx ? sizeof(cf) : sizeof(float));
    size_t img = 0;
#define R_(XT) img = XT::C::lds_bytes(1);
    switch (M) {
        SP_CASE_P(2, R_) SP_CASE_P(4, R_) SP_CASE_P(8, R_) SP_CASE_P(16, R_) SP_CASE_P(32, R_) SP_CASE_P(64, R_) SP_CASE_P(128, R_)
        SP_CASE_P(256, R_) SP_CASE_P(512, R_) SP_CASE_P(1024, R_) SP_CASE_P(2048, R_) SP_CASE_P(4096, R_) SP_CASE_P(8192, R_)
        default: return 0;
    }
#undef R_
    if (img + ring > SP_LDS_MAX) return 0;
    const size_t fit = (SP_LDS_MAX - img) / ring, fpw = (size_t)fpw_of(M);
    const int ag = (int)(fit < fpw ? fit : fpw);
    if (lds_out) *lds_out = img + (size_t)ag * ring;
    return ag;
}

int launch_pfb_synth(LaunchCtx c, const cf *X, bool cplx, int64_t batch, int64_t nframes, const float *taps, int P, int hop,
                     int64_t first, int phase_ref, int r0, const Xf &xf, int64_t fpg, int halo, bool fused, int64_t nout, void *y,
                     void *v) {
    if (xf.blue || batch < 1 || nframes < 1 || P < 1 || P > SP_PFB_MAXP || hop < 1 || fpg < 1 || halo < 0 || nout < 1) return -1;
    size_t lds_f = 0;
    const int ag = fused ? pfb_synth_groups(xf.L, P * xf.L, cplx, &lds_f) : fpw_of(xf.L);
    if (ag < 1) return -1;
    const int64_t groups = (nframes + fpg - 1) / fpg, blocks = (groups + ag - 1) / ag;
    if (blocks * batch > 0x7fffffff) return -1;
    const dim3 grid((unsigned)(blocks * batch));
#define L_(XT, CP, FU)                                                                                \
    {                                                                                                 \
        const size_t lds = FU ? lds_f : XT::C::lds_bytes(1);                                          \
        if (lds_raise<k_pfb_synth<XT, CP, FU>>(lds)) return -1;                                       \
        hipLaunchKernelGGL((k_pfb_synth<XT, CP, FU>), grid, dim3(XT::C::WG), lds, c.stream, X, nframes, taps, P, hop, first, fpg,   \
                           halo, (int)blocks, ag, phase_ref, r0, xf.tb, nout, y, v);                     \
    }
#define M_(XT)                                                                                        \
    if (cplx) {                                                                                       \
        if (fused) L_(XT, true, true) else L_(XT, true, false)                                        \
    } else {                                                                                          \
        if (fused) L_(XT, false, true) else L_(XT, false, false)                                      \
    }
    SP_DISPATCH_P(xf, M_)
#undef M_
#undef L_
    return 0;
}

int launch_pfb_synth_gather(LaunchCtx c, const void *v, bool cplx, int64_t batch, int64_t nframes, const float *taps, int ntaps, int M,
                            int hop, int64_t first, int phase_ref, int r0, int64_t nout, void *y) {
    if (batch < 1 || batch > 0x7fffffff || nframes < 1 || nout < 1 || hop < 1) return -1;
    int64_t bpr = (nout + 255) / 256;
    const int64_t cap = 0x7fffffff / batch;
    bpr = bpr < cap ? bpr : cap;
    const dim3 grid((unsigned)(bpr * batch));
    if (cplx)
        hipLaunchKernelGGL((k_pfb_synth_gather<true>), grid, dim3(256), 0, c.stream, v, nframes, taps, ntaps, M, hop, first, phase_ref,
                           r0, nout, (int)bpr, y);
    else
        hipLaunchKernelGGL((k_pfb_synth_gather<false>), grid, dim3(256), 0, c.stream, v, nframes, taps, ntaps, M, hop, first, phase_ref,
                           r0, nout, (int)bpr, y);
    return 0;
}

}   // namespace sp
