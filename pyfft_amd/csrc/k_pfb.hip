// k_pfb.hip -- polyphase filter-bank channelizer (weighted overlap-add DFT bank): fold P M weighted samples down to M, transform.
//   X[m,k] = sum_{n<L} h[n] x[s + n] exp(-2 pi i k (n + rho_m) / M),  L = P M,  s = first + m hop,  x = 0 outside [0, nsig)
//   rho_m  = 0 (phase_ref 0) or (r0 + m hop) mod M (phase_ref 1: the phase of every channel refers to absolute time)
// as  u[i] = sum_{p<P} h[p M + j] x[s + p M + j],  j = (i - rho_m) mod M,  X[m,:] = FFT_M(u)   (spectral.h, sp_pfb).
//
// A transform group (T threads, SP_KERNEL_PROLOGUE) owns the run of frames [g0, g0 + fpg) of one row.  Thread tid holds the elements
// i = tid + T t of u.  For one branch p the T lanes of a group read consecutive j (one wrap at rho), so every load instruction of the
// samples and of the taps is coalesced across the group; the P branches are summed in the order p = 0 .. P - 1 with fused multiply-adds,
// which fixes the arithmetic of a frame whatever group computes it.  Consecutive frames of a group overlap in L - hop samples: they are
// re-read through L1 / L2 (plain loads), so that HBM sees the span of a run once.  The taps come from the device table cache.
// A frame whose L samples all lie inside the row takes the path without predicates; any other frame tests every sample against
// [0, nsig) and counts the ones outside as zero.  Both paths run the same multiply-adds, and which one a frame takes depends on the
// frame alone, so a frame's bits do not depend on the partition.
//
// OUT 0: frames, complex64 [row][frame][nb], streaming stores (sp_pfb transposes for the bin-major layout).
// OUT 1: power: |X|^2 summed over the run in fp32 registers, one partial[row][group][M] per group; k_pfb_finish sums the groups of a
//        row in float64 in a fixed order (no atomics) and scales.
// CPLX false: real float32 samples, zero imaginary part, one frame per transform; only the bins 0 .. M/2 are written.
// TREG: the taps of a thread are the same for every frame (rho constant), P <= SP_PFB_TREG_P and M <= SP_PFB_TREG_MAXM (at 8192 points
//       the 64 extra registers spill): held in registers across the run.
// blockIdx.x = row * blocks + block of the row (a grid of one dimension: the row count is not bounded by 65535).
#include "launch.h"
namespace sp {

template <class X, bool CPLX, int OUT, bool TREG>
__global__ __launch_bounds__(X::C::WG) void k_pfb(const void *__restrict__ x, int64_t x_ld, int64_t nsig, const float *__restrict__ taps,
                                                   int P, int hop, int64_t first, int64_t nframes, int64_t fpg, int blocks, int phase_ref,
                                                   int r0, XfTables tb, void *__restrict__ out, float *__restrict__ partial) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT, "power-of-two transforms only");
    constexpr int M = X::L, NB = CPLX ? M : M / 2 + 1;
    constexpr int PR = TREG ? SP_PFB_TREG_P : 1;
    const int64_t row = (int64_t)blockIdx.x / blocks;
    const int blk = (int)((int64_t)blockIdx.x % blocks);
    const int64_t gid = (int64_t)blk * C::FPW + grp;
    const int64_t g0 = gid * fpg;
    const int64_t L = (int64_t)P * M;
    const float *xr = reinterpret_cast<const float *>(x) + row * x_ld * (CPLX ? 2 : 1);
    float acc[OUT == 1 ? C::R : 1];
    if constexpr (OUT == 1) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) acc[t] = 0.f;
    }
    float hr[PR][C::R];
    if constexpr (TREG) {                         // rho is the same for every frame: r0 (phase_ref 1, hop a multiple of M) or 0
        const int rho = phase_ref ? r0 : 0;
#pragma unroll
        for (int p = 0; p < PR; ++p)
#pragma unroll
            for (int t = 0; t < C::R; ++t) hr[p][t] = p < P ? taps[p * M + ((tid + C::T * t - rho) & (M - 1))] : 0.f;
    }
    for (int64_t it = 0; it < fpg; ++it) {
        const int64_t m = g0 + it;
        const bool act = m < nframes;             // a frame past the end repeats the last one and is dropped: every barrier is met
        const int64_t mc = act ? m : nframes - 1;
        const int64_t s = first + mc * hop;
        const int rho = phase_ref ? (int)(((int64_t)r0 + mc * hop) & (M - 1)) : 0;
        int j[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) j[t] = (tid + C::T * t - rho) & (M - 1);
        cf v[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) v[t] = mk(0.f, 0.f);
        // one branch: v += h (.) x[s + p M + j], with or without the test against the row
        auto branch = [&](int p, const float (&h)[C::R], bool pred) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int64_t idx = s + p * M + j[t];
                const bool in = !pred || (idx >= 0 && idx < nsig);
                const int64_t e = in ? idx : 0;
                if constexpr (CPLX) {
                    cf a = reinterpret_cast<const cf *>(xr)[e];
                    a = in ? a : mk(0.f, 0.f);
                    v[t].x = __builtin_fmaf(h[t], a.x, v[t].x);
                    v[t].y = __builtin_fmaf(h[t], a.y, v[t].y);
                } else {
                    const float a = in ? xr[e] : 0.f;
                    v[t].x = __builtin_fmaf(h[t], a, v[t].x);
                }
            }
        };
        auto fold = [&](bool pred) __attribute__((always_inline)) {
            if constexpr (TREG) {
#pragma unroll
                for (int p = 0; p < PR; ++p)
                    if (p < P) branch(p, hr[p], pred);
            } else {
                for (int p = 0; p < P; ++p) {
                    float h[C::R];
#pragma unroll
                    for (int t = 0; t < C::R; ++t) h[t] = taps[p * M + j[t]];
                    branch(p, h, pred);
                }
            }
        };
        if (s >= 0 && s + L <= nsig) fold(false);
        else fold(true);
        fwd_row(xf, v, lds, tid, n);
        if constexpr (OUT == 1) {
            const float keep = act ? 1.f : 0.f;
#pragma unroll
            for (int t = 0; t < C::R; ++t) acc[t] += keep * cnorm(v[t]);
        } else if (act) {
            cf *o = reinterpret_cast<cf *>(out) + (row * nframes + m) * NB;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int k = tid + C::T * t;
                if (CPLX || k < NB) st_stream(o + k, v[t]);
            }
        }
    }
    if constexpr (OUT == 1) {
        float *p = partial + (row * ((int64_t)blocks * C::FPW) + gid) * M;
#pragma unroll
        for (int t = 0; t < C::R; ++t) p[tid + C::T * t] = acc[t];
    }
}

// pxx[row][k] = scale * sum_g partial[row][g][k], k < nb, in float64: 8 slices of the groups, each in group order, then the slices in
// order -- the same sum whatever ran first
#define SP_PFB_FIN_BINS 32
#define SP_PFB_FIN_SLICES 8
static __global__ __launch_bounds__(SP_PFB_FIN_BINS *SP_PFB_FIN_SLICES) void k_pfb_finish(const float *__restrict__ partial, int64_t G,
                                                                                         int M, int nb, double scale,
                                                                                         double *__restrict__ out) {
    __shared__ double sh[SP_PFB_FIN_SLICES][SP_PFB_FIN_BINS];
    const int lane = threadIdx.x % SP_PFB_FIN_BINS, sl = threadIdx.x / SP_PFB_FIN_BINS;
    const int k = blockIdx.x * SP_PFB_FIN_BINS + lane;
    const float *p = partial + (int64_t)blockIdx.y * G * M;
    double s = 0.0;
    if (k < nb)
        for (int64_t g = sl; g < G; g += SP_PFB_FIN_SLICES) s += (double)p[g * M + k];
    sh[sl][lane] = s;
    __syncthreads();
    if (sl == 0 && k < nb) {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < SP_PFB_FIN_SLICES; ++i) tot += sh[i][lane];
        out[(int64_t)blockIdx.y * nb + k] = tot * scale;
    }
}

bool pfb_treg_wanted(int M, int P, int hop, int phase_ref) {
    return M <= SP_PFB_TREG_MAXM && P <= SP_PFB_TREG_P && (phase_ref == 0 || hop % M == 0) && env_int("SP_PFB_TREG", SP_PFB_TREG_DEFAULT) != 0;
}

int launch_pfb(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const float *taps, int P, int hop,
               int64_t first, int64_t nframes, int phase_ref, int r0, const Xf &xf, const RunPart &rp, int out_kind, void *out,
               float *partial) {
    if (xf.blue || batch < 1 || nframes < 1 || P < 1 || P > SP_PFB_MAXP || hop < 1 || rp.fpg < 1 || rp.blocks < 1) return -1;
    if ((int64_t)rp.blocks * batch > 0x7fffffff) return -1;
    const bool treg = pfb_treg_wanted(xf.L, P, hop, phase_ref);
    const dim3 grid((unsigned)((int64_t)rp.blocks * batch));
#define L_(XT, CP, OK, TR)                                                                            \
    hipLaunchKernelGGL((k_pfb<XT, CP, OK, TR>), grid, dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, x_ld, nsig, taps, P, hop, \
                       first, nframes, rp.fpg, rp.blocks, phase_ref, r0, xf.tb, out, partial)
#define T_(XT, CP, OK)                                                                                \
    if constexpr (XT::L <= SP_PFB_TREG_MAXM) {                                                        \
        if (treg) L_(XT, CP, OK, true);                                                               \
        else L_(XT, CP, OK, false);                                                                   \
    } else {                                                                                          \
        L_(XT, CP, OK, false);                                                                        \
    }
#define M_(XT)                                                                                        \
    if (cplx) {                                                                                       \
        if (out_kind) { T_(XT, true, 1) } else { T_(XT, true, 0) }                                    \
    } else {                                                                                          \
        if (out_kind) { T_(XT, false, 1) } else { T_(XT, false, 0) }                                  \
    }
    SP_DISPATCH_P(xf, M_)
#undef M_
#undef T_
#undef L_
    return 0;
}

int launch_pfb_finish(LaunchCtx c, const float *partial, int64_t G, int M, int nb, int64_t batch, double scale, double *out) {
    if (batch < 1 || G < 1 || nb < 1) return -1;
    for (int64_t b0 = 0; b0 < batch; b0 += 65535) {              // grid.y takes 65535 rows
        const int64_t rows = batch - b0 < 65535 ? batch - b0 : 65535;
        hipLaunchKernelGGL(k_pfb_finish, dim3((nb + SP_PFB_FIN_BINS - 1) / SP_PFB_FIN_BINS, (unsigned)rows),
                           dim3(SP_PFB_FIN_BINS * SP_PFB_FIN_SLICES), 0, c.stream, partial + b0 * G * M, G, M, nb, scale, out + b0 * nb);
    }
    return 0;
}

}   // namespace sp
