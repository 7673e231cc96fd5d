// k_welch.hip -- fused Welch PSD launchers (generic + register-carried metric kernel + one-pass detrend epilogue)
#include "launch.h"
#include <map>
#include <mutex>
namespace sp {

// column sums, in double, of two float matrices with G rows in ONE launch: m0[G][c0] -> o0[c0] (the raw |X|^2 sums
// A[k]) and m1[G][c1] -> o1[c1] (the block sums: spartial[G][H] complex seen as [G][2H] floats -> Sl[2j], Sl[2j+1]).
// block = 32 columns x 32 row slices (1024 threads), 4 independent loads in flight per thread; deterministic order.
static __global__ __launch_bounds__(1024) void k_op_colsums(const float *__restrict__ m0, int c0, double *__restrict__ o0,
                                                             const float *__restrict__ m1, int c1, double *__restrict__ o1,
                                                             int64_t G) {
    __shared__ double sh[32][32];
    const int nb0 = (c0 + 31) / 32;
    const bool second = (int)blockIdx.x >= nb0;
    const float *__restrict__ m = second ? m1 : m0;
    const int cols = second ? c1 : c0;
    double *__restrict__ o = second ? o1 : o0;
    const int lane = threadIdx.x % 32, sl = threadIdx.x / 32;
    const int k = ((int)blockIdx.x - (second ? nb0 : 0)) * 32 + lane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (k < cols) {
        int64_t g = sl;
        for (; g + 96 < G; g += 128) {
            const float a0 = m[g * cols + k], a1 = m[(g + 32) * cols + k], a2 = m[(g + 64) * cols + k], a3 = m[(g + 96) * cols + k];
            s0 += (double)a0;
            s1 += (double)a1;
            s2 += (double)a2;
            s3 += (double)a3;
        }
        for (; g < G; g += 32) s0 += (double)m[g * cols + k];
    }
    sh[sl][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0 && k < cols) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 32; ++q) t += sh[q][lane];
        o[k] = t;
    }
}

// tot = sum_{i < nmean} (x[i] - mu0): block sums cover [(r-1)H, (M+r-1)H); add the head blocks and fix the end.
// one block of 1024 threads.
// also: sum_out = tot + nmean*mu0 (the shard's plain sample sum) and dlt = tot/nmean (delta for the shard's own mean)
template <bool CPLX>
static __global__ __launch_bounds__(1024) void k_op_total(const void *__restrict__ x, const float *__restrict__ trend,
                                                           const double *__restrict__ Sl, int H, int r, int64_t M,
                                                           int64_t nmean, double *__restrict__ tot,
                                                           double *__restrict__ dlt, double *__restrict__ sum_out) {
    __shared__ double sh[2][1024];
    const cf mu = mk(trend[0], trend[1]);
    double a = 0, b = 0;
    for (int j = threadIdx.x; j < H; j += 1024) {
        a += Sl[2 * j];
        b += Sl[2 * j + 1];
    }
    const int64_t head = (int64_t)(r - 1) * H;           // samples before the first counted block
    const int64_t cov = (M + r - 1) * (int64_t)H;        // end of the last counted block
    for (int64_t i = threadIdx.x; i < head; i += 1024) {
        const cf v = load_sample(x, i, CPLX) - mu;
        a += v.x;
        b += v.y;
    }
    if (nmean > cov) {
        for (int64_t i = cov + threadIdx.x; i < nmean; i += 1024) {
            const cf v = load_sample(x, i, CPLX) - mu;
            a += v.x;
            b += v.y;
        }
    } else {
        for (int64_t i = nmean + threadIdx.x; i < cov; i += 1024) {
            const cf v = load_sample(x, i, CPLX) - mu;
            a -= v.x;
            b -= v.y;
        }
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tot[0] = sh[0][0];
        tot[1] = sh[1][0];
        dlt[0] = sh[0][0] / (double)nmean;
        dlt[1] = sh[1][0] / (double)nmean;
        sum_out[0] = sh[0][0] + (double)nmean * (double)trend[0];
        sum_out[1] = sh[1][0] + (double)nmean * (double)trend[1];
    }
}

// one workgroup: c[n] = sum_g x_g[n] rebuilt from the block sums and the few edge blocks, B = FFT(w c) = sum_g X_g,
// then out[slot] = scale * doubling * (A[k] - 2 Re(conj(d W[k]) B[k]) + M |d W[k]|^2) with d = mean - mu0.
// mean_in != null (the caller's global mean) overrides the shard's own delta.
// EXPORT: instead of the finished spectrum, write this shard's additive state (see sp_welch_export) into `out`:
//   out[0..N) = A[k]   out[N..3N) = B[k] (re, im)   out[3N..5N) = conj(mu0) B[k]
//   out[5N..5N+8) = M mu0 (re, im), M |mu0|^2, sum of the nmean own samples (re, im), M, nmean, 0
template <int N, bool CPLX, bool EXPORT = false>
static __global__ __launch_bounds__(WgCfg<N>::WG) void k_op_finish(const void *__restrict__ x, const float *__restrict__ trend,
                                                                    const float *__restrict__ win,
                                                                    const double *__restrict__ Sl,
                                                                    const double *__restrict__ A, const cf *__restrict__ Wf,
                                                                    const double *__restrict__ dlt_local,
                                                                    const double *__restrict__ mean_in, int H, int r,
                                                                    int64_t M, int64_t nmean, int sided, double scale,
                                                                    XfTables tb, double *__restrict__ out, int sym,
                                                                    int64_t x_cs = 0, int64_t sl_cs = 0, int64_t out_cs = 0) {
    using X = XfPow2<N>;
    SP_KERNEL_PROLOGUE(X)
    (void)n;
    // one workgroup per signal: blockIdx.x selects the channel of a multi-channel call (strides in samples / doubles; all zero
    // for the single-signal callers, whose grid is one workgroup)
    x = reinterpret_cast<const char *>(x) + (int64_t)blockIdx.x * x_cs * (CPLX ? 8 : 4);
    trend += x_cs ? 4 * blockIdx.x : 0;
    Sl += (int64_t)blockIdx.x * sl_cs;
    out += (int64_t)blockIdx.x * out_cs;
    const cf mu = mk(trend[0], trend[1]);
    // this single workgroup is one chain of memory round trips: everything that does not depend on a computed value
    // (window, raw sums, FFT(window)) is fetched up front, together with the twiddle tables of the prologue
    double a_pre[C::R];
    cf wf_pre[C::R];
    float win_pre[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int k = tid + C::T * t;
        a_pre[t] = sym ? 0.5 * (A[k] + A[(N - k) & (N - 1)]) : A[k];
        wf_pre[t] = Wf[k];
        win_pre[t] = win[k];
    }
    double dr, di;
    double tot_r = 0.0, tot_i = 0.0;
    if (!EXPORT && mean_in) {
        dr = mean_in[0] - (double)trend[0];
        di = mean_in[1] - (double)trend[1];
    } else if (!EXPORT && dlt_local) {
        dr = dlt_local[0];
        di = dlt_local[1];
    } else {
        // the shard's own mean (what k_op_total computes for the split ABI), here without the extra launch:
        // sum_{i<nmean}(x[i] - mu0) = all block sums + head blocks +/- the ragged end
        double a = 0, b = 0;
        // H <= N and head < N: fixed trip counts with masks, so that all loads of a thread are in flight together
        // (this workgroup is one latency chain; with data-dependent loops it cost 28 us per step)
        constexpr int NIT = N / C::WG > 0 ? N / C::WG : 1;
        const int64_t head = (int64_t)(r - 1) * H, cov = (M + r - 1) * (int64_t)H;
        {
            double sa[NIT], sb[NIT];
            cf hv[NIT];
#pragma unroll
            for (int q = 0; q < NIT; ++q) {
                const int j = (int)threadIdx.x + q * C::WG;
                const int jc = j < H ? j : 0;
                sa[q] = Sl[2 * jc];
                sb[q] = Sl[2 * jc + 1];
                hv[q] = load_sample(x, j < head ? j : 0, CPLX);
            }
#pragma unroll
            for (int q = 0; q < NIT; ++q) {
                const int j = (int)threadIdx.x + q * C::WG;
                if (j < H) {
                    a += sa[q];
                    b += sb[q];
                }
                if (j < head) {
                    a += (double)(hv[q].x - mu.x);
                    b += (double)(hv[q].y - mu.y);
                }
            }
        }
        const int64_t lo = nmean > cov ? cov : nmean, hi = nmean > cov ? nmean : cov;
        const double sgn = nmean > cov ? 1.0 : -1.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += C::WG) {
            const cf s = load_sample(x, i, CPLX) - mu;
            a += sgn * s.x;
            b += sgn * s.y;
        }
        double *red = reinterpret_cast<double *>(smem);           // 2 x WG doubles, before the transform uses the LDS
        red[threadIdx.x] = a;
        red[C::WG + threadIdx.x] = b;
        __syncthreads();
        for (int o = C::WG / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                red[threadIdx.x] += red[threadIdx.x + o];
                red[C::WG + threadIdx.x] += red[C::WG + threadIdx.x + o];
            }
            __syncthreads();
        }
        tot_r = red[0];
        tot_i = red[C::WG];
        dr = tot_r / (double)nmean;
        di = tot_i / (double)nmean;
        __syncthreads();
    }
    cf v[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int nidx = tid + C::T * t;
        const int q = nidx / H, j = nidx % H;
        double a = Sl[2 * j], b = Sl[2 * j + 1];
        for (int bb = q; bb <= r - 2; ++bb) {
            const cf s = load_sample(x, (int64_t)bb * H + j, CPLX) - mu;
            a += s.x;
            b += s.y;
        }
        for (int64_t bb = M + q; bb <= M + r - 2; ++bb) {
            const cf s = load_sample(x, bb * H + j, CPLX) - mu;
            a -= s.x;
            b -= s.y;
        }
        const double wn = (double)win_pre[t];
        v[t] = (grp == 0) ? mk((float)(wn * a), (float)(wn * b)) : mk(0.f, 0.f);
    }
    xf.fwd(v, lds, tid, N);
    if constexpr (EXPORT) {
        if (grp == 0) {
            const double mr = (double)mu.x, mi = (double)mu.y;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int k = tid + C::T * t;
                const double br = (double)v[t].x, bi = (double)v[t].y;
                out[k] = a_pre[t];
                out[N + 2 * k] = br;
                out[N + 2 * k + 1] = bi;
                out[3 * N + 2 * k] = mr * br + mi * bi;          // conj(mu0) B
                out[3 * N + 2 * k + 1] = mr * bi - mi * br;
            }
            if (threadIdx.x == 0) {
                double *sc = out + 5 * N;
                sc[0] = (double)M * mr;
                sc[1] = (double)M * mi;
                sc[2] = (double)M * (mr * mr + mi * mi);
                sc[3] = tot_r + (double)nmean * mr;
                sc[4] = tot_i + (double)nmean * mi;
                sc[5] = (double)M;
                sc[6] = (double)nmean;
                sc[7] = 0.0;
            }
        }
        return;
    }
    if (grp == 0) {
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int k = tid + C::T * t;
            const int slot = bin_slot(k, N, sided);
            if (slot < 0) continue;
            const double wr = wf_pre[t].x, wi = wf_pre[t].y;
            const double er = dr * wr - di * wi, ei = dr * wi + di * wr;       // d * Wf[k]
            const double p = a_pre[t] - 2.0 * (er * (double)v[t].x + ei * (double)v[t].y) + (double)M * (er * er + ei * ei);
            out[slot] = p * scale * (bin_doubled(k, N, sided) ? 2.0 : 1.0);
        }
    }
}

// The all-reduced (summed over shards) state of k_op_finish<EXPORT> -> the PSD of the whole stream, detrended by the
// global mean mu = S / n:  P[k] = A - 2 Re(conj(W) (conj(mu) B - C)) + |W|^2 (|mu|^2 M - 2 Re(conj(mu) S1) + S2)
// (each shard's sum |X - (mu - mu0_r) W|^2, expanded so that only sums over shards appear).
// mean != null: the caller's (re, im) mean instead of the state's own S / n (the split ABI's finish on a pending state)
static __global__ __launch_bounds__(256) void k_op_apply(const double *__restrict__ st, const cf *__restrict__ Wf, int n,
                                                         int sided, double scale, double *__restrict__ out,
                                                         const double *__restrict__ mean) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int slot = bin_slot(k, n, sided);
    if (slot < 0) return;
    const double *sc = st + 5 * (int64_t)n;
    const double Mt = sc[5], nt = sc[6];
    const double mr = mean ? mean[0] : sc[3] / nt, mi = mean ? mean[1] : sc[4] / nt;
    const double br = st[n + 2 * k], bi = st[n + 2 * k + 1], cr = st[3 * n + 2 * k], ci = st[3 * n + 2 * k + 1];
    const double dr = mr * br + mi * bi - cr, di = mr * bi - mi * br - ci;            // conj(mu) B - C
    const double wr = Wf[k].x, wi = Wf[k].y;
    const double cross = wr * dr + wi * di;                                            // Re(conj(W) D)
    const double s = (mr * mr + mi * mi) * Mt - 2.0 * (mr * sc[0] + mi * sc[1]) + sc[2];
    const double p = st[k] - 2.0 * cross + (wr * wr + wi * wi) * s;
    out[slot] = p * scale * (bin_doubled(k, n, sided) ? 2.0 : 1.0);
}

template <bool CPLX>
static __global__ __launch_bounds__(1024) void k_op_estimate(const void *__restrict__ x, int64_t nsig,
                                                              float *__restrict__ trend) {
    __shared__ double sh[2][1024];
    const int64_t len = nsig / SP_EST_RUNS < SP_EST_LEN ? nsig / SP_EST_RUNS : SP_EST_LEN;     // may be 0 for tiny signals
    const int64_t pitch = nsig / SP_EST_RUNS;
    double a = 0, b = 0;
    // wave w covers runs w, w+16, w+32, w+48; lane l the elements l + 64 j of a run.  All 64 loads of a thread are
    // independent and unconditional (index clamped, value masked) so that they are in flight together: the kernel
    // costs one memory round trip instead of sixteen.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (len > 0) {
#pragma unroll
        for (int m = 0; m < SP_EST_RUNS / 16; ++m) {
            const int64_t base = pitch * (wv + 16 * m);
            cf v[SP_EST_LEN / 64];
#pragma unroll
            for (int j = 0; j < SP_EST_LEN / 64; ++j) {
                const int64_t i = lane + 64 * j;
                v[j] = load_sample(x, base + (i < len ? i : len - 1), CPLX);
            }
            float fa = 0.f, fb = 0.f;          // 16 terms per partial: float is ample, the rest is summed in double
#pragma unroll
            for (int j = 0; j < SP_EST_LEN / 64; ++j) {
                const float keep = (lane + 64 * j) < len ? 1.f : 0.f;
                fa = fmaf(keep, v[j].x, fa);
                fb = fmaf(keep, v[j].y, fb);
            }
            a += (double)fa;
            b += (double)fb;
        }
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = (double)(len * SP_EST_RUNS);
        trend[0] = cnt > 0 ? (float)(sh[0][0] / cnt) : 0.f;
        trend[1] = cnt > 0 ? (float)(sh[1][0] / cnt) : 0.f;
        trend[2] = 0.f;
        trend[3] = 0.f;
    }
}

static __global__ __launch_bounds__(SP_FIN_BINS *SP_FIN_SLICES) void k_welch_finish(const float *__restrict__ partial, int64_t G,
                                                                                     int L, int n, int sided, double scale,
                                                                                     double *__restrict__ out, int sym) {
    __shared__ double sh[SP_FIN_SLICES][SP_FIN_BINS];
    const int lane = threadIdx.x % SP_FIN_BINS, sl = threadIdx.x / SP_FIN_BINS;
    const int k = blockIdx.x * SP_FIN_BINS + lane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (k < n) {
        int64_t g = sl;
        for (; g + 3 * SP_FIN_SLICES < G; g += 4 * SP_FIN_SLICES) {
            const float a0 = partial[g * L + k], a1 = partial[(g + SP_FIN_SLICES) * L + k];
            const float a2 = partial[(g + 2 * SP_FIN_SLICES) * L + k], a3 = partial[(g + 3 * SP_FIN_SLICES) * L + k];
            s0 += (double)a0;
            s1 += (double)a1;
            s2 += (double)a2;
            s3 += (double)a3;
        }
        for (; g < G; g += SP_FIN_SLICES) s0 += (double)partial[g * L + k];
        if (sym) {
            const int km = k == 0 ? 0 : n - k;
            double m = 0.0;
            for (int64_t g2 = sl; g2 < G; g2 += SP_FIN_SLICES) m += (double)partial[g2 * L + km];
            s0 = 0.5 * ((s0 + s1) + (s2 + s3) + m);
            s1 = s2 = s3 = 0.0;
        }
    }
    sh[sl][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0 && k < n) {
        const int slot = bin_slot(k, n, sided);
        if (slot >= 0) {
            double tot = 0.0;
#pragma unroll
            for (int j = 0; j < SP_FIN_SLICES; ++j) tot += sh[j][lane];
            out[slot] = tot * scale * (bin_doubled(k, n, sided) ? 2.0 : 1.0);
        }
    }
}

// LOBEB: the main kernel ran in mode 9 (k_welch_pipe): no block sums -- m1 is lobeB[G][8], the groups' sums of the spectra at the
// bins ks = -3 .. 3 (index ks + 3), and the window adds up to the constant cola_c at this hop.  B[ks] = sum_G lobeB; the plain sum
// of the samples follows from the DC bin: B[0] = sum_i cov(i) (x[i] - mu0), cov(i) = sum of the window values of the frames that
// cover sample i = cola_c everywhere but within N - H samples of the two ends, so sum_i (x[i] - mu0) = (B[0] + sum_edges (cola_c -
// cov(i)) (x[i] - mu0)) / cola_c -- a few thousand samples read by the last block.  No column sums of block sums (half of phase 1),
// no c[n] rebuild (the last block's big round trip).
template <bool CPLX, bool EXPORT, int E, bool LIGHT = false, bool LOBEB = false>
static __global__ __launch_bounds__(LIGHT ? SP_OPF_WG_LIGHT : SP_OPF_WG)
    __attribute__((amdgpu_waves_per_eu(LIGHT ? 6 : 2, LIGHT ? 8 : 2))) void k_op_fused(const float *__restrict__ m0, int N, double *__restrict__ Acol,
                                                                const float *__restrict__ m1, int H, double *__restrict__ Sl,
                                                                int64_t G, unsigned *__restrict__ ticket,
                                                                const void *__restrict__ x, const float *__restrict__ trend,
                                                                const float *__restrict__ win, CogLobe lb,
                                                                const double *__restrict__ mean_in, int64_t M, int64_t nmean,
                                                                int sided, double scale, double *__restrict__ out, int sym,
                                                                OpPrev prev, double step_c, double step_s, double cola_c) {
    constexpr int WG = LIGHT ? SP_OPF_WG_LIGHT : SP_OPF_WG, NW = WG / 64, NSL = WG / 8;
    __shared__ double sh[NW][32];
    __shared__ double tot_sh[16];
    __shared__ int last_flag;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    {   // ---- phase 1: column sums of m0 [G][N] -> Acol and of m1 [G][2H] -> Sl.  A block owns 32 columns = 8 lanes of float4;
        // its NSL row slices: 8 per wave (summed by shuffles), NW waves (summed through LDS); 4 loads per thread in flight
        const int c0 = N, c1 = 2 * H;
        const int nb0 = c0 / 32;
        const bool second = (int)blockIdx.x >= nb0;
        const float *__restrict__ m = second ? m1 : m0;
        const int cols = second ? c1 : c0;
        double *__restrict__ o = second ? Sl : Acol;
        const int l8 = threadIdx.x & 7, sl = threadIdx.x >> 3;
        const int kb = ((int)blockIdx.x - (second ? nb0 : 0)) * 32;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t g0 = sl; g0 < G; g0 += 4 * NSL) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t g = g0 + NSL * u;
                v[u] = g < G ? *reinterpret_cast<const float4 *>(m + g * cols + kb + 4 * l8) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s[0] += (double)v[u].x;
                s[1] += (double)v[u].y;
                s[2] += (double)v[u].z;
                s[3] += (double)v[u].w;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[q] += __shfl_xor(s[q], 8);
            s[q] += __shfl_xor(s[q], 16);
            s[q] += __shfl_xor(s[q], 32);
        }
        if (ln < 8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sh[wv][4 * ln + q] = s[q];
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += sh[w][threadIdx.x];
            st_sc1(o + kb + threadIdx.x, t);
        }
    }
    // ---- hand-off: the sc1 stores above all come from wave 0; it drains them, its lane 0 takes a ticket
    if (threadIdx.x < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) {
        // two levels (256 adds on one word take 3 us): the blocks with equal blockIdx % 8 share a counter (64 bytes apart), the
        // last arriver of each group adds to the top counter, the last of those is the last block of the grid
        const unsigned grp = blockIdx.x & 7u, ngrp = gridDim.x < 8u ? gridDim.x : 8u;
        const unsigned members = (gridDim.x - 1u - grp) / 8u + 1u;
        int last = 0;
        if (__hip_atomic_fetch_add(ticket + 16 * grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1u)
            last = __hip_atomic_fetch_add(ticket + 16 * 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngrp - 1u;
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag) return;
    // ---- phase 2 (the last block to arrive; Acol / Sl are read with sc1 loads only)
    const cf mu = mk(trend[0], trend[1]);
    const int hs = __builtin_ctz((unsigned)H);                 // H is a power of two on this path (launch_op_fused checks)
    const int r = N >> hs;
    const int64_t cov = (M + r - 1) * (int64_t)H;
    // 16 sums of ONE block reduction: [0,1] sum_{i < nmean} (x[i] - mu0), [2 + 2 q, 3 + 2 q] B[ks = q - 3]
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    if (EXPORT || !mean_in) {         // the ragged end (nothing for a whole signal, one hop for a shard)
        const int64_t lo = nmean > cov ? cov : nmean, hi = nmean > cov ? nmean : cov;
        const double sgn = nmean > cov ? 1.0 : -1.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += WG) {
            const cf v = load_sample(x, i, CPLX) - mu;
            acc[0] += sgn * v.x;
            acc[1] += sgn * v.y;
        }
    }
    constexpr int NPT = LIGHT ? 2 : ((E > 1 && CPLX) ? 4 : 8);    // bins per thread and chunk: N <= 4096 is one chunk, one round trip (hop = N/4, complex: two)
    double ak[NPT];                                 // raw sums A[k] of the thread's bins (kept for the output loop)
    if constexpr (LOBEB) {
        const cf *__restrict__ lobeB = reinterpret_cast<const cf *>(m1);
        for (int64_t g = threadIdx.x; g < G; g += WG) {
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const cf v = lobeB[g * 8 + q];
                acc[2 + 2 * q] += (double)v.x;
                acc[3 + 2 * q] += (double)v.y;
            }
        }
        if (EXPORT || !mean_in) {
            // the two edges, where fewer than r frames cover a sample: (cola_c - cov(i)) (x[i] - mu0) / cola_c
            const int64_t nhead = (int64_t)(r - 1) * H, mh = M * (int64_t)H;
            const int64_t tail0 = mh > nhead ? mh : nhead;
            const double ic = 1.0 / cola_c;
            for (int side = 0; side < 2; ++side) {
                const int64_t i0 = side ? tail0 : 0, i1 = side ? cov : (nhead < cov ? nhead : cov);
                for (int64_t i = i0 + threadIdx.x; i < i1; i += WG) {
                    int64_t ghi = i >> hs;
                    ghi = ghi < M - 1 ? ghi : M - 1;
                    const int64_t glo = i >= N ? ((i - N) >> hs) + 1 : 0;
                    double cv = 0.0;
                    for (int64_t gg = glo; gg <= ghi; ++gg) cv += (double)win[i - (gg << hs)];
                    const cf v = load_sample(x, i, CPLX) - mu;
                    const double d = (cola_c - cv) * ic;
                    acc[0] += d * (double)v.x;
                    acc[1] += d * (double)v.y;
                }
            }
        }
    } else {
    // uniform bases + 32-bit lane offsets (scalar-base addressing: one offset register per load instead of a 64-bit address)
    const char *xh = reinterpret_cast<const char *>(x), *xt = xh + M * (int64_t)H * (CPLX ? 8 : 4);
    for (int base = 0; base < N; base += WG * NPT) {
        double slr[NPT], sli[NPT];
        float wn[NPT];
        cf eh[NPT][E], et[NPT][E];
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const unsigned nidx = (unsigned)(base + (int)threadIdx.x + WG * t);
            const bool on = nidx < (unsigned)N;
            const unsigned nc = on ? nidx : 0u;
            const unsigned q = nc >> hs, j = nc & (unsigned)(H - 1);
            slr[t] = ld_sc1(Sl + 2u * j);
            sli[t] = ld_sc1(Sl + 2u * j + 1u);
            ak[t] = ld_sc1(Acol + nc);
            wn[t] = win[nc];
#pragma unroll
            for (int e = 0; e < E; ++e) {           // edge blocks of c[n]: b = q + e <= r - 2 (head), b = M + q + e <= M + r - 2 (tail)
                const bool he = on && (int)q + e <= r - 2;
                const unsigned off = he ? ((q + (unsigned)e) << hs) + j : 0u;
                const cf vh = load_sample(xh, off, CPLX), vt = load_sample(xt, off, CPLX);
                eh[t][e] = he ? vh - mu : mk(0.f, 0.f);
                et[t][e] = he ? vt - mu : mk(0.f, 0.f);
            }
        }
        __builtin_amdgcn_sched_barrier(0);          // (all loads issued above; consumed one bin at a time below)
        // e^{-i theta_n}, theta_n = 2 pi n / N, for n = base + tid, then rotated by the step e^{-2 pi i WG / N} from bin to bin
        double c1, s1;
        sincospi(-2.0 * (double)(base + (int)threadIdx.x) / (double)N, &s1, &c1);
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int nidx = base + (int)threadIdx.x + WG * t;
            if (nidx < N) {
                const int q = nidx >> hs;
                double a = slr[t], b = sli[t];
                if (q == 0) {                     // every j once: the block sums, and below the head blocks i < (r - 1) H
                    acc[0] += a;
                    acc[1] += b;
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if (q == 0) {
                        acc[0] += (double)eh[t][e].x;
                        acc[1] += (double)eh[t][e].y;
                    }
                    a += (double)eh[t][e].x - (double)et[t][e].x;
                    b += (double)eh[t][e].y - (double)et[t][e].y;
                }
                a *= (double)wn[t];
                b *= (double)wn[t];
                acc[2 + 6] += a;
                acc[3 + 6] += b;
                double pr = 1.0, pi_ = 0.0;
#pragma unroll
                for (int ks = 1; ks <= 3; ++ks) {
                    const double tr_ = pr * c1 - pi_ * s1, ti_ = pr * s1 + pi_ * c1;      // e^{-i ks theta}
                    pr = tr_;
                    pi_ = ti_;
                    acc[2 + 2 * (3 + ks)] += a * pr - b * pi_;
                    acc[3 + 2 * (3 + ks)] += a * pi_ + b * pr;
                    acc[2 + 2 * (3 - ks)] += a * pr + b * pi_;                          // the conjugate phase for -ks
                    acc[3 + 2 * (3 - ks)] += b * pr - a * pi_;
                }
            }
            const double nc1 = c1 * step_c - s1 * step_s, ns1 = c1 * step_s + s1 * step_c;
            c1 = nc1;
            s1 = ns1;
        }
    }
    }
    // across the wave: the mean's total in double (shuffles), the lobe sums in float through DPP (no LDS round trips; they enter
    // the spectrum multiplied by d = mean - mu0: float32 is ample); across the waves: LDS
    acc[0] = wave_sum64d(acc[0]);
    acc[1] = wave_sum64d(acc[1]);
#pragma unroll
    for (int q = 2; q < 16; ++q) acc[q] = (double)wave_sum64((float)acc[q]);
    __syncthreads();                               // (phase 1's use of sh is over in every wave)
    if (ln == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) sh[wv][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) a += sh[w][threadIdx.x];
        tot_sh[threadIdx.x] = a;
    }
    __syncthreads();
    // (LOBEB: the samples' sum = ragged end + edges / c [both in slot 0, 1] + B[0] / c)
    const double tot_r = tot_sh[0] + (LOBEB ? tot_sh[2 + 6] / cola_c : 0.0), tot_i = tot_sh[1] + (LOBEB ? tot_sh[3 + 6] / cola_c : 0.0);
    double dr, di;
    if (!EXPORT && mean_in) {
        dr = mean_in[0] - (double)trend[0];
        di = mean_in[1] - (double)trend[1];
    } else {
        dr = tot_r / (double)nmean;
        di = tot_i / (double)nmean;
    }
    const double mr = (double)mu.x, mi = (double)mu.y;
    const bool one_chunk = !LOBEB && N <= WG * NPT;
    for (int base = 0; base < N; base += WG * NPT) {
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int k = base + (int)threadIdx.x + WG * t;
            if (k >= N) continue;
            double a = one_chunk ? ak[t] : ld_sc1(Acol + k);
            if (sym) a = 0.5 * (a + ld_sc1(Acol + ((N - k) & (N - 1))));          // real-pair transforms: |Z|^2 symmetrised
            const int ks = k <= lb.K ? k : (k >= N - lb.K ? k - N : 99);
            double Br = 0.0, Bi = 0.0, wr = 0.0, wi = 0.0;
            if (ks != 99) {                                                      // (2 K + 1 bins of the whole block)
                Br = tot_sh[2 + 2 * (ks + 3)];
                Bi = tot_sh[3 + 2 * (ks + 3)];
#pragma unroll
                for (int u = 0; u < 7; ++u)
                    if (u == ks + 3) {
                        wr = lb.wr[u];
                        wi = lb.wi[u];
                    }
            }
            if constexpr (EXPORT) {
                out[k] = a;
                out[N + 2 * k] = Br;
                out[N + 2 * k + 1] = Bi;
                out[3 * N + 2 * k] = mr * Br + mi * Bi;          // conj(mu0) B
                out[3 * N + 2 * k + 1] = mr * Bi - mi * Br;
            } else {
                const int slot = bin_slot(k, N, sided);
                if (slot >= 0) {
                    const double er = dr * wr - di * wi, ei = dr * wi + di * wr;       // d W[k]
                    const double p = a - 2.0 * (er * Br + ei * Bi) + (double)M * (er * er + ei * ei);
                    out[slot] = p * scale * (bin_doubled(k, N, sided) ? 2.0 : 1.0);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        if constexpr (EXPORT) {
            double *sc = out + 5 * (int64_t)N;
            sc[0] = (double)M * mr;
            sc[1] = (double)M * mi;
            sc[2] = (double)M * (mr * mr + mi * mi);
            sc[3] = tot_r + (double)nmean * mr;
            sc[4] = tot_i + (double)nmean * mi;
            sc[5] = (double)M;
            sc[6] = (double)nmean;
            sc[7] = 0.0;
        }
        // ready for the next launch (plain stores: the atomic form cost 1.6 us at the kernel boundary)
    }
    if (threadIdx.x < 9) ticket[16 * threadIdx.x] = 0u;
    if constexpr (EXPORT) {
        if (prev.st) {          // k_op_apply's arithmetic on the previous step's summed state (same N)
            const double *st = prev.st;
            const double *sc = st + 5 * (int64_t)N;
            const double Mt = sc[5], nt = sc[6];
            const double gr = sc[3] / nt, gi = sc[4] / nt;
            const double sq = (gr * gr + gi * gi) * Mt - 2.0 * (gr * sc[0] + gi * sc[1]) + sc[2];
            for (int k = threadIdx.x; k < N; k += WG) {
                const int slot = bin_slot(k, N, prev.sided);
                if (slot < 0) continue;
                const double b_r = st[N + 2 * k], b_i = st[N + 2 * k + 1], cr = st[3 * N + 2 * k], ci = st[3 * N + 2 * k + 1];
                const double d_r = gr * b_r + gi * b_i - cr, d_i = gr * b_i - gi * b_r - ci;            // conj(mu) B - C
                const double wr = prev.Wf[k].x, wi = prev.Wf[k].y;
                const double p = st[k] - 2.0 * (wr * d_r + wi * d_i) + (wr * wr + wi * wi) * sq;
                prev.out[slot] = p * prev.scale * (bin_doubled(k, N, prev.sided) ? 2.0 : 1.0);
            }
        }
    }
}

bool welch_carry_eligible(const Xf &xf, int hop, bool lin) {
    if (xf.blue || lin || xf.L < 256 || xf.L > 8192) return false;
    const int T = xf.L / 16;
    if (hop % T != 0) return false;
    const int shift = hop / T;
    return shift == 4 || shift == 8 || shift == 16;
}

template <int N, bool CPLX>
static bool try_carry(LaunchCtx c, const void *x, const float *win, int hop, int64_t nframes, const float *trend,
                      const Xf &xf, float *partial, const RunPart &rp, cf *spartial) {
    using C = WgCfg<N>;
    const int shift = hop / C::T;
    constexpr bool HINT = N >= 512;       // see k_welch_carry / k_welch_carry_nh
    const size_t lds = C::lds_bytes(1);
#define CARRY_(S)                                                                                     \
    case S:                                                                                           \
        if constexpr (HINT) {                                                                         \
            if (spartial) hipLaunchKernelGGL((k_welch_carry<N, CPLX, S, true>), dim3(rp.blocks), dim3(C::WG), lds, c.stream, \
                                             x, win, nframes, rp.fpg, trend, xf.tb, partial, spartial); \
            else hipLaunchKernelGGL((k_welch_carry<N, CPLX, S, false>), dim3(rp.blocks), dim3(C::WG), lds, c.stream, \
                                    x, win, nframes, rp.fpg, trend, xf.tb, partial, spartial);        \
        } else {                                                                                      \
            if (spartial) hipLaunchKernelGGL((k_welch_carry_nh<N, CPLX, S, true>), dim3(rp.blocks), dim3(C::WG), lds, c.stream, \
                                             x, win, nframes, rp.fpg, trend, xf.tb, partial, spartial); \
            else hipLaunchKernelGGL((k_welch_carry_nh<N, CPLX, S, false>), dim3(rp.blocks), dim3(C::WG), lds, c.stream, \
                                    x, win, nframes, rp.fpg, trend, xf.tb, partial, spartial);        \
        }                                                                                             \
        return true;
    switch (shift) {
        CARRY_(4) CARRY_(8) CARRY_(16)
        default: return false;
    }
#undef CARRY_
}

// centre-of-gravity moments per frame on the carry kernel (power-of-two nfft, hop = nfft/4, /2 or nfft; constant detrend;
// every bin)
template <int N, bool CPLX>
static bool try_carry_cog(LaunchCtx c, const void *x, const float *win, int hop, int64_t nframes, const float *trend,
                          const Xf &xf, cf *cog, const RunPart &rp) {
    using C = WgCfg<N>;
    const int shift = hop / C::T;
#define COG_(S)                                                                                       \
    case S:                                                                                           \
        hipLaunchKernelGGL((k_welch_carry_cog<N, CPLX, S>), dim3(rp.blocks), dim3(C::WG), C::lds_bytes(1), \
                           c.stream, x, win, nframes, rp.fpg, trend, xf.tb, cog);                    \
        return true;
    switch (shift) {
        COG_(4) COG_(8) COG_(16)
        default: return false;
    }
#undef COG_
}

// returns 1 when the shape is not eligible (the caller falls back to the generic frame kernel)
int launch_cog_carry(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                     const Xf &xf, cf *cog, const RunPart &rp, int klo, int khi) {
    if (!welch_carry_eligible(xf, hop, false)) return 1;
    if (klo > 0 || khi < xf.L / 2) return 1;          // the streaming kernel weighs every bin; a band goes the generic way
    bool done = false;
#define TRY_(NN)                                                                                      \
    case NN:                                                                                          \
        done = cplx ? try_carry_cog<NN, true>(c, x, win, hop, nframes, trend, xf, cog, rp)  \
                    : try_carry_cog<NN, false>(c, x, win, hop, nframes, trend, xf, cog, rp); \
        break;
    switch (xf.L) {
        TRY_(256) TRY_(512) TRY_(1024) TRY_(2048) TRY_(4096) TRY_(8192)
        default: break;
    }
#undef TRY_
    return done ? 0 : 1;
}

int launch_welch(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                 bool lin, const Xf &xf, float *partial, const RunPart &rp, bool allow_carry, cf *spartial,
                 const char **kname, int segmean) {
    if (kname) *kname = "k_welch";
    if (segmean) allow_carry = false;        // per-segment detrend exists only in the generic kernel
    if (allow_carry && welch_carry_eligible(xf, hop, lin)) {
        bool done = false;
#define TRY_(NN)                                                                                      \
    case NN:                                                                                          \
        done = cplx ? try_carry<NN, true>(c, x, win, hop, nframes, trend, xf, partial, rp, spartial)  \
                    : try_carry<NN, false>(c, x, win, hop, nframes, trend, xf, partial, rp, spartial); \
        break;
        switch (xf.L) {
            TRY_(256) TRY_(512) TRY_(1024) TRY_(2048) TRY_(4096) TRY_(8192)
            default: break;
        }
#undef TRY_
        if (done) {
            if (kname) *kname = spartial ? "k_welch_carry(onepass)" : "k_welch_carry";
            return 0;
        }
    }
    if (spartial) return -1;      // one-pass accumulation exists only in the carry kernel
#define M_(XT)                                                                                        \
    if (cplx) {                                                                                       \
        if (lin) hipLaunchKernelGGL((k_welch<XT, true, true>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), \
                                    c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, segmean);   \
        else hipLaunchKernelGGL((k_welch<XT, true, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), \
                                c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, segmean);       \
    } else {                                                                                          \
        if (lin) hipLaunchKernelGGL((k_welch<XT, false, true>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), \
                                    c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, segmean);   \
        else hipLaunchKernelGGL((k_welch<XT, false, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), \
                                c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, partial, segmean);       \
    }
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

int launch_welch_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int sided, double scale, double *out,
                        int sym) {
    const int n = xf.tb.n;
    hipLaunchKernelGGL(k_welch_finish, dim3((n + SP_FIN_BINS - 1) / SP_FIN_BINS), dim3(SP_FIN_BINS * SP_FIN_SLICES), 0,
                       c.stream, partial, G, xf.L, n, sided, scale, out, sym);
    return 0;
}

// smallest power-of-two transform that uses the hinted entry point of k_welch_rp.
// Round 3: 4096 (was 2048).  The round-1 finding "the 2-wave hint is 13 % faster at 2048 points" was an artefact of the run
// partition: 4 groups per CU against the 3 workgroups the unhinted kernel keeps resident = a last round a third full.  With the
// partition a multiple of the residency (welch_rp_groups_per_cu) the plain form wins: 0.281 -> 0.252 ms at 2^26 samples, nfft 2048,
// 75 % overlap.
#define SP_RP_HINT_MIN 4096
int resident_per_cu(const void *fn, int threads, size_t lds_bytes) {
    struct Key {
        const void *fn;
        int threads;
        size_t lds;
        bool operator<(const Key &o) const { return fn != o.fn ? fn < o.fn : (threads != o.threads ? threads < o.threads : lds < o.lds); }
    };
    static std::mutex mu;
    static std::map<Key, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    const Key k{fn, threads, lds_bytes};
    auto it = cache.find(k);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds_bytes) != hipSuccess || nb < 1) nb = 0;
    cache[k] = nb;
    return nb;
}
int welch_rp_groups_per_cu(const Xf &xf, bool lin) {
    int res = 0;
#define M_(XT)                                                                                        \
    if constexpr (XT::EXACT && XT::L >= SP_RP_HINT_MIN) {                                             \
        res = lin ? resident_per_cu((const void *)k_welch_rp<XT, true>, XT::C::WG, XT::C::lds_bytes(1))   \
                  : resident_per_cu((const void *)k_welch_rp_h<XT, false>, XT::C::WG, XT::C::lds_bytes(1)); \
    } else {                                                                                          \
        res = lin ? resident_per_cu((const void *)k_welch_rp<XT, true>, XT::C::WG, XT::C::lds_bytes(1))   \
                  : resident_per_cu((const void *)k_welch_rp<XT, false>, XT::C::WG, XT::C::lds_bytes(1)); \
    }
    SP_DISPATCH_X(xf, M_)
#undef M_
    // 1 or 2 resident: 4 per CU as before (whole rounds); 3: 3; more: one round
    if (res <= 0) return 4;
    if (res <= 2) return 4;
    return res > 8 ? 8 : res;
}
// real input, two frames per transform (power only); rp partitions PAIRS of frames
int launch_welch_rp(LaunchCtx c, const float *x, const float *win, int hop, int64_t nframes, const float *trend, bool lin,
                    const Xf &xf, float *partial, const RunPart &rp) {
#define M_(XT)                                                                                        \
    if constexpr (XT::EXACT && XT::L >= SP_RP_HINT_MIN) {                                             \
        /* (not for the linear-detrend variants: the hint makes them spill) */                        \
        if (lin) hipLaunchKernelGGL((k_welch_rp<XT, true>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                                    x, win, hop, nframes, rp.fpg, trend, xf.tb, partial);             \
        else hipLaunchKernelGGL((k_welch_rp_h<XT, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                                x, win, hop, nframes, rp.fpg, trend, xf.tb, partial);                 \
    } else {                                                                                          \
        if (lin) hipLaunchKernelGGL((k_welch_rp<XT, true>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                                    x, win, hop, nframes, rp.fpg, trend, xf.tb, partial);             \
        else hipLaunchKernelGGL((k_welch_rp<XT, false>), dim3(rp.blocks), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, \
                                x, win, hop, nframes, rp.fpg, trend, xf.tb, partial);                 \
    }
    SP_DISPATCH_X(xf, M_)
#undef M_
    return 0;
}

// ---- one-pass detrend epilogue: 4 launches (estimate | main kernel | two reductions | totals) + 1 at finish -------
int launch_op_estimate(LaunchCtx c, const void *x, bool cplx, int64_t nsig, double *, float *trend) {
    if (cplx) hipLaunchKernelGGL((k_op_estimate<true>), dim3(1), dim3(1024), 0, c.stream, x, nsig, trend);
    else hipLaunchKernelGGL((k_op_estimate<false>), dim3(1), dim3(1024), 0, c.stream, x, nsig, trend);
    return 0;
}

// A[k] raw sums, Sl[j] block sums, tot = sum_{i<nmean}(x - mu0), local delta, plain sample sum
int launch_op_reduce(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *partial, const cf *spartial,
                     int64_t G, const Xf &xf, int hop, int64_t nframes, int64_t nmean, OnePass st, double *sum_out) {
    const int N = xf.L, H = hop, r = N / H;
    hipLaunchKernelGGL(k_op_colsums, dim3((N + 31) / 32 + (2 * H + 31) / 32), dim3(1024), 0, c.stream, partial, N, st.A,
                       reinterpret_cast<const float *>(spartial), 2 * H, st.Sl, G);
    if (!sum_out) return 0;          // single-call path: k_op_finish derives the shard mean itself
    if (cplx) hipLaunchKernelGGL((k_op_total<true>), dim3(1), dim3(1024), 0, c.stream, x, trend, st.Sl, H, r, nframes, nmean, st.tot, st.dlt, sum_out);
    else hipLaunchKernelGGL((k_op_total<false>), dim3(1), dim3(1024), 0, c.stream, x, trend, st.Sl, H, r, nframes, nmean, st.tot, st.dlt, sum_out);
    return 0;
}

// c -> B = FFT(w c) -> combine, one workgroup.  export_state: write the shard's additive state instead (out = state)
int launch_op_finish(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *win, OnePass st,
                     const double *mean_in, int64_t nmean, const Xf &xf, int hop, int64_t nframes, cf *, const cf *Wf,
                     int sided, double scale, double *out, bool export_state) {
    const int H = hop, r = xf.L / H;
#define FIN_(NN)                                                                                      \
    case NN:                                                                                          \
        if (export_state) {                                                                           \
            if (cplx)                                                                                 \
                hipLaunchKernelGGL((k_op_finish<NN, true, true>), dim3(1), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1), c.stream, \
                                   x, trend, win, st.Sl, st.A, Wf, st.dlt, mean_in, H, r, nframes, nmean, sided, scale, xf.tb, out, st.sym); \
            else                                                                                      \
                hipLaunchKernelGGL((k_op_finish<NN, false, true>), dim3(1), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1), c.stream, \
                                   x, trend, win, st.Sl, st.A, Wf, st.dlt, mean_in, H, r, nframes, nmean, sided, scale, xf.tb, out, st.sym); \
        } else if (cplx)                                                                              \
            hipLaunchKernelGGL((k_op_finish<NN, true>), dim3(1), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1), c.stream, x, \
                               trend, win, st.Sl, st.A, Wf, st.dlt, mean_in, H, r, nframes, nmean, sided, scale, xf.tb, out, st.sym); \
        else                                                                                          \
            hipLaunchKernelGGL((k_op_finish<NN, false>), dim3(1), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1), c.stream, x, \
                               trend, win, st.Sl, st.A, Wf, st.dlt, mean_in, H, r, nframes, nmean, sided, scale, xf.tb, out, st.sym); \
        break;
    switch (xf.L) {
        FIN_(256) FIN_(512) FIN_(1024) FIN_(2048) FIN_(4096) FIN_(8192)
        default: return -1;
    }
#undef FIN_
    return 0;
}

int launch_op_fused(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *win, const float *partial,
                    const cf *spartial, int64_t G, int n, int hop, int64_t nframes, int64_t nmean, OnePass st, unsigned *ticket,
                    CogLobe lb, const double *mean_in, int sided, double scale, double *out, bool export_state, OpPrev prev, bool light,
                    double cola_c) {
    if (n % hop != 0 || n / hop > 4 || (hop & (hop - 1)) != 0 || n % 32 != 0 || (2 * hop) % 32 != 0 || lb.K < 0 || lb.K > 3 || n < 2 * lb.K + 2)
        return -1;
    const bool lobeb = cola_c > 0.0;             // the main kernel left lobe sums (k_welch_pipe mode 9), not block sums
    const int wg = light ? SP_OPF_WG_LIGHT : SP_OPF_WG;
    const dim3 grid(n / 32 + (lobeb ? 0 : (2 * hop) / 32)), block(wg);
    const double ang = -2.0 * M_PI * (double)wg / (double)n;                   // the bin-to-bin rotation of the last block's twiddles
    const double step_c = cos(ang), step_s = sin(ang);
#define FUSED_(CP, EX, EE, LT, LB)                                                                     \
    hipLaunchKernelGGL((k_op_fused<CP, EX, EE, LT, LB>), grid, block, 0, c.stream, partial, n, st.A, reinterpret_cast<const float *>(spartial), \
                       hop, st.Sl, G, ticket, x, trend, win, lb, mean_in, nframes, nmean, sided, scale, out, st.sym, prev, step_c, step_s, cola_c)
#define FUSED_E_(CP, EX)                                                                               \
    {                                                                                                 \
        if (lobeb) {                                                                                  \
            if (light) FUSED_(CP, EX, 1, true, true); else FUSED_(CP, EX, 1, false, true);             \
        } else if (light) {                                                                           \
            if (n / hop <= 2) FUSED_(CP, EX, 1, true, false); else FUSED_(CP, EX, 3, true, false);     \
        } else {                                                                                      \
            if (n / hop <= 2) FUSED_(CP, EX, 1, false, false); else FUSED_(CP, EX, 3, false, false);   \
        }                                                                                             \
    }
    if (cplx) {
        if (export_state) FUSED_E_(true, true) else FUSED_E_(true, false)
    } else {
        if (export_state) FUSED_E_(false, true) else FUSED_E_(false, false)
    }
#undef FUSED_E_
#undef FUSED_
    return 0;
}

int launch_op_apply(LaunchCtx c, const double *state, const cf *Wf, int n, int sided, double scale, double *out,
                    const double *mean) {
    hipLaunchKernelGGL(k_op_apply, dim3((n + 255) / 256), dim3(256), 0, c.stream, state, Wf, n, sided, scale, out, mean);
    return 0;
}

// one-pass mean detrend of MANY real channels (the CSD matrix on packed pair spectra): per channel, from the block sums Sl and
// the mean estimate in its trend record, the state of k_op_finish<EXPORT>: B = sum_g X_g, the plain sample sum, ... (5 L + 8
// doubles per channel)
int launch_op_finish_channels(LaunchCtx c, const void *x, int64_t x_cs, int nch, const float *trend, const float *win,
                              const double *Sl, const cf *Wf, int hop, int64_t nframes, int64_t nmean, const Xf &xf, double *out,
                              bool cplx) {
    if (xf.L != 4096) return -1;
    const int H = hop, r = xf.L / H;
    if (cplx) {
        hipLaunchKernelGGL((k_op_finish<4096, true, true>), dim3(nch), dim3(WgCfg<4096>::WG), WgCfg<4096>::lds_bytes(1), c.stream, x,
                           trend, win, Sl, Sl, Wf, (const double *)nullptr, (const double *)nullptr, H, r, nframes, nmean, 2, 1.0, xf.tb,
                           out, 0, x_cs, (int64_t)2 * H, (int64_t)5 * xf.L + 8);
        return 0;
    }
    hipLaunchKernelGGL((k_op_finish<4096, false, true>), dim3(nch), dim3(WgCfg<4096>::WG), WgCfg<4096>::lds_bytes(1), c.stream,
                       x, trend, win, Sl, Sl /* A: unused by the consumers of this state */, Wf, (const double *)nullptr,
                       (const double *)nullptr, H, r, nframes, nmean, 2, 1.0, xf.tb, out, 0, x_cs, (int64_t)2 * H,
                       (int64_t)5 * xf.L + 8);
    return 0;
}

}   // namespace sp
