// k_sos.hip -- cascades of K <= 8 second-order sections  y = scipy.signal.sosfilt(sos, x)  on nrows independent float32
// rows, and the two passes of a zero-phase sosfiltfilt, evaluated exactly.  The blocked scan of k_iir.hip generalised to
// a cascade: every section is in transposed direct form II (scipy's sosfilt convention)
//
//   y = b0 v + z1,   z1' = b1 v - a1 y + z2,   z2' = b2 v - a2 y        (v: the section's input, y: its output)
//
// so the cascade state is s = (z1, z2) of every section, S = 2K float64 values, and a chunk run "from rest" starts at s = 0
// with no neighbour samples.  A run of C samples started from s ends in M_C s + f (f: its end state from rest) and its
// last section's outputs are y_rest[j] + H[j] . s.  Per pass, three launches (k_iir.hip's shape, one row per grid row):
//   k_sos_tile<K, false>   per tile: end state from rest (in-tile log-step scan of the chunk end states)   reads x
//   k_sos_chain<K>         per row: incoming state of every tile from the row's initial state; one workgroup per row
//   k_sos_tile<K, true>    per tile: outputs with the right incoming state (+ the row's final state zf)   reads x, writes y
// = 12 B per sample.  The plan (coefficients, steady state, H, the scan powers of M_C and of the tile map) is a device
// table indexed only by compile-time positions, so every load of it is wave-uniform (scalar).
//
// Where a pass reads its samples from is an index map (SosIO), not a copy: the forward pass of sosfiltfilt reads the
// odd / even / constant extension of a row straight from x, the reverse pass reads the forward output backwards.
#include "launch.h"

#include <limits.h>
#include <vector>

namespace sp {

// samples per thread and threads per tile (compile-time; -D overrides build the A/B variants of tools/sos_ab.sh)
#ifndef SP_SOS_C
#define SP_SOS_C 64
#endif
#ifndef SP_SOS_WG
#define SP_SOS_WG 128
#endif
#define SP_SOS_TILE (SP_SOS_C * SP_SOS_WG)
__host__ __device__ constexpr int sos_log2(int v) { return v <= 1 ? 0 : 1 + sos_log2(v / 2); }
#define SP_SOS_LOGWG sos_log2(SP_SOS_WG)

// chain workgroup: its scan keeps S doubles per thread in LDS (<= 48 KiB)
__host__ __device__ constexpr int sos_chain_threads(int K) { return K <= 3 ? 1024 : K <= 6 ? 512 : 256; }
__host__ __device__ constexpr int sos_chain_levels(int K) { return K <= 3 ? 10 : K <= 6 ? 9 : 8; }

// plan layout in doubles (S = 2K); the same formulas on host and device
__host__ __device__ constexpr int sos_o_zss() { return 5 * SP_SOS_MAXK; }                      // [K][5] b0 b1 b2 a1 a2 first
__host__ __device__ constexpr int sos_o_h() { return sos_o_zss() + 2 * SP_SOS_MAXK; }          // zss[S]: sosfilt_zi
__host__ __device__ constexpr int sos_o_pw(int S) { return sos_o_h() + SP_SOS_C * S; }         // H[C][S]
__host__ __device__ constexpr int sos_o_mt(int S) { return sos_o_pw(S) + SP_SOS_LOGWG * S * S; }   // M_C^(2^d)[8][S][S]
__host__ __device__ constexpr int sos_o_cpw(int S) { return sos_o_mt(S) + S * S; }             // M_tile[S][S]
__host__ __device__ constexpr int sos_o_end(int S) { return sos_o_cpw(S) + 10 * S * S; }       // (M_tile^per)^(2^d)[10][S][S]

__device__ __forceinline__ int sos_pidx(int i) { return i + i / SP_SOS_C; }   // one pad word per chunk: chunk-strided reads

// tile states of a row (end states from rest, incoming states): S * per * CT doubles, component-major and ordered so that
// chain thread i's j-th tile (k = i per + j) is slot [s][j][i] -- the chain's loads and stores are coalesced across threads
__host__ __device__ __forceinline__ int64_t sos_tslot(int64_t k, int s, int per, int CT) {
    const int64_t i = k / per;
    return ((int64_t)s * per + (k - i * per)) * CT + i;
}

// v <- m v, m row major [S][S] (a wave-uniform table)
template <int S> __device__ __forceinline__ void sos_mv(const double *__restrict__ m, double (&v)[S]) {
    double r[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) a = fma(m[i * S + j], v[j], a);
        r[i] = a;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) v[i] = r[i];
}

// one sample through the cascade; returns the last section's output
template <int K> __device__ __forceinline__ double sos_step(const double *__restrict__ cf, double (&z)[2 * K], double v) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double y = fma(cf[5 * k], v, z[2 * k]);
        z[2 * k] = fma(cf[5 * k + 1], v, fma(-cf[5 * k + 3], y, z[2 * k + 1]));
        z[2 * k + 1] = fma(cf[5 * k + 2], v, -cf[5 * k + 4] * y);
        v = y;
    }
    return v;
}

// sample e (0 <= e) of the pass over row xr; 0 past the pass
__device__ __forceinline__ float sos_src(const SosIO &io, const float *__restrict__ xr, int64_t e) {
    if (e >= io.len) return 0.f;
    const int64_t t = io.rev ? io.len - 1 - e : e - io.pad;
    if (t < 0) {                          // left extension (scipy odd_ext / even_ext / const_ext), 1 <= -t <= pad < n
        const float a = xr[0];
        return io.padtype == 1 ? 2.f * a - xr[-t] : io.padtype == 2 ? xr[-t] : a;
    }
    if (t >= io.n) {                      // right extension
        const int64_t k = t - (io.n - 1);
        const float a = xr[io.n - 1];
        return io.padtype == 1 ? 2.f * a - xr[io.n - 1 - k] : io.padtype == 2 ? xr[io.n - 1 - k] : a;
    }
    return xr[t];
}

template <int K, bool APPLY>
static __global__ __launch_bounds__(SP_SOS_WG) void k_sos_tile(SosIO io, const double *__restrict__ plan, int64_t nt,
                                                               int per, const double *__restrict__ tile_in,
                                                               double *__restrict__ tile_end /*[rows][S][per][CT]*/,
                                                               double *__restrict__ zf /*[rows][S] or null*/) {
    constexpr int S = 2 * K, T = SP_SOS_TILE, WG = SP_SOS_WG;
    constexpr int XSF = T + T / SP_SOS_C + 8;                 // floats of the staged tile
    constexpr int SD = (XSF + 1) / 2 > S * WG ? (XSF + 1) / 2 : S * WG;
    __shared__ double smem[SD];                              // the staged tile, or (between the passes over it) the scan slots
    float *xs = reinterpret_cast<float *>(smem);
    double *st = smem;
    const int64_t row = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * T;
    const int tid = threadIdx.x;
    const float *xr = io.x + row * io.x_ld;

    // stage the tile.  When it is one contiguous run of the source row (every tile but the edges): 16-byte loads from the
    // run's start rounded down to 16 bytes, `sh` samples early (one more float4 at the end), placed back by the shift
    int64_t p0 = 0;
    int sh = 0;
    bool fast = false;
    if (t0 + T <= io.len) {
        p0 = io.rev ? io.len - t0 - T : t0 - io.pad;
        if (p0 >= 0 && p0 + T <= io.n) {
            sh = (int)(((uintptr_t)(xr + p0) >> 2) & 3);
            fast = sh == 0 || (p0 - sh + T + 4 <= io.n && p0 - sh >= 0);
        }
    }
    if (fast) {
        const float4 *x4 = reinterpret_cast<const float4 *>(xr + p0 - sh);
        float4 r[T / 4 / WG];
#pragma unroll
        for (int k = 0; k < T / 4 / WG; ++k) r[k] = x4[tid + WG * k];
        float4 rt = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sh != 0 && tid == 0) rt = x4[T / 4];
        auto put = [&](int m, float v) {                       // m: sample of the aligned run -> its place in the tile
            const int l = m - sh;
            if (l >= 0 && l < T) xs[sos_pidx(io.rev ? T - 1 - l : l)] = v;
        };
#pragma unroll
        for (int k = 0; k < T / 4 / WG; ++k) {
            const int m = 4 * (tid + WG * k);
            put(m, r[k].x);
            put(m + 1, r[k].y);
            put(m + 2, r[k].z);
            put(m + 3, r[k].w);
        }
        if (sh != 0 && tid == 0) {
            put(T, rt.x);
            put(T + 1, rt.y);
            put(T + 2, rt.z);
            put(T + 3, rt.w);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < T; i += WG) xs[sos_pidx(i)] = sos_src(io, xr, t0 + i);
    }
    __syncthreads();

    // the chunk from rest
    const double *cf = plan;
    const int c0 = tid * SP_SOS_C;
    double z[S];
#pragma unroll
    for (int s = 0; s < S; ++s) z[s] = 0.0;
    double yl[SP_SOS_C];
#pragma unroll
    for (int j = 0; j < SP_SOS_C; ++j) {
        const double v = sos_step<K>(cf, z, (double)xs[sos_pidx(c0 + j)]);
        if constexpr (APPLY) yl[j] = v;
    }
    __syncthreads();                                          // the tile's LDS becomes the scan slots

    // inclusive scan of the chunk end states: f_i <- f_i + M_C^(2^d) f_{i - 2^d}
#pragma unroll
    for (int d = 0; d < SP_SOS_LOGWG; ++d) {
#pragma unroll
        for (int s = 0; s < S; ++s) st[s * WG + tid] = z[s];
        __syncthreads();
        if (tid >= (1 << d)) {
            double q[S];
#pragma unroll
            for (int s = 0; s < S; ++s) q[s] = st[s * WG + tid - (1 << d)];
            sos_mv<S>(plan + sos_o_pw(S) + d * S * S, q);
#pragma unroll
            for (int s = 0; s < S; ++s) z[s] += q[s];
        }
        __syncthreads();
    }
    constexpr int CT = sos_chain_threads(K);
    const int64_t rb = row * (int64_t)S * per * CT;
    if (!APPLY) {
        if (tid == WG - 1) {
#pragma unroll
            for (int s = 0; s < S; ++s) tile_end[rb + sos_tslot(blockIdx.x, s, per, CT)] = z[s];
        }
        return;
    }
    // incoming state of this chunk: the chunks before it from rest + M_C^tid (tile's incoming state), tid in binary
#pragma unroll
    for (int s = 0; s < S; ++s) st[s * WG + tid] = z[s];
    __syncthreads();
    double sp[S], tp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        sp[s] = tid > 0 ? st[s * WG + tid - 1] : 0.0;
        tp[s] = tile_in[rb + sos_tslot(blockIdx.x, s, per, CT)];
    }
#pragma unroll
    for (int d = 0; d < SP_SOS_LOGWG; ++d)
        if (tid & (1 << d)) sos_mv<S>(plan + sos_o_pw(S) + d * S * S, tp);
#pragma unroll
    for (int s = 0; s < S; ++s) sp[s] += tp[s];
    __syncthreads();

    // the row's final state: the chunk holding the pass's last sample runs it again from its incoming state
    if (zf != nullptr) {
        const int64_t last = io.len - 1 - t0 - c0;
        if (last >= 0 && last < SP_SOS_C) {
            double w[S];
#pragma unroll
            for (int s = 0; s < S; ++s) w[s] = sp[s];
            for (int j = 0; j <= (int)last; ++j) (void)sos_step<K>(cf, w, (double)sos_src(io, xr, t0 + c0 + j));
#pragma unroll
            for (int s = 0; s < S; ++s) zf[row * S + s] = w[s];
        }
    }

    // outputs: rest response + homogeneous response to sp, staged through the LDS for coalesced stores
    const double *H = plan + sos_o_h();
#pragma unroll
    for (int j = 0; j < SP_SOS_C; ++j) {
        double o = yl[j];
#pragma unroll
        for (int s = 0; s < S; ++s) o = fma(H[j * S + s], sp[s], o);
        xs[sos_pidx(c0 + j)] = (float)o;
    }
    __syncthreads();
    // pass sample e lands at q = (rev ? len-1-e : e) - out_off of the output row when 0 <= q < out_n
    float *yr = io.y + row * io.y_ld;
    int64_t q0 = 0;
    bool run = false, vst = false;
    if (t0 + T <= io.len) {
        q0 = (io.rev ? io.len - t0 - T : t0) - io.out_off;
        run = q0 >= 0 && q0 + T <= io.out_n;
        vst = run && (((uintptr_t)(yr + q0)) & 15) == 0;
    }
    if (vst) {
        float4 *y4 = reinterpret_cast<float4 *>(yr + q0);
#pragma unroll
        for (int k = 0; k < T / 4 / WG; ++k) {
            const int i = 4 * (tid + WG * k);
            y4[tid + WG * k] = io.rev ? make_float4(xs[sos_pidx(T - 1 - i)], xs[sos_pidx(T - 2 - i)], xs[sos_pidx(T - 3 - i)],
                                                    xs[sos_pidx(T - 4 - i)])
                                      : make_float4(xs[sos_pidx(i)], xs[sos_pidx(i + 1)], xs[sos_pidx(i + 2)], xs[sos_pidx(i + 3)]);
        }
    } else if (run) {                                        // contiguous but not 16-byte aligned: 4-byte stores
#pragma unroll 8
        for (int m = tid; m < T; m += WG) yr[q0 + m] = xs[sos_pidx(io.rev ? T - 1 - m : m)];
    } else {
#pragma unroll 4
        for (int i = tid; i < T; i += WG) {
            const int64_t e = t0 + i;
            if (e >= io.len) break;
            const int64_t q = (io.rev ? io.len - 1 - e : e) - io.out_off;
            if (q >= 0 && q < io.out_n) yr[q] = xs[sos_pidx(i)];
        }
    }
}

// incoming state of every tile of a row from the tiles' from-rest end states: s_{k+1} = M_tile s_k + f_k, s_0 = the row's
// initial state (zmode 0: zero, 1: zi[row], 2: zss * the pass's first sample).  One workgroup per row; thread i owns tiles
// [i per, (i+1) per).
template <int K>
static __global__ __launch_bounds__(sos_chain_threads(K)) void k_sos_chain(SosIO io, const double *__restrict__ plan, int64_t nt,
                                                                          int per, const double *__restrict__ tile_end,
                                                                          double *__restrict__ tile_in, int zmode,
                                                                          const double *__restrict__ zi) {
    constexpr int S = 2 * K, CT = sos_chain_threads(K), LV = sos_chain_levels(K), U = K <= 2 ? 8 : 4;
    __shared__ double st[S * CT];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const double *te = tile_end + row * (int64_t)S * per * CT;        // [S][per][CT]: thread tid's j-th tile at [s][j][tid]
    double *ti = tile_in + row * (int64_t)S * per * CT;
    double s0[S];
    if (zmode == 1) {
#pragma unroll
        for (int s = 0; s < S; ++s) s0[s] = zi[row * S + s];
    } else {
        const double v = zmode == 2 ? (double)sos_src(io, io.x + row * io.x_ld, 0) : 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) s0[s] = plan[sos_o_zss() + s] * v;
    }
    const double *mt = plan + sos_o_mt(S);
    const int64_t k0 = (int64_t)tid * per;
    double p[S];
#pragma unroll
    for (int s = 0; s < S; ++s) p[s] = tid == 0 ? s0[s] : 0.0;
    // U tiles' end states are loaded ahead of their use: the loop is a dependent chain, a load per step would expose its latency
    for (int j0 = 0; j0 < per; j0 += U) {
        double f[U][S];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + j0 + u;
#pragma unroll
            for (int s = 0; s < S; ++s) f[u][s] = (j0 + u < per && k < nt) ? te[((int64_t)s * per + j0 + u) * CT + tid] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j0 + u >= per) break;
            sos_mv<S>(mt, p);                 // (tiles past the end contribute f = 0: the state just decays on)
#pragma unroll
            for (int s = 0; s < S; ++s) p[s] += f[u][s];
        }
    }
#pragma unroll
    for (int d = 0; d < LV; ++d) {
#pragma unroll
        for (int s = 0; s < S; ++s) st[s * CT + tid] = p[s];
        __syncthreads();
        if (tid >= (1 << d)) {
            double q[S];
#pragma unroll
            for (int s = 0; s < S; ++s) q[s] = st[s * CT + tid - (1 << d)];
            sos_mv<S>(plan + sos_o_cpw(S) + d * S * S, q);
#pragma unroll
            for (int s = 0; s < S; ++s) p[s] += q[s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < S; ++s) st[s * CT + tid] = p[s];
    __syncthreads();
    double sp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) sp[s] = tid > 0 ? st[s * CT + tid - 1] : s0[s];
    for (int j0 = 0; j0 < per; j0 += U) {
        double f[U][S];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + j0 + u;
#pragma unroll
            for (int s = 0; s < S; ++s) f[u][s] = (j0 + u < per && k < nt) ? te[((int64_t)s * per + j0 + u) * CT + tid] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + j0 + u;
            if (j0 + u >= per || k >= nt) break;
#pragma unroll
            for (int s = 0; s < S; ++s) ti[((int64_t)s * per + j0 + u) * CT + tid] = sp[s];
            sos_mv<S>(mt, sp);
#pragma unroll
            for (int s = 0; s < S; ++s) sp[s] += f[u][s];
        }
    }
}

// ------------------------------------------------------------------------------------------ host side
int64_t sos_tiles(int64_t len) { return (len + SP_SOS_TILE - 1) / SP_SOS_TILE; }
static int64_t sos_per(int nsec, int64_t len) { return (sos_tiles(len) + sos_chain_threads(nsec) - 1) / sos_chain_threads(nsec); }
int64_t sos_work_doubles(int nsec, int64_t len, int64_t nrows) {
    return 2 * nrows * 2 * nsec * sos_per(nsec, len) * sos_chain_threads(nsec);
}
int sos_plan_doubles(int nsec) { return sos_o_end(2 * nsec); }

static void sos_mmul(const double *x, const double *y, double *r, int S) {
    std::vector<double> t((size_t)S * S, 0.0);
    for (int i = 0; i < S; ++i)
        for (int k = 0; k < S; ++k)
            for (int j = 0; j < S; ++j) t[(size_t)i * S + j] += x[i * S + k] * y[k * S + j];
    for (int i = 0; i < S * S; ++i) r[i] = t[(size_t)i];
}

// sos[nsec][6] (a0 != 0, checked by the caller) -> plan[sos_plan_doubles(nsec)] for passes of len samples
void sos_build_plan(const double *sos, int nsec, int64_t len, double *plan) {
    const int K = nsec, S = 2 * K;
    for (int i = 0; i < sos_plan_doubles(nsec); ++i) plan[i] = 0.0;
    double scale = 1.0;
    for (int k = 0; k < K; ++k) {
        const double *r = sos + 6 * k;
        const double b0 = r[0] / r[3], b1 = r[1] / r[3], b2 = r[2] / r[3], a1 = r[4] / r[3], a2 = r[5] / r[3];
        plan[5 * k] = b0;
        plan[5 * k + 1] = b1;
        plan[5 * k + 2] = b2;
        plan[5 * k + 3] = a1;
        plan[5 * k + 4] = a2;
        // scipy.signal.sosfilt_zi: the section's steady state for a constant input `scale`, gain G = sum(b) / sum(a)
        const double G = (b0 + b1 + b2) / (1.0 + a1 + a2);
        plan[sos_o_zss() + 2 * k] = scale * (G - b0);
        plan[sos_o_zss() + 2 * k + 1] = scale * (b2 - a2 * G);
        scale *= G;
    }
    // homogeneous responses H[j][s] and the one-chunk state map M_C (column s: unit incoming state s, zero input)
    std::vector<double> mc((size_t)S * S);
    for (int s = 0; s < S; ++s) {
        std::vector<double> w((size_t)S, 0.0);
        w[(size_t)s] = 1.0;
        for (int j = 0; j < SP_SOS_C; ++j) {
            double v = 0.0;
            for (int k = 0; k < K; ++k) {
                const double *c = plan + 5 * k;
                const double y = c[0] * v + w[2 * k];
                w[2 * k] = c[1] * v - c[3] * y + w[2 * k + 1];
                w[2 * k + 1] = c[2] * v - c[4] * y;
                v = y;
            }
            plan[sos_o_h() + j * S + s] = v;
        }
        for (int i = 0; i < S; ++i) mc[(size_t)i * S + s] = w[(size_t)i];
    }
    std::vector<double> m = mc;
    for (int d = 0; d < SP_SOS_LOGWG; ++d) {
        for (int i = 0; i < S * S; ++i) plan[sos_o_pw(S) + d * S * S + i] = m[(size_t)i];
        sos_mmul(m.data(), m.data(), m.data(), S);
    }
    for (int i = 0; i < S * S; ++i) plan[sos_o_mt(S) + i] = m[(size_t)i];   // M_C^WG
    // (M_tile^per)^(2^d) for the chain's scan
    const int64_t per = sos_per(K, len);
    std::vector<double> mp((size_t)S * S, 0.0), b = m;
    for (int i = 0; i < S; ++i) mp[(size_t)i * S + i] = 1.0;
    for (int64_t e = per; e > 0; e >>= 1) {
        if (e & 1) sos_mmul(mp.data(), b.data(), mp.data(), S);
        sos_mmul(b.data(), b.data(), b.data(), S);
    }
    for (int d = 0; d < sos_chain_levels(K); ++d) {
        for (int i = 0; i < S * S; ++i) plan[sos_o_cpw(S) + d * S * S + i] = mp[(size_t)i];
        sos_mmul(mp.data(), mp.data(), mp.data(), S);
    }
}

template <int K>
static void sos_pass_k(LaunchCtx c, const double *plan, const SosIO &io, int64_t nrows, int zmode, const double *zi, double *zf,
                       double *work) {
    constexpr int S = 2 * K;
    const int64_t nt = sos_tiles(io.len);
    const int per = (int)sos_per(K, io.len);
    const int64_t rb = (int64_t)S * per * sos_chain_threads(K);     // tile states of one row
    double *tile_end = work, *tile_in = work + nrows * rb;
    for (int64_t r0 = 0; r0 < nrows; r0 += 65535) {          // grid.y limit: rows in batches
        const int64_t nr = nrows - r0 < 65535 ? nrows - r0 : 65535;
        SosIO b = io;
        b.x += r0 * io.x_ld;
        b.y += r0 * io.y_ld;
        double *te = tile_end + r0 * rb, *ti = tile_in + r0 * rb;
        const double *zib = zi ? zi + r0 * S : nullptr;
        double *zfb = zf ? zf + r0 * S : nullptr;
        const dim3 grid((unsigned)nt, (unsigned)nr);
        hipLaunchKernelGGL((k_sos_tile<K, false>), grid, dim3(SP_SOS_WG), 0, c.stream, b, plan, nt, per, (const double *)nullptr,
                           te, (double *)nullptr);
        hipLaunchKernelGGL((k_sos_chain<K>), dim3((unsigned)nr), dim3(sos_chain_threads(K)), 0, c.stream, b, plan, nt, per,
                           (const double *)te, ti, zmode, zib);
        hipLaunchKernelGGL((k_sos_tile<K, true>), grid, dim3(SP_SOS_WG), 0, c.stream, b, plan, nt, per, (const double *)ti, te,
                           zfb);
    }
}

int launch_sos_pass(LaunchCtx c, int nsec, const double *plan, const SosIO &io, int64_t nrows, int zmode, const double *zi,
                    double *zf, double *work) {
    if (io.len < 1 || nrows < 1 || sos_tiles(io.len) > INT_MAX) return -1;
    switch (nsec) {
        case 1: sos_pass_k<1>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 2: sos_pass_k<2>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 3: sos_pass_k<3>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 4: sos_pass_k<4>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 5: sos_pass_k<5>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 6: sos_pass_k<6>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 7: sos_pass_k<7>(c, plan, io, nrows, zmode, zi, zf, work); break;
        case 8: sos_pass_k<8>(c, plan, io, nrows, zmode, zi, zf, work); break;
        default: return -1;
    }
    return 0;
}

}   // namespace sp
