// k_ddc.hip -- digital down-converter: mix with a carrier, low-pass, decimate, in one pass over the record.
//   v[n] = x[n] e(-nu (n0 + n)),  n < nsig, 0 outside the row;   e(t) = exp(2 pi i t), nu in cycles per sample
//   y[k] = sum_{j<T} h[j] v[k q + (T - 1) / 2 - j],  k < ceil(nsig / q)      (scipy.signal.resample_poly(v, 1, q, window=h), T odd)
// Polyphase form: with j = p q + s the sum runs over the decimated components U_s[i] = v[i q + c - s], c = (T - 1) / 2:
//   y[k] = sum_{s<q} sum_p h[p q + s] U_s[k - p]
// so that for one s a thread that owns R consecutive outputs reads a sliding window of U_s: R + P - 1 LDS reads for R P MACs.
//
// A workgroup produces the K outputs kt .. kt + K - 1 of one row (geometry: ddc_geom, launch.h).  It
//   1. copies the taps, laid out [s][p'] with p' = PP - 1 - p (the sum becomes a correlation that walks up the row), into LDS;
//   2. stages the NI q samples from (kt - PP + 1) q + c - q + 1 on: 16-byte loads aligned on the absolute element index, mixed on the
//      way in, written as float2 to the row of their component: sample d of the span is entry d / q of row q - 1 - d % q.  Entry i of
//      a row sits at i + (i >> 5): the 32 lanes of a ds_read_b64 group read entries 8 apart, and the pad of one float2 per 32 entries
//      spreads them over all 64 banks;
//   3. runs the FIR: thread (og, sg) accumulates the outputs og R .. og R + R - 1 over the components s = sg, sg + SG, ..; four taps
//      (one broadcast ds_read_b128) per step against a register window of R + 3 entries that slides by four;
//   4. sums the SG partial results of every output through LDS in a fixed order and stores the tile with coalesced stores.
// Oscillator: the phase of a sample is ph0 + dnu n modulo 2^64 (units of 2^-64 turns; the wrap IS the reduction modulo one turn).
// Every thread takes the phasor of the first staged sample from a float64 sincospi, multiplies it in float64 with the table entry
// exp(-2 pi i nu j) of its sample (float32, built on the host in float64, j < the span) and rounds once to float32.
#include "launch.h"
namespace sp {

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool CPLX, bool MIX>
__global__ __launch_bounds__(256) void k_ddc(const void *__restrict__ x, int64_t x_ld, int64_t nsig, int64_t nout, int64_t tiles,
                                             DdcGeom g, uint64_t ph0, uint64_t dnu, const cf *__restrict__ tab,
                                             const float *__restrict__ taps, int vec, cf *__restrict__ out) {
    extern __shared__ float4 smem4[];
    constexpr int R = SP_DDC_R;
    constexpr int V = CPLX ? 2 : 4;               // samples per 16-byte load
    const int q = g.q, PP = g.PP, pitch = g.pitch, K = g.K, span = g.span;
    v2f *U = reinterpret_cast<v2f *>(smem4);
    float *G = reinterpret_cast<float *>(U + (size_t)q * pitch);
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / tiles, kt = ((int64_t)blockIdx.x % tiles) * K;
    const int64_t nb = (kt - (PP - 1)) * q + (g.ntaps - 1) / 2 - (q - 1);     // the first staged sample (row index, may be < 0)

    for (int i = tid; i < q * PP / 4; i += 256) reinterpret_cast<float4 *>(G)[i] = reinterpret_cast<const float4 *>(taps)[i];

    const int64_t e0 = b * x_ld + nb;             // its element index from x
    const int shift = (int)(e0 & (V - 1));
    const int64_t na = nb - shift;                // the row index of table entry 0: na + b x_ld is a multiple of V
    double c0 = 1.0, s0 = 0.0;
    if constexpr (MIX) {
        const uint64_t ph = ph0 + dnu * (uint64_t)na;
        sincospi(ldexp((double)(int64_t)ph, -63), &s0, &c0);                   // e(-t) = (c0, -s0)
    }
    const float *xf = reinterpret_cast<const float *>(x);
    const int nvec = (span + shift + V - 1) / V;
    for (int iv = tid; iv < nvec; iv += 256) {
        const int jt = iv * V;
        const int64_t n = na + jt;
        float xs[4];
        if (vec && n >= 0 && n + V <= nsig) {
            const float4 t = *reinterpret_cast<const float4 *>(xf + (b * x_ld + n) * (CPLX ? 2 : 1));
            xs[0] = t.x;
            xs[1] = t.y;
            xs[2] = t.z;
            xs[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool in = n + j >= 0 && n + j < nsig;
                const int64_t e = b * x_ld + (in ? n + j : 0);
                if constexpr (CPLX) {
                    const cf t = in ? reinterpret_cast<const cf *>(x)[e] : mk(0.f, 0.f);
                    xs[2 * j] = t.x;
                    xs[2 * j + 1] = t.y;
                } else {
                    xs[j] = in ? xf[e] : 0.f;
                }
            }
        }
        float tb[2 * V];
        if constexpr (MIX) {
#pragma unroll
            for (int j = 0; j < V / 2; ++j) {
                const float4 t = reinterpret_cast<const float4 *>(tab + jt)[j];
                tb[4 * j] = t.x;
                tb[4 * j + 1] = t.y;
                tb[4 * j + 2] = t.z;
                tb[4 * j + 3] = t.w;
            }
        }
        const int d0 = jt - shift + 4 * q;        // >= 1: the division below is unsigned
        int ip = d0 / q - 4, rem = d0 % q;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int d = jt - shift + j;
            v2f v;
            if constexpr (CPLX) {
                v.x = xs[2 * j];
                v.y = xs[2 * j + 1];
            } else {
                v.x = xs[j];
                v.y = 0.f;
            }
            if constexpr (MIX) {
                const double tc = (double)tb[2 * j], ts = (double)tb[2 * j + 1];
                const float pr = (float)(c0 * tc + s0 * ts), pi = (float)(c0 * ts - s0 * tc);
                if constexpr (CPLX) {
                    const float a = v.x, bb = v.y;
                    v.x = a * pr - bb * pi;
                    v.y = a * pi + bb * pr;
                } else {
                    v.y = v.x * pi;
                    v.x = v.x * pr;
                }
            }
            if (d >= 0 && d < span) U[(q - 1 - rem) * pitch + ip + (ip >> 5)] = v;
            if (++rem == q) {
                rem = 0;
                ++ip;
            }
        }
    }
    __syncthreads();

    const int og = tid & ((1 << g.og_log2) - 1), sg = tid >> g.og_log2;
    const int o = og * R;
    v2f acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = v2f{0.f, 0.f};
    for (int s = sg; s < q; s += g.sg) {
        const v2f *Us = U + s * pitch;
        const float4 *Gs = reinterpret_cast<const float4 *>(G + s * PP);
        v2f w[R + 3];
#pragma unroll
        for (int i = 0; i < R + 3; ++i) w[i] = Us[o + i + ((o + i) >> 5)];
        for (int pc = 0; pc < PP; pc += 4) {
            const float4 g4 = Gs[pc >> 2];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                acc[r] += g4.x * w[r];
                acc[r] += g4.y * w[r + 1];
                acc[r] += g4.z * w[r + 2];
                acc[r] += g4.w * w[r + 3];
            }
#pragma unroll
            for (int i = 0; i < R - 1; ++i) w[i] = w[i + 4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = o + pc + R + 3 + i;
                w[R - 1 + i] = Us[e + (e >> 5)];
            }
        }
    }
    __syncthreads();                              // the components are read: their LDS now carries the partial results [sg][K]
#pragma unroll
    for (int r = 0; r < R; ++r) U[sg * K + o + r] = acc[r];
    __syncthreads();
    for (int oo = tid; oo < K; oo += 256) {
        v2f a = U[oo];
        for (int i = 1; i < g.sg; ++i) a += U[i * K + oo];
        const int64_t k = kt + oo;
        if (k < nout) out[b * nout + k] = mk(a.x, a.y);
    }
}

int launch_ddc(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const DdcGeom &g, uint64_t ph0,
               uint64_t dnu, const cf *tab, const float *taps, bool vec, cf *out) {
    const int64_t nout = (nsig + g.q - 1) / g.q, tiles = (nout + g.K - 1) / g.K;
    if (batch < 1 || nsig < 1 || x_ld < nsig || tiles * batch > 0x7fffffff) return -1;
    const dim3 grid((unsigned)(tiles * batch));
#define L_(CP, MX)                                                                                    \
    {                                                                                                 \
        if (lds_raise<k_ddc<CP, MX>>(g.lds)) return -1;       /* the largest shapes stage more than 64 KiB */ \
        hipLaunchKernelGGL((k_ddc<CP, MX>), grid, dim3(256), g.lds, c.stream, x, x_ld, nsig, nout, tiles, g, ph0, dnu, tab, taps, vec ? 1 : 0, out); \
    }
    if (!cplx) {
        if (tab == nullptr) L_(false, false) else L_(false, true)
    } else {
        if (tab == nullptr) L_(true, false) else L_(true, true)
    }
#undef L_
    return 0;
}

}   // namespace sp
