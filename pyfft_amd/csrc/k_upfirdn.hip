// k_upfirdn.hip -- rational resampler: zero-stuff by `up`, filter with the real taps h, keep every `down`-th sample, in one pass.
//   xu[i up] = x[i], i < nsig, 0 elsewhere;   y[m] = sum_{j<T} h[j] xu[m down - j]
// Polyphase form: only the taps j = phi + p up meet a sample, with phi = (m down) mod up and i0 = floor(m down / up):
//   y[m] = sum_{p<P} h[phi + p up] x[i0 - p],  P = ceil(T / up)      (scipy.signal.upfirdn(h, x, up, down))
// The outputs m, m + up, m + 2 up, .. share phi, and their i0 step by `down`: a thread that owns R of them reads every tap once.
//
// A workgroup produces the K outputs mt .. mt + K - 1 of one row (geometry: upf_geom, launch.h).  It
//   1. copies the taps, phase-major [phi][p] at an odd row pitch (zero-padded to P), into LDS;
//   2. stages the NI samples from ib = floor(mt down / up) - (P - 1) on: 16-byte loads aligned on the absolute element index, zero
//      outside the row, sample i at entry i: the inner loop then needs no address arithmetic (the taps of a slice are immediate
//      offsets from one pointer per output);
//   3. runs the sums: the thread (s, ot) takes the items ot, ot + OT, ..; item w < up NG is the R outputs mt + w + r up NG, r < R, which
//      share the phase of output w (neighbouring lanes own neighbouring outputs: their samples lie down / up apart); it accumulates
//      them over the taps p = s, s + SG, .. of that phase's row;
//   4. sums the SG partial results of every output through LDS in the order s = 0, 1, .. and stores the tile with coalesced stores.
// All index arithmetic from m down on is 64-bit; inside a tile everything is relative to ib and fits 32 bits.
#include "launch.h"
namespace sp {

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool CPLX> struct UpfT { typedef float T; };
template <> struct UpfT<true> { typedef v2f T; };

template <bool CPLX>
__global__ __launch_bounds__(256) void k_upfirdn(const void *__restrict__ x, int64_t x_ld, int64_t nsig, int64_t m0, int64_t nout,
                                                 int64_t tiles, UpfGeom g, const float *__restrict__ taps, int vec,
                                                 void *__restrict__ out) {
    extern __shared__ float4 smem4[];
    typedef typename UpfT<CPLX>::T E;
    constexpr int R = SP_UPF_R;
    constexpr int V = CPLX ? 2 : 4;               // samples per 16-byte load
    const int up = g.up, down = g.down, P = g.P, pitch = g.pitch, K = g.K, NI = g.NI;
    E *X = reinterpret_cast<E *>(smem4);
    E *S = X + g.xlen;                            // the partial sums [sg][K]
    float *G = reinterpret_cast<float *>(S + (size_t)g.sg * K);
    const int tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / tiles, kt = ((int64_t)blockIdx.x % tiles) * K;
    const int64_t md = (m0 + kt) * down;          // the tile's first output on the zero-stuffed grid
    const int64_t q0 = md / up;
    const int r0 = (int)(md % up);
    const int64_t ib = q0 - (P - 1);              // the first staged sample (row index, may be < 0)

    for (int i = tid; i < up * pitch; i += 256) G[i] = taps[i];

    const int64_t e0 = b * x_ld + ib;             // its element index from x
    const int shift = (int)(e0 & (V - 1));
    const int64_t na = ib - shift;                // na + b x_ld is a multiple of V
    const float *xf = reinterpret_cast<const float *>(x);
    const int nvec = (NI + shift + V - 1) / V;
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
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int d = jt - shift + j;
            if (d >= 0 && d < NI) {
                if constexpr (CPLX) X[d] = v2f{xs[2 * j], xs[2 * j + 1]};
                else X[d] = xs[j];
            }
        }
    }
    __syncthreads();

    const int SG = g.sg, s = tid & (SG - 1), ot = tid >> g.sg_log2, OT = 256 >> g.sg_log2;
    // output w of the tile (w + items, w + 2 items, .. share its phase): phi and its i0 relative to ib, j0; the others of the item
    // follow NG down apart.  From round to round w grows by OT: the two advance without a division
    const int step = g.NG * down, dq = OT * down / up, dr = OT * down % up;
    int phi = (r0 + ot * down) % up, j0 = (r0 + ot * down) / up + (P - 1);
    for (int rd = 0; rd < g.rounds; ++rd, phi += dr, j0 += dq) {
        const int w = ot + rd * OT;
        if (w >= g.items) break;
        if (phi >= up) {
            phi -= up;
            ++j0;
        }
        const float *Gp = G + phi * pitch;
        E acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (CPLX) acc[r] = v2f{0.f, 0.f};
            else acc[r] = 0.f;
        }
#pragma unroll 4
        for (int p = s; p < P; p += SG) {
            const float gp = Gp[p];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += gp * X[j0 + r * step - p];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) S[s * K + w + r * g.items] = acc[r];
    }
    __syncthreads();
    E *y = reinterpret_cast<E *>(out);
    for (int oo = tid; oo < K; oo += 256) {
        E a = S[oo];
        for (int i = 1; i < SG; ++i) a += S[i * K + oo];
        const int64_t k = kt + oo;
        if (k < nout) y[b * nout + k] = a;
    }
}

int launch_upfirdn(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const UpfGeom &g,
                   const float *taps, bool vec, int64_t m0, int64_t nout, void *out) {
    const int64_t tiles = (nout + g.K - 1) / g.K;
    if (batch < 1 || nsig < 1 || nout < 1 || m0 < 0 || x_ld < nsig || tiles > 0x7fffffff / batch) return -1;
    if (g.lds > SP_LDS_MAX) return -1;
    const dim3 grid((unsigned)(tiles * batch));
#define L_(CP)                                                                                        \
    {                                                                                                 \
        if (lds_raise<k_upfirdn<CP>>(g.lds)) return -1;   /* long filters and heavy decimation stage more than 64 KiB */ \
        hipLaunchKernelGGL((k_upfirdn<CP>), grid, dim3(256), g.lds, c.stream, x, x_ld, nsig, m0, nout, tiles, g, taps, vec ? 1 : 0, \
                           out);                                                                      \
    }
    if (cplx) L_(true) else L_(false)
#undef L_
    return 0;
}

}   // namespace sp
