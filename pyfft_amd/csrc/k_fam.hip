// k_fam.hip -- the FFT accumulation method (Roberts, Brown & Loomis 1991): the spectral correlation of the whole (f, alpha) plane.
// The channelizer is the unchanged STFT kernel; its frames reach this file bin-major, Y, X [np][ld] complex64 with the frames of a
// pass along a row, frame-referenced (no demodulation).  With g a real taper of P taps, block b = the frames bP .. bP + P - 1 and
// 2Q = P hop / np, the pair i = (k, l) gets
//   F_b[m] = sum_{p < P} g[p] Y[k][bP + p] conj(X[l][bP + p]) e(-m p / P)          (conj != 0: ... X[l][bP + p], no conjugate)
//   S[i][j] = scale sum_b F_b[(j - Q + d 2Q) mod P],  j = 0 .. 2Q - 1,  d = k - l  (conj != 0: d = k + l)
// The demodulation of the channels to absolute time, e(-k p hop / np) on Y and e(+l p hop / np) on conj(X), is a factor
// e(-d p 2Q / P) on the product because P hop is a multiple of np: it only moves the output bin, by d 2Q.  No phase table.
// A transform group of P / 16 threads owns ONE pair and walks the blocks of the pass in ascending order: per block 16 P bytes of
// loads (two rows of P frames), one P-point forward transform, and the sum over the blocks in float32 registers.  Pairs sorted by k
// put the same row of Y under the groups of a workgroup and of its neighbours, so that row comes from L1 / L2.  Across passes the
// sums are float64 in memory (acc[npairs][2Q] re, im), touched only where a call has more than one pass; the last pass multiplies by
// `scale` once, in float64, and rounds to complex64.  No atomics and a fixed order: two calls agree bitwise.
// Pairs past the table's end in the last workgroup are clamped to the last pair and store nothing: every load is inside the
// scratch and every barrier is met.
#include "launch.h"
namespace sp {

// two waves per SIMD (amdgpu_waves_per_eu), as k_cyclic: sums, a product and a transform with its constants take 110 .. 200 registers
template <class X>
__global__ __launch_bounds__(X::C::WG) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_fam(FamArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= SP_FAM_MAX_P, "power-of-two transforms of 32 .. 8192 points");
    constexpr int P = X::L;
    const int64_t pr = (int64_t)blockIdx.x * C::FPW + grp;
    const bool act = pr < a.npairs;
    const int2 kl = a.pairs[act ? pr : a.npairs - 1];
    const cf *__restrict__ yr = a.Y + (int64_t)kl.x * a.ld;
    const cf *__restrict__ xr = a.X + (int64_t)kl.y * a.ld;
    const float sgn = a.conj ? 1.f : -1.f;          // the second operand is conj(X) in the plain form
    cf acc[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) acc[t] = mk(0.f, 0.f);
    for (int64_t b = 0; b < a.nb; ++b) {
        // the thread's index is opaque in every block: the addresses of the loads are otherwise hoisted and held across the transform
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int64_t base = b * P + tq;
        cf v[C::R], u[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) v[t] = yr[base + C::T * t];
#pragma unroll
        for (int t = 0; t < C::R; ++t) u[t] = xr[base + C::T * t];
#pragma unroll
        for (int t = 0; t < C::R; ++t) v[t] = a.g[tq + C::T * t] * cmul(v[t], mk(u[t].x, sgn * u[t].y));
        fwd_row(xf, v, lds, tid, n);
#pragma unroll
        for (int t = 0; t < C::R; ++t) acc[t] = acc[t] + v[t];
    }
    if (!act) return;
    // bin m of the transform is the output column j = (m - d 2Q + Q) mod P, kept where j < 2Q
    const int d = a.conj ? kl.x + kl.y : kl.x - kl.y;
    const int shift = (int)(((int64_t)(d & (P - 1)) * a.twoQ) & (P - 1));
    const int Q = a.twoQ / 2;
    const int64_t o = pr * a.twoQ;
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int j = (tid + C::T * t - shift + Q) & (P - 1);
        if (j >= a.twoQ) continue;
        double re = (double)acc[t].x, im = (double)acc[t].y;
        if (!a.first) {
            re += a.acc[2 * (o + j)];
            im += a.acc[2 * (o + j) + 1];
        }
        if (a.last) {
            a.S[o + j] = mk((float)(a.scale * re), (float)(a.scale * im));
        } else {
            a.acc[2 * (o + j)] = re;
            a.acc[2 * (o + j) + 1] = im;
        }
    }
}

// channel powers from the same scratch: workgroup k sums g[f mod P] |Z[k][f]|^2 over the frames of the pass in float64 -- thread t the
// frames t, t + 256, ..., then a tree over the 256 threads in a fixed order -- and adds the passes before it from acc[k]
static __global__ __launch_bounds__(256) void k_fam_pw(const cf *__restrict__ Z, int64_t ld, int64_t nframes, int P,
                                                       const float *__restrict__ g, double *__restrict__ acc, int first, int last,
                                                       double scale, float *__restrict__ Pw) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const cf *z = Z + (int64_t)k * ld;
    double s = 0.0;
    for (int64_t f = tid; f < nframes; f += 256) s += (double)g[f & (P - 1)] * (double)cnorm(z[f]);
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double tot = (first ? 0.0 : acc[k]) + red[0];
        if (last) Pw[k] = (float)(scale * tot);
        else acc[k] = tot;
    }
}

int launch_fam(LaunchCtx c, const FamArgs &a, int P, const cf *tw) {
    if (a.npairs < 1 || a.npairs > SP_FAM_MAX_PAIRS || a.nb < 1 || a.ld < a.nb * P || a.twoQ < 2 || a.twoQ > P || (a.twoQ & (a.twoQ - 1))) return -1;
    if (!a.Y || !a.X || !a.g || !a.pairs || (a.last && !a.S) || (!(a.first && a.last) && !a.acc)) return -1;
    const int fpw = fpw_of(P);
    const int64_t blocks = (a.npairs + fpw - 1) / fpw;
    const size_t lds_bytes = xf_image_bytes(P);
    const XfTables tb{tw, nullptr, nullptr, P};
    return for_pow2<32, SP_FAM_MAX_P>(P, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (lds_raise<k_fam<XT>>(lds_bytes)) return -1;
        hipLaunchKernelGGL((k_fam<XT>), dim3((unsigned)blocks), dim3(XT::C::WG), lds_bytes, c.stream, a, tb);
        return 0;
    });
}

int launch_fam_pw(LaunchCtx c, const cf *Z, int np, int64_t ld, int64_t nframes, int P, const float *g, double *acc, bool first, bool last,
                  double scale, float *Pw) {
    if (np < 1 || np > 65535 || nframes < 1 || ld < nframes || !Z || !g || !acc || (last && !Pw)) return -1;
    hipLaunchKernelGGL(k_fam_pw, dim3((unsigned)np), dim3(256), 0, c.stream, Z, ld, nframes, P, g, acc, first ? 1 : 0, last ? 1 : 0, scale, Pw);
    return 0;
}

}   // namespace sp
