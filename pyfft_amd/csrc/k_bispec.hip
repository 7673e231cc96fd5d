// k_bispec.hip -- bispectrum / bicoherence: the contraction over frames of per-frame spectra (k_stft output)
//   B(i, j) = sum_g X_g(i) Y_g(j) conj(Z_g(s)),  D(i, j) = sum_g |X_g(i) Y_g(j)|^2,  P(s) = sum_g |Z_g(s)|^2,  s = i + j - c0
// Spectra are frame-major [m][nb] complex64 (c0 = 0: bins 0 .. nfft/2; c0 = nfft/2: two-sided, fftshift-ed).
#include "launch.h"
namespace sp {

// k_bispec_tile: one workgroup = one 64 x 64 tile of (i, j) pairs x one chunk of <= BS_FC frames.  256 threads, 4 x 4 pairs per
// thread: i = i0 + 4 (t & 15) + a, j = j0 + 4 (t >> 4) + b, so a thread's 16 sums need 4 X, 4 Y and the 7 Z at s0 + 0 .. 6.
// Frames are staged in LDS BS_FB at a time, double-buffered: each thread fetches its 8 values of the next batch into registers
// while it computes the current one, so there is one barrier per batch.  LDS image of one frame (2 KiB):
//   [0, 64)    X, split so that the 16 lanes of a ds_read_b128 lane group read 256 contiguous bytes: slot 2q + r holds
//              X[4q + r] for r < 2, slot 32 + 2q + r - 2 holds X[4q + r] for r >= 2
//   [64, 128)  Y[j0 .. j0 + 63]   (4 distinct addresses per wave: broadcast)
//   [128, 256) Z[i0 + j0 - c0 .. + 127]
// Values outside the spectra (i or j >= nb, s outside [0, nb), frames past the chunk) are staged as 0 and add nothing: the pairs
// outside the valid region of a boundary tile end with B = 0 and are replaced by NaN in k_bispec_finish.
// Output: this (tile, chunk)'s fp32 sums, part[(tile * nfc + chunk)][3][64 * 64] (Re B, Im B, D), summed in float64 by
// k_bispec_reduce -- no float atomics, a fixed order, deterministic.
#define BS_T 64
#define BS_FC 256
#define BS_FB 8
#define BS_FRAME 256                        // complex values per staged frame
#define BS_PART (3 * BS_T * BS_T)           // floats per (tile, chunk)

static __global__ __launch_bounds__(256) void k_bispec_tile(const cf *__restrict__ X, const cf *__restrict__ Y,
                                                            const cf *__restrict__ Z, int nb, int c0, int64_t m,
                                                            const int2 *__restrict__ tiles, int nfc, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) cf sh[2][BS_FB][BS_FRAME];
    const int tid = threadIdx.x;
    const int2 tl = tiles[blockIdx.x];
    const int i0 = tl.x * BS_T, j0 = tl.y * BS_T;
    const int64_t g0 = (int64_t)blockIdx.y * BS_FC;
    const int64_t g1 = g0 + BS_FC < m ? g0 + BS_FC : m;
    // this thread's staging slot: source row, column and LDS position
    const cf *src;
    int col, pos;
    if (tid < 64) {
        src = X;
        col = i0 + tid;
        const int q = tid >> 2, r = tid & 3;
        pos = (r < 2 ? 0 : 32) + 2 * q + (r & 1);
    } else if (tid < 128) {
        src = Y;
        col = j0 + tid - 64;
        pos = tid;
    } else {
        src = Z;
        col = i0 + j0 - c0 + tid - 128;
        pos = tid;
    }
    const bool colok = col >= 0 && col < nb;
    const int ib = 4 * (tid & 15), jb = 4 * (tid >> 4);
    float bre[4][4], bim[4][4], dd[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) bre[a][b] = bim[a][b] = dd[a][b] = 0.f;

    cf st[BS_FB];
    auto fetch = [&](int64_t gb) {
#pragma unroll
        for (int f = 0; f < BS_FB; ++f) {
            const int64_t g = gb + f;
            st[f] = (colok && g < g1) ? src[g * nb + col] : mk(0.f, 0.f);
        }
    };
    fetch(g0);
    int buf = 0;
    for (int64_t gb = g0; gb < g1; gb += BS_FB) {
#pragma unroll
        for (int f = 0; f < BS_FB; ++f) sh[buf][f][pos] = st[f];
        __syncthreads();
        if (gb + BS_FB < g1) fetch(gb + BS_FB);     // in flight while this batch is computed
#pragma unroll 2
        for (int f = 0; f < BS_FB; ++f) {
            const cf *fr = sh[buf][f];
            const float4 xa = *reinterpret_cast<const float4 *>(fr + (ib >> 1));
            const float4 xb = *reinterpret_cast<const float4 *>(fr + 32 + (ib >> 1));
            const float4 ya = *reinterpret_cast<const float4 *>(fr + 64 + jb);
            const float4 yb = *reinterpret_cast<const float4 *>(fr + 64 + jb + 2);
            float4 zq[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) zq[k] = *reinterpret_cast<const float4 *>(fr + 128 + ib + jb + 2 * k);
            const float xr[4] = {xa.x, xa.z, xb.x, xb.z}, xi[4] = {xa.y, xa.w, xb.y, xb.w};
            const float yr[4] = {ya.x, ya.z, yb.x, yb.z}, yi[4] = {ya.y, ya.w, yb.y, yb.w};
            const float zr[8] = {zq[0].x, zq[0].z, zq[1].x, zq[1].z, zq[2].x, zq[2].z, zq[3].x, zq[3].z};
            const float zi[8] = {zq[0].y, zq[0].w, zq[1].y, zq[1].w, zq[2].y, zq[2].w, zq[3].y, zq[3].w};
            float ay[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) ay[b] = yr[b] * yr[b] + yi[b] * yi[b];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float ax = xr[a] * xr[a] + xi[a] * xi[a];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float pr = xr[a] * yr[b] - xi[a] * yi[b];
                    const float pi = xr[a] * yi[b] + xi[a] * yr[b];
                    const int s = a + b;
                    bre[a][b] += pr * zr[s] + pi * zi[s];        // p conj(z)
                    bim[a][b] += pi * zr[s] - pr * zi[s];
                    dd[a][b] += ax * ay[b];
                }
            }
        }
        buf ^= 1;
    }
    float *out = part + ((int64_t)blockIdx.x * nfc + blockIdx.y) * BS_PART;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int o = (ib + a) * BS_T + jb;
        *reinterpret_cast<float4 *>(out + o) = make_float4(bre[a][0], bre[a][1], bre[a][2], bre[a][3]);
        *reinterpret_cast<float4 *>(out + BS_T * BS_T + o) = make_float4(bim[a][0], bim[a][1], bim[a][2], bim[a][3]);
        *reinterpret_cast<float4 *>(out + 2 * BS_T * BS_T + o) = make_float4(dd[a][0], dd[a][1], dd[a][2], dd[a][3]);
    }
}

// ppart[chunk][s] = sum over the chunk's frames of |Z_g(s)|^2, float64, frames in order
static __global__ __launch_bounds__(256) void k_bispec_pzz(const cf *__restrict__ Z, int nb, int64_t m, double *__restrict__ ppart) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nb) return;
    const int64_t g0 = (int64_t)blockIdx.y * BS_FC;
    const int64_t g1 = g0 + BS_FC < m ? g0 + BS_FC : m;
    double acc = 0.0;
    for (int64_t g = g0; g < g1; ++g) {
        const cf z = Z[g * nb + s];
        acc += (double)z.x * z.x + (double)z.y * z.y;
    }
    ppart[(int64_t)blockIdx.y * nb + s] = acc;
}

// acc[tile][3][4096] (+)= sum over the nfc chunks of part, p64[s] (+)= sum of ppart: float64, chunks in order
static __global__ __launch_bounds__(256) void k_bispec_reduce(const float *__restrict__ part, const double *__restrict__ ppart, int ntiles,
                                                              int nfc, int nb, int first, double *__restrict__ acc, double *__restrict__ p64) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ne = (int64_t)ntiles * BS_PART;
    if (gid < ne) {
        const int64_t tile = gid / BS_PART, e = gid - tile * BS_PART;
        const float *p = part + tile * nfc * BS_PART + e;
        double sum = first ? 0.0 : acc[gid];
        for (int c = 0; c < nfc; ++c) sum += (double)p[(int64_t)c * BS_PART];
        acc[gid] = sum;
    } else if (gid - ne < nb) {
        const int s = (int)(gid - ne);
        double sum = first ? 0.0 : p64[s];
        for (int c = 0; c < nfc; ++c) sum += ppart[(int64_t)c * nb + s];
        p64[s] = sum;
    }
}

// the nb x nb outputs: B = acc / M (complex128), b2 = |B|^2 / (D P[s]) (0 where D P = 0), NaN outside 0 <= s < nb; the auto case
// holds only j <= i tiles and reads (j, i) for j > i -- the same float64 sums, so the result is exactly symmetric
static __global__ __launch_bounds__(256) void k_bispec_finish(const double *__restrict__ acc, const double *__restrict__ p64,
                                                              const int *__restrict__ tmap, int ntd, int nb, int c0, int sym,
                                                              int64_t M, double2 *__restrict__ B, double *__restrict__ b2,
                                                              double *__restrict__ pzz) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double inv = 1.0 / (double)M;
    if (pzz != nullptr && gid < nb) pzz[gid] = p64[gid] * inv;
    if (gid >= (int64_t)nb * nb) return;
    const int i = (int)(gid / nb), j = (int)(gid - (int64_t)i * nb);
    const int s = i + j - c0;
    if (s < 0 || s >= nb) {
        B[gid] = make_double2(__builtin_nan(""), __builtin_nan(""));
        b2[gid] = __builtin_nan("");
        return;
    }
    const int ii = (sym && j > i) ? j : i, jj = (sym && j > i) ? i : j;
    const int tile = tmap[(ii / BS_T) * ntd + jj / BS_T];
    const double *a = acc + (int64_t)tile * BS_PART + (ii % BS_T) * BS_T + jj % BS_T;
    const double re = a[0] * inv, im = a[BS_T * BS_T] * inv, d = a[2 * BS_T * BS_T] * inv;
    const double den = d * (p64[s] * inv);
    B[gid] = make_double2(re, im);
    b2[gid] = den > 0.0 ? (re * re + im * im) / den : 0.0;
}

// trend records of the frames [f0, ...): a line m + s t over the whole record, evaluated from sample off = f0 hop on
static __global__ void k_bispec_trend_shift(const float *__restrict__ src, float *__restrict__ dst, int nrec, int64_t off) {
    const int k = threadIdx.x;
    if (k >= nrec) return;
    const float *s = src + 4 * k;
    float *d = dst + 4 * k;
    d[0] = (float)((double)s[0] + (double)s[2] * (double)off);
    d[1] = (float)((double)s[1] + (double)s[3] * (double)off);
    d[2] = s[2];
    d[3] = s[3];
}

int bispec_tile_dim() { return BS_T; }
int bispec_frame_chunk() { return BS_FC; }
size_t bispec_part_floats() { return BS_PART; }

int launch_bispec_tile(LaunchCtx c, const cf *X, const cf *Y, const cf *Z, int nb, int c0, int64_t m, const int2 *tiles, int ntiles,
                       float *part) {
    const int nfc = (int)((m + BS_FC - 1) / BS_FC);
    hipLaunchKernelGGL(k_bispec_tile, dim3(ntiles, nfc), dim3(256), 0, c.stream, X, Y, Z, nb, c0, m, tiles, nfc, part);
    return 0;
}

int launch_bispec_pzz(LaunchCtx c, const cf *Z, int nb, int64_t m, double *ppart) {
    const int nfc = (int)((m + BS_FC - 1) / BS_FC);
    hipLaunchKernelGGL(k_bispec_pzz, dim3((nb + 255) / 256, nfc), dim3(256), 0, c.stream, Z, nb, m, ppart);
    return 0;
}

int launch_bispec_reduce(LaunchCtx c, const float *part, const double *ppart, int ntiles, int64_t m, int nb, int first, double *acc,
                         double *p64) {
    const int nfc = (int)((m + BS_FC - 1) / BS_FC);
    const int64_t n = (int64_t)ntiles * BS_PART + nb;
    hipLaunchKernelGGL(k_bispec_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, part, ppart, ntiles, nfc, nb, first,
                       acc, p64);
    return 0;
}

int launch_bispec_finish(LaunchCtx c, const double *acc, const double *p64, const int *tmap, int ntd, int nb, int c0, int sym, int64_t M,
                         void *B, double *b2, double *pzz) {
    const int64_t n = (int64_t)nb * nb;
    hipLaunchKernelGGL(k_bispec_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, acc, p64, tmap, ntd, nb, c0, sym, M,
                       (double2 *)B, b2, pzz);
    return 0;
}

int launch_bispec_trend_shift(LaunchCtx c, const float *src, float *dst, int nrec, int64_t off) {
    hipLaunchKernelGGL(k_bispec_trend_shift, dim3(1), dim3(64), 0, c.stream, src, dst, nrec, off);
    return 0;
}

}   // namespace sp
