// k_wbic.hip -- wavelet bispectrum / bicoherence (van Milligen, Hidalgo & Sanchez 1995): the contraction over time of wavelet transforms
//   B(i, j) = (1/T) sum_n X[i][n] Y[j][n] conj(Z[m][n]),  D(i, j) = (1/T) sum_n |X[i][n] Y[j][n]|^2,  P(m) = (1/T) sum_n |Z[m][n]|^2,
//   m = i + j + k_lo  (row i is the frequency (k_lo + i) df, so the frequencies of i and j add up to that of m)
// over the samples of a block.  X, Y, Z are read as k_cwt writes them, scale-major [S][ld] complex64: no transposed copy.
#include "launch.h"
namespace sp {

// k_wbic_tile: one workgroup = one 64 x 64 tile of (i, j) pairs x one group of <= WBIC_GROUP consecutive samples of one cell.
// 256 threads, 4 x 4 pairs per thread as in k_bispec_tile: i = i0 + 4 (t & 15) + a, j = j0 + 4 (t >> 4) + b, so a thread's 16 sums
// need 4 X, 4 Y and the 7 Z at m0 + 0 .. 6 of every sample.  Samples are staged in LDS WB_NB at a time, double-buffered: a thread
// fetches its 8 values of the next batch into registers while it computes the current one, so there is one barrier per batch.
// Staging: thread t takes sample t & 7 of the rows (t >> 3) + 32 r, r = 0 .. 7 (r < 2: X, r < 4: Y, else Z), so the 8 lanes of a row
// load 64 contiguous bytes of it.  LDS image of one sample (WB_STRIDE slots of 8 bytes):
//   [0, 64)    X, split so that the 16 lanes of a ds_read_b128 lane group read 256 contiguous bytes: slot 2q + r holds X[4q + r]
//              for r < 2, slot 32 + 2q + r - 2 holds X[4q + r] for r >= 2
//   [64, 128)  Y[j0 .. j0 + 63]   (4 distinct addresses per wave: broadcast)
//   [128, 256) Z[i0 + j0 + k_lo .. + 127]
//   WB_STRIDE = 258: the 16 lanes of a ds_write_b64 group (two rows x 8 samples) then fall on 16 different slots modulo 16, that is
//   on the 32 banks once each; 258 * 8 bytes keeps every image 16-byte aligned for the ds_read_b128.
// Rows outside [0, S) and samples outside the group are staged as 0 and add nothing: the pairs outside the valid region of a
// boundary tile end with B = 0 and are replaced by NaN in k_wbic_finish.
// Output: this (tile, group)'s fp32 sums, part[(tile * ngroups + group)][3][64 * 64] (Re B, Im B, D), summed in float64 by
// k_wbic_cells -- no atomics, a fixed order, deterministic.
#define WB_NB 8
#define WB_STRIDE 258

static __global__ __launch_bounds__(256) void k_wbic_tile(const cf *__restrict__ X, const cf *__restrict__ Y, const cf *__restrict__ Z,
                                                          int S, int k_lo, int64_t ld, int64_t shift,
                                                          const WbicGroup *__restrict__ groups, const int2 *__restrict__ tiles,
                                                          float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) cf sh[2][WB_NB][WB_STRIDE];
    const int tid = threadIdx.x;
    const int2 tl = tiles[blockIdx.x];
    const int i0 = tl.x * WBIC_TILE, j0 = tl.y * WBIC_TILE;
    const WbicGroup gr = groups[blockIdx.y];
    const int64_t c0 = gr.start - shift, c1 = c0 + gr.len;
    // this thread's staging slots: sample fs of 8 rows, each with its source, its offset (-1: outside the transform) and LDS position
    const int fs = tid & 7, rs = tid >> 3;
    const cf *src[8];
    int64_t off[8];
    int pos[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int slot = rs + 32 * r;
        int row;
        if (r < 2) {
            src[r] = X;
            row = i0 + slot;
            const int q = slot >> 2, rr = slot & 3;
            pos[r] = (rr < 2 ? 0 : 32) + 2 * q + (rr & 1);
        } else if (r < 4) {
            src[r] = Y;
            row = j0 + slot - 64;
            pos[r] = slot;
        } else {
            src[r] = Z;
            row = i0 + j0 + k_lo + slot - 128;
            pos[r] = slot;
        }
        off[r] = (row >= 0 && row < S) ? (int64_t)row * ld : -1;
    }
    const int ib = 4 * (tid & 15), jb = 4 * (tid >> 4);
    float bre[4][4], bim[4][4], dd[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) bre[a][b] = bim[a][b] = dd[a][b] = 0.f;

    cf st[8];
    auto fetch = [&](int64_t nb) {
        const int64_t n = nb + fs;
#pragma unroll
        for (int r = 0; r < 8; ++r) st[r] = (off[r] >= 0 && n < c1) ? src[r][off[r] + n] : mk(0.f, 0.f);
    };
    fetch(c0);
    int buf = 0;
    for (int64_t nb = c0; nb < c1; nb += WB_NB) {
#pragma unroll
        for (int r = 0; r < 8; ++r) sh[buf][fs][pos[r]] = st[r];
        __syncthreads();
        if (nb + WB_NB < c1) fetch(nb + WB_NB);     // in flight while this batch is computed
#pragma unroll 2
        for (int f = 0; f < WB_NB; ++f) {
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
    float *out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * WBIC_PART;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int o = (ib + a) * WBIC_TILE + jb;
        *reinterpret_cast<float4 *>(out + o) = make_float4(bre[a][0], bre[a][1], bre[a][2], bre[a][3]);
        *reinterpret_cast<float4 *>(out + WBIC_TILE * WBIC_TILE + o) = make_float4(bim[a][0], bim[a][1], bim[a][2], bim[a][3]);
        *reinterpret_cast<float4 *>(out + 2 * WBIC_TILE * WBIC_TILE + o) = make_float4(dd[a][0], dd[a][1], dd[a][2], dd[a][3]);
    }
}

// ppart[group][m] = sum over the group's samples of |Z[m][n]|^2 in float64: a wave per row, lane l takes the samples l, l + 64, .. in
// ascending order, lane 0 adds the 64 sums in ascending order
static __global__ __launch_bounds__(256) void k_wbic_pz(const cf *__restrict__ Z, int S, int64_t ld, int64_t shift,
                                                        const WbicGroup *__restrict__ groups, double *__restrict__ ppart) {
    __shared__ double sums[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = blockIdx.x * 4 + (tid >> 6);
    const WbicGroup gr = groups[blockIdx.y];
    const int64_t c0 = gr.start - shift, c1 = c0 + gr.len;
    double acc = 0.0;
    if (m < S) {
        const cf *__restrict__ zr = Z + (int64_t)m * ld;
        for (int64_t n = c0 + lane; n < c1; n += 64) {
            const cf z = zr[n];
            acc += (double)z.x * z.x + (double)z.y * z.y;
        }
    }
    sums[tid] = acc;
    __syncthreads();
    if (lane == 0 && m < S) {
        double tot = 0.0;
        for (int l = 0; l < 64; ++l) tot += sums[tid + l];
        ppart[(int64_t)blockIdx.y * S + m] = tot;
    }
}

// acc[cell][tile][3][4096] += the partials of the cell's groups among gA .. gB - 1, pcell[cell][S] += their ppart: float64, groups in
// ascending order, for the cells cell0 .. cell0 + ncells - 1 (the ones the pass touched)
static __global__ __launch_bounds__(256) void k_wbic_cells(const float *__restrict__ part, const double *__restrict__ ppart,
                                                           const int *__restrict__ gfirst, int64_t cell0, int64_t ncells, int64_t gA,
                                                           int64_t gB, int ntiles, int S, double *__restrict__ acc,
                                                           double *__restrict__ pcell) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (int64_t)ntiles * WBIC_PART, ne = ncells * per, ng = gB - gA;
    if (gid < ne) {
        const int64_t cl = gid / per, e = gid - cl * per;
        const int64_t tile = e / WBIC_PART, ee = e - tile * WBIC_PART;
        const int64_t c = cell0 + cl;
        const int64_t g0 = gfirst[c] > gA ? gfirst[c] : gA, g1 = gfirst[c + 1] < gB ? gfirst[c + 1] : gB;
        double *a = acc + (c * ntiles + tile) * WBIC_PART + ee;
        double sum = *a;
        for (int64_t gq = g0; gq < g1; ++gq) sum += (double)part[(tile * ng + (gq - gA)) * WBIC_PART + ee];
        *a = sum;
    } else if (gid - ne < ncells * S) {
        const int64_t r = gid - ne, cl = r / S, m = r - cl * S;
        const int64_t c = cell0 + cl;
        const int64_t g0 = gfirst[c] > gA ? gfirst[c] : gA, g1 = gfirst[c + 1] < gB ? gfirst[c + 1] : gB;
        double sum = pcell[c * S + m];
        for (int64_t gq = g0; gq < g1; ++gq) sum += ppart[(gq - gA) * S + m];
        pcell[c * S + m] = sum;
    }
}

// the nblocks x S x S outputs: block b is the sum of the cells b .. b + cpb - 1 in ascending order; B = sum / T (complex128),
// b2 = |B|^2 / (D P[m]) (0 where D P = 0), NaN where m = i + j + k_lo >= S; the auto form holds only tj <= ti tiles and reads (j, i) for
// j > i -- the same float64 sums, so the result is exactly symmetric
static __global__ __launch_bounds__(256) void k_wbic_finish(const double *__restrict__ acc, const double *__restrict__ pcell,
                                                            const int *__restrict__ tmap, int ntd, int ntiles, int S, int k_lo, int sym,
                                                            int64_t nblocks, int64_t cpb, int64_t T, double2 *__restrict__ B,
                                                            double *__restrict__ b2, double *__restrict__ P) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t SS = (int64_t)S * S;
    if (gid >= nblocks * SS) return;
    const double inv = 1.0 / (double)T;
    const int64_t b = gid / SS, r = gid - b * SS;
    if (r < S) {
        double p = 0.0;
        for (int64_t c = b; c < b + cpb; ++c) p += pcell[c * S + r];
        P[b * S + r] = p * inv;
    }
    const int i = (int)(r / S), j = (int)(r - (int64_t)i * S);
    const int m = i + j + k_lo;
    if (m >= S) {
        B[gid] = make_double2(__builtin_nan(""), __builtin_nan(""));
        b2[gid] = __builtin_nan("");
        return;
    }
    const int ii = (sym && j > i) ? j : i, jj = (sym && j > i) ? i : j;
    const int tile = tmap[(ii / WBIC_TILE) * ntd + jj / WBIC_TILE];
    const int64_t e = (int64_t)(ii % WBIC_TILE) * WBIC_TILE + jj % WBIC_TILE;
    double re = 0.0, im = 0.0, d = 0.0, p = 0.0;
    for (int64_t c = b; c < b + cpb; ++c) {
        const double *a = acc + (c * ntiles + tile) * WBIC_PART + e;
        re += a[0];
        im += a[WBIC_TILE * WBIC_TILE];
        d += a[2 * WBIC_TILE * WBIC_TILE];
        p += pcell[c * S + m];
    }
    re *= inv;
    im *= inv;
    const double den = (d * inv) * (p * inv);
    B[gid] = make_double2(re, im);
    b2[gid] = den > 0.0 ? (re * re + im * im) / den : 0.0;
}

int launch_wbic_tile(LaunchCtx c, const cf *X, const cf *Y, const cf *Z, int S, int k_lo, int64_t ld, int64_t shift, const WbicGroup *groups,
                     int ngroups, const int2 *tiles, int ntiles, float *part) {
    if (S < 1 || S > WBIC_MAX_S || k_lo < 1 || ld < 1 || ngroups < 1 || ngroups > WBIC_MAX_PASS_GROUPS || ntiles < 1) return -1;
    hipLaunchKernelGGL(k_wbic_tile, dim3((unsigned)ntiles, (unsigned)ngroups), dim3(256), 0, c.stream, X, Y, Z, S, k_lo, ld, shift, groups,
                       tiles, part);
    return 0;
}

int launch_wbic_pz(LaunchCtx c, const cf *Z, int S, int64_t ld, int64_t shift, const WbicGroup *groups, int ngroups, double *ppart) {
    if (S < 1 || S > WBIC_MAX_S || ld < 1 || ngroups < 1 || ngroups > WBIC_MAX_PASS_GROUPS) return -1;
    hipLaunchKernelGGL(k_wbic_pz, dim3((unsigned)((S + 3) / 4), (unsigned)ngroups), dim3(256), 0, c.stream, Z, S, ld, shift, groups, ppart);
    return 0;
}

int launch_wbic_cells(LaunchCtx c, const float *part, const double *ppart, const int *gfirst, int64_t cell0, int64_t ncells, int64_t gA,
                      int64_t gB, int ntiles, int S, double *acc, double *pcell) {
    const int64_t n = ncells * ((int64_t)ntiles * WBIC_PART + S);
    if (ncells < 1 || gB <= gA || ntiles < 1 || (n + 255) / 256 > INT_MAX) return -1;
    hipLaunchKernelGGL(k_wbic_cells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, part, ppart, gfirst, cell0, ncells, gA, gB,
                       ntiles, S, acc, pcell);
    return 0;
}

int launch_wbic_finish(LaunchCtx c, const double *acc, const double *pcell, const int *tmap, int ntd, int ntiles, int S, int k_lo, int sym,
                       int64_t nblocks, int64_t cpb, int64_t T, void *B, double *b2, double *P) {
    const int64_t n = nblocks * (int64_t)S * S;
    if (nblocks < 1 || cpb < 1 || T < 1 || (n + 255) / 256 > INT_MAX) return -1;
    hipLaunchKernelGGL(k_wbic_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, acc, pcell, tmap, ntd, ntiles, S, k_lo, sym,
                       nblocks, cpb, T, (double2 *)B, b2, P);
    return 0;
}

}   // namespace sp
