// k_nufft2.hip -- the non-uniform FFT of type 2: a spectrum on a uniform frequency grid evaluated at uneven times,
//   c_r[j] = sum_m F_r[m] e(sign (f0 + m df) tau_j),  j = 0 .. N - 1,  e(p) = exp(2 pi i p),  tau = t - t_ref
// (include/spectral_nufft2.h), the adjoint of k_nufft.hip's transform and built from its parts: the prepared samples and tile lists
// of k_nufft_prep / k_nufft_scan / k_nufft_fill, the kernel phi and its transform of nufft_plan.h, the same fine grid of nf cells and
// the same long transform.  The modes are divided by the kernel's transform and placed on the fine grid, one forward transform runs
// over it, and every sample gathers the NUFFT_W cells of its footprint.
// Kernels:
//   k_nufft2_place   one lane per cell of the fine grid: cell (m - M / 2) mod nf takes F_r[m] / phihat(m - M / 2), the division in
//           float64 and formed once per cell for all rows of the pass, every other cell zero.  Every cell is written once: no memset.
//   k_nufft2_interp  one workgroup per (tile, group of NUFFT2_RG rows).  The tile's NUFFT_TILE cells and the NUFFT_W - 1 after them
//           (wrapped at nf) of every row of the group are staged in LDS with 16-byte loads; lanes take samples from the tile's list,
//           skip those whose first cell belongs to the tile before (they are that tile's), evaluate the NUFFT_W kernel values once
//           per sample and sum kernel value x cell per row in float32 in the order l = 0 .. NUFFT_W - 1, multiply by the sample's
//           centre phase and store: one store per (row, sample).  A tile with an empty list returns before it stages anything.
// No atomics of any kind: an output depends on its own sample alone, so two calls agree bitwise and a permutation of the samples
// permutes the outputs bit for bit.
#include "launch.h"
namespace sp {

static __global__ __launch_bounds__(256) void k_nufft2_place(const cf *__restrict__ F, int64_t F_ld, int64_t M, int64_t nrows, int64_t nf,
                                                             NufftQuad q, cf *__restrict__ grid) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= nf) return;
    const int64_t k = cell < nf / 2 ? cell : cell - nf;
    const int64_t m = k + M / 2;
    if (m < 0 || m >= M) {
        for (int64_t r = 0; r < nrows; ++r) grid[r * nf + cell] = mk(0.f, 0.f);
        return;
    }
    const double inv = 1.0 / nufft_phihat(q, k);
    for (int64_t r = 0; r < nrows; ++r) {
        const cf v = F[r * F_ld + m];
        grid[r * nf + cell] = mk((float)((double)v.x * inv), (float)((double)v.y * inv));
    }
}

#ifdef NUFFT2_DIRECT
// The other form, built only with -DNUFFT2_DIRECT and kept for the comparison of profiles/nufft2_variants.txt: one lane per sample
// gathers its cells straight from the grid in L2, over all rows of the pass, with no staging and no lists.
static __global__ __launch_bounds__(256) void k_nufft2_interp(Nufft2InterpArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.N) return;
    const NufftRec rc = a.rec[j];
    float kv[NUFFT_W];
#pragma unroll
    for (int l = 0; l < NUFFT_W; ++l) kv[l] = nufft_phi((rc.dx + (float)(l - NUFFT_W / 2)) * (2.f / NUFFT_W));
    for (int r = 0; r < a.nrows; ++r) {
        const cf *g = a.grid + (int64_t)r * a.nf;
        float sr = 0.f, si = 0.f;
#pragma unroll
        for (int l = 0; l < NUFFT_W; ++l) {
            const cf v = g[((int64_t)rc.i0 + l) & (a.nf - 1)];
            sr += kv[l] * v.x;
            si += kv[l] * v.y;
        }
        a.out[(int64_t)r * a.out_ld + j] = mk(sr * rc.pc - si * rc.ps, sr * rc.ps + si * rc.pc);
    }
}
#else
static __global__ __launch_bounds__(256) void k_nufft2_interp(Nufft2InterpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 stg[];       // [rows of the group][NUFFT2_PITCH] cells, two to a float4
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t e0 = a.off[tile], e1 = a.off[tile + 1];
    if (e0 == e1) return;                                              // nothing lands here: the whole workgroup leaves
    const int r0 = blockIdx.y * NUFFT2_RG;                             // first row of the group inside the pass
    const int nr = a.nrows - r0 < NUFFT2_RG ? a.nrows - r0 : NUFFT2_RG;
    const int64_t c0 = tile * NUFFT_TILE;
    const int64_t c1 = (c0 + NUFFT_TILE) & (a.nf - 1);                 // the cells after the tile: the next tile's, or the grid's first
    constexpr int Q = NUFFT2_PITCH / 2;                                // float4 of a staged row: NUFFT_TILE / 2 of the tile, then 4 behind it
    for (int i = tid; i < nr * Q; i += 256) {
        const int r = i / Q, k = i - r * Q;
        const cf *row = a.grid + (int64_t)(r0 + r) * a.nf;
        const cf *src = k < NUFFT_TILE / 2 ? row + c0 + 2 * k : row + c1 + (2 * k - NUFFT_TILE);
        stg[i] = *(const float4 *)src;
    }
    __syncthreads();
    const cf *cells = (const cf *)stg;
    for (int64_t e = e0 + tid; e < e1; e += 256) {
        const int64_t j = a.list[e];
        const NufftRec rc = a.rec[j];
        if (rc.i0 / NUFFT_TILE != tile) continue;                      // listed here for its last cells: the tile before handles it
        const int loc = (int)(rc.i0 - c0);                             // 0 .. NUFFT_TILE - 1: the footprint ends before cell NUFFT2_PITCH - 1
        float kv[NUFFT_W];
#pragma unroll
        for (int l = 0; l < NUFFT_W; ++l) kv[l] = nufft_phi((rc.dx + (float)(l - NUFFT_W / 2)) * (2.f / NUFFT_W));
#pragma unroll
        for (int r = 0; r < NUFFT2_RG; ++r) {
            if (r >= nr) break;
            const cf *g = cells + r * NUFFT2_PITCH + loc;
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int l = 0; l < NUFFT_W; ++l) {
                const cf v = g[l];
                sr += kv[l] * v.x;
                si += kv[l] * v.y;
            }
            a.out[(int64_t)(r0 + r) * a.out_ld + j] = mk(sr * rc.pc - si * rc.ps, sr * rc.ps + si * rc.pc);
        }
    }
}

#endif

int launch_nufft2_place(LaunchCtx c, const cf *F, int64_t F_ld, int64_t M, int64_t nrows, int64_t nf, const NufftQuad &q, cf *grid) {
    if (M < 1 || M > NUFFT_MAX_M || F_ld < M || nf < 2 * M || nf < NUFFT_TILE || nf > NUFFT_MAX_NF || (nf & (nf - 1)) || nrows < 1 ||
        nrows > 65535 || !F || !grid)
        return -1;
    hipLaunchKernelGGL(k_nufft2_place, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, c.stream, F, F_ld, M, nrows, nf, q, grid);
    return 0;
}

int launch_nufft2_interp(LaunchCtx c, const Nufft2InterpArgs &a) {
    if (a.nrows < 1 || a.nrows > 65535 * NUFFT2_RG || a.N < 1 || a.N >= ((int64_t)1 << 31) || a.out_ld < a.N || a.nf < NUFFT_TILE ||
        a.nf > NUFFT_MAX_NF || (a.nf & (a.nf - 1)) || !a.grid || !a.rec || !a.off || !a.list || !a.out)
        return -1;
    static_assert(NUFFT2_PITCH >= NUFFT_TILE + NUFFT_W - 1 && NUFFT2_PITCH % 2 == 0 && NUFFT_TILE % 2 == 0, "a staged row holds the tile and the cells behind it, in float4s");
    static_assert((size_t)NUFFT2_RG * NUFFT2_PITCH * sizeof(cf) <= 64 * 1024, "the staged rows stay within the LDS a launch gets unasked");
    const int nr = a.nrows < NUFFT2_RG ? a.nrows : NUFFT2_RG;
    const size_t lds = (size_t)nr * NUFFT2_PITCH * sizeof(cf);
#ifdef NUFFT2_DIRECT
    (void)lds;
    hipLaunchKernelGGL(k_nufft2_interp, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, c.stream, a);
#else
    hipLaunchKernelGGL(k_nufft2_interp, dim3((unsigned)(a.nf / NUFFT_TILE), (unsigned)((a.nrows + NUFFT2_RG - 1) / NUFFT2_RG)), dim3(256), lds,
                       c.stream, a);
#endif
    return 0;
}

}   // namespace sp
