// k_nufft.hip -- the non-uniform FFT of type 1: the spectrum of an unevenly sampled complex record on a uniform frequency grid,
//   F_r[m] = sum_j c_r[j] e((f0 + m df) tau_j),  m = 0 .. M - 1,  e(p) = exp(2 pi i p),  tau = t - t_ref
// (include/spectral_nufft.h; the arithmetic and its reasons: nufft_plan.h), and with it the Lomb-Scargle sums of k_lomb.hip on a
// uniform grid in O(N w + M log M).  The samples are spread onto a fine grid of nf cells with a kernel of NUFFT_W cells, one long
// transform runs over the grid, and a per-bin division by the kernel's transform follows.
// Kernels:
//   k_nufft_prep    per sample, in float64: the position p = frac(q tau), the first cell of its footprint and the float32 offset in
//           it, the centre phase e(fc tau) rounded to float32, and the sample counted into the tiles its footprint touches (integer
//           atomics on counters: the only global atomics here, and none on data).
//   k_nufft_rowmax, k_nufft_rowshift  per row the largest component magnitude (over runs of samples, then over the runs), which with N
//           gives the row's fixed-point shift (nufft_shift): a maximum, so that no order of the samples changes it.  Also the check
//           for strengths that are not finite.
//   k_nufft_scan, k_nufft_fill   the counts scanned into list offsets, and every sample entered into the list of its one or two tiles
//           (a footprint that crosses a tile seam or the periodic end of the grid is entered in both).  The order inside a list is
//           whatever the atomics made it; nothing below depends on it.
//   k_nufft_spread  one workgroup per (tile, group of NUFFT_RG rows).  int64 sums [rows][NUFFT_TILE][2] live in LDS; lanes take
//           samples from the tile's list, evaluate the NUFFT_W kernel values once per sample for all rows of the group and add
//           llrint(v 2^shift) onto the cells inside the tile with 64-bit LDS integer adds.  Integer sums are exact, so any order of
//           the samples gives the same bits.  After a barrier the tile is converted to float32 and stored whole: every cell of the
//           grid is written exactly once, by the workgroup that owns it, empty tiles as zeros (no memset, no global data atomics).
//   k_nufft_pick    bin k = m - M / 2 of the transformed grid divided by the kernel's transform, a Gauss-Legendre sum in float64:
//           complex64 for sp_nufft1, float64 in the layout of sp_lomb_sums for sp_lomb_sums_grid.
// No float atomics anywhere: two calls agree bitwise, and so do two orders of the samples.
#include "launch.h"
namespace sp {

static __device__ __forceinline__ float2 nufft_strength(const NufftSrc &s, int64_t row, int64_t j) {
    if (s.c) {
        const cf v = s.c[row * s.c_ld + j];
        return make_float2(v.x, v.y);
    }
    if (row == 0) return make_float2(s.head[j].w, 0.f);
    const int64_t q = row - 1;
    return make_float2(s.wy[(q / s.R) * s.npad * s.RP + j * s.RP + q % s.R], 0.f);
}

// the tile counters of a workgroup's NUFFT_PREP_SPT * 256 samples are gathered in LDS first where the tiles fit (NUFFT_HIST), and added
// to the global counters once per tile: samples in time order land on the tiles in no order at all, and with few tiles a global
// atomic per sample serialises on them (profiles/nufft_kernel_resources.txt)
static __global__ __launch_bounds__(256) void k_nufft_prep(NufftPrepArgs a) {
    __shared__ unsigned hist[2 * NUFFT_HIST];
    const int tid = threadIdx.x;
    const bool local = a.tiles <= NUFFT_HIST;
    const int nbins = (int)(a.sets * a.tiles);
    if (local) {
        for (int i = tid; i < nbins; i += 256) hist[i] = 0u;
        __syncthreads();
    }
    for (int u = 0; u < NUFFT_PREP_SPT; ++u) {
        const int64_t j = ((int64_t)blockIdx.x * NUFFT_PREP_SPT + u) * 256 + tid;
        if (j >= a.N) break;
        const double tau = a.t[j] - a.t_ref;
        for (int s = 0; s < a.sets; ++s) {
            double p = nufft_frac(a.q[s], tau), ph = nufft_frac(a.fc[s], tau);
            if (!(p >= 0.0 && p <= 1.0) || !(ph >= 0.0 && ph <= 1.0)) {         // a time that is not finite, or a product beyond float64
                a.status[0] = 1;
                p = ph = 0.0;
            }
            const NufftCell cl = nufft_cell(p, a.nf);
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            a.rec[(int64_t)s * a.N + j] = NufftRec{(int)cl.i0, cl.dx, (float)cs, (float)sn};
            int64_t ta, tb;
            nufft_tiles(cl.i0, a.nf, &ta, &tb);
            unsigned *cnt = local ? hist + s * a.tiles : a.count + (int64_t)s * a.tiles;
            atomicAdd(cnt + ta, 1u);
            if (tb != ta) atomicAdd(cnt + tb, 1u);
        }
    }
    if (local) {
        __syncthreads();
        for (int i = tid; i < nbins; i += 256)
            if (hist[i]) atomicAdd(a.count + i, hist[i]);
    }
}

// row = row0 + blockIdx.y: part[row][blockIdx.x] = the largest |re|, |im| of the row over the block's run of samples; a strength that is not finite sets status[1]
static __global__ __launch_bounds__(256) void k_nufft_rowmax(NufftSrc src, int64_t row0, int64_t N, int64_t len, float *part, int *status) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int64_t row = row0 + blockIdx.y;
    const int64_t n0 = blockIdx.x * len, n1 = n0 + len < N ? n0 + len : N;
    float m = 0.f;
    bool bad = false;
    for (int64_t j = n0 + tid; j < n1; j += 256) {
        const float2 v = nufft_strength(src, row, j);
        bad |= !isfinite(v.x) || !isfinite(v.y);
        m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
    }
    if (bad) status[1] = 1;
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
        __syncthreads();
    }
    if (tid == 0) part[row * gridDim.x + blockIdx.x] = red[0];
}
// shift[row] from the row's largest magnitude (0 for a row of zeros): a maximum, so no order of the samples changes it
static __global__ __launch_bounds__(256) void k_nufft_rowshift(const float *part, int blocks, int64_t rows, int64_t N, int *shift) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float top = 0.f;
    for (int b = 0; b < blocks; ++b) top = fmaxf(top, part[row * blocks + b]);
    int e = 0;
    const bool ok = top > 0.f && isfinite(top);
    if (ok) (void)frexpf(top, &e);
    shift[row] = ok ? nufft_shift(e, N) : 0;
}

// off[i] = the counts before tile i, off[tiles] = their sum; the counts are zeroed: they become the fill's cursors
static __global__ __launch_bounds__(1024) void k_nufft_scan(unsigned *count, int64_t *off, int64_t tiles) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (tiles + 1023) / 1024;
    const int64_t i0 = tid * per, i1 = i0 + per < tiles ? i0 + per : tiles;
    int64_t s = 0;
    for (int64_t i = i0; i < i1; ++i) s += count[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int k = 0; k < 1024; ++k) {
            const int64_t v = part[k];
            part[k] = run;
            run += v;
        }
        off[tiles] = run;
    }
    __syncthreads();
    int64_t run = part[tid];
    for (int64_t i = i0; i < i1; ++i) {
        off[i] = run;
        run += count[i];
        count[i] = 0;
    }
}

// as k_nufft_prep counts: where the tiles fit, a workgroup counts its samples per tile in LDS, reserves a run of every tile's list with
// one global add per tile, and deals the slots of the run out with LDS adds
static __global__ __launch_bounds__(256) void k_nufft_fill(const NufftRec *rec, int64_t N, int64_t nf, unsigned *cursor, const int64_t *off,
                                                           int *list) {
    __shared__ unsigned hist[NUFFT_HIST], base[NUFFT_HIST];
    const int tid = threadIdx.x;
    const int tiles = (int)(nf / NUFFT_TILE);
    const bool local = tiles <= NUFFT_HIST;
    if (local) {
        for (int i = tid; i < tiles; i += 256) hist[i] = 0u;
        __syncthreads();
        for (int u = 0; u < NUFFT_PREP_SPT; ++u) {
            const int64_t j = ((int64_t)blockIdx.x * NUFFT_PREP_SPT + u) * 256 + tid;
            if (j >= N) break;
            int64_t ta, tb;
            nufft_tiles(rec[j].i0, nf, &ta, &tb);
            atomicAdd(hist + ta, 1u);
            if (tb != ta) atomicAdd(hist + tb, 1u);
        }
        __syncthreads();
        for (int i = tid; i < tiles; i += 256) {
            const unsigned c = hist[i];
            base[i] = c ? atomicAdd(cursor + i, c) : 0u;
            hist[i] = 0u;
        }
        __syncthreads();
    }
    for (int u = 0; u < NUFFT_PREP_SPT; ++u) {
        const int64_t j = ((int64_t)blockIdx.x * NUFFT_PREP_SPT + u) * 256 + tid;
        if (j >= N) break;
        int64_t ta, tb;
        nufft_tiles(rec[j].i0, nf, &ta, &tb);
        list[off[ta] + (local ? base[ta] + atomicAdd(hist + ta, 1u) : atomicAdd(cursor + ta, 1u))] = (int)j;
        if (tb != ta) list[off[tb] + (local ? base[tb] + atomicAdd(hist + tb, 1u) : atomicAdd(cursor + tb, 1u))] = (int)j;
    }
}

static __device__ __forceinline__ unsigned long long nufft_fixed(float v, int sh) {
    return (unsigned long long)llrint(ldexp((double)v, sh));
}

static __global__ __launch_bounds__(256) void k_nufft_spread(NufftSpreadArgs a) {
    extern __shared__ unsigned long long acc[];                  // [rows of the group][NUFFT_TILE][2]
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int r0 = blockIdx.y * NUFFT_RG;                        // first row of the group inside the pass
    const int nr = a.nrows - r0 < NUFFT_RG ? a.nrows - r0 : NUFFT_RG;
    for (int i = tid; i < nr * NUFFT_TILE * 2; i += 256) acc[i] = 0ull;
    int sh[NUFFT_RG];
#pragma unroll
    for (int r = 0; r < NUFFT_RG; ++r) sh[r] = r < nr ? a.shift[a.row0 + r0 + r] : 0;
    __syncthreads();
    const int64_t c0 = tile * NUFFT_TILE;
    for (int64_t e = a.off[tile] + tid; e < a.off[tile + 1]; e += 256) {
        const int64_t j = a.list[e];
        const NufftRec rc = a.rec[j];
        float kv[NUFFT_W];
        int loc[NUFFT_W];
#pragma unroll
        for (int l = 0; l < NUFFT_W; ++l) {
            kv[l] = nufft_phi((rc.dx + (float)(l - NUFFT_W / 2)) * (2.f / NUFFT_W));
            const int64_t cell = (((int64_t)rc.i0 + l) & (a.nf - 1)) - c0;
            loc[l] = cell >= 0 && cell < NUFFT_TILE ? (int)cell : -1;        // cells of the neighbouring tile are that tile's
        }
#pragma unroll
        for (int r = 0; r < NUFFT_RG; ++r) {
            if (r >= nr) break;
            const float2 cv = nufft_strength(a.src, a.row0 + r0 + r, j);
            const float vr = cv.x * rc.pc - cv.y * rc.ps, vi = cv.x * rc.ps + cv.y * rc.pc;
            unsigned long long *dst = acc + (size_t)r * NUFFT_TILE * 2;
#pragma unroll
            for (int l = 0; l < NUFFT_W; ++l)
                if (loc[l] >= 0) {
                    atomicAdd(dst + 2 * loc[l], nufft_fixed(vr * kv[l], sh[r]));
                    atomicAdd(dst + 2 * loc[l] + 1, nufft_fixed(vi * kv[l], sh[r]));
                }
        }
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
        cf *g = a.grid + (int64_t)(r0 + r) * a.nf + c0;
        const unsigned long long *src = acc + (size_t)r * NUFFT_TILE * 2;
        for (int i = tid; i < NUFFT_TILE; i += 256)
            g[i] = mk((float)ldexp((double)(long long)src[2 * i], -sh[r]), (float)ldexp((double)(long long)src[2 * i + 1], -sh[r]));
    }
}

// bin k = m - M / 2 of the rows of the transformed grid over the kernel's transform, formed once per bin; dst row r at dst + r * row_ld,
// bin m `stride` elements on: complex64 (F32) or two float64
template <bool F32>
static __global__ __launch_bounds__(256) void k_nufft_pick(const cf *__restrict__ grid, int64_t nf, int64_t M, int64_t nrows, NufftQuad q,
                                                           void *dst, int64_t row_ld, int64_t stride) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int64_t k = m - M / 2;
    const double inv = 1.0 / nufft_phihat(q, k);
    const cf *src = grid + (k < 0 ? k + nf : k);
    for (int64_t r = 0; r < nrows; ++r) {
        const cf v = src[r * nf];
        const int64_t o = r * row_ld + m * stride;
        if constexpr (F32) {
            ((cf *)dst)[o] = mk((float)((double)v.x * inv), (float)((double)v.y * inv));
        } else {
            ((double *)dst)[o] = (double)v.x * inv;
            ((double *)dst)[o + 1] = (double)v.y * inv;
        }
    }
}

static bool nufft_src_ok(const NufftSrc &s) {
    return s.c ? s.c_ld >= 1 : (s.head && s.npad >= 1 && (s.wy ? s.R >= 1 && s.RP >= s.R : true));
}

int launch_nufft_prep(LaunchCtx c, const NufftPrepArgs &a) {
    if (a.N < 1 || a.N >= ((int64_t)1 << 31) || a.sets < 1 || a.sets > 2 || a.nf < NUFFT_TILE || a.nf > NUFFT_MAX_NF || a.nf % NUFFT_TILE ||
        a.tiles != a.nf / NUFFT_TILE || !a.t || !a.rec || !a.count || !a.status)
        return -1;
    hipLaunchKernelGGL(k_nufft_prep, dim3((unsigned)((a.N + 256 * NUFFT_PREP_SPT - 1) / (256 * NUFFT_PREP_SPT))), dim3(256), 0, c.stream, a);
    return 0;
}

int launch_nufft_rowshift(LaunchCtx c, const NufftSrc &src, int64_t rows, int64_t N, float *part, int *shift, int *status) {
    if (rows < 1 || rows > 65536 || N < 1 || !nufft_src_ok(src) || !part || !shift || !status) return -1;
    const int blocks = nufft_rowmax_blocks(N);
    const int64_t len = (N + blocks - 1) / blocks;
    for (int64_t r0 = 0; r0 < rows; r0 += 32768)          // 65536 rows (the weights' and 65535 of values) are more than a grid's y
        hipLaunchKernelGGL(k_nufft_rowmax, dim3((unsigned)blocks, (unsigned)(rows - r0 < 32768 ? rows - r0 : 32768)), dim3(256), 0, c.stream, src,
                           r0, N, len, part, status);
    hipLaunchKernelGGL(k_nufft_rowshift, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c.stream, part, blocks, rows, N, shift);
    return 0;
}

int launch_nufft_bin(LaunchCtx c, const NufftRec *rec, int64_t N, int64_t nf, unsigned *count, int64_t *off, int *list) {
    if (N < 1 || N >= ((int64_t)1 << 31) || nf < NUFFT_TILE || nf > NUFFT_MAX_NF || nf % NUFFT_TILE || !rec || !count || !off || !list) return -1;
    hipLaunchKernelGGL(k_nufft_scan, dim3(1), dim3(1024), 0, c.stream, count, off, nf / NUFFT_TILE);
    hipLaunchKernelGGL(k_nufft_fill, dim3((unsigned)((N + 256 * NUFFT_PREP_SPT - 1) / (256 * NUFFT_PREP_SPT))), dim3(256), 0, c.stream, rec, N, nf,
                       count, off, list);
    return 0;
}

int launch_nufft_spread(LaunchCtx c, const NufftSpreadArgs &a) {
    if (a.nrows < 1 || a.nrows > 65535 * NUFFT_RG || a.row0 < 0 || a.nf < NUFFT_TILE || a.nf > NUFFT_MAX_NF || a.nf % NUFFT_TILE ||
        !nufft_src_ok(a.src) || !a.rec || !a.off || !a.list || !a.shift || !a.grid)
        return -1;
    const int nr = a.nrows < NUFFT_RG ? a.nrows : NUFFT_RG;
    const size_t lds = (size_t)nr * NUFFT_TILE * 2 * sizeof(unsigned long long);
    static_assert((size_t)NUFFT_RG * NUFFT_TILE * 16 <= 64 * 1024, "the spread kernel's sums stay within the LDS a launch gets unasked");
    hipLaunchKernelGGL(k_nufft_spread, dim3((unsigned)(a.nf / NUFFT_TILE), (unsigned)((a.nrows + NUFFT_RG - 1) / NUFFT_RG)), dim3(256), lds,
                       c.stream, a);
    return 0;
}

int launch_nufft_pick(LaunchCtx c, const cf *grid, int64_t nf, int64_t M, int64_t nrows, const NufftQuad &q, bool f32, void *dst,
                      int64_t row_ld, int64_t stride) {
    if (M < 1 || M > NUFFT_MAX_M || nf < 2 * M || nrows < 1 || nrows > 65535 || !grid || !dst) return -1;
    const dim3 g((unsigned)((M + 255) / 256));
    if (f32) hipLaunchKernelGGL(k_nufft_pick<true>, g, dim3(256), 0, c.stream, grid, nf, M, nrows, q, dst, row_ld, stride);
    else hipLaunchKernelGGL(k_nufft_pick<false>, g, dim3(256), 0, c.stream, grid, nf, M, nrows, q, dst, row_ld, stride);
    return 0;
}

}   // namespace sp
