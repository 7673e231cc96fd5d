// k_csd.hip -- reference-vs-channels cross-spectral density launchers
#include "launch.h"
namespace sp {

// block sums of ONE real signal (the reference of the one-pass pair path): slice blockIdx.y of the hop-blocks b = 1 .. M writes
// out[slice][j] = sum_b (x[b H + j] - mu); k_cm_blocksums adds the slices in a fixed order (no atomics: reproducible)
static __global__ void k_colsum_real(const float *__restrict__ x, const float *__restrict__ trend, int H, int64_t M, cf *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= H) return;
    const float mu = trend[0];
    const int64_t per = (M + gridDim.y - 1) / gridDim.y;
    const int64_t b0 = 1 + (int64_t)blockIdx.y * per, b1 = b0 + per < M + 1 ? b0 + per : M + 1;
    double a = 0.0;
#pragma unroll 8
    for (int64_t b = b0; b < b1; ++b) a += (double)(x[b * H + j] - mu);
    out[(int64_t)blockIdx.y * H + j] = mk((float)a, 0.f);
}

// pyy[ch][slot] = (a[k] + a[n-k]) / 2,  pxy[ch][slot] = (A[k] + conj(A[n-k])) / 2, scaled / doubled per sidedness
// st_y != null (one-pass mean detrend): the channels were detrended by estimates mu0; with d = mean - mu0 (real), W = FFT(window),
// B = sum_g of the spectra (k_op_finish<EXPORT> states st_y[ch], st_x), M frames, nmean samples per signal:
//   sum |Y - dy W|^2 = a - 2 Re(conj(dy W) By) + M |dy W|^2,   sum (Y - dy W) conj(X - dx W) = A - dx conj(W) By - dy W conj(Bx) + M dx dy |W|^2
static __global__ __launch_bounds__(SP_FIN_BINS *SP_FIN_SLICES) void k_csd_pair_finish(const float *__restrict__ partial,
                                                                                 int64_t G, int n, int nch, int sided,
                                                                                 double scale, double *__restrict__ pyy,
                                                                                 double *__restrict__ pxy,
                                                                                 const double *__restrict__ st_y,
                                                                                 const double *__restrict__ st_x,
                                                                                 const cf *__restrict__ Wf,
                                                                                 const float *__restrict__ trend_x,
                                                                                 const float *__restrict__ trend_y, int64_t nmean,
                                                                                 int64_t M) {
    __shared__ double sh[6][SP_FIN_SLICES][SP_FIN_BINS];
    const int lane = threadIdx.x % SP_FIN_BINS, sl = threadIdx.x / SP_FIN_BINS;
    const int k = blockIdx.x * SP_FIN_BINS + lane;
    const int ch = blockIdx.y;
    const int nb = nbins_of(n, sided);
    double s[6] = {0, 0, 0, 0, 0, 0};       // a[k], a[km], Re A[k], Im A[k], Re A[km], Im A[km]
    const float *p = partial + (int64_t)ch * G * 3 * n;
    if (k < n) {
        const int km = k == 0 ? 0 : n - k;
        for (int64_t g = sl; g < G; g += SP_FIN_SLICES) {
            s[0] += (double)p[(g * 3 + 0) * n + k];
            s[1] += (double)p[(g * 3 + 0) * n + km];
            s[2] += (double)p[(g * 3 + 1) * n + k];
            s[3] += (double)p[(g * 3 + 2) * n + k];
            s[4] += (double)p[(g * 3 + 1) * n + km];
            s[5] += (double)p[(g * 3 + 2) * n + km];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) sh[j][sl][lane] = s[j];
    fin_reduce<6>(sh, sl, lane);
    if (sl == 0 && k < n) {
        const int slot = bin_slot(k, n, sided);
        if (slot >= 0) {
            double t[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) t[j] = sh[j][0][lane];
            const double m = 0.5 * scale * (bin_doubled(k, n, sided) ? 2.0 : 1.0);
            double cyy = 0.0, cr = 0.0, ci = 0.0;
            if (st_y) {
                const int64_t ss = (int64_t)5 * n + 8;
                const double *sy = st_y + ch * ss;
                const double dy = sy[5 * n + 3] / (double)nmean - (double)trend_y[4 * ch];
                const double dx = st_x[5 * n + 3] / (double)nmean - (double)trend_x[0];
                const double wr = Wf[k].x, wi = Wf[k].y, w2 = wr * wr + wi * wi;
                const double byr = sy[n + 2 * k], byi = sy[n + 2 * k + 1], bxr = st_x[n + 2 * k], bxi = st_x[n + 2 * k + 1];
                cyy = -2.0 * dy * (wr * byr + wi * byi) + (double)M * dy * dy * w2;
                cr = -dx * (wr * byr + wi * byi) - dy * (wr * bxr + wi * bxi) + (double)M * dx * dy * w2;
                ci = -dx * (wr * byi - wi * byr) - dy * (wi * bxr - wr * bxi);
            }
            pyy[(int64_t)ch * nb + slot] = (t[0] + t[1] + 2.0 * cyy) * m;
            pxy[((int64_t)ch * nb + slot) * 2] = (t[2] + t[4] + 2.0 * cr) * m;
            pxy[((int64_t)ch * nb + slot) * 2 + 1] = (t[3] - t[5] + 2.0 * ci) * m;
        }
    }
}

static __global__ __launch_bounds__(SP_FIN_BINS *SP_FIN_SLICES) void k_csd_rp_finish(const float *__restrict__ partial,
                                                                               int64_t G, int n, int nch, int sided,
                                                                               double scale, double *__restrict__ pxx,
                                                                               double *__restrict__ pyy,
                                                                               double *__restrict__ pxy) {
    __shared__ double sh[4][SP_FIN_SLICES][SP_FIN_BINS];
    const int lane = threadIdx.x % SP_FIN_BINS, sl = threadIdx.x / SP_FIN_BINS;
    const int k = blockIdx.x * SP_FIN_BINS + lane;
    const int ch = blockIdx.y;
    const int nb = nbins_of(n, sided);
    double s[4] = {0, 0, 0, 0};       // a[k], a[km], Re c[k], Im c[k]
    const float *p = partial + (int64_t)ch * G * 3 * n;
    if (k < n) {
        const int km = k == 0 ? 0 : n - k;
        for (int64_t g = sl; g < G; g += SP_FIN_SLICES) {
            s[0] += (double)p[(g * 3 + 0) * n + k];
            s[1] += (double)p[(g * 3 + 0) * n + km];
            s[2] += (double)p[(g * 3 + 1) * n + k];
            s[3] += (double)p[(g * 3 + 2) * n + k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[j][sl][lane] = s[j];
    fin_reduce<4>(sh, sl, lane);
    if (sl == 0 && k < n) {
        const int slot = bin_slot(k, n, sided);
        if (slot >= 0) {
            double t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = sh[j][0][lane];
            const double m = scale * (bin_doubled(k, n, sided) ? 2.0 : 1.0);
            if (ch == 0) pxx[slot] = 0.25 * (t[0] + t[1] + 2.0 * t[2]) * m;
            pyy[(int64_t)ch * nb + slot] = 0.25 * (t[0] + t[1] - 2.0 * t[2]) * m;
            pxy[((int64_t)ch * nb + slot) * 2] = 0.5 * t[3] * m;
            pxy[((int64_t)ch * nb + slot) * 2 + 1] = -0.25 * (t[0] - t[1]) * m;
        }
    }
}

// out layouts: pxx[nbins] (from channel 0's copy), pyy[nch][nbins], pxy[nch][nbins][2]
static __global__ __launch_bounds__(SP_FIN_BINS *SP_FIN_SLICES) void k_csd_finish(const float *__restrict__ partial, int64_t G,
                                                                            int L, int n, int nch, int sided,
                                                                            double scale, double *__restrict__ pxx,
                                                                            double *__restrict__ pyy,
                                                                            double *__restrict__ pxy) {
    __shared__ double sh[4][SP_FIN_SLICES][SP_FIN_BINS];
    const int lane = threadIdx.x % SP_FIN_BINS, sl = threadIdx.x / SP_FIN_BINS;
    const int k = blockIdx.x * SP_FIN_BINS + lane;
    const int ch = blockIdx.y;
    const int nb = nbins_of(n, sided);
    double s[4] = {0, 0, 0, 0};
    const float *p = partial + (int64_t)ch * G * 4 * L;
    if (k < n)
        for (int64_t g = sl; g < G; g += SP_FIN_SLICES) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += (double)p[(g * 4 + j) * L + k];
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[j][sl][lane] = s[j];
    fin_reduce<4>(sh, sl, lane);
    if (sl == 0 && k < n) {
        const int slot = bin_slot(k, n, sided);
        if (slot >= 0) {
            double tot[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[j] = sh[j][0][lane];
            const double m = scale * (bin_doubled(k, n, sided) ? 2.0 : 1.0);
            if (ch == 0) pxx[slot] = tot[0] * m;
            pyy[(int64_t)ch * nb + slot] = tot[1] * m;
            pxy[((int64_t)ch * nb + slot) * 2] = tot[2] * m;
            pxy[((int64_t)ch * nb + slot) * 2 + 1] = tot[3] * m;
        }
    }
}

template <bool DIAG>
static __global__ __launch_bounds__(256) void k_csdm_mfma(const cf *Xt, int nch, int nchp, int64_t mp, int nsb,
                                                           double *__restrict__ G /*[nb][nch][nch][2]*/, int64_t fs,
                                                           int64_t unit0, int slices, int atomic) {
    __shared__ float red[3][16][64];
    constexpr int NBLK = DIAG ? 3 : 4;
    // work unit = (bin, frame slice); blockIdx.x + unit0 enumerates them slice-fastest
    const int64_t unit = unit0 + blockIdx.x;
    const int k = (int)(unit / slices), zslice = (int)(unit % slices);
    int si, sj;
    if (DIAG) {
        si = sj = blockIdx.y;
    } else {
        // blockIdx.y enumerates the pairs si < sj
        int rem = blockIdx.y;
        si = 0;
        while (rem >= nsb - 1 - si) {
            rem -= nsb - 1 - si;
            ++si;
        }
        sj = si + 1 + rem;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
    const int64_t gbeg = (int64_t)zslice * fs, gend = gbeg + fs < mp ? gbeg + fs : mp;          // multiples of 32
    if (gbeg >= mp) return;                                                                      // empty slice (uniform)
    const int nsteps = (int)((gend - gbeg) / 8);                                                 // multiple of SP_CMM_PF, >= 4
    // step s of this wave: frames gbeg + 8 s + 2 wave + {0, 1}
    const cf *pa = Xt + ((int64_t)k * mp + gbeg + 2 * wave + half) * nchp + si * 64 + col;
    const cf *pb = Xt + ((int64_t)k * mp + gbeg + 2 * wave + half) * nchp + sj * 64 + col;
    const int64_t step_stride = (int64_t)8 * nchp;
    f32x16 accR[NBLK], accI[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            accR[b][v] = 0.f;
            accI[b][v] = 0.f;
        }
    // operand ring, SP_CMM_PF steps deep.  The loads are inline asm with hand-placed s_waitcnt: with ordinary loads
    // hipcc turns the loop-carried operands back into load-then-use inside one iteration (the IR carries the addresses,
    // not the data), which exposes the whole memory latency at every step.  The body is branch-free: frame padding
    // makes nsteps a multiple of the depth, loads past the end are clamped to the last step and never used.
    v2f a0[SP_CMM_PF], a1[SP_CMM_PF], b0[SP_CMM_PF], b1[SP_CMM_PF];
    const int last = nsteps - 1;
#define SP_GLOAD2(dst, ptr) asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(dst) : "v"(ptr) : "memory")
#pragma unroll
    for (int u = 0; u < SP_CMM_PF; ++u) {
        const int64_t o = (int64_t)(u < last ? u : last) * step_stride;
        SP_GLOAD2(a0[u], pa + o);
        SP_GLOAD2(a1[u], pa + o + 32);
        if (!DIAG) {
            SP_GLOAD2(b0[u], pb + o);
            SP_GLOAD2(b1[u], pb + o + 32);
        }
    }
    for (int s0 = 0; s0 < nsteps; s0 += SP_CMM_PF) {
#pragma unroll
        for (int u = 0; u < SP_CMM_PF; ++u) {
            // the oldest slot's loads are complete when only the (SP_CMM_PF - 1) younger slots' loads are outstanding
            if (DIAG) asm volatile("s_waitcnt vmcnt(6)" : "+v"(a0[u]), "+v"(a1[u])::"memory");
            else asm volatile("s_waitcnt vmcnt(12)" : "+v"(a0[u]), "+v"(a1[u]), "+v"(b0[u]), "+v"(b1[u])::"memory");
            const v2f x0 = a0[u], x1 = a1[u];
            const v2f y0 = DIAG ? x0 : b0[u], y1 = DIAG ? x1 : b1[u];
            const float n0 = -x0.x, n1 = -x1.x;
            // blocks 0: (I=0,J=0)  1: (0,1)  2: (1,1)  3: (1,0); consecutive MFMAs use different accumulators
            accR[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, y0.x, accR[0], 0, 0, 0);
            accR[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, y1.x, accR[1], 0, 0, 0);
            accR[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, y1.x, accR[2], 0, 0, 0);
            if constexpr (!DIAG) accR[NBLK - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, y0.x, accR[NBLK - 1], 0, 0, 0);
            accI[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y0.x, accI[0], 0, 0, 0);
            accI[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y1.x, accI[1], 0, 0, 0);
            accI[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y1.x, accI[2], 0, 0, 0);
            if constexpr (!DIAG) accI[NBLK - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y0.x, accI[NBLK - 1], 0, 0, 0);
            accR[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y0.y, accR[0], 0, 0, 0);
            accR[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y1.y, accR[1], 0, 0, 0);
            accR[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y1.y, accR[2], 0, 0, 0);
            if constexpr (!DIAG) accR[NBLK - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y0.y, accR[NBLK - 1], 0, 0, 0);
            accI[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(n0, y0.y, accI[0], 0, 0, 0);
            accI[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(n0, y1.y, accI[1], 0, 0, 0);
            accI[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(n1, y1.y, accI[2], 0, 0, 0);
            if constexpr (!DIAG) accI[NBLK - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(n1, y0.y, accI[NBLK - 1], 0, 0, 0);
            // refill the slot for step s0 + u + SP_CMM_PF
            const int sn = s0 + u + SP_CMM_PF;
            const int64_t o = (int64_t)(sn < last ? sn : last) * step_stride;
            SP_GLOAD2(a0[u], pa + o);
            SP_GLOAD2(a1[u], pa + o + 32);
            if (!DIAG) {
                SP_GLOAD2(b0[u], pb + o);
                SP_GLOAD2(b1[u], pb + o + 32);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef SP_GLOAD2
    // sum the four waves through LDS (one 32 x 32 accumulator at a time), then wave 0 adds into the float64 matrix.
    // Accumulator layout of the instruction: register v of lane l is D[i = 8 (v/4) + 4 (l/32) + v%4][j = l%32].
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        const int bi = (b == 0 || b == 1) ? 0 : 1, bj = (b == 0 || b == 3) ? 0 : 1;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            f32x16 &acc = part ? accI[b] : accR[b];
            __syncthreads();
            if (wave > 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) red[wave - 1][v][lane] = acc[v];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float t = (acc[v] + red[0][v][lane]) + (red[1][v][lane] + red[2][v][lane]);
                    const int i = si * 64 + 32 * bi + 8 * (v / 4) + 4 * half + (v % 4), j = sj * 64 + 32 * bj + col;
                    if (i < nch && j < nch) {
                        double *p = G + (((int64_t)k * nch + i) * nch + j) * 2 + part;
                        if (atomic) atomicAdd(p, (double)t);
                        else *p += (double)t;
                    }
                }
            }
        }
    }
}

static __global__ __launch_bounds__(1024) void k_csdm_fused(const cf *Xs, int nch, int64_t m, int nb /* row pitch of Xs */,
                                                             double *__restrict__ G, int64_t fs, int slices, int atomic) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf *lds = reinterpret_cast<cf *>(smem_raw);
    constexpr int F = SP_CMF_F;
    const int unit = blockIdx.x;
    const int k0 = (unit / slices) * SP_CMF_BINS, zslice = unit % slices;
    const int64_t gbeg = (int64_t)zslice * fs, gend = gbeg + fs < m ? gbeg + fs : m;
    if (gbeg >= gend) return;
    const int ntiles = (int)((gend - gbeg + F - 1) / F);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, half = lane >> 5, col = lane & 31;
    // staging: 2 passes x (128 rows x 8 parts of 2 bins); row = frame * 64 + channel.  The channel of a thread is
    // fixed, so is its row base; only 32 arch VGPRs are left beside the 96 accumulators (4 waves per SIMD).
    const int part = t & 7, rowq = t >> 3, cl = rowq & 63, f0 = rowq >> 6;
    const float keepc = cl < nch ? 1.f : 0.f;
    const cf *rowbase = Xs + (int64_t)(cl < nch ? cl : 0) * m * nb + k0 + 2 * part;
    cf *ldst = lds + (f0 * 64 + cl) * SP_CMF_P + 2 * part;
    cf st[2][2];
    float keep[2];
    auto gfetch = [&](int64_t g0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t g = g0 + f0 + 2 * q;
            const bool ok = g < gend;
            const cf *src = rowbase + (ok ? g : gbeg) * nb;          // clamped address; the value is masked at lstore,
            st[q][0] = src[0];                                       // so nothing here waits for the loads
            st[q][1] = src[1];
            keep[q] = ok ? keepc : 0.f;
        }
    };
    auto lstore = [&](int bufsel) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            cf *dst = ldst + bufsel * SP_CMF_TILE + (2 * q * 64) * SP_CMF_P;
            dst[0] = keep[q] * st[q][0];
            dst[1] = keep[q] * st[q][1];
        }
    };
    f32x16 accR[3], accI[3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            accR[b][v] = 0.f;
            accI[b][v] = 0.f;
        }
    gfetch(gbeg);
    lstore(0);
    __syncthreads();
    const cf *pa0 = lds + (half * 64 + col) * SP_CMF_P + wave;
    for (int it = 0; it < ntiles; ++it) {
        const bool more = it + 1 < ntiles;                    // workgroup-uniform
        if (more) gfetch(gbeg + (int64_t)(it + 1) * F);
        const cf *pa = pa0 + (it & 1) * SP_CMF_TILE;
#pragma unroll
        for (int p = 0; p < F / 2; ++p) {
            const cf x0 = pa[(2 * p * 64) * SP_CMF_P], x1 = pa[(2 * p * 64 + 32) * SP_CMF_P];
            const float n0 = -x0.x;
            // blocks 0: (0,0)  1: (0,1)  2: (1,1); consecutive MFMAs use different accumulators.  On the diagonal blocks
            // Im G = P - P^T with P = Im Re^T: only P is accumulated (10 MFMAs per frame pair instead of 12), the
            // transpose is taken once at the end
            accR[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, x0.x, accR[0], 0, 0, 0);
            accR[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, x1.x, accR[1], 0, 0, 0);
            accR[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, x1.x, accR[2], 0, 0, 0);
            accI[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, x0.x, accI[0], 0, 0, 0);
            accI[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, x1.x, accI[1], 0, 0, 0);
            accI[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, x1.x, accI[2], 0, 0, 0);
            accR[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, x0.y, accR[0], 0, 0, 0);
            accR[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, x1.y, accR[1], 0, 0, 0);
            accR[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, x1.y, accR[2], 0, 0, 0);
            accI[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(n0, x1.y, accI[1], 0, 0, 0);
        }
        if (more) lstore((it + 1) & 1);
        __syncthreads();
    }
    // register v of lane l is D[i = 8 (v/4) + 4 (l/32) + v%4][j = l%32]
    const int k = k0 + wave;
    float *tp = reinterpret_cast<float *>(lds) + wave * (32 * 33);       // this wave's 32 x 32 transpose image (pitch 33)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int bi = b == 2 ? 1 : 0, bj = b == 0 ? 0 : 1;
        if (b != 1) {
            // diagonal block: Im = P - P^T
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 16; ++v) tp[(8 * (v / 4) + 4 * half + (v % 4)) * 33 + col] = accI[b][v];
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 16; ++v) accI[b][v] -= tp[col * 33 + 8 * (v / 4) + 4 * half + (v % 4)];
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int i = 32 * bi + 8 * (v / 4) + 4 * half + (v % 4), j = 32 * bj + col;
            if (i < nch && j < nch) {
                double *p = G + (((int64_t)k * nch + i) * nch + j) * 2;
                if (atomic) {
                    atomicAdd(p, (double)accR[b][v]);
                    atomicAdd(p + 1, (double)accI[b][v]);
                } else {
                    p[0] += (double)accR[b][v];
                    p[1] += (double)accI[b][v];
                }
            }
        }
    }
}

// tail bins for the fused path: Xt2[kk][g][c] = Xs[c][g][kfirst + kk], zero padded (kk < ntail <= 16)
static __global__ void k_csdm_gather_bins(const cf *__restrict__ Xs, cf *__restrict__ Xt, int nch, int nchp, int64_t m, int64_t mp,
                                          int nb /* row pitch of Xs */, int kfirst, int ntail) {
    const int64_t g = blockIdx.x;
    for (int e = threadIdx.x; e < ntail * nchp; e += blockDim.x) {
        const int kk = e / nchp, c = e % nchp;
        const bool ok = c < nch && g < m;
        const cf v = Xs[ok ? ((int64_t)c * m + g) * nb + kfirst + kk : 0];
        Xt[((int64_t)kk * mp + g) * nchp + c] = ok ? v : mk(0.f, 0.f);
    }
}

// Xs[c][g][k] (k fastest) -> Xt2[k][g][c] (c fastest, nchp channels, mp frames; the padding is written as zeros)
static __global__ void k_csdm_transpose_kgc(const cf *__restrict__ Xs, cf *__restrict__ Xt, int nch, int nchp, int64_t m,
                                            int64_t mp, int nb) {
    __shared__ cf tile[32][33];
    const int64_t g = blockIdx.z;
    const int k0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = c0 + j, k = k0 + threadIdx.x;
        const bool ok = c < nch && g < m && k < nb;
        const cf v = Xs[ok ? ((int64_t)c * m + g) * nb + k : 0];
        tile[j][threadIdx.x] = ok ? v : mk(0.f, 0.f);
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int k = k0 + j, c = c0 + threadIdx.x;
        if (k < nb) Xt[((int64_t)k * mp + g) * nchp + c] = tile[threadIdx.x][j];
    }
}

// scale, and fill the blocks below the block diagonal from their Hermitian mirrors
// (blk = granularity of the computed upper block triangle: 64 for the VALU kernel, 32 for the MFMA kernel)
static __global__ void k_csdm_finish(double *__restrict__ G, int nch, int nb, double scale, int blk) {
    const int64_t total = (int64_t)nb * nch * nch;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nch), i = (int)((e / nch) % nch);
        if (j / blk >= i / blk) {
            G[2 * e] *= scale;
            G[2 * e + 1] *= scale;
        }
    }
}

static __global__ void k_csdm_mirror(double *__restrict__ G, int nch, int nb, int blk) {
    const int64_t total = (int64_t)nb * nch * nch;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nch), i = (int)((e / nch) % nch);
        const int64_t k = e / ((int64_t)nch * nch);
        if (j / blk < i / blk) {
            const int64_t m = ((k * nch + j) * nch + i);
            G[2 * e] = G[2 * m];
            G[2 * e + 1] = -G[2 * m + 1];
        }
    }
}

int launch_csd(LaunchCtx c, const void *x, const void *y, bool cplx, int nch, int64_t y_ld, const float *win, int hop,
               int64_t nframes, const float *trend_x, const float *trend_y, bool lin, const Xf &xf, float *partial,
               const RunPart &rp, int segmean) {
#define L_(XT, CP, LN)                                                                                \
    hipLaunchKernelGGL((k_welch_csd<XT, CP, LN>), dim3(rp.blocks, nch), dim3(XT::C::WG), XT::C::lds_bytes(1), c.stream, x, \
                       y, y_ld, win, hop, nframes, rp.fpg, trend_x, trend_y, xf.tb, partial, rp.groups, segmean)
#define M_(XT)                                                                                        \
    if (cplx) {                                                                                       \
        if (lin) L_(XT, true, true);                                                                  \
        else L_(XT, true, false);                                                                     \
    } else {                                                                                          \
        if (lin) L_(XT, false, true);                                                                 \
        else L_(XT, false, false);                                                                    \
    }
    SP_DISPATCH_X(xf, M_)
#undef M_
#undef L_
    return 0;
}

int launch_csd_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                      double *pxx, double *pyy, double *pxy) {
    const int n = xf.tb.n;
    hipLaunchKernelGGL(k_csd_finish, dim3((n + SP_FIN_BINS - 1) / SP_FIN_BINS, nch), dim3(SP_FIN_BINS * SP_FIN_SLICES), 0,
                       c.stream, partial, G, xf.L, n, nch, sided, scale, pxx, pyy, pxy);
    return 0;
}

// real x, y, power-of-two n >= 32: one transform per (frame, channel)
bool csd_rp_eligible(const Xf &xf) { return !xf.blue && xf.L >= 32 && xf.L <= 8192; }

int launch_csd_rp(LaunchCtx c, const float *x, const float *y, int nch, int64_t y_ld, const float *win, int hop,
                  int64_t nframes, const float *trend_x, const float *trend_y, bool lin, const Xf &xf, float *partial,
                  const RunPart &rp) {
#define RP_(NN)                                                                                       \
    case NN:                                                                                          \
        if (lin) hipLaunchKernelGGL((k_welch_csd_rp<NN, true>), dim3(rp.blocks, nch), dim3(WgCfg<NN>::WG),       \
                                    WgCfg<NN>::lds_bytes(1), c.stream, x, y, y_ld, win, hop, nframes, rp.fpg, trend_x,  \
                                    trend_y, xf.tb, partial, rp.groups);                              \
        else hipLaunchKernelGGL((k_welch_csd_rp<NN, false>), dim3(rp.blocks, nch), dim3(WgCfg<NN>::WG),          \
                                WgCfg<NN>::lds_bytes(1), c.stream, x, y, y_ld, win, hop, nframes, rp.fpg, trend_x,      \
                                trend_y, xf.tb, partial, rp.groups);                                  \
        break;
    switch (xf.L) {
        RP_(32) RP_(64) RP_(128) RP_(256) RP_(512) RP_(1024) RP_(2048) RP_(4096) RP_(8192)
        default: return -1;
    }
#undef RP_
    return 0;
}

// reference-once form: Zx = packed pair spectra of x, then one transform per (channel, frame pair)
int launch_pairspec(LaunchCtx c, const float *x, const float *win, int hop, int64_t nframes, const float *trend, bool lin,
                    const Xf &xf, const RunPart &rp, cf *Zx) {
#define PS_(NN)                                                                                       \
    case NN:                                                                                          \
        if (lin) hipLaunchKernelGGL((k_pairspec<NN, true>), dim3(rp.blocks), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1),    \
                                    c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, Zx);         \
        else hipLaunchKernelGGL((k_pairspec<NN, false>), dim3(rp.blocks), dim3(WgCfg<NN>::WG), WgCfg<NN>::lds_bytes(1),       \
                                c.stream, x, win, hop, nframes, rp.fpg, trend, xf.tb, Zx);             \
        break;
    switch (xf.L) {
        PS_(32) PS_(64) PS_(128) PS_(256) PS_(512) PS_(1024) PS_(2048) PS_(4096) PS_(8192)
        default: return -1;
    }
#undef PS_
    return 0;
}

// workgroups of the selected k_welch_csd_pair instantiation one CU keeps resident (0: unknown)
int csd_pair_resident(const Xf &xf, bool lin, bool onepass) {
    if (onepass) return resident_per_cu((const void *)k_welch_csd_pair<4096, false, true>, WgCfg<4096>::WG, WgCfg<4096>::lds_bytes(1));
#define CR_(NN)                                                                                       \
    case NN:                                                                                          \
        return lin ? resident_per_cu((const void *)k_welch_csd_pair<NN, true>, WgCfg<NN>::WG, WgCfg<NN>::lds_bytes(1)) \
                   : resident_per_cu((const void *)k_welch_csd_pair<NN, false>, WgCfg<NN>::WG, WgCfg<NN>::lds_bytes(1));
    switch (xf.L) {
        CR_(32) CR_(64) CR_(128) CR_(256) CR_(512) CR_(1024) CR_(2048) CR_(4096) CR_(8192)
        default: return 0;
    }
#undef CR_
}

int launch_csd_pair(LaunchCtx c, const float *y, int nch, int64_t y_ld, const float *win, int hop, int64_t nframes,
                    float *trend_y, bool lin, const Xf &xf, const cf *Zx, float *partial, const RunPart &rp, cf *spartial) {
    const int cf_ = rp.blocks <= 65535 ? 1 : 0;       // channel-fastest block order (grid.y <= 65535)
    const dim3 grid_ = cf_ ? dim3(nch, rp.blocks) : dim3(rp.blocks, nch);
    if (spartial) {
        // one-pass mean detrend (see the kernel): nfft 4096 at hop 2048 only
        if (lin || xf.L != 4096 || hop != 2048) return -1;
        hipLaunchKernelGGL((k_welch_csd_pair<4096, false, true>), grid_, dim3(WgCfg<4096>::WG), WgCfg<4096>::lds_bytes(1), c.stream, y,
                           y_ld, win, hop, nframes, rp.fpg, trend_y, xf.tb, Zx, partial, rp.groups, cf_, spartial);
        return 0;
    }
#define CP_(NN)                                                                                       \
    case NN:                                                                                          \
        if (lin) hipLaunchKernelGGL((k_welch_csd_pair<NN, true>), grid_, dim3(WgCfg<NN>::WG),         \
                                    WgCfg<NN>::lds_bytes(1), c.stream, y, y_ld, win, hop, nframes, rp.fpg, trend_y, xf.tb, Zx, \
                                    partial, rp.groups, cf_, (cf *)nullptr);                          \
        else hipLaunchKernelGGL((k_welch_csd_pair<NN, false>), grid_, dim3(WgCfg<NN>::WG),            \
                                WgCfg<NN>::lds_bytes(1), c.stream, y, y_ld, win, hop, nframes, rp.fpg, trend_y, xf.tb, Zx,     \
                                partial, rp.groups, cf_, (cf *)nullptr);                              \
        break;
    switch (xf.L) {
        CP_(32) CP_(64) CP_(128) CP_(256) CP_(512) CP_(1024) CP_(2048) CP_(4096) CP_(8192)
        default: return -1;
    }
#undef CP_
    return 0;
}

int launch_csd_pair_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                           double *pyy, double *pxy, const double *st_y, const double *st_x, const cf *Wf, const float *trend_x,
                           const float *trend_y, int64_t nmean, int64_t M) {
    const int n = xf.tb.n;
    hipLaunchKernelGGL(k_csd_pair_finish, dim3((n + SP_FIN_BINS - 1) / SP_FIN_BINS, nch), dim3(SP_FIN_BINS * SP_FIN_SLICES), 0,
                       c.stream, partial, G, n, nch, sided, scale, pyy, pxy, st_y, st_x, Wf, trend_x, trend_y, nmean, M);
    return 0;
}
// block sums of one real signal in SP_COLSUM_SLICES slices (out: [slices][H] complex), see k_colsum_real
int launch_colsum_real(LaunchCtx c, const float *x, const float *trend, int H, int64_t M, cf *out) {
    hipLaunchKernelGGL(k_colsum_real, dim3((H + 255) / 256, SP_COLSUM_SLICES), dim3(256), 0, c.stream, x, trend, H, M, out);
    return 0;
}

int launch_csd_rp_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                         double *pxx, double *pyy, double *pxy) {
    const int n = xf.tb.n;
    hipLaunchKernelGGL(k_csd_rp_finish, dim3((n + SP_FIN_BINS - 1) / SP_FIN_BINS, nch), dim3(SP_FIN_BINS * SP_FIN_SLICES), 0,
                       c.stream, partial, G, n, nch, sided, scale, pxx, pyy, pxy);
    return 0;
}

// blk: the MFMA paths' 32 x 32 blocks
int launch_csdm_finish(LaunchCtx c, double *G, int nch, int nb, double scale) {
    const int blk = 32;
    const int64_t total = (int64_t)nb * nch * nch;
    int64_t b = (total + 255) / 256;
    if (b > (int64_t)c.ncu * 16) b = (int64_t)c.ncu * 16;
    hipLaunchKernelGGL(k_csdm_finish, dim3((int)b), dim3(256), 0, c.stream, G, nch, nb, scale, blk);
    hipLaunchKernelGGL(k_csdm_mirror, dim3((int)b), dim3(256), 0, c.stream, G, nch, nb, blk);
    return 0;
}

// MFMA path: Xs[c][g][k] -> Xt2[k][g][c] (zero padded), then one workgroup per (bin, superblock pair, frame slice)
int launch_csdm_transpose_kgc(LaunchCtx c, const cf *Xs, cf *Xt, int nch, int nchp, int64_t m, int64_t mp, int nb) {
    dim3 grid((unsigned)((nb + 31) / 32), (unsigned)(nchp / 32), (unsigned)mp);
    hipLaunchKernelGGL(k_csdm_transpose_kgc, grid, dim3(32, 8), 0, c.stream, Xs, Xt, nch, nchp, m, mp, nb);
    return 0;
}

int launch_csdm_mfma(LaunchCtx c, const cf *Xt, int nch, int nchp, int64_t mp, int nb, double *G) {
    const int nsb = nchp / 64;
    const int npair = nsb * (nsb - 1) / 2;
    // Work units = (bin, frame slice), all of equal cost, 2 resident workgroups per CU (204 VGPRs).  Slices (multiples
    // of 256 frames) only when there are too few bins for >= 4 rounds; then the units that would form a partial last
    // round (e.g. the 2049th bin of cfg5: 2048 = 4 full rounds) are launched separately, cut 8 times finer, so that no
    // CU waits for a straggler.  Sliced units add into G atomically.
    const int64_t slots = (int64_t)c.ncu * 2;
    const int64_t per_bin = nsb + npair;                                         // workgroups per unit (grid.y)
    int slices = (int)((slots * 4 + (int64_t)nb * per_bin - 1) / ((int64_t)nb * per_bin));
    const int max_slices = (int)((mp + 255) / 256);
    if (slices > max_slices) slices = max_slices;
    if (slices < 1) slices = 1;
    int64_t fs = (mp + slices - 1) / slices;
    fs = (fs + 255) / 256 * 256;
    slices = (int)((mp + fs - 1) / fs);
    const int64_t units = (int64_t)nb * slices;
    int64_t main_units = units * per_bin >= slots ? (units * per_bin / slots) * slots / per_bin : units;
    if (fs < 8 * 32) main_units = units;                                          // cannot cut finer
    auto go = [&](int64_t u0, int64_t n, int sl, int64_t f, int atomic) {
        if (n <= 0) return;
        hipLaunchKernelGGL((k_csdm_mfma<true>), dim3((unsigned)n, nsb, 1), dim3(256), 0, c.stream, Xt, nch, nchp, mp, nsb, G, f,
                           u0, sl, atomic);
        if (nsb > 1)
            hipLaunchKernelGGL((k_csdm_mfma<false>), dim3((unsigned)n, npair, 1), dim3(256), 0, c.stream, Xt, nch, nchp, mp,
                               nsb, G, f, u0, sl, atomic);
    };
    go(0, main_units, slices, fs, slices > 1);
    go(main_units * 8, (units - main_units) * 8, slices * 8, fs / 8, 1);
    return 0;
}

// fused path (nch <= 64: one channel superblock): bins [0, 16*ngroups) straight from Xs; the remaining 1..16 bins
// through a gathered copy + k_csdm_mfma
int launch_csdm_fused(LaunchCtx c, const cf *Xs, cf *Xt_tail, int nch, int64_t m, int nb, double *G, int ld) {
    if (ld <= 0) ld = nb;                                  // row pitch of the spectra (>= nb)
    const int nchp = (nch + 63) / 64 * 64;
    const int ngroups = (nb - 1) / SP_CMF_BINS;
    if (ngroups > 0) {
        // frame slices (multiples of 8 frames) when there are fewer bin groups than CUs; sliced units add atomically
        int slices = (c.ncu + ngroups - 1) / ngroups;
        const int max_slices = (int)((m + 127) / 128);
        if (slices > max_slices) slices = max_slices;
        if (slices < 1) slices = 1;
        int64_t fs = (m + slices - 1) / slices;
        fs = (fs + SP_CMF_F - 1) / SP_CMF_F * SP_CMF_F;
        slices = (int)((m + fs - 1) / fs);
        const size_t lds = 2 * sizeof(cf) * SP_CMF_TILE;                          // 68 KiB
        if (lds_raise<k_csdm_fused>(lds)) return -1;
        hipLaunchKernelGGL(k_csdm_fused, dim3(ngroups * slices), dim3(1024), lds, c.stream, Xs, nch, m, ld, G, fs, slices,
                           slices > 1);
    }
    const int kfirst = SP_CMF_BINS * ngroups, ntail = nb - kfirst;
    if (ntail > 0) {
        const int64_t mp = (m + 31) / 32 * 32;
        hipLaunchKernelGGL(k_csdm_gather_bins, dim3((unsigned)mp), dim3(256), 0, c.stream, Xs, Xt_tail, nch, nchp, m, mp, ld, kfirst,
                           ntail);
        if (launch_csdm_mfma(c, Xt_tail, nch, nchp, mp, ntail, G + (int64_t)kfirst * nch * nch * 2)) return -1;
    }
    return 0;
}

}   // namespace sp
