// k_dwt.hip -- the discrete wavelet transforms: the decimated pyramid (dwt / idwt, six extension modes) and the undecimated,
// circular MODWT (modwt / imodwt), each in two forms (include/spectral_dwt.h; the host's arithmetic and the index maps in dwt_plan.h).
//
//   analysis   cA[k] = sum_{m<L} lo[m] xe[2k + c - m],  cD[k] the same with hi        (c = 1, periodization: c = L / 2)
//   synthesis  x[i]  = sum_q lo[p + 2q] cA[k0 - q] + sum_q hi[p + 2q] cD[k0 - q],  t = i + shift, p = t & 1, k0 = t >> 1, q < L / 2
//   MODWT      V_j[t] = sum_l g[l] V_{j-1}[(t - s l) mod n],  W_j the same with h,  s = 2^(j-1)
//   its inverse V_{j-1}[t] = sum_l h[l] W_j[(t + s l) mod n] + sum_l g[l] V_j[(t + s l) mod n]
//
// dwt_ana and dwt_syn are the only places a coefficient is computed: float32 FMAs, the taps ascending, one accumulator per filter.  The
// forms differ only in where the reader finds sample m of the sum, never in the values or their order, so they agree bitwise.
//
// Row form (k_dwt_row, k_idwt_row, k_modwt_row, k_imodwt_row): a workgroup owns a row (four rows of up to 1024 samples, 64 threads
// each), stages it once in LDS and runs every level there between two buffers; per level the halo of L - 1 samples on both sides is
// filled through the mode's index map, so the sums read LDS without a map.  Every detail and the last approximation leave by
// coalesced stores; nothing else touches memory.  The MODWT needs no halo: its reader steps through the row modulo n.
// Tile form (k_dwt_tile, k_idwt_tile, k_modwt_tile, k_imodwt_tile): one level per launch, a workgroup produces DWT_TILE outputs of
// one row for both filters.  The analysis stages its 2 T + L - 2 samples through the index map (the whole level is in memory, so a
// halo longer than the record is only a map; inside the row by 16-byte loads aligned on the absolute element index); the synthesis stages the T / 2 + L / 2 coefficients of cA and of cD once.  The MODWT
// tile reads V through the modulo reader from memory: outputs T apart share no sample once s >= T, and below that L2 serves the reuse.
// There are no atomics; all row x pitch arithmetic is 64-bit, everything inside a tile fits 32 bits.
#include "launch.h"
namespace sp {

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool CPLX> struct DwtT { typedef float T; };
template <> struct DwtT<true> { typedef v2f T; };

__device__ inline float dwt_fma(float h, float v, float a) { return fmaf(h, v, a); }
__device__ inline v2f dwt_fma(float h, v2f v, v2f a) { return v2f{fmaf(h, v.x, a.x), fmaf(h, v.y, a.y)}; }
template <class E> __device__ inline E dwt_zero();
template <> __device__ inline float dwt_zero<float>() { return 0.f; }
template <> __device__ inline v2f dwt_zero<v2f>() { return v2f{0.f, 0.f}; }

// sample m of a sum: m steps back from p
template <class E> struct LinRd {
    const E *p;
    __device__ E operator()(int m) const { return p[-m]; }
};
// sample m of a sum, called with m = 0, 1, ..: idx steps by inc modulo n (0 <= idx, inc < n)
template <class E> struct ModRd {
    const E *p;
    int64_t idx, inc, n;
    __device__ E operator()(int) {
        const E v = p[idx];
        idx += inc;
        if (idx >= n) idx -= n;
        return v;
    }
};

// L is even: two taps go per turn, in the same order as one by one.  The decimated analysis (k_dwt_row, k_dwt_tile) hands in the
// kernel's arguments themselves: the index is the same in every lane, so the taps arrive as scalars and cost no LDS read.
template <class E, class Rd> __device__ inline void dwt_ana(const float *lo, const float *hi, int L, Rd rd, E &a, E &d) {
    E sa = dwt_zero<E>(), sd = dwt_zero<E>();
    for (int m = 0; m < L; m += 2) {
        const E v0 = rd(m), v1 = rd(m + 1);
        sa = dwt_fma(lo[m], v0, sa);
        sd = dwt_fma(hi[m], v0, sd);
        sa = dwt_fma(lo[m + 1], v1, sa);
        sd = dwt_fma(hi[m + 1], v1, sd);
    }
    a = sa, d = sd;
}

// the taps j0, j0 + js, .. < L of fa on ra and of fd on rd; the two sums are added last.  Here the tap index differs from lane to lane
// (the parity of the output), and the synthesis and MODWT kernels read their taps from LDS: measured faster than scalar loads there.
template <class E, class RdA, class RdD> __device__ inline E dwt_syn(const float *fa, const float *fd, int j0, int js, int L, RdA ra, RdD rd) {
    E sa = dwt_zero<E>(), sd = dwt_zero<E>();
    for (int j = j0, q = 0; j < L; j += js, ++q) {
        sa = dwt_fma(fa[j], ra(q), sa);
        sd = dwt_fma(fd[j], rd(q), sd);
    }
    return sa + sd;
}

// the filters from the kernel's arguments into LDS: F[0 .. L) and F[64 .. 64 + L)
__device__ inline void dwt_filters(const DwtFilt &f, float *F) {
    for (int i = threadIdx.x; i < f.L; i += 256) F[i] = f.lo[i], F[DWT_MAX_L + i] = f.hi[i];
}

// ---- row form ------------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void k_dwt_row(const void *__restrict__ x, int64_t x_ld, int n, int64_t rows, DwtFilt f, int mode, int levels, int rpw, int cap,
                                                 DwtLv lv, void *__restrict__ outA, int64_t a_ld, void *__restrict__ outD, int64_t d_ld) {
    typedef typename DwtT<CPLX>::T E;
    extern __shared__ float4 smem4[];
    const int L = f.L, H = L - 1, tpr = 256 / rpw, r = threadIdx.x / tpr, lane = threadIdx.x % tpr, c = dwt_center(L, mode);
    const int64_t row = (int64_t)blockIdx.x * rpw + r;
    const bool live = row < rows;
    E *A = reinterpret_cast<E *>(smem4 + DWT_FILT_BYTES / 16) + (size_t)r * 2 * cap, *B = A + cap;
    if (live) {
        const E *xr = reinterpret_cast<const E *>(x) + row * x_ld;
        for (int i = lane; i < n; i += tpr) A[H + i] = xr[i];
    }
    int nj = n;
    for (int j = 1; j <= levels; ++j) {
        __syncthreads();
        if (live)
            for (int h = lane; h < 2 * H; h += tpr) {            // the halo: L - 1 samples on both sides, through the index map
                const int i = h < H ? h - H : nj + (h - H);
                const int64_t s = dwt_ext(i, nj, mode);
                A[H + i] = s < 0 ? dwt_zero<E>() : A[H + s];
            }
        __syncthreads();
        const int K = lv.len[j];
        if (live) {
            E *dr = reinterpret_cast<E *>(outD) + row * d_ld + lv.off[j];
            for (int k = lane; k < K; k += tpr) {
                E a, d;
                dwt_ana(f.lo, f.hi, L, LinRd<E>{A + H + 2 * k + c}, a, d);
                B[H + k] = a;
                dr[k] = d;
            }
        }
        E *t = A;
        A = B, B = t, nj = K;
    }
    __syncthreads();
    if (live) {
        E *ar = reinterpret_cast<E *>(outA) + row * a_ld;
        for (int k = lane; k < nj; k += tpr) ar[k] = A[H + k];
    }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_idwt_row(const void *__restrict__ inA, int64_t a_ld, const void *__restrict__ inD, int64_t d_ld, int64_t rows, DwtFilt f,
                                                  int mode, int levels, int rpw, int cap, DwtLv lv, void *__restrict__ x, int64_t x_ld) {
    typedef typename DwtT<CPLX>::T E;
    extern __shared__ float4 smem4[];
    float *F = reinterpret_cast<float *>(smem4);                                  // the filters, then the rows' buffers
    const int L = f.L, tpr = 256 / rpw, r = threadIdx.x / tpr, lane = threadIdx.x % tpr, shift = dwt_syn_shift(L, mode);
    const int64_t row = (int64_t)blockIdx.x * rpw + r;
    const bool live = row < rows, per = mode == DWT_PER;
    E *A = reinterpret_cast<E *>(smem4 + DWT_FILT_BYTES / 16) + (size_t)r * 2 * cap, *B = A + cap;      // A = [cA_j | cD_j], B takes the approximation below
    dwt_filters(f, F);
    if (live) {
        const E *ar = reinterpret_cast<const E *>(inA) + row * a_ld;
        for (int k = lane; k < lv.len[levels]; k += tpr) A[k] = ar[k];
    }
    for (int j = levels; j >= 1; --j) {
        const int K = lv.len[j], nout = lv.len[j - 1];
        if (live) {
            const E *dr = reinterpret_cast<const E *>(inD) + row * d_ld + lv.off[j];
            for (int k = lane; k < K; k += tpr) A[K + k] = dr[k];
        }
        __syncthreads();
        if (live)
            for (int i = lane; i < nout; i += tpr) {
                const int t = i + shift, p = t & 1, k0 = t >> 1;
                if (per) {
                    const int64_t s = k0 % K;
                    B[i] = dwt_syn<E>(F, F + DWT_MAX_L, p, 2, L, ModRd<E>{A, s, K - 1, K}, ModRd<E>{A + K, s, K - 1, K});
                } else {
                    B[i] = dwt_syn<E>(F, F + DWT_MAX_L, p, 2, L, LinRd<E>{A + k0}, LinRd<E>{A + K + k0});
                }
            }
        __syncthreads();
        E *t = A;
        A = B, B = t;
    }
    if (live) {
        E *xr = reinterpret_cast<E *>(x) + row * x_ld;
        for (int i = lane; i < lv.len[0]; i += tpr) xr[i] = A[i];
    }
}

// W[(j - 1) plane + row w_ld + t], j = 1 .. levels, and V_levels in the plane behind them
template <bool CPLX>
__global__ __launch_bounds__(256) void k_modwt_row(const void *__restrict__ x, int64_t x_ld, int n, int64_t rows, DwtFilt f, int levels, int rpw, int cap,
                                                   void *__restrict__ W, int64_t w_ld, int64_t plane) {
    typedef typename DwtT<CPLX>::T E;
    extern __shared__ float4 smem4[];
    float *F = reinterpret_cast<float *>(smem4);                                  // the filters, then the rows' buffers
    const int L = f.L, tpr = 256 / rpw, r = threadIdx.x / tpr, lane = threadIdx.x % tpr;
    const int64_t row = (int64_t)blockIdx.x * rpw + r;
    const bool live = row < rows;
    E *A = reinterpret_cast<E *>(smem4 + DWT_FILT_BYTES / 16) + (size_t)r * 2 * cap, *B = A + cap;
    dwt_filters(f, F);
    if (live) {
        const E *xr = reinterpret_cast<const E *>(x) + row * x_ld;
        for (int i = lane; i < n; i += tpr) A[i] = xr[i];
    }
    E *wr = reinterpret_cast<E *>(W) + row * w_ld;
    for (int j = 1; j <= levels; ++j, wr += plane) {
        __syncthreads();
        const int64_t inc = dwt_mod(-((int64_t)1 << (j - 1)), n);
        if (live)
            for (int t = lane; t < n; t += tpr) {
                E a, d;
                dwt_ana(F, F + DWT_MAX_L, L, ModRd<E>{A, t, inc, n}, a, d);
                B[t] = a;
                wr[t] = d;
            }
        E *t = A;
        A = B, B = t;
    }
    __syncthreads();
    if (live)
        for (int t = lane; t < n; t += tpr) wr[t] = A[t];
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_imodwt_row(const void *__restrict__ W, int64_t w_ld, int64_t plane, int n, int64_t rows, DwtFilt f, int levels, int rpw,
                                                    int cap, void *__restrict__ x, int64_t x_ld) {
    typedef typename DwtT<CPLX>::T E;
    extern __shared__ float4 smem4[];
    float *F = reinterpret_cast<float *>(smem4);                                  // the filters, then the rows' buffers
    const int L = f.L, tpr = 256 / rpw, r = threadIdx.x / tpr, lane = threadIdx.x % tpr;
    const int64_t row = (int64_t)blockIdx.x * rpw + r;
    const bool live = row < rows;
    E *A = reinterpret_cast<E *>(smem4 + DWT_FILT_BYTES / 16) + (size_t)r * 2 * cap, *B = A + cap;
    dwt_filters(f, F);
    const E *wr = reinterpret_cast<const E *>(W) + row * w_ld + plane * levels;
    if (live)
        for (int t = lane; t < n; t += tpr) A[t] = wr[t];                          // V_levels
    for (int j = levels; j >= 1; --j) {
        wr -= plane;                                                               // W_j: read from memory, each sample L times through L2
        __syncthreads();
        const int64_t inc = dwt_mod((int64_t)1 << (j - 1), n);
        if (live)
            for (int t = lane; t < n; t += tpr) B[t] = dwt_syn<E>(F + DWT_MAX_L, F, 0, 1, L, ModRd<E>{wr, t, inc, n}, ModRd<E>{A, t, inc, n});
        E *t = A;
        A = B, B = t;
    }
    __syncthreads();
    if (live) {
        E *xr = reinterpret_cast<E *>(x) + row * x_ld;
        for (int t = lane; t < n; t += tpr) xr[t] = A[t];
    }
}

// ---- tile form -----------------------------------------------------------------------------------------------------------------------
template <bool CPLX>
__global__ __launch_bounds__(256) void k_dwt_tile(const void *__restrict__ x, int64_t x_ld, int64_t n, int64_t tiles, DwtFilt f, int mode, int64_t K,
                                                  int vec, void *__restrict__ cA, int64_t a_ld, void *__restrict__ cD, int64_t d_ld) {
    typedef typename DwtT<CPLX>::T E;
    extern __shared__ float4 smem4[];
    E *X = reinterpret_cast<E *>(smem4);
    const int L = f.L, tid = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / tiles, k0 = ((int64_t)blockIdx.x % tiles) * DWT_TILE;
    const int Tk = (int)(K - k0 < DWT_TILE ? K - k0 : DWT_TILE), NI = 2 * Tk + L - 2;
    const int64_t ib = 2 * k0 + dwt_center(L, mode) - (L - 1);                    // the first staged sample of the extended level
    const E *xr = reinterpret_cast<const E *>(x) + b * x_ld;
    // 16-byte loads aligned on the absolute element index (as k_upfirdn stages): the group of V samples from na on lies inside the row
    // and on a 16-byte boundary wherever x itself does (vec); the groups at the ends of the row, and everything outside it, go
    // sample by sample through the index map
    constexpr int V = CPLX ? 2 : 4;
    const int shift = (int)((b * x_ld + ib) & (V - 1));
    const int64_t na = ib - shift;
    const int nvec = (NI + shift + V - 1) / V;
    for (int iv = tid; iv < nvec; iv += 256) {
        const int jt = iv * V;
        const int64_t g = na + jt;
        E xs[V];
        if (vec && g >= 0 && g + V <= n) {
            const float4 t = *reinterpret_cast<const float4 *>(xr + g);
            if constexpr (CPLX) xs[0] = v2f{t.x, t.y}, xs[1] = v2f{t.z, t.w};
            else xs[0] = t.x, xs[1] = t.y, xs[2] = t.z, xs[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int64_t s = dwt_ext(g + j, n, mode);
                xs[j] = s < 0 ? dwt_zero<E>() : xr[s];
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int d = jt - shift + j;
            if (d >= 0 && d < NI) X[d] = xs[j];
        }
    }
    __syncthreads();
    E *ar = reinterpret_cast<E *>(cA) + b * a_ld + k0, *dr = reinterpret_cast<E *>(cD) + b * d_ld + k0;
    for (int k = tid; k < Tk; k += 256) {
        E a, d;
        dwt_ana(f.lo, f.hi, L, LinRd<E>{X + 2 * k + L - 1}, a, d);
        ar[k] = a;
        dr[k] = d;
    }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_idwt_tile(const void *__restrict__ cA, int64_t a_ld, const void *__restrict__ cD, int64_t d_ld, int64_t K, int64_t tiles,
                                                   DwtFilt f, int mode, void *__restrict__ x, int64_t x_ld, int64_t nout) {
    typedef typename DwtT<CPLX>::T E;
    __shared__ float F[2 * DWT_MAX_L];
    dwt_filters(f, F);
    extern __shared__ float4 smem4[];
    const int L = f.L, tid = threadIdx.x, shift = dwt_syn_shift(L, mode), NKmax = DWT_TILE / 2 + L / 2 + 1;
    E *XA = reinterpret_cast<E *>(smem4), *XD = XA + NKmax;
    const int64_t b = (int64_t)blockIdx.x / tiles, i0 = ((int64_t)blockIdx.x % tiles) * DWT_TILE;
    const int Ti = (int)(nout - i0 < DWT_TILE ? nout - i0 : DWT_TILE);
    const int64_t kb = ((i0 + shift) >> 1) - (L / 2 - 1);                          // the first staged coefficient (periodization: may be < 0)
    const int NK = (int)(((i0 + Ti - 1 + shift) >> 1) - kb + 1);
    const E *ar = reinterpret_cast<const E *>(cA) + b * a_ld, *dr = reinterpret_cast<const E *>(cD) + b * d_ld;
    for (int q = tid; q < NK; q += 256) {
        int64_t s = kb + q;
        if (mode == DWT_PER) s = dwt_mod(s, K);
        const bool in = s >= 0 && s < K;
        XA[q] = in ? ar[s] : dwt_zero<E>();
        XD[q] = in ? dr[s] : dwt_zero<E>();
    }
    __syncthreads();
    E *xr = reinterpret_cast<E *>(x) + b * x_ld + i0;
    for (int i = tid; i < Ti; i += 256) {
        const int64_t t = i0 + i + shift;
        const int p = (int)(t & 1), k0 = (int)((t >> 1) - kb);
        xr[i] = dwt_syn<E>(F, F + DWT_MAX_L, p, 2, L, LinRd<E>{XA + k0}, LinRd<E>{XD + k0});
    }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_modwt_tile(const void *__restrict__ vin, int64_t in_ld, int64_t n, int64_t tiles, DwtFilt f, int64_t inc,
                                                    void *__restrict__ W, int64_t w_ld, void *__restrict__ vout, int64_t out_ld) {
    typedef typename DwtT<CPLX>::T E;
    __shared__ float F[2 * DWT_MAX_L];
    dwt_filters(f, F);
    const int64_t b = (int64_t)blockIdx.x / tiles, t0 = ((int64_t)blockIdx.x % tiles) * DWT_TILE;
    const E *vr = reinterpret_cast<const E *>(vin) + b * in_ld;
    E *wr = reinterpret_cast<E *>(W) + b * w_ld, *orow = reinterpret_cast<E *>(vout) + b * out_ld;
    __syncthreads();
    for (int64_t t = t0 + threadIdx.x; t < t0 + DWT_TILE && t < n; t += 256) {
        E a, d;
        dwt_ana(F, F + DWT_MAX_L, f.L, ModRd<E>{vr, t, inc, n}, a, d);
        orow[t] = a;
        wr[t] = d;
    }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_imodwt_tile(const void *__restrict__ W, int64_t w_ld, const void *__restrict__ vin, int64_t in_ld, int64_t n, int64_t tiles,
                                                     DwtFilt f, int64_t inc, void *__restrict__ vout, int64_t out_ld) {
    typedef typename DwtT<CPLX>::T E;
    __shared__ float F[2 * DWT_MAX_L];
    dwt_filters(f, F);
    const int64_t b = (int64_t)blockIdx.x / tiles, t0 = ((int64_t)blockIdx.x % tiles) * DWT_TILE;
    const E *wr = reinterpret_cast<const E *>(W) + b * w_ld, *vr = reinterpret_cast<const E *>(vin) + b * in_ld;
    E *orow = reinterpret_cast<E *>(vout) + b * out_ld;
    __syncthreads();
    for (int64_t t = t0 + threadIdx.x; t < t0 + DWT_TILE && t < n; t += 256)
        orow[t] = dwt_syn<E>(F + DWT_MAX_L, F, 0, 1, f.L, ModRd<E>{wr, t, inc, n}, ModRd<E>{vr, t, inc, n});
}

// ---- launchers: -1 for a geometry a kernel does not take ----------------------------------------------------------------------------
static bool dwt_row_ok(const DwtRowArgs &a) {
    return a.rows >= 1 && a.n >= 1 && a.levels >= 1 && a.levels <= DWT_MAX_LEVELS && a.f.L >= 2 && a.f.L <= DWT_MAX_L && !(a.f.L & 1) &&
           a.rpw == dwt_row_pack(a.n) && a.cap == dwt_row_cap(a.n, a.f.L) && a.lds == (size_t)dwt_row_lds(a.cplx, a.n, a.f.L) && a.lds <= SP_LDS_MAX &&
           a.lv.len[0] == a.n && (a.rows + a.rpw - 1) / a.rpw <= 0x7fffffff;
}

#define DWT_BOTH(CALL)                      \
    if (a.cplx) { CALL(true) } else { CALL(false) }

int launch_dwt_row(LaunchCtx c, const DwtRowArgs &a, const void *x, int64_t x_ld, void *outA, int64_t a_ld, void *outD, int64_t d_ld) {
    if (!dwt_row_ok(a) || a.mode < 0 || a.mode >= DWT_NMODES || x_ld < a.n) return -1;
    const dim3 grid((unsigned)((a.rows + a.rpw - 1) / a.rpw));
#define L_(CP)                                                                                                                          \
    if (lds_raise<k_dwt_row<CP>>(a.lds)) return -1;                                                                                      \
    hipLaunchKernelGGL((k_dwt_row<CP>), grid, dim3(256), a.lds, c.stream, x, x_ld, (int)a.n, a.rows, a.f, a.mode, a.levels, a.rpw, (int)a.cap, a.lv, outA, a_ld, \
                       outD, d_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_idwt_row(LaunchCtx c, const DwtRowArgs &a, const void *inA, int64_t a_ld, const void *inD, int64_t d_ld, void *x, int64_t x_ld) {
    if (!dwt_row_ok(a) || a.mode < 0 || a.mode >= DWT_NMODES || x_ld < a.n) return -1;
    const dim3 grid((unsigned)((a.rows + a.rpw - 1) / a.rpw));
#define L_(CP)                                                                                                                          \
    if (lds_raise<k_idwt_row<CP>>(a.lds)) return -1;                                                                                     \
    hipLaunchKernelGGL((k_idwt_row<CP>), grid, dim3(256), a.lds, c.stream, inA, a_ld, inD, d_ld, a.rows, a.f, a.mode, a.levels, a.rpw, (int)a.cap, a.lv, x, x_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_modwt_row(LaunchCtx c, const DwtRowArgs &a, const void *x, int64_t x_ld, void *W, int64_t w_ld, int64_t plane) {
    if (!dwt_row_ok(a) || a.levels > DWT_MODWT_MAX_LEVELS || x_ld < a.n || w_ld < a.n) return -1;
    const dim3 grid((unsigned)((a.rows + a.rpw - 1) / a.rpw));
#define L_(CP)                                                                                                                          \
    if (lds_raise<k_modwt_row<CP>>(a.lds)) return -1;                                                                                    \
    hipLaunchKernelGGL((k_modwt_row<CP>), grid, dim3(256), a.lds, c.stream, x, x_ld, (int)a.n, a.rows, a.f, a.levels, a.rpw, (int)a.cap, W, w_ld, plane);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_imodwt_row(LaunchCtx c, const DwtRowArgs &a, const void *W, int64_t w_ld, int64_t plane, void *x, int64_t x_ld) {
    if (!dwt_row_ok(a) || a.levels > DWT_MODWT_MAX_LEVELS || x_ld < a.n || w_ld < a.n) return -1;
    const dim3 grid((unsigned)((a.rows + a.rpw - 1) / a.rpw));
#define L_(CP)                                                                                                                          \
    if (lds_raise<k_imodwt_row<CP>>(a.lds)) return -1;                                                                                   \
    hipLaunchKernelGGL((k_imodwt_row<CP>), grid, dim3(256), a.lds, c.stream, W, w_ld, plane, (int)a.n, a.rows, a.f, a.levels, a.rpw, (int)a.cap, x, x_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

static bool dwt_tile_ok(const DwtTileArgs &a, int64_t outs) {
    const int64_t tiles = (outs + DWT_TILE - 1) / DWT_TILE;
    return a.rows >= 1 && outs >= 1 && outs <= DWT_MAX_N && a.f.L >= 2 && a.f.L <= DWT_MAX_L && !(a.f.L & 1) && tiles <= 0x7fffffff / a.rows;
}

int launch_dwt_tile(LaunchCtx c, const DwtTileArgs &a, const void *x, int64_t x_ld, int64_t n, void *cA, int64_t a_ld, void *cD, int64_t d_ld) {
    const int64_t K = dwt_coeff_len(n, a.f.L, a.mode), tiles = (K + DWT_TILE - 1) / DWT_TILE;
    if (n < 1 || n > DWT_MAX_N || a.mode < 0 || a.mode >= DWT_NMODES || !dwt_tile_ok(a, K) || x_ld < n || a_ld < K || d_ld < K) return -1;
    const size_t lds = (size_t)dwt_tile_lds(DWT_WHAT_DWT, a.cplx, a.f.L);
    const int vec = ((uintptr_t)x & 15) == 0 ? 1 : 0;
#define L_(CP) hipLaunchKernelGGL((k_dwt_tile<CP>), dim3((unsigned)(tiles * a.rows)), dim3(256), lds, c.stream, x, x_ld, n, tiles, a.f, a.mode, K, vec, cA, a_ld, cD, d_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_idwt_tile(LaunchCtx c, const DwtTileArgs &a, const void *cA, int64_t a_ld, const void *cD, int64_t d_ld, void *x, int64_t x_ld, int64_t nout) {
    const int64_t K = dwt_coeff_len(nout, a.f.L, a.mode), tiles = (nout + DWT_TILE - 1) / DWT_TILE;
    if (a.mode < 0 || a.mode >= DWT_NMODES || !dwt_tile_ok(a, nout) || x_ld < nout || a_ld < K || d_ld < K) return -1;
    const size_t lds = (size_t)dwt_tile_lds(DWT_WHAT_IDWT, a.cplx, a.f.L);
#define L_(CP) hipLaunchKernelGGL((k_idwt_tile<CP>), dim3((unsigned)(tiles * a.rows)), dim3(256), lds, c.stream, cA, a_ld, cD, d_ld, K, tiles, a.f, a.mode, x, x_ld, nout);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_modwt_tile(LaunchCtx c, const DwtTileArgs &a, int level, const void *vin, int64_t in_ld, int64_t n, void *W, int64_t w_ld, void *vout, int64_t out_ld) {
    const int64_t tiles = (n + DWT_TILE - 1) / DWT_TILE;
    if (level < 1 || level > DWT_MODWT_MAX_LEVELS || !dwt_tile_ok(a, n) || in_ld < n || w_ld < n || out_ld < n) return -1;
    const int64_t inc = dwt_mod(-((int64_t)1 << (level - 1)), n);
#define L_(CP) hipLaunchKernelGGL((k_modwt_tile<CP>), dim3((unsigned)(tiles * a.rows)), dim3(256), 0, c.stream, vin, in_ld, n, tiles, a.f, inc, W, w_ld, vout, out_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

int launch_imodwt_tile(LaunchCtx c, const DwtTileArgs &a, int level, const void *W, int64_t w_ld, const void *vin, int64_t in_ld, int64_t n, void *vout, int64_t out_ld) {
    const int64_t tiles = (n + DWT_TILE - 1) / DWT_TILE;
    if (level < 1 || level > DWT_MODWT_MAX_LEVELS || !dwt_tile_ok(a, n) || in_ld < n || w_ld < n || out_ld < n) return -1;
    const int64_t inc = dwt_mod((int64_t)1 << (level - 1), n);
#define L_(CP) hipLaunchKernelGGL((k_imodwt_tile<CP>), dim3((unsigned)(tiles * a.rows)), dim3(256), 0, c.stream, W, w_ld, vin, in_ld, n, tiles, a.f, inc, vout, out_ld);
    DWT_BOTH(L_)
#undef L_
    return 0;
}

}   // namespace sp
