// k_cond.hip -- conditioned spectral analysis of a batch of Hermitian matrices of order n <= 64 in complex128 (sp_cond; the MIMO frequency
// response, multiple and partial coherence, conditioned and ordered spectra of a cross-spectral-density matrix; include/spectral_mimo.h).
// One matrix per workgroup, held in LDS from the load to the stores; everything is read off one Cholesky factor.
//   load      A = G[order][:, order] + delta I: element (i, k), k <= i, comes from the LOWER triangle of G (G[oi][ok] if oi >= ok, else
//             the conjugate of G[ok][oi]); of the diagonal only the real part.  The permutation travels in the kernel arguments.
//             delta = loading max(sum_i Re A_ii, 0) / n, the sum in ascending order.  The diagonal as loaded (with delta) is kept aside.
//   factor    right-looking: at step j every thread reads the pivot d_j = A_jj (uniform, from LDS).  d_j > n 2^-52 A_jj(loaded), or:
//               j < q   the inputs are collinear: status = j + 1, the factorisation stops, every output asked for is zeros, piv is zeros
//                       from j on;
//               j >= q  status = j + 1 if it was 0; the pivot and the column under it are set to zero and the factorisation goes on.
//             Else L_ij = A_ij / sqrt(d_j) for i > j, barrier, A_ik -= L_ij conj(L_kj) for j < k <= i (the diagonal in real arithmetic),
//             barrier.  The diagonal keeps d_j unrooted: piv_j = d_j, and L_jj = sqrt(d_j) where a stage needs it.
//   mcoh      sum_{k<q} |L_{q+i,k}|^2 ascending, over the loaded diagonal; 0 where that is <= 0.
//   Gc        element (i, j), j <= i: sum_{m=q}^{q+j-1} L_{q+i,m} conj(L_{q+j,m}) + L_{q+i,q+j} L_{q+j,q+j}; the diagonal is a real sum
//             that ends with d; the mirror is written as the conjugate.
//   P         W = L^-1 by the same right-looking walk in a second region (row m is divided by L_mm, then W_ic -= L_im W_mc for i > m),
//             P_ij = sum_{m>=i} conj(W_mi) W_mj for j <= i, the diagonal a real sum; zeros where status != 0.
//   H         in place on the block L_yx, after everything that reads it: for k = q - 1 .. 0: X_ik = A_ik / L_kk, barrier,
//             A_im -= X_ik L_km for m < k, barrier.
// Every thread of a workgroup takes the same branches (they depend on values read from LDS after a barrier, or on the arguments), so no
// barrier is met by part of a workgroup.  No atomics; every sum has a fixed order: two calls agree bitwise.  The grid walks the batch.
#include "launch.h"
namespace sp {

static __device__ __forceinline__ double2 cd_mulc(double2 a, double2 b) {   // a conj(b)
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
static __device__ __forceinline__ double2 cd_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

static __global__ __launch_bounds__(512) void k_cond(CondArgs a) {
    extern __shared__ __align__(16) unsigned char cond_smem[];
    const int n = a.n, q = a.q, r = n - q, LD = cond_pitch(n), lg = cond_lg(n), msk = (1 << lg) - 1, WG = blockDim.x;
    const bool wantP = (a.want & COND_WANT_P) != 0;
    double2 *A = (double2 *)cond_smem;
    double2 *W = (double2 *)(cond_smem + cond_off_w(n));                  // only touched when P is wanted
    double *dg = (double *)(cond_smem + cond_off_diag(n, wantP));
    const int tid = threadIdx.x;
    const int sq = n << lg;                                               // the index space of the square: row e >> lg, column e & msk

    for (int64_t b = blockIdx.x; b < a.count; b += gridDim.x) {
        const double2 *Gb = a.G + b * a.G_ld;
        for (int e = tid; e < sq; e += WG) {
            const int i = e >> lg, k = e & msk;
            if (k <= i) {
                const int oi = a.order.p[i], ok = a.order.p[k];
                double2 z;
                if (oi >= ok) z = Gb[oi * n + ok];
                else {
                    z = Gb[ok * n + oi];
                    z.y = -z.y;
                }
                if (i == k) z.y = 0.0;
                A[i * LD + k] = z;
            }
        }
        __syncthreads();
        double tr = 0.0;
        for (int i = 0; i < n; ++i) tr += A[i * LD + i].x;                // every thread the same sum, from broadcast reads
        const double delta = a.loading * fmax(tr, 0.0) / (double)n;
        __syncthreads();
        if (tid < n) {
            const double d = A[tid * LD + tid].x + delta;
            A[tid * LD + tid].x = d;
            dg[tid] = d;
        }
        __syncthreads();

        // ---- factor
        int st = 0;
        bool hard = false;
        int jstop = n;
        for (int j = 0; j < n; ++j) {
            const double dj = A[j * LD + j].x;
            if (!(dj > (double)n * 0x1p-52 * dg[j])) {
                if (st == 0) st = j + 1;
                if (j < q) {
                    hard = true;
                    jstop = j;
                    break;
                }
                __syncthreads();                                          // everyone has read the pivot
                for (int i = j + tid; i < n; i += WG) A[i * LD + j] = make_double2(0.0, 0.0);
                __syncthreads();
                continue;
            }
            const double s = sqrt(dj);
            for (int i = j + 1 + tid; i < n; i += WG) {
                const double2 z = A[i * LD + j];
                A[i * LD + j] = make_double2(z.x / s, z.y / s);
            }
            __syncthreads();
            for (int e = tid; e < sq; e += WG) {
                const int i = e >> lg, k = e & msk;
                if (k > j && k <= i) {
                    const double2 li = A[i * LD + j];
                    double2 z = A[i * LD + k];
                    if (i == k) z.x -= li.x * li.x + li.y * li.y;
                    else {
                        const double2 t = cd_mulc(li, A[k * LD + j]);
                        z.x -= t.x;
                        z.y -= t.y;
                    }
                    A[i * LD + k] = z;
                }
            }
            __syncthreads();
        }

        if (tid == 0) a.status[b] = st;
        if (a.want & COND_WANT_PIV) {
            double *pv = a.piv + b * a.piv_ld;
            for (int j = tid; j < n; j += WG) pv[j] = j < jstop ? A[j * LD + j].x : 0.0;
        }
        if (hard) {                                                       // never NaN
            if (a.want & COND_WANT_H)
                for (int e = tid; e < r * q; e += WG) a.H[b * a.H_ld + e] = make_double2(0.0, 0.0);
            if (a.want & COND_WANT_GC)
                for (int e = tid; e < r * r; e += WG) a.Gc[b * a.Gc_ld + e] = make_double2(0.0, 0.0);
            if (a.want & COND_WANT_MCOH)
                for (int e = tid; e < r; e += WG) a.mcoh[b * a.mcoh_ld + e] = 0.0;
            if (wantP)
                for (int e = tid; e < n * n; e += WG) a.P[b * a.P_ld + e] = make_double2(0.0, 0.0);
            __syncthreads();                                              // the next matrix overwrites A
            continue;
        }

        // ---- multiple coherence of every output with all the inputs
        if (a.want & COND_WANT_MCOH) {
            for (int i = tid; i < r; i += WG) {
                double sum = 0.0;
                for (int k = 0; k < q; ++k) {
                    const double2 z = A[(q + i) * LD + k];
                    sum += z.x * z.x + z.y * z.y;
                }
                const double den = dg[q + i];
                a.mcoh[b * a.mcoh_ld + i] = den > 0.0 ? sum / den : 0.0;
            }
        }
        // ---- the conditioned matrix of the outputs
        if (a.want & COND_WANT_GC) {
            double2 *gc = a.Gc + b * a.Gc_ld;
            for (int e = tid; e < (r << lg); e += WG) {
                const int i = e >> lg, j = e & msk;
                if (j > i) continue;
                const double2 *ri = A + (q + i) * LD + q, *rj = A + (q + j) * LD + q;
                if (i == j) {
                    double sum = 0.0;
                    for (int m = 0; m < j; ++m) sum += ri[m].x * ri[m].x + ri[m].y * ri[m].y;
                    gc[i * r + i] = make_double2(sum + ri[i].x, 0.0);
                } else {
                    double2 sum = make_double2(0.0, 0.0);
                    for (int m = 0; m < j; ++m) {
                        const double2 t = cd_mulc(ri[m], rj[m]);
                        sum.x += t.x;
                        sum.y += t.y;
                    }
                    const double ljj = sqrt(rj[j].x);
                    sum.x += ri[j].x * ljj;
                    sum.y += ri[j].y * ljj;
                    gc[i * r + j] = sum;
                    gc[j * r + i] = make_double2(sum.x, -sum.y);
                }
            }
        }
        // ---- the precision matrix
        if (wantP) {
            double2 *Pb = a.P + b * a.P_ld;
            if (st != 0) {
                for (int e = tid; e < n * n; e += WG) Pb[e] = make_double2(0.0, 0.0);
            } else {
                for (int e = tid; e < sq; e += WG) {
                    const int i = e >> lg, c = e & msk;
                    if (c <= i) W[i * LD + c] = make_double2(i == c ? 1.0 : 0.0, 0.0);
                }
                __syncthreads();
                for (int m = 0; m < n; ++m) {
                    const double s = sqrt(A[m * LD + m].x);
                    for (int c = tid; c <= m; c += WG) {
                        const double2 z = W[m * LD + c];
                        W[m * LD + c] = make_double2(z.x / s, z.y / s);
                    }
                    __syncthreads();
                    for (int e = tid; e < sq; e += WG) {
                        const int i = e >> lg, c = e & msk;
                        if (i > m && c <= m) {
                            const double2 t = cd_mul(A[i * LD + m], W[m * LD + c]);
                            double2 z = W[i * LD + c];
                            z.x -= t.x;
                            z.y -= t.y;
                            W[i * LD + c] = z;
                        }
                    }
                    __syncthreads();
                }
                for (int e = tid; e < sq; e += WG) {
                    const int i = e >> lg, j = e & msk;
                    if (j > i) continue;
                    if (i == j) {
                        double sum = 0.0;
                        for (int m = i; m < n; ++m) {
                            const double2 z = W[m * LD + i];
                            sum += z.x * z.x + z.y * z.y;
                        }
                        Pb[i * n + i] = make_double2(sum, 0.0);
                    } else {
                        double2 sum = make_double2(0.0, 0.0);
                        for (int m = i; m < n; ++m) {
                            const double2 t = cd_mulc(W[m * LD + j], W[m * LD + i]);   // W_mj conj(W_mi)
                            sum.x += t.x;
                            sum.y += t.y;
                        }
                        Pb[i * n + j] = sum;
                        Pb[j * n + i] = make_double2(sum.x, -sum.y);
                    }
                }
            }
        }
        // ---- the response of the outputs to the inputs, in place on L_yx
        if (a.want & COND_WANT_H) {
            __syncthreads();                                              // mcoh has read L_yx
            for (int k = q - 1; k >= 0; --k) {
                const double s = sqrt(A[k * LD + k].x);
                for (int i = tid; i < r; i += WG) {
                    const double2 z = A[(q + i) * LD + k];
                    A[(q + i) * LD + k] = make_double2(z.x / s, z.y / s);
                }
                __syncthreads();
                for (int e = tid; e < (r << lg); e += WG) {
                    const int i = e >> lg, m = e & msk;
                    if (m < k) {
                        const double2 t = cd_mul(A[(q + i) * LD + k], A[k * LD + m]);
                        double2 z = A[(q + i) * LD + m];
                        z.x -= t.x;
                        z.y -= t.y;
                        A[(q + i) * LD + m] = z;
                    }
                }
                __syncthreads();
            }
            double2 *Hb = a.H + b * a.H_ld;
            for (int e = tid; e < (r << lg); e += WG) {
                const int i = e >> lg, k = e & msk;
                if (k < q) Hb[i * q + k] = A[(q + i) * LD + k];
            }
        }
        __syncthreads();                                                  // the next matrix overwrites A, W and the diagonal
    }
}

int launch_cond(LaunchCtx c, const CondArgs &a, const CondPlan &pl) {
    // (want may be empty here: an output without elements was taken out, and the status is still owed)
    if (a.n < 1 || a.n > COND_MAX_N || a.q < 0 || a.q > a.n || (a.want & ~COND_WANT_ALL) || a.count < 1 || a.count > COND_MAX_COUNT || !a.G || !a.status ||
        a.G_ld < (int64_t)a.n * a.n)
        return -1;
    if (pl.grid < 1 || pl.grid > a.count || pl.grid > COND_MAX_GRID || pl.wg != cond_wg(a.n) ||
        pl.lds_bytes != cond_lds(a.n, (a.want & COND_WANT_P) != 0) || (size_t)pl.lds_bytes > SP_LDS_MAX)
        return -1;
    const int n = a.n, r = a.n - a.q;
    if ((a.want & COND_WANT_H) && (int64_t)r * a.q > 0 && (!a.H || a.H_ld < (int64_t)r * a.q)) return -1;
    if ((a.want & COND_WANT_GC) && r > 0 && (!a.Gc || a.Gc_ld < (int64_t)r * r)) return -1;
    if ((a.want & COND_WANT_MCOH) && r > 0 && (!a.mcoh || a.mcoh_ld < r)) return -1;
    if ((a.want & COND_WANT_PIV) && (!a.piv || a.piv_ld < n)) return -1;
    if ((a.want & COND_WANT_P) && (!a.P || a.P_ld < (int64_t)n * n)) return -1;
    for (int i = 0; i < n; ++i)
        if (a.order.p[i] >= n) return -1;
    if (lds_raise<k_cond>((size_t)pl.lds_bytes)) return -1;
    hipLaunchKernelGGL(k_cond, dim3((unsigned)pl.grid), dim3((unsigned)pl.wg), (size_t)pl.lds_bytes, c.stream, a);
    return 0;
}

}   // namespace sp
