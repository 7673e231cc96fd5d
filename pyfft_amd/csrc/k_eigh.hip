// k_eigh.hip -- batched Hermitian eigensolver of order n <= 64 in complex128: parallel cyclic Jacobi, one matrix per workgroup, the
// matrix A and the accumulated vectors V held in LDS from the load to the store (sp_eigh; spectral POD of the CSD matrix).
//   order     n is padded to NP = 8, 16, 32 or 64 with zero rows and columns.  Rows are NP + 1 elements apart (16 B each): a stride of
//             NP elements would put a column of NP = 64 on one bank group.
//   input     only the lower triangle and the real part of the diagonal are read (numpy's UPLO = 'L'); the upper triangle is its
//             conjugate mirror.  Every entry is multiplied by 2^-e, e = ilogb(largest |re| or |im| read), so that |a_pq|^2 neither
//             overflows nor vanishes; w is multiplied by 2^e at the end.  Both are exact.
//   sweep     a round-robin tournament: NP - 1 steps, NP / 2 disjoint pairs a step.  Index NP - 1 stays put and meets st at step st;
//             pair k >= 1 of step st is ((st + k) mod (NP - 1), (st - k) mod (NP - 1)); p is the smaller index, q the larger.
//   step      threads 0 .. NP/2 - 1 compute the rotations of all pairs from the matrix as it is before the step, into LDS:
//               g = |a_pq|,  tau = (a_qq - a_pp) / 2g,  t = sgn(tau) / (|tau| + hypot(1, tau)),  c = 1 / sqrt(1 + t^2),  s = t c,
//               ph = a_pq / g;      J = [[c, s ph], [-s conj(ph), c]] on (p, q)
//             a pair is skipped (J = 1) unless g >= 2^-1000: an exact zero never rotates, so the padding never mixes with the matrix
//             however many of its own eigenvalues are zero, and a NaN never rotates.  (Deliberately wider than "a_pq == 0 exactly":
//             a nonzero entry below 2^-1000 of a matrix scaled to [1, 2) is left unannihilated, far under the stopping threshold,
//             and a_pq / g never divides subnormals.)  Barrier.  Then A <- J^H A J: a thread owns whole
//             2 x 2 pair-blocks (the rows of pair r by the columns of pair c, r <= c), reads four elements and writes the same four
//             plus their conjugates into block (c, r), which nobody reads: in place without a hazard, and A stays exactly Hermitian.
//             The diagonal block is set to a_pp - t g, a_qq + t g and an exact 0.  V <- V J on the n real rows.  Barrier.
//   stop      before each sweep off^2 = sum_{i<j} |a_ij|^2 by a fixed-order LDS tree; every thread reads the sum from LDS after a
//             barrier, so the decision off^2 <= (n eps)^2 ||A||_F^2 is uniform and no barrier is met by part of the workgroup.  After
//             max_sweeps sweeps without it: sweeps = max_sweeps + 1 (also any non-finite input; the loop is bounded by the cap).
//   finish    w_i = Re a_ii; rank by counting (descending, ties by index); column j of v is the vector of w[j], turned so that its
//             component of largest modulus (the first on ties) is real and positive.
// No atomics; every sum has a fixed order: two calls agree bitwise.  The grid walks the batch.
#include "launch.h"
namespace sp {

template <int NP> struct EighCfg {
    static constexpr int M = NP / 2, LD = NP + 1, R = NP - 1;
    static constexpr int WG = NP * NP / 4 < 64 ? 64 : (NP * NP / 4 > 1024 ? 1024 : NP * NP / 4);
    static constexpr int NBLK = M * (M + 1) / 2;            // pair-blocks r <= c
    static_assert(M % 2 == 0, "the fold of the triangle of pair-blocks needs an even number of pairs");
};

template <int NP, bool VEC> struct EighLds {
    using C = EighCfg<NP>;
    double2 A[NP * C::LD];
    double2 V[VEC ? NP * C::LD : 1];
    double2 ph[C::M];                 // the step's rotations
    double2 colph[NP];                // finish: the turn of every written column
    double c[C::M], s[C::M], tg[C::M];
    double red[C::WG];
    double w[NP];
    int skip[C::M];
    int perm[NP], imax[NP];
};

static __device__ __forceinline__ double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
static __device__ __forceinline__ double2 zmulc(double2 a, double2 b) {   // a conj(b)
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
static __device__ __forceinline__ double2 zconj(double2 a) { return make_double2(a.x, -a.y); }

// sum (MAX: maximum) of one value per thread in a fixed order; every thread of the workgroup calls it and gets the same value from LDS
template <int WG, bool MAX> static __device__ __forceinline__ double eigh_reduce(double v, double *red, int tid) {
    red[tid] = v;
    __syncthreads();
#pragma unroll 1
    for (int h = WG / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = MAX ? fmax(red[tid], red[tid + h]) : red[tid] + red[tid + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <int NP> static __device__ __forceinline__ void eigh_pair(int st, int k, int &p, int &q) {
    constexpr int R = NP - 1;
    const int a = k == 0 ? R : (st + k) % R, b = k == 0 ? st : (st - k + R) % R;
    p = a < b ? a : b;
    q = a < b ? b : a;
}

template <int NP, bool VEC>
static __global__ __launch_bounds__(EighCfg<NP>::WG) void k_eigh(const double2 *__restrict__ a, int n, int64_t batch, int nvec,
                                                                  int max_sweeps, double *__restrict__ w, double2 *__restrict__ v,
                                                                  int *__restrict__ sweeps) {
    using C = EighCfg<NP>;
    constexpr int M = C::M, LD = C::LD, WG = C::WG;
    extern __shared__ __align__(16) unsigned char eigh_smem[];
    EighLds<NP, VEC> &S = *reinterpret_cast<EighLds<NP, VEC> *>(eigh_smem);
    const double neps = (double)n * 2.220446049250313e-16;

    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));          // per matrix: the lane masks of one part are not kept in scalar registers through the others
        const double2 *ab = a + b * n * n;
        // ---- load the lower triangle, mirror it, zero the padding; V = 1
        double amax = 0.0;
        for (int e = tid; e < NP * NP; e += WG) {
            const int i = e / NP, j = e % NP;
            if (j <= i) {
                double2 z = make_double2(0.0, 0.0);
                if (i < n) {
                    z = ab[i * n + j];
                    if (i == j) z.y = 0.0;
                }
                S.A[i * LD + j] = z;
                if (j < i) S.A[j * LD + i] = zconj(z);
                amax = fmax(amax, fmax(fabs(z.x), fabs(z.y)));
            }
            if (VEC) S.V[i * LD + j] = make_double2(i == j ? 1.0 : 0.0, 0.0);
        }
        amax = eigh_reduce<WG, true>(amax, S.red, tid);
        const int ex = (amax > 0.0 && amax < INFINITY) ? ilogb(amax) : 0;
        for (int e = tid; e < NP * NP; e += WG) {
            const int i = e / NP, j = e % NP;
            const double2 z = S.A[i * LD + j];
            S.A[i * LD + j] = make_double2(ldexp(z.x, -ex), ldexp(z.y, -ex));
        }
        __syncthreads();
        double dg = 0.0;
        if (tid < NP) dg = S.A[tid * LD + tid].x * S.A[tid * LD + tid].x;
        const double diag2 = eigh_reduce<WG, false>(dg, S.red, tid);

        // ---- sweeps
        double thresh = 0.0;
        int used = max_sweeps + 1;
        for (int sw = 0; sw <= max_sweeps; ++sw) {
            double part = 0.0;
            for (int e = tid; e < NP * NP; e += WG) {
                const int i = e / NP, j = e % NP;
                if (i < j) {
                    const double2 z = S.A[i * LD + j];
                    part += z.x * z.x + z.y * z.y;
                }
            }
            const double off2 = eigh_reduce<WG, false>(part, S.red, tid);
            if (sw == 0) thresh = neps * neps * (diag2 + 2.0 * off2);
            if (off2 <= thresh && thresh < INFINITY) {          // uniform: both came out of LDS
                used = sw;
                break;
            }
            if (sw == max_sweeps) break;
#pragma unroll 1
            for (int st = 0; st < NP - 1; ++st) {
                if (tid < M) {
                    int p, q;
                    eigh_pair<NP>(st, tid, p, q);
                    const double2 apq = S.A[p * LD + q];
                    const double g = hypot(apq.x, apq.y);
                    double c = 1.0, s = 0.0, tg = 0.0;
                    double2 ph = make_double2(1.0, 0.0);
                    const bool skip = !(g >= 0x1p-1000);
                    if (!skip) {
                        const double tau = (S.A[q * LD + q].x - S.A[p * LD + p].x) / (2.0 * g);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                        tg = t * g;
                        ph = make_double2(apq.x / g, apq.y / g);
                    }
                    S.c[tid] = c;
                    S.s[tid] = s;
                    S.tg[tid] = tg;
                    S.ph[tid] = ph;
                    S.skip[tid] = skip ? 1 : 0;
                }
                __syncthreads();
                for (int e = tid; e < C::NBLK; e += WG) {
                    const int i = e / (M + 1), j = e % (M + 1);
                    const int r = j > i ? i : M - 1 - i, cb = j > i ? j - 1 : M - 1 - i + j;
                    if (S.skip[r] & S.skip[cb]) continue;
                    int pr, qr, pc, qc;
                    eigh_pair<NP>(st, r, pr, qr);
                    if (r == cb) {
                        const double t_g = S.tg[r];
                        S.A[pr * LD + pr] = make_double2(S.A[pr * LD + pr].x - t_g, 0.0);
                        S.A[qr * LD + qr] = make_double2(S.A[qr * LD + qr].x + t_g, 0.0);
                        S.A[pr * LD + qr] = make_double2(0.0, 0.0);
                        S.A[qr * LD + pr] = make_double2(0.0, 0.0);
                        continue;
                    }
                    eigh_pair<NP>(st, cb, pc, qc);
                    const double cr = S.c[r], cc = S.c[cb];
                    const double2 phr = S.ph[r], phc = S.ph[cb];
                    const double sr = S.s[r], sc = S.s[cb];
                    const double2 spr = make_double2(sr * phr.x, sr * phr.y), spc = make_double2(sc * phc.x, sc * phc.y);
                    const double2 x00 = S.A[pr * LD + pc], x01 = S.A[pr * LD + qc], x10 = S.A[qr * LD + pc], x11 = S.A[qr * LD + qc];
                    // Y = Jr^H X
                    const double2 m0 = zmul(spr, x10), m1 = zmul(spr, x11), k0 = zmulc(x00, spr), k1 = zmulc(x01, spr);
                    const double2 y00 = make_double2(cr * x00.x - m0.x, cr * x00.y - m0.y);
                    const double2 y01 = make_double2(cr * x01.x - m1.x, cr * x01.y - m1.y);
                    const double2 y10 = make_double2(k0.x + cr * x10.x, k0.y + cr * x10.y);
                    const double2 y11 = make_double2(k1.x + cr * x11.x, k1.y + cr * x11.y);
                    // X' = Y Jc
                    const double2 u0 = zmulc(y01, spc), u1 = zmulc(y11, spc), v0 = zmul(y00, spc), v1 = zmul(y10, spc);
                    const double2 n00 = make_double2(y00.x * cc - u0.x, y00.y * cc - u0.y);
                    const double2 n10 = make_double2(y10.x * cc - u1.x, y10.y * cc - u1.y);
                    const double2 n01 = make_double2(v0.x + y01.x * cc, v0.y + y01.y * cc);
                    const double2 n11 = make_double2(v1.x + y11.x * cc, v1.y + y11.y * cc);
                    S.A[pr * LD + pc] = n00;
                    S.A[pr * LD + qc] = n01;
                    S.A[qr * LD + pc] = n10;
                    S.A[qr * LD + qc] = n11;
                    S.A[pc * LD + pr] = zconj(n00);
                    S.A[qc * LD + pr] = zconj(n01);
                    S.A[pc * LD + qr] = zconj(n10);
                    S.A[qc * LD + qr] = zconj(n11);
                }
                if (VEC) {
                    for (int e = tid; e < n * M; e += WG) {
                        const int i = e / M, k = e % M;
                        if (S.skip[k]) continue;
                        int p, q;
                        eigh_pair<NP>(st, k, p, q);
                        const double c = S.c[k], s = S.s[k];
                        const double2 ph = S.ph[k];
                        const double2 sp = make_double2(s * ph.x, s * ph.y);
                        const double2 v0 = S.V[i * LD + p], v1 = S.V[i * LD + q];
                        const double2 u = zmulc(v1, sp), t2 = zmul(v0, sp);
                        S.V[i * LD + p] = make_double2(v0.x * c - u.x, v0.y * c - u.y);
                        S.V[i * LD + q] = make_double2(t2.x + v1.x * c, t2.y + v1.y * c);
                    }
                }
                __syncthreads();
            }
        }

        // ---- finish: sort by counting, scale back, turn and store the leading vectors
        if (tid < NP) {
            S.w[tid] = tid < n ? S.A[tid * LD + tid].x : 0.0;
            S.perm[tid] = tid;
        }
        __syncthreads();
        int rank = 0;
        if (tid < n) {
            const double wi = S.w[tid];
            for (int j = 0; j < n; ++j) {
                const double wj = S.w[j];
                rank += (wj > wi || (wj == wi && j < tid)) ? 1 : 0;
            }
        }
        __syncthreads();
        if (tid < n) S.perm[rank] = tid;           // rank < n; after NaNs some slots keep their initial index
        __syncthreads();
        if (tid < n) w[b * n + tid] = ldexp(S.w[S.perm[tid]], ex);
        if (tid == 0) sweeps[b] = used;
        if (VEC) {
            if (tid < nvec) {
                const int src = S.perm[tid];
                double best = -1.0;
                int bi = 0;
                for (int i = 0; i < n; ++i) {
                    const double2 z = S.V[i * LD + src];
                    const double m2 = z.x * z.x + z.y * z.y;
                    if (m2 > best) {
                        best = m2;
                        bi = i;
                    }
                }
                const double2 z = S.V[bi * LD + src];
                const double r = hypot(z.x, z.y);
                S.colph[tid] = r > 0.0 ? make_double2(z.x / r, -z.y / r) : make_double2(1.0, 0.0);
                S.imax[tid] = bi;
            }
            __syncthreads();
            double2 *vb = v + b * n * nvec;
            for (int e = tid; e < n * nvec; e += WG) {
                const int i = e / nvec, j = e % nvec;
                const double2 z = S.V[i * LD + S.perm[j]];
                double2 o = zmul(z, S.colph[j]);
                if (i == S.imax[j]) o = make_double2(hypot(z.x, z.y), 0.0);
                vb[e] = o;
            }
        }
        __syncthreads();          // the next matrix overwrites A, V and the tables
    }
}

size_t eigh_lds_bytes(int NP, bool vec) {
    switch (NP) {
    case 8: return vec ? sizeof(EighLds<8, true>) : sizeof(EighLds<8, false>);
    case 16: return vec ? sizeof(EighLds<16, true>) : sizeof(EighLds<16, false>);
    case 32: return vec ? sizeof(EighLds<32, true>) : sizeof(EighLds<32, false>);
    case 64: return vec ? sizeof(EighLds<64, true>) : sizeof(EighLds<64, false>);
    default: return 0;
    }
}
static_assert(sizeof(EighLds<64, true>) <= SP_LDS_MAX, "A and V of order 64 fit the LDS of one CU");
static_assert(EighCfg<8>::WG == 64 && EighCfg<16>::WG == 64 && EighCfg<32>::WG == 256 && EighCfg<64>::WG == 1024, "eigh_wg_of");

int launch_eigh(LaunchCtx c, const double *a, int n, int64_t batch, int nvec, int max_sweeps, double *w, double *v, int32_t *sweeps,
                const EighPlan &pl) {
    if (n < 1 || n > SP_EIGH_MAX_N || nvec < 0 || nvec > n || batch < 1 || max_sweeps < 1 || !a || !w || !sweeps || (nvec > 0 && !v))
        return -1;
    if (pl.NP != eigh_np_of(n) || pl.grid < 1 || pl.grid > batch || pl.grid > 0x7fffffff ||
        pl.lds_bytes != eigh_lds_bytes(pl.NP, nvec > 0) || pl.lds_bytes > SP_LDS_MAX)
        return -1;
#define L_(NPv, VE)                                                                                   \
    {                                                                                                 \
        if (lds_raise<k_eigh<NPv, VE>>(pl.lds_bytes)) return -1;                                      \
        hipLaunchKernelGGL((k_eigh<NPv, VE>), dim3((unsigned)pl.grid), dim3(EighCfg<NPv>::WG), pl.lds_bytes, c.stream,               \
                           (const double2 *)a, n, batch, nvec, max_sweeps, w, (double2 *)v, sweeps);  \
    }
#define N_(NPv)                                                                                       \
    case NPv:                                                                                         \
        if (nvec > 0) L_(NPv, true) else L_(NPv, false)                                               \
        break;
    switch (pl.NP) {
        N_(8) N_(16) N_(32) N_(64)
    default: return -1;
    }
#undef N_
#undef L_
    return 0;
}

}   // namespace sp
