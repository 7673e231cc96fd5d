// k_beam.hip -- the wavenumber (mode-number, slowness) scan of a sensor array from the eigendecompositions of its cross-spectral-density
// matrices (include/spectral_array.h; the host's arithmetic in beam_plan.h).  A model s is one frequency bin: V, w as k_eigh writes them.
// With the steering vector a_q(s)[i] = e(phi), phi = scale[s] sum_d pos[i][d] kv[q][d] in turns, all four classical estimators are
//   D[s, q] = sum_k g_k(s) |a_q(s)^H v_k(s)|^2
// under the weights g_k = w_k (Bartlett), 1 / (w_k + delta) (Capon), 1 for k >= p (MUSIC), 1 / w_k for k >= p (eigenvector method);
// P = D / m^2 for Bartlett and 1 / D otherwise (a sum of zero gives 0).
// Kernel:
//   k_beam   a workgroup of BEAM_WAVES waves walks (model, tile of BEAM_TQ steering vectors) items.  It writes the tile a[i][q] into LDS,
//           q fastest: one sincospi per (sensor, steering vector), the phase formed by separately rounded products and sums and reduced
//           to a turn in float64.  The eigenvectors stream through LDS BEAM_KS at a time as vec[i][kk], the next stage fetched into
//           registers while the present one is used.  Lane q of wave v projects its steering vector on the BEAM_KB vectors
//           v BEAM_KB .. of the stage at once: per sensor one 16-byte read of a (neighbouring lanes, neighbouring slots) and BEAM_KB
//           wave-uniform reads of v against 4 BEAM_KB multiply-adds.  Sums run i ascending inside a projection and k ascending inside a
//           wave; the waves' partial sums are added in wave order through LDS by wave 0, which writes the row.  The weights and the flag
//           are wave 0's too: lane k holds w_k, the trace for Capon's loading is summed k ascending out of the lanes.
// Every output element is written once, by one thread, and nothing is cleared first.  No atomics.
#include "launch.h"
namespace sp {

struct BeamArgs {
    const double2 *V;
    int64_t V_ld;
    const double *w;
    int m, ndim, method, p;
    const double *pos, *kv, *scale;       // device copies of the host tables; scale may be nullptr
    int64_t nk, tiles, items;
    double loading;
    void *P;
    int64_t P_ld;
    int *status;
};

// the denominator of a weight that has one, and whether the weight counts
static __device__ __forceinline__ double beam_weight(int method, double wk, double delta, bool *bad) {
    if (method == BEAM_BARTLETT) return wk;
    if (method == BEAM_MUSIC) return 1.0;
    const double den = method == BEAM_CAPON ? __dadd_rn(wk, delta) : wk;
    if (!(den > 0.0)) {
        *bad = true;
        return 0.0;
    }
    return 1.0 / den;
}

// v of lane k, k the same in every lane
static __device__ __forceinline__ double beam_lane(double v, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

// the phase of a turn: every product and every sum rounded on its own, as the definition's, and reduced in float64.  __dmul_rn and
// __dadd_rn are a plain product and a plain sum to the compiler, which contracts the one into the other once both are inlined; a sum
// written here, with contraction off for this function, takes no product in
static __device__ __forceinline__ double beam_turn(const double *r, const double *kq, int ndim, double sc) {
#pragma clang fp contract(off)
    double t = __dmul_rn(r[0], kq[0]);
    for (int d = 1; d < ndim; ++d) {
        const double u = __dmul_rn(r[d], kq[d]);
        t = t + u;
    }
    const double ph = __dmul_rn(sc, t);
    return ph - floor(ph);
}

template <bool O64> static __global__ __launch_bounds__(BEAM_WG) void k_beam(BeamArgs A) {
    extern __shared__ __attribute__((aligned(16))) char beam_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
    double2 *steer = (double2 *)beam_smem;                               // [m][BEAM_TQ]
    double2 *vec = steer + m * BEAM_TQ;                                  // [m][BEAM_KS]
    double *part = (double *)(vec + m * BEAM_KS);                        // [BEAM_WAVES][BEAM_TQ]
    double *gw = part + BEAM_WAVES * BEAM_TQ;                            // the weights, zero behind the last
    const int k_lo = beam_first(A.method, A.p), nn = m - k_lo, nst = (nn + BEAM_KS - 1) / BEAM_KS;
    constexpr int VPT = BEAM_MAX_M * BEAM_KS / BEAM_WG;                  // elements of a stage a thread fetches
    for (int64_t item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int64_t model = item / A.tiles, tile = item - model * A.tiles, q0 = tile * BEAM_TQ;
        const double2 *V = A.V + model * m * A.V_ld;
        const double *w = A.w + model * m;
        const double sc = A.scale ? A.scale[model] : 1.0;
        __syncthreads();                                                 // the item before has been read out of LDS
        // the weights and the flag, by the first wave alone while the others begin the steering tile: lane l holds w[l], the trace is
        // summed k ascending out of the lanes (no load inside the sum), lane l owns the weight of vector k_lo + l
        if (wv == 0) {
            const double wl = lane < m ? w[lane] : 0.0;
            double delta = 0.0;
            if (A.method == BEAM_CAPON) {
                double tr = beam_lane(wl, 0);
                for (int k = 1; k < m; ++k) tr = __dadd_rn(tr, beam_lane(wl, k));
                delta = __dmul_rn(A.loading, tr > 0.0 ? tr : 0.0) / (double)m;
            }
            bool bad = false;
            double g = 0.0;
            if (lane < nn) g = beam_weight(A.method, w[k_lo + lane], delta, &bad);
            gw[lane] = g;                                                // zero behind the last
            const int flag = __any(bad ? 1 : 0);
            if (tile == 0 && lane == 0) A.status[model] = flag ? 1 : 0;
        }
        // the steering tile
        for (int idx = tid; idx < m * BEAM_TQ; idx += BEAM_WG) {
            const int i = idx / BEAM_TQ, ql = idx - i * BEAM_TQ;
            const int64_t q = q0 + ql;
            double sn = 0.0, cs = 1.0;
            if (q < A.nk) {
                const double fr = beam_turn(A.pos + i * A.ndim, A.kv + q * A.ndim, A.ndim, sc);
                sincospi(2.0 * fr, &sn, &cs);
            }
            steer[idx] = make_double2(cs, sn);
        }
        // the eigenvectors, a stage at a time
        double2 pre[VPT];
        auto fetch = [&](int st) {
            const int k0 = st * BEAM_KS, kc = nn - k0 < BEAM_KS ? nn - k0 : BEAM_KS;
#pragma unroll
            for (int j = 0; j < VPT; ++j) {
                const int idx = tid + j * BEAM_WG, i = idx / BEAM_KS, kk = idx - i * BEAM_KS;
                pre[j] = (i < m && kk < kc) ? V[i * A.V_ld + k_lo + k0 + kk] : make_double2(0.0, 0.0);
            }
        };
        fetch(0);
        double den = 0.0;
        for (int st = 0; st < nst; ++st) {
            const int k0 = st * BEAM_KS, kc = nn - k0 < BEAM_KS ? nn - k0 : BEAM_KS;
            __syncthreads();                                             // the stage before has been used
#pragma unroll
            for (int j = 0; j < VPT; ++j) {
                const int idx = tid + j * BEAM_WG;
                if (idx < m * BEAM_KS) vec[idx] = pre[j];
            }
            __syncthreads();                                             // (the first also holds the steering tile and the weights)
            if (st + 1 < nst) fetch(st + 1);
            const int kb = wv * BEAM_KB;
            if (kb < kc) {
                double2 acc[BEAM_KB];
#pragma unroll
                for (int j = 0; j < BEAM_KB; ++j) acc[j] = make_double2(0.0, 0.0);
                const double2 *ap = steer + lane, *vp = vec + kb;
                for (int i = 0; i < m; ++i) {
                    const double2 a = ap[i * BEAM_TQ];
#pragma unroll
                    for (int j = 0; j < BEAM_KB; ++j) {                  // conj(a) v
                        const double2 v = vp[i * BEAM_KS + j];
                        acc[j].x = fma(a.y, v.y, fma(a.x, v.x, acc[j].x));
                        acc[j].y = fma(-a.y, v.x, fma(a.x, v.y, acc[j].y));
                    }
                }
#pragma unroll
                for (int j = 0; j < BEAM_KB; ++j) den += gw[k0 + kb + j] * (acc[j].x * acc[j].x + acc[j].y * acc[j].y);
            }
        }
        part[wv * BEAM_TQ + lane] = den;
        __syncthreads();
        if (wv == 0 && q0 + lane < A.nk) {
            double D = part[lane];
            for (int v = 1; v < BEAM_WAVES; ++v) D += part[v * BEAM_TQ + lane];
            const double out = A.method == BEAM_BARTLETT ? D / (double)(m * m) : (D > 0.0 ? 1.0 / D : 0.0);   // no weight: zeros, never NaN
            const int64_t o = model * A.P_ld + q0 + lane;
            if (O64) ((double *)A.P)[o] = out;
            else ((float *)A.P)[o] = (float)out;
        }
    }
}

// ---- launch glue -------------------------------------------------------------------------------------------------------------------------
int launch_beam(LaunchCtx c, const void *V, int64_t V_ld, const double *w, int m, int64_t nmodels, const double *pos, int ndim, const double *kv, int64_t nk,
                const double *scale, int method, int p, double loading, bool out64, void *P, int64_t P_ld, int *status, int64_t grid) {
    if (!V || !w || !pos || !kv || !P || !status || V_ld < m || P_ld < nk || nmodels < 1 || beam_shape(m, ndim, nk, nmodels, method, p) || !(loading >= 0.0))
        return -1;
    const BeamPlan b = beam_plan_of(m, nk, nmodels, method, p, 0);
    if (grid < 1 || grid > b.items || grid > 0x7fffffff) return -1;
    static_assert(BEAM_MAX_M * BEAM_KS % BEAM_WG == 0 && BEAM_TQ == 64 && BEAM_MAX_M <= 64 && BEAM_WG <= 1024,
                  "a stage is dealt evenly to the threads; a lane per steering vector and per eigenvalue");
    static_assert((size_t)BEAM_MAX_M * (BEAM_TQ + BEAM_KS) * 16 + BEAM_WAVES * BEAM_TQ * 8 + (BEAM_MAX_M + BEAM_KS) * 8 <= SP_LDS_MAX, "k_beam fits the LDS of a CU");
    BeamArgs A{};
    A.V = (const double2 *)V, A.V_ld = V_ld, A.w = w, A.m = m, A.ndim = ndim, A.method = method, A.p = p;
    A.pos = pos, A.kv = kv, A.scale = scale, A.nk = nk, A.tiles = b.tiles, A.items = b.items, A.loading = loading;
    A.P = P, A.P_ld = P_ld, A.status = status;
    const size_t lds = (size_t)b.lds_bytes;
    if (out64) {
        if (lds_raise<k_beam<true>>(lds)) return -1;
        hipLaunchKernelGGL(k_beam<true>, dim3((unsigned)grid), dim3(BEAM_WG), lds, c.stream, A);
    } else {
        if (lds_raise<k_beam<false>>(lds)) return -1;
        hipLaunchKernelGGL(k_beam<false>, dim3((unsigned)grid), dim3(BEAM_WG), lds, c.stream, A);
    }
    return 0;
}

}   // namespace sp
