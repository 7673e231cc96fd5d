// k_wvd.hip -- the smoothed pseudo Wigner-Ville distribution, a member of Cohen's class with a separable kernel (Flandrin 1984;
// Auger & Flandrin 1995).  With z, y complex rows that are zero outside 0 .. nsig - 1, a lag window h of 2 Lh + 1 taps, a time window g
// of 2 Lg + 1 taps (both indexed from -L) and the column times n_j = first + j hop:
//   K[j][tau] = h[tau] sum_mu g[mu] z[n_j + mu + tau] conj(y[n_j + mu - tau]),   tau = -Lh .. Lh, 0 for the other lags
//   W[j][k]   = scale sum_tau K[j][tau] exp(-2 pi i k tau / L)
// One fused kernel: K never leaves the workgroup.  A workgroup owns a run of cpr consecutive columns of one row and stages the samples
// of z the run touches in LDS once (behind the transform images; zeros outside the row); a round deals FPW transforms to its FPW groups.
// Lag products.  Thread t of a group owns the lags t, t + T, ..: it walks mu in ascending order, forms z[m + tau] conj(y[m - tau])
// and adds it under g[mu], whose index is uniform over the workgroup (a scalar load of the table).  K goes to the group's image at
// tau mod L, so that the transform needs no phase factor afterwards; the image is then read back in the transform's register layout.
// Auto (y = z): K is Hermitian in tau (h is symmetric: the host folds it), so only the lags 0 .. Lh are formed and the mirror image is
// the conjugate; and W is real, so the columns 2p and 2p + 1 of a row share one transform: v = K_a + i K_b, W_a = Re V, W_b = Im V.
// The two columns also share the lag products where their time windows overlap (hop < 2 Lg + 1): ng + hop products instead of 2 ng.
// The pairing belongs to the ROW, not to the run: a run that starts on an odd column or ends on an even one forms the whole pair and
// stores the column it owns, and the partner of an odd last column is that column itself.  Every column is therefore computed from the
// same values in the same order whatever the partition, and two partitions agree bitwise.
// Cross: one transform per column, all 2 Lh + 1 lags; y comes through the caches (staging both rows would not fit at 8192 points).
// Groups past the end of the run are clamped to its last transform: every barrier is met, nothing of theirs is stored.
// A column whose time window n_j - Lg .. n_j + Lg misses the record has no product at all: it is stored as zeros (in a shared
// transform the partner's rounding would otherwise leak into it).
#include "launch.h"
namespace sp {

template <class X, bool CROSS>
__global__ __launch_bounds__(X::C::WG) void k_wvd(WvdArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= SP_WVD_MAX_L, "power-of-two transforms of 32 .. 8192 points");
    constexpr int L = X::L, NLAG = CROSS ? C::R : C::R / 2;
    cf *zs = smem + (size_t)C::FPW * C::LDS_PER;
    const cf *__restrict__ xrow = a.x + (int64_t)blockIdx.y * a.x_ld;
    const cf *__restrict__ yrow = CROSS ? a.y + (int64_t)blockIdx.y * a.x_ld : nullptr;
    const float *__restrict__ hw = a.h, *__restrict__ gw = a.g;
    const int Lh = a.Lh, Lg = a.Lg, pad = Lh + Lg, ng = 2 * Lg + 1;
    const int64_t r0 = (int64_t)blockIdx.x * a.cpr;
    const int64_t r1 = r0 + a.cpr < a.ntimes ? r0 + a.cpr : a.ntimes;   // the run's columns: r0 .. r1 - 1
    // the staged columns c0 .. c1: auto, whole pairs
    const int64_t c0 = CROSS ? r0 : (r0 & ~(int64_t)1);
    const int64_t c1 = CROSS ? r1 - 1 : (((r1 - 1) | 1) < a.ntimes ? ((r1 - 1) | 1) : a.ntimes - 1);
    const int64_t s0 = a.first + c0 * a.hop - pad;                       // the sample staged at zs[0]
    const int span = (int)((c1 - c0) * a.hop) + 2 * pad + 1;
    for (int i = (int)threadIdx.x; i < span; i += C::WG) {
        const int64_t gi = s0 + i;
        cf z = mk(0.f, 0.f);
        if (gi >= 0 && gi < a.nsig) z = xrow[gi];
        zs[i] = z;
    }
    __syncthreads();
    // transforms of the run: auto, the pairs u = column / 2
    const int64_t u0 = CROSS ? r0 : c0 >> 1, u1 = CROSS ? r1 - 1 : c1 >> 1;
    for (int64_t ub = u0; ub <= u1; ub += C::FPW) {
        const int64_t u = ub + grp;
        const bool act = u <= u1;
        const int64_t uc = act ? u : u1;
        const int64_t ca = CROSS ? uc : 2 * uc;
        const int64_t cb = CROSS ? ca : (2 * uc + 1 < a.ntimes ? 2 * uc + 1 : a.ntimes - 1);
        const int oa = (int)((ca - c0) * a.hop) + pad - Lg, ob = (int)((cb - c0) * a.hop) + pad - Lg;   // zs index of z[n - Lg]
        int tq = tid;
        asm volatile("" : "+v"(tq));
#pragma unroll 1
        for (int t = 0; t < NLAG; ++t) {
            const int e = tq + C::T * t;
            if constexpr (!CROSS) {
                cf ka = mk(0.f, 0.f), kb = mk(0.f, 0.f);                 // e = tau = 0 .. L/2 - 1
                if (e <= Lh) {
                    // the products of column b are those of column a `shift` samples on: where the two time windows overlap a
                    // product is formed once and added to both (each column's sum keeps its ascending order)
                    const cf *pa = zs + oa, *pb = zs + ob;
                    const int shift = ob - oa, lap = shift < ng ? shift : ng;
                    for (int m = 0; m < lap; ++m) {
                        const cf p = cmulc(pa[m + e], pa[m - e]);
                        const float gm = gw[m];
                        ka = mk(fmaf(gm, p.x, ka.x), fmaf(gm, p.y, ka.y));
                    }
                    for (int m = lap; m < ng; ++m) {
                        const cf p = cmulc(pa[m + e], pa[m - e]);
                        const float gm = gw[m], gq = gw[m - shift];
                        ka = mk(fmaf(gm, p.x, ka.x), fmaf(gm, p.y, ka.y));
                        kb = mk(fmaf(gq, p.x, kb.x), fmaf(gq, p.y, kb.y));
                    }
                    for (int m = ng - lap; m < ng; ++m) {
                        const cf q = cmulc(pb[m + e], pb[m - e]);
                        const float gq = gw[m];
                        kb = mk(fmaf(gq, q.x, kb.x), fmaf(gq, q.y, kb.y));
                    }
                    const float hv = hw[Lh + e];
                    ka = hv * ka;
                    kb = hv * kb;
                }
                lds[e] = mk(ka.x - kb.y, ka.y + kb.x);                   // K_a + i K_b
                if (e) lds[L - e] = mk(ka.x + kb.y, kb.x - ka.y);        // conj K_a + i conj K_b
            } else {
                const int tau = e <= L / 2 ? e : e - L;
                cf k = mk(0.f, 0.f);
                if (tau >= -Lh && tau <= Lh) {
                    const cf *pa = zs + oa;
                    const int64_t yb = a.first + ca * a.hop - Lg - tau;      // the sample of y under g[-Lg]
                    for (int m = 0; m < ng; ++m) {
                        const int64_t yi = yb + m;
                        cf w = mk(0.f, 0.f);
                        if (yi >= 0 && yi < a.nsig) w = yrow[yi];
                        const float gm = gw[m];
                        const cf p = cmulc(pa[m + tau], w);
                        k = mk(fmaf(gm, p.x, k.x), fmaf(gm, p.y, k.y));
                    }
                    k = hw[Lh + tau] * k;
                }
                lds[e] = k;
            }
        }
        if constexpr (!CROSS) {
            if (tq == 0) lds[L / 2] = mk(0.f, 0.f);
        }
        __syncthreads();                  // K is in the group's image
        cf v[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) v[t] = lds[tq + C::T * t];
        __syncthreads();                  // the transform exchanges through the image
        fwd_row(xf, v, lds, tid, n);
        if (act) {
            const int64_t na = a.first + ca * a.hop, nb_ = a.first + cb * a.hop;
            const bool sa = ca >= r0 && ca < r1, sb = !CROSS && cb != ca && cb < r1;
            const bool za = na + Lg < 0 || na - Lg >= a.nsig, zb = nb_ + Lg < 0 || nb_ - Lg >= a.nsig;
            const int64_t rowa = ((int64_t)blockIdx.y * a.ntimes + ca) * a.nb, rowb = ((int64_t)blockIdx.y * a.ntimes + cb) * a.nb;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int jb = (tq + C::T * t - a.b0) & (L - 1);
                if (jb < a.nb) {
                    if constexpr (CROSS) {
                        if (sa) st_stream(reinterpret_cast<cf *>(a.W) + rowa + jb, za ? mk(0.f, 0.f) : a.scale * v[t]);
                    } else {
                        if (sa) st_stream(reinterpret_cast<float *>(a.W) + rowa + jb, za ? 0.f : a.scale * v[t].x);
                        if (sb) st_stream(reinterpret_cast<float *>(a.W) + rowb + jb, zb ? 0.f : a.scale * v[t].y);
                    }
                }
            }
        }
        __syncthreads();                  // the image is free for the next round
    }
}

int launch_wvd(LaunchCtx c, const WvdArgs &a, int L, const cf *tw, int64_t runs, int64_t rows, size_t lds_bytes) {
    const bool cross = a.y != nullptr;
    const int nh = 2 * a.Lh + 1, ng = 2 * a.Lg + 1;
    if (a.ntimes < 1 || a.cpr < 1 || a.cpr > a.ntimes || !runs_cover(a.ntimes, a.cpr, runs)) return -1;
    if (rows < 1 || rows > 65535 || a.hop < 1 || a.nsig < 1 || a.x_ld < a.nsig || !a.x || !a.h || !a.g || !a.W) return -1;
    if (a.Lh < 0 || nh > L - 1 || a.Lg < 0 || ng > SP_WVD_MAX_NG || a.nb < 1 || a.nb > L || a.b0 < 0 || a.b0 >= L) return -1;
    if (a.hop > SP_WVD_MAX_SPAN / a.ntimes || a.first > SP_WVD_MAX_SPAN || a.first < -SP_WVD_MAX_SPAN) return -1;
    if (lds_bytes > SP_LDS_MAX || lds_bytes != wvd_lds_bytes(cross, L, nh, ng, a.hop, a.cpr, a.ntimes)) return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(CR)                                                                                        \
    {                                                                                                 \
        if (lds_raise<k_wvd<XT, CR>>(lds_bytes)) return -1;                                           \
        hipLaunchKernelGGL((k_wvd<XT, CR>), dim3((unsigned)runs, (unsigned)rows), dim3(XT::C::WG), lds_bytes, c.stream, a, tb); \
    }
    return for_pow2<32, SP_WVD_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (cross) L_(true) else L_(false)
        return 0;
    });
#undef L_
}

}   // namespace sp
