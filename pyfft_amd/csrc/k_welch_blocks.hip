// k_welch_blocks.hip -- time-resolved Welch spectra: PSD, CSD (and from them the coherogram) over blocks of navg consecutive frames,
// block after block along the record.
//   a_g = win (x[g hop : g hop + L] - m_g),  b_g likewise from y_c,  X_g = FFT_L(a_g),  Y_g = FFT_L(b_g)
//   block b = frames b step .. b step + navg - 1:   Pxx[b][k] = s_k / navg sum_g |X_g[k]|^2,  Pyy[c][b][k] likewise,
//                                                   Pxy[c][b][k] = s_k / navg sum_g conj(X_g[k]) Y_g[k]     (scipy.signal.csd)
// Modelled on k_skf: frames are never materialised, and slots past the end are clamped to the record's last frame so that every load
// is unconditional and every barrier is met (they are transformed and then left out of the sums).
// Work split.  A RUN is q consecutive frames whose sum is formed once: q = navg when step >= navg (a run is a block, frames
// r step .. r step + navg - 1), q = gcd(navg, step) when step < navg (the runs tile the record, frames r q .. r q + q - 1, and block b is
// the navg / q runs from b step / q on: every frame is transformed once, whatever the block overlap).  A workgroup owns TEAMS x rpt
// consecutive runs.  Its FPW transform groups are dealt to TEAMS teams of GPT groups; a team walks its rpt runs as one sequence of
// rpt q slots (slot s = frame s % q of run s / q), GPT slots a round.  TEAMS = 1 from 256 points on; below, a spectrum has fewer bins
// than the workgroup has threads, and the teams keep them busy.
// Ownership: after the round's barrier, thread t of a team owns the bins t, t + NBP, .. and adds the team's slots of the round in
// ascending slot order into registers (BPT bins x 4 floats: at most 16 bins, 64 VGPRs, at 4096 complex points; LDS could not hold
// 8192 complex bins x 16 bytes behind two transform images).  When a run's last frame has been added the thread writes its bins
// and starts again from zero.  No atomics: every output value has one writer and a fixed order of additions (frames ascending), and
// neither depends on where in the record, the grid or the workgroup the run lies.
// Transforms.  Every record has its own transform, real records as z = a + 0i (bins 0 .. L/2 are kept).  With y a group makes X_g,
// parks it in a second image in natural order, makes Y_g, and the three products come from X and Y themselves.  Packing a real pair
// as z = a + i b into ONE transform (k_skf) was built first and dropped, for three reasons.  (1) The rounding of the packed X depends
// on the y it shares the transform with, so pxx changed in the last bits with the choice of y; now pxx is bitwise the same for every
// y and every nch.  (2) The separation X = (P + conj zm) / 2, Y = (P - conj zm) / 2i is a difference: the transform's rounding, 1e-7
// of the LARGER half, lands in both, and a channel 10^3 below the other is lost unless every frame is first balanced by powers of
// two.  (3) A coherence needs |X|^2, |Y|^2 and conj(X) Y from the same X and Y: a single frame's is then 1 to a few ulp whatever
// their ratio.  The price is two transforms per real pair and frame where the packed form took one.
// y == null: the PSD alone, one transform per frame.
// Output.  step >= navg: the final float32 pxx, pyy and complex64 pxy with s_k / navg applied.  Otherwise float32 run sums
// partial[pair][run][plane][nb] (plane 0 pxx -- pair 0 only -- 1 pyy, 2 and 3 pxy), and k_block_sum forms every block from its navg / q runs in
// ascending order in float64.
#include "launch.h"
namespace sp {

// sum of one (re, im) pair per thread over the T threads of a transform group; every thread of the workgroup must call it.
// T <= 64 and several groups per workgroup: the group is lanes of one wave (shuffles, no LDS).  Otherwise T is a multiple of 64:
// wave sums, then the group's T / 64 waves meet in its image.
template <class C> __device__ __forceinline__ cf wb_group_sum(cf s, cf *lds, int tid) {
    if constexpr (C::T <= 64 && C::FPW > 1) {
        return mk(group_lane_sum<C::T>(s.x), group_lane_sum<C::T>(s.y));
    } else {
        static_assert(C::T % 64 == 0, "whole waves");
        const cf w = mk(wave_sum64(s.x), wave_sum64(s.y));
        __syncthreads();                  // the image may still be read by the previous round's sums or the previous group sum
        if ((tid & 63) == 0) lds[tid >> 6] = w;
        __syncthreads();
        cf tot = mk(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < C::T / 64; ++j) tot = tot + lds[j];
        return tot;
    }
}

// CPLX: complex64 records (all L bins), else float32 records (bins 0 .. L/2); PAIR: with y
template <class X, bool CPLX, bool PAIR>
__global__ __launch_bounds__(X::C::WG) void k_welch_blocks(WelchBlocksArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= 8192, "power-of-two transforms of 32 .. 8192 points");
    constexpr int L = X::L, WG = C::WG, FPW = C::FPW;
    constexpr int NBP = L < WG ? L : WG;                  // threads of a team = bin stride of a thread
    constexpr int TEAMS = WG / NBP, GPT = FPW / TEAMS;    // teams, transform groups of a team
    constexpr int NB = CPLX ? L : L / 2 + 1;
    // a complex pair at 8192 points would hold 16 bins x 4 floats a thread and spill 14 registers at the 256 its 512-thread workgroup
    // leaves a wave: there the bins are split over two workgroups (grid z), each of which transforms the frames and sums its half
    constexpr int BS = welch_blocks_bin_split(CPLX, PAIR, L);
    constexpr int BPT = (NB + NBP - 1) / NBP / BS;        // bins a thread owns
    static_assert(BS == 1 || BPT * BS * NBP == NB, "the halves tile the bins");
    const int j0 = BS > 1 ? (int)blockIdx.z * BPT : 0;    // its first
    static_assert(TEAMS * NBP == WG && GPT * TEAMS == FPW && GPT >= 1, "teams tile the workgroup");
    const int wt = (int)threadIdx.x;
    const int team = grp / GPT, gi = grp - team * GPT;    // of the transform group this thread belongs to
    const int ateam = wt / NBP, abin = wt - ateam * NBP;  // of the bins this thread owns
    const int c = (int)blockIdx.y, q = a.q;
    using S = typename std::conditional<CPLX, cf, float>::type;          // a sample
    const S *__restrict__ xs = reinterpret_cast<const S *>(a.x);
    const S *__restrict__ ys = reinterpret_cast<const S *>(a.y) + (int64_t)c * a.y_ld;
    const float *__restrict__ win = a.win;
    cf *park = smem + (FPW + grp) * C::LDS_PER;           // PAIR: this group's X while Y is made
    // the runs of this thread's two teams (as a transform group, as a bin owner)
    const int64_t wg_run0 = (int64_t)blockIdx.x * TEAMS * a.rpt;
    const int64_t g_run0 = wg_run0 + (int64_t)team * a.rpt, a_run0 = wg_run0 + (int64_t)ateam * a.rpt;
    const int nslots = a.rpt * q, rounds = (nslots + GPT - 1) / GPT;
    float acc[BPT][4];
#pragma unroll
    for (int j = 0; j < BPT; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f;
    int aj = 0;                                           // the owner's walk: frame within its current run ..
    int64_t arun = a_run0;                                // .. and that run
    for (int r = 0; r < rounds; ++r) {
        const int s = r * GPT + gi;                       // this group's slot of the round
        const int sr = s / q, sj = s - sr * q;
        const int64_t run = g_run0 + sr;
        const bool live = s < nslots && run < a.runs;
        // slots past the end are clamped to the record's last frame
        const int64_t g = live ? run * a.rstride + sj : a.nframes - 1;
        const int64_t base = g * a.hop;
        int tq = tid;                                     // opaque in every round (as in k_skf: taper and offsets are not hoisted)
        asm volatile("" : "+v"(tq));
        auto taper = [&](int j) __attribute__((always_inline)) { return win != nullptr ? win[j] : 1.f; };
        cf v[C::R];
        auto prep = [&](const S *__restrict__ src, cf (&rr)[C::R]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                if constexpr (CPLX) rr[t] = src[base + tq + C::T * t];
                else rr[t] = mk(src[base + tq + C::T * t], 0.f);
            }
            if (a.segmean) {
                cf sm = mk(0.f, 0.f);
#pragma unroll
                for (int t = 0; t < C::R; ++t) sm = sm + rr[t];
                const cf m = (1.f / (float)L) * wb_group_sum<C>(sm, lds, tq);
#pragma unroll
                for (int t = 0; t < C::R; ++t) rr[t] = rr[t] - m;
            }
#pragma unroll
            for (int t = 0; t < C::R; ++t) rr[t] = taper(tq + C::T * t) * rr[t];
        };
        prep(xs, v);
        if constexpr (PAIR) {
            fwd_row(xf, v, lds, tid, n);
            // X waits in the second image, in natural order; nobody reads it before the barrier in front of the sums
#pragma unroll
            for (int t = 0; t < C::R; ++t) park[tq + C::T * t] = v[t];
            prep(ys, v);
        }
        fwd_row(xf, v, lds, tid, n);
        __syncthreads();                  // the image may still be read by the transform
#pragma unroll
        for (int t = 0; t < C::R; ++t) lds[tq + C::T * t] = v[t];
        __syncthreads();                  // every group's spectrum is in its image
        // the sums: ownership by team thread, the team's slots of the round in ascending order
        for (int u = 0; u < GPT; ++u) {
            const int su = r * GPT + u;
            if (su >= nslots || arun >= a.runs) break;    // uniform over the team; nothing follows a dead slot
            const cf *img = smem + (ateam * GPT + u) * C::LDS_PER;
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const int k = abin + NBP * (j0 + j);
                if (BPT * BS * NBP == NB || k < NB) {
                    if constexpr (PAIR) {
                        const cf xk = img[FPW * C::LDS_PER + k], yk = img[k];
                        acc[j][0] += cnorm(xk);
                        acc[j][1] += cnorm(yk);
                        acc[j][2] += xk.x * yk.x + xk.y * yk.y;                                         // conj(X) Y
                        acc[j][3] += xk.x * yk.y - xk.y * yk.x;
                    } else {
                        acc[j][0] += cnorm(img[k]);
                    }
                }
            }
            if (++aj == q) {              // the run is complete: out with it, and from zero again
#pragma unroll
                for (int j = 0; j < BPT; ++j) {
                    const int k = abin + NBP * (j0 + j);
                    if (BPT * BS * NBP == NB || k < NB) {
                        if (a.partial != nullptr) {
                            float *o = a.partial + (((int64_t)c * a.runs + arun) * a.planes) * NB + k;
                            if (c == 0) o[0] = acc[j][0];
                            if constexpr (PAIR) {
                                o[NB] = acc[j][1];
                                o[2 * NB] = acc[j][2];
                                o[3 * NB] = acc[j][3];
                            }
                        } else {
                            const float m = (!CPLX && k >= 1 && k < L / 2) ? a.mult2 : a.mult;
                            if (c == 0) a.pxx[arun * NB + k] = m * acc[j][0];
                            if constexpr (PAIR) {
                                const int64_t o = ((int64_t)c * a.runs + arun) * NB + k;
                                a.pyy[o] = m * acc[j][1];
                                a.pxy[o] = mk(m * acc[j][2], m * acc[j][3]);
                            }
                        }
                    }
                    acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.f;
                }
                aj = 0;
                ++arun;
            }
        }
        __syncthreads();                  // the images are free for the next round
    }
}

// block b = the nsum runs from b adv on, summed in float64 in ascending order; a thread owns one bin of one block of one pair
#define WB_SUM_WG 256
static __global__ __launch_bounds__(WB_SUM_WG) void k_block_sum(const float *__restrict__ partial, int64_t runs, int planes, int nb,
                                                                 int64_t nblocks, int adv, int nsum, int dbl_lo, int dbl_hi, double mult,
                                                                 float *__restrict__ pxx, float *__restrict__ pyy, cf *__restrict__ pxy) {
    const int k = (int)blockIdx.y * WB_SUM_WG + (int)threadIdx.x;
    if (k >= nb) return;
    const int64_t b = blockIdx.x;
    const int c = (int)blockIdx.z;
    const float *p = partial + (((int64_t)c * runs + b * adv) * planes) * nb + k;
    const int64_t rs = (int64_t)planes * nb;
    const double m = (k >= dbl_lo && k < dbl_hi) ? 2.0 * mult : mult;
    if (c == 0) {
        double s = 0.0;
        for (int i = 0; i < nsum; ++i) s += (double)p[i * rs];
        pxx[b * nb + k] = (float)(m * s);
    }
    if (planes == 4) {
        double sy = 0.0, sr = 0.0, si = 0.0;
        for (int i = 0; i < nsum; ++i) {
            sy += (double)p[i * rs + nb];
            sr += (double)p[i * rs + 2 * (int64_t)nb];
            si += (double)p[i * rs + 3 * (int64_t)nb];
        }
        const int64_t o = ((int64_t)c * nblocks + b) * nb + k;
        pyy[o] = (float)(m * sy);
        pxy[o] = mk((float)(m * sr), (float)(m * si));
    }
}

int launch_welch_blocks(LaunchCtx c, const WelchBlocksArgs &a, bool cplx, int L, const cf *tw, int pairs, int64_t wgs) {
    const bool have_y = a.y != nullptr;
    if (a.q < 1 || a.rpt < 1 || a.runs < 1 || a.rstride < 1 || a.hop < 1 || a.nframes < 1 || pairs < 1 || pairs > 65535) return -1;
    if ((a.runs - 1) * a.rstride + a.q > a.nframes) return -1;                           // the last run ends inside the frames
    if ((int64_t)a.rpt * a.q > 0x3fffffff) return -1;
    const int64_t per = (int64_t)welch_blocks_teams(L) * a.rpt;
    if (wgs < 1 || wgs > 0x7fffffff || wgs * per < a.runs || (wgs - 1) * per >= a.runs) return -1;
    if (a.partial != nullptr ? a.planes != (have_y ? 4 : 1) : (a.pxx == nullptr || (have_y && (a.pyy == nullptr || a.pxy == nullptr))))
        return -1;
    if (!have_y && pairs != 1) return -1;
    const size_t lds = welch_blocks_lds_bytes(have_y, L);
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(CP, PR)                                                                                    \
    {                                                                                                 \
        if (lds_raise<k_welch_blocks<XT, CP, PR>>(lds)) return -1;                                    \
        hipLaunchKernelGGL((k_welch_blocks<XT, CP, PR>), dim3((unsigned)wgs, (unsigned)pairs, (unsigned)welch_blocks_bin_split(CP, PR, XT::L)), dim3(XT::C::WG), lds, c.stream, a, tb); \
    }
    return for_pow2<32, 8192>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (cplx) {
            if (have_y) L_(true, true) else L_(true, false)
        } else {
            if (have_y) L_(false, true) else L_(false, false)
        }
        return 0;
    });
#undef L_
}

int launch_block_sum(LaunchCtx c, const float *partial, int64_t runs, int planes, int nb, int64_t nblocks, int adv, int nsum, bool dbl,
                     int L, double mult, int pairs, float *pxx, float *pyy, cf *pxy) {
    if (runs < 1 || (planes != 1 && planes != 4) || nb < 1 || nblocks < 1 || nblocks > 0x7fffffff || adv < 1 || nsum < 1 ||
        (nblocks - 1) * adv + nsum > runs || pairs < 1 || pairs > 65535)
        return -1;
    hipLaunchKernelGGL(k_block_sum, dim3((unsigned)nblocks, (unsigned)((nb + WB_SUM_WG - 1) / WB_SUM_WG), (unsigned)pairs),
                       dim3(WB_SUM_WG), 0, c.stream, partial, runs, planes, nb, nblocks, adv, nsum, dbl ? 1 : 0, dbl ? L / 2 : 0, mult, pxx,
                       pyy, pxy);
    return 0;
}

}   // namespace sp
