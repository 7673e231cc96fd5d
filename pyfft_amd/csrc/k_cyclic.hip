// k_cyclic.hip -- spectral correlation by the averaged cyclic periodogram (Gardner 1986; Antoni 2007): for every cycle frequency
// alpha = nu fs a Welch cross spectrum between the record shifted down and up by alpha / 2.  With e(t) = exp(2 pi i t), nu_h = nu / 2,
// the frames s = g hop, a real window w of n taps and absolute sample indices first + s + j:
//   Z+[g][k] = DFT_n( w[j] (y[s + j] - m_y) e(-nu_h (first + s + j)) )
//   Z-[g][k] = DFT_n( w[j] (x'[s + j] - m_x') e(+nu_h (first + s + j)) ),   x' = conj(x) in the conjugate form, else x
//   S = sum_g Z+ conj(Z-),   Pp = sum_g |Z+|^2,   Pm = sum_g |Z-|^2
// A workgroup owns ONE alpha and, per transform group, a run of fpg consecutive frames of one row.  Every thread builds its 16
// entries of the rotated window w[j] e(-nu_h j) once, in float64 (sincospi of the exact phase: nu_h is a multiple of 2^-64 turn and
// the products wrap modulo 2^64, which IS the reduction modulo one turn), rounded to float32, and keeps them in registers -- at the
// longer transforms in LDS or in memory, see below.  The
// factor of the frame's origin, e(-+nu_h (first + s)), has modulus one and cancels in Pp and Pm; on the product Z+ conj(Z-) it
// is p2 = e(-nu (first + s)), again from a float64 sincospi of the exact phase, applied to the product before it is added.
// Forms:
//   MIRROR (a real row, or a complex row in the conjugate form; y = x): the input of Z- is the conjugate of the input of Z+, so
//           Z-[k] = conj(Z+[n - k]): ONE transform per (frame, alpha), S += p2 U[k] U[n - k] through one mirrored LDS read (MT_XRP's
//           exchange, k_mtaper.hip), and Pm[k] = Pp[n - k] is formed by the finish kernel.  Partials: |U|^2, Re, Im.
//   general (a complex row in the plain form, every cross form): two transforms.  Z- is made first and parked in the group's second
//           image, the samples of y are then loaded (from L1 / L2 when y = x) for Z+: two transforms in flight and four accumulators
//           do not fit 256 registers at 8192 points.  Partials: |U+|^2, |U-|^2, Re, Im.
// One partial per (row, alpha, group) goes to memory; k_cyclic_finish sums the groups in ascending order in float64 and writes the
// band.  No atomics: two calls agree bitwise.
// Grid: block w takes the alpha w mod A of the frame run w / A: the A workgroups of a run start together, and the record is re-read once
// per alpha from L2 or the Infinity Cache.  (Dealing a run's workgroups to one XCD was measured and is no faster: DESIGN.md.)
// Frames past the end of a group's run are clamped to the last frame and weighted 0: every load is inside the row and every
// barrier is met.
#include "launch.h"
namespace sp {

// two waves per SIMD (amdgpu_waves_per_eu): the accumulators, the window and a transform with its constants take 150 .. 240 registers,
// the next occupancy step (168) is out of reach for most lengths, and without the hint a few instantiations run over 256 into AGPRs
// and down to one wave
template <class X, bool MIRROR, bool CPLX>
__global__ __launch_bounds__(X::C::WG) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_cyclic(CycArgs a, XfTables tb) {
    const int ai = (int)(blockIdx.x % a.A);
    const int64_t bx = blockIdx.x / a.A;
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 32 && X::L <= SP_CYC_MAX_L, "power-of-two transforms of 32 .. 8192 points");
    constexpr int L = X::L;
    const int64_t row = blockIdx.y;
    const uint64_t nuh = a.nuh[ai];
    // w[j] e(-nu_h j): in registers.  One transform, from 2048 points on, where the transform's own constants take 68 .. 96 registers:
    // in an image of the group's behind the exchange image.  Two transforms, from 512 points on, where four accumulators, the window
    // and a transform no longer fit 256 registers: in a slot of the group's in memory (L1 / L2) -- a third image beside the parked Z-
    // would halve the workgroups a CU holds, and does not fit at all at 8192 points.  Every thread reads back what it wrote: no barrier.
    constexpr int PLACE = cyc_tab_place(L, MIRROR);
    constexpr bool TABL = PLACE != 0;
    const int64_t gid = bx * C::FPW + grp;
    cf tab[TABL ? 1 : C::R];
    cf *tabl = PLACE == 2 ? a.gtab + ((blockIdx.y * (int64_t)a.A + ai) * a.groups + gid) * L : smem + (size_t)(C::FPW + grp) * C::LDS_PER;
    auto tab_entry = [&](int j) {
        const uint64_t ph = nuh * (uint64_t)j;
        double sn, cs;
        sincospi(ldexp((double)(int64_t)ph, -63), &sn, &cs);
        const double wv = (double)a.win[j];
        return mk((float)(wv * cs), (float)(-(wv * sn)));
    };
    if constexpr (TABL) {
#pragma unroll 1
        for (int t = 0; t < C::R; ++t) tabl[tid + C::T * t] = tab_entry(tid + C::T * t);
    } else {
        // one entry after the other: each index is tied to the entry before it, or sixteen float64 sincospi run interleaved and
        // their temporaries, not the frame loop, set the kernel's register count
        int j = tid;
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            tab[t] = tab_entry(j);
            j += C::T;
            asm volatile("" : "+v"(j), "+v"(tab[t].x), "+v"(tab[t].y));
        }
    }
    auto tab_of = [&](int t, int tq) {
        if constexpr (TABL) return tabl[tq + C::T * t];
        else return tab[t];
    };
    // sample minus mean under an entry of the table; a real row's mean has no imaginary part
    auto rotated = [](cf e, cf smp, cf m) {
        if constexpr (CPLX) return cmul(e, smp - m);
        else return (smp.x - m.x) * e;
    };
    const float sgn = a.conj ? -1.f : 1.f;         // x' = conj(x): the sign of the imaginary part of x and of its mean
    const float *mp = a.means + 4 * row;
    cf mx = mk(mp[0], sgn * mp[1]), my = mk(mp[2], mp[3]);
    // one transform: the mean in VGPRs (load_trend, kernels.h); two: left to the compiler, which keeps it in SGPRs -- four registers
    // that the two-transform form does not have to spare at 512 and 1024 points
    if constexpr (MIRROR) asm volatile("" : "+v"(my.x), "+v"(my.y));
    const int64_t roff = row * a.x_ld;
    float a0[C::R], a1[MIRROR ? 1 : C::R];
    cf cc[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        a0[t] = 0.f;
        if constexpr (!MIRROR) a1[t] = 0.f;
        cc[t] = mk(0.f, 0.f);
    }
    const int64_t g0 = gid * a.fpg;
    for (int64_t i = 0; i < a.fpg; ++i) {
        const int64_t g = g0 + i;
        const float keep = g < a.nframes ? 1.f : 0.f;
        const int64_t s = (g < a.nframes ? g : a.nframes - 1) * a.hop;
        const int64_t base = roff + s;
        cf p2;
        {
            const uint64_t ph = (nuh << 1) * (uint64_t)(a.first + s);
            double sn, cs;
            sincospi(ldexp((double)(int64_t)ph, -63), &sn, &cs);
            p2 = mk(keep * (float)cs, keep * (float)(-sn));
        }
        // the thread's index is opaque in every frame: the sixteen 64-bit addresses of each stream of loads are otherwise hoisted
        // out of the loop and held in registers across the transforms (k_wvd.hip does the same)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        cf v[C::R];
        if constexpr (MIRROR) {
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = load_sample(a.x, base + tq + C::T * t, CPLX);
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = rotated(tab_of(t, tq), v[t], my);      // y = x: my is the row's own mean
            fwd_row(xf, v, lds, tid, n);
            asm volatile("" : "+v"(tq));
            __syncthreads();
#pragma unroll
            for (int t = 0; t < C::R; ++t) lds[tq + C::T * t] = v[t];
            __syncthreads();
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int kk = tq + C::T * t;
                const cf zm = lds[(L - kk) & (L - 1)];
                a0[t] = fmaf(keep, cnorm(v[t]), a0[t]);
                cc[t] = cc[t] + cmul(p2, cmul(v[t], zm));
            }
        } else {
            cf *park = smem + (size_t)(C::FPW + grp) * C::LDS_PER;      // Z- waits in the group's second image (this form never keeps tabl there)
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = load_sample(a.x, base + tq + C::T * t, CPLX);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                v[t] = rotated(cconj(tab_of(t, tq)), mk(v[t].x, sgn * v[t].y), mx);
            }
            fwd_row(xf, v, lds, tid, n);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                a1[t] = fmaf(keep, cnorm(v[t]), a1[t]);
                park[tq + C::T * t] = v[t];       // read back by the thread that wrote it: no barrier
            }
            asm volatile("" : "+v"(tq));
#pragma unroll
            for (int t = 0; t < C::R; ++t) v[t] = load_sample(a.y, base + tq + C::T * t, CPLX);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                v[t] = rotated(tab_of(t, tq), v[t], my);
            }
            fwd_row(xf, v, lds, tid, n);
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const cf zn = park[tq + C::T * t];
                a0[t] = fmaf(keep, cnorm(v[t]), a0[t]);
                cc[t] = cc[t] + cmul(p2, cmulc(v[t], zn));
            }
        }
    }
    constexpr int NP = MIRROR ? 3 : 4;
    float *p = a.partial + (((row * a.A + ai) * a.groups + gid) * NP) * L;
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int kk = tid + C::T * t;
        p[kk] = a0[t];
        if constexpr (!MIRROR) p[L + kk] = a1[t];
        p[(NP - 2) * L + kk] = cc[t].x;
        p[(NP - 1) * L + kk] = cc[t].y;
    }
}

// the groups of one (row, alpha) summed in ascending order in float64; band bin jb stands for the bin k = (b0 + jb) mod L
static __global__ __launch_bounds__(256) void k_cyclic_finish(const float *__restrict__ partial, int64_t groups, int64_t used, int L,
                                                              int mirror, int A, int a_off, int a_total, int b0, int nb, double scale,
                                                              cf *__restrict__ S, float *__restrict__ Pp, float *__restrict__ Pm) {
    const int jb = blockIdx.x * 256 + threadIdx.x;
    if (jb >= nb) return;
    const int ai = blockIdx.y;
    const int64_t row = blockIdx.z;
    const int np = mirror ? 3 : 4;
    const int k = (b0 + jb) & (L - 1), km = (L - k) & (L - 1);
    const float *p = partial + ((row * A + ai) * groups * np) * (int64_t)L;
    double sp = 0.0, sm = 0.0, sr = 0.0, si = 0.0;
    for (int64_t g = 0; g < used; ++g, p += (int64_t)np * L) {
        sp += (double)p[k];
        sm += (double)(mirror ? p[km] : p[L + k]);
        sr += (double)p[(np - 2) * L + k];
        si += (double)p[(np - 1) * L + k];
    }
    const int64_t o = (row * a_total + a_off + ai) * nb + jb;
    if (S) S[o] = mk((float)(scale * sr), (float)(scale * si));
    if (Pp) Pp[o] = (float)(scale * sp);
    if (Pm) Pm[o] = (float)(scale * sm);
}

int launch_cyclic(LaunchCtx c, const CycArgs &a, bool mirror, bool cplx, int L, const cf *tw, int64_t rows) {
    if (a.A < 1 || a.A > 65535 || rows < 1 || rows > 65535 || a.nframes < 1 || a.fpg < 1 || a.hop < 1 || a.blocks < 1) return -1;
    if (a.groups != a.blocks * fpw_of(L) || a.groups * a.fpg < a.nframes || !a.x || !a.y || !a.win || !a.nuh || !a.means || !a.partial ||
        (cyc_tab_place(L, mirror) == 2 && !a.gtab))
        return -1;
    if (a.blocks * a.A > 0x7fffffff) return -1;
    const size_t lds_bytes = cyc_lds_bytes(L, mirror);
    const XfTables tb{tw, nullptr, nullptr, L};
#define L_(MR, CP)                                                                                    \
    {                                                                                                 \
        if (lds_raise<k_cyclic<XT, MR, CP>>(lds_bytes)) return -1;                                    \
        hipLaunchKernelGGL((k_cyclic<XT, MR, CP>), dim3((unsigned)(a.blocks * a.A), (unsigned)rows), dim3(XT::C::WG), lds_bytes, c.stream, a, tb); \
    }
    return for_pow2<32, SP_CYC_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (mirror) {
            if (cplx) L_(true, true) else L_(true, false)
        } else {
            if (cplx) L_(false, true) else L_(false, false)
        }
        return 0;
    });
#undef L_
}

int launch_cyclic_finish(LaunchCtx c, const float *partial, int64_t groups, int64_t used, int L, bool mirror, int A, int a_off,
                         int a_total, int b0, int nb, double scale, int64_t rows, cf *S, float *Pp, float *Pm) {
    if (A < 1 || A > 65535 || rows < 1 || rows > 65535 || used < 1 || used > groups || nb < 1 || nb > L || b0 < 0 || b0 >= L) return -1;
    if (a_off < 0 || a_off + A > a_total) return -1;
    hipLaunchKernelGGL(k_cyclic_finish, dim3((unsigned)((nb + 255) / 256), (unsigned)A, (unsigned)rows), dim3(256), 0, c.stream, partial,
                       groups, used, L, mirror ? 1 : 0, A, a_off, a_total, b0, nb, scale, S, Pp, Pm);
    return 0;
}

}   // namespace sp
