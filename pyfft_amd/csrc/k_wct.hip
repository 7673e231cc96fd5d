// k_wct.hip -- cross-wavelet spectra and wavelet coherence (Torrence & Webster 1999) on the overlap-save frames of k_cwt.hip.
//   Wx, Wy          the continuous wavelet transforms of two records, as k_cwt forms them (the same filter, evaluated on the fly)
//   Wxy             = Wx conj(Wy)                                                          -- the cross-wavelet transform, and all of it
//   a, b, c         = |Wx|^2 / s', |Wy|^2 / s', Wxy / s' on 0 <= n < N, zero outside
//   A_t, B_t, C_t   = a, b, c convolved along n with the Gaussian whose transform is exp(-(s' w_k)^2 / 2), w_k the signed bin frequency
//   A, B, C         = A_t, B_t, C_t summed over neighbouring scales with the taps of the caller (k_wct_scale)
//   R2 = |C|^2 / (A B),  phase = atan2(Im C, Re C),  both 0 where A B == 0
// k_wct_time: frames of L samples with the margin M = Mw + Mg (the reach of the wavelets plus that of the Gaussians), hop = L - 2 M; the
// loads are clamped and unconditional, selected to zero outside the record, and every barrier is met by every thread; groups past the
// last frame repeat it and write nothing.  A transform group loads x and y once, transforms both and keeps the bins 1 .. L / 2 of
// either spectrum (the filter is zero elsewhere): in registers below 2048 points, in an LDS stash of L / 2 complex per record from
// there on (bin L / 2 in the slot of bin 0, thread 0's own; every thread reads back only slots it wrote itself: no barrier).  Per scale: two filtered inverse
// transforms give Wx and Wy, valid on [Mw, L - Mw); the products go through forward transform, Gaussian (one v_exp_f32 per bin, the
// 1 / L of the inverse an exact factor beside it) and inverse transform as the two complex records a + i b and c -- the Gaussian's kernel is real,
// so the first returns A_t + i B_t with nothing to unpack -- and the elements M .. M + hop - 1 are stored, 16 bytes per sample.  Six
// transforms per scale and frame, no atomics, a fixed order of operations.  Grid: frame blocks x scale chunks x rows.
#include "launch.h"
namespace sp {

// v <- the linear filter exp(-u^2 / 2) / L, u = step x (signed bin), applied to v by forward transform, product and inverse transform.
// The 1 / L of the inverse is an exact power of two beside the exponential, not a term -ln L inside it: v_exp_f32 takes the exponent
// times log2(e) rounded to float32, so a constant of -9 in it costs the filter's unit gain at the lowest bins 5e-7 at 8192 points, and
// a and b, which are positive and live there, show that at their peaks as several 1e-6 of the row rms.
template <class X> __device__ __forceinline__ void wct_smooth(const X &xf, cf (&v)[X::C::R], cf *lds, int tid, int n, float step) {
    using C = typename X::C;
    fwd_row(xf, v, lds, tid, n);
    __builtin_amdgcn_sched_barrier(0);
    int tq = tid;                                                          // opaque, as in the scale loop below
    asm volatile("" : "+v"(tq));
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int k = tq + C::T * t;
        const float u = (float)(k <= X::L / 2 ? k : k - X::L) * step;
        const float gk = __expf(-0.5f * u * u) * (1.f / (float)X::L);
        v[t] = mk(gk * v[t].x, -gk * v[t].y);                              // the first conj of conj . forward . conj
    }
    __builtin_amdgcn_sched_barrier(0);
    fwd_row(xf, v, lds, tid, n);
#pragma unroll
    for (int t = 0; t < C::R; ++t) v[t].y = -v[t].y;
}

// XWT: the cross-wavelet transform alone.  (A compile-time mode: as a run-time branch inside the scale loop it cost the coherence
// form 40 registers, and the 8192-point instantiation spilled.)
template <class X, bool XWT> __global__ __launch_bounds__(X::C::WG) void k_wct_time(WctArgs a, XfTables tb) {
    SP_KERNEL_PROLOGUE(X)
    static_assert(X::EXACT && X::L >= 256 && X::C::R == 16, "power-of-two transforms of at least 256 points");
    constexpr int L = X::L, H = L / 2, RH = C::R / 2;
    constexpr bool STASH = wct_stash(L);
    const int64_t g = (int64_t)blockIdx.x * C::FPW + grp;
    // groups past the last frame repeat it and write nothing
    const bool act = g < a.nframes;
    const int64_t n0 = (act ? g : a.nframes - 1) * a.hop;              // the frame's first output sample
    const int row = blockIdx.z;
    const int s_lo = blockIdx.y * a.chunk, s_hi = s_lo + a.chunk < a.S ? s_lo + a.chunk : a.S;
    const int64_t N = a.nsig;
    cf *sx = STASH ? smem + C::FPW * C::LDS_PER + grp * L : nullptr, *sy = STASH ? sx + H : nullptr;
    cf xs[C::R], ys[C::R];
#pragma unroll
    for (int t = 0; t < C::R; ++t) {
        const int64_t i = n0 - a.M + tid + C::T * t;
        const int64_t ic = i < 0 ? 0 : (i < N ? i : N - 1);
        const cf sa = load_sample(a.x, (int64_t)row * a.x_ld + ic, a.cplx != 0);
        const cf sb = load_sample(a.y, (int64_t)row * a.y_ld + ic, a.cplx != 0);
        xs[t] = i == ic ? sa : mk(0.f, 0.f);
        ys[t] = i == ic ? sb : mk(0.f, 0.f);
    }
    fwd_row(xf, xs, lds, tid, n);
    fwd_row(xf, ys, lds, tid, n);
    if constexpr (STASH) {
        // bins 0 .. L / 2 - 1 are the thread's first eight; bin L / 2 is thread 0's ninth and takes the slot of bin 0, which no filter reads
#pragma unroll
        for (int t = 0; t < RH; ++t) {
            const bool ny = t == 0 && tid == 0;
            sx[tid + C::T * t] = ny ? xs[RH] : xs[t];
            sy[tid + C::T * t] = ny ? ys[RH] : ys[t];
        }
    }
    const float fp = a.p, fa = a.a, fb = a.b, u0 = a.u0;
    for (int s = s_lo; s < s_hi; ++s) {
        const float step = a.sc[4 * s], c = a.sc[4 * s + 1], inv_s = a.sc[4 * s + 2];
        // the thread's index, opaque to the compiler in every scale (as in k_cwt: nothing that depends on it alone is hoisted out of
        // the scale loop and held in registers across the transforms)
        int tq = tid;
        asm volatile("" : "+v"(tq));
        cf vx[C::R], vy[C::R];
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int k = tq + C::T * t;
            const float u = (float)k * step, d = fmaf((float)k, step, -u0);
            float e = fmaf(-fa * d, d, fmaf(-fb, d, c));
            if (fp != 0.f) e = fmaf(fp, __logf(u), e);
            const float h = (k >= 1 && k <= H) ? __expf(e) : 0.f;
            if (t > RH) {                                                  // bins above L / 2: the spectra kept there are dead
                vx[t] = vy[t] = mk(0.f, 0.f);
                continue;
            }
            cf zx = xs[t], zy = ys[t];
            if constexpr (STASH) {
                // t == RH: thread 0 finds bin L / 2 in its slot 0; the others have h = 0 and read their own first slot, never
                // slot 0, which another wave writes and no barrier orders
                const int ks = t < RH ? k : tq;
                zx = sx[ks];
                zy = sy[ks];
            }
            vx[t] = mk(h * zx.x, -h * zx.y);                               // the first conj of conj . forward . conj
            vy[t] = mk(h * zy.x, -h * zy.y);
        }
        // (the stages are fenced for the scheduler: interleaving two of them costs more registers than a wave has at 8192 points)
        __builtin_amdgcn_sched_barrier(0);
        fwd_row(xf, vx, lds, tid, n);
        __builtin_amdgcn_sched_barrier(0);
        fwd_row(xf, vy, lds, tid, n);
        __builtin_amdgcn_sched_barrier(0);
        // Wx = conj(vx), Wy = conj(vy):  Wx conj(Wy) = conj(vx) vy
        if constexpr (XWT) {
            cf *__restrict__ Wrow = a.Wxy + ((int64_t)row * a.S + s) * N;
#pragma unroll
            for (int t = 0; t < C::R; ++t) {
                const int j = tq + C::T * t;
                const int64_t nn = n0 - a.M + j;
                const bool ok = act && j >= a.M && j < a.M + a.hop && nn < N;
                const cf w = mk(fmaf(vx[t].x, vy[t].x, vx[t].y * vy[t].y), fmaf(vx[t].x, vy[t].y, -vx[t].y * vy[t].x));
                if (ok) st_stream(Wrow + nn, w);
            }
            continue;
        }
        // vx <- a + i b, vy <- c, zero outside the record (the index is made opaque again before every use, so that no stage's bins,
        // masks or offsets are computed ahead and held across a transform)
        asm volatile("" : "+v"(tq));
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int64_t nn = n0 - a.M + tq + C::T * t;
            const float m = nn >= 0 && nn < N ? inv_s : 0.f;
            const cf wx = vx[t], wy = vy[t];
            vx[t] = mk(m * cnorm(wx), m * cnorm(wy));
            vy[t] = mk(m * fmaf(wx.x, wy.x, wx.y * wy.y), m * fmaf(wx.x, wy.y, -wx.y * wy.x));
        }
        __builtin_amdgcn_sched_barrier(0);
        wct_smooth(xf, vx, lds, tid, n, step);
        __builtin_amdgcn_sched_barrier(0);
        wct_smooth(xf, vy, lds, tid, n, step);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(tq));
        float4 *__restrict__ Trow = a.T + ((int64_t)row * a.S + s) * N;
#pragma unroll
        for (int t = 0; t < C::R; ++t) {
            const int j = tq + C::T * t;
            const int64_t nn = n0 - a.M + j;
            const bool ok = act && j >= a.M && j < a.M + a.hop && nn < N;
            if (ok) st_stream(Trow + nn, make_float4(vx[t].x, vx[t].y, vy[t].x, vy[t].y));
        }
    }
}

__device__ __forceinline__ void wct_finish(float4 acc, int64_t o, float *__restrict__ R2, float *__restrict__ phase, float *__restrict__ A,
                                           float *__restrict__ B, cf *__restrict__ C) {
    const float den = acc.x * acc.y;
    const bool ok = den != 0.f;
    st_stream(R2 + o, ok ? fmaf(acc.z, acc.z, acc.w * acc.w) / den : 0.f);
    st_stream(phase + o, ok ? atan2f(acc.w, acc.z) : 0.f);
    if (A != nullptr) {
        st_stream(A + o, acc.x);
        st_stream(B + o, acc.y);
        st_stream(C + o, mk(acc.z, acc.w));
    }
}

// k_wct_scale<NT>, ntaps <= NT: one thread per sample walks the scale rows in ascending order and keeps the last NT rows of its column
// in registers, so that every element of T is read from memory once; coalesced along n.  The walk is unrolled NT rows at a time, which
// makes every ring slot a register known at compile time: row r lives in slot (r - hi) mod NT, hi = ntaps - 1 - ntaps / 2 the rows the
// window reaches ahead, and with the taps aligned to the END of an NT-long window (position jj = NT - ntaps + j) the row of position jj
// for output s = base + u is in slot (u + jj + 1) mod NT.  Positions before the first tap are skipped (a uniform branch), rows outside
// the scale set are zeros in the ring: adding w x 0 changes nothing, so the sum is the one over the rows inside, in ascending order.
template <int NT> static __global__ __launch_bounds__(256) void k_wct_scale(const float4 *__restrict__ T, const float *__restrict__ taps,
                                                                           int ntaps, int S, int64_t N, float *__restrict__ R2,
                                                                           float *__restrict__ phase, float *__restrict__ A,
                                                                           float *__restrict__ B, cf *__restrict__ C) {
    const int64_t row = blockIdx.y, base = row * S;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;                                                    // (no barrier below)
    const int first = NT - ntaps, hi = ntaps - 1 - ntaps / 2;
    float w[NT];
#pragma unroll
    for (int jj = 0; jj < NT; ++jj) w[jj] = jj >= first ? taps[NT - 1 - jj] : 0.f;     // row position j takes taps[ntaps - 1 - j]
    float4 ring[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) ring[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *__restrict__ Tc = T + base * N + i;
    // the rows 0 .. hi - 1 come before the first output; row r goes to slot (r - hi) mod NT = NT - hi + r
    for (int r = 0; r < hi && r < S; ++r) {
        const float4 v = Tc[(int64_t)r * N];
#pragma unroll
        for (int q = 0; q < NT; ++q)
            if (q == NT - hi + r) ring[q] = v;
    }
    for (int sb = 0; sb < S; sb += NT) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int s = sb + u;
            if (s < S) {                                                   // uniform
                const int r = s + hi;
                ring[u] = r < S ? Tc[(int64_t)r * N] : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int jj = 0; jj < NT; ++jj) {
                    if (jj >= first) {                                     // uniform
                        const float4 v = ring[(u + jj + 1) % NT];
                        acc = make_float4(fmaf(w[jj], v.x, acc.x), fmaf(w[jj], v.y, acc.y), fmaf(w[jj], v.z, acc.z), fmaf(w[jj], v.w, acc.w));
                    }
                }
                wct_finish(acc, (base + s) * N + i, R2, phase, A, B, C);
            }
        }
    }
}

// any number of taps: one thread per sample and scale row, the neighbouring rows re-read through the caches
static __global__ __launch_bounds__(256) void k_wct_scale_any(const float4 *__restrict__ T, const float *__restrict__ taps, int ntaps, int S,
                                                              int64_t N, float *__restrict__ R2, float *__restrict__ phase,
                                                              float *__restrict__ A, float *__restrict__ B, cf *__restrict__ C) {
    const int s = blockIdx.y;
    const int64_t row = blockIdx.z, base = row * S;
    const int r_lo = s - ntaps / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < ntaps; ++j) {
            const int r = r_lo + j;
            if (r < 0 || r >= S) continue;
            const float w = taps[ntaps - 1 - j];
            const float4 v = T[(base + r) * N + i];
            acc = make_float4(fmaf(w, v.x, acc.x), fmaf(w, v.y, acc.y), fmaf(w, v.z, acc.z), fmaf(w, v.w, acc.w));
        }
        wct_finish(acc, (base + s) * N + i, R2, phase, A, B, C);
    }
}

int launch_wct_time(LaunchCtx c, const WctArgs &a, int L, const cf *tw, const CwtPlan &pl, int64_t rows) {
    if (a.nframes < 1 || a.S < 1 || a.chunk < 1 || a.M < 0 || a.hop != L - 2 * a.M || a.hop < 1 || rows < 1 || rows > 65535 ||
        pl.nchunks < 1 || pl.nchunks > 65535 || pl.blocks_x < 1 || pl.blocks_x > INT_MAX || (a.T == nullptr) == (a.Wxy == nullptr))
        return -1;
    const XfTables tb{tw, nullptr, nullptr, L};
    const dim3 grid((unsigned)pl.blocks_x, (unsigned)pl.nchunks, (unsigned)rows);
    const size_t lds = wct_lds_bytes(L);
#define L_(XW)                                                                                        \
    {                                                                                                 \
        if (lds_raise<k_wct_time<XT, XW>>(lds)) return -1;                                            \
        hipLaunchKernelGGL((k_wct_time<XT, XW>), grid, dim3(XT::C::WG), lds, c.stream, a, tb);        \
    }
    return for_pow2<SP_CWT_MIN_L, SP_CWT_MAX_L>(L, [&](auto x) {
        using XT = typename decltype(x)::type;
        if (lds != sizeof(cf) * (size_t)XT::C::FPW * ((size_t)XT::C::LDS_PER + (wct_stash(XT::L) ? (size_t)XT::L : 0))) return -1;
        if (a.T == nullptr) L_(true) else L_(false)
        return 0;
    });
#undef L_
}

int launch_wct_scale(LaunchCtx c, const float4 *T, const float *taps, int ntaps, int S, int64_t N, int64_t rows, float *R2, float *phase,
                     float *A, float *B, cf *C) {
    if (S < 1 || S > 65535 || N < 1 || rows < 1 || rows > 65535 || ntaps < 1 || !T || !taps || !R2 || !phase ||
        ((A != nullptr) != (B != nullptr)) || ((A != nullptr) != (C != nullptr)))
        return -1;
    const int64_t bx = (N + 255) / 256;
    if (ntaps <= 16) {                                                     // (a ring of 32 rows does not stay in registers)
        if (bx > INT_MAX) return -1;
        const dim3 grid((unsigned)bx, (unsigned)rows);
#define R_(NTv) hipLaunchKernelGGL(k_wct_scale<NTv>, grid, dim3(256), 0, c.stream, T, taps, ntaps, S, N, R2, phase, A, B, C)
        if (ntaps <= 8) R_(8);
        else R_(16);
#undef R_
    } else {
        const int64_t cap = (int64_t)c.ncu * 16;
        hipLaunchKernelGGL(k_wct_scale_any, dim3((unsigned)(bx > cap ? cap : bx), (unsigned)S, (unsigned)rows), dim3(256), 0, c.stream, T,
                           taps, ntaps, S, N, R2, phase, A, B, C);
    }
    return 0;
}

}   // namespace sp
