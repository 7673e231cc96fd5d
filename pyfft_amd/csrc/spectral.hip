// spectral.hip -- C ABI (include/spectral.h) over the gfx950 kernels (kernels.h via launch.h).
#include "../../include/spectral.h"
#include "../../include/spectral_ext.h"
#include "../../include/spectral_tfr.h"
#include "../../include/spectral_quad.h"
#include "../../include/spectral_cyclo.h"
#include "../../include/spectral_uneven.h"
#include "../../include/spectral_wbic.h"
#include "../../include/spectral_fam.h"
#include "../../include/spectral_nufft.h"
#include "../../include/spectral_nufft2.h"
#include "../../include/spectral_ar.h"
#include "../../include/spectral_sub.h"
#include "../../include/spectral_dwt.h"
#include "../../include/spectral_array.h"
#include "../../include/spectral_mimo.h"
#include "launch.h"
#include "stage.h"
#include "table_cache.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and enums only: the functions are resolved with dlsym (no link-time dependency)
#include <dlfcn.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace sp;

#define SP_VERSION 110
#define SP_MAX_WG_FFT 8192
#define SP_MAX_BIG_LOG2 26          /* longest multi-pass power-of-two transform: 2^26 points (512 MiB per buffer) */

namespace {

thread_local std::string g_err;

int fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LAUNCHCHK(expr)                                                                               \
    do {                                                                                              \
        if ((expr) != 0) return fail("%s: no kernel instantiated for this transform length (%s:%d)", #expr, __FILE__, __LINE__); \
        HIPCHK(hipGetLastError());                                                                    \
    } while (0)

struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + (bytes >> 3) + 4096;
        if (hipMalloc(&p, want) != hipSuccess) return fail("hipMalloc(%zu) failed", want);
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct BlueTab {
    cf *chirp, *bf;
    int L;
};

struct Ctx {
    bool ready = false;
    int device = 0;
    int ncu = 256;
    hipStream_t stream = nullptr;
    std::map<int64_t, cf *> twiddles;   // L -> exp(-2 pi i m/L)
    std::map<int64_t, BlueTab> blue;    // n -> Bluestein tables
    Scratch in0, in1, out0, work, small, trends, onepass, ticket, epi;
    Scratch pend_trend;                       // trend record a pending sp_welch_accum keeps until sp_welch_finish
    Scratch pend_x;                           // ... and the staged record of a host-memory sp_welch_accum: sp_welch_finish reads its edge blocks
    Scratch bigA, bigB, bigT, blueA, blueB, longrec;   // long (multi-kernel) paths
    Scratch sosY, sosZ;                            // cascaded sections: sosfiltfilt's forward output, staged zi / zf
    Scratch bsIn, bsS, bsP, bsA;                    // bispectrum: staged inputs, spectra, fp32 partials, float64 sums
    Scratch mtS;                                    // multitaper: the per-taper cross spectra behind the weighted one
    Scratch wbW, wbP, wbA;                          // wavelet bispectrum: the transforms of a pass, its fp32 partials, the float64 cell sums
    Scratch famZ, famA;                             // FFT accumulation: the bin-major frames of a pass, the float64 sums across passes
    Scratch nuRec, nuGrid;                          // type-1 NUFFT: the prepared samples, tile lists and shifts of a call; the fine grids of a pass
    Scratch subPart, subMat;                        // covariance matrices: the per-tile partial rows of a pass; the matrices of a pass of fits
    Scratch dwtS;                                   // discrete wavelet transforms: the approximations between the levels of a pass (tile form)
    Scratch arPart, arSmall;                        // autoregressive fits: the per-tile partial lags of a pass; the flag, the tiles' sums and the means
    Scratch cmS, cmT, cmG, cmH, cmO;               // CSD matrix: spectra, bin-major spectra, float64 accumulator, packed-spectra sums, one-pass means state
    std::map<int64_t, BigTw> bigtw;           // N -> two-level twiddle tables of the multi-pass FFT
    std::map<int64_t, BlueTab> blue_big;      // n -> chirp[n], FFT_L(chirp*) (unscaled) for multi-pass Bluestein
    std::mutex mu;
    bool profile = false, prof_valid = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_sw = nullptr;
    const char *last_kernel = "";
} g;

LaunchCtx lc() { return LaunchCtx{g.stream, g.ncu}; }

// pending one-pass Welch accumulation (sp_welch_accum -> sp_welch_finish)
struct Pending {
    bool valid = false;
    const void *xd = nullptr;
    bool cplx = false;
    int64_t nsig = 0, nframes = 0, nmean = 0;
    int nfft = 0, hop = 0;
    Xf xf;
    const float *win_d = nullptr;
    const cf *Wf = nullptr;
    OnePass st;
    float *trend_f = nullptr;
    cf *cw = nullptr;
    double *sum_d = nullptr;
    double *state = nullptr;     // generic shapes (k_welch_opx): the exported state, finished by k_op_apply
} g_pend;

struct ProfScope {   // brackets one kernel launch with HIP events on its stream (default: the launch stream) when profiling is on
    bool on;
    hipStream_t st;
    explicit ProfScope(hipStream_t s = nullptr) : on(g.profile), st(s ? s : g.stream) {
        if (on) (void)hipEventRecord(g.ev0, st);
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(g.ev1, st);
            g.prof_valid = true;
        }
    }
};

int ensure_init() {
    if (g.ready) return 0;
    return sp_init(-1);
}

bool is_pow2(int64_t n) { return n >= 1 && (n & (n - 1)) == 0; }
int64_t next_pow2(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

int get_twiddles(int64_t n, const cf **out) {
    auto it = g.twiddles.find(n);
    if (it != g.twiddles.end()) {
        *out = it->second;
        return 0;
    }
    std::vector<cf> h((size_t)n);
    for (int64_t m = 0; m < n; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)n;
        h[(size_t)m] = make_float2((float)cos(a), (float)sin(a));
    }
    cf *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, sizeof(cf) * (size_t)n));
    HIPCHK(hipMemcpy(d, h.data(), sizeof(cf) * (size_t)n, hipMemcpyHostToDevice));
    g.twiddles[n] = d;
    *out = d;
    return 0;
}

// transform plan for length n handled inside one workgroup
int get_xf(int64_t n, Xf *xf) {
    if (n < 2) return fail("transform length %lld too short", (long long)n);
    if (is_pow2(n) && n <= SP_MAX_WG_FFT) {
        xf->L = (int)n;
        xf->blue = false;
        xf->tb.n = (int)n;
        xf->tb.chirp = xf->tb.bf = nullptr;
        return get_twiddles(n, &xf->tb.tw);
    }
    int64_t L = next_pow2(2 * n - 1);
    if (L < 16) L = 16;
    if (L > SP_MAX_WG_FFT)
        return fail("transform length %lld not supported yet (powers of two up to %d, other lengths up to %d)",
                    (long long)n, SP_MAX_WG_FFT, SP_MAX_WG_FFT / 2);
    xf->L = (int)L;
    xf->blue = true;
    xf->tb.n = (int)n;
    if (get_twiddles(L, &xf->tb.tw)) return -1;
    auto it = g.blue.find(n);
    if (it == g.blue.end()) {
        // chirp[m] = exp(-i pi m^2/n); bf = FFT_L(wrapped conj(chirp)) / L   (angles reduced mod 2n in integers)
        std::vector<cf> ch((size_t)n), bw((size_t)L, make_float2(0.f, 0.f));
        for (int64_t m = 0; m < n; ++m) {
            const int64_t q = (m * m) % (2 * n);
            const double a = M_PI * (double)q / (double)n;
            ch[(size_t)m] = make_float2((float)cos(a), (float)-sin(a));
            const cf b = make_float2((float)(cos(a) / (double)L), (float)(sin(a) / (double)L));
            bw[(size_t)m] = b;
            if (m > 0) bw[(size_t)(L - m)] = b;
        }
        BlueTab t;
        t.L = (int)L;
        HIPCHK(hipMalloc((void **)&t.chirp, sizeof(cf) * (size_t)n));
        HIPCHK(hipMalloc((void **)&t.bf, sizeof(cf) * (size_t)L));
        HIPCHK(hipMemcpy(t.chirp, ch.data(), sizeof(cf) * (size_t)n, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.bf, bw.data(), sizeof(cf) * (size_t)L, hipMemcpyHostToDevice));
        Xf p2;
        if (get_xf(L, &p2)) return -1;
        LAUNCHCHK(launch_fft_c2c(lc(), t.bf, t.bf, 1, 0, p2));
        HIPCHK(hipStreamSynchronize(g.stream));
        g.blue[n] = t;
        it = g.blue.find(n);
    }
    xf->tb.chirp = it->second.chirp;
    xf->tb.bf = it->second.bf;
    return 0;
}

// Small host tables (windows, filter spectra) live in a content-keyed device cache: a table is uploaded
// once into its own allocation and never overwritten, so asynchronous (mem=1) callers can reuse the
// host buffer immediately and repeated calls with the same window cost no copy and no synchronisation.
// (bookkeeping and eviction policy: table_cache.h.)  A miss on a full cache drops the least recently used entry that
// the current API call has not touched and that a pending sp_welch_accum does not hold; the device is synchronised
// before the entry is freed, because asynchronous (mem=1) work of an earlier call may still read it.
TableCache g_tables;

// sp_last_passes: [0] the passes of the current call's outermost frame-chunk loop, [1] the most slice passes one
// dev_fft_any / sp_czt loop made inside it, [2] the passes over the cycle-frequency list of sp_cyclic, [3] the passes over the
// frequency list of sp_lomb / sp_lomb_sums, [4] the most launches the row groups of one such pass were dealt to, [5] the passes over the
// blocks of sp_fam, [6] the passes over the rows of sp_nufft1 / sp_lomb_sums_grid / sp_nufft2, [7] the passes over
// the segments of sp_burg / sp_yule, [8] the passes over the segments of sp_covmat / sp_ar_ls, [9] the passes over the
// rows of the tile form of sp_dwt / sp_idwt / sp_modwt / sp_imodwt and their single-level entries.  All are zeroed
// where a call begins (ApiLock), so that a test can assert that the shape it chose really walks a loop past its first pass.
int g_passes[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline void note_slices(int64_t n) {
    if (n > g_passes[1]) g_passes[1] = (int)n;
}
// a test hook that caps a loop's budget: unset or <= 0 leaves `v` as it is
inline int64_t hook_cap(const char *name, int64_t v) {
    const int64_t h = env_int(name, 0);
    return h > 0 && h < v ? h : v;
}

// every C-ABI entry point that touches device state holds this for its whole body: the library lock, and the start of
// a new "current call" for the table cache
struct ApiLock {
    std::lock_guard<std::mutex> lk;
    ApiLock() : lk(g.mu) {
        g_tables.begin_call();
        g_passes[0] = g_passes[1] = g_passes[2] = g_passes[3] = g_passes[4] = g_passes[5] = g_passes[6] = g_passes[7] = g_passes[8] = g_passes[9] = 0;
    }
};

// Staging of one call's host-memory (mem = 0) arguments: the one place that grows the scratch buffers, copies inputs in
// and results back (layout rules: stage.h).  in / out / inout name a scratch, the caller's pointer and its size and take the
// address of the pointer the kernels will use: with mem = 1 that is the caller's own pointer at once and nothing else
// happens.  With mem = 0, commit() sizes every scratch named since the last commit once, sets the pointers and enqueues the
// copies in on g.stream; finish(), at every successful return, enqueues the copies back in registration order and
// synchronises.  An error return in between copies nothing back.
struct Stage {
    const bool host;
    int done = 0;       // pieces already committed
    StagePlan plan;
    explicit Stage(int mem) : host(!mem) {}
    template <class H, class D> void in(Scratch &s, const H *h, size_t bytes, const D **dev) {
        *dev = (const D *)h;
        if (host) plan.add(&s, h, nullptr, bytes, dev);
    }
    template <class H, class D> void out(Scratch &s, H *h, size_t bytes, D **dev) {
        *dev = (D *)h;
        if (host) plan.add(&s, nullptr, h, bytes, dev);
    }
    // one piece that is copied in from `h_in` and back to `h_out`: the kernels read *din and write *dout, the same staged
    // address for host arrays (the work is done in place there), the caller's two pointers otherwise
    template <class H, class D> void inout(Scratch &s, const H *h_in, H *h_out, size_t bytes, const D **din, D **dout) {
        *din = (const D *)h_in;
        *dout = (D *)h_out;
        if (host) plan.add(&s, h_in, h_out, bytes, dout, din);
    }
    // an output of `count` rows of `len` elements of `el` bytes, `ld` apart.  Rows further apart than they are long leave room
    // between them that is the caller's: then the piece is staged in both directions, so that the room comes back as it was.
    // `both` states that choice where a site makes another one
    template <class H, class D> void rows(Scratch &s, H *h, size_t el, int64_t count, int64_t ld, int64_t len, D **dev, bool both) {
        *dev = (D *)h;
        if (host) plan.add(&s, both ? h : nullptr, h, el * (size_t)((count - 1) * ld + len), dev);
    }
    template <class H, class D> void rows(Scratch &s, H *h, size_t el, int64_t count, int64_t ld, int64_t len, D **dev) {
        rows(s, h, el, count, ld, len, dev, ld > len);
    }
    int commit() {
        if (!host) return 0;
        if (plan.err) return fail("staging: %s", plan.err);
        for (int a = 0; a < plan.nareas; ++a)
            if (!plan.area[a].sealed) {
                if (((Scratch *)plan.area[a].key)->ensure(plan.area[a].total)) return -1;
                plan.seal(a);
            }
        for (; done < plan.npieces; ++done) {
            const StagePlan::Piece &p = plan.piece[done];
            void *d = (char *)((Scratch *)plan.area[p.area].key)->p + p.off;
            memcpy(p.slot, &d, sizeof d);
            if (p.slot2) memcpy(p.slot2, &d, sizeof d);
            if (p.from && p.bytes) HIPCHK(hipMemcpyAsync(d, p.from, p.bytes, hipMemcpyHostToDevice, g.stream));
        }
        return 0;
    }
    int finish() {
        if (!host) return 0;
        for (int i = plan.next_back(-1); i >= 0; i = plan.next_back(i)) {
            const StagePlan::Piece &p = plan.piece[i];
            const void *d = (const char *)((Scratch *)plan.area[p.area].key)->p + p.off;
            if (p.bytes) HIPCHK(hipMemcpyAsync(p.to, d, p.bytes, hipMemcpyDeviceToHost, g.stream));
        }
        HIPCHK(hipStreamSynchronize(g.stream));
        return 0;
    }
};

// content hash of a host table (FNV-1a style, 8 bytes per step: a 4096-point window hashes in ~1 us)
uint64_t fnv1a(const void *p, size_t n, uint64_t h) {
    const unsigned char *b = (const unsigned char *)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, b + i, 8);
        h ^= w;
        h *= 1099511628211ull;
        h ^= h >> 29;
    }
    for (; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

// content hash of a WINDOW, memoised by comparing with a kept copy: a streamed Welch step asked for the same window's hash four
// times (window table, its spectrum, lobe test, COLA test: 3-5 us per pass over 16 KiB, half of the call's host time); a memcmp
// of 16 KiB is 0.2 us.  Called under the library lock.
uint64_t window_key(const float *win, int n) {
    struct Memo {
        std::vector<float> copy;
        uint64_t h = 0;
    };
    static Memo memo[4];
    static int next = 0;
    const size_t bytes = sizeof(float) * (size_t)n;
    for (Memo &m : memo)
        if ((int)m.copy.size() == n && memcmp(m.copy.data(), win, bytes) == 0) return m.h;
    Memo &m = memo[next];
    next = (next + 1) & 3;
    m.copy.assign(win, win + n);
    m.h = fnv1a(win, bytes, 1469598103934665603ull);
    return m.h;
}
static uint64_t mix_key(uint64_t h, uint64_t a, uint64_t b) {
    h ^= a * 0x9E3779B97F4A7C15ull;
    h *= 1099511628211ull;
    h ^= h >> 29;
    h ^= b;
    h *= 1099511628211ull;
    return h ^ (h >> 32);
}

void tables_release() {
    for (auto &kv : g_tables.map) (void)hipFree(kv.second.dev);
    g_tables.map.clear();
}

// device table keyed by the CONTENT of `key_data`.  upload != null: a miss uploads `bytes` from it; upload == null: a
// miss only allocates `bytes` and reports fresh = true (the caller fills the table, e.g. FFT(window) keyed by the window)
int get_table_keyed(uint64_t kind, const void *key_data, size_t key_bytes, const void *upload, size_t bytes, void **dev,
                    bool *fresh) {
    // (kinds 1 and 3 are keyed by a window's float32 values: the memoised hash)
    const uint64_t key = ((kind == 1 || kind == 3) && key_bytes % sizeof(float) == 0 && key_bytes > 0)
                             ? mix_key(window_key((const float *)key_data, (int)(key_bytes / sizeof(float))), kind, bytes)
                             : fnv1a(key_data, key_bytes, 1469598103934665603ull ^ (kind * 0x9E3779B97F4A7C15ull) ^ bytes);
    if (TableEntry *e = g_tables.find(key, bytes)) {
        *dev = e->dev;
        if (fresh) *fresh = false;
        return 0;
    }
    if (g_tables.full()) {
        const void *pinned[2] = {g_pend.valid ? (const void *)g_pend.win_d : nullptr, g_pend.valid ? (const void *)g_pend.Wf : nullptr};
        uint64_t victim;
        bool synced = false;
        while (g_tables.full() && g_tables.pick_victim(pinned, 2, &victim)) {
            if (!synced) HIPCHK(hipDeviceSynchronize());
            synced = true;
            (void)hipFree(g_tables.erase(victim));
        }   // nothing evictable: every entry is in use by this call -- grow past the cap rather than free live memory
    }
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes));
    if (upload) HIPCHK(hipMemcpy(d, upload, bytes, hipMemcpyHostToDevice));
    if (void *old = g_tables.insert(key, d, bytes)) {
        HIPCHK(hipDeviceSynchronize());
        (void)hipFree(old);
    }
    *dev = d;
    if (fresh) *fresh = true;
    return 0;
}
int get_table(uint64_t kind, const void *host, size_t bytes, void **dev, bool *fresh) {
    return get_table_keyed(kind, host, bytes, host, bytes, dev, fresh);
}

__global__ void k_set4(float *dst, float a, float b, float c, float d) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        dst[0] = a;
        dst[1] = b;
        dst[2] = c;
        dst[3] = d;
    }
}

// dst[c] = trend of src[c] re-based to start at sample `offset`: (m + s*offset, s)
__global__ void k_trend_shift(const float *src, float *dst, int count, double offset) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < count) {
        dst[4 * c + 0] = (float)((double)src[4 * c + 0] + (double)src[4 * c + 2] * offset);
        dst[4 * c + 1] = (float)((double)src[4 * c + 1] + (double)src[4 * c + 3] * offset);
        dst[4 * c + 2] = src[4 * c + 2];
        dst[4 * c + 3] = src[4 * c + 3];
    }
}

__global__ void k_xcorr_norm(const double *mom1, const double *mom2, int64_t n, double *out /*[4]*/) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double m1 = mom1[0], m2 = mom2[0];
        const double v1 = mom1[2] / (double)n - m1 * m1, v2 = mom2[2] / (double)n - m2 * m2;
        out[0] = m1;
        out[1] = m2;
        out[2] = 1.0 / ((double)n * sqrt(v1 > 0 ? v1 : 0) * sqrt(v2 > 0 ? v2 : 0));
        out[3] = 0;
    }
}

// device block: nsig trend records (4 floats each) followed by 8 doubles per signal
struct TrendBuf {
    float *f;
    double *d;
};
int get_trendbuf(int nsig, TrendBuf *tb) {
    const size_t fbytes = ((sizeof(float) * 4 * (size_t)nsig) + 63) & ~(size_t)63;
    if (g.trends.ensure(fbytes + sizeof(double) * 8 * (size_t)nsig + 64)) return -1;
    tb->f = (float *)g.trends.p;
    tb->d = (double *)((char *)g.trends.p + fbytes);
    return 0;
}
double *moments_scratch() {
    if (g.small.ensure(sizeof(double) * 8 * 4096 + 256)) return nullptr;
    return (double *)g.small.p;
}

// fill trend record `idx` for signal x: detrend 0 -> explicit (re,im), 1 -> mean, 2 -> LS line
int set_trend(const TrendBuf &tb, int idx, const void *x, bool cplx, int64_t n, int detrend, double re, double im) {
    if (detrend == 0) {
        hipLaunchKernelGGL(k_set4, dim3(1), dim3(64), 0, g.stream, tb.f + 4 * idx, (float)re, (float)im, 0.f, 0.f);
        HIPCHK(hipGetLastError());
        return 0;
    }
    double *scr = moments_scratch();
    if (!scr) return -1;
    LAUNCHCHK(launch_moments(lc(), x, cplx, n, detrend, scr, tb.d + 8 * idx, tb.f + 4 * idx));
    return 0;
}

int check_frames(const char *who, int64_t nsig, int nfft, int hop, int64_t nframes) {
    if (nfft < 2 || hop < 1 || nframes < 1) return fail("%s: bad nfft/hop/nframes", who);
    if ((nframes - 1) * (int64_t)hop + nfft > nsig)
        return fail("%s: %lld frames of %d with hop %d need %lld samples, signal has %lld", who, (long long)nframes, nfft,
                    hop, (long long)((nframes - 1) * (int64_t)hop + nfft), (long long)nsig);
    return 0;
}

int nbins_host(int n, int sided) {
    if (sided == SP_SIDED_ONE) return (n & 1) ? (n + 1) / 2 : n / 2;
    if (sided == SP_SIDED_HALF) return n / 2 + 1;
    return n;
}


// ---- transforms longer than one workgroup ---------------------------------------------------------
bool wg_capable(int64_t n) {
    if (n < 2) return false;
    if (is_pow2(n)) return n <= SP_MAX_WG_FFT;
    int64_t L = next_pow2(2 * n - 1);
    return (L < 16 ? 16 : L) <= SP_MAX_WG_FFT;
}

int get_bigtw(int64_t N, BigTw *bt) {
    auto it = g.bigtw.find(N);
    if (it != g.bigtw.end()) {
        *bt = it->second;
        return 0;
    }
    int lg = 0;
    while (((int64_t)1 << lg) < N) ++lg;
    const int lb = lg < 13 ? lg : 13;
    const int64_t nlo = (int64_t)1 << lb, nhi = N >> lb;
    std::vector<cf> lo((size_t)nlo), hi((size_t)nhi);
    for (int64_t j = 0; j < nlo; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)N;
        lo[(size_t)j] = make_float2((float)cos(a), (float)sin(a));
    }
    for (int64_t j = 0; j < nhi; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)nhi;      // j * 2^lb / N
        hi[(size_t)j] = make_float2((float)cos(a), (float)sin(a));
    }
    cf *dlo = nullptr, *dhi = nullptr;
    HIPCHK(hipMalloc((void **)&dlo, sizeof(cf) * (size_t)nlo));
    HIPCHK(hipMalloc((void **)&dhi, sizeof(cf) * (size_t)nhi));
    HIPCHK(hipMemcpy(dlo, lo.data(), sizeof(cf) * (size_t)nlo, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dhi, hi.data(), sizeof(cf) * (size_t)nhi, hipMemcpyHostToDevice));
    bt->hi = dhi;
    bt->lo = dlo;
    bt->lb = lb;
    bt->mod = 0;
    g.bigtw[N] = *bt;
    return 0;
}

// N = 2^k, 2^14 <= N <= 2^26:  x viewed as [N1][N2]; transpose, N2 row FFTs of N1 (+ twiddle W_N^{n2 k1}),
// transpose, N1 row FFTs of N2, transpose back to natural order.  5 passes over the data (80 B / point).
// three-pass form available for N (then hmask may be fused into the first pass of an inverse transform)
bool big_three_pass(int64_t N) {
    return is_pow2(N) && N >= ((int64_t)1 << 20) && !env_flag("SP_BIGFFT_5PASS");
}

// fused first-pass input / last-pass output of ONE three-pass transform (see ColsIn / RowsOut in kernels.h)
struct BigFuse {
    ColsIn ci = ColsIn{0, nullptr, nullptr, nullptr, 0};
    RowsOut ro = RowsOut{nullptr, 0, 0, nullptr};
};
int dev_fft_big_pow2(const cf *in, cf *out, int64_t N, int inverse, int hmask = 0, int64_t batch = 1, const BigFuse *fz = nullptr) {
    int lg = 0;
    while (((int64_t)1 << lg) < N) ++lg;
    if (((int64_t)1 << lg) != N || lg > SP_MAX_BIG_LOG2) return fail("internal: dev_fft_big_pow2(%lld)", (long long)N);
    if (batch < 1) return fail("internal: dev_fft_big_pow2 batch");
    const int64_t N1 = (int64_t)1 << ((lg + 1) / 2), N2 = N / N1;
    Xf x1, x2;
    if (get_xf(N1, &x1) || get_xf(N2, &x2)) return -1;
    BigTw bt;
    if (get_bigtw(N, &bt)) return -1;
    const float sc = inverse ? (float)(1.0 / (double)N) : 1.f;
    if ((hmask || fz) && !big_three_pass(N)) return fail("internal: fused Hilbert mask / pack need the three-pass transform");
    if (fz && batch != 1) return fail("internal: fused long transform is a single transform");
    if (big_three_pass(N)) {
        // three passes over whole lines, N = A B C (kernels.h: k_fft_cols / k_fft_rows_rev); a batch runs row by row
        // (each pass already fills the chip at these lengths)
        if (g.bigT.ensure(sizeof(cf) * (size_t)N)) return -1;
        cf *tmp = (cf *)g.bigT.p;
        // the two COLUMN passes want short transforms: a workgroup then owns many adjacent columns and every access is a
        // whole 128-byte line or more (256 points: 16 columns; 512 points would be 8 columns = 64-byte segments, measured
        // 1.4 TB/s for that pass at 2^25 points) -- A, B <= 256, the rest goes to the contiguous row pass
        int la_ = (lg + 2) / 3;
        if (la_ > 8) la_ = 8;
        int lb_ = (lg - la_ + 1) / 2;
        if (lb_ > 8) lb_ = 8;
        const int lc_ = lg - la_ - lb_;
        const int64_t A = (int64_t)1 << la_, B = (int64_t)1 << lb_, C = (int64_t)1 << lc_;
        Xf xa, xb, xc;
        if (get_xf(A, &xa) || get_xf(B, &xb) || get_xf(C, &xc)) return -1;
        for (int64_t b = 0; b < batch; ++b) {
            if (fz) {
                LAUNCHCHK(launch_fft_cols(lc(), in, tmp, B * C, 1, B * C, 0, 1, inverse, xa, bt, hmask ? N : 0, fz->ci));
                LAUNCHCHK(launch_fft_cols(lc(), tmp, tmp, C, A, C, B * C, A, 0, xb, bt));
                LAUNCHCHK(launch_fft_rows_rev(lc(), tmp, out, A, B, inverse, sc, xc, fz->ro));
                continue;
            }
            LAUNCHCHK(launch_fft_cols(lc(), in + b * N, tmp, B * C, 1, B * C, 0, 1, inverse, xa, bt, hmask ? N : 0));
            LAUNCHCHK(launch_fft_cols(lc(), tmp, tmp, C, A, C, B * C, A, 0, xb, bt));
            LAUNCHCHK(launch_fft_rows_rev(lc(), tmp, out + b * N, A, B, inverse, sc, xc));
        }
        return 0;
    }
    // N = 2^k, 2^14 <= N < 2^20:  x viewed as [N1][N2]; transpose, N2 row FFTs of N1 (+ twiddle W_N^{n2 k1}), transpose,
    // N1 row FFTs of N2, transpose back to natural order: 5 passes over the data (80 B / point).  The whole batch of
    // transforms goes through each of the five launches together (rows numbered modulo N2 for the twiddle).
    if (batch > 65535) return fail("internal: dev_fft_big_pow2 batch %lld", (long long)batch);
    if (g.bigT.ensure(sizeof(cf) * (size_t)N * (size_t)batch)) return -1;
    cf *tmp = (cf *)g.bigT.p;
    BigTw btb = bt;
    btb.mod = N2;
    if (in != out) {
        LAUNCHCHK(launch_transpose_c(lc(), in, out, N1, N2, inverse, 1.f, batch));        // out[n2][n1]
        LAUNCHCHK(launch_fft_c2c(lc(), out, out, N2 * batch, 0, x1, btb));                 // A[n2][k1] W^{n2 k1}
        LAUNCHCHK(launch_transpose_c(lc(), out, tmp, N2, N1, 0, 1.f, batch));              // tmp[k1][n2]
        LAUNCHCHK(launch_fft_c2c(lc(), tmp, tmp, N1 * batch, 0, x2));                      // B[k1][k2]
        LAUNCHCHK(launch_transpose_c(lc(), tmp, out, N1, N2, inverse, sc, batch));         // out[k2][k1]
    } else {
        if (g.blueB.ensure(sizeof(cf) * (size_t)N * (size_t)batch)) return -1;     // second temporary for the in-place form
        cf *t2 = (cf *)g.blueB.p;
        LAUNCHCHK(launch_transpose_c(lc(), in, tmp, N1, N2, inverse, 1.f, batch));
        LAUNCHCHK(launch_fft_c2c(lc(), tmp, tmp, N2 * batch, 0, x1, btb));
        LAUNCHCHK(launch_transpose_c(lc(), tmp, t2, N2, N1, 0, 1.f, batch));
        LAUNCHCHK(launch_fft_c2c(lc(), t2, t2, N1 * batch, 0, x2));
        LAUNCHCHK(launch_transpose_c(lc(), t2, out, N1, N2, inverse, sc, batch));
    }
    return 0;
}

int get_blue_big(int64_t n, BlueTab *t) {
    auto it = g.blue_big.find(n);
    if (it != g.blue_big.end()) {
        *t = it->second;
        return 0;
    }
    const int64_t L = next_pow2(2 * n - 1);
    std::vector<cf> ch((size_t)n), bw((size_t)L, make_float2(0.f, 0.f));
    for (int64_t m = 0; m < n; ++m) {
        const int64_t q = (int64_t)(((__int128)m * m) % (2 * n));
        const double a = M_PI * (double)q / (double)n;
        const float c = (float)cos(a), sn = (float)sin(a);
        ch[(size_t)m] = make_float2(c, -sn);
        bw[(size_t)m] = make_float2(c, sn);
        if (m > 0) bw[(size_t)(L - m)] = make_float2(c, sn);
    }
    BlueTab nt;
    nt.L = 0;
    HIPCHK(hipMalloc((void **)&nt.chirp, sizeof(cf) * (size_t)n));
    HIPCHK(hipMalloc((void **)&nt.bf, sizeof(cf) * (size_t)L));
    HIPCHK(hipMemcpy(nt.chirp, ch.data(), sizeof(cf) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(nt.bf, bw.data(), sizeof(cf) * (size_t)L, hipMemcpyHostToDevice));
    if (dev_fft_big_pow2(nt.bf, nt.bf, L, 0)) return -1;
    HIPCHK(hipStreamSynchronize(g.stream));
    g.blue_big[n] = nt;
    *t = nt;
    return 0;
}

// any length, device pointers.  in == out allowed.  Batches of long transforms go through the multi-kernel paths in
// slices of at most SP_LONG_SLICE_BYTES of work buffer (every launch then covers a whole slice).
#define SP_LONG_SLICE_BYTES ((size_t)256 << 20)
int dev_fft_any(const cf *in, cf *out, int64_t n, int64_t batch, int inverse) {
    if (n == 1) {
        if (in != out) HIPCHK(hipMemcpyAsync(out, in, sizeof(cf) * (size_t)batch, hipMemcpyDeviceToDevice, g.stream));
        return 0;
    }
    if (wg_capable(n)) {
        Xf xf;
        if (get_xf(n, &xf)) return -1;
        LAUNCHCHK(launch_fft_c2c(lc(), in, out, batch, inverse, xf));
        return 0;
    }
    const int64_t L = is_pow2(n) ? n : next_pow2(2 * n - 1);
    if (L > ((int64_t)1 << SP_MAX_BIG_LOG2))
        return fail("transform length %lld needs a %lld-point multi-pass transform; the limit is 2^%d", (long long)n,
                    (long long)L, SP_MAX_BIG_LOG2);
    int64_t slice = (int64_t)(SP_LONG_SLICE_BYTES / (sizeof(cf) * (size_t)L));
    if (slice < 1) slice = 1;
    if (slice > 32768) slice = 32768;
    slice = hook_cap("SP_LONG_SLICE_ROWS", slice);
    note_slices((batch + slice - 1) / slice);
    if (is_pow2(n)) {
        for (int64_t b0 = 0; b0 < batch; b0 += slice) {
            const int64_t m = batch - b0 < slice ? batch - b0 : slice;
            if (dev_fft_big_pow2(in + b0 * n, out + b0 * n, n, inverse, 0, m)) return -1;
        }
        return 0;
    }
    BlueTab bt;
    if (get_blue_big(n, &bt)) return -1;
    if (slice > batch) slice = batch;
    if (g.blueA.ensure(sizeof(cf) * (size_t)L * (size_t)slice)) return -1;
    cf *A = (cf *)g.blueA.p;
    for (int64_t b0 = 0; b0 < batch; b0 += slice) {
        const int64_t m = batch - b0 < slice ? batch - b0 : slice;
        LAUNCHCHK(launch_blue_pre(lc(), in + b0 * n, bt.chirp, n, L, inverse, A, m));
        if (dev_fft_big_pow2(A, A, L, 0, 0, m)) return -1;
        LAUNCHCHK(launch_cmul_vec(lc(), A, bt.bf, L, 0, A, m));
        if (dev_fft_big_pow2(A, A, L, 1, 0, m)) return -1;
        LAUNCHCHK(launch_blue_post(lc(), A, bt.chirp, n, inverse, inverse ? (float)(1.0 / (double)n) : 1.f, out + b0 * n, m, L));
    }
    return 0;
}


// ---- chirp-z transform on an arc of the unit circle (k_czt.hip) ----------------------------------
// Table phases.  step j^2 / 2 must be reduced modulo 1 BEFORE it becomes a floating-point number: at j ~ 2^25 the float64 product has
// no fractional bit left.  The integer tables above reduce m^2 modulo 2n; a real step has no such modulus, so the phase is held in
// wrap-around fixed point: step / 2 mod 1 and start mod 1 as 128-bit binary fractions (a double is a dyadic rational: the conversion
// drops only bits below 2^-128), multiplied by the integers j^2 and j modulo 2^128 -- which IS reduction modulo one turn.  The
// error of a phase is the dropped bits times j^2 (< 2^-128 2^52 = 2^-76 turns for the indices the library accepts, |j| < 2^26) plus
// the rounding of the top 64 bits to a double (2^-54 turns): far below the 1e-9 turns asked for, at every such index.
typedef unsigned __int128 u128;
u128 frac128(double x) {
    const double a = fmod(fabs(x), 1.0);                   // exact
    const double s = ldexp(a, 64), hi = floor(s);          // exact: a < 1 has at most 53 significant bits
    const double lo = floor(ldexp(s - hi, 64));
    const u128 v = ((u128)(uint64_t)hi << 64) | (u128)(uint64_t)lo;
    return x < 0 ? (u128)0 - v : v;
}
// cs[c] = (cos, sin) of e(-start i - step i^2 / 2), i = i0 + c.  Host only: no HIP call.
void czt_chirp_host(int64_t i0, int64_t count, double step, double start, float *cs) {
    const u128 S = frac128(0.5 * step), A = frac128(start);
    for (int64_t c = 0; c < count; ++c) {
        const u128 ui = (u128)(__int128)(i0 + c);
        const u128 t = S * (ui * ui) + A * ui;
        const double turns = ldexp((double)(int64_t)(uint64_t)(t >> 64), -64);       // in [-1/2, 1/2)
        const double a = -2.0 * M_PI * turns;
        cs[2 * c] = (float)cos(a);
        cs[2 * c + 1] = (float)sin(a);
    }
}

#define SP_CZT_MIN_L 512            /* the fused kernels are compiled for L = 512 .. SP_MAX_WG_FFT; shorter shapes are padded up */
#define SP_CZT_CACHE 32
struct CztTab {
    cf *pre, *post, *bf;            // bf: FFT_L(kern) / L for one workgroup transform, unscaled for the multi-pass form
    int64_t L;
};
struct CztKey {
    int64_t n, m;
    uint64_t start, step;           // the doubles' bits
    bool operator<(const CztKey &o) const {
        if (n != o.n) return n < o.n;
        if (m != o.m) return m < o.m;
        if (start != o.start) return start < o.start;
        return step < o.step;
    }
};
std::map<CztKey, CztTab> g_czt;
Scratch g_cztAcc;                   // float64 sums of the long zoom spectra

int64_t czt_len(int64_t n, int64_t m) {
    const int64_t L = next_pow2(n + m - 1);
    return L < SP_CZT_MIN_L ? SP_CZT_MIN_L : L;
}
void czt_release() {
    for (auto &kv : g_czt) {
        (void)hipFree(kv.second.pre);
        (void)hipFree(kv.second.post);
        (void)hipFree(kv.second.bf);
    }
    g_czt.clear();
}
// tables of one (n, m, start, step), cached like g.blue / g.blue_big
int get_czt(int64_t n, int64_t m, double start, double step, CztTab *t) {
    CztKey key{n, m, 0, 0};
    memcpy(&key.start, &start, 8);
    memcpy(&key.step, &step, 8);
    auto it = g_czt.find(key);
    if (it != g_czt.end()) {
        *t = it->second;
        return 0;
    }
    if (g_czt.size() >= SP_CZT_CACHE) {            // asynchronous work of an earlier call may still read a table
        HIPCHK(hipDeviceSynchronize());
        czt_release();
    }
    const int64_t L = czt_len(n, m);
    const bool fused = L <= SP_MAX_WG_FFT;
    std::vector<cf> pre((size_t)n), post((size_t)m), arc((size_t)(n + m - 1)), kern((size_t)L, make_float2(0.f, 0.f));
    czt_chirp_host(0, n, step, start, (float *)pre.data());
    czt_chirp_host(0, m, step, 0.0, (float *)post.data());
    czt_chirp_host(-(n - 1), n + m - 1, step, 0.0, (float *)arc.data());
    const float sc = fused ? 1.f / (float)L : 1.f;                              // a power of two: exact
    for (int64_t i = -(n - 1); i < m; ++i) {
        const cf c = arc[(size_t)(i + n - 1)];
        kern[(size_t)(i < 0 ? i + L : i)] = make_float2(sc * c.x, -sc * c.y);     // e(+step i^2 / 2)
    }
    CztTab nt{nullptr, nullptr, nullptr, L};
    HIPCHK(hipMalloc((void **)&nt.pre, sizeof(cf) * (size_t)n));
    HIPCHK(hipMalloc((void **)&nt.post, sizeof(cf) * (size_t)m));
    HIPCHK(hipMalloc((void **)&nt.bf, sizeof(cf) * (size_t)L));
    HIPCHK(hipMemcpy(nt.pre, pre.data(), sizeof(cf) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(nt.post, post.data(), sizeof(cf) * (size_t)m, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(nt.bf, kern.data(), sizeof(cf) * (size_t)L, hipMemcpyHostToDevice));
    if (fused) {
        Xf p2;
        if (get_xf(L, &p2)) return -1;
        LAUNCHCHK(launch_fft_c2c(lc(), nt.bf, nt.bf, 1, 0, p2));
    } else if (dev_fft_big_pow2(nt.bf, nt.bf, L, 0)) {
        return -1;
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    g_czt[key] = nt;
    *t = nt;
    return 0;
}
// the shared refusals of sp_czt / sp_zoom_welch, before the device is touched
int czt_check(const char *who, int64_t n, int64_t m, double start, double step) {
    if (n < 1 || m < 1) return fail("%s: n = %lld inputs and m = %lld outputs must both be at least 1", who, (long long)n, (long long)m);
    if (!isfinite(start) || !isfinite(step)) return fail("%s: start and step must be finite", who);
    const int64_t cap = (int64_t)1 << SP_MAX_BIG_LOG2;
    if (n > cap || m > cap || czt_len(n, m) > cap)
        return fail("%s: n + m - 1 = %lld needs a transform beyond the limit of 2^%d points", who, (long long)(n + m - 1),
                    SP_MAX_BIG_LOG2);
    return 0;
}
// rows [r0, r0 + rows) through the multi-pass chirp-z: A[rows][L] <- IFFT_L(FFT_L(src pre) . bf); the caller keeps the first m
int czt_long_rows(const void *xd, bool cplx, int64_t ld, int64_t r0, int64_t rows, const float *win_d, const float *trend, bool lin,
                  const CztTab &t, int64_t n, cf *A) {
    LAUNCHCHK(launch_czt_pre(lc(), xd, cplx, ld, r0, rows, win_d, trend, lin, t.pre, n, t.L, A));
    if (dev_fft_big_pow2(A, A, t.L, 0, 0, rows)) return -1;
    LAUNCHCHK(launch_cmul_vec(lc(), A, t.bf, t.L, 0, A, rows));
    return dev_fft_big_pow2(A, A, t.L, 1, 0, rows);
}


// ---- segments longer than one workgroup transform (k_long.hip) -----------------------------------
// frames per chunk: the chunk's spectra (m x nfft complex64) stay below SP_LONG_CHUNK_BYTES
#define SP_LONG_CHUNK_BYTES ((size_t)192 << 20)
int64_t long_chunk_frames(int nfft, int64_t nframes) {
    int64_t m = (int64_t)(SP_LONG_CHUNK_BYTES / (sizeof(cf) * (size_t)nfft));
    if (m > 32768) m = 32768;
    if (m > nframes) m = nframes;
    if (m < 1) m = 1;
    return hook_cap("SP_LONG_CHUNK_FRAMES", m);
}
// spectra of frames [f0, f0+m) of one signal -> buf[m][nfft] (natural bin order, unscaled); segmean: 1 / 2 = every
// frame's own mean / least-squares line is removed first; pseg_d (optional, zeroed): per-frame time-domain power
int long_spectra(const void *xd, bool cplx, const float *win_d, int nfft, int hop, int64_t f0, int64_t m, const float *trend,
                 bool lin, int segmean, cf *buf, double *pseg_d) {
    const float *rec = nullptr;
    if (segmean) {
        if (g.longrec.ensure(sizeof(float) * 4 * (size_t)m)) return -1;
        LAUNCHCHK(launch_long_segstats(lc(), xd, cplx, f0, m, hop, nfft, segmean, (float *)g.longrec.p));
        rec = (const float *)g.longrec.p;
    }
    LAUNCHCHK(launch_long_pack(lc(), xd, cplx, win_d, nfft, hop, f0, m, trend, lin, rec, buf, pseg_d));
    return dev_fft_any(buf, buf, nfft, m, 0);
}


// ---- one-pass Welch: accumulate, then finish with a (possibly global) mean ------------------------
// Wf = FFT(window) on the device, cached under the window's content
int get_window_spectrum(const float *win, int nfft, const Xf &xf, void **Wf_d) {
    bool fresh = false;
    if (get_table_keyed(3, win, sizeof(float) * (size_t)nfft, nullptr, sizeof(cf) * (size_t)nfft, Wf_d, &fresh)) return -1;
    if (fresh) {
        std::vector<cf> wc((size_t)nfft);
        for (int i = 0; i < nfft; ++i) wc[(size_t)i] = make_float2(win[i], 0.f);
        HIPCHK(hipMemcpy(*Wf_d, wc.data(), sizeof(cf) * (size_t)nfft, hipMemcpyHostToDevice));
        LAUNCHCHK(launch_fft_c2c(lc(), (const cf *)*Wf_d, (cf *)*Wf_d, 1, 0, xf));
    }
    return 0;
}

// the nfft-4096 Welch shapes run as a pipeline of specialised waves (k_welch_pipe.hip): one 768-thread workgroup per CU.
// The pipeline spends 4 periods per workgroup filling and draining; the symmetric kernel takes ~4 periods per frame and workgroup at
// two workgroups per CU, so the pipeline wins from 2 frames per CU on (round 3, step / kernel ms: 2^24 samples
// 0.054 / 0.045 against 0.071 / 0.060, 2^22: 0.045 / 0.024 against 0.062 / 0.036, 2^20: 0.038 / 0.019 against 0.053 / 0.020; the
// threshold had been 32 per CU, which sent every shard below 2^25 samples to the symmetric kernel).  SP_WELCH_PIPE=0 turns the
// pipeline off, 2 forces it for any frame count (the tests' way to reach its tail handling).
#define SP_PIPE_MINFPC_DEFAULT 2
static bool welch_pipe_wanted(const Xf &xf, int hop, int64_t nframes) {
    const int mode = env_int("SP_WELCH_PIPE", 1);
    const int64_t minfpc = SP_PIPE_MINFPC_DEFAULT;   // frames per CU
    return welch_pipe_eligible(xf, hop) && (mode >= 2 || (mode == 1 && nframes >= minfpc * (int64_t)g.ncu - minfpc));
}

// FFT(window) on the host in float64, to find out whether it is confined to the bins ks = -K .. K, K <= 3 (periodic cosine-sum
// windows: Hann, Hamming, Blackman, Nuttall ...): everything outside below 1e-9 of the peak.  Cached under the window's content.
static bool cog_window_lobe(const float *win, int n, CogLobe *lb) {
    struct Entry {
        uint64_t key;
        int n;
        bool ok;
        CogLobe lb;
    };
    static std::vector<Entry> cache;
    const uint64_t h = mix_key(window_key(win, n), 11, 0);
    for (const Entry &e : cache)
        if (e.key == h && e.n == n) {
            *lb = e.lb;
            return e.ok;
        }
    Entry e{h, n, false, CogLobe{}};
    // the lobe bins exactly, and the energy outside them by Parseval: sum |W|^2 = n sum w^2
    double tot = 0.0;
    for (int i = 0; i < n; ++i) tot += (double)win[i] * (double)win[i];
    tot *= (double)n;
    double in = 0.0, peak = 0.0;
    CogLobe l{};
    l.K = 3;
    for (int ks = -3; ks <= 3; ++ks) {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < n; ++i) {
            const double a = -2.0 * M_PI * (double)(((int64_t)ks * i) % n) / (double)n;
            re += (double)win[i] * std::cos(a);
            im += (double)win[i] * std::sin(a);
        }
        l.wr[ks + 3] = re;
        l.wi[ks + 3] = im;
        in += re * re + im * im;
        if (re * re + im * im > peak) peak = re * re + im * im;
    }
    e.ok = peak > 0.0 && std::fabs(tot - in) <= 1e-9 * tot;      // (float32 window values: the tables' own rounding leaks ~1e-14)
    e.lb = l;
    if (cache.size() < 64) cache.push_back(e);
    *lb = l;
    return e.ok;
}


// does the window add up to a constant at this hop (COLA)?  c = sum_j w[n + j hop] for every n < hop, host float64 on the float32
// table (periodic Hann / Hamming at 50 % and 75 %: yes; Blackman at 50 %: no).  Cached under the window's content and the hop.
static bool window_cola(const float *win, int n, int hop, double *c_out) {
    struct Entry {
        uint64_t key;
        int n, hop;
        bool ok;
        double c;
    };
    static std::vector<Entry> cache;
    if (hop < 1 || n % hop != 0) return false;
    const uint64_t h = mix_key(window_key(win, n), 7, (uint64_t)hop);
    for (const Entry &e : cache)
        if (e.key == h && e.n == n && e.hop == hop) {
            *c_out = e.c;
            return e.ok;
        }
    double lo = 1e300, hi = -1e300, sum = 0.0;
    for (int i = 0; i < hop; ++i) {
        double c = 0.0;
        for (int j = i; j < n; j += hop) c += (double)win[j];
        lo = c < lo ? c : lo;
        hi = c > hi ? c : hi;
        sum += c;
    }
    Entry e{h, n, hop, false, sum / (double)hop};
    e.ok = e.c > 0.0 && (hi - lo) <= 2e-6 * e.c;          // (float32 table values: their own rounding leaves ~1e-7)
    if (cache.size() < 64) cache.push_back(e);
    *c_out = e.c;
    return e.ok;
}

// request for the epilogue in the same call (k_op_fused: column sums + finish / export in ONE launch; taken when the window's
// spectrum is confined to the bins -3 .. 3 -- every cosine-sum window -- unless SP_OP_UNFUSED=1): done = true on return when
// `out` has been produced, otherwise the caller runs k_op_finish as before
struct FusedOut {
    bool export_state;
    int sided;
    double scale;          // already divided by the frame count
    double *out;
    bool done;
    // pipelined sharded PSD: the previous step's summed state, applied by the same launch behind `prev_wait` (its all-reduce)
    OpPrev prev = OpPrev{nullptr, nullptr, nullptr, 0, 0.0};
    hipEvent_t prev_wait = nullptr;
    bool prev_done = false;
};
unsigned *get_ticket(Scratch &t) {
    if (!t.p) {                         // 9 counters, 64 bytes apart (k_op_fused)
        if (t.ensure(1024)) return nullptr;
        if (hipMemset(t.p, 0, 1024) != hipSuccess) return nullptr;
    }
    return (unsigned *)t.p;
}
// streaming engine (sp_welch_dist_*): a scratch set of its own per step parity, and the epilogue launched on another stream
// behind an event recorded after the main kernel -- so that it runs beside the NEXT step's main kernel
struct SplitLaunch {
    Scratch *work, *onepass, *trend, *ticket;
    hipStream_t epi;
    hipEvent_t ev_main;
    int reserve_cus = 0;       // CUs left to the collective's kernel: the main kernel is partitioned over ncu - reserve_cus
};

// the shard state (5 n + 8 doubles, k_op_finish<EXPORT>'s layout) of a shape the carry / pipeline kernels do not take -- any hop,
// any workgroup transform length (k_welch_opx.hip): mean estimate and main kernel on the launch stream, the two reductions on
// the streaming engine's epilogue stream behind the main kernel's event when `sl` is given (its scratch set of the step's
// parity), else on the launch stream.  Real input runs two frames per transform from two frames on (SP_NO_REALPAIR: one).
int welch_export_generic(const void *xd, bool cplx, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                         int64_t nmean, const Xf &xf, double *st_d, const void **win_out = nullptr, const SplitLaunch *sl = nullptr) {
    Scratch &S_work = sl ? *sl->work : g.work, &S_trend = sl ? *sl->trend : g.pend_trend;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    if (win_out) *win_out = win_d;
    // FFT(window) for the apply that follows: made (when not cached) on the launch stream BEFORE the main kernel, so that an
    // epilogue-stream apply ordered behind the main kernel's event finds it
    void *Wf_d;
    if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
    if (S_trend.ensure(256)) return -1;
    float *trend = (float *)S_trend.p;
    const bool pair = !cplx && nframes >= 2 && !env_flag("SP_NO_REALPAIR");
    const int ncu_p = (sl && sl->reserve_cus > 0 && sl->reserve_cus < g.ncu) ? g.ncu - sl->reserve_cus : g.ncu;
    const RunPart rp = run_partition(xf.L, pair ? (nframes + 1) / 2 : nframes, ncu_p);
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_part = pad(sizeof(float) * (size_t)rp.groups * xf.L), b_cpart = pad(sizeof(cf) * (size_t)rp.groups * nfft);
    const size_t b_red = pad(sizeof(double) * (3 * (size_t)nfft + 2 * (size_t)opx_tot_blocks()));
    if (S_work.ensure(b_part + b_cpart + b_red)) return -1;
    char *w0 = (char *)S_work.p;
    float *partial = (float *)w0;
    cf *cpart = (cf *)(w0 + b_part);
    double *A = (double *)(w0 + b_part + b_cpart), *csum = A + nfft, *tpart = csum + 2 * (size_t)nfft;
    const LaunchCtx mc = lc();
    LAUNCHCHK(launch_op_estimate(mc, xd, cplx, nsig, nullptr, trend));
    {
        ProfScope ps(mc.stream);
        LAUNCHCHK(launch_welch_opx(mc, xd, cplx, pair, (const float *)win_d, hop, nframes, trend, xf, rp, partial, cpart));
    }
    g.last_kernel = pair ? "k_welch_opx(realpair)" : "k_welch_opx";
    LaunchCtx ec = mc;
    if (sl) {
        HIPCHK(hipEventRecord(sl->ev_main, mc.stream));
        HIPCHK(hipStreamWaitEvent(sl->epi, sl->ev_main, 0));
        ec = LaunchCtx{sl->epi, g.ncu};
    }
    LAUNCHCHK(launch_opx_reduce(ec, partial, cpart, rp.groups, xf, xd, cplx, trend, hop, nframes, nmean, A, csum, tpart));
    LAUNCHCHK(launch_opx_finish(ec, (const float *)win_d, A, csum, tpart, trend, hop, nframes, nmean, pair, xf, st_d));
    return 0;
}

// want_sum: also produce the shard's plain sample sum (split ABI, one more tiny launch); without it the finish kernel
// derives the shard mean itself
int welch_accum_locked(const void *xd, bool cplx, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                       int64_t nmean, bool want_sum, FusedOut *fo = nullptr, const SplitLaunch *sl = nullptr) {
    Scratch &S_work = sl ? *sl->work : g.work, &S_one = sl ? *sl->onepass : g.onepass, &S_trend = sl ? *sl->trend : g.pend_trend;
    Scratch &S_ticket = sl ? *sl->ticket : g.ticket;
    if (!wg_capable(nfft))
        return fail("sharded / split Welch PSD (sp_welch_accum, sp_welch_export, sp_welch_dist_*): segments longer than one workgroup "
                    "transform are not sharded (nfft = %d; powers of two up to %d, other lengths up to %d) -- the "
                    "long-segment regime has few, large frames: run sp_welch_psd on one GPU", nfft, SP_MAX_WG_FFT, SP_MAX_WG_FFT / 2);
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    if (nmean < 1 || nmean > nsig) return fail("sp_welch_accum: nmean must be in [1, nsig]");
    if (!welch_carry_eligible(xf, hop, false)) {
        // every other shape: the generic one-pass kernel exports the state; the split ABI keeps it pending for k_op_apply.
        // A shard of a frame-sharded stream owns at most its frames' hops plus the halo and tail: more is a caller error
        if (nmean > nframes * (int64_t)hop + nfft - 1)
            return fail("one-pass Welch: %lld own samples (nmean) cannot belong to %lld frames of %d with hop %d (at most "
                        "nframes * hop + nfft - 1 = %lld)", (long long)nmean, (long long)nframes, nfft, hop,
                        (long long)(nframes * (int64_t)hop + nfft - 1));
        if (fo && fo->export_state) {
            if (welch_export_generic(xd, cplx, nsig, win, nfft, hop, nframes, nmean, xf, fo->out, nullptr, sl)) return -1;
            fo->done = true;
            g_pend.valid = false;
            return 0;
        }
        if (fo || sl) return fail("internal: generic one-pass Welch exports its state only");
        if (S_one.ensure(sizeof(double) * (5 * (size_t)nfft + 8))) return -1;
        double *st_d = (double *)S_one.p;
        const void *win_d = nullptr;
        if (welch_export_generic(xd, cplx, nsig, win, nfft, hop, nframes, nmean, xf, st_d, &win_d)) return -1;
        void *Wf_d;
        if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
        g_pend = Pending{};
        g_pend.valid = true;
        g_pend.xd = xd;
        g_pend.cplx = cplx;
        g_pend.nsig = nsig;
        g_pend.nframes = nframes;
        g_pend.nmean = nmean;
        g_pend.nfft = nfft;
        g_pend.hop = hop;
        g_pend.xf = xf;
        g_pend.win_d = (const float *)win_d;
        g_pend.Wf = (const cf *)Wf_d;
        g_pend.state = st_d;
        g_pend.sum_d = st_d + 5 * (size_t)nfft + 3;          // the own samples' plain sum (re, im)
        return 0;
    }
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    void *Wf_d;
    if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
    // its own trend record: calls between sp_welch_accum and sp_welch_finish reuse the shared one
    if (S_trend.ensure(256)) return -1;
    TrendBuf tb{(float *)S_trend.p, nullptr};
    // real input at hop = nfft/2: two frames per transform on the pipeline (k_welch_pipe modes 3/4), partitioned over frame PAIRS
    const bool realpair = !cplx && 2 * hop == nfft && nframes >= 2 && !env_flag("SP_NO_REALPAIR") &&
                          welch_pipe_wanted(xf, hop, (nframes + 1) / 2);
    // (not at hop = nfft: the one-pass front role with 16 new samples per thread and their block sums spills 20 registers and
    //  runs at half the symmetric kernel's rate, 1.00 against 0.50 ms at 2^28 samples; the plain mode is faster there, 0.40 / 0.44)
    //  (SP_WELCH_PIPE=2 still forces it: tests/test_gpu_pipe.py keeps the instantiation correct)
    const bool pipe = realpair || ((hop != nfft || env_int("SP_WELCH_PIPE", 1) >= 2) && welch_pipe_wanted(xf, hop, nframes));
    const int ncu_p = (sl && sl->reserve_cus > 0 && sl->reserve_cus < g.ncu) ? g.ncu - sl->reserve_cus : g.ncu;   // (pipeline: one workgroup per CU)
    const RunPart rp = realpair ? run_partition(xf.L, (nframes + 1) / 2, ncu_p, 1)
                                : (pipe ? run_partition(xf.L, nframes, ncu_p, 1) : run_partition(xf.L, nframes, g.ncu));
    if (S_work.ensure(sizeof(float) * (size_t)rp.groups * xf.L)) return -1;
    const size_t sp_bytes = sizeof(cf) * (size_t)rp.groups * (size_t)hop;
    const size_t st_doubles = (size_t)nfft + 2 * (size_t)hop + 8;
    const size_t sp_pad = (sp_bytes + 255) & ~(size_t)255;
    const size_t st_pad = (sizeof(double) * st_doubles + 255) & ~(size_t)255;
    if (S_one.ensure(sp_pad + st_pad + sizeof(cf) * (size_t)nfft)) return -1;
    cf *spartial = (cf *)S_one.p;
    double *stp = (double *)((char *)S_one.p + sp_pad);
    OnePass st;
    st.A = stp;
    st.Sl = stp + nfft;
    st.tot = st.Sl + 2 * (size_t)hop;
    st.dlt = st.tot + 2;
    double *sum_d = st.dlt + 2;
    cf *cw = (cf *)((char *)S_one.p + sp_pad + st_pad);
    float *partial = (float *)S_work.p;
    double *est = moments_scratch();
    if (!est) return -1;
    (void)est;                       // the main kernel estimates mu0 itself and publishes it in tb.f
    st.sym = realpair ? 1 : 0;
    // mode 9 of the pipeline kernel: the window's lobe bins of sum_g X_g accumulated by the BACK role (4 VALU per frame) instead of
    // the front role's block sums (16), for cosine-sum windows that are COLA at this hop and the one-launch epilogue (SP_OP_NOLOBESUM=1
    // keeps the block sums)
    CogLobe lobe{};
    double cola_c = 0.0;
    const bool fused_ok = fo && !want_sum && !env_flag("SP_OP_UNFUSED") && cog_window_lobe(win, nfft, &lobe);
    const bool lobesum = fused_ok && pipe && !realpair && hop != nfft && !env_flag("SP_OP_NOLOBESUM") && window_cola(win, nfft, hop, &cola_c);
    if (!lobesum) cola_c = 0.0;
    const LaunchCtx mc = lc();
    // (streaming engine: the main kernel's event as the launch's own completion signal, not a record behind it)
    const bool stop_ev = sl && pipe && !g.profile;
    if (pipe) {
        ProfScope ps(mc.stream);
        LaunchCtx mcs = mc;
        if (stop_ev) mcs.stop = sl->ev_main;
        LAUNCHCHK(launch_welch_pipe(mcs, xd, cplx, (const float *)win_d, hop, nframes, tb.f, xf, partial, rp, spartial,
                                    realpair ? 3 : (lobesum ? 9 : 0)));
        g.last_kernel = realpair ? "k_welch_pipe(onepass,realpair)" : (lobesum ? "k_welch_pipe(onepass,lobesum)" : "k_welch_pipe(onepass)");
    } else {
        ProfScope ps(mc.stream);
        LAUNCHCHK(launch_welch(mc, xd, cplx, (const float *)win_d, hop, nframes, tb.f, false, xf, partial, rp, true,
                               spartial, &g.last_kernel));
    }
    if (!want_sum) st.dlt = nullptr;
    // the epilogue's launch context: the launch stream, or the engine's epilogue stream behind the main kernel's event
    LaunchCtx ec = lc();
    if (sl) {
        if (!stop_ev) HIPCHK(hipEventRecord(sl->ev_main, mc.stream));
        HIPCHK(hipStreamWaitEvent(sl->epi, sl->ev_main, 0));
        ec = LaunchCtx{sl->epi, g.ncu};
    }
    if (fused_ok) {
        unsigned *ticket = get_ticket(S_ticket);
        if (!ticket) return fail("ticket allocation failed");
        if (fo->prev.st && fo->prev_wait) HIPCHK(hipStreamWaitEvent(ec.stream, fo->prev_wait, 0));
        LAUNCHCHK(launch_op_fused(ec, xd, cplx, tb.f, (const float *)win_d, partial, spartial, rp.groups, nfft, hop, nframes, nmean,
                                  st, ticket, lobe, nullptr, fo->sided, fo->scale, fo->out, fo->export_state, fo->prev,
                                  sl != nullptr, cola_c));
        fo->done = true;
        fo->prev_done = fo->prev.st != nullptr;
        g_pend.valid = false;
        return 0;
    }
    LAUNCHCHK(launch_op_reduce(ec, xd, cplx, tb.f, partial, spartial, rp.groups, xf, hop, nframes, nmean, st,
                               want_sum ? sum_d : nullptr));
    g_pend.state = nullptr;
    g_pend.valid = true;
    g_pend.xd = xd;
    g_pend.cplx = cplx;
    g_pend.nsig = nsig;
    g_pend.nframes = nframes;
    g_pend.nmean = nmean;
    g_pend.nfft = nfft;
    g_pend.hop = hop;
    g_pend.xf = xf;
    g_pend.win_d = (const float *)win_d;
    g_pend.Wf = (const cf *)Wf_d;
    g_pend.st = st;
    g_pend.trend_f = tb.f;
    g_pend.cw = cw;
    g_pend.sum_d = sum_d;
    return 0;
}

int welch_finish_locked(const double *mean_d /*device or null*/, int64_t frames_total, int sided, double scale,
                        double *out_d, const LaunchCtx *ctx = nullptr) {
    if (!g_pend.valid) return fail("sp_welch_finish: no pending sp_welch_accum");
    g_pend.valid = false;
    if (g_pend.state) {          // generic shape: the pending state applied with the caller's mean, or the shard's own
        LAUNCHCHK(launch_op_apply(ctx ? *ctx : lc(), g_pend.state, g_pend.Wf, g_pend.nfft, sided, scale / (double)frames_total, out_d,
                                  mean_d));
        return 0;
    }
    LAUNCHCHK(launch_op_finish(ctx ? *ctx : lc(), g_pend.xd, g_pend.cplx, g_pend.trend_f, g_pend.win_d, g_pend.st, mean_d, g_pend.nmean,
                               g_pend.xf, g_pend.hop, g_pend.nframes, g_pend.cw, g_pend.Wf, sided,
                               scale / (double)frames_total, out_d));
    return 0;
}

// ---- RCCL inside the library: one process per GPU, the library owns a communicator and a stream for the collective ---------
// The functions come from the RCCL that is already in the process when there is one (torch ships its own copy under the
// same soname, so dlopen returns that instance), else from /opt/rocm/lib.
struct Rccl {
    void *dl = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitRankConfig)(ncclComm_t *, int, ncclUniqueId, int, void *) = nullptr;      // optional (NCCL >= 2.17)
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
} rccl;

int rccl_load() {
    if (rccl.dl) return 0;
    const char *names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    void *h = nullptr;
    for (const char *nm : names)
        if ((h = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return fail("RCCL not found (librccl.so.1): %s", dlerror());
    *(void **)&rccl.GetUniqueId = dlsym(h, "ncclGetUniqueId");
    *(void **)&rccl.CommInitRank = dlsym(h, "ncclCommInitRank");
    *(void **)&rccl.CommInitRankConfig = dlsym(h, "ncclCommInitRankConfig");
    *(void **)&rccl.CommDestroy = dlsym(h, "ncclCommDestroy");
    *(void **)&rccl.AllReduce = dlsym(h, "ncclAllReduce");
    *(void **)&rccl.GetErrorString = dlsym(h, "ncclGetErrorString");
    if (!rccl.GetUniqueId || !rccl.CommInitRank || !rccl.CommDestroy || !rccl.AllReduce || !rccl.GetErrorString)
        return fail("librccl lacks an expected symbol");
    rccl.dl = h;
    return 0;
}
#define NCCLCHK(expr)                                                                                 \
    do {                                                                                              \
        ncclResult_t r_ = (expr);                                                                     \
        if (r_ != ncclSuccess) return fail("%s failed: %s (%s:%d)", #expr, rccl.GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

struct Comm {
    ncclComm_t comm = nullptr;
    int world = 0, rank = -1;
    int ctas = 0;              // workgroups the communicator's kernels were limited to (0: RCCL's own choice)
} gcomm;

// RCCL's collective kernel cannot run beside k_welch_pipe: rcclGenericKernel takes 261-280 VGPRs + 17-32 AGPRs per lane at 256
// threads (code object metadata of librccl for gfx950) against the 80 per SIMD the pipeline leaves -- its workgroups would wait
// for pipeline workgroups to retire and then hold back the NEXT main kernel's on those CUs for the collective's duration (all 256
// workgroups of a main kernel are equal, so its makespan grows by that much).  Hence, with a communicator of more than one rank:
// the communicator is created with at most SP_DIST_RCCL_CTAS workgroups (default 4: the state is 160 KiB, latency-bound) and the
// streaming engine partitions its main kernels over ncu - that many CUs, so the collective always finds CUs of its own and
// runs beside the main kernel like the light epilogue does.  SP_DIST_RESERVE_CUS overrides the number of CUs left free (also for
// one rank, which is how the one-GPU tests reach the path), 0 turns it off.
static int dist_rccl_ctas() {
    const int v = env_int("SP_DIST_RCCL_CTAS", 4);
    return v < 0 ? 0 : (v > 64 ? 64 : v);
}
static int dist_reserved_cus() {
    if (getenv("SP_DIST_RESERVE_CUS")) {
        const int v = env_int("SP_DIST_RESERVE_CUS", 0);
        return v < 0 ? 0 : (v > g.ncu / 2 ? g.ncu / 2 : v);
    }
    // (twice the workgroup limit, at least 8: a limit RCCL rounds up must still find room; 8 CUs cost 1.2-1.5 % of the main
    //  kernel, tools/reserve_ab.sh: 0.5495 -> 0.5550 / 0.5580 ms at 2^28 samples for 4 / 8, 0.0819 -> 0.0825 / 0.0829 at 2^25)
    //  A multiple of 8 = one CU on every XCD: workgroups are dealt to the XCDs in turn, a reserve of 4 leaves XCDs 0-3 full --
    //  exactly where the collective's first workgroups go (tools/ubench/coexec_rccl.hip))
    const int want = 2 * gcomm.ctas > 8 ? 2 * gcomm.ctas : 8;
    return (gcomm.comm && gcomm.world > 1) ? (want + 7) / 8 * 8 : 0;
}

// ---- the streaming engine behind sp_welch_dist_submit / _flush ------------------------------------------------------------
// Step k: the main kernel (k_welch_pipe / k_welch_carry) on the launch stream A into the scratch set of parity k & 1; an event;
// the epilogue on the engine's stream B behind it: k_op_fused (with a communicator: EXPORT of this step's state + the apply of
// step k-1's all-reduced state, then ncclAllReduce of this step's state, all B-ordered).  A's next main kernel does not depend
// on B, so the epilogue (15-20 us of mostly one workgroup) and the collective run BESIDE it (tools/ubench/coexec.hip: two
// kernels from two streams share the CUs when the first leaves registers and wave slots free; the main kernel takes 408 of a
// SIMD's 512 VGPRs and 12 of a CU's 32 wave slots).  Only then does A wait for the PREVIOUS step's epilogue event -- which is
// what makes that step's (without communicator) or the step before's (with) output valid for the caller, in stream order.
// x must stay valid until the step is reported.
struct EngineSlot {
    bool busy = false;
    std::vector<float> win;
    int64_t frames_total = 0;
    int sided = 0;
    double scale = 0;
    double *out = nullptr;
};
struct Engine {
    hipStream_t epi = nullptr;
    hipEvent_t ev_main[2] = {nullptr, nullptr}, ev_epi[2] = {nullptr, nullptr};
    Scratch work[2], onepass[2], trend[2], ticket[2], st[2];
    EngineSlot slot[2];
    int64_t nsub = 0;            // submits since the last flush
    bool with_comm = false;      // mode of the steps in flight
} geng;

int engine_init() {
    if (geng.epi) return 0;
    HIPCHK(hipStreamCreateWithFlags(&geng.epi, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipEventCreateWithFlags(&geng.ev_main[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&geng.ev_epi[i], hipEventDisableTiming));
    }
    return 0;
}
void engine_release() {
    if (!geng.epi) return;
    (void)hipStreamSynchronize(geng.epi);
    for (int i = 0; i < 2; ++i) {
        (void)hipEventDestroy(geng.ev_main[i]);
        (void)hipEventDestroy(geng.ev_epi[i]);
        geng.ev_main[i] = geng.ev_epi[i] = nullptr;
        geng.work[i].release();
        geng.onepass[i].release();
        geng.trend[i].release();
        geng.ticket[i].release();
        geng.st[i].release();
        geng.slot[i].busy = false;
    }
    (void)hipStreamDestroy(geng.epi);
    geng.epi = nullptr;
    geng.nsub = 0;
}

// apply the all-reduced state of slot s -> its output, on the engine's stream (B-ordered behind the collective)
int engine_apply_locked(int s) {
    EngineSlot &sl = geng.slot[s];
    const int nfft = (int)sl.win.size();
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    void *Wf_d;
    if (get_window_spectrum(sl.win.data(), nfft, xf, &Wf_d)) return -1;
    LAUNCHCHK(launch_op_apply(LaunchCtx{geng.epi, g.ncu}, (const double *)geng.st[s].p, (const cf *)Wf_d, nfft, sl.sided,
                              sl.scale / (double)sl.frames_total, sl.out));
    return 0;
}

// a shape the generic one-pass kernel takes (every workgroup transform that the carry / pipeline kernels do not)
bool welch_generic_shape(int nfft, int hop) {
    if (!wg_capable(nfft)) return false;
    Xf xf;
    if (get_xf(nfft, &xf)) return false;
    return !welch_carry_eligible(xf, hop, false);
}

// this shard's additive state (sp_welch_export) into st_d (device, 5 nfft + 8 doubles)
int welch_export_locked(const void *xd, bool cplx, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                        int64_t nmean, double *st_d, const OpPrev *prev = nullptr, hipEvent_t prev_wait = nullptr,
                        bool *prev_done = nullptr, const SplitLaunch *sl = nullptr) {
    FusedOut fo{true, SP_SIDED_RAW, 1.0, st_d, false};
    if (prev) {
        fo.prev = *prev;
        fo.prev_wait = prev_wait;
    }
    if (welch_accum_locked(xd, cplx, nsig, win, nfft, hop, nframes, nmean, false, &fo, sl)) return -1;
    g_pend.valid = false;
    if (prev_done) *prev_done = fo.prev_done;
    if (fo.done) return 0;
    LAUNCHCHK(launch_op_finish(sl ? LaunchCtx{sl->epi, g.ncu} : lc(), g_pend.xd, g_pend.cplx, g_pend.trend_f, g_pend.win_d, g_pend.st, nullptr, g_pend.nmean,
                               g_pend.xf, g_pend.hop, g_pend.nframes, g_pend.cw, g_pend.Wf, SP_SIDED_RAW, 1.0, st_d, true));
    return 0;
}

}   // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int sp_version(void) { return SP_VERSION; }
int sp_max_wg_fft(void) { return SP_MAX_WG_FFT; }
const char *sp_last_error(void) { return g_err.c_str(); }
int sp_last_passes(int which) {
    std::lock_guard<std::mutex> lk(g.mu);
    return which >= 0 && which <= 9 ? g_passes[which] : 0;
}

int sp_init(int device_id) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.ready && (device_id < 0 || device_id == g.device)) return 0;
    if (g.ready)
        return fail("libspectral is bound to device %d for the life of the process (asked for %d)", g.device, device_id);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail("no HIP device visible (libspectral has no CPU fallback)");
    if (device_id < 0) {
        if (hipGetDevice(&device_id) != hipSuccess) device_id = 0;
    }
    if (device_id >= count) return fail("device %d out of range (%d visible)", device_id, count);
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("device %d is %s; libspectral is built for gfx950 only", device_id, prop.gcnArchName);
    g.device = device_id;
    g.ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    g.ready = true;
    return 0;
}

void sp_shutdown(void) {
    (void)sp_comm_destroy();
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.ready) return;
    engine_release();
    (void)hipDeviceSynchronize();
    for (auto &kv : g.twiddles) (void)hipFree(kv.second);
    g.twiddles.clear();
    for (auto &kv : g.blue) {
        (void)hipFree(kv.second.chirp);
        (void)hipFree(kv.second.bf);
    }
    g.blue.clear();
    g.in0.release();
    g.in1.release();
    g.out0.release();
    g.work.release();
    g.small.release();
    g.trends.release();
    g.onepass.release();
    g.ticket.release();
    g.epi.release();
    g.pend_trend.release();
    g.pend_x.release();
    g.cmS.release();
    g.cmT.release();
    g.cmG.release();
    g.cmH.release();
    g.cmO.release();
    g.bigA.release();
    g.bigB.release();
    g.bigT.release();
    g.blueA.release();
    g.blueB.release();
    g.longrec.release();
    g.mtS.release();
    g.wbW.release();
    g.wbP.release();
    g.wbA.release();
    g.famZ.release();
    g.famA.release();
    g.nuRec.release();
    g.nuGrid.release();
    g.arPart.release();
    g.subPart.release();
    g.subMat.release();
    g.dwtS.release();
    g.arSmall.release();
    for (auto &kv : g.bigtw) {
        (void)hipFree((void *)kv.second.hi);
        (void)hipFree((void *)kv.second.lo);
    }
    g.bigtw.clear();
    for (auto &kv : g.blue_big) {
        (void)hipFree(kv.second.chirp);
        (void)hipFree(kv.second.bf);
    }
    g.blue_big.clear();
    czt_release();
    g_cztAcc.release();
    g_pend.valid = false;
    tables_release();
    g.ready = false;
}

int sp_set_stream(void *hip_stream) {
    if (ensure_init()) return -1;
    ApiLock lk;
    hipStream_t ns = (hipStream_t)hip_stream;
    if (ns != g.stream) {
        // the library's scratch buffers are shared by all calls: work already queued on the old stream must finish
        // before work on the new one may reuse them.  (The old stream may have been destroyed by its owner: errors of
        // the record are dropped, there is nothing left to order against then.)
        if (!g.ev_sw && hipEventCreateWithFlags(&g.ev_sw, hipEventDisableTiming) != hipSuccess) g.ev_sw = nullptr;
        if (g.ev_sw) {
            if (hipEventRecord(g.ev_sw, g.stream) == hipSuccess) (void)hipStreamWaitEvent(ns, g.ev_sw, 0);
            (void)hipGetLastError();
        }
        g.stream = ns;
    }
    return 0;
}

int sp_synchronize(void) {
    if (ensure_init()) return -1;
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}

int sp_profile_enable(int on) {
    if (ensure_init()) return -1;
    if (on && !g.ev0) {
        HIPCHK(hipEventCreate(&g.ev0));
        HIPCHK(hipEventCreate(&g.ev1));
    }
    g.profile = on != 0;
    g.prof_valid = false;
    return 0;
}

int sp_profile_last_ms(double *ms) {
    if (ensure_init()) return -1;
    if (!g.profile || !g.prof_valid) return fail("sp_profile_last_ms: no profiled launch recorded");
    HIPCHK(hipEventSynchronize(g.ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, g.ev0, g.ev1));
    *ms = (double)t;
    return 0;
}

const char *sp_profile_last_kernel(void) { return g.last_kernel; }

int sp_device_info(int64_t out[4]) {
    if (ensure_init()) return -1;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, g.device));
    out[0] = prop.multiProcessorCount;
    out[1] = (int64_t)prop.maxSharedMemoryPerMultiProcessor;
    out[2] = prop.clockRate;
    out[3] = prop.warpSize;
    return 0;
}

int sp_mean(const void *x, int x_dtype, int64_t n, double out[2], int mem) {
    if (ensure_init()) return -1;
    if (n <= 0) return fail("sp_mean: n must be positive");
    ApiLock lk;
    const size_t esz = x_dtype == SP_DTYPE_C64 ? 8 : 4;
    Stage st(mem);
    const void *xd;
    st.in(g.in0, x, esz * (size_t)n, &xd);
    if (st.commit()) return -1;
    TrendBuf tb;
    if (get_trendbuf(1, &tb)) return -1;
    if (set_trend(tb, 0, xd, x_dtype == SP_DTYPE_C64, n, 1, 0, 0)) return -1;
    double h[2];   // (the result goes to the host in both modes: no finish())
    HIPCHK(hipMemcpyAsync(h, tb.d, sizeof h, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    out[0] = h[0];
    out[1] = h[1];
    return 0;
}

int sp_fft_c2c(const void *in, void *out, int64_t n, int64_t batch, int direction, int mem) {
    if (ensure_init()) return -1;
    if (n < 1 || batch < 0) return fail("sp_fft_c2c: bad n/batch");
    if (direction != -1 && direction != 1) return fail("sp_fft_c2c: direction must be -1 or +1");
    if (batch == 0) return 0;
    ApiLock lk;
    const size_t bytes = sizeof(cf) * (size_t)n * (size_t)batch;
    Stage st(mem);
    const cf *din;
    cf *dout;
    st.inout(g.in0, in, out, bytes, &din, &dout);
    if (st.commit()) return -1;
    if (dev_fft_any(din, dout, n, batch, direction > 0)) return -1;
    return st.finish();
}

int sp_welch_psd(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                 int detrend, double mean_re, double mean_im, int sided, double scale, double *pxx_out, int mem) {
    if (ensure_init()) return -1;
    if (check_frames("sp_welch_psd", nsig, nfft, hop, nframes)) return -1;
    if (sided < 1 || sided > 3) return fail("sp_welch_psd: bad sided");
    if (detrend < 0 || detrend > 4) return fail("sp_welch_psd: detrend must be 0..4");
    const int segmean = detrend == SP_DETREND_SEGMEAN ? 1 : (detrend == SP_DETREND_SEGLINEAR ? 2 : 0);   // per-segment: generic kernel
    if (segmean) {
        detrend = SP_DETREND_CONST;
        mean_re = mean_im = 0.0;
    }
    ApiLock lk;
    const bool lng = !wg_capable(nfft);          // segment longer than one workgroup transform: multi-kernel path
    Xf xf;
    if (!lng && get_xf(nfft, &xf)) return -1;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    const int nb = nbins_host(nfft, sided);
    Stage st(mem);
    const void *xd;
    double *out_d;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.out(g.out0, pxx_out, sizeof(double) * (size_t)nb, &out_d);
    if (st.commit()) return -1;
    const bool allow_carry = !env_flag("SP_WELCH_GENERIC");
    if (lng) {
        void *win_d;
        if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
        TrendBuf tb;
        if (get_trendbuf(1, &tb)) return -1;
        if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_re, mean_im)) return -1;
        const int64_t mc = long_chunk_frames(nfft, nframes);
        if (g.bigA.ensure(sizeof(cf) * (size_t)mc * (size_t)nfft) || g.work.ensure(sizeof(double) * (size_t)nfft)) return -1;
        cf *S = (cf *)g.bigA.p;
        double *acc = (double *)g.work.p;
        HIPCHK(hipMemsetAsync(acc, 0, sizeof(double) * (size_t)nfft, g.stream));
        for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
            const int64_t m = nframes - f0 < mc ? nframes - f0 : mc;
            if (long_spectra(xd, cplx, (const float *)win_d, nfft, hop, f0, m, tb.f, detrend == 2, segmean, S, nullptr)) return -1;
            LAUNCHCHK(launch_long_acc_psd(lc(), S, m, nfft, acc));
        }
        LAUNCHCHK(launch_long_finish(lc(), acc, nfft, sided, scale / (double)nframes, false, out_d));
        g.last_kernel = "k_long_acc_psd";
    } else if (detrend == SP_DETREND_MEAN && allow_carry && !segmean && !env_flag("SP_WELCH_TWOPASS") &&
               welch_carry_eligible(xf, hop, false) &&
               (cplx || (2 * hop == nfft && nframes >= 2 && !env_flag("SP_NO_REALPAIR") &&
                         welch_pipe_wanted(xf, hop, (nframes + 1) / 2)))) {
        // global-mean detrend in ONE pass over the signal (estimate + exact correction in the epilogue)
        FusedOut fo{false, sided, scale / (double)nframes, out_d, false};
        if (welch_accum_locked(xd, cplx, nsig, win, nfft, hop, nframes, nsig, false, &fo)) return -1;
        if (!fo.done && welch_finish_locked(nullptr, nframes, sided, scale, out_d)) return -1;
    } else {
        void *win_d;
        if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
        TrendBuf tb;
        if (get_trendbuf(1, &tb)) return -1;
        if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_re, mean_im)) return -1;
        const bool pair = !cplx && nframes >= 2 && !segmean && !env_flag("SP_NO_REALPAIR");
        const bool pipe = !pair && !segmean && detrend != 2 && allow_carry && welch_pipe_wanted(xf, hop, nframes);
        const bool pipe_rp = pair && detrend != 2 && allow_carry && 2 * hop == nfft && welch_pipe_wanted(xf, hop, (nframes + 1) / 2);
        const RunPart rp = pipe_rp ? run_partition(xf.L, (nframes + 1) / 2, g.ncu, 1)
                                   : (pipe ? run_partition(xf.L, nframes, g.ncu, 1)
                                           : (pair ? run_partition(xf.L, (nframes + 1) / 2, g.ncu,
                                                                   welch_rp_groups_per_cu(xf, detrend == 2))
                                                   : run_partition(xf.L, nframes, g.ncu)));
        if (g.work.ensure(sizeof(float) * (size_t)rp.groups * xf.L)) return -1;
        float *partial = (float *)g.work.p;
        {
            ProfScope ps;
            if (pipe_rp) {
                LAUNCHCHK(launch_welch_pipe(lc(), xd, false, (const float *)win_d, hop, nframes, tb.f, xf, partial, rp, nullptr, 3));
                g.last_kernel = "k_welch_pipe(realpair)";
            } else if (pair) {
                // real input: two frames per complex transform, |Z|^2 accumulated, symmetrised by the finish kernel
                LAUNCHCHK(launch_welch_rp(lc(), (const float *)xd, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf,
                                          partial, rp));
                g.last_kernel = "k_welch_rp";
            } else if (pipe) {
                LAUNCHCHK(launch_welch_pipe(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, xf, partial, rp, nullptr));
                g.last_kernel = "k_welch_pipe";
            } else {
                LAUNCHCHK(launch_welch(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, partial,
                                       rp, allow_carry, nullptr, &g.last_kernel, segmean));
            }
        }
        LAUNCHCHK(launch_welch_finish(lc(), partial, rp.groups, xf, sided, scale / (double)nframes, out_d, pair ? 1 : 0));
    }
    return st.finish();
}

int sp_welch_accum(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                   int64_t nmean, double *sum_out, int mem) {
    if (ensure_init()) return -1;
    if (check_frames("sp_welch_accum", nsig, nfft, hop, nframes)) return -1;
    ApiLock lk;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    Stage st(mem);
    const void *xd;
    // staged in a scratch of its own, not in g.in0: the pending state keeps xd (k_op_finish reads the record's edge blocks), and every
    // host-memory call between sp_welch_accum and sp_welch_finish stages into g.in0 (and may grow it, which frees it)
    st.in(g.pend_x, x, esz * (size_t)nsig, &xd);
    if (st.commit()) return -1;
    if (welch_accum_locked(xd, cplx, nsig, win, nfft, hop, nframes, nmean, true)) return -1;
    if (!sum_out) return 0;
    // real difference: the sums live in the pending state, not in a staged piece -- a device caller gets them by a copy in stream order
    HIPCHK(hipMemcpyAsync(sum_out, g_pend.sum_d, sizeof(double) * 2, mem ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream));
    return st.finish();
}

int sp_welch_finish(const double *mean, int64_t frames_total, int sided, double scale, double *pxx_out, int mem) {
    if (ensure_init()) return -1;
    if (sided < 1 || sided > 3) return fail("sp_welch_finish: bad sided");
    if (frames_total < 1) return fail("sp_welch_finish: frames_total must be positive");
    ApiLock lk;
    if (!g_pend.valid) return fail("sp_welch_finish: no pending sp_welch_accum");
    const int nb = nbins_host(g_pend.nfft, sided);
    Stage st(mem);
    double *out_d;
    const double *mean_d;
    st.out(g.out0, pxx_out, sizeof(double) * (size_t)nb, &out_d);
    st.in(g.out0, mean, sizeof(double) * 2, &mean_d);
    if (st.commit()) return -1;
    if (welch_finish_locked(mean_d, frames_total, sided, scale, out_d)) return -1;
    return st.finish();
}

int sp_welch_export(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                    int64_t nmean, double *state, int mem) {
    if (ensure_init()) return -1;
    if (check_frames("sp_welch_export", nsig, nfft, hop, nframes)) return -1;
    ApiLock lk;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    const size_t nst = 5 * (size_t)nfft + 8;
    Stage st(mem);
    const void *xd;
    double *st_d;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.out(g.out0, state, sizeof(double) * nst, &st_d);
    if (st.commit()) return -1;
    if (welch_export_locked(xd, cplx, nsig, win, nfft, hop, nframes, nmean, st_d)) return -1;
    return st.finish();
}

int sp_welch_apply(const double *state, const float *win, int nfft, int64_t frames_total, int sided, double scale,
                   double *pxx_out, int mem) {
    if (ensure_init()) return -1;
    if (sided < 1 || sided > 3) return fail("sp_welch_apply: bad sided");
    if (frames_total < 1) return fail("sp_welch_apply: frames_total must be positive");
    ApiLock lk;
    if (!wg_capable(nfft))
        return fail("sp_welch_apply: segments longer than one workgroup transform are not sharded (nfft = %d, at most %d)", nfft,
                    SP_MAX_WG_FFT);
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    void *Wf_d;
    if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
    const int nb = nbins_host(nfft, sided);
    const size_t nst = 5 * (size_t)nfft + 8;
    Stage st(mem);
    const double *st_d;
    double *out_d;
    st.in(g.out0, state, sizeof(double) * nst, &st_d);
    st.out(g.out0, pxx_out, sizeof(double) * (size_t)nb, &out_d);
    if (st.commit()) return -1;
    LAUNCHCHK(launch_op_apply(lc(), st_d, (const cf *)Wf_d, nfft, sided, scale / (double)frames_total, out_d));
    return st.finish();
}

/* ---- multi-GPU inside the library: one process per GPU, RCCL over xGMI --------------------------------------------------- */
int sp_comm_unique_id(void *id_out) {
    if (!id_out) return fail("sp_comm_unique_id: null pointer");
    std::lock_guard<std::mutex> lk(g.mu);
    if (rccl_load()) return -1;
    static_assert(sizeof(ncclUniqueId) == SP_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(rccl.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return 0;
}

int sp_comm_init(const void *id_in, int world, int rank) {
    if (ensure_init()) return -1;
    if (!id_in || world < 1 || rank < 0 || rank >= world) return fail("sp_comm_init: bad id/world/rank");
    ApiLock lk;
    if (gcomm.comm) return fail("sp_comm_init: a communicator exists already (sp_comm_destroy first)");
    if (geng.nsub) return fail("sp_comm_init: streaming steps are in flight (sp_welch_dist_flush first)");
    if (rccl_load()) return -1;
    HIPCHK(hipSetDevice(g.device));
    ncclUniqueId id;
    memcpy(&id, id_in, sizeof id);
    // at most `ctas` workgroups for this communicator's kernels (ncclConfig_t in its first public layout, NCCL 2.17: newer
    // libraries accept the shorter structure by its size / version fields); without the entry point: RCCL's own choice
    struct ConfigV217 {
        size_t size;
        unsigned magic, version;
        int blocking, cgaClusterSize, minCTAs, maxCTAs;
        const char *netName;
    };
    const int ctas = dist_rccl_ctas();
    gcomm.ctas = 0;
    if (rccl.CommInitRankConfig && ctas > 0) {
        ConfigV217 cfg{sizeof(ConfigV217), 0xcafebeefu, 21700u, INT_MIN, INT_MIN, 1, ctas, nullptr};
        NCCLCHK(rccl.CommInitRankConfig(&gcomm.comm, world, id, rank, &cfg));
        gcomm.ctas = ctas;
    } else {
        NCCLCHK(rccl.CommInitRank(&gcomm.comm, world, id, rank));
    }
    gcomm.world = world;
    gcomm.rank = rank;
    return 0;
}

int sp_comm_info(int out[2]) {
    out[0] = gcomm.comm ? gcomm.world : 0;
    out[1] = gcomm.comm ? gcomm.rank : -1;
    return 0;
}

int sp_comm_destroy(void) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (!gcomm.comm) return 0;
    if (geng.epi) (void)hipStreamSynchronize(geng.epi);
    (void)hipStreamSynchronize(g.stream);
    (void)rccl.CommDestroy(gcomm.comm);
    gcomm.comm = nullptr;
    gcomm.world = 0;
    gcomm.rank = -1;
    geng.nsub = 0;
    geng.slot[0].busy = geng.slot[1].busy = false;
    return 0;
}

int sp_welch_dist_submit(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                         int64_t nmean, int64_t frames_total, int sided, double scale, double *pxx_out, int *ndone) {
    if (ensure_init()) return -1;
    if (check_frames("sp_welch_dist_submit", nsig, nfft, hop, nframes)) return -1;
    if (sided < 1 || sided > 3) return fail("sp_welch_dist_submit: bad sided");
    if (frames_total < nframes) return fail("sp_welch_dist_submit: frames_total is the frame count of the WHOLE stream");
    if (!x || !pxx_out) return fail("sp_welch_dist_submit: null pointer");
    if (ndone) *ndone = 0;
    ApiLock lk;
    if (engine_init()) return -1;
    const bool comm = gcomm.comm != nullptr;
    if (geng.nsub && comm != geng.with_comm) return fail("sp_welch_dist_submit: communicator changed with steps in flight");
    geng.with_comm = comm;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const int64_t k = geng.nsub;
    const int s = (int)(k & 1), o = 1 - s;
    // slot s held step k - 2: its epilogue event was waited for on the launch stream during submit k - 1 (below), so the main
    // kernel of this step may overwrite its scratch set
    EngineSlot &cur = geng.slot[s], &prv = geng.slot[o];
    SplitLaunch sl{&geng.work[s], &geng.onepass[s], &geng.trend[s], &geng.ticket[s], geng.epi, geng.ev_main[s]};
    sl.reserve_cus = comm ? dist_reserved_cus() : 0;
    const LaunchCtx ec{geng.epi, g.ncu};
    if (comm) {
        const size_t nst = 5 * (size_t)nfft + 8;
        if (geng.st[s].ensure(sizeof(double) * nst)) return -1;
        double *st_d = (double *)geng.st[s].p;
        // the launch that finishes THIS step's state also applies the previous step's all-reduced state (same transform length;
        // B-ordered behind that step's collective) -- otherwise a k_op_apply launch of its own, on B as well
        OpPrev prev{nullptr, nullptr, nullptr, 0, 0.0};
        if (prv.busy && (int)prv.win.size() == nfft) {
            Xf xfo;
            if (get_xf(nfft, &xfo)) return -1;
            void *Wf_o;
            if (get_window_spectrum(prv.win.data(), nfft, xfo, &Wf_o)) return -1;
            prev = OpPrev{(const double *)geng.st[o].p, (const cf *)Wf_o, prv.out, prv.sided, prv.scale / (double)prv.frames_total};
        }
        bool prev_done = false;
        if (welch_export_locked(x, cplx, nsig, win, nfft, hop, nframes, nmean, st_d, prev.st ? &prev : nullptr, nullptr, &prev_done, &sl))
            return -1;
        if (prv.busy && !prev_done && engine_apply_locked(o)) return -1;
        NCCLCHK(rccl.AllReduce(st_d, st_d, nst, ncclDouble, ncclSum, gcomm.comm, geng.epi));
    } else if (welch_generic_shape(nfft, hop)) {
        // shapes of the generic one-pass kernel: this step's state, then k_op_apply on the engine's stream (B-ordered)
        if (geng.st[s].ensure(sizeof(double) * (5 * (size_t)nfft + 8))) return -1;
        double *st_d = (double *)geng.st[s].p;
        if (welch_export_locked(x, cplx, nsig, win, nfft, hop, nframes, nmean, st_d, nullptr, nullptr, nullptr, &sl)) return -1;
        Xf xf;
        if (get_xf(nfft, &xf)) return -1;
        void *Wf_d;
        if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
        LAUNCHCHK(launch_op_apply(ec, st_d, (const cf *)Wf_d, nfft, sided, scale / (double)frames_total, pxx_out));
    } else {
        FusedOut fo{false, sided, scale / (double)frames_total, pxx_out, false};
        if (welch_accum_locked(x, cplx, nsig, win, nfft, hop, nframes, nmean, false, &fo, &sl)) return -1;
        if (!fo.done && welch_finish_locked(nullptr, frames_total, sided, scale, pxx_out, &ec)) return -1;
    }
    HIPCHK(hipEventRecord(geng.ev_epi[s], geng.epi));
    cur.busy = true;
    cur.win.assign(win, win + nfft);
    cur.frames_total = frames_total;
    cur.sided = sided;
    cur.scale = scale;
    cur.out = pxx_out;
    geng.nsub = k + 1;
    // the previous step's epilogue has had this step's main kernel to run beside: wait for it on the launch stream NOW (behind
    // the main kernel just enqueued).  That makes valid, in stream order: without communicator the output of step k - 1; with
    // one the output of step k - 2 (applied by step k - 1's epilogue launch).
    if (prv.busy) {
        // (this wait is a packet of its own between two main kernels: ~4 us per step, measured by leaving it out -- 0.0826 ->
        //  0.0784 ms at 2^25 samples.  It is what orders the scratch reuse and validates outputs in stream order; waiting only every
        //  few steps over more scratch sets would save most of it at the price of results arriving in batches: not done)
        HIPCHK(hipStreamWaitEvent(g.stream, geng.ev_epi[o], 0));
        if (!comm) {
            prv.busy = false;
            if (ndone) *ndone = 1;
        } else if (k >= 2 && ndone) {
            *ndone = 1;
        }
    }
    return 0;
}

int sp_welch_dist_flush(int *ndone) {
    if (ensure_init()) return -1;
    if (ndone) *ndone = 0;
    ApiLock lk;
    const int64_t k = geng.nsub;
    if (k == 0 || !geng.epi) return 0;
    const int s = (int)((k - 1) & 1);                 // the slot submitted last
    int done = 1;
    if (geng.with_comm) {
        // the last step's state still waits for its apply (B-ordered behind its collective); the step before it was applied by the
        // last step's epilogue launch and becomes valid with the same wait
        if (engine_apply_locked(s)) return -1;
        HIPCHK(hipEventRecord(geng.ev_epi[s], geng.epi));
        if (k >= 2) done = 2;
    }
    HIPCHK(hipStreamWaitEvent(g.stream, geng.ev_epi[s], 0));
    geng.slot[0].busy = geng.slot[1].busy = false;
    geng.nsub = 0;
    if (ndone) *ndone = done;
    return 0;
}

int sp_welch_psd_dist(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                      int64_t nmean, int64_t frames_total, int sided, double scale, double *pxx_out) {
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (geng.nsub) return fail("sp_welch_psd_dist: streaming steps are in flight (sp_welch_dist_flush first)");
    }
    int n = 0;
    if (sp_welch_dist_submit(x, x_dtype, nsig, win, nfft, hop, nframes, nmean, frames_total, sided, scale, pxx_out, &n)) return -1;
    return sp_welch_dist_flush(&n);
}

int sp_welch_csd(const void *x, const void *y, int dtype, int64_t nsig, int nch, int64_t y_ld, const float *win,
                 int nfft, int hop, int64_t nframes, int detrend, const double *mean_x, const double *mean_y,
                 int sided, double scale, double *pxx, double *pyy, double *pxy, int mem) {
    // (the frame kernels and their finish take the channel as grid.y; long segments walk the channels one by one)
    if (nch > 65535 && wg_capable(nfft)) return fail("sp_welch_csd: nch = %d is beyond the limit of 65535 channels per call", nch);
    if (ensure_init()) return -1;
    if (check_frames("sp_welch_csd", nsig, nfft, hop, nframes)) return -1;
    if (nch < 1 || y_ld < nsig) return fail("sp_welch_csd: bad nch / y_ld");
    if (sided < 1 || sided > 3) return fail("sp_welch_csd: bad sided");
    if (detrend < 0 || detrend > 4) return fail("sp_welch_csd: detrend must be 0..4");
    const int segmean = detrend == SP_DETREND_SEGMEAN ? 1 : (detrend == SP_DETREND_SEGLINEAR ? 2 : 0);
    if (segmean) {
        detrend = SP_DETREND_CONST;
        mean_x = mean_y = nullptr;
    }
    ApiLock lk;
    const bool lng = !wg_capable(nfft);
    Xf xf;
    if (!lng && get_xf(nfft, &xf)) return -1;
    const bool cplx = dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    Stage st(mem);
    const void *xd, *yd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * (size_t)y_ld * (size_t)nch, &yd);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(nch + 1, &tb)) return -1;
    if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_x ? mean_x[0] : 0, mean_x ? mean_x[1] : 0)) return -1;
    // real x against many real channels: the pair path below; with mean detrend at nfft 4096 / 50 % overlap the channels' means
    // are not taken by a pass of their own (4.2 GB at 63 channels x 2^24: 0.7 of 2.9 ms) but in one pass with the spectra
    // (k_welch_csd_pair<OP>: estimate + block sums, exact correction in k_csd_pair_finish); SP_CSD_TWOPASS=1: the separate pass
    const bool pair_path = !lng && !cplx && !segmean && csd_rp_eligible(xf) && nch >= 2 && nframes >= 2 && !env_flag("SP_NO_REALPAIR") &&
                           !env_flag("SP_CSD_XIY");
    // (from 8 channels on: below, the epilogue's fixed ~0.1 ms costs more than the channels' pass, 0.39 against 0.35 ms at 2 channels
    //  x 2^24, 0.55 / 0.56 at 8, 0.76 / 0.83 at 16; SP_CSD_ONEPASS=1 forces the form)
    const bool pair_op = pair_path && detrend == SP_DETREND_MEAN && xf.L == 4096 && 2 * hop == xf.L && nch <= 512 &&
                         (nch >= 8 || env_flag("SP_CSD_ONEPASS")) && !env_flag("SP_CSD_TWOPASS");
    if (pair_op) {
        HIPCHK(hipMemsetAsync(tb.f + 4, 0, sizeof(float) * 4 * (size_t)nch, g.stream));     // (the kernel publishes its estimates here)
    } else if (detrend != 0 && nch <= 512) {
        // all channels' means / trend lines in one launch pair (64 channels one by one cost 3 ms of launches)
        double *scr = moments_scratch();
        if (!scr) return -1;
        LAUNCHCHK(launch_moments(lc(), yd, cplx, nsig, detrend, scr, tb.d + 8, tb.f + 4, nch, y_ld));
    } else {
        for (int c = 0; c < nch; ++c)
            if (set_trend(tb, c + 1, (const char *)yd + esz * (size_t)y_ld * (size_t)c, cplx, nsig, detrend,
                          mean_y ? mean_y[2 * c] : 0, mean_y ? mean_y[2 * c + 1] : 0))
                return -1;
    }
    const size_t nb = (size_t)nbins_host(nfft, sided);
    double *pxx_d, *pyy_d, *pxy_d;
    st.out(g.out0, pxx, sizeof(double) * nb, &pxx_d);
    st.out(g.out0, pyy, sizeof(double) * nb * nch, &pyy_d);
    st.out(g.out0, pxy, sizeof(double) * nb * nch * 2, &pxy_d);
    if (st.commit()) return -1;
    if (lng) {
        // long segments: spectra of a chunk of frames of x, then of every channel against them (k_long.hip)
        const int64_t mc = long_chunk_frames(nfft, nframes);
        const size_t nf = (size_t)nfft;
        if (g.bigA.ensure(sizeof(cf) * (size_t)mc * nf) || g.bigB.ensure(sizeof(cf) * (size_t)mc * nf) ||
            g.work.ensure(sizeof(double) * nf * (1 + 3 * (size_t)nch)))
            return -1;
        cf *Sx = (cf *)g.bigA.p, *Sy = (cf *)g.bigB.p;
        double *axx = (double *)g.work.p, *ayy = axx + nf, *axy = ayy + nf * (size_t)nch;
        HIPCHK(hipMemsetAsync(axx, 0, sizeof(double) * nf * (1 + 3 * (size_t)nch), g.stream));
        for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
            const int64_t m = nframes - f0 < mc ? nframes - f0 : mc;
            if (long_spectra(xd, cplx, (const float *)win_d, nfft, hop, f0, m, tb.f, detrend == 2, segmean, Sx, nullptr)) return -1;
            LAUNCHCHK(launch_long_acc_psd(lc(), Sx, m, nfft, axx));
            for (int c = 0; c < nch; ++c) {
                if (long_spectra((const char *)yd + esz * (size_t)y_ld * (size_t)c, cplx, (const float *)win_d, nfft, hop, f0, m,
                                 tb.f + 4 * (c + 1), detrend == 2, segmean, Sy, nullptr))
                    return -1;
                LAUNCHCHK(launch_long_acc_csd(lc(), Sx, Sy, m, nfft, ayy + nf * (size_t)c, axy + 2 * nf * (size_t)c));
            }
        }
        const double sc = scale / (double)nframes;
        LAUNCHCHK(launch_long_finish(lc(), axx, nfft, sided, sc, false, pxx_d));
        for (int c = 0; c < nch; ++c) {
            LAUNCHCHK(launch_long_finish(lc(), ayy + nf * (size_t)c, nfft, sided, sc, false, pyy_d + nb * (size_t)c));
            LAUNCHCHK(launch_long_finish(lc(), axy + 2 * nf * (size_t)c, nfft, sided, sc, true, pxy_d + 2 * nb * (size_t)c));
        }
        return st.finish();
    }
    const RunPart rp = run_partition_2d(xf.L, nframes, g.ncu, nch);
    if (g.work.ensure(sizeof(float) * (size_t)rp.groups * xf.L * 4 * (size_t)nch)) return -1;
    float *partial = (float *)g.work.p;
    if (pair_path) {
        // real x against many real channels: the reference's packed pair spectra once, then one transform per
        // (channel, frame PAIR); Pxx from the real-pair PSD kernel.  (SP_CSD_XIY=1: the x + i y_c form below.)
        const int64_t npairs = (nframes + 1) / 2;
        const RunPart rpp = run_partition_2d(xf.L, npairs, g.ncu, nch, (int64_t)g.ncu * csd_pair_resident(xf, detrend == 2, pair_op));
        if (g.work.ensure(sizeof(float) * (size_t)rpp.groups * xf.L * 4 * (size_t)nch)) return -1;
        partial = (float *)g.work.p;
        if (g.cmS.ensure(sizeof(cf) * (size_t)npairs * (size_t)xf.L)) return -1;
        cf *Zx = (cf *)g.cmS.p;
        const RunPart rpx = run_partition(xf.L, npairs, g.ncu);
        LAUNCHCHK(launch_pairspec(lc(), (const float *)xd, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, rpx, Zx));
        if (pair_op) {
            const size_t N5 = (size_t)(5 * nfft + 8);
            const size_t b_spy = sizeof(cf) * (size_t)nch * (size_t)rpp.groups * (size_t)hop;
            const size_t b_sp = b_spy + sizeof(cf) * SP_COLSUM_SLICES * (size_t)hop;          // + the reference's slice sums
            const size_t b_sl = sizeof(double) * 2 * (size_t)hop * (size_t)(nch + 1), b_st = sizeof(double) * N5 * (size_t)(nch + 1);
            if (g.cmO.ensure(b_sp + b_sl + b_st)) return -1;
            cf *spartial = (cf *)g.cmO.p;
            double *Sl = (double *)((char *)g.cmO.p + b_sp), *Slx = Sl + 2 * (size_t)hop * (size_t)nch;
            double *st = (double *)((char *)g.cmO.p + b_sp + b_sl), *stx = st + N5 * (size_t)nch;
            void *Wf_d;
            if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
            LAUNCHCHK(launch_csd_pair(lc(), (const float *)yd, nch, y_ld, (const float *)win_d, hop, nframes, tb.f + 4, false, xf, Zx,
                                      partial, rpp, spartial));
            LAUNCHCHK(launch_cm_blocksums(lc(), spartial, nch, (int)rpp.groups, hop, Sl));
            LAUNCHCHK(launch_op_finish_channels(lc(), (const float *)yd, y_ld, nch, tb.f + 4, (const float *)win_d, Sl, (const cf *)Wf_d,
                                                hop, nframes, nsig, xf, st));
            // the reference (detrended by its exact mean: its d is rounding only, but B_x is needed for the channels' terms)
            cf *spx = (cf *)((char *)g.cmO.p + b_spy);
            LAUNCHCHK(launch_colsum_real(lc(), (const float *)xd, tb.f, hop, nframes, spx));
            LAUNCHCHK(launch_cm_blocksums(lc(), spx, 1, SP_COLSUM_SLICES, hop, Slx));
            LAUNCHCHK(launch_op_finish_channels(lc(), (const float *)xd, 0, 1, tb.f, (const float *)win_d, Slx, (const cf *)Wf_d, hop,
                                                nframes, nsig, xf, stx));
            LAUNCHCHK(launch_csd_pair_finish(lc(), partial, rpp.groups, xf, nch, sided, scale / (double)nframes, pyy_d, pxy_d, st, stx,
                                             (const cf *)Wf_d, tb.f, tb.f + 4, nsig, nframes));
        } else {
            LAUNCHCHK(launch_csd_pair(lc(), (const float *)yd, nch, y_ld, (const float *)win_d, hop, nframes, tb.f + 4, detrend == 2,
                                      xf, Zx, partial, rpp));
            LAUNCHCHK(launch_csd_pair_finish(lc(), partial, rpp.groups, xf, nch, sided, scale / (double)nframes, pyy_d, pxy_d));
        }
        // Pxx: real-pair Welch PSD of x (its own small partial buffer after the channels' one)
        if (g.bigT.ensure(sizeof(float) * (size_t)rpx.groups * xf.L)) return -1;
        float *px = (float *)g.bigT.p;
        LAUNCHCHK(launch_welch_rp(lc(), (const float *)xd, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, px, rpx));
        LAUNCHCHK(launch_welch_finish(lc(), px, rpx.groups, xf, sided, scale / (double)nframes, pxx_d, 1));
    } else if (!cplx && !segmean && csd_rp_eligible(xf) && !env_flag("SP_NO_REALPAIR")) {
        // real x, y: x + i y_c in one transform per (frame, channel)
        LAUNCHCHK(launch_csd_rp(lc(), (const float *)xd, (const float *)yd, nch, y_ld, (const float *)win_d, hop, nframes,
                                tb.f, tb.f + 4, detrend == 2, xf, partial, rp));
        LAUNCHCHK(launch_csd_rp_finish(lc(), partial, rp.groups, xf, nch, sided, scale / (double)nframes, pxx_d, pyy_d,
                                       pxy_d));
    } else {
        LAUNCHCHK(launch_csd(lc(), xd, yd, cplx, nch, y_ld, (const float *)win_d, hop, nframes, tb.f, tb.f + 4,
                             detrend == 2, xf, partial, rp, segmean));
        LAUNCHCHK(launch_csd_finish(lc(), partial, rp.groups, xf, nch, sided, scale / (double)nframes, pxx_d, pyy_d,
                                    pxy_d));
    }
    return st.finish();
}

__global__ void k_set_trends(const double *__restrict__ means, float *__restrict__ trend, int nch) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nch) {
        trend[4 * c + 0] = (float)means[c];
        trend[4 * c + 1] = 0.f;
        trend[4 * c + 2] = 0.f;
        trend[4 * c + 3] = 0.f;
    }
}

static int csd_matrix_impl(const char *who, const float *x, int nch, int64_t nsig, int64_t x_ld, const float *win, int nfft,
                           int hop, int64_t nframes, int detrend, const double *means_host, double scale, double *g_out,
                           int mem) {
    // (the transposed contraction takes the pairs of 64-channel superblocks, nsb (nsb - 1) / 2 with nsb = ceil(nch / 64), as grid.y)
    if (nch > 23168) return fail("%s: nch = %d is beyond the limit of 23168 channels", who, nch);
    if (ensure_init()) return -1;
    if (check_frames(who, nsig, nfft, hop, nframes)) return -1;
    if (nch < 1 || x_ld < nsig) return fail("%s: bad nch / x_ld", who);
    if (detrend < 0 || detrend > 2) return fail("%s: detrend must be 0, 1 or 2", who);
    ApiLock lk;
    const bool lng = !wg_capable(nfft);          // segments longer than one workgroup transform: spectra by the long path
    Xf xf;
    xf.L = 0;
    xf.blue = true;
    if (!lng && get_xf(nfft, &xf)) return -1;
    const int nb = nfft / 2 + 1;
    const size_t gbytes = sizeof(double) * 2 * (size_t)nb * (size_t)nch * (size_t)nch;
    Stage st(mem);
    const float *xd;
    double *G;
    st.in(g.in0, x, sizeof(float) * (size_t)x_ld * (size_t)nch, &xd);
    st.out(g.cmG, g_out, gbytes, &G);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(2 * nch, &tb)) return -1;           // second half: trends re-based to the current frame chunk
    // (G is zeroed lazily, by the first chunk that adds into it directly: a call whose chunks all go through the packed spectra
    //  never needs it -- k_csdm_fold then stores, scales and mirrors in its one sweep)
    bool g_zeroed = false;
    // frames are processed in chunks so the two spectra buffers stay <= 8 GiB each (and float sums stay short)
    int64_t mc = ((int64_t)1 << 31) / ((int64_t)nch * nb);     // <= 16 GiB per spectra buffer
    if (mc > 16384) mc = 16384;
    mc = hook_cap("SP_CSDM_CHUNK_FRAMES", mc);
    if (mc < 32) mc = 32;
    mc &= ~(int64_t)31;
    {
        // equal chunks (a ragged last chunk of a few frames costs whole launches)
        const int64_t nchunks = (nframes + mc - 1) / mc;
        mc = (nframes + nchunks - 1) / nchunks;
        mc = (mc + 31) & ~(int64_t)31;
    }
    if (lng) {
        const int64_t lm = long_chunk_frames(nfft, nframes);
        if (mc > lm) mc = lm;
    }
    if (mc > nframes) mc = nframes;
    // contraction on the matrix cores: fused form reading the STFT output as it lies (default), or the form with a
    // transposed copy (more than 64 channels, or SP_CSDM_TRANSPOSED=1 for the tests)
    const bool use_fused = nch <= 64 && !env_flag("SP_CSDM_TRANSPOSED");   // off-diagonal superblocks need 128 accumulators
    const int nchp = (nch + 63) / 64 * 64;                       // MFMA layout: channels padded to whole 64-superblocks,
    const int64_t mcp = (mc + 31) / 32 * 32;                     // frames to a multiple of 32 (zero filled)
    // fused path: every (channel, frame) row of the spectra starts on a 128-byte line (row pitch padded to a multiple of 16
    // bins).  With the natural pitch nb = nfft/2 + 1 (odd) almost every 16-bin tile row straddled two lines and the
    // contraction fetched 1.9x its algorithmic bytes (calibrated PMC: profiles/r02_fetch_size_calibration.txt)
    const bool rp_stft = !lng && !xf.blue && xf.L >= 32 && nch <= 65535;
    // bf16-split contraction (k_csdm_bf16.hip): needs the pair-interleaved spectra the real-pair STFT kernel can write
    const bool use_bf16 = use_fused && rp_stft && !env_flag("SP_CSDM_FP32");
    // two bf16 pieces per operand (16 bits, k_csdm_bf16<4>: 10 MFMAs per two frame pairs instead of 16) from 1024 frame pairs
    // on: there the float32 accumulation bounds the accuracy of both forms alike (1.6e-6 of the peak at 2049 frames against
    // the float64 oracle) and the operand rounding (rms 2^-17/sqrt 3 per value, zero mean) averages to <= 2e-7.
    // SP_CSDM_SPLIT3=1: three pieces always
    const int split2 = env_flag("SP_CSDM_SPLIT3") ? 0 : ((nframes + 1) / 2 >= 1024 ? 1 : 0);
    const int ld = use_bf16 ? (nb + 7) / 8 * 8 : ((use_fused && (rp_stft || lng)) ? (nb + 15) / 16 * 16 : nb);
    const size_t sbytes = use_bf16 ? sizeof(cf) * 2 * (size_t)64 * (size_t)((mc + 1) / 2) * (size_t)ld       // 64 channel slots
                                   : sizeof(cf) * (size_t)nch * (size_t)mc * (size_t)ld;
    const size_t tbytes = sizeof(cf) * (size_t)nchp * (size_t)mcp * (use_fused ? 16 : (size_t)nb);
    if (g.cmS.ensure(sbytes) || g.cmT.ensure(tbytes)) return -1;
    cf *Xs = (cf *)g.cmS.p, *Xt = (cf *)g.cmT.p;
    // nfft 4096 at 50 % overlap: spectra by the pipeline of specialised waves (see below); m = frames of a chunk
    auto pipe_spec = [&](int64_t m) {
        const int64_t minp = 32;    // pairs per run
        return use_bf16 && nfft == 4096 && 2 * hop == nfft && detrend != 2 && (m + 1) / 2 >= minp * (int64_t)((g.ncu + nch - 1) / nch) &&
               welch_pipe_wanted(xf, hop, (int64_t)1 << 40) && !env_flag("SP_CSDM_NOPIPESPEC");
    };
    // mean detrend in ONE pass over the signals (single chunk): the spectra stage subtracts an estimate mu0 of every channel's
    // mean and leaves its block sums; the exact means and B_i = sum_g X_i,g follow from them (k_op_finish per channel) and the
    // matrix is corrected at the end (in k_csdm_fold).  Saves the separate pass over all samples for the means
    const bool cm_onepass = detrend == 1 && !means_host && nframes <= mc && pipe_spec(nframes) && !env_flag("SP_CSDM_TWOPASS");
    if (cm_onepass) {
        HIPCHK(hipMemsetAsync(tb.f, 0, sizeof(float) * 4 * (size_t)nch, g.stream));   // (the spectra stage estimates and publishes mu0)
    } else if (means_host) {
        // caller-supplied constants (detrend == SP_DETREND_CONST semantics)
        double *md = tb.d;
        HIPCHK(hipMemcpyAsync(md, means_host, sizeof(double) * (size_t)nch, hipMemcpyHostToDevice, g.stream));
        hipLaunchKernelGGL(k_set_trends, dim3((nch + 63) / 64), dim3(64), 0, g.stream, md, tb.f, nch);
    } else if (detrend == 0) {
        HIPCHK(hipMemsetAsync(tb.f, 0, sizeof(float) * 4 * (size_t)nch, g.stream));
    } else if (nch <= 512) {
        double *scr = moments_scratch();                 // all channels in one launch
        if (!scr) return -1;
        LAUNCHCHK(launch_moments(lc(), xd, false, nsig, detrend, scr, tb.d, tb.f, nch, x_ld));
    } else {
        for (int c = 0; c < nch; ++c)
            if (set_trend(tb, c, xd + (size_t)x_ld * (size_t)c, false, nsig, detrend, 0, 0)) return -1;
    }
    size_t op_sp = 0, op_sl = 0;
    int op_runs = 0;
    bool fold_pending = false;                            // packed-spectra path used: H (g.cmH) is folded into G at the end
    for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
        const int64_t m = nframes - f0 < mc ? nframes - f0 : mc;
        hipLaunchKernelGGL(k_trend_shift, dim3((nch + 63) / 64), dim3(64), 0, g.stream, tb.f, tb.f + 4 * nch, nch,
                           (double)f0 * (double)hop);
        if (lng) {
            // long segments: every channel's frames through pack -> batched long FFT, the rfft half of each row copied into Xs
            if (g.bigA.ensure(sizeof(cf) * (size_t)m * (size_t)nfft)) return -1;
            cf *S = (cf *)g.bigA.p;
            for (int c = 0; c < nch; ++c) {
                if (long_spectra(xd + (size_t)x_ld * (size_t)c, false, (const float *)win_d, nfft, hop, f0, m, tb.f + 4 * c,
                                 detrend == 2, 0, S, nullptr))
                    return -1;
                LAUNCHCHK(launch_long_stft_out(lc(), S, m, nfft, SP_SIDED_HALF, 1.f, 0, Xs + (size_t)c * (size_t)m * (size_t)ld, 0, ld));
            }
        } else if (pipe_spec(m)) {
            // nfft 4096 at 50 % overlap: the spectra stage is the pipeline of specialised waves (k_welch_pipe mode 5).  It writes
            // the PACKED pair spectra Z = X_2q + i X_2q+1 (all 4096 bins, two pairs side by side) and needs no mirror exchange;
            // the contraction runs on them as they are (H[k] = sum Z_i conj Z_j, same work: 4096 bins x pairs instead of 2049 x
            // frames) and the mirror combination G[k] = (H[k] + conj H[N-k]) / 2 is taken once at the end (k_csdm_fold)
            const int64_t pairs = (m + 1) / 2;
            const int runs = (g.ncu + nch - 1) / nch > 0 ? (g.ncu + nch - 1) / nch : 1;
            RunPart rp;
            rp.fpg = ((pairs + runs - 1) / runs + 1) & ~(int64_t)1;               // even: every run starts at an even pair
            rp.blocks = (int)((pairs + rp.fpg - 1) / rp.fpg);
            rp.groups = rp.blocks;
            const size_t zbytes = (size_t)128 * 64 * 512 * (size_t)((pairs + 1) / 2);
            const size_t hbytes = sizeof(double) * 2 * (size_t)nfft * (size_t)nch * (size_t)nch;
            if (g.cmS.ensure(zbytes) || g.cmH.ensure(hbytes)) return -1;
            Xs = (cf *)g.cmS.p;
            const int h_init = fold_pending ? 0 : 1;             // first chunk: H is initialised by the contraction itself
            fold_pending = true;
            cf *spartial = nullptr;
            if (cm_onepass) {
                // [channel][run][hop] block sums, then per channel Sl (2 hop doubles) and the finish state (5 nfft + 8 doubles)
                op_sp = sizeof(cf) * (size_t)nch * (size_t)rp.blocks * (size_t)hop;
                op_sl = sizeof(double) * 2 * (size_t)hop * (size_t)nch;
                if (g.cmO.ensure(op_sp + op_sl + sizeof(double) * (size_t)(5 * nfft + 8) * (size_t)nch)) return -1;
                spartial = (cf *)g.cmO.p;
                op_runs = rp.blocks;
            }
            LAUNCHCHK(launch_welch_pipe(lc(), xd + (size_t)f0 * (size_t)hop, false, (const float *)win_d, hop, m, tb.f + 4 * nch, xf,
                                        (float *)Xs, rp, spartial, 5, nch, x_ld, nfft / 8));
            LAUNCHCHK(launch_csdm_bf16(lc(), Xs, Xt, nch, pairs, nfft, (double *)g.cmH.p, nfft, split2, h_init));
            g.last_kernel = cm_onepass ? "k_welch_pipe(spectra,onepass)" : "k_welch_pipe(spectra)";
            continue;
        } else if (use_bf16) {
            const RunPart rp = run_partition_2d(xf.L, (m + 1) / 2, g.ncu, nch);
            LAUNCHCHK(launch_stft_rp(lc(), xd + (size_t)f0 * (size_t)hop, (const float *)win_d, hop, m, tb.f + 4 * nch,
                                     detrend == 2, xf, rp, SP_SIDED_HALF, 1.f, 2, Xs, nullptr, nch, x_ld,
                                     ((m + 1) / 2) * (int64_t)ld * 2, ld));
        } else if (rp_stft && (m >= 2 || ld != nb)) {
            // all channels in one grid, two real frames per transform
            // (channels x groups) workgroups: about 8 per CU in all, so that each amortises its twiddle prologue over a long
            // run of frame pairs (256 groups per channel = 16 pairs per workgroup paid ~9 % for it)
            const RunPart rp = run_partition_2d(xf.L, (m + 1) / 2, g.ncu, nch);
            LAUNCHCHK(launch_stft_rp(lc(), xd + (size_t)f0 * (size_t)hop, (const float *)win_d, hop, m, tb.f + 4 * nch,
                                     detrend == 2, xf, rp, SP_SIDED_HALF, 1.f, 0, Xs, nullptr, nch, x_ld,
                                     (int64_t)m * ld, ld));
        } else {
            const RunPart rp = run_partition(xf.L, m, g.ncu, 2);
            for (int c = 0; c < nch; ++c)
                LAUNCHCHK(launch_stft(lc(), xd + (size_t)x_ld * (size_t)c + (size_t)f0 * (size_t)hop, false,
                                      (const float *)win_d, hop, m, tb.f + 4 * (nch + c), detrend == 2, xf, rp, SP_SIDED_HALF,
                                      1.f, 0, Xs + (size_t)c * (size_t)m * (size_t)nb, nullptr));
        }
        if (!g_zeroed) {
            HIPCHK(hipMemsetAsync(G, 0, gbytes, g.stream));
            g_zeroed = true;
        }
        if (use_bf16) {
            LAUNCHCHK(launch_csdm_bf16(lc(), Xs, Xt, nch, m, nb, G, ld, split2));
        } else if (use_fused) {
            LAUNCHCHK(launch_csdm_fused(lc(), Xs, Xt, nch, m, nb, G, ld));
        } else {
            const int64_t mp = (m + 31) / 32 * 32;
            LAUNCHCHK(launch_csdm_transpose_kgc(lc(), Xs, Xt, nch, nchp, m, mp, nb));   // (this form: ld == nb)
            LAUNCHCHK(launch_csdm_mfma(lc(), Xt, nch, nchp, mp, nb, G));
        }
    }
    const double gscale = scale / (double)nframes;
    const int fold_init = (fold_pending && !g_zeroed) ? 1 : 0;          // nothing was added into G directly: the fold finishes G
    if (cm_onepass) {
        void *Wf_d;
        if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
        double *Sl = (double *)((char *)g.cmO.p + op_sp), *st = (double *)((char *)g.cmO.p + op_sp + op_sl);
        LAUNCHCHK(launch_cm_blocksums(lc(), (const cf *)g.cmO.p, nch, op_runs, hop, Sl));
        LAUNCHCHK(launch_op_finish_channels(lc(), xd, x_ld, nch, tb.f + 4 * nch, (const float *)win_d, Sl, (const cf *)Wf_d, hop,
                                            nframes, nsig, xf, st));
        LAUNCHCHK(launch_csdm_fold(lc(), (const double *)g.cmH.p, G, nch, nfft, st, (const cf *)Wf_d, tb.f + 4 * nch, nsig, nframes,
                                   gscale, fold_init));
    } else if (fold_pending) {
        LAUNCHCHK(launch_csdm_fold(lc(), (const double *)g.cmH.p, G, nch, nfft, nullptr, nullptr, nullptr, 0, 0, gscale, fold_init));
    }
    if (!fold_init) LAUNCHCHK(launch_csdm_finish(lc(), G, nch, nb, gscale));
    return st.finish();
}

int sp_csd_matrix(const float *x, int nch, int64_t nsig, int64_t x_ld, const float *win, int nfft, int hop,
                  int64_t nframes, int detrend, double scale, double *g_out, int mem) {
    return csd_matrix_impl("sp_csd_matrix", x, nch, nsig, x_ld, win, nfft, hop, nframes, detrend, nullptr, scale, g_out, mem);
}

int sp_csd_matrix_means(const float *x, int nch, int64_t nsig, int64_t x_ld, const float *win, int nfft, int hop,
                        int64_t nframes, const double *means, double scale, double *g_out, int mem) {
    if (!means) return fail("sp_csd_matrix_means: means is NULL");
    return csd_matrix_impl("sp_csd_matrix_means", x, nch, nsig, x_ld, win, nfft, hop, nframes, 0, means, scale, g_out, mem);
}

int sp_channel_means(const float *x, int nch, int64_t nsig, int64_t x_ld, double *means_out, int mem) {
    if (ensure_init()) return -1;
    if (nch < 1 || nch > 512 || nsig < 1 || x_ld < nsig) return fail("sp_channel_means: need 1 <= nch <= 512, 1 <= nsig <= x_ld");
    ApiLock lk;
    Stage st(mem);
    const float *xd;
    st.in(g.in0, x, sizeof(float) * (size_t)x_ld * (size_t)nch, &xd);
    if (st.commit()) return -1;
    TrendBuf tb;
    if (get_trendbuf(nch, &tb)) return -1;
    double *scr = moments_scratch();
    if (!scr) return -1;
    LAUNCHCHK(launch_moments(lc(), xd, false, nsig, 1, scr, tb.d, tb.f, nch, x_ld));
    // tb.d holds 8 doubles per channel, the mean first.  real difference: the means are gathered by one strided copy straight
    // into the caller's array, host or device, instead of through a staged piece
    HIPCHK(hipMemcpy2DAsync(means_out, sizeof(double), tb.d, sizeof(double) * 8, sizeof(double), (size_t)nch,
                            mem ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, g.stream));
    return st.finish();
}

int sp_stft(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
            int detrend, double mean_re, double mean_im, int sided, double amp_scale, int out_kind, int out_major,
            void *out, double *pseg_out, int mem) {
    if (out_major == 1 && nframes > (int64_t)65535 * 32)
        return fail("sp_stft: nframes = %lld is beyond the %lld frames the bin-major layout takes per call", (long long)nframes,
                    (long long)65535 * 32);
    if (ensure_init()) return -1;
    if (check_frames("sp_stft", nsig, nfft, hop, nframes)) return -1;
    if (sided < 1 || sided > 4) return fail("sp_stft: bad sided");
    if (detrend < 0 || detrend > 4) return fail("sp_stft: detrend must be 0..4");
    const int segmean = detrend == SP_DETREND_SEGMEAN ? 1 : (detrend == SP_DETREND_SEGLINEAR ? 2 : 0);   // per-window: generic kernel
    if (segmean) {
        detrend = SP_DETREND_CONST;
        mean_re = mean_im = 0.0;
    }
    ApiLock lk;
    const bool lng = !wg_capable(nfft);
    Xf xf;
    if (!lng && get_xf(nfft, &xf)) return -1;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    const size_t osz = out_kind ? 4 : 8;
    const size_t nb = (size_t)nbins_host(nfft, sided);
    const size_t obytes = osz * nb * (size_t)nframes;
    Stage st(mem);
    const void *xd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(1, &tb)) return -1;
    if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_re, mean_im)) return -1;
    void *fin;                           // final layout
    double *pseg_d;
    st.out(g.out0, out, obytes, &fin);
    st.out(g.out0, pseg_out, sizeof(double) * (size_t)nframes, &pseg_d);
    if (st.commit()) return -1;
    void *fm = fin;                      // frame-major result; bin-major needs a transpose into `fin`
    if (out_major == 1) {
        if (g.work.ensure(obytes)) return -1;
        fm = g.work.p;
    }
    if (pseg_d) HIPCHK(hipMemsetAsync(pseg_d, 0, sizeof(double) * (size_t)nframes, g.stream));
    const bool pair = !lng && !cplx && !segmean && !xf.blue && xf.L >= 32 && nframes >= 2 && !env_flag("SP_NO_REALPAIR");
    if (lng) {
        const int64_t mc = long_chunk_frames(nfft, nframes);
        if (g.bigA.ensure(sizeof(cf) * (size_t)mc * (size_t)nfft)) return -1;
        cf *S = (cf *)g.bigA.p;
        for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
            const int64_t m = nframes - f0 < mc ? nframes - f0 : mc;
            if (long_spectra(xd, cplx, (const float *)win_d, nfft, hop, f0, m, tb.f, detrend == 2, segmean, S, pseg_d)) return -1;
            LAUNCHCHK(launch_long_stft_out(lc(), S, m, nfft, sided, (float)amp_scale, out_kind, fm, f0, (int)nb));
        }
    } else if (pair) {
        const RunPart rp = run_partition(xf.L, (nframes + 1) / 2, g.ncu,
                                         stft_rp_groups_per_cu(xf, detrend == 2, hop, sided, out_kind, pseg_d != nullptr));
        LAUNCHCHK(launch_stft_rp(lc(), (const float *)xd, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, rp, sided,
                                 (float)amp_scale, out_kind, fm, pseg_d));
    } else {
        const RunPart rp = run_partition(xf.L, nframes, g.ncu);
        LAUNCHCHK(launch_stft(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, rp, sided,
                              (float)amp_scale, out_kind, fm, pseg_d, segmean));
    }
    if (out_major == 1) LAUNCHCHK(launch_transpose(lc(), fm, fin, nframes, (int64_t)nb, (int)osz));
    return st.finish();
}

int sp_stft_cog(const void *x, int x_dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                int detrend, double mean_re, double mean_im, double fs, double fmin, double fmax, double *cog_out, int mem) {
    if (ensure_init()) return -1;
    if (check_frames("sp_stft_cog", nsig, nfft, hop, nframes)) return -1;
    if (detrend < 0 || detrend > 4) return fail("sp_stft_cog: detrend must be 0..4");
    if (!(fs > 0.0) || fmin < 0.0 || fmax < fmin) return fail("sp_stft_cog: need fs > 0 and 0 <= fmin <= fmax");
    const int segmean = detrend == SP_DETREND_SEGMEAN ? 1 : (detrend == SP_DETREND_SEGLINEAR ? 2 : 0);
    if (segmean) {
        detrend = SP_DETREND_CONST;
        mean_re = mean_im = 0.0;
    }
    ApiLock lk;
    const bool lng = !wg_capable(nfft);
    Xf xf;
    if (!lng && get_xf(nfft, &xf)) return -1;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    Stage st(mem);
    const void *xd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(1, &tb)) return -1;
    // band in bins of df = fs/nfft: klo = ceil(fmin/df), khi = floor(fmax/df), with a relative guard against a frequency
    // that is a bin centre up to rounding
    const double df = fs / (double)nfft;
    const double eps = 1e-9;
    const int klo = (int)std::ceil(fmin / df - eps);
    const double kh = std::floor(fmax / df + eps);
    const int khi = kh > (double)nfft ? nfft : (int)kh;
    const int wpf = lng ? 1 : (xf.L / 16 >= 64 ? xf.L / 16 / 64 : 1);   // waves per frame: one (num, den) slot each
    // mean detrend in ONE pass (pipeline mode 8) when the window's spectrum is confined to a few bins: per-frame results cannot be
    // corrected afterwards in general, but |X - d W|^2 differs from |X|^2 only where W is non-zero -- 3 bins for Hann.  The
    // kernel keeps those bins of every frame and k_cog_finish_op corrects the moments with the exact mean.  SP_COG_TWOPASS=1:
    // the separate pass for the mean (0.35 of 0.79 ms at 2^28 complex64 samples)
    const bool cog_pipe = !lng && !segmean && detrend != 2 && klo <= 0 && khi >= nfft / 2 && !env_flag("SP_COG_GENERIC") &&
                          welch_pipe_wanted(xf, hop, nframes);
    CogLobe lobe_w{};
    const bool cog_op = cog_pipe && detrend == SP_DETREND_MEAN && xf.L == 4096 && (hop == 2048 || hop == 1024) &&
                        !env_flag("SP_COG_TWOPASS") && cog_window_lobe(win, nfft, &lobe_w);
    if (cog_op) {
        HIPCHK(hipMemsetAsync(tb.f, 0, sizeof(float) * 4, g.stream));            // (the kernel publishes its estimate here)
    } else if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_re, mean_im)) {
        return -1;
    }
    const size_t abytes = sizeof(cf) * (size_t)wpf * (size_t)nframes + (cog_op ? sizeof(cf) * 8 * (size_t)nframes : 0);
    if (g.work.ensure(abytes)) return -1;
    cf *acc = (cf *)g.work.p;
    double *fin;
    st.out(g.out0, cog_out, sizeof(double) * (size_t)nframes, &fin);
    if (st.commit()) return -1;
    if (lng) {
        const int64_t mc = long_chunk_frames(nfft, nframes);
        if (g.bigA.ensure(sizeof(cf) * (size_t)mc * (size_t)nfft)) return -1;
        cf *S = (cf *)g.bigA.p;
        for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
            const int64_t m = nframes - f0 < mc ? nframes - f0 : mc;
            if (long_spectra(xd, cplx, (const float *)win_d, nfft, hop, f0, m, tb.f, detrend == 2, segmean, S, nullptr)) return -1;
            LAUNCHCHK(launch_long_cog(lc(), S, m, nfft, klo, khi, acc, f0));
        }
    } else {
        const bool pipe = cog_pipe;
        const RunPart rp = pipe ? run_partition(xf.L, nframes, g.ncu, 1) : run_partition(xf.L, nframes, g.ncu);
        // streaming form (every sample read once, the overlap carried in registers) when the shape allows; SP_COG_GENERIC=1
        // forces the generic frame kernel (A/B test); nfft 4096: the pipeline of specialised waves (k_welch_pipe.hip, mode 2)
        int generic = 1;
        if (cog_op) {
            // (Sl: 2 hop doubles; k_op_finish also reads nfft doubles through its unused A argument, hence the larger of the two)
            const size_t b_sp = sizeof(cf) * (size_t)rp.groups * (size_t)hop, b_sl = sizeof(double) * (size_t)(2 * hop > nfft ? 2 * hop : nfft);
            if (g.cmO.ensure(b_sp + b_sl + sizeof(double) * (size_t)(5 * nfft + 8))) return -1;
            cf *spartial = (cf *)g.cmO.p;
            double *Sl = (double *)((char *)g.cmO.p + b_sp), *ops = (double *)((char *)g.cmO.p + b_sp + b_sl);
            void *Wf_d;
            if (get_window_spectrum(win, nfft, xf, &Wf_d)) return -1;
            LAUNCHCHK(launch_welch_pipe(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, xf, (float *)acc, rp, spartial, 2));
            g.last_kernel = "k_welch_pipe(cog,onepass)";
            LAUNCHCHK(launch_cm_blocksums(lc(), spartial, 1, (int)rp.groups, hop, Sl));
            LAUNCHCHK(launch_op_finish_channels(lc(), xd, 0, 1, tb.f, (const float *)win_d, Sl, (const cf *)Wf_d, hop, nframes, nsig, xf,
                                                ops, cplx));
            LAUNCHCHK(launch_cog_finish_op(lc(), acc, wpf, nframes, df, fin, acc + (size_t)wpf * (size_t)nframes, lobe_w, ops, tb.f, nsig,
                                           nfft));
            return st.finish();
        }
        if (pipe) {
            LAUNCHCHK(launch_welch_pipe(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, xf, (float *)acc, rp, nullptr, 2));
            g.last_kernel = "k_welch_pipe(cog)";
            generic = 0;
        } else if (!segmean && detrend != 2 && !env_flag("SP_COG_GENERIC"))
            generic = launch_cog_carry(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, xf, acc, rp, klo, khi);
        if (generic < 0) return fail("sp_stft_cog: launch failed");
        if (generic)
            LAUNCHCHK(launch_stft(lc(), xd, cplx, (const float *)win_d, hop, nframes, tb.f, detrend == 2, xf, rp, 2, 1.f, 1, nullptr,
                                  nullptr, segmean, acc, klo, khi));
    }
    LAUNCHCHK(launch_cog_finish(lc(), acc, wpf, nframes, df, fin));
    return st.finish();
}

int sp_bispectrum(const void *x, const void *y, const void *z, int x_dtype, int64_t nsig, const float *win, int nfft, int hop,
                  int64_t nframes, int detrend, double mean_re, double mean_im, void *B_out, double *b2_out, double *pzz_out,
                  int mem) {
    if (ensure_init()) return -1;
    if (nfft < 8 || nfft > 4096 || !wg_capable(nfft)) return fail("sp_bispectrum: nfft %d outside 8 .. 4096", nfft);
    if (check_frames("sp_bispectrum", nsig, nfft, hop, nframes)) return -1;
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("sp_bispectrum: unknown dtype %d", x_dtype);
    if (detrend < SP_DETREND_CONST || detrend > SP_DETREND_LINEAR) return fail("sp_bispectrum: detrend must be 0, 1 or 2");
    if (!x || !B_out || !b2_out) return fail("sp_bispectrum: x, B_out and b2_out are required");
    ApiLock lk;
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const bool sym = y == nullptr && z == nullptr;       // auto bispectrum: one spectrum, j <= i tiles, mirrored
    const int nsp = sym ? 1 : 3;
    const int nb = cplx ? nfft : nfft / 2 + 1, c0 = cplx ? nfft / 2 : 0;
    const int sided = cplx ? SP_SIDED_TWO : SP_SIDED_HALF;
    const size_t esz = cplx ? 8 : 4;
    const void *src[3] = {x, y ? y : x, z ? z : x};
    const void *xd[3];
    Stage st(mem);
    for (int k = 0; k < nsp; ++k) st.in(g.bsIn, src[k], esz * (size_t)nsig, &xd[k]);
    if (st.commit()) return -1;
    if (sym) xd[1] = xd[2] = xd[0];
    // the tiles that meet the valid region (j <= i for the auto case) and the map (ti, tj) -> tile number (-1: none)
    const int T = bispec_tile_dim(), ntd = (nb + T - 1) / T;
    std::vector<int> tbl((size_t)ntd * ntd, -1);        // [tmap | tile list as int2]
    std::vector<int> tl;
    for (int ti = 0; ti < ntd; ++ti)
        for (int tj = 0; tj < (sym ? ti + 1 : ntd); ++tj) {
            const int imax = std::min(ti * T + T, nb) - 1, jmax = std::min(tj * T + T, nb) - 1;
            if (ti * T + tj * T - c0 > nb - 1 || imax + jmax - c0 < 0) continue;
            tbl[(size_t)ti * ntd + tj] = (int)tl.size() / 2;
            tl.push_back(ti);
            tl.push_back(tj);
        }
    const int ntiles = (int)tl.size() / 2;
    const size_t nmap = tbl.size() + (tbl.size() & 1);   // the int2 list starts 8-byte aligned
    tbl.resize(nmap, -1);
    tbl.insert(tbl.end(), tl.begin(), tl.end());
    void *tab_d;
    if (get_table(6, tbl.data(), sizeof(int) * tbl.size(), &tab_d, nullptr)) return -1;
    const int *tmap_d = (const int *)tab_d;
    const int2 *tiles_d = (const int2 *)((const int *)tab_d + nmap);
    // frames in chunks of whole 256-frame partial chunks: the spectra and the partials stay within SP_BISPEC_MIB MiB each
    // (default 256; a test hook like those of launch.h, read on every call)
    const int64_t FC = bispec_frame_chunk();
    const size_t budget = (size_t)std::max(1, env_int("SP_BISPEC_MIB", 256)) << 20;
    const size_t part_bytes = sizeof(float) * bispec_part_floats() * (size_t)ntiles;   // per partial chunk
    const size_t spec_bytes = sizeof(cf) * (size_t)nb * (size_t)nsp * (size_t)FC;      // per partial chunk
    int64_t cpc = (int64_t)std::min(budget / spec_bytes, budget / part_bytes);
    cpc = std::max<int64_t>(1, std::min<int64_t>(cpc, 4096));
    const int64_t mc = std::min(nframes, cpc * FC);
    const int64_t nfc = (mc + FC - 1) / FC;
    if (g.bsS.ensure(sizeof(cf) * (size_t)nb * (size_t)nsp * (size_t)mc) || g.bsP.ensure(part_bytes * (size_t)nfc) ||
        g.bsA.ensure(sizeof(double) * (bispec_part_floats() * (size_t)ntiles + (size_t)nb * (size_t)(nfc + 1))))
        return -1;
    cf *S[3];
    for (int k = 0; k < 3; ++k) S[k] = (cf *)g.bsS.p + (size_t)nb * (size_t)mc * (size_t)(sym ? 0 : k);
    float *part = (float *)g.bsP.p;
    double *acc = (double *)g.bsA.p, *p64 = acc + bispec_part_floats() * (size_t)ntiles, *ppart = p64 + nb;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(6, &tb)) return -1;                  // records 0 .. 2: the signals' trends; 3 .. 5: shifted to a chunk
    for (int k = 0; k < nsp; ++k)
        if (set_trend(tb, k, xd[k], cplx, nsig, detrend, mean_re, mean_im)) return -1;
    for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
        const int64_t m = std::min(mc, nframes - f0);
        LAUNCHCHK(launch_bispec_trend_shift(lc(), tb.f, tb.f + 12, nsp, f0 * (int64_t)hop));
        const RunPart rp = run_partition(xf.L, m, g.ncu);
        for (int k = 0; k < nsp; ++k)
            LAUNCHCHK(launch_stft(lc(), (const char *)xd[k] + esz * (size_t)(f0 * hop), cplx, (const float *)win_d, hop, m,
                                  tb.f + 12 + 4 * k, detrend == SP_DETREND_LINEAR, xf, rp, sided, 1.f, 0, S[k], nullptr));
        {
            ProfScope ps;
            LAUNCHCHK(launch_bispec_tile(lc(), S[0], S[1], S[2], nb, c0, m, tiles_d, ntiles, part));
        }
        LAUNCHCHK(launch_bispec_pzz(lc(), S[2], nb, m, ppart));
        LAUNCHCHK(launch_bispec_reduce(lc(), part, ppart, ntiles, m, nb, f0 == 0, acc, p64));
    }
    void *Bd;
    double *b2d, *pzd;
    const size_t nn = (size_t)nb * (size_t)nb;
    st.out(g.out0, B_out, 2 * sizeof(double) * nn, &Bd);
    st.out(g.out0, b2_out, sizeof(double) * nn, &b2d);
    st.out(g.out0, pzz_out, sizeof(double) * (size_t)nb, &pzd);
    if (st.commit()) return -1;
    LAUNCHCHK(launch_bispec_finish(lc(), acc, p64, tmap_d, ntd, nb, c0, sym ? 1 : 0, nframes, Bd, b2d, pzd));
    return st.finish();
}

int sp_multitaper(const void *x, const void *y, int dtype, int64_t nsig, const float *tapers, int ntapers, int nfft, int hop,
                  int64_t nframes, int detrend, const double *mean_x, const double *mean_y, const double *weights, double scale,
                  double *pxx, double *pyy, double *pxy, double *skx, double *sky, int mem) {
    // every refusal comes before the device is touched
    if (ntapers < 1 || ntapers > SP_MTAPER_MAXK) return fail("sp_multitaper: %d tapers, need 1 .. %d", ntapers, SP_MTAPER_MAXK);
    if (nfft < 8 || !wg_capable(nfft))
        return fail("sp_multitaper: nfft %d outside one workgroup transform (8 .. %d for powers of two, .. %d otherwise)", nfft,
                    SP_MAX_WG_FFT, SP_MAX_WG_FFT / 2);
    if (check_frames("sp_multitaper", nsig, nfft, hop, nframes)) return -1;
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_multitaper: unknown dtype %d", dtype);
    if (detrend < SP_DETREND_CONST || detrend > SP_DETREND_LINEAR) return fail("sp_multitaper: detrend must be 0, 1 or 2");
    const bool cross = y != nullptr, eigen = weights != nullptr;
    if (!x || !tapers || !pxx || (cross && (!pyy || !pxy))) return fail("sp_multitaper: x, tapers and the weighted outputs are required");
    if (eigen && (!skx || (cross && !sky))) return fail("sp_multitaper: weights are given, so the eigenspectra outputs are required");
    double wsum = 0.0;
    if (eigen) {
        for (int k = 0; k < ntapers; ++k) {
            if (!(weights[k] >= 0.0) || !isfinite(weights[k])) return fail("sp_multitaper: weight %d is negative or not finite", k);
            wsum += weights[k];
        }
        if (!(wsum > 0.0)) return fail("sp_multitaper: the weights are all zero");
    }
    if (ensure_init()) return -1;
    ApiLock lk;
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    const bool cplx = dtype == SP_DTYPE_C64, lin = detrend == SP_DETREND_LINEAR;
    const size_t esz = cplx ? 8 : 4;
    const int sided = cplx ? SP_SIDED_RAW : SP_SIDED_HALF;
    const size_t nb = (size_t)nbins_host(nfft, sided), K = (size_t)ntapers;
    Stage st(mem);
    const void *xd, *yd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * (size_t)nsig, &yd);
    if (st.commit()) return -1;
    void *tap_d;
    if (get_table(8, tapers, sizeof(float) * K * (size_t)nfft, &tap_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(2, &tb)) return -1;
    if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_x ? mean_x[0] : 0, mean_x ? mean_x[1] : 0)) return -1;
    if (cross && set_trend(tb, 1, yd, cplx, nsig, detrend, mean_y ? mean_y[0] : 0, mean_y ? mean_y[1] : 0)) return -1;
    // the outputs the call's form has; the others are not written, whatever the caller passed
    double *pxx_d, *pyy_d, *pxy_d, *skx_d, *sky_d;
    st.out(g.out0, pxx, sizeof(double) * nb, &pxx_d);
    st.out(g.out0, cross ? pyy : nullptr, sizeof(double) * nb, &pyy_d);
    st.out(g.out0, cross ? pxy : nullptr, sizeof(double) * 2 * nb, &pxy_d);
    st.out(g.out0, eigen ? skx : nullptr, sizeof(double) * K * nb, &skx_d);
    st.out(g.out0, eigen && cross ? sky : nullptr, sizeof(double) * K * nb, &sky_d);
    if (st.commit()) return -1;
    // the PSD of a real record transforms PAIRS of frames; the eigenspectra run one taper per grid row
    const bool pair = !cross && !cplx;
    const int64_t nunits = pair ? (nframes + 1) / 2 : nframes;
    const int nblocks = eigen ? ntapers : 1, ktap = eigen ? 1 : ntapers;
    const RunPart rp = eigen ? run_partition_2d(xf.L, nunits, g.ncu, nblocks) : run_partition(xf.L, nunits, g.ncu);
    const size_t planes = (size_t)mtaper_partial_planes(xf, cplx, cross), blk = (size_t)rp.groups * planes * (size_t)xf.L;
    if (g.work.ensure(sizeof(float) * blk * (size_t)nblocks)) return -1;
    float *partial = (float *)g.work.p;
    {
        ProfScope ps;
        LAUNCHCHK(launch_mtaper(lc(), xd, cross ? yd : nullptr, cplx, (const float *)tap_d, nblocks, ktap, hop, nframes, tb.f, lin, xf,
                                partial, rp));
        g.last_kernel = "k_mtaper";
    }
    const double sc = scale / (double)nframes;
    double *sxy_d = nullptr;
    if (eigen && cross) {
        if (g.mtS.ensure(sizeof(double) * 2 * K * nb)) return -1;
        sxy_d = (double *)g.mtS.p;
    }
    for (int b = 0; b < nblocks; ++b) {
        const float *pb = partial + blk * (size_t)b;
        double *oxx = eigen ? skx_d + nb * (size_t)b : pxx_d, *oyy = eigen ? sky_d + nb * (size_t)b : pyy_d;
        double *oxy = eigen ? sxy_d + 2 * nb * (size_t)b : pxy_d;
        if (!cross) LAUNCHCHK(launch_welch_finish(lc(), pb, rp.groups, xf, sided, sc, oxx, pair ? 1 : 0));
        else if (planes == 3) LAUNCHCHK(launch_csd_rp_finish(lc(), pb, rp.groups, xf, 1, sided, sc, oxx, oyy, oxy));
        else LAUNCHCHK(launch_csd_finish(lc(), pb, rp.groups, xf, 1, sided, sc, oxx, oyy, oxy));
    }
    if (eigen) {
        double cn[SP_MTAPER_MAXK];
        for (int k = 0; k < ntapers; ++k) cn[k] = weights[k] / wsum;
        LAUNCHCHK(launch_mtaper_combine(lc(), skx_d, ntapers, (int64_t)nb, cn, pxx_d));
        if (cross) {
            LAUNCHCHK(launch_mtaper_combine(lc(), sky_d, ntapers, (int64_t)nb, cn, pyy_d));
            LAUNCHCHK(launch_mtaper_combine(lc(), sxy_d, ntapers, (int64_t)(2 * nb), cn, pxy_d));
        }
    }
    return st.finish();
}

int sp_czt_chirp(int64_t i0, int64_t count, double step, double start, float *cs_out) {
    if (count < 0 || (count > 0 && !cs_out)) return fail("sp_czt_chirp: count must not be negative and cs_out is required");
    if (!isfinite(start) || !isfinite(step)) return fail("sp_czt_chirp: start and step must be finite");
    if (count > 0 && i0 > INT64_MAX - count) return fail("sp_czt_chirp: the index range overflows");
    czt_chirp_host(i0, count, step, start, cs_out);
    return 0;
}

int sp_czt(const void *x, int x_dtype, int64_t n, int64_t x_ld, int64_t batch, int64_t m, double start, double step, void *out,
           int mem) {
    // every refusal comes before the device is touched
    if (czt_check("sp_czt", n, m, start, step)) return -1;
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("sp_czt: unknown dtype %d", x_dtype);
    if (batch < 0 || x_ld < n) return fail("sp_czt: need batch >= 0 and a row stride x_ld >= n");
    if (batch == 0) return 0;
    if (!x || !out) return fail("sp_czt: x and out are required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4, in_elems = (size_t)((batch - 1) * x_ld + n), obytes = sizeof(cf) * (size_t)batch * (size_t)m;
    Stage st(mem);
    const void *xd;
    cf *od;
    st.in(g.in0, x, esz * in_elems, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    CztTab t;
    if (get_czt(n, m, start, step, &t)) return -1;
    if (t.L <= SP_MAX_WG_FFT) {
        CztTables tb{nullptr, t.pre, t.post, t.bf, (int)n, (int)m};
        if (get_twiddles(t.L, &tb.tw)) return -1;
        ProfScope ps;
        LAUNCHCHK(launch_czt_rows(lc(), xd, cplx, x_ld, batch, (int)t.L, tb, od));
        g.last_kernel = "k_czt_rows";
    } else {
        int64_t slice = (int64_t)(SP_LONG_SLICE_BYTES / (sizeof(cf) * (size_t)t.L));
        if (slice < 1) slice = 1;
        if (slice > 32768) slice = 32768;
        slice = hook_cap("SP_LONG_SLICE_ROWS", slice);
        if (slice > batch) slice = batch;
        note_slices((batch + slice - 1) / slice);
        if (g.blueA.ensure(sizeof(cf) * (size_t)t.L * (size_t)slice)) return -1;
        cf *A = (cf *)g.blueA.p;
        for (int64_t b0 = 0; b0 < batch; b0 += slice) {
            const int64_t rows = batch - b0 < slice ? batch - b0 : slice;
            if (czt_long_rows(xd, cplx, x_ld, b0, rows, nullptr, nullptr, false, t, n, A)) return -1;
            LAUNCHCHK(launch_czt_post(lc(), A, t.L, rows, t.post, m, 1.f, b0, od));
        }
    }
    return st.finish();
}

// ---- digital down-converter (k_ddc.hip) -----------------------------------------------------------
#define SP_DDC_MAX_INDEX ((int64_t)1 << 40)
#define SP_DDC_MAX_NSIG ((int64_t)1 << 32)
// the refusals of sp_ddc, before the device is touched
static int ddc_check(const char *who, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, double nu, int64_t n0, int q, int ntaps) {
    if (q < 1 || q > SP_DDC_MAXQ) return fail("%s: the decimation q = %d must lie in 1 .. %d", who, q, SP_DDC_MAXQ);
    if (ntaps < 1 || ntaps > SP_DDC_MAXTAPS || ntaps % 2 == 0)
        return fail("%s: ntaps = %d must be odd and lie in 1 .. %d", who, ntaps, SP_DDC_MAXTAPS);
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("%s: unknown dtype %d", who, x_dtype);
    if (nsig < 1 || nsig > SP_DDC_MAX_NSIG) return fail("%s: nsig = %lld must lie in 1 .. 2^32 samples per launch", who, (long long)nsig);
    if (batch < 0 || x_ld < nsig) return fail("%s: need batch >= 0 and a row stride x_ld >= nsig", who);
    if (!isfinite(nu)) return fail("%s: nu must be finite", who);
    if (n0 > SP_DDC_MAX_INDEX || n0 < -SP_DDC_MAX_INDEX) return fail("%s: n0 = %lld must lie within +-2^40", who, (long long)n0);
    return 0;
}

int sp_ddc_tile(int q) {
    if (q < 1 || q > SP_DDC_MAXQ) return 0;
    return ddc_geom(q, 1).K;
}

int sp_ddc(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, double nu, int64_t n0, int q, const float *h,
           int ntaps, void *out, int mem) {
    if (ddc_check("sp_ddc", x_dtype, nsig, x_ld, batch, nu, n0, q, ntaps)) return -1;
    if (batch == 0) return 0;
    if (!x || !h || !out) return fail("sp_ddc: x, h and out are required");
    for (int j = 0; j < ntaps; ++j)
        if (!isfinite(h[j])) return fail("sp_ddc: the taps must be finite");
    const DdcGeom geom = ddc_geom(q, ntaps);
    const int64_t nout = (nsig + q - 1) / q;
    if ((nout + geom.K - 1) / geom.K * batch > INT_MAX) return fail("sp_ddc: %lld rows of %lld outputs are too many tiles for one launch",
                                                                   (long long)batch, (long long)nout);
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4, in_elems = (size_t)((batch - 1) * x_ld + nsig), obytes = sizeof(cf) * (size_t)batch * (size_t)nout;
    Stage st(mem);
    const void *xd;
    cf *od;
    st.in(g.in0, x, esz * in_elems, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    // the taps, one row per polyphase component, reversed: taps[s][p] = h[(PP - 1 - p) q + s]
    std::vector<float> tp((size_t)q * geom.PP, 0.f);
    for (int s = 0; s < q; ++s)
        for (int p = 0; p < geom.PP; ++p) {
            const int j = (geom.PP - 1 - p) * q + s;
            if (j < ntaps) tp[(size_t)s * geom.PP + p] = h[j];
        }
    void *taps_d = nullptr;
    if (get_table(10, tp.data(), sizeof(float) * tp.size(), &taps_d, nullptr)) return -1;
    // the oscillator: nu n0 modulo one turn in 128-bit fixed point, the step rounded to 2^-64 turns (over the <= 2^32 samples of a
    // launch that is <= 2^-33 turns), and the float32 table exp(-2 pi i nu j) over the staged span of a tile
    const u128 A = frac128(nu);
    const uint64_t ph0 = (uint64_t)((A * (u128)(__int128)n0) >> 64);
    const uint64_t dnu = (uint64_t)((A + ((u128)1 << 63)) >> 64);
    void *tab_d = nullptr;
    if (A != 0) {
        struct {
            double nu;
            int64_t W;
        } key = {nu, geom.W};
        bool fresh = false;
        if (get_table_keyed(9, &key, sizeof key, nullptr, sizeof(cf) * (size_t)geom.W, &tab_d, &fresh)) return -1;
        if (fresh) {
            std::vector<cf> tab((size_t)geom.W);
            czt_chirp_host(0, geom.W, 0.0, nu, (float *)tab.data());
            HIPCHK(hipMemcpy(tab_d, tab.data(), sizeof(cf) * (size_t)geom.W, hipMemcpyHostToDevice));
        }
    }
    {
        ProfScope ps;
        if (launch_ddc(lc(), xd, cplx, x_ld, nsig, batch, geom, ph0, dnu, (const cf *)tab_d, (const float *)taps_d,
                       ((uintptr_t)xd & 15) == 0, od) != 0)
            return fail("sp_ddc: the launch was refused (q = %d, ntaps = %d, %zu bytes of LDS)", q, ntaps, geom.lds);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_ddc";
    }
    return st.finish();
}

// ---- rational resampler (k_upfirdn.hip) ------------------------------------------------------------
static bool upf_admits(int up, int down, int ntaps) {
    return up >= 1 && up <= SP_UPF_MAXF && down >= 1 && down <= SP_UPF_MAXF && ntaps >= 1 && ntaps <= SP_UPF_MAXTAPS;
}

int sp_upfirdn_tile(int up, int down, int ntaps, int cplx) {
    if (!upf_admits(up, down, ntaps)) return 0;
    const UpfGeom geom = upf_geom(up, down, ntaps, cplx != 0);
    return geom.lds <= SP_LDS_MAX ? geom.K : 0;
}

int sp_upfirdn(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, const float *h, int ntaps, int up, int down,
               int64_t m0, int64_t nout, void *out, int mem) {
    // every refusal comes before the device is touched
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("sp_upfirdn: unknown dtype %d", x_dtype);
    if (!upf_admits(up, down, ntaps))
        return fail("sp_upfirdn: need up and down in 1 .. %d and ntaps in 1 .. %d, got up = %d, down = %d, ntaps = %d", SP_UPF_MAXF,
                    SP_UPF_MAXTAPS, up, down, ntaps);
    if (nsig < 1 || batch < 0 || x_ld < nsig) return fail("sp_upfirdn: need nsig >= 1, batch >= 0 and a row stride x_ld >= nsig");
    if (m0 < 0 || nout < 0) return fail("sp_upfirdn: m0 = %lld and nout = %lld must not be negative", (long long)m0, (long long)nout);
    const int64_t mmax = ((int64_t)1 << 62) / down;
    if (m0 >= mmax || nout >= mmax - m0)
        return fail("sp_upfirdn: (m0 + nout) down must stay below 2^62 (m0 = %lld, nout = %lld, down = %d)", (long long)m0,
                    (long long)nout, down);
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const UpfGeom geom = upf_geom(up, down, ntaps, cplx);
    if (geom.lds > SP_LDS_MAX)
        return fail("sp_upfirdn: up = %d, down = %d, ntaps = %d need %zu bytes of LDS", up, down, ntaps, geom.lds);
    if (batch > 0 && (nout + geom.K - 1) / geom.K > INT_MAX / batch)
        return fail("sp_upfirdn: %lld rows of %lld outputs are too many tiles for one launch", (long long)batch, (long long)nout);
    if (nout == 0 || batch == 0) return 0;
    if (!x || !h || !out) return fail("sp_upfirdn: x, h and out are required");
    for (int j = 0; j < ntaps; ++j)
        if (!isfinite(h[j])) return fail("sp_upfirdn: the taps must be finite");
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t esz = cplx ? 8 : 4, in_elems = (size_t)((batch - 1) * x_ld + nsig), obytes = esz * (size_t)batch * (size_t)nout;
    Stage st(mem);
    const void *xd;
    void *od;
    st.in(g.in0, x, esz * in_elems, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    // the taps, one row per phase: taps[phi][p] = h[phi + p up]
    std::vector<float> tp((size_t)up * geom.pitch, 0.f);
    for (int j = 0; j < ntaps; ++j) tp[(size_t)(j % up) * geom.pitch + j / up] = h[j];
    void *taps_d = nullptr;
    if (get_table(14, tp.data(), sizeof(float) * tp.size(), &taps_d, nullptr)) return -1;
    {
        ProfScope ps;
        if (launch_upfirdn(lc(), xd, cplx, x_ld, nsig, batch, geom, (const float *)taps_d, ((uintptr_t)xd & 15) == 0, m0, nout, od) != 0)
            return fail("sp_upfirdn: the launch was refused (up = %d, down = %d, ntaps = %d, %zu bytes of LDS)", up, down, ntaps,
                        geom.lds);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_upfirdn";
    }
    return st.finish();
}

// ---- polyphase filter-bank channelizer (k_pfb.hip) ------------------------------------------------
int sp_pfb(const void *x, int x_dtype, int64_t nsig, int64_t x_ld, int64_t batch, const float *h, int ntaps, int M, int hop,
           int64_t first, int64_t nframes, int phase_ref, int r0, int out_kind, int out_major, double scale, void *out, int mem) {
    // every refusal comes before the device is touched
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("sp_pfb: unknown dtype %d", x_dtype);
    if (M < 2 || M > SP_MAX_WG_FFT || !is_pow2(M))
        return fail("sp_pfb: M = %d must be a power of two from 2 to %d", M, SP_MAX_WG_FFT);
    if (ntaps < M || ntaps % M != 0 || ntaps / M > SP_PFB_MAXP)
        return fail("sp_pfb: ntaps = %d must be P M with 1 <= P <= %d (M = %d)", ntaps, SP_PFB_MAXP, M);
    if (hop < 1) return fail("sp_pfb: hop = %d must be at least 1", hop);
    if (nframes < 1) return fail("sp_pfb: nframes = %lld must be at least 1", (long long)nframes);
    if (phase_ref != 0 && phase_ref != 1) return fail("sp_pfb: phase_ref must be 0 (frame) or 1 (time)");
    if (r0 < 0 || r0 >= M) return fail("sp_pfb: r0 = %d must lie in 0 .. M - 1", r0);
    if (out_kind != 0 && out_kind != 1) return fail("sp_pfb: out_kind must be 0 (frames) or 1 (accumulated power)");
    if (out_major != 0 && out_major != 1) return fail("sp_pfb: out_major must be 0 or 1");
    if (!isfinite(scale)) return fail("sp_pfb: scale must be finite");
    if (nsig < 1 || batch < 0 || x_ld < nsig) return fail("sp_pfb: need nsig >= 1, batch >= 0 and a row stride x_ld >= nsig");
    // every frame touches the row: the first ends inside it or later, the last starts inside it or earlier
    if (first <= -(int64_t)ntaps || first >= nsig || nframes - 1 > (nsig - 1 - first) / hop)
        return fail("sp_pfb: frames 0 .. %lld from first = %lld at hop %d do not all touch the %lld samples of the row",
                    (long long)(nframes - 1), (long long)first, hop, (long long)nsig);
    const int fpw = fpw_of(M);
    if (batch > 0 && (nframes + fpw - 1) / fpw > INT_MAX / batch)
        return fail("sp_pfb: %lld rows of %lld frames are too many workgroups for one launch", (long long)batch, (long long)nframes);
    if (out_kind == 0 && out_major == 1 && nframes > (int64_t)65535 * 32)
        return fail("sp_pfb: the bin-major layout takes at most %lld frames per launch", (long long)65535 * 32);
    if (batch == 0) return 0;
    if (!x || !h || !out) return fail("sp_pfb: x, h and out are required");
    for (int j = 0; j < ntaps; ++j)
        if (!isfinite(h[j])) return fail("sp_pfb: the taps must be finite");
    if (ensure_init()) return -1;
    ApiLock lk;
    Xf xf;
    if (get_xf(M, &xf)) return -1;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const int P = ntaps / M, nb = cplx ? M : M / 2 + 1;
    const size_t esz = cplx ? 8 : 4, in_elems = (size_t)((batch - 1) * x_ld + nsig);
    const size_t obytes = (out_kind ? sizeof(double) : sizeof(cf) * (size_t)nframes) * (size_t)nb * (size_t)batch;
    Stage st(mem);
    const void *xd;
    void *od;
    st.in(g.in0, x, esz * in_elems, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    void *taps_d = nullptr;
    if (get_table(11, h, sizeof(float) * (size_t)ntaps, &taps_d, nullptr)) return -1;
    // the run partition of one row (SP_PFB_FPG: a test hook like those of launch.h, read on every call; any value >= 1 is valid)
    RunPart rp = run_partition_2d(M, nframes, g.ncu, (int)(batch < INT_MAX ? batch : INT_MAX));
    {
        const int64_t f = env_int("SP_PFB_FPG", 0);
        if (f >= 1) {
            const int64_t G = (nframes + f - 1) / f;
            rp.fpg = f;
            rp.blocks = (int)((G + fpw - 1) / fpw);
            rp.groups = (int64_t)rp.blocks * fpw;
        }
    }
    void *kout = od;                     // what the kernel writes: frame-major frames, or the groups' partial sums
    if (out_kind == 1) {
        if (g.work.ensure(sizeof(float) * (size_t)batch * (size_t)rp.groups * (size_t)M)) return -1;
        kout = g.work.p;
    } else if (out_major == 1) {
        if (g.work.ensure(obytes)) return -1;
        kout = g.work.p;
    }
    {
        ProfScope ps;
        if (launch_pfb(lc(), xd, cplx, x_ld, nsig, batch, (const float *)taps_d, P, hop, first, nframes, phase_ref, r0, xf, rp, out_kind,
                       out_kind ? nullptr : kout, out_kind ? (float *)kout : nullptr) != 0)
            return fail("sp_pfb: the launch was refused (M = %d, P = %d, %lld rows)", M, P, (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_pfb";
    }
    if (out_kind == 1) {
        LAUNCHCHK(launch_pfb_finish(lc(), (const float *)kout, rp.groups, M, nb, batch, scale / (double)nframes, (double *)od));
    } else if (out_major == 1) {
        const size_t row = sizeof(cf) * (size_t)nframes * (size_t)nb;
        for (int64_t b = 0; b < batch; ++b)
            LAUNCHCHK(launch_transpose(lc(), (const char *)kout + (size_t)b * row, (char *)od + (size_t)b * row, nframes, (int64_t)nb,
                                       (int)sizeof(cf)));
    }
    return st.finish();
}

// ---- polyphase synthesis bank (k_pfb_synth.hip) -----------------------------------------------------
// the default route and run length of one call (host arithmetic; ncu = the device's CU count).  The route is the composed path at
// every shape: measured (profiles/pfb_synth_bench.txt, M = 1024 / 4096, P = 4 / 8) the fused kernel takes 2.3 - 3.3 x the composed
// time where all its rings fit and 2.2 - 6.9 x where only some do, so it runs only when SP_PFBS_PATH=fused asks for it
// runs: about 4 groups per CU, and long enough that the halo frames a run transforms without writing stay <= 1/16 of it
namespace {
struct PfbsPlan {
    int groups, fpw, halo;     // groups of a workgroup that fit a ring (0: none), groups per workgroup, halo frames of a fused run
    bool fused;                // the default route
    int64_t fpg;               // frames per run on the fused path
};
PfbsPlan pfbs_plan(int M, int ntaps, bool cplx, int hop, int64_t nframes, int64_t batch, int ncu) {
    PfbsPlan p;
    p.fpw = fpw_of(M);
    p.groups = pfb_synth_groups(M, ntaps, cplx, nullptr);
    p.fused = false;
    p.halo = (ntaps + hop - 1) / hop - 1;
    const int64_t target = std::max<int64_t>(1, (int64_t)ncu * 4 * std::max(p.groups, 1) / std::max<int64_t>(batch, 1));
    p.fpg = std::max<int64_t>(1, std::max((nframes + target - 1) / target, std::min<int64_t>(16 * (int64_t)p.halo, nframes)));
    return p;
}
}   // namespace

int sp_pfb_synth_plan(int sided, int64_t batch, int64_t nframes, int ntaps, int M, int hop, int64_t *out) {
    if (sided != SP_SIDED_HALF && sided != SP_SIDED_RAW) return fail("sp_pfb_synth_plan: sided must be SP_SIDED_HALF or SP_SIDED_RAW");
    if (M < 2 || M > SP_MAX_WG_FFT || !is_pow2(M) || ntaps < M || ntaps % M != 0 || ntaps / M > SP_PFB_MAXP || hop < 1 || nframes < 1 ||
        batch < 1 || !out)
        return fail("sp_pfb_synth_plan: a shape sp_pfb_synth refuses, or out is NULL");
    if (ensure_init()) return -1;
    const PfbsPlan p = pfbs_plan(M, ntaps, sided == SP_SIDED_RAW, hop, nframes, batch, g.ncu);
    out[0] = p.fused ? 1 : 0;
    out[1] = p.groups;
    out[2] = p.fpw;
    out[3] = p.fpg;
    out[4] = p.halo;
    return 0;
}

int sp_pfb_synth(const void *X, int sided, int in_major, int64_t batch, int64_t nframes, const float *gt, int ntaps, int M, int hop,
                 int64_t first, int phase_ref, int r0, double scale, int64_t nout, void *y, int mem) {
    // every refusal comes before the device is touched
    if (sided != SP_SIDED_HALF && sided != SP_SIDED_RAW) return fail("sp_pfb_synth: sided must be SP_SIDED_HALF or SP_SIDED_RAW");
    if (in_major != 0 && in_major != 1) return fail("sp_pfb_synth: in_major must be 0 or 1");
    if (M < 2 || M > SP_MAX_WG_FFT || !is_pow2(M))
        return fail("sp_pfb_synth: M = %d must be a power of two from 2 to %d", M, SP_MAX_WG_FFT);
    if (ntaps < M || ntaps % M != 0 || ntaps / M > SP_PFB_MAXP)
        return fail("sp_pfb_synth: ntaps = %d must be P M with 1 <= P <= %d (M = %d)", ntaps, SP_PFB_MAXP, M);
    if (hop < 1) return fail("sp_pfb_synth: hop = %d must be at least 1", hop);
    if (nframes < 1) return fail("sp_pfb_synth: nframes = %lld must be at least 1", (long long)nframes);
    if (nout < 1) return fail("sp_pfb_synth: nout = %lld must be at least 1", (long long)nout);
    if (batch < 0) return fail("sp_pfb_synth: batch = %lld must not be negative", (long long)batch);
    if (phase_ref != 0 && phase_ref != 1) return fail("sp_pfb_synth: phase_ref must be 0 (frame) or 1 (time)");
    if (r0 < 0 || r0 >= M) return fail("sp_pfb_synth: r0 = %d must lie in 0 .. M - 1", r0);
    if (!isfinite(scale)) return fail("sp_pfb_synth: scale must be finite");
    const int64_t lim = (int64_t)1 << 40;
    if (first > lim || first < -lim || nframes > lim / hop || nout > lim)
        return fail("sp_pfb_synth: first = %lld, nframes * hop = %lld * %d and nout = %lld must stay within 2^40", (long long)first,
                    (long long)nframes, hop, (long long)nout);
    if (!X || !gt || !y) return fail("sp_pfb_synth: X, g and y are required");
    // tap = float32(g scale / M), rounded once
    std::vector<float> tap((size_t)ntaps);
    for (int j = 0; j < ntaps; ++j) {
        if (!isfinite(gt[j])) return fail("sp_pfb_synth: the taps must be finite");
        tap[(size_t)j] = (float)((double)gt[j] * scale / (double)M);
        if (!isfinite(tap[(size_t)j])) return fail("sp_pfb_synth: tap %d times scale / M is beyond float32", j);
    }
    // the path (SP_PFBS_PATH: a test hook like those of launch.h, read on every call): by default the rule of pfbs_plan
    const bool cplx = sided == SP_SIDED_RAW;
    const int fpw = fpw_of(M), ag = pfb_synth_groups(M, ntaps, cplx, nullptr);
    bool fused = pfbs_plan(M, ntaps, cplx, hop, nframes, batch, 1).fused;
    if (const char *pv = getenv("SP_PFBS_PATH")) {
        if (!strcmp(pv, "fused")) {
            if (ag < 1)
                return fail("sp_pfb_synth: SP_PFBS_PATH=fused, but one ring of %d %s accumulators behind the %d-point exchange image "
                            "is beyond the %zu bytes of LDS a workgroup may take", ntaps, cplx ? "complex" : "real", M, SP_LDS_MAX);
            fused = true;
        } else if (!strcmp(pv, "composed")) {
            fused = false;
        } else if (pv[0]) {
            return fail("sp_pfb_synth: SP_PFBS_PATH must be fused or composed, got '%s'", pv);
        }
    }
    const int gpw = fused ? ag : fpw;                      // groups of a workgroup that own frames
    if (batch > 0 && (nframes + gpw - 1) / gpw > INT_MAX / batch)
        return fail("sp_pfb_synth: %lld rows of %lld frames are too many workgroups for one launch", (long long)batch,
                    (long long)nframes);
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    Xf xf;
    if (get_xf(M, &xf)) return -1;
    const int P = ntaps / M, nb = cplx ? M : M / 2 + 1;
    const size_t xbytes = sizeof(cf) * (size_t)nb * (size_t)nframes * (size_t)batch;
    const size_t esz = cplx ? sizeof(cf) : sizeof(float), ybytes = esz * (size_t)nout * (size_t)batch;
    Stage st(mem);
    const cf *xd;
    void *yd;
    st.in(g.in0, X, xbytes, &xd);
    st.out(g.out0, y, ybytes, &yd);
    if (st.commit()) return -1;
    void *taps_d = nullptr;
    if (get_table(12, tap.data(), sizeof(float) * (size_t)ntaps, &taps_d, nullptr)) return -1;
    if (in_major == 1) {                 // bin-major frames [row][nb][nframes]: transposed per row into scratch, as sp_pfb writes them
        if (g.bigA.ensure(xbytes)) return -1;
        const size_t rowb = sizeof(cf) * (size_t)nframes * (size_t)nb;
        for (int64_t b = 0; b < batch; ++b)
            LAUNCHCHK(launch_transpose(lc(), (const char *)xd + (size_t)b * rowb, (char *)g.bigA.p + (size_t)b * rowb, (int64_t)nb, nframes,
                                       (int)sizeof(cf)));
        xd = (const cf *)g.bigA.p;
    }
    if (fused) {
        // the run length of pfbs_plan (SP_PFBS_FPG: a test hook, read on every call; any value >= 1 is valid, also below the halo)
        const PfbsPlan pl = pfbs_plan(M, ntaps, cplx, hop, nframes, batch, g.ncu);
        const int halo = pl.halo;
        int64_t f = env_int("SP_PFBS_FPG", 0);
        if (f < 1) f = pl.fpg;
        ProfScope ps;
        if (launch_pfb_synth(lc(), xd, cplx, batch, nframes, (const float *)taps_d, P, hop, first, phase_ref, r0, xf, f, halo, true, nout,
                             yd, nullptr) != 0)
            return fail("sp_pfb_synth: the fused launch was refused (M = %d, P = %d, %lld rows)", M, P, (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_pfb_synth(fused)";
    } else {
        if (g.work.ensure(esz * (size_t)M * (size_t)nframes * (size_t)batch)) return -1;
        RunPart rp = run_partition_2d(M, nframes, g.ncu, (int)(batch < INT_MAX ? batch : INT_MAX));
        const int64_t fe = env_int("SP_PFBS_FPG", 0);
        if (fe >= 1) rp.fpg = fe;
        ProfScope ps;
        if (launch_pfb_synth(lc(), xd, cplx, batch, nframes, (const float *)taps_d, P, hop, first, phase_ref, r0, xf, rp.fpg, 0, false, nout,
                             nullptr, g.work.p) != 0)
            return fail("sp_pfb_synth: the launch was refused (M = %d, P = %d, %lld rows)", M, P, (long long)batch);
        HIPCHK(hipGetLastError());
        LAUNCHCHK(launch_pfb_synth_gather(lc(), g.work.p, cplx, batch, nframes, (const float *)taps_d, ntaps, M, hop, first, phase_ref, r0,
                                          nout, yd));
        g.last_kernel = "k_pfb_synth(composed)";
    }
    return st.finish();
}

int sp_zoom_welch(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes,
                  int detrend, const double *mean_x, const double *mean_y, int64_t m, double start, double step, double scale,
                  double *pxx, double *pyy, double *pxy, void *frames, int mem) {
    // every refusal comes before the device is touched
    if (czt_check("sp_zoom_welch", nfft, m, start, step)) return -1;
    if (hop < 1) return fail("sp_zoom_welch: hop must be at least 1");
    if (nframes < 1) return fail("sp_zoom_welch: nframes must be at least 1");
    if ((nframes - 1) * (int64_t)hop + nfft > nsig)
        return fail("sp_zoom_welch: %lld frames of %d with hop %d need %lld samples, signal has %lld", (long long)nframes, nfft, hop,
                    (long long)((nframes - 1) * (int64_t)hop + nfft), (long long)nsig);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_zoom_welch: unknown dtype %d", dtype);
    if (detrend < SP_DETREND_CONST || detrend > SP_DETREND_LINEAR) return fail("sp_zoom_welch: detrend must be 0, 1 or 2");
    const bool cross = y != nullptr, stft = frames != nullptr;
    if (!x || !win) return fail("sp_zoom_welch: x and win are required");
    if (stft && cross) return fail("sp_zoom_welch: the frames output takes one signal");
    if (!stft && (!pxx || (cross && (!pyy || !pxy)))) return fail("sp_zoom_welch: an output is required: frames, pxx, or pxx, pyy and pxy");
    if (!isfinite(scale)) return fail("sp_zoom_welch: scale must be finite");
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64, lin = detrend == SP_DETREND_LINEAR;
    const size_t esz = cplx ? 8 : 4, mm = (size_t)m;
    Stage st(mem);
    const void *xd, *yd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * (size_t)nsig, &yd);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(2, &tb)) return -1;
    if (set_trend(tb, 0, xd, cplx, nsig, detrend, mean_x ? mean_x[0] : 0, mean_x ? mean_x[1] : 0)) return -1;
    if (cross && set_trend(tb, 1, yd, cplx, nsig, detrend, mean_y ? mean_y[0] : 0, mean_y ? mean_y[1] : 0)) return -1;
    CztTab t;
    if (get_czt(nfft, m, start, step, &t)) return -1;
    // the outputs the call's form has: the frames, or pxx, or pxx, pyy and pxy
    double *pxx_d, *pyy_d, *pxy_d;
    cf *fr_d;
    st.out(g.out0, frames, sizeof(cf) * (size_t)nframes * mm, &fr_d);
    st.out(g.out0, stft ? nullptr : pxx, sizeof(double) * mm, &pxx_d);
    st.out(g.out0, !stft && cross ? pyy : nullptr, sizeof(double) * mm, &pyy_d);
    st.out(g.out0, !stft && cross ? pxy : nullptr, sizeof(double) * 2 * mm, &pxy_d);
    if (st.commit()) return -1;
    const double sc = scale / (double)nframes;
    if (t.L <= SP_MAX_WG_FFT) {
        CztTables ct{nullptr, t.pre, t.post, t.bf, nfft, (int)m};
        if (get_twiddles(t.L, &ct.tw)) return -1;
        const RunPart rp = run_partition((int)t.L, nframes, g.ncu);
        float *partial = nullptr;
        if (!stft) {
            if (g.work.ensure(sizeof(float) * (size_t)rp.groups * (cross ? 4 : 1) * (size_t)t.L)) return -1;
            partial = (float *)g.work.p;
        }
        {
            ProfScope ps;
            LAUNCHCHK(launch_zoom(lc(), xd, cross ? yd : nullptr, cplx, (const float *)win_d, hop, nframes, tb.f, lin, (int)t.L, ct, rp,
                                  (float)scale, partial, stft ? fr_d : nullptr));
            g.last_kernel = "k_zoom";
        }
        if (!stft) {
            Xf fx;                       // the finish kernels read rows of L floats and keep the first m bins
            fx.L = (int)t.L;
            fx.blue = true;
            fx.tb = XfTables{ct.tw, nullptr, nullptr, (int)m};
            if (!cross) LAUNCHCHK(launch_welch_finish(lc(), partial, rp.groups, fx, SP_SIDED_RAW, sc, pxx_d, 0));
            else LAUNCHCHK(launch_csd_finish(lc(), partial, rp.groups, fx, 1, SP_SIDED_RAW, sc, pxx_d, pyy_d, pxy_d));
        }
    } else {
        // chunks of frames, as long_spectra: pre-multiply straight from the signal, the multi-pass transforms, then one kernel adds
        // the chunk's products of the first m bins into float64 sums in frame order
        const int64_t mc = long_chunk_frames((int)t.L, nframes);
        if (g.bigA.ensure(sizeof(cf) * (size_t)mc * (size_t)t.L) || (cross && g.bigB.ensure(sizeof(cf) * (size_t)mc * (size_t)t.L)))
            return -1;
        cf *Sx = (cf *)g.bigA.p, *Sy = cross ? (cf *)g.bigB.p : nullptr;
        double *acc = nullptr;
        if (!stft) {
            if (g_cztAcc.ensure(sizeof(double) * 4 * mm)) return -1;
            acc = (double *)g_cztAcc.p;
            HIPCHK(hipMemsetAsync(acc, 0, sizeof(double) * 4 * mm, g.stream));
        }
        for (int64_t f0 = 0; f0 < nframes; f0 += mc, ++g_passes[0]) {
            const int64_t rows = nframes - f0 < mc ? nframes - f0 : mc;
            if (czt_long_rows(xd, cplx, hop, f0, rows, (const float *)win_d, tb.f, lin, t, nfft, Sx)) return -1;
            if (cross && czt_long_rows(yd, cplx, hop, f0, rows, (const float *)win_d, tb.f + 4, lin, t, nfft, Sy)) return -1;
            if (stft) LAUNCHCHK(launch_czt_post(lc(), Sx, t.L, rows, t.post, m, (float)scale, f0, fr_d));
            else LAUNCHCHK(launch_zoom_acc(lc(), Sx, Sy, rows, t.L, m, acc));
        }
        if (!stft) LAUNCHCHK(launch_zoom_acc_out(lc(), acc, m, sc, pxx_d, pyy_d, pxy_d));
    }
    return st.finish();
}

// ---- short-time cross-correlation (k_xcorr_frames.hip) -------------------------------------------
int sp_xcorr_frames_len(int nw, int maxlag) {
    if (nw < 2 || maxlag < 0 || maxlag > nw - 1) return -1;
    const int64_t L = next_pow2((int64_t)nw + maxlag);
    if (L > SP_MAX_WG_FFT) return -1;
    return L < 32 ? 32 : (int)L;
}

int sp_xcorr_frames(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nw, int hop, int64_t nframes,
                    int maxlag, int detrend, int norm, double beta, const float *weight, void *frames, double *avg, float *peak,
                    int mem) {
    // every refusal comes before the device is touched
    if (nw < 2) return fail("sp_xcorr_frames: the window needs at least 2 samples, got %d", nw);
    if (maxlag < 0 || maxlag > nw - 1) return fail("sp_xcorr_frames: maxlag %d outside 0 .. nw - 1 = %d", maxlag, nw - 1);
    const int L = sp_xcorr_frames_len(nw, maxlag);
    if (L < 0)
        return fail("sp_xcorr_frames: nw + maxlag = %lld is beyond one workgroup transform (%d points)", (long long)nw + maxlag,
                    SP_MAX_WG_FFT);
    if (hop < 1) return fail("sp_xcorr_frames: hop must be at least 1");
    if (nframes < 1) return fail("sp_xcorr_frames: nframes must be at least 1");
    if (nsig < nw || (nframes - 1) > (nsig - nw) / hop)
        return fail("sp_xcorr_frames: %lld frames of %d with hop %d overrun the record of %lld samples", (long long)nframes, nw, hop,
                    (long long)nsig);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_xcorr_frames: unknown dtype %d", dtype);
    if (detrend != SP_DETREND_CONST && detrend != SP_DETREND_SEGMEAN)
        return fail("sp_xcorr_frames: detrend must be SP_DETREND_CONST or SP_DETREND_SEGMEAN, got %d", detrend);
    if (norm != SP_XC_RAW && norm != SP_XC_COEFF) return fail("sp_xcorr_frames: unknown norm %d", norm);
    if (!(beta >= 0.0) || !isfinite(beta)) return fail("sp_xcorr_frames: beta must be finite and not negative");
    if (beta > 0.0 && norm != SP_XC_COEFF) return fail("sp_xcorr_frames: beta > 0 (PHAT) takes norm SP_XC_COEFF");
    if (!x || !y) return fail("sp_xcorr_frames: x and y are required");
    if (!frames && !avg && !peak) return fail("sp_xcorr_frames: an output is required: frames, avg or peak");
    if (weight && dtype == SP_DTYPE_F32) {               // a real pair keeps Re(IFFT): the weights must be even, W[k] == W[L - k]
        for (int k = 1; k < L - k; ++k)
            if (!(weight[k] == weight[L - k])) return fail("sp_xcorr_frames: the weight of a real pair must be even, W[%d] != W[%d]", k, L - k);
    }
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4, lsz = cplx ? sizeof(cf) : sizeof(float), nl = 2 * (size_t)maxlag + 1;
    Stage st(mem);
    const void *xd, *yd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * (size_t)nsig, &yd);
    if (st.commit()) return -1;
    void *win_d = nullptr, *wt_d = nullptr;
    if (win && get_table(1, win, sizeof(float) * (size_t)nw, &win_d, nullptr)) return -1;
    if (weight && get_table(13, weight, sizeof(float) * (size_t)L, &wt_d, nullptr)) return -1;
    const cf *tw;
    if (get_twiddles(L, &tw)) return -1;
    void *fr_d;
    double *avg_d;
    float *pk_d;
    st.out(g.out0, frames, lsz * (size_t)nframes * nl, &fr_d);
    st.out(g.out0, avg, sizeof(double) * (cplx ? 2 : 1) * nl, &avg_d);
    st.out(g.out0, peak, sizeof(float) * 2 * (size_t)nframes, &pk_d);
    if (st.commit()) return -1;
    RunPart rp = run_partition(L, nframes, g.ncu);
    if (const int fpg = env_int("SP_XCF_FPG", 0); fpg > 0) {           // test hook: runs of this many frames
        const int fpw = fpw_of(L);
        rp.fpg = fpg;
        rp.blocks = (int)(((nframes + fpg - 1) / fpg + fpw - 1) / fpw);
        rp.groups = (int64_t)rp.blocks * fpw;
    }
    void *partial = nullptr;
    if (avg) {
        if (g.work.ensure(lsz * (size_t)rp.groups * (size_t)L)) return -1;
        partial = g.work.p;
    }
    const XcfArgs a{xd, yd, (const float *)win_d, (const float *)wt_d, nw, hop, maxlag, detrend == SP_DETREND_SEGMEAN ? 1 : 0,
                    norm == SP_XC_COEFF ? 1 : 0, (float)beta, nframes};
    {
        ProfScope ps;
        LAUNCHCHK(launch_xcorr_frames(lc(), a, cplx, L, tw, rp, fr_d, partial, pk_d));
        g.last_kernel = "k_xcorr_frames";
    }
    if (avg) LAUNCHCHK(launch_xcorr_frames_finish(lc(), partial, cplx, rp.groups, L, maxlag, nframes, avg_d));
    return st.finish();
}

// ---- two-point wavenumber-frequency spectrum S(k, f) (k_skf.hip) --------------------------------
static bool skf_shape_ok(int nfft, int nk) {
    return nfft >= 32 && nfft <= SP_SKF_MAX_L && is_pow2(nfft) && nk >= 2 && nk <= SP_SKF_MAX_NK;
}

int sp_skf_plan(int cplx, int nfft, int nb, int nk, int64_t *out) {
    if (!skf_shape_ok(nfft, nk) || !out) return -1;
    if (!band_in_transform(cplx != 0, nfft, 0, nb)) return -1;
    const SkfPlan p = skf_plan_of(cplx != 0, nfft, nb, nk, env_int("SP_SKF_CELLS", 0));
    out[0] = p.tiles;
    out[1] = p.tile_bins;
    out[2] = (int64_t)p.lds_bytes;
    out[3] = (int64_t)p.tiles * (cplx ? 2 : 1);
    return 0;
}

int sp_skf(const void *x, const void *y, int dtype, int64_t nsig, const float *win, int nfft, int hop, int64_t nframes, int detrend,
           int power, int b0, int nb, int nk, double scale, double *s_out, int mem) {
    // every refusal comes before the device is touched
    if (nfft < 32 || nfft > SP_SKF_MAX_L || !is_pow2(nfft))
        return fail("sp_skf: nfft = %d must be a power of two from 32 to %d", nfft, SP_SKF_MAX_L);
    if (nk < 2 || nk > SP_SKF_MAX_NK) return fail("sp_skf: nk = %d outside 2 .. %d", nk, SP_SKF_MAX_NK);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_skf: dtype must be float32 or complex64, got %d", dtype);
    const bool cplx = dtype == SP_DTYPE_C64;
    if (nb < 1) return fail("sp_skf: the band needs at least one bin, got nb = %d", nb);
    if (!band_in_transform(cplx, nfft, b0, nb))
        return fail("sp_skf: the band of %d bins from %d lies outside the %d bins of the spectrum", nb, b0, cplx ? nfft : nfft / 2 + 1);
    if (hop < 1) return fail("sp_skf: hop must be at least 1");
    if (nframes < 1) return fail("sp_skf: nframes must be at least 1");
    if (nsig < nfft || (nframes - 1) > (nsig - nfft) / hop)
        return fail("sp_skf: %lld frames of %d with hop %d overrun the record of %lld samples", (long long)nframes, nfft, hop,
                    (long long)nsig);
    if (detrend != SP_DETREND_NONE && detrend != SP_DETREND_SEGMEAN)
        return fail("sp_skf: detrend must be SP_DETREND_NONE or SP_DETREND_SEGMEAN, got %d", detrend);
    if (power != SP_SKF_MEAN && power != SP_SKF_CROSS) return fail("sp_skf: unknown power %d", power);
    if (!isfinite(scale)) return fail("sp_skf: scale must be finite");
    if (!x || !y || !s_out) return fail("sp_skf: x, y and s_out are required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t esz = cplx ? 8 : 4;
    Stage st(mem);
    const void *xd, *yd;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * (size_t)nsig, &yd);
    if (st.commit()) return -1;
    void *win_d = nullptr;
    if (win && get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    const cf *tw;
    if (get_twiddles(nfft, &tw)) return -1;
    const SkfPlan pl = skf_plan_of(cplx, nfft, nb, nk, env_int("SP_SKF_CELLS", 0));
    // runs: about four workgroups per CU over runs x tiles, as few more as keeps the partials within 64 MiB; a run is whole rounds
    const int fpw = fpw_of(nfft);
    const int64_t cells = (int64_t)nb * nk;
    int64_t want = (int64_t)g.ncu * 4 / pl.tiles, room = ((int64_t)64 << 20) / (4 * cells);
    if (want > room) want = room;
    if (want < 1) want = 1;
    int64_t fpr = ((nframes + want - 1) / want + fpw - 1) / fpw * fpw;
    if (const int v = env_int("SP_SKF_FPG", 0); v > 0) fpr = v;            // test hook: runs of this many frames
    const int64_t runs = (nframes + fpr - 1) / fpr;
    if (g.work.ensure(sizeof(float) * (size_t)runs * (size_t)cells)) return -1;
    double *out_d;
    st.out(g.out0, s_out, sizeof(double) * (size_t)cells, &out_d);
    if (st.commit()) return -1;
    const SkfArgs a{xd, yd, (const float *)win_d, hop, detrend == SP_DETREND_SEGMEAN ? 1 : 0, power == SP_SKF_CROSS ? 1 : 0, b0, nb, nk,
                    pl.tile_bins, pl.stride, nframes, fpr};
    {
        ProfScope ps;
        LAUNCHCHK(launch_skf(lc(), a, cplx, nfft, tw, runs, pl, (float *)g.work.p));
        g.last_kernel = "k_skf";
    }
    LAUNCHCHK(launch_skf_finish(lc(), (const float *)g.work.p, runs, nb, nk, scale / (double)nframes, out_d));
    return st.finish();
}

// ---- time-resolved Welch spectra (k_welch_blocks.hip) ---------------------------------------------
// the shape checks sp_welch_blocks and its plan share; 0 or the message's tail
static const char *welch_blocks_shape(int nfft, int hop, int64_t nframes, int navg, int step) {
    if (nfft < 32 || nfft > SP_MAX_WG_FFT || !is_pow2(nfft)) return "nfft must be a power of two from 32 to 8192";
    if (hop < 1 || hop > nfft) return "hop must lie in 1 .. nfft";
    if (navg < 1) return "navg must be at least 1";
    if (step < 1) return "step must be at least 1";
    if (nframes < navg) return "nframes must be at least navg";
    if (nframes > ((int64_t)1 << 40) / hop) return "nframes: too many frames";
    return nullptr;
}

int sp_welch_blocks_plan(int cplx, int nfft, int hop, int64_t nframes, int navg, int step, int nch, int64_t out[8]) {
    if (welch_blocks_shape(nfft, hop, nframes, navg, step) || nch < 0 || nch > 65535 || !out) return -1;
    const WelchBlocksPlan p = welch_blocks_plan_of(cplx != 0, nfft, nframes, navg, step, nch, g.ncu);
    out[0] = p.nblocks;
    out[1] = p.nb;
    out[2] = p.q;
    out[3] = p.runs;
    // every record of every pair has its own transform; twice where the bins are split over two workgroups
    out[4] = p.runs * p.q * (nch < 1 ? 1 : 2 * (int64_t)nch) * welch_blocks_bin_split(cplx != 0, nch >= 1, nfft);
    out[5] = (int64_t)p.scratch_bytes;
    out[6] = p.wgs;
    out[7] = (int64_t)p.lds_bytes;
    return 0;
}

int sp_welch_blocks(const void *x, const void *y, int dtype, int64_t nsig, int nch, int64_t y_ld, const float *win, int nfft, int hop,
                    int64_t nframes, int navg, int step, int detrend, double scale, int doubled, float *pxx, float *pyy, void *pxy,
                    int mem) {
    // every refusal comes before the device is touched
    if (const char *why = welch_blocks_shape(nfft, hop, nframes, navg, step))
        return fail("sp_welch_blocks: %s (nfft %d, hop %d, nframes %lld, navg %d, step %d)", why, nfft, hop, (long long)nframes, navg,
                    step);
    if (nsig < nfft || (nframes - 1) > (nsig - nfft) / hop)
        return fail("sp_welch_blocks: nsig = %lld is shorter than the %lld frames of %d with hop %d", (long long)nsig, (long long)nframes,
                    nfft, hop);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_welch_blocks: dtype must be float32 or complex64, got %d", dtype);
    if (y && (nch < 1 || nch > 65535)) return fail("sp_welch_blocks: nch = %d outside 1 .. 65535", nch);
    if (y && y_ld < nsig) return fail("sp_welch_blocks: y_ld = %lld is below nsig = %lld", (long long)y_ld, (long long)nsig);
    if (detrend != SP_DETREND_NONE && detrend != SP_DETREND_SEGMEAN)
        return fail("sp_welch_blocks: detrend must be SP_DETREND_NONE or SP_DETREND_SEGMEAN, got %d", detrend);
    if (!isfinite(scale)) return fail("sp_welch_blocks: scale must be finite");
    if (!x) return fail("sp_welch_blocks: x is required");
    if (!pxx) return fail("sp_welch_blocks: pxx is required");
    if (y && !pyy) return fail("sp_welch_blocks: pyy is required when y is given");
    if (y && !pxy) return fail("sp_welch_blocks: pxy is required when y is given");
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64, dbl = !cplx && doubled != 0;
    const int pairs = y ? nch : 1;
    const WelchBlocksPlan pl = welch_blocks_plan_of(cplx, nfft, nframes, navg, step, y ? nch : 0, g.ncu);
    const size_t esz = cplx ? 8 : 4, cells = (size_t)pl.nblocks * (size_t)pl.nb;
    const size_t xxb = sizeof(float) * cells, yyb = y ? sizeof(float) * cells * (size_t)nch : 0, xyb = 2 * yyb;
    Stage st(mem);
    const void *xd, *yd;
    float *pxx_d, *pyy_d;
    cf *pxy_d;
    st.in(g.in0, x, esz * (size_t)nsig, &xd);
    st.in(g.in1, y, esz * ((size_t)(pairs - 1) * (size_t)y_ld + (size_t)nsig), &yd);
    st.out(g.out0, pxx, xxb, &pxx_d);
    st.out(g.out0, y ? pyy : nullptr, yyb, &pyy_d);
    st.out(g.out0, y ? pxy : nullptr, xyb, &pxy_d);
    if (st.commit()) return -1;
    void *win_d = nullptr;
    if (win && get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    const cf *tw;
    if (get_twiddles(nfft, &tw)) return -1;
    float *partial = nullptr;
    if (!pl.final_form) {
        if (g.work.ensure(pl.scratch_bytes)) return -1;
        partial = (float *)g.work.p;
    }
    const double mult = scale / (double)navg;
    const WelchBlocksArgs a{xd, yd, (const float *)win_d, hop, detrend == SP_DETREND_SEGMEAN ? 1 : 0, pl.q, pl.rpt, y ? 4 : 1,
                            y_ld, nframes, pl.runs, pl.rstride, (float)mult, (float)(dbl ? 2.0 * mult : mult), partial,
                            pxx_d, pyy_d, pxy_d};
    {
        ProfScope ps;
        LAUNCHCHK(launch_welch_blocks(lc(), a, cplx, nfft, tw, pairs, pl.wgs));
        g.last_kernel = "k_welch_blocks";
    }
    if (!pl.final_form)
        LAUNCHCHK(launch_block_sum(lc(), partial, pl.runs, y ? 4 : 1, pl.nb, pl.nblocks, pl.adv, pl.nsum, dbl, nfft, mult, pairs, pxx_d,
                                   pyy_d, pxy_d));
    return st.finish();
}

// ---- continuous wavelet transform (k_cwt.hip) ------------------------------------------------------
// the shape checks sp_cwt and its plan share; 0 or the message's tail
static const char *cwt_shape(int64_t nsig, int nscales, int64_t batch, int L, int M) {
    if (L < SP_CWT_MIN_L || L > SP_CWT_MAX_L || !is_pow2(L)) return "L must be a power of two from 256 to 8192";
    if (M < 0 || 2 * (int64_t)M >= L) return "M must lie in 0 .. L / 2 - 1";
    if (L - 2 * M < L / 4) return "M leaves hop = L - 2 M below L / 4";
    if (nscales < 1) return "nscales must be at least 1";
    if (nsig < 1) return "nsig must be at least 1";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    return nullptr;
}

int sp_cwt_plan(int64_t nsig, int nscales, int64_t batch, int L, int M, int outputs, int64_t out[5]) {
    if (cwt_shape(nsig, nscales, batch, L, M) || !out || (outputs & 15) == 0 || (outputs & ~15) != 0) return -1;
    const CwtPlan p = cwt_plan_of(L, M, nsig, nscales, batch, (outputs & 12) != 0, (outputs & 2) != 0, g.ncu, env_int("SP_CWT_CHUNK", 0));
    out[0] = p.hop;
    out[1] = p.frames;
    out[2] = p.chunk;
    out[3] = p.grid;
    out[4] = (int64_t)p.scratch_bytes;
    return 0;
}

int sp_cwt(const void *x, int dtype, int64_t nsig, int64_t x_ld, int64_t batch, const double *scales, int nscales, int family, double p0,
           double p1, int L, int M, const float *wrec, const float *wband, void *W, double *gws, void *recon, float *bandpow, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = cwt_shape(nsig, nscales, batch, L, M))
        return fail("sp_cwt: %s (L %d, M %d, nscales %d, nsig %lld, batch %lld)", why, L, M, nscales, (long long)nsig, (long long)batch);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_cwt: dtype must be float32 or complex64, got %d", dtype);
    if (x_ld < nsig) return fail("sp_cwt: x_ld = %lld is below nsig = %lld", (long long)x_ld, (long long)nsig);
    if (family != SP_CWT_MORLET && family != SP_CWT_PAUL) return fail("sp_cwt: family %d is neither SP_CWT_MORLET nor SP_CWT_PAUL", family);
    if (!isfinite(p0) || !(p0 > 0.0) || p0 > 64.0 || (family == SP_CWT_PAUL && p0 < 1.0) || p1 != 0.0)
        return fail("sp_cwt: parameter p0 = %g must lie in (0, 64] (Morlet's w0) or [1, 64] (Paul's m), and p1 = %g must be 0", p0, p1);
    if (!scales) return fail("sp_cwt: scales is required");
    for (int s = 0; s < nscales; ++s)
        if (!isfinite(scales[s]) || !(scales[s] > 0.0) || scales[s] > 1e9)
            return fail("sp_cwt: scales[%d] = %g must be positive and finite", s, scales[s]);
    if (!W && !gws && !recon && !bandpow) return fail("sp_cwt: an output is required: W, gws, recon or bandpow");
    if (recon && !wrec) return fail("sp_cwt: wrec is required with recon");
    if (bandpow && !wband) return fail("sp_cwt: wband is required with bandpow");
    for (int s = 0; s < nscales; ++s)
        if ((recon && !isfinite(wrec[s])) || (bandpow && !isfinite(wband[s]))) return fail("sp_cwt: weights must be finite (scale %d)", s);
    if (batch == 0) return 0;
    if (!x) return fail("sp_cwt: x is required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64, whole = recon || bandpow;
    const CwtPlan pl = cwt_plan_of(L, M, nsig, nscales, batch, whole, gws != nullptr, g.ncu, env_int("SP_CWT_CHUNK", 0));
    if (pl.blocks_x > INT_MAX) return fail("sp_cwt: nsig = %lld is too many frames for one launch", (long long)nsig);
    const size_t esz = cplx ? 8 : 4, in_elems = (size_t)((batch - 1) * x_ld + nsig), S = (size_t)nscales, rows = (size_t)batch;
    // the scales' filter constants: step = 2 pi s' / L, c = ln(norm sqrt(2 pi s') / L)
    const double lognorm = family == SP_CWT_MORLET ? -0.25 * log(M_PI) : p0 * log(2.0) - 0.5 * (log(p0) + lgamma(2.0 * p0));
    std::vector<float> sc(2 * S);
    for (size_t s = 0; s < S; ++s) {
        sc[2 * s] = (float)(2.0 * M_PI * scales[s] / (double)L);
        sc[2 * s + 1] = (float)(lognorm + 0.5 * log(2.0 * M_PI * scales[s]) - log((double)L));
    }
    void *sc_d = nullptr, *wr_d = nullptr, *wb_d = nullptr;
    if (get_table(15, sc.data(), sizeof(float) * sc.size(), &sc_d, nullptr)) return -1;
    if (recon && get_table(16, wrec, sizeof(float) * S, &wr_d, nullptr)) return -1;
    if (bandpow && get_table(17, wband, sizeof(float) * S, &wb_d, nullptr)) return -1;
    const cf *tw;
    if (get_twiddles(L, &tw)) return -1;
    Stage st(mem);
    const void *xd;
    cf *W_d, *rec_d;
    double *gws_d;
    float *bp_d;
    st.in(g.in0, x, esz * in_elems, &xd);
    st.out(g.out0, W, sizeof(cf) * rows * S * (size_t)nsig, &W_d);
    st.out(g.out0, gws, sizeof(double) * rows * S, &gws_d);
    st.out(g.out0, recon, sizeof(cf) * rows * (size_t)nsig, &rec_d);
    st.out(g.out0, bandpow, sizeof(float) * rows * (size_t)nsig, &bp_d);
    if (st.commit()) return -1;
    float *gpart = nullptr;
    if (gws) {
        if (g.work.ensure(pl.scratch_bytes)) return -1;
        gpart = (float *)g.work.p;
    }
    CwtArgs a;
    a.x = xd;
    a.cplx = cplx ? 1 : 0;
    a.nsig = nsig;
    a.x_ld = x_ld;
    a.nframes = pl.frames;
    a.sc = (const float *)sc_d;
    a.p = family == SP_CWT_PAUL ? (float)p0 : 0.f;
    a.a = family == SP_CWT_MORLET ? 0.5f : 0.f;
    a.b = family == SP_CWT_PAUL ? 1.f : 0.f;
    a.u0 = family == SP_CWT_MORLET ? (float)p0 : 0.f;
    a.S = nscales;
    a.chunk = pl.chunk;
    a.M = M;
    a.hop = pl.hop;
    a.wr = (const float *)wr_d;
    a.wb = (const float *)wb_d;
    a.W = W_d;
    a.gpart = gpart;
    a.recon = rec_d;
    a.bandpow = bp_d;
    {
        ProfScope ps;
        if (launch_cwt(lc(), a, L, tw, pl, batch) != 0)
            return fail("sp_cwt: the launch was refused (L %d, M %d, nscales %d, %lld rows)", L, M, nscales, (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_cwt";
    }
    if (gws) LAUNCHCHK(launch_cwt_gws_finish(lc(), gpart, (int64_t)(rows * S), pl.frames, gws_d));
    return st.finish();
}

int sp_icwt(const void *W, int64_t nsig, int nscales, int64_t batch, const float *w, void *out, int mem) {
    // every refusal comes before the device is touched
    if (nscales < 1) return fail("sp_icwt: nscales must be at least 1");
    if (nsig < 1) return fail("sp_icwt: nsig must be at least 1");
    if (batch < 0 || batch > 65535) return fail("sp_icwt: batch must lie in 0 .. 65535");
    if (!w) return fail("sp_icwt: w is required");
    for (int s = 0; s < nscales; ++s)
        if (!isfinite(w[s])) return fail("sp_icwt: weights must be finite (scale %d)", s);
    if (batch == 0) return 0;
    if (!W || !out) return fail("sp_icwt: W and out are required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t ibytes = sizeof(cf) * (size_t)batch * (size_t)nscales * (size_t)nsig, obytes = sizeof(cf) * (size_t)batch * (size_t)nsig;
    Stage st(mem);
    const void *Wd;
    void *od;
    st.in(g.in0, W, ibytes, &Wd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    void *w_d = nullptr;
    if (get_table(16, w, sizeof(float) * (size_t)nscales, &w_d, nullptr)) return -1;
    {
        ProfScope ps;
        LAUNCHCHK(launch_icwt(lc(), (const cf *)Wd, (const float *)w_d, nscales, nsig, batch, (cf *)od));
        g.last_kernel = "k_icwt";
    }
    return st.finish();
}

// ---- cross-wavelet spectra and wavelet coherence (k_wct.hip; include/spectral_ext.h) -------------------
// the shape checks sp_wct_time and its plan share; 0 or the message's tail
static const char *wct_shape(int64_t nsig, int nscales, int64_t batch, int L, int Mw, int Mg, bool xwt) {
    if (L < SP_CWT_MIN_L || L > SP_CWT_MAX_L || !is_pow2(L)) return "L must be a power of two from 256 to 8192";
    if (Mw < 0 || Mg < 0 || 2 * ((int64_t)Mw + Mg) >= L) return "Mw and Mg must not be negative, and Mw + Mg must lie in 0 .. L / 2 - 1";
    if (L - 2 * (Mw + Mg) < L / 4) return "Mw + Mg leaves hop = L - 2 (Mw + Mg) below L / 4";
    if (xwt && Mg != 0) return "Mg must be 0 with Wxy";
    if (nscales < 1 || nscales > 65535) return "nscales must lie in 1 .. 65535";
    if (nsig < 1) return "nsig must be at least 1";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    return nullptr;
}

int sp_wct_plan(int64_t nsig, int nscales, int64_t batch, int L, int Mw, int Mg, int xwt, int64_t out[5]) {
    if (wct_shape(nsig, nscales, batch, L, Mw, Mg, xwt != 0) || !out) return -1;
    const CwtPlan p = cwt_plan_of(L, Mw + Mg, nsig, nscales, batch, false, false, g.ncu, env_int("SP_WCT_CHUNK", 0));
    out[0] = p.hop;
    out[1] = p.frames;
    out[2] = p.chunk;
    out[3] = p.grid;
    out[4] = (int64_t)wct_lds_bytes(L);
    return 0;
}

int sp_wct_time(const void *x, int64_t x_ld, const void *y, int64_t y_ld, int dtype, int64_t nsig, int64_t batch, const double *scales,
                int nscales, int family, double p0, int L, int Mw, int Mg, void *T, void *Wxy, int mem) {
    // every refusal comes before the device is touched
    if ((T != nullptr) == (Wxy != nullptr)) return fail("sp_wct_time: exactly one output is required: T or Wxy");
    if (const char *why = wct_shape(nsig, nscales, batch, L, Mw, Mg, Wxy != nullptr))
        return fail("sp_wct_time: %s (L %d, Mw %d, Mg %d, nscales %d, nsig %lld, batch %lld)", why, L, Mw, Mg, nscales, (long long)nsig,
                    (long long)batch);
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("sp_wct_time: dtype must be float32 or complex64, got %d", dtype);
    if (x_ld < nsig) return fail("sp_wct_time: x_ld = %lld is below nsig = %lld", (long long)x_ld, (long long)nsig);
    if (y_ld < nsig) return fail("sp_wct_time: y_ld = %lld is below nsig = %lld", (long long)y_ld, (long long)nsig);
    if (family != SP_CWT_MORLET && family != SP_CWT_PAUL)
        return fail("sp_wct_time: family %d is neither SP_CWT_MORLET nor SP_CWT_PAUL", family);
    if (T && family != SP_CWT_MORLET) return fail("sp_wct_time: family must be SP_CWT_MORLET with T (the smoothing operator is Morlet's)");
    if (!isfinite(p0) || !(p0 > 0.0) || p0 > 64.0 || (family == SP_CWT_PAUL && p0 < 1.0))
        return fail("sp_wct_time: parameter p0 = %g must lie in (0, 64] (Morlet's w0) or [1, 64] (Paul's m)", p0);
    if (!scales) return fail("sp_wct_time: scales is required");
    for (int s = 0; s < nscales; ++s)
        if (!isfinite(scales[s]) || !(scales[s] > 0.0) || scales[s] > 1e9)
            return fail("sp_wct_time: scales[%d] = %g must be positive and finite", s, scales[s]);
    // real difference: a device caller's own T is stored with 16-byte vectors (a staged T starts a scratch buffer)
    if (mem && T && ((uintptr_t)T & 15) != 0) return fail("sp_wct_time: T must be 16-byte aligned");
    if (batch == 0) return 0;
    if (!x || !y) return fail("sp_wct_time: x and y are required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64;
    const int M = Mw + Mg;
    const CwtPlan pl = cwt_plan_of(L, M, nsig, nscales, batch, false, false, g.ncu, env_int("SP_WCT_CHUNK", 0));
    if (pl.blocks_x > INT_MAX) return fail("sp_wct_time: nsig = %lld is too many frames for one launch", (long long)nsig);
    const size_t esz = cplx ? 8 : 4, S = (size_t)nscales, rows = (size_t)batch;
    const size_t x_elems = (size_t)((batch - 1) * x_ld + nsig), y_elems = (size_t)((batch - 1) * y_ld + nsig);
    // the scales' constants: step = 2 pi s' / L, c = ln(norm sqrt(2 pi s') / L), 1 / s'
    const double lognorm = family == SP_CWT_MORLET ? -0.25 * log(M_PI) : p0 * log(2.0) - 0.5 * (log(p0) + lgamma(2.0 * p0));
    std::vector<float> sc(4 * S);
    for (size_t s = 0; s < S; ++s) {
        sc[4 * s] = (float)(2.0 * M_PI * scales[s] / (double)L);
        sc[4 * s + 1] = (float)(lognorm + 0.5 * log(2.0 * M_PI * scales[s]) - log((double)L));
        sc[4 * s + 2] = (float)(1.0 / scales[s]);
        sc[4 * s + 3] = 0.f;
    }
    void *sc_d = nullptr;
    if (get_table(18, sc.data(), sizeof(float) * sc.size(), &sc_d, nullptr)) return -1;
    const cf *tw;
    if (get_twiddles(L, &tw)) return -1;
    const size_t obytes = (T ? sizeof(float4) : sizeof(cf)) * rows * S * (size_t)nsig;
    Stage st(mem);
    const void *xd, *yd;
    void *od;
    st.in(g.in0, x, esz * x_elems, &xd);
    st.in(g.in1, y, esz * y_elems, &yd);
    st.out(g.out0, T ? T : Wxy, obytes, &od);
    if (st.commit()) return -1;
    WctArgs a;
    a.x = xd;
    a.y = yd;
    a.cplx = cplx ? 1 : 0;
    a.nsig = nsig;
    a.x_ld = x_ld;
    a.y_ld = y_ld;
    a.nframes = pl.frames;
    a.sc = (const float *)sc_d;
    a.p = family == SP_CWT_PAUL ? (float)p0 : 0.f;
    a.a = family == SP_CWT_MORLET ? 0.5f : 0.f;
    a.b = family == SP_CWT_PAUL ? 1.f : 0.f;
    a.u0 = family == SP_CWT_MORLET ? (float)p0 : 0.f;
    a.S = nscales;
    a.chunk = pl.chunk;
    a.M = M;
    a.hop = pl.hop;
    a.T = T ? (float4 *)od : nullptr;
    a.Wxy = T ? nullptr : (cf *)od;
    {
        ProfScope ps;
        if (launch_wct_time(lc(), a, L, tw, pl, batch) != 0)
            return fail("sp_wct_time: the launch was refused (L %d, Mw %d, Mg %d, nscales %d, %lld rows)", L, Mw, Mg, nscales,
                        (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_wct_time";
    }
    return st.finish();
}

int sp_wct_scale(const void *T, int64_t nsig, int nscales, int64_t batch, const float *taps, int ntaps, float *R2, float *phase, float *A,
                 float *B, void *C, int mem) {
    // every refusal comes before the device is touched
    if (nscales < 1 || nscales > 65535) return fail("sp_wct_scale: nscales must lie in 1 .. 65535");
    if (nsig < 1) return fail("sp_wct_scale: nsig must be at least 1");
    if (batch < 0 || batch > 65535) return fail("sp_wct_scale: batch must lie in 0 .. 65535");
    if (ntaps < 1 || ntaps > 4096) return fail("sp_wct_scale: ntaps must lie in 1 .. 4096");
    if (!taps) return fail("sp_wct_scale: taps is required");
    for (int j = 0; j < ntaps; ++j)
        if (!isfinite(taps[j])) return fail("sp_wct_scale: taps must be finite (tap %d)", j);
    if ((A != nullptr) != (B != nullptr) || (A != nullptr) != (C != nullptr))
        return fail("sp_wct_scale: A, B and C are given together or not at all");
    // real difference: a device caller's own T is read with 16-byte vectors (a staged T starts a scratch buffer)
    if (mem && T && ((uintptr_t)T & 15) != 0) return fail("sp_wct_scale: T must be 16-byte aligned");
    if (batch == 0) return 0;
    if (!T || !R2 || !phase) return fail("sp_wct_scale: T, R2 and phase are required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t cells = (size_t)batch * (size_t)nscales * (size_t)nsig, fb = sizeof(float) * cells;
    Stage st(mem);
    const void *Td;
    float *R2_d, *ph_d, *A_d, *B_d;
    cf *C_d;
    st.in(g.in0, T, sizeof(float4) * cells, &Td);
    st.out(g.out0, R2, fb, &R2_d);
    st.out(g.out0, phase, fb, &ph_d);
    st.out(g.out0, A, fb, &A_d);
    st.out(g.out0, B, fb, &B_d);
    st.out(g.out0, C, 2 * fb, &C_d);
    if (st.commit()) return -1;
    void *taps_d = nullptr;
    if (get_table(19, taps, sizeof(float) * (size_t)ntaps, &taps_d, nullptr)) return -1;
    {
        ProfScope ps;
        LAUNCHCHK(launch_wct_scale(lc(), (const float4 *)Td, (const float *)taps_d, ntaps, nscales, nsig, batch, R2_d, ph_d, A_d, B_d, C_d));
        g.last_kernel = "k_wct_scale";
    }
    return st.finish();
}

// ---- synchrosqueezed STFT and reassignment fields (k_ssq.hip; include/spectral_tfr.h) ------------------
// the checks the three front ends share; 0 or the message's tail
static const char *ssq_shape(int n, int hop, int64_t first, int64_t nframes, int64_t batch, int dtype, int64_t nsig, int64_t x_ld,
                             double gamma, double rel) {
    if (n < 32 || n > SP_SSQ_MAX_L || !is_pow2(n)) return "n must be a power of two from 32 to 8192";
    if (hop < 1) return "hop must be at least 1";
    if (nframes < 0) return "nframes must not be negative";
    if (nframes > ((int64_t)1 << 40) / hop || first > ((int64_t)1 << 40) || first < -((int64_t)1 << 40)) return "nframes, hop and first: the frames lie beyond 2^40 samples";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return "dtype must be float32 or complex64";
    if (nsig < 1) return "nsig must be at least 1";
    if (x_ld < nsig) return "x_ld is below nsig";
    if (!isfinite(gamma) || gamma < 0.0) return "gamma must be finite and not negative";
    if (!isfinite(rel) || rel < 0.0) return "rel must be finite and not negative";
    return nullptr;
}

int sp_ssq_plan(int cplx, int n, int64_t nframes, int64_t batch, int nb, int what, int64_t out[5]) {
    if (n < 32 || n > SP_SSQ_MAX_L || !is_pow2(n) || nframes < 0 || batch < 0 || batch > 65535 || !out) return -1;
    const bool bands = what == 8;
    if (!bands && (what < 1 || what > 7)) return -1;
    if (!bands && !band_in_transform(cplx != 0, n, 0, nb)) return -1;
    const bool fields = !bands && (what & 4);
    const int64_t fpr = ssq_fpr(n, nframes, batch, g.ncu, env_int("SP_SSQ_FPG", 0));
    const size_t lds = ssq_lds_bytes(cplx != 0, n, bands ? 0 : nb, !bands && (what & 1), !bands && (what & 2), fields);
    out[0] = fpr;
    out[1] = (nframes + fpr - 1) / fpr * batch;
    out[2] = (int64_t)lds;
    out[3] = ssq_transforms(cplx != 0, fields);
    out[4] = lds <= SP_LDS_MAX ? 1 : 0;
    return 0;
}

// the frames of one call: stages x for host callers, uploads the windows, fills what the two kernels' arguments share
static int ssq_front(const char *who, SsqArgs &a, const void *x, int64_t x_ld, bool cplx, int64_t nsig, int64_t batch, const float *h,
                     const float *dh, const float *th, int n, int hop, int64_t first, int64_t nframes, int segmean, double gamma,
                     double rel, Stage &st, const cf **tw) {
    const size_t esz = cplx ? 8 : 4, x_elems = (size_t)((batch - 1) * x_ld + nsig);
    const void *xd;
    st.in(g.in0, x, esz * x_elems, &xd);
    if (st.commit()) return -1;
    void *h_d = nullptr, *dh_d = nullptr, *th_d = nullptr;
    if (get_table(1, h, sizeof(float) * (size_t)n, &h_d, nullptr)) return -1;
    if (get_table(20, dh, sizeof(float) * (size_t)n, &dh_d, nullptr)) return -1;
    if (th && get_table(21, th, sizeof(float) * (size_t)n, &th_d, nullptr)) return -1;
    if (get_twiddles(n, tw)) return -1;
    a = SsqArgs{};
    a.x = xd;
    a.x_ld = x_ld;
    a.nsig = nsig;
    a.first = first;
    a.nframes = nframes;
    a.fpr = ssq_fpr(n, nframes, batch, g.ncu, env_int("SP_SSQ_FPG", 0));
    a.h = (const float *)h_d;
    a.dh = (const float *)dh_d;
    a.th = (const float *)th_d;
    a.hop = hop;
    a.segmean = segmean ? 1 : 0;
    a.gamma = (float)gamma;
    a.rel = (float)rel;
    if ((a.nframes + a.fpr - 1) / a.fpr > INT_MAX) return fail("%s: nframes = %lld is too many runs for one launch", who, (long long)nframes);
    return 0;
}

int sp_ssq(const void *x, int64_t x_ld, int dtype, int64_t nsig, int64_t batch, const float *h, const float *dh, const float *th, int n,
           int hop, int64_t first, int64_t nframes, int segmean, double gamma, double rel, int b0, int nb, void *T, float *P, float *IF,
           float *GD, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = ssq_shape(n, hop, first, nframes, batch, dtype, nsig, x_ld, gamma, rel))
        return fail("sp_ssq: %s (n %d, hop %d, nframes %lld, batch %lld, nsig %lld, x_ld %lld)", why, n, hop, (long long)nframes,
                    (long long)batch, (long long)nsig, (long long)x_ld);
    const bool cplx = dtype == SP_DTYPE_C64, fields = IF || GD;
    if (!T && !P && !IF && !GD) return fail("sp_ssq: an output is required: T, P, IF or GD");
    if (fields && !th) return fail("sp_ssq: th is required with IF or GD");
    if (!band_in_transform(cplx, n, b0, nb))
        return fail("sp_ssq: nb = %d bins from b0 = %d lie outside the %d bins of the spectrum", nb, b0, cplx ? n : n / 2 + 1);
    const size_t lds = ssq_lds_bytes(cplx, n, nb, T != nullptr, P != nullptr, fields);
    if (lds > SP_LDS_MAX)
        return fail("sp_ssq: the LDS of a workgroup, %zu bytes, does not fit %zu (n %d, nb %d): take a narrower band or fewer outputs", lds,
                    SP_LDS_MAX, n, nb);
    if (!h || !dh) return fail("sp_ssq: h and dh are required");
    if (batch == 0 || nframes == 0) return 0;
    if (!x) return fail("sp_ssq: x is required");
    if (ensure_init()) return -1;
    ApiLock lk;
    SsqArgs a;
    const cf *tw;
    Stage st(mem);
    if (ssq_front("sp_ssq", a, x, x_ld, cplx, nsig, batch, h, dh, fields ? th : nullptr, n, hop, first, nframes, segmean, gamma, rel, st, &tw))
        return -1;
    const size_t cells = (size_t)batch * (size_t)nframes * (size_t)nb, fb = sizeof(float) * cells;
    a.b0 = b0;
    a.nb = nb;
    st.out(g.out0, T, 2 * fb, &a.T);
    st.out(g.out0, P, fb, &a.P);
    st.out(g.out0, IF, fb, &a.IF);
    st.out(g.out0, GD, fb, &a.GD);
    if (st.commit()) return -1;
    {
        ProfScope ps;
        if (launch_ssq(lc(), a, cplx, n, tw, (nframes + a.fpr - 1) / a.fpr, batch, lds) != 0)
            return fail("sp_ssq: the launch was refused (n %d, nb %d, %lld frames, %lld rows)", n, nb, (long long)nframes, (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_ssq";
    }
    return st.finish();
}

// the band edges of sp_ssq_bands / sp_ssq_sum; 0 or the message's tail
static const char *ssq_edges_why(int nbands, const double *edges, const float *edges_t, double scale) {
    if (nbands < 1 || nbands > SP_SSQ_MAX_BANDS) return "nbands must lie in 1 .. 8";
    if ((edges != nullptr) == (edges_t != nullptr)) return "exactly one of edges and edges_t is required";
    if (edges)
        for (int j = 0; j < 2 * nbands; ++j)
            if (!isfinite(edges[j])) return "edges must be finite";
    if (!isfinite(scale)) return "scale must be finite";
    return nullptr;
}
// the edges as float32: the constant pairs by value, the per-frame ones staged for host callers
static int ssq_edges(int nbands, const double *edges, const float *edges_t, int64_t nframes, Stage &st, SsqEdges *ec, const float **out) {
    *ec = SsqEdges{};
    *out = nullptr;
    if (edges) {
        for (int j = 0; j < 2 * nbands; ++j) ec->v[j] = (float)edges[j];
        return 0;
    }
    st.in(g.in1, edges_t, sizeof(float) * 2 * (size_t)nbands * (size_t)nframes, out);
    return st.commit();
}

int sp_ssq_bands(const void *x, int64_t x_ld, int dtype, int64_t nsig, int64_t batch, const float *h, const float *dh, int n, int hop,
                 int64_t first, int64_t nframes, int segmean, double gamma, double rel, int nbands, const double *edges,
                 const float *edges_t, double scale, void *out, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = ssq_shape(n, hop, first, nframes, batch, dtype, nsig, x_ld, gamma, rel))
        return fail("sp_ssq_bands: %s (n %d, hop %d, nframes %lld, batch %lld, nsig %lld, x_ld %lld)", why, n, hop, (long long)nframes,
                    (long long)batch, (long long)nsig, (long long)x_ld);
    if (const char *why = ssq_edges_why(nbands, edges, edges_t, scale)) return fail("sp_ssq_bands: %s (nbands %d)", why, nbands);
    const bool cplx = dtype == SP_DTYPE_C64;
    const size_t lds = ssq_lds_bytes(cplx, n, 0, false, false, false);
    if (lds > SP_LDS_MAX) return fail("sp_ssq_bands: the LDS of a workgroup, %zu bytes, does not fit %zu", lds, SP_LDS_MAX);
    if (!h || !dh) return fail("sp_ssq_bands: h and dh are required");
    if (!out) return fail("sp_ssq_bands: out is required");
    if (batch == 0 || nframes == 0) return 0;
    if (!x) return fail("sp_ssq_bands: x is required");
    if (ensure_init()) return -1;
    ApiLock lk;
    SsqArgs a;
    const cf *tw;
    Stage st(mem);
    if (ssq_front("sp_ssq_bands", a, x, x_ld, cplx, nsig, batch, h, dh, nullptr, n, hop, first, nframes, segmean, gamma, rel, st, &tw)) return -1;
    if (ssq_edges(nbands, edges, edges_t, nframes, st, &a.edges_c, &a.edges)) return -1;
    a.nbands = nbands;
    a.per_frame = edges ? 0 : 1;
    a.scale = (float)scale;
    st.out(g.out0, out, sizeof(cf) * (size_t)batch * (size_t)nbands * (size_t)nframes, &a.out);
    if (st.commit()) return -1;
    {
        ProfScope ps;
        if (launch_ssq(lc(), a, cplx, n, tw, (nframes + a.fpr - 1) / a.fpr, batch, lds) != 0)
            return fail("sp_ssq_bands: the launch was refused (n %d, %d bands, %lld frames, %lld rows)", n, nbands, (long long)nframes,
                        (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_ssq";
    }
    return st.finish();
}

int sp_ssq_sum(const void *T, int64_t nframes, int nb, int64_t batch, int n, int b0, int nbands, const double *edges, const float *edges_t,
               int half, double scale, void *out, int mem) {
    // every refusal comes before the device is touched
    if (n < 32 || n > SP_SSQ_MAX_L || !is_pow2(n)) return fail("sp_ssq_sum: n = %d must be a power of two from 32 to 8192", n);
    if (nframes < 0) return fail("sp_ssq_sum: nframes must not be negative");
    if (batch < 0 || batch > 65535) return fail("sp_ssq_sum: batch must lie in 0 .. 65535");
    if (!band_in_transform(true, n, b0, nb)) return fail("sp_ssq_sum: nb = %d bins from b0 = %d lie outside the %d bins of the spectrum", nb, b0, n);
    if (const char *why = ssq_edges_why(nbands, edges, edges_t, scale)) return fail("sp_ssq_sum: %s (nbands %d)", why, nbands);
    if (!out) return fail("sp_ssq_sum: out is required");
    if (batch == 0 || nframes == 0) return 0;
    if (!T) return fail("sp_ssq_sum: T is required");
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t tbytes = sizeof(cf) * (size_t)batch * (size_t)nframes * (size_t)nb;
    const size_t obytes = sizeof(cf) * (size_t)batch * (size_t)nbands * (size_t)nframes;
    Stage st(mem);
    const void *Td;
    cf *od;
    st.in(g.in0, T, tbytes, &Td);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    const float *ed;
    SsqEdges ec;
    if (ssq_edges(nbands, edges, edges_t, nframes, st, &ec, &ed)) return -1;
    {
        ProfScope ps;
        LAUNCHCHK(launch_ssq_sum(lc(), (const cf *)Td, nframes, nb, n, b0, nbands, edges ? 0 : 1, ed, ec, half ? 1 : 0, (float)scale, batch, od));
        g.last_kernel = "k_ssq_sum";
    }
    return st.finish();
}

// ---- smoothed pseudo Wigner-Ville distribution (k_wvd.hip; include/spectral_quad.h) --------------------
// the checks sp_wvd and sp_wvd_plan share; 0 or the message's tail
static const char *wvd_shape(int nfft, int nh, int ng, int64_t hop, int64_t first, int64_t ntimes, int64_t batch, int nb) {
    if (nfft < 32 || nfft > SP_WVD_MAX_L || !is_pow2(nfft)) return "nfft must be a power of two from 32 to 8192";
    if (nh < 1 || !(nh & 1) || nh > nfft - 1) return "nh must be odd and lie in 1 .. nfft - 1";
    if (ng < 1 || !(ng & 1) || ng > SP_WVD_MAX_NG) return "ng must be odd and lie in 1 .. 255";
    if (hop < 1) return "hop must be at least 1";
    if (ntimes < 0) return "ntimes must not be negative";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    if (nb < 1 || nb > nfft) return "nb must lie in 1 .. nfft";
    if (hop > SP_WVD_MAX_SPAN || ntimes > SP_WVD_MAX_SPAN / hop || first > SP_WVD_MAX_SPAN || first < -SP_WVD_MAX_SPAN)
        return "ntimes, hop and first: the columns lie beyond 2^40 samples";
    return nullptr;
}

int sp_wvd_plan(int cross, int nfft, int nh, int ng, int64_t hop, int64_t ntimes, int64_t batch, int nb, int64_t out[5]) {
    if (!out || wvd_shape(nfft, nh, ng, hop, 0, ntimes, batch, nb)) return -1;
    const int64_t cpr = wvd_cpr(cross != 0, nfft, nh, ng, hop, ntimes, batch, g.ncu, env_int("SP_WVD_CPR", 0));
    const size_t lds = wvd_lds_bytes(cross != 0, nfft, nh, ng, hop, cpr, ntimes);
    out[0] = cpr;
    out[1] = (ntimes + cpr - 1) / cpr * batch;
    out[2] = (int64_t)lds;
    out[3] = wvd_transforms_per_run(cross != 0, cpr);
    out[4] = lds <= SP_LDS_MAX ? 1 : 0;
    return 0;
}

int sp_wvd(const void *x, const void *y, int64_t x_ld, int64_t nsig, int64_t batch, const float *h, int nh, const float *gw, int ng,
           int nfft, int64_t hop, int64_t first, int64_t ntimes, int b0, int nb, double scale, void *W, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = wvd_shape(nfft, nh, ng, hop, first, ntimes, batch, nb))
        return fail("sp_wvd: %s (nfft %d, nh %d, ng %d, hop %lld, ntimes %lld, batch %lld, nb %d)", why, nfft, nh, ng, (long long)hop,
                    (long long)ntimes, (long long)batch, nb);
    if (nsig < 1) return fail("sp_wvd: nsig = %lld must be at least 1", (long long)nsig);
    if (x_ld < nsig) return fail("sp_wvd: x_ld = %lld is below nsig = %lld", (long long)x_ld, (long long)nsig);
    if (b0 < 0 || b0 >= nfft) return fail("sp_wvd: b0 = %d lies outside 0 .. nfft - 1 = %d", b0, nfft - 1);
    if (!isfinite(scale)) return fail("sp_wvd: scale must be finite");
    if (!x) return fail("sp_wvd: x is required");
    if (!h) return fail("sp_wvd: h is required");
    if (!gw) return fail("sp_wvd: g is required");
    if (!W) return fail("sp_wvd: W is required");
    const bool cross = y != nullptr;
    const int64_t cpr = wvd_cpr(cross, nfft, nh, ng, hop, ntimes, batch, g.ncu, env_int("SP_WVD_CPR", 0));
    const size_t lds = wvd_lds_bytes(cross, nfft, nh, ng, hop, cpr, ntimes);
    if (lds > SP_LDS_MAX)
        return fail("sp_wvd: the LDS of a workgroup, %zu bytes, does not fit %zu (nfft %d, nh %d, ng %d, hop %lld, %lld columns per run)",
                    lds, SP_LDS_MAX, nfft, nh, ng, (long long)hop, (long long)cpr);
    if (batch == 0 || ntimes == 0) return 0;
    const int64_t runs = (ntimes + cpr - 1) / cpr;
    if (runs > INT_MAX) return fail("sp_wvd: ntimes = %lld is too many runs for one launch", (long long)ntimes);
    if (ensure_init()) return -1;
    ApiLock lk;
    WvdArgs a{};
    Stage st(mem);
    const size_t x_elems = (size_t)((batch - 1) * x_ld + nsig);
    st.in(g.in0, x, sizeof(cf) * x_elems, &a.x);
    st.in(g.in1, y, sizeof(cf) * x_elems, &a.y);
    st.out(g.out0, W, (cross ? sizeof(cf) : sizeof(float)) * (size_t)batch * (size_t)ntimes * (size_t)nb, &a.W);
    if (st.commit()) return -1;
    // auto: W is the real part, the distribution under the even part of h (h itself when it is symmetric: (v + v) / 2 is exact)
    std::vector<float> hs(h, h + nh);
    if (!cross)
        for (int j = 0; j < nh; ++j) hs[(size_t)j] = 0.5f * (h[j] + h[nh - 1 - j]);
    void *h_d = nullptr, *g_d = nullptr;
    const cf *tw;
    if (get_table(22, hs.data(), sizeof(float) * (size_t)nh, &h_d, nullptr)) return -1;
    if (get_table(23, gw, sizeof(float) * (size_t)ng, &g_d, nullptr)) return -1;
    if (get_twiddles(nfft, &tw)) return -1;
    a.x_ld = x_ld;
    a.nsig = nsig;
    a.first = first;
    a.ntimes = ntimes;
    a.cpr = cpr;
    a.hop = hop;
    a.h = (const float *)h_d;
    a.g = (const float *)g_d;
    a.Lh = nh / 2;
    a.Lg = ng / 2;
    a.b0 = b0;
    a.nb = nb;
    a.scale = (float)scale;
    {
        ProfScope ps;
        if (launch_wvd(lc(), a, nfft, tw, runs, batch, lds) != 0)
            return fail("sp_wvd: the launch was refused (nfft %d, nb %d, %lld columns, %lld rows)", nfft, nb, (long long)ntimes, (long long)batch);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_wvd";
    }
    return st.finish();
}

// ---- spectral correlation by the averaged cyclic periodogram (k_cyclic.hip; include/spectral_cyclo.h) ----------
// the checks sp_cyclic and sp_cyclic_plan share; 0 or the message's tail
static const char *cyclic_shape(int dtype, int n, int64_t hop, int64_t nframes, int A, int64_t batch) {
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return "x_dtype must be float32 or complex64";
    if (n < 32 || n > SP_CYC_MAX_L || !is_pow2(n)) return "n must be a power of two from 32 to 8192";
    if (hop < 1) return "hop must be at least 1";
    if (nframes < 0) return "nframes must not be negative";
    if (A < 1 || A > SP_CYC_MAX_A) return "A must lie in 1 .. 65535";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    return nullptr;
}
static bool cyclic_mirror(int dtype, bool cross, int conj) { return !cross && (dtype == SP_DTYPE_F32 || conj != 0); }
// nu / 2 to the nearest multiple of 2^-64 turn (ties to even), modulo one turn; |nu| <= 1
static uint64_t cyclic_nuh(double nu) {
    const double v = nearbyint(ldexp(nu * 0.5, 64));        // |v| <= 2^63, an integer
    if (v >= 9223372036854775808.0 || v <= -9223372036854775808.0) return (uint64_t)1 << 63;      // +-1/2 turn
    return (uint64_t)(int64_t)v;
}

int sp_cyclic_plan(int dtype, int cross, int conj, int n, int64_t hop, int64_t nframes, int A, int64_t batch, int64_t out[5]) {
    if (!out || cyclic_shape(dtype, n, hop, nframes, A, batch)) return -1;
    const CycPlan p = cyc_plan_of(n, nframes, A, batch, cyclic_mirror(dtype, cross != 0, conj), g.ncu, env_int("SP_CYCLIC_CHUNK", 0),
                                   env_int("SP_CYCLIC_FPG", 0));
    out[0] = p.fpg;
    out[1] = p.blocks * A * batch;
    out[2] = p.apass;
    out[3] = p.passes;
    out[4] = p.xforms;
    return 0;
}

int sp_cyclic(const void *x, const void *y, int x_dtype, int y_dtype, int64_t x_ld, int64_t nsig, int64_t batch, const float *w, int n,
              int64_t hop, int64_t nframes, int64_t first, const double *nu, int A, int conj, const double *mean_x, const double *mean_y,
              int b0, int nb, double scale, void *S, void *Pp, void *Pm, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = cyclic_shape(x_dtype, n, hop, nframes, A, batch))
        return fail("sp_cyclic: %s (x_dtype %d, n %d, hop %lld, nframes %lld, A %d, batch %lld)", why, x_dtype, n, (long long)hop,
                    (long long)nframes, A, (long long)batch);
    if (y && y_dtype != x_dtype) return fail("sp_cyclic: y_dtype = %d differs from x_dtype = %d", y_dtype, x_dtype);
    if (nsig < 1) return fail("sp_cyclic: nsig = %lld must be at least 1", (long long)nsig);
    if (x_ld < nsig) return fail("sp_cyclic: x_ld = %lld is below nsig = %lld", (long long)x_ld, (long long)nsig);
    if (nframes > 0 && (n > nsig || (nframes - 1) > (nsig - n) / hop))
        return fail("sp_cyclic: nframes = %lld frames of n = %d at hop %lld reach outside the nsig = %lld samples of a row", (long long)nframes,
                    n, (long long)hop, (long long)nsig);
    if (first > ((int64_t)1 << 62) || first < -((int64_t)1 << 62)) return fail("sp_cyclic: first = %lld lies beyond +-2^62", (long long)first);
    if (!band_in_transform(true, n, b0, nb)) return fail("sp_cyclic: the band of nb = %d bins from b0 = %d lies outside the n = %d bins", nb, b0, n);
    if (!isfinite(scale)) return fail("sp_cyclic: scale must be finite");
    if (!x) return fail("sp_cyclic: x is required");
    if (!w) return fail("sp_cyclic: w is required");
    if (!nu) return fail("sp_cyclic: nu is required");
    if (!S && !Pp && !Pm) return fail("sp_cyclic: no output: one of S, Pp and Pm is required");
    for (int a = 0; a < A; ++a)
        if (!isfinite(nu[a]) || fabs(nu[a]) > 1.0) return fail("sp_cyclic: nu[%d] = %g must be finite and lie in -1 .. 1", a, nu[a]);
    const bool cross = y != nullptr, cplx = x_dtype == SP_DTYPE_C64, mirror = cyclic_mirror(x_dtype, cross, conj);
    for (int64_t b = 0; b < batch; ++b)
        for (int c = 0; c < 2; ++c)
            if ((mean_x && !isfinite(mean_x[2 * b + c])) || (cross && mean_y && !isfinite(mean_y[2 * b + c])))
                return fail("sp_cyclic: mean_x and mean_y must be finite (row %lld)", (long long)b);
    if (batch == 0 || nframes == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const CycPlan p = cyc_plan_of(n, nframes, A, batch, mirror, g.ncu, env_int("SP_CYCLIC_CHUNK", 0), env_int("SP_CYCLIC_FPG", 0));
    CycArgs a{};
    Stage st(mem);
    const size_t es = cplx ? sizeof(cf) : sizeof(float);
    const size_t x_elems = (size_t)((batch - 1) * x_ld + nsig), o_elems = (size_t)batch * (size_t)A * (size_t)nb;
    cf *S_d;
    float *Pp_d, *Pm_d;
    st.in(g.in0, x, es * x_elems, &a.x);
    st.in(g.in1, y, es * x_elems, &a.y);
    st.out(g.out0, S, sizeof(cf) * o_elems, &S_d);
    st.out(g.out0, Pp, sizeof(float) * o_elems, &Pp_d);
    st.out(g.out0, Pm, sizeof(float) * o_elems, &Pm_d);
    if (st.commit()) return -1;
    if (!cross) a.y = a.x;
    // small tables: the window, the phases nu / 2 in 2^-64 turns, the means as float32 (x, then y; auto: y = x)
    std::vector<uint64_t> nuh((size_t)A);
    for (int i = 0; i < A; ++i) nuh[(size_t)i] = cyclic_nuh(nu[i]);
    std::vector<float> mh((size_t)batch * 4, 0.f);
    for (int64_t b = 0; b < batch; ++b)
        for (int c = 0; c < 2; ++c) {
            const float mx = mean_x ? (float)mean_x[2 * b + c] : 0.f;
            mh[(size_t)(4 * b + c)] = mx;
            mh[(size_t)(4 * b + 2 + c)] = cross ? (mean_y ? (float)mean_y[2 * b + c] : 0.f) : mx;
        }
    void *w_d = nullptr, *nu_d = nullptr, *m_d = nullptr;
    const cf *tw;
    if (get_table(1, w, sizeof(float) * (size_t)n, &w_d, nullptr)) return -1;
    if (get_table(24, nuh.data(), sizeof(uint64_t) * (size_t)A, &nu_d, nullptr)) return -1;
    if (get_table(25, mh.data(), sizeof(float) * mh.size(), &m_d, nullptr)) return -1;
    if (get_twiddles(n, &tw)) return -1;
    const size_t cells = (size_t)batch * (size_t)p.apass * (size_t)p.groups;
    if (g.work.ensure(sizeof(float) * cells * p.cell_floats)) return -1;
    a.x_ld = x_ld;
    a.first = first;
    a.hop = hop;
    a.nframes = nframes;
    a.fpg = p.fpg;
    a.groups = p.groups;
    a.blocks = p.blocks;
    a.win = (const float *)w_d;
    a.means = (const float *)m_d;
    a.conj = conj ? 1 : 0;
    a.partial = (float *)g.work.p;
    a.gtab = (cf *)(a.partial + cells * (size_t)p.planes * (size_t)n);
    for (int a0 = 0; a0 < A; a0 += (int)p.apass, ++g_passes[2]) {
        a.A = (int)std::min<int64_t>(p.apass, A - a0);
        a.nuh = (const uint64_t *)nu_d + a0;
        ProfScope ps;
        if (launch_cyclic(lc(), a, mirror, cplx, n, tw, batch) != 0)
            return fail("sp_cyclic: the launch was refused (n %d, %d cycle frequencies, %lld frames, %lld rows)", n, a.A, (long long)nframes,
                        (long long)batch);
        HIPCHK(hipGetLastError());
        LAUNCHCHK(launch_cyclic_finish(lc(), a.partial, p.groups, p.used, n, mirror, a.A, a0, A, b0, nb, scale, batch, S_d, Pp_d, Pm_d));
        g.last_kernel = "k_cyclic";
    }
    return st.finish();
}

// ---- Lomb-Scargle spectra of unevenly sampled records (k_lomb.hip; include/spectral_uneven.h) ------------------
Scratch g_lombRec, g_lombSums;      // the prepared record with the call's small tables; the reduced sums of one pass of sp_lomb

// the checks every entry shares; 0 or the message's tail
static const char *lomb_shape(int64_t N, int64_t M, int64_t batch) {
    if (N < 1 || N >= ((int64_t)1 << 31)) return "N must lie in 1 .. 2^31 - 1";
    if (M < 1 || M > LOMB_MAX_M) return "M must lie in 1 .. 2^24";
    if (batch < 0 || batch > 65535) return "batch must lie in 0 .. 65535";
    return nullptr;
}
static const char *lomb_tables(const double *f, int64_t M, double t_ref, const double *mean, int64_t batch, int64_t *where) {
    *where = -1;
    if (!isfinite(t_ref)) return "t_ref must be finite";
    for (int64_t i = 0; i < M; ++i)
        if (!isfinite(f[i])) return *where = i, "every f must be finite";
    for (int64_t b = 0; mean && b < batch; ++b)
        if (!isfinite(mean[b])) return *where = b, "every mean must be finite";
    return nullptr;
}
static LombPlan lomb_plan_now(int64_t N, int64_t M, int64_t batch) {
    return lomb_plan_of(N, M, batch, g.ncu, env_int("SP_LOMB_FREQS", 0), std::min(env_int("SP_LOMB_SPLIT", 0), 65535));
}
static size_t lomb_up(size_t v) { return (v + 255) & ~(size_t)255; }

int sp_lomb_plan(int64_t N, int64_t M, int64_t batch, int64_t out[5]) {
    if (!out || lomb_shape(N, M, batch)) return -1;
    const LombPlan p = lomb_plan_now(N, M, batch);
    out[0] = p.R;
    out[1] = p.fpass;
    out[2] = p.passes;
    out[3] = p.split;
    out[4] = p.workgroups;
    return 0;
}

// f[M] (null: none) and mean[batch] behind one another at `at` in g_lombRec (sized by the caller), on the stream
static int lomb_upload(size_t at, const double *f, int64_t M, const double *mean, int64_t batch, const double **f_d, const double **mean_d) {
    char *base = (char *)g_lombRec.p + at;
    if (f) HIPCHK(hipMemcpyAsync(base, f, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, g.stream));
    *f_d = f ? (const double *)base : nullptr;
    *mean_d = nullptr;
    if (mean && batch > 0) {
        char *mp = base + lomb_up(sizeof(double) * (size_t)M);
        HIPCHK(hipMemcpyAsync(mp, mean, sizeof(double) * (size_t)batch, hipMemcpyHostToDevice, g.stream));
        *mean_d = (const double *)mp;
    }
    return 0;
}

// the record prepared in g_lombRec beside the call's small tables (f null: no frequency list), and what it must not hold looked
// for: 0, -1, or SP_LOMB_BAD_RECORD with nothing written anywhere else
struct LombRec {
    LombPrepArgs pa;
    const double *f_d, *mean_d;
};
static int lomb_prepare(const char *who, const LombPlan &p, const double *t_d, const double *w_d, const float *y_d, int64_t y_ld, int64_t N,
                        int64_t batch, double t_ref, double wnorm, const double *f, int64_t M, const double *mean, LombRec *out) {
    const int64_t npad = lomb_npad(N), nt = 1 + 2 * batch;
    // the prepared record and the call's small tables, each at a multiple of 256 bytes
    const size_t o_head = 0, o_wy = o_head + lomb_up(sizeof(LombHead) * (size_t)npad);
    const size_t o_wpart = o_wy + lomb_up(sizeof(float) * (size_t)p.groups * (size_t)npad * (size_t)p.RP);
    const size_t o_tpart = o_wpart + lomb_up(sizeof(double) * LOMB_PREP_BLOCKS);
    const size_t o_tot = o_tpart + lomb_up(sizeof(double) * (size_t)nt * LOMB_PREP_BLOCKS);
    const size_t o_status = o_tot + lomb_up(sizeof(double) * (size_t)nt);
    const size_t o_f = o_status + 256;
    const size_t total = o_f + lomb_up(sizeof(double) * (size_t)M) + lomb_up(sizeof(double) * (size_t)(batch + 1));
    if (g_lombRec.ensure(total)) return -1;
    char *rec = (char *)g_lombRec.p;
    const double *f_d, *mean_d;
    if (lomb_upload(o_f, f, M, mean, batch, &f_d, &mean_d)) return -1;
    LombPrepArgs pa{};
    pa.t = t_d, pa.w = w_d, pa.y = y_d;
    pa.y_ld = y_ld, pa.N = N, pa.npad = npad, pa.batch = batch, pa.rows_padded = p.R ? p.groups * p.RP : 0;
    pa.R = p.R, pa.RP = p.RP;
    pa.t_ref = t_ref, pa.wnorm = wnorm;
    pa.mean = mean_d;
    pa.blocks = p.prep_blocks, pa.len = p.prep_len;
    pa.wpart = (double *)(rec + o_wpart);
    pa.head = (LombHead *)(rec + o_head);
    pa.wy = p.RP ? (float *)(rec + o_wy) : nullptr;
    pa.tpart = (double *)(rec + o_tpart);
    pa.totals = (double *)(rec + o_tot);
    pa.status = (int *)(rec + o_status);
    HIPCHK(hipMemsetAsync(pa.status, 0, 4 * sizeof(int), g.stream));
    if (launch_lomb_prep(lc(), pa) != 0) return fail("%s: the record could not be prepared (N %lld, batch %lld)", who, (long long)N, (long long)batch);
    HIPCHK(hipGetLastError());
    int flags[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(flags, pa.status, sizeof flags, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (flags[0]) return fail("%s: t holds a value that is not finite", who), SP_LOMB_BAD_RECORD;
    if (flags[1]) return fail("%s: w holds a weight that is negative or not finite", who), SP_LOMB_BAD_RECORD;
    if (flags[2]) return fail("%s: the weights (w, or wnorm) do not sum to a positive finite value", who), SP_LOMB_BAD_RECORD;
    if (flags[3]) return fail("%s: y holds a value that is not finite", who), SP_LOMB_BAD_RECORD;
    out->pa = pa, out->f_d = f_d, out->mean_d = mean_d;
    return 0;
}

// sp_lomb (P given) and sp_lomb_sums (common, rows, totals given): the record prepared, then for every pass of frequencies the
// sums kernel over the row groups, their runs added, and for sp_lomb the finish step
static int lomb_run(const char *who, const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref,
                    double wnorm, const double *f, int64_t M, const double *mean, int floating_mean, int normalize, void *P, double *common,
                    double *rows, double *totals, int mem) {
    const bool sums_only = P == nullptr;
    // every refusal comes before the device is touched
    if (const char *why = lomb_shape(N, M, batch))
        return fail("%s: %s (N %lld, M %lld, batch %lld)", who, why, (long long)N, (long long)M, (long long)batch);
    if (batch > 0 && y_ld < N) return fail("%s: y_ld = %lld is below N = %lld", who, (long long)y_ld, (long long)N);
    if (normalize < 0 || normalize > 2) return fail("%s: normalize = %d must be 0 (power), 1 (normalize) or 2 (amplitude)", who, normalize);
    if (!t) return fail("%s: t is required", who);
    if (batch > 0 && !y) return fail("%s: y is required", who);
    if (!f) return fail("%s: f is required", who);
    if (!isfinite(wnorm)) return fail("%s: wnorm must be finite", who);
    int64_t where;
    if (const char *why = lomb_tables(f, M, t_ref, mean, batch, &where)) return fail("%s: %s (index %lld)", who, why, (long long)where);
    if (!sums_only && batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const LombPlan p = lomb_plan_now(N, M, batch);
    if (batch == 0) y = nullptr;
    const size_t esz = normalize == 2 ? sizeof(cf) : sizeof(float);
    const int64_t npad = lomb_npad(N), nt = 1 + 2 * batch;
    Stage st(mem);
    const double *t_d, *w_d;
    const float *y_d;
    double *common_d = nullptr, *rows_d = nullptr, *totals_d = nullptr;
    char *P_d = nullptr;
    st.in(g.in0, t, sizeof(double) * (size_t)N, &t_d);
    st.in(g.in0, w, sizeof(double) * (size_t)N, &w_d);
    st.in(g.in0, y, sizeof(float) * (size_t)((batch - 1) * y_ld + N), &y_d);
    if (sums_only) {
        st.out(g.out0, common, sizeof(double) * 4 * (size_t)M, &common_d);
        st.out(g.out0, batch > 0 ? rows : nullptr, sizeof(double) * 2 * (size_t)batch * (size_t)M, &rows_d);
        st.out(g.out0, totals, sizeof(double) * (size_t)nt, &totals_d);
    } else {
        st.out(g.out0, (char *)P, esz * (size_t)batch * (size_t)M, &P_d);
    }
    if (st.commit()) return -1;
    LombRec rec;
    if (const int rc = lomb_prepare(who, p, t_d, w_d, y_d, y_ld, N, batch, t_ref, wnorm, f, M, mean, &rec)) return rc;
    const LombPrepArgs &pa = rec.pa;
    const double *f_d = rec.f_d, *mean_d = rec.mean_d;
    if (sums_only) HIPCHK(hipMemcpyAsync(totals_d, pa.totals, sizeof(double) * (size_t)nt, hipMemcpyDeviceToDevice, g.stream));
    if (g.work.ensure(sizeof(double) * (size_t)p.gpl * (size_t)p.split * (size_t)p.nv * (size_t)p.fpass)) return -1;
    double *sc_common = nullptr, *sc_rows = nullptr;
    if (!sums_only) {
        if (g_lombSums.ensure(sizeof(double) * (size_t)p.fpass * (size_t)(4 + 2 * batch))) return -1;
        sc_common = (double *)g_lombSums.p;
        sc_rows = sc_common + 4 * p.fpass;
    }
    for (int64_t m0 = 0; m0 < M; m0 += p.fpass, ++g_passes[3]) {
        const int fc = (int)std::min<int64_t>(p.fpass, M - m0);
        double *cm = sums_only ? common_d + 4 * m0 : sc_common;
        double *rw = sums_only ? (rows_d ? rows_d + 2 * m0 : nullptr) : sc_rows;
        const int64_t rld = sums_only ? M : p.fpass;
        int launches = 0;
        for (int64_t g0 = 0; g0 < p.groups; g0 += p.gpl, g_passes[4] = std::max(g_passes[4], ++launches)) {
            const int64_t ng = std::min<int64_t>(p.gpl, p.groups - g0);
            LombSumArgs a{};
            a.head = pa.head;
            a.wy = p.RP ? pa.wy + g0 * npad * p.RP : nullptr;
            a.f = f_d + m0;
            a.npad = npad, a.N4 = (N + 3) / 4 * 4, a.run_len = p.run_len, a.split = p.split;
            a.fcount = fc;
            a.partial = (double *)g.work.p;
            {
                ProfScope ps;
                if (launch_lomb_sums(lc(), a, p.R, ng) != 0)
                    return fail("%s: the launch was refused (%d frequencies, %lld runs of %lld samples, %lld row groups)", who, fc,
                                (long long)p.split, (long long)p.run_len, (long long)ng);
            }
            HIPCHK(hipGetLastError());
            g.last_kernel = "k_lomb_sums";
            if (launch_lomb_reduce(lc(), a.partial, p.R, ng, p.split, fc, g0, batch, g0 == 0 ? cm : nullptr, rw, rld) != 0)
                return fail("%s: the sum over the runs was refused", who);
            HIPCHK(hipGetLastError());
        }
        if (!sums_only) {
            if (launch_lomb_finish(lc(), cm, rw, rld, pa.totals, mean_d, f_d + m0, fc, batch, N, t_ref, floating_mean, normalize,
                                   P_d + esz * (size_t)m0, M) != 0)
                return fail("%s: the finish step was refused", who);
            HIPCHK(hipGetLastError());
        }
    }
    return st.finish();
}

int sp_lomb(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, const double *f,
            int64_t M, const double *mean, int floating_mean, int normalize, void *P, int mem) {
    if (!P) return fail("sp_lomb: P is required");
    return lomb_run("sp_lomb", t, w, y, y_ld, N, batch, t_ref, 0.0, f, M, mean, floating_mean, normalize, P, nullptr, nullptr, nullptr, mem);
}

int sp_lomb_sums(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, double wnorm,
                 const double *f, int64_t M, const double *mean, double *common, double *rows, double *totals, int mem) {
    if (!common) return fail("sp_lomb_sums: common is required");
    if (!totals) return fail("sp_lomb_sums: totals is required");
    if (batch > 0 && !rows) return fail("sp_lomb_sums: rows is required");
    return lomb_run("sp_lomb_sums", t, w, y, y_ld, N, batch, t_ref, wnorm, f, M, mean, 0, 0, nullptr, common, rows, totals, mem);
}

int sp_lomb_finish(const double *common, const double *rows, const double *totals, int64_t N, int64_t batch, double t_ref,
                   const double *f, int64_t M, const double *mean, int floating_mean, int normalize, void *P, int mem) {
    const char *who = "sp_lomb_finish";
    if (const char *why = lomb_shape(N, M, batch))
        return fail("%s: %s (N %lld, M %lld, batch %lld)", who, why, (long long)N, (long long)M, (long long)batch);
    if (normalize < 0 || normalize > 2) return fail("%s: normalize = %d must be 0 (power), 1 (normalize) or 2 (amplitude)", who, normalize);
    if (!common) return fail("%s: common is required", who);
    if (!rows) return fail("%s: rows is required", who);
    if (!totals) return fail("%s: totals is required", who);
    if (!f) return fail("%s: f is required", who);
    if (!P) return fail("%s: P is required", who);
    int64_t where;
    if (const char *why = lomb_tables(f, M, t_ref, mean, batch, &where)) return fail("%s: %s (index %lld)", who, why, (long long)where);
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t esz = normalize == 2 ? sizeof(cf) : sizeof(float);
    Stage st(mem);
    const double *common_d, *rows_d, *totals_d;
    char *P_d;
    st.in(g.in0, common, sizeof(double) * 4 * (size_t)M, &common_d);
    st.in(g.in0, rows, sizeof(double) * 2 * (size_t)batch * (size_t)M, &rows_d);
    st.in(g.in0, totals, sizeof(double) * (size_t)(1 + 2 * batch), &totals_d);
    st.out(g.out0, (char *)P, esz * (size_t)batch * (size_t)M, &P_d);
    if (st.commit()) return -1;
    if (g_lombRec.ensure(lomb_up(sizeof(double) * (size_t)M) + lomb_up(sizeof(double) * (size_t)(batch + 1)))) return -1;
    const double *f_d, *mean_d;
    if (lomb_upload(0, f, M, mean, batch, &f_d, &mean_d)) return -1;
    if (launch_lomb_finish(lc(), common_d, rows_d, M, totals_d, mean_d, f_d, (int)M, batch, N, t_ref, floating_mean, normalize, P_d, M) != 0)
        return fail("%s: the finish step was refused", who);
    HIPCHK(hipGetLastError());
    if (!st.host) HIPCHK(hipStreamSynchronize(g.stream));       // f and mean are the caller's again
    return st.finish();
}

// ---- type-1 NUFFT and the Lomb-Scargle sums on a uniform frequency grid (k_nufft.hip; include/spectral_nufft.h) ----------
static const char *nufft_shape(int64_t N, int64_t M, int64_t batch) {
    if (const char *why = lomb_shape(N, M, batch)) return why;
    if (nufft_nf(M) > NUFFT_MAX_NF) return "the fine grid of next_pow2(2 M) cells is beyond 2^26";
    return nullptr;
}
// fc = f0 + (M / 2) df, the centre of the modes; 0 or the message's tail
static const char *nufft_grid_args(double t_ref, double f0, double df, int64_t M, double *fc) {
    if (!isfinite(t_ref)) return "t_ref must be finite";
    if (!isfinite(f0)) return "f0 must be finite";
    if (!isfinite(df)) return "df must be finite";
    if (df == 0.0) return "df must not be zero";
    *fc = f0 + (double)(M / 2) * df;
    if (!isfinite(2.0 * *fc) || !isfinite(f0 + (double)M * df)) return "f0 + M df must be finite";
    return nullptr;
}
static NufftPlan nufft_plan_now(int64_t M, int64_t rows) { return nufft_plan_of(M, rows, NUFFT_GRID_BYTES, env_int("SP_NUFFT_ROWS", 0)); }

int sp_nufft1_plan(int64_t N, int64_t M, int64_t batch, int64_t out[8]) {
    if (!out || nufft_shape(N, M, batch)) return -1;
    const NufftPlan p = nufft_plan_now(M, batch);
    out[0] = p.nf;
    out[1] = NUFFT_W;
    out[2] = p.tiles;
    out[3] = NUFFT_TILE;
    out[4] = p.rpp;
    out[5] = p.passes;
    out[6] = p.workgroups;
    out[7] = LOMB_FAST_MIN_PAIRS;
    return 0;
}

struct NufftWork {
    NufftRec *rec;                  // [sets][N]
    unsigned *count;                // [sets][tiles]
    int64_t *off;                   // [sets][tiles + 1]
    int *list;                      // [sets][2 N]
    int *shift;                     // [rows]
    int flags[2];                   // read back: a time, a strength that is not finite
};
// the samples of `sets` position sets prepared and entered into their tile lists, the shifts of `rows` rows taken, and the status read
// back (one synchronisation): everything the passes share.  src_n: the elements of a row of src the shift and the check for values that
// are not finite look at: N for strengths at the samples, M for the modes of the type-2 transform
static int nufft_prepare(const char *who, const double *t_d, int64_t N, double t_ref, int sets, const double *q, const double *fc,
                         const NufftPlan &p, const NufftSrc &src, int64_t rows, int64_t src_n, NufftWork *w) {
    const size_t o_rec = 0, o_list = o_rec + lomb_up(sizeof(NufftRec) * (size_t)sets * (size_t)N);
    const size_t o_count = o_list + lomb_up(sizeof(int) * (size_t)sets * 2 * (size_t)N);
    const size_t o_off = o_count + lomb_up(sizeof(unsigned) * (size_t)sets * (size_t)p.tiles);
    const size_t o_shift = o_off + lomb_up(sizeof(int64_t) * (size_t)sets * (size_t)(p.tiles + 1));
    const size_t o_part = o_shift + lomb_up(sizeof(int) * (size_t)rows);
    const size_t o_status = o_part + lomb_up(sizeof(float) * (size_t)rows * (size_t)nufft_rowmax_blocks(src_n));
    if (g.nuRec.ensure(o_status + 256)) return -1;
    char *base = (char *)g.nuRec.p;
    w->rec = (NufftRec *)(base + o_rec);
    w->list = (int *)(base + o_list);
    w->count = (unsigned *)(base + o_count);
    w->off = (int64_t *)(base + o_off);
    w->shift = (int *)(base + o_shift);
    int *status = (int *)(base + o_status);
    HIPCHK(hipMemsetAsync(w->count, 0, sizeof(unsigned) * (size_t)sets * (size_t)p.tiles, g.stream));
    HIPCHK(hipMemsetAsync(status, 0, 2 * sizeof(int), g.stream));
    NufftPrepArgs a{};
    a.t = t_d, a.N = N, a.nf = p.nf, a.tiles = p.tiles, a.t_ref = t_ref, a.sets = sets;
    for (int s = 0; s < sets; ++s) a.q[s] = q[s], a.fc[s] = fc[s];
    a.rec = w->rec, a.count = w->count, a.status = status;
    if (launch_nufft_prep(lc(), a) != 0) return fail("%s: the samples could not be prepared (N %lld, nf %lld)", who, (long long)N, (long long)p.nf);
    HIPCHK(hipGetLastError());
    if (launch_nufft_rowshift(lc(), src, rows, src_n, (float *)(base + o_part), w->shift, status) != 0) return fail("%s: the rows' shifts could not be taken", who);
    HIPCHK(hipGetLastError());
    for (int s = 0; s < sets; ++s) {
        if (launch_nufft_bin(lc(), w->rec + (int64_t)s * N, N, p.nf, w->count + (int64_t)s * p.tiles, w->off + (int64_t)s * (p.tiles + 1),
                             w->list + (int64_t)s * 2 * N) != 0)
            return fail("%s: the tile lists could not be filled", who);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(w->flags, status, sizeof w->flags, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    return 0;
}
// rows row0 .. row0 + nrows - 1 of position set `set` spread onto the pass's grids and transformed in place
static int nufft_grids(const char *who, const NufftWork &w, int set, const NufftSrc &src, int64_t N, int64_t row0, int64_t nrows,
                       const NufftPlan &p, bool timed) {
    NufftSpreadArgs a{};
    a.src = src, a.row0 = row0, a.nrows = (int)nrows, a.nf = p.nf;
    a.rec = w.rec + (int64_t)set * N, a.off = w.off + (int64_t)set * (p.tiles + 1), a.list = w.list + (int64_t)set * 2 * N;
    a.shift = w.shift, a.grid = (cf *)g.nuGrid.p;
    int rc;
    if (timed) {                    // the profile keeps the spread of the rows, not the one-row spread of A2 behind it
        ProfScope ps;
        rc = launch_nufft_spread(lc(), a);
    } else {
        rc = launch_nufft_spread(lc(), a);
    }
    if (rc != 0)
        return fail("%s: the spread was refused (%lld rows from %lld on %lld cells)", who, (long long)nrows, (long long)row0, (long long)p.nf);
    HIPCHK(hipGetLastError());
    g.last_kernel = "k_nufft_spread";
    return dev_fft_any(a.grid, a.grid, p.nf, nrows, 0);
}

int sp_nufft1(const double *t, const void *c, int64_t c_ld, int64_t N, int64_t batch, double t_ref, double f0, double df, int64_t M,
              int sign, void *out, int mem) {
    const char *who = "sp_nufft1";
    if (const char *why = nufft_shape(N, M, batch))
        return fail("%s: %s (N %lld, M %lld, batch %lld)", who, why, (long long)N, (long long)M, (long long)batch);
    if (c_ld < N) return fail("%s: c_ld = %lld is below N = %lld", who, (long long)c_ld, (long long)N);
    if (sign != 1 && sign != -1) return fail("%s: sign = %d must be +1 or -1", who, sign);
    double fc;
    if (const char *why = nufft_grid_args(t_ref, f0, df, M, &fc)) return fail("%s: %s", who, why);
    if (!t) return fail("%s: t is required", who);
    if (!c) return fail("%s: c is required", who);
    if (!out) return fail("%s: out is required", who);
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const NufftPlan p = nufft_plan_now(M, batch);
    Stage st(mem);
    const double *t_d;
    const cf *c_d;
    cf *out_d;
    st.in(g.in0, t, sizeof(double) * (size_t)N, &t_d);
    st.in(g.in0, (const cf *)c, sizeof(cf) * (size_t)((batch - 1) * c_ld + N), &c_d);
    st.out(g.out0, (cf *)out, sizeof(cf) * (size_t)batch * (size_t)M, &out_d);
    if (st.commit()) return -1;
    NufftSrc src{};
    src.c = c_d, src.c_ld = c_ld;
    const double q = -(double)sign * df, fcs = (double)sign * fc;
    NufftWork w;
    if (nufft_prepare(who, t_d, N, t_ref, 1, &q, &fcs, p, src, batch, N, &w)) return -1;
    if (w.flags[0]) return fail("%s: t holds a value that is not finite, or one whose product with df or f0 is not", who), SP_NUFFT_BAD_RECORD;
    if (w.flags[1]) return fail("%s: c holds a value that is not finite", who), SP_NUFFT_BAD_RECORD;
    if (g.nuGrid.ensure(sizeof(cf) * (size_t)p.rpp * (size_t)p.nf)) return -1;
    const NufftQuad quad = nufft_quad(p.nf);
    for (int64_t r0 = 0; r0 < batch; r0 += p.rpp, ++g_passes[6]) {
        const int64_t nr = std::min<int64_t>(p.rpp, batch - r0);
        if (nufft_grids(who, w, 0, src, N, r0, nr, p, true)) return -1;
        if (launch_nufft_pick(lc(), (const cf *)g.nuGrid.p, p.nf, M, nr, quad, true, out_d + r0 * M, M, 1) != 0)
            return fail("%s: the pick was refused", who);
        HIPCHK(hipGetLastError());
    }
    return st.finish();
}

int sp_lomb_sums_grid(const double *t, const double *w, const float *y, int64_t y_ld, int64_t N, int64_t batch, double t_ref, double wnorm,
                      double f0, double df, int64_t M, const double *mean, double *common, double *rows, double *totals, int mem) {
    const char *who = "sp_lomb_sums_grid";
    if (const char *why = nufft_shape(N, M, batch))
        return fail("%s: %s (N %lld, M %lld, batch %lld)", who, why, (long long)N, (long long)M, (long long)batch);
    if (batch > 0 && y_ld < N) return fail("%s: y_ld = %lld is below N = %lld", who, (long long)y_ld, (long long)N);
    double fc;
    if (const char *why = nufft_grid_args(t_ref, f0, df, M, &fc)) return fail("%s: %s", who, why);
    if (!isfinite(wnorm)) return fail("%s: wnorm must be finite", who);
    for (int64_t b = 0; mean && b < batch; ++b)
        if (!isfinite(mean[b])) return fail("%s: every mean must be finite (index %lld)", who, (long long)b);
    if (!t) return fail("%s: t is required", who);
    if (batch > 0 && !y) return fail("%s: y is required", who);
    if (!common) return fail("%s: common is required", who);
    if (!totals) return fail("%s: totals is required", who);
    if (batch > 0 && !rows) return fail("%s: rows is required", who);
    if (ensure_init()) return -1;
    ApiLock lk;
    const LombPlan lp = lomb_plan_now(N, M, batch);                 // its row groups and prep blocks: the record sp_lomb_sums prepares
    const NufftPlan p = nufft_plan_now(M, 1 + batch);
    if (batch == 0) y = nullptr;
    const int64_t nt = 1 + 2 * batch;
    Stage st(mem);
    const double *t_d, *w_d;
    const float *y_d;
    double *common_d = nullptr, *rows_d = nullptr, *totals_d = nullptr;
    st.in(g.in0, t, sizeof(double) * (size_t)N, &t_d);
    st.in(g.in0, w, sizeof(double) * (size_t)N, &w_d);
    st.in(g.in0, y, sizeof(float) * (size_t)((batch - 1) * y_ld + N), &y_d);
    st.out(g.out0, common, sizeof(double) * 4 * (size_t)M, &common_d);
    st.out(g.out0, batch > 0 ? rows : nullptr, sizeof(double) * 2 * (size_t)batch * (size_t)M, &rows_d);
    st.out(g.out0, totals, sizeof(double) * (size_t)nt, &totals_d);
    if (st.commit()) return -1;
    LombRec rec;
    if (const int rc = lomb_prepare(who, lp, t_d, w_d, y_d, y_ld, N, batch, t_ref, wnorm, nullptr, 0, mean, &rec)) return rc;
    NufftSrc src{};
    src.head = rec.pa.head, src.wy = rec.pa.wy, src.npad = rec.pa.npad, src.R = lp.R ? lp.R : 1, src.RP = lp.RP ? lp.RP : 1;
    const double q[2] = {-df, -2.0 * df}, fcs[2] = {fc, 2.0 * fc};
    NufftWork wk;
    if (nufft_prepare(who, t_d, N, t_ref, 2, q, fcs, p, src, 1 + batch, N, &wk)) return -1;
    if (wk.flags[0]) return fail("%s: a time's product with df or f0 is not finite", who), SP_LOMB_BAD_RECORD;
    if (wk.flags[1]) return fail("%s: a weight or a value leaves float32 once the weights are normalised", who), SP_LOMB_BAD_RECORD;
    HIPCHK(hipMemcpyAsync(totals_d, rec.pa.totals, sizeof(double) * (size_t)nt, hipMemcpyDeviceToDevice, g.stream));
    if (g.nuGrid.ensure(sizeof(cf) * (size_t)p.rpp * (size_t)p.nf)) return -1;
    const cf *grid = (const cf *)g.nuGrid.p;
    const NufftQuad quad = nufft_quad(p.nf);
    // A1 and the B_r: row 0 is w32, row 1 + r is wy32_r, under the positions of phi
    for (int64_t r0 = 0; r0 < 1 + batch; r0 += p.rpp, ++g_passes[6]) {
        const int64_t nr = std::min<int64_t>(p.rpp, 1 + batch - r0);
        if (nufft_grids(who, wk, 0, src, N, r0, nr, p, true)) return -1;
        const int64_t lead = r0 == 0 ? 1 : 0;                       // the pass's rows that go to common
        if (lead && launch_nufft_pick(lc(), grid, p.nf, M, 1, quad, false, common_d, 0, 4) != 0) return fail("%s: the pick was refused", who);
        if (nr > lead &&
            launch_nufft_pick(lc(), grid + lead * p.nf, p.nf, M, nr - lead, quad, false, rows_d + 2 * M * (r0 + lead - 1), 2 * M, 2) != 0)
            return fail("%s: the pick was refused", who);
        HIPCHK(hipGetLastError());
    }
    // A2: w32 under the doubled positions, on the same grid length
    if (nufft_grids(who, wk, 1, src, N, 0, 1, p, false)) return -1;
    if (launch_nufft_pick(lc(), grid, p.nf, M, 1, quad, false, common_d + 2, 0, 4) != 0) return fail("%s: the pick was refused", who);
    HIPCHK(hipGetLastError());
    return st.finish();
}

// ---- type-2 NUFFT (k_nufft2.hip; include/spectral_nufft2.h): the parts of type 1 above, run the other way ------------------------
static int64_t nufft2_workgroups(const NufftPlan &p, int64_t rows) {
    int64_t n = 0;
    for (int64_t r0 = 0; r0 < rows; r0 += p.rpp) n += p.tiles * ((std::min<int64_t>(p.rpp, rows - r0) + NUFFT2_RG - 1) / NUFFT2_RG);
    return n;
}

int sp_nufft2_plan(int64_t N, int64_t M, int64_t batch, int64_t out[8]) {
    if (!out || nufft_shape(N, M, batch)) return -1;
    const NufftPlan p = nufft_plan_now(M, batch);
    out[0] = p.nf;
    out[1] = NUFFT_W;
    out[2] = p.tiles;
    out[3] = NUFFT_TILE;
    out[4] = p.rpp;
    out[5] = p.passes;
    out[6] = nufft2_workgroups(p, batch);
    out[7] = NUFFT2_RG;
    return 0;
}

int sp_nufft2(const double *t, const void *F, int64_t F_ld, int64_t N, int64_t batch, double t_ref, double f0, double df, int64_t M,
              int sign, void *out, int64_t out_ld, int mem) {
    const char *who = "sp_nufft2";
    if (const char *why = nufft_shape(N, M, batch))
        return fail("%s: %s (N %lld, M %lld, batch %lld)", who, why, (long long)N, (long long)M, (long long)batch);
    if (F_ld < M) return fail("%s: F_ld = %lld is below M = %lld", who, (long long)F_ld, (long long)M);
    if (out_ld < N) return fail("%s: out_ld = %lld is below N = %lld", who, (long long)out_ld, (long long)N);
    if (sign != 1 && sign != -1) return fail("%s: sign = %d must be +1 or -1", who, sign);
    double fc;
    if (const char *why = nufft_grid_args(t_ref, f0, df, M, &fc)) return fail("%s: %s", who, why);
    if (!t) return fail("%s: t is required", who);
    if (!F) return fail("%s: F is required", who);
    if (!out) return fail("%s: out is required", who);
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const NufftPlan p = nufft_plan_now(M, batch);
    Stage st(mem);
    const double *t_d;
    const cf *F_d;
    cf *out_d;
    st.in(g.in0, t, sizeof(double) * (size_t)N, &t_d);
    st.in(g.in0, (const cf *)F, sizeof(cf) * (size_t)((batch - 1) * F_ld + M), &F_d);
    st.rows(g.out0, (cf *)out, sizeof(cf), batch, out_ld, N, &out_d);
    if (st.commit()) return -1;
    NufftSrc src{};
    src.c = F_d, src.c_ld = F_ld;                                   // the row-shift step's source: its status word finds modes that are not finite
    const double q = -(double)sign * df, fcs = (double)sign * fc;
    NufftWork w;
    if (nufft_prepare(who, t_d, N, t_ref, 1, &q, &fcs, p, src, batch, M, &w)) return -1;
    if (w.flags[0]) return fail("%s: t holds a value that is not finite, or one whose product with df or f0 is not", who), SP_NUFFT_BAD_RECORD;
    if (w.flags[1]) return fail("%s: F holds a value that is not finite", who), SP_NUFFT_BAD_RECORD;
    if (g.nuGrid.ensure(sizeof(cf) * (size_t)p.rpp * (size_t)p.nf)) return -1;
    const NufftQuad quad = nufft_quad(p.nf);
    cf *grid = (cf *)g.nuGrid.p;
    for (int64_t r0 = 0; r0 < batch; r0 += p.rpp, ++g_passes[6]) {
        const int64_t nr = std::min<int64_t>(p.rpp, batch - r0);
        if (launch_nufft2_place(lc(), F_d + r0 * F_ld, F_ld, M, nr, p.nf, quad, grid) != 0) return fail("%s: the placing of the modes was refused", who);
        HIPCHK(hipGetLastError());
        if (dev_fft_any(grid, grid, p.nf, nr, 0)) return -1;
        Nufft2InterpArgs a{};
        a.grid = grid, a.nrows = (int)nr, a.nf = p.nf, a.N = N;
        a.rec = w.rec, a.off = w.off, a.list = w.list;
        a.out = out_d + r0 * out_ld, a.out_ld = out_ld;
        int rc;
        {
            ProfScope ps;
            rc = launch_nufft2_interp(lc(), a);
        }
        if (rc != 0)
            return fail("%s: the interpolation was refused (%lld rows from %lld on %lld cells)", who, (long long)nr, (long long)r0, (long long)p.nf);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_nufft2_interp";
    }
    return st.finish();
}

// ---- autoregressive fits and spectra (k_burg.hip; include/spectral_ar.h; the host's arithmetic in ar_plan.h) --------------------
static ArPlan ar_plan_now(int method, bool cplx, int64_t n, int order, int64_t segs) {
    return ar_plan_of(method, cplx, n, order, segs, env_int("SP_BURG_FORM", 0), env_int("SP_AR_SEGS", 0));
}

int sp_ar_plan(int method, int dtype, int64_t n, int order, int64_t batch, int64_t nframes, int64_t out[8]) {
    if (!out || (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) || ar_shape(method, n, order, batch, nframes)) return -1;
    const ArPlan p = ar_plan_now(method, dtype == SP_DTYPE_C64, n, order, batch * nframes);
    out[0] = p.form;
    out[1] = p.segs_per_wg;
    out[2] = method == AR_METHOD_BURG ? p.spl : p.chunk;
    out[3] = p.lds_bytes;
    out[4] = p.workgroups;
    out[5] = p.passes;
    out[6] = p.threads;
    out[7] = p.tiles;
    return 0;
}

// The front of the entries that work on a framed record -- the fits here, the covariance entries below: what they refuse about the
// record, the look at it, and what opens every pass.
//
// the refusals about the frames, the pitch, the detrending and the record itself, in one order; 0 or -1
static int frames_refusals(const char *who, const void *x, int64_t x_ld, int64_t nsig, int64_t n, int64_t hop, int64_t first, int64_t nframes, int detrend,
                           double mean_re, double mean_im) {
    if (hop < 1) return fail("%s: hop = %lld must be at least 1", who, (long long)hop);
    if (first < 0) return fail("%s: first = %lld must not be negative", who, (long long)first);
    if (nsig < 1 || nsig > ((int64_t)1 << 40)) return fail("%s: nsig = %lld must lie in 1 .. 2^40", who, (long long)nsig);
    if (nframes > 0 && (first > nsig - n || (nframes - 1) > (nsig - n - first) / hop))
        return fail("%s: %lld frames of %lld at hop %lld from %lld on reach outside the %lld samples of a row", who, (long long)nframes, (long long)n,
                    (long long)hop, (long long)first, (long long)nsig);
    if (x_ld < nsig) return fail("%s: x_ld = %lld is below nsig = %lld", who, (long long)x_ld, (long long)nsig);
    if (detrend != SP_DETREND_CONST && detrend != SP_DETREND_SEGMEAN) return fail("%s: detrend = %d must be SP_DETREND_CONST or SP_DETREND_SEGMEAN", who, detrend);
    if (!std::isfinite(mean_re) || !std::isfinite(mean_im)) return fail("%s: the mean must be finite", who);
    if (!x) return fail("%s: x is required", who);
    return 0;
}

// the small scratch (g.arSmall): the flag of the look; with `means` behind it, at 256, the means of a pass and then its tiles' sums
struct ArSmall {
    int *flag;
    double *mean, *sums;
};

extern "C++" {   // two templates: p is the entry's plan (ArPlan, SubPlan), pass a lambda of the entry
// the look at the record: every segment is looked at before anything is written; one pass keeps the sums of that look.  pass(s0)
// sets A to the pass that begins with segment s0.  0, -1 or SP_AR_BAD_RECORD
template <class Plan, class Pass>
static int ar_look(const char *who, const ArArgs &A, Pass pass, int64_t segs, const Plan &p, bool means, bool want_sums, ArSmall *s) {
    const size_t o_mean = 256, o_sums = o_mean + lomb_up(16 * (size_t)p.spp);
    if (g.arSmall.ensure(means ? o_sums + 16 * (size_t)p.spp * (size_t)p.tiles + 256 : o_mean)) return -1;
    s->flag = (int *)g.arSmall.p;
    s->mean = (double *)((char *)g.arSmall.p + o_mean), s->sums = (double *)((char *)g.arSmall.p + o_sums);
    HIPCHK(hipMemsetAsync(s->flag, 0, sizeof(int), g.stream));
    for (int64_t s0 = 0; s0 < segs; s0 += p.spp) {
        pass(s0);
        if (launch_ar_scan(lc(), A, p.chunk, p.tiles, p.passes == 1 && want_sums ? s->sums : nullptr, s->flag) != 0)
            return fail("%s: the look at the record was refused", who);
        HIPCHK(hipGetLastError());
    }
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, s->flag, sizeof(int), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    if (bad) return fail("%s: x holds a value that is not finite", who), SP_AR_BAD_RECORD;
    return 0;
}

// what opens a pass: the tiles' sums if there are several passes, then the means
template <class Plan> static int ar_pass_means(const char *who, const ArArgs &A, const Plan &p, bool want_sums, const ArSmall &s) {
    if (want_sums && p.passes > 1) {
        if (launch_ar_scan(lc(), A, p.chunk, p.tiles, s.sums, s.flag) != 0) return fail("%s: the tiles' sums were refused", who);
        HIPCHK(hipGetLastError());
    }
    if (launch_ar_mean(lc(), A, p.tiles, want_sums ? s.sums : nullptr, s.mean) != 0) return fail("%s: the means were refused", who);
    HIPCHK(hipGetLastError());
    return 0;
}
}   // extern "C++"

static int ar_fit(const char *who, int method, const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop,
                  int64_t first, int64_t nframes, int order, int detrend, double mean_re, double mean_im, void *a, double *evar, void *k,
                  int64_t out_ld, int mem) {
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("%s: dtype = %d must be SP_DTYPE_F32 or SP_DTYPE_C64", who, dtype);
    if (const char *why = ar_shape(method, n, order, batch, nframes))
        return fail("%s: %s (n %lld, order %d, batch %lld, nframes %lld)", who, why, (long long)n, order, (long long)batch, (long long)nframes);
    if (frames_refusals(who, x, x_ld, nsig, n, hop, first, nframes, detrend, mean_re, mean_im)) return -1;
    if (out_ld < order + 1) return fail("%s: out_ld = %lld is below order + 1 = %d", who, (long long)out_ld, order + 1);
    if (!a) return fail("%s: a is required", who);
    if (!evar) return fail("%s: evar is required", who);
    if (!k) return fail("%s: k is required", who);
    const int64_t segs = batch * nframes;
    if (segs == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64;
    const ArPlan p = ar_plan_now(method, cplx, n, order, segs);
    const size_t xel = cplx ? 8 : 4, el = cplx ? 16 : 8;
    Stage st(mem);
    const char *x_d;
    char *a_d, *k_d;
    double *e_d;
    st.in(g.in0, (const char *)x, xel * (size_t)((batch - 1) * x_ld + nsig), &x_d);
    st.rows(g.out0, (char *)a, el, segs, out_ld, order + 1, &a_d);
    st.rows(g.out0, evar, 8, segs, out_ld, order + 1, &e_d);
    st.rows(g.out0, (char *)k, el, segs, out_ld, order, &k_d, segs > 1);   // rows of `order` at a pitch of at least order + 1: room wherever there are two
    if (st.commit()) return -1;
    const bool yule = method == AR_METHOD_YULE;
    const bool want_sums = yule && detrend == SP_DETREND_SEGMEAN;
    if (yule && g.arPart.ensure(el * (size_t)p.spp * (size_t)p.tiles * (size_t)(order + 1))) return -1;
    ArArgs A{};
    A.x = x_d, A.cplx = cplx, A.x_ld = x_ld, A.first = first, A.hop = hop, A.nframes = nframes, A.n = n;
    A.p = order;
    A.detrend = detrend == SP_DETREND_SEGMEAN ? 1 : ((mean_re != 0.0 || mean_im != 0.0) ? 2 : 0);
    A.mre = mean_re, A.mim = mean_im;
    A.out_ld = out_ld;
    auto pass = [&](int64_t s0) {
        A.seg0 = s0, A.nseg = std::min<int64_t>(p.spp, segs - s0);
        A.a = a_d + el * (size_t)(s0 * out_ld), A.e = e_d + s0 * out_ld, A.k = k_d + el * (size_t)(s0 * out_ld);
    };
    ArSmall sm;                                                     // Yule-Walker keeps means there; k_burg forms its own
    if (int rc = ar_look(who, A, pass, segs, p, yule, want_sums, &sm)) return rc;
    for (int64_t s0 = 0; s0 < segs; s0 += p.spp, ++g_passes[7]) {
        pass(s0);
        int rc;
        if (yule) {
            if (ar_pass_means(who, A, p, want_sums, sm)) return -1;
            {
                ProfScope ps;
                rc = launch_ar_lags(lc(), A, p.chunk, p.tiles, sm.mean, g.arPart.p);
            }
            if (rc != 0) return fail("%s: the lags were refused (%lld segments of %lld in %lld tiles)", who, (long long)A.nseg, (long long)n, (long long)p.tiles);
            HIPCHK(hipGetLastError());
            if (launch_levinson(lc(), A, p.tiles, g.arPart.p) != 0) return fail("%s: the Levinson recursion was refused", who);
            HIPCHK(hipGetLastError());
            g.last_kernel = "k_ar_lags";
        } else {
            {
                ProfScope ps;
                rc = launch_burg(lc(), A, p.spl, p.nw);
            }
            if (rc != 0) return fail("%s: no kernel for %lld samples (%d per lane, %d waves)", who, (long long)n, p.spl, p.nw);
            HIPCHK(hipGetLastError());
            g.last_kernel = "k_burg";
        }
    }
    return st.finish();
}

int sp_burg(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
            int order, int detrend, double mean_re, double mean_im, void *a, double *evar, void *k, int64_t out_ld, int mem) {
    return ar_fit("sp_burg", AR_METHOD_BURG, x, dtype, x_ld, nsig, batch, n, hop, first, nframes, order, detrend, mean_re, mean_im, a, evar, k,
                  out_ld, mem);
}

int sp_yule(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
            int order, int detrend, double mean_re, double mean_im, void *a, double *evar, void *k, int64_t out_ld, int mem) {
    return ar_fit("sp_yule", AR_METHOD_YULE, x, dtype, x_ld, nsig, batch, n, hop, first, nframes, order, detrend, mean_re, mean_im, a, evar, k,
                  out_ld, mem);
}

int sp_ar_psd(const void *a, int cplx, int64_t a_ld, const double *e, int64_t e_ld, int order, int64_t nmodels, int64_t m, double start,
              double step, double scale, int out64, void *P, int64_t P_ld, int mem) {
    const char *who = "sp_ar_psd";
    if (order < 0 || order > AR_MAX_ORDER) return fail("%s: order = %d must lie in 0 .. 256", who, order);
    if (a_ld < order + 1) return fail("%s: a_ld = %lld is below order + 1 = %d", who, (long long)a_ld, order + 1);
    if (e_ld < 1) return fail("%s: e_ld = %lld must be at least 1", who, (long long)e_ld);
    if (m < 1 || m > 0x7fffffff) return fail("%s: m = %lld must lie in 1 .. 2^31 - 1", who, (long long)m);
    if (P_ld < m) return fail("%s: P_ld = %lld is below m = %lld", who, (long long)P_ld, (long long)m);
    if (nmodels < 0 || (nmodels > 0 && (m + 255) / 256 > 0x7fffffff / nmodels))
        return fail("%s: nmodels = %lld must not be negative, nor nmodels x ceil(m / 256) exceed 2^31 - 1", who, (long long)nmodels);
    if (!std::isfinite(start) || !std::isfinite(step) || !std::isfinite(scale)) return fail("%s: start, step and scale must be finite", who);
    if (!a) return fail("%s: a is required", who);
    if (!e) return fail("%s: e is required", who);
    if (!P) return fail("%s: P is required", who);
    if (nmodels == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t el = cplx ? 16 : 8, pel = out64 ? 8 : 4;
    Stage st(mem);
    const char *a_d;
    const double *e_d;
    char *P_d;
    st.in(g.in0, (const char *)a, el * (size_t)((nmodels - 1) * a_ld + order + 1), &a_d);
    st.in(g.in0, e, 8 * (size_t)((nmodels - 1) * e_ld + 1), &e_d);
    st.rows(g.out0, (char *)P, pel, nmodels, P_ld, m, &P_d);
    if (st.commit()) return -1;
    int rc;
    {
        ProfScope ps;
        rc = launch_ar_psd(lc(), a_d, cplx != 0, a_ld, e_d, e_ld, order, nmodels, m, start, step, scale, out64 != 0, P_d, P_ld);
    }
    if (rc != 0) return fail("%s: the launch was refused (%lld models, %lld bins)", who, (long long)nmodels, (long long)m);
    HIPCHK(hipGetLastError());
    g.last_kernel = "k_ar_psd";
    return st.finish();
}

// ---- covariance matrices, covariance least-squares fits and pseudospectra (k_subspace.hip; include/spectral_sub.h; sub_plan.h) ------
static SubPlan sub_plan_now(int what, bool cplx, int64_t n, int m, int64_t segs) { return sub_plan_of(what, cplx, n, m, segs, env_int("SP_AR_SEGS", 0)); }

int sp_sub_plan(int what, int dtype, int64_t n, int m, int64_t batch, int64_t nframes, int64_t out[8]) {
    if (!out || (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) || sub_shape(what, n, m, batch, nframes)) return -1;
    const SubPlan p = sub_plan_now(what, dtype == SP_DTYPE_C64, n, m, batch * nframes);
    out[0] = p.chunk;
    out[1] = p.tiles;
    out[2] = p.nsub;
    out[3] = p.lds_bytes;
    out[4] = p.workgroups;
    out[5] = p.passes;
    out[6] = p.seg_bytes;
    out[7] = p.spp;
    return 0;
}

// what the two entries refuse about the record and the matrix order, in one order; 0 or -1
static int sub_refusals(const char *who, int what, const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first,
                        int64_t nframes, int m, int fb, int detrend, double mean_re, double mean_im) {
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("%s: dtype = %d must be SP_DTYPE_F32 or SP_DTYPE_C64", who, dtype);
    if (const char *why = sub_shape(what, n, m, batch, nframes))
        return fail("%s: %s (n %lld, %s %d, batch %lld, nframes %lld)", who, why, (long long)n, what == SUB_WHAT_LS ? "order" : "m", what == SUB_WHAT_LS ? m - 1 : m,
                    (long long)batch, (long long)nframes);
    if (fb != 0 && fb != 1) return fail("%s: fb = %d must be 0 (covariance) or 1 (modified covariance)", who, fb);
    return frames_refusals(who, x, x_ld, nsig, n, hop, first, nframes, detrend, mean_re, mean_im);
}

// the passes of both entries over staged pointers: the look at the record, then per pass the means, row 0 by tiles, the matrices (into
// C_d, or into scratch for a fit) and, for a fit, the Cholesky solves
static int sub_passes(const char *who, int what, const char *x_d, bool cplx, int64_t x_ld, int64_t segs, int64_t n, int64_t hop, int64_t first, int64_t nframes,
                      int m, int fb, int detrend, double mean_re, double mean_im, char *C_d, int64_t C_ld, char *a_d, double *e_d, int32_t *st_d, int64_t out_ld) {
    const SubPlan p = sub_plan_now(what, cplx, n, m, segs);
    const size_t el = cplx ? 16 : 8;
    const bool ls = what == SUB_WHAT_LS, want_sums = detrend == SP_DETREND_SEGMEAN;
    if (g.subPart.ensure(el * (size_t)p.spp * (size_t)p.tiles * (size_t)m)) return -1;
    if (ls && g.subMat.ensure(16 * (size_t)p.spp * (size_t)m * (size_t)m)) return -1;
    CovArgs K{};
    ArArgs &A = K.A;
    A.x = x_d, A.cplx = cplx, A.x_ld = x_ld, A.first = first, A.hop = hop, A.nframes = nframes, A.n = n;
    A.detrend = detrend == SP_DETREND_SEGMEAN ? 1 : ((mean_re != 0.0 || mean_im != 0.0) ? 2 : 0);
    A.mre = mean_re, A.mim = mean_im;
    K.m = m, K.fb = fb;
    ArSmall sm;                                                     // carved by the look, before it sets its first pass
    auto pass = [&](int64_t s0) {
        A.seg0 = s0, A.nseg = std::min<int64_t>(p.spp, segs - s0);
        A.p = 1, A.out_ld = 2, A.a = sm.flag, A.e = sm.mean, A.k = sm.flag;   // what k_ar_scan's launch asks for and neither kernel here touches
        K.C = ls ? (char *)g.subMat.p : C_d + 16 * (size_t)(s0 * C_ld);
        K.C_ld = ls ? (int64_t)m * m : C_ld;
    };
    if (int rc = ar_look(who, A, pass, segs, p, true, want_sums, &sm)) return rc;
    double *mean = sm.mean;
    for (int64_t s0 = 0; s0 < segs; s0 += p.spp, ++g_passes[8]) {
        pass(s0);
        if (ar_pass_means(who, A, p, want_sums, sm)) return -1;
        int rc;
        {
            ProfScope ps;
            rc = launch_cov_row(lc(), K, p.chunk, p.tiles, mean, g.subPart.p);
        }
        if (rc != 0) return fail("%s: row 0 was refused (%lld segments of %lld in %lld tiles, m %d)", who, (long long)A.nseg, (long long)n, (long long)p.tiles, m);
        HIPCHK(hipGetLastError());
        if (launch_cov_fill(lc(), K, p.tiles, mean, g.subPart.p) != 0) return fail("%s: the fill of the matrices was refused", who);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_cov_row";
        if (ls) {
            if (launch_ls_chol(lc(), K.C, K.C_ld, m, A.nseg, cplx, a_d + el * (size_t)(s0 * out_ld), e_d + s0, st_d + s0, out_ld) != 0)
                return fail("%s: the Cholesky solve was refused", who);
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

int sp_covmat(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
              int m, int fb, int detrend, double mean_re, double mean_im, void *C, int64_t C_ld, int mem) {
    const char *who = "sp_covmat";
    if (sub_refusals(who, SUB_WHAT_COVMAT, x, dtype, x_ld, nsig, batch, n, hop, first, nframes, m, fb, detrend, mean_re, mean_im)) return -1;
    if (C_ld < (int64_t)m * m) return fail("%s: C_ld = %lld is below m m = %d", who, (long long)C_ld, m * m);
    if (!C) return fail("%s: C is required", who);
    const int64_t segs = batch * nframes;
    if (segs == 0) return 0;
    if (segs > ((int64_t)1 << 40) / C_ld) return fail("%s: %lld matrices %lld apart are more than 2^40 elements", who, (long long)segs, (long long)C_ld);
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64;
    Stage st(mem);
    const char *x_d;
    char *C_d;
    st.in(g.in0, (const char *)x, (cplx ? 8 : 4) * (size_t)((batch - 1) * x_ld + nsig), &x_d);
    st.rows(g.out0, (char *)C, 16, segs, C_ld, (int64_t)m * m, &C_d);
    if (st.commit()) return -1;
    if (int rc = sub_passes(who, SUB_WHAT_COVMAT, x_d, cplx, x_ld, segs, n, hop, first, nframes, m, fb, detrend, mean_re, mean_im, C_d, C_ld, nullptr, nullptr,
                            nullptr, 0))
        return rc;
    return st.finish();
}

int sp_ar_ls(const void *x, int dtype, int64_t x_ld, int64_t nsig, int64_t batch, int64_t n, int64_t hop, int64_t first, int64_t nframes,
             int order, int fb, int detrend, double mean_re, double mean_im, void *a, double *e, int32_t *status, int64_t out_ld, int mem) {
    const char *who = "sp_ar_ls";
    if (order < 1 || order > SUB_MAX_M - 1) return fail("%s: order must lie in 1 .. 63 (order %d)", who, order);
    const int m = order + 1;
    if (sub_refusals(who, SUB_WHAT_LS, x, dtype, x_ld, nsig, batch, n, hop, first, nframes, m, fb, detrend, mean_re, mean_im)) return -1;
    if (out_ld < order + 1) return fail("%s: out_ld = %lld is below order + 1 = %d", who, (long long)out_ld, order + 1);
    if (!a) return fail("%s: a is required", who);
    if (!e) return fail("%s: e is required", who);
    if (!status) return fail("%s: status is required", who);
    const int64_t segs = batch * nframes;
    if (segs == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const bool cplx = dtype == SP_DTYPE_C64;
    const size_t el = cplx ? 16 : 8;
    Stage st(mem);
    const char *x_d;
    char *a_d;
    double *e_d;
    int32_t *s_d;
    st.in(g.in0, (const char *)x, (cplx ? 8 : 4) * (size_t)((batch - 1) * x_ld + nsig), &x_d);
    st.rows(g.out0, (char *)a, el, segs, out_ld, order + 1, &a_d);
    st.out(g.out0, e, 8 * (size_t)segs, &e_d);
    st.out(g.out0, status, 4 * (size_t)segs, &s_d);
    if (st.commit()) return -1;
    if (int rc = sub_passes(who, SUB_WHAT_LS, x_d, cplx, x_ld, segs, n, hop, first, nframes, m, fb, detrend, mean_re, mean_im, nullptr, 0, a_d, e_d, s_d, out_ld))
        return rc;
    return st.finish();
}

int sp_pseudospectrum(const void *V, int64_t V_ld, const double *w, int m, int p, int64_t nmodels, int weighting, int64_t nbins, double start,
                      double step, int out64, void *P, int64_t P_ld, int32_t *status, int mem) {
    const char *who = "sp_pseudospectrum";
    if (m < 2 || m > SUB_MAX_M) return fail("%s: m = %d must lie in 2 .. 64", who, m);
    if (p < 0 || p > m - 1) return fail("%s: p = %d must lie in 0 .. m - 1 = %d", who, p, m - 1);
    if (V_ld < m) return fail("%s: V_ld = %lld is below m = %d", who, (long long)V_ld, m);
    if (weighting != SP_SUB_MUSIC && weighting != SP_SUB_EV) return fail("%s: weighting = %d must be SP_SUB_MUSIC or SP_SUB_EV", who, weighting);
    if (nbins < 1 || nbins > 0x7fffffff) return fail("%s: nbins = %lld must lie in 1 .. 2^31 - 1", who, (long long)nbins);
    if (P_ld < nbins) return fail("%s: P_ld = %lld is below nbins = %lld", who, (long long)P_ld, (long long)nbins);
    if (nmodels < 0 || (nmodels > 0 && (nbins + 255) / 256 > 0x7fffffff / nmodels))
        return fail("%s: nmodels = %lld must not be negative, nor nmodels x ceil(nbins / 256) exceed 2^31 - 1", who, (long long)nmodels);
    if (!std::isfinite(start) || !std::isfinite(step)) return fail("%s: start and step must be finite", who);
    if (!V) return fail("%s: V is required", who);
    if (!w) return fail("%s: w is required", who);
    if (!P) return fail("%s: P is required", who);
    if (!status) return fail("%s: status is required", who);
    if (nmodels == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t pel = out64 ? 8 : 4;
    Stage st(mem);
    const char *V_d;
    const double *w_d;
    char *P_d;
    int32_t *s_d;
    st.in(g.in0, (const char *)V, 16 * (size_t)((nmodels * m - 1) * V_ld + m), &V_d);
    st.in(g.in0, w, 8 * (size_t)(nmodels * m), &w_d);
    st.rows(g.out0, (char *)P, pel, nmodels, P_ld, nbins, &P_d);
    st.out(g.out0, status, 4 * (size_t)nmodels, &s_d);
    if (st.commit()) return -1;
    int rc;
    {
        ProfScope ps;
        rc = launch_pseudo(lc(), V_d, V_ld, w_d, m, p, nmodels, weighting == SP_SUB_EV, nbins, start, step, out64 != 0, P_d, P_ld, s_d);
    }
    if (rc != 0) return fail("%s: the launch was refused (%lld models, %lld bins)", who, (long long)nmodels, (long long)nbins);
    HIPCHK(hipGetLastError());
    g.last_kernel = "k_pseudo";
    return st.finish();
}

// ---- the array scan: Bartlett, Capon, MUSIC and eigenvector spectra over steering vectors (k_beam.hip; include/spectral_array.h; beam_plan.h) ----
int sp_beamscan_plan(int m, int ndim, int64_t nk, int64_t nmodels, int method, int p, int64_t out[8]) {
    if (!out || beam_shape(m, ndim, nk, nmodels, method, p)) return -1;
    const BeamPlan b = beam_plan_of(m, nk, nmodels, method, p, env_int("SP_BEAM_GRID", 0));
    out[0] = b.tq;
    out[1] = b.tiles;
    out[2] = b.ks;
    out[3] = b.lds_bytes;
    out[4] = b.grid;
    out[5] = b.per_wg;
    out[6] = b.stages;
    out[7] = 0;
    return 0;
}

int sp_beamscan(const void *V, int64_t V_ld, const double *w, int m, int64_t nmodels, const double *pos, int ndim, const double *kv, int64_t nk,
                const double *scale, int method, int p, double loading, int out64, void *P, int64_t P_ld, int32_t *status, int mem) {
    const char *who = "sp_beamscan";
    if (const char *why = beam_shape(m, ndim, nk, nmodels, method, p))
        return fail("%s: %s (m %d, ndim %d, nk %lld, nmodels %lld, method %d, p %d)", who, why, m, ndim, (long long)nk, (long long)nmodels, method, p);
    if (V_ld < m) return fail("%s: V_ld = %lld is below m = %d", who, (long long)V_ld, m);
    if (P_ld < nk) return fail("%s: P_ld = %lld is below nk = %lld", who, (long long)P_ld, (long long)nk);
    if (!(loading >= 0.0) || !std::isfinite(loading)) return fail("%s: loading must be finite and not negative", who);
    if (!V) return fail("%s: V is required", who);
    if (!w) return fail("%s: w is required", who);
    if (!pos) return fail("%s: pos is required", who);
    if (!kv) return fail("%s: kv is required", who);
    if (!P) return fail("%s: P is required", who);
    if (!status) return fail("%s: status is required", who);
    if (!beam_finite(pos, (int64_t)m * ndim)) return fail("%s: pos must be finite", who);
    if (!beam_finite(kv, nk * ndim)) return fail("%s: kv must be finite", who);
    if (scale && !beam_finite(scale, nmodels)) return fail("%s: scale must be finite", who);
    if (nmodels == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const BeamPlan b = beam_plan_of(m, nk, nmodels, method, p, env_int("SP_BEAM_GRID", 0));
    void *pos_d = nullptr, *kv_d = nullptr, *sc_d = nullptr;
    if (get_table(29, pos, sizeof(double) * (size_t)m * ndim, &pos_d, nullptr)) return -1;
    if (get_table(30, kv, sizeof(double) * (size_t)nk * ndim, &kv_d, nullptr)) return -1;
    if (scale && get_table(31, scale, sizeof(double) * (size_t)nmodels, &sc_d, nullptr)) return -1;
    const size_t pel = out64 ? 8 : 4;
    Stage st(mem);
    const char *V_d;
    const double *w_d;
    char *P_d;
    int32_t *s_d;
    st.in(g.in0, (const char *)V, 16 * (size_t)((nmodels * m - 1) * V_ld + m), &V_d);
    st.in(g.in0, w, 8 * (size_t)(nmodels * m), &w_d);
    st.rows(g.out0, (char *)P, pel, nmodels, P_ld, nk, &P_d);
    st.out(g.out0, status, 4 * (size_t)nmodels, &s_d);
    if (st.commit()) return -1;
    int rc;
    {
        ProfScope ps;
        rc = launch_beam(lc(), V_d, V_ld, w_d, m, nmodels, (const double *)pos_d, ndim, (const double *)kv_d, nk, (const double *)sc_d, method, p, loading,
                         out64 != 0, P_d, P_ld, s_d, b.grid);
    }
    if (rc != 0) return fail("%s: the launch was refused (%lld models, %lld scan points, %lld bytes of LDS)", who, (long long)nmodels, (long long)nk, (long long)b.lds_bytes);
    HIPCHK(hipGetLastError());
    g.last_kernel = "k_beam";
    return st.finish();
}

// ---- conditioned spectral analysis: MIMO responses, multiple and partial coherence (k_cond.hip; include/spectral_mimo.h; cond_plan.h) ----
int sp_cond_plan(int n, int q, int64_t count, unsigned want, int64_t out[8]) {
    if (!out || cond_shape(n, q, count, want)) return -1;
    const CondPlan p = cond_plan_of(n, count, want, env_int("SP_COND_GRID", 0));
    const bool wantP = (want & COND_WANT_P) != 0;
    out[0] = p.pitch;
    out[1] = p.wg;
    out[2] = p.lds_bytes;
    out[3] = p.raised;
    out[4] = p.grid;
    out[5] = p.per_wg;
    out[6] = wantP ? cond_off_w(n) : 0;
    out[7] = cond_off_diag(n, wantP);
    return 0;
}

int sp_cond(const void *G, int64_t G_ld, int n, int64_t count, const int32_t *order, int q, unsigned want, double loading, void *H, int64_t H_ld,
            void *Gc, int64_t Gc_ld, double *mcoh, int64_t mcoh_ld, double *piv, int64_t piv_ld, void *P, int64_t P_ld, int32_t *status, int mem) {
    const char *who = "sp_cond";
    if (const char *why = cond_shape(n, q, count, want))
        return fail("%s: %s (n %d, q %d, count %lld, want %u)", who, why, n, q, (long long)count, want);
    const int64_t r = n - q, nn = (int64_t)n * n;
    const bool wH = (want & COND_WANT_H) && r * q > 0, wG = (want & COND_WANT_GC) && r > 0, wM = (want & COND_WANT_MCOH) && r > 0;
    const bool wV = (want & COND_WANT_PIV) != 0, wP = (want & COND_WANT_P) != 0;
    if (G_ld < nn) return fail("%s: G_ld = %lld is below n^2 = %lld", who, (long long)G_ld, (long long)nn);
    if (wH && H_ld < r * q) return fail("%s: H_ld = %lld is below r q = %lld", who, (long long)H_ld, (long long)(r * q));
    if (wG && Gc_ld < r * r) return fail("%s: Gc_ld = %lld is below r^2 = %lld", who, (long long)Gc_ld, (long long)(r * r));
    if (wM && mcoh_ld < r) return fail("%s: mcoh_ld = %lld is below r = %lld", who, (long long)mcoh_ld, (long long)r);
    if (wV && piv_ld < n) return fail("%s: piv_ld = %lld is below n = %d", who, (long long)piv_ld, n);
    if (wP && P_ld < nn) return fail("%s: P_ld = %lld is below n^2 = %lld", who, (long long)P_ld, (long long)nn);
    if (!(loading >= 0.0) || !std::isfinite(loading)) return fail("%s: loading must be finite and not negative", who);
    if (order && !cond_is_perm(order, n)) return fail("%s: order is not a permutation of 0 .. n - 1", who);
    if (count == 0) return 0;
    if (!G) return fail("%s: G is required", who);
    if (!status) return fail("%s: status is required", who);
    if (wH && !H) return fail("%s: H is wanted and NULL", who);
    if (wG && !Gc) return fail("%s: Gc is wanted and NULL", who);
    if (wM && !mcoh) return fail("%s: mcoh is wanted and NULL", who);
    if (wV && !piv) return fail("%s: piv is wanted and NULL", who);
    if (wP && !P) return fail("%s: P is wanted and NULL", who);
    if (ensure_init()) return -1;
    ApiLock lk;
    const CondPlan pl = cond_plan_of(n, count, want, env_int("SP_COND_GRID", 0));
    CondArgs a{};
    a.G_ld = G_ld, a.count = count, a.n = n, a.q = q, a.loading = loading;
    a.want = (wH ? COND_WANT_H : 0u) | (wG ? COND_WANT_GC : 0u) | (wM ? COND_WANT_MCOH : 0u) | (wV ? COND_WANT_PIV : 0u) | (wP ? COND_WANT_P : 0u);
    a.H_ld = H_ld, a.Gc_ld = Gc_ld, a.mcoh_ld = mcoh_ld, a.piv_ld = piv_ld, a.P_ld = P_ld;
    for (int i = 0; i < COND_MAX_N; ++i) a.order.p[i] = (unsigned char)(i < n ? (order ? order[i] : i) : 0);
    Stage st(mem);
    const char *G_d;
    char *H_d = nullptr, *Gc_d = nullptr, *P_d = nullptr;
    double *m_d = nullptr, *v_d = nullptr;
    int32_t *s_d;
    st.in(g.in0, (const char *)G, 16 * (size_t)((count - 1) * G_ld + nn), &G_d);
    if (wH) st.rows(g.out0, (char *)H, 16, count, H_ld, r * q, &H_d);
    if (wG) st.rows(g.out0, (char *)Gc, 16, count, Gc_ld, r * r, &Gc_d);
    if (wM) st.rows(g.out0, mcoh, 8, count, mcoh_ld, r, &m_d);
    if (wV) st.rows(g.out0, piv, 8, count, piv_ld, n, &v_d);
    if (wP) st.rows(g.out0, (char *)P, 16, count, P_ld, nn, &P_d);
    st.out(g.out0, status, 4 * (size_t)count, &s_d);
    if (st.commit()) return -1;
    a.G = (const double2 *)G_d;
    a.H = (double2 *)H_d, a.Gc = (double2 *)Gc_d, a.P = (double2 *)P_d, a.mcoh = m_d, a.piv = v_d, a.status = s_d;
    int rc;
    {
        ProfScope ps;
        rc = launch_cond(lc(), a, pl);
    }
    if (rc != 0) return fail("%s: the launch was refused (n %d, %lld matrices, %lld bytes of LDS)", who, n, (long long)count, (long long)pl.lds_bytes);
    HIPCHK(hipGetLastError());
    g.last_kernel = "k_cond";
    return st.finish();
}

// ---- the discrete wavelet transforms (k_dwt.hip; include/spectral_dwt.h; dwt_plan.h) ----------------------------------------------
// what every entry refuses about its shape and filters, in one order, and what it then works with; 0 or -1
struct DwtCall {
    DwtFilt f;
    DwtPlan p;
    bool cplx;
    size_t el;
};
static int dwt_enter(const char *who, int what, int dtype, int64_t n, int64_t batch, const double *lo, const double *hi, int L, int mode, int levels, int form,
                     DwtCall *c) {
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return fail("%s: dtype = %d must be SP_DTYPE_F32 or SP_DTYPE_C64", who, dtype);
    if (const char *why = dwt_shape(what, n, L, mode, levels, batch))
        return fail("%s: %s (n %lld, L %d, mode %d, levels %d, batch %lld)", who, why, (long long)n, L, mode, levels, (long long)batch);
    if (!lo || !hi) return fail("%s: both filters are required", who);
    const double scale = what >= DWT_WHAT_MODWT ? 0.70710678118654752440 : 1.0;
    c->f.L = L;
    for (int i = 0; i < DWT_MAX_L; ++i) c->f.lo[i] = c->f.hi[i] = 0.f;
    for (int i = 0; i < L; ++i) {
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i])) return fail("%s: the filters must be finite (tap %d)", who, i);
        c->f.lo[i] = (float)(lo[i] * scale), c->f.hi[i] = (float)(hi[i] * scale);
    }
    if (form != SP_DWT_AUTO && form != SP_DWT_ROW && form != SP_DWT_TILE) return fail("%s: form = %d must be 0 (auto), 1 (row) or 2 (tile)", who, form);
    c->cplx = dtype == SP_DTYPE_C64, c->el = c->cplx ? 8 : 4;
    c->p = dwt_plan_of(what, c->cplx, n, L, mode, levels, batch, form, env_int("SP_DWT_ROWS", 0));
    if (form == SP_DWT_ROW && !c->p.row_fits)
        return fail("%s: the row form does not fit: two buffers of a row of %lld samples take %lld bytes of LDS, a workgroup has %lld", who, (long long)n,
                    (long long)dwt_row_lds(c->cplx, n, L), (long long)DWT_LDS_MAX);
    return 0;
}

int sp_dwt_plan(int what, int dtype, int64_t n, int L, int mode, int levels, int64_t batch, int form, int64_t out[80]) {
    if (!out || (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) || dwt_shape(what, n, L, mode, levels, batch)) return -1;
    if (form != SP_DWT_AUTO && form != SP_DWT_ROW && form != SP_DWT_TILE) return -1;
    const DwtPlan p = dwt_plan_of(what, dtype == SP_DTYPE_C64, n, L, mode, levels, batch, form, env_int("SP_DWT_ROWS", 0));
    if (form == SP_DWT_ROW && !p.row_fits) return -1;
    const int64_t head[10] = {p.form, p.tile, p.lds_bytes, p.workgroups, p.launches, p.passes, p.scratch_bytes, p.rpp, p.max_levels, p.rpw};
    for (int i = 0; i < 10; ++i) out[i] = head[i];
    for (int e = 0; e < p.nent; ++e) out[10 + 2 * e] = p.len[e], out[11 + 2 * e] = p.off[e];
    return 0;
}

static DwtRowArgs dwt_row_args(const DwtCall &c, int64_t n, int64_t rows, int mode, int levels) {
    DwtRowArgs a{};
    a.cplx = c.cplx, a.n = n, a.rows = rows, a.f = c.f, a.mode = mode, a.levels = levels, a.rpw = c.p.rpw, a.cap = c.p.cap;
    a.lds = (size_t)dwt_row_lds(c.cplx, n, c.f.L), a.lv = c.p.lv;
    return a;
}

// the two scratch buffers of a pass of the tile form: the approximation of level j in S[j & 1], its rows buf[j & 1] apart
static int dwt_scratch(const DwtCall &c, char *S[2]) {
    const size_t b0 = (c.el * (size_t)c.p.rpp * (size_t)c.p.buf[0] + 255) & ~(size_t)255;
    if (g.dwtS.ensure(b0 + c.el * (size_t)c.p.rpp * (size_t)c.p.buf[1] + 256)) return -1;
    S[0] = (char *)g.dwtS.p, S[1] = S[0] + b0;
    return 0;
}

// analysis over device pointers: the details of row b at outD + b d_ld + lv.off[j], the last approximation at outA + b a_ld
static int dwt_run(const char *who, const DwtCall &c, int mode, int levels, const char *x, int64_t x_ld, int64_t n, int64_t batch, char *outA, int64_t a_ld,
                   char *outD, int64_t d_ld) {
    const size_t el = c.el;
    if (c.p.form == DWT_FORM_ROW) {
        int rc;
        {
            ProfScope ps;
            rc = launch_dwt_row(lc(), dwt_row_args(c, n, batch, mode, levels), x, x_ld, outA, a_ld, outD, d_ld);
        }
        if (rc != 0) return fail("%s: the row form's launch was refused (n %lld, L %d, levels %d)", who, (long long)n, c.f.L, levels);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_dwt_row";
        return 0;
    }
    char *S[2];
    if (dwt_scratch(c, S)) return -1;
    for (int64_t r0 = 0; r0 < batch; r0 += c.p.rpp, ++g_passes[9]) {
        DwtTileArgs a{c.cplx, std::min<int64_t>(c.p.rpp, batch - r0), c.f, mode};
        const char *src = x + el * (size_t)(r0 * x_ld);
        int64_t sld = x_ld, nj = n;
        for (int j = 1; j <= levels; ++j) {
            char *dA = j == levels ? outA + el * (size_t)(r0 * a_ld) : S[j & 1];
            const int64_t dld = j == levels ? a_ld : c.p.buf[j & 1];
            int rc;
            {
                ProfScope ps;
                rc = launch_dwt_tile(lc(), a, src, sld, nj, dA, dld, outD + el * (size_t)(r0 * d_ld + c.p.lv.off[j]), d_ld);
            }
            if (rc != 0) return fail("%s: the tile form's launch of level %d was refused (%lld samples)", who, j, (long long)nj);
            HIPCHK(hipGetLastError());
            src = dA, sld = dld, nj = c.p.lv.len[j];
        }
    }
    g.last_kernel = "k_dwt_tile";
    return 0;
}

static int idwt_run(const char *who, const DwtCall &c, int mode, int levels, const char *inA, int64_t a_ld, const char *inD, int64_t d_ld, int64_t n, int64_t batch,
                    char *x, int64_t x_ld) {
    const size_t el = c.el;
    if (c.p.form == DWT_FORM_ROW) {
        int rc;
        {
            ProfScope ps;
            rc = launch_idwt_row(lc(), dwt_row_args(c, n, batch, mode, levels), inA, a_ld, inD, d_ld, x, x_ld);
        }
        if (rc != 0) return fail("%s: the row form's launch was refused (n %lld, L %d, levels %d)", who, (long long)n, c.f.L, levels);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_idwt_row";
        return 0;
    }
    char *S[2];
    if (dwt_scratch(c, S)) return -1;
    for (int64_t r0 = 0; r0 < batch; r0 += c.p.rpp, ++g_passes[9]) {
        DwtTileArgs a{c.cplx, std::min<int64_t>(c.p.rpp, batch - r0), c.f, mode};
        const char *src = inA + el * (size_t)(r0 * a_ld);
        int64_t sld = a_ld;
        for (int j = levels; j >= 1; --j) {
            char *dst = j == 1 ? x + el * (size_t)(r0 * x_ld) : S[(j - 1) & 1];
            const int64_t dld = j == 1 ? x_ld : c.p.buf[(j - 1) & 1];
            int rc;
            {
                ProfScope ps;
                rc = launch_idwt_tile(lc(), a, src, sld, inD + el * (size_t)(r0 * d_ld + c.p.lv.off[j]), d_ld, dst, dld, c.p.lv.len[j - 1]);
            }
            if (rc != 0) return fail("%s: the tile form's launch of level %d was refused", who, j);
            HIPCHK(hipGetLastError());
            src = dst, sld = dld;
        }
    }
    g.last_kernel = "k_idwt_tile";
    return 0;
}

// what the entries refuse about their buffers; `need` elements of a row of each
static int dwt_buffers(const char *who, const void *in, int64_t in_ld, int64_t in_need, const char *in_name, const void *out, int64_t out_ld, int64_t out_need,
                       const char *out_name) {
    if (in_ld < in_need) return fail("%s: %s_ld = %lld is below the %lld elements of a row", who, in_name, (long long)in_ld, (long long)in_need);
    if (out_ld < out_need) return fail("%s: %s_ld = %lld is below the %lld elements of a row", who, out_name, (long long)out_ld, (long long)out_need);
    if (in_ld > ((int64_t)1 << 40) || out_ld > ((int64_t)1 << 40)) return fail("%s: a pitch beyond 2^40 elements", who);
    if (!in) return fail("%s: %s is required", who, in_name);
    if (!out) return fail("%s: %s is required", who, out_name);
    return 0;
}

int sp_dwt(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *dec_lo, const double *dec_hi, int L, int mode, int levels,
           void *out, int64_t out_ld, int form, int mem) {
    const char *who = "sp_dwt";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_DWT, dtype, n, batch, dec_lo, dec_hi, L, mode, levels, form, &c)) return -1;
    if (dwt_buffers(who, x, x_ld, n, "x", out, out_ld, c.p.total, "out")) return -1;
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    Stage st(mem);
    const char *x_d;
    char *o_d;
    st.in(g.in0, (const char *)x, c.el * (size_t)((batch - 1) * x_ld + n), &x_d);
    st.rows(g.out0, (char *)out, c.el, batch, out_ld, c.p.total, &o_d);
    if (st.commit()) return -1;
    if (int rc = dwt_run(who, c, mode, levels, x_d, x_ld, n, batch, o_d, out_ld, o_d, out_ld)) return rc;
    return st.finish();
}

int sp_dwt_level(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *dec_lo, const double *dec_hi, int L, int mode,
                 void *cA, int64_t a_ld, void *cD, int64_t d_ld, int form, int mem) {
    const char *who = "sp_dwt_level";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_DWT, dtype, n, batch, dec_lo, dec_hi, L, mode, 1, form, &c)) return -1;
    const int64_t K = c.p.lv.len[1];
    if (dwt_buffers(who, x, x_ld, n, "x", cA, a_ld, K, "cA") || dwt_buffers(who, x, x_ld, n, "x", cD, d_ld, K, "cD")) return -1;
    if (batch == 0) return 0;
    const size_t a_bytes = c.el * (size_t)((batch - 1) * a_ld + K), d_bytes = c.el * (size_t)((batch - 1) * d_ld + K);
    if (!mem && (const char *)cA < (const char *)cD + d_bytes && (const char *)cD < (const char *)cA + a_bytes)
        return fail("%s: with mem = 0 the rows of cA and cD must not overlap", who);
    if (ensure_init()) return -1;
    ApiLock lk;
    Stage st(mem);
    const char *x_d;
    char *a_d, *d_d;
    st.in(g.in0, (const char *)x, c.el * (size_t)((batch - 1) * x_ld + n), &x_d);
    st.rows(g.out0, (char *)cA, c.el, batch, a_ld, K, &a_d);
    st.rows(g.out0, (char *)cD, c.el, batch, d_ld, K, &d_d);
    if (st.commit()) return -1;
    c.p.lv.off[1] = 0;
    if (int rc = dwt_run(who, c, mode, 1, x_d, x_ld, n, batch, a_d, a_ld, d_d, d_ld)) return rc;
    return st.finish();
}

int sp_idwt(const void *coef, int dtype, int64_t c_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int mode, int levels,
            void *x, int64_t x_ld, int form, int mem) {
    const char *who = "sp_idwt";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_IDWT, dtype, n, batch, rec_lo, rec_hi, L, mode, levels, form, &c)) return -1;
    if (dwt_buffers(who, coef, c_ld, c.p.total, "coef", x, x_ld, n, "x")) return -1;
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    Stage st(mem);
    const char *c_d;
    char *x_d;
    st.in(g.in0, (const char *)coef, c.el * (size_t)((batch - 1) * c_ld + c.p.total), &c_d);
    st.rows(g.out0, (char *)x, c.el, batch, x_ld, n, &x_d);
    if (st.commit()) return -1;
    if (int rc = idwt_run(who, c, mode, levels, c_d, c_ld, c_d, c_ld, n, batch, x_d, x_ld)) return rc;
    return st.finish();
}

int sp_idwt_level(const void *cA, int64_t a_ld, const void *cD, int64_t d_ld, int dtype, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi,
                  int L, int mode, void *x, int64_t x_ld, int form, int mem) {
    const char *who = "sp_idwt_level";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_IDWT, dtype, n, batch, rec_lo, rec_hi, L, mode, 1, form, &c)) return -1;
    const int64_t K = c.p.lv.len[1];
    if (dwt_buffers(who, cA, a_ld, K, "cA", x, x_ld, n, "x") || dwt_buffers(who, cD, d_ld, K, "cD", x, x_ld, n, "x")) return -1;
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    Stage st(mem);
    const char *a_d, *d_d;
    char *x_d;
    st.in(g.in0, (const char *)cA, c.el * (size_t)((batch - 1) * a_ld + K), &a_d);
    st.in(g.in0, (const char *)cD, c.el * (size_t)((batch - 1) * d_ld + K), &d_d);
    st.rows(g.out0, (char *)x, c.el, batch, x_ld, n, &x_d);
    if (st.commit()) return -1;
    c.p.lv.off[1] = 0;
    if (int rc = idwt_run(who, c, mode, 1, a_d, a_ld, d_d, d_ld, n, batch, x_d, x_ld)) return rc;
    return st.finish();
}

int sp_modwt(const void *x, int dtype, int64_t x_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int levels, void *W,
             int64_t w_ld, int form, int mem) {
    const char *who = "sp_modwt";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_MODWT, dtype, n, batch, rec_lo, rec_hi, L, 0, levels, form, &c)) return -1;
    if (dwt_buffers(who, x, x_ld, n, "x", W, w_ld, n, "W")) return -1;
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const int64_t plane = batch * w_ld;
    Stage st(mem);
    const char *x_d;
    char *w_d;
    st.in(g.in0, (const char *)x, c.el * (size_t)((batch - 1) * x_ld + n), &x_d);
    st.rows(g.out0, (char *)W, c.el, (int64_t)(levels + 1) * batch, w_ld, n, &w_d);
    if (st.commit()) return -1;
    if (c.p.form == DWT_FORM_ROW) {
        int rc;
        {
            ProfScope ps;
            rc = launch_modwt_row(lc(), dwt_row_args(c, n, batch, 0, levels), x_d, x_ld, w_d, w_ld, plane);
        }
        if (rc != 0) return fail("%s: the row form's launch was refused (n %lld, L %d, levels %d)", who, (long long)n, L, levels);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_modwt_row";
        return st.finish();
    }
    char *S[2];
    if (dwt_scratch(c, S)) return -1;
    for (int64_t r0 = 0; r0 < batch; r0 += c.p.rpp, ++g_passes[9]) {
        DwtTileArgs a{c.cplx, std::min<int64_t>(c.p.rpp, batch - r0), c.f, 0};
        const char *src = x_d + c.el * (size_t)(r0 * x_ld);
        int64_t sld = x_ld;
        for (int j = 1; j <= levels; ++j) {
            char *wj = w_d + c.el * (size_t)((j - 1) * plane + r0 * w_ld);
            char *dst = j == levels ? w_d + c.el * (size_t)(levels * plane + r0 * w_ld) : S[j & 1];
            const int64_t dld = j == levels ? w_ld : c.p.buf[j & 1];
            int rc;
            {
                ProfScope ps;
                rc = launch_modwt_tile(lc(), a, j, src, sld, n, wj, w_ld, dst, dld);
            }
            if (rc != 0) return fail("%s: the tile form's launch of level %d was refused", who, j);
            HIPCHK(hipGetLastError());
            src = dst, sld = dld;
        }
    }
    g.last_kernel = "k_modwt_tile";
    return st.finish();
}

int sp_imodwt(const void *W, int dtype, int64_t w_ld, int64_t n, int64_t batch, const double *rec_lo, const double *rec_hi, int L, int levels, void *x,
              int64_t x_ld, int form, int mem) {
    const char *who = "sp_imodwt";
    DwtCall c;
    if (dwt_enter(who, DWT_WHAT_IMODWT, dtype, n, batch, rec_lo, rec_hi, L, 0, levels, form, &c)) return -1;
    if (dwt_buffers(who, W, w_ld, n, "W", x, x_ld, n, "x")) return -1;
    if (batch == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    const int64_t plane = batch * w_ld;
    Stage st(mem);
    const char *w_d;
    char *x_d;
    st.in(g.in0, (const char *)W, c.el * (size_t)(((int64_t)(levels + 1) * batch - 1) * w_ld + n), &w_d);
    st.rows(g.out0, (char *)x, c.el, batch, x_ld, n, &x_d);
    if (st.commit()) return -1;
    if (c.p.form == DWT_FORM_ROW) {
        int rc;
        {
            ProfScope ps;
            rc = launch_imodwt_row(lc(), dwt_row_args(c, n, batch, 0, levels), w_d, w_ld, plane, x_d, x_ld);
        }
        if (rc != 0) return fail("%s: the row form's launch was refused (n %lld, L %d, levels %d)", who, (long long)n, L, levels);
        HIPCHK(hipGetLastError());
        g.last_kernel = "k_imodwt_row";
        return st.finish();
    }
    char *S[2];
    if (dwt_scratch(c, S)) return -1;
    for (int64_t r0 = 0; r0 < batch; r0 += c.p.rpp, ++g_passes[9]) {
        DwtTileArgs a{c.cplx, std::min<int64_t>(c.p.rpp, batch - r0), c.f, 0};
        const char *src = w_d + c.el * (size_t)(levels * plane + r0 * w_ld);
        int64_t sld = w_ld;
        for (int j = levels; j >= 1; --j) {
            char *dst = j == 1 ? x_d + c.el * (size_t)(r0 * x_ld) : S[(j - 1) & 1];
            const int64_t dld = j == 1 ? x_ld : c.p.buf[(j - 1) & 1];
            int rc;
            {
                ProfScope ps;
                rc = launch_imodwt_tile(lc(), a, j, w_d + c.el * (size_t)((j - 1) * plane + r0 * w_ld), w_ld, src, sld, n, dst, dld);
            }
            if (rc != 0) return fail("%s: the tile form's launch of level %d was refused", who, j);
            HIPCHK(hipGetLastError());
            src = dst, sld = dld;
        }
    }
    g.last_kernel = "k_imodwt_tile";
    return st.finish();
}

// ---- wavelet bispectrum and bicoherence (k_wbic.hip; include/spectral_wbic.h) ------------------------------------
#define WBIC_MAX_M 3072
#define WBIC_W_BYTES ((size_t)128 << 20)            // the transforms of a pass
#define WBIC_PART_BYTES ((size_t)128 << 20)         // the fp32 partials of a pass
#define WBIC_OUT_BYTES ((size_t)1 << 30)            // B and b2
#define WBIC_ACC_BYTES ((size_t)2 << 30)            // the float64 cell sums

struct WbicPlan {
    int ntd, ntiles;
    int64_t ncells, cell_len, cpb, chunk, span_max, pass_groups_max;
    std::vector<WbicGroup> groups;
    std::vector<int> gfirst;            // [ncells + 1]: the first group of every cell, then the number of groups
    std::vector<int64_t> pass;          // [passes + 1]: the first group of every pass, then the number of groups
    std::vector<int> tbl;               // [tmap | the tile list as int2]
    size_t nmap, w_bytes, part_bytes, acc_bytes;
};

// the checks sp_wbic and sp_wbic_plan share; 0 or the message's tail
static const char *wbic_shape(int64_t nsig, int S, int k_lo, int L, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks,
                              int nrec, bool sym) {
    if (S < 2 || S > WBIC_MAX_S) return "nscales must lie in 2 .. 512";
    if (k_lo < 1) return "k_lo must be at least 1";
    if (k_lo > S - 1) return "k_lo is above nscales - 1: no pair is valid";
    if (M > WBIC_MAX_M) return "M is above 3072: a scale does not fuse, and there is no composed path here";
    if (const char *why = cwt_shape(nsig, S, 1, L, M)) return why;
    if (nrec < 1 || nrec > 3) return "1 .. 3 distinct records";
    if (block < 1 || step < 1) return "block and step must be at least 1";
    if (step < block && block % step != 0) return "either step >= block or block % step == 0";
    if (nblocks < 1) return "nblocks must be at least 1";
    if ((size_t)nblocks > WBIC_OUT_BYTES / ((size_t)S * (size_t)S * 24)) return "nblocks S^2 24 bytes are above 1 GiB";
    if (n0 < 0 || n0 >= nsig || block > nsig || (double)n0 + (double)(nblocks - 1) * (double)step + (double)block > (double)nsig ||
        n0 + (nblocks - 1) * step + block > nsig)
        return "a block lies outside the record";
    const int64_t cpb = step < block ? block / step : 1, ncells = nblocks - 1 + cpb;
    const int ntd = (S + WBIC_TILE - 1) / WBIC_TILE;
    const size_t tiles_most = (size_t)(sym ? ntd * (ntd + 1) / 2 : ntd * ntd);
    if ((size_t)ncells > WBIC_ACC_BYTES / (tiles_most * sizeof(double) * WBIC_PART)) return "the float64 cell sums are above 2 GiB";
    const int64_t cell_len = step < block ? step : block;
    if ((double)ncells * (double)((cell_len + WBIC_GROUP - 1) / WBIC_GROUP) > (double)(1 << 30)) return "more than 2^30 groups";
    return nullptr;
}

// cells, groups, passes and tiles of an accepted shape
static WbicPlan wbic_plan_of(int64_t nsig, int S, int k_lo, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks, int nrec,
                             bool sym) {
    WbicPlan p;
    p.cpb = step < block ? block / step : 1;
    p.ncells = nblocks - 1 + p.cpb;
    p.cell_len = step < block ? step : block;
    // the tiles that hold a valid pair (tj <= ti in the auto form) and the map (ti, tj) -> tile number (-1: none)
    p.ntd = (S + WBIC_TILE - 1) / WBIC_TILE;
    p.tbl.assign((size_t)p.ntd * p.ntd, -1);
    std::vector<int> tl;
    for (int ti = 0; ti < p.ntd; ++ti)
        for (int tj = 0; tj < (sym ? ti + 1 : p.ntd); ++tj) {
            if (ti * WBIC_TILE + tj * WBIC_TILE + k_lo > S - 1) continue;
            p.tbl[(size_t)ti * p.ntd + tj] = (int)tl.size() / 2;
            tl.push_back(ti);
            tl.push_back(tj);
        }
    p.ntiles = (int)tl.size() / 2;
    p.nmap = p.tbl.size() + (p.tbl.size() & 1);          // the int2 list starts 8-byte aligned
    p.tbl.resize(p.nmap, -1);
    p.tbl.insert(p.tbl.end(), tl.begin(), tl.end());
    // groups: every cell in runs of WBIC_GROUP samples, the last one ragged
    p.gfirst.reserve((size_t)p.ncells + 1);
    for (int64_t c = 0; c < p.ncells; ++c) {
        p.gfirst.push_back((int)p.groups.size());
        const int64_t s0 = n0 + c * step;
        for (int64_t o = 0; o < p.cell_len; o += WBIC_GROUP)
            p.groups.push_back(WbicGroup{s0 + o, (int)c, (int)std::min<int64_t>(WBIC_GROUP, p.cell_len - o)});
    }
    p.gfirst.push_back((int)p.groups.size());
    // passes: runs of whole groups that span at most `chunk` samples, hold at most pass_groups_max groups, and at least one
    p.chunk = std::max<int64_t>(1, (int64_t)(WBIC_W_BYTES / (sizeof(cf) * (size_t)S * (size_t)nrec)));
    p.chunk = hook_cap("SP_WBIC_CHUNK", p.chunk);
    const size_t group_part = sizeof(float) * WBIC_PART * (size_t)std::max(p.ntiles, 1);
    const int64_t gcap = std::max<int64_t>(1, std::min<int64_t>(WBIC_MAX_PASS_GROUPS, (int64_t)(WBIC_PART_BYTES / group_part)));
    const int64_t ng = (int64_t)p.groups.size();
    p.span_max = p.pass_groups_max = 0;
    for (int64_t gA = 0; gA < ng;) {
        int64_t gB = gA + 1;
        while (gB < ng && gB - gA < gcap && p.groups[(size_t)gB].start + p.groups[(size_t)gB].len - p.groups[(size_t)gA].start <= p.chunk) ++gB;
        p.pass.push_back(gA);
        const int64_t a = p.groups[(size_t)gA].start, b = p.groups[(size_t)gB - 1].start + p.groups[(size_t)gB - 1].len;
        p.span_max = std::max(p.span_max, std::min(b + M, nsig) - std::max<int64_t>(a - M, 0));
        p.pass_groups_max = std::max(p.pass_groups_max, gB - gA);
        gA = gB;
    }
    p.pass.push_back(ng);
    p.w_bytes = sizeof(cf) * (size_t)nrec * (size_t)S * (size_t)p.span_max;
    p.part_bytes = (size_t)p.pass_groups_max * (group_part + sizeof(double) * (size_t)S);
    p.acc_bytes = (size_t)p.ncells * sizeof(double) * (WBIC_PART * (size_t)std::max(p.ntiles, 1) + (size_t)S);
    return p;
}

int sp_wbic_plan(int64_t nsig, int nscales, int k_lo, int L, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks, int nrec,
                 int sym, int64_t out[8]) {
    if (!out || wbic_shape(nsig, nscales, k_lo, L, M, n0, block, step, nblocks, nrec, sym != 0)) return -1;
    const WbicPlan p = wbic_plan_of(nsig, nscales, k_lo, M, n0, block, step, nblocks, nrec, sym != 0);
    out[0] = p.ncells;
    out[1] = p.cell_len;
    out[2] = (int64_t)p.groups.size();
    out[3] = (int64_t)p.pass.size() - 1;
    out[4] = (int64_t)p.groups.size() * p.ntiles;
    out[5] = (int64_t)(p.w_bytes + p.part_bytes + p.acc_bytes);
    out[6] = p.chunk;
    out[7] = p.ntiles;
    return 0;
}

int sp_wbic(const void *x, const void *y, const void *z, int x_dtype, int y_dtype, int z_dtype, int64_t nsig, const double *scales,
            int nscales, int k_lo, int family, double p0, int L, int M, int64_t n0, int64_t block, int64_t step, int64_t nblocks, void *B,
            double *b2, double *P, int *passes, int mem) {
    // every refusal comes before the device is touched
    if (!x || !scales || !B || !b2 || !P) return fail("sp_wbic: x, scales, B, b2 and P are required");
    if (x_dtype != SP_DTYPE_F32 && x_dtype != SP_DTYPE_C64) return fail("sp_wbic: dtype must be float32 or complex64, got %d", x_dtype);
    if ((y && y_dtype != x_dtype) || (z && z_dtype != x_dtype))
        return fail("sp_wbic: the records differ in dtype (x %d, y %d, z %d)", x_dtype, y_dtype, z_dtype);
    // the records that are transformed: x, then y and z where they are other pointers
    const void *src[3] = {x, y ? y : x, z ? z : x};
    int rec[3] = {0, 0, 0}, nrec = 1;
    if (src[1] != src[0]) rec[1] = nrec++;
    if (src[2] != src[0]) rec[2] = src[2] == src[1] ? rec[1] : nrec++;
    const bool sym = rec[1] == 0;
    if (const char *why = wbic_shape(nsig, nscales, k_lo, L, M, n0, block, step, nblocks, nrec, sym))
        return fail("sp_wbic: %s (nscales %d, k_lo %d, L %d, M %d, nsig %lld, n0 %lld, block %lld, step %lld, nblocks %lld)", why, nscales,
                    k_lo, L, M, (long long)nsig, (long long)n0, (long long)block, (long long)step, (long long)nblocks);
    if (family != SP_CWT_MORLET && family != SP_CWT_PAUL) return fail("sp_wbic: family %d is neither SP_CWT_MORLET nor SP_CWT_PAUL", family);
    if (!isfinite(p0) || !(p0 > 0.0) || p0 > 64.0 || (family == SP_CWT_PAUL && p0 < 1.0))
        return fail("sp_wbic: parameter p0 = %g must lie in (0, 64] (Morlet's w0) or [1, 64] (Paul's m)", p0);
    for (int s = 0; s < nscales; ++s)
        if (!isfinite(scales[s]) || !(scales[s] > 0.0) || scales[s] > 1e9)
            return fail("sp_wbic: scales[%d] = %g must be positive and finite", s, scales[s]);
    if (ensure_init()) return -1;
    ApiLock lk;
    const WbicPlan p = wbic_plan_of(nsig, nscales, k_lo, M, n0, block, step, nblocks, nrec, sym);
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4, S = (size_t)nscales;
    // the scales' filter constants, as sp_cwt forms them
    const double lognorm = family == SP_CWT_MORLET ? -0.25 * log(M_PI) : p0 * log(2.0) - 0.5 * (log(p0) + lgamma(2.0 * p0));
    std::vector<float> sc(2 * S);
    for (size_t s = 0; s < S; ++s) {
        sc[2 * s] = (float)(2.0 * M_PI * scales[s] / (double)L);
        sc[2 * s + 1] = (float)(lognorm + 0.5 * log(2.0 * M_PI * scales[s]) - log((double)L));
    }
    // the call's small tables: [tmap | tiles] and [gfirst | groups]
    const size_t nfirst = p.gfirst.size() + (p.gfirst.size() & 1);      // the groups start 8-byte aligned
    std::vector<char> gt(sizeof(int) * nfirst + sizeof(WbicGroup) * p.groups.size(), 0);
    memcpy(gt.data(), p.gfirst.data(), sizeof(int) * p.gfirst.size());
    memcpy(gt.data() + sizeof(int) * nfirst, p.groups.data(), sizeof(WbicGroup) * p.groups.size());
    void *sc_d = nullptr, *tab_d = nullptr, *gt_d = nullptr;
    if (get_table(15, sc.data(), sizeof(float) * sc.size(), &sc_d, nullptr)) return -1;
    if (get_table(26, p.tbl.data(), sizeof(int) * p.tbl.size(), &tab_d, nullptr)) return -1;
    if (get_table(27, gt.data(), gt.size(), &gt_d, nullptr)) return -1;
    const int *tmap_d = (const int *)tab_d;
    const int2 *tiles_d = (const int2 *)((const int *)tab_d + p.nmap);
    const int *gfirst_d = (const int *)gt_d;
    const WbicGroup *groups_d = (const WbicGroup *)((const char *)gt_d + sizeof(int) * nfirst);
    const cf *tw;
    if (get_twiddles(L, &tw)) return -1;
    Stage st(mem);
    const void *xd[3] = {nullptr, nullptr, nullptr};
    void *Bd;
    double *b2d, *Pd;
    for (int k = 0; k < 3; ++k)
        if (k == 0 || rec[k] > rec[k - 1]) st.in(g.bsIn, src[k], esz * (size_t)nsig, &xd[rec[k]]);
    const size_t nn = (size_t)nblocks * S * S;
    st.out(g.out0, B, 2 * sizeof(double) * nn, &Bd);
    st.out(g.out0, b2, sizeof(double) * nn, &b2d);
    st.out(g.out0, P, sizeof(double) * (size_t)nblocks * S, &Pd);
    if (st.commit()) return -1;
    if (g.wbW.ensure(p.w_bytes) || g.wbP.ensure(p.part_bytes) || g.wbA.ensure(p.acc_bytes)) return -1;
    float *part = (float *)g.wbP.p;
    double *ppart = (double *)(part + (size_t)p.pass_groups_max * WBIC_PART * (size_t)p.ntiles);
    double *acc = (double *)g.wbA.p, *pcell = acc + (size_t)p.ncells * WBIC_PART * (size_t)p.ntiles;
    HIPCHK(hipMemsetAsync(g.wbA.p, 0, p.acc_bytes, g.stream));
    CwtArgs a{};
    a.cplx = cplx ? 1 : 0;
    a.sc = (const float *)sc_d;
    a.p = family == SP_CWT_PAUL ? (float)p0 : 0.f;
    a.a = family == SP_CWT_MORLET ? 0.5f : 0.f;
    a.b = family == SP_CWT_PAUL ? 1.f : 0.f;
    a.u0 = family == SP_CWT_MORLET ? (float)p0 : 0.f;
    a.S = nscales;
    a.M = M;
    const int npass = (int)p.pass.size() - 1;
    for (int q = 0; q < npass; ++q) {
        const int64_t gA = p.pass[(size_t)q], gB = p.pass[(size_t)q + 1];
        const WbicGroup &first = p.groups[(size_t)gA], &last = p.groups[(size_t)gB - 1];
        const int64_t sub0 = std::max<int64_t>(first.start - M, 0), sub1 = std::min<int64_t>(last.start + last.len + M, nsig);
        const int64_t nsub = sub1 - sub0;
        // the transforms of the samples [sub0, sub1) of every distinct record, [S][nsub] each: k_cwt on the sub-record
        const CwtPlan pl = cwt_plan_of(L, M, nsub, nscales, 1, false, false, g.ncu, env_int("SP_CWT_CHUNK", 0));
        cf *W[3];
        for (int k = 0; k < nrec; ++k) {
            W[k] = (cf *)g.wbW.p + (size_t)k * S * (size_t)nsub;
            a.x = (const char *)xd[k] + esz * (size_t)sub0;
            a.nsig = a.x_ld = nsub;
            a.nframes = pl.frames;
            a.chunk = pl.chunk;
            a.hop = pl.hop;
            a.W = W[k];
            if (launch_cwt(lc(), a, L, tw, pl, 1) != 0)
                return fail("sp_wbic: the transform's launch was refused (L %d, M %d, nscales %d, %lld samples)", L, M, nscales, (long long)nsub);
            HIPCHK(hipGetLastError());
        }
        {
            ProfScope ps;
            LAUNCHCHK(launch_wbic_tile(lc(), W[rec[0]], W[rec[1]], W[rec[2]], nscales, k_lo, nsub, sub0, groups_d + gA, (int)(gB - gA), tiles_d,
                                       p.ntiles, part));
            g.last_kernel = "k_wbic_tile";
        }
        LAUNCHCHK(launch_wbic_pz(lc(), W[rec[2]], nscales, nsub, sub0, groups_d + gA, (int)(gB - gA), ppart));
        LAUNCHCHK(launch_wbic_cells(lc(), part, ppart, gfirst_d, first.cell, (int64_t)last.cell - first.cell + 1, gA, gB, p.ntiles, nscales, acc,
                                    pcell));
    }
    LAUNCHCHK(launch_wbic_finish(lc(), acc, pcell, tmap_d, p.ntd, p.ntiles, nscales, k_lo, sym ? 1 : 0, nblocks, p.cpb, block, Bd, b2d, Pd));
    if (passes) *passes = npass;
    return st.finish();
}

// ---- FFT accumulation method (k_fam.hip; include/spectral_fam.h) -------------------------------------------------
#define FAM_PASS_BYTES ((size_t)256 << 20)          // the bin-major frames of a pass
#define FAM_ACC_BYTES ((size_t)2 << 30)             // the float64 sums of a call of several passes

struct FamPlan {
    int64_t twoQ, bpp, passes, workgroups;
    size_t z_bytes, acc_bytes;
};

// the checks sp_fam and sp_fam_plan share; 0 or the message's tail
static const char *fam_shape(int dtype, int np, int64_t hop, int P, int64_t nblocks, int64_t npairs) {
    if (dtype != SP_DTYPE_F32 && dtype != SP_DTYPE_C64) return "dtype must be float32 or complex64";
    if (np < 32 || np > SP_MAX_WG_FFT || !is_pow2(np)) return "np must be a power of two from 32 to 8192";
    if (P < 32 || P > SP_FAM_MAX_P || !is_pow2(P)) return "P must be a power of two from 32 to 8192";
    if (hop < 1 || hop > np || !is_pow2(hop)) return "hop must be a power of two from 1 to np";
    if ((int64_t)P * hop < 2 * (int64_t)np) return "P hop is below 2 np: no bin lies within half a channel spacing";
    if (nblocks < 0) return "nblocks must not be negative";
    if (npairs < 1 || npairs > SP_FAM_MAX_PAIRS) return "npairs must lie in 1 .. 2^22";
    return nullptr;
}

// blocks per pass and passes of an accepted shape
static FamPlan fam_plan_of(int nrec, int np, int64_t hop, int P, int64_t nblocks, int64_t npairs) {
    FamPlan p;
    p.twoQ = (int64_t)P * hop / np;
    const size_t block_bytes = sizeof(cf) * (size_t)nrec * (size_t)np * (size_t)P;
    p.bpp = std::max<int64_t>(1, (int64_t)(FAM_PASS_BYTES / block_bytes));
    p.bpp = std::min(hook_cap("SP_FAM_BLOCKS", p.bpp), nblocks);
    p.passes = nblocks > 0 ? (nblocks + p.bpp - 1) / p.bpp : 0;
    p.workgroups = p.passes * ((npairs + fpw_of(P) - 1) / fpw_of(P));
    p.z_bytes = block_bytes * (size_t)p.bpp;
    p.acc_bytes = p.passes > 1 ? 2 * sizeof(double) * (size_t)npairs * (size_t)p.twoQ : 0;
    return p;
}

int sp_fam_plan(int dtype, int cross, int np, int64_t hop, int P, int64_t nblocks, int64_t npairs, int64_t out[5]) {
    if (!out || fam_shape(dtype, np, hop, P, nblocks, npairs)) return -1;
    const FamPlan p = fam_plan_of(cross ? 2 : 1, np, hop, P, nblocks, npairs);
    if (p.acc_bytes > FAM_ACC_BYTES) return -1;
    out[0] = p.twoQ / 2;
    out[1] = p.bpp;
    out[2] = p.passes;
    out[3] = p.workgroups;
    out[4] = (int64_t)p.z_bytes;
    return 0;
}

int sp_fam(const void *x, const void *y, int dtype, int64_t nsig, const float *a, int np, int64_t hop, const float *taper, int P,
           int64_t nblocks, const int32_t *pairs, int64_t npairs, int conj, const double *mean_x, const double *mean_y, double scale,
           void *S, void *Pwx, void *Pwy, int mem) {
    // every refusal comes before the device is touched
    if (const char *why = fam_shape(dtype, np, hop, P, nblocks, npairs))
        return fail("sp_fam: %s (dtype %d, np %d, hop %lld, P %d, nblocks %lld, npairs %lld)", why, dtype, np, (long long)hop, P,
                    (long long)nblocks, (long long)npairs);
    if (nblocks > 0 && (nsig < np || nblocks > ((nsig - np) / hop + 1) / P))
        return fail("sp_fam: nblocks = %lld blocks of P = %d frames of np = %d at hop %lld reach outside the nsig = %lld samples of the row",
                    (long long)nblocks, P, np, (long long)hop, (long long)nsig);
    if (!isfinite(scale)) return fail("sp_fam: scale must be finite");
    for (int c = 0; c < 2; ++c)
        if ((mean_x && !isfinite(mean_x[c])) || (mean_y && !isfinite(mean_y[c]))) return fail("sp_fam: mean_x and mean_y must be finite");
    if (!x) return fail("sp_fam: x is required");
    if (!a) return fail("sp_fam: a is required");
    if (!taper) return fail("sp_fam: g is required");
    if (!pairs) return fail("sp_fam: pairs is required");
    if (!S && !Pwx && !Pwy) return fail("sp_fam: no output: one of S, Pwx and Pwy is required");
    for (int64_t i = 0; i < 2 * npairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= np)
            return fail("sp_fam: pairs[%lld][%d] = %d lies outside the channels 0 .. %d", (long long)(i / 2), (int)(i & 1), pairs[i], np - 1);
    const bool cross = y != nullptr, cplx = dtype == SP_DTYPE_C64;
    const int nrec = cross ? 2 : 1;
    const FamPlan p = fam_plan_of(nrec, np, hop, P, nblocks, npairs);
    if (p.acc_bytes > FAM_ACC_BYTES)
        return fail("sp_fam: npairs = %lld pairs of %lld bins in %lld passes need float64 sums above 2 GiB", (long long)npairs, (long long)p.twoQ,
                    (long long)p.passes);
    if (nblocks == 0) return 0;
    if (ensure_init()) return -1;
    ApiLock lk;
    Xf xf;
    if (get_xf(np, &xf)) return -1;
    const cf *twP;
    if (get_twiddles(P, &twP)) return -1;
    const size_t esz = cplx ? sizeof(cf) : sizeof(float);
    const int64_t nframes = nblocks * P;
    const size_t used = (size_t)((nframes - 1) * hop + np);           // the samples the frames reach
    Stage st(mem);
    const void *xd[2] = {nullptr, nullptr};
    cf *S_d;
    float *Pw_d[2];
    st.in(g.in0, x, esz * used, &xd[0]);
    st.in(g.in1, y, esz * used, &xd[1]);
    st.out(g.out0, S, sizeof(cf) * (size_t)npairs * (size_t)p.twoQ, &S_d);
    st.out(g.out0, Pwx, sizeof(float) * (size_t)np, &Pw_d[0]);
    st.out(g.out0, Pwy, sizeof(float) * (size_t)np, &Pw_d[1]);
    if (st.commit()) return -1;
    // small tables: both windows, the pair table, the means as trend records (x, then y)
    void *a_d = nullptr, *g_d = nullptr, *pairs_d = nullptr;
    if (get_table(1, a, sizeof(float) * (size_t)np, &a_d, nullptr)) return -1;
    if (get_table(1, taper, sizeof(float) * (size_t)P, &g_d, nullptr)) return -1;
    if (get_table(28, pairs, sizeof(int32_t) * 2 * (size_t)npairs, &pairs_d, nullptr)) return -1;
    TrendBuf tb;
    if (get_trendbuf(2, &tb)) return -1;
    if (set_trend(tb, 0, xd[0], cplx, nsig, 0, mean_x ? mean_x[0] : 0.0, mean_x && cplx ? mean_x[1] : 0.0)) return -1;
    if (cross && set_trend(tb, 1, xd[1], cplx, nsig, 0, mean_y ? mean_y[0] : 0.0, mean_y && cplx ? mean_y[1] : 0.0)) return -1;
    // scratch: the bin-major frames of a pass (x, then y), the frame-major frames of one record before their transposition, the
    // float64 sums (S across passes; the channel powers of x and y)
    const int64_t ld = p.bpp * P;
    const size_t rec_elems = (size_t)np * (size_t)ld;
    if (g.famZ.ensure(sizeof(cf) * rec_elems * (size_t)nrec) || g.work.ensure(sizeof(cf) * rec_elems)) return -1;
    if (g.famA.ensure(p.acc_bytes + 2 * sizeof(double) * (size_t)np)) return -1;
    double *pw_acc = (double *)g.famA.p, *s_acc = pw_acc + 2 * (size_t)np;
    cf *Z[2] = {(cf *)g.famZ.p, (cf *)g.famZ.p + rec_elems};
    const bool pair = !cplx && !env_flag("SP_NO_REALPAIR");
    FamArgs fa{};
    fa.g = (const float *)g_d;
    fa.pairs = (const int2 *)pairs_d;
    fa.acc = p.passes > 1 ? s_acc : nullptr;
    fa.S = S_d;
    fa.npairs = npairs;
    fa.scale = scale;
    fa.twoQ = (int)p.twoQ;
    fa.conj = conj ? 1 : 0;
    for (int64_t b0 = 0; b0 < nblocks; b0 += p.bpp, ++g_passes[5]) {
        const int64_t nb = std::min(p.bpp, nblocks - b0), m = nb * P;
        const bool first = b0 == 0, last = b0 + nb == nblocks;
        for (int r = 0; r < nrec; ++r) {
            const void *xr = (const char *)xd[r] + esz * (size_t)(b0 * P * hop);
            if (pair) {
                const RunPart rp = run_partition(xf.L, m / 2, g.ncu);
                LAUNCHCHK(launch_stft_rp(lc(), (const float *)xr, (const float *)a_d, (int)hop, m, tb.f + 4 * r, false, xf, rp, SIDED_RAW, 1.f,
                                         0, g.work.p, nullptr));
            } else {
                const RunPart rp = run_partition(xf.L, m, g.ncu);
                LAUNCHCHK(launch_stft(lc(), xr, cplx, (const float *)a_d, (int)hop, m, tb.f + 4 * r, false, xf, rp, SIDED_RAW, 1.f, 0,
                                      g.work.p, nullptr));
            }
            // [m][np] -> [np][m]: the rows of a short last pass keep the pitch of their own frame count
            LAUNCHCHK(launch_transpose(lc(), g.work.p, Z[r], m, (int64_t)np, (int)sizeof(cf)));
            if (Pw_d[r]) LAUNCHCHK(launch_fam_pw(lc(), Z[r], np, m, m, P, (const float *)g_d, pw_acc + (size_t)r * np, first, last, scale, Pw_d[r]));
        }
        // y = x: Pwy is Pwx, copied where both are asked for
        if (!cross && Pw_d[1] && !Pw_d[0])
            LAUNCHCHK(launch_fam_pw(lc(), Z[0], np, m, m, P, (const float *)g_d, pw_acc + (size_t)np, first, last, scale, Pw_d[1]));
        if (!cross && Pw_d[1] && Pw_d[0] && last)
            HIPCHK(hipMemcpyAsync(Pw_d[1], Pw_d[0], sizeof(float) * (size_t)np, hipMemcpyDeviceToDevice, g.stream));
        if (S_d) {
            fa.Y = Z[cross ? 1 : 0];
            fa.X = Z[0];
            fa.ld = m;
            fa.nb = nb;
            fa.first = first ? 1 : 0;
            fa.last = last ? 1 : 0;
            ProfScope ps;
            if (launch_fam(lc(), fa, P, twP) != 0)
                return fail("sp_fam: the launch was refused (P %d, %lld pairs, %lld blocks)", P, (long long)npairs, (long long)nb);
            HIPCHK(hipGetLastError());
            g.last_kernel = "k_fam";
        }
    }
    return st.finish();
}

// ---- batched Hermitian eigensolver (k_eigh.hip) --------------------------------------------------
int sp_eigh_plan(int n, int nvec, int64_t batch, int64_t out[4]) {
    if (n < 1 || n > SP_EIGH_MAX_N || nvec < 0 || nvec > n || batch < 0 || !out) return -1;
    const EighPlan p = eigh_plan_of(n, nvec > 0, batch, g.ncu, env_int("SP_EIGH_GRID", 0));
    out[0] = p.NP;
    out[1] = (int64_t)p.lds_bytes;
    out[2] = p.wg_per_cu;
    out[3] = p.grid;
    return 0;
}

int sp_eigh(const double *a, int n, int64_t batch, int nvec, int max_sweeps, double *w, double *v, int32_t *sweeps, int mem) {
    // every refusal comes before the device is touched
    if (n < 1 || n > SP_EIGH_MAX_N) return fail("sp_eigh: n = %d outside 1 .. %d", n, SP_EIGH_MAX_N);
    if (nvec < 0 || nvec > n) return fail("sp_eigh: nvec = %d outside 0 .. n = %d", nvec, n);
    if (batch < 0) return fail("sp_eigh: batch = %lld must not be negative", (long long)batch);
    if (max_sweeps < 1 || max_sweeps > INT_MAX - 1) return fail("sp_eigh: max_sweeps = %d must be at least 1", max_sweeps);
    if (batch == 0) return 0;
    if (!a || !w || !sweeps) return fail("sp_eigh: a, w and sweeps are required");
    if (nvec > 0 && !v) return fail("sp_eigh: v is required for nvec = %d > 0", nvec);
    if (ensure_init()) return -1;
    ApiLock lk;
    const size_t abytes = sizeof(double) * 2 * (size_t)batch * n * n, wbytes = sizeof(double) * (size_t)batch * n;
    const size_t vbytes = sizeof(double) * 2 * (size_t)batch * n * nvec, sbytes = sizeof(int32_t) * (size_t)batch;
    Stage st(mem);
    const double *ad;
    double *wd, *vd;
    int32_t *sd;
    st.in(g.in0, a, abytes, &ad);
    st.out(g.out0, nvec > 0 ? v : nullptr, vbytes, &vd);
    st.out(g.out0, w, wbytes, &wd);
    st.out(g.out0, sweeps, sbytes, &sd);
    if (st.commit()) return -1;
    const EighPlan pl = eigh_plan_of(n, nvec > 0, batch, g.ncu, env_int("SP_EIGH_GRID", 0));
    {
        ProfScope ps;
        LAUNCHCHK(launch_eigh(lc(), ad, n, batch, nvec, max_sweeps, wd, vd, sd, pl));
        g.last_kernel = "k_eigh";
    }
    return st.finish();
}

// reciprocal window-square envelope of sp_istft as [period: hop][head: head_len][tail: n - hop] float32 from float64 sums; entries
// whose envelope is <= 1e-10 are 1 (scipy's rule: such samples are not divided).  Away from the ends env[a] = P[a mod hop]; the first
// n - hop samples lack the frames before 0 and the last n - hop those from M on.  With so few frames that the two ends meet
// (M hop < n - hop) the head piece covers the whole output instead and there is no tail.
static int64_t istft_head_len(int n, int hop, int64_t M) {
    return M * (int64_t)hop >= (int64_t)(n - hop) ? (int64_t)(n - hop) : (M - 1) * (int64_t)hop + n;
}
static void istft_envelope(const float *win, int n, int hop, int64_t M, std::vector<float> *out) {
    const int64_t H = istft_head_len(n, hop, M);
    const bool whole = H != (int64_t)(n - hop);
    std::vector<double> per((size_t)hop, 0.0), head((size_t)H, 0.0), tail(whole ? 0 : (size_t)(n - hop), 0.0);
    for (int j = 0; j < n; ++j) per[(size_t)(j % hop)] += (double)win[j] * (double)win[j];
    if (whole) {
        for (int64_t g = 0; g < M; ++g)
            for (int j = 0; j < n; ++j) head[(size_t)(g * hop + j)] += (double)win[j] * (double)win[j];
    } else {
        for (int a = 0; a < n - hop; ++a) head[(size_t)a] = (double)win[a] * (double)win[a] + (a >= hop ? head[(size_t)(a - hop)] : 0.0);
        for (int i = n - hop - 1; i >= 0; --i)
            tail[(size_t)i] = (double)win[i + hop] * (double)win[i + hop] + (i + hop < n - hop ? tail[(size_t)(i + hop)] : 0.0);
    }
    out->clear();
    out->reserve(per.size() + head.size() + tail.size());
    for (const std::vector<double> *v : {&per, &head, &tail})
        for (double e : *v) out->push_back(e > 1e-10 ? (float)(1.0 / e) : 1.f);
}

int sp_istft(const void *Z, int sided, int in_major, int nch, int64_t nframes, const float *win, int nfft, int hop, double scale,
             int64_t skip, int64_t nout, void *y, int mem) {
    if (!Z || !win || !y) return fail("sp_istft: Z, win and y are required");
    if (sided != SP_SIDED_HALF && sided != SP_SIDED_RAW) return fail("sp_istft: sided must be SP_SIDED_HALF or SP_SIDED_RAW");
    if (in_major != 0 && in_major != 1) return fail("sp_istft: in_major must be 0 or 1");
    if (nfft < 2 || hop < 1 || hop > nfft) return fail("sp_istft: need nfft >= 2 and 1 <= hop <= nfft (nfft %d, hop %d)", nfft, hop);
    if (nframes < 1 || nch < 1) return fail("sp_istft: nframes and nch must be at least 1");
    if (nch > 65535) return fail("sp_istft: nch = %d is beyond the limit of 65535 channels per call", nch);
    if (!wg_capable(nfft))
        return fail("sp_istft: nfft %d not supported (powers of two up to %d, other lengths up to %d)", nfft, SP_MAX_WG_FFT,
                    SP_MAX_WG_FFT / 2);
    if (nframes > ((int64_t)1 << 40) / hop) return fail("sp_istft: too many frames");
    const int64_t M = nframes, Lout = (M - 1) * (int64_t)hop + nfft;
    if (skip < 0 || nout < 1 || skip > Lout || nout > Lout - skip)
        return fail("sp_istft: skip %lld + nout %lld outside the %lld overlap-added samples", (long long)skip, (long long)nout,
                    (long long)Lout);
    if (ensure_init()) return -1;
    ApiLock lk;
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    const bool cplx = sided == SP_SIDED_RAW;
    const int nb = cplx ? nfft : nfft / 2 + 1;
    // real output from a power-of-two transform: two frames per transform
    const int mode = cplx ? 0 : ((!xf.blue && xf.L >= 32 && M >= 2 && !env_flag("SP_NO_REALPAIR")) ? 2 : 1);
    const size_t zbytes = sizeof(cf) * (size_t)nb * (size_t)M * (size_t)nch, ybytes = (cplx ? 8 : 4) * (size_t)nout * (size_t)nch;
    Stage st(mem);
    const cf *zd;
    void *yd;
    st.in(g.in0, Z, zbytes, &zd);
    st.out(g.out0, y, ybytes, &yd);
    if (st.commit()) return -1;
    void *win_d;
    if (get_table(1, win, sizeof(float) * (size_t)nfft, &win_d, nullptr)) return -1;
    // the envelope pieces, cached beside the window by (window, hop, and the frame count where the two ends meet)
    const int64_t head_len = istft_head_len(nfft, hop, M);
    const bool ends_apart = head_len == (int64_t)(nfft - hop);
    const uint64_t ekey[4] = {window_key(win, nfft), (uint64_t)nfft, (uint64_t)hop, ends_apart ? ~(uint64_t)0 : (uint64_t)M};
    const size_t ebytes = sizeof(float) * ((size_t)hop + (size_t)head_len + (ends_apart ? (size_t)(nfft - hop) : 0));
    void *rcp_d;
    bool fresh = false;
    if (get_table_keyed(7, ekey, sizeof ekey, nullptr, ebytes, &rcp_d, &fresh)) return -1;
    if (fresh) {
        std::vector<float> e;
        istft_envelope(win, nfft, hop, M, &e);
        HIPCHK(hipMemcpy(rcp_d, e.data(), ebytes, hipMemcpyHostToDevice));
    }
    // runs: about 4 groups per CU, and long enough that the q - 1 halo frames a run transforms twice stay a few per cent of it
    // (SP_ISTFT_FPG: a test hook like those of launch.h, read on every call; any value >= 1 is valid, also below q)
    const int FR = mode == 2 ? 2 : 1;
    const int q = (nfft + hop - 1) / hop;
    const int halo = (q - 1 + FR - 1) / FR * FR;
    const int fpw = fpw_of(xf.L);
    auto run_len = [&](int64_t m) {
        int64_t f = env_int("SP_ISTFT_FPG", 0);
        if (f < 1) {
            const int64_t target = std::max<int64_t>(1, (int64_t)g.ncu * 4 * fpw / nch);
            f = std::max((m + target - 1) / target, std::min<int64_t>(16 * (int64_t)halo, m));
        }
        f = std::max<int64_t>(f, 1);
        return (f + FR - 1) / FR * FR;
    };
    const float wscale = (float)(scale / (double)nfft);
    if (in_major == 0) {
        LAUNCHCHK(launch_istft(lc(), zd, (int64_t)nb * M, 0, M, 0, M, run_len(M), halo, (const float *)win_d, wscale, hop, xf, mode,
                               (const float *)rcp_d, head_len, skip, nout, yd, nch, 1));
    } else {
        // bin-major spectra: chunks of frames, each with its halo, are transposed into scratch held to SP_ISTFT_MIB MiB (default 256)
        const size_t budget = (size_t)std::max(1, env_int("SP_ISTFT_MIB", 256)) << 20;
        int64_t mc = (int64_t)(budget / (sizeof(cf) * (size_t)nb * (size_t)nch)) - halo;
        mc = std::max<int64_t>(mc, std::max<int64_t>(halo, 2)) / FR * FR;
        mc = std::min(mc, (M + FR - 1) / FR * FR);
        if (g.work.ensure(sizeof(cf) * (size_t)nb * (size_t)nch * (size_t)(mc + halo))) return -1;
        for (int64_t c0 = 0; c0 < M; c0 += mc) {
            const int64_t c1 = std::min(M, c0 + mc), zb = std::max<int64_t>(0, c0 - halo), m = c1 - zb;
            LAUNCHCHK(launch_istft_gather(lc(), zd, M, nb, zb, m, (cf *)g.work.p, nch));
            LAUNCHCHK(launch_istft(lc(), (const cf *)g.work.p, (int64_t)nb * m, zb, M, c0, c1, run_len(c1 - c0), halo,
                                   (const float *)win_d, wscale, hop, xf, mode, (const float *)rcp_d, head_len, skip, nout, yd, nch,
                                   c1 == M));
        }
    }
    return st.finish();
}

int sp_hilbert(const float *x, int64_t n_in, int64_t x_ld, int64_t nfft, int64_t batch, void *out, int mem) {
    if (ensure_init()) return -1;
    if (n_in < 1 || nfft < 2 || batch < 1 || x_ld < n_in) return fail("sp_hilbert: bad sizes");
    ApiLock lk;
    const size_t ibytes = sizeof(float) * (size_t)x_ld * (size_t)batch;
    const size_t obytes = sizeof(cf) * (size_t)nfft * (size_t)batch;
    Stage st(mem);
    const float *xd;
    cf *od;
    st.in(g.in0, x, ibytes, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    const int64_t nuse = n_in < nfft ? n_in : nfft;
    if (wg_capable(nfft)) {
        Xf xf;
        if (get_xf(nfft, &xf)) return -1;
        LAUNCHCHK(launch_hilbert(lc(), xd, nuse, x_ld, batch, xf, od));     // fwd + mask + inverse fused, one workgroup per row
    } else {
        // long rows: pack -> FFT -> mask -> inverse FFT, each a multi-pass transform
        if (g.bigA.ensure(sizeof(cf) * (size_t)nfft)) return -1;
        cf *A = (cf *)g.bigA.p;
        const int64_t Mh = nfft / 2;
        const bool half_len = (nfft & (nfft - 1)) == 0 && big_three_pass(Mh);
        BigTw btN;
        if (half_len && get_bigtw(nfft, &btN)) return -1;
        for (int64_t b = 0; b < batch; ++b) {
            if (half_len && (((uintptr_t)(od + b * nfft)) & 15) == 0) {
                // real input: ONE half-length transform each way (z[n] = x[2n] + i x[2n+1], M = nfft/2 points).  Forward with
                // the pair load fused into its first pass; k_hilbert_mid turns Z into the half-length spectrum of the
                // Hilbert transform y (real-FFT split, analytic mask and inverse merge in one in-place step); the inverse
                // transform's last pass writes a = x + i y.  960 MB of traffic at 2^24 points instead of 1.45 GB, on 64 MB
                // buffers.
                BigFuse fz;
                const float *row = xd + b * x_ld;
                fz.ci = ColsIn{3, row, (((uintptr_t)row) & 7) == 0 ? row : nullptr, nullptr, nuse};      // r2 == r1: aligned pairs
                if (!env_flag("SP_HILBERT_NOFUSEMID")) {
                    // round 3: the middle step inside a row pass that owns mirror row pairs, the inverse as the adjoint passes in
                    // reversed order (k_hilbert_rowsmid, k_fft_cols_inv): 5 launches, 768 MB at 2^24 samples instead of 7 / 960
                    int lg = 0;
                    while (((int64_t)1 << lg) < Mh) ++lg;
                    int la_ = (lg + 2) / 3;
                    if (la_ > 8) la_ = 8;
                    int lb_ = (lg - la_ + 1) / 2;
                    if (lb_ > 8) lb_ = 8;
                    const int lc_ = lg - la_ - lb_;
                    const int64_t Aa = (int64_t)1 << la_, Bb = (int64_t)1 << lb_, Cc = (int64_t)1 << lc_;
                    Xf xa, xb, xc;
                    BigTw btM;
                    if (get_xf(Aa, &xa) || get_xf(Bb, &xb) || get_xf(Cc, &xc) || get_bigtw(Mh, &btM)) return -1;
                    const cf *tw2c = nullptr;                     // exp(-2 pi i m / (2 C)): the row pass's share of W_N^k
                    if (get_twiddles(2 * Cc, &tw2c)) return -1;
                    if (Aa >= 64 && Bb >= 64 && Cc >= 32 && Cc <= 2048) {
                        // (a full, 8-byte aligned row IS the complex sequence z: the plain first pass at three workgroups per CU
                        //  instead of the predicated pair load at two -- 58 -> 38 us at 2^24 samples)
                        if (nuse == nfft && fz.ci.r2 != nullptr && !env_flag("SP_HILBERT_PAIRLOAD")) {
                            LAUNCHCHK(launch_fft_cols(lc(), reinterpret_cast<const cf *>(row), A, Bb * Cc, 1, Bb * Cc, 0, 1, 0, xa, btM));
                        } else {
                            LAUNCHCHK(launch_fft_cols(lc(), A, A, Bb * Cc, 1, Bb * Cc, 0, 1, 0, xa, btM, 0, fz.ci));
                        }
                        LAUNCHCHK(launch_fft_cols(lc(), A, A, Cc, Aa, Cc, Bb * Cc, Aa, 0, xb, btM));
                        LAUNCHCHK(launch_hilbert_rowsmid(lc(), A, Aa, Bb, xc, btN, tw2c));
                        LAUNCHCHK(launch_fft_cols_inv(lc(), A, A, Cc, Aa, Cc, Bb * Cc, Aa, xb, btM, 1.f, nullptr));
                        RowsOut ao;
                        ao.co = reinterpret_cast<float *>(od + b * nfft);
                        ao.n = nuse;
                        ao.Ltot = nfft;
                        ao.mom = nullptr;
                        ao.rx = row;
                        ao.kind = 2;
                        LAUNCHCHK(launch_fft_cols_inv(lc(), A, nullptr, Bb * Cc, 1, Bb * Cc, 0, 1, xa, btM, (float)(1.0 / (double)Mh), &ao));
                        continue;
                    }
                }
                if (dev_fft_big_pow2(A, A, Mh, 0, 0, 1, &fz)) return -1;
                LAUNCHCHK(launch_hilbert_mid(lc(), A, Mh, btN));
                BigFuse fo;
                fo.ro.co = reinterpret_cast<float *>(od + b * nfft);
                fo.ro.n = nuse;
                fo.ro.Ltot = nfft;
                fo.ro.rx = xd + b * x_ld;
                fo.ro.kind = 2;
                if (dev_fft_big_pow2(A, A, Mh, 1, 0, 1, &fo)) return -1;
                continue;
            }
            if (big_three_pass(nfft)) {
                // real -> complex pack fused into the first pass of the forward transform (the zero padding is not loaded),
                // the analytic-signal mask into the first pass of the inverse one
                BigFuse fz;
                fz.ci = ColsIn{1, xd + b * x_ld, nullptr, nullptr, nuse};
                if (dev_fft_big_pow2(A, A, nfft, 0, 0, 1, &fz)) return -1;
                if (dev_fft_big_pow2(A, od + b * nfft, nfft, 1, 1)) return -1;
                continue;
            }
            LAUNCHCHK(launch_pack_real(lc(), xd + b * x_ld, nuse, nullptr, nfft, A));
            if (dev_fft_any(A, A, nfft, 1, 0)) return -1;
            if (big_three_pass(nfft)) {
                // the mask rides on the first pass of the inverse transform
                if (dev_fft_big_pow2(A, od + b * nfft, nfft, 1, 1)) return -1;
            } else {
                LAUNCHCHK(launch_hilbert_mask(lc(), A, nfft));
                if (dev_fft_any(A, od + b * nfft, nfft, 1, 1)) return -1;
            }
        }
    }
    return st.finish();
}

int sp_frame_sum(const void *x, int x_dtype, int64_t nsig, int nch, int64_t x_ld, int nfft, int hop, int64_t nframes,
                 int detrend, double *out, int mem) {
    if (ensure_init()) return -1;
    if (check_frames("sp_frame_sum", nsig, nfft, hop, nframes)) return -1;
    if (nch < 1 || nch > 65535 || x_ld < nsig) return fail("sp_frame_sum: bad nch / x_ld");
    if (detrend < 0 || detrend > 2) return fail("sp_frame_sum: detrend must be 0, 1 or 2");
    ApiLock lk;
    const bool cplx = x_dtype == SP_DTYPE_C64;
    const size_t esz = cplx ? 8 : 4;
    const size_t ibytes = esz * ((size_t)x_ld * (size_t)(nch - 1) + (size_t)nsig);
    const size_t obytes = sizeof(double) * 2 * (size_t)nfft * (size_t)nch;
    Stage st(mem);
    const void *xd;
    double *od;
    st.in(g.in1, x, ibytes, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    TrendBuf tb;
    if (get_trendbuf(nch + 1, &tb)) return -1;
    if (detrend != 0 && nch <= 512) {
        double *scr = moments_scratch();
        if (!scr) return -1;
        LAUNCHCHK(launch_moments(lc(), xd, cplx, nsig, detrend, scr, tb.d + 8, tb.f + 4, nch, x_ld));
    } else {
        for (int c = 0; c < nch; ++c)
            if (set_trend(tb, c + 1, (const char *)xd + esz * (size_t)x_ld * (size_t)c, cplx, nsig, detrend, 0, 0)) return -1;
    }
    const size_t pbytes = obytes * (size_t)frame_sum_slices(g.ncu, nch, nfft, nframes);
    if (g.work.ensure(pbytes)) return -1;
    LAUNCHCHK(launch_frame_sum(lc(), xd, cplx, x_ld, nch, nfft, hop, nframes, tb.f + 4, detrend == 2, od, (double *)g.work.p));
    return st.finish();
}

int sp_spectral_filter(const float *x, int64_t n_in, int64_t x_ld, int64_t nfft, int64_t batch, const void *H, void *out,
                       int mem) {
    if (ensure_init()) return -1;
    if (n_in < 1 || nfft < 2 || batch < 1 || x_ld < n_in || H == nullptr) return fail("sp_spectral_filter: bad sizes");
    ApiLock lk;
    const size_t ibytes = sizeof(float) * (size_t)x_ld * (size_t)batch;
    const size_t obytes = sizeof(cf) * (size_t)nfft * (size_t)batch;
    const size_t hbytes = sizeof(cf) * (size_t)nfft;
    Stage st(mem);
    const float *xd;
    cf *od;
    st.in(g.in0, x, ibytes, &xd);
    st.out(g.out0, out, obytes, &od);
    if (st.commit()) return -1;
    const int64_t nuse = n_in < nfft ? n_in : nfft;
    if (wg_capable(nfft)) {
        Xf xf;
        if (get_xf(nfft, &xf)) return -1;
        void *H_d;
        if (get_table(4, H, hbytes, &H_d, nullptr)) return -1;          // the response table is a host array (like win)
        LAUNCHCHK(launch_hilbert(lc(), xd, nuse, x_ld, batch, xf, od, (const cf *)H_d));   // fwd, x H, inverse: one workgroup per row
    } else {
        if (g.bigA.ensure(sizeof(cf) * (size_t)nfft) || g.bigB.ensure(hbytes)) return -1;
        cf *A = (cf *)g.bigA.p, *Hd = (cf *)g.bigB.p;
        HIPCHK(hipMemcpyAsync(Hd, H, hbytes, hipMemcpyHostToDevice, g.stream));
        for (int64_t b = 0; b < batch; ++b) {
            LAUNCHCHK(launch_pack_real(lc(), xd + b * x_ld, nuse, nullptr, nfft, A));
            if (dev_fft_any(A, A, nfft, 1, 0)) return -1;
            LAUNCHCHK(launch_spec_mul(lc(), A, Hd, nfft));
            if (dev_fft_any(A, od + b * nfft, nfft, 1, 1)) return -1;
        }
        HIPCHK(hipStreamSynchronize(g.stream));        // H was read from the caller's host array
    }
    return st.finish();
}

int sp_xcorr(const float *x1, const float *x2, int64_t n, float *co_out, int mem) {
    if (ensure_init()) return -1;
    if (n < 1) return fail("sp_xcorr: n must be positive");
    const int64_t L = next_pow2(2 * n) < 2 ? 2 : next_pow2(2 * n);
    if (L > ((int64_t)1 << SP_MAX_BIG_LOG2))
        return fail("sp_xcorr: n=%lld needs a %lld-point transform; the limit is 2^%d", (long long)n, (long long)L, SP_MAX_BIG_LOG2);
    ApiLock lk;
    const size_t ibytes = sizeof(float) * (size_t)n, obytes = sizeof(float) * (size_t)(2 * n - 1);
    Stage st(mem);
    const float *a, *b;
    float *od;
    st.in(g.in0, x1, ibytes, &a);
    st.in(g.in1, x2, ibytes, &b);
    st.out(g.out0, co_out, obytes, &od);
    if (st.commit()) return -1;
    TrendBuf tb;
    if (get_trendbuf(3, &tb)) return -1;
    double *scr = moments_scratch();
    if (!scr) return -1;
    // both signals' mean / variance in ONE pair of launches (two "channels" b - a samples apart: any two device rows; each
    // signal's own pass cost 21 + 8 us of the long ccf's 0.9 ms)
    // (and the normalisation record behind them: one finish launch for both signals, no k_xcorr_norm)
    LAUNCHCHK(launch_moments_xc(lc(), a, n, scr, tb.d, tb.d + 16, (int64_t)(b - a)));
    if (L <= SP_MAX_WG_FFT) {
        Xf xf;
        if (get_xf(L, &xf)) return -1;
        LAUNCHCHK(launch_xcorr(lc(), a, b, n, tb.d + 16, xf, od));          // one workgroup, everything in registers/LDS
    } else {
        if (g.bigA.ensure(sizeof(cf) * (size_t)L) || g.bigB.ensure(sizeof(cf) * (size_t)L)) return -1;
        cf *A = (cf *)g.bigA.p, *B = (cf *)g.bigB.p;
        if (big_three_pass(L)) {
            // two of the three elementwise kernels ride on the transforms: the pack in the first pass of the first transform
            // (the zero half is never loaded), lag re-ordering + real part in the last pass of the second
            BigFuse f1, f2;
            f1.ci = ColsIn{1, a, b, tb.d + 16, n};
            if (big_three_pass(L / 2) && !env_flag("SP_XC_NOFUSEMID")) {
                // round 3: the forward transform's row pass, the middle step and the FIRST pass of the half-length transform in one
                // kernel that owns mirror row pairs (k_xc_rowsmid); the half-length transform's two remaining passes are column
                // passes over the half rows it leaves ([ka][kb][ka'], C/2 per row), the last one writing the lags
                int lg = 0;
                while (((int64_t)1 << lg) < L) ++lg;
                int la_ = (lg + 2) / 3;
                if (la_ > 8) la_ = 8;
                int lb_ = (lg - la_ + 1) / 2;
                if (lb_ > 8) lb_ = 8;
                const int lc_ = lg - la_ - lb_;
                const int64_t Aa = (int64_t)1 << la_, Bb = (int64_t)1 << lb_, Cc = (int64_t)1 << lc_, C2 = Cc / 2;
                Xf xa, xb, xc, xc2;
                BigTw btL, btM;
                if (get_xf(Aa, &xa) || get_xf(Bb, &xb) || get_xf(Cc, &xc) || get_xf(C2, &xc2) || get_bigtw(L, &btL) ||
                    get_bigtw(L / 2, &btM))
                    return -1;
                if (Aa >= 64 && Aa <= 256 && Bb >= 64 && Bb <= 256 && Cc >= 64 && Cc <= 2048) {
                    LAUNCHCHK(launch_fft_cols(lc(), A, A, Bb * Cc, 1, Bb * Cc, 0, 1, 0, xa, btL, 0, f1.ci));
                    LAUNCHCHK(launch_fft_cols(lc(), A, A, Cc, Aa, Cc, Bb * Cc, Aa, 0, xb, btL));
                    LAUNCHCHK(launch_xc_rowsmid(lc(), A, Aa, Bb, xc, xc2, btL, btM));
                    // M-point transform, split (A' = C/2 [done], B' = B, C' = A) on the layout [ka][kb][ka']:
                    //   over kb (stride = the row pitch C, columns ka' < C/2, outer ka), twiddle W_M^{A' ka kb''}: by the OUTER index
                    LAUNCHCHK(launch_fft_cols(lc(), A, A, C2, Aa, Cc, Bb * Cc, C2, 0, xb, btM, 0, ColsIn{0, nullptr, nullptr, nullptr, 0}, 1));
                    //   over ka (stride B C): natural index k' = ka' + A' kb'' + A' B' kc''; the lags leave from here
                    RowsOut ro{od, n, L, tb.d + 16};
                    ro.kind = 3;
                    LAUNCHCHK(launch_fft_cols_lag(lc(), A, C2, Bb, Bb * Cc, Cc, xa, ro));
                    return st.finish();
                }
            }
            if (dev_fft_big_pow2(A, B, L, 0, 0, 1, &f1)) return -1;          // B = FFT(z)
            if (big_three_pass(L / 2)) {
                // the correlation is real: its inverse transform runs at half length (k_xc_mid_half forms the M-point spectrum
                // of r[2n] + i r[2n+1]; the last pass writes two lags per element): 3.0 GB of traffic at 2^24 samples
                // instead of 3.8
                BigTw btL;
                if (get_bigtw(L, &btL)) return -1;
                LAUNCHCHK(launch_xc_mid_half(lc(), B, L, btL, A));
                f2.ro = RowsOut{od, n, L, tb.d + 16};
                f2.ro.kind = 3;
                if (dev_fft_big_pow2(A, A, L / 2, 0, 0, 1, &f2)) return -1;
            } else {
                LAUNCHCHK(launch_xc_mid(lc(), B, L, A));                     // conj(A conj(B)) spectrum
                f2.ro = RowsOut{od, n, L, tb.d + 16};
                f2.ro.kind = 1;
                if (dev_fft_big_pow2(A, B, L, 0, 0, 1, &f2)) return -1;      // writes co from its last pass
            }
        } else {
            LAUNCHCHK(launch_xc_pack(lc(), a, b, n, L, tb.d + 16, A));
            if (dev_fft_big_pow2(A, B, L, 0)) return -1;
            LAUNCHCHK(launch_xc_mid(lc(), B, L, A));                         // conj(A conj(B)) spectrum
            if (dev_fft_big_pow2(A, B, L, 0)) return -1;                     // forward of the conjugate = L * real inverse
            LAUNCHCHK(launch_xc_out(lc(), B, n, L, tb.d + 16, od));
        }
    }
    return st.finish();
}

int sp_csd_epilogue(const double *pxx, const double *pyy, const double *pxy, int nch, int nb, int nfft, int onesided, double enbw,
                    double *out, int mem) {
    if (ensure_init()) return -1;
    if (nch < 1 || nch > 20000 || nb < 1 || nfft < 2 || nb > nfft) return fail("sp_csd_epilogue: bad sizes");
    if (onesided && nb != nbins_host(nfft, SP_SIDED_ONE)) return fail("sp_csd_epilogue: one-sided spectra hold %d bins for nfft=%d", nbins_host(nfft, SP_SIDED_ONE), nfft);
    if (!onesided && nb != nfft) return fail("sp_csd_epilogue: two-sided spectra hold nfft bins");
    ApiLock lk;
    const size_t NB = (size_t)nb, NF = (size_t)nfft, C = (size_t)nch;
    const size_t n_out = sp_csd_epilogue_doubles(nch, nb, nfft);
    Stage st(mem);
    const double *dxx, *dyy, *dxy;
    double *od;
    st.in(g.out0, pxx, sizeof(double) * NB, &dxx);
    st.in(g.out0, pyy, sizeof(double) * NB * C, &dyy);
    st.in(g.out0, pxy, sizeof(double) * 2 * NB * C, &dxy);
    st.out(g.out0, out, sizeof(double) * n_out, &od);
    if (st.commit()) return -1;
    // out layout (doubles): cxy[C][NB][2] | cxy2[C][NB] | phi[C][NB] | lxx[NB] | lyy[C][NB] | lxy[C][NB] |
    //                       rxx[NF][2] | ryy[C][NF][2] | rxy[C][NF][2] | icxy[C][NF][2] | corrcoef[C][NF][2] | e[1+C][2]
    double *cxy = od, *cxy2 = cxy + 2 * C * NB, *phi = cxy2 + C * NB, *lxx = phi + C * NB, *lyy = lxx + NB, *lxy = lyy + C * NB;
    double *rxx = lxy + C * NB, *ryy = rxx + 2 * NF, *rxy = ryy + 2 * C * NF, *icxy = rxy + 2 * C * NF, *cc = icxy + 2 * C * NF;
    double *ee = cc + 2 * C * NF;
    LAUNCHCHK(launch_epi_elem(lc(), dxx, dyy, dxy, nch, nb, nfft, onesided, enbw, cxy, cxy2, phi, lxx, lyy, lxy));
    const size_t nsig = 3 * C + 1;
    if (g.bigA.ensure(sizeof(cf) * nsig * NF) || g.epi.ensure(sizeof(double) * (C + 1))) return -1;
    cf *X = (cf *)g.bigA.p;
    // the rows' scales: the inverse transforms run in float32 on rows normalised to O(1) (k_epilogue.hip)
    double *rowmax = (double *)g.epi.p;
    LAUNCHCHK(launch_epi_spec(lc(), dxx, dyy, dxy, cxy, nch, nb, nfft, onesided, X, rowmax));
    if (dev_fft_any(X, X, nfft, (int64_t)nsig, 1)) return -1;
    LAUNCHCHK(launch_epi_corr(lc(), X, nch, nfft, onesided, rxx, ryy, rxy, icxy, ee, cc, rowmax));
    return st.finish();
}

int64_t sp_csd_epilogue_doubles(int nch, int nb, int nfft) {
    const int64_t C = nch, NB = nb, NF = nfft;
    return 2 * C * NB + C * NB + C * NB + NB + C * NB + C * NB + 2 * NF + 4 * 2 * C * NF + 2 * (1 + C);
}

int sp_biquad(const double *b, const double *a, const float *x, int64_t n, float *y, int mem) {
    if (ensure_init()) return -1;
    if (n < 1 || b == nullptr || a == nullptr) return fail("sp_biquad: bad arguments");
    if (a[0] == 0.0) return fail("sp_biquad: a[0] must not be zero");
    {   // the blocked scan raises the state map to powers up to n: an unstable section overflows them to inf and inf * 0 = NaN
        // would reach every output (scipy's lfilter returns the valid early samples) -- refuse instead
        const double a1 = a[1] / a[0], a2 = a[2] / a[0], disc = a1 * a1 - 4.0 * a2;
        const double rad = disc < 0.0 ? sqrt(a2) : 0.5 * (fabs(a1) + sqrt(disc));
        if (!(rad <= 1.0 + 1e-12))
            return fail("sp_biquad: unstable section (pole radius %.9g > 1): the blocked scan of the state maps does not apply", rad);
    }
    ApiLock lk;
    const size_t bytes = sizeof(float) * (size_t)n;
    Stage st(mem);
    const float *xd;
    float *yd;
    st.in(g.in0, x, bytes, &xd);
    st.out(g.out0, y, bytes, &yd);
    if (st.commit()) return -1;
    if (g.work.ensure(sizeof(double) * 4 * (size_t)biquad_tiles(n) + 64)) return -1;
    LAUNCHCHK(launch_biquad(lc(), b, a, xd, n, yd, (double *)g.work.p));
    return st.finish();
}

int sp_fftfilt(const float *h, int ntaps, const float *x, int64_t n, int nfft, float *y, int mem) {
    if (ensure_init()) return -1;
    if (ntaps < 1 || n < 1) return fail("sp_fftfilt: bad sizes");
    if (nfft == 0) {
        int64_t c = next_pow2(8 * (int64_t)ntaps);
        if (c < 1024) c = 1024;
        if (c > SP_MAX_WG_FFT) c = SP_MAX_WG_FFT;
        nfft = (int)c;
    }
    if (!(is_pow2(nfft) && nfft >= 2 && nfft <= SP_MAX_WG_FFT) || nfft < 2 * (ntaps - 1) || nfft <= ntaps - 1)
        return fail("sp_fftfilt: nfft=%d must be a power of two with 2*(ntaps-1) <= nfft <= %d", nfft, SP_MAX_WG_FFT);
    ApiLock lk;
    Xf xf;
    if (get_xf(nfft, &xf)) return -1;
    // Hs = FFT(h zero-padded)/nfft, cached per (taps, nfft)
    std::vector<cf> hp((size_t)nfft, make_float2(0.f, 0.f));
    for (int i = 0; i < ntaps; ++i) hp[(size_t)i] = make_float2(h[i] / (float)nfft, 0.f);
    void *H_d;
    bool fresh = false;
    if (get_table(2, hp.data(), sizeof(cf) * (size_t)nfft, &H_d, &fresh)) return -1;
    if (fresh) LAUNCHCHK(launch_fft_c2c(lc(), (const cf *)H_d, (cf *)H_d, 1, 0, xf));
    const size_t bytes = sizeof(float) * (size_t)n;
    Stage st(mem);
    const float *xd;
    float *yd;
    st.in(g.in0, x, bytes, &xd);
    st.out(g.out0, y, bytes, &yd);
    if (st.commit()) return -1;
    LAUNCHCHK(launch_fftfilt(lc(), xd, n, ntaps, (const cf *)H_d, xf, yd));
    return st.finish();
}

// checks shared by sp_sosfilt / sp_sosfiltfilt: refuses before any launch
static int sos_check(const char *who, const double *sos, int nsec) {
    if (sos == nullptr) return fail("%s: sos is NULL", who);
    if (nsec < 1 || nsec > SP_SOS_MAXK) return fail("%s: %d sections; 1 to %d are supported (filter order <= %d)", who, nsec,
                                                    SP_SOS_MAXK, 2 * SP_SOS_MAXK);
    for (int k = 0; k < nsec; ++k) {
        const double *r = sos + 6 * k;
        for (int i = 0; i < 6; ++i)
            if (!isfinite(r[i])) return fail("%s: section %d has a non-finite coefficient", who, k);
        if (r[3] == 0.0) return fail("%s: section %d has a0 = 0", who, k);
        // the scan raises the state maps to powers up to the record length: an unstable section would overflow them
        const double a1 = r[4] / r[3], a2 = r[5] / r[3], disc = a1 * a1 - 4.0 * a2;
        const double rad = disc < 0.0 ? sqrt(a2) : 0.5 * (fabs(a1) + sqrt(disc));
        if (!(rad <= 1.0 + 1e-12))
            return fail("%s: section %d is unstable (pole radius %.9g > 1): the blocked scan of the state maps does not apply", who,
                        k, rad);
    }
    return 0;
}

static int sos_plan_table(const double *sos, int nsec, int64_t len, const double **plan_d) {
    std::vector<double> plan((size_t)sos_plan_doubles(nsec));
    sos_build_plan(sos, nsec, len, plan.data());
    void *d = nullptr;
    if (get_table(5, plan.data(), sizeof(double) * plan.size(), &d, nullptr)) return -1;
    *plan_d = (const double *)d;
    return 0;
}

int sp_sosfilt(const double *sos, int nsec, const float *x, int64_t nrows, int64_t n, const double *zi, float *y, double *zf,
               int mem) {
    if (sos_check("sp_sosfilt", sos, nsec)) return -1;
    if (x == nullptr || y == nullptr || nrows < 1 || n < 1) return fail("sp_sosfilt: bad arguments");
    if (ensure_init()) return -1;
    ApiLock lk;
    const int S = 2 * nsec;
    const double *plan_d;
    if (sos_plan_table(sos, nsec, n, &plan_d)) return -1;
    const size_t bytes = sizeof(float) * (size_t)(nrows * n), zbytes = sizeof(double) * (size_t)(nrows * S);
    Stage st(mem);
    const float *xd;
    float *yd;
    const double *zid;
    double *zfd;
    st.in(g.in0, x, bytes, &xd);
    st.out(g.out0, y, bytes, &yd);
    st.in(g.sosZ, zi, zbytes, &zid);
    st.out(g.sosZ, zf, zbytes, &zfd);
    if (st.commit()) return -1;
    if (g.work.ensure(sizeof(double) * (size_t)sos_work_doubles(nsec, n, nrows) + 64)) return -1;
    const SosIO io{xd, n, n, n, 0, 0, 0, yd, n, 0, n};
    LAUNCHCHK(launch_sos_pass(lc(), nsec, plan_d, io, nrows, zid ? 1 : 0, zid, zfd, (double *)g.work.p));
    return st.finish();
}

int sp_sosfiltfilt(const double *sos, int nsec, const float *x, int64_t nrows, int64_t n, int padtype, int64_t padlen, float *y,
                   int mem) {
    if (sos_check("sp_sosfiltfilt", sos, nsec)) return -1;
    if (x == nullptr || y == nullptr || nrows < 1 || n < 1) return fail("sp_sosfiltfilt: bad arguments");
    if (padtype < 0 || padtype > 3) return fail("sp_sosfiltfilt: padtype must be 0 (none), 1 (odd), 2 (even) or 3 (constant)");
    if (padlen < 0) return fail("sp_sosfiltfilt: padlen must not be negative");
    if (padtype == 0) padlen = 0;
    if (padlen > 0 && n <= padlen)
        return fail("sp_sosfiltfilt: the signal length (%lld) must be greater than padlen (%lld)", (long long)n, (long long)padlen);
    for (int k = 0; k < nsec; ++k) {            // sosfilt_zi: a section with a pole at z = 1 has no steady state
        const double *r = sos + 6 * k;
        if (r[3] + r[4] + r[5] == 0.0) return fail("sp_sosfiltfilt: section %d has a pole at z = 1 (no steady state)", k);
    }
    if (ensure_init()) return -1;
    ApiLock lk;
    const int64_t N = n + 2 * padlen;
    const double *plan_d;
    if (sos_plan_table(sos, nsec, N, &plan_d)) return -1;
    const size_t bytes = sizeof(float) * (size_t)(nrows * n);
    Stage st(mem);
    const float *xd;
    float *yd;
    st.in(g.in0, x, bytes, &xd);
    st.out(g.out0, y, bytes, &yd);
    if (st.commit()) return -1;
    if (g.sosY.ensure(sizeof(float) * (size_t)(nrows * N)) ||
        g.work.ensure(sizeof(double) * (size_t)sos_work_doubles(nsec, N, nrows) + 64))
        return -1;
    float *mid = (float *)g.sosY.p;
    // forward over the extended record into the scratch, from zss * x_ext[0]; then backwards over it from zss * its last
    // sample, keeping [padlen, padlen + n) -- two passes on one stream, no host synchronisation in between
    const SosIO fwd{xd, n, n, N, padlen, padtype, 0, mid, N, 0, N};
    const SosIO bwd{mid, N, N, N, 0, 0, 1, yd, n, padlen, n};
    LAUNCHCHK(launch_sos_pass(lc(), nsec, plan_d, fwd, nrows, 2, nullptr, nullptr, (double *)g.work.p));
    LAUNCHCHK(launch_sos_pass(lc(), nsec, plan_d, bwd, nrows, 2, nullptr, nullptr, (double *)g.work.p));
    return st.finish();
}

}   // extern "C"
