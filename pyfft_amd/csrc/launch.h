// launch.h -- host-side launchers, one translation unit per kernel family so they compile in parallel.
#pragma once
#include <limits.h>
#include <stdlib.h>
#include "kernels.h"
#include "nufft_plan.h"
#include "ar_plan.h"
#include "sub_plan.h"
#include "dwt_plan.h"
#include "beam_plan.h"
#include "cond_plan.h"
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace sp {

// Run-time test hooks.  Each forces a live alternative path so that a test can compare two implementations, and each is
// read on every call (never cached), so that setting or clearing it takes effect at once:
//   SP_NO_REALPAIR, SP_WELCH_GENERIC, SP_WELCH_TWOPASS, SP_WELCH_PIPE (int: 0 off, 2 for any frame count)
//   SP_OP_UNFUSED, SP_OP_NOLOBESUM
//   SP_CSDM_SPLIT3, SP_CSDM_FP32, SP_CSDM_NOPIPESPEC, SP_CSDM_TWOPASS, SP_CSDM_TRANSPOSED
//   SP_CSD_XIY, SP_CSD_ONEPASS, SP_CSD_TWOPASS
//   SP_STFT_NOFAST, SP_COG_TWOPASS, SP_COG_GENERIC
//   SP_HILBERT_NOFUSEMID, SP_HILBERT_PAIRLOAD, SP_COLS_NOHALF, SP_XC_NOFUSEMID, SP_BIGFFT_5PASS
//   SP_DIST_RESERVE_CUS, SP_DIST_RCCL_CTAS (int: the sharded PSD's CU reserve and the communicator's workgroup limit)
//   SP_BISPEC_MIB (int: the bispectrum's spectra and partials budget per frame chunk, MiB)
//   SP_ISTFT_FPG, SP_ISTFT_MIB (int: the inverse STFT's frames per run; its budget for transposed bin-major spectra, MiB)
//   SP_PFB_FPG, SP_PFB_TREG (int: the channelizer's frames per run; 0 / 1: its taps from the table / held in registers)
//   SP_PFBS_FPG, SP_PFBS_PATH (int: the synthesis bank's frames per run; "fused" / "composed": its path, a fused that does not fit is refused)
//   SP_XCF_FPG (int: the short-time correlation's frames per run)
//   SP_SKF_FPG, SP_SKF_CELLS (int: the wavenumber-frequency histogram's frames per run; a cap on the cells nk x bins of a tile)
//   SP_EIGH_GRID (int: the eigensolver's workgroups, so that a small batch walks the batch loop)
//   SP_CWT_CHUNK (int: the wavelet transform's scales per workgroup, where no output needs the whole scale set in one)
//   SP_WCT_CHUNK (int: the same for the cross-wavelet and coherence kernel)
//   SP_SSQ_FPG (int: the synchrosqueezed STFT's frames per run)
//   SP_WVD_CPR (int: the Wigner-Ville kernel's columns per run)
//   SP_LONG_CHUNK_FRAMES (int: a cap on the frames per chunk of the long-segment paths, long_chunk_frames)
//   SP_LONG_SLICE_ROWS (int: a cap on the rows per slice of a batch of long transforms, dev_fft_any and sp_czt)
//   SP_CSDM_CHUNK_FRAMES (int: a cap on the frames per chunk of sp_csd_matrix, before the chunks are equalised)
//   SP_CYCLIC_CHUNK (int: a cap on the cycle frequencies per pass of sp_cyclic, before its partials fill their budget)
//   SP_CYCLIC_FPG (int: sp_cyclic's frames per group, so that a small shape walks the kernel's frame loop and its clamped tail)
//   SP_LOMB_FREQS (int: a cap on the frequencies per pass of sp_lomb / sp_lomb_sums, before the partials fill their budget)
//   SP_LOMB_SPLIT (int: the sample runs sp_lomb deals a record into, so that a small record walks the sum over the runs)
//   (the last six: unset or <= 0 leaves the budget alone; sp_last_passes reports the passes a call made)
//   SP_WBIC_CHUNK (int: a cap on the samples per pass of sp_wbic, which reports its passes itself; unset or <= 0: the budget alone)
//   SP_FAM_BLOCKS (int: a cap on the blocks per pass of sp_fam; unset or <= 0: the budget alone; sp_last_passes(5) reports the passes)
//   SP_NUFFT_ROWS (int: a cap on the rows per pass of sp_nufft1 / sp_nufft2 / sp_lomb_sums_grid, before the fine grids fill their budget; unset or
//                  <= 0: the budget alone; sp_last_passes(6) reports the passes)
//   SP_AR_SEGS (int: a cap on the segments per pass of sp_burg / sp_yule; unset or <= 0: the budget alone; sp_last_passes(7) reports the passes)
//                  the same cap holds for sp_covmat / sp_ar_ls, whose passes sp_last_passes(8) reports
//   SP_DWT_ROWS (int: a cap on the rows per pass of the tile form of sp_dwt / sp_idwt / sp_modwt / sp_imodwt; unset or <= 0: the budget alone;
//                  sp_last_passes(9) reports the passes)
//   SP_BEAM_GRID (int: a cap on the workgroups of sp_beamscan, so that a small call walks the loop over its (model, tile) items past the
//                  first; unset or <= 0: the plan's own grid)
//   SP_COND_GRID (int: a cap on the workgroups of sp_cond, so that a small call walks the loop over its matrices past the first; unset or
//                  <= 0: the plan's own grid)
//   SP_BURG_FORM (int: 1 the wave form of k_burg wherever a segment fits it, 2 the workgroup form at every length; unset or 0: by length)
inline bool env_flag(const char *name) {
    const char *v = getenv(name);
    return v && v[0] && v[0] != '0';
}
inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

struct LaunchCtx {
    hipStream_t stream;
    int ncu;
    // optional: recorded as the launch's own completion signal (hipExtLaunchKernelGGL) by the launchers that honour it
    // (launch_welch_pipe) -- a hipEventRecord behind the kernel is a packet of its own and costs the next launch on the
    // stream 3-5 us (tools/ubench/coexec_rccl.hip)
    hipEvent_t stop = nullptr;
};

// transform selection for a length n: pow2 workgroup FFT, or Bluestein on an L-point one
struct Xf {
    XfTables tb;
    int L;
    bool blue;
};

constexpr int fpw_of(int L) {
    const int R = L < 16 ? L : 16, T = L / R, WG = T >= 256 ? T : 256;
    return WG / T;
}
// LDS of `nbuf` transform images for each of a workgroup's groups: L + 16 complex per image
constexpr size_t xf_image_bytes(int L, int nbuf = 1) { return (size_t)fpw_of(L) * (size_t)(L + 16) * 8 * nbuf; }
template <int L> constexpr bool xf_image_agrees() {
    if constexpr (L < 8192) {
        if (!xf_image_agrees<2 * L>()) return false;
    }
    return WgCfg<L>::FPW == fpw_of(L) && WgCfg<L>::lds_bytes(1) == xf_image_bytes(L) && WgCfg<L>::lds_bytes(2) == xf_image_bytes(L, 2);
}
static_assert(xf_image_agrees<32>(), "fpw_of and xf_image_bytes are the kernels' FPW and lds_bytes at every L of 32 .. 8192");

// The dynamic LDS a workgroup may take on gfx950, and the one place that lifts a kernel's limit to it: 0, or -1 where lds_bytes is
// beyond SP_LDS_MAX or the runtime refuses.  Below 64 KiB nothing is asked.  The limit is only a cap: a launch occupies the lds_bytes
// it passes.  The raise is remembered per instantiation for the life of the process, which assumes that the process is bound to one
// device, as sp_init enforces; it outlives sp_shutdown, so an sp_init on another device afterwards finds the raise already recorded.
#define SP_LDS_MAX ((size_t)160 * 1024)
template <auto K> int lds_raise(size_t lds_bytes) {
    static size_t raised = 64 * 1024;
    if (lds_bytes <= raised) return 0;
    if (lds_bytes > SP_LDS_MAX ||
        hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SP_LDS_MAX) != hipSuccess)
        return -1;
    raised = SP_LDS_MAX;
    return 0;
}

// f(XfTag<XfPow2<L>>{}) for a power of two L in LO .. HI, -1 outside: only the lengths of the range are instantiated
template <class X> struct XfTag {
    using type = X;
};
template <int LO, int HI, class F> int for_pow2(int L, F f) {
    if (L == LO) return f(XfTag<XfPow2<LO>>{});
    if constexpr (LO < HI) return for_pow2<2 * LO, HI>(L, f);
    else return -1;
}

// `runs` runs of `per` consecutive items cover the n items, the last run not empty
inline bool runs_cover(int64_t n, int64_t per, int64_t runs) {
    return runs >= 1 && runs <= 0x7fffffff && (runs - 1) * per < n && runs * per >= n;
}
// the nb bins from b0 on lie inside an L-point spectrum: anywhere modulo L for complex records, within 0 .. L / 2 for real ones
inline bool band_in_transform(bool cplx, int L, int b0, int nb) {
    return nb >= 1 && b0 >= 0 && b0 < L && nb <= L && (cplx || b0 + nb <= L / 2 + 1);
}

// frames are dealt to transform groups in contiguous runs
struct RunPart {
    int64_t groups, fpg;
    int blocks;
};
// groups_per_cu: 4 by default = two rounds at the 2 resident workgroups per CU of the 200-VGPR segment kernels.  Measured
// on the metric shape (bench.py step / kernel, ms): 2 -> 0.651 / 0.607, 4 -> 0.660 / 0.605, 8 -> 0.680 / 0.634,
// 3 -> 0.73 / 0.685 (one and a half rounds), 6 ~ 8, 12 and 24 worse: longer runs amortise the per-workgroup prologue
// (twiddle constants, first frame) and halve the partial spectra the epilogue has to sum.
inline RunPart run_partition(int L, int64_t nframes, int ncu, int groups_per_cu = 0) {
    if (groups_per_cu <= 0) groups_per_cu = 4;
    const int fpw = fpw_of(L);
    const int64_t target = (int64_t)ncu * groups_per_cu * fpw;
    int64_t f = (nframes + target - 1) / target;
    if (f < 1) f = 1;
    const int64_t G = (nframes + f - 1) / f;
    RunPart r;
    r.fpg = f;
    r.blocks = (int)((G + fpw - 1) / fpw);
    r.groups = (int64_t)r.blocks * fpw;
    return r;
}
// the same for kernels whose grid has a second dimension of `ny` independent rows (channels): about 8 workgroups per
// CU in total, so that the per-group partial spectra (ny x groups x 3..4 x L floats) stay small -- with 63 channels the
// per-CU rule above wrote and re-read 1.6 GB of partials
// slots (optional) = workgroups the whole GPU keeps resident for this kernel: the group count per row is then rounded so that the
// grid is just under a whole number of rounds (63 channels x 33 groups = 2079 workgroups over 512 slots ran a fifth round of 31;
// 32 groups = 2016 run four: 2.51 -> 2.41 ms for the reference against 63 channels of 2^24 samples)
inline RunPart run_partition_2d(int L, int64_t nframes, int ncu, int ny, int64_t slots = 0) {
    const int fpw = fpw_of(L);
    int64_t target = ((int64_t)ncu * 8 + ny - 1) / (ny > 0 ? ny : 1) * fpw;
    if (target < 8 * fpw) target = 8 * fpw;
    int64_t f = (nframes + target - 1) / target;
    if (f < 1) f = 1;
    if (slots > 0 && ny > 0) {
        const int64_t wg = ((nframes + f - 1) / f + fpw - 1) / fpw * ny;          // workgroups of the default rule
        int64_t rounds = (wg + slots / 2) / slots;
        if (rounds < 1) rounds = 1;
        const int64_t groups = rounds * slots / ny * fpw;                          // groups per row that fill `rounds` rounds
        if (groups >= 1) {
            const int64_t f2 = (nframes + groups - 1) / groups;
            if (f2 >= 1 && f2 <= 4 * f) f = f2;
        }
    }
    const int64_t G = (nframes + f - 1) / f;
    RunPart r;
    r.fpg = f;
    r.blocks = (int)((G + fpw - 1) / fpw);
    r.groups = (int64_t)r.blocks * fpw;
    return r;
}
// grid of the row kernels (FFT rows, Hilbert rows, FIR block pairs): every workgroup pays a prologue (twiddle constants with
// 30 divisions per twiddled pass) before its first row, so few, long-lived workgroups win for the long transforms -- measured
// (ms): 4096 rows of 4096: 0.088 at 16 blocks per CU, 0.062 at 4, 0.055 at 2; 65536 rows: 0.825 / 0.790 /
// 0.823; 8192 points: 0.245 / 0.170 / 0.160; 2048 points: 4 per CU wins for 4096 rows (0.039 vs 0.050), 16 for 65536 rows
// (0.394 vs 0.413); <= 1024 points: no difference.  Rule: 4 per CU from 4096 points up; at 2048 points at least 4 rows per
// workgroup (not below 2 per CU); 16 per CU otherwise.
// per_cu: the cap for L >= 4096 in workgroups per CU -- a multiple of what the kernel keeps resident per CU, so that the last
// round of workgroups is a full one (round 3: k_fft_c2c<4096> holds 3 per CU; 4 per CU = 1024 workgroups ran 768 + a 256 tail:
// 0.88 against 0.79 ms at 12 per CU for 65536 rows; the batched Hilbert, 4 rows per workgroup at 4096 rows: 0.065 -> 0.060 at 3)
inline int strided_blocks(int L, int64_t items, int ncu, int per_cu = 4) {
    const int fpw = fpw_of(L);
    int64_t b = (items + fpw - 1) / fpw;
    int64_t cap = (int64_t)ncu * (L >= 4096 ? per_cu : 16);
    if (L == 2048) {
        const int64_t q = b / 4;
        if (q < cap) cap = q > (int64_t)ncu * 2 ? q : (int64_t)ncu * 2;
    }
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// workgroups of `fn` one CU keeps resident (registers, LDS, wave slots; asked once per kernel from the runtime): grids and run
// partitions are sized as a multiple of it, so that the last round of workgroups is a full one
int resident_per_cu(const void *fn, int threads, size_t lds_bytes);
// groups per CU for k_welch_rp's run partition at this transform (a multiple of what the selected instantiation keeps resident)
int welch_rp_groups_per_cu(const Xf &xf, bool lin);
int csd_pair_resident(const Xf &xf, bool lin, bool onepass);
int stft_rp_groups_per_cu(const Xf &xf, bool lin, int hop, int sided, int out_power, bool pseg);

// every launcher returns 0 or -1 (unsupported L); kernel launch errors surface through hipGetLastError
int launch_fft_c2c(LaunchCtx c, const cf *in, cf *out, int64_t batch, int inverse, const Xf &xf,
                   BigTw bt = BigTw{nullptr, nullptr, 0, 0});
int launch_fft_cols(LaunchCtx c, const cf *in, cf *out, int64_t ncols, int64_t nouter, int64_t es, int64_t os, int64_t twmul,
                    int conj_in, const Xf &xf, BigTw bt, int64_t hmask_n = 0,
                    ColsIn ci = ColsIn{0, nullptr, nullptr, nullptr, 0}, int tw_outer = 0);
int launch_fft_rows_rev(LaunchCtx c, const cf *in, cf *out, int64_t A, int64_t B, int conj_out, float scale, const Xf &xf,
                        RowsOut ro = RowsOut{nullptr, 0, 0, nullptr});
// elementwise / transpose pieces of the long paths (k_fft.hip)
int launch_transpose_c(LaunchCtx c, const cf *in, cf *out, int64_t rows, int64_t cols, int conj, float scale, int64_t batch = 1);
int launch_pack_real(LaunchCtx c, const float *x, int64_t n_in, const double *mean, int64_t L, cf *out);
int launch_cmul_vec(LaunchCtx c, const cf *a, const cf *b, int64_t n, int conj_out, cf *out, int64_t batch = 1);
int launch_blue_pre(LaunchCtx c, const cf *in, const cf *chirp, int64_t n, int64_t L, int conj_in, cf *out, int64_t batch = 1);
int launch_blue_post(LaunchCtx c, const cf *in, const cf *chirp, int64_t n, int conj_out, float scale, cf *out, int64_t batch = 1,
                     int64_t in_ld = 0);
int launch_hilbert_mask(LaunchCtx c, cf *X, int64_t n);
int launch_xc_pack(LaunchCtx c, const float *x1, const float *x2, int64_t n, int64_t L, const double *mom, cf *z);
int launch_xc_mid(LaunchCtx c, const cf *Z, int64_t L, cf *R);
int launch_xc_mid_half(LaunchCtx c, const cf *Z, int64_t L, BigTw bt, cf *Zp);
int launch_xc_out(LaunchCtx c, const cf *r, int64_t n, int64_t L, const double *mom, float *co);
bool welch_carry_eligible(const Xf &xf, int hop, bool lin);
int launch_welch(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                 bool lin, const Xf &xf, float *partial, const RunPart &rp, bool allow_carry, cf *spartial,
                 const char **kname, int segmean = 0);
bool welch_pipe_eligible(const Xf &xf, int hop);
int launch_welch_pipe(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, float *trend,
                      const Xf &xf, float *partial, const RunPart &rp, cf *spartial, int mode = 0, int nch = 1, int64_t x_cs = 0,
                      int gpr = 0);
int launch_op_estimate(LaunchCtx c, const void *x, bool cplx, int64_t nsig, double *part, float *trend);
int launch_op_reduce(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *partial, const cf *spartial,
                     int64_t G, const Xf &xf, int hop, int64_t nframes, int64_t nmean, OnePass st, double *sum_out);
int launch_op_finish(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *win, OnePass st,
                     const double *mean_in, int64_t nmean, const Xf &xf, int hop, int64_t nframes, cf *cw, const cf *Wf,
                     int sided, double scale, double *out, bool export_state = false);
// mean (device, optional): apply this (re, im) mean instead of the state's own sample sum / count
int launch_op_apply(LaunchCtx c, const double *state, const cf *Wf, int n, int sided, double scale, double *out,
                    const double *mean = nullptr);
// one-pass sharded state for any hop and any workgroup transform (k_welch_opx.hip).  Scratch: partial[G][L] floats, cpart[G][n],
// A[n], csum[2n], tpart[2 * opx_tot_blocks()] doubles
int opx_tot_blocks();
int launch_welch_opx(LaunchCtx c, const void *x, bool cplx, bool pair, const float *win, int hop, int64_t nframes,
                     const float *trend, const Xf &xf, const RunPart &rp, float *partial, cf *cpart);
int launch_opx_reduce(LaunchCtx c, const float *partial, const cf *cpart, int64_t G, const Xf &xf, const void *x, bool cplx,
                      const float *trend, int hop, int64_t nframes, int64_t nmean, double *A, double *csum, double *tpart);
int launch_opx_finish(LaunchCtx c, const float *win, const double *A, const double *csum, const double *tpart, const float *trend,
                      int hop, int64_t nframes, int64_t nmean, bool sym, const Xf &xf, double *out);
// colsums + finish (or export) in one launch for a window whose spectrum is confined to the bins -3 .. 3 (k_op_fused)
int launch_op_fused(LaunchCtx c, const void *x, bool cplx, const float *trend, const float *win, const float *partial,
                    const cf *spartial, int64_t G, int n, int hop, int64_t nframes, int64_t nmean, OnePass st, unsigned *ticket,
                    CogLobe lb, const double *mean_in, int sided, double scale, double *out, bool export_state,
                    OpPrev prev = OpPrev{nullptr, nullptr, nullptr, 0, 0.0}, bool light = false, double cola_c = 0.0);
int launch_welch_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int sided, double scale, double *out,
                        int sym = 0);
int launch_welch_rp(LaunchCtx c, const float *x, const float *win, int hop, int64_t nframes, const float *trend, bool lin,
                    const Xf &xf, float *partial, const RunPart &rp);
int launch_stft_rp(LaunchCtx c, const float *x, const float *win, int hop, int64_t nframes, const float *trend, bool lin,
                   const Xf &xf, const RunPart &rp, int sided, float amp, int out_power, void *out, double *pseg,
                   int nchan = 1, int64_t x_cs = 0, int64_t out_cs = 0, int out_ld = 0);
int launch_csd(LaunchCtx c, const void *x, const void *y, bool cplx, int nch, int64_t y_ld, const float *win, int hop,
               int64_t nframes, const float *trend_x, const float *trend_y, bool lin, const Xf &xf, float *partial,
               const RunPart &rp, int segmean = 0);
int launch_csd_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                      double *pxx, double *pyy, double *pxy);
int launch_stft(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                bool lin, const Xf &xf, const RunPart &rp, int sided, float amp, int out_power, void *out, double *pseg, int segmean = 0,
                cf *cog = nullptr, int klo = 0, int khi = 0);
int launch_cog_finish(LaunchCtx c, const cf *acc, int wpf, int64_t nframes, double df, double *out);
int launch_cog_carry(LaunchCtx c, const void *x, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                     const Xf &xf, cf *cog, const RunPart &rp, int klo, int khi);
bool csd_rp_eligible(const Xf &xf);
int launch_csd_rp(LaunchCtx c, const float *x, const float *y, int nch, int64_t y_ld, const float *win, int hop,
                  int64_t nframes, const float *trend_x, const float *trend_y, bool lin, const Xf &xf, float *partial,
                  const RunPart &rp);
int launch_csd_rp_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                         double *pxx, double *pyy, double *pxy);
int launch_pairspec(LaunchCtx c, const float *x, const float *win, int hop, int64_t nframes, const float *trend, bool lin,
                    const Xf &xf, const RunPart &rp, cf *Zx);
int launch_csd_pair(LaunchCtx c, const float *y, int nch, int64_t y_ld, const float *win, int hop, int64_t nframes,
                    float *trend_y, bool lin, const Xf &xf, const cf *Zx, float *partial, const RunPart &rp, cf *spartial = nullptr);
int launch_csd_pair_finish(LaunchCtx c, const float *partial, int64_t G, const Xf &xf, int nch, int sided, double scale,
                           double *pyy, double *pxy, const double *st_y = nullptr, const double *st_x = nullptr, const cf *Wf = nullptr,
                           const float *trend_x = nullptr, const float *trend_y = nullptr, int64_t nmean = 0, int64_t M = 0);
#define SP_COLSUM_SLICES 256
int launch_colsum_real(LaunchCtx c, const float *x, const float *trend, int H, int64_t M, cf *out);
int launch_csdm_finish(LaunchCtx c, double *G, int nch, int nb, double scale);
int launch_csdm_transpose_kgc(LaunchCtx c, const cf *Xs, cf *Xt, int nch, int nchp, int64_t m, int64_t mp, int nb);
int launch_csdm_mfma(LaunchCtx c, const cf *Xt, int nch, int nchp, int64_t mp, int nb, double *G);
int launch_csdm_bf16(LaunchCtx c, const cf *Xs, cf *Xt_tail, int nch, int64_t m, int nb, double *G, int ld, int two_pieces = 0, int init = 0);
int launch_csdm_fold(LaunchCtx c, const double *H, double *G, int nch, int n, const double *st = nullptr, const cf *Wf = nullptr,
                     const float *trend = nullptr, int64_t nmean = 0, int64_t M = 0, double scale = 1.0, int init = 0);
int launch_cm_blocksums(LaunchCtx c, const cf *spartial, int nch, int runs, int hop, double *Sl);
int launch_op_finish_channels(LaunchCtx c, const void *x, int64_t x_cs, int nch, const float *trend, const float *win,
                              const double *Sl, const cf *Wf, int hop, int64_t nframes, int64_t nmean, const Xf &xf, double *out,
                              bool cplx = false);
int launch_cog_finish_op(LaunchCtx c, const cf *acc, int wpf, int64_t nframes, double df, double *out, const cf *lobe, CogLobe lb,
                         const double *st, const float *trend, int64_t nmean, int n);
int launch_csdm_fused(LaunchCtx c, const cf *Xs, cf *Xt_tail, int nch, int64_t m, int nb, double *G, int ld = 0);
int launch_hilbert_mid(LaunchCtx c, cf *Z, int64_t M, BigTw bt);
// half-length Hilbert with the middle step inside the row pass + the two adjoint column passes (k_hilbert_rowsmid, k_fft_cols_inv)
int launch_hilbert_rowsmid(LaunchCtx c, cf *Tm, int64_t A, int64_t B, const Xf &xc, BigTw btN, const cf *tw2c);
// long ccf with the middle step and the half-length transform's first pass inside the row pass (k_xc_rowsmid, k_fft_cols_lag)
int launch_xc_rowsmid(LaunchCtx c, cf *Tm, int64_t A, int64_t B, const Xf &xc, const Xf &xc2, BigTw btL, BigTw btM);
int launch_fft_cols_lag(LaunchCtx c, const cf *in, int64_t ncols, int64_t nouter, int64_t es, int64_t os, const Xf &xf, RowsOut ro);
int launch_fft_cols_inv(LaunchCtx c, const cf *in, cf *out, int64_t ncols, int64_t nouter, int64_t es, int64_t os, int64_t twmul,
                        const Xf &xf, BigTw bt, float scale, const RowsOut *analytic);
int launch_hilbert(LaunchCtx c, const float *x, int64_t n_in, int64_t x_ld, int64_t batch, const Xf &xf, cf *out,
                   const cf *H = nullptr);
int launch_spec_mul(LaunchCtx c, cf *X, const cf *H, int64_t n);
int frame_sum_slices(int ncu, int nch, int nfft, int64_t nframes);
int launch_frame_sum(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int nch, int nfft, int hop, int64_t nframes,
                     const float *trend, bool lin, double *out, double *part);
int launch_fftfilt(LaunchCtx c, const float *x, int64_t n, int ntaps, const cf *Hs, const Xf &xf, float *y);
int launch_xcorr(LaunchCtx c, const float *x1, const float *x2, int64_t n, const double *mom, const Xf &xf, float *co);
int launch_moments(LaunchCtx c, const void *x, bool cplx, int64_t n, int mode, double *partial_scratch, double *out_d,
                   float *trend_f, int nsignals = 1, int64_t x_cs = 0);
int launch_moments_xc(LaunchCtx c, const float *x, int64_t n, double *partial, double *out_d, double *xc_out, int64_t x_cs);
int launch_transpose(LaunchCtx c, const void *in, void *out, int64_t rows, int64_t cols, int elem_bytes);
// segments longer than one workgroup transform (k_long.hip); m frames starting at frame f0, rows S[m][nfft]
int launch_long_segstats(LaunchCtx c, const void *x, bool cplx, int64_t f0, int64_t m, int hop, int nfft, int mode, float *rec);
int launch_long_pack(LaunchCtx c, const void *x, bool cplx, const float *win, int nfft, int hop, int64_t f0, int64_t m,
                     const float *trend, bool lin, const float *segrec, cf *S, double *pseg);
int launch_long_acc_psd(LaunchCtx c, const cf *S, int64_t m, int nfft, double *acc);
int launch_long_acc_csd(LaunchCtx c, const cf *Sx, const cf *Sy, int64_t m, int nfft, double *ayy, double *axy);
int launch_long_finish(LaunchCtx c, const double *acc, int nfft, int sided, double scale, bool cplx, double *out);
int launch_long_stft_out(LaunchCtx c, const cf *S, int64_t m, int nfft, int sided, float amp, int out_power, void *out,
                         int64_t f0, int nb);
int launch_long_cog(LaunchCtx c, const cf *S, int64_t m, int nfft, int klo, int khi, cf *acc, int64_t f0);

// exact second-order IIR section (k_iir.hip)
int64_t biquad_tiles(int64_t n);
int launch_biquad(LaunchCtx c, const double *b, const double *a, const float *x, int64_t n, float *y, double *work);

// cascades of second-order sections (k_sos.hip).  One pass over nrows rows; where its samples come from and where its
// outputs go is an index map, so that sosfiltfilt's extension and reversal cost no copies.
#define SP_SOS_MAXK 8
struct SosIO {
    const float *x;      // source rows, row stride x_ld, n valid samples each
    int64_t x_ld, n;
    int64_t len;         // samples of the pass
    int64_t pad;         // forward: pass sample e is x_ext[e - pad] (padtype 1 odd, 2 even, 3 constant; 0: pad = 0)
    int padtype;
    int rev;             // 1: pass sample e is x[len - 1 - e] (pad = 0, n = len)
    float *y;            // pass sample e lands at y[q - out_off], q = rev ? len - 1 - e : e, when 0 <= q - out_off < out_n
    int64_t y_ld, out_off, out_n;
};
int64_t sos_tiles(int64_t len);
int64_t sos_work_doubles(int nsec, int64_t len, int64_t nrows);
int sos_plan_doubles(int nsec);
void sos_build_plan(const double *sos, int nsec, int64_t len, double *plan);
// work: sos_work_doubles(nsec, io.len, nrows) doubles; zmode 0: rest, 1: zi[nrows][2 nsec], 2: sosfilt_zi * the first sample;
// zf (or null): [nrows][2 nsec] state after the pass's last sample
int launch_sos_pass(LaunchCtx c, int nsec, const double *plan, const SosIO &io, int64_t nrows, int zmode, const double *zi,
                    double *zf, double *work);

// fft_pwelch epilogue on device-resident spectra (k_epilogue.hip)
int launch_epi_elem(LaunchCtx c, const double *pxx, const double *pyy, const double *pxy, int nch, int nb, int nfft, int onesided,
                    double enbw, double *cxy, double *cxy2, double *phi, double *lxx, double *lyy, double *lxy);
int launch_epi_spec(LaunchCtx c, const double *pxx, const double *pyy, const double *pxy, const double *cxy, int nch, int nb,
                    int nfft, int onesided, cf *X, double *rowmax /* [1 + nch] scratch: the rows' scales */);
int launch_epi_corr(LaunchCtx c, const cf *X, int nch, int nfft, int onesided, double *rxx, double *ryy, double *rxy, double *icxy,
                    double *ee, double *cc, const double *rowmax);

// bispectrum (k_bispec.hip): 64 x 64 tiles of (i, j) pairs x chunks of 256 frames over frame-major spectra [m][nb]; fp32 partials
// part[tile][chunk][3][4096] summed in float64 into acc[tile][3][4096] and p64[nb] (first: start from zero), then the nb x nb outputs
int bispec_tile_dim();
int bispec_frame_chunk();
size_t bispec_part_floats();
int launch_bispec_tile(LaunchCtx c, const cf *X, const cf *Y, const cf *Z, int nb, int c0, int64_t m, const int2 *tiles, int ntiles,
                       float *part);
int launch_bispec_pzz(LaunchCtx c, const cf *Z, int nb, int64_t m, double *ppart);
int launch_bispec_reduce(LaunchCtx c, const float *part, const double *ppart, int ntiles, int64_t m, int nb, int first, double *acc,
                         double *p64);
int launch_bispec_finish(LaunchCtx c, const double *acc, const double *p64, const int *tmap, int ntd, int nb, int c0, int sym, int64_t M,
                         void *B, double *b2, double *pzz);
int launch_bispec_trend_shift(LaunchCtx c, const float *src, float *dst, int nrec, int64_t off);

// inverse STFT (k_istft.hip): runs of `fpg` frames from [fbeg, fend) overlap-added in an LDS ring, each preceded by `halo` frames that
// are only accumulated; Z holds the frames zbase .. frame-major (zbase <= max(0, fbeg - halo)).  mode 0: two-sided spectra -> complex
// output, 1: one-sided -> real, 2: one-sided, two frames per transform (power-of-two n >= 32; fbeg, fpg and halo even).
// rcp = reciprocal envelope [period: hop][head: head_len][tail: n - hop]; emit_tail: the run that ends at frame M also writes [M hop, L)
int istft_resident(const Xf &xf, int mode);
int launch_istft(LaunchCtx c, const cf *Z, int64_t z_cs, int64_t zbase, int64_t M, int64_t fbeg, int64_t fend, int64_t fpg, int halo,
                 const float *win, float wscale, int hop, const Xf &xf, int mode, const float *rcp, int64_t head_len, int64_t skip,
                 int64_t nout, void *y, int nch, int emit_tail);
// bin-major in[ch][nb][M] -> frame-major out[ch][m][nb] for the frames f0 .. f0 + m - 1
int launch_istft_gather(LaunchCtx c, const cf *in, int64_t M, int nb, int64_t f0, int64_t m, cf *out, int nch);

// multitaper spectra (k_mtaper.hip): the frames of x (and y: cross spectra) under every taper of tapers[nblocks * ktap][n] in one
// launch; grid.y = nblocks taper blocks, each with its own partials.  rp partitions PAIRS of frames for the PSD of a real record and
// frames otherwise.  partial[nblocks][rp.groups][planes][L], planes = mtaper_partial_planes: 1 in the layout k_welch_finish reads (sym
// for a real record), 3 that of k_csd_rp_finish (mtaper_xrp_eligible), 4 that of k_csd_finish.  trend: the records of x and y.
#define SP_MTAPER_MAXK 32
bool mtaper_xrp_eligible(const Xf &xf, bool cplx);
int mtaper_partial_planes(const Xf &xf, bool cplx, bool cross);
int launch_mtaper(LaunchCtx c, const void *x, const void *y, bool cplx, const float *tapers, int nblocks, int ktap, int hop,
                  int64_t nframes, const float *trend, bool lin, const Xf &xf, float *partial, const RunPart &rp);
// out[b] = sum_k weights[k] sk[k][b] in float64 (weights: host, K <= SP_MTAPER_MAXK)
int launch_mtaper_combine(LaunchCtx c, const double *sk, int K, int64_t nb, const double *weights, double *out);

// chirp-z transform on an arc and the zoom spectra (k_czt.hip).  Device tables of one (n, m, start, step):
struct CztTables {
    const cf *tw;      // exp(-2 pi i j / L), j < L
    const cf *pre;     // e(-start j - step j^2 / 2), j < n
    const cf *post;    // e(-step k^2 / 2), k < m
    const cf *bf;      // FFT_L(wrapped e(+step i^2 / 2)) / L
    int n, m;
};
// one workgroup transform, n + m - 1 <= L, L in {512 .. 8192}: rows of n samples (row stride x_ld) -> out[batch][m]
int launch_czt_rows(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t batch, int L, const CztTables &tb, cf *out);
// frames of x (and y) under the window: frames != null -> frames[nframes][m] = amp X; else y != null -> partial[rp.groups][4][L] in
// k_csd_finish's layout; else partial[rp.groups][L] in k_welch_finish's.  trend: the records of x and y.
int launch_zoom(LaunchCtx c, const void *x, const void *y, bool cplx, const float *win, int hop, int64_t nframes, const float *trend,
                bool lin, int L, const CztTables &tb, const RunPart &rp, float amp, float *partial, cf *frames);
// the ends of the multi-pass form, rows L apart.  pre: A[b][i] = src(b, i) pre[i] zero-padded to L, src = row f0 + b of x (stride ld;
// win == null) or win * (frame f0 + b at hop ld, minus the trend record); post: out[(f0 + b) m + k] = amp A[b][k] post[k];
// acc: float64 sums over the rows of |Sx|^2 and, with Sy, |Sy|^2, Sy conj(Sx) as acc[4][m]; acc_out: scaled into the outputs
int launch_czt_pre(LaunchCtx c, const void *x, bool cplx, int64_t ld, int64_t f0, int64_t rows, const float *win, const float *trend,
                   bool lin, const cf *pre, int64_t n, int64_t L, cf *A);
int launch_czt_post(LaunchCtx c, const cf *A, int64_t L, int64_t rows, const cf *post, int64_t m, float amp, int64_t f0, cf *out);
int launch_zoom_acc(LaunchCtx c, const cf *Sx, const cf *Sy, int64_t rows, int64_t L, int64_t m, double *acc);
int launch_zoom_acc_out(LaunchCtx c, const double *acc, int64_t m, double scale, double *pxx, double *pyy, double *pxy);

// digital down-converter (k_ddc.hip): mixer + polyphase decimating FIR, one workgroup of 256 threads per tile of K outputs of a row.
// The thread grid is og x sg: an output group owns SP_DDC_R consecutive outputs, a phase group the polyphase components s = sg, sg + SG, ..
// of the q; SG = the largest power of two <= min(q, 32), so that K q, the samples a tile consumes, stays between 2048 and 4096.
#define SP_DDC_R 8
#define SP_DDC_MAXQ 64
#define SP_DDC_MAXTAPS 4095        // with q <= SP_DDC_MAXQ: at most 90720 bytes of LDS (q = 63)
struct DdcGeom {
    int q, ntaps;
    int sg, og_log2;   // phase groups; log2 of the 256 / sg output groups
    int K;             // outputs per tile
    int PP;            // taps per polyphase component, rounded up to a multiple of 4
    int NI;            // staged entries per component
    int pitch;         // LDS row pitch of a component in float2 (entry i sits at i + (i >> 5))
    int span;          // staged samples, NI q
    int W;             // entries of the phasor table
    size_t lds;        // bytes: the staged components, then the taps [q][PP]
};
inline DdcGeom ddc_geom(int q, int ntaps) {
    DdcGeom g;
    g.q = q;
    g.ntaps = ntaps;
    g.sg = 1;
    while (g.sg * 2 <= q && g.sg < 32) g.sg *= 2;
    g.og_log2 = 0;
    while ((g.sg << g.og_log2) < 256) ++g.og_log2;
    g.K = (256 / g.sg) * SP_DDC_R;
    g.PP = ((ntaps + q - 1) / q + 3) & ~3;
    g.NI = g.K + g.PP + 3;              // the sliding window's last (unused) refill reads entry K + PP + 2
    g.pitch = g.NI + (g.NI >> 5) + 1;
    while ((g.pitch & 7) != 2) ++g.pitch;   // even (the taps behind stay 16-byte aligned); rows of neighbouring phases on other banks
    g.span = g.NI * q;
    g.W = g.span + 8;
    g.lds = sizeof(float2) * (size_t)q * g.pitch + sizeof(float) * (size_t)q * g.PP;
    return g;
}
// x: rows of nsig samples (row stride x_ld) -> out[batch][nout], nout = ceil(nsig / q).  ph0: the phase of the row's first sample,
// dnu: the step per sample, both in 2^-64 turns; tab[j] = exp(-2 pi i nu j), j < g.W (null: no mixing); taps[s][p] = h[(PP - 1 - p) q + s]
// or 0 past the last tap; vec: x is 16-byte aligned
int launch_ddc(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const DdcGeom &g, uint64_t ph0,
               uint64_t dnu, const cf *tab, const float *taps, bool vec, cf *out);

// rational resampler (k_upfirdn.hip): y[m] = sum_p h[phi + p up] x[i0 - p], i0 = floor(m down / up), phi = (m down) mod up; one
// workgroup of 256 threads per tile of K consecutive outputs of a row.  Outputs a multiple of `up` apart share the taps row phi, and
// their i0 lie that multiple of `down` apart: K = up NG R, and work item w < up NG is the R = SP_UPF_R outputs w, w + up NG, .. of the
// tile.  The items are dealt to a thread grid of OT x SG: an item thread owns the R outputs of its item over the taps p = s, s + SG, ..
// of its slice s.  Few items (heavy decimation: up = 1, K small) leave room for many slices, many items run in several rounds.
// K is chosen so that a tile consumes about max(4096, 2 P) samples, P = ceil(ntaps / up), at most SP_UPF_MAXK outputs, and so that the
// LDS image stays within SP_LDS_MAX.
#ifndef SP_UPF_R           // -DSP_UPF_R=8 is the variant of profiles/resample_dropped_variants.txt
#define SP_UPF_R 4
#endif
#define SP_UPF_MAXF 256
#define SP_UPF_MAXTAPS 8191
#define SP_UPF_MAXK 4096
struct UpfGeom {
    int up, down, ntaps;
    int P;             // taps per phase, ceil(ntaps / up)
    int pitch;         // floats per phase row of the taps image [up][pitch]: P rounded up to odd
    int NG, K;         // groups of R outputs per phase class; outputs per tile
    int items;         // up NG
    int sg, sg_log2;   // tap slices (a power of two), the fast index of the thread grid
    int rounds;        // ceil(items / (256 / sg))
    int NI;            // staged samples
    int xlen;          // entries of the staged image (NI rounded up to even)
    size_t lds;        // bytes: the staged samples, the partial sums [sg][K], the taps
};
inline UpfGeom upf_geom(int up, int down, int ntaps, bool cplx) {
    UpfGeom g;
    g.up = up;
    g.down = down;
    g.ntaps = ntaps;
    g.P = (ntaps + up - 1) / up;
    g.pitch = g.P | 1;
    const size_t es = cplx ? 8 : 4;
    const int64_t want = g.P > 2048 ? 2 * (int64_t)g.P : 4096;                     // samples a tile should consume
    int64_t ng = want / ((int64_t)down * SP_UPF_R);
    if (ng > SP_UPF_MAXK / (up * SP_UPF_R)) ng = SP_UPF_MAXK / (up * SP_UPF_R);
    if (ng < 1) ng = 1;
    for (;; --ng) {
        g.NG = (int)ng;
        g.K = up * g.NG * SP_UPF_R;
        g.items = up * g.NG;
        g.sg = 1;
        g.sg_log2 = 0;
        while (g.sg * 2 * g.items <= 256 && g.sg * 2 <= g.P) {
            g.sg *= 2;
            ++g.sg_log2;
        }
        const int ot = 256 / g.sg;
        g.rounds = (g.items + ot - 1) / ot;
        g.NI = g.P + (int)(((int64_t)(g.K - 1) * down) / up) + 2;
        g.xlen = (g.NI + 1) & ~1;                                                // even: what follows stays 8-byte aligned
        g.lds = es * (size_t)g.xlen + es * (size_t)g.sg * g.K + sizeof(float) * (size_t)up * g.pitch;
        if (g.lds <= SP_LDS_MAX || ng == 1) break;
    }
    return g;
}
// x: rows of nsig samples (row stride x_ld) -> out[batch][nout] = y[m0 .. m0 + nout - 1] (float, or cf when cplx);
// taps[phi][p] = h[phi + p up] or 0 past the last tap, row pitch g.pitch; vec: x is 16-byte aligned
int launch_upfirdn(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const UpfGeom &g,
                   const float *taps, bool vec, int64_t m0, int64_t nout, void *out);

// polyphase filter-bank channelizer (k_pfb.hip): frames m < nframes of every row, frame m = the L = P M samples from first + m hop on
// (zero outside the row) folded to M under the taps and transformed; rp partitions the frames of ONE row, the grid is rp.blocks x batch
// workgroups in one dimension.  out_kind 0: out = complex64 [batch][nframes][nb], nb = M (complex rows) or M/2 + 1 (real rows);
// out_kind 1: partial[batch][rp.groups][M] floats, summed by launch_pfb_finish into float64 out[batch][nb] = scale * sum.
// The taps stay in registers when every frame sees the same rotation, P <= SP_PFB_TREG_P and M <= SP_PFB_TREG_MAXM (SP_PFB_TREG=0: never).
#define SP_PFB_MAXP 32
#define SP_PFB_TREG_P 4
#define SP_PFB_TREG_MAXM 4096
#define SP_PFB_TREG_DEFAULT 1
bool pfb_treg_wanted(int M, int P, int hop, int phase_ref);
int launch_pfb(LaunchCtx c, const void *x, bool cplx, int64_t x_ld, int64_t nsig, int64_t batch, const float *taps, int P, int hop,
               int64_t first, int64_t nframes, int phase_ref, int r0, const Xf &xf, const RunPart &rp, int out_kind, void *out,
               float *partial);
int launch_pfb_finish(LaunchCtx c, const float *partial, int64_t G, int M, int nb, int64_t batch, double scale, double *out);

// polyphase synthesis bank (k_pfb_synth.hip): X = complex64 [batch][nframes][nb] frame-major, nb = M (cplx) or M/2 + 1; taps = the
// scaled synthesis prototype [P M] on the device; y = [batch][nout] cf (cplx) or float.  fused: runs of fpg frames, each preceded by
// `halo` frames that are only accumulated, overlap-added in an LDS ring of P M accumulators per group (v unused).  Not fused: fpg frames
// per group, the inverse transforms go to v[batch][nframes][M] (cf, or float when !cplx; halo and y unused), and
// launch_pfb_synth_gather sums every output sample from them.
// pfb_synth_groups: the groups of a workgroup that get a ring in the fused form (<= FPW; 0: not even one ring fits) and the LDS bytes
// that takes (host only).
int pfb_synth_groups(int M, int ntaps, bool cplx, size_t *lds_out);
int launch_pfb_synth(LaunchCtx c, const cf *X, bool cplx, int64_t batch, int64_t nframes, const float *taps, int P, int hop,
                     int64_t first, int phase_ref, int r0, const Xf &xf, int64_t fpg, int halo, bool fused, int64_t nout, void *y,
                     void *v);
int launch_pfb_synth_gather(LaunchCtx c, const void *v, bool cplx, int64_t batch, int64_t nframes, const float *taps, int ntaps, int M,
                            int hop, int64_t first, int phase_ref, int r0, int64_t nout, void *y);

// short-time cross-correlation (k_xcorr_frames.hip): frame g of x and y (nw samples at g hop) -> the lags -maxlag .. maxlag of the
// L-point circular correlation, L a power of two in 32 .. 8192, nw + maxlag <= L.  win (null: boxcar) and weight (null: ones, else
// L floats in FFT order) are device tables; segmean: every window's own mean is removed; coeff: / sqrt(sum |a|^2 sum |b|^2);
// beta > 0: the regularised PHAT.  Any of frames ([nframes][2 maxlag + 1] float or cf), partial ([rp.groups][L] float or cf, summed by
// launch_xcorr_frames_finish into avg = float64 [2 maxlag + 1] (x 2 for cf) / nframes) and peak ([nframes][2]) may be null.
struct XcfArgs {
    const void *x, *y;
    const float *win, *weight;
    int nw, hop, maxlag, segmean, coeff;
    float beta;
    int64_t nframes;
};
int launch_xcorr_frames(LaunchCtx c, const XcfArgs &a, bool cplx, int L, const cf *tw, const RunPart &rp, void *frames, void *partial,
                        float *peak);
int launch_xcorr_frames_finish(LaunchCtx c, const void *partial, bool cplx, int64_t G, int L, int maxlag, int64_t nframes, double *avg);

// two-point wavenumber-frequency spectrum S(k, f) (k_skf.hip): frame g of x and y (L samples at g hop, L a power of two in 32 .. 4096)
// -> theta = arg(X conj Y) and p = (|X|^2 + |Y|^2) / 2 (cross: |X| |Y|) at the nb bins from b0 on (modulo L for complex records),
// histogrammed over nk equal phase bins.  A workgroup owns a run of fpr consecutive frames and one frequency tile of the band; its
// histogram lives in LDS behind the transform images, row j (one phase bin) `stride` floats long.  Grid: runs x tiles.
// partial: float [runs][nk][nb] (phase-major like the tile, so that the tile leaves LDS and enters memory at unit stride), summed by
// launch_skf_finish in float64 in ascending run order into s_out[nb][nk] * scale / nframes.
#define SP_SKF_MAX_L 4096
#define SP_SKF_MAX_NK 1024
struct SkfPlan {
    int tiles, tile_bins, stride;       // frequency tiles, bins of a tile (the last may hold fewer), floats per histogram row
    size_t lds_bytes;                   // transform images + histogram tile
};
// LDS of the transform images of one workgroup: max(1, 4096 / L) groups of L + 16 complex each, twice for complex records
inline size_t skf_image_bytes(bool cplx, int L) { return xf_image_bytes(L, cplx ? 2 : 1); }
// cells_cap > 0: at most that many cells (nk x bins) per tile.  Rows are padded to a multiple of 32 floats (the bank of an LDS add is
// its dword address mod 32, so the bank is the lane's bin whatever the phase bin); where not even 32 bins fit, 16, 8 .. 1.
inline SkfPlan skf_plan_of(bool cplx, int L, int nb, int nk, int cells_cap) {
    const int64_t room = (int64_t)(SP_LDS_MAX - skf_image_bytes(cplx, L)) / 4 / nk;      // floats per row
    int gran = 32;
    while (gran > 1 && room < gran) gran /= 2;
    int tb = (int)(room / gran) * gran;
    if (tb > nb) tb = nb;
    if (cells_cap > 0 && tb > cells_cap / nk) tb = cells_cap / nk < 1 ? 1 : cells_cap / nk;
    SkfPlan p;
    p.tile_bins = tb;
    p.tiles = (nb + tb - 1) / tb;
    p.stride = (tb + gran - 1) / gran * gran;
    p.lds_bytes = skf_image_bytes(cplx, L) + sizeof(float) * (size_t)nk * (size_t)p.stride;
    return p;
}
struct SkfArgs {
    const void *x, *y;
    const float *win;
    int hop, segmean, cross, b0, nb, nk, tile_bins, stride;
    int64_t nframes, fpr;
};
int launch_skf(LaunchCtx c, const SkfArgs &a, bool cplx, int L, const cf *tw, int64_t runs, const SkfPlan &pl, float *partial);
int launch_skf_finish(LaunchCtx c, const float *partial, int64_t runs, int nb, int nk, double mult, double *s_out);

// time-resolved Welch spectra (k_welch_blocks.hip): blocks of navg frames, step frames apart.  A run is q consecutive frames summed
// once: q = navg and run r = block r = the frames from r step on when step >= navg (final: the kernel writes the outputs); else
// q = gcd(navg, step), the runs tile the frames, and launch_block_sum forms block b from the navg / q runs from b step / q on.
// A workgroup owns welch_blocks_teams(L) x rpt consecutive runs (teams: 256 / L below 256 points, else 1).
struct WelchBlocksArgs {
    const void *x, *y;                  // y null: the PSD alone; else pairs rows, y_ld samples apart
    const float *win;                   // device table or null (boxcar)
    int hop, segmean, q, rpt, planes;   // planes of the partials: 4 with y, else 1
    int64_t y_ld, nframes, runs, rstride;      // rstride: frames from one run's first frame to the next one's
    float mult, mult2;                  // final form: s / navg, and the same doubled (real records, bins 1 .. L/2 - 1) or not
    float *partial;                     // [pairs][runs][planes][nb], or null: the final form ->
    float *pxx, *pyy;                   // [runs][nb], [pairs][runs][nb]
    cf *pxy;                            // [pairs][runs][nb]
};
struct WelchBlocksPlan {
    int64_t nblocks, runs, rstride, wgs;
    int nb, q, rpt, final_form, adv, nsum;      // block b = runs b adv .. b adv + nsum - 1
    size_t lds_bytes, scratch_bytes;
};
inline int welch_blocks_teams(int L) { return L < 256 ? 256 / L : 1; }
// a complex pair at 8192 points: the bins are split over two workgroups, each transforms the frames (registers; k_welch_blocks.hip)
constexpr int welch_blocks_bin_split(bool cplx, bool pair, int L) { return cplx && pair && L >= 8192 ? 2 : 1; }
// the transform images of a workgroup: two per group with y (X is parked while Y is made)
inline size_t welch_blocks_lds_bytes(bool pair, int L) { return xf_image_bytes(L, pair ? 2 : 1); }
// pairs = max(nch, 1); have_y = nch >= 1.  rpt: a team should run about four rounds of its groups, as long as that leaves the grid
// about four workgroups per CU
inline WelchBlocksPlan welch_blocks_plan_of(bool cplx, int L, int64_t nframes, int navg, int step, int nch, int ncu) {
    WelchBlocksPlan p;
    p.nb = cplx ? L : L / 2 + 1;
    p.nblocks = (nframes - navg) / step + 1;
    p.final_form = step >= navg ? 1 : 0;
    if (p.final_form) {
        p.q = navg;
        p.runs = p.nblocks;
        p.rstride = step;
        p.adv = p.nsum = 1;
    } else {
        int g = navg, h = step;
        while (h) {
            const int r = g % h;
            g = h;
            h = r;
        }
        p.q = g;
        p.runs = ((p.nblocks - 1) * step + navg) / g;
        p.rstride = g;
        p.adv = step / g;
        p.nsum = navg / g;
    }
    const int teams = welch_blocks_teams(L), gpt = fpw_of(L) / teams, pairs = nch > 1 ? nch : 1;
    int64_t rpt = ((int64_t)4 * gpt + p.q - 1) / p.q;
    const int64_t room = p.runs * pairs / ((int64_t)teams * 4 * ncu);
    if (rpt > room) rpt = room;
    if (rpt < 1) rpt = 1;
    p.rpt = (int)rpt;
    p.wgs = (p.runs + teams * rpt - 1) / (teams * rpt);
    p.lds_bytes = welch_blocks_lds_bytes(nch >= 1, L);
    p.scratch_bytes = p.final_form ? 0 : sizeof(float) * (size_t)pairs * (size_t)p.runs * (nch >= 1 ? 4 : 1) * (size_t)p.nb;
    return p;
}
int launch_welch_blocks(LaunchCtx c, const WelchBlocksArgs &a, bool cplx, int L, const cf *tw, int pairs, int64_t wgs);
int launch_block_sum(LaunchCtx c, const float *partial, int64_t runs, int planes, int nb, int64_t nblocks, int adv, int nsum, bool dbl,
                     int L, double mult, int pairs, float *pxx, float *pyy, cf *pxy);

// batched Hermitian eigensolver (k_eigh.hip): a[batch][n][n] complex128, lower triangle -> w[batch][n] descending, the nvec leading
// vectors v[batch][n][nvec] and the sweeps used; parallel cyclic Jacobi, one matrix per workgroup, A (and V, if nvec > 0) in LDS at the
// padded order NP.  The grid walks the batch: at most workgroups-per-CU x CUs workgroups.
#define SP_EIGH_MAX_N 64
struct EighPlan {
    int NP, wg, wg_per_cu;
    size_t lds_bytes;
    int64_t grid;
};
size_t eigh_lds_bytes(int NP, bool vec);       // sizeof the kernel's LDS image
inline int eigh_np_of(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }
inline int eigh_wg_of(int NP) { return NP * NP / 4 < 64 ? 64 : NP * NP / 4; }
// workgroups per CU: what the LDS, the 2048 threads of a CU and the registers allow, 16 at the most.  The kernels take 78 .. 92 VGPRs,
// which is 5 waves per SIMD, 20 per CU (profiles/eigh_kernel_resources.txt): one workgroup of 1024 threads, five of 256.
// grid_cap > 0 limits the grid (test hook)
#define SP_EIGH_WAVES_PER_CU 20
inline EighPlan eigh_plan_of(int n, bool vec, int64_t batch, int ncu, int grid_cap) {
    EighPlan p;
    p.NP = eigh_np_of(n);
    p.wg = eigh_wg_of(p.NP);
    p.lds_bytes = eigh_lds_bytes(p.NP, vec);
    int per = (int)(SP_LDS_MAX / p.lds_bytes);
    if (per > 2048 / p.wg) per = 2048 / p.wg;
    if (per > SP_EIGH_WAVES_PER_CU * 64 / p.wg) per = SP_EIGH_WAVES_PER_CU * 64 / p.wg;
    if (per > 16) per = 16;
    p.wg_per_cu = per;
    p.grid = (int64_t)per * ncu;
    if (grid_cap > 0 && p.grid > grid_cap) p.grid = grid_cap;
    if (p.grid > batch) p.grid = batch;
    return p;
}
int launch_eigh(LaunchCtx c, const double *a, int n, int64_t batch, int nvec, int max_sweeps, double *w, double *v, int32_t *sweeps,
                const EighPlan &pl);

// continuous wavelet transform by overlap-save (k_cwt.hip): frame g = the L samples from g hop - M on (zero outside the row), hop = L - 2 M,
// every scale's filter H_s[k] = exp(c_s + p ln u - a d^2 - b d), u = k step_s, d = u - u0, on the bins 0 < k <= L / 2; sc[s] = (step_s, c_s)
// is a device table, c_s includes the 1 / L of the inverse transform.  Any of the outputs may be null: W [rows][S][nsig], gpart
// [rows][S][nframes] (summed by launch_cwt_gws_finish into float64 gws[rows][S]), recon [rows][nsig] = sum_s wr[s] W, bandpow
// [rows][nsig] = sum_s wb[s] |W|^2 (wr, wb: device tables [S]; with either the chunk must be the whole scale set).
#define SP_CWT_MIN_L 256
#define SP_CWT_MAX_L 8192
struct CwtArgs {
    const void *x;
    int cplx;
    int64_t nsig, x_ld, nframes;
    const float *sc;
    float p, a, b, u0;
    int S, chunk, M, hop;
    const float *wr, *wb;
    cf *W;
    float *gpart;
    cf *recon;
    float *bandpow;
};
struct CwtPlan {
    int hop, chunk, nchunks;
    int64_t frames, blocks_x, grid;
    size_t scratch_bytes;
};
// whole: an output needs every scale of a frame in one workgroup (recon, bandpow).  Otherwise the scales are cut into as many chunks as
// bring the grid to about four workgroups per CU (every chunk repeats the forward transform); chunk_force > 0 sets the chunk (test hook)
inline CwtPlan cwt_plan_of(int L, int M, int64_t nsig, int S, int64_t rows, bool whole, bool gws, int ncu, int chunk_force) {
    CwtPlan p;
    p.hop = L - 2 * M;
    p.frames = (nsig + p.hop - 1) / p.hop;
    const int fpw = fpw_of(L);
    p.blocks_x = (p.frames + fpw - 1) / fpw;
    int64_t nch = 1;
    if (!whole) {
        const int64_t wg = p.blocks_x * (rows > 0 ? rows : 1);
        nch = ((int64_t)4 * ncu + wg - 1) / wg;
        if (nch > S) nch = S;
        if (nch < 1) nch = 1;
    }
    p.chunk = (int)((S + nch - 1) / nch);
    if (!whole && chunk_force > 0) p.chunk = chunk_force < S ? chunk_force : S;
    p.nchunks = (S + p.chunk - 1) / p.chunk;
    p.grid = p.blocks_x * p.nchunks * rows;
    p.scratch_bytes = gws ? sizeof(float) * (size_t)rows * (size_t)S * (size_t)p.frames : 0;
    return p;
}
int launch_cwt(LaunchCtx c, const CwtArgs &a, int L, const cf *tw, const CwtPlan &pl, int64_t rows);
int launch_cwt_gws_finish(LaunchCtx c, const float *gpart, int64_t rows_x_scales, int64_t nframes, double *gws);
// out[row][n] = sum_s w[s] W[row][s][n] (w: device table)
int launch_icwt(LaunchCtx c, const cf *W, const float *w, int S, int64_t N, int64_t rows, cf *out);

// cross-wavelet spectra and wavelet coherence by overlap-save (k_wct.hip): the frames of k_cwt with the margin M = Mw + Mg, Mw the reach of
// the wavelets and Mg that of the time-smoothing Gaussians, hop = L - 2 M.  Per frame the spectra of x and y are kept (bins 1 .. L / 2:
// in registers below 2048 points, in an LDS stash from there on); per scale Wx and Wy, then either Wxy = Wx conj(Wy) [rows][S][nsig]
// (T null: the cross-wavelet transform, Mg = 0) or the products |Wx|^2 / s', |Wy|^2 / s', Wx conj(Wy) / s' (zero outside the row)
// filtered by exp(-(s' w)^2 / 2) as two complex records (a + i b, c) and stored as T [rows][S][nsig] float4 = (A_t, B_t, Re C_t, Im C_t).
// sc[s] = (step_s, c_s, 1 / s', 0) is a device table, step and c as in CwtArgs.
struct WctArgs {
    const void *x, *y;
    int cplx;
    int64_t nsig, x_ld, y_ld, nframes;
    const float *sc;
    float p, a, b, u0;
    int S, chunk, M, hop;
    float4 *T;
    cf *Wxy;
};
constexpr bool wct_stash(int L) { return L >= 2048; }
// the exchange images and, from 2048 points on, two half spectra per transform group
inline size_t wct_lds_bytes(int L) {
    const int R = 16, T = L / R;
    const size_t img = (size_t)(R * (T + 1) > L ? R * (T + 1) : L);
    return sizeof(cf) * (size_t)fpw_of(L) * (img + (wct_stash(L) ? (size_t)L : 0));
}
int launch_wct_time(LaunchCtx c, const WctArgs &a, int L, const cf *tw, const CwtPlan &pl, int64_t rows);
// every scale row of T summed with its neighbours (taps [ntaps], a device table: row s - ntaps / 2 + j takes taps[ntaps - 1 - j], rows
// outside the set count as zero, ascending row order; up to 16 taps a thread walks the rows of its sample with the window in registers
// and reads T once, beyond that the rows are re-read through the caches), then R2 = |C|^2 / (A B) and phase = atan2(Im C, Re C), 0 where A B == 0: float32
// [rows][S][nsig] each; A, B (float32) and C (complex64) of the same shape on request (all three or none)
int launch_wct_scale(LaunchCtx c, const float4 *T, const float *taps, int ntaps, int S, int64_t N, int64_t rows, float *R2, float *phase,
                     float *A, float *B, cf *C);

// synchrosqueezed STFT and reassignment fields (k_ssq.hip): frame g of a row = the L samples from first + g hop on (zero outside the
// row), L a power of two in 32 .. 8192, under the windows h, dh and (for IF / GD) th, device tables of L floats.  A workgroup owns a
// run of fpr consecutive frames of one row; grid: runs x rows.  Scatter form (out null): any of T complex64, P, IF, GD float32
// [rows][nframes][nb], the band of nb bins from b0 on (modulo L for complex rows).  Band form (out set): out[rows][nbands][nframes],
// edges (lo, hi) per band by value or, per_frame, a device table float32 [nbands][nframes][2].
// LDS of a workgroup: an image of L + 16 complex per transform and group, and behind them the groups' 64-bit accumulators: 16 bytes a
// bin for T, 8 for P.
#define SP_SSQ_MAX_L 8192
#define SP_SSQ_MAX_BANDS 8
struct SsqEdges {
    float v[2 * SP_SSQ_MAX_BANDS];      // (lo, hi) per band, constant over the frames: passed by value, no table
};
struct SsqArgs {
    const void *x;
    int64_t x_ld, nsig, first, nframes, fpr;
    const float *h, *dh, *th;
    int hop, segmean;
    float gamma, rel;
    int b0, nb;
    cf *T;
    float *P, *IF, *GD;
    int nbands, per_frame;
    const float *edges;                 // per_frame: [nbands][nframes][2], else edges_c
    SsqEdges edges_c;
    float scale;
    cf *out;
};
inline int ssq_transforms(bool cplx, bool fields) { return (cplx ? 2 : 1) + (fields ? 1 : 0); }
inline size_t ssq_lds_bytes(bool cplx, int L, int nb, bool wantT, bool wantP, bool fields) {
    return xf_image_bytes(L, ssq_transforms(cplx, fields)) + (size_t)fpw_of(L) * (size_t)nb * ((wantT ? 16 : 0) + (wantP ? 8 : 0));
}
// frames per run: about four workgroups per CU over runs x rows, whole rounds of the workgroup's groups; forced > 0: that many
inline int64_t ssq_fpr(int L, int64_t nframes, int64_t rows, int ncu, int forced) {
    if (forced > 0) return forced;
    const int fpw = fpw_of(L);
    int64_t want = (int64_t)ncu * 4 / (rows > 0 ? rows : 1);
    if (want < 1) want = 1;
    const int64_t f = ((nframes + want - 1) / want + fpw - 1) / fpw * fpw;
    return f < fpw ? fpw : f;
}
int launch_ssq(LaunchCtx c, const SsqArgs &a, bool cplx, int L, const cf *tw, int64_t runs, int64_t rows, size_t lds_bytes);
// out[row][b][g] = scale * sum over lo <= m < hi of w_m T[row][g][j], m = (b0 + j) mod n, w = 1/2 at the bins 0 and n / 2 when `half`
int launch_ssq_sum(LaunchCtx c, const cf *T, int64_t nframes, int nb, int n, int b0, int nbands, int per_frame, const float *edges,
                   const SsqEdges &ec, int half, float scale, int64_t rows, cf *out);

// smoothed pseudo Wigner-Ville distribution (k_wvd.hip): column j of a row sits at n_j = first + j hop;
//   K[j][tau] = h[tau] sum_mu g[mu] z[n_j + mu + tau] conj(y[n_j + mu - tau]),   W[j][k] = scale FFT_L(K[j][tau mod L])[k]
// h = device table of 2 Lh + 1 taps, g of 2 Lg + 1, both indexed from -L.  A workgroup owns a run of cpr consecutive columns of one row
// and stages the samples of z they touch in LDS behind its transform images.  Auto (y null): the columns 2p and 2p + 1 of a ROW share
// one transform whatever the runs are -- a run that starts or ends inside a pair forms the pair and stores its own column -- so the
// staged columns are cpr rounded up to even; the partner of an odd last column is that column itself.  Cross: one transform per
// column, y is read through the caches.  W: float [rows][ntimes][nb] (auto) or cf, the nb bins from b0 on modulo L.
#define SP_WVD_MAX_L 8192
#define SP_WVD_MAX_NG 255
#define SP_WVD_MAX_SPAN ((int64_t)1 << 40)
struct WvdArgs {
    const cf *x, *y;
    int64_t x_ld, nsig, first, ntimes, cpr, hop;
    const float *h, *g;
    int Lh, Lg, b0, nb;
    float scale;
    void *W;
};
// columns a run stages
inline int64_t wvd_staged_cols(bool cross, int64_t cpr, int64_t ntimes) {
    const int64_t nc = cross ? cpr : cpr + (cpr & 1);
    return nc < ntimes ? nc : (ntimes > 1 ? ntimes : 1);
}
inline size_t wvd_image_bytes(int L) { return xf_image_bytes(L); }
// images + 8 bytes per staged sample: (staged columns - 1) hop + 2 (Lh + Lg) + 1 of them
inline size_t wvd_lds_bytes(bool cross, int L, int nh, int ng, int64_t hop, int64_t cpr, int64_t ntimes) {
    const int64_t nc = wvd_staged_cols(cross, cpr, ntimes);
    if (nc > 1 && hop > SP_WVD_MAX_SPAN / (nc - 1)) return (size_t)-1 / 2;
    return wvd_image_bytes(L) + 8 * (size_t)((nc - 1) * hop + (nh - 1) + (ng - 1) + 1);
}
// columns per run: about four workgroups per CU over runs x rows in whole rounds of the workgroup's groups, cut down to what the LDS
// holds (auto: kept even); forced > 0: that many.  Never more than the row has.
inline int64_t wvd_cpr(bool cross, int L, int nh, int ng, int64_t hop, int64_t ntimes, int64_t rows, int ncu, int forced) {
    if (ntimes < 1) return 1;
    int64_t c = forced;
    if (forced <= 0) {
        const int per = fpw_of(L) * (cross ? 1 : 2);
        int64_t want = (int64_t)ncu * 4 / (rows > 0 ? rows : 1);
        if (want < 1) want = 1;
        c = ((ntimes + want - 1) / want + per - 1) / per * per;
        const int64_t room = (int64_t)((SP_LDS_MAX - wvd_image_bytes(L)) / 8) - ((nh - 1) + (ng - 1) + 1);
        if (room >= 0 && c > room / hop + 1) {
            c = room / hop + 1;
            if (!cross && c > 1) c &= ~(int64_t)1;
        }
    }
    return c < ntimes ? c : ntimes;
}
inline int64_t wvd_transforms_per_run(bool cross, int64_t cpr) { return cross ? cpr : (cpr + 1) / 2; }
int launch_wvd(LaunchCtx c, const WvdArgs &a, int L, const cf *tw, int64_t runs, int64_t rows, size_t lds_bytes);

// spectral correlation by the averaged cyclic periodogram (k_cyclic.hip): for every nu_h of nuh[A] (nu / 2 in units of 2^-64 turn) the
// frames g < nframes of every row (n = L samples from g hop on, absolute index first + g hop + j) under win[j] e(-+nu_h j), transformed
// and summed over the frames of a group: partial[rows][A][groups][planes][L], planes 3 (mirror: |U|^2, Re, Im of sum p2 U[k] U[n - k])
// or 4 (|U+|^2, |U-|^2, Re, Im of sum p2 U+ conj(U-)).  mirror: y = x and x' = conj(x) (or x real): one transform per (frame, alpha);
// else two.  means: device float [rows][4] = mean of x (re, im), mean of y.  Grid: blocks x A workgroups x rows.
#define SP_CYC_MAX_L 8192
#define SP_CYC_MAX_A 65535
#define SP_CYC_PARTIAL_BYTES ((size_t)256 << 20)
// where a group keeps its rotated window: 0 registers; 1 (one transform, from 2048 points on) an LDS image; 2 (two transforms, from 512
// points on) a slot of L complex per (row, alpha, group) in memory, gtab.  Images of L + 16 complex per transform group: the
// exchange image, the window's (place 1), and in the two-transform form the parked Z-.
constexpr int cyc_tab_place(int L, bool mirror) { return mirror ? (L < 2048 ? 0 : 1) : (L < 512 ? 0 : 2); }
constexpr size_t cyc_lds_bytes(int L, bool mirror) {
    return xf_image_bytes(L, 1 + (cyc_tab_place(L, mirror) == 1 ? 1 : 0) + (mirror ? 0 : 1));
}
struct CycArgs {
    const void *x, *y;
    int64_t x_ld, first, hop, nframes, fpg, groups, blocks;
    const float *win;
    const uint64_t *nuh;
    const float *means;
    int A, conj;
    float *partial;
    cf *gtab;           // place 2: [rows][A][groups][L]
};
struct CycPlan {
    int64_t fpg, groups, used, blocks, apass, passes;
    int planes, xforms;
    size_t lds_bytes, cell_floats;      // cell_floats: scratch floats per (row, alpha, group): the partial planes and gtab's slot
};
// groups: (alpha, group) workgroups number about four per CU -- a scan of many alpha fills the device by itself and gets one block;
// alpha per pass: what keeps the partials of a pass within SP_CYC_PARTIAL_BYTES, at least one (one alpha of every row is never cut);
// chunk_force > 0 caps it, fpg_force > 0 sets the frames per group (test hooks)
inline CycPlan cyc_plan_of(int L, int64_t nframes, int A, int64_t rows, bool mirror, int ncu, int chunk_force, int fpg_force = 0) {
    CycPlan p;
    const int fpw = fpw_of(L);
    const int64_t cells = (int64_t)A * (rows > 0 ? rows : 1);
    int64_t want = ((int64_t)4 * ncu + cells - 1) / cells;
    if (want < 1) want = 1;
    int64_t f = (nframes + want * fpw - 1) / (want * fpw);
    if (f < 1) f = 1;
    if (fpg_force > 0) f = fpg_force;
    p.fpg = f;
    p.used = nframes > 0 ? (nframes + f - 1) / f : 1;
    p.blocks = (p.used + fpw - 1) / fpw;
    p.groups = p.blocks * fpw;
    p.planes = mirror ? 3 : 4;
    p.xforms = mirror ? 1 : 2;
    p.lds_bytes = cyc_lds_bytes(L, mirror);
    p.cell_floats = (size_t)(p.planes + (cyc_tab_place(L, mirror) == 2 ? 2 : 0)) * (size_t)L;
    const size_t per = sizeof(float) * (size_t)(rows > 0 ? rows : 1) * (size_t)p.groups * p.cell_floats;
    int64_t ap = (int64_t)(SP_CYC_PARTIAL_BYTES / per);
    if (ap < 1) ap = 1;
    if (ap > A) ap = A;
    if (chunk_force > 0 && chunk_force < ap) ap = chunk_force;
    p.apass = ap;
    p.passes = (A + ap - 1) / ap;
    return p;
}
int launch_cyclic(LaunchCtx c, const CycArgs &a, bool mirror, bool cplx, int L, const cf *tw, int64_t rows);
// out[(row a_total + a_off + ai) nb + jb] = scale * the float64 sum over the `used` groups, bin (b0 + jb) mod L; Pm of the mirrored
// form is Pp at the mirrored bin.  Any of S, Pp, Pm may be null.
int launch_cyclic_finish(LaunchCtx c, const float *partial, int64_t groups, int64_t used, int L, bool mirror, int A, int a_off,
                         int a_total, int b0, int nb, double scale, int64_t rows, cf *S, float *Pp, float *Pm);

// Lomb-Scargle sums of an unevenly sampled record (k_lomb.hip).  With e(p) = exp(2 pi i p), phi = f (t - t_ref), the normalised
// weights wn = w / wnorm and d_r = y_r - m_r, per frequency
//   A1 = sum w32 e(phi),  A2 = sum w32 e(2 phi),  B_r = sum wy32_r e(phi);    w32 = float32(wn), wy32_r = float32(wn d_r)
// and per row the totals W = sum w32, Y'_r = sum wy32_r, YY'_r = sum wy32_r d_r (float64 sums of the float32 values).
// The prepared record: head[npad] = (t - t_ref as float64, w32, 0) and wy[groups][npad][RP] floats, RP = the rows of a group padded
// to 4 or 8; samples from N on and rows from batch on are zeros, npad = N rounded up to 4, plus LOMB_SUB, so that no piece of a run
// is loaded from outside the arrays.
#define LOMB_SUB 256                      // samples of a sub-run: float32 sums inside it, float64 across; also the staged piece
#define LOMB_WG 256                       // frequencies of a workgroup: one per lane
#define LOMB_MAX_M (1 << 24)
#define LOMB_PARTIAL_BYTES ((size_t)256 << 20)
#define LOMB_PREP_BLOCKS 64               // at most so many blocks along the samples in the two prep stages
#define LOMB_PREP_COLS 32768              // at most so many columns of the prepared record in one launch of k_lomb_prep
struct LombHead {
    double t;
    float w, pad;
};
constexpr int lomb_rp(int R) { return R == 0 ? 0 : (R <= 4 ? 4 : 8); }
constexpr int lomb_nv(int R) { return 4 + 2 * R; }
inline int64_t lomb_npad(int64_t N) { return (N + 3) / 4 * 4 + LOMB_SUB; }
struct LombPlan {
    int R, RP, nv;                        // rows of a group (0: no rows, the window sums alone), their padded count, sums per frequency
    int64_t groups, gpl;                  // row groups; groups per launch
    int64_t fpass, passes;                // frequencies per pass, passes over the list
    int64_t split, run_len;               // sample runs and the samples of one (a multiple of 4)
    int64_t workgroups;                   // over all passes and launches
    int64_t prep_blocks, prep_len;        // the prep stages' blocks along the samples and the samples of one
};
// split: (tile, group) workgroups number about four per CU, a run is no shorter than four sub-runs; frequencies per pass: what keeps
// the partials [groups of a launch][split][nv][fpass] of float64 within LOMB_PARTIAL_BYTES, whole tiles, at least one; where even
// one tile of all groups does not fit, the groups are dealt to several launches.  freqs_force > 0 caps the frequencies per pass
// at any figure, split_force > 0 sets the runs (test hooks).
inline LombPlan lomb_plan_of(int64_t N, int64_t M, int64_t batch, int ncu, int freqs_force, int split_force) {
    LombPlan p;
    p.R = batch <= 0 ? 0 : (batch == 1 ? 1 : (batch <= 4 ? 4 : 8));
    p.RP = lomb_rp(p.R);
    p.nv = lomb_nv(p.R);
    p.groups = p.R ? (batch + p.R - 1) / p.R : 1;
    const int64_t tiles_all = (M + LOMB_WG - 1) / LOMB_WG;
    int64_t split = ((int64_t)4 * ncu + tiles_all * p.groups - 1) / (tiles_all * p.groups);
    const int64_t most = (N + 4 * LOMB_SUB - 1) / (4 * LOMB_SUB);
    if (split > most) split = most;
    if (split_force > 0) split = split_force;
    if (split < 1) split = 1;
    if (split > N) split = N;
    p.run_len = ((N + split - 1) / split + 3) / 4 * 4;
    p.split = (N + p.run_len - 1) / p.run_len;
    const size_t tile_bytes = sizeof(double) * (size_t)p.split * (size_t)p.nv * LOMB_WG;       // one tile of one group
    int64_t tiles_fit = (int64_t)(LOMB_PARTIAL_BYTES / tile_bytes);
    if (tiles_fit < 1) tiles_fit = 1;
    p.gpl = tiles_fit < p.groups ? tiles_fit : p.groups;
    int64_t tp = tiles_fit / p.gpl;
    if (tp < 1) tp = 1;
    if (tp > tiles_all) tp = tiles_all;
    p.fpass = tp * LOMB_WG < M ? tp * LOMB_WG : M;
    if (freqs_force > 0 && freqs_force < p.fpass) p.fpass = freqs_force;
    p.passes = (M + p.fpass - 1) / p.fpass;
    int64_t tiles = 0;
    for (int64_t m0 = 0; m0 < M; m0 += p.fpass) tiles += ((M - m0 < p.fpass ? M - m0 : p.fpass) + LOMB_WG - 1) / LOMB_WG;
    p.workgroups = tiles * p.split * p.groups;
    p.prep_blocks = (N + 4095) / 4096;
    if (p.prep_blocks > LOMB_PREP_BLOCKS) p.prep_blocks = LOMB_PREP_BLOCKS;
    p.prep_len = (lomb_npad(N) + p.prep_blocks - 1) / p.prep_blocks;
    return p;
}
struct LombPrepArgs {
    const double *t, *w;                  // w null: equal weights
    const float *y;
    int64_t y_ld, N, npad, batch, rows_padded;      // rows_padded = groups * RP
    int R, RP;                            // rows of a group and their padded count
    double t_ref, wnorm;                  // wnorm <= 0: the weights' own sum
    const double *mean;                   // [batch] or null
    int64_t blocks, len;                  // blocks along the samples, samples of one
    double *wpart;                        // [blocks]: the blocks' sums of w
    LombHead *head;
    float *wy;
    double *tpart;                        // [1 + 2 batch][blocks]: the blocks' sums of w32; wy32_r; wy32_r d_r
    double *totals;                       // [1 + 2 batch]: W, then (Y'_r, YY'_r) row by row
    int *status;                          // [4]: a non-finite t; a weight that is negative or not finite; a weight sum that is not
};                                        //      positive and finite; a non-finite y
struct LombSumArgs {
    const LombHead *head;
    const float *wy;                      // of the launch's first group
    const double *f;                      // the pass's frequencies
    int64_t npad, N4, run_len, split;     // N4: N rounded up to 4
    int fcount;                           // frequencies of the pass
    double *partial;                      // [groups of the launch][split][nv][fcount]
};
int launch_lomb_prep(LaunchCtx c, const LombPrepArgs &a);
int launch_lomb_sums(LaunchCtx c, const LombSumArgs &a, int R, int64_t groups);
// the runs added in ascending order: common[j][4] (from the launch's first group, when common is given) and
// rows[(g0 R + r) rows_ld + j][2] for the rows below batch
int launch_lomb_reduce(LaunchCtx c, const double *partial, int R, int64_t groups, int64_t split, int fcount, int64_t g0, int64_t batch,
                       double *common, double *rows, int64_t rows_ld);
// P[r][j] of fcount frequencies from their sums (scipy.signal.lombscargle's body in float64): float32, or complex64 for normalize 2
int launch_lomb_finish(LaunchCtx c, const double *common, const double *rows, int64_t rows_ld, const double *totals, const double *mean,
                       const double *f, int fcount, int64_t batch, int64_t N, double t_ref, int floating_mean, int normalize, void *P,
                       int64_t p_ld);

// wavelet bispectrum and bicoherence (k_wbic.hip): the contraction over time of wavelet transforms in the layout k_cwt writes, X, Y, Z
// [S][ld] complex64, row i the frequency (k_lo + i) df.  A group is a run of at most WBIC_GROUP consecutive samples of one cell (a
// block, or the `step` samples overlapping blocks share); `start` is the absolute sample index, the column of X, Y, Z is start - shift.
//   part[(tile * ngroups + g)][3][64 * 64]  fp32 sums over the group of Re, Im of X[i] Y[j] conj(Z[i + j + k_lo]) and of |X[i] Y[j]|^2
//   ppart[g][S]                             float64 sums over the group of |Z[m]|^2
// launch_wbic_cells adds the groups gA .. gB - 1 (the ones the launches above covered) in ascending order into the float64 sums of
// their cells, acc[cell][tile][3][4096] and pcell[cell][S] (zeroed by the caller before the first pass); gfirst[c] = the first group of
// cell c, gfirst[ncells] = the number of groups.  launch_wbic_finish forms block b from the cells b .. b + cpb - 1:
// B = sum / T (complex128), b2 = |B|^2 / (D P[m]) (0 where D P = 0), NaN where m = i + j + k_lo >= S, P[b][m]; sym: only tiles tj <= ti
// are held and (i, j) with j > i reads (j, i).  No atomics, every order fixed.
#define WBIC_TILE 64
#define WBIC_GROUP 2048
#define WBIC_PART (3 * WBIC_TILE * WBIC_TILE)       // floats per (tile, group), float64 sums per (cell, tile)
#define WBIC_MAX_S 512
#define WBIC_MAX_PASS_GROUPS 32768
struct WbicGroup {
    int64_t start;
    int cell, len;
};
int launch_wbic_tile(LaunchCtx c, const cf *X, const cf *Y, const cf *Z, int S, int k_lo, int64_t ld, int64_t shift, const WbicGroup *groups,
                     int ngroups, const int2 *tiles, int ntiles, float *part);
int launch_wbic_pz(LaunchCtx c, const cf *Z, int S, int64_t ld, int64_t shift, const WbicGroup *groups, int ngroups, double *ppart);
int launch_wbic_cells(LaunchCtx c, const float *part, const double *ppart, const int *gfirst, int64_t cell0, int64_t ncells, int64_t gA,
                      int64_t gB, int ntiles, int S, double *acc, double *pcell);
int launch_wbic_finish(LaunchCtx c, const double *acc, const double *pcell, const int *tmap, int ntd, int ntiles, int S, int k_lo, int sym,
                       int64_t nblocks, int64_t cpb, int64_t T, void *B, double *b2, double *P);

// FFT accumulation method (k_fam.hip): Y, X [np][ld] complex64 are the frames of a pass bin-major, as the STFT kernel and a transposition
// leave them (frame-referenced); nb blocks of P frames from column 0 on.  pairs[npairs] = (k, l): row k of Y against row l of X.  The
// pair kernel sums the blocks of the pass in float32 and the passes in float64 through acc[npairs][2Q][2] (`first`: nothing to add;
// `last`: S = scale sum, complex64 [npairs][2Q]; a call of one pass never touches acc).  launch_fam_pw: Pw[k] = scale sum_f g[f mod P]
// |Z[k][f]|^2 over the frames of all passes, float64 throughout, through acc[np].
#define SP_FAM_MAX_P 8192
#define SP_FAM_MAX_PAIRS ((int64_t)1 << 22)
struct FamArgs {
    const cf *Y, *X;
    const float *g;
    const int2 *pairs;
    double *acc;
    cf *S;
    int64_t ld, nb, npairs;
    double scale;
    int twoQ, conj, first, last;
};
int launch_fam(LaunchCtx c, const FamArgs &a, int P, const cf *tw);
int launch_fam_pw(LaunchCtx c, const cf *Z, int np, int64_t ld, int64_t nframes, int P, const float *g, double *acc, bool first, bool last,
                  double scale, float *Pw);

// Type-1 NUFFT and the Lomb-Scargle sums on a uniform frequency grid (k_nufft.hip; the arithmetic: nufft_plan.h).  A pass holds the
// fine grids grid[rows of the pass][nf] complex64 of as many rows as NUFFT_GRID_BYTES take.
#define NUFFT_GRID_BYTES ((size_t)256 << 20)
// ls_periodogram / ls_window with method="auto" take the fast path for a uniform grid of N samples x M frequencies from so many
// (sample, frequency) pairs on.  Measured (tools/nufft_bench.py -> profiles/nufft_bench.txt, the "crossing" lines, N = M = 2^k): with one
// row the direct sums win up to k = 14 (0.27 against 0.34 ms) and lose from k = 15 on (0.66 against 0.34 ms); with eight rows they
// lose from k = 14 on.  2^30 pairs is the first measured point from which the fast path wins at both row counts.
#define LOMB_FAST_MIN_PAIRS ((int64_t)1 << 30)
#define NUFFT_HIST 2048                   // up to so many tiles a workgroup counts its samples per tile in LDS first
#define NUFFT_PREP_SPT 8                  // samples per thread of k_nufft_prep and k_nufft_fill: 2048 per workgroup
inline int nufft_rowmax_blocks(int64_t N) { return (int)(N < 4096 * 64 ? (N + 4095) / 4096 : 64); }
struct NufftRec {                         // a prepared sample: the first cell of its footprint, the offset in it, the centre phase
    int i0;
    float dx, pc, ps;
};
// the strengths of row q at sample j: complex rows c_ld apart, or (c null) the prepared Lomb record: row 0 = head[j].w, row q >= 1 = row
// q - 1 of wy[groups][npad][RP] (R rows to a group), all real
struct NufftSrc {
    const cf *c;
    int64_t c_ld;
    const LombHead *head;
    const float *wy;
    int64_t npad;
    int R, RP;
};
struct NufftPrepArgs {
    const double *t;
    int64_t N, nf, tiles;
    double t_ref;
    int sets;                             // position sets: 1, or 2 for the Lomb sums (phi and 2 phi)
    double q[2], fc[2];                   // per set: the position is frac(q tau), the centre phase frac(fc tau)
    NufftRec *rec;                        // [sets][N]
    unsigned *count;                      // [sets][tiles], zeroed by the caller
    int *status;                          // [2]: a time (or a product with it) that is not finite; set by launch_nufft_rowshift: a strength that is not
};
struct NufftSpreadArgs {
    NufftSrc src;
    int64_t row0;                         // first row of the pass
    int nrows;                            // rows of the pass
    int64_t nf;
    const NufftRec *rec;
    const int64_t *off;                   // [tiles + 1]
    const int *list;
    const int *shift;                     // [rows]
    cf *grid;                             // [nrows][nf]
};
int launch_nufft_prep(LaunchCtx c, const NufftPrepArgs &a);
// part: [rows][nufft_rowmax_blocks(N)] floats of scratch
int launch_nufft_rowshift(LaunchCtx c, const NufftSrc &src, int64_t rows, int64_t N, float *part, int *shift, int *status);
// the counts of one set scanned into off[tiles + 1] (and zeroed), then every sample entered into list (2 N entries at most)
int launch_nufft_bin(LaunchCtx c, const NufftRec *rec, int64_t N, int64_t nf, unsigned *count, int64_t *off, int *list);
int launch_nufft_spread(LaunchCtx c, const NufftSpreadArgs &a);
// row r of the transformed grid -> dst + r * row_ld + m * stride: complex64 elements (f32) or pairs of float64
int launch_nufft_pick(LaunchCtx c, const cf *grid, int64_t nf, int64_t M, int64_t nrows, const NufftQuad &q, bool f32, void *dst,
                      int64_t row_ld, int64_t stride);

// Type-2 NUFFT (k_nufft2.hip): the adjoint of the above over the same prepared samples, tile lists, kernel and fine grids.
// Rows of a row group of k_nufft2_interp: a workgroup stages NUFFT_TILE + NUFFT_W - 1 = 1031 cells per row (held at a pitch of
// NUFFT2_PITCH = 1032, so that every row starts on 16 bytes).  4 rows are 33 KB: well within the 64 KiB a launch gets unasked, four
// workgroups (16 waves) to a CU's 160 KiB, and the 8 kernel values of a sample are shared by 4 rows.  7 rows would fit the 64 KiB and
// leave two workgroups to a CU, too few to hide the latency of the scattered LDS reads and the global stores.
#define NUFFT2_RG 4
#define NUFFT2_PITCH (NUFFT_TILE + NUFFT_W)
struct Nufft2InterpArgs {
    const cf *grid;                       // [nrows][nf], transformed
    int nrows;                            // rows of the pass
    int64_t nf, N;
    const NufftRec *rec;
    const int64_t *off;                   // [tiles + 1]
    const int *list;
    cf *out;                              // row r of the pass at out + r * out_ld, sample j at + j
    int64_t out_ld;
};
// grid[r][(m - M / 2) mod nf] = F[r * F_ld + m] / phihat(m - M / 2), every other cell of grid[nrows][nf] zero: each cell written once
int launch_nufft2_place(LaunchCtx c, const cf *F, int64_t F_ld, int64_t M, int64_t nrows, int64_t nf, const NufftQuad &q, cf *grid);
int launch_nufft2_interp(LaunchCtx c, const Nufft2InterpArgs &a);

// Autoregressive fits and spectra (k_burg.hip; include/spectral_ar.h; the host's arithmetic in ar_plan.h).  Segment s of a pass is frame
// g = (seg0 + s) % nframes of row r = (seg0 + s) / nframes: the n samples from x + r x_ld + first + g hop on.  Model s of the pass is
// written at a + s out_ld (p + 1 coefficients, float64 or complex128), e + s out_ld (p + 1 prediction-error powers) and k + s out_ld
// (p reflection coefficients): the pointers are the pass's own.
// BURG_WAVE_MAX (ar_plan.h) is where the two forms of k_burg meet; profiles/burg_variants.txt has both forms on either side of it.
struct ArArgs {
    const void *x;                        // float32 or complex64 rows
    bool cplx;
    int64_t x_ld, first, hop, nframes, n;
    int p, detrend;                       // detrend: 0 nothing, 1 the segment's own mean, 2 the constant (mre, mim)
    double mre, mim;
    int64_t seg0, nseg;                   // the pass
    void *a;
    double *e;
    void *k;
    int64_t out_ld;
};
// sums[nseg][tiles] (re, im) of the tiles' samples in float64 (nullptr: not wanted); *flag = 1 where a sample is not finite
int launch_ar_scan(LaunchCtx c, const ArArgs &a, int64_t chunk, int64_t tiles, double *sums, int *flag);
// mean[nseg] (re, im): the tiles' sums added in order over n, the given constant, or zero
int launch_ar_mean(LaunchCtx c, const ArArgs &a, int64_t tiles, const double *sums, double *mean);
int launch_burg(LaunchCtx c, const ArArgs &a, int spl, int nw);
// part[nseg][tiles][p + 1] float64 or complex128: sum over the tile's i of x[i] conj(x[i - l]), detrended with mean[seg]
int launch_ar_lags(LaunchCtx c, const ArArgs &a, int64_t chunk, int64_t tiles, const double *mean, void *part);
int launch_levinson(LaunchCtx c, const ArArgs &a, int64_t tiles, const void *part);
// P[model][q] = scale e[model e_ld] / |sum_j a[model a_ld + j] e(-j (start + q step))|^2, q = 0 .. m - 1; float32, or float64 with out64
int launch_ar_psd(LaunchCtx c, const void *a, bool cplx, int64_t a_ld, const double *e, int64_t e_ld, int p, int64_t nmodels, int64_t m,
                  double start, double step, double scale, bool out64, void *P, int64_t P_ld);

// The data covariance matrix, the covariance least-squares fits and the pseudospectrum (k_subspace.hip; include/spectral_sub.h; the host's
// arithmetic in sub_plan.h).  A holds the segments of a pass as for the fits above (its p, a, e, k, out_ld are not looked at here);
// matrix s of the pass is written at C + s C_ld, complex128 [m][m].
struct CovArgs {
    ArArgs A;
    int m, fb;                            // the matrix order; 1: the forward-backward (modified) form
    void *C;
    int64_t C_ld;
};
// part[nseg][tiles][m] float64 or complex128: the tile's share of sum_{t >= m-1} conj(s[t]) s[t - j], detrended with mean[seg]
int launch_cov_row(LaunchCtx c, const CovArgs &k, int64_t chunk, int64_t tiles, const double *mean, void *part);
int launch_cov_fill(LaunchCtx c, const CovArgs &k, int64_t tiles, const double *mean, const void *part);
// a[model out_ld + j], j = 0 .. m - 1 (float64, or complex128 with cplx), e[model], status[model] from C[model C_ld + i m + j]
int launch_ls_chol(LaunchCtx c, const void *C, int64_t C_ld, int m, int64_t nmodels, bool cplx, void *a, double *e, int *status, int64_t out_ld);
// P[model P_ld + q] = 1 / sum_{k >= p} g_k |sum_i V[model m V_ld + i V_ld + k] e(-i (start + q step))|^2; status[model]: a weight was not positive
int launch_pseudo(LaunchCtx c, const void *V, int64_t V_ld, const double *w, int m, int p, int64_t nmodels, bool ev, int64_t nbins, double start, double step,
                  bool out64, void *P, int64_t P_ld, int *status);

// The array scan (k_beam.hip; include/spectral_array.h; the host's arithmetic in beam_plan.h): P[model P_ld + q] from V, w as k_eigh writes
// them and the device copies of the host tables pos[m][ndim], kv[nk][ndim], scale[nmodels] (or nullptr); `grid` workgroups walk the
// nmodels x ceil(nk / BEAM_TQ) items.  status[model]: a weight that was needed had a denominator that was not positive.
int launch_beam(LaunchCtx c, const void *V, int64_t V_ld, const double *w, int m, int64_t nmodels, const double *pos, int ndim, const double *kv, int64_t nk,
                const double *scale, int method, int p, double loading, bool out64, void *P, int64_t P_ld, int *status, int64_t grid);

// Conditioned spectral analysis (k_cond.hip; include/spectral_mimo.h; the host's arithmetic in cond_plan.h): one Cholesky factor of
// A = G[order][:, order] + delta I per matrix, and what `want` names of H [r][q], Gc [r][r], mcoh [r], piv [n], P [n][n] (r = n - q) at
// their pitches per matrix; pointers of outputs that are not wanted are never touched.  The permutation travels by value.
struct CondOrder {
    unsigned char p[COND_MAX_N];
};
struct CondArgs {
    const double2 *G;
    int64_t G_ld, count;
    int n, q;
    unsigned want;
    double loading;
    double2 *H, *Gc, *P;
    double *mcoh, *piv;
    int64_t H_ld, Gc_ld, mcoh_ld, piv_ld, P_ld;
    int *status;
    CondOrder order;
};
int launch_cond(LaunchCtx c, const CondArgs &a, const CondPlan &pl);

// The discrete wavelet transforms (k_dwt.hip; include/spectral_dwt.h; the host's arithmetic in dwt_plan.h).  Row form: a workgroup runs
// every level of rpw rows in LDS (lds = dwt_row_lds, cap = dwt_row_cap, lv the levels' lengths and the details' offsets in a row of outD /
// inD); tile form: one level per launch, DWT_TILE outputs of one row per workgroup.  Pitches count elements.
static_assert((size_t)DWT_LDS_MAX == SP_LDS_MAX, "dwt_plan.h states the LDS a workgroup may take");
struct DwtRowArgs {
    bool cplx;
    int64_t n, rows;
    DwtFilt f;
    int mode, levels, rpw;
    int64_t cap;
    size_t lds;
    DwtLv lv;
};
struct DwtTileArgs {
    bool cplx;
    int64_t rows;
    DwtFilt f;
    int mode;
};
int launch_dwt_row(LaunchCtx c, const DwtRowArgs &a, const void *x, int64_t x_ld, void *outA, int64_t a_ld, void *outD, int64_t d_ld);
int launch_idwt_row(LaunchCtx c, const DwtRowArgs &a, const void *inA, int64_t a_ld, const void *inD, int64_t d_ld, void *x, int64_t x_ld);
// W[(j - 1) plane + row w_ld + t], j = 1 .. levels, V_levels in the plane behind them
int launch_modwt_row(LaunchCtx c, const DwtRowArgs &a, const void *x, int64_t x_ld, void *W, int64_t w_ld, int64_t plane);
int launch_imodwt_row(LaunchCtx c, const DwtRowArgs &a, const void *W, int64_t w_ld, int64_t plane, void *x, int64_t x_ld);
int launch_dwt_tile(LaunchCtx c, const DwtTileArgs &a, const void *x, int64_t x_ld, int64_t n, void *cA, int64_t a_ld, void *cD, int64_t d_ld);
int launch_idwt_tile(LaunchCtx c, const DwtTileArgs &a, const void *cA, int64_t a_ld, const void *cD, int64_t d_ld, void *x, int64_t x_ld, int64_t nout);
int launch_modwt_tile(LaunchCtx c, const DwtTileArgs &a, int level, const void *vin, int64_t in_ld, int64_t n, void *W, int64_t w_ld, void *vout, int64_t out_ld);
int launch_imodwt_tile(LaunchCtx c, const DwtTileArgs &a, int level, const void *W, int64_t w_ld, const void *vin, int64_t in_ld, int64_t n, void *vout, int64_t out_ld);

// dispatch over the transform: MACRO(XTYPE) with XTYPE = XfPow2<L> or XfBlue<L>
#define SP_CASE_P(Lv, MACRO) case Lv: { MACRO(XfPow2<Lv>) } break;
#define SP_CASE_B(Lv, MACRO) case Lv: { MACRO(XfBlue<Lv>) } break;
#define SP_DISPATCH_X(xf, MACRO)                                                                      \
    if (!(xf).blue) {                                                                                 \
        switch ((xf).L) {                                                                             \
            SP_CASE_P(2, MACRO) SP_CASE_P(4, MACRO) SP_CASE_P(8, MACRO) SP_CASE_P(16, MACRO)          \
            SP_CASE_P(32, MACRO) SP_CASE_P(64, MACRO) SP_CASE_P(128, MACRO) SP_CASE_P(256, MACRO)     \
            SP_CASE_P(512, MACRO) SP_CASE_P(1024, MACRO) SP_CASE_P(2048, MACRO) SP_CASE_P(4096, MACRO) \
            SP_CASE_P(8192, MACRO)                                                                    \
            default: return -1;                                                                       \
        }                                                                                             \
    } else {                                                                                          \
        switch ((xf).L) {                                                                             \
            SP_CASE_B(16, MACRO) SP_CASE_B(32, MACRO) SP_CASE_B(64, MACRO) SP_CASE_B(128, MACRO)      \
            SP_CASE_B(256, MACRO) SP_CASE_B(512, MACRO) SP_CASE_B(1024, MACRO) SP_CASE_B(2048, MACRO) \
            SP_CASE_B(4096, MACRO) SP_CASE_B(8192, MACRO)                                             \
            default: return -1;                                                                       \
        }                                                                                             \
    }
#define SP_DISPATCH_P(xf, MACRO)                                                                      \
    switch ((xf).L) {                                                                                 \
        SP_CASE_P(2, MACRO) SP_CASE_P(4, MACRO) SP_CASE_P(8, MACRO) SP_CASE_P(16, MACRO)              \
        SP_CASE_P(32, MACRO) SP_CASE_P(64, MACRO) SP_CASE_P(128, MACRO) SP_CASE_P(256, MACRO)         \
        SP_CASE_P(512, MACRO) SP_CASE_P(1024, MACRO) SP_CASE_P(2048, MACRO) SP_CASE_P(4096, MACRO)    \
        SP_CASE_P(8192, MACRO)                                                                        \
        default: return -1;                                                                           \
    }

}   // namespace sp
