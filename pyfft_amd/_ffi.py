"""ctypes binding of libspectral.so (include/spectral.h).

The HIP library is the product: there is no CPU fallback.  Importing this module never touches
the GPU; the first call does (sp_init), and fails loudly if the shared object is missing, was not
built for gfx950, or no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SP_LIB_PATH") or os.path.join(_HERE, "lib", "libspectral.so")   # SP_LIB_PATH: diagnostic builds

DTYPE_F32, DTYPE_C64 = 0, 1
SIDED_ONE, SIDED_TWO, SIDED_RAW, SIDED_HALF = 1, 2, 3, 4
DETREND_CONST, DETREND_MEAN, DETREND_LINEAR, DETREND_SEGMEAN, DETREND_SEGLINEAR = 0, 1, 2, 3, 4
XC_RAW, XC_COEFF = 0, 1
DETREND_NONE = 0
SKF_MEAN, SKF_CROSS = 0, 1
CWT_MORLET, CWT_PAUL = 0, 1

_lib = None

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double

# name -> (restype, argtypes); must list every symbol include/spectral.h declares
SIGNATURES = {
    "sp_init": (_i, [_i]),
    "sp_shutdown": (None, []),
    "sp_last_error": (C.c_char_p, []),
    "sp_set_stream": (_i, [_vp]),
    "sp_synchronize": (_i, []),
    "sp_version": (_i, []),
    "sp_max_wg_fft": (_i, []),
    "sp_device_info": (_i, [C.POINTER(_i64)]),
    "sp_profile_enable": (_i, [_i]),
    "sp_profile_last_ms": (_i, [C.POINTER(_d)]),
    "sp_profile_last_kernel": (C.c_char_p, []),
    "sp_fft_c2c": (_i, [_vp, _vp, _i64, _i64, _i, _i]),
    "sp_welch_psd": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i, _d, _d, _i, _d, _vp, _i]),
    "sp_welch_accum": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i64, _vp, _i]),
    "sp_welch_finish": (_i, [_vp, _i64, _i, _d, _vp, _i]),
    "sp_welch_export": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i64, _vp, _i]),
    "sp_welch_apply": (_i, [_vp, _vp, _i, _i64, _i, _d, _vp, _i]),
    "sp_comm_unique_id": (_i, [_vp]),
    "sp_comm_init": (_i, [_vp, _i, _i]),
    "sp_comm_info": (_i, [C.POINTER(_i)]),
    "sp_comm_destroy": (_i, []),
    "sp_welch_dist_submit": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i64, _i64, _i, _d, _vp, C.POINTER(_i)]),
    "sp_welch_dist_flush": (_i, [C.POINTER(_i)]),
    "sp_welch_psd_dist": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i64, _i64, _i, _d, _vp]),
    "sp_welch_csd": (_i, [_vp, _vp, _i, _i64, _i, _i64, _vp, _i, _i, _i64, _i, _vp, _vp, _i, _d, _vp, _vp, _vp, _i]),
    "sp_csd_matrix": (_i, [_vp, _i, _i64, _i64, _vp, _i, _i, _i64, _i, _d, _vp, _i]),
    "sp_csd_matrix_means": (_i, [_vp, _i, _i64, _i64, _vp, _i, _i, _i64, _vp, _d, _vp, _i]),
    "sp_channel_means": (_i, [_vp, _i, _i64, _i64, _vp, _i]),
    "sp_stft": (_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i, _d, _d, _i, _d, _i, _i, _vp, _vp, _i]),
    "sp_istft": (_i, [_vp, _i, _i, _i, _i64, _vp, _i, _i, _d, _i64, _i64, _vp, _i]),
    "sp_bispectrum": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _i, _i, _i64, _i, _d, _d, _vp, _vp, _vp, _i]),
    "sp_multitaper": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i, _i64, _i, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp, _i]),
    "sp_czt": (_i, [_vp, _i, _i64, _i64, _i64, _i64, _d, _d, _vp, _i]),
    "sp_zoom_welch": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i64, _i, _vp, _vp, _i64, _d, _d, _d, _vp, _vp, _vp, _vp, _i]),
    "sp_czt_chirp": (_i, [_i64, _i64, _d, _d, _vp]),
    "sp_ddc": (_i, [_vp, _i, _i64, _i64, _i64, _d, _i64, _i, _vp, _i, _vp, _i]),
    "sp_ddc_tile": (_i, [_i]),
    "sp_upfirdn": (_i, [_vp, _i, _i64, _i64, _i64, _vp, _i, _i, _i, _i64, _i64, _vp, _i]),
    "sp_upfirdn_tile": (_i, [_i, _i, _i, _i]),
    "sp_pfb": (_i, [_vp, _i, _i64, _i64, _i64, _vp, _i, _i, _i, _i64, _i64, _i, _i, _i, _i, _d, _vp, _i]),
    "sp_pfb_synth": (_i, [_vp, _i, _i, _i64, _i64, _vp, _i, _i, _i, _i64, _i, _i, _d, _i64, _vp, _i]),
    "sp_pfb_synth_plan": (_i, [_i, _i64, _i64, _i, _i, _i, C.POINTER(_i64)]),
    "sp_stft_cog":(_i, [_vp, _i, _i64, _vp, _i, _i, _i64, _i, _d, _d, _d, _d, _d, _vp, _i]),
    "sp_hilbert": (_i, [_vp, _i64, _i64, _i64, _i64, _vp, _i]),
    "sp_frame_sum": (_i, [_vp, _i, _i64, _i, _i64, _i, _i, _i64, _i, _vp, _i]),
    "sp_spectral_filter": (_i, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _i]),
    "sp_xcorr": (_i, [_vp, _vp, _i64, _vp, _i]),
    "sp_xcorr_frames": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i64, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _i]),
    "sp_xcorr_frames_len": (_i, [_i, _i]),
    "sp_skf": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i64, _i, _i, _i, _i, _i, _d, _vp, _i]),
    "sp_skf_plan": (_i, [_i, _i, _i, _i, _vp]),
    "sp_welch_blocks": (_i, [_vp, _vp, _i, _i64, _i, _i64, _vp, _i, _i, _i64, _i, _i, _i, _d, _i, _vp, _vp, _vp, _i]),
    "sp_welch_blocks_plan": (_i, [_i, _i, _i, _i64, _i, _i, _i, _vp]),
    "sp_cwt": (_i, [_vp, _i, _i64, _i64, _i64, _vp, _i, _i, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "sp_cwt_plan": (_i, [_i64, _i, _i64, _i, _i, _i, _vp]),
    "sp_icwt": (_i, [_vp, _i64, _i, _i64, _vp, _vp, _i]),
    "sp_eigh": (_i, [_vp, _i, _i64, _i, _i, _vp, _vp, _vp, _i]),
    "sp_eigh_plan": (_i, [_i, _i, _i64, C.POINTER(_i64)]),
    "sp_fftfilt": (_i, [_vp, _i, _vp, _i64, _i, _vp, _i]),
    "sp_biquad": (_i, [_vp, _vp, _vp, _i64, _vp, _i]),
    "sp_sosfilt": (_i, [_vp, _i, _vp, _i64, _i64, _vp, _vp, _vp, _i]),
    "sp_sosfiltfilt": (_i, [_vp, _i, _vp, _i64, _i64, _i, _i64, _vp, _i]),
    "sp_csd_epilogue_doubles": (_i64, [_i, _i, _i]),
    "sp_csd_epilogue": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _d, _vp, _i]),
    "sp_mean": (_i, [_vp, _i, _i64, C.POINTER(_d), _i]),
}

# the second table: must list every symbol include/spectral_ext.h declares, and none of the first
EXT_SIGNATURES = {
    "sp_wct_time": (_i, [_vp, _i64, _vp, _i64, _i, _i64, _i64, _vp, _i, _i, _d, _i, _i, _i, _vp, _vp, _i]),
    "sp_wct_scale": (_i, [_vp, _i64, _i, _i64, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "sp_wct_plan": (_i, [_i64, _i, _i64, _i, _i, _i, _i, _vp]),
    "sp_last_passes": (_i, [_i]),
}

# the third table: must list every symbol include/spectral_tfr.h declares, and none of the other two
TFR_SIGNATURES = {
    "sp_ssq": (_i, [_vp, _i64, _i, _i64, _i64, _vp, _vp, _vp, _i, _i, _i64, _i64, _i, _d, _d, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "sp_ssq_bands": (_i, [_vp, _i64, _i, _i64, _i64, _vp, _vp, _i, _i, _i64, _i64, _i, _d, _d, _i, _vp, _vp, _d, _vp, _i]),
    "sp_ssq_sum": (_i, [_vp, _i64, _i, _i64, _i, _i, _i, _vp, _vp, _i, _d, _vp, _i]),
    "sp_ssq_plan": (_i, [_i, _i, _i64, _i64, _i, _i, _vp]),
}

# the fourth table: must list every symbol include/spectral_quad.h declares, and none of the other three
QUAD_SIGNATURES = {
    "sp_wvd": (_i, [_vp, _vp, _i64, _i64, _i64, _vp, _i, _vp, _i, _i, _i64, _i64, _i64, _i, _i, _d, _vp, _i]),
    "sp_wvd_plan": (_i, [_i, _i, _i, _i, _i64, _i64, _i64, _i, _vp]),
}

# the fifth table: must list every symbol include/spectral_cyclo.h declares, and none of the other four
CYCLO_SIGNATURES = {
    "sp_cyclic": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i64, _vp, _i, _i64, _i64, _i64, _vp, _i, _i, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _i]),
    "sp_cyclic_plan": (_i, [_i, _i, _i, _i, _i64, _i64, _i, _i64, _vp]),
}

# the sixth table: must list every symbol include/spectral_uneven.h declares, and none of the other five
UNEVEN_SIGNATURES = {
    "sp_lomb": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _d, _vp, _i64, _vp, _i, _i, _vp, _i]),
    "sp_lomb_sums": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _d, _d, _vp, _i64, _vp, _vp, _vp, _vp, _i]),
    "sp_lomb_finish": (_i, [_vp, _vp, _vp, _i64, _i64, _d, _vp, _i64, _vp, _i, _i, _vp, _i]),
    "sp_lomb_plan": (_i, [_i64, _i64, _i64, _vp]),
}

# the seventh table: must list every symbol include/spectral_wbic.h declares, and none of the other six
WBIC_SIGNATURES = {
    "sp_wbic": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp, _i, _i, _i, _d, _i, _i, _i64, _i64, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i), _i]),
    "sp_wbic_plan": (_i, [_i64, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _i, _i, _vp]),
}

# the eighth table: must list every symbol include/spectral_fam.h declares, and none of the other seven
FAM_SIGNATURES = {
    "sp_fam": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i64, _vp, _i, _i64, _vp, _i64, _i, _vp, _vp, _d, _vp, _vp, _vp, _i]),
    "sp_fam_plan": (_i, [_i, _i, _i, _i64, _i, _i64, _i64, _vp]),
}

# the ninth table: must list every symbol include/spectral_nufft.h declares, and none of the other eight
NUFFT_SIGNATURES = {
    "sp_nufft1": (_i, [_vp, _vp, _i64, _i64, _i64, _d, _d, _d, _i64, _i, _vp, _i]),
    "sp_lomb_sums_grid": (_i, [_vp, _vp, _vp, _i64, _i64, _i64, _d, _d, _d, _d, _i64, _vp, _vp, _vp, _vp, _i]),
    "sp_nufft1_plan": (_i, [_i64, _i64, _i64, _vp]),
}

# the tenth table: must list every symbol include/spectral_nufft2.h declares, and none of the other nine
NUFFT2_SIGNATURES = {
    "sp_nufft2": (_i, [_vp, _vp, _i64, _i64, _i64, _d, _d, _d, _i64, _i, _vp, _i64, _i]),
    "sp_nufft2_plan": (_i, [_i64, _i64, _i64, _vp]),
}

# the eleventh table: must list every symbol include/spectral_ar.h declares, and none of the other ten
_AR_FIT = (_i, [_vp, _i, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i, _i, _d, _d, _vp, _vp, _vp, _i64, _i])
AR_SIGNATURES = {
    "sp_burg": _AR_FIT,
    "sp_yule": _AR_FIT,
    "sp_ar_psd": (_i, [_vp, _i, _i64, _vp, _i64, _i, _i64, _i64, _d, _d, _d, _i, _vp, _i64, _i]),
    "sp_ar_plan": (_i, [_i, _i, _i64, _i, _i64, _i64, _vp]),
}

# the twelfth table: must list every symbol include/spectral_sub.h declares, and none of the other eleven
_SUB_REC = [_vp, _i, _i64, _i64, _i64, _i64, _i64, _i64, _i64]
SUB_SIGNATURES = {
    "sp_covmat": (_i, _SUB_REC + [_i, _i, _i, _d, _d, _vp, _i64, _i]),
    "sp_ar_ls": (_i, _SUB_REC + [_i, _i, _i, _d, _d, _vp, _vp, _vp, _i64, _i]),
    "sp_pseudospectrum": (_i, [_vp, _i64, _vp, _i, _i, _i64, _i, _i64, _d, _d, _i, _vp, _i64, _vp, _i]),
    "sp_sub_plan": (_i, [_i, _i, _i64, _i, _i64, _i64, _vp]),
}

# the thirteenth table: must list every symbol include/spectral_dwt.h declares, and none of the other twelve
_DWT_ROWS = [_vp, _i, _i64, _i64, _i64, _vp, _vp, _i]                 # rows, dtype, pitch, n, batch, the two filters (host float64), L
DWT_SIGNATURES = {
    "sp_dwt": (_i, _DWT_ROWS + [_i, _i, _vp, _i64, _i, _i]),
    "sp_dwt_level": (_i, _DWT_ROWS + [_i, _vp, _i64, _vp, _i64, _i, _i]),
    "sp_idwt": (_i, _DWT_ROWS + [_i, _i, _vp, _i64, _i, _i]),
    "sp_idwt_level": (_i, [_vp, _i64, _vp, _i64, _i, _i64, _i64, _vp, _vp, _i, _i, _vp, _i64, _i, _i]),
    "sp_modwt": (_i, _DWT_ROWS + [_i, _vp, _i64, _i, _i]),
    "sp_imodwt": (_i, _DWT_ROWS + [_i, _vp, _i64, _i, _i]),
    "sp_dwt_plan": (_i, [_i, _i, _i64, _i, _i, _i, _i64, _i, _vp]),
}

# the fourteenth table: must list every symbol include/spectral_array.h declares, and none of the other thirteen
ARRAY_SIGNATURES = {
    "sp_beamscan": (_i, [_vp, _i64, _vp, _i, _i64, _vp, _i, _vp, _i64, _vp, _i, _i, _d, _i, _vp, _i64, _vp, _i]),
    "sp_beamscan_plan": (_i, [_i, _i, _i64, _i64, _i, _i, _vp]),
}

# the fifteenth table: must list every symbol include/spectral_mimo.h declares, and none of the other fourteen
_u = C.c_uint                          # the bit mask of wanted outputs
MIMO_SIGNATURES = {
    "sp_cond": (_i, [_vp, _i64, _i, _i64, _vp, _i, _u, _d, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i]),
    "sp_cond_plan": (_i, [_i, _i, _i64, _u, _vp]),
}

# the six tables the engine trace counts, in the order of their headers
TABLES = (SIGNATURES, EXT_SIGNATURES, TFR_SIGNATURES, QUAD_SIGNATURES, CYCLO_SIGNATURES, UNEVEN_SIGNATURES)
# the tables added since: bound like the six, outside the trace
MORE_TABLES = (WBIC_SIGNATURES, FAM_SIGNATURES, NUFFT_SIGNATURES, NUFFT2_SIGNATURES, SUB_SIGNATURES, AR_SIGNATURES)
# ... and those added after them, bound alike
LATER_TABLES = (DWT_SIGNATURES,)
# ... and the array scan, in a tuple of its own: the three above stay as they are
ARRAY_TABLES = (ARRAY_SIGNATURES,)
# ... and conditioned spectral analysis, alike
MIMO_TABLES = (MIMO_SIGNATURES,)


class SpectralError(RuntimeError):
    pass


def load_library():
    """dlopen libspectral.so and bind every declared symbol (no GPU work)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SpectralError("libspectral.so not found at %s -- run `make` (or __graft_entry__.build()); "
                            "pyfft_amd has no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for table in TABLES + MORE_TABLES + LATER_TABLES + ARRAY_TABLES + MIMO_TABLES:
        for name, (res, args) in table.items():
            fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def lib():
    l = load_library()
    return l


def check(rc):
    if rc != 0:
        raise SpectralError((lib().sp_last_error() or b"unknown error").decode())


def init(device=-1):
    check(lib().sp_init(int(device)))


def ptr(a):
    """void* of a C-contiguous numpy array or a raw device address (int) / None."""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


def dtype_code(arr_dtype):
    if arr_dtype == np.float32:
        return DTYPE_F32
    if arr_dtype == np.complex64:
        return DTYPE_C64
    raise TypeError("device path takes float32 or complex64 samples, got %s" % arr_dtype)


def as_samples(x):
    """Cast like the reference's device boundary would: real -> float32, complex -> complex64, contiguous."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return np.ascontiguousarray(x, dtype=np.complex64)
    return np.ascontiguousarray(x, dtype=np.float32)
