"""pyfft_amd -- MI355X-native spectral-analysis engine behind gmweir/PYFFT's function signatures.

Mirrors the reference package's export list (__init__.py:11-31) for the hot path:
    fft_analysis (alias `fft`), fft_pwelch, fftanal, windows, specgram, stft, hilbert, hilbert_1d, ccf,
    iirnotch, iirpeak, butter_lowpass_filter, butter_bandpass, plus the build-defined fftfilt / apply_notch.
(upsample / downsample / downsample_efficient need the absent pybaseutils.utils.interp: filters.py raises
NotImplementedError for them.)
Importing the package loads nothing from the GPU; the first kernel call initialises the HIP library
(pyfft_amd/lib/libspectral.so) and fails loudly if it is missing -- there is no CPU fallback.
"""
from . import _ffi                      # noqa: F401
from . import engine                    # noqa: F401
from . import fft_analysis              # noqa: F401
from . import fft_analysis as fft       # noqa: F401   (reference: `import fft_analysis as fft`, __init__.py:21)
from . import spectrogram, hilbert as _hilbert_mod, ccf as _ccf_mod, filters, notch_filter   # noqa: F401
from .windows import windows            # noqa: F401
from .fft_analysis import fft_pwelch, fftanal, Cxy_Cxy2, psd, csd, coh, coh2     # noqa: F401
from .fft_analysis import detrend_none, detrend_mean, detrend_linear, unwrap_tol, fft_deriv   # noqa: F401  (__init__.py:22-23)
from .fft_analysis import integratespectra, varcoh, varphi, mean_angle                       # noqa: F401  (fft_analysis.py:835, :1218-1376)
from .spectrogram import specgram, stft, istft               # noqa: F401
from .hilbert import hilbert, hilbert_1d                     # noqa: F401
from .ccf import ccf, ccf_sh, ccf_frames, delay_track, ccf_plan   # noqa: F401
from .notch_filter import iirnotch, iirpeak, apply_notch     # noqa: F401
from .filters import fftfilt                                 # noqa: F401
from .filters import butter_lowpass_filter, butter_bandpass  # noqa: F401   (__init__.py:27)
from . import doppler                                        # noqa: F401   (Doppler.cog / cogspec window loop)
from .doppler import cog, cog_frames                         # noqa: F401
from . import heatpulse                                      # noqa: F401   (HeatPulse_Funcs._PWELCH_chloop as one call)
from .heatpulse import pwelch_chloop                         # noqa: F401
from . import bispectrum as _bispectrum_mod                     # noqa: F401
from .bispectrum import bispectrum, bicoherence              # noqa: F401
from . import multitaper as _multitaper_mod                  # noqa: F401
from .multitaper import (multitaper_psd, multitaper_spectra, multitaper_csd, multitaper_coherence,  # noqa: F401
                         multitaper_plan)
from . import zoom as _zoom_mod                                # noqa: F401
from .zoom import czt, zoom_fft, zoom_stft, zoom_psd, zoom_csd, zoom_coherence, zoom_plan   # noqa: F401
from . import baseband as _baseband_mod                        # noqa: F401
from .baseband import ddc, ddc_plan, band_stft, band_psd, band_csd, band_coherence, band_plan   # noqa: F401
from . import channelizer as _channelizer_mod                  # noqa: F401
from .channelizer import pfb_prototype, pfb_plan, channelize, pfb_psd   # noqa: F401
from .channelizer import pfb_alias_terms, pfb_dual, pfb_synthesis_plan, synthesize   # noqa: F401
from . import wavenumber as _wavenumber_mod                    # noqa: F401
from .wavenumber import skf, skf_moments, dispersion, skf_plan   # noqa: F401
from . import spod as _spod_mod                                # noqa: F401
from .spod import spod, spod_energy, spod_reconstruct, spod_plan   # noqa: F401
from . import resample as _resample_mod                        # noqa: F401
from .resample import upfirdn, resample_poly, resample_rate, resample_plan   # noqa: F401
from . import running as _running_mod                          # noqa: F401
from .running import (running_psd, running_csd, running_coherence, running_spectra, running_plan,   # noqa: F401
                      coherence_level)
from . import wavelet as _wavelet_mod                          # noqa: F401
from .wavelet import Morlet, Paul, cwt_scales, cwt, icwt, cwt_power, cwt_filter, cwt_plan   # noqa: F401
from .wavelet import xwt, wct, wct_plan   # noqa: F401
from . import reassign as _reassign_mod                        # noqa: F401
from .reassign import (reassignment_windows, ssq_stft, issq_stft, squeezed_spectrogram, reassignment_fields,   # noqa: F401
                       ssq_extract, ssq_plan)
from . import wigner as _wigner_mod                            # noqa: F401
from .wigner import spwvd, pwvd, wvd, xwvd, wvd_plan           # noqa: F401
from . import cyclic as _cyclic_mod                            # noqa: F401
from .cyclic import (scd, cyclic_coherence, cyclic_spectra, cyclic_profile, alpha_grid, cyclic_level,   # noqa: F401
                     cyclic_plan)
from . import lomb as _lomb_mod                                # noqa: F401
from .lomb import lombscargle, ls_periodogram, ls_window, ls_grid, ls_level, ls_plan     # noqa: F401
from . import nufft as _nufft_mod                              # noqa: F401
from .nufft import (nufft1, nufft1_modes, nufft_plan, nufft2, nufft2_modes, nufft2_plan, nufft_fit, regrid,   # noqa: F401
                    NufftFit)
from . import parametric as _parametric_mod                    # noqa: F401
from .parametric import (arburg, aryule, pburg, pyulear, ar_spectrogram, ar_psd, ar_order, ar_stepup, ar_poles, ar_plan,   # noqa: F401
                         ArRefused, arcov, armcov, pcov, pmcov)
from . import subspace as _subspace_mod                        # noqa: F401
from .subspace import (corrmtx_cov, pmusic, peig, subspace_spectrogram, subspace_order, esprit, subspace_plan,   # noqa: F401
                       SubRefused)
from . import dwt as _dwt_mod                                  # noqa: F401
from .dwt import (wavelet_filters, dwt_max_level, dwt_coeff_len, dwt, idwt, wavedec, waverec, modwt, imodwt, modwt_mra,   # noqa: F401
                  modwt_variance, wpdec, wprec, dwt_plan, DwtRefused)
from . import beamform as _beamform_mod                        # noqa: F401
from .beamform import (array_spectrum, mode_spectrum, beam_scan, slowness_scan, array_pattern, beam_peaks, beam_plan,   # noqa: F401
                       BeamRefused)
from . import mimo as _mimo_mod                                # noqa: F401
from .mimo import (cond, cond_plan, mimo_frf, multiple_coherence, partial_coherence, conditioned_spectra, ordered_spectra,   # noqa: F401
                   multiple_coherence_level, CondRefused, CondResult)
from . import wbicoherence as _wbic_mod                        # noqa: F401
from .wbicoherence import (wbic_freqs, wavelet_bispectrum, wavelet_bicoherence, summed_bicoherence,   # noqa: F401
                           total_bicoherence, wbic_plan)
from . import fam as _fam_mod                                  # noqa: F401
from .fam import FamPlane, fam_pairs, fam_axes, scd_fam, fam_coherence, fam_profile, fam_cells, fam_plan     # noqa: F401
