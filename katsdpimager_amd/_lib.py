"""ctypes binding of libkimg.so (the C ABI declared in include/kimg.h).

The HIP extension is mandatory: there is no CPU fallback.  ``lib()`` raises
:class:`KimgLibraryError` if the shared library has not been built or cannot
be loaded.  PyTorch-ROCm is imported first so that libkimg.so resolves the HIP
runtime and rocFFT already loaded by torch (same SONAMEs) -- device pointers
and streams created by torch are then valid inside the library.
"""
import ctypes
import threading
import os
from ctypes import c_int, c_int64, c_float, c_double, c_size_t, c_uint32, c_void_p, c_char_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libkimg.so')

P = c_void_p
I = c_int
L = c_int64
F = c_float
D = c_double

VERSION = 5     # KIMG_VERSION of include/kimg.h

PROTOTYPES = {
    'kimg_version': (c_int, []),
    'kimg_error_string': (c_char_p, [I]),
    'kimg_kernel_table': (c_int, [P, P, I, I, I, I, c_double, c_double, c_double, P]),
    'kimg_grid_workspace_bytes': (c_size_t, [L, I, I, I, I]),
    'kimg_grid_binned_workspace_bytes': (c_size_t, [L, I, I, I, I]),
    'kimg_grid_jumps': (c_int, [P, L, I, P, P]),
    'kimg_fold_runs_workspace_bytes': (c_size_t, [I, L]),
    'kimg_fold_runs': (c_int, [P, P, P, L, I, L, P, c_size_t, P]),
    'kimg_grid': (c_int, [P, L, L, I, I, P, L, L, P, P, P, L, P, I, I, I, P, c_size_t, I, I, P]),
    # fold plans: the unplanned argument lists plus the plan
    'kimg_fold_plan_bytes': (c_size_t, []),
    'kimg_fold_plan': (c_int, [P, P, L, I, P, P]),
    'kimg_fold_runs_planned': (c_int, [P, P, P, L, I, L, P, c_size_t, P, P]),
    'kimg_grid_planned': (c_int, [P, L, L, I, I, P, L, L, P, P, P, L, P, I, I, I, P, c_size_t, I, I, P, P]),
    # fold maps: (num_vis, P, heads); (uv, w_plane, num_vis, P, plan, map, map_bytes, stream); the
    # unplanned argument lists plus the map
    'kimg_fold_map_bytes': (c_size_t, [L, I, L]),
    'kimg_fold_map': (c_int, [P, P, L, I, P, P, c_size_t, P]),
    'kimg_fold_runs_mapped': (c_int, [P, P, P, L, I, L, P, c_size_t, P, P]),
    'kimg_grid_mapped': (c_int, [P, L, L, I, I, P, L, L, P, P, P, L, P, I, I, I, P, c_size_t, I, I, P, P]),
    'kimg_degrid': (c_int, [P, L, L, I, I, P, P, P, P, L, P, I, I, I, P, c_size_t, I, I, P]),
    'kimg_degrid_workspace_bytes': (c_size_t, [I, I, I, I]),
    'kimg_degrid_binned_workspace_bytes': (c_size_t, [L, I, I, I, I]),
    'kimg_predict': (c_int, [P, P, P, P, P, P, L, I, I, I, F, F, F, P]),
    'kimg_grid_weights': (c_int, [P, L, L, I, I, I, P, P, L, P]),
    'kimg_mean_weight': (c_int, [P, P, L, I, I, P]),
    'kimg_density_weights': (c_int, [P, P, L, L, I, I, I, F, F, P]),
    'kimg_density_weights_robust': (c_int, [P, P, L, L, I, I, I, P, c_double, F, P]),
    # uv taper: kimg_density_weights' arguments, (mean_sums, robust), the cell steps, kimg_uv_taper *
    'kimg_density_weights_taper': (c_int, [P, P, L, L, I, I, I, F, F, P, D, D, D, P, P]),
    'kimg_fill': (c_int, [P, L, F, P]),
    'kimg_preprocess_convert': (c_int, [I, I, L, P, P, P, P, P, P, P, F, I, I, I, F, P, P, P, P]),
    'kimg_preprocess_workspace_bytes': (ctypes.c_size_t, [L, I]),
    'kimg_preprocess_compress': (c_int, [I, L, I, P, P, P, P, P, P, P, P, L, P, ctypes.c_size_t, P]),
    'kimg_real_to_complex': (c_int, [P, P, L, P]),
    'kimg_store_reorder_workspace_bytes': (c_size_t, [L]),
    'kimg_store_reorder': (c_int, [I, L, I, I, I, I, P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    'kimg_grid_to_layer': (c_int, [P, I, P, L, I, P]),
    'kimg_grid_to_half_layer': (c_int, [P, I, P, L, I, P]),
    'kimg_real_layer_to_image': (c_int, [P, L, P, L, I, P, F, F, P]),
    'kimg_image_to_real_layer': (c_int, [P, L, P, L, I, P, F, F, P]),
    'kimg_half_layer_to_grid': (c_int, [P, L, I, P, I, P]),
    'kimg_set_window_cus': (c_int, [I]),
    'kimg_get_window_cus': (c_int, []),
    'kimg_grid_image_real_supported': (c_int, [I, I]),
    'kimg_grid_image_real_workspace_bytes': (c_size_t, [I, I]),
    'kimg_grid_to_image_real': (c_int, [P, L, I, P, L, I, P, F, F, I, P, c_size_t, P]),
    'kimg_image_to_grid_real': (c_int, [P, L, I, P, L, I, P, F, F, P, c_size_t, P]),
    'kimg_convolve_beam': (c_int, [P, L, I, F, F, F, F, P, c_size_t, P]),
    'kimg_grid_image_w_workspace_bytes': (c_size_t, [I, I]),
    'kimg_grid_to_image_w': (c_int, [P, L, I, P, L, I, P, F, F, F, I, P, c_size_t, P]),
    'kimg_image_to_grid_w': (c_int, [P, L, I, P, L, I, P, F, F, F, P, c_size_t, P]),
    'kimg_layer_to_grid': (c_int, [P, L, I, P, I, P]),
    'kimg_layer_to_image': (c_int, [P, L, P, I, P, F, F, F, P]),
    'kimg_image_to_layer': (c_int, [P, P, L, I, P, F, F, F, P]),
    'kimg_fft_plan_create': (c_int, [ctypes.POINTER(c_void_p), I, I]),
    'kimg_fft_exec': (c_int, [P, P, I, P]),
    'kimg_fft_plan_destroy': (c_int, [P]),
    'kimg_rfft_plan_create': (c_int, [ctypes.POINTER(c_void_p), I, I]),
    'kimg_rfft_exec': (c_int, [P, P, P, I, P]),
    'kimg_rfft_plan_destroy': (c_int, [P]),
    'kimg_fourier_beam': (c_int, [P, L, I, I, F, F, F, F, P]),
    'kimg_image_peak': (c_int, [P, L, L, P, L, I, I, I, F, P, P]),
    'kimg_image_nansum': (c_int, [P, L, L, I, I, I, P, P]),
    'kimg_scale': (c_int, [P, L, L, I, I, I, ctypes.POINTER(c_float), P]),
    'kimg_pixel_reciprocal': (c_int, [P, L, L, I, I, I, I, I, P, P]),
    'kimg_scale_device': (c_int, [P, L, L, I, I, I, P, P]),
    'kimg_add_image': (c_int, [P, L, L, P, L, L, I, I, I, P]),
    'kimg_apply_primary_beam': (c_int, [P, L, L, P, L, I, I, I, F, F, P]),
    'kimg_psf_patch': (c_int, [P, L, L, I, I, I, I, I, I, I, F, P, P]),
    'kimg_abs_histogram': (c_int, [P, L, L, I, I, I, I, I, c_uint32, P, P]),
    'kimg_abs_count_le': (c_int, [P, L, L, I, I, I, I, F, P, P]),
    'kimg_update_tiles': (c_int, [P, L, L, I, I, I, I, I, P, P, I, I, I, I, I, I, P]),
    'kimg_find_peak': (c_int, [P, L, L, I, P, P, I, I, P, P, P, P]),
    'kimg_subtract_psf': (c_int, [P, P, L, L, I, I, I, P, L, L, I, I, I, I, P, I, I, F, P]),
    'kimg_noise_est_scratch_bytes': (c_size_t, []),
    'kimg_preload': (c_int, []),
    'kimg_noise_est': (c_int, [P, L, L, I, I, I, I, F, P, P, P]),
    'kimg_clean_state_bytes': (c_size_t, [I, I, I]),
    'kimg_clean_cycles': (c_int, [P, P, L, L, I, I, I, P, L, L, I, I, I, I, I, I, F, F,
                                  P, P, I, I, I, I, P, P, P]),
    'kimg_clean_major_cycles': (c_int, [P, P, L, L, I, I, I, P, L, L, I, I, I, I, I, I, F, c_double, c_double,
                                        P, P, I, I, I, I, P, P, P, P, P]),
    'kimg_clean_cycles_batch': (c_int, [P, I, L, L, I, I, I, L, L, I, I, I, I, F, I, I, P]),
    # CLEAN masks: the unmasked argument lists plus (mask, mask_row_stride)
    'kimg_update_tiles_masked': (c_int, [P, L, L, I, I, I, I, I, P, P, I, I, I, I, I, I, P, P, L]),
    'kimg_find_peak_masked': (c_int, [P, L, L, I, P, P, I, I, P, P, P, P, P, L]),
    'kimg_clean_cycles_masked': (c_int, [P, P, L, L, I, I, I, P, L, L, I, I, I, I, I, I, F, F,
                                         P, P, I, I, I, I, P, P, P, P, L]),
    # CLEAN auto-masks
    'kimg_mask_threshold': (c_int, [P, L, L, I, I, I, I, I, F, P, L, P]),
    'kimg_mask_dilate': (c_int, [P, L, P, L, I, I, I, P, L, P, L, P, P]),
    # multi-scale CLEAN
    'kimg_image_convolve_separable': (c_int, [P, L, L, P, L, L, P, L, L, I, I, I, P, I, P]),
    'kimg_clean_scales_workspace_bytes': (c_size_t, [I, I, I, I, I, I, I, P]),
    'kimg_clean_scales_setup': (c_int, [P, L, L, P, L, L, I, I, I, I, I, I, I, P, P, P, I, P, L,
                                        P, c_size_t, P]),
    'kimg_clean_scales_cycles': (c_int, [P, P, L, L, I, I, I, I, I, I, I, F, F, I, P, P, I, P, L,
                                         P, c_size_t, P, P, P]),
    # UV-plane continuum subtraction
    'kimg_uvcontsub': (c_int, [P, L, P, L, I, L, P, P, I, P, P]),
    # phase-centre shift
    'kimg_phase_shift': (c_int, [P, L, I, L, I, P, P, P, P, P]),
    # primary-beam correction: (beam_power, pitch), (model, dirty, pitches), the shape, (row,
    # num_samples, inv_step), lm_scale, lm_bias, threshold
    'kimg_primary_beam': (c_int, [P, L, P, P, L, L, I, I, I, P, I, F, F, F, F, P]),
    # spectral filter: (vis_in, pitch, weights_in, pitch, C_in), (vis_out, pitch, weights_out, pitch,
    # C_out), plane_elements, (coeff_host, length, offset, step), min_sum, counts, stream
    'kimg_spectral_filter': (c_int, [P, L, P, L, I, P, L, P, L, I, L, P, I, I, I, D, P, P]),
    # statistical reweighting: (vis, pitch, weights, pitch, C, N, P), fit_mask_host, (group_offsets, G,
    # row_group), time_bin, min_samples, (chi2_lo, chi2_hi), chi2, (workspace, bytes), counts, stream
    'kimg_statwt': (c_int, [P, L, P, L, I, L, I, P, P, L, P, I, I, D, D, P, P, c_size_t, P, P]),
    # RFI flagging: (vis, pitch, weights, pitch, C, N, P), mask_host, (group_offsets, G, row_group),
    # time_bin, (factors_host, max_window), directions, (level_iterations, level_clip), (extend_freq,
    # extend_time, extend_pols), flags, level, (workspace, bytes), counts, stream
    'kimg_rfi_flag': (c_int, [P, L, P, L, I, L, I, P, P, L, P, I, P, I, I, I, D, D, D, I, P, P, P,
                              c_size_t, P, P]),
    # moment maps: (cube, pitch, C, M), (first, stop), (x, cut, filled_host), width, select_hanning,
    # outputs (KIMG_MOMENT_* bits), (moment0, moment1, moment2, moment8, moment9, count), stream
    'kimg_moments': (c_int, [P, L, I, L, I, I, P, P, P, D, I, I, P, P, P, P, P, P, P]),
    # image-plane continuum subtraction: (cube, pitch, line, pitch, C, M), (filled_host, fit_host,
    # w_host), (w, basis, order), bref0 .. bref3, min_samples, outputs (KIMG_IMCONTSUB_* bits),
    # (continuum, coefficients, coefficient_pitch, rms, count), stream
    'kimg_imcontsub': (c_int, [P, L, P, L, I, L, P, P, P, P, P, I, D, D, D, D, I, I, P, P, L, P, P, P]),
    # cube smoothing to a common beam: (cube, pitch, out, pitch), (C, P, H, W), (filled_host,
    # radius_host), (taps, taps_pitch), stream
    'kimg_cube_smooth': (c_int, [P, L, P, L, I, I, I, I, P, P, P, L, P]),
    # cube plane statistics: (C, G); (cube, pitch), (C, P, H, W), filled_host, (first, stop),
    # pool_polarizations, estimator, border, region, scratch, (count, min, max, median, sigma), stream
    'kimg_cube_stats_scratch_bytes': (c_size_t, [I, I]),
    'kimg_cube_stats': (c_int, [P, L, I, I, I, I, P, I, I, I, I, I, P, P, P, P, P, P, P, P]),
    # spectrum statistics: (cube, pitch, C, M), (first, stop), (stat_host, filled_host), estimator,
    # min_samples, outputs (KIMG_SPECTRUM_* bits), (median, sigma, min, max, count), (line, pitch),
    # form, stream
    'kimg_spectrum_stats_resident_limit': (c_int, []),
    'kimg_spectrum_stats': (c_int, [P, L, I, L, I, I, P, P, I, I, I, P, P, P, P, P, P, L, I, P]),
    # detection mask: boxcar (cube, pitch, mask_or_null, mask_pitch, out, pitch, C, M, filled_host, width,
    # blank, stream); reblank (work, pitch, cube, pitch, C, M, filled_host, stream); threshold (work,
    # pitch, mask, mask_pitch, C, P, H, W, filled_host, sigma, groups, threshold, polarity, stream);
    # prune (mask, mask_pitch, C, M, min_channels, stream); apply (cube, pitch, mask, mask_pitch, line,
    # pitch, C, M, filled_host, invert, stream)
    'kimg_cube_boxcar': (c_int, [P, L, P, L, P, L, I, L, P, I, I, P]),
    'kimg_cube_reblank': (c_int, [P, L, P, L, I, L, P, P]),
    'kimg_cube_threshold': (c_int, [P, L, P, L, I, I, I, I, P, P, I, F, I, P]),
    'kimg_cube_mask_prune': (c_int, [P, L, I, L, I, P]),
    'kimg_cube_mask_apply': (c_int, [P, L, P, L, P, L, I, L, P, I, P]),
    # source linking: scratch bytes (C, M); catalogue work bytes (capacity); link (mask, mask_pitch,
    # labels, label_pitch, C, P, H, W, filled_host, reach_xy_sq, reach_z, scratch, counts, stream);
    # measure (labels, label_pitch, cube, pitch, C, P, H, W, filled_host, kimg_catalogue *, capacity,
    # counts, stream); filter (labels, label_pitch, C, M, kimg_catalogue *, capacity, min_voxels,
    # min_size_xy, min_size_z, counts, stream); label mask (labels, label_pitch, mask, mask_pitch, C, M,
    # source, stream)
    'kimg_cube_link_scratch_bytes': (c_size_t, [I, L]),
    'kimg_cube_catalogue_work_bytes': (c_size_t, [I]),
    'kimg_cube_link': (c_int, [P, L, P, L, I, I, I, I, P, I, I, P, P, P]),
    'kimg_cube_measure': (c_int, [P, L, P, L, I, I, I, I, P, P, I, P, P]),
    'kimg_cube_link_filter': (c_int, [P, L, I, L, P, I, I, I, I, P, P]),
    'kimg_cube_label_mask': (c_int, [P, L, P, L, I, L, I, P]),
    # source spectra and lines: spectra (labels, label_pitch, cube, pitch, C, M, filled_host, N, c0,
    # offsets, total, sum, voxels, finite, stream); lines (N, c0, offsets, total, sum, finite, C, unit_host,
    # width_host, coord_host, variance_host, channel_tables, kimg_source_line_table *, stream)
    'kimg_cube_source_spectra': (c_int, [P, L, P, L, I, L, P, I, P, P, L, P, P, P, P]),
    'kimg_source_lines': (c_int, [I, P, P, L, P, P, I, P, P, P, P, P, P, P]),
    # per-source moment maps: workspace bytes (total); maps (labels, label_pitch, cube, pitch, C, P, H, W,
    # filled_host, x, N, rows, total, workspace, workspace_bytes, stream); finish (N, rows, total, workspace,
    # workspace_bytes, x, C, outputs, moment0, moment1, moment2, moment8, moment9, count, stream)
    'kimg_cube_source_maps_workspace_bytes': (c_size_t, [L]),
    'kimg_cube_source_maps': (c_int, [P, L, P, L, I, I, I, I, P, P, I, P, L, P, c_size_t, P]),
    'kimg_source_maps_finish': (c_int, [I, P, L, P, c_size_t, P, I, I, P, P, P, P, P, P, P]),
    # float64 path
    'kimg_grid_f64': (c_int, [P, L, L, I, I, P, L, L, P, P, P, L, P, I, I, I, P, c_size_t, I, P]),
    'kimg_degrid_f64': (c_int, [P, L, L, I, I, P, P, P, P, L, P, I, I, I, P, c_size_t, I, P]),
    'kimg_grid_to_layer_f64': (c_int, [P, I, P, L, I, P]),
    'kimg_layer_to_grid_f64': (c_int, [P, L, I, P, I, P]),
    'kimg_layer_to_image_f64': (c_int, [P, L, P, I, P, D, D, D, P]),
    'kimg_image_to_layer_f64': (c_int, [P, P, L, I, P, D, D, D, P]),
    'kimg_fft_plan_create_f64': (c_int, [ctypes.POINTER(c_void_p), I, I]),
    'kimg_scale_f64': (c_int, [P, L, L, I, I, I, ctypes.POINTER(c_double), P]),
    'kimg_add_image_f64': (c_int, [P, L, L, P, L, L, I, I, I, P]),
    'kimg_apply_primary_beam_f64': (c_int, [P, L, L, P, L, I, I, I, D, D, P]),
}


class CleanChannel(ctypes.Structure):
    """``kimg_clean_channel`` of include/kimg.h (one channel of kimg_clean_cycles_batch)."""
    _fields_ = [('dirty', c_void_p), ('model', c_void_p), ('psf', c_void_p),
                ('tile_max', c_void_p), ('tile_pos', c_void_p), ('state', c_void_p),
                ('log', c_void_p), ('patch_width', ctypes.c_int32),
                ('patch_height', ctypes.c_int32), ('threshold', c_float),
                ('max_cycles', ctypes.c_int32)]


CLEAN_BATCH_MAX = 8     # KIMG_CLEAN_BATCH_MAX
PRIMARY_BEAM_MAX_SAMPLES = 4096     # KIMG_PRIMARY_BEAM_MAX_SAMPLES


class UVTaper(ctypes.Structure):
    """``kimg_uv_taper`` of include/kimg.h (the taper of kimg_density_weights_taper)."""
    _fields_ = [('quad_uu', c_double), ('quad_uv', c_double), ('quad_vv', c_double),
                ('min_uv', c_double), ('max_uv', c_double),
                ('inner_tukey', c_double), ('outer_tukey', c_double)]


class Catalogue(ctypes.Structure):
    """``kimg_catalogue`` of include/kimg.h (the tables of kimg_cube_measure and kimg_cube_link_filter)."""
    _fields_ = [(name, c_void_p) for name in (
        'first', 'voxels', 'finite', 'c0', 'c1', 'y0', 'y1', 'x0', 'x1', 'peak', 'peak_index', 'trough',
        'trough_index', 'sum', 'sum_c', 'sum_y', 'sum_x', 'work')]


class SourceLineTable(ctypes.Structure):
    """``kimg_source_line_table`` of include/kimg.h (the rows of kimg_source_lines)."""
    _fields_ = [(name, c_void_p) for name in (
        'flux', 'flux_err', 'peak', 'peak_channel', 'centroid', 'w50', 'w20', 'w50_lo', 'w50_hi', 'w20_lo',
        'w20_hi', 'channels')]


class KimgLibraryError(RuntimeError):
    pass


class KimgError(RuntimeError):
    def __init__(self, code, what):
        super().__init__('{} failed: {} ({})'.format(what, error_string(code), code))
        self.code = code


_lib = None


_load_lock = threading.Lock()


def lib():
    """Load libkimg.so once; raise KimgLibraryError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:
        return _load()


def preload():
    """``kimg_preload`` (include/kimg.h): every code object of the library loaded on the current
    device now, in this thread -- before several threads make their first launches at once."""
    check(lib().kimg_preload(), 'kimg_preload')


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KimgLibraryError(
            'libkimg.so has not been built (run `python -m katsdpimager_amd.build`); '
            'katsdpimager_amd has no CPU fallback')
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 / librocfft first)
    except ImportError:
        pass
    try:
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:
        raise KimgLibraryError('cannot load {}: {}'.format(LIB_PATH, e)) from e
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise KimgLibraryError('libkimg.so lacks symbol ' + name) from e
        fn.restype = restype
        fn.argtypes = argtypes
    if handle.kimg_version() != VERSION:
        raise KimgLibraryError('libkimg.so version mismatch')
    _lib = handle
    return _lib


def error_string(code):
    return lib().kimg_error_string(code).decode()


def check(code, what):
    if code != 0:
        raise KimgError(code, what)
