"""ctypes loader of libvwgpu.so (include/vwgpu.h).  Fails loudly: there is no CPU fallback in the product."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VWGPU_LIBRARY") or os.path.join(_HERE, "lib", "libvwgpu.so")  # override: experiments only
_LIB = None

SYMBOLS = [
    "vwgpu_abi_version", "vwgpu_create", "vwgpu_destroy", "vwgpu_set_stream", "vwgpu_reset_stream", "vwgpu_synchronize", "vwgpu_trim",
    "vwgpu_strerror", "vwgpu_last_error", "vwgpu_force_path", "vwgpu_last_path", "vwgpu_set_option", "vwgpu_get_option",
    "vwgpu_profile_enable", "vwgpu_profile_reset", "vwgpu_profile_read",
    "vwgpu_calc_disparity_dev", "vwgpu_calc_disparity", "vwgpu_fast_box_sum_dev", "vwgpu_fast_box_sum",
    "vwgpu_cross_corr_consistency_check_dev", "vwgpu_cross_corr_consistency_check",
    "vwgpu_cross_corr_consistency_check_diff_dev", "vwgpu_cross_corr_consistency_check_diff",
    "vwgpu_generate_gaussian_kernel",
    "vwgpu_separable_convolution_dev", "vwgpu_separable_convolution",
    "vwgpu_convolution_2d_dev", "vwgpu_convolution_2d",
    "vwgpu_subsample_mask_by_two_dev", "vwgpu_subsample_mask_by_two",
    "vwgpu_prefilter_image_dev", "vwgpu_prefilter_image",
    "vwgpu_parabola_subpixel_dev", "vwgpu_parabola_subpixel",
    "vwgpu_pyramid_subpixel_dev", "vwgpu_pyramid_subpixel",
    "vwgpu_phase_subpixel_dev", "vwgpu_phase_subpixel",
    "vwgpu_corr_eval_dev", "vwgpu_corr_eval",
    "vwgpu_disparity_median_filter_dev", "vwgpu_disparity_median_filter",
    "vwgpu_disparity_neighbor_filter_dev", "vwgpu_disparity_neighbor_filter",
    "vwgpu_texture_measure_dev", "vwgpu_texture_measure",
    "vwgpu_texture_preserving_disparity_filter_dev", "vwgpu_texture_preserving_disparity_filter",
    "vwgpu_rm_outliers_dev", "vwgpu_rm_outliers", "vwgpu_std_dev_image_dev", "vwgpu_std_dev_image",
    "vwgpu_get_disparity_range_dev", "vwgpu_get_disparity_range", "vwgpu_disparity_range_mask_dev", "vwgpu_disparity_range_mask",
    "vwgpu_transform_disparities_dev", "vwgpu_transform_disparities",
    "vwgpu_disparity_subsample_dev", "vwgpu_disparity_subsample", "vwgpu_disparity_upsample_dev", "vwgpu_disparity_upsample",
    "vwgpu_disparity_warp_dev", "vwgpu_disparity_warp", "vwgpu_missing_pixel_image_dev", "vwgpu_missing_pixel_image",
    "vwgpu_intersect_mask_and_data_dev", "vwgpu_intersect_mask_and_data",
    "vwgpu_grassfire_dev", "vwgpu_grassfire", "vwgpu_blob_index_dev", "vwgpu_blob_index", "vwgpu_blob_sizes_dev", "vwgpu_blob_sizes",
    "vwgpu_erode_blobs_dev", "vwgpu_erode_blobs", "vwgpu_inpaint_dev", "vwgpu_inpaint",
    "vwgpu_fill_holes_grass_dev", "vwgpu_fill_holes_grass", "vwgpu_fill_nodata_with_avg_dev", "vwgpu_fill_nodata_with_avg",
    "vwgpu_composite_create", "vwgpu_composite_destroy", "vwgpu_composite_insert_dev", "vwgpu_composite_insert",
    "vwgpu_composite_set_draft_mode", "vwgpu_composite_set_fill_holes", "vwgpu_composite_prepare", "vwgpu_composite_cols",
    "vwgpu_composite_rows", "vwgpu_composite_levels", "vwgpu_composite_bbox", "vwgpu_composite_mask",
    "vwgpu_composite_generate_patch_dev", "vwgpu_composite_generate_patch",
    "vwgpu_image_min_max_dev", "vwgpu_image_min_max", "vwgpu_image_moments_dev", "vwgpu_image_moments", "vwgpu_moments_mean",
    "vwgpu_moments_stddev", "vwgpu_image_histogram_dev", "vwgpu_image_histogram", "vwgpu_histogram_percentile",
    "vwgpu_otsu_from_histogram", "vwgpu_otsu_threshold_dev", "vwgpu_otsu_threshold",
    "vwgpu_image_order_statistic_dev", "vwgpu_image_order_statistic", "vwgpu_image_rescale_dev", "vwgpu_image_rescale",
    "vwgpu_percentile_scale_convert_dev", "vwgpu_percentile_scale_convert", "vwgpu_u8_convert_dev", "vwgpu_u8_convert",
    "vwgpu_auto_normalize_dev", "vwgpu_auto_normalize",
    "vwgpu_pinhole_camera", "vwgpu_stereo_triangulate_dev", "vwgpu_stereo_triangulate",
    "vwgpu_convergence_angle_dev", "vwgpu_convergence_angle", "vwgpu_universe_radius_dev", "vwgpu_universe_radius",
    "vwgpu_pinhole_camera_matrix", "vwgpu_epipolar_pinhole", "vwgpu_epipolar_cahv",
    "vwgpu_camera_transform_dev", "vwgpu_camera_transform", "vwgpu_camera_transform_points_dev", "vwgpu_camera_transform_points",
    "vwgpu_cahvor_camera", "vwgpu_cahvore_camera", "vwgpu_linearize_camera", "vwgpu_camera_set_lens", "vwgpu_lens_coordinates",
    "vwgpu_transform_make", "vwgpu_transform_rotate", "vwgpu_transform_invert", "vwgpu_transform_points",
    "vwgpu_transform_image_dev", "vwgpu_transform_image",
    "vwgpu_ip_match_chunk", "vwgpu_ip_match_dev", "vwgpu_ip_match", "vwgpu_host_last_error", "vwgpu_ip_remove_duplicates", "vwgpu_fit_transform", "vwgpu_ransac",
    "vwgpu_integral_image_dev", "vwgpu_integral_image", "vwgpu_ip_detect_dev", "vwgpu_ip_detect", "vwgpu_ip_orientation_dev", "vwgpu_ip_orientation",
    "vwgpu_ip_describe_dev", "vwgpu_ip_describe", "vwgpu_ip_cull_order",
    "vwgpu_disparity_filter_dev", "vwgpu_disparity_filter",
    "vwgpu_disparity_mask_dev", "vwgpu_disparity_mask",
    "vwgpu_subdivide_regions",
    "vwgpu_disparity_blob_filter_dev", "vwgpu_disparity_blob_filter",
    "vwgpu_pyramid_correlate_dev", "vwgpu_pyramid_correlate", "vwgpu_pyramid_correlate_batch_dev", "vwgpu_pyramid_correlate_batch",
    "vwgpu_calc_disparity_sgm_dev", "vwgpu_calc_disparity_sgm", "vwgpu_mgm_front_count", "vwgpu_mgm_front_pixel",
    "vwgpu_comm_unique_id", "vwgpu_comm_create", "vwgpu_comm_destroy", "vwgpu_halo_plan", "vwgpu_halo_headers_agree", "vwgpu_fetch_strip_window_dev",
]


class SgmParams(ctypes.Structure):
    """struct vwgpu_sgm_params (include/vwgpu.h)."""
    _fields_ = [
        ("cost_type", ctypes.c_int), ("use_mgm", ctypes.c_int), ("kernel_size", ctypes.c_int), ("subpixel_mode", ctypes.c_int),
        ("search_buffer_x", ctypes.c_int), ("search_buffer_y", ctypes.c_int), ("memory_limit_mb", ctypes.c_size_t),
        ("p1", ctypes.c_int), ("p2", ctypes.c_int), ("ternary_census_threshold", ctypes.c_int), ("num_threads", ctypes.c_int),
        ("allow_block_cost", ctypes.c_int),
    ]


class Camera(ctypes.Structure):
    """struct vwgpu_camera (include/vwgpu.h)."""
    _fields_ = [
        ("kind", ctypes.c_int), ("distortion_kind", ctypes.c_int), ("center", ctypes.c_double * 3),
        ("inv_camera_transform", ctypes.c_double * 9), ("pixel_pitch", ctypes.c_double),
        ("fu", ctypes.c_double), ("fv", ctypes.c_double), ("cu", ctypes.c_double), ("cv", ctypes.c_double),
        ("distortion", ctypes.c_double * 5), ("A", ctypes.c_double * 3), ("H", ctypes.c_double * 3), ("V", ctypes.c_double * 3),
    ]


class Transform(ctypes.Structure):
    """struct vwgpu_transform (include/vwgpu.h)."""
    _fields_ = [("kind", ctypes.c_int), ("reserved", ctypes.c_int), ("fwd", ctypes.c_double * 9), ("rev", ctypes.c_double * 9)]


class TransformParams(ctypes.Structure):
    """struct vwgpu_transform_params (include/vwgpu.h)."""
    _fields_ = [("interp", ctypes.c_int), ("edge", ctypes.c_int), ("edge_value", ctypes.c_float), ("edge_valid", ctypes.c_int),
                ("nodata", ctypes.c_int), ("nodata_value", ctypes.c_float), ("nodata_valid", ctypes.c_int)]


class IpMatchParams(ctypes.Structure):
    """struct vwgpu_ip_match_params (include/vwgpu.h)."""
    _fields_ = [("metric", ctypes.c_int), ("mode", ctypes.c_int), ("threshold", ctypes.c_double), ("constraint", ctypes.c_int),
                ("bidirectional", ctypes.c_int), ("bounds", ctypes.c_double * 4)]


class IpDetectParams(ctypes.Structure):
    """struct vwgpu_ip_detect_params (include/vwgpu.h)."""
    _fields_ = [("detector", ctypes.c_int), ("scales", ctypes.c_int), ("threshold", ctypes.c_double), ("max_points", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class IpPoints(ctypes.Structure):
    """struct vwgpu_ip_points (include/vwgpu.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("x", "y", "ix", "iy", "orientation", "scale", "interest")]


class ImageRange(ctypes.Structure):
    """struct vwgpu_image_range (include/vwgpu.h)."""
    _fields_ = [("min", ctypes.c_double), ("max", ctypes.c_double), ("count", ctypes.c_longlong), ("nan_count", ctypes.c_longlong)]


class TriangulateStats(ctypes.Structure):
    """struct vwgpu_triangulate_stats (include/vwgpu.h)."""
    _fields_ = [("point_count", ctypes.c_longlong), ("max_error", ctypes.c_double), ("sum_error", ctypes.c_double)]


class PyramidParams(ctypes.Structure):
    """struct vwgpu_pyramid_params (include/vwgpu.h)."""
    _fields_ = [
        ("prefilter_mode", ctypes.c_int), ("prefilter_width", ctypes.c_float),
        ("search_min_x", ctypes.c_int), ("search_min_y", ctypes.c_int),
        ("search_max_x", ctypes.c_int), ("search_max_y", ctypes.c_int),
        ("kernel_x", ctypes.c_int), ("kernel_y", ctypes.c_int),
        ("cost_type", ctypes.c_int), ("corr_timeout", ctypes.c_int), ("seconds_per_op", ctypes.c_double),
        ("consistency_threshold", ctypes.c_float), ("min_consistency_level", ctypes.c_int),
        ("filter_half_kernel", ctypes.c_int), ("max_pyramid_levels", ctypes.c_int),
        ("algorithm", ctypes.c_int), ("blob_filter_area", ctypes.c_int),
        ("sgm_subpixel_mode", ctypes.c_int), ("sgm_search_buffer_x", ctypes.c_int), ("sgm_search_buffer_y", ctypes.c_int),
        ("memory_limit_mb", ctypes.c_size_t), ("sgm_num_threads", ctypes.c_int),
        ("lr_disp_diff", ctypes.c_void_p), ("lr_disp_diff_cols", ctypes.c_int), ("lr_disp_diff_rows", ctypes.c_int),
        ("lr_disp_diff_stride", ctypes.c_ssize_t), ("region_ul_x", ctypes.c_int), ("region_ul_y", ctypes.c_int),
    ]


def build(force=False):
    """Compile every HIP translation unit for gfx950 into lib/libvwgpu.so (hipcc cross-compiles on CPU)."""
    args = ["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "visionworkbench_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback)" % LIB_PATH)
    # torch bundles its own libamdhip64.so.7; libvwgpu.so names the same SONAME (RUNPATH /opt/rocm).  Whichever
    # is loaded first serves both, and a process that ends up with two half-initialised HIP runtimes fails in
    # hipGetDeviceCount.  Import torch first so that torch tensors and our kernels share one runtime.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    P, I, F, PD = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_ssize_t
    lib.vwgpu_abi_version.restype = I
    lib.vwgpu_create.argtypes = [ctypes.POINTER(P), I]
    lib.vwgpu_destroy.argtypes = [P]
    lib.vwgpu_destroy.restype = None
    lib.vwgpu_set_stream.argtypes = [P, P]
    lib.vwgpu_reset_stream.argtypes = [P]
    lib.vwgpu_synchronize.argtypes = [P]
    lib.vwgpu_trim.argtypes = [P, ctypes.POINTER(ctypes.c_size_t)]
    lib.vwgpu_strerror.argtypes = [I]
    lib.vwgpu_strerror.restype = ctypes.c_char_p
    lib.vwgpu_last_error.argtypes = [P]
    lib.vwgpu_last_error.restype = ctypes.c_char_p
    lib.vwgpu_force_path.argtypes = [P, I]
    lib.vwgpu_last_path.argtypes = [P]
    lib.vwgpu_set_option.argtypes = [P, I, I]
    lib.vwgpu_get_option.argtypes = [P, I, ctypes.POINTER(ctypes.c_int)]
    lib.vwgpu_profile_enable.argtypes = [P, I]
    lib.vwgpu_profile_reset.argtypes = [P]
    lib.vwgpu_profile_read.argtypes = [P, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(F), I]
    bm = [P, I, P, I, I, PD, P, I, I, PD, I, I, I, I, P, PD]
    lib.vwgpu_calc_disparity_dev.argtypes = bm
    lib.vwgpu_calc_disparity.argtypes = bm
    IP = ctypes.POINTER(ctypes.c_int)
    lib.vwgpu_comm_unique_id.argtypes = [P]
    lib.vwgpu_comm_create.argtypes = [P, P, I, I, ctypes.POINTER(P)]
    lib.vwgpu_comm_destroy.argtypes = [P]
    lib.vwgpu_halo_plan.argtypes = [I, I, I, I, I, IP, IP, IP, IP]
    lib.vwgpu_halo_headers_agree.argtypes = [ctypes.POINTER(ctypes.c_longlong), I, IP, IP]
    lib.vwgpu_mgm_front_count.argtypes = [I, I, I]
    lib.vwgpu_mgm_front_pixel.argtypes = [I, I, I, I, I, P, P, IP]
    lib.vwgpu_fetch_strip_window_dev.argtypes = [P, P, P, I, I, I, I, I, P, IP]
    bs = [P, P, I, I, PD, I, I, P, PD]
    lib.vwgpu_fast_box_sum_dev.argtypes = bs
    lib.vwgpu_fast_box_sum.argtypes = bs
    lr = [P, P, I, I, PD, P, I, I, PD, F]
    lib.vwgpu_cross_corr_consistency_check_dev.argtypes = lr
    lib.vwgpu_cross_corr_consistency_check.argtypes = lr
    lrd = lr + [P, I, I, PD, I, I]
    lib.vwgpu_cross_corr_consistency_check_diff_dev.argtypes = lrd
    lib.vwgpu_cross_corr_consistency_check_diff.argtypes = lrd
    lib.vwgpu_generate_gaussian_kernel.argtypes = [ctypes.c_double, I, P, I]
    sc = [P, P, I, I, PD, P, I, I, P, I, I, I, I, P, PD]
    lib.vwgpu_separable_convolution_dev.argtypes = sc
    lib.vwgpu_separable_convolution.argtypes = sc
    c2 = [P, P, I, I, PD, P, I, I, I, I, I, P, PD]
    lib.vwgpu_convolution_2d_dev.argtypes = c2
    lib.vwgpu_convolution_2d.argtypes = c2
    mk = [P, P, I, I, PD, P, PD]
    lib.vwgpu_subsample_mask_by_two_dev.argtypes = mk
    lib.vwgpu_subsample_mask_by_two.argtypes = mk
    pf = [P, P, I, I, PD, I, F, P, PD]
    lib.vwgpu_prefilter_image_dev.argtypes = pf
    lib.vwgpu_prefilter_image.argtypes = pf
    ps = [P, P, I, I, PD, P, PD, P, I, I, PD, I, F, I, I, P, PD]
    lib.vwgpu_parabola_subpixel_dev.argtypes = ps
    lib.vwgpu_parabola_subpixel.argtypes = ps
    pys = [P, P, I, I, PD, P, PD, P, I, I, PD, I, F, I, I, I, I, P, I, P, PD, P]
    lib.vwgpu_pyramid_subpixel_dev.argtypes = pys
    lib.vwgpu_pyramid_subpixel.argtypes = pys
    phs = pys    # the same layout: phase_subpixel_accuracy where vwgpu_pyramid_subpixel takes algorithm
    lib.vwgpu_phase_subpixel_dev.argtypes = phs
    lib.vwgpu_phase_subpixel.argtypes = phs
    ce = [P, P, I, I, PD, P, P, PD, P, P, I, I, PD, I, I, I, I, I, I, F, P, I, P, PD, P]
    lib.vwgpu_corr_eval_dev.argtypes = ce
    lib.vwgpu_corr_eval.argtypes = ce
    D = ctypes.c_double
    med = [P, P, I, I, PD, I, I, P, I, P, PD, P]
    lib.vwgpu_disparity_median_filter_dev.argtypes = med
    lib.vwgpu_disparity_median_filter.argtypes = med
    nbf = [P, P, I, I, PD, I, P, I, P, PD, P]
    lib.vwgpu_disparity_neighbor_filter_dev.argtypes = nbf
    lib.vwgpu_disparity_neighbor_filter.argtypes = nbf
    txm = [P, P, I, I, PD, I, D, D, P, I, P, PD, P]
    lib.vwgpu_texture_measure_dev.argtypes = txm
    lib.vwgpu_texture_measure.argtypes = txm
    tpf = [P, P, I, I, PD, P, PD, F, I, I, P, I, P, PD, P]
    lib.vwgpu_texture_preserving_disparity_filter_dev.argtypes = tpf
    lib.vwgpu_texture_preserving_disparity_filter.argtypes = tpf
    rmo = [P, I, I, P, I, I, PD, I, I, D, D, I, I, P, PD, P]
    lib.vwgpu_rm_outliers_dev.argtypes = rmo
    lib.vwgpu_rm_outliers.argtypes = rmo
    sdi = [P, P, I, I, PD, I, I, I, P, PD]
    lib.vwgpu_std_dev_image_dev.argtypes = sdi
    lib.vwgpu_std_dev_image.argtypes = sdi
    lib.vwgpu_get_disparity_range_dev.argtypes = [P, I, P, I, I, PD, P, P]
    lib.vwgpu_get_disparity_range.argtypes = [P, I, P, I, I, PD, P]
    drm = [P, I, P, I, I, PD, I, I, P, P, I, P, PD, P]
    lib.vwgpu_disparity_range_mask_dev.argtypes = drm
    lib.vwgpu_disparity_range_mask.argtypes = drm
    trd = [P, I, P, I, I, PD, I, I, P, I, P, PD]
    lib.vwgpu_transform_disparities_dev.argtypes = trd
    lib.vwgpu_transform_disparities.argtypes = trd
    rsm = [P, I, P, I, I, PD, P, PD]
    for name in ("disparity_subsample", "disparity_upsample", "missing_pixel_image"):
        getattr(lib, "vwgpu_%s_dev" % name).argtypes = rsm
        getattr(lib, "vwgpu_%s" % name).argtypes = rsm
    dwp = [P, P, I, I, PD, P, I, I, PD, P, PD]
    lib.vwgpu_disparity_warp_dev.argtypes = dwp
    lib.vwgpu_disparity_warp.argtypes = dwp
    imd = [P, I, P, PD, P, PD, I, I, P, PD]
    lib.vwgpu_intersect_mask_and_data_dev.argtypes = imd
    lib.vwgpu_intersect_mask_and_data.argtypes = imd
    gfr = [P, I, P, I, I, PD, I, P, PD]
    lib.vwgpu_grassfire_dev.argtypes = gfr
    lib.vwgpu_grassfire.argtypes = gfr
    bix = [P, I, P, I, I, PD, I, I, I, P, PD, P, I, ctypes.POINTER(ctypes.c_int)]
    lib.vwgpu_blob_index_dev.argtypes = bix
    lib.vwgpu_blob_index.argtypes = bix
    bsz = [P, I, P, I, I, PD, ctypes.c_uint32, P, PD]
    lib.vwgpu_blob_sizes_dev.argtypes = bsz
    lib.vwgpu_blob_sizes.argtypes = bsz
    ero = [P, I, P, I, I, PD, I, P, PD]
    lib.vwgpu_erode_blobs_dev.argtypes = ero
    lib.vwgpu_erode_blobs.argtypes = ero
    inp = [P, I, P, I, I, PD, P, PD, P, I, I, P, I, I, P, PD]
    lib.vwgpu_inpaint_dev.argtypes = inp
    lib.vwgpu_inpaint.argtypes = inp
    fhg = [P, I, P, I, I, PD, I, I, P, PD]
    lib.vwgpu_fill_holes_grass_dev.argtypes = fhg
    lib.vwgpu_fill_holes_grass.argtypes = fhg
    fna = [P, P, I, I, PD, I, P, PD]
    lib.vwgpu_fill_nodata_with_avg_dev.argtypes = fna
    lib.vwgpu_fill_nodata_with_avg.argtypes = fna
    lib.vwgpu_composite_create.argtypes = [P, ctypes.POINTER(P)]
    lib.vwgpu_composite_destroy.argtypes = [P]
    lib.vwgpu_composite_destroy.restype = None
    cin = [P, P, P, I, I, PD, I, I, I]
    lib.vwgpu_composite_insert_dev.argtypes = cin
    lib.vwgpu_composite_insert.argtypes = cin
    lib.vwgpu_composite_set_draft_mode.argtypes = [P, P, I]
    lib.vwgpu_composite_set_fill_holes.argtypes = [P, P, I]
    lib.vwgpu_composite_prepare.argtypes = [P, P, ctypes.POINTER(ctypes.c_int)]
    lib.vwgpu_composite_cols.argtypes = [P]
    lib.vwgpu_composite_rows.argtypes = [P]
    lib.vwgpu_composite_levels.argtypes = [P]
    lib.vwgpu_composite_bbox.argtypes = [P, I, ctypes.POINTER(ctypes.c_int)]
    lib.vwgpu_composite_mask.argtypes = [P, P, I, P, PD]
    cgp = [P, P, I, I, I, I, P, PD]
    lib.vwgpu_composite_generate_patch_dev.argtypes = cgp
    lib.vwgpu_composite_generate_patch.argtypes = cgp
    img = [P, P, I, I, PD, P, PD]      # ctx, image, w, h, stride, mask, mask stride
    lib.vwgpu_image_min_max_dev.argtypes = img + [I, I, I, P, ctypes.POINTER(ImageRange)]
    lib.vwgpu_image_min_max.argtypes = img + [I, I, I, ctypes.POINTER(ImageRange)]
    lib.vwgpu_image_moments_dev.argtypes = img + [I, I, P, P]
    lib.vwgpu_image_moments.argtypes = img + [I, I, P]
    lib.vwgpu_moments_mean.argtypes = [P, ctypes.POINTER(D)]
    lib.vwgpu_moments_stddev.argtypes = [P, ctypes.POINTER(D)]
    ihs = img + [I, I, I, D, D, I, P, ctypes.POINTER(D)]
    lib.vwgpu_image_histogram_dev.argtypes = ihs
    lib.vwgpu_image_histogram.argtypes = ihs
    lib.vwgpu_histogram_percentile.argtypes = [P, I, ctypes.c_uint64, D, ctypes.POINTER(ctypes.c_int)]
    lib.vwgpu_otsu_from_histogram.argtypes = [P, I, ctypes.c_uint64, D, D, I, ctypes.POINTER(D)]
    ots = img + [I, I, I, I, ctypes.POINTER(D)]
    lib.vwgpu_otsu_threshold_dev.argtypes = ots
    lib.vwgpu_otsu_threshold.argtypes = ots
    lib.vwgpu_image_order_statistic_dev.argtypes = img + [I, D, P, ctypes.POINTER(D)]
    lib.vwgpu_image_order_statistic.argtypes = img + [I, D, ctypes.POINTER(D)]
    irs = [P, P, I, I, PD, I, P, I, P, PD]
    lib.vwgpu_image_rescale_dev.argtypes = irs
    lib.vwgpu_image_rescale.argtypes = irs
    psc = img + [D, D, I, I, P, PD, P]
    lib.vwgpu_percentile_scale_convert_dev.argtypes = psc
    lib.vwgpu_percentile_scale_convert.argtypes = psc
    u8c = img + [I, P, PD, P]
    lib.vwgpu_u8_convert_dev.argtypes = u8c
    lib.vwgpu_u8_convert.argtypes = u8c
    anm = img + [D, D, P, PD, P]
    lib.vwgpu_auto_normalize_dev.argtypes = anm
    lib.vwgpu_auto_normalize.argtypes = anm
    CP = ctypes.POINTER(Camera)
    lib.vwgpu_pinhole_camera.argtypes = [P, P, D, D, D, D, P, P, P, D, I, P, CP]
    tri = [P, I, P, I, I, PD, I, I, CP, CP, D, I, P, PD, P, PD, P, PD, P]
    lib.vwgpu_stereo_triangulate_dev.argtypes = tri
    lib.vwgpu_stereo_triangulate.argtypes = tri
    cva = [P, I, P, I, I, PD, I, I, CP, CP, I, P, PD]
    lib.vwgpu_convergence_angle_dev.argtypes = cva
    lib.vwgpu_convergence_angle.argtypes = cva
    unr = [P, P, I, I, I, PD, P, D, D, P, PD, P]
    lib.vwgpu_universe_radius_dev.argtypes = unr
    lib.vwgpu_universe_radius.argtypes = unr
    lib.vwgpu_pinhole_camera_matrix.argtypes = [P, P, D, D, D, D, P, P, P, D, I, P, P]
    lib.vwgpu_epipolar_pinhole.argtypes = [P, P, P, P, D, P, P, P, P, D, P, P, P, P]
    lib.vwgpu_epipolar_cahv.argtypes = [CP, CP, CP, CP]
    lib.vwgpu_cahvor_camera.argtypes = [P, P, P, P, P, P, CP]
    lib.vwgpu_cahvore_camera.argtypes = [P, P, P, P, P, P, P, I, D, CP]
    lib.vwgpu_linearize_camera.argtypes = [CP, I, I, I, I, CP]
    lib.vwgpu_camera_set_lens.argtypes = [CP, I, P, I]
    lib.vwgpu_lens_coordinates.argtypes = [CP, I, P, ctypes.c_longlong, P, P]
    ctr = [P, P, I, I, PD, P, PD, CP, P, CP, P, I, I, I, I, F, I, I, P, PD, P, PD, P]
    lib.vwgpu_camera_transform_dev.argtypes = ctr
    lib.vwgpu_camera_transform.argtypes = ctr
    ctp = [P, CP, P, CP, P, I, I, P, ctypes.c_longlong, P, P]
    lib.vwgpu_camera_transform_points_dev.argtypes = ctp
    lib.vwgpu_camera_transform_points.argtypes = ctp
    TP = ctypes.POINTER(Transform)
    lib.vwgpu_transform_make.argtypes = [I, P, I, TP]
    lib.vwgpu_transform_rotate.argtypes = [D, D, D, TP]
    lib.vwgpu_transform_invert.argtypes = [TP, TP]
    lib.vwgpu_transform_points.argtypes = [P, I, I, P, ctypes.c_longlong, P]
    tfi = [P, P, I, I, PD, P, PD, P, I, ctypes.POINTER(TransformParams), I, I, I, I, P, PD, P, PD]
    lib.vwgpu_transform_image_dev.argtypes = tfi
    lib.vwgpu_transform_image.argtypes = tfi
    lib.vwgpu_ip_match_chunk.argtypes = [I]
    ipm = [P, P, I, PD, P, I, PD, I, P, P, P, P, ctypes.POINTER(IpMatchParams), P, P, P]
    lib.vwgpu_ip_match_dev.argtypes = ipm
    lib.vwgpu_ip_match.argtypes = ipm
    lib.vwgpu_host_last_error.argtypes = []
    lib.vwgpu_host_last_error.restype = ctypes.c_char_p
    lib.vwgpu_ip_remove_duplicates.argtypes = [P, P, ctypes.c_longlong, P, P]
    lib.vwgpu_fit_transform.argtypes = [I, P, P, ctypes.c_longlong, P, P]
    lib.vwgpu_ransac.argtypes = [I, P, P, ctypes.c_longlong, P, I, D, I, I, P, P, P]
    itg = [P, P, I, I, PD, P, PD]
    lib.vwgpu_integral_image_dev.argtypes = itg
    lib.vwgpu_integral_image.argtypes = itg
    ipd = [P, P, I, I, PD, P, I, ctypes.POINTER(IpDetectParams), P, I, ctypes.POINTER(IpPoints), P]
    lib.vwgpu_ip_detect_dev.argtypes = ipd
    lib.vwgpu_ip_detect.argtypes = ipd
    ipo = [P, P, I, I, PD, I, P, P, P, P]
    lib.vwgpu_ip_orientation_dev.argtypes = ipo
    lib.vwgpu_ip_orientation.argtypes = ipo
    ips = [P, P, I, I, PD, P, I, P, P, P, P, I, P, PD]
    lib.vwgpu_ip_describe_dev.argtypes = ips
    lib.vwgpu_ip_describe.argtypes = ips
    lib.vwgpu_ip_cull_order.argtypes = [I, I, I, P, P, IP]
    df = [P, P, I, I, I, I, D, D, I, P]
    lib.vwgpu_disparity_filter_dev.argtypes = df
    lib.vwgpu_disparity_filter.argtypes = df
    dm = [P, P, I, I, P, P, I, I]
    lib.vwgpu_disparity_mask_dev.argtypes = dm
    lib.vwgpu_disparity_mask.argtypes = dm
    lib.vwgpu_subdivide_regions.argtypes = [P, I, I, I, I, P, I]
    lib.vwgpu_disparity_blob_filter_dev.argtypes = [P, P, I, I, I]
    lib.vwgpu_disparity_blob_filter.argtypes = [P, P, I, I, I]
    pc = [P, P, I, I, PD, P, I, I, PD, P, PD, P, PD, ctypes.POINTER(PyramidParams), I, I, I, I, P, PD]
    lib.vwgpu_pyramid_correlate_dev.argtypes = pc
    lib.vwgpu_pyramid_correlate.argtypes = pc
    pb = [P, P, I, I, PD, P, I, I, PD, P, PD, P, PD, ctypes.POINTER(PyramidParams), I, P, P, P, P, P, P]
    lib.vwgpu_pyramid_correlate_batch_dev.argtypes = pb
    lib.vwgpu_pyramid_correlate_batch.argtypes = pb
    IP = ctypes.POINTER(ctypes.c_int)
    sg = [P, ctypes.POINTER(SgmParams), P, I, I, PD, P, I, I, PD, I, I, P, I, I, P, I, I, P, I, I, P, P, ctypes.c_size_t, IP, IP]
    lib.vwgpu_calc_disparity_sgm_dev.argtypes = sg
    lib.vwgpu_calc_disparity_sgm.argtypes = sg
    for name in SYMBOLS:
        getattr(lib, name)  # AttributeError if the ABI and the header drifted apart
    _LIB = lib
    return lib
