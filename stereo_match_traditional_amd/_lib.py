"""ctypes binding of libsmt_hip.so (the C ABI in include/smt.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the import of
any compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMT_HIP_LIB") or os.path.join(_HERE, "lib", "libsmt_hip.so")  # override: A/B kernel builds

SMT_OK = 0
SMT_ERR_ARG = -1
SMT_ERR_DOMAIN = -4
SMT_ERR_REF_UB = -5
SMT_ERR_STATE = -6          # e.g. smt_scratch_poison outside arena mode
VIEW_LEFT, VIEW_RIGHT, VIEW_BOTH = 1, 2, 3
SMT_FILL_UB_LIST, SMT_FILL_UB_THIRD = 1, 2          # flags of smt_fill_the_hole_batch's status
QUIRK_FIX_RIGHT_ARM_STRIDE = 0x1
QUIRK_FIX_STICKY_TAU = 0x2
QUIRK_FIX_SCAN_VERTICAL = 0x4
QUIRK_FIX_CENSUS_RIGHT_EDGE = 0x8
QUIRK_FIX_ALL = 0xF
SAD_FORM_COMPOSED, SAD_FORM_BOX_KEYS, SAD_FORM_BOX_VOLUME = 1, 2, 3
NCC_FORM_LOOP, NCC_FORM_DOT4, NCC_FORM_BOX = 1, 2, 3
LRNCC_FORM_COMPOSED, LRNCC_FORM_KEYS = 1, 2
CBLSM_COST_LEFT, CBLSM_COST_RIGHT, CBLSM_COST_V4 = 1, 2, 3   # SMT_CBLSM_COST_* (smt_cblsm_window_cost_batch)
CBLSM_WINDOW_FORM_TAP, CBLSM_WINDOW_FORM_BOX = 1, 2          # smt_cblsm_window_last_form
NCC_WHOLE_FORM_LOOP, NCC_WHOLE_FORM_INT = 1, 2               # smt_whole_ncc_last_form
ASW_FIX_FILL_ROW_END = 0x1   # SMT_ASW_FIX_FILL_ROW_END (smt_fill_image_new_batch, smt_asw_post_params.fix)


class SmtError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: {strerror(status)} (status {status}, hip {last_hip_error()})")


class CrossArmParams(C.Structure):
    _fields_ = [("tau", C.c_int), ("tau_low", C.c_int), ("sec_length", C.c_int),
                ("max_length", C.c_int), ("chain_tau", C.c_int), ("quirks", C.c_uint)]


class PipelineParams(C.Structure):
    _fields_ = [("sigmaC", C.c_float), ("sigmaS", C.c_float), ("tao", C.c_int), ("p1", C.c_int), ("p2", C.c_int),
                ("gate", C.c_int)]


class CBLSMParams(C.Structure):
    """smt_cblsm_params: CBLSM.cpp:30-32's tao, secLength, maxLength."""
    _fields_ = [("tau", C.c_int), ("sec_length", C.c_int), ("max_length", C.c_int)]


class CrossAggFlowParams(C.Structure):
    """smt_crossagg_flow_params: adcensus_types.h:69-70's cross_L1, cross_L2, cross_t1, cross_t2, CBLSM.cpp:142's iteration
    count and :155's gate."""
    _fields_ = [("L1", C.c_int), ("L2", C.c_int), ("t1", C.c_int), ("t2", C.c_int), ("num_iters", C.c_int),
                ("gate", C.c_int)]


class ASWParams(C.Structure):
    """smt_asw_params: ASWeight.cpp:43-47's winSize, T, sigma_space, sigma_color."""
    _fields_ = [("winSize", C.c_int), ("T", C.c_int), ("sigma_space", C.c_double), ("sigma_color", C.c_double)]


class SADParams(C.Structure):
    """smt_sad_params: SADmain.cpp:34's winsize."""
    _fields_ = [("winsize", C.c_int)]


class NCCParams(C.Structure):
    """smt_ncc_params: NCC_main.cpp:17's winSize."""
    _fields_ = [("winSize", C.c_int)]


class NCCWholeParams(C.Structure):
    """smt_whole_ncc_params: NCC.h:121-122's kernel_size and max_offset, :117's add_constant."""
    _fields_ = [("kernel_size", C.c_int), ("max_offset", C.c_int), ("add_constant", C.c_int)]


class PostParams(C.Structure):
    """smt_post_params: main.cpp:93-94's RemoveSpeckles / MedianFilter arguments."""
    _fields_ = [("speckle_diff", C.c_int), ("speckle_min_area", C.c_uint), ("speckle_invalid", C.c_int),
                ("median_wnd", C.c_int)]


class CBLSMPostParams(C.Structure):
    """smt_cblsm_post_params: CBLSM.cpp:155's gate and :161-162's RemoveSpeckles / MedianFilter arguments."""
    _fields_ = [("gate", C.c_int), ("speckle_diff", C.c_int), ("speckle_min_area", C.c_uint),
                ("speckle_invalid", C.c_int), ("median_wnd", C.c_int)]


class ASWPostParams(C.Structure):
    """smt_asw_post_params: ASWeight.cpp:73-78's filterSpeckles / medianBlur arguments and the SMT_ASW_FIX_* flags."""
    _fields_ = [("speckle_newval", C.c_int), ("speckle_max_size", C.c_int), ("speckle_max_diff", C.c_int),
                ("median_first", C.c_int), ("median_last", C.c_int), ("fix", C.c_uint)]


class ADCensusOption(C.Structure):
    """struct ADCensusOption (CBLSM/adcensus_types.h:45-75)."""
    _fields_ = [("min_disparity", C.c_int32), ("max_disparity", C.c_int32), ("lambda_ad", C.c_int32),
                ("lambda_census", C.c_int32), ("cross_L1", C.c_int32), ("cross_L2", C.c_int32), ("cross_t1", C.c_int32),
                ("cross_t2", C.c_int32), ("so_p1", C.c_float), ("so_p2", C.c_float), ("so_tso", C.c_int32),
                ("irv_ts", C.c_int32), ("irv_th", C.c_float), ("lrcheck_thres", C.c_float), ("do_lr_check", C.c_int32),
                ("do_filling", C.c_int32), ("do_discontinuity_adjustment", C.c_int32)]


_lib = None


def _declare_ncc_flow(l):
    """The signatures of the NCC box form and smt_ncc_flow_* (include/smt.h); a library without them (an older build
    loaded through SMT_HIP_LIB for an A/B run) is left as it is."""
    if not hasattr(l, "smt_ncc_flow_run_batch"):
        return
    vp, i = C.c_void_p, C.c_int
    l.smt_ncc_box_set_band.argtypes = [i]
    l.smt_ncc_last_form.argtypes = []
    l.smt_ncc_selftest_box.argtypes = [i, i, i, i, C.c_uint]
    l.smt_ncc_default_params.argtypes = [C.POINTER(NCCParams)]
    l.smt_ncc_default_params.restype = None
    l.smt_ncc_flow_create_on.argtypes = [i, i, i, i, C.POINTER(NCCParams), C.POINTER(vp)]
    l.smt_ncc_flow_destroy.argtypes = [vp]
    l.smt_ncc_flow_set_stream.argtypes = [vp, vp]
    l.smt_ncc_flow_set_form.argtypes = [vp, i]
    l.smt_ncc_flow_run_batch.argtypes = [vp, vp, vp, i, vp, vp]
    if hasattr(l, "smt_lrncc"):                                # both views (csrc/ncc_both.hip)
        l.smt_lrncc.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, vp, vp]
        l.smt_lrncc_set_impl.argtypes = [i]
        l.smt_lrncc_last_form.argtypes = []
        l.smt_lrncc_selftest_keys.argtypes = [i, i, i, C.c_uint]
        l.smt_lrncc_flow_run_batch.argtypes = [vp, vp, vp, i, vp, vp, vp, vp]


def _declare_asw_tail(l):
    """The signatures of ASWeight.cpp's tail (include/smt.h); an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_asw_tail_batch"):
        return
    vp, i, z = C.c_void_p, C.c_int, C.c_size_t
    l.smt_minmax_normalize_u8_batch.argtypes = [vp, vp, i, z, i, i, vp]
    l.smt_minmax_normalize_f32_u8_batch.argtypes = [vp, vp, i, z, i, i, vp]
    l.smt_filter_speckles_u8_batch.argtypes = [vp, i, z, i, i, i, i, i, vp, vp]
    l.smt_median_blur_u8_batch.argtypes = [vp, vp, i, z, i, i, i, vp]
    l.smt_median_blur_selftest_nets.argtypes = []
    l.smt_fill_image_new_batch.argtypes = [vp, i, z, i, i, C.c_uint, vp, vp]
    l.smt_fill_image_new_host.argtypes = [vp, i, z, i, i, C.c_uint, vp]
    l.smt_asw_post_default_params.argtypes = [C.POINTER(ASWPostParams)]
    l.smt_asw_post_default_params.restype = None
    l.smt_asw_tail_batch.argtypes = [vp, i, z, i, i, C.POINTER(ASWPostParams), vp, vp, vp, vp, vp]
    l.smt_asw_flow_run_batch_post.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, C.POINTER(ASWPostParams), vp, vp, vp]
    l.smt_asw_flow_status.argtypes = [vp]


def _declare_cblsm_window(l):
    """The signatures of CBLSM's window cost volumes (include/smt.h); an older build loaded through SMT_HIP_LIB is left
    as it is."""
    if not hasattr(l, "smt_cblsm_window_cost_batch"):
        return
    vp, i, z = C.c_void_p, C.c_int, C.c_size_t
    l.smt_cblsm_window_cost_batch.argtypes = [vp, vp, i, z, i, i, i, i, i, vp, z, vp]
    l.smt_cblsm_window_cost_host.argtypes = [vp, vp, i, z, i, i, i, i, i, vp, z]
    l.smt_cblsm_window_set_impl.argtypes = [i]
    l.smt_cblsm_window_set_band.argtypes = [i]
    l.smt_cblsm_window_set_store.argtypes = [i]
    l.smt_cblsm_window_last_form.argtypes = []
    l.smt_cblsm_window_quotient.argtypes = [vp, z, i, vp, vp]
    l.smt_cblsm_selftest_window.argtypes = [i, i, i, i, i, C.c_uint]
    l.smt_cblsm_flow_run_batch_window.argtypes = [vp, vp, vp, i, i, vp, vp]


def _declare_ncc_whole(l):
    """The signatures of NCC.h's whole-image ncc() (include/smt.h); an older build loaded through SMT_HIP_LIB is left as
    it is."""
    if not hasattr(l, "smt_whole_ncc"):
        return
    vp, i = C.c_void_p, C.c_int
    pp = C.POINTER(NCCWholeParams)
    l.smt_whole_ncc_default_params.argtypes = [pp]
    l.smt_whole_ncc_default_params.restype = None
    l.smt_whole_ncc.argtypes = [vp, vp, i, i, pp, i, vp, vp, vp, vp]
    l.smt_whole_ncc_set_impl.argtypes = [i]
    l.smt_whole_ncc_last_form.argtypes = []
    l.smt_whole_ncc_set_groups.argtypes = [i]
    l.smt_whole_ncc_last_groups.argtypes = []
    l.smt_whole_ncc_selftest_box.argtypes = [i, i, i, i, i, C.c_uint]
    l.smt_bgr_to_grey_batch.argtypes = [vp, i, i, i, vp, vp]
    l.smt_whole_ncc_flow_create_on.argtypes = [i, i, i, pp, C.POINTER(vp)]
    l.smt_whole_ncc_flow_destroy.argtypes = [vp]
    l.smt_whole_ncc_flow_set_stream.argtypes = [vp, vp]
    l.smt_whole_ncc_flow_set_form.argtypes = [vp, i]
    l.smt_whole_ncc_flow_run_batch.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp]


class SubpixelParams(C.Structure):
    """smt_subpixel_params: the parabola rule's clamp (Sad.h:80's literal 1)."""
    _fields_ = [("min_den", C.c_float)]


def _declare_subpixel(l):
    """The signatures of the sub-pixel entry points (include/smt.h); an older build loaded through SMT_HIP_LIB is left
    as it is."""
    if not hasattr(l, "smt_wta_subpixel"):
        return
    vp, i = C.c_void_p, C.c_int
    pp = C.POINTER(SubpixelParams)
    l.smt_subpixel_default_params.argtypes = [pp]
    l.smt_subpixel_default_params.restype = None
    l.smt_wta_subpixel.argtypes = [vp, i, i, i, pp, vp, vp]
    l.smt_wta_subpixel_host.argtypes = [vp, i, i, i, pp, vp]
    for name in ("smt_scanline_set_subpixel", "smt_crossarm_set_subpixel", "smt_pipeline_set_subpixel"):
        getattr(l, name).argtypes = [vp, pp]


def _declare_sad_subpixel(l):
    """The signatures of include/smt_sad_subpixel.h; an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_sad_subpixel"):
        return
    vp, i = C.c_void_p, C.c_int
    pp = C.POINTER(SubpixelParams)
    l.smt_sad_subpixel.argtypes = [vp, vp, i, i, i, i, i, pp, vp, vp, vp]
    l.smt_sad_both_subpixel.argtypes = [vp, vp, i, i, i, i, pp, vp, vp, vp, vp, vp, vp]
    l.smt_sad_subpixel_host.argtypes = [vp, vp, i, i, i, i, pp, vp, vp, vp, vp]
    l.smt_sad_flow_run_batch_subpixel.argtypes = [vp, vp, vp, i, pp, vp, vp, vp, vp]


def _declare_scan_views(l):
    """The signatures of include/smt_scan_views.h; an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_scanline_run_pair"):
        return
    vp = C.c_void_p
    l.smt_scanline_run_pair.argtypes = [vp] * 9
    l.smt_scanline_run_map.argtypes = [vp] * 4
    l.smt_pipeline_set_scan_views.argtypes = [vp, C.c_int]
    l.smt_pipeline_scan_right_volume.argtypes = [vp, C.POINTER(vp)]


BILATERAL_NORM_RECIPROCAL, BILATERAL_NORM_DIVIDE = 0, 1      # SMT_BILATERAL_NORM_* (include/smt_bilateral.h)
BILATERAL_FORM_DIRECT, BILATERAL_FORM_STAGED = 1, 2          # smt_bilateral_set_impl / smt_bilateral_last_form


def _declare_bilateral(l):
    """The signatures of include/smt_bilateral.h; an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_bilateral_filter_batch"):
        return
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    l.smt_bilateral_masks.argtypes = [i, i, d, d, vp, vp]
    l.smt_bilateral_filter_batch.argtypes = [vp, i, i, i, i, i, i, vp, vp, i, vp, vp, vp]
    l.smt_bilateral_filter_host.argtypes = [vp, i, i, i, i, i, i, vp, vp, i, vp, vp]
    l.smt_bilateral_set_impl.argtypes = [i]
    l.smt_bilateral_last_form.argtypes = []


REFINE_ARM_CLAMPED = 1                                       # SMT_REFINE_ARM_CLAMPED (include/smt_refine.h)
REFINE_STATE_INTERPOLATED, REFINE_STATE_OUTLIER = 254, 255   # SMT_REFINE_STATE_*
REFINE_FORM_DIRECT, REFINE_FORM_WAVE = 1, 2                  # smt_refine_set_impl / smt_refine_last_form


class RefineParams(C.Structure):
    """smt_refine_params: irv_ts, irv_th (adcensus_types.h:58-59, 72), the iteration count and the ray length."""
    _fields_ = [("irv_ts", C.c_int), ("irv_th", C.c_float), ("irv_iters", C.c_int), ("search", C.c_int)]


def _declare_refine(l):
    """The signatures of include/smt_refine.h; an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_refine_batch"):
        return
    vp, i, z = C.c_void_p, C.c_int, C.c_size_t
    l.smt_refine_default_params.argtypes = [vp]
    l.smt_refine_default_params.restype = None
    vote = [vp, i, z, vp, vp, vp, vp, z, i, i, i, vp, vp, z, vp]
    interp = [vp, i, z, vp, z, vp, z, i, i, i, vp, vp, z, vp]
    both = [vp, i, z, vp, vp, vp, vp, z, vp, z, vp, z, i, i, i, vp, vp, z, vp]
    l.smt_region_vote_batch.argtypes = vote + [vp]
    l.smt_interpolate_outliers_batch.argtypes = interp + [vp]
    l.smt_refine_batch.argtypes = both + [vp]
    l.smt_region_vote_batch_host.argtypes = vote
    l.smt_interpolate_outliers_batch_host.argtypes = interp
    l.smt_refine_batch_host.argtypes = both
    l.smt_refine_set_impl.argtypes = [i]
    l.smt_refine_last_form.argtypes = []
    l.smt_pipeline_run_batch_refined.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]


FILLHOLES_UB_NAN = 1                                         # SMT_FILLHOLES_UB_NAN (include/smt_fill_holes.h)
FILLHOLES_MAX_DIM = 8192                                     # SMT_FILLHOLES_MAX_DIM


def _declare_fill_holes(l):
    """The signatures of include/smt_fill_holes.h; an older build loaded through SMT_HIP_LIB is left as it is."""
    if not hasattr(l, "smt_fill_holes_batch"):
        return
    vp, i, z, f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    l.smt_fill_holes_batch.argtypes = [vp, vp, i, z, z, i, i, f, vp, vp]
    l.smt_fill_holes_batch_host.argtypes = [vp, vp, i, z, z, i, i, f, vp]
    l.smt_fill_holes_constants.argtypes = [vp]
    l.smt_fill_holes_constants.restype = None
    l.smt_fill_holes_probe.argtypes = [i, i, i, i, C.POINTER(i), C.POINTER(i)]
    l.smt_fill_holes_walk.argtypes = [i, i, i, i, i, vp, vp, i]
    l.smt_fill_holes_host_passes.argtypes = [vp, vp, i, i, f, i]
    l.smt_pipeline_run_batch_filled.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, i, f, vp, vp]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -m stereo_match_traditional_amd.build` "
                "(hipcc, gfx950).  This package has no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _lib.smt_strerror.restype = C.c_char_p
        _declare_ncc_flow(_lib)
        _declare_asw_tail(_lib)
        _declare_cblsm_window(_lib)
        _declare_ncc_whole(_lib)
        _declare_subpixel(_lib)
        _declare_sad_subpixel(_lib)
        _declare_scan_views(_lib)
        _declare_bilateral(_lib)
        _declare_refine(_lib)
        _declare_fill_holes(_lib)
    return _lib


def strerror(status):
    return lib().smt_strerror(int(status)).decode()


def last_hip_error():
    return int(lib().smt_last_hip_error())


def check(status, what):
    if status != SMT_OK:
        raise SmtError(status, what)
