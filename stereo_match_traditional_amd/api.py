"""Host-side mirrors of the reference's classes / free functions over the C ABI.

Names and argument meaning follow the reference (file:line cited per class); buffers are
torch CUDA(=HIP) tensors whose data_ptr() is handed to libsmt_hip.so.  Nothing here
computes on the CPU.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, lib, VIEW_LEFT, VIEW_RIGHT, VIEW_BOTH, SMT_FILL_UB_LIST, SMT_FILL_UB_THIRD  # noqa: F401
from ._lib import (QUIRK_FIX_RIGHT_ARM_STRIDE, QUIRK_FIX_STICKY_TAU, QUIRK_FIX_SCAN_VERTICAL,  # noqa: F401
                   QUIRK_FIX_CENSUS_RIGHT_EDGE, QUIRK_FIX_ALL)
from ._lib import NCC_FORM_LOOP, NCC_FORM_DOT4, NCC_FORM_BOX  # noqa: F401
from ._lib import LRNCC_FORM_COMPOSED, LRNCC_FORM_KEYS  # noqa: F401
from ._lib import ASW_FIX_FILL_ROW_END  # noqa: F401
from ._lib import NCC_WHOLE_FORM_LOOP, NCC_WHOLE_FORM_INT  # noqa: F401
from ._lib import BILATERAL_NORM_RECIPROCAL, BILATERAL_NORM_DIVIDE, BILATERAL_FORM_DIRECT, BILATERAL_FORM_STAGED  # noqa: F401
from ._lib import REFINE_ARM_CLAMPED, REFINE_STATE_INTERPOLATED, REFINE_STATE_OUTLIER, REFINE_FORM_DIRECT, REFINE_FORM_WAVE  # noqa: F401
from ._lib import FILLHOLES_UB_NAN, FILLHOLES_MAX_DIM  # noqa: F401
from ._lib import CBLSM_COST_LEFT, CBLSM_COST_RIGHT, CBLSM_COST_V4, CBLSM_WINDOW_FORM_TAP, CBLSM_WINDOW_FORM_BOX  # noqa: F401

__all__ = ["QUIRK_FIX_RIGHT_ARM_STRIDE", "QUIRK_FIX_STICKY_TAU", "QUIRK_FIX_SCAN_VERTICAL", "QUIRK_FIX_CENSUS_RIGHT_EDGE", "QUIRK_FIX_ALL", "MedianFilterInPlace", "median_inplace_set_impl", "CBLSMTail", "FillTheHole", "FillTheHoleBatch", "chooseArmLengthLeft", "chooseArmLengthRight", "chooseArmLengthUp", "chooseArmLengthDown", "costAggregationNew", "costAggregationV4", "AD_Census", "wta", "wta_subpixel", "GetPointDepthSubpixel", "GetPointDepthBothSubpixel", "current_stream_ptr", "CrossArmAggregation", "cblsm_ComputeAD",
           "ScanlineOptimizer", "LeftRightConsistency", "LeftAndRightConsistency", "CrossAggregator", "GetPointDepthLeft",
           "GetPointDepthRight", "sad_CrossCheckDiaparity", "NCC_algorithem", "ncc_set_impl", "sad_set_impl", "asw_masks",
           "AdaptiveSupportWeight", "sad_batch", "ncc_batch", "asw_batch", "asw_set_impl", "asw_CrossCheckDiaparity", "cvtColor_BGR2GRAY", "copyMakeBorder_replicate",
           "to_float", "MedianFilter", "RemoveSpeckles", "MedianFilterBatch", "RemoveSpecklesBatch", "imread", "imwrite", "ADCensusOption", "adcensus_option_aggregate", "Pipeline", "scratch_trim", "scratch_info", "scratch_poison",
           "ADCensusHostBatch", "CBLSMFlow", "AdaptiveSupportWeightBoth", "asw_both_set_impl", "ASWFlow",
           "GetPointDepthBoth", "sad_both_set_impl", "sad_both_set_dispatch", "sad_both_set_band", "sad_both_last_form", "SADFlow",
           "CrossAggFlow", "ncc_box_set_band", "ncc_last_form", "NCCFlow", "NCC_FORM_LOOP", "NCC_FORM_DOT4", "NCC_FORM_BOX",
           "NCC_both", "lrncc_set_impl", "lrncc_last_form", "LRNCC_FORM_COMPOSED", "LRNCC_FORM_KEYS",
           "ComputeDispLeft", "ComputeDispRight", "ComputeDispV4", "cblsm_window_set_impl", "cblsm_window_set_band",
           "cblsm_window_set_store", "cblsm_window_last_form", "CBLSM_WINDOW_FORM_TAP", "CBLSM_WINDOW_FORM_BOX",
           "ncc", "bgr_to_grey", "ncc_whole_set_impl", "ncc_whole_last_form", "ncc_whole_set_groups", "ncc_whole_last_groups", "NCCWholeFlow", "NCC_WHOLE_FORM_LOOP",
           "NCC_WHOLE_FORM_INT",
           "ASW_FIX_FILL_ROW_END", "MinMaxNormalizeU8", "FilterSpecklesU8", "MedianBlurU8", "FillImageNew", "ASWTail",
           "bilateralfiter", "bilateral_masks", "bilateral_set_impl", "bilateral_last_form", "BILATERAL_NORM_RECIPROCAL",
           "BILATERAL_NORM_DIVIDE", "BILATERAL_FORM_DIRECT", "BILATERAL_FORM_STAGED",
           "RegionVote", "InterpolateOutliers", "Refine", "refine_params", "refine_set_impl", "refine_last_form",
           "REFINE_ARM_CLAMPED", "REFINE_STATE_INTERPOLATED", "REFINE_STATE_OUTLIER", "REFINE_FORM_DIRECT",
           "REFINE_FORM_WAVE", "FillHolesInDispMap", "FILLHOLES_UB_NAN", "FILLHOLES_MAX_DIM"]


def current_stream_ptr(device=None):
    """torch's current stream on `device` (default: the current device) as a void*."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _on_tensor_device(f):
    """Stateless entry points launch on the current HIP device: make the device of the first tensor argument current
    for the call (a no-op on a one-GPU process), so that the kernels and the stream belong to the tensors' GPU."""
    import functools

    @functools.wraps(f)
    def g(*a, **kw):
        for t in list(a) + list(kw.values()):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                if t.device.index is not None and t.device.index != torch.cuda.current_device():
                    with torch.cuda.device(t.device):
                        return f(*a, **kw)
                break
        return f(*a, **kw)
    return g


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(t, dtype, shape=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a torch tensor on the GPU")
    if t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{name} must be contiguous {dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _dev_index(device):
    """HIP device ordinal of a torch device (cuda without an index = the current one)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"{device} is not a GPU")
    return torch.cuda.current_device() if device.index is None else int(device.index)


def _view_of(base_ptr, shape, dtype, device):
    """Zero-copy torch view of a library-owned device buffer (borrowed pointer)."""
    n = 1
    for s in shape:
        n *= s
    esz = torch.empty((), dtype=dtype).element_size()

    class _Holder:  # __cuda_array_interface__ provider
        pass

    h = _Holder()
    typestr = {torch.float32: "<f4", torch.int32: "<i4", torch.uint8: "|u1", torch.float64: "<f8"}[dtype]
    h.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(base_ptr), False),
                                  "version": 2, "strides": None}
    return torch.as_tensor(h, device=device)


class AD_Census:
    """class AD_Census (AD-CensusV1/AD-Census.h:9-43).

    Initialize(leftImage, rightImage, dispRange, row, col, LImage, RImage, sigmaC, sigmaS)
    -> here the images are bound at ComputeADcensus time and the two unused Mat
    arguments are dropped.
    """

    def __init__(self):
        self._h = None

    def Initialize(self, leftImage, rightImage, dispRange, row, col, sigmaC, sigmaS, placement_search=True, store_calibration=True,
                   quirks=0):
        """AD-Census.h:322-344.  placement_search / store_calibration = False skip the two measuring steps of
        smt_adcensus_create (smt_adcensus_create_ex flags): for handles created per request.  quirks: QUIRK_FIX_*
        (QUIRK_FIX_CENSUS_RIGHT_EDGE acts here), 0 = the reference's results."""
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self._L = _dev(leftImage, torch.float32, (row, col), "leftImage")
        self._R = _dev(rightImage, torch.float32, (row, col), "rightImage")
        self.device = leftImage.device
        h = C.c_void_p()
        if rightImage.device != self.device:
            raise ValueError("leftImage and rightImage live on different devices")
        flags = (0 if placement_search else 1) | (0 if store_calibration else 2)
        check(lib().smt_adcensus_create_ex(_dev_index(self.device), self.row, self.col, self.dispRange, C.c_float(sigmaC),
                                           C.c_float(sigmaS), C.c_uint(flags), C.byref(h)), "smt_adcensus_create_ex")
        self._h = h
        self._views = 0
        if quirks:
            self.set_quirks(quirks)
        return self

    def set_quirks(self, quirks):
        """QUIRK_FIX_* from the next Compute* on."""
        check(lib().smt_adcensus_set_quirks(self._h, C.c_uint(quirks)), "smt_adcensus_set_quirks")

    def _bind_stream(self):
        check(lib().smt_adcensus_set_stream(self._h, current_stream_ptr(self.device)), "smt_adcensus_set_stream")

    def _compute(self, views, dispL=None, dispR=None):
        self._bind_stream()
        check(lib().smt_adcensus_compute(self._h, _ptr(self._L), _ptr(self._R), views, _ptr(dispL),
                                         _ptr(dispR)), "smt_adcensus_compute")

    def ComputeADcensus(self):
        """AD-Census.h:271-294"""
        self._compute(VIEW_LEFT)

    def ComputeADcensusRight(self):
        """AD-Census.h:296-318"""
        self._compute(VIEW_RIGHT)

    def ComputeBoth(self, leftdisp=None, rightDisp=None):
        """ComputeADcensus + ComputeADcensusRight + WTA in one fused launch."""
        if leftdisp is not None:
            _dev(leftdisp, torch.float32, (self.row, self.col), "leftdisp")
            _dev(rightDisp, torch.float32, (self.row, self.col), "rightDisp")
        self._compute(VIEW_BOTH, leftdisp, rightDisp)

    def ComputeBatch(self, L, R, leftdisp, rightDisp, views=VIEW_BOTH):
        """[pairs][row][col] batches (smt_adcensus_compute_batch).  Afterwards the volumes hold the last pair's costs;
        with both views and D <= 256 the other pairs' volumes are never written (SMT_BATCH_VOLUMES=all writes them).
        There, until GetPtrLeft / GetPtrRight / WTA has been called once on this object, the last pair's volumes are
        written by the first such call after the batch, not by the batch; from then on every batch writes them itself
        (SMT_BATCH_VOLUMES=last: always)."""
        pairs = L.shape[0]
        _dev(L, torch.float32, (pairs, self.row, self.col), "L")
        _dev(R, torch.float32, (pairs, self.row, self.col), "R")
        _dev(leftdisp, torch.float32, (pairs, self.row, self.col), "leftdisp")
        _dev(rightDisp, torch.float32, (pairs, self.row, self.col), "rightDisp")
        self._bind_stream()
        check(lib().smt_adcensus_compute_batch(self._h, _ptr(L), _ptr(R), pairs, views, _ptr(leftdisp),
                                               _ptr(rightDisp)), "smt_adcensus_compute_batch")

    def WTA(self, leftdisp, rightDisp):
        """AD-Census.h:346-380 over the volumes already computed."""
        _dev(leftdisp, torch.float32, (self.row, self.col), "leftdisp")
        _dev(rightDisp, torch.float32, (self.row, self.col), "rightDisp")
        wta(self.GetPtrLeft(), leftdisp)
        wta(self.GetPtrRight(), rightDisp)

    def _vol(self, view):
        p = C.c_void_p()
        check(lib().smt_adcensus_volume(self._h, view, C.byref(p)), "smt_adcensus_volume")
        return _view_of(p.value, (self.row, self.col, self.dispRange), torch.float32, self.device)

    def GetPtrLeft(self):
        """AD-Census.h:50-60 (borrowed view of costVolume)."""
        return self._vol(VIEW_LEFT)

    def GetPtrRight(self):
        """AD-Census.h:62-72"""
        return self._vol(VIEW_RIGHT)

    def status(self):
        check(lib().smt_adcensus_status(self._h), "smt_adcensus_status")

    def force_generic(self, on=True):
        check(lib().smt_adcensus_force_generic(self._h, int(on)), "smt_adcensus_force_generic")

    def timing(self, enable=True):
        """False / 0: off.  True / 1: record HIP events around the kernels of every pair; N > 1: of every
        N-th pair (an event record costs about 3 us on the stream)."""
        check(lib().smt_adcensus_timing(self._h, int(enable)), "smt_adcensus_timing")

    def kernel_times(self):
        """(prep_ms[], cost_ms[]) of the pairs processed since timing(True); synchronises."""
        cap = 1024
        a = (C.c_float * cap)()
        b = (C.c_float * cap)()
        n = C.c_int()
        check(lib().smt_adcensus_kernel_times(self._h, a, b, cap, C.byref(n)), "smt_adcensus_kernel_times")
        return list(a[:n.value]), list(b[:n.value])

    def placement(self):
        """(candidate volume pairs tried at Initialize, store-only ms of the pair kept)."""
        n, ms = C.c_int(), C.c_float()
        check(lib().smt_adcensus_placement(self._h, C.byref(n), C.byref(ms)), "smt_adcensus_placement")
        return n.value, ms.value

    def store_mode(self):
        """(plain stores chosen?, calibration ms with streaming stores, with plain stores)."""
        pl, a, b = C.c_int(), C.c_float(), C.c_float()
        check(lib().smt_adcensus_store_mode(self._h, C.byref(pl), C.byref(a), C.byref(b)), "smt_adcensus_store_mode")
        return bool(pl.value), a.value, b.value

    def diag(self, reps=20):
        """smt_adcensus_diag: (in-kernel shader clock in MHz, stamped cost-kernel ms, store-only ms)."""
        self._bind_stream()
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        check(lib().smt_adcensus_diag(self._h, int(reps), C.byref(a), C.byref(b), C.byref(c)), "smt_adcensus_diag")
        return a.value, b.value, c.value

    def close(self):
        if self._h is not None:
            lib().smt_adcensus_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@_on_tensor_device
def wta(vol, disp=None):
    """First-strict-minimum argmin over d (CrossArm.cpp:33-57, ScanlineOptimizer.h:40-64,
    CBLSM.h:383-407)."""
    H, W, D = vol.shape
    _dev(vol, torch.float32, name="vol")
    if disp is None:
        disp = torch.empty((H, W), dtype=torch.float32, device=vol.device)
    _dev(disp, torch.float32, (H, W), "disp")
    check(lib().smt_wta(_ptr(vol), H, W, D, _ptr(disp), current_stream_ptr()), "smt_wta")
    return disp


def _subpixel_arg(min_den):
    """NULL (switch off) for None, else a pointer to smt_subpixel_params; the library checks the value"""
    return None if min_den is None else C.byref(_lib.SubpixelParams(float(min_den)))


@_on_tensor_device
def wta_subpixel(vol, min_den=1.0, disp=None):
    """wta() with the winner refined by the parabola through it and its two neighbours: the value Sad.h:76-81 and
    CBLSM.h:285-290 compute and drop.  min_den is the clamp of the denominator (the reference's literal 1; pass a small
    value for the true parabola on volumes of AD-Census magnitude).  A winner at either end of the range is kept."""
    H, W, D = vol.shape
    _dev(vol, torch.float32, name="vol")
    if disp is None:
        disp = torch.empty((H, W), dtype=torch.float32, device=vol.device)
    _dev(disp, torch.float32, (H, W), "disp")
    check(lib().smt_wta_subpixel(_ptr(vol), H, W, D, _subpixel_arg(min_den), _ptr(disp), current_stream_ptr()), "smt_wta_subpixel")
    return disp


# ======================================================================================
# CrossArmAggregation  (AD-CensusV1/CrossArm.h:9-36) + CBLSM.h arms / costAggregationV5
# ======================================================================================
class CrossArmAggregation:
    """Initialize(row, col, leftImage, rightImage, tao, dispRange) -- the two float image
    pointers are stored but never used by the reference (CrossArm.cpp:10-11) and are
    dropped here.  `style="cblsm"` selects the CBLSM.cpp:28-32 constants (tau=25, by-value
    threshold, no right-arm stride bug)."""

    def __init__(self):
        self._h = None

    def Initialize(self, row, col, tao, dispRange, device=None, style="adcensus", quirks=None,
                   sec_length=17, max_length=34, tau_low=6):
        """quirks: QUIRK_FIX_* (QUIRK_FIX_RIGHT_ARM_STRIDE and QUIRK_FIX_STICKY_TAU act here); None = the style's own
        (0, the reference's results, for "adcensus")."""
        self.close()
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.CrossArmParams()
        if style == "cblsm":
            lib().smt_crossarm_cblsm_params(C.byref(p))
        else:
            lib().smt_crossarm_default_params(C.byref(p))
        p.tau, p.tau_low, p.sec_length, p.max_length = int(tao), tau_low, sec_length, max_length
        if quirks is not None:
            p.quirks = quirks
        h = C.c_void_p()
        check(lib().smt_crossarm_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p), C.byref(h)),
              "smt_crossarm_create_on")
        self._h = h
        return self

    def _bind(self):
        check(lib().smt_crossarm_set_stream(self._h, current_stream_ptr(self.device)), "smt_crossarm_set_stream")

    def set_subpixel(self, min_den=None):
        """From the next aggregation on, the `disp` map carries the parabola's fraction (wta_subpixel's rule with this
        min_den); None = integer maps, the default."""
        check(lib().smt_crossarm_set_subpixel(self._h, _subpixel_arg(min_den)), "smt_crossarm_set_subpixel")

    def ComputeArmLengths(self, Image):
        """ComputeLeftArmLength, ComputeRightArmLength, ComputeTopArmLength,
        ComputeButtonArmLength (CrossArm.cpp:147-598) in main.cpp:69-72's order.
        Image: uint8 [row][col] or [row][col][3]."""
        ch = 1 if Image.dim() == 2 else int(Image.shape[2])
        _dev(Image, torch.uint8, (self.row, self.col) if ch == 1 else (self.row, self.col, ch), "Image")
        self._bind()
        check(lib().smt_crossarm_arms(self._h, _ptr(Image), ch), "smt_crossarm_arms")

    def Reset(self):
        """The state part of Initialize (CrossArm.cpp:13-17): `_tao = tao`, four zeroed maps."""
        self._bind()
        check(lib().smt_crossarm_reset(self._h), "smt_crossarm_reset")

    def _arm_dir(self, Image, dirn):
        ch = 1 if Image.dim() == 2 else int(Image.shape[2])
        _dev(Image, torch.uint8, (self.row, self.col) if ch == 1 else (self.row, self.col, ch), "Image")
        self._bind()
        check(lib().smt_crossarm_arm_dir(self._h, _ptr(Image), ch, dirn), "smt_crossarm_arm_dir")

    def ComputeLeftArmLength(self, Image):
        """CrossArm.cpp:147-260, with the sticky threshold as the previous call left it."""
        self._arm_dir(Image, 0)

    def ComputeRightArmLength(self, Image):
        """CrossArm.cpp:262-373 (`col = _row`, :265)."""
        self._arm_dir(Image, 1)

    def ComputeTopArmLength(self, Image):
        """CrossArm.cpp:375-486."""
        self._arm_dir(Image, 2)

    def ComputeButtonArmLength(self, Image):
        """CrossArm.cpp:488-598."""
        self._arm_dir(Image, 3)

    def tao(self):
        """Current value of the member `_tao` (CrossArm.h:34)."""
        t = C.c_int()
        check(lib().smt_crossarm_tau(self._h, C.byref(t)), "smt_crossarm_tau")
        return t.value

    def arm_maps(self):
        ps = [C.c_void_p() for _ in range(4)]
        check(lib().smt_crossarm_arm_maps(self._h, *[C.byref(p) for p in ps]), "smt_crossarm_arm_maps")
        return [_view_of(p.value, (self.row, self.col), torch.int32, self.device) for p in ps]

    def load_arm_maps(self, left, right, top, bottom):
        """Arm maps computed elsewhere (int32 [row][col] device tensors) become this handle's maps -- the shape of
        costAggregationV5(dispvolume, CostVolume, ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown, ...)."""
        for t, nm in zip((left, right, top, bottom), ("left", "right", "top", "bottom")):
            _dev(t, torch.int32, (self.row, self.col), nm)
        self._bind()
        check(lib().smt_crossarm_load_arm_maps(self._h, _ptr(left), _ptr(right), _ptr(top), _ptr(bottom)),
              "smt_crossarm_load_arm_maps")

    def _agg(self, dispVolume, aggregatedCostVolume, order, disp):
        shp = (self.row, self.col, self.dispRange)
        _dev(dispVolume, torch.float32, shp, "dispVolume")
        _dev(aggregatedCostVolume, torch.float32, shp, "aggregatedCostVolume")
        if disp is not None:
            _dev(disp, torch.float32, (self.row, self.col), "disp")
        self._bind()
        check(lib().smt_crossarm_aggregate(self._h, _ptr(dispVolume), _ptr(aggregatedCostVolume), order,
                                           _ptr(disp)), "smt_crossarm_aggregate")

    def AggregationVertical(self, dispVolume, aggregatedCostVolume, disp=None):
        """CrossArm.cpp:60-102 (+ fused WTA :33-57 when disp is given)."""
        self._agg(dispVolume, aggregatedCostVolume, 0, disp)

    def Aggregation(self, dispVolume, aggregatedCostVolume, disp=None):
        """CrossArm.cpp:104-145 (no call site in the reference): rows outer, exclusive upper bounds; empty
        rectangles give NaN and status() raises SMT_ERR_REF_UB."""
        self._agg(dispVolume, aggregatedCostVolume, 2, disp)

    def costAggregationV5(self, dispvolume, CostVolume, disp=None):
        """CBLSM.h:1179-1224 (row-major add order)."""
        self._agg(dispvolume, CostVolume, 1, disp)

    def WTA(self, AggredCostVolume, disp):
        wta(AggredCostVolume, disp)

    def set_variant(self, variant):
        """13 = 4x4 pixels per wave sharing union taps, lock-step workgroups, packed scalar word and fast quotient
        (default), 12 = the same kernel without the packed scalar word and the fast quotient, 7 = 12 with 2x8 tiles,
        6 = free-running, 4 / 5 / 3 = earlier shared-tap forms, 8-11 = flagged accumulate on the matrix pipe,
        0 = four pixels per wave, 1 plain walk, 2 pipelined walk (include/smt.h).  Also selects the variant's default
        strip width (8 from variant 7 on, else 16)."""
        check(lib().smt_crossarm_set_variant(self._h, int(variant)), "smt_crossarm_set_variant")

    def set_arm_walk(self, on=True):
        """Arms by the neighbour-by-neighbour kernels (independent formulation) instead of the bit-mask ones."""
        check(lib().smt_crossarm_set_arm_walk(self._h, int(on)), "smt_crossarm_set_arm_walk")

    def set_sweep(self, sweep):
        """Placement hook of variants 3-13: 0 = strips interleaved over the XCDs, 1 = one band of rows per XCD."""
        check(lib().smt_crossarm_set_sweep(self._h, int(sweep)), "smt_crossarm_set_sweep")

    def set_strip_width(self, w):
        """Placement hook: strip width, a multiple of 4 from 4 to 4096 (rounded per variant, include/smt.h)."""
        check(lib().smt_crossarm_set_strip_width(self._h, int(w)), "smt_crossarm_set_strip_width")

    def set_occupancy(self, waves_per_simd):
        """Aggregation waves per SIMD: 3, 4 or 5 (an LDS claim per workgroup), 0 = no limit (default)."""
        check(lib().smt_crossarm_set_occupancy(self._h, int(waves_per_simd)), "smt_crossarm_set_occupancy")

    def status(self):
        check(lib().smt_crossarm_status(self._h), "smt_crossarm_status")

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_crossarm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@_on_tensor_device
def cblsm_ComputeAD(L, R, dispRange, view=VIEW_LEFT, out=None):
    """CBLSM.h:327-353 (view left) / :355-381 (view right): uchar images -> float AD volume."""
    H, W = L.shape
    _dev(L, torch.uint8, (H, W), "L")
    _dev(R, torch.uint8, (H, W), "R")
    if out is None:
        out = torch.empty((H, W, dispRange), dtype=torch.float32, device=L.device)
    check(lib().smt_cblsm_ad(_ptr(L), _ptr(R), H, W, dispRange, view, _ptr(out), current_stream_ptr()),
          "smt_cblsm_ad")
    return out


@_on_tensor_device
def _choose_arm(dirn, own, vert, ArmRL, ArmRR, dispRange, Armvolume, row, col):
    for a in (own, vert, ArmRL, ArmRR):
        if a is not None:
            _dev(a, torch.int32, (row, col), "arm map")
    if Armvolume is None:
        Armvolume = torch.empty((row, col, dispRange), dtype=torch.int32, device=own.device)
    _dev(Armvolume, torch.int32, (row, col, dispRange), "Armvolume")
    check(lib().smt_cblsm_choose_arm_length(dirn, _ptr(own), _ptr(vert) if vert is not None else None, _ptr(ArmRL),
                                            _ptr(ArmRR), row, col, int(dispRange), _ptr(Armvolume),
                                            current_stream_ptr()), "smt_cblsm_choose_arm_length")
    return Armvolume


def chooseArmLengthLeft(ArmLL, ArmLR, ArmRL, ArmRR, dispRange, Armvolume, row, col):
    """CBLSM.h:65-102 (argument order of the reference; ArmLR is unused there too)."""
    return _choose_arm(0, ArmLL, None, ArmRL, ArmRR, dispRange, Armvolume, row, col)


def chooseArmLengthRight(ArmLL, ArmLR, ArmRL, ArmRR, dispRange, Armvolume, row, col):
    """CBLSM.h:104-147."""
    return _choose_arm(1, ArmLR, None, ArmRL, ArmRR, dispRange, Armvolume, row, col)


def chooseArmLengthUp(ArmLUp, ArmLDown, ArmRUp, ArmRDown, ArmRL, ArmRR, dispRange, Armvolume, row, col):
    """CBLSM.h:151-192."""
    return _choose_arm(2, ArmLUp, ArmRUp, ArmRL, ArmRR, dispRange, Armvolume, row, col)


def chooseArmLengthDown(ArmLUp, ArmLDown, ArmRUp, ArmRDown, ArmRL, ArmRR, dispRange, Armvolume, row, col):
    """CBLSM.h:195-236."""
    return _choose_arm(3, ArmLDown, ArmRDown, ArmRL, ArmRR, dispRange, Armvolume, row, col)


@_on_tensor_device
def costAggregationNew(leftImage, rightImage, CostVolume, ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown, dispRange,
                       _row_, _col_, winSize):
    """CBLSM.h:1087-1126 (argument order of the reference).  Padded uint8 images, int32 [row][col][D] arm
    volumes, float32 [row][col][D] CostVolume (allocated when None)."""
    w = winSize + 1
    _dev(leftImage, torch.uint8, (_row_ + 2 * w, _col_ + 2 * w), "leftImage")
    _dev(rightImage, torch.uint8, (_row_ + 2 * w, _col_ + 2 * w), "rightImage")
    for a in (ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown):
        _dev(a, torch.int32, (_row_, _col_, dispRange), "arm volume")
    if CostVolume is None:
        CostVolume = torch.empty((_row_, _col_, dispRange), dtype=torch.float32, device=leftImage.device)
    _dev(CostVolume, torch.float32, (_row_, _col_, dispRange), "CostVolume")
    check(lib().smt_cblsm_cost_aggregation_new(_ptr(leftImage), _ptr(rightImage), _row_, _col_, int(dispRange), int(winSize),
                                               _ptr(ArmvolumeL), _ptr(ArmvolumeR), _ptr(ArmvolumeUp), _ptr(ArmvolumeDown),
                                               _ptr(CostVolume), current_stream_ptr()), "smt_cblsm_cost_aggregation_new")
    return CostVolume


@_on_tensor_device
def costAggregationV4(dispvolume, CostVolume, ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown, dispRange, _row_, _col_,
                      winSize=0, disp=None, ub_flag=None):
    """CBLSM.h:1128-1176 (argument order of the reference; winSize is unused there too).  float32 [row][col][D] volume
    in, int32 [row][col][D] arm volumes, float32 CostVolume out (allocated when None); rectangles are half-open, an
    empty one gives NaN.  `disp`: optional float32 [row][col] that receives ComputeDispOringin of the result; `ub_flag`:
    optional int32 tensor of one element, ORed with 1 when a tap lies outside the plane."""
    shp = (_row_, _col_, int(dispRange))
    _dev(dispvolume, torch.float32, shp, "dispvolume")
    for a in (ArmvolumeL, ArmvolumeR, ArmvolumeUp, ArmvolumeDown):
        _dev(a, torch.int32, shp, "arm volume")
    if CostVolume is None:
        CostVolume = torch.empty(shp, dtype=torch.float32, device=dispvolume.device)
    _dev(CostVolume, torch.float32, shp, "CostVolume")
    if disp is not None:
        _dev(disp, torch.float32, (_row_, _col_), "disp")
    if ub_flag is not None:
        _dev(ub_flag, torch.int32, (1,), "ub_flag")
    check(lib().smt_cblsm_cost_aggregation_v4(_ptr(dispvolume), _ptr(ArmvolumeL), _ptr(ArmvolumeR), _ptr(ArmvolumeUp),
                                              _ptr(ArmvolumeDown), _row_, _col_, int(dispRange), _ptr(CostVolume),
                                              _ptr(disp) if disp is not None else None,
                                              _ptr(ub_flag) if ub_flag is not None else None, current_stream_ptr()),
          "smt_cblsm_cost_aggregation_v4")
    return CostVolume


@_on_tensor_device
def _window_cost(form, leftimg, rightimg, winsize, dispRange, out):
    w = int(winsize) + 1
    batched = leftimg.dim() == (4 if form == CBLSM_COST_V4 else 3)
    L, R = (leftimg, rightimg) if batched else (leftimg[None], rightimg[None])
    P, Hp, Wp = L.shape[0], L.shape[1], L.shape[2]
    H, W, D = Hp - 2 * w, Wp - 2 * w, int(dispRange)
    shp = (P, Hp, Wp, 3) if form == CBLSM_COST_V4 else (P, Hp, Wp)
    _dev(L, torch.uint8, shp, "leftimg")
    _dev(R, torch.uint8, shp, "rightimg")
    if H <= 0 or W <= 0:
        raise ValueError(f"padded images of {Hp} x {Wp} hold no pixel for winsize {winsize}")
    if out is None:
        out = torch.empty((P, H, W, D) if batched else (H, W, D), dtype=torch.float32, device=L.device)
    _dev(out, torch.float32, (P, H, W, D) if batched else (H, W, D), "dispVolume")
    check(lib().smt_cblsm_window_cost_batch(_ptr(L), _ptr(R), P, 0, H, W, D, int(winsize), form, _ptr(out), 0,
                                            current_stream_ptr()), "smt_cblsm_window_cost_batch")
    return out


def ComputeDispLeft(leftimg, rightimg, winsize, dispRange, out=None):
    """CBLSM.h:451-489: uint8 images replicate-padded by winsize + 1, [row + 2w][col + 2w] (or a batch of them) ->
    float32 window cost volume [row][col][dispRange] over the unpadded pixels (`out=` to fill a caller's)."""
    return _window_cost(CBLSM_COST_LEFT, leftimg, rightimg, winsize, dispRange, out)


def ComputeDispRight(leftimg, rightimg, winsize, dispRange, out=None):
    """CBLSM.h:409-447, with its early stop: the view ends winsize + 1 columns before its data does and the last
    columns of a row repeat one cost.  Raises (SMT_ERR_REF_UB) when col <= winsize + 1."""
    return _window_cost(CBLSM_COST_RIGHT, leftimg, rightimg, winsize, dispRange, out)


def ComputeDispV4(leftimg, rightimg, winsize, dispRange, out=None):
    """CBLSM.h:494-532: 3-channel padded images [row + 2w][col + 2w][3]; per tap the smallest channel difference, summed
    in a uchar, divided as an integer."""
    return _window_cost(CBLSM_COST_V4, leftimg, rightimg, winsize, dispRange, out)


def cblsm_window_set_impl(impl):
    """Test hook: 0 = the dispatch rule, 1 = the tap loop, 2 = the box kernel (gray forms)."""
    check(lib().smt_cblsm_window_set_impl(int(impl)), "smt_cblsm_window_set_impl")


def cblsm_window_set_band(band):
    """Test hook: rows per band of the box kernel's grid, 0 = its own choice."""
    check(lib().smt_cblsm_window_set_band(int(band)), "smt_cblsm_window_set_band")


def cblsm_window_set_store(mode):
    """Timing hook: 0 = the default, 1 = plain, 2 = non-temporal stores of the box kernel."""
    check(lib().smt_cblsm_window_set_store(int(mode)), "smt_cblsm_window_set_store")


def cblsm_window_last_form():
    """CBLSM_WINDOW_FORM_TAP or CBLSM_WINDOW_FORM_BOX: what the last window cost call ran."""
    return int(lib().smt_cblsm_window_last_form())


# ======================================================================================
# ScanlineOptimizer  (AD-CensusV1/ScanlineOptimizer.h:8-34)
# ======================================================================================
class ScanlineOptimizer:
    def __init__(self):
        self._h = None

    def Initialize(self, row, col, dispRange, p1, p2, device=None, quirks=0):
        """:66-79 (the costVolume pointer argument is re-passed to ScanLine anyway).  quirks: QUIRK_FIX_*
        (QUIRK_FIX_SCAN_VERTICAL acts here), 0 = the reference's results."""
        self.close()
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p()
        check(lib().smt_scanline_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, int(p1), int(p2), C.byref(h)),
              "smt_scanline_create_on")
        self._h = h
        self._processed = None
        if quirks:
            self.set_quirks(quirks)
        return self

    def set_quirks(self, quirks):
        """QUIRK_FIX_* from the next ScanLine / ScanPass on."""
        check(lib().smt_scanline_set_quirks(self._h, C.c_uint(quirks)), "smt_scanline_set_quirks")

    def set_subpixel(self, min_den=None):
        """From the next ScanLine on, its `disp` map carries the parabola's fraction (wta_subpixel's rule with this
        min_den); None = the integer map, the default."""
        check(lib().smt_scanline_set_subpixel(self._h, _subpixel_arg(min_den)), "smt_scanline_set_subpixel")

    def ScanLine(self, costVolume, Image, out=None, disp=None):
        """:104-128; returns `_ProcessedVolume`.  Image = float32 gray guidance."""
        shp = (self.row, self.col, self.dispRange)
        _dev(costVolume, torch.float32, shp, "costVolume")
        _dev(Image, torch.float32, (self.row, self.col), "Image")
        if out is None:
            out = torch.empty(shp, dtype=torch.float32, device=costVolume.device)
        _dev(out, torch.float32, shp, "out")
        check(lib().smt_scanline_set_stream(self._h, current_stream_ptr(self.device)), "smt_scanline_set_stream")
        check(lib().smt_scanline_run(self._h, _ptr(costVolume), _ptr(Image), _ptr(out), _ptr(disp)),
              "smt_scanline_run")
        self._processed = out
        return out

    def ScanLinePair(self, costL, ImageL, costR, ImageR, out=None, disp=None, maps_only=False):
        """ScanLine on two volumes of the handle's shape in the same launches (smt_scanline_run_pair): per view exactly
        what ScanLine gives.  out = (outL, outR) and disp = (dispL, dispR), entries may be None.  maps_only: True, or a
        pair of flags per view -- that view stores no volume (its `out` entry must be None) and needs its disp map.
        Without maps_only a missing `out` entry is allocated.  Returns (outL, outR, dispL, dispR), None for what a view
        does not produce."""
        shp = (self.row, self.col, self.dispRange)
        mo = (bool(maps_only),) * 2 if isinstance(maps_only, (bool, int)) else tuple(bool(m) for m in maps_only)
        out = list(out) if out is not None else [None, None]
        disp = list(disp) if disp is not None else [None, None]
        for v, (cost, img) in enumerate(((costL, ImageL), (costR, ImageR))):
            _dev(cost, torch.float32, shp, "cost" + "LR"[v])
            _dev(img, torch.float32, (self.row, self.col), "Image" + "LR"[v])
            if mo[v]:
                if out[v] is not None:
                    raise ValueError("a maps-only view takes no `out` volume")
                if disp[v] is None:
                    disp[v] = torch.empty((self.row, self.col), dtype=torch.float32, device=cost.device)
            elif out[v] is None:
                out[v] = torch.empty(shp, dtype=torch.float32, device=cost.device)
            if out[v] is not None:
                _dev(out[v], torch.float32, shp, "out" + "LR"[v])
            if disp[v] is not None:
                _dev(disp[v], torch.float32, (self.row, self.col), "disp" + "LR"[v])
        check(lib().smt_scanline_set_stream(self._h, current_stream_ptr(self.device)), "smt_scanline_set_stream")
        check(lib().smt_scanline_run_pair(self._h, _ptr(costL), _ptr(ImageL), _ptr(out[0]), _ptr(disp[0]),
                                          _ptr(costR), _ptr(ImageR), _ptr(out[1]), _ptr(disp[1])), "smt_scanline_run_pair")
        if out[0] is not None:
            self._processed = out[0]
        return out[0], out[1], disp[0], disp[1]

    def ScanLineMap(self, costVolume, Image, disp=None):
        """ScanLine + WTA with no volume returned (smt_scanline_run_map): the last pass stores the map only."""
        _dev(costVolume, torch.float32, (self.row, self.col, self.dispRange), "costVolume")
        _dev(Image, torch.float32, (self.row, self.col), "Image")
        if disp is None:
            disp = torch.empty((self.row, self.col), dtype=torch.float32, device=costVolume.device)
        _dev(disp, torch.float32, (self.row, self.col), "disp")
        check(lib().smt_scanline_set_stream(self._h, current_stream_ptr(self.device)), "smt_scanline_set_stream")
        check(lib().smt_scanline_run_map(self._h, _ptr(costVolume), _ptr(Image), _ptr(disp)), "smt_scanline_run_map")
        return disp

    def ScanPass(self, costVolume, Image, which):
        """One path volume: 'left' (ScanLineLeftRight isLeft=true, :130-192), 'right', 'up'
        (ScanLineUpDown isUp=true, :194-253), 'down'."""
        pass_id = {"left": 0, "right": 1, "up": 2, "down": 3}[which]
        out = torch.empty_like(costVolume)
        check(lib().smt_scanline_set_stream(self._h, current_stream_ptr(self.device)), "smt_scanline_set_stream")
        check(lib().smt_scanline_pass(self._h, _ptr(costVolume), _ptr(Image), pass_id, _ptr(out)),
              "smt_scanline_pass")
        return out

    def WTA(self, disp):
        """:40-64 over `_ProcessedVolume`."""
        wta(self._processed, disp)

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_scanline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ======================================================================================
# LeftRightConsistency  (AD-CensusV1/PostProcessing.h:72-135)
# ======================================================================================
@_on_tensor_device
def LeftRightConsistency(col, row, gate, leftDisp, rightDisp, want_lists=False):
    """In place on leftDisp (+inf = invalid).  Returns (cls uint8 [row][col], n_occlusion,
    n_mismatch[, occlusions, mismatches]); the lists are (row, col) pairs in the
    reference's row-major order."""
    _dev(leftDisp, torch.float32, (row, col), "leftDisp")
    _dev(rightDisp, torch.float32, (row, col), "rightDisp")
    cls = torch.empty((row, col), dtype=torch.uint8, device=leftDisp.device)
    counts = torch.zeros(2, dtype=torch.int32, device=leftDisp.device)
    check(lib().smt_lrcheck(_ptr(leftDisp), _ptr(rightDisp), row, col, int(gate), _ptr(cls), _ptr(counts),
                            current_stream_ptr()), "smt_lrcheck")
    n = counts.cpu().tolist()
    if not want_lists:
        return cls, n[0], n[1]
    import numpy as np
    ch = np.ascontiguousarray(cls.cpu().numpy())
    occ = np.empty((row * col, 2), np.int32)
    mis = np.empty((row * col, 2), np.int32)
    no, nm = C.c_int(), C.c_int()
    check(lib().smt_lrcheck_lists(ch.ctypes.data_as(C.c_void_p), row, col, occ.ctypes.data_as(C.c_void_p),
                                  C.byref(no), mis.ctypes.data_as(C.c_void_p), C.byref(nm)), "smt_lrcheck_lists")
    return cls, n[0], n[1], occ[:no.value], mis[:nm.value]


@_on_tensor_device
def LeftAndRightConsistency(leftDisp, rightDisp, lastDisp, col, row, gate):
    """PostProcessing.h:10-70 (argument order of the reference; no call site there): out of place, lastDisp
    receives the kept disparities and 0 for rejected pixels.  Returns (cls, n_occlusion, n_mismatch)."""
    _dev(leftDisp, torch.float32, (row, col), "leftDisp")
    _dev(rightDisp, torch.float32, (row, col), "rightDisp")
    _dev(lastDisp, torch.float32, (row, col), "lastDisp")
    cls = torch.empty((row, col), dtype=torch.uint8, device=leftDisp.device)
    counts = torch.zeros(2, dtype=torch.int32, device=leftDisp.device)
    check(lib().smt_lrcheck_variant(_ptr(leftDisp), _ptr(rightDisp), _ptr(lastDisp), row, col, C.c_float(gate),
                                    _ptr(cls), _ptr(counts), current_stream_ptr()), "smt_lrcheck_variant")
    n = counts.cpu().tolist()
    return cls, n[0], n[1]


@_on_tensor_device
def FillTheHole(row, col, dispRange, dispLeft, occlusion, mismatch):
    """PostProcessing.h:156-248, in place on the device map dispLeft ([row][col] float32; the
    reference's internal width/height swap is reproduced).  occlusion / mismatch: (first, second)
    pairs ([n, 2] int arrays or lists of pairs) in list order.  Returns the mismatch list as the
    reference leaves it: the third pass's pixels when that pass ran, else the input list."""
    import numpy as np
    _dev(dispLeft, torch.float32, (row, col), "dispLeft")
    occ = np.ascontiguousarray(np.asarray(occlusion, np.int32).reshape(-1, 2))
    mis = np.ascontiguousarray(np.asarray(mismatch, np.int32).reshape(-1, 2))
    third = np.empty((row * col, 2), np.int32)
    nt = C.c_int(-1)
    check(lib().smt_fill_the_hole(_ptr(dispLeft), row, col, int(dispRange), occ.ctypes.data_as(C.c_void_p),
                                  len(occ), mis.ctypes.data_as(C.c_void_p), len(mis),
                                  third.ctypes.data_as(C.c_void_p), C.byref(nt), current_stream_ptr()),
          "smt_fill_the_hole")
    return third[:nt.value].copy() if nt.value >= 0 else mis


@_on_tensor_device
def FillTheHoleBatch(maps, cls, dispRange, check=False):
    """FillTheHole (PostProcessing.h:156-248) on every map of [pairs][row][col] float32, in place, with the lists
    LeftRightConsistency would have produced taken from cls (uint8, same shape, as smt_lrcheck writes it) on the
    device: FillTheHole(row, col, dispRange, maps[b], *lists of cls[b]) for every b.  Asynchronous (enqueued on the
    current stream, nothing waits).  Returns the [pairs, 4] int32 status tensor {n_occ, n_mis, n_third, flags}; pairs
    on which the reference writes out of bounds are flagged (SMT_FILL_UB_LIST: untouched; SMT_FILL_UB_THIRD: passes 0
    and 1 only).  check=True synchronises and raises SmtError(SMT_ERR_REF_UB) naming the first flagged pair."""
    P, row, col, stride = _map_batch(maps, "maps")
    if not isinstance(cls, torch.Tensor) or not cls.is_cuda or cls.dtype != torch.uint8 or cls.device != maps.device:
        raise TypeError("cls must be a uint8 [pairs][row][col] tensor on the maps' GPU")
    if tuple(cls.shape) != (P, row, col):
        raise ValueError(f"cls has shape {tuple(cls.shape)}, expected {(P, row, col)}")
    if cls.stride(2) != 1 or (row > 1 and cls.stride(1) != col) or (P > 1 and cls.stride(0) < row * col):
        raise TypeError(f"cls: every map must be dense and the maps must not overlap (strides {cls.stride()})")
    cstride = cls.stride(0) if P > 1 else row * col
    status = torch.empty((P, 4), dtype=torch.int32, device=maps.device)
    if P == 0:
        return status
    _lib.check(lib().smt_fill_the_hole_batch(_ptr(maps), _ptr(cls), P, C.c_size_t(stride), C.c_size_t(cstride), row,
                                             col, int(dispRange), _ptr(status), current_stream_ptr()),
               "smt_fill_the_hole_batch")
    if check:
        flags = status[:, 3].cpu().tolist()
        for b, f in enumerate(flags):
            if f:
                raise _lib.SmtError(_lib.SMT_ERR_REF_UB, "smt_fill_the_hole_batch: pair %d, %s" % (
                    b, "list entry outside the buffer" if f & SMT_FILL_UB_LIST else "more holes than mismatches"))
    return status


@_on_tensor_device
def FillHolesInDispMap(maps, cls, invalid=float("inf"), check=False):
    """FillHolesInDispMap (SAD/Sad.h:317-400) on every map of [pairs][row][col] (or one [row][col]) float32, in place,
    with the occlusion and mismatch lists taken from cls (uint8, same shape, as smt_lrcheck writes it: 1 and 2): the
    filler for the +inf holes LeftRightConsistency leaves, which FillTheHole[Batch] (holes of 65535) does not see.
    invalid: the hole value.  Asynchronous (one launch on the current stream, nothing waits).  Returns the [pairs, 4]
    int32 status tensor {n_occ, n_mis, n_third, flags} ([4] for one map); a map that holds a NaN is not modified and
    flagged FILLHOLES_UB_NAN.  check=True synchronises and raises SmtError(SMT_ERR_REF_UB) naming the first flagged
    map."""
    single = isinstance(maps, torch.Tensor) and maps.dim() == 2
    m3 = maps[None] if single else maps
    P, row, col, stride = _map_batch(m3, "maps")
    c3, cstride = _plane_batch(cls, torch.uint8, P, row, col, "cls")
    if c3.device != m3.device:
        raise TypeError("cls must be on the maps' GPU")
    status = torch.empty((P, 4), dtype=torch.int32, device=m3.device)
    if P == 0:
        return status
    _lib.check(lib().smt_fill_holes_batch(_ptr(m3), _ptr(c3), P, C.c_size_t(stride), C.c_size_t(cstride), row, col,
                                          C.c_float(invalid), _ptr(status), current_stream_ptr()), "smt_fill_holes_batch")
    if check:
        for b, f in enumerate(status[:, 3].cpu().tolist()):
            if f:
                raise _lib.SmtError(_lib.SMT_ERR_REF_UB, "smt_fill_holes_batch: map %d holds a NaN" % b)
    return status[0] if single else status


# ======================================================================================
# CrossAggregator  (CBLSM/cross_aggregator.h:27-113)
# ======================================================================================
class CrossAggregator:
    def __init__(self):
        self._h = None

    def Initialize(self, width, height, min_disparity, max_disparity, device=None):
        """:19-58; returns False where the reference does."""
        self.close()
        self.width, self.height = int(width), int(height)
        self.disp_range = int(max_disparity) - int(min_disparity)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        h = C.c_void_p()
        rc = lib().smt_crossagg_create_on(_dev_index(self.device), self.width, self.height, self.disp_range, C.byref(h))
        if rc == -1:
            return False
        check(rc, "smt_crossagg_create")
        self._h = h
        return True

    def SetData(self, img_left, img_right, cost_init):
        """:60-65 (img_right is stored but never read by the reference)."""
        self._img = _dev(img_left, torch.uint8, (self.height, self.width, 3), "img_left")
        self._cost = _dev(cost_init, torch.float32, (self.height, self.width, self.disp_range), "cost_init")

    def SetParams(self, cross_L1, cross_L2, cross_t1, cross_t2):
        check(lib().smt_crossagg_set_params(self._h, int(cross_L1), int(cross_L2), int(cross_t1), int(cross_t2)),
              "smt_crossagg_set_params")

    def Aggregate(self, num_iters):
        """:89-118; silently does nothing when uninitialised, like the reference (:91-93)."""
        if self._h is None:
            return
        check(lib().smt_crossagg_set_stream(self._h, current_stream_ptr(self.device)), "smt_crossagg_set_stream")
        check(lib().smt_crossagg_aggregate(self._h, _ptr(self._img), _ptr(self._cost), int(num_iters)),
              "smt_crossagg_aggregate")

    def set_impl(self, impl):
        """2 = shared-tap passes (default), 1 = one pixel per wave (test hook)."""
        check(lib().smt_crossagg_set_impl(self._h, int(impl)), "smt_crossagg_set_impl")

    def get_cost_ptr(self):
        p = C.c_void_p()
        check(lib().smt_crossagg_cost(self._h, C.byref(p)), "smt_crossagg_cost")
        return _view_of(p.value, (self.height, self.width, self.disp_range), torch.float32, self.device)

    def get_arms_ptr(self):
        p = C.c_void_p()
        check(lib().smt_crossagg_arms(self._h, C.byref(p)), "smt_crossagg_arms")
        return _view_of(p.value, (self.height, self.width, 4), torch.uint8, self.device)

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_crossagg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ======================================================================================
# Window matchers  (SAD/Sad.h, NCC/NCC.h, ASW/ASW.h)
# ======================================================================================
def GetPointDepthLeft(leftimg, rightimg, MaxDisparity, winsize):
    """Sad.h:96-139.  leftimg/rightimg: uint8 replicate-padded by winsize+1."""
    return _sad(leftimg, rightimg, MaxDisparity, winsize, VIEW_LEFT)


def GetPointDepthRight(leftimg, rightimg, MaxDisparity, winsize):
    """Sad.h:141-182."""
    return _sad(leftimg, rightimg, MaxDisparity, winsize, VIEW_RIGHT)


@_on_tensor_device
def _sad(Lp, Rp, D, winsize, view):
    w = winsize + 1
    Hp, Wp = Lp.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    _dev(Lp, torch.uint8, (Hp, Wp), "leftimg")
    _dev(Rp, torch.uint8, (Hp, Wp), "rightimg")
    disp = torch.empty((H, W), dtype=torch.int32, device=Lp.device)
    check(lib().smt_sad(_ptr(Lp), _ptr(Rp), H, W, D, winsize, view, _ptr(disp), current_stream_ptr()), "smt_sad")
    return disp


@_on_tensor_device
def GetPointDepthBoth(leftimg, rightimg, MaxDisparity, winsize, want_cost=False):
    """smt_sad_both: SADmain.cpp:66-67's two views from one evaluation of the hypotheses.  uint8 images replicate-padded by
    winsize+1 -> (dispL, dispR) int32, or (dispL, dispR, costL) with want_cost (float32 [H][W][D], integer-valued)."""
    w = winsize + 1
    Hp, Wp = leftimg.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    _dev(leftimg, torch.uint8, (Hp, Wp), "leftimg")
    _dev(rightimg, torch.uint8, (Hp, Wp), "rightimg")
    dl = torch.empty((H, W), dtype=torch.int32, device=leftimg.device)
    dr = torch.empty_like(dl)
    cl = torch.empty((H, W, MaxDisparity), dtype=torch.float32, device=leftimg.device) if want_cost else None
    check(lib().smt_sad_both(_ptr(leftimg), _ptr(rightimg), H, W, MaxDisparity, winsize, _ptr(dl), _ptr(dr), _ptr(cl),
                             current_stream_ptr()), "smt_sad_both")
    return (dl, dr, cl) if want_cost else (dl, dr)


@_on_tensor_device
def GetPointDepthSubpixel(leftimg, rightimg, MaxDisparity, winsize, view=VIEW_LEFT, min_den=1.0, want_winner=False):
    """smt_sad_subpixel: one SAD view with the parabola of Sad.h:76-81 kept (include/smt_sad_subpixel.h).  uint8 images
    replicate-padded by winsize+1 -> disp float32 [H][W], or (disp, winner) with want_winner (int32: smt_sad's map).
    min_den None = the library's default."""
    w = winsize + 1
    Hp, Wp = leftimg.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    _dev(leftimg, torch.uint8, (Hp, Wp), "leftimg")
    _dev(rightimg, torch.uint8, (Hp, Wp), "rightimg")
    disp = torch.empty((H, W), dtype=torch.float32, device=leftimg.device)
    win = torch.empty((H, W), dtype=torch.int32, device=leftimg.device) if want_winner else None
    check(lib().smt_sad_subpixel(_ptr(leftimg), _ptr(rightimg), H, W, MaxDisparity, winsize, view, _subpixel_arg(min_den),
                                 _ptr(disp), _ptr(win), current_stream_ptr()), "smt_sad_subpixel")
    return (disp, win) if want_winner else disp


@_on_tensor_device
def GetPointDepthBothSubpixel(leftimg, rightimg, MaxDisparity, winsize, min_den=1.0, want_winner=False, want_cost=False):
    """smt_sad_both_subpixel: both sub-pixel SAD maps from one evaluation of the hypotheses, behind GetPointDepthBoth's
    hooks.  -> (dispL, dispR) float32, then (winL, winR) int32 with want_winner, then costL with want_cost."""
    w = winsize + 1
    Hp, Wp = leftimg.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    _dev(leftimg, torch.uint8, (Hp, Wp), "leftimg")
    _dev(rightimg, torch.uint8, (Hp, Wp), "rightimg")
    dl = torch.empty((H, W), dtype=torch.float32, device=leftimg.device)
    dr = torch.empty_like(dl)
    wl = torch.empty((H, W), dtype=torch.int32, device=leftimg.device) if want_winner else None
    wr = torch.empty_like(wl) if want_winner else None
    cl = torch.empty((H, W, MaxDisparity), dtype=torch.float32, device=leftimg.device) if want_cost else None
    check(lib().smt_sad_both_subpixel(_ptr(leftimg), _ptr(rightimg), H, W, MaxDisparity, winsize, _subpixel_arg(min_den),
                                      _ptr(dl), _ptr(dr), _ptr(wl), _ptr(wr), _ptr(cl), current_stream_ptr()),
          "smt_sad_both_subpixel")
    return (dl, dr) + ((wl, wr) if want_winner else ()) + ((cl,) if want_cost else ())


def sad_both_set_impl(impl):
    """2 = rank keys, no volume (default), 1 = left volume + diagonal-gather minimum (test hook)."""
    check(lib().smt_sad_both_set_impl(int(impl)), "smt_sad_both_set_impl")


def sad_both_set_dispatch(mode):
    """0 = the dispatch rule (default), 1 = the box kernel wherever it covers the window, 2 = smt_sad per view (test hook)."""
    check(lib().smt_sad_both_set_dispatch(int(mode)), "smt_sad_both_set_dispatch")


def sad_both_set_band(band):
    """Rows per band of the box kernel's grid, 0 = chosen from the image size (test hook)."""
    check(lib().smt_sad_both_set_band(int(band)), "smt_sad_both_set_band")


def sad_both_last_form():
    """What the last GetPointDepthBoth ran: _lib.SAD_FORM_COMPOSED / SAD_FORM_BOX_KEYS / SAD_FORM_BOX_VOLUME (test hook)."""
    return int(lib().smt_sad_both_last_form())


@_on_tensor_device
def sad_CrossCheckDiaparity(leftdisp, rightdisp):
    """Sad.h:184-222 -> (lastdisp int32, cls uint8)."""
    H, W = leftdisp.shape
    _dev(leftdisp, torch.int32, (H, W), "leftdisp")
    _dev(rightdisp, torch.int32, (H, W), "rightdisp")
    out = torch.empty_like(leftdisp)
    cls = torch.empty((H, W), dtype=torch.uint8, device=leftdisp.device)
    check(lib().smt_sad_crosscheck(_ptr(leftdisp), _ptr(rightdisp), H, W, _ptr(out), _ptr(cls),
                                   current_stream_ptr()), "smt_sad_crosscheck")
    return out, cls


@_on_tensor_device
def NCC_algorithem(leftImage, rigthImage, winSize, dispRange, want_cost=False):
    """NCC.h:69-95.  uint8 [H][W] unpadded images -> int32 disparity (argmax)."""
    H, W = leftImage.shape
    _dev(leftImage, torch.uint8, (H, W), "leftImage")
    _dev(rigthImage, torch.uint8, (H, W), "rigthImage")
    disp = torch.empty((H, W), dtype=torch.int32, device=leftImage.device)
    cost = torch.full((H, W, dispRange), float("nan"), dtype=torch.float64, device=leftImage.device) if want_cost else None
    check(lib().smt_ncc(_ptr(leftImage), _ptr(rigthImage), H, W, dispRange, winSize, _ptr(disp), _ptr(cost),
                        current_stream_ptr()), "smt_ncc")
    return (disp, cost) if want_cost else disp


@_on_tensor_device
def NCC_both(leftImage, rigthImage, winSize, dispRange, want_cost=False):
    """smt_lrncc: NCC.h:69-95 and its mirror from one pass over the costs.  uint8 [H][W] unpadded images -> (dispL, dispR)
    int32, or (dispL, dispR, costL, costR) with float64 [H][W][dispRange] costs.  dispR equals
    fliplr(NCC_algorithem(fliplr(R), fliplr(L)))."""
    H, W = leftImage.shape
    _dev(leftImage, torch.uint8, (H, W), "leftImage")
    _dev(rigthImage, torch.uint8, (H, W), "rigthImage")
    dl = torch.empty((H, W), dtype=torch.int32, device=leftImage.device)
    dr = torch.empty_like(dl)
    cl = torch.full((H, W, dispRange), float("nan"), dtype=torch.float64, device=leftImage.device) if want_cost else None
    cr = torch.full_like(cl, float("nan")) if want_cost else None
    check(lib().smt_lrncc(_ptr(leftImage), _ptr(rigthImage), H, W, dispRange, winSize, _ptr(dl), _ptr(dr), _ptr(cl), _ptr(cr),
                          current_stream_ptr()), "smt_lrncc")
    return (dl, dr, cl, cr) if want_cost else (dl, dr)


def lrncc_set_impl(impl):
    """Which form smt_lrncc and NCCFlow.run_both take: 0 = the dispatch rule (default), 1 = LRNCC_FORM_COMPOSED (mirrored
    single-view calls), 2 = LRNCC_FORM_KEYS wherever it exists (test hook)."""
    check(lib().smt_lrncc_set_impl(int(impl)), "smt_lrncc_set_impl")


def lrncc_last_form():
    """Which form the last both-view NCC call ran: LRNCC_FORM_COMPOSED or LRNCC_FORM_KEYS (0: none yet)."""
    return int(lib().smt_lrncc_last_form())


def _ncc_whole_params(kernel_size, max_offset, add_constant):
    p = _lib.NCCWholeParams()
    p.kernel_size, p.max_offset, p.add_constant = int(kernel_size), int(max_offset), int(bool(add_constant))
    return p


@_on_tensor_device
def ncc(in1, in2, type, add_constant=False, kernel_size=5, max_offset=79, want_offset=False, want_cost=False):
    """ncc() (NCC.h:117-272): uint8 [H][W] gray images, type "left" or "right" -> depth uint8 [H][W] = (uchar)(3 * offset) of
    the winner, every pixel written (0 where every offset's cost is NaN).  kernel_size and max_offset are the two values the
    reference fixes at 5 and 79.  want_offset adds the winning offset int32 [H][W] (0: none won), want_cost the costs
    float64 [H][W][max_offset], index offset - 1; the return value is depth, or a tuple in the order depth, offset, cost.
    add_constant works on a copy: in2 stays as it is.  want_cost is a diagnostic: the integer form stores the volume with a
    stride of max_offset doubles across lanes, 1.5 to 1.7 times the maps-only call at 450x375."""
    if type not in ("left", "right"):
        raise ValueError(f"type must be 'left' or 'right', not {type!r}")   # the reference returns an empty Mat
    H, W = in1.shape
    _dev(in1, torch.uint8, (H, W), "in1")
    _dev(in2, torch.uint8, (H, W), "in2")
    depth = torch.empty((H, W), dtype=torch.uint8, device=in1.device)
    off = torch.empty((H, W), dtype=torch.int32, device=in1.device) if want_offset else None
    cost = torch.full((H, W, int(max_offset)), float("nan"), dtype=torch.float64, device=in1.device) if want_cost else None
    p = _ncc_whole_params(kernel_size, max_offset, add_constant)
    check(lib().smt_whole_ncc(_ptr(in1), _ptr(in2), H, W, C.byref(p), VIEW_LEFT if type == "left" else VIEW_RIGHT, _ptr(depth),
                              _ptr(off), _ptr(cost), current_stream_ptr()), "smt_whole_ncc")
    out = (depth,) + ((off,) if want_offset else ()) + ((cost,) if want_cost else ())
    return out if len(out) > 1 else depth


@_on_tensor_device
def bgr_to_grey(bgr):
    """bgr_to_grey (NCC.h:97-115): uint8 [H][W][3] or [n][H][W][3] -> uint8 [H][W] or [n][H][W]; each channel is
    uchar(0.333 * v), truncated, then the three are added.  Not cvtColor_BGR2GRAY's rule."""
    single = bgr.dim() == 3
    b = bgr[None] if single else bgr
    n, H, W, ch = b.shape
    _dev(b, torch.uint8, (n, H, W, 3), "bgr")
    grey = torch.empty((n, H, W), dtype=torch.uint8, device=bgr.device)
    check(lib().smt_bgr_to_grey_batch(_ptr(b), n, H, W, _ptr(grey), current_stream_ptr()), "smt_bgr_to_grey_batch")
    return grey[0] if single else grey


def ncc_whole_set_impl(impl):
    """Which form ncc() and NCCWholeFlow take: 0 = the dispatch rule (default), 1 = NCC_WHOLE_FORM_LOOP (the reference's loop
    nest), 2 = NCC_WHOLE_FORM_INT wherever it exists, kernel_size <= 35 (test hook)."""
    check(lib().smt_whole_ncc_set_impl(int(impl)), "smt_whole_ncc_set_impl")


def ncc_whole_set_groups(groups):
    """Into how many runs a cost launch of ncc() / NCCWholeFlow splits the offsets; 0 = chosen from the grid (test hook: every
    value gives the same results)."""
    check(lib().smt_whole_ncc_set_groups(int(groups)), "smt_whole_ncc_set_groups")


def ncc_whole_last_groups():
    """Into how many runs the last ncc() / NCCWholeFlow call split the offsets (0: none yet)."""
    return int(lib().smt_whole_ncc_last_groups())


def ncc_whole_last_form():
    """Which form the last ncc() / NCCWholeFlow call ran: NCC_WHOLE_FORM_LOOP or NCC_WHOLE_FORM_INT (0: none yet)."""
    return int(lib().smt_whole_ncc_last_form())


def sad_set_impl(impl):
    """2 = LDS-staged SAD kernel (default), 1 = first formulation (test hook)."""
    check(lib().smt_sad_set_impl(int(impl)), "smt_sad_set_impl")


def ncc_set_impl(impl):
    """2 = window statistics + dot4 cross term (default, sides <= 31), 3 = window statistics + box-summed cross term (sides
    <= 181), 1 = the reference's loop nest (test hook)."""
    check(lib().smt_ncc_set_impl(int(impl)), "smt_ncc_set_impl")


def ncc_box_set_band(band):
    """Window rows per band of the NCC box kernel's grid; 0 = chosen from the image size (test hook)."""
    check(lib().smt_ncc_box_set_band(int(band)), "smt_ncc_box_set_band")


def ncc_last_form():
    """Which cost kernel the last NCC call launched: NCC_FORM_LOOP, NCC_FORM_DOT4 or NCC_FORM_BOX (0: none yet)."""
    return int(lib().smt_ncc_last_form())


def asw_masks(winSize, spaceSigma, colorSigma, device):
    """getGausssianMask (ASW.h:16-35) + getColorMask (:41-47), host float64 -> device tensors."""
    import numpy as np
    side = 2 * winSize + 3
    sp = np.empty((side, side), np.float64)
    cm = np.empty(256, np.float64)
    check(lib().smt_asw_masks(winSize, C.c_double(spaceSigma), C.c_double(colorSigma),
                              sp.ctypes.data_as(C.c_void_p), cm.ctypes.data_as(C.c_void_p)), "smt_asw_masks")
    return torch.from_numpy(sp).to(device), torch.from_numpy(cm).to(device)


def bilateral_masks(wsize, spaceSigma, colorSigma, device):
    """getGausssianMask (BiliteralFilter.h:12-31) + getColorMask (:36-43), host float64 -> device tensors.  wsize:
    (height, width) or one side; the space table is [height][width]."""
    import numpy as np
    h, w = (int(wsize), int(wsize)) if isinstance(wsize, int) else (int(wsize[0]), int(wsize[1]))
    if not (1 <= h <= 64 and 1 <= w <= 64):
        raise ValueError(f"wsize {wsize}: sides of 1..64 expected")
    sp = np.empty((h, w), np.float64)
    cm = np.empty(256, np.float64)
    check(lib().smt_bilateral_masks(h, w, C.c_double(spaceSigma), C.c_double(colorSigma),
                                    sp.ctypes.data_as(C.c_void_p), cm.ctypes.data_as(C.c_void_p)), "smt_bilateral_masks")
    return torch.from_numpy(sp).to(device), torch.from_numpy(cm).to(device)


_bilateral_tables = {}          # (h, w, spaceSigma, colorSigma, device) -> (space, color) on that device


def bilateral_set_impl(impl):
    """0 = the measured default, BILATERAL_FORM_DIRECT = one thread per pixel from global memory, BILATERAL_FORM_STAGED =
    the LDS-staged tile kernel (test hook)."""
    check(lib().smt_bilateral_set_impl(int(impl)), "smt_bilateral_set_impl")


def bilateral_last_form():
    """Which kernel the last bilateralfiter call launched: BILATERAL_FORM_DIRECT or BILATERAL_FORM_STAGED (0: none yet)."""
    return int(lib().smt_bilateral_last_form())


@_on_tensor_device
def bilateralfiter(src, wsize=(23, 23), spaceSigma=10, colorSigma=30, norm=BILATERAL_NORM_RECIPROCAL, return_acc=False,
                   tables=None):
    """BiliteralFilter.h:49-142 (smt_bilateral_filter_batch): the bilateral filter of uint8 images [H,W], [H,W,3], or
    with a leading images axis [n,H,W] (gray; a three-dimensional tensor whose last extent is 3 is one colour image, so
    a gray stack 3 pixels wide goes in as [n,H,3,1]), [n,H,W,1] or [n,H,W,3]; every channel on its own, replicate padding.
    wsize: (height, width) or one side, 1..64 (an even side acts as the odd side below it).  norm:
    BILATERAL_NORM_RECIPROCAL (the weights times 1 / their sum, what OpenCV 3.1's Mat / double evaluates) or
    BILATERAL_NORM_DIVIDE.  tables: (space, color) device float64 tensors instead of the cached ones of
    bilateral_masks.  -> the filtered images, shaped like src; with return_acc also the unclamped float64 sums."""
    h, w = (int(wsize), int(wsize)) if isinstance(wsize, int) else (int(wsize[0]), int(wsize[1]))
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype != torch.uint8 or not src.is_contiguous():
        raise TypeError("src must be a contiguous uint8 torch tensor on the GPU")
    if src.dim() == 2:
        n, (H, W), ch = 1, src.shape, 1
    elif src.dim() == 3 and src.shape[2] == 3:
        n, (H, W), ch = 1, src.shape[:2], 3
    elif src.dim() == 3:
        (n, H, W), ch = src.shape, 1
    elif src.dim() == 4 and src.shape[3] in (1, 3):
        n, H, W, ch = src.shape
    else:
        raise ValueError(f"src has shape {tuple(src.shape)}: [H,W], [H,W,3], [n,H,W], [n,H,W,1] or [n,H,W,3] expected")
    if tables is None:
        key = (h, w, float(spaceSigma), float(colorSigma), src.device)
        if key not in _bilateral_tables:
            _bilateral_tables[key] = bilateral_masks((h, w), spaceSigma, colorSigma, src.device)
        tables = _bilateral_tables[key]
    space, color = tables
    _dev(space, torch.float64, (h, w), "space")
    _dev(color, torch.float64, (256,), "color")
    dst = torch.empty_like(src)
    acc = torch.empty(src.shape, dtype=torch.float64, device=src.device) if return_acc else None
    check(lib().smt_bilateral_filter_batch(_ptr(src), int(n), int(H), int(W), int(ch), h, w, _ptr(space), _ptr(color), int(norm),
                                           _ptr(dst), _ptr(acc), current_stream_ptr()), "smt_bilateral_filter_batch")
    return (dst, acc) if return_acc else dst


@_on_tensor_device
def AdaptiveSupportWeight(leftGray, rightGray, winSize, dispRange, space, color, T, view=VIEW_LEFT, want_cost=False):
    """ASW.h:329-378 (view left) / :382-431 (view right).  Padded uint8 images."""
    wins = winSize + 1
    Hp, Wp = leftGray.shape
    H, W = Hp - 2 * wins, Wp - 2 * wins
    _dev(leftGray, torch.uint8, (Hp, Wp), "leftGray")
    _dev(rightGray, torch.uint8, (Hp, Wp), "rightGray")
    _dev(space, torch.float64, (2 * winSize + 3, 2 * winSize + 3), "space")
    _dev(color, torch.float64, (256,), "color")
    disp = torch.empty((H, W), dtype=torch.float32, device=leftGray.device)
    cost = torch.empty((H, W, dispRange), dtype=torch.float32, device=leftGray.device) if want_cost else None
    check(lib().smt_asw(_ptr(leftGray), _ptr(rightGray), H, W, dispRange, winSize, _ptr(space), _ptr(color), int(T),
                        view, _ptr(disp), _ptr(cost), current_stream_ptr()), "smt_asw")
    return (disp, cost) if want_cost else disp


@_on_tensor_device
def AdaptiveSupportWeightBoth(leftGray, rightGray, winSize, dispRange, space, color, T, want_cost=False):
    """smt_asw_both: ASWeight.cpp:60-61's two views from one evaluation of the hypotheses.  Padded uint8 images.
    -> (dispL, dispR), or (dispL, dispR, costL, costR) with want_cost."""
    wins = winSize + 1
    Hp, Wp = leftGray.shape
    H, W = Hp - 2 * wins, Wp - 2 * wins
    _dev(leftGray, torch.uint8, (Hp, Wp), "leftGray")
    _dev(rightGray, torch.uint8, (Hp, Wp), "rightGray")
    _dev(space, torch.float64, (2 * winSize + 3, 2 * winSize + 3), "space")
    _dev(color, torch.float64, (256,), "color")
    dl = torch.empty((H, W), dtype=torch.float32, device=leftGray.device)
    dr = torch.empty_like(dl)
    cl = torch.empty((H, W, dispRange), dtype=torch.float32, device=leftGray.device) if want_cost else None
    cr = torch.empty_like(cl) if want_cost else None
    check(lib().smt_asw_both(_ptr(leftGray), _ptr(rightGray), H, W, dispRange, winSize, _ptr(space), _ptr(color), int(T),
                             _ptr(dl), _ptr(dr), _ptr(cl), _ptr(cr), current_stream_ptr()), "smt_asw_both")
    return (dl, dr, cl, cr) if want_cost else (dl, dr)


def asw_both_set_impl(impl):
    """2 = rank keys, no volume (default), 1 = left volume + diagonal WinTakeAll (test hook; costR always comes from 1)."""
    check(lib().smt_asw_both_set_impl(int(impl)), "smt_asw_both_set_impl")


@_on_tensor_device
def sad_batch(leftimgs, rightimgs, MaxDisparity, winsize, view=VIEW_LEFT):
    """smt_sad_batch: [P, H+2w, W+2w] uint8 padded pairs -> int32 [P, H, W] (GetPointDepthLeft / Right per pair)."""
    w = winsize + 1
    P, Hp, Wp = leftimgs.shape
    H, W = Hp - 2 * w, Wp - 2 * w
    _dev(leftimgs, torch.uint8, (P, Hp, Wp), "leftimgs")
    _dev(rightimgs, torch.uint8, (P, Hp, Wp), "rightimgs")
    disp = torch.empty((P, H, W), dtype=torch.int32, device=leftimgs.device)
    check(lib().smt_sad_batch(_ptr(leftimgs), _ptr(rightimgs), P, C.c_size_t(0), H, W, MaxDisparity, winsize, view,
                              _ptr(disp), C.c_size_t(0), current_stream_ptr()), "smt_sad_batch")
    return disp


@_on_tensor_device
def ncc_batch(leftImages, rightImages, winSize, dispRange):
    """smt_ncc_batch: [P, H, W] uint8 pairs -> int32 [P, H, W] (NCC_algorithem per pair)."""
    P, H, W = leftImages.shape
    _dev(leftImages, torch.uint8, (P, H, W), "leftImages")
    _dev(rightImages, torch.uint8, (P, H, W), "rightImages")
    disp = torch.empty((P, H, W), dtype=torch.int32, device=leftImages.device)
    check(lib().smt_ncc_batch(_ptr(leftImages), _ptr(rightImages), P, C.c_size_t(0), H, W, dispRange, winSize, _ptr(disp),
                              C.c_size_t(0), current_stream_ptr()), "smt_ncc_batch")
    return disp


@_on_tensor_device
def asw_batch(leftGrays, rightGrays, winSize, dispRange, space, color, T, view=VIEW_LEFT):
    """smt_asw_batch: [P, H+2w, W+2w] uint8 padded pairs -> float32 [P, H, W] (AdaptiveSupportWeight per pair)."""
    wins = winSize + 1
    P, Hp, Wp = leftGrays.shape
    H, W = Hp - 2 * wins, Wp - 2 * wins
    _dev(leftGrays, torch.uint8, (P, Hp, Wp), "leftGrays")
    _dev(rightGrays, torch.uint8, (P, Hp, Wp), "rightGrays")
    _dev(space, torch.float64, (2 * winSize + 3, 2 * winSize + 3), "space")
    _dev(color, torch.float64, (256,), "color")
    disp = torch.empty((P, H, W), dtype=torch.float32, device=leftGrays.device)
    check(lib().smt_asw_batch(_ptr(leftGrays), _ptr(rightGrays), P, C.c_size_t(0), H, W, dispRange, winSize, _ptr(space),
                              _ptr(color), int(T), view, _ptr(disp), C.c_size_t(0), current_stream_ptr()), "smt_asw_batch")
    return disp


def asw_set_impl(impl):
    """0 = automatic (default: 3 up to a 6 GiB table, 6 beyond), 3 / 4 / 5 = whole-image anchor table variants, 6 = per-workgroup anchor slots, 1 = first formulation (test hook)."""
    check(lib().smt_asw_set_impl(int(impl)), "smt_asw_set_impl")


@_on_tensor_device
def asw_CrossCheckDiaparity(leftdisp, rightdisp):
    """ASW.h:108-145 -> uint8 map (0 = rejected)."""
    H, W = leftdisp.shape
    _dev(leftdisp, torch.float32, (H, W), "leftdisp")
    _dev(rightdisp, torch.float32, (H, W), "rightdisp")
    out = torch.empty((H, W), dtype=torch.uint8, device=leftdisp.device)
    check(lib().smt_asw_crosscheck(_ptr(leftdisp), _ptr(rightdisp), H, W, _ptr(out), current_stream_ptr()),
          "smt_asw_crosscheck")
    return out


# ======================================================================================
# Either side of the path: input staging and the first post-filter
# ======================================================================================
@_on_tensor_device
def cvtColor_BGR2GRAY(bgr):
    """cvtColor(img, gray, CV_BGR2GRAY) (main.cpp:19-20); uint8 [H][W][3] -> uint8 [H][W]."""
    H, W, _ = bgr.shape
    _dev(bgr, torch.uint8, (H, W, 3), "bgr")
    gray = torch.empty((H, W), dtype=torch.uint8, device=bgr.device)
    check(lib().smt_bgr2gray(_ptr(bgr), H, W, _ptr(gray), current_stream_ptr()), "smt_bgr2gray")
    return gray


@_on_tensor_device
def copyMakeBorder_replicate(img, pad):
    """copyMakeBorder(img, out, pad, pad, pad, pad, BORDER_REPLICATE) (SADmain.cpp:47-48)."""
    H, W = img.shape
    _dev(img, torch.uint8, (H, W), "img")
    out = torch.empty((H + 2 * pad, W + 2 * pad), dtype=torch.uint8, device=img.device)
    check(lib().smt_pad_replicate(_ptr(img), H, W, int(pad), _ptr(out), current_stream_ptr()), "smt_pad_replicate")
    return out


@_on_tensor_device
def to_float(img):
    """uchar -> float copy of main.cpp:46-55."""
    H, W = img.shape
    _dev(img, torch.uint8, (H, W), "img")
    out = torch.empty((H, W), dtype=torch.float32, device=img.device)
    check(lib().smt_u8_to_f32(_ptr(img), H, W, _ptr(out), current_stream_ptr()), "smt_u8_to_f32")
    return out


@_on_tensor_device
def MedianFilter(inp, width, height, wnd_size):
    """PostProcessing.h:314-344."""
    _dev(inp, torch.float32, (height, width), "in")
    out = torch.empty_like(inp)
    check(lib().smt_median_filter(_ptr(inp), _ptr(out), width, height, int(wnd_size), current_stream_ptr()),
          "smt_median_filter")
    return out


@_on_tensor_device
def RemoveSpeckles(disparity_map, width, height, diff_insame, min_speckle_aera, invalid_val):
    """PostProcessing.h:250-311, in place.  invalid_val: int, as in the reference's signature."""
    _dev(disparity_map, torch.float32, (height, width), "disparity_map")
    check(lib().smt_remove_speckles(_ptr(disparity_map), width, height, int(diff_insame), C.c_uint(min_speckle_aera),
                                    int(invalid_val), current_stream_ptr()), "smt_remove_speckles")
    return disparity_map


def _map_batch(maps, name):
    """[P][H][W] float32 maps on the GPU, each map dense, consecutive maps stride(0) >= H*W elements apart."""
    if not isinstance(maps, torch.Tensor) or not maps.is_cuda or maps.dtype != torch.float32 or maps.dim() != 3:
        raise TypeError(f"{name} must be a float32 [pairs][H][W] tensor on the GPU")
    P, H, W = maps.shape
    if maps.stride(2) != 1 or (H > 1 and maps.stride(1) != W) or (P > 1 and maps.stride(0) < H * W):
        raise TypeError(f"{name}: every map must be dense and the maps must not overlap (strides {maps.stride()})")
    return P, H, W, (maps.stride(0) if P > 1 else H * W)


@_on_tensor_device
def MedianFilterBatch(maps, wnd_size):
    """MedianFilter (PostProcessing.h:314-344) on every map of [pairs][H][W], one launch -> new dense [pairs][H][W]."""
    P, H, W, stride = _map_batch(maps, "maps")
    src = maps if stride == H * W else maps.contiguous()
    out = torch.empty((P, H, W), dtype=torch.float32, device=maps.device)
    check(lib().smt_median_filter_batch(_ptr(src), _ptr(out), P, C.c_size_t(0), W, H, int(wnd_size),
                                        current_stream_ptr()), "smt_median_filter_batch")
    return out


@_on_tensor_device
def RemoveSpecklesBatch(maps, diff_insame, min_speckle_aera, invalid_val):
    """RemoveSpeckles (PostProcessing.h:250-311) on every map of [pairs][H][W], in place, asynchronous (enqueued on
    the current stream, nothing waits).  Consecutive maps may lie further apart than H*W (stride(0))."""
    P, H, W, stride = _map_batch(maps, "maps")
    check(lib().smt_remove_speckles_batch(_ptr(maps), P, C.c_size_t(stride), W, H, int(diff_insame),
                                          C.c_uint(min_speckle_aera), int(invalid_val), None, current_stream_ptr()),
          "smt_remove_speckles_batch")
    return maps


# ---- region voting and outlier interpolation (include/smt_refine.h; parity unpinned: no reference code) ----------------
def refine_params(option=None, **overrides):
    """smt_refine_params: the defaults (irv_ts 20, irv_th 0.4, irv_iters 5, search 0), irv_ts and irv_th taken from an
    ADCensusOption when one is given (adcensus_types.h:58-59), then the keywords."""
    p = _lib.RefineParams()
    lib().smt_refine_default_params(C.byref(p))
    if option is not None:
        p.irv_ts, p.irv_th = int(option.irv_ts), float(option.irv_th)
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def refine_set_impl(impl):
    """0 = the default, REFINE_FORM_DIRECT = one thread per pixel, REFINE_FORM_WAVE = one wave per outlier: the voting
    formulation, identical bits (test hook)."""
    check(lib().smt_refine_set_impl(int(impl)), "smt_refine_set_impl")


def refine_last_form():
    """Which voting kernel the last call launched: REFINE_FORM_DIRECT or REFINE_FORM_WAVE (0: none yet)."""
    return int(lib().smt_refine_last_form())


def _plane_batch(t, dtype, P, H, W, name):
    """[P][H][W] (or [H][W] when P == 1) planes on the GPU, each dense -> (tensor, stride between planes in elements)."""
    t3 = t[None] if isinstance(t, torch.Tensor) and t.dim() == 2 else t
    if not isinstance(t3, torch.Tensor) or not t3.is_cuda or t3.dtype != dtype or t3.dim() != 3:
        raise TypeError(f"{name} must be a {dtype} [pairs][H][W] tensor on the GPU")
    if tuple(t3.shape) != (P, H, W):
        raise ValueError(f"{name} has shape {tuple(t3.shape)}, expected {(P, H, W)}")
    if t3.stride(2) != 1 or (H > 1 and t3.stride(1) != W) or (P > 1 and t3.stride(0) < H * W):
        raise TypeError(f"{name}: every plane must be dense and the planes must not overlap (strides {t3.stride()})")
    return t3, (t3.stride(0) if P > 1 else H * W)


def _refine_call(maps, arms, cls, gray, D, params, want_state, kw):
    m3 = maps[None] if isinstance(maps, torch.Tensor) and maps.dim() == 2 else maps
    P, H, W, stride = _map_batch(m3, "maps")
    p = params if params is not None else refine_params(**kw)
    if params is not None and kw:
        raise TypeError("give params or keywords, not both")
    state = torch.empty((P, H, W), dtype=torch.uint8, device=maps.device) if want_state else None
    status = torch.zeros((P, 4), dtype=torch.int32, device=maps.device)
    z, st = C.c_size_t, current_stream_ptr()
    a = c = g = None
    if arms is not None:
        a = [_plane_batch(x, torch.int32, P, H, W, "arms[%d]" % k) for k, x in enumerate(arms)]
        if len(a) != 4 or len({s for _, s in a}) != 1:
            raise ValueError("arms: four int32 [pairs][H][W] tensors (left, right, top, bottom) with one stride")
    if cls is not None:
        c, g = _plane_batch(cls, torch.uint8, P, H, W, "cls"), _plane_batch(gray, torch.uint8, P, H, W, "gray")
    single = maps.dim() == 2                             # one map in: state and status come back without the pairs axis
    if P == 0:
        return maps, state, status
    tail = (H, W, int(D), C.byref(p), _ptr(state), z(0), _ptr(status), st)
    if a is not None and c is not None:
        check(lib().smt_refine_batch(_ptr(m3), P, z(stride), *[_ptr(x) for x, _ in a], z(a[0][1]), _ptr(c[0]), z(c[1]),
                                     _ptr(g[0]), z(g[1]), *tail), "smt_refine_batch")
    elif a is not None:
        check(lib().smt_region_vote_batch(_ptr(m3), P, z(stride), *[_ptr(x) for x, _ in a], z(a[0][1]), *tail),
              "smt_region_vote_batch")
    else:
        check(lib().smt_interpolate_outliers_batch(_ptr(m3), P, z(stride), _ptr(c[0]), z(c[1]), _ptr(g[0]), z(g[1]), *tail),
              "smt_interpolate_outliers_batch")
    return (maps, state[0] if want_state else None, status[0]) if single else (maps, state, status)


@_on_tensor_device
def RegionVote(maps, arms, dispRange, params=None, want_state=False, **kw):
    """Iterative region voting (smt_region_vote_batch) on float32 [pairs][H][W] (or [H][W]) maps, in place,
    asynchronous on the current stream.  arms: (left, right, top, bottom) int32 tensors of the maps' shape, as
    CrossArmAggregation's arm maps.  params: refine_params(...), or its keywords (irv_ts, irv_th, irv_iters).
    -> (maps, state uint8 or None, status int32 [pairs][4] = {outliers on entry, voted, 0, flags}); for one [H][W] map
    state is [H][W] and status [4]."""
    return _refine_call(maps, arms, None, None, dispRange, params, want_state, kw)


@_on_tensor_device
def InterpolateOutliers(maps, cls, gray, dispRange, params=None, want_state=False, **kw):
    """Outlier interpolation along 16 rays (smt_interpolate_outliers_batch), in place, asynchronous.  cls: uint8 as
    LeftRightConsistency writes it (1 = occlusion: the smallest candidate; otherwise the candidate nearest in gray);
    gray: the uint8 left images.  Keyword: search.  -> (maps, state or None, status)."""
    return _refine_call(maps, None, cls, gray, dispRange, params, want_state, kw)


@_on_tensor_device
def Refine(maps, arms, cls, gray, dispRange, params=None, want_state=False, **kw):
    """RegionVote, then InterpolateOutliers (smt_refine_batch) -> (maps, state or None, status)."""
    return _refine_call(maps, arms, cls, gray, dispRange, params, want_state, kw)


@_on_tensor_device
def MedianFilterInPlace(maps, wnd_size):
    """MedianFilter(d, d, ...) (PostProcessing.h:314-344 with in == out, as CBLSM.cpp:162 calls it): the raster-order
    recurrence, not the out-of-place filter.  [H][W] or [pairs][H][W] float32 on the GPU, in place, one launch,
    asynchronous on the current stream.  Returns the same tensor."""
    m3 = maps[None] if isinstance(maps, torch.Tensor) and maps.dim() == 2 else maps
    P, H, W, stride = _map_batch(m3, "maps")
    check(lib().smt_median_filter_inplace_batch(_ptr(m3), P, C.c_size_t(stride), W, H, int(wnd_size),
                                                current_stream_ptr()), "smt_median_filter_inplace_batch")
    return maps


def median_inplace_set_impl(impl):
    """0 = rings in LDS and a sliding register window (default), 1 = the plain formulation.  Identical bits."""
    check(lib().smt_median_inplace_set_impl(int(impl)), "smt_median_inplace_set_impl")


def _u8_batch(maps, name, dtype=torch.uint8):
    """[P][H][W] (or [H][W]) maps on the GPU, each map dense, consecutive maps stride(0) >= H*W elements apart."""
    m3 = maps[None] if isinstance(maps, torch.Tensor) and maps.dim() == 2 else maps
    if not isinstance(m3, torch.Tensor) or not m3.is_cuda or m3.dtype != dtype or m3.dim() != 3:
        raise TypeError(f"{name} must be a {dtype} [pairs][H][W] tensor on the GPU")
    P, H, W = m3.shape
    if m3.stride(2) != 1 or (H > 1 and m3.stride(1) != W) or (P > 1 and m3.stride(0) < H * W):
        raise TypeError(f"{name}: every map must be dense and the maps must not overlap (strides {m3.stride()})")
    return m3, P, H, W, (m3.stride(0) if P > 1 else H * W)


def _asw_post(post):
    q = _lib.ASWPostParams()
    lib().smt_asw_post_default_params(C.byref(q))
    for k, v in post.items():
        if not hasattr(q, k):
            raise AttributeError(k)
        setattr(q, k, v)
    return q


@_on_tensor_device
def MinMaxNormalizeU8(maps, out=None):
    """normalize(m, m, 0, 255, NORM_MINMAX) + convertTo(CV_8UC1) (ASWeight.cpp:67-72) per map of [pairs][H][W] (or
    [H][W]): uint8 maps (smt_minmax_normalize_u8_batch) or finite float32 maps (smt_minmax_normalize_f32_u8_batch) ->
    uint8 maps of the same layout (`out`: default a new tensor; for uint8 maps it may be `maps` itself).  The library's
    restatement of OpenCV 3.1, parity unpinned.  Asynchronous on the current stream."""
    if isinstance(maps, torch.Tensor) and maps.dtype == torch.float32:
        m3, P, H, W, stride = _u8_batch(maps, "maps", torch.float32)
        fn, what = lib().smt_minmax_normalize_f32_u8_batch, "smt_minmax_normalize_f32_u8_batch"
    else:
        m3, P, H, W, stride = _u8_batch(maps, "maps")
        fn, what = lib().smt_minmax_normalize_u8_batch, "smt_minmax_normalize_u8_batch"
    if out is None:
        out = torch.empty_strided(tuple(maps.shape), tuple(maps.stride()), dtype=torch.uint8, device=maps.device)
    o3, Po, Ho, Wo, ostride = _u8_batch(out, "out")
    if (Po, Ho, Wo, ostride) != (P, H, W, stride):
        raise ValueError("out must have the shape and strides of maps")
    check(fn(_ptr(m3), _ptr(o3), P, stride, H, W, current_stream_ptr()), what)
    return out


@_on_tensor_device
def FilterSpecklesU8(maps, newVal, maxSpeckleSize, maxDiff, err=None):
    """filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on CV_8UC1 (ASWeight.cpp:73), in place on [pairs][H][W] (or
    [H][W]) uint8 maps: 4-neighbour components of at most maxSpeckleSize pixels become newVal.  The library's restatement
    of OpenCV 3.1, parity unpinned.  err: optional int32 [1] device flag (loop cap, never expected).  Asynchronous."""
    m3, P, H, W, stride = _u8_batch(maps, "maps")
    check(lib().smt_filter_speckles_u8_batch(_ptr(m3), P, stride, W, H, int(newVal), int(maxSpeckleSize), int(maxDiff),
                                             _ptr(err), current_stream_ptr()), "smt_filter_speckles_u8_batch")
    return maps


@_on_tensor_device
def MedianBlurU8(maps, ksize):
    """medianBlur(src, dst, ksize) (ASWeight.cpp:74, :78), ksize 3 or 5, uint8, BORDER_REPLICATE, on every map of
    [pairs][H][W] (or [H][W]) -> a new tensor of the same layout (OpenCV's in-place call copies, so this is it).  The
    library's restatement of OpenCV 3.1, parity unpinned.  One launch, asynchronous."""
    m3, P, H, W, stride = _u8_batch(maps, "maps")
    out = torch.empty_strided(tuple(maps.shape), tuple(maps.stride()), dtype=torch.uint8, device=maps.device)
    o3 = out[None] if out.dim() == 2 else out
    check(lib().smt_median_blur_u8_batch(_ptr(m3), _ptr(o3), P, stride, W, H, int(ksize), current_stream_ptr()),
          "smt_median_blur_u8_batch")
    return out


@_on_tensor_device
def FillImageNew(maps, fix=0, counts=False):
    """FillImageNew (ASW/ASW.h:434-511) in place on [pairs][H][W] (or [H][W]) uint8 maps, with the reference's defects
    (include/smt.h); fix=ASW_FIX_FILL_ROW_END makes column W count as outside.  counts=True: also returns int32
    [pairs][2] (holes that pushed nothing, holes left 0 for want of a list entry).  Three launches, asynchronous."""
    m3, P, H, W, stride = _u8_batch(maps, "maps")
    cnt = torch.zeros((P, 2), dtype=torch.int32, device=maps.device) if counts else None
    check(lib().smt_fill_image_new_batch(_ptr(m3), P, stride, H, W, C.c_uint(int(fix)), _ptr(cnt), current_stream_ptr()),
          "smt_fill_image_new_batch")
    return (maps, cnt) if counts else maps


@_on_tensor_device
def ASWTail(lastDisp, stages=False, err=None, **post):
    """ASWeight.cpp:69 + :72-78 in place on [pairs][H][W] (or [H][W]) uint8 maps (smt_asw_tail_batch): normalize,
    filterSpeckles, medianBlur 5, FillImageNew, medianBlur 3, each once over the batch.  Keywords override
    smt_asw_post_default_params.  -> (lastDisp, fill counts [pairs][2]); stages=True: (lastDisp, after_median,
    after_fill, counts), the driver's speckle.png and filled.png states.  Asynchronous on the current stream."""
    m3, P, H, W, stride = _u8_batch(lastDisp, "lastDisp")
    q = _asw_post(post)
    cnt = torch.zeros((P, 2), dtype=torch.int32, device=lastDisp.device)
    am = torch.empty_strided(tuple(m3.shape), tuple(m3.stride()), dtype=torch.uint8, device=m3.device) if stages else None
    af = torch.empty_strided(tuple(m3.shape), tuple(m3.stride()), dtype=torch.uint8, device=m3.device) if stages else None
    check(lib().smt_asw_tail_batch(_ptr(m3), P, stride, H, W, C.byref(q), _ptr(am), _ptr(af), _ptr(cnt), _ptr(err),
                                   current_stream_ptr()), "smt_asw_tail_batch")
    if stages:
        if lastDisp.dim() == 2:
            am, af = am[0], af[0]
        return lastDisp, am, af, cnt
    return lastDisp, cnt


def _cblsm_post(post):
    q = _lib.CBLSMPostParams()
    lib().smt_cblsm_post_default_params(C.byref(q))
    for k, v in post.items():
        if not hasattr(q, k):
            raise AttributeError(k)
        setattr(q, k, v)
    return q


@_on_tensor_device
def CBLSMTail(dispL, dispR, **post):
    """CBLSM.cpp:160-162 on [pairs][H][W] (or [H][W]) float32 maps on the GPU: LeftRightConsistency in place on dispL,
    RemoveSpeckles, MedianFilter in place -> (dispL, cls uint8, counts int32 [pairs][2]).  Keywords override
    smt_cblsm_post_default_params: gate, speckle_diff, speckle_min_area, speckle_invalid, median_wnd.  Asynchronous on
    the current stream."""
    l3, r3 = (dispL[None], dispR[None]) if dispL.dim() == 2 else (dispL, dispR)
    P, H, W, stride = _map_batch(l3, "dispL")
    if _map_batch(r3, "dispR") != (P, H, W, stride) or r3.device != l3.device:
        raise TypeError("dispR must have dispL's shape, stride and device")
    q = _cblsm_post(post)
    cls = torch.empty((P, H, W), dtype=torch.uint8, device=l3.device)
    counts = torch.zeros((P, 2), dtype=torch.int32, device=l3.device)
    check(lib().smt_cblsm_tail_batch(_ptr(l3), _ptr(r3), P, C.c_size_t(stride), H, W, C.byref(q), _ptr(cls), _ptr(counts),
                                     None, current_stream_ptr()), "smt_cblsm_tail_batch")
    return dispL, (cls[0] if dispL.dim() == 2 else cls), counts


# ======================================================================================
# Image files (host side): imread / imwrite of the reference's drivers
# ======================================================================================
def imread(path, want_channels=3):
    """cv::imread(path) (main.cpp:16-17): numpy uint8 [H][W][3] in B, G, R order by default;
    want_channels=1 gray, 0 as stored.  PNG / PGM / PPM, decoded by libsmt_hip.so's own reader."""
    import numpy as np
    p = C.POINTER(C.c_uint8)()
    H, W, ch = C.c_int(), C.c_int(), C.c_int()
    check(lib().smt_image_read(str(path).encode(), int(want_channels), C.byref(p), C.byref(H), C.byref(W), C.byref(ch)),
          "smt_image_read")
    try:
        a = np.ctypeslib.as_array(p, shape=(H.value * W.value * ch.value,)).copy()
    finally:
        lib().smt_image_free(p)
    return a.reshape(H.value, W.value) if ch.value == 1 else a.reshape(H.value, W.value, ch.value)


def imwrite(path, img):
    """cv::imwrite(path, img) (main.cpp:115-117) for uint8 [H][W] or [H][W][3] (B, G, R) arrays /
    CPU tensors; .png, .pgm, .ppm."""
    import numpy as np
    a = np.ascontiguousarray(img.cpu().numpy() if isinstance(img, torch.Tensor) else img, dtype=np.uint8)
    H, W = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    check(lib().smt_image_write(str(path).encode(), a.ctypes.data_as(C.c_void_p), H, W, ch), "smt_image_write")


# ======================================================================================
# ADCensusOption (CBLSM/adcensus_types.h:45-75) and the caller shape of CBLSM.cpp:138-143
# ======================================================================================
def ADCensusOption(**overrides):
    """Default-constructed ADCensusOption (adcensus_types.h:69-75) with fields overridden by keyword."""
    o = _lib.ADCensusOption()
    lib().smt_adcensus_option_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


@_on_tensor_device
def adcensus_option_aggregate(option, bytes_left, dispVolum, num_iters=4, want_disp=True):
    """CBLSM.cpp:138-143 + :152: CrossAggregator driven by an ADCensusOption -> (cost, disp)."""
    H, W, _ = bytes_left.shape
    D = option.max_disparity - option.min_disparity
    _dev(bytes_left, torch.uint8, (H, W, 3), "bytes_left")
    _dev(dispVolum, torch.float32, (H, W, D), "dispVolum")
    cost = torch.empty((H, W, D), dtype=torch.float32, device=dispVolum.device)
    disp = torch.empty((H, W), dtype=torch.float32, device=dispVolum.device) if want_disp else None
    check(lib().smt_adcensus_option_aggregate(C.byref(option), _ptr(bytes_left), _ptr(dispVolum), W, H, int(num_iters),
                                              _ptr(cost), _ptr(disp), current_stream_ptr()), "smt_adcensus_option_aggregate")
    return cost, disp


# ======================================================================================
# The whole AD-CensusV1/main.cpp pipeline, batched (smt_pipeline_*)
# ======================================================================================
def scratch_trim(keep_bytes=0, device=None):
    """smt_scratch_trim on `device` (default: current): idle scratch of smt_asw / smt_ncc back to the driver."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib().smt_scratch_trim(C.c_size_t(int(keep_bytes))), "smt_scratch_trim")


def scratch_poison(byte, device=None):
    """smt_scratch_poison on `device` (default: current): test hook, fills every idle block of the scratch arena with
    `byte` (synchronising), so that the next call runs on hostile scratch."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib().smt_scratch_poison(C.c_int(int(byte))), "smt_scratch_poison")


def scratch_info(device=None):
    """(reserved_bytes, used_bytes) of the library's scratch arena on `device`."""
    r, u = C.c_size_t(0), C.c_size_t(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib().smt_scratch_info(C.byref(r), C.byref(u)), "smt_scratch_info")
    return int(r.value), int(u.value)


class Pipeline:
    """main.cpp:46-92 (scanline and LR check enabled) for batches of gray pairs; the sharding unit of config 3."""

    def __init__(self, row, col, dispRange, device=None, quirks=0, subpixel=None, scan_views=VIEW_LEFT, **params):
        """params: the fields of smt_pipeline_params.  quirks: QUIRK_FIX_* for every stage, 0 = the reference's
        results; QUIRK_FIX_RIGHT_ARM_STRIDE also admits row > col.  subpixel: min_den of set_subpixel, None = integer
        maps.  scan_views: VIEW_LEFT = main.cpp's flow, VIEW_BOTH = set_scan_views."""
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.PipelineParams()
        lib().smt_pipeline_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_pipeline_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p), C.byref(h)),
              "smt_pipeline_create_on")
        self._h = h
        if quirks:
            self.set_quirks(quirks)
        if subpixel is not None:
            self.set_subpixel(subpixel)
        if scan_views != VIEW_LEFT:
            self.set_scan_views(scan_views)

    def set_quirks(self, quirks):
        """QUIRK_FIX_* from the next run on (between runs)."""
        check(lib().smt_pipeline_set_quirks(self._h, C.c_uint(quirks)), "smt_pipeline_set_quirks")

    def set_scan_views(self, views):
        """From the next run on (between runs): VIEW_BOTH scanline-optimises the aggregated right volume too (guided by
        the float right image), so dispR is the WTA of that sum and the LR check compares two optimised maps; VIEW_LEFT
        = main.cpp's flow, the default."""
        check(lib().smt_pipeline_set_scan_views(self._h, int(views)), "smt_pipeline_set_scan_views")

    def scan_right_volume(self):
        """The right view's scanline sum of the last pair of the last VIEW_BOTH run (borrowed, [row][col][dispRange])."""
        p = C.c_void_p()
        check(lib().smt_pipeline_scan_right_volume(self._h, C.byref(p)), "smt_pipeline_scan_right_volume")
        return _view_of(p.value, (self.row, self.col, self.dispRange), torch.float32, self.device)

    def set_subpixel(self, min_den=None):
        """From the next run on (between runs), dispL and dispR carry the parabola's fraction (wta_subpixel's rule with
        this min_den), and the LR check, RemoveSpeckles and MedianFilter run on those maps; None = integer maps."""
        check(lib().smt_pipeline_set_subpixel(self._h, _subpixel_arg(min_den)), "smt_pipeline_set_subpixel")

    def run(self, grayL, grayR):
        """uint8 [pairs][row][col] (or [row][col]) -> (dispL after LR check, dispR, cls, counts[pairs][2])."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"pipeline handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        check(lib().smt_pipeline_set_stream(self._h, current_stream_ptr(self.device)), "smt_pipeline_set_stream")
        check(lib().smt_pipeline_run_batch(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(cls), _ptr(counts)),
              "smt_pipeline_run_batch")
        return dl, dr, cls, counts

    def run_post(self, grayL, grayR, **post):
        """run() plus main.cpp:93-94 per pair -> (dispL after the LR check and RemoveSpeckles, dispR, cls, counts,
        lastDisp = MedianFilter of dispL).  Keywords override smt_post_default_params: speckle_diff,
        speckle_min_area, speckle_invalid, median_wnd."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"pipeline handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        q = _lib.PostParams()
        lib().smt_post_default_params(C.byref(q))
        for k, v in post.items():
            if not hasattr(q, k):
                raise AttributeError(k)
            setattr(q, k, v)
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        check(lib().smt_pipeline_set_stream(self._h, current_stream_ptr(self.device)), "smt_pipeline_set_stream")
        check(lib().smt_pipeline_run_batch_post(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(cls),
                                                _ptr(counts), C.byref(q), _ptr(last)), "smt_pipeline_run_batch_post")
        return dl, dr, cls, counts, last

    def run_refined(self, grayL, grayR, refine=None, **post):
        """run_post() with region voting and outlier interpolation between RemoveSpeckles and MedianFilter
        (smt_pipeline_run_batch_refined; the arms are recomputed from every pair's left image) -> (dispL after the LR
        check, RemoveSpeckles and the refinement, dispR, cls, counts, lastDisp = MedianFilter of dispL, state uint8
        [pairs][row][col], status int32 [pairs][4]).  refine: refine_params(...), None = the defaults; keywords as
        run_post."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"pipeline handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        q = _lib.PostParams()
        lib().smt_post_default_params(C.byref(q))
        for k, v in post.items():
            if not hasattr(q, k):
                raise AttributeError(k)
            setattr(q, k, v)
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        state = torch.empty_like(cls)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        status = torch.zeros((P, 4), dtype=torch.int32, device=grayL.device)
        check(lib().smt_pipeline_set_stream(self._h, current_stream_ptr(self.device)), "smt_pipeline_set_stream")
        check(lib().smt_pipeline_run_batch_refined(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(cls),
                                                   _ptr(counts), C.byref(q), C.byref(refine) if refine is not None else None,
                                                   _ptr(last), _ptr(state), _ptr(status)), "smt_pipeline_run_batch_refined")
        return dl, dr, cls, counts, last, state, status

    def run_filled(self, grayL, grayR, median_wnd=3, invalid=float("inf")):
        """run() plus, per pair behind the LR check, Sad.h's FillHolesInDispMap on dispL with the pair's cls and the
        MedianFilter (smt_pipeline_run_batch_filled; no RemoveSpeckles stage) -> (dispL after the LR check and the
        filler, dispR, cls, counts, lastDisp = MedianFilter of dispL, status int32 [pairs][4] = {n_occ, n_mis, n_third,
        flags})."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"pipeline handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        status = torch.zeros((P, 4), dtype=torch.int32, device=grayL.device)
        check(lib().smt_pipeline_set_stream(self._h, current_stream_ptr(self.device)), "smt_pipeline_set_stream")
        check(lib().smt_pipeline_run_batch_filled(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(cls),
                                                  _ptr(counts), int(median_wnd), C.c_float(invalid), _ptr(last),
                                                  _ptr(status)), "smt_pipeline_run_batch_filled")
        return dl, dr, cls, counts, last, status

    def volumes(self):
        ps = [C.c_void_p() for _ in range(5)]
        check(lib().smt_pipeline_volumes(self._h, *[C.byref(p) for p in ps]), "smt_pipeline_volumes")
        shp = (self.row, self.col, self.dispRange)
        return [_view_of(p.value, shp, torch.float32, self.device) for p in ps]

    def status(self):
        check(lib().smt_pipeline_status(self._h), "smt_pipeline_status")

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CBLSMFlow:
    """CBLSM.cpp's active flow (:64-67, 101-104, 133-134, 146-153) for batches of gray pairs: arms of both images, two
    costAggregationV5 passes per view (the right view's second on the LEFT arms, :150), ComputeDispOringin of each.
    Keywords override smt_cblsm_default_params: tau, sec_length, max_length.  The sharding unit of shard.cblsm_batch."""

    def __init__(self, row, col, dispRange, device=None, **params):
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.CBLSMParams()
        lib().smt_cblsm_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_cblsm_flow_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p),
                                             C.byref(h)), "smt_cblsm_flow_create_on")
        self._h = h

    def run(self, grayL, grayR):
        """uint8 [pairs][row][col] (or [row][col]) -> (dispL, dispR), float32 [pairs][row][col], on torch's current
        stream of the handle's device; nothing synchronises."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"CBLSM handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        check(lib().smt_cblsm_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_cblsm_flow_set_stream")
        check(lib().smt_cblsm_flow_run_batch(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr)),
              "smt_cblsm_flow_run_batch")
        return dl, dr

    def run_post(self, grayL, grayR, **post):
        """run() for all pairs, then CBLSM.cpp:160-162 once over the batch -> (dispL = the finished map, dispR, cls,
        counts[pairs][2]).  Keywords override smt_cblsm_post_default_params: gate, speckle_diff, speckle_min_area,
        speckle_invalid, median_wnd."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"CBLSM handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        q = _cblsm_post(post)
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        check(lib().smt_cblsm_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_cblsm_flow_set_stream")
        check(lib().smt_cblsm_flow_run_batch_post(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(cls),
                                                  _ptr(counts), C.byref(q)), "smt_cblsm_flow_run_batch_post")
        return dl, dr, cls, counts

    def run_window(self, grayL, grayR, winSize=1):
        """CBLSM.cpp with :132 enabled (smt_cblsm_flow_run_batch_window): the window costs of ComputeDispLeft /
        ComputeDispRight in place of the absolute differences, then the same two aggregation passes and WTA as run().
        uint8 [pairs][row][col] (or [row][col]) -> (dispL, dispR), float32 [pairs][row][col]."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"CBLSM handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        check(lib().smt_cblsm_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_cblsm_flow_set_stream")
        check(lib().smt_cblsm_flow_run_batch_window(self._h, _ptr(grayL), _ptr(grayR), P, int(winSize), _ptr(dl), _ptr(dr)),
              "smt_cblsm_flow_run_batch_window")
        return dl, dr

    def run_v4(self, grayL, grayR):
        """The per-hypothesis-arm flow (chooseArmLength*, ComputeAD, costAggregationV4, ComputeDispOringin;
        smt_cblsm_flow_run_batch_v4): uint8 [pairs][row][col] (or [row][col]) -> dispL, float32 [pairs][row][col].  Left
        view only, as the reference's arm rules are.  volumes()[0] is then the last pair's V4 volume."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"CBLSM handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        check(lib().smt_cblsm_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_cblsm_flow_set_stream")
        check(lib().smt_cblsm_flow_run_batch_v4(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl)),
              "smt_cblsm_flow_run_batch_v4")
        return dl

    def volumes(self):
        """The last pair's first-pass volumes (left view, right view), float32 [row][col][dispRange], borrowed."""
        ps = [C.c_void_p() for _ in range(2)]
        check(lib().smt_cblsm_flow_volumes(self._h, *[C.byref(p) for p in ps]), "smt_cblsm_flow_volumes")
        shp = (self.row, self.col, self.dispRange)
        return [_view_of(p.value, shp, torch.float32, self.device) for p in ps]

    def status(self):
        check(lib().smt_cblsm_flow_status(self._h), "smt_cblsm_flow_status")

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_cblsm_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CrossAggFlow:
    """CBLSM.cpp:133-143, 152 for batches of colour pairs: ComputeAD / ComputeADRight, CrossAggregator::Aggregate on the
    view's own colour image, ComputeDispOringin, and on request LeftRightConsistency (:160).  Keywords override
    smt_crossagg_flow_default_params: L1, L2, t1, t2, num_iters, gate.  The sharding unit of shard.crossagg_batch."""

    def __init__(self, row, col, dispRange, device=None, **params):
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.CrossAggFlowParams()
        lib().smt_crossagg_flow_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_crossagg_flow_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p),
                                                C.byref(h)), "smt_crossagg_flow_create_on")
        self._h = h

    def run(self, bgrL, bgrR, grayL=None, grayR=None, views=VIEW_BOTH, lr_check=False, dispL=None, dispR=None):
        """uint8 [pairs][row][col][3] (or [row][col][3]) BGR, optionally the gray pair uint8 [pairs][row][col] (derived
        with cvtColor_BGR2GRAY's rule when omitted) -> (dispL, dispR), float32 [pairs][row][col]; with lr_check (both
        views) -> (dispL after LeftRightConsistency, dispR, cls, counts[pairs][2]).  The map of a view that `views`
        leaves out is None, or the caller's dispL / dispR untouched.  On torch's current stream of the handle's device;
        nothing synchronises."""
        if bgrL.dim() == 3:
            bgrL, bgrR = bgrL[None], bgrR[None]
            if grayL is not None:
                grayL = grayL[None]
            if grayR is not None:
                grayR = grayR[None]
        P = bgrL.shape[0]
        if _dev_index(bgrL.device) != _dev_index(self.device) or bgrR.device != bgrL.device:
            raise ValueError(f"CrossAggFlow handle lives on {self.device}, images on {bgrL.device} / {bgrR.device}")
        _dev(bgrL, torch.uint8, (P, self.row, self.col, 3), "bgrL")
        _dev(bgrR, torch.uint8, (P, self.row, self.col, 3), "bgrR")
        for g, name in ((grayL, "grayL"), (grayR, "grayR")):
            if g is not None:
                _dev(g, torch.uint8, (P, self.row, self.col), name)
        shp = (P, self.row, self.col)
        if dispL is None and views & VIEW_LEFT:
            dispL = torch.empty(shp, dtype=torch.float32, device=bgrL.device)
        if dispR is None and views & VIEW_RIGHT:
            dispR = torch.empty(shp, dtype=torch.float32, device=bgrL.device)
        for d, name in ((dispL, "dispL"), (dispR, "dispR")):
            if d is not None:
                _dev(d, torch.float32, shp, name)
        cls = torch.empty(shp, dtype=torch.uint8, device=bgrL.device) if lr_check else None
        counts = torch.zeros((P, 2), dtype=torch.int32, device=bgrL.device) if lr_check else None
        check(lib().smt_crossagg_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_crossagg_flow_set_stream")
        check(lib().smt_crossagg_flow_run_batch(self._h, _ptr(bgrL), _ptr(bgrR), _ptr(grayL), _ptr(grayR), P, int(views),
                                                _ptr(dispL), _ptr(dispR), _ptr(cls), _ptr(counts)),
              "smt_crossagg_flow_run_batch")
        if lr_check:
            return dispL, dispR, cls, counts
        return dispL, dispR

    def run_post(self, bgrL, bgrR, grayL=None, grayR=None, **post):
        """run() with both views for all pairs, then CBLSM.cpp:160-162 once over the batch -> (dispL = the finished map,
        dispR, cls, counts[pairs][2]).  The gate comes from `post` (default 5), not from the handle.  Keywords override
        smt_cblsm_post_default_params."""
        if bgrL.dim() == 3:
            bgrL, bgrR = bgrL[None], bgrR[None]
            if grayL is not None:
                grayL = grayL[None]
            if grayR is not None:
                grayR = grayR[None]
        P = bgrL.shape[0]
        if _dev_index(bgrL.device) != _dev_index(self.device) or bgrR.device != bgrL.device:
            raise ValueError(f"CrossAggFlow handle lives on {self.device}, images on {bgrL.device} / {bgrR.device}")
        _dev(bgrL, torch.uint8, (P, self.row, self.col, 3), "bgrL")
        _dev(bgrR, torch.uint8, (P, self.row, self.col, 3), "bgrR")
        for g, name in ((grayL, "grayL"), (grayR, "grayR")):
            if g is not None:
                _dev(g, torch.uint8, (P, self.row, self.col), name)
        q = _cblsm_post(post)
        shp = (P, self.row, self.col)
        dl = torch.empty(shp, dtype=torch.float32, device=bgrL.device)
        dr = torch.empty_like(dl)
        cls = torch.empty(shp, dtype=torch.uint8, device=bgrL.device)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=bgrL.device)
        check(lib().smt_crossagg_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_crossagg_flow_set_stream")
        check(lib().smt_crossagg_flow_run_batch_post(self._h, _ptr(bgrL), _ptr(bgrR), _ptr(grayL), _ptr(grayR), P, _ptr(dl),
                                                     _ptr(dr), _ptr(cls), _ptr(counts), C.byref(q)),
              "smt_crossagg_flow_run_batch_post")
        return dl, dr, cls, counts

    def status(self):
        check(lib().smt_crossagg_flow_status(self._h), "smt_crossagg_flow_status")

    def volumes(self):
        """The last pair's aggregated volumes (left view, right view), float32 [row][col][dispRange], borrowed."""
        ps = [C.c_void_p() for _ in range(2)]
        check(lib().smt_crossagg_flow_volumes(self._h, *[C.byref(p) for p in ps]), "smt_crossagg_flow_volumes")
        shp = (self.row, self.col, self.dispRange)
        return [_view_of(p.value, shp, torch.float32, self.device) for p in ps]

    def set_impl(self, impl):
        """0 = fused kernels (default), 1 = the composed path (smt_cblsm_ad, the aggregation passes, smt_wta)."""
        check(lib().smt_crossagg_flow_set_impl(self._h, int(impl)), "smt_crossagg_flow_set_impl")
        return self

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_crossagg_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ASWFlow:
    """ASWeight.cpp's active lines (:54-55, :60-61, :66) for batches of gray pairs: replicate padding by winSize + 1, both
    views from one pass over the hypotheses (smt_asw_both), CrossCheckDiaparity.  Keywords override
    smt_asw_default_params: winSize, T, sigma_space, sigma_color.  The sharding unit of shard.asw_batch."""

    def __init__(self, row, col, dispRange, device=None, **params):
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.ASWParams()
        lib().smt_asw_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_asw_flow_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p),
                                           C.byref(h)), "smt_asw_flow_create_on")
        self._h = h

    def run(self, grayL, grayR):
        """uint8 [pairs][row][col] (or [row][col]) -> (dispL, dispR, lastDisp): float32, float32, uint8
        [pairs][row][col], on torch's current stream of the handle's device; nothing synchronises."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"ASW handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        check(lib().smt_asw_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_asw_flow_set_stream")
        check(lib().smt_asw_flow_run_batch(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(last)),
              "smt_asw_flow_run_batch")
        return dl, dr, last

    def run_post(self, grayL, grayR, **post):
        """run(), then the file's tail (:67-78, smt_asw_flow_run_batch_post) once over the batch -> dict: dispL, dispR
        (the un-normalised float maps of run()), dispL8, dispR8 (:67-68 + :70-71), lastDisp (the finished map, medain.png),
        after_median, after_fill (speckle.png, filled.png), fill_counts int32 [pairs][2].  Keywords override
        smt_asw_post_default_params."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"ASW handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        q = _asw_post(post)
        shp = (P, self.row, self.col)
        dl = torch.empty(shp, dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        u8 = [torch.empty(shp, dtype=torch.uint8, device=grayL.device) for _ in range(5)]
        last, dl8, dr8, am, af = u8
        cnt = torch.zeros((P, 2), dtype=torch.int32, device=grayL.device)
        check(lib().smt_asw_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_asw_flow_set_stream")
        check(lib().smt_asw_flow_run_batch_post(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(last),
                                                _ptr(dl8), _ptr(dr8), C.byref(q), _ptr(am), _ptr(af), _ptr(cnt)),
              "smt_asw_flow_run_batch_post")
        return {"dispL": dl, "dispR": dr, "dispL8": dl8, "dispR8": dr8, "lastDisp": last, "after_median": am,
                "after_fill": af, "fill_counts": cnt}

    def status(self):
        check(lib().smt_asw_flow_status(self._h), "smt_asw_flow_status")

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_asw_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SADFlow:
    """SADmain.cpp with :67-68 enabled (:47-48, :66-68) for batches of gray pairs: replicate padding by winsize + 1, both
    views from one pass over the hypotheses (smt_sad_both), CrossCheckDiaparity.  Keywords override
    smt_sad_default_params: winsize.  The sharding unit of shard.sad_batch."""

    def __init__(self, row, col, dispRange, device=None, **params):
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.SADParams()
        lib().smt_sad_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_sad_flow_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p),
                                           C.byref(h)), "smt_sad_flow_create_on")
        self._h = h

    def run(self, grayL, grayR):
        """uint8 [pairs][row][col] (or [row][col]) -> (dispL, dispR, lastdisp, cls): int32, int32, int32, uint8
        [pairs][row][col], on torch's current stream of the handle's device; nothing synchronises."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"SAD handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.int32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        check(lib().smt_sad_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_sad_flow_set_stream")
        check(lib().smt_sad_flow_run_batch(self._h, _ptr(grayL), _ptr(grayR), P, _ptr(dl), _ptr(dr), _ptr(last), _ptr(cls)),
              "smt_sad_flow_run_batch")
        return dl, dr, last, cls

    def run_subpixel(self, grayL, grayR, min_den=1.0):
        """run() with the parabola of Sad.h:76-81 kept (smt_sad_flow_run_batch_subpixel) -> (dispL, dispR, lastdisp, cls):
        float32, float32, float32, uint8.  The cross-check is decided on the integer winners, so cls is run()'s; lastdisp
        is dispL where accepted and +inf where rejected."""
        if grayL.dim() == 2:
            grayL, grayR = grayL[None], grayR[None]
        P = grayL.shape[0]
        if _dev_index(grayL.device) != _dev_index(self.device) or grayR.device != grayL.device:
            raise ValueError(f"SAD handle lives on {self.device}, images on {grayL.device} / {grayR.device}")
        _dev(grayL, torch.uint8, (P, self.row, self.col), "grayL")
        _dev(grayR, torch.uint8, (P, self.row, self.col), "grayR")
        dl = torch.empty((P, self.row, self.col), dtype=torch.float32, device=grayL.device)
        dr = torch.empty_like(dl)
        last = torch.empty_like(dl)
        cls = torch.empty((P, self.row, self.col), dtype=torch.uint8, device=grayL.device)
        check(lib().smt_sad_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_sad_flow_set_stream")
        check(lib().smt_sad_flow_run_batch_subpixel(self._h, _ptr(grayL), _ptr(grayR), P, _subpixel_arg(min_den), _ptr(dl),
                                                    _ptr(dr), _ptr(last), _ptr(cls)), "smt_sad_flow_run_batch_subpixel")
        return dl, dr, last, cls

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_sad_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NCCFlow:
    """NCC_main.cpp:33 for batches of gray pairs (smt_ncc_flow_*): one statistics launch and one cost launch per batch.
    Keywords override smt_ncc_default_params: winSize.  The sharding unit of shard.ncc_batch."""

    def __init__(self, row, col, dispRange, device=None, **params):
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _lib.NCCParams()
        lib().smt_ncc_default_params(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        h = C.c_void_p()
        check(lib().smt_ncc_flow_create_on(_dev_index(self.device), self.row, self.col, self.dispRange, C.byref(p),
                                           C.byref(h)), "smt_ncc_flow_create_on")
        self._h = h

    def set_form(self, form):
        """0 = the dispatch rule (default), else NCC_FORM_LOOP / NCC_FORM_DOT4 / NCC_FORM_BOX."""
        check(lib().smt_ncc_flow_set_form(self._h, int(form)), "smt_ncc_flow_set_form")
        return self

    def run(self, L8, R8, want_cost=False):
        """uint8 [pairs][row][col] (or [row][col]) -> disp int32 [pairs][row][col], or (disp, cost) with cost float64
        [pairs][row][col][dispRange], on torch's current stream of the handle's device; nothing synchronises."""
        if L8.dim() == 2:
            L8, R8 = L8[None], R8[None]
        P = L8.shape[0]
        if _dev_index(L8.device) != _dev_index(self.device) or R8.device != L8.device:
            raise ValueError(f"NCC handle lives on {self.device}, images on {L8.device} / {R8.device}")
        _dev(L8, torch.uint8, (P, self.row, self.col), "L8")
        _dev(R8, torch.uint8, (P, self.row, self.col), "R8")
        disp = torch.empty((P, self.row, self.col), dtype=torch.int32, device=L8.device)
        cost = torch.empty((P, self.row, self.col, self.dispRange), dtype=torch.float64, device=L8.device) if want_cost else None
        check(lib().smt_ncc_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_ncc_flow_set_stream")
        check(lib().smt_ncc_flow_run_batch(self._h, _ptr(L8), _ptr(R8), P, _ptr(disp), _ptr(cost)), "smt_ncc_flow_run_batch")
        return (disp, cost) if want_cost else disp

    def run_both(self, L8, R8, want=("dispL", "dispR", "lastdisp", "cls")):
        """smt_lrncc_flow_run_batch: uint8 [pairs][row][col] (or [row][col]) -> (dispL, dispR, lastdisp, cls), int32, int32,
        int32 and uint8 [pairs][row][col]; an output not named in `want` is not computed for the caller and comes back as
        None.  lastdisp and cls are sad_CrossCheckDiaparity of the two maps.  On torch's current stream of the handle's
        device; nothing synchronises."""
        if L8.dim() == 2:
            L8, R8 = L8[None], R8[None]
        P = L8.shape[0]
        if _dev_index(L8.device) != _dev_index(self.device) or R8.device != L8.device:
            raise ValueError(f"NCC handle lives on {self.device}, images on {L8.device} / {R8.device}")
        _dev(L8, torch.uint8, (P, self.row, self.col), "L8")
        _dev(R8, torch.uint8, (P, self.row, self.col), "R8")
        unknown = set(want) - {"dispL", "dispR", "lastdisp", "cls"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        shape = (P, self.row, self.col)
        outs = [torch.empty(shape, dtype=torch.uint8 if n == "cls" else torch.int32, device=L8.device) if n in want else None
                for n in ("dispL", "dispR", "lastdisp", "cls")]
        check(lib().smt_ncc_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_ncc_flow_set_stream")
        check(lib().smt_lrncc_flow_run_batch(self._h, _ptr(L8), _ptr(R8), P, *[_ptr(o) for o in outs]), "smt_lrncc_flow_run_batch")
        return tuple(outs)

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_ncc_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NCCWholeFlow:
    """NCC_main.cpp with :24 enabled, both types, for batches of gray pairs (smt_whole_ncc_flow_*), followed by the int-map
    cross-check of Sad.h:184-222 on the two offset maps.  Keywords: kernel_size, max_offset, add_constant (defaults 5, 79,
    False).  The sharding unit of shard.ncc_whole_batch."""
    OUTS = ("depthL", "depthR", "offL", "offR", "lastdisp", "cls")

    def __init__(self, row, col, device=None, kernel_size=5, max_offset=79, add_constant=False):
        self.row, self.col = int(row), int(col)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        p = _ncc_whole_params(kernel_size, max_offset, add_constant)
        h = C.c_void_p()
        check(lib().smt_whole_ncc_flow_create_on(_dev_index(self.device), self.row, self.col, C.byref(p), C.byref(h)),
              "smt_whole_ncc_flow_create_on")
        self._h = h

    def set_form(self, form):
        """0 = as ncc() chooses (default), else NCC_WHOLE_FORM_LOOP / NCC_WHOLE_FORM_INT."""
        check(lib().smt_whole_ncc_flow_set_form(self._h, int(form)), "smt_whole_ncc_flow_set_form")
        return self

    def run(self, L8, R8, want=OUTS):
        """uint8 [pairs][row][col] (or [row][col]) -> (depthL, depthR, offL, offR, lastdisp, cls): uint8, uint8, int32, int32,
        int32 and uint8 [pairs][row][col]; an output not named in `want` comes back as None.  lastdisp and cls are
        sad_CrossCheckDiaparity of the two offset maps.  On torch's current stream of the handle's device; nothing
        synchronises."""
        if L8.dim() == 2:
            L8, R8 = L8[None], R8[None]
        P = L8.shape[0]
        if _dev_index(L8.device) != _dev_index(self.device) or R8.device != L8.device:
            raise ValueError(f"NCC handle lives on {self.device}, images on {L8.device} / {R8.device}")
        _dev(L8, torch.uint8, (P, self.row, self.col), "L8")
        _dev(R8, torch.uint8, (P, self.row, self.col), "R8")
        unknown = set(want) - set(self.OUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        shape = (P, self.row, self.col)
        outs = [torch.empty(shape, dtype=torch.int32 if n in ("offL", "offR", "lastdisp") else torch.uint8, device=L8.device)
                if n in want else None for n in self.OUTS]
        check(lib().smt_whole_ncc_flow_set_stream(self._h, current_stream_ptr(self.device)), "smt_whole_ncc_flow_set_stream")
        check(lib().smt_whole_ncc_flow_run_batch(self._h, _ptr(L8), _ptr(R8), P, *[_ptr(o) for o in outs]),
              "smt_whole_ncc_flow_run_batch")
        return tuple(outs)

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_whole_ncc_flow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostStats(C.Structure):
    """smt_host_stats (include/smt.h)."""
    _fields_ = [("wall_ms", C.c_double), ("h2d_ms", C.c_double), ("compute_ms", C.c_double), ("d2h_ms", C.c_double),
                ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("chunks", C.c_int), ("pinned_in", C.c_int),
                ("pinned_out", C.c_int)]


class ADCensusHostBatch:
    """AD-Census of whole batches fed from host memory (smt_adcensus_host_*): what AD-CensusV1/main.cpp does around the
    hot path (imread + cvtColor BGR2GRAY, the uchar -> float staging, the maps back to the host) for many pairs, with
    the copies in and out overlapped with the compute.  Both views; the maps equal AD_Census.ComputeBatch's bit for bit.

    channels: 1 (gray images [P, row, col]) or 3 (B, G, R images [P, row, col, 3]).  out_dtype: torch.float32 or
    torch.uint8 (exact, dispRange <= 256 only).  chunk: pairs per step; the default 16 is the fastest point of the
    measured sweep 2 / 4 / 8 / 16 / 32 at config 5 (256 KITTI pairs, D = 256; profiles/hostfeed_cfg5.json, DESIGN.md
    section 5).  Pinned tensors
    (pin_memory()) make the copies overlap; pageable ones give the same maps, slower."""

    def __init__(self, row, col, dispRange, sigmaC=10.0, sigmaS=30.0, channels=1, out_dtype=torch.float32, chunk=16,
                 device=None):
        if channels not in (1, 3):
            raise ValueError("channels must be 1 or 3")
        if out_dtype not in (torch.float32, torch.uint8):
            raise ValueError("out_dtype must be torch.float32 or torch.uint8")
        self.row, self.col, self.dispRange = int(row), int(col), int(dispRange)
        self.channels, self.out_dtype, self.chunk = int(channels), out_dtype, int(chunk)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        fmt = 1 if out_dtype == torch.uint8 else 0
        h = C.c_void_p()
        check(lib().smt_adcensus_host_create(_dev_index(self.device), self.row, self.col, self.dispRange,
                                             C.c_float(sigmaC), C.c_float(sigmaS), self.channels, fmt, self.chunk,
                                             C.byref(h)), "smt_adcensus_host_create")
        self._h = h

    def _host(self, t, dtype, shape, name):
        if not isinstance(t, torch.Tensor) or t.device.type != "cpu":
            raise ValueError(f"{name} must be a CPU torch tensor")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t

    def run(self, L, R, dispL=None, dispR=None):
        """L, R: CPU uint8 [P, row, col] (channels=1) or [P, row, col, 3]; returns CPU (dispL, dispR) [P, row, col] of
        out_dtype, allocated with pin_memory=True when not given.  Returns once every map is in host memory."""
        if not isinstance(L, torch.Tensor) or L.dim() < 1:
            raise ValueError("L must be a CPU torch tensor")
        P = int(L.shape[0])
        img = (P, self.row, self.col) + ((3,) if self.channels == 3 else ())
        self._host(L, torch.uint8, img, "L")
        self._host(R, torch.uint8, img, "R")
        shp = (P, self.row, self.col)
        if dispL is None:
            dispL = torch.empty(shp, dtype=self.out_dtype, pin_memory=True)
        if dispR is None:
            dispR = torch.empty(shp, dtype=self.out_dtype, pin_memory=True)
        self._host(dispL, self.out_dtype, shp, "dispL")
        self._host(dispR, self.out_dtype, shp, "dispR")
        check(lib().smt_adcensus_host_run(self._h, _ptr(L), _ptr(R), P, _ptr(dispL), _ptr(dispR)),
              "smt_adcensus_host_run")
        return dispL, dispR

    def stats(self):
        """Device-event times and byte counts of the last run (smt_host_stats) as a dict."""
        s = HostStats()
        check(lib().smt_adcensus_host_stats(self._h, C.byref(s)), "smt_adcensus_host_stats")
        return {name: getattr(s, name) for name, _ in HostStats._fields_}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().smt_adcensus_host_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
