"""The table of the bounds suite: every entry point of include/smt.h that takes caller buffers -> the cases it is
run at, and how one case is laid out in an arena (tests/arena.py), called through the C ABI and compared with the oracle.

An entry of ENTRIES is `make(A, X, **params) -> (call, verify)`: it declares the call's tensors in the arena A (inputs
with their data, outputs by shape), returns `call() -> status` -- which takes its pointers from A after A.build() --
and `verify(outs)`, which holds the outputs (and what call() put into A.extra: buffers the library owns, copied back)
to the CPU oracle by the rule the entry's own parity test applies; the helpers of those tests are imported, not restated.
CASES maps the same names to lists of params.  NOT_CALLER_BUFFER names every other declaration of the header with the
reason it has no case; tests/test_bounds_cpu.py holds the union to the header.

Shapes: the smallest at which a tile edge exists, from the kernels' own constants -- 32-pixel strips (STP) of the SAD
kernels, 16-pixel NCC / ASW workgroups, 64 hypotheses per lane slot (D = 1, 64, 65 and one D > 256 where the dispatch
has a carry path), 64-pixel chunks of the AD-Census kernels, padded widths with (W + 2w) % 4 in {1, 2, 3} for the
dword-staged matchers, H = 1 and odd H.  Images are random bytes (or few-level noise where arms must be long), never
flat: a stray read of a neighbouring in-image byte moves the result away from the oracle too.
"""
import ctypes as C

import numpy as np

import arena
import cblsm_v4_cases as VC
import exact_matchers as XM
import fill_batch_cases as FC
import median_inplace_cases as MC

INT_MIN = -(2 ** 31)
SMT_ERR_REF_UB = -5
VL, VR, VB = 1, 2, 3
sz, f32, u32 = C.c_size_t, C.c_float, C.c_uint


class Ctx:
    """what a case needs besides its arena: the library, the oracle, the device (None: host twins only)"""

    def __init__(self, O, device=None):
        from stereo_match_traditional_amd import _lib
        self.O, self.device, self.L = O, device, _lib
        self.lib = _lib.lib()
        self.dev_index = 0
        if device is not None:
            import torch
            self.torch = torch
            self.dev_index = torch.cuda.current_device()

    def st(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def sync(self):
        if self.device is not None:
            self.torch.cuda.synchronize()

    def d2h(self, ptr, shape, dtype):
        """copy of a buffer the library owns"""
        self.sync()
        out = np.empty(shape, dtype)
        assert self.lib.smt_memcpy_d2h(out.ctypes.data_as(C.c_void_p), ptr, sz(out.nbytes), None) == 0
        assert self.lib.smt_stream_sync(None) == 0
        return out


def rb(shape, seed, lo=0, hi=256):
    return np.random.default_rng([seed, *shape]).integers(lo, hi, shape).astype(np.uint8)


def rf(shape, seed, scale=2.0):
    return (np.random.default_rng([seed, *shape]).random(shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


def bits_eq(got, ref, what=""):
    ref = np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got.view(np.uint8) != ref.view(np.uint8)
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ from the oracle, first at flat byte {int(np.flatnonzero(bad)[0])}"


def val_eq(got, ref, what=""):
    assert got.shape == np.shape(ref), (what, got.shape, np.shape(ref))
    bad = ~(got == ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries differ from the oracle, first at {np.argwhere(bad)[0].tolist()}"


def nan_bits_eq(got, ref, what=""):
    """bit-equal where the oracle is not NaN, NaN where it is"""
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    ok = ~np.isnan(ref)
    bits_eq(np.ascontiguousarray(got[ok]), np.ascontiguousarray(ref[ok].astype(got.dtype)), what)


ENTRIES, CASES = {}, {}


def entry(name, *cases):
    def deco(f):
        ENTRIES[name] = f
        CASES[name] = list(cases)
        return f
    return deco


# ================================================================================================ staging, reductions
@entry("smt_bgr2gray", dict(H=1, W=63), dict(H=5, W=65), dict(H=3, W=257))
def _bgr2gray(A, X, H, W):
    bgr = rb((H, W, 3), 1)
    A.inp("bgr", bgr); A.out("gray", (H, W), np.uint8)
    return (lambda: X.lib.smt_bgr2gray(A.ptr("bgr"), H, W, A.ptr("gray"), X.st()),
            lambda o: bits_eq(o["gray"], X.O.bgr2gray(bgr), "gray"))


@entry("smt_pad_replicate", dict(H=1, W=7, pad=2), dict(H=5, W=65, pad=3), dict(H=4, W=33, pad=0), dict(H=3, W=255, pad=17))
def _pad(A, X, H, W, pad):
    src = rb((H, W), 2)
    A.inp("src", src); A.out("dst", (H + 2 * pad, W + 2 * pad), np.uint8)
    return (lambda: X.lib.smt_pad_replicate(A.ptr("src"), H, W, pad, A.ptr("dst"), X.st()),
            lambda o: bits_eq(o["dst"], X.O.pad_replicate(src, pad), "dst"))


@entry("smt_u8_to_f32", dict(H=1, W=63), dict(H=3, W=257))
def _u8f32(A, X, H, W):
    src = rb((H, W), 3)
    A.inp("src", src); A.out("dst", (H, W), np.float32)
    return (lambda: X.lib.smt_u8_to_f32(A.ptr("src"), H, W, A.ptr("dst"), X.st()),
            lambda o: bits_eq(o["dst"], src.astype(np.float32), "dst"))


@entry("smt_sum_f32", dict(n=1), dict(n=255), dict(n=70001))
def _sum(A, X, n):
    """integer-valued terms: the float64 sum is exact in any order"""
    x = np.random.default_rng(n).integers(-1000, 1000, n).astype(np.float32)
    A.inp("x", x); A.out("sum", (1,), np.float64)
    return (lambda: X.lib.smt_sum_f32(A.ptr("x"), sz(n), A.ptr("sum"), X.st()),
            lambda o: bits_eq(o["sum"], np.array([x.astype(np.float64).sum()]), "sum"))


@entry("smt_wta", dict(H=1, W=9, D=1), dict(H=3, W=65, D=64), dict(H=5, W=33, D=65), dict(H=2, W=17, D=300))
def _wta(A, X, H, W, D):
    vol = np.random.default_rng(D).integers(0, 6, (H, W, D)).astype(np.float32)          # exact ties
    A.inp("vol", vol); A.out("disp", (H, W), np.float32)
    return (lambda: X.lib.smt_wta(A.ptr("vol"), H, W, D, A.ptr("disp"), X.st()),
            lambda o: val_eq(o["disp"], X.O.wta(vol), "disp"))


# ================================================================================================ AD-Census
def _adcensus(batch):
    def make(A, X, H, W, D, P=1, maps=True):
        Ls = np.stack([rb((H, W), 10 + b) for b in range(P)]).astype(np.float32)
        Rs = np.stack([rb((H, W), 20 + b) for b in range(P)]).astype(np.float32)
        shp = (P, H, W) if batch else (H, W)
        A.inp("L", Ls.reshape(shp)); A.inp("R", Rs.reshape(shp))
        if maps:
            A.out("dispL", shp, np.float32); A.out("dispR", shp, np.float32)
        dl, dr = ("dispL", "dispR") if maps else (None, None)

        def call():
            lib, h = X.lib, C.c_void_p()
            rc = lib.smt_adcensus_create_ex(X.dev_index, H, W, D, f32(10.0), f32(30.0), u32(3), C.byref(h))
            if rc:
                return rc
            try:
                rc = lib.smt_adcensus_set_stream(h, X.st())
                if batch:
                    rc = rc or lib.smt_adcensus_compute_batch(h, A.ptr("L"), A.ptr("R"), P, VB, A.ptr(dl), A.ptr(dr))
                else:
                    rc = rc or lib.smt_adcensus_compute(h, A.ptr("L"), A.ptr("R"), VB, A.ptr(dl), A.ptr(dr))
                rc = rc or lib.smt_adcensus_status(h)
                for view, nm in ((VL, "volL"), (VR, "volR")):
                    p = C.c_void_p()
                    rc = rc or lib.smt_adcensus_volume(h, view, C.byref(p))
                    if not rc:
                        A.extra[nm] = X.d2h(p, (H, W, D), np.float32)
                return rc
            finally:
                lib.smt_adcensus_destroy(h)

        def verify(o):
            for b in range(P):
                L, R = Ls[b].astype(np.uint8), Rs[b].astype(np.uint8)
                vl, vr = (X.O.adcensus_view(L, R, D, 10.0, 30.0, v) for v in (0, 1))
                if maps:
                    val_eq(o["dispL"].reshape(P, H, W)[b], X.O.wta(vl), f"dispL[{b}]")
                    val_eq(o["dispR"].reshape(P, H, W)[b], X.O.wta(vr), f"dispR[{b}]")
            bits_eq(o["volL"], vl, "left volume of the last pair"); bits_eq(o["volR"], vr, "right volume of the last pair")
        return call, verify
    return make


entry("smt_adcensus_compute", dict(H=1, W=63, D=64), dict(H=3, W=65, D=65), dict(H=2, W=40, D=300),
      dict(H=3, W=70, D=1), dict(H=3, W=33, D=16, maps=False))(_adcensus(False))
entry("smt_adcensus_compute_batch", dict(H=3, W=65, D=64, P=3), dict(H=1, W=63, D=65, P=2), dict(H=2, W=40, D=300, P=2),
      dict(H=3, W=33, D=16, P=2, maps=False))(_adcensus(True))


# ================================================================================================ cross arms
def _crossarm(X, H, W, D, cblsm=False):
    p, h = X.L.CrossArmParams(), C.c_void_p()
    (X.lib.smt_crossarm_cblsm_params if cblsm else X.lib.smt_crossarm_default_params)(C.byref(p))
    rc = X.lib.smt_crossarm_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
    rc = rc or X.lib.smt_crossarm_set_stream(h, X.st())
    return rc, h


def _arm_maps(A, X, h, H, W):
    ps = [C.c_void_p() for _ in range(4)]
    rc = X.lib.smt_crossarm_arm_maps(h, *[C.byref(p) for p in ps])
    if not rc:
        for nm, p in zip("LRTB", ps):
            A.extra["arm" + nm] = X.d2h(p, (H, W), np.int32)
    return rc


def _arm_image(H, W, ch, seed):
    g = VC.noisy_pair(H, W, seed)[0]
    return g if ch == 1 else np.stack([g, np.roll(g, 1, 1), g[::-1]], axis=2).copy()


def _arms(by_dir):
    def make(A, X, H, W, ch):
        img = _arm_image(H, W, ch, 31)
        A.inp("img", img)

        def call():
            rc, h = _crossarm(X, H, W, 8)
            try:
                if by_dir:
                    rc = rc or X.lib.smt_crossarm_reset(h)
                    for d in range(4):
                        rc = rc or X.lib.smt_crossarm_arm_dir(h, A.ptr("img"), ch, d)
                else:
                    rc = rc or X.lib.smt_crossarm_arms(h, A.ptr("img"), ch)
                return rc or _arm_maps(A, X, h, H, W)
            finally:
                X.lib.smt_crossarm_destroy(h)

        def verify(o):
            for nm, r in zip("LRTB", X.O.arms_all(img)):
                val_eq(o["arm" + nm], r, "arm " + nm)
        return call, verify
    return make


entry("smt_crossarm_arms", dict(H=1, W=63, ch=1), dict(H=7, W=65, ch=3), dict(H=9, W=130, ch=1))(_arms(False))
entry("smt_crossarm_arm_dir", dict(H=1, W=63, ch=1), dict(H=7, W=65, ch=3))(_arms(True))


def _aggregate(load):
    def make(A, X, H, W, D, order, disp=True):
        img = VC.noisy_pair(H, W, 33)[0]
        arms = X.O.arms_all(img, 25, 6, 17, 34, chain=False, right_row_bug=False) if load else X.O.arms_all(img)
        vol = rf((H, W, D), 34)
        A.inp("vol_in", vol); A.out("vol_out", (H, W, D), np.float32)
        if load:
            for nm, a in zip("LRTB", arms):
                A.inp("arm" + nm, a.astype(np.int32))
        else:
            A.inp("img", img)
        if disp:
            A.out("disp", (H, W), np.float32)

        def call():
            rc, h = _crossarm(X, H, W, D, cblsm=load)
            try:
                if load:
                    rc = rc or X.lib.smt_crossarm_load_arm_maps(h, *[A.ptr("arm" + nm) for nm in "LRTB"])
                else:
                    rc = rc or X.lib.smt_crossarm_arms(h, A.ptr("img"), 1)
                rc = rc or X.lib.smt_crossarm_aggregate(h, A.ptr("vol_in"), A.ptr("vol_out"), order, A.ptr("disp" if disp else None))
                return rc or X.lib.smt_crossarm_status(h)
            finally:
                X.lib.smt_crossarm_destroy(h)

        def verify(o):
            ref, oob = X.O.aggregate_rect(vol, arms, order)
            assert oob == 0
            bits_eq(o["vol_out"], ref, "vol_out")
            if disp:
                val_eq(o["disp"], X.O.wta(ref), "disp")
        return call, verify
    return make


entry("smt_crossarm_aggregate", dict(H=9, W=70, D=64, order=0), dict(H=5, W=65, D=65, order=0, disp=False),
      dict(H=7, W=66, D=7, order=1), dict(H=4, W=40, D=300, order=0), dict(H=1, W=33, D=1, order=1))(_aggregate(False))
entry("smt_crossarm_load_arm_maps", dict(H=9, W=70, D=64, order=1), dict(H=5, W=65, D=5, order=1, disp=False))(_aggregate(True))


# ================================================================================================ CBLSM helpers
@entry("smt_cblsm_ad", dict(H=1, W=63, D=64, view=VL), dict(H=3, W=65, D=65, view=VR), dict(H=2, W=9, D=300, view=VL),
       dict(H=3, W=33, D=1, view=VR))
def _cblsm_ad(A, X, H, W, D, view):
    L, R = rb((H, W), 40), rb((H, W), 41)
    A.inp("L", L); A.inp("R", R); A.out("vol", (H, W, D), np.float32)
    return (lambda: X.lib.smt_cblsm_ad(A.ptr("L"), A.ptr("R"), H, W, D, view, A.ptr("vol"), X.st()),
            lambda o: bits_eq(o["vol"], X.O.cblsm_ad(L, R, D, view - 1), "vol"))


def _cblsm_arms(X, H, W, seed):
    L, R = VC.noisy_pair(H, W, seed)
    aL = X.O.arms_all(L, 25, 6, 17, 34, chain=False, right_row_bug=False)
    aR = X.O.arms_all(R, 25, 6, 17, 34, chain=False, right_row_bug=False)
    return L, R, [a.astype(np.int32) for a in aL], [a.astype(np.int32) for a in aR]


@entry("smt_cblsm_choose_arm_length", *[dict(H=h, W=w, D=d, dirn=k) for k in range(4) for h, w, d in ((7, 65, 65), (1, 33, 1))],
       dict(H=5, W=20, D=300, dirn=0))
def _choose(A, X, H, W, D, dirn):
    _, _, aL, aR = _cblsm_arms(X, H, W, 42)
    A.inp("own", aL[dirn]); A.inp("RL", aR[0]); A.inp("RR", aR[1])
    if dirn >= 2:
        A.inp("vert", aR[dirn])
    A.out("armvol", (H, W, D), np.int32)
    return (lambda: X.lib.smt_cblsm_choose_arm_length(dirn, A.ptr("own"), A.ptr("vert" if dirn >= 2 else None), A.ptr("RL"),
                                                      A.ptr("RR"), H, W, D, A.ptr("armvol"), X.st()),
            lambda o: val_eq(o["armvol"], X.O.choose_arm_length(dirn, aL[dirn], aR[dirn] if dirn >= 2 else None, aR[0], aR[1], D),
                             "arm volume"))


@entry("smt_cblsm_cost_aggregation_new", dict(H=7, W=33, D=9, win=1), dict(H=1, W=65, D=65, win=2))
def _agg_new(A, X, H, W, D, win):
    L, R, aL, aR = _cblsm_arms(X, H, W, 43)
    vols = [X.O.choose_arm_length(k, aL[k], aR[k] if k >= 2 else None, aR[0], aR[1], D) for k in range(4)]
    Lp, Rp = np.pad(L, win + 1, mode="edge"), np.pad(R, win + 1, mode="edge")
    A.inp("Lp", Lp); A.inp("Rp", Rp)
    for k, v in enumerate(vols):
        A.inp(f"av{k}", v.astype(np.int32))
    A.out("cost", (H, W, D), np.float32)
    return (lambda: X.lib.smt_cblsm_cost_aggregation_new(A.ptr("Lp"), A.ptr("Rp"), H, W, D, win, *[A.ptr(f"av{k}") for k in range(4)],
                                                         A.ptr("cost"), X.st()),
            lambda o: bits_eq(o["cost"], X.O.cblsm_cost_aggregation_new(Lp, Rp, win, *vols), "cost"))


@entry("smt_cblsm_cost_aggregation_v4", dict(H=7, W=9, D=5), dict(H=5, W=6, D=1, disp=False), dict(H=3, W=8, D=65),
       dict(H=1, W=5, D=300))
def _agg_v4(A, X, H, W, D, disp=True):
    vol = (np.random.default_rng(H * 100 + D).standard_normal((H, W, D)) * 37.0).astype(np.float32)
    vols = VC.random_arm_volumes(H, W, D, seed=D)
    A.inp("vol_in", vol)
    for k, v in enumerate(vols):
        A.inp(f"av{k}", v)
    A.out("vol_out", (H, W, D), np.float32)
    A.inout("ub", np.zeros(1, np.int32))
    if disp:
        A.out("disp", (H, W), np.float32)

    def verify(o):
        ref = VC.v4_numpy(vol, *vols)
        assert VC.same_volume(o["vol_out"], ref), "vol_out"
        assert int(o["ub"][0]) == 0
        if disp:
            val_eq(o["disp"], VC.disp_origin(ref), "disp")
    return (lambda: X.lib.smt_cblsm_cost_aggregation_v4(A.ptr("vol_in"), *[A.ptr(f"av{k}") for k in range(4)], H, W, D,
                                                        A.ptr("vol_out"), A.ptr("disp" if disp else None), A.ptr("ub"), X.st()),
            verify)


# ================================================================================================ scanline
def _scan_ref(O, cost, gray, which, fixed):
    """the vertical passes under SMT_QUIRK_FIX_SCAN_VERTICAL are the horizontal passes of the transposed volume and
    guide (tests/test_quirks_gpu.py's rule)"""
    if fixed and which in ("up", "down"):
        t = O.scan_pass(np.ascontiguousarray(cost.transpose(1, 0, 2)), np.ascontiguousarray(gray.T), 10, 150,
                        "left" if which == "up" else "right")
        return np.ascontiguousarray(t.transpose(1, 0, 2))
    return O.scan_pass(cost, gray, 10, 150, which)


def _scanline(run):
    def make(A, X, H, W, D, quirks=0, disp=True):
        rng = np.random.default_rng([H, W, D])
        cost = rng.integers(0, 8, (H, W, D)).astype(np.float32)
        gray = rng.integers(0, 256, (H, W)).astype(np.float32)
        A.inp("vol_in", cost); A.inp("gray", gray)
        names = ("left", "right", "up", "down")
        if run:
            A.out("vol_out", (H, W, D), np.float32)
            if disp:
                A.out("disp", (H, W), np.float32)
        else:
            for nm in names:
                A.out(nm, (H, W, D), np.float32)

        def call():
            h = C.c_void_p()
            rc = X.lib.smt_scanline_create_on(X.dev_index, H, W, D, 10, 150, C.byref(h))
            try:
                rc = rc or X.lib.smt_scanline_set_stream(h, X.st()) or X.lib.smt_scanline_set_quirks(h, u32(quirks))
                if run:
                    return rc or X.lib.smt_scanline_run(h, A.ptr("vol_in"), A.ptr("gray"), A.ptr("vol_out"), A.ptr("disp" if disp else None))
                for k, nm in enumerate(names):
                    rc = rc or X.lib.smt_scanline_pass(h, A.ptr("vol_in"), A.ptr("gray"), k, A.ptr(nm))
                X.sync()
                return rc
            finally:
                X.sync()
                X.lib.smt_scanline_destroy(h)

        def verify(o):
            p = [_scan_ref(X.O, cost, gray, nm, bool(quirks & 4)) for nm in names]
            if not run:
                for nm, r in zip(names, p):
                    bits_eq(o[nm], r, nm)
                return
            ref = ((p[0] + p[1]) + p[2]) + p[3]
            if not quirks:
                bits_eq(ref, X.O.scanline(cost, gray, 10, 150), "oracle passes against oracle sum")
            bits_eq(o["vol_out"], ref, "vol_out")
            if disp:
                val_eq(o["disp"], X.O.wta(ref), "disp")
        return call, verify
    return make


_SCAN = [dict(H=1, W=9, D=1), dict(H=5, W=7, D=64), dict(H=3, W=6, D=65), dict(H=4, W=5, D=320),
         dict(H=5, W=7, D=64, quirks=4), dict(H=3, W=6, D=65, quirks=4), dict(H=4, W=5, D=320, quirks=4)]
entry("smt_scanline_run", *_SCAN, dict(H=3, W=6, D=65, disp=False))(_scanline(True))
entry("smt_scanline_pass", *_SCAN)(_scanline(False))


# ================================================================================================ pipeline
def _pipeline(post):
    def make(A, X, H, W, D, P, counts=True, last=True):
        Ls = np.stack([VC.noisy_pair(H, W, 50 + b)[0] for b in range(P)])
        Rs = np.stack([VC.noisy_pair(H, W, 50 + b)[1] for b in range(P)])
        A.inp("L", Ls); A.inp("R", Rs)
        A.out("dispL", (P, H, W), np.float32); A.out("dispR", (P, H, W), np.float32); A.out("cls", (P, H, W), np.uint8)
        if counts:
            A.out("counts", (P, 2), np.int32)
        if post and last:
            A.out("last", (P, H, W), np.float32)

        def call():
            p, q, h = X.L.PipelineParams(), X.L.PostParams(), C.c_void_p()
            X.lib.smt_pipeline_default_params(C.byref(p)); X.lib.smt_post_default_params(C.byref(q))
            q.speckle_min_area = 5
            rc = X.lib.smt_pipeline_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
            try:
                rc = rc or X.lib.smt_pipeline_set_stream(h, X.st())
                args = (h, A.ptr("L"), A.ptr("R"), P, A.ptr("dispL"), A.ptr("dispR"), A.ptr("cls"), A.ptr("counts" if counts else None))
                if post:
                    rc = rc or X.lib.smt_pipeline_run_batch_post(*args, C.byref(q), A.ptr("last" if last else None))
                else:
                    rc = rc or X.lib.smt_pipeline_run_batch(*args)
                st = X.lib.smt_pipeline_status(h)
                return rc or (0 if st == SMT_ERR_REF_UB else st)          # as tests/test_post_batch_gpu.py
            finally:
                X.lib.smt_pipeline_destroy(h)

        def verify(o):
            from test_post_batch_gpu import oracle_pipeline
            O = X.O
            for b in range(P):
                L, R = Ls[b], Rs[b]
                lr = oracle_pipeline(O, L, R, D)
                ar, _ = O.aggregate_rect(O.adcensus_view(L, R, D, 10.0, 30.0, 1), O.arms_all(R), 0)
                al, _ = O.aggregate_rect(O.adcensus_view(L, R, D, 10.0, 30.0, 0), O.arms_all(L), 0)
                d_r = O.wta(ar)
                lr2, cls, no, nm = O.lrcheck(O.wta(O.scanline(al, L.astype(np.float32), 10, 150)), d_r, 2)
                bits_eq(lr2, lr, "oracle")
                val_eq(o["dispR"][b], d_r, f"dispR[{b}]"); bits_eq(o["cls"][b], cls, f"cls[{b}]")
                if counts:
                    assert tuple(o["counts"][b]) == (no, nm), ("counts", b)
                if post:
                    sp = O.remove_speckles(lr, 1, 5, INT_MIN)
                    bits_eq(o["dispL"][b], sp, f"dispL[{b}]")
                    if last:
                        bits_eq(o["last"][b], O.median(sp, 3), f"lastDisp[{b}]")
                else:
                    bits_eq(o["dispL"][b], lr, f"dispL[{b}]")
        return call, verify
    return make


entry("smt_pipeline_run_batch", dict(H=5, W=65, D=64, P=2), dict(H=3, W=40, D=65, P=1, counts=False),
      dict(H=1, W=33, D=1, P=2), dict(H=3, W=20, D=300, P=1))(_pipeline(False))
entry("smt_pipeline_run_batch_post", dict(H=5, W=65, D=64, P=2), dict(H=3, W=40, D=65, P=1, counts=False, last=False),
      dict(H=1, W=33, D=1, P=2))(_pipeline(True))


# ================================================================================================ CBLSM flows
def _cblsm_flow(kind):
    def make(A, X, H, W, D, P, counts=True):
        Ls = np.stack([VC.noisy_pair(H, W, 60 + b)[0] for b in range(P)])
        Rs = np.stack([VC.noisy_pair(H, W, 60 + b)[1] for b in range(P)])
        A.inp("L", Ls); A.inp("R", Rs); A.out("dispL", (P, H, W), np.float32)
        if kind != "v4":
            A.out("dispR", (P, H, W), np.float32)
        if kind == "post":
            A.out("cls", (P, H, W), np.uint8)
            if counts:
                A.out("counts", (P, 2), np.int32)

        def call():
            p, h = X.L.CBLSMParams(), C.c_void_p()
            X.lib.smt_cblsm_default_params(C.byref(p))
            rc = X.lib.smt_cblsm_flow_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
            try:
                rc = rc or X.lib.smt_cblsm_flow_set_stream(h, X.st())
                if kind == "v4":
                    rc = rc or X.lib.smt_cblsm_flow_run_batch_v4(h, A.ptr("L"), A.ptr("R"), P, A.ptr("dispL"))
                elif kind == "post":
                    rc = rc or X.lib.smt_cblsm_flow_run_batch_post(h, A.ptr("L"), A.ptr("R"), P, A.ptr("dispL"), A.ptr("dispR"), A.ptr("cls"),
                                                                   A.ptr("counts" if counts else None), None)
                else:
                    rc = rc or X.lib.smt_cblsm_flow_run_batch(h, A.ptr("L"), A.ptr("R"), P, A.ptr("dispL"), A.ptr("dispR"))
                return rc or X.lib.smt_cblsm_flow_status(h)
            finally:
                X.lib.smt_cblsm_flow_destroy(h)

        def verify(o):
            from test_cblsm_flow_gpu import _oracle
            from test_cblsm_post_gpu import _chain
            for b in range(P):
                if kind == "v4":
                    ref = VC.v4_numpy(X.O.cblsm_ad(Ls[b], Rs[b], D, 0), *VC.oracle_arm_volumes(X.O, Ls[b], Rs[b], D))
                    val_eq(o["dispL"][b], VC.disp_origin(ref), f"dispL[{b}]")
                    continue
                _, _, dl, dr = _oracle(X.O, Ls[b], Rs[b], D)
                val_eq(o["dispR"][b], dr, f"dispR[{b}]")
                if kind == "post":
                    _, _, fin, cls, cnt = _chain(X.O, dl, dr)
                    assert MC.same_bits(o["dispL"][b], fin), f"dispL[{b}]"
                    bits_eq(o["cls"][b], cls, f"cls[{b}]")
                    if counts:
                        assert tuple(o["counts"][b]) == cnt, ("counts", b)
                else:
                    val_eq(o["dispL"][b], dl, f"dispL[{b}]")
        return call, verify
    return make


_FLOW = [dict(H=5, W=65, D=64, P=2), dict(H=3, W=33, D=65, P=1), dict(H=1, W=20, D=1, P=2), dict(H=3, W=17, D=300, P=1)]
entry("smt_cblsm_flow_run_batch", *_FLOW)(_cblsm_flow("run"))
entry("smt_cblsm_flow_run_batch_v4", dict(H=5, W=17, D=20, P=2), dict(H=3, W=9, D=65, P=1), dict(H=1, W=9, D=1, P=2))(_cblsm_flow("v4"))
entry("smt_cblsm_flow_run_batch_post", *_FLOW[:3], dict(H=3, W=33, D=65, P=1, counts=False))(_cblsm_flow("post"))


# ================================================================================================ CrossAggregator
def _bgr_of(gray, seed):
    n = rb(gray.shape + (3,), seed, 0, 4).astype(np.int32)
    return np.clip(gray[..., None].astype(np.int32) + n - 2, 0, 255).astype(np.uint8)


@entry("smt_crossagg_aggregate", dict(H=5, W=65, D=64, iters=4), dict(H=3, W=17, D=65, iters=1), dict(H=1, W=33, D=1, iters=2),
       dict(H=3, W=17, D=300, iters=2))
def _crossagg(A, X, H, W, D, iters):
    bgr = _bgr_of(VC.noisy_pair(H, W, 70)[0], 71)
    cost = rf((H, W, D), 72)
    A.inp("img", bgr); A.inp("cost", cost)

    def call():
        h, p, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = X.lib.smt_crossagg_create_on(X.dev_index, W, H, D, C.byref(h))
        try:
            rc = rc or X.lib.smt_crossagg_set_stream(h, X.st())
            rc = rc or X.lib.smt_crossagg_aggregate(h, A.ptr("img"), A.ptr("cost"), iters)
            rc = rc or X.lib.smt_crossagg_cost(h, C.byref(p)) or X.lib.smt_crossagg_arms(h, C.byref(q))
            if not rc:
                A.extra["agg"] = X.d2h(p, (H, W, D), np.float32)
                A.extra["arms"] = X.d2h(q, (H, W, 4), np.uint8)
            return rc
        finally:
            X.lib.smt_crossagg_destroy(h)

    def verify(o):
        a_ref, c_ref = X.O.crossagg(bgr, cost, iters=iters)
        bits_eq(o["arms"], a_ref, "arms"); bits_eq(o["agg"], c_ref, "aggregated volume")
    return call, verify


@entry("smt_adcensus_option_aggregate", dict(H=5, W=65, D=64), dict(H=3, W=17, D=65, disp=False), dict(H=1, W=33, D=1))
def _option(A, X, H, W, D, disp=True):
    bgr = _bgr_of(VC.noisy_pair(H, W, 73)[0], 74)
    cost = rf((H, W, D), 75)
    A.inp("img", bgr); A.inp("cost", cost); A.out("cost_out", (H, W, D), np.float32)
    if disp:
        A.out("disp", (H, W), np.float32)

    def call():
        o = X.L.ADCensusOption()
        X.lib.smt_adcensus_option_default(C.byref(o))
        o.min_disparity, o.max_disparity = 0, D
        return X.lib.smt_adcensus_option_aggregate(C.byref(o), A.ptr("img"), A.ptr("cost"), W, H, 4, A.ptr("cost_out"),
                                                   A.ptr("disp" if disp else None), X.st())

    def verify(o):
        _, ref = X.O.crossagg(bgr, cost, iters=4)
        bits_eq(o["cost_out"], ref, "cost_out")
        if disp:
            val_eq(o["disp"], X.O.wta(ref), "disp")
    return call, verify


def _crossagg_flow(post):
    def make(A, X, H, W, D, P, gray=True, cls=True, counts=True, views=VB):
        Ls = np.stack([VC.noisy_pair(H, W, 80 + b)[0] for b in range(P)])
        Rs = np.stack([VC.noisy_pair(H, W, 80 + b)[1] for b in range(P)])
        bL, bR = _bgr_of(Ls, 81), _bgr_of(Rs, 82)
        if not gray:
            Ls, Rs = np.stack([X.O.bgr2gray(b) for b in bL]), np.stack([X.O.bgr2gray(b) for b in bR])
        A.inp("bgrL", bL); A.inp("bgrR", bR)
        if gray:
            A.inp("L", Ls); A.inp("R", Rs)
        if views & VL:
            A.out("dispL", (P, H, W), np.float32)
        if views & VR:
            A.out("dispR", (P, H, W), np.float32)
        cls = cls or post
        if cls:
            A.out("cls", (P, H, W), np.uint8)
            if counts:
                A.out("counts", (P, 2), np.int32)

        def call():
            h = C.c_void_p()
            rc = X.lib.smt_crossagg_flow_create_on(X.dev_index, H, W, D, None, C.byref(h))
            try:
                rc = rc or X.lib.smt_crossagg_flow_set_stream(h, X.st())
                args = (h, A.ptr("bgrL"), A.ptr("bgrR"), A.ptr("L" if gray else None), A.ptr("R" if gray else None), P)
                outs = (A.ptr("dispL" if views & VL else None), A.ptr("dispR" if views & VR else None), A.ptr("cls" if cls else None),
                        A.ptr("counts" if cls and counts else None))
                if post:
                    rc = rc or X.lib.smt_crossagg_flow_run_batch_post(*args, *outs, None)
                else:
                    rc = rc or X.lib.smt_crossagg_flow_run_batch(*args, views, *outs)
                return rc or X.lib.smt_crossagg_flow_status(h)
            finally:
                X.lib.smt_crossagg_flow_destroy(h)

        def verify(o):
            from test_crossagg_flow_gpu import _expect
            from test_cblsm_post_gpu import _chain
            for b in range(P):
                dl = _expect(X.O, bL[b], Ls[b], Rs[b], D, 0)[1] if views & VL else None
                dr = _expect(X.O, bR[b], Ls[b], Rs[b], D, 1)[1] if views & VR else None
                if views & VR:
                    val_eq(o["dispR"][b], dr, f"dispR[{b}]")
                if post:
                    _, _, fin, c, cnt = _chain(X.O, dl, dr)
                    assert MC.same_bits(o["dispL"][b], fin), f"dispL[{b}]"
                elif cls:
                    lr, c, no, nm = X.O.lrcheck(dl, dr, 5)
                    cnt = (no, nm)
                    bits_eq(o["dispL"][b], lr, f"dispL[{b}]")
                elif views & VL:
                    val_eq(o["dispL"][b], dl, f"dispL[{b}]")
                if cls:
                    bits_eq(o["cls"][b], c, f"cls[{b}]")
                    if counts:
                        assert tuple(o["counts"][b]) == cnt, ("counts", b)
        return call, verify
    return make


entry("smt_crossagg_flow_run_batch", dict(H=5, W=65, D=64, P=2), dict(H=3, W=33, D=65, P=1, gray=False, counts=False),
      dict(H=1, W=20, D=1, P=2, cls=False), dict(H=3, W=17, D=300, P=1, cls=False, views=VL),
      dict(H=3, W=17, D=16, P=1, cls=False, views=VR))(_crossagg_flow(False))
entry("smt_crossagg_flow_run_batch_post", dict(H=5, W=65, D=64, P=2), dict(H=3, W=33, D=65, P=1, gray=False, counts=False),
      dict(H=1, W=20, D=1, P=2))(_crossagg_flow(True))


# ================================================================================================ LR check, filling
def _lr_maps(H, W, seed):
    rng = np.random.default_rng([seed, H, W])
    dL = rng.integers(0, 24, (H, W)).astype(np.float32)
    dR = rng.integers(0, 24, (H, W)).astype(np.float32)
    dL[rng.random((H, W)) < 0.05] = np.inf
    return dL, dR


@entry("smt_lrcheck", dict(H=1, W=63), dict(H=5, W=257), dict(H=3, W=65, counts=False))
def _lrcheck(A, X, H, W, counts=True):
    dL, dR = _lr_maps(H, W, 90)
    A.inout("dispL", dL); A.inp("dispR", dR); A.out("cls", (H, W), np.uint8)
    if counts:
        A.out("counts", (2,), np.int32)

    def verify(o):
        ref, cls, no, nm = X.O.lrcheck(dL, dR, 2)
        bits_eq(o["dispL"], ref, "dispL"); bits_eq(o["cls"], cls, "cls")
        if counts:
            assert tuple(o["counts"]) == (no, nm)
    return (lambda: X.lib.smt_lrcheck(A.ptr("dispL"), A.ptr("dispR"), H, W, 2, A.ptr("cls"), A.ptr("counts" if counts else None), X.st()),
            verify)


@entry("smt_lrcheck_variant", dict(H=1, W=63), dict(H=5, W=257), dict(H=3, W=65, counts=False))
def _lrvariant(A, X, H, W, counts=True):
    dL, dR = _lr_maps(H, W, 91)
    dL[0, ::7] = np.nan; dR[0, 3::11] = -4e9; dL[H - 1, 1::5] += 0.5
    A.inp("dispL", dL); A.inp("dispR", dR); A.out("last", (H, W), np.float32); A.out("cls", (H, W), np.uint8)
    if counts:
        A.out("counts", (2,), np.int32)

    def verify(o):
        ref, cls, no, nm = X.O.lrcheck_variant(dL, dR, 1.5)
        bits_eq(o["last"], ref, "lastDisp"); bits_eq(o["cls"], cls, "cls")
        if counts:
            assert tuple(o["counts"]) == (no, nm)
    return (lambda: X.lib.smt_lrcheck_variant(A.ptr("dispL"), A.ptr("dispR"), A.ptr("last"), H, W, f32(1.5), A.ptr("cls"),
                                              A.ptr("counts" if counts else None), X.st()), verify)


@entry("smt_fill_the_hole", dict(row=9, col=33, D=8), dict(row=1, col=50, D=4), dict(row=33, col=33, D=1))
def _fill(A, X, row, col, D):
    d, cls = FC.lr_case(X.O, row, col, 5)
    occ, mis = FC.lists(cls)
    A.inout("disp", d)

    def call():
        third, nt = np.empty((row * col, 2), np.int32), C.c_int(-1)
        o, m = np.ascontiguousarray(occ), np.ascontiguousarray(mis)
        rc = X.lib.smt_fill_the_hole(A.ptr("disp"), row, col, D, o.ctypes.data_as(C.c_void_p), len(o), m.ctypes.data_as(C.c_void_p),
                                     len(m), third.ctypes.data_as(C.c_void_p), C.byref(nt), X.st())
        A.extra["n_third"] = np.array([nt.value], np.int32)
        return rc

    def verify(o):
        ref, st, _ = FC.expected(X.O, d, cls, D)
        bits_eq(o["disp"], ref, "disp")
        assert int(o["n_third"][0]) == st[2]
    return call, verify


def _fill_batch(host):
    def make(A, X, row, col, D, P, gap=0, status=True):
        cases = [FC.lr_case(X.O, row, col, 7 + b) for b in range(P)]
        d, cls = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
        ds = row * col + gap if gap else 0
        A.inout("disp", d, stride=ds); A.inp("cls", cls, stride=ds)
        if status:
            A.out("status", (P, 4), np.int32)

        def call():
            args = (A.ptr("disp"), A.ptr("cls"), P, sz(ds), sz(ds), row, col, D, A.ptr("status" if status else None))
            if host:
                return X.lib.smt_fill_the_hole_batch_host(*args)
            return X.lib.smt_fill_the_hole_batch(*args, X.st())

        def verify(o):
            for b in range(P):
                ref, st, _ = FC.expected(X.O, d[b], cls[b], D)
                bits_eq(o["disp"][b], ref, f"disp[{b}]")
                if status:
                    assert o["status"][b].tolist() == st, ("status", b)
        return call, verify
    return make


_FILL = [dict(row=9, col=33, D=8, P=3), dict(row=9, col=33, D=8, P=3, gap=7), dict(row=1, col=50, D=4, P=2, gap=7, status=False),
         dict(row=33, col=33, D=1, P=1)]
entry("smt_fill_the_hole_batch", *_FILL)(_fill_batch(False))
entry("smt_fill_the_hole_batch_host", *_FILL)(_fill_batch(True))


# ================================================================================================ SAD
def _padded(H, W, w, seed):
    L, R = rb((H, W), seed), rb((H, W), seed + 1)
    R[:, :max(W - 3, 0)] = np.where(rb((H, W), seed + 2)[:, :max(W - 3, 0)] < 200, L[:, 3:], R[:, :max(W - 3, 0)])   # mostly L shifted by 3
    return L, R, np.pad(L, w, mode="edge"), np.pad(R, w, mode="edge")


# (H, W, D, winsize): 32-pixel strips -- below, at + 1; (W + 2w) % 4 = 1, 2, 3; H = 1; every slot count; 3x3 (impl 1 only)
_SAD_SHAPES = [(1, 31, 1, 1), (3, 33, 64, 1), (5, 29, 65, 2), (3, 34, 20, 3), (2, 40, 300, 1), (3, 30, 16, 0)]


@entry("smt_sad", *[dict(H=h, W=w, D=d, ws=k, view=v, impl=i) for h, w, d, k in _SAD_SHAPES for v in (VL, VR) for i in (2, 1)])
def _sad(A, X, H, W, D, ws, view, impl):
    _, _, Lp, Rp = _padded(H, W, ws + 1, 100)
    A.inp("Lp", Lp); A.inp("Rp", Rp); A.out("disp", (H, W), np.int32)

    def call():
        X.lib.smt_sad_set_impl(impl)
        try:
            rc = X.lib.smt_sad(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, view, A.ptr("disp"), X.st())
            X.sync()
            return rc
        finally:
            X.lib.smt_sad_set_impl(2)
    return call, lambda o: val_eq(o["disp"], X.O.sad(Lp, Rp, D, ws, view - 1), "disp")


@entry("smt_sad_both", *[dict(H=h, W=w, D=d, ws=k, dispatch=m, impl=i, cost=c) for h, w, d, k in _SAD_SHAPES[:5]
                         for m, i in ((1, 2), (1, 1), (2, 2)) for c in (False, True)],
       dict(H=7, W=33, D=64, ws=1, dispatch=1, impl=2, cost=True, band=3), dict(H=7, W=33, D=64, ws=1, dispatch=0, impl=2, cost=False))
def _sad_both(A, X, H, W, D, ws, dispatch, impl, cost, band=0):
    _, _, Lp, Rp = _padded(H, W, ws + 1, 101)
    A.inp("Lp", Lp); A.inp("Rp", Rp); A.out("dispL", (H, W), np.int32); A.out("dispR", (H, W), np.int32)
    if cost:
        A.out("costL", (H, W, D), np.float32)

    def call():
        lib = X.lib
        lib.smt_sad_both_set_dispatch(dispatch); lib.smt_sad_both_set_impl(impl); lib.smt_sad_both_set_band(band)
        try:
            rc = lib.smt_sad_both(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, A.ptr("dispL"), A.ptr("dispR"), A.ptr("costL" if cost else None), X.st())
            X.sync()
            A.extra["form"] = np.array([lib.smt_sad_both_last_form()], np.int32)
            return rc
        finally:
            lib.smt_sad_both_set_dispatch(0); lib.smt_sad_both_set_impl(2); lib.smt_sad_both_set_band(0)

    def verify(o):
        from test_sad_both_cpu import left_costs
        if dispatch:
            assert int(o["form"][0]) == {(1, 2): 2, (1, 1): 3, (2, 2): 1}[(dispatch, impl)], "the hooks must select the form"
        val_eq(o["dispL"], X.O.sad(Lp, Rp, D, ws, 0), "dispL"); val_eq(o["dispR"], X.O.sad(Lp, Rp, D, ws, 1), "dispR")
        if cost:
            val_eq(o["costL"], left_costs(Lp, Rp, D, ws), "costL")
    return call, verify


def _strided(stride_kind, dense_elems):
    return 0 if not stride_kind else dense_elems + 7


@entry("smt_sad_batch", *[dict(H=3, W=33, D=65, ws=1, view=v, gap=g) for v in (VL, VR) for g in (0, 1)], dict(H=1, W=31, D=1, ws=2, view=VL, gap=1))
def _sad_batch(A, X, H, W, D, ws, view, gap, P=3):
    pads = [_padded(H, W, ws + 1, 110 + 3 * b) for b in range(P)]
    Lp, Rp = np.stack([p[2] for p in pads]), np.stack([p[3] for p in pads])
    si, sd = _strided(gap, Lp[0].size), _strided(gap, H * W)
    A.inp("Lp", Lp, stride=si); A.inp("Rp", Rp, stride=si); A.out("disp", (P, H, W), np.int32, stride=sd)

    def verify(o):
        for b in range(P):
            val_eq(o["disp"][b], X.O.sad(Lp[b], Rp[b], D, ws, view - 1), f"disp[{b}]")
    return (lambda: X.lib.smt_sad_batch(A.ptr("Lp"), A.ptr("Rp"), P, sz(si), H, W, D, ws, view, A.ptr("disp"), sz(sd), X.st()), verify)


@entry("smt_sad_crosscheck", dict(H=1, W=63), dict(H=5, W=257))
def _sad_cc(A, X, H, W):
    rng = np.random.default_rng([120, H, W])
    dL, dR = rng.integers(0, 9, (H, W)).astype(np.int32), rng.integers(0, 9, (H, W)).astype(np.int32)
    A.inp("dL", dL); A.inp("dR", dR); A.out("out", (H, W), np.int32); A.out("cls", (H, W), np.uint8)

    def verify(o):
        ro, rc = X.O.sad_crosscheck(dL, dR)
        val_eq(o["out"], ro, "out"); val_eq(o["cls"], rc, "cls")
    return (lambda: X.lib.smt_sad_crosscheck(A.ptr("dL"), A.ptr("dR"), H, W, A.ptr("out"), A.ptr("cls"), X.st()), verify)


@entry("smt_sad_flow_run_batch", dict(H=3, W=33, D=65, ws=1, P=2), dict(H=1, W=31, D=1, ws=2, P=2, outs=("dispL", "lastdisp")),
       dict(H=5, W=34, D=300, ws=3, P=1))
def _sad_flow(A, X, H, W, D, ws, P, outs=("dispL", "dispR", "lastdisp", "cls")):
    imgs = [_padded(H, W, ws + 1, 130 + 3 * b) for b in range(P)]
    A.inp("L", np.stack([i[0] for i in imgs])); A.inp("R", np.stack([i[1] for i in imgs]))
    for nm in outs:
        A.out(nm, (P, H, W), np.uint8 if nm == "cls" else np.int32)

    def call():
        p, h = X.L.SADParams(), C.c_void_p()
        p.winsize = ws
        rc = X.lib.smt_sad_flow_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
        try:
            rc = rc or X.lib.smt_sad_flow_set_stream(h, X.st())
            rc = rc or X.lib.smt_sad_flow_run_batch(h, A.ptr("L"), A.ptr("R"), P, *[A.ptr(nm if nm in outs else None)
                                                                                  for nm in ("dispL", "dispR", "lastdisp", "cls")])
            X.sync()
            return rc
        finally:
            X.lib.smt_sad_flow_destroy(h)

    def verify(o):
        for b in range(P):
            dl, dr = X.O.sad(imgs[b][2], imgs[b][3], D, ws, 0), X.O.sad(imgs[b][2], imgs[b][3], D, ws, 1)
            ro, rc = X.O.sad_crosscheck(dl, dr)
            for nm, ref in (("dispL", dl), ("dispR", dr), ("lastdisp", ro), ("cls", rc)):
                if nm in outs:
                    val_eq(o[nm][b], ref, f"{nm}[{b}]")
    return call, verify


# ================================================================================================ NCC
# 16-pixel workgroups: interior widths below, at + 1; H = 1 interior row; every slot count
_NCC_SHAPES = [(3, 17, 1, 1), (5, 19, 64, 1), (7, 37, 65, 2), (3, 21, 300, 1), (5, 40, 20, 0), (4, 9, 5, 3), (6, 22, 33, 2)]


def _ncc_check(X, o, L, R, D, win, impl, cost, name="disp", cname="cost"):
    H, W = L.shape
    if cost and H > 2 * win and W > 2 * win:
        exact, flat, sentinel = XM.ncc_exact(L, R, D, win)
        XM.check_ncc(o[cname], exact, flat, sentinel, win, XM.ncc_form(win, impl))
        val_eq(o[name], XM.ncc_wta(o[cname], win), "the map is WinTakeAll of the call's own costs")
    val_eq(o[name], X.O.ncc(L, R, D, win), name)


@entry("smt_ncc", *[dict(H=h, W=w, D=d, win=k, impl=i, cost=c) for h, w, d, k in _NCC_SHAPES for i in (2, 1) for c in (False, True)])
def _ncc(A, X, H, W, D, win, impl, cost):
    L, R = _padded(H, W, 0, 140)[:2]
    A.inp("L", L); A.inp("R", R); A.out("disp", (H, W), np.int32)
    if cost:
        A.out("cost", (H, W, D), np.float64)

    def call():
        X.lib.smt_ncc_set_impl(impl)
        try:
            rc = X.lib.smt_ncc(A.ptr("L"), A.ptr("R"), H, W, D, win, A.ptr("disp"), A.ptr("cost" if cost else None), X.st())
            X.sync()
            return rc
        finally:
            X.lib.smt_ncc_set_impl(2)
    return call, lambda o: _ncc_check(X, o, L, R, D, win, impl, cost)


@entry("smt_ncc_batch", dict(H=5, W=19, D=65, win=1, gap=0), dict(H=5, W=19, D=65, win=1, gap=1), dict(H=3, W=17, D=1, win=1, gap=1))
def _ncc_batch(A, X, H, W, D, win, gap, P=3):
    imgs = [_padded(H, W, 0, 150 + 3 * b)[:2] for b in range(P)]
    s = _strided(gap, H * W)
    A.inp("L", np.stack([i[0] for i in imgs]), stride=s); A.inp("R", np.stack([i[1] for i in imgs]), stride=s)
    A.out("disp", (P, H, W), np.int32, stride=s)

    def verify(o):
        for b in range(P):
            val_eq(o["disp"][b], X.O.ncc(imgs[b][0], imgs[b][1], D, win), f"disp[{b}]")
    return (lambda: X.lib.smt_ncc_batch(A.ptr("L"), A.ptr("R"), P, sz(s), H, W, D, win, A.ptr("disp"), sz(s), X.st()), verify)


# ================================================================================================ ASW
# (H, W, D, winSize): 16- / 32-pixel workgroups; (W + 2 wins) % 4 = 1, 2, 3; H = 1; D = 1, 64, 65, > 256 (the carried WinTakeAll)
_ASW_SHAPES = [(1, 15, 1, 1), (3, 33, 64, 1), (2, 17, 65, 2), (2, 18, 300, 1), (3, 4, 4, 2)]


def _asw_tables(A, X, ws):
    sp, cm = X.O.asw_masks(ws, 50.0, 30.0)
    A.inp("space", sp); A.inp("color", cm)
    return sp, cm


def _asw_check(X, o, Lp, Rp, D, ws, sp, cm, view, cost, name="disp", cname="cost"):
    H, W = Lp.shape[0] - 2 * ws - 2, Lp.shape[1] - 2 * ws - 2
    if cost:
        XM.check_asw(o[cname], XM.asw_exact(Lp, Rp, D, ws, sp, cm, 40, view), ws, XM.asw_nan_mask(H, W, D, ws, view))
        val_eq(o[name], XM.asw_wta(o[cname]), "the map is WinTakeAll of the call's own costs")
    else:
        _asw_map_check(X, o[name], Lp, Rp, D, ws, sp, cm, view, name)


def _asw_map_check(X, got, Lp, Rp, D, ws, sp, cm, view, name):
    """without the call's costs: the oracle's map wherever its two smallest costs are more than 2 float ulps apart
    (tests/test_matchers_gpu.py's rule)"""
    rd, rc = X.O.asw(Lp, Rp, D, ws, sp, cm, 40, view, want_cost=True)
    srt = np.sort(np.where(np.isnan(rc), np.float32(np.inf), rc), axis=2)
    if D > 1:
        with np.errstate(invalid="ignore"):
            tie = (srt[..., 1] - srt[..., 0]).astype(np.float64) <= 2.0 * np.spacing(srt[..., 0]).astype(np.float64)
    else:
        tie = np.zeros(rd.shape, bool)
    bad = (got != rd) & ~tie
    assert not bad.any(), f"{name}: {int(bad.sum())} pixels differ from the oracle outside the tie band"


@entry("smt_asw", *[dict(H=h, W=w, D=d, ws=k, view=v, impl=i, cost=c) for h, w, d, k in _ASW_SHAPES for v in (VL, VR)
                    for i in (0, 1, 3, 4, 5, 6) for c in (False, True)])
def _asw(A, X, H, W, D, ws, view, impl, cost):
    _, _, Lp, Rp = _padded(H, W, ws + 1, 160)
    A.inp("Lp", Lp); A.inp("Rp", Rp)
    sp, cm = _asw_tables(A, X, ws)
    A.out("disp", (H, W), np.float32)
    if cost:
        A.out("cost", (H, W, D), np.float32)

    def call():
        X.lib.smt_asw_set_impl(impl)
        try:
            rc = X.lib.smt_asw(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, A.ptr("space"), A.ptr("color"), 40, view, A.ptr("disp"),
                               A.ptr("cost" if cost else None), X.st())
            X.sync()
            return rc
        finally:
            X.lib.smt_asw_set_impl(0)
    return call, lambda o: _asw_check(X, o, Lp, Rp, D, ws, sp, cm, view - 1, cost)


@entry("smt_asw_both", *[dict(H=h, W=w, D=d, ws=k, impl=i, costs=c) for h, w, d, k in _ASW_SHAPES for i in (2, 1)
                         for c in ("", "L", "LR")], dict(H=3, W=33, D=64, ws=1, impl=2, costs="R"))
def _asw_both(A, X, H, W, D, ws, impl, costs):
    _, _, Lp, Rp = _padded(H, W, ws + 1, 161)
    A.inp("Lp", Lp); A.inp("Rp", Rp)
    sp, cm = _asw_tables(A, X, ws)
    A.out("dispL", (H, W), np.float32); A.out("dispR", (H, W), np.float32)
    for c in costs:
        A.out("cost" + c, (H, W, D), np.float32)

    def call():
        X.lib.smt_asw_both_set_impl(impl)
        try:
            rc = X.lib.smt_asw_both(A.ptr("Lp"), A.ptr("Rp"), H, W, D, ws, A.ptr("space"), A.ptr("color"), 40, A.ptr("dispL"), A.ptr("dispR"),
                                    A.ptr("costL" if "L" in costs else None), A.ptr("costR" if "R" in costs else None), X.st())
            X.sync()
            return rc
        finally:
            X.lib.smt_asw_both_set_impl(2)

    def verify(o):
        from test_asw_both_cpu import right_from_left
        _asw_check(X, o, Lp, Rp, D, ws, sp, cm, 0, "L" in costs, "dispL", "costL")
        if "L" in costs:
            cr, dr = right_from_left(o["costL"], ws + 1)           # the right view follows from the call's own left costs exactly
            val_eq(o["dispR"], dr, "dispR")
            if "R" in costs:
                nan_bits_eq(o["costR"], cr, "costR")
        elif "R" in costs:
            nanR = XM.asw_nan_mask(H, W, D, ws, 1)
            assert np.array_equal(np.isnan(o["costR"]), nanR), "costR NaN pattern"
            val_eq(o["dispR"], XM.asw_wta(o["costR"]), "dispR is WinTakeAll of costR")
        else:
            _asw_map_check(X, o["dispR"], Lp, Rp, D, ws, sp, cm, 1, "dispR")
        assert (o["dispR"][:, max(W - ws - 2, 0):] == 0).all(), "dispR is 0 in the costVolume[-1] columns"
    return call, verify


@entry("smt_asw_batch", *[dict(H=2, W=17, D=65, ws=1, view=v, gap=g) for v in (VL, VR) for g in (0, 1)])
def _asw_batch(A, X, H, W, D, ws, view, gap, P=3):
    pads = [_padded(H, W, ws + 1, 170 + 3 * b) for b in range(P)]
    Lp, Rp = np.stack([p[2] for p in pads]), np.stack([p[3] for p in pads])
    si, sd = _strided(gap, Lp[0].size), _strided(gap, H * W)
    A.inp("Lp", Lp, stride=si); A.inp("Rp", Rp, stride=si)
    sp, cm = _asw_tables(A, X, ws)
    A.out("disp", (P, H, W), np.float32, stride=sd)

    def verify(o):
        for b in range(P):
            _asw_map_check(X, o["disp"][b], Lp[b], Rp[b], D, ws, sp, cm, view - 1, f"disp[{b}]")
    return (lambda: X.lib.smt_asw_batch(A.ptr("Lp"), A.ptr("Rp"), P, sz(si), H, W, D, ws, A.ptr("space"), A.ptr("color"), 40, view,
                                        A.ptr("disp"), sz(sd), X.st()), verify)


@entry("smt_asw_crosscheck", dict(H=1, W=63), dict(H=5, W=257))
def _asw_cc(A, X, H, W):
    rng = np.random.default_rng([180, H, W])
    dL, dR = rng.integers(0, 9, (H, W)).astype(np.float32), rng.integers(0, 9, (H, W)).astype(np.float32)
    A.inp("dL", dL); A.inp("dR", dR); A.out("out", (H, W), np.uint8)
    return (lambda: X.lib.smt_asw_crosscheck(A.ptr("dL"), A.ptr("dR"), H, W, A.ptr("out"), X.st()),
            lambda o: val_eq(o["out"], X.O.asw_crosscheck(dL, dR), "out"))


@entry("smt_asw_flow_run_batch", dict(H=2, W=17, D=65, ws=1, P=2), dict(H=1, W=15, D=1, ws=2, P=2, outs=("lastDisp",)),
       dict(H=3, W=33, D=64, ws=1, P=1, outs=("dispL", "dispR")))
def _asw_flow(A, X, H, W, D, ws, P, outs=("dispL", "dispR", "lastDisp")):
    imgs = [_padded(H, W, ws + 1, 190 + 3 * b) for b in range(P)]
    A.inp("L", np.stack([i[0] for i in imgs])); A.inp("R", np.stack([i[1] for i in imgs]))
    for nm in outs:
        A.out(nm, (P, H, W), np.uint8 if nm == "lastDisp" else np.float32)
    sp, cm = X.O.asw_masks(ws, 50.0, 30.0)

    def call():
        p, h = X.L.ASWParams(), C.c_void_p()
        X.lib.smt_asw_default_params(C.byref(p))
        p.winSize, p.T, p.sigma_space, p.sigma_color = ws, 40, 50.0, 30.0
        rc = X.lib.smt_asw_flow_create_on(X.dev_index, H, W, D, C.byref(p), C.byref(h))
        try:
            rc = rc or X.lib.smt_asw_flow_set_stream(h, X.st())
            rc = rc or X.lib.smt_asw_flow_run_batch(h, A.ptr("L"), A.ptr("R"), P, *[A.ptr(nm if nm in outs else None)
                                                                                  for nm in ("dispL", "dispR", "lastDisp")])
            X.sync()
            return rc
        finally:
            X.lib.smt_asw_flow_destroy(h)

    def verify(o):
        for b in range(P):
            Lp, Rp = imgs[b][2], imgs[b][3]
            for nm, v in (("dispL", 0), ("dispR", 1)):
                if nm in outs:
                    _asw_map_check(X, o[nm][b], Lp, Rp, D, ws, sp, cm, v, f"{nm}[{b}]")
            if "lastDisp" in outs and "dispL" in outs and "dispR" in outs:
                val_eq(o["lastDisp"][b], X.O.asw_crosscheck(o["dispL"][b], o["dispR"][b]), f"lastDisp[{b}] of the call's own maps")
            elif "lastDisp" in outs:
                rl, rr = (X.O.asw(Lp, Rp, D, ws, sp, cm, 40, v) for v in (0, 1))
                val_eq(o["lastDisp"][b], X.O.asw_crosscheck(rl, rr), f"lastDisp[{b}]")
    return call, verify


# ================================================================================================ post-filters
def _disp_map(H, W, seed):
    rng = np.random.default_rng([seed, H, W])
    d = (np.add.outer(np.arange(H) // 3, np.arange(W) // 5) * 3).astype(np.float32) + rng.integers(0, 2, (H, W)).astype(np.float32)
    d[rng.random((H, W)) < 0.05] += 20
    d[rng.random((H, W)) < 0.05] = np.inf
    return d


@entry("smt_median_filter", *[dict(H=h, W=w, wnd=k) for h, w in ((1, 63), (5, 65), (3, 257)) for k in (1, 3, 7)])
def _median(A, X, H, W, wnd):
    d = _disp_map(H, W, 200)
    A.inp("in", d); A.out("out", (H, W), np.float32)
    return (lambda: X.lib.smt_median_filter(A.ptr("in"), A.ptr("out"), W, H, wnd, X.st()),
            lambda o: bits_eq(o["out"], X.O.median(d, wnd), "out"))


@entry("smt_median_filter_batch", *[dict(H=5, W=65, wnd=k, gap=g) for k in (3, 5) for g in (0, 1)], dict(H=1, W=63, wnd=7, gap=1))
def _median_batch(A, X, H, W, wnd, gap, P=3):
    d = np.stack([_disp_map(H, W, 210 + b) for b in range(P)])
    s = _strided(gap, H * W)
    A.inp("in", d, stride=s); A.out("out", (P, H, W), np.float32, stride=s)

    def verify(o):
        for b in range(P):
            bits_eq(o["out"][b], X.O.median(d[b], wnd), f"out[{b}]")
    return (lambda: X.lib.smt_median_filter_batch(A.ptr("in"), A.ptr("out"), P, sz(s), W, H, wnd, X.st()), verify)


def _median_inplace(kind):
    def make(A, X, H, W, wnd, impl=0, gap=0, P=1, band=0, reverse=0):
        d = np.stack([MC.rand_map(H, W, 220 + b) for b in range(P)])
        s = _strided(gap, H * W)
        A.inout("disp", d if kind != "single" else d[0], stride=s)

        def call():
            if kind == "host":
                return X.lib.smt_median_filter_inplace_host(A.ptr("disp"), P, sz(s), W, H, wnd)
            if kind == "host_ex":
                return X.lib.smt_median_filter_inplace_host_ex(A.ptr("disp"), P, sz(s), W, H, wnd, impl, band, reverse)
            X.lib.smt_median_inplace_set_impl(impl)
            try:
                if kind == "single":
                    rc = X.lib.smt_median_filter_inplace(A.ptr("disp"), W, H, wnd, X.st())
                else:
                    rc = X.lib.smt_median_filter_inplace_batch(A.ptr("disp"), P, sz(s), W, H, wnd, X.st())
                X.sync()
                return rc
            finally:
                X.lib.smt_median_inplace_set_impl(0)

        def verify(o):
            got = o["disp"].reshape(P, H, W)
            for b in range(P):
                assert MC.same_bits(got[b], MC.oracle_inplace(d[b], wnd)), ("disp", b)
        return call, verify
    return make


_MED = [(1, 63), (5, 65), (3, 4), (130, 9)]
entry("smt_median_filter_inplace", *[dict(H=h, W=w, wnd=k, impl=i) for h, w in _MED for k in (3, 7) for i in (0, 1)])(_median_inplace("single"))
entry("smt_median_filter_inplace_batch", *[dict(H=h, W=w, wnd=k, impl=i, gap=g, P=3) for h, w in _MED[:3] for k in (3, 5) for i in (0, 1)
                                           for g in (0, 1)])(_median_inplace("batch"))
entry("smt_median_filter_inplace_host", *[dict(H=h, W=w, wnd=k, gap=g, P=3) for h, w in _MED[:3] for k in (3, 7) for g in (0, 1)])(_median_inplace("host"))
entry("smt_median_filter_inplace_host_ex", *[dict(H=h, W=w, wnd=k, impl=i, gap=g, P=2, band=b, reverse=r) for h, w in _MED for k in (3, 5)
                                             for i, b, r in ((0, 0, 0), (0, 3, 1), (1, 2, 0)) for g in (0, 1)])(_median_inplace("host_ex"))


@entry("smt_remove_speckles", dict(H=1, W=63), dict(H=9, W=65), dict(H=33, W=34))
def _speckles(A, X, H, W):
    d = _disp_map(H, W, 230)
    A.inout("disp", d)
    return (lambda: X.lib.smt_remove_speckles(A.ptr("disp"), W, H, 1, u32(5), INT_MIN, X.st()),
            lambda o: bits_eq(o["disp"], X.O.remove_speckles(d, 1, 5, INT_MIN), "disp"))


@entry("smt_remove_speckles_batch", dict(H=9, W=65, gap=0), dict(H=9, W=65, gap=1), dict(H=1, W=63, gap=1, err=False), dict(H=33, W=34, gap=1))
def _speckles_batch(A, X, H, W, gap, err=True, P=3):
    d = np.stack([_disp_map(H, W, 240 + b) for b in range(P)])
    s = _strided(gap, H * W)
    A.inout("disp", d, stride=s)
    if err:
        A.inout("err", np.zeros(1, np.int32))

    def verify(o):
        for b in range(P):
            bits_eq(o["disp"][b], X.O.remove_speckles(d[b], 1, 5, INT_MIN), f"disp[{b}]")
        assert not err or int(o["err"][0]) == 0
    return (lambda: X.lib.smt_remove_speckles_batch(A.ptr("disp"), P, sz(s), W, H, 1, u32(5), INT_MIN, A.ptr("err" if err else None), X.st()),
            verify)


@entry("smt_cblsm_tail_batch", dict(H=9, W=65, gap=0), dict(H=9, W=65, gap=1, counts=False, err=False), dict(H=1, W=63, gap=1))
def _tail(A, X, H, W, gap, counts=True, err=True, P=3):
    from test_cblsm_post_gpu import _chain, _surface_pair
    pairs = [_surface_pair(H, W, 250 + b) for b in range(P)]
    dL, dR = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    s = _strided(gap, H * W)
    A.inout("dispL", dL, stride=s); A.inp("dispR", dR, stride=s); A.out("cls", (P, H, W), np.uint8)
    if counts:
        A.out("counts", (P, 2), np.int32)
    if err:
        A.inout("err", np.zeros(1, np.int32))

    def call():
        q = X.L.CBLSMPostParams()
        X.lib.smt_cblsm_post_default_params(C.byref(q))
        q.speckle_min_area = 5
        return X.lib.smt_cblsm_tail_batch(A.ptr("dispL"), A.ptr("dispR"), P, sz(s), H, W, C.byref(q), A.ptr("cls"),
                                          A.ptr("counts" if counts else None), A.ptr("err" if err else None), X.st())

    def verify(o):
        for b in range(P):
            _, _, fin, cls, cnt = _chain(X.O, dL[b], dR[b], area=5)
            assert MC.same_bits(o["dispL"][b], fin), ("dispL", b)
            bits_eq(o["cls"][b], cls, f"cls[{b}]")
            assert not counts or tuple(o["counts"][b]) == cnt
        assert not err or int(o["err"][0]) == 0
    return call, verify


# ================================================================================================ the runner
def run_once(X, name, params, seed):
    """one call in a fresh arena of `seed` -> (outputs after check(), verify)"""
    A = arena.Arena(seed, X.device)
    call, verify = ENTRIES[name](A, X, **params)
    A.build()
    rc = call()
    X.sync()
    assert rc == 0, f"{name}{params}: status {rc}"
    o = A.check()
    o.update(A.extra)
    return o, verify


def assert_same(a, b, what):
    for k in a:
        assert arena.same_bytes(a[k], b[k]), (
            f"{what}: {k}: {int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum())} bytes differ")


def run_case(X, name, params):
    """one case under both seeds -> the outputs (of the first seed), after every assertion of the suite"""
    outs = [run_once(X, name, params, seed) for seed in arena.SEEDS]
    assert_same(outs[0][0], outs[1][0], f"{name}{params} depends on the prefill or on what lies beside its tensors (two seeds)")
    outs[0][1](outs[0][0])
    return outs[0][0]


def case_id(p):
    return "-".join(f"{k}{'.'.join(v) if isinstance(v, tuple) else v}" for k, v in p.items()) or "default"


# ================================================================================================ everything else
NOT_CALLER_BUFFER = {
    "smt_strerror": "returns a string", "smt_version": "no buffers", "smt_last_hip_error": "no buffers",
    "smt_device_count": "host int out", "smt_set_device": "setter",
    "smt_malloc": "allocator plumbing", "smt_free": "allocator plumbing", "smt_memcpy_h2d": "hipMemcpy plumbing",
    "smt_memcpy_d2h": "hipMemcpy plumbing", "smt_memset": "hipMemset plumbing", "smt_stream_create": "stream plumbing",
    "smt_stream_destroy": "stream plumbing", "smt_stream_sync": "stream plumbing",
    "smt_host_malloc": "pinned host allocator", "smt_host_free": "pinned host allocator",
    "smt_adcensus_timing": "setter", "smt_adcensus_kernel_times": "host arrays out",
    "smt_adcensus_diag": "measurement hook on library-owned volumes",
    "smt_adcensus_create": "create", "smt_adcensus_create_on": "create", "smt_adcensus_create_ex": "create",
    "smt_adcensus_destroy": "destroy", "smt_adcensus_placement": "host accessor", "smt_adcensus_store_mode": "host accessor",
    "smt_adcensus_set_stream": "setter", "smt_adcensus_set_quirks": "setter",
    "smt_adcensus_host_create": "create", "smt_adcensus_host_run": "host memory in and out; device buffers are the handle's",
    "smt_adcensus_host_stats": "host struct out", "smt_adcensus_host_destroy": "destroy",
    "smt_adcensus_host_selftest_schedule": "host-only selftest",
    "smt_adcensus_volume": "accessor of a library-owned volume", "smt_adcensus_force_generic": "setter",
    "smt_adcensus_selftest_fused_grid": "host-only selftest", "smt_adcensus_selftest_maps_grid": "host-only selftest",
    "smt_adcensus_selftest_cost_rank": "host-only selftest", "smt_adcensus_status": "status",
    "smt_crossarm_default_params": "host struct out", "smt_crossarm_cblsm_params": "host struct out",
    "smt_crossarm_create": "create", "smt_crossarm_create_on": "create", "smt_crossarm_destroy": "destroy",
    "smt_crossarm_set_stream": "setter", "smt_crossarm_reset": "state of library-owned maps", "smt_crossarm_tau": "host int out",
    "smt_crossarm_set_arm_walk": "setter", "smt_crossarm_arm_maps": "accessor of library-owned maps",
    "smt_crossarm_status": "status", "smt_crossarm_set_variant": "setter", "smt_crossarm_set_strip_width": "setter",
    "smt_crossarm_set_occupancy": "setter", "smt_crossarm_set_sweep": "setter",
    "smt_crossarm_selftest_grid": "host-only selftest",
    "smt_scanline_create": "create", "smt_scanline_create_on": "create", "smt_scanline_destroy": "destroy",
    "smt_scanline_set_stream": "setter", "smt_scanline_set_quirks": "setter",
    "smt_pipeline_default_params": "host struct out", "smt_pipeline_create": "create", "smt_pipeline_create_on": "create",
    "smt_pipeline_destroy": "destroy", "smt_pipeline_set_stream": "setter", "smt_pipeline_set_quirks": "setter",
    "smt_pipeline_volumes": "accessor of library-owned volumes", "smt_pipeline_status": "status",
    "smt_post_default_params": "host struct out",
    "smt_cblsm_default_params": "host struct out", "smt_cblsm_flow_create_on": "create", "smt_cblsm_flow_destroy": "destroy",
    "smt_cblsm_flow_set_stream": "setter", "smt_cblsm_flow_volumes": "accessor of library-owned volumes",
    "smt_cblsm_flow_status": "status", "smt_cblsm_selftest_box": "host-only selftest", "smt_cblsm_selftest_v4": "host-only selftest",
    "smt_lrcheck_lists": "host memory in and out",
    "smt_crossagg_create": "create", "smt_crossagg_create_on": "create", "smt_crossagg_destroy": "destroy",
    "smt_crossagg_set_stream": "setter", "smt_crossagg_set_params": "setter", "smt_crossagg_set_impl": "setter",
    "smt_crossagg_cost": "accessor of a library-owned volume", "smt_crossagg_arms": "accessor of library-owned arms",
    "smt_adcensus_option_default": "host struct out",
    "smt_crossagg_flow_default_params": "host struct out", "smt_crossagg_flow_create_on": "create",
    "smt_crossagg_flow_destroy": "destroy", "smt_crossagg_flow_set_stream": "setter",
    "smt_crossagg_flow_volumes": "accessor of library-owned volumes", "smt_crossagg_flow_set_impl": "setter",
    "smt_crossagg_flow_status": "status", "smt_crossagg_selftest_first_pass": "host-only selftest",
    "smt_sad_set_impl": "setter", "smt_ncc_set_impl": "setter", "smt_asw_masks": "host arrays out",
    "smt_asw_both_set_impl": "setter", "smt_asw_selftest_right_keys": "host-only selftest",
    "smt_scratch_trim": "arena control", "smt_scratch_info": "host ints out", "smt_scratch_poison": "arena control (test hook)",
    "smt_asw_set_impl": "setter",
    "smt_asw_default_params": "host struct out", "smt_asw_flow_create_on": "create", "smt_asw_flow_destroy": "destroy",
    "smt_asw_flow_set_stream": "setter",
    "smt_sad_both_set_impl": "setter", "smt_sad_both_set_dispatch": "setter", "smt_sad_both_set_band": "setter",
    "smt_sad_both_last_form": "no buffers", "smt_sad_selftest_box": "host-only selftest",
    "smt_sad_selftest_right_keys": "host-only selftest",
    "smt_sad_default_params": "host struct out", "smt_sad_flow_create_on": "create", "smt_sad_flow_destroy": "destroy",
    "smt_sad_flow_set_stream": "setter",
    "smt_image_read": "image I/O on host memory", "smt_image_free": "image I/O on host memory",
    "smt_image_write": "image I/O on host memory",
    "smt_median_inplace_set_impl": "setter", "smt_cblsm_post_default_params": "host struct out",
    "smt_speckle_selftest_tiles": "host-only selftest",
}

# the entry points that take caller device buffers: none of these may move to NOT_CALLER_BUFFER
REQUIRED = """smt_bgr2gray smt_pad_replicate smt_u8_to_f32 smt_sum_f32 smt_wta smt_adcensus_compute smt_adcensus_compute_batch
smt_crossarm_arms smt_crossarm_arm_dir smt_crossarm_load_arm_maps smt_crossarm_aggregate smt_cblsm_ad
smt_cblsm_choose_arm_length smt_cblsm_cost_aggregation_new smt_cblsm_cost_aggregation_v4 smt_scanline_run smt_scanline_pass
smt_pipeline_run_batch smt_pipeline_run_batch_post smt_cblsm_flow_run_batch smt_cblsm_flow_run_batch_v4
smt_cblsm_flow_run_batch_post smt_crossagg_aggregate smt_adcensus_option_aggregate smt_crossagg_flow_run_batch
smt_crossagg_flow_run_batch_post smt_lrcheck smt_lrcheck_variant smt_fill_the_hole smt_fill_the_hole_batch smt_sad smt_sad_both
smt_sad_batch smt_sad_crosscheck smt_sad_flow_run_batch smt_ncc smt_ncc_batch smt_asw smt_asw_both smt_asw_batch
smt_asw_crosscheck smt_asw_flow_run_batch smt_median_filter smt_median_filter_batch smt_median_filter_inplace
smt_median_filter_inplace_batch smt_remove_speckles smt_remove_speckles_batch smt_cblsm_tail_batch""".split()

HOST_ENTRIES = ("smt_fill_the_hole_batch_host", "smt_median_filter_inplace_host", "smt_median_filter_inplace_host_ex")
