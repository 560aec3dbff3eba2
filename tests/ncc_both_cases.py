"""The rows of the bounds suite (tests/bounds_cases.py) and of the stream-order suite (tests/stream_order_cases.py) for the
both-view NCC exports, kept beside their tests and registered on import, as tests/ncc_box_cases.py does: a reason in
NOT_CALLER_BUFFER for the three hooks, real entries with cases for smt_lrncc and smt_lrncc_flow_run_batch, and their
decisions in SYNCHRONISING (asynchronous; the flow as smt_ncc_flow_run_batch: a warm call neither allocates nor
synchronises).  test_ncc_both_cpu.py and test_ncc_both_gpu.py import this module, so the completeness tests see the rows
whenever the suite is collected as a whole.

The right view is defined as the mirror of NCC_algorithem: right(L, R) = fliplr(view(fliplr(R), fliplr(L))).  mirror_*
below state that once, for the oracle's map and for the exact reference."""
import ctypes as C

import numpy as np

import bounds_cases as BC
import exact_matchers as XM
import ncc_box_cases as NC  # noqa: F401  (the rows of smt_ncc_flow_run_batch: SC.cases() imports it too)
import stream_order_cases as SC

LOOP, DOT4, BOX = 1, 2, 3
COMPOSED, KEYS = 1, 2
OUTS = ("dispL", "dispR", "lastdisp", "cls")

BC.NOT_CALLER_BUFFER.update({
    "smt_lrncc_set_impl": "setter", "smt_lrncc_last_form": "no buffers", "smt_lrncc_selftest_keys": "host-only selftest",
})


def flip(a):
    return np.ascontiguousarray(np.asarray(a)[:, ::-1])


def mirror_map(O, L, R, D, win):
    """the right map by the definition: fliplr(NCC_algorithem(fliplr(R), fliplr(L))), on the oracle"""
    return flip(O.ncc(flip(R), flip(L), D, win))


def mirror_exact(L, R, D, win):
    """(exact, flat, sentinel) of the right view's costs, [H][W][D]: exact_matchers.ncc_exact on the mirrored pair, flipped back"""
    return tuple(flip(a) for a in XM.ncc_exact(flip(R), flip(L), D, win))


def expected_form(H, W, win, left_form, lr):
    """SMT_LRNCC_FORM_* a call must report, None for an empty interior (nothing runs, the hook keeps its value)"""
    if H <= 2 * win or W <= 2 * win:
        return None
    return KEYS if left_form != LOOP and lr != COMPOSED else COMPOSED


# (H, W, D, win): interior widths 15, 17 and 148 (16-pixel dot4 groups, 64-column box strips, a right pixel fed from three
# strips), one interior row; D of 1, 64, 65, 70, 200, 300 (one, two, four and eight slots; W < D at 300); sides 1, 3, 5; an
# empty interior
SHAPES = [(3, 17, 1, 1), (5, 19, 64, 1), (7, 37, 65, 2), (3, 21, 300, 1), (5, 40, 20, 0), (4, 9, 5, 3), (6, 150, 70, 1),
          (3, 215, 200, 1)]
# (smt_ncc impl, smt_lrncc impl, costs): KEYS on both integer kernels, COMPOSED on one, and the loop nest (always COMPOSED)
LRNCC_CASES = [dict(H=h, W=w, D=d, win=k, impl=i, lr=m, cost=c) for h, w, d, k in SHAPES
               for i, m, c in ((2, 2, True), (3, 2, True), (2, 1, True), (1, 0, False))]


def pair(H, W, seed):
    return BC._padded(H, W, 0, seed)[:2]


def case_pairs(name, p):
    """the image pairs of one case (what the CPU test holds to the no-near-tie condition)"""
    if name == "smt_lrncc":
        return [pair(p["H"], p["W"], 240)]
    return [pair(p["H"], p["W"], 250 + 3 * b) for b in range(p.get("P", 3))]


def check_right(X, dispR, costR, L, R, D, win, form, what):
    H, W = L.shape
    if H <= 2 * win or W <= 2 * win:
        assert (dispR == 0).all() and (costR is None or (costR.view(np.uint64) == 0).all()), what
        return
    if costR is not None:
        exact, flat, sentinel = mirror_exact(L, R, D, win)
        XM.check_ncc(costR, exact, flat, sentinel, win, form)
        BC.val_eq(dispR, XM.ncc_wta(costR, win), f"{what}: the right map is WinTakeAll of the call's own right costs")
        border = np.ones((H, W), bool)
        border[win:H - win, win:W - win] = False
        assert (costR[border].view(np.uint64) == 0).all(), what
    BC.val_eq(dispR, mirror_map(X.O, L, R, D, win), what)


@BC.entry("smt_lrncc", *LRNCC_CASES)
def _lrncc(A, X, H, W, D, win, impl, lr, cost):
    L, R = pair(H, W, 240)
    A.inp("L", L); A.inp("R", R)
    A.out("dispL", (H, W), np.int32); A.out("dispR", (H, W), np.int32)
    if cost:
        A.out("costL", (H, W, D), np.float64); A.out("costR", (H, W, D), np.float64)

    def call():
        lib = X.lib
        lib.smt_ncc_set_impl(impl); lib.smt_lrncc_set_impl(lr)
        try:
            rc = lib.smt_lrncc(A.ptr("L"), A.ptr("R"), H, W, D, win, A.ptr("dispL"), A.ptr("dispR"),
                               A.ptr("costL" if cost else None), A.ptr("costR" if cost else None), X.st())
            X.sync()
            A.extra["form"] = np.array([lib.smt_lrncc_last_form()], np.int32)
            return rc
        finally:
            lib.smt_ncc_set_impl(2); lib.smt_lrncc_set_impl(0)

    def verify(o):
        want = expected_form(H, W, win, {1: LOOP, 2: DOT4, 3: BOX}[impl], lr)
        assert want is None or int(o["form"][0]) == want, "the hooks must select the form"
        BC._ncc_check(X, o, L, R, D, win, 2 if impl == 3 else impl, cost, "dispL", "costL")
        check_right(X, o["dispR"], o["costR"] if cost else None, L, R, D, win, "loop" if impl == 1 else "int", "dispR")
    return call, verify


# (H, W, D, win, form, lr, outs)
FLOW_CASES = [dict(H=h, W=w, D=d, win=k, form=f, lr=m, outs=o) for h, w, d, k, f, m, o in [
    (5, 19, 64, 1, BOX, 2, OUTS), (5, 19, 64, 1, DOT4, 2, OUTS), (5, 19, 64, 1, LOOP, 0, OUTS), (5, 19, 64, 1, 0, 0, OUTS),
    (7, 37, 65, 2, BOX, 2, ("dispR",)), (7, 37, 65, 2, DOT4, 1, ("lastdisp",)), (7, 37, 65, 2, DOT4, 2, ("cls",)),
    (3, 21, 300, 1, BOX, 2, ("dispL", "cls")), (3, 21, 300, 1, DOT4, 2, ("dispR", "lastdisp")),
    (6, 150, 70, 1, BOX, 2, OUTS), (6, 150, 70, 1, BOX, 1, OUTS), (4, 9, 5, 3, BOX, 2, OUTS), (5, 40, 20, 0, DOT4, 2, OUTS)]]


@BC.entry("smt_lrncc_flow_run_batch", *FLOW_CASES)
def _lrncc_flow(A, X, H, W, D, win, form, lr, outs, P=3):
    imgs = [pair(H, W, 250 + 3 * b) for b in range(P)]
    A.inp("L", np.stack([i[0] for i in imgs])); A.inp("R", np.stack([i[1] for i in imgs]))
    for nm in outs:
        A.out(nm, (P, H, W), np.uint8 if nm == "cls" else np.int32)

    def call():
        h = C.c_void_p()
        prm = X.L.NCCParams()
        prm.winSize = win
        rc = X.lib.smt_ncc_flow_create_on(X.dev_index, H, W, D, C.byref(prm), C.byref(h))
        if rc:
            return rc
        X.lib.smt_lrncc_set_impl(lr)
        try:
            rc = X.lib.smt_ncc_flow_set_form(h, form) or X.lib.smt_ncc_flow_set_stream(h, X.st())
            rc = rc or X.lib.smt_lrncc_flow_run_batch(h, A.ptr("L"), A.ptr("R"), P, *[A.ptr(nm if nm in outs else None) for nm in OUTS])
            X.sync()
            A.extra["form"] = np.array([X.lib.smt_lrncc_last_form()], np.int32)
            return rc
        finally:
            X.lib.smt_lrncc_set_impl(0)
            X.lib.smt_ncc_flow_destroy(h)

    def verify(o):
        if form:
            want = expected_form(H, W, win, form, lr)
            assert want is None or int(o["form"][0]) == want, "the hooks must select the form"
        for b, (L, R) in enumerate(imgs):
            dl, dr = X.O.ncc(L, R, D, win), mirror_map(X.O, L, R, D, win)
            ro, rc = X.O.sad_crosscheck(dl, dr)
            for nm, ref in (("dispL", dl), ("dispR", dr), ("lastdisp", ro), ("cls", rc)):
                if nm in outs:
                    BC.val_eq(o[nm][b], ref, f"{nm}[{b}]")
    return call, verify


SC.SYNCHRONISING.update({
    "smt_lrncc": SC.ASYNC,
    "smt_lrncc_flow_run_batch": SC.ASYNC_WARM,      # the tables of the handle grow as in smt_ncc_flow_run_batch
})
