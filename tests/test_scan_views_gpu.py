"""The scanline optimiser on both views on the device (include/smt_scan_views.h), against the
oracle per view: smt_scanline_run_pair and smt_scanline_run_map on the shapes of tests/scan_views_cases.py (stored and
maps-only per view, SMT_QUIRK_FIX_SCAN_VERTICAL, sub-pixel), non-finite costs, the pipeline under SMT_VIEW_BOTH under every
schedule on a reused handle, all three on a busy stream with late inputs, and the error paths.  Outputs live in arenas
(tests/arena.py): NaN-prefilled under the odd seed, with guards that are checked after every call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402
import scan_views_cases as SV  # noqa: E402
from subpixel_cases import restate  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMT_ERR_ARG, SMT_ERR_STATE, SMT_ERR_REF_UB = -1, -6, -5
VIEW_LEFT, VIEW_RIGHT, VIEW_BOTH = 1, 2, 3
ENV = "SMT_PIPE_SCHEDULE"


@pytest.fixture(scope="module")
def X(smt, O):
    return BC.Ctx(O, "cuda:0")


def _sub(X, min_den):
    return None if min_den is None else C.byref(X.L.SubpixelParams(min_den))


def _scan_handle(X, H, W, D, quirks=0, min_den=None):
    h = C.c_void_p()
    assert X.lib.smt_scanline_create_on(X.dev_index, H, W, D, SV.P1, SV.P2, C.byref(h)) == 0
    assert X.lib.smt_scanline_set_stream(h, X.st()) == 0
    assert X.lib.smt_scanline_set_quirks(h, C.c_uint(quirks)) == 0
    assert X.lib.smt_scanline_set_subpixel(h, _sub(X, min_den)) == 0
    return h


# ================================================================================================ run_pair / run_map
def _pair_make(X, H, W, D, quirks, min_den, stored, inputs=SV.inputs):
    """arena declaration + closure of one smt_scanline_run_pair call; stored = per view whether vout is given"""
    def make(A):
        for v, nm in enumerate("LR"):
            cost, gray = inputs(H, W, D, v)
            A.inp("vin" + nm, cost); A.inp("gray" + nm, gray)
            if stored[v]:
                A.out("vout" + nm, (H, W, D), np.float32)
            A.out("disp" + nm, (H, W), np.float32)

        def call(A):
            h = _scan_handle(X, H, W, D, quirks, min_den)
            try:
                return X.lib.smt_scanline_run_pair(h, A.ptr("vinL"), A.ptr("grayL"), A.ptr("voutL" if stored[0] else None), A.ptr("dispL"),
                                                   A.ptr("vinR"), A.ptr("grayR"), A.ptr("voutR" if stored[1] else None), A.ptr("dispR"))
            finally:
                X.sync()
                X.lib.smt_scanline_destroy(h)
        return call
    return make


def _map_make(X, H, W, D, quirks, min_den, view):
    def make(A):
        cost, gray = SV.inputs(H, W, D, view)
        A.inp("vin", cost); A.inp("gray", gray); A.out("disp", (H, W), np.float32)

        def call(A):
            h = _scan_handle(X, H, W, D, quirks, min_den)
            try:
                return X.lib.smt_scanline_run_map(h, A.ptr("vin"), A.ptr("gray"), A.ptr("disp"))
            finally:
                X.sync()
                X.lib.smt_scanline_destroy(h)
        return call
    return make


@pytest.mark.parametrize("fixed", [False, True], ids=["faithful", "fixv"])
@pytest.mark.parametrize("shape", SV.SHAPES, ids=["x".join(map(str, s)) for s in SV.SHAPES])
def test_run_pair_and_run_map_against_the_oracle_per_view(X, O, shape, fixed):
    """every combination of stored and maps-only per view, sub-pixel off and at min_den 1 and 2^-20"""
    H, W, D = shape
    quirks = SV.QUIRK_FIX_SCAN_VERTICAL if fixed else 0
    refs = [SV.reference(O, H, W, D, v, fixed) for v in (0, 1)]
    if not fixed:
        for v in (0, 1):                                     # the transpose identity agrees with the oracle's sum where both exist
            cost, gray = SV.inputs(H, W, D, v)
            p = [SV.scan_pass_ref(O, cost, gray, w, False) for w in ("left", "right", "up", "down")]
            BC.bits_eq(((p[0] + p[1]) + p[2]) + p[3], refs[v], "oracle passes against oracle sum")
    assert not arena.same_bytes(refs[0], refs[1])
    for min_den in SV.MIN_DENS:
        maps = [SV.disp_of(O, refs[v], min_den) for v in (0, 1)]
        for stored in SV.COMBOS:
            o, _ = arena.run_two_seeds(_pair_make(X, H, W, D, quirks, min_den, stored), "cuda:0", X.sync)
            what = f"{shape} fixed={fixed} min_den={min_den} stored={stored}"
            for v, nm in enumerate("LR"):
                if stored[v]:
                    BC.bits_eq(o["vout" + nm], refs[v], f"vout{nm} {what}")
                BC.bits_eq(o["disp" + nm], maps[v], f"disp{nm} {what}")
        for v in (0, 1):
            o, _ = arena.run_two_seeds(_map_make(X, H, W, D, quirks, min_den, v), "cuda:0", X.sync)
            BC.bits_eq(o["disp"], maps[v], f"run_map view {v} {shape} fixed={fixed} min_den={min_den}")


@pytest.mark.parametrize("shape", SV.TALL, ids=["x".join(map(str, s)) for s in SV.TALL])
def test_run_pair_on_both_sides_of_the_launch_rule(X, O, shape):
    """H = 512 runs the view axis, H = 513 the single-view launches: the same results, stored and maps-only, with FIXV and
    sub-pixel on in the mixed combinations"""
    H, W, D = shape
    for fixed, min_den, combos in ((False, None, SV.COMBOS), (True, 1.0, ((True, False), (False, True)))):
        refs = [SV.reference(O, H, W, D, v, fixed) for v in (0, 1)]
        maps = [SV.disp_of(O, refs[v], min_den) for v in (0, 1)]
        for stored in combos:
            o, _ = arena.run_two_seeds(_pair_make(X, H, W, D, SV.QUIRK_FIX_SCAN_VERTICAL if fixed else 0, min_den, stored), "cuda:0", X.sync)
            for v, nm in enumerate("LR"):
                if stored[v]:
                    BC.bits_eq(o["vout" + nm], refs[v], f"vout{nm} {shape} stored={stored}")
                BC.bits_eq(o["disp" + nm], maps[v], f"disp{nm} {shape} stored={stored} fixed={fixed}")


def _t(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")


@pytest.mark.parametrize("shape", SV.SHAPES, ids=["x".join(map(str, s)) for s in SV.SHAPES])
def test_pair_equals_two_runs_on_a_reused_handle_in_either_order(X, shape):
    """smt_scanline_run_pair against two smt_scanline_run calls bit for bit; one handle serves run, run_pair and run_map
    in both orders (its scratch volumes are shared between the entries)"""
    H, W, D = shape
    (cL, gL), (cR, gR) = (tuple(_t(a) for a in SV.inputs(H, W, D, v)) for v in (0, 1))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    nan = lambda *s: torch.full(s, float("nan"), device="cuda:0")

    def two_runs(h):
        o = [nan(H, W, D), nan(H, W), nan(H, W, D), nan(H, W)]
        assert X.lib.smt_scanline_run(h, p(cL), p(gL), p(o[0]), p(o[1])) == 0
        assert X.lib.smt_scanline_run(h, p(cR), p(gR), p(o[2]), p(o[3])) == 0
        return o

    def pair(h, stored):
        o = [nan(H, W, D) if stored[0] else None, nan(H, W), nan(H, W, D) if stored[1] else None, nan(H, W)]
        assert X.lib.smt_scanline_run_pair(h, p(cL), p(gL), p(o[0]), p(o[1]), p(cR), p(gR), p(o[2]), p(o[3])) == 0
        return o

    def maps(h):
        o = [nan(H, W), nan(H, W)]
        assert X.lib.smt_scanline_run_map(h, p(cL), p(gL), p(o[0])) == 0
        assert X.lib.smt_scanline_run_map(h, p(cR), p(gR), p(o[1])) == 0
        return o

    for quirks, min_den in ((0, None), (SV.QUIRK_FIX_SCAN_VERTICAL, 1.0)):
        h1, h2 = (_scan_handle(X, H, W, D, quirks, min_den) for _ in range(2))
        try:
            first = two_runs(h1) + pair(h1, (True, True)) + pair(h1, (False, True)) + maps(h1) + pair(h1, (True, False))
            second = pair(h2, (True, False)) + maps(h2) + pair(h2, (False, True)) + pair(h2, (True, True)) + two_runs(h2)
            X.sync()
        finally:
            X.lib.smt_scanline_destroy(h1); X.lib.smt_scanline_destroy(h2)
        ref = [t.cpu().numpy() for t in first[:4]]
        assert not np.isnan(ref[1]).any() and not np.isnan(ref[3]).any()

        def hold(o, what):
            for k, t in enumerate(o):
                if t is not None:
                    BC.bits_eq(t.cpu().numpy(), ref[k], f"{what} output {k} quirks={quirks} min_den={min_den}")
        hold(first[4:8], "pair after two runs"); hold(first[8:12], "pair (maps, stored)")
        hold([None, first[12], None, first[13]], "run_map"); hold(first[14:18], "pair (stored, maps)")
        hold(second[0:4], "fresh pair (stored, maps)"); hold([None, second[4], None, second[5]], "run_map after pair")
        hold(second[6:10], "pair (maps, stored) after run_map"); hold(second[10:14], "pair after maps-only pairs")
        hold(second[14:18], "two runs after pairs")


@pytest.mark.parametrize("shape", SV.NONFINITE, ids=["x".join(map(str, s)) for s in SV.NONFINITE])
def test_nonfinite_costs_follow_the_reference_in_the_new_modes(X, O, shape):
    """a NaN at the first pixel of a line in front of which the true minimum lies (the min-after-last-NaN rule of the
    prologue), NaN and +inf rows elsewhere, per view: stored and maps-only, integer and sub-pixel maps"""
    H, W, D = shape
    ins = {v: SV.nonfinite_inputs(H, W, D, v) for v in (0, 1)}
    refs = [SV.scan_sum(O, ins[v][0], ins[v][1], False) for v in (0, 1)]
    assert all(np.isnan(r).any() and np.isinf(r).any() for r in refs)
    for min_den in (None, 1.0):
        maps = [SV.disp_of(O, refs[v], min_den) for v in (0, 1)]
        for stored in SV.COMBOS:
            o, _ = arena.run_two_seeds(_pair_make(X, H, W, D, 0, min_den, stored, inputs=lambda h, w, d, v: ins[v]), "cuda:0", X.sync)
            for v, nm in enumerate("LR"):
                if stored[v]:
                    BC.nan_bits_eq(o["vout" + nm], refs[v], f"vout{nm} stored={stored}")
                BC.nan_bits_eq(o["disp" + nm], maps[v], f"disp{nm} stored={stored} min_den={min_den}")


# ================================================================================================ the pipeline under BOTH
class Pipe:
    """one smt_pipeline handle for arenas that come and go"""

    def __init__(self, X, case, views, min_den=None):
        self.X, self.case, self.h = X, case, C.c_void_p()
        p = X.L.PipelineParams()
        X.lib.smt_pipeline_default_params(C.byref(p))
        assert X.lib.smt_pipeline_create_on(X.dev_index, case["H"], case["W"], case["D"], C.byref(p), C.byref(self.h)) == 0
        if case["fix"]:
            assert X.lib.smt_pipeline_set_quirks(self.h, C.c_uint(SV.QUIRK_FIX_RIGHT_ARM_STRIDE)) == 0
        assert X.lib.smt_pipeline_set_subpixel(self.h, _sub(X, min_den)) == 0
        assert X.lib.smt_pipeline_set_scan_views(self.h, views) == 0

    def views(self, v):
        assert self.X.lib.smt_pipeline_set_scan_views(self.h, v) == 0

    def run(self, pairs, post=False, seed=arena.SEEDS[1]):
        """-> the arena's outputs after a checked run of the pairs [(L, R)]"""
        X, c, P = self.X, self.case, len(pairs)
        A = arena.Arena(seed, "cuda:0")
        A.inp("L", np.stack([p[0] for p in pairs])); A.inp("R", np.stack([p[1] for p in pairs]))
        for nm in ("dispL", "dispR") + (("last",) if post else ()):
            A.out(nm, (P, c["H"], c["W"]), np.float32)
        A.out("cls", (P, c["H"], c["W"]), np.uint8); A.out("counts", (P, 2), np.int32)
        A.build()
        assert X.lib.smt_pipeline_set_stream(self.h, X.st()) == 0
        args = (self.h, A.ptr("L"), A.ptr("R"), P, A.ptr("dispL"), A.ptr("dispR"), A.ptr("cls"), A.ptr("counts"))
        if post:
            q = X.L.PostParams()
            X.lib.smt_post_default_params(C.byref(q))
            rc = X.lib.smt_pipeline_run_batch_post(*args, C.byref(q), A.ptr("last"))
        else:
            rc = X.lib.smt_pipeline_run_batch(*args)
        assert rc == 0, rc
        st = X.lib.smt_pipeline_status(self.h)
        assert st in (0, SMT_ERR_REF_UB), st                 # as tests/test_post_batch_gpu.py
        return A.check()

    def right_volume(self):
        c, p = self.case, C.c_void_p()
        rc = self.X.lib.smt_pipeline_scan_right_volume(self.h, C.byref(p))
        return rc, (self.X.d2h(p, (c["H"], c["W"], c["D"]), np.float32) if rc == 0 else None)

    def volumes(self):
        c, ps = self.case, [C.c_void_p() for _ in range(5)]
        assert self.X.lib.smt_pipeline_volumes(self.h, *[C.byref(p) for p in ps]) == 0
        return [self.X.d2h(p, (c["H"], c["W"], c["D"]), np.float32) for p in ps]

    def close(self):
        self.X.sync()
        self.X.lib.smt_pipeline_destroy(self.h)


def _hold_pairs(o, refs, side, post, what):
    for b, r in enumerate(refs):
        r = r[side]
        BC.bits_eq(o["dispR"][b], r["dr"], f"{what} dispR[{b}]")
        BC.bits_eq(o["cls"][b], r["cls"], f"{what} cls[{b}]")
        assert tuple(o["counts"][b]) == tuple(r["counts"]), (what, "counts", b)
        BC.bits_eq(o["dispL"][b], r["sp"] if post else r["lr"], f"{what} dispL[{b}]")
        if post:
            BC.bits_eq(o["last"][b], r["med"], f"{what} lastDisp[{b}]")


@pytest.mark.parametrize("sched", SV.SCHEDULES, ids=["unset", "s0", "s1", "s2"])
@pytest.mark.parametrize("case", SV.PIPE_CASES, ids=[c["name"] for c in SV.PIPE_CASES])
def test_pipeline_both_views_against_the_oracle_composition(X, O, monkeypatch, case, sched):
    """batches of 1, 2, 3 and 5 pairs on one handle (five pairs reuse both double-buffer sets), the odd batches through
    _post; scan_right_volume() is the last pair's sum after every batch"""
    SV.check_pipe_conditions(O, case)
    monkeypatch.delenv(ENV, raising=False)
    if sched is not None:
        monkeypatch.setenv(ENV, sched)
    pairs = SV.pipe_pairs(O, case)
    pipe = Pipe(X, case, VIEW_BOTH)
    try:
        assert pipe.right_volume()[0] == SMT_ERR_STATE
        for i, ks in enumerate(SV.batch_slices()):
            post = bool(i % 2)
            o = pipe.run([pairs[k] for k in ks], post=post)
            refs = [SV.pipe_pair_oracle(O, case, k) for k in ks]
            _hold_pairs(o, refs, "both", post, f"{case['name']} schedule {sched} batch {i}")
            rc, vol = pipe.right_volume()
            assert rc == 0
            BC.bits_eq(vol, refs[-1]["sumR"], f"scan_right_volume after batch {i}")
            vols = pipe.volumes()
            BC.bits_eq(vols[4], refs[-1]["vols"]["scanline_sum"], "the left view's sum is still lent")
            BC.bits_eq(vols[3], refs[-1]["vols"]["agg_right"], "agg_right")
    finally:
        pipe.close()


@pytest.mark.parametrize("sched", SV.SCHEDULES, ids=["unset", "s0", "s1", "s2"])
def test_pipeline_both_views_subpixel(X, O, monkeypatch, sched):
    case, min_den = SV.PIPE_CASES[0], 1.0
    monkeypatch.delenv(ENV, raising=False)
    if sched is not None:
        monkeypatch.setenv(ENV, sched)
    pairs = SV.pipe_pairs(O, case)
    pipe = Pipe(X, case, VIEW_BOTH, min_den)
    try:
        for ks, post in ((range(0, 3), False), (range(3, 5), True)):
            o = pipe.run([pairs[k] for k in ks], post=post)
            refs = [SV.pipe_pair_oracle(O, case, k, min_den) for k in ks]
            assert any((r["both"]["dr"] != np.round(r["both"]["dr"])).any() for r in refs), "no fraction in any right map"
            _hold_pairs(o, refs, "both", post, f"sub-pixel schedule {sched}")
    finally:
        pipe.close()


@pytest.mark.parametrize("sched", SV.SCHEDULES, ids=["unset", "s0", "s1", "s2"])
def test_left_after_both_equals_a_fresh_left_handle(X, O, monkeypatch, sched):
    case = SV.PIPE_CASES[1]
    monkeypatch.delenv(ENV, raising=False)
    if sched is not None:
        monkeypatch.setenv(ENV, sched)
    pairs = SV.pipe_pairs(O, case)
    a, b = pairs[0:3], pairs[3:6]
    used, fresh = Pipe(X, case, VIEW_BOTH), Pipe(X, case, VIEW_LEFT)
    try:
        used.run(a)
        used.views(VIEW_LEFT)
        got, want = used.run(b, post=True), fresh.run(b, post=True)
        BC.assert_same(got, want, "LEFT after BOTH against a fresh LEFT handle")
        _hold_pairs(got, [SV.pipe_pair_oracle(O, case, k) for k in range(3, 6)], "left", True, "LEFT after BOTH")
        for k, (u, f) in enumerate(zip(used.volumes(), fresh.volumes())):
            assert arena.same_bytes(u, f), f"smt_pipeline_volumes[{k}] differs after a BOTH run"
        rc, vol = used.right_volume()                        # still the last BOTH call's
        assert rc == 0
        BC.bits_eq(vol, SV.pipe_pair_oracle(O, case, 2)["sumR"], "scan_right_volume after a LEFT run")
        used.views(VIEW_BOTH)
        _hold_pairs(used.run(b), [SV.pipe_pair_oracle(O, case, k) for k in range(3, 6)], "both", False, "BOTH again")
    finally:
        used.close(); fresh.close()


# ================================================================================================ stream order
def _busy_entries(X, O):
    H, W, D = 6, 10, 70
    refs = [SV.reference(O, H, W, D, v, False) for v in (0, 1)]

    def pair(A, Xp):
        call = _pair_make(Xp, H, W, D, 0, None, (True, False))(A)

        def verify(o):
            BC.bits_eq(o["voutL"], refs[0], "voutL")
            for v, nm in enumerate("LR"):
                BC.bits_eq(o["disp" + nm], O.wta(refs[v]), "disp" + nm)
        return (lambda: call(A)), verify

    def one(A, Xp):
        call = _map_make(Xp, H, W, D, 0, None, 1)(A)
        return (lambda: call(A)), (lambda o: BC.bits_eq(o["disp"], O.wta(refs[1]), "disp"))

    def both(A, Xp):
        case = SV.PIPE_CASES[0]
        pairs = SV.pipe_pairs(O, case)[0:3]
        A.inp("L", np.stack([p[0] for p in pairs])); A.inp("R", np.stack([p[1] for p in pairs]))
        for nm in ("dispL", "dispR"):
            A.out(nm, (3, case["H"], case["W"]), np.float32)
        A.out("cls", (3, case["H"], case["W"]), np.uint8); A.out("counts", (3, 2), np.int32)

        def call():
            p, h = Xp.L.PipelineParams(), C.c_void_p()
            Xp.lib.smt_pipeline_default_params(C.byref(p))
            rc = Xp.lib.smt_pipeline_create_on(Xp.dev_index, case["H"], case["W"], case["D"], C.byref(p), C.byref(h))
            try:
                rc = rc or Xp.lib.smt_pipeline_set_stream(h, Xp.st()) or Xp.lib.smt_pipeline_set_scan_views(h, VIEW_BOTH)
                rc = rc or Xp.lib.smt_pipeline_run_batch(h, A.ptr("L"), A.ptr("R"), 3, A.ptr("dispL"), A.ptr("dispR"), A.ptr("cls"), A.ptr("counts"))
                A.extra["snap"] = A.buf.clone()               # a consumer on the caller's stream, before anything waits
                st = Xp.lib.smt_pipeline_status(h)
                return rc or (0 if st == SMT_ERR_REF_UB else st)
            finally:
                Xp.lib.smt_pipeline_destroy(h)

        def verify(o):
            _hold_pairs(A.check(o.pop("snap")), [SV.pipe_pair_oracle(O, case, k) for k in range(3)], "both", False, f"busy stream schedule {os.environ[ENV]}")
        return call, verify
    return pair, one, both


@pytest.mark.parametrize("which", ["run_pair", "run_map", "both_s0", "both_s1", "both_s2"])
def test_on_a_busy_stream_with_late_inputs(X, O, monkeypatch, which):
    """stream_order_cases' method (tests/test_stream_order_gpu.py's run_deferred): the stream sleeps, the inputs arrive
    behind the sleep, a consumer follows on the same stream; the entry must return while the sleep still runs"""
    from test_stream_order_gpu import run_deferred
    monkeypatch.setenv(ENV, which[-1] if which.startswith("both") else "1")       # read when the handle is created
    pair, one, both = _busy_entries(X, O)
    if which == "run_pair":
        name, make = "smt_scanline_run_pair", lambda A, Xp: pair(A, Xp)
    elif which == "run_map":
        name, make = "smt_scanline_run_map", lambda A, Xp: one(A, Xp)
    else:
        name, make = "smt_pipeline_run_batch", lambda A, Xp: both(A, Xp)
    probe = run_deferred(X, name, make, {})
    assert probe.returns, f"the closure never called {name}"
    # the first BOTH run allocates the handle's extra volumes, which may wait (as a first _post call may): the
    # scanline entries allocate too, on their first call -- hipMalloc does not wait for the stream
    assert all(p for p, _ in probe.returns), f"{name} waited: {probe.returns}"


# ================================================================================================ error paths, upper layers
def test_error_paths(X):
    H, W, D = 3, 5, 16
    t = lambda *s: torch.zeros(s, device="cuda:0")
    p = lambda x: C.c_void_p(x.data_ptr())
    a, b, g, o1, o2, d1, d2 = t(H, W, D), t(H, W, D), t(H, W), t(H, W, D), t(H, W, D), t(H, W), t(H, W)
    h = _scan_handle(X, H, W, D)
    run = X.lib.smt_scanline_run_pair
    try:
        assert run(None, p(a), p(g), p(o1), p(d1), p(b), p(g), p(o2), p(d2)) == SMT_ERR_ARG
        for k in (1, 2, 5, 6):                               # a NULL input volume or guide
            args = [h, p(a), p(g), p(o1), p(d1), p(b), p(g), p(o2), p(d2)]
            args[k] = None
            assert run(*args) == SMT_ERR_ARG, k
        assert run(h, p(a), p(g), None, None, p(b), p(g), p(o2), p(d2)) == SMT_ERR_ARG      # a view with neither output
        assert run(h, p(a), p(g), p(o1), p(d1), p(b), p(g), None, None) == SMT_ERR_ARG
        assert run(h, p(a), p(g), p(a), p(d1), p(b), p(g), p(o2), p(d2)) == SMT_ERR_ARG      # vout aliases its input
        assert run(h, p(a), p(g), p(b), p(d1), p(b), p(g), p(o2), p(d2)) == SMT_ERR_ARG      # ... the other view's input
        assert run(h, p(a), p(g), p(o1), p(d1), p(b), p(g), p(a), p(d2)) == SMT_ERR_ARG
        assert run(h, p(a), p(g), p(o1), p(d1), p(b), p(g), p(o1), p(d2)) == SMT_ERR_ARG     # one volume for both sums
        assert run(h, p(a), p(g), p(o1), p(d1), p(b), p(g), p(o2), p(d1)) == SMT_ERR_ARG     # one map for both views
        assert run(h, p(a), p(g), p(o1), None, p(b), p(g), None, p(d2)) == 0                 # no map for one view: allowed
        assert run(h, p(a), p(g), p(o1), p(d1), p(a), p(g), p(o2), p(d2)) == 0               # the same input twice: allowed
        m = X.lib.smt_scanline_run_map
        assert m(None, p(a), p(g), p(d1)) == m(h, None, p(g), p(d1)) == m(h, p(a), None, p(d1)) == m(h, p(a), p(g), None) == SMT_ERR_ARG
        X.sync()
    finally:
        X.lib.smt_scanline_destroy(h)
    pipe = Pipe(X, dict(H=4, W=12, D=8, fix=False), VIEW_LEFT)
    try:
        sv = X.lib.smt_pipeline_set_scan_views
        assert sv(None, VIEW_BOTH) == SMT_ERR_ARG
        for bad in (VIEW_RIGHT, 0, 4, -1):
            assert sv(pipe.h, bad) == SMT_ERR_ARG, bad
        q = C.c_void_p()
        assert X.lib.smt_pipeline_scan_right_volume(pipe.h, None) == SMT_ERR_ARG
        assert X.lib.smt_pipeline_scan_right_volume(None, C.byref(q)) == SMT_ERR_ARG
        assert X.lib.smt_pipeline_scan_right_volume(pipe.h, C.byref(q)) == SMT_ERR_STATE
        rng = np.random.default_rng(5)
        pipe.run([tuple(rng.integers(0, 256, (4, 12)).astype(np.uint8) for _ in range(2))])
        assert X.lib.smt_pipeline_scan_right_volume(pipe.h, C.byref(q)) == SMT_ERR_STATE      # a LEFT run lends nothing
    finally:
        pipe.close()


def test_api_shard_and_host_program(X, O, smt):
    """the upper layers: api.ScanlineOptimizer.ScanLinePair / ScanLineMap, api.Pipeline(scan_views=), shard.pipeline_batch
    and adcensus_main --scan-both, each against the oracle"""
    from stereo_match_traditional_amd import api, shard
    H, W, D = 6, 10, 70
    ins = [tuple(_t(a) for a in SV.inputs(H, W, D, v)) for v in (0, 1)]
    refs = [SV.reference(O, H, W, D, v, False) for v in (0, 1)]
    so = api.ScanlineOptimizer().Initialize(H, W, D, SV.P1, SV.P2)
    oL, oR, dL, dR = so.ScanLinePair(ins[0][0], ins[0][1], ins[1][0], ins[1][1], maps_only=(False, True))
    assert oR is None
    BC.bits_eq(oL.cpu().numpy(), refs[0], "ScanLinePair outL")
    BC.bits_eq(dR.cpu().numpy(), O.wta(refs[1]), "ScanLinePair dispR")
    assert dL is None
    BC.bits_eq(so.ScanLineMap(ins[0][0], ins[0][1]).cpu().numpy(), O.wta(refs[0]), "ScanLineMap")
    with pytest.raises(ValueError):
        so.ScanLinePair(ins[0][0], ins[0][1], ins[1][0], ins[1][1], out=(oL, oL), maps_only=True)
    so.close()

    case = SV.PIPE_CASES[0]
    pairs = SV.pipe_pairs(O, case)[0:2]
    L8, R8 = (_t(np.stack([p[i] for p in pairs])) for i in (0, 1))
    pipe = api.Pipeline(case["H"], case["W"], case["D"], scan_views=api.VIEW_BOTH)
    dl, dr, cls, counts = pipe.run(L8, R8)
    try:
        pipe.status()
    except api._lib.SmtError as e:                           # as tests/test_post_batch_gpu.py
        assert e.status == SMT_ERR_REF_UB
    ref = [SV.pipe_pair_oracle(O, case, k) for k in range(2)]
    for b in range(2):
        BC.bits_eq(dr[b].cpu().numpy(), ref[b]["both"]["dr"], f"api dispR[{b}]")
        BC.bits_eq(dl[b].cpu().numpy(), ref[b]["both"]["lr"], f"api dispL[{b}]")
    BC.bits_eq(pipe.scan_right_volume().cpu().numpy(), ref[1]["sumR"], "api scan_right_volume")
    pipe.set_scan_views(api.VIEW_LEFT)
    BC.bits_eq(pipe.run(L8, R8)[1][0].cpu().numpy(), ref[0]["left"]["dr"], "api LEFT dispR")
    with pytest.raises(api._lib.SmtError):
        pipe.set_scan_views(api.VIEW_RIGHT)
    pipe.close()
    case = SV.PIPE_CASES[2]                                  # with its arm fix no rectangle leaves the plane: a clean status
    pairs = SV.pipe_pairs(O, case)[0:2]
    L8, R8 = (_t(np.stack([p[i] for p in pairs])) for i in (0, 1))
    sl, sr = shard.pipeline_batch(L8, R8, case["D"], quirks=SV.QUIRK_FIX_RIGHT_ARM_STRIDE, scan_views=api.VIEW_BOTH)
    for b in range(2):
        r = SV.pipe_pair_oracle(O, case, b)["both"]
        BC.bits_eq(sr[b].cpu().numpy(), r["dr"], f"shard dispR[{b}]")
        BC.bits_eq(sl[b].cpu().numpy(), r["lr"], f"shard dispL[{b}]")

    # host/adcensus_main.cpp --scan-both through the C++ mirror: FNV-1a of the maps as the program prints them
    def fnv(a):
        h = 1469598103934665603
        for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return f"{h:016x}"
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "adcensus_main")
    Hh, Wh, Dh, seed = 16, 48, 16, 3
    r = subprocess.run([exe, "--scan-both", str(Hh), str(Wh), str(Dh), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = dict(line.split() for line in r.stdout.splitlines())
    L, R = O.synth_pair(Hh, Wh, Dh, seed)
    _, vols = SV.FC.pipeline_pair(O, L, R, Dh, False)
    wl = O.wta(vols["scanline_sum"])
    wr = O.wta(O.scanline(vols["agg_right"], R.astype(np.float32), SV.P1, SV.P2))
    assert out["so_wta_left"] == fnv(wl) and out["so_wta_right"] == fnv(wr)
    assert out["lr_left"] == fnv(O.lrcheck(wl, wr, SV.GATE)[0])
