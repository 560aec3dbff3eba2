"""Region voting and outlier interpolation on the device (include/smt_refine.h), bit for bit against the NumPy
restatement of tests/refine_cases.py on maps, state and status: the direct form, the wave-per-outlier form and the default
dispatch on the whole case table and on the crafted cases; three maps in one call; strides, guards, both prefills and a
poisoned scratch arena (tests/arena.py); a busy side stream with late inputs.  Then the pipeline: run_refined against the
composition of the entry points it sequences, under every schedule, both scan_views, the fix bits and sub-pixel maps,
with the coverage condition -- voted, interpolated and left outliers in one call -- checked on its status; run_post
unchanged around it; the wrappers, shard.pipeline_refined_batch and adcensus_main --refine.  No tolerance anywhere."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import refine_cases as R  # noqa: E402
from prefill import first_diff, flows  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (R.DIRECT, R.WAVE)
INT_MIN = -2 ** 31


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the table's arrays are read-only


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (what, first_diff(got, ref))


def same3(got, want, what):
    for g, w, n in zip(got, want, ("map", "state", "status")):
        same(g, w, what + (n,))


@pytest.fixture
def hooks(flows):
    yield flows
    flows.refine_set_impl(0)


def cparams(smt, p):
    return smt.refine_params(**p)


def every_form(smt, which, M, arms, cls, gray, D, p, want, what):
    """the direct form, the wave form and the default dispatch"""
    for impl in FORMS + (0,):
        smt.refine_set_impl(impl)
        m = T(M)
        if which == "vote":
            got = smt.RegionVote(m, [T(a) for a in arms], D, cparams(smt, p), want_state=True)
        elif which == "interpolate":
            got = smt.InterpolateOutliers(m, T(cls), T(gray), D, cparams(smt, p), want_state=True)
        else:
            got = smt.Refine(m, [T(a) for a in arms], T(cls), T(gray), D, cparams(smt, p), want_state=True)
        if which != "interpolate" and p["irv_iters"] > 0:
            form = smt.refine_last_form()
            assert form == impl if impl else form in FORMS, (what, impl, form)
        same3(got, want, what + (which, impl))


@pytest.mark.parametrize("gid,H,W,D,seed", R.TABLE, ids=[t[0] for t in R.TABLE])
def test_every_form_equals_the_restatement(hooks, gid, H, W, D, seed):
    M, arms, cls, gray = R.case(H, W, D, seed)
    for which in ("vote", "interpolate", "refine"):
        every_form(hooks, which, M, arms, cls, gray, D, R.TABLE_PARAMS, R.table_expected(H, W, D, seed, which), (gid,))


VOTE = R.crafted_vote()
INTERP = R.crafted_interp()


@pytest.mark.parametrize("name", sorted(VOTE))
def test_voting_crafted(hooks, name):
    M, arms, D, p, chk = VOTE[name]
    want = R.vote(M, arms, D, p)
    assert chk is None or chk(*want), name
    every_form(hooks, "vote", M, arms, None, None, D, p, want, (name,))


@pytest.mark.parametrize("name", sorted(INTERP))
def test_interpolation_crafted(hooks, name):
    M, cls, gray, D, p, chk = INTERP[name]
    want = R.interpolate(M, cls, gray, D, p)
    assert chk is None or chk(*want), name
    every_form(hooks, "interpolate", M, None, cls, gray, D, p, want, (name,))


def test_three_maps_in_one_call_equal_three_calls(hooks):
    smt = hooks
    H, W, D = 17, 65, 200
    cases = [R.case(H, W, D, s) for s in (4, 21, 22)]
    p = R.TABLE_PARAMS
    arms = [T(np.stack([c[1][k] for c in cases])) for k in range(4)]
    cls, gray = T(np.stack([c[2] for c in cases])), T(np.stack([c[3] for c in cases]))
    for impl in FORMS:
        smt.refine_set_impl(impl)
        m, s, t = smt.Refine(T(np.stack([c[0] for c in cases])), arms, cls, gray, D, cparams(smt, p), want_state=True)
        for k, c in enumerate(cases):
            m1, s1, t1 = smt.Refine(T(c[0]), [T(a) for a in c[1]], T(c[2]), T(c[3]), D, cparams(smt, p), want_state=True)
            want = R.refine(*c, D, p)
            same(m[k], m1, (impl, k, "map")); same(s[k], s1, (impl, k, "state")); same(t[k], t1, (impl, k, "status"))
            same(m[k], want[0], (impl, k, "map, restatement")); same(s[k], want[1], (impl, k, "state, restatement"))
            same(t[k], want[2], (impl, k, "status, restatement"))


ARENA = [((9, 33), 192, R.WAVE, 3), ((17, 65), 16, R.WAVE, 7), ((17, 65), 16, R.DIRECT, 7), ((37, 130), 64, R.WAVE, 8),
         ((1, 70), 16, R.DIRECT, 1), ((7, 1), 64, R.WAVE, 2), ((1, 1), 1, R.DIRECT, 0), ((9, 33), 512, R.DIRECT, 9)]


@pytest.mark.parametrize("shape,D,impl,seed", ARENA, ids=[f"{s[0]}x{s[1]}-D{d}-{i}" for s, d, i, _ in ARENA])
def test_in_the_arena(hooks, shape, D, impl, seed):
    """guards on both sides of every tensor, both prefill seeds (one all-NaN), non-dense strides in elements, the scratch
    arena poisoned, the inputs untouched; two maps, the second one the first one's inputs turned round"""
    smt = hooks
    from stereo_match_traditional_amd import _lib
    lib = _lib.lib()
    H, W = shape
    N = H * W
    one = R.case(H, W, D, seed)
    two = (one[0][::-1, ::-1].copy(), tuple(a[::-1].copy() for a in one[1]), one[2][:, ::-1].copy(), one[3][::-1].copy())
    cases = (one, two)
    p = R.TABLE_PARAMS
    smt.refine_set_impl(impl)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = C.c_size_t
    q = cparams(smt, p)
    for byte in (0xFF, 0x00):
        smt.scratch_poison(byte)

        def make(A):
            A.inout("maps", np.stack([c[0] for c in cases]), stride=N + 5)
            for k, n in enumerate("LRTB"):
                A.inp("a" + n, np.stack([c[1][k] for c in cases]), stride=N + 3)
            A.inp("cls", np.stack([c[2] for c in cases]), stride=N + 7)
            A.inp("gray", np.stack([c[3] for c in cases]), stride=N + 1)
            A.out("state", (2, H, W), np.uint8, stride=N + 9)
            A.out("status", (2, 4), np.int32)
            return lambda A: lib.smt_refine_batch(A.ptr("maps"), 2, z(N + 5), A.ptr("aL"), A.ptr("aR"), A.ptr("aT"), A.ptr("aB"), z(N + 3),
                                                  A.ptr("cls"), z(N + 7), A.ptr("gray"), z(N + 1), H, W, D, C.byref(q), A.ptr("state"),
                                                  z(N + 9), A.ptr("status"), st())
        out, _ = arena.run_two_seeds(make, "cuda:0", torch.cuda.synchronize)
        assert smt.refine_last_form() == impl
        for k, c in enumerate(cases):
            want = R.refine(*c, D, p)
            same(out["maps"][k], want[0], (shape, D, impl, byte, k, "map")); same(out["state"][k], want[1], (shape, D, impl, byte, k, "state"))
            same(out["status"][k], want[2], (shape, D, impl, byte, k, "status"))

        def make_vote_only(A):                                     # no state, no status; an odd number of passes
            A.inout("maps", np.stack([c[0] for c in cases]), stride=N + 5)
            for k, n in enumerate("LRTB"):
                A.inp("a" + n, np.stack([c[1][k] for c in cases]))
            return lambda A: lib.smt_region_vote_batch(A.ptr("maps"), 2, z(N + 5), A.ptr("aL"), A.ptr("aR"), A.ptr("aT"), A.ptr("aB"), z(0),
                                                       H, W, D, C.byref(q), None, z(0), None, st())
        out, _ = arena.run_two_seeds(make_vote_only, "cuda:0", torch.cuda.synchronize)
        for k, c in enumerate(cases):
            same(out["maps"][k], R.vote(c[0], c[1], D, p)[0], (shape, D, impl, byte, k, "vote only"))


@pytest.mark.parametrize("impl", FORMS)
def test_asynchronous_on_a_busy_side_stream(hooks, impl):
    """enqueued behind a long sleep on a side stream, the call returns while the stream is still busy and reads the inputs
    that copies behind the sleep put there: every launch and the memset are ordered on that stream"""
    smt = hooks
    H, W, D, seed = 17, 65, 16, 7
    M, arms, cls, gray = R.case(H, W, D, seed)
    want = R.table_expected(H, W, D, seed, "refine")
    smt.refine_set_impl(impl)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        src = [T(M)] + [T(a) for a in arms] + [T(cls), T(gray)]
        late = [torch.zeros_like(t) for t in src]
        late[0].fill_(float("nan"))
        smt.Refine(late[0].clone(), late[1:5], late[5], late[6], D, cparams(smt, R.TABLE_PARAMS))   # the arena holds the scratch
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        for a, b in zip(late, src):
            a.copy_(b, non_blocking=True)
        got = smt.Refine(late[0], late[1:5], late[5], late[6], D, cparams(smt, R.TABLE_PARAMS), want_state=True)
        pending = not s.query()
    s.synchronize()
    assert pending, "the call waited for the stream"
    same3(got, want, (impl,))


# ---- the pipeline ------------------------------------------------------------------------------------------------------
PIPE_SHAPES = {"32x96": (32, 96, 64, 4), "40x130": (40, 130, 192, 1)}
SEARCH2 = R.params(search=2)            # with two probes per ray some outliers stay: the coverage condition's third part


def _pairs(O, H, W, D, seed, n=3):
    prs = [O.synth_pair(H, W, D, seed + k) for k in range(n)]
    return T(np.stack([p[0] for p in prs])), T(np.stack([p[1] for p in prs]))


def _composition(smt, pipe, L8, R8, D, quirks, p):
    """run -> RemoveSpecklesBatch -> smt_crossarm_arms(left) + Refine -> MedianFilterBatch, pair by pair"""
    P, H, W = L8.shape
    dl, dr, cls, counts = pipe.run(L8, R8)
    smt.RemoveSpecklesBatch(dl, 1, 30, INT_MIN)
    ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, quirks=quirks)
    states, stats = [], []
    for b in range(P):
        ca.ComputeArmLengths(L8[b])
        _, s, t = smt.Refine(dl[b], [a.clone() for a in ca.arm_maps()], cls[b], L8[b], D, cparams(smt, p), want_state=True)
        states.append(s); stats.append(t)
    ca.close()
    return dl, dr, cls, counts, smt.MedianFilterBatch(dl, 3), torch.stack(states), torch.stack(stats)


def _pipeline_case(smt, O, shape, quirks=0, subpixel=None, views=None, p=SEARCH2, coverage=False):
    H, W, D, seed = PIPE_SHAPES[shape]
    L8, R8 = _pairs(O, H, W, D, seed)
    pipe = smt.Pipeline(H, W, D, quirks=quirks, subpixel=subpixel, scan_views=views if views is not None else smt.VIEW_LEFT)
    try:
        before = pipe.run_post(L8, R8)
        names = ("dispL", "dispR", "cls", "counts", "lastDisp", "state", "status")
        for rep in range(2):                                       # a reused handle
            got = pipe.run_refined(L8, R8, refine=cparams(smt, p))
            want = _composition(smt, pipe, L8, R8, D, quirks, p)
            for g, w, n in zip(got, want, names):
                same(g, w, (shape, quirks, subpixel, views, rep, n))
        after = pipe.run_post(L8, R8)
        for a, b, n in zip(before, after, names):
            same(b, a, (shape, "run_post around a refined call", n))
        status = got[6].cpu().numpy()
        state = got[5].cpu().numpy()
        for b in range(L8.shape[0]):                               # status is what state shows
            assert status[b, 0] == int((state[b] != 0).sum()) and status[b, 1] == int(((state[b] >= 1) & (state[b] <= 16)).sum())
            assert status[b, 2] == int((state[b] == R.INTERPOLATED).sum()) and status[b, 3] == 0
        if coverage:
            left = (state == R.OUTLIER).reshape(len(state), -1).sum(1)
            print("status", status.tolist(), "left", left.tolist())
            assert ((status[:, 1] > 0) & (status[:, 2] > 0) & (left > 0)).any(), (status.tolist(), left.tolist())
    finally:
        pipe.close()


@pytest.mark.parametrize("views", (1, 3), ids=("left", "both"))
@pytest.mark.parametrize("sched", ("0", "1", "2"))
@pytest.mark.parametrize("shape", sorted(PIPE_SHAPES))
def test_run_refined_equals_the_composition(hooks, O, monkeypatch, shape, sched, views):
    """SMT_PIPE_SCHEDULE is read by smt_pipeline_create, so a handle created here takes it; the coverage condition holds in
    every one of these cases (checked on the CPU with the restatement on the oracle's pipeline: e.g. 32 x 96, the pair of
    seed 5, search 2: 761 voted, 200 interpolated, 278 left of 1 239)"""
    monkeypatch.setenv("SMT_PIPE_SCHEDULE", sched)
    _pipeline_case(hooks, O, shape, views=views, coverage=True)


@pytest.mark.parametrize("shape", sorted(PIPE_SHAPES))
def test_run_refined_with_the_fix_bits_subpixel_and_defaults(hooks, O, shape):
    smt = hooks
    _pipeline_case(smt, O, shape, quirks=smt.QUIRK_FIX_ALL, coverage=True)
    _pipeline_case(smt, O, shape, subpixel=1.0)
    _pipeline_case(smt, O, shape, quirks=smt.QUIRK_FIX_ALL, subpixel=1.0, views=smt.VIEW_BOTH, p=R.params())


def test_both_forms_inside_the_pipeline(hooks, O):
    smt = hooks
    for impl in FORMS:
        smt.refine_set_impl(impl)
        _pipeline_case(smt, O, "32x96")
        assert smt.refine_last_form() == impl


def test_wrappers_and_shard(hooks, O):
    smt = hooks
    from stereo_match_traditional_amd import shard
    H, W, D, seed = PIPE_SHAPES["32x96"]
    L8, R8 = _pairs(O, H, W, D, seed, n=2)
    pipe = smt.Pipeline(H, W, D)
    want = pipe.run_refined(L8, R8)                               # the defaults
    one = pipe.run_refined(L8[0], R8[0], refine=smt.refine_params(smt.ADCensusOption()), median_wnd=3)   # [row][col] in
    for g, w in zip(one, want):
        same(g[0], w[0], "a single pair")
    pipe.close()
    last, dl = shard.pipeline_refined_batch(L8, R8, D)
    same(last, want[4], "shard lastDisp"); same(dl, want[0], "shard dispL")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        def compute(a, b, d):
            x, y = shard.pipeline_refined_batch(a, b, d)
            return x.cpu(), y.cpu()
        gl, gd = shard.run_sharded(L8, R8, D, compute)
    finally:
        dist.destroy_process_group()
    same(gl, want[4], "run_sharded lastDisp"); same(gd, want[0], "run_sharded dispL")
    e1, e2 = shard.pipeline_refined_batch(L8[:0], R8[:0], D)
    assert e1.shape == (0, H, W) and e2.dtype == torch.float32
    # stateless wrappers: keywords instead of a struct, no state, empty batches
    M, arms, cls, gray = R.case(9, 33, 192, 3)
    m, s, t = smt.RegionVote(T(M), [T(a) for a in arms], 192, irv_ts=4, irv_th=0.3, irv_iters=3)
    assert s is None
    same(m, R.table_expected(9, 33, 192, 3, "vote")[0], "keywords")
    with pytest.raises(TypeError):
        smt.RegionVote(T(M), [T(a) for a in arms], 192, smt.refine_params(), irv_ts=4)
    with pytest.raises(ValueError):
        smt.RegionVote(T(M), [T(a) for a in arms[:3]], 192)
    with pytest.raises(smt.SmtError):
        smt.RegionVote(T(M), [T(a) for a in arms], 513)
    e = smt.InterpolateOutliers(T(M)[None][:0], T(cls)[None][:0], T(gray)[None][:0], 192)
    assert e[0].shape == (0, 9, 33) and e[2].shape == (0, 4)


def fnv(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_adcensus_main_refine(hooks, O):
    """host/adcensus_main.cpp --refine through the C++ mirror: FNV-1a of the maps as the program prints them, against the
    device entry points on the same synthetic pair"""
    smt = hooks
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "adcensus_main")
    H, W, D, seed = 32, 96, 64, 4
    r = subprocess.run([exe, "--refine", str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = dict(line.split(None, 1) for line in r.stdout.splitlines())
    L, Rr = O.synth_pair(H, W, D, seed)
    pipe = smt.Pipeline(H, W, D)
    dl, dr, cls, counts, last, state, status = pipe.run_refined(T(L), T(Rr))
    pipe.close()
    assert out["refined_left"] == fnv(dl.cpu().numpy()) and out["median_left"] == fnv(last.cpu().numpy())
    assert out["refine_status"].split() == [str(v) for v in status[0].cpu().tolist()]
