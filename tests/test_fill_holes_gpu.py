"""Sad.h's FillHolesInDispMap on the device (include/smt_fill_holes.h), bit for bit against the NumPy restatement of
tests/fill_holes_cases.py on maps and status: the case table (1 x 1 to 1030 x 9, more rows than a workgroup has threads),
the crafted cases of the rule's sentences, the three invalid values, a NaN map beside a clean one; three maps in one call
against three calls; strides, guards, both prefills of status and a poisoned scratch arena with the class maps untouched
(tests/arena.py); a busy side stream with late inputs.  Then the pipeline: run_filled against LR check + restatement +
the oracle's median under every schedule, run_post unchanged around it, shard.pipeline_filled_batch.  No tolerance
anywhere.  adcensus_main --fill-holes through the C++ mirror against the same entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import fill_holes_cases as FH  # noqa: E402
from prefill import first_diff, flows  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the table's arrays are read-only


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (what, first_diff(got, ref))


def device(smt, M, cls, invalid=FH.INF):
    m, c = T(M), T(cls)
    status = smt.FillHolesInDispMap(m, c, invalid)
    same(c, cls, "cls is only read")
    return m, status


@pytest.mark.parametrize("gid", [t[0] for t in FH.TABLE])
def test_the_device_equals_the_restatement(flows, gid):
    M, cls = FH.table_case(gid)
    after, st = FH.table_expected(gid)
    m, status = device(flows, M, cls)
    same(m, after[2], (gid, "map")); same(status, st, (gid, "status"))


CRAFTED = FH.crafted()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted(flows, name):
    M, cls, invalid, chk = CRAFTED[name]
    after, st = FH.expected(("crafted", name), M, cls, invalid)
    assert chk is None or chk(after, st), name
    m, status = device(flows, M, cls, invalid)
    same(m, after[2], (name, "map")); same(status, st, (name, "status"))


def test_the_run_of_holes_is_filled_in_place(flows):
    """the device gives the raster-order recurrence, which on this input is not what a collect-then-write pass gives"""
    M, cls, invalid, _ = CRAFTED["run_1x9"]
    occ, mis = FH.lists_of(cls)
    jacobi, _ = FH.fill_holes_lists(M, occ, mis, invalid, collect_then_write=True)
    m, _ = device(flows, M, cls, invalid)
    got = m.cpu().numpy()
    assert (got[0, :8] == 3).all() and not np.array_equal(got, jacobi[2])


def test_a_nan_map_beside_a_clean_one(flows):
    smt = flows
    maps, cls = FH.nan_pair()
    m = T(maps)
    status = smt.FillHolesInDispMap(m, T(cls))
    same(m[0], maps[0], "the NaN map is not modified")
    after, st = FH.fill_holes(maps[1], cls[1])
    same(m[1], after[2], "the clean map"); same(status[1], st, "the clean map's status")
    same(status[0], FH.fill_holes(maps[0], cls[0])[1], "the NaN map's status")
    assert int(status[0, 3]) == smt.FILLHOLES_UB_NAN
    with pytest.raises(smt.SmtError):
        smt.FillHolesInDispMap(T(maps), T(cls), check=True)
    smt.FillHolesInDispMap(T(maps[1]), T(cls[1]), check=True)


def test_three_maps_in_one_call_equal_three_calls(flows):
    smt = flows
    H, W = 17, 65
    cases = [FH.case(H, W, s) for s in (4, 21, 22)]
    m = T(np.stack([c[0] for c in cases]))
    status = smt.FillHolesInDispMap(m, T(np.stack([c[1] for c in cases])))
    assert status.shape == (3, 4)
    for k, c in enumerate(cases):
        m1, s1 = device(smt, *c)
        assert s1.shape == (4,)
        after, st = FH.fill_holes(*c)
        same(m[k], m1, (k, "map")); same(status[k], s1, (k, "status"))
        same(m[k], after[2], (k, "map, restatement")); same(status[k], st, (k, "status, restatement"))
    e = smt.FillHolesInDispMap(m[:0], T(np.stack([c[1] for c in cases]))[:0])
    assert e.shape == (0, 4)


ARENA = [((9, 33), 3), ((17, 65), 7), ((37, 130), 8), ((1, 70), 1), ((7, 1), 2), ((1, 1), 0), ((1030, 9), 9)]


@pytest.mark.parametrize("shape,seed", ARENA, ids=[f"{s[0]}x{s[1]}" for s, _ in ARENA])
def test_in_the_arena(flows, shape, seed):
    """guards on both sides of every tensor and in the batch gaps, both prefill seeds of status (one all negative),
    non-dense strides in elements, the scratch arena poisoned, the class maps untouched; two maps, the second one the
    first one turned round; then without status"""
    smt = flows
    from stereo_match_traditional_amd import _lib
    lib = _lib.lib()
    H, W = shape
    N = H * W
    one = FH.case(H, W, seed)
    two = (one[0][::-1, ::-1].copy(), one[1][::-1, ::-1].copy())
    cases = (one, two)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = C.c_size_t
    for byte in (0xFF, 0x00):
        smt.scratch_poison(byte)
        for with_status in (True, False):
            def make(A):
                A.inout("maps", np.stack([c[0] for c in cases]), stride=N + 5)
                A.inp("cls", np.stack([c[1] for c in cases]), stride=N + 7)
                if with_status:
                    A.out("status", (2, 4), np.int32)
                return lambda A: lib.smt_fill_holes_batch(A.ptr("maps"), A.ptr("cls"), 2, z(N + 5), z(N + 7), H, W,
                                                          C.c_float(FH.INF), A.ptr("status" if with_status else None), st())
            out, _ = arena.run_two_seeds(make, "cuda:0", torch.cuda.synchronize)
            for k, c in enumerate(cases):
                after, want = FH.fill_holes(*c)
                same(out["maps"][k], after[2], (shape, byte, k, "map"))
                if with_status:
                    same(out["status"][k], want, (shape, byte, k, "status"))


def test_asynchronous_on_a_busy_side_stream(flows):
    """enqueued behind a long sleep on a side stream, the call returns while the stream is still busy and reads the inputs
    that copies behind the sleep put there: the launch is ordered on that stream"""
    smt = flows
    M, cls = FH.table_case("17x65")
    after, want = FH.table_expected("17x65")
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        src = [T(M), T(cls)]
        late = [torch.full_like(src[0], float("nan")), torch.zeros_like(src[1])]
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        for a, b in zip(late, src):
            a.copy_(b, non_blocking=True)
        status = smt.FillHolesInDispMap(late[0], late[1])
        pending = not s.query()
    s.synchronize()
    assert pending, "the call waited for the stream"
    same(late[0], after[2], "map"); same(status, want, "status")


# ---- the pipeline ------------------------------------------------------------------------------------------------------
PIPE_SHAPES = {"32x96": (32, 96, 64, 4), "40x130": (40, 130, 192, 1)}
NAMES = ("dispL", "dispR", "cls", "counts", "lastDisp", "status")


def _pairs(O, H, W, D, seed, n=2):
    prs = [O.synth_pair(H, W, D, seed + k) for k in range(n)]
    return T(np.stack([p[0] for p in prs])), T(np.stack([p[1] for p in prs]))


def _composition(O, pipe, L8, R8, wnd):
    """run (LR check included) -> the restatement on every left map with its class map -> the oracle's median"""
    dl, dr, cls, counts = pipe.run(L8, R8)
    maps, c = dl.cpu().numpy(), cls.cpu().numpy()
    filled, last, status = [], [], []
    for b in range(maps.shape[0]):
        after, st = FH.fill_holes(maps[b], c[b])
        filled.append(after[2]); status.append(st)
        last.append(np.asarray(O.median(after[2], wnd), np.float32))
    return np.stack(filled), dr, cls, counts, np.stack(last), np.stack(status)


@pytest.mark.parametrize("sched", ("0", "1", "2"))
@pytest.mark.parametrize("shape", sorted(PIPE_SHAPES))
def test_run_filled_equals_the_composition(flows, O, monkeypatch, shape, sched):
    """SMT_PIPE_SCHEDULE is read by smt_pipeline_create, so a handle created here takes it"""
    smt = flows
    monkeypatch.setenv("SMT_PIPE_SCHEDULE", sched)
    H, W, D, seed = PIPE_SHAPES[shape]
    L8, R8 = _pairs(O, H, W, D, seed)
    pipe = smt.Pipeline(H, W, D)
    try:
        before = pipe.run_post(L8, R8)
        want = _composition(O, pipe, L8, R8, 3)
        assert (want[5][:, 0] > 0).all() and (want[5][:, 1] > 0).all(), want[5].tolist()     # both lists are in play
        for rep in range(2):                                       # a reused handle
            got = pipe.run_filled(L8, R8)
            for g, w, n in zip(got, want, NAMES):
                same(g, w, (shape, sched, rep, n))
        after = pipe.run_post(L8, R8)
        for a, b in zip(before, after):
            same(b, a, (shape, sched, "run_post around a filled call"))
        pipe.status()
    finally:
        pipe.close()


def test_wrappers_and_shard(flows, O):
    smt = flows
    from stereo_match_traditional_amd import shard
    H, W, D, seed = PIPE_SHAPES["32x96"]
    L8, R8 = _pairs(O, H, W, D, seed)
    pipe = smt.Pipeline(H, W, D)
    want = pipe.run_filled(L8, R8)
    one = pipe.run_filled(L8[0], R8[0], median_wnd=3, invalid=float("inf"))       # [row][col] in
    for g, w in zip(one, want):
        same(g[0], w[0], "a single pair")
    five = pipe.run_filled(L8, R8, median_wnd=5)
    same(five[0], want[0], "the window does not reach dispL")
    same(five[4], np.stack([np.asarray(O.median(m, 5), np.float32) for m in want[0].cpu().numpy()]), "median 5")
    with pytest.raises(smt.SmtError):
        pipe.run_filled(L8, R8, median_wnd=8)
    with pytest.raises(smt.SmtError):
        pipe.run_filled(L8, R8, invalid=float("nan"))
    pipe.close()
    last, dl = shard.pipeline_filled_batch(L8, R8, D)
    same(last, want[4], "shard lastDisp"); same(dl, want[0], "shard dispL")
    e1, e2 = shard.pipeline_filled_batch(L8[:0], R8[:0], D)
    assert e1.shape == (0, H, W) and e2.dtype == torch.float32
    with pytest.raises(smt.SmtError):
        smt.FillHolesInDispMap(T(np.zeros((2, 3), np.float32)), T(np.zeros((2, 3), np.uint8)), invalid=float("nan"))
    with pytest.raises(ValueError):
        smt.FillHolesInDispMap(T(np.zeros((2, 3), np.float32)), T(np.zeros((3, 2), np.uint8)))


def fnv(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_adcensus_main_fill_holes(flows, O):
    """host/adcensus_main.cpp --fill-holes through the C++ mirror on the reference's signature (host/smt_fill_holes.hpp
    linked against the library): FNV-1a of the maps as the program prints them, against run_filled on the same synthetic
    pair; the program itself holds the device map to the host twin"""
    smt = flows
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "adcensus_main")
    H, W, D, seed = 32, 96, 64, 4
    r = subprocess.run([exe, "--fill-holes", str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = dict(line.split(None, 1) for line in r.stdout.splitlines())
    L, Rr = O.synth_pair(H, W, D, seed)
    pipe = smt.Pipeline(H, W, D)
    dl, dr, cls, counts, last, status = pipe.run_filled(T(L), T(Rr))
    pipe.close()
    assert out["filled_left"] == fnv(dl.cpu().numpy()) and out["median_left"] == fnv(last.cpu().numpy())
    assert out["fill_holes_status"].split() == [str(v) for v in status[0].cpu().tolist()]
    assert out["fill_holes_host_twin"] == "equal"
    assert int(status[0, 0]) > 0 and int(status[0, 1]) > 0
    r = subprocess.run([exe, "--fill-holes", "--refine", str(H), str(W), str(D), str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "give one" in r.stderr
