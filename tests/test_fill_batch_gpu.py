"""smt_fill_the_hole_batch on the GPU: bit-exact against the oracle's FillTheHole on the lists of the same class map and
against smt_fill_the_hole fed with smt_lrcheck_lists' lists (a second formulation: explicit lists, atomicMax winners, a
full-map third pass), on the cases of tests/test_fill_batch_cpu.py, at 1920 x 1080, chained behind the pipeline on one
stream, and its use of the scratch arena."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fill_batch_cases as fc  # noqa: E402
from fill_batch_cases import bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -(2 ** 31)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def strided(arrs, pad, fill, dtype):
    P, (H, W) = len(arrs), arrs[0].shape
    base = torch.full((P, H * W + pad), fill, dtype=dtype, device=DEV)
    view = base[:, :H * W].view(P, H, W)
    view.copy_(T(np.stack(arrs)))
    return base, view


def gpu_batch(smt, maps, clss, D, pad_d=0, pad_c=0):
    base, view = strided(maps, pad_d, 12345.0, torch.float32)
    _, cview = strided(clss, pad_c, 1, torch.uint8)
    status = smt.FillTheHoleBatch(view, cview, D)
    got = view.cpu().numpy()
    if pad_d:
        assert (base[:, -pad_d:] == 12345.0).all(), "wrote into the padding between maps"
    return [got[b] for b in range(len(maps))], status.cpu().numpy()


def single_call(smt, d, cls, D):
    """smt.FillTheHole with the lists smt_lrcheck_lists makes of cls."""
    from stereo_match_traditional_amd._lib import lib
    row, col = cls.shape
    ch = np.ascontiguousarray(cls)
    occ = np.empty((row * col, 2), np.int32)
    mis = np.empty((row * col, 2), np.int32)
    no, nm = C.c_int(), C.c_int()
    assert lib().smt_lrcheck_lists(ch.ctypes.data_as(C.c_void_p), row, col, occ.ctypes.data_as(C.c_void_p), C.byref(no),
                                   mis.ctypes.data_as(C.c_void_p), C.byref(nm)) == 0
    g = T(d)
    third = smt.FillTheHole(row, col, D, g, occ[:no.value], mis[:nm.value])
    return g.cpu().numpy(), no.value, nm.value, (len(third) if nm.value else -1)


def check_pair(smt, O, d, cls, D, tag):
    ref, st, _ = fc.expected(O, d, cls, D)
    (got,), status = gpu_batch(smt, [d], [cls], D)
    one, no, nm, nt = single_call(smt, d, cls, D)
    print(tag, "status", status[0].tolist(), "expected", st, "differing from the oracle", int((bits(got) != bits(ref)).sum()),
          "single call differing", int((bits(one) != bits(ref)).sum()))
    assert status[0].tolist() == st == [no, nm, nt, 0], tag
    assert np.array_equal(bits(got), bits(ref)), tag
    assert np.array_equal(bits(one), bits(ref)), tag


@pytest.mark.parametrize("row,col,D", fc.SHAPES)
def test_single_pairs_match_the_oracle_and_the_list_form(smt, O, row, col, D):
    d, cls = fc.lr_case(O, row, col, row * 7 + col)
    check_pair(smt, O, d, cls, D, (row, col, D))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_middle_row_in_one_list_only(smt, O, which):
    d, cls, D = fc.mid_case(O, which)
    check_pair(smt, O, d, cls, D, ("mid", which))


@pytest.mark.parametrize("row,col,D", [(37, 61, 32), (50, 70, 24)])
def test_batches_with_strides(smt, O, row, col, D):
    maps, clss = fc.batch_of_five(O, row, col, 300 + row)
    got, status = gpu_batch(smt, maps, clss, D, pad_d=37, pad_c=5)
    for b in range(5):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        (single,), s1 = gpu_batch(smt, [maps[b]], [clss[b]], D)
        assert status[b].tolist() == st == s1[0].tolist(), b
        assert np.array_equal(bits(got[b]), bits(ref)) and np.array_equal(bits(single), bits(ref)), b
    assert np.array_equal(bits(got[3]), bits(maps[3])) and status[3].tolist() == [0, 0, -1, 0]
    assert status[4, 1] == 0 and status[4, 2] == -1 and (got[4] == fc.HOLE).sum() > 0
    # dense batch, and the check=True form on a batch without flags
    dense, cd = T(np.stack(maps)), T(np.stack(clss))
    st2 = smt.FillTheHoleBatch(dense, cd, D, check=True)
    assert np.array_equal(bits(dense.cpu().numpy()), bits(np.stack(got))) and np.array_equal(st2.cpu().numpy(), status)
    # pairs == 0 is a no-op
    empty = smt.FillTheHoleBatch(dense[:0], cd[:0], D)
    assert tuple(empty.shape) == (0, 4)


def test_list_entries_outside_the_buffer_flag_the_pair_and_leave_it_alone(smt, O):
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
    maps, clss, D = fc.portrait_batch(O)
    got, status = gpu_batch(smt, maps, clss, D, pad_d=11)
    occ, mis = fc.lists(clss[1])
    with pytest.raises(ValueError):
        O.fill_the_hole(maps[1], D, occ, mis)
    assert status[1].tolist() == [len(occ), len(mis), -1, fc.UB_LIST]
    assert np.array_equal(bits(got[1]), bits(maps[1])), "a flagged pair must not be modified"
    for b in (0, 2):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        assert status[b].tolist() == st and np.array_equal(bits(got[b]), bits(ref)), b
    with pytest.raises(SmtError) as e:
        smt.FillTheHoleBatch(T(np.stack(maps)), T(np.stack(clss)), D, check=True)
    assert e.value.status == SMT_ERR_REF_UB and "pair 1" in str(e.value)


def test_more_holes_than_mismatches_applies_passes_0_and_1_only(smt, O):
    maps, clss, D = fc.third_overrun_batch(O)
    got, status = gpu_batch(smt, maps, clss, D)
    fc.check_third_overrun(O, maps[1], clss[1], D, got[1], status[1])
    for b in (0, 2):
        ref, st, _ = fc.expected(O, maps[b], clss[b], D)
        assert status[b].tolist() == st and np.array_equal(bits(got[b]), bits(ref)), b


def test_full_size_maps_with_lists_from_left_right_consistency(smt, O):
    """1920 x 1080, D = 192, 4 pairs: smt.LeftRightConsistency's map, cls and lists; pairs 2 and 3 get a seeded 2 % of
    65535 after the LR check.  Every map bit-equal to the oracle on those lists."""
    row, col, D = fc.FULL
    maps, clss, lsts = [], [], []
    for b in range(4):
        dL, dR, rng = fc.full_size_inputs(b)
        g = T(dL)
        cls, no, nm, occ, mis = smt.LeftRightConsistency(col, row, 2, g, T(dR), want_lists=True)
        d = g.cpu().numpy()
        if b >= 2:
            d[rng.random((row, col)) < 0.02] = fc.HOLE
        maps.append(d); clss.append(cls.cpu().numpy()); lsts.append((occ, mis))
    dev = T(np.stack(maps))
    status = smt.FillTheHoleBatch(dev, T(np.stack(clss)), D).cpu().numpy()
    got = dev.cpu().numpy()
    for b in range(4):
        occ, mis = lsts[b]
        ref, third = O.fill_the_hole(maps[b], D, occ, mis)
        diff = int((bits(got[b]) != bits(ref)).sum())
        print("pair", b, "status", status[b].tolist(), "oracle", [len(occ), len(mis), len(third), 0], "aliased",
              fc.aliased(clss[b]), "differing", diff)
        assert status[b].tolist() == [len(occ), len(mis), len(third), 0], b
        assert diff == 0, b
        assert (len(third) > 0) == (b >= 2)


def oracle_pipeline(O, L, R, D):
    cl = O.adcensus_view(L, R, D, 10.0, 30.0, 0)
    cr = O.adcensus_view(L, R, D, 10.0, 30.0, 1)
    al, _ = O.aggregate_rect(cl, O.arms_all(L), 0)
    ar, _ = O.aggregate_rect(cr, O.arms_all(R), 0)
    d_so, d_r = O.wta(O.scanline(al, L.astype(np.float32), 10, 150)), O.wta(ar)
    return O.lrcheck(d_so, d_r, 2)


def test_chain_behind_the_pipeline_on_one_stream(smt, O):
    """Pipeline.run -> FillTheHoleBatch(dispL, cls) -> RemoveSpecklesBatch -> MedianFilterBatch on one non-default
    stream, nothing synchronises in between; per pair the oracle's chain."""
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
    H, W, D, P = 64, 96, 32, 3
    pairs = [O.synth_pair(H, W, D, 30 + b) for b in range(P)]
    Lb = T(np.stack([p[0] for p in pairs]))
    Rb = T(np.stack([p[1] for p in pairs]))
    pipe = smt.Pipeline(H, W, D, DEV)
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dl, dr, cls, counts = pipe.run(Lb, Rb)
        status = smt.FillTheHoleBatch(dl, cls, D)
        smt.RemoveSpecklesBatch(dl, 1, 30, INT_MIN)
        last = smt.MedianFilterBatch(dl, 3)
    s.synchronize()
    try:
        pipe.status()
    except SmtError as e:
        assert e.status == SMT_ERR_REF_UB, e                              # as test_pipeline_batch_small_pairs_vs_oracle
    filled = 0
    for b, (L, R) in enumerate(pairs):
        lr, ocls, no, nm = oracle_pipeline(O, L, R, D)
        assert np.array_equal(cls[b].cpu().numpy(), ocls), b
        ref, st, _ = fc.expected(O, lr, ocls, D)
        filled += int((bits(ref) != bits(lr)).sum())
        assert status[b].cpu().tolist() == st, b
        sp = O.remove_speckles(ref, 1, 30, INT_MIN)
        assert np.array_equal(bits(dl[b].cpu().numpy()), bits(sp)), b
        assert np.array_equal(bits(last[b].cpu().numpy()), bits(O.median(sp, 3))), b
    assert filled > 0, "FillTheHole changed nothing on these pairs: the test would not see it"
    pipe.close()


def test_stream_order_behind_the_kernel_that_writes_cls(smt, O):
    """smt_lrcheck and the batch call enqueued back to back on a busy side stream: the call returns while the stream
    is still running and reads the cls (and the map) that the kernel before it writes."""
    from stereo_match_traditional_amd._lib import lib
    row, col, D = 50, 70, 24
    rng = np.random.default_rng(8)
    i, j = np.mgrid[0:row, 0:col]
    dL = ((i // 7 + j // 9) % 7 + 1).astype(np.float32)
    dL[rng.random((row, col)) < 0.08] = np.inf
    dR = dL.copy()
    redraw = rng.random((row, col)) < 0.15
    dR[redraw] = rng.integers(0, 12, int(redraw.sum())).astype(np.float32)
    lr, ocls, _, _ = O.lrcheck(dL, dR, 2)
    ref, st, _ = fc.expected(O, lr, ocls, D)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        warm, wcls = T(lr[None]), T(ocls[None])
        smt.FillTheHoleBatch(warm, wcls, D)                               # the arena holds the scratch from here on
        g, gr = T(dL[None]), T(dR)
        cls = torch.full((1, row, col), 7, dtype=torch.uint8, device=DEV)
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        sp = C.c_void_p(s.cuda_stream)
        assert lib().smt_lrcheck(C.c_void_p(g.data_ptr()), C.c_void_p(gr.data_ptr()), row, col, 2,
                                 C.c_void_p(cls.data_ptr()), None, sp) == 0
        status = smt.FillTheHoleBatch(g, cls, D)
        pending = not s.query()
    s.synchronize()
    assert pending, "smt_fill_the_hole_batch waited for the stream"
    assert np.array_equal(cls[0].cpu().numpy(), ocls)
    assert status[0].cpu().tolist() == st
    assert np.array_equal(bits(g[0].cpu().numpy()), bits(ref))


def test_scratch_comes_from_the_arena_and_does_not_grow(smt, O):
    row, col, D = 90, 120, 12
    cases = [fc.lr_case(O, row, col, 900 + b) for b in range(3)]
    src, cls = T(np.stack([c[0] for c in cases])), T(np.stack([c[1] for c in cases]))
    work = src.clone()
    smt.FillTheHoleBatch(work, cls, D)
    torch.cuda.synchronize()
    first = work.clone()
    reserved, _ = smt.scratch_info()
    assert reserved >= 3 * row * col * 4
    for _ in range(10):
        work.copy_(src)
        smt.FillTheHoleBatch(work, cls, D)
    torch.cuda.synchronize()
    assert smt.scratch_info()[0] == reserved
    assert torch.equal(work.view(torch.int32), first.view(torch.int32))


def fnv(a):
    h = 1469598103934665603
    for x in np.ascontiguousarray(a).view(np.uint8).reshape(-1).tolist():
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_cpp_host_mirror(smt, O):
    """host/fill_main.cpp: smt::FillTheHoleBatch of smt_host.hpp on maps this test rebuilds (one LCG step per pixel)."""
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "fill_main")
    P, row, col, D, seed = 3, 40, 90, 16, 5
    out = subprocess.run([exe, str(P), str(row), str(col), str(D), str(seed)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    n = row * col
    s = seed
    disp = np.empty(P * n, np.float32)
    cls = np.empty(P * n, np.uint8)
    for k in range(P * n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        c, h = s >> 28, (s >> 23) & 31
        cls[k] = 1 if c == 0 else 2 if c <= 3 else 0
        disp[k] = np.inf if cls[k] else 65535.0 if h == 0 else float((s >> 16) & 15)
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(lines) == P
    for b in range(P):
        ref, st, _ = fc.expected(O, disp[b * n:(b + 1) * n].reshape(row, col), cls[b * n:(b + 1) * n].reshape(row, col), D)
        assert lines[b][:2] == ["pair", str(b)]
        assert [int(x) for x in lines[b][3:]] == st, b
        assert int(lines[b][2], 16) == fnv(ref), b
