"""The bilateral image filter on the device (include/smt_bilateral.h), bit for bit against the NumPy restatement of
tests/bilateral_cases.py, on the float64 sums and on the bytes, under both norms: the direct form, the staged form and
the default dispatch on every shape of the table.  Outputs are prefilled (tests/prefill.py) or sit between guards
(tests/arena.py); one case runs behind a sleep on a side stream.  Then the wrappers: api.bilateralfiter,
shard.bilateral_batch and host/bilateral_main.cpp.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bilateral_cases as B  # noqa: E402
from prefill import first_diff, flows  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (B.DIRECT, B.STAGED)


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the table's arrays are read-only


def same(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (what, first_diff(got, ref))


@pytest.fixture
def hooks(flows):
    yield flows
    flows.bilateral_set_impl(0)


def every_form(smt, img, wsize, space, color, norm, rdst, racc, what):
    """the direct form, the staged form and the default dispatch, with and without the sums"""
    t, tabs = T(img), (T(space), T(color))
    for impl in FORMS + (0,):
        smt.bilateral_set_impl(impl)
        dst, acc = smt.bilateralfiter(t, wsize, norm=norm, return_acc=True, tables=tabs)
        form = smt.bilateral_last_form()
        assert form == impl if impl else form in FORMS, (what, impl, form)
        same(acc, racc, what + (impl, "acc")); same(dst, rdst, what + (impl, "bytes"))
        same(smt.bilateralfiter(t, wsize, norm=norm, tables=tabs), rdst, what + (impl, "bytes, no acc"))
    same(t, img, what + ("the input",))


@pytest.mark.parametrize("gid,kind,H,W,ch", B.groups(), ids=[g[0] for g in B.groups()])
def test_every_form_equals_the_restatement(hooks, gid, kind, H, W, ch):
    img = B.image(kind, H, W, ch)
    for wsize, ss, sc in B.windows_for((H, W)):
        space, color = B.tables(wsize, ss, sc)
        for norm in B.NORMS:
            rdst, racc = B.restate(kind, H, W, ch, wsize, ss, sc, norm)
            every_form(hooks, img, wsize, space, color, norm, rdst, racc, (gid, wsize, norm))


@pytest.mark.parametrize("value,wsize,want", B.FLAT, ids=[f"flat{v}-{w[0]}x{w[1]}" for v, w, _ in B.FLAT])
def test_flat_images_lose_a_grey_level_where_the_sums_say_so(hooks, value, wsize, want):
    space, color = B.tables(wsize, 10, 30)
    for ch in B.CHANNELS:
        img = B.image(("flat", value), *B.FLAT_SHAPE, ch)
        for norm in B.NORMS:
            rdst, racc = B.restate(("flat", value), *B.FLAT_SHAPE, ch, wsize, 10, 30, norm)
            if norm == B.RECIPROCAL:
                assert (rdst == want).all()
            every_form(hooks, img, wsize, space, color, norm, rdst, racc, ("flat", value, wsize, ch, norm))


def test_three_images_in_one_call_equal_three_calls(hooks):
    smt = hooks
    for ch, wsize in ((3, (7, 3)), (1, (23, 23))):
        one = B.image("noise", 17, 65, ch)
        imgs = np.stack([one, B.image("stairs", 17, 65, ch), one[::-1, ::-1].copy()])
        space, color = B.tables(wsize, 10, 30)
        tabs = (T(space), T(color))
        stack = T(imgs) if ch == 3 else T(imgs[..., None])
        for norm in B.NORMS:
            for impl in FORMS:
                smt.bilateral_set_impl(impl)
                dst, acc = smt.bilateralfiter(stack, wsize, norm=norm, return_acc=True, tables=tabs)
                dst, acc = dst.reshape(imgs.shape), acc.reshape(imgs.shape)
                for k in range(3):
                    d1, a1 = smt.bilateralfiter(T(imgs[k]), wsize, norm=norm, return_acc=True, tables=tabs)
                    rdst, racc = B.restate_with(imgs[k], wsize, space, color, norm)
                    same(dst[k], d1, (ch, norm, impl, k, "bytes")); same(acc[k], a1, (ch, norm, impl, k, "acc"))
                    same(d1, rdst, (ch, norm, impl, k, "bytes, restatement")); same(a1, racc, (ch, norm, impl, k, "acc, restatement"))


def test_more_images_than_the_grid_holds(hooks):
    """the images axis of the grid stops at 1 024 and a workgroup walks on from there (the staged form stages a second
    tile into the same LDS): 1 030 small images against the host twin, which the CPU tests hold to the restatement"""
    smt = hooks
    from stereo_match_traditional_amd import _lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n, H, W, ch, wsize = 1030, 2, 3, 3, (3, 5)
    imgs = np.random.RandomState(11).randint(0, 256, (n, H, W, ch)).astype(np.uint8)
    space, color = (np.array(t) for t in B.tables(wsize, 10, 30))
    hdst, hacc = np.full(imgs.shape, 0xEE, np.uint8), np.full(imgs.shape, np.nan)
    assert _lib.lib().smt_bilateral_filter_host(vp(imgs), n, H, W, ch, wsize[0], wsize[1], vp(space), vp(color), B.RECIPROCAL, vp(hdst), vp(hacc)) == 0
    same(hdst[1029], B.restate_with(imgs[1029], wsize, space, color, B.RECIPROCAL)[0], "the host twin's last image")
    for impl in FORMS:
        smt.bilateral_set_impl(impl)
        dst, acc = smt.bilateralfiter(T(imgs), wsize, return_acc=True, tables=(T(space), T(color)))
        same(dst, hdst, (impl, "bytes")); same(acc, hacc, (impl, "acc"))


def test_hostile_tables_against_the_host_twin(hooks):
    """all zeros: every weight and every sum of weights 0, the sums of pass 2 NaN, the bytes 0; 1e300 throughout: the
    weights overflow and S is infinite.  A NaN's sign and payload are the processor's, so the sums are compared as NaN
    where the host twin's are NaN and bit for bit elsewhere."""
    smt = hooks
    from stereo_match_traditional_amd import _lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for ch in B.CHANNELS:
        img = np.ascontiguousarray(B.image("noise", 9, 33, ch))
        for wsize in ((5, 5), (4, 6)):
            real_space, real_color = B.tables(wsize, 10, 30)
            for fill, part in ((0.0, "all"), (1e300, "all"), (1e300, "space"), (0.0, "color")):
                space = np.full(wsize, fill) if part in ("all", "space") else np.array(real_space)
                color = np.full(256, fill) if part in ("all", "color") else np.array(real_color)
                for norm in B.NORMS:
                    hdst, hacc = np.full(img.shape, 0xEE, np.uint8), np.full(img.shape, 1.5)
                    assert _lib.lib().smt_bilateral_filter_host(vp(img), 1, 9, 33, ch, wsize[0], wsize[1], vp(space), vp(color), norm,
                                                                vp(hdst), vp(hacc)) == 0
                    if part == "all" or fill == 0.0:
                        assert (hdst == 0).all() and np.isnan(hacc).all(), (fill, part, norm)
                    for impl in FORMS:
                        smt.bilateral_set_impl(impl)
                        dst, acc = smt.bilateralfiter(T(img), wsize, norm=norm, return_acc=True, tables=(T(space), T(color)))
                        same(dst, hdst, (ch, wsize, fill, part, norm, impl, "bytes"))
                        acc = acc.cpu().numpy()
                        nan = np.isnan(hacc)
                        assert np.array_equal(np.isnan(acc), nan), (ch, wsize, fill, part, norm, impl, "NaNs")
                        assert np.array_equal(B.bits(np.where(nan, 0.0, acc)), B.bits(np.where(nan, 0.0, hacc))), (ch, wsize, fill, part, norm, impl)


ARENA = [((9, 33), 3, (63, 63), B.STAGED), ((9, 33), 1, (64, 64), B.STAGED), ((17, 65), 3, (4, 6), B.STAGED), ((17, 65), 1, (23, 23), B.STAGED),
         ((20, 31), 3, (3, 7), B.DIRECT), ((1, 70), 1, (7, 3), B.DIRECT), ((7, 1), 3, (5, 5), B.STAGED), ((1, 1), 1, (25, 25), B.STAGED)]


@pytest.mark.parametrize("shape,ch,wsize,impl", ARENA, ids=[f"{s[0]}x{s[1]}x{c}-{w[0]}x{w[1]}-{i}" for s, c, w, i in ARENA])
def test_in_the_arena(hooks, shape, ch, wsize, impl):
    """guards on both sides of every tensor, both prefill seeds (one all-NaN), the scratch arena poisoned, the inputs and
    both tables untouched; two images, so that the second starts where the first ends"""
    smt = hooks
    from stereo_match_traditional_amd import _lib
    lib = _lib.lib()
    H, W = shape
    one = B.image("noise", H, W, ch)
    imgs = np.stack([one, one[::-1, ::-1].copy()])
    space, color = B.tables(wsize, 10, 30)
    smt.bilateral_set_impl(impl)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for norm, byte in ((B.RECIPROCAL, 0xFF), (B.DIVIDE, 0x00)):
        smt.scratch_poison(byte)

        def make(A):
            A.inp("src", imgs); A.inp("space", space); A.inp("color", color)
            A.out("dst", imgs.shape, np.uint8); A.out("acc", imgs.shape, np.float64)
            return lambda A: lib.smt_bilateral_filter_batch(A.ptr("src"), 2, H, W, ch, wsize[0], wsize[1], A.ptr("space"), A.ptr("color"),
                                                            norm, A.ptr("dst"), A.ptr("acc"), st())
        out, _ = arena.run_two_seeds(make, "cuda:0", torch.cuda.synchronize)
        assert smt.bilateral_last_form() == impl
        for k in range(2):
            rdst, racc = B.restate_with(imgs[k], wsize, space, color, norm)
            same(out["dst"][k], rdst, (shape, ch, wsize, impl, norm, k, "bytes")); same(out["acc"][k], racc, (shape, ch, wsize, impl, norm, k, "acc"))

        def make_no_acc(A):
            A.inp("src", imgs); A.inp("space", space); A.inp("color", color); A.out("dst", imgs.shape, np.uint8)
            return lambda A: lib.smt_bilateral_filter_batch(A.ptr("src"), 2, H, W, ch, wsize[0], wsize[1], A.ptr("space"), A.ptr("color"),
                                                            norm, A.ptr("dst"), None, st())
        out2, _ = arena.run_two_seeds(make_no_acc, "cuda:0", torch.cuda.synchronize)
        same(out2["dst"], out["dst"], (shape, ch, wsize, impl, norm, "without acc"))


@pytest.mark.parametrize("impl", FORMS)
def test_asynchronous_on_a_busy_side_stream(hooks, impl):
    """enqueued behind a long sleep on a side stream, the call returns while the stream is still busy and reads the image
    that a copy behind the sleep put there: it is ordered on that stream"""
    smt = hooks
    H, W, ch, wsize = 17, 65, 3, (23, 23)
    img = B.image("noise", H, W, ch)
    rdst, racc = B.restate("noise", H, W, ch, wsize, 10, 30, B.RECIPROCAL)
    smt.bilateral_set_impl(impl)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        a = T(img)
        t = torch.zeros_like(a)
        smt.bilateralfiter(t, wsize)                           # the tables of this parameter set are on the device
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        t.copy_(a, non_blocking=True)
        dst, acc = smt.bilateralfiter(t, wsize, return_acc=True)
        pending = not s.query()
    s.synchronize()
    assert pending, "the call waited for the stream"
    same(dst, rdst, (impl, "bytes")); same(acc, racc, (impl, "acc"))


def test_api_shapes_and_the_table_cache(hooks):
    smt = hooks
    from stereo_match_traditional_amd import api
    g, c = B.image("noise", 20, 31, 1), B.image("noise", 20, 31, 3)
    rg = B.restate("noise", 20, 31, 1, (23, 23), 10, 30, B.RECIPROCAL)
    rc = B.restate("noise", 20, 31, 3, (23, 23), 10, 30, B.RECIPROCAL)
    d, a = smt.bilateralfiter(T(g), return_acc=True)                         # the defaults: 23 x 23, sigma 10 / 30, reciprocal
    same(d, rg[0], "[H,W]"); same(a, rg[1], "[H,W] acc")
    d, a = smt.bilateralfiter(T(c), return_acc=True)
    same(d, rc[0], "[H,W,3]"); same(a, rc[1], "[H,W,3] acc")
    n_tables = len(api._bilateral_tables)
    d = smt.bilateralfiter(T(np.stack([c, c[::-1].copy()])), (23, 23), 10, 30)
    assert len(api._bilateral_tables) == n_tables                            # the same parameter set: the cached tables
    same(d[0], rc[0], "[n,H,W,3] 0"); same(d[1], B.restate_with(c[::-1], (23, 23), *B.tables((23, 23), 10, 30), B.RECIPROCAL)[0], "[n,H,W,3] 1")
    d = smt.bilateralfiter(T(np.stack([g, g])))
    assert d.shape == (2, 20, 31)
    same(d[0], rg[0], "[n,H,W] 0"); same(d[1], rg[0], "[n,H,W] 1")
    d = smt.bilateralfiter(T(c), 25, 50, 25, norm=smt.BILATERAL_NORM_DIVIDE)     # one side: a square window
    same(d, B.restate("noise", 20, 31, 3, (25, 25), 50, 25, B.DIVIDE)[0], "25, 50 / 25, divide")
    sp, cm = smt.bilateral_masks((4, 6), 10, 30, DEV)
    assert sp.shape == (4, 6) and cm.shape == (256,) and sp.dtype == torch.float64
    with pytest.raises(ValueError):
        smt.bilateralfiter(T(np.zeros((2, 3, 4, 2), np.uint8)))
    with pytest.raises(ValueError):
        smt.bilateral_masks((65, 3), 10, 30, DEV)
    with pytest.raises(TypeError):
        smt.bilateralfiter(T(g).to(torch.float32))
    with pytest.raises(smt.SmtError):
        smt.bilateralfiter(T(g), norm=5)


def test_shard_bilateral_batch(hooks):
    from stereo_match_traditional_amd import shard
    L8 = np.stack([B.image("noise", 9, 33, 1), B.image("stairs", 9, 33, 1)])
    R8 = np.stack([B.image("stairs", 9, 33, 1)[::-1].copy(), B.image("noise", 9, 33, 1)[:, ::-1].copy()])
    fl, fr = shard.bilateral_batch(T(L8), T(R8), None, wsize=(5, 5))
    gl, gr = shard.run_sharded(T(L8), T(R8), None, lambda a, b, d: shard.bilateral_batch(a, b, d, wsize=(5, 5)))
    space, color = B.tables((5, 5), 10, 30)
    for k in range(2):
        same(fl[k], B.restate_with(L8[k], (5, 5), space, color, B.RECIPROCAL)[0], ("left", k))
        same(fr[k], B.restate_with(R8[k], (5, 5), space, color, B.RECIPROCAL)[0], ("right", k))
    same(gl, fl, "run_sharded left"); same(gr, fr, "run_sharded right")
    el, er = shard.bilateral_batch(T(L8)[:0], T(R8)[:0])
    assert el.shape == (0, 9, 33) and er.dtype == torch.uint8


def fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).reshape(-1).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_bilateral_main(smt, tmp_path):
    """host/bilateral_main.cpp on a PPM written here: TeddyBilateral.cpp's window and sigmas by default, the overrides,
    the written file and the printed hash against the restatement (the file holds R, G, B; the filter treats every
    channel on its own, so it commutes with the channel order)"""
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "bilateral_main")
    assert os.path.exists(exe)
    H, W = 20, 31
    rgb = B.image("noise", H, W, 3)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (W, H) + rgb.tobytes())
    for extra, wsize, ss, sc, norm in (((), (25, 25), 50, 25, B.RECIPROCAL), (("--wsize", "5", "--sigma", "10", "30", "--divide"), (5, 5), 10, 30, B.DIVIDE),
                                       (("--wsize", "6", "4"), (4, 6), 50, 25, B.RECIPROCAL)):
        out = tmp_path / "out.ppm"
        r = subprocess.run([exe, str(src), str(out), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = B.restate_with(rgb, wsize, *B.tables(wsize, ss, sc), norm)[0]
        raw = out.read_bytes()
        head = b"P6\n%d %d\n255\n" % (W, H)
        assert raw.startswith(head) and len(raw) == len(head) + H * W * 3
        got = np.frombuffer(raw[len(head):], np.uint8).reshape(H, W, 3)
        same(got, want, (extra, "the written file"))
        assert r.stdout.split() == ["target", f"{fnv1a(want[:, :, ::-1]):016x}"], (extra, r.stdout)     # B, G, R in memory
    assert subprocess.run([exe, str(src)], capture_output=True, text=True).returncode == 1
