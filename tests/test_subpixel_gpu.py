"""Sub-pixel disparities on the device, bit for bit against the NumPy restatement of tests/subpixel_cases.py:
the volume kernel smt_wta_subpixel on the whole case table (hostile prefill, default and side stream, a volume that is
4-byte but not 16-byte aligned); the rule fused into smt_crossarm_aggregate and smt_scanline_run against the composed
route (smt_wta_subpixel of the volume the same call wrote) and against the oracle's volumes; the pipeline under every
schedule against the composition from the oracle, with the fraction check that fails without the feature and the
switch-off check; shard.pipeline_batch and adcensus_main --subpixel."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bounds_cases as BC  # noqa: E402
import subpixel_cases as SP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -(2 ** 31)
_O = None


@pytest.fixture(autouse=True)
def _oracle(O):
    global _O
    _O = O


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, ref, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    bad = bits(got) != bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def hostile(shape):
    """a map no kernel writes: NaN words with a payload"""
    return torch.full(shape, float("nan"), device=DEV).view(torch.int32).bitwise_or_(0x5A5A5).view(torch.float32)


# ------------------------------------------------------------------------------------------------ the volume kernel
@pytest.mark.parametrize("D,min_den,shape", SP.TABLE, ids=[f"D{d}-m{m:g}-{s[0]}x{s[1]}" for d, m, s in SP.TABLE])
def test_volume_kernel_equals_the_restatement(smt, O, D, min_den, shape):
    H, W = shape
    vol = SP.volume(D, shape)
    ref = SP.restate(O, vol, min_den)
    # the volume one float behind a 256-byte aligned allocation: 4-byte aligned, never 16
    buf = torch.empty(H * W * D + 4, device=DEV)
    v = buf[1:1 + H * W * D].view(H, W, D)
    v.copy_(T(vol))
    assert v.data_ptr() % 16 == 4
    d0 = hostile((H, W))
    smt.wta_subpixel(v, min_den, d0)
    same(d0, ref, "default stream, offset volume")
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        va = T(vol)                                        # 16-byte aligned: the vector load where D == 64 C
        d1 = hostile((H, W))
        smt.wta_subpixel(va, min_den, d1)
    s.synchronize()
    same(d1, ref, "side stream, aligned volume")


@pytest.mark.parametrize("params", SP.BOUNDS, ids=BC.case_id)
def test_volume_kernel_in_the_arena(smt, O, params):
    """guards on both sides of both tensors, both prefill seeds, the input untouched (tests/test_bounds_gpu.py's rules)"""
    SP.run_case(BC.Ctx(O, "cuda:0"), False, params)


def test_volume_kernel_is_asynchronous_on_the_callers_stream(smt, O):
    """enqueued behind a long sleep on a side stream, the call returns while the stream is still busy, and reads the
    volume that a copy behind the sleep put there: it is ordered on that stream"""
    D, shape = 192, SP.SHAPES[-1]
    vol = SP.volume(D, shape)
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        src, v, d = T(vol), torch.zeros(shape + (D,), device=DEV), hostile(shape)
        s.synchronize()
        torch.cuda._sleep(400_000_000)
        v.copy_(src, non_blocking=True)
        smt.wta_subpixel(v, 1.0, d)
        pending = not s.query()
    s.synchronize()
    assert pending, "smt_wta_subpixel waited for the stream"
    same(d, SP.restate(O, vol, 1.0), "behind the sleep")


# ------------------------------------------------------------------------------------------------ aggregation
def smooth_img(H, W, seed, step=3):
    rng = np.random.default_rng(seed)
    base = (np.add.outer(np.arange(H) // 9, np.arange(W) // 23) * 17) % 200 + 20
    return (base + rng.integers(0, step, (H, W))).astype(np.uint8)


def _img(H, W, kind, seed):
    if kind == "synth":
        return _O.synth_pair(H, W, 32, seed)[0]
    if kind == "noise":
        return _O.synth_pair(H, W, 32, seed, True)[0]
    if kind == "smooth":
        return smooth_img(H, W, seed)
    return np.full((H, W), 77, np.uint8)


# tests/test_pipeline_gpu.py's AGG_CASES, plus D = 65 (two registers, partial), 192 is among them, 300 (the plain walk)
AGG_CASES = [(72, 160, 16, "synth", 3), (64, 150, 64, "smooth", 5), (72, 160, 100, "noise", 4),
             (48, 180, 192, "synth", 8), (50, 183, 128, "smooth", 9), (40, 200, 256, "flat", 0),
             (70, 155, 60, "smooth", 12), (66, 149, 7, "synth", 13), (30, 70, 65, "smooth", 14), (44, 150, 300, "synth", 15)]
MIN_DEN_AGG = 2.0 ** -6                                    # costs in [0, 2): below the clamp of 1 on most pixels, above it on some


@functools.lru_cache(maxsize=None)
def agg_reference(H, W, D, kind, seed, order):
    img = _img(H, W, kind, seed)
    vol = np.random.default_rng(seed).random((H, W, D), dtype=np.float32) * 2
    arms = _O.arms_all(img) if order == 0 else _O.arms_all(img, 25, 6, 17, 34, chain=False, right_row_bug=False)
    ref, oob = _O.aggregate_rect(vol, arms, order)
    assert oob == 0
    return img, vol, ref, SP.restate(_O, ref, MIN_DEN_AGG), _O.wta(ref)


@pytest.mark.parametrize("H,W,D,kind,seed", AGG_CASES)
@pytest.mark.parametrize("order", [0, 1])
def test_aggregation_fused_against_composed_every_variant(smt, O, H, W, D, kind, seed, order):
    img, vol, ref, sub, whole = agg_reference(H, W, D, kind, seed, order)
    assert (sub != np.floor(sub)).any()
    ca = smt.CrossArmAggregation().Initialize(H, W, 30 if order == 0 else 25, D, DEV, style="adcensus" if order == 0 else "cblsm")
    ca.ComputeArmLengths(T(img))
    run = ca.AggregationVertical if order == 0 else ca.costAggregationV5
    tv = T(vol)
    for variant in range(14):
        ca.set_variant(variant)
        ca.set_subpixel(MIN_DEN_AGG)
        out, disp = hostile((H, W, D)), hostile((H, W))
        run(tv, out, disp)
        same(out, ref, ("vout", variant))
        same(disp, smt.wta_subpixel(out, MIN_DEN_AGG), ("fused against composed", variant))
        same(disp, sub, ("against the oracle's volume", variant))
        ca.set_subpixel(None)
        disp0 = hostile((H, W))
        run(tv, hostile((H, W, D)), disp0)
        same(disp0, whole, ("switched off", variant))
    ca.status()
    ca.close()


# ------------------------------------------------------------------------------------------------ scanline
# tests/test_pipeline_gpu.py's SCAN_CASES sizes at D = 60, 64, 65, 192 (one register partial / full, two partial, three full)
SCAN_SUB = [(20, 40, 60, 3), (12, 70, 64, 4), (9, 33, 65, 5), (10, 50, 192, 6), (1, 9, 64, 9), (9, 1, 65, 10)]


@pytest.mark.parametrize("H,W,D,seed", SCAN_SUB)
@pytest.mark.parametrize("fixv", [False, True])
def test_scanline_fused_against_composed(smt, O, H, W, D, seed, fixv):
    rng = np.random.default_rng(seed)
    cost = rng.random((H, W, D), dtype=np.float32) * 2
    gray = rng.integers(0, 256, (H, W)).astype(np.float32)
    so = smt.ScanlineOptimizer().Initialize(H, W, D, 10, 150, DEV, quirks=smt.QUIRK_FIX_SCAN_VERTICAL if fixv else 0)
    for min_den in (1.0, 2.0 ** -20):
        so.set_subpixel(min_den)
        disp = hostile((H, W))
        out = so.ScanLine(T(cost), T(gray), disp=disp)
        same(disp, smt.wta_subpixel(out, min_den), ("fused against composed", min_den))
        same(disp, SP.restate(O, out.cpu().numpy(), min_den), ("against the restatement", min_den))
        if not fixv:
            ref = O.scanline(cost, gray, 10, 150)
            same(out, ref, "sum")
            same(disp, SP.restate(O, ref, min_den), ("against the oracle's volume", min_den))
    so.set_subpixel(None)
    disp0 = hostile((H, W))
    out0 = so.ScanLine(T(cost), T(gray), disp=disp0)
    same(out0, out.cpu().numpy(), "the sum does not depend on the switch")
    same(disp0, O.wta(out0.cpu().numpy()), "switched off")
    so.close()


# ------------------------------------------------------------------------------------------------ pipeline
PIPE_SHAPES = [(24, 120, 32), (72, 160, 64)]
P = 3


@functools.lru_cache(maxsize=None)
def pipeline_volumes(H, W, D):
    """per pair: the images, the oracle's scanline sum of the left view and its aggregated right volume"""
    out = []
    for b in range(P):
        L, R = _O.synth_pair(H, W, D, 30 + b, b == 1)
        cl = _O.adcensus_view(L, R, D, 10.0, 30.0, 0)
        cr = _O.adcensus_view(L, R, D, 10.0, 30.0, 1)
        al, _ = _O.aggregate_rect(cl, _O.arms_all(L), 0)
        ar, _ = _O.aggregate_rect(cr, _O.arms_all(R), 0)
        out.append((L, R, _O.scanline(al, L.astype(np.float32), 10, 150), ar))
    return out


@functools.lru_cache(maxsize=None)
def pipeline_reference(H, W, D, min_den):
    """per pair: the composition from the oracle, refined (min_den) or whole (None)"""
    out = []
    for L, R, so, ar in pipeline_volumes(H, W, D):
        pick = (lambda v: _O.wta(v)) if min_den is None else (lambda v: SP.restate(_O, v, min_den))
        d_so, d_r = pick(so), pick(ar)
        lr, cls, no, nm = _O.lrcheck(d_so, d_r, 2)
        sp = _O.remove_speckles(lr, 1, 30, INT_MIN)
        out.append(dict(L=L, R=R, raw=d_so, dispL=lr, dispR=d_r, cls=cls, counts=(no, nm), speckled=sp, last=_O.median(sp, 3)))
    return out


def _status(pipe):
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import SMT_ERR_REF_UB
    try:
        pipe.status()
    except SmtError as e:
        assert e.status == SMT_ERR_REF_UB, e                 # a noise pair's rectangles may leave the plane, as in the other pipeline tests


def _check_run(res, ref, post, what):
    dl, dr, cls, counts = res[:4]
    for b, r in enumerate(ref):
        same(dl[b], r["speckled"] if post else r["dispL"], what + ("dispL", b))
        same(dr[b], r["dispR"], what + ("dispR", b))
        assert np.array_equal(cls[b].cpu().numpy(), r["cls"]), what + ("cls", b)
        assert tuple(counts[b].cpu().tolist()) == r["counts"], what + ("counts", b)
        if post:
            same(res[4][b], r["last"], what + ("lastDisp", b))


@pytest.mark.parametrize("H,W,D", PIPE_SHAPES)
@pytest.mark.parametrize("schedule", ["0", "1", "2"])
def test_pipeline_against_the_composition_from_the_oracle(smt, O, H, W, D, schedule, monkeypatch):
    monkeypatch.setenv("SMT_PIPE_SCHEDULE", schedule)                # read at create
    min_den = 1.0
    ref, whole = pipeline_reference(H, W, D, min_den), pipeline_reference(H, W, D, None)
    Lb, Rb = T(np.stack([r["L"] for r in ref])), T(np.stack([r["R"] for r in ref]))
    pipe = smt.Pipeline(H, W, D, DEV, subpixel=min_den)
    for rep in range(2):                                              # twice on one handle
        _check_run(pipe.run(Lb, Rb), ref, False, (schedule, rep, "run"))
        _check_run(pipe.run_post(Lb, Rb), ref, True, (schedule, rep, "run_post"))
    _status(pipe)
    # the fraction check: the maps hold fractions, and the integer pipeline's maps are other maps
    dl, dr, _, _ = pipe.run(Lb, Rb)
    for t, key in ((dl, "dispL"), (dr, "dispR")):
        m = t.cpu().numpy()
        fin = np.isfinite(m)
        assert (m[fin] != np.floor(m[fin])).sum() > m.size // 20, key
        assert not np.array_equal(bits(m), bits(np.stack([r[key] for r in whole]))), key
    # switched off on the same handle: the integer maps again, bit for bit
    pipe.set_subpixel(None)
    _check_run(pipe.run(Lb, Rb), whole, False, (schedule, "off", "run"))
    _check_run(pipe.run_post(Lb, Rb), whole, True, (schedule, "off", "run_post"))
    pipe.set_subpixel(2.0 ** -20)                                     # and on again with another parameter
    _check_run(pipe.run(Lb, Rb), pipeline_reference(H, W, D, 2.0 ** -20), False, (schedule, "2^-20", "run"))
    _status(pipe)
    pipe.close()


def test_setters_reject_bad_parameters(smt):
    from stereo_match_traditional_amd import SmtError
    pipe = smt.Pipeline(8, 40, 8, DEV)
    so = smt.ScanlineOptimizer().Initialize(8, 40, 8, 10, 150, DEV)
    ca = smt.CrossArmAggregation().Initialize(8, 40, 30, 8, DEV)
    for h in (pipe, so, ca):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(SmtError):
                h.set_subpixel(bad)
        h.set_subpixel(0.5); h.set_subpixel(None)
        h.close()


# ------------------------------------------------------------------------------------------------ the other layers
def test_shard_pipeline_batch_on_one_rank(smt, O):
    from stereo_match_traditional_amd import shard
    H, W, D = PIPE_SHAPES[0]
    ref = pipeline_reference(H, W, D, 1.0)
    Lb, Rb = T(np.stack([r["L"] for r in ref])), T(np.stack([r["R"] for r in ref]))
    dl, dr = shard.run_sharded(Lb, Rb, D, lambda l, r, d: shard.pipeline_batch(l, r, d, subpixel=1.0))
    for b, r in enumerate(ref):
        same(dl[b], r["dispL"], ("dispL", b)); same(dr[b], r["dispR"], ("dispR", b))
    dl0, _ = shard.pipeline_batch(Lb, Rb, D)
    for b, r in enumerate(pipeline_reference(H, W, D, None)):
        same(dl0[b], r["dispL"], ("integer dispL", b))


def test_adcensus_main_subpixel_from_image_files(smt, O, tmp_path):
    """tests/test_cpp_host_gpu.py's file path (imread -> cvtColor -> the stages -> imwrite) with --subpixel: the maps of
    the aggregation and of the scanline optimiser are the restatement of the oracle's volumes, and the LR check runs on
    them"""
    import struct
    import zlib
    exe = os.path.join(ROOT, "stereo_match_traditional_amd", "lib", "adcensus_main")
    assert os.path.exists(exe)

    def png(path, bgr):
        H, W, _ = bgr.shape
        raw = b"".join(b"\x00" + bgr[r, :, ::-1].tobytes() for r in range(H))
        ch = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
        path.write_bytes(b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                         ch(b"IDAT", zlib.compress(raw, 6)) + ch(b"IEND", b""))

    H, W, D = 48, 120, 32
    L, R = O.synth_pair(H, W, D, 7)
    Lb, Rb = O.synth_bgr(L, 3), O.synth_bgr(R, 4)
    png(tmp_path / "l.png", Lb); png(tmp_path / "r.png", Rb)
    Lg, Rg = O.bgr2gray(Lb), O.bgr2gray(Rb)
    cl, cr = O.adcensus_view(Lg, Rg, D, 10.0, 30.0, 0), O.adcensus_view(Lg, Rg, D, 10.0, 30.0, 1)
    al, _ = O.aggregate_rect(cl, O.arms_all(Lg), 0)
    ar, _ = O.aggregate_rect(cr, O.arms_all(Rg), 0)
    so = O.scanline(al, Lg.astype(np.float32), 10, 150)
    for args, min_den in ((["--subpixel"], 1.0), (["--subpixel", "0.015625"], 2.0 ** -6)):
        r = subprocess.run([exe, "--images", str(tmp_path / "l.png"), str(tmp_path / "r.png"), str(D), str(tmp_path / "d.png")] + args,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = dict(line.split() for line in r.stdout.strip().splitlines())
        dl, dr = SP.restate(O, so, min_den), SP.restate(O, ar, min_den)
        lr, cls, no, nm = O.lrcheck(dl, dr, 2)
        assert got["agg_left"] == f"{O.fnv1a(al):016x}" and got["wta_left"] == f"{O.fnv1a(O.wta(cl)):016x}"
        assert got["so_wta_left"] == f"{O.fnv1a(dl):016x}", min_den
        assert got["lr_left"] == f"{O.fnv1a(lr):016x}", min_den
        assert int(got["n_occlusion"]) == no and int(got["n_mismatch"]) == nm
        assert got["so_wta_left"] != f"{O.fnv1a(O.wta(so)):016x}"
