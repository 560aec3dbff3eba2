"""Image-pair sharding for the batched configuration (configs[4]: 256 KITTI-size pairs over
the 8 GPUs of a node).  Pairs are independent -- no halo, no exchange on the compute path --
so each rank runs a contiguous block of pairs on its own GPU; the only collective is the
final gather of the [pairs, H, W] disparity maps (1.86 MB each at 1242x375) plus an 8-byte
checksum all-reduce.  Works with any torch.distributed backend (RCCL/"nccl" on GPUs, gloo
on CPU for the tests).
"""
import torch
import torch.distributed as dist


def shard_range(n_pairs, world, rank):
    """Contiguous block of pair indices for `rank`: (start, count); the first n_pairs % world
    ranks take one extra pair."""
    if n_pairs < 0 or world <= 0 or not (0 <= rank < world):
        raise ValueError("bad shard arguments")
    q, r = divmod(n_pairs, world)
    count = q + (1 if rank < r else 0)
    start = rank * q + min(rank, r)
    return start, count


def gather_disparities(local, n_pairs, group=None):
    """all_gather the per-rank [count, H, W] maps into [n_pairs, H, W] in pair order (every
    rank gets the result).  Ranks may hold different counts (ragged shards): shards are
    padded to the largest count for the collective and trimmed afterwards."""
    if not (dist.is_available() and dist.is_initialized()):
        return local
    world = dist.get_world_size(group)
    counts = [shard_range(n_pairs, world, r)[1] for r in range(world)]
    cmax = max(counts) if counts else 0
    H, W = local.shape[-2:]
    pad = torch.zeros((cmax, H, W), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    return torch.cat([b[:c] for b, c in zip(bufs, counts)], dim=0)


def checksum(t, group=None):
    """Sum of all disparities over all ranks (float64), the scalar cross-check of the gather."""
    s = t.to(torch.float64).sum().reshape(1)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(s, group=group)
    return float(s.item())


def run_sharded(L_all, R_all, D, compute, group=None):
    """Shard `n_pairs` pairs over the ranks, run `compute(L_shard, R_shard, D)` ->
    (dispL, dispR) on each, gather both maps.  `compute` is the HIP path in production
    (adcensus_batch below); tests substitute a CPU callable to exercise the N>1 plumbing."""
    n = L_all.shape[0]
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    s, c = shard_range(n, world, rank)
    dl, dr = compute(L_all[s:s + c], R_all[s:s + c], D)
    return gather_disparities(dl, n, group), gather_disparities(dr, n, group)


def adcensus_batch(L, R, D, sigmaC=10.0, sigmaS=30.0):
    """The production `compute`: AD-Census both views + WTA for a [count, H, W] shard on this
    rank's GPU through the C ABI."""
    from .api import AD_Census
    c, H, W = L.shape
    dl = torch.empty((c, H, W), dtype=torch.float32, device=L.device)
    dr = torch.empty((c, H, W), dtype=torch.float32, device=L.device)
    if c == 0:
        return dl, dr
    adc = AD_Census().Initialize(L[0], R[0], D, H, W, sigmaC, sigmaS)
    adc.ComputeBatch(L.contiguous(), R.contiguous(), dl, dr)
    adc.status()
    adc.close()
    return dl, dr


def pipeline_batch(L8, R8, D, quirks=0, subpixel=None, scan_views=1, **params):
    """`compute` for run_sharded on configs[2]: the whole main.cpp pipeline (smt_pipeline_run_batch) for a
    [count, H, W] uint8 shard on this rank's GPU -> (LR-checked left maps, right maps).  quirks: QUIRK_FIX_* as
    api.Pipeline (0 = the reference's results).  subpixel: min_den of api.Pipeline.set_subpixel (both maps carry the
    parabola's fraction), None = integer maps.  scan_views: VIEW_LEFT (1) = main.cpp's flow, VIEW_BOTH (3) = the right
    map comes from the scanline-optimised right volume too (api.Pipeline.set_scan_views)."""
    from .api import Pipeline
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    pipe = Pipeline(H, W, D, L8.device, quirks=quirks, subpixel=subpixel, scan_views=scan_views, **params)
    dl, dr, _, _ = pipe.run(L8.contiguous(), R8.contiguous())
    pipe.status()
    pipe.close()
    return dl, dr


def pipeline_refined_batch(L8, R8, D, quirks=0, subpixel=None, scan_views=1, refine=None, post=None, **params):
    """`compute` for run_sharded on the pipeline with its whole tail and the refinement (smt_pipeline_run_batch_refined:
    LR check, RemoveSpeckles, region voting and outlier interpolation, MedianFilter) for a [count, H, W] uint8 shard on
    this rank's GPU -> (lastDisp, the refined left maps before the median).  refine: api.refine_params(...), None = the
    defaults; post: a dict of run_post's keywords; the rest as pipeline_batch."""
    from .api import Pipeline
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    pipe = Pipeline(H, W, D, L8.device, quirks=quirks, subpixel=subpixel, scan_views=scan_views, **params)
    dl, _, _, _, last, _, _ = pipe.run_refined(L8.contiguous(), R8.contiguous(), refine=refine, **(post or {}))
    pipe.status()
    pipe.close()
    return last, dl


def pipeline_filled_batch(L8, R8, D, quirks=0, subpixel=None, scan_views=1, median_wnd=3, invalid=float("inf"), **params):
    """`compute` for run_sharded on the pipeline with Sad.h's FillHolesInDispMap and the median behind the LR check
    (smt_pipeline_run_batch_filled) for a [count, H, W] uint8 shard on this rank's GPU -> (lastDisp, the filled left
    maps before the median).  The rest as pipeline_batch."""
    from .api import Pipeline
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    pipe = Pipeline(H, W, D, L8.device, quirks=quirks, subpixel=subpixel, scan_views=scan_views, **params)
    dl, _, _, _, last, _ = pipe.run_filled(L8.contiguous(), R8.contiguous(), median_wnd=median_wnd, invalid=invalid)
    pipe.status()
    pipe.close()
    return last, dl


def cblsm_batch(L8, R8, D, **params):
    """`compute` for run_sharded on CBLSM.cpp's flow (smt_cblsm_flow_run_batch) for a [count, H, W] uint8 shard on this
    rank's GPU -> (left maps, right maps).  Keywords as api.CBLSMFlow."""
    from .api import CBLSMFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CBLSMFlow(H, W, D, L8.device, **params)
    dl, dr = flow.run(L8.contiguous(), R8.contiguous())
    flow.status()
    flow.close()
    return dl, dr


def cblsm_v4_batch(L8, R8, D, **params):
    """`compute` for run_sharded on the per-hypothesis-arm flow (smt_cblsm_flow_run_batch_v4) for a [count, H, W] uint8
    shard on this rank's GPU -> (left maps, left maps again: the flow has no right view and run_sharded gathers two
    map sets).  Keywords as api.CBLSMFlow."""
    from .api import CBLSMFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CBLSMFlow(H, W, D, L8.device, **params)
    dl = flow.run_v4(L8.contiguous(), R8.contiguous())
    flow.status()
    flow.close()
    return dl, dl


def cblsm_window_batch(L8, R8, D, winSize=1, **params):
    """`compute` for run_sharded on CBLSM.cpp's flow with :132 enabled (smt_cblsm_flow_run_batch_window: window costs in
    place of absolute differences) for a [count, H, W] uint8 shard on this rank's GPU -> (left maps, right maps).
    Keywords as api.CBLSMFlow."""
    from .api import CBLSMFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CBLSMFlow(H, W, D, L8.device, **params)
    dl, dr = flow.run_window(L8.contiguous(), R8.contiguous(), winSize)
    flow.status()
    flow.close()
    return dl, dr


def crossagg_batch(L8, R8, D, **params):
    """`compute` for run_sharded on the CrossAggregator flow of CBLSM.cpp:133-143, 152 (smt_crossagg_flow_run_batch) for
    a [count, H, W, 3] uint8 BGR shard on this rank's GPU -> (left maps, right maps).  Keywords as api.CrossAggFlow."""
    from .api import CrossAggFlow
    c, H, W = L8.shape[:3]
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CrossAggFlow(H, W, D, L8.device, **params)
    dl, dr = flow.run(L8.contiguous(), R8.contiguous())
    flow.close()
    return dl, dr


def cblsm_post_batch(L8, R8, D, post=None, **params):
    """`compute` for run_sharded on CBLSM.cpp's flow with its tail (:160-162, smt_cblsm_flow_run_batch_post) for a
    [count, H, W] uint8 shard on this rank's GPU -> (finished left maps, right maps).  `post`: dict of
    smt_cblsm_post_params overrides; other keywords as api.CBLSMFlow."""
    from .api import CBLSMFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CBLSMFlow(H, W, D, L8.device, **params)
    dl, dr, _, _ = flow.run_post(L8.contiguous(), R8.contiguous(), **(post or {}))
    flow.status()
    flow.close()
    return dl, dr


def crossagg_post_batch(L8, R8, D, post=None, **params):
    """`compute` for run_sharded on the CrossAggregator flow with CBLSM.cpp's tail (smt_crossagg_flow_run_batch_post) for
    a [count, H, W, 3] uint8 BGR shard on this rank's GPU -> (finished left maps, right maps).  `post`: dict of
    smt_cblsm_post_params overrides; other keywords as api.CrossAggFlow."""
    from .api import CrossAggFlow
    c, H, W = L8.shape[:3]
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = CrossAggFlow(H, W, D, L8.device, **params)
    dl, dr, _, _ = flow.run_post(L8.contiguous(), R8.contiguous(), **(post or {}))
    flow.status()
    flow.close()
    return dl, dr


def asw_batch(L8, R8, D, **params):
    """`compute` for run_sharded on ASWeight.cpp's flow (smt_asw_flow_run_batch) for a [count, H, W] uint8 shard on this
    rank's GPU -> (left maps, right maps).  Keywords as api.ASWFlow."""
    from .api import ASWFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = ASWFlow(H, W, D, L8.device, **params)
    dl, dr, _ = flow.run(L8.contiguous(), R8.contiguous())
    flow.close()
    return dl, dr


def asw_post_batch(L8, R8, D, post=None, **params):
    """`compute` for run_sharded on ASWeight.cpp's flow with its tail (smt_asw_flow_run_batch_post) for a [count, H, W]
    uint8 shard on this rank's GPU -> (finished lastDisp maps, normalised left maps), uint8.  `post`: dict of
    smt_asw_post_params overrides; other keywords as api.ASWFlow."""
    from .api import ASWFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.uint8, device=L8.device)
        return z, z.clone()
    flow = ASWFlow(H, W, D, L8.device, **params)
    r = flow.run_post(L8.contiguous(), R8.contiguous(), **(post or {}))
    flow.status()
    flow.close()
    return r["lastDisp"], r["dispL8"]


def sad_batch(L8, R8, D, **params):
    """`compute` for run_sharded on SADmain.cpp's flow (smt_sad_flow_run_batch) for a [count, H, W] uint8 shard on this
    rank's GPU -> (left maps, right maps), int32.  Keywords as api.SADFlow."""
    from .api import SADFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.int32, device=L8.device)
        return z, z.clone()
    flow = SADFlow(H, W, D, L8.device, **params)
    dl, dr, _, _ = flow.run(L8.contiguous(), R8.contiguous())
    flow.close()
    return dl, dr


def sad_subpixel_batch(L8, R8, D, min_den=1.0, **params):
    """sad_batch with the parabola of Sad.h:76-81 kept (smt_sad_flow_run_batch_subpixel) -> (left maps, right maps),
    float32.  Keywords as api.SADFlow."""
    from .api import SADFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.float32, device=L8.device)
        return z, z.clone()
    flow = SADFlow(H, W, D, L8.device, **params)
    dl, dr, _, _ = flow.run_subpixel(L8.contiguous(), R8.contiguous(), min_den)
    flow.close()
    return dl, dr


def ncc_batch(L8, R8, D, **params):
    """`compute` for run_sharded on NCC_main.cpp's flow (smt_ncc_flow_run_batch) for a [count, H, W] uint8 shard on this
    rank's GPU -> (left maps, left maps again: NCC has no right view and run_sharded gathers two map sets), int32.
    Keywords as api.NCCFlow."""
    from .api import NCCFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.int32, device=L8.device)
        return z, z.clone()
    flow = NCCFlow(H, W, D, L8.device, **params)
    dl = flow.run(L8.contiguous(), R8.contiguous())
    flow.close()
    return dl, dl


def ncc_both_batch(L8, R8, D, **params):
    """`compute` for run_sharded on both NCC views (smt_lrncc_flow_run_batch) for a [count, H, W] uint8 shard on this
    rank's GPU -> (left maps, right maps), int32.  Keywords as api.NCCFlow."""
    from .api import NCCFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.int32, device=L8.device)
        return z, z.clone()
    flow = NCCFlow(H, W, D, L8.device, **params)
    dl, dr, _, _ = flow.run_both(L8.contiguous(), R8.contiguous(), want=("dispL", "dispR"))
    flow.close()
    return dl, dr


def ncc_whole_batch(L8, R8, D=None, **params):
    """`compute` for run_sharded on NCC.h's whole-image ncc(), both types (smt_whole_ncc_flow_run_batch), for a
    [count, H, W] uint8 shard on this rank's GPU -> (left offset maps, right offset maps), int32.  D, when given, is
    max_offset; keywords as api.NCCWholeFlow."""
    from .api import NCCWholeFlow
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.int32, device=L8.device)
        return z, z.clone()
    if D is not None:
        params = dict(params, max_offset=D)
    flow = NCCWholeFlow(H, W, L8.device, **params)
    _, _, ol, orr, _, _ = flow.run(L8.contiguous(), R8.contiguous(), want=("offL", "offR"))
    flow.close()
    return ol, orr


def bilateral_batch(L8, R8, D=None, **params):
    """`compute` for run_sharded on the bilateral image filter of BiliteralFilter.h:49-142 (smt_bilateral_filter_batch)
    for a [count, H, W] uint8 shard of gray pairs on this rank's GPU -> (filtered left images, filtered right images),
    uint8, both images of every pair in one call.  D is not used (an image-domain stage has no disparity range).
    Keywords as api.bilateralfiter (wsize, spaceSigma, colorSigma, norm).  Colour stacks are not sharded: run_sharded
    gathers [n, H, W] maps; filter [n, H, W, 3] stacks with api.bilateralfiter on the rank that holds them."""
    from .api import bilateralfiter
    c, H, W = L8.shape
    if c == 0:
        z = torch.empty((0, H, W), dtype=torch.uint8, device=L8.device)
        return z, z.clone()
    out = bilateralfiter(torch.cat([L8, R8], dim=0).contiguous().unsqueeze(-1), **params).squeeze(-1)
    return out[:c], out[c:]
