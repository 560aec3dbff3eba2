"""smt_adcensus_compute_batch with the maps-only kernel for pairs 0 .. n-2 (adcensus_kernels.h, k_cost_maps2p): every map
against the oracle, the last pair's volumes bit for bit, the domain flag of a non-last pair, and the same maps with
SMT_BATCH_VOLUMES=all -- under every batch schedule and for both / one / no map requested."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(20, 130, 100, 4), (24, 200, 64, 9), (18, 100, 192, 3), (9, 70, 256, 2), (40, 64, 192, 5)]
SCHEDS = ["0", "1", "2", None]
MAPS = ["both", "left", "right", "none"]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _batch(adc, Lb, Rb, maps, dev):
    from stereo_match_traditional_amd._lib import lib, VIEW_BOTH
    B, H, W = Lb.shape
    dl = torch.full((B, H, W), -1.0, device=dev) if maps in ("both", "left") else None
    dr = torch.full((B, H, W), -1.0, device=dev) if maps in ("both", "right") else None
    adc._bind_stream()
    rc = lib().smt_adcensus_compute_batch(adc._h, _p(Lb), _p(Rb), B, VIEW_BOTH, _p(dl), _p(dr))
    assert rc == 0
    return dl, dr


@pytest.mark.parametrize("H,W,D,B", SHAPES)
def test_maps_only_batch(smt, O, H, W, D, B, monkeypatch):
    dev = torch.device("cuda:0")
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 900 + b, noise=(b % 2 == 0)) for b in range(B)])
    Lb = torch.from_numpy(np.stack(Ls).astype(np.float32)).to(dev)
    Rb = torch.from_numpy(np.stack(Rs).astype(np.float32)).to(dev)
    refs = [(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0), O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1))
            for b in range(B)]
    maps = [(O.wta(a), O.wta(c)) for a, c in refs]
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    monkeypatch.delenv("SMT_BATCH_VOLUMES", raising=False)
    for sched in SCHEDS:
        if sched is None: monkeypatch.delenv("SMT_OVERLAP", raising=False)
        else: monkeypatch.setenv("SMT_OVERLAP", sched)
        for m in MAPS:
            dl, dr = _batch(adc, Lb, Rb, m, dev)
            adc.status()
            for b in range(B):
                if dl is not None: assert np.array_equal(dl[b].cpu().numpy(), maps[b][0]), (sched, m, b)
                if dr is not None: assert np.array_equal(dr[b].cpu().numpy(), maps[b][1]), (sched, m, b)
            # the last pair always writes both volumes, whatever maps were asked for
            assert np.array_equal(adc.GetPtrLeft().cpu().numpy().view(np.uint32), refs[-1][0].view(np.uint32)), (sched, m)
            assert np.array_equal(adc.GetPtrRight().cpu().numpy().view(np.uint32), refs[-1][1].view(np.uint32)), (sched, m)
        # every pair's volumes written: the same maps
        monkeypatch.setenv("SMT_BATCH_VOLUMES", "all")
        dl2, dr2 = _batch(adc, Lb, Rb, "both", dev)
        adc.status()
        monkeypatch.delenv("SMT_BATCH_VOLUMES")
        dl, dr = _batch(adc, Lb, Rb, "both", dev)
        adc.status()
        assert torch.equal(dl, dl2) and torch.equal(dr, dr2), sched
    adc.close()


@pytest.mark.parametrize("knob", [("SMT_MAPS_CHUNKS", "1"), ("SMT_MAPS_CHUNKS", "3"), ("SMT_MAPS_CHUNKS", "64"),
                                  ("SMT_MAPS_KERNEL", "rank")])
def test_maps_only_tuning_hooks(smt, O, knob, monkeypatch):
    """Chunks per workgroup and the rank-key form of the maps-only kernel give the same maps."""
    H, W, D, B = 37, 150, 192, 3
    dev = torch.device("cuda:0")
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 950 + b, noise=True) for b in range(B)])
    Lb = torch.from_numpy(np.stack(Ls).astype(np.float32)).to(dev)
    Rb = torch.from_numpy(np.stack(Rs).astype(np.float32)).to(dev)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    monkeypatch.setenv(*knob)
    for sched in ("2", "0"):
        monkeypatch.setenv("SMT_OVERLAP", sched)
        dl, dr = _batch(adc, Lb, Rb, "both", dev)
        adc.status()
        for b in range(B):
            assert np.array_equal(dl[b].cpu().numpy(), O.wta(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 0))), (sched, b)
            assert np.array_equal(dr[b].cpu().numpy(), O.wta(O.adcensus_view(Ls[b], Rs[b], D, 10.0, 30.0, 1))), (sched, b)
    adc.close()


@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("m", MAPS)
def test_domain_flag_of_a_non_last_pair(smt, O, sched, m, monkeypatch):
    """A bad pixel in pair 0 of a batch raises SMT_ERR_DOMAIN at the next status, with or without maps."""
    from stereo_match_traditional_amd import SmtError
    H, W, D, B = 16, 96, 64, 3
    dev = torch.device("cuda:0")
    Ls, Rs = zip(*[O.synth_pair(H, W, D, 970 + b) for b in range(B)])
    Lb = torch.from_numpy(np.stack(Ls).astype(np.float32)).to(dev)
    Rb = torch.from_numpy(np.stack(Rs).astype(np.float32)).to(dev)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    if sched is None: monkeypatch.delenv("SMT_OVERLAP", raising=False)
    else: monkeypatch.setenv("SMT_OVERLAP", sched)
    _batch(adc, Lb, Rb, m, dev)
    adc.status()                                        # clean batch: no flag
    bad = Lb.clone()
    bad[0, 5, 7] = 3.5
    _batch(adc, bad, Rb, m, dev)
    with pytest.raises(SmtError):
        adc.status()
    adc.status()                                        # read-and-clear
    adc.close()
