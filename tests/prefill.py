"""Shared by tests/test_fuzz_flows_gpu.py and tests/test_consistency_hostile_gpu.py: the `flows` fixture, under which the
tensors that stereo_match_traditional_amd.api allocates for its outputs come prefilled, so that an element an entry
point does not write cannot pass a comparison, and first_diff, which words a mismatch.  A plain helper module, not a conftest."""
import numpy as np
import pytest
import torch

INT_SENTINEL = -77777777
U8_SENTINEL = 0xEE


def _poison(t):
    if t.numel():
        t.fill_(float("nan") if t.is_floating_point() else U8_SENTINEL if t.dtype == torch.uint8 else INT_SENTINEL)
    return t


class _PrefillingTorch:
    """`torch` as stereo_match_traditional_amd.api sees it during these tests: empty / empty_like hand out tensors
    prefilled with NaN (float) or a sentinel (int), everything else is torch's own."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *a, **kw):
        return _poison(self._real.empty(*a, **kw))

    def empty_like(self, *a, **kw):
        return _poison(self._real.empty_like(*a, **kw))


@pytest.fixture
def flows(smt, monkeypatch):
    from stereo_match_traditional_amd import api
    monkeypatch.setattr(api, "torch", _PrefillingTorch(torch))
    probe = api.torch.empty((3,), dtype=torch.float32, device=torch.device("cuda:0"))
    assert bool(torch.isnan(probe).all())
    return smt


def first_diff(got, want, limit=5):
    """'n differ, first at (index): got x, want y; ...' for a mismatch message; compares bytes"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    w = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.argwhere(got.view(w) != want.view(w))
    return f"{len(bad)} of {got.size} differ; " + "; ".join(
        f"{tuple(int(x) for x in ix)}: got {got[tuple(ix)]!r}, want {want[tuple(ix)]!r}" for ix in bad[:limit])
