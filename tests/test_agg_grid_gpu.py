"""Aggregation placement hooks and long-arm rectangles, bit for bit against the oracle (O.aggregate_rect + O.wta) with the
fused disparity map on.  Before every launch the two outputs are filled with 0xFF bytes -- a NaN, which no mean of
non-negative finite values is -- so a pixel that no workgroup wrote fails the comparison instead of keeping the value an
earlier launch left there.  Arms are loaded with load_arm_maps and clamped to the plane (agg_grid_cases.py, whose
conditions test_agg_grid_cpu.py checks): any shape is legal and ca.status() must stay clean."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_grid_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (0, 1)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """One (arms, volume, order): the handle with the arms loaded, the input and the oracle's outputs on the device."""

    def __init__(self, smt, O, arms, vol, order):
        H, W, D = vol.shape
        ref, oob = O.aggregate_rect(vol, arms, order)
        assert oob == 0
        self.order, self.vol = order, T(vol)
        self.ref = T(ref).view(torch.int32)
        self.ref_disp = T(O.wta(ref)).view(torch.int32)
        self.out = torch.empty((H, W, D), device=DEV)
        self.disp = torch.empty((H, W), device=DEV)
        self.ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, DEV)
        self.ca.load_arm_maps(*[T(a) for a in arms])
        self.ca.status()

    def launch(self):
        """One aggregation into sentinel-filled outputs; '' when every bit is the oracle's, else what differs."""
        self.out.view(torch.int32).fill_(-1)
        self.disp.view(torch.int32).fill_(-1)
        fn = self.ca.AggregationVertical if self.order == 0 else self.ca.costAggregationV5
        fn(self.vol, self.out, self.disp)
        self.ca.status()
        o, d = self.out.view(torch.int32), self.disp.view(torch.int32)
        if torch.equal(o, self.ref) and torch.equal(d, self.ref_disp):
            return ""
        unwritten = int((o == -1).all(dim=2).sum())
        return "%d pixels differ (%d never written), %d disparities differ" % (
            int((o != self.ref).any(dim=2).sum()), unwritten, int((d != self.ref_disp).sum()))

    def close(self):
        self.ca.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", G.PLACEMENT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_placement_hooks_reach_every_pixel_once(smt, O, case, order):
    """Every variant at its default strip width, then every variant x requested width x sweep (about 240 tiny launches):
    the hooks change which workgroup owns a pixel, never a bit of the result."""
    H, W, D, max_arm = case
    c = Case(smt, O, G.random_arms(H, W, max_arm, 100 + max_arm), G.ordinary_volume(H, W, D, 7), order)
    bad = []
    for v in G.VARIANTS:                                   # a fresh handle: set_variant's own widths
        c.ca.set_variant(v)
        msg = c.launch()
        if msg:
            bad.append((v, "default", 0, msg))
    for v in G.VARIANTS:                                   # variant 10 runs as 12 where D % 64 != 0
        c.ca.set_variant(v)
        for w in G.PLACEMENT_WIDTHS:
            c.ca.set_strip_width(w)
            for sweep in G.SWEEPS:                         # variants 0 .. 2 ignore it
                c.ca.set_sweep(sweep)
                msg = c.launch()
                if msg:
                    bad.append((v, w, sweep, msg))
    c.close()
    assert not bad, (len(bad), bad[:10])


def test_strip_width_bound(smt):
    from stereo_match_traditional_amd import SmtError
    ca = smt.CrossArmAggregation().Initialize(4, 4, 30, 4, DEV)
    ca.set_strip_width(G.MAX_STRIP_WIDTH)
    for w in (G.MAX_STRIP_WIDTH + 4, 1 << 20, 0, 2, 6, -4):
        with pytest.raises(SmtError) as e:
            ca.set_strip_width(w)
        assert e.value.status == -1, w
    ca.close()


@pytest.mark.parametrize("order", ORDERS)
def test_occupancy_claim_changes_no_bit(smt, O, order):
    """set_occupancy limits the waves per SIMD through an LDS claim the kernel never touches."""
    from stereo_match_traditional_amd import SmtError
    H, W, D = G.OCCUPANCY_SHAPE
    c = Case(smt, O, G.random_arms(H, W, 6, 106), G.ordinary_volume(H, W, D, 7), order)
    bad = []
    for v in G.OCCUPANCY_VARIANTS:
        c.ca.set_variant(v)
        for waves in G.OCCUPANCY_VALUES:
            c.ca.set_occupancy(waves)
            msg = c.launch()
            if msg:
                bad.append((v, waves, msg))
    for waves in G.OCCUPANCY_BAD:
        with pytest.raises(SmtError) as e:
            c.ca.set_occupancy(waves)
        assert e.value.status == -1, waves
    c.close()
    assert not bad, bad


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import agg_grid_cases as G
import stereo_match_traditional_amd as smt
from oracle import oracle as O
H, W, D = G.OCCUPANCY_SHAPE
dev = torch.device("cuda:0")
arms, vol = G.random_arms(H, W, 6, 106), G.ordinary_volume(H, W, D, 7)
ref, oob = O.aggregate_rect(vol, arms, 0)
ca = smt.CrossArmAggregation().Initialize(H, W, 30, D, dev)
ca.load_arm_maps(*[torch.from_numpy(a).to(dev) for a in arms])
out = torch.empty((H, W, D), device=dev); disp = torch.empty((H, W), device=dev)
out.view(torch.int32).fill_(-1); disp.view(torch.int32).fill_(-1)
ca.AggregationVertical(torch.from_numpy(vol).to(dev), out, disp)
ca.status()
ok = oob == 0 and np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and \
    np.array_equal(disp.cpu().numpy(), O.wta(ref))
print("AGG_WAVES_CHILD", "ok" if ok else "MISMATCH")
"""


@pytest.mark.parametrize("value", ["3", "9", "many"])
def test_agg_waves_environment(value, tmp_path):
    """SMT_AGG_WAVES is read once per process: 3 claims LDS for every handle, 9 or a non-number behaves as unset.  One
    aggregation in a fresh process gives the oracle's bits either way."""
    script = tmp_path / "agg_waves_child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, SMT_AGG_WAVES=value)
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "AGG_WAVES_CHILD ok" in r.stdout, r.stdout[-2000:]


# ---- long arms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["ordinary", "spread"])
@pytest.mark.parametrize("D", G.LONG_A_D)
def test_long_arms_around_the_quotient_boundary(smt, O, D, kind, order):
    """Rectangles of 255 x 257 = 65535 (the last divisor of variant 13's fast quotient), 256 x 256 = 65536 (the first on
    the division path), 257 x 257 and an off-centre 262 x 254 among arms <= 6, every variant.  The ordinary volume keeps
    the sums inside the fast quotient's range, the spread one (exponents -75 .. 75) sends every pixel to the division."""
    H, W = G.LONG_A_HW
    vol = G.ordinary_volume(H, W, D, 5) if kind == "ordinary" else G.spread_volume(H, W, D, 6)
    c = Case(smt, O, G.long_a_arms(), vol, order)
    bad = []
    for v in G.VARIANTS:
        c.ca.set_variant(v)
        msg = c.launch()
        if msg:
            bad.append((v, msg))
    c.close()
    assert not bad, bad


@pytest.fixture(scope="module")
def long_b(smt, O):
    """Case B's inputs and the oracle's outputs for both orders, computed once."""
    H, W, D = G.LONG_B_HWD
    arms, vol = G.long_b_arms(), G.ordinary_volume(H, W, D, 9)
    return {order: Case(smt, O, arms, vol, order) for order in ORDERS}


@pytest.mark.parametrize("variant", G.LONG_B_VARIANTS)
@pytest.mark.parametrize("order", ORDERS)
def test_long_arms_box_beyond_2_pow_24(long_b, order, variant):
    """One pixel with arms of 2048 on all four sides in a 4100 x 4104 plane: 4097^2 > 2^24 box positions, the smallest box
    at which (float)n of the kernels' index split is inexact.  The time of each launch is printed."""
    c = long_b[order]
    c.ca.set_variant(variant)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    msg = c.launch()
    dt = time.perf_counter() - t0
    print("long-arm case B: variant %d order %d: %.3f s (launch + compare)" % (variant, order, dt))
    assert not msg, msg
