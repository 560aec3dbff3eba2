"""Shared by test_cblsm_v4_cpu.py and test_cblsm_v4_gpu.py: costAggregationV4 (CBLSM.h:1128-1176) and ComputeDispOringin
(:383-407) restated in NumPy, input builders, and the comparison the tests use (bit for bit where finite, by position
where NaN)."""
import numpy as np

CBLSM_ARMS = dict(tau_low=6, chain=False, right_row_bug=False)     # smt_crossarm_cblsm_params, as CBLSM.cpp runs them


def v4_numpy(vol, aL, aR, aUp, aDown):
    """:1160-1172 for every (i, j, d): rows top in [-up, down) outer, columns left in [-L, R) inner, one np.float32 add
    per tap in that order, then value / number with number the int tap count (0.0f / 0 = NaN).  Taps must lie inside
    the plane."""
    H, W, D = vol.shape
    vol = np.asarray(vol, np.float32)
    out = np.empty((H, W, D), np.float32)
    for i in range(H):
        for j in range(W):
            for d in range(D):
                L, R, up, down = int(aL[i, j, d]), int(aR[i, j, d]), int(aUp[i, j, d]), int(aDown[i, j, d])
                value = np.float32(0)
                number = 0
                for top in range(-up, down):
                    assert 0 <= i + top < H
                    for left in range(-L, R):
                        assert 0 <= j + left < W
                        value = np.float32(value + vol[i + top, j + left, d])
                        number += 1
                out[i, j, d] = value / np.float32(number) if number else np.float32(np.nan)
    return out


def disp_origin(vol):
    """:392-404: minCost = cost[0]; a later d wins on `cost < minCost` only (a NaN never does; a NaN at 0 stays)."""
    vol = np.asarray(vol, np.float32)
    mincost = vol[..., 0].copy()
    best = np.zeros(vol.shape[:2], np.float32)
    with np.errstate(invalid="ignore"):
        for d in range(vol.shape[2]):
            m = vol[..., d] < mincost
            mincost[m] = vol[..., d][m]
            best[m] = d
    return best


def same_volume(got, ref):
    """bit-equal where finite, NaN where NaN (sign and payload of a NaN are not compared)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ng, nr = np.isnan(got), np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(ng, nr) and \
        np.array_equal(got[~ng].view(np.uint32), ref[~nr].view(np.uint32))


def random_arm_volumes(H, W, D, seed, max_arm=4):
    """Four int32 [H][W][D] volumes whose half-open rectangles stay inside the plane; about a quarter of the entries are
    0, so that empty rectangles (NaN) occur."""
    rng = np.random.default_rng(seed)
    i = np.arange(H)[:, None, None]
    j = np.arange(W)[None, :, None]
    lim = [np.broadcast_to(x, (H, W, D)) for x in (j, W - j, i, H - i)]           # L, R, up, down
    vols = []
    for m in lim:
        a = rng.integers(0, max_arm + 1, (H, W, D)) * (rng.integers(0, 4, (H, W, D)) != 0)
        vols.append(np.minimum(a, m).astype(np.int32))
    return vols


def oracle_arm_volumes(O, L, R, D, tau=25, sec=17, maxlen=34):
    """CBLSM.cpp:64-67, 101-104, 108-111 from the oracle -> (ArmVolumL, ArmVolumR, ArmVolumUp, ArmVolumDown)."""
    aL = O.arms_all(L, tau0=tau, sec=sec, maxlen=maxlen, **CBLSM_ARMS)           # LL, LR, Lup, Ldown
    aR = O.arms_all(R, tau0=tau, sec=sec, maxlen=maxlen, **CBLSM_ARMS)           # RL, RR, Rup, Rdown
    return (O.choose_arm_length(0, aL[0], None, aR[0], aR[1], D), O.choose_arm_length(1, aL[1], None, aR[0], aR[1], D),
            O.choose_arm_length(2, aL[2], aR[2], aR[0], aR[1], D), O.choose_arm_length(3, aL[3], aR[3], aR[0], aR[1], D))


def noisy_pair(H, W, seed, levels=3, step=20):
    """A pair with few, well separated gray levels: arms of every length from 0 up, differing between the images."""
    rng = np.random.default_rng(seed)
    L = (rng.integers(0, levels, (H, W)) * step + rng.integers(0, 4, (H, W))).astype(np.uint8)
    R = np.roll(L, -2, axis=1)
    flip = rng.integers(0, 5, (H, W)) == 0
    R[flip] = (rng.integers(0, levels, (H, W)) * step).astype(np.uint8)[flip]
    return L, np.ascontiguousarray(R)
