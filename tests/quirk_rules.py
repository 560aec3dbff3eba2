"""Shared by test_quirks_cpu.py and test_quirks_gpu.py: the SMT_QUIRK_* constants, a numpy restatement of the arm rule
written from SURVEY.md Appendix A.4 and parameterised by the flags, and the fixed inputs of the arm tests.

The restatement is anchored in test_quirks_cpu.py: with flags 0 it equals the oracle's arm maps bit for bit on the
images below, and on the same images the fixed maps differ from the faithful ones in every direction, so a test that
holds the kernels to the fixed branch cannot pass where the flag is a no-op."""
import numpy as np

FIX_RIGHT_ARM_STRIDE = 0x1
FIX_STICKY_TAU = 0x2
FIX_SCAN_VERTICAL = 0x4
FIX_CENSUS_RIGHT_EDGE = 0x8
FIX_ALL = 0xF


def _diff(img, a, b):
    """|I(a) - I(b)|, the largest over the channels for a 3-channel image (CrossArm.cpp's Vec3b branch)."""
    return int(np.abs(img[a].astype(np.int32) - img[b].astype(np.int32)).max())


def arm_dir(img, dirn, tau_in, tau, tau_low, sec, maxlen, quirks):
    """One Compute*ArmLength call (A.4), dirn 0 left, 1 right, 2 top, 3 bottom -> ([H][W] int32 map, threshold afterwards).

    Faithful: one threshold, entered as `tau_in`, lowered to tau_low on entering iteration sec + 1 and never raised.
    FIX_STICKY_TAU: the threshold belongs to the walk -- every walk starts at `tau`; the state is left alone.
    Without FIX_RIGHT_ARM_STRIDE the right-arm call runs over j < H, tests j + k < H and stores with stride H."""
    H, W = img.shape[:2]
    px = img.reshape(H * W, -1)
    colR = H if (dirn == 1 and not (quirks & FIX_RIGHT_ARM_STRIDE)) else W
    out = np.zeros(H * W, np.int32)
    local = bool(quirks & FIX_STICKY_TAU)
    state = tau_in
    for i in range(H):
        for j in range(colR):
            t = tau if local else state
            saved, k = 0, 0
            while True:
                saved = k
                k += 1
                if k > sec:                                   # (1) the flip precedes the bounds test
                    t = tau_low
                    if k > maxlen:                            # (2)
                        break
                ni, nj = i, j
                if dirn == 0:
                    nj, inside, far = j - k, j - k >= 0, j - 1 >= 1
                elif dirn == 1:
                    nj, inside, far = j + k, j + k < colR, j + 1 < colR - 1
                elif dirn == 2:
                    ni, inside, far = i - k, i - k >= 0, i - 1 >= 1
                else:
                    ni, inside, far = i + k, i + k < H, i + 1 < H - 1
                if not inside:                                # (3)
                    break
                if _diff(px, i * W + j, ni * W + nj) > t:     # (4), with the forced minimum of 1
                    if far and saved < 1:
                        saved = 1
                    break
            if not local:
                state = t
            out[i * colR + j] = saved
    return out.reshape(H, W), state


def arms(img, tau=30, tau_low=6, sec=17, maxlen=34, chain=1, quirks=0):
    """Initialize + the four calls in main.cpp's order -> [left, right, top, bottom].  chain = 0: every call is entered
    with `tau` (CBLSM's by-value threshold)."""
    maps, state = [], tau
    for dirn in range(4):
        m, state = arm_dir(img, dirn, state, tau, tau_low, sec, maxlen, quirks)
        if not chain:
            state = tau
        maps.append(m)
    return maps


def _with_channels(gray, ch, seed):
    if ch == 1:
        return gray
    rs = np.random.RandomState(seed)
    bgr = gray[:, :, None].astype(np.int32) + rs.randint(-2, 3, gray.shape + (3,))
    return np.clip(bgr, 0, 255).astype(np.uint8)


def arm_image_ramp(ch=1):
    """40 x 48, default parameters (sec 17, max 34): a ramp of 1 grey level per pixel in both axes, so that every
    direction has walks that pass 17 neighbours under tau = 30 (the flip) and later pixels whose neighbours differ by
    7 .. 17 (which tau_low = 6 cuts short); rows 16 .. 23 carry noise that stops arms at every length."""
    H, W = 40, 48
    i, j = np.mgrid[0:H, 0:W]
    g = 60 + i + j
    rs = np.random.RandomState(7)
    g[16:24] += rs.randint(-45, 46, (8, W))
    return _with_channels(np.clip(g, 0, 255).astype(np.uint8), ch, 11)


def arm_image_small(ch=1):
    """8 x 9 for sec_length = 3, max_length = 6: 8 grey levels per pixel in both axes -- three neighbours pass under 30,
    the first fails under 6 -- and two outliers."""
    H, W = 8, 9
    i, j = np.mgrid[0:H, 0:W]
    g = 20 + 8 * i + 8 * j
    g[2, 5] = 250
    g[6, 1] = 0
    return _with_channels(np.clip(g, 0, 255).astype(np.uint8), ch, 13)


# (name, image builder, keyword arguments of arms() and of CrossArmAggregation.Initialize)
ARM_CASES = [
    ("ramp40x48", arm_image_ramp, dict(tau=30, tau_low=6, sec=17, maxlen=34)),
    ("small8x9", arm_image_small, dict(tau=30, tau_low=6, sec=3, maxlen=6)),
]
