"""SMT_QUIRK_* without a GPU: the arm restatement of quirk_rules.py is anchored to the oracle with flags 0, the arm test
inputs are shown to bite (faithful and fixed maps differ in every direction), and the header and the library carry the
new flags and entry points."""
import os
import re

import numpy as np
import pytest

import quirk_rules as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, ch, chain) for name, _, _ in Q.ARM_CASES for ch in (1, 3) for chain in (1, 0)]


def _case(name):
    return next(c for c in Q.ARM_CASES if c[0] == name)


@pytest.fixture(scope="module")
def arm_maps():
    """{(name, ch, chain, quirks): four maps} of the restatement, computed once."""
    out = {}
    for name, ch, chain in CASES:
        _, build, kw = _case(name)
        img = build(ch)
        for q in (0, Q.FIX_STICKY_TAU, Q.FIX_RIGHT_ARM_STRIDE, Q.FIX_RIGHT_ARM_STRIDE | Q.FIX_STICKY_TAU):
            out[(name, ch, chain, q)] = Q.arms(img, chain=chain, quirks=q, **kw)
    return out


@pytest.mark.parametrize("name,ch,chain", CASES)
def test_arm_restatement_equals_oracle_with_flags_0(O, arm_maps, name, ch, chain):
    _, build, kw = _case(name)
    img = build(ch)
    for bug, q in ((True, 0), (False, Q.FIX_RIGHT_ARM_STRIDE)):
        ref = O.arms_all(img, kw["tau"], kw["tau_low"], kw["sec"], kw["maxlen"], chain=bool(chain), right_row_bug=bug)
        for d in range(4):
            assert np.array_equal(arm_maps[(name, ch, chain, q)][d], ref[d]), (name, ch, chain, bug, d)


@pytest.mark.parametrize("name,ch,chain", CASES)
def test_arm_inputs_bite(arm_maps, name, ch, chain):
    """every direction: a flip, and a later pixel that the lowered threshold shortens"""
    for stride in (0, Q.FIX_RIGHT_ARM_STRIDE):
        faithful, fixed = arm_maps[(name, ch, chain, stride)], arm_maps[(name, ch, chain, stride | Q.FIX_STICKY_TAU)]
        for d in range(4):
            n = int((faithful[d] != fixed[d]).sum())
            assert n > 0, (name, ch, chain, stride, d)
            assert (fixed[d] >= faithful[d]).all(), (name, ch, chain, stride, d)   # a higher threshold never stops earlier


def test_fixed_top_arms_are_left_arms_of_the_transpose():
    """the identity the GPU test holds the kernels to, on the restatement"""
    for name, build, kw in Q.ARM_CASES:
        img = build(1)
        a = Q.arms(img, quirks=Q.FIX_ALL, **kw)
        b = Q.arms(np.ascontiguousarray(img.T), quirks=Q.FIX_ALL, **kw)
        assert np.array_equal(a[2], b[0].T) and np.array_equal(a[3], b[1].T), name


def test_header_and_exports():
    """fails without the feature"""
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    for flag, val in (("SMT_QUIRK_FIX_RIGHT_ARM_STRIDE", 1), ("SMT_QUIRK_FIX_STICKY_TAU", 2),
                      ("SMT_QUIRK_FIX_SCAN_VERTICAL", 4), ("SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE", 8)):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+)u" % flag, hdr)
        assert m and int(m.group(1), 16) == val, flag
    m = re.search(r"#define\s+SMT_QUIRK_FIX_ALL\s+\(([^)]*)\)", hdr)
    assert m, "SMT_QUIRK_FIX_ALL"
    assert sorted(re.findall(r"SMT_QUIRK_\w+", m.group(1))) == sorted(
        ["SMT_QUIRK_FIX_RIGHT_ARM_STRIDE", "SMT_QUIRK_FIX_STICKY_TAU", "SMT_QUIRK_FIX_SCAN_VERTICAL",
         "SMT_QUIRK_FIX_CENSUS_RIGHT_EDGE"])
    entries = ["smt_scanline_set_quirks", "smt_adcensus_set_quirks", "smt_pipeline_set_quirks"]
    for e in entries:
        assert re.search(r"int\s+%s\s*\(\s*smt_\w+\s*\*\s*h\s*,\s*unsigned\s+quirks\s*\)\s*;" % e, hdr), e
    from stereo_match_traditional_amd import _lib
    so = _lib.lib()                                    # loads without a GPU; a missing library raises
    for e in entries:
        assert hasattr(so, e), e                       # ctypes resolves the symbol in libsmt_hip.so or raises AttributeError
    assert (_lib.QUIRK_FIX_RIGHT_ARM_STRIDE, _lib.QUIRK_FIX_STICKY_TAU, _lib.QUIRK_FIX_SCAN_VERTICAL,
            _lib.QUIRK_FIX_CENSUS_RIGHT_EDGE, _lib.QUIRK_FIX_ALL) == (1, 2, 4, 8, 15)
    assert (Q.FIX_RIGHT_ARM_STRIDE, Q.FIX_STICKY_TAU, Q.FIX_SCAN_VERTICAL, Q.FIX_CENSUS_RIGHT_EDGE, Q.FIX_ALL) == (1, 2, 4, 8, 15)
