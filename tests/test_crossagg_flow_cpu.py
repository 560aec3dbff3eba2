"""The fused first pass of smt_crossagg_flow_run_batch replaces the AD volume and the first horizontal aggregation pass
by integer prefix differences (csrc/crossagg_first.h).  The library restates that form on the host through the same
inline arithmetic the kernel runs (smt_crossagg_selftest_first_pass) and compares it, bit for bit, with sequential
float sums over the chained ComputeAD / ComputeADRight volumes.  Plus the flow's defaults and the argument errors that
need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMT_ERR_ARG = -1


def _lib():
    from stereo_match_traditional_amd import build
    return ctypes.CDLL(build.build())


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("H,W,D,max_arm", [(3, 70, 16, 34), (2, 40, 64, 255), (1, 5, 9, 3), (4, 33, 300, 17), (2, 1, 4, 0)])
def test_first_pass_integer_form_equals_sequential_float_sums(H, W, D, max_arm, fill):
    """Arms at the default limit, at the uint8 limit (rows shorter than the arms), W < D with the whole chain, D > 256,
    one column with no arm; random bytes and left 255 / right 0 (every cost 255: the largest sums); three seeds."""
    f = _lib().smt_crossagg_selftest_first_pass
    for seed in (1, 77, 2024):
        assert f(H, W, D, max_arm, fill, seed) == 0, seed


def test_first_pass_longest_sum():
    """511 taps of 255 = 130 305: past 2^16, where one uint16 prefix difference would wrap; the two-half form holds."""
    assert _lib().smt_crossagg_selftest_first_pass(1, 600, 2, 255, 1, 3) == 0


def test_selftest_rejects_bad_sizes():
    f = _lib().smt_crossagg_selftest_first_pass
    assert f(0, 4, 1, 1, 0, 0) == SMT_ERR_ARG
    assert f(4, 0, 1, 1, 0, 0) == SMT_ERR_ARG
    assert f(4, 4, 0, 1, 0, 0) == SMT_ERR_ARG
    assert f(4, 4, 1, -1, 0, 0) == SMT_ERR_ARG
    assert f(4, 4, 1, 256, 0, 0) == SMT_ERR_ARG
    assert f(1 << 10, 1 << 10, 17, 1, 0, 0) == SMT_ERR_ARG            # more than 2^24 hypotheses


def test_default_params():
    from stereo_match_traditional_amd import _lib as L
    p = L.CrossAggFlowParams()
    _lib().smt_crossagg_flow_default_params(ctypes.byref(p))
    assert (p.L1, p.L2, p.t1, p.t2, p.num_iters, p.gate) == (34, 17, 20, 6, 4, 5)
    _lib().smt_crossagg_flow_default_params(None)                     # a no-op


def test_argument_errors_that_need_no_device():
    from stereo_match_traditional_amd import _lib as L
    lib = _lib()
    h = ctypes.c_void_p()

    def create(H, W, D, **kw):
        p = L.CrossAggFlowParams()
        lib.smt_crossagg_flow_default_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.smt_crossagg_flow_create_on(0, H, W, D, ctypes.byref(p), ctypes.byref(h))

    assert lib.smt_crossagg_flow_create_on(0, 8, 8, 8, None, None) == SMT_ERR_ARG
    for H, W, D in [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, 8, 0), (8, 8, 513), (1 << 16, 1 << 16, 8)]:
        assert create(H, W, D) == SMT_ERR_ARG, (H, W, D)
    for kw in (dict(L1=-1), dict(L1=256), dict(num_iters=-1)):
        assert create(8, 8, 8, **kw) == SMT_ERR_ARG, kw
    assert h.value is None
    assert lib.smt_crossagg_flow_run_batch(None, None, None, None, None, 1, 3, None, None, None, None) == SMT_ERR_ARG
    assert lib.smt_crossagg_flow_destroy(None) == SMT_ERR_ARG
    assert lib.smt_crossagg_flow_set_stream(None, None) == SMT_ERR_ARG
    assert lib.smt_crossagg_flow_set_impl(None, 0) == SMT_ERR_ARG
    assert lib.smt_crossagg_flow_volumes(None, None, None) == SMT_ERR_ARG


def test_flow_is_declared_in_the_header_and_bound():
    hdr = open(os.path.join(ROOT, "include", "smt.h")).read()
    for name in ("smt_crossagg_flow_default_params", "smt_crossagg_flow_create_on", "smt_crossagg_flow_destroy",
                 "smt_crossagg_flow_set_stream", "smt_crossagg_flow_run_batch", "smt_crossagg_flow_volumes",
                 "smt_crossagg_flow_set_impl", "smt_crossagg_selftest_first_pass"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_lib(), name), name
    from stereo_match_traditional_amd import api, shard
    assert callable(api.CrossAggFlow) and "CrossAggFlow" in api.__all__ and callable(shard.crossagg_batch)
