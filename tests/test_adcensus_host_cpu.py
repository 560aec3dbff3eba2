"""Host-side check of the host-fed batch's enqueue schedule (hostfeed.hip, no GPU): the op list a run executes, simulated
with happens-before over its three streams -- every wait after its record, no slot overwritten before its last reader,
every pair copied in and out once, every pair's tables built once."""
import ctypes

import pytest

SMT_OK, SMT_ERR_ARG = 0, -1


@pytest.fixture(scope="module")
def lib():
    from stereo_match_traditional_amd import build
    lib = ctypes.CDLL(build.build())
    lib.smt_adcensus_host_selftest_schedule.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


@pytest.mark.parametrize("pairs", [1, 2, 3, 7, 8, 9, 64, 257])
@pytest.mark.parametrize("chunk", [1, 2, 3, 8, 32])
def test_schedule_is_sound(lib, pairs, chunk):
    """Fewer pairs than a chunk, ragged last chunks, one and many chunks."""
    assert lib.smt_adcensus_host_selftest_schedule(pairs, chunk) == SMT_OK


def test_schedule_of_no_pairs_is_empty_and_sound(lib):
    assert lib.smt_adcensus_host_selftest_schedule(0, 4) == SMT_OK


@pytest.mark.parametrize("pairs,chunk", [(4, 0), (4, -1), (-1, 4), (-5, 0)])
def test_schedule_rejects_bad_arguments(lib, pairs, chunk):
    assert lib.smt_adcensus_host_selftest_schedule(pairs, chunk) == SMT_ERR_ARG


def test_create_rejects_bad_arguments_without_a_device(lib):
    """Argument checks come before any HIP call: u8 maps need D <= 256, channels 1 or 3, chunk >= 1."""
    f = lib.smt_adcensus_host_create
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    h = ctypes.c_void_p()
    for args in [(-1, 24, 130, 320, 10.0, 30.0, 1, 1, 4), (-1, 24, 130, 64, 10.0, 30.0, 2, 0, 4),
                 (-1, 24, 130, 64, 10.0, 30.0, 1, 2, 4), (-1, 24, 130, 64, 10.0, 30.0, 1, 0, 0),
                 (-1, 0, 130, 64, 10.0, 30.0, 1, 0, 4), (-1, 24, 130, 513, 10.0, 30.0, 1, 0, 4)]:
        assert f(*args, ctypes.byref(h)) == SMT_ERR_ARG, args
    assert lib.smt_adcensus_host_run(None, None, None, 0, None, None) == SMT_ERR_ARG
