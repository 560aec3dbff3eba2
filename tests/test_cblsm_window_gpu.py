"""CBLSM's window cost volumes and the window-cost flow on the device (csrc/cblsm_window.hip,
smt_cblsm_flow_run_batch_window) against the restatement of tests/cblsm_window_cases.py: both gray forms bit for bit under
the tap loop and under the box kernel with three band heights, V4, the identity between the two views, the kernel's own
quotient over every sum, the caller's memory (guards, gaps, prefill, scratch history, a busy side stream), and the flow
against the oracle composition, on reused handles and against the composed single calls.

No test provokes a fault: the undefined case of RIGHT is an argument check that returns before any launch."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena  # noqa: E402
import bounds_cases as BC  # noqa: E402
import cblsm_window_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAY = {"left": WC.LEFT, "right": WC.RIGHT}
# (impl, band): the tap loop; the box kernel under its own band, one row per band and three
HOOKS = [(1, 0), (2, 0), (2, 1), (2, 3)]


@pytest.fixture(scope="module")
def X(smt, O):
    return BC.Ctx(O, "cuda:0")


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(case, form):
    """(padded pair, restated volume) of a table case, computed once"""
    H, W, D, ws = case
    Lp, Rp = WC.pair(H, W, ws, 1, 3) if form == WC.V4 else WC.case_pair(case)
    return Lp, Rp, WC.ref_volume(Lp, Rp, D, ws, form)


def _device(smt, Lp, Rp, D, ws, form, impl=0, band=0):
    """-> (volume on NaN-prefilled memory, last_form); the inputs must come back unchanged"""
    f = {WC.LEFT: smt.ComputeDispLeft, WC.RIGHT: smt.ComputeDispRight, WC.V4: smt.ComputeDispV4}[form]
    w = ws + 1
    Lt, Rt = _T(Lp), _T(Rp)
    out = torch.full((Lp.shape[0] - 2 * w, Lp.shape[1] - 2 * w, D), float("nan"), device=DEV)
    smt.cblsm_window_set_impl(impl); smt.cblsm_window_set_band(band)
    try:
        f(Lt, Rt, ws, D, out=out)
        torch.cuda.synchronize()
        last = smt.cblsm_window_last_form()
    finally:
        smt.cblsm_window_set_impl(0); smt.cblsm_window_set_band(0)
    assert np.array_equal(Lt.cpu().numpy(), Lp) and np.array_equal(Rt.cpu().numpy(), Rp)
    return out, last


# ================================================================================================ volumes
@pytest.mark.parametrize("impl,band", HOOKS, ids=[f"impl{i}-band{b}" for i, b in HOOKS])
@pytest.mark.parametrize("form", GRAY)
@pytest.mark.parametrize("case", WC.TABLE, ids=str)
def test_gray_volumes_bit_for_bit(smt, case, form, impl, band):
    f = GRAY[form]
    if not WC.legal(case, f):
        Lp, Rp = WC.case_pair(case)
        with pytest.raises(smt._lib.SmtError) as e:
            _device(smt, Lp, Rp, case[2], case[3], f, impl, band)
        assert e.value.status == BC.SMT_ERR_REF_UB
        return
    Lp, Rp, want = _case(case, f)
    got, last = _device(smt, Lp, Rp, case[2], case[3], f, impl, band)
    assert last == impl
    assert np.array_equal(_bits(got), _bits(want))


def test_dispatch_rule_runs_a_formulation_and_agrees(smt):
    case = (9, 20, 12, 1)
    for f in (WC.LEFT, WC.RIGHT):
        Lp, Rp, want = _case(case, f)
        got, last = _device(smt, Lp, Rp, 12, 1, f)
        assert last in (1, 2) and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("case", WC.TABLE, ids=str)
def test_v4_bit_for_bit(smt, case):
    Lp, Rp, want = _case(case, WC.V4)
    got, last = _device(smt, Lp, Rp, case[2], case[3], WC.V4, impl=2)
    assert last == 1, "V4 ships as the tap loop"
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("impl", (1, 2))
@pytest.mark.parametrize("case", [(9, 20, 12, 1), (6, 70, 65, 1), (5, 150, 130, 1), (40, 50, 16, 14)], ids=str)
def test_right_is_left_on_the_diagonal(smt, case, impl):
    """RIGHT[y][x'][d] == LEFT[y][x' + d][d] wherever x' + d <= W - 1 - w: the same two windows, from device results only"""
    H, W, D, ws = case
    w = ws + 1
    Lp, Rp = WC.case_pair(case)
    left = _device(smt, Lp, Rp, D, ws, WC.LEFT, impl)[0].cpu().numpy()
    right = _device(smt, Lp, Rp, D, ws, WC.RIGHT, impl)[0].cpu().numpy()
    seen = 0
    for d in range(min(D, W - w)):
        n = W - w - d                                              # x' = 0 .. W - 1 - w - d
        assert np.array_equal(right[:, :n, d].view(np.uint32), left[:, d:d + n, d].view(np.uint32)), d
        seen += n
    assert seen > 0


@pytest.mark.parametrize("side", (3, 5, 9, 31, 181))
def test_kernel_quotient_for_every_sum(smt, side):
    n = side * side
    S = np.arange(255 * n + 1, dtype=np.uint32)
    St, out = _T(S), torch.full((S.size,), float("nan"), device=DEV)
    rc = smt._lib.lib().smt_cblsm_window_quotient(C.c_void_p(St.data_ptr()), S.size, n, C.c_void_p(out.data_ptr()),
                                                   smt.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    got, want = out.cpu().numpy(), WC.quotient(S.astype(np.int64), n)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"side {side}: {bad.size} sums differ, first S = {int(bad[0])}: {got[bad[0]]!r} != {want[bad[0]]!r}"


# ================================================================================================ bounds and stream
_TABLE = [(n, p) for n in ("smt_cblsm_window_cost_batch", "smt_cblsm_flow_run_batch_window") for p in BC.CASES[n]]


@pytest.mark.parametrize("name,params", _TABLE, ids=[f"{n}-{BC.case_id(p)}" for n, p in _TABLE])
def test_guards_gaps_prefill_inputs_and_restatement(X, name, params):
    """tests/arena.py: guard words on both sides of every tensor and in the gaps of a strided batch, inputs unchanged, two
    prefills (one of NaN words) giving the same bytes, the restatement"""
    BC.run_case(X, name, params)


def test_scratch_history_does_not_reach_the_result(X, smt):
    name, params = "smt_cblsm_window_cost_batch", dict(H=5, W=33, D=20, ws=1, form=WC.RIGHT, impl=2, band=2, gap=1, P=3)
    warm = BC.run_case(X, name, params)
    for byte in (0xFF, 0x00):
        smt.scratch_poison(byte)
        o, verify = BC.run_once(X, name, params, arena.SEEDS[0])
        verify(o)
        BC.assert_same(warm, o, f"{name}: warm call against the call after smt_scratch_poison({byte:#x})")


@pytest.mark.parametrize("name,params", [
    ("smt_cblsm_window_cost_batch", dict(H=5, W=33, D=20, ws=1, form=WC.LEFT, impl=2, gap=1, P=3)),
    ("smt_cblsm_flow_run_batch_window", dict(H=5, W=65, D=64, ws=1, P=2))], ids=("volume", "flow"))
def test_busy_side_stream_with_inputs_written_on_it(X, name, params):
    from test_stream_order_gpu import run_deferred
    probe = run_deferred(X, name, BC.ENTRIES[name], params)
    assert probe.returns and all(busy for busy, _ in probe.returns), probe.returns


# ================================================================================================ the flow
def _flow_check(O, L, R, D, ws, dl, dr, vols=None):
    cl, cr, wl, wr = WC.flow_oracle(O, L, R, D, ws)
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr)
    if vols is not None:
        assert np.array_equal(_bits(vols[0]), _bits(cl)) and np.array_equal(_bits(vols[1]), _bits(cr))


@pytest.mark.parametrize("H,W,D,ws", [(12, 17, 20, 1), (6, 5, 9, 1), (20, 30, 40, 2), (375, 450, 60, 1)])
def test_flow_against_the_oracle_composition(smt, O, H, W, D, ws):
    """maps and both first-pass volumes; the last shape is CBLSM.cpp's own (:28-32) with its 5 x 5 window"""
    L, R = O.synth_pair(H, W, D, 11 + H)
    f = smt.CBLSMFlow(H, W, D)
    dl, dr = f.run_window(_T(L), _T(R), ws)
    f.status()
    vols = [v.clone() for v in f.volumes()]
    f.close()
    assert dl.shape == (1, H, W)
    _flow_check(O, L, R, D, ws, dl[0].cpu().numpy(), dr[0].cpu().numpy(), vols)


def test_reused_handle_batches_and_window_sizes(smt, O):
    H, W, D = 10, 21, 24
    batches = [[O.synth_pair(H, W, D, 30 + 10 * k + b, noise=(b == 1)) for b in range(n)] for k, n in enumerate((3, 1, 2))]
    f = smt.CBLSMFlow(H, W, D)

    def run(batch, ws):
        L, R = np.stack([p[0] for p in batch]), np.stack([p[1] for p in batch])
        dl, dr = f.run_window(_T(L), _T(R), ws)
        f.status()
        vols = [v.clone() for v in f.volumes()]
        return dl.cpu().numpy(), dr.cpu().numpy(), vols

    first = None
    for batch in batches:
        dl, dr, vols = run(batch, 1)
        first = first or (dl, dr)
        for b, (l, r) in enumerate(batch):
            _flow_check(O, l, r, D, 1, dl[b], dr[b], vols if b == len(batch) - 1 else None)
    for ws in (0, 2):
        dl, dr, vols = run(batches[1], ws)
        _flow_check(O, *batches[1][0], D, ws, dl[0], dr[0], vols)
    dl, dr, _ = run(batches[0], 1)
    f.close()
    assert np.array_equal(dl, first[0]) and np.array_equal(dr, first[1])


def test_flow_equals_the_composed_single_calls(smt, O):
    """ComputeDispLeft / ComputeDispRight on the padded images plus four costAggregationV5 on the library's own arms"""
    H, W, D, ws = 14, 33, 30, 1
    L, R = O.synth_pair(H, W, D, 5)
    Lt, Rt = _T(L), _T(R)
    ca = [smt.CrossArmAggregation().Initialize(H, W, 25, D, DEV, style="cblsm", sec_length=17, max_length=34) for _ in range(2)]
    ca[0].ComputeArmLengths(Lt)
    ca[1].ComputeArmLengths(Rt)
    Lp, Rp = smt.copyMakeBorder_replicate(Lt, ws + 1), smt.copyMakeBorder_replicate(Rt, ws + 1)
    vl, vr = smt.ComputeDispLeft(Lp, Rp, ws, D), smt.ComputeDispRight(Lp, Rp, ws, D)
    gl, gr, g2 = torch.empty_like(vl), torch.empty_like(vl), torch.empty_like(vl)
    dL, dR = torch.empty((H, W), device=DEV), torch.empty((H, W), device=DEV)
    ca[1].costAggregationV5(vr, gr)
    ca[0].costAggregationV5(vl, gl)
    ca[0].costAggregationV5(gl, g2, dL)
    ca[0].costAggregationV5(gr, g2, dR)
    for c in ca:
        c.status()
        c.close()
    f = smt.CBLSMFlow(H, W, D)
    dl, dr = f.run_window(Lt, Rt, ws)
    f.status()
    pl, pr = f.volumes()
    assert np.array_equal(_bits(pl), _bits(gl)) and np.array_equal(_bits(pr), _bits(gr))
    assert torch.equal(dl[0], dL) and torch.equal(dr[0], dR)
    f.close()


def test_run_and_run_window_interleave_on_one_handle(smt, O):
    from test_cblsm_flow_gpu import _oracle
    H, W, D = 9, 26, 20
    L, R = O.synth_pair(H, W, D, 8)
    Lt, Rt = _T(L), _T(R)
    _, _, al, ar = _oracle(O, L, R, D)
    f = smt.CBLSMFlow(H, W, D)
    for _ in range(2):
        dl, dr = f.run(Lt, Rt)
        f.status()
        assert np.array_equal(dl[0].cpu().numpy(), al) and np.array_equal(dr[0].cpu().numpy(), ar)
        dl, dr = f.run_window(Lt, Rt, 1)
        f.status()
        _flow_check(O, L, R, D, 1, dl[0].cpu().numpy(), dr[0].cpu().numpy(), [v.clone() for v in f.volumes()])
    f.close()


def test_flow_rejects_the_undefined_width_before_any_launch(smt):
    f = smt.CBLSMFlow(4, 2, 3)
    z = torch.zeros((1, 4, 2), dtype=torch.uint8, device=DEV)
    with pytest.raises(smt._lib.SmtError) as e:
        f.run_window(z, z, 1)
    assert e.value.status == BC.SMT_ERR_REF_UB
    f.status()
    f.close()


def test_cblsm_main_window_switch(smt, O):
    """host/cblsm_main.cpp --window=1: smt::ComputeDispLeft / ComputeDispRight on host-padded images and
    smt::CBLSMFlow::runWindow through the C++ mirror, hashes against the restatement and the oracle composition"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo_match_traditional_amd", "lib", "cblsm_main")
    assert os.path.exists(exe)
    H, W, D, seed, ws = 24, 40, 16, 6, 1
    r = subprocess.run([exe, str(H), str(W), str(D), str(seed), f"--window={ws}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    L, R = O.synth_pair(H, W, D, seed)
    Lp, Rp = np.pad(L, ws + 1, mode="edge"), np.pad(R, ws + 1, mode="edge")
    _, _, dl, dr = WC.flow_oracle(O, L, R, D, ws)
    exp = {"window_left": WC.ref_volume(Lp, Rp, D, ws, WC.LEFT), "window_right": WC.ref_volume(Lp, Rp, D, ws, WC.RIGHT),
           "disp_left_window": dl, "disp_right_window": dr}
    for k, v in exp.items():
        assert got[k] == f"{O.fnv1a(v):016x}", k
