"""The NCC and ASW kernels against exact arithmetic (exact_matchers.py): every formulation's cost volume within the bound
derived for its arithmetic, NaN and sentinel patterns exactly, and every returned map equal to the reference's WinTakeAll
rule applied to the same call's own cost volume -- exactly, with no tie band.  The oracle is held to the same references
in test_exact_matchers_cpu.py; here it only serves the count of bit differences against the loop-nest kernel."""
import numpy as np
import pytest
import torch

import exact_matchers as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}                                     # (family, formulation) -> largest error seen, in units of its bound


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)


def say(capsys, text):
    with capsys.disabled():
        print("\n" + text)


@pytest.fixture
def hooks(smt):
    yield smt
    smt.ncc_set_impl(2)
    smt.asw_set_impl(0)
    smt.asw_both_set_impl(2)


NCC_FORM_NAME = {"int": "integer sums (k_ncc_stats + k_ncc2), 2^-50 |exact|", "loop": "loop nest (k_ncc), 4 n 2^-53"}


@pytest.mark.parametrize("idx", range(len(X.NCC_CASES)), ids=X.NCC_IDS)
def test_ncc_against_exact(hooks, O, capsys, idx):
    smt = hooks
    H, W, D, win, _ = X.NCC_CASES[idx]
    L, R, exact, flat, sentinel = X.ncc_case(idx)
    border = np.ones((H, W), bool)
    border[win:H - win, win:W - win] = False
    lines, costs = [], {}
    for impl in (2, 1):
        smt.ncc_set_impl(impl)
        disp, cost = smt.NCC_algorithem(T(L), T(R), win, D, want_cost=True)
        disp, cost = disp.cpu().numpy(), cost.cpu().numpy()
        form = X.ncc_form(win, impl)
        worst = X.check_ncc(cost, exact, flat, sentinel, win, form)
        note(("NCC", NCC_FORM_NAME[form]), worst)
        assert np.array_equal(disp, X.ncc_wta(cost, win)), impl           # the map of the call's own costs, exactly
        assert (disp[border] == 0).all(), impl
        costs[impl] = cost
        lines.append(f"  ncc_set_impl({impl}) [{form}]: largest |cost - exact| = {worst:.6g} x bound")
    if 2 * win + 1 > 31:                       # both settings took the loop nest
        ok = ~np.isnan(costs[1])
        assert np.array_equal(costs[1][ok].view(np.uint64), costs[2][ok].view(np.uint64))
    if win == 0:                               # side 1: every window is flat
        assert np.isnan(costs[2][~sentinel & ~border[..., None]]).all()
    # the loop-nest kernel against the oracle, bit for bit: counted and printed, not asserted
    _, oc = O.ncc(L, R, D, win, want_cost=True)
    valid = ~np.isnan(exact)
    differ = int((costs[1][valid].view(np.uint64) != oc[valid].view(np.uint64)).sum())
    note(("NCC", "loop nest vs oracle: hypotheses whose bits differ"), float(differ))
    lines.append(f"  loop nest against the oracle: {differ} of {int(valid.sum())} hypotheses differ in their bits")
    say(capsys, f"NCC {X.NCC_IDS[idx]}:\n" + "\n".join(lines))


def test_ncc_batch_equals_single_calls(hooks):
    """smt_ncc_batch on two of the cases (same shape, different images) stacked: the single calls' maps"""
    smt = hooks
    a, b = 0, 8
    assert X.NCC_CASES[a][:4] == X.NCC_CASES[b][:4]
    H, W, D, win, _ = X.NCC_CASES[a]
    Ls = T(np.stack([X.ncc_case(a)[0], X.ncc_case(b)[0]]))
    Rs = T(np.stack([X.ncc_case(a)[1], X.ncc_case(b)[1]]))
    for impl in (2, 1):
        smt.ncc_set_impl(impl)
        got = smt.ncc_batch(Ls, Rs, win, D)
        for k in range(2):
            disp, cost = smt.NCC_algorithem(Ls[k], Rs[k], win, D, want_cost=True)
            assert torch.equal(got[k], disp), (impl, k)
            assert np.array_equal(disp.cpu().numpy(), X.ncc_wta(cost.cpu().numpy(), win)), (impl, k)


@pytest.mark.parametrize("idx", range(len(X.ASW_CASES)), ids=X.ASW_IDS)
def test_asw_against_exact(hooks, O, capsys, idx):
    smt = hooks
    H, W, D, ws, Tt, _, _ = X.ASW_CASES[idx]
    _, _, Lp, Rp, sp, cm, exact, nan = X.asw_case(idx)
    tl, tr, tsp, tcm = T(Lp), T(Rp), T(sp), T(cm)
    lines = []

    def held(name, cost, disp, v):
        cost, disp = cost.cpu().numpy(), disp.cpu().numpy()
        worst = X.check_asw(cost, exact[v], ws, nan[v])
        note(("ASW", name), worst)
        assert np.array_equal(disp, X.asw_wta(cost)), (name, v)           # first strict minimum of the call's own costs
        assert (disp[nan[v][..., 0]] == 0).all(), (name, v)
        if Tt == 0:
            assert (cost[~nan[v]].view(np.uint32) == 0).all(), (name, v)
        lines.append(f"  {name}, view {v}: largest |cost - exact| = {worst:.6g} x bound")
        return disp

    maps = {}
    for impl in (0, 6, 1):
        smt.asw_set_impl(impl)
        for view, v in ((smt.VIEW_LEFT, 0), (smt.VIEW_RIGHT, 1)):
            disp, cost = smt.AdaptiveSupportWeight(tl, tr, ws, D, tsp, tcm, Tt, view, want_cost=True)
            maps[impl, v] = held(f"smt_asw, asw_set_impl({impl})", cost, disp, v)
    smt.asw_set_impl(0)
    for both in (2, 1):
        smt.asw_both_set_impl(both)
        dl, dr, cl, cr = smt.AdaptiveSupportWeightBoth(tl, tr, ws, D, tsp, tcm, Tt, want_cost=True)
        ml = held(f"smt_asw_both costL, asw_both_set_impl({both})", cl, dl, 0)
        mr = held(f"smt_asw_both costR, asw_both_set_impl({both})", cr, dr, 1)
        dl2, dr2 = smt.AdaptiveSupportWeightBoth(tl, tr, ws, D, tsp, tcm, Tt)          # maps only
        assert np.array_equal(dl2.cpu().numpy(), ml) and np.array_equal(dr2.cpu().numpy(), mr), both
    if (H, W) == (4, 3):
        assert nan[1].all() and (maps[0, 1] == 0).all()
    say(capsys, f"ASW {X.ASW_IDS[idx]}:\n" + "\n".join(lines))


def test_asw_flow_returns_the_rule_on_the_single_calls_costs(hooks, O):
    """ASWFlow on the first case: its maps are the first-minimum rule applied to the cost volumes of the single calls"""
    smt = hooks
    idx = 0
    H, W, D, ws, Tt, _, sc = X.ASW_CASES[idx]
    L, R, Lp, Rp, sp, cm, _, _ = X.asw_case(idx)
    f = smt.ASWFlow(H, W, D, winSize=ws, T=Tt, sigma_space=X.ASW_SIGMA_SPACE, sigma_color=sc)
    dl, dr, _ = f.run(T(L), T(R))
    f.close()
    for view, got in ((smt.VIEW_LEFT, dl), (smt.VIEW_RIGHT, dr)):
        _, cost = smt.AdaptiveSupportWeight(T(Lp), T(Rp), ws, D, T(sp), T(cm), Tt, view, want_cost=True)
        assert np.array_equal(got[0].cpu().numpy(), X.asw_wta(cost.cpu().numpy())), view


def test_report_of_the_largest_errors(capsys):
    """prints what the tests above collected: per family and formulation, the largest error in units of its bound"""
    say(capsys, "largest observed error in units of the bound:\n" +
        "\n".join(f"  {fam}: {name}: {val:.6g}" for (fam, name), val in sorted(WORST.items())))
