"""Random-shape sweep of the batched flows on reused handles (the table and the oracle compositions:
tests/fuzz_flow_cases.py; what the table reaches: tests/test_fuzz_flows_cpu.py).  One test function per family.  For
every group: one handle, its three batches with different images and pair counts in order, then the first batch again.
Every output of every pair against the oracle -- maps, class maps, counts and volumes bit for bit, NCC / ASW costs under
the bounds of exact_matchers.py -- and the repeated first batch against the bytes of its first run.  The tensors the api
allocates for its outputs are prefilled (NaN, or a sentinel no output holds), so an element a flow does not write cannot
pass.  status() follows every run; the only status let through is SMT_ERR_REF_UB of a pipeline under flags 0, where the
reference's right-arm stride reads beside the plane (as the two existing pipeline tests let it through)."""
import numpy as np
import pytest
import torch

import cblsm_v4_cases as VC
import exact_matchers as X
import fuzz_flow_cases as FC
from prefill import U8_SENTINEL, flows  # noqa: F401  (the fixture: the api's output tensors come prefilled)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                           # a copy: the tables' arrays are read-only


def N(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)


class Checker:
    """names a mismatch: family, group, batch, pair, output, and the first differing elements"""

    def __init__(self, family, g, k):
        self.tag = f"{family} {g['name']} batch {k} (P = {g['batches'][k]['P']})"

    def same(self, p, name, got, want):
        got, want = N(got), np.ascontiguousarray(want)
        if got.shape != want.shape or got.dtype != want.dtype or got.tobytes() != want.tobytes():
            pytest.fail(f"{self.tag} pair {p} {name}: {FC.first_diff(got, want)}", pytrace=False)

    def same_volume(self, p, name, got, want):
        """bit for bit where finite, NaN where NaN (costAggregationV4's empty rectangles)"""
        got = N(got)
        if not VC.same_volume(got, want):
            g2 = np.where(np.isnan(got), np.float32(0), got)
            w2 = np.where(np.isnan(want), np.float32(0), want)
            pytest.fail(f"{self.tag} pair {p} {name}: NaN pattern equal: {np.array_equal(np.isnan(got), np.isnan(want))}; "
                        f"finite part: {FC.first_diff(g2, w2)}", pytrace=False)

    def ok(self, cond, p, what):
        if not cond:
            pytest.fail(f"{self.tag} pair {p}: {what}", pytrace=False)


def _again(family, g, first, second):
    for name in first:
        a, b = first[name], second[name]
        if a.tobytes() != b.tobytes():
            pytest.fail(f"{family} {g['name']}: batch 0 run again after the third batch, {name}: {FC.first_diff(b, a)}",
                        pytrace=False)


def _sweep(family, O, make, run, close):
    """make(g) -> handle; run(handle, g, k, pairs, oracle, vols, Checker) -> dict of every output as numpy"""
    for g in FC.groups(family):
        h = make(g)
        first = None
        for k in (0, 1, 2, 0):
            outs, vols = FC.oracle_batch(family, g, k, O)
            pairs = FC.bgr_pairs(g, k, O) if family == "crossagg" or g.get("channels") == 3 else FC.gray_pairs(g, k, O)
            got = run(h, g, k, pairs, outs, vols, Checker(family, g, k))
            if first is None:
                first = got
            elif k == 0:
                _again(family, g, first, got)
        close(h)


def _stack(pairs, i):
    return np.stack([p[i] for p in pairs])


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline(flows, O, monkeypatch):
    smt = flows
    from stereo_match_traditional_amd import SmtError
    from stereo_match_traditional_amd._lib import QUIRK_FIX_RIGHT_ARM_STRIDE, SMT_ERR_REF_UB

    def make(g):
        if g["schedule"] is None:
            monkeypatch.delenv("SMT_PIPE_SCHEDULE", raising=False)
        else:
            monkeypatch.setenv("SMT_PIPE_SCHEDULE", g["schedule"])               # read when the handle is created
        return smt.Pipeline(g["H"], g["W"], g["D"], DEV, quirks=QUIRK_FIX_RIGHT_ARM_STRIDE if g["fix_stride"] else 0)

    def status(pipe, g):
        try:
            pipe.status()
        except SmtError as e:
            if g["fix_stride"] or e.status != SMT_ERR_REF_UB:
                raise

    def run(pipe, g, k, pairs, outs, vols, C):
        Lb, Rb = T(_stack(pairs, 0)), T(_stack(pairs, 1))
        dl, dr, cls, counts = pipe.run(Lb, Rb)
        status(pipe, g)
        got = dict(run_dl=N(dl), run_dr=N(dr), run_cls=N(cls), run_counts=N(counts))
        for name, v in zip(("cost_left", "cost_right", "agg_left", "agg_right", "scanline_sum"), pipe.volumes()):
            got["vol_" + name] = N(v.clone())
            C.same(len(pairs) - 1, "volume " + name, got["vol_" + name], vols[name])
        pl, pr, pcls, pcounts, last = pipe.run_post(Lb, Rb)
        status(pipe, g)
        got.update(post_dl=N(pl), post_dr=N(pr), post_cls=N(pcls), post_counts=N(pcounts), post_last=N(last))
        for p, o in enumerate(outs):
            C.same(p, "run dispL", got["run_dl"][p], o["lr"])
            C.same(p, "run dispR", got["run_dr"][p], o["dr"])
            C.same(p, "run cls", got["run_cls"][p], o["cls"])
            C.same(p, "run counts", got["run_counts"][p], o["counts"])
            C.same(p, "run_post dispL", got["post_dl"][p], o["sp"])
            C.same(p, "run_post dispR", got["post_dr"][p], o["dr"])
            C.same(p, "run_post cls", got["post_cls"][p], o["cls"])
            C.same(p, "run_post counts", got["post_counts"][p], o["counts"])
            C.same(p, "run_post lastDisp", got["post_last"][p], o["med"])
        return got

    _sweep("pipeline", O, make, run, lambda pipe: pipe.close())


# ------------------------------------------------------------------------------------------------ CBLSM
def test_cblsm(flows, O):
    smt = flows

    def make(g):
        return smt.CBLSMFlow(g["H"], g["W"], g["D"], DEV, tau=g["tau"], max_length=g["max_length"], sec_length=g["sec_length"])

    def run(f, g, k, pairs, outs, vols, C):
        Lb, Rb = T(_stack(pairs, 0)), T(_stack(pairs, 1))
        last = len(pairs) - 1
        dl, dr = f.run(Lb, Rb)
        f.status()
        got = dict(run_dl=N(dl), run_dr=N(dr))
        for name, v in zip(("pass1_left", "pass1_right"), f.volumes()):
            got[name] = N(v.clone())
            C.same(last, "volume " + name, got[name], vols[name])
        pl, pr, cls, counts = f.run_post(Lb, Rb)
        f.status()
        got.update(post_dl=N(pl), post_dr=N(pr), post_cls=N(cls), post_counts=N(counts))
        v4 = f.run_v4(Lb, Rb)
        f.status()
        got.update(v4_dl=N(v4), v4_volume=N(f.volumes()[0].clone()))
        C.same_volume(last, "costAggregationV4 volume", got["v4_volume"], vols["v4"])
        for p, o in enumerate(outs):
            C.same(p, "run dispL", got["run_dl"][p], o["dl"])
            C.same(p, "run dispR", got["run_dr"][p], o["dr"])
            C.same(p, "run_post dispL", got["post_dl"][p], o["post_fin"])
            C.same(p, "run_post dispR", got["post_dr"][p], o["dr"])
            C.same(p, "run_post cls", got["post_cls"][p], o["post_cls"])
            C.same(p, "run_post counts", got["post_counts"][p], o["post_counts"])
            C.same(p, "run_v4 dispL", got["v4_dl"][p], o["v4"])
        return got

    _sweep("cblsm", O, make, run, lambda f: f.close())


# ------------------------------------------------------------------------------------------------ CrossAgg
def test_crossagg(flows, O):
    smt = flows

    def make(g):
        return smt.CrossAggFlow(g["H"], g["W"], g["D"], DEV, L1=g["L1"], L2=g["L2"], t1=g["t1"], t2=g["t2"],
                                num_iters=g["num_iters"], gate=g["gate"])

    def run(f, g, k, pairs, outs, vols, C):
        bL, bR = T(_stack(pairs, 0)), T(_stack(pairs, 1))
        gray = (T(_stack(pairs, 2)), T(_stack(pairs, 3))) if g["gray_given"] else (None, None)
        last = len(pairs) - 1
        dl, dr = f.run(bL, bR, *gray)
        f.status()
        got = dict(run_dl=N(dl), run_dr=N(dr))
        for name, v in zip(("left", "right"), f.volumes()):
            got["vol_" + name] = N(v.clone())
            C.same(last, "volume " + name, got["vol_" + name], vols[name])
        keep = torch.full(dl.shape, -7.0, dtype=torch.float32, device=DEV)
        ol, orr = f.run(bL, bR, *gray, views=smt.VIEW_LEFT, dispR=keep)
        f.status()
        C.ok(orr is keep and bool((keep == -7.0).all()), "all", "views = left wrote dispR")
        got["left_only"] = N(ol)
        ol, orr = f.run(bL, bR, *gray, views=smt.VIEW_RIGHT, dispL=keep)
        f.status()
        C.ok(ol is keep and bool((keep == -7.0).all()), "all", "views = right wrote dispL")
        got["right_only"] = N(orr)
        ll, lr_, cls, counts = f.run(bL, bR, *gray, lr_check=True)
        f.status()
        got.update(lr_dl=N(ll), lr_dr=N(lr_), lr_cls=N(cls), lr_counts=N(counts))
        pl, pr, pcls, pcounts = f.run_post(bL, bR, *gray)
        f.status()
        got.update(post_dl=N(pl), post_dr=N(pr), post_cls=N(pcls), post_counts=N(pcounts))
        for p, o in enumerate(outs):
            C.same(p, "run dispL", got["run_dl"][p], o["dl"])
            C.same(p, "run dispR", got["run_dr"][p], o["dr"])
            C.same(p, "run(views = left) dispL", got["left_only"][p], o["dl"])
            C.same(p, "run(views = right) dispR", got["right_only"][p], o["dr"])
            C.same(p, "run(lr_check) dispL", got["lr_dl"][p], o["lr"])
            C.same(p, "run(lr_check) dispR", got["lr_dr"][p], o["dr"])
            C.same(p, "run(lr_check) cls", got["lr_cls"][p], o["cls"])
            C.same(p, "run(lr_check) counts", got["lr_counts"][p], o["counts"])
            C.same(p, "run_post dispL", got["post_dl"][p], o["post_fin"])
            C.same(p, "run_post dispR", got["post_dr"][p], o["dr"])
            C.same(p, "run_post cls", got["post_cls"][p], o["post_cls"])
            C.same(p, "run_post counts", got["post_counts"][p], o["post_counts"])
        return got

    _sweep("crossagg", O, make, run, lambda f: f.close())


# ------------------------------------------------------------------------------------------------ SAD
def test_sad(flows, O):
    smt = flows

    def run(f, g, k, pairs, outs, vols, C):
        dl, dr, last, cls = f.run(T(_stack(pairs, 0)), T(_stack(pairs, 1)))
        got = dict(dl=N(dl), dr=N(dr), last=N(last), cls=N(cls))
        for p, o in enumerate(outs):
            for name in ("dl", "dr", "last", "cls"):
                C.same(p, name, got[name][p], o[name])
        return got

    _sweep("sad", O, lambda g: smt.SADFlow(g["H"], g["W"], g["D"], DEV, winsize=g["winsize"]), run, lambda f: f.close())


# ------------------------------------------------------------------------------------------------ NCC
def test_ncc(flows, O):
    """Costs against the exact rational reference under the bound of the form that ran (integer sums: 2^-50 |exact|; loop
    nest: 4 n 2^-53), NaN and sentinel patterns exactly, border costs +0.0; the map is the reference's argmax rule on
    the call's own costs and O.ncc's map, both exactly."""
    smt = flows

    def run(f, g, k, pairs, outs, vols, C):
        win, D, H, W = g["winSize"], g["D"], g["H"], g["W"]
        Lb, Rb = T(_stack(pairs, 0)), T(_stack(pairs, 1))
        border = np.ones((H, W), bool)
        border[win:H - win, win:W - win] = False
        got = {}
        for form in g["forms"]:
            f.set_form(form)
            disp, cost = f.run(Lb, Rb, want_cost=True)
            disp, cost = N(disp), N(cost)
            got[f"disp_form{form}"], got[f"cost_form{form}"] = disp, cost
            ran = form or FC.ncc_rule(2 * win + 1, D)
            if not border.all():
                C.ok(smt.ncc_last_form() == ran, "all", f"form {form}: ran form {smt.ncc_last_form()}, expected {ran}")
            for p, o in enumerate(outs):
                C.ok((disp[p][border] == 0).all() and (cost[p][border].view(np.uint64) == 0).all(), p,
                     f"form {form}: border pixels must hold map 0 and cost +0.0")
                if "exact" not in o:
                    continue
                try:
                    X.check_ncc(cost[p], o["exact"], o["flat"], o["sentinel"], win, "loop" if ran == FC.NCC_LOOP else "int")
                except AssertionError as e:
                    pytest.fail(f"{C.tag} pair {p} form {form} (ran {ran}): {e}", pytrace=False)
                C.same(p, f"form {form}: map against the rule on the call's own costs", disp[p], X.ncc_wta(cost[p], win))
                C.same(p, f"form {form}: map against O.ncc", disp[p], o["disp"])
        return got

    _sweep("ncc", O, lambda g: smt.NCCFlow(g["H"], g["W"], g["D"], DEV, winSize=g["winSize"]), run, lambda f: f.close())


# ------------------------------------------------------------------------------------------------ ASW
def test_asw(flows, O):
    """The flow's maps are the first-minimum rule on the costs of smt_asw_both for the same pair (as
    test_asw_flow_returns_the_rule_on_the_single_calls_costs), those costs are held to the exact reference under
    exact_matchers.asw_bound, and the cross-checked map is O.asw_crosscheck of the flow's own two maps.  Against O.asw's own
    maps a pixel may differ only inside the oracle's two-ulp tie band (then the cross-checked maps may differ as well)."""
    smt = flows

    def run(f, g, k, pairs, outs, vols, C):
        ws, D, H, W = g["winSize"], g["D"], g["H"], g["W"]
        dl, dr, last = f.run(T(_stack(pairs, 0)), T(_stack(pairs, 1)))
        got = dict(dl=N(dl), dr=N(dr), last=N(last))
        sp, cm = smt.asw_masks(ws, FC.ASW_SIGMA_SPACE, FC.ASW_SIGMA_COLOR, DEV)
        for p, o in enumerate(outs):
            _, _, cl, cr = smt.AdaptiveSupportWeightBoth(T(o["Lp"]), T(o["Rp"]), ws, D, sp, cm, FC.ASW_T, want_cost=True)
            for v, cost, name in ((0, N(cl), "dl"), (1, N(cr), "dr")):
                try:
                    X.check_asw(cost, o["exact_l" if v == 0 else "exact_r"], ws, X.asw_nan_mask(H, W, D, ws, v))
                except AssertionError as e:
                    pytest.fail(f"{C.tag} pair {p} view {v}: {e}", pytrace=False)
                C.same(p, f"{name} against the rule on the pair's own costs", got[name][p], X.asw_wta(cost))
                # against O.asw's map: a pixel may differ only where the oracle's two smallest float costs lie within two
                # float ulps (the rule of test_wide_disparity_gpu.py; the float64 sums are reassociated)
                ref = o["cost_l" if v == 0 else "cost_r"]
                srt = np.sort(np.where(np.isnan(ref), np.float32(np.inf), ref), axis=2)
                if D > 1:
                    with np.errstate(invalid="ignore"):
                        tie = (srt[..., 1] - srt[..., 0]).astype(np.float64) <= 2.0 * np.spacing(srt[..., 0]).astype(np.float64)
                else:
                    tie = np.zeros((H, W), bool)
                off = (got[name][p] != o[name]) & ~tie
                C.ok(not off.any(), p, f"{name} differs from O.asw outside the oracle's tie band at {np.argwhere(off)[:5].tolist()}")
            C.same(p, "lastDisp", got["last"][p], O.asw_crosscheck(got["dl"][p], got["dr"][p]))
        return got

    _sweep("asw", O, lambda g: smt.ASWFlow(g["H"], g["W"], g["D"], DEV, winSize=g["winSize"]), run, lambda f: f.close())


# ------------------------------------------------------------------------------------------------ host-fed AD-Census
def test_host_fed(flows, O):
    smt = flows

    def make(g):
        return smt.ADCensusHostBatch(g["H"], g["W"], g["D"], g["sigmaC"], g["sigmaS"], channels=g["channels"],
                                     out_dtype=torch.uint8 if g["u8"] else torch.float32, chunk=g["chunk"], device=DEV)

    def run(hb, g, k, pairs, outs, vols, C):
        L, R = torch.from_numpy(_stack(pairs, 0)), torch.from_numpy(_stack(pairs, 1))
        shp = (len(pairs), g["H"], g["W"])
        if g["u8"]:
            dl, dr = (torch.full(shp, U8_SENTINEL, dtype=torch.uint8).pin_memory() for _ in range(2))
        else:
            dl, dr = (torch.full(shp, float("nan"), dtype=torch.float32).pin_memory() for _ in range(2))
        ol, orr = hb.run(L.pin_memory() if k % 2 else L, R.pin_memory() if k % 2 else R, dl, dr)
        C.ok(ol is dl and orr is dr, "all", "run must fill the caller's tensors")
        got = dict(dl=dl.numpy().copy(), dr=dr.numpy().copy())
        for p, o in enumerate(outs):
            C.same(p, "dispL", got["dl"][p], o["dl"])
            C.same(p, "dispR", got["dr"][p], o["dr"])
        return got

    _sweep("host", O, make, run, lambda hb: hb.close())
