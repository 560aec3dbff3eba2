"""The HIP kernels against the reference's own compiled AD-CensusV1 / CBLSM.h code, without the oracle in between:
every case of tests/golden/ref_pin_cases.py goes through the C ABI (by the Python mirror), the outputs are hashed
(NaN canonicalised) and compared with tests/golden/ref_pin_hashes.json, which `make_golden.py ref-pin` wrote from
the reference builds.  Reads tests/golden/ only.  Each stage runs under every formulation that promises identical
bits: smt_adcensus_force_generic 0 / 1, smt_crossarm_set_arm_walk 0 / 1, aggregation variants 1, 12 and 13."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ref_pin_cases as RP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = {r["case"]["name"]: r for r in
        json.load(open(os.path.join(ROOT, "tests", "golden", "ref_pin_hashes.json")))["cases"]}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _forms(case):
    k = case["kind"]
    if k == "adcensus":
        return [("generic", 0), ("generic", 1)]
    if k in ("arms", "cblsm_arms"):
        return [("arm_walk", 0), ("arm_walk", 1)]
    if k == "agg":
        if case["order"] == 2 or case["D"] > 256:
            return [("variant", 1)]         # the library runs these as the plain walk whatever the variant
        return [("variant", 1), ("variant", 12), ("variant", 13)]
    return [("only", 0)]


PARAMS = [pytest.param(c, f, id="%s-%s%d" % (c["name"], f[0], f[1])) for c in RP.CASES for f in _forms(c)]


def run_gpu(smt, case, inp, form):
    k = case["kind"]
    if k == "adcensus":
        H, W, D = case["H"], case["W"], case["D"]
        adc = smt.AD_Census().Initialize(T(inp["L"]), T(inp["R"]), D, H, W, 10.0, 30.0, placement_search=False,
                                         store_calibration=False)
        adc.force_generic(form[1])
        dl = torch.empty((H, W), device=DEV)
        dr = torch.empty((H, W), device=DEV)
        adc.ComputeBoth(dl, dr)
        adc.status()
        out = dict(volL=N(adc.GetPtrLeft()), volR=N(adc.GetPtrRight()), dispL=N(dl), dispR=N(dr))
        adc.close()
        return out
    if k in ("arms", "cblsm_arms"):
        H, W = case["H"], case["W"]
        ca = smt.CrossArmAggregation().Initialize(H, W, case["tau"], 8, DEV, style="cblsm" if k == "cblsm_arms" else "adcensus")
        ca.set_arm_walk(form[1])
        img = T(inp["img"])
        if k == "arms" and case["single"]:
            ca.Reset()
            for d in case["dirs"]:
                ca._arm_dir(img, d)
        else:
            ca.ComputeArmLengths(img)
        m = [N(a) for a in ca.arm_maps()]
        out = dict(armL=m[0], armR=m[1], armT=m[2], armB=m[3])
        if k == "arms" and case["single"]:
            out["tau"] = np.array([ca.tao()], np.int32)
        ca.close()
        return out
    if k == "agg":
        H, W, D, order = case["H"], case["W"], case["D"], case["order"]
        ca = smt.CrossArmAggregation().Initialize(H, W, 25 if order == 1 else 30, D, DEV,
                                                  style="cblsm" if order == 1 else "adcensus")
        ca.set_variant(form[1])
        ca.load_arm_maps(*[T(inp[n]) for n in ("armL", "armR", "armT", "armB")])
        out = torch.empty((H, W, D), device=DEV)
        disp = torch.empty((H, W), device=DEV)
        {0: ca.AggregationVertical, 1: ca.costAggregationV5, 2: ca.Aggregation}[order](T(inp["vol"]), out, disp)
        ca.status()          # the case is defined in the reference: no SMT_ERR_REF_UB
        res = dict(out=N(out), disp=N(disp))
        ca.close()
        return res
    if k == "scan":
        H, W, D = case["H"], case["W"], case["D"]
        so = smt.ScanlineOptimizer().Initialize(H, W, D, case["p1"], case["p2"], DEV)
        cost, gray = T(inp["cost"]), T(inp["gray"])
        o = {w: N(so.ScanPass(cost, gray, w)) for w in ("left", "right", "up", "down")}
        disp = torch.empty((H, W), device=DEV)
        o["sum"] = N(so.ScanLine(cost, gray, disp=disp))
        o["disp"] = N(disp)
        so.close()
        return o
    if k == "lrcheck":
        t = T(inp["dL"].copy())
        cls, no, nm = smt.LeftRightConsistency(case["W"], case["H"], case["gate"], t, T(inp["dR"]))
        return dict(dL=N(t), cls=N(cls), counts=np.array([no, nm], np.int32))
    if k == "lrvariant":
        last = torch.zeros((case["H"], case["W"]), device=DEV)
        cls, no, nm = smt.LeftAndRightConsistency(T(inp["dL"]), T(inp["dR"]), last, case["W"], case["H"], case["gate"])
        return dict(last=N(last), cls=N(cls), counts=np.array([no, nm], np.int32))
    if k == "fill":
        g = T(inp["disp"].copy())
        lst = smt.FillTheHole(case["row"], case["col"], case["D"], g, inp["occ"], inp["mis"])
        return dict(disp=N(g), mismatch=np.ascontiguousarray(np.asarray(lst, np.int32).reshape(-1, 2)))
    if k == "speckle":
        t = T(inp["disp"].copy())
        smt.RemoveSpeckles(t, case["W"], case["H"], case["diff"], case["area"], case["inv"])
        return dict(disp=N(t))
    if k == "median":
        return dict(out=N(smt.MedianFilter(T(inp["disp"]), case["W"], case["H"], case["wnd"])))
    if k == "cblsm_ad":
        L, R = T(inp["L"]), T(inp["R"])
        return dict(left=N(smt.cblsm_ComputeAD(L, R, case["D"], smt.VIEW_LEFT)),
                    right=N(smt.cblsm_ComputeAD(L, R, case["D"], smt.VIEW_RIGHT)))
    if k == "cblsm_disp":
        return dict(disp=N(smt.wta(T(inp["vol"]))))
    if k == "choose":
        H, W, D = case["H"], case["W"], case["D"]
        d = {n: T(a) for n, a in inp.items()}
        return dict(left=N(smt.chooseArmLengthLeft(d["LL"], d["LR"], d["RL"], d["RR"], D, None, H, W)),
                    right=N(smt.chooseArmLengthRight(d["LL"], d["LR"], d["RL"], d["RR"], D, None, H, W)),
                    up=N(smt.chooseArmLengthUp(d["LU"], d["LD"], d["RU"], d["RD"], d["RL"], d["RR"], D, None, H, W)),
                    down=N(smt.chooseArmLengthDown(d["LU"], d["LD"], d["RU"], d["RD"], d["RL"], d["RR"], D, None, H, W)))
    raise KeyError(k)


@pytest.mark.parametrize("case,form", PARAMS)
def test_hip_vs_reference_build(smt, O, case, form):
    """O only regenerates the inputs (integer synthetic images, numpy generators) and hashes; the expected values
    are the reference builds' hashes."""
    rec = GOLD[case["name"]]
    inp = RP.inputs(case, O)
    assert RP.hashes(inp, O) == rec["inputs"]
    out = run_gpu(smt, case, inp, form)
    got = RP.hashes(out, O)
    assert list(got) == list(rec["outputs"])
    wrong = [k for k in got if got[k] != rec["outputs"][k]]
    assert not wrong, "outputs %s differ from the reference build" % wrong
