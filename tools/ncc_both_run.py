"""One smt_lrncc call at NCC_main.cpp's window (21x21) on a 450x375 pair -- timing / rocprofv3.
usage: ncc_both_run.py [reps] [lrncc impl: 0 rule, 1 composed, 2 keys] [smt_ncc impl: 2 dot4, 3 box] [D]"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_match_traditional_amd as smt
from stereo_match_traditional_amd import synth
DEV = torch.device("cuda:0")
D = int(sys.argv[4]) if len(sys.argv) > 4 else 64
H, W, win = 375, 450, 10
L, R = synth.synth_pair(H, W, min(D, 64), 1)
Lt, Rt = torch.from_numpy(L).to(DEV), torch.from_numpy(R).to(DEV)
smt.lrncc_set_impl(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
smt.ncc_set_impl(int(sys.argv[3]) if len(sys.argv) > 3 else 2)
for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 2):
    dl, dr = smt.NCC_both(Lt, Rt, win, D)
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record(); dl, dr = smt.NCC_both(Lt, Rt, win, D); b.record(); torch.cuda.synchronize()
print("ncc both ms", a.elapsed_time(b), "form", smt.lrncc_last_form(), "left form", smt.ncc_last_form(),
      "Mdisp/s (both views)", 2 * (H - 2 * win) * (W - 2 * win) * D / a.elapsed_time(b) / 1e3)
