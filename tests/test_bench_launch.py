"""bench.py as its own launcher: `python bench.py --gpus N` with no WORLD_SIZE starts N ranks
itself, relays rank 0's JSON line and fails if any rank fails.  CPU part: argument / failure handling.  GPU part: the
whole thing once with two ranks on the one visible device (SMT_BENCH_ONE_DEVICE=1: gloo rendezvous, host-side
exchange) -- a rehearsal of the plumbing, the line says it is not a scaling measurement."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_self_launch_relays_a_failing_rank():
    """No GPU here: both children die in torch.cuda.set_device; the parent must exit non-zero, promptly, with no
    JSON line.  (On a GPU box this test still holds: SMT_HIP_LIB points the children at a library that does not exist.)"""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-extras", "--cpu-rows", "0"],
             {"SMT_BENCH_ONE_DEVICE": "1", "SMT_HIP_LIB": "/nonexistent/libsmt_hip.so"}, timeout=300)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr


def test_more_ranks_than_devices_is_refused_without_the_rehearsal_switch():
    import torch
    n = torch.cuda.device_count() + 1
    if n < 2:
        n = 2
    r = _run(["--gpus", str(n), "--steps", "1"])
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr


@pytest.mark.gpu
def test_two_ranks_on_one_device_rehearsal():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--cpu-rows", "0", "--pairs-per-step", "2", "--full"],
             {"SMT_BENCH_ONE_DEVICE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["ranks_joined"] == 2 and rec["config"]["world_size"] == 2
    assert rec["config"]["launcher"].startswith("self")
    assert rec["value"] > 0 and rec["scaling"] == "weak"
    s = rec["extra"]["cfg5_kitti_256pairs_strong"]
    assert s["pairs_total"] == 256 and s["pairs_this_rank"] == 128 and s["ranks"] == 2
    assert s["gathered_maps"] == [256, 375, 1242] and s["checksum_allreduce_equals_sum_of_gathered"]
    assert s["value_with_gather"] > 0 and s["value_without_gather"] >= s["value_with_gather"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(smt, tmp_path):
    """A plain run prints the headline only (no --full measurements) and --dump-outputs writes the maps of the last timed
    step: the same bits as one ComputeBatch call over the same seeded pairs."""
    import numpy as np
    import torch
    from stereo_match_traditional_amd import synth
    out = tmp_path / "dump"
    r = _run(["--steps", "3", "--warmup", "1", "--workload", "adcensus_kitti_d256", "--pairs-per-step", "2",
              "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["unit"] == "Mdisp/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert not {"roofline", "extra", "cpu_baseline", "ms_single_pair_call"} & set(rec)
    assert sorted(p.name for p in out.iterdir()) == ["disp_left.npy", "disp_right.npy"]
    H, W, D = 375, 1242, 256
    dev = torch.device("cuda:0")
    Ls, Rs = zip(*[synth.synth_pair(H, W, D, 1000 + b) for b in range(2)])
    Lb = torch.from_numpy(np.stack(Ls).astype(np.float32)).to(dev)
    Rb = torch.from_numpy(np.stack(Rs).astype(np.float32)).to(dev)
    dl, dr = torch.empty((2, H, W), device=dev), torch.empty((2, H, W), device=dev)
    adc = smt.AD_Census().Initialize(Lb[0], Rb[0], D, H, W, 10.0, 30.0)
    adc.ComputeBatch(Lb, Rb, dl, dr)
    adc.status()
    adc.close()
    for name, want in (("disp_left", dl), ("disp_right", dr)):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (2, H, W)
        assert np.array_equal(got, want.cpu().numpy())
