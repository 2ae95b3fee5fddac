"""GPU: every BASELINE.json configuration at its stated size.

configs[3] (batch 256 over 8 GPUs) runs 32 frames per GPU: its per-GPU share is the B=32 float32 forward below (the
8-process launch itself is the driver's; the sharding + all-gather are covered over gloo in test_dist_gloo.py and over
RCCL - or, on a 1-GPU box, with both ranks on one device - by test_two_ranks_launch_sharding_and_all_gather).  configs[2] is B=32 with bf16 V2V storage;
configs[4] is the 128^3 grid.  Frames are independent, so inside a large batch the frames taken from the reference
goldens must reproduce the goldens' joints (<= 1e-3 m, BASELINE.json north_star), every frame must equal its own B=1
run, and a batch permutation must permute the result.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sceneego_amd import _lib, load_config, synth
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth

from conftest import ROOT, case_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
JOINT_TOL = 1e-3
RUN_NOISE = 5e-5        # MIOpen's atomic split-K backbone kernels are not bitwise reproducible (test_gpu_forward.py)


def _build(volume_size=64, **kw):
    cfg = load_config()
    cfg.model.volume_size = volume_size
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False, **kw)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


def _forward(net, img, depth):
    with torch.no_grad():
        out = net(img.to(DEV), net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth.to(DEV))
    torch.cuda.synchronize()
    return out


def _batch_with_golden_frames(golden_meta, total):
    """[total] frames: frame 0 = golden b1_floor, frames 1-2 = golden b2_uniform, the rest seeded (uniform / floor mix)."""
    m1 = next(c for c in golden_meta["cases"] if c["name"] == "b1_floor")
    m2 = next(c for c in golden_meta["cases"] if c["name"] == "b2_uniform")
    i1, d1 = case_inputs(m1)
    i2, d2 = case_inputs(m2)
    n_u = (total - 3 + 1) // 2
    iu, du = synth.make_inputs(4242, n_u, "uniform")
    i_f, d_f = synth.make_inputs(4243, total - 3 - n_u, "floor")
    return torch.cat([i1, i2, iu, i_f]), torch.cat([d1, d2, du, d_f])


@pytest.fixture(scope="module")
def net64():
    return _build()


def test_config4_per_gpu_share_b32_fp32(net64, golden, golden_meta):
    """configs[3]: 32 frames per GPU, float32."""
    img, depth = _batch_with_golden_frames(golden_meta, 32)
    kp, feats, vols, _ = _forward(net64, img, depth)
    assert tuple(kp.shape) == (32, 15, 3) and tuple(vols.shape) == (32, 15, 64, 64, 64)
    k = kp.cpu().numpy()
    e1 = float(np.abs(k[0:1] - golden("b1_floor")["joints"]).max())
    e2 = float(np.abs(k[1:3] - golden("b2_uniform")["joints"]).max())
    assert e1 <= JOINT_TOL and e2 <= JOINT_TOL, (e1, e2)
    # every 5th frame equals its own B=1 run
    for b in range(3, 32, 5):
        one = _forward(net64, img[b:b + 1], depth[b:b + 1])[0]
        assert float((one - kp[b:b + 1]).abs().max()) < RUN_NOISE, b
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(1))
    kp_perm = _forward(net64, img[perm], depth[perm])[0]
    assert float((kp_perm - kp[perm.to(DEV)]).abs().max()) < RUN_NOISE
    assert bool(torch.isfinite(kp).all()) and bool(torch.isfinite(vols).all())
    s = vols.reshape(32, 15, -1).sum(dim=2)
    assert float((s - 1).abs().max()) < 1e-3          # softmaxed volumes


def test_config3_b32_bf16_accuracy(golden, golden_meta):
    """configs[2]: B=32 with bf16 V2V storage.  The bound is the accuracy this mode is specified to."""
    from test_gpu_bf16 import BF16_JOINT_TOL
    net = _build()
    net.set_v2v_dtype("bf16")
    img, depth = _batch_with_golden_frames(golden_meta, 32)
    kp, _, vols, _ = _forward(net, img, depth)
    assert net.volume_net.program.dtype == torch.bfloat16
    k = kp.cpu().numpy()
    e1 = float(np.abs(k[0:1] - golden("b1_floor")["joints"]).max())
    e2 = float(np.abs(k[1:3] - golden("b2_uniform")["joints"]).max())
    print(f"bf16 B=32: joint error vs float32 reference goldens {e1:.2e} / {e2:.2e} m")
    assert e1 <= BF16_JOINT_TOL and e2 <= BF16_JOINT_TOL, (e1, e2)
    # logits of both programs on the same input: the bound that does not depend on the sharpness of the soft-argmax
    from test_gpu_bf16 import BF16_LOGIT_RMS_TOL
    cap = {}
    orig, orig_finish = _lib.softargmax3d, _lib.softargmax3d_finish

    def hook(vol, *a, **k):             # the two-pass kernel: (logits, coord, ...)
        cap["logits"] = vol.clone()
        return orig(vol, *a, **k)

    def hook_finish(vol, *a, **k):      # pass 2 behind a fused tail (float32 since round 4, bf16 since round 6): (logits, scratch, ...)
        cap["logits"] = vol.clone()
        return orig_finish(vol, *a, **k)
    _lib.softargmax3d, _lib.softargmax3d_finish = hook, hook_finish
    try:
        _forward(net, img[:4], depth[:4])
        lg_b = cap.pop("logits").double()
        net.set_v2v_dtype("fp32")
        kp32 = _forward(net, img, depth)[0]
        cap.clear()
        _forward(net, img[:4], depth[:4])
        lg_f = cap.pop("logits").double()
    finally:
        _lib.softargmax3d, _lib.softargmax3d_finish = orig, orig_finish
    assert not torch.equal(lg_b, lg_f)          # two programs, two captures
    rel = float((lg_b - lg_f).pow(2).mean().sqrt() / lg_f.std())
    err = float((kp - kp32).abs().max())
    print(f"bf16 B=32: max joint difference to the float32 program over all 32 frames {err:.2e} m; logits rms error {rel:.2e} x std")
    per_joint = (kp - kp32).norm(dim=-1).flatten()
    med = float(per_joint.median())
    print(f"           per-joint distance to the float32 program: median {med:.2e} m, 95 % {float(per_joint.quantile(0.95)):.2e} m, max {float(per_joint.max()):.2e} m")
    # 480 joints: the tail is wider than on the 45 golden joints and moves from run to run with MIOpen's non-reproducible
    # float32 backbone (measured over runs: median 3.4e-3 .. 6e-3 m, 95 % 1.7e-2 m, max 4.9e-2 .. 6.3e-2 m)
    assert med <= 1.5e-2 and float(per_joint.quantile(0.95)) <= BF16_JOINT_TOL and err <= 0.15, (med, err)
    assert rel <= BF16_LOGIT_RMS_TOL, rel
    assert bool(torch.isfinite(vols).all())


def test_config5_g128_b8(golden, golden_meta):
    """configs[4] at its stated size (128^3 grid, batch 8): frame 0 reproduces the reference golden, every frame equals its own
    B=1 run, a batch permutation permutes the result."""
    net = _build(volume_size=128)
    m = next(c for c in golden_meta["cases"] if c["name"] == "b1_g128_floor")
    i1, d1 = case_inputs(m)
    i2, d2 = synth.make_inputs(909, 4, "uniform")
    i3, d3 = synth.make_inputs(910, 3, "floor")
    img, depth = torch.cat([i1, i2, i3]), torch.cat([d1, d2, d3])
    kp, _, vols, _ = _forward(net, img, depth)
    assert tuple(kp.shape) == (8, 15, 3) and tuple(vols.shape) == (8, 15, 128, 128, 128)
    err = float(np.abs(kp[0:1].cpu().numpy() - golden("b1_g128_floor")["joints"]).max())
    print(f"128^3 B=8: frame 0 vs reference golden {err:.2e} m")
    assert err <= JOINT_TOL, err
    s = vols.reshape(8, 15, -1).sum(dim=2)
    assert float((s - 1).abs().max()) < 1e-3 and bool(torch.isfinite(kp).all())
    del vols
    for b in (1, 4, 7):
        one = _forward(net, img[b:b + 1], depth[b:b + 1])[0]
        assert float((one - kp[b:b + 1]).abs().max()) < RUN_NOISE, b
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(5))
    kp_perm = _forward(net, img[perm], depth[perm])[0]
    assert float((kp_perm - kp[perm.to(DEV)]).abs().max()) < RUN_NOISE


def test_conv7_planar3_g128_b32_unit_table_budget():
    """the F(4,7) front layer at 128^3 with B >= 28 used to overflow its per-workgroup unit table (436 entries) and
    raise; the launcher now cuts the batch by the table budget.  Every sample of the B=32 launch equals the B=2 launch."""
    from sceneego_amd.v2v import _PackedConv
    torch.manual_seed(3)
    conv = torch.nn.Conv3d(33, 16, 7, padding=3).to(DEV)
    bn = torch.nn.BatchNorm3d(16).to(DEV).eval()
    pc = _PackedConv(conv, bn, 48, torch.float32)
    G = 128
    base = torch.randn((2, 11, G, G, G, 3), device=DEV)
    x = base.repeat(16, 1, 1, 1, 1, 1).contiguous()
    out = torch.empty((32, G, G, G, 16), device=DEV)
    _lib.conv3d(x, pc.w, pc.b, None, out, 32, G, 33, 48, 16, 7, _lib.EPI_RELU | _lib.IN_PLANAR3)
    ref = torch.empty((2, G, G, G, 16), device=DEV)
    _lib.conv3d(base, pc.w, pc.b, None, ref, 2, G, 33, 48, 16, 7, _lib.EPI_RELU | _lib.IN_PLANAR3)
    torch.cuda.synchronize()
    for k in (0, 13, 27, 31):
        assert torch.equal(out[k], ref[k % 2]), k
    assert float(out.abs().max()) > 0


def test_materialize_features_matches_reference_golden(golden):
    """Boundary: with materialize_features=True the 2nd return value is the reference's literal [B,32,1024,1280] tensor
    (network/voxel_net_depth.py:238,275); compared with values sampled from the real reference forward (tools/make_golden.py
    --only-features-big)."""
    g = golden("b1_floor_features_big")
    net = _build(materialize_features=True)
    img, depth = synth.make_inputs(77, 1, "floor")
    kp, feats, _, _ = _forward(net, img, depth)
    assert tuple(feats.shape) == tuple(g["shape"]) == (1, 32, 1024, 1280) and feats.dtype == torch.float32
    rows = torch.from_numpy(g["rows"]).to(DEV)
    cols = torch.from_numpy(g["cols"]).to(DEV)
    got = feats[0][:, rows][:, :, cols].cpu().numpy()
    np.testing.assert_allclose(got, g["values"], rtol=2e-3, atol=2e-3)          # MIOpen vs oneDNN float32 backbone
    assert float(np.abs(g["values"][:, :, -7]).max()) == 0.0 and float(np.abs(got[:, :, -7]).max()) == 0.0   # column 127: zero pad
    assert float(np.abs(kp.cpu().numpy() - golden("b1_floor")["joints"]).max()) <= JOINT_TOL
    # default build: compact map, documented deviation
    assert tuple(_forward(_build(), img, depth)[1].shape) == (1, 32, 64, 64)


def test_softargmax_propagates_nan():
    """torch.softmax + einsum propagate a NaN logit (utils/op.py:83-96); so must the HIP soft-argmax."""
    G = 16
    N = G ** 3
    vol = torch.randn((2, N), device=DEV)
    vol[1, 1234] = float("nan")
    coord = torch.rand((N, 3), device=DEV)
    out_vol = torch.empty_like(vol)
    joints = torch.empty((2, 3), device=DEV)
    _lib.softargmax3d(vol, coord, out_vol, joints, 2, N, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(joints[0]).all()) and bool(torch.isfinite(out_vol[0]).all())
    assert bool(torch.isnan(joints[1]).all()) and bool(torch.isnan(out_vol[1]).all())


def test_two_ranks_launch_sharding_and_all_gather():
    """configs[3]'s launch path at world size 2: `python bench.py --gpus 2` typed without a launcher starts its own 2-rank job, every
    rank runs its shard with consecutive steps pipelined over the default number of HIP streams, the joints are all-gathered once per step behind each
    step's event, and the line carries the parity of rank 0's frames and the cross-rank shard check.  With two GPUs: one rank per GPU
    over RCCL (the production backend).  On a 1-GPU box: both ranks on cuda:0 (SCENEEGO_SHARE_GPU=1) with gloo for the collective -
    RCCL refuses two ranks on one device - so the stream ordering + sharding code is still executed on hardware every round."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    two = torch.cuda.device_count() >= 2
    if not two:
        env.update(SCENEEGO_SHARE_GPU="1", SCENEEGO_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--batch", "2",
                        "--full", "--no-cpu-baseline", "--no-extras", "--profile-steps", "2"], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4 and line["config"]["streams"] == 3
    assert line["parity"]["pass"] and line["parity"]["max_joint_err_m"] <= JOINT_TOL
    assert line["shard_check"]["max_abs_diff_m"] <= line["shard_check"]["tol"]
    assert line["rccl_ranks"] == {"world_size": 2, "backend": "nccl" if two else "gloo"} and len(line["rank_ms_per_step"]) == 2
    assert line["step_ms"]["min"] <= line["step_ms"]["median"] <= line["step_ms"]["max"] and len(line["repeat_values"]["values"]) == 3
    # round 5: the collective's cost on the line (HIP events around all_gather_into_tensor in the separate timing pass)
    assert line["allgather_us"]["n"] >= 1 and 0.0 < line["allgather_us"]["median"] <= line["allgather_us"]["max"]
    print(("RCCL, one rank per GPU" if two else "both ranks on cuda:0, gloo collective") + f": {line['value']} frames/s, parity "
          f"{line['parity']['max_joint_err_m']:.2e} m, shard check {line['shard_check']['max_abs_diff_m']:.2e} m")


@pytest.mark.parametrize("batch,steps,streams", [(1, 3, 2), (32, 2, 1)])
def test_eight_ranks_launch_on_whatever_gpus_there_are(batch, steps, streams):
    """configs[3] is 8 ranks on one node.  The launcher, rendezvous, per-rank core pinning, sharded seeds, step-ordered all-gather
    and the cross-rank shard check at WORLD_SIZE 8 - `python bench.py --gpus 8 --batch N` as the driver will type it - every round:
    one rank per GPU over RCCL when the box has 8 devices, otherwise all ranks share the visible device(s) with gloo for the
    collective (RCCL refuses two ranks on one device).  batch 1: the launch path; batch 32: configs[3]'s REAL
    per-rank workload - 32 frames per rank, the [256, 15, 3] gather, every rank's buffers at size (8 x ~12 GB on a shared device)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    full = torch.cuda.device_count() >= 8
    if not full:
        env.update(SCENEEGO_SHARE_GPU="1", SCENEEGO_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", str(steps), "--warmup", "1", "--batch", str(batch),
                        "--streams", str(streams), "--full", "--no-cpu-baseline", "--no-extras", "--no-kernel-events", "--no-repeats"],
                       capture_output=True, text=True, env=env, timeout=2400)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["config"]["global_batch"] == 8 * batch
    assert line["rccl_ranks"] == {"world_size": 8, "backend": "nccl" if full else "gloo"} and len(line["rank_ms_per_step"]) == 8
    assert line["parity"]["pass"] and line["parity"]["max_joint_err_m"] <= JOINT_TOL
    assert line["shard_check"]["max_abs_diff_m"] <= line["shard_check"]["tol"]
    assert r.stderr.count("[sceneego dist] rank") == 8          # every rank reported its device / backend / cores once
    print(("RCCL, one rank per GPU" if full else "8 ranks on the visible device(s), gloo collective") +
          f": {line['value']} frames/s, shard check {line['shard_check']['max_abs_diff_m']:.2e} m, per-rank ms {line['rank_ms_per_step']}")
