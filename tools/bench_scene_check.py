#!/usr/bin/env python3
"""Cost of the scene check (SceneConsistency.check: se_scene_probe_f64 + its torch epilogue) beside the forward of the same batch
and beside the same quantities written in plain torch on the same device, at full frame size (1024 x 1280 rays, the demo frame's
512 x 640 depth map).

    python tools/bench_scene_check.py [--batches 1 8 32] [--samples 0 3] [--warmup 3] [--reps 20] [--baseline_reps 3]
                                      [--no_forward] [--no_baseline] [--out result.json]

HIP events around one call, median of --reps after --warmup; the torch baseline (scene_points-style masking, broadcast distances
and dot products, min / argmin / max / argmax, chunked over frames and probes to fit memory) runs --baseline_reps times after one
warm-up: it is tens of times slower.  ``kernel_ms`` times the bare ``_lib.scene_probe`` call (both launches), ``check_ms`` the
whole ``check()``.  ``model_gbps`` is the traffic model "ray table once + B depth maps" (H W 24 B + B dh dw 4 B) over kernel_ms: a
lower bound on the bytes the first launch moves, so a figure, not a share of peak - the launch is bound by float64 arithmetic
(``pairs_per_ns``: B P H W probe-pixel pairs over kernel_ms).  Prints one JSON line per (batch, probes)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, load_config, synth  # noqa: E402
from sceneego_amd.config import resolve_calibration_path  # noqa: E402
from sceneego_amd.render import MAX_DEPTH, MIN_Z  # noqa: E402
from sceneego_amd.scene_check import SceneConsistency  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def timed(fn, warmup, reps):
    """(median, min, max) milliseconds of fn()."""
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_probe(depth, ray_tab, probes, frame_chunk=4, probe_chunk=4):
    """The kernel's quantities in plain torch float64: (nearest_q, nearest_index, sight_dot, sight_index), each [B,P]."""
    B, dh, dw = depth.shape
    H, W = ray_tab.shape[:2]
    P = probes.shape[1]
    dev = depth.device
    sy = (torch.arange(H, device=dev) * dh) // H
    sx = (torch.arange(W, device=dev) * dw) // W
    rays = ray_tab.reshape(-1, 3)
    q_out = torch.empty((B, P), device=dev, dtype=torch.float64)
    t_out = torch.empty((B, P), device=dev, dtype=torch.float64)
    qi = torch.empty((B, P), device=dev, dtype=torch.int64)
    ti = torch.empty((B, P), device=dev, dtype=torch.int64)
    for b0 in range(0, B, frame_chunk):
        dd = depth[b0:b0 + frame_chunk][:, sy][:, :, sx].double().reshape(-1, H * W)      # [b,N]
        s = rays[None] * dd[..., None]                                                    # [b,N,3]
        keep = (dd > 0) & (dd <= MAX_DEPTH) & (s[..., 2] > MIN_Z)
        for p0 in range(0, P, probe_chunk):
            c = probes[b0:b0 + frame_chunk, p0:p0 + probe_chunk]                          # [b,p,3]
            e = s[:, None] - c[:, :, None]                                                # [b,p,N,3]
            q = (e * e).sum(dim=-1)
            q = torch.where(keep[:, None], q, torch.full_like(q, float("inf")))
            v, i = q.min(dim=2)
            q_out[b0:b0 + frame_chunk, p0:p0 + probe_chunk], qi[b0:b0 + frame_chunk, p0:p0 + probe_chunk] = v, i
            t = torch.einsum("nk,bpk->bpn", rays, c)
            v, i = t.max(dim=2)
            t_out[b0:b0 + frame_chunk, p0:p0 + probe_chunk], ti[b0:b0 + frame_chunk, p0:p0 + probe_chunk] = v, i
    return q_out, qi, t_out, ti


def measure(sc, net, depth_half, B, S, args):
    dev = sc.device
    depth = depth_half[None].expand(B, -1, -1).contiguous()
    joints = torch.from_numpy(np.load(os.path.join(GOLD, "demo_exr_b1.npz"))["joints"][:1]).to(dev).double().expand(B, -1, -1)
    # every frame its own skeleton: the golden joints shifted by a few centimetres
    shift = torch.linspace(-0.05, 0.05, B, device=dev, dtype=torch.float64)[:, None, None]
    joints = (joints + shift).contiguous()
    probes = sc.probes(joints, S)
    P = probes.shape[1]
    out, index, scratch = sc._buffers(B, P)
    H, W = sc.H, sc.W
    r = {"batch": B, "probes": P, "rays": [H, W], "depth": list(depth.shape[1:])}

    med, lo, hi = timed(lambda: _lib.scene_probe(depth, sc.ray_tab, probes, out, index, scratch=scratch, min_z=MIN_Z, max_depth=MAX_DEPTH),
                        args.warmup, args.reps)
    r["kernel_ms"], r["kernel_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    model_bytes = H * W * 24 + B * depth.shape[1] * depth.shape[2] * 4
    r["model_mb"] = round(model_bytes / 1e6, 1)
    r["model_gbps"] = round(model_bytes / 1e6 / med, 1)                         # MB / ms = GB / s
    r["pairs_per_ns"] = round(B * P * H * W / (med * 1e6), 2)
    med, lo, hi = timed(lambda: sc.check(depth, joints, samples_per_bone=S), args.warmup, args.reps)
    r["check_ms"], r["check_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]

    if args.no_baseline:
        return r
    # the baseline, and that it computes the same thing
    q, qi, t, ti = torch_probe(depth, sc.ray_tab, probes)
    _lib.scene_probe(depth, sc.ray_tab, probes, out, index, scratch=scratch, min_z=MIN_Z, max_depth=MAX_DEPTH)
    r["baseline_matches"] = bool(torch.equal(qi.int(), index[..., 0]) and torch.equal(ti.int(), index[..., 1])
                                 and torch.allclose(q, out[..., 0], rtol=1e-12, atol=0) and torch.allclose(t, out[..., 5], rtol=1e-12, atol=0))
    med, lo, hi = timed(lambda: torch_probe(depth, sc.ray_tab, probes), 1, args.baseline_reps)
    r["torch_ms"], r["torch_ms_range"] = round(med, 3), [round(lo, 3), round(hi, 3)]
    r["torch_over_kernel"] = round(med / r["kernel_ms"], 1)
    r["torch_over_check"] = round(med / r["check_ms"], 1)
    return r


def measure_forward(net, r, B, dev, args):
    if net is not None:
        img, d = synth.make_inputs(77, B, "floor")
        img, d = img.to(dev), d.to(dev)

        def forward():
            with torch.no_grad():
                net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=d)
        med, lo, hi = timed(forward, 2, max(3, args.reps // 4))
        r["forward_ms"], r["forward_ms_range"] = round(med, 3), [round(lo, 3), round(hi, 3)]
        r["check_share_of_forward"] = round(r["check_ms"] / med, 4)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--samples", type=int, nargs="+", default=[0, 3], help="samples per bone: 0 -> 15 probes, 3 -> 60")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline_reps", type=int, default=3)
    ap.add_argument("--no_forward", action="store_true", help="skip the forward beside it (no network is built)")
    ap.add_argument("--no_baseline", action="store_true", help="skip the torch baseline (profiler runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_check.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth
    dev = torch.device("cuda")
    cfg = load_config()
    sc = SceneConsistency(resolve_calibration_path(cfg.dataset.camera_calibration_path), device=dev, config=cfg)
    depth_half = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))).to(dev)
    net = None
    if not args.no_forward:
        from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
        net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
        net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
        net = net.to(dev).eval()
    results = []
    for B in args.batches:
        for S in args.samples:
            r = measure_forward(net, measure(sc, net, depth_half, B, S, args), B, dev, args)
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
