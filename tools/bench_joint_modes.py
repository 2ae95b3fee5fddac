#!/usr/bin/env python3
"""Cost of the joint modes (se_joint_modes_f32) beside the joint statistics (se_joint_stats_f32), which read the same volumes once,
and beside the forward of the same batch: B x 15 rows of G^3 voxels.

    python tools/bench_joint_modes.py [--batches 1 8 32] [--grid 64] [--k 4] [--radius 2] [--warmup 3] [--reps 20] [--no_forward]
                                      [--out result.json]

HIP events around one call, median of --reps after --warmup, the same call back to back.  Two kinds of volumes:
  forward: the softmaxed volumes the network's own forward wrote for a synthetic batch (synthetic weights: flat, noisy distributions
           with about ten thousand local maxima per joint: the worst case for the mode search);
  bumps:   one or two Gaussian bumps per joint whose tails underflow, a handful of modes per joint (what the tests use).
GB/s is the volume read once (rows * G^3 * 4 B) over the time.  The forward is the eager module call at that batch (no graph, one
stream), timed the same way.  Prints one JSON line per batch size.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, load_config, op, synth  # noqa: E402

JOINTS = 15


def timed(fn, warmup, reps):
    """Median, minimum and maximum milliseconds of fn()."""
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


def bump_volumes(rows, G, coord, dev, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    ax = torch.arange(G, dtype=torch.float64)
    logits = torch.empty((rows, G, G, G), dtype=torch.float32)
    for r in range(rows):
        v = torch.zeros((G, G, G), dtype=torch.float64)
        for _ in range(1 + r % 2):
            c = torch.rand(3, generator=gen, dtype=torch.float64) * (G - 2) + 0.5
            w = float(torch.rand(1, generator=gen)) * 2.0 + 1.0
            g = [torch.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
            v += g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
        v = (v - v.mean()) / v.std() * 7.0
        logits[r] = (v + 0.01 * torch.randn(v.shape, generator=gen, dtype=torch.float64)).float()
    logits = logits.reshape(rows, G ** 3).to(dev)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=dev)
    _lib.softargmax3d(logits, coord, prob, joints, rows, G ** 3, 1)
    return prob, joints


def measure_ops(prob, joints, coord, G, K, radius, warmup, reps):
    rows, N = prob.shape
    dev = prob.device
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev)
    idx = torch.empty((rows,), device=dev, dtype=torch.int32)
    ws_js = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev)
    modes = torch.empty((rows, K, _lib.MODES_SLOTS), device=dev)
    index = torch.empty((rows, K), device=dev, dtype=torch.int32)
    count = torch.empty((rows,), device=dev, dtype=torch.int32)
    total = torch.empty((rows,), device=dev, dtype=torch.int32)
    ws_jm = torch.empty(_lib.joint_modes_scratch_bytes(rows, G, K), device=dev, dtype=torch.uint8)

    def joint_stats():
        _lib.joint_stats(prob, coord, joints, stats, idx, rows, N, scratch=ws_js)

    def joint_modes():
        _lib.joint_modes(prob, coord, modes, index, count, total, rows, N, G, K, radius, 0.0, scratch=ws_jm)

    mb = rows * N * 4 / 1e6
    r = {}
    for name, fn in (("joint_stats", joint_stats), ("joint_modes", joint_modes)):
        med, lo, hi = timed(fn, warmup, reps)
        r[f"{name}_ms"] = round(med, 4)
        r[f"{name}_ms_range"] = [round(lo, 4), round(hi, 4)]
        r[f"{name}_gbps"] = round(mb / med, 1)          # MB / ms = GB / s
    r["ratio_to_joint_stats"] = round(r["joint_modes_ms"] / r["joint_stats_ms"], 3)
    r["modes_per_row_median"] = int(total.float().median().item())
    return r


def measure(B, G, K, radius, warmup, reps, dev, net):
    rows, N = B * JOINTS, G ** 3
    coord = op.build_coord_volume(G, 2.0).reshape(N, 3).contiguous().to(dev)
    r = {"batch": B, "grid": G, "rows": rows, "k": K, "radius": radius, "volume_mb": round(rows * N * 4 / 1e6, 1)}
    prob, joints = bump_volumes(rows, G, coord, dev, seed=B)
    r["bumps"] = measure_ops(prob, joints, coord, G, K, radius, warmup, reps)
    if net is not None:
        img, depth = synth.make_inputs(77, B, "floor")
        img, depth = img.to(dev), depth.to(dev)

        def forward():
            return net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)

        with torch.no_grad():
            med, lo, hi = timed(forward, warmup, reps)
            kp, _, vols, _ = forward()
        r["forward_ms"] = round(med, 4)
        r["forward_ms_range"] = [round(lo, 4), round(hi, 4)]
        fwd_coord = net.coord_volumes[0].reshape(N, 3).to(device=dev, dtype=torch.float32).contiguous()
        r["forward_volumes"] = measure_ops(vols.reshape(rows, N).contiguous(), kp.reshape(rows, 3).contiguous(), fwd_coord, G, K, radius,
                                           warmup, reps)
        r["joint_modes_share_of_forward"] = round(r["forward_volumes"]["joint_modes_ms"] / med, 5)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="skip the forward and its volumes (needed for a --grid other than the model's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_joint_modes.py needs an MI355X (HIP device)")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda")
    net = None
    if not args.no_forward:
        from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
        net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
        net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
        net = net.to(dev).eval()
        if net.volume_size != args.grid:
            raise SystemExit(f"the model's grid is {net.volume_size}: pass --grid {net.volume_size} or --no_forward")
    results = []
    for B in args.batches:
        r = measure(B, args.grid, args.k, args.radius, args.warmup, args.reps, dev, net)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
