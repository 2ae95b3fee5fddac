#!/usr/bin/env python3
"""Cost of one step of the grid Bayes filter (se_volume_filter_f32; VolumeFilter.step) beside the joint statistics
(se_joint_stats_f32) on the same volumes and beside the forward of the same batch: B frames x 15 rows of G^3 voxels.

    python tools/bench_volume_filter.py [--batches 1 8 32] [--grid 64] [--radius 10] [--floor 1e-3] [--warmup 3] [--reps 20]
                                        [--no_forward] [--out result.json]

HIP events around one call, median of --reps after --warmup, the same call back to back (the filter's state is warm: every timed step
is an update, none a restart).  The volumes are the softmaxed volumes the network's own forward wrote for a synthetic batch, or, with
--no_forward, Gaussian bumps.  A step of B frames is B sequential frames of 15 rows each (the batch of a sequence run is one track), so
its time grows with B at 15 rows' worth of parallelism per launch; ``step_beliefs`` also returns the beliefs.  TB/s is the kernel's own
byte model (csrc/volume_filter.hip: 28 B per frame, row and voxel, 32 B with the beliefs returned) over the time.  The forward is the
eager module call at that batch (no graph, one stream), timed the same way.  Prints one JSON line per batch size.
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
from sceneego_amd.volume_filter import VolumeFilter  # noqa: E402

JOINTS = 15
MODEL_BYTES = 28            # per frame, row and voxel (csrc/volume_filter.hip: BYTE MODEL); + 4 with the beliefs returned


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


def bump_volumes(B, G, coord, dev, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    ax = torch.arange(G, dtype=torch.float64)
    rows = B * JOINTS
    logits = torch.empty((rows, G, G, G), dtype=torch.float32)
    for r in range(rows):
        c = torch.rand(3, generator=gen, dtype=torch.float64) * (G - 2) + 0.5
        w = float(torch.rand(1, generator=gen)) * 2.0 + 1.0
        g = [torch.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
        v = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
        logits[r] = ((v - v.mean()) / v.std() * 7.0).float()
    logits = logits.reshape(rows, G ** 3).to(dev)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=dev)
    _lib.softargmax3d(logits, coord, prob, joints, rows, G ** 3, 1)
    return prob.view(B, JOINTS, G, G, G), joints.view(B, JOINTS, 3)


def measure_ops(vols, joints, coord, G, radius, floor, warmup, reps):
    B, J = vols.shape[:2]
    rows, N = B * J, G ** 3
    dev = vols.device
    flat, kp = vols.reshape(rows, N).contiguous(), joints.reshape(rows, 3).contiguous()
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev)
    idx = torch.empty((rows,), device=dev, dtype=torch.int32)
    ws_js = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev)
    h = 2.0 / G
    filt = VolumeFilter(coord, G, 2.0, sigma=radius * h / 3.0, radius=radius, floor=floor)
    filt.step(vols)                                     # the state is warm from here on

    def joint_stats():
        _lib.joint_stats(flat, coord, kp, stats, idx, rows, N, scratch=ws_js)

    def step():
        filt.step(vols)

    def step_beliefs():
        filt.step(vols, return_beliefs=True)

    r = {}
    med, lo, hi = timed(joint_stats, warmup, reps)
    r["joint_stats_ms"], r["joint_stats_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    for name, fn, per in (("step", step, MODEL_BYTES), ("step_beliefs", step_beliefs, MODEL_BYTES + 4)):
        med, lo, hi = timed(fn, warmup, reps)
        r[f"{name}_ms"] = round(med, 4)
        r[f"{name}_ms_range"] = [round(lo, 4), round(hi, 4)]
        r[f"{name}_ms_per_frame"] = round(med / B, 4)
        r[f"{name}_tbps"] = round(rows * N * per / 1e9 / med, 3)          # GB / ms = TB / s
    r["ratio_to_joint_stats"] = round(r["step_ms"] / r["joint_stats_ms"], 3)
    return r


def measure(B, G, radius, floor, warmup, reps, dev, net):
    N = G ** 3
    r = {"batch": B, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor,
         "volume_mb": round(B * JOINTS * N * 4 / 1e6, 1), "model_bytes_per_voxel": MODEL_BYTES}
    if net is None:
        coord = op.build_coord_volume(G, 2.0).reshape(N, 3).contiguous().to(dev)
        vols, joints = bump_volumes(B, G, coord, dev, seed=B)
        r["bumps"] = measure_ops(vols, joints, coord, G, radius, floor, warmup, reps)
        return r
    img, depth = synth.make_inputs(77, B, "floor")
    img, depth = img.to(dev), depth.to(dev)

    def forward():
        return net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)

    with torch.no_grad():
        med, lo, hi = timed(forward, warmup, reps)
        kp, _, vols, _ = forward()
    r["forward_ms"], r["forward_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    coord = net.coord_volumes[0].reshape(N, 3).to(device=dev, dtype=torch.float32).contiguous()
    r["forward_volumes"] = measure_ops(vols, kp, coord, G, radius, floor, warmup, reps)
    r["step_share_of_forward"] = round(r["forward_volumes"]["step_ms"] / med, 5)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="bump volumes instead of the forward's (needed for a --grid other than the model's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_filter.py needs an MI355X (HIP device)")
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
        r = measure(B, args.grid, args.radius, args.floor, args.warmup, args.reps, dev, net)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
