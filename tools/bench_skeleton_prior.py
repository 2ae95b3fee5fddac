#!/usr/bin/env python3
"""Cost of the skeleton-coupled joints (se_skeleton_couple_f32; SkeletonPrior.couple) and of one shell correlation launch
(se_shell_correlate_f32) beside the joint statistics (se_joint_stats_f32) on the same volumes and beside the forward of the same
batch: B frames x 15 joints of G^3 voxels.

    python tools/bench_skeleton_prior.py [--batches 1 8 32] [--grid 64] [--tau 0.03] [--floor 1e-3] [--warmup 3] [--reps 20]
                                         [--no_forward] [--out result.json]

HIP events around one call, median of --reps after --warmup, the same call back to back.  The volumes are the softmaxed volumes the
network's own forward wrote for a synthetic batch, or, with --no_forward, Gaussian bumps.  The bone lengths are 14 values from 0.15 to
0.45 m, so at 64^3 and tau 0.03 the taps reach R = 18 voxels.  ``correlate``: one launch of se_shell_correlate_f32 over the 14 x B
volumes a level of the tree would hold at most, every edge with its own shell (the run table's small launch included).  The FMA and
LDS-read counts are the kernel's own (csrc/skeleton_prior.hip): every lane of a workgroup executes one fused multiply-add per
non-zero tap of every plane that lies inside the grid for its output plane, halo zeros included; a run of n taps costs 3 + 4 (n // 4)
LDS reads in groups of four (n >= 4) and 4 per tap of its tail.  The rate is set against the float32 vector peak of 157.3 TFLOP/s
(78.65 T FMA/s).  Prints one JSON line per batch size.
"""
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

from sceneego_amd import _lib, load_config, op, synth  # noqa: E402
from sceneego_amd.skeleton_prior import SkeletonPrior  # noqa: E402

JOINTS = 15
BONES = np.linspace(0.15, 0.45, JOINTS - 1)
PEAK_TFMA = 157.3 / 2.0
TILE_J, TILE_K = 16, 64           # csrc/skeleton_prior.hip: SK_TJ, SK_KC


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


def kernel_counts(block, G, R):
    """(fused multiply-adds, LDS reads) per lane-instruction count of one volume's correlation with the dense ``block``, as the
    kernel executes them: per lane, times the lanes of all workgroups."""
    W = 2 * R + 1
    w = np.asarray(block).reshape(W, W, W) != 0
    fma_plane = w.sum(axis=(1, 2)).astype(np.int64)                  # per di
    reads_plane = np.zeros(W, dtype=np.int64)
    for di in range(W):
        for dk in range(W):
            col = w[di, :, dk]
            n, runs = 0, []
            for v in col:                                            # maximal runs of non-zero taps along dj
                if v:
                    n += 1
                elif n:
                    runs.append(n)
                    n = 0
            if n:
                runs.append(n)
            for k, n in enumerate(runs):
                first_or_last = k == 0 or k == len(runs) - 1
                g = n // 4 if first_or_last else 0                   # a run between the first and the last goes tap by tap
                reads_plane[di] += (3 + 4 * g if g else 0) + 4 * (n - 4 * g)
    planes = np.zeros(W, dtype=np.int64)                             # for how many output planes i the plane di lies inside the grid
    for di in range(-R, R + 1):
        planes[di + R] = max(0, G - abs(di))
    lanes = -(-G // TILE_J) * TILE_J * -(-G // TILE_K) * TILE_K // 4  # lanes per output plane: four outputs each
    return int(4 * lanes * (fma_plane * planes).sum()), int(lanes * (reads_plane * planes).sum())


def bump_volumes(B, G, coord, dev, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    ax = torch.arange(G, dtype=torch.float64)
    rows = B * JOINTS
    logits = torch.empty((rows, G, G, G), dtype=torch.float32)
    for r in range(rows):
        c = torch.rand(3, generator=gen, dtype=torch.float64) * (G - 2) + 0.5
        w = float(torch.rand(1, generator=gen)) * 2.0 + 1.0
        g = [torch.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
        logits[r] = (12.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).float()
    logits = logits.reshape(rows, G ** 3).to(dev)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=dev)
    _lib.softargmax3d(logits, coord, prob, joints, rows, G ** 3, 1)
    return prob.view(B, JOINTS, G, G, G), joints.view(B, JOINTS, 3)


def measure_ops(vols, joints, coord, G, side, tau, floor, warmup, reps):
    B, J = vols.shape[:2]
    rows, N = B * J, G ** 3
    dev = vols.device
    flat, kp = vols.reshape(rows, N).contiguous(), joints.reshape(rows, 3).contiguous()
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev)
    idx = torch.empty((rows,), device=dev, dtype=torch.int32)
    ws_js = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev)
    sp = SkeletonPrior(coord, G, side, BONES, tau=tau, floor=floor)
    R = sp.radius
    out = sp.couple(vols)
    taps = sp._dev["taps"]
    # one correlation launch over the volumes of joints 1..14 of every frame, each with its own edge's shell
    edge_rows = (J - 1) * B
    a = vols[:, 1:].reshape(edge_rows, N).contiguous()
    tap_row = torch.arange(1, J, device=dev, dtype=torch.int32).repeat(B)
    s = torch.ones(edge_rows, device=dev)
    corr_out = torch.empty_like(a)
    ws_c = torch.empty(_lib.shell_correlate_scratch_bytes(J, R), device=dev, dtype=torch.uint8)

    def joint_stats():
        _lib.joint_stats(flat, coord, kp, stats, idx, rows, N, scratch=ws_js)

    def couple():
        sp.couple(vols)

    def couple_beliefs():
        sp.couple(vols, return_beliefs=True)

    def correlate():
        _lib.shell_correlate(a, taps, tap_row, s, corr_out, edge_rows, G, R, 1.0 - floor, floor / N, scratch=ws_c)

    r = {"radius": R, "coupled_frames": int(out["coupled"].sum())}
    med, lo, hi = timed(joint_stats, warmup, reps)
    r["joint_stats_ms"], r["joint_stats_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    for name, fn in (("couple", couple), ("couple_beliefs", couple_beliefs), ("correlate", correlate)):
        med, lo, hi = timed(fn, warmup, reps)
        r[f"{name}_ms"] = round(med, 4)
        r[f"{name}_ms_range"] = [round(lo, 4), round(hi, 4)]
    r["couple_ms_per_frame"] = round(r["couple_ms"] / B, 4)
    counts = [kernel_counts(sp.taps[j], G, R) for j in range(1, J)]
    fma, reads = sum(c[0] for c in counts), sum(c[1] for c in counts)             # one frame's 14 edges, one direction
    r["taps_per_edge"] = [int(np.count_nonzero(sp.taps[j])) for j in range(1, J)]
    r["correlate_gfma"] = round(B * fma / 1e9, 3)
    r["correlate_tfma_per_s"] = round(B * fma / 1e9 / r["correlate_ms"], 3)       # G FMA / ms = T FMA / s
    r["correlate_share_of_fp32_peak"] = round(r["correlate_tfma_per_s"] / PEAK_TFMA, 4)
    r["lds_reads_per_fma"] = round(reads / fma, 4)
    r["couple_tfma_per_s"] = round(2 * B * fma / 1e9 / r["couple_ms"], 3)         # both directions; the other launches ride along
    r["ratio_to_joint_stats"] = round(r["couple_ms"] / r["joint_stats_ms"], 2)
    return r


def measure(B, G, tau, floor, warmup, reps, dev, net):
    N = G ** 3
    r = {"batch": B, "grid": G, "joints": JOINTS, "tau": tau, "floor": floor, "volume_mb": round(B * JOINTS * N * 4 / 1e6, 1)}
    if net is None:
        coord = op.build_coord_volume(G, 2.0).reshape(N, 3).contiguous().to(dev)
        vols, joints = bump_volumes(B, G, coord, dev, seed=B)
        r["bumps"] = measure_ops(vols, joints, coord, G, 2.0, tau, floor, warmup, reps)
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
    r["forward_volumes"] = measure_ops(vols, kp, coord, G, float(net.cuboid_side), tau, floor, warmup, reps)
    r["couple_share_of_forward"] = round(r["forward_volumes"]["couple_ms"] / med, 4)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_forward", action="store_true", help="bump volumes instead of the forward's (needed for a --grid other than the model's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_prior.py needs an MI355X (HIP device)")
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
        r = measure(B, args.grid, args.tau, args.floor, args.warmup, args.reps, dev, net)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
