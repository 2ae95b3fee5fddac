#!/usr/bin/env python3
"""Cost of the most probable pose (se_skeleton_pose_f32; SkeletonPose.solve) and of one max-correlation launch (se_shell_maxcorr_f32)
beside the skeleton-coupled joints (SkeletonPrior.couple) and one sum-correlation launch (se_shell_correlate_f32) on the same volumes,
taps and batch: B frames x 15 joints of G^3 voxels.

    python tools/bench_skeleton_pose.py [--batches 1 8 32] [--grid 64] [--tau 0.03] [--floor 1e-3] [--warmup 3] [--reps 20]
                                        [--torch] [--out result.json]

HIP events around one call, median, minimum and maximum of --reps after --warmup, the same call back to back; ``solve`` and ``couple``
alternate inside one process.  The volumes are softmaxed Gaussian bumps (tools/bench_skeleton_prior.py: bump_volumes), the bone lengths
its 14 values from 0.15 to 0.45 m, so at 64^3 and tau 0.03 the taps reach R = 18 voxels for both.  ``maxcorr`` / ``correlate``: one
launch over the 14 x B volumes a level of the tree would hold at most, every edge with its own shell (the run table's small launch
included).  Per tap and output the max form executes one multiply and half a three-operand maximum where the sum form executes one
fused multiply-add (csrc/skeleton_pose.hip); the tap and LDS-read counts are those of tools/bench_skeleton_prior.py: kernel_counts.
``--torch``: the same upward recursion at B = 1 in plain torch - per non-zero tap one shifted product and one torch.maximum over the
volume, ldexp and where around them - timed once after one warm correlation, and its log score compared with the kernel's.
Prints one JSON line per batch size.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_skeleton_prior import BONES, JOINTS, bump_volumes, kernel_counts, timed  # noqa: E402
from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.skeleton_pose import SkeletonPose  # noqa: E402
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior  # noqa: E402

SIDE = 2.0


def torch_shell_max(s, block, G, R):
    """max over the non-zero taps of s(x + d) w(d) by shifted products: s [G, G, G] on the device, block [(2R+1)^3] numpy."""
    W = 2 * R + 1
    pad = torch.nn.functional.pad(s, (R, R, R, R, R, R))
    best = torch.zeros_like(s)
    for tap in np.flatnonzero(block):
        di, dj, dk = int(tap // (W * W)), int(tap // W % W), int(tap % W)
        best = torch.maximum(best, pad[di:di + G, dj:dj + G, dk:dk + G] * float(block[tap]))
    return best


def torch_recursion(vols, taps, parents, G, R, floor):
    """The upward pass of one frame in plain torch: (seconds, log score, taps walked)."""
    J, N = len(parents), G ** 3
    keep, uniform = 1.0 - floor, floor / N
    kids = [[c for c in range(1, J) if parents[c] == j] for j in range(J)]
    warm = np.zeros_like(taps[1])
    warm[np.flatnonzero(taps[1])[:50]] = 1.0
    torch_shell_max(vols[1], warm, G, R)                                 # warm: the kernels of one short correlation
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m, log2 = [None] * J, 0
    walked = 0
    for j in range(J - 1, -1, -1):
        A = vols[j]
        for c in kids[j]:
            A = A * m[c]
        M = A.max()
        e = int(math.floor(math.log2(float(M))))
        log2 += e
        s = torch.ldexp(A, torch.tensor(-e, device=A.device))
        if j > 0:
            step = keep * torch_shell_max(s, taps[j], G, R)
            jump = uniform * s.max()
            m[j] = torch.where(jump > step, jump, step)
            walked += int(np.count_nonzero(taps[j]))
    best = float(s.max())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, math.log(best) + math.log(2.0) * log2, walked


def measure(B, G, tau, floor, warmup, reps, dev, with_torch):
    N, J = G ** 3, JOINTS
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols, joints = bump_volumes(B, G, coord, dev, seed=B)
    pose = SkeletonPose(coord, G, SIDE, BONES, tau=tau, floor=floor)
    prior = SkeletonPrior(coord, G, SIDE, BONES, tau=tau, floor=floor)
    R = pose.radius
    first = pose.solve(vols)
    prior.couple(vols)
    taps = prior._device_state(dev)["taps"]
    edge_rows = (J - 1) * B
    a = vols[:, 1:].reshape(edge_rows, N).contiguous()
    tap_row = torch.arange(1, J, device=dev, dtype=torch.int32).repeat(B)
    s = torch.ones(edge_rows, device=dev)
    out = torch.empty_like(a)
    ws = torch.empty(_lib.shell_correlate_scratch_bytes(J, R), device=dev, dtype=torch.uint8)
    fns = {"solve": lambda: pose.solve(vols), "couple": lambda: prior.couple(vols),
           "maxcorr": lambda: _lib.shell_maxcorr(a, taps, tap_row, out, edge_rows, G, R, 1.0 - floor, scratch=ws),
           "correlate": lambda: _lib.shell_correlate(a, taps, tap_row, s, out, edge_rows, G, R, 1.0 - floor, floor / N, scratch=ws)}
    r = {"batch": B, "grid": G, "joints": J, "tau": tau, "floor": floor, "radius": R, "volume_mb": round(B * J * N * 4 / 1e6, 1),
         "solved_frames": int(first["solved"].sum()), "jumps": int(first["jumped"].sum())}
    for half in (0, 1):                                                  # solve and couple alternate: two windows each, both reported
        for name in ("solve", "couple", "maxcorr", "correlate"):
            med, lo, hi = timed(fns[name], warmup, reps)
            r.setdefault(f"{name}_ms", []).append(round(med, 4))
            r.setdefault(f"{name}_ms_range", []).append([round(lo, 4), round(hi, 4)])
    for name in ("solve", "couple"):
        r[f"{name}_ms_per_frame"] = round(min(r[f"{name}_ms"]) / B, 4)
    r["solve_over_couple"] = round(min(r["solve_ms"]) / min(r["couple_ms"]), 3)
    r["maxcorr_ms_per_volume"] = round(min(r["maxcorr_ms"]) / edge_rows, 4)
    r["correlate_ms_per_volume"] = round(min(r["correlate_ms"]) / edge_rows, 4)
    counts = [kernel_counts(pose.taps[j], G, R) for j in range(1, J)]
    taps_exec, reads = sum(c[0] for c in counts), sum(c[1] for c in counts)      # one frame's 14 edges
    r["taps_per_edge"] = [int(np.count_nonzero(pose.taps[j])) for j in range(1, J)]
    r["maxcorr_gtap"] = round(B * taps_exec / 1e9, 3)
    r["maxcorr_ttap_per_s"] = round(B * taps_exec / 1e9 / min(r["maxcorr_ms"]), 3)          # G taps / ms = T taps / s
    r["correlate_tfma_per_s"] = round(B * taps_exec / 1e9 / min(r["correlate_ms"]), 3)
    r["lds_reads_per_tap"] = round(reads / taps_exec, 4)
    if with_torch and B == 1:
        sec, score, walked = torch_recursion(vols[0].reshape(J, G, G, G), pose.taps, KINEMATIC_PARENTS, G, R, floor)
        r["torch_recursion_s"], r["torch_taps_walked"] = round(sec, 3), walked
        r["torch_log_score"], r["log_score"] = round(score, 6), round(float(first["log_score"][0]), 6)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch", action="store_true", help="also time the same recursion in plain torch at B = 1 (seconds)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_pose.py needs an MI355X (HIP device)")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda")
    results = []
    for B in args.batches:
        r = measure(B, args.grid, args.tau, args.floor, args.warmup, args.reps, dev, args.torch)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
