#!/usr/bin/env python3
"""Cost of the runner-up poses (se_skeleton_alternatives_f32; SkeletonPose.alternatives) beside the most probable pose
(SkeletonPose.solve) and the skeleton-coupled joints (SkeletonPrior.couple) on the same volumes, taps and batch: B frames x 15 joints of
G^3 voxels.

    python tools/bench_skeleton_alternatives.py [--batches 1 8 32] [--grid 64] [--tau 0.03] [--floor 1e-3] [--separation 2]
                                                [--warmup 3] [--reps 20] [--out result.json]

HIP events around one call, median, minimum and maximum of --reps after --warmup, the same call back to back; the calls alternate inside
one process, two windows each.  The volumes and bone lengths are those of tools/bench_skeleton_pose.py (R = 18 voxels at 64^3).
``alternatives``: the public call (the library call, the refinement of the J x J alternative poses and the float64 bookkeeping in
torch); ``alternatives_lib``: the library call alone; ``alternatives_volumes_lib``: the same writing the max-marginal volumes;
``no_walk_lib``: the library call with a window that covers the grid, so that no anchor has an alternative and every walk returns at
once - the difference to ``alternatives_lib`` is the share of the walks.  Prints one JSON line per batch size.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_skeleton_prior import BONES, JOINTS, bump_volumes, timed  # noqa: E402
from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.skeleton_pose import SkeletonPose  # noqa: E402
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior  # noqa: E402

SIDE = 2.0


def lib_call(pose, vols, taps, separation, volumes):
    """The library call on preallocated outputs: a closure for ``timed``."""
    B, J, N, dev = int(vols.shape[0]), pose.joints, pose.voxels, vols.device
    shape = {"solved": (B,), "complete": (B,), "best_root": (B,), "alt_pose": (B, J, J), "alt_jumped": (B, J, J)}
    ints = ("index", "jumped", "exponent", "solved", "down_exponent", "mm_peak", "alt_index", "alt_pose", "alt_jumped", "complete")
    out = {k: torch.empty(shape.get(k, (B, J)), device=dev, dtype=torch.int32) for k in ints}
    out.update({k: torch.empty(shape.get(k, (B, J)), device=dev) for k in ("best_root", "mm_best", "pose_value", "alt_value")})
    out["max_marginals"] = torch.empty((B, J, N), device=dev) if volumes else None
    ws = torch.empty(_lib.skeleton_alternatives_scratch_bytes(B, J, pose.grid, pose.radius), device=dev, dtype=torch.uint8)
    prob = vols.reshape(B, J, N)
    return out, lambda: _lib.skeleton_alternatives(prob, taps, KINEMATIC_PARENTS, separation, frames=B, voxels=N, grid=pose.grid,
                                                   radius=pose.radius, floor=pose.floor, scratch=ws, **out)


def measure(B, G, tau, floor, separation, warmup, reps, dev):
    N, J = G ** 3, JOINTS
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols, _ = bump_volumes(B, G, coord, dev, seed=B)
    pose = SkeletonPose(coord, G, SIDE, BONES, tau=tau, floor=floor)
    prior = SkeletonPrior(coord, G, SIDE, BONES, tau=tau, floor=floor)
    first = pose.alternatives(vols, separation=separation)
    prior.couple(vols)
    taps = prior._device_state(dev)["taps"]
    fns = {"alternatives": lambda: pose.alternatives(vols, separation=separation), "solve": lambda: pose.solve(vols),
           "couple": lambda: prior.couple(vols), "alternatives_lib": lib_call(pose, vols, taps, separation, False)[1],
           "alternatives_volumes_lib": lib_call(pose, vols, taps, separation, True)[1]}
    idle, fns["no_walk_lib"] = lib_call(pose, vols, taps, G - 1, False)
    fns["no_walk_lib"]()
    torch.cuda.synchronize()
    margins = first["runner_up_margin"]
    r = {"batch": B, "grid": G, "joints": J, "tau": tau, "floor": floor, "radius": pose.radius, "separation": separation,
         "volume_mb": round(B * J * N * 4 / 1e6, 1), "complete_frames": int(first["complete"].sum()),
         "alternatives_found": int((first["alt_index"] >= 0).sum()), "alternatives_of_no_walk": int((idle["alt_index"] >= 0).sum()),
         "mean_runner_up_margin": round(float(margins[torch.isfinite(margins)].mean()), 4),
         "scratch_mb": round(_lib.skeleton_alternatives_scratch_bytes(B, J, G, pose.radius) / 1e6, 1),
         "solve_scratch_mb": round(_lib.skeleton_pose_scratch_bytes(B, J, G, pose.radius) / 1e6, 1)}
    for half in (0, 1):                                                  # the calls alternate: two windows each, both reported
        for name in fns:
            med, lo, hi = timed(fns[name], warmup, reps)
            r.setdefault(f"{name}_ms", []).append(round(med, 4))
            r.setdefault(f"{name}_ms_range", []).append([round(lo, 4), round(hi, 4)])
    for name in fns:
        r[f"{name}_ms_per_frame"] = round(min(r[f"{name}_ms"]) / B, 4)
    lib = min(r["alternatives_lib_ms"])
    r["alternatives_lib_over_solve"] = round(lib / min(r["solve_ms"]), 3)
    r["alternatives_lib_over_couple"] = round(lib / min(r["couple_ms"]), 3)
    r["walk_ms"] = round(lib - min(r["no_walk_lib_ms"]), 4)
    r["walk_share"] = round(r["walk_ms"] / lib, 4)
    r["torch_side_ms"] = round(min(r["alternatives_ms"]) - lib, 4)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--separation", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_alternatives.py needs an MI355X (HIP device)")
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda")
    results = []
    for B in args.batches:
        r = measure(B, args.grid, args.tau, args.floor, args.separation, args.warmup, args.reps, dev)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
