#!/usr/bin/env python3
"""Cost of the pose sampler (se_skeleton_upward_f32, se_skeleton_sample_f32; SkeletonPrior.sample) beside SkeletonPrior.couple and
SkeletonPose.solve on the same volumes: B frames x 15 joints of G^3 voxels.

    python tools/bench_skeleton_sampler.py [--batches 1 8 32] [--samples 1 16 64] [--grid 64] [--tau 0.03] [--floor 1e-3]
                                           [--warmup 3] [--reps 20] [--hashes] [--out result.json]

HIP events around one call, median of --reps after --warmup, the same call back to back, milliseconds PER CALL.  The volumes are
softmaxed Gaussian bumps (tools/bench_skeleton_prior.py: bump_volumes) and the bone lengths 14 values from 0.15 to 0.45 m, so at 64^3
and tau 0.03 the taps reach R = 18 voxels.  ``sample_ms`` is the whole SkeletonPrior.sample: per group of at most 8 frames the upward
call and the sampler's two launches, and behind them the gather of the coordinates, the mean, the spread and the bone errors in
torch.  ``upward_ms`` is _lib.skeleton_upward over the same groups and ``sums_and_walk_ms`` _lib.skeleton_sample on their output.
``sums_ms`` is that call over the same groups with every frame marked invalid - the sums pass runs, every workgroup of the walk
writes -1 and returns - and ``walk_ms`` the difference of the two medians.  ``couple_ms`` and ``solve_ms`` are measured in the same
run, before and after the sampler.  Every entry is [median, min, max].  Prints one JSON line per (B, S).

--hashes prints the SHA-256 of the outputs of one call each of couple, solve and VolumeSmoother.sample on fixed inputs (G = 16): the
same figures under two builds of the library say that their bits did not move.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_skeleton_prior import BONES, JOINTS, bump_volumes, timed  # noqa: E402

from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.skeleton_pose import SkeletonPose  # noqa: E402
from sceneego_amd.skeleton_prior import SAMPLE_GROUP, SkeletonPrior  # noqa: E402
from sceneego_amd.volume_smoother import VolumeSmoother  # noqa: E402

SIDE = 2.0


def measure(B, samples, vols, joints, coord, G, side, tau, floor, warmup, reps):
    dev, N, J = vols.device, G ** 3, JOINTS
    sp = SkeletonPrior(coord, G, side, BONES, tau=tau, floor=floor)
    pose = SkeletonPose(coord, G, side, BONES, tau=tau, floor=floor)
    R = sp.radius
    taps = sp._device_state(dev)["taps"]
    flat = vols.reshape(B, J, N).contiguous()
    groups = [(a, min(a + SAMPLE_GROUP, B)) for a in range(0, B, SAMPLE_GROUP)]
    n = min(B, SAMPLE_GROUP)
    A = torch.empty((B, J, N), device=dev)
    sums, valid = torch.empty((B, J), device=dev), torch.empty((B,), device=dev, dtype=torch.int32)
    ws_up = torch.empty(_lib.skeleton_upward_scratch_bytes(n, J, G, R), device=dev, dtype=torch.uint8)
    ws_sm = torch.empty(_lib.skeleton_sample_scratch_bytes(n, J, G) + 8, device=dev, dtype=torch.uint8)
    ws_sm = ws_sm[(-ws_sm.data_ptr()) % 8:]

    def upward():
        for a, b in groups:
            _lib.skeleton_upward(flat[a:b], taps, sp.parents, A[a:b], sums[a:b], valid[a:b], b - a, N, G, R, floor, scratch=ws_up)

    none = torch.zeros((B,), device=dev, dtype=torch.int32)

    def draws(S, flags=None):
        flags = valid if flags is None else flags
        out = [(torch.empty((S, b - a, J), device=dev, dtype=torch.int32), torch.empty((S, b - a, J), device=dev, dtype=torch.int32))
               for a, b in groups]

        def run():
            for (a, b), (idx, knd) in zip(groups, out):
                _lib.skeleton_sample(A[a:b], flags[a:b], taps, sp.parents, idx, knd, b - a, N, G, R, floor, S, first_frame=a,
                                     scratch=ws_sm)
        return run

    couple_a = timed(lambda: sp.couple(vols), warmup, reps)
    solve_a = timed(lambda: pose.solve(vols), warmup, reps)
    up = timed(upward, warmup, reps)
    sums_only = timed(draws(1, none), warmup, reps)
    results = []
    for S in samples:
        both = timed(draws(S), warmup, reps)
        last = {}

        def whole():
            last["r"] = sp.sample(vols, samples=S, seed=0, joints=joints)
        smp = timed(whole, warmup, reps)
        r = last["r"]
        results.append({"batch": B, "samples": S, "grid": G, "radius": R, "floor": floor,
                        "sample_ms": [round(v, 4) for v in smp], "upward_ms": [round(v, 4) for v in up],
                        "sums_and_walk_ms": [round(v, 4) for v in both], "sums_ms": [round(v, 4) for v in sums_only],
                        "walk_ms": round(both[0] - sums_only[0], 4),
                        "valid_share": float(r["valid"].float().mean()), "jump_share": float((r["kind"] == _lib.SAMPLE_JUMP).float().mean()),
                        "mean_spread_m": float(r["spread"][torch.isfinite(r["spread"])].mean()) if S > 1 else None,
                        "mean_bone_error_m": float(r["bone_error"][torch.isfinite(r["bone_error"])].mean())})
    couple_b = timed(lambda: sp.couple(vols), warmup, reps)
    solve_b = timed(lambda: pose.solve(vols), warmup, reps)
    for r in results:
        r["couple_ms"] = [round(couple_a[0], 4), round(couple_b[0], 4)]
        r["solve_ms"] = [round(solve_a[0], 4), round(solve_b[0], 4)]
        r["upward_over_couple"] = round(up[0] / couple_a[0], 3)
        r["sample_over_couple"] = round(r["sample_ms"][0] / couple_a[0], 3)
    return results


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()[:16]


def hashes():
    """One call each of couple, solve and VolumeSmoother.sample on fixed inputs at G = 16: the digests of their outputs."""
    dev, G, side = torch.device("cuda"), 16, 2.0
    coord = op.build_coord_volume(G, side).reshape(G ** 3, 3).contiguous().to(dev)
    vols, joints = bump_volumes(3, G, coord, dev, seed=7)
    bones = np.linspace(0.2, 0.55, JOINTS - 1)
    c = SkeletonPrior(coord, G, side, bones, tau=0.06, floor=1e-3).couple(vols, joints=joints, return_beliefs=True)
    s = SkeletonPose(coord, G, side, bones, tau=0.06, floor=1e-3).solve(vols, joints=joints)
    sm = VolumeSmoother(coord, G, side, sigma=0.15, radius=3, floor=1e-3)
    sm.push(vols, joints=joints)
    t = sm.sample(samples=8, seed=5)
    torch.cuda.synchronize()
    out = {"couple": digest(c["beliefs"], c["joints"], c["evidence"], c["coupled"]),
           "solve": digest(*[s[k] for k in sorted(s) if isinstance(s[k], torch.Tensor)]),
           "volume_sample": digest(t["index"], t["kind"], t["coord"], t["mean"], t["spread"]), "library": _lib.built_fingerprint()}
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hashes", action="store_true", help="print the digests of couple, solve and VolumeSmoother.sample and stop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_sampler.py needs an MI355X (HIP device)")
    if args.hashes:
        return hashes()
    if args.reps < 1 or args.warmup < 0 or min(args.samples) < 1 or min(args.batches) < 1:
        raise SystemExit("--reps, every --samples and every --batches must be at least 1 and --warmup at least 0")
    dev = torch.device("cuda")
    G = args.grid
    side = SIDE
    coord = op.build_coord_volume(G, side).reshape(G ** 3, 3).contiguous().to(dev)
    results = []
    for B in args.batches:
        vols, joints = bump_volumes(B, G, coord, dev, seed=B)
        rows = measure(B, args.samples, vols, joints, coord, G, side, args.tau, args.floor, args.warmup, args.reps)
        for r in rows:
            print(json.dumps(r), flush=True)
        results.extend(rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
