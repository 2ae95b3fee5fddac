#!/usr/bin/env python3
"""Cost of the forward-backward smoother (se_volume_smooth_f32; VolumeSmoother.push / finish) per frame of a recorded track, beside
VolumeFilter.step on the same volumes and beside the same backward pass written in plain torch on the same device.

    python tools/bench_volume_smoother.py [--frames 8 32] [--grid 64] [--radius 10] [--floor 1e-3] [--batch 8] [--warmup 3]
                                          [--reps 20] [--out result.json]

The track is T frames of 15 rows of G^3 voxels (Gaussian bumps that take a random walk, softmaxed on the device), pushed in batches of
--batch.  HIP events around the T / batch pushes and around finish(), median of --reps after --warmup; every repetition is a whole
track (reset, pushes, finish), so the first frame of every track is a restart as in use.  ``filter_ms`` is VolumeFilter.step
(return_beliefs=True, as push calls it) over the same batches: push minus that is the smoother's copies.  ``torch_ms`` is the backward
pass of the definition in plain torch on the device: three conv1d's per frame (the separable blur, the rows as channels' batch), the
floor, two products, two sums, two divisions and the expectation, float32, on the beliefs the filter wrote; it is compared with
``finish`` and checked against it (the largest difference of the joints is printed).  TB/s is the kernel's byte model
(csrc/volume_filter.hip: 32 B per frame, row and voxel, 44 B with the smoothed beliefs).  Prints one JSON line per T.
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

from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.volume_filter import VolumeFilter  # noqa: E402
from sceneego_amd.volume_smoother import VolumeSmoother  # noqa: E402

JOINTS = 15
SIDE = 2.0
MODEL_BYTES = 32            # per frame, row and voxel (csrc/volume_filter.hip: BYTE MODEL of the smoother); + 12 with the beliefs


def timed_pair(fn, warmup, reps):
    """fn() -> (ms of its first part, ms of its second part); the medians, minima and maxima of both."""
    a, b = [], []
    for i in range(warmup + reps):
        x, y = fn()
        if i >= warmup:
            a.append(x)
            b.append(y)
    return [(statistics.median(v), min(v), max(v)) for v in (a, b)]


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def walking_bumps(T, G, coord, dev, seed):
    """[T, 15, G, G, G] softmaxed volumes: per row a bump of 1-3 voxels x G / 32 that walks at most 2 voxels per axis and frame."""
    rng = np.random.default_rng(seed)
    ax = torch.arange(G, dtype=torch.float64)
    logits = torch.empty((T, JOINTS, G, G, G), dtype=torch.float32)
    for r in range(JOINTS):
        c = rng.uniform(4, G - 5, size=3)
        w = max(1.0, G / 32.0) * rng.uniform(1.0, 3.0)
        for t in range(T):
            c = np.clip(c + rng.uniform(-2, 2, size=3), 0.5, G - 1.5)
            g = [torch.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
            v = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
            logits[t, r] = ((v - v.mean()) / v.std() * 7.0).float()
    logits = logits.reshape(T * JOINTS, G ** 3).to(dev)
    prob = torch.empty_like(logits)
    joints = torch.empty((T * JOINTS, 3), device=dev)
    _lib.softargmax3d(logits, coord, prob, joints, T * JOINTS, G ** 3, 1)
    return prob.view(T, JOINTS, G, G, G)


def torch_backward(vols, beliefs, restarted, coord, taps, floor):
    """The definition in plain torch, float32: joints [T, J, 3] of the smoothed beliefs (nothing else is kept)."""
    T, J, G = vols.shape[:3]
    N = G ** 3
    R = (taps.numel() - 1) // 2
    w = taps.flip(0).view(1, 1, -1)                      # conv1d is a correlation: the reversed taps, as the kernel uses them
    keep, uniform = 1.0 - floor, floor / N
    joints = torch.empty((T, J, 3), device=vols.device)
    r = None
    for t in range(T - 1, -1, -1):
        p, b = vols[t].reshape(J, N), beliefs[t].reshape(J, N)
        gamma, new_r = b, p
        if t < T - 1:
            u = r.view(J, G, G, G)
            for axis in (3, 2, 1):
                u = u.movedim(axis, 3)
                shape = u.shape
                u = torch.nn.functional.conv1d(u.reshape(-1, 1, G), w, padding=R).view(shape).movedim(3, axis)
            u = u.reshape(J, N) * keep + uniform
            g, a = b * u, p * u
            S, s = g.sum(dim=1, keepdim=True), a.sum(dim=1, keepdim=True)
            linked = (restarted[t + 1] == 0).view(J, 1)
            gamma = torch.where(linked & (S > 0) & torch.isfinite(S), g / S, b)
            new_r = torch.where(linked & (s > 0) & torch.isfinite(s), a / s, p)
        r = new_r
        joints[t] = gamma @ coord
    return joints


def measure(T, G, radius, floor, batch, warmup, reps, dev):
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols = walking_bumps(T, G, coord, dev, seed=T)
    h = SIDE / G
    kw = {"sigma": radius * h / 3.0, "radius": radius, "floor": floor}
    cuts = [(i, min(i + batch, T)) for i in range(0, T, batch)]
    r = {"frames": T, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor, "push_batch": batch,
         "stored_mb": round(2 * T * JOINTS * N * 4 / 1e6, 1), "model_bytes_per_voxel": MODEL_BYTES}
    filt = VolumeFilter(coord, G, SIDE, **kw)
    sm = VolumeSmoother(coord, G, SIDE, **kw)
    last = {}

    def filter_track():
        filt.reset()
        e = events(2)
        e[0].record()
        parts = [filt.step(vols[a:b], return_beliefs=True) for a, b in cuts]
        e[1].record()
        e[1].synchronize()
        last["filter"] = parts
        return e[0].elapsed_time(e[1]), 0.0

    def smoother_track(beliefs):
        def run():
            sm.reset()
            e = events(3)
            e[0].record()
            for a, b in cuts:
                sm.push(vols[a:b])
            e[1].record()
            last["smooth"] = sm.finish(return_beliefs=beliefs)
            e[2].record()
            e[2].synchronize()
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
        return run

    (f_ms, f_lo, f_hi), _ = timed_pair(filter_track, warmup, reps)
    r["filter_ms_per_frame"], r["filter_ms_range"] = round(f_ms / T, 4), [round(f_lo / T, 4), round(f_hi / T, 4)]
    for name, beliefs, per in (("finish", False, MODEL_BYTES), ("finish_beliefs", True, MODEL_BYTES + 12)):
        (p_ms, p_lo, p_hi), (b_ms, b_lo, b_hi) = timed_pair(smoother_track(beliefs), warmup, reps)
        if not beliefs:
            r["push_ms_per_frame"], r["push_ms_range"] = round(p_ms / T, 4), [round(p_lo / T, 4), round(p_hi / T, 4)]
        r[f"{name}_ms_per_frame"], r[f"{name}_ms_range"] = round(b_ms / T, 4), [round(b_lo / T, 4), round(b_hi / T, 4)]
        r[f"{name}_tbps"] = round(T * JOINTS * N * per / 1e9 / b_ms, 3)            # GB / ms = TB / s
    sm.reset()
    for a, b in cuts:
        sm.push(vols[a:b])
    kernel_joints = sm.finish()["joints"]
    beliefs = torch.cat([p["beliefs"] for p in last["filter"]])
    restarted = torch.cat([p["restarted"] for p in last["filter"]]).to(torch.int32)
    taps = torch.from_numpy(filt.taps).to(dev)

    def torch_track():
        e = events(2)
        e[0].record()
        last["torch"] = torch_backward(vols, beliefs, restarted, coord, taps, float(np.float32(floor)))
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]), 0.0

    (t_ms, t_lo, t_hi), _ = timed_pair(torch_track, warmup, reps)
    r["torch_ms_per_frame"], r["torch_ms_range"] = round(t_ms / T, 4), [round(t_lo / T, 4), round(t_hi / T, 4)]
    r["torch_over_finish"] = round(r["torch_ms_per_frame"] / r["finish_ms_per_frame"], 3)
    r["torch_vs_kernel_joints_max_abs_m"] = float((last["torch"] - kernel_joints).abs().max())
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=8, help="frames per push")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_smoother.py needs an MI355X (HIP device)")
    if args.reps < 1 or args.warmup < 0:
        raise SystemExit("--reps must be at least 1 and --warmup at least 0")
    dev = torch.device("cuda")
    results = []
    for T in args.frames:
        r = measure(T, args.grid, args.radius, args.floor, args.batch, args.warmup, args.reps, dev)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
