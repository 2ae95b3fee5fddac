#!/usr/bin/env python3
"""Cost of the trajectory sampler (se_volume_sample_f32; VolumeSmoother.sample) over a recorded track, beside VolumeSmoother.finish on
the same stored frames.

    python tools/bench_volume_sampler.py [--frames 8 32] [--samples 1 16 64] [--grid 64] [--radius 10] [--floor 1e-3] [--batch 8]
                                         [--warmup 3] [--reps 20] [--out result.json]

The track is that of tools/bench_volume_smoother.py: T frames of 15 rows of G^3 voxels (Gaussian bumps that take a random walk,
softmaxed on the device), pushed in batches of --batch.  Every repetition is a whole track (reset, pushes, sample, finish) with HIP
events around sample() and around finish(); median of --reps after --warmup.  ``sample_ms`` is the whole call: per push the two
launches (the sums of every frame, then one workgroup per (sample, row) that walks the push's frames inside the launch) and behind
them the gather of the coordinates, the mean and the spread in torch.  ``kernel_ms`` is the launches alone (``_lib.volume_sample`` over
the same pushes).  ``finish_ms`` is the smoother's backward pass without the beliefs, on the same frames.  Prints one JSON line per
(T, S).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_volume_smoother import JOINTS, SIDE, events, timed_pair, walking_bumps  # noqa: E402

from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.volume_smoother import VolumeSmoother  # noqa: E402


def measure(T, S, vols, coord, G, radius, floor, batch, warmup, reps):
    N = G ** 3
    h = SIDE / G
    sm = VolumeSmoother(coord, G, SIDE, sigma=radius * h / 3.0, radius=radius, floor=floor)
    cuts = [(i, min(i + batch, T)) for i in range(0, T, batch)]
    last = {}

    def track():
        sm.reset()
        for a, b in cuts:
            sm.push(vols[a:b])
        e = events(3)
        e[0].record()
        last["sample"] = sm.sample(samples=S, seed=0)
        e[1].record()
        sm.finish()
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    (s_ms, s_lo, s_hi), (f_ms, f_lo, f_hi) = timed_pair(track, warmup, reps)
    # the launches alone, on the stored frames of one more track
    sm.reset()
    for a, b in cuts:
        sm.push(vols[a:b])
    pushes, fd, f = list(sm._pushes), sm.filter._dev, sm.filter
    dev = vols.device
    nxt = torch.empty((S, JOINTS), device=dev, dtype=torch.int32)
    out = [(torch.empty((S, b - a, JOINTS), device=dev, dtype=torch.int32), torch.empty((S, b - a, JOINTS), device=dev, dtype=torch.int32))
           for a, b in cuts]
    ws = [torch.empty(_lib.volume_sample_scratch_bytes(b - a, JOINTS, G), device=dev, dtype=torch.uint8) for a, b in cuts]

    def kernels():
        e = events(2)
        e[0].record()
        for i in range(len(cuts) - 1, -1, -1):
            link = None if i == len(cuts) - 1 else (pushes[i + 1].restarted[0] == 0).to(torch.int32)
            _lib.volume_sample(pushes[i].beliefs, pushes[i].restarted, fd["taps"], nxt, out[i][0], out[i][1], cuts[i][1] - cuts[i][0],
                               JOINTS, N, G, f.radius, f.floor, S, first_frame=cuts[i][0], seed=0, have_link=link, scratch=ws[i])
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]), 0.0

    (k_ms, k_lo, k_hi), _ = timed_pair(kernels, warmup, reps)
    sm.reset()
    res = last["sample"]
    return {"frames": T, "samples": S, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor, "push_batch": batch,
            "sample_ms": round(s_ms, 4), "sample_ms_range": [round(s_lo, 4), round(s_hi, 4)],
            "kernel_ms": round(k_ms, 4), "kernel_ms_range": [round(k_lo, 4), round(k_hi, 4)],
            "finish_ms": round(f_ms, 4), "finish_ms_range": [round(f_lo, 4), round(f_hi, 4)],
            "sample_over_finish": round(s_ms / f_ms, 3), "kernel_ms_per_frame": round(k_ms / T, 4),
            "valid_share": float(res["valid"].float().mean()), "jump_share": float((res["kind"] == _lib.SAMPLE_JUMP).float().mean()),
            "mean_spread_m": float(res["spread"][torch.isfinite(res["spread"])].mean()) if S > 1 else None}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=8, help="frames per push")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_sampler.py needs an MI355X (HIP device)")
    if args.reps < 1 or args.warmup < 0 or min(args.samples) < 1:
        raise SystemExit("--reps and every --samples must be at least 1 and --warmup at least 0")
    dev = torch.device("cuda")
    G = args.grid
    coord = op.build_coord_volume(G, SIDE).reshape(G ** 3, 3).contiguous().to(dev)
    results = []
    for T in args.frames:
        vols = walking_bumps(T, G, coord, dev, seed=T)
        for S in args.samples:
            r = measure(T, S, vols, coord, G, args.radius, args.floor, args.batch, args.warmup, args.reps)
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
