#!/usr/bin/env python3
"""Cost of one EM iteration of the motion-model fit (MotionModelFit.fit: se_volume_filter_f32, then se_volume_transition_stats_f32,
over the stored frames) per frame, the forward pass and the statistics pass apart, beside VolumeSmoother.push + finish on the same
volumes.

    python tools/bench_motion_fit.py [--frames 8 32] [--grid 64] [--radius 10] [--floor 1e-3] [--batch 8] [--warmup 3] [--reps 20]
                                     [--out result.json]

The track is that of tools/bench_volume_smoother.py: T frames of 15 rows of G^3 voxels (Gaussian bumps that take a random walk,
softmaxed on the device), in pushes of --batch.  The two passes are called as fit() calls them, at the _lib level on a stored track
(per push one call, the statistics last push first), between HIP events; median of --reps after --warmup.  ``fit_ms_per_iteration`` is
a whole ``fit(iterations=1)`` by the host's clock: two forward passes, one statistics pass, the copies of the sums to the host and the
float64 M-step.  TB/s is the kernel's byte model (csrc/volume_filter.hip: 40 B per frame, row and voxel for the statistics, 32 B for
the forward pass with the beliefs kept).  Prints one JSON line per T.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_volume_smoother import JOINTS, SIDE, events, timed_pair, walking_bumps  # noqa: E402
from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.motion_fit import MotionModelFit  # noqa: E402
from sceneego_amd.volume_smoother import VolumeSmoother  # noqa: E402

STATS_BYTES = 40            # per frame, row and voxel (csrc/volume_filter.hip: BYTE MODEL of the transition statistics)
FORWARD_BYTES = 32          # the filter's 28 B and the beliefs written


def measure(T, G, radius, floor, batch, warmup, reps, dev):
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols = walking_bumps(T, G, coord, dev, seed=T)
    kw = {"sigma": radius * (SIDE / G) / 3.0, "radius": radius, "floor": floor}
    cuts = [(i, min(i + batch, T)) for i in range(0, T, batch)]
    r = {"frames": T, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor, "push_batch": batch,
         "stored_mb": round(2 * T * JOINTS * N * 4 / 1e6, 1)}
    fit = MotionModelFit(coord, G, SIDE, **kw)
    for a, b in cuts:
        fit.push(vols[a:b])
    f = fit.filter
    ws = fit._workspace(dev, JOINTS, T)
    fd = f._device_constants(dev, JOINTS)
    taps, ones = fd["taps"], fd["ones"]
    pushes = fit._pushes

    def iteration():
        e = events(3)
        e[0].record()
        t0 = 0
        for i, p in enumerate(pushes):
            B = int(p.volumes.shape[0])
            _lib.volume_filter(p.volumes, fd["coord"], taps, ws["state"], p.beliefs, ws["joints"][t0:t0 + B], ws["evidence"][t0:t0 + B],
                               p.restarted, B, JOINTS, N, G, radius, floor, have_prior=None if i == 0 else ones, scratch=ws["scratch"])
            t0 += B
        e[1].record()
        t1 = T
        for i in range(len(pushes) - 1, -1, -1):
            p = pushes[i]
            B = int(p.volumes.shape[0])
            link = None if i == len(pushes) - 1 else (pushes[i + 1].restarted[0] == 0).to(torch.int32)
            _lib.volume_transition_stats(p.volumes, p.beliefs, p.restarted, taps, ws["state"], ws["stats"][t1 - B:t1],
                                         ws["linked"][t1 - B:t1], B, JOINTS, N, G, radius, floor, have_link=link, scratch=ws["scratch"])
            t1 -= B
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    (f_ms, f_lo, f_hi), (s_ms, s_lo, s_hi) = timed_pair(iteration, warmup, reps)
    r["forward_ms_per_frame"], r["forward_ms_range"] = round(f_ms / T, 4), [round(f_lo / T, 4), round(f_hi / T, 4)]
    r["stats_ms_per_frame"], r["stats_ms_range"] = round(s_ms / T, 4), [round(s_lo / T, 4), round(s_hi / T, 4)]
    r["forward_tbps"] = round(T * JOINTS * N * FORWARD_BYTES / 1e9 / f_ms, 3)            # GB / ms = TB / s
    r["stats_tbps"] = round(T * JOINTS * N * STATS_BYTES / 1e9 / s_ms, 3)

    host = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fit.fit(iterations=1)
        torch.cuda.synchronize()
        if i >= warmup:
            host.append((time.perf_counter() - t) * 1e3)
    r["fit_ms_per_iteration"] = round(statistics.median(host), 3)
    r["fitted_sigma"], r["fitted_floor"] = res["sigma"], res["floor"]
    r["log_likelihood"] = res["log_likelihood"]

    sm = VolumeSmoother(coord, G, SIDE, **kw)

    def smoother_track():
        sm.reset()
        e = events(3)
        e[0].record()
        for a, b in cuts:
            sm.push(vols[a:b])
        e[1].record()
        sm.finish()
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    (p_ms, p_lo, p_hi), (b_ms, b_lo, b_hi) = timed_pair(smoother_track, warmup, reps)
    r["smoother_push_ms_per_frame"], r["smoother_push_ms_range"] = round(p_ms / T, 4), [round(p_lo / T, 4), round(p_hi / T, 4)]
    r["smoother_finish_ms_per_frame"], r["smoother_finish_ms_range"] = round(b_ms / T, 4), [round(b_lo / T, 4), round(b_hi / T, 4)]
    r["stats_over_finish"] = round(r["stats_ms_per_frame"] / r["smoother_finish_ms_per_frame"], 3)
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
        raise SystemExit("bench_motion_fit.py needs an MI355X (HIP device)")
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
