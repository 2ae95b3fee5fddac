#!/usr/bin/env python3
"""Cost of the joint statistics (se_joint_stats_f32) beside the two-pass soft-argmax it follows (se_softargmax3d_f32, mode 1) on the
same shape: B x 15 rows of G^3 voxels.

    python tools/bench_joint_stats.py [--batches 1 8 32] [--grid 64] [--warmup 3] [--reps 20] [--step_ms B=ms ...] [--out result.json]

HIP events around one call, median of --reps after --warmup.  Two cache states per operator:
  after:  each timed statistics call directly follows a soft-argmax call on the same buffers (and each timed soft-argmax a statistics
          call): the state the forward leaves - the finish pass has just written the volumes, what fits is still in the 256 MB MALL;
  loop:   the same call back to back (its own previous pass is what the caches hold).
GB/s is the volume read once (rows * G^3 * 4 B) over the time, for both operators (the soft-argmax really moves three times that:
two reads and one write).  --step_ms 8=10.4 adds the share of a forward step of that batch size (bench.py's ms_per_step).
Prints one JSON line per batch size.
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

from sceneego_amd import _lib, op  # noqa: E402

JOINTS = 15


def timed(fn, before, warmup, reps):
    """Median milliseconds of fn(); ``before`` (or nothing) runs untimed ahead of every call."""
    ms = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def measure(B, G, warmup, reps, dev):
    rows, N = B * JOINTS, G ** 3
    coord = op.build_coord_volume(G, 2.0).reshape(N, 3).contiguous().to(dev)
    gen = torch.Generator(device=dev).manual_seed(B)
    logits = torch.randn((rows, N), device=dev, generator=gen) * 7.0
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=dev)
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev)
    idx = torch.empty((rows,), device=dev, dtype=torch.int32)
    ws_sa = torch.empty(_lib.softargmax3d_scratch_elems(rows), device=dev)
    ws_js = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev)

    def softargmax():
        _lib.softargmax3d(logits, coord, prob, joints, rows, N, 1, scratch=ws_sa)

    def joint_stats():
        _lib.joint_stats(prob, coord, joints, stats, idx, rows, N, scratch=ws_js)

    softargmax()
    mb = rows * N * 4 / 1e6
    r = {"batch": B, "grid": G, "rows": rows, "volume_mb": round(mb, 1)}
    for name, fn, other in (("joint_stats", joint_stats, softargmax), ("softargmax", softargmax, joint_stats)):
        for state, before in (("after", other), ("loop", None)):
            med, lo, hi = timed(fn, before, warmup, reps)
            r[f"{name}_{state}_ms"] = round(med, 4)
            r[f"{name}_{state}_ms_range"] = [round(lo, 4), round(hi, 4)]
            r[f"{name}_{state}_gbps"] = round(mb / med, 1)          # MB / ms = GB / s
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step_ms", nargs="*", default=[], help="B=ms: bench.py's ms_per_step at that batch size")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_joint_stats.py needs an MI355X (HIP device)")
    step = {int(k): float(v) for k, v in (s.split("=") for s in args.step_ms)}
    results = []
    for B in args.batches:
        r = measure(B, args.grid, args.warmup, args.reps, torch.device("cuda"))
        if B in step:
            r["step_ms"] = step[B]
            r["joint_stats_share_of_step"] = round(r["joint_stats_after_ms"] / step[B], 5)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
