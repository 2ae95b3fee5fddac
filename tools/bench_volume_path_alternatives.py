#!/usr/bin/env python3
"""Cost of the runner-up trajectories (se_volume_viterbi_keep_f32, se_volume_viterbi_back_f32, se_volume_viterbi_branch_i32;
VolumeViterbi(alternatives=True).push / alternatives) per frame of a recorded track, beside VolumeViterbi.push / finish and
VolumeSmoother.push / finish on the same volumes in the same run.

    python tools/bench_volume_path_alternatives.py [--frames 8 32] [--grid 64] [--radius 10] [--floor 1e-3] [--batch 8]
                                                   [--separation 2] [--warmup 3] [--reps 20] [--out result.json]

The track is that of tools/bench_volume_viterbi.py (15 rows of G^3 voxels, walking bumps), pushed in batches of --batch.  HIP events,
median of --reps after --warmup; every repetition is a whole track.  ``push`` / ``finish``: the class without the kept scores;
``push_keep`` / ``alternatives``: with them (alternatives() is finish() plus the backward pass, the host's margins and anchors, the two
branch walks and the second refinement).  ``back`` and ``branch``: the _lib-level backward pass (the successor pointers written over
the scores) and the two branch walks alone, over the same chunks.  ``smoother_push`` / ``smoother_finish``: VolumeSmoother.  TB/s is
the byte model of csrc/volume_viterbi.hip: 28 B per frame, row and voxel for the forward pass, + 4 for the kept scores, + 4 for the
copy of the volumes; 36 B for the backward pass.  Prints one JSON line per T.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_volume_viterbi import JOINTS, SIDE, events, timed_pair, walking_bumps  # noqa: E402
from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.volume_smoother import VolumeSmoother  # noqa: E402
from sceneego_amd.volume_viterbi import VolumeViterbi, path_margins, runner_up_anchors  # noqa: E402

FORWARD_BYTES, BACKWARD_BYTES = 28, 36


def measure(T, G, radius, floor, batch, separation, warmup, reps, dev):
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols = walking_bumps(T, G, coord, dev, seed=T)
    kw = {"sigma": radius * (SIDE / G) / 3.0, "radius": radius, "floor": floor}
    cuts = [(i, min(i + batch, T)) for i in range(0, T, batch)]
    r = {"frames": T, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor, "push_batch": batch,
         "separation": separation, "stored_mb": round(3 * T * JOINTS * N * 4 / 1e6, 1)}
    last = {}

    def track(obj, end):
        def run():
            obj.reset()
            e = events(3)
            e[0].record()
            for a, b in cuts:
                obj.push(vols[a:b])
            e[1].record()
            last["result"] = end(obj)
            e[2].record()
            e[2].synchronize()
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
        return run

    def put(name, stats, model_bytes=None):
        ms, lo, hi = stats
        r[f"{name}_ms_per_frame"], r[f"{name}_ms_range"] = round(ms / T, 4), [round(lo / T, 4), round(hi / T, 4)]
        if model_bytes is not None:
            r[f"{name}_tbps"] = round(T * JOINTS * N * model_bytes / 1e9 / ms, 3)               # GB / ms = TB / s

    plain = VolumeViterbi(coord, G, SIDE, **kw)
    a, b = timed_pair(track(plain, lambda v: v.finish()), warmup, reps)
    put("push", a, FORWARD_BYTES + 4)
    put("finish", b)
    path = {k: v.clone() for k, v in last["result"].items()}
    keep = VolumeViterbi(coord, G, SIDE, alternatives=True, **kw)
    a, b = timed_pair(track(keep, lambda v: v.alternatives(separation=separation)), warmup, reps)
    put("push_keep", a, FORWARD_BYTES + 8)
    put("alternatives", b)
    alt = last["result"]
    r["same_path"] = bool(torch.equal(alt["index"], path["index"]) and torch.equal(alt["joints"], path["joints"]))
    fin = torch.isfinite(alt["margin"])
    r["mean_margin"] = round(float(alt["margin"][fin].mean()), 3) if fin.any() else None
    r["margin_below_ln2_share"] = round(float((alt["margin"] < np.log(2.0)).float().mean()), 4)
    smoother = VolumeSmoother(coord, G, SIDE, **kw)
    a, b = timed_pair(track(smoother, lambda s: s.finish()), warmup, reps)
    put("smoother_push", a)
    put("smoother_finish", b)
    # the backward pass and the branch walks alone, at the _lib level, over the same chunks
    rows, flat = JOINTS, vols.reshape(T, JOINTS, N)
    taps = torch.from_numpy(plain.filter.taps).to(dev)
    state = torch.empty((rows, N), device=dev)
    peak_state, best_state = torch.empty(rows, device=dev, dtype=torch.int32), torch.empty(rows, device=dev)
    back = torch.empty((T, rows, N), device=dev, dtype=torch.int32)
    scores = torch.empty((T, rows, N), device=dev)
    peak, exponent, restarted = (torch.empty((T, rows), device=dev, dtype=torch.int32) for _ in range(3))
    best = torch.empty((T, rows), device=dev)
    ones = torch.ones(rows, device=dev, dtype=torch.int32)
    for a0, b0 in cuts:
        _lib.volume_viterbi_keep(flat[a0:b0], taps, state, peak_state, best_state, back[a0:b0], peak[a0:b0], best[a0:b0],
                                 exponent[a0:b0], restarted[a0:b0], scores[a0:b0], b0 - a0, rows, N, G, radius, floor,
                                 have_prior=None if a0 == 0 else ones)
    index = path["index"]
    carry = {"r": torch.empty((rows, N), device=dev), "link": torch.empty(rows, device=dev, dtype=torch.int32),
             "best": torch.empty(rows, device=dev), "complete": torch.empty(rows, device=dev, dtype=torch.int32)}
    out = {name: torch.empty((T, rows), device=dev, dtype=dtype) for name, dtype in _lib.BACK_OUTPUTS}
    work = torch.empty_like(scores)
    cursor = torch.empty(rows, device=dev, dtype=torch.int32)
    ru_index, ru_jumped = (torch.empty((T, rows), device=dev, dtype=torch.int32) for _ in range(2))
    anchors = {}

    def back_and_branch():
        work.copy_(scores)                   # the pointers overwrite the scores: a fresh copy per repetition, outside the timing
        succ = work.view(torch.int32)
        e = events(3)
        e[0].record()
        for a0, b0 in reversed(cuts):
            _lib.volume_viterbi_back(flat[a0:b0], work[a0:b0], exponent[a0:b0], restarted[a0:b0], index[a0:b0], taps, carry,
                                     {k: v[a0:b0] for k, v in out.items()}, b0 - a0, rows, N, G, radius, floor, separation,
                                     int(b0 != T), succ=succ[a0:b0])
        e[1].record()
        if "dev" not in anchors:             # the host's part once: it is in the `alternatives` figure
            margin = path_margins(out["path_value"].cpu().numpy(), out["alt_value"].cpu().numpy(), out["alt_index"].cpu().numpy(),
                                  index.cpu().numpy())
            anchors["dev"] = torch.from_numpy(runner_up_anchors(margin, out["alt_index"].cpu().numpy(), restarted.cpu().numpy())[0]).to(dev)
            e[1].record()
        for direction, order in ((-1, list(reversed(cuts))), (1, cuts)):
            for n, (a0, b0) in enumerate(order):
                _lib.volume_viterbi_branch(back[a0:b0], succ[a0:b0], restarted[a0:b0], anchors["dev"][a0:b0], cursor, ru_index[a0:b0],
                                           ru_jumped[a0:b0], b0 - a0, rows, N, direction, int(n > 0))
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    a, b = timed_pair(back_and_branch, warmup, reps)
    put("back", a, BACKWARD_BYTES)
    put("branch", b)
    r["same_runner_up"] = bool(torch.equal(ru_index, alt["runner_up_index"]))
    r["push_keep_over_push"] = round(r["push_keep_ms_per_frame"] / r["push_ms_per_frame"], 3)
    r["back_over_push"] = round(r["back_ms_per_frame"] / r["push_ms_per_frame"], 3)
    r["byte_model_ratios"] = {"push_keep_over_push": round((FORWARD_BYTES + 8) / (FORWARD_BYTES + 4), 3),
                              "back_over_push": round(BACKWARD_BYTES / (FORWARD_BYTES + 4), 3)}
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=8, help="frames per push")
    ap.add_argument("--separation", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_path_alternatives.py needs an MI355X (HIP device)")
    if args.reps < 1 or args.warmup < 0:
        raise SystemExit("--reps must be at least 1 and --warmup at least 0")
    dev = torch.device("cuda")
    results = []
    for T in args.frames:
        r = measure(T, args.grid, args.radius, args.floor, args.batch, args.separation, args.warmup, args.reps, dev)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
