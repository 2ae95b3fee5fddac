#!/usr/bin/env python3
"""Cost of one E-step of the skeleton-model fit (se_skeleton_edge_stats_f32) per frame beside SkeletonPrior.couple on the same
volumes, and of one moments launch (se_shell_moments_f32) beside one correlation launch (se_shell_correlate_f32) over the same rows:
B frames x 15 joints of G^3 voxels.

    python tools/bench_skeleton_fit.py [--batches 1 8 32] [--grid 64] [--tau 0.03] [--floor 1e-3] [--warmup 3] [--reps 20]
                                       [--out result.json]

HIP events around one call, median of --reps after --warmup, the same call back to back.  The volumes are the Gaussian bumps of
tools/bench_skeleton_prior.py (--no_forward there), the bone lengths its 14 values from 0.15 to 0.45 m, so at 64^3 and tau 0.03 the
taps reach R = 18 voxels.  ``moments`` / ``correlate``: one launch over the 14 x B rows of joints 1..14, every edge with its own shell
(the small launches before and behind it included: the run table, for the moments also the interleaving of the three blocks and the
fold of the workgroup records).  By count a moments launch executes three times the fused multiply-adds of the correlation on the
same LDS reads (tools/bench_skeleton_prior.py: kernel_counts) and one 16-byte scalar load per tap where the correlation has one of 4
bytes; an E-step is 28 correlations and 14 moment rows per frame.  ``fit_ms_per_iteration``: a whole ``SkeletonModelFit.fit(
iterations=1)`` by the host's clock: two E-steps, the copies to the host and the float64 M-step.  Prints one JSON line per batch size.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_skeleton_prior import BONES, JOINTS, PEAK_TFMA, bump_volumes, kernel_counts, timed  # noqa: E402
from sceneego_amd import _lib, op  # noqa: E402
from sceneego_amd.skeleton_fit import SkeletonModelFit, cut_support, support_taps  # noqa: E402
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior  # noqa: E402

SIDE = 2.0


def measure(B, G, tau, floor, warmup, reps, dev):
    N, J = G ** 3, JOINTS
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    vols, _ = bump_volumes(B, G, coord, dev, seed=B)
    sp = SkeletonPrior(coord, G, SIDE, BONES, tau=tau, floor=floor)
    R = sp.radius
    blocks = support_taps(cut_support(sp.bone_lengths, tau, SIDE / G, R), sp.bone_lengths, tau)
    w = [torch.from_numpy(b).to(dev) for b in blocks]
    flat = vols.reshape(B, J, N)
    stats = torch.empty((B, J, _lib.EDGE_STATS_SLOTS), device=dev)
    norms = torch.empty((B, J, 3), device=dev)
    valid = torch.empty((B,), device=dev, dtype=torch.int32)
    ws_e = torch.empty(_lib.skeleton_edge_stats_scratch_bytes(B, J, G, R), device=dev, dtype=torch.uint8)
    edge_rows = (J - 1) * B
    a = vols[:, 1:].reshape(edge_rows, N).contiguous()
    e = a.flip(0).contiguous()
    tap_row = torch.arange(1, J, device=dev, dtype=torch.int32).repeat(B)
    s = torch.ones(edge_rows, device=dev)
    corr_out = torch.empty_like(a)
    mom_out = torch.empty((edge_rows, 3), device=dev)
    ws_c = torch.empty(_lib.shell_correlate_scratch_bytes(J, R), device=dev, dtype=torch.uint8)
    ws_m = torch.empty(_lib.shell_moments_scratch_bytes(edge_rows, J, G, R), device=dev, dtype=torch.uint8)

    def couple():
        sp.couple(vols)

    def e_step():
        _lib.skeleton_edge_stats(flat, w[0], w[1], w[2], KINEMATIC_PARENTS, stats, norms, valid, B, N, G, R, floor, scratch=ws_e)

    def correlate():
        _lib.shell_correlate(a, w[0], tap_row, s, corr_out, edge_rows, G, R, 1.0 - floor, floor / N, scratch=ws_c)

    def moments():
        _lib.shell_moments(e, a, w[0], w[1], w[2], tap_row, mom_out, edge_rows, G, R, scratch=ws_m)

    r = {"batch": B, "grid": G, "joints": J, "tau": tau, "floor": floor, "radius": R, "volume_mb": round(B * J * N * 4 / 1e6, 1),
         "scratch_mb": round(ws_e.numel() / 1e6, 1)}
    for name, fn in (("couple", couple), ("e_step", e_step), ("correlate", correlate), ("moments", moments)):
        med, lo, hi = timed(fn, warmup, reps)
        r[f"{name}_ms"], r[f"{name}_ms_range"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    r["valid_frames"] = int(valid.sum())
    r["couple_ms_per_frame"], r["e_step_ms_per_frame"] = round(r["couple_ms"] / B, 4), round(r["e_step_ms"] / B, 4)
    r["e_step_over_couple"] = round(r["e_step_ms"] / r["couple_ms"], 3)
    r["moments_over_correlate"] = round(r["moments_ms"] / r["correlate_ms"], 3)
    counts = [kernel_counts(blocks[0][j], G, R) for j in range(1, J)]
    fma, reads = sum(c[0] for c in counts), sum(c[1] for c in counts)             # one frame's 14 edges, one block
    r["correlate_gfma"], r["moments_gfma"] = round(B * fma / 1e9, 3), round(3 * B * fma / 1e9, 3)
    r["correlate_tfma_per_s"] = round(B * fma / 1e9 / r["correlate_ms"], 3)       # G FMA / ms = T FMA / s
    r["moments_tfma_per_s"] = round(3 * B * fma / 1e9 / r["moments_ms"], 3)
    r["moments_share_of_fp32_peak"] = round(r["moments_tfma_per_s"] / PEAK_TFMA, 4)
    r["lds_reads_per_fma"] = {"correlate": round(reads / fma, 4), "moments": round(reads / (3 * fma), 4)}
    r["lds_gread_per_s"] = {"correlate": round(B * reads / 1e6 / r["correlate_ms"], 1), "moments": round(B * reads / 1e6 / r["moments_ms"], 1)}

    fit = SkeletonModelFit(G, SIDE, BONES, tau=tau, floor=floor)
    fit.push(vols)
    host = []
    for i in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fit.fit(iterations=1)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t) * 1e3)
    r["fit_ms_per_iteration"] = round(min(host), 1)
    r["log_likelihood"] = res["log_likelihood"]
    r["fitted_tau"], r["fitted_floor"] = res["tau"], res["floor"]
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.03)
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skeleton_fit.py needs an MI355X (HIP device)")
    if args.reps < 1 or args.warmup < 0:
        raise SystemExit("--reps must be at least 1 and --warmup at least 0")
    dev = torch.device("cuda")
    results = []
    for B in args.batches:
        r = measure(B, args.grid, args.tau, args.floor, args.warmup, args.reps, dev)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
