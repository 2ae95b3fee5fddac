#!/usr/bin/env python3
"""Cost of the most probable joint trajectory (se_volume_viterbi_f32; VolumeViterbi.push / finish) per frame of a recorded track,
beside VolumeFilter.step on the same volumes, beside track.select_modes end to end on the same frames and beside the same recursion
written in plain torch on the same device.

    python tools/bench_volume_viterbi.py [--frames 8 32] [--grid 64] [--radius 10] [--floor 1e-3] [--batch 8] [--warmup 3]
                                         [--reps 20] [--out result.json]

The track is T frames of 15 rows of G^3 voxels (Gaussian bumps that take a random walk, softmaxed on the device), pushed in batches of
--batch.  HIP events around the T / batch pushes and around finish(), median of --reps after --warmup; every repetition is a whole
track (reset, pushes, finish), so the first frame of every track is a restart as in use.  finish() includes its host part (the segment
scores are summed in float64 on the host).  ``filter_ms`` is VolumeFilter.step over the same batches.  ``select_modes_ms`` is wall
time, end to end: joint_modes (k = 4) on the device per batch, its results to the host and track.select_modes over the T frames.
``torch_ms`` is the forward recursion of the definition in plain torch on the device: per axis a loop over the 2 R + 1 taps of a
shifted product and torch.maximum (with the winning offset), the composition of the offsets, step or jump, the product, the maximum
and the rescaling; its back-pointers are compared with the kernel's (the fraction that differs is printed: torch does not promise one
rounding per operation).  TB/s is the kernel's byte model (csrc/volume_viterbi.hip: 28 B per frame, row and voxel for the forward
pass, plus the 4 B copy of the volumes that push keeps for the refinement).  Prints one JSON line per T.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, op, track  # noqa: E402
from sceneego_amd.volume_filter import VolumeFilter  # noqa: E402
from sceneego_amd.volume_viterbi import VolumeViterbi  # noqa: E402

JOINTS = 15
SIDE = 2.0
MODEL_BYTES = 28            # per frame, row and voxel (csrc/volume_viterbi.hip: BYTE MODEL); + 4 for the stored copy of the volumes


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


def torch_stage(v, taps, R, axis):
    """(best, offset) of the stage along ``axis`` of ``v`` [J, G, G, G]: a loop of shifted products and torch.maximum."""
    G = v.shape[axis]
    best = torch.zeros_like(v)
    off = torch.zeros(v.shape, device=v.device, dtype=torch.int8)
    for d in range(-R, R + 1):
        dst = best.narrow(axis, max(0, -d), G - abs(d))
        cand = v.narrow(axis, max(0, d), G - abs(d)) * taps[d + R]
        take = cand > dst
        off.narrow(axis, max(0, -d), G - abs(d)).masked_fill_(take, d)
        torch.maximum(dst, cand, out=dst)
    return best, off


def torch_forward(vols, taps, floor):
    """The forward recursion in plain torch, float32: the back-pointers [T, J, N] (int32) and the peaks [T, J]."""
    T, J, G = vols.shape[:3]
    N = G ** 3
    R = (taps.numel() - 1) // 2
    dev = vols.device
    keep = torch.tensor(1.0, device=dev) - torch.tensor(floor, device=dev)
    uniform = torch.tensor(floor, device=dev) / float(N)
    ar = torch.arange(G, device=dev)
    ii, jj, kk = ar.view(1, G, 1, 1), ar.view(1, 1, G, 1), ar.view(1, 1, 1, G)
    rr = torch.arange(J, device=dev).view(J, 1, 1, 1)
    back = torch.full((T, J, N), -1, device=dev, dtype=torch.int32)
    peaks = torch.empty((T, J), device=dev, dtype=torch.int64)
    s = vols[0].reshape(J, N)
    M, peak = s.max(dim=1)
    e = torch.frexp(M)[1] - 1
    s, best = torch.ldexp(s, -e[:, None]), torch.ldexp(M, -e)
    peaks[0] = peak
    for t in range(1, T):
        e1, dk = torch_stage(s.view(J, G, G, G), taps, R, 3)
        e2, dj = torch_stage(e1, taps, R, 2)
        e3, di = torch_stage(e2, taps, R, 1)
        ip = (ii + di).expand(J, G, G, G)
        jp = jj + dj[rr, ip, jj.expand_as(ip), kk.expand_as(ip)]
        kp = kk + dk[rr, ip, jp, kk.expand_as(ip)]
        y = ((ip * G + jp) * G + kp).reshape(J, N)
        step = keep * e3.reshape(J, N)
        jump = (uniform * best)[:, None]
        take = jump > step
        back[t] = torch.where(take, (peak | _lib.VITERBI_JUMP)[:, None], y).to(torch.int32)
        a = vols[t].reshape(J, N) * torch.where(take, jump, step)
        M, peak = a.max(dim=1)
        e = torch.frexp(M)[1] - 1
        s, best = torch.ldexp(a, -e[:, None]), torch.ldexp(M, -e)
        peaks[t] = peak
    return back, peaks


def measure(T, G, radius, floor, batch, warmup, reps, dev):
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(dev)
    coord_volumes = coord.view(1, G, G, G, 3)
    vols = walking_bumps(T, G, coord, dev, seed=T)
    h = SIDE / G
    kw = {"sigma": radius * h / 3.0, "radius": radius, "floor": floor}
    cuts = [(i, min(i + batch, T)) for i in range(0, T, batch)]
    r = {"frames": T, "grid": G, "rows_per_frame": JOINTS, "radius": radius, "floor": floor, "push_batch": batch,
         "stored_mb": round(2 * T * JOINTS * N * 4 / 1e6, 1), "model_bytes_per_voxel": MODEL_BYTES}
    filt = VolumeFilter(coord, G, SIDE, **kw)
    last = {}

    def filter_track():
        filt.reset()
        e = events(2)
        e[0].record()
        for a, b in cuts:
            filt.step(vols[a:b])
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]), 0.0

    def path_track(vv):
        def run():
            vv.reset()
            e = events(3)
            e[0].record()
            for a, b in cuts:
                vv.push(vols[a:b])
            e[1].record()
            last["path"] = vv.finish()
            e[2].record()
            e[2].synchronize()
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
        return run

    def modes_track():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = []
        for a, b in cuts:
            frames.extend(op.joint_modes_to_numpy(op.joint_modes(vols[a:b], coord_volumes, k=4, radius=2)))
        fallback = np.zeros((T, JOINTS, 3), dtype=np.float32)
        track.select_modes(frames, sigma=kw["sigma"] if kw["sigma"] > 0 else 0.1, fallback=fallback)
        return (time.perf_counter() - t0) * 1e3, 0.0

    (f_ms, f_lo, f_hi), _ = timed_pair(filter_track, warmup, reps)
    r["filter_ms_per_frame"], r["filter_ms_range"] = round(f_ms / T, 4), [round(f_lo / T, 4), round(f_hi / T, 4)]
    for name, refine in (("", 1), ("_refine0", 0)):
        vv = VolumeViterbi(coord, G, SIDE, refine=refine, **kw)
        (p_ms, p_lo, p_hi), (b_ms, b_lo, b_hi) = timed_pair(path_track(vv), warmup, reps)
        per = MODEL_BYTES + (4 if refine else 0)
        r[f"push{name}_ms_per_frame"], r[f"push{name}_ms_range"] = round(p_ms / T, 4), [round(p_lo / T, 4), round(p_hi / T, 4)]
        r[f"push{name}_tbps"] = round(T * JOINTS * N * per / 1e9 / p_ms, 3)               # GB / ms = TB / s
        r[f"finish{name}_ms_per_frame"], r[f"finish{name}_ms_range"] = round(b_ms / T, 4), [round(b_lo / T, 4), round(b_hi / T, 4)]
    (m_ms, m_lo, m_hi), _ = timed_pair(modes_track, warmup, max(3, reps // 4))
    r["select_modes_ms_per_frame"], r["select_modes_ms_range"] = round(m_ms / T, 4), [round(m_lo / T, 4), round(m_hi / T, 4)]
    # the kernel's back-pointers for the comparison with torch: one call over the whole track
    state = torch.empty((JOINTS, N), device=dev)
    small_i = [torch.empty((T, JOINTS), device=dev, dtype=torch.int32) for _ in range(3)]
    best = torch.empty((T, JOINTS), device=dev)
    back = torch.empty((T, JOINTS, N), device=dev, dtype=torch.int32)
    taps = torch.from_numpy(filt.taps).to(dev)
    _lib.volume_viterbi(vols.reshape(T, JOINTS, N), taps, state, torch.empty(JOINTS, device=dev, dtype=torch.int32),
                        torch.empty(JOINTS, device=dev), back, small_i[0], best, small_i[1], small_i[2], T, JOINTS, N, G, radius, floor)

    def torch_track():
        e = events(2)
        e[0].record()
        last["torch"] = torch_forward(vols, taps, float(np.float32(floor)))
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]), 0.0

    (t_ms, t_lo, t_hi), _ = timed_pair(torch_track, 1, max(3, reps // 4))
    r["torch_ms_per_frame"], r["torch_ms_range"] = round(t_ms / T, 4), [round(t_lo / T, 4), round(t_hi / T, 4)]
    r["torch_over_push"] = round(r["torch_ms_per_frame"] / r["push_ms_per_frame"], 2)
    r["torch_back_pointers_that_differ"] = float((last["torch"][0][1:] != back[1:]).float().mean())
    r["torch_peaks_equal"] = bool(torch.equal(last["torch"][1].to(torch.int32), small_i[0]))
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
        raise SystemExit("bench_volume_viterbi.py needs an MI355X (HIP device)")
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
